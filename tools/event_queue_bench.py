"""Timing of event retention across chunks: `EventQueue.push` / `push_dat` / `frames` (sast_amd/events.py) on a recording that arrives in
chunks of a quarter window, beside one `EventStreams` call on the same events in one buffer, in the same process.

Gen4 sensor (720 x 1280, downsampled by 2), 50 ms windows, --windows windows of --events events per recording, S in --streams.  One
session pushes the recording chunk by chunk and asks for window k as soon as the first chunk of window k + 1 is in (the last window
after the last chunk), as a camera loop does; the queue holds 3.5 windows' events per row (the sizing rule 2 R + P: R = a window + a chunk live
after a `frames` call, P = a window's four chunks pushed before the next).  Every call of a session is bracketed by device events; the table gives, over --rounds sessions, the median time of
  push       one chunk as int16 x / y / p and int32 t columns (10 bytes per event)
  push_dat   the same chunk as packed Event2D records (8 bytes per event), in a session of its own
  frames     one `frames` call (T = 1: window search, 4 frame launches, retirement)
  streams    one EventStreams call on the whole recording, T = --windows steps, divided by T
The chunks are already in device memory: the copy over PCIe, where the packed form saves 2 of 10 bytes, is not part of any figure.
The frames of the three forms are checked equal.  The inputs are synthetic (tools/event_streams_bench.py: uniform pixels, a few hot
pixels, one timestamp in 16 pulled back); no real sensor's event rate has been measured here.

  python tools/event_queue_bench.py [--streams 1,8] [--windows 4] [--events 500000] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from event_streams_bench import H, W, WINDOW_US, synthetic, timed  # noqa: E402

CHUNKS_PER_WINDOW = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8")
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--events", type=int, default=500000, help="events per recording and window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd import _lib
    from sast_amd.events import EventQueue, EventStreams
    if not torch.cuda.is_available():
        raise SystemExit("tools/event_queue_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _lib.lib()
    props = torch.cuda.get_device_properties(0)
    T, E = a.windows, a.events
    chunk = E // CHUNKS_PER_WINDOW
    lines = [f"# tools/event_queue_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; Gen4 720 x 1280 downsampled by 2, 50 ms windows, {T} windows of {E} synthetic events per recording, "
             f"chunks of {chunk} events per row, queue capacity {7 * E // 2} per row; bins 10, cutoff 10, fastmode; median (min .. max) ms per call "
             f"over {a.rounds} sessions",
             "# push: int16 x / y / p + int32 t columns;  push_dat: packed Event2D records;  frames: one EventQueue.frames call (T = 1);  "
             "streams: one EventStreams call on the whole recording / its T windows;  launches: library kernel launches per push, frames",
             f"{'S':>3}{'chunk ev':>10}  {'push ms':<26}{'push_dat ms':<26}{'frames ms':<26}{'streams ms / window':<26}{'launches':>9}"]
    kw = dict(height=H, width=W, bins=10, count_cutoff=10, duration_us=WINDOW_US, downsample_by_2=True)
    for S in (int(v) for v in a.streams.split(",")):
        cols, ends = synthetic(S, T, E, seed=100 * S + T)
        n = T * E
        whole = [c.to(dev) for c in cols]
        ends = ends.to(dev)
        counts_whole = torch.full((S,), n, dtype=torch.int64, device=dev)
        x, y, p, t = cols
        rec = torch.stack([t, x | (y << 14) | (p << 28)], -1).to(torch.int32)                   # t < 2^31 here
        cuts = [(lo, min(lo + chunk, n)) for lo in range(0, n, chunk)]
        col_chunks = [[c[:, lo:hi].to(d).contiguous().to(dev) for c, d in zip(cols, (torch.int16,) * 3 + (torch.int32,))] for lo, hi in cuts]
        rec_chunks = [rec[:, lo:hi].contiguous().to(dev) for lo, hi in cuts]
        counts = [torch.full((S,), hi - lo, dtype=torch.int64, device=dev) for lo, hi in cuts]
        assert len(cuts) == T * CHUNKS_PER_WINDOW, "--events must be a multiple of 4"
        q = EventQueue(S, 7 * E // 2, window_capacity=2 * E, **kw)
        es = EventStreams(S, window_capacity=2 * E, **kw)

        def session(packed, marks=None):
            q.reset()
            out = []
            for i in range(len(cuts)):
                m0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                m0[0].record()
                if packed:
                    q.push_dat(rec_chunks[i], counts[i])
                else:
                    q.push(*col_chunks[i], counts[i])
                m0[1].record()
                if marks is not None:
                    marks["push"].append(m0)
                # window k is asked for after the chunk that starts window k + 1 (events later than its end have then arrived), the
                # last one after the last chunk
                ks = [i // CHUNKS_PER_WINDOW - 1] if i and i % CHUNKS_PER_WINDOW == 0 else []
                if i == len(cuts) - 1:
                    ks.append(T - 1)
                for k in ks:
                    m1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    m1[0].record()
                    out.append(q.frames(ends[k]))
                    m1[1].record()
                    if marks is not None:
                        marks["frames"].append(m1)
            return torch.stack(out)

        def streams_call():
            es.reset()
            return es(*whole, counts_whole, ends)

        es(*whole, counts_whole, ends)                               # warm-up: the carry, workspaces, code objects
        want = streams_call()
        for packed in (False, True):
            got = session(packed)
            assert torch.equal(got, want), (S, packed)               # chunked == whole, for both input forms
            assert q.errors() == (0, 0, 0, 0), q.errors()
        n0 = lib.sast_launch_count()
        q.push(*col_chunks[0], counts[0])
        n1 = lib.sast_launch_count()
        q.frames(ends[0])
        n2 = lib.sast_launch_count()
        res = {"push": [], "push_dat": [], "frames": [], "streams": []}
        for _ in range(a.rounds):
            for packed in (False, True):
                marks = {"push": [], "frames": []}
                session(packed, marks)
                torch.cuda.synchronize()
                res["push_dat" if packed else "push"].append(statistics.median(u.elapsed_time(v) for u, v in marks["push"]))
                if not packed:
                    res["frames"].append(statistics.median(u.elapsed_time(v) for u, v in marks["frames"]))
            res["streams"].append(timed(streams_call, 3) / T)

        def cell(v):
            return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"

        lines.append(f"{S:>3}{chunk:>10}  {cell(res['push']):<26}{cell(res['push_dat']):<26}{cell(res['frames']):<26}{cell(res['streams']):<26}"
                     f"{f'{n1 - n0}, {n2 - n1}':>9}")
        print(lines[-1], flush=True)
        del q, es, whole, col_chunks, rec_chunks
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
