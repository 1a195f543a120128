"""Timing of the batched event front end: one `EventStreams` call for S recordings side by side against S `EventFrames` calls, one
per recording, on the same events in the same process (sast_amd/events.py).

Gen4 sensor (720 x 1280, downsampled by 2), 50 ms windows, T steps per recording, S in --streams.  Per (S, T):
  streams   one EventStreams call -> uint8 [T, S, 20, 360, 640]
  loop      S EventFrames calls on the rows of the same buffers (each object with its own carry, bounds and workspace) + torch.stack
            into the same [T, S, ...] layout
Both start a new recording with every timed call (one fill of the carry tensor per object: without it the carry of the previous
call would raise every timestamp of the same events to it and empty the windows).  The two forms are timed in alternating rounds with
device events; the table gives the median round and the spread over the rounds.  `launches` are the library's kernel launches per call
(sast_launch_count(); the fills and the stack are ATen's and not counted).  The frames of both forms are checked equal.
The inputs are synthetic (uniform pixels, a few hot pixels, one timestamp in 16 pulled back); no real sensor's event rate has been
measured here.

  python tools/event_streams_bench.py [--streams 1,4,8] [--steps 1,5] [--events 500000] [--reps 20] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, WINDOW_US = 720, 1280, 50000


def synthetic(S, T, n_window, seed=0):
    """-> x, y, p, t int64 [S, T * n_window] (row s: its own recording on its own clock, unsorted by up to 40 us), ends int64 [T, S]"""
    g = np.random.default_rng(seed)
    n = T * n_window
    x = g.integers(0, W, (S, n), dtype=np.int64)
    y = g.integers(0, H, (S, n), dtype=np.int64)
    p = g.integers(0, 2, (S, n), dtype=np.int64)
    hot = g.random((S, n)) < 0.002
    x[hot] = g.choice([11, 301, 641], hot.sum())
    y[hot] = g.choice([21, 99, 359], hot.sum())
    start = g.integers(0, 10 * WINDOW_US, (S, 1), dtype=np.int64)          # every recording has its own clock
    t = start + np.sort(g.integers(0, T * WINDOW_US, (S, n), dtype=np.int64), axis=1)
    back = g.random((S, n)) < 1 / 16
    t[back] -= g.integers(0, 40, int(back.sum()), dtype=np.int64)
    ends = start.T + np.arange(1, T + 1, dtype=np.int64)[:, None] * WINDOW_US
    return [torch.from_numpy(a) for a in (x, y, p, np.maximum(t, 0))], torch.from_numpy(np.ascontiguousarray(ends))


def timed(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,4,8")
    ap.add_argument("--steps", default="1,5")
    ap.add_argument("--events", type=int, default=500000, help="events per recording and window")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd import _lib
    from sast_amd.events import EventFrames, EventStreams
    if not torch.cuda.is_available():
        raise SystemExit("tools/event_streams_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _lib.lib()
    props = torch.cuda.get_device_properties(0)
    lines = [f"# tools/event_streams_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; Gen4 720 x 1280 downsampled by 2, 50 ms windows, {a.events} synthetic events per recording and window "
             f"(int64 columns), bins 10, cutoff 10, fastmode; {a.rounds} alternating rounds of {a.reps} calls, median (min .. max) ms per call",
             "# streams: one EventStreams call;  loop: S EventFrames calls + torch.stack into [T, S, ...];  launches: library kernel launches "
             "per call;  Mev/s: events of the call over the median time of the streams form"]
    lines.append(f"{'S':>3}{'T':>3}{'events':>11}  {'streams ms':<26}{'loop ms':<26}{'loop/streams':>13}{'launches s':>11}{'launches l':>11}{'Mev/s':>9}")
    kw = dict(height=H, width=W, bins=10, count_cutoff=10, duration_us=WINDOW_US, downsample_by_2=True)
    for T in (int(v) for v in a.steps.split(",")):
        for S in (int(v) for v in a.streams.split(",")):
            cols, ends = synthetic(S, T, a.events, seed=100 * S + T)
            cols = [c.to(dev) for c in cols]
            ends = ends.to(dev)
            cap = cols[0].shape[1]
            counts = torch.full((S,), cap, dtype=torch.int64, device=dev)
            es = EventStreams(S, window_capacity=2 * a.events, **kw)
            efs = [EventFrames(window_capacity=2 * a.events, **kw) for _ in range(S)]
            rows = [[c[s] for c in cols] for s in range(S)]
            row_ends = [ends[:, s].contiguous() for s in range(S)]
            row_n = [counts[s:s + 1] for s in range(S)]
            last = {}

            def streams_call():
                es.t_last.zero_()
                last["streams"] = es(*cols, counts, ends)

            def loop_call():
                outs = []
                for s in range(S):
                    efs[s].t_last.zero_()
                    outs.append(efs[s](*rows[s], row_ends[s], n=row_n[s]))
                last["loop"] = torch.stack(outs, 1)

            es(*cols, counts, ends)                                     # warm-up: workspaces, code objects
            for s in range(S):
                efs[s](*rows[s], row_ends[s], n=row_n[s])
            streams_call()
            loop_call()
            n0 = lib.sast_launch_count()
            streams_call()
            n1 = lib.sast_launch_count()
            loop_call()
            n2 = lib.sast_launch_count()
            t_s, t_l = [], []
            for _ in range(a.rounds):
                t_s.append(timed(streams_call, a.reps))
                t_l.append(timed(loop_call, a.reps))
            assert torch.equal(last["streams"], last["loop"]), (S, T)   # the frames of the last timed calls
            assert all(int(torch.count_nonzero(last["streams"][k, s])) > 0 for k in range(T) for s in range(S)), (S, T)
            assert es.errors() == (0, 0) and all(ef.errors() == (0, 0) for ef in efs)
            ms, ml = statistics.median(t_s), statistics.median(t_l)
            lines.append(f"{S:>3}{T:>3}{S * cap:>11}  {f'{ms:.3f} ({min(t_s):.3f} .. {max(t_s):.3f})':<26}"
                         f"{f'{ml:.3f} ({min(t_l):.3f} .. {max(t_l):.3f})':<26}{ml / ms:>12.2f}x{n1 - n0:>11}{n2 - n1:>11}{S * cap / ms / 1e3:>9.0f}")
            print(lines[-1], flush=True)
            del es, efs, cols, rows, last
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
