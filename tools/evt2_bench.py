"""Timing of the raw-sensor-word paths side by side: `EventQueue.push_evt2` of EVT 2.0 and of EVT 2.1 words (sast_amd/events.py,
csrc/k_evt2.hip) beside `push_evt3` of the same events as EVT 3.0 words, `push` of them as pre-decoded columns and `push_dat` of them as
packed Event2D records, in one process.  The yardsticks are the other forms in the same job, not figures of earlier records.

Gen4 sensor (720 x 1280, the queue downsampled by 2), S in --streams, --chunks chunks of --events events per row and session.  The
events are the synthetic ones of tools/evt3_bench.py (groups of one time, row and polarity that are a single pixel or, with probability
--vectors, up to 12 pixels inside 12 columns; times climb by up to --step us per group), and every form is built from the same events:
EVT 2.0 one word per event, EVT 2.1 one word per run of one (t, y, p) with ascending x inside 32 columns (base: the run's first column),
both with an EVT_TIME_HIGH wherever t >> 6 changes.  No real sensor has been measured.  The chunks are already in device memory: the
copy over PCIe is not part of any figure; `B/ev` says what it would move, counted from the streams.  Every push is bracketed by device
events; a figure is the median (min .. max over --rounds sessions of the session's median) time of one push of one chunk, eager and
replayed from a graph captured on the same tensors, after a warm-up session.  The decoders' staging holds the largest chunk's events
(max_events), as a host that knows its sensor's rate would set it.  Before anything is timed the queues are checked to hold the same
events.

The "encode 2.0" / "encode 2.1" rows are the way back, in the same job: `Evt2Encoder` (csrc/k_evt2_enc.hip) on the column chunks of the
push row, one call per chunk, `words` the words it gives per row and chunk (its canonical rule aligns an EVT 2.1 base to 32 columns, so
it gives more words than the stream above, whose base is the run's first column); before it is timed `Evt2Decoder` is checked to give
the columns back from its words.  The "copy" row is a device copy of the same four column tensors, for scale.  The decode rows keep
their host-built words, so they stay comparable with earlier records.

  python tools/evt2_bench.py [--streams 1,8] [--chunks 4] [--events 125000] [--rounds 5] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from evt3_bench import H, W, WINDOW_US, cell, encode_rows, synthetic_chunk  # noqa: E402

TIME_HIGH = 0x8
FORMS = ("push", "push_dat", "push_evt3", "push_evt2 2.0", "push_evt2 2.1")


def _with_time_high(event_words, high, prev_high, shift, payload_shift):
    """the event words (one per entry of `high`, the unwrapped t >> 6 in front of each) with an EVT_TIME_HIGH in front of every word whose
    `high` differs from its predecessor's (`prev_high` for the first) -> the stream"""
    new = np.concatenate([[prev_high], high[:-1]]) != high
    assert (np.diff(np.concatenate([[max(prev_high, 0)], high])) <= 1 << 26).all(), "--step is too large for the TIME_HIGH keep-alive rule"
    at = np.arange(len(high)) + np.cumsum(new)
    out = np.zeros(len(high) + int(new.sum()), event_words.dtype)
    out[at] = event_words
    th = (np.uint64(TIME_HIGH) << np.uint64(shift)) | ((high[new].astype(np.uint64) & np.uint64(0x0FFFFFFF)) << np.uint64(payload_shift))
    out[at[new] - 1] = th.astype(event_words.dtype)
    return out


def evt2_words(x, y, p, t, prev_t):
    """the events as (EVT 2.0 uint32 words, EVT 2.1 uint64 words); prev_t: the last time of the chunk before (-1: the stream starts here)"""
    x, y, p, t = (np.asarray(c, np.int64) for c in (x, y, p, t))
    prev_high = -1 if prev_t < 0 else prev_t >> 6
    ts6 = (t & 63).astype(np.uint64)
    w20 = ((p.astype(np.uint64) << np.uint64(28)) | (ts6 << np.uint64(22)) | (x.astype(np.uint64) << np.uint64(11)) | y.astype(np.uint64))
    words20 = _with_time_high(w20.astype(np.uint32), t >> 6, prev_high, 28, 0)
    # EVT 2.1: a new word where (t, y, p) changes, x does not ascend, or x runs 32 columns past the word's first
    start = np.ones(len(t), bool)
    start[1:] = (np.diff(t) != 0) | (np.diff(y) != 0) | (np.diff(p) != 0) | (np.diff(x) <= 0)
    while True:
        first = np.maximum.accumulate(np.where(start, np.arange(len(t)), 0))
        far = (x - x[first] >= 32) & ~start
        if not far.any():
            break
        start[far & ~np.concatenate([[False], far[:-1]])] = True       # the first such pixel of every run starts a word
    idx = np.flatnonzero(start)
    valid = np.bitwise_or.reduceat(np.uint64(1) << (x - x[first]).astype(np.uint64), idx)
    w21 = ((p[idx].astype(np.uint64) << np.uint64(60)) | (ts6[idx] << np.uint64(54)) | (x[idx].astype(np.uint64) << np.uint64(43))
           | (y[idx].astype(np.uint64) << np.uint64(32)) | valid)
    words21 = _with_time_high(w21, t[idx] >> 6, prev_high, 60, 32)
    return words20, words21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8")
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--events", type=int, default=125000, help="events per row and chunk (about)")
    ap.add_argument("--vectors", type=float, default=0.3, help="share of groups that are up to 12 pixels of one row (EVT 3.0: VECT_BASE_X + VECT_12)")
    ap.add_argument("--step", type=int, default=2, help="largest time step between groups, us")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd import _lib
    from sast_amd.events import EventQueue, Evt2Decoder, Evt2Encoder
    if not torch.cuda.is_available():
        raise SystemExit("tools/evt2_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _lib.lib()
    props = torch.cuda.get_device_properties(0)
    lines = [f"# tools/evt2_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; Gen4 720 x 1280, the synthetic events of tools/evt3_bench.py ({a.vectors:.0%} of the groups up to 12 pixels "
             f"of one row, time steps up to {a.step} us) in five forms, {a.chunks} chunks of about {a.events} events per row and session; "
             f"median (min .. max) ms per push of one chunk over {a.rounds} sessions after a warm-up session; chunks already in device memory",
             "# push: int16 x / y / p + int32 t columns;  push_dat: packed Event2D records;  push_evt3 / push_evt2 2.0 / push_evt2 2.1: the raw "
             "16- / 32- / 64-bit words, decoded on the device;  B/ev: bytes in per event, counted from the streams;  launches: library kernel "
             "launches per push",
             "# encode 2.0 / encode 2.1: Evt2Encoder on the columns of the push row, ms per call, `words` the words it gives per row and chunk;  "
             "copy: a device copy of the same four column tensors, for scale (no library launch)",
             f"{'S':>3}{'form':>15}{'ev/chunk':>10}{'words':>9}{'B/ev':>7}  {'eager ms':<26}{'replayed ms':<26}{'launches':>9}"]
    kw = dict(height=H, width=W, bins=10, count_cutoff=10, duration_us=WINDOW_US, downsample_by_2=True)
    word_np = {"push_evt3": np.uint16, "push_evt2 2.0": np.uint32, "push_evt2 2.1": np.uint64}
    word_view = {np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}
    for S in (int(v) for v in a.streams.split(",")):
        rng = np.random.RandomState(100 + S)
        rows = []                                                    # rows[s][k]: the chunk's events and its words per word form
        for s in range(S):
            t0, prev_t, parts = 1000 * s, -1, []
            for k in range(a.chunks):
                w3, x, y, p, t, t0 = synthetic_chunk(rng, a.events, a.vectors, a.step, t0, k == 0)
                w20, w21 = evt2_words(x, y, p, t, prev_t)
                prev_t = int(t[-1])
                parts.append({"x": x, "y": y, "p": p, "t": t, "push_evt3": w3, "push_evt2 2.0": w20, "push_evt2 2.1": w21})
            rows.append(parts)
        ev_cap = max(len(part["x"]) for parts in rows for part in parts)
        assert max(int(part["t"][-1]) for parts in rows for part in parts) < 2 ** 31
        total = max(sum(len(part["x"]) for part in parts) for parts in rows)
        n_events = sum(len(part["x"]) for parts in rows for part in parts) / (S * a.chunks)
        n_words = {form: sum(len(part[form]) for parts in rows for part in parts) / (S * a.chunks) for form in word_np}

        def stacked(key, cap, dtype, k):
            buf = np.zeros((S, cap), dtype)
            for s in range(S):
                buf[s, :len(rows[s][k][key])] = rows[s][k][key]
            return torch.from_numpy(buf.view(word_view[dtype]) if dtype in word_view else buf).to(dev)

        chunks = {form: [] for form in FORMS}
        for k in range(a.chunks):
            x, y, p = (stacked(key, ev_cap, np.int16, k) for key in "xyp")
            t = stacked("t", ev_cap, np.int32, k)
            n_ev = torch.tensor([len(rows[s][k]["x"]) for s in range(S)], dtype=torch.int64, device=dev)
            rec = torch.stack([t, x.to(torch.int32) | (y.to(torch.int32) << 14) | (p.to(torch.int32) << 28)], -1).contiguous()
            chunks["push"].append(([x, y, p, t], n_ev))
            chunks["push_dat"].append(([rec], n_ev))
            for form, dtype in word_np.items():
                cap = (max(len(rows[s][kk][form]) for s in range(S) for kk in range(a.chunks)) + 7) // 8 * 8
                chunks[form].append(([stacked(form, cap, dtype, k)],
                                     torch.tensor([len(rows[s][k][form]) for s in range(S)], dtype=torch.int64, device=dev)))
        queues = {form: EventQueue(S, total + 8, **kw) for form in FORMS}
        calls = {"push": lambda q, ts, n: q.push(*ts, n), "push_dat": lambda q, ts, n: q.push_dat(*ts, n),
                 "push_evt3": lambda q, ts, n: q.push_evt3(*ts, n, max_events=ev_cap),
                 "push_evt2 2.0": lambda q, ts, n: q.push_evt2(*ts, n, max_events=ev_cap, version="2.0"),
                 "push_evt2 2.1": lambda q, ts, n: q.push_evt2(*ts, n, max_events=ev_cap, version="2.1")}
        # the five forms hold the same events
        for form, q in queues.items():
            for ts, n in chunks[form]:
                calls[form](q, ts, n)
        ref = queues["push"]
        for form, q in queues.items():
            assert torch.equal(q.count, ref.count) and q.errors() == (0, 0, 0, 0), (form, q.errors())
            for name in ("x", "y", "p", "t"):
                assert torch.equal(getattr(q, name), getattr(ref, name)), (form, name)
            assert q.evt3_errors() == (0, 0, 0) and q.evt2_errors() == (0, 0, 0), (form, q.evt3_errors(), q.evt2_errors())
        bytes_in = {"push": 10.0, "push_dat": 8.0, "push_evt3": 2.0 * n_words["push_evt3"] / n_events,
                    "push_evt2 2.0": 4.0 * n_words["push_evt2 2.0"] / n_events, "push_evt2 2.1": 8.0 * n_words["push_evt2 2.1"] / n_events}
        for form, q in queues.items():
            static, static_n = [t.clone() for t in chunks[form][0][0]], chunks[form][0][1].clone()
            q.reset()
            before = lib.sast_launch_count()
            calls[form](q, static, static_n)
            launches = lib.sast_launch_count() - before
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                calls[form](q, static, static_n)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                calls[form](q, static, static_n)
            res = {"eager": [], "replayed": []}
            for mode in ("eager", "replayed"):
                for _ in range(a.rounds + 1):                            # the first session warms up
                    q.reset()
                    marks = []
                    for ts, n in chunks[form]:
                        for dst, src in zip(static + [static_n], ts + [n]):
                            dst.copy_(src)
                        m = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        m[0].record()
                        if mode == "eager":
                            calls[form](q, static, static_n)
                        else:
                            g.replay()
                        m[1].record()
                        marks.append(m)
                    torch.cuda.synchronize()
                    res[mode].append(statistics.median(u.elapsed_time(v) for u, v in marks))
                    assert torch.equal(q.count, ref.count), (form, mode)     # the session stored what the checked one stored
                res[mode] = res[mode][1:]

            lines.append(f"{S:>3}{form:>15}{n_events:>10.0f}{n_words.get(form, 0):>9.0f}{bytes_in[form]:>7.2f}  "
                         f"{cell(res['eager']):<26}{cell(res['replayed']):<26}{launches:>9}")
            print(lines[-1], flush=True)
        extra = []
        for version in ("2.0", "2.1"):
            coders = Evt2Encoder(S, version=version), Evt2Decoder(S, max_events=ev_cap, version=version)
            extra = [r for r in extra if r[0] != "copy"] + encode_rows(S, chunks["push"], a.rounds, lib, coders, f"encode {version}")
        for form, words, eager, replayed, launches in extra:
            b_ev = f"{bytes_in['push']:>7.2f}"
            lines.append(f"{S:>3}{form:>15}{n_events:>10.0f}{words:>9.0f}{b_ev}  {cell(eager):<26}{cell(replayed):<26}{launches:>9}")
            print(lines[-1], flush=True)
        del queues, chunks
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
