"""Timing of the raw-sensor-word path: `EventQueue.push_evt3` (the EVT 3.0 decode on the device, sast_amd/events.py, csrc/k_evt3.hip) beside
`push` of the same events as pre-decoded columns and `push_dat` of the same events as packed Event2D records, in one process.

Gen4 sensor (720 x 1280, the queue downsampled by 2), S in --streams, --chunks chunks of --events events per row and session.  The
streams are synthetic and built as words and events together: groups of one time, row and polarity that are a single event
(EVT_ADDR_X) or, with probability --vectors, a VECT_BASE_X + VECT_12 pair with a random 12-bit mask, with EVT_TIME_HIGH / EVT_TIME_LOW /
EVT_ADDR_Y words in front wherever the value changes; event times climb by up to --step us per group.  No real sensor has been measured.
The chunks are already in device memory: the copy over PCIe is not part of any figure; `bytes / event` says what it would move.
Every push is bracketed by device events; a figure is the median (min .. max over --rounds sessions of the session's median) time
of one push of one chunk, eager and replayed from a graph captured on the same tensors.  The decoder's staging holds the largest
chunk's events (max_events), as a host that knows its sensor's rate would set it.  Before anything is timed the three queues are
checked to hold the same events.  The "encode" row is the way back, in the same job: `Evt3Encoder` (csrc/k_evt3_enc.hip) on the
column chunks of the push row, beside a device copy of the same column tensors ("copy") for scale.

  python tools/evt3_bench.py [--streams 1,8] [--chunks 4] [--events 125000] [--rounds 5] [--out FILE]
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

H, W, WINDOW_US = 720, 1280, 50_000
TIME_HIGH, TIME_LOW, ADDR_Y, ADDR_X, VECT_BASE_X, VECT_12 = 0x8, 0x6, 0x0, 0x2, 0x3, 0x4


def synthetic_chunk(rng, events: int, vectors: float, step: int, t0: int, first: bool):
    """about `events` events as (uint16 words, int64 x, y, p, t, the last time).  Vectorised: per group the words it needs."""
    per_group = 1 + vectors * 5.0                                # a random 12-bit mask has 6 bits set on average
    G = max(int(events / per_group), 1)
    t = t0 + np.cumsum(rng.randint(0, step + 1, size=G))
    y, p = rng.randint(0, H, size=G), rng.randint(0, 2, size=G)
    vec = rng.rand(G) < vectors
    mask = np.where(vec, rng.randint(1, 4096, size=G), 1)
    x0 = np.where(vec, rng.randint(0, W - 12, size=G), rng.randint(0, W, size=G))
    high, low = (t >> 12) & 0xFFF, t & 0xFFF
    prev = lambda a, init: np.concatenate([[init], a[:-1]])      # noqa: E731
    th = prev(t >> 12, -1 if first else t0 >> 12) != (t >> 12)
    tl = prev(low, -1 if first else t0 & 0xFFF) != low
    ay = prev(y, -1) != y                                        # a chunk's first group always names its row
    assert (np.diff(t >> 12) <= 1024).all(), "--step is too large for the TIME_HIGH keep-alive rule"
    n_words = th.astype(np.int64) + tl + ay + np.where(vec, 2, 1)
    at = np.cumsum(n_words) - n_words
    words = np.zeros(int(n_words.sum()), np.uint16)
    for flag, code, v in ((th, TIME_HIGH, high), (tl, TIME_LOW, low), (ay, ADDR_Y, y)):
        words[at[flag]] = (code << 12) | v[flag]
        at = at + flag
    words[at[vec]] = (VECT_BASE_X << 12) | x0[vec] | (p[vec] << 11)
    words[at[vec] + 1] = (VECT_12 << 12) | mask[vec]
    words[at[~vec]] = (ADDR_X << 12) | x0[~vec] | (p[~vec] << 11)
    g, bit = np.nonzero((mask[:, None] >> np.arange(12)[None, :]) & 1)
    return words, x0[g] + bit, y[g], p[g], t[g], int(t[-1])


def cell(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def encode_rows(S, chunks, rounds, lib, coders=None, form="encode"):
    """the "encode" row: `Evt3Encoder` on the column chunks of the push rows (the events the stream was synthesised with), and the "copy"
    row: a device copy of the same input bytes, for scale -> (form, words per row and chunk, eager ms, replayed ms, launches) each.
    The sessions are the push rows': the encoder's state is reset, then the chunks are encoded one after the other.  Before anything
    is timed `Evt3Decoder` is checked to give the columns back from the encoder's words.  coders: another (encoder, decoder) pair with
    the same calls (tools/evt2_bench.py: `Evt2Encoder` and `Evt2Decoder`), its row named `form`."""
    from sast_amd.events import Evt3Decoder, Evt3Encoder
    enc, dec = coders or (Evt3Encoder(S), Evt3Decoder(S, max_events=chunks[0][0][0].shape[1]))
    words_out = []
    for cols, n in chunks:
        words, n_words = enc(*cols, n)
        got = dec(words, n_words)
        assert torch.equal(got[4], n) and enc.errors() == (0, 0, 0, 0), enc.errors()
        for s in range(S):
            k = int(n[s])
            assert all(torch.equal(g[s, :k].to(torch.int64), c[s, :k].to(torch.int64)) for g, c in zip(got[:4], cols))
        words_out.append(float(n_words.sum()) / S)
    del dec
    static, static_n = [t.clone() for t in chunks[0][0]], chunks[0][1].clone()
    sink = [torch.empty_like(t) for t in static]

    def copy():
        for d, s in zip(sink, static):
            d.copy_(s)

    rows = []
    for form, call in ((form, lambda: enc(*static, static_n)), ("copy", copy)):
        enc.reset()
        before = lib.sast_launch_count()
        call()
        launches = lib.sast_launch_count() - before
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        res = {"eager": [], "replayed": []}
        for mode in ("eager", "replayed"):
            for _ in range(rounds + 1):                                  # the first session warms up
                enc.reset()
                marks = []
                for ts, n in chunks:
                    for dst, src in zip(static + [static_n], ts + [n]):
                        dst.copy_(src)
                    m = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    m[0].record()
                    if mode == "eager":
                        call()
                    else:
                        g.replay()
                    m[1].record()
                    marks.append(m)
                torch.cuda.synchronize()
                res[mode].append(statistics.median(u.elapsed_time(v) for u, v in marks))
                assert enc.errors() == (0, 0, 0, 0) and float(enc.n_words.sum()) / S == words_out[-1], form
            res[mode] = res[mode][1:]
        rows.append((form, statistics.mean(words_out) if form != "copy" else 0, res["eager"], res["replayed"], launches))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8")
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--events", type=int, default=125000, help="events per row and chunk (about)")
    ap.add_argument("--vectors", type=float, default=0.3, help="share of groups that are a VECT_BASE_X + VECT_12 pair")
    ap.add_argument("--step", type=int, default=2, help="largest time step between groups, us")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd import _lib
    from sast_amd.events import EventQueue
    if not torch.cuda.is_available():
        raise SystemExit("tools/evt3_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _lib.lib()
    props = torch.cuda.get_device_properties(0)
    lines = [f"# tools/evt3_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; Gen4 720 x 1280, synthetic EVT 3.0 streams ({a.vectors:.0%} of the groups VECT_BASE_X + VECT_12, time steps "
             f"up to {a.step} us), {a.chunks} chunks of about {a.events} events per row and session; median (min .. max) ms per push of one "
             f"chunk over {a.rounds} sessions; chunks already in device memory",
             "# push: int16 x / y / p + int32 t columns;  push_dat: packed Event2D records;  push_evt3: the raw 16-bit words, decoded on the "
             "device;  B/ev: bytes in per event;  launches: library kernel launches per push",
             "# encode: Evt3Encoder on the columns of the push row, ms per call, `words` the words it gives per row and chunk;  copy: a device "
             "copy of the same four column tensors, for scale (no library launch)",
             f"{'S':>3}{'form':>11}{'ev/chunk':>10}{'words':>9}{'B/ev':>7}  {'eager ms':<26}{'replayed ms':<26}{'launches':>9}"]
    kw = dict(height=H, width=W, bins=10, count_cutoff=10, duration_us=WINDOW_US, downsample_by_2=True)
    for S in (int(v) for v in a.streams.split(",")):
        rng = np.random.RandomState(100 + S)
        rows = []
        for s in range(S):
            t0, parts = 1000 * s, []
            for k in range(a.chunks):
                part = synthetic_chunk(rng, a.events, a.vectors, a.step, t0, k == 0)
                t0 = part[-1]
                parts.append(part)
            rows.append(parts)
        ev_cap = max(len(part[1]) for parts in rows for part in parts)
        w_cap = (max(len(part[0]) for parts in rows for part in parts) + 7) // 8 * 8
        assert max(part[-1] for parts in rows for part in parts) < 2 ** 31
        total = max(sum(len(part[1]) for part in parts) for parts in rows)
        n_events = sum(len(part[1]) for parts in rows for part in parts) / (S * a.chunks)
        n_words = sum(len(part[0]) for parts in rows for part in parts) / (S * a.chunks)

        def stacked(idx, cap, dtype, k):
            buf = np.zeros((S, cap), dtype)
            for s in range(S):
                buf[s, :len(rows[s][k][idx])] = rows[s][k][idx]
            return torch.from_numpy(buf.view(np.int16) if dtype == np.uint16 else buf).to(dev)

        chunks = {"push": [], "push_dat": [], "push_evt3": []}
        for k in range(a.chunks):
            x, y, p = (stacked(i, ev_cap, np.int16, k) for i in (1, 2, 3))
            t = stacked(4, ev_cap, np.int32, k)
            n_ev = torch.tensor([len(rows[s][k][1]) for s in range(S)], dtype=torch.int64, device=dev)
            rec = torch.stack([t, x.to(torch.int32) | (y.to(torch.int32) << 14) | (p.to(torch.int32) << 28)], -1).contiguous()
            chunks["push"].append(([x, y, p, t], n_ev))
            chunks["push_dat"].append(([rec], n_ev))
            chunks["push_evt3"].append(([stacked(0, w_cap, np.uint16, k)],
                                        torch.tensor([len(rows[s][k][0]) for s in range(S)], dtype=torch.int64, device=dev)))
        queues = {form: EventQueue(S, total + 8, **kw) for form in chunks}
        calls = {"push": lambda q, ts, n: q.push(*ts, n), "push_dat": lambda q, ts, n: q.push_dat(*ts, n),
                 "push_evt3": lambda q, ts, n: q.push_evt3(*ts, n, max_events=ev_cap)}
        # the three forms hold the same events
        for form, q in queues.items():
            for ts, n in chunks[form]:
                calls[form](q, ts, n)
        ref = queues["push"]
        for form, q in queues.items():
            assert torch.equal(q.count, ref.count) and q.errors() == (0, 0, 0, 0), (form, q.errors())
            for name in ("x", "y", "p", "t"):
                assert torch.equal(getattr(q, name), getattr(ref, name)), (form, name)
        assert queues["push_evt3"].evt3_errors() == (0, 0, 0), queues["push_evt3"].evt3_errors()
        bytes_in = {"push": 10.0, "push_dat": 8.0, "push_evt3": 2.0 * n_words / n_events}
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

            lines.append(f"{S:>3}{form:>11}{n_events:>10.0f}{n_words if form == 'push_evt3' else 0:>9.0f}{bytes_in[form]:>7.2f}  "
                         f"{cell(res['eager']):<26}{cell(res['replayed']):<26}{launches:>9}")
            print(lines[-1], flush=True)
        for row in encode_rows(S, chunks["push"], a.rounds, lib):
            lines.append(f"{S:>3}{row[0]:>11}{n_events:>10.0f}{row[1]:>9.0f}{10.0:>7.2f}  {cell(row[2]):<26}{cell(row[3]):<26}{row[4]:>9}")
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
