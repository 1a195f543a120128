"""Timing of the random-access sampler: `RandomAccessPool.index`, `.batch` and `.frames` (sast_amd/sampling.py) on a pool of Gen1-sized
synthetic recordings, with an `EventStreams` call that produces the same number of windows next to them.

Pool: R = --rows recordings of --seconds s; per recording --events events (uniform pixels, timestamps spread evenly with one in 16 out
of order) and 4 Hz box labels (--boxes per label timestamp), gen1 filters, split 'train'.  A batch is B = --batch items of
L = --length windows of 50 ms, stacked histogram of 10 bins.  Every call is bracketed by device events; the table gives, over --rounds
calls after one warm-up call, the median (min .. max) time of
  load_events     the time correction of all R rows (once per resident recording)
  index           the item index; index(weighted) also the class totals and the fp64 weights (once per pool)
  batch           the label tensors of one batch of random items
  frames          the event frames of that batch: L * B windows found through the row map
  EventStreams    one EventStreams call for T = L steps of S = B of the rows: L * B windows too, including its time correction, which
                  the pool did once in load_events (correct_time=False: without it)
Events and records are already in device memory.  The inputs are synthetic; no real recording has been measured here.

  python tools/random_access_bench.py [--rows 8] [--batch 8] [--length 21] [--seconds 60] [--events 2000000] [--boxes 6] [--rounds 9]
                                      [--out FILE]
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

H, W = 240, 304


def synthetic_labels(seconds: int, boxes: int, seed: int) -> np.ndarray:
    from sast_amd.labels import BBOX_DTYPE, LabelStreams
    rng = np.random.default_rng(seed)
    n_ts = seconds * 4
    ts = 130000 + np.arange(n_ts, dtype=np.int64) * 250000 + rng.integers(-300, 301, n_ts)
    n = n_ts * boxes
    b = np.zeros(n, dtype=BBOX_DTYPE)
    b["t"] = np.repeat(ts, boxes)
    b["x"], b["y"] = rng.uniform(0, W - 80, n), rng.uniform(0, H - 80, n)
    b["w"], b["h"] = rng.uniform(25, 75, n), rng.uniform(25, 75, n)
    b["class_id"] = rng.integers(0, 2, n)
    b["class_confidence"] = rng.uniform(0, 1, n)
    return LabelStreams.pack(b)


def synthetic_events(seconds: int, n: int, seed: int):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, seconds * 1000000, n)).astype(np.int64)
    late = rng.integers(0, 16, n) == 0
    t[late] -= rng.integers(0, 2000, int(late.sum()))
    return (rng.integers(0, W, n).astype(np.int16), rng.integers(0, H, n).astype(np.int16), rng.integers(0, 2, n).astype(np.int16),
            np.maximum(t, 0))


def timed(fn, rounds):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--length", type=int, default=21)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--events", type=int, default=2000000)
    ap.add_argument("--boxes", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd import _lib
    from sast_amd.events import EventStreams
    from sast_amd.labels import LabelStreams
    from sast_amd.sampling import RandomAccessPool
    if not torch.cuda.is_available():
        raise SystemExit("tools/random_access_bench.py needs a GPU: nothing is measured without one")
    if a.batch > a.rows:
        raise SystemExit("--batch must not exceed --rows: the EventStreams call beside the pool takes one window per row and step")
    dev = torch.device("cuda")
    lib = _lib.lib()
    R, B, L = a.rows, a.batch, a.length
    recs = [synthetic_labels(a.seconds, a.boxes, 100 + r) for r in range(R)]
    cap = max(len(r) for r in recs)
    rec = torch.from_numpy(np.stack([np.pad(r, ((0, cap - len(r)), (0, 0))) for r in recs])).to(dev)
    cnt = torch.tensor([len(r) for r in recs], dtype=torch.int64, device=dev)
    n_frames = 4 * a.seconds + 16
    ls = LabelStreams(R, cap, dataset="gen1", split="train", max_frames=n_frames, max_windows=2 * n_frames + 16, max_labels_per_frame=a.boxes)
    ls.load(rec, cnt, check=True)
    ev = [synthetic_events(a.seconds, a.events, 200 + r) for r in range(R)]
    cols = [torch.from_numpy(np.stack([e[k] for e in ev])).to(dev) for k in range(4)]
    n_ev = torch.full((R,), a.events, dtype=torch.int64, device=dev)
    wcap = max(4 * a.events * 50000 // (a.seconds * 1000000), 1024)          # four times the mean events of a 50 ms window
    kw = dict(bins=10, count_cutoff=10, duration_us=50000, window_capacity=wcap)
    pool = RandomAccessPool(ls, H, W, sequence_length=L, **kw)
    pool.load_events(*cols, n_ev)
    n, _sizes = pool.index(weighted=True)
    items = torch.multinomial(pool.weights[:n].cpu(), B, replacement=True).to(dev)
    out = pool.batch(items)
    frames = pool.frames(out)
    assert pool.errors() == ([()] * R, ()) and pool.frame_errors() == (0, 0) and int(frames.count_nonzero()) > 0, (pool.errors(), pool.frame_errors())
    streams = {ct: EventStreams(B, H, W, correct_time=ct, **kw) for ct in (True, False)}
    sub = [c[:B].contiguous() for c in cols]
    sub_t = {True: sub[3], False: pool.t[:B].contiguous()}
    ends = ls.ends_us[:B, 40:40 + L].t().contiguous()
    ones = torch.ones(B, dtype=torch.uint8, device=dev)
    es_out = torch.empty((L, B) + pool.get_shape(), dtype=torch.uint8, device=dev)

    def count(fn):
        before = lib.sast_launch_count()
        fn()
        return lib.sast_launch_count() - before

    calls = [
        ("load_events", lambda: pool.load_events(*cols, n_ev)),
        ("index", lambda: pool.index()),
        ("index(weighted)", lambda: pool.index(weighted=True)),
        ("batch", lambda: pool.batch(items, out=out)),
        ("frames", lambda: pool.frames(out, out_frames=frames)),
        ("EventStreams", lambda: streams[True](*sub[:3], sub_t[True], n_ev[:B], ends, reset=ones, out=es_out)),
        ("EventStreams, correct_time=False", lambda: streams[False](*sub[:3], sub_t[False], n_ev[:B], ends, out=es_out)),
    ]
    props = torch.cuda.get_device_properties(0)
    lines = [f"# tools/random_access_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; R = {R} gen1 rows of {a.seconds} s, {a.events} events and {int(ls.n_frames.max())} label frames each, "
             f"N = {n} items; B = {B}, L = {L}: {L * B} windows of 50 ms, 10 bins, window_capacity {wcap}; synthetic; median (min .. max) ms "
             f"per call over {a.rounds} calls after a warm-up call",
             "# index and index(weighted) include their one synchronising copy of the cumulative sizes to the host",
             f"{'call':<36}{'ms':<28}{'launches':>9}"]
    for name, fn in calls:
        k = count(fn)
        v = timed(fn, a.rounds)
        lines.append(f"{name:<36}{f'{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})':<28}{k:>9}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
