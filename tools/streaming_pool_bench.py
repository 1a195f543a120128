"""Timing of the streaming sampler: `StreamingPool.index`, `.next` and `.frames` (sast_amd/sampling.py) on a pool of Gen1-sized
synthetic recordings, with the `RandomAccessPool.batch` / `.frames` calls of the same batch shape next to them.

Pool: R = --rows recordings of --seconds s; per recording --events events (uniform pixels, timestamps spread evenly with one in 16 out
of order) and 4 Hz box labels (--boxes per label timestamp) with a gap of 3 s every 10 s, so that guarantee_labels cuts every recording
into several sub-sequences; gen1 filters, split 'train'.  A batch is B = --batch rows of L = --length windows of 50 ms, stacked
histogram of 10 bins; the schedule is `concat_orders(B)`.  Every call is bracketed by device events; the table gives, over --rounds
calls after one warm-up call, the median (min .. max) time of
  load_events     the time correction of all R rows (once per resident recording; shared with the random-access pool by events=)
  index           the sequence table, including its one synchronising copy to the host (once per pool contents)
  set_schedule    the host validation and the stream-ordered copies of the schedule
  next            the label tensors, masks and window ends of one streamed batch; the cursors advance
  frames          the event frames of that batch: L * B windows found through the per-step row map
  batch / frames (random access)   the same batch shape from `RandomAccessPool`
Events and records are already in device memory.  The inputs are synthetic; no real recording has been measured here.

  python tools/streaming_pool_bench.py [--rows 8] [--batch 8] [--length 21] [--seconds 60] [--events 2000000] [--boxes 6] [--rounds 9]
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
    k = np.arange(seconds * 4, dtype=np.int64)
    k = k[k % 40 < 28]                                     # 7 s of labels, 3 s without: 13 label periods between two label frames
    ts = 130000 + k * 250000 + rng.integers(-300, 301, len(k))
    n = len(ts) * boxes
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
    from sast_amd.labels import LabelStreams
    from sast_amd.sampling import RandomAccessPool, StreamingPool
    if not torch.cuda.is_available():
        raise SystemExit("tools/streaming_pool_bench.py needs a GPU: nothing is measured without one")
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
    pool = StreamingPool(ls, H, W, sequence_length=L, guarantee_labels=True, **kw)
    pool.load_events(*cols, n_ev)
    n_seq, sequences = pool.index(check=True)
    torch.manual_seed(0)
    orders = pool.concat_orders(B)
    pool.set_schedule(orders)
    out = pool.next()
    frames = pool.frames(out)
    assert pool.errors() == () and pool.frame_errors() == (0, 0) and int(frames.count_nonzero()) > 0, (pool.errors(), pool.frame_errors())
    rnd = RandomAccessPool(ls, H, W, sequence_length=L, **kw)
    rnd.load_events(*cols, n_ev)
    n_items, _sizes = rnd.index()
    items = torch.randperm(n_items)[:B].to(dev)
    r_out = rnd.batch(items)
    r_frames = rnd.frames(r_out)

    def count(fn):
        before = lib.sast_launch_count()
        fn()
        return lib.sast_launch_count() - before

    calls = [
        ("load_events", lambda: pool.load_events(*cols, n_ev)),
        ("index", lambda: pool.index()),
        ("set_schedule", lambda: pool.set_schedule(orders)),
        ("next", lambda: pool.next(out=out)),
        ("frames", lambda: pool.frames(out, out_frames=frames)),
        ("batch (random access)", lambda: rnd.batch(items, out=r_out)),
        ("frames (random access)", lambda: rnd.frames(r_out, out_frames=r_frames)),
    ]
    props = torch.cuda.get_device_properties(0)
    samples = int(sequences[:, 3].sum())
    lines = [f"# tools/streaming_pool_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; R = {R} gen1 rows of {a.seconds} s, {a.events} events and {int(ls.n_frames.max())} label frames each, "
             f"{n_seq} sub-sequences of {samples} samples; B = {B}, L = {L}: {L * B} windows of 50 ms, 10 bins, window_capacity {wcap}; "
             f"synthetic; median (min .. max) ms per call over {a.rounds} calls after a warm-up call",
             "# index includes its one synchronising copy to the host; set_schedule is host work plus three copies to the device;",
             "# next is timed on consecutive samples of the schedule (the cursors advance), frames on the last of them",
             f"{'call':<36}{'ms':<28}{'launches':>9}"]
    for name, fn in calls:
        k = count(fn)
        if name in ("next", "frames"):
            pool.set_schedule(orders)                        # enough steps for the timed calls of this row
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
