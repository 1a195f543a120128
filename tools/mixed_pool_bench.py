"""Timing of the merged mixed batch: `MixedPool.next` + `.frames` + `JoinedAugmentor` for B = Bs + Br columns (sast_amd/sampling.py,
sast_amd/augment.py) against the path it replaces for the same rows -- `StreamingPool.next` + `.frames` + its augmentor for the Bs
streamed rows, `RandomAccessPool.batch` + `.frames` + its augmentor for the Br random-access samples, and the `torch.cat`s that merge
frames, labels, counts, `labelled` and the reset flags along the batch axis.  The replaced path runs none of the new code.

Pool: the synthetic recordings of tools/streaming_pool_bench.py (R = --rows Gen1-sized recordings of --seconds s, --events events each,
4 Hz box labels with gaps; gen1 filters, split 'train'), one job, events and records already in device memory.  A batch is L = --length
windows of 50 ms per column, stacked histogram of 10 bins; the stream schedule is `concat_orders(Bs)`, the items a `randperm`.  Every
call is bracketed by device events; the table gives the median (min .. max) time over --rounds calls after one warm-up call, and the
launches of the library each call makes (`sast_launch_count`; a `torch.cat` is a launch of torch's on top).  The augmentor states are
fixed (a flip, a zoom-out, a zoom-in, none, repeated).  The inputs are synthetic; no real recording has been measured here.

  python tools/mixed_pool_bench.py [--rows 8] [--stream 4] [--random 4] [--length 21] [--seconds 60] [--events 2000000] [--boxes 6]
                                   [--rounds 9] [--out FILE]
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
from streaming_pool_bench import H, W, synthetic_events, synthetic_labels, timed  # noqa: E402

STREAM_AUG = dict(prob_hflip=0.5, rotate=dict(prob=0, min_angle_deg=2, max_angle_deg=6),
                  zoom=dict(prob=0.5, zoom_out=dict(factor=dict(min=1, max=1.2))))
RANDOM_AUG = dict(prob_hflip=0.5, rotate=dict(prob=0, min_angle_deg=2, max_angle_deg=6),
                  zoom=dict(prob=0.8, zoom_in=dict(weight=8, factor=dict(min=1, max=1.5)), zoom_out=dict(weight=2, factor=dict(min=1, max=1.2))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--stream", type=int, default=4)
    ap.add_argument("--random", type=int, default=4)
    ap.add_argument("--length", type=int, default=21)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--events", type=int, default=2000000)
    ap.add_argument("--boxes", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd import _lib
    from sast_amd import augment as A
    from sast_amd.labels import LabelStreams
    from sast_amd.sampling import MixedPool, RandomAccessPool, StreamingPool
    if not torch.cuda.is_available():
        raise SystemExit("tools/mixed_pool_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _lib.lib()
    R, Bs, Br, L = a.rows, a.stream, a.random, a.length
    B = Bs + Br
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
    rnd = RandomAccessPool(ls, H, W, sequence_length=L, **kw)
    rnd.load_events(*cols, n_ev)
    n_items, _sizes = rnd.index()
    # two stream pools on the same events: the merged path's and the replaced path's, each with its own cursors
    sp, sp_old = (StreamingPool(ls, H, W, sequence_length=L, guarantee_labels=True, events=rnd, **kw) for _ in range(2))
    n_seq, sequences = sp.index(check=True)
    sp_old.index(check=True)
    torch.manual_seed(0)
    orders = sp.concat_orders(Bs)
    items = torch.randperm(n_items)[:Br].to(dev)
    mixed = MixedPool(sp, rnd)

    def states(n):
        kinds = [A.AugmentationState(apply_h_flip=True), A.AugmentationState(zoom_out=A.ZoomOutState(True, 20, 10, 1.15)),
                 A.AugmentationState(apply_zoom_in=True, zoom_in=A.ZoomInState(True, 30, 12, 1.3)), A.AugmentationState()]
        return [kinds[i % 4] for i in range(n)]

    parts = [A.SpatialAugmentor((H, W), STREAM_AUG, Bs), A.SpatialAugmentor((H, W), RANDOM_AUG, Br)]
    old = [A.SpatialAugmentor((H, W), STREAM_AUG, Bs), A.SpatialAugmentor((H, W), RANDOM_AUG, Br)]
    for p, o, n, skip in zip(parts, old, (Bs, Br), (0, Bs)):
        p.set_state(states(skip + n)[skip:])
        o.set_state(states(skip + n)[skip:])
    joined = A.JoinedAugmentor(parts)

    # ---- the merged path: every output keeps its place
    sp.set_schedule(orders)
    m_out = mixed.next(items)
    m_frames = mixed.frames(m_out)
    m_aug = torch.empty_like(m_frames)

    def merged():
        mixed.next(items, out=m_out)
        mixed.frames(m_out, out_frames=m_frames)
        return joined.joined(m_frames, m_out.labels, m_out.counts, yolox=True, out=m_aug)

    # ---- the path it replaces
    sp_old.set_schedule(orders)
    s_out = sp_old.next()
    s_frames = sp_old.frames(s_out)
    s_aug = torch.empty_like(s_frames)
    r_out = rnd.batch(items)
    r_frames = rnd.frames(r_out)
    r_aug = torch.empty_like(r_frames)
    ones = torch.ones(Br, dtype=torch.uint8, device=dev)

    def stream_half():
        sp_old.next(out=s_out)
        sp_old.frames(s_out, out_frames=s_frames)
        return old[0](s_frames, s_out.labels, s_out.counts, yolox=True, out=s_aug)

    def random_half():
        rnd.batch(items, out=r_out)
        rnd.frames(r_out, out_frames=r_frames)
        return old[1](r_frames, r_out.labels, r_out.counts, yolox=True, out=r_aug)

    def cats(s, r):
        return (torch.cat([s[0], r[0]], 1), torch.cat([s[1], r[1]], 1), torch.cat([s[2], r[2]], 1),
                torch.cat([s_out.labelled, r_out.labelled], 1), torch.cat([s_out.is_first, ones]))

    def replaced():
        return cats(stream_half(), random_half())

    # both paths give the same batch (same schedule, same items, same states)
    sp.set_schedule(orders)
    sp_old.set_schedule(orders)
    got, want = merged(), replaced()
    for g, w in zip(got + (m_out.labelled, m_out.is_first), want):
        assert torch.equal(g, w)
    assert mixed.errors() == ((), ([()] * R, ())) and mixed.frame_errors() == (0, 0) and int(got[0].count_nonzero()) > 0

    def count(fn):
        before = lib.sast_launch_count()
        fn()
        return lib.sast_launch_count() - before

    halves = [None, None]

    def keep(k, fn):
        halves[k] = fn()

    calls = [
        ("merged: next", lambda: mixed.next(items, out=m_out), ""),
        ("merged: frames", lambda: mixed.frames(m_out, out_frames=m_frames), ""),
        ("merged: joined augment", lambda: joined.joined(m_frames, m_out.labels, m_out.counts, yolox=True, out=m_aug), ""),
        ("merged: all three", merged, ""),
        ("replaced: stream next+frames+aug", lambda: keep(0, stream_half), ""),
        ("replaced: random batch+frames+aug", lambda: keep(1, random_half), ""),
        ("replaced: the concatenations", lambda: cats(*halves), " + 5 torch.cat"),
        ("replaced: all of it", replaced, " + 5 torch.cat"),
    ]
    props = torch.cuda.get_device_properties(0)
    lines = [f"# tools/mixed_pool_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; R = {R} gen1 rows of {a.seconds} s, {a.events} events and {int(ls.n_frames.max())} label frames each, "
             f"{n_seq} sub-sequences, {n_items} random-access items; B = {Bs} streamed + {Br} random = {B} columns, L = {L}: {L * B} windows "
             f"of 50 ms, 10 bins, window_capacity {wcap}; synthetic; median (min .. max) ms per call over {a.rounds} calls after a warm-up call",
             "# both paths give the same batch (checked before timing); next is timed on consecutive samples of the schedule",
             f"{'call':<40}{'ms':<28}{'launches':>9}"]
    for name, fn, extra in calls:
        for pool in (sp, sp_old):
            pool.set_schedule(orders)                        # enough steps for the timed calls of this row
        k = count(fn)
        v = timed(fn, a.rounds)
        lines.append(f"{name:<40}{f'{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})':<28}{k:>9}{extra}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
