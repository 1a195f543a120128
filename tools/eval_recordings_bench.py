"""Timing of `PropheseeEvaluator.add_recordings` beside the per-frame `add` of the same images (sast_amd/evaluation.py, csrc/k_eval.hip).

One synthetic recording: --seconds (60) of labels at 60 Hz (1 .. 6 boxes per timestamp, quarter-pixel coordinates), and detections
every 50 ms, 3 at a time (60 % jittered copies of a label near them in time, 64 score levels).  With time_tol_us = 50 000 every label
timestamp is an image whose window holds the detections of two or three of those instants.  All in this one process, in turn:
  add_recordings  the whole recording in one call (S = 1; four launches, no host sync), timed with device events around --reps calls
                  into a buffer sized for them, the median of --rounds rounds after one warm-up round
  add             the existing per-frame path on THE SAME IMAGES: one frame per label timestamp, its labels and the detections of its
                  window as padded rows, all frames in one call (three launches) -- what this evaluation cost before add_recordings
                  existed, had someone aligned windows and labels by hand on the host (that host work is not timed)
  evaluate_buffer after one call of each, wall clock around the call (it ends in the one host copy), 3 calls each
The two buffers hold the same images, so their six numbers must be equal; the tool says whether they are.  No time is a pass criterion.

  python tools/eval_recordings_bench.py [--seconds 60] [--reps 20] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOL, M, HW = 50000, 6, (240, 304)


def _q(v):
    return np.round(np.asarray(v, np.float64) * 4) / 4


def synthetic(seconds, seed=0):
    """-> gt, dt as structured `labels.BBOX_DTYPE` arrays sorted by t"""
    from sast_amd.labels import BBOX_DTYPE
    rs = np.random.RandomState(seed)
    H, W = HW
    ts = 600000 + (np.arange(seconds * 60) * (1e6 / 60)).astype(np.int64)
    n = rs.randint(1, M + 1, len(ts))
    gt = np.zeros(int(n.sum()), BBOX_DTYPE)
    gt['t'] = np.repeat(ts, n)
    gt['w'], gt['h'] = _q(rs.uniform(12, 120, len(gt))), _q(rs.uniform(12, 100, len(gt)))
    gt['x'], gt['y'] = _q(rs.uniform(0, 1, len(gt)) * (W - gt['w'])), _q(rs.uniform(0, 1, len(gt)) * (H - gt['h']))
    gt['class_id'], gt['class_confidence'] = rs.randint(0, 2, len(gt)), 1.0
    td = np.repeat(600000 + 50000 * np.arange(seconds * 20, dtype=np.int64), 3)
    dt = np.zeros(len(td), BBOX_DTYPE)
    dt['t'] = td
    src = gt[np.clip(np.searchsorted(gt['t'], td) + rs.randint(0, M, len(td)), 0, len(gt) - 1)]
    copy = rs.rand(len(td)) < 0.6
    j = rs.uniform(-0.2, 0.2, (len(td), 4))
    dt['w'] = np.where(copy, _q(src['w'] * (1 + j[:, 2])), _q(rs.uniform(12, 120, len(td))))
    dt['h'] = np.where(copy, _q(src['h'] * (1 + j[:, 3])), _q(rs.uniform(12, 100, len(td))))
    dt['x'] = np.where(copy, _q(src['x'] + j[:, 0] * src['w']), _q(rs.uniform(0, 1, len(td)) * (W - dt['w'])))
    dt['y'] = np.where(copy, _q(src['y'] + j[:, 1] * src['h']), _q(rs.uniform(0, 1, len(td)) * (H - dt['h'])))
    dt['class_id'] = np.where(copy & (rs.rand(len(td)) < 0.8), src['class_id'], rs.randint(0, 2, len(td)))
    dt['class_confidence'] = rs.randint(1, 65, len(td)) / 64.0
    return gt, dt


def as_frames(gt, dt):
    """the same images as padded frames: labels fp32 [N, M, 7], counts int32 [N], det fp32 [N, A, 7], n_det int32 [N]"""
    ts = np.unique(gt['t'])
    lo, hi = np.searchsorted(dt['t'], ts - TOL, 'left'), np.searchsorted(dt['t'], ts + TOL, 'right')
    A = int((hi - lo).max())
    lab, cnt = np.zeros((len(ts), M, 7), np.float32), np.zeros(len(ts), np.int32)
    det, nd = np.zeros((len(ts), A, 7), np.float32), (hi - lo).astype(np.int32)
    first = np.searchsorted(gt['t'], ts, 'left')
    for i, t in enumerate(ts):
        g = gt[first[i]:first[i] + (gt['t'][first[i]:first[i] + M] == t).sum()]
        cnt[i] = len(g)
        lab[i, :len(g)] = np.stack([g['t'].astype(np.float32), g['x'], g['y'], g['w'], g['h'], g['class_id'].astype(np.float32),
                                    g['class_confidence']], 1)
        d = dt[lo[i]:hi[i]]
        det[i, :len(d)] = np.stack([d['x'], d['y'], d['x'] + d['w'], d['y'] + d['h'], np.full(len(d), 0.5, np.float32), d['class_confidence'],
                                    d['class_id'].astype(np.float32)], 1)
    return lab, cnt, det, nd


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_recordings_bench.py measures on the GPU: none found, nothing measured")
    from sast_amd import _lib
    from sast_amd.evaluation import PropheseeEvaluator
    from sast_amd.labels import LabelStreams
    dev = torch.device("cuda")
    props = torch.cuda.get_device_properties(0)
    gt, dt = synthetic(a.seconds)
    lab, cnt, det, nd = as_frames(gt, dt)
    n_img, members = len(cnt), int(nd.sum())
    lines = [f"# tools/eval_recordings_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; {a.rounds} rounds of {a.reps} calls each after a warm-up round, the median round",
             f"recording: {a.seconds} s, {n_img} label timestamps (60 Hz), {len(gt)} label records, {len(dt)} detection records (3 per 50 ms), "
             f"time_tol_us {TOL}: {members} detection memberships, at most {int(nd.max())} records per window"]
    rec = [torch.from_numpy(np.ascontiguousarray(LabelStreams.pack(v))[None]).to(dev) for v in (gt, dt)]
    n_rec = [torch.tensor([len(v)], dtype=torch.int64, device=dev) for v in (gt, dt)]
    frames = [torch.from_numpy(v).to(dev) for v in (lab, cnt, det, nd)]
    caps = dict(max_images=n_img * a.reps, max_detections=members * a.reps, max_labels_per_frame=M)
    ev_r, ev_f = PropheseeEvaluator("gen1", False, **caps), PropheseeEvaluator("gen1", False, **caps)

    def add_recordings():
        ev_r.add_recordings(rec[0], n_rec[0], rec[1], n_rec[1], time_tol_us=TOL, max_window_detections=64)

    def add():
        ev_f.add(*frames)

    result = {}
    for name, ev, fn, launches in (("add_recordings", ev_r, add_recordings, 4), ("add", ev_f, add, 3)):
        ms = []
        for i in range(a.rounds + 1):
            ev.reset_buffer()
            before = _lib.lib().sast_launch_count()
            ms.append(timed(fn, a.reps))
            assert i == 0 or _lib.lib().sast_launch_count() - before == launches * a.reps     # (the first call also clears the new buffer)
        ev.evaluate_buffer(*HW)                        # raises if anything was refused
        ev.reset_buffer()
        fn()
        torch.cuda.synchronize()
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            stats = ev.evaluate_buffer(*HW)
            wall.append((time.perf_counter() - t0) * 1e3)
        st = ev._state
        result[name] = (statistics.median(ms[1:]), min(ms[1:]), max(ms[1:]), statistics.median(wall), stats, [int(v) for v in st[:4]])
        lines.append(f"{name:<15} {launches} launches, {n_img} images per call: {result[name][0]:.3f} ms per call (rounds {result[name][1]:.3f} .. "
                     f"{result[name][2]:.3f});  evaluate_buffer after one call ({st[0]} images, {st[1]} ground truths, {st[2]} detections, "
                     f"{st[3]} records): {result[name][3]:.2f} ms wall (3 calls: {', '.join(f'{v:.2f}' for v in wall)});  AP {stats['AP']:.6f}")
        print(lines[-1], flush=True)
    r, f = result["add_recordings"], result["add"]
    lines.append(f"add_recordings / add: {r[0] / f[0]:.2f} x per call;  the two buffers hold "
                 + ("the same counts and give the same six numbers" if r[4] == f[4] and r[5] == f[5] else f"DIFFERENT results: {r[4:]} vs {f[4:]}"))
    lines.append(f"library {_lib.loaded_path() if not _lib.is_product_library() else 'in-tree product'}; knobs read: {_lib.knobs()}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
