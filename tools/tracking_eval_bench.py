"""Timing of the device-resident tracking evaluator (sast_amd/tracking.py `TrackingEvaluator`, csrc/k_trackeval.hip), with its two
comparison points in the same process and on the same records:

  S rows of 1200 frames (60 s at 50 ms) with n labelled objects each, the detections jittered copies of them; n = 30, and the crowded
  variant n = 100.  `DetectionTracker.track_recordings` gives the detections their ids, `TrackingEvaluator.add_recordings` scores them
  against the labels, `PropheseeEvaluator.add_recordings` (time_tol_us 0) computes the mAP records of the same tensors.

Medians after warm-up, (min .. max) behind them.

  python tools/tracking_eval_bench.py [--reps 10] [--streams 8] [--out FILE] [--commit TEXT]
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

STEPS = 1200


def med(v):
    return f"{statistics.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})"


def rows(S, n, seed):
    """-> (gt, dt) numpy int32 [S, STEPS * n, 10]: n objects per row drifting over a 640 x 360 field (an object is replaced now and then, under a
    new label id), the detections their copies moved by up to 2 px, in another order, with track_id 0"""
    from sast_amd.labels import BBOX_DTYPE
    rs = np.random.RandomState(seed)
    wh = rs.randint(176, 320, (S, n, 2)) * 0.25                        # 44 .. 80 px: past gen4's box filter
    xy = np.floor(rs.rand(S, n, 2) * (np.array([640, 360]) - wh) * 4) / 4
    cls, ids, next_id = rs.randint(0, 3, (S, n)), np.tile(np.arange(1, n + 1), (S, 1)), n + 1
    gt, dt = np.zeros((S, STEPS, n), BBOX_DTYPE), np.zeros((S, STEPS, n), BBOX_DTYPE)
    for k in range(STEPS):
        xy = xy + rs.randint(-8, 9, (S, n, 2)) * 0.25
        swap = rs.rand(S, n) < 0.02
        m = int(swap.sum())
        if m:
            xy[swap], cls[swap] = np.floor(rs.rand(m, 2) * (np.array([640, 360]) - wh[swap]) * 4) / 4, rs.randint(0, 3, m)
            ids[swap], next_id = np.arange(next_id, next_id + m), next_id + m
        for out, jitter in ((gt, 0), (dt, 8)):
            order = np.argsort(rs.rand(S, n), axis=1)
            take = lambda a: np.take_along_axis(a, order, axis=1)          # noqa: E731
            r = out[:, k]
            r["t"], r["class_id"], r["class_confidence"] = 50000 * (k + 11), take(cls), rs.randint(32, 65, (S, n)) / 64.0
            r["x"], r["y"] = take(xy[..., 0]) + rs.randint(-jitter, jitter + 1, (S, n)) * 0.25, take(xy[..., 1]) + rs.randint(-jitter, jitter + 1, (S, n)) * 0.25
            r["w"], r["h"], r["track_id"] = take(wh[..., 0]), take(wh[..., 1]), take(ids) if out is gt else 0
    return tuple(a.reshape(S, STEPS * n).view(np.int32).reshape(S, STEPS * n, 10).copy() for a in (gt, dt))


def timed(fn, reps, before=None):
    out = []
    for _ in range(reps + 2):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out[2:]


def section(S, n, reps, lines):
    from sast_amd.evaluation import PropheseeEvaluator
    from sast_amd.tracking import DetectionTracker, TrackingEvaluator
    gt, dt = (torch.from_numpy(a).cuda() for a in rows(S, n, seed=n))
    cnt = torch.full((S,), STEPS * n, dtype=torch.int64, device="cuda")
    tr = DetectionTracker(S, 128, max_tracks=128, iou_thre=0.3, max_age_us=200_000)
    t_track = timed(lambda: tr.track_recordings(dt, cnt), reps)               # every call starts from an empty table: the same ids each time
    te = TrackingEvaluator("gen4", False, iou_thre=0.5, max_gt_tracks=65536, max_labels_per_frame=128, max_hyp_per_frame=128)
    t_eval = timed(lambda: te.add_recordings(gt, cnt, dt, cnt), reps, before=te.reset)
    ev = PropheseeEvaluator("gen4", False, max_images=S * STEPS, max_detections=S * STEPS * n, max_labels_per_frame=128)
    t_map = timed(lambda: ev.add_recordings(gt, cnt, dt, cnt, time_tol_us=0, max_window_detections=1024), reps, before=ev.reset_buffer)
    e, err = te.evaluate(), te.errors()
    lines.append(f"S {S} rows of {STEPS} frames, {n} labels and {n} hypotheses per frame ({S * STEPS * n} records a side; tracker errors {tr.errors()}, "
                 f"evaluator errors {sum(err.values())})")
    lines.append(f"  MOTA {e['MOTA']:.4f} MOTP {e['MOTP']:.4f} matches {e['matches']} fp {e['fp']} fn {e['fn']} idsw {e['idsw']} frag {e['frag']} "
                 f"tracks {e['gt_tracks']} (mt {e['mt']}, pt {e['pt']}, ml {e['ml']})")
    lines.append(f"  DetectionTracker.track_recordings    ms {med(t_track)}")
    lines.append(f"  TrackingEvaluator.add_recordings     ms {med(t_eval)}")
    lines.append(f"  PropheseeEvaluator.add_recordings    ms {med(t_map)}")
    print("\n".join(lines[-5:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tracking_eval_bench.py needs a GPU: nothing is measured without one")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# python tools/tracking_eval_bench.py --reps {a.reps} --streams {a.streams}",
             f"# commit {a.commit}; {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}; "
             f"medians (min .. max) after warm-up, one call each"]
    for n in (30, 100):
        section(a.streams, n, a.reps, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
