"""Timing of the device-resident Prophesee mAP evaluator (sast_amd/evaluation.py, csrc/k_eval.hip).

Per call, all in this one process:
  forward   RNNDetector + YOLOPAFPN + YOLOXHead in eval mode on B = 8 Gen1-sized frames (256 x 320 padded, 2 classes, random weights):
            the work a validation step does before it evaluates
  post      postprocess_padded of that step's predictions at the reference's validation threshold (confidence 0.001, NMS 0.45)
  add       PropheseeEvaluator.add of N = 8 frames with D detections each (three launches, no host sync), for several D
  evaluate  PropheseeEvaluator.evaluate_buffer over a buffer of --frames frames with --dets detections each: the epoch-end sort,
            accumulate and summaries, the final host copy included
  summary   PropheseeEvaluator.summary behind an evaluate_buffer on that buffer: the accumulate at maxDets 1 / 10 / 100 with the recall
            and score tables, the twelve stats and its host copy.  Left out when the loaded library has no sast_evsum_accumulate
  merge     two evaluators with half of those frames each: PropheseeEvaluator.merge of one into the other (two launches, no host
            sync; timed once with events, after a warm-up on a small pair), then evaluate_buffer on the merged buffer.  Left out when
            the loaded library has no sast_evmerge_append (an A/B run against an older build through SAST_LIB_PATH)
A randomly initialised head puts nearly nothing above the threshold, so the detections that `add` and `evaluate` are timed on are
synthetic: per frame 1..12 labels, D boxes of which 60 % are jittered copies of a label and the rest random, 64 score levels.  D stands
for what survives confidence 0.001 and NMS on a trained detector; it is an input of this tool, not a measurement of one.

  python tools/eval_bench.py [--reps 20] [--rounds 5] [--frames 20000] [--dets 300] [--no-summary] [--out FILE]
"""
from __future__ import annotations

import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HW, PART, B, NC, M = (256, 320), (4, 5), 8, 2, 12


def synthetic(n_frames, dets, seed):
    """labels fp32 [n, M, 7], counts int32 [n], det fp32 [n, dets, 7], n_det int32 [n] on the host"""
    rs = np.random.RandomState(seed)
    H, W = 240, 304
    counts = rs.randint(1, M + 1, n_frames).astype(np.int32)
    lab = np.zeros((n_frames, M, 7), np.float32)
    wh = rs.uniform(8, 120, (n_frames, M, 2))
    xy = rs.uniform(0, 1, (n_frames, M, 2)) * (np.array([W, H]) - wh)
    lab[..., 0] = 600000 + 50000 * np.arange(n_frames)[:, None]
    lab[..., 1:3], lab[..., 3:5], lab[..., 5], lab[..., 6] = xy, wh, rs.randint(0, NC, (n_frames, M)), 1
    lab *= (np.arange(M)[None, :] < counts[:, None])[..., None]
    src = rs.randint(0, M, (n_frames, dets)) % counts[:, None]
    copy = rs.rand(n_frames, dets) < 0.6
    base = np.take_along_axis(lab, src[..., None], 1)
    j = rs.uniform(-0.25, 0.25, (n_frames, dets, 4))
    cx, cy = base[..., 1] + j[..., 0] * base[..., 3], base[..., 2] + j[..., 1] * base[..., 4]
    cw, ch = base[..., 3] * (1 + j[..., 2]), base[..., 4] * (1 + j[..., 3])
    rw, rh = rs.uniform(8, 120, (n_frames, dets)), rs.uniform(8, 120, (n_frames, dets))
    rx, ry = rs.uniform(0, 1, (n_frames, dets)) * (W - rw), rs.uniform(0, 1, (n_frames, dets)) * (H - rh)
    x, y, w, h = (np.where(copy, a, b) for a, b in ((cx, rx), (cy, ry), (cw, rw), (ch, rh)))
    det = np.zeros((n_frames, dets, 7), np.float32)
    det[..., 0], det[..., 1], det[..., 2], det[..., 3] = x, y, x + w, y + h
    det[..., 4], det[..., 5] = 0.5, rs.randint(1, 65, (n_frames, dets)) / 64.0
    det[..., 6] = np.where(copy & (rs.rand(n_frames, dets) < 0.8), base[..., 5], rs.randint(0, NC, (n_frames, dets)))
    return lab, counts, det, np.full(n_frames, dets, np.int32)


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--dets", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-summary", action="store_true", help="leave summary() out (what a library without it runs)")
    a = ap.parse_args()
    from sast_amd.config import backbone_config
    from sast_amd.detection import RNNDetector, YOLOPAFPN, YOLOXHead
    from sast_amd.evaluation import PropheseeEvaluator
    from sast_amd.functional import postprocess_padded
    dev = torch.device("cuda")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# tools/eval_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; {a.rounds} rounds of {a.reps} calls each, the median round; synthetic detections (see the tool's docstring)"]

    torch.manual_seed(0)
    net = RNNDetector(backbone_config(HW, PART, embed_dim=64, AMP=2e-4, ls_init_value=1e-5)).to(dev).eval()
    fpn = YOLOPAFPN(depth=0.67, in_stages=(2, 3, 4), in_channels=(128, 256, 512)).to(dev).eval()
    head = YOLOXHead(num_classes=NC, strides=(8, 16, 32), in_channels=(128, 256, 512)).to(dev).eval()
    x = (torch.rand(B, 20, *HW) > 0.5).int().to(dev)
    out = {}

    def forward():
        with torch.no_grad():
            feats, _st, _p = net.forward_nhwc(x)
            out["pred"] = head.forward_nhwc(fpn.forward_nhwc(feats))

    def post():
        out["det"] = postprocess_padded(out["pred"], NC, conf_thre=0.001, nms_thre=0.45)

    for fn in (forward, post):
        fn()
        fn()
    torch.cuda.synchronize()
    t_fwd = statistics.median(timed(forward, a.reps) for _ in range(a.rounds))
    t_post = statistics.median(timed(post, a.reps) for _ in range(a.rounds))
    A = int(out["pred"].shape[1])
    lines.append(f"forward  B={B} {HW[0]}x{HW[1]} backbone + PAFPN + head, eval, eager: {t_fwd:.3f} ms;  postprocess_padded of its {A} anchors "
                 f"per frame at confidence 0.001 (random weights: {int(out['det'][1].sum())} boxes kept): {t_post:.3f} ms")
    lines.append(f"{'add: N=8, D per frame':<26}{'ms per add':>12}{'share of forward':>18}")
    for D in (100, 300, 1000):
        lab, cnt, det, nd = (torch.from_numpy(v).to(dev) for v in synthetic(8, D, seed=D))
        ev = PropheseeEvaluator("gen1", False, max_images=8 * (a.reps + 2), max_detections=8 * D * (a.reps + 2), max_labels_per_frame=M)

        def add():
            ev.add(lab, cnt, det, nd)

        ms = []
        for _ in range(a.rounds + 1):
            ev.reset_buffer()
            ms.append(timed(add, a.reps))
        ev.evaluate_buffer(*HW)                     # raises if anything overflowed
        t = statistics.median(ms[1:])
        lines.append(f"{'D = ' + str(D):<26}{t:>12.4f}{t / t_fwd:>17.1%}")
        print(lines[-1], flush=True)

    F, D = a.frames, a.dets
    chunk = 8
    ev = PropheseeEvaluator("gen1", False, max_images=F, max_detections=F * D, max_labels_per_frame=M)
    pool = [tuple(torch.from_numpy(v).to(dev) for v in synthetic(chunk, D, seed=1000 + i)) for i in range(16)]
    for i in range(F // chunk):
        lab, cnt, det, nd = pool[i % len(pool)]
        ev.add(lab, cnt, det, nd)
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        stats = ev.evaluate_buffer(*HW)
        ms.append((time.perf_counter() - t0) * 1e3)
    bits = hashlib.sha256(ev.precision().cpu().numpy().tobytes()).hexdigest()[:16]
    st = ev._state
    lines.append(f"evaluate_buffer: {int(st[0])} images, {int(st[1])} ground truths, {int(st[2])} filtered detections, {int(st[3])} records "
                 f"(at most 100 per image and category): {statistics.median(ms):.2f} ms wall (3 calls: {', '.join(f'{v:.2f}' for v in ms)}), "
                 f"= {statistics.median(ms) / t_fwd:.1f} forward calls;  AP {stats['AP']:.4f}, precision table sha256 {bits}")
    from sast_amd import _lib
    if hasattr(_lib.lib(), "sast_evsum_accumulate") and not a.no_summary:
        ms_sum, ms_both = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            ev.evaluate_buffer(*HW)
            t1 = time.perf_counter()
            full = ev.summary()
            t2 = time.perf_counter()
            ms_sum.append((t2 - t1) * 1e3)
            ms_both.append((t2 - t0) * 1e3)
        tabs = ev.coco_eval()
        bits_s = hashlib.sha256(b"".join(tabs[k].cpu().numpy().tobytes() for k in ("precision", "recall", "scores"))).hexdigest()[:16]
        same = bool(torch.equal(tabs["precision"][..., 2], ev.precision())) and all(full[k] == stats[k] for k in stats)
        lines.append(f"summary() behind it (maxDets 1 / 10 / 100: precision, recall and score tables, twelve stats, per class; its host copy "
                     f"included): {statistics.median(ms_sum):.2f} ms wall (3 calls: {', '.join(f'{v:.2f}' for v in ms_sum)});  evaluate_buffer + "
                     f"summary(): {statistics.median(ms_both):.2f} ms;  AR_1 {full['AR_1']:.4f}, AR_10 {full['AR_10']:.4f}, AR_100 "
                     f"{full['AR_100']:.4f}, tables sha256 {bits_s}" + (" (maxDets-100 slice and first six equal evaluate_buffer's)" if same else ""))
    lines.append(f"library {_lib.loaded_path() if not _lib.is_product_library() else 'in-tree product'}; knobs read: {_lib.knobs()}")
    if hasattr(_lib.lib(), "sast_evmerge_append"):
        del ev
        half = (F // chunk // 2) * chunk

        def filled(n_frames, first, max_images, max_detections):
            e = PropheseeEvaluator("gen1", False, max_images=max_images, max_detections=max_detections, max_labels_per_frame=M)
            for i in range(first, first + n_frames // chunk):
                e.add(*pool[i % len(pool)])
            return e

        small_a, small_b = filled(chunk, 0, 2 * chunk, 2 * chunk * D), filled(chunk, 1, chunk, chunk * D)
        small_a.merge(small_b)                      # first use of the two kernels
        dst, src = filled(half, 0, 2 * half, 2 * half * D), filled(half, half // chunk, half, half * D)
        torch.cuda.synchronize()
        t_merge = timed(lambda: dst.merge(src), 1)
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            stats_m = dst.evaluate_buffer(*HW)
            ms.append((time.perf_counter() - t0) * 1e3)
        st = dst._state
        bits_m = hashlib.sha256(dst.precision().cpu().numpy().tobytes()).hexdigest()[:16]
        lines.append(f"merge of {half} frames into {half}: {t_merge:.3f} ms;  evaluate_buffer on the merged buffer: {int(st[0])} images, "
                     f"{int(st[3])} records: {statistics.median(ms):.2f} ms wall (3 calls: {', '.join(f'{v:.2f}' for v in ms)});  "
                     f"AP {stats_m['AP']:.4f}, precision table sha256 {bits_m}"
                     + (" (stats and table equal to the one evaluator's)" if stats_m == stats and bits_m == bits else ""))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
