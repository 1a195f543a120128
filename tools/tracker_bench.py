"""Timing of the device-resident tracker (sast_amd/tracking.py, csrc/k_track.hip), all in this one process:

  step      one sast_tracker_step at S = 8 rows, max_det 100, max_tracks 64 with about 30 live tracks and 30 detections per row (and the
            worst case beside it: 100 detections against a full table), next to one sast_detections_export of the same rows.  Both are
            timed as 50 launches captured in one graph and replayed, so the figure is the GPU's time per launch and not the host's issue rate.
  push      one captured `OnlineDetector` push (windows_per_step 2) with and without the tracker, on the detector and the synthetic Gen4
            recordings of tools/online_detector_bench.py; the objectness bias is raised as tests/test_online_detector.py does, so that the
            randomly initialised head gives records at all.  Wall clock from the replay to the results on the host, and the graph alone.
  run       `track_recordings` on one row of 1200 steps (60 s at 50 ms) with about 30 records each.

Medians after warm-up, (min .. max) behind them.

  python tools/tracker_bench.py [--reps 20] [--streams 8] [--out FILE] [--commit TEXT]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

MAX_DET, MAX_TRACKS, PER_GRAPH = 100, 64, 50


def objects(rs, S, n):
    """n boxes per row on a 640 x 360 field: fp32 [S, n, 4] (x, y, w, h), classes [S, n]"""
    wh = rs.randint(40, 240, (S, n, 2)) * 0.25
    xy = rs.rand(S, n, 2) * (np.array([640, 360]) - wh)
    return np.concatenate([np.floor(xy * 4) / 4, wh], -1).astype(np.float32), rs.randint(0, 3, (S, n))


def det_rows(box, cls, rs):
    """what postprocess_padded gives: fp32 [S, MAX_DET, 7] (x1, y1, x2, y2, obj, class_conf, class)"""
    S, n = cls.shape
    det = np.zeros((S, MAX_DET, 7), np.float32)
    det[:, :n, 0:2], det[:, :n, 2:4] = box[..., 0:2], box[..., 0:2] + box[..., 2:4]
    det[:, :n, 4], det[:, :n, 5], det[:, :n, 6] = 0.9, rs.randint(32, 65, (S, n)) / 64.0, cls
    return det


def med(v):
    return f"{statistics.median(v):9.2f} ({min(v):.2f} .. {max(v):.2f})"


def graph_us(fn, reps):
    """us per call of fn, PER_GRAPH calls captured once and replayed: the median over `reps` replays"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(PER_GRAPH):
            fn()
    out = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b) / PER_GRAPH)
    return out[2:]


def step_section(S, reps, lines):
    from sast_amd.online import export_detections
    from sast_amd.tracking import DetectionTracker
    dev, rs = torch.device("cuda"), np.random.RandomState(1)
    for n, label in ((30, "about 30 live tracks, 30 detections per row"), (MAX_DET, f"a full table, {MAX_DET} detections per row")):
        box, cls = objects(rs, S, n)
        det, n_det = torch.from_numpy(det_rows(box, cls, rs)).to(dev), torch.full((S,), n, dtype=torch.int32, device=dev)
        ends, due = torch.full((S,), 50000, dtype=torch.int64, device=dev), torch.ones(S, dtype=torch.uint8, device=dev)
        records = torch.zeros(S, MAX_DET, 40, dtype=torch.uint8, device=dev)
        counts, trunc = torch.zeros(S, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        tr = DetectionTracker(S, MAX_DET, max_tracks=MAX_TRACKS)
        export_detections(det, n_det, ends, due, records, counts, trunc)
        tr.step(records, counts, ends, due)                               # the tracks are born; every later step continues them
        live = int((tr.ids != 0).sum()) / S
        t_exp = graph_us(lambda: export_detections(det, n_det, ends, due, records, counts, trunc), reps)
        t_trk = graph_us(lambda: tr.step(records, counts, ends, due), reps)
        matched = int(tr.hits.max())
        lines.append(f"step, S {S}, max_det {MAX_DET}, max_tracks {MAX_TRACKS}, {label} ({live:.0f} live per row, longest track {matched} steps)")
        lines.append(f"  sast_detections_export  us per launch {med(t_exp)}")
        lines.append(f"  sast_tracker_step       us per launch {med(t_trk)}")
        print("\n".join(lines[-3:]), flush=True)


def push_section(S, lines):
    import online_detector_bench as B
    from sast_amd.config import backbone_config, modified_hw, to_attr
    from sast_amd.detection import YoloXDetector
    from sast_amd.events import EventQueue
    from sast_amd.online import OnlineDetector
    from sast_amd.tracking import DetectionTracker
    dev, T, E, W = torch.device("cuda"), 8, 200000, 2
    hw, part = modified_hw((B.H // 2, B.W // 2))
    torch.manual_seed(0)
    det = YoloXDetector(to_attr({"backbone": backbone_config(hw, part, embed_dim=64, AMP=2e-4, ls_init_value=1e-5),
                                 "fpn": {"name": "PAFPN", "depth": 0.67, "in_stages": [2, 3, 4], "depthwise": False, "act": "silu"},
                                 "head": {"name": "YoloX", "depthwise": False, "act": "silu", "num_classes": B.NUM_CLASSES}})).to(dev).eval()
    with torch.no_grad():
        for m in det.yolox_head.obj_preds:
            m.bias.fill_(2.0)
        for m in det.yolox_head.cls_preds:
            m.bias.fill_(0.0)
    cols, ends = B.synthetic(S, T, E, seed=100 * S + T)
    cols[3] = torch.clamp(cols[3] - (ends[0:1].T - B.WINDOW_US), min=0)
    chunk = 2 * E                                                         # two windows per chunk: both steps of a push are due
    chunks = [[c[:, lo:lo + chunk].to(d).contiguous().to(dev) for c, d in zip(cols, (torch.int16,) * 3 + (torch.int32,))]
              for lo in range(0, T * E, chunk)]
    counts = torch.full((S,), chunk, dtype=torch.int64, device=dev)
    kw = dict(height=B.H, width=B.W, bins=10, count_cutoff=10, duration_us=B.WINDOW_US, downsample_by_2=True)
    rows = []
    for tracked in (False, True, False, True):
        tr = DetectionTracker(S, MAX_DET, max_tracks=MAX_TRACKS, max_age_us=4 * B.WINDOW_US) if tracked else None
        od = OnlineDetector(det, EventQueue(S, 4 * chunk, window_capacity=2 * E, **kw), windows_per_step=W, max_det=MAX_DET, conf_thre=0.3,
                            nms_thre=0.45, tracker=tr)
        static = [torch.zeros_like(c) for c in chunks[0]]
        wall, graph, n_rec, n_ids = [], [], 0, 0
        with torch.no_grad():
            for rep in range(3):                                          # the recording again and again: reset at its first chunk
                for i, cols_i in enumerate(chunks):
                    reset = torch.full((S,), int(i == 0), dtype=torch.uint8, device=dev)
                    for dst, src in zip(static, cols_i):
                        dst.copy_(src)
                    if od._graph is None:
                        flags = reset.clone()
                        od.push(*static, counts, flags)
                        res = od.drain()
                        od.capture()
                        continue
                    flags.copy_(reset)
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    od._graph.replay()
                    b.record()
                    od._copy_out()
                    res = od.drain()
                    wall.append(1e3 * (time.perf_counter() - t0))
                    graph.append(a.elapsed_time(b))
                    n_rec += sum(len(r) for _s, r in res)
                    n_ids += sum(int((r["track_id"] != 0).sum()) for _s, r in res)
        rows.append((tracked, wall[2:], graph[2:], n_rec, n_ids))
        del od
        torch.cuda.empty_cache()
    lines.append(f"push, S {S}, windows_per_step {W}, max_det {MAX_DET}: one captured OnlineDetector push per chunk of two 50 ms windows (Gen4 / 2, "
                 f"{E} events per window and row), ms; two passes each, interleaved")
    for tracked, wall, graph, n_rec, n_ids in rows:
        lines.append(f"  {'with tracker   ' if tracked else 'without tracker'}  graph alone {med(graph)}   replay to host {med(wall)}   "
                     f"records {n_rec}, with an id {n_ids}")
    print("\n".join(lines[-5:]), flush=True)


def run_section(reps, lines):
    from sast_amd.labels import BBOX_DTYPE
    from sast_amd.tracking import DetectionTracker
    rs, steps, n = np.random.RandomState(3), 1200, 30
    box, cls = objects(rs, 1, n)
    rec = np.zeros(steps * n, BBOX_DTYPE)
    for k in range(steps):
        box[..., 0:2] += rs.randint(-8, 9, (1, n, 2)) * 0.25
        swap = rs.rand(n) < 0.03                                          # an object leaves, another comes
        if swap.any():
            box[0, swap], cls[0, swap] = objects(rs, 1, int(swap.sum()))[0][0], rs.randint(0, 3, int(swap.sum()))
        order = rs.permutation(n)
        r = rec[k * n:(k + 1) * n]
        r["t"], r["class_id"], r["class_confidence"] = 50000 * (k + 1), cls[0, order], rs.randint(32, 65, n) / 64.0
        r["x"], r["y"], r["w"], r["h"] = (box[0, order, c] for c in range(4))
    log = torch.from_numpy(rec.view(np.int32).reshape(1, steps * n, 10).copy()).cuda()
    cnt = torch.tensor([steps * n], dtype=torch.int64).cuda()
    tr = DetectionTracker(1, MAX_DET, max_tracks=MAX_TRACKS)
    out = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.track_recordings(log, cnt)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    ids = log.cpu().numpy().view(np.uint8).reshape(-1).view(BBOX_DTYPE)["track_id"]
    lines.append(f"run, one row of {steps} steps with {n} records each ({steps * n} records, {int(ids.max())} tracks, errors {tr.errors()}): "
                 f"track_recordings ms {med(out[2:])}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--no-push", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tracker_bench.py needs a GPU: nothing is measured without one")
    props = torch.cuda.get_device_properties(0)
    # the options that shape the measurement; where the table is written is not one of them
    lines = [f"# python tools/tracker_bench.py --reps {a.reps} --streams {a.streams}{' --no-push' if a.no_push else ''}",
             f"# commit {a.commit}; {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}; "
             f"medians (min .. max) after warm-up"]
    step_section(a.streams, a.reps, lines)
    run_section(a.reps, lines)
    if not a.no_push:
        push_section(a.streams, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
