"""Timing of the label front end: `LabelStreams.load` and `LabelStreams.labels` (sast_amd/labels.py) on a Gen4-sized synthetic recording.

Per recording: --seconds s of labels at 60 Hz (period 16 667 us, a few hundred us of jitter), --boxes boxes per label timestamp
(uniform positions and sizes, classes 0 .. 4), gen4 filters, split 'train', downsampled by 2; S in --streams recordings side by side.
Every call is bracketed by device events; the table gives, over --rounds calls, the median time of
  load     one `load` of all S rows (once per recording: filters, label frames, window ends, label rows)
  labels   one `labels` call for T = --steps consecutive windows of every row
The records are already in device memory.  The inputs are synthetic; no real recording has been measured here.

  python tools/label_streams_bench.py [--streams 1,8] [--seconds 60] [--boxes 20] [--steps 10] [--rounds 9] [--out FILE]
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

PERIOD_US = 16667


def synthetic(seconds: int, boxes: int, seed: int) -> np.ndarray:
    """one recording's BBOX_DTYPE records as int32 [n, 10]"""
    from sast_amd.labels import BBOX_DTYPE, LabelStreams
    rng = np.random.default_rng(seed)
    n_ts = seconds * 1000000 // PERIOD_US
    ts = 120000 + np.arange(n_ts, dtype=np.int64) * PERIOD_US + rng.integers(-300, 301, n_ts)
    n = n_ts * boxes
    b = np.zeros(n, dtype=BBOX_DTYPE)
    b["t"] = np.repeat(ts, boxes)
    b["x"], b["y"] = rng.uniform(-40, 1300, n), rng.uniform(-40, 740, n)
    b["w"], b["h"] = rng.uniform(2, 400, n), rng.uniform(2, 300, n)
    b["class_id"] = rng.integers(0, 5, n)
    b["class_confidence"] = rng.uniform(0, 1, n)
    return LabelStreams.pack(b)


def timed(fn, rounds):
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
    ap.add_argument("--streams", default="1,8")
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--boxes", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd import _lib
    from sast_amd.labels import LabelStreams
    if not torch.cuda.is_available():
        raise SystemExit("tools/label_streams_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda")
    lib = _lib.lib()
    props = torch.cuda.get_device_properties(0)
    lines = [f"# tools/label_streams_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; gen4 / train / downsampled by 2, {a.seconds} s of labels at 60 Hz, {a.boxes} boxes per timestamp, synthetic; "
             f"median (min .. max) ms per call over {a.rounds} calls",
             f"# load: one LabelStreams.load of all S rows;  labels: one LabelStreams.labels call, T = {a.steps} steps;  launches: library "
             "kernel launches per load, labels",
             f"{'S':>3}{'records/row':>12}{'frames':>8}{'windows':>9}  {'load ms':<26}{'labels ms':<26}{'launches':>9}"]
    for S in (int(v) for v in a.streams.split(",")):
        rows = [synthetic(a.seconds, a.boxes, 1000 * S + s) for s in range(S)]
        cap = max(len(r) for r in rows)
        rec = torch.from_numpy(np.stack([np.pad(r, ((0, cap - len(r)), (0, 0))) for r in rows])).to(dev)
        cnt = torch.tensor([len(r) for r in rows], dtype=torch.int64, device=dev)
        n_frames = 10 * a.seconds + 16
        ls = LabelStreams(S, cap, dataset="gen4", split="train", downsample_by_2=True, max_frames=n_frames, max_windows=2 * n_frames + 16,
                          max_labels_per_frame=a.boxes)
        ls.load(rec, cnt, check=True)
        idx = (ls.frame_2_window[:, 3:4] + torch.arange(a.steps, device=dev)).t().contiguous()
        out = ls.labels(idx)
        assert int(out[3].sum()) >= S and ls.errors() == [()] * S, ls.errors()
        n0 = lib.sast_launch_count()
        ls.load(rec, cnt)
        n1 = lib.sast_launch_count()
        ls.labels(idx, out=out)
        n2 = lib.sast_launch_count()
        t_load = timed(lambda: ls.load(rec, cnt), a.rounds)
        t_lab = timed(lambda: ls.labels(idx, out=out), a.rounds)

        def cell(v):
            return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"

        lines.append(f"{S:>3}{cap:>12}{int(ls.n_frames.max()):>8}{int(ls.n_windows.max()):>9}  {cell(t_load):<26}{cell(t_lab):<26}"
                     f"{f'{n1 - n0}, {n2 - n1}':>9}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
