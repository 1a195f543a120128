"""Timing of the raw-events front end (sast_amd/events.py): B windows of synthetic events -> uint8 stacked-histogram frames.

Three forms of the same algorithm (time correction, window bounds, histogram, downsampling), per input size:
  device    EventFrames: the HIP kernels of csrc/k_events.hip
  aten_gpu  the reference's construct restated in ATen (`aten_construct`: put_(accumulate=True) on device tensors) + torch searchsorted /
            cummax / interpolate, on the same GPU
  cpu       the same ATen form on the CPU, torch.set_num_threads(16)
The inputs are synthetic (uniform pixels, a few hot pixels); no real sensor's event rate has been measured here.

  python tools/event_frames_bench.py [--sizes 100000,1000000,4000000] [--reps 20] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def aten_construct(x, y, pol, time_, bins, height, width, cutoff, fastmode):
    """representations.py:86-121 (StackedHistogram.construct) restated in ATen, on whatever device the tensors are on"""
    dtype = torch.uint8 if fastmode else torch.int16
    rep = torch.zeros((2, bins, height, width), dtype=dtype, device=x.device)
    if x.numel() == 0:
        return rep.to(torch.uint8).reshape(-1, height, width)
    t0, t1 = time_[0], time_[-1]
    t_norm = (time_ - t0) / torch.clamp(t1 - t0, min=1)           # int64 / int64 -> float32, true division
    t_idx = torch.clamp((t_norm * bins).floor(), max=bins - 1)
    idx = x.long() + width * y.long() + height * width * t_idx.long() + bins * height * width * pol.long()
    rep.put_(idx, torch.ones_like(idx, dtype=dtype), accumulate=True)
    rep = torch.clamp(rep, min=0, max=cutoff)
    return rep.to(torch.uint8).reshape(-1, height, width)


def aten_frames(x, y, p, t, ends, bins, height, width, cutoff, fastmode, duration_us, ds):
    """the windowing of preprocess_dataset.py:159-177 / :463-530 around aten_construct (one window after another, as the script does)"""
    t = torch.cummax(t, 0).values.clamp(min=0)
    p = p.clamp(min=0)
    e_idx = torch.searchsorted(t, ends, right=True)
    s_idx = torch.searchsorted(t, ends - duration_us, right=False)
    out = []
    for s, e in zip(s_idx.tolist(), e_idx.tolist()):
        r = aten_construct(x[s:e], y[s:e], p[s:e], t[s:e], bins, height, width, cutoff, fastmode)
        if ds:
            r = torch.nn.functional.interpolate(r.unsqueeze(0), scale_factor=0.5, mode="nearest-exact")[0]
        out.append(r)
    return torch.stack(out)


def synthetic(n_total, B, height, width, window_us, seed=0):
    g = np.random.default_rng(seed)
    x = g.integers(0, width, n_total, dtype=np.int64)
    y = g.integers(0, height, n_total, dtype=np.int64)
    p = g.integers(0, 2, n_total, dtype=np.int64)
    hot = g.random(n_total) < 0.002                    # a few hot pixels
    x[hot] = g.choice([11, 301, 7], hot.sum()) % width
    y[hot] = g.choice([21, 99, 201], hot.sum()) % height
    t = np.sort(g.integers(0, B * window_us, n_total, dtype=np.int64))
    ends = np.arange(1, B + 1, dtype=np.int64) * window_us
    return [torch.from_numpy(a) for a in (x, y, p, t)], torch.from_numpy(ends)


def timed(fn, reps, cuda):
    fn()
    if cuda:
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,4000000", help="events per window")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd.events import EventFrames
    torch.set_num_threads(16)
    dev = torch.device("cuda")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# tools/event_frames_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}, "
             f"CPU form on {torch.get_num_threads()} threads; synthetic events (uniform + 0.2 % on hot pixels), 50 ms windows, "
             "bins 10, cutoff 10, fastmode; every timed device call starts a new recording (reset of the time carry) and the frames"
             " of the last timed call are checked equal to the ATen frames",
             "# GB/s dev: algorithmic bytes of the device form over its time -- int64 x/y/p/t read 3x by the bucketing passes, t read and the"
             " corrected t written by the time correction, 4-byte records written and read (an upper bound: downsampling drops 3/4 of the"
             " records), the uint8 frames written; repeated reads partly hit the caches"]
    lines.append(f"{'case':<14}{'ev/window':>11}{'device ms':>11}{'aten_gpu ms':>13}{'cpu ms':>10}{'dev/aten':>10}{'Gev/s dev':>11}{'GB/s dev':>10}")
    for name, B, H, W, ds in (("gen4_ds2_b4", 4, 720, 1280, True), ("gen1_b4", 4, 240, 304, False)):
        for n in (int(s) for s in a.sizes.split(",")):
            cols, ends = synthetic(n * B, B, H, W, 50000, seed=n)
            dcols = [c.to(dev) for c in cols]
            dends = ends.to(dev)
            ef = EventFrames(H, W, bins=10, count_cutoff=10, duration_us=50000, downsample_by_2=ds, window_capacity=2 * n)
            last = {}

            def device_call():
                # every call is a new recording: without reset() the time-correction carry of the previous call (its maximum
                # timestamp) would raise every timestamp of the same events to it and empty the windows
                ef.reset()
                last["frames"] = ef(*dcols, dends)

            ref = aten_frames(*dcols, dends, 10, H, W, 10, True, 50000, ds)
            t_dev = timed(device_call, a.reps, True)
            got = last["frames"]
            assert torch.equal(got, ref), (name, n)                    # the frames of the last TIMED call
            assert ef.errors() == (0, 0), ef.errors()
            assert all(int(torch.count_nonzero(f)) > 0 for f in got), (name, n)
            t_aten = timed(lambda: aten_frames(*dcols, dends, 10, H, W, 10, True, 50000, ds), a.reps, True)
            t_cpu = timed(lambda: aten_frames(*cols, ends, 10, H, W, 10, True, 50000, ds), a.cpu_reps, False)
            ev = n * B
            moved = ev * (8 * 4 * 3 + 8 + 8 + 4 * 2) + got.numel()
            lines.append(f"{name:<14}{n:>11}{t_dev:>11.3f}{t_aten:>13.3f}{t_cpu:>10.1f}{t_aten / t_dev:>9.1f}x"
                         f"{ev / t_dev / 1e6:>11.2f}{moved / t_dev / 1e6:>10.0f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
