"""Timing of the raw-events front end (sast_amd/events.py): B windows of synthetic events -> uint8 stacked-histogram frames.

Three forms of the same algorithm (time correction, window bounds, histogram, downsampling), per input size:
  device    EventFrames: the HIP kernels of csrc/k_events.hip
  aten_gpu  the reference's construct restated in ATen (`aten_construct`: put_(accumulate=True) on device tensors) + torch searchsorted /
            cummax / interpolate, on the same GPU
  cpu       the same ATen form on the CPU, torch.set_num_threads(16)
The inputs are synthetic (uniform pixels, a few hot pixels); no real sensor's event rate has been measured here.

  python tools/event_frames_bench.py [--sizes 100000,1000000,4000000] [--reps 20] [--out FILE]

--representation mixed_density | both: the mixed-density event stack (int8 [B, 20, H', W'], bins 20, cutoff 10) of the same windows,
timed beside the stacked-histogram call on the same events in the same job (device form of both, and the ATen restatement
`aten_md_construct` on the same GPU, against which the frames of the last timed call are checked):
  python tools/event_frames_bench.py --representation both --out profiles/r12_mixed_density_frames.txt
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


def aten_md_construct(x, y, pol, time_, bins, height, width, cutoff):
    """the mixed-density event stack (representations.py:164-218) in ATen with the bin taken from the fp32 exponent, as the device
    kernel does: int32 sums, prefix sum over the bins, int8 wrap, clamp"""
    rep = torch.zeros((bins, height, width), dtype=torch.int32, device=x.device)
    if x.numel() == 0:
        return rep.to(torch.int8)
    t0, t1 = time_[0], time_[-1]
    t_norm = ((time_ - t0) / torch.clamp(t1 - t0, min=1)).clamp(min=1e-6, max=1 - 1e-6)
    t_idx = torch.clamp(bins + torch.frexp(t_norm).exponent.long() - 1, min=0)
    idx = x.long() + width * y.long() + height * width * t_idx
    rep.put_(idx, (2 * pol - 1).to(torch.int32), accumulate=True)
    rep = ((torch.cumsum(rep, 0) + 128) % 256) - 128
    if cutoff is not None:
        rep = rep.clamp(min=-cutoff, max=cutoff)
    return rep.to(torch.int8)


def aten_frames(x, y, p, t, ends, bins, height, width, cutoff, fastmode, duration_us, ds, mixed_density=False):
    """the windowing of preprocess_dataset.py:159-177 / :463-530 around aten_construct (one window after another, as the script does)"""
    t = torch.cummax(t, 0).values.clamp(min=0)
    p = p.clamp(min=0)
    e_idx = torch.searchsorted(t, ends, right=True)
    s_idx = torch.searchsorted(t, ends - duration_us, right=False)
    out = []
    for s, e in zip(s_idx.tolist(), e_idx.tolist()):
        if mixed_density:
            r = aten_md_construct(x[s:e], y[s:e], p[s:e], t[s:e], bins, height, width, cutoff)
            r = r[:, 1::2, 1::2] if ds else r                     # nearest-exact at 0.5 (interpolate does not take int8)
        else:
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


def representations_table(a, dev, props):
    """the mixed-density call beside the stacked-histogram call: the same events, the same windows, one job"""
    from sast_amd.events import EventFrames
    both = a.representation == "both"
    lines = [f"# tools/event_frames_bench.py --representation {a.representation} on {props.name} ({getattr(props, 'gcnArchName', '?')}, "
             f"{props.multi_processor_count} CUs), torch {torch.__version__}; synthetic events (uniform + 0.2 % on hot pixels), 50 ms windows; "
             "stacked histogram: bins 10, cutoff 10, fastmode -> uint8 [B, 20, H', W'];  mixed density: bins 20, cutoff 10 -> int8 "
             "[B, 20, H', W'];  every timed device call starts a new recording, and the frames of the last timed call are checked "
             "equal to the ATen frames of the same representation",
             f"{'case':<14}{'ev/window':>11}{'hist ms':>10}{'mixed ms':>10}{'mixed/hist':>12}{'aten mixed ms':>15}{'Gev/s mixed':>13}"]
    for name, B, H, W, ds in (("gen4_ds2_b4", 4, 720, 1280, True), ("gen1_b4", 4, 240, 304, False)):
        for n in (int(s) for s in a.sizes.split(",")):
            cols, ends = synthetic(n * B, B, H, W, 50000, seed=n)
            dcols = [c.to(dev) for c in cols]
            dends = ends.to(dev)
            times = {}
            for rep, bins in (("stacked_histogram", 10), ("mixed_density", 20)):
                if rep == "stacked_histogram" and not both:
                    continue
                md = rep == "mixed_density"
                ef = EventFrames(H, W, bins=bins, count_cutoff=10, duration_us=50000, downsample_by_2=ds, window_capacity=2 * n,
                                 representation=rep)
                last = {}

                def device_call():
                    ef.reset()
                    last["frames"] = ef(*dcols, dends)

                ref = aten_frames(*dcols, dends, bins, H, W, 10, True, 50000, ds, mixed_density=md)
                times[rep] = timed(device_call, a.reps, True)
                assert torch.equal(last["frames"], ref), (name, n, rep)
                assert ef.errors() == (0, 0), ef.errors()
                if md:
                    times["aten"] = timed(lambda: aten_frames(*dcols, dends, bins, H, W, 10, True, 50000, ds, mixed_density=True), a.reps, True)
            t_md, t_h = times["mixed_density"], times.get("stacked_histogram")
            lines.append(f"{name:<14}{n:>11}" + (f"{t_h:>10.3f}" if both else f"{'-':>10}") + f"{t_md:>10.3f}" +
                         (f"{t_md / t_h:>11.2f}x" if both else f"{'-':>12}") + f"{times['aten']:>15.3f}{n * B / t_md / 1e6:>13.2f}")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--representation", default="stacked_histogram", choices=("stacked_histogram", "mixed_density", "both"),
                    help="mixed_density / both: time the mixed-density call (beside the stacked-histogram call) on the same events")
    ap.add_argument("--sizes", default="100000,1000000,4000000", help="events per window")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd.events import EventFrames
    torch.set_num_threads(16)
    dev = torch.device("cuda")
    props = torch.cuda.get_device_properties(0)
    if a.representation != "stacked_histogram":
        text = "\n".join(representations_table(a, dev, props)) + "\n"
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
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
