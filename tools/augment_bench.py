"""Timing of the spatial augmentation (sast_amd/augment.py): uint8 event frames [T, B, 20, H, W] -> augmented frames.

Three things per shape, all timed in this one call, interleaved over `--rounds` rounds (the median round is reported):
  device  SpatialAugmentor: one launch of csrc/k_augment.hip for all T * B frames
  aten    the reference's algorithm (data/utils/augmentor.py:134-153, :203-222, :288-292) restated in ATen on the same GPU, per sample
          and timestep as the reference's data loader applies it: flip, slice, interpolate('nearest-exact'), zeros_like, paste
  copy    out.copy_(frames) of the same buffers: the streaming-copy rate of this call at this size (smaller cases fit the 256 MB
          Infinity Cache; tools/copy_calibration.py gives the rate of buffers far larger than it)
The frames of the last timed device call are checked equal to the ATen frames.  The states are a fixed mix, one of each flip x zoom
combination first.  Synthetic frames: one pixel in 12 holds a count 1..10.

  python tools/augment_bench.py [--reps 20] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIG = dict(prob_hflip=0.5, rotate=dict(prob=0, min_angle_deg=2, max_angle_deg=6),
              zoom=dict(prob=0.8, zoom_in=dict(weight=8, factor=dict(min=1, max=1.5)), zoom_out=dict(weight=2, factor=dict(min=1, max=1.2))))
# (flip, mode, factor, x0 as a share of the free width, y0 as a share of the free height)
MIX = [(1, "in", 1.3, 0.5, 0.4), (0, "out", 1.15, 0.4, 0.6), (1, "out", 1.2, 1.0, 0.0), (0, "in", 1.5, 0.2, 0.8),
       (1, "none", 1.0, 0, 0), (0, "none", 1.0, 0, 0), (0, "in", 1.1, 0.9, 0.1), (1, "out", 1.05, 0.0, 1.0)]


def states(B, H, W):
    from sast_amd import augment as A
    out = []
    for flip, mode, f, sx, sy in (MIX[b % len(MIX)] for b in range(B)):
        st = A.AugmentationState(apply_h_flip=bool(flip))
        wh, ww = int(H / f), int(W / f)
        x0, y0 = int(sx * (W - ww)), int(sy * (H - wh))
        if mode == "in":
            st.apply_zoom_in, st.zoom_in = True, A.ZoomInState(True, x0, y0, f)
        elif mode == "out":
            st.zoom_out = A.ZoomOutState(True, x0, y0, f)
        out.append(st)
    return out


def aten_augment(frames, sts, out):
    """frames, out: [T, B, C, H, W]; one sample and timestep after the other, each with the reference's tensor operations"""
    T, B, _C, H, W = frames.shape
    for t in range(T):
        for b, st in enumerate(sts):
            x = frames[t, b]
            if st.apply_h_flip:
                x = torch.flip(x, dims=[-1])
            if st.apply_zoom_in and st.zoom_in.active and st.zoom_in.zoom_in_factor != 1:
                f, x0, y0 = st.zoom_in.zoom_in_factor, st.zoom_in.x0, st.zoom_in.y0
                wh, ww = int(H / f), int(W / f)
                x = torch.nn.functional.interpolate(x[..., y0:y0 + wh, x0:x0 + ww].unsqueeze(0), size=(H, W), mode="nearest-exact")[0]
            elif st.zoom_out.active and st.zoom_out.zoom_out_factor != 1:
                f, x0, y0 = st.zoom_out.zoom_out_factor, st.zoom_out.x0, st.zoom_out.y0
                wh, ww = int(H / f), int(W / f)
                win = torch.nn.functional.interpolate(x.unsqueeze(0), size=(wh, ww), mode="nearest-exact")[0]
                x = torch.zeros_like(x)
                x[:, y0:y0 + wh, x0:x0 + ww] = win
            out[t, b].copy_(x)
    return out


def algorithmic_bytes(sts, T, C, H, W):
    """bytes the gather has to move: every output byte written once; read: the zoom-in window, the source rows a zoom-out uses, or the
    whole frame"""
    rd = 0
    for st in sts:
        if st.apply_zoom_in and st.zoom_in.active and st.zoom_in.zoom_in_factor != 1:
            f = st.zoom_in.zoom_in_factor
            rd += min(int(H / f), H - st.zoom_in.y0) * min(int(W / f), W - st.zoom_in.x0)
        elif st.zoom_out.active and st.zoom_out.zoom_out_factor != 1:
            rd += int(H / st.zoom_out.zoom_out_factor) * W
        else:
            rd += H * W
    return T * C * (rd + len(sts) * H * W)


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd.augment import SpatialAugmentor
    dev = torch.device("cuda")
    props = torch.cuda.get_device_properties(0)
    lines = [f"# tools/augment_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; uint8 frames [T, B, 20, H, W], a fixed mix of states (one of each flip x zoom combination first); "
             f"{a.rounds} interleaved rounds of {a.reps} calls each, the median round; the frames of the last timed device call are checked "
             "equal to the ATen frames",
             "# device: SpatialAugmentor (one launch); aten: flip / slice / interpolate / zeros_like / paste per sample and timestep on the "
             "same GPU; copy: out.copy_(frames) of the same buffers.  MB: algorithmic bytes of the gather (output written once; read: the "
             "zoom-in window, the source rows of a zoom-out, else the frame).  GB/s dev = MB / device ms; GB/s copy = 2 x buffer / copy ms; "
             "dev/copy = their ratio"]
    lines.append(f"{'case':<16}{'MB':>8}{'device ms':>11}{'aten ms':>10}{'copy ms':>9}{'aten/dev':>10}{'GB/s dev':>10}{'GB/s copy':>11}{'dev/copy':>10}")
    g = torch.Generator(device="cpu").manual_seed(0)
    slower = []
    for name, H, W in (("gen1", 240, 304), ("gen4", 360, 640)):
        for B in (4, 8):
            for T in (1, 5, 10):
                shape = (T, B, 20, H, W)
                on = torch.randint(0, 12, shape, generator=g, dtype=torch.uint8) == 0
                frames = (on * torch.randint(1, 11, shape, generator=g, dtype=torch.uint8)).to(dev)
                sts = states(B, H, W)
                aug = SpatialAugmentor((H, W), CONFIG, B)
                aug.set_state(sts)
                out_dev, out_aten, out_copy = (torch.empty_like(frames) for _ in range(3))
                forms = {"device": lambda: aug(frames, out=out_dev), "aten": lambda: aten_augment(frames, sts, out_aten),
                         "copy": lambda: out_copy.copy_(frames)}
                for fn in forms.values():          # warm up every form at this shape
                    fn()
                    fn()
                torch.cuda.synchronize()
                ms = {k: [] for k in forms}
                for _ in range(a.rounds):
                    for k, fn in forms.items():
                        ms[k].append(timed(fn, a.reps))
                assert torch.equal(out_dev, out_aten), (name, B, T)       # the frames of the last TIMED device call
                assert torch.equal(out_copy, frames)
                t = {k: statistics.median(v) for k, v in ms.items()}
                if not t["device"] < t["aten"]:
                    slower.append((name, B, T, t))
                moved = algorithmic_bytes(sts, T, 20, H, W)
                r_dev, r_copy = moved / t["device"] / 1e6, 2 * frames.numel() / t["copy"] / 1e6
                lines.append(f"{name + f'_b{B}_t{T}':<16}{moved / 1e6:>8.1f}{t['device']:>11.4f}{t['aten']:>10.3f}{t['copy']:>9.4f}"
                             f"{t['aten'] / t['device']:>9.1f}x{r_dev:>10.0f}{r_copy:>11.0f}{r_dev / r_copy:>10.2f}")
                print(lines[-1], flush=True)
                del frames, out_dev, out_aten, out_copy
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    assert not slower, f"the device form is not faster than the ATen form: {slower}"


if __name__ == "__main__":
    main()
