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

--rotation times the augmentor with rotation instead (SpatialAugmentor(rotation=True), csrc/k_rotaug.hip), Gen1 and Gen4 / 2 frames,
T x B = 5 x 8, every sample rotated by an angle of 2..6 degrees of either sign on top of the same mix of flips and zooms:
  rotating  one launch of the rotating kernel
  plain     the kernel without rotation on the same frames and states, rotation inactive (what rotation costs on top)
  aten      flip, torchvision's tensor rotate restated in ATen (the sampling grid built once per sample outside the timing;
            .float(), grid_sample(nearest, zeros), round, .to(uint8) per frame), then the zoom as above
The rotating kernel's frames are compared with the ATen frames: torch's matrix product may round a source coordinate that lies on a tie
the other way, so the number of differing bytes is reported and bounded, not required to be 0 (the rule is include/sast_hip.h's).

  python tools/augment_bench.py --rotation [--reps 20] [--rounds 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import math
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


ANGLES = [2.0, -3.5, 6.0, -2.0, 4.25, -6.0, 3.0, -5.0]


def rotation_grid(angle, H, W, dev):
    """the sampling grid of torchvision.transforms.functional.rotate(expand=False, center=None): the inverse affine matrix of -angle,
    the linspace base grid, theta divided by the half sizes, bmm -> fp32 [1, H, W, 2]"""
    r = math.radians(-angle)
    theta = torch.tensor([math.cos(r), math.sin(r), 0.0, -math.sin(r), math.cos(r), 0.0], dtype=torch.float32, device=dev).reshape(1, 2, 3)
    base = torch.empty(1, H, W, 3, dtype=torch.float32, device=dev)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + 0.5, W * 0.5 + 0.5 - 1, steps=W, device=dev))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + 0.5, H * 0.5 + 0.5 - 1, steps=H, device=dev).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float32, device=dev)
    return base.view(1, H * W, 3).bmm(rescaled).view(1, H, W, 2)


def aten_augment_rotation(frames, sts, grids, out):
    """aten_augment with the rotation between the flip and the zoom; grids[b]: rotation_grid of sample b, or None"""
    T, B, _C, H, W = frames.shape
    plain = [type(st)(apply_h_flip=False, apply_zoom_in=st.apply_zoom_in, zoom_out=st.zoom_out, zoom_in=st.zoom_in) for st in sts]
    for t in range(T):
        for b, st in enumerate(sts):
            x = frames[t, b]
            if st.apply_h_flip:
                x = torch.flip(x, dims=[-1])
            if grids[b] is not None:
                y = torch.nn.functional.grid_sample(x.unsqueeze(0).float(), grids[b], mode="nearest", padding_mode="zeros", align_corners=False)
                x = torch.round(y[0]).to(frames.dtype)
            aten_augment(x[None, None], plain[b:b + 1], out[t:t + 1, b:b + 1])
    return out


def main_rotation(a):
    from sast_amd import augment as A
    dev = torch.device("cuda")
    props = torch.cuda.get_device_properties(0)
    cfg = dict(CONFIG, rotate=dict(prob=0.5, min_angle_deg=2, max_angle_deg=6))
    lines = [f"# tools/augment_bench.py --rotation on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), "
             f"torch {torch.__version__}; uint8 frames [5, 8, 20, H, W], the fixed mix of flips and zooms, every sample rotated by 2..6 degrees; "
             f"{a.rounds} interleaved rounds of {a.reps} calls each, the median round",
             "# rotating: SpatialAugmentor(rotation=True), one launch; plain: the kernel without rotation, same frames and states, rotation "
             "inactive; aten: flip / grid_sample on a prebuilt grid / zoom per sample and timestep on the same GPU; differing bytes: "
             "rotating vs aten frames (source coordinates on a rounding tie)"]
    lines.append(f"{'case':<16}{'rotating ms':>13}{'plain ms':>10}{'aten ms':>10}{'rot/plain':>11}{'aten/rot':>10}{'differing bytes':>17}")
    g = torch.Generator(device="cpu").manual_seed(0)
    slower = []
    T, B = 5, 8
    for name, H, W in (("gen1", 240, 304), ("gen4_half", 360, 640)):
        shape = (T, B, 20, H, W)
        on = torch.randint(0, 12, shape, generator=g, dtype=torch.uint8) == 0
        frames = (on * torch.randint(1, 11, shape, generator=g, dtype=torch.uint8)).to(dev)
        sts_plain, sts = states(B, H, W), states(B, H, W)
        for b, st in enumerate(sts):
            st.rotation = A.RotationState(True, ANGLES[b % len(ANGLES)])
        rot, plain = A.SpatialAugmentor((H, W), cfg, B, rotation=True), A.SpatialAugmentor((H, W), CONFIG, B)
        rot.set_state(sts)
        plain.set_state(sts_plain)
        grids = [rotation_grid(st.rotation.angle_deg, H, W, dev) for st in sts]
        out_rot, out_plain, out_aten = (torch.empty_like(frames) for _ in range(3))
        forms = {"rotating": lambda: rot(frames, out=out_rot), "plain": lambda: plain(frames, out=out_plain),
                 "aten": lambda: aten_augment_rotation(frames, sts, grids, out_aten)}
        for fn in forms.values():
            fn()
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, fn in forms.items():
                ms[k].append(timed(fn, a.reps))
        differing = int((out_rot != out_aten).sum())
        assert differing <= 1e-4 * frames.numel(), (name, differing)
        assert torch.equal(out_plain, aten_augment(frames, sts_plain, torch.empty_like(frames)))
        t = {k: statistics.median(v) for k, v in ms.items()}
        if not t["rotating"] <= t["aten"]:
            slower.append((name, t))
        lines.append(f"{name + f'_b{B}_t{T}':<16}{t['rotating']:>13.4f}{t['plain']:>10.4f}{t['aten']:>10.3f}{t['rotating'] / t['plain']:>10.2f}x"
                     f"{t['aten'] / t['rotating']:>9.1f}x{differing:>17d}")
        print(lines[-1], flush=True)
        del frames, out_rot, out_plain, out_aten, grids
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    assert not slower, f"the rotating kernel is slower than the ATen form: {slower}"


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
    ap.add_argument("--rotation", action="store_true", help="time the augmentor with rotation instead (see the module docstring)")
    a = ap.parse_args()
    if a.rotation:
        return main_rotation(a)
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
