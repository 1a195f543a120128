"""Spatial augmentation of event frames and box labels on the GPU (csrc/k_augment.hip, csrc/k_rotaug.hip).

The reference augments in its data-loader workers on the CPU: RandomSpatialAugmentorGenX (data/utils/augmentor.py) flips, then zooms in
or out (with `rotation=True`: flips, rotates, then zooms), every tensor of a sample and its ObjectLabels
(data/genx_utils/labels.py:210-339).  `SpatialAugmentor` does the same to frames
that already live on the device (`sast_amd.events.EventFrames`): one launch for all frames of a [T, B, C, H, W] batch, one for the
labels, byte for byte / bit for bit what the reference computes.

- The random draws stay on the host, as in the reference (a dozen scalars per sample): `randomize()` makes the reference's calls on
  torch's global CPU generator in the reference's order, so the same `torch.manual_seed` gives the same states.
- The parameters the kernels read live in a small device tensor (`params`): a captured graph is replayed with new parameters by
  calling `randomize()` / `set_state()` between replays.
- Rotation is opt-in: `SpatialAugmentor(..., rotation=True)`.  Without it nothing differs from an augmentor that cannot rotate
  (`rotate.prob > 0` and a state with `rotation.active` raise NotImplementedError, as every shipped dataset config has `rotate.prob: 0`).
  With it the rotating kernels of csrc/k_rotaug.hip serve every sample, rotated or not -- flip, then rotate, then zoom, the reference's
  order -- and read the angles from a second device tensor (`rot_params`, include/sast_hip.h).  The frame rule is torchvision's tensor
  `rotate` (NEAREST, expand=False, center=None, fill=None) restated one fp32 rounding at a time, the label rule ObjectLabels.rotate_
  (tests/augment_rotation_model.py states both in numpy).  torchvision is not a dependency: parity with its own `rotate` is unpinned.
- Frames are uint8 or int8 (the mixed-density representation): the kernels move bytes, the border is 0, the result has the input's dtype.
- Vertical flip and optical-flow tensors are not reachable from the reference's __call__.

There is no CPU path: CPU tensors raise the library's "no CPU fallback" error.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple
from warnings import warn

import math

import numpy as np
import torch

from . import _lib as L
from ._frontend import not_capturing, same_device
from .functional import _need_gpu, _stream

NO_LABEL_WARN_MSG = 'No Labels found. This can lead to a crash and should not happen often.'


@dataclass
class ZoomOutState:
    active: bool = False
    x0: int = 0
    y0: int = 0
    zoom_out_factor: float = 1.0


@dataclass
class ZoomInState:
    """what the reference keeps in locals of _zoom_in_and_rescale: `active` is False when zoom-in was chosen but not applied (a factor
    of exactly 1, or no label frame to place the window on)"""
    active: bool = False
    x0: int = 0
    y0: int = 0
    zoom_in_factor: float = 1.0


@dataclass
class RotationState:
    active: bool = False
    angle_deg: float = 0.0


@dataclass
class AugmentationState:
    apply_h_flip: bool = False
    rotation: RotationState = field(default_factory=RotationState)
    apply_zoom_in: bool = False
    zoom_out: ZoomOutState = field(default_factory=ZoomOutState)
    zoom_in: ZoomInState = field(default_factory=ZoomInState)


def _get(cfg, key, *default):
    """cfg.key for attribute- or item-access configs (omegaconf.DictConfig, dict)"""
    if isinstance(cfg, dict):
        if key in cfg:
            return cfg[key]
    elif hasattr(cfg, key):
        return getattr(cfg, key)
    elif hasattr(cfg, "__getitem__"):
        try:
            return cfg[key]
        except (KeyError, IndexError, TypeError):
            pass
    if default:
        return default[0]
    raise KeyError(f"sast_amd.augment: augm_config has no '{key}'")


def _has(cfg, key) -> bool:
    sentinel = object()
    return _get(cfg, key, sentinel) is not sentinel


def _uniform(min_value, max_value):
    # utils/helpers.py:6-10 torch_uniform_sample_scalar: nothing is drawn when the interval is empty
    assert max_value >= min_value, f'{max_value=} is smaller than {min_value=}'
    if max_value == min_value:
        return min_value
    return min_value + (max_value - min_value) * torch.rand(1).item()


def _sample_window_from_label(label_xywh, input_height, input_width, zoom_window_height, zoom_window_width) -> Tuple[int, int]:
    # augmentor.py:407-448 randomly_sample_zoom_window_from_label_rectangle
    assert input_height >= zoom_window_height
    assert input_width >= zoom_window_width
    x0_l, y0_l, w_l, h_l = label_xywh
    x1_l = x0_l + w_l
    y1_l = y0_l + h_l
    assert x0_l >= 0
    assert y0_l >= 0
    assert w_l > 0
    assert h_l > 0
    assert x1_l <= input_width + 1e-2 - 1
    assert y1_l <= input_height + 1e-2 - 1
    x0_valid = max(x1_l - max(zoom_window_width, w_l), 0)
    y0_valid = max(y1_l - max(zoom_window_height, h_l), 0)
    x1_valid = min(x0_l + max(zoom_window_width, w_l), input_width - 1)
    y1_valid = min(y0_l + max(zoom_window_height, h_l), input_height - 1)
    x1_valid = max(x1_valid - zoom_window_width, x0_valid)
    y1_valid = max(y1_valid - zoom_window_height, y0_valid)
    x = int(_uniform(x0_valid, x1_valid))
    assert 0 <= x < input_width
    y = int(_uniform(y0_valid, y1_valid))
    assert 0 <= y < input_height
    return x, y


def _f32_bits(values) -> np.ndarray:
    return np.asarray(values, dtype=np.float64).astype(np.float32).view(np.int32)


def _rotation_words(angle_deg: float, H: int, W: int) -> np.ndarray:
    """one sample's row of rot_params (include/sast_hip.h) for an active rotation by angle_deg"""
    f32 = np.float32
    r = math.radians(-angle_deg)                                # torchvision: _get_inverse_affine_matrix on -angle
    m = [f32(math.cos(r)), f32(math.sin(r)), f32(-math.sin(r)), f32(math.cos(r))]
    half_w, half_h = f32(0.5 * W), f32(0.5 * H)                 # _gen_affine_grid: theta / [0.5 w, 0.5 h], an fp32 division
    p = np.zeros(L.ROTAUG_PARAM_WORDS, dtype=np.int32)
    p[0] = 1
    p[1:5] = np.array([m[0] / half_w, m[1] / half_w, m[2] / half_h, m[3] / half_h], dtype=f32).view(np.int32)
    a = angle_deg / 180 * math.pi                               # labels.py:228
    p[5:7] = _f32_bits([math.cos(a), math.sin(a)])
    return p


def _rotate_boxes_host(x, y, w, h, words: np.ndarray, H: int, W: int):
    """ObjectLabels.rotate_ (labels.py:210-248) on fp32 numpy columns, as the label kernel computes it (one rounding per operation)
    -> x, y, w, h of the boxes that are not flat.  The host needs it to place a zoom-in window on rotated labels."""
    f32 = np.float32
    co, si = words[5:7].view(f32)
    cx, cy = f32(W // 2), f32(H // 2)
    xs, ys = [], []
    for X, Y in ((x, y), (x + w, y), (x, y + h), (x + w, y + h)):
        px, py = X - cx, Y - cy
        xs.append((co * px + si * py) + cx)
        ys.append((-si * px + co * py) + cy)
    x0, x1 = np.clip(np.min(xs, axis=0), 0, f32(W - 1)), np.clip(np.max(xs, axis=0), 0, f32(W - 1))
    y0, y1 = np.clip(np.min(ys, axis=0), 0, f32(H - 1)), np.clip(np.max(ys, axis=0), 0, f32(H - 1))
    w, h = x1 - x0, y1 - y0
    keep = (w > 0) & (h > 0)
    return x0[keep], y0[keep], w[keep], h[keep]


class SpatialAugmentor:
    """RandomSpatialAugmentorGenX for a batch of device frames.

    aug = SpatialAugmentor(dataset_hw, augm_config, batch_size, rotation=False)
      rotation=True: rotate.prob > 0 and RotationState(True, angle_deg) are accepted, and every call goes through the rotating kernels
      (the host's choice of kernel never depends on a sample's state); the default refuses both and is the augmentor without rotation.
      augm_config: the reference's keys -- prob_hflip, rotate.{prob, min_angle_deg, max_angle_deg}, zoom.prob,
      zoom.zoom_in.{weight, factor.min, factor.max} (optional), zoom.zoom_out.{weight, factor.min, factor.max}.
    aug.randomize(samples=None, latest_labels=None)   new random states for all (or the listed) batch rows, host side
    aug.set_state(states)                             explicit states, one AugmentationState per batch row
    frames_out = aug(frames)                          frames: uint8 / int8 [T, B, C, H, W] or [B, C, H, W] on the device
    frames_out, labels_out, counts_out = aug(frames, labels, counts, yolox=False)
      labels: fp32 [T, B, M, 7] / [B, M, 7] rows (t, x, y, w, h, class_id, class_confidence); counts: int32 [T, B] / [B] valid rows
      (0: no labels).  labels_out has the surviving rows at the front in their order, zeros after; with yolox=True it is the head's
      [.., M, 5] = (class_id, cx, cy, w, h) layout instead (what YOLOXHead.forward(xin, labels) takes).
    A call only enqueues two launches: nothing is synchronised, and after one warm-up call it can be captured in a graph."""

    def __init__(self, dataset_hw: Tuple[int, int], augm_config, batch_size: int, rotation: bool = False):
        assert isinstance(dataset_hw, tuple)
        assert len(dataset_hw) == 2
        assert all(x > 0 for x in dataset_hw)
        if int(batch_size) < 1:
            raise ValueError("sast_amd.augment: batch_size must be >= 1")
        if max(dataset_hw) > 4096:
            raise ValueError("sast_amd.augment: frames up to 4096 x 4096 are supported")
        self.hw_tuple = (int(dataset_hw[0]), int(dataset_hw[1]))
        self.batch_size = int(batch_size)
        self.rotation = bool(rotation)
        rotate, zoom = _get(augm_config, "rotate"), _get(augm_config, "zoom")
        self.h_flip_prob = _get(augm_config, "prob_hflip")
        self.rot_prob = _get(rotate, "prob")
        self.rot_min_angle_deg = _get(rotate, "min_angle_deg", 0)
        self.rot_max_angle_deg = _get(rotate, "max_angle_deg")
        self.zoom_prob = _get(zoom, "prob")
        zoom_out = _get(zoom, "zoom_out")
        zoom_out_weight = _get(zoom_out, "weight", 1)
        self.min_zoom_out_factor = _get(_get(zoom_out, "factor"), "min")
        self.max_zoom_out_factor = _get(_get(zoom_out, "factor"), "max")
        has_zoom_in = _has(zoom, "zoom_in")
        zoom_in = _get(zoom, "zoom_in") if has_zoom_in else None
        zoom_in_weight = _get(zoom_in, "weight") if has_zoom_in else 0
        self.min_zoom_in_factor = _get(_get(zoom_in, "factor"), "min") if has_zoom_in else 1
        self.max_zoom_in_factor = _get(_get(zoom_in, "factor"), "max") if has_zoom_in else 1

        assert 0 <= self.h_flip_prob <= 1
        assert 0 <= self.rot_prob <= 1
        assert 0 <= self.rot_min_angle_deg <= self.rot_max_angle_deg
        assert 0 <= self.zoom_prob <= 1
        assert 0 <= zoom_in_weight
        assert self.max_zoom_in_factor >= self.min_zoom_in_factor >= 1
        assert 0 <= zoom_out_weight
        assert self.max_zoom_out_factor >= self.min_zoom_out_factor >= 1
        if self.rot_prob > 0 and not self.rotation:
            raise NotImplementedError("sast_amd.augment: rotation is not implemented without rotation=True (rotate.prob must be 0, as "
                                      "in every shipped dataset config)")
        self.zoom_in_or_out_distribution = torch.distributions.categorical.Categorical(
            probs=torch.tensor([zoom_in_weight, zoom_out_weight]))

        self.states: List[AugmentationState] = [AugmentationState() for _ in range(self.batch_size)]
        self._host = np.zeros((self.batch_size, L.AUGMENT_PARAM_WORDS), dtype=np.int32)
        self.params: Optional[torch.Tensor] = None   # int32 [B, AUGMENT_PARAM_WORDS] on the device, made by the first call
        self._rot_host = np.zeros((self.batch_size, L.ROTAUG_PARAM_WORDS), dtype=np.int32)
        self.rot_params: Optional[torch.Tensor] = None   # int32 [B, ROTAUG_PARAM_WORDS] on the device (rotation=True only)
        self._joined: Optional["JoinedAugmentor"] = None   # the JoinedAugmentor this one is a part of

    # ------------------------------------------------------------------------------------------------------------------- states
    def _draw(self, latest) -> AugmentationState:
        H, W = self.hw_tuple
        st = AugmentationState()
        # randomize_augmentation, augmentor.py:89-121
        st.apply_h_flip = self.h_flip_prob > torch.rand(1).item()
        st.rotation.active = self.rot_prob > torch.rand(1).item()      # without rotation=True never: rot_prob is 0, the draw is spent
        if st.rotation.active:                                         # augmentor.py:99-102
            sign = 1 if torch.randn(1).item() >= 0 else -1
            st.rotation.angle_deg = sign * _uniform(self.rot_min_angle_deg, self.rot_max_angle_deg)
        do_zoom = self.zoom_prob > torch.rand(1).item()
        do_zoom_in = self.zoom_in_or_out_distribution.sample().item() == 0
        do_zoom_out = not do_zoom_in
        do_zoom_in &= do_zoom
        do_zoom_out &= do_zoom
        st.apply_zoom_in = do_zoom_in
        st.zoom_out.active = do_zoom_out
        if do_zoom_out:
            f = _uniform(self.min_zoom_out_factor, self.max_zoom_out_factor)
            wh, ww = int(H / f), int(W / f)
            st.zoom_out.x0 = int(_uniform(0, W - ww))
            st.zoom_out.y0 = int(_uniform(0, H - wh))
            st.zoom_out.zoom_out_factor = f
        if do_zoom_in:
            # _zoom_in_and_rescale, augmentor.py:182-200, on the labels as __call__ sees them there: already flipped and rotated
            f = _uniform(self.min_zoom_in_factor, self.max_zoom_in_factor)
            if f == 1:
                return st
            wh, ww = int(H / f), int(W / f)
            if latest is None or latest.shape[0] == 0:
                warn(message=NO_LABEL_WARN_MSG, category=UserWarning, stacklevel=3)
                return st
            lab = latest.detach().to("cpu")
            x, y, w, h = lab[:, 1], lab[:, 2], lab[:, 3], lab[:, 4]
            if st.apply_h_flip:
                x = W - 1 - x - w                                         # labels.py:339, in the labels' dtype
            if st.rotation.active:
                x, y, w, h = (torch.from_numpy(v) for v in _rotate_boxes_host(
                    *(v.to(torch.float32).numpy() for v in (x, y, w, h)), _rotation_words(st.rotation.angle_deg, H, W), H, W))
                if x.shape[0] == 0:                                       # the rotation removed every box of the frame
                    warn(message=NO_LABEL_WARN_MSG, category=UserWarning, stacklevel=3)
                    return st
            samples = [_sample_window_from_label((x[i].item(), y[i].item(), w[i].item(), h[i].item()), H, W, wh, ww)
                       for i in range(x.shape[0])]
            idx = 0 if len(samples) == 1 else torch.randint(low=0, high=len(samples) - 1, size=(1,)).item()
            x0, y0 = samples[idx]
            assert W > x0 >= 0, f'{x0=}'
            assert H > y0 >= 0, f'{y0=}'
            st.zoom_in = ZoomInState(active=True, x0=x0, y0=y0, zoom_in_factor=f)
        return st

    def randomize(self, samples: Optional[Sequence[int]] = None, latest_labels: Optional[Sequence[Optional[torch.Tensor]]] = None):
        """New random states for the batch rows in `samples` (default: all), drawn from torch's global CPU generator with the
        reference's calls in its order, one row after the other.  latest_labels[b]: a CPU tensor [K, 7] with the most recent non-empty
        label frame of row b before augmentation, or None; zoom-in places its window on it, and without one warns and does not zoom."""
        rows = range(self.batch_size) if samples is None else [int(b) for b in samples]
        if latest_labels is not None and len(latest_labels) != self.batch_size:
            raise ValueError("sast_amd.augment: latest_labels must have one entry per batch row")
        for b in rows:
            if not 0 <= b < self.batch_size:
                raise ValueError(f"sast_amd.augment: batch row {b} outside 0..{self.batch_size - 1}")
            self.states[b] = self._draw(None if latest_labels is None else latest_labels[b])
            self._host[b], self._rot_host[b] = self._encode(self.states[b]), self._encode_rotation(self.states[b])
        self._upload()
        return self.states

    def set_state(self, states: Sequence[AugmentationState]):
        """explicit parameters: one AugmentationState per batch row (validated here, on the host)"""
        if len(states) != self.batch_size:
            raise ValueError(f"sast_amd.augment: {len(states)} states for a batch of {self.batch_size}")
        host, rot_host = np.stack([self._encode(s) for s in states]), np.stack([self._encode_rotation(s) for s in states])
        self.states = list(states)
        self._host[...] = host                                # in place: a JoinedAugmentor's part writes its rows of the joined array
        self._rot_host[...] = rot_host
        self._upload()

    def _encode(self, st: AugmentationState) -> np.ndarray:
        H, W = self.hw_tuple
        p = np.zeros(L.AUGMENT_PARAM_WORDS, dtype=np.int32)
        if st.rotation.active and not self.rotation:
            raise NotImplementedError("sast_amd.augment: rotation is not implemented without rotation=True")
        zin = bool(st.apply_zoom_in) and st.zoom_in.active and st.zoom_in.zoom_in_factor != 1
        zout = bool(st.zoom_out.active) and st.zoom_out.zoom_out_factor != 1
        if st.apply_zoom_in and st.zoom_out.active:
            raise ValueError("sast_amd.augment: zoom-in and zoom-out are mutually exclusive")
        p[0] = int(bool(st.apply_h_flip))
        if zin:
            f, x0, y0 = float(st.zoom_in.zoom_in_factor), int(st.zoom_in.x0), int(st.zoom_in.y0)
            if not f >= 1:
                raise ValueError(f"sast_amd.augment: zoom-in factor {f} must be >= 1")
            wh, ww = int(H / f), int(W / f)
            if wh < 1 or ww < 1 or not (0 <= x0 <= W - 1 and 0 <= y0 <= H - 1):
                raise ValueError(f"sast_amd.augment: zoom-in window {wh}x{ww} at ({x0}, {y0}) does not start inside the {H}x{W} frame")
            p[1:6] = (L.AUGMENT_ZOOM_IN, x0, y0, wh, ww)
            # labels.py:271-281, 323-327: the label side keeps the un-truncated window
            zh_, zw_ = H / f, W / f
            z_x1, z_y1 = min(x0 + zw_, W - 1), min(y0 + zh_, H - 1)
            p[8:15] = _f32_bits([x0, z_x1 - 1, y0, z_y1 - 1, f, f * zw_ - 1, f * zh_ - 1])
        elif zout:
            f, x0, y0 = float(st.zoom_out.zoom_out_factor), int(st.zoom_out.x0), int(st.zoom_out.y0)
            if not f >= 1:
                raise ValueError(f"sast_amd.augment: zoom-out factor {f} must be >= 1")
            wh, ww = int(H / f), int(W / f)
            if wh < 1 or ww < 1 or x0 < 0 or y0 < 0 or x0 + ww > W or y0 + wh > H:
                raise ValueError(f"sast_amd.augment: zoom-out window {wh}x{ww} at ({x0}, {y0}) does not fit the {H}x{W} frame")
            p[1:6] = (L.AUGMENT_ZOOM_OUT, x0, y0, wh, ww)
            s = 1 / f                                                      # labels.py:306, 323-327
            p[12:15] = _f32_bits([s, s * W - 1, s * H - 1])
        return p

    def _encode_rotation(self, st: AugmentationState) -> np.ndarray:
        if not st.rotation.active:
            return np.zeros(L.ROTAUG_PARAM_WORDS, dtype=np.int32)
        angle = float(st.rotation.angle_deg)
        if not math.isfinite(angle):
            raise ValueError(f"sast_amd.augment: rotation angle {angle} must be finite")
        return _rotation_words(angle, *self.hw_tuple)

    def _upload(self):
        if self.params is not None:
            self.params.copy_(torch.from_numpy(self._host))   # stream-ordered: later launches and graph replays see the new rows
        if self.rotation and self.rot_params is not None:
            self.rot_params.copy_(torch.from_numpy(self._rot_host))

    def _device_params(self, dev) -> torch.Tensor:
        if self._joined is not None:
            self._joined._device_params(dev)                  # this part's params are its rows of the joined tensor
            return self.params
        if self.params is None or self.params.device != dev:
            not_capturing("augment")
            self.params = torch.from_numpy(self._host).to(dev)
            self.rot_params = torch.from_numpy(self._rot_host).to(dev) if self.rotation else None
        return self.params

    # --------------------------------------------------------------------------------------------------------------------- call
    def __call__(self, frames: torch.Tensor, labels: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                 yolox: bool = False, out: Optional[torch.Tensor] = None):
        _need_gpu(frames, labels, counts, out)
        H, W = self.hw_tuple
        B = self.batch_size
        if frames.dtype not in (torch.uint8, torch.int8) or frames.dim() not in (4, 5):
            raise TypeError("sast_amd.augment: frames must be uint8 or int8 [T, B, C, H, W] or [B, C, H, W]")
        if tuple(frames.shape[-2:]) != (H, W) or frames.shape[-4] != B:
            raise ValueError(f"sast_amd.augment: frames of shape {tuple(frames.shape)} do not match batch {B} of {H}x{W} frames")
        if (labels is None) != (counts is None):
            raise ValueError("sast_amd.augment: give labels and counts together")
        frames = frames.contiguous()
        N, Cc = frames.numel() // (frames.shape[-3] * H * W), frames.shape[-3]
        if N < 1:
            raise ValueError("sast_amd.augment: no frames")
        if out is None:
            out = torch.empty_like(frames)
        elif out.shape != frames.shape or out.dtype != frames.dtype or not out.is_contiguous() or out.device != frames.device:
            raise ValueError("sast_amd.augment: out must be a contiguous tensor of the frames' dtype and shape on their device")
        elif out.data_ptr() == frames.data_ptr():
            raise ValueError("sast_amd.augment: out must not be the input (the gather is not in place)")
        params = self._device_params(frames.device)
        rot = self.rot_params.data_ptr() if self.rotation else None      # made beside params; the kernels are chosen by the flag alone
        if self.rotation:
            L.check(L.lib().sast_rotaug_frames(frames.data_ptr(), out.data_ptr(), params.data_ptr(), rot, N, B, Cc, H, W, _stream()),
                    "rotaug_frames")
        else:
            L.check(L.lib().sast_augment_frames(frames.data_ptr(), out.data_ptr(), params.data_ptr(), N, B, Cc, H, W, _stream()),
                    "augment_frames")
        if labels is None:
            return out
        if labels.dtype != torch.float32 or labels.dim() < 3 or labels.shape[-1] != 7 or labels.shape[-3] != B:
            raise TypeError("sast_amd.augment: labels must be fp32 [T, B, M, 7] or [B, M, 7]")
        if counts.dtype != torch.int32 or counts.shape != labels.shape[:-2]:
            raise TypeError("sast_amd.augment: counts must be int32 with the labels' leading shape")
        same_device("augment", "frames, labels and counts", frames, labels, counts)
        labels, counts = labels.contiguous(), counts.contiguous()
        M = labels.shape[-2]
        NL = counts.numel()
        if M < 1 or NL < 1:
            raise ValueError("sast_amd.augment: labels need at least one row per frame")
        lab_out = torch.empty_like(labels)
        cnt_out = torch.empty_like(counts)
        head = torch.empty(labels.shape[:-1] + (5,), dtype=torch.float32, device=labels.device) if yolox else None
        head_ptr = None if head is None else head.data_ptr()
        if self.rotation:
            L.check(L.lib().sast_rotaug_labels(labels.data_ptr(), counts.data_ptr(), params.data_ptr(), rot, NL, B, M, H, W,
                                               lab_out.data_ptr(), cnt_out.data_ptr(), head_ptr, _stream()), "rotaug_labels")
        else:
            L.check(L.lib().sast_augment_labels(labels.data_ptr(), counts.data_ptr(), params.data_ptr(), NL, B, M, W, lab_out.data_ptr(),
                                                cnt_out.data_ptr(), head_ptr, _stream()), "augment_labels")
        self.last_labels = lab_out
        return out, (head if yolox else lab_out), cnt_out


class JoinedAugmentor:
    """One augment call for a batch whose parts are drawn by different configurations.

    The reference augments the streamed rows of a mixed batch with `data_augmentation.stream` (one draw per sub-sequence) and the
    random-access rows with `data_augmentation.random` (one draw per item, with zoom-in), each in its own loader, before
    merge_mixed_batches concatenates them.  The kernels read per-sample parameters as params[n % B], so only the host side is needed:

    joined = JoinedAugmentor([stream_aug, random_aug])       SpatialAugmentors with the same dataset_hw, in batch-column order
    stream_aug.randomize(samples=...); random_aug.randomize(latest_labels=...)      as before: draws, order and validation untouched
    frames_out, labels_out, counts_out = joined(frames, labels, counts, yolox=False, out=None)

    The joined object owns ONE host array and ONE device tensor `params` [sum B_i, AUGMENT_PARAM_WORDS], and likewise one `rot_params`
    [sum B_i, ROTAUG_PARAM_WORDS]: it rotates (uses the rotating kernels) iff any part was built with rotation=True, and the rows of the
    other parts stay inactive.  From then on
    parts[i].randomize(...) and parts[i].set_state(...) rewrite only their own rows of it, by a stream-ordered copy.  The call is
    `SpatialAugmentor.__call__` over the union batch: 2 launches (1 for frames alone), capturable after one warm-up call.  A part can
    still be called alone on a batch of its own size; it reads the same rows.  A SpatialAugmentor belongs to one JoinedAugmentor at
    most."""

    def __init__(self, parts: Sequence[SpatialAugmentor]):
        parts = list(parts)
        if not parts or not all(isinstance(p, SpatialAugmentor) for p in parts):
            raise TypeError("sast_amd.augment: JoinedAugmentor takes a non-empty sequence of SpatialAugmentors")
        if len({id(p) for p in parts}) != len(parts) or any(p._joined is not None for p in parts):
            raise ValueError("sast_amd.augment: a SpatialAugmentor can be a part of one JoinedAugmentor, once")
        if len({p.hw_tuple for p in parts}) != 1:
            raise ValueError("sast_amd.augment: the parts must have the same dataset_hw")
        self.parts = parts
        self.hw_tuple = parts[0].hw_tuple
        self.batch_size = sum(p.batch_size for p in parts)
        self.offsets = [sum(p.batch_size for p in parts[:i]) for i in range(len(parts))]
        self.rotation = any(p.rotation for p in parts)
        self._host = np.concatenate([p._host for p in parts])
        self._rot_host = np.concatenate([p._rot_host for p in parts])
        self.params: Optional[torch.Tensor] = None
        self.rot_params: Optional[torch.Tensor] = None
        for p, o in zip(parts, self.offsets):
            p._host = self._host[o:o + p.batch_size]          # a view: the part's draws land in the joined array
            p._rot_host = self._rot_host[o:o + p.batch_size]
            p.params = p.rot_params = None
            p._joined = self

    @property
    def states(self) -> List[AugmentationState]:
        return [s for p in self.parts for s in p.states]

    def _device_params(self, dev) -> torch.Tensor:
        if self.params is None or self.params.device != dev:
            not_capturing("augment")
            self.params = torch.from_numpy(self._host).to(dev)
            self.rot_params = torch.from_numpy(self._rot_host).to(dev) if self.rotation else None
            for p, o in zip(self.parts, self.offsets):
                p.params = self.params[o:o + p.batch_size]    # a contiguous view: the part's uploads rewrite its rows only
                p.rot_params = self.rot_params[o:o + p.batch_size] if p.rotation else None
        return self.params

    def __call__(self, frames: torch.Tensor, labels: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                 yolox: bool = False, out: Optional[torch.Tensor] = None):
        return SpatialAugmentor.__call__(self, frames, labels, counts, yolox, out)

    joined = __call__
