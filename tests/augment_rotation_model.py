"""A numpy model of the augmentation with rotation (sast_amd/augment.py with rotation=True, csrc/k_rotaug.hip): the contract the GPU
tests hold the kernels to, fp32 one operation at a time (numpy float32 arithmetic never fuses a product into a sum).

A state is (flip, mode, factor, x0, y0, angle_deg): the first five as in tests/golden/make_golden_augment.py ("none" / "in" / "out" /
"in_nolabels"), angle_deg None for no rotation.  The order is the reference's (data/utils/augmentor.py:355-363): flip, rotate, zoom.

  rotation_matrix(angle_deg, H, W)   the host side of the frame rule: a, b, c, d as fp32
  rotation_src(angle_deg, H, W)      sy, sx int64 [H, W] and inside bool [H, W]: the source pixel of every pixel of the rotated image
  frame_map(state, H, W)             int64 [H, W]: offset of the source pixel in its plane, -1 where the output is 0
  apply_map(frames, fmap)            frames [..., H, W] (any 1-byte dtype) gathered through the map
  frames(x, states)                  x [T, B, C, H, W] -> the augmented batch
  labels(rows, state, H, W)          rows fp32 [k, 7] -> the surviving rows after flip_lr_, rotate_, the zoom transform
  batch_labels(lab, cnt, states, H, W)   [T, B, M, 7], [T, B] -> labels, counts, yolox as the label kernel lays them out
"""
import math

import numpy as np

f32 = np.float32


# ---- frames ------------------------------------------------------------------------------------------------------------------------

def rotation_matrix(angle_deg, H, W):
    """torchvision.transforms.functional.rotate (center=None) -> _get_inverse_affine_matrix([0, 0], -angle, ...) -> _gen_affine_grid:
    theta (fp32) divided by [0.5 w, 0.5 h] in fp32"""
    r = math.radians(-angle_deg)
    m = [f32(math.cos(r)), f32(math.sin(r)), f32(-math.sin(r)), f32(math.cos(r))]
    hw, hh = f32(0.5 * W), f32(0.5 * H)
    return m[0] / hw, m[1] / hw, m[2] / hh, m[3] / hh


def rotation_src(angle_deg, H, W):
    a, b, c, d = rotation_matrix(angle_deg, H, W)
    x = np.arange(W, dtype=f32)[None, :]
    y = np.arange(H, dtype=f32)[:, None]
    bx = x + (f32(0.5) - f32(0.5) * f32(W))
    by = y + (f32(0.5) - f32(0.5) * f32(H))
    gx = (bx * a) + (by * b)
    gy = (bx * c) + (by * d)
    assert gx.dtype == f32 and gy.dtype == f32
    ix = (((gx + f32(1)) * f32(W)) - f32(1)) / f32(2)
    iy = (((gy + f32(1)) * f32(H)) - f32(1)) / f32(2)
    sx, sy = np.rint(ix), np.rint(iy)                       # ties to even
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    return np.where(inside, sy, 0).astype(np.int64), np.where(inside, sx, 0).astype(np.int64), inside


def nearest_exact(d, in_, out):
    """ATen's nearest-exact source index in fp32: min(int(floor((d + 0.5) * (in / out))), in - 1)"""
    scale = f32(in_) / f32(out)
    return np.minimum(np.floor((d.astype(f32) + f32(0.5)) * scale).astype(np.int64), in_ - 1)


def axis_src(full, mode, o0, win):
    """int64 [full]: the source index of every output index of one axis, -1 on the border of zoom-out"""
    d = np.arange(full, dtype=np.int64)
    if mode == "in":
        return o0 + nearest_exact(d, min(win, full - o0), full)
    if mode == "out":
        s = np.full(full, -1, dtype=np.int64)
        s[o0:o0 + win] = nearest_exact(d[:win], full, win)
        return s
    return d


def frame_map(state, H, W):
    flip, mode, f, x0, y0, angle = state
    if mode in ("in", "out") and f != 1:
        wh, ww = int(H / f), int(W / f)
    else:
        mode, wh, ww = "none", H, W
    sy = np.broadcast_to(axis_src(H, mode, y0, wh)[:, None], (H, W))
    sx = np.broadcast_to(axis_src(W, mode, x0, ww)[None, :], (H, W))
    ok = (sy >= 0) & (sx >= 0)
    sy, sx = np.where(ok, sy, 0), np.where(ok, sx, 0)
    if angle is not None:
        ry, rx, inside = rotation_src(angle, H, W)
        ok = ok & inside[sy, sx]
        sy, sx = ry[sy, sx], rx[sy, sx]
    if flip:
        sx = W - 1 - sx
    return np.where(ok, sy * W + sx, -1)


def apply_map(frames, fmap):
    H, W = fmap.shape
    flat = frames.reshape(frames.shape[:-2] + (H * W,))
    out = np.where(fmap.reshape(-1) >= 0, flat[..., np.maximum(fmap.reshape(-1), 0)], 0).astype(frames.dtype)
    return out.reshape(frames.shape)


def frames(x, states):
    """x [T, B, C, H, W] -> augmented, sample b by states[b]"""
    out = np.empty_like(x)
    H, W = x.shape[-2:]
    for b, st in enumerate(states):
        out[:, b] = apply_map(x[:, b], frame_map(st, H, W))
    return out


# ---- labels ------------------------------------------------------------------------------------------------------------------------

def _flat(x, y, w, h, rest):
    keep = (w > 0) & (h > 0)
    return x[keep], y[keep], w[keep], h[keep], rest[keep]


def rotate_boxes(x, y, w, h, angle_deg, H, W):
    """ObjectLabels.rotate_ (data/genx_utils/labels.py:217-246) without remove_flat_labels_: the plain (unfused) form of the einsum"""
    a = angle_deg / 180 * math.pi
    co, si, nsi = f32(math.cos(a)), f32(math.sin(a)), f32(-math.sin(a))
    cx, cy = f32(W // 2), f32(H // 2)
    xs, ys = [], []
    for X, Y in ((x, y), (x + w, y), (x, y + h), (x + w, y + h)):
        px, py = X - cx, Y - cy
        xs.append(((co * px) + (si * py)) + cx)
        ys.append(((nsi * px) + (co * py)) + cy)
    x0 = np.clip(np.min(xs, axis=0), f32(0), f32(W - 1))
    x1 = np.clip(np.max(xs, axis=0), f32(0), f32(W - 1))
    y0 = np.clip(np.min(ys, axis=0), f32(0), f32(H - 1))
    y1 = np.clip(np.max(ys, axis=0), f32(0), f32(H - 1))
    return x0, y0, x1 - x0, y1 - y0


def labels(rows, state, H, W):
    flip, mode, f, zx0, zy0, angle = state
    rows = np.asarray(rows, dtype=f32)
    x, y, w, h = (rows[:, i].copy() for i in (1, 2, 3, 4))
    rest = rows[:, [0, 5, 6]]
    if flip:                                                                      # labels.py:339
        x = (f32(W - 1) - x) - w
    if angle is not None and len(x):
        x, y, w, h = rotate_boxes(x, y, w, h, angle, H, W)
        x, y, w, h, rest = _flat(x, y, w, h, rest)
    s = None
    if mode == "in" and f != 1:                                                   # labels.py:267-291
        zh, zw = H / f, W / f
        zx1, zy1 = min(zx0 + zw, W - 1), min(zy0 + zh, H - 1)
        lox, hix, loy, hiy = f32(zx0), f32(zx1 - 1), f32(zy0), f32(zy1 - 1)
        cx0, cy0 = np.minimum(np.maximum(x, lox), hix), np.minimum(np.maximum(y, loy), hiy)
        cx1, cy1 = np.minimum(np.maximum(x + w, lox), hix), np.minimum(np.maximum(y + h, loy), hiy)
        x, y, w, h = cx0 - f32(zx0), cy0 - f32(zy0), cx1 - cx0, cy1 - cy0
        x, y, w, h, rest = _flat(x, y, w, h, rest)
        s, ht, wd = f, zh, zw
    elif mode == "out" and f != 1:                                                # labels.py:305-306
        s, ht, wd = 1 / f, H, W
    if s is not None:                                                             # scale_: labels.py:322-334
        sc, maxx, maxy = f32(s), f32(s * wd - 1), f32(s * ht - 1)
        x1, y1 = np.minimum((x + w) * sc, maxx), np.minimum((y + h) * sc, maxy)
        x, y = x * sc, y * sc
        w, h = x1 - x, y1 - y
        x, y, w, h, rest = _flat(x, y, w, h, rest)
        if mode == "out":                                                         # labels.py:313-314
            x, y = x + f32(zx0), y + f32(zy0)
    out = np.zeros((len(x), 7), dtype=f32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4], out[:, 5], out[:, 6] = rest[:, 0], x, y, w, h, rest[:, 1], rest[:, 2]
    return out


def batch_labels(lab, cnt, states, H, W):
    T, B, M, _ = lab.shape
    out, n, head = np.zeros_like(lab), np.zeros_like(cnt), np.zeros((T, B, M, 5), dtype=f32)
    for t in range(T):
        for b in range(B):
            r = labels(lab[t, b, :cnt[t, b]], states[b], H, W)
            k = len(r)
            out[t, b, :k], n[t, b] = r, k
            head[t, b, :k, 0] = r[:, 5]                                           # labels.py:348-352
            head[t, b, :k, 1], head[t, b, :k, 2] = r[:, 1] + f32(0.5) * r[:, 3], r[:, 2] + f32(0.5) * r[:, 4]
            head[t, b, :k, 3], head[t, b, :k, 4] = r[:, 3], r[:, 4]
    return out, n, head
