"""Fixtures of the augmentation with rotation (sast_amd/augment.py, rotation=True):
`python tests/golden/make_golden_augment_rotation.py` -> augment_rotation.npz.

Every expected value comes from the reference's own RandomSpatialAugmentorGenX.__call__ (data/utils/augmentor.py), driven the way
make_golden_augment.py drives it, with `augm_state.rotation` set as well.  The reference rotates frames with
torchvision.transforms.functional.rotate(interpolation=NEAREST); torchvision is not installed, so `torch_rotate` below stands in for
it: the tensor path of that function restated with torch alone (the inverse affine matrix, the linspace base grid, theta divided by
the half sizes, bmm, grid_sample(nearest, zeros, align_corners=False)).  Labels go through the reference's ObjectLabels.rotate_
untouched.  So the fixture pins the order of operations (flip, rotate, zoom) and the labels through the reference's code, and the frame
rule through the restatement.

Three parts:
  cases      frames (small geometries, stored whole), labels, counts and the head's layout for explicit states
  big        one frame of 64 boxes: torch's einsum takes a fused form there, so the kernel is held to it within a tolerance only
  rng        consecutive seeded draws of the reference with rotate.prob 0.5 and angles 2..6 (flip, rotation, zoom, windows)
The generator asserts that every keep / remove decision has make_golden_augment.FLAT_MARGIN, that the reference's labels equal
tests/augment_rotation_model.py bit for bit on the frames of at most 6 boxes, and that the stored frames equal that model.
Inputs are not stored: they come from make_golden_augment's integer hash.
"""
from __future__ import annotations

import math
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_augment as G  # noqa: E402
import augment_rotation_model as M  # noqa: E402

OUT = os.path.join(HERE, "augment_rotation.npz")
M_ROWS = G.M_ROWS
GEOMS = {"a": (3, 45, 80), "b": (3, 60, 76), "c": (3, 33, 47)}       # W % 16 == 0, W % 4 == 0, odd
BIG = dict(geom="b", boxes=64, seed=77, state=(1, "out", 1.1, 3, 2, 3.7))
RNG_CONFIG = {
    "random": dict(prob_hflip=0.5, rotate=dict(prob=0.5, min_angle_deg=2, max_angle_deg=6),
                   zoom=dict(prob=0.8, zoom_in=dict(weight=8, factor=dict(min=1, max=1.5)),
                             zoom_out=dict(weight=2, factor=dict(min=1, max=1.2)))),
    "stream": dict(prob_hflip=0.5, rotate=dict(prob=0.5, min_angle_deg=2, max_angle_deg=6),
                   zoom=dict(prob=0.5, zoom_out=dict(factor=dict(min=1, max=1.2)))),
}
RNG_SEEDS = G.RNG_SEEDS
RNG_DRAWS = G.RNG_DRAWS
RNG_HW = G.RNG_HW


def cases():
    """a state is (flip, mode, factor, x0, y0, angle_deg), angle_deg None: rotation inactive"""
    out = []
    for i, g in enumerate(GEOMS):
        _C, H, W = GEOMS[g]
        ih, iw = int(H / 1.3), int(W / 1.3)
        oh, ow = int(H / 1.15), int(W / 1.15)
        out.append(dict(name=f"{g}_combos", geom=g, T=1, seed=31 + i, states=[
            (0, "none", 1.0, 0, 0, 3.7), (0, "none", 1.0, 0, 0, -6.0), (1, "none", 1.0, 0, 0, 2.0), (0, "none", 1.0, 0, 0, None),
            (0, "in", 1.3, (W - iw) // 3, (H - ih) // 2, -4.25), (1, "in", 1.3, (W - iw) // 2, (H - ih) // 3, 6.0),
            (0, "out", 1.15, (W - ow) // 2, (H - oh) // 3, 17.3), (1, "out", 1.15, (W - ow) // 3, (H - oh) // 2, -2.0)]))
    # T > 1 with B > 1, active and inactive rows mixed, label frames missing at some steps
    out.append(dict(name="b_seq", geom="b", T=2, seed=35, states=[(1, "in", 1.45, 20, 15, 5.0), (0, "out", 1.2, 5, 2, None),
                                                                  (1, "none", 1.0, 0, 0, -3.0)], counts=[[6, 0, 3], [2, 6, 0]]))
    # quarter and half turns: every pixel on an exact tie (90 on an even width), the whole frame kept (180), and the identity
    out.append(dict(name="a_turns", geom="a", T=1, seed=36, states=[(0, "none", 1.0, 0, 0, 90.0), (1, "none", 1.0, 0, 0, -90.0),
                                                                    (0, "none", 1.0, 0, 0, 180.0), (1, "none", 1.0, 0, 0, 0.0)]))
    return out


def case_inputs(case):
    """-> frames uint8 [T, B, C, H, W], labels fp32 [T, B, M_ROWS, 7] (zero after the count), counts int32 [T, B]"""
    C, H, W = GEOMS[case["geom"]]
    T, B = case["T"], len(case["states"])
    fr = G.frames(case["seed"], (T, B, C, H, W))
    counts = np.zeros((T, B), dtype=np.int32)
    labels = np.zeros((T, B, M_ROWS, 7), dtype=np.float32)
    pattern = (3, 6, 1, 5, 2, 4)
    for t in range(T):
        for b in range(B):
            k = case["counts"][t][b] if "counts" in case else pattern[(t + b) % len(pattern)]
            counts[t, b] = k
            labels[t, b, :k] = G.boxes(case["seed"] * 1000 + t * 37 + b, k, H, W, t=float(t))
    return fr, labels, counts


def big_inputs():
    C, H, W = GEOMS[BIG["geom"]]
    k = BIG["boxes"]
    lab = np.zeros((1, 1, k + 4, 7), dtype=np.float32)
    lab[0, 0, :k] = G.boxes(BIG["seed"], k, H, W)
    return G.frames(BIG["seed"], (1, 1, C, H, W)), lab, np.full((1, 1), k, dtype=np.int32)


# ---- torchvision's tensor rotate, restated ------------------------------------------------------------------------------------------

def rotation_grid(angle, H, W):
    """the sampling grid of torchvision.transforms.functional.rotate(img [.., H, W], angle) with expand=False, center=None:
    _get_inverse_affine_matrix([0, 0], -angle, [0, 0], 1, [0, 0]) -> _gen_affine_grid -> fp32 [1, H, W, 2]"""
    import torch
    r = math.radians(-angle)
    theta = torch.tensor([math.cos(r), math.sin(r), 0.0, -math.sin(r), math.cos(r), 0.0], dtype=torch.float32).reshape(1, 2, 3)
    d = 0.5
    base = torch.empty(1, H, W, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + d, W * 0.5 + d - 1, steps=W))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + d, H * 0.5 + d - 1, steps=H).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float32)
    return base.view(1, H * W, 3).bmm(rescaled).view(1, H, W, 2)


def torch_rotate(img, angle, interpolation=None, **_kw):
    """_apply_grid_transform: to float, grid_sample(nearest, zeros, align_corners=False), round, back to the image's dtype"""
    import torch
    H, W = img.shape[-2:]
    x = img.reshape(-1, H, W).unsqueeze(0).to(torch.float32)
    y = torch.nn.functional.grid_sample(x, rotation_grid(angle, H, W), mode="nearest", padding_mode="zeros", align_corners=False)
    return torch.round(y[0]).to(img.dtype).reshape(img.shape)


def _import_reference():
    ns = G._import_reference()
    ns.aug.rotate = torch_rotate                      # in place of the stub that raises
    return ns


# ---- the reference -------------------------------------------------------------------------------------------------------------------

def _run(ns, fr, labels, counts, states, H, W, stats):
    import torch
    T, B = counts.shape
    Mr = labels.shape[2]
    out_fr = np.zeros_like(fr)
    out_lab, out_cnt, out_head = np.zeros_like(labels), np.zeros_like(counts), np.zeros((T, B, Mr, 5), dtype=np.float32)
    for b, state in enumerate(states):
        flip, mode, f, x0, y0, angle = state
        a = ns.aug.RandomSpatialAugmentorGenX((H, W), False, ns.to_cfg(G._case_config(state[:5])))
        a.augm_state.apply_h_flip = bool(flip)
        a.augm_state.rotation = ns.aug.RotationState(active=angle is not None, angle_deg=0.0 if angle is None else float(angle))
        a.augm_state.apply_zoom_in = mode.startswith("in")
        a.augm_state.zoom_out = ns.aug.ZoomOutState(active=mode == "out", x0=x0, y0=y0, zoom_out_factor=f)
        objs = [ns.ObjectLabels(torch.from_numpy(labels[t, b, :counts[t, b]].copy()), (H, W)) if counts[t, b] else None for t in range(T)]
        data = {ns.DataType.EV_REPR: [torch.from_numpy(fr[t, b].copy()) for t in range(T)], ns.DataType.OBJLABELS_SEQ: ns.Sparse(objs)}
        sampler = ns.aug.randomly_sample_zoom_window_from_objframe
        ns.aug.randomly_sample_zoom_window_from_objframe = lambda objframe, zoom_window_height, zoom_window_width: (x0, y0)
        try:
            with warnings.catch_warnings(), G._flat_label_margin(ns, stats):
                warnings.simplefilter("ignore")
                res = a(data)
        finally:
            ns.aug.randomly_sample_zoom_window_from_objframe = sampler
        valid, where = [], []
        for t in range(T):
            o = res[ns.DataType.EV_REPR][t]
            assert o.dtype == torch.uint8 and tuple(o.shape) == fr.shape[2:]
            out_fr[t, b] = o.numpy()
            lab = res[ns.DataType.OBJLABELS_SEQ][t]
            if lab is not None and len(lab) > 0:
                k = len(lab)
                out_lab[t, b, :k] = lab.object_labels.numpy()
                out_cnt[t, b] = k
                valid.append(lab)
                where.append(t)
        if valid:
            head = ns.ObjectLabels.get_labels_as_batched_tensor(valid, format_='yolox').numpy()
            for i, t in enumerate(where):
                out_head[t, b, :head.shape[1]] = head[i]
    return out_fr, out_lab, out_cnt, out_head


def reference_rng(ns, which: str, seed: int):
    """RNG_DRAWS consecutive states of the reference after torch.manual_seed(seed), as make_golden_augment.reference_rng draws them.
    -> ints [n, 9] (flip, zoom-in chosen, zoom-in applied, its x0, y0, zoom-out active, its x0, y0, rotation active),
    floats [n, 3] (zoom-in factor, zoom-out factor, angle_deg; 1, 1, 0 where not active)"""
    import torch
    H, W = RNG_HW
    seen = {}
    orig = ns.aug.RandomSpatialAugmentorGenX._zoom_in_and_rescale_recursive.__func__

    def spy(cls, input_, zoom_coordinates_x0y0, zoom_in_factor, datatype):
        seen["x0y0"], seen["f"] = zoom_coordinates_x0y0, zoom_in_factor
        return orig(cls, input_, zoom_coordinates_x0y0=zoom_coordinates_x0y0, zoom_in_factor=zoom_in_factor, datatype=datatype)

    ns.aug.RandomSpatialAugmentorGenX._zoom_in_and_rescale_recursive = classmethod(spy)
    ints, floats = np.zeros((RNG_DRAWS, 9), dtype=np.int64), np.ones((RNG_DRAWS, 3), dtype=np.float64)
    try:
        torch.manual_seed(seed)
        a = ns.aug.RandomSpatialAugmentorGenX((H, W), which == "random", ns.to_cfg(RNG_CONFIG[which]))
        for i in range(RNG_DRAWS):
            lab = G.rng_labels(i)
            objs = [ns.ObjectLabels(torch.from_numpy(lab.copy()), (H, W)) if lab is not None else None]
            data = {ns.DataType.EV_REPR: [torch.zeros(1, H, W, dtype=torch.uint8)], ns.DataType.OBJLABELS_SEQ: ns.Sparse(objs)}
            seen.clear()
            if which == "stream":
                a.randomize_augmentation()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                a(data)
            st = a.augm_state
            ints[i] = (st.apply_h_flip, st.apply_zoom_in, "f" in seen, *(seen.get("x0y0", (0, 0))), st.zoom_out.active,
                       st.zoom_out.x0 if st.zoom_out.active else 0, st.zoom_out.y0 if st.zoom_out.active else 0, st.rotation.active)
            floats[i] = (seen.get("f", 1.0), st.zoom_out.zoom_out_factor if st.zoom_out.active else 1.0,
                         st.rotation.angle_deg if st.rotation.active else 0.0)
    finally:
        ns.aug.RandomSpatialAugmentorGenX._zoom_in_and_rescale_recursive = classmethod(orig)
    return ints, floats


def generate():
    import torch
    ns = _import_reference()
    fx = {"torch_version": np.array(torch.__version__)}
    stats = {"removed": 0, "emptied": 0}
    for case in cases():
        _C, H, W = GEOMS[case["geom"]]
        fr, lab, cnt = case_inputs(case)
        o_fr, o_lab, o_cnt, o_head = _run(ns, fr, lab, cnt, case["states"], H, W, stats)
        n = case["name"]
        fx[f"{n}/frames"], fx[f"{n}/labels"], fx[f"{n}/counts"], fx[f"{n}/yolox"] = o_fr, o_lab, o_cnt, o_head
        assert np.array_equal(o_fr, M.frames(fr, case["states"])), f"{n}: the restated rotate and the model pick different pixels"
        m_lab, m_cnt, m_head = M.batch_labels(lab, cnt, case["states"], H, W)
        assert np.array_equal(o_cnt, m_cnt), n
        assert np.array_equal(o_lab.view(np.int32), m_lab.view(np.int32)), f"{n}: the reference's labels are not the model's bit for bit"
        assert np.array_equal(o_head.view(np.int32), m_head.view(np.int32)), n
    assert stats["removed"] >= 3, stats
    _C, H, W = GEOMS[BIG["geom"]]
    fr, lab, cnt = big_inputs()
    _f, o_lab, o_cnt, o_head = _run(ns, fr, lab, cnt, [BIG["state"]], H, W, stats)
    fx["big/labels"], fx["big/counts"], fx["big/yolox"] = o_lab, o_cnt, o_head
    m_lab, m_cnt, _h = M.batch_labels(lab, cnt, [BIG["state"]], H, W)
    assert np.array_equal(o_cnt, m_cnt) and np.abs(o_lab.astype(np.float64) - m_lab.astype(np.float64)).max() <= 1e-3
    for which in RNG_CONFIG:
        rotated = 0
        for seed in RNG_SEEDS:
            ints, floats = reference_rng(ns, which, seed)
            fx[f"rng/{which}/{seed}/ints"], fx[f"rng/{which}/{seed}/floats"] = ints, floats
            rotated += int(ints[:, 8].sum())
            assert {(int(r[8]), int(r[2])) for r in ints} >= ({(0, 0), (1, 0), (0, 1), (1, 1)} if which == "random" else {(0, 0), (1, 0)})
        assert 0.35 * 3 * RNG_DRAWS < rotated < 0.65 * 3 * RNG_DRAWS
    return fx


if __name__ == "__main__":
    fixtures = generate()
    np.savez_compressed(OUT, **fixtures)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(fixtures)} arrays")
