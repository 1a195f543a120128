"""Fixtures of the spatial augmentation (sast_amd/augment.py): `python tests/golden/make_golden_augment.py` -> augment.npz.

Every expected value comes from the reference's own RandomSpatialAugmentorGenX.__call__ (data/utils/augmentor.py) on
{EV_REPR: [frames], OBJLABELS_SEQ: SparselyBatchedObjectLabels([...])}, imported from the reference root that `_ref_import.py` names.
The reference imports torchvision.transforms at module scope (rotation only); it is not installed, so a stub stands in and rotation is
never exercised.  Explicit states go in the way the reference takes them: flip and zoom-out through `augm_state`; the zoom-in factor
through a config whose factor.min == factor.max (no draw then), the zoom-in window by replacing the module's window sampler
`randomly_sample_zoom_window_from_objframe` for the call (the reference keeps that window in locals only).

Inputs are not stored: frames and boxes are regenerated from a small integer hash, so the GPU tests rebuild them without the
reference.  Small geometries are stored whole; full-size frames as the sha256 of their bytes plus per-channel sums.

The random-state fixture records consecutive seeded draws of the reference (flip, zoom decision, factors, windows) with the torch
version that drew them: it pins torch's CPU generator stream together with the order of the reference's calls.
"""
from __future__ import annotations

import contextlib
import enum
import hashlib
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "augment.npz")

_M64 = (1 << 64) - 1
M_ROWS = 8          # label rows per frame in every case: more than any count
GEOMS = {"s1": (4, 45, 80), "s2": (20, 60, 76), "gen1": (20, 240, 304), "gen4": (20, 360, 640), "ev": (20, 128, 160)}
# the end-to-end cases: frames built from raw events (make_golden_events.stream / reference_frames), two windows = two samples
EVENTS = dict(stream=dict(seed=51, n=12000, height=128, width=160, t_step=2, jitter=8),
              frames=dict(height=128, width=160, bins=10, count_cutoff=10, duration_us=10000))
SHIPPED = {
    # config/dataset/base.yaml:12-41
    "random": dict(prob_hflip=0.5, rotate=dict(prob=0, min_angle_deg=2, max_angle_deg=6),
                   zoom=dict(prob=0.8, zoom_in=dict(weight=8, factor=dict(min=1, max=1.5)),
                             zoom_out=dict(weight=2, factor=dict(min=1, max=1.2)))),
    "stream": dict(prob_hflip=0.5, rotate=dict(prob=0, min_angle_deg=2, max_angle_deg=6),
                   zoom=dict(prob=0.5, zoom_out=dict(factor=dict(min=1, max=1.2)))),
}
RNG_SEEDS = (0, 1, 2)
RNG_DRAWS = 240
RNG_HW = (240, 304)


def _hash(seed: int, n: int, salt: int) -> np.ndarray:
    """splitmix64 of (seed, salt, index): n uint64 values"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x1000193 + salt * 0x9E3779B1) & _M64)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def frames(seed: int, shape) -> np.ndarray:
    """uint8 event frames: about one pixel in 12 holds a count 1..10, the rest 0"""
    n = int(np.prod(shape))
    h = _hash(seed, n, 1)
    on = (h % np.uint64(12)) == 0
    return np.where(on, 1 + (h >> np.uint64(20)) % np.uint64(10), 0).astype(np.uint8).reshape(shape)


def boxes(seed: int, k: int, H: int, W: int, t: float = 0.0) -> np.ndarray:
    """k label rows (t, x, y, w, h, class_id, class_confidence), fp32, inside the frame, on a 1/8 px grid"""
    out = np.zeros((k, 7), dtype=np.float32)
    hx, hy, hw, hh, hc = (_hash(seed, k, s) for s in (11, 12, 13, 14, 15))
    w = 3 + (hw % np.uint64(8 * (W // 3))).astype(np.float64) / 8
    h = 3 + (hh % np.uint64(8 * (H // 3))).astype(np.float64) / 8
    x = (hx % np.uint64(1 << 20)).astype(np.float64) / (1 << 20) * (W - 2 - w)
    y = (hy % np.uint64(1 << 20)).astype(np.float64) / (1 << 20) * (H - 2 - h)
    out[:, 0] = t
    out[:, 1], out[:, 2] = np.round(x * 8) / 8, np.round(y * 8) / 8
    out[:, 3], out[:, 4] = w, h
    out[:, 5] = (hc % np.uint64(3)).astype(np.float32)
    out[:, 6] = 1.0
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
# a state is (flip, mode, factor, x0, y0), mode one of "none" / "in" / "out" / "in_nolabels" (zoom-in chosen, no label frame: the
# reference warns and does not zoom)

def _win(H, W, f):
    return int(H / f), int(W / f)


def cases():
    out = []
    for g in ("s1", "s2", "gen1", "gen4"):
        C, H, W = GEOMS[g]
        ih, iw = _win(H, W, 1.3)
        oh, ow = _win(H, W, 1.15)
        out.append(dict(name=f"{g}_combos", geom=g, T=1, seed=1, states=[
            (0, "none", 1.0, 0, 0), (1, "none", 1.0, 0, 0),
            (0, "in", 1.3, (W - iw) // 3, (H - ih) // 2), (1, "in", 1.3, (W - iw) // 2, (H - ih) // 3),
            (0, "out", 1.15, (W - ow) // 2, (H - oh) // 3), (1, "out", 1.15, (W - ow) // 3, (H - oh) // 2)]))
    for g in ("s1", "s2"):
        C, H, W = GEOMS[g]
        ih, iw = _win(H, W, 1.5)
        oh, ow = _win(H, W, 1.2)
        # both ends of the shipped factor ranges, and factors of exactly 1
        out.append(dict(name=f"{g}_ends", geom=g, T=1, seed=2, states=[
            (0, "in", 1.5, 3, 2), (1, "in", 1.0, 5, 4), (1, "out", 1.2, 4, 3), (0, "out", 1.0, 0, 0),
            (1, "in", 1.5, W - iw, H - ih), (0, "in", 1.01, 0, 0)]))
        # windows at all four frame edges (corners) for zoom-out, both far corners for zoom-in
        out.append(dict(name=f"{g}_edges", geom=g, T=1, seed=3, states=[
            (0, "out", 1.2, 0, 0), (1, "out", 1.2, W - ow, 0), (0, "out", 1.2, 0, H - oh), (1, "out", 1.2, W - ow, H - oh),
            (1, "in", 1.5, 0, 0), (0, "in", 1.5, W - iw, H - ih)]))
        # zoom-in crops cut by the frame edge, down to a 1 x 1 canvas; zoom-in without any label frame
        out.append(dict(name=f"{g}_cut", geom=g, T=1, seed=4, states=[
            (0, "in", 1.5, W - iw // 2, H - ih // 2), (1, "in", 1.25, W - 7, 3), (0, "in", 1.4, 2, H - 5), (1, "in", 1.5, W - 1, H - 1),
            (1, "in_nolabels", 1.3, 0, 0)]))
    # T > 1 with B > 1, different parameters per sample, label frames missing at some steps, a frame that loses all its boxes
    C, H, W = GEOMS["s1"]
    out.append(dict(name="s1_seq", geom="s1", T=3, seed=5, states=[(1, "in", 1.5, 0, 0), (0, "out", 1.1, 3, 1), (1, "none", 1.0, 0, 0)],
                    counts=[[1, 0, 3], [0, 5, 0], [6, 6, 2]], corner_box=(0, 0)))
    C, H, W = GEOMS["s2"]
    out.append(dict(name="s2_seq", geom="s2", T=2, seed=6, states=[(0, "in", 1.45, 20, 15), (1, "out", 1.2, 5, 2)],
                    counts=[[6, 0], [3, 6]]))
    # frames from raw events, one state set per case: the graph test captures with the first and replays with the second
    out.append(dict(name="ev_a", geom="ev", T=1, seed=7, events=True, states=[(1, "in", 1.35, 30, 20), (0, "out", 1.2, 11, 9)]))
    out.append(dict(name="ev_b", geom="ev", T=1, seed=7, events=True, states=[(0, "out", 1.1, 2, 5), (1, "in", 1.5, 50, 40)]))
    for c in out:
        c["stored"] = c["geom"] in ("s1", "s2", "ev")
    return out


def event_columns():
    """-> int64 x, y, p, t of the end-to-end cases and the two window ends"""
    import make_golden_events as GE
    x, y, p, t = GE.stream(**EVENTS["stream"])
    return (x, y, p, t), [10000, int(t.max())]


def case_inputs(case):
    """-> frames uint8 [T, B, C, H, W], labels fp32 [T, B, M_ROWS, 7] (zero after the count), counts int32 [T, B]"""
    C, H, W = GEOMS[case["geom"]]
    T, B = case["T"], len(case["states"])
    fr = None if case.get("events") else frames(case["seed"], (T, B, C, H, W))   # from raw events: the caller builds them
    counts = np.zeros((T, B), dtype=np.int32)
    labels = np.zeros((T, B, M_ROWS, 7), dtype=np.float32)
    pattern = (3, 6, 1, 5, 2, 4)
    for t in range(T):
        for b in range(B):
            k = case["counts"][t][b] if "counts" in case else pattern[(t + b) % len(pattern)]
            if case["states"][b][1] == "in_nolabels":
                k = 0
            counts[t, b] = k
            labels[t, b, :k] = boxes(case["seed"] * 1000 + t * 37 + b, k, H, W, t=float(t))
    if "corner_box" in case:   # one box in the far corner: wholly outside a zoom-in window at the origin, so the frame loses it
        t, b = case["corner_box"]
        labels[t, b, 0, 1:5] = (W - 9.5, H - 8.25, 6.0, 5.0)
    return fr, labels, counts


# ---- the reference -------------------------------------------------------------------------------------------------------------------

def _import_reference():
    import _ref_import as R
    if not R.reference_available():
        raise RuntimeError(f"reference not found under {R.REF_ROOT}")
    sys.dont_write_bytecode = True
    R._install_stubs()
    if "torchvision.transforms" not in sys.modules:
        tv = sys.modules["torchvision"]
        tr, tf = types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")

        class InterpolationMode(enum.Enum):
            NEAREST = "nearest"

        def rotate(*a, **k):
            raise NotImplementedError("torchvision is not installed: rotation cannot be exercised")

        tr.InterpolationMode, tf.rotate, tr.functional, tv.transforms = InterpolationMode, rotate, tf, tr
        sys.modules["torchvision.transforms"], sys.modules["torchvision.transforms.functional"] = tr, tf
    if R.REF_ROOT not in sys.path:
        sys.path.insert(0, R.REF_ROOT)
    ns = types.SimpleNamespace()
    import data.utils.augmentor as aug
    from data.genx_utils.labels import ObjectLabels, SparselyBatchedObjectLabels
    from data.utils.types import DataType
    ns.aug, ns.ObjectLabels, ns.Sparse, ns.DataType, ns.to_cfg = aug, ObjectLabels, SparselyBatchedObjectLabels, DataType, R.to_cfg
    return ns


FLAT_MARGIN = 0.01


@contextlib.contextmanager
def _flat_label_margin(ns, stats):
    """every keep / remove decision of the reference's remove_flat_labels_ has a margin of FLAT_MARGIN px, or is exactly flat"""
    orig = ns.ObjectLabels.remove_flat_labels_

    def checked(self):
        for v in (self.w, self.h):
            assert bool(((v == 0) | (v.abs() >= FLAT_MARGIN)).all()), f"a box within {FLAT_MARGIN} px of flat: {v.tolist()}"
        n = len(self)
        orig(self)
        stats["removed"] += n - len(self)

    ns.ObjectLabels.remove_flat_labels_ = checked
    try:
        yield
    finally:
        ns.ObjectLabels.remove_flat_labels_ = orig


def _case_config(state):
    cfg = {k: v for k, v in SHIPPED["random"].items()}
    f = state[2] if state[1].startswith("in") else 1
    cfg["zoom"] = dict(prob=0.8, zoom_in=dict(weight=8, factor=dict(min=f, max=f)), zoom_out=dict(weight=2, factor=dict(min=1, max=1.2)))
    return cfg


def reference_case(ns, case, stats):
    import torch
    C, H, W = GEOMS[case["geom"]]
    fr, labels, counts = case_inputs(case)
    if case.get("events"):
        import make_golden_events as GE
        cols, ends = event_columns()
        fr = GE.reference_frames(GE.load_representations(), *cols, EVENTS["frames"], ends)[0][None]
    T, B = counts.shape
    out_fr = np.zeros_like(fr)
    out_lab, out_cnt, out_head = np.zeros_like(labels), np.zeros_like(counts), np.zeros((T, B, M_ROWS, 5), dtype=np.float32)
    for b, state in enumerate(case["states"]):
        flip, mode, f, x0, y0 = state
        a = ns.aug.RandomSpatialAugmentorGenX((H, W), False, ns.to_cfg(_case_config(state)))
        a.augm_state.apply_h_flip = bool(flip)
        a.augm_state.apply_zoom_in = mode.startswith("in")
        a.augm_state.zoom_out = ns.aug.ZoomOutState(active=mode == "out", x0=x0, y0=y0, zoom_out_factor=f)
        objs = [ns.ObjectLabels(torch.from_numpy(labels[t, b, :counts[t, b]].copy()), (H, W)) if counts[t, b] else None for t in range(T)]
        data = {ns.DataType.EV_REPR: [torch.from_numpy(fr[t, b].copy()) for t in range(T)], ns.DataType.OBJLABELS_SEQ: ns.Sparse(objs)}
        sampler = ns.aug.randomly_sample_zoom_window_from_objframe
        ns.aug.randomly_sample_zoom_window_from_objframe = lambda objframe, zoom_window_height, zoom_window_width: (x0, y0)
        try:
            with warnings.catch_warnings(), _flat_label_margin(ns, stats):
                warnings.simplefilter("ignore")
                res = a(data)
        finally:
            ns.aug.randomly_sample_zoom_window_from_objframe = sampler
        valid, where = [], []
        for t in range(T):
            o = res[ns.DataType.EV_REPR][t]
            assert o.dtype == torch.uint8 and tuple(o.shape) == (C, H, W)
            out_fr[t, b] = o.numpy()
            lab = res[ns.DataType.OBJLABELS_SEQ][t]
            if lab is not None and len(lab) > 0:
                k = len(lab)
                out_lab[t, b, :k] = lab.object_labels.numpy()
                out_cnt[t, b] = k
                valid.append(lab)
                where.append(t)
            elif counts[t, b]:
                stats["emptied"] += 1
        if valid:
            head = ns.ObjectLabels.get_labels_as_batched_tensor(valid, format_='yolox').numpy()
            for i, t in enumerate(where):
                out_head[t, b, :head.shape[1]] = head[i]
    return out_fr, out_lab, out_cnt, out_head


def rng_labels(i: int):
    """the label frames of draw i of the random-state fixture: none, one box, several"""
    H, W = RNG_HW
    k = (0, 1, 4, 2)[i % 4]
    return boxes(900 + i, k, H, W) if k else None


def reference_rng(ns, which: str, seed: int):
    """RNG_DRAWS consecutive states of the reference after torch.manual_seed(seed).  "random": automatic randomization inside __call__,
    as the random-access loader uses it; "stream": randomize_augmentation() then __call__, as the streaming loader does at a new
    sequence.  -> ints [n, 8] (flip, zoom-in chosen, zoom-in applied, its x0, y0, zoom-out active, its x0, y0), floats [n, 2]"""
    import torch
    H, W = RNG_HW
    seen = {}
    orig = ns.aug.RandomSpatialAugmentorGenX._zoom_in_and_rescale_recursive.__func__

    def spy(cls, input_, zoom_coordinates_x0y0, zoom_in_factor, datatype):
        seen["x0y0"], seen["f"] = zoom_coordinates_x0y0, zoom_in_factor
        return orig(cls, input_, zoom_coordinates_x0y0=zoom_coordinates_x0y0, zoom_in_factor=zoom_in_factor, datatype=datatype)

    ns.aug.RandomSpatialAugmentorGenX._zoom_in_and_rescale_recursive = classmethod(spy)
    ints, floats = np.zeros((RNG_DRAWS, 8), dtype=np.int64), np.ones((RNG_DRAWS, 2), dtype=np.float64)
    try:
        torch.manual_seed(seed)
        a = ns.aug.RandomSpatialAugmentorGenX((H, W), which == "random", ns.to_cfg(SHIPPED[which]))
        for i in range(RNG_DRAWS):
            lab = rng_labels(i)
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
                       st.zoom_out.x0 if st.zoom_out.active else 0, st.zoom_out.y0 if st.zoom_out.active else 0)
            floats[i] = (seen.get("f", 1.0), st.zoom_out.zoom_out_factor if st.zoom_out.active else 1.0)
    finally:
        ns.aug.RandomSpatialAugmentorGenX._zoom_in_and_rescale_recursive = classmethod(orig)
    return ints, floats


def generate():
    import torch
    ns = _import_reference()
    fx = {"torch_version": np.array(torch.__version__)}
    stats = {"removed": 0, "emptied": 0}
    for case in cases():
        fr, lab, cnt, head = reference_case(ns, case, stats)
        n = case["name"]
        fx[f"{n}/labels"], fx[f"{n}/counts"], fx[f"{n}/yolox"] = lab, cnt, head
        if case["stored"]:
            fx[f"{n}/frames"] = fr
        else:
            fx[f"{n}/sha256"] = np.frombuffer(hashlib.sha256(fr.tobytes()).digest(), dtype=np.uint8)
            fx[f"{n}/sums"] = fr.astype(np.int64).sum(axis=(-1, -2))
    assert stats["removed"] >= 10 and stats["emptied"] >= 1, stats
    combos = set()
    for which in SHIPPED:
        for seed in RNG_SEEDS:
            ints, floats = reference_rng(ns, which, seed)
            fx[f"rng/{which}/{seed}/ints"], fx[f"rng/{which}/{seed}/floats"] = ints, floats
            if which == "random":
                seq = {(int(r[0]), int(r[1]), int(r[5])) for r in ints}
                assert len(seq) == 6, f"seed {seed}: not all six flip x zoom combinations were drawn: {sorted(seq)}"
                combos |= seq
    return fx


if __name__ == "__main__":
    fixtures = generate()
    np.savez_compressed(OUT, **fixtures)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(fixtures)} arrays")
