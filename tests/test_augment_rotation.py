"""Rotation in the spatial augmentation, and int8 frames (sast_amd/augment.py with rotation=True, csrc/k_rotaug.hip).

The contract is tests/augment_rotation_model.py: torchvision's tensor rotate (NEAREST) and ObjectLabels.rotate_ restated in numpy, fp32 one
operation at a time, composed with flip and zoom in the reference's order.  CPU tests hold that model to the torch restatement of
torchvision's rotate (tests/golden/make_golden_augment_rotation.py) and the seeded draws to the reference's; GPU tests hold the kernels to
the model byte for byte (frames) and to the fixture the reference produced (tests/golden/augment_rotation.npz) bit for bit (labels of
frames of at most 6 boxes; within COORD_TOL on the 64-box frame, where torch's einsum takes a fused form).  Inputs are regenerated from
make_golden_augment's integer hash: nothing here reads the reference on the GPU box."""
import hashlib
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_rotation_model as M  # noqa: E402
import make_golden_augment as G  # noqa: E402
import make_golden_augment_rotation as R  # noqa: E402

gpu = pytest.mark.gpu
CASES = {c["name"]: c for c in R.cases()}
SHAPES = [(45, 80), (60, 76), (33, 47)]
ANGLES = [2.0, -2.0, 6.0, -6.0, 3.7, -4.25, 17.3]
# a source coordinate is the result of at most 8 fp32 roundings of <= 1/2 ulp at magnitudes < 1024 (ulp 6.1e-5): 2.4e-4 px < DELTA
DELTA = 1e-3
# the derived bound on a box coordinate (tests/test_augment.py): fp32 roundings of <= 1/2 ulp at magnitudes < 2048 -> < 1e-3 px
COORD_TOL = 1e-3


def _fixtures():
    return np.load(os.path.join(GOLDEN, "augment_rotation.npz"))


def _ref_available():
    import _ref_import as RI
    return os.path.isfile(os.path.join(RI.REF_ROOT, "data", "utils", "augmentor.py"))


def _state(t):
    from sast_amd import augment as A
    flip, mode, f, x0, y0, angle = t
    st = A.AugmentationState(apply_h_flip=bool(flip))
    if angle is not None:
        st.rotation = A.RotationState(True, angle)
    if mode == "in":
        st.apply_zoom_in, st.zoom_in = True, A.ZoomInState(active=True, x0=x0, y0=y0, zoom_in_factor=f)
    elif mode == "out":
        st.zoom_out = A.ZoomOutState(active=True, x0=x0, y0=y0, zoom_out_factor=f)
    return st


def _augmentor(hw, states, rotation=True):
    from sast_amd.augment import SpatialAugmentor
    aug = SpatialAugmentor(hw, R.RNG_CONFIG["random"] if rotation else G.SHIPPED["random"], len(states), rotation=rotation)
    aug.set_state([_state(s) for s in states])
    return aug


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def _restated_src(angle, H, W):
    """the source pixel torch's grid_sample picks for every pixel: an image of its own pixel indices + 1 (exact in fp32), 0 = outside"""
    idx = torch.arange(1, H * W + 1, dtype=torch.float32).reshape(1, 1, H, W)
    got = torch.nn.functional.grid_sample(idx, R.rotation_grid(angle, H, W), mode="nearest", padding_mode="zeros", align_corners=False)
    return got[0, 0].numpy().astype(np.int64) - 1


def _model_src(angle, H, W):
    sy, sx, inside = M.rotation_src(angle, H, W)
    return np.where(inside, sy * W + sx, -1)


@pytest.mark.parametrize("hw", SHAPES)
def test_model_agrees_with_the_torch_restatement_away_from_rounding_ties(hw):
    """every pixel whose exact (fp64) source coordinate is more than DELTA from a rounding boundary (k + 1/2; the frame's edge is one)
    has the same source pixel in the model and in affine grid + grid_sample; at most 1 % of a frame's pixels are that close to one"""
    H, W = hw
    for angle in ANGLES:
        r = math.radians(-angle)
        bx = np.arange(W, dtype=np.float64)[None, :] + (0.5 - 0.5 * W)
        by = np.arange(H, dtype=np.float64)[:, None] + (0.5 - 0.5 * H)
        ix = math.cos(r) * bx + math.sin(r) * by + (W - 1) / 2
        iy = -math.sin(r) * bx + math.cos(r) * by + (H - 1) / 2
        clear = (np.abs(ix - np.floor(ix) - 0.5) > DELTA) & (np.abs(iy - np.floor(iy) - 0.5) > DELTA)
        excluded = 1 - clear.mean()
        print(f"{H}x{W} at {angle}: {100 * excluded:.2f} % of the pixels within {DELTA} px of a tie")
        assert excluded <= 0.01
        model, restated = _model_src(angle, H, W), _restated_src(angle, H, W)
        assert np.array_equal(model[clear], restated[clear]), (hw, angle)
        # and the exact coordinate rounds to the model's pixel there: the model is the rule, not merely torch's twin
        ex, ey = np.floor(ix + 0.5).astype(np.int64), np.floor(iy + 0.5).astype(np.int64)
        exact = np.where((ex >= 0) & (ex < W) & (ey >= 0) & (ey < H), ey * W + ex, -1)
        assert np.array_equal(model[clear], exact[clear]), (hw, angle)


def test_model_equals_the_restatement_outright_at_quarter_and_half_turns():
    """90 degrees on 45 x 80 puts every pixel on an exact tie (ties go to even); 180 and 0 degrees are far from any"""
    assert np.array_equal(_model_src(90.0, 45, 80), _restated_src(90.0, 45, 80))
    sy, sx, inside = M.rotation_src(90.0, 45, 80)
    assert 0 < inside.sum() < 45 * 80
    for H, W in SHAPES:
        for angle in (180.0, 0.0):
            assert np.array_equal(_model_src(angle, H, W), _restated_src(angle, H, W)), (H, W, angle)
        assert np.array_equal(_model_src(0.0, H, W), np.arange(H * W).reshape(H, W))
        assert np.array_equal(_model_src(180.0, H, W), np.arange(H * W)[::-1].reshape(H, W))


@pytest.mark.parametrize("which", sorted(R.RNG_CONFIG))
def test_seeded_randomize_reproduces_the_reference_states_with_rotation(which):
    """rotate.prob 0.5, angles 2..6: after the same torch.manual_seed, randomize() reaches the reference's states -- the rotation draw,
    its sign (randn) and angle, and the zoom-in windows placed on the flipped AND rotated labels"""
    from sast_amd.augment import SpatialAugmentor
    fx = _fixtures()
    drew = str(fx["torch_version"])
    assert drew == torch.__version__, (f"the fixture pins the CPU generator stream of torch {drew}; this is torch {torch.__version__}: "
                                       "regenerate tests/golden/augment_rotation.npz with this version and compare")
    for seed in R.RNG_SEEDS:
        want_i, want_f = fx[f"rng/{which}/{seed}/ints"], fx[f"rng/{which}/{seed}/floats"]
        assert len(want_i) >= 200
        torch.manual_seed(seed)
        aug = SpatialAugmentor(R.RNG_HW, R.RNG_CONFIG[which], 1, rotation=True)
        for i in range(len(want_i)):
            lab = G.rng_labels(i)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                st = aug.randomize(latest_labels=[None if lab is None else torch.from_numpy(lab)])[0]
            zo = st.zoom_out
            got_i = (st.apply_h_flip, st.apply_zoom_in, st.zoom_in.active, st.zoom_in.x0, st.zoom_in.y0, zo.active,
                     zo.x0 if zo.active else 0, zo.y0 if zo.active else 0, st.rotation.active)
            got_f = (st.zoom_in.zoom_in_factor if st.zoom_in.active else 1.0, zo.zoom_out_factor if zo.active else 1.0,
                     st.rotation.angle_deg if st.rotation.active else 0.0)
            assert tuple(int(v) for v in got_i) == tuple(int(v) for v in want_i[i]), (seed, i)
            assert got_f == tuple(float(v) for v in want_f[i]), (seed, i)
            assert aug._rot_host[0, 0] == int(st.rotation.active)
            if st.rotation.active:
                assert 2 <= abs(st.rotation.angle_deg) <= 6


def test_rotation_is_opt_in_and_validated():
    from sast_amd import _lib
    from sast_amd import augment as A
    cfg = R.RNG_CONFIG["random"]
    # the default: both refusals, and the draws of an augmentor that cannot rotate
    with pytest.raises(NotImplementedError, match="rotation"):
        A.SpatialAugmentor((45, 80), cfg, 1)
    plain = A.SpatialAugmentor((45, 80), G.SHIPPED["random"], 1)
    assert plain.rotation is False
    with pytest.raises(NotImplementedError):
        plain.set_state([A.AugmentationState(rotation=A.RotationState(True, 3.0))])
    # opted in: accepted, the words are the host side of the rule
    aug = A.SpatialAugmentor((45, 80), cfg, 2, rotation=True)
    assert aug.rotation and aug._rot_host.shape == (2, _lib.ROTAUG_PARAM_WORDS) and not aug._rot_host.any()
    aug.set_state([A.AugmentationState(rotation=A.RotationState(True, 3.7)), A.AugmentationState(apply_h_flip=True)])
    row = aug._rot_host[0]
    assert row[0] == 1 and row[7] == 0 and not aug._rot_host[1].any()
    assert np.array_equal(row[1:5].view(np.float32), np.array(M.rotation_matrix(3.7, 45, 80), dtype=np.float32))
    a = 3.7 / 180 * math.pi
    assert np.array_equal(row[5:7].view(np.float32), np.array([math.cos(a), math.sin(a)], dtype=np.float32))
    assert list(aug._host[:, 0]) == [0, 1]
    before = aug._rot_host.copy(), aug._host.copy()
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            aug.set_state([A.AugmentationState(rotation=A.RotationState(True, bad)), A.AugmentationState()])
    with pytest.raises(ValueError):           # a bad zoom beside a good rotation
        aug.set_state([A.AugmentationState(rotation=A.RotationState(True, 1.0)), A.AugmentationState(zoom_out=A.ZoomOutState(True, 0, -1, 1.2))])
    assert np.array_equal(aug._rot_host, before[0]) and np.array_equal(aug._host, before[1])      # a rejected state changes nothing
    aug.set_state([A.AugmentationState(rotation=A.RotationState(False, 9.0))] * 2)                # inactive: the angle is ignored
    assert not aug._rot_host.any()
    # an opted-in augmentor with rotate.prob 0 never draws a rotation and spends the draws of the plain one
    torch.manual_seed(3)
    s1 = [A.SpatialAugmentor((240, 304), G.SHIPPED["stream"], 1, rotation=True).randomize()[0] for _ in range(20)]
    torch.manual_seed(3)
    s2 = [A.SpatialAugmentor((240, 304), G.SHIPPED["stream"], 1).randomize()[0] for _ in range(20)]
    assert s1 == s2 and not any(s.rotation.active for s in s1)
    # JoinedAugmentor rotates iff a part does; the other parts' rows stay inactive
    p0, p1 = A.SpatialAugmentor((45, 80), G.SHIPPED["stream"], 2), A.SpatialAugmentor((45, 80), cfg, 3, rotation=True)
    j = A.JoinedAugmentor([p0, p1])
    assert j.rotation and j._rot_host.shape == (5, 8)
    p1.set_state([A.AugmentationState(rotation=A.RotationState(True, -5.0))] * 3)
    assert list(j._rot_host[:, 0]) == [0, 0, 1, 1, 1]
    with pytest.raises(NotImplementedError):
        p0.set_state([A.AugmentationState(rotation=A.RotationState(True, 1.0))] * 2)
    assert not A.JoinedAugmentor([A.SpatialAugmentor((45, 80), G.SHIPPED["stream"], 1)]).rotation


def test_rotaug_entry_points_declared_bound_and_refuse_bad_sizes():
    import ctypes as C
    from sast_amd import _lib
    from sast_amd import build as B
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_rotaug_")]
    assert sorted(names) == ["sast_rotaug_frames", "sast_rotaug_labels"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    with open(_lib.HEADER_PATH) as f:
        assert f"#define SAST_ROTAUG_PARAM_WORDS {_lib.ROTAUG_PARAM_WORDS}" in f.read()
    assert _lib.ROTAUG_PARAM_WORDS == 8 and _lib.AUGMENT_PARAM_WORDS == 16
    assert "k_rotaug.hip" in B.SOURCES and B.SOURCE_FLAGS["k_rotaug.hip"] == ["-ffp-contract=off"] and "aug_map.cuh" in B.HEADERS
    # bad sizes are refused on the host, before anything is enqueued (no device needed)
    buf = (C.c_uint8 * 64)()
    p, q = C.addressof(buf), C.addressof(buf) + 32
    assert lib.sast_rotaug_frames(p, q, p, p, 1, 1, 1, 4097, 16, None) == -22
    assert lib.sast_rotaug_frames(p, q, p, p, 1, 1, 1, 16, 0, None) == -22
    assert lib.sast_rotaug_frames(p, q, p, p, 65536, 1, 1, 16, 16, None) == -22
    assert lib.sast_rotaug_frames(p, p, p, p, 1, 1, 1, 16, 16, None) == -22          # in place
    assert lib.sast_rotaug_frames(p, q, p, None, 1, 1, 1, 16, 16, None) == -22       # no rot_params
    assert lib.sast_rotaug_labels(p, p, p, p, 1, 1, 0, 16, 16, q, q, None, None) == -22
    assert lib.sast_rotaug_labels(p, p, p, p, 1, 1, 4, 0, 16, q, q, None, None) == -22     # H
    assert lib.sast_rotaug_labels(p, p, p, None, 1, 1, 4, 16, 16, q, q, None, None) == -22
    assert lib.sast_rotaug_labels(p, p, p, p, 1, 1, 4, 16, 16, p, q, None, None) == -22    # in place


def test_rotation_fixture_covers_what_it_is_for():
    fx = _fixtures()
    removed = 0
    for name, case in CASES.items():
        _fr, _lab, cnt = R.case_inputs(case)
        assert cnt.max() <= 6 and f"{name}/frames" in fx.files
        removed += int((cnt - fx[f"{name}/counts"]).sum())
        assert any(s[5] is not None for s in case["states"])
    assert removed >= 3
    assert any(s[5] is None for s in CASES["b_seq"]["states"]) and CASES["b_seq"]["T"] == 2
    assert int(fx["big/counts"][0, 0]) > 32 and R.BIG["boxes"] == 64


def test_model_composes_flip_rotation_and_zoom_like_the_fixture():
    """the reference's __call__ with the restated rotate: the model's frames byte for byte, its labels bit for bit (<= 6 boxes a frame)"""
    fx = _fixtures()
    for name, case in CASES.items():
        _C, H, W = R.GEOMS[case["geom"]]
        fr, lab, cnt = R.case_inputs(case)
        assert np.array_equal(M.frames(fr, case["states"]), fx[f"{name}/frames"]), name
        m_lab, m_cnt, m_head = M.batch_labels(lab, cnt, case["states"], H, W)
        assert np.array_equal(m_cnt, fx[f"{name}/counts"]), name
        assert np.array_equal(m_lab.view(np.int32), fx[f"{name}/labels"].view(np.int32)), name
        assert np.array_equal(m_head.view(np.int32), fx[f"{name}/yolox"].view(np.int32)), name


def test_tool_aten_restatement_with_rotation_equals_the_fixture_frames():
    """tools/augment_bench.py --rotation times flip / rotate / zoom restated in ATen: on the CPU it gives the fixture's frames"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import augment_bench as T
    fx = _fixtures()
    for name, case in CASES.items():
        fr = torch.from_numpy(R.case_inputs(case)[0])
        H, W = fr.shape[-2:]
        sts = [_state(s) for s in case["states"]]
        grids = [T.rotation_grid(st.rotation.angle_deg, H, W, "cpu") if st.rotation.active else None for st in sts]
        got = T.aten_augment_rotation(fr, sts, grids, torch.empty_like(fr))
        assert torch.equal(got, torch.from_numpy(fx[f"{name}/frames"])), name


@pytest.mark.skipif(not _ref_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_rotation_fixture():
    got = R.generate()
    want = _fixtures()
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert np.array_equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------------------------------------- GPU

def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_MODEL_FRAMES = {}


def _model_frames(name):
    """the model's frames of a case, computed once"""
    if name not in _MODEL_FRAMES:
        case = CASES[name]
        _MODEL_FRAMES[name] = M.frames(R.case_inputs(case)[0], case["states"])
    return _MODEL_FRAMES[name]


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_rotated_frames_equal_the_model_and_the_fixture_byte_for_byte(name):
    """45 x 80 (16-byte loads and stores, two tiles), 60 x 76 and 33 x 47 (the byte path), C = 3: rotation alone, with flip, with zoom-in and zoom-out, a row
    without rotation; T = 2, B = 3 with active and inactive rows; quarter and half turns"""
    case, fx = CASES[name], _fixtures()
    _C, H, W = R.GEOMS[case["geom"]]
    fr = R.case_inputs(case)[0]
    aug = _augmentor((H, W), case["states"])
    x = _dev(fr)
    got = aug(x)
    assert got.shape == x.shape and got.dtype == torch.uint8
    assert torch.equal(got, _dev(_model_frames(name)))
    assert torch.equal(got, _dev(fx[f"{name}/frames"]))
    if fr.shape[0] == 1:          # [B, C, H, W] is the same call with T = 1
        assert torch.equal(aug(x[0]), got[0])
    assert torch.equal(x, _dev(fr))                                  # the input is left alone
    # the rows without rotation are what the default augmentor gives (its own kernel)
    plain_rows = [b for b, s in enumerate(case["states"]) if s[5] is None]
    if plain_rows:
        plain = _augmentor((H, W), [s[:5] + (None,) for s in case["states"]], rotation=False)(x)
        for b in plain_rows:
            assert torch.equal(got[:, b], plain[:, b]), b


@gpu
def test_rotation_inactive_everywhere_equals_the_default_augmentor():
    """rotation=True with no active row: the rotating kernels give the frames and labels of sast_augment_frames / _labels, for every
    flip x zoom combination of the existing fixture"""
    case = {c["name"]: c for c in G.cases()}["s2_combos"]
    _C, H, W = G.GEOMS[case["geom"]]
    fr, lab, cnt = G.case_inputs(case)
    states = [s + (None,) for s in case["states"]]
    a, b = _augmentor((H, W), states, rotation=True), _augmentor((H, W), states, rotation=False)
    for yolox in (False, True):
        got, want = a(_dev(fr), _dev(lab), _dev(cnt), yolox=yolox), b(_dev(fr), _dev(lab), _dev(cnt), yolox=yolox)
        for u, v in zip(got, want):
            assert torch.equal(u, v)
    assert torch.equal(got[0], _dev(np.load(os.path.join(GOLDEN, "augment.npz"))["s2_combos/frames"]))


@gpu
def test_rotation_misaligned_bases_take_the_byte_path_with_the_same_frames():
    name = "a_combos"
    case = CASES[name]
    fr = R.case_inputs(case)[0]
    aug = _augmentor((45, 80), case["states"])
    want = _dev(_model_frames(name))
    store = torch.zeros(fr.size + 64, dtype=torch.uint8, device="cuda")
    for off in (1, 8):
        x = store[off:off + fr.size].view(fr.shape)
        x.copy_(_dev(fr))
        assert x.data_ptr() % 16 == off
        assert torch.equal(aug(x), want)                               # a misaligned input alone: still 16-byte stores
        out = torch.zeros(fr.size + 64, dtype=torch.uint8, device="cuda")
        o = out[off:off + fr.size].view(fr.shape)
        assert aug(_dev(fr), out=o) is o and torch.equal(o, want)
        assert int(out[:off].sum()) == 0 and int(out[off + fr.size:].sum()) == 0      # nothing written outside the frames
        out.fill_(0)
        assert aug(x, out=o) is o and torch.equal(o, want)


BIGGER = {
    # 128 x 160 with C = 20: 2 x 3 tiles (the last column of tiles partial) and more than one channel per workgroup
    "ev": dict(shape=(2, 2, 20, 128, 160), seed=41, states=[(1, "in", 1.35, 30, 20, 4.5), (0, "out", 1.2, 11, 9, -3.25)]),
    # 360 x 640 (Gen4 / 2): 6 x 10 tiles a frame, the last row of tiles partial.  The third sample zooms out by 3 at 45 degrees: the
    # source box of a tile (about 270 x 270 pixels) does not fit the staging area, so its tiles are gathered from global memory
    "gen4": dict(shape=(1, 3, 20, 360, 640), seed=42, states=[(1, "in", 1.3, 70, 40, 5.5), (0, "out", 1.15, 40, 30, -2.75),
                                                              (1, "out", 3.0, 100, 50, 45.0)]),
}


@gpu
@pytest.mark.parametrize("name", sorted(BIGGER))
def test_rotated_frames_of_full_size_equal_the_model(name):
    c = BIGGER[name]
    fr = G.frames(c["seed"], c["shape"])
    H, W = c["shape"][-2:]
    want = M.frames(fr, c["states"])
    assert 0 < np.count_nonzero(want) < np.count_nonzero(fr)
    got = _augmentor((H, W), c["states"])(_dev(fr)).cpu().numpy()
    assert hashlib.sha256(got.tobytes()).digest() == hashlib.sha256(want.tobytes()).digest()
    if name == "ev":
        assert np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_rotated_labels_equal_the_reference_bit_for_bit(name):
    case, fx = CASES[name], _fixtures()
    _C, H, W = R.GEOMS[case["geom"]]
    fr, lab, cnt = R.case_inputs(case)
    aug = _augmentor((H, W), case["states"])
    assert lab.shape[-2] > cnt.max()                                  # M larger than any count
    _f, got, got_n = aug(_dev(fr), _dev(lab), _dev(cnt))
    want, want_n = fx[f"{name}/labels"], fx[f"{name}/counts"]
    assert np.array_equal(got_n.cpu().numpy(), want_n)                # counts exact
    g = got.cpu().numpy()
    assert np.array_equal(g[..., [0, 5, 6]], want[..., [0, 5, 6]])    # row order: t / class / confidence travel with their rows
    err = float(np.abs(g.astype(np.float64) - want.astype(np.float64)).max())
    print(f"{name}: max |coordinate error| = {err:.3e} px")
    assert np.array_equal(g.view(np.int32), want.view(np.int32))      # bitwise, zero rows after the count included
    _f, head, head_n = aug(_dev(fr), _dev(lab), _dev(cnt), yolox=True)
    assert head.shape == lab.shape[:-1] + (5,)
    assert np.array_equal(head_n.cpu().numpy(), want_n)
    assert np.array_equal(head.cpu().numpy().view(np.int32), fx[f"{name}/yolox"].view(np.int32))


@gpu
def test_rotated_labels_of_a_64_box_frame_within_the_coordinate_bound():
    """64 boxes (more than one wave's worth of rows): torch's einsum fuses there, so the reference is matched within COORD_TOL; the
    model (the plain form) is matched bit for bit; counts and row order are exact against both"""
    fx = _fixtures()
    _C, H, W = R.GEOMS[R.BIG["geom"]]
    fr, lab, cnt = R.big_inputs()
    aug = _augmentor((H, W), [R.BIG["state"]])
    m_lab, m_cnt, m_head = M.batch_labels(lab, cnt, [R.BIG["state"]], H, W)
    for yolox, want, model in ((False, fx["big/labels"], m_lab), (True, fx["big/yolox"], m_head)):
        _f, got, got_n = aug(_dev(fr), _dev(lab), _dev(cnt), yolox=yolox)
        g = got.cpu().numpy()
        assert np.array_equal(got_n.cpu().numpy(), fx["big/counts"]) and np.array_equal(fx["big/counts"], m_cnt)
        order = [0] if yolox else [0, 5, 6]
        assert np.array_equal(g[..., order], want[..., order])
        err = float(np.abs(g.astype(np.float64) - want.astype(np.float64)).max())
        print(f"64 boxes, yolox={yolox}: max |coordinate error| against the reference = {err:.3e} px")
        assert err <= COORD_TOL
        assert np.array_equal(g.view(np.int32), model.view(np.int32))


@gpu
@pytest.mark.parametrize("rotation", [False, True])
def test_int8_frames_are_the_uint8_result_of_the_same_bytes(rotation):
    """mixed-density frames (int8, negative values included) through both frame kernels, the byte path (W = 72) and 16-byte stores
    (W = 64)"""
    from sast_amd.augment import SpatialAugmentor
    md = np.load(os.path.join(GOLDEN, "mixed_density.npz"))["batched/duration_ds0/frames"]
    assert md.dtype == np.int8 and md.shape == (4, 10, 24, 72) and (md < 0).any()
    for W in (72, 64):
        fr = np.ascontiguousarray(md[..., :W])
        states = [(1, "none", 1.0, 0, 0, 5.0), (0, "in", 1.3, 5, 2, -3.0), (1, "out", 1.2, 3, 1, 2.5), (0, "none", 1.0, 0, 0, None)]
        if not rotation:
            states = [s[:5] + (None,) for s in states]
        aug = _augmentor((24, W), states, rotation=rotation)
        x = _dev(fr)
        got = aug(x)
        assert got.dtype == torch.int8 and got.shape == x.shape
        as_u8 = aug(x.view(torch.uint8))
        assert as_u8.dtype == torch.uint8 and torch.equal(got.view(torch.uint8), as_u8)
        assert np.array_equal(got.cpu().numpy(), M.frames(fr[None], states)[0])
        assert (got < 0).any()
        out = torch.empty_like(x)
        assert aug(x, out=out) is out and torch.equal(out, got)
        with pytest.raises(ValueError):
            aug(x, out=torch.empty_like(x, dtype=torch.uint8))           # out has the input's dtype
        with pytest.raises(TypeError):
            aug(x.to(torch.int16))


@gpu
def test_rotation_graph_replays_with_new_angles_and_states():
    """frames and labels captured once; replayed after set_state() rewrote params and rot_params, the graph gives the eager result"""
    case = CASES["b_seq"]
    _C, H, W = R.GEOMS[case["geom"]]
    fr, lab, cnt = R.case_inputs(case)
    x, lab_d, cnt_d = _dev(fr), _dev(lab), _dev(cnt)
    aug = _augmentor((H, W), case["states"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            aug(x, lab_d, cnt_d, yolox=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_fr, g_lab, g_n = aug(x, lab_d, cnt_d, yolox=True)
    sets = [case["states"],
            [(0, "out", 1.15, 4, 3, -6.0), (1, "in", 1.3, 10, 8, 2.5), (0, "none", 1.0, 0, 0, None)],
            [(1, "none", 1.0, 0, 0, None), (0, "none", 1.0, 0, 0, 17.3), (1, "in", 1.2, 3, 30, -2.0)],
            case["states"]]
    for states in sets:
        aug.set_state([_state(t) for t in states])
        g.replay()
        torch.cuda.synchronize()
        got = g_fr.clone(), g_lab.clone(), g_n.clone()
        assert torch.equal(got[0], _dev(M.frames(fr, states)))
        m_lab, m_cnt, m_head = M.batch_labels(lab, cnt, states, H, W)
        assert np.array_equal(got[2].cpu().numpy(), m_cnt)
        assert np.array_equal(got[1].cpu().numpy().view(np.int32), m_head.view(np.int32))
        for u, v in zip(got, aug(x, lab_d, cnt_d, yolox=True)):
            assert torch.equal(u, v)


@gpu
def test_joined_augmentor_with_one_rotating_and_one_plain_part():
    from sast_amd import augment as A
    H, W = 60, 76
    plain = A.SpatialAugmentor((H, W), G.SHIPPED["stream"], 2)
    rot = A.SpatialAugmentor((H, W), R.RNG_CONFIG["random"], 3, rotation=True)
    joined = A.JoinedAugmentor([plain, rot])
    st_plain = [(1, "out", 1.2, 5, 2, None), (0, "none", 1.0, 0, 0, None)]
    st_rot = [(1, "in", 1.45, 20, 15, 5.0), (0, "none", 1.0, 0, 0, None), (0, "out", 1.1, 2, 3, -4.0)]
    plain.set_state([_state(s) for s in st_plain])
    rot.set_state([_state(s) for s in st_rot])
    fr = G.frames(51, (2, 5, 3, H, W))
    cnt = np.array([[3, 0, 6, 2, 5], [1, 4, 0, 6, 3]], dtype=np.int32)
    lab = np.zeros((2, 5, 8, 7), dtype=np.float32)
    for t in range(2):
        for b in range(5):
            lab[t, b, :cnt[t, b]] = G.boxes(5100 + 10 * t + b, cnt[t, b], H, W, t=float(t))
    got, got_lab, got_n = joined(_dev(fr), _dev(lab), _dev(cnt))
    states = st_plain + st_rot
    m_lab, m_cnt, _h = M.batch_labels(lab, cnt, states, H, W)
    assert torch.equal(got, _dev(M.frames(fr, states)))
    assert np.array_equal(got_n.cpu().numpy(), m_cnt) and np.array_equal(got_lab.cpu().numpy().view(np.int32), m_lab.view(np.int32))
    assert joined.rot_params.shape == (5, 8) and joined.rot_params[:, 0].tolist() == [0, 0, 1, 0, 1]
    assert plain.rot_params is None and rot.rot_params.data_ptr() == joined.rot_params[2:].data_ptr()
    # a part's new states reach the joined tensors, its own rows only; the parts still work alone on their rows
    rot.set_state([_state(s) for s in st_rot[::-1]])
    states = st_plain + st_rot[::-1]
    assert torch.equal(joined(_dev(fr)), _dev(M.frames(fr, states)))
    assert torch.equal(rot(_dev(fr[:, 2:])), _dev(M.frames(fr[:, 2:], st_rot[::-1])))
    assert torch.equal(plain(_dev(fr[:, :2])), _dev(M.frames(fr[:, :2], st_plain)))
