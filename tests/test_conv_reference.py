"""CPU tests of the conv operator sweep's own instruments (no GPU): the float64 reference of tests/conv_reference.py against torch.nn
modules, the case table and its committed fp32 bounds, and the size rule of the downsampling conv (functional.downsample_out_hw)."""
import pytest
import torch
import torch.nn as nn

import conv_cases as CC
import conv_reference as R
import operator_sweep as SW

TOL = 1e-12


def close(a, b, what):
    err = float((a.detach() - b.detach()).abs().max())
    assert a.shape == b.shape and err <= TOL * max(1.0, float(b.detach().abs().max())), f"{what}: {err:.3e}"


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("k,stride,groups,two_src", [(1, 1, 1, False), (3, 1, 1, False), (3, 2, 1, False), (1, 2, 1, False), (3, 4, 1, False),
                                                     (1, 1, 1, True), (3, 1, 12, False), (3, 2, 12, False)])
@pytest.mark.parametrize("mode", ["train", "eval", "infer"])
def test_conv_bn_silu_reference_matches_nn_modules(k, stride, groups, two_src, mode):
    """outputs, every gradient and the running statistics after one step equal nn.Conv2d + nn.BatchNorm2d + nn.SiLU in float64"""
    B, H, W, cin, cout = 2, 7, 9, 12, (12 if groups > 1 else 20)
    conv = nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, groups=groups, bias=False).double()
    bn = nn.BatchNorm2d(cout, momentum=0.1, eps=1e-5).double()
    with torch.no_grad():
        conv.weight.copy_(_rand(*conv.weight.shape, seed=1) * 0.3)
        bn.weight.copy_(1 + 0.1 * _rand(cout, seed=2))
        bn.bias.copy_(0.1 * _rand(cout, seed=3))
        bn.running_mean.copy_(0.1 * _rand(cout, seed=4))
        bn.running_var.copy_(0.5 + _rand(cout, seed=5).abs())
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    net = nn.Sequential(conv, bn, nn.SiLU()).train(mode == "train")
    x = _rand(B, H, W, cin, seed=6)
    g = _rand(B, *CC.conv_hw(H, W, k, stride), cout, seed=7) + 0.5
    xm = x.clone().requires_grad_(mode != "infer")
    with torch.set_grad_enabled(mode != "infer"):
        ym = R.nhwc(net(R.nchw(xm)))
    leaves = [t.clone().requires_grad_(mode != "infer") for t in (x, conv.weight.detach(), bn.weight.detach(), bn.bias.detach())]
    xr, w, bw, bb = leaves
    xin = (xr[..., :4], xr[..., 4:]) if two_src else xr
    y, rm, rv = R.conv_bn_silu(xin, w, bw, bb, rm0, rv0, k, stride, mode, 0.1, 1e-5)
    close(y, ym, "y")
    close(rm, bn.running_mean, "running_mean")
    close(rv, bn.running_var, "running_var")
    if mode == "train":
        assert float((bn.running_var - rv0).abs().max()) > 1e-3      # the statistics did move
    if mode == "infer":
        assert not y.requires_grad
        return
    (ym * g).sum().backward()
    (y * g).sum().backward()
    for a, b, what in zip((xr, w, bw, bb), (xm, conv.weight, bn.weight, bn.bias), ("dx", "dw", "d bn_w", "d bn_b")):
        close(a.grad, b.grad, what)


def test_batchnorm_reference_remembers_the_unbiased_variance():
    """the running variance moves by momentum * var * n / (n - 1), the output is normalised by the biased one"""
    x = _rand(1, 2, 4, 4, seed=1)
    w = torch.eye(4, dtype=torch.float64).view(4, 4, 1, 1)
    one, zero = torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    _y, _rm, rv = R.conv_bn_silu(x, w, one, zero, zero, one, 1, 1, "train", momentum=1.0)
    close(rv, x.reshape(8, 4).var(0, unbiased=True), "running_var")


@pytest.mark.parametrize("f,overlap,hw", [(2, True, (8, 12)), (4, True, (8, 12)), (2, False, (9, 13)), (4, False, (13, 18))])
@pytest.mark.parametrize("pe", [False, True])
def test_downsample_ln_reference_matches_nn_modules(f, overlap, hw, pe):
    B, cin, cout = 2, 4, 12
    H, W = hw
    k = 2 * f - 1 if overlap else f
    conv = nn.Conv2d(cin, cout, k, f, f - 1 if overlap else 0, bias=False, padding_mode="replicate" if overlap else "zeros").double()
    ln = nn.LayerNorm(cout, eps=1e-5).double()
    with torch.no_grad():
        ln.weight.copy_(1 + 0.1 * _rand(cout, seed=1))
        ln.bias.copy_(0.1 * _rand(cout, seed=2))
    x = _rand(B, H, W, cin, seed=3)
    Ho, Wo = H // f, W // f
    table = _rand(Ho * Wo, cout, seed=4) if pe else None
    g = _rand(B, Ho, Wo, cout, seed=5) + 0.5
    xm = x.clone().requires_grad_(True)
    ym = ln(R.nhwc(conv(R.nchw(xm))))
    if pe:
        ym = ym + table.view(1, Ho, Wo, cout)
    xr, w, lw, lb = [t.clone().requires_grad_(True) for t in (x, conv.weight.detach(), ln.weight.detach(), ln.bias.detach())]
    y = R.downsample_ln(xr, w, lw, lb, table, f)
    close(y, ym, "y")
    (ym * g).sum().backward()
    (y * g).sum().backward()
    for a, b, what in zip((xr, w, lw, lb), (xm, conv.weight, ln.weight, ln.bias), ("dx", "dw", "d ln_w", "d ln_b")):
        close(a.grad, b.grad, what)
    xb = torch.randint(0, 256, (B, H, W, cin), dtype=torch.uint8, generator=torch.Generator().manual_seed(6))
    close(R.downsample_ln(xb, w, lw, lb, table, f), R.downsample_ln(xb.double(), w, lw, lb, table, f), "uint8 input")


@pytest.mark.parametrize("k,c0,cw,bias", [(1, 0, 8, True), (3, 0, 8, False), (5, 4, 16, True), (7, 8, 16, True)])
def test_dwconv_reference_matches_nn_conv2d(k, c0, cw, bias):
    B, H, W, C = 2, 5, 4, 8
    conv = nn.Conv2d(C, C, k, 1, k // 2, groups=C, bias=bias).double()
    wfull, bfull = _rand(cw, 1, k, k, seed=1), (_rand(cw, seed=2) if bias else None)
    with torch.no_grad():
        conv.weight.copy_(wfull[c0:c0 + C])
        if bias:
            conv.bias.copy_(bfull[c0:c0 + C])
    x, g = _rand(B, H, W, C, seed=3), _rand(B, H, W, C, seed=4) + 0.5
    xm = x.clone().requires_grad_(True)
    ym = R.nhwc(conv(R.nchw(xm)))
    xr, w = x.clone().requires_grad_(True), wfull.clone().requires_grad_(True)
    b = bfull.clone().requires_grad_(True) if bias else None
    y = R.dwconv(xr, w, b, c0)
    close(y, ym, "y")
    (ym * g).sum().backward()
    (y * g).sum().backward()
    close(xr.grad, xm.grad, "dx")
    close(w.grad[c0:c0 + C], conv.weight.grad, "dw")
    outside = torch.ones(cw, dtype=torch.bool)
    outside[c0:c0 + C] = False
    assert float(w.grad[outside].abs().sum()) == 0.0
    if bias:
        close(b.grad[c0:c0 + C], conv.bias.grad, "db")
        assert float(b.grad[outside].abs().sum()) == 0.0


def test_upsample_cat_and_cat2_reference_match_nn_upsample():
    a, b = _rand(2, 3, 5, 4, seed=1).requires_grad_(True), _rand(2, 6, 10, 8, seed=2).requires_grad_(True)
    am = a.detach().clone().requires_grad_(True)
    up = nn.Upsample(scale_factor=2, mode="nearest")
    ym = torch.cat((R.nhwc(up(R.nchw(am))), b.detach()), dim=-1)
    y = R.upsample_cat(a, b)
    close(y, ym, "upsample_cat")
    g = _rand(*y.shape, seed=3) + 0.5
    (y * g).sum().backward()
    (ym * g).sum().backward()
    close(a.grad, am.grad, "da")
    close(b.grad, g[..., 4:], "db")
    c = _rand(2, 3, 5, 8, seed=4)
    assert torch.equal(R.cat2(a.detach(), c), torch.cat((a.detach(), c), -1))


# ------------------------------------------------------------------------------------------------ size rule of the downsampling conv
def test_downsample_out_hw_floors_without_overlap_and_needs_multiples_with_it():
    from sast_amd.functional import downsample_out_hw
    assert downsample_out_hw(64, 48, 4, 7) == (16, 12) and downsample_out_hw(24, 40, 2, 3) == (12, 20)
    assert downsample_out_hw(8, 8, 4, 7) == (2, 2) and downsample_out_hw(2, 2, 2, 3) == (1, 1)
    # no overlap: floor, exactly nn.Conv2d's size (and the library's geom_of: (H - k) / f + 1)
    for H, W, f in ((9, 13, 2), (65, 47, 2), (13, 30, 4), (26, 41, 4), (24, 40, 4), (4, 7, 4)):
        assert downsample_out_hw(H, W, f, f) == (H // f, W // f) == ((H - f) // f + 1, (W - f) // f + 1)
        assert tuple(nn.Conv2d(1, 1, f, f)(torch.zeros(1, 1, H, W)).shape[2:]) == (H // f, W // f)
    # overlap at a non-multiple: the conv has ceil(H / f) rows, more than the H // f the buffers would be sized for
    for H, W, f in ((66, 64, 4), (65, 64, 2), (64, 66, 4), (64, 65, 2), (7, 8, 2), (3, 4, 4)):
        with pytest.raises(RuntimeError) as e:
            downsample_out_hw(H, W, f, 2 * f - 1)
        msg = str(e.value)
        assert f"H = {H}" in msg and f"W = {W}" in msg and f"factor {f}" in msg, msg
    assert tuple(nn.Conv2d(1, 1, 7, 4, 3)(torch.zeros(1, 1, 66, 64)).shape[2:]) == (17, 16)     # what the refusal is about: 17 > 66 // 4
    assert tuple(nn.Conv2d(1, 1, 3, 2, 1)(torch.zeros(1, 1, 65, 64)).shape[2:]) == (33, 32)
    for bad in ((8, 8, 4, 5), (8, 8, 2, 4), (3, 8, 4, 4)):
        with pytest.raises(RuntimeError):
            downsample_out_hw(*bad)


@pytest.mark.parametrize("H,W,f", [(66, 64, 4), (65, 64, 2), (64, 62, 4)])
def test_downsample_ln_refuses_overlap_at_non_multiples_before_touching_the_library(H, W, f, monkeypatch):
    """the wrapper raises the size error first: before the device check (these are CPU tensors) and before the library is loaded"""
    from sast_amd import _lib, functional as SF

    def no_lib():
        raise AssertionError("the library must not be touched")

    monkeypatch.setattr(_lib, "lib", no_lib)
    k = 2 * f - 1
    x = torch.zeros(1, H, W, 4)
    w = torch.zeros(32, k, k, 4).permute(0, 3, 1, 2)
    with pytest.raises(RuntimeError) as e:
        SF.downsample_ln(x, w, torch.ones(32), torch.zeros(32), None, f)
    msg = str(e.value)
    assert f"H = {H}" in msg and f"W = {W}" in msg and f"factor {f}" in msg, msg
    from sast_amd.layers.ops import ConvDownsampling_Cf2Cl
    m = ConvDownsampling_Cf2Cl(4, 32, f)
    with pytest.raises(RuntimeError, match=f"factor {f}"):
        m(torch.zeros(1, 4, H, W))


# ------------------------------------------------------------------------------------------------ the case table and its bounds
def test_case_table_covers_the_classes_the_sweep_is_about():
    cbs = [c for c in CC.CBS_CASES]
    for k, s in ((1, 1), (3, 1), (3, 2), (1, 2), (3, 4)):
        rows = [c for c in cbs if (c["k"], c["s"]) == (k, s)]
        assert any(c["cin"] % 16 == 0 for c in rows) and any(c["cin"] % 16 for c in rows), (k, s)
        assert any(c["cout"] % 16 == 0 for c in rows) and any(c["cout"] % 16 for c in rows), (k, s)
        assert any(CC.conv_hw(c["H"], c["W"], k, s)[0] == 1 for c in rows), (k, s)
        assert any(c["modes"] == ("infer",) for c in rows), (k, s)
    assert {c["cin"] for c in cbs} >= {4, 12, 20, 100, 32, 64, 256} and {c["cout"] for c in cbs} >= {4, 12, 36, 132, 16, 48, 128}
    s2 = [c for c in cbs if (c["k"], c["s"]) == (3, 2) and "train" in c["modes"]]
    mc = lambda c: c["B"] * (c["H"] // 2) * (c["W"] // 2)       # noqa: E731
    even = lambda c: c["H"] % 2 == 0 and c["W"] % 2 == 0        # noqa: E731
    assert sum(even(c) and mc(c) % 64 == 0 for c in s2) >= 2 and sum(even(c) and mc(c) % 64 != 0 for c in s2) >= 3
    assert sum(not even(c) for c in s2) >= 3
    for c in CC.ALL_CASES:
        if c["op"] in ("cbs", "cbs_dw") and "train" in c["modes"]:
            Ho, Wo = CC.conv_hw(c["H"], c["W"], c["k"], c["s"])
            assert c["B"] * Ho * Wo >= 8, c["id"]
    assert any(c["modes"] == ("infer",) and c["B"] * c["H"] * c["W"] == 1 for c in cbs)
    down = CC.DOWN_CASES
    assert {c["cout"] for c in down} >= {32, 48, 64, 96, 128, 192, 256} and {c["cin"] for c in down} >= {4, 20, 32, 64}
    assert all(c["H"] % c["f"] == 0 and c["W"] % c["f"] == 0 for c in down if c["overlap"]), "the overlapping form never runs at a non-multiple"
    assert any((c["H"] % c["f"] or c["W"] % c["f"]) for c in down if not c["overlap"])
    assert {c["k"] for c in CC.DWCONV_CASES} == {1, 3, 5, 7} and {c["c"] for c in CC.DWCONV_CASES} >= {4, 48, 64, 256}


def test_committed_bounds_hold_every_case_and_stay_inside_the_project_bars():
    doc = SW.load_bounds("conv")
    want = {CC.bounds_id(c) for c in CC.ALL_CASES}
    assert set(doc["cases"]) == want
    for cid in sorted(want)[::9]:        # a sample is re-evaluated: same quantities, figures of the same size (thread counts move fp32 sums)
        case = CC.BY_ID[cid]
        inp = CC.make_inputs(case)
        r64, r32 = CC.reference(case, inp, torch.float64), CC.reference(case, inp, torch.float32)
        assert set(r64) == set(doc["cases"][cid]), cid
        for q in r64:
            e = SW.measure(q, r32[q], r64[q])[0]
            floor = doc["operators"][case["op"]][CC.pool_key(q)]["median"]
            assert e <= 8 * max(doc["cases"][cid][q], floor) + 1e-30, (cid, q, e, doc["cases"][cid][q])
    for op, qs in doc["operators"].items():
        for q, v in qs.items():
            assert v["median"] <= v["worst"] < SW.project_bar(q) / 2, (op, q, v)
