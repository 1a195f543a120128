"""The case table of the conv operator sweep (tests/test_conv_operators.py), the inputs of every case and its CPU reference evaluation.

Shared by the GPU test and by the bounds generator (tests/operator_sweep.py, which evaluates every case in float32 against float64 on the
CPU), so that both see the same cases, the same numbers and the same quantity names.  CPU only: nothing here imports the library.

A case is a dict with an "id", an "op" (the operator family its error statistics are pooled over) and the shape parameters.
`make_inputs(case)` -> fp32 (uint8 for the stem cases) CPU tensors drawn from a generator seeded by the id.
`reference(case, inputs, dtype)` -> {quantity: tensor}; quantity names are "<mode>/out:<name>" (forward results, compared absolutely:
every output is O(1)), "<mode>/grad:<name>" and "<mode>/stat:<name>" (gradients, running statistics: relative to the max-norm).

Input recipe: weights ~ randn / sqrt(k * k * Cin) so every conv output is O(1) and one wrong border tap moves an element by O(0.1);
BatchNorm / LayerNorm weight 1 + 0.1 randn, bias 0.1 randn; running mean 0.1 randn and running var in [0.5, 1.5) -- NOT the defaults, an
ignored statistic shows; upstream gradient randn + 0.5 (a symmetric one makes the per-channel sums cancel and the bias gradients
ill-conditioned).  Training-mode rows have M = B * Ho * Wo >= 8: with two rows per channel batch-statistics BatchNorm amplifies rounding
until fp32 itself misses the forward bar.
The "sat" cases (k = 1 and k = 3) multiply bn_w by 8 and set bn_b to +4 / -4 on alternating channels: the SiLU of the unit and its backward
see arguments of standard deviation about 9 around +-4, |x| up to 29 (k = 3) and 48 (k = 1), a quarter of them beyond 10, where the
Gaussian recipe never leaves O(1).
"""
import math
import re

import torch

import conv_reference as R
import operator_sweep as SW


def conv_hw(H, W, k, s):
    p = (k - 1) // 2
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ------------------------------------------------------------------------------------------------ the table
def _cbs(k, s, bhw, cin, cout, modes="tei", cin1=0, two=False, env=None, tag=""):
    B, H, W = bhw
    cid = f"cbs-k{k}s{s}-{B}x{H}x{W}-{cin}to{cout}" + (f"-src{cin1}" if cin1 else "") + ("-two" if two else "") + (f"-{tag}" if tag else "")
    Ho, Wo = conv_hw(H, W, k, s)
    modes = tuple({"t": "train", "e": "eval", "i": "infer"}[m] for m in modes)
    assert "train" not in modes or B * Ho * Wo >= 8, cid
    return dict(id=cid, op="cbs", k=k, s=s, B=B, H=H, W=W, cin=cin, cout=cout, cin1=cin1, two=two, modes=modes, env=env or {}, dw=False,
                sat=tag == "sat")


def _dw(s, bhw, c, modes="tei"):
    B, H, W = bhw
    Ho, Wo = conv_hw(H, W, 3, s)
    modes = tuple({"t": "train", "e": "eval", "i": "infer"}[m] for m in modes)
    assert "train" not in modes or B * Ho * Wo >= 8
    return dict(id=f"cbsdw-k3s{s}-{B}x{H}x{W}-{c}", op="cbs_dw", k=3, s=s, B=B, H=H, W=W, cin=c, cout=c, cin1=0, two=False, modes=modes,
                env={}, dw=True)


# knob sets that force a tile family whatever the shape (gemm_dispatch.cuh: gemm_auto, gemm_pair_ep)
ENV_K2 = {"SAST_TINY_NB": "0", "SAST_THIN_NB": "0"}
ENV_THIN = {"SAST_TINY_NB": "0"}
ENV_K1 = {"SAST_KS_MINR": "1000000000"}

CBS_CASES = [
    # ---- 1x1 stride 1 (row loaders; Cin / Cout on both sides of % 16; Cout = 4: one float4 per row; Ho == 1)
    _cbs(1, 1, (2, 5, 9), 4, 4),
    _cbs(1, 1, (2, 1, 9), 12, 12),
    _cbs(1, 1, (3, 13, 20), 20, 36),
    _cbs(1, 1, (1, 31, 33), 100, 132),
    _cbs(1, 1, (2, 24, 40), 20, 64),            # short reduction: the 1-k-group tile
    _cbs(1, 1, (1, 16, 16), 256, 48),
    _cbs(1, 1, (2, 24, 40), 32, 16),
    _cbs(1, 1, (1, 1, 7), 64, 128, "i"),
    _cbs(1, 1, (1, 1, 1), 32, 16, "i"),         # M = 1
    _cbs(1, 1, (2, 5, 9), 32, 36, cin1=12),     # two-source input 12 + 20
    _cbs(1, 1, (3, 13, 20), 144, 48, cin1=48),  # 48 + 96
    _cbs(1, 1, (2, 24, 40), 128, 128, cin1=64),  # 64 + 64
    _cbs(1, 1, (2, 5, 9), 32, 48, "t", two=True),
    _cbs(1, 1, (2, 5, 9), 32, 48),
    _cbs(1, 1, (2, 5, 9), 32, 48, "t", env={"SAST_BN_STATS_SEPARATE": "8"}, tag="statsep"),
    _cbs(1, 1, (3, 13, 20), 20, 36, tag="sat"),  # saturated SiLU
    # ---- 3x3 stride 1
    _cbs(3, 1, (1, 16, 16), 64, 64),            # tiny tile forward
    _cbs(3, 1, (2, 24, 40), 32, 128),           # thin tile
    _cbs(3, 1, (2, 80, 80), 32, 128, "t"),      # nb = 400: the 2-k-group tile; BatchNorm apply kernels with iters = 3, ragged last block
    _cbs(3, 1, (2, 80, 80), 128, 32, "t"),      # dX job with nb = 400: the 2-k-group tile inside the pair
    _cbs(3, 1, (2, 5, 9), 4, 12),
    _cbs(3, 1, (2, 1, 9), 12, 4),
    _cbs(3, 1, (3, 13, 20), 20, 36),
    _cbs(3, 1, (1, 31, 33), 100, 16),
    _cbs(3, 1, (2, 5, 9), 256, 132),
    _cbs(3, 1, (1, 1, 7), 12, 36, "i"),
    _cbs(3, 1, (1, 1, 1), 64, 16, "i"),         # M = 1, every tap but the centre is padding
    _cbs(3, 1, (2, 5, 9), 32, 48, "t", two=True),
    _cbs(3, 1, (1, 16, 16), 64, 64, "ti", env=ENV_K2, tag="forceK2"),
    _cbs(3, 1, (1, 16, 16), 64, 64, "ti", env=ENV_THIN, tag="forceThin"),
    _cbs(3, 1, (2, 24, 40), 32, 128, "ti", env=ENV_K1, tag="forceK1"),
    _cbs(3, 1, (3, 13, 20), 20, 36, "t", env={"SAST_GEMM_PAIR": "0"}, tag="nopair"),
    _cbs(3, 1, (2, 5, 9), 4, 12, tag="sat"),     # (a short reduction: the gain of 8 multiplies the rounding of the conv sum as well)
    # ---- 3x3 stride 2: the parity-class dX (even H, W and Mc = B (H/2) (W/2) a multiple of 64) and the generic gather (everything else)
    _cbs(3, 2, (2, 16, 32), 32, 48),            # Mc = 256
    _cbs(3, 2, (1, 32, 48), 12, 36),            # Mc = 384
    _cbs(3, 2, (1, 6, 10), 4, 16),              # Mc = 15
    _cbs(3, 2, (3, 10, 14), 20, 12),            # Mc = 105
    _cbs(3, 2, (2, 24, 40), 64, 128),           # Mc = 480: the B = 2 PAFPN shape does not take the parity form
    _cbs(3, 2, (2, 5, 9), 32, 36),
    _cbs(3, 2, (3, 13, 20), 100, 48),
    _cbs(3, 2, (1, 31, 33), 12, 132),
    _cbs(3, 2, (2, 1, 9), 64, 16),              # Ho == 1
    _cbs(3, 2, (1, 1, 7), 20, 4, "i"),
    # ---- 1x1 stride 2, 3x3 stride 4 (reachable through the wrappers)
    _cbs(1, 2, (2, 5, 9), 4, 12),
    _cbs(1, 2, (3, 13, 20), 32, 48),
    _cbs(1, 2, (2, 24, 40), 100, 16),
    _cbs(1, 2, (2, 1, 9), 64, 36),
    _cbs(1, 2, (1, 16, 16), 20, 128),
    _cbs(1, 2, (1, 1, 7), 12, 4, "i"),
    _cbs(3, 4, (2, 5, 9), 12, 16),
    _cbs(3, 4, (3, 13, 20), 64, 36),
    _cbs(3, 4, (2, 24, 40), 20, 48),
    _cbs(3, 4, (1, 31, 33), 32, 132),
    _cbs(3, 4, (1, 16, 16), 256, 4),
    _cbs(3, 4, (3, 1, 9), 4, 4),                # Ho == 1
    _cbs(3, 4, (1, 1, 7), 64, 12, "i"),
]
PARITY_AB_CASE = "cbs-k3s2-2x16x32-32to48"      # also runs under SAST_CONVDX_PARITY=0; the two dX are compared with each other

DW_CASES = [
    _dw(1, (2, 5, 9), 4), _dw(1, (3, 13, 20), 48), _dw(1, (2, 24, 40), 64), _dw(1, (1, 31, 33), 100), _dw(1, (1, 16, 16), 256),
    _dw(2, (2, 5, 9), 256), _dw(2, (3, 13, 20), 100), _dw(2, (2, 24, 40), 48), _dw(2, (1, 31, 33), 64), _dw(2, (1, 16, 16), 4),
    _dw(1, (1, 1, 1), 48, "i"), _dw(2, (1, 1, 7), 64, "i"),
]


def _chain(name, bhw, cin, units, join=False):
    """units: (k, stride, Cout).  join False: a sequence, every conv the sole consumer of its predecessor's output.  join True: units
    0 and 1 both read x, unit 2 (1x1) reads the pair (y0, y1) as a two-source input and is the sole consumer of both."""
    B, H, W = bhw
    return dict(id=f"chain-{name}-{B}x{H}x{W}-{cin}-" + "-".join(f"k{k}s{s}c{c}" for k, s, c in units), op="chain", B=B, H=H, W=W, cin=cin,
                units=tuple(units), join=join, env={})


CHAIN_CASES = [
    _chain("seq", (2, 13, 20), 20, [(1, 1, 32), (3, 1, 36)]),       # 1x1 -> 3x3 s1 (generic dX loader + producer reduction)
    _chain("seq", (1, 16, 16), 64, [(1, 1, 64), (3, 1, 48)]),       # ... uniform-tap dX loader
    _chain("seq", (2, 16, 32), 32, [(3, 2, 48), (1, 1, 36)]),       # 3x3 s2 -> 1x1
    _chain("seq", (3, 13, 20), 12, [(3, 2, 20), (1, 1, 64)]),
    _chain("join", (2, 9, 11), 12, [(3, 1, 20), (1, 1, 32), (1, 1, 48)], join=True),      # (conv, conv) -> two-source 1x1
    _chain("join", (2, 24, 40), 32, [(1, 1, 64), (3, 1, 64), (1, 1, 36)], join=True),
]


def _cbs2(bhw, cin, cout, cin1=0):
    B, H, W = bhw
    return dict(id=f"cbs2-{B}x{H}x{W}-{cin}to{cout}" + (f"-src{cin1}" if cin1 else ""), op="cbs2", B=B, H=H, W=W, cin=cin, cout=cout,
                cin1=cin1, env={})


CBS2_CASES = [_cbs2((2, 13, 20), 32, 48), _cbs2((2, 5, 9), 32, 64, cin1=12), _cbs2((1, 16, 16), 64, 48), _cbs2((3, 13, 20), 144, 64, cin1=48)]


def _down(f, overlap, bhw, cin, cout, pe=False, u8=False):
    B, H, W = bhw
    return dict(id=f"down-f{f}{'o' if overlap else 'n'}-{B}x{H}x{W}-{cin}to{cout}" + ("-pe" if pe else "") + ("-u8" if u8 else ""), op="down",
                f=f, overlap=overlap, B=B, H=H, W=W, cin=cin, cout=cout, pe=pe, u8=u8, env={})


DOWN_CASES = [
    # overlap, f = 2: 3x3 stride 2 with replicate padding -- the parity-class dX with its replicate fold when Mc % 64 == 0
    _down(2, True, (1, 8, 8), 4, 32, pe=True), _down(2, True, (2, 24, 40), 32, 64), _down(2, True, (1, 64, 48), 64, 128, pe=True),
    _down(2, True, (3, 12, 28), 20, 48), _down(2, True, (2, 16, 32), 32, 96, pe=True), _down(2, True, (1, 64, 48), 4, 256),
    _down(2, True, (1, 8, 8), 64, 192),
    # overlap, f = 4: 7x7 stride 4, replicate padding 3
    _down(4, True, (1, 8, 8), 20, 32), _down(4, True, (3, 12, 28), 4, 64, pe=True), _down(4, True, (2, 24, 40), 20, 64, pe=True),
    _down(4, True, (1, 64, 48), 32, 96), _down(4, True, (1, 8, 8), 64, 256, pe=True), _down(4, True, (2, 24, 40), 32, 128),
    _down(4, True, (3, 12, 28), 64, 192),
    # no overlap (k = f, no padding), also at sizes that are not multiples of the factor (floor on both sides)
    _down(2, False, (1, 8, 8), 20, 48, pe=True), _down(2, False, (3, 12, 28), 32, 128), _down(2, False, (2, 24, 40), 4, 192, pe=True),
    _down(2, False, (2, 9, 13), 20, 64), _down(2, False, (1, 65, 47), 64, 32, pe=True),
    _down(4, False, (1, 64, 48), 20, 96), _down(4, False, (2, 24, 40), 64, 256, pe=True), _down(4, False, (3, 13, 30), 4, 64, pe=True),
    _down(4, False, (2, 26, 41), 32, 48),
    # the stem on the stored uint8 event tensor (weight gradient only)
    _down(4, True, (2, 24, 40), 20, 64, pe=True, u8=True), _down(2, True, (1, 64, 48), 4, 32, u8=True), _down(4, False, (3, 12, 28), 20, 48, u8=True),
]


def _dwc(k, bhw, c, bias=True, c0=0, cw=0):
    B, H, W = bhw
    return dict(id=f"dwconv-k{k}-{B}x{H}x{W}-{c}" + ("" if bias else "-nobias") + (f"-win{c0}of{cw}" if cw else ""), op="dwconv", k=k, B=B, H=H,
                W=W, c=c, bias=bias, c0=c0, cw=cw or c, env={})


DWCONV_CASES = [
    _dwc(1, (2, 5, 9), 4), _dwc(1, (1, 1, 1), 256, bias=False), _dwc(3, (1, 1, 1), 48), _dwc(3, (2, 24, 40), 64, bias=False),
    _dwc(5, (2, 5, 9), 256), _dwc(5, (1, 7, 3), 48, bias=False), _dwc(5, (2, 24, 40), 256), _dwc(7, (1, 7, 3), 64),      # k = 7 larger than the map
    _dwc(7, (2, 24, 40), 4), _dwc(7, (2, 5, 9), 48, bias=False), _dwc(3, (2, 5, 9), 64, c0=32, cw=128), _dwc(7, (1, 7, 3), 48, c0=4, cw=64),
    _dwc(5, (2, 24, 40), 4, bias=False, c0=8, cw=12),
]


def _cat(op, bhw, c1, c2):
    B, H, W = bhw
    return dict(id=f"{op}-{B}x{H}x{W}-{c1}+{c2}", op=op, B=B, H=H, W=W, c1=c1, c2=c2, env={})


CAT_CASES = [_cat(op, bhw, c1, c2) for op in ("upcat", "cat2")
             for bhw, (c1, c2) in zip(((2, 5, 9), (1, 7, 3), (3, 13, 11)), ((4, 4), (12, 100), (64, 128)))]

ALL_CASES = CBS_CASES + DW_CASES + CHAIN_CASES + CBS2_CASES + DOWN_CASES + DWCONV_CASES + CAT_CASES
BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES), "duplicate case ids"


def bounds_id(case):
    """cases that differ only in the library knobs they run under are the same arithmetic: they share the fp32 figures of the plain case"""
    cid = case["id"]
    for tag in ("-forceK2", "-forceThin", "-forceK1", "-nopair", "-statsep"):
        cid = cid.replace(tag, "")
    return cid


# ------------------------------------------------------------------------------------------------ inputs
def _unit_params(g, cin, cout, k, dw=False, prefix=""):
    fan = k * k * (1 if dw else cin)
    return {prefix + "w": torch.randn(cout, 1 if dw else cin, k, k, generator=g) / math.sqrt(fan),
            prefix + "bn_w": 1 + 0.1 * torch.randn(cout, generator=g), prefix + "bn_b": 0.1 * torch.randn(cout, generator=g),
            prefix + "run_mean": 0.1 * torch.randn(cout, generator=g), prefix + "run_var": 0.5 + torch.rand(cout, generator=g)}


def make_inputs(case):
    g = SW.gen(bounds_id(case))
    op = case["op"]
    B, H, W = case["B"], case["H"], case["W"]
    if op in ("cbs", "cbs_dw"):
        k, s, cin, cout, cin1 = case["k"], case["s"], case["cin"], case["cout"], case["cin1"]
        Ho, Wo = conv_hw(H, W, k, s)
        inp = {"x": torch.randn(B, H, W, cin1 or cin, generator=g)}
        if cin1:
            inp["x2"] = torch.randn(B, H, W, cin - cin1, generator=g)
        inp.update(_unit_params(g, cin, cout, k, case["dw"]))
        if case.get("sat"):
            inp["bn_w"] = inp["bn_w"] * 8.0
            inp["bn_b"] = 4.0 * (1 - 2 * (torch.arange(cout) % 2)).float()
        inp["g"] = SW.up(g, B, Ho, Wo, cout)
        if case["two"]:
            inp["g2"] = SW.up(g, B, Ho, Wo, cout)
        return inp
    if op == "chain":
        inp = {"x": torch.randn(B, H, W, case["cin"], generator=g)}
        c_prev, hw = case["cin"], (H, W)
        for i, (k, s, c) in enumerate(case["units"]):
            cin = c_prev
            if case["join"]:
                cin = case["cin"] if i < 2 else case["units"][0][2] + case["units"][1][2]
            inp.update(_unit_params(g, cin, c, k, prefix=f"u{i}."))
            if not (case["join"] and i < 2):
                hw = conv_hw(hw[0], hw[1], k, s)
            c_prev = c
        if case["join"]:
            assert all(s == 1 for _k, s, _c in case["units"])
        inp["g"] = SW.up(g, B, hw[0], hw[1], c_prev)
        return inp
    if op == "cbs2":
        cin, cout, cin1 = case["cin"], case["cout"], case["cin1"]
        inp = {"x": torch.randn(B, H, W, cin1 or cin, generator=g)}
        if cin1:
            inp["x2"] = torch.randn(B, H, W, cin - cin1, generator=g)
        inp.update(_unit_params(g, cin, cout, 1, prefix="u0."))
        inp.update(_unit_params(g, cin, cout, 1, prefix="u1."))
        inp["g0"], inp["g1"] = SW.up(g, B, H, W, cout), SW.up(g, B, H, W, cout)
        return inp
    if op == "down":
        f, cin, cout = case["f"], case["cin"], case["cout"]
        k = 2 * f - 1 if case["overlap"] else f
        Ho, Wo = H // f, W // f
        if case["u8"]:      # event counts: mostly 0, a few up to 255
            x = (torch.rand(B, H, W, cin, generator=g) < 0.15) * torch.randint(1, 256, (B, H, W, cin), generator=g)
            x = x.to(torch.uint8)
        else:
            x = torch.randn(B, H, W, cin, generator=g)
        inp = {"x": x, "w": torch.randn(cout, cin, k, k, generator=g) / math.sqrt(k * k * cin),
               "ln_w": 1 + 0.1 * torch.randn(cout, generator=g), "ln_b": 0.1 * torch.randn(cout, generator=g)}
        if case["pe"]:
            inp["pe"] = torch.randn(Ho * Wo, cout, generator=g)
        inp["g"] = SW.up(g, B, Ho, Wo, cout)
        return inp
    if op == "dwconv":
        k, c, cw = case["k"], case["c"], case["cw"]
        inp = {"x": torch.randn(B, H, W, c, generator=g), "w": torch.randn(cw, 1, k, k, generator=g) / k}
        if case["bias"]:
            inp["b"] = 0.1 * torch.randn(cw, generator=g)
        inp["g"] = SW.up(g, B, H, W, c)
        return inp
    if op in ("upcat", "cat2"):
        c1, c2 = case["c1"], case["c2"]
        up = 2 if op == "upcat" else 1
        return {"a": torch.randn(B, H, W, c1, generator=g), "b": torch.randn(B, up * H, up * W, c2, generator=g),
                "g": SW.up(g, B, up * H, up * W, c1 + c2)}
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------ reference evaluation
NO_GRAD = ("g", "g0", "g1", "g2", "run_mean", "run_var", "pe")


def _leaves(inp, dtype, grads=True):
    return SW.leaves(inp, dtype, NO_GRAD, grads)


def _unit(p, prefix=""):
    return tuple(p[prefix + n] for n in ("w", "bn_w", "bn_b", "run_mean", "run_var"))


def reference(case, inp, dtype):
    op, out = case["op"], {}
    if op in ("cbs", "cbs_dw"):
        for mode in case["modes"]:
            p = _leaves(inp, dtype, mode != "infer")
            x = (p["x"], p["x2"]) if "x2" in p else p["x"]
            y, rm, rv = R.conv_bn_silu(x, *_unit(p), case["k"], case["s"], mode)
            out[f"{mode}/out:y"] = y.detach()
            if mode == "train":
                out["train/stat:run_mean"], out["train/stat:run_var"] = rm, rv
            if mode != "infer":
                loss = (y * p["g"]).sum() + ((y * p["g2"]).sum() if case["two"] else 0)
                loss.backward()
                SW.grads(out, p, mode + "/")
        return out
    if op == "chain":
        p = _leaves(inp, dtype)
        us = case["units"]
        if case["join"]:
            y0, m0, v0 = R.conv_bn_silu(p["x"], *_unit(p, "u0."), us[0][0], us[0][1], "train")
            y1, m1, v1 = R.conv_bn_silu(p["x"], *_unit(p, "u1."), us[1][0], us[1][1], "train")
            y, m2, v2 = R.conv_bn_silu((y0, y1), *_unit(p, "u2."), us[2][0], us[2][1], "train")
            stats = [(m0, v0), (m1, v1), (m2, v2)]
        else:
            y, stats = p["x"], []
            for i, (k, s, _c) in enumerate(us):
                y, m, v = R.conv_bn_silu(y, *_unit(p, f"u{i}."), k, s, "train")
                stats.append((m, v))
        out["train/out:y"] = y.detach()
        for i, (m, v) in enumerate(stats):
            out[f"train/stat:u{i}.run_mean"], out[f"train/stat:u{i}.run_var"] = m, v
        (y * p["g"]).sum().backward()
        SW.grads(out, p, "train/")
        return out
    if op == "cbs2":
        p = _leaves(inp, dtype)
        x = (p["x"], p["x2"]) if "x2" in p else p["x"]
        loss = 0
        for i in (0, 1):
            y, m, v = R.conv_bn_silu(x, *_unit(p, f"u{i}."), 1, 1, "train")
            out[f"train/out:y{i}"] = y.detach()
            out[f"train/stat:u{i}.run_mean"], out[f"train/stat:u{i}.run_var"] = m, v
            loss = loss + (y * p[f"g{i}"]).sum()
        loss.backward()
        SW.grads(out, p, "train/")
        return out
    if op == "down":
        p = _leaves(inp, dtype)
        y = R.downsample_ln(p["x"], p["w"], p["ln_w"], p["ln_b"], p.get("pe"), case["f"])
        out["train/out:y"] = y.detach()
        (y * p["g"]).sum().backward()
        SW.grads(out, p, "train/")
        return out
    if op == "dwconv":
        p = _leaves(inp, dtype)
        y = R.dwconv(p["x"], p["w"], p.get("b"), case["c0"])
        out["train/out:y"] = y.detach()
        (y * p["g"]).sum().backward()
        SW.grads(out, p, "train/")
        return out
    if op in ("upcat", "cat2"):
        p = _leaves(inp, dtype)
        y = (R.upsample_cat if op == "upcat" else R.cat2)(p["a"], p["b"])
        out["train/out:y"] = y.detach()
        (y * p["g"]).sum().backward()
        SW.grads(out, p, "train/")
        return out
    raise KeyError(op)


def pool_key(quantity):
    """the units of a chain / stacked pair pool their figures: u0.w, u1.w, ... -> u.w"""
    return re.sub(r"u\d\.", "u.", quantity)


BOUNDS_CASES = [c for c in ALL_CASES if bounds_id(c) == c["id"]]      # the cases with an entry of their own in the bounds file
float_quantities = sorted
DISCRETE = ()
