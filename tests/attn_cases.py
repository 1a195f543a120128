"""The case table of the window-attention sweep (tests/test_attn_operators.py: the eleven kernels of csrc/k_attn_mfma.hip behind
attn_fwd_mfma_launch / attn_bwd_mfma_launch, reached on their own through sast_test_attn_fwd / sast_test_attn_bwd of the tools library),
the inputs of every case and its CPU reference.  The fifth suite of tests/operator_sweep.py ("attn"), shared by the GPU test, the bounds
generator and tests/test_attn_reference.py.  CPU only: nothing here imports the library.

A case is a partition size T (what the launchers dispatch on), a list of groups Ks in compact rows (0: a dropped group), a width C and a
dim_head.  Quantities: "out:o" (absolute), "rel:lse", "grad:q", "grad:k", "grad:v" (each relative to its own reference tensor's max-norm:
dqkv is split per operand so that an error in the smallest is not hidden by the max-norm of the largest).

  T      kernels                                                   Ks
  60     fwd<2>, bwd<2,split> / <2>                                both tile counts around 32, K = 1, a dropped group in the middle
  64     "                                                         the upper end of the class
  80     fwd<3>, bwd<3,split> / <3>                                three tiles around 64, a dropped group
  96     "                                                         the upper end
  100    fwd<4>, bwd<4>                                            the two-tile body of the four-wave kernels (K = 64, 33), which the lists
                                                                   of T = 120 and 128 do not reach
  120    "                                                         four tiles around 96, a dropped group
  128    "                                                         the upper end, K = 1 last
  240    attn_fwd_big, attn_bwd_big_q + attn_bwd_big_kv            five .. eight tiles around 128 / 192 / 224, every smaller count, a dropped group
  256    "                                                         the upper end
Each T at dim_head 4, 8, 16, 24 (C = 3 dim_head: three heads) and 32 (C = 32 and 64: one and two heads); every case with T <= 96 again
with SAST_ATTN_BWD_SPLIT=0 (the same arithmetic: it shares the plain case's bounds entry).

Inputs are randn (logit std 1).  The "peaked" cases (operator "attn_peaked", so that their figures do not move the Gaussian medians)
multiply the q and k columns by 2: logit std about 4, |lse| up to about 26 -- one per dispatch class at dim_head 32, one at dim_head 8,
and the T = 240 list, where `check_conditions` asserts on the float64 reference that some query of a group with K > 128 has its maximum
logit in the last key tile, at least 8 above the maximum of the first tile: the big kernel's running sum really is rescaled by a factor
of exp(-8) or less.  (At gain 4 the float32 reference itself is at 1.4e-5 on o, half the project's bar: the peaked cases stop at 2.)
"""
import torch

import attn_reference as R
import operator_sweep as SW

KS = {60: [60, 33, 32, 31, 1, 0, 17, 2], 64: [64, 63], 80: [80, 65, 64, 63, 0, 3, 40], 96: [96, 95, 33],
      100: [100, 64, 33], 120: [120, 97, 96, 95, 31, 0, 70], 128: [128, 127, 1], 240: [240, 225, 224, 193, 129, 128, 127, 100, 33, 32, 1, 0, 200],
      256: [256, 255, 161]}
DIM_HEADS = (4, 8, 16, 24, 32)
NOSPLIT = {"SAST_ATTN_BWD_SPLIT": "0"}
TAIL_DEPTH = 8.0        # the rescaling the T = 240 peaked case must contain: exp(-TAIL_DEPTH) or less on a running sum


def dispatch_class(T):
    return 2 if T <= 64 else 3 if T <= 96 else 4 if T <= 128 else 8


def _case(T, C, dh, peaked=False, env=None):
    name = f"attn-{'peaked-' if peaked else ''}t{T}-c{C}-dh{dh}"
    c = dict(id=name + ("-nosplit" if env else ""), op="attn_peaked" if peaked else "attn", T=T, Ks=KS[T], C=C, dh=dh, peaked=peaked,
             env=dict(env or {}), shares=name if env else None)
    return c


def _with_nosplit(cases):
    return [c for p in cases for c in ([p] + ([_case(p["T"], p["C"], p["dh"], p["peaked"], NOSPLIT)] if p["T"] <= 96 else []))]


GAUSS_CASES = _with_nosplit([_case(T, C, dh) for T in KS for dh in DIM_HEADS for C in ((3 * dh,) if dh < 32 else (32, 64))])
PEAKED_CASES = _with_nosplit([_case(T, 64, 32, True) for T in (60, 80, 120, 240)] + [_case(96, 24, 8, True)])
ALL_CASES = GAUSS_CASES + PEAKED_CASES
BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES), "duplicate case ids"
QUANTITIES = ("grad:k", "grad:q", "grad:v", "out:o", "rel:lse")


def bounds_id(case):
    """the sequential backward is the split one's arithmetic in the same order: the knob cases share the plain case's figures"""
    return case.get("shares") or case["id"]


def pool_key(quantity):
    return quantity


def make_inputs(case):
    g = SW.gen(bounds_id(case))
    rows, C, dh = sum(case["Ks"]), case["C"], case["dh"]
    qkv = torch.randn(rows, 3 * C, generator=g)
    if case["peaked"]:
        qkv.view(rows, C // dh, 3, dh)[:, :, :2] *= 2.0
    return {"qkv": qkv, "dout": SW.up(g, rows, C)}


def check_conditions(case, inp):
    T, Ks, C, dh = case["T"], case["Ks"], case["C"], case["dh"]
    assert max(Ks) == T <= 256 and min(Ks) >= 0 and C % dh == 0 and dh % 4 == 0 and 4 <= dh <= 32
    assert tuple(inp["qkv"].shape) == (sum(Ks), 3 * C) and tuple(inp["dout"].shape) == (sum(Ks), C)
    assert case["env"] in ({}, NOSPLIT) and (not case["env"] or T <= 96)
    s = R.logits(inp["qkv"].double(), Ks, dh)
    std = float(torch.cat([x.reshape(-1) for x in s]).std())
    assert (3.0 < std < 5.0) if case["peaked"] else (0.8 < std < 1.2), std
    if case["peaked"] and T == 240:
        depth = max(float((x[:, :, (K - 1) // 32 * 32:].max(2).values - x[:, :, :32].max(2).values).max())
                    for x, K in zip(s, [K for K in Ks if K]) if K > 128)
        assert depth >= TAIL_DEPTH, depth


def reference(case, inp, dtype):
    p = SW.leaves(inp, dtype, ("dout",))
    o, lse = R.attention(p["qkv"], case["Ks"], case["dh"])
    (o * p["dout"]).sum().backward()
    q, k, v = R.split_qkv(p["qkv"].grad, case["dh"])
    return {"out:o": o.detach(), "rel:lse": lse.detach(), "grad:q": q.clone(), "grad:k": k.clone(), "grad:v": v.clone()}


BOUNDS_CASES = [c for c in ALL_CASES if bounds_id(c) == c["id"]]
float_quantities = sorted
DISCRETE = ()
