"""CPU tests of the attention sweep's own instruments (no GPU): the stand-alone expression of tests/attn_reference.py against the oracle
lines it restates (oracle/sast_oracle.py:260-268; on full windows, and in the padded -1e4 formulation on ragged selections) and against
F.scaled_dot_product_attention, the case table of tests/attn_cases.py with the input conditions it is stated under, and what the
committed fp32 bounds (tests/golden/attn_operator_bounds.json) hold per case (tests/test_operator_bounds.py regenerates them).
"""
import pytest
import torch
import torch.nn.functional as F

import attn_cases as AC
import attn_reference as R
import operator_sweep as SW
import token_reference as TR


def _close(a, b, rtol, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = float((a - b).abs().max()), max(float(b.abs().max()), 1e-30)
    assert err <= rtol * scale, f"{what}: {err:.3e} of {scale:.3e}"


def _oracle_lines(x_qkv, heads, dh, index_token=None, padding_index=None, rows=None):
    """oracle/sast_oracle.py:260-268 on qkv (M, Kmax, 3C); with index lists, the column mask of lines 263-266"""
    M = x_qkv.shape[0]
    q, k, v = x_qkv.view(M, -1, heads, dh * 3).transpose(1, 2).chunk(3, dim=3)
    attn = (q @ k.transpose(-2, -1)) * (dh ** -0.5)
    if index_token is not None:
        Kmax = q.shape[2]
        amap = torch.zeros((rows, Kmax, heads), dtype=attn.dtype)
        amap[index_token] = attn.transpose(1, 3).reshape(-1, Kmax, heads)
        amap[padding_index] = -1e4
        attn = amap[index_token].view(M, -1, Kmax, heads).transpose(1, 3)
    attn = attn.softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(M, -1, heads * dh)


@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 2e-6), (torch.float64, 1e-14)])
@pytest.mark.parametrize("C,dh", [(64, 32), (24, 8), (48, 24)])
def test_expression_reproduces_the_oracle_lines_on_full_windows(dtype, rtol, C, dh):
    M, T = 3, 20
    qkv = torch.randn(M, T, 3 * C, generator=SW.gen(f"full-{C}-{dh}")).to(dtype)
    o, lse = R.attention(qkv.view(M * T, 3 * C), [T] * M, dh)
    _close(o.view(M, T, C), _oracle_lines(qkv, C // dh, dh), rtol, "o")
    q, k, _v = R.split_qkv(qkv.view(M * T, 3 * C), dh)
    s = torch.einsum("mihd,mjhd->mhij", q.reshape(M, T, -1, dh), k.reshape(M, T, -1, dh)) * dh ** -0.5
    _close(lse.view(M, T, -1), s.exp().sum(-1).log().transpose(1, 2), rtol, "lse")


@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 2e-6), (torch.float64, 1e-14)])
def test_expression_reproduces_the_padded_formulation_on_ragged_selections(dtype, rtol):
    """the oracle gathers Kmax rows per kept window (the kept slots, then fillers), masks the filler KEYS with -1e4 and keeps the kept
    queries; the compact-row expression on the kept rows alone gives the same numbers (exp(-1e4 - max) is exactly 0)"""
    T, C, dh = 20, 64, 16
    g = SW.gen("ragged")
    kept = {0: list(range(T)), 1: [4], 3: sorted(torch.randperm(T, generator=g)[:13].tolist()), 4: sorted(torch.randperm(T, generator=g)[:7].tolist())}
    _iw, index_token, padding_index, asy_index, K = TR.index_lists(kept, T)
    M = len(kept)
    assert K.tolist() == [20, 1, 13, 7] and padding_index.numel() == M * T - int(K.sum())
    slots = torch.randn(M * T, 3 * C, generator=g).to(dtype)          # qkv of every slot of the kept windows
    x = _oracle_lines(slots[index_token].view(M, -1, 3 * C), C // dh, dh, index_token, padding_index, M * T)
    XX = torch.zeros(M * T, C, dtype=dtype)
    XX[index_token] = x.view(-1, C)
    o, _lse = R.attention(slots[asy_index], K.tolist(), dh)
    _close(o, XX[asy_index], rtol, "o")


@pytest.mark.parametrize("cid", ["attn-t60-c64-dh32", "attn-t80-c12-dh4", "attn-peaked-t96-c24-dh8"])
def test_expression_agrees_with_scaled_dot_product_attention(cid):
    case = AC.BY_ID[cid]
    qkv, dh = AC.make_inputs(case)["qkv"].double(), case["dh"]
    o, lse = R.attention(qkv, case["Ks"], dh)
    q, k, v = R.split_qkv(qkv, dh)
    r0 = 0
    for K in case["Ks"]:
        sl = slice(r0, r0 + K)
        if K:
            want = F.scaled_dot_product_attention(q[sl].transpose(0, 1), k[sl].transpose(0, 1), v[sl].transpose(0, 1))
            _close(o[sl].view(K, -1, dh), want.transpose(0, 1), 1e-13, f"o of the group at row {r0}")
        r0 += K
    assert r0 == o.shape[0] == lse.shape[0] and lse.shape[1] == case["C"] // dh


def test_gradients_are_those_of_the_written_out_backward():
    """dV = P^T dO, dS = P (dP - D), dQ = dS K / sqrt(dh), dK = dS^T Q / sqrt(dh): what the kernels evaluate, against autograd"""
    case = AC.BY_ID["attn-t60-c24-dh8"]
    inp = AC.make_inputs(case)
    ref, dh = AC.reference(case, inp, torch.float64), case["dh"]
    q, k, v = R.split_qkv(inp["qkv"].double(), dh)
    do = inp["dout"].double().view(-1, case["C"] // dh, dh)
    r0 = 0
    for K in case["Ks"]:
        sl = slice(r0, r0 + K)
        for h in range(case["C"] // dh if K else 0):
            P = torch.softmax(q[sl, h] @ k[sl, h].t() / dh ** 0.5, 1)
            dP = do[sl, h] @ v[sl, h].t()
            dS = P * (dP - (P * dP).sum(1, keepdim=True))
            _close(ref["grad:v"][sl, h], P.t() @ do[sl, h], 1e-12, "dv")
            _close(ref["grad:q"][sl, h], dS @ k[sl, h] / dh ** 0.5, 1e-12, "dq")
            _close(ref["grad:k"][sl, h], dS.t() @ q[sl, h] / dh ** 0.5, 1e-12, "dk")
        r0 += K


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_covers_every_kernel_tile_count_head_width_and_knob_value():
    cases = AC.ALL_CASES
    assert {AC.dispatch_class(c["T"]) for c in cases} == {2, 3, 4, 8}
    for cls, (lo, hi) in {2: (1, 64), 3: (65, 96), 4: (97, 128), 8: (129, 256)}.items():
        Ts = {c["T"] for c in cases if AC.dispatch_class(c["T"]) == cls}
        assert hi in Ts and any(lo <= T < hi for T in Ts), cls
        tiles = {(K + 31) // 32 for c in cases if AC.dispatch_class(c["T"]) == cls for K in c["Ks"] if K}
        # every body of the switch; the big kernels loop over the tiles: every trip count their class adds, the smaller ones somewhere
        assert tiles == set(range(1, cls + 1)) if cls < 8 else {5, 6, 7, 8} <= tiles, (cls, tiles)
    allK = {K for c in cases for K in c["Ks"]}
    for n in range(1, 5):       # either side of every multiple of 32 up to 128, and the multiple itself
        assert {32 * n - 1, 32 * n, 32 * n + 1} <= allK, n
    assert {0, 1, 161, 193, 224, 225, 255, 256} <= allK
    assert any(c["Ks"][-1] == 0 or 0 in c["Ks"][1:-1] for c in cases) and all(c["Ks"][0] == c["T"] for c in cases)
    for T in AC.KS:
        plain = [c for c in AC.GAUSS_CASES if c["T"] == T and not c["env"]]
        assert {c["dh"] for c in plain} == set(AC.DIM_HEADS) and {c["C"] // c["dh"] for c in plain} == {1, 2, 3}, T
        knob = [c for c in cases if c["T"] == T and c["env"]]
        assert len(knob) == (len([c for c in cases if c["T"] == T and not c["env"]]) if T <= 96 else 0)
        assert all(c["env"] == AC.NOSPLIT and AC.bounds_id(c) in AC.BY_ID and AC.bounds_id(c) != c["id"] for c in knob)
    peaked = [c for c in AC.PEAKED_CASES if not c["env"]]
    assert {AC.dispatch_class(c["T"]) for c in peaked if c["dh"] == 32} == {2, 3, 4, 8} and any(c["dh"] == 8 for c in peaked)
    assert any(c["T"] == 240 for c in peaked) and all(c["op"] == "attn_peaked" for c in peaked)
    assert all(c["op"] == "attn" for c in AC.GAUSS_CASES)


@pytest.mark.parametrize("case", AC.ALL_CASES, ids=SW.ids(AC.ALL_CASES))
def test_input_conditions_hold(case):
    AC.check_conditions(case, AC.make_inputs(case))


def test_the_tail_condition_refuses_inputs_without_a_late_maximum():
    case = AC.BY_ID["attn-peaked-t240-c64-dh32"]
    inp = AC.make_inputs(case)
    AC.check_conditions(case, inp)
    flat = dict(inp, qkv=inp["qkv"] / 2)       # the Gaussian logits: neither the spread nor the depth
    with pytest.raises(AssertionError):
        AC.check_conditions(case, flat)


# ------------------------------------------------------------------------------------------------ the committed bounds
bounds = SW.bounds_fixture("attn")


def test_bounds_hold_every_compared_quantity_and_stay_inside_the_project_bars(bounds):
    for case in AC.ALL_CASES:
        entry = bounds["cases"][AC.bounds_id(case)]
        assert set(entry) == set(AC.QUANTITIES), case["id"]
        for q, e in entry.items():
            assert 0.0 < e < SW.project_bar(q) / 2, (case["id"], q, e)
    assert set(bounds["operators"]) == {"attn", "attn_peaked"}
    for op, qs in bounds["operators"].items():
        for q, v in qs.items():
            assert v["median"] <= v["worst"] < SW.project_bar(q) / 2 and v["n"] >= 2, (op, q, v)
    # the Gaussian figures the sweep's bounds rest on: the fp32 reference is within 1e-6 on o and of the max-norm of every gradient
    for q, v in bounds["operators"]["attn"].items():
        assert v["worst"] < 1e-6, (q, v)
