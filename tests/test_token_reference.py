"""CPU tests of the token-path operator sweep's own instruments (no GPU): the stand-alone restatements of tests/token_reference.py
against the oracle lines they restate, the case table of tests/token_cases.py with the input conditions it is stated under, and what
the committed fp32 bounds (tests/golden/token_operator_bounds.json) hold per case (tests/test_operator_bounds.py regenerates them).

One figure of the bounds file is NOT inside the project's bar: the reference LayerNorm in float32 misses the 3e-5 output bar on the
ill-conditioned MS-WSA case (rows 30 + 0.1 randn: e32 = 3.1e-5; 3.1e-5 .. 4.5e-5 at the widths 32 .. 128) -- the mean of 64 values
near 30 carries a rounding error of about an ulp of 30 (1.9e-6), which the division by the spread of 0.1 turns into 2e-5 .. 4e-5 of
the normalised row.  Every other figure is below half its bar, as in the conv suite.
"""
import pytest
import torch

import operator_sweep as SW
import token_cases as TC
import token_reference as R
from oracle import sast_oracle as O

COND_CASE = "mswsa-c64-dh32-mix-cond"
SAT_CASE = "lstm-c256-given-sat"


def _close(a, b, rtol, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = float((a - b).abs().max()), max(float(b.abs().max()), 1e-30)
    assert err <= rtol * scale, f"{what}: {err:.3e} of {scale:.3e}"


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 2e-6), (torch.float64, 1e-14)])
@pytest.mark.parametrize("inf_rows", [False, True])
def test_scoring_expression_reproduces_the_oracle_block(dtype, rtol, inf_rows):
    """`score_stp` against what O.sast_block computes inline (oracle/sast_oracle.py:339-354): the pre-activation, the token scores
    (scores_win.sum(-1)) and the weighted x.  The block runs with empty forced selections, so neither attention layer touches the
    weighted x and the block returns it (in image layout)."""
    B, H, W, C, part = 2, 8, 10, 32, (4, 5)
    cfg = O.BackboneCfg(in_res_hw=(32, 40), partition_size=part, embed_dim=C, amp=2e-2)
    pre = "stages.0.att_blocks.0.att."
    g = torch.Generator().manual_seed(5)
    p = {k[len(pre):]: v.to(dtype) for k, v in O.init_backbone_params(cfg, seed=3, ls_init=0.5).items() if k.startswith(pre)}
    p["to_controls.weight"] = (1 + 0.1 * torch.randn(C, 20, generator=g)).to(dtype)
    if inf_rows:
        p["to_controls.weight"][[1, 7]] = -float("inf")
    x = torch.randn(B, H, W, C, generator=g).to(dtype)
    pe = O.position_embedding_sine(H, W, C).to(dtype)
    r = (torch.rand(B, 20, generator=g) * torch.tensor([[0.02], [0.0]])).to(dtype)       # a quiet frame and an empty one
    empty = [torch.zeros(0, dtype=torch.long)] * 5
    kl = {}
    xw_o, _cnt, _lists, scores_win = O.sast_block(x, pe, r, p, "", cfg.attn, first_block=True, return_scores=True,
                                                  forced_lists=[empty, empty], kink_log=kl)
    xp = R.add_pos_embedding(x, pe)
    assert torch.equal(xp, x + pe[:, :H, :W, :].repeat(B, 1, 1, 1))
    xw, tok = R.score_stp(xp.view(B, H * W, C), r, p["to_scores.weight"], p["to_scores.bias"], p["to_controls.weight"], cfg.amp)
    assert bool(torch.isfinite(tok).all()) and bool(torch.isfinite(xw).all())
    N, T = H * W // 20, 20
    win = lambda t: O.window_partition(t, part).reshape(B, N, T, -1)      # noqa: E731
    _close(win(R.score_preact(xp, p["to_scores.weight"], p["to_scores.bias"])), kl[""][0]["z"], rtol, "z")
    _close(win(tok.view(B, H, W, 1))[..., 0], scores_win.sum(-1), rtol, "tok")
    _close(xw.view(B, H, W, C), xw_o, rtol, "xw")
    if inf_rows:        # scale = 0 there: no contribution to the token scores, weight 0.5 * sigmoid(s)
        s = torch.relu(R.score_preact(xp, p["to_scores.weight"], p["to_scores.bias"]))
        assert float(scores_win[..., [1, 7]].abs().max()) == 0.0
        assert torch.equal(xw.view(B, H, W, C)[..., [1, 7]], ((0.5 * s.sigmoid()) * xp)[..., [1, 7]])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_mask_token_and_pos_emb_expressions_reproduce_the_oracle_lines(dtype):
    """oracle/sast_oracle.py:428-430 (x[token_mask] = mask_token, before the block) followed by :339 (x + pe): the device order is the
    other way round (the rows already carry pe, a masked row becomes token + pe) -- the same numbers bit for bit"""
    B, H, W, C = 2, 4, 5, 8
    g = torch.Generator().manual_seed(1)
    x, pe = torch.randn(B, H, W, C, generator=g).to(dtype), torch.randn(1, H, W, C, generator=g).to(dtype)
    token = torch.randn(1, 1, 1, C, generator=g).to(dtype)
    mask = torch.rand(B, H, W, generator=g) < 0.3
    xo = x.clone()
    xo[mask] = token.to(xo.dtype)
    assert torch.equal(R.mask_token(x, mask, token), xo)
    want = xo + pe[:, :H, :W, :].repeat(B, 1, 1, 1)
    assert torch.equal(R.mask_token(R.add_pos_embedding(x, pe), mask, token, pe), want)
    assert torch.equal(R.mask_token(R.add_pos_embedding(x, pe), torch.zeros_like(mask), token, pe), x + pe)


def test_index_lists_are_the_oracles_selection():
    """the lists built from explicit kept slots are what oracle.select_tokens builds from scores that keep exactly those slots"""
    case = TC.BY_ID["mswsa-c64-dh32-mix"]
    kept = TC.kept_slots(case)
    iw, it, pad, asy, K = R.index_lists(kept, 20)
    assert iw.tolist() == sorted(kept) and K.tolist() == [len(kept[w]) for w in sorted(kept)]
    assert asy.tolist() == [m * 20 + t for m, w in enumerate(sorted(kept)) for t in kept[w]]
    assert it.numel() == len(kept) * 20 and set(asy.tolist()) <= set(it.tolist())
    assert sorted(pad.tolist()) == sorted(set(it.tolist()) - set(asy.tolist()))


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_covers_what_the_sweep_is_about():
    sc = [c for c in TC.SCORE_CASES if c["kind"] == "exact"]
    assert {c["C"] for c in sc if (c["B"], c["L"]) == (3, 33)} == set(TC.WIDTHS)
    assert {c["L"] for c in sc if c["C"] == 32} >= {7, 33, 1030, 8200} and {(c["C"], c["B"]) for c in sc} >= {(96, 1), (768, 1)}
    assert {c["amp"] for c in sc} == set(TC.AMPS) == {c["amp"] for c in sc if c["C"] == 64}
    assert {c["C"] for c in TC.SCORE_CASES if c["kind"] == "gauss"} == {64, 192, 1024}
    assert [c["C"] for c in TC.SCORE_CASES if c["kind"] == "inf"] == [64]
    ms = TC.MSWSA_CASES
    plain = [c for c in ms if c["id"].endswith("-mix") and not c["fused"]]
    assert {c["C"] for c in plain} == set(TC.WIDTHS) and {c["dh"] for c in plain if c["C"] == 64} == {8, 16, 32}
    assert all(c["inner"] == O.mlp_inner_dim(c["C"]) and c["C"] % c["dh"] == 0 for c in ms)
    assert {(c["C"], c["dh"]) for c in plain} >= {(48, 24), (96, 16)}
    assert sorted((c["fused"], c["nograd"]) for c in ms if c["fused"]) == [(True, False), (True, True)]
    assert {c["C"] for c in ms if c["env"].get("SAST_LN_BLOCKS") == "1"} == {32, 192, 1024}
    for C in (48, 192):
        feats = [c for c in ms if c["C"] == C]
        assert any(not c["ls"] for c in feats) and any(c["cb"] for c in feats) and any(c["drop"] for c in feats) and any(c["act"] == "prelu" for c in feats)
    assert sum(c["cond"] for c in ms) == 1 and any(c["sel"] == "empty2" for c in ms)
    pt = TC.PART_CASES
    assert all(c["op"] == "mswsa_part" and c["B"] == 1 for c in pt) and all(c["op"] == "mswsa" and c["T"] == 20 for c in ms)
    assert {c["T"] for c in pt} == {60, 80, 120, 240} == set(TC.PART_KS) and all(max(TC.PART_KS[T]) == T for T in TC.PART_KS)
    for T in TC.PART_KS:        # every tile count up to the partition's, through the class's own kernels; two widths
        tiles = {(K + 31) // 32 for K in TC.PART_KS[T]}
        assert tiles >= ({1, 2} if T == 60 else {1, 2, 3} if T == 80 else {1, 3, 4} if T == 120 else {2, 4, 5, 8}), T
        assert len({c["C"] for c in pt if c["T"] == T and not c["shares"]}) == 2, T
        knob = {c["C"] for c in pt if c["T"] == T and c["env"] == TC.NOSPLIT}
        assert knob == ({c["C"] for c in pt if c["T"] == T} if T <= 96 else set()), T
    assert any((2 * c["C"]) % 6 and (2 * c["C"]) % 3 for c in pt if c["T"] == 80)          # a ragged last side block: wpb2 = 6, wpb = 3
    assert sorted((c["T"], c["nograd"]) for c in pt if c["fused"]) == [(80, False), (80, True), (120, False), (120, True)]
    assert all(c["C"] == 64 and c["dh"] == 32 and TC.BY_ID[c["shares"]]["C"] == 64 for c in pt if c["fused"])
    assert [(c["T"], c["C"]) for c in pt if c["peaked"]] == [(240, 64)] and not any(c.get("peaked") for c in ms)
    assert all(TC.BY_ID[c["shares"]]["T"] == c["T"] and not TC.BY_ID[c["shares"]]["shares"] for c in pt if c["shares"])
    assert {(c["C"], c["pattern"]) for c in TC.MASK_CASES if c["pe"]} == {(C, p) for C in (32, 48, 1024) for p in ("none", "all", "every257")}
    assert any(not c["pe"] for c in TC.MASK_CASES) and {c["C"] for c in TC.ADDPOS_CASES} == {32, 48, 1024}
    ac = TC.MSWSA_ACT_CASES       # every activation code but gelu and prelu (which `mswsa` runs), at both widths, with saturating gates
    from sast_amd.functional import GLU_ACTIVATIONS
    assert {GLU_ACTIVATIONS[c["act"]] for c in ac} == set(range(14)) - {GLU_ACTIVATIONS["gelu"], GLU_ACTIVATIONS["prelu"]} and len(ac) == 24
    assert {(c["act"], c["C"], c["dh"]) for c in ac} == {(a, C, dh) for a in TC.ACT_KINKS for C, dh in ((48, 24), (192, 32))}
    assert all(c["op"] == "mswsa_act" and c["sel"] == "mix" and c["B"] == 2 and c["T"] == 20 and c["gate_gain"] == TC.GATE_GAIN and not c["shares"] for c in ac)
    assert all(c["gate_gain"] == 1.0 for c in ms + pt)
    assert {k for ks in TC.ACT_KINKS.values() for k in ks} == {0.0, 6.0, 3.0, -3.0, -2.0}
    ls = TC.LSTM_CASES
    assert {(c["C"], c["state"]) for c in ls} >= {(C, s) for C in TC.WIDTHS for s in ("given", "none", "zero")}
    assert {c["C"] for c in ls if c["two"]} == {48, 256} == {c["C"] for c in ls if c["drop"]}
    assert [(c["C"], c["state"]) for c in ls if c["sat"]] == [(48, "given"), (256, "given")]
    # the k-split group tiles through the operators: same inputs and bounds entry as the plain case
    assert {c["C"] for c in ms if c["env"] == TC.GLU_TILE} == {256, 512}
    assert {(c["C"], c["state"]) for c in ls if c["env"] == TC.LSTM_TILE} == {(256, "given"), (256, "none")}
    for c in ms + ls:
        if c["env"] in (TC.GLU_TILE, TC.LSTM_TILE):
            plain = TC.BY_ID[c["shares"]]
            assert not plain["env"] and not plain.get("shares") and all(torch.equal(a, b) for a, b in zip(TC.make_inputs(c).values(), TC.make_inputs(plain).values()))


@pytest.mark.parametrize("case", TC.ALL_CASES, ids=[c["id"] for c in TC.ALL_CASES])
def test_input_conditions_hold(case):
    """what the cases are stated under (exact-gate inputs: min |z| >= 1/256 on the float64 reference, the r slice, the -inf control rows,
    the selections, the mask patterns, the row counts)"""
    TC.check_conditions(case, TC.make_inputs(case))


def test_the_gate_conditions_refuse_unsaturated_gates_and_an_element_on_a_kink():
    case = TC.BY_ID["mswsa-c48-dh24-mix-relu6-s0"]
    inp, inner = TC.make_inputs(case), case["inner"]
    TC.check_conditions(case, inp)
    plain = dict(inp, fc1_w=inp["fc1_w"].clone(), fc1_b=inp["fc1_b"].clone())       # the gates of the Gaussian recipe: nothing reaches 6
    plain["fc1_w"][inner:] /= TC.GATE_GAIN
    plain["fc1_b"][inner:] /= TC.GATE_GAIN
    with pytest.raises(AssertionError):
        TC.check_conditions(case, plain)
    gate = TC.gate_preactivations(case, inp)
    on = dict(inp, fc1_b=inp["fc1_b"].clone())       # one gate element moved onto the clamp
    on["fc1_b"][inner + 5] += float(6.0 - gate[7, 5])
    assert abs(float(TC.gate_preactivations(case, on)[7, 5]) - 6.0) < 1e-6
    with pytest.raises(AssertionError):
        TC.check_conditions(case, on)


# ------------------------------------------------------------------------------------------------ the committed bounds
bounds = SW.bounds_fixture("token")


def test_bounds_hold_every_compared_quantity_and_stay_inside_the_project_bars(bounds):
    for case in TC.ALL_CASES:
        entry = bounds["cases"][TC.bounds_id(case)]
        want = {"score": {"exact": {"out:xw", "rel:tok", "grad:xp", "grad:ws_w", "grad:ws_b", "grad:wc"}, "gauss": {"out:xw", "rel:tok", "grad:wc"},
                          "inf": {"out:xw", "rel:tok"}}.get(case.get("kind")),
                "mask_token": {"out:y", "grad:x", "grad:token"}, "add_pos": {"out:y", "grad:x"}}.get(case["op"])
        if case["op"] == "lstm":
            want = {"out:h1", "out:c1", "grad:x", "grad:w", "grad:b"} | {f"grad:{s}" for s in ("h0", "c0") if
                                                                         (s == "h0" and case["state"] != "none") or (s == "c0" and case["state"] in ("given", "zero"))}
        if case["op"] in TC.MSWSA_OPS:
            want = {"out:y", "grad:x"} | {f"grad:{k}" for k in R.MSWSA_NAMES if k != "act_w" and (case["ls"] or k not in ("ls1", "ls2"))}
            if case["act"] == "prelu":
                want.add("grad:act_w")
        assert set(entry) == want, case["id"]
        assert set(TC.compared(case, entry)) == ({"out:y"} if case.get("nograd") else want)
        for q, e in entry.items():
            med = bounds["operators"][case["op"]][TC.pool_key(q)]["median"]
            assert e >= 0.0 and med >= 0.0
            exact = q in TC.EXACT.get(case["op"], ()) or (case.get("pattern") == "none" and q == "grad:token")
            if not exact:       # (copies, single adds and an empty sum: the GPU test asks for bit equality with the float32 reference there)
                assert e > 0.0, (case["id"], q)
            if not ((TC.bounds_id(case) == COND_CASE and q == "out:y") or (case["id"] == SAT_CASE and q == "out:c1")):
                assert e < SW.project_bar(q) / 2, (case["id"], q, e)
    assert 3e-5 < bounds["cases"][COND_CASE]["out:y"] < 4e-5        # the figure of the module docstring
    assert 1.5e-5 < bounds["cases"][SAT_CASE]["out:c1"] < 2.5e-5     # |c1| up to 15 from 512-term gate sums times 8: fp32 itself is past half the bar
    for op, qs in bounds["operators"].items():
        for q, v in qs.items():
            assert v["median"] <= v["worst"] and v["median"] < SW.project_bar(q) / 2 and v["n"] >= 2, (op, q, v)
