"""CPU tests of the selection sweep's own instruments (no GPU): the restatement of tests/selection_reference.py against the oracle's
select_windows / select_tokens in both precisions, the structure of its compaction and packs, the case table of tests/selection_cases.py
with the margin condition it is stated under, and that `torch.equal` on the compared fields refuses the kernel mistakes the sweep is
there to catch (restated on the CPU)."""
import pytest
import torch

import selection_cases as SC
import selection_reference as R
from oracle import sast_oracle as O

CASE_IDS = [c["id"] for c in SC.ALL_CASES]


def _oracle_lists(case, tok, mode, dtype):
    B, H, W, ph, pw = SC.geometry(case)
    N, T = case["N"], case["T"]
    gid = R.group_token_ids(H, W, ph, pw, mode)
    sc = tok.to(dtype).view(B, H * W)[:, gid].reshape(B, N, T, 1)
    iw = O.select_windows(sc, B, N, T, case["bounce"])
    _it, asy, K = O.select_tokens(sc, iw, B, N, T, case["bounce"])
    return {"index_window": iw, "asy_index": asy, "K_list": K}


def check_structure(ref, case):
    """the size-independent properties test_selection_properties_full_size asks of the device: compaction is a bijection between kept
    tokens and compact rows in window-major / slot-ascending order, the counts agree, the packs tile the compact rows"""
    B, N, T, L = case["B"], case["N"], case["T"], case["L"]
    total, M = int(ref["counts"][0]), int(ref["counts"][1])
    assert total == ref["total"] and int(ref["win_keep"].sum()) == M and int(ref["K"].sum()) == total and int(ref["counts"][2]) == total // B
    K, ro, pr = ref["K"].long(), ref["row_off"].long(), ref["pack_rows"].long()
    assert torch.equal(K, ref["bits"].sum(1)) and bool((K[ref["win_keep"] == 0] == 0).all()) and bool((K[ref["win_keep"] == 1] > 0).all())
    assert torch.equal(ro, torch.cumsum(K, 0) - K)
    assert torch.equal(ref["win_rank"][ref["win_keep"] == 1].long(), torch.arange(M)) and bool((ref["win_rank"][ref["win_keep"] == 0] == -1).all())
    slot = ref["tok_slot"].long()
    kept = torch.nonzero(slot >= 0).view(-1)
    assert kept.numel() == total and torch.equal(torch.sort(slot[kept])[0], torch.arange(total))
    assert torch.equal(ref["row_tok"].long()[slot[kept]], kept)
    row_group = torch.repeat_interleave(torch.arange(B * N), K)
    assert torch.equal(ref["row_tok"].long() // L, row_group // N)                       # every row in its own sample
    gid = R.group_token_ids(case["H"], case["W"], case["ph"], case["pw"], ref["mode"])
    pos = torch.empty(L, dtype=torch.long)
    pos[gid.reshape(-1)] = torch.arange(N * T)
    flat = (ref["row_tok"].long() // L) * (N * T) + pos[ref["row_tok"].long() % L]        # b * N * T + n * T + t: strictly ascending
    assert bool((flat[1:] > flat[:-1]).all()) and torch.equal(flat // T, row_group)
    lim = SC.limit(case)
    assert int(pr.sum()) == total and (int(pr.max()) <= lim or int(K.max()) > lim)
    seg = ref["row_seg"].long()
    lo, hi = seg & 0xffff, seg >> 16
    assert torch.equal(hi - lo, K[row_group])
    leaders = torch.nonzero(pr).view(-1)
    pack_start = torch.repeat_interleave(ro[leaders], pr[leaders])
    assert pack_start.numel() == total
    assert torch.equal(torch.arange(total) - pack_start, lo + (torch.arange(total) - ro[row_group]))
    assert bool(((pr[leaders] <= lim) | (pr[leaders] == K[leaders])).all())       # a pack of several groups fits the budget
    last_row_group = row_group[ro[leaders] + pr[leaders] - 1]                      # ... and stays inside its aligned block of 16 groups
    assert torch.equal(last_row_group // 16, leaders // 16)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_restatement_reproduces_the_oracle_and_the_conditions_hold(cid):
    """both precisions of the restatement give the oracle's index_window / asy_index / K; the margin, float32 == float64 and the
    per-kind conditions hold; the reference's own output has the structure the device test asks of the kernels"""
    case = SC.BY_ID[cid]
    inp = SC.make_inputs(case)
    SC.check_conditions(case, inp)
    for mode in SC.MODES:
        for dtype in (torch.float32, torch.float64):
            ref, want = SC.reference(case, mode, dtype), _oracle_lists(case, inp["tok"], mode, dtype)
            for name in R.LISTS:
                assert torch.equal(ref[name], want[name]), (cid, mode, dtype, name)
        check_structure(dict(SC.reference(case, mode), mode=mode), case)


def test_case_table_covers_what_the_sweep_is_about():
    cs = SC.SWEEP_CASES
    assert {c["shape"] for c in cs} == set(SC.SHAPES) and len(SC.SHAPES) == 10
    assert {c["T"] for c in cs} == {4, 20, 60, 64, 65, 128, 129, 240, 256} and {c["N"] for c in cs} == {4, 8, 16, 17, 1056}
    assert any(c["B"] * c["N"] % 16 and c["B"] * c["N"] > 1 for c in cs) and any(c["B"] == 1 for c in cs)
    for shape in SC.SHAPES:
        mine = [c for c in cs if c["shape"] == shape]
        assert {(c["sharp"], c["bounce"]) for c in mine if c["kind"] == "rand"} == {(s, b) for s in (0.3, 0.8) for b in (0.0, 1e-3, 0.5)}
        assert {c["bounce"] for c in mine if c["kind"] == "const"} == {0.0, 1e-3}
        assert any(c["kind"] == "quiet" for c in mine) == (shape[0] > 1)
    assert {(c["T"], c["knob"], SC.limit(c)) for c in SC.KNOB_CASES} >= {(60, 64, 64), (80, 1000, 96), (60, 1, 1)}
    # what each knob case must tell its limit from (check_conditions asserts it on the reference's packs, in both modes)
    assert {(c["T"], c["knob"]): set(c["unlike"]) for c in SC.KNOB_CASES} == {(60, 64): {32, 96}, (80, 1000): {32, 64, 128}, (60, 1): {32, 0}, (4, 1): {32, 0}}
    assert all(not c["unlike"] for c in cs)
    assert all(SC.limit(c) == 32 for c in cs if c["T"] >= 20) and R.pack_limit(60) == 32 and R.pack_limit(4, 1000) == 64 and R.pack_limit(129, 1000) == 128


def test_the_cases_reach_the_edges_they_are_there_for():
    """single-token windows, dropped and full windows, bit 63, a token in the second / fourth word, packs of several groups and a pack
    led by a dropped group, packs that straddle samples -- all in the float64 reference of some case"""
    seen = set()
    for case in SC.ALL_CASES:
        for mode in SC.MODES:
            r = SC.reference(case, mode)
            K, T, N = r["K"], case["T"], case["N"]
            seen |= {"k1"} if bool((K == 1).any()) else set()
            seen |= {"dropped"} if bool((r["win_keep"] == 0).any()) else set()
            seen |= {"partial"} if bool(((K > 0) & (K < T)).any()) else set()
            if T == 64 and case["kind"] == "rand" and bool(r["bits"][:, 63].any()) and not bool(r["bits"][:, 63].all()):
                seen.add("bit63")
            if T == 65 and case["kind"] == "rand" and bool(r["bits"][:, 64].any()) and not bool(r["bits"][:, 64].all()):
                seen.add("word2")
            if T > 192 and case["kind"] == "rand" and bool(r["bits"][:, 192:].any()):
                seen.add("word4")
            lead = torch.nonzero(r["pack_rows"]).view(-1)
            if bool((r["pack_rows"] > K).any()):
                seen.add("shared-pack")
            if bool(((r["pack_rows"] > 0) & (K == 0)).any()):
                seen.add("dropped-leader")
            if N % 16 and case["B"] > 1 and N > 1:
                for w in lead.tolist():
                    rows, j = int(r["pack_rows"][w]), w
                    while rows > 0:
                        rows -= int(K[j])
                        j += 1
                    if (j - 1) // N != w // N and int(K[j - 1]) > 0:
                        seen.add("pack-across-samples")
    assert seen == {"k1", "dropped", "partial", "bit63", "word2", "word4", "shared-pack", "dropped-leader", "pack-across-samples"}, seen


# ------------------------------------------------------------------------------------------------ the comparison bites
def _mutant(case, mode, what):
    """the float32 restatement with one kernel mistake restated on the CPU"""
    B, H, W, ph, pw = SC.geometry(case)
    tok = SC.make_inputs(case)["tok"]
    ref = SC.reference(case, mode, torch.float32)
    out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ref.items()}
    if what == "strict-token-compare":                 # `>=` -> `>` in the token ballot
        nw, nt = R.probabilities(tok, B, H, W, ph, pw, mode, torch.float32)
        thr_t = R.thresholds(case["N"], case["T"], case["bounce"], torch.float32)[1]
        out["bits"] = (nt > thr_t) & ref["win_keep"].bool()[:, None]
        out["K"] = out["bits"].sum(1).int()
    elif what == "below-from-the-top":                 # rank of a kept token = popcount of the mask bits ABOVE (63 - lane) instead of below lane
        bits = ref["bits"]
        T = case["T"]
        words = torch.zeros(bits.shape[0], 256, dtype=torch.bool)
        words[:, :T] = bits
        slot = torch.full_like(ref["tok_slot"], -1)
        gid = R.group_token_ids(H, W, ph, pw, mode)
        for w in torch.nonzero(ref["K"]).view(-1).tolist():
            b, n, before = w // case["N"], w % case["N"], int(ref["row_off"][w])
            for q in range(0, 256, 64):
                word = words[w, q:q + 64]
                for lane in torch.nonzero(word).view(-1).tolist():       # below = ~0 >> (63 - lane): the bits 0 .. lane, the own one included
                    slot[b * case["L"] + int(gid[n, q + lane])] = before + int(word[:lane + 1].sum())
                before += int(word.sum())
        out["tok_slot"] = slot
    return out


def test_exact_comparison_refuses_a_strict_token_compare_on_the_constant_map():
    case = next(c for c in SC.SWEEP_CASES if c["kind"] == "const" and c["bounce"] == 0.0 and c["T"] == 60)
    for mode in SC.MODES:
        ref, bad = SC.reference(case, mode), _mutant(case, mode, "strict-token-compare")
        assert int(ref["K"].sum()) == case["B"] * case["L"] and int(bad["K"].sum()) == 0
        assert not torch.equal(bad["bits"], ref["bits"]) and not torch.equal(bad["K"], ref["K"])


@pytest.mark.parametrize("cid", [c["id"] for c in SC.SWEEP_CASES if c["shape"] in ((2, 8, 10, 4, 5), (2, 10, 26, 5, 13))])
def test_exact_comparison_refuses_a_rank_counted_with_the_own_bit(cid):
    case = SC.BY_ID[cid]
    for mode in SC.MODES:
        ref, bad = SC.reference(case, mode), _mutant(case, mode, "below-from-the-top")
        assert bool((ref["K"] > 1).any())
        assert not torch.equal(bad["tok_slot"], ref["tok_slot"])
