"""The selection kernels (csrc/k_select.hip: sast_select, sast_select_pair, sast_select_packs) against the float64 restatement of
tests/selection_reference.py, EXACTLY: every entry of every field of SastSel by torch.equal, on the cases of tests/selection_cases.py.

No decision is excluded and there is no tolerance.  That is a fair demand because of a condition on the inputs, asserted here for every
case before the kernels run (selection_cases.check_conditions): in the float64 evaluation every window and token decision is at least
1e-3 (relative) from its threshold in both partitions, a thousand times a float32 softmax error, and the float32 restatement reaches
the same result; exactly uniform rows (a constant map, an empty frame) are ties in every precision and are kept.

The buffers are handed over full of a sentinel: what the kernels must write is compared, and what they must leave alone (the compact rows
behind the kept ones) must still hold the sentinel.
"""
import ctypes as C

import pytest
import torch

import selection_cases as SC
from operator_sweep import SAST_EINVAL, dev, ids, restore_knobs, set_knobs  # noqa: F401  (dev, restore_knobs: fixtures)

pytestmark = pytest.mark.gpu

SENTINEL = -7
SCALARS = ("win_keep", "K", "row_off", "win_rank", "pack_rows", "counts", "tok_slot")


def fresh_selection(case, mode, dev):
    from sast_amd import functional as SF
    B, H, W, ph, pw = SC.geometry(case)
    sel = SF.Selection(B, H, W, ph, pw, mode, dev)
    sel._buf.fill_(SENTINEL)
    sel.mask.fill_(-1)
    return sel


def run_select(case, mode, tok, dev):
    """sast_select the way functional.select calls it, into sentinel-filled buffers"""
    from sast_amd import _lib as L, functional as SF
    sel = fresh_selection(case, mode, dev)
    s = sel.struct()
    L.check(L.lib().sast_select(tok.data_ptr(), *SC.geometry(case), mode, float(case["bounce"]), C.byref(s), SF._stream()), "select")
    sel.tok = tok
    torch.cuda.synchronize()
    return sel


def run_pair(case, tok, dev):
    from sast_amd import _lib as L, functional as SF
    a, b = fresh_selection(case, 0, dev), fresh_selection(case, 1, dev)
    sa, sb = a.struct(), b.struct()
    L.check(L.lib().sast_select_pair(tok.data_ptr(), *SC.geometry(case), float(case["bounce"]), C.byref(sa), C.byref(sb), SF._stream()), "select_pair")
    a.tok = b.tok = tok
    torch.cuda.synchronize()
    return a, b


def mask_bits(sel):
    """[B * N, 64 * words] bool from the mask words (bit 63 sits in the sign of the int64 view)"""
    m = sel.mask.cpu()
    ar = torch.arange(64, dtype=torch.int64)
    return (((m[:, :, None] >> ar) & 1) != 0).reshape(m.shape[0], -1)


def assert_matches(sel, ref, case, what=""):
    """every field against the reference; nothing written past the kept rows; no mask bit at or above T"""
    T, total, misses = case["T"], ref["total"], []
    for f in SCALARS:
        got = getattr(sel, f).cpu()
        if not torch.equal(got, ref[f]):
            misses.append(f"{f}: {int((got != ref[f]).sum())} of {got.numel()} entries differ")
    bits = mask_bits(sel)
    assert bits.shape[1] == (128 if T <= 128 else 256)
    if bool(bits[:, T:].any()):
        misses.append(f"mask: {int(bits[:, T:].sum())} bits at or above T = {T}")
    if not torch.equal(bits[:, :T], ref["bits"]):
        misses.append(f"mask: {int((bits[:, :T] != ref['bits']).sum())} bits differ")
    for f in ("row_tok", "row_seg"):
        got = getattr(sel, f).cpu()
        if not torch.equal(got[:total], ref[f]):
            misses.append(f"{f}[:total]: {int((got[:total] != ref[f]).sum())} of {total} entries differ")
        if not bool((got[total:] == SENTINEL).all()):
            misses.append(f"{f}[total:]: {int((got[total:] != SENTINEL).sum())} entries written past the kept rows")
    for name, got in (("index_window", sel.index_window()), ("asy_index", sel.asy_index()), ("K_list", sel.K_list())):
        if not torch.equal(got.cpu(), ref[name]):
            misses.append(f"{name}() differs from the reference list")
    assert not misses, f"{case['id']} {what}:\n  " + "\n  ".join(misses)


def assert_same(a, b, what):
    for f in SCALARS + ("row_tok", "row_seg", "mask"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f"{what}: {f}"


def inputs(case, dev):
    inp = SC.make_inputs(case)
    SC.check_conditions(case, inp)
    return inp["tok"].to(dev)


# ------------------------------------------------------------------------------------------------ sast_select
@pytest.mark.parametrize("mode", SC.MODES, ids=["window", "grid"])
@pytest.mark.parametrize("case", SC.SWEEP_CASES, ids=ids(SC.SWEEP_CASES))
def test_select(case, mode, dev):
    """both mask-word instantiations, T on either side of 64 / 128 / 256, N below 16, no multiple of 16 and above 1024, B * N ending
    inside a block of 16 groups, sparse / mixed / nearly full / constant / empty-frame maps, bounce 0 / 1e-3 / 0.5"""
    tok = inputs(case, dev)
    assert_matches(run_select(case, mode, tok, dev), SC.reference(case, mode), case, f"mode {mode}")


@pytest.mark.parametrize("mode", SC.MODES, ids=["window", "grid"])
@pytest.mark.parametrize("case", SC.KNOB_CASES, ids=ids(SC.KNOB_CASES))
def test_select_under_the_pack_budget_knob(case, mode, dev, monkeypatch):
    """SAST_ATTN_PACKS = 64 at T = 60, 1000 at T = 80 (the cap of 96 binds), 1: the packs of the reference with that limit"""
    set_knobs(monkeypatch, case["env"])
    tok = inputs(case, dev)         # (check_conditions: the packs of this limit differ from those of the default and of the neighbouring caps)
    assert case["unlike"] and 32 in case["unlike"]
    assert_matches(run_select(case, mode, tok, dev), SC.reference(case, mode), case, f"mode {mode}")


# ------------------------------------------------------------------------------------------------ sast_select_pair
# the shipped bounce on every kind of map, and the exact ties at bounce 0 (constant maps, empty frames) through the second partition too
PAIR_CASES = [c for c in SC.SWEEP_CASES if (c["bounce"] == SC.SHIPPED_BOUNCE and c["sharp"] in (None, 0.8))
              or (c["bounce"] == 0.0 and c["kind"] in ("const", "quiet"))]


@pytest.mark.parametrize("case", PAIR_CASES, ids=ids(PAIR_CASES))
def test_select_pair_equals_two_selects(case, dev):
    tok = inputs(case, dev)
    pair = run_pair(case, tok, dev)
    for mode in SC.MODES:
        assert_same(pair[mode], run_select(case, mode, tok, dev), f"{case['id']} mode {mode}")
        assert_matches(pair[mode], SC.reference(case, mode), case, f"pair, mode {mode}")


def test_select_pair_in_a_graph_replays_on_new_scores(dev):
    """one select_pair captured on a static `tok`; replayed after another case's scores were copied in, it gives that case's reference"""
    from sast_amd import _lib as L, functional as SF
    first, second = (SC.BY_ID[f"sel-2x24x40-p6x10-rand{s}-b0.001"] for s in ("0.8", "0.3"))
    tok = inputs(first, dev).clone()
    other = inputs(second, dev)
    assert not torch.equal(SC.reference(first, 0)["tok_slot"], SC.reference(second, 0)["tok_slot"])
    a, b = fresh_selection(first, 0, dev), fresh_selection(first, 1, dev)
    sa, sb = a.struct(), b.struct()

    def call():
        L.check(L.lib().sast_select_pair(tok.data_ptr(), *SC.geometry(first), float(first["bounce"]), C.byref(sa), C.byref(sb), SF._stream()), "select_pair")

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for case, scores in ((second, other), (first, inputs(first, dev))):
        tok.copy_(scores)
        for sel in (a, b):
            sel._buf.fill_(SENTINEL)
            sel.mask.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for mode, sel in ((0, a), (1, b)):
            assert_matches(sel, SC.reference(case, mode), case, f"graph replay, mode {mode}")


# ------------------------------------------------------------------------------------------------ sast_select_packs
PACKS_CASES = SC.KNOB_CASES + [c for c in SC.SWEEP_CASES if c["bounce"] == SC.SHIPPED_BOUNCE and c["sharp"] in (None, 0.8)]


@pytest.mark.parametrize("case", PACKS_CASES, ids=ids(PACKS_CASES))
def test_select_packs_on_index_lists(case, dev, monkeypatch):
    """selection_from_index_lists on the reference's lists (partitioned layout): sast_select_packs gives the packs sast_select writes"""
    from sast_amd import functional as SF
    if case["env"]:
        set_knobs(monkeypatch, case["env"])
    SC.check_conditions(case, SC.make_inputs(case))
    for mode in SC.MODES:
        ref = SC.reference(case, mode)
        W, T, total = case["B"] * case["N"], case["T"], ref["total"]
        sel = SF.selection_from_index_lists(ref["index_window"], ref["asy_index"], ref["K_list"], W, T, dev)
        torch.cuda.synchronize()
        assert torch.equal(sel.K.cpu(), ref["K"]) and torch.equal(sel.row_off.cpu(), ref["row_off"]) and int(sel.counts[0]) == total
        assert torch.equal(sel.pack_rows.cpu(), ref["pack_rows"]), (case["id"], mode)
        assert torch.equal(sel.row_seg[:total].cpu(), ref["row_seg"]), (case["id"], mode)
        assert torch.equal(mask_bits(sel)[:, :T], ref["bits"]) and not bool(mask_bits(sel)[:, T:].any())


# ------------------------------------------------------------------------------------------------ refusals
def test_select_refuses_bad_arguments(dev):
    from sast_amd import _lib as L, functional as SF
    lib = L.lib()
    B, H, W, ph, pw = 1, 16, 34, 16, 17                 # T = 272: past the four mask words
    tok = torch.ones(B, H * W, device=dev)
    # (functional.Selection itself refuses T > 256: buffers by hand, sized for the call)
    buf = torch.full((5 * 2 + 4 + 3 * B * H * W,), SENTINEL, device=dev, dtype=torch.int32)
    mask = torch.full((2, 5), -1, device=dev, dtype=torch.int64)
    s = L.SastSel()
    nw, n = 2, B * H * W
    SF._fill(s, win_keep=buf[0:nw], K=buf[nw:2 * nw], row_off=buf[2 * nw:3 * nw], win_rank=buf[3 * nw:4 * nw], pack_rows=buf[4 * nw:5 * nw],
             counts=buf[5 * nw:5 * nw + 4], tok_slot=buf[5 * nw + 4:5 * nw + 4 + n], row_tok=buf[5 * nw + 4 + n:5 * nw + 4 + 2 * n],
             row_seg=buf[5 * nw + 4 + 2 * n:], mask=mask)
    assert lib.sast_select(tok.data_ptr(), B, H, W, ph, pw, 0, 1e-3, C.byref(s), SF._stream()) == SAST_EINVAL
    assert lib.sast_select_pair(tok.data_ptr(), B, H, W, ph, pw, 1e-3, C.byref(s), C.byref(s), SF._stream()) == SAST_EINVAL
    assert lib.sast_select(None, B, H, W, ph, pw, 0, 1e-3, C.byref(s), SF._stream()) == SAST_EINVAL
    assert lib.sast_select(tok.data_ptr(), B, H, W, ph, pw, 0, 1e-3, None, SF._stream()) == SAST_EINVAL
    assert lib.sast_select_pair(tok.data_ptr(), B, H, W, ph, pw, 1e-3, C.byref(s), None, SF._stream()) == SAST_EINVAL
    assert lib.sast_select_pair(tok.data_ptr(), B, H, W, ph, pw, 1e-3, None, C.byref(s), SF._stream()) == SAST_EINVAL
    assert lib.sast_select_packs(None, 2, 60, SF._stream()) == SAST_EINVAL
    assert lib.sast_select_packs(C.byref(L.SastSel()), 2, 60, SF._stream()) == SAST_EINVAL          # null K / row_off / pack_rows / row_seg
    assert lib.sast_select_packs(C.byref(s), 2, 272, SF._stream()) == SAST_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all()) and bool((mask == -1).all())                                # refused before anything was written
    with pytest.raises(AssertionError, match="must be divisible by partition"):
        SF.select(tok, 1, 16, 34, 5, 17, 0, 1e-3)
    with pytest.raises(AssertionError, match="must be divisible by partition"):
        SF.select_pair(tok, 1, 16, 34, 16, 5, 1e-3)
