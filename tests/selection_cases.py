"""The case table of the selection sweep (tests/test_selection_operators.py), the inputs of every case and the conditions they are stated
under.  Shared by the GPU test and by tests/test_selection_reference.py.  CPU only: nothing here imports the library.

The selection is a set of threshold compares: a wrong bit produces no NaN, the model trains on other tokens.  So the kernels are compared
EXACTLY (torch.equal on every field of SastSel) with the float64 restatement of tests/selection_reference.py, and no decision is excluded.
What makes that a fair demand is a condition on the inputs, asserted by `check_conditions`, not a measurement of the kernels:

  MARGIN  in the float64 evaluation every window decision and every token decision (of dropped windows too) lies at a relative distance
          of at least 1e-3 from its threshold, in BOTH partitions of the same scores (window and grid: `sast_select_pair` serves both from
          one `tok`).  A float32 softmax is off by about 1e-6, the full-size test's disagreement band is 1e-5.  Exactly uniform rows (the
          `const` map, the empty frame of `quiet`) are ties by construction: every value is fl(1 / n) in every precision, kept at any
          bounce >= 0 (selection_reference.margins).
          The inputs are made to satisfy it: exp(sharp * randn) quantised to multiples of 1 / 1024; while a decision is inside the margin
          the offending token (for a window decision: the window's first token) is multiplied by 1.03125 and everything is recomputed.
  the float32 restatement then reaches the same fields and lists as the float64 one.

Shapes (B, H, W, ph, pw), the smallest that reach each branch of csrc/k_select.hip:
  (2,   8, 10,  4,  5)  T  20  N    4  less than one wave of tokens, N < 16
  (1, 102, 10,  6, 10)  T  60  N   17  a second 16-window chunk holding one window, B = 1
  (2,  24, 40,  6, 10)  T  60  N   16  the shipped partition: one full chunk per sample, B * N = 32, packs across full blocks
  (3,  16, 16,  8,  8)  T  64  N    4  one full mask word, bit 63 set, B * N = 12 ends inside a block of 16 groups
  (2,  10, 26,  5, 13)  T  65  N    4  one token in the second word
  (2,  32, 32,  8, 16)  T 128  N    8  two full words, the last T of the 2-word kernels
  (1,   6, 86,  3, 43)  T 129  N    4  the first T of the 4-word kernels
  (2,  24, 40, 12, 20)  T 240  N    8  the gen4 split-1 partition
  (1,  32, 32, 16, 16)  T 256  N    4  the limit
  (2,  66, 64,  2,  2)  T   4  N 1056  N > 1024: the thread-strided max / sum loops take a second trip, 66 chunks, B * N = 2112
Every shape: sharp in {0.3, 0.8} x bounce in {0, 1e-3 (the shipped BOUNCE), 0.5} (sparse maps with windows of a single token, mixed maps,
nearly full ones); `const` (tok = 1 at bounce 0 and 1e-3: everything kept, every mask bit below T set); where B > 1, `quiet` (the last
sample all zero: an empty frame next to a busy one).  Each case is run in both modes.
Knob cases (SAST_ATTN_PACKS, the row budget of an attention pack): 64 at T = 60; 1000 at T = 80, where the cap of 96 binds, on
(2, 16, 40, 8, 10) at bounce 0.5 (K of 1 .. 33 per group: aligned sub-blocks sum to 65 .. 96 and to 97 .. 128, so the packs at 96 differ
from those at 64 and at 128); 1.  Each knob case asserts that its packs differ from those of the neighbouring limits (`unlike`).

Settling the margin in both partitions at once takes at most 17 rounds on these cases (0 .. 4 for most); the loop gives up after MAX_ROUNDS.
"""
import functools

import torch

import operator_sweep as SW
import selection_reference as R

MARGIN = 1e-3
NUDGE = 1.03125
MAX_ROUNDS = 24
MODES = (0, 1)
SHIPPED_BOUNCE = 1e-3

SHAPES = ((2, 8, 10, 4, 5), (1, 102, 10, 6, 10), (2, 24, 40, 6, 10), (3, 16, 16, 8, 8), (2, 10, 26, 5, 13), (2, 32, 32, 8, 16),
          (1, 6, 86, 3, 43), (2, 24, 40, 12, 20), (1, 32, 32, 16, 16), (2, 66, 64, 2, 2))
KNOB_SHAPE_T80 = (2, 16, 40, 8, 10)


def _case(shape, kind, bounce, sharp=None, knob=None, unlike=()):
    B, H, W, ph, pw = shape
    name = kind + (f"{sharp:g}" if sharp is not None else "")
    base = f"sel-{B}x{H}x{W}-p{ph}x{pw}-{name}-b{bounce:g}"          # a knob case runs on the inputs of the case without the knob
    return dict(id=base + (f"-packs{knob}" if knob is not None else ""), inputs_id=base, shape=shape, B=B, H=H, W=W, ph=ph, pw=pw, T=ph * pw, N=(H // ph) * (W // pw), L=H * W, kind=kind, sharp=sharp,
                bounce=bounce, knob=knob, unlike=tuple(unlike), env={} if knob is None else {"SAST_ATTN_PACKS": knob})


SWEEP_CASES = [c for shape in SHAPES for c in (
    [_case(shape, "rand", bounce, sharp) for sharp in (0.3, 0.8) for bounce in (0.0, SHIPPED_BOUNCE, 0.5)]
    + [_case(shape, "const", bounce) for bounce in (0.0, SHIPPED_BOUNCE)]
    + ([_case(shape, "quiet", bounce, 0.8) for bounce in (0.0, SHIPPED_BOUNCE)] if shape[0] > 1 else []))]
# `unlike`: the limits whose packs the reference must differ from in both modes (check_conditions): the default of 32 and, around a cap,
# the neighbouring caps -- sub-block sums of the case fall on both sides of each
KNOB_CASES = [_case((2, 24, 40, 6, 10), "rand", SHIPPED_BOUNCE, 0.3, knob=64, unlike=(32, 96)),
              _case(KNOB_SHAPE_T80, "rand", 0.5, 0.8, knob=1000, unlike=(32, 64, 128)),
              _case((2, 24, 40, 6, 10), "quiet", SHIPPED_BOUNCE, 0.8, knob=1, unlike=(32, 0)), _case((2, 66, 64, 2, 2), "rand", 0.0, 0.8, knob=1, unlike=(32, 0))]
ALL_CASES = SWEEP_CASES + KNOB_CASES
BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES), "duplicate case ids"


def geometry(case):
    return case["B"], case["H"], case["W"], case["ph"], case["pw"]


def limit(case):
    return R.pack_limit(case["T"]) if case["knob"] is None else R.pack_limit(case["T"], case["knob"])


# ------------------------------------------------------------------------------------------------ inputs
def _inside(case, tok):
    """flat bool mask over the B * L tokens: the tokens to nudge for the decisions inside the margin (None: there is none)"""
    B, H, W, ph, pw = geometry(case)
    hit = torch.zeros(B * case["L"], dtype=torch.bool)
    for mode in MODES:
        mw, mt = R.margins(tok, B, H, W, ph, pw, mode, case["bounce"])
        gid = R.group_token_ids(H, W, ph, pw, mode)
        image_tok = (torch.arange(B).view(B, 1, 1) * case["L"] + gid.view(1, *gid.shape)).reshape(B * case["N"], case["T"])
        hit[image_tok[(mw < MARGIN).reshape(-1), 0]] = True
        hit[image_tok[mt < MARGIN]] = True
    return hit if bool(hit.any()) else None


@functools.lru_cache(maxsize=None)
def _settled(cid):
    case = next(c for c in ALL_CASES if c["inputs_id"] == cid)
    B, L = case["B"], case["L"]
    if case["kind"] == "const":
        return torch.ones(B, L), 0
    g = SW.gen(cid)
    tok = torch.round(torch.exp(case["sharp"] * torch.randn(B, L, generator=g)) * 1024) / 1024
    if case["kind"] == "quiet":
        tok[-1] = 0.0
    for rounds in range(MAX_ROUNDS + 1):
        hit = _inside(case, tok)
        if hit is None:
            return tok, rounds
        tok.view(-1)[hit] *= NUDGE
    raise AssertionError(f"{cid}: decisions inside the margin after {MAX_ROUNDS} rounds")


def make_inputs(case):
    """{"tok": [B, L] float32}; computed once per case, handed out as a copy"""
    return {"tok": _settled(case["inputs_id"])[0].clone()}


def settle_rounds(case):
    return _settled(case["inputs_id"])[1]


@functools.lru_cache(maxsize=None)
def _reference(cid, mode, dtype):
    case = BY_ID[cid]
    return R.select(_settled(case["inputs_id"])[0], *geometry(case), mode, case["bounce"], limit(case), dtype)


def reference(case, mode, dtype=torch.float64):
    """the restatement on the case's inputs: computed once, shared by the tests, not to be modified"""
    return _reference(case["id"], mode, dtype)


# ------------------------------------------------------------------------------------------------ conditions the cases are stated under
def check_conditions(case, inp):
    B, H, W, ph, pw = geometry(case)
    N, T, L = case["N"], case["T"], case["L"]
    tok = inp["tok"]
    assert tok.dtype == torch.float32 and tuple(tok.shape) == (B, L) and torch.equal(tok, _settled(case["inputs_id"])[0])
    assert float(tok.min()) >= 0.0
    for mode in MODES:
        mw, mt = R.margins(tok, B, H, W, ph, pw, mode, case["bounce"])
        assert float(mw.min()) >= MARGIN and float(mt.min()) >= MARGIN, (case["id"], mode, float(mw.min()), float(mt.min()))
        r64, r32 = reference(case, mode), reference(case, mode, torch.float32)
        for f in R.FIELDS + R.LISTS:
            assert torch.equal(r64[f], r32[f]), f"{case['id']} mode {mode}: {f} differs between float32 and float64"
        assert r64["total"] == r32["total"] == int(r64["K"].sum())
        keep = r64["win_keep"].view(B, N)
        if case["kind"] == "const":
            assert int(r64["K"].sum()) == B * L and bool(r64["bits"].all()) and bool(keep.all())
        elif case["kind"] == "quiet":
            assert float(tok[-1].abs().max()) == 0.0 and float(tok[0].min()) > 0.0
            assert bool(keep[-1].all()) and bool(r64["bits"].view(B, N, T)[-1].all()), "the empty frame keeps everything"
        if case["kind"] != "const" and case["bounce"] <= SHIPPED_BOUNCE:       # the sparse and the mixed maps
            assert 0 < int(keep.sum()) < B * N, (case["id"], mode, "no dropped or no kept window")
            assert bool((keep[0] == 0).any()) and bool((keep[0] == 1).any())
        for other in case["unlike"]:        # a knob case tells its limit from the neighbouring ones: another knob default or cap would show
            assert limit(case) != other
            assert R.packs(r64["K"].tolist(), other)[0] != r64["pack_rows"].tolist(), (case["id"], mode, f"packs as with limit {other}")
