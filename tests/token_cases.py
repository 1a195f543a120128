"""The case table of the token-path operator sweep (tests/test_token_operators.py), the inputs of every case and its CPU reference.

Shared by the GPU test, by the bounds generator (tests/operator_sweep.py: every case in float32 against float64 on the CPU) and by
tests/test_token_reference.py, so that all three see the same cases, numbers and quantity names.  CPU only: nothing here imports the library.

A case is a dict with an "id", an "op" (the operator family its error statistics are pooled over), shapes and options.
`make_inputs(case)` -> fp32 CPU tensors from a generator seeded by the id.  `reference(case, inputs, dtype)` -> {quantity: tensor}.
Quantity names: "out:<name>" (forward results, every one O(1): compared absolutely), "rel:tok" (the token scores: they feed a threshold
compare and scale with amp, so they are compared like a gradient) and "grad:<name>" (relative to the reference tensor's max-norm).
`measure` and `project_bar` are those of tests/operator_sweep.py, `pool_key` is that of tests/conv_cases.py.

Families:
  score       STP scoring.  "exact" inputs put every pre-activation of the scoring linear on an odd multiple of 1/256, computed without
              rounding in fp32 in any summation order (|z| < 2^12 at a resolution of 2^-8, operands of at most 6 significant bits), so
              the gate s > 0 of the backward cannot differ between a correct kernel and the reference: xp multiples of 1/8 in [-2, 2],
              ws_w multiples of 1/16 in [-1, 1], ws_b odd multiples of 1/256.  The upstream gradient is Gaussian, so dz, both backward
              GEMMs and the d(scale) sums still round.  "gauss" inputs compare only what does not pass the gate's derivative (xw, tok,
              d_wc).  "inf": three channels whose 20 control weights are -inf, so exp is exactly 0, scale = 0 and amp / scale = inf -> 0.
              r is a [:, :20] slice of a [B, 32] buffer; the last sample of a B = 3 case is an empty frame (r = 0); wc is drawn around
              the value the model initialises it with (1), with spread so that a slipped index shows.
  mswsa       the MS-WSA layer on explicit selections in partitioned layout: B = 2 on an 8 x 10 map with partition 4 x 5 (T = 20, four
              windows per sample, 160 rows), inner = mlp_inner_dim(C), dim_head 32 (24 at C = 48; 8 and 16 as well at C = 64, 16 at C = 96).
              "mix": K per window = 20, 1, dropped, 19 | 7, 12, 20, 3.  "empty2": the second sample keeps
              nothing.  "cond": input rows 30 + 0.1 randn (mean far above the spread).
  mswsa_part  the same layer at the partition sizes the attention launchers dispatch on (csrc/k_attn_mfma.hip: T <= 64, <= 96, <= 128,
              <= 256), with an operator of its own so that the medians of `mswsa` stay what they were: B = 1, one dropped window,
              T = 60 with K = 60, 33, 32, 1, 17; T = 80 with 80, 65, 64, 3; T = 120 with 120, 97, 96, 31; T = 240 with 240, 129, 128, 33.
              What the stand-alone attention suite (tests/attn_cases.py) does not run: the LayerScale-finish side workgroups of the
              attention backward (2 C rows in blocks of 4 | 2 (T = 60, split | sequential), 6 | 3 (T = 80: ragged at C = 32 and 64),
              4 (T = 120) and 8 (T = 240) rows) and the one-kernel forward with three and four waves (C = 64 at T = 80 and 120).
              T = 60 and 80 again with SAST_ATTN_BWD_SPLIT=0; "peaked": the q and k rows of qkv_w times 2 (logit std about 4) at T = 240.
  mswsa_act   the twelve gate activations the `mswsa` family does not run (every code of csrc/common.cuh: glu_act but gelu and prelu)
              through the layer, forward and backward, on the "mix" selection at C = 48 (dim_head 24) and C = 192, with an operator of its
              own.  `gate_gain` multiplies the gate half of fc1_w and fc1_b so that the gate pre-activations of the kept rows have a
              standard deviation of about 3: `check_conditions` asserts on the float64 reference that at least 1 % of them lie on each
              side of every kink of the case's activation (ACT_KINKS: 0, the clamp of relu6 at 6, the +-3 ends of hard_sigmoid and
              hard_swish, the -2 end of hard_mish) and that none lies within KINK_BAND x max|gate| of one, so that a derivative jump
              cannot land on different sides in fp32 and fp64.  The seed tag of an id ("-s<n>") is the first for which the band is empty.
  mask_token / add_pos   B = 3 on an 11 x 25 map (825 rows: three blocks of 256 and a partial one), the table has one row per position.
  lstm        ConvLSTM at B = 2, 5 x 7 (M = 70: a partial 64-row tile).  States: "given", "none" (h0 = c0 = None: the reduction drops
              the h half and the forget gate is skipped), "zero" (all-zero tensors, present: the full path, dh0 / dc0 requested),
              "h0zero" (zero h0 present, c0 None: forget-gate skip with the full reduction; dc0 is never requested without a c0).
              "sat" (state given, C = 48 and 256): w times 8 and c0 times 4, so that the gate pre-activations have a standard deviation
              of about 6 (a tenth of them beyond |z| = 10, where sigmoid_hw and tanh_hw are saturated to the last bit) and tanh_hw(c1)
              runs on |c| up to about 15.
  "glutile" (mswsa, C = 256 and 512) and "lstmtile" (lstm, C = 256, states "given" and "none") run the plain case under SAST_GLU_TILE=1 /
  SAST_LSTM_TILE=1: the k-split group tiles TileG2K4, TileG4K4 and TileG3K4 through the operator's own wiring; same arithmetic, so
  they share the plain case's bounds entry (tests/test_gemm_exact.py runs those tiles on exact operands).
"""
import math

import torch

import operator_sweep as SW
import token_reference as R
from parity_helpers import KINK_BAND
from conv_cases import pool_key  # noqa: F401  (part of the suite's face: the token quantities have no unit prefixes to pool)
from oracle import sast_oracle as O

WIDTHS = (32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024)       # csrc/k_rows.hip: SAST_DISPATCH_C
AMPS = (1.0, 2e-2, 2e-4)
INF_CHANNELS = (3, 17, 40)


# ------------------------------------------------------------------------------------------------ the table
def _score(C, B, L, amp, kind="exact"):
    return dict(id=f"score-{kind}-{B}x{L}x{C}-amp{amp:g}", op="score", kind=kind, B=B, L=L, C=C, amp=amp, env={})


SCORE_CASES = (
    # all eleven widths; L = 33: one row over rpb = 32 (stp_bwd_launch), a partial last block
    [_score(C, 3, 33, AMPS[i % 3]) for i, C in enumerate(WIDTHS)]
    + [_score(64, 3, 33, 1.0), _score(64, 3, 33, 2e-2)]                          # (64 has 2e-4 above): every amp at one width
    # the three rpb branches of stp_bwd_launch (32 / 64 / 128 rows per block), each with a remainder
    + [_score(32, 3, 7, 2e-2), _score(32, 3, 1030, 2e-4), _score(32, 3, 8200, 1.0)]
    + [_score(96, 1, 33, 2e-2), _score(768, 1, 33, 2e-4)]
    + [_score(C, 3, 33, amp, "gauss") for C, amp in ((64, 2e-2), (192, 2e-4), (1024, 1.0))]
    + [_score(64, 3, 33, 2e-2, "inf")])


def dim_head_of(C):
    return 32 if C % 32 == 0 else {48: 24}[C]


GLU_TILE = {"SAST_GLU_TILE": "1"}
LSTM_TILE = {"SAST_LSTM_TILE": "1"}


def _mswsa(C, dh=None, sel="mix", tag="", **opt):
    dh = dh or dim_head_of(C)
    c = dict(id=f"mswsa-c{C}-dh{dh}-{sel}" + (f"-{tag}" if tag else ""), op="mswsa", C=C, dh=dh, sel=sel, inner=O.mlp_inner_dim(C), B=2, N=4,
             T=20, fused=False, nograd=False, ls=True, cb=False, drop=False, act="gelu", cond=False, gate_gain=1.0, env={}, shares=None)
    c.update(opt)
    return c


MSWSA_CASES = (
    [_mswsa(C) for C in WIDTHS]
    + [_mswsa(C, sel="empty2") for C in (32, 48, 64, 192, 1024)]
    + [_mswsa(64, 8), _mswsa(64, 16), _mswsa(96, 16)]
    # the one-kernel forward (C = 64, inner 160, dim_head 32 only) against the same reference, with and without a backward behind it
    + [_mswsa(64, tag="fused", fused=True, shares="mswsa-c64-dh32-mix"),
       _mswsa(64, tag="fused-nograd", fused=True, nograd=True, shares="mswsa-c64-dh32-mix")]
    # one workgroup for the row backward: the grid-stride loop of ln1_gather_bwd takes several passes (ragged at C = 32 and 192)
    + [_mswsa(C, tag="lnblocks1", env={"SAST_LN_BLOCKS": "1"}, shares=f"mswsa-c{C}-dh32-mix") for C in (32, 192, 1024)]
    + [_mswsa(C, tag=tag, **opt) for C in (48, 192)
       for tag, opt in (("nols", dict(ls=False)), ("cb", dict(cb=True)), ("drop", dict(drop=True)), ("prelu", dict(act="prelu")))]
    + [_mswsa(64, tag="cond", cond=True)]
    # the k-split GLU tile of fc1 (csrc/k_block.hip: SAST_GLU_TILE, C >= 256: TileG2K4 at this grid)
    + [_mswsa(C, tag="glutile", env=dict(GLU_TILE), shares=f"mswsa-c{C}-dh32-mix") for C in (256, 512)])

# the gate activations beside gelu and prelu, and where the derivative of each jumps or its formula changes branch
ACT_KINKS = {"relu": (0.0,), "silu": (), "sigmoid": (), "tanh": (), "mish": (), "relu6": (0.0, 6.0), "leaky_relu": (0.0,), "elu": (0.0,), "selu": (0.0,),
             "hard_sigmoid": (-3.0, 3.0), "hard_swish": (-3.0, 3.0), "hard_mish": (-2.0, 0.0)}
GATE_GAIN = 3.0
ACT_SEEDS = {(192, "relu6"): 10, (48, "leaky_relu"): 4, (192, "leaky_relu"): 1, (192, "elu"): 7, (48, "selu"): 1, (192, "selu"): 2,
             (192, "hard_sigmoid"): 1, (48, "hard_swish"): 1, (192, "hard_swish"): 3, (48, "hard_mish"): 1}      # (default 0)


def _mswsa_act(C, act):
    return _mswsa(C, tag=f"{act}-s{ACT_SEEDS.get((C, act), 0)}", op="mswsa_act", act=act, gate_gain=GATE_GAIN)


MSWSA_ACT_CASES = [_mswsa_act(C, act) for act in ACT_KINKS for C in (48, 192)]

PART_KS = {60: [60, 33, 32, 1, 17], 80: [80, 65, 64, 3], 120: [120, 97, 96, 31], 240: [240, 129, 128, 33]}
PART_DROPPED = 2        # the window of a partition case that keeps nothing
NOSPLIT = {"SAST_ATTN_BWD_SPLIT": "0"}


def _part(T, C, tag="", **opt):
    return _mswsa(C, sel=f"part{T}", tag=tag, **dict(dict(op="mswsa_part", B=1, N=len(PART_KS[T]) + 1, T=T, peaked=False), **opt))


def _part_family():
    out = []
    for T, widths in ((60, (32, 64)), (80, (32, 64)), (120, (48, 64)), (240, (48, 64))):
        for C in widths:
            plain = _part(T, C)
            out.append(plain)
            if T <= 96:
                out.append(_part(T, C, "nosplit", env=dict(NOSPLIT), shares=plain["id"]))
            if C == 64 and T in (80, 120):      # the one-kernel forward: ntw = 3 and 4
                out += [_part(T, C, "fused", fused=True, shares=plain["id"]), _part(T, C, "fused-nograd", fused=True, nograd=True, shares=plain["id"])]
    return out + [_part(240, 64, "peaked", peaked=True)]


PART_CASES = _part_family()

MAP_HW = (11, 25)       # 275 positions, 825 rows at B = 3


def _mask(C, pattern, pe=True):
    return dict(id=f"masktoken-c{C}-{pattern}" + ("" if pe else "-nope"), op="mask_token", C=C, B=3, pattern=pattern, pe=pe, env={})


MASK_CASES = ([_mask(C, pat) for C in (32, 48, 1024) for pat in ("none", "all", "every257")]
              + [_mask(48, "every257", pe=False), _mask(1024, "all", pe=False)])
ADDPOS_CASES = [dict(id=f"addpos-c{C}", op="add_pos", C=C, B=3, env={}) for C in (32, 48, 1024)]

LSTM_HW = (5, 7)


def _lstm(C, state, two=False, drop=False, sat=False):
    return dict(id=f"lstm-c{C}-{state}" + ("-two" if two else "") + ("-drop" if drop else "") + ("-sat" if sat else ""), op="lstm", C=C, B=2,
                state=state, two=two, drop=drop, sat=sat, env={})


LSTM_CASES = ([_lstm(C, st) for C in WIDTHS for st in ("given", "none", "zero", "h0zero")]
              + [_lstm(C, st, two, drop) for C in (48, 256) for st, two, drop in (("given", True, True), ("none", False, True), ("h0zero", True, False))]
              + [_lstm(C, "given", sat=True) for C in (48, 256)]
              # the k-split gate tiles (csrc/k_block.hip: SAST_LSTM_TILE, reduction >= 256): TileG4K4 with a state, TileG3K4 without
              + [dict(_lstm(256, st), id=f"lstm-c256-{st}-lstmtile", env=dict(LSTM_TILE), shares=f"lstm-c256-{st}") for st in ("given", "none")])

ALL_CASES = SCORE_CASES + MSWSA_CASES + MSWSA_ACT_CASES + PART_CASES + MASK_CASES + ADDPOS_CASES + LSTM_CASES
BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES), "duplicate case ids"


def bounds_id(case):
    """cases that differ only in the library form or knob they run under are the same arithmetic: they share the plain case's figures"""
    return case.get("shares") or case["id"]


# ------------------------------------------------------------------------------------------------ inputs
def kept_slots(case):
    """{window id: sorted kept slots} of the case's selection: "mix" / "empty2" on eight windows of T = 20 slots (windows 0-3 are sample
    0), "part<T>" the K list of PART_KS[T] on consecutive windows of T slots with window PART_DROPPED left out"""
    if case["sel"].startswith("part"):
        Ks = dict(zip([w for w in range(case["N"]) if w != PART_DROPPED], PART_KS[case["T"]]))
    else:
        Ks = {"mix": {0: 20, 1: 1, 3: 19, 4: 7, 5: 12, 6: 20, 7: 3}, "empty2": {0: 20, 1: 5, 3: 11}}[case["sel"]]
    g = SW.gen("selection-" + case["sel"])
    return {w: sorted(torch.randperm(case["T"], generator=g)[:k].tolist()) for w, k in Ks.items()}


def token_mask(case):
    B, (H, W) = case["B"], MAP_HW
    m = torch.zeros(B * H * W, dtype=torch.bool)
    if case["pattern"] == "all":
        m[:] = True
    elif case["pattern"] == "every257":
        m[::257] = True
    return m.view(B, H, W)


def make_inputs(case):
    g = SW.gen(bounds_id(case))
    op, C = case["op"], case["C"]
    if op == "score":
        B, L = case["B"], case["L"]
        if case["kind"] == "gauss":
            inp = {"xp": torch.randn(B, L, C, generator=g), "ws_w": torch.randn(C, C, generator=g) / math.sqrt(C), "ws_b": 0.1 * torch.randn(C, generator=g)}
        else:
            inp = {"xp": torch.randint(-16, 17, (B, L, C), generator=g) / 8.0, "ws_w": torch.randint(-16, 17, (C, C), generator=g) / 16.0,
                   "ws_b": (2 * torch.randint(-128, 128, (C,), generator=g) + 1) / 256.0}
        # event ratios in [0, 1): a busy frame, a quiet one (scale of order 1: the sigmoid of the controls is not saturated), an empty one
        rows = torch.tensor([1.0, 0.02, 0.0])[:B] if B == 3 else torch.tensor([0.02])
        inp["r_buf"] = torch.rand(B, 32, generator=g) * rows[:, None]
        inp["wc"] = 1 + 0.1 * torch.randn(C, 20, generator=g)
        if case["kind"] == "inf":
            inp["wc"][list(INF_CHANNELS)] = -math.inf
        inp["g"] = SW.up(g, B, L, C)
        return inp
    if op in MSWSA_OPS:
        NW, T, inner = case["B"] * case["N"], case["T"], case["inner"]
        x = torch.randn(NW, T, C, generator=g)
        if case["cond"]:
            x = 30 + 0.1 * x
        rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc      # noqa: E731
        inp = {"x": x, "ln1_w": 1 + rn(C, sc=0.1), "ln1_b": rn(C, sc=0.1), "ln2_w": 1 + rn(C, sc=0.1), "ln2_b": rn(C, sc=0.1),
               "qkv_w": rn(3 * C, C, sc=C ** -0.5), "qkv_b": rn(3 * C, sc=0.1), "proj_w": rn(C, C, sc=C ** -0.5), "proj_b": rn(C, sc=0.1),
               "ls1": 0.5 + rn(C, sc=0.1), "fc1_w": rn(2 * inner, C, sc=C ** -0.5), "fc1_b": rn(2 * inner, sc=0.1),
               "fc2_w": rn(C, inner, sc=inner ** -0.5), "fc2_b": rn(C, sc=0.1), "ls2": 0.5 + rn(C, sc=0.1)}
        if case["gate_gain"] != 1.0:      # (val, gate) = the two halves of the fc1 output
            inp["fc1_w"][inner:] *= case["gate_gain"]
            inp["fc1_b"][inner:] *= case["gate_gain"]
        if case.get("peaked"):
            inp["qkv_w"].view(C // case["dh"], 3, case["dh"], C)[:, :2] *= 2.0
        if not case["ls"]:
            del inp["ls1"], inp["ls2"]
        if case["act"] == "prelu":
            inp["act_w"] = torch.full((1,), 0.25)
        if case["drop"]:        # one entry per row upper bound; entry m serves the m-th kept row
            inp["drop.d1"] = torch.bernoulli(torch.full((NW * T,), 0.8), generator=g) / 0.8
            inp["drop.d2"] = torch.bernoulli(torch.full((NW * T,), 0.8), generator=g) / 0.8
            inp["drop.mlp"] = torch.bernoulli(torch.full((NW * T, inner), 0.9), generator=g) / 0.9
        inp["g"] = SW.up(g, NW, T, C)
        return inp
    if op in ("mask_token", "add_pos"):
        B, (H, W) = case["B"], MAP_HW
        inp = {"x": torch.randn(B, H, W, C, generator=g), "table": torch.randn(1, H, W, C, generator=g)}
        if op == "mask_token":
            inp["token"] = 0.02 * torch.randn(1, 1, 1, C, generator=g)
            if not case["pe"]:
                del inp["table"]
        inp["g"] = SW.up(g, B, H, W, C)
        return inp
    if op == "lstm":
        B, (H, W) = case["B"], LSTM_HW
        shape = (B, H, W, C)
        inp = {"x": torch.randn(*shape, generator=g), "w": torch.randn(4 * C, 2 * C, 1, 1, generator=g) * (2 * C) ** -0.5, "b": 0.1 * torch.randn(4 * C, generator=g)}
        h0, c0 = 0.5 * torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
        if case["sat"]:
            inp["w"], c0 = inp["w"] * 8.0, c0 * 4.0
        if case["state"] == "given":
            inp["h0"], inp["c0"] = h0, c0
        elif case["state"] == "zero":
            inp["h0"], inp["c0"] = torch.zeros(shape), torch.zeros(shape)
        elif case["state"] == "h0zero":
            inp["h0"] = torch.zeros(shape)
        inp["gh"], inp["gc"] = SW.up(g, *shape), SW.up(g, *shape)
        if case["two"]:
            inp["gh2"] = SW.up(g, *shape)
        if case["drop"]:
            inp["drop"] = torch.bernoulli(torch.full(shape, 0.75), generator=g) / 0.75
        return inp
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------ conditions the cases are stated under
def check_conditions(case, inp):
    """the input conditions of the module docstring, asserted on the inputs and on the float64 reference (CPU and GPU test both call it)"""
    op = case["op"]
    if op == "score":
        assert inp["r_buf"].shape[1] == 32 and inp["r_buf"][:, :20].stride(0) != 20
        if case["B"] == 3:
            assert float(inp["r_buf"][2].abs().max()) == 0.0 and float(inp["r_buf"][0, :20].min()) > 0.0
        if case["kind"] != "gauss":
            for name, step, top in (("xp", 8, 2), ("ws_w", 16, 1)):
                t = inp[name] * step
                assert torch.equal(t, t.round()) and float(inp[name].abs().max()) <= top, name
            b = inp["ws_b"] * 256
            assert torch.equal(b, b.round()) and bool((b.long() % 2 == 1).all())
            z = R.score_preact(inp["xp"].double(), inp["ws_w"].double(), inp["ws_b"].double()) * 256
            assert torch.equal(z, z.round()) and bool((z.long() % 2 == 1).all()), "a pre-activation is not an odd multiple of 1/256"
            assert float(z.abs().min()) >= 1.0 and float(z.abs().max()) < 256 * 2 ** 12
            z32 = R.score_preact(inp["xp"], inp["ws_w"], inp["ws_b"])
            assert torch.equal(z32.double() * 256, z), "the pre-activations are not exact in fp32"
        if case["kind"] == "inf":
            assert bool(torch.isneginf(inp["wc"][list(INF_CHANNELS)]).all()) and int(torch.isinf(inp["wc"]).sum()) == 20 * len(INF_CHANNELS)
            assert float(torch.exp(inp["wc"][list(INF_CHANNELS)]).abs().max()) == 0.0
    elif op in MSWSA_OPS:
        kept = kept_slots(case)
        assert all(0 <= w < case["B"] * case["N"] and v == sorted(set(v)) and 0 <= v[0] and v[-1] < case["T"] for w, v in kept.items())
        if op in ("mswsa", "mswsa_act"):
            assert case["B"] * case["N"] * case["T"] == 160
        if op == "mswsa_act":
            assert case["sel"] == "mix" and case["act"] in ACT_KINKS and case["gate_gain"] == GATE_GAIN
            gate = gate_preactivations(case, inp)
            assert gate.shape == (sum(len(v) for v in kept.values()), case["inner"]) and 2.5 < float(gate.std()) < 3.5, float(gate.std())
            for k in ACT_KINKS[case["act"]]:
                assert min(float((gate < k).double().mean()), float((gate > k).double().mean())) >= 0.01, (k, float((gate > k).double().mean()))
                assert float((gate - k).abs().min()) > KINK_BAND * float(gate.abs().max()), (k, float((gate - k).abs().min()))
        if case["sel"] == "mix":
            assert sorted(len(v) for v in kept.values()) == [1, 3, 7, 12, 19, 20, 20] and 2 not in kept
        elif case["sel"] == "empty2":
            assert all(w < case["N"] for w in kept), "the second sample keeps nothing"
        else:
            Ks = [len(kept[w]) for w in sorted(kept)]
            assert op == "mswsa_part" and case["B"] == 1 and Ks == PART_KS[case["T"]] and max(Ks) == case["T"] and PART_DROPPED not in kept
            assert sorted(kept) == [w for w in range(case["N"]) if w != PART_DROPPED] and case["C"] % case["dh"] == 0
            assert case["env"] in ({}, NOSPLIT) and (not case["env"] or case["T"] <= 96) and (not case["fused"] or case["C"] == 64)
            w = inp["qkv_w"].double().view(case["C"] // case["dh"], 3, case["dh"], case["C"])
            gain = float((w[:, :2].std() / w[:, 2].std()))
            assert (1.8 < gain < 2.2) if case["peaked"] else (0.9 < gain < 1.1), gain
        if case["cond"]:
            rows = inp["x"].double().reshape(-1, case["C"])
            assert float((rows.mean(1) / rows.std(1)).min()) > 100
    elif op in ("mask_token", "add_pos"):
        rows = case["B"] * MAP_HW[0] * MAP_HW[1]
        assert rows % 256 and rows > 3 * 256 and case["C"] % 4 == 0
        if op == "mask_token":
            n = int(token_mask(case).sum())
            assert n == {"none": 0, "all": rows, "every257": -(-rows // 257)}[case["pattern"]]
    elif op == "lstm":
        M = case["B"] * LSTM_HW[0] * LSTM_HW[1]
        assert M == 70 and M % 64
        if case["state"] in ("zero", "h0zero"):
            assert float(inp["h0"].abs().max()) == 0.0
        if case["sat"]:
            z = torch.nn.functional.conv2d(R.nchw(torch.cat([inp["x"], inp["h0"]], -1).double()), inp["w"].double(), inp["b"].double())
            c1 = reference(case, inp, torch.float64)["out:c1"]
            assert 5.0 < float(z.std()) < 8.0 and float((z.abs() > 10).double().mean()) > 0.08 and float(c1.abs().max()) > 8.0


# ------------------------------------------------------------------------------------------------ reference evaluation
MSWSA_OPS = ("mswsa", "mswsa_part", "mswsa_act")
NO_GRAD = ("g", "gh", "gc", "gh2", "r_buf", "table", "drop", "drop.d1", "drop.d2", "drop.mlp")


def _leaves(inp, dtype, grads=True):
    return SW.leaves(inp, dtype, NO_GRAD, grads)


def oracle_drop(case, p):
    """the DropPath / dropout factors of a mswsa case as the oracle takes them: one entry per KEPT row"""
    if not case["drop"]:
        return None
    n = sum(len(v) for v in kept_slots(case).values())
    return p["drop.d1"][:n], p["drop.d2"][:n], p["drop.mlp"][:n]


def gate_preactivations(case, inp):
    """the gate half of the fc1 output on the kept rows, float64: the argument of the case's activation in the reference evaluation"""
    seen, act = [], O.GLU_ACTS[case["act"]]
    O.GLU_ACTS[case["act"]] = lambda gate: (seen.append(gate.detach().clone()), act(gate))[1]
    try:
        reference(dict(case, nograd=True), inp, torch.float64)
    finally:
        O.GLU_ACTS[case["act"]] = act
    assert len(seen) == 1
    return seen[0]


def reference(case, inp, dtype):
    op, out = case["op"], {}
    if op == "score":
        fwd_only = case["kind"] == "inf"
        p = _leaves(inp, dtype, not fwd_only)
        with torch.set_grad_enabled(not fwd_only):
            xw, tok = R.score_stp(p["xp"], p["r_buf"][:, :20], p["ws_w"], p["ws_b"], p["wc"], case["amp"])
        out["out:xw"], out["rel:tok"] = xw.detach(), tok.detach()
        if not fwd_only:
            (xw * p["g"]).sum().backward()
            SW.grads(out, p, only=("wc",) if case["kind"] == "gauss" else None)
        return out
    if op in MSWSA_OPS:
        p = _leaves(inp, dtype, not case["nograd"])
        params = {k: p[k] for k in R.MSWSA_NAMES if k in p}
        lists = R.index_lists(kept_slots(case), case["T"])
        with torch.set_grad_enabled(not case["nograd"]):
            y = R.mswsa(p["x"], lists, case["B"], params, case["dh"], cb=case["cb"], act=case["act"], drop=oracle_drop(case, p))
        out["out:y"] = y.detach()
        if not case["nograd"]:
            (y * p["g"]).sum().backward()
            SW.grads(out, p)
        return out
    if op == "add_pos":
        p = _leaves(inp, dtype)
        y = R.add_pos_embedding(p["x"], p["table"])
        out["out:y"] = y.detach()
        (y * p["g"]).sum().backward()
        SW.grads(out, p)
        return out
    if op == "mask_token":
        p = _leaves(inp, dtype)
        y = R.mask_token(p["x"], token_mask(case), p["token"], p.get("table"))
        out["out:y"] = y.detach()
        (y * p["g"]).sum().backward()
        SW.grads(out, p)
        return out
    if op == "lstm":
        p = _leaves(inp, dtype)
        h1, c1 = R.conv_lstm(p["x"], p.get("h0"), p.get("c0"), p["w"], p["b"], p.get("drop"))
        out["out:h1"], out["out:c1"] = h1.detach(), c1.detach()
        loss = (h1 * p["gh"]).sum() + (c1 * p["gc"]).sum()
        if case["two"]:
            loss = loss + (h1 * p["gh2"]).sum()
        loss.backward()
        SW.grads(out, p)
        return out
    raise KeyError(op)


def compared(case, quantities):
    """the quantities the GPU test compares for this case (a subset of its bounds entry where cases share one)"""
    return sorted(q for q in quantities if not (case.get("nograd") and q != "out:y"))


EXACT = {"mask_token": ("out:y", "grad:x"), "add_pos": ("out:y", "grad:x")}      # copies and single adds: bit equality with the fp32 reference

BOUNDS_CASES = [c for c in ALL_CASES if bounds_id(c) == c["id"]]      # the cases with an entry of their own in the bounds file
float_quantities = sorted
DISCRETE = ()
