"""The cases of the exact-result tests of the GEMM template (tests/test_gemm_exact.py on the GPU, tests/test_gemm_reference.py on the
CPU): operand families for which fp32 cannot round, the shape tables, the fp64 references.  CPU only: nothing here imports the library.

The template (sast_amd/csrc/gemm.cuh) evaluates D = A B^T with fp32 operands as six bf16 products over the three-way split x = h + m + l
(top, middle and bottom 8 significand bits).  A term is named with A's plane first: "mh" = A's middle plane times B's top plane.  A family
chooses operands so that every partial sum of every product term is an integer below 2^24, or so that an output is ONE product with a
power of two: then any correct kernel returns the fp64 result to the last bit -- whatever the tile, the number of k-groups, the split
count or the order of the atomics -- and a missing, doubled or misplaced k-tile, a wrong tail or a wrong plane is a difference.

  hh    A, B integers in [-15, 15]                                                      h.h
  mh    A integers in [-1023, 1023], B in [-15, 15]                                     m.h (and h.h)
  hm    the mirror                                                                      h.m (and h.h)
  mm    A integers in [-1023, 1023] inside a window of 16 consecutive r per row (the start moves with the row), zero elsewhere; B dense
        integers in [-1023, 1023]; dense A where R <= 16                                 m.m (and m.h, h.m, h.h)
  lh    A full-precision fp32 (randn); B one non-zero per row j, +-2^e with |e| <= 3, at r_j = (7 j + 3) mod R: the output is
        A[i][r_j] B[j][r_j] exactly -- the three terms add suffixes of one significand   l.h, m.h, h.h
  hl    the mirror                                                                      h.l, h.m, h.h
  prod  A full-precision, B one full-precision non-zero per row: one product per output, held to the per-product bound PROD_BOUND;
        both operands carry forced significands (all ones, 1 + 2^-23, a top plane with a last-place bit)

PROD_BOUND = 1.5 * 2^-21 |x y|: the dropped terms m.l + l.m + l.l are below 2^-21 (1 + 2^-9) |x y| (m < 2^-7 |h|, l < 2^-15 |h|); the
add of h.h is one rounding of the result, at most 2^-23; the adds of the small terms are below 2^-30.

Forms (the entry points of csrc/k_test.hip):  nt  c[M, N] = a[M, R] w[N, R]^T + bias;  tn  out[Mo, NJ] = dy[R, Mo]^T x[R, NJ] with the
column sums of dy;  groups  c[M, G, NJ] = a[M, K] w[G NJ, K]^T;  pair  dw[N, K] = dy[R, N]^T x[R, K], db = column sums of dy,
dx[R, K] = dy w[N, K].  Reduce-contiguous operands need R % 4 == 0, index-contiguous ones index dimensions % 4 == 0 (the loaders read
16 bytes): Mo, NJ of `tn` and N, K of `pair` are multiples of 4, the rows of `pair` and M of `nt` are free.  Bias and column sums are
compared where they are integers too (bias: the integer families; column sums: every family whose A is not full-precision).
"""
import functools

import torch

import operator_sweep as SW

FAMILIES = ("hh", "mh", "hm", "mm", "lh", "hl", "prod")
EXACT_FAMILIES = FAMILIES[:-1]
INTEGER_FAMILIES = ("hh", "mh", "hm", "mm")
TERMS = ("lh", "hl", "mm", "mh", "hm", "hh")        # the issue order of gemm_body::compute, A's plane first
EXERCISES = {"hh": ("hh",), "mh": ("mh",), "hm": ("hm",), "mm": ("mm",), "lh": ("lh", "mh", "hh"), "hl": ("hl", "hm", "hh"), "prod": TERMS}
PROD_BOUND = 1.5 * 2.0 ** -21
LIMIT = float(2 ** 24)
WINDOW = 16

# ------------------------------------------------------------------------------------------------ shapes
# M in {1, 31, 64, 65, 129, 200}, N in {4, 36, 64, 68, 132, 330}, R in {4, 12, 16, 20, 60, 64, 68, 124, 128, 132, 260, 516} (+ 40 for the
# eight-way split): R = 4 is shorter than a k-tile and leaves k-groups without one; 20 | 60, 60 | 68, 124 | 132 lie on both sides of
# BK KS = 32, 64, 128 (KS = 2, 4, 8 at BK = 16); 200 x 330 is a grid of >= 16 tiles that is no multiple of 8 for the 32-row tiles (the
# XCD remap with surplus workgroups)
NT_SHAPES = [(1, 4, 4), (31, 36, 12), (64, 64, 16), (65, 68, 20), (129, 132, 60), (200, 330, 64), (31, 4, 68), (65, 36, 124), (64, 132, 128),
             (129, 68, 132), (31, 64, 260), (65, 4, 516)]
TN_SHAPES = [(4, 4, 4), (36, 68, 12), (64, 64, 16), (68, 36, 20), (132, 132, 60), (64, 132, 64), (36, 4, 68), (68, 64, 124), (4, 36, 128),
             (132, 68, 132), (36, 36, 260), (68, 132, 516), (64, 68, 40)]       # (Mo, NJ, R); R = 40 in 8 splits: empty splits
GROUP_SHAPES = [(1, 4, 4), (65, 36, 68), (129, 68, 132), (31, 132, 260), (200, 36, 16)]       # (M, NJ, K), for G = 2, 3, 4
PAIR_SHAPES = [(65, 68, 36), (200, 260, 132), (31, 516, 4)]       # (R rows, N, K): the dX reduction (N) on both sides of SAST_KS_MINR = 256
AUTO_SHAPES = [(65, 68, 260), (31, 36, 516), (200, 330, 60), (129, 132, 516)]       # (31, 36, 516): small enough for TileTinyK8
COUNT_NT_SHAPE = (200, 330, 20)        # the remap path with a device-side row count for the 32-row tiles
COUNT_TN_SHAPE = (68, 132, 260)
COUNT_GROUP_SHAPE = (200, 36, 16)
COUNT_AUTO_SHAPE = (200, 330, 260)
COUNT_PAIR_SHAPE = (200, 260, 132)


def case(form, family, shape, G=1):
    assert form in ("nt", "tn", "groups", "pair") and family in FAMILIES
    return dict(id=f"{form}{G if form == 'groups' else ''}-{family}-" + "x".join(map(str, shape)), form=form, family=family, shape=tuple(shape), G=G)


NT_CASES = [case("nt", f, s) for s in NT_SHAPES for f in FAMILIES]
TN_CASES = [case("tn", f, s) for s in TN_SHAPES for f in FAMILIES]
GROUP_CASES = [case("groups", f, s, G) for G in (2, 3, 4) for s in GROUP_SHAPES for f in FAMILIES]
PAIR_CASES = [case("pair", f, s) for s in PAIR_SHAPES for f in FAMILIES]
AUTO_CASES = [case("nt", f, s) for s in AUTO_SHAPES for f in FAMILIES]
COUNT_CASES = ([case("nt", f, COUNT_NT_SHAPE) for f in ("hh", "lh")] + [case("tn", f, COUNT_TN_SHAPE) for f in ("hh", "hl")]
               + [case("groups", f, COUNT_GROUP_SHAPE, G) for G in (2, 3, 4) for f in ("hh", "lh")]
               + [case("nt", f, COUNT_AUTO_SHAPE) for f in ("mh", "hl")] + [case("pair", f, COUNT_PAIR_SHAPE) for f in ("hh", "mm", "hl")])
ALL_CASES = list({c["id"]: c for c in NT_CASES + TN_CASES + GROUP_CASES + PAIR_CASES + AUTO_CASES + COUNT_CASES}.values())


# ------------------------------------------------------------------------------------------------ operands
def _ints(g, top, *shape):
    return torch.randint(-top, top + 1, shape, generator=g).float()


def _window(I, R):
    """[I, R] mask: WINDOW consecutive r per row, the start moves by 3 per row, wrapping over the R - WINDOW + 1 places"""
    if R <= WINDOW:
        return torch.ones(I, R, dtype=torch.bool)
    start = (3 * torch.arange(I)) % (R - WINDOW + 1)
    r = torch.arange(R)[None, :]
    return (r >= start[:, None]) & (r < start[:, None] + WINDOW)


def _pow2(g, n):
    return (2.0 ** torch.randint(-3, 4, (n,), generator=g).float()) * (2.0 * torch.randint(0, 2, (n,), generator=g).float() - 1.0)


def force_significands(t):
    """every entry whose flat index is 0, 1 or 2 mod 5 gets a forced significand: all ones | 1 + 2^-23 | seven top bits and the last
    place (a top plane with l = 1 ulp, m = 0); sign and exponent stay"""
    bits = t.contiguous().view(torch.int32).flatten().clone()
    k = torch.arange(bits.numel()) % 5
    keep = bits & ~0x7FFFFF
    bits = torch.where(k == 0, keep | 0x7FFFFF, bits)
    bits = torch.where(k == 1, keep | 0x000001, bits)
    bits = torch.where(k == 2, (bits & ~0x00FFFF) | 0x000001, bits)
    return bits.view(torch.float32).view(t.shape)


def _one_per_row(values, J, R):
    """[J, R] with values[j] at r_j = (7 j + 3) mod R"""
    out = torch.zeros(J, R)
    out[torch.arange(J), (7 * torch.arange(J) + 3) % R] = values
    return out


def operands(family, I, J, R, g):
    """A [I, R], B [J, R] of D = A B^T"""
    if family == "hh":
        return _ints(g, 15, I, R), _ints(g, 15, J, R)
    if family == "mh":
        return _ints(g, 1023, I, R), _ints(g, 15, J, R)
    if family == "hm":
        return _ints(g, 15, I, R), _ints(g, 1023, J, R)
    if family == "mm":
        return _ints(g, 1023, I, R) * _window(I, R), _ints(g, 1023, J, R)
    if family == "lh":
        return torch.randn(I, R, generator=g), _one_per_row(_pow2(g, J), J, R)
    if family == "hl":
        return _one_per_row(_pow2(g, I), I, R), torch.randn(J, R, generator=g)
    if family == "prod":
        return force_significands(torch.randn(I, R, generator=g)), _one_per_row(force_significands(torch.randn(J, generator=g)), J, R)
    raise KeyError(family)


def _pair_operands(family, R, N, K, g):
    """dy [R, N] is the A operand of BOTH jobs (reduced over R in dw, over N in dx); x [R, K] and w [N, K] are the B operands"""
    if family in ("hh", "mh", "hm"):
        ta, tb = (1023 if family == "mh" else 15), (1023 if family == "hm" else 15)
        return _ints(g, ta, R, N), _ints(g, tb, R, K), _ints(g, tb, N, K)
    if family == "mm":       # a band: at most WINDOW entries of every row AND of every column of dy
        P = max(R, N)
        band = ((torch.arange(R)[:, None] + torch.arange(N)[None, :]) % P) < WINDOW
        return _ints(g, 1023, R, N) * band, _ints(g, 1023, R, K), _ints(g, 1023, N, K)
    if family in ("lh", "prod"):
        dy = torch.randn(R, N, generator=g)
        vx, vw = (_pow2(g, K), _pow2(g, K)) if family == "lh" else (force_significands(torch.randn(K, generator=g)), force_significands(torch.randn(K, generator=g)))
        x, w = _one_per_row(vx, K, R).t().contiguous(), _one_per_row(vw, K, N).t().contiguous()
        return (force_significands(dy) if family == "prod" else dy), x, w
    if family == "hl":       # at most one entry per row and per column of dy: row r < N holds one at n_r = (7 r + 3) mod N (7 and N coprime)
        n = min(R, N)
        dy = torch.zeros(R, N)
        dy[torch.arange(n), (7 * torch.arange(n) + 3) % N] = _pow2(g, n)
        return dy, torch.randn(R, K, generator=g), torch.randn(N, K, generator=g)
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = BY_ID[cid]
    g, fam, form = SW.gen("gemm-" + cid), c["family"], c["form"]
    if form == "nt":
        M, N, R = c["shape"]
        a, w = operands(fam, M, N, R, g)
        return {"a": a, "w": w, "bias": _ints(g, 15, N) if fam in INTEGER_FAMILIES else None}
    if form == "tn":
        Mo, NJ, R = c["shape"]
        A, B = operands(fam, Mo, NJ, R, g)
        return {"dy": A.t().contiguous(), "x": B.t().contiguous()}
    if form == "groups":
        M, NJ, K = c["shape"]
        a, w = operands(fam, M, c["G"] * NJ, K, g)
        return {"a": a, "w": w}
    R, N, K = c["shape"]
    dy, x, w = _pair_operands(fam, R, N, K, g)
    return {"dy": dy, "x": x, "w": w}


def make_inputs(c):
    """fp32 CPU tensors of the case (shared: do not modify); None: the entry point gets a null pointer"""
    return _inputs(c["id"])


def has_colsum(c):
    """whether the column sums of the A operand (tn: colsum, pair: db) are exact: not where dy is full-precision"""
    return c["family"] not in ("lh", "prod")


def products(c, inp, count=None):
    """{name: (A, B, bias)} of the abstract products D = A B^T + bias behind the case's outputs; count: the device-side row count"""
    form = c["form"]
    if form in ("nt", "groups"):
        return {"c": (inp["a"], inp["w"], inp.get("bias"))}
    n = inp["dy"].shape[0] if count is None else min(count, inp["dy"].shape[0])
    dy = inp["dy"][:n]
    if form == "tn":
        return {"out": (dy.t(), inp["x"][:n].t(), None)}
    return {"dw": (dy.t(), inp["x"][:n].t(), None), "dx": (dy, inp["w"].t(), None)}


def reference(c, inp, count=None):
    """{output: fp64 tensor}.  A device-side count cuts the reduction of tn / dw and the rows of dx (the caller compares the first
    `count` rows of c / dx; the others keep their prefill)"""
    out = {}
    for name, (A, B, bias) in products(c, inp, count).items():
        out[name] = A.double() @ B.double().t() + (0.0 if bias is None else bias.double())
    if c["form"] == "groups":
        M, NJ, _K = c["shape"]
        out["c"] = out["c"].view(M, c["G"], NJ)
    if c["form"] in ("tn", "pair") and has_colsum(c):
        n = inp["dy"].shape[0] if count is None else min(count, inp["dy"].shape[0])
        out["colsum" if c["form"] == "tn" else "db"] = inp["dy"][:n].double().sum(0)
    return out


# ------------------------------------------------------------------------------------------------ conditions
def _is_int(t, top):
    return torch.equal(t, t.round()) and float(t.abs().max()) <= top


def _pow2_entries(t):
    v = t[t != 0].double().abs()
    e = torch.log2(v)
    return v.numel() > 0 and torch.equal(e, e.round()) and float(e.abs().max()) <= 3


def _forced(t):
    m = t[t != 0].contiguous().view(torch.int32) & 0x7FFFFF
    return bool((m == 0x7FFFFF).any()) and bool((m == 1).any()) and bool(((m & 0xFFFF) == 1).any() and ((m >> 16) != 0).any())


def check_product(family, A, B, bias, single):
    """the family's conditions on one product D = A B^T + bias.  single: the one-entry operand has EXACTLY one entry per row, in the
    documented place (False, the pair form: at most one per row, and the full-precision side may be cut to fewer rows)"""
    (I, R), J = A.shape, B.shape[0]
    assert B.shape[1] == R and A.dtype == B.dtype == torch.float32
    if family in INTEGER_FAMILIES:
        ta, tb = (15 if family in ("hh", "hm") else 1023), (15 if family in ("hh", "mh") else 1023)
        assert _is_int(A, ta) and _is_int(B, tb) and (bias is None or _is_int(bias, 15))
        reach = (A.double().abs() @ B.double().abs().t()).max() + (0.0 if bias is None else float(bias.abs().max()))
        assert float(reach) < LIMIT, float(reach)
        assert float(A.abs().sum(1).max()) < LIMIT        # the column sums of the A operand
        if family == "mm":
            nz = A != 0
            assert int(nz.sum(1).max()) <= WINDOW
            if single and R > WINDOW:        # one window of consecutive r per row
                assert bool((nz <= _window(I, R)).all())
                assert I < 4 or len({int(v) for v in _window(I, R).int().argmax(1)}) > 1       # ... that moves with the row
            assert float(A.abs().max()) > 255 and float(B.abs().max()) > 255       # middle planes on both sides
        elif family != "hh":
            assert float((A if family == "mh" else B).abs().max()) > 255
        return
    assert bias is None
    one, full = (B, A) if family in ("lh", "prod") else (A, B)
    per_row = (one != 0).sum(1)
    assert int(per_row.max()) == 1 and (not single or int(per_row.min()) == 1)
    if single:
        n = one.shape[0]
        assert bool((one[torch.arange(n), (7 * torch.arange(n) + 3) % R] != 0).all())
    assert bool(torch.isfinite(full).all()) and float(full.abs().max()) > 0
    if family == "prod":
        assert _forced(one) and _forced(full)
    else:
        assert _pow2_entries(one)
        low = full.contiguous().view(torch.int32) & 0xFF       # the full-precision side has bottom planes
        assert float((low != 0).float().mean()) > 0.9


def check_conditions(c, inp):
    """the conditions under which the case's results are exact (or, `prod`, one product each), asserted on the inputs in fp64"""
    fam, form = c["family"], c["form"]
    for name, (A, B, bias) in products(c, inp).items():
        check_product(fam, A, B, bias, single=form != "pair")
    if form == "pair":
        R, N, K = c["shape"]
        assert N % 4 == 0 and K % 4 == 0 and inp["dy"].shape == (R, N) and inp["x"].shape == (R, K) and inp["w"].shape == (N, K)
        if fam == "hl":
            assert int((inp["dy"] != 0).sum(0).max()) == 1 and int((inp["dy"] != 0).sum()) == min(R, N)
    elif form == "tn":
        Mo, NJ, R = c["shape"]
        assert Mo % 4 == 0 and NJ % 4 == 0 and inp["dy"].shape == (R, Mo) and inp["x"].shape == (R, NJ)
    else:
        assert c["shape"][2] % 4 == 0
    if form in ("tn", "pair") and has_colsum(c):
        s = inp["dy"].double().sum(0)
        if fam in INTEGER_FAMILIES:
            assert torch.equal(s, s.round()) and float(inp["dy"].double().abs().sum(0).max()) < LIMIT
        else:       # hl: at most one power of two per column
            assert int((inp["dy"] != 0).sum(0).max()) == 1
    ref = reference(c, inp)
    for name, t in ref.items():
        assert bool(torch.isfinite(t).all()), name
        if fam in EXACT_FAMILIES:
            assert torch.equal(t.float().double(), t), (name, "the reference is not an fp32 number")


BY_ID = {c["id"]: c for c in ALL_CASES}
