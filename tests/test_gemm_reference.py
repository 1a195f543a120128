"""CPU side of the exact-result GEMM tests: a model of the three-way bf16 split and of the six-term product of sast_amd/csrc/gemm.cuh,
written from its description, on the cases of tests/gemm_cases.py.

For every exact family the model with all six terms reproduces the fp64 result bit for bit, and without any term the family claims to
exercise it does not -- so tests/test_gemm_exact.py, which asks the kernels for that same result with torch.equal, fails on a kernel
that loses, doubles or misplaces such a term.  For `prod` the full model stays within the per-product bound and the model without any
one term exceeds it on the chosen operands.  Every case passes its input conditions."""
import pytest
import torch

import gemm_cases as GC

LOW16 = -65536       # 0xffff0000 as int32


def _top(x):
    return (x.contiguous().view(torch.int32) & LOW16).view(torch.float32)


def split3(x):
    """x = h + m + l: the top, middle and bottom 8 significand bits by truncation; the residuals are formed in fp32 (exact)"""
    h = _top(x)
    r1 = x - h
    m = _top(r1)
    l = _top(r1 - m)         # at most 8 significant bits are left: the truncation changes nothing (asserted below)
    return {"h": h, "m": m, "l": l}


def model(A, B, bias=None, drop=None):
    """D = A B^T as the template evaluates it: the six terms in issue order, each added to the fp32 accumulator with one rounding
    (an exact sum of bf16 x bf16 products in fp64), then the bias in fp32.  drop: a term left out"""
    pa, pb = split3(A), split3(B)
    acc = torch.zeros(A.shape[0], B.shape[0])
    for term in GC.TERMS:
        if term != drop:
            acc = (acc.double() + pa[term[0]].double() @ pb[term[1]].double().t()).float()
    return acc if bias is None else (acc.double() + bias.double()).float()


def test_split3_is_exact_and_every_plane_is_a_bf16():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 7, (4096,), generator=g).float(),
                   GC.force_significands(torch.randn(4096, generator=g)), torch.tensor([0.0, 1.0, -1023.0, 2.0 ** -120, 3.0e38])])
    p = split3(x)
    assert torch.equal(p["h"].double() + p["m"].double() + p["l"].double(), x.double())
    r1 = x - p["h"]
    assert torch.equal(r1 - p["m"], p["l"])                                      # the bottom plane needed no truncation
    for q in p.values():
        assert int((q.view(torch.int32) & 0xFFFF).abs().max()) == 0
    nz = x != 0
    assert bool((p["m"].abs()[nz] < 2.0 ** -7 * p["h"].abs()[nz]).all()) and bool((p["l"].abs()[nz] < 2.0 ** -15 * p["h"].abs()[nz]).all())


def test_the_shape_tables_hold_the_edges():
    Rs = {s[2] for s in GC.NT_SHAPES} | {s[2] for s in GC.TN_SHAPES}
    assert 4 in Rs and {1, 200} <= {s[0] for s in GC.NT_SHAPES} and (200, 330) in {s[:2] for s in GC.NT_SHAPES}
    assert any(s[2] == 40 for s in GC.TN_SHAPES)                                   # 3 k-tiles in 8 splits
    for edge in (32, 64, 128):                                                     # BK KS for KS = 2, 4, 8 at BK = 16
        assert any(r < edge for r in Rs) and any(r > edge for r in Rs) and {64, 128} <= Rs
    assert all(s[2] % 4 == 0 for s in GC.NT_SHAPES + GC.GROUP_SHAPES + GC.AUTO_SHAPES)
    assert all(s[0] % 4 == 0 and s[1] % 4 == 0 for s in GC.TN_SHAPES) and all(s[1] % 4 == 0 and s[2] % 4 == 0 for s in GC.PAIR_SHAPES)
    M, N, _R = GC.COUNT_NT_SHAPE
    nb = -(-M // 32) * -(-N // 32)
    assert nb >= 16 and nb % 8
    assert any(m * n <= 128 * 32 * 64 and r >= 512 for m, n, r in GC.AUTO_SHAPES)  # gemm_dispatch.cuh: use_tiny
    assert {f for c in GC.NT_CASES for f in [c["family"]]} == set(GC.FAMILIES) == set(GC.EXERCISES)
    assert len(GC.ALL_CASES) == len(GC.BY_ID)


EXACT_CASES = [c for c in GC.ALL_CASES if c["family"] in GC.EXACT_FAMILIES]
PROD_CASES = [c for c in GC.ALL_CASES if c["family"] == "prod"]


@pytest.mark.parametrize("case", GC.ALL_CASES, ids=[c["id"] for c in GC.ALL_CASES])
def test_input_conditions_hold(case):
    GC.check_conditions(case, GC.make_inputs(case))


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c["id"] for c in EXACT_CASES])
def test_six_terms_give_the_fp64_result_and_five_do_not(case):
    inp = GC.make_inputs(case)
    ref = GC.reference(case, inp)
    for name, (A, B, bias) in GC.products(case, inp).items():
        want = ref[name].float().reshape(A.shape[0], B.shape[0])
        assert torch.equal(want.double(), ref[name].reshape(want.shape))
        assert torch.equal(model(A, B, bias), want), name
        for term in GC.EXERCISES[case["family"]]:
            assert not torch.equal(model(A, B, bias, drop=term), want), (name, "without", term)


@pytest.mark.parametrize("case", PROD_CASES, ids=[c["id"] for c in PROD_CASES])
def test_one_product_stays_inside_the_bound_and_leaves_it_without_any_term(case):
    inp = GC.make_inputs(case)
    ref = GC.reference(case, inp)

    def worst(got, want):
        return float(((got.double() - want).abs() / want.abs()).max())

    for name, (A, B, _bias) in GC.products(case, inp).items():
        want = ref[name].reshape(A.shape[0], B.shape[0])
        assert float(want.abs().min()) > 0.0
        full = worst(model(A, B), want)
        print(f"{case['id']} {name}: six terms {full * 2 ** 23:.2f} x 2^-23")
        assert full <= GC.PROD_BOUND, (name, full)
        for term in GC.TERMS:
            assert worst(model(A, B, drop=term), want) > GC.PROD_BOUND, (name, "without", term)


def test_per_product_error_of_random_significands():
    """the figures behind the bound stated in gemm.cuh: 2^18 operand pairs with random 24-bit significands"""
    g = torch.Generator().manual_seed(2)
    n = 1 << 18
    sig = lambda: (1.0 + torch.randint(0, 1 << 23, (n,), generator=g).double() * 2.0 ** -23).float()      # noqa: E731
    x, y = sig(), sig()
    px, py = split3(x), split3(y)
    want = x.double() * y.double()

    def run(drop=None):
        acc = torch.zeros(n)
        for term in GC.TERMS:
            if term != drop:
                acc = (acc.double() + px[term[0]].double() * py[term[1]].double()).float()
        return (acc.double() - want).abs() / want

    full = run()
    print(f"six terms: max {float(full.max()) * 2 ** 23:.2f} x 2^-23, median {float(full.median()) * 2 ** 23:.2f} x 2^-23")
    assert float(full.max()) <= GC.PROD_BOUND and float(full.max()) > 2.0 ** -23        # the old claim (one rounding) does not hold
    assert float(full.median()) < 0.5 * 2.0 ** -23
    for term in GC.TERMS:
        assert float(run(term).max()) >= 254 * 2.0 ** -23, term
