"""The GEMM template (sast_amd/csrc/gemm.cuh) on operands for which fp32 cannot round (tests/gemm_cases.py): every result is compared
with torch.equal against the fp64 reference cast to fp32 -- for any tile, any number of k-groups, any split count and any order of the
atomics -- so a dropped product term, a wrong plane of the operand split, a missing or doubled k-tile or a wrong tail is an integer
difference, named by the family and the tile that fail.  tests/test_gemm_reference.py shows on the CPU that losing any term a family
exercises changes the result.  `prod` (one full-precision product per output) is held to the derived per-product bound instead and its
worst figure is recorded.

Beyond the tiles of tests/test_gemm_template.py this runs what only whole operators reached: device-side row counts (0, 1, a tile, a
tile + 1, the static bound, beyond it) on every entry point, the seven group tiles the product launches, gemm_auto and the paired
dW || dX launch of gemm_dispatch.cuh under the knobs that move them between tiles, reductions shorter than a k-tile, k-groups and
splits that own no k-tile, M = 1.  Outputs live inside NaN buffers: stores start from NaN, atomics from 0, rows at or beyond a device
count keep their prefill and the guards stay intact."""
import ctypes as C

import pytest
import torch

import conv_cases as CC
import gemm_cases as GC
from conftest import record_error
from operator_sweep import restore_knobs, set_knobs  # noqa: F401  (restore_knobs: autouse fixture)
from test_gemm_buffer_loads import guarded, guarded_out, guards_intact
from test_gemm_template import NT_TILES, TN_TILES

pytestmark = pytest.mark.gpu

NAN = float("nan")
# csrc/k_test.hip: the row-tile height of every NT tile code, the reduction one pass of all k-groups covers (BK KS) of every TN code
NT_BM = {0: 64, 1: 64, 2: 128, 3: 128, 9: 32, 10: 32, 11: 64, 13: 64, 14: 64, 17: 32, 18: 32, 19: 32, 30: 64, 31: 64, 33: 32, 35: 32, 40: 64,
         41: 64, 43: 32, 44: 64}
TN_BKKS = {0: 16, 1: 32, 2: 64, 8: 16, 30: 16, 32: 16, 33: 16, 34: 16, 35: 16, 40: 64, 41: 32, 50: 32, 51: 64, 52: 64, 53: 64, 54: 128}
GROUP_TILES = {0: (2, 64), 1: (2, 64), 2: (2, 32), 3: (3, 64), 4: (3, 32), 5: (4, 64), 6: (4, 32)}       # code: (G, BM)
SPLITS = (1, 3, 8)
ENVS = {"default": {}, "k2": CC.ENV_K2, "thin": CC.ENV_THIN, "k1": CC.ENV_K1, "nopair": {"SAST_GEMM_PAIR": "0"},
        "tnblocks1": {"SAST_TN_BLOCKS_PAIRED": "1"}, "tnblocks192": {"SAST_TN_BLOCKS_PAIRED": "192"}, "noremap": {"SAST_XCD_REMAP": "0"}}
assert set(NT_BM) == set(NT_TILES) and set(TN_BKKS) == set(TN_TILES)


@pytest.fixture(scope="module")
def tools():
    from sast_amd import _lib as L
    lib = L.tools_lib()
    P, I = C.c_void_p, C.c_int
    for name, args in (("sast_test_gemm_nt_dev", [P] * 4 + [I] * 4 + [P] * 2), ("sast_test_gemm_tn_dev", [P] * 4 + [I] * 5 + [P] * 2),
                       ("sast_test_gemm_auto", [P] * 4 + [I] * 3 + [P] * 2), ("sast_test_gemm_pair", [P] * 6 + [I] * 3 + [P] * 2),
                       ("sast_test_gemm_groups", [P] * 3 + [I] * 5 + [P] * 2)):
        getattr(lib, name).restype, getattr(lib, name).argtypes = I, args
    return lib


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


_COUNTS = {}


def count_ptr(n, dev):
    """a device-side row count (None: the entry point gets a null pointer)"""
    if n is None:
        return None
    if n not in _COUNTS:
        _COUNTS[n] = torch.tensor([n], dtype=torch.int32, device=dev)
    return _COUNTS[n].data_ptr()


class Case:
    """the inputs of a case on the device (every operand inside a NaN buffer) and its references by device-side count"""

    def __init__(self, case, dev):
        self.case, self.dev, self.inp = case, dev, GC.make_inputs(case)
        GC.check_conditions(case, self.inp)
        self.d = {k: (None if v is None else guarded(v, dev)[0]) for k, v in self.inp.items()}
        self.refs, self.misses, self.worst = {}, [], 0.0

    def ref(self, count=None):
        if count not in self.refs:
            self.refs[count] = {k: (v, v.float().to(self.dev)) for k, v in GC.reference(self.case, self.inp, count).items()}
        return self.refs[count]

    def compare(self, what, name, got, buf, count=None, rows=None):
        """`got` (a view of the guarded buffer `buf`) against reference `name`; rows: the first `rows` rows are written, the others
        keep their NaN prefill"""
        ref64, ref32 = self.ref(count)[name]
        if not guards_intact(buf):
            self.misses.append(f"{what} {name}: written outside the output")
        if rows is not None:
            if not bool(torch.isnan(got[rows:]).all()):
                self.misses.append(f"{what} {name}: rows at or beyond the count {rows} were written")
            got, ref64, ref32 = got[:rows], ref64[:rows], ref32[:rows]
        if self.case["family"] == "prod":
            err = (got.double().cpu() - ref64).abs() / ref64.abs().clamp_min(1e-300)
            worst = float(err.max()) if err.numel() else 0.0
            self.worst = max(self.worst, worst)
            if not worst <= GC.PROD_BOUND:       # (a NaN left behind misses too)
                self.misses.append(f"{what} {name}: {worst * 2 ** 23:.2f} x 2^-23 of the product, bound {GC.PROD_BOUND * 2 ** 23:.0f} x 2^-23")
        elif not torch.equal(got, ref32):
            diff = (got.double() - ref32.double()).abs()
            self.misses.append(f"{what} {name}: {int((got != ref32).sum())} of {got.numel()} entries differ (largest difference "
                               f"{float(diff.nan_to_num(nan=float('inf')).max()):.6g})")

    def finish(self, test):
        torch.cuda.synchronize()
        if self.case["family"] == "prod":
            print(f"{self.case['id']}: worst product error {self.worst * 2 ** 23:.2f} x 2^-23")
            record_error(test, self.case["id"], self.worst, 1.0, GC.PROD_BOUND)
        assert not self.misses, f"{self.case['id']}:\n  " + "\n  ".join(self.misses[:40]) + f"\n  ({len(self.misses)} misses)"


def launch_nt(tools, k, tile, count=None, auto=False):
    M, N, R = k.case["shape"]
    c, buf = guarded_out((M, N), k.dev, NAN)
    args = (ptr(k.d["a"]), ptr(k.d["w"]), ptr(k.d["bias"]), ptr(c), M, N, R)
    rc = tools.sast_test_gemm_auto(*args, count_ptr(count, k.dev), stream()) if auto else \
        tools.sast_test_gemm_nt_dev(*args, tile, count_ptr(count, k.dev), stream())
    assert rc == 0, (k.case["id"], tile, rc)
    return c, buf


def launch_pair(tools, k, count=None):
    R, N, K = k.case["shape"]
    (dw, dwb), (db, dbb), (dx, dxb) = guarded_out((N, K), k.dev, 0.0), guarded_out((N,), k.dev, 0.0), guarded_out((R, K), k.dev, NAN)
    with_db = GC.has_colsum(k.case)
    rc = tools.sast_test_gemm_pair(ptr(k.d["dy"]), ptr(k.d["x"]), ptr(k.d["w"]), ptr(dw), ptr(db) if with_db else None, ptr(dx), R, N, K,
                                   count_ptr(count, k.dev), stream())
    assert rc == 0, (k.case["id"], rc)
    return (dw, dwb), ((db, dbb) if with_db else None), (dx, dxb)


def compare_pair(k, what, res, count=None):
    (dw, dwb), dbs, (dx, dxb) = res
    k.compare(what, "dw", dw, dwb, count)
    if dbs is not None:
        k.compare(what, "db", dbs[0], dbs[1], count)
    k.compare(what, "dx", dx, dxb, count, rows=None if count is None else min(count, k.case["shape"][0]))


def counts_of(tile_rows, bound):
    return sorted({0, 1, tile_rows, tile_rows + 1, bound, bound + 7})


# ------------------------------------------------------------------------------------------------ tiles
@pytest.mark.parametrize("case", GC.NT_CASES, ids=[c["id"] for c in GC.NT_CASES])
def test_nt_tiles(case, tools, dev):
    """reduce-contiguous A and B through every tile of NT_TILES: 16- and 32-wide k-tiles, 1 to 8 k-groups, presplit and fp32 LDS layouts"""
    k = Case(case, dev)
    for tile in NT_TILES:
        c, buf = launch_nt(tools, k, tile)
        k.compare(f"tile {tile}", "c", c, buf)
    k.finish("test_nt_tiles")


@pytest.mark.parametrize("case", GC.TN_CASES, ids=[c["id"] for c in GC.TN_CASES])
def test_tn_tiles_with_column_sums(case, tools, dev):
    """index-contiguous A and B through every tile of TN_TILES in 1, 3 and 8 splits of the reduction, atomic epilogue, with the column
    sums of dy where they are exact (gemm_cases.has_colsum)"""
    k = Case(case, dev)
    Mo, NJ, R = case["shape"]
    for tile in TN_TILES:
        for splits in SPLITS:
            (out, obuf), (cs, csbuf) = guarded_out((Mo, NJ), dev, 0.0), guarded_out((Mo,), dev, 0.0)
            with_cs = GC.has_colsum(case)
            rc = tools.sast_test_gemm_tn_dev(ptr(k.d["dy"]), ptr(k.d["x"]), ptr(out), ptr(cs) if with_cs else None, Mo, NJ, R, tile, splits,
                                             None, stream())
            assert rc == 0, (case["id"], tile, rc)
            k.compare(f"tile {tile} splits {splits}", "out", out, obuf)
            if with_cs:
                k.compare(f"tile {tile} splits {splits}", "colsum", cs, csbuf)
    k.finish("test_tn_tiles_with_column_sums")


def launch_groups(tools, k, tile, count=None):
    M, NJ, K = k.case["shape"]
    G = k.case["G"]
    c, buf = guarded_out((M, G, NJ), k.dev, NAN)
    rc = tools.sast_test_gemm_groups(ptr(k.d["a"]), ptr(k.d["w"]), ptr(c), M, NJ, K, G, tile, count_ptr(count, k.dev), stream())
    assert rc == 0, (k.case["id"], tile, rc)
    return c, buf


@pytest.mark.parametrize("case", GC.GROUP_CASES, ids=[c["id"] for c in GC.GROUP_CASES])
def test_group_tiles(case, tools, dev):
    """the G = 2 / 3 / 4 tiles the product launches (TileG2, TileG2K2, TileG2K4, TileG3, TileG3K4, TileG4, TileG4K4): G weight rows of
    one output channel in one lane, the group stride of LdWeightNT, the column map of a group tile"""
    k = Case(case, dev)
    for tile, (G, _bm) in GROUP_TILES.items():
        if G == case["G"]:
            c, buf = launch_groups(tools, k, tile)
            k.compare(f"group tile {tile}", "c", c, buf)
    k.finish("test_group_tiles")


# ------------------------------------------------------------------------------------------------ device-side counts
def _count_cases(form, shape):
    return [c for c in GC.COUNT_CASES if c["form"] == form and c["shape"] == shape]


@pytest.mark.parametrize("case", _count_cases("nt", GC.COUNT_NT_SHAPE), ids=lambda c: c["id"])
def test_nt_device_row_count(case, tools, dev):
    """dM on every NT tile: Meff = min(M, *dM), the effective grid of the XCD remap, rows at or beyond the count untouched"""
    k = Case(case, dev)
    M = case["shape"][0]
    for tile in NT_TILES:
        for n in counts_of(NT_BM[tile], M):
            c, buf = launch_nt(tools, k, tile, count=n)
            k.compare(f"tile {tile} count {n}", "c", c, buf, rows=min(n, M))
    k.finish("test_nt_device_row_count")


@pytest.mark.parametrize("case", _count_cases("tn", GC.COUNT_TN_SHAPE), ids=lambda c: c["id"])
def test_tn_device_reduction_count(case, tools, dev):
    """dR on every TN tile and split count: Reff = min(R, *dR); a count of 0 adds nothing"""
    k = Case(case, dev)
    Mo, NJ, R = case["shape"]
    for tile in TN_TILES:
        for splits in SPLITS:
            for n in counts_of(TN_BKKS[tile], R):
                (out, obuf), (cs, csbuf) = guarded_out((Mo, NJ), dev, 0.0), guarded_out((Mo,), dev, 0.0)
                rc = tools.sast_test_gemm_tn_dev(ptr(k.d["dy"]), ptr(k.d["x"]), ptr(out), ptr(cs), Mo, NJ, R, tile, splits, count_ptr(n, dev), stream())
                assert rc == 0, (case["id"], tile, rc)
                k.compare(f"tile {tile} splits {splits} count {n}", "out", out, obuf, count=n)
                k.compare(f"tile {tile} splits {splits} count {n}", "colsum", cs, csbuf, count=n)
    k.finish("test_tn_device_reduction_count")


@pytest.mark.parametrize("case", _count_cases("groups", GC.COUNT_GROUP_SHAPE), ids=lambda c: c["id"])
def test_group_tiles_device_row_count(case, tools, dev):
    k = Case(case, dev)
    M = case["shape"][0]
    for tile, (G, bm) in GROUP_TILES.items():
        if G == case["G"]:
            for n in counts_of(bm, M):
                c, buf = launch_groups(tools, k, tile, count=n)
                k.compare(f"group tile {tile} count {n}", "c", c, buf, rows=min(n, M))
    k.finish("test_group_tiles_device_row_count")


@pytest.mark.parametrize("env", ["default", "k2", "k1"])
@pytest.mark.parametrize("case", _count_cases("nt", GC.COUNT_AUTO_SHAPE), ids=lambda c: c["id"])
def test_auto_device_row_count(case, env, tools, dev, monkeypatch):
    """gemm_auto with dM: the 32-row tile by default (42 tiles: the device-count branch of the remap), the 64-row tiles under the knobs"""
    set_knobs(monkeypatch, ENVS[env])
    k = Case(case, dev)
    M = case["shape"][0]
    for n in sorted(set(counts_of(32, M)) | set(counts_of(64, M))):
        c, buf = launch_nt(tools, k, None, count=n, auto=True)
        k.compare(f"{env} count {n}", "c", c, buf, rows=min(n, M))
    k.finish("test_auto_device_row_count")


@pytest.mark.parametrize("env", ["default", "k2", "nopair"])
@pytest.mark.parametrize("case", _count_cases("pair", GC.COUNT_PAIR_SHAPE), ids=lambda c: c["id"])
def test_pair_device_row_count(case, env, tools, dev, monkeypatch):
    """one count for both jobs of the paired launch: the reduction of dW / db and the rows of dX"""
    set_knobs(monkeypatch, ENVS[env])
    k = Case(case, dev)
    R = case["shape"][0]
    for n in sorted(set(counts_of(32, R)) | set(counts_of(64, R))):
        compare_pair(k, f"{env} count {n}", launch_pair(tools, k, count=n), count=n)
    k.finish("test_pair_device_row_count")


# ------------------------------------------------------------------------------------------------ dispatch
@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("case", GC.AUTO_CASES, ids=[c["id"] for c in GC.AUTO_CASES])
def test_auto_dispatch(case, env, tools, dev, monkeypatch):
    """gemm_auto: TileTinyK8 / TileThinK4 / TileSmallK2 / TileSmall as the knobs decide; every variant equals the reference, so all agree"""
    set_knobs(monkeypatch, ENVS[env])
    k = Case(case, dev)
    c, buf = launch_nt(tools, k, None, auto=True)
    k.compare(env, "c", c, buf)
    k.finish("test_auto_dispatch")


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("case", GC.PAIR_CASES, ids=[c["id"] for c in GC.PAIR_CASES])
def test_pair_dispatch(case, env, tools, dev, monkeypatch):
    """the backward of a linear layer as sast_mswsa_bwd issues it: gemm_dual_kernel (n1 padded to a multiple of 8 in front of a remapped
    dX job, surplus waves of the larger workgroup shape exiting) with each dX tile, one or many splits of dW, and as two launches"""
    set_knobs(monkeypatch, ENVS[env])
    k = Case(case, dev)
    compare_pair(k, env, launch_pair(tools, k))
    k.finish("test_pair_dispatch")
