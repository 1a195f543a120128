"""Random-access training sequences (sast_amd.sampling.RandomAccessPool, the sast_rnd_* entry points of csrc/k_sampler.hip and, for
the window search through a row map, csrc/k_events.hip).

Everything is compared for equality: integers, fp32 label rows and fp64 weights by their bits, frames byte for byte.  The expected
values of the fixture (tests/golden/random_access.npz) were written by the reference's own SequenceDataset / CustomConcatDataset and
get_weighted_random_sampler; a numpy model (tests/random_access_model.py, on top of tests/label_streams_model.py) is pinned to the
fixture on the CPU and stands in for the reference at the batches the fixture does not hold.  Every device row carries stale,
valid-looking records and events past its count."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import label_streams_model as M  # noqa: E402
import random_access_model as RM  # noqa: E402
import make_golden_events as G  # noqa: E402
import make_golden_random_access as GR  # noqa: E402
from pool_labels import labels_of  # noqa: E402

gpu = pytest.mark.gpu

LOAD_EVENTS_LAUNCHES, INDEX_LAUNCHES, INDEX_WEIGHTED_LAUNCHES, BATCH_LAUNCHES, FRAMES_LAUNCHES = 2, 1, 3, 1, 5     # the class docstring
H, W = 240, 304                                  # the Gen1 sensor
LABEL_KW = dict(max_frames=128, max_windows=512, max_labels_per_frame=16)
NAMES = ("rows", "window_idx", "ends_us", "labels", "counts", "labelled", "latest", "latest_count")


@functools.lru_cache(maxsize=None)
def _fx():
    with np.load(os.path.join(GOLDEN, "random_access.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _model(pool, split, ds, L, end):
    return GR.model_pool(pool, split, ds, L, end)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_random_access_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    from sast_amd import sampling as SP
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_rnd_")]
    assert sorted(names) == ["sast_rnd_gather", "sast_rnd_index", "sast_rnd_window_bounds"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert [f for f, _t in _lib.SastRndArgs._fields_] == [
        "start_idx_offset", "length", "cum", "class_total", "weights", "status", "ticket", "sequence_length", "only_load_end_labels",
        "max_classes", "weighted"]
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for (bit, name, _msg), model_bit in ((SP.ROW_FLAGS[0], RM.CLASS_ID), (SP.POOL_FLAGS[0], RM.ITEM_INDEX)):
        assert f"SAST_RND_{name.upper()} = {bit}," in header or f"SAST_RND_{name.upper()} = {bit} " in header, name
        assert bit == model_bit
    import sast_amd.build as B
    assert "k_sampler.hip" in B.SOURCES and B.SOURCE_FLAGS["k_sampler.hip"] == ["-ffp-contract=off"]


def _label_args(**over):
    """a SastLabelArgs of non-null, never dereferenced pointers: the checks run before any launch"""
    from sast_amd import _lib
    a = _lib.SastLabelArgs()
    for f, _t in _lib.SastLabelArgs._fields_[:11]:
        setattr(a, f, 0x1000)
    a.capacity, a.base_delta_us, a.align_t_us, a.delta_t_us = 1024, 250000, 100000, 50000
    a.S, a.width, a.height, a.class_max = 4, 304, 240, -1
    a.min_diag2, a.min_side, a.max_width = 900.0, 10.0, 273.0
    a.reprs_per_frame, a.downsample_by_2, a.max_frames, a.max_windows, a.max_labels_per_frame = 2, 0, 64, 256, 16
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _rnd_args(**over):
    from sast_amd import _lib
    q = _lib.SastRndArgs()
    for f, _t in _lib.SastRndArgs._fields_[:7]:
        setattr(q, f, 0x1000)
    q.sequence_length, q.only_load_end_labels, q.max_classes, q.weighted = 5, 0, 16, 1
    for k, v in over.items():
        setattr(q, k, v)
    return q


def test_random_access_entry_points_reject_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib = _lib.lib()
    EINVAL, p = -22, 0x1000
    before = lib.sast_launch_count()
    used = ("ends_us", "n_windows", "n_frames", "frame_2_window", "window_2_frame", "labels", "frame_start", "frame_count")
    bad_a = [None] + [_label_args(**{f: None}) for f in used]
    bad_a += [_label_args(**kw) for kw in (dict(S=0), dict(S=65536), dict(capacity=0), dict(capacity=2 ** 27), dict(max_frames=0),
                                           dict(max_windows=0), dict(max_labels_per_frame=0), dict(max_windows=2 ** 30))]
    bad_q = [None] + [_rnd_args(**{f: None}) for f in ("start_idx_offset", "length", "cum", "class_total", "status", "ticket")]
    bad_q += [_rnd_args(**kw) for kw in (dict(sequence_length=0), dict(sequence_length=65536), dict(max_classes=0), dict(max_classes=257))]
    ok_a, ok_q = _label_args(), _rnd_args()

    def ref(v):
        return None if v is None else C.byref(v)

    for a in bad_a:
        assert lib.sast_rnd_index(ref(a), ref(ok_q), None) == EINVAL
        assert lib.sast_rnd_gather(ref(a), ref(ok_q), p, 4, *([p] * 8), None) == EINVAL
    for q in bad_q:
        assert lib.sast_rnd_index(ref(ok_a), ref(q), None) == EINVAL
        assert lib.sast_rnd_gather(ref(ok_a), ref(q), p, 4, *([p] * 8), None) == EINVAL
    assert lib.sast_rnd_index(ref(ok_a), ref(_rnd_args(weights=None)), None) == EINVAL          # weighted, but nowhere to put them
    for k in range(9):
        ptrs = [p] * 9
        ptrs[k] = None
        assert lib.sast_rnd_gather(ref(ok_a), ref(ok_q), ptrs[0], 4, *ptrs[1:], None) == EINVAL
    for B in (0, -1, 2 ** 26):
        assert lib.sast_rnd_gather(ref(ok_a), ref(ok_q), p, B, *([p] * 8), None) == EINVAL
    # t, counts, R, stream_capacity, rows, ends_us, B, T, mode, value, bounds
    good = [p, p, 3, 1000, p, p, 4, 5, 0, 50000, p]
    for k, v in ((0, None), (1, None), (4, None), (5, None), (10, None), (2, 0), (2, 65536), (3, -1), (3, 2 ** 30), (6, 0), (7, 0),
                 (7, 2 ** 30), (8, 2), (9, -1)):
        args = list(good)
        args[k] = v
        assert lib.sast_rnd_window_bounds(*args, None) == EINVAL, (k, v)
    assert lib.sast_launch_count() == before


def _cpu_labels(R=3):
    from sast_amd.labels import LabelStreams
    return LabelStreams(R, 100, max_frames=8, max_windows=32, max_labels_per_frame=4)


def test_random_access_pool_constructor_validation():
    from sast_amd.labels import LabelStreams
    from sast_amd.sampling import RandomAccessPool
    ls = _cpu_labels()
    pool = RandomAccessPool(ls, H, W, sequence_length=5)
    assert pool.get_shape() == (20, H, W) and pool.num_rows == 3 and pool.frame_dtype == torch.uint8
    md = RandomAccessPool(ls, H, W, sequence_length=5, representation="mixed_density", count_cutoff=None)
    assert md.get_shape() == (10, H, W) and md.frame_dtype == torch.int8
    ds = RandomAccessPool(LabelStreams(2, 100, downsample_by_2=True), H, W, sequence_length=3, downsample_by_2=True)
    assert ds.get_shape() == (20, H // 2, W // 2)
    with pytest.raises(TypeError):
        RandomAccessPool(None, H, W, sequence_length=5)
    for bad in (dict(sequence_length=0), dict(sequence_length=65536), dict(sequence_length=2.0), dict(max_classes=0), dict(max_classes=257),
                dict(duration_us=None), dict(duration_us=-1), dict(downsample_by_2=True), dict(representation="voxel"), dict(bins=0)):
        with pytest.raises(ValueError):
            RandomAccessPool(ls, H, W, **{**dict(sequence_length=5), **bad})
    assert pool.errors() == ([(), (), ()], ()) and pool.frame_errors() == (0, 0)


def test_random_access_pool_call_validation_and_cpu_tensors_raise():
    from sast_amd.sampling import RandomAccessBatch, RandomAccessPool
    ls = _cpu_labels()
    pool = RandomAccessPool(ls, H, W, sequence_length=3)
    col, cnt = torch.zeros(3, 50, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError):
        pool.load_events(col.to(torch.float32), col, col, col, cnt)
    with pytest.raises(TypeError):
        pool.load_events(col, col, col, col.to(torch.int16), cnt)
    flipped = col.t().contiguous().t()
    for x, y, p, t, c, rs in ((col[:2], col[:2], col[:2], col[:2], cnt, None), (col, col, col, col[:, :40], cnt, None),
                              (flipped, col, col, col, cnt, None), (col, col, col, col, cnt.to(torch.int32), None),
                              (col, col, col, col, cnt[:2], None), (col, col, col, col, cnt, torch.zeros(3, dtype=torch.int32)),
                              (col, col, col, col, cnt, torch.zeros(2, dtype=torch.uint8)),
                              (col[:, :0], col[:, :0], col[:, :0], col[:, :0], cnt, None), (col[0], col[0], col[0], col[0], cnt, None)):
        with pytest.raises(ValueError):
            pool.load_events(x, y, p, t, c, rs)
    for items in (torch.zeros(4, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                  torch.zeros(8, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError):
            pool.batch(items)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pool.load_events(col, col, col, col, cnt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pool.load_events(col, col, col, col, cnt, torch.ones(3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pool.batch(torch.zeros(4, dtype=torch.int64))
    want = pool._want(4)
    cpu_batch = RandomAccessBatch(*(torch.zeros(sh, dtype=dt) for sh, dt in want))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pool.frames(cpu_batch)
    with pytest.raises(RuntimeError, match="labels.load"):
        pool.index()
    with pytest.raises(RuntimeError, match="index"):
        pool.labelled_pairs([0, 1])


@pytest.mark.parametrize("pool,split,ds,L,end", GR.case_keys())
def test_model_equals_the_reference_fixture(pool, split, ds, L, end):
    fx, key = _fx(), GR.key_of(pool, split, ds, L, end)
    p = _model(pool, split, ds, L, end)
    assert np.array_equal(p.start_idx_offset, fx[f"{key}/start_idx_offset"]) and np.array_equal(p.length, fx[f"{key}/length"])
    assert np.array_equal(p.cum[1:], fx[f"{key}/cumulative_sizes"]) and p.N == len(fx[f"{key}/item_windows"]) > 0
    assert [p.locate(g)[2:] for g in range(p.N)] == [tuple(w) for w in fx[f"{key}/item_windows"].tolist()]
    assert p.locate(-1) is None and p.locate(p.N) is None
    step_counts, step_labels = fx[f"{key}/step_counts"], fx[f"{key}/step_labels"]
    Mx = 16
    out = p.batch(list(range(p.N)), Mx)
    rows, widx, _ends, labels, counts, labelled, latest, latest_count = out
    assert np.array_equal(labelled.T, step_counts >= 0) and np.array_equal(counts.T, np.maximum(step_counts, 0))
    assert np.array_equal(widx[0], fx[f"{key}/item_windows"][:, 0]) and np.array_equal(widx[-1] + 1, fx[f"{key}/item_windows"][:, 1])
    assert np.array_equal(rows, np.repeat(np.arange(len(p.rows)), p.length))
    got = np.concatenate([labels[k, g, :counts[k, g]] for g in range(p.N) for k in range(L)] + [np.zeros((0, 7), np.float32)])
    assert np.array_equal(_bits(got), _bits(step_labels))
    for g in range(p.N):                                  # the most recent step that holds a box
        ks = [k for k in range(L) if step_counts[g, k] > 0]
        assert latest_count[g] == (step_counts[g, ks[-1]] if ks else 0)
        if ks:
            assert np.array_equal(_bits(latest[g]), _bits(labels[ks[-1], g]))
    total, weights = p.weights()
    assert np.array_equal(_bits(weights), _bits(fx[f"{key}/weights"])) and total.sum() == np.maximum(step_counts, 0).sum()
    assert p.status == [0] * len(p.rows) and p.labelled_pairs(range(p.N)) == int((step_counts >= 0).sum())


def test_fixture_inputs_meet_the_conditions():
    GR.check_inputs()
    fx = _fx()
    assert fx["gen1/train/full/L11/all/length"][1] == 0 and fx["gen1/train/full/L11/all/length"][2] > 0
    assert (fx["gen1/train/full/L3/all/start_idx_offset"] > 0).any()
    assert (fx["gen1/train/full/L3/all/item_windows"][:, 0] == 0).any()
    sc = fx["gen1/val/full/L11/all/step_counts"]
    assert ((sc[:, 0] >= 0) & (sc[:, 1] < 0) & (sc[:, 2] >= 0)).any()              # an unlabelled step between two labelled ones
    assert not np.array_equal(fx["gen1/train/full/L11/all/weights"], fx["gen1/train/full/L11/end/weights"])
    assert (fx["gen1/train/full/L5/end/step_counts"][:, :-1] == -1).all()


@pytest.mark.skipif(not GR.reference_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_random_access_fixture():
    new, old = GR.generate(), _fx()
    assert sorted(new) == sorted(old)
    for k in new:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert np.ascontiguousarray(new[k]).tobytes() == np.ascontiguousarray(old[k]).tobytes(), k


def test_model_flags_a_class_outside_the_table_and_leaves_it_out():
    p = GR.model_pool("gen4", "val", False, 3, False)
    small = RM.Pool(p.rows, 3, False, max_classes=2)          # gen4 keeps class ids 0 .. 2
    total, weights = small.weights()
    assert small.status == [RM.CLASS_ID] and len(total) == 2 and np.array_equal(total, p.weights()[0][:2]) and (weights > 0).any()


# ---------------------------------------------------------------------------------------------------------------------------- GPU

@functools.lru_cache(maxsize=None)
def _words(pool):
    return tuple(M.pack(GR.pool_records(n)) for n in GR.POOLS[pool])


def _labels(pool, split, ds):
    """a loaded LabelStreams of the pool's recordings, stale records behind every row's count"""
    from sast_amd.labels import LabelStreams
    rows = _words(pool)
    cap = max(len(w) for w in rows) + 5
    rec = np.stack([np.resize(rows[0][-40:], (cap, 10)) for _ in rows])
    for s, w in enumerate(rows):
        rec[s, :len(w)] = w
    ls = LabelStreams(len(rows), cap, dataset=GR.dataset_of(pool), split=split, downsample_by_2=ds, **LABEL_KW)
    ls.load(torch.from_numpy(rec).cuda(), torch.tensor([len(w) for w in rows], dtype=torch.int64, device="cuda"))
    return ls


N_EV = (4000, 3000, 3500, 2500)


@functools.lru_cache(maxsize=None)
def _event_columns(R, salt=0):
    """R rows of hashed events over the ~20 s the label schedules span, one event in 16 out of order, different counts, stale events
    behind every count -> (x, y, p, t) int64 [R, cap] numpy, counts"""
    cap = max(N_EV) + 3
    cols = [np.zeros((R, cap), np.int64) for _ in range(4)]
    for r in range(R):
        ev = G.stream(seed=70 + 10 * salt + r, n=cap, height=H, width=W, t_start=0, t_step=10000, jitter=3000)
        for c, e in zip(cols, ev):
            c[r] = e
        cols[3][r, N_EV[r]:] = cols[3][r, N_EV[r] // 2]          # stale: times in the middle of the row
    return tuple(cols), np.asarray(N_EV[:R], np.int64)


def _cuda(cols, counts):
    return [torch.from_numpy(c).cuda() for c in cols], torch.from_numpy(counts).cuda()


def _pool(ls, L, end=False, **kw):
    from sast_amd.sampling import RandomAccessPool
    return RandomAccessPool(ls, ls.height, ls.width, sequence_length=L, only_load_end_labels=end, **kw)


def _same_batch(got, want):
    for g, w, name in zip(got, want, NAMES):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(_bits(g), _bits(w)), name


@gpu
@pytest.mark.parametrize("pool,split,ds", [(p, s, d) for p in GR.POOLS for s in GR.SPLITS for d in (False, True)])
def test_index_equals_the_model_and_the_reference_weights(pool, split, ds):
    fx = _fx()
    ls = _labels(pool, split, ds)
    R, F = ls.num_streams, ls.max_frames
    assert ls.errors() == [()] * R
    for L in GR.LENGTHS:
        for end in (False, True):
            key, m = GR.key_of(pool, split, ds, L, end), _model(pool, split, ds, L, end)
            rp = _pool(ls, L, end, downsample_by_2=ds)
            n, sizes = rp.index(weighted=True)
            assert n == m.N == len(fx[f"{key}/weights"]) and sizes == m.cum[1:] == fx[f"{key}/cumulative_sizes"].tolist()
            assert rp.start_idx_offset.tolist() == m.start_idx_offset == fx[f"{key}/start_idx_offset"].tolist()
            assert rp.length.tolist() == m.length and rp.cum.tolist() == m.cum
            weights = rp.weights.cpu().numpy()
            assert weights.shape == (R * F,) and weights.dtype == np.float64
            assert np.array_equal(_bits(weights[:n]), _bits(fx[f"{key}/weights"])) and not _bits(weights[n:]).any()
            assert np.array_equal(rp.class_total.cpu().numpy(), m.weights()[0])
            assert rp.errors() == ([()] * R, ())
            # unweighted: the same index, and a second call replays on the same state
            rp.weights.fill_(7.0)
            assert rp.index() == (n, sizes) and rp.cum.tolist() == m.cum and int(rp._ticket) == 0
            assert bool((rp.weights == 7.0).all()) and not bool(rp.class_total.any())


@gpu
def test_index_flags_a_class_outside_the_table():
    ls = _labels("gen4", "val", False)
    m = RM.Pool(GR.model_pool("gen4", "val", False, 3, False).rows, 3, False, max_classes=2)
    rp = _pool(ls, 3, max_classes=2)
    n, _sizes = rp.index(weighted=True)
    total, weights = m.weights()
    assert np.array_equal(rp.class_total.cpu().numpy(), total) and np.array_equal(_bits(rp.weights[:n].cpu().numpy()), _bits(weights))
    assert rp.errors() == ([("class_id",)], ()) and m.status == [RM.CLASS_ID]
    rp.index()
    assert rp.errors() == ([()], ())


def _batch_items(m):
    """gen1 pool: the first and the last item of the dataset, two items of one row, the first item of a row behind a length-0 row"""
    assert m.length[1] == 0 and m.length[0] > 6 and m.length[2] > 4
    items = [0, m.N - 1, 5, m.cum[2]]
    assert [m.locate(g)[0] for g in items] == [0, 2, 0, 2]
    return items


@gpu
@pytest.mark.parametrize("pool", ["gen1", "gen4"])
@pytest.mark.parametrize("L", [3, 5])
@pytest.mark.parametrize("end", [False, True])
def test_batch_equals_the_model(pool, L, end):
    """gen1: rows of different lengths with an empty one between them; gen4: one row of the larger sensor's labels"""
    ls = _labels(pool, "train", False)
    R, Mx = ls.num_streams, LABEL_KW["max_labels_per_frame"]
    m = RM.Pool(_model(pool, "train", False, L, end).rows, L, end)
    rp = _pool(ls, L, end)
    rp.index()
    items = _batch_items(m) if pool == "gen1" else [0, m.N - 1, 5, 6]
    dev_items = torch.tensor(items, dtype=torch.int64, device="cuda")
    out = rp.batch(dev_items)
    want = m.batch(items, Mx)
    _same_batch(out, want)
    window_idx, counts, labelled, latest_count = want[1], want[4], want[5], want[7]
    assert labelled[-1].all() and counts[-1].min() > 0 and latest_count.min() > 0
    if pool == "gen1":
        assert L != 3 or window_idx[0, 3] == 0                      # an item whose first window is window 0
    # two windows per label period: the step before the last is unlabelled, earlier ones are labelled again
    assert (labelled[-2] == 0).all() and (labelled[:-1].sum() == 0 if end else labelled[:-1].sum() >= 3)
    assert rp.errors() == ([()] * R, ())
    assert rp.labelled_pairs(items) == m.labelled_pairs(items) == int(labelled.sum()) == rp.labelled_pairs(torch.tensor(items))
    # `out` is written in place
    again = tuple(torch.full_like(t, 7) for t in out)
    res = rp.batch(dev_items, out=again)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(res, again)) and all(torch.equal(a, b) for a, b in zip(out, again))
    # the whole dataset in one batch
    everything = list(range(m.N))
    _same_batch(rp.batch(torch.tensor(everything, dtype=torch.int64, device="cuda")), m.batch(everything, Mx))
    assert ls.errors() == [()] * R


@gpu
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("end", [False, True])
def test_batch_reads_the_label_state_as_the_gather_does(L, end):
    """`batch` and `LabelStreams.labels` (and `StreamingPool.next`, held to the same gather in tests/test_streaming_pool.py) read one
    state through one reader: frames cut to max_labels_per_frame = 4, and a label frame without boxes.  The loader itself never leaves
    such a frame (the filters keep w, h >= 5, which scale_(0.5) cannot flatten), so one frame's count is set to 0 in the device state:
    labelled stays 1, counts is 0, and `latest` has to step over it."""
    from sast_amd.labels import LabelStreams
    rows = _words("gen1")
    R, cap = len(rows), max(len(w) for w in rows) + 5
    rec = np.stack([np.resize(rows[0][-40:], (cap, 10)) for _ in rows])
    for s, w in enumerate(rows):
        rec[s, :len(w)] = w
    ls = LabelStreams(R, cap, dataset="gen1", split="train", max_frames=128, max_windows=512, max_labels_per_frame=4, downsample_by_2=True)
    ls.load(torch.from_numpy(rec).cuda(), torch.tensor([len(w) for w in rows], dtype=torch.int64, device="cuda"))
    assert R == 3 and ls.errors() == [("frame_overfull",)] * R
    rp = _pool(ls, L, end, downsample_by_2=True)
    n, sizes = rp.index()
    items = [0, 5, sizes[1], n - 1]                               # two samples in row 0, two in row 2
    emptied = rp.start_idx_offset.tolist()[0] + 5                 # the label frame item 5 ends at
    ls.frame_count[0, emptied] = 0
    out = rp.batch(torch.tensor(items, dtype=torch.int64, device="cuda"))
    assert out.rows.tolist() == [0, 0, 2, 2]
    ref = labels_of(ls, out, R)
    assert max(int(c.max()) for _l, c, _e, _d in ref) == 4        # a frame cut to the four rows a step holds
    assert int(ref[1][1][-1]) == 0 and int(ref[1][3][-1]) == 1    # the emptied frame: labelled, no box
    for b, (labels, counts, ends, labelled) in enumerate(ref):
        first = L - 1 if end else 0                               # only_load_end_labels: the steps before the last read as unlabelled
        assert torch.equal(out.ends_us[:, b], ends)
        for got, exp in ((out.labels[:, b], labels), (out.counts[:, b], counts), (out.labelled[:, b], labelled)):
            assert torch.equal(got[first:], exp[first:]) and not bool(got[:first].any())
        full = [k for k in range(first, L) if int(counts[k]) > 0]
        if full:
            assert torch.equal(out.latest[b], labels[full[-1]]) and int(out.latest_count[b]) == int(counts[full[-1]]) > 0
        else:
            assert not bool(out.latest[b].any()) and int(out.latest_count[b]) == 0
    assert (int(out.latest_count[1]) > 0) == (L == 3 and not end)  # item 5: an earlier step's frame, or none
    assert rp.errors() == ([()] * R, ()) and ls.errors() == [("frame_overfull",)] * R


@gpu
def test_an_item_out_of_range_is_flagged_and_leaves_the_other_samples_alone():
    L = 3
    ls = _labels("gen1", "val", False)
    m = RM.Pool(_model("gen1", "val", False, L, False).rows, L)
    rp = _pool(ls, L)
    n, _ = rp.index()
    cols, counts = _cuda(*_event_columns(3))
    rp.load_events(*cols, counts)
    good = [4, m.cum[2] + 1]
    items = [-1, good[0], n, good[1]]
    out = rp.batch(torch.tensor(items, dtype=torch.int64, device="cuda"))
    _same_batch(out, m.batch(items, LABEL_KW["max_labels_per_frame"]))
    assert out.rows.tolist() == [-1, 0, -1, 2] and out.window_idx[:, 0].tolist() == [-1] * L and out.ends_us[:, 2].tolist() == [-1] * L
    assert int(out.counts[:, [0, 2]].sum()) == 0 and int(out.latest_count[0]) == 0 and not bool(out.labels[:, [0, 2]].any())
    assert rp.errors() == ([(), (), ()], ("item_index",)) and m.pool_status == RM.ITEM_INDEX
    frames = rp.frames(out)
    alone = rp.batch(torch.tensor(good, dtype=torch.int64, device="cuda"))
    alone_frames = rp.frames(alone)
    for name, t_all, t_good in zip(NAMES, out, alone):
        sel = t_all[[1, 3]] if name in ("rows", "latest", "latest_count") else t_all[:, [1, 3]]
        assert torch.equal(sel, t_good), name
    assert torch.equal(frames[:, [1, 3]], alone_frames) and int(alone_frames.count_nonzero()) > 0
    assert not bool(frames[:, [0, 2]].any()) and rp.frame_errors() == (0, 0)
    assert rp.labelled_pairs(items) == rp.labelled_pairs(good) == int(alone.labelled.sum())
    rp.index()
    assert rp.errors() == ([(), (), ()], ())


@gpu
@pytest.mark.parametrize("representation", ["stacked_histogram", "mixed_density"])
def test_frames_equal_event_streams_window_by_window(representation):
    from sast_amd.events import EventStreams
    L, R = 5, 3
    ls = _labels("gen1", "train", False)
    m = _model("gen1", "train", False, L, False)
    kw = dict(bins=4, count_cutoff=5, duration_us=50000, representation=representation)
    rp = _pool(ls, L, **kw)
    rp.index()
    cols, counts = _cuda(*_event_columns(R))
    rp.load_events(*cols, counts)
    items = _batch_items(m)
    out = rp.batch(torch.tensor(items, dtype=torch.int64, device="cuda"))
    frames = rp.frames(out)
    assert frames.shape == (L, 4) + rp.get_shape() and frames.dtype == rp.frame_dtype and rp.frame_errors() == (0, 0)
    es = EventStreams(R, H, W, **kw)
    ones = torch.ones(R, dtype=torch.uint8, device="cuda")
    rows, ends = out.rows.tolist(), out.ends_us
    for b, r in enumerate(rows):
        per_row = torch.zeros(L, R, dtype=torch.int64, device="cuda")
        per_row[:, r] = ends[:, b]
        want = es(*cols, counts, per_row, reset=ones)
        assert torch.equal(frames[:, b], want[:, r]), b
        assert int(want[:, r].count_nonzero()) > 0
    es_t = es._state["t"].view(R, -1)
    for r in range(R):                                            # the corrected timestamps are EventStreams'
        assert torch.equal(rp.t[r, :N_EV[r]], es_t[r, :N_EV[r]]) and not torch.equal(rp.t[r, :N_EV[r]], cols[3][r, :N_EV[r]])
    assert es.errors() == (0, 0)
    assert rows[0] == rows[2] and not torch.equal(frames[:, 0], frames[:, 2])
    into = torch.full_like(frames, 9)
    assert rp.frames(out, out_frames=into).data_ptr() == into.data_ptr() and torch.equal(into, frames)


@gpu
def test_partial_load_events_leaves_the_other_rows_bit_identical():
    from sast_amd.events import EventStreams
    L, R = 3, 3
    ls = _labels("gen1", "train", False)
    m = _model("gen1", "train", False, L, False)
    rp = _pool(ls, L, bins=4)
    rp.index()
    cols, counts = _cuda(*_event_columns(R))
    rp.load_events(*cols, counts)
    items = torch.tensor([3, m.cum[2] + 2, 9, m.N - 1], dtype=torch.int64, device="cuda")
    out = rp.batch(items)
    assert out.rows.tolist() == [0, 2, 0, 2]
    before_t, before_frames = rp.t.clone(), rp.frames(out).clone()
    other, other_counts = _cuda(*_event_columns(R, salt=1))
    new = [c.clone() for c in cols]
    for c, o in zip(new, other):
        c[1] = o[1]
    new_counts = torch.tensor([17, 2800, 23], dtype=torch.int64, device="cuda")     # rows 0 and 2 are not reset: their counts are not taken
    rp.load_events(*new, new_counts, reset=torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda"))
    assert torch.equal(rp.t[0], before_t[0]) and torch.equal(rp.t[2], before_t[2]) and not torch.equal(rp.t[1], before_t[1])
    assert rp.counts.tolist() == [N_EV[0], 2800, N_EV[2]]
    assert torch.equal(rp.frames(out), before_frames)
    es = EventStreams(R, H, W, bins=4, duration_us=50000)
    full_counts = torch.tensor([N_EV[0], 2800, N_EV[2]], dtype=torch.int64, device="cuda")
    es(*new, full_counts, torch.zeros(R, dtype=torch.int64, device="cuda"), reset=torch.ones(R, dtype=torch.uint8, device="cuda"))
    want_t = es._state["t"].view(R, -1)
    assert torch.equal(rp.t[1, :2800], want_t[1, :2800])
    rp.load_events(*new, full_counts, reset=torch.tensor([True, False, True], device="cuda"))
    assert torch.equal(rp.t[0], before_t[0]) and torch.equal(rp.t[1, :2800], want_t[1, :2800])


@gpu
def test_random_access_launch_counts_are_the_documented_ones():
    from sast_amd import _lib
    from sast_amd.sampling import RandomAccessPool
    lib = _lib.lib()
    assert (RandomAccessPool.LOAD_EVENTS_LAUNCHES, RandomAccessPool.INDEX_LAUNCHES, RandomAccessPool.INDEX_WEIGHTED_LAUNCHES,
            RandomAccessPool.BATCH_LAUNCHES, RandomAccessPool.FRAMES_LAUNCHES) == (
        LOAD_EVENTS_LAUNCHES, INDEX_LAUNCHES, INDEX_WEIGHTED_LAUNCHES, BATCH_LAUNCHES, FRAMES_LAUNCHES)
    ls = _labels("gen1", "train", False)
    cols, counts = _cuda(*_event_columns(3))

    def launches(fn):
        before = lib.sast_launch_count()
        res = fn()
        return lib.sast_launch_count() - before, res

    for L in (3, 5):
        for representation in ("stacked_histogram", "mixed_density"):
            rp = _pool(ls, L, bins=4, representation=representation)
            for reset in (None, torch.tensor([0, 1, 1], dtype=torch.uint8, device="cuda")):
                assert launches(lambda: rp.load_events(*cols, counts, reset=reset))[0] == LOAD_EVENTS_LAUNCHES
            assert launches(rp.index)[0] == INDEX_LAUNCHES
            assert launches(lambda: rp.index(weighted=True))[0] == INDEX_WEIGHTED_LAUNCHES
            for B in (1, 4, 7):
                n, out = launches(lambda: rp.batch(torch.arange(B, dtype=torch.int64, device="cuda")))
                assert n == BATCH_LAUNCHES, (L, B)
                assert launches(lambda: rp.frames(out))[0] == FRAMES_LAUNCHES, (L, B)


@gpu
def test_batch_frames_and_augmentation_in_one_graph():
    """batch + frames + SpatialAugmentor(yolox=True) captured once after a warm-up, replayed on a second set of items written into the
    same tensor == the eager run on those items"""
    import make_golden_augment as GA
    from sast_amd import augment as A
    L, R, B = 3, 3, 4
    ls = _labels("gen1", "train", False)
    m = _model("gen1", "train", False, L, False)
    rp = _pool(ls, L, bins=4)
    rp.index()
    cols, counts = _cuda(*_event_columns(R))
    rp.load_events(*cols, counts)
    aug = A.SpatialAugmentor((H, W), GA.SHIPPED["random"], B)
    aug.set_state([A.AugmentationState(apply_h_flip=True), A.AugmentationState(zoom_out=A.ZoomOutState(True, 20, 10, 1.25)),
                   A.AugmentationState(), A.AugmentationState(apply_h_flip=True)])
    sets = [[2, m.cum[2] + 1, 7, 8], [m.N - 1, 0, m.cum[2], 11]]
    items = torch.zeros(B, dtype=torch.int64, device="cuda")

    def call():
        out = rp.batch(items)
        frames = rp.frames(out)
        return aug(frames, out.labels, out.counts, yolox=True) + (out.rows, out.ends_us, out.labelled, out.latest, out.latest_count)

    eager = []
    for st in sets:
        items.copy_(torch.tensor(st))
        eager.append([t.clone() for t in call()])
    assert int(eager[1][0].count_nonzero()) > 0 and int(eager[1][2].sum()) > 0 and not torch.equal(eager[0][0], eager[1][0])
    items.copy_(torch.tensor(sets[0]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = call()
    for st, want in zip(sets, eager):
        items.copy_(torch.tensor(st))
        g.replay()
        torch.cuda.synchronize()
        for got, exp in zip(captured, want):
            assert torch.equal(got, exp)
    assert rp.errors() == ([(), (), ()], ()) and rp.frame_errors() == (0, 0) and ls.errors() == [(), (), ()]
