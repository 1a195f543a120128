"""Streamed training / evaluation sequences (sast_amd.sampling.StreamingPool, the sast_stream_* entry points of csrc/k_stream.hip and,
for the frames, the row-mapped window search of csrc/k_events.hip).

Everything is compared for equality: integers, fp32 label rows by their bits, frames byte for byte.  The expected values of the fixture
(tests/golden/streaming.npz) were written by the reference's own SequenceForIter and ShardedStreamingDataPipe; a numpy model
(tests/streaming_model.py, on top of tests/label_streams_model.py) is pinned to the fixture on the CPU and stands in for the reference
at the schedules the fixture does not hold.  Every device row carries stale, valid-looking records and events past its count."""
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
import streaming_model as SM  # noqa: E402
import make_golden_events as G  # noqa: E402
import make_golden_random_access as GR  # noqa: E402
import make_golden_streaming as GS  # noqa: E402
from pool_labels import labels_of as _labels_of  # noqa: E402

gpu = pytest.mark.gpu

LOAD_EVENTS_LAUNCHES, INDEX_LAUNCHES, NEXT_LAUNCHES, FRAMES_LAUNCHES = 2, 2, 1, 5     # the class docstring
H, W = 240, 304                                  # the Gen1 sensor
LABEL_KW = dict(max_frames=128, max_windows=512, max_labels_per_frame=16)
MX = LABEL_KW["max_labels_per_frame"]


@functools.lru_cache(maxsize=None)
def _fx():
    with np.load(os.path.join(GOLDEN, "streaming.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _rows(pool, split, ds):
    return tuple(GS.model_rows(pool, split, ds))


def _model(pool, split, ds, L, g, **kw):
    return SM.Pool(_rows(pool, split, ds), L, g, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_batch(got, want, where=""):
    for g, w, name in zip(got, want, SM.NAMES):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.shape == w.shape and g.dtype == w.dtype, (name, where)
        assert np.array_equal(_bits(g), _bits(w)), (name, where)


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_streaming_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    from sast_amd import sampling as SP
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_stream_")]
    assert sorted(names) == ["sast_stream_index", "sast_stream_next"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert [f for f, _t in _lib.SastStreamArgs._fields_] == [
        "seq_row", "seq_start", "seq_stop", "seq_samples", "row_first_seq", "row_count", "n_seq", "status", "order", "order_len", "cursor",
        "sequence_length", "guarantee_labels", "max_sequences", "order_capacity"]
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for (bit, name, _msg), model_bit in zip(SP.STREAM_FLAGS, (SM.TRUNCATED, SM.SCHEDULE_INDEX)):
        assert f"SAST_STREAM_{name.upper()} = {bit}," in header or f"SAST_STREAM_{name.upper()} = {bit} " in header, name
        assert bit == model_bit
    assert SP.StreamingBatch._fields == SM.NAMES
    import sast_amd.build as B
    assert "k_stream.hip" in B.SOURCES and B.SOURCE_FLAGS["k_stream.hip"] == ["-ffp-contract=off"]


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


def _stream_args(**over):
    from sast_amd import _lib
    q = _lib.SastStreamArgs()
    for f, _t in _lib.SastStreamArgs._fields_[:11]:
        setattr(q, f, 0x1000)
    q.sequence_length, q.guarantee_labels, q.max_sequences, q.order_capacity = 5, 1, 64, 64
    for k, v in over.items():
        setattr(q, k, v)
    return q


def test_streaming_entry_points_reject_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib = _lib.lib()
    EINVAL, p = -22, 0x1000
    before = lib.sast_launch_count()
    used = ("ends_us", "n_windows", "n_frames", "frame_2_window", "window_2_frame", "labels", "frame_start", "frame_count")
    bad_a = [None] + [_label_args(**{f: None}) for f in used]
    bad_a += [_label_args(**kw) for kw in (dict(S=0), dict(S=65536), dict(capacity=0), dict(capacity=2 ** 27), dict(max_frames=0),
                                           dict(max_windows=0), dict(max_labels_per_frame=0), dict(max_windows=2 ** 30))]
    table = ("seq_row", "seq_start", "seq_stop", "seq_samples", "row_first_seq", "row_count", "n_seq", "status")
    bad_q = [None] + [_stream_args(**{f: None}) for f in table]
    bad_q += [_stream_args(**kw) for kw in (dict(sequence_length=0), dict(sequence_length=65536), dict(max_sequences=0),
                                            dict(guarantee_labels=2), dict(guarantee_labels=-1))]
    bad_next = [_stream_args(**kw) for kw in (dict(order=None), dict(order_len=None), dict(cursor=None), dict(order_capacity=0),
                                              dict(order_capacity=2 ** 30))]
    ok_a, ok_q = _label_args(), _stream_args()

    def ref(v):
        return None if v is None else C.byref(v)

    for a in bad_a:
        assert lib.sast_stream_index(ref(a), ref(ok_q), None) == EINVAL
        assert lib.sast_stream_next(ref(a), ref(ok_q), 4, *([p] * 12), None) == EINVAL
    for q in bad_q:
        assert lib.sast_stream_index(ref(ok_a), ref(q), None) == EINVAL
        assert lib.sast_stream_next(ref(ok_a), ref(q), 4, *([p] * 12), None) == EINVAL
    for q in bad_next:
        assert lib.sast_stream_next(ref(ok_a), ref(q), 4, *([p] * 12), None) == EINVAL
    for k in range(12):
        ptrs = [p] * 12
        ptrs[k] = None
        assert lib.sast_stream_next(ref(ok_a), ref(ok_q), 4, *ptrs, None) == EINVAL
    for B in (0, -1, 65536, 2 ** 26):
        assert lib.sast_stream_next(ref(ok_a), ref(ok_q), B, *([p] * 12), None) == EINVAL
    assert lib.sast_stream_next(ref(ok_a), ref(_stream_args(sequence_length=65535)), 4096, *([p] * 12), None) == EINVAL     # L * B * M
    assert lib.sast_launch_count() == before


def _cpu_labels(R=3, **kw):
    from sast_amd.labels import LabelStreams
    return LabelStreams(R, 100, max_frames=8, max_windows=32, max_labels_per_frame=4, **kw)


def test_streaming_pool_constructor_validation():
    from sast_amd.labels import LabelStreams
    from sast_amd.sampling import RandomAccessPool, StreamingPool
    ls = _cpu_labels()
    pool = StreamingPool(ls, H, W, sequence_length=5)
    assert pool.get_shape() == (20, H, W) and pool.num_rows == 3 and pool.frame_dtype == torch.uint8
    assert pool.guarantee_labels and pool.max_sequences == 3 * 8 == pool.order_capacity
    val = StreamingPool(ls, H, W, sequence_length=5, guarantee_labels=False, order_capacity=7)
    assert val.max_sequences == 3 and val.order_capacity == 7
    md = StreamingPool(ls, H, W, sequence_length=5, representation="mixed_density", count_cutoff=None)
    assert md.get_shape() == (10, H, W) and md.frame_dtype == torch.int8
    ds = StreamingPool(LabelStreams(2, 100, downsample_by_2=True), H, W, sequence_length=3, downsample_by_2=True)
    assert ds.get_shape() == (20, H // 2, W // 2)
    rp = RandomAccessPool(ls, H, W, sequence_length=5)
    shared = StreamingPool(ls, H, W, sequence_length=5, events=rp)
    assert shared._events is rp and StreamingPool(ls, H, W, sequence_length=2, events=shared)._events is rp
    for bad in (None, 3):
        with pytest.raises(TypeError):
            StreamingPool(bad, H, W, sequence_length=5)
    with pytest.raises(TypeError):
        StreamingPool(ls, H, W, sequence_length=5, events=ls)
    other = RandomAccessPool(_cpu_labels(2), H, W, sequence_length=5)
    for bad in (dict(sequence_length=0), dict(sequence_length=65536), dict(sequence_length=2.0), dict(max_sequences=0),
                dict(max_sequences=2.5), dict(order_capacity=0), dict(order_capacity=2 ** 31), dict(duration_us=None),
                dict(duration_us=-1), dict(downsample_by_2=True), dict(representation="voxel"), dict(bins=0), dict(events=other)):
        with pytest.raises(ValueError):
            StreamingPool(ls, H, W, **{**dict(sequence_length=5), **bad})
    assert pool.errors() == () and pool.frame_errors() == (0, 0)
    assert (StreamingPool.LOAD_EVENTS_LAUNCHES, StreamingPool.INDEX_LAUNCHES, StreamingPool.NEXT_LAUNCHES,
            StreamingPool.FRAMES_LAUNCHES) == (LOAD_EVENTS_LAUNCHES, INDEX_LAUNCHES, NEXT_LAUNCHES, FRAMES_LAUNCHES)


def _host_pool(m, **kw):
    """a StreamingPool carrying the host mirrors index() would have fetched, for the host-only methods"""
    from sast_amd.sampling import StreamingPool
    sp = StreamingPool(_cpu_labels(len(m.rows)), H, W, sequence_length=m.L, guarantee_labels=m.guarantee, **kw)
    sp._host = (m.sequences, [r.window_2_frame >= 0 for r in m.rows])
    return sp


def test_streaming_pool_call_validation_and_cpu_tensors_raise():
    from sast_amd.sampling import RandomAccessPool, StreamingBatch, StreamingPool
    ls = _cpu_labels()
    pool = StreamingPool(ls, H, W, sequence_length=3)
    col, cnt = torch.zeros(3, 50, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError):
        pool.load_events(col.to(torch.float32), col, col, col, cnt)
    for x, y, p, t, c, rs in ((col[:2], col[:2], col[:2], col[:2], cnt, None), (col, col, col, col[:, :40], cnt, None),
                              (col, col, col, col, cnt.to(torch.int32), None), (col, col, col, col, cnt, torch.zeros(3, dtype=torch.int32)),
                              (col[:, :0], col[:, :0], col[:, :0], col[:, :0], cnt, None)):
        with pytest.raises(ValueError):
            pool.load_events(x, y, p, t, c, rs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pool.load_events(col, col, col, col, cnt)
    shared = StreamingPool(ls, H, W, sequence_length=3, events=RandomAccessPool(ls, H, W, sequence_length=3))
    with pytest.raises(RuntimeError, match="events="):
        shared.load_events(col, col, col, col, cnt)
    want = pool._want(4)
    cpu_batch = StreamingBatch(*(torch.zeros(sh, dtype=dt) for sh, dt in want))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pool.next(out=cpu_batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pool.frames(cpu_batch)
    with pytest.raises(RuntimeError, match="labels.load"):
        pool.index()
    with pytest.raises(RuntimeError, match="index"):
        pool.next()
    for call in (lambda: pool.concat_orders(2), lambda: pool.sharded_orders(2), lambda: pool.set_schedule([[0]]), pool.plan,
                 lambda: pool.steps("shortest")):
        with pytest.raises(RuntimeError, match="index"):
            call()
    # the schedule is validated on the host, before anything is written
    m = _model("gen1", "train", False, 3, True)
    sp = _host_pool(m, order_capacity=4)
    for bad in ([], [[0, m.n_seq]], [[-1]], [[0, 1, 2, 3, 4]], [[0]] * 65536):
        with pytest.raises(ValueError):
            sp.set_schedule(bad)
    with pytest.raises(RuntimeError, match="set_schedule"):
        sp.plan()
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            sp.concat_orders(bad)
        with pytest.raises(ValueError):
            sp.sharded_orders(bad)
    sp._orders = [[0]]
    with pytest.raises(ValueError):
        sp.steps("all")


@pytest.mark.parametrize("pool,split,ds,L,g", GS.case_keys())
def test_model_equals_the_reference_fixture(pool, split, ds, L, g):
    fx, key = _fx(), GS.key_of(pool, split, ds, L, g)
    m = _model(pool, split, ds, L, g)
    assert np.array_equal(m.sequences, fx[f"{key}/sequences"]) and m.sequences.dtype == fx[f"{key}/sequences"].dtype and m.status == 0
    assert m.row_first_seq == [int((m.sequences[:, 0] < r).sum()) for r in range(len(m.rows) + 1)]
    # every sample of every sequence, through the cursor: one batch row that walks all sequences in order
    m.set_schedule([list(range(m.n_seq))])
    n = m.steps("longest")
    assert n == m.steps("shortest") == int(m.sequences[:, 3].sum()) == len(fx[f"{key}/sample_seq"])
    K, first, seq = m.plan()
    assert np.array_equal(seq[:, 0], fx[f"{key}/sample_seq"]) and np.array_equal(first[:, 0], fx[f"{key}/is_first"] != 0)
    step_counts, windows, got_rows = fx[f"{key}/step_counts"], fx[f"{key}/windows"], []
    assert np.array_equal(K, (step_counts >= 0).sum(1))
    for i in range(n):
        rows, step_rows, sq, sample, is_first, exhausted, widx, _ends, labels, counts, labelled, padded = m.next(MX)
        assert sq[0] == fx[f"{key}/sample_seq"][i] and rows[0] == m.sequences[sq[0], 0] and is_first[0] == fx[f"{key}/is_first"][i]
        assert exhausted[0] == 0 and is_first[0] == (sample[0] == 0)
        assert np.array_equal(padded[:, 0], fx[f"{key}/is_padded"][i]) and np.array_equal(widx[:, 0], windows[i])
        assert np.array_equal(step_rows[:, 0], np.where(padded[:, 0] != 0, -1, rows[0]))
        assert np.array_equal(labelled[:, 0], step_counts[i] >= 0) and np.array_equal(counts[:, 0], np.maximum(step_counts[i], 0))
        got_rows += [labels[k, 0, :counts[k, 0]] for k in range(L)]
        assert not labels[padded[:, 0] != 0].any()
    got = np.concatenate(got_rows + [np.zeros((0, 7), np.float32)])
    assert np.array_equal(_bits(got), _bits(fx[GS.labels_key(pool, split, ds)]))
    # the schedule is used up: get_fully_padded_sample
    out = m.next(MX)
    assert out[0][0] == -1 and out[4][0] == 0 and out[5][0] == 1 and out[11].all() and (out[6] == -1).all() and not out[8].any()
    assert m.cursor == [[m.n_seq, 0]] and m.status == 0
    # ShardedStreamingDataPipe's deals
    for (B, Wk, w), want in GS.sharded_cases(fx[f"{key}/sharded"]).items():
        if want is None:
            with pytest.raises(ValueError):
                m.sharded_orders(B, Wk, w)
        else:
            assert m.sharded_orders(B, Wk, w) == want, (B, Wk, w)


def test_fixture_inputs_meet_the_conditions():
    GS.check_inputs()
    fx = _fx()
    assert fx["gen1/train/full/L3/guaranteed/sequences"][:, 0].tolist() == [0, 0, 0, 1, 2, 2, 2, 2, 2]
    assert fx["gen4/train/full/L3/guaranteed/sequences"][:, 0].tolist() == [0] * 4
    assert len(fx["gen1/val/full/L11/unsplit/sequences"]) == 3
    pad = fx["gen1/train/full/L3/guaranteed/is_padded"]
    assert pad[:, 0].sum() == 0 and 0 < pad[:, -1].sum() < len(pad)
    cases = [GS.sharded_cases(fx[f"{GS.key_of(p, 'val', False, 11, False)}/sharded"]) for p in ("gen1", "gen4")]
    assert cases[0][(2, 2, 0)] is None and cases[0][(2, 2, 1)] is not None and cases[1][(2, 1, 0)] is None      # both asserts of the reference
    deal = GS.sharded_cases(fx["gen1/train/full/L3/guaranteed/sharded"])[(3, 1, 0)]
    assert sorted(s for row in deal for s in row) == list(range(9)) and [len(r) for r in deal] == [3, 3, 3]


@pytest.mark.skipif(not GS.reference_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_streaming_fixture():
    new, old = GS.generate(), _fx()
    assert sorted(new) == sorted(old)
    for k in new:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert np.ascontiguousarray(new[k]).tobytes() == np.ascontiguousarray(old[k]).tobytes(), k


def test_concat_orders_are_torch_randperm_in_batch_row_order():
    m = _model("gen1", "train", False, 3, True)
    sp = _host_pool(m)
    torch.manual_seed(1234)
    got = sp.concat_orders(3)
    torch.manual_seed(1234)
    want = [torch.randperm(m.n_seq).tolist() for _ in range(3)]
    assert got == want and all(sorted(o) == list(range(m.n_seq)) for o in got) and got[0] != got[1]


@pytest.mark.parametrize("pool,split,L,g", [("gen1", "train", 3, True), ("gen1", "val", 11, False), ("gen4", "val", 3, True),
                                            ("gen4", "val", 5, False), ("gen1", "train", 1, True)])
def test_sharded_orders_equal_the_reference_fixture(pool, split, L, g):
    fx, m = _fx(), _model(pool, split, False, L, g)
    sp = _host_pool(m)
    for (B, Wk, w), want in GS.sharded_cases(fx[f"{GS.key_of(pool, split, False, L, g)}/sharded"]).items():
        if want is None:
            with pytest.raises(ValueError):
                sp.sharded_orders(B, Wk, w)
        else:
            assert sp.sharded_orders(B, Wk, w) == want, (B, Wk, w)
    with pytest.raises(ValueError):
        sp.sharded_orders(1, 2, 2)                          # total_num_workers > global_worker_id


def _schedules(m, B):
    """batch rows of different lengths; with B = 3, rows 0 and 1 start on the same sequence"""
    n = m.n_seq
    return [[n - 1, 0]] if B == 1 else [[1 % n, n - 1], [1 % n], [0, (n - 1) // 2, n - 1]]


@pytest.mark.parametrize("L,g", [(1, True), (3, True), (11, True), (3, False)])
def test_plan_and_steps_equal_the_model(L, g):
    m = _model("gen1", "train", False, L, g)
    sp = _host_pool(m)
    for B in (1, 3):
        orders = _schedules(m, B)
        m.set_schedule(orders)
        sp._orders = orders                                 # what set_schedule keeps once the copies to the device are made
        K, first, seq = m.plan()
        got = sp.plan()
        assert np.array_equal(got.K, K) and np.array_equal(got.is_first, first) and np.array_equal(got.seq, seq)
        assert got.K.dtype == np.int64 and got.is_first.dtype == bool and got.seq.dtype == np.int32
        assert sp.steps("shortest") == m.steps("shortest") and sp.steps("longest") == m.steps("longest") == len(K)
        assert B == 1 or sp.steps("shortest") < sp.steps("longest")
        assert K.sum() > 0 and (seq[-1] == -1).sum() == B - 1


# ---------------------------------------------------------------------------------------------------------------------------- GPU

@functools.lru_cache(maxsize=None)
def _words(names):
    return tuple(M.pack(GR.pool_records(n)) if n != "unsorted" else M.pack(GR.pool_records("gen1"))[::-1].copy() for n in names)


def _labels(names, dataset, split, ds):
    """a loaded LabelStreams of the named recordings, stale records behind every row's count"""
    from sast_amd.labels import LabelStreams
    rows = _words(tuple(names))
    cap = max(len(w) for w in rows) + 5
    rec = np.stack([np.resize(rows[0][-40:], (cap, 10)) for _ in rows])
    for s, w in enumerate(rows):
        rec[s, :len(w)] = w
    ls = LabelStreams(len(rows), cap, dataset=dataset, split=split, downsample_by_2=ds, **LABEL_KW)
    ls.load(torch.from_numpy(rec).cuda(), torch.tensor([len(w) for w in rows], dtype=torch.int64, device="cuda"))
    return ls


def _pool_labels(pool, split, ds):
    return _labels(GR.POOLS[pool], GR.dataset_of(pool), split, ds)


N_EV = (4000, 3000, 3500)


@functools.lru_cache(maxsize=None)
def _event_columns(R, salt=0):
    """R rows of hashed events over the time the label schedules span, one event in 16 out of order, different counts, stale events
    behind every count; the first corrected timestamps of rows 0 and 1 are 0 -> (x, y, p, t) int64 [R, cap] numpy, counts"""
    cap = max(N_EV) + 3
    cols = [np.zeros((R, cap), np.int64) for _ in range(4)]
    for r in range(R):
        ev = G.stream(seed=170 + 10 * salt + r, n=cap, height=H, width=W, t_start=0, t_step=4000, jitter=1500)
        for c, e in zip(cols, ev):
            c[r] = e
        cols[3][r, N_EV[r]:] = cols[3][r, N_EV[r] // 2]          # stale: times in the middle of the row
    cols[3][:2, :6] = 0
    return tuple(cols), np.asarray(N_EV[:R], np.int64)


def _cuda(cols, counts):
    return [torch.from_numpy(c).cuda() for c in cols], torch.from_numpy(counts).cuda()


def _pool(ls, L, g=True, **kw):
    from sast_amd.sampling import StreamingPool
    return StreamingPool(ls, ls.height, ls.width, sequence_length=L, guarantee_labels=g, **kw)


@gpu
@pytest.mark.parametrize("pool,split,ds", [(p, s, d) for p in GS.POOLS for s in GS.SPLITS for d in (False, True)])
def test_index_equals_the_model_and_the_reference_fixture(pool, split, ds):
    fx = _fx()
    ls = _pool_labels(pool, split, ds)
    R = ls.num_streams
    assert ls.errors() == [()] * R
    for L in GS.LENGTHS:
        for g in (True, False):
            key, m = GS.key_of(pool, split, ds, L, g), _model(pool, split, ds, L, g)
            sp = _pool(ls, L, g, downsample_by_2=ds)
            n, sequences = sp.index(check=True)
            assert n == m.n_seq and sequences.dtype == np.int32 and np.array_equal(sequences, fx[f"{key}/sequences"])
            assert np.array_equal(sequences, m.sequences) and sp.row_first_seq.tolist() == m.row_first_seq and int(sp.n_seq) == n
            table = torch.stack([sp.seq_row, sp.seq_start, sp.seq_stop, sp.seq_samples], 1).cpu().numpy()
            assert np.array_equal(table[:n], sequences) and sp.errors() == ()
            # a second call replays on the same state
            again = sp.index()
            assert again[0] == n and np.array_equal(again[1], sequences)


@gpu
@pytest.mark.parametrize("g", [True, False])
def test_index_skips_a_flagged_row_and_flags_a_table_that_is_too_small(g):
    names = ("gen1", "unsorted", "gen1_b")
    ls = _labels(names, "gen1", "train", False)
    assert ls.errors() == [(), ("unsorted",), ()] and ls.n_frames.tolist()[1] == 0
    rows = [M.load_row(w, "gen1", "train") for w in _words(names)]
    assert rows[1].status == M.UNSORTED and rows[1].n_frames == 0
    L = 3
    m = SM.Pool(rows, L, g)
    sp = _pool(ls, L, g)
    n, sequences = sp.index(check=True)
    assert n == m.n_seq == (8 if g else 2) and np.array_equal(sequences, m.sequences) and 1 not in sequences[:, 0]
    assert sp.row_first_seq.tolist() == m.row_first_seq and m.row_first_seq[1] == m.row_first_seq[2]
    # one sequence too many for the table: the first ones are kept, and it is said
    small, ms = _pool(ls, L, g, max_sequences=n - 1), SM.Pool(rows, L, g, max_sequences=n - 1)
    n2, seq2 = small.index()
    assert n2 == n - 1 == ms.n_seq and np.array_equal(seq2, sequences[:n - 1]) and np.array_equal(seq2, ms.sequences)
    assert small.row_first_seq.tolist() == ms.row_first_seq and small.errors() == ("truncated",) and ms.status == SM.TRUNCATED
    with pytest.raises(ValueError, match="truncated"):
        small.index(check=True)
    exact = _pool(ls, L, g, max_sequences=n)
    assert exact.index(check=True)[0] == n and exact.errors() == ()


@gpu
@pytest.mark.parametrize("L", [1, 3, 11])
@pytest.mark.parametrize("B", [1, 3])
def test_next_over_a_whole_schedule_equals_the_model(L, B):
    """rows of different lengths (exhausted rows appear), two rows on one sequence at once, full and padded tails"""
    ls = _pool_labels("gen1", "train", False)
    R = ls.num_streams
    m = _model("gen1", "train", False, L, True)
    sp = _pool(ls, L)
    assert sp.index(check=True)[0] == m.n_seq
    orders = _schedules(m, B)
    sp.set_schedule(orders)
    m.set_schedule(orders)
    plan, (K, first, seq) = sp.plan(), m.plan()
    assert np.array_equal(plan.K, K) and np.array_equal(plan.is_first, first) and np.array_equal(plan.seq, seq)
    n = sp.steps("longest")
    assert sp.order.shape == (B, sp.order_capacity) and sp.order_len.tolist() == [len(o) for o in orders] and not bool(sp.cursor.any())
    seen_pad = seen_done = 0
    for i in range(n + 1):                                 # one more step: every row is exhausted
        out = sp.next()
        want = m.next(MX)
        _same_batch(out, want, i)
        assert sp.cursor.tolist() == m.cursor
        if i < n:
            assert int(out.labelled.sum()) == K[i] and out.seq.tolist() == seq[i].tolist()
            assert out.is_first.tolist() == first[i].astype(int).tolist()
        seen_pad += int(want[11][:, want[0] >= 0].sum())
        seen_done += int(want[5].sum())
        for b, ref in enumerate(_labels_of(ls, out, R)):   # a real step is LabelStreams.labels at (rows, window_idx)
            if ref is None:
                continue
            real = out.is_padded[:, b] == 0
            for got, exp in zip((out.labels[:, b], out.counts[:, b], out.ends_us[:, b], out.labelled[:, b]), ref):
                assert torch.equal(got[real], exp[real])
    assert (L == 1 or seen_pad > 0) and seen_done >= B and out.exhausted.tolist() == [1] * B and out.rows.tolist() == [-1] * B
    if B == 3:
        assert orders[0][0] == orders[1][0]                 # one sequence in two rows at once
    assert sp.errors() == () and ls.errors() == [()] * R
    # `out` is written in place, and a new schedule starts from zeroed cursors
    sp.set_schedule(orders)
    m.set_schedule(orders)
    into = tuple(torch.full_like(t, 7) for t in out)
    res = sp.next(out=into)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(res, into))
    _same_batch(res, m.next(MX))


@gpu
def test_a_schedule_entry_out_of_range_is_flagged_padded_and_skipped():
    L, B = 3, 3
    ls = _pool_labels("gen1", "val", False)
    m = _model("gen1", "val", False, L, True)
    sp, clean = _pool(ls, L), _pool(ls, L)
    n, _ = sp.index()
    clean.index()
    orders = [[1, 2], [0, 3], [4]]
    sp.set_schedule(orders)
    clean.set_schedule([orders[0], orders[2]])
    sp.order[1, 0] = n                                      # written past set_schedule, which would have refused it
    sp.order[1, 1] = -1
    bad = [orders[0], [n, -1], orders[2]]
    m.set_schedule(bad)
    for i in range(4):
        out, want, alone = sp.next(), m.next(MX), clean.next()
        _same_batch(out, want, i)
        assert sp.cursor.tolist() == m.cursor
        if i < 2:
            assert out.rows[1] == -1 and out.exhausted[1] == 0 and out.is_first[1] == 0 and bool(out.is_padded[:, 1].all())
            assert int(out.counts[:, 1].sum()) == 0 and not bool(out.labels[:, 1].any()) and out.window_idx[:, 1].tolist() == [-1] * L
        else:
            assert out.exhausted[1] == 1
        for name, t_all, t_good in zip(SM.NAMES, out, alone):               # the other rows are untouched
            sel = t_all[[0, 2]] if t_all.dim() == 1 else t_all[:, [0, 2]]
            assert torch.equal(sel, t_good), name
    assert sp.errors() == ("schedule_index",) and m.status == SM.SCHEDULE_INDEX and clean.errors() == ()
    sp.index()
    assert sp.errors() == ()


def _frame_setup(L, representation="stacked_histogram", g=True):
    ls = _pool_labels("gen1", "train", False)
    kw = dict(bins=4, count_cutoff=5, duration_us=50000, representation=representation)
    sp = _pool(ls, L, g, **kw)
    sp.index(check=True)
    cols, counts = _cuda(*_event_columns(3))
    return ls, sp, kw, cols, counts


@gpu
@pytest.mark.parametrize("representation", ["stacked_histogram", "mixed_density"])
def test_frames_equal_event_streams_on_real_steps_and_are_zero_on_padded_ones(representation):
    from sast_amd.events import EventStreams
    L, R, B = 3, 3, 3
    ls, sp, kw, cols, counts = _frame_setup(L, representation)
    sp.load_events(*cols, counts)
    m = _model("gen1", "train", False, L, True)
    single = m.row_first_seq[1]
    assert m.sequences[single].tolist()[2:] == [2, 1] and m.sequences[0, 1] == 0            # a padded tail; a sample that starts at window 0
    sp.set_schedule([[0], [m.row_first_seq[2]], [single]])
    es = EventStreams(R, H, W, **kw)
    ones = torch.ones(R, dtype=torch.uint8, device="cuda")
    for step in range(2):
        out = sp.next()
        frames = sp.frames(out)
        assert frames.shape == (L, B) + sp.get_shape() and frames.dtype == sp.frame_dtype and sp.frame_errors() == (0, 0)
        rows, padded = out.rows.tolist(), out.is_padded.cpu().numpy() != 0
        assert rows == ([0, 2, 1] if step == 0 else [0, 2, -1])
        for b, r in enumerate(rows):
            assert not bool(frames[:, b][torch.from_numpy(padded[:, b]).cuda()].any())         # padded steps and exhausted rows
            if r < 0:
                assert padded[:, b].all()
                continue
            per_row = torch.zeros(L, R, dtype=torch.int64, device="cuda")
            per_row[:, r] = out.ends_us[:, b].clamp(min=0)
            want = es(*cols, counts, per_row, reset=ones)
            for k in range(L):
                if not padded[k, b]:
                    assert torch.equal(frames[k, b], want[k, r]), (step, b, k)
                    assert int(want[k, r].count_nonzero()) > 0
        if step == 0:
            assert padded[:, 2].tolist() == [False, False, True] and out.ends_us[2, 2] == -1 and out.step_rows[:, 2].tolist() == [1, 1, -1]
        into = torch.full_like(frames, 9)
        assert sp.frames(out, out_frames=into).data_ptr() == into.data_ptr() and torch.equal(into, frames)
    assert int(sp.t[:2, :6].abs().sum()) == 0                 # the first corrected timestamps of rows 0 and 1 (the padded sample's) are 0
    assert es.errors() == (0, 0) and sp.errors() == ()


@gpu
def test_a_pool_that_shares_another_pools_events_gives_the_same_frames():
    from sast_amd.sampling import RandomAccessPool
    L = 3
    ls, own, kw, cols, counts = _frame_setup(L)
    own.load_events(*cols, counts)
    rp = RandomAccessPool(ls, H, W, sequence_length=L, **kw)
    rp.load_events(*cols, counts)
    n_items, _ = rp.index()
    items = torch.tensor([0, n_items - 1, 5], dtype=torch.int64, device="cuda")
    batch = rp.batch(items)
    before = rp.frames(batch).clone()
    shared = _pool(ls, L, events=rp, **kw)
    second = _pool(ls, L, events=shared, **kw)
    for sp in (shared, second):
        sp.index()
    m = _model("gen1", "train", False, L, True)
    orders = [[m.row_first_seq[1], 2], [m.row_first_seq[2]]]
    for sp in (own, shared, second):
        sp.set_schedule(orders)
    for _ in range(2):
        outs = [sp.next() for sp in (own, shared, second)]
        fr = [sp.frames(o) for sp, o in zip((own, shared, second), outs)]
        assert torch.equal(fr[0], fr[1]) and torch.equal(fr[0], fr[2]) and int(fr[0].count_nonzero()) > 0
        assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert shared.t is None and torch.equal(rp.t, own.t)
    assert torch.equal(rp.frames(batch), before) and rp.frame_errors() == (0, 0) == shared.frame_errors()
    with pytest.raises(RuntimeError, match="events="):
        shared.load_events(*cols, counts)


@gpu
def test_streaming_launch_counts_are_the_documented_ones():
    from sast_amd import _lib
    lib = _lib.lib()
    ls = _pool_labels("gen1", "train", False)
    cols, counts = _cuda(*_event_columns(3))

    def launches(fn):
        before = lib.sast_launch_count()
        res = fn()
        return lib.sast_launch_count() - before, res

    for L in (3, 5):
        for representation in ("stacked_histogram", "mixed_density"):
            for g in (True, False):
                sp = _pool(ls, L, g, bins=4, representation=representation)
                for reset in (None, torch.tensor([0, 1, 1], dtype=torch.uint8, device="cuda")):
                    assert launches(lambda: sp.load_events(*cols, counts, reset=reset))[0] == LOAD_EVENTS_LAUNCHES
                k, (n, _seqs) = launches(sp.index)
                assert k == INDEX_LAUNCHES
                for B in (1, 4):
                    assert launches(lambda: sp.set_schedule([[b % n] for b in range(B)]))[0] == 0
                    k, out = launches(sp.next)
                    assert k == NEXT_LAUNCHES, (L, B)
                    assert launches(lambda: sp.frames(out))[0] == FRAMES_LAUNCHES, (L, B)


@gpu
def test_next_frames_and_augmentation_in_one_graph_advance_under_replay():
    """next + frames + SpatialAugmentor(yolox=True) captured once after a warm-up; then a new schedule and n replays == n eager next
    calls on a second pool, step by step: the cursor in device memory moves under replay"""
    import make_golden_augment as GA
    from sast_amd import augment as A
    L, B, n = 3, 3, 6
    ls, sp, kw, cols, counts = _frame_setup(L)
    sp.load_events(*cols, counts)
    eager_pool = _pool(ls, L, events=sp, **kw)
    eager_pool.index()
    m = _model("gen1", "train", False, L, True)
    aug = A.SpatialAugmentor((H, W), GA.SHIPPED["random"], B)
    aug.set_state([A.AugmentationState(apply_h_flip=True), A.AugmentationState(zoom_out=A.ZoomOutState(True, 20, 10, 1.25)),
                   A.AugmentationState()])

    def call(pool):
        out = pool.next()
        frames = pool.frames(out)
        return aug(frames, out.labels, out.counts, yolox=True) + tuple(out)

    warm = [[0], [1], [2]]
    orders = [[m.row_first_seq[1], 1], [m.row_first_seq[2], 0], [1]]      # a padded tail at once, sequence changes, an exhausted row
    sp.set_schedule(warm)
    eager_pool.set_schedule(orders)
    eager = [[t.clone() for t in call(eager_pool)] for _ in range(n)]
    assert eager_pool.steps("shortest") < n <= eager_pool.steps("longest")
    assert int(eager[0][0].count_nonzero()) > 0 and not torch.equal(eager[0][0], eager[1][0]) and int(eager[n - 1][8].sum()) == 2
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(sp)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = call(sp)
    sp.set_schedule(orders)
    for i in range(n):
        g.replay()
        torch.cuda.synchronize()
        for got, exp in zip(captured, eager[i]):
            assert torch.equal(got, exp), i
    assert sp.cursor.tolist() == eager_pool.cursor.tolist() and sp.cursor[2].tolist() == [1, 0]
    assert sp.errors() == () and sp.frame_errors() == (0, 0) and ls.errors() == [(), (), ()]
