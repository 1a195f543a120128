"""The merged batch of `sampling: 'mixed'` (sast_amd.sampling.MixedPool, RandomAccessPool.latest, sast_amd.augment.JoinedAugmentor and
the entry points sast_mixed_next of csrc/k_mixed.hip and sast_mixed_latest of csrc/k_sampler.hip).

The yardstick of every equality is the concatenation, along the batch axis and stream columns first, of what the existing entry points
give on identical state: a second `StreamingPool(events=...)` with the same schedule, and `RandomAccessPool.batch` / `.frames` on the
same items.  Both are pinned to reference fixtures by tests/test_streaming_pool.py and tests/test_random_access.py, so equality with
their concatenation pins the merged form.  Integers are compared as they are, fp32 label rows by their bits, frames byte for byte."""
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
import make_golden_augment as GA  # noqa: E402
import make_golden_events as G  # noqa: E402
import make_golden_random_access as GR  # noqa: E402

gpu = pytest.mark.gpu

NEXT_LAUNCHES, FRAMES_LAUNCHES, JOINED_LAUNCHES, LATEST_LAUNCHES = 1, 5, 2, 1          # the class docstrings
H, W = 240, 304                                  # the Gen1 sensor
LABEL_KW = dict(max_frames=128, max_windows=512, max_labels_per_frame=16)
MX = LABEL_KW["max_labels_per_frame"]
FRAME_KW = dict(bins=4, count_cutoff=5, duration_us=50000)
N_EV = (4000, 3000, 3500)
FIELDS = ("rows", "step_rows", "seq", "sample", "is_first", "exhausted", "window_idx", "ends_us", "labels", "counts", "labelled", "is_padded",
          "latest", "latest_count")


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_mixed_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    from sast_amd import sampling as SP
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_mixed_")]
    assert sorted(names) == ["sast_mixed_latest", "sast_mixed_next"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert len(_lib._SIGNATURES["sast_mixed_next"][1]) == 6 + len(FIELDS) + 1 and len(_lib._SIGNATURES["sast_mixed_latest"][1]) == 7
    assert SP.MixedBatch._fields == FIELDS
    assert SP.MixedBatch._fields[:12] == SP.StreamingBatch._fields and SP.MixedBatch._fields[12:] == SP.RandomAccessBatch._fields[-2:]
    assert SP.RandomAccessLatest._fields == ("latest", "latest_count")
    assert (SP.MixedPool.NEXT_LAUNCHES, SP.MixedPool.FRAMES_LAUNCHES, SP.RandomAccessPool.LATEST_LAUNCHES) == (
        NEXT_LAUNCHES, FRAMES_LAUNCHES, LATEST_LAUNCHES)
    import sast_amd.build as B
    assert "k_mixed.hip" in B.SOURCES and B.SOURCE_FLAGS["k_mixed.hip"] == ["-ffp-contract=off"] and "sampler_rows.cuh" in B.HEADERS


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


def _rnd_args(**over):
    from sast_amd import _lib
    q = _lib.SastRndArgs()
    for f, _t in _lib.SastRndArgs._fields_[:7]:
        setattr(q, f, 0x1000)
    q.sequence_length, q.only_load_end_labels, q.max_classes, q.weighted = 5, 0, 16, 0
    for k, v in over.items():
        setattr(q, k, v)
    return q


def test_mixed_entry_points_reject_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib = _lib.lib()
    EINVAL, p, n_out = -22, 0x1000, len(FIELDS)
    before = lib.sast_launch_count()

    def ref(v):
        return None if v is None else C.byref(v)

    def nxt(a, qs, qr, Bs=2, items=p, Br=2, ptrs=None):
        return lib.sast_mixed_next(ref(a), ref(qs), ref(qr), Bs, items, Br, *(ptrs or [p] * n_out), None)

    def latest(a, qr, items=p, B=2, out=(p, p)):
        return lib.sast_mixed_latest(ref(a), ref(qr), items, B, *out, None)

    used = ("ends_us", "n_windows", "n_frames", "frame_2_window", "window_2_frame", "labels", "frame_start", "frame_count")
    bad_a = [None] + [_label_args(**{f: None}) for f in used]
    bad_a += [_label_args(**kw) for kw in (dict(S=0), dict(S=65536), dict(capacity=0), dict(capacity=2 ** 27), dict(max_frames=0),
                                           dict(max_windows=0), dict(max_labels_per_frame=0), dict(max_windows=2 ** 30))]
    table = ("seq_row", "seq_start", "seq_stop", "seq_samples", "row_first_seq", "row_count", "n_seq", "status", "order", "order_len", "cursor")
    bad_qs = [None] + [_stream_args(**{f: None}) for f in table]
    bad_qs += [_stream_args(**kw) for kw in (dict(sequence_length=0), dict(sequence_length=65536), dict(max_sequences=0), dict(guarantee_labels=2),
                                             dict(order_capacity=0), dict(order_capacity=2 ** 30), dict(sequence_length=4))]     # 4: not the random pool's
    bad_qr = [None] + [_rnd_args(**{f: None}) for f in ("start_idx_offset", "length", "cum", "class_total", "status", "ticket")]
    bad_qr += [_rnd_args(**kw) for kw in (dict(sequence_length=0), dict(sequence_length=65536), dict(max_classes=0), dict(max_classes=257))]
    ok_a, ok_qs, ok_qr = _label_args(), _stream_args(), _rnd_args()
    for a in bad_a:
        assert nxt(a, ok_qs, ok_qr) == EINVAL and latest(a, ok_qr) == EINVAL
    for qs in bad_qs:
        assert nxt(ok_a, qs, ok_qr) == EINVAL
    for qr in bad_qr:
        assert nxt(ok_a, ok_qs, qr) == EINVAL and latest(ok_a, qr) == EINVAL
    for k in range(n_out):
        ptrs = [p] * n_out
        ptrs[k] = None
        assert nxt(ok_a, ok_qs, ok_qr, ptrs=ptrs) == EINVAL, FIELDS[k]
    assert nxt(ok_a, ok_qs, ok_qr, items=None) == EINVAL and latest(ok_a, ok_qr, items=None) == EINVAL
    assert latest(ok_a, ok_qr, out=(None, p)) == EINVAL and latest(ok_a, ok_qr, out=(p, None)) == EINVAL
    for Bs, Br in ((0, 2), (-1, 2), (65536, 2), (2, 0), (2, -1), (2, 2 ** 26), (2 ** 15, 2 ** 24)):
        assert nxt(ok_a, ok_qs, ok_qr, Bs=Bs, Br=Br) == EINVAL, (Bs, Br)
    for B in (0, -1, 2 ** 26):
        assert latest(ok_a, ok_qr, B=B) == EINVAL
    big = dict(sequence_length=65535)
    assert nxt(ok_a, _stream_args(**big), _rnd_args(**big), Bs=2048, Br=2048) == EINVAL                     # (Bs + Br) * L * M
    assert lib.sast_launch_count() == before


def _cpu_labels(R=3, **kw):
    from sast_amd.labels import LabelStreams
    return LabelStreams(R, 100, max_frames=8, max_windows=32, max_labels_per_frame=4, **kw)


def test_mixed_pool_constructor_validation_and_cpu_tensors_raise():
    from sast_amd.sampling import MixedBatch, MixedPool, RandomAccessLatest, RandomAccessPool, StreamingPool
    ls = _cpu_labels()
    rp = RandomAccessPool(ls, H, W, sequence_length=5)
    sp = StreamingPool(ls, H, W, sequence_length=5, events=rp)
    mp = MixedPool(sp, rp)
    assert mp.stream is sp and mp.random is rp and mp.sequence_length == 5 and mp.num_rows == 3
    assert mp.frame_errors() == (0, 0) and mp.errors() == ((), ([()] * 3, ()))
    MixedPool(StreamingPool(ls, H, W, sequence_length=5, events=sp), rp)                    # shared through the existing sharing
    for s, r in ((rp, rp), (sp, sp), (None, rp), (sp, None)):
        with pytest.raises(TypeError):
            MixedPool(s, r)
    other = RandomAccessPool(ls, H, W, sequence_length=5)
    bad = [(StreamingPool(_cpu_labels(), H, W, sequence_length=5, events=rp), rp),          # another LabelStreams
           (StreamingPool(ls, H, W, sequence_length=3, events=rp), rp),                     # another sequence_length
           (StreamingPool(ls, H, W, sequence_length=5, events=rp, bins=4), rp),             # another geometry ...
           (StreamingPool(ls, H, W, sequence_length=5, events=rp, count_cutoff=3), rp),
           (StreamingPool(ls, H, W, sequence_length=5, events=rp, duration_us=10000), rp),
           (StreamingPool(ls, H, W, sequence_length=5, events=rp, window_capacity=10), rp),
           (StreamingPool(ls, H, W, sequence_length=5, events=rp, representation="mixed_density", count_cutoff=None), rp),
           (StreamingPool(ls, H, W, sequence_length=5), rp),                                # its own events
           (StreamingPool(ls, H, W, sequence_length=5, events=other), rp)]                  # another pool's events
    for s, r in bad:
        with pytest.raises(ValueError):
            MixedPool(s, r)
    # CPU tensors raise before anything else is looked at
    items = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mp.next(items)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rp.latest(items)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mp.prefetch_latest(items)
    cpu_batch = MixedBatch(*(torch.zeros(sh, dtype=dt) for sh, dt in mp._want(2, 2)))
    assert [tuple(t.shape) for t in cpu_batch[-2:]] == [(2, 4, 7), (2,)] and cpu_batch.labels.shape == (5, 4, 4, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mp.next(items, out=cpu_batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mp.frames(cpu_batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rp.latest(items, out=RandomAccessLatest(*cpu_batch[-2:]))
    for bad_items in (items.to(torch.int32), items[:0], items.view(1, 2)):
        with pytest.raises(ValueError):
            mp.next(bad_items)
        with pytest.raises(ValueError):
            rp.latest(bad_items)
    with pytest.raises(RuntimeError, match="prefetch_latest"):
        mp.latest_labels()
    with pytest.raises(RuntimeError, match="index"):
        mp.steps(2)
    for bad_b in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            mp.steps(bad_b)


def _reference_split(batch_size, w_stream, w_random):
    """set_mixed_sampling_mode_variables_for_train (modules/data/genx.py:116-129), its asserts as AssertionError"""
    assert batch_size >= 2
    assert w_random > 0
    assert w_stream > 0
    bs_rnd = min(round(batch_size * w_random / (w_stream + w_random)), batch_size - 1)
    return batch_size - bs_rnd, bs_rnd


def test_batch_sizes_equal_the_reference_formula():
    """batch sizes 2 .. 16 and the weight pairs 1:1, 1:3, 3:1 and 0.1:1, each pair both ways round (w_stream : w_random and
    w_random : w_stream).  Where the reference's split leaves a half empty the call must raise: a random weight of 0.1 against 1 at
    batch size 2 does (round(2 * 0.1 / 1.1) = 0), the other way round it gives min(round(1.82), 1) = 1 and 1."""
    from sast_amd.sampling import MixedPool
    pairs = ((1, 1), (1, 3), (3, 1), (0.1, 1))
    raised = []
    for bs in range(2, 17):
        for a, b in pairs:
            for w_stream, w_random in ((a, b), (b, a)):
                want = _reference_split(bs, w_stream, w_random)
                if min(want) < 1:
                    with pytest.raises(ValueError):
                        MixedPool.batch_sizes(bs, w_stream, w_random)
                    raised.append((bs, w_stream, w_random))
                    continue
                got = MixedPool.batch_sizes(bs, w_stream, w_random)
                assert got == want and sum(got) == bs and all(isinstance(v, int) for v in got), (bs, w_stream, w_random)
    assert (2, 1, 0.1) in raised and (2, 0.1, 1) not in raised and all(w_random < w_stream for _bs, w_stream, w_random in raised)
    assert MixedPool.batch_sizes(8, 1, 1) == (4, 4) and MixedPool.batch_sizes(8, 3, 1) == (6, 2) and MixedPool.batch_sizes(3, 0.1, 1) == (1, 2)
    assert MixedPool.batch_sizes(2, 0.1, 1) == (1, 1)                      # min(round(1.82), 2 - 1)
    for bad in ((1, 1, 1), (0, 1, 1), (2.0, 1, 1), (True, 1, 1), (4, 0, 1), (4, 1, 0), (4, -1, 1), (4, 1, float("nan"))):
        with pytest.raises(ValueError):
            MixedPool.batch_sizes(*bad)
    for bad in ((1, 1, 1), (4, 0, 1), (4, 1, 0)):                          # where the reference asserts
        with pytest.raises(AssertionError):
            _reference_split(*bad)


def _state(kind):
    from sast_amd import augment as A
    return {"flip": A.AugmentationState(apply_h_flip=True),
            "out": A.AugmentationState(zoom_out=A.ZoomOutState(True, 20, 10, 1.25)),
            "in": A.AugmentationState(apply_zoom_in=True, zoom_in=A.ZoomInState(True, 30, 12, 1.5)),
            "in2": A.AugmentationState(apply_h_flip=True, apply_zoom_in=True, zoom_in=A.ZoomInState(True, 7, 40, 1.25)),
            "none": A.AugmentationState()}[kind]


def test_joined_augmentor_row_bookkeeping_on_the_host():
    from sast_amd import _lib
    from sast_amd import augment as A
    alone = [A.SpatialAugmentor((H, W), GA.SHIPPED["stream"], 2), A.SpatialAugmentor((H, W), GA.SHIPPED["random"], 3)]
    parts = [A.SpatialAugmentor((H, W), GA.SHIPPED["stream"], 2), A.SpatialAugmentor((H, W), GA.SHIPPED["random"], 3)]
    parts[0].set_state([_state("flip"), _state("none")])                   # a state from before the join is kept
    alone[0].set_state([_state("flip"), _state("none")])
    j = A.JoinedAugmentor(parts)
    assert j.batch_size == 5 and j.offsets == [0, 2] and j.hw_tuple == (H, W) and j._host.shape == (5, _lib.AUGMENT_PARAM_WORDS)
    assert j.params is None and all(p.params is None and p._joined is j for p in parts)
    assert np.shares_memory(parts[0]._host, j._host) and np.shares_memory(parts[1]._host, j._host)

    def rows():
        return np.concatenate([a._host for a in alone])

    assert np.array_equal(j._host, rows()) and j._host[0, 0] == 1
    # set_state of one part rewrites its rows only, and validates as before
    states = [_state("in"), _state("out"), _state("in2")]
    parts[1].set_state(states)
    alone[1].set_state(states)
    assert np.array_equal(j._host, rows()) and np.array_equal(j._host[:2], np.concatenate([alone[0]._host]))
    assert np.shares_memory(parts[1]._host, j._host) and j.states == parts[0].states + parts[1].states and len(j.states) == 5
    with pytest.raises(ValueError):
        parts[1].set_state(states[:2])
    with pytest.raises(ValueError):
        parts[0].set_state([A.AugmentationState(apply_zoom_in=True, zoom_out=A.ZoomOutState(True, 0, 0, 1.1)), _state("none")])
    assert np.array_equal(j._host, rows())
    # randomize: the parts' draws, in the order of the calls, are those of stand-alone augmentors on the same generator
    latest = [torch.tensor(GA.boxes(5 + b, 2, H, W)) if b != 1 else None for b in range(3)]
    torch.manual_seed(77)
    parts[1].randomize(latest_labels=latest)
    parts[0].randomize(samples=[1])
    torch.manual_seed(77)
    alone[1].randomize(latest_labels=latest)
    alone[0].randomize(samples=[1])
    assert np.array_equal(j._host, rows()) and j.states == alone[0].states + alone[1].states
    assert np.shares_memory(parts[0]._host, j._host) and np.shares_memory(parts[1]._host, j._host)
    # what cannot be joined
    with pytest.raises(ValueError):
        A.JoinedAugmentor(parts)                                           # already parts of `j`
    fresh = A.SpatialAugmentor((H, W), GA.SHIPPED["stream"], 1)
    with pytest.raises(ValueError):
        A.JoinedAugmentor([fresh, fresh])
    with pytest.raises(ValueError):
        A.JoinedAugmentor([fresh, A.SpatialAugmentor((H // 2, W // 2), GA.SHIPPED["random"], 1)])
    for bad in ([], [fresh, None]):
        with pytest.raises(TypeError):
            A.JoinedAugmentor(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        j(torch.zeros(5, 2, H, W, dtype=torch.uint8))
    # a stand-alone augmentor is what it was: its own host array, its own params
    assert fresh._joined is None and fresh.params is None and not np.shares_memory(fresh._host, j._host)


# ---------------------------------------------------------------------------------------------------------------------------- GPU

@functools.lru_cache(maxsize=None)
def _words():
    return tuple(M.pack(GR.pool_records(n)) for n in GR.POOLS["gen1"])


def _labels(ds=False):
    """a loaded LabelStreams of the three gen1 fixture recordings, stale records behind every row's count"""
    from sast_amd.labels import LabelStreams
    rows = _words()
    assert len(rows) == 3
    cap = max(len(w) for w in rows) + 5
    rec = np.stack([np.resize(rows[0][-40:], (cap, 10)) for _ in rows])
    for s, w in enumerate(rows):
        rec[s, :len(w)] = w
    ls = LabelStreams(len(rows), cap, dataset="gen1", split="train", downsample_by_2=ds, **LABEL_KW)
    ls.load(torch.from_numpy(rec).cuda(), torch.tensor([len(w) for w in rows], dtype=torch.int64, device="cuda"))
    return ls


@functools.lru_cache(maxsize=None)
def _event_columns(R):
    """tests/test_streaming_pool.py's: R rows of hashed events over the time the label schedules span, one event in 16 out of order,
    different counts, stale events behind every count; the first corrected timestamps of rows 0 and 1 are 0"""
    cap = max(N_EV) + 3
    cols = [np.zeros((R, cap), np.int64) for _ in range(4)]
    for r in range(R):
        ev = G.stream(seed=170 + r, n=cap, height=H, width=W, t_start=0, t_step=4000, jitter=1500)
        for c, e in zip(cols, ev):
            c[r] = e
        cols[3][r, N_EV[r]:] = cols[3][r, N_EV[r] // 2]
    cols[3][:2, :6] = 0
    return tuple(cols), np.asarray(N_EV[:R], np.int64)


class _Rig:
    """a RandomAccessPool with the events, the StreamingPool and MixedPool under test on top of it, and a second StreamingPool on the same
    events: the stand-alone yardstick, which walks the same schedule on cursors of its own"""

    def __init__(self, L, end=False, ds=False, **kw):
        from sast_amd.sampling import MixedPool, RandomAccessPool, StreamingPool
        kw = {**FRAME_KW, **kw}
        self.L, self.kw = L, kw
        self.ls = ls = _labels(ds)
        self.rp = RandomAccessPool(ls, H, W, sequence_length=L, only_load_end_labels=end, downsample_by_2=ds, **kw)
        cols, counts = _event_columns(3)
        self.cols, self.counts = [torch.from_numpy(c).cuda() for c in cols], torch.from_numpy(counts).cuda()
        self.rp.load_events(*self.cols, self.counts)
        self.n_items, sizes = self.rp.index()
        self.cum = [0] + sizes
        self.sp = StreamingPool(ls, H, W, sequence_length=L, events=self.rp, downsample_by_2=ds, **kw)
        self.alone = StreamingPool(ls, H, W, sequence_length=L, events=self.rp, downsample_by_2=ds, **kw)
        self.n_seq, self.sequences = self.sp.index(check=True)
        assert self.alone.index(check=True)[0] == self.n_seq
        self.first_seq = self.sp.row_first_seq.tolist()
        self.mixed = MixedPool(self.sp, self.rp)

    def set_schedule(self, orders):
        self.sp.set_schedule(orders)
        self.alone.set_schedule(orders)

    def schedule(self, Bs):
        """the busiest recording (the one with most random-access items) leads batch row 0, followed by another sequence; row 1 holds one
        short sequence and runs out early; row 2 starts on the sequence of row 0 -> the orders, and that recording"""
        lengths = [b - a for a, b in zip(self.cum[:-1], self.cum[1:])]
        r = int(np.argmax(lengths))
        assert lengths[r] >= 2
        s0 = self.first_seq[r]
        padded = [s for s in range(self.n_seq) if (self.sequences[s, 2] - self.sequences[s, 1]) % self.L]
        short = int(np.argmin(self.sequences[:, 3]))
        tail = padded[0] if padded else (s0 + 1) % self.n_seq
        orders = [[s0, tail, short], [short], [s0, (s0 + 2) % self.n_seq]][:Bs]
        return orders, r

    def items(self, step, Br, r):
        """step 0: two items of recording r (one with Br = 1); later steps walk over all items"""
        if step == 0:
            return [self.cum[r], self.cum[r + 1] - 1, self.cum[r] + 1][:Br]
        return [(5 * step + 3 * j) % self.n_items for j in range(Br)]


def _expected(a, rb, L):
    """the concatenation of a StreamingBatch and a RandomAccessBatch in the MixedBatch layout"""
    Br = rb.rows.numel()
    dev = rb.rows.device

    def full(v, dtype, *shape):
        return torch.full(shape, v, dtype=dtype, device=dev)

    return (torch.cat([a.rows, rb.rows]), torch.cat([a.step_rows, rb.rows.expand(L, Br)], 1),
            torch.cat([a.seq, full(-1, torch.int32, Br)]), torch.cat([a.sample, full(-1, torch.int32, Br)]),
            torch.cat([a.is_first, full(1, torch.uint8, Br)]), torch.cat([a.exhausted, full(0, torch.uint8, Br)]),
            torch.cat([a.window_idx, rb.window_idx], 1), torch.cat([a.ends_us, rb.ends_us], 1), torch.cat([a.labels, rb.labels], 1),
            torch.cat([a.counts, rb.counts], 1), torch.cat([a.labelled, rb.labelled], 1),
            torch.cat([a.is_padded, full(0, torch.uint8, L, Br)], 1), rb.latest, rb.latest_count)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, where=""):
    assert len(got) == len(want) == len(FIELDS)
    for g, w, name in zip(got, want, FIELDS):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, where)
        assert torch.equal(_bits(g), _bits(w)), (name, where)


def _filled(mixed, Bs, Br):
    """every out= tensor holds 9s: an element the launch does not write shows"""
    return tuple(torch.full(sh, 9, dtype=dt, device="cuda") for sh, dt in mixed._want(Bs, Br))


def _dev_items(v):
    return torch.tensor(v, dtype=torch.int64, device="cuda")


def _walk_whole_schedule(L, Bs, Br, end):
    rig = _Rig(L, end)
    orders, r = rig.schedule(Bs)
    rig.set_schedule(orders)
    n = rig.sp.steps("longest")
    assert rig.mixed.steps(Br) == min(rig.sp.steps("shortest"), rig.n_items // Br)
    plan = rig.sp.plan()
    seen_pad = seen_done = seen_change = 0
    prev_seq = None
    for i in range(n + 1):                                  # one more step: every stream row has run out, the random columns go on
        host = rig.items(i, Br, r)
        items = _dev_items(host)
        into = _filled(rig.mixed, Bs, Br)
        out = rig.mixed.next(items, out=into)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, into))
        a, rb = rig.alone.next(), rig.rp.batch(items)
        _same(out, _expected(a, rb, L), i)
        assert torch.equal(rig.sp.cursor, rig.alone.cursor)
        rows = out.rows.tolist()
        assert min(rows[Bs:]) >= 0 and out.is_first[Bs:].tolist() == [1] * Br and not bool(out.is_padded[:, Bs:].any())
        if i < n:
            assert rig.mixed.labelled_pairs(i, host) == int(out.labelled.sum()) == int(plan.K[i]) + rig.rp.labelled_pairs(host)
        if i == 0 and Br >= 2:                              # two random samples on the recording a stream row is on
            assert rows[Bs] == rows[Bs + 1] == r == rows[0]
        seq = out.seq[:Bs].tolist()
        seen_pad += int(out.is_padded[:, :Bs][:, [v >= 0 for v in rows[:Bs]]].sum())
        seen_done += int(out.exhausted.sum())
        seen_change += sum(1 for p, s in zip(prev_seq or seq, seq) if p >= 0 and s >= 0 and p != s)
        if i > 0 and int(a.exhausted.sum()) > 0:
            assert int(out.labelled[:, Bs:].sum()) > 0      # a stream row has run out while the random columns go on
        prev_seq = seq
    assert (L == 1 or seen_pad > 0) and seen_done >= Bs and seen_change > 0 and out.exhausted.tolist() == [1] * Bs + [0] * Br
    assert rig.mixed.errors() == ((), ([()] * 3, ())) and rig.ls.errors() == [()] * 3
    # without out= the tensors are the pool's own, and a new schedule starts from zeroed cursors
    rig.set_schedule(orders)
    items = _dev_items(rig.items(0, Br, r))
    _same(rig.mixed.next(items), _expected(rig.alone.next(), rig.rp.batch(items), L))


@gpu
@pytest.mark.parametrize("L,Bs,Br", [(1, 1, 1), (3, 1, 3), (3, 3, 1), (3, 2, 2), (11, 2, 2)])
def test_next_over_a_whole_schedule_equals_the_concatenation(L, Bs, Br):
    _walk_whole_schedule(L, Bs, Br, end=False)


@gpu
@pytest.mark.parametrize("L,Bs,Br", [(3, 2, 2), (11, 1, 3)])
def test_next_with_only_load_end_labels_equals_the_concatenation(L, Bs, Br):
    _walk_whole_schedule(L, Bs, Br, end=True)


@gpu
def test_a_bad_schedule_entry_and_a_bad_item_each_set_their_own_status_word():
    L, Bs, Br = 3, 2, 2
    rig = _Rig(L)
    orders, r = rig.schedule(Bs)
    clean = ((), ([()] * 3, ()))
    # a schedule entry out of range (written past set_schedule, which would have refused it)
    rig.set_schedule(orders)
    for pool in (rig.sp, rig.alone):
        pool.order[1, 0] = rig.n_seq
    items = _dev_items(rig.items(0, Br, r))
    out = rig.mixed.next(items, out=_filled(rig.mixed, Bs, Br))
    assert rig.mixed.errors() == (("schedule_index",), ([()] * 3, ()))
    assert out.rows[1] == -1 and out.exhausted[1] == 0 and out.is_first[1] == 0 and bool(out.is_padded[:, 1].all())
    assert out.step_rows[:, 1].tolist() == [-1] * L == out.window_idx[:, 1].tolist() == out.ends_us[:, 1].tolist()
    assert int(out.counts[:, 1].sum()) == 0 and not bool(out.labels[:, 1].any()) and rig.sp.cursor[1].tolist() == [1, 0]
    _same(out, _expected(rig.alone.next(), rig.rp.batch(items), L), "bad schedule entry")
    assert min(out.rows[[0, 2, 3]].tolist()) >= 0
    rig.sp.index()
    rig.alone.index()
    assert rig.mixed.errors() == clean
    # an item out of range
    rig.set_schedule(orders)
    for k, bad in enumerate((rig.n_items, -1)):
        items = _dev_items([rig.cum[r], bad])
        out = rig.mixed.next(items, out=_filled(rig.mixed, Bs, Br))
        assert rig.mixed.errors() == ((), ([()] * 3, ("item_index",)))
        c = Bs + 1
        assert out.rows[c] == -1 and out.step_rows[:, c].tolist() == [-1] * L == out.window_idx[:, c].tolist() == out.ends_us[:, c].tolist()
        assert int(out.counts[:, c].sum()) == 0 and not bool(out.labels[:, c].any()) and int(out.labelled[:, c].sum()) == 0
        assert out.latest_count.tolist()[1] == 0 and not bool(out.latest[1].any())
        assert out.is_first[c] == 1 and out.seq[c] == -1 and out.exhausted[c] == 0 and not bool(out.is_padded[:, c].any())
        rig.rp.index()
        assert rig.mixed.errors() == clean
        _same(out, _expected(rig.alone.next(), rig.rp.batch(items), L), ("bad item", k))
        assert out.rows[0] >= 0 and out.rows[Bs] == r
        rig.rp.index()
    # the look-ahead flags a bad item as the gather does
    got = rig.rp.latest(_dev_items([rig.n_items]))
    assert got.latest_count.tolist() == [0] and not bool(got.latest.any()) and rig.mixed.errors() == ((), ([()] * 3, ("item_index",)))


@gpu
@pytest.mark.parametrize("representation", ["stacked_histogram", "mixed_density"])
def test_frames_equal_the_concatenation_of_both_pools_frames(representation):
    L, Bs, Br = 3, 2, 2
    kw = dict(representation=representation, count_cutoff=None) if representation == "mixed_density" else {}
    rig = _Rig(L, **kw)
    orders, r = rig.schedule(Bs)
    rig.set_schedule([[rig.first_seq[1]], orders[0]])                        # recording 1's one sequence: two windows, a padded tail at once
    seen_pad = 0
    for step in range(3):
        items = _dev_items(rig.items(step, Br, r))
        out = rig.mixed.next(items)
        a, rb = rig.alone.next(), rig.rp.batch(items)
        want = torch.cat([rig.alone.frames(a), rig.rp.frames(rb)], 1)
        into = torch.full((L, Bs + Br) + rig.sp.get_shape(), 9, dtype=rig.sp.frame_dtype, device="cuda")
        frames = rig.mixed.frames(out, out_frames=into)
        assert frames.data_ptr() == into.data_ptr() and frames.shape == want.shape and frames.dtype == want.dtype == rig.sp.frame_dtype
        assert torch.equal(frames, want), step
        assert torch.equal(rig.mixed.frames(out), want)
        padded = out.is_padded != 0
        seen_pad += int(padded.sum())
        assert not bool(frames[padded].any()) and int(frames[:, Bs:].count_nonzero()) > 0 and int(frames[:, :Bs].count_nonzero()) > 0
    assert seen_pad > 0 and rig.mixed.frame_errors() == (0, 0) == rig.alone.frame_errors() == rig.rp.frame_errors()
    assert rig.mixed.errors() == ((), ([()] * 3, ()))


@gpu
@pytest.mark.parametrize("end", [False, True])
def test_latest_and_its_prefetch_equal_the_batch(end, monkeypatch):
    L, Br = 3, 4
    rig = _Rig(L, end)
    rig.set_schedule([[0]])
    seen_some = 0
    for step in range(4):
        host = [(7 * step + 3 * j) % rig.n_items for j in range(Br)]
        items = _dev_items(host)
        rb = rig.rp.batch(items)
        into = (torch.full((Br, MX, 7), 9.0, device="cuda"), torch.full((Br,), 9, dtype=torch.int32, device="cuda"))
        got = rig.rp.latest(items, out=into)
        assert got.latest.data_ptr() == into[0].data_ptr()
        assert torch.equal(_bits(got.latest), _bits(rb.latest)) and torch.equal(got.latest_count, rb.latest_count)
        fresh = rig.rp.latest(items)
        assert torch.equal(_bits(fresh.latest), _bits(rb.latest)) and torch.equal(fresh.latest_count, rb.latest_count)
        # section 3g's host path against the look-ahead
        latest, n_latest = rb.latest.cpu(), rb.latest_count.tolist()
        want = [latest[b, :k] if k else None for b, k in enumerate(n_latest)]
        rig.mixed.prefetch_latest(items)
        rig.mixed.next(_dev_items(host[:1]))                 # work enqueued behind the prefetch does not disturb it
        have = rig.mixed.latest_labels()
        assert len(have) == len(want) == Br
        for h, w in zip(have, want):
            assert (h is None) == (w is None)
            if w is not None:
                assert not h.is_cuda and h.shape == w.shape and h.shape[1] == 7 and torch.equal(_bits(h), _bits(w))
        seen_some += sum(w is not None for w in want)
    assert seen_some > 0
    assert rig.mixed.errors() == ((), ([()] * 3, ()))
    # the look-ahead of step n + 1 is enqueued before step n's labels are read: two may be pending, handed out oldest first
    ahead = [_dev_items([(j + k) % rig.n_items for j in range(Br)]) for k in (0, 1)]
    for it in ahead:
        rig.mixed.prefetch_latest(it)
    with pytest.raises(RuntimeError, match="pending"):
        rig.mixed.prefetch_latest(items)
    for it in ahead:
        rb, have = rig.rp.batch(it), rig.mixed.latest_labels()
        assert [0 if h is None else len(h) for h in have] == rb.latest_count.tolist()
        assert all(h is None or torch.equal(_bits(h), _bits(rb.latest[b, :len(h)].cpu())) for b, h in enumerate(have))
    with pytest.raises(RuntimeError, match="prefetch_latest"):
        rig.mixed.latest_labels()
    rig.mixed.prefetch_latest(items)
    # both calls copy to the host or wait for the copy: they refuse to run while the stream is capturing (no capture is begun here)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for call in (lambda: rig.mixed.prefetch_latest(items), rig.mixed.latest_labels):
        with pytest.raises(RuntimeError, match="outside graph capture"):
            call()


def _aug_inputs(rig, Bs, Br, r):
    out = rig.mixed.next(_dev_items(rig.items(0, Br, r)))
    return out, rig.mixed.frames(out)


@gpu
def test_joined_augmentor_equals_each_part_on_its_half():
    from sast_amd import augment as A
    L, Bs, Br = 3, 2, 2
    rig = _Rig(L)
    orders, r = rig.schedule(Bs)
    rig.set_schedule(orders)
    out, frames = _aug_inputs(rig, Bs, Br, r)
    assert int(out.counts[:, :Bs].sum()) > 0 and int(out.counts[:, Bs:].sum()) > 0
    cfgs = (GA.SHIPPED["stream"], GA.SHIPPED["random"])
    parts = [A.SpatialAugmentor((H, W), cfgs[0], Bs), A.SpatialAugmentor((H, W), cfgs[1], Br)]
    alone = [A.SpatialAugmentor((H, W), cfgs[0], Bs), A.SpatialAugmentor((H, W), cfgs[1], Br)]
    joined = A.JoinedAugmentor(parts)
    halves = (slice(0, Bs), slice(Bs, Bs + Br))

    def want(yolox):
        res = [a(frames[:, h].contiguous(), out.labels[:, h].contiguous(), out.counts[:, h].contiguous(), yolox=yolox)
               for a, h in zip(alone, halves)]
        return [torch.cat([res[0][k], res[1][k]], 1) for k in range(3)]

    def check(got, exp, what):
        for g, w, name in zip(got, exp, ("frames", "labels", "counts")):
            assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(_bits(g), _bits(w)), (what, name)

    states = ([_state("flip"), _state("out")], [_state("in"), _state("none")])
    for p, a, s in zip(parts, alone, states):
        p.set_state(s)
        a.set_state(s)
    first = {}
    for yolox in (False, True):
        first[yolox] = joined.joined(frames, out.labels, out.counts, yolox=yolox)
        check(first[yolox], want(yolox), f"yolox={yolox}")
    assert first[True][1].shape == (L, Bs + Br, MX, 5) and joined.params.shape[0] == Bs + Br
    assert not torch.equal(first[False][0], frames) and int(first[False][2].sum()) > 0
    # the random part alone gets new states: only the random columns change
    new = [_state("none"), _state("in2")]
    parts[1].set_state(new)
    alone[1].set_state(new)
    into = torch.full_like(frames, 9)
    second = joined(frames, out.labels, out.counts, yolox=True, out=into)
    assert second[0].data_ptr() == into.data_ptr()
    check(second, want(True), "after parts[1].set_state")
    for a, b in zip(first[True], second):
        assert torch.equal(_bits(a[:, :Bs]), _bits(b[:, :Bs]))
    assert not torch.equal(first[True][0][:, Bs:], second[0][:, Bs:])
    # frames alone, and a part called on its own half reads its rows of the joined tensor
    assert torch.equal(joined(frames), second[0])
    assert torch.equal(parts[1](frames[:, Bs:].contiguous()), second[0][:, Bs:])


@gpu
def test_mixed_launch_counts_are_the_documented_ones():
    from sast_amd import _lib
    from sast_amd import augment as A
    lib = _lib.lib()

    def launches(fn):
        before = lib.sast_launch_count()
        res = fn()
        return lib.sast_launch_count() - before, res

    for L, Bs, Br in ((3, 2, 2), (5, 1, 3)):
        rig = _Rig(L)
        orders, r = rig.schedule(Bs)
        rig.set_schedule(orders)
        items = _dev_items(rig.items(0, Br, r))
        k, out = launches(lambda: rig.mixed.next(items))
        assert k == NEXT_LAUNCHES
        k, frames = launches(lambda: rig.mixed.frames(out))
        assert k == FRAMES_LAUNCHES
        joined = A.JoinedAugmentor([A.SpatialAugmentor((H, W), GA.SHIPPED["stream"], Bs), A.SpatialAugmentor((H, W), GA.SHIPPED["random"], Br)])
        assert launches(lambda: joined.joined(frames, out.labels, out.counts, yolox=True))[0] == JOINED_LAUNCHES
        assert launches(lambda: rig.rp.latest(items))[0] == LATEST_LAUNCHES
        assert launches(lambda: rig.mixed.prefetch_latest(items))[0] == LATEST_LAUNCHES
        assert launches(rig.mixed.latest_labels)[0] == 0
        assert launches(lambda: joined.parts[1].set_state([_state("none")] * Br))[0] == 0


@gpu
def test_next_frames_and_joined_augmentation_in_one_graph_follow_new_items_and_a_new_schedule():
    """next + frames + joined(yolox=True) captured once after a warm-up; then a new schedule, and before each of six replays new items
    written into the captured `items` tensor == six eager merged calls on a second pair of pools, step by step"""
    from sast_amd import augment as A
    L, Bs, Br, n = 3, 2, 2, 6
    rig, twin = _Rig(L), _Rig(L)
    orders, r = rig.schedule(Bs)

    def augmentor():
        parts = [A.SpatialAugmentor((H, W), GA.SHIPPED["stream"], Bs), A.SpatialAugmentor((H, W), GA.SHIPPED["random"], Br)]
        parts[0].set_state([_state("flip"), _state("out")])
        parts[1].set_state([_state("in"), _state("none")])
        return A.JoinedAugmentor(parts)

    def call(g, aug, items):
        out = g.mixed.next(items)
        frames = g.mixed.frames(out)
        return aug.joined(frames, out.labels, out.counts, yolox=True) + tuple(out)

    aug, twin_aug = augmentor(), augmentor()
    items, twin_items = _dev_items([0] * Br), _dev_items([0] * Br)
    host_items = [rig.items(i, Br, r) for i in range(n)]
    twin.set_schedule(orders)
    eager = []
    for i in range(n):
        twin_items.copy_(torch.tensor(host_items[i]))
        eager.append([t.clone() for t in call(twin, twin_aug, twin_items)])
    assert twin.sp.steps("shortest") < n and int(eager[0][0].count_nonzero()) > 0 and not torch.equal(eager[0][0], eager[1][0])
    rig.set_schedule([[0], [1]])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(rig, aug, items)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = call(rig, aug, items)
    rig.set_schedule(orders)
    for i in range(n):
        items.copy_(torch.tensor(host_items[i]))
        graph.replay()
        torch.cuda.synchronize()
        for k, (got, exp) in enumerate(zip(captured, eager[i])):
            assert torch.equal(_bits(got), _bits(exp)), (i, k)
    assert torch.equal(rig.sp.cursor, twin.sp.cursor) and int(rig.sp.cursor.sum()) > 0
    assert rig.mixed.errors() == ((), ([()] * 3, ())) and rig.mixed.frame_errors() == (0, 0)


# ------------------------------------------------------------------------------------------------------------- the training step

# tests/test_device_selection.py's smallest rig and its bars: 10x what two runs of the same eager step differ by on twin rigs at these
# shapes (profiles/r15_device_selection.txt), the gradient's capped at 1e-4 of its max-norm.  Here both rigs run the same step on
# bit-identical inputs, so the order of the floating-point atomics is all that differs, as there.
HW, PART, EMBED, T_SEQ, NUM_CLASSES = (128, 160), (4, 5), 32, 3, 2
LOSS_RTOL, GRAD_RTOL = 10 * 8.165e-08, min(10 * 1.068e-06, 1e-4)


def _load_params(module, params):
    """oracle-named parameters -> a sast_amd module (tests/test_gpu_parity.py's load_params)"""
    sd = module.state_dict()
    new = {}
    for k in sd:
        kk = k
        for a, b in (("sub_layers.0.", "ls1."), ("sub_layers.2.", "norm2."), ("sub_layers.3.", "mlp."), ("sub_layers.4.", "ls2.")):
            kk = kk.replace(a, b)
        new[k] = sd[k] if kk.endswith("num_batches_tracked") else params[kk]
    module.load_state_dict(new, strict=True)


def _train_rig(params):
    from sast_amd.config import backbone_config
    from sast_amd.detection import RNNDetector, YOLOPAFPN, YOLOXHead
    from sast_amd.training import TrainStep
    net = RNNDetector(backbone_config(HW, PART, embed_dim=EMBED, AMP=2e-2, ls_init_value=0.5, dim_head=32)).cuda()
    fpn = YOLOPAFPN(depth=0.67, in_stages=(2, 3, 4), in_channels=(64, 128, 256)).cuda().train()
    head = YOLOXHead(num_classes=NUM_CLASSES, strides=(8, 16, 32), in_channels=(64, 128, 256)).cuda().train()
    for m, p in zip((net, fpn, head), params):
        _load_params(m, p)
    return TrainStep(net, fpn, head, lr=0.0, segmented=True)


@gpu
def test_one_merged_training_step_equals_the_step_on_hand_concatenated_tensors():
    """three steps of TrainStep(selection=, reset=batch.is_first, carry_states=True) on the merged batch (2 streamed rows + 1 random
    sample, gen1 frames at half resolution, 20 channels, zero-padded to the backbone's 128 x 160) against the same rig fed with the two
    stand-alone pools' tensors concatenated by hand: kept-token counts, loss and flat gradient of every step.
    Measured on the MI355X: loss rel 0 in all three steps (bar 8.2e-07); flat gradient 7.8e-07 .. 9.0e-07 of its max-norm (bar 1.07e-05)."""
    from oracle import sast_oracle as O
    from sast_amd import augment as A
    from sast_amd import functional as SF
    L, Bs, Br = T_SEQ, 2, 1
    B = Bs + Br
    rig = _Rig(L, ds=True, bins=10, count_cutoff=10)
    hw = (H // 2, W // 2)
    assert rig.sp.get_shape() == (20,) + hw
    ocfg = O.BackboneCfg(in_res_hw=HW, partition_size=PART, embed_dim=EMBED, amp=2e-2)
    params = (O.init_backbone_params(ocfg, seed=61, ls_init=0.5), O.init_pafpn_params((64, 128, 256), seed=62),
              O.init_head_params((64, 128, 256), num_classes=NUM_CLASSES, seed=63))
    merged, by_hand = _train_rig(params), _train_rig(params)
    orders, r = rig.schedule(Bs)
    rig.set_schedule(orders)
    aug = A.SpatialAugmentor(hw, GA.SHIPPED["stream"], B)                  # no state set: it only turns the label rows into the head's layout

    def inputs(frames, labels, counts):
        frames, labels5, counts5 = aug(frames, labels, counts, yolox=True)
        frames = torch.nn.functional.pad(frames, (0, HW[1] - hw[1], 0, HW[0] - hw[0]))
        return [f.contiguous() for f in frames.unbind(0)], labels5, counts5

    # the state tensors of both rigs: zeros of the shapes a first step leaves
    probe = inputs(torch.zeros((L, B, 20) + hw, dtype=torch.uint8, device="cuda"), torch.zeros(L, B, MX, 7, device="cuda"),
                   torch.zeros(L, B, dtype=torch.int32, device="cuda"))
    with torch.no_grad():
        _out, shapes, _P = merged.net.forward_nhwc(probe[0][0], None)
    states = [[(torch.zeros_like(h), torch.zeros_like(c)) for h, c in shapes] for _ in range(2)]
    tables = {}
    for step in range(3):
        host = rig.items(step, Br, r)
        items = _dev_items(host)
        batch = rig.mixed.next(items)
        xs, labels5, counts5 = inputs(rig.mixed.frames(batch), batch.labels, batch.counts)
        a, rb = rig.alone.next(), rig.rp.batch(items)
        cat = [torch.cat(p, 1) for p in ((rig.alone.frames(a), rig.rp.frames(rb)), (a.labels, rb.labels), (a.counts, rb.counts),
                                         (a.labelled, rb.labelled))]
        hand_xs, hand_labels5, hand_counts5 = inputs(*cat[:3])
        hand_reset = torch.cat([a.is_first, torch.ones(Br, dtype=torch.uint8, device="cuda")])
        # the random column is reset at every step: the states it carried were zeroed when this step read them
        assert batch.is_first[Bs:].tolist() == [1] * Br and torch.equal(batch.is_first, hand_reset)
        if step > 0:
            assert all(float(h[Bs:].abs().max()) > 0 for h, _c in states[0])      # ... and there was something to zero
        K = rig.mixed.labelled_pairs(step, host)
        assert K == int(batch.labelled.sum()) and K >= 1
        for ts, st, (x, lab, cnt, labelled, reset) in ((merged, states[0], (xs, labels5, counts5, batch.labelled, batch.is_first)),
                                                        (by_hand, states[1], (hand_xs, hand_labels5, hand_counts5, cat[3], hand_reset))):
            sel = tables.setdefault((id(ts), K), SF.SelectionTable(L, B, K, labelled.device)).update(labelled, check=True)
            ts.step(x, st, lab, selection=sel, reset=reset, carry_states=True, label_counts=cnt)
        torch.cuda.synchronize()
        la, lb = float(merged.loss.detach()), float(by_hand.loss.detach())
        ga, gb = merged.flat.grad, by_hand.flat.grad
        scale, err = float(gb.abs().max()), float((ga - gb).abs().max())
        print(f"[mixed-pool] step {step}: K {K}, loss {la:.9g} vs {lb:.9g} (rel {abs(la - lb) / abs(lb):.3e}, bar {LOSS_RTOL:.1e}); flat "
              f"gradient max err {err:.3e} of max-norm {scale:.3e} (rel {err / scale:.3e}, bar {GRAD_RTOL:.1e})")
        assert [int(p) for p in merged.P] == [int(p) for p in by_hand.P], step
        assert scale > 0 and bool(torch.isfinite(ga).all())
        assert abs(la - lb) <= LOSS_RTOL * abs(lb), (step, la, lb)
        assert err <= GRAD_RTOL * scale, (step, err, scale)
    assert rig.mixed.errors() == ((), ([()] * 3, ())) and rig.mixed.frame_errors() == (0, 0)
