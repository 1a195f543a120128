"""Events -> raw EVT 3.0 sensor words on the device (sast_amd.events.Evt3Encoder, evt3_raw_header; the sast_evt3enc_* entry points of
csrc/k_evt3_enc.hip).

The CPU tests hold the sequential model of the canonical rule (tests/evt3_encoder_model.py) to the decoder's model (tests/evt3_model.py):
every event comes back, whatever the cuts.  The GPU tests hold the device encoder, call by call, to that model: the words, their
number, the state after every chunk and the four counters.  Everything is integers: there is no tolerance.  Every chunk row carries
stale events past its count that would give words."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import evt3_encoder_model as E  # noqa: E402
import evt3_model as M  # noqa: E402

gpu = pytest.mark.gpu

ENCODE_LAUNCHES = 2
GEO = dict(height=48, width=64)


def _keep_alives(t, t_first_prev=None):
    prev = np.concatenate([[t[0] if t_first_prev is None else t_first_prev], t[:-1]])
    gap = (t >> 12) - (prev >> 12)
    return int(np.where(gap > 0, (gap - 1) // 1024, 0).sum())


def _round_trip(ev, cuts=()):
    """the events through the encoder's model (in chunks cut at `cuts`) and the decoder's model: every event back, no event before the
    first TIME_HIGH, no unknown word, at most 5 words per event plus the keep-alives, no single event sent as a vector -> the words"""
    x, y, p, t = ev
    words = E.encode(x, y, p, t, cuts=cuts)
    got, counters, _state = M.decode(words)
    base = (int(t[0]) >> 24) << 24 if len(t) else 0                  # a fresh decoder starts its wraps at 0
    assert counters == (0, 0)
    for name, g, w in zip("xypt", got, (x, y, p, t - base)):
        assert np.array_equal(g, w), name
    assert len(words) <= 5 * len(t) + _keep_alives(t)
    codes = words >> 12
    assert set(codes.tolist()) <= {M.TIME_HIGH, M.TIME_LOW, M.ADDR_Y, M.ADDR_X, M.VECT_BASE_X, M.VECT_12}
    masks = (words[codes == M.VECT_12] & 0xFFF).astype(np.int64)
    assert all(bin(int(m)).count("1") >= 2 for m in masks)
    return words


# ---------------------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("kw,rate", [(dict(bursts=0.0), (2.0, 3.1)), (dict(bursts=0.9, t_step=4), (1.0, 1.5))],
                         ids=["sparse", "bursts"])
def test_model_round_trips_sparse_and_burst_streams(kw, rate):
    for seed in range(6):
        ev = M.recording(100 + seed, 3000 - 400 * seed, **kw)
        words = _round_trip(ev)
        assert rate[0] <= len(words) / len(ev[0]) <= rate[1], len(words) / len(ev[0])
        rng = np.random.RandomState(seed)
        _round_trip(ev, cuts=rng.randint(0, len(ev[0]) + 1, size=7))
    assert ((_round_trip(M.recording(7, 400, bursts=0.9)) >> 12) == M.VECT_12).sum() > 100


def test_model_round_trips_three_clock_wraps_and_keep_alives():
    for bursts, wraps in ((0.3, 1), (0.0, 3)):                       # a burst takes one time step for several events
        ev = M.recording(1, 3000, t_end=60_000_000, bursts=bursts)
        assert int(ev[3][-1]) >> 24 >= wraps
        assert M.decode(_round_trip(ev))[2][5] == int(ev[3][-1]) >> 24
        _round_trip(ev, cuts=[1, 700, 701, 2999])
    ev = M.recording(2, 200, t_step=5_000_000)                       # gaps of several times 1024 TIME_HIGH steps
    assert _keep_alives(ev[3]) >= 10 and int(ev[3][-1]) >> 24 > 10
    words = _round_trip(ev)
    highs = (words[(words >> 12) == M.TIME_HIGH] & 0xFFF).astype(np.int64)
    assert (np.diff(highs) % 4096 <= 1024).all()
    _round_trip(ev, cuts=[50, 51, 120])


def test_model_first_event_beyond_the_24_bit_clock():
    ev = M.recording(3, 500, t_start=5 * (1 << 24) + 77)
    words = _round_trip(ev)                                          # _round_trip subtracts (t0 >> 24) << 24
    assert int(words[0]) == M.word(M.TIME_HIGH, (int(ev[3][0]) >> 12) & 0xFFF)
    got, _c, state = M.decode(words)
    assert got[3][0] == int(ev[3][0]) - 5 * (1 << 24) and state[5] == (int(ev[3][-1]) >> 24) - 5


def test_model_gives_the_events_back_at_every_cut_of_a_stream():
    ev = M.recording(4, 60, bursts=0.8, t_step=3000)
    whole = E.encode(*ev)
    lengths = set()
    for k in range(61):
        words = _round_trip(ev, cuts=[k])
        lengths.add(len(words))
        for k2 in (k // 2, min(k + 3, 60)):
            _round_trip(ev, cuts=[k, k2])
    assert len(whole) == min(lengths) and len(lengths) > 1           # a cut ends a group: the words depend on the cuts


def test_model_on_hand_written_events():
    W = M.word
    t0 = 3 * 4096 + 5
    # a single, a group over a 12-boundary (two groups, the second chained), a group whose second block starts fresh after a gap in x
    x = [5, 20, 22, 23, 24, 26, 40, 41, 60]
    y = [7, 7, 7, 7, 7, 7, 9, 9, 9]
    p = [1, 0, 0, 0, 0, 0, 1, 1, 1]
    t = [t0, t0, t0, t0, t0, t0, t0 + 1, t0 + 1, t0 + 1 + 4096]
    words = E.encode(*(np.array(c, np.int64) for c in (x, y, p, t)))
    assert words.tolist() == [
        W(M.TIME_HIGH, 3), W(M.TIME_LOW, 5), W(M.ADDR_Y, 7), W(M.ADDR_X, 5 | 0x800),
        W(M.VECT_BASE_X, 12), W(M.VECT_12, 1 << 8 | 1 << 10 | 1 << 11), W(M.VECT_12, 1 << 0 | 1 << 2),     # 24, 26: chained, no base
        W(M.TIME_LOW, 6), W(M.ADDR_Y, 9), W(M.VECT_BASE_X, 36 | 0x800), W(M.VECT_12, 1 << 4 | 1 << 5),
        W(M.TIME_HIGH, 4), W(M.TIME_LOW, 6), W(M.ADDR_X, 60 | 0x800)]                                   # the same low bits, sent again
    # bad input: nothing is dropped, every change is counted
    enc = E.Encoder()
    words = enc.feed([3000, 1, -4], [2, 5000, 2], [5, 0, -1], [50, 40, 60])
    got, _c, _s = M.decode(words)
    assert [g.tolist() for g in got] == [[2047, 1, 0], [2, 2047, 2], [1, 0, 1], [50, 50, 60]]
    assert (enc.raised, enc.clamped, enc.refused) == (1, 3, 0) and enc.state().tolist() == [1, 60, 2, 0]
    assert len(enc.feed([1] * 4, [1] * 4, [0] * 4, [70, 80, 90, 100], max_words=4)) == 0          # 3 + 2 + 2 + 2 words: refused
    assert (enc.raised, enc.clamped, enc.refused) == (1, 3, 1) and enc.state().tolist() == [1, 60, 2, 0]


def test_raw_header_round_trips():
    from sast_amd.events import evt3_raw_header, raw_header
    for h, w in ((720, 1280), (48, 64), (1, 2048)):
        head = evt3_raw_header(h, w)
        assert isinstance(head, bytes) and head.startswith(b"% ") and head.endswith(b"% end\n")
        assert all(line.startswith(b"% ") for line in head.splitlines())
        words = E.encode(*M.recording(5, 40, height=min(h, 48), width=min(w, 64)))
        got = raw_header(head + words.astype("<u2").tobytes())
        assert (got.format, got.height, got.width, got.offset) == ("evt3", h, w, len(head))
        assert np.array_equal(np.frombuffer((head + words.astype("<u2").tobytes())[got.offset:], "<u2"), words)
        assert raw_header(head + b"%").offset == len(head)           # a data byte 0x25 right behind the header is data
    for bad in ((0, 64), (48, 0), (2049, 64), (48, 4096)):
        with pytest.raises(ValueError, match="2048"):
            evt3_raw_header(*bad)


def test_encode_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_evt3enc_")]
    assert sorted(names) == ["sast_evt3enc_encode", "sast_evt3enc_encode_dat", "sast_evt3enc_ws_bytes"]
    lib = _lib.lib()
    P = C.c_void_p
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert _lib._SIGNATURES["sast_evt3enc_encode"] == (C.c_int, [P, P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int64, C.c_int, P, P, P, P,
                                                              C.c_int64, P, P, P])
    assert _lib._SIGNATURES["sast_evt3enc_encode_dat"] == (C.c_int, [P, P, C.c_int64, C.c_int, P, P, P, P, C.c_int64, P, P, P])
    assert (_lib.EVT3_ENC_STATE_WORDS, _lib.EVT3_ENC_BLOCK_EVENTS, _lib.EVT3_ENC_MAX_BLOCKS) == (4, 1024, 256)
    for n_streams in (1, 3, 65535):
        assert lib.sast_evt3enc_ws_bytes(n_streams) == n_streams * (_lib.EVT3_ENC_MAX_BLOCKS + 1) * 32
    assert lib.sast_evt3enc_ws_bytes(0) == 0 and lib.sast_evt3enc_ws_bytes(65536) == 0


def test_encode_rejects_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib = _lib.lib()
    q = 0x1000
    common = dict(counts=q, chunk_events=256, S=3, reset=None, state=q, ws=q, words=q, max_words=2304, n_words=q, err=q)
    cols = dict(x=q, y=q, p=q, t=q, x_dtype=_lib.DT_I16, y_dtype=_lib.DT_I32, p_dtype=_lib.DT_I64, t_dtype=_lib.DT_I64, **common)
    dat = dict(records=q, **common)
    for fn, good in ((lib.sast_evt3enc_encode, cols), (lib.sast_evt3enc_encode_dat, dat)):

        def call(**kw):
            a = dict(good, **kw)
            return fn(*[a[k] for k in good], None)

        for name in [k for k, v in good.items() if v == q]:
            assert call(**{name: None}) == -22, name
        for kw in (dict(S=0), dict(S=65536), dict(chunk_events=-1), dict(S=8, chunk_events=2 ** 28), dict(max_words=0), dict(max_words=-4),
                   dict(max_words=2 ** 30), dict(words=q + 1), dict(ws=q + 4)):
            assert call(**kw) == -22, kw
    for kw in (dict(x_dtype=_lib.DT_F32), dict(y_dtype=_lib.DT_U8), dict(p_dtype=99), dict(t_dtype=_lib.DT_I16), dict(t_dtype=_lib.EVQUEUE_DT_DAT)):
        a = dict(cols, **kw)
        assert lib.sast_evt3enc_encode(*[a[k] for k in cols], None) == -22, kw
    assert lib.sast_evt3enc_encode_dat(*[dict(dat, records=q + 4)[k] for k in dat], None) == -22


def test_encoder_python_argument_validation(monkeypatch):
    from sast_amd.events import Evt3Encoder
    S = 3
    with pytest.raises(ValueError, match="num_streams"):
        Evt3Encoder(0)
    with pytest.raises(ValueError, match="max_words"):
        Evt3Encoder(3, 0)
    with pytest.raises(ValueError, match="2\\^31"):
        Evt3Encoder(3, 2 ** 30)
    enc = Evt3Encoder(S)
    assert enc.errors() == (0, 0, 0, 0) and enc.ENCODE_LAUNCHES == ENCODE_LAUNCHES and enc.state is None
    enc.reset()
    enc.reset(streams=[1])
    cols = [torch.zeros(S, 16, dtype=d) for d in (torch.int16, torch.int32, torch.int64, torch.int64)]
    counts = torch.zeros(S, dtype=torch.int64)
    records = torch.zeros(S, 16, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(*cols, counts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.encode_dat(records, counts)
    with pytest.raises(TypeError, match="int64"):
        enc(cols[0].to(torch.uint8), *cols[1:], counts)
    with pytest.raises(TypeError, match="t must be"):
        enc(*cols[:3], cols[3].to(torch.int16), counts)
    with pytest.raises(ValueError, match="num_streams=3"):
        enc(*(c[:2] for c in cols), counts)
    with pytest.raises(ValueError, match="same shape"):
        enc(cols[0], cols[1][:, :8].contiguous(), *cols[2:], counts)
    with pytest.raises(ValueError, match="contiguous"):
        enc(cols[0].t().contiguous().t(), *cols[1:], counts)
    with pytest.raises(TypeError, match="int32"):
        enc.encode_dat(records.to(torch.int64), counts)
    with pytest.raises(ValueError, match="num_streams=3"):
        enc.encode_dat(records[:, :, :1], counts)
    for call, args in ((enc, cols), (enc.encode_dat, [records])):
        with pytest.raises(ValueError, match="counts"):
            call(*args, counts.to(torch.int32))
        with pytest.raises(ValueError, match="counts"):
            call(*args, counts[:2])
        with pytest.raises(ValueError, match="reset"):
            call(*args, counts, torch.zeros(S, dtype=torch.int32))
        with pytest.raises(ValueError, match="reset"):
            call(*args, counts, torch.zeros(S + 1, dtype=torch.uint8))
    assert enc.state is None and enc.words is None                  # nothing was allocated on the way
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="un-captured"):          # the state and the staging are never born in a capture
        enc._buffers(torch.device("cpu"), 16)
    assert enc.state is None and enc.words is None


# ---------------------------------------------------------------------------------------------------------------------------- GPU

STALE = (7, 3, 1, 1 << 40)                # what lies past a row's count: it would be an event
DTYPES = (torch.int16, torch.int32, torch.int64, torch.int64)


def _dev_columns(parts, cap, dtypes=DTYPES):
    """per-row (x, y, p, t) -> (four [S, cap] tensors with stale events past each count, counts int64 [S]) on the device"""
    cols = [np.full((len(parts), cap), g, np.int64) for g in STALE]
    if dtypes[3] == torch.int32:
        cols[3][:] = 2 ** 31 - 1
    for s, part in enumerate(parts):
        for c, a in zip(cols, part):
            c[s, :len(a)] = a
    return ([torch.from_numpy(c).to(d).cuda() for c, d in zip(cols, dtypes)],
            torch.tensor([len(part[0]) for part in parts], dtype=torch.int64).cuda())


def _dev_records(parts, cap):
    """the same events as packed Event2D records int32 [S, cap, 2]"""
    rec = np.zeros((len(parts), cap, 2), np.uint32)
    rec[:, :, 0], rec[:, :, 1] = 0xFFFFFFF0, 7 | (3 << 14) | (1 << 28)
    for s, (x, y, p, t) in enumerate(parts):
        rec[s, :len(t), 0] = t
        rec[s, :len(t), 1] = x | (y << 14) | (p << 28)
    return torch.from_numpy(rec.view(np.int32)).cuda(), torch.tensor([len(part[0]) for part in parts], dtype=torch.int64).cuda()


def _cut(ev, a, b):
    return tuple(c[a:b] for c in ev)


class _Session:
    """a device encoder beside one model per row: every `call` encodes one chunk per row on both and compares all of it"""

    def __init__(self, S, max_words=None, dtypes=DTYPES):
        from sast_amd.events import Evt3Encoder
        self.S, self.dtypes = S, dtypes
        self.enc = Evt3Encoder(S, max_words)
        self.models = [E.Encoder() for _ in range(S)]

    def expect(self, parts, reset, limit):
        want = []
        for s, part in enumerate(parts):
            if reset is not None and reset[s]:
                self.models[s].reset()
            want.append(self.models[s].feed(*part, max_words=limit))
        return want

    def check(self, words, n, want, tag):
        assert words.dtype == torch.int16 and n.dtype == torch.int64 and tuple(n.shape) == (self.S,) and words.shape[0] == self.S
        got_n, got = n.cpu().tolist(), words.cpu().numpy().view(np.uint16)
        for s, w in enumerate(want):
            assert got_n[s] == len(w), (tag, s, got_n[s], len(w))
            assert np.array_equal(got[s, :len(w)], w), (tag, s, np.nonzero(got[s, :len(w)] != w)[0][:5])
        assert np.array_equal(self.enc.state.cpu().numpy(), np.stack([m.state() for m in self.models])), tag
        return got_n

    def call(self, parts, cap=None, reset=None, tag=None, dat=False):
        cap = max(len(part[0]) for part in parts) + 3 if cap is None else cap
        rst = None if reset is None else torch.tensor(reset, dtype=torch.uint8).cuda()
        if dat:
            rec, counts = _dev_records(parts, cap)
            words, n = self.enc.encode_dat(rec, counts, rst)
        else:
            cols, counts = _dev_columns(parts, cap, self.dtypes)
            words, n = self.enc(*cols, counts, rst)
        return self.check(words, n, self.expect(parts, reset, words.shape[1]), tag)

    def counters(self):
        return sum(m.raised for m in self.models), sum(m.clamped for m in self.models), sum(m.refused for m in self.models), 0

    def finish(self):
        assert self.enc.errors() == self.counters()


@pytest.fixture(scope="module")
def Bk():
    from sast_amd import _lib
    return _lib.EVT3_ENC_BLOCK_EVENTS


@pytest.fixture(scope="module")
def recs(Bk):
    """a bursty recording through a clock wrap and a sparse one with keep-alive gaps, each longer than 2 x Bk + 3 events"""
    a = M.recording(21, 2 * Bk + 40, bursts=0.7, t_end=int(1.3 * 2 ** 24), **GEO)
    b = M.recording(22, 2 * Bk + 40, bursts=0.1, t_step=9000, height=720, width=1280)
    b[3][50:] += 20_000_000                                          # silences that need keep-alives, one of them at event Bk
    b[3][Bk:] += 9_000_000
    assert int(b[3][-1]) < 2 ** 31 and E.keep_alives(int(b[3][49]), int(b[3][50])) == 4 and E.keep_alives(int(b[3][Bk - 1]), int(b[3][Bk])) >= 2
    return a, b


@gpu
@pytest.mark.parametrize("n", ["0", "1", "2", "Bk-1", "Bk", "Bk+1", "2*Bk+3"])
def test_encoder_equals_the_model_over_sizes(recs, Bk, n):
    """row 0: n events of the bursty recording, then the n after them (the state carries a group's end); row 1: n + 1 events of the
    sparse one with int32 times.  The capacity 2 x Bk + 8 gives every row three workgroups."""
    n = eval(n, {"Bk": Bk})
    a, b = recs
    ses = _Session(2, dtypes=(torch.int64, torch.int16, torch.int32, torch.int32))
    ses.call([_cut(a, 0, n), _cut(b, 0, n + 1)], 2 * Bk + 8, tag=(n, 0))
    ses.call([_cut(a, n, min(2 * n, len(a[0]))), _cut(b, n + 1, n + 1)], 2 * Bk + 8, tag=(n, 1))
    ses.finish()
    assert ses.counters() == (0, 0, 0, 0)
    assert ses.enc.words.shape == (2, 5 * (2 * Bk + 8) + 1024)


@gpu
def test_encoder_equals_the_model_over_rows(recs, Bk):
    a, b = recs
    ses = _Session(3)
    ses.call([_cut(a, 0, 0), _cut(b, 0, 5), _cut(a, 0, Bk + 7)], Bk + 9)
    ses.call([_cut(a, 0, 3), _cut(b, 5, 5), _cut(a, Bk + 7, Bk + 30)], Bk + 9)
    assert ses.call([_cut(a, 0, 0)] * 3, 0, tag="columns without storage") == [0, 0, 0]
    assert ses.call([_cut(a, 0, 0)] * 3, 0, tag="records without storage", dat=True) == [0, 0, 0]
    ses.call([_cut(a, 3, 9), _cut(b, 5, 6), _cut(a, Bk + 30, Bk + 31)], 8)
    ses.finish()
    assert ses.counters() == (0, 0, 0, 0) and ses.models[0].have and ses.models[1].have


def _burst_row(n, at, groups):
    """n events: singles 100 us apart and, from index `at` on, the groups given as lists of x (one time, row and polarity)"""
    x = (np.arange(n) * 5) % 60
    y = (np.arange(n) * 7) % 40
    p = np.arange(n) % 2
    t = 1000 + 100 * np.arange(n)
    i = at
    for g in groups:
        x[i:i + len(g)] = g
        i += len(g)
    y[at:i], p[at:i], t[at:i] = y[at], p[at], t[at]
    return x, y, p, t


@gpu
def test_groups_that_straddle_a_workgroup_boundary(Bk):
    """2 x Bk events in a capacity of 2 x Bk: two workgroups, the boundary in front of event Bk.  One group of five events, and a
    chained pair of groups of three, placed so that the boundary falls at every position inside and around them."""
    n = 2 * Bk
    five, pair = [[13, 15, 17, 20, 23]], [[1, 5, 11], [12, 13, 20]]
    for groups, shifts in ((five, range(0, 6)), (pair, range(0, 7))):
        parts = [_burst_row(n, Bk - k, groups) for k in shifts]
        ses = _Session(len(parts))
        got = ses.call(parts, n, tag=groups)
        ses.finish()
        whole = len(E.encode(*_burst_row(n, 5, groups)))
        assert all(g == whole for g in got)                          # the pieces of a chunk are no cuts: no group ends at one
    words = E.encode(*_burst_row(40, 5, pair))
    assert ((words >> 12) == M.VECT_12).sum() == 2 and ((words >> 12) == M.VECT_BASE_X).sum() == 1      # the pair is chained


@gpu
def test_three_chunks_with_a_cut_inside_a_burst_and_reset_on_one_row(recs):
    a, b = recs
    inside = next(i for i in range(300, 600) if a[3][i] == a[3][i - 1] == a[3][i + 1] and a[1][i] == a[1][i - 1] == a[1][i + 1])
    ses = _Session(3)
    ses.call([_cut(a, 0, inside), _cut(b, 0, 100), _cut(a, 0, 50)], 700, tag=0)
    before = ses.enc.state.clone()
    ses.call([_cut(a, inside, 650), _cut(b, 100, 100), _cut(b, 0, 40)], 700, reset=[0, 1, 1], tag=1)
    assert torch.equal(ses.enc.state[0, :1], before[0, :1]) and ses.enc.state[1].tolist() == [0, 0, 0, 0]     # reset, no event: zero
    ses.call([_cut(a, 650, 900), _cut(b, 100, 300), _cut(b, 40, 90)], 700, tag=2)
    ses.enc.reset(streams=[0])                                         # the host-side form
    ses.models[0].reset()
    ses.call([_cut(a, 900, 1000), _cut(b, 300, 310), _cut(b, 90, 91)], 700, tag=3)
    ses.finish()
    # the chunks of row 0 decode to the recording whatever the cuts
    assert ses.counters() == (0, 0, 0, 0)
    ses.enc.reset()
    assert ses.enc.errors() == (0, 0, 0, 0) and int(ses.enc.state.abs().sum()) == 0


@gpu
def test_bad_input_is_normalised_and_counted(recs, Bk):
    """row 0: 2 x Bk + 3 events whose times step back in several places (one of them right at the start: the whole row is raised), with
    bursts all along: the running maximum, counted in [0].  row 1: x = 3000, y = -1, p = 5 among good events: clamped, counted in [1].
    row 2: good events.  Then a chunk whose first time lies below the carry."""
    a, b = recs
    n = 2 * Bk + 3
    x, y, p, t = (c[:n].copy() for c in a)
    t[0] = t[700]
    t[Bk - 1:Bk + 2] -= 3000
    t[n - 5] = 0
    bx, by, bp, bt = (c[:40].copy() for c in b)
    bx[3], by[4], bp[5], bx[6], bp[6] = 3000, -1, 5, -7, -1
    ses = _Session(3)
    ses.call([(x, y, p, t), (bx, by, bp, bt), _cut(b, 0, 30)], n + 5, tag="raised")
    raised, clamped, _r, _z = ses.counters()
    assert raised > 600 and clamped == 4
    ses.call([_cut(a, n, n + 20), _cut(b, 0, 12), _cut(b, 30, 60)], n + 5, tag="below the carry")
    assert ses.counters()[0] == raised + 12 and ses.counters()[1] == 4
    ses.finish()
    row = ses.enc.words[1, :int(ses.enc.n_words[1])].cpu().numpy().view(np.uint16) >> 12
    assert not ((row == M.TIME_HIGH) | (row == M.TIME_LOW)).any()      # twelve events at the carry's time: no time word at all


@gpu
def test_a_row_without_room_is_refused_whole(recs):
    a, b = recs
    def second_chunk(ev, hi):                                        # the words of events 10 .. hi behind a first chunk of 10 events
        m = E.Encoder()
        m.feed(*_cut(ev, 0, 10))
        return len(m.feed(*_cut(ev, 10, hi)))

    limit = second_chunk(b, 210) - 1
    assert second_chunk(a, 210) <= limit                             # the sparse row needs more words than the bursty ones
    ses = _Session(3, max_words=limit)
    ses.call([_cut(a, 0, 10), _cut(b, 0, 10), _cut(a, 0, 10)], 200, tag="before")
    before = ses.enc.state.clone()
    got = ses.call([_cut(a, 10, 210), _cut(b, 10, 210), _cut(a, 10, 210)], 200, tag="refused")
    assert got[1] == 0 and got[0] > 0 and got[2] > 0 and torch.equal(ses.enc.state[1], before[1])
    assert ses.enc.errors() == (0, 0, 1, 0)
    fit = next(k for k in range(210, 10, -1) if second_chunk(b, k) <= limit)
    got = ses.call([_cut(a, 210, 300), _cut(b, 10, fit), _cut(a, 210, 300)], 200, tag="after")
    assert fit >= 200 and 0 < got[1] <= limit                        # the row is taken again, a few events short of the refused chunk
    # refused under its reset flag: the reset is done, the chunk is not
    got = ses.call([_cut(a, 300, 300), _cut(b, 10, 210), _cut(a, 300, 301)], 200, reset=[0, 1, 0], tag="reset and refused")
    assert got == [0, 0, got[2]] and got[2] > 0 and ses.enc.state[1].tolist() == [0, 0, 0, 0]
    ses.finish()
    assert ses.counters() == (0, 0, 2, 0)


@gpu
def test_device_decoder_gives_the_columns_back(recs, Bk):
    from sast_amd.events import Evt3Decoder, Evt3Encoder
    a, b = recs
    n = Bk + 100
    parts = [_cut(a, 0, n), _cut(b, 0, 0), _cut(b, 0, n - 1)]
    enc, dec = Evt3Encoder(3), Evt3Decoder(3)
    at = 0
    for size in (n // 3, n // 2, n):                                 # three chunks, the decoder's state carried beside the encoder's
        cols, counts = _dev_columns([_cut(part, at, size) for part in parts], n)
        words, n_words = enc(*cols, counts)
        x, y, p, t, got_n = dec(words, n_words)
        assert torch.equal(got_n, counts)
        for s in range(3):
            k = int(counts[s])
            for got, want in zip((x, y, p, t), cols):
                assert torch.equal(got[s, :k].to(torch.int64), want[s, :k].to(torch.int64)), (size, s)
        at = size
    assert enc.errors() == (0, 0, 0, 0) and dec.errors() == (0, 0, 0)


@gpu
def test_workgroups_that_take_several_steps_round_trip(Bk):
    """more than 256 x Bk events in a row: the workgroup count stops at 256 and every workgroup takes two steps, its carries handed from
    one step to the next.  Too long for the sequential model: the device decoder must give the columns back, bursts included."""
    from sast_amd import _lib
    from sast_amd.events import Evt3Decoder, Evt3Encoder
    n = _lib.EVT3_ENC_MAX_BLOCKS * Bk + 2 * Bk + 5
    rng = np.random.RandomState(41)
    size = rng.randint(1, 7, size=n // 2)                            # groups of 1 .. 6 events of one time, row and polarity
    group = np.repeat(np.arange(len(size)), size)[:n]
    first = np.concatenate([[0], np.cumsum(size)[:-1]])
    t = (100 + np.cumsum(rng.randint(0, 40, size=len(size))))[group]
    y, p = rng.randint(0, 720, size=len(size))[group], rng.randint(0, 2, size=len(size))[group]
    x = rng.randint(0, 1200, size=len(size))[group] + 2 * (np.arange(n) - first[group])       # ascending inside a group, over 12-boundaries
    assert len(t) == n and int(t[-1]) < 2 ** 24
    parts = [(x, y, p, t), tuple(c[:Bk + 1] for c in (x, y, p, t))]
    cols, counts = _dev_columns(parts, n)
    enc, dec = Evt3Encoder(2), Evt3Decoder(2, max_events=n)
    words, n_words = enc(*cols, counts)
    got = dec(words, n_words)
    assert torch.equal(got[4], counts) and enc.errors() == (0, 0, 0, 0) and dec.errors() == (0, 0, 0)
    assert 2 * n > int(n_words[0]) > n // 2 and ((words[0, :int(n_words[0])] >> 12) & 0xF == M.VECT_12).sum() > n // 8
    for s in range(2):
        k = int(counts[s])
        for g, c in zip(got[:4], cols):
            assert torch.equal(g[s, :k].to(torch.int64), c[s, :k].to(torch.int64)), s
    assert enc.state.cpu().tolist() == [[1, int(t[-1]), int(y[-1]), 0], [1, int(t[Bk]), int(y[Bk]), 0]]


@gpu
def test_packed_records_give_the_words_of_the_columns(recs, Bk):
    a, b = recs
    n = Bk + 9
    ses_c, ses_d = _Session(2), _Session(2)
    for k, (lo, hi) in enumerate(((0, 300), (300, n))):
        parts = [_cut(a, lo, hi), _cut(b, lo, hi - 1)]
        ses_c.call(parts, n, tag=("columns", k))
        ses_d.call(parts, n, tag=("records", k), dat=True)
        assert torch.equal(ses_c.enc.n_words, ses_d.enc.n_words) and torch.equal(ses_c.enc.state, ses_d.enc.state)
        for s in range(2):
            assert torch.equal(ses_c.enc.words[s, :int(ses_c.enc.n_words[s])], ses_d.enc.words[s, :int(ses_d.enc.n_words[s])])
    # x, y up to 16383 in a record: clamped to 2047 like a column's
    ses_d.call([(np.array([16383, 5]), np.array([2, 9000]), np.array([1, 0]), np.array([2 ** 31 + 5, 2 ** 32 - 1])), _cut(b, 0, 0)], n,
               reset=[1, 0], tag="wide", dat=True)
    ses_d.finish()
    assert ses_d.counters() == (0, 2, 0, 0)


@gpu
def test_push_evt3_of_the_words_gives_the_frames_of_push_of_the_columns():
    from sast_amd.events import EventQueue, Evt3Encoder
    S = 3
    kw = dict(bins=2, duration_us=2000, **GEO)
    evs = [M.recording(31, 2500, t_step=12, **GEO), M.recording(32, 0, **GEO), M.recording(33, 1700, t_step=16, bursts=0.7, **GEO)]
    ends = torch.tensor([[2000 * (k + 1)] * S for k in range(5)], dtype=torch.int64).cuda()
    ref, q, enc = EventQueue(S, 4096, **kw), EventQueue(S, 4096, **kw), Evt3Encoder(S)
    for lo, hi in ((0, 900), (900, 2500)):
        cols, counts = _dev_columns([_cut(ev, lo, hi) for ev in evs], 1600)
        ref.push(*cols, counts)
        words, n_words = enc(*cols, counts)
        q.push_evt3(words, n_words)
    assert q.count.cpu().tolist() == [2500, 0, 1700] and torch.equal(q.count, ref.count) and torch.equal(q.t_last, ref.t_last)
    want, got = ref.frames(ends), q.frames(ends)
    assert int(want[:, 0].count_nonzero()) > 0 and got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert q.errors() == ref.errors() == (0, 0, 0, 0) and q.evt3_errors() == (0, 0, 0) and enc.errors() == (0, 0, 0, 0)


@gpu
def test_a_captured_call_replays_on_new_events_and_counts(recs, Bk):
    from sast_amd import _lib
    from sast_amd.events import Evt3Encoder
    a, b = recs
    cap = Bk + 50
    steps = [([_cut(a, 0, 400), _cut(b, 0, 0), _cut(b, 0, cap)], [0, 0, 0]),
             ([_cut(a, 400, 400 + cap), _cut(b, 0, 7), _cut(b, cap, cap + 3)], [0, 0, 0]),
             ([_cut(a, 0, 90), _cut(b, 7, 500), _cut(b, cap + 3, cap + 3)], [1, 0, 0]),
             ([_cut(a, 90, 91), _cut(b, 500, 501), _cut(a, 0, cap)], [0, 0, 1])]
    cols, counts = _dev_columns(steps[0][0], cap)
    rst = torch.zeros(3, dtype=torch.uint8).cuda()
    ses = _Session(3)
    enc, lib = ses.enc, _lib.lib()
    for _ in range(2):                                               # the first call allocates; the launches are the same
        before = lib.sast_launch_count()
        enc(*cols, counts, rst)
        assert lib.sast_launch_count() - before == ENCODE_LAUNCHES == enc.ENCODE_LAUNCHES
        enc.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc(*cols, counts, rst)
    torch.cuda.current_stream().wait_stream(side)
    enc.reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        words, n_words = enc(*cols, counts, rst)
    enc.reset()
    for k, (parts, reset) in enumerate(steps):
        new_cols, new_counts = _dev_columns(parts, cap)
        for dst, src in zip(cols + [counts, rst], new_cols + [new_counts, torch.tensor(reset, dtype=torch.uint8)]):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        ses.check(words, n_words, ses.expect(parts, reset, words.shape[1]), ("replay", k))
    ses.finish()
