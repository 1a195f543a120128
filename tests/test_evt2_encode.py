"""Events -> raw EVT 2.0 / EVT 2.1 sensor words on the device (sast_amd.events.Evt2Encoder, evt2_raw_header; the sast_evt2enc_* entry
points of csrc/k_evt2_enc.hip).

The CPU tests hold the sequential model of the canonical rule (tests/evt2_encoder_model.py) to the decoder's model (tests/evt2_model.py):
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
import evt2_encoder_model as E  # noqa: E402
import evt2_model as M  # noqa: E402

gpu = pytest.mark.gpu

ENCODE_LAUNCHES = 2
GEO = dict(height=48, width=64)
VERSIONS = M.VERSIONS
GAPS = (2 ** 32 + 5, 3 * 2 ** 32 + 2 ** 31, 2 ** 34 - 7)              # silences that need keep-alives and cross wraps of the 34-bit clock
WORD_TORCH = {M.V20: torch.int32, M.V21: torch.int64}


def recording(seed, n, height=48, width=64, t_start=100, t_step=40, bursts=0.3):
    """n events: non-decreasing times from t_start (mean step t_step / 2), single pixels and, with probability `bursts`, runs of
    2 .. 40 events of one time, row and polarity on ascending columns that start anywhere: a run crosses multiples of 32 and can be
    longer than one EVT 2.1 word -> int64 x, y, p, t"""
    rng = np.random.RandomState(seed)
    xs, ys, ps, ts = [], [], [], []
    t = t_start
    while len(ts) < n:
        t += int(rng.randint(0, t_step + 1))
        yy, pp = int(rng.randint(height)), int(rng.randint(2))
        if rng.rand() < bursts:
            x0 = int(rng.randint(0, width - 1))
            span = min(int(rng.randint(2, 49)), width - x0)
            cols = x0 + np.sort(rng.choice(span, size=min(int(rng.randint(2, 41)), span), replace=False))
        else:
            cols = [int(rng.randint(width))]
        for c in cols:
            xs.append(int(c)), ys.append(yy), ps.append(pp), ts.append(t)
    return tuple(np.array(c[:n], np.int64) for c in (xs, ys, ps, ts))


def _keep_alives(t, t_first_prev=None):
    prev = np.concatenate([[t[0] if t_first_prev is None else t_first_prev], t[:-1]])
    gap = (t >> 6) - (prev >> 6)
    return int(np.where(gap > 0, (gap - 1) // E.KEEP_STEPS, 0).sum())


def _round_trip(ev, version, cuts=()):
    """the events through the encoder's model (in chunks cut at `cuts`) and the decoder's model: every event back, no event before the
    first TIME_HIGH, no unknown word, at most 2 words per event plus the keep-alives, only TIME_HIGH and event words -> the words"""
    x, y, p, t = ev
    words = E.encode(x, y, p, t, version, cuts=cuts)
    assert words.dtype == M.WORD_DTYPE[version]
    got, counters, _state = M.decode(words, version)
    base = (int(t[0]) >> 34) << 34 if len(t) else 0                  # a fresh decoder starts its wraps at 0
    assert counters == (0, 0)
    for name, g, w in zip("xypt", got, (x, y, p, t - base)):
        assert np.array_equal(g, w), name
    assert len(words) <= 2 * len(t) + _keep_alives(t)
    codes = (words >> np.array(M.WORD_BITS[version] - 4, words.dtype)).astype(np.int64)
    assert set(codes.tolist()) <= {M.CD_OFF, M.CD_ON, M.TIME_HIGH}
    if version == M.V20:
        assert (codes <= M.CD_ON).sum() == len(t)
    else:
        ev_words = words[codes <= M.CD_ON]
        assert ((ev_words >> np.uint64(43)) & np.uint64(31) == 0).all() and (ev_words & np.uint64(0xFFFFFFFF) != 0).all()     # aligned bases
    return words


# ---------------------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("kw,rate21", [(dict(bursts=0.0), (1.0, 2.0)), (dict(bursts=0.9, t_step=4), (0.0, 0.5))], ids=["sparse", "bursts"])
def test_model_round_trips_sparse_and_burst_streams(version, kw, rate21):
    for seed in range(4):
        ev = recording(100 + seed, 3000 - 400 * seed, **kw)
        words = _round_trip(ev, version)
        rate = len(words) / len(ev[0])
        assert (1.0 < rate <= 2.0) if version == M.V20 else (rate21[0] <= rate <= rate21[1]), rate
        rng = np.random.RandomState(seed)
        _round_trip(ev, version, cuts=rng.randint(0, len(ev[0]) + 1, size=7))


@pytest.mark.parametrize("version", VERSIONS)
def test_model_round_trips_keep_alive_gaps_and_clock_wraps(version):
    ev = recording(1, 400, bursts=0.4)
    at = 0
    for k, gap in enumerate(GAPS):                                   # each silence in front of event 100 * (k + 1)
        at = 100 * (k + 1)
        ev[3][at:] += gap
    assert _keep_alives(ev[3]) in (6, 7) and int(ev[3][-1]) >> 34 == 2       # 0 or 1 (2^26 steps and a bit), 3 and 3 of them
    words = _round_trip(ev, version)
    shift = M.WORD_BITS[version] - 4
    highs = np.array([(int(w) >> (shift - 28)) & M.HIGH_MASK for w in words.tolist() if int(w) >> shift == M.TIME_HIGH], np.int64)
    steps = np.diff(highs) % (1 << 28)
    assert ((1 <= steps) & (steps <= 1 << 26)).all()                 # the decoder sees every wrap of the 28 bits exactly once
    assert M.decode(words, version)[2].tolist() == [(int(ev[3][-1]) >> 6) & M.HIGH_MASK, 2, 1, 0]
    _round_trip(ev, version, cuts=[1])
    _round_trip(ev, version, cuts=[100, 200, 201])                   # cuts right at a silence: the state carries the time in front
    _round_trip(ev, version, cuts=[137, 301, 302])


@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("t_start", [2 ** 35 + 12345, 2 ** 34 - 1000])
def test_model_first_event_beyond_the_34_bit_clock(version, t_start):
    ev = recording(3, 500, t_start=t_start, t_step=9, bursts=0.0)
    words = _round_trip(ev, version)                                 # _round_trip subtracts (t0 >> 34) << 34
    assert int(words[0]) == M.time_high(version, (int(ev[3][0]) >> 6) & M.HIGH_MASK)
    got, _c, state = M.decode(words, version)
    assert got[3][0] == int(ev[3][0]) - ((t_start >> 34) << 34) and state[1] == (int(ev[3][-1]) >> 34) - (int(ev[3][0]) >> 34)
    assert state[1] == (1 if t_start < 2 ** 34 else 0)               # 2^34 - 1000: the stream itself crosses the wrap


@pytest.mark.parametrize("version", VERSIONS)
def test_model_gives_the_events_back_at_every_cut_of_a_stream(version):
    ev = recording(4, 120, bursts=0.8, t_step=3000)
    whole = E.encode(*ev, version)
    lengths = set()
    for k in range(121):
        words = _round_trip(ev, version, cuts=[k])
        lengths.add(len(words))
        for k2 in (k // 2, min(k + 3, 120)):
            _round_trip(ev, version, cuts=[k, k2])
    assert len(whole) == min(lengths)
    assert (len(lengths) > 1) == (version == M.V21)                  # a cut ends a group: the words of 2.1 depend on the cuts


def _np(*cols):
    return tuple(np.array(c, np.int64) for c in cols)


def test_model_on_hand_written_events():
    two = _np([5, 6], [7, 7], [1, 1], [100, 100])
    assert E.encode(*two, M.V20).tolist() == [0x80000001, 0x19002807, 0x19003007]
    assert E.encode(*two, M.V21).tolist() == [0x8000000100000000, 0x1900000700000060]
    # 33 columns 31 .. 63 of one time, row and polarity: column 31 ends the first block of 32, columns 32 .. 63 fill a whole word
    run = _np(np.arange(31, 64), [9] * 33, [0] * 33, [64 * 5 + 3] * 33)
    assert E.encode(*run, M.V21).tolist() == [M.time_high(M.V21, 5), M.cd(M.V21, 0, 3, 0, 9, 1 << 31), M.cd(M.V21, 0, 3, 32, 9, 0xFFFFFFFF)]
    assert E.encode(*run, M.V21, cuts=[20]).tolist() == [M.time_high(M.V21, 5), M.cd(M.V21, 0, 3, 0, 9, 1 << 31),
                                                         M.cd(M.V21, 0, 3, 32, 9, (1 << 19) - 1), M.cd(M.V21, 0, 3, 32, 9, 0xFFFFFFFF ^ ((1 << 19) - 1))]
    words20 = E.encode(*run, M.V20).tolist()
    assert words20 == [M.time_high(M.V20, 5)] + [M.cd(M.V20, 0, 3, c, 9) for c in range(31, 64)]
    # what ends a group: a column that does not ascend, another row, polarity or time
    mixed = _np([40, 41, 41, 42, 43, 44, 45], [1, 1, 1, 1, 2, 2, 2], [1, 1, 1, 1, 1, 0, 0], [70, 70, 70, 70, 70, 70, 71])
    assert E.encode(*mixed, M.V21).tolist() == [M.time_high(M.V21, 1), M.cd(M.V21, 1, 6, 32, 1, 3 << 8), M.cd(M.V21, 1, 6, 32, 1, 3 << 9),
                                                M.cd(M.V21, 1, 6, 32, 2, 1 << 11), M.cd(M.V21, 0, 6, 32, 2, 1 << 12),
                                                M.cd(M.V21, 0, 7, 32, 2, 1 << 13)]
    for version in VERSIONS:
        # keep-alives: H goes from 1 to 1 + 3 * 2^26 + 1: floor((3 * 2^26 + 1 - 1) / 2^26) = 3 of them, the last 1 step in front of H;
        # one step less and there are 2, the last 2^26 steps in front of H
        TH, K = (lambda v: M.time_high(version, v)), 1 << 26
        gap = _np([1, 2, 3], [4, 4, 4], [0, 1, 1], [64, 64 * (2 + 3 * K) + 9, 64 * (2 + 3 * K) + 64 * (3 * K) + 10])
        assert E.encode(*gap, version).tolist() == [
            TH(1), M.cd(version, 0, 0, 1 if version == M.V20 else 0, 4, 1 << 1),
            TH(1 + K), TH(1 + 2 * K), TH(1 + 3 * K), TH(2 + 3 * K), M.cd(version, 1, 9, 2 if version == M.V20 else 0, 4, 1 << 2),
            TH((2 + 4 * K) & M.HIGH_MASK), TH((2 + 5 * K) & M.HIGH_MASK), TH((2 + 6 * K) & M.HIGH_MASK),
            M.cd(version, 1, 10, 3 if version == M.V20 else 0, 4, 1 << 3)]
        assert M.decode(E.encode(*gap, version), version)[0][3].tolist() == gap[3].tolist()
        # bad input: nothing is dropped, every change is counted
        enc = E.Encoder(version)
        words = enc.feed([3000, 1, -4], [2, 5000, 2], [5, 0, -1], [50, 40, 60])
        got, _c, _s = M.decode(words, version)
        assert [g.tolist() for g in got] == [[2047, 1, 0], [2, 2047, 2], [1, 0, 1], [50, 50, 60]]
        assert (enc.raised, enc.clamped, enc.refused) == (1, 3, 0) and enc.state().tolist() == [1, 60, 0, 0]
        assert len(enc.feed([1] * 4, [1] * 4, [0] * 4, [70, 80, 90, 200], max_words=5)) == 0         # 2 + 1 + 1 + 2 words: refused
        assert (enc.raised, enc.clamped, enc.refused) == (1, 3, 1) and enc.state().tolist() == [1, 60, 0, 0]
        assert len(enc.feed([1] * 4, [1] * 4, [0] * 4, [70, 80, 90, 200], max_words=6)) == 6


@pytest.mark.parametrize("version", VERSIONS)
def test_raw_header_round_trips(version):
    from sast_amd.events import evt2_raw_header, raw_header
    for h, w in ((720, 1280), (48, 64), (1, 2048)):
        head = evt2_raw_header(h, w, version)
        assert isinstance(head, bytes) and head.startswith(b"% ") and head.endswith(b"% end\n")
        assert all(line.startswith(b"% ") for line in head.splitlines())
        words = E.encode(*recording(5, 40, height=min(h, 48), width=min(w, 64)), version)
        le = "<u4" if version == M.V20 else "<u8"
        got = raw_header(head + words.astype(le).tobytes())
        assert (got.format, got.height, got.width, got.offset) == ("evt2" if version == M.V20 else "evt21", h, w, len(head))
        assert np.array_equal(np.frombuffer((head + words.astype(le).tobytes())[got.offset:], le), words)
        assert raw_header(head + b"%").offset == len(head)           # a data byte 0x25 right behind the header is data
    assert evt2_raw_header(48, 64) == evt2_raw_header(48, 64, "2.0")
    for bad in ((0, 64), (48, 0), (2049, 64), (48, 4096)):
        with pytest.raises(ValueError, match="2048"):
            evt2_raw_header(*bad, version)
    with pytest.raises(ValueError, match="version"):
        evt2_raw_header(48, 64, "3.0")


def test_encode_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_evt2enc_")]
    assert sorted(names) == ["sast_evt2enc_encode", "sast_evt2enc_encode_dat", "sast_evt2enc_ws_bytes"]
    lib = _lib.lib()
    P = C.c_void_p
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert _lib._SIGNATURES["sast_evt2enc_encode"] == (C.c_int, [P, P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int64, C.c_int, C.c_int,
                                                                 P, P, P, P, C.c_int64, P, P, P])
    assert _lib._SIGNATURES["sast_evt2enc_encode_dat"] == (C.c_int, [P, P, C.c_int64, C.c_int, C.c_int, P, P, P, P, C.c_int64, P, P, P])
    assert (_lib.EVT2_ENC_STATE_WORDS, _lib.EVT2_ENC_BLOCK_EVENTS, _lib.EVT2_ENC_MAX_BLOCKS) == (4, 1024, 256)
    for n_streams in (1, 3, 65535):
        assert lib.sast_evt2enc_ws_bytes(n_streams) == n_streams * (_lib.EVT2_ENC_MAX_BLOCKS + 1) * 32
    assert lib.sast_evt2enc_ws_bytes(0) == 0 and lib.sast_evt2enc_ws_bytes(65536) == 0
    import sast_amd.events as ev
    assert ev.Evt2Encoder.ENCODE_LAUNCHES == ENCODE_LAUNCHES and callable(ev.evt2_raw_header)


def test_encode_rejects_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib = _lib.lib()
    q = 0x1000
    for version, word_bytes in ((_lib.EVT2_V20, 4), (_lib.EVT2_V21, 8)):
        common = dict(counts=q, chunk_events=256, S=3, version=version, reset=None, state=q, ws=q, words=q, max_words=2304, n_words=q, err=q)
        cols = dict(x=q, y=q, p=q, t=q, x_dtype=_lib.DT_I16, y_dtype=_lib.DT_I32, p_dtype=_lib.DT_I64, t_dtype=_lib.DT_I64, **common)
        dat = dict(records=q, **common)
        for fn, good in ((lib.sast_evt2enc_encode, cols), (lib.sast_evt2enc_encode_dat, dat)):

            def call(**kw):
                a = dict(good, **kw)
                return fn(*[a[k] for k in good], None)

            for name in [k for k, v in good.items() if v == q]:
                assert call(**{name: None}) == -22, name
            for kw in (dict(S=0), dict(S=65536), dict(chunk_events=-1), dict(S=8, chunk_events=2 ** 28), dict(max_words=0),
                       dict(max_words=-4), dict(max_words=2 ** 30), dict(version=2), dict(version=-1), dict(words=q + word_bytes // 2),
                       dict(words=q + 1), dict(ws=q + 4)):
                assert call(**kw) == -22, kw
        for kw in (dict(x_dtype=_lib.DT_F32), dict(y_dtype=_lib.DT_U8), dict(p_dtype=99), dict(t_dtype=_lib.DT_I16),
                   dict(t_dtype=_lib.EVQUEUE_DT_DAT)):
            a = dict(cols, **kw)
            assert lib.sast_evt2enc_encode(*[a[k] for k in cols], None) == -22, kw
        assert lib.sast_evt2enc_encode_dat(*[dict(dat, records=q + 4)[k] for k in dat], None) == -22


def test_encoder_python_argument_validation(monkeypatch):
    from sast_amd.events import Evt2Encoder
    S = 3
    with pytest.raises(ValueError, match="num_streams"):
        Evt2Encoder(0)
    with pytest.raises(ValueError, match="max_words"):
        Evt2Encoder(3, 0)
    with pytest.raises(ValueError, match="2\\^31"):
        Evt2Encoder(3, 2 ** 30)
    for bad in ("3.0", 2.0, None, "evt2"):
        with pytest.raises(ValueError, match="version"):
            Evt2Encoder(3, version=bad)
    assert Evt2Encoder(3).version == "2.0"
    for version in VERSIONS:
        enc = Evt2Encoder(S, version=version)
        assert enc.errors() == (0, 0, 0, 0) and enc.ENCODE_LAUNCHES == ENCODE_LAUNCHES and enc.state is None and enc.version == version
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
        assert enc.state is None and enc.words is None              # nothing was allocated on the way
        with monkeypatch.context() as mp:
            mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
            with pytest.raises(RuntimeError, match="un-captured"):  # the state and the staging are never born in a capture
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

    def __init__(self, S, version, max_words=None, dtypes=DTYPES):
        from sast_amd.events import Evt2Encoder
        self.S, self.dtypes, self.version = S, dtypes, version
        self.enc = Evt2Encoder(S, max_words, version)
        self.models = [E.Encoder(version) for _ in range(S)]

    def expect(self, parts, reset, limit):
        want = []
        for s, part in enumerate(parts):
            if reset is not None and reset[s]:
                self.models[s].reset()
            want.append(self.models[s].feed(*part, max_words=limit))
        return want

    def check(self, words, n, want, tag):
        assert words.dtype == WORD_TORCH[self.version] and n.dtype == torch.int64 and tuple(n.shape) == (self.S,) and words.shape[0] == self.S
        got_n, got = n.cpu().tolist(), words.cpu().numpy().view(M.WORD_DTYPE[self.version])
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
    return _lib.EVT2_ENC_BLOCK_EVENTS


@pytest.fixture(scope="module")
def recs(Bk):
    """a bursty recording (runs over multiples of 32 all along) and a sparse one with keep-alive gaps, each longer than 2 x Bk + 3
    events; both fit the 32-bit times of a DAT record"""
    a = recording(21, 2 * Bk + 40, bursts=0.5, t_step=30, **GEO)
    b = recording(22, 2 * Bk + 40, bursts=0.05, t_step=9000, height=720, width=1280)
    a[3].setflags(write=False), b[3].setflags(write=False)
    return a, b


@gpu
@pytest.mark.parametrize("dat", [False, True], ids=["columns", "records"])
@pytest.mark.parametrize("version", VERSIONS)
@pytest.mark.parametrize("n", ["0", "1", "2", "Bk-1", "Bk", "Bk+1", "2*Bk+3"])
def test_encoder_equals_the_model_over_sizes(recs, Bk, n, version, dat):
    """row 0: n events of the bursty recording, then the n after them (the state carries the time in front); row 1: n + 1 events of the
    sparse one with int32 times.  The capacity 2 x Bk + 8 gives every row three workgroups."""
    n = eval(n, {"Bk": Bk})
    a, b = recs
    ses = _Session(2, version, dtypes=(torch.int64, torch.int16, torch.int32, torch.int32))
    ses.call([_cut(a, 0, n), _cut(b, 0, n + 1)], 2 * Bk + 8, tag=(n, 0), dat=dat)
    ses.call([_cut(a, n, min(2 * n, len(a[0]))), _cut(b, n + 1, n + 1)], 2 * Bk + 8, tag=(n, 1), dat=dat)
    ses.finish()
    assert ses.counters() == (0, 0, 0, 0)
    assert ses.enc.words.shape == (2, 2 * (2 * Bk + 8) + 16)


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_encoder_equals_the_model_over_rows_and_dtypes(recs, Bk, version):
    a, b = recs
    for dtypes in ((torch.int16, torch.int32, torch.int64, torch.int64), (torch.int64, torch.int16, torch.int32, torch.int32),
                   (torch.int32, torch.int64, torch.int16, torch.int64)):
        ses = _Session(3, version, dtypes=dtypes)
        ses.call([_cut(a, 0, 0), _cut(b, 0, 5), _cut(a, 0, Bk + 7)], Bk + 9)
        ses.call([_cut(a, 0, 3), _cut(b, 5, 5), _cut(a, Bk + 7, Bk + 30)], Bk + 9)
        assert ses.call([_cut(a, 0, 0)] * 3, 0, tag="columns without storage") == [0, 0, 0]
        assert ses.call([_cut(a, 0, 0)] * 3, 0, tag="records without storage", dat=True) == [0, 0, 0]
        ses.call([_cut(a, 3, 9), _cut(b, 5, 6), _cut(a, Bk + 30, Bk + 31)], 8)
        ses.finish()
        assert ses.counters() == (0, 0, 0, 0) and ses.models[0].have and ses.models[1].have


def _burst_row(n, at, cols):
    """n events: singles 100 us apart and, from index `at` on, a run of one time, row and polarity on the columns `cols`"""
    x = (np.arange(n) * 5) % 60
    y = (np.arange(n) * 7) % 40
    p = np.arange(n) % 2
    t = 1000 + 100 * np.arange(n)
    x[at:at + len(cols)] = cols
    y[at:at + len(cols)], p[at:at + len(cols)], t[at:at + len(cols)] = y[at], p[at], t[at]
    return x, y, p, t


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_groups_of_32_that_straddle_a_workgroup_boundary(Bk, version):
    """A full group, columns 64 .. 95 (its last member exactly 31 events ahead of its leader), between two shorter ones; its leader at
    Bk - 33 .. Bk + 1.  2 x Bk events in a capacity of 2 x Bk: two workgroups, the piece boundary in front of event Bk.  (A workgroup
    takes a second step only in a row of more than 256 x Bk events: test_workgroups_that_take_several_steps_round_trip.)"""
    n = 2 * Bk
    cols = list(range(40, 64, 3)) + list(range(64, 96)) + [96, 99, 127]
    parts = [_burst_row(n, Bk - 8 - k, cols) for k in range(33, -2, -1)]
    whole = len(E.encode(*parts[0], version))
    assert whole == 2 * (n - len(cols) + 1) + (2 if version == M.V21 else len(cols) - 1)      # a TIME_HIGH per time; the run: 3 / 43 words
    for lo in range(0, len(parts), 12):
        ses = _Session(len(parts[lo:lo + 12]), version)
        got = ses.call(parts[lo:lo + 12], n, tag=lo)
        ses.finish()
        assert all(g == whole for g in got)                          # the pieces of a chunk are no cuts: no group ends at one


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_three_chunks_with_a_cut_inside_a_burst_and_reset_on_one_row(recs, version):
    a, b = recs
    inside = next(i for i in range(300, 600) if a[3][i] == a[3][i - 1] == a[3][i + 1] and a[1][i] == a[1][i - 1] == a[1][i + 1]
                  and a[0][i - 1] >> 5 == a[0][i] >> 5 == a[0][i + 1] >> 5)
    ses = _Session(3, version)
    ses.call([_cut(a, 0, inside), _cut(b, 0, 100), _cut(a, 0, 50)], 700, tag=0)
    before = ses.enc.state.clone()
    ses.call([_cut(a, inside, 650), _cut(b, 100, 100), _cut(b, 0, 40)], 700, reset=[0, 1, 1], tag=1)
    assert torch.equal(ses.enc.state[0, :1], before[0, :1]) and ses.enc.state[1].tolist() == [0, 0, 0, 0]     # reset, no event: zero
    ses.call([_cut(a, 650, 900), _cut(b, 100, 300), _cut(b, 40, 90)], 700, tag=2)
    ses.enc.reset(streams=[0])                                         # the host-side form
    ses.models[0].reset()
    ses.call([_cut(a, 900, 1000), _cut(b, 300, 310), _cut(b, 90, 91)], 700, tag=3)
    ses.finish()
    assert ses.counters() == (0, 0, 0, 0)
    ses.enc.reset()
    assert ses.enc.errors() == (0, 0, 0, 0) and int(ses.enc.state.abs().sum()) == 0


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_bad_input_is_normalised_and_counted(recs, Bk, version):
    """row 0: 2 x Bk + 3 events whose times step back in several places (one of them right at the start: the whole row is raised), with
    bursts all along: the running maximum, counted in [0], the row walked by one workgroup.  row 1: x = 3000, y = -1, p = 2 among good
    events: clamped, counted in [1].  row 2: int64 times with the keep-alive silences of GAPS.  Then a chunk whose first time lies
    below the carry."""
    a, b = recs
    n = 2 * Bk + 3
    x, y, p, t = (c[:n].copy() for c in a)
    t[0] = t[700]
    t[Bk - 1:Bk + 2] -= 3000
    t[n - 5] = 0
    bx, by, bp, bt = (c[:40].copy() for c in b)
    bx[3], by[4], bp[5], bx[6], bp[6] = 3000, -1, 2, -7, -1
    g = tuple(c[:Bk + 30].copy() for c in a)
    for k, gap in enumerate(GAPS):
        g[3][(Bk - 2, Bk, Bk + 9)[k]:] += gap                        # silences around the piece boundary
    ses = _Session(3, version)
    ses.call([(x, y, p, t), (bx, by, bp, bt), g], n + 5, tag="raised")
    raised, clamped, _r, _z = ses.counters()
    assert raised > 600 and clamped == 4
    words = ses.enc.words[2, :int(ses.enc.n_words[2])].cpu().numpy().view(M.WORD_DTYPE[version])
    assert (words >> np.array(M.WORD_BITS[version] - 4, words.dtype) == M.TIME_HIGH).sum() >= 7 + 3     # the keep-alives are there
    ses.call([_cut(a, n, n + 20), _cut(b, 0, 12), _cut(a, 0, 9)], n + 5, tag="below the carry")
    assert ses.counters()[0] == raised + 12 + 9 and ses.counters()[1] == 4
    ses.finish()


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_a_row_without_room_is_refused_whole(recs, version):
    a, b = recs

    def second_chunk(ev, hi):                                        # the words of events 10 .. hi behind a first chunk of 10 events
        m = E.Encoder(version)
        m.feed(*_cut(ev, 0, 10))
        return len(m.feed(*_cut(ev, 10, hi)))

    limit = second_chunk(b, 210) - 1
    assert second_chunk(a, 210) <= limit                             # the sparse row needs more words than the bursty ones
    ses = _Session(3, version, max_words=limit)
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
@pytest.mark.parametrize("version", VERSIONS)
def test_device_decoder_gives_the_columns_back(recs, Bk, version):
    from sast_amd.events import Evt2Decoder, Evt2Encoder
    a, b = recs
    n = Bk + 100
    parts = [_cut(a, 0, n), _cut(b, 0, 0), _cut(b, 0, n - 1)]
    enc, dec = Evt2Encoder(3, version=version), Evt2Decoder(3, max_events=n, version=version)
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


def _count_words(ev, version):
    """the words of a sorted, valid row on a fresh encoder, without keep-alives: the rule restated over whole columns"""
    x, y, p, t = ev
    lead = np.ones(len(t), bool)
    if version == M.V21:
        lead[1:] = ~((t[1:] == t[:-1]) & (y[1:] == y[:-1]) & (p[1:] == p[:-1]) & (x[:-1] < x[1:]) & (x[:-1] >> 5 == x[1:] >> 5))
    high = np.ones(len(t), bool)
    high[1:] = (t[1:] >> 6) > (t[:-1] >> 6)
    return int(lead.sum() + (lead & high).sum())


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_workgroups_that_take_several_steps_round_trip(Bk, version):
    """more than 256 x Bk events in a row: the workgroup count stops at 256 and every workgroup takes two steps, its carries handed from
    one step to the next.  In the pieces 0 .. 33 a full group of 32 has its leader 0 .. 33 events in front of the piece's step boundary.
    Too long for the sequential model: the device decoder must give the columns back, and the number of words is that of the rule
    restated over whole columns (a group split at a step would give one more)."""
    from sast_amd import _lib
    from sast_amd.events import Evt2Decoder, Evt2Encoder
    n = _lib.EVT2_ENC_MAX_BLOCKS * Bk + 2 * Bk + 5
    per = ((n + 255) // 256 + 3) // 4 * 4                            # the events of a workgroup's piece
    assert Bk < per < 2 * Bk
    rng = np.random.RandomState(41)
    size = rng.randint(1, 41, size=n // 8)                           # groups of 1 .. 40 events of one time, row and polarity
    group = np.repeat(np.arange(len(size)), size)[:n]
    first = np.concatenate([[0], np.cumsum(size)[:-1]])
    t = (100 + np.cumsum(rng.randint(0, 40, size=len(size))))[group]
    y, p = rng.randint(0, 720, size=len(size))[group], rng.randint(0, 2, size=len(size))[group]
    x = rng.randint(0, 1200, size=len(size))[group] + 2 * (np.arange(n) - first[group])       # ascending inside a group, over 32-boundaries
    for k in range(34):
        at = k * per + Bk - k
        x[at:at + 32], y[at:at + 32], p[at:at + 32], t[at:at + 32] = np.arange(64, 96), 700 + k, 1, t[at]
    assert len(t) == n and int(t[-1]) < 2 ** 31 and (np.diff(t) >= 0).all()
    parts = [(x, y, p, t), tuple(c[:Bk + 1] for c in (x, y, p, t))]
    cols, counts = _dev_columns(parts, n)
    enc, dec = Evt2Encoder(2, version=version), Evt2Decoder(2, max_events=n, version=version)
    words, n_words = enc(*cols, counts)
    got = dec(words, n_words)
    assert torch.equal(got[4], counts) and enc.errors() == (0, 0, 0, 0) and dec.errors() == (0, 0, 0)
    assert n_words.cpu().tolist() == [_count_words(part, version) for part in parts]
    assert (n < int(n_words[0]) <= n + len(size)) if version == M.V20 else (n // 16 < int(n_words[0]) < n // 4)
    for s in range(2):
        k = int(counts[s])
        for g, c in zip(got[:4], cols):
            assert torch.equal(g[s, :k].to(torch.int64), c[s, :k].to(torch.int64)), s
    assert enc.state.cpu().tolist() == [[1, int(t[-1]), 0, 0], [1, int(t[Bk]), 0, 0]]


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_packed_records_give_the_words_of_the_columns(recs, Bk, version):
    a, b = recs
    n = Bk + 9
    ses_c, ses_d = _Session(2, version), _Session(2, version)
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
@pytest.mark.parametrize("version", VERSIONS)
def test_push_evt2_of_the_words_gives_the_frames_of_push_of_the_columns(version):
    from sast_amd.events import EventQueue, Evt2Encoder
    S = 3
    kw = dict(bins=2, duration_us=2000, **GEO)
    evs = [recording(31, 2500, t_step=8, **GEO), recording(32, 0, **GEO), recording(33, 1700, t_step=30, bursts=0.7, **GEO)]
    ends = torch.tensor([[2000 * (k + 1)] * S for k in range(5)], dtype=torch.int64).cuda()
    ref, q, enc = EventQueue(S, 4096, **kw), EventQueue(S, 4096, **kw), Evt2Encoder(S, version=version)
    for lo, hi in ((0, 900), (900, 2500)):
        cols, counts = _dev_columns([_cut(ev, lo, hi) for ev in evs], 1600)
        ref.push(*cols, counts)
        words, n_words = enc(*cols, counts)
        q.push_evt2(words, n_words, max_events=1600, version=version)
    assert q.count.cpu().tolist() == [2500, 0, 1700] and torch.equal(q.count, ref.count) and torch.equal(q.t_last, ref.t_last)
    want, got = ref.frames(ends), q.frames(ends)
    assert int(want[:, 0].count_nonzero()) > 0 and got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert q.errors() == ref.errors() == (0, 0, 0, 0) and q.evt2_errors() == (0, 0, 0) and enc.errors() == (0, 0, 0, 0)


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_a_captured_call_replays_on_new_events_and_counts(recs, Bk, version):
    from sast_amd import _lib
    a, b = recs
    cap = Bk + 50
    steps = [([_cut(a, 0, 400), _cut(b, 0, 0), _cut(b, 0, cap)], [0, 0, 0]),
             ([_cut(a, 400, 400 + cap), _cut(b, 0, 7), _cut(b, cap, cap + 3)], [0, 0, 0]),
             ([_cut(a, 0, 90), _cut(b, 7, 500), _cut(b, cap + 3, cap + 3)], [1, 0, 0]),
             ([_cut(a, 90, 91), _cut(b, 500, 501), _cut(a, 0, cap)], [0, 0, 1])]
    cols, counts = _dev_columns(steps[0][0], cap)
    rst = torch.zeros(3, dtype=torch.uint8).cuda()
    ses = _Session(3, version)
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
