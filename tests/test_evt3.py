"""Raw EVT 3.0 sensor words on the device (sast_amd.events.Evt3Decoder, EventQueue.push_evt3, OnlineDetector.push_evt3; the sast_evt3_*
entry points of csrc/k_evt3.hip).

The decoder is held, call by call, to the sequential model of tests/evt3_model.py: events, their order, the counts, the three counters
and the state after every chunk.  The CPU tests hold the model to its encoder and to itself over every cut of a stream.  Everything is
integers: there is no tolerance.  Every chunk row carries stale words that would give events past its count; S = 3 rows, the middle
one with a count of 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import evt3_model as M  # noqa: E402

gpu = pytest.mark.gpu

S = 3
DECODE_LAUNCHES, PUSH_EVT3_LAUNCHES = 2, 4        # summaries, decode; + the queue's partial maxima, scan + append
W = M.word
STALE = W(M.ADDR_X, 0x805)                        # what lies past a row's count: it would be an event
TH, TL, AY, AX, BX, V12, V8 = M.TIME_HIGH, M.TIME_LOW, M.ADDR_Y, M.ADDR_X, M.VECT_BASE_X, M.VECT_12, M.VECT_8

# hand-written streams: every position of each is a cut in the CPU and in the GPU test
HAND = {
    # VECT_BASE_X | VECT_12 | VECT_12 of one base | VECT_8 with its ignored high bits; TIME_HIGH | TIME_LOW; ADDR_Y (bit 11 set) | events
    "vectors": [W(TH, 5), W(TL, 100), W(AY, 7 | 0x800), W(BX, 100 | 0x800), W(V12, 0xFFF), W(V12, 0x805), W(V8, 0xF81), W(TH, 6), W(TL, 3),
                W(AY, 9), W(AX, 50), W(AX, 51 | 0x800), W(V12, 0x002), W(BX, 7), W(V8, 0x0FF), W(AX, 2047 | 0x800)],
    # the wrap threshold: a TIME_HIGH 2047 below its predecessor is taken as written, 2048 below is a wrap; then a second wrap
    "wraps": [W(TH, 3000), W(AX, 1), W(TH, 953), W(AX, 2), W(TH, 3001), W(TL, 9), W(AX, 3), W(TH, 953), W(AX, 4), W(TH, 4095), W(AX, 5),
              W(TH, 0), W(TL, 0), W(AX, 6)],
    # events before the first TIME_HIGH (single and vector) are counted, not given; state set before it still holds after it
    "before_high": [W(TL, 77), W(AY, 5), W(AX, 9), W(BX, 20 | 0x800), W(V12, 0x00F), W(V8, 0x003), W(TH, 1), W(AX, 10), W(V12, 0x001)],
    "time_only": [W(TH, 10), W(TL, 5), W(TL, 6), W(TH, 11), W(TH, 12), W(TL, 4095), W(TH, 4000), W(TH, 100), W(TL, 1)],
    # every type code, the unknown ones (0x1, 0x9, 0xB, 0xC, 0xD) and the valid ones without effect (0x7, 0xA, 0xE, 0xF)
    "codes": [W(TH, 2)] + [W(tc, 0xABC) for tc in range(16)] + [W(AX, 3)] + [W(tc, 0x123) for tc in (1, 9, 0xB, 0xC, 0xD, 7, 0xA, 0xE, 0xF)],
}
HAND = {k: np.array(v, np.uint16) for k, v in HAND.items()}


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_model_round_trips_the_encoder_through_three_clock_wraps():
    ev = M.recording(1, 3000, t_end=int(6.6 * 2 ** 24))
    words = M.encode(*ev, seed=2)
    types = set((words >> 12).tolist())
    assert {TH, TL, AY, AX, BX, V12, V8} <= types and types & set(M.IGNORED) and not types & set(M.UNKNOWN)
    got, counters, state = M.decode(words)
    assert all(np.array_equal(a, b) for a, b in zip(got, ev))
    assert counters == (0, 0) and int(ev[3][-1]) >> 24 == 3 and state[5] == 3 and state[6] == 1
    highs = (words[(words >> 12) == TH] & 0xFFF).astype(np.int64)
    assert (np.diff(highs) % 4096 <= 1024).all()                     # the keep-alives
    # the same recording batch by batch through one encoder decodes to the same events
    enc = M.Encoder(5)
    parts = [enc.feed(*(c[a:a + 170] for c in ev)) for a in range(0, 3000, 170)]
    got, counters, _state = M.decode(np.concatenate(parts))
    assert all(np.array_equal(a, b) for a, b in zip(got, ev)) and counters == (0, 0)


def test_model_is_invariant_to_a_cut_at_every_word():
    streams = dict(HAND, encoded=M.encode(*M.recording(3, 150, t_end=int(2.5 * 2 ** 24)), seed=4))
    for name, words in streams.items():
        whole = M.decode(words)
        for k in range(len(words) + 1):
            cut = M.decode(words, cuts=[k])
            assert all(np.array_equal(a, b) for a, b in zip(cut[0], whole[0])), (name, k)
            assert cut[1] == whole[1] and np.array_equal(cut[2], whole[2]), (name, k)
    rng = np.random.RandomState(0)
    words = streams["encoded"]
    for _ in range(20):                                              # several cuts at once, empty pieces included
        cuts = rng.randint(0, len(words) + 1, size=rng.randint(2, 9))
        cut, whole = M.decode(words, cuts=cuts), M.decode(words)
        assert all(np.array_equal(a, b) for a, b in zip(cut[0], whole[0])) and cut[1:2] == whole[1:2] and np.array_equal(cut[2], whole[2])


def test_model_on_hand_written_words():
    (x, y, p, t), counters, state = M.decode(HAND["vectors"])
    t0, t1 = 5 * 4096 + 100, 6 * 4096 + 3
    assert x.tolist() == list(range(100, 112)) + [112, 114, 123] + [124, 131] + [50, 51, 133, 7, 8, 9, 10, 11, 12, 13, 14, 2047]
    assert y.tolist() == [7] * 17 + [9] * 12 and p.tolist() == [1] * 17 + [0, 1, 1] + [0] * 8 + [1]      # y bit 11 ignored
    assert t.tolist() == [t0] * 17 + [t1] * 12 and counters == (0, 0)
    assert state.tolist() == [9, 15, 0, 3, 6, 0, 1, 0]
    (x, _y, _p, t), counters, state = M.decode(HAND["wraps"])
    w = 1 << 24
    assert x.tolist() == [1, 2, 3, 4, 5, 6] and counters == (0, 0)
    assert t.tolist() == [3000 * 4096, 953 * 4096, 3001 * 4096 + 9, w + 953 * 4096 + 9, w + 4095 * 4096 + 9, 2 * w]
    assert state.tolist() == [0, 0, 0, 0, 0, 2, 1, 0]
    (x, y, p, t), counters, state = M.decode(HAND["before_high"])
    assert counters == (1 + 4 + 2, 0) and x.tolist() == [10, 40] and y.tolist() == [5, 5] and p.tolist() == [0, 1]
    assert t.tolist() == [4096 + 77] * 2 and state.tolist() == [5, 52, 1, 77, 1, 0, 1, 0]
    (x, *_), counters, state = M.decode(HAND["time_only"])
    assert len(x) == 0 and counters == (0, 0) and state.tolist() == [0, 0, 0, 1, 100, 1, 1, 0]
    (x, y, p, t), counters, state = M.decode(HAND["codes"])
    # the sixteen codes with v = 0xABC after TIME_HIGH 2: y = 0x2BC, one event x = 0x2BC p = 1, base 0x2BC pol 1, VECT_12 0xABC (7 bits),
    # VECT_8 0xBC (5 bits), low = 0xABC, TIME_HIGH 0xABC
    assert counters == (0, 5 + 5) and len(x) == 1 + 7 + 5 + 1
    assert x[0] == 0x2BC and p[0] == 1 and x[1:8].tolist() == [0x2BC + i for i in range(12) if 0xABC >> i & 1]
    assert x[8:13].tolist() == [0x2BC + 12 + i for i in range(8) if 0xBC >> i & 1] and (y == 0x2BC).all()
    assert t[:13].tolist() == [2 * 4096] * 13 and t[13] == 0xABC * 4096 + 0xABC and x[13] == 3 and p[13] == 0
    assert state.tolist() == [0x2BC, 0x2BC + 20, 1, 0xABC, 0xABC, 0, 1, 0]
    # base_x runs past 2047 and past int16: x is stored with saturation
    words = np.array([W(TH, 1), W(BX, 2040)] + [W(V12, 0x801)] * 2600, np.uint16)
    (x, *_), _c, state = M.decode(words)
    assert x[:4].tolist() == [2040, 2051, 2052, 2063] and x.max() == 32767 and (np.diff(x) >= 0).all() and state[1] == 2040 + 12 * 2600


def test_evt3_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_evt3_")]
    assert sorted(names) == ["sast_evt3_decode", "sast_evt3_ws_bytes"]
    lib = _lib.lib()
    P = C.c_void_p
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert _lib._SIGNATURES["sast_evt3_decode"] == (C.c_int, [P, P, C.c_int64, C.c_int, P, P, P, P, P, P, P, C.c_int64, P, P, P])
    assert _lib._SIGNATURES["sast_evt3_ws_bytes"] == (C.c_size_t, [C.c_int])
    assert (_lib.EVT3_STATE_WORDS, _lib.EVT3_BLOCK_WORDS, _lib.EVT3_MAX_BLOCKS) == (8, 2048, 256)
    for n_streams in (1, 3, 65535):
        assert lib.sast_evt3_ws_bytes(n_streams) == n_streams * (_lib.EVT3_MAX_BLOCKS + 1) * 40
    assert lib.sast_evt3_ws_bytes(0) == 0 and lib.sast_evt3_ws_bytes(-1) == 0 and lib.sast_evt3_ws_bytes(65536) == 0


def test_evt3_decode_rejects_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib = _lib.lib()
    p = 0x1000
    good = dict(words=p, counts=p, chunk_words=256, S=3, reset=None, state=p, ws=p, x=p, y=p, p=p, t=p, max_events=3072, out_counts=p, err=p)

    def call(**kw):
        a = dict(good, **kw)
        return lib.sast_evt3_decode(*[a[k] for k in good], None)

    for name in ("words", "counts", "state", "ws", "x", "y", "p", "t", "out_counts", "err"):
        assert call(**{name: None}) == -22, name
    for kw in (dict(S=0), dict(S=65536), dict(chunk_words=-1), dict(chunk_words=2 ** 31 // 12 + 1), dict(S=8, chunk_words=2 ** 28),
               dict(max_events=0), dict(max_events=-4), dict(max_events=2 ** 30), dict(words=p + 1), dict(ws=p + 2)):
        assert call(**kw) == -22, kw


def test_evt3_python_argument_validation(monkeypatch):
    from sast_amd.events import EventQueue, Evt3Decoder
    from sast_amd.online import OnlineDetector
    with pytest.raises(ValueError, match="num_streams"):
        Evt3Decoder(0)
    with pytest.raises(ValueError, match="max_events"):
        Evt3Decoder(3, 0)
    with pytest.raises(ValueError, match="2\\^31"):
        Evt3Decoder(3, 2 ** 30)
    dec = Evt3Decoder(S)
    assert dec.errors() == (0, 0, 0) and dec.DECODE_LAUNCHES == DECODE_LAUNCHES and dec.state is None
    dec.reset()
    dec.reset(streams=[1])
    q = EventQueue(S, 64, 48, 64, duration_us=1000)
    assert q.evt3_errors() == (0, 0, 0) and q.PUSH_EVT3_LAUNCHES == PUSH_EVT3_LAUNCHES and q.errors() == (0, 0, 0, 0)

    class _Det:
        training = False

        class yolox_head:
            num_classes = 2

    od = OnlineDetector(_Det(), q, windows_per_step=2)
    words, counts = torch.zeros(S, 16, dtype=torch.int16), torch.zeros(S, dtype=torch.int64)
    for push in (dec, q.push_evt3, od.push_evt3):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            push(words, counts)
        if hasattr(torch, "uint16"):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                push(words.view(torch.uint16), counts)
        for bad in (torch.int32, torch.uint8, torch.int64, torch.float16):
            with pytest.raises(TypeError, match="int16"):
                push(words.to(bad), counts)
        with pytest.raises(ValueError, match="num_streams=3"):
            push(words[:2], counts)
        with pytest.raises(ValueError, match="num_streams=3"):
            push(words[:, :, None], counts)
        with pytest.raises(ValueError, match="contiguous"):
            push(words.t().contiguous().t(), counts)
        with pytest.raises(ValueError, match="counts"):
            push(words, counts.to(torch.int32))
        with pytest.raises(ValueError, match="counts"):
            push(words, counts[:2])
        with pytest.raises(ValueError, match="reset"):
            push(words, counts, torch.zeros(S, dtype=torch.int32))
        with pytest.raises(ValueError, match="reset"):
            push(words, counts, torch.zeros(S + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="final"):
        od.push_evt3(words, counts, None, torch.zeros(S, dtype=torch.int64))
    assert dec.state is None and q.evt3 is not None and q.evt3.state is None        # nothing was allocated on the way
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="un-captured"):                          # the state and the staging are never born in a capture
        dec._buffers(torch.device("cpu"), 16)
    assert dec.state is None and dec.x is None


# ---------------------------------------------------------------------------------------------------------------------------- GPU

def _dev_words(parts, cap):
    """per-row word arrays -> (int16 [S, cap] with stale event words past each count, counts int64 [S]) on the device"""
    buf = np.full((len(parts), cap), STALE, np.uint16)
    for s, part in enumerate(parts):
        buf[s, :len(part)] = part
    return torch.from_numpy(buf.view(np.int16)).cuda(), torch.tensor([len(part) for part in parts], dtype=torch.int64).cuda()


class _Session:
    """a device decoder beside one model per row: every `call` decodes one chunk per row on both and compares all of it"""

    def __init__(self, max_events=None):
        from sast_amd.events import Evt3Decoder
        self.dec = Evt3Decoder(S, max_events)
        self.models = [M.Decoder() for _ in range(S)]
        self.dropped = self.events = 0

    def call(self, parts, cap=None, reset=None, tag=None):
        cap = max(len(part) for part in parts) + 3 if cap is None else cap
        words, counts = _dev_words(parts, cap)
        rst = None if reset is None else torch.tensor(reset, dtype=torch.uint8).cuda()
        x, y, p, t, n = self.dec(words, counts, rst)
        limit = x.shape[1]
        assert x.dtype == y.dtype == p.dtype == torch.int16 and t.dtype == n.dtype == torch.int64 and tuple(n.shape) == (S,)
        got_n = n.cpu().tolist()
        got = [c.cpu().numpy() for c in (x, y, p, t)]
        for s, part in enumerate(parts):
            if reset is not None and reset[s]:
                self.models[s].reset()
            want = self.models[s].feed(part)
            keep = min(len(want[0]), limit)
            self.dropped += len(want[0]) - keep
            self.events += keep
            assert got_n[s] == keep, (tag, s, got_n[s], keep)
            for name, g, w in zip("xypt", got, want):
                assert np.array_equal(g[s, :keep].astype(np.int64), w[:keep]), (tag, s, name)
        assert np.array_equal(self.dec.state.cpu().numpy(), np.stack([m.state() for m in self.models])), tag
        return got_n

    def counters(self):
        return sum(m.before_high for m in self.models), sum(m.unknown for m in self.models), self.dropped

    def finish(self):
        assert self.dec.errors() == self.counters()


@pytest.fixture(scope="module")
def streams():
    """two encoded recordings through clock wraps (rows 0 and 2), and a long one for the chunks that span several workgroups"""
    a = M.encode(*M.recording(11, 900, t_end=int(4.4 * 2 ** 24)), seed=12)
    b = M.encode(*M.recording(13, 700, t_end=int(2.2 * 2 ** 24), bursts=0.6), seed=14, others=0.3)
    long = M.encode(*M.recording(15, 30000, t_start=5000, t_step=30), seed=16)
    assert len(a) > 1800 and len(b) > 1200 and len(long) > 40000
    return a, b, long


@gpu
@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 255, 256, 257])
def test_decoder_equals_the_model_over_chunk_lengths(streams, length):
    """row 0 in chunks of `length` words, row 2 in chunks of length + 2 of another stream (shorter: its last chunks are empty), row 1
    never gets a word"""
    a, b, _long = streams
    if length <= 2:
        a, b = a[:300], b[:200]
    ses = _Session()
    cap = length + 7 if length % 2 else length + 6                    # odd lengths: rows not 16-byte aligned; even: capacity % 8 varies
    for k in range((len(a) + length - 1) // length):
        ses.call([a[k * length:(k + 1) * length], a[:0], b[k * (length + 2):(k + 1) * (length + 2)]], cap, tag=(length, k))
    ses.finish()
    assert ses.events > 150 and ses.counters() == (0, 0, 0) and (length <= 2 or ses.models[0].wraps >= 2)


@gpu
@pytest.mark.parametrize("cap", [3 * 2048, 3 * 2048 - 3])
def test_decoder_equals_the_model_when_a_row_spans_several_workgroups(streams, cap):
    """capacity 3 x 2048 words: three workgroups per row, pieces of ceil(n / 3) words rounded up to 8.  The counts put the last piece at
    one word, at none and at full, a piece's end inside a thread's 8 words, and n at the capacity and one below; the capacity that is
    no multiple of 8 takes the loads word by word."""
    from sast_amd import _lib
    _a, b, long = streams
    assert _lib.EVT3_BLOCK_WORDS == 2048 and -(-cap // _lib.EVT3_BLOCK_WORDS) == 3
    lengths = [8, 9, 16, 17, 24, 25, 2047, 2048, 2049, 4095, 4096, 4097, cap - 7, cap - 1, cap]
    assert sum(lengths) <= len(long)
    ses, at, bt = _Session(), 0, 0
    for k, n in enumerate(lengths):
        m = lengths[-1 - k] % 1000                                    # row 2: other counts, below one workgroup's piece
        ses.call([long[at:at + n], long[:0], b[bt:bt + m]], cap, tag=(cap, n))
        at, bt = at + n, bt + m
    ses.finish()
    assert ses.events > 10000 and ses.counters() == (0, 0, 0)


@gpu
def test_decoder_equals_the_model_when_workgroups_take_several_steps():
    """more than 256 x 2048 words in a row: the workgroup count stops at 256 and every workgroup takes two steps.  Random words of every
    type; the staging holds the row's events exactly."""
    from sast_amd import _lib
    n = _lib.EVT3_MAX_BLOCKS * _lib.EVT3_BLOCK_WORDS + 4096 + 5
    rng = np.random.RandomState(21)
    codes = np.array([M.OTHERS, TL, AY, AX, BX, V12, V8, TH, 0x9], np.int64)
    tc = codes[rng.choice(len(codes), p=[.55, .15, .05, .08, .04, .04, .03, .05, .01], size=n)]
    v = rng.randint(0, 4096, size=n)
    hi = tc == TH
    v[hi] = (np.cumsum(rng.randint(0, 3, size=int(hi.sum()))) + 5) & 0xFFF          # a clock that climbs through its wraps
    words = ((tc << 12) | v).astype(np.uint16)
    other = HAND["vectors"]
    total = len(M.decode(words)[0][0])
    ses = _Session(max_events=total)
    ses.call([words, words[:0], other], n + 3)
    ses.finish()
    assert ses.events == total + 29 and ses.counters()[1] > 1000 and ses.counters()[2] == 0 and ses.models[0].wraps >= 2


@gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_decoder_equals_the_model_at_every_cut_of_the_hand_written_streams(name):
    """a cut between VECT_BASE_X and VECT_12, between two VECT_12 of one base, between TIME_HIGH and TIME_LOW, right after ADDR_Y, in
    front of and behind a wrap of TIME_HIGH, inside a chunk of only time words and between unknown codes: every position.  Row 0 takes
    the stream in two chunks (with its reset flag set for the first), row 2 whole and then nothing."""
    words = HAND[name]
    ses = _Session()
    for k in range(len(words) + 1):
        ses.call([words[:k], words[:0], words], 32, reset=[1, 0, 1], tag=(name, k, 0))
        ses.call([words[k:], words[:0], words[:0]], 32, tag=(name, k, 1))
    ses.finish()
    want = M.decode(words)
    assert ses.counters() == (2 * (len(words) + 1) * want[1][0], 2 * (len(words) + 1) * want[1][1], 0)
    assert np.array_equal(ses.models[0].state(), want[2]) and np.array_equal(ses.models[2].state(), want[2])


@gpu
def test_full_vectors_fill_the_staging_exactly_and_five_too_many_are_counted():
    head = np.array([W(TH, 3), W(TL, 9), W(AY, 4), W(BX, 0 | 0x800)], np.uint16)
    full = np.full(40, W(V12, 0xFFF), np.uint16)                       # fan-out 12: 480 events from 40 words
    for short in (0, 5):
        ses = _Session(max_events=480 - short)
        ses.call([head, head[:0], head], 8)
        n = ses.call([full, full[:0], full[:13]], 40)
        assert n == [480 - short, 0, 156]
        ses.finish()
        assert ses.counters() == (0, 0, short) and ses.dec.x.shape == (S, 480 - short)
        x = ses.dec.x[0, :480 - short].cpu().tolist()
        assert x == list(range(480 - short))                            # the FIRST events are the ones kept
    ses = _Session()                                                    # the default staging, 12 x the chunk's words, never drops
    ses.call([head, head[:0], head], 40)
    ses.call([full, full[:0], full], 40)
    ses.finish()
    assert ses.dec.x.shape == (S, 480) and ses.counters() == (0, 0, 0)


@gpu
def test_reset_on_one_row_only(streams):
    a, b, _long = streams
    ses = _Session()
    cut = 400 + next(i for i, w in enumerate(b[400:]) if (int(w) >> 12) in (AX, V12, V8))     # row 2 starts over in front of an event
    ses.call([a[:500], a[:0], b[:cut]], 512)
    before = [m.state().copy() for m in ses.models]
    ses.call([a[500:900], a[:0], b[cut:700]], 512, reset=[0, 1, 1], tag="reset")
    # row 2 started over in the middle of its stream: its events up to the next TIME_HIGH are counted, row 0 lost nothing
    assert ses.counters()[0] > 0 and ses.models[0].before_high == 0 and ses.models[0].wraps >= before[0][5]
    ses.call([a[900:1300], a[:0], b[700:1000]], 512)
    ses.dec.reset(streams=[0])                                          # the host-side form
    ses.models[0].reset()
    ses.call([a[1300:1700], a[:0], b[1000:1200]], 512, tag="host reset")
    ses.finish()
    ses.dec.reset()
    assert ses.dec.errors() == (0, 0, 0) and int(ses.dec.state.abs().sum()) == 0


@gpu
def test_decode_launch_counts_equal_the_class_constants(streams):
    from sast_amd import _lib
    from sast_amd.events import EventQueue, Evt3Decoder
    a, _b, long = streams
    lib = _lib.lib()
    assert (Evt3Decoder.DECODE_LAUNCHES, EventQueue.PUSH_EVT3_LAUNCHES) == (DECODE_LAUNCHES, PUSH_EVT3_LAUNCHES)
    for n_streams, cap in ((1, 64), (3, 5000), (8, 20000)):
        words, counts = _dev_words([long[:cap - s] for s in range(n_streams)], cap)
        dec = Evt3Decoder(n_streams)
        q = EventQueue(n_streams, 12 * cap + 8, 48, 64, duration_us=1000)
        for _ in range(2):                                              # the first calls allocate; the count is the same
            before = lib.sast_launch_count()
            dec(words, counts)
            assert lib.sast_launch_count() - before == DECODE_LAUNCHES, (n_streams, cap)
            before = lib.sast_launch_count()
            q.push_evt3(words, counts)
            assert lib.sast_launch_count() - before == PUSH_EVT3_LAUNCHES, (n_streams, cap)
            q.reset()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the queue

GEO = dict(height=48, width=64)
Q_KW = dict(bins=2, duration_us=2000, **GEO)


def _columns(parts, cap):
    cols = [np.full((len(parts), cap), g, np.int64) for g in (5, 5, 1, 123)]
    for s, part in enumerate(parts):
        for c, a in zip(cols, part):
            c[s, :len(a)] = a
    return [torch.from_numpy(c).cuda() for c in cols], torch.tensor([len(part[0]) for part in parts], dtype=torch.int64).cuda()


@pytest.fixture(scope="module")
def recordings():
    recs = [M.recording(31, 2500, t_step=12, **GEO), M.recording(32, 0, **GEO), M.recording(33, 1700, t_step=16, bursts=0.7, **GEO)]
    return recs, [M.encode(*r, seed=40 + s) for s, r in enumerate(recs)]


@gpu
def test_push_evt3_gives_the_frames_of_push_on_the_original_events(recordings):
    from sast_amd.events import EventQueue
    recs, words = recordings
    ends = torch.tensor([[2000 * (k + 1)] * S for k in range(5)], dtype=torch.int64).cuda()
    ref = EventQueue(S, 4096, **Q_KW)
    cols, counts = _columns(recs, 2500)
    ref.push(*cols, counts)
    stored = {name: getattr(ref, name).clone() for name in ("x", "y", "p", "t")}        # before `frames` retires and moves rows
    want = ref.frames(ends)
    assert int(want[:, 0].count_nonzero()) > 0 and int(want[:, 2].count_nonzero()) > 0 and ref.errors() == (0, 0, 0, 0)
    for chunk in (97, 256, 1000):
        q = EventQueue(S, 4096, **Q_KW)
        for k in range(max(-(-len(w) // chunk) for w in words)):
            w, n = _dev_words([w[k * chunk:(k + 1) * chunk] for w in words], chunk)
            q.push_evt3(w, n)
        assert q.count.cpu().tolist() == [2500, 0, 1700]
        for name in ("x", "y", "p", "t"):
            assert all(torch.equal(getattr(q, name)[s, :len(recs[s][0])], stored[name][s, :len(recs[s][0])]) for s in range(S)), (chunk, name)
        got = q.frames(ends)
        assert got.dtype == torch.uint8 and torch.equal(got, want), chunk
        assert q.errors() == (0, 0, 0, 0) and q.evt3_errors() == (0, 0, 0)
        assert torch.equal(q.t_last, ref.t_last)


@gpu
def test_columns_past_the_sensor_are_counted_invalid_and_never_drawn():
    """base_x runs past the sensor's 64 columns, past 2047 and past int16: those events are stored with x outside the sensor, `frames`
    counts them invalid and draws none of them (x = 32767 + 1 must not come back as a column)"""
    from sast_amd.events import EventQueue
    words = np.array([W(TH, 0), W(TL, 50), W(AY, 10), W(BX, 56), W(V12, 0xFFF), W(AY, 11), W(BX, 2040)] + [W(V12, 0x801)] * 2800, np.uint16)
    (x, y, p, t), _c, state = M.decode(words)
    assert (x < 64).sum() == 8 and x.max() == 32767 and state[1] > 32767 + 64
    q, ref = EventQueue(S, 8192, **Q_KW), EventQueue(S, 8192, **Q_KW)
    w, n = _dev_words([words, words[:0], words[:5]], len(words))
    q.push_evt3(w, n, torch.ones(S, dtype=torch.uint8).cuda())
    assert q.x[0, :len(x)].cpu().tolist() == x.tolist() and int(q.count[0]) == len(x)
    empty = tuple(x[:0] for _ in range(4))
    cols, counts = _columns([(x, y, p, t), empty, (x[:12], y[:12], p[:12], t[:12])], len(x))
    ref.push(*cols, counts)
    ends = torch.tensor([[2000] * S], dtype=torch.int64).cuda()
    got, want = q.frames(ends), ref.frames(ends)
    assert torch.equal(got, want) and int(got[0, 0].sum()) == 8 and int(got[0, 2].sum()) == 8
    assert q.errors() == ref.errors() == (len(x) - 8 + 4, 0, 0, 0) and q.evt3_errors() == (0, 0, 0)


@gpu
def test_captured_push_evt3_and_frames_replay_on_new_words_like_the_eager_run(recordings):
    from sast_amd.events import EventQueue
    recs, words = recordings
    chunk = 1200
    steps = []
    for k in range(4):
        parts = [w[k * chunk:(k + 1) * chunk] for w in words]
        if k == 2:
            parts[2] = words[0][:700]                                  # row 2 starts another recording with its reset flag
        steps.append((parts, [0, 0, int(k == 2)], [[1000 * (2 * k + 1)] * S, [1000 * (2 * k + 2)] * S]))     # a chunk of row 0 spans about 2000 us
    w, n = _dev_words(steps[0][0], chunk)
    rst, ends = torch.zeros(S, dtype=torch.uint8).cuda(), torch.zeros(2, S, dtype=torch.int64).cuda()

    def load(step):
        nw, nn = _dev_words(step[0], chunk)
        w.copy_(nw), n.copy_(nn), rst.copy_(torch.tensor(step[1], dtype=torch.uint8)), ends.copy_(torch.tensor(step[2], dtype=torch.int64))

    def call(q):
        q.push_evt3(w, n, rst)
        return q.frames(ends)

    eager, qe = [], EventQueue(S, 8192, **Q_KW)
    for step in steps:
        load(step)
        fr = call(qe)
        eager.append((fr.clone(), qe.count.clone(), qe.t_last.clone(), qe.evt3.state.clone()))
    assert int(eager[3][0].count_nonzero()) > 0 and not torch.equal(eager[0][0], eager[1][0]) and qe.evt3_errors()[1:] == (0, 0)
    q = EventQueue(S, 8192, **Q_KW)
    load(steps[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(q)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_fr = call(q)
    q.reset()
    for step, (fr, count, t_last, state) in zip(steps, eager):
        load(step)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_fr, fr) and torch.equal(q.count, count) and torch.equal(q.t_last, t_last) and torch.equal(q.evt3.state, state)
    assert q.errors() == qe.errors() and q.evt3_errors() == qe.evt3_errors()


# ------------------------------------------------------------------------------------------------------------------ the detector

@pytest.fixture(scope="module")
def detector():
    """the small detector of tests/test_online_detector.py"""
    import test_online_detector as T
    from oracle import sast_oracle as O
    from sast_amd.config import backbone_config, to_attr
    from sast_amd.detection import YoloXDetector
    hw, part, E, nc = (128, 160), (4, 5), 32, 2
    cfg = to_attr({"backbone": backbone_config(hw, part, embed_dim=E, AMP=2e-2, ls_init_value=0.5),
                   "fpn": {"name": "PAFPN", "depth": 0.67, "in_stages": [2, 3, 4], "depthwise": False, "act": "silu"},
                   "head": {"name": "YoloX", "depthwise": False, "act": "silu", "num_classes": nc}})
    det = YoloXDetector(cfg).cuda()
    T._load(det.backbone, O.init_backbone_params(O.BackboneCfg(in_res_hw=hw, partition_size=part, embed_dim=E, amp=2e-2), seed=41, ls_init=0.5))
    T._load(det.fpn, O.init_pafpn_params((64, 128, 256), seed=42))
    T._load(det.yolox_head, O.init_head_params((64, 128, 256), num_classes=nc, seed=43))
    with torch.no_grad():
        for m in det.yolox_head.obj_preds:
            m.bias.fill_(2.0)
        for m in det.yolox_head.cls_preds:
            m.bias.fill_(0.0)
    return det.eval()


@gpu
def test_online_detector_push_evt3_gives_the_records_of_push(detector):
    """the same event chunks, as columns into one OnlineDetector and as sensor words (each chunk through the row's encoder) into another:
    the same records, byte for byte, push by push, eager and then replayed from a graph; row 1 starts a second recording on the way"""
    from sast_amd.events import EventQueue
    from sast_amd.online import OnlineDetector
    geo, D, chunk, wcap = dict(height=128, width=160), 600, 300, 1024
    recs = [M.recording(51 + s, 1500, t_start=40, t_step=step, **geo) for s, step in enumerate((16, 8, 8))]
    second = M.recording(57, 600, t_start=20, t_step=8, **geo)
    encs = [M.Encoder(61 + s) for s in range(S)]
    rng = np.random.RandomState(7)
    rounds, cur, src = [], [0] * S, list(recs)
    for r in range(8):
        reset, final = np.zeros(S, np.uint8), np.zeros(S, np.uint8)
        if r == 4:
            src[1], cur[1], encs[1], reset[1] = second, 0, M.Encoder(71), 1
        if r == 7:
            final[2] = 1
        parts = []
        for s in range(S):
            hi = min(len(src[s][0]), cur[s] + int(rng.randint(0, chunk + 1)))
            parts.append(tuple(c[cur[s]:hi] for c in src[s]))
            cur[s] = hi
        rounds.append((parts, [encs[s].feed(*parts[s]) for s in range(S)], reset, final))
    assert max(len(w) for _p, ws, _r, _f in rounds for w in ws) <= wcap

    def make():
        return OnlineDetector(detector, EventQueue(S, 8192, duration_us=D, **geo), windows_per_step=2, max_det=100, conf_thre=0.45,
                              nms_thre=0.45)

    def same(got, want):
        assert [s for s, _a in got] == [s for s, _a in want]
        assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for (_s, a), (_t, b) in zip(got, want))

    od_cols, od_words, od_graph = make(), make(), make()
    w, n = _dev_words(rounds[0][1], wcap)
    rst, fin = torch.zeros(S, dtype=torch.uint8).cuda(), torch.zeros(S, dtype=torch.uint8).cuda()
    n_records = n_windows = 0
    for r, (parts, words, reset, final) in enumerate(rounds):
        cols, counts = _columns(parts, chunk)
        od_cols.push(*cols, counts, torch.from_numpy(reset).cuda(), torch.from_numpy(final).cuda())
        want = od_cols.drain()
        nw, nn = _dev_words(words, wcap)
        od_words.push_evt3(nw, nn, torch.from_numpy(reset).cuda(), torch.from_numpy(final).cuda())
        same(od_words.drain(), want)
        w.copy_(nw), n.copy_(nn), rst.copy_(torch.from_numpy(reset)), fin.copy_(torch.from_numpy(final))
        if r == 0:
            od_graph.push_evt3(w, n, rst, fin)
            od_graph.capture()
        else:
            od_graph.replay()
        same(od_graph.drain(), want)
        n_records += sum(len(a) for _s, a in want)
        n_windows += len(want)
    assert n_records > 0 and n_windows >= 6
    for other in (od_words, od_graph):
        assert other.errors() == od_cols.errors() and other.queue.evt3_errors() == (0, 0, 0)
        for (h, c), (h2, c2) in zip(other.states, od_cols.states):
            assert torch.equal(h, h2) and torch.equal(c, c2)
