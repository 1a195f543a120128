"""Raw EVT 2.0 and EVT 2.1 sensor words on the device (sast_amd.events.Evt2Decoder, EventQueue.push_evt2, OnlineDetector.push_evt2; the
sast_evt2_* entry points of csrc/k_evt2.hip), and sast_amd.events.raw_header.

The decoder is held, call by call, to the sequential model of tests/evt2_model.py: events, their order, the counts, the three counters
and the state after every chunk.  The CPU tests hold the model to its encoder and to itself over every cut of a stream.  Everything is
integers: there is no tolerance.  Every chunk row carries stale words that would give events past its count; S = 3 rows, the middle
one with a count of 0.  Parity with the Metavision SDK's decoder is unpinned: the model is what is pinned."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import evt2_model as M  # noqa: E402
import evt3_model as M3  # noqa: E402  (its `recording` generator)
from sast_amd import _lib as L  # noqa: E402

gpu = pytest.mark.gpu

S = 3
DECODE_LAUNCHES, PUSH_EVT2_LAUNCHES = 2, 4        # summaries, decode; + the queue's partial maxima, scan + append
VERSIONS = M.VERSIONS
PT, BW, MAXB = L.EVT2_THREAD_WORDS, L.EVT2_BLOCK_WORDS, L.EVT2_MAX_BLOCKS      # a thread's, a workgroup's words; workgroups per row
WAVE = 64 * PT                                                                  # a wave's words
TORCH_DTYPE = {M.V20: torch.int32, M.V21: torch.int64}
SIGNED = {M.V20: np.int32, M.V21: np.int64}
STALE = {v: M.cd(v, 1, 5, 5, 5, 0x805) for v in VERSIONS}                       # what lies past a row's count: it would be events
H27 = 1 << 27


def _hand(v):
    """hand-written streams: every position of each is a cut in the CPU and in the GPU test"""
    TH, EV, W = (lambda h: M.time_high(v, h)), (lambda *a: M.cd(v, *a)), (lambda tc, pay: M.word(v, tc, pay))
    pay = 0x0ABCDEF if v == M.V20 else (0x0ABCDEF << 32) | 0x80000001
    hand = {
        # events before the first TIME_HIGH are counted, not given
        "before_high": [EV(1, 3, 10, 20), EV(0, 4, 11, 21, 0x7), TH(1), EV(1, 5, 12, 22), EV(0, 63, 2047, 2047)],
        # a TIME_HIGH lower by exactly 2^27 wraps; one lower by 2^27 - 1 steps back; the field's own wrap from its top to 0
        "wraps": [TH(H27 + 5), EV(1, 1, 1, 1), TH(5), EV(1, 2, 2, 1), TH(H27 + 4), EV(0, 3, 3, 1), TH(5), EV(0, 4, 4, 1),
                  TH(M.HIGH_MASK), EV(1, 63, 5, 1), TH(0), EV(1, 0, 6, 1)],
        "time_only": [TH(10), TH(11), TH(11), TH(H27 + 11), TH(3), TH(2), TH(M.HIGH_MASK)],
        # every type code, the unknown ones and the valid ones without effect, twice
        "codes": [TH(2)] + [W(tc, pay) for tc in range(16)] + [EV(0, 1, 3, 4)] + [W(tc, 0x123) for tc in M.UNKNOWN + M.IGNORED],
    }
    if v == M.V21:
        # valid == 0 gives nothing; a full vector; x_base = 2047 with bit 31 set: x = 2078
        hand["vectors"] = [TH(7), EV(1, 9, 100, 50, 0), EV(1, 9, 64, 50, 0xFFFFFFFF), EV(0, 10, 2047, 2047, 0x80000001),
                           EV(1, 11, 0, 0, 0x00010000), EV(0, 11, 32, 7, 0), TH(8), EV(0, 0, 1000, 3, 0x80000000)]
    return {k: M.array(v, ws) for k, ws in hand.items()}


HAND = {v: _hand(v) for v in VERSIONS}
CASES = [(v, name) for v in VERSIONS for name in sorted(HAND[v])]


# ---------------------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("version", VERSIONS)
def test_model_round_trips_the_encoder_through_three_clock_wraps(version):
    ev = M3.recording(1, 3000, t_end=int(6.6 * 2 ** 34))
    assert int(ev[3][-1]) > 3 * 2 ** 34
    words = M.encode(*ev, version, seed=2)
    assert words.dtype == M.WORD_DTYPE[version]
    types = set((words >> np.array(M.WORD_BITS[version] - 4, words.dtype)).tolist())
    assert {M.CD_OFF, M.CD_ON, M.TIME_HIGH} <= types and types & set(M.IGNORED) and not types & set(M.UNKNOWN)
    got, counters, state = M.decode(words, version)
    assert all(np.array_equal(a, b) for a, b in zip(got, ev))
    assert counters == (0, 0) and int(ev[3][-1]) >> 34 == 3 and state[1] == 3 and state[2] == 1
    high_words = [int(w) for w in words.tolist() if int(w) >> (M.WORD_BITS[version] - 4) == M.TIME_HIGH]
    highs = np.array([(w >> (32 if version == M.V21 else 0)) & M.HIGH_MASK for w in high_words], np.int64)
    assert (np.diff(highs) % (1 << 28) <= 1 << 26).all()              # the keep-alives
    n_event_words = sum(1 for w in words.tolist() if int(w) >> (M.WORD_BITS[version] - 4) <= M.CD_ON)
    if version == M.V21:                                               # runs of one (t, y, p) share a word
        assert n_event_words < len(ev[0]) * 3 // 4 and max(bin(int(w) & 0xFFFFFFFF).count("1") for w in words.tolist()) >= 3
    else:
        assert n_event_words == len(ev[0])
    # the same recording batch by batch through one encoder decodes to the same events
    enc = M.Encoder(version, 5)
    parts = [enc.feed(*(c[a:a + 170] for c in ev)) for a in range(0, 3000, 170)]
    got, counters, _state = M.decode(np.concatenate(parts), version)
    assert all(np.array_equal(a, b) for a, b in zip(got, ev)) and counters == (0, 0)


@pytest.mark.parametrize("version", VERSIONS)
def test_model_is_invariant_to_a_cut_at_every_word(version):
    streams = dict(HAND[version], encoded=M.encode(*M3.recording(3, 150, t_end=int(2.5 * 2 ** 34)), version, seed=4, others=0.3))
    assert 150 <= len(streams["encoded"]) <= 600
    for name, words in streams.items():
        whole = M.decode(words, version)
        for k in range(len(words) + 1):
            cut = M.decode(words, version, cuts=[k])
            assert all(np.array_equal(a, b) for a, b in zip(cut[0], whole[0])), (name, k)
            assert cut[1] == whole[1] and np.array_equal(cut[2], whole[2]), (name, k)
    rng = np.random.RandomState(0)
    words = streams["encoded"]
    for _ in range(20):                                              # several cuts at once, empty pieces included
        cuts = rng.randint(0, len(words) + 1, size=rng.randint(2, 9))
        cut, whole = M.decode(words, version, cuts=cuts), M.decode(words, version)
        assert all(np.array_equal(a, b) for a, b in zip(cut[0], whole[0])) and cut[1:2] == whole[1:2] and np.array_equal(cut[2], whole[2])


def test_model_on_hand_written_words():
    w34 = 1 << 34
    for v in VERSIONS:
        hand = HAND[v]
        (x, y, p, t), counters, state = M.decode(hand["before_high"], v)
        assert counters == ((1 + 1, 0) if v == M.V20 else (1 + 3, 0))
        assert x.tolist() == [12, 2047] and y.tolist() == [22, 2047] and p.tolist() == [1, 0] and t.tolist() == [64 + 5, 64 + 63]
        assert state.tolist() == [1, 0, 1, 0]
        (x, y, p, t), counters, state = M.decode(hand["wraps"], v)
        assert x.tolist() == [1, 2, 3, 4, 5, 6] and p.tolist() == [1, 1, 0, 0, 1, 1] and counters == (0, 0)
        assert t.tolist() == [(H27 + 5) * 64 + 1, w34 + 5 * 64 + 2, w34 + (H27 + 4) * 64 + 3, w34 + 5 * 64 + 4,       # exactly 2^27: a wrap;
                              w34 + M.HIGH_MASK * 64 + 63, 2 * w34]                                                  # 2^27 - 1: a step back
        assert state.tolist() == [0, 2, 1, 0]
        (x, *_), counters, state = M.decode(hand["time_only"], v)
        assert len(x) == 0 and counters == (0, 0) and state.tolist() == [M.HIGH_MASK, 1, 1, 0]      # H27 + 11 -> 3 wraps, 3 -> 2 and 2 -> top do not
        (x, y, p, t), counters, state = M.decode(hand["codes"], v)
        # the sixteen codes with one payload after TIME_HIGH 2: two event words (types 0 and 1), ten unknown, TIME_HIGH = the payload
        assert counters == (0, 10 + 10) and state.tolist() == [0x0ABCDEF, 0, 1, 0]
        if v == M.V20:
            assert x.tolist() == [(0x0ABCDEF >> 11) & 0x7FF] * 2 + [3] and y.tolist() == [0x0ABCDEF & 0x7FF] * 2 + [4] and p.tolist() == [0, 1, 0]
            assert t.tolist() == [2 * 64 + ((0x0ABCDEF >> 22) & 0x3F)] * 2 + [0x0ABCDEF * 64 + 1]
        else:
            x0, yy = (0x0ABCDEF >> 11) & 0x7FF, 0x0ABCDEF & 0x7FF
            assert x.tolist() == [x0, x0 + 31] * 2 + [3] and y.tolist() == [yy] * 4 + [4] and p.tolist() == [0, 0, 1, 1, 0]
            assert t.tolist() == [2 * 64 + ((0x0ABCDEF >> 22) & 0x3F)] * 4 + [0x0ABCDEF * 64 + 1]
    (x, y, p, t), counters, state = M.decode(HAND[M.V21]["vectors"], M.V21)
    assert x.tolist() == list(range(64, 96)) + [2047, 2078, 16, 1031] and y.tolist() == [50] * 32 + [2047, 2047, 0, 3]
    assert p.tolist() == [1] * 32 + [0, 0, 1, 0] and t.tolist() == [7 * 64 + 9] * 32 + [7 * 64 + 10] * 2 + [7 * 64 + 11, 8 * 64]
    assert counters == (0, 0) and state.tolist() == [8, 0, 1, 0]


def test_evt2_entry_points_declared_exported_and_bound():
    names = [n for n in L.declared_symbols() if n.startswith("sast_evt2_")]
    assert sorted(names) == ["sast_evt2_decode", "sast_evt2_ws_bytes"]
    lib = L.lib()
    P = C.c_void_p
    for n in names:
        assert hasattr(lib, n) and n in L._SIGNATURES
    assert L._SIGNATURES["sast_evt2_decode"] == (C.c_int, [P, P, C.c_int64, C.c_int, C.c_int, P, P, P, P, P, P, P, C.c_int64, P, P, P])
    assert L._SIGNATURES["sast_evt2_ws_bytes"] == (C.c_size_t, [C.c_int])
    assert (L.EVT2_V20, L.EVT2_V21, L.EVT2_STATE_WORDS) == (0, 1, 4)
    assert BW == 256 * PT and 1 <= MAXB <= 256 and PT * 4 % 16 == 0    # 256 threads; the fold in front takes one summary per thread
    for n_streams in (1, 3, 65535):
        assert lib.sast_evt2_ws_bytes(n_streams) == n_streams * (MAXB + 1) * 24
    assert lib.sast_evt2_ws_bytes(0) == 0 and lib.sast_evt2_ws_bytes(-1) == 0 and lib.sast_evt2_ws_bytes(65536) == 0


def test_evt2_decode_rejects_bad_arguments_before_any_launch():
    lib = L.lib()
    p = 0x1000
    good = dict(words=p, counts=p, chunk_words=256, S=3, version=L.EVT2_V20, reset=None, state=p, ws=p, x=p, y=p, p=p, t=p, max_events=256,
                out_counts=p, err=p)
    before = lib.sast_launch_count()

    def call(**kw):
        a = dict(good, **kw)
        return lib.sast_evt2_decode(*[a[k] for k in good], None)

    for version in (L.EVT2_V20, L.EVT2_V21):
        for name in ("words", "counts", "state", "ws", "x", "y", "p", "t", "out_counts", "err"):
            assert call(version=version, **{name: None}) == -22, name
        for kw in (dict(S=0), dict(S=-1), dict(S=65536), dict(chunk_words=-1), dict(S=8, chunk_words=2 ** 28), dict(S=1, chunk_words=2 ** 31),
                   dict(max_events=0), dict(max_events=-4), dict(max_events=2 ** 30), dict(S=1, max_events=2 ** 31), dict(words=p + 1),
                   dict(words=p + 2), dict(ws=p + 2)):
            assert call(version=version, **kw) == -22, (version, kw)
    for version in (2, -1, 3, 21):
        assert call(version=version) == -22, version
    assert call(version=L.EVT2_V21, S=1, chunk_words=(2 ** 31 - 1) // 32 + 1, max_events=2 ** 31 - 1) == -22      # 32 events a word
    assert call(version=L.EVT2_V21, words=p + 4) == -22                 # aligned to 4 bytes: not a 64-bit word's
    assert lib.sast_launch_count() == before


def test_evt2_python_argument_validation(monkeypatch):
    from sast_amd.events import EventQueue, Evt2Decoder
    from sast_amd.online import OnlineDetector
    with pytest.raises(ValueError, match="num_streams"):
        Evt2Decoder(0)
    with pytest.raises(ValueError, match="max_events"):
        Evt2Decoder(3, 0)
    with pytest.raises(ValueError, match="2\\^31"):
        Evt2Decoder(3, 2 ** 30)
    for bad in ("3.0", 2.0, None, "2"):
        with pytest.raises(ValueError, match="version"):
            Evt2Decoder(3, version=bad)

    class _Det:
        training = False

        class yolox_head:
            num_classes = 2

    other = {M.V20: M.V21, M.V21: M.V20}
    for v in VERSIONS:
        dec = Evt2Decoder(S, version=v)
        assert dec.errors() == (0, 0, 0) and dec.DECODE_LAUNCHES == DECODE_LAUNCHES and dec.state is None and dec.version == v
        dec.reset()
        dec.reset(streams=[1])
        q = EventQueue(S, 64, 48, 64, duration_us=1000)
        assert q.evt2_errors() == (0, 0, 0) and q.PUSH_EVT2_LAUNCHES == PUSH_EVT2_LAUNCHES and q.errors() == (0, 0, 0, 0)
        od = OnlineDetector(_Det(), q, windows_per_step=2)
        words, counts = torch.zeros(S, 16, dtype=TORCH_DTYPE[v]), torch.zeros(S, dtype=torch.int64)
        pushes = (dec, lambda *a: q.push_evt2(*a, version=v), lambda *a: od.push_evt2(*a, version=v))
        for push in pushes:
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                push(words, counts)
            if v == M.V20 and hasattr(torch, "uint32"):
                with pytest.raises(RuntimeError, match="no CPU fallback"):
                    push(words.view(torch.uint32), counts)
            for bad in (torch.int16, torch.uint8, TORCH_DTYPE[other[v]], torch.float32):
                with pytest.raises(TypeError, match=str(TORCH_DTYPE[v]).replace("torch.", "")):
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
            od.push_evt2(words, counts, None, torch.zeros(S, dtype=torch.int64), version=v)
        # the queue's decoder is made by the first call: another version or max_events is refused before anything else is looked at
        assert q.evt2 is not None and q.evt2.version == v and q.evt2.max_events is None
        with pytest.raises(ValueError, match="version"):
            q.push_evt2(words, counts, version=other[v])
        with pytest.raises(ValueError, match="version"):
            q.push_evt2(words, counts, version="3.0")
        with pytest.raises(ValueError, match="max_events"):
            q.push_evt2(words, counts, max_events=99, version=v)
        q2 = EventQueue(S, 64, 48, 64, duration_us=1000)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            q2.push_evt2(words, counts, max_events=50, version=v)
        with pytest.raises(ValueError, match="max_events=50"):
            q2.push_evt2(words, counts, max_events=51, version=v)
        with pytest.raises(RuntimeError, match="no CPU fallback"):          # leaving max_events out keeps the decoder's
            q2.push_evt2(words, counts, version=v)
        assert dec.state is None and q.evt2.state is None and q2.evt2.state is None        # nothing was allocated on the way
    dec = Evt2Decoder(S, version=M.V20)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="un-captured"):                          # the state and the staging are never born in a capture
        dec._buffers(torch.device("cpu"), 16)
    assert dec.state is None and dec.x is None


def test_evt2_python_limits_of_two_to_the_31():
    """S * chunk_words and, for 2.1, 32 * chunk_words above 2^31 - 1 are refused from the shape alone (meta tensors: nothing that large
    is allocated), before the "no CPU fallback" error"""
    from sast_amd.events import Evt2Decoder
    counts = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="32 \\* chunk words must be below 2\\^31"):
        Evt2Decoder(1, version=M.V21)(torch.empty(1, (2 ** 31 - 1) // 32 + 1, dtype=torch.int64, device="meta"), counts)
    with pytest.raises(ValueError, match="num_streams \\* chunk words"):
        Evt2Decoder(8, version=M.V20)(torch.empty(8, 2 ** 28, dtype=torch.int32, device="meta"), torch.zeros(8, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # at the limit the shape passes
        Evt2Decoder(1, version=M.V21)(torch.empty(1, (2 ** 31 - 1) // 32, dtype=torch.int64, device="meta"), counts)
    with pytest.raises(ValueError, match="num_streams \\* max_events must be below 2\\^31"):
        Evt2Decoder(8, 2 ** 28, version=M.V21)


def test_the_decoders_are_one_python_path_and_keep_their_fanouts():
    """`Evt3Decoder` and `Evt2Decoder` only name their format: the buffers, the counters, the reset and the call are `_EventDecoder`'s;
    the default staging of a row is 12, 1 and 32 events per word"""
    from sast_amd.events import Evt2Decoder, Evt3Decoder, _EventDecoder
    for cls in (Evt3Decoder, Evt2Decoder):
        assert issubclass(cls, _EventDecoder)
        assert not {"_buffers", "errors", "reset", "__call__"} & set(vars(cls))
    decoders = (Evt3Decoder(S), Evt2Decoder(S, version=M.V20), Evt2Decoder(S, version=M.V21))
    assert [d.fanout for d in decoders] == [12, 1, 32]
    assert [d._room(16) for d in decoders] == [12 * 16, 16, 32 * 16]
    assert Evt2Decoder(S, 7, version=M.V21)._room(16) == 7           # an explicit max_events is the staging


HEADER = (b"% camera_integrator_name Prophesee\r\n% date 2023-03-29 16:37:46\n% evt 3.0\n% format EVT3;height=720;width=1280\n"
          b"% generation 4.2\n% geometry 1280x720\n% end\n")


def test_raw_header():
    from sast_amd.events import RawHeader, raw_header
    # "% end" ends the header whatever follows: the first data byte here is 0x25, '%'
    for wrap in (bytes, bytearray, memoryview):
        h = raw_header(wrap(HEADER + b"\x25\x00\x01\x02"))
        assert isinstance(h, RawHeader) and h == ("evt3", 1280, 720, len(HEADER), h.fields)
    assert h.fields == {"camera_integrator_name": "Prophesee", "date": "2023-03-29 16:37:46", "evt": "3.0",        # the \r is dropped
                        "format": "EVT3;height=720;width=1280", "generation": "4.2", "geometry": "1280x720"}
    assert raw_header(HEADER).offset == len(HEADER)                      # nothing behind "% end" is needed
    # without "% end": the header ends at the first line that does not start with '%'
    old = b"% Date 2020-01-01\n% evt 2.0\n% geometry 640x480\n"
    h = raw_header(old + b"\x00\x00\x00\x80")
    assert (h.format, h.width, h.height, h.offset) == ("evt2", 640, 480, len(old)) and h.fields["Date"] == "2020-01-01"
    # CRLF lines throughout
    crlf = b"% format EVT21;width=320;height=320\r\n% end\r\n"
    h = raw_header(crlf + b"\r\n")
    assert (h.format, h.width, h.height, h.offset) == ("evt21", 320, 320, len(crlf)) and h.fields == {"format": "EVT21;width=320;height=320"}
    # `format` wins over `evt` and `geometry`; without it they are read; without any of them None
    h = raw_header(b"% evt 2.0\n% geometry 1x2\n% format EVT2;height=480;width=640\n% end\n")
    assert (h.format, h.width, h.height) == ("evt2", 640, 480)
    assert raw_header(b"% format EVT3\n% end\n")[:3] == ("evt3", None, None)
    assert raw_header(b"% format EVT3\n% geometry 1280x720\n% end\n")[:3] == ("evt3", 1280, 720)
    for text, fmt in ((b"2.0", "evt2"), (b"2.1", "evt21"), (b"3.0", "evt3"), (b"4.0", None)):
        assert raw_header(b"% evt " + text + b"\n% end\n").format == fmt
    h = raw_header(b"% serial_number 00001\n% end\nDATA")
    assert h == (None, None, None, 28, {"serial_number": "00001"})
    assert raw_header(b"% format HISTO3D;width=320\n% end\n")[:3] == (None, 320, None)
    assert raw_header(b"\x00\x01") == (None, None, None, 0, {})           # no header at all
    # a buffer that ends inside the header: in the middle of a line, behind a line that another may follow, or empty
    for cut in (1, 10, len(HEADER) - 6, len(HEADER) - 1):
        with pytest.raises(ValueError, match="more bytes are needed"):
            raw_header(HEADER[:cut])
    for short in (b"", old, old[:-1]):
        with pytest.raises(ValueError, match="more bytes are needed"):
            raw_header(short)
    with pytest.raises(TypeError, match="bytes"):
        raw_header("% end\n")


# ---------------------------------------------------------------------------------------------------------------------------- GPU

def _dev_words(parts, cap, version):
    """per-row word arrays -> (int32 / int64 [S, cap] with stale event words past each count, counts int64 [S]) on the device"""
    buf = np.full((len(parts), cap), STALE[version], M.WORD_DTYPE[version])
    for s, part in enumerate(parts):
        buf[s, :len(part)] = part
    return torch.from_numpy(buf.view(SIGNED[version])).cuda(), torch.tensor([len(part) for part in parts], dtype=torch.int64).cuda()


class _Session:
    """a device decoder beside one model per row: every `call` decodes one chunk per row on both and compares all of it"""

    def __init__(self, version, max_events=None):
        from sast_amd.events import Evt2Decoder
        self.version = version
        self.dec = Evt2Decoder(S, max_events, version)
        self.models = [M.Decoder(version) for _ in range(S)]
        self.dropped = self.events = self.calls = 0

    def call(self, parts, cap=None, reset=None, tag=None):
        cap = max(len(part) for part in parts) + 3 if cap is None else cap
        words, counts = _dev_words(parts, cap, self.version)
        rst = None if reset is None else torch.tensor(reset, dtype=torch.uint8).cuda()
        self.calls += 1
        if self.version == M.V20 and self.calls % 2 == 0 and hasattr(torch, "uint32"):
            words = words.view(torch.uint32)                          # every second EVT 2.0 chunk as the unsigned dtype
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
    """per version: two encoded recordings through clock wraps (rows 0 and 2), and a long one for the chunks that span several
    workgroups.  The events are made once and shared."""
    evs = (M3.recording(11, 900, t_end=int(4.4 * 2 ** 34)), M3.recording(13, 700, t_end=int(2.2 * 2 ** 34), bursts=0.6),
           M3.recording(15, 40000, t_start=5000, t_step=30))
    out = {}
    for v in VERSIONS:
        a, b, long = M.encode(*evs[0], v, seed=12), M.encode(*evs[1], v, seed=14, others=0.3), M.encode(*evs[2], v, seed=16)
        assert len(a) > 800 and len(a) > len(b) > 400 and len(long) > 20 * BW
        out[v] = a, b, long
    return out


CHUNK_LENGTHS = sorted({1, 2, PT - 1, PT, PT + 1, WAVE - 1, WAVE, WAVE + 1, BW - 1, BW, BW + 1})


@gpu
@pytest.mark.parametrize("length", CHUNK_LENGTHS)
@pytest.mark.parametrize("version", VERSIONS)
def test_decoder_equals_the_model_over_chunk_lengths(streams, version, length):
    """row 0 in chunks of `length` words, row 2 in chunks of length + 2 of another stream (shorter: its last chunks are empty), row 1
    never gets a word.  The capacity length + 3 is a multiple of the 16-byte load for some lengths and not for others."""
    a, b, long = streams[version]
    if length <= PT + 1:
        a, b = a[:300], b[:200]
    elif length >= BW - 1:
        a = long[:6 * length + 11]
    ses = _Session(version)
    for k in range((len(a) + length - 1) // length):
        ses.call([a[k * length:(k + 1) * length], a[:0], b[k * (length + 2):(k + 1) * (length + 2)]], length + 3, tag=(length, k))
    ses.finish()
    assert ses.events > 100 and ses.counters() == (0, 0, 0) and (not PT + 1 < length < BW - 1 or ses.models[0].wraps >= 2)


@gpu
@pytest.mark.parametrize("cap", [3 * BW, 3 * BW - 3])
@pytest.mark.parametrize("version", VERSIONS)
def test_decoder_equals_the_model_when_a_row_spans_several_workgroups(streams, version, cap):
    """capacity 3 x BLOCK_WORDS: three workgroups per row, pieces of ceil(n / 3) words rounded up to a thread's words.  The counts put
    the last piece at one word, at none and at full, a piece's end inside a thread's words, and n at the capacity and one below; the
    capacity 3 x BLOCK_WORDS - 3 is odd: its rows are not 16-byte aligned and the loads go word by word."""
    _a, b, long = streams[version]
    assert -(-cap // BW) == 3 and (cap % 2 == 1 or cap % PT == 0)
    lengths = [PT, PT + 1, 2 * PT, 2 * PT + 1, 3 * PT, 3 * PT + 1, BW - 1, BW, BW + 1, 2 * BW - 1, 2 * BW, 2 * BW + 1, cap - 7, cap - 1, cap]
    assert sum(lengths) <= len(long)
    ses, at, bt = _Session(version), 0, 0
    for k, n in enumerate(lengths):
        m = lengths[-1 - k] % 300                                     # row 2: other counts, below one workgroup's piece
        ses.call([long[at:at + n], long[:0], b[bt:bt + m]], cap, tag=(cap, n))
        at, bt = at + n, bt + m
    ses.finish()
    assert ses.events > 5000 and ses.counters() == (0, 0, 0)


def _random_words(version, n, seed):
    """n words of every type, built with numpy: a TIME_HIGH that climbs through its wraps, EVT 2.1 masks of a few bits (some empty)"""
    rng = np.random.RandomState(seed)
    codes = np.array([M.OTHERS, M.CD_OFF, M.CD_ON, M.TIME_HIGH, M.EXT_TRIGGER, 0x9, 0x3], np.uint64)
    tc = codes[rng.choice(len(codes), p=[.45, .15, .15, .15, .05, .02, .03], size=n)]
    low = rng.randint(0, 1 << 28, size=n).astype(np.uint64)
    hi = tc == M.TIME_HIGH
    low[hi] = ((np.cumsum(rng.randint(0, 1 << 20, size=int(hi.sum()))) + 5) & M.HIGH_MASK).astype(np.uint64)
    if version == M.V20:
        return ((tc << np.uint64(28)) | low).astype(np.uint32)
    valid = (rng.randint(0, 1 << 32, size=n, dtype=np.int64) & rng.randint(0, 1 << 32, size=n, dtype=np.int64)
             & rng.randint(0, 1 << 32, size=n, dtype=np.int64)).astype(np.uint64)
    valid[rng.rand(n) < 0.1] = 0
    return (tc << np.uint64(60)) | (low << np.uint64(32)) | valid


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_decoder_equals_the_model_when_workgroups_take_several_steps(version):
    """more than MAX_BLOCKS x BLOCK_WORDS words in a row: the workgroup count stops at MAX_BLOCKS and every workgroup takes two steps.
    Random words of every type; the staging holds the row's events exactly."""
    n = MAXB * BW + BW + 5
    words = _random_words(version, n, 21)
    other = HAND[version]["wraps"]
    total = len(M.decode(words, version)[0][0])
    ses = _Session(version, max_events=total)
    ses.call([words, words[:0], other], n + 3)
    ses.finish()
    assert ses.events == total + 6 and total > n // 4 and ses.counters()[1] > 1000 and ses.counters()[2] == 0 and ses.models[0].wraps >= 2


@gpu
@pytest.mark.parametrize("version, name", CASES)
def test_decoder_equals_the_model_at_every_cut_of_the_hand_written_streams(version, name):
    """a cut in front of and behind the first TIME_HIGH, in front of and behind a wrap and a step back of TIME_HIGH, inside a chunk of
    only time words, between unknown codes and around every vector: every position.  Row 0 takes the stream in two chunks (with its
    reset flag set for the first), row 2 whole and then nothing."""
    words = HAND[version][name]
    ses = _Session(version)
    for k in range(len(words) + 1):
        ses.call([words[:k], words[:0], words], 48, reset=[1, 0, 1], tag=(name, k, 0))
        ses.call([words[k:], words[:0], words[:0]], 48, tag=(name, k, 1))
    ses.finish()
    want = M.decode(words, version)
    assert ses.counters() == (2 * (len(words) + 1) * want[1][0], 2 * (len(words) + 1) * want[1][1], 0)
    assert np.array_equal(ses.models[0].state(), want[2]) and np.array_equal(ses.models[2].state(), want[2])


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_words_fill_the_staging_exactly_and_five_too_many_are_counted_and_not_written(version):
    """EVT 2.1: full vectors (fan-out 32).  With max_events five short, the first events are the ones kept, and the slot behind the last
    one (row 1's first slot: row 1 is empty) keeps the sentinel the staging was filled with"""
    fan = M.FANOUT[version]
    head = M.array(version, [M.time_high(version, 3)])
    full = M.array(version, [M.cd(version, 1, 9, fan * k, 4, 0xFFFFFFFF if fan == 32 else 1) for k in range(40)])
    total = 40 * fan
    for short in (0, 5):
        ses = _Session(version, max_events=total - short)
        ses.call([head, head[:0], head], 8)
        for col in (ses.dec.x, ses.dec.y, ses.dec.p, ses.dec.t):
            col.fill_(-7)
        n = ses.call([full, full[:0], full[:13]], 40)
        assert n == [total - short, 0, 13 * fan]
        ses.finish()
        assert ses.counters() == (0, 0, short) and ses.dec.x.shape == (S, total - short)
        assert ses.dec.x[0].cpu().tolist() == list(range(total - short))           # the FIRST events are the ones kept
        for col in (ses.dec.x, ses.dec.y, ses.dec.p, ses.dec.t):
            assert col[1].eq(-7).all() and col[2, 13 * fan:].eq(-7).all() and not col[2, :13 * fan].eq(-7).any()
    ses = _Session(version)                                             # the default staging, fan-out x the chunk's words, never drops
    ses.call([head, head[:0], head], 40)
    ses.call([full, full[:0], full], 40)
    ses.finish()
    assert ses.dec.x.shape == (S, total) and ses.counters() == (0, 0, 0)


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_reset_on_one_row_only(streams, version):
    a, b, _long = streams[version]
    ses = _Session(version)
    cut = 200 + next(i for i, w in enumerate(b[200:].tolist()) if (int(w) >> (M.WORD_BITS[version] - 4)) <= M.CD_ON)   # in front of an event
    ses.call([a[:300], a[:0], b[:cut]], 320)
    before = [m.state().copy() for m in ses.models]
    ses.call([a[300:600], a[:0], b[cut:cut + 200]], 320, reset=[0, 1, 1], tag="reset")
    # row 2 started over in the middle of its stream: its events up to the next TIME_HIGH are counted, row 0 lost nothing
    assert ses.counters()[0] > 0 and ses.models[0].before_high == 0 and ses.models[0].wraps >= before[0][1]
    ses.call([a[600:900], a[:0], b[cut + 200:cut + 400]], 320)
    ses.dec.reset(streams=[0])                                          # the host-side form
    ses.models[0].reset()
    ses.call([a[900:1200], a[:0], b[cut + 400:cut + 500]], 320, tag="host reset")
    ses.finish()
    ses.dec.reset()
    assert ses.dec.errors() == (0, 0, 0) and int(ses.dec.state.abs().sum()) == 0


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_decode_launch_counts_equal_the_class_constants(streams, version):
    from sast_amd.events import EventQueue, Evt2Decoder
    _a, _b, long = streams[version]
    lib = L.lib()
    assert (Evt2Decoder.DECODE_LAUNCHES, EventQueue.PUSH_EVT2_LAUNCHES) == (DECODE_LAUNCHES, PUSH_EVT2_LAUNCHES)
    for n_streams, cap in ((1, 64), (3, 5000), (8, 20000)):
        words, counts = _dev_words([long[:cap - s] for s in range(n_streams)], cap, version)
        dec = Evt2Decoder(n_streams, version=version)
        q = EventQueue(n_streams, 32 * cap + 8, 48, 64, duration_us=1000)
        for _ in range(2):                                              # the first calls allocate; the count is the same
            before = lib.sast_launch_count()
            dec(words, counts)
            assert lib.sast_launch_count() - before == DECODE_LAUNCHES, (n_streams, cap)
            before = lib.sast_launch_count()
            q.push_evt2(words, counts, version=version)
            assert lib.sast_launch_count() - before == PUSH_EVT2_LAUNCHES, (n_streams, cap)
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
    recs = [M3.recording(31, 2500, t_step=12, **GEO), M3.recording(32, 0, **GEO), M3.recording(33, 1700, t_step=16, bursts=0.7, **GEO)]
    return recs, {v: [M.encode(*r, v, seed=40 + s) for s, r in enumerate(recs)] for v in VERSIONS}


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_push_evt2_gives_the_frames_of_push_on_the_original_events(recordings, version):
    """chunks of 97, 256 and 1000 words: cut wherever the words fall, away from the 2 ms window ends"""
    from sast_amd.events import EventQueue
    recs, words = recordings[0], recordings[1][version]
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
            w, n = _dev_words([w[k * chunk:(k + 1) * chunk] for w in words], chunk, version)
            q.push_evt2(w, n, version=version)
        assert q.count.cpu().tolist() == [2500, 0, 1700]
        for name in ("x", "y", "p", "t"):
            assert all(torch.equal(getattr(q, name)[s, :len(recs[s][0])], stored[name][s, :len(recs[s][0])]) for s in range(S)), (chunk, name)
        got = q.frames(ends)
        assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), chunk
        assert q.errors() == (0, 0, 0, 0) and q.evt2_errors() == (0, 0, 0)
        assert torch.equal(q.t_last, ref.t_last)


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_columns_past_the_sensor_are_counted_invalid_and_never_drawn(version):
    """events past the sensor's 64 columns (for 2.1: a vector that starts inside and runs out, and x_base = 2047 with bit 31 set, x =
    2078) are stored with x as written, `frames` counts them invalid and draws none of them"""
    from sast_amd.events import EventQueue
    if version == M.V21:
        body = [M.cd(version, 1, 50, 56, 10, 0xFFFFFFFF), M.cd(version, 0, 51, 2047, 11, 0x80000001), M.cd(version, 1, 52, 40, 12, 0x01FFFFFF)]
    else:
        body = [M.cd(version, 1, 50, x, 10) for x in (56, 63, 64, 65, 2047)] + [M.cd(version, 0, 51, 1000, 11), M.cd(version, 0, 52, 0, 47)]
    words = M.array(version, [M.time_high(version, 0)] + body)
    (x, y, p, t), _c, _state = M.decode(words, version)
    inside = int((x < 64).sum())
    assert inside in (3, 8 + 24) and x.max() == (2078 if version == M.V21 else 2047) and len(x) - inside >= 4
    q, ref = EventQueue(S, 256, **Q_KW), EventQueue(S, 256, **Q_KW)
    w, n = _dev_words([words, words[:0], words[:0]], len(words) + 2, version)
    q.push_evt2(w, n, torch.ones(S, dtype=torch.uint8).cuda(), version=version)
    assert q.x[0, :len(x)].cpu().tolist() == x.tolist() and q.count.cpu().tolist() == [len(x), 0, 0]
    empty = tuple(x[:0] for _ in range(4))
    cols, counts = _columns([(x, y, p, t), empty, empty], len(x))
    ref.push(*cols, counts)
    ends = torch.tensor([[2000] * S], dtype=torch.int64).cuda()
    got, want = q.frames(ends), ref.frames(ends)
    assert torch.equal(got, want) and int(got[0, 0].to(torch.int64).sum()) == inside and int(got[0, 1:].count_nonzero()) == 0
    assert q.errors() == ref.errors() == (len(x) - inside, 0, 0, 0) and q.evt2_errors() == (0, 0, 0)


@gpu
@pytest.mark.parametrize("version", VERSIONS)
def test_captured_push_evt2_and_frames_replay_on_new_words_like_the_eager_run(recordings, version):
    from sast_amd.events import EventQueue
    words = recordings[1][version]
    chunk = max(len(w) for w in words) // 4 + 1
    steps = []
    for k in range(4):
        parts = [w[k * chunk:(k + 1) * chunk] for w in words]
        if k == 2:
            parts[2] = words[0][:chunk // 2]                           # row 2 starts another recording with its reset flag
        steps.append((parts, [0, 0, int(k == 2)], [[1000 * (2 * k + 1)] * S, [1000 * (2 * k + 2)] * S]))     # a chunk of row 0 spans about 2000 us
    w, n = _dev_words(steps[0][0], chunk, version)
    rst, ends = torch.zeros(S, dtype=torch.uint8).cuda(), torch.zeros(2, S, dtype=torch.int64).cuda()

    def load(step):
        nw, nn = _dev_words(step[0], chunk, version)
        w.copy_(nw), n.copy_(nn), rst.copy_(torch.tensor(step[1], dtype=torch.uint8)), ends.copy_(torch.tensor(step[2], dtype=torch.int64))

    def call(q):
        q.push_evt2(w, n, rst, version=version)
        return q.frames(ends)

    eager, qe = [], EventQueue(S, 8192, **Q_KW)
    for step in steps:
        load(step)
        fr = call(qe)
        eager.append((fr.clone(), qe.count.clone(), qe.t_last.clone(), qe.evt2.state.clone()))
    assert int(eager[3][0].count_nonzero()) > 0 and not torch.equal(eager[0][0], eager[1][0]) and qe.evt2_errors()[1:] == (0, 0)
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
        assert torch.equal(g_fr, fr) and torch.equal(q.count, count) and torch.equal(q.t_last, t_last) and torch.equal(q.evt2.state, state)
    assert q.errors() == qe.errors() and q.evt2_errors() == qe.evt2_errors()


# ------------------------------------------------------------------------------------------------------------------ the detector

from test_evt3 import detector  # noqa: E402, F401  (the small detector fixture the EVT 3.0 test builds)


@gpu
def test_online_detector_push_evt2_gives_the_records_of_push(detector):  # noqa: F811
    """the same event chunks, as columns into one OnlineDetector and as EVT 2.0 and EVT 2.1 sensor words (each chunk through the row's
    encoder) into others: the same records, byte for byte, push by push, eager and then replayed from a graph; row 1 starts a second
    recording on the way"""
    from sast_amd.events import EventQueue
    from sast_amd.online import OnlineDetector
    geo, D, chunk, wcap = dict(height=128, width=160), 600, 300, 1024
    recs = [M3.recording(51 + s, 1500, t_start=40, t_step=step, **geo) for s, step in enumerate((16, 8, 8))]
    second = M3.recording(57, 600, t_start=20, t_step=8, **geo)
    encs = {v: [M.Encoder(v, 61 + s) for s in range(S)] for v in VERSIONS}
    rng = np.random.RandomState(7)
    rounds, cur, src = [], [0] * S, list(recs)
    for r in range(8):
        reset, final = np.zeros(S, np.uint8), np.zeros(S, np.uint8)
        if r == 4:
            src[1], cur[1], reset[1] = second, 0, 1
            for v in VERSIONS:
                encs[v][1] = M.Encoder(v, 71)
        if r == 7:
            final[2] = 1
        parts = []
        for s in range(S):
            hi = min(len(src[s][0]), cur[s] + int(rng.randint(0, chunk + 1)))
            parts.append(tuple(c[cur[s]:hi] for c in src[s]))
            cur[s] = hi
        rounds.append((parts, {v: [encs[v][s].feed(*parts[s]) for s in range(S)] for v in VERSIONS}, reset, final))
    assert max(len(w) for _p, ws, _r, _f in rounds for v in VERSIONS for w in ws[v]) <= wcap

    def make():
        return OnlineDetector(detector, EventQueue(S, 8192, duration_us=D, **geo), windows_per_step=2, max_det=100, conf_thre=0.45,
                              nms_thre=0.45)

    def same(got, want):
        assert [s for s, _a in got] == [s for s, _a in want]
        assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for (_s, a), (_t, b) in zip(got, want))

    od_cols = make()
    od_words, od_graph = {v: make() for v in VERSIONS}, {v: make() for v in VERSIONS}
    static = {v: _dev_words(rounds[0][1][v], wcap, v) for v in VERSIONS}
    rst, fin = torch.zeros(S, dtype=torch.uint8).cuda(), torch.zeros(S, dtype=torch.uint8).cuda()
    n_records = n_windows = 0
    for r, (parts, words, reset, final) in enumerate(rounds):
        cols, counts = _columns(parts, chunk)
        od_cols.push(*cols, counts, torch.from_numpy(reset).cuda(), torch.from_numpy(final).cuda())
        want = od_cols.drain()
        rst.copy_(torch.from_numpy(reset)), fin.copy_(torch.from_numpy(final))
        for v in VERSIONS:
            nw, nn = _dev_words(words[v], wcap, v)
            od_words[v].push_evt2(nw, nn, torch.from_numpy(reset).cuda(), torch.from_numpy(final).cuda(), version=v)
            same(od_words[v].drain(), want)
            w, n = static[v]
            w.copy_(nw), n.copy_(nn)
            if r == 0:
                od_graph[v].push_evt2(w, n, rst, fin, version=v)
                od_graph[v].capture()
            else:
                od_graph[v].replay()
            same(od_graph[v].drain(), want)
        n_records += sum(len(a) for _s, a in want)
        n_windows += len(want)
    assert n_records > 0 and n_windows >= 6
    for other in list(od_words.values()) + list(od_graph.values()):
        assert other.errors() == od_cols.errors() and other.queue.evt2_errors() == (0, 0, 0)
        for (h, c), (h2, c2) in zip(other.states, od_cols.states):
            assert torch.equal(h, h2) and torch.equal(c, c2)
