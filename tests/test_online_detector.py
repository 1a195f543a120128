"""sast_amd.online on the MI355X: the window scheduler, the predicated state commit and the record export each against a host
restatement, then `OnlineDetector` end to end against a host-scheduled loop of the same detector, across batches and under a graph.

Geometry of the queue tests: a 128 x 160 sensor, 600 us windows, streams from tests/golden/make_golden_events.py's generator."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_events as G  # noqa: E402
import online_model as OM  # noqa: E402

gpu = pytest.mark.gpu

GEO = dict(height=128, width=160)
D, S, CAP, CHUNK = 600, 3, 8192, 320
FAST, SLOW_A, SLOW_B, SECOND, OTHER_A, OTHER_B = range(6)


def _recording(which):
    kw = {FAST: dict(seed=71, n=1200, t_start=40, t_step=32, jitter=60),        # 4 x the others' clock rate: its windows pile up
          SLOW_A: dict(seed=72, n=1200, t_start=90, t_step=8, jitter=60),
          SLOW_B: dict(seed=73, n=1200, t_start=55, t_step=8, jitter=60),
          SECOND: dict(seed=74, n=700, t_start=20, t_step=8, jitter=30),          # what row 1 starts after its reset: a clock far below
          OTHER_A: dict(seed=75, n=1500, t_start=70, t_step=6, jitter=40),
          OTHER_B: dict(seed=76, n=900, t_start=30, t_step=10, jitter=0)}[which]
    return [np.array(c) for c in G.stream(**kw, **GEO)]


def _corrected(t):
    return np.maximum.accumulate(np.concatenate([[0], np.asarray(t, np.int64)]))[1:]


def _session(W, seed, rows=(FAST, SLOW_A, SLOW_B), reset_round=3, max_rounds=None):
    """a streaming session over three rows -> (rounds, recordings, exact): every round is (parts, reset, final, ends, due, backlog,
    next_end), the last four from the model.  Chunk cuts are random, one chunk in four is empty, one cut in three falls on the last
    event of a window, and row 2 is cut once right behind an event whose time IS a window end (exact: that round).  Row 1 starts its
    second recording at `reset_round`; once every event is pushed row 2 is final, and empty chunks follow until no window is owed."""
    rngs = [np.random.RandomState(100 * seed + s) for s in range(S)]         # one per row: a row's cuts do not depend on its neighbours
    recs = [_recording(r) for r in rows]
    i = int(np.searchsorted(_corrected(recs[2][3]), 2 * D, side="left"))
    recs[2][3][i] = 2 * D                                      # corrected time exactly 2 D, whatever it was
    exact_idx, exact_round = i, None
    src, cur = list(recs), [0] * S
    model = OM.StepModel(S, D, W)
    rounds, tail = [], 2
    while tail > 0 and (max_rounds is None or len(rounds) < max_rounds):
        r = len(rounds)
        reset = np.zeros(S, np.uint8)
        if r == reset_round:
            src[1], cur[1], reset[1] = _recording(SECOND), 0, 1
        parts = []
        for s in range(S):
            rng = rngs[s]
            n, tc = len(src[s][3]), _corrected(src[s][3])
            hi = min(n, cur[s] + (int(rng.randint(0, CHUNK + 1)) if rng.randint(4) else 0))
            if hi > cur[s] and rng.randint(3) == 0:                # up to the last event of the window the chunk ends in
                hi = min(max(int(np.searchsorted(tc, (tc[hi - 1] // D) * D, side="right")), cur[s] + 1), cur[s] + CHUNK)
            if s == 2 and src[s] is recs[2] and cur[s] <= exact_idx < hi:
                hi, exact_round = exact_idx + 1, r
            parts.append(tuple(c[cur[s]:hi] for c in src[s]))
            cur[s] = hi
        done = all(cur[s] == len(src[s][3]) for s in range(S)) and r > reset_round
        final = np.array([0, 0, int(done)], np.uint8)
        ends, due, backlog = model.push([p[3] for p in parts], reset, final)
        rounds.append((parts, reset, final, ends, due, backlog, model.sched.next_end.copy()))
        if done and not backlog.any():
            tail -= 1
    return rounds, recs, exact_round


def _i64(a):
    return torch.tensor(np.asarray(a, np.int64)).cuda()


def _u8(a):
    return torch.tensor(np.asarray(a, np.uint8)).cuda()


def _chunk(parts, cap=CHUNK):
    cols = [np.full((len(parts), cap), g, np.int64) for g in (5, 5, 1, 123)]        # stale events past the counts
    for s, part in enumerate(parts):
        for c, a in zip(cols, part):
            c[s, :len(a)] = a
    return [torch.from_numpy(c).cuda() for c in cols], _i64([len(p[0]) for p in parts])


def _queue(**kw):
    from sast_amd.events import EventQueue
    return EventQueue(S, CAP, duration_us=D, **GEO, **kw)


def _whole_frames(recs, ends):
    """EventStreams' frames of the whole recordings at ends [T, S]"""
    from sast_amd.events import EventStreams
    cap = max(len(r[3]) for r in recs)
    cols, counts = _chunk(recs, cap)
    return EventStreams(S, duration_us=D, **GEO)(*cols, counts, _i64(ends), check=True)


# ------------------------------------------------------------------------------------------------------------------ 1, 2: scheduler, frames

def _scheduler_run(W, keep_frames=False):
    from sast_amd.online import schedule_windows
    rounds, recs, exact_round = _session(W, seed=10 + W)
    q, q2 = _queue(), _queue()
    next_end = torch.full((S,), D, dtype=torch.int64, device="cuda")
    ends, due, backlog = torch.zeros(W, S, dtype=torch.int64).cuda(), torch.zeros(W, S, dtype=torch.uint8).cuda(), _i64([0] * S)
    kept, saw_backlog = [], False
    for r, (parts, reset, final, m_ends, m_due, m_backlog, m_next) in enumerate(rounds):
        cols, counts = _chunk(parts)
        rst, fin = _u8(reset), _u8(final)
        q.push(*cols, counts, rst)
        schedule_windows(q, next_end, D, ends, due, backlog, rst, fin)
        frames = q.frames(ends)
        assert np.array_equal(ends.cpu().numpy(), m_ends), r
        assert np.array_equal(due.cpu().numpy(), m_due), r
        assert backlog.cpu().tolist() == m_backlog.tolist() and next_end.cpu().tolist() == m_next.tolist(), r
        if r == exact_round:                                      # t_last == the end exactly: that window is not due yet
            assert int(q.t_last[2]) == 2 * D and int(m_next[2]) == 2 * D
        # a second queue that a host loop asks for the due windows only (rows with fewer of them repeat their last end, as they must)
        q2.push(*cols, counts, rst)
        K = int(m_due.sum(0).max())
        if K:
            q2.frames(_i64(m_ends[:K]))
        for name in ("head", "count", "retired", "retired_t", "t_last"):
            assert getattr(q, name).cpu().tolist() == getattr(q2, name).cpu().tolist(), (name, r)
        saw_backlog |= bool(m_backlog.any())
        if keep_frames:
            kept += [(r, k, s, int(m_ends[k, s]), frames[k, s].clone()) for k in range(W) for s in range(S) if m_due[k, s]]
    assert q.errors() == (0, 0, 0, 0) and q2.errors() == (0, 0, 0, 0)          # nothing dropped, no late window
    assert saw_backlog and exact_round is not None
    return rounds, recs, kept


@gpu
@pytest.mark.parametrize("W", [1, 2, 3])
def test_scheduler_equals_the_model_and_asks_the_queue_for_nothing_new(W):
    _scheduler_run(W)


@gpu
def test_frames_at_due_steps_equal_event_streams_on_the_whole_recording():
    rounds, recs, kept = _scheduler_run(2, keep_frames=True)
    reset_round = next(r for r, rd in enumerate(rounds) if rd[1].any())
    assert any(s == 1 and r < reset_round for r, _k, s, _e, _f in kept) and any(s == 1 and r >= reset_round for r, _k, s, _e, _f in kept)
    for first in (True, False):                                   # row 1 before its reset, and its second recording after
        part = [x for x in kept if x[2] != 1 or (x[0] < reset_round) == first]
        per_row = [[e for _r, _k, s, e, _f in part if s == row] or [D] for row in range(S)]
        T = max(len(v) for v in per_row)
        ends = np.array([[v[min(j, len(v) - 1)] for v in per_row] for j in range(T)], np.int64)
        whole = _whole_frames([recs[0], recs[1] if first else _recording(SECOND), recs[2]], ends)
        seen = [0] * S
        for _r, _k, s, e, f in part:
            assert int(ends[seen[s], s]) == e
            assert torch.equal(f, whole[seen[s], s]), (s, e)
            seen[s] += 1
    assert len(kept) > 20 and any(int(f.max()) > 0 for *_x, f in kept)


# ------------------------------------------------------------------------------------------------------------------ 3: commit

def _pairs(B, sizes, canary=7):
    """dense fp32 (dst, src) pairs inside flat buffers, a canary region behind every destination: a list of (dst, src, whole, n)"""
    out = []
    for i, n in enumerate(sizes):
        if n == "cl":                                             # a channels-last 4-D tensor: NCHW view of NHWC memory
            numel = B * 3 * 5 * 8
            whole, sflat = torch.randn(numel + canary).cuda(), torch.randn(numel).cuda()
            dst = whole[:numel].view(B, 3, 5, 8).permute(0, 3, 1, 2)
            src = sflat.view(B, 3, 5, 8).permute(0, 3, 1, 2)
            assert not dst.is_contiguous()
        elif n == "off":                                          # 4 bytes off 16-byte alignment: the single-word path for a 4k sample
            numel = B * 64
            whole, sflat = torch.randn(1 + numel + canary).cuda(), torch.randn(numel).cuda()
            dst, src = whole[1:1 + numel].view(B, 64), sflat.view(B, 64)
            assert dst.data_ptr() % 16 == 4 and src.data_ptr() % 16 == 0
        else:
            numel = B * n
            whole, sflat = torch.randn(numel + canary).cuda(), torch.randn(numel).cuda()
            dst, src = whole[:numel].view(B, n), sflat.view(B, n)
        out.append((dst, src, whole, numel))
    return out


@gpu
@pytest.mark.parametrize("B", [1, 5, 256])
def test_commit_samples_dev_moves_exactly_the_flagged_samples(B):
    from sast_amd import _lib
    from sast_amd import functional as SF
    torch.manual_seed(B)
    sizes = [1, 3, 64, 65, "cl", "off", 4, 5, 1024, 1025, 2, 7, 8, 9, 12, 13, 16]
    assert len(sizes) == _lib.ZERO_MAX_TENSORS + 1                      # two launches
    mixed = (torch.arange(B) % 3 != 1).to(torch.uint8)
    for flags in (torch.zeros(B, dtype=torch.uint8), torch.ones(B, dtype=torch.uint8), mixed, mixed.bool()):
        pairs = _pairs(B, sizes)
        before = [w.clone() for _d, _s, w, _n in pairs]
        sources = [s.clone() for _d, s, *_ in pairs]
        ret = SF.commit_samples_dev([d for d, *_ in pairs], [s for _d, s, *_ in pairs], flags.cuda())
        assert ret[0] is pairs[0][0]
        f = flags.bool().cuda()
        for (dst, src, whole, numel), old in zip(pairs, before):
            lead = whole.numel() - numel - 7
            old_dst = old[lead:lead + numel].view(dst.permute(0, 2, 3, 1).shape).permute(0, 3, 1, 2) if dst.dim() == 4 else old[lead:lead + numel].view(dst.shape)
            want = torch.where(f.view(-1, *([1] * (dst.dim() - 1))), src, old_dst)
            assert torch.equal(dst.view(torch.int32) if dst.is_contiguous() else dst.contiguous().view(torch.int32),
                               want.contiguous().view(torch.int32)), (tuple(dst.shape), int(flags.sum()))
            assert torch.equal(whole[lead + numel:].view(torch.int32), old[lead + numel:].view(torch.int32))      # the canary
            assert torch.equal(whole[:lead].view(torch.int32), old[:lead].view(torch.int32))                      # and what lies in front
        assert all(torch.equal(s, c) for (_d, s, *_), c in zip(pairs, sources))


# ------------------------------------------------------------------------------------------------------------------ 4: export

@gpu
def test_detections_export_equals_to_prophesee_byte_for_byte():
    from sast_amd.labels import BBOX_DTYPE
    from sast_amd.online import export_detections
    M, A = 70, 80                                                  # more records than the 64 lanes of the wave that writes a row
    n_det = np.array([0, 1, M, M + 3, 1, M, M + 3, M + 3], np.int32)
    due = np.array([1, 1, 1, 1, 0, 0, 0, 1], np.uint8)
    R = len(n_det)
    rng = np.random.RandomState(5)
    det = np.full((R, A, 7), np.nan, np.float32)                   # rows past n_det are uninitialised memory in the product: never read
    for s, n in enumerate(n_det):
        xy = rng.uniform(-20, 300, size=(n, 2)).astype(np.float32)
        det[s, :n, 0:2] = xy
        det[s, :n, 2:4] = xy + rng.uniform(0.01, 157.3, size=(n, 2)).astype(np.float32)
        det[s, :n, 4:6] = rng.uniform(0, 1, size=(n, 2)).astype(np.float32)
        det[s, :n, 6] = rng.randint(0, 3, size=n)
    ends = np.array([600, 1200, 600 * 2 ** 33, 1800, 2400, 3000, 3600, 4200], np.int64)       # one end past 32 bits
    records = torch.full((R, M, 40), 0xCD, dtype=torch.uint8).cuda()
    counts, truncated = torch.full((R,), -1, dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    export_detections(torch.from_numpy(det).cuda(), torch.from_numpy(n_det).cuda(), _i64(ends), _u8(due), records, counts, truncated)
    got, got_n = records.cpu().numpy(), counts.cpu().numpy()
    for s in range(R):
        m = min(int(n_det[s]), M) if due[s] else 0
        assert got_n[s] == m, s
        want = OM.to_prophesee_records(det[s, :m], int(ends[s]), BBOX_DTYPE)
        assert got[s, :m].tobytes() == want.tobytes(), s
        assert np.array_equal(got[s, :m].reshape(-1).view(BBOX_DTYPE), want)
        assert (got[s, m:] == 0xCD).all(), s                       # nothing written past the count
    assert int(truncated.item()) == 3 * 2                           # rows 3 and 7; row 6 is cut as well but not due
    export_detections(torch.from_numpy(det).cuda(), torch.from_numpy(n_det).cuda(), _i64(ends), _u8(due), records, counts, truncated)
    assert int(truncated.item()) == 3 * 4                           # the counter accumulates


# ------------------------------------------------------------------------------------------------------------------ the detector

def _load(module, params):
    """oracle-named parameters into a sast_amd module (the names are the reference's but for the block's sub-layer list)"""
    sd = module.state_dict()
    new = {}
    for k in sd:
        kk = k
        for a, b in (("sub_layers.0.", "ls1."), ("sub_layers.2.", "norm2."), ("sub_layers.3.", "mlp."), ("sub_layers.4.", "ls2.")):
            kk = kk.replace(a, b)
        new[k] = sd[k] if kk.endswith("num_batches_tracked") else params[kk]
    module.load_state_dict(new, strict=True)


@pytest.fixture(scope="module")
def detector():
    from oracle import sast_oracle as O
    from sast_amd.config import backbone_config, to_attr
    from sast_amd.detection import YoloXDetector
    hw, part, E, nc = (128, 160), (4, 5), 32, 2
    cfg = to_attr({"backbone": backbone_config(hw, part, embed_dim=E, AMP=2e-2, ls_init_value=0.5),
                   "fpn": {"name": "PAFPN", "depth": 0.67, "in_stages": [2, 3, 4], "depthwise": False, "act": "silu"},
                   "head": {"name": "YoloX", "depthwise": False, "act": "silu", "num_classes": nc}})
    det = YoloXDetector(cfg).cuda()
    _load(det.backbone, O.init_backbone_params(O.BackboneCfg(in_res_hw=hw, partition_size=part, embed_dim=E, amp=2e-2), seed=41, ls_init=0.5))
    _load(det.fpn, O.init_pafpn_params((64, 128, 256), seed=42))
    _load(det.yolox_head, O.init_head_params((64, 128, 256), num_classes=nc, seed=43))
    with torch.no_grad():                                          # objectness around 0.9, classes around 0.5: scores on both sides of CONF
        for m in det.yolox_head.obj_preds:
            m.bias.fill_(2.0)
        for m in det.yolox_head.cls_preds:
            m.bias.fill_(0.0)
    return det.eval()


CONF, NMS, MAX_DET = 0.45, 0.45, 100


def _online(detector, W=2, **kw):
    from sast_amd.online import OnlineDetector
    return OnlineDetector(detector, _queue(), windows_per_step=W, max_det=MAX_DET, conf_thre=CONF, nms_thre=NMS, **kw)


def _push(od, parts, reset, final):
    cols, counts = _chunk(parts)
    od.push(*cols, counts, _u8(reset), _u8(final))


def _same(got, want):
    assert [s for s, _a in got] == [s for s, _a in want]
    for (s, a), (_s, b) in zip(got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), s


# ------------------------------------------------------------------------------------------------------------------ 5: end to end

@gpu
def test_online_detector_equals_a_host_scheduled_loop_of_the_same_batch(detector):
    """Equality, not closeness: both sides run the same kernels on the same [S, ...] inputs."""
    from sast_amd import functional as SF
    from sast_amd.labels import BBOX_DTYPE
    W = 2
    rounds, recs, _exact = _session(W, seed=21, max_rounds=14)
    od = _online(detector)
    whole = {False: [recs[0], recs[1], recs[2]], True: [recs[0], _recording(SECOND), recs[2]]}
    states, after_reset, n_records, n_placeholder = None, False, 0, 0
    with torch.no_grad():
        for r, (parts, reset, final, ends, due, _backlog, _next) in enumerate(rounds):
            _push(od, parts, reset, final)
            got = od.drain()
            # the reference loop: scheduled by the model, frames of the whole recordings, states selected by plain indexing on clones
            after_reset |= bool(reset[1])
            frames = _whole_frames(whole[after_reset], ends)
            if states is None:
                states = [(torch.zeros_like(h), torch.zeros_like(c)) for h, c in detector(frames[0], None)[2]]
            if reset.any():
                states = [(h.clone(), c.clone()) for h, c in states]
                for h, c in states:
                    h[torch.from_numpy(reset).bool().cuda()] = 0
                    c[torch.from_numpy(reset).bool().cuda()] = 0
            want = []
            for k in range(W):
                out, _losses, new, _p = detector(frames[k], states)
                rows = torch.from_numpy(due[k]).bool().cuda()
                nxt = []
                for (h, c), (h1, c1) in zip(states, new):
                    h, c = h.clone(), c.clone()
                    h[rows] = h1[rows]
                    c[rows] = c1[rows]
                    nxt.append((h, c))
                if not due[k].any():
                    n_placeholder += 1
                    assert all(torch.equal(a, b) for old, cur in zip(states, nxt) for a, b in zip(old, cur))
                states = nxt
                dets = SF.postprocess(out, 2, CONF, NMS)
                for s in range(S):
                    if due[k, s]:
                        rows7 = np.zeros((0, 7), np.float32) if dets[s] is None else dets[s][:MAX_DET].cpu().numpy()
                        want.append((s, OM.to_prophesee_records(rows7, int(ends[k, s]), BBOX_DTYPE)))
            _same(got, want)
            n_records += sum(len(a) for _s, a in want)
            for (h, c), (h2, c2) in zip(od.states, states):        # the held states, flagged and unflagged rows alike
                assert torch.equal(h, h2) and torch.equal(c, c2), r
    assert n_records > 0 and n_placeholder > 0 and after_reset
    assert od.errors()[:4] == (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------------------------ 6: independence

@gpu
def test_a_stream_does_not_depend_on_what_shares_its_batch(detector):
    """Stream 0's decoded predictions with rows 1 and 2 carrying one pair of recordings against the same stream beside another pair.  The
    other rows change how many token rows the batch keeps and with that the GEMMs' k-split, so sums may be taken in another order: the
    bar is the one tests/test_gpu_parity.py::test_yolox_head_eval_vs_golden holds decoded predictions to, 1e-4 of their largest value.
    Measured on the MI355X at this size: the two runs agree bit for bit (error 0 of a scale of 152)."""
    from conftest import record_error
    W = 2
    rounds_a, _recs, _e = _session(W, seed=31, rows=(FAST, SLOW_A, SLOW_B), reset_round=99, max_rounds=5)
    rounds_b, _recs, _e = _session(W, seed=31, rows=(FAST, OTHER_A, OTHER_B), reset_round=99, max_rounds=5)
    od_a, od_b = _online(detector), _online(detector)
    compared = 0
    for ra, rb in zip(rounds_a, rounds_b):
        assert all(np.array_equal(u, v) for u, v in zip(ra[0][0], rb[0][0])) and np.array_equal(ra[4][:, 0], rb[4][:, 0])     # row 0: the same chunks
        _push(od_a, ra[0], ra[1], ra[2])
        _push(od_b, rb[0], rb[1], rb[2])
        for k in range(W):
            if ra[4][k, 0]:
                a, b = od_a.predictions[k][0].float().cpu(), od_b.predictions[k][0].float().cpu()
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                record_error("test_a_stream_does_not_depend_on_what_shares_its_batch", f"round {compared}", err, scale, 1e-4)
                print(f"independence: max err {err:.3e} of scale {scale:.3e}")
                assert err <= 1e-4 * scale
                compared += 1
    assert compared >= 4
    od_a.drain(), od_b.drain()


# ------------------------------------------------------------------------------------------------------------------ 7: graph

@gpu
def test_captured_push_replays_on_new_chunks_like_the_eager_run(detector):
    W = 2
    rounds, _recs, _e = _session(W, seed=41, reset_round=2, max_rounds=4)
    rounds[3][2][2] = 1                                            # the last chunk is row 2's last: final, written into the same tensor
    eager = _online(detector)
    want = []
    for parts, reset, final, *_m in rounds:
        _push(eager, parts, reset, final)
        want.append(eager.drain())
    od = _online(detector)
    with pytest.raises(RuntimeError, match="one un-captured call is needed"):
        od.capture()
    cols, counts = _chunk(rounds[0][0])
    reset, final = _u8(rounds[0][1]), _u8(rounds[0][2])
    od.push(*cols, counts, reset, final)
    _same(od.drain(), want[0])
    od.capture()
    for (parts, rst, fin, *_m), expect in zip(rounds[1:], want[1:]):
        new_cols, new_counts = _chunk(parts)
        for dst, src in zip(cols + [counts, reset, final], new_cols + [new_counts, _u8(rst), _u8(fin)]):
            dst.copy_(src)
        od.replay()
        _same(od.drain(), expect)
    assert sum(len(a) for step in want for _s, a in step) > 0 and any(r[1].any() for r in rounds[1:])
    for (h, c), (h2, c2) in zip(od.states, eager.states):
        assert torch.equal(h, h2) and torch.equal(c, c2)
    assert od.errors() == eager.errors()


@gpu
def test_poll_never_waits_and_a_third_push_keeps_the_oldest_step(detector):
    rounds, _recs, _e = _session(2, seed=41, reset_round=2, max_rounds=4)
    eager, od = _online(detector), _online(detector)
    want = []
    for parts, reset, final, *_m in rounds:
        _push(eager, parts, reset, final)
        want += eager.drain()
        _push(od, parts, reset, final)                             # four pushes, two slots, no poll in between
    got = od.poll()                                                # whatever has landed, in order
    got += od.drain()
    _same(got, want)
    assert od.poll() == [] and od.drain() == []


# ------------------------------------------------------------------------------------------------------------------ 8: errors

def test_online_detector_refuses_count_windows_cpu_tensors_and_too_many_windows():
    from sast_amd.events import EventQueue
    from sast_amd.online import OnlineDetector

    class _Det:
        training = False

        class yolox_head:
            num_classes = 2

    with pytest.raises(ValueError, match="duration windows"):
        OnlineDetector(_Det(), EventQueue(S, CAP, num_events=300, **GEO), windows_per_step=2)
    with pytest.raises(ValueError):
        OnlineDetector(_Det(), _queue(), windows_per_step=65536 // S + 1)          # windows_per_step * S beyond what `frames` takes
    od = OnlineDetector(_Det(), _queue(), windows_per_step=2)
    with pytest.raises(RuntimeError, match="one un-captured call is needed"):
        od.capture()
    cols = [torch.zeros(S, 8, dtype=torch.int64) for _ in range(4)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        od.push(*cols, torch.zeros(S, dtype=torch.int64))
