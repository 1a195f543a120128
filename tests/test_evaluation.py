"""The device-resident Prophesee mAP evaluator (sast_amd/evaluation.py, csrc/k_eval.hip) and `postprocess_padded`.

Two yardsticks:
- tests/golden/prophesee_eval.npz: the image / annotation / result tables the reference's own to_prophesee, filter_boxes, _match_times
  and _to_coco_format give for seeded frames (tests/golden/make_golden_eval.py), for gen1, gen4 and gen4 with downsample_by_2;
- tests/coco_reference.py: a numpy fp64 restatement of pycocotools' COCOeval, pinned by tests/test_coco_reference.py.  pycocotools is
  not installed where these tests run, so parity with pycocotools itself is unpinned.
Bounds: tables and the precision table are exact (every precision entry is one correctly rounded fp64 division of integer counts); the
six summaries are means of at most 3030 values in [0, 1], so any summation order stays within 3030 * 2^-53 ~ 3.4e-13 < 1e-12."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coco_reference as CR  # noqa: E402
import make_golden_eval as G  # noqa: E402
from sast_amd import evaluation as E  # noqa: E402
from sast_amd.functional import postprocess, postprocess_padded  # noqa: E402

gpu = pytest.mark.gpu
SUMMARY_TOL = 1e-12
_FX = None


def _fixtures():
    global _FX
    if _FX is None:
        with np.load(os.path.join(GOLDEN, "prophesee_eval.npz")) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def _case(name):
    fx = _fixtures()
    return tuple(fx[f"{name}/{k}"] for k in ("labels", "counts", "det", "n_det"))


def _tables(name):
    fx = _fixtures()
    return {k: fx[f"{name}/{k}"] for k in G.TABLE_KEYS}


def _ref_available():
    sys.path.insert(0, GOLDEN)
    import _ref_import as R
    return os.path.isdir(os.path.join(R.REF_ROOT, "utils", "evaluation", "prophesee"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _evaluator(name, **caps):
    dataset, ds2, _hw, _seed = G.CASES[name]
    kw = dict(max_images=64, max_detections=4096, max_labels_per_frame=G.M_ROWS)
    kw.update(caps)
    return E.PropheseeEvaluator(dataset, ds2, **kw)


def _feed(ev, name, splits=None):
    labels, counts, det, n_det = (_dev(a) for a in _case(name))
    bounds = [0] + list(splits or []) + [labels.shape[0]]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        ev.add(labels[lo:hi], counts[lo:hi], det[lo:hi], n_det[lo:hi])


def _restatement(name):
    t = _tables(name)
    gt = {"image_id": t["gt_image_id"], "category_id": t["gt_category_id"], "bbox": t["gt_bbox"], "area": t["gt_area"]}
    dt = {"image_id": t["dt_image_id"], "category_id": t["dt_category_id"], "bbox": t["dt_bbox"], "area": t["dt_area"], "score": t["dt_score"]}
    return CR.evaluate(int(t["n_images"]), gt, dt, G.N_CLASSES[G.CASES[name][0]])


# ------------------------------------------------------------------------------------------------------------------- without a GPU
def test_eval_cpu_tensors_raise_no_fallback():
    ev = E.PropheseeEvaluator("gen1", False, 8, 64, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.add(torch.zeros(1, 4, 7), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 8, 7), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        postprocess_padded(torch.zeros(1, 8, 7), 2)
    assert not ev.has_data()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert ev.evaluate_buffer(240, 304) is None            # evaluator.py:58-60
    assert len(w) == 1 and "empty" in str(w[0].message)
    with pytest.raises(AssertionError):
        E.PropheseeEvaluator("gen5", False, 8, 64, 4)
    for bad in (dict(max_images=0), dict(max_detections=1 << 30), dict(max_labels_per_frame=129)):
        with pytest.raises(ValueError):
            E.PropheseeEvaluator("gen1", False, **{**dict(max_images=8, max_detections=64, max_labels_per_frame=4), **bad})
    assert (E.PropheseeEvaluator("gen4", True, 8, 64, 4).min_box_diag, E.PropheseeEvaluator("gen4", True, 8, 64, 4).min_box_side) == (30, 10)
    assert np.array_equal(E.IOU_THRS, CR.IOU_THRS) and np.array_equal(E.REC_THRS, CR.REC_THRS)


def test_eval_entry_points_declared_bound_and_exported():
    import ctypes as C
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_eval_")]
    assert sorted(names) == ["sast_eval_accumulate", "sast_eval_add", "sast_eval_reset", "sast_eval_sort_ws_bytes"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    with open(_lib.HEADER_PATH) as f:
        src = f.read()
    assert f"#define SAST_EVAL_STATE_WORDS {_lib.EVAL_STATE_WORDS}" in src and f"#define SAST_EVAL_MAX_CLASSES {_lib.EVAL_MAX_CLASSES}" in src
    assert f"#define SAST_EVAL_IOU_THRS {_lib.EVAL_IOU_THRS}" in src and f"#define SAST_EVAL_REC_THRS {_lib.EVAL_REC_THRS}" in src
    from sast_amd import build as B
    assert "k_eval.hip" in B.SOURCES and B.SOURCE_FLAGS["k_eval.hip"] == ["-ffp-contract=off"]
    # bad arguments are refused on the host, before anything is enqueued (no device needed)
    a = _lib.SastEvalArgs()
    assert lib.sast_eval_add(C.byref(a), None) == -22 and lib.sast_eval_reset(C.byref(a), None) == -22
    assert lib.sast_eval_accumulate(C.byref(a), None) == -22 and lib.sast_eval_add(None, None) == -22
    assert lib.sast_eval_sort_ws_bytes(0) == 0 and lib.sast_eval_sort_ws_bytes(1 << 30) == 0


def test_fixture_covers_the_corner_cases():
    seen = set()
    for name, (dataset, ds2, _hw, _seed) in G.CASES.items():
        labels, counts, det, n_det = _case(name)
        t = _tables(name)
        K = G.N_CLASSES[dataset]
        diag, side = G.thresholds(dataset, ds2)
        N = labels.shape[0]
        lab_t = labels[:, 0, 0].astype(np.int64)
        w, h = labels[..., 3], labels[..., 4]
        valid = np.arange(labels.shape[1])[None, :] < counts[:, None]
        ok = valid & (labels[..., 0].astype(np.int64) > 500000) & (w * w + h * h >= diag ** 2) & (w >= side) & (h >= side)
        dw, dh = det[..., 2] - det[..., 0], det[..., 3] - det[..., 1]
        dvalid = np.arange(det.shape[1])[None, :] < n_det[:, None]
        dok = dvalid & (dw * dw + dh * dh >= diag ** 2) & (dw >= side) & (dh >= side)
        assert int(t["n_images"]) == int(ok.any(1).sum()) and len(t["gt_id"]) == int(ok.sum())
        assert len(t["dt_score"]) == int(dok[ok.any(1)].sum())
        for n in range(N):
            if counts[n] > 0 and lab_t[n] <= 500000 and n_det[n] > 0:
                seen.add("before 0.5 s")
            if counts[n] > 0 and lab_t[n] > 500000 and not ok[n].any() and dok[n].any():
                seen.add("emptied by the filter, with detections")
            if counts[n] == 0 and n_det[n] > 0:
                seen.add("counts == 0")
            if ok[n].any() and max(int((dok[n] & (det[n, :, 6] == k)).sum()) for k in range(K)) > 100:
                seen.add("more than 100 of one category")
            if ok[n].any() and labels[n, 0, 0] > 2 ** 31:
                seen.add("timestamp beyond int32")
        if (valid & (w * w + h * h == diag ** 2)).any() and (valid & (w == side)).any() and (dvalid & (dh == side)).any():
            seen.add("on the thresholds")
        if (valid & (w * w + h * h < diag ** 2) & (w >= side) & (h >= side)).any() and (valid & (w == side - 0.25)).any():
            seen.add("just under the thresholds")
        s = t["dt_score"]
        img = t["dt_image_id"]
        same = s[:, None] == s[None, :]
        if (same & (img[:, None] == img[None, :]) & ~np.eye(len(s), dtype=bool)).any() and (same & (img[:, None] != img[None, :])).any():
            seen.add("equal scores within and across frames")
        if any(k + 1 not in set(t["gt_category_id"]) and k + 1 in set(t["dt_category_id"]) for k in range(K)):
            seen.add("a category without labels")
        for i in range(len(s)):
            g = np.nonzero((t["gt_image_id"] == img[i]) & (t["gt_category_id"] == t["dt_category_id"][i]))[0]
            ious = [CR.iou_xywh(t["dt_bbox"][i], t["gt_bbox"][j]) for j in g]
            if any(v == 0.5 for v in ious):
                seen.add("IoU equal to a threshold")
            if ious and max(ious) >= 0.5:
                a = t["gt_area"][g[int(np.argmax(ious))]]
                if a > 1024:                  # outside the small range [0, 32^2]: matched there all the same, and ignored
                    seen.add("best overlap out of range")
    assert seen == {"before 0.5 s", "emptied by the filter, with detections", "counts == 0", "more than 100 of one category",
                    "timestamp beyond int32", "on the thresholds", "just under the thresholds", "equal scores within and across frames",
                    "a category without labels", "IoU equal to a threshold", "best overlap out of range"}


def test_fixture_inputs_regenerate_without_the_reference():
    for name in G.CASES:
        for got, want in zip(G.case_inputs(name), _case(name)):
            assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.skipif(not _ref_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_eval_fixture():
    fx = _fixtures()
    new = G.build()
    assert sorted(new) == sorted(fx)
    for k in fx:
        assert new[k].dtype == fx[k].dtype and np.array_equal(new[k], fx[k]), k


def test_restatement_on_the_fixture_is_a_real_measurement():
    """the fixture is not degenerate: AP, AP_50, AP_75 and the size classes that exist are strictly between 0 and 1 (gen4's filter
    leaves no box of at most 32 x 32 pixels: its AP_S is -1), and the precision table holds -1, 0 and fractions"""
    for name in G.CASES:
        stats, prec = _restatement(name)
        print(name, stats)
        assert all(0.0 < stats[k] < 1.0 for k in ("AP", "AP_50", "AP_75", "AP_M", "AP_L")), (name, stats)
        assert (stats["AP_S"] == -1.0) if name == "gen4" else (0.0 < stats["AP_S"] < 1.0), (name, stats)
        assert ((prec > 0) & (prec < 1)).any() and (prec == 0).any()
    assert (_restatement("gen4")[1][:, :, 1, :] == -1).all()       # the category without labels


# ------------------------------------------------------------------------------------------------------------------------ on the GPU
@gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_tables_equal_the_reference_exactly(name):
    ev = _evaluator(name)
    _feed(ev, name)
    got, want = ev.tables(), _tables(name)
    assert len(got["image_t"]) == int(want["n_images"])
    for k in ("gt_image_id", "gt_category_id", "gt_bbox", "gt_area", "dt_image_id", "dt_category_id", "dt_bbox", "dt_area"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["dt_score"].astype(np.float64), want["dt_score"])
    labels, counts, _d, _n = _case(name)
    lab_t = labels[:, 0, 0].astype(np.int64)
    w, h = labels[..., 3], labels[..., 4]
    diag, side = G.thresholds(*G.CASES[name][:2])
    ok = (np.arange(labels.shape[1])[None, :] < counts[:, None]) & (labels[..., 0].astype(np.int64) > 500000) & (w * w + h * h >= diag ** 2) \
        & (w >= side) & (h >= side)
    assert np.array_equal(got["image_t"], lab_t[ok.any(1)])          # int64(fp32 t), box_loading.py:74


@gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_precision_table_exact_and_summaries_within_bound(name):
    ev = _evaluator(name)
    _feed(ev, name)
    hw = G.CASES[name][2]
    got = ev.evaluate_buffer(*hw)
    want, want_prec = _restatement(name)
    prec = ev.precision().cpu().numpy()
    assert prec.dtype == np.float64 and prec.shape == want_prec.shape == (10, 101, G.N_CLASSES[G.CASES[name][0]], 4)
    diff = prec != want_prec
    print(name, "precision entries that differ:", int(diff.sum()), "of", prec.size)
    for k in CR.OUT_KEYS:
        print(name, k, got[k], want[k], abs(got[k] - want[k]))
    assert not diff.any(), np.argwhere(diff)[:8]
    assert list(got) == list(CR.OUT_KEYS) and all(type(v) is float for v in got.values())
    for k in CR.OUT_KEYS:
        assert abs(got[k] - want[k]) <= SUMMARY_TOL, (k, got[k], want[k])


@gpu
def test_results_do_not_depend_on_how_frames_are_split_and_repeat_bitwise():
    name = "gen4_ds2"
    runs = []
    for splits in (None, None, [5, 13], list(range(1, G.N_FRAMES))):
        ev = _evaluator(name)
        _feed(ev, name, splits)
        stats = ev.evaluate_buffer(360, 640)
        runs.append((stats, ev.precision().cpu().numpy(), ev.tables()))
    for stats, prec, tab in runs[1:]:
        assert stats == runs[0][0]
        assert np.array_equal(prec.view(np.int64), runs[0][1].view(np.int64))
        for k in tab:
            assert np.array_equal(tab[k], runs[0][2][k]), k
    # the same evaluator after reset_buffer gives the same bits again; without the reset the frames are there twice
    ev = _evaluator(name)
    _feed(ev, name)
    first = ev.evaluate_buffer(360, 640)
    again = ev.evaluate_buffer(360, 640)
    assert first == again == runs[0][0]
    _feed(ev, name)
    assert len(ev.tables()["image_t"]) == 2 * len(runs[0][2]["image_t"])
    ev.reset_buffer()
    assert not ev.has_data()
    _feed(ev, name, [7])
    assert ev.has_data() and ev.evaluate_buffer(360, 640) == runs[0][0]
    assert np.array_equal(ev.precision().cpu().numpy().view(np.int64), runs[0][1].view(np.int64))


@gpu
def test_capacity_overflow_is_counted_and_raised():
    for caps, word in ((dict(max_images=5), "max_images=5"), (dict(max_detections=100), "max_detections=100"),
                       (dict(max_labels_per_frame=3), "max_labels_per_frame=3")):
        ev = _evaluator("gen1", **caps)
        _feed(ev, "gen1")
        with pytest.raises(OverflowError, match=word):
            ev.evaluate_buffer(240, 304)
        with pytest.raises(RuntimeError):
            ev.precision()
    t = _tables("gen1")
    ev = _evaluator("gen1", max_images=int(t["n_images"]), max_detections=len(t["dt_score"]), max_labels_per_frame=G.M_ROWS)   # an exact fit
    _feed(ev, "gen1")
    assert abs(ev.evaluate_buffer(240, 304)["AP"] - _restatement("gen1")[0]["AP"]) <= SUMMARY_TOL


@gpu
def test_no_detection_in_any_image_gives_six_zeros():
    labels, counts, det, n_det = _case("gen1")
    ev = _evaluator("gen1")
    ev.add(_dev(labels), _dev(counts), _dev(det), _dev(np.zeros_like(n_det)))
    assert ev.evaluate_buffer(240, 304) == {k: 0.0 for k in CR.OUT_KEYS}
    # detections only in frames that are no images
    ev.reset_buffer()
    keep = np.zeros_like(n_det)
    keep[:4] = n_det[:4]
    ev.add(_dev(labels), _dev(counts), _dev(det), _dev(keep))
    assert ev.evaluate_buffer(240, 304) == {k: 0.0 for k in CR.OUT_KEYS} and len(ev.tables()["dt_score"]) == 0


@gpu
def test_add_refuses_bad_tensors():
    ev = _evaluator("gen1")
    labels, counts, det, n_det = (_dev(a) for a in _case("gen1"))
    with pytest.raises(TypeError):
        ev.add(labels.double(), counts, det, n_det)
    with pytest.raises(TypeError):
        ev.add(labels, counts.long(), det, n_det)
    with pytest.raises(TypeError):
        ev.add(labels, counts, det[:4], n_det)
    with pytest.raises(TypeError):
        ev.add(labels, counts, det[..., :6], n_det)
    with pytest.raises(RuntimeError):
        ev.tables()
    assert not ev.has_data()


def _prediction(seed, B, A, nc):
    rs = np.random.RandomState(seed)
    p = np.zeros((B, A, 5 + nc), np.float32)
    p[..., 0], p[..., 1] = rs.uniform(20, 280, (B, A)), rs.uniform(20, 220, (B, A))
    p[..., 2], p[..., 3] = rs.uniform(4, 80, (B, A)), rs.uniform(4, 80, (B, A))
    p[..., 4:] = rs.uniform(0, 1, (B, A, 1 + nc))
    return p


@gpu
@pytest.mark.parametrize("conf,agnostic", [(0.001, False), (0.3, False), (0.3, True), (2.0, False)])
def test_postprocess_padded_equals_postprocess_row_for_row(conf, agnostic):
    pred = _dev(_prediction(5, 3, 600, 2))
    want = postprocess(pred, 2, conf_thre=conf, nms_thre=0.45, class_agnostic=agnostic)
    out, n_out = postprocess_padded(pred, 2, conf_thre=conf, nms_thre=0.45, class_agnostic=agnostic)
    assert out.shape == (3, 600, 7) and out.dtype == torch.float32 and n_out.dtype == torch.int32 and n_out.shape == (3,)
    for b, w in enumerate(want):
        n = int(n_out[b])
        assert n == (0 if w is None else w.shape[0])
        if n:
            assert torch.equal(out[b, :n], w)
    if conf == 2.0:
        assert int(n_out.sum()) == 0


@gpu
def test_head_postprocess_and_add_in_one_graph():
    """YOLOX head + postprocess_padded + PropheseeEvaluator.add captured once after an eager warm-up: the capture would fail on any host
    synchronisation.  Replayed, it fills the buffer with the same metrics as the eager calls, for the features of each replay."""
    from sast_amd.detection import YOLOXHead
    torch.manual_seed(7)
    B, nc, chans = 4, 2, (16, 32, 64)
    head = YOLOXHead(num_classes=nc, strides=(8, 16, 32), in_channels=chans).cuda().eval()
    feats_a = tuple(torch.randn(B, c, 128 // s, 160 // s, device="cuda") * 2 for c, s in zip(chans, (8, 16, 32)))
    feats_b = tuple(torch.randn(B, c, 128 // s, 160 // s, device="cuda") * 2 for c, s in zip(chans, (8, 16, 32)))
    feats = tuple(f.clone() for f in feats_a)
    lab = np.zeros((B, 6, 7), np.float32)
    cnt = np.array([3, 0, 6, 2], np.int32)
    rs = np.random.RandomState(3)
    for b in range(B):
        for i in range(cnt[b]):
            lab[b, i] = (700000 + b, rs.randint(0, 100), rs.randint(0, 80), rs.randint(24, 60), rs.randint(24, 48), rs.randint(nc), 1)
    lab_d, cnt_d = _dev(lab), _dev(cnt)
    ev = E.PropheseeEvaluator("gen1", False, max_images=32, max_detections=8192, max_labels_per_frame=8)

    def step():
        with torch.no_grad():
            pred, _ = head(feats)
            det, n_det = postprocess_padded(pred, nc, conf_thre=0.0, nms_thre=0.45)
            ev.add(lab_d, cnt_d, det, n_det)
        return n_det

    def eager(src):
        for f, s in zip(feats, src):
            f.copy_(s)
        ev.reset_buffer()
        n = step()
        stats = ev.evaluate_buffer(128, 160)
        return stats, ev.precision().cpu().numpy(), ev.tables(), n.cpu().numpy()

    want_a, want_b = eager(feats_a), eager(feats_b)
    assert want_a[3].sum() > 0 and len(want_a[2]["dt_score"]) > 0 and len(want_a[2]["image_t"]) == 3
    assert not np.array_equal(want_a[2]["dt_bbox"], want_b[2]["dt_bbox"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for src, want in ((feats_a, want_a), (feats_b, want_b), (feats_a, want_a)):
        for f, v in zip(feats, src):
            f.copy_(v)
        ev.reset_buffer()
        g.replay()
        stats = ev.evaluate_buffer(128, 160)
        assert stats == want[0]
        assert np.array_equal(ev.precision().cpu().numpy().view(np.int64), want[1].view(np.int64))
        tab = ev.tables()
        for k in tab:
            assert np.array_equal(tab[k], want[2][k]), k
    g.replay()                                  # a second replay without a reset appends the same frames again
    assert len(ev.tables()["image_t"]) == 6
