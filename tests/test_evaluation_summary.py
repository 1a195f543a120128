"""The full COCO summary of the device evaluator: `PropheseeEvaluator.summary / coco_eval / per_class` (sast_amd/evaluation.py) and
sast_evsum_accumulate (csrc/k_eval.hip) -- COCOeval's precision, recall and score tables at maxDets [1, 10, 100] and its twelve stats.

Yardstick: tests/coco_reference_full.py (pinned by tests/test_coco_reference_full.py) applied to the run's own tables.  pycocotools is
not installed where these tests run: parity with pycocotools itself is unpinned.
Bounds: every table entry is exact -- a precision or recall is one correctly rounded fp64 division of integer counts, a score is an fp32
score widened -- so the tables are compared as bits (int64 views).  The twelve stats and the per-category numbers are means of at most
3030 values in [-1, 1]: any summation order stays within 3030 * 2^-53 ~ 3.4e-13 < SUMMARY_TOL = 1e-12 (the bar of
tests/test_evaluation.py).  The fixture separates the three maxDets (tests/test_coco_reference_full.py asserts it): every case has a
group above 100 detections and many above 10, so a kernel that ignores a record's rank cannot pass."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coco_reference as CR  # noqa: E402
import coco_reference_full as CF  # noqa: E402
import make_golden_eval as G  # noqa: E402
import make_golden_eval_recordings as GR  # noqa: E402
import recording_model as RM  # noqa: E402
from sast_amd import _lib  # noqa: E402
from sast_amd import evaluation as E  # noqa: E402

gpu = pytest.mark.gpu
SUMMARY_TOL = 1e-12
CAPS = dict(max_images=64, max_detections=8192, max_labels_per_frame=G.M_ROWS)
KNOB = "SAST_EVAL_ACC_CHUNK"
TABLES = ("precision", "recall", "scores")
_FX = None
_ONE = {}


def _case(name):
    global _FX
    if _FX is None:
        with np.load(os.path.join(GOLDEN, "prophesee_eval.npz")) as z:
            _FX = {k: z[k] for k in z.files}
    return tuple(_FX[f"{name}/{k}"] for k in ("labels", "counts", "det", "n_det"))


def _evaluator(name, **caps):
    dataset, ds2, _hw, _seed = G.CASES[name]
    return E.PropheseeEvaluator(dataset, ds2, **{**CAPS, **caps})


def _feed(ev, name, lo=0, hi=None):
    labels, counts, det, n_det = (torch.from_numpy(np.ascontiguousarray(a[lo:hi])).cuda() for a in _case(name))
    ev.add(labels, counts, det, n_det)


def _result(ev, hw):
    six = ev.evaluate_buffer(*hw)
    return {"six": six, "summary": ev.summary(), "per_class": ev.per_class(), "prec100": ev.precision().cpu().numpy(),
            **{k: v.cpu().numpy() for k, v in ev.coco_eval().items()}}


def _one(name, times=1):
    """one evaluator fed the whole case `times` times, and the restatement on its tables: computed once, shared, never changed"""
    if (name, times) not in _ONE:
        ev = _evaluator(name)
        for _ in range(times):
            _feed(ev, name)
        got = _result(ev, G.CASES[name][2])
        got["ref"] = CF.evaluate(*RM.coco_inputs(ev.tables()), len(ev.classes)) if times == 1 else None
        _ONE[(name, times)] = got
    return _ONE[(name, times)]


def _same_bits(got, want, what=""):
    for k in TABLES:
        assert got[k].dtype == want[k].dtype == np.float64 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), (what, k)


def _same_result(got, want, what=""):
    _same_bits(got, want, what)
    assert got["six"] == want["six"] and got["summary"] == want["summary"] and got["per_class"] == want["per_class"], what


def _check_against_restatement(got, ref_stats, ref, classes, what):
    K = len(classes)
    assert got["precision"].shape == got["scores"].shape == (10, 101, K, 4, 3) and got["recall"].shape == (10, K, 4, 3)
    for k in TABLES:
        diff = got[k].view(np.int64) != ref[k].view(np.int64)
        print(what, k, "entries whose bits differ:", int(diff.sum()), "of", diff.size)
    ref_pc = CF.per_class(ref, classes)
    for k in CF.STAT_KEYS:
        print(what, k, got["summary"][k], ref_stats[k], abs(got["summary"][k] - ref_stats[k]))
    for n in classes:
        print(what, n, got["per_class"][n], ref_pc[n])
    _same_bits(got, ref, what)
    assert list(got["summary"]) == list(CF.STAT_KEYS) and all(type(v) is float for v in got["summary"].values())
    for k in CF.STAT_KEYS:
        assert abs(got["summary"][k] - ref_stats[k]) <= SUMMARY_TOL, (what, k)
    assert list(got["per_class"]) == list(classes)
    for n in classes:
        assert list(got["per_class"][n]) == list(CF.CLASS_KEYS)
        for k in CF.CLASS_KEYS:
            assert abs(got["per_class"][n][k] - ref_pc[n][k]) <= SUMMARY_TOL, (what, n, k)
    assert all(got["summary"][k] == got["six"][k] for k in CR.OUT_KEYS), what          # exactly evaluate_buffer's numbers
    assert np.array_equal(got["precision"][..., 2].view(np.int64), got["prec100"].view(np.int64)), what


# ------------------------------------------------------------------------------------------------------------------- without a GPU
def test_summary_entry_points_declared_bound_exported_and_refusing():
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_evsum_")]
    assert sorted(names) == ["sast_evsum_accumulate", "sast_evsum_ws_bytes"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert _lib.EVSUM_MAXDETS == len(E.MAX_DETS) == len(CF.MAX_DETS) == 3 and _lib.EVSUM_STATS == len(E.SUMMARY_KEYS) == 12
    assert E.SUMMARY_KEYS == CF.STAT_KEYS and E.CLASS_KEYS == CF.CLASS_KEYS and E.MAX_DETS == CF.MAX_DETS
    EINVAL = -22
    a, s = _lib.SastEvalArgs(), _lib.SastEvSumArgs()
    assert lib.sast_evsum_accumulate(None, None, None) == EINVAL and lib.sast_evsum_accumulate(C.byref(a), C.byref(s), None) == EINVAL
    # a buffer and a summary that pass every check, then one argument at a time taken away (the pointers are never followed on the host)
    for i, f in enumerate("state rec_key rec_match rec_ign sorted rec_thr".split()):
        setattr(a, f, (1 << 20) + 4096 * i)
    a.K, a.max_images, a.max_labels_per_frame, a.max_detections = 2, 8, 4, 64
    for i, f in enumerate("precision scores recall stats per_class ws".split()):
        setattr(s, f, (1 << 24) + 4096 * i)
    s.ws_bytes = lib.sast_evsum_ws_bytes(64)
    assert s.ws_bytes > 0 and s.ws_bytes % (3 * 1024) == 0
    assert lib.sast_evsum_accumulate(None, C.byref(s), None) == EINVAL and lib.sast_evsum_accumulate(C.byref(a), None, None) == EINVAL
    for obj, field, value in ((a, "sorted", 0), (a, "rec_thr", 0), (a, "rec_ign", 0), (a, "state", 0), (a, "K", 5), (s, "precision", 0),
                              (s, "scores", 0), (s, "recall", 0), (s, "stats", 0), (s, "per_class", 0), (s, "ws", 0), (s, "ws", (1 << 24) + 4),
                              (s, "ws_bytes", s.ws_bytes - 1)):
        keep = getattr(obj, field)
        setattr(obj, field, value)
        assert lib.sast_evsum_accumulate(C.byref(a), C.byref(s), None) == EINVAL, field
        setattr(obj, field, keep)
    assert lib.sast_evsum_ws_bytes(0) == 0 and lib.sast_evsum_ws_bytes(1 << 30) == 0


def test_summary_methods_follow_evaluate_buffer_and_have_no_cpu_path():
    ev = E.PropheseeEvaluator("gen1", False, 8, 64, 4)
    for method in (ev.summary, ev.coco_eval, ev.per_class):
        with pytest.raises(RuntimeError, match="evaluate_buffer"):
            method()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.add(torch.zeros(1, 4, 7), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 8, 7), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="evaluate_buffer"):
        ev.summary()


# ------------------------------------------------------------------------------------------------------------------------ on the GPU
@gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_tables_stats_and_per_class_equal_the_restatement(name):
    got = _one(name)
    ref_stats, ref = got["ref"]
    _check_against_restatement(got, ref_stats, ref, E.CLASSES[G.CASES[name][0]], name)
    s = got["summary"]
    assert 0.0 < s["AR_1"] < s["AR_10"] < s["AR_100"] < 1.0                            # the rank decides
    assert all((got["precision"][..., i] != got["precision"][..., i + 1]).sum() > 1000 for i in (0, 1))


@gpu
def test_summary_bits_do_not_depend_on_the_chunk_length():
    name = "gen4"
    want = _one(name)
    before = os.environ.get(KNOB)
    try:
        ev = _evaluator(name)
        _feed(ev, name)
        n = int(ev._t["state"][4:8].cpu().numpy().max())          # the largest record count of a category
        assert n >= 3 * 64 - 63
        for chunk in (1, 7, 64, n - 1, n, n + 1, 1 << 20):
            os.environ[KNOB] = str(chunk)
            _lib.reload_knobs()
            got = _result(ev, G.CASES[name][2])
            assert _lib.knobs()[KNOB] == chunk
            for k in TABLES:
                print(name, "chunk", chunk, k, "entries whose bits differ:", int((got[k].view(np.int64) != want[k].view(np.int64)).sum()))
            _same_result(got, want, chunk)
    finally:
        if before is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = before
        _lib.reload_knobs()


@gpu
def test_merge_and_import_equal_one_evaluator():
    name = "gen4_ds2"
    hw = G.CASES[name][2]
    a, b, c = _evaluator(name), _evaluator(name), _evaluator(name)
    _feed(a, name, 0, 7), _feed(b, name, 7, None), _feed(c, name, 0, 7)
    a.merge(b)
    c.import_buffer(b.export_buffer())
    want = _one(name)
    _same_result(_result(a, hw), want, "merge")
    _same_result(_result(c, hw), want, "import_buffer(export_buffer())")
    # a summary made before a merge is not handed out after it
    with_old = _evaluator(name)
    _feed(with_old, name, 0, 7)
    with_old.evaluate_buffer(*hw)
    old = with_old.summary()
    with_old.merge(b)
    with pytest.raises(RuntimeError):
        with_old.summary()
    got = _result(with_old, hw)
    _same_result(got, want, "merge after a summary")
    assert old != got["summary"]


@gpu
def test_merge_of_a_twin_equals_feeding_twice():
    name = "gen1"
    a, b = _evaluator(name), _evaluator(name)
    _feed(a, name), _feed(b, name)
    a.merge(b)
    _same_result(_result(a, G.CASES[name][2]), _one(name, 2), "twin")
    _same_result(_result(b, G.CASES[name][2]), _one(name), "the source is left as it was")


@gpu
@pytest.mark.parametrize("tol", GR.TOLS)
def test_recordings_equal_the_restatement(tol):
    from test_recording_model import fixture_rows
    rows = fixture_rows()
    ev = E.PropheseeEvaluator("gen1", False, max_images=64, max_detections=4096, max_labels_per_frame=12)
    packed = []
    for side in (0, 1):
        recs = [r[side] for r in rows]
        w = np.zeros((len(recs), max(len(r) for r in recs) + 3, 10), np.int32)
        for s, r in enumerate(recs):
            w[s, :len(r)] = RM.words(r)
        packed += [torch.from_numpy(w).cuda(), torch.tensor([len(r) for r in recs], dtype=torch.int64).cuda()]
    ev.add_recordings(*packed, time_tol_us=tol)
    got = _result(ev, (240, 304))
    ref_stats, ref = CF.evaluate(*RM.coco_inputs(ev.tables()), GR.K)
    assert ref is not None and got["six"]["AP"] > 0
    _check_against_restatement(got, ref_stats, ref, ev.classes, f"recordings tol {tol}")


@gpu
def test_no_detection_anywhere_gives_twelve_zeros():
    labels, counts, det, n_det = (torch.from_numpy(a).cuda() for a in _case("gen1"))
    ev = _evaluator("gen1")
    ev.add(labels, counts, det, torch.zeros_like(n_det))
    with pytest.raises(RuntimeError):
        ev.summary()                                              # before evaluate_buffer
    assert ev.evaluate_buffer(240, 304) == {k: 0.0 for k in CR.OUT_KEYS}
    s = ev.summary()
    assert s == {k: 0.0 for k in CF.STAT_KEYS} and list(s) == list(CF.STAT_KEYS)
    ref = CF.accumulate(*RM.coco_inputs(ev.tables()), 2)
    got = {k: v.cpu().numpy() for k, v in ev.coco_eval().items()}
    _same_bits(got, ref, "no detection")
    assert {0.0} <= set(np.unique(got["recall"])) <= {-1.0, 0.0} and {0.0} <= set(np.unique(got["scores"])) <= {-1.0, 0.0}
    pc, ref_pc = ev.per_class(), CF.per_class(ref, ev.classes)
    assert pc == ref_pc and all(v in (0.0, -1.0) for d in pc.values() for v in d.values())
