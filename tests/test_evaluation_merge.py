"""Merging evaluation buffers (PropheseeEvaluator.merge / export_buffer / import_buffer / all_gather, sast_evmerge_append) and the
chunk-parallel accumulate of csrc/k_eval.hip.

The yardstick of a merge is ONE evaluator fed the same frames in the same order: stats, the precision table as bits and every table are
equal, score ties included (tests/golden/prophesee_eval.npz has hundreds of equal scores per case, and the record index that breaks
them is what a merge rebases).  The yardstick of the chunked accumulate is tests/coco_reference.py on the run's own tables: every entry
of the precision table is one correctly rounded fp64 division of integer counts, so it is compared as bits, for every chunk length."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coco_reference as CR  # noqa: E402
import make_golden_eval as G  # noqa: E402
from sast_amd import _lib  # noqa: E402
from sast_amd import evaluation as E  # noqa: E402

gpu = pytest.mark.gpu
CAPS = dict(max_images=64, max_detections=8192, max_labels_per_frame=G.M_ROWS)
KNOB = "SAST_EVAL_ACC_CHUNK"
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
    if labels.shape[0]:
        ev.add(labels, counts, det, n_det)


def _result(ev, name):
    stats = ev.evaluate_buffer(*G.CASES[name][2])
    return stats, ev.precision().cpu().numpy(), ev.tables()


def _one(name, times=1):
    """one evaluator fed the whole case `times` times: computed once, shared, never changed"""
    if (name, times) not in _ONE:
        ev = _evaluator(name)
        for _ in range(times):
            _feed(ev, name)
        _ONE[(name, times)] = _result(ev, name)
    return _ONE[(name, times)]


def _assert_same(got, want):
    assert got[0] == want[0]
    assert got[1].shape == want[1].shape and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    assert sorted(got[2]) == sorted(want[2])
    for k in want[2]:
        assert got[2][k].dtype == want[2][k].dtype and np.array_equal(got[2][k], want[2][k]), k


def _restate(tab, K):
    gt = {"image_id": tab["gt_image_id"], "category_id": tab["gt_category_id"], "bbox": tab["gt_bbox"], "area": tab["gt_area"]}
    dt = {"image_id": tab["dt_image_id"], "category_id": tab["dt_category_id"], "bbox": tab["dt_bbox"], "area": tab["dt_area"],
          "score": tab["dt_score"].astype(np.float64)}
    return CR.evaluate(len(tab["image_t"]), gt, dt, K)


def _fake_args(base):
    """arguments that pass every host-side check of a lone buffer; the pointers are never followed on the host"""
    a = _lib.SastEvalArgs()
    for i, f in enumerate("state gt_box gt_cls gt_img img_t det_box det_cls det_img rec_key rec_match rec_ign".split()):
        setattr(a, f, base + 4096 * i)
    a.K, a.min_diag2, a.min_side = 2, 900.0, 10.0
    a.max_images, a.max_labels_per_frame, a.max_detections = 8, 4, 64
    return a


# ------------------------------------------------------------------------------------------------------------------- without a GPU
def test_merge_entry_point_declared_bound_exported_and_refusing():
    assert "sast_evmerge_append" in _lib.declared_symbols() and "sast_evmerge_append" in _lib._SIGNATURES
    lib = _lib.lib()
    assert hasattr(lib, "sast_evmerge_append")
    EINVAL = -22
    a, b = _fake_args(1 << 20), _fake_args(1 << 24)
    assert lib.sast_evmerge_append(None, None, None) == EINVAL
    assert lib.sast_evmerge_append(C.byref(a), None, None) == EINVAL and lib.sast_evmerge_append(None, C.byref(b), None) == EINVAL
    assert lib.sast_evmerge_append(C.byref(a), C.byref(a), None) == EINVAL                # dst == src
    b.state = a.state
    assert lib.sast_evmerge_append(C.byref(a), C.byref(b), None) == EINVAL                # one state for both
    for field, value in (("K", 3), ("min_diag2", 225.0), ("min_side", 5.0), ("max_labels_per_frame", 5), ("gt_box", 0), ("img_t", 0),
                         ("rec_key", 0), ("state", 0)):
        b = _fake_args(1 << 24)
        setattr(b, field, value)
        assert lib.sast_evmerge_append(C.byref(a), C.byref(b), None) == EINVAL, field
    # the workspace query keeps refusing what it refused
    assert lib.sast_eval_sort_ws_bytes(0) == 0 and lib.sast_eval_sort_ws_bytes(1 << 30) == 0


def test_merge_cpu_tensors_and_blobs_raise_no_fallback():
    ev, other = E.PropheseeEvaluator("gen1", False, 8, 64, 4), E.PropheseeEvaluator("gen1", False, 8, 64, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        other.add(torch.zeros(1, 4, 7), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 8, 7), torch.zeros(1, dtype=torch.int32))
    ev.merge(other)                                       # never allocated: a no-op, on any machine
    assert not ev.has_data()
    blob = {"state": torch.zeros(32, dtype=torch.int32), "dataset": "gen1", "downsample_by_2": False, "max_labels_per_frame": 4,
            "img_t": torch.zeros(0, dtype=torch.int64), "gt_box": torch.zeros(0, 4), "gt_cls": torch.zeros(0, dtype=torch.int32),
            "gt_img": torch.zeros(0, dtype=torch.int32), "det_box": torch.zeros(0, 5), "det_cls": torch.zeros(0, dtype=torch.int32),
            "det_img": torch.zeros(0, dtype=torch.int32), "rec_key": torch.zeros(0, dtype=torch.int64),
            "rec_match": torch.zeros(0, dtype=torch.int64), "rec_ign": torch.zeros(0, dtype=torch.int64)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.import_buffer(blob)
    with pytest.raises(ValueError):
        ev.merge(ev)
    with pytest.raises(ValueError):
        ev.merge(E.PropheseeEvaluator("gen4", False, 8, 64, 4))
    with pytest.raises(ValueError):
        ev.merge(E.PropheseeEvaluator("gen1", True, 8, 64, 4))
    with pytest.raises(RuntimeError):
        ev.export_buffer()                                # nothing was added
    ev.all_gather()                                       # no process group: a no-op


# ------------------------------------------------------------------------------------------------------------------------ on the GPU
@gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_merge_equals_one_evaluator(name):
    a, b, c = _evaluator(name), _evaluator(name), _evaluator(name)
    _feed(a, name, 0, 5), _feed(b, name, 5, 13), _feed(c, name, 13, None)
    cuts = [len(a.tables()["image_t"]), len(a.tables()["image_t"]) + len(b.tables()["image_t"])]
    a.merge(b)
    a.merge(c)
    want = _one(name)
    _assert_same(_result(a, name), want)
    # the tie-break is tested: in one category, equal scores on both sides of a split
    tab = want[2]
    straddle = 0
    for cut in cuts:
        for k in np.unique(tab["dt_category_id"]):
            sel = tab["dt_category_id"] == k
            left = set(tab["dt_score"][sel & (tab["dt_image_id"] <= cut)].tolist())
            straddle += len(left & set(tab["dt_score"][sel & (tab["dt_image_id"] > cut)].tolist()))
    print(name, "image counts at the splits", cuts, "equal scores of one category across a split:", straddle)
    assert 0 < cuts[0] < cuts[1] < len(tab["image_t"]) and straddle > 0


@gpu
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_merge_of_a_duplicate_buffer_equals_feeding_twice(name):
    a, b = _evaluator(name), _evaluator(name)
    _feed(a, name), _feed(b, name)
    a.merge(b)
    _assert_same(_result(a, name), _one(name, 2))
    _assert_same(_result(b, name), _one(name))            # the source is left as it was


@gpu
def test_merge_edge_cases():
    name = "gen1"
    want = _one(name)
    a = _evaluator(name)
    _feed(a, name)
    a.merge(_evaluator(name))                             # never used: a no-op
    _assert_same(_result(a, name), want)
    fresh = _evaluator(name)
    fresh.merge(a)                                        # into a fresh one: equals the source
    assert fresh.has_data()
    _assert_same(_result(fresh, name), want)
    b = _evaluator(name)
    _feed(b, name)
    b.reset_buffer()
    a.merge(b)                                            # a reset one: nothing arrives
    _assert_same(_result(a, name), want)
    b.merge(a)                                            # and into a reset one
    _assert_same(_result(b, name), want)
    # merge after evaluate_buffer, then evaluate again
    head, tail = _evaluator(name), _evaluator(name)
    _feed(head, name, 0, 9), _feed(tail, name, 9, None)
    first = head.evaluate_buffer(240, 304)
    head.merge(tail)
    with pytest.raises(RuntimeError):
        head.precision()                                  # the table of before the merge is not handed out
    got = _result(head, name)
    _assert_same(got, want)
    assert first != got[0]


@gpu
def test_export_and_import_equal_merge():
    name = "gen4"
    a, b, c = _evaluator(name), _evaluator(name), _evaluator(name)
    _feed(a, name, 0, 7), _feed(b, name, 7, None), _feed(c, name, 0, 7)
    blob = b.export_buffer()
    tab = b.tables()
    st = blob["state"].cpu().numpy()
    assert blob["dataset"] == "gen4" and blob["downsample_by_2"] is False and blob["state"].shape == (32,) and blob["state"].is_cuda
    assert (st[0], st[1], st[2]) == (len(tab["image_t"]), len(tab["gt_bbox"]), len(tab["dt_score"])) and st[3] == st[4:8].sum() > 0
    for k, n in (("img_t", st[0]), ("gt_box", st[1]), ("gt_cls", st[1]), ("gt_img", st[1]), ("det_box", st[2]), ("det_cls", st[2]),
                 ("det_img", st[2]), ("rec_key", st[3]), ("rec_match", st[3]), ("rec_ign", st[3])):
        assert blob[k].is_cuda and blob[k].shape[0] == n, k
    a.merge(b)
    c.import_buffer(blob)
    want = _one(name)
    _assert_same(_result(a, name), want)
    _assert_same(_result(c, name), want)
    with pytest.raises(ValueError):
        _evaluator("gen4_ds2").import_buffer(blob)


@gpu
def test_merge_overflow_is_all_or_nothing_and_raised():
    name = "gen1"
    dst0, src = _evaluator(name), _evaluator(name)
    _feed(dst0, name, 0, 9), _feed(src, name, 9, None)
    td, ts = dst0.tables(), src.tables()
    (ni_d, ng_d, nd_d), (ni_s, ng_s, nd_s) = ((len(t["image_t"]), len(t["gt_bbox"]), len(t["dt_score"])) for t in (td, ts))
    # a frame holds at most max_labels_per_frame rows, so the ground-truth table can only overflow together with the images: the
    # third case lacks both and must name both
    assert ng_d + ng_s > ni_d * G.M_ROWS and nd_d + nd_s > 0
    for caps, words in ((dict(max_images=ni_d + ni_s - 1), [f"max_images={ni_d + ni_s - 1}"]),
                        (dict(max_detections=nd_d + nd_s - 1), [f"max_detections={nd_d + nd_s - 1}"]),
                        (dict(max_images=ni_d), [f"max_labels_per_frame={G.M_ROWS}", f"max_images={ni_d}"])):
        dst = _evaluator(name, **caps)
        _feed(dst, name, 0, 9)
        dst.merge(src)
        after = dst.tables()
        for k in td:
            assert np.array_equal(after[k], td[k]), k
        with pytest.raises(OverflowError) as err:
            dst.evaluate_buffer(240, 304)
        print(caps, err.value)
        for w in words:
            assert w in str(err.value)
        if len(words) == 1:
            assert sum(f"{c}=" in str(err.value) for c in ("max_images", "max_detections", "max_labels_per_frame")) == 1
    exact = _evaluator(name, max_images=ni_d + ni_s, max_detections=nd_d + nd_s)
    _feed(exact, name, 0, 9)
    exact.merge(src)                                      # an exact fit
    _assert_same(_result(exact, name), _one(name))
    # a source that itself refused frames hands its refusals on
    small = _evaluator(name, max_images=2)
    _feed(small, name, 9, None)
    big = _evaluator(name)
    big.merge(small)
    with pytest.raises(OverflowError, match="max_images=64"):
        big.evaluate_buffer(240, 304)


@gpu
def test_merge_refusals():
    a = _evaluator("gen4")
    _feed(a, "gen4")
    with pytest.raises(ValueError):
        a.merge(a)
    ds2, gen1 = _evaluator("gen4_ds2"), _evaluator("gen1")
    _feed(ds2, "gen4_ds2"), _feed(gen1, "gen1")
    for other in (ds2, gen1):
        with pytest.raises(ValueError):
            a.merge(other)
    wide = _evaluator("gen4", max_labels_per_frame=G.M_ROWS + 1)
    _feed(wide, "gen4")
    with pytest.raises(ValueError):
        a.merge(wide)
    _assert_same(_result(a, "gen4"), _one("gen4"))


@gpu
def test_add_and_merge_in_one_graph():
    name = "gen4_ds2"
    want = _one(name)
    labels, counts, det, n_det = (torch.from_numpy(np.ascontiguousarray(v[5:])).cuda() for v in _case(name))
    a, b = _evaluator(name), _evaluator(name)

    def step():
        b.add(labels, counts, det, n_det)
        a.merge(b)

    def start():
        a.reset_buffer(), b.reset_buffer()
        _feed(a, name, 0, 5)

    start()
    step()                                                # the eager call (it allocates)
    _assert_same(_result(a, name), want)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    start()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                             # would fail on any host synchronisation
        step()
    for _ in range(2):
        start()
        g.replay()
        assert a.has_data()
        _assert_same(_result(a, name), want)


@gpu
def test_precision_bits_do_not_depend_on_the_chunk_length():
    name = "gen4"
    K = G.N_CLASSES[G.CASES[name][0]]
    before = os.environ.get(KNOB)
    try:
        for times in (1, 2):
            ev = _evaluator(name)
            _feed(ev, name)
            if times == 2:
                twin = _evaluator(name)
                _feed(twin, name)
                ev.merge(twin)
            per_cat = ev._t["state"][4:8].cpu().numpy()
            n = int(per_cat.max())
            assert n >= 3 * 64 - 63                       # some category spans at least three chunks of 64
            stats_ref, prec_ref = _restate(ev.tables(), K)
            runs = {}
            for chunk in (1, 7, 64, n, n - 1, n + 1, 1 << 20):
                os.environ[KNOB] = str(chunk)
                _lib.reload_knobs()
                stats = ev.evaluate_buffer(*G.CASES[name][2])
                assert _lib.knobs()[KNOB] == chunk
                runs[chunk] = (stats, ev.precision().cpu().numpy())
                diff = runs[chunk][1] != prec_ref
                print(name, "x", times, "chunk", chunk, "records per category", per_cat[:K], "entries that differ:", int(diff.sum()))
            for chunk, (stats, prec) in runs.items():
                assert np.array_equal(prec.view(np.int64), prec_ref.view(np.int64)), chunk
                assert np.array_equal(prec.view(np.int64), runs[1][1].view(np.int64)) and stats == runs[1][0], chunk
                assert all(abs(stats[k] - stats_ref[k]) <= 1e-12 for k in CR.OUT_KEYS), chunk
    finally:
        if before is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = before
        _lib.reload_knobs()


_RANK_WORKER = r"""
import hashlib, json, os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_evaluation_merge as T
dist.init_process_group("gloo")                          # two ranks sharing the one GPU: the collective is what is tested
rank = dist.get_rank()
torch.cuda.set_device(0)
name = sys.argv[2]
ev = T._evaluator(name)
T._feed(ev, name, 0, 7) if rank == 0 else T._feed(ev, name, 7, None)
ev.all_gather()
stats = ev.evaluate_buffer(*T.G.CASES[name][2])
bits = hashlib.sha256(ev.precision().cpu().numpy().tobytes()).hexdigest()
print("RESULT " + json.dumps({"rank": rank, "stats": stats, "bits": bits, "images": len(ev.tables()["image_t"])}), flush=True)
dist.barrier()
dist.destroy_process_group()
"""


@gpu
def test_all_gather_two_ranks_equal_one_evaluator(tmp_path):
    name = "gen4"
    want = _one(name)
    script = tmp_path / "worker.py"
    script.write_text(_RANK_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29761", str(script), ROOT, name], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    # the two ranks share one pipe: their lines may arrive glued together
    got = [json.JSONDecoder().raw_decode(piece)[0] for piece in r.stdout.split("RESULT ")[1:]]
    assert sorted(g["rank"] for g in got) == [0, 1], r.stdout[-2000:]
    bits = hashlib.sha256(want[1].tobytes()).hexdigest()
    for g in got:
        assert g["stats"] == want[0] and g["bits"] == bits and g["images"] == len(want[2]["image_t"]), g


@gpu
def test_all_gather_of_one_rank_leaves_the_buffer(tmp_path):
    import torch.distributed as dist
    name = "gen1"
    ev = _evaluator(name)
    _feed(ev, name)
    ev.all_gather()                                       # no process group
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'store'}", rank=0, world_size=1)
    try:
        ev.all_gather()
    finally:
        dist.destroy_process_group()
    _assert_same(_result(ev, name), _one(name))
