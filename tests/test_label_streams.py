"""The label front end (sast_amd.labels.LabelStreams, the sast_labels_* entry points of csrc/k_labels.hip).

Everything is compared for equality: integers, and fp32 values by their bits.  The expected values of the fixture
(tests/golden/label_streams.npz) were written by the reference's own labels_and_ev_repr_timestamps and ObjectLabelFactory; a numpy model
(tests/label_streams_model.py) is pinned to the fixture on the CPU and stands in for the reference at the shapes the fixture does not
hold.  Every device row carries stale, valid-looking records past its count."""
import ctypes as C
import functools
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
import label_streams_model as M  # noqa: E402
import make_golden_labels as GL  # noqa: E402
import make_golden_events as G  # noqa: E402

gpu = pytest.mark.gpu

LOAD_LAUNCHES, LABELS_LAUNCHES = 1, 1      # LabelStreams' docstring: one workgroup per row does a whole load; one gather
CASE_KEYS = [(n, s, ds) for n in GL.CASES for s in GL.SPLITS for ds in (False, True)]


@functools.lru_cache(maxsize=None)
def _fx():
    with np.load(os.path.join(GOLDEN, "label_streams.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _words(name):
    return M.pack(GL.records(name))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _fx_frames(name, split, ds):
    fx = _fx()
    tag = "ds" if ds else "full"
    labels, counts = fx[f"{name}/{split}/{tag}/labels"], fx[f"{name}/{split}/{tag}/counts"]
    starts = np.cumsum(counts) - counts
    return [labels[o:o + n] for o, n in zip(starts, counts)]


def _boxes(rows):
    """[(t, x, y, w, h, class_id)] -> int32 [n, 10]"""
    b = np.zeros(len(rows), dtype=M.BBOX_DTYPE)
    for i, r in enumerate(rows):
        b[i]["t"], b[i]["x"], b[i]["y"], b[i]["w"], b[i]["h"], b[i]["class_id"] = r
        b[i]["class_confidence"] = 0.5
    return M.pack(b)


def _box(t, x=50.0, y=60.0, w=40.0, h=50.0, cls=0):
    return (t, x, y, w, h, cls)


# ---------------------------------------------------------------------------------------------------------------------------- CPU

def test_label_entry_points_declared_exported_and_bound():
    from sast_amd import _lib
    names = [n for n in _lib.declared_symbols() if n.startswith("sast_labels_")]
    assert sorted(names) == ["sast_labels_gather", "sast_labels_load", "sast_labels_ws_bytes"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib._SIGNATURES
    assert [f for f, _t in _lib.SastLabelArgs._fields_] == [
        "ws", "ends_us", "n_windows", "frame_ts_us", "n_frames", "frame_2_window", "window_2_frame", "labels", "frame_start", "frame_count",
        "status", "capacity", "base_delta_us", "align_t_us", "delta_t_us", "S", "width", "height", "class_max", "min_diag2", "min_side",
        "max_width", "reprs_per_frame", "downsample_by_2", "max_frames", "max_windows", "max_labels_per_frame", "reserved"]
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    from sast_amd import labels as LB
    for bit, name, _msg in LB.FLAGS:
        assert f"SAST_LABELS_{name.upper()} = {bit}," in header or f"SAST_LABELS_{name.upper()} = {bit} " in header, name
        assert getattr(M, name.upper()) == bit


def test_label_workspace_size():
    from sast_amd import _lib
    lib = _lib.lib()
    assert lib.sast_labels_ws_bytes(1, 10, 4) == 10 * (8 + 8 + 24 + 4) + 4 * 12
    assert lib.sast_labels_ws_bytes(3, 5003, 7) == 3 * (5004 * 44 + 8 * 12)          # odd sizes are rounded up to even: 8-byte slices
    for bad in ((0, 10, 4), (65536, 10, 4), (1, 0, 4), (1, 10, 0), (16, 2 ** 27, 4)):
        assert lib.sast_labels_ws_bytes(*bad) == 0


def _fake_args(**over):
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


def test_label_entry_points_reject_bad_arguments_before_any_launch():
    from sast_amd import _lib
    lib = _lib.lib()
    EINVAL, p = -22, 0x1000
    before = lib.sast_launch_count()
    bad = [None] + [_fake_args(**{f: None}) for f, _t in _lib.SastLabelArgs._fields_[:11]]
    bad += [_fake_args(**kw) for kw in (
        dict(S=0), dict(S=65536), dict(capacity=0), dict(capacity=2 ** 27), dict(max_frames=0), dict(max_windows=0),
        dict(max_labels_per_frame=0), dict(max_windows=2 ** 30), dict(width=1), dict(height=0), dict(base_delta_us=-1), dict(delta_t_us=0),
        dict(align_t_us=-1), dict(reprs_per_frame=0), dict(reprs_per_frame=101), dict(min_side=-1.0), dict(min_diag2=-1.0))]
    for a in bad:
        ref = None if a is None else C.byref(a)
        assert lib.sast_labels_load(ref, p, p, None, None) == EINVAL
        assert lib.sast_labels_gather(ref, p, 1, p, p, p, p, None) == EINVAL
    a = _fake_args()
    assert lib.sast_labels_load(C.byref(a), None, p, None, None) == EINVAL
    assert lib.sast_labels_load(C.byref(a), p, None, None, None) == EINVAL
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert lib.sast_labels_gather(C.byref(a), ptrs[0], 1, *ptrs[1:], None) == EINVAL
    for T in (0, -1, 2 ** 28):
        assert lib.sast_labels_gather(C.byref(a), p, T, p, p, p, p, None) == EINVAL
    assert lib.sast_launch_count() == before


def test_label_streams_constructor_validation():
    from sast_amd.labels import LabelStreams
    ok = dict(num_streams=2, capacity=100, max_frames=8, max_windows=32, max_labels_per_frame=4)
    ls = LabelStreams(**ok)
    assert (ls.apply_psee_bbox_filter, ls.apply_faulty_bbox_filter, ls.height, ls.width) == (True, True, 240, 304)
    ls = LabelStreams(dataset="gen4", split="val", **ok)
    assert (ls.apply_psee_bbox_filter, ls.apply_faulty_bbox_filter, ls.height, ls.width) == (False, True, 720, 1280)
    assert LabelStreams(dataset="gen4", apply_psee_bbox_filter=True, **ok).apply_psee_bbox_filter is True
    for bad in (dict(dataset="gen2"), dict(split="dev"), dict(ts_step_ev_repr_ms=0), dict(ts_step_ev_repr_ms=30), dict(ts_step_ev_repr_ms=-50),
                dict(ts_step_ev_repr_ms=200), dict(align_t_ms=-1), dict(num_streams=0), dict(num_streams=65536), dict(capacity=0),
                dict(capacity=2 ** 27), dict(max_frames=0), dict(max_windows=0), dict(max_labels_per_frame=0), dict(max_windows=2 ** 31)):
        with pytest.raises(ValueError):
            LabelStreams(**{**ok, **bad})
    for step in (1, 2, 4, 5, 10, 20, 25, 50, 100):
        LabelStreams(ts_step_ev_repr_ms=step, **ok)


def test_label_streams_call_validation_and_cpu_tensors_raise():
    from sast_amd.labels import LabelStreams
    ls = LabelStreams(2, 100, max_frames=8, max_windows=32, max_labels_per_frame=4)
    rec, cnt = torch.zeros(2, 100, 10, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError):
        ls.load(rec.to(torch.int64), cnt)
    for r, c, rs in ((rec[:1], cnt, None), (rec[:, :50], cnt, None), (rec[:, :, :9], cnt, None), (rec, cnt.to(torch.int32), None),
                     (rec, cnt[:1], None), (rec, cnt, torch.zeros(2, dtype=torch.int32)), (rec, cnt, torch.zeros(3, dtype=torch.uint8)),
                     (rec.transpose(0, 1).contiguous().transpose(0, 1), cnt, None)):
        with pytest.raises(ValueError):
            ls.load(r, c, rs)
    for idx in (torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64), torch.zeros(2, 2, 2, dtype=torch.int64),
                torch.zeros(0, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ls.labels(idx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ls.load(rec, cnt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ls.load(rec, cnt, torch.ones(2, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ls.labels(torch.zeros(2, dtype=torch.int64))
    assert ls.errors() == [(), ()]


def test_pack_round_trips_bbox_dtype_and_the_old_spelling():
    from sast_amd.labels import BBOX_DTYPE, LabelStreams
    b = GL.records("gen1")[:50]
    w = LabelStreams.pack(b)
    assert w.dtype == np.int32 and w.shape == (50, 10)
    assert np.array_equal(w.reshape(-1).view(BBOX_DTYPE), b) and BBOX_DTYPE == M.BBOX_DTYPE
    assert np.array_equal(w[:, 0].astype(np.int64) | (w[:, 1].astype(np.int64) << 32), b["t"])
    assert np.array_equal(w[:, 2].view(np.float32), b["x"]) and np.array_equal(w[:, 6].view(np.uint32), b["class_id"])
    assert np.array_equal(w[:, 8].view(np.float32), b["class_confidence"]) and not w[:, 9].any()
    old = np.zeros(50, dtype=[("ts", "<u8"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("class_id", "u1"), ("confidence", "<f4"),
                              ("track_id", "<u4")])
    for name in old.dtype.names:
        old[name] = b[{"ts": "t", "confidence": "class_confidence"}.get(name, name)]
    assert np.array_equal(LabelStreams.pack(old), w)
    assert np.array_equal(M.pack(old), w)
    with pytest.raises(ValueError):
        LabelStreams.pack(old[["ts", "x", "y", "w", "h"]])
    assert LabelStreams.pack(b[:0]).shape == (0, 10)


@pytest.mark.parametrize("name,split,ds", CASE_KEYS)
def test_model_equals_the_reference_fixture(name, split, ds):
    fx = _fx()
    r = M.load_row(_words(name), GL.CASES[name]["dataset"], split, downsample_by_2=ds)
    key = f"{name}/{split}"
    assert r.status == 0
    assert np.array_equal(r.ends_us, fx[f"{key}/ends_us"]) and np.array_equal(r.frame_ts_us, fx[f"{key}/frame_ts_us"])
    assert np.array_equal(r.frame_2_window, fx[f"{key}/frame_2_window"])
    assert np.array_equal(r.ends_us[r.frame_2_window], r.frame_ts_us)
    frames = _fx_frames(name, split, ds)
    assert np.array_equal(r.frame_count, [len(f) for f in frames])
    assert np.array_equal(_bits(r.labels), _bits(np.concatenate(frames)))


def test_model_factory_removes_the_flat_boxes_the_reference_removes():
    fx = _fx()
    raw = M.unpack(fx["factory_raw/records"])
    kept = M.factory_labels(raw, "gen1", True)
    assert 0 < len(kept) < len(raw) and np.array_equal(_bits(kept), _bits(fx["factory_raw/ds/labels"]))
    assert len(M.factory_labels(raw, "gen1", False)) == len(raw)


def test_fixture_inputs_exercise_the_pipeline():
    for name in GL.CASES:
        GL.check_inputs(name)
    fx = _fx()
    assert len(fx["single/train/frame_ts_us"]) == 1 and len(fx["single/train/ends_us"]) == 2
    assert not np.array_equal(fx["gen1/train/full/counts"], fx["gen1/val/full/counts"])


@pytest.mark.skipif(not GL.reference_available(), reason="the reference is not on this machine")
def test_generator_reproduces_committed_label_fixture():
    new, old = GL.generate(), _fx()
    assert sorted(new) == sorted(old)
    for k in new:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert np.ascontiguousarray(new[k]).tobytes() == np.ascontiguousarray(old[k]).tobytes(), k


_READER_PROGRAM = r"""
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>
#include "label_state.cuh"
using namespace sast;

static std::vector<void*> g_heap;
// an allocation of its own, of exactly n elements: reading one element past it is caught
template <class T> static T* heap(size_t n, const T* from, T fill) {
  T* p = (T*)malloc(n * sizeof(T));
  for (size_t i = 0; i < n; ++i) p[i] = from ? from[i] : fill;
  g_heap.push_back(p);
  return p;
}
template <class T> static T* heap(std::initializer_list<T> v) { return heap<T>(v.size(), v.begin(), T()); }
static void check(bool ok, const char* what, int id) {
  if (!ok) { printf("FAILED %s in state %d\n", what, id); exit(1); }
}
static SastLabelArgs sizes(int S, int F, int W, int M, int cap) {
  SastLabelArgs a = {};
  a.S = S; a.max_frames = F; a.max_windows = W; a.max_labels_per_frame = M; a.capacity = cap;
  return a;
}
// every (row, window) of the state through the view, the step and the copy; `print`: a line per step
static void walk(const SastLabelArgs& a, int id, bool print) {
  check(label_state_ok(&a), "label_state_ok", id);
  const int M = a.max_labels_per_frame, cap = (int)a.capacity;
  float* out = heap<float>((size_t)M * 7, nullptr, -1.f);
  for (int r = 0; r < a.S; ++r) {
    const LabelRow v = label_row(a, r);
    check(v.nw >= 0 && v.nw <= a.max_windows && v.nf >= 0 && v.nf <= a.max_frames && (v.nw > 0 || v.nf == 0), "row sizes", id);
    check(v.Mc <= M && v.Mc <= cap, "Mc", id);
    long long sum = 0;
    for (int j = 0; j < v.nf; ++j) sum += v.frame_2_window[j];
    for (int w = 0; w < v.nw; ++w) {
      sum += v.ends_us[w];
      const LabelStep st = v.step(w);
      check(st.count >= 0 && st.count <= v.Mc, "count <= Mc", id);
      check(st.start >= 0 && st.start <= cap - st.count, "0 <= start <= capacity - count", id);
      check(st.labelled == 1 || (st.count == 0 && st.start == 0), "an unlabelled step is empty", id);
      for (int tid = 0; tid < 5; ++tid) v.copy(st, out, M, tid, 5);
      if (!print) continue;
      printf("%d %d %d %d %d", r, w, st.labelled, st.count, st.start);
      for (int i = 0; i < M * 7; ++i) printf(" %.1f", out[i]);
      printf("\n");
    }
    if (sum == 12345) printf("#\n");
  }
}
// S = 2, max_frames = 4, max_windows = 8: every window a label frame of 2 boxes from row 1 on, but for the one hostile value
static void hostile(int id, int cap, int M, int fc, int fs, int w2f, int nw, int nf) {
  SastLabelArgs a = sizes(2, 4, 8, M, cap);
  int32_t frames[16];
  for (int i = 0; i < 16; ++i) frames[i] = w2f == 1 << 30 ? i % 4 : w2f;
  a.n_windows = heap<int32_t>(2, nullptr, nw);
  a.n_frames = heap<int32_t>(2, nullptr, nf);
  a.window_2_frame = heap<int32_t>(16, frames, 0);
  a.frame_count = heap<int32_t>(8, nullptr, fc);
  a.frame_start = heap<int32_t>(8, nullptr, fs);
  a.ends_us = heap<int64_t>(16, nullptr, 7);
  a.frame_2_window = heap<int64_t>(8, nullptr, 3);
  a.labels = heap<float>((size_t)2 * cap * 7, nullptr, 1.f);
  walk(a, id, false);
}
int main() {
  {
    SastLabelArgs a = sizes(@S@, @F@, @W@, @M@, @CAP@);
    a.n_windows = heap<int32_t>({@n_windows@});
    a.n_frames = heap<int32_t>({@n_frames@});
    a.window_2_frame = heap<int32_t>({@window_2_frame@});
    a.frame_count = heap<int32_t>({@frame_count@});
    a.frame_start = heap<int32_t>({@frame_start@});
    a.ends_us = heap<int64_t>({@ends_us@});
    a.frame_2_window = heap<int64_t>({@frame_2_window@});
    a.labels = heap<float>({@labels@});
    walk(a, 0, true);
  }
  const int ANY = 1 << 30;      // window_2_frame: every window its own valid frame
  hostile(1, 2, 3, 3, 1, ANY, 8, 4);                  // capacity 2 < M 3, frame_count 3
  hostile(2, 6, 3, INT_MAX, 1, ANY, 8, 4);
  hostile(3, 6, 3, -5, 1, ANY, 8, 4);
  hostile(4, 6, 3, 2, -1, ANY, 8, 4);
  hostile(5, 6, 3, 2, 6, ANY, 8, 4);                  // frame_start = capacity
  hostile(6, 6, 3, 2, INT_MAX, ANY, 8, 4);
  hostile(7, 6, 3, 2, 1, 4, 8, 4);                    // window_2_frame = max_frames
  hostile(8, 6, 3, 2, 1, -7, 8, 4);
  hostile(9, 6, 3, 2, 1, INT_MAX, 8, 4);
  hostile(10, 6, 3, 2, 1, ANY, -1, 4);
  hostile(11, 6, 3, 2, 1, ANY, 8 + 9, 4);             // n_windows = max_windows + 9
  hostile(12, 6, 3, 2, 1, ANY, 8, 4 + 1);             // n_frames = max_frames + 1
  for (void* p : g_heap) free(p);
  printf("done\n");
  return 0;
}
"""


def test_label_state_reader_under_the_host_sanitizers(tmp_path):
    """csrc/label_state.cuh, built by the host compiler as it stands and run under ASan + UBSan with every array of the state in a heap
    allocation of exactly its size: (a) on a valid tiny state `step` and the row copy equal the model's gather at every (row, window);
    (b) on hostile states -- capacity < max_labels_per_frame with a full frame, counts, starts, frame ids and row sizes far outside
    their ranges -- nothing outside an array is read, count <= Mc and 0 <= start <= capacity - count"""
    import sast_amd.build as B
    S, F, W, Mx, cap = 2, 4, 8, 3, 6
    n_windows, n_frames = [8, 5], [3, 2]
    w2f = np.array([[-1, 0, -1, 1, -1, -1, 2, -1], [0, -1, -1, -1, 1, 0, 1, 2]], np.int32)     # row 1: stale frame ids behind its windows
    fcount = np.array([[0, 3, 2, 3], [1, 3, 3, 3]], np.int32)                                  # no box, exactly M boxes; stale behind n_frames
    fstart = np.array([[0, 0, 3, 1], [0, 1, 2, 2]], np.int32)
    ends = np.arange(S * W, dtype=np.int64).reshape(S, W) * 50000 + 100000
    f2w = np.array([[1, 3, 6, 7], [0, 4, 5, 6]], np.int64)
    labels = (np.arange(S * cap * 7, dtype=np.float32) + 1).reshape(S, cap, 7)
    assert (fcount[0, :3] == 0).any() and (fcount[:, :2] == Mx).any() and (w2f[0] < 0).any()
    src = _READER_PROGRAM
    for key, v in dict(S=S, F=F, W=W, M=Mx, CAP=cap, n_windows=n_windows, n_frames=n_frames, window_2_frame=w2f, frame_count=fcount,
                       frame_start=fstart, ends_us=ends, frame_2_window=f2w).items():
        src = src.replace(f"@{key}@", ", ".join(str(int(x)) for x in np.asarray(v).reshape(-1)))
    src = src.replace("@labels@", ", ".join(f"{float(x)}f" for x in labels.reshape(-1)))
    (tmp_path / "reader.cpp").write_text(src)
    exe = tmp_path / "reader"
    # the runtimes are linked into the program: it starts whatever else the environment loads into a process
    r = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                        "-static-libubsan", "-Wall", "-Werror", "-I", B.CSRC, "-o", str(exe), str(tmp_path / "reader.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("done\n"), (r.stdout[-2000:], r.stderr[-4000:])
    rows = []
    for s in range(S):
        row = M.Row()
        nw, nf = n_windows[s], n_frames[s]
        row.ends_us, row.window_2_frame, row.frame_2_window = ends[s, :nw], w2f[s, :nw], f2w[s, :nf]
        row.frame_ts_us, row.frame_count, row.frame_start, row.labels = ends[s, f2w[s, :nf]], fcount[s, :nf], fstart[s, :nf], labels[s]
        rows.append(row)
    idx = np.repeat(np.arange(W, dtype=np.int64)[:, None], S, 1)
    want_labels, want_counts, _ends, want_labelled = M.gather(rows, idx, Mx)
    lines = [ln.split() for ln in r.stdout.splitlines()[:-1]]
    assert [(int(ln[0]), int(ln[1])) for ln in lines] == [(s, w) for s in range(S) for w in range(n_windows[s])]
    for ln in lines:
        s, w, labelled, count, start = (int(v) for v in ln[:5])
        assert (labelled, count) == (want_labelled[w, s], want_counts[w, s]), (s, w)
        assert start == (fstart[s, w2f[s, w]] if labelled else 0), (s, w)
        assert np.array_equal(np.array(ln[5:], np.float32), want_labels[w, s].reshape(-1)), (s, w)
    assert want_labelled.sum() == 5 and sorted(want_counts[want_labelled == 1].tolist()) == [0, 1, 2, 3, 3]


# ---------------------------------------------------------------------------------------------------------------------------- GPU

_STALE = _boxes([_box(5_000_000 + 250_000 * k) for k in range(4)])      # what lies past a row's count: boxes every filter would keep


def _device_rows(rows, cap):
    """[int32 [n, 10]] -> records [S, cap, 10] (stale records behind each row's count), counts [S]"""
    rec = np.tile(_STALE, ((cap + 3) // 4, 1))[:cap]
    rec = np.stack([rec.copy() for _ in rows])
    for s, w in enumerate(rows):
        rec[s, :len(w)] = w
    return torch.from_numpy(rec).cuda(), torch.tensor([len(w) for w in rows], dtype=torch.int64, device="cuda")


def _streams(rows, dataset, split="train", cap=None, **kw):
    from sast_amd.labels import LabelStreams
    cap = cap or max(max(len(w) for w in rows), 1)
    kw = {**dict(max_frames=128, max_windows=512, max_labels_per_frame=16), **kw}
    ls = LabelStreams(len(rows), cap, dataset=dataset, split=split, **kw)
    rec, cnt = _device_rows(rows, cap)
    ls.load(rec, cnt)
    return ls


def _state(ls, s):
    """row s of the device state, cut to its counts"""
    nw, nf = int(ls.n_windows[s]), int(ls.n_frames[s])
    fc, fs = ls.frame_count[s, :nf].cpu().numpy(), ls.frame_start[s, :nf].cpu().numpy()
    total = int(fc.sum())
    return dict(status=int(ls.status[s]), ends_us=ls.ends_us[s, :nw].cpu().numpy(), frame_ts_us=ls.frame_ts_us[s, :nf].cpu().numpy(),
                frame_2_window=ls.frame_2_window[s, :nf].cpu().numpy(), window_2_frame=ls.window_2_frame[s, :nw].cpu().numpy(),
                frame_start=fs, frame_count=fc, labels=_bits(ls.label_rows[s, :total].cpu().numpy()))


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _model_state(r):
    return dict(status=r.status, ends_us=r.ends_us, frame_ts_us=r.frame_ts_us, frame_2_window=r.frame_2_window,
                window_2_frame=r.window_2_frame, frame_start=r.frame_start, frame_count=r.frame_count, labels=_bits(r.labels))


@gpu
@pytest.mark.parametrize("name,split,ds", CASE_KEYS)
def test_fixture_rows_one_at_a_time(name, split, ds):
    """S = 1, capacities exactly as large as the recording needs: the schedule and every label frame equal the reference's"""
    fx = _fx()
    key = f"{name}/{split}"
    frames = _fx_frames(name, split, ds)
    ends, fts, f2w = fx[f"{key}/ends_us"], fx[f"{key}/frame_ts_us"], fx[f"{key}/frame_2_window"]
    Mx = max(len(f) for f in _fx_frames(name, split, False))
    assert any(len(f) == Mx for f in frames) or ds
    ls = _streams([_words(name)], GL.CASES[name]["dataset"], split, downsample_by_2=ds, max_frames=len(fts), max_windows=len(ends),
                  max_labels_per_frame=Mx)
    assert ls.errors() == [()]
    assert int(ls.n_windows[0]) == len(ends) and int(ls.n_frames[0]) == len(fts)
    assert np.array_equal(ls.ends_us[0].cpu().numpy(), ends) and np.array_equal(ls.frame_ts_us[0].cpu().numpy(), fts)
    assert np.array_equal(ls.frame_2_window[0].cpu().numpy(), f2w)
    labels, counts, e, labelled = ls.labels(ls.frame_2_window[0].reshape(-1, 1).contiguous())
    assert labels.shape == (len(fts), 1, Mx, 7) and ls.errors() == [()]
    labels = labels.cpu().numpy()
    assert np.array_equal(counts[:, 0].cpu().numpy(), [len(f) for f in frames])
    assert np.array_equal(e[:, 0].cpu().numpy(), fts) and bool(labelled.all())
    for k, f in enumerate(frames):
        assert np.array_equal(_bits(labels[k, 0, :len(f)]), _bits(f)), k
        assert not _bits(labels[k, 0, len(f):]).any()


_SIDE_BY_SIDE = {
    "gen1": (["gen1", "single", None, _boxes([_box(20_000), _box(60_000)])], M.NO_ALIGNED_LABEL),
    "gen4": (["gen4_60hz", "gen4_30hz", None, _boxes([_box(400_000, cls=1), _box(400_000, x=300.0, cls=2)])], M.BAD_RATE),
}


@gpu
@pytest.mark.parametrize("dataset", ["gen1", "gen4"])
@pytest.mark.parametrize("ds", [False, True])
def test_rows_side_by_side_equal_their_own_runs(dataset, ds):
    """S = 4: rows of different lengths, an empty row and a flagged row next to each other; every good row equals the S = 1 run of the
    same recording and the model, the flagged rows have their flag and no windows"""
    names, flag = _SIDE_BY_SIDE[dataset]
    rows = [np.zeros((0, 10), np.int32) if n is None else (_words(n) if isinstance(n, str) else n) for n in names]
    ls = _streams(rows, dataset, "val", cap=max(len(w) for w in rows) + 5, downsample_by_2=ds)
    for s in (0, 1):
        alone = _streams([rows[s]], dataset, "val", downsample_by_2=ds)
        assert int(alone.n_frames[0]) > 0 and int(alone.status[0]) == 0
        _same_state(_state(ls, s), _state(alone, 0))
        _same_state(_state(ls, s), _model_state(M.load_row(rows[s], dataset, "val", downsample_by_2=ds)))
    assert _state(ls, 2)["status"] == M.NO_LABELS and int(ls.n_windows[2]) == 0 and int(ls.n_frames[2]) == 0
    assert _state(ls, 3)["status"] == flag and int(ls.n_windows[3]) == 0 and int(ls.n_frames[3]) == 0
    assert M.load_row(rows[3], dataset, "val").status == flag
    assert ls.errors()[:2] == [(), ()] and len(ls.errors()[3]) == 1


def _long_row(n, seed):
    return M.pack(GL.records(dict(dataset="gen1", seed=seed, n_ts=n // 4, period=250000, jitter=300))[:n])


@gpu
def test_long_rows_equal_the_model():
    """rows longer than one pass of the workgroup, a capacity that is no multiple of it, survivors only at the very end of a row"""
    long = _long_row(5000, 17)
    assert len(long) == 5000
    tail = M.unpack(_long_row(3000, 18)).copy()
    tail["x"][:-3] = 400.0                      # outside the frame: only the last three records survive
    tail["x"][-3:], tail["y"][-3:], tail["w"][-3:], tail["h"][-3:] = 20.0, 30.0, 50.0, 60.0
    tail = M.pack(tail)
    kw = dict(max_frames=1024, max_windows=4096, max_labels_per_frame=16)
    ls = _streams([long, tail], "gen1", "train", cap=5003, **kw)
    for s, w in enumerate((long, tail)):
        r = M.load_row(w, "gen1", "train", **kw)
        assert r.status == 0 and r.n_frames >= 1
        _same_state(_state(ls, s), _model_state(r))
    assert int(ls.n_frames[0]) > 500 and int(ls.frame_count[1, :int(ls.n_frames[1])].sum()) == 3


@gpu
def test_step_access_mixes_label_frames_unlabelled_windows_and_a_bad_index():
    rows = [_words("gen1"), _words("single"), _long_row(400, 5), _words("gen1")[:300]]
    kw = dict(max_frames=128, max_windows=512, max_labels_per_frame=6)        # some frames of gen1 hold more than 6 boxes
    ls = _streams(rows, "gen1", "val", **kw)
    model = [M.load_row(w, "gen1", "val", **kw) for w in rows]
    assert any(r.status == M.FRAME_OVERFULL for r in model) and all(r.status & ~M.FRAME_OVERFULL == 0 for r in model)
    f2w = [r.frame_2_window for r in model]
    k6 = int(np.argmax(model[0].frame_count == 6))              # a frame that fills all six rows
    assert model[0].frame_count[k6] == 6
    idx = np.array([[f2w[0][k6], 0, f2w[2][1] + 1, f2w[3][0]],
                    [f2w[0][k6] + 1, f2w[1][0], f2w[2][2], model[3].n_windows],          # the last one: out of range
                    [f2w[0][5], 1, 0, f2w[3][2]]], np.int64)
    out = ls.labels(torch.from_numpy(idx).cuda())
    want = M.gather(model, idx, 6)
    for got, exp, name in zip(out, want, ("labels", "counts", "ends_us", "labelled")):
        got = got.cpu().numpy()
        assert got.shape == exp.shape and got.dtype == exp.dtype, name
        assert np.array_equal(_bits(got) if name == "labels" else got, _bits(exp) if name == "labels" else exp), name
    counts, labelled, ends = (out[k].cpu().numpy() for k in (1, 3, 2))
    assert labelled.sum() >= 6 and (labelled == 0).sum() >= 4 and counts.max() == 6 and ends[1, 3] == -1 and ends[0, 2] > 0
    assert [int(v) for v in ls.status.tolist()] == [r.status for r in model] and model[3].status & M.WINDOW_INDEX
    assert "window_index" in ls.errors()[3]
    # `out` is written in place, and a 1-D index gives the 1-D layout
    again = tuple(torch.full_like(t, 7) for t in out)
    res = ls.labels(torch.from_numpy(idx).cuda(), out=again)
    assert all(a.data_ptr() == b.data_ptr() and torch.equal(a, b) for a, b in zip(res, again)) and all(torch.equal(a, b) for a, b in zip(out, again))
    one = ls.labels(torch.from_numpy(idx[0]).cuda())
    assert one[0].shape == (4, 6, 7) and all(torch.equal(a, b[0]) for a, b in zip(one, out))


@gpu
def test_partial_reload_leaves_the_other_rows_bit_identical():
    rows = [_words("gen1"), _long_row(600, 9), _words("single")]
    ls = _streams(rows, "gen1", "train", cap=700)
    tensors = ("ends_us", "n_windows", "frame_ts_us", "n_frames", "frame_2_window", "window_2_frame", "label_rows", "frame_start",
               "frame_count", "status")
    before = {k: getattr(ls, k).clone() for k in tensors}
    new_rows = [rows[1], rows[2], rows[0]]
    rec, cnt = _device_rows(new_rows, 700)
    ls.load(rec, cnt, reset=torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda"))
    for k in tensors:
        assert torch.equal(getattr(ls, k)[0], before[k][0]) and torch.equal(getattr(ls, k)[2], before[k][2]), k
    _same_state(_state(ls, 1), _model_state(M.load_row(rows[2], "gen1", "train")))
    assert int(ls.n_frames[1]) == 1 and int(before["n_frames"][1]) > 50
    ls.load(rec, cnt, reset=torch.tensor([True, False, True], device="cuda"))
    _same_state(_state(ls, 0), _model_state(M.load_row(rows[1], "gen1", "train")))
    _same_state(_state(ls, 2), _model_state(M.load_row(rows[0], "gen1", "train")))


_P60 = 16530      # a 60 Hz label period whose 6-fold, 99 180 us, lets a label frame land <= 98 000 us after the last one
FLAG_INPUTS = {
    "unsorted": ("gen1", [_box(300_000), _box(200_000)], {}),
    "negative_size": ("gen1", [_box(300_000, w=-1.0)], {}),
    "no_labels": ("gen1", [_box(300_000, x=400.0), _box(300_000, w=4.0)], {}),
    "bad_rate": ("gen4", [_box(300_000, cls=1), _box(300_000, x=300.0, cls=2)], {}),
    "no_aligned_label": ("gen1", [_box(50_000)], {}),
    "zero_count": ("gen1", [_box(200_000), _box(201_000)], {}),
    "too_many_frames": ("gen1", [_box(200_000), _box(450_000), _box(700_000)], dict(max_frames=2)),
    "too_many_windows": ("gen1", [_box(200_000), _box(450_000)], dict(max_windows=4)),
    "frame_overfull": ("gen1", [_box(200_000), _box(200_000, x=100.0), _box(200_000, x=150.0)], dict(max_labels_per_frame=2)),
    "frames_too_close": ("gen4", [_box(200_000 + _P60 * k, cls=1) for k in range(6)] + [_box(200_000 + 97_500, cls=1)], {}),
}


@gpu
@pytest.mark.parametrize("name", list(FLAG_INPUTS))
def test_every_flag_has_a_smallest_input(name):
    from sast_amd import labels as LB
    dataset, rows, kw = FLAG_INPUTS[name]
    bit = {n: b for b, n, _m in LB.FLAGS}[name]
    w = _boxes(rows)
    kw = {**dict(max_frames=8, max_windows=32, max_labels_per_frame=16), **kw}
    assert M.load_row(w, dataset, "train", **kw).status == bit
    good = _boxes([_box(200_000)]) if dataset == "gen1" else _words("gen4_60hz")[:300]
    assert M.load_row(good, dataset, "train", **kw).status == 0
    ls = LB.LabelStreams(2, 400, dataset=dataset, **kw)
    rec, cnt = _device_rows([good, w], 400)
    ls.load(rec, cnt)
    assert [int(v) for v in ls.status.tolist()] == [0, bit] and ls.errors() == [(), (name,)]
    assert int(ls.n_frames[0]) >= 1 and int(ls.n_windows[0]) >= 3
    if name == "frame_overfull":
        assert (int(ls.n_frames[1]), int(ls.n_windows[1]), int(ls.frame_count[1, 0])) == (1, 3, 2)
        _same_state(_state(ls, 1), _model_state(M.load_row(w, dataset, "train", **kw)))
    else:
        assert int(ls.n_frames[1]) == 0 and int(ls.n_windows[1]) == 0
    with pytest.raises(ValueError, match=f"row 1: {name}"):
        ls.load(rec, cnt, check=True)
    ls.load(rec, cnt, reset=torch.tensor([1, 0], dtype=torch.uint8, device="cuda"), check=False)
    # one count more or one capacity more and the flag is gone
    relaxed = dict(too_many_frames=dict(max_frames=3), too_many_windows=dict(max_windows=5), frame_overfull=dict(max_labels_per_frame=3))
    if name in relaxed:
        ok = LB.LabelStreams(1, len(w), dataset=dataset, **{**kw, **relaxed[name]})
        rec1, cnt1 = _device_rows([w], len(w))
        ok.load(rec1, cnt1, check=True)
        _same_state(_state(ok, 0), _model_state(M.load_row(w, dataset, "train", **{**kw, **relaxed[name]})))


@gpu
def test_label_launch_counts_are_the_documented_ones():
    from sast_amd import _lib
    from sast_amd.labels import LabelStreams
    lib = _lib.lib()
    assert (LabelStreams.LOAD_LAUNCHES, LabelStreams.LABELS_LAUNCHES) == (LOAD_LAUNCHES, LABELS_LAUNCHES)
    for S in (1, 3):
        for n in (0, 40, 684):
            ls = LabelStreams(S, 700, max_frames=128, max_windows=512, max_labels_per_frame=16)
            rec, cnt = _device_rows([_words("gen1")[:n]] * S, 700)
            for reset in (None, torch.ones(S, dtype=torch.uint8, device="cuda")):
                before = lib.sast_launch_count()
                ls.load(rec, cnt, reset=reset)
                assert lib.sast_launch_count() - before == LOAD_LAUNCHES, (S, n)
            for T in (None, 1, 5):
                idx = torch.zeros((S,) if T is None else (T, S), dtype=torch.int64, device="cuda")
                before = lib.sast_launch_count()
                ls.labels(idx)
                assert lib.sast_launch_count() - before == LABELS_LAUNCHES, (S, n, T)


@gpu
def test_labels_event_frames_and_augmentation_in_one_graph():
    """labels + EventStreams + SpatialAugmentor(yolox=True) captured once after a warm-up, replayed on a second set of window indices
    written into the same tensor == the eager run on those indices"""
    import make_golden_augment as GA
    from sast_amd import augment as A
    from sast_amd.events import EventStreams
    S, T, H, W, n_ev = 2, 2, 240, 304, 20000
    rows = [_words("gen1")[:120], _long_row(120, 3)]
    ls = _streams(rows, "gen1", "train", max_frames=32, max_windows=128, max_labels_per_frame=12)
    assert ls.errors() == [(), ()] and int(ls.n_frames.min()) >= 4
    ev = [G.stream(seed=40 + s, n=n_ev, height=H, width=W, t_start=0, t_step=300, jitter=50) for s in range(S)]
    cols = [torch.from_numpy(np.stack([e[k] for e in ev])).cuda() for k in range(4)]
    n = torch.full((S,), n_ev, dtype=torch.int64, device="cuda")
    es = EventStreams(S, H, W, bins=10, count_cutoff=10, duration_us=50000)
    aug = A.SpatialAugmentor((H, W), GA.SHIPPED["random"], S)
    aug.set_state([A.AugmentationState(apply_h_flip=True), A.AugmentationState(zoom_out=A.ZoomOutState(True, 20, 10, 1.25))])
    f2w = ls.frame_2_window.cpu().numpy()
    sets = [np.array([[f2w[0][1], f2w[1][1]], [f2w[0][1] + 1, f2w[1][2]]], np.int64),
            np.array([[f2w[0][2] + 1, f2w[1][3]], [f2w[0][3], f2w[1][3] + 1]], np.int64)]
    idx = torch.zeros(T, S, dtype=torch.int64, device="cuda")

    def call():
        labels, counts, ends, labelled = ls.labels(idx)
        frames = es(*cols, n, ends, reset=None)
        es.reset()
        return aug(frames, labels, counts, yolox=True) + (ends, labelled)

    eager = []
    for st in sets:
        idx.copy_(torch.from_numpy(st))
        eager.append([t.clone() for t in call()])
    assert int(eager[1][0].count_nonzero()) > 0 and int(eager[1][2].sum()) > 0 and not torch.equal(eager[0][0], eager[1][0])
    idx.copy_(torch.from_numpy(sets[0]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = call()
    for st, want in zip(sets, eager):
        idx.copy_(torch.from_numpy(st))
        g.replay()
        torch.cuda.synchronize()
        for got, exp in zip(captured, want):
            assert torch.equal(got, exp)
    assert ls.errors() == [(), ()] and es.errors() == (0, 0)


@gpu
def test_evaluator_takes_the_returned_labels_unchanged():
    from sast_amd.evaluation import PropheseeEvaluator
    rows = [_words("gen1"), _long_row(300, 21), _long_row(200, 22)]
    ls = _streams(rows, "gen1", "val")
    f2w = ls.frame_2_window.cpu().numpy()
    idx = torch.tensor([f2w[0][4], f2w[1][2] + 1, f2w[2][3]], dtype=torch.int64, device="cuda")      # row 1: not a label frame
    labels, counts, _ends, labelled = ls.labels(idx)
    assert labelled.tolist() == [1, 0, 1] and counts.tolist()[1] == 0
    ev = PropheseeEvaluator("gen1", False, max_images=16, max_detections=256, max_labels_per_frame=16)
    det = torch.zeros(3, 4, 7, device="cuda")
    ev.add(labels, counts, det, torch.zeros(3, dtype=torch.int32, device="cuda"))
    lab = labels.cpu().numpy()
    keep = 0
    for s, c in enumerate(counts.tolist()):
        t, w, h = lab[s, :c, 0], lab[s, :c, 3], lab[s, :c, 4]          # the evaluator's own filter: past the first 0.5 s, Prophesee's sizes
        keep += int(((t > 500000) & (w * w + h * h >= np.float32(900)) & (w >= 10) & (h >= 10)).sum())
    state = ev._t["state"].tolist()
    assert keep > 0 and state[0] == 2 and state[1] == keep and state[10] == 0
