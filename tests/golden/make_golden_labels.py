"""Fixture of the label front end (sast_amd/labels.py): `python tests/golden/make_golden_labels.py` -> label_streams.npz.

The expected values come from the reference's own functions: labels_and_ev_repr_timestamps of scripts/genx/preprocess_dataset.py
(:336-428; loaded by path, with stub modules for the packages it imports at module scope and never uses on this route) on a temporary
.npy of BBOX_DTYPE records, then ObjectLabelFactory.from_structured_array(...)[i] of data/genx_utils/labels.py with and without
downsample_factor=2.

The box records are not stored: `records(case)` regenerates them from the integer hash of make_golden_events.py, so the GPU tests
rebuild the same inputs without the reference.  `check_inputs` asserts, on the CPU, that the inputs exercise every filter, a rejected
timestamp, a skipped label frame and a single-frame recording.

One condition cannot hold for any input: a box that the 0.5 scaling removes.  scale_ (labels.py:316-334) leaves w' = min((x + w) / 2,
W / 2 - 1) - x / 2; a box that passed the filters has x + w <= W - 1 and w >= 5 (the smallest side either size filter lets through),
so w' >= w / 2 - 1 / 2 >= 2.  The removal is therefore pinned where it can happen: case `factory_raw` feeds unfiltered boxes with
x > W - 2 to the reference's factory directly, and the numpy model's factory_labels is held to it.
"""
from __future__ import annotations

import enum
import importlib
import importlib.util
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "label_streams.npz")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import label_streams_model as M  # noqa: E402
from make_golden_events import _hash  # noqa: E402

# name: dataset, seed, label timestamps, label period (us), jitter (+-us)
CASES = {
    "gen1": dict(dataset="gen1", seed=101, n_ts=90, period=250000, jitter=400),
    "gen4_60hz": dict(dataset="gen4", seed=202, n_ts=400, period=16667, jitter=300),
    "gen4_30hz": dict(dataset="gen4", seed=303, n_ts=240, period=33333, jitter=350),
    "single": dict(dataset="gen1", seed=404, n_ts=1, period=250000, jitter=0),
}
SPLITS = ("train", "val")
ALIGN_T_MS, TS_STEP_EV_REPR_MS = 100, 50


def _u(seed, n, salt, mod):
    return (_hash(seed, n, salt) % np.uint64(mod)).astype(np.int64)


def records(name) -> np.ndarray:
    """the structured BBOX_DTYPE boxes of one case (its name, or a dict like the entries of CASES), sorted by t"""
    c = CASES[name] if isinstance(name, str) else name
    H, W = M.HW[c["dataset"]]
    seed, n_ts = c["seed"], c["n_ts"]
    k = np.arange(n_ts, dtype=np.int64)
    ts = 130000 + k * c["period"] + (_u(seed, n_ts, 1, 2 * c["jitter"] + 1) - c["jitter"])
    keep = np.ones(n_ts, bool)
    if n_ts > 40:
        per_frame = max(round(100000 / c["period"]), 1)    # label timestamps per accepted frame
        ts[7 * per_frame] += 3000                           # a frame > 2 ms off its grid: rejected
        keep[12 * per_frame - (per_frame - 1):13 * per_frame] = False   # a missing label frame: the next accepted count is 2
        if c["dataset"] == "gen1":
            ts = np.sort(np.concatenate([ts, ts[[20, 33]] + 117000]))   # labels between the 4 Hz frames: rejected
            keep = np.concatenate([keep, [True, True]])
    ts = ts[keep]
    n_ts = len(ts)
    per = 4 + _u(seed, n_ts, 2, 8)                          # 4 .. 11 boxes per timestamp
    n = int(per.sum())
    b = np.zeros(n, dtype=M.BBOX_DTYPE)
    b["t"] = np.repeat(ts, per)
    b["x"] = (_u(seed, n, 3, 97 * (W + 70)).astype(np.float64) / 97.0 - 40.0).astype(np.float32)
    b["y"] = (_u(seed, n, 4, 97 * (H + 70)).astype(np.float64) / 97.0 - 40.0).astype(np.float32)
    b["w"] = (_u(seed, n, 5, 89 * (W // 2)).astype(np.float64) / 89.0 + 1.0).astype(np.float32)
    b["h"] = (_u(seed, n, 6, 89 * (H // 2)).astype(np.float64) / 89.0 + 1.0).astype(np.float32)
    b["class_id"] = _u(seed, n, 7, 5 if c["dataset"] == "gen4" else 2)
    b["track_id"] = _u(seed, n, 8, 1000)
    b["class_confidence"] = (_u(seed, n, 9, 1000).astype(np.float64) / 999.0).astype(np.float32)
    special = _u(seed, n, 10, 23)
    wide = special == 0                                     # spans the frame: only the train split's faulty-box filter drops it
    b["x"][wide], b["w"][wide] = 3.25, np.float32(0.95 * W)
    b["h"][wide] = np.maximum(b["h"][wide], 40)
    b["y"][wide] = 10.5
    out = special == 1                                      # wholly outside the frame
    b["x"][out] = W + 5.5
    small = special == 2                                    # passes the 5-pixel filter, fails Prophesee's side / diagonal filter
    b["x"][small], b["y"][small], b["w"][small], b["h"][small] = 50.5, 60.25, 7.5, 8.25
    if c["dataset"] == "gen4":
        b["class_id"][wide | small] = 1
    return b


def check_inputs(name: str):
    """conditions on the inputs, from the reference's rules restated in label_streams_model.py"""
    c = CASES[name]
    if c["n_ts"] == 1:
        return
    b = records(name)
    ds = c["dataset"]
    H, W = M.HW[ds]
    psee = M.FILTER_DEFAULTS[ds][0]
    steps = []
    if ds == "gen4":
        steps.append(b["class_id"] <= 2)
        b = b[steps[-1]]
    partly = ((b["x"] < 0) | (b["x"] + b["w"] > W - 1)) & (b["x"] < W - 1) & (b["x"] + b["w"] > 0)
    assert partly.any(), "no box partly outside the frame"
    cropped = M.apply_filters(b, ds, "val", False, False)           # class + crop + the 5-pixel filter
    crop_only = b[(np.clip(b["x"] + b["w"], 0, W - 1) - np.clip(b["x"], 0, W - 1) > 0) &
                  (np.clip(b["y"] + b["h"], 0, H - 1) - np.clip(b["y"], 0, H - 1) > 0)]
    assert 0 < len(crop_only) < len(b), "the crop filter must drop and keep boxes"
    assert 0 < len(cropped) < len(crop_only), "the conservative size filter must drop and keep boxes"
    sized = M.apply_filters(b, ds, "val", True, False)
    assert 0 < len(sized) < len(cropped), "Prophesee's size filter must drop boxes the conservative one keeps"
    val, train = M.apply_filters(b, ds, "val", psee, True), M.apply_filters(b, ds, "train", psee, True)
    assert 0 < len(train) < len(val), "the faulty-box filter must make train and val differ"
    for s in steps:
        assert 0 < s.sum() < len(s), "the class filter must drop and keep boxes"
    for split in SPLITS:
        r = M.load_row(M.pack(records(name)), ds, split)
        assert r.status == 0 and r.n_frames >= 8
        uts = np.unique(M.apply_filters(records(name), ds, split, psee, True)["t"])
        inside = uts[(uts > r.frame_ts_us[0]) & (uts < r.frame_ts_us[-1])]
        base = 250000 if ds == "gen1" else None
        assert len(np.setdiff1d(inside, r.frame_ts_us)) > 0, "no rejected timestamp"
        if base:
            off = np.abs((inside - r.frame_ts_us[0] + base // 2) % base - base // 2)
            assert (off > 2000).any(), "no timestamp more than 2 ms off the grid"
        per_frame = 100 // TS_STEP_EV_REPR_MS
        assert (np.diff(r.frame_2_window) >= 2 * per_frame).any(), "no accepted count >= 2"


# ---- the reference -------------------------------------------------------------------------------------------------------------------

def install_stubs():
    """h5py, numba, omegaconf, strenum (and whatever else is absent) as empty stand-ins: preprocess_dataset.py imports them at module
    scope; labels_and_ev_repr_timestamps touches none of them"""
    def stub(name, **attrs):
        m = sys.modules.get(name)
        if m is None:
            try:
                m = importlib.import_module(name)
            except Exception:
                m = sys.modules[name] = types.ModuleType(name)
        for k, v in attrs.items():             # another fixture generator's stand-in may be there already, with fewer names
            if not hasattr(m, k):
                setattr(m, k, v)

    class _Cfg(dict):
        __getattr__ = dict.__getitem__

    stub("h5py", File=object)
    stub("hdf5plugin")
    stub("numba", jit=lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f)))
    stub("omegaconf", OmegaConf=type("OmegaConf", (), {}), DictConfig=_Cfg, MISSING="???")
    class StrEnum(str, enum.Enum):
        pass

    stub("strenum", StrEnum=StrEnum)


def load_reference():
    import _ref_import as RI
    install_stubs()
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    path = os.path.join(RI.REF_ROOT, "scripts", "genx", "preprocess_dataset.py")
    spec = importlib.util.spec_from_file_location("_ref_preprocess_dataset", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    labels = importlib.import_module("data.genx_utils.labels")
    return mod, labels


def reference_available() -> bool:
    import _ref_import as RI
    return os.path.isfile(os.path.join(RI.REF_ROOT, "scripts", "genx", "preprocess_dataset.py"))


class _FilterCfg(dict):
    __getattr__ = dict.__getitem__


def generate() -> dict:
    pre, lab = load_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, c in CASES.items():
            check_inputs(name)
            ds = c["dataset"]
            npy = Path(tmp) / f"{name}.npy"
            np.save(str(npy), records(name))
            psee, faulty = M.FILTER_DEFAULTS[ds]
            for split in SPLITS:
                per_frame, frame_ts, ends, f2w = pre.labels_and_ev_repr_timestamps(
                    npy_file=npy, split_type=pre.split_name_2_type[split],
                    filter_cfg=_FilterCfg(apply_psee_bbox_filter=psee, apply_faulty_bbox_filter=faulty),
                    align_t_ms=ALIGN_T_MS, ts_step_ev_repr_ms=TS_STEP_EV_REPR_MS, dataset_type=ds)
                key = f"{name}/{split}"
                out[f"{key}/frame_ts_us"] = np.asarray(frame_ts, np.int64)
                out[f"{key}/ends_us"] = np.asarray(ends, np.int64)
                out[f"{key}/frame_2_window"] = np.asarray(f2w, np.int64)
                starts = np.cumsum([0] + [len(p) for p in per_frame])[:-1]
                for dsf in (None, 2):
                    fac = lab.ObjectLabelFactory.from_structured_array(np.concatenate(per_frame), starts, M.HW[ds], downsample_factor=dsf)
                    rows = [fac[i].object_labels.numpy() for i in range(len(fac))]
                    tag = "ds" if dsf else "full"
                    out[f"{key}/{tag}/labels"] = np.concatenate(rows).astype(np.float32)
                    out[f"{key}/{tag}/counts"] = np.asarray([len(r) for r in rows], np.int32)
        # the removal of flat boxes by the 0.5 scaling, on boxes the filters would never pass (see the module docstring)
        H, W = M.HW["gen1"]
        raw = np.zeros(6, dtype=M.BBOX_DTYPE)
        raw["t"] = 777
        raw["x"] = np.asarray([W - 1.5, W - 2.0, W - 2.5, 10.0, 20.0, 30.5], np.float32)
        raw["y"] = np.asarray([5.0, 6.0, 7.0, H - 1.25, H - 2.0, 8.5], np.float32)
        raw["w"] = np.asarray([0.25, 0.5, 1.0, 20.0, 20.0, 40.25], np.float32)
        raw["h"] = np.asarray([30.0, 30.0, 30.0, 0.125, 0.5, 50.75], np.float32)
        raw["class_id"] = [0, 1, 0, 1, 0, 1]
        fac = lab.ObjectLabelFactory.from_structured_array(raw, np.zeros(1, np.int64), (H, W), downsample_factor=2)
        kept = fac[0].object_labels.numpy().astype(np.float32)
        assert 0 < len(kept) < len(raw), "the 0.5 scaling must remove and keep boxes"
        out["factory_raw/records"] = M.pack(raw)
        out["factory_raw/ds/labels"] = kept
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(data)} arrays")
