"""Fixture of the random-access sampler (sast_amd/sampling.py): `python tests/golden/make_golden_random_access.py` ->
random_access.npz, expected values only.

They come from the reference's own classes.  For every recording of a pool, labels_and_ev_repr_timestamps of
scripts/genx/preprocess_dataset.py (as in make_golden_labels.py) gives the label frames and the frame -> window map, which are written
into a temporary recording directory the way the preprocessing script lays it out: labels_v2/labels.npz (labels,
objframe_idx_2_label_idx), event_representations_v2/<name>/objframe_idx_2_repr_idx.npy and empty event_representations*.h5 files (only
tested for existence).  SequenceDataset / CustomConcatDataset of data/genx_utils/dataset_rnd.py then run on those directories in
only-load-labels mode, and get_weighted_random_sampler gives the weights.  h5py, torchdata, torchvision.transforms, omegaconf and
strenum are not installed and not reached on this route: stand-ins are installed here.

The box records are not stored: `pool_records(name)` regenerates them (make_golden_labels.records, and a second seeded gen1 recording
whose clock is shifted by one window so that an item starts at window 0).  `check_inputs` asserts the conditions the tests rely on.
"""
from __future__ import annotations

import contextlib
import enum
import importlib
import io
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "random_access.npz")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import label_streams_model as M  # noqa: E402
import make_golden_labels as GL  # noqa: E402
import random_access_model as RM  # noqa: E402

GEN1_B = dict(dataset="gen1", seed=505, n_ts=60, period=250000, jitter=400)
POOLS = {"gen1": ("gen1", "single", "gen1_b"), "gen4": ("gen4_30hz",)}     # `gen1_b` lies behind a row that is empty for every L
SPLITS = GL.SPLITS
LENGTHS = (3, 5, 11)
EV_REPR_NAME = "stacked_histogram_dt=50_nbins=10"
MAX_CLASSES = 16


def pool_records(name: str) -> np.ndarray:
    if name != "gen1_b":
        return GL.records(name)
    b = GL.records(GEN1_B)
    b["t"] += 50000          # the first label frame then sits at window 2: the first item of sequence_length 3 starts at window 0
    return b


def dataset_of(pool: str) -> str:
    return "gen4" if pool == "gen4" else "gen1"


def case_keys():
    return [(pool, split, ds, L, end) for pool in POOLS for split in SPLITS for ds in (False, True) for L in LENGTHS for end in (False, True)]


def key_of(pool, split, ds, L, end) -> str:
    return f"{pool}/{split}/{'ds' if ds else 'full'}/L{L}/{'end' if end else 'all'}"


def model_pool(pool, split, ds, L, end) -> RM.Pool:
    rows = [M.load_row(M.pack(pool_records(n)), dataset_of(pool), split, downsample_by_2=ds) for n in POOLS[pool]]
    return RM.Pool(rows, L, end, MAX_CLASSES)


def check_inputs():
    """conditions on the inputs, from the rules restated in random_access_model.py"""
    seen = dict(offset=False, empty=False, window0=False, gap=False, behind_empty=False)
    for pool, split, ds, L, end in case_keys():
        p = model_pool(pool, split, ds, L, end)
        assert p.N > 0
        seen["offset"] |= any(o > 0 and n > 0 for o, n in zip(p.start_idx_offset, p.length))
        for r, n in enumerate(p.length):
            if n == 0:
                seen["empty"] = True
                seen["behind_empty"] |= any(m > 0 for m in p.length[r + 1:])
        for g in range(p.N):
            _r, _j, start, _e = p.locate(g)
            seen["window0"] |= start == 0
            if not end:
                f = [x is not None for x in p.step_frames(g)[1]]
                seen["gap"] |= any(f[i] and not f[i + 1] and any(f[i + 2:]) for i in range(len(f) - 2))
    assert all(seen.values()), seen
    single = model_pool("gen1", "train", False, 11, False)
    assert single.length[1] == 0 and single.rows[1].n_frames == 1, "`single` must have length 0 at sequence_length 11"


# ---- the reference -------------------------------------------------------------------------------------------------------------------

def install_stubs():
    """stand-ins for the packages the reference imports at module scope on this route and never uses: data/genx_utils/sequence_base.py
    (h5py, torchdata.datapipes.map.MapDataPipe), data/utils/augmentor.py (torchvision.transforms), omegaconf, strenum"""
    GL.install_stubs()

    def module(name):
        m = sys.modules.get(name)
        if m is None:
            try:
                m = importlib.import_module(name)
            except Exception:
                m = sys.modules[name] = types.ModuleType(name)
        return m

    td, dp, mp = module("torchdata"), module("torchdata.datapipes"), module("torchdata.datapipes.map")
    if not hasattr(mp, "MapDataPipe"):
        mp.MapDataPipe = type("MapDataPipe", (), {})
    td.datapipes, dp.map = dp, mp
    tv, tr, tf = module("torchvision"), module("torchvision.transforms"), module("torchvision.transforms.functional")
    if not hasattr(tr, "InterpolationMode"):
        tr.InterpolationMode = enum.Enum("InterpolationMode", {"NEAREST": "nearest"})
    if not hasattr(tf, "rotate"):
        def rotate(*a, **k):
            raise NotImplementedError("torchvision is not installed: rotation cannot be exercised")
        tf.rotate = rotate
    tr.functional, tv.transforms = tf, tr


def load_reference():
    pre, _lab = GL.load_reference()
    install_stubs()
    sys.dont_write_bytecode = True
    ns = types.SimpleNamespace(pre=pre)
    ns.rnd = importlib.import_module("data.genx_utils.dataset_rnd")
    ns.types = importlib.import_module("data.utils.types")
    return ns


def reference_available() -> bool:
    return GL.reference_available()


def write_recording(ns, root: Path, name: str, dataset: str, split: str) -> Path:
    """one recording directory (sequence_base.py:29-39) from the reference's own label schedule"""
    npy = root / f"{name}.npy"
    np.save(str(npy), pool_records(name))
    psee, faulty = M.FILTER_DEFAULTS[dataset]
    per_frame, _frame_ts, _ends, f2w = ns.pre.labels_and_ev_repr_timestamps(
        npy_file=npy, split_type=ns.pre.split_name_2_type[split],
        filter_cfg=GL._FilterCfg(apply_psee_bbox_filter=psee, apply_faulty_bbox_filter=faulty),
        align_t_ms=GL.ALIGN_T_MS, ts_step_ev_repr_ms=GL.TS_STEP_EV_REPR_MS, dataset_type=dataset)
    seq = root / name
    (seq / "labels_v2").mkdir(parents=True)
    ev = seq / "event_representations_v2" / EV_REPR_NAME
    ev.mkdir(parents=True)
    starts = np.cumsum([0] + [len(p) for p in per_frame])[:-1]
    np.savez(str(seq / "labels_v2" / "labels.npz"), labels=np.concatenate(per_frame), objframe_idx_2_label_idx=starts)
    np.save(str(ev / "objframe_idx_2_repr_idx.npy"), np.asarray(f2w))
    for f in ("event_representations.h5", "event_representations_ds2_nearest.h5"):
        (ev / f).touch()
    return seq


def generate() -> dict:
    import _ref_import as RI
    from make_golden_augment import SHIPPED
    ns = load_reference()
    check_inputs()
    DataType, DatasetMode = ns.types.DataType, ns.types.DatasetMode
    out = {}
    for pool, names in POOLS.items():
        dataset = dataset_of(pool)
        for split in SPLITS:
            mode = DatasetMode.TRAIN if split == "train" else DatasetMode.VALIDATION
            with tempfile.TemporaryDirectory() as tmp:
                dirs = [write_recording(ns, Path(tmp), n, dataset, split) for n in names]
                for ds in (False, True):
                    for L in LENGTHS:
                        for end in (False, True):
                            cfg = RI.to_cfg(dict(name=dataset, sequence_length=L, ev_repr_name=EV_REPR_NAME, downsample_by_factor_2=ds,
                                                 only_load_end_labels=end, resolution_hw=M.HW[dataset],
                                                 data_augmentation=dict(random=SHIPPED["random"])))
                            seqs = [ns.rnd.SequenceDataset(path=d, dataset_mode=mode, dataset_config=cfg) for d in dirs]
                            concat = ns.rnd.CustomConcatDataset(seqs)
                            key = key_of(pool, split, ds, L, end)
                            out[f"{key}/start_idx_offset"] = np.asarray([s.sequence.start_idx_offset for s in seqs], np.int32)
                            out[f"{key}/length"] = np.asarray([len(s) for s in seqs], np.int32)
                            out[f"{key}/cumulative_sizes"] = np.asarray(concat.cumulative_sizes, np.int64)
                            # the windows of an item: the window indices __getitem__ asks labels for
                            asked = []
                            for s in seqs:
                                inner = s.sequence._get_labels_from_repr_idx
                                s.sequence._get_labels_from_repr_idx = lambda i, inner=inner: (asked.append(int(i)), inner(i))[1]
                            concat.only_load_labels()
                            windows, step_counts, step_labels = [], [], []
                            for g in range(len(concat)):
                                del asked[:]
                                labels = concat[g][DataType.OBJLABELS_SEQ]
                                assert len(labels) == L and (end or asked == list(range(asked[0], asked[0] + L)))
                                windows.append((asked[-1] + 1 - L, asked[-1] + 1))
                                row = []
                                for lab in labels:
                                    row.append(-1 if lab is None else len(lab))
                                    if lab is not None:
                                        step_labels.append(lab.object_labels.numpy().astype(np.float32).reshape(-1, 7))
                                step_counts.append(row)
                            concat.load_everything()
                            out[f"{key}/item_windows"] = np.asarray(windows, np.int64).reshape(-1, 2)
                            out[f"{key}/step_counts"] = np.asarray(step_counts, np.int32).reshape(-1, L)
                            out[f"{key}/step_labels"] = np.concatenate(step_labels + [np.zeros((0, 7), np.float32)])
                            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                                sampler = ns.rnd.get_weighted_random_sampler(concat)
                            out[f"{key}/weights"] = sampler.weights.numpy().astype(np.float64)
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(data)} arrays")
