"""Fixture of the streaming sampler (sast_amd/sampling.py, StreamingPool): `python tests/golden/make_golden_streaming.py` ->
streaming.npz, expected values only.

They come from the reference's own classes, on the recording directories make_golden_random_access.write_recording lays out (the same
pools and box records): SequenceForIter / SequenceForIter.get_sequences_with_guaranteed_labels of
data/genx_utils/sequence_for_streaming.py give the sub-sequences, their __getitem__ the samples (is_first_sample, is_padded_mask, the
window indices asked for, the labels), and ShardedStreamingDataPipe.assign_datapipes_to_worker /
get_zipped_stream_from_worker_datapipes of data/utils/stream_sharded_datapipe.py the per-batch-row lists.

h5py and torchdata are not installed; stand-ins are installed here: an h5py.File whose ['data'] reports the recording's window count
(the number of window ends labels_and_ev_repr_timestamps returns) and gives zeros for a slice, and the torchdata.datapipes.iter names,
of which Concater and ZipperLongest only keep their arguments, so that the per-row lists are read back from what the reference's code
built.  What Zipper / ZipperLongest / Concater then do with those lists cannot be exercised here.

`check_inputs` asserts the conditions the tests rely on.
"""
from __future__ import annotations

import importlib
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "streaming.npz")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import label_streams_model as M  # noqa: E402
import make_golden_labels as GL  # noqa: E402
import make_golden_random_access as GR  # noqa: E402
import streaming_model as SM  # noqa: E402

POOLS, SPLITS = GR.POOLS, GR.SPLITS
LENGTHS = (1, 3, 5, 11)
BATCHES, WORKERS = (2, 3), (1, 2)


def case_keys():
    return [(pool, split, ds, L, g) for pool in POOLS for split in SPLITS for ds in (False, True) for L in LENGTHS for g in (True, False)]


def key_of(pool, split, ds, L, g) -> str:
    return f"{pool}/{split}/{'ds' if ds else 'full'}/L{L}/{'guaranteed' if g else 'unsplit'}"


def labels_key(pool, split, ds) -> str:
    """every label frame lies in exactly one sample, whatever the sequence length and the cut: the label rows of all samples in order
    are the recordings' label frames in order, stored once per (pool, split, resolution); `generate` asserts it for every case"""
    return f"{pool}/{split}/{'ds' if ds else 'full'}/step_labels"


def sharded_cases(packed) -> dict:
    """`<key>/sharded` -> {(B, W, w): the per-batch-row lists of sequence ids, or None where the reference asserts}"""
    v, out, at = [int(x) for x in packed], {}, 0
    while at < len(v):
        B, W, w, ok = v[at:at + 4]
        at += 4
        if not ok:
            out[(B, W, w)] = None
            continue
        lens = v[at:at + B]
        at += B
        rows = []
        for n in lens:
            rows.append(v[at:at + n])
            at += n
        out[(B, W, w)] = rows
    return out


def model_rows(pool, split, ds):
    return [M.load_row(M.pack(GR.pool_records(n)), GR.dataset_of(pool), split, downsample_by_2=ds) for n in POOLS[pool]]


def model_pool(pool, split, ds, L, g) -> SM.Pool:
    return SM.Pool(model_rows(pool, split, ds), L, g)


def check_inputs():
    """conditions on the inputs, from the rules restated in streaming_model.py (train split, full resolution)"""
    def per_row(p):
        return [p.row_first_seq[r + 1] - p.row_first_seq[r] for r in range(len(p.rows))]

    def tails(p):
        return [int(s[2] - s[1]) % p.L for s in p.sequences]

    g1, g4 = model_pool("gen1", "train", False, 3, True), model_pool("gen4", "train", False, 3, True)
    assert per_row(g1) == [3, 1, 5] and per_row(g4) == [4], "sequence_length 3 must split gen1, gen1_b and gen4_30hz into 3, 5 and 4"
    for p in (g1, g4):
        assert 0 in tails(p) and any(tails(p)), "sequence_length 3 must give exact and padded tails"
    s = g1.sequences[g1.row_first_seq[1]]
    assert s[3] == 1 and s[2] - s[1] == 2, "`single` must be one sample of 2 real windows and 1 padded one"
    for pool in POOLS:
        p = model_pool(pool, "train", False, 1, True)
        assert per_row(p) == [r.n_frames for r in p.rows] and (p.sequences[:, 2] - p.sequences[:, 1] == 1).all()
        for L in (5, 11):
            for g in (True, False):
                assert per_row(model_pool(pool, "train", False, L, g)) == [1] * len(POOLS[pool])
    t5, t11 = tails(model_pool("gen1", "train", False, 5, True)), tails(model_pool("gen1", "train", False, 11, True))
    assert t5[0] == 0 and t5[2] > 0, "sequence_length 5: gen1 ends exactly, gen1_b with a padded tail"
    assert t11[0] > 0 and t11[1] > 0 and tails(model_pool("gen4", "train", False, 11, True))[0] > 0
    for pool, split, ds, L, g in case_keys():                 # the unsplit sequence runs to the recording's last window
        p = model_pool(pool, split, ds, L, g)
        assert p.n_seq > 0 and p.status == 0
        if not g:
            assert p.sequences[:, 2].tolist() == [r.n_windows for r in p.rows]


# ---- the reference -------------------------------------------------------------------------------------------------------------------

WINDOWS = {}          # recording directory -> its number of windows (event representations)


class _H5Data:
    def __init__(self, n):
        self.shape = (n, 2, 2, 2)

    def __getitem__(self, sl):
        return np.zeros((len(range(*sl.indices(self.shape[0]))),) + self.shape[1:], np.uint8)


class _H5File:
    """h5py.File of an event_representations*.h5: only ['data'].shape[0] and slices of it are asked for"""

    def __init__(self, path, mode="r"):
        self.n = WINDOWS[str(Path(path).parents[2])]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __getitem__(self, name):
        assert name == "data"
        return _H5Data(self.n)


class _Keep:
    """a datapipe stand-in that keeps what it was built from"""

    def __init__(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs


def install_stubs():
    GR.install_stubs()
    sys.modules["h5py"].File = _H5File
    it = sys.modules.get("torchdata.datapipes.iter")
    if it is None:
        it = sys.modules["torchdata.datapipes.iter"] = types.ModuleType("torchdata.datapipes.iter")
    it.IterDataPipe = type("IterDataPipe", (), {})
    for name in ("Concater", "ZipperLongest", "Zipper", "IterableWrapper"):
        setattr(it, name, type(name, (_Keep,), {}))
    sys.modules["torchdata.datapipes"].iter = it
    sys.modules["torchdata.datapipes.map"].MapDataPipe.to_iter_datapipe = lambda self: self


def load_reference():
    ns = GR.load_reference()
    install_stubs()
    ns.stream = importlib.import_module("data.genx_utils.sequence_for_streaming")
    ns.sharded = importlib.import_module("data.utils.stream_sharded_datapipe")
    return ns


def reference_available() -> bool:
    return GR.reference_available()


def _window_count(ns, root: Path, name: str, dataset: str, split: str) -> int:
    psee, faulty = M.FILTER_DEFAULTS[dataset]
    _per_frame, _frame_ts, ends, _f2w = ns.pre.labels_and_ev_repr_timestamps(
        npy_file=root / f"{name}.npy", split_type=ns.pre.split_name_2_type[split],
        filter_cfg=GL._FilterCfg(apply_psee_bbox_filter=psee, apply_faulty_bbox_filter=faulty),
        align_t_ms=GL.ALIGN_T_MS, ts_step_ev_repr_ms=GL.TS_STEP_EV_REPR_MS, dataset_type=dataset)
    return len(ends)


def generate() -> dict:
    ns = load_reference()
    check_inputs()
    DataType, DatasetType = ns.types.DataType, ns.types.DatasetType
    out = {}
    for pool, names in POOLS.items():
        dataset = GR.dataset_of(pool)
        dtype = DatasetType.GEN4 if dataset == "gen4" else DatasetType.GEN1
        for split in SPLITS:
            with tempfile.TemporaryDirectory() as tmp:
                dirs = [GR.write_recording(ns, Path(tmp), n, dataset, split) for n in names]
                for d, n in zip(dirs, names):
                    WINDOWS[str(d)] = _window_count(ns, Path(tmp), n, dataset, split)
                for ds in (False, True):
                    for L in LENGTHS:
                        for g in (True, False):
                            kw = dict(ev_representation_name=GR.EV_REPR_NAME, sequence_length=L, dataset_type=dtype, downsample_by_factor_2=ds)
                            seqs, seq_rows = [], []
                            for r, d in enumerate(dirs):              # datapipes.extend(new_datapipes) over the recordings
                                new = ns.stream.SequenceForIter.get_sequences_with_guaranteed_labels(path=d, **kw) if g \
                                    else [ns.stream.SequenceForIter(path=d, **kw)]
                                seqs.extend(new)
                                seq_rows.extend([r] * len(new))
                            key = key_of(pool, split, ds, L, g)
                            out[f"{key}/sequences"] = np.asarray(
                                [(r, s.start_indices[0], s.stop_indices[-1], len(s)) for r, s in zip(seq_rows, seqs)], np.int32).reshape(-1, 4)
                            asked = []
                            for s in seqs:
                                inner = s._get_labels_from_repr_idx
                                s._get_labels_from_repr_idx = lambda i, inner=inner: (asked.append(int(i)), inner(i))[1]
                            sample_seq, first, padded, windows, step_counts, step_labels = [], [], [], [], [], []
                            for k, s in enumerate(seqs):
                                for i in range(len(s)):
                                    del asked[:]
                                    item = s[i]
                                    labels = item[DataType.OBJLABELS_SEQ]
                                    assert len(labels) == L == len(item[DataType.EV_REPR]) == len(item[DataType.IS_PADDED_MASK])
                                    sample_seq.append(k)
                                    first.append(bool(item[DataType.IS_FIRST_SAMPLE]))
                                    padded.append([bool(v) for v in item[DataType.IS_PADDED_MASK]])
                                    windows.append(asked + [-1] * (L - len(asked)))
                                    row = []
                                    for lab in labels:
                                        row.append(-1 if lab is None else len(lab))
                                        if lab is not None:
                                            step_labels.append(lab.object_labels.numpy().astype(np.float32).reshape(-1, 7))
                                    step_counts.append(row)
                            filler = seqs[0].get_fully_padded_sample()
                            assert filler[DataType.IS_FIRST_SAMPLE] is False and all(filler[DataType.IS_PADDED_MASK]) \
                                and all(lab is None for lab in filler[DataType.OBJLABELS_SEQ])
                            out[f"{key}/sample_seq"] = np.asarray(sample_seq, np.int32)
                            out[f"{key}/is_first"] = np.asarray(first, np.uint8)
                            out[f"{key}/is_padded"] = np.asarray(padded, np.uint8).reshape(-1, L)
                            out[f"{key}/windows"] = np.asarray(windows, np.int64).reshape(-1, L)
                            out[f"{key}/step_counts"] = np.asarray(step_counts, np.int32).reshape(-1, L)
                            rows7 = np.concatenate(step_labels + [np.zeros((0, 7), np.float32)])
                            if out.setdefault(labels_key(pool, split, ds), rows7) is not rows7:
                                assert out[labels_key(pool, split, ds)].tobytes() == rows7.tobytes(), key
                            ident = {id(s): k for k, s in enumerate(seqs)}
                            packed = []
                            for B in BATCHES:
                                pipe = ns.sharded.ShardedStreamingDataPipe(datapipe_list=list(seqs), batch_size=B, fill_value=filler)
                                for W in WORKERS:
                                    for w in range(W):
                                        try:
                                            local = pipe.assign_datapipes_to_worker(sorted_datapipe_list=pipe.datapipe_list,
                                                                                    total_num_workers=W, global_worker_id=w)
                                            zipped = pipe.get_zipped_stream_from_worker_datapipes(datapipe_list=local, batch_size=B)
                                        except AssertionError:
                                            packed += [B, W, w, 0]
                                            continue
                                        assert type(zipped).__name__ == "ZipperLongest" and len(zipped.args) == B
                                        rows = [[ident[id(s)] for s in c.args] for c in zipped.args]
                                        packed += [B, W, w, 1] + [len(r) for r in rows] + [s for r in rows for s in r]
                            out[f"{key}/sharded"] = np.asarray(packed, np.int32)
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(data)} arrays")
