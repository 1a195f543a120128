"""The label-sparse selection of the training step as DEVICE data (functional.SelectionTable, gather_samples_dev, select_labels,
zero_samples_dev, sequence.DeviceFeatureSelector, RNNStates.reset_on_device, TrainStep(selection=, reset=, carry_states=), keyed graph sets).

Data movement is compared bit for bit: against a numpy restatement of the table written here, against torch indexing, and against the
host-table path (functional.gather_samples / zero_samples).  The two step tests compare a step that selects by the device table with the
same step selecting by host index lists on a twin rig.  What is gathered is bit-identical; what follows differs by the order of the
floating-point atomics only.  Their tolerance is 10x what two runs of the HOST-index step differ by on twin rigs at these shapes (measured
on the parent of this change, profiles/r15_device_selection.txt), capped at 1e-4 of the gradient max-norm -- a wrongly selected or unzeroed
row is an O(1) error."""
import numpy as np
import pytest
import torch

# profiles/r15_device_selection.txt: two eager host-index steps on twin rigs, worst of the measured scenarios, as
# (|loss_a - loss_b| / |loss_b|, max |g_a - g_b| / max |g_b| over the flat gradient)
FLOOR = (8.165e-08, 1.068e-06)
GRAD_CAP_REL = 1e-4


def _bars():
    loss, grad = FLOOR
    return 10 * loss, min(10 * grad, GRAD_CAP_REL)

HW, PART, EMBED, T_SEQ, BATCH, NUM_CLASSES, MAX_LABELS = (128, 160), (4, 5), 32, 3, 3, 2, 5


# ------------------------------------------------------------------------------------------------ CPU
def test_argument_errors_without_a_gpu():
    from sast_amd import functional as SF
    from sast_amd.detection.sequence import DeviceFeatureSelector, RNNStates
    from sast_amd.training import TrainStep
    for bad in ((0, 3, 1), (33, 3, 1), (3, 0, 1), (3, 257, 1), (3, 3, 257), (3, 3, -1)):
        with pytest.raises(ValueError, match="SelectionTable supports"):
            SF.SelectionTable(*bad, "cpu")
    sel = SF.SelectionTable(3, 4, 2, "cpu")
    assert tuple(sel.table.shape) == (2, 2) and tuple(sel.slot_of.shape) == (3, 4) and tuple(sel.n_sel.shape) == (1,) and tuple(sel.err.shape) == (2,)
    ok = torch.zeros(3, 4, dtype=torch.uint8)
    # CPU tensors: the library's error, no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sel.update(ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.gather_samples_dev([torch.zeros(4, 8)] * 3, sel)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.select_labels(torch.zeros(3, 4, 5, 5), torch.zeros(3, 4, dtype=torch.int32), sel)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.zero_samples_dev([torch.zeros(4, 8)], torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.copy_tensors([torch.zeros(4, 8)], [torch.zeros(4, 8)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _three_steps(DeviceFeatureSelector(sel)).get_batched_backbone_features()
    rs = RNNStates()
    rs.save_states_and_detach(0, [(torch.zeros(4, 8), torch.zeros(4, 8))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs.reset_on_device(0, torch.zeros(4, dtype=torch.uint8))
    rs.reset_on_device(7, torch.zeros(4, dtype=torch.uint8))              # unknown worker: nothing held, nothing done (as `reset`)
    # labelled: dtype and shape
    for bad in (torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4), [[0] * 4] * 3):
        with pytest.raises(TypeError, match="uint8 or bool"):
            sel.update(bad)
    for bad in (torch.zeros(4, 3, dtype=torch.uint8), torch.zeros(12, dtype=torch.bool), torch.zeros(3, 8, dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError, match=r"shape \[3, 4\]"):
            sel.update(bad)
    # flags: dtype and shape
    with pytest.raises(TypeError, match="uint8 or bool"):
        SF.zero_samples_dev([torch.zeros(4, 8)], torch.zeros(4, dtype=torch.int64))
    for bad in (torch.zeros(5, dtype=torch.uint8), torch.zeros(4, 1, dtype=torch.bool)):
        with pytest.raises(ValueError, match=r"shape \[4\]"):
            SF.zero_samples_dev([torch.zeros(4, 8)], bad)
    with pytest.raises(RuntimeError, match="same batch"):
        SF.zero_samples_dev([torch.zeros(4, 8), torch.zeros(5, 8)], torch.zeros(4, dtype=torch.uint8))
    # the gather: a table for other sizes, a wrong selection object, label tensors of the wrong kind
    with pytest.raises(TypeError, match="SelectionTable"):
        SF.gather_samples_dev([torch.zeros(4, 8)] * 3, [[0], [], [1]])
    with pytest.raises(ValueError, match="select_labels needs labels"):
        SF.select_labels(torch.zeros(3, 5, 5, 5), None, sel)
    with pytest.raises(ValueError, match="select_labels needs counts"):
        SF.select_labels(torch.zeros(3, 4, 5, 5), torch.zeros(3, 4, dtype=torch.int64), sel)
    # the step: one selection only, and it must fit the sequence; reset / carry need state tensors
    ts = TrainStep.__new__(TrainStep)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ts.forward([None] * 3, None, None, [[0], [], [1]], selection=sel)
    with pytest.raises(ValueError, match="3 timesteps, the sequence has 2"):
        ts.forward([None] * 2, None, None, selection=sel)
    with pytest.raises(ValueError, match="input state tensors"):
        ts.forward([None] * 3, None, None, selection=sel, reset=torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="input state tensors"):
        ts.forward([None] * 3, None, None, selection=sel, carry_states=True)
    ts._sets = {}
    with pytest.raises(KeyError):
        ts.replay(key=5)


def test_the_sample_movers_are_built():
    from sast_amd import build as B
    assert "k_samples.hip" in B.SOURCES and "k_samples.hip" not in B.SOURCE_FLAGS


def _three_steps(fs):
    for _ in range(3):
        fs.add_backbone_features({2: torch.zeros(4, 8)})
    return fs


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from sast_amd import functional as SF
    SF._FUSED_MIN_ROWS = 0           # as tests/test_gpu_parity.py: every eligible MS-WSA layer takes the one-kernel forward
    return torch.device("cuda:0")


def table_model(lab: np.ndarray, n_out: int):
    """the contract of sast_select_table, restated: pairs timestep-major then batch ascending; what does not fit is not listed"""
    T, B = lab.shape
    pairs = [(t, b) for t in range(T) for b in range(B) if lab[t, b]]
    table, slot = np.full((n_out, 2), -1, np.int32), np.full((T, B), -1, np.int32)
    for j, (t, b) in enumerate(pairs[:n_out]):
        table[j] = (t, b)
        slot[t, b] = j
    return table, slot, len(pairs)


def _patterns(T, B, seed):
    rng = np.random.default_rng(seed)
    some = rng.random((T, B)) < min(0.5, 200.0 / (T * B))        # at the maximum size about 200 of the 8192 pairs: n_out stays <= 256
    some[T - 1, B - 1] = True                                    # the last flag of the last chunk
    stripes = np.zeros((T, B), bool)
    stripes.reshape(-1)[::37] = True
    return {"none": np.zeros((T, B), bool), "all": np.ones((T, B), bool), "random": some, "stripes": stripes}


@pytest.mark.gpu
@pytest.mark.parametrize("T,B", [(3, 3), (5, 13), (32, 256)])
def test_selection_table_matches_numpy(dev, T, B):
    """(5, 13): 65 flags, the prefix crosses a wave; (32, 256): the maximum, 8 chunks of 1024 flags.  n_out equal to, below and above
    the count; table, slot_of, n_sel and both error counters exactly (the counters count UPDATES: two updates, twice)."""
    from sast_amd import functional as SF
    for name, lab in _patterns(T, B, seed=T * B).items():
        n = int(lab.sum())
        as_bool = name == "random"
        d = torch.from_numpy(lab).to(dev) if as_bool else torch.from_numpy(lab.astype(np.uint8) * (3 if name == "stripes" else 1)).to(dev)
        for n_out in sorted({min(n, 256), max(min(n, 256) - 1, 0), min(n + 3, 256), 0}):
            sel = SF.SelectionTable(T, B, n_out, dev)
            assert sel.update(d) is sel
            sel.update(d)
            table, slot, n_ref = table_model(lab, n_out)
            assert n_ref == n
            assert np.array_equal(sel.table.cpu().numpy(), table), (name, n_out)
            assert np.array_equal(sel.slot_of.cpu().numpy(), slot), (name, n_out)
            assert sel.n_sel.tolist() == [n], (name, n_out)
            assert sel.err.tolist() == [2 * int(n > n_out), 2 * int(n < n_out)], (name, n_out)
            assert sel.errors() == {"truncated": 2 * int(n > n_out), "under_full": 2 * int(n < n_out)}
            if n > n_out:
                with pytest.raises(ValueError, match="truncated"):
                    sel.update(d, check=True)
            elif n < n_out:
                with pytest.raises(ValueError, match="under-full"):
                    sel.update(d, check=True)
            else:
                sel.update(d, check=True)
    # a table is reused: a new pattern replaces the old one completely
    sel = SF.SelectionTable(T, B, 2, dev)
    for lab in (np.eye(T, B, dtype=bool), np.eye(T, B, k=1, dtype=bool)[::-1].copy()):
        sel.update(torch.from_numpy(lab).to(dev))
        table, slot, _n = table_model(lab, 2)
        assert np.array_equal(sel.table.cpu().numpy(), table) and np.array_equal(sel.slot_of.cpu().numpy(), slot)


def _pairs(lab):
    return [(t, b) for t in range(lab.shape[0]) for b in range(lab.shape[1]) if lab[t, b]]


def _index_lists(lab):
    return [[b for b in range(lab.shape[1]) if lab[t, b]] for t in range(lab.shape[0])]


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [(1,), (5, 7), (4096,), (8197,), (8200,)], ids=lambda s: "x".join(map(str, s)))
def test_gather_samples_dev_forward_and_backward_bit_exact(dev, sample):
    """1 and 5 x 7 floats per sample: rows that are not 16-byte aligned and a scalar tail; 4096: the aligned path and the host-table
    path's own limit (multiples of 4) to compare with; 8197 / 8200: two workgroups per row, unaligned and aligned.  Against
    torch.cat([x[idx]]) and functional.gather_samples, forward and backward; unselected gradients and the rows behind n_sel exactly zero."""
    from sast_amd import functional as SF
    T, B = 3, 4
    lab = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [0, 1, 1, 1]], bool)           # (0, 0): an aligned row with a tail; timestep 1: nothing
    pairs, idx = _pairs(lab), _index_lists(lab)
    K = len(pairs)
    g = torch.Generator().manual_seed(7)
    xs_cpu = [torch.randn((B,) + sample, generator=g) for _ in range(T)]
    for n_out in (K, K + 2):
        sel = SF.SelectionTable(T, B, n_out, dev).update(torch.from_numpy(lab).to(dev))
        xs = [x.to(dev).requires_grad_(True) for x in xs_cpu]
        out = SF.gather_samples_dev(xs, sel)
        ref_leaves = [x.clone().requires_grad_(True) for x in xs_cpu]
        ref = torch.cat([x[i] for x, i in zip(ref_leaves, idx) if i])
        assert tuple(out.shape) == (n_out,) + sample
        assert torch.equal(out[:K].cpu(), ref)
        assert float(out[K:].detach().abs().sum()) == 0.0
        w = torch.randn(out.shape, generator=g)
        (out * w.to(dev)).sum().backward()
        (ref * w[:K]).sum().backward()
        for t in range(T):
            want = ref_leaves[t].grad if ref_leaves[t].grad is not None else torch.zeros_like(xs_cpu[t])   # a timestep without labels: zeros
            assert torch.equal(xs[t].grad.cpu(), want), t
            unsel = [b for b in range(B) if not lab[t, b]]
            assert float(xs[t].grad[unsel].abs().sum()) == 0.0
        if n_out == K and xs_cpu[0][0].numel() % 4 == 0:
            hs = [x.to(dev).requires_grad_(True) for x in xs_cpu]
            host = SF.gather_samples(hs, idx)
            assert torch.equal(host, out)
            (host * w.to(dev)).sum().backward()
            assert all(torch.equal(a.grad, b.grad) for a, b in zip(hs, xs))


@pytest.mark.gpu
def test_device_feature_selector_and_nchw_views(dev):
    """DeviceFeatureSelector == BackboneFeatureSelector on the same pairs, for NHWC buffers and for logical NCHW tensors in channels-last
    memory (the result is the same kind of view); a selector that has not seen every timestep of the table refuses"""
    from sast_amd import functional as SF
    from sast_amd.detection.sequence import BackboneFeatureSelector, DeviceFeatureSelector
    T, B = 3, 3
    lab = np.array([[1, 0, 1], [0, 0, 0], [1, 1, 1]], bool)
    sel = SF.SelectionTable(T, B, int(lab.sum()), dev).update(torch.from_numpy(lab).to(dev))
    g = torch.Generator().manual_seed(3)
    feats = [{2: torch.randn(B, 8, 6, 10, generator=g), 3: torch.randn(B, 16, 3, 5, generator=g)} for _ in range(T)]
    for layout in ("contiguous", "channels_last"):
        dsel, hsel = DeviceFeatureSelector(sel), BackboneFeatureSelector()
        for t, f in enumerate(feats):
            fd = {k: (v.to(dev).contiguous(memory_format=torch.channels_last) if layout == "channels_last" else v.to(dev)) for k, v in f.items()}
            dsel.add_backbone_features(fd)
            idx = _index_lists(lab)[t]
            if idx:
                hsel.add_backbone_features(fd, idx)
        got, want = dsel.get_batched_backbone_features(), hsel.get_batched_backbone_features()
        for k in (2, 3):
            assert got[k].shape == want[k].shape and got[k].stride() == want[k].stride() and torch.equal(got[k], want[k]), (layout, k)
    assert DeviceFeatureSelector(sel).get_batched_backbone_features() is None
    short = DeviceFeatureSelector(sel)
    short.add_backbone_features({2: feats[0][2].to(dev)})
    with pytest.raises(RuntimeError, match="1 timesteps"):
        short.get_batched_backbone_features()


@pytest.mark.gpu
def test_zero_samples_dev_equals_zero_samples(dev):
    """three tensors of different sample sizes in one launch == functional.zero_samples on each; all-zero flags leave every byte; a sample
    size that is no multiple of 4 (the host path refuses it) against torch indexing; RNNStates.reset_on_device == RNNStates.reset"""
    from sast_amd import _lib, functional as SF
    from sast_amd.detection.sequence import RNNStates
    B = 5
    g = torch.Generator().manual_seed(11)
    cpu = [torch.randn(B, 8, generator=g), torch.randn(B, 3, 4, 4, generator=g), torch.randn(B, 3 * 4096, generator=g)]
    flags = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)
    want = [SF.zero_samples(x.to(dev), flags.bool()) for x in cpu]
    got = [x.to(dev) for x in cpu]
    n0 = _lib.lib().sast_launch_count()
    assert SF.zero_samples_dev(got, flags.to(dev))[0] is got[0]
    assert _lib.lib().sast_launch_count() - n0 == 1
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert float(got[2][1].abs().min()) > 0.0                                  # (an unflagged sample is still there)
    keep = [x.to(dev) for x in cpu]
    SF.zero_samples_dev(keep, torch.zeros(B, dtype=torch.bool, device=dev))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(keep, cpu))
    odd = torch.randn(B, 7, generator=g)
    ref = odd.clone()
    ref[flags.bool()] = 0
    assert torch.equal(SF.zero_samples_dev([odd.to(dev)], flags.bool().to(dev))[0].cpu(), ref)
    many = [torch.ones(B, 4, device=dev) for _ in range(_lib.ZERO_MAX_TENSORS + 1)]       # more than one struct holds: two launches
    SF.zero_samples_dev(many, flags.to(dev))
    assert all(x.sum(1).tolist() == [0.0, 4.0, 0.0, 0.0, 4.0] for x in many)
    a, b = RNNStates(), RNNStates()
    for rs in (a, b):
        rs.save_states_and_detach(0, [(cpu[1].to(dev), cpu[1].to(dev) + 1.0), (cpu[0].to(dev), cpu[2].to(dev))])
    a.reset(0, flags.bool())
    b.reset_on_device(0, flags.to(dev))
    for (h0, c0), (h1, c1) in zip(a.get_states(0), b.get_states(0)):
        assert torch.equal(h0, h1) and torch.equal(c0, c1)
    src = [x.to(dev) for x in cpu] + [odd.to(dev)]                             # the state hand-back kernel: whole tensors, one launch
    dst = [torch.zeros_like(x) for x in src]
    n0 = _lib.lib().sast_launch_count()
    SF.copy_tensors(dst, src)
    assert _lib.lib().sast_launch_count() - n0 == 1 and all(torch.equal(d, s) for d, s in zip(dst, src))


def _host_pairs_at_the_limits():
    """32 timesteps of 256 samples, 8 pairs each = the 256 rows a host table holds, in no particular order within a timestep; (0, 0) and
    (31, 255) are the smallest and the largest values its uint8 entries carry"""
    rng = np.random.default_rng(256)
    idx = [[int(b) for b in rng.permutation(256)[:8]] for _ in range(32)]
    idx[0] = [0] + [b for b in idx[0] if b != 0][:7]
    idx[31] = [b for b in idx[31] if b != 255][:7] + [255]
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("B,sample,idx", [(256, 4, None), (3, 8200, [[2, 0], []])], ids=["table-at-its-limits", "two-workgroups-per-row"])
def test_host_table_gather_at_its_limits(dev, B, sample, idx):
    """The host-table form (BackboneFeatureSelector -> functional.gather_samples) on the mover it shares with the device form: a full table
    (T = 32, B = 256, n_out = 256, 4 floats per sample) and rows of 8200 floats (two workgroups each; the second timestep has no pair and
    takes no part, so its gradient is None).  Forward against torch.cat([x[idx]]), backward against torch autograd of that expression,
    unselected gradients exactly zero, one launch each way."""
    from sast_amd import _lib
    from sast_amd.detection.sequence import BackboneFeatureSelector
    idx = _host_pairs_at_the_limits() if idx is None else idx
    g = torch.Generator().manual_seed(B)
    xs_cpu = [torch.randn(B, sample, generator=g) for _ in idx]
    xs = [x.to(dev).requires_grad_(True) for x in xs_cpu]
    ref_leaves = [x.clone().requires_grad_(True) for x in xs_cpu]
    ref = torch.cat([x[i] for x, i in zip(ref_leaves, idx) if i])
    hsel = BackboneFeatureSelector()
    for x, i in zip(xs, idx):
        if i:
            hsel.add_backbone_features({1: x}, i)
    count = _lib.lib().sast_launch_count
    n0 = count()
    out = hsel.get_batched_backbone_features()[1]
    assert count() - n0 == 1
    assert torch.equal(out.cpu(), ref)
    w = torch.randn(ref.shape, generator=g)
    w_dev = w.to(dev)
    n0 = count()
    out.backward(w_dev)
    assert count() - n0 == 1
    ref.backward(w)
    for t, i in enumerate(idx):
        if not i:
            assert xs[t].grad is None and ref_leaves[t].grad is None, t
            continue
        assert torch.equal(xs[t].grad.cpu(), ref_leaves[t].grad), t
        assert float(xs[t].grad[[b for b in range(B) if b not in i]].abs().sum()) == 0.0, t


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [4, 8200])
def test_host_zero_samples_at_the_largest_batch(dev, sample):
    """functional.zero_samples at B = 256 with the first and the last sample flagged, by bool mask and by the index list [0, -1] (indices
    are taken modulo B), one and two workgroups per sample: against torch indexing, one launch per call"""
    from sast_amd import _lib, functional as SF
    B = 256
    x_cpu = torch.randn(B, sample, generator=torch.Generator().manual_seed(sample))
    ref = x_cpu.clone()
    ref[[0, B - 1]] = 0
    mask = torch.zeros(B, dtype=torch.bool)
    mask[0] = mask[B - 1] = True
    for which in (mask, [0, -1]):
        x = x_cpu.to(dev)
        n0 = _lib.lib().sast_launch_count()
        assert SF.zero_samples(x, which) is x
        assert _lib.lib().sast_launch_count() - n0 == 1
        assert torch.equal(x.cpu(), ref)
    assert float(ref[1:B - 1].abs().min()) > 0.0                               # (the unflagged samples are still there)


@pytest.mark.gpu
def test_host_forms_still_refuse_samples_that_are_no_multiple_of_4_floats(dev):
    """the host-table entry points share the device form's row mover, which takes any row; their own contract (sample_floats % 4 == 0)
    stands: functional.gather_samples / zero_samples raise as before, the C entry points return an error, and nothing is launched"""
    import ctypes as C
    from sast_amd import _lib, functional as SF
    x = torch.randn(4, 7, device=dev)
    n0 = _lib.lib().sast_launch_count()
    with pytest.raises(RuntimeError, match="gather_samples supports"):
        SF.gather_samples([x, x], [[0, 1], [3]])
    with pytest.raises(RuntimeError, match="zero_samples failed"):
        SF.zero_samples(x.clone(), [0])
    out, dx = torch.zeros(1, 7, device=dev), torch.zeros(4, 7, device=dev)
    a = _lib.SastSampleGather()
    a.n_src, a.n_out, a.B, a.sample_floats, a.out = 1, 1, 4, 7, out.data_ptr()
    a.src[0], a.dsrc[0] = x.data_ptr(), dx.data_ptr()
    assert _lib.lib().sast_gather_samples(C.byref(a), None) != 0
    assert _lib.lib().sast_gather_samples_bwd(C.byref(a), None) != 0
    torch.cuda.synchronize()
    assert _lib.lib().sast_launch_count() == n0
    assert float(out.abs().sum()) == 0.0 and float(dx.abs().sum()) == 0.0


@pytest.mark.gpu
def test_table_and_gather_replay_on_a_new_pattern(dev):
    """sel.update + gather_samples_dev + select_labels captured in ONE graph after one eager call; `labelled`, the feature maps and the
    labels are rewritten in place (another pattern with the same K): the replay equals torch indexing of the NEW pattern"""
    from sast_amd import functional as SF
    T, B, M = 3, 4, 6
    g = torch.Generator().manual_seed(5)
    lab0 = np.array([[1, 0, 1, 0], [0, 0, 0, 0], [0, 1, 1, 1]], bool)
    lab1 = np.array([[0, 1, 0, 0], [1, 1, 0, 1], [0, 0, 0, 1]], bool)
    K = int(lab0.sum())
    assert int(lab1.sum()) == K

    def data():
        xs = [torch.randn(B, 6, 5, 8, generator=g) for _ in range(T)]
        return xs, torch.randn(T, B, M, 5, generator=g), torch.randint(0, M + 1, (T, B), generator=g, dtype=torch.int32)

    xs0, labels0, counts0 = data()
    labelled = torch.from_numpy(lab0).to(dev)
    xs, labels, counts = [x.to(dev) for x in xs0], labels0.to(dev), counts0.to(dev)
    sel = SF.SelectionTable(T, B, K, dev)

    def run():
        sel.update(labelled)
        return (SF.gather_samples_dev(xs, sel),) + SF.select_labels(labels, counts, sel)

    def expect(lab, xs_c, labels_c, counts_c):
        p = _pairs(lab)
        return (torch.stack([xs_c[t][b] for t, b in p]), torch.stack([labels_c[t, b] for t, b in p]), torch.stack([counts_c[t, b] for t, b in p]))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for a, b in zip(eager, expect(lab0, xs0, labels0, counts0)):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    xs1, labels1, counts1 = data()
    labelled.copy_(torch.from_numpy(lab1))
    for d, src in zip(xs + [labels, counts], xs1 + [labels1, counts1]):
        d.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, expect(lab1, xs1, labels1, counts1)):
        assert torch.equal(a.cpu(), b)
    assert sel.errors() == {"truncated": 0, "under_full": 0} and sel.n_sel.tolist() == [K]


@pytest.mark.gpu
def test_labelled_windows_is_the_label_frame_map_of_the_reference_fixture(dev):
    """LabelStreams.labelled_windows(): per row, True exactly at the windows frame_2_window names (tests/golden/label_streams.npz, what
    the reference's labels_and_ev_repr_timestamps returned), cut to the row's n_windows; it agrees with the `labelled` output of
    `labels`, so a loader that counts K from it gets the n_sel of the device table"""
    from sast_amd import functional as SF
    from test_label_streams import _fx, _streams, _words
    fx = _fx()
    names = ["gen1", "single"]
    ls = _streams([_words(n) for n in names], "gen1", "train")
    got = ls.labelled_windows()
    assert len(got) == 2
    for n, g in zip(names, got):
        want = np.zeros(len(fx[f"{n}/train/ends_us"]), bool)
        want[fx[f"{n}/train/frame_2_window"]] = True
        assert g.dtype == np.bool_ and np.array_equal(g, want), n
    T = 6
    window = torch.arange(T, dtype=torch.int64).view(T, 1).repeat(1, 2).contiguous().to(dev)          # windows 0 .. 5 of both rows
    labelled = ls.labels(window)[3]
    host = np.array([[bool(g[w]) if w < len(g) else False for g in got] for w in range(T)])
    assert np.array_equal(labelled.cpu().numpy().astype(bool), host)
    K = int(host.sum())
    assert K > 0
    sel = SF.SelectionTable(T, 2, K, dev).update(labelled, check=True)
    assert sel.n_sel.tolist() == [K]


# ------------------------------------------------------------------------------------------------ the step
@pytest.fixture(scope="module")
def model_params():
    from oracle import sast_oracle as O
    ocfg = O.BackboneCfg(in_res_hw=HW, partition_size=PART, embed_dim=EMBED, amp=2e-2)
    return (O.init_backbone_params(ocfg, seed=61, ls_init=0.5), O.init_pafpn_params((64, 128, 256), seed=62),
            O.init_head_params((64, 128, 256), num_classes=NUM_CLASSES, seed=63))


def _rig(dev, model_params):
    """the rig of test_gpu_parity.test_label_sparse_sequence_step; lr 0: the parameters stay put, gradients are what is compared"""
    from sast_amd.detection import RNNDetector, YOLOPAFPN, YOLOXHead
    from sast_amd.training import TrainStep
    from test_gpu_parity import _rcfg, load_params
    net = RNNDetector(_rcfg(HW, PART, EMBED, 2e-2, 0.5)).to(dev)
    fpn = YOLOPAFPN(depth=0.67, in_stages=(2, 3, 4), in_channels=(64, 128, 256)).to(dev).train()
    head = YOLOXHead(num_classes=NUM_CLASSES, strides=(8, 16, 32), in_channels=(64, 128, 256)).to(dev).train()
    for m, p in zip((net, fpn, head), model_params):
        load_params(m, p)
    return TrainStep(net, fpn, head, lr=0.0, segmented=True)


def _frames(seed):
    from oracle import sast_oracle as O
    return [O.count_events(BATCH, HW, seed=seed + t, density=0.05) for t in range(T_SEQ)]


def _labels(indices, seed):
    """labels of the K selected pairs in gather order [K, M, 5], and the full [T, B, M, 5] / [T, B] tensors that hold the same rows at
    the selected pairs and OTHER boxes everywhere else (a step that reads an unselected row gets a different loss)"""
    from oracle import sast_oracle as O
    pairs = [(t, b) for t, idx in enumerate(indices) for b in idx]
    lab_k = O.synthetic_labels(len(pairs), HW, NUM_CLASSES, max_labels=MAX_LABELS, seed=seed)
    lab_tb = O.synthetic_labels(T_SEQ * BATCH, HW, NUM_CLASSES, max_labels=MAX_LABELS, seed=seed + 1000).view(T_SEQ, BATCH, MAX_LABELS, 5).clone()
    for j, (t, b) in enumerate(pairs):
        lab_tb[t, b] = lab_k[j]
    counts = (lab_tb.abs().sum(-1) > 0).sum(-1).to(torch.int32)
    labelled = torch.zeros(T_SEQ, BATCH, dtype=torch.uint8)
    for t, b in pairs:
        labelled[t, b] = 1
    return lab_k, lab_tb, counts, labelled


def _steps_close(a, b, what):
    """a: the device-selection step, b: the host-index twin.  Figures first, then the assertions."""
    LOSS_RTOL, GRAD_RTOL = _bars()
    torch.cuda.synchronize()
    la, lb = float(a.loss.detach()), float(b.loss.detach())
    ga, gb = a.flat.grad, b.flat.grad
    scale = float(gb.abs().max())
    err = float((ga - gb).abs().max())
    print(f"[device-selection] {what}: loss {la:.9g} vs {lb:.9g} (rel {abs(la - lb) / abs(lb):.3e}, bar {LOSS_RTOL:.1e}); "
          f"flat gradient max err {err:.3e} of max-norm {scale:.3e} (rel {err / scale:.3e}, bar {GRAD_RTOL:.1e}); P {[int(p) for p in a.P]}")
    assert [int(p) for p in a.P] == [int(p) for p in b.P], what
    assert scale > 0 and torch.isfinite(ga).all()
    assert abs(la - lb) <= LOSS_RTOL * abs(lb), (what, la, lb)
    assert err <= GRAD_RTOL * scale, (what, err, scale)


@pytest.mark.gpu
def test_step_with_device_selection_matches_host_indices(dev, model_params):
    """eager: ts.step(xs, None, labels_K, indices) on one rig, ts.step(xs, None, labels_TB, selection=sel) on its twin -- kept-token
    counts, loss and flat gradient.  Measured on the MI355X (profiles/r15_device_selection.txt): loss rel <= 8.1e-08 (bar 8.2e-07), flat
    gradient 5.1e-07 .. 5.4e-07 of its max-norm (bar 1.07e-05)."""
    from sast_amd import functional as SF
    indices = [[0, 2], [], [0, 1, 2]]
    lab_k, lab_tb, counts, labelled = _labels(indices, seed=64)
    xs = [x.to(dev) for x in _frames(70)]
    host, devs = _rig(dev, model_params), _rig(dev, model_params)
    host.step(xs, None, lab_k.to(dev), indices)
    sel = SF.SelectionTable(T_SEQ, BATCH, len(lab_k), dev).update(labelled.to(dev), check=True)
    devs.step(xs, None, lab_tb.to(dev), selection=sel, label_counts=counts.to(dev))
    _steps_close(devs, host, "eager step")
    assert devs.label_counts.tolist() == [int(counts[t, b]) for t, idx in enumerate(indices) for b in idx]
    assert torch.equal(devs.losses["loss"], devs.loss)


@pytest.mark.gpu
@pytest.mark.parametrize((), [pytest.param(id="paired")])       # no argument: keeps the id, and with it the parity-record key, of this case
def test_captured_step_replays_new_pattern_resets_and_carried_states(dev, model_params):
    """captured with the pattern [[0, 2], [], [1]]; replayed with new frames, the pattern [[1], [0, 2], []], reset = [0, 1, 0] and
    carry_states=True, against the twin's eager step with host indices from states reset by RNNStates.reset; replayed once more, it has
    continued from the states it carried; a table whose n_sel is not the captured K raises under check=True, an unknown key is a KeyError.
    Measured on the MI355X (profiles/r15_device_selection.txt): loss rel 0 in every phase; flat gradient 3.8e-07 .. 9.9e-07 of its
    max-norm (bar 1.07e-05)."""
    from sast_amd import functional as SF
    from sast_amd.detection.sequence import RNNStates
    ind0, ind1 = [[0, 2], [], [1]], [[1], [0, 2], []]
    K = 3
    lab_k0, lab_tb0, counts0, labelled0 = _labels(ind0, seed=64)
    lab_k1, lab_tb1, counts1, labelled1 = _labels(ind1, seed=65)
    host, devs = _rig(dev, model_params), _rig(dev, model_params)
    # sequence 0 on the twin (host indices, fresh states): where both rigs start from
    host.step([x.to(dev) for x in _frames(70)], None, lab_k0.to(dev), ind0)
    start = [(h.detach().clone(), c.detach().clone()) for h, c in host.states]
    # the static inputs of the captured step
    xs = [x.to(dev) for x in _frames(70)]
    states = [(h.clone(), c.clone()) for h, c in start]
    lab_tb, counts, labelled = lab_tb0.to(dev), counts0.to(dev), labelled0.to(dev)
    reset = torch.zeros(BATCH, dtype=torch.uint8, device=dev)
    sel = SF.SelectionTable(T_SEQ, BATCH, K, dev).update(labelled, check=True)
    kw = dict(selection=sel, reset=reset, carry_states=False, label_counts=counts)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        devs.step(xs, states, lab_tb, **kw)                  # eager warm-up (nothing carried, nothing reset: the states are untouched)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for sa, sb in zip(states, start) for a, b in zip(sa, sb))
    devs.capture(xs, states, lab_tb, key=K, **dict(kw, carry_states=True))
    with pytest.raises(KeyError):
        devs.replay(key=K + 1)
    # sequence 1: new frames, new labels, new pattern, sample 1 starts a new recording
    new_xs = _frames(80)
    for d, src in zip(xs, new_xs):
        d.copy_(src)
    lab_tb.copy_(lab_tb1)
    counts.copy_(counts1)
    labelled.copy_(labelled1)
    reset.copy_(torch.tensor([0, 1, 0], dtype=torch.uint8))
    sel.update(labelled, check=True)
    devs.replay(key=K)
    rs = RNNStates()
    rs.save_states_and_detach(worker_id=0, states=start)
    rs.reset(worker_id=0, indices_or_bool_tensor=torch.tensor([False, True, False]))
    host.step([x.to(dev) for x in new_xs], rs.get_states(0), lab_k1.to(dev), ind1)
    _steps_close(devs, host, "replay 1 (new pattern, reset [0, 1, 0])")
    assert devs.label_counts.tolist() == [int(counts1[t, b]) for t, idx in enumerate(ind1) for b in idx]
    for (h_in, c_in), (h, c) in zip(states, devs.states):      # carried: the input tensors now hold the final states
        assert torch.equal(h_in, h) and torch.equal(c_in, c)
        assert float(h_in[1].abs().max()) > 0.0
    carried = [(h.clone(), c.clone()) for h, c in states]
    loss1 = float(devs.loss)
    # once more, nothing reset: the replay continues from what it carried
    reset.zero_()
    devs.replay(key=K)
    host.step([x.to(dev) for x in new_xs], carried, lab_k1.to(dev), ind1)
    _steps_close(devs, host, "replay 2 (continues from the carried states)")
    assert float(devs.loss) != loss1
    assert not torch.equal(states[0][0], carried[0][0])
    # a K that has no graph: the caller's fallback is the eager step, between replays of the captured one; then the graph again
    carried = [(h.clone(), c.clone()) for h, c in states]
    devs.step(xs, states, lab_tb, **dict(kw, carry_states=True))
    host.step([x.to(dev) for x in new_xs], carried, lab_k1.to(dev), ind1)
    _steps_close(devs, host, "eager step between replays")
    assert all(torch.equal(a, b) for sa, sb in zip(states, devs.states) for a, b in zip(sa, sb))
    carried = [(h.clone(), c.clone()) for h, c in states]
    devs.replay(key=K)
    host.step([x.to(dev) for x in new_xs], carried, lab_k1.to(dev), ind1)
    _steps_close(devs, host, "replay 3 (after the eager step)")
    # a pattern with another number of pairs does not fit the captured K
    for bad, word in ((torch.tensor([[1, 1, 0], [0, 1, 0], [1, 0, 0]]), "truncated"), (torch.tensor([[0, 0, 0], [0, 1, 0], [1, 0, 0]]), "under-full")):
        with pytest.raises(ValueError, match=word):
            sel.update(bad.to(torch.uint8).to(dev), check=True)
