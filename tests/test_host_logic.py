"""CPU tests of the host side: the C-ABI library loads and exports every declared symbol (no compute calls),
the product package never touches the oracle, config mirrors, flat-parameter data-parallel plumbing over gloo."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from sast_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from sast_amd import build
        build.build()
    lib = _lib.lib()
    names = _lib.declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), n
        assert n in _lib._SIGNATURES, f"{n} declared in include/sast_hip.h but not bound in sast_amd/_lib.py"
    assert lib.sast_version() >= 100


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "sast_amd")
    for d, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".h")):
                txt = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", txt, re.M), os.path.join(d, f)
                assert "sast_oracle" not in txt, os.path.join(d, f)


def test_kernel_sources_carry_no_parked_compile_time_switches():
    """the only SAST_* names a preprocessor conditional under csrc/ may test are the arithmetic classes (builds something uses) and the
    timeline instrumentation (tools/*timeline*.py, tools/gemm_kloop_cycles.py); see DESIGN "Retired compile-time switches" """
    kept = {"SAST_MFMA_SPLIT3", "SAST_MFMA_BF16",
            "SAST_TL", "SAST_TL_ENABLE", "SAST_TL_JOB", "SAST_TLF", "SAST_TLF_ENABLE", "SAST_FUSED_TL"}
    csrc = os.path.join(ROOT, "sast_amd", "csrc")
    seen = {}
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".cuh", ".h", ".inc")):
            continue
        for n, line in enumerate(open(os.path.join(csrc, f)), 1):
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                for name in re.findall(r"\bSAST_[A-Z0-9_]+\b", line):
                    seen.setdefault(name, f"{f}:{n}")
    parked = {k: v for k, v in seen.items() if k not in kept}
    assert not parked, (f"compile-time switch(es) {parked} in the kernel sources: experiments are measured in a variant build and then "
                        "either adopted as plain code or recorded in DESIGN, not parked behind a switch")


def test_hot_path_fails_loudly_without_gpu():
    from sast_amd import functional as SF
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SF.non_zero_ratio(torch.zeros(1, 20, 32, 32))
    from sast_amd.layers import SAST_block
    from sast_amd.detection import PositionEmbeddingSine
    blk = SAST_block(64, dict(partition_size=(4, 5), mlp_activation="gelu"), first_block=True)
    pe = PositionEmbeddingSine(32, normalize=True, input_size=(1, 8, 10))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blk(torch.randn(1, 8, 10, 64), pe, torch.rand(1, 20), None)


def test_modified_hw_and_state_dict_keys():
    from sast_amd.config import modified_hw, backbone_config
    assert modified_hw((360, 640)) == ((384, 640), (6, 10))       # 1Mpx, config/modifier.py:27-41
    assert modified_hw((240, 304), 1) == ((256, 320), (8, 10))    # Gen1: partition_split_32 = 1 (config/experiment/gen1)
    from sast_amd.detection import RNNDetector, YOLOPAFPN, PositionEmbeddingSine
    from oracle import sast_oracle as O
    net = RNNDetector(backbone_config((128, 160), (4, 5), embed_dim=32))
    ref = O.init_backbone_params(O.BackboneCfg(in_res_hw=(128, 160), partition_size=(4, 5), embed_dim=32))
    mine = {k: tuple(v.shape) for k, v in net.state_dict().items() if "sub_layers" not in k}
    assert mine == {k: tuple(v.shape) for k, v in ref.items()}    # reference names + shapes
    assert "stages.0.att_blocks.0.att.win_attn.sub_layers.3.net.0.proj.weight" in net.state_dict()   # aliased duplicates
    fpn = YOLOPAFPN(depth=0.67, in_channels=(64, 128, 256))
    fr = O.init_pafpn_params((64, 128, 256))
    assert {k for k in fpn.state_dict() if "num_batches" not in k} == set(fr)
    pe = PositionEmbeddingSine(32, normalize=True, input_size=(1, 16, 20))
    assert torch.equal(pe.pos_embedding, O.position_embedding_sine(16, 20, 64))


def test_partition_maps_match_oracle():
    from sast_amd.layers import ops
    from oracle import sast_oracle as O
    x = torch.arange(2 * 12 * 20 * 3, dtype=torch.float32).view(2, 12, 20, 3)
    for mine, ref in ((ops.window_partition, O.window_partition), (ops.grid_partition, O.grid_partition)):
        assert torch.equal(mine(x, (6, 10)), ref(x, (6, 10)))
    w = ops.window_partition(x, (6, 10))
    assert torch.equal(ops.window_reverse(w, (6, 10), (12, 20)), x)
    g = ops.grid_partition(x, (6, 10))
    assert torch.equal(ops.grid_reverse(g, (6, 10), (12, 20)), x)


_DIST_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from sast_amd.dist import FlatParams, FusedAdamW
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.manual_seed(0)
m = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4))
conv = torch.nn.Module(); w = torch.empty(4, 3, 3, 2); torch.nn.init.normal_(w); conv.weight = torch.nn.Parameter(w.permute(0, 3, 1, 2))
fp = FlatParams([m, conv])
assert conv.weight.permute(0, 2, 3, 1).is_contiguous() and conv.weight.grad.stride() == conv.weight.stride()
opt = FusedAdamW(fp, lr=1e-2)
ref = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4)); ref.load_state_dict(m.state_dict())
ropt = torch.optim.AdamW(ref.parameters(), lr=1e-2, weight_decay=0.0)
xs = [torch.randn(5, 8, generator=torch.Generator().manual_seed(100 + r)) for r in range(world)]
for step in range(3):
    fp.zero_grad()
    out = m(xs[rank]); loss = (out ** 2).mean()
    # emulate the fused in-place accumulation of the HIP backward: grads are added into the flat views
    gs = torch.autograd.grad(loss, list(m.parameters()))
    for p, g in zip(m.parameters(), gs): p.grad.add_(g)
    fp.all_reduce(); opt.step(grad_scale=1.0 / world)
    ropt.zero_grad(); sum((ref(x) ** 2).mean() for x in xs).div(world).backward(); ropt.step()
for a, b in zip(m.parameters(), ref.parameters()):
    assert torch.allclose(a, b, atol=1e-6), (a - b).abs().max()
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
import os as _os, sys as _sys
_sys.stdout.flush()
_os._exit(0)      # (skip interpreter teardown: gloo's pair destructors abort now and then when 8 peers close their sockets together)
'''


def test_flat_params_allreduce_adamw_gloo_world2(tmp_path):
    """N>1 path on CPU: 2 ranks, gloo; averaged gradients + fused AdamW == single-process AdamW on the mean loss."""
    script = tmp_path / "worker.py"
    script.write_text(_DIST_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29731", str(script), ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2


_INPLACE_DDP_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from sast_amd import functional as SF
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
mode = sys.argv[2]
SF.set_autograd_visible_grads(mode == "visible")


class Lin(torch.autograd.Function):
    """a linear layer under sast_amd's parameter-gradient contract (functional._ParamGrads): in-place mode = accumulate into `.grad`
    and return None on the parameter's autograd edge; autograd-visible mode = return the buffer"""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x)
        ctx.w = w
        return x @ w.t()

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        pg = SF._ParamGrads(ctx.w)
        pg[0].add_(dy.t() @ x)                 # what the backward kernels do: "+=" into the buffer they are handed
        return dy @ ctx.w, pg.out()[0]


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w1 = torch.nn.Parameter(torch.randn(4, 3))
        self.w2 = torch.nn.Parameter(torch.randn(2, 4))

    def forward(self, x):
        return Lin.apply(Lin.apply(x, self.w1), self.w2)


torch.manual_seed(0)
net = Net()
ddp = torch.nn.parallel.DistributedDataParallel(net, find_unused_parameters=False, gradient_as_bucket_view=True)     # train.py:96-98
for it, set_to_none in enumerate((True, True, False)):
    ddp.zero_grad(set_to_none=set_to_none)
    torch.manual_seed(100 * it + rank)
    x = torch.randn(5, 3)
    ddp(x).pow(2).sum().backward()
    xs = [torch.zeros_like(x) for _ in range(world)]
    dist.all_gather(xs, x)
    ref1, ref2 = 0, 0
    for xx in xs:                              # DDP: the mean of the ranks' gradients
        w1, w2 = net.w1.detach().clone().requires_grad_(True), net.w2.detach().clone().requires_grad_(True)
        ((xx @ w1.t()) @ w2.t()).pow(2).sum().backward()
        ref1, ref2 = ref1 + w1.grad / world, ref2 + w2.grad / world
    assert torch.allclose(net.w1.grad, ref1, rtol=1e-5, atol=1e-6), (mode, it, float((net.w1.grad - ref1).abs().max()))
    assert torch.allclose(net.w2.grad, ref2, rtol=1e-5, atol=1e-6), (mode, it)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, mode, "ok")
import os as _os, sys as _sys
_sys.stdout.flush()
_os._exit(0)      # (skip interpreter teardown: gloo's pair destructors abort now and then when 8 peers close their sockets together)
'''


@pytest.mark.parametrize("mode", ["inplace", "visible"])
def test_parameter_gradient_contract_under_ddp_gloo_world2(tmp_path, mode):
    """the assumption the in-place gradient contract rests on, pinned for THIS torch: when a Function returns None for a parameter, the
    parameter's AccumulateGrad node still runs (with an undefined gradient) and DistributedDataParallel's hooks on it fire -- after the
    backward that filled `.grad` in place -- so DDP (find_unused_parameters=False, gradient_as_bucket_view=True: the reference's strategy,
    train.py:96-98) reduces the right values over three iterations, with grads set to None and zeroed in place (bucket views).  The
    autograd-visible mode must give the same.  (The real modules run the same scenario on the GPU:
    test_reference_ddp_caller_with_sync_batchnorm.)"""
    script = tmp_path / "worker.py"
    script.write_text(_INPLACE_DDP_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29733" if mode == "inplace" else "29734", str(script), ROOT, mode],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2


def test_positive_linear_forward_matches_reference_expression():
    """SAST.py:325-328: F.linear(input, exp(weight), bias) -- the stand-alone module computes (inside SAST_block it is fused)"""
    import torch
    from sast_amd.layers.sast import PositiveLinear
    torch.manual_seed(0)
    m = PositiveLinear(20, 8, bias=True)
    x = torch.rand(3, 20)
    assert torch.equal(m(x), torch.nn.functional.linear(x, m.weight.exp(), m.bias))


def test_onecycle_lr_matches_torch():
    """dist.OneCycleLR (the closed form the fused AdamW kernel evaluates on the device) == torch.optim.lr_scheduler.OneCycleLR as
    the reference configures it (modules/detection.py:418-431), every step of a short and of the shipped 400k-step schedule"""
    import torch
    from sast_amd.dist import OneCycleLR
    for total, pct in ((400000, 0.005), (50, 0.3)):
        lin = torch.nn.Linear(2, 2)
        opt = torch.optim.AdamW(lin.parameters(), lr=2e-4)
        sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=2e-4, div_factor=25, final_div_factor=10000 / 25, total_steps=total, pct_start=pct,
                                                  cycle_momentum=False, anneal_strategy='linear')
        mine = OneCycleLR(2e-4, total, pct, 25, 10000)
        for k in range(min(total, 2500)):
            assert abs(opt.param_groups[0]['lr'] - mine.lr_at(k)) <= 1e-12 * 2e-4, k
            opt.step()
            if k < total - 1:
                sch.step()


_DDP_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from oracle import sast_oracle as O              # test infrastructure: produces the per-rank gradients that are injected
from sast_amd.config import backbone_config
from sast_amd.detection import RNNDetector, YOLOPAFPN
from sast_amd.dist import FlatParams, FusedAdamW, OneCycleLR
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
hw, part, E, Bl = (128, 160), (4, 5), 32, 2
ocfg = O.BackboneCfg(in_res_hw=hw, partition_size=part, embed_dim=E, amp=2e-2)
params = O.init_backbone_params(ocfg, seed=3, ls_init=0.5)
fparams = O.init_pafpn_params((64, 128, 256), seed=4)
net = RNNDetector(backbone_config(hw, part, embed_dim=E, AMP=2e-2, ls_init_value=0.5))          # the REAL modules (CPU parameters only:
fpn = YOLOPAFPN(depth=0.67, in_stages=(2, 3, 4), in_channels=(64, 128, 256))                      # their forward needs the MI355X)
def load(module, p):
    sd = module.state_dict(); new = {}
    for k in sd:
        kk = k
        for a, b in (("sub_layers.0.", "ls1."), ("sub_layers.2.", "norm2."), ("sub_layers.3.", "mlp."), ("sub_layers.4.", "ls2.")):
            kk = kk.replace(a, b)
        new[k] = sd[k] if kk.endswith("num_batches_tracked") else p[kk]
    module.load_state_dict(new, strict=True)
load(net, params); load(fpn, fparams)
stages = list(net.stages)
flat = FlatParams([], buckets=[[fpn], [stages[3]], [stages[2], stages[1], stages[0]]])       # the bucket layout of training.TrainStep
sched = OneCycleLR(1e-3, total_steps=10, pct_start=0.3)
opt = FusedAdamW(flat, lr=1e-3, schedule=sched, clip_value=1.0)
names = {}
for mod, pre in ((net, "net."), (fpn, "fpn.")):
    for k, v in mod.named_parameters():
        names.setdefault(id(v), pre + k)

def oracle_grads(x, P, F):
    po = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    pf = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in F.items()}
    out, _s, _P = O.backbone(x, None, po, ocfg)
    O.proxy_loss(O.pafpn({k: out[k] for k in (2, 3, 4)}, pf, training=True)).backward()      # BatchNorm batch statistics of THIS shard only
    return po, pf

def current(mod, pre):
    return {k: v.detach().clone() for k, v in mod.state_dict().items() if "sub_layers" not in k}

xs = [O.count_events(Bl, hw, seed=10 + r, density=0.05) for r in range(world)]
# single-process reference: "world independent replicas + averaged gradients" (SURVEY 8e), torch.optim.AdamW + OneCycleLR + clip by value
ref_p = {("net." + k): v.clone().requires_grad_(True) for k, v in current(net, "net.").items()}
ref_f = {("fpn." + k): (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone()) for k, v in current(fpn, "fpn.").items()}
ref_all = {**ref_p, **{k: v for k, v in ref_f.items() if v.requires_grad}}
ropt = torch.optim.AdamW(list(ref_all.values()), lr=1e-3, weight_decay=0.0)
rsch = torch.optim.lr_scheduler.OneCycleLR(ropt, max_lr=1e-3, div_factor=25, final_div_factor=10000 / 25, total_steps=10, pct_start=0.3,
                                           cycle_momentum=False, anneal_strategy='linear')
for step in range(3):
    # ---- this rank: gradients of its shard, injected into the flat views (what the HIP backward does in place)
    po, pf = oracle_grads(xs[rank], current(net, "net."), current(fpn, "fpn."))
    flat.zero_grad()
    for prm in flat.params:
        n = names[id(prm)]
        g = (po if n.startswith("net.") else pf)[n[4:]].grad
        prm.grad.add_(g)
    opt.begin_step()
    for b in (0, 1, 2):                       # bucket order of the segmented backward
        flat.all_reduce(bucket=b)
        opt.update(grad_scale=1.0 / world, bucket=b)
    # ---- reference
    ropt.zero_grad()
    acc = {k: torch.zeros_like(v) for k, v in ref_all.items()}
    for r in range(world):
        P = {k[4:]: v.detach() for k, v in ref_p.items()}
        F = {k[4:]: v.detach() for k, v in ref_f.items()}
        qo, qf = oracle_grads(xs[r], P, F)
        for k in acc:
            acc[k] += (qo if k.startswith("net.") else qf)[k[4:]].grad / world
    for k, v in ref_all.items():
        v.grad = acc[k].clamp(-1.0, 1.0)
    ropt.step(); rsch.step()
worst = 0.0
for prm in flat.params:
    n = names[id(prm)]
    worst = max(worst, float((prm.detach() - ref_all[n].detach()).abs().max()))
assert worst <= 1e-5, worst      # updates are lr-sized (up to 1e-3 per step): <= 1 % of one update after 3 steps (measured 2.6e-6)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok", worst)
import os as _os, sys as _sys
_sys.stdout.flush()
_os._exit(0)      # (skip interpreter teardown: gloo's pair destructors abort now and then when 8 peers close their sockets together)
'''


@pytest.mark.parametrize("world", [2, 8])
def test_replicas_bucketed_allreduce_equals_averaged_single_process_gloo(tmp_path, world):
    """SURVEY 8(e) parity for the data-parallel path, on CPU: 2 ranks, and the 8 ranks of BASELINE config C4 (bucket ranges, grad_scale =
    1 / world and the bucket order have to hold there too) (gloo), the REAL modules' parameters re-homed into the bucketed
    flat buffers of training.TrainStep, per-rank gradients (oracle, rank-local BatchNorm statistics) injected into the flat views,
    per-bucket all-reduce + fused AdamW (OneCycleLR, clip by value)  ==  one process that evaluates both shards as independent replicas,
    averages the gradients and steps torch.optim.AdamW + torch OneCycleLR.  Three optimizer steps."""
    script = tmp_path / "ddp_worker.py"
    script.write_text(_DDP_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2" if world == 2 else "1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(29741 + world), str(script), ROOT], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == world


def test_kink_aware_scores_gradient_comparison():
    """parity_helpers.scores_grads_close on the CPU: a 'device' gradient that differs from the reference only by the ReLU decision of a
    few pre-activations within rounding of zero passes at GRAD_RTOL; one that differs anywhere else (an O(1e-3) error in a row without
    ambiguous elements, or a wrong contribution of an ambiguous one) fails."""
    import pytest
    from parity_helpers import scores_grads_close
    g = torch.Generator().manual_seed(0)
    n, C = 4000, 32
    x = torch.randn(n, C, generator=g)
    W = (torch.randn(C, C, generator=g) * 0.2).requires_grad_(True)
    b = (torch.randn(C, generator=g) * 0.1).requires_grad_(True)
    # plant pre-activations within 1e-7 of the kink: solve for the bias-free hit by nudging the rows of x
    z0 = torch.nn.functional.linear(x, W, b).detach()
    planted = [(5, 3), (77, 3), (1234, 17), (3999, 30)]
    for t, c in planted:
        x[t] -= (z0[t, c] - 1e-7 * (1 if (t % 2) else -1)) * W[c].detach() / W[c].detach().pow(2).sum()
    z = torch.nn.functional.linear(x, W, b)
    s = torch.relu(z)
    s.retain_grad()
    w_out = torch.randn(n, C, generator=g)
    (torch.sigmoid(s) * w_out).sum().backward()
    rec = [{"x": x, "z": z, "s": s}]
    rW, rb = W.grad.clone(), b.grad.clone()
    for t, c in planted:
        assert abs(float(z[t, c].detach())) < 1e-5 * float(z.detach().abs().max())
    # the "device": every planted element decided the other way
    dW, db = rW.clone(), rb.clone()
    for t, c in planted:
        sign = -1.0 if float(z[t, c]) > 0 else 1.0
        dW[c] += sign * s.grad[t, c] * x[t]
        db[c] += sign * s.grad[t, c]
    scores_grads_close("blk.", dW, db, rW, rb, rec)
    bad = dW.clone()
    bad[9] += 2e-3 * float(rW.abs().max())                       # a row without ambiguous elements
    with pytest.raises(AssertionError):
        scores_grads_close("blk.", bad, db, rW, rb, rec)
    bad = dW.clone()
    bad[3] += 3.0 * s.grad[5, 3] * x[5]                          # more than flipping every ambiguous element of the row could move it
    if float((2.0 * s.grad[5, 3] * x[5]).abs().max()) > 1e-3 * float(rW.abs().max()):
        with pytest.raises(AssertionError, match="raw error exceeds"):
            scores_grads_close("blk.", bad, db, rW, rb, rec)
    bad = dW.clone()
    bad[3] += 0.4 * s.grad[5, 3] * x[5]                          # a fractional (impossible) share of an ambiguous element
    if float((0.4 * s.grad[5, 3] * x[5]).abs().max()) > 1e-3 * float(rW.abs().max()):
        with pytest.raises(AssertionError):
            scores_grads_close("blk.", bad, db, rW, rb, rec)


def test_convert_sync_batchnorm_marks_every_unit_and_is_inert_on_one_rank():
    """train.py:167 (sync_batchnorm under DDP): the conversion shares ONE group object between all conv + BatchNorm + SiLU units and the
    models that open a pass; without a process group (world 1) it is inactive, so the fused two-conv launches stay in use"""
    from sast_amd.detection import YOLOPAFPN, YOLOXHead, BaseConv, convert_sync_batchnorm
    from sast_amd.detection.network_blocks import sync_active
    from sast_amd.functional import SyncBatchNormGroup
    fpn = YOLOPAFPN(depth=0.33, in_stages=(2, 3, 4), in_channels=(16, 32, 64))
    head = YOLOXHead(num_classes=2, strides=(8, 16, 32), in_channels=(16, 32, 64))
    both = torch.nn.ModuleList([fpn, head])
    keys = list(both.state_dict().keys())
    assert convert_sync_batchnorm(both) is both
    units = [m for m in both.modules() if isinstance(m, BaseConv)]
    assert len(units) > 20 and all(isinstance(m.sync_bn, SyncBatchNormGroup) for m in units)
    assert len({id(m.sync_bn) for m in units} | {id(fpn._sync_group), id(head._sync_group)}) == 1
    assert not fpn._sync_group.active() and not any(sync_active(m) for m in units)
    assert list(both.state_dict().keys()) == keys          # same parameters / buffers / names: checkpoints are unaffected
    g = SyncBatchNormGroup()
    g._ratio = (7, 2)                                      # 7 samples over all ranks, 2 here
    assert g.rows_total(2 * 40 * 50, 2) == 7 * 40 * 50
    with pytest.raises(RuntimeError):
        g.rows_total(3 * 40 * 50, 3)                       # a pass with another local batch needs its own exchange


def test_sync_batchnorm_group_forced_and_capturable():
    """round 4: the statistics all-reduces are captured into the step's hipGraphs on RCCL.  Host logic of the group: `force` keeps the
    two-phase path on with one rank (the single-GPU check of the capture), a group without a process group is capturable (nothing to
    enqueue), and with one rank the sample-count exchange needs no collective"""
    from sast_amd.functional import SyncBatchNormGroup
    g = SyncBatchNormGroup()
    assert not g.active() and g.capturable()
    f = SyncBatchNormGroup(force=True)
    assert f.active() and f.world == 1 and f.capturable()
    f.exchange_batch(3, torch.device("cpu"))
    assert f.n_collectives == 0 and f.rows_total(3 * 8 * 10, 3) == 3 * 8 * 10
    tok = f.exchange_batch(3, torch.device("cpu"))
    x, y = torch.zeros(3, 2), torch.zeros(3, 2)
    x._sast_sync_pass = tok                                # the PAFPN tags its outputs with the pass token ...
    assert f.same_pass(x) and not f.same_pass(y)           # ... and only a head handed THOSE tensors takes the exchange over
    assert not SyncBatchNormGroup(force=True).same_pass(x)  # (another group's token does not count)
    t = torch.ones(4, dtype=torch.float64)
    f.all_reduce(t)                                        # no process group: the identity, but counted
    assert f.n_collectives == 1 and torch.equal(t, torch.ones(4, dtype=torch.float64))
    f.all_reduce_many([t, torch.ones(2, dtype=torch.float64)])     # several independent units: ONE collective
    assert f.n_collectives == 2


_SYNC_MANY_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from sast_amd.functional import SyncBatchNormGroup
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
g = SyncBatchNormGroup()
assert g.active() and g.world == world and not g.capturable()
arena = torch.zeros(40, dtype=torch.float64)               # the units' blocks are slices of one arena, NOT adjacent (their backward blocks sit between)
a, b, c = arena[0:6], arena[10:14], arena[30:40]
for i, t in enumerate((a, b, c)):
    t.fill_(float((rank + 1) * (i + 1)))
g.all_reduce_many([a, b, c])
tot = world * (world + 1) // 2
assert g.n_collectives == 1
assert torch.equal(a, torch.full((6,), 1.0 * tot, dtype=torch.float64)) and torch.equal(b, torch.full((4,), 2.0 * tot, dtype=torch.float64))
assert torch.equal(c, torch.full((10,), 3.0 * tot, dtype=torch.float64))
assert float(arena[6:10].abs().sum() + arena[14:30].abs().sum()) == 0.0      # nothing outside the blocks was touched
g.all_reduce_many([a])
assert g.n_collectives == 2 and float(a[0]) == tot * world
# ragged per-rank sample counts (a label-sparse step keeps different numbers of samples per rank, modules/detection.py:161-171): every
# BatchNorm of the pass sees rows = samples of ALL ranks x (H_out * W_out)
n_local = rank % 3 + 1
tok = g.exchange_batch(n_local, torch.device("cpu"))
n_total = sum(r % 3 + 1 for r in range(world))
assert tok == (g, n_local) and g._ratio == (n_total, n_local) and g.n_collectives == 3
assert g.rows_total(n_local * 48 * 80, n_local) == n_total * 48 * 80
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
import os as _os, sys as _sys
_sys.stdout.flush()
_os._exit(0)      # (skip interpreter teardown: gloo's pair destructors abort now and then when 8 peers close their sockets together)
'''


@pytest.mark.parametrize("world", [2, 8])
def test_sync_batchnorm_group_one_collective_for_independent_units_gloo(tmp_path, world):
    """SyncBatchNorm with several ranks (2, and the 8 of BASELINE config C4): the statistics blocks of INDEPENDENT units (CSPLayer.conv1 / conv2, the YOLOX head's levels and
    towers) travel in one collective (`SyncBatchNormGroup.all_reduce_many`; host-side backends: one flat buffer, RCCL: the coalesced
    all-reduce) -- every block summed over the ranks, nothing around them touched, one call counted."""
    script = tmp_path / "worker.py"
    script.write_text(_SYNC_MANY_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(29737 + world), str(script), ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == world


def test_torch_sync_batchnorm_conversion_is_honoured_not_silently_local():
    """the reference's own caller: Lightning's Trainer(sync_batchnorm=True) runs torch.nn.SyncBatchNorm.convert_sync_batchnorm on the model
    before DDP wraps it (train.py:166-167).  That swaps BaseConv.bn for a torch.nn.SyncBatchNorm the fused op never calls; the units
    must then take their statistics over the ranks of that module's process group (one shared SyncBatchNormGroup per process group), the
    reduction scratch must still be sized (SyncBatchNorm is not a BatchNorm2d), and the state_dict keys must not move."""
    from sast_amd.detection import YOLOPAFPN, YOLOXHead, BaseConv
    from sast_amd.detection.network_blocks import pass_sync_group, sync_active, bn_scratch_floats
    from sast_amd.functional import SyncBatchNormGroup
    fpn = YOLOPAFPN(depth=0.33, in_stages=(2, 3, 4), in_channels=(16, 32, 64))
    head = YOLOXHead(num_classes=2, strides=(8, 16, 32), in_channels=(16, 32, 64))
    both = torch.nn.ModuleList([fpn, head])
    keys = list(both.state_dict().keys())
    floats = bn_scratch_floats(fpn)
    assert pass_sync_group(fpn) is None and floats > 0
    conv = torch.nn.SyncBatchNorm.convert_sync_batchnorm(both)
    assert conv is both and list(both.state_dict().keys()) == keys
    units = [m for m in both.modules() if isinstance(m, BaseConv)]
    assert all(isinstance(m.bn, torch.nn.SyncBatchNorm) and m.sync_bn is None for m in units)
    assert bn_scratch_floats(fpn) == floats
    g = pass_sync_group(fpn)
    assert isinstance(g, SyncBatchNormGroup) and pass_sync_group(head) is g and fpn._sync_group is g
    assert all(m.sync_bn is g for m in units)
    assert not g.active() and not any(sync_active(m) for m in units)     # one process, no process group: inert like torch's module
    lone = BaseConv(8, 8, 1, 1)
    lone.bn = torch.nn.SyncBatchNorm(8)
    assert lone.sync_group() is g                                        # a unit on its own resolves to the same default-group object
    half = YOLOPAFPN(depth=0.33, in_stages=(2, 3, 4), in_channels=(16, 32, 64))
    half.lateral_conv0.bn = torch.nn.SyncBatchNorm(32)
    with pytest.raises(RuntimeError, match="only some"):
        pass_sync_group(half)


def test_param_grads_modes_on_cpu_tensors():
    """functional._ParamGrads: the in-place contract hands out `p.grad` (created zero-filled, parameter's strides) and returns None on
    the autograd edge; the autograd-visible mode hands out views of one fresh zero block and returns them; frozen parameters and
    non-parameter stand-ins accumulate into throw-away buffers in both modes."""
    from sast_amd import functional as SF
    w = torch.nn.Parameter(torch.randn(8, 3, 3, 4).permute(0, 3, 1, 2))     # channels-last conv weight
    b = torch.nn.Parameter(torch.randn(5))
    frozen = torch.nn.Parameter(torch.randn(6), requires_grad=False)
    prev = SF.set_autograd_visible_grads(False)
    try:
        pg = SF._ParamGrads(w, None, b, frozen)
        assert pg[0] is w.grad and pg[2] is b.grad and pg[1] is None and pg[3] is not None and frozen.grad is None
        assert pg[0].stride() == w.stride() and pg.out() == (None, None, None, None)
        SF.set_autograd_visible_grads(True)
        w.grad = b.grad = None
        pg = SF._ParamGrads(w, None, b, frozen)
        out = pg.out()
        assert w.grad is None and b.grad is None and out[0] is pg[0] and out[2] is pg[2] and out[1] is None and out[3] is None
        assert pg[0].shape == w.shape and pg[0].stride() == w.stride() and float(pg[0].abs().sum()) == 0.0
        assert pg[0].data_ptr() % 16 == 0 and pg[2].data_ptr() % 16 == 0
        n0 = len(SF._SCRATCH_KEEP)
        for _ in range(2 * SF._SCRATCH_KEEP_MAX):
            SF._scratch_grad(frozen)
        assert len(SF._SCRATCH_KEEP) <= SF._SCRATCH_KEEP_MAX and SF._scratch_bytes == sum(t.numel() * 4 for t in SF._SCRATCH_KEEP)
        assert n0 <= SF._SCRATCH_KEEP_MAX
    finally:
        SF.set_autograd_visible_grads(prev)


def test_glu_activation_names():
    """attention_cfg.mlp_activation (SAST.py:38,55): the reference resolves the name through layers/create_act.py:62-79 and hands MS_WSA
    the activation CLASS; the mirror accepts the name, such a class, or None (= gelu), and refuses what the GLU epilogues do not implement"""
    from sast_amd.layers.sast import _glu_activation_name, SAST_block
    from sast_amd.functional import GLU_ACTIVATIONS
    # every name of the reference's get_act_layer (layers/create_act.py:62-98); elu / celu coincide at alpha = 1; prelu carries a parameter
    assert GLU_ACTIVATIONS == {"gelu": 0, "relu": 1, "silu": 2, "swish": 2, "sigmoid": 3, "tanh": 4, "mish": 5, "relu6": 6, "leaky_relu": 7,
                               "elu": 8, "celu": 8, "selu": 9, "hard_sigmoid": 10, "hardsigmoid": 10, "hard_swish": 11, "hardswish": 11,
                               "hard_mish": 12, "prelu": 13}
    assert _glu_activation_name(None) == "gelu" and _glu_activation_name("swish") == "swish"
    assert [_glu_activation_name(c) for c in (torch.nn.GELU, torch.nn.ReLU, torch.nn.SiLU, torch.nn.Sigmoid, torch.nn.Tanh, torch.nn.Mish,
                                              torch.nn.Hardswish)] == ["gelu", "relu", "silu", "sigmoid", "tanh", "mish", "hard_swish"]
    class RefPReLU(torch.nn.PReLU):                        # the reference's own subclass (layers/activations.py:124)
        pass
    assert _glu_activation_name(torch.nn.PReLU) == _glu_activation_name(RefPReLU) == "prelu"
    with pytest.raises(NotImplementedError):
        _glu_activation_name(torch.nn.Softplus)            # not a name of get_act_layer
    cfg = dict(partition_size=(4, 5), dim_head=32, attention_bias=True, mlp_activation="relu", mlp_bias=True, mlp_ratio=4, drop_mlp=0,
               drop_path=0, ls_init_value=1e-5, enable_CB=False, AMP=2e-4, BOUNCE=1e-3)
    blk = SAST_block(64, cfg, first_block=True)
    assert blk.win_attn.mlp_activation == blk.grid_attn.mlp_activation == "relu"
    assert SAST_block(64, dict(cfg, mlp_activation="hard_mish"), first_block=True).win_attn.mlp_activation == "hard_mish"
    # prelu: ONE learnable slope per layer under the reference's state_dict name (nn.PReLU inside the GLU, init 0.25), also through the
    # aliased `sub_layers` container (SAST.py:194); the parameter-free activations add no key
    pre = SAST_block(64, dict(cfg, mlp_activation="prelu"), first_block=True)
    sd = pre.state_dict()
    for layer in ("win_attn", "grid_attn"):
        for path in ("mlp.net.0.act_layer.weight", "sub_layers.3.net.0.act_layer.weight"):
            assert tuple(sd[f"{layer}.{path}"].shape) == (1,) and float(sd[f"{layer}.{path}"]) == 0.25
    assert pre.win_attn.kernel_params()["act_w"] is pre.win_attn.mlp.net[0].act_layer.weight
    assert not any("act_layer" in k for k in blk.state_dict()) and blk.win_attn.kernel_params()["act_w"] is None
    with pytest.raises(NotImplementedError):
        SAST_block(64, dict(cfg, mlp_activation="softplus"), first_block=True)
    # dim_head: any multiple of 4 up to 32 that divides dim (SAST.py:35,171-179 accept any divisor)
    assert SAST_block(64, dict(cfg, dim_head=16), first_block=True).win_attn.num_heads == 4
    for bad in (48, 6, 64):
        with pytest.raises(NotImplementedError):
            SAST_block(96, dict(cfg, dim_head=bad), first_block=True)


def test_depthwise_modules_have_the_reference_state_dict_keys():
    """depthwise=True: DWConv = dconv (depth-wise, weight (C,1,k,k) stored [C][k*k]) + pconv (network_blocks.py:57-76); the key sets are
    the oracle's, which tests/golden/depthwise.npz was generated against with strict loading into the reference modules"""
    from sast_amd.detection import YOLOPAFPN, YOLOXHead, DWConv, BaseConv
    from oracle import sast_oracle as O
    chans = (32, 64, 128)
    fpn = YOLOPAFPN(depth=0.67, in_stages=(2, 3, 4), in_channels=chans, depthwise=True)
    assert {k for k in fpn.state_dict() if not k.endswith("num_batches_tracked")} == set(O.init_pafpn_params(chans, depthwise=True))
    head = YOLOXHead(num_classes=2, strides=(8, 16, 32), in_channels=chans, depthwise=True)
    assert {k for k in head.state_dict() if not k.endswith("num_batches_tracked")} == set(O.init_head_params(chans, num_classes=2, depthwise=True))
    d = fpn.bu_conv1
    assert isinstance(d, DWConv) and d.dconv.groups == 64 and d.dconv.stride == 2 and d.pconv.groups == 1
    w = d.dconv.conv.weight
    assert tuple(w.shape) == (64, 1, 3, 3) and w.permute(0, 2, 3, 1).is_contiguous()
    with pytest.raises(NotImplementedError):
        BaseConv(64, 64, 3, 1, groups=2)


def test_library_knobs_registry_and_reload(monkeypatch):
    """include/sast_hip.h sast_config_*: the SAST_* tuning knobs are read through one registry; a value changed in os.environ inside the
    process is seen after reload_knobs() (round-4 / round-5 advice: knobs latched at first use ignored in-process toggling silently)"""
    from sast_amd import _lib as SL
    lib = SL.lib()
    monkeypatch.delenv("SAST_TN_BLOCKS", raising=False)
    SL.reload_knobs()
    assert lib.sast_config_get(b"SAST_TN_BLOCKS", 768) == 768
    monkeypatch.setenv("SAST_TN_BLOCKS", "123")
    n = SL.reload_knobs()
    assert n >= 1
    assert lib.sast_config_get(b"SAST_TN_BLOCKS", 768) == 123
    assert SL.knobs()["SAST_TN_BLOCKS"] == 123
    monkeypatch.delenv("SAST_TN_BLOCKS")
    SL.reload_knobs()
    assert lib.sast_config_get(b"SAST_TN_BLOCKS", 768) == 768


def test_deferred_weight_gradients_are_retired():
    """deferred weight gradients left the product (tools/experiments/r06_deferred_weight_gradients.patch):
    no name of the path in the C header, in the package sources or in the built library (its whole image: the dynamic symbol table and
    the device code objects' kernel names with it), and TrainStep refuses the two keywords bench.py can still pass (no GPU needed)"""
    from sast_amd import _lib as SL
    from sast_amd.training import TrainStep
    needles = ("sast_dw_", "dw_defer", "DwGroup", "gemm_group_kernel")
    pkg = os.path.join(ROOT, "sast_amd")
    texts = [os.path.join(ROOT, "include", "sast_hip.h")]
    for d, dirs, files in os.walk(pkg):
        dirs[:] = [x for x in dirs if x not in ("build", "__pycache__")]
        texts += [os.path.join(d, f) for f in files if f.endswith((".py", ".hip", ".cuh", ".h", ".inc"))]
    assert len(texts) > 40 and os.path.join(pkg, "csrc", "gemm_dispatch.cuh") in texts
    for path in texts + [SL.lib()._name]:
        with open(path, "rb") as f:
            data = f.read()
        assert not [n for n in needles if n.encode() in data], path
    assert b"gemm_dual_kernel" in data and b"sast_version" in data       # the search does see kernel and entry-point names
    for kw in ("defer_dw", "dw_discard"):
        with pytest.raises(ValueError, match="r06_deferred_weight_gradients.patch"):
            TrainStep(None, None, **{kw: True})


def test_sync_group_forgets_a_destroyed_process_group():
    """functional.SyncBatchNormGroup is cached per process group (`sync_group_for`) and installed on the modules: after
    destroy_process_group() + a new init_process_group() in the same process it must not keep the world size, the private communicator or
    the sample ratio of the dead group (round-5 advice)"""
    import torch.distributed as dist
    from sast_amd.functional import sync_group_for
    assert not dist.is_initialized()
    g = sync_group_for(None)
    assert g.world == 1 and g._world is None                  # nothing cached while no group exists
    try:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:29533", rank=0, world_size=1)
        assert g.world == 1 and g._world == 1
        g._world, g._ratio, g._comm = 5, (20, 4), object()    # what a 5-rank group would have left behind
        dist.destroy_process_group()
        assert g.world == 1 and g._world is None and g._ratio is None and g._comm is None
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:29534", rank=0, world_size=1)
        g._world = 5                                          # (stale value written behind the validation's back)
        g._epoch = object()
        assert g.world == 1
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
