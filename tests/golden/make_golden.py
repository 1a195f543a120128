"""Generate the golden fixtures in tests/golden/ by running the upstream reference.

Runs ONLY in the build container (needs /root/reference, never present on the GPU
box).  It imports the reference (with the omegaconf/strenum stubs of
`_ref_import.py`), feeds it seeded inputs and parameters drawn by
`oracle.sast_oracle.init_*_params(seed)` (so fixtures do not have to carry the
weights), and stores inputs + expected outputs as .npz.  Fixtures are data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import _ref_import as RI  # noqa: E402
from oracle import sast_oracle as O  # noqa: E402

torch.set_num_threads(8)
MIN_MARGIN = 3e-5  # >= 300x the fp32 rounding noise on tok/softmax (~1e-7)


def np_(t):
    return t.detach().cpu().numpy()


def load_into(module, params, prefix=""):
    """copy an oracle param dict into a reference module (handles the aliased sub_layers.* keys)."""
    sd = module.state_dict()
    new = {}
    for k in sd:
        kk = k
        for a, b in ((".sub_layers.0.", ".ls1."), (".sub_layers.2.", ".norm2."),
                     (".sub_layers.3.", ".mlp."), (".sub_layers.4.", ".ls2.")):
            kk = kk.replace(a, b)
        if kk.endswith("num_batches_tracked"):
            new[k] = sd[k]
            continue
        new[k] = params[prefix + kk].clone()
    module.load_state_dict(new, strict=True)


def param_checksum(params):
    return float(sum(float(v.double().abs().sum()) for v in params.values()))


def lists_to_np(lists, tag):
    out = {}
    for li, l in enumerate(lists):
        for name, t in zip(("index_window", "index_token", "padding_index", "asy_index", "K"), l):
            out[f"{tag}l{li}_{name}"] = np_(t).astype(np.int64)
    return out


def block_params(C, seed, ls_init, nblocks=1):
    cfg = O.BackboneCfg(in_res_hw=(64, 80), partition_size=(4, 5), embed_dim=C, num_blocks=(nblocks, 1, 1, 1))
    p = O.init_backbone_params(cfg, seed=seed, ls_init=ls_init)
    return {k[len("stages.0."):]: v for k, v in p.items() if k.startswith("stages.0.att_blocks.")}


def gen_nzr(ref):
    x = O.count_events(2, (64, 96), seed=3, density=0.02)
    r = ref.sast_rnn.non_zero_ratio(x)
    assert torch.equal(r, O.non_zero_ratio(x))
    xb = O.synthetic_events(2, (64, 96), seed=4, sparsity=0.97)
    rb = ref.sast_rnn.non_zero_ratio(xb)
    np.savez_compressed(os.path.join(HERE, "nzr.npz"), x=np_(x), r=np_(r), xb=np_(xb).astype(np.int32), rb=np_(rb))
    print("nzr ok")


def run_ref_block(ref, params, x, r, pe_mod, acfg, first=True, index_list=None, pre="att_blocks.0.att."):
    blk = ref.SAST.SAST_block(x.shape[-1], RI.to_cfg(acfg), first_block=first)
    load_into(blk, params, pre)
    xx = x.clone().requires_grad_(True)
    out, cnt, lists = blk(xx, pe_mod, r, index_list)
    return blk, xx, out, cnt, lists


def gen_block(ref, name, B, amp, enable_cb=False, seed0=0, C=64, dim_head=32, bias=True, act="gelu", hw=(16, 20), part=(4, 5)):
    """bias=False: attention_bias: False and mlp_bias: False (qkv / proj / MLP linears without bias vectors, SAST.py:180-181);
    act: attention_cfg.mlp_activation (SAST.py:38,55: get_act_layer(name) -> the GLU's gate activation, ops.py:133-137);
    hw / part: map size and partition size (round 5: (24, 40) / (12, 20) = 240 tokens per partition, the gen4 model with
    partition_split_32: 1, config/modifier.py:37)"""
    H, W = hw
    acfg = dict(partition_size=part, dim_head=dim_head, attention_bias=bias, mlp_activation=act, mlp_bias=bias,
                mlp_ratio=4, drop_mlp=0, drop_path=0, ls_init_value=0.5, enable_CB=enable_cb, AMP=amp, BOUNCE=1e-3)
    ocfg = O.AttnCfg(partition_size=part, amp=amp, bounce=1e-3, enable_cb=enable_cb, dim_head=dim_head, mlp_activation=act)
    pe_mod = ref.sast_rnn.PositionEmbeddingSine(C // 2, normalize=True, input_size=(1, H, W))
    pe = O.position_embedding_sine(H, W, C)
    assert torch.equal(pe, pe_mod.pos_embedding)
    for seed in range(seed0, seed0 + 200):
        g = torch.Generator().manual_seed(1000 + seed)
        x = torch.randn(B, H, W, C, generator=g)
        r = torch.rand(B, 20, generator=g) * 0.05
        params = block_params(C, seed, 0.5)
        if not bias:
            params = {k: v for k, v in params.items() if not (k.endswith(".bias") and ("qkv." in k or "proj." in k or "mlp.net" in k))}
        if act == "prelu":      # the one activation with a parameter (layers/activations.py:124-131): a slope per layer, away from the init value
            for layer, slope in zip(("win_attn", "grid_attn"), PRELU_SLOPES):
                params[f"att_blocks.0.att.{layer}.mlp.net.0.act_layer.weight"] = torch.tensor([slope])
        blk, xx, out, cnt, lists = run_ref_block(ref, params, x, r, pe_mod, acfg)
        # margins via the oracle's scores
        _o, _c, _l, sc = O.sast_block(x, pe, r, params, "att_blocks.0.att.", ocfg, return_scores=True)
        T = part[0] * part[1]
        N = H * W // T
        mw, mt = O.selection_margins(sc, B, N, T, 1e-3)
        scg = O.grid_partition(O.window_reverse(sc.view(B * N, part[0], part[1], C), part, (H, W)), part).view(B, N, -1, C)
        mw2, mt2 = O.selection_margins(scg, B, N, T, 1e-3)
        margin = float(min(mw.min(), mt.min(), mw2.min(), mt2.min()))
        kept = [len(l[3]) for l in lists]
        if margin >= MIN_MARGIN and all(0 < k for k in kept):
            break
    else:
        raise RuntimeError("no seed with a safe margin")
    loss = (out ** 2).mean()
    loss.backward()
    # oracle must agree
    xo = x.clone().requires_grad_(True)
    po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    oo, oc, ol = O.sast_block(xo, pe, r, po, "att_blocks.0.att.", ocfg)
    assert oc == cnt
    for a, b in zip(sum(lists, []), sum(ol, [])):
        assert torch.equal(a, b)
    assert torch.equal(oo, out), float((oo - out).abs().max())
    (oo ** 2).mean().backward()
    assert torch.allclose(xo.grad, xx.grad, atol=1e-7, rtol=1e-5)
    d = dict(x=np_(x), r=np_(r), out=np_(out), count=np.int64(cnt), seed=np.int64(seed), amp=np.float64(amp),
             margin=np.float64(margin), dx=np_(xx.grad), param_checksum=np.float64(param_checksum(params)),
             enable_cb=np.int64(enable_cb), dim_head=np.int64(dim_head), bias=np.int64(bias), act=np.array(act),
             part=np.array(part, dtype=np.int64))
    if act == "prelu":
        d["prelu_slopes"] = np.array(PRELU_SLOPES, dtype=np.float32)
    d.update(lists_to_np(lists, ""))
    named = dict(blk.named_parameters())
    for k, v in named.items():
        if "sub_layers" in k:
            continue
        gk = "g_" + k
        gv = v.grad if v.grad is not None else torch.zeros_like(v)
        ref_g = po["att_blocks.0.att." + k].grad
        assert torch.allclose(ref_g, gv, atol=1e-7, rtol=1e-4), k
        d[gk] = np_(gv)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
    print(f"{name}: seed {seed} margin {margin:.2e} kept {kept} of {B * H * W} count {cnt}")


def gen_block_drop_path(ref, name="block_drop_path", pdrop=0.25, pmlp=0.0, enable_cb=False):
    """drop_path > 0 (SAST.py:42,188,193,232,248; shipped YAML: 0): DropPath on both residual branches of both MS-WSA layers, training mode,
    fixed RNG state.  The oracle (same torch calls in the same order) reproduces the reference bit for bit and records the factor
    vectors it drew (= the reference's); the fixture holds them next to the reference's outputs and gradients.
    pmlp > 0: `drop_mlp` (SAST.py:43,191 -> ops.py:167: nn.Dropout on the MLP hidden) -- its masks join the record in call order."""
    H, W, part, C, B, amp = 16, 20, (4, 5), 32, 2, 2e-2
    acfg = dict(partition_size=part, dim_head=32, attention_bias=True, mlp_activation="gelu", mlp_bias=True,
                mlp_ratio=4, drop_mlp=pmlp, drop_path=pdrop, ls_init_value=0.5, enable_CB=enable_cb, AMP=amp, BOUNCE=1e-3)
    pe_mod = ref.sast_rnn.PositionEmbeddingSine(C // 2, normalize=True, input_size=(1, H, W))
    pe = O.position_embedding_sine(H, W, C)
    T, N = part[0] * part[1], H * W // (part[0] * part[1])
    for seed in range(0, 200):
        g = torch.Generator().manual_seed(3000 + seed)
        x = torch.randn(B, H, W, C, generator=g)
        r = torch.rand(B, 20, generator=g) * 0.05
        params = block_params(C, seed, 0.5)
        ocfg0 = O.AttnCfg(partition_size=part, amp=amp, bounce=1e-3)
        _o, _c, _l, sc = O.sast_block(x, pe, r, params, "att_blocks.0.att.", ocfg0, return_scores=True)
        mw, mt = O.selection_margins(sc, B, N, T, 1e-3)
        scg = O.grid_partition(O.window_reverse(sc.view(B * N, part[0], part[1], C), part, (H, W)), part).view(B, N, -1, C)
        mw2, mt2 = O.selection_margins(scg, B, N, T, 1e-3)
        margin = float(min(mw.min(), mt.min(), mw2.min(), mt2.min()))
        if margin >= MIN_MARGIN:
            break
    else:
        raise RuntimeError("no seed with a safe margin")
    blk = ref.SAST.SAST_block(C, RI.to_cfg(acfg), first_block=True)       # a fresh module is in training mode
    load_into(blk, params, "att_blocks.0.att.")
    xx = x.clone().requires_grad_(True)
    torch.manual_seed(91)                                                  # (the constructor's parameter init consumed the generator)
    out, cnt, lists = blk(xx, pe_mod, r, None)
    (out ** 2).mean().backward()
    log = []
    ocfg = O.AttnCfg(partition_size=part, amp=amp, bounce=1e-3, drop_path=pdrop, drop_mlp=pmlp, training=True, drop_log=log, enable_cb=enable_cb)
    xo = x.clone().requires_grad_(True)
    po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    torch.manual_seed(91)
    oo, oc, ol = O.sast_block(xo, pe, r, po, "att_blocks.0.att.", ocfg)
    assert oc == cnt and torch.equal(oo, out), float((oo - out).abs().max())
    assert len(log) == 2 * ((2 if pdrop else 0) + (1 if pmlp else 0)) and all(0.1 < float((m == 0).float().mean()) < 0.4 for m in log)
    (oo ** 2).mean().backward()
    assert torch.allclose(xo.grad, xx.grad, atol=1e-7, rtol=1e-5)
    blk.eval()
    with torch.no_grad():
        eout, _ec, _el = blk(x, pe_mod, r, None)
    d = dict(x=np_(x), r=np_(r), out=np_(out), eval_out=np_(eout), count=np.int64(cnt), seed=np.int64(seed), amp=np.float64(amp),
             margin=np.float64(margin), dx=np_(xx.grad), param_checksum=np.float64(param_checksum(params)), p=np.float64(pdrop),
             p_mlp=np.float64(pmlp), rng_seed=np.int64(91), enable_cb=np.int64(enable_cb))
    for i, m in enumerate(log):
        d[f"drop{i}"] = np_(m)
    d.update(lists_to_np(lists, ""))
    for k, v in blk.named_parameters():
        if "sub_layers" in k:
            continue
        gv = v.grad if v.grad is not None else torch.zeros_like(v)
        assert torch.allclose(po["att_blocks.0.att." + k].grad, gv, atol=1e-7, rtol=1e-4), k
        d["g_" + k] = np_(gv)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **d)
    print(f"{name}: seed {seed} margin {margin:.2e} kept {[len(l[3]) for l in lists]} dropped {[float((m == 0).float().mean()) for m in log]}")


def gen_downsample_variants(ref):
    """ConvDownsampling_Cf2Cl with downsample_cfg.overlap False (k = f, no padding) and norm_affine False (ops.py:69-76,87; no shipped
    YAML): the reference module's outputs and gradients for factor 4 (stem-like, 20 input channels) and factor 2."""
    d = {}
    g = torch.Generator().manual_seed(97)
    for tag, cin, cout, f, hw in (("f4", 20, 32, 4, (16, 40)), ("f2", 32, 64, 2, (8, 20))):
        m = ref.ops.ConvDownsampling_Cf2Cl(cin, cout, f, RI.to_cfg(dict(type="patch", overlap=False, norm_affine=False)))
        w = (torch.rand(cout, cin, f, f, generator=g) * 2 - 1) / (cin * f * f) ** 0.5
        m.load_state_dict({"conv.weight": w}, strict=True)
        x = torch.randn(2, cin, *hw, generator=g)
        wy = torch.randn(2, hw[0] // f, hw[1] // f, cout, generator=g)
        xx = x.clone().requires_grad_(True)
        y = m(xx)
        (y * wy).sum().backward()
        po = {"conv.weight": w.clone().requires_grad_(True)}
        xo = x.clone().requires_grad_(True)
        yo = O.conv_downsample_cf2cl(xo, po, "", f)
        assert torch.equal(yo, y), tag
        (yo * wy).sum().backward()
        assert torch.allclose(xo.grad, xx.grad, atol=1e-7, rtol=1e-5) and torch.allclose(po["conv.weight"].grad, m.conv.weight.grad, atol=1e-6, rtol=1e-5)
        d.update({tag + "_x": np_(x), tag + "_w": np_(w), tag + "_wy": np_(wy), tag + "_y": np_(y), tag + "_dx": np_(xx.grad),
                  tag + "_dw": np_(m.conv.weight.grad)})
    np.savez_compressed(os.path.join(HERE, "downsample_variants.npz"), **d)
    print("downsample_variants ok")


ACTS_R4 = ("relu", "silu", "sigmoid", "tanh")
# round 5: the remaining parameter-free names of get_act_layer (layers/create_act.py:62-98)
ACTS_R5 = ("mish", "relu6", "leaky_relu", "elu", "celu", "selu", "hard_sigmoid", "hard_swish", "hard_mish")


PRELU_SLOPES = (0.3, 0.15)


def gen_acts(ref, names=ACTS_R4 + ACTS_R5 + ("prelu",)):
    for act in names:
        gen_block(ref, "block_act_" + act, 1, 2e-2, C=32, act=act)


def gen_big_partitions(ref):
    """partitions of more than 128 tokens: (12, 20) = 240 on a 24 x 40 map (4 partitions per sample), dense (every token kept: eight
    32-token tiles) and sparse (AMP 2e-2: partitions of different kept counts); C = 32 with two heads of 16"""
    gen_block(ref, "block_t240_dense", 2, 2e-4, C=32, dim_head=16, hw=(24, 40), part=(12, 20))
    gen_block(ref, "block_t240_sparse", 2, 2e-2, C=32, dim_head=16, hw=(24, 40), part=(12, 20))


def gen_dim_heads(ref):
    """dim_head other than the shipped 32 / 24 (SAST.py:35,171-179 accept any divisor of dim): 16 and 8 at C = 32 (2 / 4 heads)"""
    gen_block(ref, "block_dh16", 2, 2e-2, C=32, dim_head=16)
    gen_block(ref, "block_dh8", 1, 2e-2, C=32, dim_head=8)


def gen_two_blocks(ref):
    """one stage with num_blocks=2: second block reuses the first block's index lists (SAST.py:124-128)."""
    C, H, W, part = 64, 16, 20, (4, 5)
    amp = 2e-2
    acfg = dict(partition_size=part, dim_head=32, attention_bias=True, mlp_activation="gelu", mlp_bias=True,
                mlp_ratio=4, drop_mlp=0, drop_path=0, ls_init_value=0.5, enable_CB=False, AMP=amp, BOUNCE=1e-3)
    ocfg = O.AttnCfg(partition_size=part, amp=amp, bounce=1e-3)
    pe_mod = ref.sast_rnn.PositionEmbeddingSine(C // 2, normalize=True, input_size=(1, H, W))
    pe = O.position_embedding_sine(H, W, C)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, H, W, C, generator=g)
    r = torch.rand(2, 20, generator=g) * 0.05
    params = block_params(C, 5, 0.5, nblocks=2)
    _b, _xx, o1, c1, l1 = run_ref_block(ref, params, x, r, pe_mod, acfg, True, None, "att_blocks.0.att.")
    _b, _xx, o2, c2, l2 = run_ref_block(ref, params, o1.detach(), r, pe_mod, acfg, False, l1, "att_blocks.1.att.")
    a1, ac1, al1 = O.sast_block(x, pe, r, params, "att_blocks.0.att.", ocfg)
    a2, ac2, al2 = O.sast_block(a1, pe, r, params, "att_blocks.1.att.", ocfg, index_list=al1, first_block=False)
    assert torch.equal(a2, o2) and ac2 == c2
    d = dict(x=np_(x), r=np_(r), out1=np_(o1), out2=np_(o2), count1=np.int64(c1), count2=np.int64(c2),
             seed=np.int64(5), amp=np.float64(amp), param_checksum=np.float64(param_checksum(params)))
    d.update(lists_to_np(l1, ""))
    np.savez_compressed(os.path.join(HERE, "stage_two_blocks.npz"), **d)
    print("two blocks ok", c1, c2)


def gen_backbone_tiny(ref):
    """F-4: embed_dim 32, (128,160) input, partition (4,5), B=2, two timesteps (second with LSTM state)."""
    hw, part, E = (128, 160), (4, 5), 32
    for amp, tag in ((2e-4, "dense"), (2e-2, "sparse")):
        rcfg = RI.backbone_cfg(hw, part, embed_dim=E, amp=amp, ls_init=0.5)
        ocfg = O.BackboneCfg(in_res_hw=hw, partition_size=part, embed_dim=E, amp=amp)
        params = O.init_backbone_params(ocfg, seed=11, ls_init=0.5)
        net = ref.sast_rnn.RNNDetector(rcfg)
        load_into(net, params)
        x0 = O.count_events(2, hw, seed=21, density=0.05)
        x1 = O.count_events(2, hw, seed=22, density=0.05)
        out0, st0, P0 = net(x0)
        out1, st1, P1 = net(x1, [(h.detach(), c.detach()) for h, c in st0])
        loss = sum((out1[k] ** 2).mean() for k in (1, 2, 3, 4))
        loss.backward()
        oo0, os0, oP0 = O.backbone(x0, None, params, ocfg)
        oo1, os1, oP1 = O.backbone(x1, os0, params, ocfg)
        assert oP0 == P0 and oP1 == P1, (oP0, P0, oP1, P1)
        for k in (1, 2, 3, 4):
            assert torch.equal(oo0[k], out0[k]) and torch.equal(oo1[k], out1[k]), k
        d = dict(x0=np_(x0), x1=np_(x1), P0=np.array(P0), P1=np.array(P1), seed=np.int64(11), amp=np.float64(amp),
                 param_checksum=np.float64(param_checksum(params)), loss=np.float64(float(loss)))
        for k in (1, 2, 3, 4):
            d[f"h0_{k}"] = np_(out0[k])
            d[f"h1_{k}"] = np_(out1[k])
            d[f"c1_{k}"] = np_(st1[k - 1][1])
        gn = {}
        for k, v in net.named_parameters():
            if "sub_layers" in k or v.grad is None:
                continue
            gn[k] = [float(v.grad.double().norm()), float(v.grad.double().sum())]
        d["grad_stats_json"] = np.array(json.dumps(gn))
        for k in ("stages.0.att_blocks.0.att.to_scores.bias", "stages.3.lstm.conv1x1.bias",
                  "stages.1.downsample_cf2cl.norm.weight", "stages.2.att_blocks.0.att.grid_attn.ls2.gamma"):
            d["g_" + k] = np_(dict(net.named_parameters())[k].grad)
        np.savez_compressed(os.path.join(HERE, f"backbone_tiny_{tag}.npz"), **d)
        print(f"backbone_tiny_{tag}: P0 {P0} P1 {P1}")


def gen_backbone_live(ref):
    """the reference backbone on a seed no other fixture uses (embed_dim 32, (128,160), partition (4,5), B=3, AMP 2e-3, one
    timestep): inputs, outputs and kept-token counts for test_oracle_equals_reference_live."""
    hw, part = (128, 160), (4, 5)
    rcfg = RI.backbone_cfg(hw, part, embed_dim=32, amp=2e-3, ls_init=0.5)
    ocfg = O.BackboneCfg(in_res_hw=hw, partition_size=part, embed_dim=32, amp=2e-3)
    params = O.init_backbone_params(ocfg, seed=5, ls_init=0.5)
    net = ref.sast_rnn.RNNDetector(rcfg)
    load_into(net, params)
    x = O.count_events(3, hw, seed=9, density=0.03)
    with torch.no_grad():
        out, _st, P = net(x)
    d = dict(x=np_(x), P=np.array(P), seed=np.int64(5), amp=np.float64(2e-3), param_checksum=np.float64(param_checksum(params)))
    for k in (1, 2, 3, 4):
        d[f"h_{k}"] = np_(out[k])
    np.savez_compressed(os.path.join(HERE, "backbone_live.npz"), **d)
    print(f"backbone_live: P {P}")


def gen_pafpn(ref):
    chans = (64, 128, 256)
    params = O.init_pafpn_params(chans, seed=31)
    net = ref.yolo_pafpn.YOLOPAFPN(depth=0.67, in_stages=(2, 3, 4), in_channels=chans, depthwise=False, act="silu")
    sd = {k: (params[k].clone() if not k.endswith("num_batches_tracked") else v) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    g = torch.Generator().manual_seed(32)
    feats = {2: torch.randn(2, 64, 16, 20, generator=g), 3: torch.randn(2, 128, 8, 10, generator=g),
             4: torch.randn(2, 256, 4, 5, generator=g)}
    fin = {k: v.clone().requires_grad_(True) for k, v in feats.items()}
    net.train()
    outs = net(fin)
    loss = sum((o ** 2).mean() for o in outs)
    loss.backward()
    oo = O.pafpn(feats, params, training=True)
    for a, b in zip(outs, oo):
        assert torch.equal(a, b)
    d = dict(seed=np.int64(31), param_checksum=np.float64(param_checksum(params)))
    for k, v in feats.items():
        d[f"in{k}"] = np_(v)
        d[f"din{k}"] = np_(fin[k].grad)
    for i, o in enumerate(outs):
        d[f"train_out{i}"] = np_(o)
    d["rm_lateral"] = np_(net.lateral_conv0.bn.running_mean)
    d["rv_lateral"] = np_(net.lateral_conv0.bn.running_var)
    gn = {k: [float(v.grad.double().norm()), float(v.grad.double().sum())] for k, v in net.named_parameters()}
    d["grad_stats_json"] = np.array(json.dumps(gn))
    d["g_C3_p3.conv3.conv.weight"] = np_(net.C3_p3.conv3.conv.weight.grad)
    d["g_bu_conv2.bn.weight"] = np_(net.bu_conv2.bn.weight.grad)
    net.eval()
    with torch.no_grad():
        eo = net(feats)
    bufs = {k: v.clone() for k, v in net.state_dict().items()}
    ee = O.pafpn(feats, bufs, training=False)
    for i, (a, b) in enumerate(zip(eo, ee)):
        assert torch.equal(a, b)
        d[f"eval_out{i}"] = np_(a)
    np.savez_compressed(os.path.join(HERE, "pafpn.npz"), **d)
    print("pafpn ok")


def gen_depthwise(ref):
    """depthwise=True (yolo_pafpn.py:37, network_blocks.py:93, yolo_head.py:42): Bottleneck.conv2, bu_conv* and the head's tower convs
    are DWConvs (depth-wise 3x3 + BN + SiLU, then 1x1 + BN + SiLU).  PAFPN in train and eval mode, head in eval mode, reference modules."""
    chans, nc, strides = (32, 64, 128), 2, (8, 16, 32)
    params = O.init_pafpn_params(chans, seed=41, depthwise=True)
    net = ref.yolo_pafpn.YOLOPAFPN(depth=0.67, in_stages=(2, 3, 4), in_channels=chans, depthwise=True, act="silu")
    sd0 = net.state_dict()
    assert set(params) <= set(sd0), sorted(set(params) - set(sd0))[:5]
    assert {k for k in sd0 if not k.endswith("num_batches_tracked")} == set(params)
    net.load_state_dict({k: (params[k].clone() if not k.endswith("num_batches_tracked") else v) for k, v in sd0.items()})
    g = torch.Generator().manual_seed(42)
    feats = {2: torch.randn(2, chans[0], 16, 20, generator=g), 3: torch.randn(2, chans[1], 8, 10, generator=g),
             4: torch.randn(2, chans[2], 4, 5, generator=g)}
    fin = {k: v.clone().requires_grad_(True) for k, v in feats.items()}
    net.train()
    outs = net(fin)
    sum((o ** 2).mean() for o in outs).backward()
    po = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in params.items()}
    fo = {k: v.clone().requires_grad_(True) for k, v in feats.items()}
    oo = O.pafpn(fo, po, training=True)
    for a, b in zip(outs, oo):
        assert torch.equal(a, b)
    sum((o ** 2).mean() for o in oo).backward()
    d = dict(seed=np.int64(41), param_checksum=np.float64(param_checksum(params)))
    for k, v in feats.items():
        d[f"in{k}"] = np_(v)
        d[f"din{k}"] = np_(fin[k].grad)
        assert torch.allclose(fo[k].grad, fin[k].grad, atol=1e-7, rtol=1e-4)
    for i, o in enumerate(outs):
        d[f"train_out{i}"] = np_(o)
    named = dict(net.named_parameters())
    for k, v in named.items():
        assert torch.allclose(po[k].grad, v.grad, atol=1e-7, rtol=1e-3), k
    d["grad_stats_json"] = np.array(json.dumps({k: [float(v.grad.double().norm()), float(v.grad.double().sum())] for k, v in named.items()}))
    for k in ("bu_conv2.dconv.conv.weight", "bu_conv2.pconv.conv.weight", "C3_p3.m.0.conv2.dconv.conv.weight", "bu_conv1.dconv.bn.weight"):
        d["g_" + k] = np_(named[k].grad)
    d["rm_bu_dconv"] = np_(net.bu_conv2.dconv.bn.running_mean)
    d["rv_bu_dconv"] = np_(net.bu_conv2.dconv.bn.running_var)
    net.eval()
    with torch.no_grad():
        eo = net(feats)
    bufs = {k: v.clone() for k, v in net.state_dict().items()}
    for i, (a, b) in enumerate(zip(eo, O.pafpn(feats, bufs, training=False))):
        assert torch.equal(a, b)
        d[f"eval_out{i}"] = np_(a)
    # the head on the PAFPN's eval outputs
    hp = O.init_head_params(chans, num_classes=nc, seed=43, depthwise=True)
    head = ref.yolo_head.YOLOXHead(num_classes=nc, strides=strides, in_channels=chans, depthwise=True)
    hsd = head.state_dict()
    assert {k for k in hsd if not k.endswith("num_batches_tracked")} == set(hp), sorted(set(hp) ^ {k for k in hsd if not k.endswith("num_batches_tracked")})[:6]
    head.load_state_dict({k: (v if k.endswith("num_batches_tracked") else hp[k]) for k, v in hsd.items()}, strict=True)
    head.eval()
    with torch.no_grad():
        hout, _ = head(tuple(eo))
    mine = O.yolox_head_eval(list(eo), hp, strides)
    assert torch.allclose(mine, hout, atol=1e-5, rtol=1e-5), float((mine - hout).abs().max())
    d.update(head_out=np_(hout), head_seed=np.int64(43), num_classes=np.int64(nc))
    np.savez_compressed(os.path.join(HERE, "depthwise.npz"), **d)
    print("depthwise ok: head oracle max abs diff", float((mine - hout).abs().max()))


def gen_full_stats(ref):
    """F-7: full-size M1 / G1 statistics (tensors too large to commit)."""
    res = {}
    for tag, hw, part, B in (("M1", (384, 640), (6, 10), 4), ("G1", (256, 320), (8, 10), 4)):
        rcfg = RI.backbone_cfg(hw, part)
        ocfg = O.BackboneCfg(in_res_hw=hw, partition_size=part)
        params = O.init_backbone_params(ocfg, seed=0)
        net = ref.sast_rnn.RNNDetector(rcfg)
        load_into(net, params)
        x = O.synthetic_events(B, hw, seed=0, sparsity=0.9)
        with torch.no_grad():
            out, st, P = net(x)
            oo, os_, oP, lists = O.backbone(x, None, params, ocfg, return_lists=True)
        assert oP == P
        ent = {"P": [int(v) for v in P], "param_checksum": param_checksum(params)}
        for k in (1, 2, 3, 4):
            assert torch.equal(oo[k], out[k])
            t = out[k].double()
            ent[f"h{k}"] = {"mean": float(t.mean()), "absmean": float(t.abs().mean()), "maxabs": float(t.abs().max()),
                            "sha256": hashlib.sha256(np_(out[k]).tobytes()).hexdigest()}
        ent["index_sha256"] = [[hashlib.sha256(np_(l[3]).astype(np.int64).tobytes()).hexdigest() for l in ls[0]]
                               for ls in lists]
        ent["M"] = [[int(len(l[0])) for l in ls[0]] for ls in lists]
        ent["sumK"] = [[int(len(l[3])) for l in ls[0]] for ls in lists]
        res[tag] = ent
        print(tag, ent["P"], ent["M"], ent["sumK"])
    with open(os.path.join(HERE, "full_stats.json"), "w") as f:
        json.dump(res, f, indent=1)


# (tag, hw, partition, B, AMP, seed): seeds found by tests/golden/margin_search.py -- the seed with the WIDEST minimum threshold margin
# among 500 (weights init_backbone_params(seed, ls 0.5), events count_events(B, hw, 100 + seed, density 0.1)).  At AMP 2e-2 roughly 35
# decisions of a run lie within 1e-5 of their threshold, so no seed clears 1e-5; the chosen ones clear 1e-6, ten times the
# fp32 rounding noise of the softmax values (~1e-7).
SPARSE_CASES = [("M1", (384, 640), (6, 10), 4, 2e-2, None), ("M1", (384, 640), (6, 10), 4, 1.0, None),
                ("M1", (384, 640), (6, 10), 8, 2e-2, None), ("M1", (384, 640), (6, 10), 8, 1.0, None),
                ("G1", (256, 320), (8, 10), 4, 2e-2, None), ("G1", (256, 320), (8, 10), 4, 1.0, None)]


def sparse_key(tag, B, amp):
    return f"{tag}_B{B}_amp{amp:g}"


def gen_full_sparse(ref, seeds):
    """F-7, sparse: full-size selection of the IMPORTED REFERENCE at kept fractions below 50 % -- sha256 of index_window / asy_index / K
    of every stage and layer, P, the threshold-margin histogram, output and gradient-norm scalars (tensors too large to commit).
    seeds: {sparse_key: seed} from margin_search.py.  Written to full_stats_sparse.json."""
    res = {}
    for tag, hw, part, B, amp, _ in SPARSE_CASES:
        key = sparse_key(tag, B, amp)
        seed = int(seeds[key])
        rcfg = RI.backbone_cfg(hw, part, amp=amp, ls_init=0.5)
        ocfg = O.BackboneCfg(in_res_hw=hw, partition_size=part, amp=amp)
        params = O.init_backbone_params(ocfg, seed=seed, ls_init=0.5)
        net = ref.sast_rnn.RNNDetector(rcfg)
        load_into(net, params)
        x = O.count_events(B, hw, seed=100 + seed, density=0.1)
        out, st, P = net(x)                                   # the reference, with autograd (gradient scalars below)
        loss = sum((out[k] ** 2).mean() for k in (1, 2, 3, 4))
        loss.backward()
        ml = []
        with torch.no_grad():
            oo, os_, oP, lists = O.backbone(x, None, params, ocfg, return_lists=True, margin_log=ml)
        assert oP == [int(p) for p in P]
        for k in (1, 2, 3, 4):
            assert torch.equal(oo[k], out[k].detach()), (key, k)
        L = [(hw[0] >> (2 + s)) * (hw[1] >> (2 + s)) for s in range(4)]
        ent = {"tag": tag, "hw": list(hw), "partition": list(part), "B": B, "amp": amp, "seed": seed, "ls_init": 0.5, "density": 0.1,
               "P": [int(v) for v in P], "kept_fraction": [round(int(p) / (2 * l), 4) for p, l in zip(P, L)],
               "param_checksum": param_checksum(params), "loss": float(loss),
               "margin_min": min(min(m["win_min"], m["tok_min"]) for m in ml),
               "margin_below": {k: sum(m["below"][k] for m in ml) for k in ("1e-7", "1e-6", "1e-5", "1e-4")},
               "decisions": sum(m["decisions"] for m in ml)}
        for nm, idx in (("index_window", 0), ("asy_index", 3), ("K", 4)):
            ent[nm + "_sha256"] = [[hashlib.sha256(np_(l[idx]).astype(np.int64).tobytes()).hexdigest() for l in ls[0]] for ls in lists]
        ent["M"] = [[int(len(l[0])) for l in ls[0]] for ls in lists]
        ent["sumK"] = [[int(len(l[3])) for l in ls[0]] for ls in lists]
        for k in (1, 2, 3, 4):
            t = out[k].detach().double()
            ent[f"h{k}"] = {"absmean": float(t.abs().mean()), "maxabs": float(t.abs().max())}
        named = dict(net.named_parameters())
        ent["grad_norm"] = {k: float(named[k].grad.double().norm()) for k in
                            ("stages.0.att_blocks.0.att.to_scores.weight", "stages.0.att_blocks.0.att.win_attn.qkv.weight",
                             "stages.1.att_blocks.0.att.grid_attn.mlp.net.2.weight", "stages.2.lstm.conv1x1.weight",
                             "stages.3.downsample_cf2cl.conv.weight")}
        res[key] = ent
        print(key, "seed", seed, "P", ent["P"], "kept", ent["kept_fraction"], f"margin_min {ent['margin_min']:.2e}", ent["margin_below"])
    with open(os.path.join(HERE, "full_stats_sparse.json"), "w") as f:
        json.dump(res, f, indent=1)


def gen_lstm_dws(ref):
    """a12 with dws_conv=True (the reference class default, rnn.py:13,24-28): DWSConvLSTM2d of the reference, depth-wise conv on the
    previous hidden state (only_hidden) and on cat(x, h); with a previous state and without one (the zero state is convolved too:
    the depth-wise bias reaches the gates).  Outputs and every gradient of sum(w_h * h1) + sum(w_c * c1)."""
    B, C, H, W = 2, 32, 8, 10
    d = {}
    for mode, only_hidden in (("hidden", True), ("xh", False)):
        cfgp = O.BackboneCfg(in_res_hw=(128, 160), partition_size=(4, 5), embed_dim=C)
        full = O.init_backbone_params(cfgp, seed=71, dws_conv=mode)
        params = {k[len("stages.0.lstm."):]: v for k, v in full.items() if k.startswith("stages.0.lstm.")}
        m = ref.rnn.DWSConvLSTM2d(C, dws_conv=True, dws_conv_only_hidden=only_hidden, dws_conv_kernel_size=3)
        m.load_state_dict({k: v.clone() for k, v in params.items()}, strict=True)
        g = torch.Generator().manual_seed(72)
        x = torch.randn(B, C, H, W, generator=g)
        h0, c0 = torch.randn(B, C, H, W, generator=g) * 0.5, torch.randn(B, C, H, W, generator=g) * 0.5
        wh, wc = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
        for tag, prev in (("prev", True), ("zero", False)):
            xx, hh, cc = x.clone().requires_grad_(True), h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
            m.zero_grad()
            h1, c1 = m(xx, (hh, cc) if prev else None)
            ((h1 * wh).sum() + (c1 * wc).sum()).backward()
            po = {"lstm." + k: v.clone().requires_grad_(True) for k, v in params.items()}
            xo, ho, co = x.clone().requires_grad_(True), h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
            oh, oc = O.conv_lstm(xo, (ho, co) if prev else None, po, "lstm.")
            assert torch.equal(oh, h1) and torch.equal(oc, c1), (mode, tag)
            ((oh * wh).sum() + (oc * wc).sum()).backward()
            for k, v in m.named_parameters():
                assert torch.allclose(po["lstm." + k].grad, v.grad, atol=1e-6, rtol=1e-5), (mode, tag, k)
            pre = f"{mode}_{tag}_"
            d[pre + "h1"], d[pre + "c1"], d[pre + "dx"] = np_(h1), np_(c1), np_(xx.grad)
            if prev:
                d[pre + "dh0"], d[pre + "dc0"] = np_(hh.grad), np_(cc.grad)
            for k, v in m.named_parameters():
                d[pre + "g_" + k] = np_(v.grad)
        d[mode + "_param_checksum"] = np.float64(param_checksum(params))
    d.update(x=np_(x), h0=np_(h0), c0=np_(c0), wh=np_(wh), wc=np_(wc), seed=np.int64(71))
    np.savez_compressed(os.path.join(HERE, "lstm_dws.npz"), **d)
    print("lstm_dws ok")


def gen_lstm_dropout(ref):
    """a12 with cell_update_dropout > 0 (rnn.py:34,64; reference default 0): DWSConvLSTM2d of the reference in training mode under a fixed
    RNG state.  The fixture holds the keep mask the reference drew (recovered from an identical nn.Dropout call under the same RNG state, and
    proven by the oracle reproducing the reference's outputs with it), outputs and every gradient."""
    B, C, H, W, pdrop = 2, 32, 8, 10, 0.3
    cfgp = O.BackboneCfg(in_res_hw=(128, 160), partition_size=(4, 5), embed_dim=C)
    full = O.init_backbone_params(cfgp, seed=81)
    params = {k[len("stages.0.lstm."):]: v for k, v in full.items() if k.startswith("stages.0.lstm.")}
    m = ref.rnn.DWSConvLSTM2d(C, dws_conv=False, cell_update_dropout=pdrop)
    m.load_state_dict({k: v.clone() for k, v in params.items()}, strict=True)
    m.train()
    g = torch.Generator().manual_seed(82)
    x = torch.randn(B, C, H, W, generator=g)
    h0, c0 = torch.randn(B, C, H, W, generator=g) * 0.5, torch.randn(B, C, H, W, generator=g) * 0.5
    wh, wc = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    xx, hh, cc = x.clone().requires_grad_(True), h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    torch.manual_seed(83)
    h1, c1 = m(xx, (hh, cc))
    ((h1 * wh).sum() + (c1 * wc).sum()).backward()
    torch.manual_seed(83)
    mask = torch.nn.functional.dropout(torch.ones(B, C, H, W), pdrop, True)          # keep / (1 - p), NCHW like the reference's cell input
    assert 0.2 < float((mask == 0).float().mean()) < 0.4
    po = {"lstm." + k: v.clone().requires_grad_(True) for k, v in params.items()}
    xo, ho, co = x.clone().requires_grad_(True), h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    torch.manual_seed(83)
    oh, oc = O.conv_lstm(xo, (ho, co), po, "lstm.", cell_update_dropout=pdrop, training=True)
    assert torch.equal(oh, h1) and torch.equal(oc, c1)
    # the recovered mask is the one in use: c1 = f c0 + i tanh(.) mask  <=>  zero mask entries leave c1 = f c0
    ((oh * wh).sum() + (oc * wc).sum()).backward()
    for k, v in m.named_parameters():
        assert torch.allclose(po["lstm." + k].grad, v.grad, atol=1e-6, rtol=1e-5), k
    m.eval()
    with torch.no_grad():
        eh, ec = m(x, (h0, c0))
        oe = O.conv_lstm(x, (h0, c0), {"lstm." + k: v for k, v in params.items()}, "lstm.", cell_update_dropout=pdrop, training=False)
    assert torch.equal(eh, oe[0]) and torch.equal(ec, oe[1])
    d = dict(x=np_(x), h0=np_(h0), c0=np_(c0), wh=np_(wh), wc=np_(wc), mask=np_(mask), p=np.float64(pdrop), seed=np.int64(81),
             rng_seed=np.int64(83), h1=np_(h1), c1=np_(c1), dx=np_(xx.grad), dh0=np_(hh.grad), dc0=np_(cc.grad), eval_h1=np_(eh), eval_c1=np_(ec),
             param_checksum=np.float64(param_checksum(params)))
    for k, v in m.named_parameters():
        d["g_" + k] = np_(v.grad)
    np.savez_compressed(os.path.join(HERE, "lstm_dropout.npz"), **d)
    print("lstm_dropout ok: dropped", float((mask == 0).float().mean()))


def gen_head_eval(ref):
    """YOLOX head, inference path: the oracle restatement against the reference module in eval mode."""
    if ref.yolo_head is None:
        raise RuntimeError("reference yolo_head not importable: " + ref.yolo_head_error)
    chans, nc, strides = (64, 128, 256), 2, (8, 16, 32)
    params = O.init_head_params(chans, num_classes=nc, seed=5)
    head = ref.yolo_head.YOLOXHead(num_classes=nc, strides=strides, in_channels=chans)
    sd = head.state_dict()
    new = {k: (v if k.endswith("num_batches_tracked") else params[k]) for k, v in sd.items()}
    assert set(params) <= set(sd), sorted(set(params) - set(sd))[:5]
    head.load_state_dict(new, strict=True)
    head.eval()
    g = torch.Generator().manual_seed(77)
    feats = [torch.randn(2, c, 16 // (2 ** i), 20 // (2 ** i), generator=g) for i, c in enumerate(chans)]
    with torch.no_grad():
        out, losses = head(tuple(feats))
    assert losses is None
    mine = O.yolox_head_eval(feats, params, strides)
    assert torch.allclose(mine, out, atol=1e-5, rtol=1e-5), float((mine - out).abs().max())
    head.decode_in_inference = False
    with torch.no_grad():
        raw, _ = head(tuple(feats))
    assert torch.allclose(O.yolox_head_eval(feats, params, strides, decode=False), raw, atol=1e-5, rtol=1e-5)
    d = {f"in{i}": np_(f) for i, f in enumerate(feats)}
    d.update(out=np_(out), raw=np_(raw), num_classes=np.int64(nc), seed=np.int64(5), max_abs_diff_oracle=np.float64(float((mine - out).abs().max())))
    np.savez_compressed(os.path.join(HERE, "head_eval.npz"), **d)
    print("head_eval ok:", tuple(out.shape), "oracle max abs diff", float((mine - out).abs().max()))


def gen_masked_backbone(ref):
    """enable_masking (mask_token write, sast_rnn.py:271-273): oracle vs the reference backbone with a token mask."""
    hw, part, E = (128, 160), (4, 5), 32
    cfg = RI.backbone_cfg(hw, part, embed_dim=E, amp=2e-2, ls_init=0.5)
    cfg["enable_masking"] = True
    net = ref.sast_rnn.RNNDetector(cfg)
    ocfg = O.BackboneCfg(in_res_hw=hw, partition_size=part, embed_dim=E, amp=2e-2)
    params = O.init_backbone_params(ocfg, seed=61, ls_init=0.5)
    g = torch.Generator().manual_seed(62)
    params["stages.0.mask_token"] = torch.randn(1, 1, 1, E, generator=g) * 0.02
    load_into(net, params)
    x = O.count_events(2, hw, seed=63, density=0.05)
    mask = torch.rand(2, hw[0] // 4, hw[1] // 4, generator=g) < 0.3
    out, _st, P = net(x, None, mask)
    loss = sum((out[k] ** 2).mean() for k in (1, 2, 3, 4))
    loss.backward()
    po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    oo, _s, Po = O.backbone(x, None, po, ocfg, token_mask=mask)
    for k in (1, 2, 3, 4):
        assert torch.equal(oo[k], out[k]), k
    assert [int(p) for p in Po] == [int(p) for p in P]
    sum((oo[k] ** 2).mean() for k in (1, 2, 3, 4)).backward()
    gm = dict(net.named_parameters())["stages.0.mask_token"].grad
    assert torch.allclose(po["stages.0.mask_token"].grad, gm, atol=1e-8, rtol=1e-4)
    d = dict(x=np_(x), mask=np_(mask).astype(np.uint8), seed=np.int64(61), mask_token=np_(params["stages.0.mask_token"]),
             P=np.array([int(p) for p in P]), g_mask_token=np_(gm), loss=np.float64(float(loss)))
    for k in (1, 2, 3, 4):
        d[f"h{k}"] = np_(out[k])
    np.savez_compressed(os.path.join(HERE, "backbone_masked.npz"), **d)
    print("backbone_masked ok: P", [int(p) for p in P], "masked tokens", int(mask.sum()))


def gen_head_train(ref):
    """YOLOX head, training branch (SimOTA assignment + IoU / BCE losses): oracle restatement against the reference module."""
    chans, nc, strides = (64, 128, 256), 2, (8, 16, 32)
    params = O.init_head_params(chans, num_classes=nc, seed=6)
    head = ref.yolo_head.YOLOXHead(num_classes=nc, strides=strides, in_channels=chans)
    sd = head.state_dict()
    head.load_state_dict({k: (v if k.endswith("num_batches_tracked") else params[k].clone()) for k, v in sd.items()}, strict=True)
    head.train()
    g = torch.Generator().manual_seed(78)
    B = 3
    feats = [torch.randn(B, c, 16 // (2 ** i), 20 // (2 ** i), generator=g).requires_grad_(True) for i, c in enumerate(chans)]
    labels = O.synthetic_labels(B, (128, 160), nc, max_labels=6, seed=4)
    out, losses = head(tuple(feats), labels)
    losses["loss"].backward()
    po = {k: (v.clone().requires_grad_(True) if "running" not in k else v.clone()) for k, v in params.items()}
    fo = [f.detach().clone().requires_grad_(True) for f in feats]
    mine = O.yolox_head_train(fo, labels, po, strides, num_classes=nc)
    for k in ("loss", "iou_loss", "conf_loss", "cls_loss"):
        assert torch.allclose(mine[k], losses[k], atol=1e-6, rtol=1e-6), (k, float(mine[k]), float(losses[k]))
    assert abs(float(mine["num_fg"]) - float(losses["num_fg"])) < 1e-9
    mine["loss"].backward()
    for a, b in zip(fo, feats):
        assert torch.allclose(a.grad, b.grad, atol=1e-7, rtol=1e-4)
    named = dict(head.named_parameters())
    for k, v in named.items():
        assert torch.allclose(po[k].grad, v.grad, atol=1e-7, rtol=1e-4), k
    d = {f"in{i}": np_(f) for i, f in enumerate(feats)}
    d.update({f"din{i}": np_(f.grad) for i, f in enumerate(feats)})
    d.update(labels=np_(labels), num_classes=np.int64(nc), seed=np.int64(6))
    for k in ("loss", "iou_loss", "conf_loss", "cls_loss"):
        d[k] = np.float64(float(losses[k]))
    d["num_fg"] = np.float64(float(losses["num_fg"]))
    for b, (fg, matched, pious) in enumerate(mine["assign"]):
        d[f"fg{b}"] = np_(fg).astype(np.uint8); d[f"matched{b}"] = np_(matched).astype(np.int64); d[f"piou{b}"] = np_(pious)
    for k in ("cls_preds.0.weight", "cls_preds.0.bias", "reg_preds.1.weight", "obj_preds.2.bias", "stems.0.conv.weight", "reg_convs.1.1.bn.weight"):
        d["g_" + k] = np_(named[k].grad)
    import json as _json
    d["grad_norms_json"] = np.array(_json.dumps({k: float(v.grad.double().norm()) for k, v in named.items()}))
    np.savez_compressed(os.path.join(HERE, "head_train.npz"), **d)
    print("head_train ok:", {k: round(float(losses[k]), 6) for k in ("loss", "iou_loss", "conf_loss", "cls_loss", "num_fg")},
          "fg per image", [int(a[0].sum()) for a in mine["assign"]])


def gen_sequence_gather(ref):
    """(f)2: BackboneFeatureSelector / RNNStates of modules/utils/detection.py driven as modules/detection.py:161-171 does."""
    if RI.REF_ROOT not in sys.path:
        sys.path.insert(0, RI.REF_ROOT)
    from modules.utils.detection import BackboneFeatureSelector, RNNStates
    g = torch.Generator().manual_seed(17)
    T, B = 4, 3
    shapes = {1: (8, 6, 10), 2: (16, 3, 5), 3: (32, 2, 3), 4: (64, 1, 2)}       # (C, H, W)
    idx_seq = [[0, 2], [], [1], [2, 0, 1]]
    sel = BackboneFeatureSelector()
    d = {"idx_json": np.array(json.dumps(idx_seq))}
    feats_seq = []
    for t in range(T):
        f = {k: torch.randn(B, *shp, generator=g) for k, shp in shapes.items()}
        feats_seq.append(f)
        for k, v in f.items():
            d[f"f{t}_{k}"] = np_(v)
        if len(idx_seq[t]) > 0:
            sel.add_backbone_features(backbone_features=f, selected_indices=idx_seq[t])
    out = sel.get_batched_backbone_features()
    mine = O.select_backbone_features(feats_seq, idx_seq)
    for k, v in out.items():
        assert torch.equal(v, mine[k])
        d[f"out_{k}"] = np_(v)
    # RNNStates: save + detach, reset of samples {0, 2} by bool tensor and of sample 1 by index list
    st = RNNStates()
    states = [(torch.randn(B, c, h, w, generator=g), torch.randn(B, c, h, w, generator=g)) for c, h, w in shapes.values()]
    for i, (h, c) in enumerate(states):
        d[f"h_{i}"], d[f"c_{i}"] = np_(h), np_(c)
    st.save_states_and_detach(worker_id=0, states=[(h.clone().requires_grad_(True) * 1.0, c.clone()) for h, c in states])
    assert all(not h.requires_grad for h, _ in st.get_states(0))
    st.reset(worker_id=0, indices_or_bool_tensor=torch.tensor([True, False, True]))
    mine = O.rnn_states_reset(states, torch.tensor([True, False, True]))
    for i, (h, c) in enumerate(st.get_states(0)):
        assert torch.equal(h, mine[i][0]) and torch.equal(c, mine[i][1])
        d[f"reset_bool_h_{i}"], d[f"reset_bool_c_{i}"] = np_(h).copy(), np_(c).copy()      # (the next reset works in place)
    st.reset(worker_id=0, indices_or_bool_tensor=[1])
    for i, (h, c) in enumerate(st.get_states(0)):
        d[f"reset_idx_h_{i}"] = np_(h)
        assert float(h.abs().max()) == 0.0
    assert st.get_states(5) is None
    np.savez_compressed(os.path.join(HERE, "sequence_gather.npz"), **d)
    print("sequence_gather ok")


def main():
    ref = RI.import_reference()
    if "--sparse-only" in sys.argv:   # python make_golden.py --sparse-only seeds.json   (seeds.json: output of margin_search.py)
        with open(sys.argv[sys.argv.index("--sparse-only") + 1]) as f:
            gen_full_sparse(ref, json.load(f))
        return
    if "--sequence-only" in sys.argv:
        gen_sequence_gather(ref)
        return
    if "--mask-only" in sys.argv:
        gen_masked_backbone(ref)
        return
    if "--head-only" in sys.argv:
        gen_head_eval(ref)
        gen_head_train(ref)
        return
    if "--lstm-dws-only" in sys.argv:
        gen_lstm_dws(ref)
        return
    if "--nobias-only" in sys.argv:
        gen_block(ref, "block_nobias", 2, 2e-2, bias=False)
        return
    if "--downsample-only" in sys.argv:
        gen_downsample_variants(ref)
        return
    if "--drop-path-only" in sys.argv:
        gen_block_drop_path(ref)
        return
    if "--drop-mlp-only" in sys.argv:
        gen_block_drop_path(ref, "block_drop_mlp", pdrop=0.0, pmlp=0.2)
        return
    if "--drop-cb-only" in sys.argv:
        gen_block_drop_path(ref, "block_drop_path_cb", pdrop=0.25, pmlp=0.2, enable_cb=True)
        return
    if "--lstm-dropout-only" in sys.argv:
        gen_lstm_dropout(ref)
        return
    if "--depthwise-only" in sys.argv:
        gen_depthwise(ref)
        return
    if "--acts-only" in sys.argv:    # the gate activations beside gelu (B=1, C=32: small fixtures)
        gen_acts(ref)
        return
    if "--prelu-only" in sys.argv:
        gen_acts(ref, ("prelu",))
        return
    if "--acts-r5-only" in sys.argv:
        gen_acts(ref, ACTS_R5)
        return
    if "--dim-heads-only" in sys.argv:
        gen_dim_heads(ref)
        return
    if "--big-partitions-only" in sys.argv:
        gen_big_partitions(ref)
        return
    if "--sizes-only" in sys.argv:   # the two fixtures added for the reference's other model sizes (small: dim_head 24, large: C=96)
        gen_block(ref, "block_small_dh24", 2, 2e-2, C=48, dim_head=24)
        gen_block(ref, "block_large_c96", 2, 2e-2, C=96)
        return
    if "--live-only" in sys.argv:
        gen_backbone_live(ref)
        return
    gen_nzr(ref)
    gen_block(ref, "block_amp2e-4", 2, 2e-4)
    gen_block(ref, "block_amp2e-2", 2, 2e-2)
    gen_block(ref, "block_amp1", 2, 1.0)
    gen_block(ref, "block_b1", 1, 2e-2)
    gen_block(ref, "block_cb", 2, 2e-2, enable_cb=True)
    gen_block(ref, "block_small_dh24", 2, 2e-2, C=48, dim_head=24)
    gen_block(ref, "block_large_c96", 2, 2e-2, C=96)
    gen_block(ref, "block_nobias", 2, 2e-2, bias=False)
    gen_acts(ref)
    gen_dim_heads(ref)
    gen_big_partitions(ref)
    gen_block_drop_path(ref)
    gen_block_drop_path(ref, "block_drop_mlp", pdrop=0.0, pmlp=0.2)
    gen_block_drop_path(ref, "block_drop_path_cb", pdrop=0.25, pmlp=0.2, enable_cb=True)
    gen_downsample_variants(ref)
    gen_two_blocks(ref)
    gen_backbone_tiny(ref)
    gen_backbone_live(ref)
    gen_pafpn(ref)
    gen_depthwise(ref)
    gen_head_eval(ref)
    gen_head_train(ref)
    gen_masked_backbone(ref)
    gen_full_stats(ref)
    gen_lstm_dws(ref)
    gen_lstm_dropout(ref)
    gen_sequence_gather(ref)


if __name__ == "__main__":
    main()
