"""The case tables of the YOLOX head sweep (tests/test_head_operators.py), the inputs of every case and its CPU reference.

Shared by the GPU test, by the bounds generator (tests/operator_sweep.py: every case in float32 against float64 on the CPU) and by
tests/test_head_reference.py.  CPU only: nothing here imports the library.

A case is a dict with an "id" and an "op" (the family its error statistics are pooled over).  `make_inputs(case)` -> fp32 CPU tensors
from a generator seeded by the id and the case's "seed".  `reference(case, inputs, dtype)` -> {quantity: tensor} (float quantities) and,
under "exact:", the discrete results.  Quantity names: "out:<name>" is compared absolutely (sigmoid and raw columns, matched_iou);
"rel:<name>" (decoded box columns, losses) and "grad:<name>" relative to the reference tensor's max-norm.

Families:
  pred   one level (B, H, W, hid) cut out of a three-level buffer (six anchors of another level in front, two behind): forward in the
         case's mode (both outputs / train only / pred only, decoded or raw) and the backward on a random draw with the weight and bias
         gradients accumulated into non-zero buffers.  Rows of the other levels are NaN before and must be NaN afterwards.
  loss   sast_yolox_loss on a synthetic `train` tensor and labels.  Base: levels (5, 7, 8), (3, 4, 16), (2, 2, 32) -> A = 51, B = 3, G = 4;
         image 0 has all G rows in use, image 1 two, image 2 none.  Predictions are jittered copies of the image's ground truths at some
         anchors and boxes around the anchor elsewhere.  The variants are described at `LOSS_CASES`.
  e2e    SF.head_pred_loss: the prediction convs of all levels, the loss, and the backward through 3 * losses[0] into features and
         parameters that carry a gradient already; pred with decode on and off.
  nms    SF.postprocess on B = 3 images (the last one below the confidence threshold), scores on multiples of 1/16.

Every discrete outcome must be decided with a margin the reference itself shows (`check_conditions`); the seeds are those for which
that holds.  Tie cases hold bit-identical values by construction: there the reference's tie rule decides, in every precision.
"""
import math
import re
import zlib

import numpy as np
import torch

import head_reference as R

BASE_LEVELS = ((5, 7, 8.0), (3, 4, 16.0), (2, 2, 32.0))
COST_GAP, DYNK_GAP, CENTRE_GAP, L1_GAP, NMS_IOU_GAP, NMS_SCORE_GAP = 1e-3, 1e-3, 1e-3, 1e-3, 1e-5, 1e-6


def pool_key(quantity):
    """the levels of an e2e case pool their figures: L0.w_reg, L1.w_reg -> L.w_reg"""
    return re.sub(r"L\d\.", "L.", quantity)


# ------------------------------------------------------------------------------------------------ the tables
HIDS = (4, 48, 64, 96, 128, 256, 320, 512)
NCS = (1, 2, 3, 4, 11, 12, 32)
PRED_SHAPES = ((1, 1, 1), (3, 3, 7), (1, 8, 8), (1, 5, 13), (2, 5, 7))
PRED_MODES = ("both-dec", "both-raw", "train", "pred-dec", "pred-raw")


def _pred(hid, nc, bhw, mode):
    B, H, W = bhw
    return dict(id=f"pred-h{hid}-nc{nc}-{B}x{H}x{W}-{mode}", op="pred", hid=hid, nc=nc, B=B, H=H, W=W, mode=mode, stride=16.0, seed=0)


PRED_CASES = [_pred(hid, NCS[(3 * hi + 2 * j) % 7], PRED_SHAPES[(hi + j) % 5], PRED_MODES[(hi + 2 * j) % 5]) for hi, hid in enumerate(HIDS) for j in range(4)]


def _loss(variant, nc=3, levels=BASE_LEVELS, B=3, G=4, nlab=(4, 2, 0), use_l1=False, ties=False, seed=0):
    return dict(id=f"loss-{variant}-nc{nc}", op="loss", variant=variant, nc=nc, levels=tuple(levels), B=B, G=G, nlab=tuple(nlab), use_l1=use_l1,
                ties=ties, seed=seed)


LOSS_CASES = [
    _loss("base", nc=1), _loss("base", nc=2), _loss("base", nc=3), _loss("base", nc=32),
    _loss("single", levels=BASE_LEVELS[:1]),
    _loss("four", levels=BASE_LEVELS + ((1, 1, 64.0),)),
    _loss("nolabels", nlab=(0, 0, 0)),                  # num_fg = 0: only the objectness loss and its gradient remain
    _loss("coincident", ties=True),                     # a prediction bit-equal to its ground truth: every edge ties, 0.5 sub-gradients
    _loss("disjoint", nlab=(1, 2, 0)),                                  # the cheapest anchor of a ground truth does not overlap it: en = 0, loss 1, no box gradient
    _loss("resolve"),                                   # two ground truths contend for the same anchors
    _loss("dupgt", ties=True),                          # two bit-identical label rows: every pick is contested, the lower row wins
    _loss("tie-k1", ties=True, nlab=(4, 1, 0)),                         # bit-identical predictions at two anchors, k = 1: the lower anchor wins
    _loss("few", levels=(BASE_LEVELS[0], BASE_LEVELS[2]), nlab=(4, 1, 0)),   # 8 candidate anchors: the selection round for k ends early
    _loss("k1"), _loss("k10", ties=True, nlab=(4, 1, 0), levels=(BASE_LEVELS[0], BASE_LEVELS[0], BASE_LEVELS[2])),
    _loss("saturated", nc=2),                           # logits of +-200: the -100 clamp of the logs
    _loss("l1", use_l1=True), _loss("l1", nc=2, use_l1=True),
    _loss("a1030", levels=((10, 103, 8.0),), B=2, nlab=(4, 1)),        # register slot j = 1 of the match kernel holds 6 anchors
    _loss("a8192", levels=((64, 128, 8.0),), B=1, G=2, nlab=(2,)),     # the cap: all eight register slots full
    # bit-identical predictions at anchors 3 and 1027, which one thread of the matcher holds in its slots 0 and 1: both IoUs are among the
    # ten largest of ground truth 0, and k = 2 only if the selection round visits both
    _loss("tie-slots", levels=((10, 103, 8.0),), B=1, G=2, nlab=(2,)),
    # the same for the cost round: two levels of the same 32 x 32 grid, so anchors 400 and 1424 are one cell, both inside the centre
    # region; bit-identical predictions, k = 1: the lower anchor wins
    _loss("tie-slots-cost", levels=((32, 32, 8.0), (32, 32, 8.0)), B=1, G=1, nlab=(1,), ties=True),
]


def _e2e(hid, nc, levels, B=2, G=3, nlab=(3, 1), use_l1=False):
    tag = "x".join(f"{h}.{w}" for h, w, _ in levels)
    return dict(id=f"e2e-h{hid}-nc{nc}-{tag}" + ("-l1" if use_l1 else ""), op="e2e", hid=hid, nc=nc, levels=tuple(levels), B=B, G=G, nlab=tuple(nlab),
                use_l1=use_l1, ties=False, variant="e2e", seed=0)


E2E_CASES = [_e2e(64, 2, BASE_LEVELS), _e2e(96, 3, BASE_LEVELS, use_l1=True), _e2e(64, 3, ((6, 10, 8.0), (3, 5, 16.0))),
             _e2e(96, 2, ((9, 8, 8.0), (4, 4, 16.0), (2, 2, 32.0)), B=3, nlab=(3, 2, 0))]


def _nms(A, nc, agnostic, kind="random", counts=None, padded=False, conf=0.25, seed=0):
    return dict(id=f"nms-{kind}-a{A}-nc{nc}" + ("-agn" if agnostic else "") + (f"-n{counts[0]}" if counts else ""), op="nms", A=A, nc=nc,
                agnostic=agnostic, kind=kind, counts=counts, padded=padded, conf=conf, thr=0.45, B=3, seed=seed)


NMS_CASES = [
    _nms(1, 1, False), _nms(63, 3, False), _nms(64, 3, True, counts=(64, 20)), _nms(65, 3, False, counts=(65, 64), padded=True),
    _nms(100, 3, False), _nms(100, 1, True), _nms(100, 3, False, kind="disjoint"), _nms(100, 3, False, kind="identical"),
    _nms(100, 3, True, kind="identical"),
    _nms(1000, 3, False, kind="near", counts=(1000, 37)), _nms(1001, 3, False, kind="near", counts=(1001, 1000)),
    _nms(1250, 3, False, kind="near", counts=(1250, 1001), padded=True), _nms(1250, 3, True),
    _nms(8192, 3, False, counts=(8192, 4097)), _nms(8192, 1, True, counts=(4200, 8192)),
]

ALL_CASES = PRED_CASES + LOSS_CASES + E2E_CASES + NMS_CASES
FLOAT_CASES = PRED_CASES + LOSS_CASES + E2E_CASES          # the cases with float quantities: they have an entry in the bounds file
BOUNDS_CASES = FLOAT_CASES
BY_ID = {c["id"]: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES), "duplicate case ids"


def bounds_id(case):
    return case["id"]


# ------------------------------------------------------------------------------------------------ inputs
def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case["id"].encode()) + case["seed"])


def _u(g, lo, hi, *shape):
    return lo + (hi - lo) * torch.rand(*shape, generator=g)


PRED_PARAMS = ("w_reg", "b_reg", "w_obj", "b_obj", "w_cls", "b_cls")


def pred_layout(case):
    """(anchor offset, anchors in total) of the level inside its three-level buffer"""
    return 6, 6 + case["H"] * case["W"] + 2


def _pred_params(g, hid, nc, prefix=""):
    sc = 0.35 / math.sqrt(hid)         # raw w / h stay inside [-2, 2] (asserted)
    p = {"w_reg": torch.randn(4, hid, generator=g) * sc, "b_reg": _u(g, -0.3, 0.3, 4), "w_obj": torch.randn(1, hid, generator=g) * 3 * sc,
         "b_obj": _u(g, -0.3, 0.3, 1), "w_cls": torch.randn(nc, hid, generator=g) * 3 * sc, "b_cls": _u(g, -0.3, 0.3, nc)}
    return {prefix + k: v for k, v in p.items()}


def _labels(g, B, G, nc, nlab, img_w, img_h):
    lab = torch.zeros(B, G, 5)
    for b in range(B):
        for i in range(nlab[b]):
            w, h = float(_u(g, 0.2, 0.5, 1)) * img_w, float(_u(g, 0.2, 0.5, 1)) * img_h
            lab[b, i] = torch.tensor([float(torch.randint(0, nc, (1,), generator=g)), float(_u(g, 0.25, 0.75, 1)) * img_w,
                                      float(_u(g, 0.25, 0.75, 1)) * img_h, w, h])
    return lab


def _train_rows(g, lab, nlab, levels, nc, near=0.6, small=False):
    """(B, A, 5 + nc): at a share `near` of the anchors a jittered copy of one of the image's ground truths, a box around the anchor
    elsewhere (`small`: boxes of 0.5 - 1.5 px); Gaussian logits"""
    xs, ys, ss = R.level_grid(levels, torch.float32)
    B, A = lab.shape[0], xs.numel()
    cx, cy = (xs + 0.5 + _u(g, -1, 1, B, A)) * ss, (ys + 0.5 + _u(g, -1, 1, B, A)) * ss
    wh = _u(g, 0.5, 1.5, B, A, 2) if small else ss[None, :, None] * torch.exp(_u(g, -1, 2, B, A, 2))
    box = torch.cat([cx[..., None], cy[..., None], wh], -1)
    for b in range(B):
        if not nlab[b] or small:
            continue
        pick = torch.randint(0, nlab[b], (A,), generator=g)
        gt = lab[b, pick, 1:5]
        jit = torch.cat([gt[:, :2] + _u(g, -0.2, 0.2, A, 2) * gt[:, 2:], gt[:, 2:] * torch.exp(_u(g, -0.4, 0.4, A, 2))], 1)
        box[b] = torch.where((torch.rand(A, generator=g) < near)[:, None], jit, box[b])
    return torch.cat([box, 2 * torch.randn(B, A, 1 + nc, generator=g)], -1)


def _anchor(levels, k, y, x):
    return sum(h * w for h, w, _ in levels[:k]) + y * levels[k][1] + x


def _loss_inputs(case, g):
    levels, B, G, nc, nlab, v = case["levels"], case["B"], case["G"], case["nc"], case["nlab"], case["variant"]
    img_w, img_h = levels[0][1] * levels[0][2], levels[0][0] * levels[0][2]
    lab = _labels(g, B, G, nc, nlab, img_w, img_h)
    train = _train_rows(g, lab, nlab, levels, nc, small=v in ("tie-k1", "k1", "disjoint", "k10", "tie-slots", "tie-slots-cost"))
    if v == "coincident":       # level 0, anchor (y 2, x 3): w = h = stride, so that the decode of the recovered raw outputs is exact
        a = _anchor(levels, 0, 2, 3)
        lab[1, 0] = torch.tensor([1.0, 26.0, 20.0, 8.0, 8.0])
        train[1, a, :4] = lab[1, 0, 1:5]
        train[1, a, 4:] = 3.0           # the cheapest anchor by far
        # image 0, anchor (y 1, x 5): only the left and the top edges coincide, so the 0.5 stays in the result
        a = _anchor(levels, 0, 1, 5)
        lab[0, 0] = torch.tensor([2.0, 43.0, 13.0, 10.0, 10.0])
        train[0, a, :4] = torch.tensor([42.0, 12.0, 8.0, 8.0])
        train[0, a, 4:] = torch.tensor([8.0, -8.0, -8.0, 8.0])        # sure of class 2: the cheapest anchor of that ground truth
    elif v == "disjoint":
        # image 0: one ground truth; every prediction is 0.5 - 1.5 px wide and sits 3 - 4 cells to the right of its anchor, so no candidate
        # overlaps it -- except two, which overlap but whose logit of the ground truth's class is -200 (class cost 100)
        lab[0] = 0
        lab[0, 0] = torch.tensor([1.0, 22.3, 18.9, 4.0, 4.0])
        xs, ys, ss = R.level_grid(levels, torch.float32)
        train[0, :, 0] = (xs + _u(g, 3, 4, xs.numel())) * ss
        for a, dx in ((_anchor(levels, 0, 2, 2), 1.0), (_anchor(levels, 0, 2, 3), -1.5)):
            train[0, a, :4] = torch.tensor([22.3 + dx, 18.9, 4.0, 4.0])
            train[0, a, 5 + 1] = -200.0
    elif v == "resolve":
        lab[0, 1, 1:5] = lab[0, 0, 1:5] * torch.tensor([1.03, 0.98, 1.1, 0.93])
    elif v == "dupgt":
        lab[0, 1] = lab[0, 0]
    elif v == "tie-k1":
        lab[1] = 0
        lab[1, 0] = torch.tensor([0.0, 32.25, 20.5, 10.0, 10.0])
        for x in (3, 4):
            a = _anchor(levels, 0, 2, x)
            train[1, a, :4] = torch.tensor([33.25, 20.5, 8.0, 8.0])
            train[1, a, 4:] = train[1, _anchor(levels, 0, 2, 3), 4:]
    elif v == "tie-slots":
        # w = h = stride and centres on multiples of 1/4: the decode of the recovered raw outputs is exact at both anchors
        lab[0, 0] = torch.tensor([1.0, 30.5, 6.0, 9.0, 8.0])
        lab[0, 1] = torch.tensor([0.0, 806.0, 74.0, 20.0, 12.0])
        sure = torch.tensor([8.0, -8.0, 8.0, -8.0])
        for a in (3, 1027):
            train[0, a] = torch.cat([torch.tensor([30.0, 6.0, 8.0, 8.0]), sure])             # IoU 64 / 72 with ground truth 0
        train[0, 4] = torch.cat([torch.tensor([31.5, 6.0, 10.0, 8.0]), sure])                # IoU 68 / 84
    elif v == "tie-slots-cost":
        lab[0, 0] = torch.tensor([0.0, 132.25, 100.5, 10.0, 10.0])
        for a in (400, 1424):           # cell (y 12, x 16), centre (132, 100)
            train[0, a] = torch.cat([torch.tensor([133.25, 100.5, 8.0, 8.0]), torch.tensor([8.0, 8.0, -8.0, -8.0])])
    elif v == "few":
        lab[1] = 0
        lab[1, 0] = torch.tensor([0.0, 2.0, 2.0, 14.0, 12.0])
        train[1] = _train_rows(g, lab[1:2], (1,), levels, nc)[0]
    elif v == "k10":
        # levels 0 and 1 are the same 5 x 7 grid of stride 8: 18 candidates.  Ten of them predict the ground truth bit for bit (IoU
        # exactly 1, w = h = stride), the other eight predict boxes of about a pixel
        lab[1] = 0
        lab[1, 0] = torch.tensor([2.0, 28.0, 20.0, 8.0, 8.0])
        picks = [_anchor(levels, 0, y, x) for y in (1, 2, 3) for x in (2, 3, 4)] + [_anchor(levels, 1, 2, 3)]
        for i, a in enumerate(picks):
            train[1, a, :4] = lab[1, 0, 1:5]
            train[1, a, 4:] = 1.0 + 0.25 * i
    elif v == "saturated":
        sat = torch.rand(B, train.shape[1], 1 + nc, generator=g)
        train[..., 4:] = torch.where(sat < 0.1, torch.full_like(sat, 200.0), torch.where(sat > 0.9, torch.full_like(sat, -200.0), train[..., 4:]))
    elif v in ("a1030", "a8192"):
        # the last label row of image 0 sits in the bottom right corner; the last anchor predicts it almost exactly
        H, W, s = levels[0]
        lab[0, nlab[0] - 1] = torch.tensor([0.0, (W - 1.4) * s, (H - 0.6) * s, 2.5 * s, 1.5 * s])
        train[0, H * W - 1, :4] = lab[0, nlab[0] - 1, 1:5] * torch.tensor([1.0, 1.0, 1.02, 0.97])
        train[0, H * W - 1, 4:] = 2.0
    return {"train": train.contiguous(), "labels": lab}


NMS_SPECIAL = 17        # a "near" image starts with one far box that sets the class offset to 2^22, then eight pairs of class 1


def _nms_inputs(case, g):
    """continuous clustered boxes up to A = 100; from A = 1000 on a lattice of disjoint 64 px cells with a few integer box shapes per cell,
    so that the IoUs form a small set of rationals none of which is near the threshold, however many pairs there are.
    "near": eight pairs of class 1 whose IoU is 0.4414 as given (second kept) and 0.4545 once the corners are shifted by 2^22, where
    x.25 and x.75 round to the even multiple of 0.5 (second suppressed): the coordinate trick and the per-class form keep different
    sets, each decided by 4e-3"""
    B, A, nc, kind = case["B"], case["A"], case["nc"], case["kind"]
    n = torch.arange(A)
    if kind == "disjoint":                                   # a lattice of 20 x 20 boxes 32 px apart
        cxcy = torch.stack([(n % 40) * 32.0 + 16, (n // 40) * 32.0 + 16], 1).expand(B, A, 2).clone()
        wh = torch.full((B, A, 2), 20.0)
    elif kind == "identical":
        cxcy, wh = torch.full((B, A, 2), 100.0), torch.full((B, A, 2), 40.0)
    elif A >= 1000:
        cell = torch.randint(0, max(1, A // 64), (B, A), generator=g)
        cxcy = torch.stack([(cell % 40) * 64.0 + 32, (cell // 40) * 64.0 + 32], -1) + 4.0 * torch.randint(0, 3, (B, A, 2), generator=g)
        wh = 24.0 + 8.0 * torch.randint(0, 2, (B, A, 2), generator=g)
    else:
        nclu = max(1, A // 12)
        centres = torch.rand(B, nclu, 2, generator=g) * torch.tensor([640.0, 384.0])
        pick = torch.randint(0, nclu, (B, A), generator=g)
        cxcy = torch.gather(centres, 1, pick.unsqueeze(-1).expand(B, A, 2)) + torch.randn(B, A, 2, generator=g) * 6
        wh = 20 + torch.rand(B, A, 2, generator=g) * 60
    # obj and class confidences on multiples of 1/4: scores on multiples of 1/16 with many duplicates, 0.25 = 0.5 x 0.5 among them
    obj = torch.randint(2, 5, (B, A, 1), generator=g) / 4.0
    cls = torch.randint(2, 5, (B, A, nc), generator=g) / 4.0
    pred = torch.cat([cxcy, wh, obj, cls], -1)
    first = 0
    if kind == "near":
        first = NMS_SPECIAL
        pred[:, 0] = torch.tensor([2.0 ** 22 - 11, 5000.0, 20.0, 20.0, 1.0, 1.0, 0.5, 0.5])          # x2 = 2^22 - 1: max coordinate + 1 = 2^22
        for i in range(8):
            y = 6000.0 + 100 * i
            pred[:, 1 + 2 * i] = torch.tensor([110.5, y, 20.0, 20.0, 1.0, 0.5, 1.0, 0.5])            # x1 = 100.5: an odd multiple of 0.5
            pred[:, 2 + 2 * i] = torch.tensor([118.25, y, 20.0, 20.0, 0.75, 0.5, 1.0, 0.5])          # x1 = 108.25, x2 = 128.25
    if A > 1:
        pred[:, first, 4:] = 0.5        # a score of exactly 0.25 = conf_thre: a candidate
    if case["counts"]:      # exactly counts[b] candidates in image b: the others get obj = 1/8 (score <= 1/8 < conf)
        for b, cnt in enumerate(case["counts"]):
            drop = first + 1 + torch.randperm(A - first - 1, generator=g)[: A - cnt]
            pred[b, drop, 4] = 0.125
    pred[2, :, 4] = 0.0     # image 2: nothing above the confidence threshold
    return {"pred": pred}


def make_inputs(case):
    g, op = _gen(case), case["op"]
    if op == "pred":
        B, H, W, hid, nc = case["B"], case["H"], case["W"], case["hid"], case["nc"]
        off, A = pred_layout(case)
        inp = {"reg_feat": torch.randn(B, H, W, hid, generator=g), "cls_feat": torch.randn(B, H, W, hid, generator=g)}
        inp.update(_pred_params(g, hid, nc))
        draw = torch.full((B, A, 5 + nc), float("nan"))
        draw[:, off:off + H * W] = torch.randn(B, H * W, 5 + nc, generator=g) + 0.5
        inp["draw"] = draw
        for k in PRED_PARAMS:          # what the gradient buffers hold before the backward adds to them
            inp["prev." + k] = torch.randn(inp[k].shape, generator=g)
        return inp
    if op == "loss":
        return _loss_inputs(case, g)
    if op == "e2e":
        levels, B, G, nc, hid = case["levels"], case["B"], case["G"], case["nc"], case["hid"]
        inp = {"labels": _labels(g, B, G, nc, case["nlab"], levels[0][1] * levels[0][2], levels[0][0] * levels[0][2])}
        for k, (H, W, _s) in enumerate(levels):
            inp[f"L{k}.reg_feat"], inp[f"L{k}.cls_feat"] = torch.randn(B, H, W, hid, generator=g), torch.randn(B, H, W, hid, generator=g)
            inp.update(_pred_params(g, hid, nc, f"L{k}."))
            for name in PRED_PARAMS:
                inp[f"prev.L{k}.{name}"] = torch.randn(inp[f"L{k}.{name}"].shape, generator=g)
        return inp
    if op == "nms":
        return _nms_inputs(case, g)
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------ reference evaluation
E2E_SCALE = 3.0


def _pred_args(inp, dtype, prefix=""):
    return [inp[prefix + k].to(dtype) for k in ("reg_feat", "cls_feat") + PRED_PARAMS]


def reference(case, inp, dtype):
    op, out = case["op"], {}
    if op == "pred":
        H, W, mode = case["H"], case["W"], case["mode"]
        off, _A = pred_layout(case)
        a = _pred_args(inp, dtype)
        pred, train = R.pred_fwd(*a, H, W, case["stride"], not mode.endswith("raw"))
        if mode.startswith("both") or mode == "train":
            out["rel:train_box"], out["out:train_logit"] = train[..., :4], train[..., 4:]
        if mode != "train":
            out["out:pred_box" if mode.endswith("raw") else "rel:pred_box"], out["out:pred_sig"] = pred[..., :4], pred[..., 4:]
        g = R.pred_bwd(inp["draw"][:, off:off + H * W].to(dtype), a[0], a[1], a[2], a[4], a[6])
        out["grad:reg_feat"], out["grad:cls_feat"] = g[0], g[1]
        for k, v in zip(PRED_PARAMS, g[2:]):
            out["grad:" + k] = inp["prev." + k].to(dtype) + v.reshape(inp[k].shape)
        return out
    if op == "loss":
        r = R.yolox_loss(inp["train"], inp["labels"], case["levels"], case["nc"], case["use_l1"], dtype)
        return {"rel:losses": r["losses"], "grad:draw": r["draw"], "out:matched_iou": r["matched_iou"], "exact:fg": r["fg"],
                "exact:matched_gt": r["matched_gt"], "margins": r["margins"], "raw": r["raw"]}
    if op == "e2e":
        labels = inp["labels"]
        preds, raws, trains, args = [], [], [], []
        for k, (H, W, s) in enumerate(case["levels"]):
            a = _pred_args(inp, dtype, f"L{k}.")
            args.append(a)
            pd, tr = R.pred_fwd(*a, H, W, s, True)
            pr, _ = R.pred_fwd(*a, H, W, s, False)
            preds.append(pd); raws.append(pr); trains.append(tr)
        pred, raw, train = torch.cat(preds, 1), torch.cat(raws, 1), torch.cat(trains, 1)
        r = R.yolox_loss(train, labels, case["levels"], case["nc"], case["use_l1"], dtype, scale=E2E_SCALE)
        out = {"rel:losses": r["losses"], "out:matched_iou": r["matched_iou"], "exact:fg": r["fg"], "exact:matched_gt": r["matched_gt"],
               "margins": r["margins"], "raw": r["raw"], "rel:pred_box_dec": pred[..., :4], "out:pred_box_raw": raw[..., :4], "out:pred_sig": pred[..., 4:]}
        off = 0
        for k, (H, W, _s) in enumerate(case["levels"]):
            a = args[k]
            g = R.pred_bwd(r["draw"][:, off:off + H * W], a[0], a[1], a[2], a[4], a[6])
            out[f"grad:L{k}.reg_feat"], out[f"grad:L{k}.cls_feat"] = g[0], g[1]
            for name, v in zip(PRED_PARAMS, g[2:]):
                out[f"grad:L{k}.{name}"] = inp[f"prev.L{k}.{name}"].to(dtype) + v.reshape(inp[f"L{k}.{name}"].shape)
            off += H * W
        return out
    if op == "nms":
        return R.postprocess(inp["pred"], case["nc"], case["conf"], case["thr"], case["agnostic"], dtype={torch.float32: np.float32, torch.float64: np.float64}[dtype])
    raise KeyError(op)


def float_quantities(ref):
    return sorted(q for q in ref if q.split(":")[0] in ("out", "rel", "grad"))


# ------------------------------------------------------------------------------------------------ conditions the cases are stated under
def check_margins(case, m):
    """the gap conditions on the float64 reference's margins.  Tie cases hold bit-identical costs: those pairs are exempt (and must be
    there), every other gap is held to the same figure"""
    assert m["centre"] >= CENTRE_GAP, f"{case['id']}: an anchor centre lies {m['centre']:.2e} px off the edge of a centre region"
    assert m["cost_gap"] >= COST_GAP, f"{case['id']}: k-th and (k+1)-th cost {m['cost_gap']:.2e} apart"
    assert m["resolve_gap"] >= COST_GAP, f"{case['id']}: best and second-best ground truth of a contested anchor {m['resolve_gap']:.2e} apart"
    assert m["dynk"] >= DYNK_GAP, f"{case['id']}: a top-10 IoU sum lies {m['dynk']:.2e} off an integer"
    if case["use_l1"]:
        assert m["l1"] >= L1_GAP, f"{case['id']}: |raw - target| = {m['l1']:.2e}"
    if not case["ties"]:
        assert m["n_cost_ties"] == 0 and m["n_resolve_ties"] == 0 and m["n_dynk_exact"] == 0, (case["id"], m)


def check_conditions(case, inp, ref=None):
    """the input conditions, asserted on the inputs and on the float64 reference (CPU and GPU test both call it); `ref`: the float64
    reference when the caller has it already"""
    op = case["op"]
    ref = ref if ref is not None else reference(case, inp, torch.float64)
    if op == "pred":
        off, A = pred_layout(case)
        HW = case["H"] * case["W"]
        assert off > 0 and A > off + HW and case["hid"] % 4 == 0
        d = inp["draw"]
        assert bool(torch.isnan(d[:, :off]).all()) and bool(torch.isnan(d[:, off + HW:]).all()) and bool(torch.isfinite(d[:, off:off + HW]).all())
        a = _pred_args(inp, torch.float64)
        raw = R.pred_fwd(*a, case["H"], case["W"], case["stride"], False)[0][..., 2:4]
        assert float(raw.abs().max()) <= 2.0, f"{case['id']}: raw w/h up to {float(raw.abs().max()):.2f}"
        assert all(float(inp["prev." + k].abs().min()) > 0 for k in PRED_PARAMS)
    elif op in ("loss", "e2e"):
        lab = inp["labels"]
        n = (lab.sum(2) > 0).sum(1).tolist()
        assert n == list(case["nlab"]), (case["id"], n)
        for b, k in enumerate(n):       # valid rows first, class ids inside [0, nc), positive sizes
            assert bool((lab[b, k:] == 0).all()) and bool((lab[b, :k, 3:] > 0).all())
            assert bool(((lab[b, :k, 0] >= 0) & (lab[b, :k, 0] < case["nc"]) & (lab[b, :k, 0] == lab[b, :k, 0].round())).all())
        assert sum(h * w for h, w, _ in case["levels"]) <= 8192
        if op == "loss":
            assert bool(torch.isfinite(inp["train"]).all()) and bool((inp["train"][..., 2:4] > 0).all())
        check_margins(case, ref["margins"])
        for b, k in enumerate(n):       # the model reference raises when no anchor lies in any centre region of an image with labels
            assert k == 0 or bool(ref["exact:fg"][b].any()), (case["id"], b)
    elif op == "nms":
        p = inp["pred"]
        assert ref["n_cand"][2] == 0 and ref["det"][2] is None
        if case["counts"]:
            assert tuple(ref["n_cand"][:2]) == tuple(case["counts"]), (case["id"], ref["n_cand"])
        assert ref["margin"] >= NMS_IOU_GAP, f"{case['id']}: an IoU lies {ref['margin']:.2e} off the threshold"
        sc = p[..., 4].double() * p[..., 5:].max(-1).values.double()
        assert bool((sc * 32 == (sc * 32).round()).all()), "scores are multiples of 1/32"
        on = sc == case["conf"]         # the deliberate on-threshold scores (0.5 x 0.5): candidates, exempt from the score condition
        assert bool(on[:2].any()) or case["A"] < 63, f"{case['id']}: no score exactly on conf_thre"
        assert float((sc[~on] - case["conf"]).abs().min()) >= NMS_SCORE_GAP


EXACT = ("exact:fg", "exact:matched_gt")
DISCRETE = EXACT
