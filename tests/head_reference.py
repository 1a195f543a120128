"""Plain CPU references of the YOLOX head family (csrc/k_head.hip), parametrised by dtype: the prediction convs with their decode, forward
and backward; the SimOTA assignment with the training losses and their gradient; the confidence filter with greedy NMS.

Nothing here imports the library.  tests/test_head_reference.py ties these functions to oracle/sast_oracle.py (which head_train.npz pins to
the model reference); tests/test_head_operators.py compares the kernels with them in float64.

The assignment is written out so that the tie rule k_head.hip documents is part of the reference: both selection rounds order the anchors
by (value, anchor index), and an anchor picked by several ground truths goes to the FIRST ground truth with the smallest cost.
`torch.topk`, which the oracle uses, leaves the order among equal values undefined.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def level_grid(levels, dtype):
    """(xs, ys, strides), one entry per anchor, levels concatenated: levels = [(H, W, stride)]"""
    xs, ys, ss = [], [], []
    for H, W, s in levels:
        yv, xv = torch.meshgrid([torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype)], indexing="ij")
        xs.append(xv.reshape(-1)); ys.append(yv.reshape(-1)); ss.append(torch.full((H * W,), float(s), dtype=dtype))
    return torch.cat(xs), torch.cat(ys), torch.cat(ss)


# ------------------------------------------------------------------------------------------------ prediction convs
def pred_fwd(reg_feat, cls_feat, w_reg, b_reg, w_obj, b_obj, w_cls, b_cls, H, W, stride, decode):
    """one level.  feats (B, H, W, hid); w_reg (4, hid), w_obj (1, hid), w_cls (nc, hid) -> (pred, train), each (B, H*W, 5 + nc):
    train = decoded box, raw obj / cls logits; pred = box (decoded, or raw when not decode), sigmoid(obj), sigmoid(cls)"""
    B, hid = reg_feat.shape[0], reg_feat.shape[-1]
    rf, cf = reg_feat.reshape(B, H * W, hid), cls_feat.reshape(B, H * W, hid)
    reg = rf @ w_reg.reshape(4, hid).t() + b_reg
    obj = rf @ w_obj.reshape(1, hid).t() + b_obj
    cls = cf @ w_cls.reshape(-1, hid).t() + b_cls
    xs, ys, _ = level_grid([(H, W, stride)], reg.dtype)
    box = torch.cat([(reg[..., 0:1] + xs[None, :, None]) * stride, (reg[..., 1:2] + ys[None, :, None]) * stride, torch.exp(reg[..., 2:4]) * stride], -1)
    train = torch.cat([box, obj, cls], -1)
    pred = torch.cat([box if decode else reg, torch.sigmoid(obj), torch.sigmoid(cls)], -1)
    return pred, train


def pred_bwd(draw, reg_feat, cls_feat, w_reg, w_obj, w_cls):
    """draw (B, H*W, 5 + nc) = d loss / d raw conv output of the level -> d reg_feat, d cls_feat, dw_reg, db_reg, dw_obj, db_obj, dw_cls,
    db_cls (weights flat [out, hid]); matmuls, no autograd"""
    hid = reg_feat.shape[-1]
    d = draw.reshape(-1, draw.shape[-1])
    rf, cf = reg_feat.reshape(-1, hid), cls_feat.reshape(-1, hid)
    wr, wo, wc = w_reg.reshape(4, hid), w_obj.reshape(1, hid), w_cls.reshape(-1, hid)
    d_rf = d[:, 0:4] @ wr + d[:, 4:5] @ wo
    d_cf = d[:, 5:] @ wc
    return (d_rf.reshape(reg_feat.shape), d_cf.reshape(cls_feat.shape), d[:, 0:4].t() @ rf, d[:, 0:4].sum(0), d[:, 4:5].t() @ rf, d[:, 4:5].sum(0),
            d[:, 5:].t() @ cf, d[:, 5:].sum(0))


# ------------------------------------------------------------------------------------------------ SimOTA + losses
def pairwise_iou(gt, boxes):
    """yolox/utils/boxes.py bboxes_iou with xyxy=False: gt (G, 4), boxes (A, 4) in (cx, cy, w, h) -> (G, A)"""
    tl = torch.max(gt[:, None, :2] - gt[:, None, 2:] / 2, boxes[:, :2] - boxes[:, 2:] / 2)
    br = torch.min(gt[:, None, :2] + gt[:, None, 2:] / 2, boxes[:, :2] + boxes[:, 2:] / 2)
    en = ((tl < br).to(gt.dtype)).prod(2)
    ai = (br - tl).prod(2) * en
    return ai / ((gt[:, 2] * gt[:, 3])[:, None] + boxes[:, 2] * boxes[:, 3] - ai)


def iou_loss(pred, target):
    """IOUloss("iou"), reduction none: 1 - iou^2"""
    tl = torch.max(pred[:, :2] - pred[:, 2:] / 2, target[:, :2] - target[:, 2:] / 2)
    br = torch.min(pred[:, :2] + pred[:, 2:] / 2, target[:, :2] + target[:, 2:] / 2)
    en = ((tl < br).to(pred.dtype)).prod(1)
    ai = (br - tl).prod(1) * en
    iou = ai / (pred[:, 2:].prod(1) + target[:, 2:].prod(1) - ai + 1e-16)
    return 1 - iou ** 2


def _ordered(values, descending):
    """anchor positions by (value, position): a stable sort, so equal values keep the lower position first"""
    return torch.sort(values, descending=descending, stable=True).indices


def simota_assign(gt_boxes, gt_classes, boxes, cls_logits, obj_logits, xs, ys, ss, nc, margins=None):
    """get_assignments for one image over ALL A anchors -> fg (A,) bool, matched_gt (A,) long (-1 = background), matched_iou (A,).
    `margins`, when given, collects how far every discrete decision was from going the other way (see head_cases.check_conditions)."""
    G, A = gt_boxes.shape[0], boxes.shape[0]
    xc, yc, dist = (xs + 0.5) * ss, (ys + 0.5) * ss, ss * 1.5
    gx, gy = gt_boxes[:, 0:1], gt_boxes[:, 1:2]
    m = torch.stack([xc - (gx - dist), yc - (gy - dist), (gx + dist) - xc, (gy + dist) - yc], 2).min(-1).values       # (G, A)
    is_in = m > 0
    cand = is_in.any(0)
    ious = pairwise_iou(gt_boxes, boxes)
    p = (torch.sigmoid(cls_logits) * torch.sigmoid(obj_logits)).sqrt()                                                # (A, nc)
    onehot = F.one_hot(gt_classes.to(torch.int64), nc).to(p.dtype)
    cls_cost = F.binary_cross_entropy(p[None].expand(G, A, nc), onehot[:, None].expand(G, A, nc), reduction="none").sum(-1)
    cost = cls_cost + 3.0 * (-torch.log(ious + 1e-8)) + 1e6 * (~is_in).to(p.dtype)
    ci = torch.nonzero(cand)[:, 0]
    matching = torch.zeros(G, A, dtype=torch.bool)
    for g in range(G):
        iv, cv = ious[g, ci], cost[g, ci]
        top = iv[_ordered(iv, True)[:10]]
        s = float(top.sum())
        k = min(max(int(s), 1), ci.numel())
        order = _ordered(cv, False)
        matching[g, ci[order[:k]]] = True
        if margins is not None:
            margins["ks"].append(k)
            margins["n_cand"].append(int(ci.numel()))
            if bool((top == 1.0).all()) and top.numel() == 10:
                margins["n_dynk_exact"] += 1          # ten IoUs of exactly 1: their sum is exact in every precision
            else:
                margins["dynk"] = min(margins["dynk"], abs(s - round(s)))
            if k < ci.numel():
                gap = float(cv[order[k]] - cv[order[k - 1]])
                if gap == 0.0:
                    margins["n_cost_ties"] += 1
                else:
                    margins["cost_gap"] = min(margins["cost_gap"], gap)
    per_anchor = matching.sum(0)
    multi = per_anchor > 1
    if bool(multi.any()):
        cm = cost[:, multi]
        first_min = (cm == cm.min(0).values).to(torch.int64).argmax(0)       # argmax returns the FIRST maximal value
        matching[:, multi] = False
        matching[first_min, torch.nonzero(multi)[:, 0]] = True
        if margins is not None and G > 1:
            two = torch.sort(cm, dim=0).values[:2]
            gaps = two[1] - two[0]
            margins["n_resolve_ties"] += int((gaps == 0).sum())
            if bool((gaps > 0).any()):
                margins["resolve_gap"] = min(margins["resolve_gap"], float(gaps[gaps > 0].min()))
    if margins is not None:
        margins["n_multi"] += int(multi.sum())
        margins["centre"] = min(margins["centre"], float(m.abs().min()))
    fg = per_anchor > 0
    mg = torch.where(fg, matching.to(torch.int64).argmax(0), torch.full((A,), -1, dtype=torch.int64))
    piou = torch.where(fg, (matching.to(ious.dtype) * ious).sum(0), torch.zeros(A, dtype=ious.dtype))
    return fg, mg, piou


def new_margins():
    inf = math.inf
    return {"ks": [], "n_cand": [], "dynk": inf, "n_dynk_exact": 0, "cost_gap": inf, "n_cost_ties": 0, "resolve_gap": inf, "n_resolve_ties": 0,
            "n_multi": 0, "centre": inf, "l1": inf}


def yolox_loss(train, labels, levels, nc, use_l1, dtype, scale=1.0):
    """train (B, A, 5 + nc) as the prediction kernel writes it (decoded box, raw logits), labels (B, G, 5) = (class, cx, cy, w, h) with the
    valid rows first.  -> dict: losses (6,) = total, 5 * iou, obj, cls, l1, num_fg / max(num_gt, 1); draw (B, A, 5 + nc) = d (scale *
    losses[0]) / d raw conv output; fg (B, A) bool; matched_gt (B, A) long; matched_iou (B, A); margins.
    The raw outputs are recovered from `train` by the inverse decode in `dtype`, made leaves and decoded again."""
    t, labels = train.detach().to(dtype), labels.to(dtype)
    B, A, no = t.shape
    xs, ys, ss = level_grid(levels, dtype)
    assert xs.numel() == A and no == 5 + nc
    raw = torch.cat([t[..., 0:1] / ss[None, :, None] - xs[None, :, None], t[..., 1:2] / ss[None, :, None] - ys[None, :, None],
                     torch.log(t[..., 2:4] / ss[None, :, None]), t[..., 4:]], -1).requires_grad_(True)
    out = torch.cat([(raw[..., 0:1] + xs[None, :, None]) * ss[None, :, None], (raw[..., 1:2] + ys[None, :, None]) * ss[None, :, None],
                     torch.exp(raw[..., 2:4]) * ss[None, :, None], raw[..., 4:]], -1)
    boxes, objp, clsp = out[..., :4], out[..., 4:5], out[..., 5:]
    nlabel = (labels.sum(2) > 0).sum(1)
    margins = new_margins()
    fgs, mgs, pious = [], [], []
    for b in range(B):
        G = int(nlabel[b])
        if G == 0:
            fgs.append(torch.zeros(A, dtype=torch.bool)); mgs.append(torch.full((A,), -1, dtype=torch.int64)); pious.append(torch.zeros(A, dtype=dtype))
            continue
        with torch.no_grad():
            fg, mg, piou = simota_assign(labels[b, :G, 1:5], labels[b, :G, 0], boxes[b], clsp[b], objp[b], xs, ys, ss, nc, margins)
        fgs.append(fg); mgs.append(mg); pious.append(piou)
    fg, mg, piou = torch.stack(fgs), torch.stack(mgs), torch.stack(pious)
    num_fg = max(int(fg.sum()), 1)
    bi, ai = torch.nonzero(fg, as_tuple=True)
    gt = labels[bi, mg[bi, ai]]                                       # (n, 5)
    l_iou = iou_loss(boxes[bi, ai], gt[:, 1:5]).sum() / num_fg
    l_obj = F.binary_cross_entropy_with_logits(objp[..., 0], fg.to(dtype), reduction="none").sum() / num_fg
    cls_t = F.one_hot(gt[:, 0].to(torch.int64), nc).to(dtype) * piou[bi, ai][:, None]
    l_cls = F.binary_cross_entropy_with_logits(clsp[bi, ai], cls_t, reduction="none").sum() / num_fg
    l_l1 = torch.zeros((), dtype=dtype)
    if use_l1 and bi.numel():
        sm = ss[ai]
        tgt = torch.stack([gt[:, 1] / sm - xs[ai], gt[:, 2] / sm - ys[ai], torch.log(gt[:, 3] / sm + 1e-8), torch.log(gt[:, 4] / sm + 1e-8)], 1)
        diff = raw[bi, ai, :4] - tgt
        margins["l1"] = float(diff.detach().abs().min())
        l_l1 = diff.abs().sum() / num_fg
    total = 5.0 * l_iou + l_obj + l_cls + l_l1
    (scale * total).backward()
    losses = torch.stack([total, 5.0 * l_iou, l_obj, l_cls, l_l1, torch.tensor(num_fg / max(int(nlabel.sum()), 1), dtype=dtype)]).detach()
    return {"losses": losses, "draw": raw.grad, "fg": fg, "matched_gt": mg, "matched_iou": piou.detach(), "margins": margins, "raw": raw.detach()}


# ------------------------------------------------------------------------------------------------ confidence filter + NMS
TRICK_MAX_COORDS = 4000       # torchvision 0.15 batched_nms on CPU tensors: the coordinate trick up to here, a per-class evaluation beyond


def _greedy(boxes, order, classes, thr, per_class, dtype):
    """greedy NMS over `order`; every candidate against the whole kept set at once.  The IoU arithmetic runs in `dtype` on the float32
    boxes as given.  -> kept positions (in order of decreasing score), smallest float64 |IoU - thr| over the pairs compared"""
    b = boxes.astype(dtype)
    b64 = boxes.astype(np.float64)
    area, area64 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), (b64[:, 2] - b64[:, 0]) * (b64[:, 3] - b64[:, 1])
    n = len(order)
    kept = np.empty(n, dtype=np.int64)
    thr = np.float32(thr)         # the threshold the kernel is handed
    nk, margin, zero = 0, math.inf, dtype(0)
    for i in order:
        ks = kept[:nk]
        if per_class:
            ks = ks[classes[ks] == classes[i]]
        if ks.size:
            w = np.maximum(np.minimum(b[i, 2], b[ks, 2]) - np.maximum(b[i, 0], b[ks, 0]), zero)
            h = np.maximum(np.minimum(b[i, 3], b[ks, 3]) - np.maximum(b[i, 1], b[ks, 1]), zero)
            inter = w * h
            iou = inter / (area[i] + area[ks] - inter)
            w64 = np.maximum(np.minimum(b64[i, 2], b64[ks, 2]) - np.maximum(b64[i, 0], b64[ks, 0]), 0.0)
            h64 = np.maximum(np.minimum(b64[i, 3], b64[ks, 3]) - np.maximum(b64[i, 1], b64[ks, 1]), 0.0)
            i64 = w64 * h64
            margin = min(margin, float(np.abs(i64 / (area64[i] + area64[ks] - i64) - float(thr)).min()))
            if bool((iou > dtype(thr)).any()):
                continue
        kept[nk] = i
        nk += 1
    return kept[:nk], margin


def postprocess(pred, nc, conf_thre, nms_thre, class_agnostic, dtype=np.float32, form=None):
    """pred (B, A, 5 + nc) float32 -> dict: det = list of (n, 7) float32 arrays (x1, y1, x2, y2, obj, class conf, class) by decreasing
    score (None without detections), kept = list of kept anchor indices, n_cand = candidates per image, margin = smallest float64
    |IoU - nms_thre| over all compared pairs, score_margin = smallest |score - conf_thre|.
    Everything up to the boxes the NMS sees is float32 in the oracle's order of operations (the rounding of the shifted corners is part
    of the result); `dtype` is the precision of the IoU arithmetic only.  `form` forces "trick" or "per_class" (default: by size)."""
    p = pred.detach().cpu().numpy().astype(np.float32)
    one, half = np.float32(1), np.float32(2)
    det, keeps, ncand, margin, smargin = [], [], [], math.inf, math.inf
    for ip in p:
        x1, y1 = ip[:, 0] - ip[:, 2] / half, ip[:, 1] - ip[:, 3] / half
        x2, y2 = ip[:, 0] + ip[:, 2] / half, ip[:, 1] + ip[:, 3] / half
        cc, cp = ip[:, 5:5 + nc].max(1), ip[:, 5:5 + nc].argmax(1)           # argmax: the first maximal class
        score = ip[:, 4] * cc
        smargin = min(smargin, float(np.abs(score.astype(np.float64) - float(np.float32(conf_thre))).min()))
        idx = np.nonzero(score >= np.float32(conf_thre))[0]
        ncand.append(int(idx.size))
        if not idx.size:
            det.append(None); keeps.append(np.empty(0, dtype=np.int64))
            continue
        rows = np.stack([x1, y1, x2, y2, ip[:, 4], cc, cp.astype(np.float32)], 1)[idx]
        boxes, sc, cl = rows[:, :4], score[idx], cp[idx]
        order = np.argsort(-sc, kind="stable")
        use = form or ("agnostic" if class_agnostic else ("trick" if boxes.size <= TRICK_MAX_COORDS else "per_class"))
        if use == "trick":
            off = cl.astype(np.float32) * (boxes.max() + one)
            boxes = boxes + off[:, None]
        k, mg = _greedy(boxes, order, cl, nms_thre, use == "per_class", dtype)
        margin = min(margin, mg)
        det.append(rows[k]); keeps.append(idx[k])
    return {"det": det, "kept": keeps, "n_cand": ncand, "margin": margin, "score_margin": smargin}
