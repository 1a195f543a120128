"""CPU tests of the YOLOX head sweep's references and case tables (tests/head_reference.py, tests/head_cases.py): the references agree with
the oracle (which head_train.npz pins to the model reference), the case tables reach what the sweep is about, every case meets its input
conditions and is decided the same way in float32 and float64, and the committed e32 figures hold the quantities the references give
(tests/test_operator_bounds.py regenerates them)."""
import numpy as np
import pytest
import torch

import head_cases as HC
import head_reference as R
import operator_sweep as SW
from oracle import sast_oracle as O

_CACHE = {}


def evaluated(case):
    """(inputs, float64 reference, float32 reference) of a case, computed once for the whole module and never modified"""
    if case["id"] not in _CACHE:
        inp = HC.make_inputs(case)
        _CACHE[case["id"]] = (inp, HC.reference(case, inp, torch.float64), HC.reference(case, inp, torch.float32))
    return _CACHE[case["id"]]


def case(cid):
    return HC.BY_ID[cid]


_ids = SW.ids


# ------------------------------------------------------------------------------------------------ agreement with the oracle
NO_TIE_LOSS = [c for c in HC.LOSS_CASES if not c["ties"] and c["variant"] not in ("nolabels", "a8192")]


@pytest.mark.parametrize("c", NO_TIE_LOSS, ids=_ids(NO_TIE_LOSS))
def test_assignment_and_iou_loss_match_the_oracle(c):
    """oracle.simota_assign image by image (it sees the candidate anchors only and orders with topk) and oracle._iou_loss"""
    inp = HC.make_inputs(c)
    t, lab = inp["train"].double(), inp["labels"].double()
    xs, ys, ss = R.level_grid(c["levels"], torch.float64)
    for b, G in enumerate(c["nlab"]):
        if not G:
            continue
        args = (lab[b, :G, 1:5], lab[b, :G, 0], t[b, :, :4], t[b, :, 5:], t[b, :, 4:5])
        fg, mg, piou = R.simota_assign(*args, xs, ys, ss, c["nc"])
        ofg, omatched, opiou, _ocls = O.simota_assign(*args, ss, xs, ys, c["nc"])
        assert torch.equal(fg, ofg), b
        assert torch.equal(mg[fg], omatched) and float((piou[fg] - opiou).abs().max()) < 1e-12
        assert float((R.iou_loss(t[b, fg, :4], lab[b, mg[fg], 1:5]) - O._iou_loss(t[b, fg, :4], lab[b, mg[fg], 1:5])).abs().max()) == 0.0


def _towers(feats, p):
    out = []
    for k, x in enumerate(feats):
        x = O.base_conv(x, p, f"stems.{k}.", 1, True)
        cf, rf = x, x
        for i in range(2):
            cf = O.conv_unit(cf, p, f"cls_convs.{k}.{i}.", 1, True)
            rf = O.conv_unit(rf, p, f"reg_convs.{k}.{i}.", 1, True)
        out.append((rf.permute(0, 2, 3, 1), cf.permute(0, 2, 3, 1)))
    return out


@pytest.mark.parametrize("use_l1", [False, True])
def test_losses_assignment_and_gradients_match_oracle_yolox_head_train(use_l1):
    """oracle.yolox_head_train end to end: the towers' output is fed through pred_fwd, yolox_loss and pred_bwd, the feature gradients are
    handed back to the towers: losses, assignment, the gradient of every input map and of every prediction-conv parameter"""
    chans, nc, B, strides = (32, 64, 128), 3, 3, (8, 16, 32)
    hw = ((6, 10), (3, 5), (2, 3))
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn(B, ch, h, w, generator=g, dtype=torch.float64) for ch, (h, w) in zip(chans, hw)]
    labels = O.synthetic_labels(B, (48, 80), nc, max_labels=4, seed=5).double()
    params = {k: v.double() for k, v in O.init_head_params(chans, num_classes=nc, seed=4).items()}
    for k in list(params):      # an untrained head predicts nothing: spread the prediction weights so that the costs and IoUs differ
        if "_preds" in k and k.endswith("weight"):
            params[k] = params[k] + 0.05 * torch.randn(params[k].shape, generator=g, dtype=torch.float64)
    fo = [f.clone().requires_grad_(True) for f in feats]
    po = {k: (v.clone().requires_grad_(True) if "running" not in k else v.clone()) for k, v in params.items()}
    ref = O.yolox_head_train(fo, labels, po, strides=strides, num_classes=nc, use_l1=use_l1)
    ref["loss"].backward()

    fm = [f.clone().requires_grad_(True) for f in feats]
    tw = _towers(fm, params)
    levels = [(h, w, float(s)) for (h, w), s in zip(hw, strides)]
    names = [(f"reg_preds.{k}.weight", f"reg_preds.{k}.bias", f"obj_preds.{k}.weight", f"obj_preds.{k}.bias", f"cls_preds.{k}.weight", f"cls_preds.{k}.bias")
             for k in range(3)]
    trains = [R.pred_fwd(rf.detach(), cf.detach(), *[params[n] for n in names[k]], h, w, s, True)[1] for k, ((rf, cf), (h, w, s)) in enumerate(zip(tw, levels))]
    mine = R.yolox_loss(torch.cat(trains, 1), labels, levels, nc, use_l1, torch.float64)
    assert float((torch.cat(trains, 1) - ref["outputs"].detach()).abs().max()) < 1e-10
    for i, k in enumerate(("loss", "iou_loss", "conf_loss", "cls_loss", "l1_loss", "num_fg")):
        want = float(ref[k].detach() if torch.is_tensor(ref[k]) else ref[k])
        assert abs(float(mine["losses"][i]) - want) < 1e-10 * max(1.0, abs(want)), k
    assert float(ref["l1_loss"].detach()) > 0.1 or not use_l1
    assert int(mine["fg"].sum()) >= 3
    for b, (rfg, rmatched, rpiou) in enumerate(ref["assign"]):
        assert torch.equal(mine["fg"][b], rfg) and torch.equal(mine["matched_gt"][b][rfg], rmatched), b
        assert float((mine["matched_iou"][b][rfg] - rpiou).abs().max() if rfg.any() else 0.0) < 1e-12
    off, outs, grads = 0, [], []
    for k, ((rf, cf), (h, w, _s)) in enumerate(zip(tw, levels)):
        gr = R.pred_bwd(mine["draw"][:, off:off + h * w], rf.detach(), cf.detach(), params[names[k][0]], params[names[k][2]], params[names[k][4]])
        off += h * w
        outs += [rf, cf]
        grads += [gr[0], gr[1]]
        for n, v in zip(names[k], gr[2:]):
            want = po[n].grad
            assert float((v.reshape(want.shape) - want).abs().max()) <= 1e-9 * float(want.abs().max()) + 1e-14, n
    torch.autograd.backward(outs, grads)
    for a, b in zip(fm, fo):
        assert float((a.grad - b.grad).abs().max()) <= 1e-8 * float(b.grad.abs().max()), "input gradient"


def _oracle_rows(pred, nc, conf, thr, agnostic):
    return O.postprocess(pred, nc, conf_thre=conf, nms_thre=thr, class_agnostic=agnostic)


SMALL_NMS = [c for c in HC.NMS_CASES if c["A"] <= 100]


@pytest.mark.parametrize("c", SMALL_NMS, ids=_ids(SMALL_NMS))
def test_postprocess_matches_the_oracle_bit_for_bit(c):
    inp, _r64, r32 = evaluated(c)
    ref = _oracle_rows(inp["pred"], c["nc"], c["conf"], c["thr"], c["agnostic"])
    for b in range(c["B"]):
        assert (ref[b] is None) == (r32["det"][b] is None), b
        if ref[b] is not None:
            assert np.array_equal(ref[b].numpy(), r32["det"][b]), b


def test_postprocess_matches_the_oracle_on_threshold_pairs_and_on_500_boxes():
    """the on-threshold fixture of test_gpu_parity.py (the coordinate trick decides), and up to 500 boxes, which the
    oracle's scalar loop can still do"""
    import test_gpu_parity as GP
    pred = GP._near_threshold_detections()
    ref = O.postprocess(pred, 3, conf_thre=0.5, nms_thre=0.45)
    got = R.postprocess(pred, 3, 0.5, 0.45, False)
    assert np.array_equal(ref[0].numpy(), got["det"][0]) and got["margin"] < 1e-6
    assert len(R.postprocess(pred, 3, 0.5, 0.45, False, form="per_class")["kept"][0]) != len(got["kept"][0])
    near = case("nms-near-a1001-nc3-n1001")
    for n in (100, 500):       # lattice boxes with the eight shifted-corner pairs in front, as far as the oracle's scalar loop is quick
        p = HC.make_inputs(near)["pred"][:1, :n].clone()
        ref = O.postprocess(p, 3, conf_thre=0.25, nms_thre=0.45)
        got = R.postprocess(p, 3, 0.25, 0.45, False)
        assert got["n_cand"][0] == n and np.array_equal(ref[0].numpy(), got["det"][0]), n


# ------------------------------------------------------------------------------------------------ what the case tables cover
def test_pred_cases_cover_the_widths_channel_groups_shapes_and_modes():
    pc = HC.PRED_CASES
    assert {c["hid"] for c in pc} == {4, 48, 64, 96, 128, 256, 320, 512}          # 64 lanes; idle threads (48, 96); no fold; a second kb pass
    assert {5 + c["nc"] for c in pc} == {6, 7, 8, 9, 16, 17, 37}
    assert {(5 + c["nc"] + 7) // 8 for c in pc} == {1, 2, 3, 5}
    assert {c["B"] * c["H"] * c["W"] for c in pc} == {1, 63, 64, 65, 70}           # one pixel, a block short of one, a full one, one over
    assert {c["mode"] for c in pc} == set(HC.PRED_MODES)
    for hid in (4, 48, 96, 256, 320, 512):       # every fold form sees a last pixel block that is not full (the bias column sums)
        assert any(c["hid"] == hid and (c["B"] * c["H"] * c["W"]) % 64 for c in pc), hid
    assert all(c["H"] != c["W"] for c in pc if c["H"] * c["W"] > 1 and (c["H"], c["W"]) != (8, 8)) and any(c["W"] > c["H"] > 1 for c in pc)
    assert all(HC.pred_layout(c)[0] > 0 for c in pc)
    assert any(c["hid"] > 256 and c["hid"] % 256 for c in pc)


def _margins(cid):
    return evaluated(case(cid))[1]["margins"]


def test_loss_cases_reach_the_structure_of_the_match_kernel():
    assert {sum(h * w for h, w, _ in c["levels"]) for c in HC.LOSS_CASES} >= {51, 35, 52, 1030, 8192}
    assert {c["nc"] for c in HC.LOSS_CASES} >= {1, 2, 3, 32}
    assert {len(c["levels"]) for c in HC.LOSS_CASES} == {1, 2, 3, 4}
    fg = evaluated(case("loss-a1030-nc3"))[1]["exact:fg"]
    assert bool(fg[0, 1024:].any()), "no matched anchor in register slot j = 1"
    fg = evaluated(case("loss-a8192-nc3"))[1]["exact:fg"]
    assert bool(fg[0, 7168:].any()), "no matched anchor in the last register slot"
    m = _margins("loss-few-nc3")
    assert min(m["n_cand"]) < 10                                          # the `fewer than 10 candidates` break
    assert 1 in _margins("loss-k1-nc3")["ks"] and 10 in _margins("loss-k10-nc3")["ks"]
    assert _margins("loss-k10-nc3")["n_dynk_exact"] == 1


def test_loss_cases_reach_ties_and_conflicts():
    assert _margins("loss-resolve-nc3")["n_multi"] >= 1 and _margins("loss-resolve-nc3")["n_resolve_ties"] == 0
    m = _margins("loss-dupgt-nc3")
    assert m["n_resolve_ties"] >= 1
    inp, r64, _ = evaluated(case("loss-dupgt-nc3"))
    assert torch.equal(inp["labels"][0, 0], inp["labels"][0, 1]) and not bool((r64["exact:matched_gt"][0] == 1).any())   # the lower row wins
    assert bool((r64["exact:matched_gt"][0] == 0).any())
    c = case("loss-tie-k1-nc3")
    inp, r64, r32 = evaluated(c)
    lo, hi = HC._anchor(c["levels"], 0, 2, 3), HC._anchor(c["levels"], 0, 2, 4)
    assert torch.equal(inp["train"][1, lo], inp["train"][1, hi]) and r64["margins"]["n_cost_ties"] == 1
    for r in (r64, r32):        # k = 1, two anchors with bit-identical cost: the lower one
        assert bool(r["exact:fg"][1, lo]) and not bool(r["exact:fg"][1, hi]) and r["margins"]["ks"][-1] == 1
        xs, ys, ss = R.level_grid(c["levels"], r["raw"].dtype)
        assert float(r["raw"][1, lo, 0] + xs[lo]) == float(r["raw"][1, hi, 0] + xs[hi]) == 33.25 / 8      # the recovered raw outputs decode exactly


def test_tie_in_two_register_slots_of_one_matcher_thread():
    c = case("loss-tie-slots-nc3")
    inp, r64, r32 = evaluated(c)
    assert torch.equal(inp["train"][0, 3], inp["train"][0, 1027]) and 1027 - 3 == 1024
    for r in (r64, r32):        # 64 / 72 twice and 68 / 84: the sum passes 2 only with both; anchor 1027 lies outside the centre region
        assert r["margins"]["ks"][0] == 2 and 64 / 72 + 68 / 84 < 2 < 2 * 64 / 72 + 68 / 84
        assert torch.nonzero(r["exact:matched_gt"][0] == 0)[:, 0].tolist() == [3, 4] and bool(r["exact:fg"][0, 1024:].any())
        xs, _ys, _ss = R.level_grid(c["levels"], r["raw"].dtype)
        assert float(r["raw"][0, 3, 0] + xs[3]) == float(r["raw"][0, 1027, 0] + xs[1027]) == 30.0 / 8


def test_cost_tie_in_two_register_slots_of_one_matcher_thread():
    c = case("loss-tie-slots-cost-nc3")
    inp, r64, r32 = evaluated(c)
    assert torch.equal(inp["train"][0, 400], inp["train"][0, 1424]) and c["levels"][0] == c["levels"][1] and _anchor_cell(c, 1424) == (12, 16)
    for r in (r64, r32):
        assert r["margins"]["ks"] == [1] and r["margins"]["n_cost_ties"] == 1
        assert torch.nonzero(r["exact:fg"][0])[:, 0].tolist() == [400]


def _anchor_cell(c, a):
    H, W, _ = c["levels"][0]
    return divmod(a - H * W, W)


def test_loss_cases_reach_the_branches_of_the_loss_kernel():
    c = case("loss-coincident-nc3")
    inp, r64, r32 = evaluated(c)
    a = HC._anchor(c["levels"], 0, 2, 3)
    n = int(r64["exact:fg"].sum())
    for r in (r64, r32):        # all four edges coincide: IoU exactly 1, and with 0.5 on every edge the box gradient cancels to zero
        assert bool(r["exact:fg"][1, a]) and int(r["exact:matched_gt"][1, a]) == 0 and float(r["out:matched_iou"][1, a]) == 1.0
        assert float(r["grad:draw"][1, a, :4].abs().max()) < 1e-6      # (a `<` in place of the tie rule gives d w = 10 / num_fg here)
    assert 10.0 / n > 0.1
    # left and top edges coincide (mtx = mty = 0.5), right and bottom are the prediction's: I = 64, U = 100, dI/dcx = (1 - 0.5) * 8,
    # d cx = k (dI U + I dI) with k = -2 iou 5 / num_fg / U^2, times the stride
    b = HC._anchor(c["levels"], 0, 1, 5)
    assert bool(r64["exact:fg"][0, b]) and int(r64["exact:matched_gt"][0, b]) == 0 and abs(float(r64["out:matched_iou"][0, b]) - 0.64) < 1e-12
    want = -2.0 * 0.64 * 5.0 / n / 100.0 ** 2 * (4.0 * 100.0 + 64.0 * 4.0) * 8.0
    assert abs(float(r64["grad:draw"][0, b, 0]) - want) < 1e-12 * abs(want) + 1e-15 and abs(float(r64["grad:draw"][0, b, 1]) - want) < 1e-12 * abs(want) + 1e-15
    c = case("loss-disjoint-nc3")
    inp, r64, _ = evaluated(c)
    fa = torch.nonzero(r64["exact:fg"][0])[:, 0]
    assert fa.numel() == 1 and float(r64["out:matched_iou"][0, fa[0]]) == 0.0 and float(r64["grad:draw"][0, fa[0], :4].abs().max()) == 0.0
    assert float(evaluated(c)[1]["margins"]["dynk"]) >= HC.DYNK_GAP          # the two overlapping candidates keep the IoU sum off zero
    inp, r64, _ = evaluated(case("loss-nolabels-nc3"))
    assert int(r64["exact:fg"].sum()) == 0 and float(r64["rel:losses"][1]) == 0.0 and float(r64["rel:losses"][2]) > 0
    assert float(r64["grad:draw"][..., 4].abs().min()) > 0 and float(r64["grad:draw"][..., :4].abs().max()) == 0.0
    base = case("loss-base-nc3")
    assert base["nlab"][0] == base["G"] and 0 in base["nlab"]                # all label rows in use; an image without labels
    inp, r64, _ = evaluated(case("loss-saturated-nc2"))
    assert int((inp["train"][..., 4:].abs() == 200).sum()) > 20 and all(bool(torch.isfinite(r64[q]).all()) for q in ("rel:losses", "grad:draw"))
    assert sum(c["use_l1"] for c in HC.LOSS_CASES) >= 2 and float(evaluated(case("loss-l1-nc3"))[1]["rel:losses"][4]) > 0.1


def test_e2e_cases():
    assert {c["hid"] for c in HC.E2E_CASES} == {64, 96} and {c["nc"] for c in HC.E2E_CASES} == {2, 3}
    assert len({c["levels"] for c in HC.E2E_CASES}) == 3 and HC.E2E_SCALE == 3.0
    for c in HC.E2E_CASES:
        inp, r64, _ = evaluated(c)
        assert int(r64["exact:fg"].sum()) >= 2
        assert all(float(inp[k].abs().min()) > 0 for k in inp if k.startswith("prev."))


def test_nms_cases_reach_the_word_edges_the_size_switch_and_the_tie_order():
    nc = HC.NMS_CASES
    assert {c["A"] for c in nc} == {1, 63, 64, 65, 100, 1000, 1001, 1250, 8192}
    assert {c["nc"] for c in nc} == {1, 3} and {c["agnostic"] for c in nc} == {False, True} and sum(c["padded"] for c in nc) == 2
    counts = {n for c in nc for n in evaluated(c)[1]["n_cand"]}
    assert counts >= {0, 64, 65, 1000, 1001, 4097, 8192}
    for c in nc:
        inp, r64, r32 = evaluated(c)
        p = inp["pred"]
        sc = (p[..., 4] * p[..., 5:].max(-1).values)[:2]
        if c["A"] >= 63:        # duplicated scores: the order among them is the anchor order; a score exactly on conf_thre is a candidate
            assert sc.unique().numel() <= 9 and bool((sc == c["conf"]).any())
            on = torch.nonzero(sc[0] == c["conf"])[:, 0]
            assert r32["n_cand"][0] == int((sc[0] >= c["conf"]).sum()) and on.numel() >= 1
    d = evaluated(case("nms-disjoint-a100-nc3"))[2]
    assert [len(k) for k in d["kept"]] == [100, 100, 0]
    assert [len(k) for k in evaluated(case("nms-identical-a100-nc3"))[2]["kept"]][:2] == [3, 3]          # one per class
    assert [len(k) for k in evaluated(case("nms-identical-a100-nc3-agn"))[2]["kept"]][:2] == [1, 1]
    # equal scores: the kept box of the identical case is the first anchor of its class with the top score
    inp, _, r = evaluated(case("nms-identical-a100-nc3-agn"))
    sc = inp["pred"][0, :, 4] * inp["pred"][0, :, 5:].max(-1).values
    assert int(r["kept"][0][0]) == int(torch.nonzero(sc == sc.max())[0, 0]) and int((sc == sc.max()).sum()) > 1


@pytest.mark.parametrize("cid,image", [("nms-near-a1000-nc3-n1000", 0), ("nms-near-a1001-nc3-n1001", 0), ("nms-near-a1001-nc3-n1001", 1),
                                       ("nms-near-a1250-nc3-n1250", 1)])
def test_coordinate_trick_and_per_class_form_keep_different_sets(cid, image):
    """at 1000 candidates (4000 coordinates) the shifted form decides, at 1001 the per-class form: on these inputs they keep different
    sets, each with the margin of check_conditions, so a kernel that switches at another size fails the exact comparison"""
    c = case(cid)
    inp, _, r32 = evaluated(c)
    forms = {f: R.postprocess(inp["pred"], c["nc"], c["conf"], c["thr"], False, form=f) for f in ("trick", "per_class")}
    n = r32["n_cand"][image]
    assert n in (1000, 1001)
    assert len(forms["trick"]["kept"][image]) + 8 == len(forms["per_class"]["kept"][image])        # the second box of each of the eight pairs
    assert min(forms["trick"]["margin"], forms["per_class"]["margin"]) >= HC.NMS_IOU_GAP
    assert np.array_equal(r32["kept"][image], forms["trick" if n <= 1000 else "per_class"]["kept"][image])


# ------------------------------------------------------------------------------------------------ input conditions, fp32 = fp64
@pytest.mark.parametrize("c", HC.ALL_CASES, ids=_ids(HC.ALL_CASES))
def test_input_conditions_hold_and_float32_decides_like_float64(c):
    inp, r64, r32 = evaluated(c)
    HC.check_conditions(c, inp, r64)
    if c["op"] in ("loss", "e2e"):
        for q in HC.EXACT:
            assert torch.equal(r64[q], r32[q]), q
        assert r64["margins"]["ks"] == r32["margins"]["ks"]
    if c["op"] == "nms":
        assert r64["n_cand"] == r32["n_cand"]
        for a, b in zip(r64["kept"], r32["kept"]):
            assert np.array_equal(a, b)


def test_a_case_without_its_margin_is_refused():
    """check_conditions is a check: ground truths moved so that an anchor centre sits on the edge of a centre region do not pass"""
    c = case("loss-base-nc3")
    inp = {k: v.clone() for k, v in evaluated(c)[0].items()}
    inp["labels"][0, 0, 1] = 4.0 + 12.0          # anchor centre x = 4 is on the left edge of the region of radius 12
    with pytest.raises(AssertionError, match="centre region"):
        HC.check_conditions(c, inp)


# ------------------------------------------------------------------------------------------------ the committed bounds
bounds = SW.bounds_fixture("head")


def test_bounds_hold_every_compared_quantity_and_stay_inside_the_project_bars(bounds):
    for c in HC.FLOAT_CASES:
        entry = bounds["cases"][c["id"]]
        assert set(entry) == set(HC.float_quantities(evaluated(c)[1])), c["id"]
        grads = {"grad:" + k for k in ("reg_feat", "cls_feat") + HC.PRED_PARAMS}
        if c["op"] == "pred":
            fwd = {"both-dec": {"rel:train_box", "out:train_logit", "rel:pred_box", "out:pred_sig"}, "train": {"rel:train_box", "out:train_logit"},
                   "both-raw": {"rel:train_box", "out:train_logit", "out:pred_box", "out:pred_sig"}, "pred-dec": {"rel:pred_box", "out:pred_sig"},
                   "pred-raw": {"out:pred_box", "out:pred_sig"}}[c["mode"]]
            assert set(entry) == fwd | grads, c["id"]
        elif c["op"] == "loss":
            assert set(entry) == {"rel:losses", "grad:draw", "out:matched_iou"}
        else:
            want = {"rel:losses", "out:matched_iou", "rel:pred_box_dec", "out:pred_box_raw", "out:pred_sig"}
            assert set(entry) == want | {q.replace("grad:", f"grad:L{k}.") for q in grads for k in range(len(c["levels"]))}
        for q, e in entry.items():
            v = bounds["operators"][c["op"]][HC.pool_key(q)]
            assert 0.0 <= e <= v["worst"] < SW.project_bar(q) / 2, (c["id"], q, e)
    for op, qs in bounds["operators"].items():
        for q, v in qs.items():
            assert 0.0 < v["median"] <= v["worst"] and v["n"] >= 4, (op, q, v)
