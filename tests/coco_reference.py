"""A plain-loop numpy fp64 restatement of pycocotools' COCOeval for boxes (iouType 'bbox', useCats, maxDets [1, 10, 100], of which only
100 is kept): evaluate (computeIoU + evaluateImg), accumulate and the six summaries the reference reads (coco_eval.py:109-133).

It is the yardstick of tests/test_evaluation.py.  pycocotools itself is not a dependency of this project, so parity of this file with
pycocotools is NOT pinned by a test here; it is pinned by the hand-derivable cases of tests/test_coco_reference.py.

Input: the flattened records of the reference's _to_coco_format --
  n_images; gt = dict(image_id [G], category_id [G], bbox [G, 4] (x, y, w, h), area [G]); dt = dict(image_id, category_id, score,
  bbox, area) in result order; image ids 1..n_images, category ids 1..K.  No ground truth is a crowd and none carries 'ignore'.
"""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DET = 100
OUT_KEYS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L')


def iou_xywh(d, g):
    """maskApi.c bbIou without crowds, on doubles"""
    d = [float(v) for v in d]
    g = [float(v) for v in g]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] + g[2] * g[3] - i
    return i / u


def evaluate_img(gt, dt, a_rng):
    """one (image, category, area range): gt / dt lists of dicts -> None or (scores, dtm [T, D] bool, dtIg [T, D] bool, npig)"""
    if len(gt) == 0 and len(dt) == 0:
        return None
    order = np.argsort([-d['score'] for d in dt], kind='mergesort')
    dt = [dt[i] for i in order[:MAX_DET]]
    ious = [[iou_xywh(d['bbox'], g['bbox']) for g in gt] for d in dt]          # gt in its own order: computeIoU
    g_ig_raw = [1 if (g['area'] < a_rng[0] or g['area'] > a_rng[1]) else 0 for g in gt]
    gtind = np.argsort(g_ig_raw, kind='mergesort')
    gt_s = [gt[i] for i in gtind]
    g_ig = [g_ig_raw[i] for i in gtind]
    T, D, G = len(IOU_THRS), len(dt), len(gt_s)
    gtm = np.zeros((T, G), dtype=bool)
    dtm = np.zeros((T, D), dtype=bool)
    dt_ig = np.zeros((T, D), dtype=bool)
    if G > 0 and D > 0:
        for tind, t in enumerate(IOU_THRS):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind]:
                        continue
                    if m > -1 and g_ig[m] == 0 and g_ig[gind] == 1:
                        break
                    v = ious[dind][gtind[gind]]
                    if v < iou:
                        continue
                    iou = v
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = g_ig[m]
                dtm[tind, dind] = True
                gtm[tind, m] = True
    out_of_range = np.array([d['area'] < a_rng[0] or d['area'] > a_rng[1] for d in dt], dtype=bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(~dtm, np.repeat(out_of_range, T, 0)))
    return [d['score'] for d in dt], dtm, dt_ig, sum(1 for v in g_ig if v == 0)


def precision_table(n_images, gt, dt, K):
    """-> precision fp64 [T, R, K, A] at maxDets 100 (COCOeval.eval['precision'][..., -1])"""
    gts, dts = {}, {}
    for i in range(len(gt['image_id'])):
        gts.setdefault((int(gt['image_id'][i]), int(gt['category_id'][i])), []).append(
            {'bbox': gt['bbox'][i], 'area': float(gt['area'][i])})
    for i in range(len(dt['image_id'])):
        dts.setdefault((int(dt['image_id'][i]), int(dt['category_id'][i])), []).append(
            {'bbox': dt['bbox'][i], 'area': float(dt['area'][i]), 'score': float(dt['score'][i])})
    T, R, A = len(IOU_THRS), len(REC_THRS), len(AREA_RNG)
    precision = -np.ones((T, R, K, A))
    for k in range(K):
        for a, a_rng in enumerate(AREA_RNG):
            E = [evaluate_img(gts.get((img, k + 1), []), dts.get((img, k + 1), []), a_rng) for img in range(1, n_images + 1)]
            E = [e for e in E if e is not None]
            if len(E) == 0:
                continue
            scores = np.concatenate([np.asarray(e[0], dtype=np.float64) for e in E])
            inds = np.argsort(-scores, kind='mergesort')
            dtm = np.concatenate([e[1] for e in E], axis=1)[:, inds]
            dt_ig = np.concatenate([e[2] for e in E], axis=1)[:, inds]
            npig = sum(e[3] for e in E)
            if npig == 0:
                continue
            tps = np.logical_and(dtm, np.logical_not(dt_ig))
            fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
            for t in range(T):
                tp, fp = 0, 0
                rc, pr = [], []
                for j in range(tps.shape[1]):
                    tp += int(tps[t, j])
                    fp += int(fps[t, j])
                    rc.append(float(tp) / npig)
                    pr.append(float(tp) / (float(fp) + float(tp) + np.spacing(1)))
                for j in range(len(pr) - 1, 0, -1):
                    if pr[j] > pr[j - 1]:
                        pr[j - 1] = pr[j]
                q = np.zeros(R)
                pos = np.searchsorted(np.asarray(rc, dtype=np.float64), REC_THRS, side='left')
                for ri, pi in enumerate(pos):
                    if pi < len(pr):
                        q[ri] = pr[pi]
                precision[t, :, k, a] = q
    return precision


def summarize(precision):
    """the first six entries of COCOeval.stats (AP, AP_50, AP_75, AP_S, AP_M, AP_L at maxDets 100)"""
    def mean(s):
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    return {
        'AP': mean(precision[:, :, :, 0]), 'AP_50': mean(precision[0, :, :, 0]), 'AP_75': mean(precision[5, :, :, 0]),
        'AP_S': mean(precision[:, :, :, 1]), 'AP_M': mean(precision[:, :, :, 2]), 'AP_L': mean(precision[:, :, :, 3]),
    }


def evaluate(n_images, gt, dt, K):
    """-> (the dict of coco_eval.py:109-133, precision or None): six zeros when there is no detection at all (coco_eval.py:112-115)"""
    if len(dt['image_id']) == 0:
        return {k: 0.0 for k in OUT_KEYS}, None
    p = precision_table(n_images, gt, dt, K)
    return summarize(p), p
