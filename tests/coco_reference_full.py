"""A plain-loop numpy fp64 restatement of ALL of pycocotools' COCOeval.accumulate and summarize for boxes at maxDets [1, 10, 100]:
the precision, recall and score tables of COCOeval.eval and the twelve numbers of COCOeval.stats.  tests/coco_reference.py keeps the
maxDets-100 precision table and the six numbers the reference reads; this file takes evaluate_img, the thresholds and the area ranges
from it, so there is one matching.

It is the yardstick of tests/test_evaluation_summary.py.  pycocotools is not a dependency of this project: parity of this file with
pycocotools is NOT pinned by a test, it is pinned by the hand-derivable cases of tests/test_coco_reference_full.py and by its
maxDets-100 precision slice being coco_reference.precision_table bit for bit.

The rules (cocoeval.py, accumulate): per (category, area range, maxDet m) the images' evaluations are cut to their first m detections
and concatenated, sorted by a stable descending sort on the score; tp / fp are cumulative counts over the detections that are not
ignored; recall[t, k, a, m] is the last cumulative tp / npig (0 without a detection); precision is made monotone from the right, and for
every recall threshold np.searchsorted(rc, thr, side='left') picks the detection whose precision and score are stored -- nothing
(zeros) from the first threshold on that no recall reaches.  Entries are -1 where a category has neither labels nor detections or no
label that is not ignored.  Input as in coco_reference.py."""
import numpy as np

from coco_reference import AREA_RNG, IOU_THRS, REC_THRS, evaluate_img

MAX_DETS = (1, 10, 100)
STAT_KEYS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L', 'AR_1', 'AR_10', 'AR_100', 'AR_S', 'AR_M', 'AR_L')
CLASS_KEYS = ('AP', 'AP_50', 'AP_75', 'AR_100')


def accumulate(n_images, gt, dt, K):
    """-> dict(precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M]), fp64: COCOeval.eval's tables"""
    gts, dts = {}, {}
    for i in range(len(gt['image_id'])):
        gts.setdefault((int(gt['image_id'][i]), int(gt['category_id'][i])), []).append(
            {'bbox': gt['bbox'][i], 'area': float(gt['area'][i])})
    for i in range(len(dt['image_id'])):
        dts.setdefault((int(dt['image_id'][i]), int(dt['category_id'][i])), []).append(
            {'bbox': dt['bbox'][i], 'area': float(dt['area'][i]), 'score': float(dt['score'][i])})
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        for a, a_rng in enumerate(AREA_RNG):
            E = [evaluate_img(gts.get((img, k + 1), []), dts.get((img, k + 1), []), a_rng) for img in range(1, n_images + 1)]
            E = [e for e in E if e is not None]
            if len(E) == 0:
                continue
            npig = sum(e[3] for e in E)
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                sc = np.concatenate([np.asarray(e[0][:max_det], dtype=np.float64) for e in E])
                inds = np.argsort(-sc, kind='mergesort')
                sc = sc[inds]
                dtm = np.concatenate([e[1][:, :max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e[2][:, :max_det] for e in E], axis=1)[:, inds]
                nd = len(sc)
                for t in range(T):
                    tp, fp = 0, 0
                    rc, pr = [], []
                    for j in range(nd):
                        if not dt_ig[t, j]:
                            tp += int(dtm[t, j])
                            fp += int(not dtm[t, j])
                        rc.append(float(tp) / npig)
                        pr.append(float(tp) / (float(fp) + float(tp) + np.spacing(1)))
                    recall[t, k, a, m] = rc[-1] if nd else 0.0
                    for j in range(nd - 1, 0, -1):
                        if pr[j] > pr[j - 1]:
                            pr[j - 1] = pr[j]
                    q, ss = np.zeros(R), np.zeros(R)
                    pos = np.searchsorted(np.asarray(rc, dtype=np.float64), REC_THRS, side='left')
                    for ri, pi in enumerate(pos):
                        if pi >= nd:        # the IndexError that ends cocoeval.py's loop: this and every later threshold stay 0
                            break
                        q[ri] = pr[pi]
                        ss[ri] = sc[pi]
                    precision[t, :, k, a, m] = q
                    scores[t, :, k, a, m] = ss
    return {'precision': precision, 'recall': recall, 'scores': scores}


def _mean(s):
    s = s[s > -1]
    return -1.0 if s.size == 0 else float(np.mean(s))


def summarize(tables):
    """COCOeval.stats, in its order"""
    p, r = tables['precision'], tables['recall']
    v = [_mean(p[:, :, :, 0, 2]), _mean(p[0, :, :, 0, 2]), _mean(p[5, :, :, 0, 2]), _mean(p[:, :, :, 1, 2]), _mean(p[:, :, :, 2, 2]),
         _mean(p[:, :, :, 3, 2]), _mean(r[:, :, 0, 0]), _mean(r[:, :, 0, 1]), _mean(r[:, :, 0, 2]), _mean(r[:, :, 1, 2]),
         _mean(r[:, :, 2, 2]), _mean(r[:, :, 3, 2])]
    return dict(zip(STAT_KEYS, v))


def per_class(tables, names):
    """per category, over all areas at maxDets 100: AP, AP_50, AP_75 and AR_100 of that category alone"""
    p, r = tables['precision'], tables['recall']
    return {n: {'AP': _mean(p[:, :, k, 0, 2]), 'AP_50': _mean(p[0, :, k, 0, 2]), 'AP_75': _mean(p[5, :, k, 0, 2]),
                'AR_100': _mean(r[:, k, 0, 2])} for k, n in enumerate(names)}


def evaluate(n_images, gt, dt, K):
    """-> (stats, tables or None): twelve zeros when there is no detection at all (coco_eval.py:112-115)"""
    if len(dt['image_id']) == 0:
        return {k: 0.0 for k in STAT_KEYS}, None
    tables = accumulate(n_images, gt, dt, K)
    return summarize(tables), tables
