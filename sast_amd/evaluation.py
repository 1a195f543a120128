"""Prophesee mAP evaluation of detections on the GPU (csrc/k_eval.hip).

The reference copies every validation step's labels and detections to the host (to_prophesee, utils/evaluation/prophesee/io/
box_loading.py:58-99), buffers them in PropheseeEvaluator (evaluator.py) and at epoch end runs filter_boxes, _match_times,
_to_coco_format and pycocotools' COCOeval in Python (evaluation.py, metrics/coco_eval.py).  `PropheseeEvaluator` here keeps the buffer
on the device: `add` takes the label tensors `SpatialAugmentor` returns and the padded detections of
`sast_amd.functional.postprocess_padded`, filters, flattens and matches them (COCOeval.evaluate is per image), and
`evaluate_buffer` sorts the per-detection records and computes COCOeval's precision table and the six numbers of coco_eval.py:109.

- `add` enqueues three launches and synchronises nothing: cursors, counts and overflow counters live in device memory, so after one
  eager call it can be captured in a graph together with the detector.
- Each added frame is its own "file" of the reference's _match_times: a frame none of whose labels passes the filter is no image and
  its detections vanish with it; image ids follow the order of `add` calls and of the rows within a call.
- What does not fit `max_images`, `max_detections` (filtered detections over the whole buffer) or `max_labels_per_frame` (filtered
  labels of one frame) is counted on the device and raised by `evaluate_buffer`, never dropped silently; so are `add_recordings`'
  windows over `max_window_detections` and its unsorted rows.
- `merge` appends another evaluator's buffer on the device (one call, no sync), `export_buffer` / `import_buffer` move a buffer as a
  dict of trimmed tensors, and `all_gather` joins the buffers of all ranks of a process group in rank order: every rank then computes
  the numbers of ONE evaluator fed rank 0's frames, then rank 1's, ... -- the dataset's mAP, whatever the number of ranks.  The
  reference averages per-rank metrics instead, which is not the dataset's AP (precision over recall is not linear in the shards).
- `add_recordings` is the protocol's own form: whole recordings as sorted box records, one label "file" against one detection "file"
  per row, every unique label timestamp an image with the detections within +-time_tol_us (_match_times, metrics/coco_eval.py:55-90).
  It feeds the same count, scan and match kernels through a second row source and may be mixed with `add` in one buffer.
- `summary`, `coco_eval` and `per_class` follow an `evaluate_buffer` and give the rest of COCOeval: the twelve numbers of its stats
  (AP and AR at maxDets 1 / 10 / 100, which the reference discards in coco_eval.py:109), the precision, recall and score tables of
  COCOeval.eval at maxDets [1, 10, 100] and the numbers per category.  Every record carries its rank inside its (image, category)
  group, so the cut to an image's first 1 or 10 detections needs no second matching or sort; `scores` is how a `conf_thre` is picked.
- Not implemented: visualisation.  Parity with pycocotools and with the Metavision toolbox is not pinned by a test: neither is
  installed where this project is built (tests/coco_reference.py and tests/coco_reference_full.py are the yardsticks).

There is no CPU path: CPU tensors raise the library's "no CPU fallback" error.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional
from warnings import warn

import numpy as np
import torch

from . import _lib as L
from ._frontend import not_capturing, same_device, tensor_arg
from .functional import _need_gpu, _stream

OUT_KEYS = ('AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L')   # coco_eval.py:109
SUMMARY_KEYS = OUT_KEYS + ('AR_1', 'AR_10', 'AR_100', 'AR_S', 'AR_M', 'AR_L')   # COCOeval.stats, in its order
CLASS_KEYS = ('AP', 'AP_50', 'AP_75', 'AR_100')
MAX_DETS = (1, 10, 100)                                        # pycocotools Params.setDetParams
CLASSES = {'gen1': ("car", "pedestrian"), 'gen4': ("pedestrian", "two-wheeler", "car")}   # evaluation.py:15-18
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)      # pycocotools Params.setDetParams
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_ANCHORS, MAX_LABELS_PER_FRAME, MAX_WINDOW_DETECTIONS = 8192, 128, 8192


class PropheseeEvaluator:
    """ev = PropheseeEvaluator(dataset, downsample_by_2, max_images, max_detections, max_labels_per_frame)
      dataset: 'gen1' (car, pedestrian) or 'gen4' (pedestrian, two-wheeler, car); the box filter is diag 30 / side 10 for gen1 and
      60 / 20 for gen4, halved with downsample_by_2.
    ev.add(labels, counts, det, n_det)
      labels fp32 [N, M, 7] rows (t, x, y, w, h, class_id, class_confidence), counts int32 [N] (0: not a frame), det fp32 [N, A, 7] and
      n_det int32 [N] as `postprocess_padded` returns them for the same N frames.
    ev.add_recordings(gt, n_gt, dt, n_dt, time_tol_us=50_000, max_window_detections=1024)
      whole recordings: label records int32 [S, Gcap, 10] / int64 [S] against detection records int32 [S, Dcap, 10] / int64 [S], matched
      by timestamp (see the method).
    ev.evaluate_buffer(img_height, img_width) -> {'AP', 'AP_50', 'AP_75', 'AP_S', 'AP_M', 'AP_L'} as Python floats (one sync, at the end)
    ev.precision() -> fp64 [10, 101, K, 4] of the last evaluate_buffer; ev.tables() -> the flattened image / annotation / result records
    ev.summary() -> the twelve numbers of COCOeval.stats (AP .. AP_L, AR_1, AR_10, AR_100, AR_S, AR_M, AR_L); ev.coco_eval() ->
      {'precision', 'scores' fp64 [10, 101, K, 4, 3], 'recall' fp64 [10, K, 4, 3]} for maxDets [1, 10, 100], on the device;
      ev.per_class() -> {class name: {'AP', 'AP_50', 'AP_75', 'AR_100'}}.  All three follow a successful evaluate_buffer.
    ev.reset_buffer(), ev.has_data() as in the reference.
    ev.merge(other): other's buffer appended, as if its frames had been added here after this one's; ev.export_buffer() -> dict of
      trimmed device tensors, ev.import_buffer(blob) appends one; ev.all_gather(group=None): every rank ends with the buffers of all
      ranks in rank order (capacities must hold the union: what does not fit raises OverflowError in evaluate_buffer)."""

    def __init__(self, dataset: str, downsample_by_2: bool, max_images: int = 65536, max_detections: int = 1 << 22,
                 max_labels_per_frame: int = 64):
        assert dataset in {'gen1', 'gen4'}
        self.dataset = dataset
        self.downsample_by_2 = bool(downsample_by_2)
        self.classes = CLASSES[dataset]
        self.max_images, self.max_detections, self.max_labels_per_frame = int(max_images), int(max_detections), int(max_labels_per_frame)
        if self.max_images < 1 or not 1 <= self.max_detections < (1 << 30) or not 1 <= self.max_labels_per_frame <= MAX_LABELS_PER_FRAME:
            raise ValueError(f"sast_amd.evaluation: capacities must be max_images >= 1, 1 <= max_detections < 2^30, "
                             f"1 <= max_labels_per_frame <= {MAX_LABELS_PER_FRAME}")
        if self.max_images * self.max_labels_per_frame >= (1 << 31):
            raise ValueError("sast_amd.evaluation: max_images * max_labels_per_frame must stay below 2^31")
        min_box_diag = 60 if dataset == 'gen4' else 30          # evaluation.py:24-31
        min_box_side = 20 if dataset == 'gen4' else 10
        if self.downsample_by_2:
            min_box_diag //= 2
            min_box_side //= 2
        self.min_box_diag, self.min_box_side = min_box_diag, min_box_side
        self.max_window_detections: Optional[int] = None      # of the last add_recordings
        self._buffer_empty = True
        self._dev: Optional[torch.device] = None
        self._t: Dict[str, torch.Tensor] = {}
        self._args = L.SastEvalArgs()
        self._evaluated = False
        self._sum: Optional[Dict[str, object]] = None         # the full summary of the last evaluate_buffer, made on demand

    # ------------------------------------------------------------------------------------------------------------------ buffers
    def _allocate(self, dev: torch.device):
        not_capturing("evaluation", "one un-captured call is needed before graph capture (it allocates the buffers)")
        K, D, G = len(self.classes), self.max_detections, self.max_images * self.max_labels_per_frame
        ws_bytes = self._ws_bytes()

        def e(shape, dt):
            return torch.empty(shape, dtype=dt, device=dev)

        t = self._t = {
            "state": e(L.EVAL_STATE_WORDS, torch.int32),
            "gt_box": e((G, 4), torch.float32), "gt_cls": e(G, torch.int32), "gt_img": e(G, torch.int32),
            "img_t": e(self.max_images, torch.int64),
            "det_box": e((D, 5), torch.float32), "det_cls": e(D, torch.int32), "det_img": e(D, torch.int32),
            "rec_key": e(D, torch.int64), "rec_match": e(D, torch.int64), "rec_ign": e(D, torch.int64), "sorted": e(D, torch.int64),
            "sort_ws": e(ws_bytes, torch.uint8),
            "iou_thr": torch.from_numpy(IOU_THRS).to(dev), "rec_thr": torch.from_numpy(REC_THRS).to(dev),
            "precision": e((L.EVAL_IOU_THRS, L.EVAL_REC_THRS, K, L.EVAL_AREAS), torch.float64),
            "result": e(8 + L.EVAL_STATE_WORDS, torch.float64),
        }
        a = self._args
        for name in ("state", "gt_box", "gt_cls", "gt_img", "img_t", "det_box", "det_cls", "det_img", "rec_key", "rec_match", "rec_ign",
                     "sorted", "sort_ws", "iou_thr", "rec_thr", "precision", "result"):
            setattr(a, name, t[name].data_ptr())
        a.sort_ws_bytes = ws_bytes
        a.K = K
        a.min_diag2, a.min_side = float(self.min_box_diag ** 2), float(self.min_box_side)
        a.max_images, a.max_labels_per_frame, a.max_detections = self.max_images, self.max_labels_per_frame, self.max_detections
        self._dev = dev
        L.check(L.lib().sast_eval_reset(C.byref(a), _stream()), "eval_reset")

    def _ws_bytes(self) -> int:
        ws_bytes = int(L.lib().sast_eval_sort_ws_bytes(self.max_detections))
        if ws_bytes == 0:
            raise RuntimeError("sast_amd.evaluation: the library refused the sort workspace size")
        return ws_bytes

    def reset_buffer(self) -> None:
        """empties the buffer (e.g. in on_validation_epoch_start): one launch, no sync"""
        self._buffer_empty = True
        self._evaluated = False
        if self._dev is not None:
            L.check(L.lib().sast_eval_reset(C.byref(self._args), _stream()), "eval_reset")

    def has_data(self) -> bool:
        """True after an `add` since the last reset.  Adds of a replayed graph are not seen by the host: when it knows of none, the
        device's count of adds is read (a synchronisation, on that path only)."""
        if not self._buffer_empty:
            return True
        return self._dev is not None and int(self._t["state"][11]) > 0

    # ---------------------------------------------------------------------------------------------------------------------- add
    def add(self, labels: torch.Tensor, counts: torch.Tensor, det: torch.Tensor, n_det: torch.Tensor) -> None:
        _need_gpu(labels, counts, det, n_det)
        if labels.dtype != torch.float32 or labels.dim() != 3 or labels.shape[-1] != 7:
            raise TypeError("sast_amd.evaluation: labels must be fp32 [N, M, 7]")
        N, M = int(labels.shape[0]), int(labels.shape[1])
        if counts.dtype != torch.int32 or tuple(counts.shape) != (N,):
            raise TypeError("sast_amd.evaluation: counts must be int32 [N]")
        if det.dtype != torch.float32 or det.dim() != 3 or det.shape[0] != N or det.shape[-1] != 7:
            raise TypeError("sast_amd.evaluation: det must be fp32 [N, A, 7] for the same N frames")
        A = int(det.shape[1])
        if n_det.dtype != torch.int32 or tuple(n_det.shape) != (N,):
            raise TypeError("sast_amd.evaluation: n_det must be int32 [N]")
        if not 1 <= N <= 65535 or M < 1 or not 1 <= A <= MAX_ANCHORS:
            raise ValueError(f"sast_amd.evaluation: need 1 <= N <= 65535 frames, M >= 1 label rows and 1 <= A <= {MAX_ANCHORS} detection rows")
        same_device("evaluation", "labels, counts, det and n_det", labels, counts, det, n_det)
        if self._dev is None:
            self._allocate(labels.device)
        elif labels.device != self._dev:
            raise ValueError("sast_amd.evaluation: the buffer lives on another device")
        labels, counts, det, n_det = labels.contiguous(), counts.contiguous(), det.contiguous(), n_det.contiguous()
        info = torch.empty(N * 16, dtype=torch.int32, device=self._dev)
        a = self._args
        a.labels, a.counts, a.det, a.n_det, a.info = labels.data_ptr(), counts.data_ptr(), det.data_ptr(), n_det.data_ptr(), info.data_ptr()
        a.N, a.M, a.A = N, M, A
        L.check(L.lib().sast_eval_add(C.byref(a), _stream()), "eval_add")
        self._buffer_empty = False
        self._evaluated = False

    def add_recordings(self, gt: torch.Tensor, n_gt: torch.Tensor, dt: torch.Tensor, n_dt: torch.Tensor, time_tol_us: int = 50_000,
                       max_window_detections: int = 1024) -> None:
        """S whole recordings, each one label "file" against one detection "file" as evaluate_list(apply_bbox_filters=True) scores them
        (evaluation.py:5-42, _match_times of metrics/coco_eval.py:55-90).
          gt int32 [S, Gcap, 10], n_gt int64 [S]: the label records of the recordings, ten words per `labels.BBOX_DTYPE` record (what
            `LabelStreams.pack` makes), the first n_gt[s] of a row valid and sorted by t; dt int32 [S, Dcap, 10], n_dt int64 [S]: the
            detection records of the same recordings, sorted by t (e.g. `online.DetectionLog.records` / `.counts`).
        Per row, in row order: both sides pass filter_boxes (t > 500 000 and the size rule; each detection on its own t); every unique
        t of the labels left is an image, numbered behind the images already in the buffer; its detections are the ones with
        t - time_tol_us <= t_det <= t + time_tol_us, so one detection may belong to several images (max_detections counts memberships).
        Everything behind that is `add`'s, and the two may be mixed in one buffer.  max_labels_per_frame is the limit per label
        timestamp; an image whose window holds more than max_window_detections records before the filter (1 .. 8192: it sizes the
        sort) is refused, a row whose records are not sorted by t adds nothing; both are counted on the device and raised by
        `evaluate_buffer` (OverflowError / ValueError).  Four launches, no synchronisation: capturable after one eager call, and a
        replay evaluates the records and counts then in the same tensors."""
        tensor_arg(gt, "gt", "evaluation", (torch.int32,), ("S", "Gcap", 10), "(ten words per box record)", dtype_error=TypeError)
        S, Gcap = int(gt.shape[0]), int(gt.shape[1])
        tensor_arg(n_gt, "n_gt", "evaluation", (torch.int64,), (S,), dtype_error=TypeError)
        tensor_arg(dt, "dt", "evaluation", (torch.int32,), (("S", S), "Dcap", 10), "(ten words per box record)", dtype_error=TypeError)
        Dcap = int(dt.shape[1])
        tensor_arg(n_dt, "n_dt", "evaluation", (torch.int64,), (S,), dtype_error=TypeError)
        if int(time_tol_us) < 0:
            raise ValueError(f"sast_amd.evaluation: time_tol_us must be >= 0, got {time_tol_us}")
        if not 1 <= int(max_window_detections) <= MAX_WINDOW_DETECTIONS:
            raise ValueError(f"sast_amd.evaluation: max_window_detections must be in 1 .. {MAX_WINDOW_DETECTIONS}, got {max_window_detections}")
        if S > 65535 or S * Gcap > ((1 << 31) - 1) // 16 or S * Dcap > (1 << 31) - 1:
            raise ValueError("sast_amd.evaluation: need S <= 65535 recordings, S * Gcap <= (2^31 - 1) / 16 and S * Dcap <= 2^31 - 1 records")
        _need_gpu(gt, n_gt, dt, n_dt)
        same_device("evaluation", "gt, n_gt, dt and n_dt", gt, n_gt, dt, n_dt)
        if self._dev is None:
            self._allocate(gt.device)
        elif gt.device != self._dev:
            raise ValueError("sast_amd.evaluation: the buffer lives on another device")
        r = L.SastEvRecArgs()
        r.gt, r.n_gt, r.dt, r.n_dt = gt.data_ptr(), n_gt.data_ptr(), dt.data_ptr(), n_dt.data_ptr()
        r.S, r.Gcap, r.Dcap, r.max_window, r.time_tol_us = S, Gcap, Dcap, int(max_window_detections), int(time_tol_us)
        r.ws_bytes = int(L.lib().sast_evrec_ws_bytes(S, Gcap))
        ws = torch.empty(r.ws_bytes, dtype=torch.uint8, device=self._dev)       # freed in stream order, behind the four launches
        r.ws = ws.data_ptr()
        L.check(L.lib().sast_evrec_add(C.byref(self._args), C.byref(r), _stream()), "evrec_add")
        self.max_window_detections = int(max_window_detections)
        self._buffer_empty = False
        self._evaluated = False

    # ----------------------------------------------------------------------------------------------------------------- evaluate
    def evaluate_buffer(self, img_height: int, img_width: int) -> Optional[Dict[str, float]]:
        """the six COCO numbers of everything added since the last reset (e.g. in on_validation_epoch_end).  img_height / img_width
        are the reference's arguments: they only fill the image records of its COCO dataset and enter no number."""
        if self._dev is None:
            warn("Attempt to use prophesee evaluation buffer, but it is empty", UserWarning, stacklevel=2)
            return None
        ws_bytes = self._ws_bytes()                 # the accumulate's share grows when SAST_EVAL_ACC_CHUNK was lowered since
        if ws_bytes > self._args.sort_ws_bytes:
            self._t["sort_ws"] = torch.empty(ws_bytes, dtype=torch.uint8, device=self._dev)
            self._args.sort_ws, self._args.sort_ws_bytes = self._t["sort_ws"].data_ptr(), ws_bytes
        L.check(L.lib().sast_eval_accumulate(C.byref(self._args), _stream()), "eval_accumulate")
        self._sum = None
        res = self._t["result"].cpu().numpy()        # the one synchronisation
        state = res[8:].astype(np.int64)
        self._state = state
        if self._buffer_empty and state[11] == 0:    # no add by the host and none by a replayed graph (the device counts them)
            warn("Attempt to use prophesee evaluation buffer, but it is empty", UserWarning, stacklevel=2)
            return None
        if state[29]:
            raise ValueError(f"sast_amd.evaluation: {int(state[29])} recording(s) given to add_recordings were not sorted by t (labels or "
                             "detections) and were not evaluated")
        refused = {"max_images": int(state[8]), "max_detections": int(state[9]), "max_labels_per_frame": int(state[10]),
                   "max_window_detections": int(state[28])}
        if any(refused.values()):
            raise OverflowError("sast_amd.evaluation: frames did not fit the buffer and were not evaluated -- "
                                + ", ".join(f"{v} frame(s) refused for {k}={getattr(self, k)}" for k, v in refused.items() if v))
        self._evaluated = True
        if state[2] == 0:                            # coco_eval.py:112-115: no detection in any image
            return {k: 0.0 for k in OUT_KEYS}
        return {k: float(res[i]) for i, k in enumerate(OUT_KEYS)}

    def precision(self) -> torch.Tensor:
        """COCOeval.eval['precision'][:, :, :, :, 2] (maxDets 100) of the last evaluate_buffer: fp64 [T=10, R=101, K, A=4] on the device"""
        if not self._evaluated:
            raise RuntimeError("sast_amd.evaluation: precision() follows a successful evaluate_buffer()")
        return self._t["precision"].clone()

    # ------------------------------------------------------------------------------------------------ the full COCO summary
    def _summarized(self) -> Dict[str, torch.Tensor]:
        """COCOeval's tables at maxDets [1, 10, 100], the twelve stats and the per-category numbers of the last evaluate_buffer: one
        library call (six launches, no sync) behind it, on the sorted records it left; made once per evaluate_buffer"""
        if not self._evaluated:
            raise RuntimeError("sast_amd.evaluation: summary(), coco_eval() and per_class() follow a successful evaluate_buffer()")
        if self._sum is None:
            K, dev = len(self.classes), self._dev
            shape = (L.EVAL_IOU_THRS, L.EVAL_REC_THRS, K, L.EVAL_AREAS, L.EVSUM_MAXDETS)
            t = {"precision": torch.empty(shape, dtype=torch.float64, device=dev), "scores": torch.empty(shape, dtype=torch.float64, device=dev),
                 "recall": torch.empty(shape[:1] + shape[2:], dtype=torch.float64, device=dev),
                 "numbers": torch.empty(L.EVSUM_STATS + 4 * K, dtype=torch.float64, device=dev)}    # stats, then per_class [K][4]
            s = L.SastEvSumArgs()
            s.precision, s.scores, s.recall = t["precision"].data_ptr(), t["scores"].data_ptr(), t["recall"].data_ptr()
            s.stats = t["numbers"].data_ptr()
            s.per_class = s.stats + 8 * L.EVSUM_STATS
            s.ws_bytes = int(L.lib().sast_evsum_ws_bytes(self.max_detections))
            if s.ws_bytes == 0:
                raise RuntimeError("sast_amd.evaluation: the library refused the summary workspace size")
            ws = torch.empty(s.ws_bytes, dtype=torch.uint8, device=dev)            # freed in stream order, behind the six launches
            s.ws = ws.data_ptr()
            L.check(L.lib().sast_evsum_accumulate(C.byref(self._args), C.byref(s), _stream()), "evsum_accumulate")
            self._sum = t
        return self._sum

    def _numbers(self) -> np.ndarray:
        t = self._summarized()
        if "host" not in t:
            t["host"] = t["numbers"].cpu().numpy()       # the one host copy: twelve stats and 4 K per-category numbers
        return t["host"]

    def summary(self) -> Dict[str, float]:
        """COCOeval.stats of the last evaluate_buffer, in its order: AP, AP_50, AP_75, AP_S, AP_M, AP_L (maxDets 100), AR_1, AR_10, AR_100
        (all areas), AR_S, AR_M, AR_L (maxDets 100); twelve zeros when no image has a detection (coco_eval.py:112-115).  The first six
        are evaluate_buffer's numbers.  One host copy."""
        v = self._numbers()
        if self._state[2] == 0:
            return {k: 0.0 for k in SUMMARY_KEYS}
        return {k: float(v[i]) for i, k in enumerate(SUMMARY_KEYS)}

    def coco_eval(self) -> Dict[str, torch.Tensor]:
        """COCOeval.eval's tables of the last evaluate_buffer for maxDets [1, 10, 100], fp64 on the device: `precision` and `scores`
        [T=10, R=101, K, A=4, M=3], `recall` [10, K, 4, 3].  scores[t, r, k, a, m] is the detection score at which recall REC_THRS[r] is
        first reached at IoU IOU_THRS[t] (0: never reached, -1: no label of that category and size)."""
        t = self._summarized()
        return {k: t[k].clone() for k in ("precision", "recall", "scores")}

    def per_class(self) -> Dict[str, Dict[str, float]]:
        """per name of `self.classes`: AP, AP_50, AP_75 and AR_100 of that category alone over all areas (maxDets 100), each the mean
        over the entries > -1, or -1 when the category has no label"""
        v = self._numbers()[L.EVSUM_STATS:].reshape(len(self.classes), 4)
        return {name: {k: float(v[i, j]) for j, k in enumerate(CLASS_KEYS)} for i, name in enumerate(self.classes)}

    def tables(self) -> Dict[str, np.ndarray]:
        """the flattened records of _to_coco_format (coco_eval.py:143-194) as numpy arrays (synchronises):
        image_t int64 [I] (image id i + 1 is row i); gt_image_id, gt_category_id int64 [G], gt_bbox fp32 [G, 4] (x, y, w, h), gt_area fp64;
        dt_image_id, dt_category_id int64 [D], dt_score fp32, dt_bbox fp32 [D, 4], dt_area fp64 (what COCO.loadRes adds)"""
        if self._dev is None:
            raise RuntimeError("sast_amd.evaluation: nothing was added")
        t = self._t
        st = t["state"].cpu().numpy()
        ni, ng, nd = int(st[0]), int(st[1]), int(st[2])
        gb, db = t["gt_box"][:ng].cpu().numpy(), t["det_box"][:nd].cpu().numpy()
        return {
            "image_t": t["img_t"][:ni].cpu().numpy(),
            "gt_image_id": t["gt_img"][:ng].cpu().numpy().astype(np.int64) + 1,
            "gt_category_id": t["gt_cls"][:ng].cpu().numpy().astype(np.int64) + 1,
            "gt_bbox": gb,
            "gt_area": (gb[:, 2] * gb[:, 3]).astype(np.float64),          # the fp32 product, widened (coco_eval.py:167, :172)
            "dt_image_id": t["det_img"][:nd].cpu().numpy().astype(np.int64) + 1,
            "dt_category_id": t["det_cls"][:nd].cpu().numpy().astype(np.int64) + 1,
            "dt_score": db[:, 4].copy(),
            "dt_bbox": db[:, :4].copy(),
            "dt_area": (db[:, 2] * db[:, 3]).astype(np.float64),
        }

    # -------------------------------------------------------------------------------------------------------------------- merge
    def _check_same_task(self, dataset, downsample_by_2) -> None:
        if dataset != self.dataset or bool(downsample_by_2) != self.downsample_by_2:
            raise ValueError(f"sast_amd.evaluation: cannot merge a buffer of ({dataset}, downsample_by_2={bool(downsample_by_2)}) into one of "
                             f"({self.dataset}, downsample_by_2={self.downsample_by_2}): the categories or the box filter differ")

    def merge(self, other: "PropheseeEvaluator") -> None:
        """appends `other`'s buffer: afterwards this evaluator is what it would be had `other`'s frames been added to it after its
        own, score ties included.  One call on the device, no sync, can be captured in a graph once both have their buffers.  What does
        not fit this evaluator's capacities is appended not at all and raises OverflowError in evaluate_buffer.  `other` is unchanged."""
        if not isinstance(other, PropheseeEvaluator):
            raise TypeError("sast_amd.evaluation: merge takes a PropheseeEvaluator")
        if other is self:
            raise ValueError("sast_amd.evaluation: cannot merge an evaluator into itself")
        self._check_same_task(other.dataset, other.downsample_by_2)
        if other._dev is None:           # never allocated: nothing was added
            return
        if other.max_labels_per_frame > self.max_labels_per_frame:
            raise ValueError(f"sast_amd.evaluation: the other buffer's max_labels_per_frame={other.max_labels_per_frame} exceeds this one's "
                             f"{self.max_labels_per_frame}")
        if self._dev is None:
            self._allocate(other._dev)
        elif other._dev != self._dev:
            raise ValueError("sast_amd.evaluation: the other buffer lives on another device")
        L.check(L.lib().sast_evmerge_append(C.byref(self._args), C.byref(other._args), _stream()), "evmerge_append")
        self._evaluated = False
        self.max_window_detections = self.max_window_detections or other.max_window_detections
        if not other._buffer_empty:      # adds that only a replayed graph made are in the device's count, which was added too
            self._buffer_empty = False

    _BLOB_TABLES = (("img_t", 0, torch.int64, ()), ("gt_box", 1, torch.float32, (4,)), ("gt_cls", 1, torch.int32, ()), ("gt_img", 1, torch.int32, ()),
                    ("det_box", 2, torch.float32, (5,)), ("det_cls", 2, torch.int32, ()), ("det_img", 2, torch.int32, ()),
                    ("rec_key", 3, torch.int64, ()), ("rec_match", 3, torch.int64, ()), ("rec_ign", 3, torch.int64, ()))

    def export_buffer(self) -> Dict[str, object]:
        """the buffer as a dict: `state` int32 [32] and the tables / records named as in include/sast_hip.h, device tensors cut to the
        used counts (copies; one read of the state synchronises), plus `dataset`, `downsample_by_2` and `max_labels_per_frame`"""
        if self._dev is None:
            raise RuntimeError("sast_amd.evaluation: nothing was added")
        t = self._t
        state = t["state"].clone()
        used = [int(v) for v in state[:4].cpu()]
        blob: Dict[str, object] = {"state": state, "dataset": self.dataset, "downsample_by_2": self.downsample_by_2,
                                   "max_labels_per_frame": self.max_labels_per_frame}
        for name, which, _dt, _tail in self._BLOB_TABLES:
            blob[name] = t[name][:used[which]].clone()
        return blob

    def import_buffer(self, blob: Dict[str, object]) -> None:
        """appends a buffer exported by `export_buffer` (of this or another evaluator, e.g. another rank's): the same device call as
        `merge`, on a source staged from the blob; no sync"""
        state = blob["state"]
        tables = [blob[name] for name, *_ in self._BLOB_TABLES]
        _need_gpu(state, *tables)
        self._check_same_task(blob["dataset"], blob["downsample_by_2"])
        mlpf = int(blob["max_labels_per_frame"])
        if mlpf > self.max_labels_per_frame:
            raise ValueError(f"sast_amd.evaluation: the blob's max_labels_per_frame={mlpf} exceeds this evaluator's {self.max_labels_per_frame}")
        if state.dtype != torch.int32 or tuple(state.shape) != (L.EVAL_STATE_WORDS,):
            raise TypeError(f"sast_amd.evaluation: blob['state'] must be int32 [{L.EVAL_STATE_WORDS}]")
        n = [0, 0, 0, 0]
        for (name, which, dt, tail), v in zip(self._BLOB_TABLES, tables):
            if v.dtype != dt or tuple(v.shape[1:]) != tail or v.dim() != 1 + len(tail):
                raise TypeError(f"sast_amd.evaluation: blob['{name}'] must be {dt} [n{''.join(', %d' % d for d in tail)}]")
            if name in ("img_t", "gt_box", "det_box", "rec_key"):
                n[which] = int(v.shape[0])
            elif int(v.shape[0]) != n[which]:
                raise ValueError(f"sast_amd.evaluation: blob['{name}'] has {int(v.shape[0])} rows, its table has {n[which]}")
        if n[1] > max(n[0], 1) * mlpf:
            raise ValueError("sast_amd.evaluation: the blob has more ground-truth rows than its images can hold")
        if self._dev is None:
            self._allocate(state.device)
        dev = self._dev
        if len({v.device for v in (state, *tables)} | {dev}) != 1:
            raise ValueError("sast_amd.evaluation: the blob lives on another device")
        # the padded source: capacities just large enough for the blob's rows (the device clamps the state's counts to them)
        src = L.SastEvalArgs()
        src.K, src.min_diag2, src.min_side = self._args.K, self._args.min_diag2, self._args.min_side
        src.max_images, src.max_labels_per_frame, src.max_detections = max(n[0], 1), mlpf, max(n[2], n[3], 1)
        rows = (src.max_images, src.max_images * mlpf, src.max_detections, src.max_detections)
        keep = [state.contiguous()]
        src.state = keep[0].data_ptr()
        for (name, which, dt, tail), v in zip(self._BLOB_TABLES, tables):
            pad = torch.empty((rows[which],) + tail, dtype=dt, device=dev)
            pad[:n[which]].copy_(v)
            keep.append(pad)
            setattr(src, name, pad.data_ptr())
        L.check(L.lib().sast_evmerge_append(C.byref(self._args), C.byref(src), _stream()), "evmerge_append")
        del keep                          # freed in stream order, behind the two launches
        self._evaluated = False           # (has_data() is decided by the device's count of adds, which the blob's was added to)

    def all_gather(self, group=None) -> None:
        """collective: afterwards every rank's buffer is rank 0's, then rank 1's, ... then the last rank's, so every rank evaluates the
        same numbers -- those of one evaluator fed all ranks' frames in rank order.  Each rank's capacities must hold the union (otherwise
        OverflowError in evaluate_buffer).  The blobs travel as device tensors where the group's backend carries them and through host
        memory otherwise (gloo).  A no-op without an initialised process group or with one rank.  Measured on one GPU shared by two
        ranks only: no node with several GPUs was available to this project."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        world = dist.get_world_size(group)
        on_device = "nccl" in str(dist.get_backend(group)).lower()
        if self._dev is None:
            self._allocate(torch.device("cuda", torch.cuda.current_device()))
        dev = self._dev
        wire = dev if on_device else torch.device("cpu")
        blob = self.export_buffer()
        names = ["state"] + [name for name, *_ in self._BLOB_TABLES]
        order = sorted(names, key=lambda k: -blob[k].element_size())        # 8-byte elements first: every part stays aligned
        packed = torch.cat([blob[k].reshape(-1).view(torch.uint8) for k in order])
        head = torch.tensor([int(blob["img_t"].shape[0]), int(blob["gt_cls"].shape[0]), int(blob["det_cls"].shape[0]),
                             int(blob["rec_key"].shape[0]), self.max_labels_per_frame, int(packed.numel()),
                             2 * sorted(CLASSES).index(self.dataset) + int(self.downsample_by_2)], dtype=torch.int64, device=wire)
        heads = [torch.empty_like(head) for _ in range(world)]
        dist.all_gather(heads, head, group=group)
        heads = [[int(v) for v in h.cpu()] for h in heads]
        if any(h[6] != heads[0][6] for h in heads):
            raise ValueError("sast_amd.evaluation: the ranks' evaluators differ in dataset or downsample_by_2")
        longest = max(h[5] for h in heads)
        mine = torch.zeros(longest, dtype=torch.uint8, device=wire)
        mine[:packed.numel()].copy_(packed)
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        self.reset_buffer()
        for h, part in zip(heads, parts):
            part = part.to(dev)
            rows = {0: h[0], 1: h[1], 2: h[2], 3: h[3]}
            got: Dict[str, object] = {"dataset": self.dataset, "downsample_by_2": self.downsample_by_2, "max_labels_per_frame": h[4]}
            shapes = {"state": (torch.int32, (L.EVAL_STATE_WORDS,))}
            shapes.update({name: (dt, (rows[which],) + tail) for name, which, dt, tail in self._BLOB_TABLES})
            at = 0
            for k in order:
                dt, shape = shapes[k]
                nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
                got[k] = part[at:at + nbytes].view(dt).reshape(shape)
                at += nbytes
            if at != h[5]:
                raise RuntimeError("sast_amd.evaluation: a rank's packed buffer does not have the length its header announces")
            self.import_buffer(got)
