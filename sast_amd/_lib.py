"""ctypes binding of libsast_hip.so (include/sast_hip.h).  Fails loudly when the library is missing:
there is NO CPU / PyTorch fallback for the hot path."""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB_PATH = os.path.join(_HERE, "libsast_hip.so")
# SAST_LIB_PATH: an A/B or variant build instead of the in-tree product library (tools / measurement scripts only).  The override is
# announced on stderr when the library is loaded and `loaded_path()` reports it (bench.py records it in its JSON line), so a stale
# variable in a shell cannot silently put a parity or benchmark claim on another binary.
LIB_PATH = os.environ.get("SAST_LIB_PATH") or DEFAULT_LIB_PATH
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sast_hip.h")

P = C.c_void_p
I32 = C.c_int32
F32 = C.c_float

DT_F32, DT_I32, DT_U8, DT_I64, DT_I16, DT_I8 = 0, 1, 2, 3, 4, 5
EVENT_WINDOW_DURATION, EVENT_WINDOW_COUNT = 0, 1
EVENT_SCAN_BLOCKS = 512   # SAST_EVENT_SCAN_BLOCKS
EVQUEUE_DT_DAT = 6        # SAST_EVQUEUE_DT_DAT
AUGMENT_PARAM_WORDS = 16  # SAST_AUGMENT_PARAM_WORDS
AUGMENT_NONE, AUGMENT_ZOOM_IN, AUGMENT_ZOOM_OUT = 0, 1, 2
EVAL_STATE_WORDS, EVAL_MAX_CLASSES = 32, 4   # SAST_EVAL_STATE_WORDS, SAST_EVAL_MAX_CLASSES
EVAL_IOU_THRS, EVAL_REC_THRS, EVAL_AREAS = 10, 101, 4
# SAST_LABELS_*: the status bits of a LabelStreams row
(LABELS_UNSORTED, LABELS_NEGATIVE_SIZE, LABELS_NO_LABELS, LABELS_BAD_RATE, LABELS_NO_ALIGNED_LABEL, LABELS_ZERO_COUNT, LABELS_TOO_MANY_FRAMES,
 LABELS_TOO_MANY_WINDOWS, LABELS_FRAME_OVERFULL, LABELS_FRAMES_TOO_CLOSE, LABELS_WINDOW_INDEX) = (1 << k for k in range(11))


def _struct(name, spec):
    """spec: list of (ctype, 'a b c') -> ctypes.Structure with fields in order."""
    fields = []
    for ct, names in spec:
        for n in names.split():
            fields.append((n, ct))
    return type(name, (C.Structure,), {"_fields_": fields})


SastDownArgs = _struct("SastDownArgs", [
    (I32, "B H W Cin Cout factor"),
    (P, "x w ln_w ln_b pe conv_out mean rstd y dy dx dw d_ln_w d_ln_b ws"),
    (I32, "x_dtype no_overlap"),
    (P, "x_nonexact"),
])
SastScoreArgs = _struct("SastScoreArgs", [
    (I32, "B L C r_stride"), (F32, "amp"),
    (P, "xp r ws_w ws_b wc scale s xw tok dxw dxp d_ws_w d_ws_b d_wc ws dscale_ws"),
])
SastSel = _struct("SastSel", [(P, "win_keep mask K row_off win_rank counts tok_slot row_tok pack_rows row_seg")])
SastMswsaArgs = _struct("SastMswsaArgs", [
    (I32, "B H W C ph pw mode inner"), (F32, "eps"), (I32, "cb_tps dim_head mlp_act"),
    (P, "xin out"), (SastSel, "sel"),
    (P, "ln1_w ln1_b ln2_w ln2_b qkv_w qkv_b proj_w proj_b ls1 fc1_w fc1_b fc2_w fc2_b ls2"),
    (P, "mean1 rstd1 mean2 rstd2 S QKV O lse Y UG Hh"),
    (P, "dout dxin"),
    (P, "d_ln1_w d_ln1_b d_ln2_w d_ln2_b d_qkv_w d_qkv_b d_proj_w d_proj_b d_ls1 d_fc1_w d_fc1_b d_fc2_w d_fc2_b d_ls2"),
    (P, "ws cb_m cb_sum raw_ws drop1 drop2 drop_ws drop_mlp fused_ws act_w d_act_w"),
])
SastConvBn2Args = _struct("SastConvBn2Args", [
    (I32, "B H W Cin Cout ldx Cin1 ldx2 bn_ws_zeroed bn_red_done0 bn_red_done1 training ksize"), (F32, "momentum0 momentum1 eps0 eps1"),
    (P, "x x2 w0 w1 bn_w0 bn_w1 bn_b0 bn_b1 run_mean0 run_mean1 run_var0 run_var1 conv_out0 conv_out1 stats0 stats1 y0 y1 "
        "bn_ws0 bn_ws1 dy0 dy1 dw0 dw1 d_bn_w0 d_bn_w1 d_bn_b0 d_bn_b1 ws0 ws1 dx dx2 "
        "p_conv_out p_stats p_bn_w p_bn_b p_bn_ws p2_conv_out p2_stats p2_bn_w p2_bn_b p2_bn_ws"),
])
SastHeadGeom = _struct("SastHeadGeom", [(I32, "n_levels"), (I32 * 4, "H"), (I32 * 4, "W"), (F32 * 4, "stride")])
SastLstmArgs = _struct("SastLstmArgs", [
    (I32, "B L C"),
    (P, "x h0 c0 w b h1 c1 gates dh1 dc1 dx dh0 dc0 dw db ws dh1b drop"),
])
SastConvBnArgs = _struct("SastConvBnArgs", [
    (I32, "B H W Cin Cout ksize stride training ldx ldy lddy lddx bn_ws_zeroed bn_red_done Cin1 ldx2"), (F32, "momentum eps"),
    (P, "x w bn_w bn_b run_mean run_var conv_out stats y dy dx dw d_bn_w d_bn_b bn_ws ws x2 dx2 "
        "p_conv_out p_stats p_bn_w p_bn_b p_bn_ws p2_conv_out p2_stats p2_bn_w p2_bn_b p2_bn_ws dy2"),
    (I32, "sync_phase m_total groups"),
])

SastSampleGather = _struct("SastSampleGather", [
    (I32, "n_src n_out B _pad"), (C.c_size_t, "sample_floats"), (P * 32, "src"), (P * 32, "dsrc"), (P, "out"),
    (C.c_uint8 * 256, "t_of"), (C.c_uint8 * 256, "b_of"),
])
SastSampleMask = _struct("SastSampleMask", [(C.c_uint8 * 256, "sel")])
SastSampleGatherDev = _struct("SastSampleGatherDev", [
    (I32, "n_src n_out B _pad"), (C.c_size_t, "sample_floats"), (P * 32, "src"), (P * 32, "dsrc"), (P, "out table slot_of"),
])
ZERO_MAX_TENSORS = 16     # SAST_ZERO_MAX_TENSORS
SastSampleZeroDev = _struct("SastSampleZeroDev", [(I32, "n B"), (P * 16, "x"), (C.c_size_t * 16, "sample_floats"), (P, "flags")])
SastTensorCopy = _struct("SastTensorCopy", [(I32, "n _pad"), (P * 16, "dst"), (P * 16, "src"), (C.c_size_t * 16, "floats")])
SastEventArgs = _struct("SastEventArgs", [
    (P, "x y p t bounds out err ws"), (C.c_int64, "capacity window_capacity"),
    (I32, "x_dtype y_dtype p_dtype t_dtype B bins height width count_cutoff fastmode downsample_by_2 clip_negative_polarity"),
])
SastMdStackArgs = _struct("SastMdStackArgs", [
    (P, "x y p t bounds out err ws"), (C.c_int64, "capacity window_capacity"),
    (I32, "x_dtype y_dtype p_dtype t_dtype B bins height width count_cutoff downsample_by_2 clip_negative_polarity"),
])
SastEvQueueArgs = _struct("SastEvQueueArgs", [
    (P, "x y p t head count t_last retired retired_t err ws"), (C.c_int64, "capacity"), (I32, "S reserved"),
])
SastLabelArgs = _struct("SastLabelArgs", [
    (P, "ws ends_us n_windows frame_ts_us n_frames frame_2_window window_2_frame labels frame_start frame_count status"),
    (C.c_int64, "capacity base_delta_us align_t_us delta_t_us"), (I32, "S width height class_max"), (F32, "min_diag2 min_side max_width"),
    (I32, "reprs_per_frame downsample_by_2 max_frames max_windows max_labels_per_frame reserved"),
])
RND_CLASS_ID, RND_ITEM_INDEX = 1, 2   # SAST_RND_*: the status bits of a RandomAccessPool (per row; pool-wide)
RND_MAX_CLASSES = 256
SastRndArgs = _struct("SastRndArgs", [
    (P, "start_idx_offset length cum class_total weights status ticket"), (I32, "sequence_length only_load_end_labels max_classes weighted"),
])
STREAM_TRUNCATED, STREAM_SCHEDULE_INDEX = 1, 2   # SAST_STREAM_*: the status bits of a StreamingPool (pool-wide)
SastStreamArgs = _struct("SastStreamArgs", [
    (P, "seq_row seq_start seq_stop seq_samples row_first_seq row_count n_seq status order order_len cursor"),
    (I32, "sequence_length guarantee_labels max_sequences order_capacity"),
])
SastEvalArgs = _struct("SastEvalArgs", [
    (P, "labels counts det n_det"), (I32, "N M A K"), (F32, "min_diag2 min_side"), (I32, "max_images max_labels_per_frame"),
    (C.c_int64, "max_detections"),
    (P, "state info gt_box gt_cls gt_img img_t det_box det_cls det_img rec_key rec_match rec_ign iou_thr rec_thr sorted sort_ws"),
    (C.c_size_t, "sort_ws_bytes"), (P, "precision result"),
])

_SIGNATURES = {
    "sast_version": (C.c_int, []),
    "sast_mfma_split3": (C.c_int, []),
    "sast_nzratio": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P]),
    "sast_nchw_to_nhwc": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "sast_nzratio_padded": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P]),
    "sast_nchw_to_nhwc_padded": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "sast_nhwc_to_nchw": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "sast_input_prep": (C.c_int, [P] + [C.c_int] * 7 + [P, P, P, P]),
    "sast_input_prep_flag": (C.c_int, [P] + [C.c_int] * 7 + [P, P, P, P, P]),
    "sast_input_prep_u8": (C.c_int, [P] + [C.c_int] * 6 + [P, P, P, P]),
    "sast_add_rows": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, P]),
    "sast_mean_square_fwd": (C.c_int, [P, P, C.c_int, P, P]),
    "sast_mean_square_bwd": (C.c_int, [P, P, C.c_int, P, C.c_int, P, P]),
    "sast_downsample_ln_fwd": (C.c_int, [C.POINTER(SastDownArgs), P]),
    "sast_downsample_ln_bwd": (C.c_int, [C.POINTER(SastDownArgs), P]),
    "sast_score_stp_fwd": (C.c_int, [C.POINTER(SastScoreArgs), P]),
    "sast_score_stp_bwd": (C.c_int, [C.POINTER(SastScoreArgs), P]),
    "sast_select": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(SastSel), P]),
    "sast_select_packs": (C.c_int, [C.POINTER(SastSel), C.c_int, C.c_int, P]),
    "sast_head_pred_decode": (C.c_int, [P] * 9 + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_int, C.c_int, P]),
    "sast_head_pred_fwd": (C.c_int, [P] * 10 + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_int, C.c_int, P]),
    "sast_head_pred_bwd": (C.c_int, [P] * 14 + [C.c_int] * 7 + [P]),
    "sast_postprocess_ws_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "sast_postprocess": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, P, P, P, P]),
    "sast_yolox_loss_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sast_yolox_loss": (C.c_int, [P, P, C.POINTER(SastHeadGeom), C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P]),
    "sast_mask_token_fwd": (C.c_int, [P, P, P, P, C.c_int, C.c_int, C.c_int, P]),
    "sast_mask_token_bwd": (C.c_int, [P, P, P, P, C.c_int, C.c_int, P]),
    "sast_select_pair": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(SastSel), C.POINTER(SastSel), P]),
    "sast_mswsa_bwd_ws_floats": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "sast_mswsa_raw_ws_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "sast_mswsa_fused_ws_floats": (C.c_size_t, [C.c_int] * 5),
    "sast_mswsa_fwd": (C.c_int, [C.POINTER(SastMswsaArgs), P]),
    "sast_mswsa_bwd": (C.c_int, [C.POINTER(SastMswsaArgs), P]),
    "sast_lstm_fwd": (C.c_int, [C.POINTER(SastLstmArgs), P]),
    "sast_lstm_bwd": (C.c_int, [C.POINTER(SastLstmArgs), P]),
    "sast_dwconv_fwd": (C.c_int, [P, P, P, P] + [C.c_int] * 5 + [P]),
    "sast_dwconv_bwd": (C.c_int, [P, P, P, P, P, P] + [C.c_int] * 5 + [P]),
    "sast_conv_bn_ws_floats": (C.c_int, [C.c_int]),
    "sast_conv_bn_silu_fwd": (C.c_int, [C.POINTER(SastConvBnArgs), P]),
    "sast_conv_bn_silu_bwd": (C.c_int, [C.POINTER(SastConvBnArgs), P]),
    "sast_conv_bn_silu2_fwd": (C.c_int, [C.POINTER(SastConvBn2Args), P]),
    "sast_conv_bn_silu2_bwd": (C.c_int, [C.POINTER(SastConvBn2Args), P]),
    "sast_upsample_cat_fwd": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "sast_upsample_cat_bwd": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P]),
    "sast_cat2_fwd": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, P]),
    "sast_cat2_bwd": (C.c_int, [P, P, P, C.c_int, C.c_int, C.c_int, P]),
    "sast_gather_samples": (C.c_int, [C.POINTER(SastSampleGather), P]),
    "sast_gather_samples_bwd": (C.c_int, [C.POINTER(SastSampleGather), P]),
    "sast_zero_samples": (C.c_int, [P, C.c_int, C.c_size_t, C.POINTER(SastSampleMask), P]),
    "sast_select_table": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P, P, P, P, P]),
    "sast_gather_samples_dev": (C.c_int, [C.POINTER(SastSampleGatherDev), P]),
    "sast_gather_samples_dev_bwd": (C.c_int, [C.POINTER(SastSampleGatherDev), P]),
    "sast_zero_samples_dev": (C.c_int, [C.POINTER(SastSampleZeroDev), P]),
    "sast_copy_tensors": (C.c_int, [C.POINTER(SastTensorCopy), P]),
    "sast_adamw_onecycle": (C.c_int, [P, P, P, P, C.c_size_t, P, C.c_double, C.c_double, F32, F32, F32, F32, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_double, P]),
    "sast_dw_defer": (C.c_int, [C.c_int]),
    "sast_dw_defer_rows": (C.c_int, [C.c_long, C.c_long]),
    "sast_dw_pending": (C.c_int, []),
    "sast_dw_discard": (C.c_int, []),
    "sast_dw_flush": (C.c_int, [P]),
    "sast_launch_count": (C.c_ulonglong, []),
    "sast_config_reload": (C.c_int, []),
    "sast_config_get": (C.c_int, [C.c_char_p, C.c_int]),
    "sast_config_report": (C.c_size_t, [C.c_char_p, C.c_size_t]),
    "sast_prof_enable": (C.c_int, [C.c_int]),
    "sast_prof_calibrate": (C.c_float, [P, C.c_int]),
    "sast_prof_report": (C.c_size_t, [C.c_char_p, C.c_size_t]),
    "sast_adamw": (C.c_int, [P, P, P, P, C.c_size_t, P, C.c_double, C.c_double, F32, F32, F32, F32, P]),
    "sast_event_correct_time": (C.c_int, [P, C.c_int, P, C.c_int64, P, P, P, P]),
    "sast_event_window_bounds": (C.c_int, [P, P, C.c_int64, P, C.c_int, C.c_int, C.c_int64, P, P]),
    "sast_event_frames_ws_bytes": (C.c_size_t, [C.c_int] * 5 + [C.c_int64]),
    "sast_event_frames": (C.c_int, [C.POINTER(SastEventArgs), P]),
    "sast_mdstack_frames_ws_bytes": (C.c_size_t, [C.c_int] * 5 + [C.c_int64]),
    "sast_mdstack_frames": (C.c_int, [C.POINTER(SastMdStackArgs), P]),
    "sast_evstreams_ws_count": (C.c_size_t, [C.c_int]),
    "sast_evstreams_correct_time": (C.c_int, [P, C.c_int, P, C.c_int, C.c_int64, P, P, P, P, P]),
    "sast_evstreams_window_bounds": (C.c_int, [P, P, C.c_int, C.c_int64, P, C.c_int, C.c_int, C.c_int64, P, P]),
    "sast_rnd_window_bounds": (C.c_int, [P, P, C.c_int, C.c_int64, P, P, C.c_int, C.c_int, C.c_int, C.c_int64, P, P]),
    "sast_evqueue_ws_count": (C.c_size_t, [C.c_int]),
    "sast_evqueue_push": (C.c_int, [C.POINTER(SastEvQueueArgs), P, P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int64, P, P]),
    "sast_evqueue_window_bounds": (C.c_int, [C.POINTER(SastEvQueueArgs), P, C.c_int, C.c_int, C.c_int64, P, P]),
    "sast_evqueue_retire": (C.c_int, [C.POINTER(SastEvQueueArgs), P, C.c_int, P]),
    "sast_labels_ws_bytes": (C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    "sast_labels_load": (C.c_int, [C.POINTER(SastLabelArgs), P, P, P, P]),
    "sast_labels_gather": (C.c_int, [C.POINTER(SastLabelArgs), P, C.c_int, P, P, P, P, P]),
    "sast_rnd_index": (C.c_int, [C.POINTER(SastLabelArgs), C.POINTER(SastRndArgs), P]),
    "sast_rnd_gather": (C.c_int, [C.POINTER(SastLabelArgs), C.POINTER(SastRndArgs), P, C.c_int] + [P] * 9),
    "sast_mixed_latest": (C.c_int, [C.POINTER(SastLabelArgs), C.POINTER(SastRndArgs), P, C.c_int, P, P, P]),
    "sast_stream_index": (C.c_int, [C.POINTER(SastLabelArgs), C.POINTER(SastStreamArgs), P]),
    "sast_stream_next": (C.c_int, [C.POINTER(SastLabelArgs), C.POINTER(SastStreamArgs), C.c_int] + [P] * 13),
    "sast_mixed_next": (C.c_int, [C.POINTER(SastLabelArgs), C.POINTER(SastStreamArgs), C.POINTER(SastRndArgs), C.c_int, P, C.c_int] + [P] * 15),
    "sast_augment_frames": (C.c_int, [P, P, P] + [C.c_int] * 5 + [P]),
    "sast_augment_labels": (C.c_int, [P, P, P] + [C.c_int] * 4 + [P, P, P, P]),
    "sast_eval_reset": (C.c_int, [C.POINTER(SastEvalArgs), P]),
    "sast_eval_add": (C.c_int, [C.POINTER(SastEvalArgs), P]),
    "sast_eval_sort_ws_bytes": (C.c_size_t, [C.c_int64]),
    "sast_eval_accumulate": (C.c_int, [C.POINTER(SastEvalArgs), P]),
    "sast_evmerge_append": (C.c_int, [C.POINTER(SastEvalArgs), C.POINTER(SastEvalArgs), P]),
}

_lib = None


def declared_symbols():
    """every function name declared in include/sast_hip.h"""
    with open(HEADER_PATH) as f:
        src = f.read()
    return sorted(set(re.findall(r"\b(sast_[a-z0-9_]+)\s*\(", src)))


def lib():
    global _lib
    if _lib is None:
        # PyTorch-ROCm ships its own libamdhip64.so: it must be in the process BEFORE this library is loaded, otherwise the dynamic
        # linker binds libsast_hip.so to the system copy under /opt/rocm and the process ends up with two HIP runtimes -- torch's
        # owns the device, ours reports "no ROCm-capable device" at the first launch (seen when build() loaded the library first)
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m sast_amd.build` (needs hipcc, gfx950). "
                "sast_amd has no CPU/PyTorch fallback for the SAST hot path.")
        if os.path.abspath(LIB_PATH) != os.path.abspath(DEFAULT_LIB_PATH):
            import sys
            print(f"[sast_amd] WARNING: SAST_LIB_PATH is set: loading {LIB_PATH} instead of the product library {DEFAULT_LIB_PATH}", file=sys.stderr)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name, None)
            if fn is None:
                if is_product_library():
                    raise AttributeError(f"{LIB_PATH} lacks {name}: rebuild it with `python -m sast_amd.build`")
                continue           # an A/B library built from another commit (tools only): that entry point raises when it is called
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def reload_knobs() -> int:
    """the library re-reads every SAST_* tuning knob from the environment at its next use (call after changing os.environ in-process)"""
    return int(lib().sast_config_reload())


def knobs() -> dict:
    """{name: value in use} of the SAST_* knobs the library has read so far"""
    n = lib().sast_config_report(None, 0)
    buf = C.create_string_buffer(n)
    lib().sast_config_report(buf, n)
    out = {}
    for line in buf.value.decode().splitlines():
        k, v = line.split("=", 1)
        out[k] = int(v.split(" ")[0])
    return out


def loaded_path() -> str:
    """the library file behind lib() (the in-tree product unless SAST_LIB_PATH overrides it)"""
    return os.path.abspath(LIB_PATH)


def is_product_library() -> bool:
    return os.path.abspath(LIB_PATH) == os.path.abspath(DEFAULT_LIB_PATH)


_tools = None


def tools_lib():
    """libsast_hip_tools.so: GEMM micro-benchmark / timeline entry points (csrc/k_test.hip) for tools/*.py -- not the product"""
    global _tools
    if _tools is None:
        lib()      # the tools library links against the product library (same directory, rpath $ORIGIN)
        _tools = C.CDLL(os.environ.get("SAST_TOOLS_LIB_PATH") or os.path.join(_HERE, "libsast_hip_tools.so"))   # (variant builds: A/B of k_test.hip)
    return _tools


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"libsast_hip: {what} failed with code {rc}")
