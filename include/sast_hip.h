/* sast_hip.h -- C ABI of libsast_hip.so: the MI355X (gfx950) implementation of the SAST hot path.
 *
 * The reference (Peterande/SAST) has no FFI: its hot path is plain torch.nn.Module code under
 * models/layers.  Each entry point below replaces the ATen op sequence of the
 * cited reference lines; the Python modules in sast_amd/ bind them with ctypes (see
 * INTEGRATION.md for the reference-side binding a maintainer would add).
 *
 * This file is the SINGLE SOURCE of that binding: sast_amd/_header.py reads it at import and sast_amd/_lib.py builds every
 * ctypes.Structure, every (restype, argtypes) pair and every integer constant from what it finds, so a new entry point, struct field
 * or constant is written here and nowhere else.  The reader knows plain, regular C only and REFUSES the rest (RuntimeError at import,
 * with the text it could not place): what it accepts is `#define SAST_X <integer literal>`, `enum { ... };` with explicit values,
 * `1 << k` or implicit increments, `typedef struct [Tag] { ... } Name;` whose fields are scalars, pointers, arrays sized by a literal
 * or an earlier constant, or an earlier struct, and prototypes of sast_* functions with named arguments.  Scalar types: int, long,
 * unsigned long long, float, double, size_t and the <stdint.h> names.  No unions, bit-fields, function pointers, nested struct bodies,
 * conditional blocks or value macros that are not integer literals; function-like macros are left to C.  tests/test_abi.py has gcc
 * check every size, offset, value and argument list the reader derives.
 *
 * Conventions
 *  - all tensors are device pointers owned by the CALLER (PyTorch caching allocator); the library
 *    never allocates, frees or retains pointers;  workspaces are caller-provided.
 *  - activations are fp32, channels-last: "image layout" = [B*H*W, C] rows (NHWC).
 *  - conv weights are [Cout][KH][KW][Cin] (torch channels_last storage of a [Cout,Cin,KH,KW] param).
 *  - every call only ENQUEUES work on `stream` (a hipStream_t); no host synchronisation, so a whole
 *    training step is hipGraph-capturable.  Data-dependent sizes (number of kept windows/tokens)
 *    stay on the device in SastSel.counts.
 *  - return 0 on success, negative errno-style code otherwise (-22 bad argument, -5 launch failure).
 *  - *_bwd calls ACCUMULATE (+=) into parameter-gradient buffers and OVERWRITE activation gradients.
 *  - size limit of every entry point that runs on the GEMM template (linear layers, convolutions, ConvLSTM, MS-WSA, the heads): an
 *    operand tensor a GEMM reads -- activations, weights, incoming gradients, the tensor a row gather reads from -- spans less than
 *    2^31 bytes from its base pointer (rows x row stride x 4; index-contiguous operands: 64 rows more).  The loaders address operands
 *    with 32-bit byte offsets; a call with a larger operand returns -22 before anything is enqueued.  (B = 32 at 1 Mpx reaches 629 MB.)
 *
 * Non-finite values (pinned by tests/test_nonfinite_operators.py on the recipes of tests/nonfinite_cases.py, and by the NaN / Inf tests
 * of tests/test_optim_operators.py and tests/test_act_operators.py)
 *  - what a call is told to ignore is never read into a result: the tokens a selection does not keep (sast_mswsa_*: every kept row and
 *    every parameter gradient but d(norm1.weight) -- an unkept row leaves the layer as LN1(x), so its own output row, its dx and that
 *    one gradient carry whatever it holds), the rows under the mask token, the samples a gather does not select, a reset does not flag
 *    or a commit does not move.  A zeroed state is exact zeros whatever it held, NaN included; data movement is bit for bit.
 *  - samples are independent outside batch-statistics BatchNorm: a NaN or Inf in one sample of x reaches the outputs and the input
 *    gradients of that sample only (conv + BatchNorm in eval mode, downsample + LayerNorm, the depth-wise conv, the ConvLSTM), and inside
 *    a sample only the pixels whose window holds it.  In training mode the batch statistics carry it to every row, as in torch.
 *  - it is not swallowed either: every result that depends on the poisoned value is non-finite, parameter gradients included.  A NaN
 *    in a gradient reaches the parameter: sast_adamw* clip by value like torch's clamp_ (NaN stays NaN, +-Inf clips to +-clip), so p, m
 *    and v turn NaN there instead of taking a finite step of -clip.  The clamps of the gate activations (relu, relu6, hard_sigmoid,
 *    hard_swish, hard_mish) keep NaN as torch's do.
 *  - where the expression itself multiplies a non-finite value by an exact zero the result may be NaN or clean: the weight-gradient
 *    rows of the ConvLSTM that an absent state skips, a weight-gradient tap that only meets padding.  An Inf in a GEMM operand may
 *    surface as NaN where fp32 arithmetic would give Inf or a saturated gate: the operand split computes Inf - Inf.
 *  - not covered: kernels whose control flow follows float values (STP scoring -> selection, the YOLOX loss / SimOTA, NMS, the
 *    evaluator, the event, label and augment kernels) expect finite input.  sast_nzratio* / sast_input_prep* pool with fmaxf, which
 *    ignores a NaN pixel where max_pool2d counts it; event tensors are integer counts.
 */
#ifndef SAST_HIP_H
#define SAST_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sast_stream_t; /* hipStream_t */

/* SAST_DT_I8: the int8 frames of the mixed-density event stack.  sast_nzratio*, sast_input_prep / sast_input_prep_flag and
 * sast_nchw_to_nhwc* take F32 / I32 / U8 / I8; a pooled cell of non_zero_ratio counts when its MAXIMUM is non-zero (max_pool2d), so for
 * signed data a cell of only {-1, 0} is empty and a cell of only negative values is occupied. */
enum { SAST_DT_F32 = 0, SAST_DT_I32 = 1, SAST_DT_U8 = 2, SAST_DT_I64 = 3, SAST_DT_I16 = 4, SAST_DT_I8 = 5 };

int sast_version(void);
/* 1: the GEMM template evaluates fp32 products as six bf16 MFMAs on an exact three-way operand split (default build);
 * 0: v_mfma_f32_32x32x2_f32 (-DSAST_MFMA_SPLIT3=0); 2: the reduced-precision library libsast_hip_bf16.so (-DSAST_MFMA_BF16=1: operands
 * rounded to bf16, one MFMA per tile step, fp32 accumulate -- `bench.py --precision bf16`, never part of an fp32 parity claim) */
int sast_mfma_split3(void);

/* a1  non_zero_ratio -- models/detection/recurrent_backbone/sast_rnn.py:45-60.
 * x: (B,Cin,H,W) NCHW of `dtype`; cnt_ws: int32[B*4*Cin] scratch; r: fp32 (B,4,Cin). H,W multiples of 32. */
int sast_nzratio(const void* x, int dtype, int B, int Cin, int H, int W, int32_t* cnt_ws, float* r, sast_stream_t stream);
/* same on an event tensor stored UNPADDED (H x W, multiples of 4) that stands for its zero padding to Hp x Wp at the bottom /
 * right -- InputPadderFromShape.pad_tensor_ev_repr, utils/padding.py:29-53, modules/detection.py:143-144 -- without building it */
int sast_nzratio_padded(const void* x, int dtype, int B, int Cin, int H, int W, int Hp, int Wp, int32_t* cnt_ws, float* r,
                        sast_stream_t stream);

/* the whole input side in ONE launch (modules/detection.py:143-144 pad + cast, sast_rnn.py:45-60 non_zero_ratio,
 * sast_rnn.py:153 / ops.py:19-24 float + NCHW->NHWC): x (B,C,H,W) of `dtype`, possibly smaller than the padded size (Hp,Wp) it stands
 * for (zeros at the bottom / right), is read ONCE -> r fp32 (B,4,C) and y fp32 (B,Hp,Wp,C).  H,W multiples of 4; Hp,Wp multiples of
 * 32 with (Hp/32)*(Wp/32) even; C = 20 (the stacked-histogram representation: 2 polarities x 10 time bins).  ws: int32[B*4*C + 1], ZERO on entry and left zero on exit (the last
 * workgroup finishes the ratios and clears it), so a caller allocates and clears it once. */
int sast_input_prep(const void* x, int dtype, int B, int C, int H, int W, int Hp, int Wp, int32_t* ws, float* r, float* y,
                    sast_stream_t stream);
/* the same, and additionally *nonexact (one word that belongs to THIS call's y, allocated with it by the caller) = 0 iff every value
 * of y is exactly one bf16 (low 16 bits of the fp32 pattern zero: stacked-histogram counts, every integer of magnitude <= 256), else
 * non-zero.  Handed to the stem conv (SastDownArgs.x_nonexact) it lets the stem GEMMs skip the three product terms of the operand's
 * zero bf16 planes; evaluated on the device at every call, also on every replay of a captured graph.  y must not be written after the call while
 * the word is in use (a stale 0 drops the lower planes: ~2^-8 relative error).  +-Inf and the default quiet NaN also have zero low
 * bits: such an input counts as exact, and an Inf then gives Inf * w where the six-term split gives NaN (Inf - Inf) -- not
 * reachable from event counts.  ws: int32[B*4*C + 2] here (one
 * more scratch word than sast_input_prep, which keeps its size), zero on entry and left zero on exit. */
int sast_input_prep_flag(const void* x, int dtype, int B, int C, int H, int W, int Hp, int Wp, int32_t* ws, float* r, float* y,
                         uint32_t* nonexact, sast_stream_t stream);
/* the same for the event tensor as the dataset stores it (uint8 counts, data/genx_utils/sequence_base.py:88-98): y keeps the BYTES,
 * (B,Hp,Wp,C) uint8 NHWC, zero padded -- a quarter of the traffic of the fp32 copy.  The stem conv reads it directly
 * (SastDownArgs.x_dtype = SAST_DT_U8); the `.float()` of modules/detection.py:143-144 / sast_rnn.py:153 happens in its loaders. */
int sast_input_prep_u8(const uint8_t* x, int B, int C, int H, int W, int Hp, int Wp, int32_t* ws, float* r, uint8_t* y, sast_stream_t stream);

/* layout changes at the NCHW API boundary (reference: ops.py:19-30 nChw_2_nhwC / nhwC_2_nChw, x.float() sast_rnn.py:153) */
int sast_nchw_to_nhwc(const void* x, int dtype, int B, int C, int H, int W, float* y, sast_stream_t stream);
/* cast + layout change + zero padding to Hp x Wp in one pass: y[B, Hp, Wp, C] */
int sast_nchw_to_nhwc_padded(const void* x, int dtype, int B, int C, int H, int W, int Hp, int Wp, float* y, sast_stream_t stream);
int sast_nhwc_to_nchw(const float* x, int B, int C, int H, int W, float* y, sast_stream_t stream);

/* a3  x + pos_emb(x) -- SAST.py:105 with the constant sine table of sast_rnn.py:180-219: y[row] = x[row] + table[row % table_rows] */
int sast_add_rows(const float* x, const float* table, float* y, int rows, int C, int table_rows, sast_stream_t stream);

/* mean squares of up to 4 dense fp32 tensors in one launch: partials[t*SAST_MEAN_SQUARE_BLOCKS + b], whose sum is
   sum_t mean(x_t^2) -- the synthetic training objective of bench.py (the reference's benchmark.py has no loss; its real
   objective is sast_yolox_loss).  x / n / dx are HOST arrays of `count` device pointers / element counts (n % 4 == 0). */
#define SAST_MEAN_SQUARE_BLOCKS 128   /* (round 5: 32 workgroups per tensor left 160 CUs idle: 11.8 + 13.6 us for 14 MB) */
int sast_mean_square_fwd(const float* const* x, const size_t* n, int count, float* partials, sast_stream_t stream);
int sast_mean_square_bwd(const float* const* x, const size_t* n, int count, const float* d_partials, int d_stride, float* const* dx,
                         sast_stream_t stream);   /* d_stride 1: one gradient per partial; 0: d_partials[0] for all (the broadcast gradient of a .sum()) */
/* a11  mask token (enable_masking) -- sast_rnn.py:271-273: x[token_mask] = mask_token, in place on the [rows, C] rows AFTER the first
 * block's position embedding was added (pos_emb [L, C] or NULL): masked rows become mask_token + pos_emb[row % L].
 * backward: dx = dy with masked rows zeroed, d_token += sum of the masked rows of dy. */
int sast_mask_token_fwd(float* x, const uint8_t* mask, const float* token, const float* pos_emb, int rows, int C, int L, sast_stream_t stream);
int sast_mask_token_bwd(const float* dy, const uint8_t* mask, float* dx, float* d_token, int rows, int C, sast_stream_t stream);

/* a2  ConvDownsampling_Cf2Cl -- models/layers/SAST/ops.py:54-95 (+ the pos-emb add of SAST.py:105 when pe != NULL) */
typedef struct SastDownArgs {
  int32_t B, H, W, Cin, Cout, factor;
  const float* x;        /* [B*H*W, Cin] NHWC */
  const float* w;        /* [Cout][k][k][Cin], k = 2*factor-1, replicate padding factor-1 (see no_overlap) */
  const float* ln_w; const float* ln_b;
  const float* pe;       /* [Ho*Wo, Cout] or NULL */
  float* conv_out;       /* [B*Ho*Wo, Cout] saved for backward */
  float* mean; float* rstd; /* [B*Ho*Wo] */
  float* y;              /* [B*Ho*Wo, Cout] = LN(conv) (+ pe) */
  /* backward */
  const float* dy; float* dx; /* dx may be NULL (stem) */
  float* dw; float* d_ln_w; float* d_ln_b;
  float* ws;             /* fp32[B*Ho*Wo*Cout] */
  int32_t x_dtype;       /* SAST_DT_F32 (0): x is fp32 NHWC.  SAST_DT_U8: x is the uint8 event tensor in NHWC bytes as written by
                            sast_input_prep_u8 (stem only: dx must be NULL) -- the conv loaders widen the bytes themselves, the fp32
                            copy of the input never exists (modules/detection.py:143-144 does `.float()` first) */
  int32_t no_overlap;    /* 0: downsample_cfg.overlap True (every shipped config): k = 2*factor-1, replicate padding factor-1.
                            1: overlap False (ops.py:74-76): k = factor, no padding; w is [Cout][factor][factor][Cin] */
  const uint32_t* x_nonexact; /* fwd + bwd, optional (stem, x_dtype SAST_DT_F32, dx == NULL in the backward): the word sast_input_prep_flag
                            wrote for x.  While it reads 0 the conv and its weight gradient issue only the three bf16 product terms of
                            x's top plane (the other three multiply zeros: same results).  NULL = nothing known about x: all six terms.
                            A SAST_DT_U8 input is exact by type and needs no word.  SAST_STEM_EXACT_BF16=0 turns both off. */
} SastDownArgs;
/* Ho = H / factor, Wo = W / factor.  The overlapping form takes H, W that are multiples of the factor only (SAST_EINVAL otherwise: the
 * conv would have ceil(H / factor) rows and a replicate clamp at the bottom / right edge); no_overlap floors, as nn.Conv2d does. */
int sast_downsample_ln_fwd(const SastDownArgs* a, sast_stream_t stream);
int sast_downsample_ln_bwd(const SastDownArgs* a, sast_stream_t stream);

/* a5  scoring + STP weighting -- SAST.py:109-119 and PositiveLinear :305-328.
 * xw = sigmoid(scale)*sigmoid(s)*xp,  s = relu(xp Ws^T + bs),  tok[b,l] = sum_c (AMP/scale[b,c]) * s */
typedef struct SastScoreArgs {
  int32_t B, L, C, r_stride;
  float amp;
  const float* xp;       /* [B*L, C] = x + pos-emb */
  const float* r;        /* r[b*r_stride + j], j < 20 */
  const float* ws_w; const float* ws_b; /* to_scores */
  const float* wc;       /* to_controls.weight [C,20] */
  float* scale;          /* [B,C] saved */
  float* s;              /* [B*L,C] saved */
  float* xw;             /* [B*L,C] out */
  float* tok;            /* [B*L] out (not differentiable) */
  /* backward */
  const float* dxw; float* dxp;
  float* d_ws_w; float* d_ws_b; float* d_wc;
  float* ws;             /* fp32[B*L*C + B*C] */
  float* dscale_ws;      /* optional fp32[B*C]: cleared by the forward, accumulated into by the backward of the same call pair;
                            NULL = the backward clears the tail of ws itself */
} SastScoreArgs;
int sast_score_stp_fwd(const SastScoreArgs* a, sast_stream_t stream);
int sast_score_stp_bwd(const SastScoreArgs* a, sast_stream_t stream);

/* a6-a8  window / token selection -- SAST.py:84-96, :258-281, :122.  All buffers caller-allocated. */
typedef struct SastSel {
  int32_t* win_keep;   /* [B*N] 0/1 */
  uint64_t* mask;      /* [B*N][2] kept-token bitmask of each group for T <= 128, [B*N][4] for 128 < T <= 256 (the limit) */
  int32_t* K;          /* [B*N] kept tokens (0 for dropped windows) */
  int32_t* row_off;    /* [B*N] first compact row of the group */
  int32_t* win_rank;   /* [B*N] index among kept windows or -1 */
  int32_t* counts;     /* [4] sum K (= len(asy_index)), M (= len(index_window)), sumK / B, 0 */
  int32_t* tok_slot;   /* [B*L] compact row of a token or -1 */
  int32_t* row_tok;    /* [B*L] token (b*L + y*W + x) of a compact row */
  /* PACKS (round 4): the kept rows of consecutive groups are contiguous, so several small groups can share the 32-token tiles of one
   * workgroup of the fused MS-WSA layer kernel (its cost follows kept tokens, not kept groups x tiles).  A pack = the largest aligned
   * block of 1, 2, 4, 8 or 16 consecutive groups whose kept rows fit one 32-token tile (SAST_ATTN_PACKS overrides the budget, at most
   * 64 rows for T <= 64); attention inside a pack is masked to the rows of the query's own group. */
  int32_t* pack_rows;  /* [B*N] rows of the pack this group LEADS (first group of its block), 0 for every other group */
  int32_t* row_seg;    /* [B*L] per compact row: lo | hi << 16 = the rows [lo, hi) of its own group, relative to the pack's first row */
} SastSel;
/* fills pack_rows / row_seg from K / row_off (sast_select and sast_select_pair do it themselves; hosts that build a SastSel from
 * index lists call this).  W = number of groups, T = tokens per group. */
int sast_select_packs(const SastSel* sel, int W, int T, sast_stream_t stream);
/* mode 0: window partition (ops.py:189-195), 1: grid partition (ops.py:206-212) */
int sast_select(const float* tok, int B, int H, int W, int ph, int pw, int mode, double bounce, const SastSel* sel,
                sast_stream_t stream);
/* both selections of one SAST block (window layer, then grid layer, on the same token scores -- SAST.py:120-123,141-147)
 * in the same launches; results identical to two sast_select calls with mode 0 and 1. */
int sast_select_pair(const float* tok, int B, int H, int W, int ph, int pw, double bounce, const SastSel* win, const SastSel* grid,
                     sast_stream_t stream);

/* a9  MS_WSA -- SAST.py:199-255 with LayerScale (ops.py:178-186) and GLU-MLP (ops.py:111-175). */
typedef struct SastMswsaArgs {
  int32_t B, H, W, C, ph, pw, mode, inner;
  float eps;
  int32_t cb_tps;        /* Context Broadcasting (enable_CB, SAST.py:240-246): tokens per sample, 0 = off */
  int32_t dim_head;      /* attention head width (SAST.py:171-181): 32 (default when 0) or 24; heads = C / dim_head */
  int32_t mlp_act;       /* gate activation of the GLU-MLP (attention_cfg.mlp_activation, SAST.py:38,55 -> ops.py:133-137; the names of
                            layers/create_act.py:62-79): 0 gelu (erf form; every shipped config)  1 relu  2 silu / swish  3 sigmoid  4 tanh
                            5 mish  6 relu6  7 leaky_relu  8 elu / celu  9 selu  10 hard_sigmoid  11 hard_swish  12 hard_mish
                            13 prelu (learnable slope: act_w / d_act_w below); the one-kernel form (fused_ws) exists for 0 only */
  const float* xin;      /* [B*L, C] image layout */
  float* out;            /* [B*L, C] */
  SastSel sel;
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *qkv_w, *qkv_b, *proj_w, *proj_b, *ls1;
  const float *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ls2;
  /* saved for backward; R = B*L rows upper bound */
  float *mean1, *rstd1;  /* [B*L] */
  float *mean2, *rstd2;  /* [R] */
  float *S, *QKV, *O, *lse, *Y, *UG, *Hh; /* [R,C] [R,3C] [R,C] [R,heads] [R,C] [R,2*inner] [R,inner] */
  /* backward */
  const float* dout; float* dxin;
  float *d_ln1_w, *d_ln1_b, *d_ln2_w, *d_ln2_b, *d_qkv_w, *d_qkv_b, *d_proj_w, *d_proj_b, *d_ls1;
  float *d_fc1_w, *d_fc1_b, *d_fc2_w, *d_fc2_b, *d_ls2;
  float* ws;             /* sast_mswsa_bwd_ws_floats() */
  float *cb_m, *cb_sum;  /* cb_tps > 0 only: scratch [R,C] and [B*L/cb_tps, C] (fwd and bwd) */
  float* raw_ws;         /* optional fp32[sast_mswsa_raw_ws_floats()]: cleared by the forward, accumulated into by the backward of the
                            SAME call pair (saves the backward a clearing launch); NULL = backward clears its own scratch */
  const float *drop1, *drop2;  /* DropPath (`drop_path > 0`, SAST.py:188,193,232,248; reference default 0): fp32[R] each, per KEPT ROW (compact
                            order = asy_index order) keep / keep_prob of the attention branch (drop1) and of the MLP branch (drop2); the caller
                            draws them.  Both or neither; NULL = no DropPath (p = 0 or eval).  Not with fused_ws. */
  float* drop_ws;        /* bwd with drop1 / drop2: fp32[2 * R * C] scratch (the scaled branch gradients) */
  const float* drop_mlp; /* `drop_mlp > 0` (ops.py:167: nn.Dropout between the GLU and the second linear; reference default 0): fp32[R, inner]
                            keep mask / (1 - p) per kept row and hidden channel, drawn by the caller; NULL = none.  Not with fused_ws. */
  float* fused_ws;       /* optional fp32[sast_mswsa_fused_ws_floats()] (16-byte aligned): when non-NULL and that size is non-zero the
                            layer runs as ONE kernel per direction (csrc/k_mswsa_fused.hip: one wave per partition, activations in
                            registers from LN to the scatter).  With S == NULL (inference) nothing else is written; with the saved-activation
                            buffers mean1 .. Hh present the same kernel also writes them, so that sast_mswsa_bwd runs unchanged.  The forward
                            fills fused_ws with the bf16x3 weight planes its kernel streams. */
  const float* act_w;    /* mlp_act 13 (prelu; layers/activations.py:124-131: nn.PReLU, one slope, init 0.25): fp32[1] on the device */
  float* d_act_w;        /* bwd, mlp_act 13: fp32[1], accumulated into (sum over the gate elements <= 0 of dh * value * gate) */
} SastMswsaArgs;
/* 0 = this layer shape has no fused form (the caller passes fused_ws = NULL and the saved-activation buffers) */
size_t sast_mswsa_fused_ws_floats(int C, int inner, int T, int dim_head, int cb_tps);
size_t sast_mswsa_raw_ws_floats(int C, int inner);
size_t sast_mswsa_bwd_ws_floats(int rows, int C, int inner);
int sast_mswsa_fwd(const SastMswsaArgs* a, sast_stream_t stream);
int sast_mswsa_bwd(const SastMswsaArgs* a, sast_stream_t stream);

/* a12  DWSConvLSTM2d (dws_conv=False) -- models/layers/rnn.py:36-69, on NHWC rows */
typedef struct SastLstmArgs {
  int32_t B, L, C;
  const float* x; const float* h0; const float* c0;   /* h0/c0 NULL = zero state */
  const float* w; const float* b;                      /* conv1x1 [4C,2C], [4C] */
  float* h1; float* c1;
  float* gates;          /* [B*L,4C] saved: sigmoid(f,i,o), tanh(g).  c0 == NULL (and SAST_LSTM_SKIP_DEAD_GATE, default 1): the forget gate
                            multiplies a zero cell state, so the forward runs the GEMM over the three live gates (weight rows [C, 4C))
                            and gates[:, 0:C] is UNDEFINED afterwards; a NaN / Inf that would enter c1 only through the forget gate's
                            pre-activation no longer does.  The backward then works on the gate rows [C, 4C) alone: dw[0:C, :] and
                            db[0:C] are left as they are (the four-gate form adds exact zeros), and a non-NULL dc0 is refused
                            (SAST_EINVAL: dc0 = dc * f needs the f that was not saved).  With c0 != NULL nothing changes.  dx / dh0
                            equal the four-gate form's bit for bit when C is a multiple of 64 (128 for the 8-k-group tile), else
                            up to summation order.  The knob
                            must not change between a forward and its backward. */
  /* backward */
  const float* dh1; const float* dc1;                  /* dc1 may be NULL */
  float* dx; float* dh0; float* dc0;                   /* dh0/dc0 may be NULL */
  float* dw; float* db;
  float* ws;             /* fp32[B*L*4C] */
  const float* dh1b;     /* bwd, optional: a second gradient of h1 (h1 consumed by two ops), added to dh1 on the fly */
  const float* drop;     /* fwd + bwd, optional: fp32[B*L, C] = the keep mask of `cell_update_dropout` divided by (1 - p) (rnn.py:34,64:
                            nn.Dropout on tanh(cell_input)); the caller draws it (torch's RNG), NULL = no dropout (p = 0 or eval mode) */
} SastLstmArgs;
int sast_lstm_fwd(const SastLstmArgs* a, sast_stream_t stream);
int sast_lstm_bwd(const SastLstmArgs* a, sast_stream_t stream);

/* Depth-wise k x k convolution with bias on NHWC rows (zero padding k / 2, stride 1): `conv3x3_dws` of DWSConvLSTM2d with
 * dws_conv=True (models/layers/rnn.py:24-28; applied to the previous hidden state :52-53, or to x and h separately when
 * dws_conv_only_hidden=False :55-56 -- a depth-wise conv of cat(x, h) is the two halves convolved on their own).
 * x, y, dy, dx: [B, H, W, C] fp32; w: [C][k][k] (the Conv2d(groups=C) weight, contiguous); b: [C] or NULL; k odd, k*k <= 49, C % 4 == 0.
 * bwd: dx may be NULL; dw / db are ACCUMULATED into. */
int sast_dwconv_fwd(const float* x, const float* w, const float* b, float* y, int B, int H, int W, int C, int k, sast_stream_t stream);
int sast_dwconv_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int B, int H, int W, int C, int k,
                    sast_stream_t stream);

/* a13  BaseConv = Conv2d(no bias, same pad) + BatchNorm2d + SiLU -- yolox/models/network_blocks.py:29-54 */
/* the conv epilogue accumulates the batch statistics with atomics; same-address atomics serialise at the memory side, so
   the row tiles spread them over SAST_BN_STAT_COPIES copies that the BatchNorm kernel adds up */
#define SAST_BN_STAT_COPIES 4
#define SAST_BN_WS_FLOATS(Cout) ((4 * SAST_BN_STAT_COPIES + 2 * SAST_BN_STAT_COPIES) * (Cout))
int sast_conv_bn_ws_floats(int Cout);   /* = SAST_BN_WS_FLOATS(Cout), for hosts that cannot read the macro */
typedef struct SastConvBnArgs {
  int32_t B, H, W, Cin, Cout, ksize, stride, training;
  int32_t ldx, ldy, lddy, lddx;   /* channel strides of x, y, dy, dx rows (slices of concat buffers) */
  int32_t bn_ws_zeroed;           /* 1: caller guarantees bn_ws is zero-filled (one memset for the whole FPN) */
  int32_t bn_red_done;            /* bwd: 1 = the conv consuming y already accumulated this conv's BatchNorm-backward sums (see p_*) */
  int32_t Cin1, ldx2;             /* 1x1 convs only, with x2 != NULL: input = channel concat [x (Cin1 ch) | x2 (Cin - Cin1 ch, row stride ldx2)]
                                     read in place (th.cat of network_blocks.py:140 / yolo_pafpn.py:129,134 never materialised) */
  float momentum, eps;
  const float* x; const float* w; const float* bn_w; const float* bn_b;
  float* run_mean; float* run_var;  /* updated in training mode */
  float* conv_out;       /* [M,Cout] saved, M = B*Ho*Wo.  NULL with training == 0: inference, BatchNorm + SiLU run in the conv
                            epilogue (one launch) and nothing is kept for a backward (stats unused) */
  float* stats;          /* [2*Cout] saved: mean, rstd actually used */
  float* y;
  /* backward */
  const float* dy; float* dx; float* dw; float* d_bn_w; float* d_bn_b;
  float* bn_ws;          /* fp32[SAST_BN_WS_FLOATS(Cout)] reduction scratch: fwd uses the first 4*COPIES*C floats as fp64
                            [COPIES][sum | sum of squares][C], bwd the 2*COPIES*C floats after them ([COPIES][sum dz | sum dz*xhat][C]) */
  float* ws;             /* bwd only: fp32[M*Cout] (dconv) */
  const float* x2;       /* second input of the virtual concat (NULL = single input) */
  float* dx2;            /* its gradient, dense [M, Cin - Cin1] */
  /* backward, training mode, stride 1, optional: the conv_bn_silu that PRODUCED x (p_*) / x2 (p2_*), when this conv is the
     ONLY consumer of that output (so the dx / dx2 written here IS the producer's dy).  The dX epilogue then also accumulates
     the producer's BatchNorm-backward column sums (sum dz, sum dz*xhat) into the producer's bn_ws, and the producer's own
     backward is called with bn_red_done = 1 and skips its reduction launch.  All NULL: no folding. */
  const float* p_conv_out; const float* p_stats; const float* p_bn_w; const float* p_bn_b; float* p_bn_ws;
  const float* p2_conv_out; const float* p2_stats; const float* p2_bn_w; const float* p2_bn_b; float* p2_bn_ws;
  const float* dy2;      /* bwd, optional: a second gradient of y (y consumed by two ops; row stride lddy), added to dy on the fly */
  /* SyncBatchNorm -- the reference trains with sync_batchnorm=True whenever it runs DDP (train.py:167; torch.nn.SyncBatchNorm
     semantics): training-mode calls split around the HOST's all-reduce of the statistics (the library never calls a collective).
       0      the whole op on the rows of this process (BatchNorm2d)
       fwd 1  conv + this process's fp64 column sums into bn_ws, return.  The host all-reduces (SUM) the fp64 block
              bn_ws[0, 4*COPIES*Cout) floats and the row counts M of the ranks;
       fwd 2  BatchNorm + SiLU from bn_ws as it now is, over m_total rows (running statistics updated with the global mean and the
              unbiased global variance, like torch); the conv is not run again.
       bwd 1  this process's (sum dz, sum dz*xhat) into the fp32 block bn_ws[4*COPIES*Cout, 6*COPIES*Cout) (not run when
              bn_red_done: the consumer's dX epilogue has them already); the block, summed over its COPIES, is added to d_bn_b /
              d_bn_w (when both are non-NULL) -- the affine gradients stay LOCAL sums as in torch.nn.SyncBatchNorm (DDP averages them
              with every other gradient); return.  The host then all-reduces (SUM) the block;
       bwd 2  the rest (BatchNorm-backward apply with 1 / m_total, dW, dX, producer folding); d_bn_w / d_bn_b NULL. */
  int32_t sync_phase, m_total;
  int32_t groups;        /* 0 / 1: dense conv.  == Cin == Cout: depth-wise conv -- the `dconv` of YOLOX's DWConv (network_blocks.py:57-76:
                            BaseConv(in, in, ksize, stride, groups=in), used for Bottleneck.conv2, bu_conv* and the head towers when the
                            model is built with depthwise=True); w is [C][ksize*ksize] (torch's (C,1,k,k)), single dense input (x2 NULL,
                            ldx == Cin), no producer folding (p_* NULL); BatchNorm / SiLU / sync_phase as for the dense conv */
} SastConvBnArgs;
int sast_conv_bn_silu_fwd(const SastConvBnArgs* a, sast_stream_t stream);
int sast_conv_bn_silu_bwd(const SastConvBnArgs* a, sast_stream_t stream);

/* a13b  TWO BaseConvs (1x1, stride 1, equal Cout) of the SAME input in training mode -- CSPLayer.conv1 / conv2
   (yolox/models/network_blocks.py:131-133) -- evaluated as one GEMM over the stacked weights [w0; w1]: one launch for both
   convs (+ one for both BatchNorm/SiLU passes); backward: one BatchNorm-backward pass for both, then ONE (dW || dX) launch
   in which dX = [dconv0 | dconv1] [w0; w1] is the SUM of both input gradients (no separate accumulation).  Fields with a
   0 / 1 suffix belong to conv 0 / conv 1 and mean what they mean in SastConvBnArgs. */
typedef struct SastConvBn2Args {
  int32_t B, H, W, Cin, Cout, ldx, Cin1, ldx2;   /* Cout of EACH conv; input = x (Cin1 == Cin) or the virtual concat [x | x2] */
  int32_t bn_ws_zeroed, bn_red_done0, bn_red_done1;
  int32_t training;               /* 1: batch statistics (everything below applies); 0: inference -- running statistics, BatchNorm +
                                     SiLU in the GEMM epilogue, ONE launch for both convs, nothing kept (conv_out / stats / bn_ws unused) */
  int32_t ksize;                  /* 1, or 3 (stride 1, same padding, single-source input: the two first tower convs of a YOLOX head level) */
  float momentum0, momentum1, eps0, eps1;
  const float* x; const float* x2;
  const float* w0; const float* w1; const float* bn_w0; const float* bn_w1; const float* bn_b0; const float* bn_b1;
  float* run_mean0; float* run_mean1; float* run_var0; float* run_var1;
  float* conv_out0; float* conv_out1; float* stats0; float* stats1; float* y0; float* y1; float* bn_ws0; float* bn_ws1;
  /* backward */
  const float* dy0; const float* dy1; float* dw0; float* dw1; float* d_bn_w0; float* d_bn_w1; float* d_bn_b0; float* d_bn_b1;
  float* ws0; float* ws1;      /* ws0: fp32[M * 2*Cout] (rows [dconv0 | dconv1]); ws1 unused */
  float* dx; float* dx2;       /* dense [M, Cin1] and [M, Cin - Cin1]; dx == NULL: weight gradients only */
  /* producers of x / x2 whose only consumers are these two convs (see SastConvBnArgs.p_*) */
  const float* p_conv_out; const float* p_stats; const float* p_bn_w; const float* p_bn_b; float* p_bn_ws;
  const float* p2_conv_out; const float* p2_stats; const float* p2_bn_w; const float* p2_bn_b; float* p2_bn_ws;
} SastConvBn2Args;
int sast_conv_bn_silu2_fwd(const SastConvBn2Args* a, sast_stream_t stream);
int sast_conv_bn_silu2_bwd(const SastConvBn2Args* a, sast_stream_t stream);

/* a13  nearest-exact x2 upsample + channel concat -- yolo_pafpn.py:49,119-120.
 * out[B,2H,2W,C1+C2] = cat(up2(a[B,H,W,C1]), b[B,2H,2W,C2]) ; backward splits/sums. */
int sast_upsample_cat_fwd(const float* a, const float* b, float* out, int B, int H, int W, int C1, int C2, sast_stream_t stream);
int sast_upsample_cat_bwd(const float* dout, float* da, float* db, int B, int H, int W, int C1, int C2, sast_stream_t stream);
/* plain channel concat of two NHWC row sets and its split (yolo_pafpn.py:129,134; network_blocks.py:140) */
int sast_cat2_fwd(const float* a, const float* b, float* out, int rows, int C1, int C2, sast_stream_t stream);
int sast_cat2_bwd(const float* dout, float* da, float* db, int rows, int C1, int C2, sast_stream_t stream);

/* ---- YOLOX head -- yolox/models/yolo_head.py.  The 15 Conv+BN+SiLU units of the head go through
 * sast_conv_bn_silu_{fwd,bwd}; below are the 1x1 prediction convs (+ decode), the SimOTA assignment and the losses. */
typedef struct SastHeadGeom {       /* FPN levels, finest first: anchors of level k are [sum_{i<k} H_i*W_i, ... + H_k*W_k) */
  int32_t n_levels;                 /* 1..4 */
  int32_t H[4], W[4];
  float stride[4];
} SastHeadGeom;
/* last step of one head level: prediction convs reg(4) / obj(1) on the regression feature and cls(nc) on the classification feature
 * (NHWC rows [B*H*W, hidden]); yolo_head.py:184-186,192-210,248-262,264-289.
 *   pred  (optional) [B, anchors_total, 5+nc]: box (decoded like decode_outputs when decode != 0), sigmoid(obj), sigmoid(cls)
 *   train (optional) same shape: decoded box ((xy + grid) * stride, exp(wh) * stride) and the RAW obj / cls logits (get_losses' input) */
int sast_head_pred_fwd(const float* reg_feat, const float* cls_feat, const float* w_reg, const float* b_reg, const float* w_obj,
                       const float* b_obj, const float* w_cls, const float* b_cls, float* pred, float* train, int B, int H, int W, int hidden,
                       int num_classes, float stride, int anchor_offset, int anchors_total, int decode, sast_stream_t stream);
/* = sast_head_pred_fwd(..., pred = out, train = NULL, ...) */
int sast_head_pred_decode(const float* reg_feat, const float* cls_feat, const float* w_reg, const float* b_reg, const float* w_obj,
                          const float* b_obj, const float* w_cls, const float* b_cls, float* out, int B, int H, int W, int hidden,
                          int num_classes, float stride, int anchor_offset, int anchors_total, int decode, sast_stream_t stream);
/* backward of the prediction convs of one level; draw[B, anchors_total, 5+nc] = d loss / d (raw conv outputs) from sast_yolox_loss.
 * d_*_feat are written, the weight / bias gradients are ACCUMULATED (+=). */
int sast_head_pred_bwd(const float* draw, const float* reg_feat, const float* cls_feat, const float* w_reg, const float* w_obj,
                       const float* w_cls, float* d_reg_feat, float* d_cls_feat, float* dw_reg, float* db_reg, float* dw_obj, float* db_obj,
                       float* dw_cls, float* db_cls, int B, int H, int W, int hidden, int num_classes, int anchor_offset, int anchors_total,
                       sast_stream_t stream);
/* get_losses (yolo_head.py:291-443) with the SimOTA assignment (:452-606) for the whole batch, no host sync:
 *   train_out [B, A, 5+nc] from sast_head_pred_fwd, labels [B, max_labels, 5] = (cls, cx, cy, w, h), valid rows first, all-zero rows = padding
 *   losses[6] = loss, 5*iou_loss, conf_loss, cls_loss, l1_loss (0 unless use_l1), num_fg / max(num_gts, 1)
 *   draw [B, A, 5+nc] = d loss / d (raw conv outputs) (chain through the decode included)
 *   fg_mask / matched_gt / matched_iou [B, A]: the assignment (matched_gt = -1, iou = 0 for background anchors)
 * use_l1 != 0 adds the L1 term on the raw regression outputs (yolo_head.py:199-208,426-430; off by default in the reference). */
size_t sast_yolox_loss_ws_bytes(int B, int anchors_total, int max_labels);
int sast_yolox_loss(const float* train_out, const float* labels, const SastHeadGeom* geom, int B, int max_labels, int num_classes, int use_l1,
                    float* losses, float* draw, int32_t* fg_mask, int32_t* matched_gt, float* matched_iou, void* ws, sast_stream_t stream);

/* postprocess -- yolox/utils/boxes.py:32-76: confidence filter (obj * max class conf >= conf_thre), greedy NMS --
 * class-aware (torchvision.ops.batched_nms in the reference) or, with class_agnostic != 0, over all boxes (torchvision.ops.nms).  prediction [B, A, 5+nc] = (cx, cy, w, h, obj, cls...) as
 * returned by the head; out [B, A, 7] = (x1, y1, x2, y2, obj_conf, class_conf, class_pred), the first n_out[b] rows of image b are
 * its detections by decreasing score.  A <= 8192. */
size_t sast_postprocess_ws_bytes(int B, int anchors_total);
int sast_postprocess(const float* prediction, int B, int anchors_total, int num_classes, float conf_thre, float nms_thre, int class_agnostic,
                     float* out, int32_t* n_out, void* ws, sast_stream_t stream);

/* (f)2  label-sparse feature gather -- BackboneFeatureSelector, modules/utils/detection.py:24-47 (used by the training step,
 * modules/detection.py:161-177): out = cat over the sequence's timesteps t of feat_t[selected_t], samples being contiguous chunks
 * of `sample_floats` floats (one NHWC feature map of one sample).  Output sample j comes from src[t_of[j]] sample b_of[j].
 * sast_gather_samples copies; sast_gather_samples_bwd writes the gradient of EVERY sample of every timestep tensor (dsrc[t], B samples
 * each): the matching rows of `out` (= d out) or zeros.  n_src <= 32 timesteps, n_out <= 256 selected samples, B <= 256. */
#define SAST_GATHER_MAX_SRC 32
#define SAST_GATHER_MAX_OUT 256
typedef struct {
  int32_t n_src, n_out, B, _pad;
  size_t sample_floats;                  /* multiple of 4 */
  const float* src[SAST_GATHER_MAX_SRC]; /* forward: the timestep tensors */
  float* dsrc[SAST_GATHER_MAX_SRC];      /* backward: their gradients (all written) */
  float* out;                            /* forward: [n_out, sample_floats]; backward: the gradient of it (read) */
  uint8_t t_of[SAST_GATHER_MAX_OUT], b_of[SAST_GATHER_MAX_OUT];
} SastSampleGather;
int sast_gather_samples(const SastSampleGather* a, sast_stream_t stream);
int sast_gather_samples_bwd(const SastSampleGather* a, sast_stream_t stream);
/* RNNStates.reset, modules/utils/detection.py:96-130: x[b] = 0 for the samples with sel[b] != 0, in place (x: [B, sample_floats]) */
typedef struct { uint8_t sel[256]; } SastSampleMask;
int sast_zero_samples(float* x, int B, size_t sample_floats, const SastSampleMask* sel, sast_stream_t stream);

/* (f)2 on the device: the same selection with the table and the reset flags in DEVICE memory, so that a captured training step is
 * replayed on a new label pattern and new sequence starts (the host-table structs above travel by value: one pattern per graph).
 * sast_select_table turns labelled [T, B] (uint8, != 0: the pair carries a label frame, modules/detection.py:161-171) into the list of
 * selected pairs in the reference's order (timestep-major, batch index ascending), one workgroup, nothing read from the host:
 *   table[j] = (t, b) for j < min(n_sel, n_out), (-1, -1) behind that;  slot_of[t * B + b] = j, or -1 (not selected, or j >= n_out)
 *   *n_sel = the number of flagged pairs;  err[0] += 1 when n_sel > n_out (pattern truncated), err[1] += 1 when n_sel < n_out (under-full)
 * T <= 32, B <= 256, n_out <= 256 (n_out = K, the batch of the PAFPN / head pass, is the host's: BatchNorm statistics over exactly K rows). */
int sast_select_table(const uint8_t* labelled, int T, int B, int n_out, int32_t* table, int32_t* slot_of, int32_t* n_sel, int32_t* err,
                      sast_stream_t stream);
typedef struct {
  int32_t n_src, n_out, B, _pad;
  size_t sample_floats;                  /* any count >= 1: 16-byte accesses where both rows are 16-byte aligned, a scalar tail */
  const float* src[SAST_GATHER_MAX_SRC]; /* forward: the timestep tensors */
  float* dsrc[SAST_GATHER_MAX_SRC];      /* backward: their gradients (all written) */
  float* out;                            /* forward: [n_out, sample_floats]; backward: the gradient of it (read) */
  const int32_t* table;                  /* device, [n_out][2] = (t, b) or (-1, -1): forward */
  const int32_t* slot_of;                /* device, [n_src * B]: backward */
} SastSampleGatherDev;
/* forward: out row j = src[table[j].t] sample table[j].b; a row whose entry is negative (or names no sample of the call) is written as zeros.
 * backward: EVERY sample of every dsrc[t] is written -- row slot_of[t * B + b] of `out`, or zeros (slot < 0 or >= n_out).  The words are
 * moved as bit patterns: the same entry points carry feature maps, label rows and int32 counts. */
int sast_gather_samples_dev(const SastSampleGatherDev* a, sast_stream_t stream);
int sast_gather_samples_dev_bwd(const SastSampleGatherDev* a, sast_stream_t stream);
/* RNNStates.reset with the flags on the device: sample b of each of the n tensors (x[i]: [B, sample_floats[i]]) is zeroed where
 * flags[b] != 0, in ONE launch (the eight ConvLSTM state tensors of a four-stage backbone go in one call) */
#define SAST_ZERO_MAX_TENSORS 16
typedef struct {
  int32_t n, B;
  float* x[SAST_ZERO_MAX_TENSORS];
  size_t sample_floats[SAST_ZERO_MAX_TENSORS];
  const uint8_t* flags;                  /* device, [B] */
} SastSampleZeroDev;
int sast_zero_samples_dev(const SastSampleZeroDev* a, sast_stream_t stream);
/* the predicated state commit of a batch whose rows advance at different moments: sample b of dst[i] takes sample b of src[i] where
 * flags[b] != 0 and keeps every bit otherwise (dst[i], src[i]: [B, sample_floats[i]], n <= 16 pairs in ONE launch).  The flags are read
 * when the kernel runs.  16-byte copies where both samples are 16-byte aligned, single words otherwise and for the tail. */
typedef struct {
  int32_t n, B;
  float* dst[SAST_ZERO_MAX_TENSORS];
  const float* src[SAST_ZERO_MAX_TENSORS];
  size_t sample_floats[SAST_ZERO_MAX_TENSORS];
  const uint8_t* flags;                  /* device, [B] */
} SastSampleCommitDev;
int sast_commit_samples_dev(const SastSampleCommitDev* a, sast_stream_t stream);
/* dst[i][0 .. floats[i]) = src[i][...] for n <= 16 tensors in ONE launch, a kernel (no memcpy node when captured): the training step
 * hands the final recurrent states back into its input state tensors with it (RNNStates.save_states_and_detach for a replayed step) */
typedef struct {
  int32_t n, _pad;
  float* dst[SAST_ZERO_MAX_TENSORS];
  const float* src[SAST_ZERO_MAX_TENSORS];
  size_t floats[SAST_ZERO_MAX_TENSORS];
} SastTensorCopy;
int sast_copy_tensors(const SastTensorCopy* a, sast_stream_t stream);

/* fused AdamW over a flat parameter buffer (torch.optim.AdamW semantics, modules/detection.py:409-441).  The betas are doubles and
 * the bias corrections 1 - beta^step are evaluated in double, as torch does with its python scalars.  Every element is updated:
 * a parameter that received no gradient counts as gradient 0 (torch skips grad=None parameters; identical when every parameter is
 * on the loss path, as in this model). */
int sast_adamw(float* p, const float* g, float* m, float* v, size_t n,
               const float* lr_step /* device fp32[2]: learning rate, step count (already incremented) */,
               double beta1, double beta2, float eps, float weight_decay, float grad_scale,
               float clip_value /* <=0: off; reference clips by value 1.0, train.py:156-157 */, sast_stream_t stream);
/* the same with the learning rate of torch.optim.lr_scheduler.OneCycleLR(anneal_strategy='linear', cycle_momentum=False, two phases)
 * as configured at modules/detection.py:418-431, evaluated ON THE DEVICE from the step counter lr_step[1] (lr_step[0] is ignored):
 * optimizer step t (1-based) uses the scheduler's lr at step_num = t - 1, i.e.
 * phase 1 (step_num <= end1): initial_lr -> max_lr, phase 2: max_lr -> min_lr at end2 = total_steps - 1; end1 = pct_start*total_steps - 1.
 * No host interaction per step: a hipGraph replay advances the schedule by itself. */
int sast_adamw_onecycle(float* p, const float* g, float* m, float* v, size_t n, float* lr_step, double beta1, double beta2, float eps,
                        float weight_decay, float grad_scale, float clip_value, double initial_lr, double max_lr, double min_lr,
                        double end1, double end2, sast_stream_t stream);

/* ---- raw events -> stacked-histogram frames (csrc/k_events.hip).  The reference builds its input offline on the CPU:
 * StackedHistogram.construct (data/utils/representations.py:37-121) once per window of scripts/genx/preprocess_dataset.py:476-530, on
 * timestamps its reader made non-decreasing (:159-168) and polarities clipped at 0 (:177), downsampled by 2 with nearest-exact
 * interpolation for Gen4 (:463-473).  Event arrays x, y, p are SAST_DT_I64 / I32 / I16, t is SAST_DT_I64 / I32.  Per-frame sizes (event
 * count n, window ends, the time carry) live in device memory; grids are sized from capacities, so the calls replay inside a graph. */
#define SAST_EVENT_SCAN_BLOCKS 512
enum { SAST_EVENT_WINDOW_DURATION = 0, SAST_EVENT_WINDOW_COUNT = 1 };

/* t_out[i] = max(t[i], t_last, t[0..i-1]) for i < min(*n, capacity), then *t_last = that running maximum (the carry into the next chunk;
 * the reader starts it at 0).  t_out may alias t when t is int64.  ws: int64[SAST_EVENT_SCAN_BLOCKS + 1]. */
int sast_event_correct_time(const void* t, int t_dtype, const int64_t* n, int64_t capacity, int64_t* t_out, int64_t* t_last, int64_t* ws,
                            sast_stream_t stream);
/* window b over the sorted t[0 .. min(*n, capacity)):  end = searchsorted(t, ends_us[b], 'right');  start = searchsorted(t, ends_us[b] -
 * value, 'left') (SAST_EVENT_WINDOW_DURATION, value in microseconds) or max(end - value, 0) (SAST_EVENT_WINDOW_COUNT, value events).
 * bounds: int64 [B, 2] = (start, end). */
int sast_event_window_bounds(const int64_t* t, const int64_t* n, int64_t capacity, const int64_t* ends_us, int B, int mode, int64_t value,
                             int64_t* bounds, sast_stream_t stream);

typedef struct SastEventArgs {
  const void* x;            /* event columns, `*_dtype` each; events [bounds[b][0], bounds[b][1]) form window b */
  const void* y;
  const void* p;            /* 0 / 1 (negative values are invalid, or 0 with clip_negative_polarity) */
  const void* t;            /* non-decreasing within a window: the bin of an event is computed from the window's first / last t */
  const int64_t* bounds;    /* int64 [B, 2], clipped to [0, capacity) */
  uint8_t* out;             /* uint8 [B, 2*bins, H', W']: H' = height / 2, W' = width / 2 with downsample_by_2, else height, width */
  int32_t* err;             /* int32 [2], ACCUMULATED: [0] invalid events (x, y outside the sensor, p outside 0..1) among those the
                               windows hold, each counted once however many windows hold it (events in no window are not read);
                               they are never written;
                               [1] windows with more than window_capacity kept events (left all zero) */
  void* ws;                 /* sast_event_frames_ws_bytes(); ZERO on first use, left zero for the next call */
  int64_t capacity;         /* events the x / y / p / t buffers hold (<= 2^31 - 1) */
  int64_t window_capacity;  /* kept events per window the workspace holds */
  int32_t x_dtype, y_dtype, p_dtype, t_dtype;
  int32_t B, bins, height, width;   /* height / width: the sensor, full resolution; 2*bins <= 640 */
  int32_t count_cutoff;     /* 1 .. 255 (the reference's None is 255) */
  int32_t fastmode;         /* 1: counts wrap modulo 256, then min(count, cutoff);  0: counts wrap as int16, then clamp(0, cutoff) */
  int32_t downsample_by_2;  /* only events with odd x and odd y count, at (y / 2, x / 2) */
  int32_t clip_negative_polarity;
} SastEventArgs;
size_t sast_event_frames_ws_bytes(int B, int bins, int height, int width, int downsample_by_2, int64_t window_capacity); /* 0: unsupported */
int sast_event_frames(const SastEventArgs* a, sast_stream_t stream);

/* ---- raw events -> mixed-density event stack (csrc/k_events.hip): MixedDensityEventStack.construct (data/utils/representations.py:
 * 130-218), the second representation of the reference's preprocessing (scripts/genx/preprocess_dataset.py:631-676), on the windows,
 * bounds, event columns, error counters and workspace rules of sast_event_frames.  Per window [s, e): t0 = t[s], t1 = t[e-1];
 * t_norm = fp32(t - t0) / fp32(max(t1 - t0, 1)) (one correctly rounded fp32 division) clamped to [fp32(1e-6), fp32(1 - 1e-6)];
 * bin = max(bins + floor(log2(t_norm)), 0), read from the fp32 exponent (what the reference's floor(bins - log(t_norm) / log(1/2)) gives
 * while neighbouring integer times stay distinguishable in fp32 near a bin boundary: window spans up to about 2 s); each event adds
 * 2p - 1 at (bin, y, x); channel i becomes the sum of channels 0..i; the sums wrap to int8 and are clamped to +-count_cutoff.
 * downsample_by_2: output (i, j) is input (2i+1, 2j+1) (downsample_ev_repr, preprocess_dataset.py:463-473, int8 branch).  Integer
 * sums: bitwise reproducible.  4 launches, grids sized from capacities: replays inside a graph. */
typedef struct SastMdStackArgs {
  const void* x;            /* event columns, `*_dtype` each; events [bounds[b][0], bounds[b][1]) form window b */
  const void* y;
  const void* p;            /* 0 / 1 (negative values are invalid, or 0 with clip_negative_polarity) */
  const void* t;            /* non-decreasing within a window */
  const int64_t* bounds;    /* int64 [B, 2], clipped to [0, capacity) */
  int8_t* out;              /* int8 [B, bins, H', W']: H' = height / 2, W' = width / 2 with downsample_by_2, else height, width */
  int32_t* err;             /* int32 [2], ACCUMULATED, as SastEventArgs.err: [0] invalid events, [1] windows over window_capacity */
  void* ws;                 /* sast_mdstack_frames_ws_bytes(); ZERO on first use, left zero for the next call */
  int64_t capacity;         /* events the x / y / p / t buffers hold (<= 2^31 - 1) */
  int64_t window_capacity;  /* kept events per window the workspace holds */
  int32_t x_dtype, y_dtype, p_dtype, t_dtype;
  int32_t B, bins, height, width;   /* height / width: the sensor, full resolution; bins <= 512 */
  int32_t count_cutoff;     /* 0 .. 127: clamp to [-cutoff, cutoff] (0: an all-zero frame);  -1: the reference's None, no clamp */
  int32_t downsample_by_2;  /* only events with odd x and odd y count, at (y / 2, x / 2) */
  int32_t clip_negative_polarity;
} SastMdStackArgs;
size_t sast_mdstack_frames_ws_bytes(int B, int bins, int height, int width, int downsample_by_2, int64_t window_capacity); /* 0: unsupported */
int sast_mdstack_frames(const SastMdStackArgs* a, sast_stream_t stream);

/* ---- S recordings side by side: event buffers [S, stream_capacity], row s one recording with counts[s] valid events at its head
 * (int64 [S] in device memory), its own time-correction carry t_last[s] and its own windows.  sast_event_correct_time /
 * sast_event_window_bounds are the S = 1 form of the two calls below (the same kernels: counts = n, t_last a one-element row, reset =
 * NULL, T = B); sast_event_frames is then called unchanged with B = T * S windows,
 * capacity = S * stream_capacity and these bounds.  A window never spans two rows: both of its bounds lie in
 * [s * stream_capacity, s * stream_capacity + n_s], n_s = min(max(counts[s], 0), stream_capacity), so events past a row's count are
 * never read.  Each call is a fixed number of launches (2 and 1) whatever S is; the grids are sized from S and stream_capacity. */

/* int64 elements of the `ws` of sast_evstreams_correct_time (0: S < 1 or S > 65535) */
size_t sast_evstreams_ws_count(int S);
/* per row s: t_out[s][i] = max(t[s][i], carry_s, t[s][0..i-1]) for i < n_s, then t_last[s] = that running maximum;  carry_s =
 * t_last[s], or 0 when reset != NULL and reset[s] != 0 (uint8 [S] in device memory: a new recording starts in row s with this call).
 * A row with n_s == 0 leaves t_last[s] = carry_s.  t: SAST_DT_I64 / I32 [S, stream_capacity]; t_out int64 [S, stream_capacity], may
 * alias t when t is int64.  The running maximum never crosses from one row into the next. */
int sast_evstreams_correct_time(const void* t, int t_dtype, const int64_t* counts, int S, int64_t stream_capacity, int64_t* t_out,
                                int64_t* t_last, const uint8_t* reset, int64_t* ws, sast_stream_t stream);
/* window w = k * S + s (ends_us int64 [T, S]) over the sorted t[s][0 .. n_s): the search of sast_event_window_bounds inside row s, as
 * absolute indices into the flattened buffer (s * stream_capacity + local).  SAST_EVENT_WINDOW_COUNT clips at the start of the row:
 * start = max(end - value, s * stream_capacity).  bounds: int64 [T * S, 2]. */
int sast_evstreams_window_bounds(const int64_t* t, const int64_t* counts, int S, int64_t stream_capacity, const int64_t* ends_us, int T,
                                 int mode, int64_t value, int64_t* bounds, sast_stream_t stream);

/* sast_evstreams_window_bounds through a row map, for the random-access sampler below (csrc/k_events.hip: the same kernel): window w = k * B + b (ends_us int64 [T, B]) is searched in row rows[b] (int32 [B] in
 * device memory) of the R rows, so a step may hold several windows of one row and rows that no window uses.  A row outside [0, R)
 * gives the empty range [0, 0): sast_event_frames / sast_mdstack_frames, called unchanged with T * B windows over capacity
 * R * stream_capacity, leave that frame zero.  R * stream_capacity <= 2^31 - 1.  bounds: int64 [T * B, 2].  1 launch. */
int sast_rnd_window_bounds(const int64_t* t, const int64_t* counts, int R, int64_t stream_capacity, const int32_t* rows,
                           const int64_t* ends_us, int B, int T, int mode, int64_t value, int64_t* bounds, sast_stream_t stream);

/* ---- event retention across chunks (csrc/k_events.hip): S rows of [S, capacity] storage keep exactly the events that later windows can
 * still need, so a host pushes chunks cut at arbitrary points (a camera's transfer size) and asks for windows as their ends pass.  The
 * reference has no such stage: it reads a whole recording and windows it offline (scripts/genx/preprocess_dataset.py:476-530); the
 * frames here equal what sast_evstreams_* + sast_event_frames give for the whole recording in one buffer.  Row s's live events are
 * storage indices [head[s], count[s]); timestamps are stored corrected (the reader's running maximum, :159-168, carried in t_last[s]).
 * All state is device memory owned by the caller; every per-row size is read on the device and clamped to capacity there; grids are
 * sized from capacities, so the calls replay inside a graph.  Rows never see each other's carry, head or events. */
typedef struct SastEvQueueArgs {
  int16_t* x;               /* retained columns, int16 [S, capacity] (narrowed with saturation: a value outside int16 stays invalid) */
  int16_t* y;
  int16_t* p;
  int64_t* t;               /* corrected timestamps, int64 [S, capacity] */
  int64_t* head;            /* int64 [S] */
  int64_t* count;           /* int64 [S] */
  int64_t* t_last;          /* int64 [S]: the time-correction carry */
  int64_t* retired;         /* int64 [S]: events retired from the row since its last reset */
  int64_t* retired_t;       /* int64 [S]: the corrected time of the last retired event */
  int32_t* err;             /* int32 [4], ACCUMULATED: [0] invalid events, [1] windows over window_capacity (both written by
                               sast_event_frames / sast_mdstack_frames, which take this pointer as their err), [2] events dropped for
                               lack of room, [3] late windows */
  int64_t* ws;              /* int64 [sast_evqueue_ws_count(S)]; no initial contents needed */
  int64_t capacity;         /* events one row holds; S * capacity <= 2^31 - 1 */
  int32_t S;                /* 1 .. 65535 */
  int32_t reserved;
} SastEvQueueArgs;
/* the dtype code of packed records (sast_evqueue_push only): Prophesee's Event2D as the reference reads it, EV_TYPE of
 * utils/evaluation/prophesee/io/dat_events_tools.py:18-50 -- 8 bytes, little-endian: u4 t, then i4 x | y << 14 | p << 28 */
enum { SAST_EVQUEUE_DT_DAT = 6 };

/* int64 elements of SastEvQueueArgs.ws: S * (SAST_EVENT_SCAN_BLOCKS + 6) -- per row the time scan's carry and partial maxima
 * (SAST_EVENT_SCAN_BLOCKS + 1), the append plan (3) and the move plan (2).  0: S < 1 or S > 65535.  Host only. */
size_t sast_evqueue_ws_count(int S);
/* per row s: with reset != NULL and reset[s] != 0 the row is emptied first (head, count, t_last, retired, retired_t = 0).  Then the
 * first n_s = min(max(counts[s], 0), chunk_capacity) events of chunk row s are appended behind count[s], as many as fit
 * (capacity - count[s]; the chunk's first ones); the rest are added to err[2].  The stored timestamps are max(t, carry, the stored
 * timestamps before it in the chunk) with carry = t_last[s] (preprocess_dataset.py:159-168); t_last[s] advances over the stored events.
 * x, y, p: SAST_DT_I64 / I32 / I16 [S, chunk_capacity], t: SAST_DT_I64 / I32.  t_dtype == SAST_EVQUEUE_DT_DAT: t holds int32
 * [S, chunk_capacity, 2] packed records, decoded as load_td_data does (dat_events_tools.py:39-50): t the unsigned word 0 (the 32-bit
 * clock is not unwrapped), x = w & 16383, y = (w >> 14) & 16383, p = (w >> 28) & 1 of word 1, bits 29-31 ignored; x, y, p and their
 * dtypes are then not read.  2 launches (partial maxima; scan + decode + append). */
int sast_evqueue_push(const SastEvQueueArgs* q, const void* x, const void* y, const void* p, const void* t, int x_dtype, int y_dtype,
                      int p_dtype, int t_dtype, const int64_t* counts, int64_t chunk_capacity, const uint8_t* reset, sast_stream_t stream);
/* sast_evstreams_window_bounds (preprocess_dataset.py:507-513) over each row's live events: window w = k * S + s (ends_us int64 [T, S])
 * -> bounds int64 [T * S, 2], indices into the flattened [S * capacity] storage; a count window stops at the row's first live event.
 * A window that needs retired events is added to err[3]: duration -- retired[s] > 0 and retired_t[s] >= end - value; count -- fewer
 * than `value` live events up to the end and retired[s] > 0.  1 launch. */
int sast_evqueue_window_bounds(const SastEvQueueArgs* q, const int64_t* ends_us, int T, int mode, int64_t value, int64_t* bounds,
                               sast_stream_t stream);
/* after the frames of `bounds` (as written by sast_evqueue_window_bounds with the same T): row s keeps its events from the start of
 * its last window, step T - 1; those before it are retired (retired[s], retired_t[s]).  A row whose live events number no more than
 * the slots in front of them is moved to the front of its storage (source and destination disjoint); any other row keeps its place,
 * so capacity >= 2 x (the most live events of a row right after this call) + (the most events pushed to it between two such calls)
 * never drops an event.
 * 2 launches (one thread per row decides and writes the plan; the copy reads only the plan). */
int sast_evqueue_retire(const SastEvQueueArgs* q, const int64_t* bounds, int T, sast_stream_t stream);
/* the scheduler contract (2) of the queue assumes, on the device: which of each row's next W duration windows are due, from the row's
 * carry t_last[s] (call it after sast_evqueue_push on the same stream).  State: next_end int64 [S], the end of the row's next window
 * (first_end_us >= value at the start of a recording).  Per row s, with D = value and e_k = next_end[s] + k * D:
 *   reset != NULL and reset[s] != 0: next_end[s] = first_end_us first (the flags given to the push);
 *   window k is due when t_last[s] > e_k (an event later than its end was pushed), and, with final_flags != NULL and
 *   final_flags[s] != 0 (the recording is over), also while e_k - D < t_last[s]; due is monotone in k: n_all windows are due, n =
 *   min(n_all, W) of them are given by this call;
 *   ends[k * S + s] = e_k for k < n, next_end[s] + (n - 1) * D behind them (the last due end; next_end[s] - D when none is due: the
 *   window the row gave last, so sast_evqueue_window_bounds / sast_evqueue_retire on `ends` retire nothing new and count no late window);
 *   due[k * S + s] = k < n;  backlog[s] = n_all - n;  next_end[s] += n * D.
 * mode must be SAST_EVENT_WINDOW_DURATION and value >= 1 (count windows have no schedule in time: SAST_EINVAL).  ends int64 [W, S],
 * due uint8 [W, S], backlog int64 [S].  1 launch, one thread per row. */
int sast_evq_schedule(const SastEvQueueArgs* q, int64_t* next_end, int mode, int64_t value, int64_t first_end_us, int W,
                          const uint8_t* reset, const uint8_t* final_flags, int64_t* ends, uint8_t* due, int64_t* backlog,
                          sast_stream_t stream);

/* ---- raw sensor words (csrc/k_evt3.hip, a format policy on the decoder driver csrc/evt_dec.cuh): Prophesee EVT 3.0, the 16-bit little-endian word stream IMX636 / GenX320 kits put on the
 * wire by default (other kits of the Gen4 family send EVT 2.0: the next section), decoded on the device into the columns sast_evqueue_push takes.  The reference has no such stage (it reads .dat / .npy
 * files, utils/evaluation/prophesee/io/); the rule below is this project's contract, and parity with the Metavision SDK's decoder is
 * unpinned (the SDK is not a dependency).  type = w >> 12, v = w & 0xFFF; per stream the state y, base_x, vpol, low, high, wraps,
 * have_high, all 0 after a reset:
 *   0x0 EVT_ADDR_Y    y = v & 0x7FF (bit 11 ignored)
 *   0x2 EVT_ADDR_X    one event (x = v & 0x7FF, y, p = v >> 11, t)
 *   0x3 VECT_BASE_X   base_x = v & 0x7FF, vpol = v >> 11
 *   0x4 VECT_12       for every set bit i of v, ascending: an event (base_x + i, y, vpol, t); then base_x += 12
 *   0x5 VECT_8        the same over bits 0..7 (bits 8-11 ignored); then base_x += 8
 *   0x6 EVT_TIME_LOW  low = v
 *   0x8 EVT_TIME_HIGH have_high and high - v >= 2048: wraps += 1; then high = v, have_high = 1
 *   0x7, 0xA, 0xE, 0xF  valid, no effect;   0x1, 0x9, 0xB, 0xC, 0xD  no effect, counted as unknown words
 * t = wraps * 2^24 + high * 4096 + low (microseconds).  An event met while have_high is 0 is not given, it is counted.  Events come
 * out in word order, inside a vector word by ascending bit.  base_x may run past 2047: it stops growing at 2^30, and x is stored as
 * int16 with saturation, so such an event stays outside the sensor (the frame kernels count it invalid).  The state after a chunk is
 * the state before the next one: a stream cut into chunks at any word gives the events, counters and state of the whole stream. */
#define SAST_EVT3_STATE_WORDS 8       /* a row of `state`: y, base_x, vpol, low, high, wraps, have_high, 0 */
#define SAST_EVT3_BLOCK_WORDS 2048    /* words a workgroup takes in one step; a row gets ceil(chunk_words / this) workgroups ... */
#define SAST_EVT3_MAX_BLOCKS 256      /* ... at most this many, which then take several steps each */
/* bytes of the decode's workspace (one summary per row for the state and for every workgroup).  0: S < 1 or S > 65535.  Host only. */
size_t sast_evt3_ws_bytes(int S);
/* per row s: with reset != NULL and reset[s] != 0 the row's state is zeroed first.  Then the first n_s = min(max(counts[s], 0),
 * chunk_words) words of words[s] (16-bit words [S, chunk_words]) are decoded: the events go to x, y, p (int16) and t (int64)
 * [S, max_events] from column 0 on, out_counts[s] = min(events, max_events) (of a row with more, the first max_events are kept),
 * state[s] (int64 [S, SAST_EVT3_STATE_WORDS]) becomes the state after the chunk.  err, int32 [3], ACCUMULATED: [0] events before
 * the first TIME_HIGH, [1] unknown words, [2] events dropped because the row's staging was full.  max_events = 12 * chunk_words never
 * drops.  Row s of the workgroup grid (blocks, S) splits its n_s words into `blocks` pieces of a multiple of 8 words.
 * S * chunk_words and S * max_events <= 2^31 - 1, chunk_words <= (2^31 - 1) / 12, max_events >= 1.  2 launches (one summary per
 * workgroup; fold the summaries in front + decode + write, the row's last workgroup writes state, count and counters): no workgroup
 * reads what another one writes in the same launch, and nothing has to be put back for a graph replay. */
int sast_evt3_decode(const void* words, const int64_t* counts, int64_t chunk_words, int S, const uint8_t* reset, int64_t* state,
                     void* ws, int16_t* x, int16_t* y, int16_t* p, int64_t* t, int64_t max_events, int64_t* out_counts, int32_t* err,
                     sast_stream_t stream);

/* ---- events -> raw sensor words (csrc/k_evt3_enc.hip): the inverse of the section above, event columns (the dtypes of
 * sast_evqueue_push) or packed Event2D records (SAST_EVQUEUE_DT_DAT's layout) -> EVT 3.0 words that sast_evt3_decode turns back into the
 * events.  The rule is canonical and deterministic; it is this project's (parity with the Metavision SDK's encoder is unpinned, the SDK
 * is not a dependency; what is pinned is the sequential model of tests/evt3_encoder_model.py).  Per stream the state have, t_last,
 * y_last, all 0 after a reset.  One row's chunk of n events:
 *   1. normalised: t the running maximum over the row, from t_last when have is set and from 0 otherwise; x and y clamped to
 *      0 .. 2047; p = p != 0.  An event changed by this is counted (err[0]: t raised, err[1]: x, y or p changed), never dropped.
 *   2. groups: event j continues the group of event j - 1 iff both are in this chunk, have the same t, y and p, x[j-1] < x[j] and
 *      x[j-1] / 12 == x[j] / 12; every other event, and a chunk's first, is a leader.  A cut ends a group: the words depend on the cuts,
 *      the decoded events do not.
 *   3. only leaders send words.  Leader i, with "the event in front" the state for i == 0, in this order:
 *        0x8 EVT_TIME_HIGH  !have: (t >> 12) & 0xFFF.  Else, with H = t >> 12 and Hp = t_front >> 12: floor((H - Hp - 1) / 1024) keep-alives
 *                           (Hp + 1024 q) & 0xFFF, q = 1 .., so that the decoder sees every wrap of the 12 bits; then H & 0xFFF if H != Hp
 *        0x6 EVT_TIME_LOW   t & 0xFFF, behind every TIME_HIGH (a decoder that clears the low bits there still agrees), or when the low
 *                           bits differ from those of the event in front
 *        0x0 EVT_ADDR_Y     y, bit 11 clear: !have, or y differs from the y in front
 *        a group of two or more events:
 *        0x3 VECT_BASE_X    12 * (x / 12) | p << 11 -- unless the group is chained: events i - 2 and i - 1 are in this chunk and end a
 *                           group, i - 1 -> i is ascending with the same t, y, p and x[i] / 12 == x[i-1] / 12 + 1: the decoder's base
 *                           and polarity already stand there
 *        0x4 VECT_12        one bit x % 12 per member
 *        a single event:
 *        0x2 EVT_ADDR_X     x | p << 11
 *      No VECT_8, CONTINUED, OTHERS or trigger word is sent.  Without keep-alives an event gives at most 5 words.
 *   4. the state after the chunk is (1, t, y) of its last event; an empty chunk leaves it alone.
 * A fresh decoder starts with wraps = 0: it returns t - ((t0 >> 24) << 24), t0 the row's first event.  That is the format's. */
#define SAST_EVT3_ENC_STATE_WORDS 4     /* a row of `state`: have, t_last, y_last, 0 */
#define SAST_EVT3_ENC_BLOCK_EVENTS 1024 /* events a workgroup takes in one step; a row gets ceil(chunk_events / this) workgroups ... */
#define SAST_EVT3_ENC_MAX_BLOCKS 256    /* ... at most this many, which then take several steps each */
/* bytes of the encode's workspace (per row the state and one summary per workgroup).  0: S < 1 or S > 65535.  Host only. */
size_t sast_evt3enc_ws_bytes(int S);
/* per row s: with reset != NULL and reset[s] != 0 the row's state is zeroed first.  Then the first n_s = min(max(counts[s], 0),
 * chunk_events) events of row s are encoded: x, y, p SAST_DT_I64 / I32 / I16 [S, chunk_events], t SAST_DT_I64 / I32.  The words go to
 * words[s] (16-bit words [S, max_words]) from column 0 on, n_words[s] is their number, state[s] (int64 [S, SAST_EVT3_ENC_STATE_WORDS])
 * becomes the state after the chunk.  A row whose words exceed max_words is refused whole (the rule of sast_evmerge_append):
 * n_words[s] = 0, its state as it was (zero if its reset flag was set), one count in err[2], nothing in err[0] and err[1].  err, int32 [4], ACCUMULATED: [0] times
 * raised to the running maximum, [1] events whose x, y or p was clamped, [2] rows refused for lack of room, [3] spare.
 * max_words = 5 * chunk_events + (the keep-alives: one per 2^22 us of silence) never refuses.  SAST_EINVAL before any launch: a null
 * pointer (reset may be), S outside 1 .. 65535, an unknown dtype, chunk_events < 0, S * chunk_events or S * max_words > 2^31 - 1,
 * max_words < 1, words not 2-byte or ws not 8-byte aligned.
 * 2 launches whatever S and the sizes are (one summary per workgroup: words, largest t, raised and clamped events; fold the summaries +
 * scan + write, the row's last workgroup writes state, n_words and counters): no workgroup reads what another one writes in the same
 * launch, nothing has to be put back for a graph replay, every store is a plain vector store.  A row with a raised time (unsorted
 * input, counted in err[0]) is walked whole by its last workgroup: the normalised times of a piece then depend on every event before. */
int sast_evt3enc_encode(const void* x, const void* y, const void* p, const void* t, int x_dtype, int y_dtype, int p_dtype, int t_dtype,
                     const int64_t* counts, int64_t chunk_events, int S, const uint8_t* reset, int64_t* state, void* ws, void* words,
                     int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream);
/* the same from packed records: int32 [S, chunk_events, 2], Prophesee's Event2D as sast_evqueue_push takes it with
 * SAST_EVQUEUE_DT_DAT (t the unsigned word 0, x = w & 16383, y = (w >> 14) & 16383, p = (w >> 28) & 1 of word 1); records 8-byte
 * aligned.  DAT -> EVT 3.0 without an unpacked copy. */
int sast_evt3enc_encode_dat(const void* records, const int64_t* counts, int64_t chunk_events, int S, const uint8_t* reset, int64_t* state,
                         void* ws, void* words, int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream);

/* ---- raw sensor words, EVT 2.0 and EVT 2.1 (csrc/k_evt2.hip): the 32-bit word stream the VGA (Gen3.1) and 720p Gen4 / Gen4.1
 * evaluation kits send by default (one word is at most one event), and the 64-bit word stream IMX636 / GenX320 kits can be set to
 * (one word is a 32-pixel vector), decoded on the device into the columns sast_evqueue_push takes.  As for EVT 3.0 the rule below is
 * this project's contract: parity with the Metavision SDK's decoder is unpinned (the SDK is not a dependency); what is pinned is the
 * sequential model of tests/evt2_model.py.  Per stream the state high, wraps, have_high, all 0 after a reset.
 * EVT 2.0, 32-bit little-endian words, type = w >> 28:
 *   0x0 CD_OFF, 0x1 CD_ON   one event (x = (w >> 11) & 0x7FF, y = w & 0x7FF, p = type, t) with ts6 = (w >> 22) & 0x3F
 *   0x8 EVT_TIME_HIGH       v = w & 0x0FFFFFFF; have_high and high - v >= 2^27: wraps += 1; then high = v, have_high = 1
 *   0xA EXT_TRIGGER, 0xE OTHERS, 0xF CONTINUED  valid, no effect;   0x2-0x7, 0x9, 0xB, 0xC, 0xD  no effect, counted as unknown words
 * EVT 2.1, 64-bit little-endian words, type = w >> 60:
 *   0x0 EVT_NEG, 0x1 EVT_POS   ts6 = (w >> 54) & 0x3F, x_base = (w >> 43) & 0x7FF, y = (w >> 32) & 0x7FF, valid = w & 0xFFFFFFFF: for
 *                              every set bit i of valid, ascending, an event (x_base + i, y, p = type, t); valid == 0 gives nothing
 *   0x8 EVT_TIME_HIGH          v = (w >> 32) & 0x0FFFFFFF, then as in EVT 2.0;   every other type as in EVT 2.0
 * t = wraps * 2^34 + high * 64 + ts6 (microseconds).  A TIME_HIGH lower than its predecessor by less than 2^27 is taken as written:
 * time steps back (the queue's running maximum holds it).  An event met while have_high is 0 is not given, it is counted.  Events
 * come out in word order, inside an EVT 2.1 word by ascending bit.  x_base + i can reach 2078 and is stored as written: such an event
 * stays outside the sensor (the frame kernels count it invalid).  An EVT 2.1 word is the 64-bit little-endian integer; a stream whose
 * 32-bit halves arrive in the other order is the caller's to swap.  The state after a chunk is the state before the next one: a
 * stream cut into chunks at any word gives the events, counters and state of the whole stream. */
#define SAST_EVT2_V20 0
#define SAST_EVT2_V21 1
#define SAST_EVT2_STATE_WORDS 4       /* a row of `state`: high, wraps, have_high, 0 */
#define SAST_EVT2_THREAD_WORDS 4      /* words a thread takes in one step: a row's pieces are multiples of this */
#define SAST_EVT2_BLOCK_WORDS 1024    /* words a workgroup takes in one step; a row gets ceil(chunk_words / this) workgroups ... */
#define SAST_EVT2_MAX_BLOCKS 256      /* ... at most this many, which then take several steps each */
/* bytes of the decode's workspace (one summary per row for the state and for every workgroup).  0: S < 1 or S > 65535.  Host only. */
size_t sast_evt2_ws_bytes(int S);
/* per row s: with reset != NULL and reset[s] != 0 the row's state is zeroed first.  Then the first n_s = min(max(counts[s], 0),
 * chunk_words) words of words[s] (version SAST_EVT2_V20: 32-bit words, SAST_EVT2_V21: 64-bit words, [S, chunk_words]) are decoded:
 * the events go to x, y, p (int16) and t (int64) [S, max_events] from column 0 on, out_counts[s] = min(events, max_events) (of a row
 * with more, the first max_events are kept), state[s] (int64 [S, SAST_EVT2_STATE_WORDS]) becomes the state after the chunk.  err,
 * int32 [3], ACCUMULATED, with the meaning and order of sast_evt3_decode: [0] events before the first TIME_HIGH, [1] unknown words,
 * [2] events dropped because the row's staging was full.  max_events = chunk_words (2.0) or 32 * chunk_words (2.1) never drops.
 * SAST_EINVAL before any launch: a null pointer, S outside 1 .. 65535, an unknown version, chunk_words < 0, S * chunk_words or
 * S * max_events > 2^31 - 1, for 2.1 chunk_words > (2^31 - 1) / 32, max_events < 1, words not aligned to its word size.  Loads are
 * 16 bytes wide when words and every row of it are 16-byte aligned.  2 launches (one summary per workgroup; fold the summaries in
 * front + decode + write, the row's last workgroup writes state, count and counters): no workgroup reads what another one writes in
 * the same launch, and nothing has to be put back for a graph replay.  The chunking rule and the two launches are those of
 * sast_evt3_decode (the driver, csrc/evt_dec.cuh, is shared). */
int sast_evt2_decode(const void* words, const int64_t* counts, int64_t chunk_words, int S, int version, const uint8_t* reset,
                     int64_t* state, void* ws, int16_t* x, int16_t* y, int16_t* p, int64_t* t, int64_t max_events, int64_t* out_counts,
                     int32_t* err, sast_stream_t stream);

/* ---- events -> raw sensor words, EVT 2.0 and EVT 2.1 (csrc/k_evt2_enc.hip): the inverse of the section above, event columns (the
 * dtypes of sast_evqueue_push) or packed Event2D records (SAST_EVQUEUE_DT_DAT's layout) -> EVT 2.0 / 2.1 words that sast_evt2_decode
 * turns back into the events.  The contract, the chunking rule and the two launches are those of sast_evt3enc_encode (the driver,
 * csrc/evt_enc.cuh, is shared).  The rule is canonical and deterministic; it is this project's (parity with the Metavision SDK's
 * encoder is unpinned, the SDK is not a dependency; what is pinned is the sequential model of tests/evt2_encoder_model.py).  Per
 * stream the state have, t_last, all 0 after a reset.  One row's chunk of n events:
 *   1. normalised: t the running maximum over the row, from t_last when have is set and from 0 otherwise; x and y clamped to
 *      0 .. 2047; p = p != 0.  An event changed by this is counted (err[0]: t raised, err[1]: x, y or p changed), never dropped.
 *   2. groups: EVT 2.0: every event is a leader.  EVT 2.1: event j continues the group of event j - 1 iff both are in this chunk, have
 *      the same t, y and p, x[j-1] < x[j] and x[j-1] >> 5 == x[j] >> 5; every other event, and a chunk's first, is a leader.  A group
 *      has at most 32 members.  A cut ends a group: the words depend on the cuts, the decoded events do not.
 *   3. only leaders send words.  Leader i, with "the event in front" the state for i == 0, H = t >> 6 and Hp = t_front >> 6, in
 *      this order:
 *        0x8 EVT_TIME_HIGH  (2.0: value in bits 0..27; 2.1: value in bits 32..59)  !have: H & 0x0FFFFFFF.  have and H > Hp:
 *                           floor((H - Hp - 1) / 2^26) keep-alives (Hp + 2^26 q) & 0x0FFFFFFF, q = 1 .., then H & 0x0FFFFFFF: two
 *                           neighbouring TIME_HIGHs are 1 .. 2^26 steps apart, so the decoder's high - v >= 2^27 test sees every
 *                           wrap of the 28 bits exactly once.  No TIME_HIGH otherwise
 *        the event word, type p (0x0 / 0x1), ts6 = t & 63:
 *          EVT 2.0  ts6 in bits 22..27, x in bits 11..21, y in bits 0..10
 *          EVT 2.1  one 64-bit little-endian word: ts6 in bits 54..59, x_base = 32 * (x >> 5) in bits 43..53 (as a sensor aligns it:
 *                   never past column 2047), y in bits 32..42, valid = one bit x & 31 per member
 *      No EXT_TRIGGER, OTHERS or CONTINUED word is sent.  Without keep-alives an event gives at most 2 words.
 *   4. the state after the chunk is (1, t) of its last event; an empty chunk leaves it alone.
 * A fresh decoder starts with wraps = 0: it returns t - ((t0 >> 34) << 34), t0 the row's first event.  That is the format's 34-bit
 * clock. */
#define SAST_EVT2_ENC_STATE_WORDS 4     /* a row of `state`: have, t_last, 0, 0 */
#define SAST_EVT2_ENC_BLOCK_EVENTS 1024 /* events a workgroup takes in one step; a row gets ceil(chunk_events / this) workgroups ... */
#define SAST_EVT2_ENC_MAX_BLOCKS 256    /* ... at most this many, which then take several steps each */
/* bytes of the encode's workspace (per row the state and one summary per workgroup).  0: S < 1 or S > 65535.  Host only. */
size_t sast_evt2enc_ws_bytes(int S);
/* as sast_evt3enc_encode, with version SAST_EVT2_V20 / SAST_EVT2_V21: per row s, with reset != NULL and reset[s] != 0 the row's state
 * is zeroed first.  Then the first n_s = min(max(counts[s], 0), chunk_events) events of row s are encoded: x, y, p SAST_DT_I64 / I32 /
 * I16 [S, chunk_events], t SAST_DT_I64 / I32.  The words go to words[s] (2.0: 32-bit words, 2.1: 64-bit words, [S, max_words]) from
 * column 0 on, n_words[s] is their number, state[s] (int64 [S, SAST_EVT2_ENC_STATE_WORDS]) becomes the state after the chunk.  A row
 * whose words exceed max_words is refused whole: n_words[s] = 0, its state as it was (zero if its reset flag was set), one count in
 * err[2], nothing in err[0] and err[1].  err, int32 [4], ACCUMULATED: [0] times raised to the running maximum, [1] events whose x, y
 * or p was clamped, [2] rows refused for lack of room, [3] spare.  max_words = 2 * chunk_events + (the keep-alives: one per 2^32 us
 * of silence) never refuses.  SAST_EINVAL before any launch: a null pointer (reset may be), S outside 1 .. 65535, an unknown version
 * or dtype, chunk_events < 0, S * chunk_events or S * max_words > 2^31 - 1, max_words < 1, words not aligned to its word size, ws not
 * 8-byte aligned.
 * 2 launches whatever S and the sizes are (one summary per workgroup: words, largest t, raised and clamped events; fold the summaries +
 * scan + write, the row's last workgroup writes state, n_words and counters): no workgroup reads what another one writes in the same
 * launch, nothing has to be put back for a graph replay, every store is a plain vector store.  A row with a raised time (unsorted
 * input, counted in err[0]) is walked whole by its last workgroup: the normalised times of a piece then depend on every event before. */
int sast_evt2enc_encode(const void* x, const void* y, const void* p, const void* t, int x_dtype, int y_dtype, int p_dtype, int t_dtype,
                        const int64_t* counts, int64_t chunk_events, int S, int version, const uint8_t* reset, int64_t* state, void* ws,
                        void* words, int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream);
/* the same from packed records: int32 [S, chunk_events, 2], Prophesee's Event2D as sast_evqueue_push takes it with
 * SAST_EVQUEUE_DT_DAT (t the unsigned word 0, x = w & 16383, y = (w >> 14) & 16383, p = (w >> 28) & 1 of word 1); records 8-byte
 * aligned.  DAT -> EVT 2.0 / 2.1 without an unpacked copy. */
int sast_evt2enc_encode_dat(const void* records, const int64_t* counts, int64_t chunk_events, int S, int version, const uint8_t* reset,
                            int64_t* state, void* ws, void* words, int64_t max_words, int64_t* n_words, int32_t* err,
                            sast_stream_t stream);

/* ---- event noise filters (csrc/k_evfilter.hip): the two standard event-level filters between decode and accumulate, on the device.
 * The rule is this project's (parity with the Metavision SDK's ActivityNoiseFilterAlgorithm / SpatioTemporalContrastAlgorithm is
 * unpinned, the SDK is not a dependency; what is pinned is the sequential model of tests/event_filter_model.py).  Per stream row s,
 * over the events in arrival order:
 *   t'_i = max(t_last[s], t_0 .. t_i), the queue's running-maximum correction, carried in the filter's own t_last[s]; 0 <= t' < 2^62.
 *   surface[s, y, x] (int64) is -1 while the pixel has seen no event since the last reset, else 2 * t'_j + (p_j > 0) of the LAST event
 *   by arrival order at that pixel.  Every event inside the sensor writes it, kept or not: the state never depends on a decision.
 *   SAST_EVFILTER_ACTIVITY, radius r in 1 .. 3: event i is kept iff some pixel q != (x_i, y_i) inside the sensor within Chebyshev
 *     distance r holds, as events 0 .. i-1 left it, a value v >= 0 with t'_i - (v >> 1) <= threshold_us.  Polarity plays no part.
 *   SAST_EVFILTER_CONTRAST: event i is kept iff its own pixel holds, as events 0 .. i-1 left it, v >= 0 with (v & 1) == (p_i > 0)
 *     and t'_i - (v >> 1) <= threshold_us.
 *   An event with x outside 0 .. width-1 or y outside 0 .. height-1 is never kept, writes nothing and is counted in err[0]; it still
 *   advances t'.  The kept events leave in arrival order: x, y, p as they came (int16, p saturated), t = t'.
 * The decision for an event depends on earlier EVENTS only, never on earlier decisions, so a chunk is decided at once: one device
 * radix sort (rocprim) of the unique keys (row * H * W + pixel) << index_bits | flat index over the fixed capacity S * chunk_capacity
 * (slots that hold no event inside the sensor carry the key S * H * W << index_bits | flat index and sort behind); the predecessor of
 * event i at pixel q is a lower bound in the sorted keys, the surface from before the call where the chunk has none; the last key of
 * each pixel's run writes the surface; the kept events are compacted per row in order.  A recording cut into calls anywhere (empty
 * chunks included) gives the events and the state of the recording in one call. */
enum { SAST_EVFILTER_ACTIVITY = 0, SAST_EVFILTER_CONTRAST = 1 };
#define SAST_EVFILTER_BLOCK_EVENTS 1024 /* slots a workgroup takes in one step; a row gets ceil(chunk_capacity / this) workgroups ... */
#define SAST_EVFILTER_MAX_BLOCKS 256    /* ... at most this many, which then take several steps each */
#define SAST_EVFILTER_LAUNCHES 4        /* the library's own launches of one call; the radix sort's passes come on top */
typedef struct SastEvFilterArgs {
  int64_t* surface;         /* int64 [S, height, width]: -1, or 2 * t' + pbit of the pixel's last event */
  int64_t* t_last;          /* int64 [S]: the time-correction carry */
  int64_t* seen;            /* int64 [S]: events taken in, cumulative (those outside the sensor included) */
  int64_t* kept;            /* int64 [S]: events kept, cumulative */
  int32_t* err;             /* int32 [1], ACCUMULATED: [0] events outside the sensor */
  void* ws;                 /* sast_evfilter_ws_bytes(S, chunk_capacity, height, width) bytes or more, 8-byte aligned */
  size_t ws_bytes;
  int16_t* x;               /* the kept events, [S, out_capacity] from column 0 on */
  int16_t* y;
  int16_t* p;
  int64_t* t;
  int64_t* out_counts;      /* int64 [S]: the kept events of this call */
  int64_t out_capacity;     /* >= chunk_capacity */
  int64_t threshold_us;     /* 0 .. 2^62 - 1 */
  int32_t S;                /* 1 .. 65535 */
  int32_t height;           /* 1 .. 32767 */
  int32_t width;
  int32_t mode;             /* SAST_EVFILTER_ACTIVITY / SAST_EVFILTER_CONTRAST */
  int32_t radius;           /* 1 .. 3 (activity; contrast does not read it) */
  int32_t reserved;
} SastEvFilterArgs;
/* bytes of the call's workspace (keys, sorted keys, surface values and keep flags of S * chunk_capacity slots, per-workgroup
 * summaries, the radix sort's own storage).  0 for shapes the filter does not take: S outside 1 .. 65535, height or width outside
 * 1 .. 32767, chunk_capacity < 0, S * chunk_capacity > 2^31 - 1, or keys that do not fit 63 bits.  Host only. */
size_t sast_evfilter_ws_bytes(int S, int64_t chunk_capacity, int height, int width);
/* per row s: with reset != NULL and reset[s] != 0 the row's surface is set to -1 and t_last[s], seen[s], kept[s] to 0 first (only
 * the workgroups of such rows sweep their H * W words).  Then the first n_s = min(max(counts[s], 0), chunk_capacity) events of row s
 * are filtered: x, y, p SAST_DT_I64 / I32 / I16 [S, chunk_capacity], t SAST_DT_I64 / I32.  A row with n_s == 0 and no reset flag is
 * untouched (out_counts[s] = 0).  SAST_EINVAL before any launch: a null pointer (reset may be), a shape sast_evfilter_ws_bytes
 * refuses, ws too small or misaligned, out_capacity < chunk_capacity or S * out_capacity > 2^31 - 1, an unknown mode or dtype, radius
 * outside 1 .. 3, threshold_us outside 0 .. 2^62 - 1.  SAST_ELAUNCH: a launch failed.
 * SAST_EVFILTER_LAUNCHES launches and one radix sort whose passes depend on the shapes alone (partial time maxima + reset sweep;
 * corrected times, keys and values; the sort; decisions; compaction + surface + state).  No workgroup reads what another one writes in
 * the same launch, every store is a plain vector store, results are bit-identical from run to run, nothing is allocated and nothing
 * synchronises: the call replays inside a graph. */
int sast_evfilter_apply(const SastEvFilterArgs* f, const void* x, const void* y, const void* p, const void* t, int x_dtype, int y_dtype,
                        int p_dtype, int t_dtype, const int64_t* counts, int64_t chunk_capacity, const uint8_t* reset,
                        sast_stream_t stream);
/* the same from packed records: int32 [S, chunk_capacity, 2], Prophesee's Event2D as sast_evqueue_push takes it with
 * SAST_EVQUEUE_DT_DAT (t the unsigned word 0, x = w & 16383, y = (w >> 14) & 16383, p = (w >> 28) & 1 of word 1); records 8-byte
 * aligned. */
int sast_evfilter_apply_dat(const SastEvFilterArgs* f, const void* records, const int64_t* counts, int64_t chunk_capacity,
                            const uint8_t* reset, sast_stream_t stream);

/* ---- label front end (csrc/k_labels.hip): the raw Prophesee box records of S recordings side by side -> the filtered labels, the
 * label-frame timestamps, the window-end schedule, the frame -> window map and per-step label tensors, all on the device.  The reference
 * does this offline, per recording: apply_filters, get_base_delta_ts_for_labels_us and labels_and_ev_repr_timestamps of
 * scripts/genx/preprocess_dataset.py:191-428, then ObjectLabelFactory (data/genx_utils/labels.py:149-198).  Every integer equals the
 * reference's, every fp32 value bit for bit.
 * records: int32 [S, capacity, 10], the 40-byte BBOX_DTYPE record of utils/evaluation/prophesee/io/box_loading.py:19-21 as ten
 * little-endian words: 0-1 t (int64, us), 2-5 the bits of fp32 x, y, w, h, 6 class_id (u32), 7 track_id (ignored), 8 class_confidence
 * (fp32), 9 padding.  counts: int64 [S], the records at the head of each row, sorted by t; clamped to [0, capacity] on the device.
 * status bits of a row (SastLabelArgs.status, set by sast_labels_load; a row with any bit but FRAME_OVERFULL / WINDOW_INDEX has
 * n_frames = n_windows = 0): */
enum {
  SAST_LABELS_UNSORTED = 1,            /* a record's t is smaller than its predecessor's */
  SAST_LABELS_NEGATIVE_SIZE = 2,       /* a record with w < 0 or h < 0 (the reference asserts) */
  SAST_LABELS_NO_LABELS = 4,           /* no record survives the filters (NoLabelsException), or the row is empty */
  SAST_LABELS_BAD_RATE = 8,            /* base_delta_us == 0: fewer than two unique timestamps, or a label rate that is not 30 / 60 Hz */
  SAST_LABELS_NO_ALIGNED_LABEL = 16,   /* no label at or after align_t_us */
  SAST_LABELS_ZERO_COUNT = 32,         /* a timestamp within 2 ms of the last label frame (the reference asserts) */
  SAST_LABELS_TOO_MANY_FRAMES = 64,    /* more than max_frames label frames */
  SAST_LABELS_TOO_MANY_WINDOWS = 128,  /* more than max_windows window ends */
  SAST_LABELS_FRAME_OVERFULL = 256,    /* a label frame with more than max_labels_per_frame boxes: cut to its first ones */
  SAST_LABELS_FRAMES_TOO_CLOSE = 512,  /* two label frames <= 98 000 us apart (the reference asserts) */
  SAST_LABELS_WINDOW_INDEX = 1024      /* sast_labels_gather was given a window index outside [0, n_windows) */
};
typedef struct SastLabelArgs {
  void* ws;                  /* sast_labels_ws_bytes(S, capacity, max_frames) bytes, 8-byte aligned; no initial contents needed */
  int64_t* ends_us;          /* [S, max_windows] window ends */
  int32_t* n_windows;        /* [S] */
  int64_t* frame_ts_us;      /* [S, max_frames] label-frame timestamps */
  int32_t* n_frames;         /* [S] */
  int64_t* frame_2_window;   /* [S, max_frames] searchsorted(ends_us, frame_ts_us, 'left') */
  int32_t* window_2_frame;   /* [S, max_windows] its inverse; -1: not a label frame */
  float* labels;             /* [S, capacity, 7] (t, x, y, w, h, class_id, class_confidence) of the label frames' boxes, in frame order */
  int32_t* frame_start;      /* [S, max_frames] first row of a frame in `labels` */
  int32_t* frame_count;      /* [S, max_frames] its rows (<= max_labels_per_frame) */
  int32_t* status;           /* [S] */
  int64_t capacity;          /* records one row holds; S * capacity <= (2^31 - 1) / 16 */
  int64_t base_delta_us;     /* the label period: 250 000 (gen1), or 0 for gen4's rule -- np.median of the differences of the unique
                                timestamps in fp64, hz = rint(1e6 / median) in {30, 60}, int(6 * median) or int(3 * median) */
  int64_t align_t_us;        /* the first label frame is the first unique timestamp >= this */
  int64_t delta_t_us;        /* ts_step_ev_repr_ms * 1000: the step of the windows before the first label frame */
  int32_t S;                 /* 1 .. 65535 */
  int32_t width, height;     /* the sensor: 304 x 240 (gen1), 1280 x 720 (gen4) */
  int32_t class_max;         /* keep class_id <= class_max (gen4: 2); < 0: no class filter */
  float min_diag2;           /* > 0: keep w * w + h * h >= min_diag2 (prophesee_bbox_filter); 0: no diagonal rule */
  float min_side;            /* keep w >= min_side and h >= min_side (10 / 20, or conservative_bbox_filter's 5) */
  float max_width;           /* >= 0: keep w <= max_width (remove_faulty_huge_bbox_filter, train split); < 0: off */
  int32_t reprs_per_frame;   /* 100 / ts_step_ev_repr_ms: windows per 100 ms */
  int32_t downsample_by_2;   /* ObjectLabels.scale_(0.5) and its removal of flat boxes */
  int32_t max_frames, max_windows, max_labels_per_frame;
  int32_t reserved;
} SastLabelArgs;
/* bytes of SastLabelArgs.ws; 0: an argument out of range.  Host only. */
size_t sast_labels_ws_bytes(int S, int64_t capacity, int max_frames);
/* once per recording and row: row s with reset == NULL or reset[s] != 0 is rebuilt from records row s, any other row is left as it
 * is.  Filters (stable), unique timestamps, base delta, the sequential acceptance of label frames (count = rint(diff / base) in fp64,
 * |diff - count * base| <= 2000), window ends (the lead-in f0 - k * delta_t_us, then numpy's linspace per pair of label frames in fp64
 * truncated to int64), frame_2_window and its inverse, and the labels of the accepted frames through clamp_to_frame_ (and scale_).
 * 1 launch, one 1024-thread workgroup per row; the grid depends on S alone, every count is read on the device. */
int sast_labels_load(const SastLabelArgs* a, const int32_t* records, const int64_t* counts, const uint8_t* reset, sast_stream_t stream);
/* window_idx int64 [T, S] -> labels fp32 [T, S, max_labels_per_frame, 7] (a frame's rows at the front, zeros behind), counts int32
 * [T, S], ends_us int64 [T, S], labelled uint8 [T, S] (1: the window is a label frame, even when all its boxes vanished in the
 * downscale).  An index outside [0, n_windows[s]): counts 0, ends_us -1, labelled 0, and SAST_LABELS_WINDOW_INDEX in status[s].
 * 1 launch. */
int sast_labels_gather(const SastLabelArgs* a, const int64_t* window_idx, int T, float* labels, int32_t* counts, int64_t* ends_us,
                       uint8_t* labelled, sast_stream_t stream);

/* ---- random-access sampler (csrc/k_sampler.hip): training sequences that end at a label frame, over the R = SastLabelArgs.S rows
 * sast_labels_load has filled.  The reference does this on the CPU: SequenceForRandomAccess (data/genx_utils/sequence_rnd.py:9-75),
 * torch's ConcatDataset, get_most_recent_objframe (data/utils/augmentor.py:367-378) and get_weighted_random_sampler
 * (data/genx_utils/dataset_rnd.py:115-149).  Integers equal the reference's, the fp64 weights equal it bit for bit.  With
 * f2w = frame_2_window[r][0 .. n_frames[r]):  start_idx_offset[r] = the first j with f2w[j] - sequence_length + 1 >= 0, or n_frames[r];
 * length[r] = n_frames[r] - start_idx_offset[r];  cum[0] = 0, cum[r + 1] = cum[r] + length[r].  Item g of the N = cum[R] items lies in
 * the row with cum[r] <= g < cum[r + 1]; its label frame is j = g - cum[r] + start_idx_offset[r], its windows are
 * f2w[j] + 1 - sequence_length ... f2w[j].  Every size is read on the device and every index clamped there; the grids are sized from
 * R, B, sequence_length, max_frames and max_classes, so the calls replay inside a graph.
 * status bits (SastRndArgs.status, int32 [R + 1]: one word per row, then one for the pool), cleared by sast_rnd_index: */
enum {
  SAST_RND_CLASS_ID = 1,               /* row r: a box of a counted label frame has a class id outside [0, max_classes); left out */
  SAST_RND_ITEM_INDEX = 2              /* word R: sast_rnd_gather was given an item outside [0, N) */
};
typedef struct SastRndArgs {
  int32_t* start_idx_offset; /* [R] */
  int32_t* length;           /* [R] */
  int64_t* cum;              /* [R + 1] */
  int64_t* class_total;      /* [max_classes]: boxes per class over all items (weighted only; zeroed otherwise) */
  double* weights;           /* [R * max_frames]: the weight of item g at [g], 0 behind N; may be NULL unless weighted */
  int32_t* status;           /* [R + 1] */
  int32_t* ticket;           /* [1], zero before the first call; every call leaves it zero */
  int32_t sequence_length;   /* 1 .. 65535 */
  int32_t only_load_end_labels; /* label frames of the last step only (the others read as unlabelled) */
  int32_t max_classes;       /* 1 .. 256 */
  int32_t weighted;          /* also class_total and weights */
} SastRndArgs;
/* start_idx_offset, length, cum (1 launch: a workgroup per row, the last one to finish scans the lengths); weighted: per item the
 * boxes per class over the label frames of its windows (only_load_end_labels: of its last window), class_total their sum over all
 * items (int64 atomics), weight = sum over c ascending of (1.0 / max(class_total[c], 1)) * count[c] in fp64, one rounding per
 * operation, starting from 0 (2 more launches, a workgroup per possible item). */
int sast_rnd_index(const SastLabelArgs* a, SastRndArgs* q, sast_stream_t stream);
/* items int64 [B] (device) -> rows int32 [B], window_idx / ends_us int64 [L, B], labels fp32 [L, B, M, 7], counts int32 [L, B],
 * labelled uint8 [L, B] (L = sequence_length, M = max_labels_per_frame; per (step, sample) what sast_labels_gather gives for row
 * rows[b] at that window; only_load_end_labels: steps before the last have counts 0, labelled 0 and zero rows), latest fp32 [B, M, 7]
 * / latest_count int32 [B]: the rows of the sample's last step with counts > 0, or 0.  An item outside [0, N): rows -1, window_idx
 * and ends_us -1, counts, labelled, latest_count 0, zero rows, SAST_RND_ITEM_INDEX in status[R].  1 launch, a workgroup per
 * (step, sample). */
int sast_rnd_gather(const SastLabelArgs* a, const SastRndArgs* q, const int64_t* items, int B, int32_t* rows, int64_t* window_idx,
                    int64_t* ends_us, float* labels, int32_t* counts, uint8_t* labelled, float* latest, int32_t* latest_count,
                    sast_stream_t stream);

/* ---- streaming sampler (csrc/k_stream.hip): the streamed half of `sampling: 'mixed'` over the R = SastLabelArgs.S rows sast_labels_load
 * has filled.  The reference does this on the CPU: _get_ev_repr_range_indices, SequenceForIter.get_sequences_with_guaranteed_labels,
 * __init__ and __getitem__ (data/genx_utils/sequence_for_streaming.py:21-181) and the per-batch-row concatenations of
 * ConcatStreamingDataPipe / ShardedStreamingDataPipe (data/utils/stream_concat_datapipe.py, stream_sharded_datapipe.py).  With
 * f2w = frame_2_window[r][0 .. n_frames[r]) and L = sequence_length:  guarantee_labels = 1 -- a new sub-sequence begins at frame 0 and at
 * every frame j with f2w[j] - f2w[j - 1] > L; sub-sequence (first frame a, last frame b) covers the windows
 * [max(f2w[a] - L + 1, 0), f2w[b] + 1).  guarantee_labels = 0 -- one sequence per row, [max(f2w[0] - L + 1, 0), n_windows[r]).  A row
 * without frames has no sequence.  Sequences are numbered row-major, in ascending window order inside a row; sequence s has
 * seq_samples[s] = ceil((seq_stop[s] - seq_start[s]) / L) samples; step k of sample i is window seq_start[s] + i * L + k, padded when
 * that window is >= seq_stop[s].  Every size is read on the device and every index clamped there; the grids are sized from R and B, no
 * kernel waits for another workgroup and none keeps a word between calls, so the calls replay inside a graph.
 * status bits (SastStreamArgs.status, int32 [1], pool-wide), cleared by sast_stream_index: */
enum {
  SAST_STREAM_TRUNCATED = 1,           /* more than max_sequences sequences: the table holds the first max_sequences */
  SAST_STREAM_SCHEDULE_INDEX = 2       /* sast_stream_next met a schedule entry outside [0, n_seq): a fully padded sample, then skipped */
};
typedef struct SastStreamArgs {
  int32_t* seq_row;          /* [max_sequences] the recording of a sequence */
  int32_t* seq_start;        /* [max_sequences] its first window */
  int32_t* seq_stop;         /* [max_sequences] one past its last window */
  int32_t* seq_samples;      /* [max_sequences] */
  int32_t* row_first_seq;    /* [R + 1]: row r's sequences are row_first_seq[r] .. row_first_seq[r + 1] - 1 */
  int32_t* row_count;        /* [R]: scratch between the two launches of sast_stream_index; no initial contents needed */
  int32_t* n_seq;            /* [1] */
  int32_t* status;           /* [1] */
  int32_t* order;            /* [B, order_capacity]: batch row b walks the sequences order[b][0 .. order_len[b]) (sast_stream_next only) */
  int32_t* order_len;        /* [B] */
  int32_t* cursor;           /* [B, 2]: (position in order[b], sample inside that sequence); zero starts the schedule */
  int32_t sequence_length;   /* 1 .. 65535 */
  int32_t guarantee_labels;  /* 0 / 1 */
  int32_t max_sequences;     /* >= 1 */
  int32_t order_capacity;    /* >= 1; B * order_capacity <= 2^31 - 1 */
} SastStreamArgs;
/* seq_row, seq_start, seq_stop, seq_samples, row_first_seq, n_seq.  More than max_sequences sequences: the first max_sequences are
 * kept and SAST_STREAM_TRUNCATED is set.  2 launches, a workgroup per row: the rows' sequence counts; then every row sums the counts
 * in front of it and writes its sequences.  order, order_len and cursor are not read. */
int sast_stream_index(const SastLabelArgs* a, const SastStreamArgs* q, sast_stream_t stream);
/* one sample per batch row b, at cursor[b], then cursor[b] moves on by one sample: rows / seq / sample int32 [B], is_first / exhausted
 * uint8 [B], step_rows int32 [L, B] (the row on a real step, -1 on a padded one: the row map of sast_rnd_window_bounds with B' = L * B,
 * T = 1), window_idx / ends_us int64 [L, B] (-1 on padded steps), labels fp32 [L, B, M, 7], counts int32 [L, B], labelled uint8 [L, B]
 * (per real step what sast_labels_gather gives for that row and window; zeros on padded steps), is_padded uint8 [L, B].  A row whose
 * schedule is used up: rows, seq, sample -1, is_first 0, exhausted 1, every step padded, the cursor stays.  A schedule entry outside
 * [0, n_seq): the same with exhausted 0, SAST_STREAM_SCHEDULE_INDEX is set and the cursor moves to the next entry.  1 launch, a
 * workgroup per batch row; no workgroup reads what another one writes. */
int sast_stream_next(const SastLabelArgs* a, const SastStreamArgs* q, int B, int32_t* rows, int32_t* step_rows, int32_t* seq, int32_t* sample,
                     uint8_t* is_first, uint8_t* exhausted, int64_t* window_idx, int64_t* ends_us, float* labels, int32_t* counts,
                     uint8_t* labelled, uint8_t* is_padded, sast_stream_t stream);

/* ---- mixed sampler (csrc/k_mixed.hip): the merged batch of `sampling: 'mixed'`.  The reference splits the batch size into streamed and
 * random-access rows (set_mixed_sampling_mode_variables_for_train, modules/data/genx.py:116-129), concatenates the two loaders' batches
 * along the batch axis, stream rows first (merge_mixed_batches, modules/utils/detection.py:133-161), and trains on the result in one
 * step.  With B = Bs + Br every output is laid out [L, B, ...] / [B]:
 *   columns [0, Bs):  exactly what sast_stream_next(a, qs, Bs, ...) writes for batch row b -- the cursor advance, the padded tail, the
 *     exhausted row and the schedule entry out of range with SAST_STREAM_SCHEDULE_INDEX in qs->status included;
 *   columns [Bs, B):  exactly what sast_rnd_gather(a, qr, items, Br, ...) writes for items[b - Bs] -- only_load_end_labels and the item
 *     outside [0, N) with SAST_RND_ITEM_INDEX in qr->status[R] included -- and in the fields only the streaming sampler has: step_rows
 *     the sample's row at every step (-1 for an item outside [0, N)), seq and sample -1, is_first 1, exhausted 0, is_padded 0.
 * latest fp32 [Br, M, 7] and latest_count int32 [Br] are sast_rnd_gather's.  step_rows and ends_us are the row map and the window ends
 * of ONE sast_rnd_window_bounds call over the union batch (B' = L * B, T = 1).  qs and qr must have the same sequence_length.
 * 1 launch: workgroups [0, Bs) each walk a streamed row's L steps, the other Br * L each take one (step, random sample); the two
 * bodies are the ones sast_stream_next and sast_rnd_gather run (csrc/sampler_rows.cuh).  No workgroup reads what another one writes,
 * nothing is kept between calls but the stream cursors, every size is read on the device and every index clamped there: the call
 * replays inside a graph. */
int sast_mixed_next(const SastLabelArgs* a, const SastStreamArgs* qs, const SastRndArgs* qr, int Bs, const int64_t* items, int Br, int32_t* rows,
                    int32_t* step_rows, int32_t* seq, int32_t* sample, uint8_t* is_first, uint8_t* exhausted, int64_t* window_idx,
                    int64_t* ends_us, float* labels, int32_t* counts, uint8_t* labelled, uint8_t* is_padded, float* latest,
                    int32_t* latest_count, sast_stream_t stream);
/* the look-ahead of the merged loop (csrc/k_sampler.hip, whose state it reads; named here because the sast_rnd_ family is closed):
 * items int64 [B] (device) -> latest fp32 [B, M, 7] and latest_count int32 [B] alone, bit for bit what sast_rnd_gather writes there for
 * the same items (an item outside [0, N): zero rows, latest_count 0 and SAST_RND_ITEM_INDEX in q->status[R]).  It fetches the label
 * frames zoom-in is placed on one step before the batch that uses them.  1 launch, a workgroup per sample. */
int sast_mixed_latest(const SastLabelArgs* a, const SastRndArgs* q, const int64_t* items, int B, float* latest, int32_t* latest_count,
                      sast_stream_t stream);

/* ---- spatial augmentation of event frames and box labels (csrc/k_augment.hip).  The reference augments on the CPU in its data-loader
 * workers: RandomSpatialAugmentorGenX.__call__ (data/utils/augmentor.py:347-364) -- horizontal flip, then zoom-in (:203-222) or zoom-out
 * (:134-153) -- with the label transforms of ObjectLabels (data/genx_utils/labels.py:255-339).  Both calls read the per-sample
 * parameters from DEVICE memory: int32 [B][SAST_AUGMENT_PARAM_WORDS], frame n uses sample n % B (frames are [T, B, ...]), so a captured
 * graph is replayed with new parameters by rewriting that tensor.  Words of one sample:
 *   0 flip (0 / 1)   1 mode (SAST_AUGMENT_NONE / ZOOM_IN / ZOOM_OUT)   2 x0   3 y0   4 window height   5 window width   6, 7 reserved
 *   8..11  fp32 bits: zoom-in clamp bounds of the labels  x lo, x hi, y lo, y hi  (z_x0, z_x1 - 1, z_y0, z_y1 - 1 of labels.py:272-281)
 *   12..14 fp32 bits: the multiplier of scale_ and its clamps  s, s * width' - 1, s * height' - 1  (labels.py:323-327)   15 reserved
 * The host computes 8..14 in double as the reference's Python does and rounds each to fp32 once; the kernels repeat the reference's
 * single fp32 operations in its order, so frames are equal byte for byte and box coordinates bit for bit.  The caller validates the
 * parameters (zoom-in: 0 <= x0 < W, 0 <= y0 < H;  zoom-out: x0 + window width <= W, y0 + window height <= H;  windows >= 1); the
 * kernels clamp every index they form all the same. */
#define SAST_AUGMENT_PARAM_WORDS 16
enum { SAST_AUGMENT_NONE = 0, SAST_AUGMENT_ZOOM_IN = 1, SAST_AUGMENT_ZOOM_OUT = 2 };

/* in, out: uint8 [N, C, H, W], distinct buffers;  H, W <= 4096, N, C <= 65535.  One launch, one pass: out[n, c, y, x] =
 * in[n, c, sy(y), W - 1 - sx(x)] (sx(x) without flip), zero outside the zoom-out window (written by the same kernel).  The source index
 * is ATen's nearest-exact one in fp32: min(int(floorf((d + 0.5f) * (float(in) / float(out)))), in - 1).  W a multiple of 16 with both
 * bases 16-byte aligned takes the 16-byte load / store path, anything else a byte path with the same result. */
int sast_augment_frames(const uint8_t* in, uint8_t* out, const int32_t* params, int N, int B, int C, int H, int W, sast_stream_t stream);
/* labels: fp32 [N, M, 7] rows (t, x, y, w, h, class_id, class_confidence) (labels.py:13-21), counts: int32 [N] valid rows at the head of
 * each frame (0: the reference's None).  out / counts_out: the same layout, the rows that survive remove_flat_labels_ compacted to the
 * front in their order, the rest zero.  yolox (may be NULL): fp32 [N, M, 5] = (class_id, x + 0.5 w, y + 0.5 h, w, h) of the same rows
 * (labels.py:341-355), zero after the count.  W: the frame width (flip_lr_).  out and counts_out must not alias the inputs. */
int sast_augment_labels(const float* labels, const int32_t* counts, const int32_t* params, int N, int B, int M, int W, float* out,
                        int32_t* counts_out, float* yolox, sast_stream_t stream);

/* the same augmentation with rotation (csrc/k_rotaug.hip): flip, then rotate, then zoom-in or zoom-out, the reference's order
 * (augmentor.py:355-363).  Named sast_rotaug_ because the sast_augment_ family is closed at the two entry points above (their set of
 * names and SAST_AUGMENT_PARAM_WORDS are pinned by tests); the rotation parameters live in a SECOND device tensor read beside `params`:
 * rot_params int32 [B][SAST_ROTAUG_PARAM_WORDS], frame n uses row n % B.  Words of one sample:
 *   0 active (0 / 1)   1..4 fp32 bits of a, b, c, d (frames)   5, 6 fp32 bits of cos, sin (labels)   7 reserved
 * A sample with active == 0 gets exactly what sast_augment_frames / sast_augment_labels give it.
 * Frames: torchvision's tensor rotate (NEAREST, expand=False, center=None, fill=None: affine_grid + grid_sample, align_corners=False)
 * restated with one fp32 rounding per operation.  Host, for angle_deg: r = radians(-angle_deg) in double; m = (cos r, sin r, -sin r,
 * cos r), each rounded to fp32 once; then in fp32 a = m0 / f32(0.5 W), b = m1 / f32(0.5 W), c = m2 / f32(0.5 H), d = m3 / f32(0.5 H).
 * Device, for pixel (y, x) of the rotated image, every operation rounded to nearest:
 *   bx = (float)x + (0.5f - 0.5f * W),  by = (float)y + (0.5f - 0.5f * H)          (exact)
 *   gx = (bx * a) + (by * b),  gy = (bx * c) + (by * d)                             (no FMA)
 *   ix = (((gx + 1) * W) - 1) / 2,  iy = (((gy + 1) * H) - 1) / 2
 *   sx = rintf(ix),  sy = rintf(iy)  (ties to even: grid_sample's nearbyint);  inside iff 0 <= sx < W && 0 <= sy < H, else the pixel is 0.
 * It is a nearest gather: bytes are copied.  torch's own matrix product need not round the same way on every build, so the contract is
 * this rule (tests/augment_rotation_model.py), not byte equality with torch; parity with torchvision's rotate itself is unpinned
 * (torchvision is not a dependency).
 * Labels: ObjectLabels.rotate_ (labels.py:210-248) after flip_lr_, before the zooms.  Host: cos, sin of angle_deg / 180 * pi in double,
 * each rounded to fp32 once.  Device, with cx = W / 2, cy = H / 2 (integer division: NOT the frames' centre (W - 1) / 2; the reference
 * is inconsistent here and that is kept), for each corner (X, Y) of (x | x + w, y | y + h), the sums fp32 adds:
 *   px = X - cx,  py = Y - cy;   rx = ((cos * px) + (sin * py)) + cx;   ry = ((-sin * px) + (cos * py)) + cy
 * then min and max over the corners, clamped to [0, W - 1] and [0, H - 1], w = x1 - x0, h = y1 - y0, the box kept iff w > 0 && h > 0.
 * This is the plain (unfused) form torch's CPU einsum computes for small frames; for frames of 64 boxes and more torch switches to a
 * fused form that differs by up to 1.3e-4 px. */
#define SAST_ROTAUG_PARAM_WORDS 8
/* in, out, params: as sast_augment_frames.  One launch for all N frames, rotated or not: out[n, c, y, x] = in[n, c, ry, W - 1 - rx] (rx
 * without flip) with (ry, rx) the rotation map of (sy(y), sx(x)); 0 on the zoom-out border and where the rotation map leaves the frame.
 * The source pixels of a 64 x 64 output tile are computed once and reused for its channels; per channel the box that holds them is
 * staged in LDS (or, where it does not fit, read from global memory); no atomics, no workspace.  W a multiple of 16 takes 16-byte
 * stores where out is 16-byte aligned and 16-byte loads where in is; anything else a byte path with the same result. */
int sast_rotaug_frames(const uint8_t* in, uint8_t* out, const int32_t* params, const int32_t* rot_params, int N, int B, int C, int H, int W,
                       sast_stream_t stream);
/* as sast_augment_labels, with H (rotate_ needs the frame height) and rot_params. */
int sast_rotaug_labels(const float* labels, const int32_t* counts, const int32_t* params, const int32_t* rot_params, int N, int B, int M, int H,
                       int W, float* out, int32_t* counts_out, float* yolox, sast_stream_t stream);

/* ---- Prophesee mAP evaluation of detections (csrc/k_eval.hip).  The reference converts every validation step's labels and detections
 * to numpy (to_prophesee, utils/evaluation/prophesee/io/box_loading.py:58-99), buffers them in PropheseeEvaluator and at epoch end runs
 * filter_boxes (io/box_filtering.py), _match_times / _to_coco_format (metrics/coco_eval.py) and pycocotools' COCOeval (bbox, useCats,
 * maxDets 100).  Here the buffer lives on the device: sast_eval_add filters, flattens and MATCHES the frames it is given (COCOeval.evaluate
 * is per image) and appends one record per kept detection; sast_eval_accumulate sorts the records and computes COCOeval.accumulate /
 * summarize.  Nothing synchronises with the host; what does not fit a capacity is counted in the state words, never dropped silently.
 *   state  int32 [SAST_EVAL_STATE_WORDS]: 0 images, 1 ground-truth rows, 2 detection rows, 3 records, 4..7 records per category,
 *          8 frames refused for max_images, 9 for max_detections, 10 for max_labels_per_frame, 11 sast_eval_add calls since the reset,
 *          12..27 non-ignored ground truths [K][4], 28 images refused for sast_evrec_add's max_window, 29 rows it refused as unsorted
 *   tables gt_box fp32 [max_images * max_labels_per_frame][4] (x, y, w, h), gt_cls / gt_img int32; det_box fp32 [max_detections][5]
 *          (x, y, w, h, score), det_cls / det_img int32; img_t int64 [max_images]: image i is the i-th frame that kept a label
 *   records rec_key / rec_match / rec_ign uint64 [max_detections]: bit (area * 10 + threshold) of match / ignore; key = category << 62 |
 *          ~(order-preserving bits of the score) << 30 | record index.  rec_ign bits 40..46: the detection's rank (0 .. 99) in its
 *          (image, category) group after the stable descending sort on the score -- what a cut to maxDets 1 or 10 needs
 *          (sast_evsum_accumulate); lanes 40..63 set no match or ignore bit, and only bits 0..39 of either word enter a result.
 *          sast_evmerge_append copies both words whole, so the rank travels with a merged, exported or gathered buffer
 *   precision fp64 [10][101][K][4] (COCOeval.eval['precision'] at maxDets 100), result fp64 [8 + SAST_EVAL_STATE_WORDS]: AP, AP_50, AP_75,
 *          AP_S, AP_M, AP_L, 2 unused, then the state words
 * iou_thr: the 10 doubles of np.linspace(.5, .95, 10); rec_thr: the 101 of np.linspace(0, 1, 101).  A <= 8192, max_labels_per_frame <= 128,
 * K <= 4, max_detections < 2^30.
 * sast_eval_accumulate cuts every category's sorted records into chunks of SAST_EVAL_ACC_CHUNK records (a knob of the registry below,
 * default 1024, honoured as an exact count >= 1) and walks the chunks in parallel: counts per chunk, a scan over the chunks, the
 * precision maximum per chunk, a suffix maximum, and a backward walk per chunk that writes the recall thresholds first reached inside it.
 * All counts are integers, every precision and recall is the one fp64 division of the sequential walk, the envelope is a maximum: the
 * table does not depend on the chunk length, bit for bit.  The per-chunk partials (1 KiB per chunk) live in sort_ws after the sort:
 * sast_eval_sort_ws_bytes returns the larger of the sort's and the chunks' need AT THE KNOB'S CURRENT VALUE, and sast_eval_accumulate
 * refuses (SAST_EINVAL) a sort_ws_bytes below it -- a host that changes the knob asks for the size again.
 * sast_evmerge_append(dst, src) appends the buffer `src` to `dst` on the device: afterwards dst is what it would be had it been fed
 * src's frames after its own (src is left as it was).  Images, img_t, ground-truth rows, detection rows and records are appended, gt_img /
 * det_img grow by dst's image count, the index bits of rec_key by dst's record count (the index breaks score ties: dst's records keep
 * going first), state words 0-7, 11 and 12-27 are added, and so are src's own refusal counters 8-10, 28 and 29.  All counts are read on the device (two
 * launches, no host synchronisation, replayable in a graph).  All or nothing: when src's images, ground-truth rows, detections or records
 * do not fit what is left of dst's max_images, max_images * max_labels_per_frame or max_detections, nothing is appended and src's image
 * count is added to dst's refusal word of every capacity that was exceeded (8, 10, 9 in that order of capacities).  Refused on the host
 * (SAST_EINVAL): null pointers, dst == src or one state for both, differing K / min_diag2 / min_side, src->max_labels_per_frame >
 * dst->max_labels_per_frame.  Only the capacities, K, the filter and the state / table / record pointers of the two are read. */
#define SAST_EVAL_STATE_WORDS 32
#define SAST_EVAL_MAX_CLASSES 4
#define SAST_EVAL_IOU_THRS 10
#define SAST_EVAL_REC_THRS 101
#define SAST_EVAL_AREAS 4
typedef struct {
  const float* labels;    /* [N, M, 7] (t, x, y, w, h, class_id, class_confidence) */
  const int32_t* counts;  /* [N] valid rows; 0: not a frame */
  const float* det;       /* [N, A, 7] (x1, y1, x2, y2, obj_conf, class_conf, class_pred): sast_postprocess's out */
  const int32_t* n_det;   /* [N] */
  int32_t N, M, A, K;
  float min_diag2, min_side; /* filter_boxes: w*w + h*h >= min_diag2, w >= min_side, h >= min_side */
  int32_t max_images, max_labels_per_frame;
  int64_t max_detections;
  int32_t* state;
  int32_t* info;          /* scratch of one add: int32 [N][16] */
  float* gt_box; int32_t* gt_cls; int32_t* gt_img; int64_t* img_t;
  float* det_box; int32_t* det_cls; int32_t* det_img;
  uint64_t* rec_key; uint64_t* rec_match; uint64_t* rec_ign;
  const double* iou_thr; const double* rec_thr;
  uint64_t* sorted;       /* [max_detections] */
  void* sort_ws; size_t sort_ws_bytes; /* sast_eval_sort_ws_bytes(max_detections) */
  double* precision; double* result;
} SastEvalArgs;
int sast_eval_reset(const SastEvalArgs* a, sast_stream_t stream);
int sast_eval_add(const SastEvalArgs* a, sast_stream_t stream);
size_t sast_eval_sort_ws_bytes(int64_t max_detections);
int sast_eval_accumulate(const SastEvalArgs* a, sast_stream_t stream);
int sast_evmerge_append(const SastEvalArgs* dst, const SastEvalArgs* src, sast_stream_t stream);

/* ---- the whole of COCOeval.accumulate / summarize at maxDets [1, 10, 100] (csrc/k_eval.hip): the tables of COCOeval.eval and the
 * twelve numbers of COCOeval.stats.  sast_evsum_accumulate runs BEHIND sast_eval_accumulate on the same stream and buffer: it reads the
 * `sorted` array that call leaves, the records and the state, and writes only what SastEvSumArgs names (buf->precision, buf->result
 * and buf->sort_ws are not touched).
 *   kept     for maxDet m an image contributes its first m detections per category: the records of rank < m (rec_ign bits 40..46).
 *            They are a subsequence of the sorted order, so there is no second sort: a record of rank >= m counts as ignored in every
 *            lane, and the chunk walk of sast_eval_accumulate (count, scan, maximum, envelope, walk) runs once more with the maxDet
 *            as a second grid dimension.  The m = 100 slice of `precision` is buf->precision bit for bit
 *   recall   [t][k][a][m]: the true positives at the category's right edge / the non-ignored ground truths; 0 when the category has
 *            no record, -1 when it has no non-ignored ground truth
 *   scores   [t][r][k][a][m]: the fp32 score, widened, of the record at which recall threshold r is first reached (where the walk
 *            writes the precision entry), recovered from the score bits of the sort key (a score of -0 reads +0); 0 where the
 *            threshold is never reached, -1 where precision is -1.  Threshold 0 is reached at the category's first kept record
 *            whether or not it is ignored in that area range (np.searchsorted, side='left'): sorted[start] for every m
 *   stats    COCOeval.stats: AP, AP_50, AP_75, AP_S, AP_M, AP_L (m = 100), AR_1, AR_10, AR_100 (all areas), AR_S, AR_M, AR_L (m = 100),
 *            each the mean over the entries > -1 of its slice or -1; the first six are buf->result[0..5] bit for bit
 *   per_class [k][4]: AP, AP_50, AP_75 and AR_100 of category k alone over all areas at m = 100, by the same rule
 * No table depends on SAST_EVAL_ACC_CHUNK, bit for bit.  Six launches, no host synchronisation, every grid sized from max_detections
 * and K.  ws: sast_evsum_ws_bytes(max_detections) bytes AT THE KNOB'S CURRENT VALUE (3 KiB per chunk), 8-byte aligned, no initial
 * contents needed.  Refused on the host (SAST_EINVAL): null pointers, a buffer sast_eval_accumulate would refuse, ws misaligned or
 * ws_bytes too small. */
#define SAST_EVSUM_MAXDETS 3
#define SAST_EVSUM_STATS 12
typedef struct {
  double* precision;       /* [10][101][K][4][3] */
  double* scores;          /* [10][101][K][4][3] */
  double* recall;          /* [10][K][4][3] */
  double* stats;           /* [12] */
  double* per_class;       /* [K][4] */
  void* ws; size_t ws_bytes;
} SastEvSumArgs;
size_t sast_evsum_ws_bytes(int64_t max_detections);   /* 0: max_detections out of range.  Host only. */
int sast_evsum_accumulate(const SastEvalArgs* buf, const SastEvSumArgs* sum, sast_stream_t stream);

/* ---- whole recordings into the evaluation buffer (csrc/k_eval.hip): the Prophesee protocol itself, one label file against one
 * detection file per recording -- evaluate_list(apply_bbox_filters=True) (evaluation.py:5-42) and evaluate_detection's loop over files
 * with _match_times (metrics/coco_eval.py:42-90).  gt / dt: int32 [S, Gcap, 10] / [S, Dcap, 10], the 40-byte BBOX_DTYPE records as ten
 * words (the layout sast_labels_load takes and sast_detections_export writes), the first n_gt[s] / n_dt[s] (int64, clamped to the
 * capacity on the device) of a row valid and sorted by t.  Per row, in row order:
 *   filter   a record passes when t > 500 000, w*w + h*h >= min_diag2, w >= min_side and h >= min_side (fp32, as sast_eval_add); labels
 *            and detections alike, each detection on its own t;
 *   images   the unique t of the passing labels, ascending; an image's ground truth is the passing labels of that t in record order,
 *            its detections the passing detections with t - time_tol_us <= t_det <= t + time_tol_us in record order (a detection
 *            inside several windows is a result row and a record in each); x, y, w, h, class_confidence and class_id are taken from
 *            the record as they are;
 *   then     sast_eval_add's cut to 100 per (image, category), IoU, matching and records: the same kernels, instantiated on record
 *            ranges instead of padded frames.  The two calls may be mixed in one buffer; both count in state word 11.
 * Refusals, counted in the state and never silent: max_images and max_detections (memberships) per image as for sast_eval_add;
 * max_labels_per_frame per timestamp, on the passing labels; an image whose window holds more than max_window records BEFORE the filter
 * (1 <= max_window <= 8192: it sizes the LDS sort) in word 28; a row whose valid records are not sorted by t, labels or detections,
 * adds nothing and counts in word 29.
 * 4 launches, no host synchronisation, every grid sized from S, Gcap and K: (1) one workgroup per row -- the sorted check and the row's
 * image starts, compacted by a workgroup scan; (2) one wave per image slot -- the two binary searches, the counts; (3) one thread -- the
 * offsets, walking the images of the rows in order (not the S * Gcap slots); (4) one wave per (image slot, category) -- tables and
 * matching.  Refused on the host (SAST_EINVAL): null pointers, S outside 1 .. 65535, Gcap or Dcap < 1, S * Gcap > (2^31 - 1) / 16,
 * S * Dcap > 2^31 - 1, max_window outside 1 .. 8192, time_tol_us < 0, gt / dt not 8-byte aligned, ws_bytes < sast_evrec_ws_bytes. */
typedef struct {
  const int32_t* gt;       /* [S, Gcap, 10] */
  const int64_t* n_gt;     /* [S] */
  const int32_t* dt;       /* [S, Dcap, 10] */
  const int64_t* n_dt;     /* [S] */
  int32_t S, Gcap, Dcap, max_window;
  int64_t time_tol_us;
  void* ws;                /* scratch of one call, sast_evrec_ws_bytes(S, Gcap) bytes; no initial contents needed */
  size_t ws_bytes;
} SastEvRecArgs;
size_t sast_evrec_ws_bytes(int S, int Gcap);   /* 0: an argument out of range.  Host only. */
int sast_evrec_add(const SastEvalArgs* buf, const SastEvRecArgs* rec, sast_stream_t stream);

/* ---- detections as Prophesee box records (csrc/k_eval.hip): what to_prophesee (io/box_loading.py:81-97) makes of one frame's
 * post-processed detections on the host, written on the device for the S rows of one online step.  A record is 40 bytes, little-endian:
 *   offset 0 int64 t (the window end), 8 fp32 x = x1, 12 fp32 y = y1, 16 fp32 w = x2 - x1, 20 fp32 h = y2 - y1 (one fp32 subtraction
 *   each), 24 uint32 class_id (column 6), 28 uint32 track_id = 0, 32 fp32 class_confidence (column 5), 36 four zero bytes.
 * Row s with due[s] != 0: the first m = min(n_det[s], max_det) rows of det[s] (already by decreasing score) become records
 * [s][0 .. m), counts[s] = m, and *truncated += n_det[s] - m.  Any other row: counts[s] = 0.  No row of det past n_det[s] is read
 * (they are uninitialised), no record past counts[s] is written.  1 launch, one wave per row. */
typedef struct {
  const float* det;        /* [S, A, 7] (x1, y1, x2, y2, obj_conf, class_conf, class_pred): sast_postprocess's out */
  const int32_t* n_det;    /* [S] */
  const int64_t* ends;     /* [S]: the rows' window ends */
  const uint8_t* due;      /* [S] */
  uint8_t* records;        /* [S, max_det, 40], 8-byte aligned */
  int32_t* counts;         /* [S] */
  int32_t* truncated;      /* [1], ACCUMULATED */
  int32_t S, A, max_det, reserved;
} SastDetExportArgs;
#define SAST_DET_RECORD_BYTES 40
int sast_detections_export(const SastDetExportArgs* a, sast_stream_t stream);
/* the detection log of an online run: what sast_evrec_add takes as dt / n_dt.  Row s appends the counts[s] (clamped to [0, max_det])
 * records sast_detections_export wrote for one step behind its log_counts[s] records and raises the count.  A step's records that do not
 * fit the row's capacity are dropped WHOLE and *dropped += 1; a row with counts[s] == 0 is left alone.  1 launch, one wave per row. */
typedef struct {
  const uint8_t* records;  /* [S, max_det, 40] of one step, 8-byte aligned */
  const int32_t* counts;   /* [S] */
  int32_t* log;            /* [S, capacity, 10], 8-byte aligned */
  int64_t* log_counts;     /* [S] */
  int32_t* dropped;        /* [1], ACCUMULATED */
  int64_t capacity;
  int32_t S, max_det;
} SastDetLogArgs;
int sast_detlog_append(const SastDetLogArgs* a, sast_stream_t stream);

/* ---- track ids for the exported detections (csrc/k_track.hip): a greedy IoU tracker without a motion model, one launch per online
 * step, between sast_detections_export and sast_detlog_append.  The reference has no tracker: the rule below is this project's own,
 * pinned by the sequential model tests/tracker_model.py; parity with any external tracker is not claimed.
 * State per stream s (device memory, the caller's): T = max_tracks slots -- ids int32 [S, T] (0: a free slot), box fp32 [S, T, 4]
 * (x, y, w, h), cls int32 [S, T], last_t int64 [S, T], hits int32 [S, T]; a FREE slot is zero in all five -- next_id int32 [S] (1 at
 * the start) and counters int32 [4], ACCUMULATED: 0 detections that found no free slot, 1 runs cut by max_det (sast_tracker_run),
 * 2 unsorted rows (sast_tracker_run), 3 reserved.
 * One step of row s, in this order:
 *   1 reset    reset[s] != 0: every slot of the row is freed and next_id[s] = 1, whether or not the row is due.
 *   2 due      due[s] == 0: nothing else of the row is read or written.  Otherwise t = ends[s], m = clamp(counts[s], 0, max_det); only
 *              the first m records of the row are read.
 *   3 expire   a live slot with t - last_t > max_age_us (int64, no wrap-around) is freed; a t that went backwards expires nothing.
 *   4 pairs    (live slot i, detection j) with equal class id (any class with class_agnostic != 0) is a candidate when its IoU passes:
 *              fp32, one rounding per operation (the file is built with -ffp-contract=off, the division is the correctly rounded one):
 *              ax2 = ax + aw, ay2, bx2, by2 likewise; iw = max(0, min(ax2, bx2) - max(ax, bx)), ih likewise, min and max giving NaN
 *              when either side is NaN; inter = iw * ih; uni = aw * ah + bw * bh - inter (left to right); iou = inter / uni if
 *              uni > 0, else 0; candidate if and only if iou >= iou_thre is true.  A box with a NaN is never a candidate.
 *   5 match    greedy over the candidates in the strict total order (IoU descending, detection index ascending, slot ascending): the
 *              first remaining pair is taken, its slot and its detection leave.  Matched slot: box := the detection's (x, y, w, h),
 *              last_t := t, hits += 1 (cls stays).  Matched record: its track_id word (offset 28) := ids[s, i].
 *   6 birth    the unmatched detections in index order: class_confidence >= new_score_thre and a free slot left (slots freed in 3
 *              count) -> the lowest free slot gets ids = next_id[s]++, hits = 1 and the detection's box, class and t, and the record the
 *              id; class_confidence >= new_score_thre and no free slot -> track_id = 0 and counter 0 is raised; otherwise (a NaN
 *              confidence too) track_id = 0 and nothing is counted.
 *   7 nothing else: unmatched live slots stay as they are (only time frees them), no other byte of a record and nothing at or past
 *              record m is touched.
 * Ids are unique within a row between two resets; wrap-around after 2^31 births is not handled.
 * The kernel does not run min(T, m) dependent argmax rounds: the order is strict, so the greedy matching equals repeated rounds in which
 * every live slot and every detection pick their best remaining candidate (one 64-bit maximum over the key IoU bits | ~detection |
 * ~slot) and the pairs that chose each other are fixed.  IoUs are recomputed, not kept: LDS holds 32 bytes per detection (box, class,
 * best key, match) and 40 per slot.  One workgroup of 256 threads per stream.
 * sast_tracker_step: 1 launch, no allocation, no synchronisation.  sast_tracker_run: whole recordings, records int32 [S, Dcap, 10] with
 * the first n[s] (int64, clamped to [0, Dcap]) of a row valid and sorted by t.  Every row starts from the reset state (its table is
 * cleared first, also when the row is then refused), a step is a maximal run of equal t, the runs are walked in order under the rule
 * above and the final table is left behind: the result is what sast_tracker_step gives on the same runs one call at a time.  A run
 * longer than max_det: its records past the first max_det get track_id = 0 and counter 1 is raised once.  A row whose t decreases
 * anywhere keeps every track_id word it had and raises counter 2.  1 launch, one workgroup per row.
 * Refused on the host (SAST_EINVAL, no launch): null pointers (reset may be), S outside 1 .. 65535, max_tracks outside 1 ..
 * SAST_TRACK_MAX_TRACKS, max_det outside 1 .. SAST_TRACK_MAX_DET (32 bytes of LDS per detection: 56 KiB), max_tracks * max_det >
 * SAST_TRACK_MAX_PAIRS (the pairs one round of the matching sweeps), iou_thre not in (0, 1], a NaN new_score_thre, max_age_us < 0,
 * records or last_t not 8-byte aligned, box not 16-byte aligned (a slot's box moves as one 16-byte word), Dcap < 1 or
 * S * Dcap > 2^31 - 1. */
#define SAST_TRACK_MAX_TRACKS 128
#define SAST_TRACK_MAX_DET 1792
#define SAST_TRACK_MAX_PAIRS 65536
typedef struct {
  int32_t* ids;            /* [S, max_tracks] */
  float* box;              /* [S, max_tracks, 4] */
  int32_t* cls;            /* [S, max_tracks] */
  int64_t* last_t;         /* [S, max_tracks] */
  int32_t* hits;           /* [S, max_tracks] */
  int32_t* next_id;        /* [S] */
  int32_t* counters;       /* [4], ACCUMULATED */
  int32_t S, max_tracks, max_det, class_agnostic;
  float iou_thre, new_score_thre;
  int64_t max_age_us;
} SastTrackerArgs;
typedef struct {
  uint8_t* records;        /* [S, max_det, 40] of one step (sast_detections_export's), 8-byte aligned */
  const int32_t* counts;   /* [S] */
  const int64_t* ends;     /* [S] */
  const uint8_t* due;      /* [S] */
  const uint8_t* reset;    /* [S] or NULL */
} SastTrackStepArgs;
typedef struct {
  int32_t* records;        /* [S, Dcap, 10], 8-byte aligned */
  const int64_t* n;        /* [S] */
  int64_t Dcap;
} SastTrackRunArgs;
int sast_tracker_step(const SastTrackerArgs* tr, const SastTrackStepArgs* step, sast_stream_t stream);
int sast_tracker_run(const SastTrackerArgs* tr, const SastTrackRunArgs* run, sast_stream_t stream);

/* ---- tracking metrics (csrc/k_trackeval.hip): the CLEAR-MOT counts (Bernardin and Stiefelhagen) of tracked detections against labelled
 * tracks, for S whole recordings in the record form of sast_evrec_add: gt int32 [S, Gcap, 10] / n_gt int64 [S] and dt int32
 * [S, Dcap, 10] / n_dt int64 [S] (counts clamped to [0, cap] on the device), both sorted by t.  Word 7 of a record, track_id, is what
 * this section reads: the label's is the ground-truth track, the detection's the hypothesis id sast_tracker_step / sast_tracker_run
 * wrote.  The rule below is pinned by the sequential model tests/tracking_eval_model.py; parity with py-motmetrics and TrackEval is
 * not pinned (neither is installed where this project is built).  Recordings are independent.  One recording, in this order:
 *   1 sorted   a label or detection record whose t is below its predecessor's: the row adds nothing and word SAST_TE_UNSORTED is raised.
 *   2 filter   both sides pass filter_boxes exactly as sast_evrec_add applies it: t > 500 000 (each record on its own t) and
 *              w * w + h * h >= min_diag2, w >= min_side, h >= min_side (fp32, one rounding per operation).  Of the records that
 *              pass: a detection with track_id == 0 is dropped (SAST_TE_UNTRACKED), then a record of either side with class_id >= K
 *              is dropped (SAST_TE_BAD_CLASS).
 *   3 frames   every unique t of the labels left is a frame.  Its hypotheses are the records left of ONE detection run (a maximal
 *              sequence of equal t in the detection records before the filter, as in sast_tracker_run): the run whose t is nearest
 *              the frame's, the earlier one on a tie, if |t_run - t| <= time_tol_us; no such run: no hypotheses.  On either side,
 *              in record order, a record whose track_id an earlier record left of the frame carries is dropped (SAST_TE_DUP_GT,
 *              SAST_TE_DUP_HYP).  A frame with more than max_labels_per_frame labels or max_hyp_per_frame hypotheses then, or a
 *              recording with more than max_gt_tracks distinct label ids, refuses the whole row: it adds nothing and raises
 *              SAST_TE_REFUSED_LABELS / _HYP / _TRACKS (once per row, for the first reason met).
 *   4 valid    a pair (label o, hypothesis h) is valid when the class ids are equal (any classes with class_agnostic != 0) and
 *              iou >= iou_thre is true, the IoU being the tracker's ("track ids", step 4: fp32, one rounding per operation, NaN never
 *              passes; the label is the first box).  Its cost is the fp64 1.0 - (double)iou.
 *   5 match    carry-over first, in record order of the labels: a track whose last matched hypothesis id last[o] (the last ever,
 *              across gaps) is not 0 keeps that pair when the id is in the frame, no earlier label has kept it, and the pair is
 *              valid.  The labels and hypotheses left are matched by the optimal assignment: of all matchings of valid pairs those
 *              with the most pairs, of these the one with the least cost sum (where that is not unique, any of them).
 *   6 count    per matched pair, to the label's class: matches += 1, sum_iou += (double)iou; idsw += 1 when last[o] is neither 0 nor
 *              h; frag += 1 when o was matched before but not in the previous frame that held it; then last[o] = h.  An unmatched
 *              label: fn += 1 (its class); an unmatched hypothesis: fp += 1 (ITS class).  gt and hyp count the labels and
 *              hypotheses of the frames by their own class.
 *   7 tracks   at the end, per label id with `present` frames and `matched` of them matched: mostly tracked when 5 * matched >=
 *              4 * present, mostly lost when 5 * matched < present, partially tracked otherwise; the track's class is that of its
 *              first record left.
 * Output of a call: rows int64 [S, K + 1, SAST_TRACKEVAL_COLS] (the columns below; row K is the sum over the classes, and `frames`
 * is the recording's frame count in every row), rows_iou fp64 [S, K + 1] (sum_iou; row K is rows 0 .. K - 1 added in that order) and
 * rows_diag int64 [S, SAST_TRACKEVAL_DIAG] (the words below, per occurrence in a frame; a refused or unsorted row: its reason 1, every
 * other word and every count 0), all overwritten; then acc, acc_iou and acc_diag, shaped like one row of each, += the rows in row order.
 * The kernel: one workgroup of 256 threads per recording, frame after frame.  A frame's labels and hypotheses (at most 128 x 128) sit
 * in LDS; the track table (id, class, last, present, matched, matched in the previous frame) is an open-addressing table keyed by
 * the label's track_id in ws; the carry-over claims are settled by an LDS atomicMin of the label index; the assignment is a
 * shortest-augmenting-path solver with fp64 potentials on one wave, two columns per lane, whose column minimum is a wave reduction
 * and whose fp32 IoUs are recomputed (no cost matrix is held); an invalid pair costs 1e3.  2 launches, no allocation, no
 * synchronisation.  Refused on the host (SAST_EINVAL, no launch): null or not 8-byte aligned pointers, S outside 1 .. 65535, Gcap or
 * Dcap < 1, S * Gcap or S * Dcap > 2^31 - 257, K outside 1 .. SAST_EVAL_MAX_CLASSES, max_labels_per_frame or max_hyp_per_frame outside
 * 1 .. SAST_TRACKEVAL_MAX_FRAME, max_gt_tracks outside 1 .. SAST_TRACKEVAL_MAX_GT_TRACKS, iou_thre not in (0, 1], time_tol_us < 0,
 * ws_bytes < sast_trackeval_ws_bytes.  sast_trackeval_reset: acc, acc_iou and acc_diag to zero, 1 launch. */
#define SAST_TRACKEVAL_COLS 12
#define SAST_TRACKEVAL_DIAG 8
#define SAST_TRACKEVAL_MAX_FRAME 128
#define SAST_TRACKEVAL_MAX_GT_TRACKS 65536
enum { SAST_TE_FRAMES, SAST_TE_GT, SAST_TE_HYP, SAST_TE_MATCHES, SAST_TE_FP, SAST_TE_FN, SAST_TE_IDSW, SAST_TE_FRAG, SAST_TE_GT_TRACKS,
       SAST_TE_MT, SAST_TE_PT, SAST_TE_ML };
enum { SAST_TE_UNSORTED, SAST_TE_REFUSED_LABELS, SAST_TE_REFUSED_HYP, SAST_TE_REFUSED_TRACKS, SAST_TE_UNTRACKED, SAST_TE_BAD_CLASS,
       SAST_TE_DUP_GT, SAST_TE_DUP_HYP };
typedef struct {
  const int32_t* gt;       /* [S, Gcap, 10] */
  const int64_t* n_gt;     /* [S] */
  const int32_t* dt;       /* [S, Dcap, 10] */
  const int64_t* n_dt;     /* [S] */
  int64_t* rows;           /* [S, K + 1, SAST_TRACKEVAL_COLS] */
  double* rows_iou;        /* [S, K + 1] */
  int64_t* rows_diag;      /* [S, SAST_TRACKEVAL_DIAG] */
  int64_t* acc;            /* [K + 1, SAST_TRACKEVAL_COLS], ACCUMULATED */
  double* acc_iou;         /* [K + 1], ACCUMULATED */
  int64_t* acc_diag;       /* [SAST_TRACKEVAL_DIAG], ACCUMULATED */
  void* ws;                /* the track tables of one call, sast_trackeval_ws_bytes(S, max_gt_tracks) bytes; no initial contents needed */
  size_t ws_bytes;
  int64_t time_tol_us;
  int32_t S, Gcap, Dcap, K;
  int32_t max_gt_tracks, max_labels_per_frame, max_hyp_per_frame, class_agnostic;
  float iou_thre, min_diag2, min_side;
  int32_t reserved;
} SastTrackEvalArgs;
size_t sast_trackeval_ws_bytes(int S, int max_gt_tracks);   /* 0: an argument out of range.  Host only. */
int sast_trackeval_add(const SastTrackEvalArgs* a, sast_stream_t stream);
int sast_trackeval_reset(const SastTrackEvalArgs* a, sast_stream_t stream);

/* ---- tuning knobs.  Every SAST_* environment variable the library reads (tile / split / launch-shape choices, all defaulting to the
 * measured-best setting: DESIGN.md section 7) goes through one registry: the value is read from the environment at first use and cached;
 * sast_config_reload() makes every call site re-read its knob at its next use (a host that sets os.environ inside the process calls
 * it), returns the number of knobs read so far.  sast_config_get(name, default): the value the library would use for `name` now.
 * sast_config_report: "NAME=value (default d)" lines of the knobs read so far; returns the bytes needed. */
unsigned long long sast_launch_count(void);   /* kernel launches this library has enqueued in this process (any thread, any stream) */
int sast_config_reload(void);
int sast_config_get(const char* name, int default_value);
size_t sast_config_report(char* buf, size_t cap);

/* measurement aid (bench.py roofline leg): HIP-event timing of every launch of the GEMM-template kernels, recorded on
 * the launch stream; the report lists per kernel instantiation: calls, total ms, total algorithmic FLOPs (2*M*N*K with
 * the device-side row counts read back).  Enabling it adds host syncs -- never enable inside a timed region. */
int sast_prof_enable(int on);
float sast_prof_calibrate(sast_stream_t stream, int n);  /* ms a hipEvent pair reports around an empty kernel */
size_t sast_prof_report(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SAST_HIP_H */
