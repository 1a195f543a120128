// Convolution-shaped entry points (implicit GEMM on NHWC through gemm.cuh loaders):
//   - ConvDownsampling_Cf2Cl (+LayerNorm, + pos-emb)     ops.py:54-95
//   - BaseConv = conv + BatchNorm2d + SiLU                network_blocks.py:29-54
//   - nearest x2 upsample + concat, concat                yolo_pafpn.py:117-137
//   - fused AdamW on the flat parameter buffer
#include <cstdlib>
#include "gemm_dispatch.cuh"
#include "kernels.h"

using namespace sast;

namespace {

// ---------------------------------------------------------------- BatchNorm pieces
// y = silu(BN(x)); training: batch statistics from the fp64 column sums the conv epilogue accumulated (BN_STAT_COPIES
// copies, added here); every block derives (mean, rstd) of all channels into LDS once and then streams `iters` x 256
// float4 of the image; block 0 also publishes (mean, rstd) for the backward and updates the running statistics (torch
// BatchNorm2d semantics: momentum, unbiased variance).  eval: running statistics.
inline double bn_unbias(long M) { return M > 1 ? (double)M / (double)(M - 1) : 1.0; }
struct BnFwdJob {
  const float* x; const double* sums; float* run_mean; float* run_var; float* stats; const float* gamma; const float* beta;
  float* y; int ldy; float momentum, eps;
};
// blockIdx.y selects the job: one conv, or the two convs of sast_conv_bn_silu2 (same M, C)
// invM = 1 / rows behind the sums, unbias = M / (M - 1) (1 for M = 1), both from the host: every block recomputes the statistics of all C
// channels in front of its element pass, so a double division or square root there is latency of all 28 launches of a PAFPN step (round 6:
// three v_div_f64 sequences and a v_sqrt_f64 + reciprocal per channel became two multiplications and one v_rsq_f32)
__global__ __launch_bounds__(256) void bn_silu_apply_kernel(BnFwdJob j0, BnFwdJob j1, double invM, double unbias, size_t n4, int C, int training, int iters,
                                                            unsigned c4_mul) {
  SAST_KERNARG_WARM_SELF(bn_silu_apply_kernel);
  const BnFwdJob& jb = blockIdx.y == 0 ? j0 : j1;
  const float* __restrict__ x = jb.x; const double* __restrict__ sums = jb.sums;
  float* __restrict__ run_mean = jb.run_mean; float* __restrict__ run_var = jb.run_var; float* __restrict__ stats = jb.stats;
  const float* __restrict__ gamma = jb.gamma; const float* __restrict__ beta = jb.beta; float* __restrict__ y = jb.y;
  const int ldy = jb.ldy; const float momentum = jb.momentum, eps = jb.eps;
  extern __shared__ float bn_sm[];   // [2C]: mean, rstd
  // Round 6: the statistics prologue issues all loads of a channel before the first is used (ISA before: two dependent rounds behind a
  // branch), -0.25 % of the step.  (Requesting every thread's first element in front of the prologue as well measured the same: DESIGN
  // "Retired compile-time switches".)
  const int c4 = C / 4;
  const size_t e0 = (size_t)blockIdx.x * 256 * iters + threadIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) {
    float mu, rs;
    if (training) {
      double sk[BN_STAT_COPIES], qk[BN_STAT_COPIES];
#pragma unroll
      for (int k = 0; k < BN_STAT_COPIES; ++k) { sk[k] = sums[(size_t)k * 2 * C + c]; qk[k] = sums[(size_t)k * 2 * C + C + c]; }
      double s = 0.0, q = 0.0;
#pragma unroll
      for (int k = 0; k < BN_STAT_COPIES; ++k) { s += sk[k]; q += qk[k]; }
      const double mean = s * invM;
      double var = q * invM - mean * mean;
      if (var < 0) var = 0;
      mu = (float)mean;
      rs = rsqrt_hw((float)var + eps);
      if (blockIdx.x == 0 && run_mean) {
        const double unb = var * unbias;
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mean;
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unb;
      }
    } else {
      mu = run_mean[c];
      rs = rsqrt_hw(run_var[c] + eps);
    }
    if (blockIdx.x == 0) { stats[c] = mu; stats[C + c] = rs; }
    bn_sm[c] = mu; bn_sm[C + c] = rs;
  }
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    const size_t e = e0 + (size_t)it * 256;
    if (e >= n4) return;
    const size_t m = fast_div((int)e, c4, c4_mul);
    const int c = (int)(e - m * c4) * 4;
    const float4 v = ld4(x + m * C + c), g = ld4(gamma + c), b = ld4(beta + c);
    const float4 mu = *(const float4*)(bn_sm + c), rs = *(const float4*)(bn_sm + C + c);
    float4 z = make_float4((v.x - mu.x) * rs.x * g.x + b.x, (v.y - mu.y) * rs.y * g.y + b.y, (v.z - mu.z) * rs.z * g.z + b.z,
                           (v.w - mu.w) * rs.w * g.w + b.w);
    z.x *= sigmoid_hw(z.x); z.y *= sigmoid_hw(z.y); z.z *= sigmoid_hw(z.z); z.w *= sigmoid_hw(z.w);
    st4(y + m * ldy + c, z);
  }
}
// eval mode with nothing saved for a backward: BatchNorm (running statistics) + SiLU applied in the conv epilogue, same
// arithmetic order as bn_silu_apply_kernel
struct EpBnSilu {
  float* y; int ldy; const float* run_mean; const float* run_var; const float* gamma; const float* beta; float eps;
  struct Col { float mu, rs, g, b; };
  using Aux = EpNone;
  __device__ __forceinline__ Col col(int j) const { return Col{run_mean[j], 1.0f / sqrtf(run_var[j] + eps), gamma[j], beta[j]}; }
  __device__ __forceinline__ Aux pre(int, int) const { return Aux{}; }
  __device__ __forceinline__ void post(int m, int j, const float (&v)[1], const Col& k, const Aux&) const {
    const float z = (v[0] - k.mu) * k.rs * k.g + k.b;
    y[(size_t)m * ldy + j] = z * sigmoid_hw(z);
  }
};
// EpBnSilu for two convs evaluated as one GEMM over the stacked weights (columns [0, C) -> conv 0, [C, 2C) -> conv 1)
struct EpBnSilu2 {
  float* y0; float* y1; int C; const float* rm0; const float* rv0; const float* g0; const float* b0; float eps0;
  const float* rm1; const float* rv1; const float* g1; const float* b1; float eps1;
  struct Col { float mu, rs, g, b; };
  using Aux = EpNone;
  __device__ __forceinline__ Col col(int j) const {
    return j < C ? Col{rm0[j], 1.0f / sqrtf(rv0[j] + eps0), g0[j], b0[j]} : Col{rm1[j - C], 1.0f / sqrtf(rv1[j - C] + eps1), g1[j - C], b1[j - C]};
  }
  __device__ __forceinline__ Aux pre(int, int) const { return Aux{}; }
  __device__ __forceinline__ void post(int m, int j, const float (&v)[1], const Col& k, const Aux&) const {
    const float z = (v[0] - k.mu) * k.rs * k.g + k.b;
    (j < C ? y0 + (size_t)m * C + j : y1 + (size_t)m * C + (j - C))[0] = z * sigmoid_hw(z);
  }
};
// forward batch statistics as a separate pass (alternative to the atomics in the conv epilogue): row-strip blocks,
// fp64 per-channel sum / sum of squares, one atomic pair per channel per block.
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, int M, int C, double* __restrict__ sums,
                                                       int rows_per_block) {
  extern __shared__ double redd[];                // [RP][C][2]
  const int c4n = C / 4;
  const int RP = 256 / c4n > 0 ? 256 / c4n : 1;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
  for (int cq = threadIdx.x % min(c4n, 256); cq < c4n; cq += 256) {
    const int rl = threadIdx.x / c4n, c = cq * 4;
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    if (rl < RP) {
      for (int r = r0 + rl; r < r1; r += RP) {
        const float4 v = ld4(x + (size_t)r * C + c);
        s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
        q[0] += (double)v.x * v.x; q[1] += (double)v.y * v.y; q[2] += (double)v.z * v.z; q[3] += (double)v.w * v.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) { redd[((rl * C) + c + e) * 2] = s[e]; redd[((rl * C) + c + e) * 2 + 1] = q[e]; }
    }
    __syncthreads();
    if (rl == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double a = s[e], b = q[e];
        for (int k = 1; k < RP; ++k) { a += redd[((k * C) + c + e) * 2]; b += redd[((k * C) + c + e) * 2 + 1]; }
        atomicAdd(sums + c + e, a);
        atomicAdd(sums + C + c + e, b);
      }
    }
    __syncthreads();
  }
}

// backward pass 1: sums[c] += dz, sums[C+c] += dz * xhat, with dz = dy * silu'(z).
// One block owns a strip of rows and ALL channels (fully coalesced float4 rows), reduces over its rows in LDS and
// issues one atomic per channel -> (M / rows_per_block) * 2C atomics in total.
constexpr int BN_RED_THREADS = 1024;   // few workgroups (one atomic per channel and workgroup), many waves each: per-CU bandwidth needs the loads in flight
struct BnBwdJob {
  const float* x; const float* stats; const float* gamma; const float* beta; const float* dy; int lddy;
  float* sums; float* dconv; float* dgamma; float* dbeta;
  const float* dy2;   // optional second gradient of y (two consumers): dy + dy2 is formed on the fly
  int lddconv;        // row stride of dconv (two stacked convs write the halves of one [M, 2C] buffer)
};
__device__ __forceinline__ float4 bn_ld_dy(const float* __restrict__ dy, const float* __restrict__ dy2, size_t off) {
  // branch-free (round 6): a load under `if (dy2)` makes hipcc drain vmcnt(0) behind it, which serialises every load issued before it;
  // without a second gradient the second load re-reads dy (an L1 hit) and is multiplied away
  float4 d = ld4(dy + off);
  const float4 e = ld4((dy2 ? dy2 : dy) + off);
  const float k = dy2 ? 1.f : 0.f;
  d.x = fmaf(k, e.x, d.x); d.y = fmaf(k, e.y, d.y); d.z = fmaf(k, e.z, d.z); d.w = fmaf(k, e.w, d.w);
  return d;
}
__global__ __launch_bounds__(BN_RED_THREADS) void bn_bwd_reduce_kernel(BnBwdJob j0, BnBwdJob j1, int M, int C, int rows_per_block) {
  SAST_KERNARG_WARM_SELF(bn_bwd_reduce_kernel);
  const BnBwdJob& jb = blockIdx.y == 0 ? j0 : j1;
  const float* __restrict__ x = jb.x; const float* __restrict__ stats = jb.stats; const float* __restrict__ gamma = jb.gamma;
  const float* __restrict__ beta = jb.beta; const float* __restrict__ dy = jb.dy; const int lddy = jb.lddy;
  float* __restrict__ sums = jb.sums;
  extern __shared__ float4 red[];                 // [RP][C/4][2]
  const int c4n = C / 4;
  const int RP = BN_RED_THREADS / c4n > 0 ? BN_RED_THREADS / c4n : 1;   // rows processed in parallel by the block
  const int r0 = blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
  for (int cq = threadIdx.x % min(c4n, BN_RED_THREADS); cq < c4n; cq += BN_RED_THREADS) {
    const int rl = threadIdx.x / c4n;
    const int c = cq * 4;
    float4 a = zero4(), b = zero4();
    if (rl < RP) {
      const float4 mu = ld4(stats + c), rs = ld4(stats + C + c), g = ld4(gamma + c), bt = ld4(beta + c);
      for (int r = r0 + rl; r < r1; r += RP) {
        const float4 v = ld4(x + (size_t)r * C + c), d = bn_ld_dy(dy, jb.dy2, (size_t)r * lddy + c);
        const float xh[4] = {(v.x - mu.x) * rs.x, (v.y - mu.y) * rs.y, (v.z - mu.z) * rs.z, (v.w - mu.w) * rs.w};
        const float gg[4] = {g.x, g.y, g.z, g.w}, bb[4] = {bt.x, bt.y, bt.z, bt.w}, dd[4] = {d.x, d.y, d.z, d.w};
        float* ap = &a.x; float* bp = &b.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float z = xh[e] * gg[e] + bb[e], sg = sigmoid_hw(z);
          const float dz = dd[e] * sg * (1.f + z * (1.f - sg));
          ap[e] += dz; bp[e] += dz * xh[e];
        }
      }
      red[(rl * c4n + cq) * 2] = a; red[(rl * c4n + cq) * 2 + 1] = b;
    }
    __syncthreads();
    if (rl == 0) {
      for (int k = 1; k < RP; ++k) {
        const float4 t = red[(k * c4n + cq) * 2], u = red[(k * c4n + cq) * 2 + 1];
        a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w; b.x += u.x; b.y += u.y; b.z += u.z; b.w += u.w;
      }
      atomicAdd(sums + c, a.x); atomicAdd(sums + c + 1, a.y); atomicAdd(sums + c + 2, a.z); atomicAdd(sums + c + 3, a.w);
      atomicAdd(sums + C + c, b.x); atomicAdd(sums + C + c + 1, b.y); atomicAdd(sums + C + c + 2, b.z); atomicAdd(sums + C + c + 3, b.w);
    }
    __syncthreads();
  }
}
// backward pass 2: dconv = gamma * rstd * (dz - mean(dz) - xhat * mean(dz*xhat))   [training]
// Every block first folds the BN_STAT_COPIES copies of the two sums (written by bn_bwd_reduce_kernel into copy 0, or by the
// consuming conv's dX epilogue into all of them) and the per-channel constants into LDS, then streams `iters` x 256 float4;
// block 0 also publishes the affine gradients.
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnBwdJob j0, BnBwdJob j1, size_t n4, int C, float invM, int training, int iters,
                                                           unsigned c4_mul) {
  SAST_KERNARG_WARM_SELF(bn_bwd_apply_kernel);
  const BnBwdJob& jb = blockIdx.y == 0 ? j0 : j1;
  const float* __restrict__ x = jb.x; const float* __restrict__ stats = jb.stats; const float* __restrict__ gamma = jb.gamma;
  const float* __restrict__ beta = jb.beta; const float* __restrict__ dy = jb.dy; const int lddy = jb.lddy;
  const float* __restrict__ sums = jb.sums; float* __restrict__ dconv = jb.dconv;
  float* __restrict__ dgamma = jb.dgamma; float* __restrict__ dbeta = jb.dbeta;
  extern __shared__ float bsm[];   // [6][C]: mean, rstd, gamma, beta, mean(dz), mean(dz*xhat)
  // (round 6, as in bn_silu_apply_kernel: all 12 loads of a channel of the prologue are issued before the first is used -- the block-0
  // publication of the affine gradients sits behind them)
  const int c4 = C / 4;
  const size_t e0 = (size_t)blockIdx.x * 256 * iters + threadIdx.x;
  for (int c = threadIdx.x; c < C; c += 256) {
    float a1[BN_STAT_COPIES], a2[BN_STAT_COPIES];
#pragma unroll
    for (int k = 0; k < BN_STAT_COPIES; ++k) { a1[k] = sums[(size_t)k * 2 * C + c]; a2[k] = sums[(size_t)k * 2 * C + C + c]; }
    const float st_mu = stats[c], st_rs = stats[C + c], gm = gamma[c], bt = beta[c];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < BN_STAT_COPIES; ++k) { s1 += a1[k]; s2 += a2[k]; }
    bsm[c] = st_mu; bsm[C + c] = st_rs; bsm[2 * C + c] = gm; bsm[3 * C + c] = bt;
    bsm[4 * C + c] = s1 * invM; bsm[5 * C + c] = s2 * invM;
    if (blockIdx.x == 0 && dbeta) { dbeta[c] += s1; dgamma[c] += s2; }   // NULL: the host already published them (SyncBatchNorm: LOCAL sums)
  }
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    const size_t e4 = e0 + (size_t)it * 256;
    if (e4 >= n4) return;
    const size_t m = fast_div((int)e4, c4, c4_mul);
    const int c = (int)(e4 - m * c4) * 4;
    const float4 v = ld4(x + m * C + c), d = bn_ld_dy(dy, jb.dy2, m * lddy + c);
    float out[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float mu = bsm[c + e], rs = bsm[C + c + e], g = bsm[2 * C + c + e];
      const float xh = ((&v.x)[e] - mu) * rs;
      const float z = xh * g + bsm[3 * C + c + e], sg = sigmoid_hw(z);
      const float dz = (&d.x)[e] * sg * (1.f + z * (1.f - sg));
      out[e] = training ? g * rs * (dz - bsm[4 * C + c + e] - xh * bsm[5 * C + c + e]) : g * rs * dz;
    }
    st4(dconv + m * jb.lddconv + c, make_float4(out[0], out[1], out[2], out[3]));
  }
}
// SyncBatchNorm, backward phase 1: the affine gradients are this process's LOCAL sums (torch.nn.SyncBatchNorm: DDP averages them with
// every other gradient) -- published from the reduction scratch before the host all-reduces it
__global__ __launch_bounds__(256) void bn_publish_affine_kernel(const float* __restrict__ sums, float* __restrict__ dgamma, float* __restrict__ dbeta, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < BN_STAT_COPIES; ++k) { s1 += sums[(size_t)k * 2 * C + c]; s2 += sums[(size_t)k * 2 * C + C + c]; }
  dbeta[c] += s1;
  dgamma[c] += s2;
}
// ---------------------------------------------------------------- upsample / concat
// IDX: unsigned when every element index fits 32 bits (the launcher checks): a 64-bit integer division is ~120 VALU instructions on
// gfx950, a 32-bit one ~35, and the index decode below has five of them IN FRONT of the first load (round 6: 517 instructions before the
// first vector memory operation of a 6 us kernel)
template <class IDX>
__global__ __launch_bounds__(256) void upsample_cat_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                               float* __restrict__ out, int H, int W, int C1, int C2, size_t n4) {
  const size_t e64 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e64 >= n4) return;
  const IDX e = (IDX)e64;
  const int Ct = C1 + C2;
  const IDX c4n = (IDX)(Ct / 4);
  const IDX row = e / c4n; const int c = (int)(e - row * c4n) * 4;
  float4 v;
  if (c < C1) {
    const IDX W2 = (IDX)(2 * W), H2 = (IDX)(2 * H);
    const IDX t = row / W2; const int x = (int)(row - t * W2); const IDX bb = t / H2; const int y = (int)(t - bb * H2);
    v = ld4(a + (((size_t)bb * H + (y >> 1)) * W + (x >> 1)) * C1 + c);
  } else {
    v = ld4(b + (size_t)row * C2 + (c - C1));
  }
  st4(out + (size_t)row * Ct + c, v);
}
// backward of upsample + concat in one launch: elements [0, n4) reduce the 2x2 children of the upsampled half into da, elements
// [n4, n4 + n4b) copy the other half of the channels into db
template <class IDX>
__global__ __launch_bounds__(256) void upsample_cat_bwd_kernel(const float* __restrict__ dout, float* __restrict__ da, float* __restrict__ db,
                                                               int H, int W, int C1, int Ct, size_t n4, size_t n4b) {
  const size_t e64 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e64 >= n4) {
    const size_t eb64 = e64 - n4;
    if (eb64 >= n4b) return;
    const IDX eb = (IDX)eb64;
    const int C2 = Ct - C1;
    const IDX c4b = (IDX)(C2 / 4);
    const IDX row = eb / c4b; const int c = (int)(eb - row * c4b) * 4;
    st4(db + (size_t)row * C2 + c, ld4(dout + (size_t)row * Ct + C1 + c));
    return;
  }
  const IDX e = (IDX)e64;
  const IDX c4n = (IDX)(C1 / 4);
  const IDX row = e / c4n; const int c = (int)(e - row * c4n) * 4;
  const IDX t = row / (IDX)W; const int x = (int)(row - t * (IDX)W); const IDX bb = t / (IDX)H; const int y = (int)(t - bb * (IDX)H);
  const size_t base = (((size_t)bb * 2 * H + 2 * y) * 2 * W + 2 * x);
  const float4 p = ld4(dout + base * Ct + c), q = ld4(dout + (base + 1) * Ct + c);
  const float4 r = ld4(dout + (base + 2 * W) * Ct + c), s = ld4(dout + (base + 2 * W + 1) * Ct + c);
  st4(da + (size_t)row * C1 + c, make_float4((p.x + q.x) + (r.x + s.x), (p.y + q.y) + (r.y + s.y), (p.z + q.z) + (r.z + s.z), (p.w + q.w) + (r.w + s.w)));
}
// copy a channel slice: dst[row, 0:Cs] = src[row*lds + off : +Cs]   (or the reverse with dst stride)
__global__ __launch_bounds__(256) void slice_copy_kernel(const float* __restrict__ src, int lds, int soff, float* __restrict__ dst,
                                                         int ldd, int doff, int Cs, size_t n4) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  const int c4n = Cs / 4;
  const size_t row = e / c4n; const int c = (int)(e % c4n) * 4;
  st4(dst + row * ldd + doff + c, ld4(src + row * lds + soff + c));
}
int slice_copy(const float* src, int lds, int soff, float* dst, int ldd, int doff, int Cs, size_t rows, hipStream_t st) {
  const size_t n4 = rows * (Cs / 4);
  if (!n4) return SAST_OK;
  SAST_LAUNCH(slice_copy_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, src, lds, soff, dst, ldd, doff, Cs, n4);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

// ---------------------------------------------------------------- AdamW
struct OneCycle { int on; double initial_lr, max_lr, min_lr, end1, end2; };
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, size_t n4, const float* __restrict__ lr_step, double b1d,
                                                    double b2d, float eps, float wd, float gscale, float clip, OneCycle oc) {
  SAST_KERNARG_WARM_SELF(adamw_kernel);
  // bias corrections in DOUBLE from the double betas, once per workgroup: torch.optim.AdamW evaluates 1 - beta**step with python
  // doubles; 1 - powf(0.999f, t) loses ~1e-5 relative at small t (cancellation, and 0.999f itself is off by 1.3e-8)
  __shared__ float s_bc[3];
  if (threadIdx.x == 0) {
    const double step = (double)lr_step[1];
    s_bc[0] = (float)(1.0 - pow(b1d, step));
    s_bc[1] = (float)sqrt(1.0 - pow(b2d, step));
    double lr = (double)lr_step[0];
    if (oc.on) {   // OneCycleLR, linear anneal, two phases (torch.optim.lr_scheduler.OneCycleLR.get_lr)
      const double sn = step - 1.0;
      if (sn <= oc.end1) lr = oc.initial_lr + (oc.max_lr - oc.initial_lr) * (oc.end1 > 0.0 ? sn / oc.end1 : 1.0);
      else lr = oc.max_lr + (oc.min_lr - oc.max_lr) * ((sn - oc.end1) / (oc.end2 - oc.end1));
    }
    s_bc[2] = (float)lr;
  }
  __syncthreads();
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  const float lr = s_bc[2];
  const float bc1 = s_bc[0], bc2s = s_bc[1];
  const float b1 = (float)b1d, b2 = (float)b2d, omb1 = (float)(1.0 - b1d), omb2 = (float)(1.0 - b2d);
  float4 pv = ld4(p + e * 4), gv = ld4(g + e * 4), mv = ld4(m + e * 4), vv = ld4(v + e * 4);
  float* pp = &pv.x; float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float gr = gp[k] * gscale;
    if (clip > 0.f) gr = clamp_keep_nan(gr, -clip, clip);      // clamp_ of clip_grad_value_: a NaN gradient reaches m, v and p
    pp[k] *= 1.f - lr * wd;
    mp[k] = b1 * mp[k] + omb1 * gr;
    vp[k] = b2 * vp[k] + omb2 * gr * gr;
    const float denom = sqrtf(vp[k]) / bc2s + eps;
    pp[k] -= (lr / bc1) * (mp[k] / denom);
  }
  st4(p + e * 4, pv); st4(m + e * 4, mv); st4(v + e * 4, vv);
}

// (dz, dz * xhat) column sums of `njobs` convs of equal shape (blockIdx.y = job)
void bn_bwd_reduce_launch(const BnBwdJob& j0, const BnBwdJob& j1, int njobs, int M, int C, hipStream_t st) {
  const int target = SAST_KNOB("SAST_BN_BLOCKS", 32);
  int rpb = (M + target - 1) / target;
  rpb = rpb < 8 ? 8 : (rpb > 512 ? 512 : rpb);
  const int c4n = C / 4, RP = BN_RED_THREADS / c4n > 0 ? BN_RED_THREADS / c4n : 1;
  SAST_LAUNCH(bn_bwd_reduce_kernel, dim3((M + rpb - 1) / rpb, njobs), dim3(BN_RED_THREADS), sizeof(float4) * 2 * RP * c4n, st, j0, j1, M, C,
                     rpb);
}
// float4 loop trips per thread of the BatchNorm-apply kernels: >= 512 blocks while the image allows it; the per-block statistics prologue
// is 2C*COPIES loads
inline int bn_apply_iters(size_t n4) {
  const int iters = (int)(n4 / (256 * 512));
  return iters < 1 ? 1 : (iters > 8 ? 8 : iters);
}
// m_stat: rows behind the sums (all ranks; 0: the M rows of this process)
void bn_bwd_apply_launch(const BnBwdJob& j0, const BnBwdJob& j1, int njobs, int M, int C, int training, hipStream_t st, int m_stat = 0) {
  const size_t n4 = (size_t)M * (C / 4);
  const int iters = bn_apply_iters(n4);
  SAST_LAUNCH(bn_bwd_apply_kernel, dim3((unsigned)((n4 + 256 * iters - 1) / (256 * iters)), njobs), dim3(256), sizeof(float) * 6 * C, st,
                     j0, j1, n4, C, 1.0f / (float)(m_stat > 0 ? m_stat : M), training, iters, div_mul_of((unsigned)(C / 4), n4));
}
// y = silu(BN(conv_out)) of `njobs` convs of equal shape (blockIdx.y = job), statistics over m_stat rows
void bn_fwd_apply_launch(const BnFwdJob& j0, const BnFwdJob& j1, int njobs, int M, int m_stat, int C, int training, hipStream_t st) {
  const size_t n4 = (size_t)M * (C / 4);
  const int iters = bn_apply_iters(n4);
  SAST_LAUNCH(bn_silu_apply_kernel, dim3((unsigned)((n4 + 256 * iters - 1) / (256 * iters)), njobs), dim3(256), sizeof(float) * 2 * C, st, j0, j1,
                     1.0 / (double)m_stat, bn_unbias(m_stat), n4, C, training, iters, div_mul_of((unsigned)(C / 4), n4));
}
// fp64 column sums of conv_out as a row-strip pass of about `target_blocks` blocks
void bn_stats_launch(const float* conv_out, int M, int C, double* sums, int target_blocks, hipStream_t st) {
  int rpb = (M + target_blocks - 1) / target_blocks;
  rpb = rpb < 8 ? 8 : rpb;
  const int c4n = C / 4, RP = 256 / c4n > 0 ? 256 / c4n : 1;
  SAST_LAUNCH(bn_stats_kernel, dim3((M + rpb - 1) / rpb), dim3(256), sizeof(double) * 2 * RP * C, st, conv_out, M, C, sums, rpb);
}
// the producer behind one source of a conv (SastConvBnArgs.p_* / p2_*): its backward sums are the second block of its reduction scratch
inline BnProducer producer_of(const float* conv_out, const float* stats, const float* w, const float* b, float* ws, int C) {
  return BnProducer{conv_out, stats, w, b, ws ? ws + 4 * BN_STAT_COPIES * C : nullptr, C};
}
inline bool complete(const BnProducer& p) { return p.stats && p.gamma && p.beta && p.sums; }
// the dX job of a backward pair with the plain epilogue or, when `fold`, with the one that also reduces the producers' BatchNorm
// backward sums.  `launch` is a generic lambda: its closure stays on the host, only the epilogue's type reaches a kernel
template <class EP, class EPR, class F>
int with_dx_epilogue(bool fold, const EP& plain, const EPR& red, const F& launch) { return fold ? launch(red) : launch(plain); }

inline ConvGeom geom_of(int B, int H, int W, int Cin, int k, int stride, int pad, int replicate, int ldx) {
  ConvGeom g;
  g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.KH = k; g.KW = k; g.stride = stride; g.pad = pad; g.replicate = replicate; g.ldx = ldx;
  g.Ho = (H + 2 * pad - k) / stride + 1;
  g.Wo = (W + 2 * pad - k) / stride + 1;
  g.stride_shift = pow2_shift(stride);     // strides are 1, 2 or 4
  g.kw_mul = small_div_mul(k);
  const unsigned long long rows = (unsigned long long)B * g.Ho * g.Wo;
  g.wo_mul = div_mul_of((unsigned)g.Wo, rows);
  g.ho_mul = div_mul_of((unsigned)g.Ho, rows);
  g.cin_mul = div_mul_of((unsigned)Cin, (unsigned long long)k * k * Cin);
  g.w_mul = div_mul_of((unsigned)W, (unsigned long long)B * H * W);
  g.h_mul = div_mul_of((unsigned)H, (unsigned long long)B * H * W);
  return g;
}

// forward implicit GEMM of a k x k convolution: the uniform-tap loader whenever a 16-wide k-tile lies inside one tap (gemm.cuh: LdIm2colU)
template <class LB, class EP>
int conv_gemm(const float* x, const ConvGeom& g, const LB& lb, const EP& ep, int M, int NJ, int K, hipStream_t st) {
  if (!g.cin_mul) return SAST_EINVAL;     // the loaders decode (tap, channel) with this multiplier only (gemm.cuh: split_tap)
  if (g.Cin % 16 == 0) return gemm_auto(LdIm2colU{{x, g}}, lb, ep, M, NJ, K, st);
  return gemm_auto(LdIm2col{x, g}, lb, ep, M, NJ, K, st);
}
// forward GEMM of a conv unit over the source(s) `src` ([x | x2]; x2 may be NULL): the row loaders for a 1x1 stride-1 conv, conv_gemm for
// everything else.  ROWS1: one source has the loader of its own (LdRows); the stacked pair reads it through LdRows2 as well (false)
template <bool ROWS1, class LB, class EP>
int conv_fwd_gemm(const ConvGeom& g, const LdRows2& src, const LB& lb, const EP& ep, int M, int NJ, int K, hipStream_t st) {
  if (g.KH != 1 || g.stride != 1) return conv_gemm(src.p1, g, lb, ep, M, NJ, K, st);
  if constexpr (ROWS1)
    if (!src.p2) return gemm_auto(LdRows{src.p1, src.ld1, nullptr}, lb, ep, M, NJ, K, st);
  return gemm_auto(src, lb, ep, M, NJ, K, st);
}

// backward of a k x k convolution.  Stride 2 with a 3x3 kernel (downsample convs of stages 2-4, the two bottom-up PAFPN convs)
// computes dX through the parity-class form (gemm.cuh: LdConvDxP) unless SAST_CONVDX_PARITY=0; everything else through the
// generic gather.
// dW (TN over the im2col rows) and dX of a k x k convolution in one launch
int conv_bwd_pair(const float* dconv, const float* x, const ConvGeom& g, int Cout, const float* w, float* dw, float* dx, int lddx,
                  hipStream_t st, const BnProducer* prod = nullptr) {
  const int k = g.KH, K = k * k * g.Cin, M = g.B * g.Ho * g.Wo;
  const unsigned shift = div_mul_of((unsigned)Cout, (unsigned long long)k * k * Cout);   // tap = umulhi(r, shift): multiplier, not a shift
  if (!shift || !g.cin_mul || g.stride_shift < 0) return SAST_EINVAL;
  const LdRowsT ta{dconv, Cout};
  const LdIm2colT tb{x, g};
  if (!dx) return gemm_tn(ta, tb, dw, K, Cout, K, M, st);
  const int parity = SAST_KNOB("SAST_CONVDX_PARITY", 1);
  const int Mc = g.B * (g.H / 2) * (g.W / 2);
  const bool fold = prod && prod->x;   // stride-1 convs only (the caller checks): dX epilogue also reduces the producer's BatchNorm backward sums
  if (fold && (g.stride != 1 || lddx != g.Cin || prod->C != g.Cin)) return SAST_EINVAL;
  if (fold || !(parity && g.stride == 2 && k == 3 && g.pad == 1 && g.H % 2 == 0 && g.W % 2 == 0 && Mc % 64 == 0))
    return with_dx_epilogue(fold, EpStore{dx, lddx, nullptr}, EpStoreBnRed{dx, lddx, fold ? *prod : BnProducer{}}, [&](const auto& ep) {
      if (Cout % 16 == 0)      // the uniform-tap loaders (gemm.cuh: LdConvDxU)
        return gemm_pair(ta, tb, dw, K, Cout, K, M, nullptr, nullptr, LdConvDxU{{dconv, g, Cout, Cout, shift}},
                         LdWeightConvDxU{{w, Cout, k * k, g.Cin, shift}}, ep, g.B * g.H * g.W, g.Cin, k * k * Cout, nullptr, st, pair_tn_blocks_conv());
      return gemm_pair(ta, tb, dw, K, Cout, K, M, nullptr, nullptr, LdConvDx{dconv, g, Cout, Cout, shift},
                       LdWeightConvDx{w, Cout, k * k, g.Cin, shift}, ep, g.B * g.H * g.W, g.Cin, k * k * Cout, nullptr, st, pair_tn_blocks_conv());
    });
  ConvDxClasses c;
  c.Hc = g.H / 2; c.Wc = g.W / 2; c.Mc = Mc;
  c.mc_mul = div_mul_of((unsigned)c.Mc, 4ull * Mc); c.wc_mul = div_mul_of((unsigned)c.Wc, 4ull * Mc); c.hc_mul = div_mul_of((unsigned)c.Hc, 4ull * Mc);
  for (int cls = 0; cls < 4; ++cls) {
    const int py = (3 - cls) >> 1, px = (3 - cls) & 1;   // row order: heaviest class first (gemm.cuh: LdConvDxP)
    // taps that can be non-zero for this class: matching parity, plus (replicate padding) the border tap kk < pad that folds
    // onto output row / column 0 for input row / column 0 (an even one); unused slots are marked 15
    int ty[2] = {15, 15}, tx[2] = {15, 15}, ny = 0, nx = 0;
    for (int kk = 0; kk < k; ++kk) {
      if ((py + g.pad - kk) % 2 == 0 || (g.replicate && py == 0 && kk < g.pad)) ty[ny++] = kk;
      if ((px + g.pad - kk) % 2 == 0 || (g.replicate && px == 0 && kk < g.pad)) tx[nx++] = kk;
    }
    c.kh_pack[cls] = c.kw_pack[cls] = 0;
    int slot = 0;
    for (int pass = 0; pass < 2; ++pass)      // used (tap row, tap column) pairs first, empty slots after them
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
          const bool used = ty[a] != 15 && tx[b] != 15;
          if (used != (pass == 0)) continue;
          c.kh_pack[cls] |= (unsigned)(used ? ty[a] : 15) << (4 * slot);
          c.kw_pack[cls] |= (unsigned)(used ? tx[b] : 15) << (4 * slot);
          ++slot;
        }
    c.nslot[cls] = ny * nx;
  }
  return gemm_pair(ta, tb, dw, K, Cout, K, M, nullptr, nullptr, LdConvDxP{dconv, g, Cout, Cout, shift, c},
                   LdWeightConvDxP{w, Cout, k * k, g.Cin, shift, g.KW, c}, EpStoreClass{dx, lddx, g.H, g.W, c}, 4 * Mc, g.Cin, 4 * Cout,
                   nullptr, st, pair_tn_blocks_conv());
}

// sizes the downsample conv accepts.  The overlapping form (k = 2f-1, replicate padding f-1) has ceil(H / f) output rows: at an H or W
// that is not a multiple of the factor that is more rows than the H / f the callers size their buffers for, and the replicate clamp
// would also act at the bottom / right edge, which LdConvDx / LdConvDxP do not fold.  The reference only uses multiples: refused.
inline bool stem_exact_bf16() { return SAST_KNOB("SAST_STEM_EXACT_BF16", 1) != 0; }
bool down_size_ok(const SastDownArgs* a) {
  if (a->factor < 1 || a->B < 1 || a->H < a->factor || a->W < a->factor) return false;
  return a->no_overlap || (a->H % a->factor == 0 && a->W % a->factor == 0);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ downsample conv + LayerNorm
int sast_downsample_ln_fwd(const SastDownArgs* a, sast_stream_t stream) { SAST_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps_("down_fwd", a ? a->Cout : 0, a ? a->B * a->H * a->W : 0, st);
  if (!a || a->Cin % 4 || a->Cout % 4 || !down_size_ok(a)) return SAST_EINVAL;
  // ops.py:70-76: overlap (default) k = 2f-1 with replicate padding f-1; no_overlap: k = f, no padding (non-overlapping patches)
  const int k = a->no_overlap ? a->factor : 2 * a->factor - 1;
  const ConvGeom g = geom_of(a->B, a->H, a->W, a->Cin, k, a->factor, a->no_overlap ? 0 : a->factor - 1, 1, a->Cin);
  const int M = a->B * g.Ho * g.Wo, K = k * k * a->Cin;
  int rc;
  // an event tensor that is exact in bf16 (uint8: by type; fp32: the word of sast_input_prep_flag, read by the kernel): the loaders with
  // the EXACT_BF16 trait (gemm.cuh), whose kernels carry the three-term k-loop beside the six-term one
  const bool exact_ok = stem_exact_bf16();
  if (a->x_dtype == SAST_DT_U8 && exact_ok)
    rc = !g.cin_mul ? SAST_EINVAL : gemm_auto(LdIm2colQ8X{{(const unsigned char*)a->x, g}}, LdWeightNT{a->w, K, 0}, EpStore{a->conv_out, a->Cout, nullptr}, M, a->Cout, K, st);
  else if (a->x_dtype == SAST_DT_U8)       // the stem on the stored uint8 event tensor (NHWC bytes, written by sast_input_prep_u8)
    rc = !g.cin_mul ? SAST_EINVAL : gemm_auto(LdIm2colQ8{(const unsigned char*)a->x, g}, LdWeightNT{a->w, K, 0}, EpStore{a->conv_out, a->Cout, nullptr}, M, a->Cout, K, st);
  else if (a->x_dtype != SAST_DT_F32) return SAST_EINVAL;
  else if (a->x_nonexact && exact_ok && g.Cin % 16)
    rc = !g.cin_mul ? SAST_EINVAL : gemm_auto(LdIm2colX{{a->x, g}, a->x_nonexact}, LdWeightNT{a->w, K, 0}, EpStore{a->conv_out, a->Cout, nullptr}, M, a->Cout, K, st);
  else rc = conv_gemm(a->x, g, LdWeightNT{a->w, K, 0}, EpStore{a->conv_out, a->Cout, nullptr}, M, a->Cout, K, st);
  if (rc) return rc;
  return ln_fwd_launch(a->conv_out, a->y, a->ln_w, a->ln_b, a->pe, g.Ho * g.Wo, a->mean, a->rstd, M, a->Cout, 1e-5f, st);
}

int sast_downsample_ln_bwd(const SastDownArgs* a, sast_stream_t stream) { SAST_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps_("down_bwd", a->Cout, a->B * a->H * a->W, st);
  if (a->Cin % 4 || a->Cout % 4 || !down_size_ok(a) || (a->x_dtype == SAST_DT_U8 && a->dx)) return SAST_EINVAL;   // (an integer input has no gradient)
  const int k = a->no_overlap ? a->factor : 2 * a->factor - 1;
  const ConvGeom g = geom_of(a->B, a->H, a->W, a->Cin, k, a->factor, a->no_overlap ? 0 : a->factor - 1, 1, a->Cin);
  const int M = a->B * g.Ho * g.Wo, K = k * k * a->Cin;
  float* dconv = a->ws;
  int rc = ln_bwd_launch(a->conv_out, a->dy, a->ln_w, a->mean, a->rstd, dconv, a->d_ln_w, a->d_ln_b, M, a->Cout, st);
  if (rc) return rc;
  if (a->x_dtype == SAST_DT_U8) {     // an integer input has no gradient: the weight gradient only
    if (a->dx || !g.cin_mul) return SAST_EINVAL;
    if (stem_exact_bf16()) return gemm_tn(LdRowsT{dconv, a->Cout}, LdIm2colTQ8X{{(const unsigned char*)a->x, g}}, a->dw, K, a->Cout, K, M, st);
    return gemm_tn(LdRowsT{dconv, a->Cout}, LdIm2colTQ8{(const unsigned char*)a->x, g}, a->dw, K, a->Cout, K, M, st);
  }
  if (a->x_dtype != SAST_DT_F32) return SAST_EINVAL;
  if (a->x_nonexact && !a->dx && stem_exact_bf16() && g.Cin % 16) {     // the stem's weight gradient on the flagged fp32 copy of the event tensor
    if (!g.cin_mul) return SAST_EINVAL;
    return gemm_tn(LdRowsT{dconv, a->Cout}, LdIm2colTX{{a->x, g}, a->x_nonexact}, a->dw, K, a->Cout, K, M, st);
  }
  return conv_bwd_pair(dconv, a->x, g, a->Cout, a->w, a->dw, a->dx, a->Cin, st);
}

// ------------------------------------------------------------------ conv + BN + SiLU
int sast_conv_bn_ws_floats(int Cout) { SAST_ENTRY(); return SAST_BN_WS_FLOATS(Cout); }

int sast_conv_bn_silu_fwd(const SastConvBnArgs* a, sast_stream_t stream) { SAST_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps_("convbn_fwd", a ? a->Cout * 10 + a->ksize : 0, a ? a->B * a->H * a->W : 0, st);
  if (!a || a->Cin % 4 || a->Cout % 4 || (a->ksize != 1 && a->ksize != 3)) return SAST_EINVAL;
  const int k = a->ksize, pad = (k - 1) / 2;
  const ConvGeom g = geom_of(a->B, a->H, a->W, a->Cin, k, a->stride, pad, 0, a->ldx);
  const int M = a->B * g.Ho * g.Wo, K = k * k * a->Cin, C = a->Cout;
  if ((unsigned long long)M * (C / 4) >= (1ull << 31)) return SAST_EINVAL;   // element indices of the BatchNorm passes are 31-bit
  // groups == Cin == Cout: the depth-wise half of YOLOX's DWConv (network_blocks.py:57-76) -- a stencil, not a GEMM (k_dwconv.hip);
  // the BatchNorm + SiLU passes around it are the dense conv's
  const bool dw = a->groups > 1;
  if (dw && (a->groups != a->Cin || a->Cin != a->Cout || a->x2 || a->ldx != a->Cin)) return SAST_EINVAL;
  const DwGeom dg{a->H, a->W, g.Ho, g.Wo, C, k, a->stride};
  double* sums = (double*)a->bn_ws;
  // SyncBatchNorm (include/sast_hip.h: sync_phase): 1 = conv + this process's column sums, 2 = BatchNorm + SiLU from the sums the host
  // all-reduced in between, over the m_total rows of all ranks
  const int phase = a->training ? a->sync_phase : 0;
  if (phase < 0 || phase > 2 || (phase == 2 && a->m_total < M)) return SAST_EINVAL;
  if (a->training && !a->bn_ws_zeroed && phase != 2) zero_fill(a->bn_ws, sizeof(float) * SAST_BN_WS_FLOATS(C), st);
  int rc = SAST_OK;
  const int sep = SAST_KNOB("SAST_BN_STATS_SEPARATE", 0);
  const bool one = k == 1 && a->stride == 1;
  if (a->x2 && (!one || a->Cin1 % 4 || a->Cin1 <= 0 || a->Cin1 >= a->Cin)) return SAST_EINVAL;   // (Cin1 == Cin refused here, accepted by the stacked pair)
  const LdRows2 src{a->x, a->ldx, a->Cin1, a->x2, a->ldx2};    // virtual channel concat [x | x2]
  const LdWeightNT lw{a->w, K, 0};
  if (!a->training && !a->conv_out) {   // inference: one launch, nothing kept for a backward
    if (!a->run_mean || !a->run_var) return SAST_EINVAL;
    if (dw) {
      if (a->ldy != C) return SAST_EINVAL;
      const DwBnSilu bn{a->run_mean, a->run_var, a->bn_w, a->bn_b, a->eps};
      rc = dwconv_fwd_launch(a->x, a->w, nullptr, a->y, a->B, dg, &bn, st);
      if (rc) return rc;
      SAST_CHECK_LAUNCH();
      return SAST_OK;
    }
    return conv_fwd_gemm<true>(g, src, lw, EpBnSilu{a->y, a->ldy, a->run_mean, a->run_var, a->bn_w, a->bn_b, a->eps}, M, C, K, st);
  }
  if (phase == 2) {            // the conv and its sums are phase 1's
  } else if (dw) {             // the stencil, then (training) its column sums as a row-strip pass
    rc = dwconv_fwd_launch(a->x, a->w, nullptr, a->conv_out, a->B, dg, nullptr, st);
    if (!rc && a->training) bn_stats_launch(a->conv_out, M, C, sums, 128, st);
  } else if (a->training && !sep) {   // conv + per-channel sum / sum-of-squares in one pass
    rc = conv_fwd_gemm<true>(g, src, lw, EpStoreStats{a->conv_out, C, sums}, M, C, K, st);
  } else {
    rc = conv_fwd_gemm<true>(g, src, lw, EpStore{a->conv_out, C, nullptr}, M, C, K, st);
  }
  if (rc) return rc;
  if (a->training && sep && phase != 2 && !dw) bn_stats_launch(a->conv_out, M, C, sums, sep, st);
  if (phase == 1) { SAST_CHECK_LAUNCH(); return SAST_OK; }
  const BnFwdJob jb{a->conv_out, sums, a->run_mean, a->run_var, a->stats, a->bn_w, a->bn_b, a->y, a->ldy, a->momentum, a->eps};
  bn_fwd_apply_launch(jb, jb, 1, M, phase == 2 ? a->m_total : M, C, a->training, st);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_conv_bn_silu_bwd(const SastConvBnArgs* a, sast_stream_t stream) { SAST_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps_("convbn_bwd", a->Cout * 10 + a->ksize, a->B * a->H * a->W, st);
  const int k = a->ksize, pad = (k - 1) / 2;
  const ConvGeom g = geom_of(a->B, a->H, a->W, a->Cin, k, a->stride, pad, 0, a->ldx);
  const int M = a->B * g.Ho * g.Wo, K = k * k * a->Cin, C = a->Cout;
  float* sums = a->bn_ws + 4 * BN_STAT_COPIES * C;      // [COPIES][2C]
  float* dconv = a->ws;                // [M, C]
  const int phase = a->training ? a->sync_phase : 0;   // SyncBatchNorm: 1 = this process's (sum dz, sum dz*xhat) only, 2 = everything after the host's all-reduce
  if (phase < 0 || phase > 2 || (phase == 2 && a->m_total < M)) return SAST_EINVAL;
  if (!a->bn_ws_zeroed && phase != 2) {
    if (a->bn_red_done) return SAST_EINVAL;   // the consumer has already accumulated into it
    zero_fill(sums, sizeof(float) * 2 * BN_STAT_COPIES * C, st);
  }
  const BnBwdJob jb{a->conv_out, a->stats, a->bn_w, a->bn_b, a->dy, a->lddy, sums, dconv, a->d_bn_w, a->d_bn_b, a->dy2, C};
  if (!a->bn_red_done && phase != 2) bn_bwd_reduce_launch(jb, jb, 1, M, C, st);   // skipped when the conv consuming y folded it into its dX epilogue
  if (phase == 1) {
    if (a->d_bn_w && a->d_bn_b) SAST_LAUNCH(bn_publish_affine_kernel, dim3((C + 255) / 256), dim3(256), 0, st, sums, a->d_bn_w, a->d_bn_b, C);
    SAST_CHECK_LAUNCH();
    return SAST_OK;
  }
  bn_bwd_apply_launch(jb, jb, 1, M, C, a->training, st, phase == 2 ? a->m_total : 0);
  SAST_CHECK_LAUNCH();
  // producers of x / x2 whose only consumer is this conv: their reductions ride on this conv's dX epilogue
  const int C2 = a->Cin - a->Cin1;
  const BnProducer p1 = producer_of(a->p_conv_out, a->p_stats, a->p_bn_w, a->p_bn_b, a->p_bn_ws, a->Cin1);
  const BnProducer p2 = producer_of(a->p2_conv_out, a->p2_stats, a->p2_bn_w, a->p2_bn_b, a->p2_bn_ws, C2);
  const bool fold = a->training && a->dx && (p1.x || p2.x);
  if (a->groups > 1) {       // depth-wise unit (see the forward): dX / dW of the stencil; no producer folding, no virtual concat
    if (a->groups != a->Cin || a->Cin != C || a->x2 || fold || a->ldx != a->Cin || (a->dx && a->lddx != a->Cin)) return SAST_EINVAL;
    int rc = dwconv_bwd_launch(a->x, a->w, dconv, a->dx, a->dw, nullptr, a->B, DwGeom{a->H, a->W, g.Ho, g.Wo, C, k, a->stride}, st);
    if (rc) return rc;
    SAST_CHECK_LAUNCH();
    return SAST_OK;
  }
  if (fold && (a->stride != 1 || (p1.x && !complete(p1)) || (p2.x && !(a->x2 && complete(p2))))) return SAST_EINVAL;
  const auto pair_1x1 = [&](const auto& tb, const auto& ep) {   // (dW || dX) of a 1x1 stride-1 conv: dW over the rows tb reads, dX = dconv W
    return gemm_pair(LdRowsT{dconv, C}, tb, a->dw, K, C, K, M, nullptr, nullptr, LdRows{dconv, C, nullptr}, LdWeightNN{a->w, K}, ep, M, a->Cin, C,
                     nullptr, st, pair_tn_blocks_1x1());
  };
  if (k == 1 && a->stride == 1 && a->x2) {   // virtual concat input: dW over [x | x2], dX split into the two gradients
    const LdRowsT2 tb{a->x, a->ldx, a->Cin1, a->x2, a->ldx2};
    if (!a->dx) return gemm_tn(LdRowsT{dconv, C}, tb, a->dw, K, C, K, M, st);
    if (a->lddx != a->Cin1) return SAST_EINVAL;
    if (fold && ((p1.x && a->ldx != a->Cin1) || (p2.x && (a->ldx2 != C2 || !a->dx2)))) return SAST_EINVAL;
    return with_dx_epilogue(fold, EpSplit2{a->dx, a->dx2, a->Cin1, C2}, EpSplit2BnRed{a->dx, a->dx2, a->Cin1, C2, p1, p2},
                            [&](const auto& ep) { return pair_1x1(tb, ep); });
  }
  if (k == 1 && a->stride == 1) {
    if (!a->dx) return gemm_tn(LdRowsT{dconv, C}, LdRowsT{a->x, a->ldx}, a->dw, K, C, K, M, st);
    if (fold && (a->lddx != a->Cin || a->ldx != a->Cin)) return SAST_EINVAL;
    return with_dx_epilogue(fold, EpStore{a->dx, a->lddx, nullptr}, EpStoreBnRed{a->dx, a->lddx, p1},
                            [&](const auto& ep) { return pair_1x1(LdRowsT{a->x, a->ldx}, ep); });
  }
  return conv_bwd_pair(dconv, a->x, g, C, a->w, a->dw, a->dx, a->lddx, st, fold ? &p1 : nullptr);
}

// ------------------------------------------------------------------ two 1x1 conv + BN + SiLU of the same input
int sast_conv_bn_silu2_fwd(const SastConvBn2Args* a, sast_stream_t stream) { SAST_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  // (Cin1 == Cin, one source, accepted here; the single unit refuses it next to an x2)
  if (!a || a->Cin % 4 || a->Cout % 4 || a->Cin1 % 4 || a->Cin1 <= 0 || a->Cin1 > a->Cin || (a->Cin1 < a->Cin && !a->x2)) return SAST_EINVAL;
  ProfScope ps_("convbn2_fwd", a->Cout * 10 + 1, a->B * a->H * a->W, st);
  const int M = a->B * a->H * a->W, C = a->Cout;
  const LdRows2 src{a->x, a->ldx, a->Cin1, a->Cin1 < a->Cin ? a->x2 : nullptr, a->ldx2};
  if (!a->training) {   // inference: one launch, nothing kept
    if (!a->run_mean0 || !a->run_var0 || !a->run_mean1 || !a->run_var1 || (a->ksize != 1 && a->ksize != 3)) return SAST_EINVAL;
    const EpBnSilu2 ep{a->y0, a->y1, C, a->run_mean0, a->run_var0, a->bn_w0, a->bn_b0, a->eps0, a->run_mean1, a->run_var1, a->bn_w1, a->bn_b1, a->eps1};
    if (a->ksize == 3 && a->Cin1 != a->Cin) return SAST_EINVAL;
    const int K = a->ksize * a->ksize * a->Cin;
    return conv_fwd_gemm<false>(geom_of(a->B, a->H, a->W, a->Cin, a->ksize, 1, a->ksize / 2, 0, a->ldx), src, LdWeightNT2{a->w0, a->w1, K, C}, ep, M,
                                2 * C, K, st);
  }
  if (a->ksize != 1 && !(a->ksize == 3 && a->Cin1 == a->Cin)) return SAST_EINVAL;
  const int K = a->ksize * a->ksize * a->Cin;
  if (!a->bn_ws_zeroed) {
    zero_fill(a->bn_ws0, sizeof(float) * SAST_BN_WS_FLOATS(C), st);
    zero_fill(a->bn_ws1, sizeof(float) * SAST_BN_WS_FLOATS(C), st);
  }
  const EpStoreStats2 ep{a->conv_out0, a->conv_out1, C, (double*)a->bn_ws0, (double*)a->bn_ws1};
  int rc = conv_fwd_gemm<false>(geom_of(a->B, a->H, a->W, a->Cin, a->ksize, 1, a->ksize / 2, 0, a->ldx), src, LdWeightNT2{a->w0, a->w1, K, C}, ep, M,
                                2 * C, K, st);
  if (rc) return rc;
  const BnFwdJob j0{a->conv_out0, (const double*)a->bn_ws0, a->run_mean0, a->run_var0, a->stats0, a->bn_w0, a->bn_b0, a->y0, C, a->momentum0, a->eps0};
  const BnFwdJob j1{a->conv_out1, (const double*)a->bn_ws1, a->run_mean1, a->run_var1, a->stats1, a->bn_w1, a->bn_b1, a->y1, C, a->momentum1, a->eps1};
  bn_fwd_apply_launch(j0, j1, 2, M, M, C, 1, st);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_conv_bn_silu2_bwd(const SastConvBn2Args* a, sast_stream_t stream) { SAST_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  if (!a || (a->Cin1 < a->Cin && !a->x2)) return SAST_EINVAL;
  ProfScope ps_("convbn2_bwd", a->Cout * 10 + 1, a->B * a->H * a->W, st);
  if (a->ksize != 1 && !(a->ksize == 3 && a->Cin1 == a->Cin)) return SAST_EINVAL;
  const int M = a->B * a->H * a->W, K = a->ksize * a->ksize * a->Cin, C = a->Cout, C2 = a->Cin - a->Cin1;
  float* sums0 = a->bn_ws0 + 4 * BN_STAT_COPIES * C;
  float* sums1 = a->bn_ws1 + 4 * BN_STAT_COPIES * C;
  if (!a->bn_ws_zeroed) {
    if (a->bn_red_done0 || a->bn_red_done1) return SAST_EINVAL;
    zero_fill(sums0, sizeof(float) * 2 * BN_STAT_COPIES * C, st);
    zero_fill(sums1, sizeof(float) * 2 * BN_STAT_COPIES * C, st);
  }
  float* dconv = a->ws0;     // [M, 2C]: rows [dconv0 | dconv1]
  const BnBwdJob j0{a->conv_out0, a->stats0, a->bn_w0, a->bn_b0, a->dy0, C, sums0, dconv, a->d_bn_w0, a->d_bn_b0, nullptr, 2 * C};
  const BnBwdJob j1{a->conv_out1, a->stats1, a->bn_w1, a->bn_b1, a->dy1, C, sums1, dconv + C, a->d_bn_w1, a->d_bn_b1, nullptr, 2 * C};
  if (!a->bn_red_done0 && !a->bn_red_done1) bn_bwd_reduce_launch(j0, j1, 2, M, C, st);
  else if (!a->bn_red_done0) bn_bwd_reduce_launch(j0, j0, 1, M, C, st);
  else if (!a->bn_red_done1) bn_bwd_reduce_launch(j1, j1, 1, M, C, st);
  bn_bwd_apply_launch(j0, j1, 2, M, C, 1, st);
  SAST_CHECK_LAUNCH();
  // dW of both convs: [dconv0 | dconv1]^T [x | x2] -> (dw0, dw1);  dX = [dconv0 | dconv1] [w0; w1]
  const LdRowsT ta{dconv, 2 * C};
  const EpAtomic2 ep1{a->dw0, a->dw1, K, C};
  const BnProducer p1 = producer_of(a->p_conv_out, a->p_stats, a->p_bn_w, a->p_bn_b, a->p_bn_ws, a->Cin1);
  if (a->ksize == 3) {   // two 3x3 stride-1 convs (the first convs of the two YOLOX head towers)
    const ConvGeom g = geom_of(a->B, a->H, a->W, a->Cin, 3, 1, 1, 0, a->ldx);
    const LdIm2colT tbc{a->x, g};
    if (!a->dx) return launch_gemm_split<TileSplitR>(ta, tbc, ep1, 2 * C, K, M, nullptr, tn_splits(2 * C, K, M), nullptr, st);
    const unsigned shift = div_mul_of((unsigned)(2 * C), 9ull * 2 * C);
    if (!shift || !g.cin_mul) return SAST_EINVAL;
    const LdConvDx lac{dconv, g, 2 * C, 2 * C, shift};
    const LdWeightConvDx2 lbc{a->w0, a->w1, 2 * C, C, 9, a->Cin, shift};
    if (p1.x && (a->ldx != a->Cin || !complete(p1))) return SAST_EINVAL;
    return with_dx_epilogue(p1.x != nullptr, EpStore{a->dx, a->Cin, nullptr}, EpStoreBnRed{a->dx, a->Cin, p1}, [&](const auto& ep) {
      return gemm_pair_ep(ta, tbc, ep1, 2 * C, K, M, nullptr, nullptr, lac, lbc, ep, M, a->Cin, 9 * 2 * C, nullptr, st, pair_tn_blocks_conv());
    });
  }
  const LdRowsT2 tb{a->x, a->ldx, a->Cin1, C2 > 0 ? a->x2 : nullptr, a->ldx2};
  if (!a->dx) return launch_gemm_split<TileSplitR>(ta, tb, ep1, 2 * C, K, M, nullptr, tn_splits(2 * C, K, M), nullptr, st);
  if (C2 > 0 && !a->dx2) return SAST_EINVAL;
  const LdRows la{dconv, 2 * C, nullptr};
  const LdWeightNN2 lb{a->w0, a->w1, K, C};
  const BnProducer p2 = producer_of(a->p2_conv_out, a->p2_stats, a->p2_bn_w, a->p2_bn_b, a->p2_bn_ws, C2);
  if ((p1.x && (a->ldx != a->Cin1 || !complete(p1))) || (p2.x && (C2 <= 0 || a->ldx2 != C2 || !complete(p2)))) return SAST_EINVAL;
  return with_dx_epilogue(p1.x || p2.x, EpSplit2{a->dx, a->dx2, a->Cin1, C2}, EpSplit2BnRed{a->dx, a->dx2, a->Cin1, C2, p1, p2}, [&](const auto& ep) {
    return gemm_pair_ep(ta, tb, ep1, 2 * C, K, M, nullptr, nullptr, la, lb, ep, M, K, 2 * C, nullptr, st, pair_tn_blocks_1x1());
  });
}

// ------------------------------------------------------------------ upsample / concat
int sast_upsample_cat_fwd(const float* a, const float* b, float* out, int B, int H, int W, int C1, int C2, sast_stream_t stream) { SAST_ENTRY();
  if (C1 % 4 || C2 % 4) return SAST_EINVAL;
  const size_t n4 = (size_t)B * 4 * H * W * ((C1 + C2) / 4);
  if (n4 < (1ull << 32)) SAST_LAUNCH(upsample_cat_fwd_kernel<unsigned>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, H, W, C1, C2, n4);
  else SAST_LAUNCH(upsample_cat_fwd_kernel<size_t>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, H, W, C1, C2, n4);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}
int sast_upsample_cat_bwd(const float* dout, float* da, float* db, int B, int H, int W, int C1, int C2, sast_stream_t stream) { SAST_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  if (C1 % 4 || C2 % 4) return SAST_EINVAL;
  const size_t n4 = (size_t)B * H * W * (C1 / 4), n4b = (size_t)B * 4 * H * W * (C2 / 4);
  if (n4 + n4b < (1ull << 32)) SAST_LAUNCH(upsample_cat_bwd_kernel<unsigned>, dim3((unsigned)((n4 + n4b + 255) / 256)), dim3(256), 0, st, dout, da, db, H, W, C1, C1 + C2, n4,
                     n4b);
  else SAST_LAUNCH(upsample_cat_bwd_kernel<size_t>, dim3((unsigned)((n4 + n4b + 255) / 256)), dim3(256), 0, st, dout, da, db, H, W, C1, C1 + C2, n4,
                     n4b);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}
int sast_cat2_fwd(const float* a, const float* b, float* out, int rows, int C1, int C2, sast_stream_t stream) { SAST_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  if (C1 % 4 || C2 % 4) return SAST_EINVAL;
  int rc = slice_copy(a, C1, 0, out, C1 + C2, 0, C1, rows, st);
  if (rc) return rc;
  return slice_copy(b, C2, 0, out, C1 + C2, C1, C2, rows, st);
}
int sast_cat2_bwd(const float* dout, float* da, float* db, int rows, int C1, int C2, sast_stream_t stream) { SAST_ENTRY();
  hipStream_t st = (hipStream_t)stream;
  int rc = slice_copy(dout, C1 + C2, 0, da, C1, 0, C1, rows, st);
  if (rc) return rc;
  return slice_copy(dout, C1 + C2, C1, db, C2, 0, C2, rows, st);
}

int sast_adamw(float* p, const float* g, float* m, float* v, size_t n, const float* lr_step, double beta1, double beta2, float eps,
               float weight_decay, float grad_scale, float clip_value, sast_stream_t stream) { SAST_ENTRY();
  if (n % 4) return SAST_EINVAL;
  const size_t n4 = n / 4;
  SAST_LAUNCH(adamw_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n4, lr_step, beta1,
                     beta2, eps, weight_decay, grad_scale, clip_value, OneCycle{0, 0, 0, 0, 0, 0});
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}
int sast_adamw_onecycle(float* p, const float* g, float* m, float* v, size_t n, float* lr_step, double beta1, double beta2, float eps,
                        float weight_decay, float grad_scale, float clip_value, double initial_lr, double max_lr, double min_lr,
                        double end1, double end2, sast_stream_t stream) { SAST_ENTRY();
  if (n % 4 || !(end2 > end1)) return SAST_EINVAL;
  const size_t n4 = n / 4;
  const OneCycle oc{1, initial_lr, max_lr, min_lr, end1, end2};
  SAST_LAUNCH(adamw_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n4, lr_step, beta1,
                     beta2, eps, weight_decay, grad_scale, clip_value, oc);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

#ifdef SAST_TL_ENABLE
// variant builds only: per-block phase stamps of the LAST GEMM launch of this translation unit (conv / FPN kernels)
int sast_tl_reset(void) { SAST_ENTRY();
  static unsigned long long zeros[8 * 8192];
  return hipMemcpyToSymbol(HIP_SYMBOL(sast_tl_buf), zeros, sizeof(zeros)) == hipSuccess ? 0 : -5;
}
int sast_tl_read(unsigned long long* host_out, int nblocks) { SAST_ENTRY();
  if (nblocks > 8192) nblocks = 8192;
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(sast_tl_buf), sizeof(unsigned long long) * 8 * nblocks) == hipSuccess ? 0 : -5;
}
#endif

}  // extern "C"
