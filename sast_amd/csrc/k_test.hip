// micro-benchmark / unit-test entry points for the GEMM template, the window-attention launchers on their own
// (sast_test_attn_fwd / sast_test_attn_bwd: tests/test_attn_operators.py) and the elementwise helpers of common.cuh on their own
// (sast_test_glu_act / sast_test_unary: tests/test_act_operators.py); not used by the product path
#include <hip/hip_runtime.h>
// phase timestamps (100 MHz wall clock) of every block of the LAST instrumented launch: only the kernel instantiations of
// this translation unit carry them (they use the test-only epilogues below, so no product kernel is affected)
__device__ unsigned long long sast_tl_buf[8 * 8192];
#define SAST_TL(k)                                                                                          \
  do {                                                                                                      \
    const unsigned bid_ = blockIdx.y * gridDim.x + blockIdx.x;                                              \
    if (threadIdx.x == 0 && bid_ < 8192) sast_tl_buf[bid_ * 8 + (k)] = wall_clock64();                      \
    if (threadIdx.x == 0 && bid_ < 8192 && (k) == 0) sast_tl_buf[bid_ * 8 + 7] = __smid();                 \
  } while (0)
// fine-grained attribution inside the k-loop (variant builds with -DSAST_TLF_ENABLE only: the clock reads perturb the schedule):
// shader-clock cycles of wave 0 of every block spent in [0] issuing the global loads, [1] LDS operand reads + MFMA issue, [2] the wait
// for the older tile + split + LDS store, [3] the barrier; [4] = phases counted
#ifdef SAST_TLF_ENABLE
__device__ unsigned long long sast_tlf_buf[8 * 8192];
#define SAST_TLF_DECL long long tlf_acc_[6] = {0, 0, 0, 0, 0, 0}; long long tlf_prev_ = clock64();
#define SAST_TLF(k) do { const long long t_ = clock64(); tlf_acc_[k] += t_ - tlf_prev_; tlf_prev_ = t_; } while (0)
#define SAST_TLF_COUNT() do { tlf_acc_[4] += 1; } while (0)
#define SAST_TLF_WAIT_OLDER(n) do { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory"); const long long t_ = clock64(); tlf_acc_[5] += t_ - tlf_prev_; tlf_prev_ = t_; } while (0)
#define SAST_TLF_FLUSH()                                                                                    \
  do {                                                                                                      \
    const unsigned bid_ = blockIdx.y * gridDim.x + blockIdx.x;                                              \
    if (threadIdx.x == 0 && bid_ < 8192) for (int q_ = 0; q_ < 6; ++q_) sast_tlf_buf[bid_ * 8 + q_] = tlf_acc_[q_]; \
  } while (0)
#endif
#include "gemm.cuh"
#include "gemm_dispatch.cuh"
#include "kernels.h"
using namespace sast;
#ifdef SAST_TLF_ENABLE
extern "C" int sast_test_tlf(unsigned long long* host_out, int nblocks) {
  if (nblocks > 8192) nblocks = 8192;
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(sast_tlf_buf), sizeof(unsigned long long) * 8 * nblocks) == hipSuccess ? 0 : -5;
}
#endif

extern "C" int sast_test_timeline_reset(void) {
  static unsigned long long zeros[8 * 8192];
  return hipMemcpyToSymbol(HIP_SYMBOL(sast_tl_buf), zeros, sizeof(zeros)) == hipSuccess ? 0 : -5;
}
extern "C" int sast_test_timeline(unsigned long long* host_out, int nblocks) {
  if (nblocks > 8192) nblocks = 8192;
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(sast_tl_buf), sizeof(unsigned long long) * 8 * nblocks) == hipSuccess ? 0 : -5;
}

struct EpStoreT : EpStore {  // distinct type: keeps the instrumented instantiations apart from the product's
  EpStoreT(float* c_, int ld_, const float* b_) : EpStore{c_, ld_, b_} {}
};

struct EpAtomicNT {  // c += v (grid-level split of the reduction of a plain GEMM: the output must be zero on entry; bias ignored)
  float* c; int ldc;
  using Col = EpNone; using Aux = EpNone;
  __device__ __forceinline__ Col col(int) const { return Col{}; }
  __device__ __forceinline__ Aux pre(int, int) const { return Aux{}; }
  __device__ __forceinline__ void post(int m, int j, const float (&v)[1], const Col&, const Aux&) const { atomicAdd(c + (size_t)m * ldc + j, v[0]); }
};

// dM (optional): the device-side row count of gemm.cuh; the grid-split kinds (tile >= 600) have none
static int test_gemm_nt(const float* a, const float* w, const float* bias, float* c, int M, int N, int K, int tile, const int* dM,
                        hipStream_t st) {
  if (dM && tile >= 600) return SAST_EINVAL;
  const LdRows la{a, K, nullptr};
  const LdWeightNT lb{w, K, 0};
  const EpStoreT ep(c, N, bias);
  // LARGE tiles with the reduction split over the GRID (atomic epilogue into a zeroed output): tile = 100 * kind + splits,
  // kind 6 = 128x128 (4 waves of 64x64), 7 = 64x128 (4 waves of 32x64), 8 = 128x64 (4 waves of 32x64)
  // round 4: the SHIPPED small tiles (intra-workgroup k-groups) with an additional grid-level split: kind 9 = 32x64 with 4 k-groups,
  // 10 = 32x32 with 8 k-groups, 11 = 64x64 with 2 k-groups (tools/gemm_gridsplit_small.py)
  if (tile >= 600 && tile < 1200) {
    const int splits = tile % 100;
    const EpAtomicNT ea{c, N};
    switch (tile / 100) {
      case 6: return launch_gemm_split<TileBig>(la, lb, ea, M, N, K, nullptr, splits, nullptr, st);
      case 7: return launch_gemm_split<TileMid>(la, lb, ea, M, N, K, nullptr, splits, nullptr, st);
      case 8: return launch_gemm_split<TileN64>(la, lb, ea, M, N, K, nullptr, splits, nullptr, st);
      case 9: return launch_gemm_split<Tile<32, 64, 1, 2, 1, 16, 4>>(la, lb, ea, M, N, K, nullptr, splits, nullptr, st);
      case 10: return launch_gemm_split<Tile<32, 32, 1, 1, 1, 16, 8>>(la, lb, ea, M, N, K, nullptr, splits, nullptr, st);
      case 11: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 2>>(la, lb, ea, M, N, K, nullptr, splits, nullptr, st);
    }
  }
  switch (tile) {
    case 0: return launch_gemm<TileSmall>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 1: return launch_gemm<TileMid>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 2: return launch_gemm<TileBig>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 3: return launch_gemm<TileN64>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 4: return launch_gemm<Tile<64, 64, 2, 2, 1, 32>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 5: return launch_gemm<Tile<64, 128, 2, 2, 1, 32>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 6: return launch_gemm<Tile<128, 128, 2, 2, 1, 32>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 7: return launch_gemm<Tile<128, 64, 2, 2, 1, 32>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 8: return launch_gemm<Tile<128, 64, 2, 2, 1, 16>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 9: return launch_gemm<TileTiny>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 10: return launch_gemm<Tile<32, 64, 1, 2, 1, 16>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 11: return launch_gemm<Tile<64, 32, 2, 1, 1, 16>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 13: return launch_gemm<TileSmallK2>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 14: return launch_gemm<TileSmallK4>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 15: return launch_gemm<Tile<64, 64, 2, 2, 1, 32, 2>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 16: return launch_gemm<Tile<64, 64, 2, 2, 1, 32, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 17: return launch_gemm<Tile<32, 32, 1, 1, 1, 16, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 18: return launch_gemm<Tile<32, 32, 1, 1, 1, 16, 8>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 19: return launch_gemm<Tile<32, 64, 1, 2, 1, 16, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 12: return launch_gemm<Tile<32, 32, 1, 1, 1, 32>>(la, lb, ep, M, N, K, dM, nullptr, st);
    // deeper register prefetch for the small grids (<= one workgroup per CU: occupancy is not what the registers cost there)
    case 50: return launch_gemm<Tile<32, 64, 1, 2, 1, 16, 4, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 51: return launch_gemm<Tile<32, 64, 1, 2, 1, 16, 4, 6>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 52: return launch_gemm<Tile<32, 64, 1, 2, 1, 16, 4, 8>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 53: return launch_gemm<Tile<32, 32, 1, 1, 1, 16, 8, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 54: return launch_gemm<Tile<32, 32, 1, 1, 1, 16, 8, 6>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 55: return launch_gemm<Tile<64, 64, 2, 2, 1, 16, 2, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 56: return launch_gemm<Tile<64, 64, 2, 2, 1, 16, 2, 6>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 57: return launch_gemm<Tile<64, 64, 2, 2, 1, 16, 1, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 58: return launch_gemm<Tile<64, 64, 2, 2, 1, 16, 4, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    // 32-wide k-tiles on presplit operands (two k16 steps per phase)
    case 40: return launch_gemm<Tile<64, 64, 2, 2, 1, 32, 1>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 41: return launch_gemm<Tile<64, 64, 2, 2, 1, 32, 2>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 42: return launch_gemm<Tile<32, 64, 1, 2, 1, 32, 2>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 43: return launch_gemm<Tile<32, 64, 1, 2, 1, 32, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 44: return launch_gemm<Tile<64, 128, 2, 2, 1, 32, 1>>(la, lb, ep, M, N, K, dM, nullptr, st);
    // wave-private tiles: one wave per k-group, no barrier in the k-loop
    case 30: return launch_gemm<Tile<64, 64, 1, 1, 1, 16, 1>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 31: return launch_gemm<Tile<64, 64, 1, 1, 1, 16, 2>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 32: return launch_gemm<Tile<64, 64, 1, 1, 1, 16, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 33: return launch_gemm<Tile<32, 64, 1, 1, 1, 16, 1>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 34: return launch_gemm<Tile<32, 64, 1, 1, 1, 16, 2>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 35: return launch_gemm<Tile<32, 64, 1, 1, 1, 16, 4>>(la, lb, ep, M, N, K, dM, nullptr, st);
    case 36: return launch_gemm<Tile<32, 32, 1, 1, 1, 16, 2>>(la, lb, ep, M, N, K, dM, nullptr, st);
    default: return SAST_EINVAL;
  }
}
extern "C" int sast_test_gemm_nt(const float* a, const float* w, const float* bias, float* c, int M, int N, int K, int tile,
                                 sast_stream_t stream) {
  return test_gemm_nt(a, w, bias, c, M, N, K, tile, nullptr, (hipStream_t)stream);
}
extern "C" int sast_test_gemm_nt_dev(const float* a, const float* w, const float* bias, float* c, int M, int N, int K, int tile,
                                     const int* dM, sast_stream_t stream) {
  return test_gemm_nt(a, w, bias, c, M, N, K, tile, dM, (hipStream_t)stream);
}

struct EpNull {  // discards the result (measures the kernel without the atomic epilogue)
  float* c;
  using Col = EpNone; using Aux = EpNone;
  __device__ __forceinline__ Col col(int) const { return Col{}; }
  __device__ __forceinline__ Aux pre(int, int) const { return Aux{}; }
  __device__ __forceinline__ void post(int, int, const float (&v)[1], const Col&, const Aux&) const {
    if (v[0] == 123456.789f) c[0] = v[0];
  }
};

struct EpAtomicT {  // same as EpAtomic, distinct type (instrumented instantiation)
  float* c; int ldc;
  using Col = EpNone; using Aux = EpNone;
  __device__ __forceinline__ Col col(int) const { return Col{}; }
  __device__ __forceinline__ Aux pre(int, int) const { return Aux{}; }
  __device__ __forceinline__ void post(int m, int j, const float (&v)[1], const Col&, const Aux&) const {
    atomicAdd(c + (size_t)m * ldc + j, v[0]);
  }
};

// diagnostic loaders: no memory access at all (what is left is LDS traffic + barriers + MFMA), and loads without the LDS/MFMA part
struct LdNullT {
  static constexpr bool RC = false;
  struct Ctx { int i; bool ok; };
  __device__ __forceinline__ Ctx prep(int i, int Ieff) const { return Ctx{i, i < Ieff}; }
  __device__ __forceinline__ Ctx prep(int j, int, int NJ) const { return Ctx{j, j < NJ}; }
  __device__ __forceinline__ void load(const Ctx& c, int r, int Reff, float4& v, float& aux, bool& ok) const {
    ok = c.ok && r < Reff;
    v = make_float4((float)(r & 7), 1.f, (float)(c.i & 3), 0.5f);
    aux = 0.f;
  }
  SAST_DEFAULT_FINISH
};

// dR (optional): the device-side length of the reduction
static int test_gemm_tn(const float* dy, const float* x, float* out, float* colsum, int Mo, int NJ, int R, int tile, int splits,
                        int null_ep, const int* dR, hipStream_t st) {
  const LdRowsT la{dy, Mo};
  const LdRowsT lb{x, NJ};
  if (null_ep) {
    const EpNull ep{out};
    switch (tile) {
      case 0: return launch_gemm_split<TileSmall>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
      case 1: return launch_gemm_split<TileSmallK2>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
      case 2: return launch_gemm_split<TileSmallK4>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    }
  }
  const EpAtomicT ep{out, NJ};
  if (tile == 50) return launch_gemm_split<Tile<64, 64, 2, 1, 1, 16, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);   // wave tile 32x64, 2 k-groups, 4 waves
  if (tile == 51) return launch_gemm_split<Tile<64, 64, 2, 1, 1, 16, 4>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);   // wave tile 32x64, 4 k-groups, 8 waves
  if (tile == 52) return launch_gemm_split<Tile<64, 64, 1, 2, 1, 16, 4>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);   // wave tile 64x32, 4 k-groups
  if (tile == 53) return launch_gemm_split<Tile<64, 64, 1, 1, 1, 16, 4>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);   // wave tile 64x64, 4 k-groups, 4 waves
  if (tile == 54) return launch_gemm_split<Tile<64, 64, 1, 1, 1, 16, 8>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);   // wave tile 64x64, 8 k-groups, 8 waves
  if (tile == 40) return launch_gemm_split<Tile<64, 64, 2, 2, 1, 32, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);   // BK = 32
  if (tile == 41) return launch_gemm_split<Tile<64, 64, 2, 2, 1, 32, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
  if (tile == 42) return launch_gemm_split<Tile<64, 64, 2, 2, 1, 64, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);   // BK = 64
  if (tile == 43) return launch_gemm_split<Tile<64, 64, 2, 2, 1, 64, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
  if (tile == 100) return launch_gemm_split<TileSmallK2>(LdNullT{}, LdNullT{}, ep, Mo, NJ, R, dR, splits, colsum, st);   // no global loads
  if (tile == 101) return launch_gemm_split<TileSmall>(LdNullT{}, LdNullT{}, ep, Mo, NJ, R, dR, splits, colsum, st);
  if (tile == 102) return launch_gemm_split<TileSmallK2>(la, LdNullT{}, ep, Mo, NJ, R, dR, splits, colsum, st);          // A only
  switch (tile) {
    case 0: return launch_gemm_split<TileSmall>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 1: return launch_gemm_split<TileSmallK2>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 2: return launch_gemm_split<TileSmallK4>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 20: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 2, 4, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 21: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 2, 4, 3>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 22: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 2, 6, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 23: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 2, 8, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 24: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 1, 4, 4>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 25: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 1, 8, 3>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 26: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 4, 4, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 27: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 2, 2, 4>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 28: return launch_gemm_split<Tile<64, 64, 2, 2, 1, 16, 1, 2, 8>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 30: return launch_gemm_split<Tile<128, 64, 2, 2, 1, 16, 1, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 32: return launch_gemm_split<Tile<64, 128, 2, 2, 1, 16, 1, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 33: return launch_gemm_split<Tile<128, 128, 2, 2, 1, 16, 1, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 34: return launch_gemm_split<Tile<192, 64, 2, 2, 1, 16, 1, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 35: return launch_gemm_split<Tile<128, 64, 4, 1, 1, 16, 1, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 36: return launch_gemm_split<Tile<128, 64, 4, 2, 1, 16, 1, 2>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 3: return launch_gemm_split<Tile<128, 128, 2, 2, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 4: return launch_gemm_split<Tile<192, 64, 2, 2, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 5: return launch_gemm_split<Tile<320, 64, 2, 2, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 6: return launch_gemm_split<Tile<64, 192, 2, 2, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 7: return launch_gemm_split<Tile<192, 128, 2, 2, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    case 8: return launch_gemm_split<Tile<128, 64, 2, 2, 1>>(la, lb, ep, Mo, NJ, R, dR, splits, colsum, st);
    default: return SAST_EINVAL;
  }
}
extern "C" int sast_test_gemm_tn(const float* dy, const float* x, float* out, float* colsum, int Mo, int NJ, int R, int tile, int splits,
                                 int null_ep, sast_stream_t stream) {
  return test_gemm_tn(dy, x, out, colsum, Mo, NJ, R, tile, splits, null_ep, nullptr, (hipStream_t)stream);
}
extern "C" int sast_test_gemm_tn_dev(const float* dy, const float* x, float* out, float* colsum, int Mo, int NJ, int R, int tile, int splits,
                                     const int* dR, sast_stream_t stream) {
  return test_gemm_tn(dy, x, out, colsum, Mo, NJ, R, tile, splits, 0, dR, (hipStream_t)stream);
}

// ---- the host-side dispatch of gemm_dispatch.cuh on its own (tests/test_gemm_exact.py): the knobs pick the tile
// c[M, N] = a[M, K] w[N, K]^T + bias through gemm_auto, with the product's loaders and epilogue
extern "C" int sast_test_gemm_auto(const float* a, const float* w, const float* bias, float* c, int M, int N, int K, const int* dM,
                                   sast_stream_t stream) {
  return gemm_auto(LdRows{a, K, nullptr}, LdWeightNT{w, K, 0}, EpStore{c, N, bias}, M, N, K, dM, (hipStream_t)stream);
}
// the backward of y[R, N] = x[R, K] w[N, K]^T as sast_mswsa_bwd issues it for `proj`: dw[N, K] += dy^T x, db[N] += column sums of dy (both
// zero on entry) and dx[R, K] = dy w, one paired launch (two with SAST_GEMM_PAIR=0); dcount: the device-side row count of both jobs
extern "C" int sast_test_gemm_pair(const float* dy, const float* x, const float* w, float* dw, float* db, float* dx, int R, int N, int K,
                                   const int* dcount, sast_stream_t stream) {
  return gemm_pair(LdRowsT{dy, N}, LdRowsT{x, K}, dw, K, N, K, R, dcount, db, LdRows{dy, N, nullptr}, LdWeightNN{w, K}, EpStore{dx, K, nullptr},
                   R, K, N, dcount, (hipStream_t)stream);
}
// the group tiles: c[m][g][j] = sum_k a[m][k] w[g * NJ + j][k], the weight [G * NJ, K] with group stride NJ.  tile: 0 TileG2, 1 TileG2K2,
// 2 TileG2K4, 3 TileG3, 4 TileG3K4, 5 TileG4, 6 TileG4K4 (the ones the product launches); G must be the tile's
template <int G>
struct EpGroupsT {  // c[m * G * NJ + g * NJ + j] = v[g]
  float* c; int NJ;
  using Col = EpNone; using Aux = EpNone;
  __device__ __forceinline__ Col col(int) const { return Col{}; }
  __device__ __forceinline__ Aux pre(int, int) const { return Aux{}; }
  __device__ __forceinline__ void post(int m, int j, const float (&v)[G], const Col&, const Aux&) const {
#pragma unroll
    for (int g = 0; g < G; ++g) c[((size_t)m * G + g) * NJ + j] = v[g];
  }
};
extern "C" int sast_test_gemm_groups(const float* a, const float* w, float* c, int M, int NJ, int K, int G, int tile, const int* dM,
                                     sast_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (tile < 0 || tile > 6 || G != (tile < 3 ? 2 : tile < 5 ? 3 : 4)) return SAST_EINVAL;
  const LdRows la{a, K, nullptr};
  const LdWeightNT lb{w, K, NJ};
  switch (tile) {
    case 0: return launch_gemm<TileG2>(la, lb, EpGroupsT<2>{c, NJ}, M, NJ, K, dM, nullptr, st);
    case 1: return launch_gemm<TileG2K2>(la, lb, EpGroupsT<2>{c, NJ}, M, NJ, K, dM, nullptr, st);
    case 2: return launch_gemm<TileG2K4>(la, lb, EpGroupsT<2>{c, NJ}, M, NJ, K, dM, nullptr, st);
    case 3: return launch_gemm<TileG3>(la, lb, EpGroupsT<3>{c, NJ}, M, NJ, K, dM, nullptr, st);
    case 4: return launch_gemm<TileG3K4>(la, lb, EpGroupsT<3>{c, NJ}, M, NJ, K, dM, nullptr, st);
    case 5: return launch_gemm<TileG4>(la, lb, EpGroupsT<4>{c, NJ}, M, NJ, K, dM, nullptr, st);
    default: return launch_gemm<TileG4K4>(la, lb, EpGroupsT<4>{c, NJ}, M, NJ, K, dM, nullptr, st);
  }
}


// ---- MFMA issue-rate calibration (tools/mfma_peak.py): what a wave / a SIMD sustains on v_mfma_f32_32x32x2_f32 with the loop
// structure of gemm_body (dependent chain on one accumulator, LDS operand reads, a workgroup barrier per 8 MFMAs)
template <int MODE>
__global__ __launch_bounds__(256) void mfma_peak_kernel(float* out, int iters) {
  __shared__ float lds[64 * 68 * 2];
  for (int i = threadIdx.x; i < 64 * 68 * 2; i += 256) lds[i] = (float)(i & 7) * 0.001f;
  __syncthreads();
  f32x16 acc0, acc1;
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
  const int lane = threadIdx.x & 63, l31 = lane & 31, hf = lane >> 5;
  float a[8], b[8];
  for (int k = 0; k < 8; ++k) { a[k] = lds[(hf * 8 + k) * 68 + l31]; b[k] = lds[64 * 68 + (hf * 8 + k) * 68 + l31]; }
  for (int it = 0; it < iters; ++it) {
    if (MODE == 2 || MODE == 4) {   // operands re-read from LDS every k-tile (ds_read_b32, [k][row] layout)
      const int o = (it & 1) * 4;
#pragma unroll
      for (int k = 0; k < 8; ++k) { a[k] = lds[(hf * 8 + k) * 68 + l31 + o]; b[k] = lds[64 * 68 + (hf * 8 + k) * 68 + l31 + o]; }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (MODE == 1 && (k & 1)) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[k], acc1, 0, 0, 0);
      else acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[k], acc0, 0, 0, 0);
    }
    if (MODE == 3 || MODE == 4) __syncthreads();
  }
  float s = 0.f;
  for (int e = 0; e < 16; ++e) s += acc0[e] + acc1[e];
  if (s == 123.456f) out[0] = s;
}
extern "C" int sast_test_mfma_peak(float* out, int mode, int blocks, int iters, sast_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  switch (mode) {
    case 0: SAST_LAUNCH(mfma_peak_kernel<0>, dim3(blocks), dim3(256), 0, st, out, iters); break;
    case 1: SAST_LAUNCH(mfma_peak_kernel<1>, dim3(blocks), dim3(256), 0, st, out, iters); break;
    case 2: SAST_LAUNCH(mfma_peak_kernel<2>, dim3(blocks), dim3(256), 0, st, out, iters); break;
    case 3: SAST_LAUNCH(mfma_peak_kernel<3>, dim3(blocks), dim3(256), 0, st, out, iters); break;
    case 4: SAST_LAUNCH(mfma_peak_kernel<4>, dim3(blocks), dim3(256), 0, st, out, iters); break;
    default: return SAST_EINVAL;
  }
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}


// ---- the window-attention launchers of k_attn_mfma.hip on their own (tests/test_attn_operators.py): qkv [rows, 3C] with head h at
// column 3 h dh as [q | k | v], o / dout [rows, C], lse [rows, heads], row_off the exclusive prefix sum of Kw; the backward runs
// without LayerScale-finish side workgroups; dbuf [rows, heads] is needed for T > 128.  Both return the launcher's code.
extern "C" int sast_test_attn_fwd(const float* qkv, float* o, float* lse, const int* row_off, const int* Kw, int W, int T, int C, int dh,
                                  sast_stream_t stream) {
  return attn_fwd_mfma_launch(qkv, o, lse, row_off, Kw, W, T, C, dh, (hipStream_t)stream);
}
extern "C" int sast_test_attn_bwd(const float* qkv, const float* dout, const float* lse, float* dqkv, const int* row_off, const int* Kw,
                                  int W, int T, int C, int dh, float* dbuf, sast_stream_t stream) {
  return attn_bwd_mfma_launch(qkv, dout, lse, dqkv, row_off, Kw, W, T, C, dh, (hipStream_t)stream, nullptr, nullptr, 0, dbuf);
}

// ---- the elementwise arithmetic of common.cuh on its own (tests/test_act_operators.py): the 14-way gate activation of the GLU-MLP
// epilogues with its derivative, and the fast-math helpers the conv, ConvLSTM, STP and GLU kernels share.  Both call the functions
// of common.cuh themselves; y / dy / x hold n floats.
__global__ __launch_bounds__(256) void test_glu_act_kernel(const float* __restrict__ g, float* __restrict__ y, float* __restrict__ dy, int n,
                                                           int act, float slope) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float v = g[i];
    y[i] = glu_act(v, act, slope);
    dy[i] = glu_act_grad(v, act, slope);
  }
}
extern "C" int sast_test_glu_act(const float* g, float* y, float* dy, int n, int act, float slope, sast_stream_t stream) {
  if (act < 0 || act >= GLU_ACT_COUNT || n < 0 || n > (1 << 30) || !g || !y || !dy) return SAST_EINVAL;      // (int index + grid stride)
  if (n == 0) return SAST_OK;
  const int blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  SAST_LAUNCH(test_glu_act_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, y, dy, n, act, slope);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}
// fn: 0 sigmoid_hw  1 tanh_hw  2 gelu_erf  3 gelu_erf_grad  4 softplus_t20  5 rsqrt_hw (positive inputs)  6 x * sigmoid_hw(x), the SiLU
// as the conv epilogues write it
constexpr int TEST_UNARY_COUNT = 7;
__device__ __forceinline__ float test_unary(float x, int fn) {
  switch (fn) {
    case 0: return sigmoid_hw(x);
    case 1: return tanh_hw(x);
    case 2: return gelu_erf(x);
    case 3: return gelu_erf_grad(x);
    case 4: return softplus_t20(x);
    case 5: return rsqrt_hw(x);
    default: return x * sigmoid_hw(x);
  }
}
__global__ __launch_bounds__(256) void test_unary_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int fn) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) y[i] = test_unary(x[i], fn);
}
extern "C" int sast_test_unary(const float* x, float* y, int n, int fn, sast_stream_t stream) {
  if (fn < 0 || fn >= TEST_UNARY_COUNT || n < 0 || n > (1 << 30) || !x || !y) return SAST_EINVAL;
  if (n == 0) return SAST_OK;
  const int blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  SAST_LAUNCH(test_unary_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, n, fn);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

// ---- launch-error latching (common.cuh: SAST_LAUNCH / SAST_CHECK_LAUNCH): a failed launch followed by good ones inside one entry
// point must still be reported by the single check at the end.  bad != 0: the first launch asks for 2048 threads per workgroup.
__global__ void latch_probe_kernel(int* p) { if (p && threadIdx.x == 0 && blockIdx.x == 0) p[0] += 1; }
extern "C" int sast_test_launch_latch(int* scratch, int bad, sast_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  SAST_LAUNCH(latch_probe_kernel, dim3(1), dim3(bad ? 2048 : 64), 0, st, scratch);
  SAST_LAUNCH(latch_probe_kernel, dim3(1), dim3(64), 0, st, scratch);
  SAST_LAUNCH(latch_probe_kernel, dim3(1), dim3(64), 0, st, scratch);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

// ---- where do float atomics of MANY workgroups to the SAME buffer cost?  Every workgroup (2 waves) adds `nfloats` values into one
// accumulation buffer, as the weight-gradient flush of a per-partition fused layer kernel would.  mode 0: one buffer shared by the
// whole chip; mode 1: one private copy per XCD (HW_REG_XCC_ID), so a line is only ever owned by one L2; mode 2: plain stores to a
// per-workgroup slice (the bandwidth floor); rot != 0: a workgroup starts at a rotated offset so that they do not hit the same
// lines at the same time.  out_xcc[block] = the XCD the workgroup ran on.
__device__ __forceinline__ int xcc_id() { return __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)); }   // hwreg(HW_REG_XCC_ID, 0, 4)
__global__ __launch_bounds__(128) void atomic_xcd_kernel(float* __restrict__ buf, int* __restrict__ out_xcc, int mode, int nfloats, int rot) {
  const int x = xcc_id();
  if (threadIdx.x == 0 && out_xcc) out_xcc[blockIdx.x] = x;
  float* dst = buf + (mode == 1 ? (size_t)x * nfloats : mode == 2 ? (size_t)blockIdx.x * nfloats : 0);
  const int start = rot ? (int)(((long long)blockIdx.x * 4099 * 128) % nfloats) : 0;
  for (int i = threadIdx.x; i < nfloats; i += 128) {
    int j = i + start; if (j >= nfloats) j -= nfloats;
    if (mode == 2) dst[j] = 1.0f; else atomicAdd(dst + j, 1.0f);
  }
}
extern "C" int sast_test_atomic_xcd(float* buf, int* out_xcc, int mode, int nfloats, int rot, int blocks, sast_stream_t stream) {
  SAST_LAUNCH(atomic_xcd_kernel, dim3(blocks), dim3(128), 0, (hipStream_t)stream, buf, out_xcc, mode, nfloats, rot);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

// ---- do the matrix pipe and the VALU of one SIMD overlap?  512 threads = two waves per SIMD (waves w and w + 4 share a SIMD).
// mode 0: every wave runs MFMA chains only; 1: VALU only; 2: waves 0-3 MFMA, waves 4-7 VALU (the pair on a SIMD is complementary);
// 3: every wave alternates 6 dependent MFMAs with NV independent VALU instructions (the shape of the fused layer kernels);
// 4: as 3 with TWO accumulator chains interleaved.  out[block] = shader-clock cycles of wave 0.
// round 5 -- modes 5 / 6: the SAME work per wave as 3 / 4 but in INTERLEAVED program order, one MFMA followed by NV / 6 VALU instructions
// (forced with sched_group_barrier: an in-order wave can only hide VALU work under an MFMA if the VALU instructions sit between two
// MFMAs in its instruction stream); 5: one accumulator chain, 6: two chains.
template <int MODE, int NV>
__global__ __launch_bounds__(512) void overlap_probe_kernel(float* __restrict__ out, long long* __restrict__ cyc, int iters) {
  using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;
  using f32x16_t = __attribute__((ext_vector_type(16))) float;
  const int w = threadIdx.x >> 6;
  f32x16_t acc0, acc1;
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
  bf16x8_t a, b;
  for (int e = 0; e < 8; ++e) { a[e] = (__bf16)(float)(threadIdx.x & 7); b[e] = (__bf16)1.0f; }
  float v[8];
  for (int e = 0; e < 8; ++e) v[e] = (float)threadIdx.x + e;
  const long long t0 = clock64();
  const bool do_m = MODE == 0 || (MODE == 2 && w < 4) || MODE >= 3, do_v = MODE == 1 || (MODE == 2 && w >= 4) || MODE >= 3;
  for (int it = 0; it < iters; ++it) {
    if constexpr (MODE == 5 || MODE == 6) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (MODE == 6 && (k & 1)) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc1, 0, 0, 0);
        else acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc0, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < NV / 6; ++q) v[(k * (NV / 6) + q) & 7] = fmaf(v[(k * (NV / 6) + q) & 7], 1.000001f, 0.5f);
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);          // one MFMA ...
        __builtin_amdgcn_sched_group_barrier(0x002, NV / 6, 0);     // ... then NV / 6 VALU
      }
      continue;
    }
    if (do_m) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (MODE == 4 && (k & 1)) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc1, 0, 0, 0);
        else acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc0, 0, 0, 0);
      }
    }
    if (do_v) {
#pragma unroll
      for (int k = 0; k < NV; ++k) v[k & 7] = fmaf(v[k & 7], 1.000001f, 0.5f);
    }
  }
  const long long t1 = clock64();
  float s = 0.f;
  for (int e = 0; e < 16; ++e) s += acc0[e] + acc1[e];
  for (int e = 0; e < 8; ++e) s += v[e];
  if (s == 123.456f) out[0] = s;
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}
extern "C" int sast_test_overlap_probe(float* out, long long* cyc, int mode, int nv, int blocks, int iters, sast_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  // mode + 10: the same with ONE wave per SIMD (256 threads)
  const int threads = mode >= 10 ? 256 : 512;
  mode %= 10;
#define OVL(M, V) SAST_LAUNCH((overlap_probe_kernel<M, V>), dim3(blocks), dim3(threads), 0, st, out, cyc, iters)
#define OVLS(V) switch (mode) { case 0: OVL(0, V); break; case 1: OVL(1, V); break; case 2: OVL(2, V); break; case 3: OVL(3, V); break; case 4: OVL(4, V); break; \
                                case 5: OVL(5, V); break; case 6: OVL(6, V); break; default: return SAST_EINVAL; }
  if (nv == 24) { OVLS(24) }
  else if (nv == 48) { OVLS(48) }
  else if (nv == 72) { OVLS(72) }
  else return SAST_EINVAL;
#undef OVL
#undef OVLS
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}
