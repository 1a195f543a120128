// Host-side tile / launch heuristics of the GEMM template, shared by k_block.hip and k_conv.hip:
//   gemm_auto  plain GEMM            64x64 tiles; 2-way intra-block k-split when the reduction is long; 32x64 tiles with a 4-way
//                                    k-split when the grid would give fewer than ~1.5 tiles per CU
//   gemm_tn    weight gradient       split-R job of ~SAST_TN_BLOCKS workgroups, atomic epilogue
//   gemm_pair  (dW, dX) of a layer   both in ONE launch (gemm.cuh: gemm_dual_kernel); SAST_GEMM_PAIR=0 restores two launches
// All thresholds were measured on the SAST shapes (tools/gemm_micro.py, gemm_tn_micro.py, gemm_small_m.py) and can be overridden
// through the environment for A/B runs.
#pragma once
#include <cstdlib>
#include "gemm.cuh"

namespace sast {

// the plain-GEMM tiles gemm_auto / the dX job of a paired launch choose from
using TileAutoThin = TileThinK4;
using TileAutoK2 = TileSmallK2;
using TileAutoK1 = TileSmall;

inline bool gemm_pair_enabled() { return SAST_KNOB("SAST_GEMM_PAIR", 1) != 0; }
inline int pair_tn_blocks() { return SAST_KNOB("SAST_TN_BLOCKS", 768); }
inline int pair_ks_min_r() { return SAST_KNOB("SAST_KS_MINR", 256); }
inline int pair_thin_nb() { return SAST_KNOB("SAST_THIN_NB", 384); }
inline int pair_ks_nb() { return SAST_KNOB("SAST_KS_NB", 1000000); }
// 32x32 tiles with 8 k-groups when even the 32x64 tiling leaves more than half of the CUs idle (PAFPN level-32 convs, M = 960)
inline int tiny_nb() { return SAST_KNOB("SAST_TINY_NB", 128); }
// (stand-alone launches only: as the dX job of a paired launch it measured slower, +0.02 ms/step)
inline bool use_tiny(int M, int NJ, int R) { return (long)((M + 31) / 32) * ((NJ + 63) / 64) <= tiny_nb() && R >= 512; }

// R_tile (optional): the reduction length the TILE is chosen for when the caller has cut a prefix of exact zeros off a longer reduction
// (ConvLSTM backward from a zero cell state): the same tile as the full-length call, and -- when the cut is a multiple of BK * KS, so
// that every k-group keeps its tiles -- the same summation order
template <class LA, class LB, class EP>
int gemm_auto(const LA& la, const LB& lb, const EP& ep, int M, int NJ, int R, const int* dM, hipStream_t st, int R_tile = 0) {
  const long nb = (long)((M + 63) / 64) * ((NJ + 63) / 64);
  const int Rt = R_tile > 0 ? R_tile : R;
  if (!dM && use_tiny(M, NJ, Rt)) return launch_gemm<TileTinyK8>(la, lb, ep, M, NJ, R, dM, nullptr, st);
  if (nb <= pair_thin_nb() && Rt >= pair_ks_min_r()) return launch_gemm<TileAutoThin>(la, lb, ep, M, NJ, R, dM, nullptr, st);
  if (nb <= pair_ks_nb() && Rt >= pair_ks_min_r()) return launch_gemm<TileAutoK2>(la, lb, ep, M, NJ, R, dM, nullptr, st);
  return launch_gemm<TileAutoK1>(la, lb, ep, M, NJ, R, dM, nullptr, st);
}
template <class LA, class LB, class EP>
int gemm_auto(const LA& la, const LB& lb, const EP& ep, int M, int NJ, int R, hipStream_t st) {
  return gemm_auto(la, lb, ep, M, NJ, R, nullptr, st);
}

// inside a paired launch the dW job shares the chip with the dX job: fewer, longer workgroups win (round 2, 4-wave split-R tile under the operand split: 192 measured best of 128 ... 512; round 1, 8-wave tile: 152; a target
// that adapts to the dX job's grid size was not better)
// the same for the k x k conv pairs (im2col / backward-data jobs)
inline int pair_tn_blocks_conv() { return SAST_KNOB("SAST_TN_BLOCKS_PAIRED_CONV", 192); }
// and for the 1x1 conv pairs of the FPN / head (k_conv.hip)
inline int pair_tn_blocks_1x1() { return SAST_KNOB("SAST_TN_BLOCKS_PAIRED_1X1", 192); }
inline int pair_tn_blocks_paired() { return SAST_KNOB("SAST_TN_BLOCKS_PAIRED", 192); }
// weight gradients of at most SAST_TN_SMALL_TILES output tiles (stage 1 / 2: 64x64 ... 128x128): every split adds its whole tile
// atomically, a same-line chain of `splits` atomic instructions (~25 ns each) -- their own target (0 = the general one)
inline int pair_tn_blocks_small() { return SAST_KNOB("SAST_TN_BLOCKS_PAIRED_SMALL", 0); }
inline int pair_tn_small_tiles() { return SAST_KNOB("SAST_TN_SMALL_TILES", 4); }

// target: workgroups of the weight-gradient job (it is split over the reduction until it has about that many)
inline int tn_splits(int Mo, int NJ, int R, int target = 0) {
  const int nb = ((Mo + 63) / 64) * ((NJ + 63) / 64);
  if (target <= 0) target = pair_tn_blocks();
  int splits = (target + nb - 1) / nb;
  const int max_splits = (R + 127) / 128;
  if (splits > max_splits) splits = max_splits;
  return splits < 1 ? 1 : splits;
}

// weight-gradient form: out[Mo, NJ] += A^T B over R rows (dR: device-side count), optional column sums of A (bias gradient)
template <class LA, class LB>
int gemm_tn(const LA& la, const LB& lb, float* out, int ldc, int Mo, int NJ, int R, const int* dR, float* colsum, hipStream_t st) {
  return launch_gemm_split<TileSplitR>(la, lb, EpAtomic{out, ldc}, Mo, NJ, R, dR, tn_splits(Mo, NJ, R), colsum, st);
}
template <class LA, class LB>
int gemm_tn(const LA& la, const LB& lb, float* out, int ldc, int Mo, int NJ, int R, hipStream_t st) {
  return gemm_tn(la, lb, out, ldc, Mo, NJ, R, nullptr, nullptr, st);
}

// job 1: out[Mo, NJ1] += A1^T B1 over R1 rows (dR1: device-side count), optional column sums of A1 (bias gradient)
// job 2: plain GEMM (M2 rows, device-side count dM2) with epilogue ep2
template <class LA1, class LB1, class EP1, class LA2, class LB2, class EP2>
int gemm_pair_ep(const LA1& la1, const LB1& lb1, const EP1& ep1, int Mo, int NJ1, int R1, const int* dR1, float* colsum,
                 const LA2& la2, const LB2& lb2, const EP2& ep2, int M2, int NJ2, int R2, const int* dM2, hipStream_t st, int tn_target = 0,
                 int R2_tile = 0);
template <class LA1, class LB1, class LA2, class LB2, class EP2>
int gemm_pair(const LA1& la1, const LB1& lb1, float* out, int ldc, int Mo, int NJ1, int R1, const int* dR1, float* colsum,
              const LA2& la2, const LB2& lb2, const EP2& ep2, int M2, int NJ2, int R2, const int* dM2, hipStream_t st, int tn_target = 0,
              int R2_tile = 0) {
  return gemm_pair_ep(la1, lb1, EpAtomic{out, ldc}, Mo, NJ1, R1, dR1, colsum, la2, lb2, ep2, M2, NJ2, R2, dM2, st, tn_target, R2_tile);
}
// the same with any accumulating epilogue for job 1
template <class LA1, class LB1, class EP1, class LA2, class LB2, class EP2>
int gemm_pair_ep(const LA1& la1, const LB1& lb1, const EP1& ep1, int Mo, int NJ1, int R1, const int* dR1, float* colsum,
                 const LA2& la2, const LB2& lb2, const EP2& ep2, int M2, int NJ2, int R2, const int* dM2, hipStream_t st, int tn_target,
                 int R2_tile) {     // R2_tile: see gemm_auto
  const long nb2 = (long)((M2 + 63) / 64) * ((NJ2 + 63) / 64);
  const int R2t = R2_tile > 0 ? R2_tile : R2;
  const bool thin = nb2 <= pair_thin_nb() && R2t >= pair_ks_min_r(), k2 = nb2 <= pair_ks_nb() && R2t >= pair_ks_min_r();
  const int nb1 = ((Mo + 63) / 64) * ((NJ1 + 63) / 64);
  if (gemm_pair_enabled() && pair_tn_blocks_small() > 0 && nb1 <= pair_tn_small_tiles()) tn_target = pair_tn_blocks_small();
  const int splits = tn_splits(Mo, NJ1, R1, gemm_pair_enabled() ? (tn_target > 0 ? tn_target : pair_tn_blocks_paired()) : 0);
  if (!gemm_pair_enabled() || Mo <= 0 || NJ1 <= 0 || R1 <= 0 || M2 <= 0 || NJ2 <= 0 || R2 <= 0) {
    int rc = launch_gemm_split<TileSplitR>(la1, lb1, ep1, Mo, NJ1, R1, dR1, splits, colsum, st);
    if (rc) return rc;
    if (thin) return launch_gemm<TileAutoThin>(la2, lb2, ep2, M2, NJ2, R2, dM2, nullptr, st);
    if (k2) return launch_gemm<TileAutoK2>(la2, lb2, ep2, M2, NJ2, R2, dM2, nullptr, st);
    return launch_gemm<TileAutoK1>(la2, lb2, ep2, M2, NJ2, R2, dM2, nullptr, st);
  }
  if (thin)      // (round 6: the 4-k-group dW tile beside a thin dX job -- the launch already pays its 72 KB of LDS -- measured +4.5 %: profiles/r06_f)
    return launch_gemm_dual<TileSplitR, LA1, LB1, EP1, TileAutoThin, LA2, LB2, EP2>(la1, lb1, ep1, Mo, NJ1, R1, dR1, splits, colsum, la2, lb2,
                                                                                      ep2, M2, NJ2, R2, dM2, st);
  if (k2)
    return launch_gemm_dual<TileSplitR, LA1, LB1, EP1, TileAutoK2, LA2, LB2, EP2>(la1, lb1, ep1, Mo, NJ1, R1, dR1, splits, colsum, la2, lb2,
                                                                                       ep2, M2, NJ2, R2, dM2, st);
  return launch_gemm_dual<TileSplitR, LA1, LB1, EP1, TileAutoK1, LA2, LB2, EP2>(la1, lb1, ep1, Mo, NJ1, R1, dR1, splits, colsum, la2, lb2, ep2,
                                                                                   M2, NJ2, R2, dM2, st);
}

}  // namespace sast
