// Whole-sample movers of the label-sparse training step and the online detector: gather the labelled (timestep, sample) pairs of a
// sequence (BackboneFeatureSelector, modules/utils/detection.py:24-47), scatter their gradients back, zero the states of samples that
// start a new sequence (RNNStates.reset, :96-130), commit states by flag, hand states back.
//
// A selection comes from one of two places, and the kernels are templates on which.  A HOST list (SastSampleGather's t_of / b_of,
// SastSampleMask) travels by value in the kernel arguments: the entry point has validated it, and a captured launch replays that one
// pattern for ever -- one pattern per graph, which is what bench.py --label-every and TrainStep(indices=) capture.  A DEVICE table
// (sast_select_table's table / slot_of, a flags tensor) is read from memory when the kernel runs, so a replay follows the pattern of the
// replay; there the entries are data, and only the NUMBER of rows, n_out = K, stays a launch parameter (it is the batch of the PAFPN).
// Source and destination pointers travel by value either way, so a captured launch keeps pointing into the graph's pool.
#include "common.cuh"
#include "kernels.h"

namespace sast {
namespace {

// the device table of a pattern.  One workgroup of 1024 threads walks the n = T * B <= 8192 flags in chunks of 1024, in index order
// (= timestep-major, batch ascending): rank of a flag = pairs before the chunk + those of the lower waves of the chunk (16 counts in
// LDS) + popcount of the wave's ballot below the lane.
__global__ __launch_bounds__(1024) void select_table_kernel(const uint8_t* __restrict__ labelled, int n, int B, int n_out,
                                                            int32_t* __restrict__ table, int32_t* __restrict__ slot_of,
                                                            int32_t* __restrict__ n_sel, int32_t* __restrict__ err) {
  __shared__ int wave_cnt[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;                                        // flagged pairs before the chunk (the same value in every thread)
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const bool f = i < n && labelled[i] != 0;
    const unsigned long long m = __ballot(f);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int below = 0, total = 0;
    for (int w = 0; w < 16; ++w) {
      const int c = wave_cnt[w];
      below += w < wave ? c : 0;
      total += c;
    }
    if (i < n) {
      const int j = base + below + __popcll(m & ((1ull << lane) - 1ull));
      const bool fits = f && j < n_out;
      slot_of[i] = fits ? j : -1;
      if (fits) {
        const int t = i / B;
        table[2 * j] = t;
        table[2 * j + 1] = i - t * B;
      }
    }
    base += total;
    __syncthreads();                                   // wave_cnt is rewritten by the next chunk
  }
  for (int j = min(base, n_out) + (int)threadIdx.x; j < n_out; j += 1024) { table[2 * j] = -1; table[2 * j + 1] = -1; }
  if (threadIdx.x == 0) {
    *n_sel = base;
    if (base > n_out) err[0] += 1;                     // pattern truncated
    if (base < n_out) err[1] += 1;                     // under-full
  }
}

// one row of n words, this workgroup's share (blockIdx.x of gridDim.x): dst = src, or zeros when src is null.  16-byte accesses where
// both rows are 16-byte aligned (always, when the row length is a multiple of 4 floats), single words otherwise and for the tail.
__device__ __forceinline__ void move_row(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
  const bool vec = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;     // (block-uniform; null counts as aligned)
  const size_t n4 = vec ? n / 4 : 0;
  if (src) {
    for (size_t i = tid; i < n4; i += step) st4(dst + 4 * i, ld4(src + 4 * i));
    for (size_t i = 4 * n4 + tid; i < n; i += step) dst[i] = src[i];
  } else {
    for (size_t i = tid; i < n4; i += step) st4(dst + 4 * i, zero4());
    for (size_t i = 4 * n4 + tid; i < n; i += step) dst[i] = 0.f;
  }
}
// workgroups of 256 threads that share one row: eight 16-byte accesses per thread, at most `cap` workgroups
inline int row_blocks(size_t floats, size_t cap = 64) {
  const size_t bx = (floats / 4 + 256 * 8 - 1) / (256 * 8);
  return (int)(bx < 1 ? 1 : (bx > cap ? cap : bx));
}

// ---------------------------------------------------------------- gather / scatter of (timestep, sample) pairs
// what SastSampleGather and SastSampleGatherDev share; the pairs themselves come from one of the two policies below
struct GatherJob {
  int n_src, n_out, B;
  size_t sample_floats;
  const float* src[SAST_GATHER_MAX_SRC];
  float* dsrc[SAST_GATHER_MAX_SRC];
  float* out;
};
template <class A>
GatherJob gather_job(const A& a) {
  GatherJob g{a.n_src, a.n_out, a.B, a.sample_floats, {}, {}, a.out};
  for (int t = 0; t < SAST_GATHER_MAX_SRC; ++t) { g.src[t] = a.src[t]; g.dsrc[t] = a.dsrc[t]; }
  return g;
}
// pair(j): the (t, b) of output row j, false when the row is to be zeros; slot(t, b): the output row of the pair, -1 when it has none
struct HostPairs {      // by value, validated by the entry point
  uint8_t t_of[SAST_GATHER_MAX_OUT], b_of[SAST_GATHER_MAX_OUT];
  __device__ __forceinline__ bool pair(const GatherJob&, int j, int& t, int& b) const { t = t_of[j]; b = b_of[j]; return true; }
  __device__ __forceinline__ int slot(const GatherJob& a, int t, int b) const {
    int j = -1;
    for (int k = 0; k < a.n_out; ++k) if (t_of[k] == t && b_of[k] == b) j = k;      // block-uniform scan (n_out <= 256)
    return j;
  }
};
struct DevicePairs {    // DATA: an entry that names no timestep / sample / row of the call moves zeros, never an address outside it
  const int32_t* table; const int32_t* slot_of;
  __device__ __forceinline__ bool pair(const GatherJob& a, int j, int& t, int& b) const {
    t = table[2 * j]; b = table[2 * j + 1];
    return t >= 0 && t < a.n_src && b >= 0 && b < a.B;
  }
  __device__ __forceinline__ int slot(const GatherJob& a, int t, int b) const {
    const int j = slot_of[t * a.B + b];                // [n_src * B]: one load per block, no scan over the rows
    return j >= 0 && j < a.n_out ? j : -1;
  }
};
// forward: one launch copies every selected sample of one feature map, grid (share of a sample, output row)
template <class Pairs>
__global__ __launch_bounds__(256) void gather_samples_kernel(GatherJob a, Pairs p) {
  const int j = blockIdx.y;
  int t, b;
  const bool ok = p.pair(a, j, t, b);
  move_row(a.out + (size_t)j * a.sample_floats, ok ? a.src[t] + (size_t)b * a.sample_floats : nullptr, a.sample_floats);
}
// backward: EVERY sample gradient of every timestep is written (the gathered gradient or zeros), grid (share, timestep * B + sample)
template <class Pairs>
__global__ __launch_bounds__(256) void scatter_samples_kernel(GatherJob a, Pairs p) {
  const int t = blockIdx.y / a.B, b = blockIdx.y % a.B;
  const int j = p.slot(a, t, b);
  move_row(a.dsrc[t] + (size_t)b * a.sample_floats, j >= 0 ? a.out + (size_t)j * a.sample_floats : nullptr, a.sample_floats);
}
template <class Pairs>
int gather_launch(const GatherJob& a, const Pairs& p, bool backward, hipStream_t st) {
  const int bx = row_blocks(a.sample_floats);
  if (!backward) SAST_LAUNCH(gather_samples_kernel<Pairs>, dim3(bx, a.n_out), dim3(256), 0, st, a, p);
  else SAST_LAUNCH(scatter_samples_kernel<Pairs>, dim3(bx, a.n_src * a.B), dim3(256), 0, st, a, p);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

// ---------------------------------------------------------------- the predicated mover: reset, commit, hand-back
// sample b of dst[i] takes sample b of src[i] (zeros when src[i] is null) where the flag source says so, and keeps every bit otherwise;
// grid (share of a sample, sample, tensor).  The flag is read once per workgroup and the branch is workgroup-uniform.
struct MoveJob {
  int n, B;
  float* dst[SAST_ZERO_MAX_TENSORS];
  const float* src[SAST_ZERO_MAX_TENSORS];
  size_t floats[SAST_ZERO_MAX_TENSORS];              // per sample
};
struct MaskFlags { SastSampleMask m; __device__ __forceinline__ bool operator()(int b) const { return m.sel[b] != 0; } };
struct DeviceFlags { const uint8_t* flags; __device__ __forceinline__ bool operator()(int b) const { return flags[b] != 0; } };
struct EveryRow { __device__ __forceinline__ bool operator()(int) const { return true; } };

template <class Flags>
__global__ __launch_bounds__(256) void move_samples_kernel(MoveJob a, Flags flagged) {
  if (!flagged(blockIdx.y)) return;
  const size_t n = a.floats[blockIdx.z], off = (size_t)blockIdx.y * n;
  const float* src = a.src[blockIdx.z];
  move_row(a.dst[blockIdx.z] + off, src ? src + off : nullptr, n);
}
size_t largest_sample(const MoveJob& a) {
  size_t most = 0;
  for (int i = 0; i < a.n; ++i) most = a.floats[i] > most ? a.floats[i] : most;
  return most;
}
template <class Flags>
int move_samples_launch(const MoveJob& a, const Flags& flagged, int bx, hipStream_t st) {
  SAST_LAUNCH(move_samples_kernel<Flags>, dim3(bx, a.B, a.n), dim3(256), 0, st, a, flagged);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

bool gather_dev_ok(const SastSampleGatherDev* a) {
  return a && a->n_src >= 1 && a->n_src <= SAST_GATHER_MAX_SRC && a->n_out >= 0 && a->n_out <= SAST_GATHER_MAX_OUT && a->B >= 1 && a->B <= 256 &&
         a->sample_floats >= 1 && (!a->n_out || a->out);
}
HostPairs host_pairs(const SastSampleGather& a) {
  HostPairs p;
  for (int j = 0; j < SAST_GATHER_MAX_OUT; ++j) { p.t_of[j] = a.t_of[j]; p.b_of[j] = a.b_of[j]; }
  return p;
}

}  // namespace
}  // namespace sast

extern "C" {

int sast_gather_samples(const SastSampleGather* a, sast_stream_t stream) { SAST_ENTRY();
  if (!a || !a->out || a->n_src < 1 || a->n_src > SAST_GATHER_MAX_SRC || a->n_out < 0 || a->n_out > SAST_GATHER_MAX_OUT || a->sample_floats % 4) return SAST_EINVAL;
  for (int j = 0; j < a->n_out; ++j) if (a->t_of[j] >= a->n_src || a->b_of[j] >= a->B || !a->src[a->t_of[j]]) return SAST_EINVAL;
  if (a->n_out == 0) return SAST_OK;
  return sast::gather_launch(sast::gather_job(*a), sast::host_pairs(*a), false, (hipStream_t)stream);
}
int sast_gather_samples_bwd(const SastSampleGather* a, sast_stream_t stream) { SAST_ENTRY();
  if (!a || a->n_src < 1 || a->n_src > SAST_GATHER_MAX_SRC || a->n_out < 0 || a->n_out > SAST_GATHER_MAX_OUT || a->B < 1 || a->B > 256 ||
      a->sample_floats % 4 || (a->n_out && !a->out)) return SAST_EINVAL;
  for (int t = 0; t < a->n_src; ++t) if (!a->dsrc[t]) return SAST_EINVAL;
  return sast::gather_launch(sast::gather_job(*a), sast::host_pairs(*a), true, (hipStream_t)stream);
}
int sast_zero_samples(float* x, int B, size_t sample_floats, const SastSampleMask* sel, sast_stream_t stream) { SAST_ENTRY();
  if (!x || !sel || B < 1 || B > 256 || sample_floats % 4) return SAST_EINVAL;
  sast::MoveJob j{1, B, {x}, {}, {sample_floats}};
  return sast::move_samples_launch(j, sast::MaskFlags{*sel}, sast::row_blocks(sample_floats), (hipStream_t)stream);
}
int sast_select_table(const uint8_t* labelled, int T, int B, int n_out, int32_t* table, int32_t* slot_of, int32_t* n_sel, int32_t* err,
                      sast_stream_t stream) { SAST_ENTRY();
  if (!labelled || !slot_of || !n_sel || !err || T < 1 || T > SAST_GATHER_MAX_SRC || B < 1 || B > 256 || n_out < 0 ||
      n_out > SAST_GATHER_MAX_OUT || (n_out && !table)) return SAST_EINVAL;
  SAST_LAUNCH(sast::select_table_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, labelled, T * B, B, n_out, table, slot_of, n_sel, err);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}
int sast_gather_samples_dev(const SastSampleGatherDev* a, sast_stream_t stream) { SAST_ENTRY();
  if (!sast::gather_dev_ok(a) || (a->n_out && !a->table)) return SAST_EINVAL;
  for (int t = 0; t < a->n_src; ++t) if (!a->src[t]) return SAST_EINVAL;      // the table is data: any timestep may be named
  if (a->n_out == 0) return SAST_OK;
  return sast::gather_launch(sast::gather_job(*a), sast::DevicePairs{a->table, a->slot_of}, false, (hipStream_t)stream);
}
int sast_gather_samples_dev_bwd(const SastSampleGatherDev* a, sast_stream_t stream) { SAST_ENTRY();
  if (!sast::gather_dev_ok(a) || !a->slot_of) return SAST_EINVAL;
  for (int t = 0; t < a->n_src; ++t) if (!a->dsrc[t]) return SAST_EINVAL;
  return sast::gather_launch(sast::gather_job(*a), sast::DevicePairs{a->table, a->slot_of}, true, (hipStream_t)stream);
}
int sast_zero_samples_dev(const SastSampleZeroDev* a, sast_stream_t stream) { SAST_ENTRY();
  if (!a || !a->flags || a->n < 0 || a->n > SAST_ZERO_MAX_TENSORS || a->B < 1 || a->B > 256) return SAST_EINVAL;
  for (int i = 0; i < a->n; ++i) if (!a->x[i] || !a->sample_floats[i]) return SAST_EINVAL;
  if (a->n == 0) return SAST_OK;
  sast::MoveJob j{a->n, a->B};
  for (int i = 0; i < a->n; ++i) { j.dst[i] = a->x[i]; j.floats[i] = a->sample_floats[i]; }
  return sast::move_samples_launch(j, sast::DeviceFlags{a->flags}, sast::row_blocks(sast::largest_sample(j)), (hipStream_t)stream);
}
int sast_commit_samples_dev(const SastSampleCommitDev* a, sast_stream_t stream) { SAST_ENTRY();
  if (!a || !a->flags || a->n < 0 || a->n > SAST_ZERO_MAX_TENSORS || a->B < 1 || a->B > 256) return SAST_EINVAL;
  for (int i = 0; i < a->n; ++i) if (!a->dst[i] || !a->src[i] || !a->sample_floats[i]) return SAST_EINVAL;
  if (a->n == 0) return SAST_OK;
  sast::MoveJob j{a->n, a->B};
  for (int i = 0; i < a->n; ++i) { j.dst[i] = a->dst[i]; j.src[i] = a->src[i]; j.floats[i] = a->sample_floats[i]; }
  return sast::move_samples_launch(j, sast::DeviceFlags{a->flags}, sast::row_blocks(sast::largest_sample(j)), (hipStream_t)stream);
}
// several whole tensors in one launch (the recurrent states handed back into the step's input tensors): each is one "sample" of a
// batch of 1, every row moves, and a tensor may take up to 256 workgroups
int sast_copy_tensors(const SastTensorCopy* a, sast_stream_t stream) { SAST_ENTRY();
  if (!a || a->n < 0 || a->n > SAST_ZERO_MAX_TENSORS) return SAST_EINVAL;
  for (int i = 0; i < a->n; ++i) if (!a->dst[i] || !a->src[i] || !a->floats[i]) return SAST_EINVAL;
  if (a->n == 0) return SAST_OK;
  sast::MoveJob j{a->n, 1};
  for (int i = 0; i < a->n; ++i) { j.dst[i] = a->dst[i]; j.src[i] = a->src[i]; j.floats[i] = a->floats[i]; }
  return sast::move_samples_launch(j, sast::EveryRow{}, sast::row_blocks(sast::largest_sample(j), 256), (hipStream_t)stream);
}

}  // extern "C"
