// Random-access training sequences over R resident recordings (include/sast_hip.h, "random-access sampler").
//
// The reference builds them on the CPU: SequenceForRandomAccess (data/genx_utils/sequence_rnd.py:9-75) gives every recording its
// start_idx_offset and length, torch's ConcatDataset maps a global item to (recording, local index) by a bisect over the cumulative
// lengths, __getitem__ turns the local index into the `sequence_length` windows that end at a label frame, get_most_recent_objframe
// (data/utils/augmentor.py:367-378) picks the label frame zoom-in is placed on, and get_weighted_random_sampler
// (data/genx_utils/dataset_rnd.py:115-149) weighs the items by their class counts.  Here all of it reads the state sast_labels_load left
// in device memory; every index is formed from sizes read on the device and clamped before it is used, so nothing past a row's
// frames, windows or label rows is ever read, whatever `items` holds.
//
// Every fp64 operation of the weights is the reference's single Python / numpy operation (this file is built with -ffp-contract=off):
// 1.0 / max(total, 1), the product with the item's count, and the sum in ascending class order starting from 0.
#include <climits>
#include "common.cuh"
#include "kernels.h"
#include "label_state.cuh"
#include "sampler_rows.cuh"

namespace sast {
namespace {

constexpr int RND_THREADS = 256;
constexpr int RND_ITEM_THREADS = 64;

// sast_rnd_index, launch 1: workgroup r finds row r's start_idx_offset and length; the workgroup that finishes last scans the lengths.
//
// Ordering across workgroups: a workgroup publishes its length, then thread 0 fences and takes a ticket.  The holder of the last
// ticket knows that every other workgroup's store came before its own ticket; it fences again and reads the lengths with device-scope
// atomic loads, so no stale line of its own cache is used.  Inside a workgroup the rules are lab_load_kernel's: a barrier between the
// phase that writes a shared word and the phase that reads it, and another one before the word is written again.  The last workgroup
// puts the ticket back to 0: the call replays inside a graph.
__global__ __launch_bounds__(RND_THREADS) void rnd_index_kernel(SastLabelArgs a, SastRndArgs q) {
  const int r = blockIdx.x, tid = threadIdx.x, R = a.S;
  __shared__ int sh_first, sh_last;
  __shared__ long long sh_wave[RND_THREADS / 64];
  const int nf = clampi(a.n_frames[r], 0, a.max_frames);
  const long long* f2w = reinterpret_cast<const long long*>(a.frame_2_window) + (size_t)r * a.max_frames;
  if (tid == 0) { sh_first = nf; sh_last = 0; }
  __syncthreads();
  // the first label frame whose window leaves room for sequence_length windows (sequence_rnd.py:24-32)
  int first = nf;
  for (int j = tid; j < nf; j += RND_THREADS)
    if (f2w[j] - q.sequence_length + 1 >= 0) { first = j; break; }
  if (first < nf) atomicMin(&sh_first, first);
  __syncthreads();
  if (tid == 0) {
    q.start_idx_offset[r] = sh_first;
    __hip_atomic_store(&q.length[r], nf - sh_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    q.status[r] = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the length has left this wave before the fence and the ticket
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int ticket = __hip_atomic_fetch_add(q.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_last = ticket == R - 1 ? 1 : 0;
  }
  if (r == 0) {
    for (int c = tid; c < q.max_classes; c += RND_THREADS) q.class_total[c] = 0;
    if (tid == 0) q.status[R] = 0;
  }
  __syncthreads();
  if (!sh_last) return;
  __threadfence();
  // ConcatDataset.cumsum: cum[0] = 0, cum[r + 1] = cum[r] + length[r], RND_THREADS rows per step with a running carry
  long long carry = 0;
  for (int base = 0; base < R; base += RND_THREADS) {
    const int i = base + tid;
    const long long v = i < R ? (long long)clampi(__hip_atomic_load(&q.length[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0, a.max_frames) : 0LL;
    long long all;
    const long long before = block_scan<RND_THREADS / 64>(v, sh_wave, &all);
    if (i < R) q.cum[i + 1] = carry + before + v;
    carry += all;
  }
  if (tid == 0) {
    q.cum[0] = 0;
    __hip_atomic_store(q.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// item (row r, local index i) of the dataset: the boxes per class over the label frames of its windows -> cnt (LDS, max_classes
// words, zero on entry).  Every thread of the workgroup calls it; the counts are complete after the caller's next barrier.
__device__ __forceinline__ void rnd_item_counts(const SastLabelArgs& a, const SastRndArgs& q, int r, int j, int* cnt) {
  const int L = q.sequence_length;
  const LabelRow row = label_row(a, r);
  const long long end = row.frame_2_window[j] + 1;
  int bad = 0;
  for (int k = (q.only_load_end_labels ? L - 1 : 0) + (int)(threadIdx.x / 8); k < L; k += RND_ITEM_THREADS / 8) {
    const long long w = end - L + k;
    if (w < 0 || w >= row.nw) continue;
    const LabelStep st = row.step(w);
    const float* rows = row.rows(st);
    for (int i = threadIdx.x % 8; i < st.count; i += 8) {
      const float c = rows[(size_t)i * 7 + 5];
      if (c >= 0.f && c < (float)q.max_classes) atomicAdd(&cnt[(int)c], 1);
      else bad = 1;
    }
  }
  if (bad) atomicOr(&q.status[r], SAST_RND_CLASS_ID);
}

// sast_rnd_index, launches 2 and 3: workgroup (i, r) is item i of row r.  TOTAL: its class counts are added to class_total and its
// slot of `weights` is cleared; otherwise its weight is written at its global index cum[r] + i.
template <bool TOTAL>
__global__ __launch_bounds__(RND_ITEM_THREADS) void rnd_weight_kernel(SastLabelArgs a, SastRndArgs q) {
  const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  __shared__ int cnt[RND_MAX_CLASSES];
  if (TOTAL && tid == 0) q.weights[(size_t)r * a.max_frames + i] = 0.0;
  const int nf = clampi(a.n_frames[r], 0, a.max_frames);
  const int off = clampi(q.start_idx_offset[r], 0, nf);
  if (i >= nf - off) return;
  for (int c = tid; c < q.max_classes; c += RND_ITEM_THREADS) cnt[c] = 0;
  __syncthreads();
  rnd_item_counts(a, q, r, off + i, cnt);
  __syncthreads();
  if (TOTAL) {
    for (int c = tid; c < q.max_classes; c += RND_ITEM_THREADS)
      if (cnt[c]) atomicAdd(reinterpret_cast<unsigned long long*>(q.class_total) + c, (unsigned long long)cnt[c]);
    return;
  }
  if (tid == 0) {
    const long long g = min(max(reinterpret_cast<const long long*>(q.cum)[r], 0LL) + i, (long long)a.S * a.max_frames - 1);
    double w = 0.0;
    for (int c = 0; c < q.max_classes; ++c) {
      if (!cnt[c]) continue;
      const long long total = max(reinterpret_cast<const long long*>(q.class_total)[c], 1LL);
      const double per_box = 1.0 / (double)total;
      w = w + per_box * (double)cnt[c];
    }
    q.weights[g] = w;
  }
}

// sast_rnd_gather: workgroup k * B + b is step k of sample b (the body is sampler_rows.cuh's, shared with sast_mixed_next)
__global__ __launch_bounds__(SAMPLER_THREADS) void rnd_gather_kernel(SastLabelArgs a, SastRndArgs q, const long long* items, int B,
                                                                     RndGatherOut o) {
  const int b = blockIdx.x % B, k = blockIdx.x / B;
  rnd_gather_step(a, q, items[b], k, B, b, b, o);
}

// sast_mixed_latest: workgroup b is sample b; the `latest` half of the last step of rnd_gather_kernel alone
__global__ __launch_bounds__(SAMPLER_THREADS) void rnd_latest_kernel(SastLabelArgs a, SastRndArgs q, const long long* items, float* latest,
                                                                     int* latest_count) {
  const int b = blockIdx.x, M = a.max_labels_per_frame;
  LabelRow row = {};
  long long w0 = 0;
  const int r = rnd_locate(a, q, items[b], &row, &w0);
  rnd_latest_rows(q, a.S, r, row, w0, M, latest + (size_t)b * M * 7, latest_count + b);
}
}  // namespace
}  // namespace sast

extern "C" {

int sast_rnd_index(const SastLabelArgs* a, SastRndArgs* q, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::label_state_ok(a) || !sast::rnd_args(q) || (q->weighted && !q->weights)) return SAST_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SAST_LAUNCH(sast::rnd_index_kernel, dim3((unsigned)a->S), dim3(sast::RND_THREADS), 0, st, *a, *q);
  if (q->weighted) {
    const dim3 grid((unsigned)a->max_frames, (unsigned)a->S);
    SAST_LAUNCH(sast::rnd_weight_kernel<true>, grid, dim3(sast::RND_ITEM_THREADS), 0, st, *a, *q);
    SAST_LAUNCH(sast::rnd_weight_kernel<false>, grid, dim3(sast::RND_ITEM_THREADS), 0, st, *a, *q);
  }
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_rnd_gather(const SastLabelArgs* a, const SastRndArgs* q, const int64_t* items, int B, int32_t* rows, int64_t* window_idx,
                    int64_t* ends_us, float* labels, int32_t* counts, uint8_t* labelled, float* latest, int32_t* latest_count,
                    sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::label_state_ok(a) || !sast::rnd_args(q) || !items || !rows || !window_idx || !ends_us || !labels || !counts || !labelled ||
      !latest || !latest_count || B < 1)
    return SAST_EINVAL;
  if (!sast::sampler_batch_fits(B, q->sequence_length, a->max_labels_per_frame)) return SAST_EINVAL;
  const sast::RndGatherOut o = {rows, nullptr, reinterpret_cast<long long*>(window_idx), reinterpret_cast<long long*>(ends_us), labels, counts,
                                labelled, nullptr, latest, latest_count};
  SAST_LAUNCH(sast::rnd_gather_kernel, dim3((unsigned)(B * q->sequence_length)), dim3(sast::SAMPLER_THREADS), 0, (hipStream_t)stream, *a, *q,
              reinterpret_cast<const long long*>(items), B, o);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_mixed_latest(const SastLabelArgs* a, const SastRndArgs* q, const int64_t* items, int B, float* latest, int32_t* latest_count,
                      sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::label_state_ok(a) || !sast::rnd_args(q) || !items || !latest || !latest_count || B < 1) return SAST_EINVAL;
  if (!sast::sampler_batch_fits(B, 1, a->max_labels_per_frame)) return SAST_EINVAL;
  SAST_LAUNCH(sast::rnd_latest_kernel, dim3((unsigned)B), dim3(sast::SAMPLER_THREADS), 0, (hipStream_t)stream, *a, *q,
              reinterpret_cast<const long long*>(items), latest, latest_count);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
