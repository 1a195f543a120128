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

namespace sast {
namespace {

constexpr int RND_THREADS = 256;
constexpr int RND_ITEM_THREADS = 64;
constexpr int RND_MAX_CLASSES = 256;

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

// sast_rnd_gather: workgroup k * B + b is step k of sample b
__global__ __launch_bounds__(128) void rnd_gather_kernel(SastLabelArgs a, SastRndArgs q, const long long* items, int B, int* rows_out,
                                                         long long* window_idx, long long* ends_out, float* labels, int* counts,
                                                         unsigned char* labelled, float* latest, int* latest_count) {
  const int blk = blockIdx.x, b = blk % B, k = blk / B, tid = threadIdx.x;
  const int R = a.S, L = q.sequence_length, M = a.max_labels_per_frame;
  const long long* cum = reinterpret_cast<const long long*>(q.cum);
  const long long g = items[b];
  // ConcatDataset.__getitem__: the row with cum[r] <= g < cum[r + 1]; a cum that does not grow (it always does after sast_rnd_index)
  // can only send the search to another row, whose own sizes then bound every index
  int r = -1;
  long long w = -1;
  LabelRow row = {};
  if (g >= 0 && g < cum[R]) {
    int lo = 0, hi = R;                       // the first r with cum[r + 1] > g
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (cum[mid + 1] > g) hi = mid; else lo = mid + 1;
    }
    r = min(lo, R - 1);
    row = label_row(a, r);
    const long long j = g - cum[r] + (long long)q.start_idx_offset[r];
    if (j >= 0 && j < row.nf) {
      const long long end = row.frame_2_window[j] + 1;
      if (end - L >= 0 && end <= row.nw) w = end - L + k;
    }
    if (w < 0) r = -1;
  }
  float* out = labels + (size_t)blk * M * 7;
  const bool last = k == L - 1;
  if (r < 0) {
    for (int i = tid; i < M * 7; i += blockDim.x) out[i] = 0.f;
    if (last) for (int i = tid; i < M * 7; i += blockDim.x) latest[(size_t)b * M * 7 + i] = 0.f;
    if (tid == 0) {
      window_idx[blk] = -1;
      ends_out[blk] = -1;
      counts[blk] = 0;
      labelled[blk] = 0;
      if (k == 0) rows_out[b] = -1;
      if (last) {
        latest_count[b] = 0;
        atomicOr(&q.status[R], SAST_RND_ITEM_INDEX);
      }
    }
    return;
  }
  // only_load_end_labels: the steps before the last read as unlabelled
  const LabelStep st = (!q.only_load_end_labels || last) ? row.step(w) : LabelStep{0, 0, 0};
  row.copy(st, out, M, tid, blockDim.x);
  if (tid == 0) {
    window_idx[blk] = w;
    ends_out[blk] = row.ends_us[w];
    counts[blk] = st.count;
    labelled[blk] = (unsigned char)st.labelled;
    if (k == 0) rows_out[b] = r;
  }
  if (!last) return;
  // get_most_recent_objframe(check_if_nonempty=True): the last step of the sample whose label frame holds a box (every thread walks
  // the same few windows and finds the same one)
  LabelStep lst = {0, 0, 0};
  for (int kk = L - 1; kk >= (q.only_load_end_labels ? L - 1 : 0); --kk) {
    const LabelStep c = row.step(w - (L - 1 - kk));
    if (c.count > 0) {
      lst = c;
      break;
    }
  }
  row.copy(lst, latest + (size_t)b * M * 7, M, tid, blockDim.x);
  if (tid == 0) latest_count[b] = lst.count;
}

bool rnd_args(const SastRndArgs* q) {
  return q && q->start_idx_offset && q->length && q->cum && q->status && q->ticket && q->sequence_length >= 1 &&
         q->sequence_length <= 65535 && q->max_classes >= 1 && q->max_classes <= RND_MAX_CLASSES && q->class_total;
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
  if ((long long)B * q->sequence_length * a->max_labels_per_frame > INT_MAX / 8) return SAST_EINVAL;
  SAST_LAUNCH(sast::rnd_gather_kernel, dim3((unsigned)(B * q->sequence_length)), dim3(128), 0, (hipStream_t)stream, *a, *q,
              reinterpret_cast<const long long*>(items), B, rows, reinterpret_cast<long long*>(window_idx),
              reinterpret_cast<long long*>(ends_us), labels, counts, labelled, latest, latest_count);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
