// Streamed training / evaluation sequences over R resident recordings (include/sast_hip.h, "streaming sampler").
//
// The reference builds them on the CPU: SequenceForIter.get_sequences_with_guaranteed_labels and _get_ev_repr_range_indices
// (data/genx_utils/sequence_for_streaming.py:21-50, 86-111) cut a recording into sub-sequences wherever two label frames lie more than
// sequence_length windows apart, SequenceForIter.__init__ / __getitem__ (:53-84, 137-181) chunk a sub-sequence into samples of
// sequence_length windows and pad the last one, and ConcatStreamingDataPipe / ShardedStreamingDataPipe (data/utils/stream_*_datapipe.py)
// walk every batch row through a list of sub-sequences, filling finished rows with get_fully_padded_sample (:120-132).  Here all of it
// reads the state sast_labels_load left in device memory and a per-row schedule + cursor in device memory; every index is formed from
// sizes read on the device and clamped before it is used, so nothing past a row's frames, windows or label rows is ever read,
// whatever the schedule, the cursor or the sequence table hold.
//
// No kernel here waits for another workgroup and none keeps a ticket or a scratch word between calls: sast_stream_index is two
// launches (a row's sequence count; every row's own prefix over those counts, then its compaction), sast_stream_next is one launch
// whose workgroups each own one batch row's cursor.  All of them replay inside a graph.
#include <climits>
#include "common.cuh"
#include "kernels.h"
#include "label_state.cuh"
#include "sampler_rows.cuh"

namespace sast {
namespace {

constexpr int STREAM_THREADS = 256;

// frame_2_window[r][j] clamped into the row's windows
__device__ __forceinline__ int stream_f2w(const int64_t* f2w, int j, int nw) {
  return (int)min(max((long long)f2w[j], 0LL), (long long)(nw - 1));
}

// frame j > 0 begins a new sub-sequence: np.diff(indices) > max_len (sequence_for_streaming.py:40)
__device__ __forceinline__ bool stream_break(const int64_t* f2w, int j, int nw, int L) {
  return stream_f2w(f2w, j, nw) - stream_f2w(f2w, j - 1, nw) > L;
}

// sast_stream_index, launch 1: workgroup r counts row r's sequences into row_count[r]
__global__ __launch_bounds__(STREAM_THREADS) void stream_count_kernel(SastLabelArgs a, SastStreamArgs q) {
  const int r = blockIdx.x, tid = threadIdx.x;
  __shared__ int sh[STREAM_THREADS / 64];
  const LabelRow row = label_row(a, r);
  int part = 0, n;
  if (q.guarantee_labels)
    for (int j = 1 + tid; j < row.nf; j += STREAM_THREADS) part += stream_break(row.frame_2_window, j, row.nw, q.sequence_length) ? 1 : 0;
  block_scan<STREAM_THREADS / 64>(part, sh, &n);
  if (tid == 0) {
    q.row_count[r] = row.nf > 0 ? n + 1 : 0;
    if (r == 0) q.status[0] = 0;
  }
}

// sast_stream_index, launch 2: workgroup r sums the counts of the rows before it (its first sequence), then writes its sequences in
// ascending window order; the last workgroup also writes the total.  Sequence k of the row holds the frames between its k-th and
// (k+1)-th break: the thread of the first frame writes the start, the thread of the last frame the stop, and after a barrier the
// sample counts follow from both.
__global__ __launch_bounds__(STREAM_THREADS) void stream_compact_kernel(SastLabelArgs a, SastStreamArgs q) {
  const int r = blockIdx.x, tid = threadIdx.x, R = a.S, L = q.sequence_length, cap = q.max_sequences;
  __shared__ int sh[STREAM_THREADS / 64];
  int before;
  {
    int part = 0;                                             // R * max_frames <= INT_MAX: no partial sum overflows
    for (int i = tid; i < r; i += STREAM_THREADS) part += clampi(q.row_count[i], 0, a.max_frames);
    block_scan<STREAM_THREADS / 64>(part, sh, &before);
  }
  const LabelRow row = label_row(a, r);
  const int nf = row.nf, nw = row.nw;
  const int64_t* f2w = row.frame_2_window;
  const int mine = clampi(q.row_count[r], 0, a.max_frames);
  const int first = min(before, cap);
  if (tid == 0) {
    q.row_first_seq[r] = first;
    if (r == R - 1) {
      const long long total = (long long)before + mine;
      q.row_first_seq[R] = (int)min(total, (long long)cap);
      q.n_seq[0] = (int)min(total, (long long)cap);
      if (total > cap) atomicOr(&q.status[0], SAST_STREAM_TRUNCATED);
    }
  }
  if (nf == 0) return;
  const int room = cap - first;                               // sequences of this row that fit into the table
  if (!q.guarantee_labels) {
    if (tid == 0 && room > 0) {
      const int start = max(stream_f2w(f2w, 0, nw) - L + 1, 0);
      q.seq_row[first] = r;
      q.seq_start[first] = start;
      q.seq_stop[first] = nw;
      q.seq_samples[first] = (nw - start + L - 1) / L;
    }
    return;
  }
  int carry = 0;                                              // breaks in front of this chunk of frames
  for (int base = 0; base < nf; base += STREAM_THREADS) {
    const int j = base + tid;
    const int brk = (j >= 1 && j < nf && stream_break(f2w, j, nw, L)) ? 1 : 0;
    int all;
    const int pre = block_scan<STREAM_THREADS / 64>(brk, sh, &all);
    if (j < nf) {
      const int k = carry + pre + brk;                        // the sequence frame j lies in: the breaks at frames 1 .. j
      if (k < room) {
        const int w = stream_f2w(f2w, j, nw);
        if (j == 0 || brk) {
          q.seq_row[first + k] = r;
          q.seq_start[first + k] = max(w - L + 1, 0);
        }
        if (j == nf - 1 || stream_break(f2w, j + 1, nw, L)) q.seq_stop[first + k] = w + 1;
      }
    }
    carry += all;
  }
  __syncthreads();                                            // the starts and stops of this workgroup's sequences are written
  const int n = min(mine, room);
  for (int k = tid; k < n; k += STREAM_THREADS) {
    const int start = q.seq_start[first + k], stop = q.seq_stop[first + k];
    q.seq_samples[first + k] = (max(stop - start, 0) + L - 1) / L;
  }
}

// sast_stream_next: workgroup b is batch row b (the walk itself is sampler_rows.cuh's, shared with sast_mixed_next)
__global__ __launch_bounds__(SAMPLER_THREADS) void stream_next_kernel(SastLabelArgs a, SastStreamArgs q, int B, StreamNextOut o) {
  stream_walk_row(a, q, (int)blockIdx.x, B, (int)blockIdx.x, o);
}
}  // namespace
}  // namespace sast

extern "C" {

int sast_stream_index(const SastLabelArgs* a, const SastStreamArgs* q, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::label_state_ok(a) || !sast::stream_args(q)) return SAST_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  SAST_LAUNCH(sast::stream_count_kernel, dim3((unsigned)a->S), dim3(sast::STREAM_THREADS), 0, st, *a, *q);
  SAST_LAUNCH(sast::stream_compact_kernel, dim3((unsigned)a->S), dim3(sast::STREAM_THREADS), 0, st, *a, *q);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_stream_next(const SastLabelArgs* a, const SastStreamArgs* q, int B, int32_t* rows, int32_t* step_rows, int32_t* seq, int32_t* sample,
                     uint8_t* is_first, uint8_t* exhausted, int64_t* window_idx, int64_t* ends_us, float* labels, int32_t* counts,
                     uint8_t* labelled, uint8_t* is_padded, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::label_state_ok(a) || !sast::stream_args(q) || !sast::stream_schedule_args(q, B) || !rows || !step_rows || !seq || !sample ||
      !is_first || !exhausted || !window_idx || !ends_us || !labels || !counts || !labelled || !is_padded)
    return SAST_EINVAL;
  if (!sast::sampler_batch_fits(B, q->sequence_length, a->max_labels_per_frame)) return SAST_EINVAL;
  const sast::StreamNextOut o = {rows, step_rows, seq, sample, is_first, exhausted, reinterpret_cast<long long*>(window_idx),
                                 reinterpret_cast<long long*>(ends_us), labels, counts, labelled, is_padded};
  SAST_LAUNCH(sast::stream_next_kernel, dim3((unsigned)B), dim3(sast::SAMPLER_THREADS), 0, (hipStream_t)stream, *a, *q, B, o);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
