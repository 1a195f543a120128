// The two bodies the samplers are made of, on top of label_state.cuh: the walk of one streamed batch row through its L steps
// (k_stream.hip, sast_stream_next) and one (step, sample) of a random-access item (k_sampler.hip, sast_rnd_gather).  Both write into
// tensors laid out [L, stride, ...] / [stride] at column `col`: the stand-alone kernels pass their own batch size and their own batch
// row, sast_mixed_next (k_mixed.hip) passes Bs + Br and puts the random columns behind the streamed ones.  Every size is read on the
// device and every index is clamped before it is used, as label_state.cuh's; nothing here reads what another workgroup writes.
//
// Device code (thread index, barrier, atomics); the argument checks at the end are host code shared by the entry points.
#pragma once
#include <climits>
#include "label_state.cuh"

namespace sast {

constexpr int SAMPLER_THREADS = 128;          // the workgroup of sast_stream_next, sast_rnd_gather, sast_mixed_latest and sast_mixed_next
constexpr int RND_MAX_CLASSES = 256;

struct StreamNextOut {                        // sast_stream_next's outputs (include/sast_hip.h)
  int *rows, *step_rows, *seq, *sample;
  unsigned char *is_first, *exhausted;
  long long *window_idx, *ends_us;
  float* labels;
  int* counts;
  unsigned char *labelled, *is_padded;
};

struct RndGatherOut {                         // sast_rnd_gather's outputs; step_rows and is_padded may be null (only sast_mixed_next has them)
  int *rows, *step_rows;
  long long *window_idx, *ends_us;
  float* labels;
  int* counts;
  unsigned char *labelled, *is_padded;
  float* latest;
  int* latest_count;
};

#ifdef __HIPCC__
// batch row b of the schedule -> column `col` of outputs whose batch axis holds `stride` columns; every thread of a workgroup of
// SAMPLER_THREADS calls it (it holds a barrier), then row b's cursor has moved on by one sample
__device__ __forceinline__ void stream_walk_row(const SastLabelArgs& a, const SastStreamArgs& q, int b, int stride, int col,
                                                const StreamNextOut& o) {
  const int tid = threadIdx.x;
  const int R = a.S, L = q.sequence_length, M = a.max_labels_per_frame;
  __shared__ int sh_row, sh_seq, sh_sample, sh_start, sh_stop, sh_done, sh_next_pos, sh_next_sample;
  if (tid == 0) {
    const int len = clampi(q.order_len[b], 0, q.order_capacity);
    const int nseq = clampi(q.n_seq[0], 0, q.max_sequences);
    const int pos = clampi(q.cursor[2 * b], 0, len);
    int sample = max(q.cursor[2 * b + 1], 0);
    int row = -1, s = -1, start = 0, stop = 0, done = 0, next_pos = pos, next_sample = sample;
    if (pos >= len) {
      done = 1;                                               // get_fully_padded_sample: the cursor stays where it is
      sample = -1;
    } else {
      s = q.order[(size_t)b * q.order_capacity + pos];
      if (s < 0 || s >= nseq) {
        atomicOr(&q.status[0], SAST_STREAM_SCHEDULE_INDEX);   // a fully padded sample, then the next entry
        s = -1;
        sample = -1;
        next_pos = pos + 1;
        next_sample = 0;
      } else {
        row = clampi(q.seq_row[s], 0, R - 1);
        const int nw = clampi(a.n_windows[row], 0, a.max_windows);
        start = clampi(q.seq_start[s], 0, nw);
        stop = clampi(q.seq_stop[s], start, nw);
        const int samples = max((stop - start + L - 1) / L, 1);
        sample = min(sample, samples - 1);
        if (sample + 1 < samples) {
          next_sample = sample + 1;
        } else {
          next_pos = pos + 1;
          next_sample = 0;
        }
      }
    }
    sh_row = row; sh_seq = s; sh_sample = sample; sh_start = start; sh_stop = stop; sh_done = done;
    sh_next_pos = next_pos; sh_next_sample = next_sample;
  }
  __syncthreads();
  const int row = sh_row, sample = sh_sample;
  // step k of sample i of a sequence is window start + i * L + k, padded from `stop` on
  const long long w0 = row >= 0 ? (long long)sh_start + (long long)sample * L : 0;
  const long long stop = row >= 0 ? sh_stop : 0;              // row < 0: every step is padded
  const LabelRow view = label_row(a, max(row, 0));
  for (int k = tid; k < L; k += SAMPLER_THREADS) {
    const long long w = w0 + k;
    const bool real = w < stop;
    const size_t at = (size_t)k * stride + col;
    const LabelStep st = real ? view.step(w) : LabelStep{0, 0, 0};
    o.step_rows[at] = real ? row : -1;
    o.window_idx[at] = real ? w : -1;
    o.ends_us[at] = real ? view.ends_us[w] : -1;
    o.counts[at] = st.count;
    o.labelled[at] = (unsigned char)st.labelled;
    o.is_padded[at] = real ? 0 : 1;
  }
  for (int k = 0; k < L; ++k) {
    const long long w = w0 + k;
    const LabelStep st = w < stop ? view.step(w) : LabelStep{0, 0, 0};
    view.copy(st, o.labels + ((size_t)k * stride + col) * M * 7, M, tid, SAMPLER_THREADS);
  }
  if (tid == 0) {
    o.rows[col] = row;
    o.seq[col] = sh_seq;
    o.sample[col] = sample;
    o.is_first[col] = row >= 0 && sample == 0 ? 1 : 0;
    o.exhausted[col] = (unsigned char)sh_done;
    q.cursor[2 * b] = sh_next_pos;
    q.cursor[2 * b + 1] = sh_next_sample;
  }
}

// ConcatDataset.__getitem__ for item g: the row with cum[r] <= g < cum[r + 1], or -1 for an item that has no sample; *row is that row
// and *w0 the first of the sample's L windows.  A cum that does not grow (it always does after sast_rnd_index) can only send the
// search to another row, whose own sizes then bound every index.
__device__ __forceinline__ int rnd_locate(const SastLabelArgs& a, const SastRndArgs& q, long long g, LabelRow* row, long long* w0) {
  const int R = a.S, L = q.sequence_length;
  const long long* cum = reinterpret_cast<const long long*>(q.cum);
  if (g < 0 || g >= cum[R]) return -1;
  int lo = 0, hi = R;                         // the first r with cum[r + 1] > g
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (cum[mid + 1] > g) hi = mid; else lo = mid + 1;
  }
  const int r = min(lo, R - 1);
  *row = label_row(a, r);
  const long long j = g - cum[r] + (long long)q.start_idx_offset[r];
  if (j < 0 || j >= row->nf) return -1;
  const long long end = row->frame_2_window[j] + 1;
  if (end - L < 0 || end > row->nw) return -1;
  *w0 = end - L;
  return r;
}

// get_most_recent_objframe(check_if_nonempty=True) of the sample that starts at window w0 of `row` (r >= 0), or the empty form of an
// item without a sample (r < 0, which also sets SAST_RND_ITEM_INDEX): latest [M, 7] and latest_count of sample b.  Every thread
// walks the same few windows and finds the same one.
__device__ __forceinline__ void rnd_latest_rows(const SastRndArgs& q, int R, int r, const LabelRow& row, long long w0, int M, float* latest,
                                                int* latest_count) {
  const int tid = threadIdx.x, L = q.sequence_length;
  if (r < 0) {
    for (int i = tid; i < M * 7; i += SAMPLER_THREADS) latest[i] = 0.f;
    if (tid == 0) {
      *latest_count = 0;
      atomicOr(&q.status[R], SAST_RND_ITEM_INDEX);
    }
    return;
  }
  LabelStep lst = {0, 0, 0};
  for (int kk = L - 1; kk >= (q.only_load_end_labels ? L - 1 : 0); --kk) {
    const LabelStep c = row.step(w0 + kk);
    if (c.count > 0) {
      lst = c;
      break;
    }
  }
  row.copy(lst, latest, M, tid, SAMPLER_THREADS);
  if (tid == 0) *latest_count = lst.count;
}

// step k of item g -> column `col` of outputs whose batch axis holds `stride` columns, and with the last step latest / latest_count of
// sample b; every thread of a workgroup of SAMPLER_THREADS calls it
__device__ __forceinline__ void rnd_gather_step(const SastLabelArgs& a, const SastRndArgs& q, long long g, int k, int stride, int col, int b,
                                                const RndGatherOut& o) {
  const int tid = threadIdx.x;
  const int R = a.S, L = q.sequence_length, M = a.max_labels_per_frame;
  LabelRow row = {};
  long long w0 = 0;
  const int r = rnd_locate(a, q, g, &row, &w0);
  const size_t at = (size_t)k * stride + col;
  float* out = o.labels + at * M * 7;
  const bool last = k == L - 1;
  if (o.step_rows && tid == 0) {
    o.step_rows[at] = r;
    o.is_padded[at] = 0;
  }
  if (r < 0) {
    for (int i = tid; i < M * 7; i += SAMPLER_THREADS) out[i] = 0.f;
    if (tid == 0) {
      o.window_idx[at] = -1;
      o.ends_us[at] = -1;
      o.counts[at] = 0;
      o.labelled[at] = 0;
      if (k == 0) o.rows[col] = -1;
    }
  } else {
    const long long w = w0 + k;
    // only_load_end_labels: the steps before the last read as unlabelled
    const LabelStep st = (!q.only_load_end_labels || last) ? row.step(w) : LabelStep{0, 0, 0};
    row.copy(st, out, M, tid, SAMPLER_THREADS);
    if (tid == 0) {
      o.window_idx[at] = w;
      o.ends_us[at] = row.ends_us[w];
      o.counts[at] = st.count;
      o.labelled[at] = (unsigned char)st.labelled;
      if (k == 0) o.rows[col] = r;
    }
  }
  if (last) rnd_latest_rows(q, R, r, row, w0, M, o.latest + (size_t)b * M * 7, o.latest_count + b);
}
#endif  // __HIPCC__

// ---- the argument checks of the entry points (host)
inline bool stream_args(const SastStreamArgs* q) {
  return q && q->seq_row && q->seq_start && q->seq_stop && q->seq_samples && q->row_first_seq && q->row_count && q->n_seq && q->status &&
         q->sequence_length >= 1 && q->sequence_length <= 65535 && q->max_sequences >= 1 &&
         (q->guarantee_labels == 0 || q->guarantee_labels == 1);
}

// what sast_stream_next needs on top: a schedule for B batch rows
inline bool stream_schedule_args(const SastStreamArgs* q, int B) {
  return q->order && q->order_len && q->cursor && q->order_capacity >= 1 && B >= 1 && B <= 65535 &&
         (long long)B * q->order_capacity <= INT_MAX;
}

inline bool rnd_args(const SastRndArgs* q) {
  return q && q->start_idx_offset && q->length && q->cum && q->status && q->ticket && q->sequence_length >= 1 &&
         q->sequence_length <= 65535 && q->max_classes >= 1 && q->max_classes <= RND_MAX_CLASSES && q->class_total;
}

// B columns of L steps with M label rows each stay inside 32-bit element counts
inline bool sampler_batch_fits(long long B, int L, int M) { return B >= 1 && B * L * M <= INT_MAX / 8; }

}  // namespace sast
