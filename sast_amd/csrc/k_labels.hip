// Raw Prophesee box labels -> window ends and label tensors, S recordings side by side (include/sast_hip.h, "label front end").
//
// The reference does this offline on the CPU, per recording: apply_filters (scripts/genx/preprocess_dataset.py:191-284),
// get_base_delta_ts_for_labels_us (:287-299), labels_and_ev_repr_timestamps (:336-428), then ObjectLabelFactory
// (data/genx_utils/labels.py:149-198) when a sample is read.  lab_load_kernel is all of it for one row per workgroup: a recording has at
// most ~1e5 boxes and a few thousand label timestamps, and the walk that accepts label frames is sequential, so one 1024-thread
// workgroup per row passes over its row with a running carry (stable compactions by a workgroup scan), one lane walks the timestamps
// out of LDS, and the window ends, the frame -> window map and the label rows are written by all threads again.  No value crosses a
// row: every index is formed from the row's own base and clamped by the row's own counts, which are read on the device.
//
// Every fp32 / fp64 operation is the reference's single numpy / torch operation (this file is built with -ffp-contract=off): fp32
// x + w, clip and subtraction of the crop, w * w + h * h of the size filter; fp64 median, division and rint of the walk; numpy's
// linspace as arange * step + start with the last value set to stop, truncated to int64.
#include <climits>
#include "common.cuh"
#include "kernels.h"
#include "label_state.cuh"

namespace sast {
namespace {

constexpr int LAB_THREADS = 1024;
constexpr int LAB_WAVES = LAB_THREADS / 64;
constexpr int LAB_CHUNK = 2048;        // unique timestamps staged in LDS per step of the walk (16 KiB)
constexpr int LAB_FATAL = ~(SAST_LABELS_FRAME_OVERFULL | SAST_LABELS_WINDOW_INDEX);

struct LabRow {            // one row's slices of the workspace (sast_labels_ws_bytes)
  long long* ft;           // [cap] timestamps of the boxes that passed the filters
  long long* uts;          // [cap] their unique values
  float* fbox;             // [cap][6] x, y, w, h (cropped), class_id, class_confidence of the survivors
  int* ustart;             // [cap] first survivor of each unique timestamp
  int* fuidx;              // [max_frames] unique-timestamp index of each label frame
  int* pair_off;           // [max_frames] first window of the linspace between frames p and p + 1
  int* pair_n;             // [max_frames] its number of steps
};

__host__ __device__ inline size_t lab_row_bytes(long long cap, int max_frames) {
  const size_t c = (size_t)((cap + 1) & ~1LL), f = (size_t)((max_frames + 1) & ~1);
  return c * 8 * 2 + c * 24 + c * 4 + f * 4 * 3;
}

__device__ __forceinline__ LabRow lab_row(const SastLabelArgs& a, int s) {
  const size_t c = (size_t)((a.capacity + 1) & ~1LL), f = (size_t)((a.max_frames + 1) & ~1);
  char* p = reinterpret_cast<char*>(a.ws) + (size_t)s * lab_row_bytes(a.capacity, a.max_frames);
  LabRow r;
  r.ft = reinterpret_cast<long long*>(p);
  r.uts = r.ft + c;
  r.fbox = reinterpret_cast<float*>(r.uts + c);
  r.ustart = reinterpret_cast<int*>(r.fbox + c * 6);
  r.fuidx = r.ustart + c;
  r.pair_off = r.fuidx + f;
  r.pair_n = r.pair_off + f;
  return r;
}

// the row's flags as every thread sees them between two phases: nobody writes them between the two barriers
__device__ __forceinline__ int block_flags(const int* flags) {
  __syncthreads();
  const int f = *flags;
  __syncthreads();
  return f;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// the k-th smallest (0-based) of the m differences uts[j + 1] - uts[j] (all >= 1, at most `span`): bisection on the value, every thread
// ends with the same result.  cnt: one LDS word
__device__ long long lab_select(const long long* uts, int m, int k, long long span, int* cnt) {
  long long lo = 0, hi = span;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (threadIdx.x == 0) *cnt = 0;
    __syncthreads();
    int c = 0;
    for (int j = threadIdx.x; j < m; j += LAB_THREADS) c += (uts[j + 1] - uts[j] <= mid) ? 1 : 0;
    if (c) atomicAdd(cnt, c);
    __syncthreads();
    const int below = *cnt;
    __syncthreads();
    if (below >= k + 1) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// ObjectLabelFactory's clamp_to_frame_ (labels.py:37-50) and, with ds, scale_(0.5) (:316-334) on one surviving box -> row[7]; false:
// removed by remove_flat_labels_
__device__ __forceinline__ bool lab_factory(const SastLabelArgs& a, long long t, const float* b, float* row) {
  const float xmax = (float)(a.width - 1), ymax = (float)(a.height - 1);
  float x = clampf(b[0], 0.f, xmax), y = clampf(b[1], 0.f, ymax);
  const float x1 = clampf(b[0] + b[2], 0.f, xmax), y1 = clampf(b[1] + b[3], 0.f, ymax);
  float w = x1 - x, h = y1 - y;
  bool keep = true;
  if (a.downsample_by_2) {
    const float sx1 = fminf((x + w) * 0.5f, (float)(0.5 * a.width - 1.0)), sy1 = fminf((y + h) * 0.5f, (float)(0.5 * a.height - 1.0));
    x = x * 0.5f;
    y = y * 0.5f;
    w = sx1 - x;
    h = sy1 - y;
    keep = w > 0.f && h > 0.f;
  }
  row[0] = (float)t;
  row[1] = x; row[2] = y; row[3] = w; row[4] = h;
  row[5] = b[4]; row[6] = b[5];
  return keep;
}

__global__ __launch_bounds__(LAB_THREADS) void lab_load_kernel(SastLabelArgs a, const int* records, const long long* counts,
                                                               const unsigned char* reset) {
  const int s = blockIdx.x, tid = threadIdx.x;
  if (reset && !reset[s]) return;
  __shared__ int sm[LAB_WAVES];
  __shared__ int sh_flags, sh_cnt, sh_nfr, sh_total, sh_lead;
  __shared__ long long sh_base;
  __shared__ long long sh_chunk[LAB_CHUNK];

  const long long cap = a.capacity;
  const int n = (int)min(max(counts[s], 0LL), cap);
  const int* rec = records + (size_t)s * (size_t)cap * 10;
  const LabRow r = lab_row(a, s);
  const size_t row = (size_t)s * (size_t)cap;
  long long* ends = reinterpret_cast<long long*>(a.ends_us) + (size_t)s * a.max_windows;
  long long* fts = reinterpret_cast<long long*>(a.frame_ts_us) + (size_t)s * a.max_frames;
  long long* f2w = reinterpret_cast<long long*>(a.frame_2_window) + (size_t)s * a.max_frames;
  int* w2f = a.window_2_frame + (size_t)s * a.max_windows;
  int* fstart = a.frame_start + (size_t)s * a.max_frames;
  int* fcount = a.frame_count + (size_t)s * a.max_frames;

  if (tid == 0) { sh_flags = 0; sh_nfr = 0; sh_total = 0; sh_lead = 0; sh_base = a.base_delta_us; }
  __syncthreads();

  // ---- 1. the filters of apply_filters, in its order, and a stable compaction of the survivors
  const float xmax = (float)(a.width - 1), ymax = (float)(a.height - 1);
  int nf = 0, flags = 0;
  for (int base = 0; base < n; base += LAB_THREADS) {
    const int i = base + tid;
    bool keep = false;
    long long t = 0;
    float x = 0.f, y = 0.f, w = 0.f, h = 0.f, conf = 0.f;
    unsigned cls = 0;
    if (i < n) {
      const int* q = rec + (size_t)i * 10;
      t = (long long)(((unsigned long long)(unsigned)q[1] << 32) | (unsigned)q[0]);
      x = __int_as_float(q[2]); y = __int_as_float(q[3]); w = __int_as_float(q[4]); h = __int_as_float(q[5]);
      cls = (unsigned)q[6];
      conf = __int_as_float(q[8]);
      if (i > 0) {
        const long long tp = (long long)(((unsigned long long)(unsigned)q[1 - 10] << 32) | (unsigned)q[0 - 10]);
        if (t < tp) flags |= SAST_LABELS_UNSORTED;
      }
      if (w < 0.f || h < 0.f) flags |= SAST_LABELS_NEGATIVE_SIZE;
      keep = a.class_max < 0 || cls <= (unsigned)a.class_max;
      const float xr = clampf(x + w, 0.f, xmax), yb = clampf(y + h, 0.f, ymax);   // crop_to_fov_filter
      x = clampf(x, 0.f, xmax);
      y = clampf(y, 0.f, ymax);
      w = xr - x;
      h = yb - y;
      keep = keep && w > 0.f && h > 0.f;
      const float ww = w * w, hh = h * h;
      if (a.min_diag2 > 0.f) keep = keep && (ww + hh >= a.min_diag2);
      keep = keep && w >= a.min_side && h >= a.min_side;
      if (a.max_width >= 0.f) keep = keep && w <= a.max_width;
    }
    int tot;
    const int pos = nf + block_scan<LAB_WAVES>(keep ? 1 : 0, sm, &tot);
    if (keep) {
      r.ft[pos] = t;
      float* fb = r.fbox + (size_t)pos * 6;
      fb[0] = x; fb[1] = y; fb[2] = w; fb[3] = h; fb[4] = (float)cls; fb[5] = conf;
    }
    nf += tot;
  }
  if (flags) atomicOr(&sh_flags, flags);
  __syncthreads();                                   // ft / fbox visible to the whole workgroup
  if (tid == 0 && sh_flags == 0 && nf == 0) sh_flags = SAST_LABELS_NO_LABELS;

  // ---- 2. unique timestamps of the survivors (sorted input: a neighbour compare) and the first survivor of each
  int nu = 0;
  if (block_flags(&sh_flags) == 0) {
    for (int base = 0; base < nf; base += LAB_THREADS) {
      const int i = base + tid;
      const bool first = i < nf && (i == 0 || r.ft[i] != r.ft[i - 1]);
      int tot;
      const int pos = nu + block_scan<LAB_WAVES>(first ? 1 : 0, sm, &tot);
      if (first) { r.uts[pos] = r.ft[i]; r.ustart[pos] = i; }
      nu += tot;
    }
  }

  // ---- 3. the base delta (get_base_delta_ts_for_labels_us): given, or from np.median of the differences
  if (block_flags(&sh_flags) == 0 && a.base_delta_us == 0) {
    if (nu < 2) {
      if (tid == 0) sh_flags = SAST_LABELS_BAD_RATE;
    } else {
      const int m = nu - 1;
      const long long span = r.uts[nu - 1] - r.uts[0];
      const long long hi = lab_select(r.uts, m, m / 2, span, &sh_cnt);
      const long long lo = (m & 1) ? hi : lab_select(r.uts, m, m / 2 - 1, span, &sh_cnt);
      if (tid == 0) {
        const double median = (m & 1) ? (double)hi : ((double)lo + (double)hi) / 2.0;
        const double hz = rint(1000000.0 / median);
        if (hz == 60.0) sh_base = (long long)(6.0 * median);
        else if (hz == 30.0) sh_base = (long long)(3.0 * median);
        else sh_flags = SAST_LABELS_BAD_RATE;
      }
    }
  }

  // ---- 4. the label frames (:366-383): one lane walks the unique timestamps, staged through LDS a chunk at a time
  if (block_flags(&sh_flags) == 0) {
    // the first unique timestamp >= align_t_us: every thread searches, all find the same
    int first = 0;
    for (int lo = 0, hi = nu; ; ) {
      if (lo >= hi) { first = lo; break; }
      const int mid = lo + (hi - lo) / 2;
      if (r.uts[mid] < a.align_t_us) lo = mid + 1; else hi = mid;
    }
    if (first >= nu) {
      if (tid == 0) sh_flags = SAST_LABELS_NO_ALIGNED_LABEL;
    } else {
      // walk state, meaningful in thread 0 only
      long long ref = 0, total = 0;
      int nfr = 0, wflags = 0;
      const long long base_us = sh_base, d = a.delta_t_us;
      if (tid == 0) {
        ref = r.uts[first];
        fts[0] = ref;
        r.fuidx[0] = first;
        nfr = 1;
        const long long lead = ref > 0 ? max((ref + d - 1) / d - 2, 0LL) : 0LL;
        total = lead;
        if (total + 1 > a.max_windows) wflags = SAST_LABELS_TOO_MANY_WINDOWS;
        else sh_lead = (int)lead;
      }
      for (int c0 = first + 1; c0 < nu; c0 += LAB_CHUNK) {
        const int cn = min(LAB_CHUNK, nu - c0);
        for (int j = tid; j < cn; j += LAB_THREADS) sh_chunk[j] = r.uts[c0 + j];
        __syncthreads();
        if (tid == 0 && !wflags) {
          for (int j = 0; j < cn; ++j) {
            const long long ts = sh_chunk[j];
            const long long diff = ts - ref;
            const double q = rint((double)diff / (double)base_us);
            if (!(fabs(q) < 1e15)) continue;
            const long long cnt = (long long)q;
            const long long off = diff - cnt * base_us;
            if (off > 2000 || off < -2000) continue;
            if (cnt <= 0) wflags = SAST_LABELS_ZERO_COUNT;
            else if (nfr >= a.max_frames) wflags = SAST_LABELS_TOO_MANY_FRAMES;
            else if (diff <= 98000) wflags = SAST_LABELS_FRAMES_TOO_CLOSE;
            else if (total + cnt * a.reprs_per_frame + 1 > a.max_windows) wflags = SAST_LABELS_TOO_MANY_WINDOWS;
            if (wflags) break;
            r.pair_off[nfr - 1] = (int)total;
            r.pair_n[nfr - 1] = (int)(cnt * a.reprs_per_frame);
            total += cnt * a.reprs_per_frame;
            fts[nfr] = ts;
            r.fuidx[nfr] = c0 + j;
            ++nfr;
            ref = ts;
          }
        }
        __syncthreads();
      }
      if (tid == 0) {
        if (wflags) sh_flags = wflags;
        sh_nfr = nfr;
        sh_total = (int)total;
      }
    }
  }
  const int fatal = block_flags(&sh_flags) & LAB_FATAL;
  const int nfr = fatal ? 0 : sh_nfr;
  const int nw = fatal ? 0 : sh_total + 1;
  const int lead = sh_lead;

  // ---- 5. the window ends (:400-416)
  for (int i = tid; i < a.max_windows; i += LAB_THREADS) w2f[i] = -1;
  if (nfr > 0) {
    const long long f0 = fts[0];
    for (int i = tid; i < lead; i += LAB_THREADS) ends[i] = f0 - (long long)(lead - i) * a.delta_t_us;
    for (int p = tid; p < nfr - 1; p += LAB_THREADS) {
      const long long ta = fts[p], tb = fts[p + 1];
      const int np = r.pair_n[p], off = r.pair_off[p];
      const double start = (double)ta, delta = (double)tb - (double)ta;
      const double step = delta / (double)np;
      for (int i = 0; i < np; ++i) {
        const double v = (double)i * step;
        ends[off + i] = (long long)(v + start);
      }
      if (p == nfr - 2) ends[off + np] = tb;
    }
    if (nfr == 1 && tid == 0) ends[lead] = f0;
  }
  __syncthreads();

  // ---- 6. frame_2_window = searchsorted(ends, frame_ts, 'left') and its inverse
  for (int k = tid; k < nfr; k += LAB_THREADS) {
    const long long ts = fts[k];
    int lo = 0, hi = nw;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (ends[mid] < ts) lo = mid + 1; else hi = mid;
    }
    f2w[k] = lo;
    if (lo < nw) w2f[lo] = k;
  }

  // ---- 7. ObjectLabelFactory on the boxes of the label frames: a thread per frame, the frames' rows packed in frame order
  int lab_total = 0, overfull = 0;
  for (int base = 0; base < nfr; base += LAB_THREADS) {
    const int k = base + tid;
    int from = 0, to = 0, cnt = 0;
    float rowv[7];
    if (k < nfr) {
      const int u = r.fuidx[k];
      from = r.ustart[u];
      to = u + 1 < nu ? r.ustart[u + 1] : nf;
      for (int i = from; i < to; ++i) cnt += lab_factory(a, r.ft[i], r.fbox + (size_t)i * 6, rowv) ? 1 : 0;
      if (cnt > a.max_labels_per_frame) { cnt = a.max_labels_per_frame; overfull = 1; }
    }
    int tot;
    const int start = lab_total + block_scan<LAB_WAVES>(cnt, sm, &tot);
    if (k < nfr) {
      fstart[k] = start;
      fcount[k] = cnt;
      int o = 0;
      for (int i = from; i < to && o < cnt; ++i) {
        if (!lab_factory(a, r.ft[i], r.fbox + (size_t)i * 6, rowv)) continue;
        float* dst = a.labels + (row + (size_t)(start + o)) * 7;
#pragma unroll
        for (int c = 0; c < 7; ++c) dst[c] = rowv[c];
        ++o;
      }
    }
    lab_total += tot;
  }
  if (overfull) atomicOr(&sh_flags, SAST_LABELS_FRAME_OVERFULL);
  __syncthreads();
  if (tid == 0) {
    a.n_frames[s] = nfr;
    a.n_windows[s] = nw;
    a.status[s] = sh_flags;
  }
}

// LabelStreams.labels: one workgroup per (step, row)
__global__ __launch_bounds__(128) void lab_gather_kernel(SastLabelArgs a, const long long* window_idx, int T, float* labels, int* counts,
                                                         long long* ends_out, unsigned char* labelled) {
  const int b = blockIdx.x;               // k * S + s
  const int s = b % a.S;
  const long long w = window_idx[b];
  const LabelRow row = label_row(a, s);
  LabelStep st = {0, 0, 0};
  long long e = -1;
  if (w < 0 || w >= row.nw) {
    if (threadIdx.x == 0) atomicOr(&a.status[s], SAST_LABELS_WINDOW_INDEX);
  } else {
    e = row.ends_us[w];
    st = row.step(w);
  }
  row.copy(st, labels + (size_t)b * a.max_labels_per_frame * 7, a.max_labels_per_frame, threadIdx.x, blockDim.x);
  if (threadIdx.x == 0) {
    counts[b] = st.count;
    ends_out[b] = e;
    labelled[b] = (unsigned char)st.labelled;
  }
}

bool lab_args(const SastLabelArgs* a) {
  return label_state_ok(a) && a->ws && a->frame_ts_us && a->status && a->width >= 2 && a->height >= 2 && a->width <= 65536 &&
         a->height <= 65536 && a->base_delta_us >= 0 && a->delta_t_us >= 1 && a->align_t_us >= 0 && a->reprs_per_frame >= 1 &&
         a->reprs_per_frame <= 100 && a->min_side >= 0.f && a->min_diag2 >= 0.f;
}
}  // namespace
}  // namespace sast

extern "C" {

size_t sast_labels_ws_bytes(int S, int64_t capacity, int max_frames) {
  if (S < 1 || S > 65535 || capacity < 1 || (long long)S * capacity > INT_MAX / 16 || max_frames < 1) return 0;
  return (size_t)S * sast::lab_row_bytes(capacity, max_frames);
}

int sast_labels_load(const SastLabelArgs* a, const int32_t* records, const int64_t* counts, const uint8_t* reset, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::lab_args(a) || !records || !counts) return SAST_EINVAL;
  SAST_LAUNCH(sast::lab_load_kernel, dim3((unsigned)a->S), dim3(sast::LAB_THREADS), 0, (hipStream_t)stream, *a, records,
              reinterpret_cast<const long long*>(counts), reset);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_labels_gather(const SastLabelArgs* a, const int64_t* window_idx, int T, float* labels, int32_t* counts, int64_t* ends_us,
                       uint8_t* labelled, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::lab_args(a) || !window_idx || !labels || !counts || !ends_us || !labelled || T < 1 || (long long)a->S * T > INT_MAX / 8)
    return SAST_EINVAL;
  if ((long long)a->S * T * a->max_labels_per_frame > INT_MAX / 8) return SAST_EINVAL;
  SAST_LAUNCH(sast::lab_gather_kernel, dim3((unsigned)(a->S * T)), dim3(128), 0, (hipStream_t)stream, *a,
              reinterpret_cast<const long long*>(window_idx), T, labels, counts, reinterpret_cast<long long*>(ends_us), labelled);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
