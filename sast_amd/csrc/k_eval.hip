// Prophesee mAP evaluation of detections on the device.
//
// Reference: PropheseeEvaluator (utils/evaluation/prophesee/evaluator.py) -> evaluate_list (evaluation.py:5-42): to_prophesee
// (io/box_loading.py:58-99), filter_boxes (io/box_filtering.py:18-36) on labels and detections, _match_times with one frame per "file"
// (metrics/coco_eval.py:55-90), _to_coco_format (:143-194), then pycocotools' COCOeval (bbox, useCats, maxDets 100): evaluate,
// accumulate, summarize.  Entry points:
//   sast_eval_reset       clears the cursors, counters and record keys of a buffer
//   sast_eval_add         N frames of labels and padded detections: three launches, no host synchronisation
//                           count   one wave per frame: boxes that pass the filter, per category the detections that enter the matching
//                           scan    one thread: image / table / record offsets from the device cursors in frame order (the order decides
//                                   score ties, so no atomics), capacity checks that count what does not fit instead of dropping it
//                           match   one wave per (frame, category): the flattened tables (category 0's wave), the category's detections
//                                   ranked by a stable descending sort on the score (bitonic network in LDS on (score, index) keys),
//                                   cut to 100, the fp64 IoU tile in LDS, then COCOeval's greedy matching with one lane per
//                                   (area range, IoU threshold) pair: 40 lanes.  One record per detection: sort key, 40 match bits, 40
//                                   ignore bits and, above them, the detection's rank in its (image, category) group.
//   sast_eval_accumulate  one device-wide radix sort (rocprim) of the record keys (category, descending score, record index: unique, so
//                         the order is the stable one), the chunk-parallel walk of every category's sorted records (counts, scan over
//                         the chunks, precision maxima, envelope, backward walk: the 101 recall thresholds), and the six summaries.
//   sast_evsum_accumulate behind sast_eval_accumulate, on the `sorted` array it leaves: the same five launches at maxDets 1, 10 and 100
//                         at once (a record whose rank is past the maxDet counts as ignored), which also write COCOeval's recall and
//                         score tables, then the twelve stats and the per-category numbers.  Six launches, no host synchronisation
//   sast_evmerge_append   one buffer behind another (two launches, no host synchronisation): what joins the buffers of several ranks
//   sast_evrec_add        S whole recordings as sorted 40-byte box records, labels and detections: evaluate_detection's loop over
//                         "files" (coco_eval.py:42-51) with _match_times' windows.  Four launches, no host synchronisation
//                           images  one 1024-thread workgroup per row: the sorted check, then the first passing label of every
//                                   timestamp, compacted by a workgroup scan into the row's list of image starts
//                           count, scan, match   the kernels of sast_eval_add, instantiated on record ranges: an image's labels are the
//                                   records of its timestamp, its detections the records with t - tol <= t_det <= t + tol (two
//                                   binary searches), each filtered on its own; the scan walks the images, not the label slots
//   sast_detlog_append    the exported records of one online step behind the per-stream logs sast_evrec_add reads (one launch)
// The count and match kernels read an image's rows through a SOURCE they are parameterised on: FrameRows (padded [N, M, 7] /
// [N, A, 7] rows, one frame per image) or RecordRows (ranges of records).  There is one matching.
// Every fp32 / fp64 operation of the reference is repeated one rounding at a time: build.py compiles this file with -ffp-contract=off.
#include "box_rules.cuh"
#include "common.cuh"
#include "kernels.h"

#include <climits>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

namespace sast {
namespace {

constexpr int EV_T = SAST_EVAL_IOU_THRS;      // 10
constexpr int EV_R = SAST_EVAL_REC_THRS;      // 101
constexpr int EV_A = SAST_EVAL_AREAS;         // 4
constexpr int EV_LANES = EV_T * EV_A;         // 40: lane = area * 10 + threshold
constexpr int EV_MAXDET = 100;
constexpr int EV_M = SAST_EVSUM_MAXDETS;      // 3: maxDets 1, 10, 100
constexpr unsigned long long EV_LANE_MASK = (1ull << EV_LANES) - 1;
constexpr int EV_RANK_SHIFT = 40;             // rec_ign bits 40..46: the record's rank in its (image, category) group
constexpr int EV_INFO = 16;                   // int32 words of per-frame scratch
constexpr unsigned long long EV_IDX_MASK = (1ull << 30) - 1;
constexpr int EV_MAX_ANCHORS = 8192, EV_MAX_LABELS = 128;

// state words
enum { ST_IMAGES = 0, ST_GT = 1, ST_DET = 2, ST_REC = 3, ST_REC_CAT = 4, ST_ERR_IMAGES = 8, ST_ERR_DETS = 9, ST_ERR_LABELS = 10, ST_ADDS = 11, ST_NPIG = 12,
       ST_ERR_WINDOW = 28, ST_ERR_UNSORTED = 29 };
// info words of a frame (an image candidate); 12..15 are RecordRows' alone
enum { IN_VALID = 0, IN_NGT = 1, IN_NDT = 2, IN_NREC = 3, IN_IMG = 8, IN_GT_OFF = 9, IN_DET_OFF = 10, IN_REC_OFF = 11,
       IN_GHI = 12, IN_DLO = 13, IN_DHI = 14, IN_OVER = 15 };
constexpr int REC_WORDS = SAST_DET_RECORD_BYTES / 4;   // a BBOX_DTYPE record as int32 words: 0-1 t, 2-5 x y w h, 6 class_id, 8 score
constexpr int EV_MAX_WINDOW = 8192;

// box_passes / label_passes (filter_boxes) are box_rules.cuh's: the tracking evaluator applies the same filter

__device__ __forceinline__ unsigned class_of(float v) { return (unsigned)(long long)v; }

// ascending on the result = ascending on the float (-0 == +0)
__device__ __forceinline__ unsigned score_key(float s) {
  if (s == 0.f) s = 0.f;
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int frame_labels(const SastEvalArgs& a, int n) { return min(max(a.counts[n], 0), a.M); }
__device__ __forceinline__ int frame_dets(const SastEvalArgs& a, int n) { return min(max(a.n_det[n], 0), a.A); }

// ---- the two sources of an image's rows.  A source answers: how many label / detection rows the image has, whether row i passes
// filter_boxes and what its box is, whether the detections count at all, and the image's timestamp.  `open` is the count kernel's
// (it may leave what it found in the image's info words), `reopen` the match kernel's.
struct Box {
  float x, y, w, h, score;
  unsigned cls;
};

// sast_eval_add: frame n of padded label rows [N, M, 7] and padded detections [N, A, 7]
struct FrameRows {
  struct Args {};
  const float* lab;
  const float* dt;
  int cnt, nd;
  __device__ __forceinline__ void bind(const SastEvalArgs& a, int n) {
    lab = a.labels + (size_t)n * a.M * 7, dt = a.det + (size_t)n * a.A * 7;
    cnt = frame_labels(a, n), nd = frame_dets(a, n);
  }
  __device__ __forceinline__ bool open(const SastEvalArgs& a, const Args&, int n, int*, int) {
    bind(a, n);
    return true;
  }
  __device__ __forceinline__ void reopen(const SastEvalArgs& a, const Args&, int n, const int*) { bind(a, n); }
  __device__ __forceinline__ int labels_n() const { return cnt; }
  __device__ __forceinline__ int dets_n() const { return nd; }
  __device__ __forceinline__ bool dets_live() const { return (long long)lab[0] > EV_SKIP_US; }   // the detections carry the frame's one timestamp (box_loading.py:90)
  __device__ __forceinline__ long long time() const { return (long long)lab[0]; }
  __device__ __forceinline__ bool label(const SastEvalArgs& a, int i, Box& b) const {
    const float* r = lab + i * 7;
    b.x = r[1], b.y = r[2], b.w = r[3], b.h = r[4], b.score = r[6], b.cls = class_of(r[5]);
    return label_passes(r, a.min_diag2, a.min_side);
  }
  __device__ __forceinline__ bool det(const SastEvalArgs& a, int i, Box& b) const {
    const float* r = dt + (size_t)i * 7;
    b.x = r[0], b.y = r[1], b.w = r[2] - r[0], b.h = r[3] - r[1], b.score = r[5], b.cls = class_of(r[6]);
    return box_passes(b.w, b.h, a.min_diag2, a.min_side);
  }
};

__device__ __forceinline__ long long rec_time(const int* row, long long i) { return *reinterpret_cast<const long long*>(row + i * REC_WORDS); }

__device__ __forceinline__ bool rec_box(const int* row, long long i, float diag2, float side, Box& b) {
  const int* r = row + i * REC_WORDS;
  b.x = __int_as_float(r[2]), b.y = __int_as_float(r[3]), b.w = __int_as_float(r[4]), b.h = __int_as_float(r[5]);
  b.cls = (unsigned)r[6], b.score = __int_as_float(r[8]);
  return rec_time(row, i) > EV_SKIP_US && box_passes(b.w, b.h, diag2, side);
}

// first index in [lo, hi) of a sorted row whose t is >= v (strict: > v)
__device__ __forceinline__ int rec_bound(const int* row, int lo, int hi, long long v, bool strict) {
  while (lo < hi) {
    const int m = lo + ((hi - lo) >> 1);
    const long long t = rec_time(row, m);
    if (strict ? t <= v : t < v) lo = m + 1;
    else hi = m;
  }
  return lo;
}

__device__ __forceinline__ int rec_rows(const long long* n, int s, int cap) { return (int)min(max(n[s], 0ll), (long long)cap); }

// sast_evrec_add: image j of row s (n = s * Gcap + j) is the j-th entry of the row's list of image starts.  Its labels are the records
// of that timestamp, its detections the records inside [t - tol, t + tol]; both rows were found sorted by evrec_images_kernel.
struct RecordRows {
  struct Args {
    const int* gt;
    const long long* n_gt;
    const int* dt;
    const long long* n_dt;
    int* starts;     // [S][Gcap] label index of a row's images, ascending
    int* nimg;       // [S]
    int* unsorted;   // [S]
    int S, Gcap, Dcap, max_window;
    long long tol;
  };
  const int* g;
  const int* d;
  int cnt, nd;
  long long t;
  bool over;
  __device__ __forceinline__ int first(const Args& r, int n, int s, const int*& grow) {
    grow = r.gt + (size_t)s * r.Gcap * REC_WORDS;
    return min(max(r.starts[n], 0), max(rec_rows(r.n_gt, s, r.Gcap) - 1, 0));
  }
  __device__ __forceinline__ bool open(const SastEvalArgs&, const Args& r, int n, int* info, int lane) {
    const int s = n / r.Gcap, j = n - s * r.Gcap;
    if (j >= min(r.nimg[s], r.Gcap)) return false;
    const int ng = rec_rows(r.n_gt, s, r.Gcap), ndt = rec_rows(r.n_dt, s, r.Dcap);
    const int* grow;
    const int i0 = first(r, n, s, grow);
    const int* drow = r.dt + (size_t)s * r.Dcap * REC_WORDS;
    t = rec_time(grow, i0);
    const int ghi = rec_bound(grow, i0, ng, t, true);
    const long long lo_t = t < LLONG_MIN + r.tol ? LLONG_MIN : t - r.tol, hi_t = t > LLONG_MAX - r.tol ? LLONG_MAX : t + r.tol;
    const int dlo = rec_bound(drow, 0, ndt, lo_t, false), dhi = rec_bound(drow, dlo, ndt, hi_t, true);
    over = dhi - dlo > r.max_window;
    if (lane == 0) info[IN_GHI] = ghi, info[IN_DLO] = dlo, info[IN_DHI] = dhi, info[IN_OVER] = over;
    g = grow + (size_t)i0 * REC_WORDS, cnt = ghi - i0;
    d = drow + (size_t)dlo * REC_WORDS, nd = dhi - dlo;
    return true;
  }
  __device__ __forceinline__ void reopen(const SastEvalArgs&, const Args& r, int n, const int* info) {
    const int s = n / r.Gcap;
    const int* grow;
    const int i0 = first(r, n, s, grow);
    t = rec_time(grow, i0), over = false;
    g = grow + (size_t)i0 * REC_WORDS, cnt = info[IN_GHI] - i0;
    d = r.dt + ((size_t)s * r.Dcap + info[IN_DLO]) * REC_WORDS, nd = info[IN_DHI] - info[IN_DLO];
  }
  __device__ __forceinline__ int labels_n() const { return cnt; }
  __device__ __forceinline__ int dets_n() const { return nd; }
  __device__ __forceinline__ bool dets_live() const { return !over; }   // a window over max_window is refused by the scan
  __device__ __forceinline__ long long time() const { return t; }
  __device__ __forceinline__ bool label(const SastEvalArgs& a, int i, Box& b) const { return rec_box(g, i, a.min_diag2, a.min_side, b); }
  __device__ __forceinline__ bool det(const SastEvalArgs& a, int i, Box& b) const { return rec_box(d, i, a.min_diag2, a.min_side, b); }
};

template <class Src>
__global__ void __launch_bounds__(64) eval_count_kernel(SastEvalArgs a, typename Src::Args sa) {
  const int n = blockIdx.x, lane = threadIdx.x;
  int* info = a.info + n * EV_INFO;
  Src src;
  if (!src.open(a, sa, n, info, lane)) {   // no image behind this slot
    if (lane == 0) info[IN_VALID] = 0;
    return;
  }
  const int cnt = src.labels_n();
  Box b;
  int ngt = 0, ndt = 0, c[SAST_EVAL_MAX_CLASSES] = {0, 0, 0, 0};
  for (int base = 0; base < cnt; base += 64) {
    const int i = base + lane;
    ngt += __popcll(__ballot(i < cnt && src.label(a, i, b)));
  }
  if (ngt > 0 && src.dets_live()) {
    const int nd = src.dets_n();
    for (int base = 0; base < nd; base += 64) {
      const int i = base + lane;
      const bool keep = i < nd && src.det(a, i, b);
      const unsigned cls = keep ? b.cls : 0u;
      ndt += __popcll(__ballot(keep));
#pragma unroll
      for (int k = 0; k < SAST_EVAL_MAX_CLASSES; ++k) c[k] += __popcll(__ballot(keep && cls == (unsigned)k));
    }
  }
  if (lane == 0) {
    info[IN_VALID] = ngt > 0;
    info[IN_NGT] = ngt;
    info[IN_NDT] = ndt;
#pragma unroll
    for (int k = 0; k < SAST_EVAL_MAX_CLASSES; ++k) info[IN_NREC + k] = k < a.K ? min(c[k], EV_MAXDET) : 0;
  }
}

// the sequential part of an add: image / table / record offsets in image order, capacity checks that count instead of dropping
struct ScanCursor {
  int img, gt, dt, rec;
};

__device__ __forceinline__ void scan_image(const SastEvalArgs& a, int* info, ScanCursor& c) {
  int* st = a.state;
  int nrec = 0;
  for (int k = 0; k < a.K; ++k) nrec += info[IN_NREC + k];
  int* err = nullptr;
  if (info[IN_NGT] > a.max_labels_per_frame) err = st + ST_ERR_LABELS;
  else if (c.img >= a.max_images) err = st + ST_ERR_IMAGES;
  else if ((long long)c.dt + info[IN_NDT] > a.max_detections) err = st + ST_ERR_DETS;
  if (err) {   // counted, reported by the host at evaluate time; the frame writes nothing
    *err += 1;
    info[IN_VALID] = 0;
    return;
  }
  info[IN_IMG] = c.img, info[IN_GT_OFF] = c.gt, info[IN_DET_OFF] = c.dt, info[IN_REC_OFF] = c.rec;
  c.img += 1, c.gt += info[IN_NGT], c.dt += info[IN_NDT], c.rec += nrec;
  for (int k = 0; k < a.K; ++k) st[ST_REC_CAT + k] += info[IN_NREC + k];
}

__device__ __forceinline__ ScanCursor scan_begin(const int* st) { return ScanCursor{st[ST_IMAGES], st[ST_GT], st[ST_DET], st[ST_REC]}; }

__device__ __forceinline__ void scan_end(int* st, const ScanCursor& c) {
  st[ST_IMAGES] = c.img, st[ST_GT] = c.gt, st[ST_DET] = c.dt, st[ST_REC] = c.rec;
  st[ST_ADDS] += 1;   // a replayed graph adds without the host's knowledge: "has data" is decided from this word
}

__global__ void eval_scan_kernel(SastEvalArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  ScanCursor c = scan_begin(a.state);
  for (int n = 0; n < a.N; ++n) {
    int* info = a.info + n * EV_INFO;
    if (info[IN_VALID]) scan_image(a, info, c);
  }
  scan_end(a.state, c);
}

// rows in order, and within a row its images: the walk is as long as the images, whatever Gcap is
__global__ void evrec_scan_kernel(SastEvalArgs a, RecordRows::Args r) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  ScanCursor c = scan_begin(a.state);
  for (int s = 0; s < r.S; ++s) {
    if (r.unsorted[s]) {   // the reference asserts (coco_eval.py:43-44): the row adds nothing
      a.state[ST_ERR_UNSORTED] += 1;
      continue;
    }
    const int ni = min(max(r.nimg[s], 0), r.Gcap);
    for (int j = 0; j < ni; ++j) {
      int* info = a.info + (s * r.Gcap + j) * EV_INFO;
      if (!info[IN_VALID]) continue;
      if (info[IN_OVER]) {   // more records in the window than the LDS sort was sized for
        a.state[ST_ERR_WINDOW] += 1;
        info[IN_VALID] = 0;
        continue;
      }
      scan_image(a, info, c);
    }
  }
  scan_end(a.state, c);
}

// One workgroup per row.  A row with a record whose t is below its predecessor's, labels or detections, gets no image.  Otherwise
// label i starts an image when it passes the filter and no passing label of the same t lies before it; the starts are compacted in
// order: per tile of 1024 slots a ballot per wave, the waves' counts through LDS.
__global__ void __launch_bounds__(1024) evrec_images_kernel(SastEvalArgs a, RecordRows::Args r) {
  __shared__ int wcount[16];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ng = rec_rows(r.n_gt, s, r.Gcap), nd = rec_rows(r.n_dt, s, r.Dcap);
  const int* grow = r.gt + (size_t)s * r.Gcap * REC_WORDS;
  const int* drow = r.dt + (size_t)s * r.Dcap * REC_WORDS;
  int bad = 0;
  for (int i = tid + 1; i < ng; i += 1024) bad |= rec_time(grow, i) < rec_time(grow, i - 1);
  for (int i = tid + 1; i < nd; i += 1024) bad |= rec_time(drow, i) < rec_time(drow, i - 1);
  bad = __syncthreads_or(bad);
  if (bad) {
    if (tid == 0) r.nimg[s] = 0, r.unsorted[s] = 1;
    return;
  }
  int* starts = r.starts + (size_t)s * r.Gcap;
  int total = 0;
  Box b;
  for (int base = 0; base < ng; base += 1024) {   // ng is the workgroup's: every thread takes every turn
    const int i = base + tid;
    bool start = i < ng && rec_box(grow, i, a.min_diag2, a.min_side, b);
    if (start) {
      const long long t = rec_time(grow, i);
      for (int j = i - 1; j >= 0 && rec_time(grow, j) == t; --j)
        if (rec_box(grow, j, a.min_diag2, a.min_side, b)) {
          start = false;
          break;
        }
    }
    const unsigned long long m = __ballot(start);
    if (lane == 0) wcount[wave] = __popcll(m);
    __syncthreads();
    int before = 0, tile = 0;
    for (int w = 0; w < 16; ++w) {
      before += w < wave ? wcount[w] : 0;
      tile += wcount[w];
    }
    if (start) starts[total + before + __popcll(m & ((1ull << lane) - 1))] = i;   // < ng <= Gcap: one slot per start
    total += tile;
    __syncthreads();
  }
  if (tid == 0) r.nimg[s] = total, r.unsorted[s] = 0;
}

struct MatchLds {
  unsigned long long* keys;   // [P]      } one region
  double* iou;                // [100][G] }
  double* dbox;               // [100][4] x y w h
  double* darea;              // [100]
  double* gbox;               // [G][4]
  double* garea;              // [G]
  float* dscore;              // [100]
  int* dsel;                  // [100]
  unsigned short* gord;       // [4][G]
  unsigned char* gig;         // [4][G]
  unsigned char* gm;          // [G][64]
};

__host__ __device__ inline size_t match_lds_carve(unsigned char* base, int P, int G, MatchLds* l) {
  size_t o = 0;
  const size_t un = (size_t)8 * (P > EV_MAXDET * G ? P : EV_MAXDET * G);
  if (l) l->keys = (unsigned long long*)(base + o), l->iou = (double*)(base + o);
  o += un;
  if (l) l->dbox = (double*)(base + o);
  o += 8 * EV_MAXDET * 4;
  if (l) l->darea = (double*)(base + o);
  o += 8 * EV_MAXDET;
  if (l) l->gbox = (double*)(base + o);
  o += (size_t)8 * G * 4;
  if (l) l->garea = (double*)(base + o);
  o += (size_t)8 * G;
  if (l) l->dscore = (float*)(base + o);
  o += 4 * EV_MAXDET;
  if (l) l->dsel = (int*)(base + o);
  o += 4 * EV_MAXDET;
  if (l) l->gord = (unsigned short*)(base + o);
  o += (size_t)2 * EV_A * G;
  if (l) l->gig = (unsigned char*)(base + o);
  o += (size_t)EV_A * G;
  o = (o + 7) & ~(size_t)7;
  if (l) l->gm = base + o;
  o += (size_t)64 * G;
  return o;
}

__device__ __forceinline__ void area_range(int ar, double& lo, double& hi) {
  lo = ar == 2 ? 1024.0 : ar == 3 ? 9216.0 : 0.0;       // 32^2, 96^2
  hi = ar == 1 ? 1024.0 : ar == 2 ? 9216.0 : 1e10;      // (1e5)^2
}

template <class Src>
__global__ void __launch_bounds__(64) eval_match_kernel(SastEvalArgs a, typename Src::Args sa, int P) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int n = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
  const int* info = a.info + n * EV_INFO;
  if (!info[IN_VALID]) return;
  const int G = a.max_labels_per_frame;
  MatchLds l;
  match_lds_carve(lds_raw, P, G, &l);
  const unsigned long long lt = (1ull << lane) - 1;
  Src src;
  src.reopen(a, sa, n, info);
  const int cnt = src.labels_n(), nd_all = info[IN_NDT] > 0 ? src.dets_n() : 0;
  const int img = info[IN_IMG];
  Box b;

  // ---- the flattened tables, in frame order (category 0's wave)
  if (k == 0) {
    int go = info[IN_GT_OFF], dofs = info[IN_DET_OFF];
    for (int base = 0; base < cnt; base += 64) {
      const int i = base + lane;
      const bool keep = i < cnt && src.label(a, i, b);
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int p = go + __popcll(m & lt);
        a.gt_box[(size_t)p * 4 + 0] = b.x, a.gt_box[(size_t)p * 4 + 1] = b.y, a.gt_box[(size_t)p * 4 + 2] = b.w, a.gt_box[(size_t)p * 4 + 3] = b.h;
        a.gt_cls[p] = (int)b.cls;
        a.gt_img[p] = img;
      }
      go += __popcll(m);
    }
    for (int base = 0; base < nd_all; base += 64) {
      const int i = base + lane;
      const bool keep = i < nd_all && src.det(a, i, b);
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int p = dofs + __popcll(m & lt);
        float* o = a.det_box + (size_t)p * 5;
        o[0] = b.x, o[1] = b.y, o[2] = b.w, o[3] = b.h, o[4] = b.score;
        a.det_cls[p] = (int)b.cls;
        a.det_img[p] = img;
      }
      dofs += __popcll(m);
    }
    if (lane == 0) a.img_t[img] = src.time();
  }

  // ---- ground truth of category k, in label order
  int ng = 0;
  for (int base = 0; base < cnt; base += 64) {
    const int i = base + lane;
    const bool keep = i < cnt && src.label(a, i, b) && b.cls == (unsigned)k;
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int p = ng + __popcll(m & lt);   // < G: the scan refused frames with more boxes than that
      l.gbox[p * 4 + 0] = b.x, l.gbox[p * 4 + 1] = b.y, l.gbox[p * 4 + 2] = b.w, l.gbox[p * 4 + 3] = b.h;
      l.garea[p] = (double)(b.w * b.h);      // the fp32 product, widened (coco_eval.py:167, :172)
    }
    ng += __popcll(m);
  }
  // ---- detections of category k: keys (descending score, ascending index), sorted
  int c = 0;
  for (int base = 0; base < nd_all; base += 64) {
    const int i = base + lane;
    const bool keep = i < nd_all && src.det(a, i, b) && b.cls == (unsigned)k;
    const unsigned long long m = __ballot(keep);
    if (keep) l.keys[c + __popcll(m & lt)] = ((unsigned long long)(~score_key(b.score)) << 32) | (unsigned)i;
    c += __popcll(m);
  }
  int P2 = 1;
  while (P2 < c) P2 <<= 1;   // <= P: c <= A (FrameRows), c <= max_window (RecordRows)
  for (int i = c + lane; i < P2; i += 64) l.keys[i] = ~0ull;
  __syncthreads();
  for (int size = 2; size <= P2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < (P2 >> 1); t += 64) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const unsigned long long u = l.keys[i], v = l.keys[j];
        if ((u > v) == ((i & size) == 0)) l.keys[i] = v, l.keys[j] = u;
      }
      __syncthreads();
    }
  const int nd = min(c, EV_MAXDET);
  for (int d = lane; d < nd; d += 64) l.dsel[d] = (int)(l.keys[d] & 0xffffffffu);
  __syncthreads();   // the key region becomes the IoU tile
  for (int d = lane; d < nd; d += 64) {
    src.det(a, l.dsel[d], b);
    l.dbox[d * 4 + 0] = b.x, l.dbox[d * 4 + 1] = b.y, l.dbox[d * 4 + 2] = b.w, l.dbox[d * 4 + 3] = b.h;
    l.darea[d] = (double)(b.w * b.h);
    l.dscore[d] = b.score;
  }
  for (int e = lane; e < ng * 64; e += 64) l.gm[e] = 0;
  if (lane < EV_A) {   // per area range: ignore flags, and the ground truths not ignored first, stably
    double lo, hi;
    area_range(lane, lo, hi);
    int p = 0;
    for (int g = 0; g < ng; ++g) {
      const bool ig = l.garea[g] < lo || l.garea[g] > hi;
      l.gig[lane * G + g] = ig;
      if (!ig) l.gord[lane * G + p++] = (unsigned short)g;
    }
    if (p > 0) atomicAdd(a.state + ST_NPIG + k * EV_A + lane, p);
    for (int g = 0; g < ng; ++g)
      if (l.gig[lane * G + g]) l.gord[lane * G + p++] = (unsigned short)g;
  }
  __syncthreads();
  for (int e = lane; e < nd * ng; e += 64) {
    const int d = e / ng, g = e - d * ng;
    const double dx = l.dbox[d * 4], dy = l.dbox[d * 4 + 1], dw = l.dbox[d * 4 + 2], dh = l.dbox[d * 4 + 3];
    const double gx = l.gbox[g * 4], gy = l.gbox[g * 4 + 1], gw = l.gbox[g * 4 + 2], gh = l.gbox[g * 4 + 3];
    const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx), ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    double o = 0.0;
    if (iw > 0 && ih > 0) {
      const double in = iw * ih;
      const double un = dw * dh + gw * gh - in;
      o = in / un;
    }
    l.iou[e] = o;
  }
  __syncthreads();
  if (nd == 0) return;

  // ---- COCOeval.evaluateImg: the detections in score order, one lane per (area range, threshold)
  const int ar = lane / EV_T, th = lane - ar * EV_T;
  const bool active = lane < EV_LANES;
  double lo = 0, hi = 0;
  const double thr = active ? fmin(a.iou_thr[th], 1 - 1e-10) : 2.0;
  if (active) area_range(ar, lo, hi);
  const unsigned short* ord = l.gord + (active ? ar : 0) * G;
  const unsigned char* ig = l.gig + (active ? ar : 0) * G;
  int rec = info[IN_REC_OFF];
  for (int kk = 0; kk < k; ++kk) rec += info[IN_NREC + kk];
  for (int d = 0; d < nd; ++d) {
    int m = -1;
    if (active) {
      double best = thr;
      for (int q = 0; q < ng; ++q) {
        const int g = ord[q];
        if (l.gm[g * 64 + lane]) continue;
        if (m > -1 && !ig[m] && ig[g]) break;
        const double v = l.iou[d * ng + g];
        if (v < best) continue;
        best = v, m = g;
      }
      if (m > -1) l.gm[m * 64 + lane] = 1;
    }
    const bool ign = active && (m > -1 ? ig[m] != 0 : (l.darea[d] < lo || l.darea[d] > hi));
    const unsigned long long mb = __ballot(m > -1), ib = __ballot(ign);
    if (lane == 0) {
      const int ro = rec + d;
      a.rec_match[ro] = mb, a.rec_ign[ro] = ib | ((unsigned long long)d << EV_RANK_SHIFT);   // d <= 99: the rank in the group
      a.rec_key[ro] = ((unsigned long long)k << 62) | ((unsigned long long)(~score_key(l.dscore[d])) << 30) | (unsigned long long)ro;
    }
  }
}

__global__ void eval_reset_kernel(SastEvalArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < SAST_EVAL_STATE_WORDS) a.state[i] = 0;
  if (i < a.max_detections) a.rec_key[i] = ~0ull;
}

// ---- COCOeval.accumulate, chunk-parallel.  A category's sorted records are cut into chunks of L records; chunk c of category k is the
// flat chunk q = (chunks of the categories before k) + c, and every per-chunk partial is one row of 64 lanes (40 in use: lane = area * 10
// + threshold, as in the matching) in the workspace.  Five launches, each ordered behind the one before by the stream:
//   count    per chunk and lane: true and false positives among its records that are not ignored
//   scan     per category, over its chunks: the counts become inclusive prefix sums (a chunk's right edge; its left edge is the row
//            before).  Also the two cases no chunk writes: npig == 0 (-1 everywhere) and a category without records (0 everywhere).
//   max      per chunk: the largest precision at a record inside it, from the left-edge counts
//   envelope per category: inclusive suffix maxima of those over the chunks
//   walk     per chunk, backwards from the right-edge counts and the envelope entering from the right: exactly the sequential walk's
//            loop.  Recall is monotone in the true-positive count, so the thresholds with recall(left edge) < threshold <= recall(right
//            edge) are first reached in this chunk and in no other; the walk stops writing at the left edge by itself.  The last chunk
//            also writes the thresholds above the final recall (0), the first the thresholds no recall is below (threshold 0).
// Every count is an integer and every precision / recall is the same fp64 division of the same integers as in a sequential walk, the
// envelope is a maximum of those: the table is the same bits for every L.
struct AccWs {
  int* tp;       // [chunks][64]
  int* fp;       // [chunks][64]
  double* mx;    // [chunks][64]
};
constexpr size_t ACC_WS_PER_CHUNK = 64 * (2 * sizeof(int) + sizeof(double));   // 1 KiB

__host__ __device__ inline long long acc_max_chunks(long long max_detections, int L) { return (max_detections + L - 1) / L + SAST_EVAL_MAX_CLASSES; }

__host__ __device__ inline AccWs acc_ws_carve(void* ws, long long chunks) {
  AccWs w;
  w.mx = (double*)ws;                       // the doubles first: 8-byte aligned whatever the chunk count
  w.tp = (int*)(w.mx + chunks * 64);
  w.fp = w.tp + chunks * 64;
  return w;
}

struct AccCat {
  int start, n;        // the category's records are sorted[start, start + n)
  long long q0, nck;   // its chunks are the flat chunks [q0, q0 + nck)
};

// the category's span, from the device's record counts clamped to the capacity (every index below is formed from these)
__device__ __forceinline__ AccCat acc_category(const SastEvalArgs& a, int k, int L) {
  AccCat c{0, 0, 0, 0};
  long long left = a.max_detections;
  for (int kk = 0; kk <= k; ++kk) {
    const int n = (int)min((long long)max(a.state[ST_REC_CAT + kk], 0), left);
    left -= n;
    if (kk < k) c.start += n, c.q0 += ((long long)n + L - 1) / L;
    else c.n = n, c.nck = ((long long)n + L - 1) / L;
  }
  return c;
}

struct AccChunk {
  int k, lo, cnt;           // category; records sorted[lo, lo + cnt)
  long long c, nck, q0;     // chunk c of nck; the category's first flat chunk
};

__device__ __forceinline__ bool acc_chunk(const SastEvalArgs& a, long long q, int L, AccChunk& p) {
  for (int k = 0; k < a.K; ++k) {
    const AccCat c = acc_category(a, k, L);
    if (q >= c.q0 && q < c.q0 + c.nck) {
      p.k = k, p.c = q - c.q0, p.nck = c.nck, p.q0 = c.q0;
      const long long off = p.c * L;                     // < n
      p.lo = c.start + (int)off;
      p.cnt = (int)min((long long)L, (long long)c.n - off);
      return true;
    }
  }
  return false;
}

// ---- the five launches are templates on SUM.  SUM = false is sast_eval_accumulate: maxDets 100, the table a.precision [T][R][K][A].
// SUM = true is sast_evsum_accumulate: blockIdx.y picks the maxDet (1, 10, 100), the tables are [T][R][K][A][3] plus scores and recall,
// and the partials of maxDet mi are the rows [mi * chunks, (mi + 1) * chunks) of the workspace.  For maxDet m a record of rank >= m in
// its (image, category) group is not among the image's first m detections (cocoeval.py cuts every image to [0:maxDet]); the records
// left are a subsequence of the sorted order, so such a record only has to count for nothing: it is loaded as ignored in all 40 lanes.
struct AccSum {
  double* precision;   // [T][R][K][A][3]
  double* scores;      // [T][R][K][A][3]
  double* recall;      // [T][K][A][3]
  long long chunks;    // workspace rows of one maxDet
};

__device__ __forceinline__ int sum_maxdet(int mi) { return mi == 0 ? 1 : mi == 1 ? 10 : EV_MAXDET; }

// the first element of column (threshold th, category k, area ar, maxDet mi) of a [T][R][K][A](x [3]) table; rs: its stride over R
template <bool SUM>
__device__ __forceinline__ size_t acc_column(const SastEvalArgs& a, int th, int k, int ar, int mi, size_t& rs) {
  const size_t M = SUM ? EV_M : 1;
  rs = (size_t)a.K * EV_A * M;
  return ((size_t)th * EV_R * a.K * EV_A + k * EV_A + ar) * M + (SUM ? mi : 0);
}

// bits 30..61 of a sort key, ~score_key(score), back to the score (-0 was sorted, and comes back, as +0)
__device__ __forceinline__ double key_score(unsigned inv) {
  const unsigned key = ~inv;
  return (double)__uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// one tile of at most 64 records of a chunk: their match / ignore words (and with sk their score bits) into LDS
template <bool SUM>
__device__ __forceinline__ void acc_load_tile(const SastEvalArgs& a, int lo, int cnt, int base, int md, unsigned long long* sm, unsigned long long* si,
                                              unsigned* sk = nullptr) {
  const int lane = threadIdx.x;
  if (base + lane < cnt) {
    const unsigned long long key = a.sorted[lo + base + lane];
    const unsigned long long ro = min(key & EV_IDX_MASK, (unsigned long long)(a.max_detections - 1));
    unsigned long long ig = a.rec_ign[ro];
    if (SUM) {
      if ((int)((ig >> EV_RANK_SHIFT) & 127) >= md) ig = EV_LANE_MASK;   // not among its image's first md detections
      if (sk) sk[lane] = (unsigned)(key >> 30);
    }
    sm[lane] = a.rec_match[ro], si[lane] = ig;
  }
}

template <bool SUM>
__global__ void __launch_bounds__(64) eval_acc_count_kernel(SastEvalArgs a, int L, AccWs w, AccSum s) {
  __shared__ unsigned long long sm[64], si[64];
  const int lane = threadIdx.x;
  const int mi = SUM ? blockIdx.y : 0, md = SUM ? sum_maxdet(mi) : EV_MAXDET;
  const size_t row = ((SUM ? (size_t)mi * s.chunks : 0) + blockIdx.x) * 64 + lane;
  AccChunk p;
  if (!acc_chunk(a, blockIdx.x, L, p)) return;
  int tp = 0, fp = 0;
  for (int base = 0; base < p.cnt; base += 64) {
    acc_load_tile<SUM>(a, p.lo, p.cnt, base, md, sm, si);
    __syncthreads();
    const int cj = min(64, p.cnt - base);
    for (int j = 0; j < cj; ++j) {
      const int m = (int)((sm[j] >> lane) & 1), g = (int)((si[j] >> lane) & 1);
      tp += m & (g ^ 1), fp += (m ^ 1) & (g ^ 1);
    }
    __syncthreads();
  }
  w.tp[row] = tp, w.fp[row] = fp;
}

template <bool SUM>
__global__ void __launch_bounds__(64) eval_acc_scan_kernel(SastEvalArgs a, int L, AccWs w, AccSum s) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const int mi = SUM ? blockIdx.y : 0;
  const long long qb = SUM ? mi * s.chunks : 0;
  const int ar = lane / EV_T, th = lane - ar * EV_T;
  const bool active = lane < EV_LANES;
  const AccCat c = acc_category(a, k, L);
  int tp = 0, fp = 0;
  for (long long q = qb + c.q0; q < qb + c.q0 + c.nck; ++q) {   // any chunk count: sequential over the chunks, 64 lanes wide
    tp += w.tp[q * 64 + lane], fp += w.fp[q * 64 + lane];
    w.tp[q * 64 + lane] = tp, w.fp[q * 64 + lane] = fp;
  }
  if (!active) return;
  const int npig = a.state[ST_NPIG + k * EV_A + ar];
  if (SUM)   // COCOeval's recall: the true positives at the category's right edge over npig; 0 without a record, -1 without a label
    s.recall[(((size_t)th * a.K + k) * EV_A + ar) * EV_M + mi] = npig > 0 ? (c.n > 0 ? (double)tp / (double)npig : 0.0) : -1.0;
  if (npig > 0 && c.n > 0) return;                    // the chunks write the column
  size_t rs;
  const size_t o = acc_column<SUM>(a, th, k, ar, mi, rs);
  double* out = (SUM ? s.precision : a.precision) + o;
  const double v = npig > 0 ? 0.0 : -1.0;             // no detection: recall 0 reaches threshold 0 only, with precision 0
  for (int r = 0; r < EV_R; ++r) out[r * rs] = v;
  if (SUM)
    for (int r = 0; r < EV_R; ++r) s.scores[o + r * rs] = v;
}

template <bool SUM>
__global__ void __launch_bounds__(64) eval_acc_max_kernel(SastEvalArgs a, int L, AccWs w, AccSum s) {
  __shared__ unsigned long long sm[64], si[64];
  const int lane = threadIdx.x;
  const int mi = SUM ? blockIdx.y : 0, md = SUM ? sum_maxdet(mi) : EV_MAXDET;
  const size_t row = ((SUM ? (size_t)mi * s.chunks : 0) + blockIdx.x) * 64 + lane;
  AccChunk p;
  if (!acc_chunk(a, blockIdx.x, L, p)) return;
  int tp = 0, fp = 0;
  if (p.c > 0) tp = w.tp[row - 64], fp = w.fp[row - 64];
  double mx = 0.0;
  for (int base = 0; base < p.cnt; base += 64) {
    acc_load_tile<SUM>(a, p.lo, p.cnt, base, md, sm, si);
    __syncthreads();
    const int cj = min(64, p.cnt - base);
    for (int j = 0; j < cj; ++j) {
      const int m = (int)((sm[j] >> lane) & 1), g = (int)((si[j] >> lane) & 1);
      if (g) continue;
      tp += m, fp += m ^ 1;
      const double s = (double)fp + (double)tp;
      mx = fmax(mx, (double)tp / (s + 2.220446049250313e-16));
    }
    __syncthreads();
  }
  w.mx[row] = mx;
}

template <bool SUM>
__global__ void __launch_bounds__(64) eval_acc_envelope_kernel(SastEvalArgs a, int L, AccWs w, AccSum s) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const long long qb = SUM ? blockIdx.y * s.chunks : 0;
  const AccCat c = acc_category(a, k, L);
  double mx = 0.0;
  for (long long q = qb + c.q0 + c.nck - 1; q >= qb + c.q0; --q) {
    mx = fmax(mx, w.mx[q * 64 + lane]);
    w.mx[q * 64 + lane] = mx;
  }
}

// SUM also writes scores: beside every precision entry the score of the record at which the walk writes it -- the first record whose
// recall reaches the threshold (np.searchsorted, side='left').  Threshold 0 is reached at index 0 of the kept records whether or not
// that record is ignored; it is sorted[start] for every maxDet, since a category's top-scored record has rank 0 in its own group.
template <bool SUM>
__global__ void __launch_bounds__(64) eval_acc_walk_kernel(SastEvalArgs a, int L, AccWs w, AccSum s) {
  __shared__ unsigned long long sm[64], si[64];
  __shared__ unsigned sk[SUM ? 64 : 1];
  __shared__ double rthr[EV_R];
  const int lane = threadIdx.x;
  const int mi = SUM ? blockIdx.y : 0, md = SUM ? sum_maxdet(mi) : EV_MAXDET;
  AccChunk p;
  if (!acc_chunk(a, blockIdx.x, L, p)) return;
  const int ar = lane / EV_T, th = lane - ar * EV_T;
  const bool active = lane < EV_LANES;
  for (int r = lane; r < EV_R; r += 64) rthr[r] = a.rec_thr[r];
  const int npig = active ? a.state[ST_NPIG + p.k * EV_A + ar] : 0;
  const bool live = active && npig > 0;
  size_t rs;
  const size_t col = acc_column<SUM>(a, th, p.k, ar, mi, rs);
  double* out = (SUM ? s.precision : a.precision) + col;
  double* sc = SUM ? s.scores + col : nullptr;
  const size_t row = ((SUM ? (size_t)mi * s.chunks : 0) + blockIdx.x) * 64 + lane;
  const bool first = p.c == 0, last = p.c == p.nck - 1;
  int tp = w.tp[row], fp = w.fp[row];                                 // at the chunk's right edge
  const int tpl = first ? 0 : w.tp[row - 64];                         // at its left edge
  double mx = last ? 0.0 : w.mx[row + 64];                            // the envelope entering from the right
  __syncthreads();
  const double dn = (double)npig;
  int ihi = 0, ilo = 0;
  if (live) {
    const double rc = (double)tp / dn, rcl = (double)tpl / dn;
    while (ihi < EV_R && rthr[ihi] <= rc) ++ihi;
    while (ilo < EV_R && rthr[ilo] <= rcl) ++ilo;
    if (last)
      for (int r = ihi; r < EV_R; ++r) {                              // np.searchsorted past the end: the entry stays 0
        out[r * rs] = 0.0;
        if (SUM) sc[r * rs] = 0.0;
      }
    if (first) {
      const double all = w.mx[row];                                   // the maximum over the whole category
      const double top = SUM ? key_score((unsigned)(a.sorted[p.lo] >> 30)) : 0.0;   // p.lo is the category's start: cnt >= 1
      for (int r = 0; r < ilo; ++r) {                                 // recall threshold 0
        out[r * rs] = all;
        if (SUM) sc[r * rs] = top;
      }
    }
  }
  // backwards: the precision envelope (the running maximum from the right) at the first record whose recall reaches each threshold;
  // thresholds [ilo, ihi) are this chunk's, and the walk ends early once every lane has written its own
  for (int base = p.cnt > 0 ? ((p.cnt - 1) / 64) * 64 : -64; base >= 0; base -= 64) {
    if (__syncthreads_or(ihi > ilo) == 0) break;
    acc_load_tile<SUM>(a, p.lo, p.cnt, base, md, sm, si, SUM ? sk : nullptr);
    __syncthreads();
    if (live && ihi > ilo) {
      for (int j = min(64, p.cnt - base) - 1; j >= 0; --j) {
        const int m = (int)((sm[j] >> lane) & 1), g = (int)((si[j] >> lane) & 1);
        if (g) continue;   // an ignored detection repeats its left neighbour's recall and precision
        const double s = (double)fp + (double)tp;
        const double pr = (double)tp / (s + 2.220446049250313e-16);
        mx = fmax(mx, pr);
        tp -= m, fp -= m ^ 1;
        const double rcp = (double)tp / dn;
        while (ihi > 0 && rthr[ihi - 1] > rcp) {
          out[--ihi * rs] = mx;
          if (SUM) sc[ihi * rs] = key_score(sk[j]);                   // record j is where this recall is first reached
        }
      }
    }
  }
}

__global__ void __launch_bounds__(64) eval_summarize_kernel(SastEvalArgs a) {
  __shared__ double ssum[64];
  __shared__ int scnt[64];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int ar = s < 3 ? 0 : s - 2;
  const int t0 = s == 2 ? 5 : 0, nt = (s == 1 || s == 2) ? 1 : EV_T;
  const int per_t = EV_R * a.K;
  double sum = 0.0;
  int cnt = 0;
  for (int e = lane; e < nt * per_t; e += 64) {
    const int t = t0 + e / per_t, rk = e % per_t;
    const double v = a.precision[((size_t)t * per_t + rk) * EV_A + ar];
    if (v > -1.0) sum += v, ++cnt;
  }
  ssum[lane] = sum, scnt[lane] = cnt;
  __syncthreads();
  if (lane == 0) {
    for (int i = 1; i < 64; ++i) sum += ssum[i], cnt += scnt[i];
    a.result[s] = cnt > 0 ? sum / (double)cnt : -1.0;
  }
  if (s == 0 && lane < SAST_EVAL_STATE_WORDS) a.result[8 + lane] = (double)a.state[lane];   // one host copy brings both
}

// COCOeval.summarize and the per-category numbers: one workgroup per number, each the mean over the entries > -1 of a slice of the
// precision or the recall table (-1 when there is none).  Workgroups 0..11 are COCOeval.stats in its order; workgroup 12 + 4 k + j is
// category k's AP, AP_50, AP_75 (all areas, maxDets 100) and AR_100.  The summation order of the first six is eval_summarize_kernel's
// over the same values, so they are its six numbers bit for bit.
__global__ void __launch_bounds__(64) evsum_stats_kernel(SastEvalArgs a, AccSum s, double* stats, double* per_class) {
  __shared__ double ssum[64];
  __shared__ int scnt[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  bool rec;                                   // the recall table, not the precision table
  int ar = 0, t0 = 0, nt = EV_T, k0 = 0, nk = a.K, mi = EV_M - 1;
  if (b < 6) rec = false, ar = b < 3 ? 0 : b - 2, t0 = b == 2 ? 5 : 0, nt = (b == 1 || b == 2) ? 1 : EV_T;
  else if (b < 9) rec = true, mi = b - 6;     // AR_1, AR_10, AR_100 over all areas
  else if (b < 12) rec = true, ar = b - 8;    // AR_S, AR_M, AR_L at maxDets 100
  else {
    const int j = (b - 12) & 3;
    k0 = (b - 12) >> 2, nk = 1, rec = j == 3, t0 = j == 2 ? 5 : 0, nt = (j == 1 || j == 2) ? 1 : EV_T;
  }
  const int per_t = (rec ? 1 : EV_R) * nk;
  double sum = 0.0;
  int cnt = 0;
  for (int e = lane; e < nt * per_t; e += 64) {
    const int t = t0 + e / per_t, rr = e % per_t, r = rr / nk, k = k0 + rr % nk;
    const double v = rec ? s.recall[(((size_t)t * a.K + k) * EV_A + ar) * EV_M + mi]
                         : s.precision[((((size_t)t * EV_R + r) * a.K + k) * EV_A + ar) * EV_M + mi];
    if (v > -1.0) sum += v, ++cnt;
  }
  ssum[lane] = sum, scnt[lane] = cnt;
  __syncthreads();
  if (lane == 0) {
    for (int i = 1; i < 64; ++i) sum += ssum[i], cnt += scnt[i];
    const double v = cnt > 0 ? sum / (double)cnt : -1.0;
    if (b < SAST_EVSUM_STATS) stats[b] = v;
    else per_class[b - SAST_EVSUM_STATS] = v;
  }
}

// ---- sast_evmerge_append: the buffer `s` behind the buffer `d`.  Every count is read from the two states on the device and clamped
// to its buffer's capacity; every index is an offset (dst's count) plus a position below src's count, and `fits` bounds their sum by
// dst's capacity before anything is written.
struct MergeCounts {
  int ni_d, ng_d, nd_d, nr_d;   // dst: images, ground-truth rows, detection rows, records
  int ni_s, ng_s, nd_s, nr_s;   // src
  bool over_img, over_gt, over_det;
  __device__ bool fits() const { return !(over_img || over_gt || over_det); }
};

__device__ __forceinline__ int clamp_count(int v, long long cap) { return (int)min((long long)max(v, 0), cap); }

__device__ __forceinline__ MergeCounts merge_counts(const SastEvalArgs& d, const SastEvalArgs& s) {
  const long long gcap_d = (long long)d.max_images * d.max_labels_per_frame, gcap_s = (long long)s.max_images * s.max_labels_per_frame;
  MergeCounts m;
  m.ni_d = clamp_count(d.state[ST_IMAGES], d.max_images), m.ng_d = clamp_count(d.state[ST_GT], gcap_d);
  m.nd_d = clamp_count(d.state[ST_DET], d.max_detections), m.nr_d = clamp_count(d.state[ST_REC], d.max_detections);
  m.ni_s = clamp_count(s.state[ST_IMAGES], s.max_images), m.ng_s = clamp_count(s.state[ST_GT], gcap_s);
  m.nd_s = clamp_count(s.state[ST_DET], s.max_detections), m.nr_s = clamp_count(s.state[ST_REC], s.max_detections);
  m.over_img = (long long)m.ni_d + m.ni_s > d.max_images;
  m.over_gt = (long long)m.ng_d + m.ng_s > gcap_d;
  m.over_det = (long long)m.nd_d + m.nd_s > d.max_detections || (long long)m.nr_d + m.nr_s > d.max_detections;
  return m;
}

// Ordering across workgroups: the offsets of an append are dst's own counts, and the append ends by raising them.  The two halves are two
// launches on one stream.  evmerge_copy_kernel only READS the two states (every workgroup computes the same MergeCounts from them) and
// writes table and record slots at or past dst's counts, which no workgroup of the launch reads; evmerge_publish_kernel, one thread,
// runs after the copy kernel has ended (stream order, also inside a replayed graph) and is the only writer of a state word.  So no
// workgroup reads a state word that another workgroup of the same launch writes, and there is no ticket to take.  A refused append (it
// does not fit) is decided by both kernels from the same unchanged words: the first copies nothing, the second only counts the refusal.
__global__ void __launch_bounds__(256) evmerge_copy_kernel(SastEvalArgs d, SastEvalArgs s) {
  const MergeCounts m = merge_counts(d, s);
  if (!m.fits()) return;
  const int n = max(max(m.ni_s, m.ng_s), max(m.nd_s, m.nr_s));
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (i < m.ni_s) d.img_t[m.ni_d + i] = s.img_t[i];
    if (i < m.ng_s) {
      const size_t o = (size_t)(m.ng_d + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) d.gt_box[o * 4 + e] = s.gt_box[(size_t)i * 4 + e];
      d.gt_cls[o] = s.gt_cls[i];
      d.gt_img[o] = s.gt_img[i] + m.ni_d;
    }
    if (i < m.nd_s) {
      const size_t o = (size_t)(m.nd_d + i);
#pragma unroll
      for (int e = 0; e < 5; ++e) d.det_box[o * 5 + e] = s.det_box[(size_t)i * 5 + e];
      d.det_cls[o] = s.det_cls[i];
      d.det_img[o] = s.det_img[i] + m.ni_d;
    }
    if (i < m.nr_s) {
      const size_t o = (size_t)(m.nr_d + i);
      const unsigned long long key = s.rec_key[i];   // category and score bits stay; the index (the tie-break) moves behind dst's
      d.rec_key[o] = (key & ~EV_IDX_MASK) | (((key & EV_IDX_MASK) + (unsigned long long)m.nr_d) & EV_IDX_MASK);
      d.rec_match[o] = s.rec_match[i], d.rec_ign[o] = s.rec_ign[i];
    }
  }
}

__global__ void evmerge_publish_kernel(SastEvalArgs d, SastEvalArgs s) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const MergeCounts m = merge_counts(d, s);
  int* st = d.state;
  const int* ss = s.state;
  st[ST_ERR_IMAGES] += max(ss[ST_ERR_IMAGES], 0), st[ST_ERR_DETS] += max(ss[ST_ERR_DETS], 0), st[ST_ERR_LABELS] += max(ss[ST_ERR_LABELS], 0);
  st[ST_ADDS] += max(ss[ST_ADDS], 0);
  st[ST_ERR_WINDOW] += max(ss[ST_ERR_WINDOW], 0), st[ST_ERR_UNSORTED] += max(ss[ST_ERR_UNSORTED], 0);   // sast_evrec_add's refusals
  if (!m.fits()) {   // counted, reported by the host at evaluate time; nothing was appended
    const int lost = max(m.ni_s, 1);
    if (m.over_img) st[ST_ERR_IMAGES] += lost;
    if (m.over_gt) st[ST_ERR_LABELS] += lost;
    if (m.over_det) st[ST_ERR_DETS] += lost;
    return;
  }
  st[ST_IMAGES] = m.ni_d + m.ni_s, st[ST_GT] = m.ng_d + m.ng_s, st[ST_DET] = m.nd_d + m.nd_s, st[ST_REC] = m.nr_d + m.nr_s;
  for (int k = 0; k < SAST_EVAL_MAX_CLASSES; ++k) st[ST_REC_CAT + k] += max(ss[ST_REC_CAT + k], 0);
  for (int e = 0; e < SAST_EVAL_MAX_CLASSES * EV_A; ++e) st[ST_NPIG + e] += max(ss[ST_NPIG + e], 0);
}

bool evmerge_tables_ok(const SastEvalArgs* a) {
  return a->gt_box && a->gt_cls && a->gt_img && a->img_t && a->det_box && a->det_cls && a->det_img &&
         (long long)a->max_images * a->max_labels_per_frame <= 0x7fffffffll;
}

int eval_acc_chunk() { return std::max(SAST_KNOB("SAST_EVAL_ACC_CHUNK", 1024), 1); }

size_t eval_acc_ws_bytes(long long max_detections, int L) { return (size_t)acc_max_chunks(max_detections, L) * ACC_WS_PER_CHUNK; }

bool eval_args_ok(const SastEvalArgs* a) {
  return a && a->state && a->rec_key && a->rec_match && a->rec_ign && a->K >= 1 && a->K <= SAST_EVAL_MAX_CLASSES && a->max_images >= 1 &&
         a->max_detections >= 1 && (unsigned long long)a->max_detections <= EV_IDX_MASK && a->max_labels_per_frame >= 1 &&
         a->max_labels_per_frame <= EV_MAX_LABELS;
}

// to_prophesee's detection half (io/box_loading.py:81-97) for the rows of one online step, one wave per row: lane j writes records
// j, j + 64, ... of the row.  A record is five 8-byte words: t | x, y | w, h | class_id, track_id = 0 | class_confidence, 0.
// w and h are one fp32 subtraction each, as numpy's (this file is built with -ffp-contract=off).  n_det is data: it is clamped to the A
// rows the detections hold before any of them is read, and no row at or past it is read at all.
__global__ __launch_bounds__(64) void detections_export_kernel(SastDetExportArgs a) {
  const int s = blockIdx.x;
  const int n = min(max(a.n_det[s], 0), a.A);
  const int m = a.due[s] ? min(n, a.max_det) : 0;
  const unsigned long long t = (unsigned long long)a.ends[s];
  const float* __restrict__ det = a.det + (size_t)s * a.A * 7;
  unsigned long long* __restrict__ rec = reinterpret_cast<unsigned long long*>(a.records + (size_t)s * a.max_det * SAST_DET_RECORD_BYTES);
  for (int i = threadIdx.x; i < m; i += 64) {
    const float* r = det + (size_t)i * 7;
    const float x1 = r[0], y1 = r[1], w = r[2] - x1, h = r[3] - y1;
    unsigned long long* o = rec + (size_t)i * (SAST_DET_RECORD_BYTES / 8);
    o[0] = t;
    o[1] = (unsigned long long)__float_as_uint(x1) | ((unsigned long long)__float_as_uint(y1) << 32);
    o[2] = (unsigned long long)__float_as_uint(w) | ((unsigned long long)__float_as_uint(h) << 32);
    o[3] = (unsigned long long)(unsigned)r[6];
    o[4] = (unsigned long long)__float_as_uint(r[5]);
  }
  if (threadIdx.x == 0) {
    a.counts[s] = m;
    if (a.due[s] && n > m) atomicAdd(a.truncated, n - m);
  }
}

// One workgroup per row: the m = counts[s] records of one step go behind the row's log, or nowhere when they do not fit.  Every
// thread reads the log's count before the barrier, thread 0 raises it behind it.  Records move as five 8-byte words.
__global__ __launch_bounds__(64) void detlog_append_kernel(SastDetLogArgs a) {
  const int s = blockIdx.x;
  const int m = min(max(a.counts[s], 0), a.max_det);
  const long long n = min(max((long long)a.log_counts[s], 0ll), (long long)a.capacity);
  if (m == 0) return;
  if (n + m > a.capacity) {   // the step is dropped whole, and counted
    if (threadIdx.x == 0) atomicAdd(a.dropped, 1);
    return;
  }
  const unsigned long long* __restrict__ src = reinterpret_cast<const unsigned long long*>(a.records + (size_t)s * a.max_det * SAST_DET_RECORD_BYTES);
  unsigned long long* __restrict__ dst = reinterpret_cast<unsigned long long*>(a.log) + ((size_t)s * a.capacity + n) * (SAST_DET_RECORD_BYTES / 8);
  for (int i = threadIdx.x; i < m * (SAST_DET_RECORD_BYTES / 8); i += 64) dst[i] = src[i];
  __syncthreads();
  if (threadIdx.x == 0) a.log_counts[s] = n + m;
}

// the dynamic LDS a match instantiation may ask for (grown monotonically; racing callers set the same attribute)
template <class Src>
bool match_lds_allow(size_t lds) {
  static size_t allowed = 0;
  if (lds > allowed) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(eval_match_kernel<Src>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return false;
    allowed = lds;
  }
  return true;
}

constexpr long long EVREC_MAX_SLOTS = 0x7fffffffll / EV_INFO;   // S * Gcap: an info index stays an int

struct EvRecWs {
  int* info;       // [S * Gcap][16]
  int* starts;     // [S * Gcap]
  int* nimg;       // [S]
  int* unsorted;   // [S]
};

size_t evrec_ws_carve(void* ws, long long S, long long Gcap, EvRecWs* w) {
  int* p = (int*)ws;
  if (w) w->info = p, w->starts = p + S * Gcap * EV_INFO, w->nimg = p + S * Gcap * (EV_INFO + 1), w->unsorted = p + S * Gcap * (EV_INFO + 1) + S;
  return sizeof(int) * (size_t)(S * Gcap * (EV_INFO + 1) + 2 * S);
}

}  // namespace
}  // namespace sast

extern "C" {

int sast_eval_reset(const SastEvalArgs* a, sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!eval_args_ok(a)) return SAST_EINVAL;
  const long long n = std::max<long long>(a->max_detections, SAST_EVAL_STATE_WORDS);
  SAST_LAUNCH(eval_reset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_eval_add(const SastEvalArgs* a, sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!eval_args_ok(a) || !a->labels || !a->counts || !a->det || !a->n_det || !a->info || !a->gt_box || !a->gt_cls || !a->gt_img ||
      !a->img_t || !a->det_box || !a->det_cls || !a->det_img || !a->iou_thr || a->N < 1 || a->N > 65535 || a->M < 1 || a->A < 1 ||
      a->A > EV_MAX_ANCHORS)
    return SAST_EINVAL;
  int P = 64;
  while (P < a->A) P <<= 1;
  const size_t lds = match_lds_carve(nullptr, P, a->max_labels_per_frame, nullptr);
  if (!match_lds_allow<FrameRows>(lds)) return SAST_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const FrameRows::Args rows{};
  SAST_LAUNCH(eval_count_kernel<FrameRows>, dim3((unsigned)a->N), dim3(64), 0, st, *a, rows);
  SAST_LAUNCH(eval_scan_kernel, dim3(1), dim3(64), 0, st, *a);
  SAST_LAUNCH(eval_match_kernel<FrameRows>, dim3((unsigned)a->N, (unsigned)a->K), dim3(64), lds, st, *a, rows, P);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

size_t sast_evrec_ws_bytes(int S, int Gcap) {
  if (S < 1 || S > 65535 || Gcap < 1 || (long long)S * Gcap > sast::EVREC_MAX_SLOTS) return 0;
  return sast::evrec_ws_carve(nullptr, S, Gcap, nullptr);
}

int sast_evrec_add(const SastEvalArgs* buf, const SastEvRecArgs* rec, sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!eval_args_ok(buf) || !evmerge_tables_ok(buf) || !buf->iou_thr || !rec || !rec->gt || !rec->n_gt || !rec->dt || !rec->n_dt || !rec->ws)
    return SAST_EINVAL;
  if (rec->S < 1 || rec->S > 65535 || rec->Gcap < 1 || rec->Dcap < 1 || (long long)rec->S * rec->Gcap > EVREC_MAX_SLOTS ||
      (long long)rec->S * rec->Dcap > 0x7fffffffll || rec->max_window < 1 || rec->max_window > EV_MAX_WINDOW || rec->time_tol_us < 0 ||
      rec->ws_bytes < evrec_ws_carve(nullptr, rec->S, rec->Gcap, nullptr) || ((reinterpret_cast<uintptr_t>(rec->gt) | reinterpret_cast<uintptr_t>(rec->dt)) & 7) ||
      (reinterpret_cast<uintptr_t>(rec->ws) & 3))
    return SAST_EINVAL;
  EvRecWs w;
  evrec_ws_carve(rec->ws, rec->S, rec->Gcap, &w);
  SastEvalArgs a = *buf;   // the buffer, with this call's scratch as the per-image info; the frame fields are not read
  a.info = w.info;
  a.N = rec->S * rec->Gcap;
  const RecordRows::Args rows{rec->gt, (const long long*)rec->n_gt, rec->dt, (const long long*)rec->n_dt, w.starts, w.nimg, w.unsorted,
                              rec->S, rec->Gcap, rec->Dcap, rec->max_window, (long long)rec->time_tol_us};
  int P = 64;
  while (P < rec->max_window) P <<= 1;
  const size_t lds = match_lds_carve(nullptr, P, a.max_labels_per_frame, nullptr);
  if (!match_lds_allow<RecordRows>(lds)) return SAST_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  SAST_LAUNCH(evrec_images_kernel, dim3((unsigned)rec->S), dim3(1024), 0, st, a, rows);
  SAST_LAUNCH(eval_count_kernel<RecordRows>, dim3((unsigned)a.N), dim3(64), 0, st, a, rows);
  SAST_LAUNCH(evrec_scan_kernel, dim3(1), dim3(64), 0, st, a, rows);
  SAST_LAUNCH(eval_match_kernel<RecordRows>, dim3((unsigned)a.N, (unsigned)a.K), dim3(64), lds, st, a, rows, P);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_detlog_append(const SastDetLogArgs* a, sast_stream_t stream) {
  SAST_ENTRY();
  if (!a || !a->records || !a->counts || !a->log || !a->log_counts || !a->dropped || a->S < 1 || a->S > 65535 || a->max_det < 1 ||
      a->capacity < 1 || ((reinterpret_cast<uintptr_t>(a->records) | reinterpret_cast<uintptr_t>(a->log)) & 7))
    return SAST_EINVAL;
  SAST_LAUNCH(sast::detlog_append_kernel, dim3((unsigned)a->S), dim3(64), 0, (hipStream_t)stream, *a);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

size_t sast_eval_sort_ws_bytes(int64_t max_detections) {
  if (max_detections < 1 || (unsigned long long)max_detections > sast::EV_IDX_MASK) return 0;
  size_t bytes = 0;
  unsigned long long* p = nullptr;
  if (rocprim::radix_sort_keys(nullptr, bytes, p, p, (size_t)max_detections, 0, 64, (hipStream_t) nullptr) != hipSuccess) return 0;
  // the accumulate's per-chunk partials take the workspace over once the sort is done
  return std::max<size_t>(std::max<size_t>(bytes, 16), sast::eval_acc_ws_bytes(max_detections, sast::eval_acc_chunk()));
}

int sast_eval_accumulate(const SastEvalArgs* a, sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!eval_args_ok(a) || !a->sorted || !a->sort_ws || !a->rec_thr || !a->precision || !a->result) return SAST_EINVAL;
  const int L = eval_acc_chunk();
  const long long chunks = acc_max_chunks(a->max_detections, L);
  if (a->sort_ws_bytes < eval_acc_ws_bytes(a->max_detections, L) || chunks > 0x7fffffffll) return SAST_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  size_t bytes = a->sort_ws_bytes;
  // the keys are unique (category, ~score, record index), so the sorted order is the stable descending-score order per category;
  // slots past the cursor hold the all-ones key the reset wrote and sort behind every record
  if (rocprim::radix_sort_keys(a->sort_ws, bytes, (const unsigned long long*)a->rec_key, (unsigned long long*)a->sorted, (size_t)a->max_detections,
                               0, 64, st) != hipSuccess)
    return SAST_ELAUNCH;
  const AccWs w = acc_ws_carve(a->sort_ws, chunks);
  const dim3 per_chunk((unsigned)chunks), per_cat((unsigned)a->K);   // sized from the capacity: the counts stay on the device
  const AccSum none{nullptr, nullptr, nullptr, 0};
  SAST_LAUNCH(eval_acc_count_kernel<false>, per_chunk, dim3(64), 0, st, *a, L, w, none);
  SAST_LAUNCH(eval_acc_scan_kernel<false>, per_cat, dim3(64), 0, st, *a, L, w, none);
  SAST_LAUNCH(eval_acc_max_kernel<false>, per_chunk, dim3(64), 0, st, *a, L, w, none);
  SAST_LAUNCH(eval_acc_envelope_kernel<false>, per_cat, dim3(64), 0, st, *a, L, w, none);
  SAST_LAUNCH(eval_acc_walk_kernel<false>, per_chunk, dim3(64), 0, st, *a, L, w, none);
  SAST_LAUNCH(eval_summarize_kernel, dim3(6), dim3(64), 0, st, *a);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

size_t sast_evsum_ws_bytes(int64_t max_detections) {
  if (max_detections < 1 || (unsigned long long)max_detections > sast::EV_IDX_MASK) return 0;
  return sast::EV_M * sast::eval_acc_ws_bytes(max_detections, sast::eval_acc_chunk());
}

int sast_evsum_accumulate(const SastEvalArgs* a, const SastEvSumArgs* sum, sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!eval_args_ok(a) || !a->sorted || !a->rec_thr || !sum || !sum->precision || !sum->scores || !sum->recall || !sum->stats ||
      !sum->per_class || !sum->ws || (reinterpret_cast<uintptr_t>(sum->ws) & 7))
    return SAST_EINVAL;
  const int L = eval_acc_chunk();
  const long long chunks = acc_max_chunks(a->max_detections, L);
  if (sum->ws_bytes < EV_M * eval_acc_ws_bytes(a->max_detections, L) || chunks > 0x7fffffffll) return SAST_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const AccWs w = acc_ws_carve(sum->ws, EV_M * chunks);
  const AccSum s{sum->precision, sum->scores, sum->recall, chunks};
  const dim3 per_chunk((unsigned)chunks, EV_M), per_cat((unsigned)a->K, EV_M);   // sized from the capacity: the counts stay on the device
  SAST_LAUNCH(eval_acc_count_kernel<true>, per_chunk, dim3(64), 0, st, *a, L, w, s);
  SAST_LAUNCH(eval_acc_scan_kernel<true>, per_cat, dim3(64), 0, st, *a, L, w, s);
  SAST_LAUNCH(eval_acc_max_kernel<true>, per_chunk, dim3(64), 0, st, *a, L, w, s);
  SAST_LAUNCH(eval_acc_envelope_kernel<true>, per_cat, dim3(64), 0, st, *a, L, w, s);
  SAST_LAUNCH(eval_acc_walk_kernel<true>, per_chunk, dim3(64), 0, st, *a, L, w, s);
  SAST_LAUNCH(evsum_stats_kernel, dim3((unsigned)(SAST_EVSUM_STATS + 4 * a->K)), dim3(64), 0, st, *a, s, sum->stats, sum->per_class);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_evmerge_append(const SastEvalArgs* dst, const SastEvalArgs* src, sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!eval_args_ok(dst) || !eval_args_ok(src) || !evmerge_tables_ok(dst) || !evmerge_tables_ok(src)) return SAST_EINVAL;
  if (dst == src || dst->state == src->state) return SAST_EINVAL;
  if (dst->K != src->K || dst->min_diag2 != src->min_diag2 || dst->min_side != src->min_side ||
      src->max_labels_per_frame > dst->max_labels_per_frame)
    return SAST_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const long long most = std::max<long long>(std::max<long long>(src->max_detections, src->max_images),
                                             (long long)src->max_images * src->max_labels_per_frame);
  const unsigned blocks = (unsigned)std::min<long long>((most + 255) / 256, 4096);   // sized from src's capacities; the kernel strides
  SAST_LAUNCH(evmerge_copy_kernel, dim3(blocks), dim3(256), 0, st, *dst, *src);
  SAST_LAUNCH(evmerge_publish_kernel, dim3(1), dim3(64), 0, st, *dst, *src);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_detections_export(const SastDetExportArgs* a, sast_stream_t stream) {
  SAST_ENTRY();
  if (!a || !a->det || !a->n_det || !a->ends || !a->due || !a->records || !a->counts || !a->truncated || a->S < 1 || a->S > 65535 ||
      a->A < 1 || a->max_det < 1 || (reinterpret_cast<uintptr_t>(a->records) & 7))
    return SAST_EINVAL;
  SAST_LAUNCH(sast::detections_export_kernel, dim3((unsigned)a->S), dim3(64), 0, (hipStream_t)stream, *a);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
