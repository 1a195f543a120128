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
//                                   ignore bits.
//   sast_eval_accumulate  one device-wide radix sort (rocprim) of the record keys (category, descending score, record index: unique, so
//                         the order is the stable one), the chunk-parallel walk of every category's sorted records (counts, scan over
//                         the chunks, precision maxima, envelope, backward walk: the 101 recall thresholds), and the six summaries.
//   sast_evmerge_append   one buffer behind another (two launches, no host synchronisation): what joins the buffers of several ranks
// Every fp32 / fp64 operation of the reference is repeated one rounding at a time: build.py compiles this file with -ffp-contract=off.
#include "common.cuh"
#include "kernels.h"

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

namespace sast {
namespace {

constexpr int EV_T = SAST_EVAL_IOU_THRS;      // 10
constexpr int EV_R = SAST_EVAL_REC_THRS;      // 101
constexpr int EV_A = SAST_EVAL_AREAS;         // 4
constexpr int EV_LANES = EV_T * EV_A;         // 40: lane = area * 10 + threshold
constexpr int EV_MAXDET = 100;
constexpr int EV_INFO = 16;                   // int32 words of per-frame scratch
constexpr long long EV_SKIP_US = 500000;
constexpr unsigned long long EV_IDX_MASK = (1ull << 30) - 1;
constexpr int EV_MAX_ANCHORS = 8192, EV_MAX_LABELS = 128;

// state words
enum { ST_IMAGES = 0, ST_GT = 1, ST_DET = 2, ST_REC = 3, ST_REC_CAT = 4, ST_ERR_IMAGES = 8, ST_ERR_DETS = 9, ST_ERR_LABELS = 10, ST_ADDS = 11, ST_NPIG = 12 };
// info words of a frame
enum { IN_VALID = 0, IN_NGT = 1, IN_NDT = 2, IN_NREC = 3, IN_IMG = 8, IN_GT_OFF = 9, IN_DET_OFF = 10, IN_REC_OFF = 11 };

__device__ __forceinline__ bool box_passes(float w, float h, float diag2, float side) {
  const float d = w * w + h * h;   // fp32, one rounding each (box_filtering.py:34)
  return d >= diag2 && w >= side && h >= side;
}

__device__ __forceinline__ unsigned class_of(float v) { return (unsigned)(long long)v; }

__device__ __forceinline__ bool label_passes(const float* r, float diag2, float side) {
  return (long long)r[0] > EV_SKIP_US && box_passes(r[3], r[4], diag2, side);
}

__device__ __forceinline__ bool det_passes(const float* r, float diag2, float side) { return box_passes(r[2] - r[0], r[3] - r[1], diag2, side); }

// ascending on the result = ascending on the float (-0 == +0)
__device__ __forceinline__ unsigned score_key(float s) {
  if (s == 0.f) s = 0.f;
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int frame_labels(const SastEvalArgs& a, int n) { return min(max(a.counts[n], 0), a.M); }
__device__ __forceinline__ int frame_dets(const SastEvalArgs& a, int n) { return min(max(a.n_det[n], 0), a.A); }

__global__ void __launch_bounds__(64) eval_count_kernel(SastEvalArgs a) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int cnt = frame_labels(a, n);
  const float* lab = a.labels + (size_t)n * a.M * 7;
  const float* det = a.det + (size_t)n * a.A * 7;
  int ngt = 0, ndt = 0, c[SAST_EVAL_MAX_CLASSES] = {0, 0, 0, 0};
  for (int base = 0; base < cnt; base += 64) {
    const int i = base + lane;
    ngt += __popcll(__ballot(i < cnt && label_passes(lab + i * 7, a.min_diag2, a.min_side)));
  }
  if (ngt > 0 && (long long)lab[0] > EV_SKIP_US) {   // the detections carry the frame's one timestamp (box_loading.py:90)
    const int nd = frame_dets(a, n);
    for (int base = 0; base < nd; base += 64) {
      const int i = base + lane;
      const bool keep = i < nd && det_passes(det + (size_t)i * 7, a.min_diag2, a.min_side);
      const unsigned cls = keep ? class_of(det[(size_t)i * 7 + 6]) : 0u;
      ndt += __popcll(__ballot(keep));
#pragma unroll
      for (int k = 0; k < SAST_EVAL_MAX_CLASSES; ++k) c[k] += __popcll(__ballot(keep && cls == (unsigned)k));
    }
  }
  if (lane == 0) {
    int* info = a.info + n * EV_INFO;
    info[IN_VALID] = ngt > 0;
    info[IN_NGT] = ngt;
    info[IN_NDT] = ndt;
#pragma unroll
    for (int k = 0; k < SAST_EVAL_MAX_CLASSES; ++k) info[IN_NREC + k] = k < a.K ? min(c[k], EV_MAXDET) : 0;
  }
}

__global__ void eval_scan_kernel(SastEvalArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int* st = a.state;
  int img = st[ST_IMAGES], gt = st[ST_GT], dt = st[ST_DET], rec = st[ST_REC];
  for (int n = 0; n < a.N; ++n) {
    int* info = a.info + n * EV_INFO;
    if (!info[IN_VALID]) continue;
    int nrec = 0;
    for (int k = 0; k < a.K; ++k) nrec += info[IN_NREC + k];
    int* err = nullptr;
    if (info[IN_NGT] > a.max_labels_per_frame) err = st + ST_ERR_LABELS;
    else if (img >= a.max_images) err = st + ST_ERR_IMAGES;
    else if ((long long)dt + info[IN_NDT] > a.max_detections) err = st + ST_ERR_DETS;
    if (err) {   // counted, reported by the host at evaluate time; the frame writes nothing
      *err += 1;
      info[IN_VALID] = 0;
      continue;
    }
    info[IN_IMG] = img, info[IN_GT_OFF] = gt, info[IN_DET_OFF] = dt, info[IN_REC_OFF] = rec;
    img += 1, gt += info[IN_NGT], dt += info[IN_NDT], rec += nrec;
    for (int k = 0; k < a.K; ++k) st[ST_REC_CAT + k] += info[IN_NREC + k];
  }
  st[ST_IMAGES] = img, st[ST_GT] = gt, st[ST_DET] = dt, st[ST_REC] = rec;
  st[ST_ADDS] += 1;   // a replayed graph adds without the host's knowledge: "has data" is decided from this word
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

__global__ void __launch_bounds__(64) eval_match_kernel(SastEvalArgs a, int P) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int n = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
  const int* info = a.info + n * EV_INFO;
  if (!info[IN_VALID]) return;
  const int G = a.max_labels_per_frame;
  MatchLds l;
  match_lds_carve(lds_raw, P, G, &l);
  const unsigned long long lt = (1ull << lane) - 1;
  const int cnt = frame_labels(a, n), nd_all = info[IN_NDT] > 0 ? frame_dets(a, n) : 0;
  const float* lab = a.labels + (size_t)n * a.M * 7;
  const float* det = a.det + (size_t)n * a.A * 7;
  const int img = info[IN_IMG];

  // ---- the flattened tables, in frame order (category 0's wave)
  if (k == 0) {
    int go = info[IN_GT_OFF], dofs = info[IN_DET_OFF];
    for (int base = 0; base < cnt; base += 64) {
      const int i = base + lane;
      const float* r = lab + i * 7;
      const bool keep = i < cnt && label_passes(r, a.min_diag2, a.min_side);
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int p = go + __popcll(m & lt);
        a.gt_box[(size_t)p * 4 + 0] = r[1], a.gt_box[(size_t)p * 4 + 1] = r[2], a.gt_box[(size_t)p * 4 + 2] = r[3], a.gt_box[(size_t)p * 4 + 3] = r[4];
        a.gt_cls[p] = (int)class_of(r[5]);
        a.gt_img[p] = img;
      }
      go += __popcll(m);
    }
    for (int base = 0; base < nd_all; base += 64) {
      const int i = base + lane;
      const float* r = det + (size_t)i * 7;
      const bool keep = i < nd_all && det_passes(r, a.min_diag2, a.min_side);
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const int p = dofs + __popcll(m & lt);
        float* o = a.det_box + (size_t)p * 5;
        o[0] = r[0], o[1] = r[1], o[2] = r[2] - r[0], o[3] = r[3] - r[1], o[4] = r[5];
        a.det_cls[p] = (int)class_of(r[6]);
        a.det_img[p] = img;
      }
      dofs += __popcll(m);
    }
    if (lane == 0) a.img_t[img] = (long long)lab[0];
  }

  // ---- ground truth of category k, in label order
  int ng = 0;
  for (int base = 0; base < cnt; base += 64) {
    const int i = base + lane;
    const float* r = lab + i * 7;
    const bool keep = i < cnt && label_passes(r, a.min_diag2, a.min_side) && class_of(r[5]) == (unsigned)k;
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int p = ng + __popcll(m & lt);   // < G: the scan refused frames with more boxes than that
      l.gbox[p * 4 + 0] = r[1], l.gbox[p * 4 + 1] = r[2], l.gbox[p * 4 + 2] = r[3], l.gbox[p * 4 + 3] = r[4];
      l.garea[p] = (double)(r[3] * r[4]);    // the fp32 product, widened (coco_eval.py:167, :172)
    }
    ng += __popcll(m);
  }
  // ---- detections of category k: keys (descending score, ascending index), sorted
  int c = 0;
  for (int base = 0; base < nd_all; base += 64) {
    const int i = base + lane;
    const float* r = det + (size_t)i * 7;
    const bool keep = i < nd_all && det_passes(r, a.min_diag2, a.min_side) && class_of(r[6]) == (unsigned)k;
    const unsigned long long m = __ballot(keep);
    if (keep) l.keys[c + __popcll(m & lt)] = ((unsigned long long)(~score_key(r[5])) << 32) | (unsigned)i;
    c += __popcll(m);
  }
  int P2 = 1;
  while (P2 < c) P2 <<= 1;   // <= P: c <= A
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
    const float* r = det + (size_t)l.dsel[d] * 7;
    const float w = r[2] - r[0], h = r[3] - r[1];
    l.dbox[d * 4 + 0] = r[0], l.dbox[d * 4 + 1] = r[1], l.dbox[d * 4 + 2] = w, l.dbox[d * 4 + 3] = h;
    l.darea[d] = (double)(w * h);
    l.dscore[d] = r[5];
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
      a.rec_match[ro] = mb, a.rec_ign[ro] = ib;
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

// one tile of at most 64 records of a chunk: their match / ignore words into LDS
__device__ __forceinline__ void acc_load_tile(const SastEvalArgs& a, int lo, int cnt, int base, unsigned long long* sm, unsigned long long* si) {
  const int lane = threadIdx.x;
  if (base + lane < cnt) {
    const unsigned long long ro = min(a.sorted[lo + base + lane] & EV_IDX_MASK, (unsigned long long)(a.max_detections - 1));
    sm[lane] = a.rec_match[ro], si[lane] = a.rec_ign[ro];
  }
}

__global__ void __launch_bounds__(64) eval_acc_count_kernel(SastEvalArgs a, int L, AccWs w) {
  __shared__ unsigned long long sm[64], si[64];
  const int lane = threadIdx.x;
  AccChunk p;
  if (!acc_chunk(a, blockIdx.x, L, p)) return;
  int tp = 0, fp = 0;
  for (int base = 0; base < p.cnt; base += 64) {
    acc_load_tile(a, p.lo, p.cnt, base, sm, si);
    __syncthreads();
    const int cj = min(64, p.cnt - base);
    for (int j = 0; j < cj; ++j) {
      const int m = (int)((sm[j] >> lane) & 1), g = (int)((si[j] >> lane) & 1);
      tp += m & (g ^ 1), fp += (m ^ 1) & (g ^ 1);
    }
    __syncthreads();
  }
  w.tp[(size_t)blockIdx.x * 64 + lane] = tp, w.fp[(size_t)blockIdx.x * 64 + lane] = fp;
}

__global__ void __launch_bounds__(64) eval_acc_scan_kernel(SastEvalArgs a, int L, AccWs w) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const int ar = lane / EV_T, th = lane - ar * EV_T;
  const bool active = lane < EV_LANES;
  const AccCat c = acc_category(a, k, L);
  int tp = 0, fp = 0;
  for (long long q = c.q0; q < c.q0 + c.nck; ++q) {   // any chunk count: sequential over the chunks, 64 lanes wide
    tp += w.tp[q * 64 + lane], fp += w.fp[q * 64 + lane];
    w.tp[q * 64 + lane] = tp, w.fp[q * 64 + lane] = fp;
  }
  if (!active) return;
  const int npig = a.state[ST_NPIG + k * EV_A + ar];
  if (npig > 0 && c.n > 0) return;                    // the chunks write the column
  double* out = a.precision + (size_t)th * EV_R * a.K * EV_A + k * EV_A + ar;   // [T][R][K][A]
  const size_t rs = (size_t)a.K * EV_A;
  const double v = npig > 0 ? 0.0 : -1.0;             // no detection: recall 0 reaches threshold 0 only, with precision 0
  for (int r = 0; r < EV_R; ++r) out[r * rs] = v;
}

__global__ void __launch_bounds__(64) eval_acc_max_kernel(SastEvalArgs a, int L, AccWs w) {
  __shared__ unsigned long long sm[64], si[64];
  const int lane = threadIdx.x;
  AccChunk p;
  if (!acc_chunk(a, blockIdx.x, L, p)) return;
  int tp = 0, fp = 0;
  if (p.c > 0) tp = w.tp[((size_t)blockIdx.x - 1) * 64 + lane], fp = w.fp[((size_t)blockIdx.x - 1) * 64 + lane];
  double mx = 0.0;
  for (int base = 0; base < p.cnt; base += 64) {
    acc_load_tile(a, p.lo, p.cnt, base, sm, si);
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
  w.mx[(size_t)blockIdx.x * 64 + lane] = mx;
}

__global__ void __launch_bounds__(64) eval_acc_envelope_kernel(SastEvalArgs a, int L, AccWs w) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const AccCat c = acc_category(a, k, L);
  double mx = 0.0;
  for (long long q = c.q0 + c.nck - 1; q >= c.q0; --q) {
    mx = fmax(mx, w.mx[q * 64 + lane]);
    w.mx[q * 64 + lane] = mx;
  }
}

__global__ void __launch_bounds__(64) eval_acc_walk_kernel(SastEvalArgs a, int L, AccWs w) {
  __shared__ unsigned long long sm[64], si[64];
  __shared__ double rthr[EV_R];
  const int lane = threadIdx.x;
  AccChunk p;
  if (!acc_chunk(a, blockIdx.x, L, p)) return;
  const int ar = lane / EV_T, th = lane - ar * EV_T;
  const bool active = lane < EV_LANES;
  for (int r = lane; r < EV_R; r += 64) rthr[r] = a.rec_thr[r];
  const int npig = active ? a.state[ST_NPIG + p.k * EV_A + ar] : 0;
  const bool live = active && npig > 0;
  double* out = a.precision + (size_t)th * EV_R * a.K * EV_A + p.k * EV_A + ar;   // [T][R][K][A]
  const size_t rs = (size_t)a.K * EV_A;
  const size_t row = (size_t)blockIdx.x * 64 + lane;
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
      for (int r = ihi; r < EV_R; ++r) out[r * rs] = 0.0;             // np.searchsorted past the end: the entry stays 0
    if (first) {
      const double all = w.mx[row];                                   // the maximum over the whole category
      for (int r = 0; r < ilo; ++r) out[r * rs] = all;                // recall threshold 0
    }
  }
  // backwards: the precision envelope (the running maximum from the right) at the first record whose recall reaches each threshold;
  // thresholds [ilo, ihi) are this chunk's, and the walk ends early once every lane has written its own
  for (int base = p.cnt > 0 ? ((p.cnt - 1) / 64) * 64 : -64; base >= 0; base -= 64) {
    if (__syncthreads_or(ihi > ilo) == 0) break;
    acc_load_tile(a, p.lo, p.cnt, base, sm, si);
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
        while (ihi > 0 && rthr[ihi - 1] > rcp) out[--ihi * rs] = mx;
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
  static size_t lds_allowed = 0;   // (grown monotonically; racing callers set the same attribute)
  if (lds > lds_allowed) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(eval_match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return SAST_EINVAL;
    lds_allowed = lds;
  }
  const hipStream_t st = (hipStream_t)stream;
  SAST_LAUNCH(eval_count_kernel, dim3((unsigned)a->N), dim3(64), 0, st, *a);
  SAST_LAUNCH(eval_scan_kernel, dim3(1), dim3(64), 0, st, *a);
  SAST_LAUNCH(eval_match_kernel, dim3((unsigned)a->N, (unsigned)a->K), dim3(64), lds, st, *a, P);
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
  SAST_LAUNCH(eval_acc_count_kernel, per_chunk, dim3(64), 0, st, *a, L, w);
  SAST_LAUNCH(eval_acc_scan_kernel, per_cat, dim3(64), 0, st, *a, L, w);
  SAST_LAUNCH(eval_acc_max_kernel, per_chunk, dim3(64), 0, st, *a, L, w);
  SAST_LAUNCH(eval_acc_envelope_kernel, per_cat, dim3(64), 0, st, *a, L, w);
  SAST_LAUNCH(eval_acc_walk_kernel, per_chunk, dim3(64), 0, st, *a, L, w);
  SAST_LAUNCH(eval_summarize_kernel, dim3(6), dim3(64), 0, st, *a);
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
