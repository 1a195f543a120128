// CLEAR-MOT tracking metrics of tracked detections against labelled tracks, on the device (include/sast_hip.h, "tracking metrics").
// The rule is this project's statement of Bernardin and Stiefelhagen's protocol; tests/tracking_eval_model.py is its sequential form.
//   sast_trackeval_add    S whole recordings as sorted 40-byte box records, labels and tracked detections: two launches
//                           frames      one workgroup of 256 threads per recording: the sorted check, then label timestamp after label
//                                       timestamp -- the frame's labels and the hypotheses of the nearest detection run into LDS, the
//                                       track table looked up, carry-over, the optimal assignment of the rest, the counts.  Writes
//                                       the recording's rows of the call.
//                           accumulate  one workgroup: the rows of the call into the accumulator, in row order
//   sast_trackeval_reset  clears the accumulator (one launch)
// The frames of a recording are sequential (a labelled track remembers its last hypothesis), so the parallelism is inside a frame:
//   - filter, duplicate check and ordered compaction of a run of records: all 256 threads, 256 records a turn
//   - the track table: one thread per label probes an open-addressing table in global memory (64-bit entries id << 32 | slot + 1,
//     inserted with one compare-and-swap; the ids of a frame are distinct, so no two threads insert the same id)
//   - carry-over: one thread per label, the claims on a hypothesis settled by an LDS atomicMin of the label index
//   - the assignment: shortest augmenting paths (Jonker-Volgenant / Hungarian) with fp64 potentials on ONE wave, the smaller side as
//     rows, two columns per lane held in registers (box, class, v, minv, way, used); a step computes the row's reduced costs, the
//     column minimum is a wave reduction (six xor shuffles of the fp64 minimum, then a ballot for the lowest column at it).  The fp32
//     IoU is recomputed (about twenty instructions against eighteen cross-lane moves per step), so LDS holds no cost matrix.
//     Invalid pairs cost TE_INVALID = 1e3 > 128 valid costs: the most valid pairs first, then the least cost sum.
//   - counts: one thread per label and per hypothesis, 64-bit LDS atomics; the fp64 IoU sums are per-thread registers over the whole
//     recording, reduced once at the end through a fixed tree: one order, the same bits every run.
// This file is built with -ffp-contract=off: the IoU is one fp32 rounding per operation, as the model's.
#include "box_rules.cuh"
#include "common.cuh"
#include "kernels.h"

#include <climits>

namespace sast {
namespace {

constexpr int TE_THREADS = 256;
constexpr int TE_WAVES = TE_THREADS / 64;
constexpr int TE_MAX = SAST_TRACKEVAL_MAX_FRAME;     // 128 labels / hypotheses in a frame
constexpr int TE_NC = SAST_TRACKEVAL_COLS;
constexpr int TE_ND = SAST_TRACKEVAL_DIAG;
constexpr int TE_K = SAST_EVAL_MAX_CLASSES;
constexpr int TE_REC_WORDS = SAST_DET_RECORD_BYTES / 4;
constexpr double TE_INVALID = 1e3, TE_INF = 1e300;
static_assert(TE_MAX == 2 * 64, "the solver holds two columns per lane");
static_assert(TE_MAX <= TE_THREADS / 2, "labels are counted by the lower half of the workgroup, hypotheses by the upper");
static_assert((TE_K + 1) * TE_NC <= TE_THREADS && TE_ND <= TE_THREADS, "one thread per word of a row");

__device__ __forceinline__ long long te_time(const int* row, long long i) { return *reinterpret_cast<const long long*>(row + i * TE_REC_WORDS); }

// first index in [lo, hi) of a sorted row whose t is >= v (strict: > v)
__device__ __forceinline__ int te_bound(const int* row, int lo, int hi, long long v, bool strict) {
  while (lo < hi) {
    const int m = lo + ((hi - lo) >> 1);
    const long long t = te_time(row, m);
    if (strict ? t <= v : t < v) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// what the lanes of ONE wave wrote to LDS is read by its other lanes behind this
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {   // a fixed tree: the same order every run
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

struct Side {   // one side of a frame
  float4 box[TE_MAX];
  unsigned cls[TE_MAX];
  unsigned id[TE_MAX];
  int match[TE_MAX];   // index on the other side, -1: none
};

struct TeLds {
  Side g, h;                        // labels, hypotheses
  int slot[TE_MAX];                 // label -> slot of the track table
  int claim[TE_MAX];                // hypothesis -> lowest label that keeps it by carry-over
  unsigned tile_id[TE_THREADS];     // one turn of `collect`
  unsigned char tile_ok[TE_THREADS];
  int wcount[TE_WAVES];
  short ridx[TE_MAX], cidx[TE_MAX]; // the labels / hypotheses the carry-over left, ascending
  double u[TE_MAX];                 // the solver's row potentials
  int p[TE_MAX], way[TE_MAX];       // column -> row (-1: free); column -> the column before it on the path (-1: the start)
  unsigned long long cnt[TE_K][TE_NC];
  double wsum[TE_WAVES][TE_K];
  int diag[TE_ND];
  int ntracks, over;
};

struct TeTable {   // the labelled tracks of one recording (global memory, the caller's workspace)
  unsigned long long* hash;   // [H] id << 32 | slot + 1; 0: empty
  int* cls;                   // [M] each
  unsigned* last;
  int* present;
  int* matched;
  int* prev;
  unsigned H;
};

__host__ __device__ inline unsigned te_hash_size(int max_gt_tracks) {
  unsigned h = 64;
  while (h < 2u * (unsigned)max_gt_tracks) h <<= 1;
  return h;
}
__host__ __device__ inline size_t te_row_bytes(int max_gt_tracks) {
  const size_t M = ((size_t)max_gt_tracks + 1) & ~(size_t)1;
  return 8 * (size_t)te_hash_size(max_gt_tracks) + 20 * M;
}
__device__ inline TeTable te_table(const SastTrackEvalArgs& a, int s) {
  unsigned char* base = static_cast<unsigned char*>(a.ws) + (size_t)s * te_row_bytes(a.max_gt_tracks);
  const size_t M = ((size_t)a.max_gt_tracks + 1) & ~(size_t)1;
  TeTable t;
  t.H = te_hash_size(a.max_gt_tracks);
  t.hash = reinterpret_cast<unsigned long long*>(base);
  t.cls = reinterpret_cast<int*>(base + 8 * (size_t)t.H);
  t.last = reinterpret_cast<unsigned*>(t.cls + M);
  t.present = reinterpret_cast<int*>(t.last + M);
  t.matched = t.present + M;
  t.prev = t.matched + M;
  return t;
}

__device__ __forceinline__ bool te_valid(const SastTrackEvalArgs& a, const float4 gb, unsigned gc, const float4 hb, unsigned hc, float& iou) {
  iou = track_iou(gb, hb);
  return (a.class_agnostic || gc == hc) && iou >= a.iou_thre;
}

// The records [lo, hi) of a sorted row that pass the filter (step 2) and are not a second record of their track_id (step 3), in record
// order into `sd`, at most `cap` of them; returns how many there are (more than cap: the frame is overfull, sd holds the first cap).
// Every thread of the workgroup calls it with the same arguments; it ends with a barrier.
template <bool HYP>
__device__ int te_collect(const SastTrackEvalArgs& a, TeLds& l, Side& sd, const int* row, int lo, int hi, int cap) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = 0;
  for (int base = lo; base < hi; base += TE_THREADS) {
    const int i = base + tid;                              // hi - base > 0 and base + 255 <= INT_MAX: hi <= 2^31 - 1 - 256 is checked on the host
    bool ok = false;
    unsigned id = 0, cls = 0;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < hi) {
      const int* r = row + (size_t)i * TE_REC_WORDS;
      b = make_float4(__int_as_float(r[2]), __int_as_float(r[3]), __int_as_float(r[4]), __int_as_float(r[5]));
      cls = (unsigned)r[6], id = (unsigned)r[7];
      ok = te_time(row, i) > EV_SKIP_US && box_passes(b.z, b.w, a.min_diag2, a.min_side);
      if (ok && HYP && id == 0u) ok = false, atomicAdd(&l.diag[SAST_TE_UNTRACKED], 1);
      if (ok && cls >= (unsigned)a.K) ok = false, atomicAdd(&l.diag[SAST_TE_BAD_CLASS], 1);
    }
    l.tile_id[tid] = id, l.tile_ok[tid] = ok;
    __syncthreads();
    if (ok) {
      bool dup = false;
      const int seen = min(n, cap);
      for (int q = 0; q < seen && !dup; ++q) dup = sd.id[q] == id;
      for (int q = 0; q < tid && !dup; ++q) dup = l.tile_ok[q] && l.tile_id[q] == id;
      if (dup) ok = false, atomicAdd(&l.diag[HYP ? SAST_TE_DUP_HYP : SAST_TE_DUP_GT], 1);
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) l.wcount[wave] = __popcll(m);
    __syncthreads();
    int before = 0, tile = 0;
    for (int w = 0; w < TE_WAVES; ++w) {
      before += w < wave ? l.wcount[w] : 0;
      tile += l.wcount[w];
    }
    if (ok) {
      const int p = n + before + __popcll(m & ((1ull << lane) - 1ull));
      if (p < cap) sd.box[p] = b, sd.cls[p] = cls, sd.id[p] = id, sd.match[p] = -1;
    }
    n += tile;
    __syncthreads();
    if (n > cap) break;                                    // the same in every thread
  }
  return n;
}

// The optimal assignment of the nr labels l.ridx and the nc hypotheses l.cidx (step 5, second part), on the calling wave alone.
__device__ void te_solve(const SastTrackEvalArgs& a, TeLds& l, int nr, int nc) {
  const int lane = threadIdx.x & 63;
  const bool rows_are_labels = nr <= nc;
  const int na = rows_are_labels ? nr : nc, nb = rows_are_labels ? nc : nr;
  const Side& A = rows_are_labels ? l.g : l.h;
  const Side& B = rows_are_labels ? l.h : l.g;
  const short* ai = rows_are_labels ? l.ridx : l.cidx;
  const short* bi = rows_are_labels ? l.cidx : l.ridx;
  float4 bb[2];
  unsigned bc[2];
  double v[2] = {0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int j = lane + 64 * q;
    bb[q] = make_float4(0.f, 0.f, 0.f, 0.f), bc[q] = 0u;
    if (j < nb) bb[q] = B.box[bi[j]], bc[q] = B.cls[bi[j]], l.p[j] = -1, l.way[j] = -1;
  }
  for (int i = lane; i < na; i += 64) l.u[i] = 0.0;
  wave_sync();
  for (int i = 0; i < na; ++i) {                           // row i joins the matching along its shortest augmenting path
    double minv[2] = {TE_INF, TE_INF};
    int way[2] = {-1, -1};
    bool used[2] = {false, false};
    int i0 = i, j0 = -1, last = -1;
    for (int it = 0; it < nb; ++it) {                      // a step marks one more column: at most nb of them
      const float4 ab = A.box[ai[i0]];
      const unsigned ac = A.cls[ai[i0]];
      const double ui0 = l.u[i0];
      double best = TE_INF;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (lane + 64 * q < nb && !used[q]) {
          float iou;
          const bool ok = rows_are_labels ? te_valid(a, ab, ac, bb[q], bc[q], iou) : te_valid(a, bb[q], bc[q], ab, ac, iou);
          const double cur = (ok ? 1.0 - (double)iou : TE_INVALID) - ui0 - v[q];
          if (cur < minv[q]) minv[q] = cur, way[q] = j0;
          best = minv[q] < best ? minv[q] : best;
        }
      }
      const double delta = wave_min_f64(best);
      const unsigned long long m0 = __ballot(lane < nb && !used[0] && minv[0] == delta);
      const unsigned long long m1 = __ballot(lane + 64 < nb && !used[1] && minv[1] == delta);
      if ((m0 | m1) == 0ull) break;                        // a NaN potential: cannot happen with finite costs; the row stays unmatched
      const int j1 = m0 ? __ffsll((long long)m0) - 1 : 64 + __ffsll((long long)m1) - 1;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = lane + 64 * q;
        if (j < nb) {
          if (used[q]) l.u[l.p[j]] += delta, v[q] -= delta;   // the rows of the marked columns are distinct, and none is row i
          else minv[q] -= delta;
        }
      }
      if (lane == 0) l.u[i] += delta;
      if ((j1 & 63) == lane) {
        if (j1 < 64) l.way[j1] = way[0], used[0] = true;
        else l.way[j1] = way[1], used[1] = true;
      }
      wave_sync();
      j0 = j1;
      const int r = l.p[j1];
      if (r < 0) {
        last = j1;
        break;
      }
      i0 = r;
    }
    if (lane == 0 && last >= 0) {                          // the path backwards: every column takes the row of the column before it
      int j = last;
      for (int g = 0; j >= 0 && g <= nb; ++g) {
        const int jp = l.way[j];
        l.p[j] = jp < 0 ? i : l.p[jp];
        j = jp;
      }
    }
    wave_sync();
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int j = lane + 64 * q;
    const int r = j < nb ? l.p[j] : -1;
    if (r < 0) continue;
    const int o = rows_are_labels ? ai[r] : bi[j], hj = rows_are_labels ? bi[j] : ai[r];
    float iou;
    if (te_valid(a, l.g.box[o], l.g.cls[o], l.h.box[hj], l.h.cls[hj], iou)) l.g.match[o] = hj, l.h.match[hj] = o;
  }
}

__global__ __launch_bounds__(TE_THREADS) void trackeval_frames_kernel(SastTrackEvalArgs a) {
  __shared__ TeLds l;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, M = a.max_gt_tracks;
  const TeTable tb = te_table(a, s);
  const int ng = (int)min(max((long long)a.n_gt[s], 0ll), (long long)a.Gcap), nd = (int)min(max((long long)a.n_dt[s], 0ll), (long long)a.Dcap);
  const int* grow = a.gt + (size_t)s * a.Gcap * TE_REC_WORDS;
  const int* drow = a.dt + (size_t)s * a.Dcap * TE_REC_WORDS;
  for (int i = tid; i < TE_K * TE_NC; i += TE_THREADS) (&l.cnt[0][0])[i] = 0ull;
  if (tid < TE_ND) l.diag[tid] = 0;
  if (tid == 0) l.ntracks = 0, l.over = 0;
  for (unsigned i = tid; i < tb.H; i += TE_THREADS) tb.hash[i] = 0ull;
  __threadfence();                                         // the cleared table is at the L2 before any compare-and-swap on it
  int bad = 0;
  for (int i = tid + 1; i < ng; i += TE_THREADS) bad |= te_time(grow, i) < te_time(grow, i - 1);
  for (int i = tid + 1; i < nd; i += TE_THREADS) bad |= te_time(drow, i) < te_time(drow, i - 1);
  bad = __syncthreads_or(bad);
  int refused = bad ? SAST_TE_UNSORTED : -1;               // the diag word of the reason; the same in every thread
  double sum[TE_K] = {0.0, 0.0, 0.0, 0.0};
  static_assert(TE_K == 4, "sum is written out for four classes");
  unsigned long long frames = 0ull;

  int gpos = 0;
  while (refused < 0 && gpos < ng) {
    const long long t = te_time(grow, gpos);
    const int gend = te_bound(grow, gpos + 1, ng, t, true);
    const int nl = te_collect<false>(a, l, l.g, grow, gpos, gend, a.max_labels_per_frame);
    gpos = gend;
    if (nl == 0) continue;                                 // no label of this t is left: no frame
    if (nl > a.max_labels_per_frame) {
      refused = SAST_TE_REFUSED_LABELS;
      break;
    }
    // ---- the detection run nearest t, the earlier one on a tie, inside the tolerance
    int nh = 0;
    {
      const int i = te_bound(drow, 0, nd, t, false);
      const bool lo_ok = i > 0, hi_ok = i < nd;
      const long long tlo = lo_ok ? te_time(drow, i - 1) : 0, thi = hi_ok ? te_time(drow, i) : 0;
      const unsigned long long dlo = (unsigned long long)t - (unsigned long long)tlo, dhi = (unsigned long long)thi - (unsigned long long)t;
      const unsigned long long tol = (unsigned long long)a.time_tol_us;
      bool has = false;
      long long ts = 0;
      if (lo_ok && (!hi_ok || dlo <= dhi)) has = dlo <= tol, ts = tlo;
      else if (hi_ok) has = dhi <= tol, ts = thi;
      if (has) {
        const int r0 = te_bound(drow, 0, nd, ts, false), r1 = te_bound(drow, r0, nd, ts, true);
        nh = te_collect<true>(a, l, l.h, drow, r0, r1, a.max_hyp_per_frame);
      }
    }
    if (nh > a.max_hyp_per_frame) {
      refused = SAST_TE_REFUSED_HYP;
      break;
    }
    // ---- the labels' tracks: looked up, or entered with the class of this, their first, record
    if (tid < nl) {
      const unsigned id = l.g.id[tid];
      unsigned at = (id * 2654435761u) & (tb.H - 1u);
      int slot = -1, fresh = -1;
      for (unsigned probe = 0; probe < tb.H; ++probe) {
        unsigned long long e = __hip_atomic_load(tb.hash + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (e == 0ull) {
          if (fresh < 0) fresh = atomicAdd(&l.ntracks, 1);
          if (fresh >= M) {                                // one id more than the table holds: nothing is written
            l.over = 1;
            break;
          }
          e = atomicCAS(tb.hash + at, 0ull, ((unsigned long long)id << 32) | (unsigned long long)(unsigned)(fresh + 1));
          if (e == 0ull) {
            slot = fresh;
            tb.cls[slot] = (int)l.g.cls[tid], tb.last[slot] = 0u, tb.present[slot] = 0, tb.matched[slot] = 0, tb.prev[slot] = 0;
            break;
          }
        }
        if ((unsigned)(e >> 32) == id) {                   // (an entry another label of this frame took holds another id)
          slot = (int)(unsigned)e - 1;
          break;
        }
        at = (at + 1u) & (tb.H - 1u);
      }
      if (slot < 0) l.over = 1;                            // (also a probe that found neither the id nor room: the row is refused)
      l.slot[tid] = slot;
    }
    if (tid < nh) l.claim[tid] = INT_MAX;
    __syncthreads();
    if (l.over) {
      refused = SAST_TE_REFUSED_TRACKS;
      break;
    }
    // ---- carry-over: a track keeps its last hypothesis when that is here, valid, and no earlier label keeps it
    int mine = -1;
    if (tid < nl) {
      const unsigned h = tb.last[l.slot[tid]];
      if (h != 0u)
        for (int j = 0; j < nh; ++j)
          if (l.h.id[j] == h) {
            float iou;
            if (te_valid(a, l.g.box[tid], l.g.cls[tid], l.h.box[j], l.h.cls[j], iou)) atomicMin(&l.claim[j], tid), mine = j;
            break;
          }
    }
    __syncthreads();
    if (mine >= 0 && l.claim[mine] == tid) l.g.match[tid] = mine, l.h.match[mine] = tid;
    __syncthreads();
    // ---- the optimal assignment of what is left
    if (wave == 0) {
      int nr = 0, nc = 0;
#pragma unroll
      for (int base = 0; base < TE_MAX; base += 64) {
        const int i = base + lane;
        const bool gfree = i < nl && l.g.match[i] < 0, hfree = i < nh && l.h.match[i] < 0;
        const unsigned long long mg = __ballot(gfree), mh = __ballot(hfree), lt = (1ull << lane) - 1ull;
        if (gfree) l.ridx[nr + __popcll(mg & lt)] = (short)i;
        if (hfree) l.cidx[nc + __popcll(mh & lt)] = (short)i;
        nr += __popcll(mg), nc += __popcll(mh);
      }
      wave_sync();
      if (nr > 0 && nc > 0) te_solve(a, l, nr, nc);
    }
    __syncthreads();
    // ---- counts (step 6): a thread per label, a thread per hypothesis
    if (tid < nl) {
      const int slot = l.slot[tid], k = (int)l.g.cls[tid], j = l.g.match[tid];
      unsigned long long* c = l.cnt[k];
      atomicAdd(c + SAST_TE_GT, 1ull);
      tb.present[slot] += 1;
      if (j >= 0) {
        const float iou = track_iou(l.g.box[tid], l.h.box[j]);
        const unsigned h = l.h.id[j], before = tb.last[slot];
        atomicAdd(c + SAST_TE_MATCHES, 1ull);
#pragma unroll
        for (int kk = 0; kk < TE_K; ++kk)
          if (kk == k) sum[kk] += (double)iou;
        if (before != 0u && before != h) atomicAdd(c + SAST_TE_IDSW, 1ull);
        if (tb.matched[slot] > 0 && !tb.prev[slot]) atomicAdd(c + SAST_TE_FRAG, 1ull);
        tb.last[slot] = h, tb.matched[slot] += 1, tb.prev[slot] = 1;
      } else {
        atomicAdd(c + SAST_TE_FN, 1ull);
        tb.prev[slot] = 0;
      }
    } else if (tid >= TE_MAX && tid - TE_MAX < nh) {
      const int j = tid - TE_MAX;
      unsigned long long* c = l.cnt[l.h.cls[j]];
      atomicAdd(c + SAST_TE_HYP, 1ull);
      if (l.h.match[j] < 0) atomicAdd(c + SAST_TE_FP, 1ull);
    }
    frames += 1ull;
    __syncthreads();                                       // the next frame overwrites the sides
  }
  __syncthreads();

  // ---- the tracks of the recording (step 7), the IoU sums, and the rows of the call
  if (refused < 0) {
    const int nt = min(l.ntracks, M);
    for (int i = tid; i < nt; i += TE_THREADS) {
      unsigned long long* c = l.cnt[tb.cls[i]];
      const long long pr = tb.present[i], ma = tb.matched[i];
      atomicAdd(c + SAST_TE_GT_TRACKS, 1ull);
      atomicAdd(c + (5 * ma >= 4 * pr ? SAST_TE_MT : 5 * ma < pr ? SAST_TE_ML : SAST_TE_PT), 1ull);
    }
  }
#pragma unroll
  for (int kk = 0; kk < TE_K; ++kk) {
    const double w = wave_sum_f64(sum[kk]);
    if (lane == 0) l.wsum[wave][kk] = w;
  }
  __syncthreads();
  int64_t* rows = a.rows + (size_t)s * (K + 1) * TE_NC;
  if (tid < (K + 1) * TE_NC) {
    const int k = tid / TE_NC, c = tid - k * TE_NC;
    unsigned long long v = 0ull;
    if (c == SAST_TE_FRAMES) v = frames;                   // the frames of the recording, in every row
    else if (k < K) v = l.cnt[k][c];
    else
      for (int kk = 0; kk < K; ++kk) v += l.cnt[kk][c];
    rows[tid] = refused < 0 ? (long long)v : 0ll;
  }
  if (tid == 0) {
    double all = 0.0;
    for (int kk = 0; kk < K; ++kk) {
      double v = 0.0;
      for (int w = 0; w < TE_WAVES; ++w) v += l.wsum[w][kk];
      if (refused >= 0) v = 0.0;
      a.rows_iou[(size_t)s * (K + 1) + kk] = v;
      all += v;
    }
    a.rows_iou[(size_t)s * (K + 1) + K] = all;
  }
  if (tid < TE_ND) a.rows_diag[(size_t)s * TE_ND + tid] = refused < 0 ? (long long)l.diag[tid] : (tid == refused ? 1ll : 0ll);
}

// the rows of a call into the accumulator, row after row: the fp64 sums have one order
__global__ __launch_bounds__(TE_THREADS) void trackeval_accumulate_kernel(SastTrackEvalArgs a) {
  const int tid = threadIdx.x, ni = (a.K + 1) * TE_NC, nf = a.K + 1;
  if (tid < ni) {
    long long v = a.acc[tid];
    for (int s = 0; s < a.S; ++s) v += a.rows[(size_t)s * ni + tid];
    a.acc[tid] = v;
  } else if (tid < ni + nf) {
    const int k = tid - ni;
    double v = a.acc_iou[k];
    for (int s = 0; s < a.S; ++s) v += a.rows_iou[(size_t)s * nf + k];
    a.acc_iou[k] = v;
  } else if (tid < ni + nf + TE_ND) {
    const int d = tid - ni - nf;
    long long v = a.acc_diag[d];
    for (int s = 0; s < a.S; ++s) v += a.rows_diag[(size_t)s * TE_ND + d];
    a.acc_diag[d] = v;
  }
}
static_assert((TE_K + 1) * TE_NC + TE_K + 1 + TE_ND <= TE_THREADS, "one thread per word of the accumulator");

__global__ __launch_bounds__(TE_THREADS) void trackeval_reset_kernel(SastTrackEvalArgs a) {
  const int tid = threadIdx.x, ni = (a.K + 1) * TE_NC, nf = a.K + 1;
  if (tid < ni) a.acc[tid] = 0ll;
  else if (tid < ni + nf) a.acc_iou[tid - ni] = 0.0;
  else if (tid < ni + nf + TE_ND) a.acc_diag[tid - ni - nf] = 0ll;
}

bool trackeval_acc_ok(const SastTrackEvalArgs* a) {
  return a && a->acc && a->acc_iou && a->acc_diag && a->K >= 1 && a->K <= TE_K && !(reinterpret_cast<uintptr_t>(a->acc) & 7) &&
         !(reinterpret_cast<uintptr_t>(a->acc_iou) & 7) && !(reinterpret_cast<uintptr_t>(a->acc_diag) & 7);
}

}  // namespace
}  // namespace sast

extern "C" {

size_t sast_trackeval_ws_bytes(int S, int max_gt_tracks) {
  if (S < 1 || S > 65535 || max_gt_tracks < 1 || max_gt_tracks > SAST_TRACKEVAL_MAX_GT_TRACKS) return 0;
  return (size_t)S * sast::te_row_bytes(max_gt_tracks);
}

int sast_trackeval_add(const SastTrackEvalArgs* a, sast_stream_t stream) {
  SAST_ENTRY();
  const long long most = 0x7fffffffll - sast::TE_THREADS;   // a turn of 256 records past the last one still has an int index
  if (!sast::trackeval_acc_ok(a) || !a->gt || !a->n_gt || !a->dt || !a->n_dt || !a->rows || !a->rows_iou || !a->rows_diag || !a->ws ||
      a->S < 1 || a->S > 65535 || a->Gcap < 1 || a->Dcap < 1 || (long long)a->S * a->Gcap > most || (long long)a->S * a->Dcap > most ||
      a->max_gt_tracks < 1 || a->max_gt_tracks > SAST_TRACKEVAL_MAX_GT_TRACKS || a->max_labels_per_frame < 1 ||
      a->max_labels_per_frame > SAST_TRACKEVAL_MAX_FRAME || a->max_hyp_per_frame < 1 || a->max_hyp_per_frame > SAST_TRACKEVAL_MAX_FRAME ||
      !(a->iou_thre > 0.f && a->iou_thre <= 1.f) || a->time_tol_us < 0 || a->ws_bytes < sast_trackeval_ws_bytes(a->S, a->max_gt_tracks))
    return SAST_EINVAL;
  for (const void* p : {(const void*)a->gt, (const void*)a->dt, (const void*)a->n_gt, (const void*)a->n_dt, (const void*)a->rows,
                        (const void*)a->rows_iou, (const void*)a->rows_diag, (const void*)a->ws})
    if (reinterpret_cast<uintptr_t>(p) & 7) return SAST_EINVAL;
  SAST_LAUNCH(sast::trackeval_frames_kernel, dim3((unsigned)a->S), dim3(sast::TE_THREADS), 0, (hipStream_t)stream, *a);
  SAST_LAUNCH(sast::trackeval_accumulate_kernel, dim3(1), dim3(sast::TE_THREADS), 0, (hipStream_t)stream, *a);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_trackeval_reset(const SastTrackEvalArgs* a, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::trackeval_acc_ok(a)) return SAST_EINVAL;
  SAST_LAUNCH(sast::trackeval_reset_kernel, dim3(1), dim3(sast::TE_THREADS), 0, (hipStream_t)stream, *a);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
