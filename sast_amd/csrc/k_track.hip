// Track ids for the exported detections: a greedy IoU tracker without a motion model (include/sast_hip.h, "track ids").  The
// reference has no tracker; the rule is this project's own and tests/tracker_model.py is its sequential statement.
//   sast_tracker_step   one online step: row s of [S, max_det, 40] records, predicated by due, following reset (one launch)
//   sast_tracker_run    whole sorted recordings [S, Dcap, 10]: every maximal run of equal t is one step (one launch)
// Both drivers are one workgroup of 256 threads per stream around ONE device body, track_rows' step(): the step driver calls it once, the
// recording driver once per run.  The table lives in global memory between calls; a step reads it into LDS, decides there, and writes
// back only what the rule changes.
// The matching is not min(T, m) dependent argmax rounds.  The order (IoU descending, detection ascending, slot ascending) is strict,
// so the pair at the head of the remaining list is the best remaining candidate of its slot AND of its detection, and taking every
// such mutually-best pair at once removes no candidate the sequential greedy would have taken later: rounds of "every slot and every
// detection pick their best, pairs that chose each other are fixed" end in the same matching.  IoU at or above a positive threshold
// orders like its bit pattern, so "best" is the maximum of the 64-bit key  IoU bits << 32 | ~detection << 8 | ~slot.
// IoUs are recomputed each round (15 flops) rather than kept: LDS holds 32 bytes per detection and 40 per slot, whatever T * m is.
// This file is built with -ffp-contract=off: the IoU is one fp32 rounding per operation, as the model's.
#include "box_rules.cuh"
#include "common.cuh"
#include "kernels.h"

#include <climits>

namespace sast {
namespace {

constexpr int TRK_THREADS = 256;
constexpr int TRK_WAVES = TRK_THREADS / 64;
static_assert(SAST_TRACK_MAX_TRACKS <= TRK_THREADS, "a thread looks after at most one slot");
constexpr int TRK_WORDS = SAST_DET_RECORD_BYTES / 8;   // a record is five 8-byte words; word 3 is class_id | track_id << 32

// track_iou (NaN when either box has a NaN, so such a box never passes the threshold) is box_rules.cuh's: the tracking evaluator
// judges a pair by the same number

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  return v;
}

struct SlotLds {   // 40 bytes per slot
  float4 box[SAST_TRACK_MAX_TRACKS];
  unsigned long long best[SAST_TRACK_MAX_TRACKS];
  int cls[SAST_TRACK_MAX_TRACKS];
  int id[SAST_TRACK_MAX_TRACKS];      // 0: free
  int open[SAST_TRACK_MAX_TRACKS];    // live and not matched in this step
  int free_list[SAST_TRACK_MAX_TRACKS];
};

// the table of one row and the rule on it
struct TrackRow {
  int* ids;
  float4* box;
  int* cls;
  long long* last_t;
  int* hits;
  int* next_id;
  int* counters;
  int T, max_det, agnostic;
  float iou_thre, score_thre;
  long long max_age;
  // LDS: the slots (static) and the detections (dynamic, 32 bytes each: best, box, cls, slot)
  SlotLds* sl;
  unsigned long long* d_best;
  float4* d_box;
  unsigned* d_cls;
  int* d_slot;

  __device__ TrackRow(const SastTrackerArgs& a, int s, SlotLds* slots, unsigned char* dyn) {
    const size_t o = (size_t)s * a.max_tracks;
    ids = a.ids + o, box = reinterpret_cast<float4*>(a.box) + o, cls = a.cls + o, last_t = reinterpret_cast<long long*>(a.last_t) + o;
    hits = a.hits + o, next_id = a.next_id + s, counters = a.counters;
    T = a.max_tracks, max_det = a.max_det, agnostic = a.class_agnostic, iou_thre = a.iou_thre, score_thre = a.new_score_thre;
    max_age = a.max_age_us;
    const size_t M = ((size_t)a.max_det + 1) & ~(size_t)1;   // even: the float4 part stays 16-byte aligned
    sl = slots;
    d_best = reinterpret_cast<unsigned long long*>(dyn);
    d_box = reinterpret_cast<float4*>(dyn + 8 * M);
    d_cls = reinterpret_cast<unsigned*>(dyn + 24 * M);
    d_slot = reinterpret_cast<int*>(dyn + 28 * M);
  }

  __device__ void free_slot(int i) const {
    ids[i] = 0, box[i] = make_float4(0.f, 0.f, 0.f, 0.f), cls[i] = 0, last_t[i] = 0, hits[i] = 0;
  }

  // step 1: every slot freed, ids start over.  Ends with a barrier.
  __device__ void reset() const {
    for (int i = threadIdx.x; i < T; i += TRK_THREADS) free_slot(i);
    if (threadIdx.x == 0) *next_id = 1;
    __syncthreads();
  }

  // steps 3 .. 7 on the m <= max_det records at rec (five words each) at time t.  Every thread of the workgroup calls it with the same
  // arguments; it ends with a barrier behind its last write.
  __device__ void step(unsigned long long* rec, int m, long long t) const {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int mine = 0;                                              // this thread's slot is live (a thread has at most one slot)
    for (int i = tid; i < T; i += TRK_THREADS) {              // expire, and the table into LDS
      int id = ids[i];
      if (id != 0) {
        const long long last = last_t[i];
        if (t > last && (unsigned long long)t - (unsigned long long)last > (unsigned long long)max_age) free_slot(i), id = 0;
      }
      sl->id[i] = id, sl->open[i] = id != 0, mine = id != 0;
      sl->box[i] = id != 0 ? box[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      sl->cls[i] = id != 0 ? cls[i] : 0;
    }
    for (int j = tid; j < m; j += TRK_THREADS) {
      const unsigned long long* r = rec + (size_t)j * TRK_WORDS;
      const unsigned long long xy = r[1], wh = r[2];
      d_box[j] = make_float4(__uint_as_float((unsigned)xy), __uint_as_float((unsigned)(xy >> 32)), __uint_as_float((unsigned)wh),
                             __uint_as_float((unsigned)(wh >> 32)));
      d_cls[j] = (unsigned)r[3];
      d_slot[j] = -1;
    }
    int open_slots = __syncthreads_count(mine), open_dets = m;    // the same in every thread: a round is run while both are left
    for (int round = 0; open_slots > 0 && open_dets > 0 && round <= T; ++round) {   // a round with a candidate left fixes at least one pair
      for (int i = tid; i < T; i += TRK_THREADS) sl->best[i] = 0ull;
      for (int j = tid; j < m; j += TRK_THREADS) d_best[j] = 0ull;
      __syncthreads();
      for (int i = wave; i < T; i += TRK_WAVES) {              // one wave per open slot, its lanes over the detections
        if (!sl->open[i]) continue;
        const float4 a = sl->box[i];
        const unsigned c = (unsigned)sl->cls[i];
        unsigned long long best = 0ull;
        for (int j = lane; j < m; j += 64) {
          if (d_slot[j] >= 0 || !(agnostic || d_cls[j] == c)) continue;
          const float iou = track_iou(a, d_box[j]);
          if (!(iou >= iou_thre)) continue;
          const unsigned long long key = ((unsigned long long)__float_as_uint(iou) << 32) | ((unsigned long long)(0xffffffu - (unsigned)j) << 8) |
                                         (unsigned long long)(0xffu - (unsigned)i);
          best = key > best ? key : best;
          atomicMax(&d_best[j], key);
        }
        best = wave_max_u64(best);
        if (lane == 0) sl->best[i] = best;
      }
      __syncthreads();
      int made = 0;
      for (int i = tid; i < T; i += TRK_THREADS) {
        const unsigned long long key = sl->best[i];
        if (key == 0ull) continue;
        const int j = (int)(0xffffffu - (unsigned)((key >> 8) & 0xffffffu));
        if (d_best[j] != key) continue;                        // the detection prefers another slot
        const float4 b = d_box[j];
        sl->open[i] = 0, d_slot[j] = i, made = 1;
        box[i] = b, last_t[i] = t, hits[i] += 1;
        rec[(size_t)j * TRK_WORDS + 3] = (unsigned long long)d_cls[j] | ((unsigned long long)(unsigned)sl->id[i] << 32);
      }
      const int fixed = __syncthreads_count(made);             // one slot per thread: the pairs this round fixed
      if (fixed == 0) break;
      open_slots -= fixed, open_dets -= fixed;
    }
    if (wave == 0) {                                           // births: the k-th eligible unmatched detection takes the k-th free slot
      int nfree = 0;
      for (int base = 0; base < T; base += 64) {
        const int i = base + lane;
        const bool is_free = i < T && sl->id[i] == 0;
        const unsigned long long mask = __ballot(is_free);
        if (is_free) sl->free_list[nfree + __popcll(mask & ((1ull << lane) - 1ull))] = i;
        nfree += __popcll(mask);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      const int first = *next_id;
      int born = 0;                                            // eligible detections so far, with and without a slot
      for (int base = 0; base < m; base += 64) {
        const int j = base + lane;
        const bool unmatched = j < m && d_slot[j] < 0;
        const bool eligible = unmatched && __uint_as_float((unsigned)rec[(size_t)j * TRK_WORDS + 4]) >= score_thre;
        const unsigned long long mask = __ballot(eligible);
        const int k = born + __popcll(mask & ((1ull << lane) - 1ull));
        born += __popcll(mask);
        if (!unmatched) continue;
        int id = 0;
        if (eligible && k < nfree) {
          const int i = sl->free_list[k];
          id = first + k;
          ids[i] = id, box[i] = d_box[j], cls[i] = (int)d_cls[j], last_t[i] = t, hits[i] = 1;
        }
        rec[(size_t)j * TRK_WORDS + 3] = (unsigned long long)d_cls[j] | ((unsigned long long)(unsigned)id << 32);
      }
      if (lane == 0) {
        *next_id = first + min(born, nfree);
        if (born > nfree) atomicAdd(counters + 0, born - nfree);
      }
    }
    __syncthreads();
  }
};

__global__ __launch_bounds__(TRK_THREADS) void tracker_step_kernel(SastTrackerArgs a, SastTrackStepArgs st) {
  __shared__ SlotLds slots;
  extern __shared__ __attribute__((aligned(16))) unsigned char track_dyn[];
  const int s = blockIdx.x;
  const TrackRow row(a, s, &slots, track_dyn);
  if (st.reset && st.reset[s]) row.reset();
  if (!st.due[s]) return;
  const int m = min(max(st.counts[s], 0), a.max_det);
  row.step(reinterpret_cast<unsigned long long*>(st.records + (size_t)s * a.max_det * SAST_DET_RECORD_BYTES), m, (long long)st.ends[s]);
}

// One workgroup per recording.  The sorted check first (a row that fails it keeps its records), then run after run: the end of the
// run at `pos` is the lowest index behind it with another t, found 256 records at a time.
__global__ __launch_bounds__(TRK_THREADS) void tracker_run_kernel(SastTrackerArgs a, SastTrackRunArgs ru) {
  __shared__ SlotLds slots;
  __shared__ int run_end;
  extern __shared__ __attribute__((aligned(16))) unsigned char track_dyn[];
  const int s = blockIdx.x, tid = threadIdx.x;
  const TrackRow row(a, s, &slots, track_dyn);
  row.reset();
  const long long n = min(max((long long)ru.n[s], 0ll), (long long)ru.Dcap);
  unsigned long long* rec = reinterpret_cast<unsigned long long*>(ru.records) + (size_t)s * ru.Dcap * TRK_WORDS;
  int unsorted = 0;
  for (long long i = 1 + tid; i < n; i += TRK_THREADS) unsorted |= (long long)rec[i * TRK_WORDS] < (long long)rec[(i - 1) * TRK_WORDS];
  if (__syncthreads_or(unsorted)) {
    if (tid == 0) atomicAdd(a.counters + 2, 1);
    return;
  }
  long long pos = 0;
  while (pos < n) {
    const long long t = (long long)rec[pos * TRK_WORDS];
    long long end = n;
    for (long long base = pos + 1; base < n; base += TRK_THREADS) {
      if (tid == 0) run_end = INT_MAX;
      __syncthreads();
      const long long i = base + tid;
      if (i < n && (long long)rec[i * TRK_WORDS] != t) atomicMin(&run_end, (int)(i - base));
      __syncthreads();
      const int hit = run_end;
      __syncthreads();
      if (hit != INT_MAX) {
        end = base + hit;
        break;
      }
    }
    const long long len = end - pos;
    const int m = (int)min(len, (long long)a.max_det);
    row.step(rec + pos * TRK_WORDS, m, t);
    if (len > m) {                                             // the run is cut: the rest carries no id
      for (long long i = pos + m + tid; i < end; i += TRK_THREADS) rec[i * TRK_WORDS + 3] &= 0xffffffffull;
      if (tid == 0) atomicAdd(a.counters + 1, 1);
    }
    pos = end;
  }
}

size_t track_lds_bytes(int max_det) { return 32 * (((size_t)max_det + 1) & ~(size_t)1); }

bool tracker_args_ok(const SastTrackerArgs* a) {
  return a && a->ids && a->box && a->cls && a->last_t && a->hits && a->next_id && a->counters && a->S >= 1 && a->S <= 65535 &&
         a->max_tracks >= 1 && a->max_tracks <= SAST_TRACK_MAX_TRACKS && a->max_det >= 1 && a->max_det <= SAST_TRACK_MAX_DET &&
         (long long)a->max_tracks * a->max_det <= SAST_TRACK_MAX_PAIRS && a->iou_thre > 0.f && a->iou_thre <= 1.f &&
         a->new_score_thre == a->new_score_thre && a->max_age_us >= 0 && !(reinterpret_cast<uintptr_t>(a->box) & 15) &&
         !(reinterpret_cast<uintptr_t>(a->last_t) & 7);
}

}  // namespace
}  // namespace sast

extern "C" {

int sast_tracker_step(const SastTrackerArgs* tr, const SastTrackStepArgs* step, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::tracker_args_ok(tr) || !step || !step->records || !step->counts || !step->ends || !step->due ||
      (reinterpret_cast<uintptr_t>(step->records) & 7))
    return SAST_EINVAL;
  SAST_LAUNCH(sast::tracker_step_kernel, dim3((unsigned)tr->S), dim3(sast::TRK_THREADS), sast::track_lds_bytes(tr->max_det), (hipStream_t)stream,
              *tr, *step);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_tracker_run(const SastTrackerArgs* tr, const SastTrackRunArgs* run, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::tracker_args_ok(tr) || !run || !run->records || !run->n || run->Dcap < 1 || (long long)tr->S * run->Dcap > 0x7fffffffll ||
      (reinterpret_cast<uintptr_t>(run->records) & 7))
    return SAST_EINVAL;
  SAST_LAUNCH(sast::tracker_run_kernel, dim3((unsigned)tr->S), dim3(sast::TRK_THREADS), sast::track_lds_bytes(tr->max_det), (hipStream_t)stream,
              *tr, *run);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
