// Prophesee EVT 3.0 sensor words -> event columns on the device (sast_evt3_*; the format and the decode rule: include/sast_hip.h).
//
// The stream is stateful (a current row, time and vector base address) and one word stands for 0 .. 12 events, but every state field
// composes over a range of words, so a range has a SUMMARY (Evt3Sum) and summaries combine associatively, in stream order:
//   y, low          last setter wins (-1: the range sets none)
//   vpol, bx        the last VECT_BASE_X (vpol >= 0, bx absolute) or, with none in the range, the increments to add (vpol < 0)
//   hfirst, hlast   the range's first and last TIME_HIGH (-1: none), wraps the descending neighbour pairs inside it; combining two
//                   ranges adds the pair across the seam
//   n, pre, unk     events, events before the range's first TIME_HIGH, unknown words
// The row's state is the summary of everything before the chunk.  With R = state o (the words before word i): word i's events are
// given iff R.hfirst >= 0, at output offset R.n - R.pre, with R's y, bx, vpol and time.
// Launch 1 writes the state's summary and one summary per (row, workgroup) into ws; in launch 2 every workgroup folds the summaries in
// front of it, scans its own words and writes its events; the row's last workgroup writes the new state, the count and the counters.
// A workgroup reads only what the earlier launch wrote.  Every index is formed from device-read counts clamped to their capacities.
#include <climits>
#include "common.cuh"
#include "kernels.h"

namespace sast {
namespace {

constexpr int E3_THREADS = 256;
constexpr int E3_PER_THREAD = 8;                                // words of one thread per step: one 16-byte load
constexpr int E3_BLOCK_WORDS = SAST_EVT3_BLOCK_WORDS;
constexpr int E3_MAX_BLOCKS = SAST_EVT3_MAX_BLOCKS;
constexpr int E3_BX_CAP = 1 << 30;                              // base_x stops growing here: far outside int16, far inside int32
static_assert(E3_BLOCK_WORDS == E3_THREADS * E3_PER_THREAD, "one step of a workgroup is one 16-byte load per thread");
static_assert(E3_MAX_BLOCKS <= E3_THREADS, "launch 2 folds the summaries in front of a workgroup one per thread");

struct Evt3Sum {
  int y, low, vpol, bx, hfirst, hlast, wraps, n, pre, unk;
};
constexpr int E3_SUM_INTS = sizeof(Evt3Sum) / sizeof(int);
constexpr int E3_ROW_WS = (E3_MAX_BLOCKS + 1) * E3_SUM_INTS;    // ints of a row's ws: slot 0 the state, slot 1 + b workgroup b

__device__ __forceinline__ Evt3Sum e3_identity() { return Evt3Sum{-1, -1, -1, 0, -1, -1, 0, 0, 0, 0}; }

// a then b
__device__ __forceinline__ Evt3Sum e3_combine(const Evt3Sum& a, const Evt3Sum& b) {
  Evt3Sum r;
  r.y = b.y >= 0 ? b.y : a.y;
  r.low = b.low >= 0 ? b.low : a.low;
  r.vpol = b.vpol >= 0 ? b.vpol : a.vpol;
  r.bx = b.vpol >= 0 ? b.bx : min(a.bx + b.bx, E3_BX_CAP);    // both <= 2^30: the sum fits an int
  const bool ah = a.hfirst >= 0, bh = b.hfirst >= 0;
  r.hfirst = ah ? a.hfirst : b.hfirst;
  r.hlast = bh ? b.hlast : a.hlast;
  r.wraps = a.wraps + b.wraps + ((ah && bh && a.hlast - b.hfirst >= 2048) ? 1 : 0);
  r.n = a.n + b.n;
  r.pre = a.pre + (ah ? 0 : b.pre);                           // without a TIME_HIGH in a, a.pre == a.n
  r.unk = a.unk + b.unk;
  return r;
}

// events of word w (0 for every word that gives none): the mask of their bits
__device__ __forceinline__ unsigned e3_mask(unsigned w) {
  const unsigned type = w >> 12;
  return type == 0x4 ? (w & 0xFFFu) : type == 0x5 ? (w & 0xFFu) : type == 0x2 ? 1u : 0u;
}

// r becomes r o (the one word w)
__device__ __forceinline__ void e3_step(Evt3Sum& r, unsigned w) {
  const unsigned type = w >> 12;
  const int v = (int)(w & 0xFFFu);
  const int c = __popc(e3_mask(w));
  r.n += c;
  if (r.hfirst < 0) r.pre += c;
  switch (type) {
    case 0x0: r.y = v & 0x7FF; break;
    case 0x3: r.bx = v & 0x7FF; r.vpol = v >> 11; break;
    case 0x4: r.bx = min(r.bx + 12, E3_BX_CAP); break;
    case 0x5: r.bx = min(r.bx + 8, E3_BX_CAP); break;
    case 0x6: r.low = v; break;
    case 0x8:
      if (r.hfirst < 0) r.hfirst = v;
      else if (r.hlast - v >= 2048) r.wraps += 1;
      r.hlast = v;
      break;
    case 0x1: case 0x9: case 0xB: case 0xC: case 0xD: r.unk += 1; break;
    default: break;                                           // 0x2 gives its event above; 0x7, 0xA, 0xE, 0xF: valid, no effect
  }
}

__device__ __forceinline__ Evt3Sum e3_shfl_up(const Evt3Sum& s, int d) {
  Evt3Sum r;
  r.y = __shfl_up(s.y, d);
  r.low = __shfl_up(s.low, d);
  r.vpol = __shfl_up(s.vpol, d);
  r.bx = __shfl_up(s.bx, d);
  r.hfirst = __shfl_up(s.hfirst, d);
  r.hlast = __shfl_up(s.hlast, d);
  r.wraps = __shfl_up(s.wraps, d);
  r.n = __shfl_up(s.n, d);
  r.pre = __shfl_up(s.pre, d);
  r.unk = __shfl_up(s.unk, d);
  return r;
}

// the summaries of the workgroup's threads in thread order: returns the combination of the threads BEFORE this one (the identity for
// thread 0) and, in *total, of all of them.  sm: Evt3Sum [E3_THREADS / 64] in LDS, free on entry and free again on return.
__device__ __forceinline__ Evt3Sum e3_block_scan(const Evt3Sum& v, Evt3Sum* sm, Evt3Sum* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Evt3Sum inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Evt3Sum o = e3_shfl_up(inc, d);
    if (lane >= d) inc = e3_combine(o, inc);
  }
  if (lane == 63) sm[wave] = inc;
  Evt3Sum before = e3_shfl_up(inc, 1);
  if (lane == 0) before = e3_identity();
  __syncthreads();
  Evt3Sum front = e3_identity(), all = e3_identity();
#pragma unroll
  for (int k = 0; k < E3_THREADS / 64; ++k) {
    const Evt3Sum t = sm[k];
    if (k < wave) front = e3_combine(front, t);
    all = e3_combine(all, t);
  }
  __syncthreads();
  *total = all;
  return e3_combine(front, before);
}

struct Evt3In {
  const unsigned short* words;     // [S, chunk_words]
  const long long* counts;
  long long chunk_words;
  const unsigned char* reset;
  int vec;                         // rows start 16-byte aligned: a thread's 8 words are one load
};

// the row's word count and this workgroup's piece [lo, hi) of it: pieces are multiples of 8 words, so a piece starts 16-byte aligned
// whenever its row does
__device__ __forceinline__ void e3_piece(const Evt3In& in, int s, long long* lo, long long* hi) {
  const long long n = min(max(in.counts[s], 0LL), in.chunk_words);
  const long long per = ((n + gridDim.x - 1) / gridDim.x + E3_PER_THREAD - 1) / E3_PER_THREAD * E3_PER_THREAD;
  *lo = min((long long)blockIdx.x * per, n);
  *hi = min(*lo + per, n);
}

// the thread's words [i0, i0 + 8) of the row, those at or past hi as 0xF000 (a word without effect)
__device__ __forceinline__ void e3_load(const Evt3In& in, const unsigned short* row, long long i0, long long hi, unsigned (&w)[E3_PER_THREAD]) {
  if (in.vec && i0 + E3_PER_THREAD <= hi) {
    const uint4 q = *reinterpret_cast<const uint4*>(row + i0);
    w[0] = q.x & 0xFFFFu; w[1] = q.x >> 16; w[2] = q.y & 0xFFFFu; w[3] = q.y >> 16;
    w[4] = q.z & 0xFFFFu; w[5] = q.z >> 16; w[6] = q.w & 0xFFFFu; w[7] = q.w >> 16;
    return;
  }
#pragma unroll
  for (int k = 0; k < E3_PER_THREAD; ++k) w[k] = i0 + k < hi ? (unsigned)row[i0 + k] : 0xF000u;
}

__device__ __forceinline__ Evt3Sum e3_words_sum(const unsigned (&w)[E3_PER_THREAD]) {
  Evt3Sum r = e3_identity();
#pragma unroll
  for (int k = 0; k < E3_PER_THREAD; ++k) e3_step(r, w[k]);
  return r;
}

// launch 1: the summary of the workgroup's piece -> ws slot 1 + blockIdx.x; workgroup 0 of a row also writes the state (zero with the
// row's reset flag) as a summary into slot 0.  Reads the state, writes only ws.
__global__ __launch_bounds__(E3_THREADS) void evt3_summary_kernel(Evt3In in, const long long* state, int* ws_all) {
  __shared__ Evt3Sum sm[E3_THREADS / 64];
  const int s = blockIdx.y;
  const unsigned short* row = in.words + (long long)s * in.chunk_words;
  long long lo, hi;
  e3_piece(in, s, &lo, &hi);
  Evt3Sum acc = e3_identity();
  for (long long b0 = lo; b0 < hi; b0 += E3_BLOCK_WORDS) {
    unsigned w[E3_PER_THREAD];
    e3_load(in, row, b0 + (long long)threadIdx.x * E3_PER_THREAD, hi, w);
    Evt3Sum total;
    e3_block_scan(e3_words_sum(w), sm, &total);
    acc = e3_combine(acc, total);
  }
  if (threadIdx.x == 0) {
    Evt3Sum* ws = reinterpret_cast<Evt3Sum*>(ws_all + (size_t)s * E3_ROW_WS);
    ws[1 + blockIdx.x] = acc;
    if (blockIdx.x == 0) {
      Evt3Sum st = Evt3Sum{0, 0, 0, 0, -1, -1, 0, 0, 0, 0};
      if (!(in.reset && in.reset[s])) {
        const long long* q = state + (size_t)s * SAST_EVT3_STATE_WORDS;
        st.y = (int)(q[0] & 0x7FF);
        st.bx = (int)min(max(q[1], 0LL), (long long)E3_BX_CAP);
        st.vpol = (int)(q[2] & 1);
        st.low = (int)(q[3] & 0xFFF);
        if (q[6]) st.hfirst = st.hlast = (int)(q[4] & 0xFFF);
        st.wraps = (int)min(max(q[5], 0LL), (long long)(INT_MAX / 2));
      }
      ws[0] = st;
    }
  }
}

struct Evt3Out {
  short *x, *y, *p;                // [S, max_events]
  long long* t;
  long long max_events;
  long long* out_counts;
  int* err;
  long long* state;
};

__device__ __forceinline__ short e3_sat16(int v) { return (short)min(v, 32767); }

// launch 2: R = slots 0 .. blockIdx.x of the row's ws combined (one per thread), then per step the scan of the threads' words and the
// events of every word at R.n - R.pre on; the row's last workgroup ends with R = the state after the chunk.
__global__ __launch_bounds__(E3_THREADS) void evt3_decode_kernel(Evt3In in, const int* ws_all, Evt3Out o) {
  __shared__ Evt3Sum sm[E3_THREADS / 64];
  const int s = blockIdx.y;
  const unsigned short* row = in.words + (long long)s * in.chunk_words;
  const Evt3Sum* ws = reinterpret_cast<const Evt3Sum*>(ws_all + (size_t)s * E3_ROW_WS);
  const long long orow = (long long)s * o.max_events;
  long long lo, hi;
  e3_piece(in, s, &lo, &hi);
  Evt3Sum R;
  e3_block_scan(threadIdx.x <= blockIdx.x ? ws[threadIdx.x] : e3_identity(), sm, &R);
  for (long long b0 = lo; b0 < hi; b0 += E3_BLOCK_WORDS) {
    unsigned w[E3_PER_THREAD];
    e3_load(in, row, b0 + (long long)threadIdx.x * E3_PER_THREAD, hi, w);
    Evt3Sum total;
    const Evt3Sum before = e3_block_scan(e3_words_sum(w), sm, &total);
    Evt3Sum r = e3_combine(R, before);
#pragma unroll
    for (int k = 0; k < E3_PER_THREAD; ++k) {
      unsigned m = e3_mask(w[k]);
      if (m && r.hfirst >= 0) {
        const bool single = (w[k] >> 12) == 0x2;
        const int x0 = single ? (int)(w[k] & 0x7FFu) : r.bx;
        const short pol = (short)(single ? (w[k] >> 11) & 1u : (unsigned)r.vpol);
        const long long t = ((long long)r.wraps << 24) + ((long long)r.hlast << 12) + r.low;
        long long e = (long long)r.n - r.pre;                 // >= 0: pre counts events of n
        for (; m && e < o.max_events; m &= m - 1, ++e) {
          o.x[orow + e] = e3_sat16(x0 + (single ? 0 : __ffs(m) - 1));
          o.y[orow + e] = (short)r.y;
          o.p[orow + e] = pol;
          o.t[orow + e] = t;
        }
      }
      e3_step(r, w[k]);
    }
    R = e3_combine(R, total);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const long long events = (long long)R.n - R.pre;
    o.out_counts[s] = min(events, o.max_events);
    long long* q = o.state + (size_t)s * SAST_EVT3_STATE_WORDS;
    q[0] = R.y; q[1] = R.bx; q[2] = R.vpol; q[3] = R.low;
    q[4] = R.hfirst >= 0 ? R.hlast : 0;
    q[5] = R.wraps;
    q[6] = R.hfirst >= 0 ? 1 : 0;
    q[7] = 0;
    if (R.pre > 0) atomicAdd(&o.err[0], R.pre);
    if (R.unk > 0) atomicAdd(&o.err[1], R.unk);
    if (events > o.max_events) atomicAdd(&o.err[2], (int)min(events - o.max_events, (long long)INT_MAX));
  }
}

}  // namespace
}  // namespace sast

extern "C" {

size_t sast_evt3_ws_bytes(int S) { return S < 1 || S > 65535 ? 0 : (size_t)S * sast::E3_ROW_WS * sizeof(int); }

int sast_evt3_decode(const void* words, const int64_t* counts, int64_t chunk_words, int S, const uint8_t* reset, int64_t* state,
                     void* ws, int16_t* x, int16_t* y, int16_t* p, int64_t* t, int64_t max_events, int64_t* out_counts, int32_t* err,
                     sast_stream_t stream) {
  SAST_ENTRY();
  if (!words || !counts || !state || !ws || !x || !y || !p || !t || !out_counts || !err || S < 1 || S > 65535 || chunk_words < 0 ||
      chunk_words > INT_MAX / 12 || chunk_words > INT_MAX / S || max_events < 1 || max_events > INT_MAX / S)
    return SAST_EINVAL;
  if (((uintptr_t)words & 1) || ((uintptr_t)ws & 3)) return SAST_EINVAL;
  const int vec = ((uintptr_t)words & 15) == 0 && chunk_words % sast::E3_PER_THREAD == 0;
  const sast::Evt3In in{static_cast<const unsigned short*>(words), reinterpret_cast<const long long*>(counts), (long long)chunk_words,
                        reinterpret_cast<const unsigned char*>(reset), vec};
  const sast::Evt3Out out{x, y, p, reinterpret_cast<long long*>(t), (long long)max_events, reinterpret_cast<long long*>(out_counts), err,
                          reinterpret_cast<long long*>(state)};
  const long long per = (chunk_words + sast::E3_BLOCK_WORDS - 1) / sast::E3_BLOCK_WORDS;
  const dim3 grid((unsigned)std::min<long long>(std::max<long long>(per, 1), sast::E3_MAX_BLOCKS), (unsigned)S);
  hipStream_t st = (hipStream_t)stream;
  SAST_LAUNCH(sast::evt3_summary_kernel, grid, dim3(sast::E3_THREADS), 0, st, in, reinterpret_cast<const long long*>(state),
              static_cast<int*>(ws));
  SAST_LAUNCH(sast::evt3_decode_kernel, grid, dim3(sast::E3_THREADS), 0, st, in, static_cast<const int*>(ws), out);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
