// Prophesee EVT 2.0 and EVT 2.1 sensor words -> event columns on the device (sast_evt2_*; the formats and the decode rule:
// include/sast_hip.h).
//
// One kernel pair for both versions, templated on a format trait (Evt2V20: 32-bit words, a word is at most one event; Evt2V21: 64-bit
// words, a word is a 32-pixel vector) that gives the word type, the event mask of a word and the TIME_HIGH payload.  The stream's only
// state is the time base, and it composes over a range of words, so a range has a SUMMARY (Evt2Sum) and summaries combine
// associatively, in stream order:
//   hfirst, hlast   the range's first and last TIME_HIGH (-1: none), wraps the pairs inside it that descend by >= 2^27; combining two
//                   ranges adds the pair across the seam
//   n, pre, unk     events, events before the range's first TIME_HIGH, unknown words
// The row's state is the summary of everything before the chunk.  With R = state o (the words before word i): word i's events are
// given iff R.hfirst >= 0, at output offset R.n - R.pre (the popcount prefix of the event masks), with R's time base.
// Launch 1 writes the state's summary and one summary per (row, workgroup) into ws; in launch 2 every workgroup folds the summaries in
// front of it, scans its own words and writes its events; the row's last workgroup writes the new state, the count and the counters.
// A workgroup reads only what the earlier launch wrote.  Every index is formed from device-read counts clamped to their capacities.
// Integers only.
#include <climits>
#include "common.cuh"
#include "kernels.h"

namespace sast {
namespace {

constexpr int E2_THREADS = 256;
constexpr int E2_PER_THREAD = SAST_EVT2_THREAD_WORDS;           // words of one thread per step: one (2.0) or two (2.1) 16-byte loads
constexpr int E2_BLOCK_WORDS = SAST_EVT2_BLOCK_WORDS;
constexpr int E2_MAX_BLOCKS = SAST_EVT2_MAX_BLOCKS;
constexpr int E2_WRAP_STEP = 1 << 27;                           // a TIME_HIGH lower than its predecessor by this much is a wrap
constexpr unsigned E2_UNKNOWN_TYPES = 0x3AFCu;                  // bit `type` set: 0x2-0x7, 0x9, 0xB, 0xC, 0xD
static_assert(E2_BLOCK_WORDS == E2_THREADS * E2_PER_THREAD, "one step of a workgroup is E2_PER_THREAD words per thread");
static_assert(E2_MAX_BLOCKS <= E2_THREADS, "launch 2 folds the summaries in front of a workgroup one per thread");

struct Evt2V20 {
  using Word = unsigned int;
  static constexpr Word FILLER = 0xF0000000u;                   // CONTINUED: a word without effect
  static __device__ __forceinline__ unsigned type(Word w) { return w >> 28; }
  static __device__ __forceinline__ unsigned mask(Word w) { return (w >> 28) <= 1u ? 1u : 0u; }
  static __device__ __forceinline__ int high(Word w) { return (int)(w & 0x0FFFFFFFu); }
  static __device__ __forceinline__ int ts6(Word w) { return (int)((w >> 22) & 0x3Fu); }
  static __device__ __forceinline__ int x0(Word w) { return (int)((w >> 11) & 0x7FFu); }
  static __device__ __forceinline__ int y(Word w) { return (int)(w & 0x7FFu); }
  static __device__ __forceinline__ void unpack(const uint4* q, Word (&w)[E2_PER_THREAD]) {
    w[0] = q[0].x; w[1] = q[0].y; w[2] = q[0].z; w[3] = q[0].w;
  }
};

struct Evt2V21 {
  using Word = unsigned long long;
  static constexpr Word FILLER = 0xF000000000000000ull;
  static __device__ __forceinline__ unsigned type(Word w) { return (unsigned)(w >> 60); }
  static __device__ __forceinline__ unsigned mask(Word w) { return (w >> 60) <= 1ull ? (unsigned)w : 0u; }
  static __device__ __forceinline__ int high(Word w) { return (int)((w >> 32) & 0x0FFFFFFFull); }
  static __device__ __forceinline__ int ts6(Word w) { return (int)((w >> 54) & 0x3Full); }
  static __device__ __forceinline__ int x0(Word w) { return (int)((w >> 43) & 0x7FFull); }
  static __device__ __forceinline__ int y(Word w) { return (int)((w >> 32) & 0x7FFull); }
  static __device__ __forceinline__ void unpack(const uint4* q, Word (&w)[E2_PER_THREAD]) {
    w[0] = q[0].x | ((Word)q[0].y << 32); w[1] = q[0].z | ((Word)q[0].w << 32);
    w[2] = q[1].x | ((Word)q[1].y << 32); w[3] = q[1].z | ((Word)q[1].w << 32);
  }
};
static_assert(E2_PER_THREAD == 4, "the unpack of both traits takes four words");

struct Evt2Sum {
  int hfirst, hlast, wraps, n, pre, unk;
};
constexpr int E2_SUM_INTS = sizeof(Evt2Sum) / sizeof(int);
constexpr int E2_ROW_WS = (E2_MAX_BLOCKS + 1) * E2_SUM_INTS;    // ints of a row's ws: slot 0 the state, slot 1 + b workgroup b

__device__ __forceinline__ Evt2Sum e2_identity() { return Evt2Sum{-1, -1, 0, 0, 0, 0}; }

// a then b
__device__ __forceinline__ Evt2Sum e2_combine(const Evt2Sum& a, const Evt2Sum& b) {
  Evt2Sum r;
  const bool ah = a.hfirst >= 0, bh = b.hfirst >= 0;
  r.hfirst = ah ? a.hfirst : b.hfirst;
  r.hlast = bh ? b.hlast : a.hlast;
  r.wraps = a.wraps + b.wraps + ((ah && bh && a.hlast - b.hfirst >= E2_WRAP_STEP) ? 1 : 0);
  r.n = a.n + b.n;
  r.pre = a.pre + (ah ? 0 : b.pre);                             // without a TIME_HIGH in a, a.pre == a.n
  r.unk = a.unk + b.unk;
  return r;
}

// r becomes r o (the one word w)
template <class F>
__device__ __forceinline__ void e2_step(Evt2Sum& r, typename F::Word w) {
  const unsigned type = F::type(w);
  const int c = __popc(F::mask(w));
  r.n += c;
  if (r.hfirst < 0) r.pre += c;
  if (type == 0x8u) {
    const int v = F::high(w);
    if (r.hfirst < 0) r.hfirst = v;
    else if (r.hlast - v >= E2_WRAP_STEP) r.wraps += 1;
    r.hlast = v;
  }
  r.unk += (int)((E2_UNKNOWN_TYPES >> type) & 1u);
}

__device__ __forceinline__ Evt2Sum e2_shfl_up(const Evt2Sum& s, int d) {
  Evt2Sum r;
  r.hfirst = __shfl_up(s.hfirst, d);
  r.hlast = __shfl_up(s.hlast, d);
  r.wraps = __shfl_up(s.wraps, d);
  r.n = __shfl_up(s.n, d);
  r.pre = __shfl_up(s.pre, d);
  r.unk = __shfl_up(s.unk, d);
  return r;
}

// the summaries of the workgroup's threads in thread order: returns the combination of the threads BEFORE this one (the identity for
// thread 0) and, in *total, of all of them.  sm: Evt2Sum [E2_THREADS / 64] in LDS, free on entry and free again on return.
__device__ __forceinline__ Evt2Sum e2_block_scan(const Evt2Sum& v, Evt2Sum* sm, Evt2Sum* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Evt2Sum inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Evt2Sum o = e2_shfl_up(inc, d);
    if (lane >= d) inc = e2_combine(o, inc);
  }
  if (lane == 63) sm[wave] = inc;
  Evt2Sum before = e2_shfl_up(inc, 1);
  if (lane == 0) before = e2_identity();
  __syncthreads();
  Evt2Sum front = e2_identity(), all = e2_identity();
#pragma unroll
  for (int k = 0; k < E2_THREADS / 64; ++k) {
    const Evt2Sum t = sm[k];
    if (k < wave) front = e2_combine(front, t);
    all = e2_combine(all, t);
  }
  __syncthreads();
  *total = all;
  return e2_combine(front, before);
}

template <class F>
struct Evt2In {
  const typename F::Word* words;   // [S, chunk_words]
  const long long* counts;
  long long chunk_words;
  const unsigned char* reset;
  int vec;                         // rows start 16-byte aligned: a thread's 4 words are whole 16-byte loads
};

// the row's word count and this workgroup's piece [lo, hi) of it: pieces are multiples of 4 words, so a piece starts 16-byte aligned
// whenever its row does
template <class F>
__device__ __forceinline__ void e2_piece(const Evt2In<F>& in, int s, long long* lo, long long* hi) {
  const long long n = min(max(in.counts[s], 0LL), in.chunk_words);
  const long long per = ((n + gridDim.x - 1) / gridDim.x + E2_PER_THREAD - 1) / E2_PER_THREAD * E2_PER_THREAD;
  *lo = min((long long)blockIdx.x * per, n);
  *hi = min(*lo + per, n);
}

// the thread's words [i0, i0 + 4) of the row, those at or past hi as a word without effect
template <class F>
__device__ __forceinline__ void e2_load(const Evt2In<F>& in, const typename F::Word* row, long long i0, long long hi,
                                        typename F::Word (&w)[E2_PER_THREAD]) {
  constexpr int Q = E2_PER_THREAD * (int)sizeof(typename F::Word) / 16;
  if (in.vec && i0 + E2_PER_THREAD <= hi) {
    uint4 q[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) q[k] = reinterpret_cast<const uint4*>(row + i0)[k];
    F::unpack(q, w);
    return;
  }
#pragma unroll
  for (int k = 0; k < E2_PER_THREAD; ++k) w[k] = i0 + k < hi ? row[i0 + k] : F::FILLER;
}

template <class F>
__device__ __forceinline__ Evt2Sum e2_words_sum(const typename F::Word (&w)[E2_PER_THREAD]) {
  Evt2Sum r = e2_identity();
#pragma unroll
  for (int k = 0; k < E2_PER_THREAD; ++k) e2_step<F>(r, w[k]);
  return r;
}

// launch 1: the summary of the workgroup's piece -> ws slot 1 + blockIdx.x; workgroup 0 of a row also writes the state (zero with the
// row's reset flag) as a summary into slot 0.  Reads the state, writes only ws.
template <class F>
__global__ __launch_bounds__(E2_THREADS) void evt2_summary_kernel(Evt2In<F> in, const long long* state, int* ws_all) {
  __shared__ Evt2Sum sm[E2_THREADS / 64];
  const int s = blockIdx.y;
  const typename F::Word* row = in.words + (long long)s * in.chunk_words;
  long long lo, hi;
  e2_piece(in, s, &lo, &hi);
  Evt2Sum acc = e2_identity();
  for (long long b0 = lo; b0 < hi; b0 += E2_BLOCK_WORDS) {
    typename F::Word w[E2_PER_THREAD];
    e2_load<F>(in, row, b0 + (long long)threadIdx.x * E2_PER_THREAD, hi, w);
    Evt2Sum total;
    e2_block_scan(e2_words_sum<F>(w), sm, &total);
    acc = e2_combine(acc, total);
  }
  if (threadIdx.x == 0) {
    Evt2Sum* ws = reinterpret_cast<Evt2Sum*>(ws_all + (size_t)s * E2_ROW_WS);
    ws[1 + blockIdx.x] = acc;
    if (blockIdx.x == 0) {
      Evt2Sum st = e2_identity();
      if (!(in.reset && in.reset[s])) {
        const long long* q = state + (size_t)s * SAST_EVT2_STATE_WORDS;
        if (q[2]) st.hfirst = st.hlast = (int)(q[0] & 0x0FFFFFFF);
        st.wraps = (int)min(max(q[1], 0LL), (long long)(INT_MAX / 2));
      }
      ws[0] = st;
    }
  }
}

struct Evt2Out {
  short *x, *y, *p;                // [S, max_events]
  long long* t;
  long long max_events;
  long long* out_counts;
  int* err;
  long long* state;
};

// launch 2: R = slots 0 .. blockIdx.x of the row's ws combined (one per thread), then per step the scan of the threads' words and the
// events of every word at R.n - R.pre on; the row's last workgroup ends with R = the state after the chunk.
template <class F>
__global__ __launch_bounds__(E2_THREADS) void evt2_decode_kernel(Evt2In<F> in, const int* ws_all, Evt2Out o) {
  __shared__ Evt2Sum sm[E2_THREADS / 64];
  const int s = blockIdx.y;
  const typename F::Word* row = in.words + (long long)s * in.chunk_words;
  const Evt2Sum* ws = reinterpret_cast<const Evt2Sum*>(ws_all + (size_t)s * E2_ROW_WS);
  const long long orow = (long long)s * o.max_events;
  long long lo, hi;
  e2_piece(in, s, &lo, &hi);
  Evt2Sum R;
  e2_block_scan(threadIdx.x <= blockIdx.x ? ws[threadIdx.x] : e2_identity(), sm, &R);
  for (long long b0 = lo; b0 < hi; b0 += E2_BLOCK_WORDS) {
    typename F::Word w[E2_PER_THREAD];
    e2_load<F>(in, row, b0 + (long long)threadIdx.x * E2_PER_THREAD, hi, w);
    Evt2Sum total;
    const Evt2Sum before = e2_block_scan(e2_words_sum<F>(w), sm, &total);
    Evt2Sum r = e2_combine(R, before);
#pragma unroll
    for (int k = 0; k < E2_PER_THREAD; ++k) {
      unsigned m = F::mask(w[k]);
      if (m && r.hfirst >= 0) {
        const int x0 = F::x0(w[k]);
        const short yy = (short)F::y(w[k]), pol = (short)F::type(w[k]);
        const long long t = (long long)(((unsigned long long)r.wraps << 34) + ((unsigned long long)r.hlast << 6) +
                                        (unsigned long long)F::ts6(w[k]));
        long long e = (long long)r.n - r.pre;                   // >= 0: pre counts events of n
        for (; m && e < o.max_events; m &= m - 1, ++e) {
          o.x[orow + e] = (short)(x0 + __ffs(m) - 1);           // <= 2047 + 31: inside int16
          o.y[orow + e] = yy;
          o.p[orow + e] = pol;
          o.t[orow + e] = t;
        }
      }
      e2_step<F>(r, w[k]);
    }
    R = e2_combine(R, total);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const long long events = (long long)R.n - R.pre;
    o.out_counts[s] = min(events, o.max_events);
    long long* q = o.state + (size_t)s * SAST_EVT2_STATE_WORDS;
    q[0] = R.hfirst >= 0 ? R.hlast : 0;
    q[1] = R.wraps;
    q[2] = R.hfirst >= 0 ? 1 : 0;
    q[3] = 0;
    if (R.pre > 0) atomicAdd(&o.err[0], R.pre);
    if (R.unk > 0) atomicAdd(&o.err[1], R.unk);
    if (events > o.max_events) atomicAdd(&o.err[2], (int)min(events - o.max_events, (long long)INT_MAX));
  }
}

template <class F>
int evt2_launch(const void* words, const int64_t* counts, int64_t chunk_words, int S, const uint8_t* reset, int64_t* state, void* ws,
                const Evt2Out& out, hipStream_t st) {
  constexpr int WB = (int)sizeof(typename F::Word);
  const int vec = ((uintptr_t)words & 15) == 0 && (chunk_words * WB) % 16 == 0;
  const Evt2In<F> in{static_cast<const typename F::Word*>(words), reinterpret_cast<const long long*>(counts), (long long)chunk_words,
                     reinterpret_cast<const unsigned char*>(reset), vec};
  const long long per = (chunk_words + E2_BLOCK_WORDS - 1) / E2_BLOCK_WORDS;
  const dim3 grid((unsigned)std::min<long long>(std::max<long long>(per, 1), E2_MAX_BLOCKS), (unsigned)S);
  SAST_LAUNCH(evt2_summary_kernel<F>, grid, dim3(E2_THREADS), 0, st, in, reinterpret_cast<const long long*>(state), static_cast<int*>(ws));
  SAST_LAUNCH(evt2_decode_kernel<F>, grid, dim3(E2_THREADS), 0, st, in, static_cast<const int*>(ws), out);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // namespace
}  // namespace sast

extern "C" {

size_t sast_evt2_ws_bytes(int S) { return S < 1 || S > 65535 ? 0 : (size_t)S * sast::E2_ROW_WS * sizeof(int); }

int sast_evt2_decode(const void* words, const int64_t* counts, int64_t chunk_words, int S, int version, const uint8_t* reset,
                     int64_t* state, void* ws, int16_t* x, int16_t* y, int16_t* p, int64_t* t, int64_t max_events, int64_t* out_counts,
                     int32_t* err, sast_stream_t stream) {
  SAST_ENTRY();
  if (!words || !counts || !state || !ws || !x || !y || !p || !t || !out_counts || !err || S < 1 || S > 65535 ||
      (version != SAST_EVT2_V20 && version != SAST_EVT2_V21) || chunk_words < 0 || chunk_words > INT_MAX / S || max_events < 1 ||
      max_events > INT_MAX / S)
    return SAST_EINVAL;
  if (version == SAST_EVT2_V21 && chunk_words > INT_MAX / 32) return SAST_EINVAL;   // a row's events are counted in an int
  if (((uintptr_t)words & (version == SAST_EVT2_V21 ? 7 : 3)) || ((uintptr_t)ws & 3)) return SAST_EINVAL;
  const sast::Evt2Out out{x, y, p, reinterpret_cast<long long*>(t), (long long)max_events, reinterpret_cast<long long*>(out_counts), err,
                          reinterpret_cast<long long*>(state)};
  hipStream_t st = (hipStream_t)stream;
  if (version == SAST_EVT2_V21) return sast::evt2_launch<sast::Evt2V21>(words, counts, chunk_words, S, reset, state, ws, out, st);
  return sast::evt2_launch<sast::Evt2V20>(words, counts, chunk_words, S, reset, state, ws, out, st);
}

}  // extern "C"
