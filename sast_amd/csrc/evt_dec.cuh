// Raw sensor words -> event columns on the device: what the decoders of k_evt3.hip (EVT 3.0) and k_evt2.hip (EVT 2.0 / 2.1) share.
// A format is a policy F:
//   Word, FILLER              the word type (16 / 32 / 64 bit) and a word without effect
//   PER_THREAD, BLOCK_WORDS, MAX_BLOCKS   words of one thread and of a workgroup per step, the most workgroups of a row
//   STATE_WORDS, FANOUT       int64 of a row's state, the events one word can give
//   Sum                       the summary of a range of words: ints only, among them hfirst (the range's first TIME_HIGH, -1: none),
//                             n, pre and unk (events, events before the range's first TIME_HIGH, unknown words)
//   identity(), combine(a, b), step(Sum&, Word)   the empty range, a then b (associative), r becomes r o (the one word)
//   mask(Word)                the event bits of a word (0 for every word that gives none)
//   unpack(const uint4*, Word (&)[PER_THREAD])    a thread's words from its 16-byte loads
//   zero_state(), load_state(const long long*), store_state(const Sum&, long long*)   a row's state <-> its summary
//   emit(r, w, m, out, orow)  the events m = mask(w) of word w with r the summary in front of it: to x, y, p, t[orow + e ..), e from
//                             r.n - r.pre on, none at or past max_events
//
// Every state field of a stream composes over a range of words, so a range has a summary and summaries combine associatively, in
// stream order.  The row's state is the summary of everything before the chunk.  With R = state o (the words before word i): word i's
// events are given iff R.hfirst >= 0, at output offset R.n - R.pre.
//   launch 1  writes the state's summary and one summary per (row, workgroup) into ws: slot 0 the state, slot 1 + b workgroup b.
//   launch 2  every workgroup folds the summaries in front of it, scans its own words and writes its events; the row's last workgroup
//             writes the new state, the count and the counters.
// A workgroup reads only what the earlier launch wrote.  Every index is formed from device-read counts clamped to their capacities.
// Integers only.
#pragma once
#include <climits>
#include "common.cuh"
#include "kernels.h"

namespace sast {
namespace {

constexpr int DEC_THREADS = 256;

template <class S>
__device__ __forceinline__ S dec_shfl_up(const S& s, int d) {
  constexpr int N = sizeof(S) / sizeof(int);
  static_assert(sizeof(S) == N * sizeof(int), "a summary is ints only");
  int v[N];
  S r;
  __builtin_memcpy(v, &s, sizeof(S));
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = __shfl_up(v[k], d);
  __builtin_memcpy(&r, v, sizeof(S));
  return r;
}

// the summaries of the workgroup's threads in thread order: returns the combination of the threads BEFORE this one (the identity for
// thread 0) and, in *total, of all of them.  sm: Sum [DEC_THREADS / 64] in LDS, free on entry and free again on return.
template <class F>
__device__ __forceinline__ typename F::Sum dec_block_scan(const typename F::Sum& v, typename F::Sum* sm, typename F::Sum* total) {
  using Sum = typename F::Sum;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Sum inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Sum o = dec_shfl_up(inc, d);
    if (lane >= d) inc = F::combine(o, inc);
  }
  if (lane == 63) sm[wave] = inc;
  Sum before = dec_shfl_up(inc, 1);
  if (lane == 0) before = F::identity();
  __syncthreads();
  Sum front = F::identity(), all = F::identity();
#pragma unroll
  for (int k = 0; k < DEC_THREADS / 64; ++k) {
    const Sum t = sm[k];
    if (k < wave) front = F::combine(front, t);
    all = F::combine(all, t);
  }
  __syncthreads();
  *total = all;
  return F::combine(front, before);
}

template <class F>
struct DecIn {
  const typename F::Word* words;   // [S, chunk_words]
  const long long* counts;
  long long chunk_words;
  const unsigned char* reset;
  int vec;                         // rows start 16-byte aligned: a thread's words are whole 16-byte loads
};

// the row's word count and this workgroup's piece [lo, hi) of it: pieces are multiples of PER_THREAD words, so a piece starts 16-byte
// aligned whenever its row does
template <class F>
__device__ __forceinline__ void dec_piece(const DecIn<F>& in, int s, long long* lo, long long* hi) {
  const long long n = min(max(in.counts[s], 0LL), in.chunk_words);
  const long long per = ((n + gridDim.x - 1) / gridDim.x + F::PER_THREAD - 1) / F::PER_THREAD * F::PER_THREAD;
  *lo = min((long long)blockIdx.x * per, n);
  *hi = min(*lo + per, n);
}

// the thread's words [i0, i0 + PER_THREAD) of the row, those at or past hi as a word without effect
template <class F>
__device__ __forceinline__ void dec_load(const DecIn<F>& in, const typename F::Word* row, long long i0, long long hi,
                                         typename F::Word (&w)[F::PER_THREAD]) {
  constexpr int Q = F::PER_THREAD * (int)sizeof(typename F::Word) / 16;
  static_assert(Q * 16 == F::PER_THREAD * (int)sizeof(typename F::Word), "a thread's words are whole 16-byte loads");
  if (in.vec && i0 + F::PER_THREAD <= hi) {
    uint4 q[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) q[k] = reinterpret_cast<const uint4*>(row + i0)[k];
    F::unpack(q, w);
    return;
  }
#pragma unroll
  for (int k = 0; k < F::PER_THREAD; ++k) w[k] = i0 + k < hi ? row[i0 + k] : F::FILLER;
}

template <class F>
__device__ __forceinline__ typename F::Sum dec_words_sum(const typename F::Word (&w)[F::PER_THREAD]) {
  typename F::Sum r = F::identity();
#pragma unroll
  for (int k = 0; k < F::PER_THREAD; ++k) F::step(r, w[k]);
  return r;
}

// launch 1: the summary of the workgroup's piece -> ws slot 1 + blockIdx.x; workgroup 0 of a row also writes the state (zero with the
// row's reset flag) as a summary into slot 0.  Reads the state, writes only ws.
template <class F>
__global__ __launch_bounds__(DEC_THREADS) void evt_dec_summary_kernel(DecIn<F> in, const long long* state, typename F::Sum* ws_all) {
  using Sum = typename F::Sum;
  __shared__ Sum sm[DEC_THREADS / 64];
  const int s = blockIdx.y;
  const typename F::Word* row = in.words + (long long)s * in.chunk_words;
  long long lo, hi;
  dec_piece(in, s, &lo, &hi);
  Sum acc = F::identity();
  for (long long b0 = lo; b0 < hi; b0 += F::BLOCK_WORDS) {
    typename F::Word w[F::PER_THREAD];
    dec_load<F>(in, row, b0 + (long long)threadIdx.x * F::PER_THREAD, hi, w);
    Sum total;
    dec_block_scan<F>(dec_words_sum<F>(w), sm, &total);
    acc = F::combine(acc, total);
  }
  if (threadIdx.x == 0) {
    Sum* ws = ws_all + (size_t)s * (F::MAX_BLOCKS + 1);
    ws[1 + blockIdx.x] = acc;
    if (blockIdx.x == 0) ws[0] = in.reset && in.reset[s] ? F::zero_state() : F::load_state(state + (size_t)s * F::STATE_WORDS);
  }
}

struct DecOut {
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
__global__ __launch_bounds__(DEC_THREADS) void evt_dec_decode_kernel(DecIn<F> in, const typename F::Sum* ws_all, DecOut o) {
  using Sum = typename F::Sum;
  __shared__ Sum sm[DEC_THREADS / 64];
  const int s = blockIdx.y;
  const typename F::Word* row = in.words + (long long)s * in.chunk_words;
  const Sum* ws = ws_all + (size_t)s * (F::MAX_BLOCKS + 1);
  const long long orow = (long long)s * o.max_events;
  long long lo, hi;
  dec_piece(in, s, &lo, &hi);
  Sum R;
  dec_block_scan<F>(threadIdx.x <= blockIdx.x ? ws[threadIdx.x] : F::identity(), sm, &R);
  for (long long b0 = lo; b0 < hi; b0 += F::BLOCK_WORDS) {
    typename F::Word w[F::PER_THREAD];
    dec_load<F>(in, row, b0 + (long long)threadIdx.x * F::PER_THREAD, hi, w);
    Sum total;
    const Sum before = dec_block_scan<F>(dec_words_sum<F>(w), sm, &total);
    Sum r = F::combine(R, before);
#pragma unroll
    for (int k = 0; k < F::PER_THREAD; ++k) {
      const unsigned m = F::mask(w[k]);
      if (m && r.hfirst >= 0) F::emit(r, w[k], m, o, orow);
      F::step(r, w[k]);
    }
    R = F::combine(R, total);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const long long events = (long long)R.n - R.pre;             // >= 0: pre counts events of n
    o.out_counts[s] = min(events, o.max_events);
    F::store_state(R, o.state + (size_t)s * F::STATE_WORDS);
    if (R.pre > 0) atomicAdd(&o.err[0], R.pre);
    if (R.unk > 0) atomicAdd(&o.err[1], R.unk);
    if (events > o.max_events) atomicAdd(&o.err[2], (int)min(events - o.max_events, (long long)INT_MAX));
  }
}

template <class F>
size_t dec_ws_bytes(int S) {
  return S < 1 || S > 65535 ? 0 : (size_t)S * (F::MAX_BLOCKS + 1) * sizeof(typename F::Sum);
}

// the argument checks of a decode entry point, then the two launches
template <class F>
int dec_launch(const void* words, const int64_t* counts, int64_t chunk_words, int S, const uint8_t* reset, int64_t* state, void* ws,
               int16_t* x, int16_t* y, int16_t* p, int64_t* t, int64_t max_events, int64_t* out_counts, int32_t* err,
               sast_stream_t stream) {
  using Word = typename F::Word;
  static_assert(F::BLOCK_WORDS == DEC_THREADS * F::PER_THREAD, "one step of a workgroup is PER_THREAD words per thread");
  static_assert(F::MAX_BLOCKS <= DEC_THREADS, "launch 2 folds the summaries in front of a workgroup one per thread");
  if (!words || !counts || !state || !ws || !x || !y || !p || !t || !out_counts || !err || S < 1 || S > 65535 || chunk_words < 0 ||
      chunk_words > INT_MAX / F::FANOUT || chunk_words > INT_MAX / S || max_events < 1 || max_events > INT_MAX / S)
    return SAST_EINVAL;                                          // a row's events are counted in an int
  if (((uintptr_t)words & (sizeof(Word) - 1)) || ((uintptr_t)ws & 3)) return SAST_EINVAL;
  const int vec = ((uintptr_t)words & 15) == 0 && (chunk_words * (int64_t)sizeof(Word)) % 16 == 0;
  const DecIn<F> in{static_cast<const Word*>(words), reinterpret_cast<const long long*>(counts), (long long)chunk_words,
                    reinterpret_cast<const unsigned char*>(reset), vec};
  const DecOut out{x, y, p, reinterpret_cast<long long*>(t), (long long)max_events, reinterpret_cast<long long*>(out_counts), err,
                   reinterpret_cast<long long*>(state)};
  const long long per = (chunk_words + F::BLOCK_WORDS - 1) / F::BLOCK_WORDS;
  const dim3 grid((unsigned)std::min<long long>(std::max<long long>(per, 1), F::MAX_BLOCKS), (unsigned)S);
  hipStream_t st = (hipStream_t)stream;
  SAST_LAUNCH(evt_dec_summary_kernel<F>, grid, dim3(DEC_THREADS), 0, st, in, reinterpret_cast<const long long*>(state),
              static_cast<typename F::Sum*>(ws));
  SAST_LAUNCH(evt_dec_decode_kernel<F>, grid, dim3(DEC_THREADS), 0, st, in, static_cast<const typename F::Sum*>(ws), out);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // namespace
}  // namespace sast
