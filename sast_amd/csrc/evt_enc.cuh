// Event columns or packed Event2D records -> raw sensor words on the device: what the encoders of k_evt3_enc.hip (EVT 3.0) and
// k_evt2_enc.hip (EVT 2.0 / 2.1) share.  A format is a policy F:
//   Word                      the word type (16 / 32 / 64 bit)
//   BACK, AHEAD               the neighbours i - BACK .. i + AHEAD an event's words depend on (BACK 1 or 2)
//   Words                     what a leader sends;  count(Words) its words (0 for an event that is no leader), leader(Words)
//   event(w, l, i, row)       the Words of event i, entry l = i - b0 + BACK of the normalised window w
//   put(Words, t, tp, e, out, pos, max_words)   the leader's words at out[pos ..), none at or past max_words
//   state2(e)                 word 2 of the row's state after the event e
//
// After an event has been encoded the state a decoder holds is fully given by that event, so the words of event i depend on its
// neighbours i - BACK .. i + AHEAD alone, once the events are NORMALISED: t the running maximum of the row (from the carry t_last, 0
// for a new recording), x and y clamped to 0 .. 2047, p != 0.  Only the running maximum reaches further back, and only in a row whose
// times are not sorted.  So:
//   launch 1  every workgroup takes its piece [lo, hi) of the row with the carry raw t[lo-1] (the row's carry for lo == 0) and writes a
//             summary into ws: the words of the piece, its largest t, the events it had to raise to the running maximum, the events it
//             clamped.  Workgroup 0 also writes the row's state (zero with its reset flag) into slot 0.
//   launch 2  every workgroup folds the row's summaries.  No raised event anywhere: the row is sorted from its carry on, every summary
//             is exact, the words of the pieces in front give the offset and the workgroup writes the words of its piece.  Otherwise
//             the times of a piece depend on every event before it: the row's LAST workgroup alone walks the whole row, once to count
//             and once to write (bad input, counted in err[0]: correct, not fast).  A row whose words exceed max_words is refused whole.
//             The row's last workgroup writes the new state, n_words and the counters.
// Both launches run en_range: per step of EN_BLOCK_EVENTS events the window [b0 - BACK, b0 + EN_BLOCK_EVENTS + AHEAD) is staged in LDS,
// normalised there (a max-scan over the threads), every event is evaluated by F::event and the word counts are scanned.
// A workgroup reads only what the earlier launch wrote.  Every index is formed from device-read counts clamped to their capacities;
// every store of a word is guarded by max_words.
#pragma once
#include <climits>
#include "common.cuh"
#include "kernels.h"

namespace sast {
namespace {

constexpr int EN_THREADS = 256;
constexpr int EN_PER_THREAD = 4;                                 // consecutive events of one thread per step
constexpr int EN_BLOCK_EVENTS = 1024;
constexpr int EN_MAX_BLOCKS = 256;
constexpr int EN_SUM_WORDS = 4;                                  // int64 of a summary: words, tmax, raised, clamped
constexpr int EN_ROW_WS = (EN_MAX_BLOCKS + 1) * EN_SUM_WORDS;    // int64 of a row's ws: slot 0 the state, slot 1 + b workgroup b
constexpr unsigned EN_OUTSIDE = 0x80000000u;                     // an entry of the window that is no event of the chunk
static_assert(EN_BLOCK_EVENTS == EN_THREADS * EN_PER_THREAD, "one step of a workgroup is EN_PER_THREAD consecutive events per thread");
static_assert(EN_MAX_BLOCKS <= EN_THREADS, "launch 2 folds the row's summaries one per thread");

struct EnColumns {
  const void *x, *y, *p, *t;       // [S, chunk_events]
  int xd, yd, pd, td;
};
struct EnRecords {
  const uint2* r;                  // [S, chunk_events]: u4 t, then x | y << 14 | p << 28
};

__device__ __forceinline__ long long en_ld(const void* p, int dt, long long i) {
  if (dt == SAST_DT_I64) return static_cast<const long long*>(p)[i];
  if (dt == SAST_DT_I32) return static_cast<const int*>(p)[i];
  return static_cast<const short*>(p)[i];
}

// x | y << 11 | p << 22 of the normalised event; *changed: the normalisation changed x, y or p
__device__ __forceinline__ unsigned en_pack(long long x, long long y, long long p, int* changed) {
  const long long xc = min(max(x, 0LL), 2047LL), yc = min(max(y, 0LL), 2047LL), pc = p != 0 ? 1 : 0;
  *changed = (xc != x || yc != y || pc != p) ? 1 : 0;
  return (unsigned)xc | ((unsigned)yc << 11) | ((unsigned)pc << 22);
}

__device__ __forceinline__ long long en_time(const EnColumns& c, long long i) { return en_ld(c.t, c.td, i); }
__device__ __forceinline__ long long en_time(const EnRecords& c, long long i) { return (long long)c.r[i].x; }
__device__ __forceinline__ unsigned en_event_at(const EnColumns& c, long long i, long long* t, int* changed) {
  *t = en_ld(c.t, c.td, i);
  return en_pack(en_ld(c.x, c.xd, i), en_ld(c.y, c.yd, i), en_ld(c.p, c.pd, i), changed);
}
__device__ __forceinline__ unsigned en_event_at(const EnRecords& c, long long i, long long* t, int* changed) {
  const uint2 r = c.r[i];                                        // one 8-byte load per record
  *t = (long long)r.x;
  return en_pack((long long)(r.y & 16383u), (long long)((r.y >> 14) & 16383u), (long long)((r.y >> 28) & 1u), changed);
}

__device__ __forceinline__ int en_x(unsigned e) { return (int)(e & 0x7FFu); }
__device__ __forceinline__ int en_y(unsigned e) { return (int)((e >> 11) & 0x7FFu); }
__device__ __forceinline__ int en_p(unsigned e) { return (int)((e >> 22) & 1u); }

template <bool MAX>
__device__ __forceinline__ long long en_op(long long a, long long b) { return MAX ? max(a, b) : a + b; }

// the values of the workgroup's threads in thread order under max or +: returns the combination of the threads BEFORE this one (the
// identity for thread 0) and, in *total, of all of them.  sm: int64 [EN_THREADS / 64] in LDS, free on entry and free again on return.
template <bool MAX>
__device__ __forceinline__ long long en_scan(long long v, long long* sm, long long* total) {
  const long long id = MAX ? LLONG_MIN : 0LL;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(inc, d);
    if (lane >= d) inc = en_op<MAX>(o, inc);
  }
  if (lane == 63) sm[wave] = inc;
  long long before = __shfl_up(inc, 1);
  if (lane == 0) before = id;
  __syncthreads();
  long long front = id, all = id;
#pragma unroll
  for (int k = 0; k < EN_THREADS / 64; ++k) {
    const long long t = sm[k];
    if (k < wave) front = en_op<MAX>(front, t);
    all = en_op<MAX>(all, t);
  }
  __syncthreads();
  *total = all;
  return en_op<MAX>(front, before);
}

template <class F>
struct EnLds {
  static constexpr int WIN = F::BACK + EN_BLOCK_EVENTS + F::AHEAD;
  long long t[WIN];                // entry l: event b0 - BACK + l, raw and then normalised
  unsigned e[WIN];
  long long sm[EN_THREADS / 64];
};

struct EnRow {
  long long n;                     // events of the chunk
  int have, y_last;                // the state in front of the chunk
  long long t_last;
};

struct EnSum {
  long long words, tmax, raised, clamped;
};

// events [lo, hi) of the row whose first event is src[row0]: c1 the normalised time of event lo - 1 (the row's carry for lo == 0), c2 of
// event lo - 2 (any value for lo < 2).  WRITE: the words go to out[base ..).  The sums come back in every thread.
template <class F, class Src, bool WRITE>
__device__ EnSum en_range(const Src& src, long long row0, const EnRow& r, long long lo, long long hi, long long c1, long long c2,
                          typename F::Word* out, long long max_words, long long base, EnLds<F>& w) {
  constexpr int BACK = F::BACK, WIN = EnLds<F>::WIN;
  static_assert(BACK == 1 || BACK == 2, "the carries c1 and c2 are what a step hands to the next");
  using Words = typename F::Words;
  EnSum acc{0, c1, 0, 0};
  long long raised = 0, clamped = 0;
  for (long long b0 = lo; b0 < hi; b0 += EN_BLOCK_EVENTS) {
    const long long end = min(b0 + EN_BLOCK_EVENTS, hi);
    // the window, raw
    for (int l = threadIdx.x; l < WIN; l += EN_THREADS) {
      const long long i = b0 - BACK + l;
      long long t = LLONG_MIN;
      unsigned e = EN_OUTSIDE;
      if (i >= 0 && i < r.n) {
        int changed;
        e = en_event_at(src, row0 + i, &t, &changed);
        if (i >= b0 && i < end) clamped += changed;
      } else if (i == -1) {
        e = EN_OUTSIDE | ((unsigned)r.y_last << 11);             // the state in front of the chunk: its row, and c1 its time
      }
      if (l < BACK) t = l == BACK - 1 ? c1 : c2;
      w.t[l] = t;
      w.e[l] = e;
    }
    __syncthreads();
    // normalised: the running maximum from c1 over the thread's events, the threads in order, then the entries ahead of the step
    const int l0 = BACK + threadIdx.x * EN_PER_THREAD;
    long long raw[EN_PER_THREAD], m = LLONG_MIN;
#pragma unroll
    for (int k = 0; k < EN_PER_THREAD; ++k) {
      raw[k] = w.t[l0 + k];
      m = max(m, raw[k]);
    }
    long long all;
    long long run = max(c1, en_scan<true>(m, w.sm, &all));
#pragma unroll
    for (int k = 0; k < EN_PER_THREAD; ++k) {
      if (b0 + threadIdx.x * EN_PER_THREAD + k < end && raw[k] < run) ++raised;
      run = max(run, raw[k]);
      w.t[l0 + k] = run;
    }
    if (threadIdx.x == 0) {
      long long tail = max(c1, all);
      for (int l = BACK + EN_BLOCK_EVENTS; l < WIN; ++l) {
        tail = max(tail, w.t[l]);
        w.t[l] = tail;
      }
    }
    __syncthreads();
    // the words of the thread's events, and where they go
    Words ws[EN_PER_THREAD];
    long long cnt = 0;
#pragma unroll
    for (int k = 0; k < EN_PER_THREAD; ++k) {
      const long long i = b0 + threadIdx.x * EN_PER_THREAD + k;
      ws[k] = i < end ? F::event(w, l0 + k, i, r) : Words{};
      cnt += F::count(ws[k]);
    }
    long long step;
    long long pos = base + en_scan<false>(cnt, w.sm, &step);
    if (WRITE) {
#pragma unroll
      for (int k = 0; k < EN_PER_THREAD; ++k) {
        if (F::leader(ws[k])) F::put(ws[k], w.t[l0 + k], w.t[l0 + k - 1], w.e[l0 + k], out, pos, max_words);
        pos += F::count(ws[k]);
      }
    }
    base += step;
    acc.words += step;
    acc.tmax = w.t[BACK + (int)(end - b0) - 1];                  // the normalised time of event end - 1
    c1 = w.t[BACK + EN_BLOCK_EVENTS - 1];                        // read by a further step only: then this one was full
    c2 = w.t[BACK + EN_BLOCK_EVENTS - 2];
    __syncthreads();
  }
  en_scan<false>(raised, w.sm, &acc.raised);
  en_scan<false>(clamped, w.sm, &acc.clamped);
  return acc;
}

struct EnIn {
  const long long* counts;
  long long chunk_events;
  const unsigned char* reset;
};

// the row's event count and this workgroup's piece [lo, hi) of it: pieces are multiples of EN_PER_THREAD events
__device__ __forceinline__ long long en_piece(const EnIn& in, int s, long long* lo, long long* hi) {
  const long long n = min(max(in.counts[s], 0LL), in.chunk_events);
  const long long per = ((n + gridDim.x - 1) / gridDim.x + EN_PER_THREAD - 1) / EN_PER_THREAD * EN_PER_THREAD;
  *lo = min((long long)blockIdx.x * per, n);
  *hi = min(*lo + per, n);
  return n;
}

// launch 1: the summary of the workgroup's piece -> ws slot 1 + blockIdx.x, taking the raw times in front of the piece as normalised;
// workgroup 0 of a row also writes the state (zero with the row's reset flag) into slot 0.  Reads the state, writes only ws.
template <class F, class Src>
__global__ __launch_bounds__(EN_THREADS) void evt_enc_summary_kernel(Src src, EnIn in, const long long* state, long long* ws_all) {
  __shared__ EnLds<F> lds;
  const int s = blockIdx.y;
  const long long row0 = (long long)s * in.chunk_events;
  long long lo, hi;
  EnRow r;
  r.n = en_piece(in, s, &lo, &hi);
  const long long* q = state + (size_t)s * EN_SUM_WORDS;
  const bool rst = in.reset && in.reset[s];
  r.have = !rst && q[0] != 0;
  r.t_last = r.have ? max(q[1], 0LL) : 0LL;
  r.y_last = r.have ? (int)(q[2] & 0x7FF) : 0;
  const long long c1 = lo > 0 ? en_time(src, row0 + lo - 1) : r.t_last;
  const long long c2 = lo > 1 ? en_time(src, row0 + lo - 2) : LLONG_MIN;
  const EnSum sum = en_range<F, Src, false>(src, row0, r, lo, hi, c1, c2, nullptr, 0, 0, lds);
  if (threadIdx.x == 0) {
    long long* ws = ws_all + (size_t)s * EN_ROW_WS;
    long long* o = ws + (size_t)(1 + blockIdx.x) * EN_SUM_WORDS;
    o[0] = sum.words; o[1] = sum.tmax; o[2] = sum.raised; o[3] = sum.clamped;
    if (blockIdx.x == 0) {
      ws[0] = r.have; ws[1] = r.t_last; ws[2] = r.y_last; ws[3] = 0;
    }
  }
}

template <class F>
struct EnOut {
  typename F::Word* words;         // [S, max_words]
  long long max_words;
  long long* n_words;
  int* err;
  long long* state;
};

__device__ __forceinline__ int en_sat(long long v) { return (int)min(v, (long long)INT_MAX); }

// launch 2: the row's summaries folded, one per thread; the words of the workgroup's piece behind those of the pieces in front, or, in
// a row with raised times, of the whole row by its last workgroup; that workgroup then writes n_words, the state and the counters.
template <class F, class Src>
__global__ __launch_bounds__(EN_THREADS) void evt_enc_write_kernel(Src src, EnIn in, const long long* ws_all, EnOut<F> o) {
  __shared__ EnLds<F> lds;
  const int s = blockIdx.y;
  const long long row0 = (long long)s * in.chunk_events;
  const long long* ws = ws_all + (size_t)s * EN_ROW_WS;
  typename F::Word* out = o.words + (long long)s * o.max_words;
  long long lo, hi;
  EnRow r;
  r.n = en_piece(in, s, &lo, &hi);
  r.have = ws[0] != 0;
  r.t_last = ws[1];
  r.y_last = (int)(ws[2] & 0x7FF);
  const bool last = blockIdx.x == gridDim.x - 1;
  const bool mine = threadIdx.x < gridDim.x;
  const long long* q = ws + (size_t)(1 + (mine ? threadIdx.x : 0)) * EN_SUM_WORDS;
  EnSum tot;
  long long front;
  en_scan<false>(mine && threadIdx.x < blockIdx.x ? q[0] : 0LL, lds.sm, &front);
  en_scan<false>(mine ? q[0] : 0LL, lds.sm, &tot.words);
  en_scan<true>(mine ? q[1] : LLONG_MIN, lds.sm, &tot.tmax);
  en_scan<false>(mine ? q[2] : 0LL, lds.sm, &tot.raised);
  en_scan<false>(mine ? q[3] : 0LL, lds.sm, &tot.clamped);
  long long* st = o.state + (size_t)s * EN_SUM_WORDS;
  if (r.n == 0) {                                                // nothing to encode: the state stays, or is zeroed by the reset flag
    if (last && threadIdx.x == 0) {
      o.n_words[s] = 0;
      if (in.reset && in.reset[s]) st[0] = st[1] = st[2] = st[3] = 0;
    }
    return;
  }
  if (tot.raised > 0) {                                          // times not sorted: one workgroup, the whole row, count then write
    if (!last) return;
    tot = en_range<F, Src, false>(src, row0, r, 0, r.n, r.t_last, LLONG_MIN, nullptr, 0, 0, lds);
    lo = 0;
    hi = r.n;
    front = 0;
  }
  if (tot.words <= o.max_words) {
    const long long c1 = lo > 0 ? en_time(src, row0 + lo - 1) : r.t_last;
    const long long c2 = lo > 1 ? en_time(src, row0 + lo - 2) : LLONG_MIN;
    en_range<F, Src, true>(src, row0, r, lo, hi, c1, c2, out, o.max_words, front, lds);
  }
  if (last && threadIdx.x == 0) {
    if (tot.words > o.max_words) {                               // refused whole: the state stays, or is zeroed by the reset flag
      o.n_words[s] = 0;
      atomicAdd(&o.err[2], 1);
      if (in.reset && in.reset[s]) st[0] = st[1] = st[2] = st[3] = 0;
    } else {
      long long t;
      int changed;
      const unsigned e = en_event_at(src, row0 + r.n - 1, &t, &changed);
      o.n_words[s] = tot.words;
      st[0] = 1; st[1] = tot.tmax; st[2] = F::state2(e); st[3] = 0;
      if (tot.raised > 0) atomicAdd(&o.err[0], en_sat(tot.raised));
      if (tot.clamped > 0) atomicAdd(&o.err[1], en_sat(tot.clamped));
    }
  }
}

template <class F, class Src>
int en_launch(const Src& src, const int64_t* counts, int64_t chunk_events, int S, const uint8_t* reset, int64_t* state, void* ws,
              void* words, int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream) {
  const EnIn in{reinterpret_cast<const long long*>(counts), (long long)chunk_events, reinterpret_cast<const unsigned char*>(reset)};
  const EnOut<F> out{static_cast<typename F::Word*>(words), (long long)max_words, reinterpret_cast<long long*>(n_words), err,
                     reinterpret_cast<long long*>(state)};
  const long long per = (chunk_events + EN_BLOCK_EVENTS - 1) / EN_BLOCK_EVENTS;
  const dim3 grid((unsigned)std::min<long long>(std::max<long long>(per, 1), EN_MAX_BLOCKS), (unsigned)S);
  hipStream_t st = (hipStream_t)stream;
  SAST_LAUNCH((evt_enc_summary_kernel<F, Src>), grid, dim3(EN_THREADS), 0, st, src, in, reinterpret_cast<const long long*>(state),
              static_cast<long long*>(ws));
  SAST_LAUNCH((evt_enc_write_kernel<F, Src>), grid, dim3(EN_THREADS), 0, st, src, in, static_cast<const long long*>(ws), out);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

// word_bytes: the size of a word of `words`, a power of two
inline bool en_args_ok(const void* counts, int64_t chunk_events, int S, const void* state, const void* ws, const void* words,
                       int64_t max_words, const void* n_words, const void* err, size_t word_bytes) {
  if (!counts || !state || !ws || !words || !n_words || !err || S < 1 || S > 65535 || chunk_events < 0 || chunk_events > INT_MAX / S ||
      max_words < 1 || max_words > INT_MAX / S)
    return false;
  return !((uintptr_t)words & (word_bytes - 1)) && !((uintptr_t)ws & 7);
}

inline bool en_int_dtype(int dt) { return dt == SAST_DT_I64 || dt == SAST_DT_I32 || dt == SAST_DT_I16; }

inline size_t en_ws_bytes(int S) { return S < 1 || S > 65535 ? 0 : (size_t)S * EN_ROW_WS * sizeof(int64_t); }

}  // namespace
}  // namespace sast
