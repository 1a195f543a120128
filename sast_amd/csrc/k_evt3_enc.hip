// Event columns or packed Event2D records -> Prophesee EVT 3.0 sensor words on the device (sast_evt3enc_*; the word table and the
// canonical rule: include/sast_hip.h).  The inverse of k_evt3.hip.
//
// After an event has been encoded the state a decoder holds is fully given by that event, so the words of event i depend on its
// neighbours i-2 .. i+11 alone, once the events are NORMALISED: t the running maximum of the row (from the carry t_last, 0 for a new
// recording), x and y clamped to 0 .. 2047, p != 0.  Only the running maximum reaches further back than two events, and only in a row
// whose times are not sorted.  So:
//   launch 1  every workgroup takes its piece [lo, hi) of the row with the carry raw t[lo-1] (the row's carry for lo == 0) and writes a
//             summary into ws: the words of the piece, its largest t, the events it had to raise to the running maximum, the events it
//             clamped.  Workgroup 0 also writes the row's state (zero with its reset flag) into slot 0.
//   launch 2  every workgroup folds the row's summaries.  No raised event anywhere: the row is sorted from its carry on, every summary
//             is exact, the words of the pieces in front give the offset and the workgroup writes the words of its piece.  Otherwise
//             the times of a piece depend on every event before it: the row's LAST workgroup alone walks the whole row, once to count
//             and once to write (bad input, counted in err[0]: correct, not fast).  A row whose words exceed max_words is refused whole.
//             The row's last workgroup writes the new state, n_words and the counters.
// Both launches run en_range: per step of EN_BLOCK_EVENTS events the window [b0 - 2, b0 + EN_BLOCK_EVENTS + 11) is staged in LDS,
// normalised there (a max-scan over the threads), every event is evaluated by en_event and the word counts are scanned.
// A workgroup reads only what the earlier launch wrote.  Every index is formed from device-read counts clamped to their capacities;
// every store of a word is guarded by max_words.
#include <climits>
#include "common.cuh"
#include "kernels.h"

namespace sast {
namespace {

constexpr int EN_THREADS = 256;
constexpr int EN_PER_THREAD = 4;                                 // consecutive events of one thread per step
constexpr int EN_BLOCK_EVENTS = SAST_EVT3_ENC_BLOCK_EVENTS;
constexpr int EN_MAX_BLOCKS = SAST_EVT3_ENC_MAX_BLOCKS;
constexpr int EN_BACK = 2, EN_AHEAD = 11;                        // the neighbours an event's words depend on
constexpr int EN_WIN = EN_BACK + EN_BLOCK_EVENTS + EN_AHEAD;
constexpr int EN_SUM_WORDS = 4;                                  // int64 of a summary: words, tmax, raised, clamped
constexpr int EN_ROW_WS = (EN_MAX_BLOCKS + 1) * EN_SUM_WORDS;    // int64 of a row's ws: slot 0 the state, slot 1 + b workgroup b
constexpr unsigned EN_OUTSIDE = 0x80000000u;                     // an entry of the window that is no event of the chunk
static_assert(EN_BLOCK_EVENTS == EN_THREADS * EN_PER_THREAD, "one step of a workgroup is EN_PER_THREAD consecutive events per thread");
static_assert(EN_MAX_BLOCKS <= EN_THREADS, "launch 2 folds the row's summaries one per thread");
static_assert(SAST_EVT3_ENC_STATE_WORDS == EN_SUM_WORDS, "slot 0 of a row's ws holds the state");

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

// event b continues the group of event a, the one in front of it: both in the chunk, one t, y and p, ascending x inside one block of 12
__device__ __forceinline__ bool en_cont(long long ta, unsigned a, long long tb, unsigned b) {
  if ((a | b) & EN_OUTSIDE) return false;
  return ta == tb && (a >> 11) == (b >> 11) && en_x(a) < en_x(b) && en_x(a) / 12 == en_x(b) / 12;
}

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

struct EnLds {
  long long t[EN_WIN];             // entry l: event b0 - 2 + l, raw and then normalised
  unsigned e[EN_WIN];
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

// what a leader sends: keep-alive TIME_HIGHs, then one bit each for TIME_HIGH, TIME_LOW, ADDR_Y, VECT_BASE_X, VECT_12 (else ADDR_X)
struct EnWords {
  long long ka;
  unsigned flags, mask;
};
constexpr unsigned EN_TH = 1, EN_TL = 2, EN_AY = 4, EN_BX = 8, EN_VEC = 16, EN_LEADER = 32;

__device__ __forceinline__ long long en_count(const EnWords& w) {
  if (!(w.flags & EN_LEADER)) return 0;
  return w.ka + __popc(w.flags & (EN_TH | EN_TL | EN_AY | EN_BX)) + 1;
}

// the words of event i, entry l = i - b0 + 2 of the normalised window; entries l - 2 .. l + 11 are read
__device__ __forceinline__ EnWords en_event(const EnLds& w, int l, long long i, const EnRow& r) {
  EnWords o{0, 0, 0};
  const long long t = w.t[l], tp = w.t[l - 1];
  const unsigned e = w.e[l], ep = w.e[l - 1];
  if (en_cont(tp, ep, t, e)) return o;
  o.flags = EN_LEADER;
  if (i == 0 && !r.have) {
    o.flags |= EN_TH | EN_TL | EN_AY;
  } else {                                                       // entry l - 1 is the event in front, or the state for i == 0
    const long long H = t >> 12, Hp = tp >> 12;
    if (H > Hp) {
      o.ka = (H - Hp - 1) >> 10;
      o.flags |= EN_TH | EN_TL;
    }
    if ((t & 0xFFF) != (tp & 0xFFF)) o.flags |= EN_TL;
    if (en_y(e) != en_y(ep)) o.flags |= EN_AY;
  }
  unsigned mask = 1u << (en_x(e) % 12);
  int members = 1;
  for (int k = 1; k <= EN_AHEAD && en_cont(w.t[l + k - 1], w.e[l + k - 1], w.t[l + k], w.e[l + k]); ++k) {
    mask |= 1u << (en_x(w.e[l + k]) % 12);
    ++members;
  }
  if (members >= 2) {
    // chained: the group in front ended with a VECT_12 that left the decoder's base and polarity where this group starts
    const bool chained = en_cont(w.t[l - 2], w.e[l - 2], tp, ep) && !(e & EN_OUTSIDE) && tp == t && (ep >> 11) == (e >> 11) &&
                         en_x(ep) < en_x(e) && en_x(e) / 12 == en_x(ep) / 12 + 1;
    o.flags |= EN_VEC | (chained ? 0 : EN_BX);
    o.mask = mask;
  }
  return o;
}

// the leader's words at out[pos ..), none at or past max_words
__device__ __forceinline__ void en_put(const EnWords& w, long long t, long long tp, unsigned e, unsigned short* out, long long pos,
                                       long long max_words) {
  const long long Hp = tp >> 12;
  for (long long q = 1; q <= w.ka && pos < max_words; ++q, ++pos) out[pos] = (unsigned short)(0x8000u | (unsigned)((Hp + 1024 * q) & 0xFFF));
  unsigned v[5];
  int m = 0;
  if (w.flags & EN_TH) v[m++] = 0x8000u | (unsigned)((t >> 12) & 0xFFF);
  if (w.flags & EN_TL) v[m++] = 0x6000u | (unsigned)(t & 0xFFF);
  if (w.flags & EN_AY) v[m++] = 0x0000u | (unsigned)en_y(e);
  if (w.flags & EN_BX) v[m++] = 0x3000u | (unsigned)(12 * (en_x(e) / 12)) | ((unsigned)en_p(e) << 11);
  v[m++] = (w.flags & EN_VEC) ? (0x4000u | w.mask) : (0x2000u | (unsigned)en_x(e) | ((unsigned)en_p(e) << 11));
  for (int k = 0; k < m; ++k)
    if (pos + k < max_words) out[pos + k] = (unsigned short)v[k];
}

// events [lo, hi) of the row whose first event is src[row0]: c1 the normalised time of event lo - 1 (the row's carry for lo == 0), c2 of
// event lo - 2 (any value for lo < 2).  WRITE: the words go to out[base ..).  The sums come back in every thread.
template <class Src, bool WRITE>
__device__ EnSum en_range(const Src& src, long long row0, const EnRow& r, long long lo, long long hi, long long c1, long long c2,
                          unsigned short* out, long long max_words, long long base, EnLds& w) {
  EnSum acc{0, c1, 0, 0};
  long long raised = 0, clamped = 0;
  for (long long b0 = lo; b0 < hi; b0 += EN_BLOCK_EVENTS) {
    const long long end = min(b0 + EN_BLOCK_EVENTS, hi);
    // the window, raw
    for (int l = threadIdx.x; l < EN_WIN; l += EN_THREADS) {
      const long long i = b0 - EN_BACK + l;
      long long t = LLONG_MIN;
      unsigned e = EN_OUTSIDE;
      if (i >= 0 && i < r.n) {
        int changed;
        e = en_event_at(src, row0 + i, &t, &changed);
        if (i >= b0 && i < end) clamped += changed;
      } else if (i == -1) {
        e = EN_OUTSIDE | ((unsigned)r.y_last << 11);             // the state in front of the chunk: its row, and c1 its time
      }
      if (l < EN_BACK) t = l == 0 ? c2 : c1;
      w.t[l] = t;
      w.e[l] = e;
    }
    __syncthreads();
    // normalised: the running maximum from c1 over the thread's events, the threads in order, then the entries ahead of the step
    const int l0 = EN_BACK + threadIdx.x * EN_PER_THREAD;
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
      for (int l = EN_BACK + EN_BLOCK_EVENTS; l < EN_WIN; ++l) {
        tail = max(tail, w.t[l]);
        w.t[l] = tail;
      }
    }
    __syncthreads();
    // the words of the thread's events, and where they go
    EnWords ws[EN_PER_THREAD];
    long long cnt = 0;
#pragma unroll
    for (int k = 0; k < EN_PER_THREAD; ++k) {
      const long long i = b0 + threadIdx.x * EN_PER_THREAD + k;
      ws[k] = i < end ? en_event(w, l0 + k, i, r) : EnWords{0, 0, 0};
      cnt += en_count(ws[k]);
    }
    long long step;
    long long pos = base + en_scan<false>(cnt, w.sm, &step);
    if (WRITE) {
#pragma unroll
      for (int k = 0; k < EN_PER_THREAD; ++k) {
        if (ws[k].flags & EN_LEADER) en_put(ws[k], w.t[l0 + k], w.t[l0 + k - 1], w.e[l0 + k], out, pos, max_words);
        pos += en_count(ws[k]);
      }
    }
    base += step;
    acc.words += step;
    acc.tmax = w.t[EN_BACK + (int)(end - b0) - 1];               // the normalised time of event end - 1
    c1 = w.t[EN_BACK + EN_BLOCK_EVENTS - 1];                     // read by a further step only: then this one was full
    c2 = w.t[EN_BACK + EN_BLOCK_EVENTS - 2];
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
template <class Src>
__global__ __launch_bounds__(EN_THREADS) void evt3_enc_summary_kernel(Src src, EnIn in, const long long* state, long long* ws_all) {
  __shared__ EnLds lds;
  const int s = blockIdx.y;
  const long long row0 = (long long)s * in.chunk_events;
  long long lo, hi;
  EnRow r;
  r.n = en_piece(in, s, &lo, &hi);
  const long long* q = state + (size_t)s * SAST_EVT3_ENC_STATE_WORDS;
  const bool rst = in.reset && in.reset[s];
  r.have = !rst && q[0] != 0;
  r.t_last = r.have ? max(q[1], 0LL) : 0LL;
  r.y_last = r.have ? (int)(q[2] & 0x7FF) : 0;
  const long long c1 = lo > 0 ? en_time(src, row0 + lo - 1) : r.t_last;
  const long long c2 = lo > 1 ? en_time(src, row0 + lo - 2) : LLONG_MIN;
  const EnSum sum = en_range<Src, false>(src, row0, r, lo, hi, c1, c2, nullptr, 0, 0, lds);
  if (threadIdx.x == 0) {
    long long* ws = ws_all + (size_t)s * EN_ROW_WS;
    long long* o = ws + (size_t)(1 + blockIdx.x) * EN_SUM_WORDS;
    o[0] = sum.words; o[1] = sum.tmax; o[2] = sum.raised; o[3] = sum.clamped;
    if (blockIdx.x == 0) {
      ws[0] = r.have; ws[1] = r.t_last; ws[2] = r.y_last; ws[3] = 0;
    }
  }
}

struct EnOut {
  unsigned short* words;           // [S, max_words]
  long long max_words;
  long long* n_words;
  int* err;
  long long* state;
};

__device__ __forceinline__ int en_sat(long long v) { return (int)min(v, (long long)INT_MAX); }

// launch 2: the row's summaries folded, one per thread; the words of the workgroup's piece behind those of the pieces in front, or, in
// a row with raised times, of the whole row by its last workgroup; that workgroup then writes n_words, the state and the counters.
template <class Src>
__global__ __launch_bounds__(EN_THREADS) void evt3_enc_write_kernel(Src src, EnIn in, const long long* ws_all, EnOut o) {
  __shared__ EnLds lds;
  const int s = blockIdx.y;
  const long long row0 = (long long)s * in.chunk_events;
  const long long* ws = ws_all + (size_t)s * EN_ROW_WS;
  unsigned short* out = o.words + (long long)s * o.max_words;
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
  long long* st = o.state + (size_t)s * SAST_EVT3_ENC_STATE_WORDS;
  if (r.n == 0) {                                                // nothing to encode: the state stays, or is zeroed by the reset flag
    if (last && threadIdx.x == 0) {
      o.n_words[s] = 0;
      if (in.reset && in.reset[s]) st[0] = st[1] = st[2] = st[3] = 0;
    }
    return;
  }
  if (tot.raised > 0) {                                          // times not sorted: one workgroup, the whole row, count then write
    if (!last) return;
    tot = en_range<Src, false>(src, row0, r, 0, r.n, r.t_last, LLONG_MIN, nullptr, 0, 0, lds);
    lo = 0;
    hi = r.n;
    front = 0;
  }
  if (tot.words <= o.max_words) {
    const long long c1 = lo > 0 ? en_time(src, row0 + lo - 1) : r.t_last;
    const long long c2 = lo > 1 ? en_time(src, row0 + lo - 2) : LLONG_MIN;
    en_range<Src, true>(src, row0, r, lo, hi, c1, c2, out, o.max_words, front, lds);
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
      st[0] = 1; st[1] = tot.tmax; st[2] = en_y(e); st[3] = 0;
      if (tot.raised > 0) atomicAdd(&o.err[0], en_sat(tot.raised));
      if (tot.clamped > 0) atomicAdd(&o.err[1], en_sat(tot.clamped));
    }
  }
}

template <class Src>
int en_launch(const Src& src, const int64_t* counts, int64_t chunk_events, int S, const uint8_t* reset, int64_t* state, void* ws,
              void* words, int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream) {
  const EnIn in{reinterpret_cast<const long long*>(counts), (long long)chunk_events, reinterpret_cast<const unsigned char*>(reset)};
  const EnOut out{static_cast<unsigned short*>(words), (long long)max_words, reinterpret_cast<long long*>(n_words), err,
                  reinterpret_cast<long long*>(state)};
  const long long per = (chunk_events + EN_BLOCK_EVENTS - 1) / EN_BLOCK_EVENTS;
  const dim3 grid((unsigned)std::min<long long>(std::max<long long>(per, 1), EN_MAX_BLOCKS), (unsigned)S);
  hipStream_t st = (hipStream_t)stream;
  SAST_LAUNCH(evt3_enc_summary_kernel<Src>, grid, dim3(EN_THREADS), 0, st, src, in, reinterpret_cast<const long long*>(state),
              static_cast<long long*>(ws));
  SAST_LAUNCH(evt3_enc_write_kernel<Src>, grid, dim3(EN_THREADS), 0, st, src, in, static_cast<const long long*>(ws), out);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

bool en_args_ok(const void* counts, int64_t chunk_events, int S, const void* state, const void* ws, const void* words, int64_t max_words,
                const void* n_words, const void* err) {
  if (!counts || !state || !ws || !words || !n_words || !err || S < 1 || S > 65535 || chunk_events < 0 || chunk_events > INT_MAX / S ||
      max_words < 1 || max_words > INT_MAX / S)
    return false;
  return !((uintptr_t)words & 1) && !((uintptr_t)ws & 7);
}

bool en_int_dtype(int dt) { return dt == SAST_DT_I64 || dt == SAST_DT_I32 || dt == SAST_DT_I16; }

}  // namespace
}  // namespace sast

extern "C" {

size_t sast_evt3enc_ws_bytes(int S) { return S < 1 || S > 65535 ? 0 : (size_t)S * sast::EN_ROW_WS * sizeof(int64_t); }

int sast_evt3enc_encode(const void* x, const void* y, const void* p, const void* t, int x_dtype, int y_dtype, int p_dtype, int t_dtype,
                     const int64_t* counts, int64_t chunk_events, int S, const uint8_t* reset, int64_t* state, void* ws, void* words,
                     int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream) {
  SAST_ENTRY();
  if (!x || !y || !p || !t || !sast::en_args_ok(counts, chunk_events, S, state, ws, words, max_words, n_words, err)) return SAST_EINVAL;
  if (!sast::en_int_dtype(x_dtype) || !sast::en_int_dtype(y_dtype) || !sast::en_int_dtype(p_dtype) ||
      (t_dtype != SAST_DT_I64 && t_dtype != SAST_DT_I32))
    return SAST_EINVAL;
  const sast::EnColumns src{x, y, p, t, x_dtype, y_dtype, p_dtype, t_dtype};
  return sast::en_launch(src, counts, chunk_events, S, reset, state, ws, words, max_words, n_words, err, stream);
}

int sast_evt3enc_encode_dat(const void* records, const int64_t* counts, int64_t chunk_events, int S, const uint8_t* reset, int64_t* state,
                         void* ws, void* words, int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream) {
  SAST_ENTRY();
  if (!records || ((uintptr_t)records & 7) || !sast::en_args_ok(counts, chunk_events, S, state, ws, words, max_words, n_words, err))
    return SAST_EINVAL;
  const sast::EnRecords src{static_cast<const uint2*>(records)};
  return sast::en_launch(src, counts, chunk_events, S, reset, state, ws, words, max_words, n_words, err, stream);
}

}  // extern "C"
