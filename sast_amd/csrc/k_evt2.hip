// Prophesee EVT 2.0 and EVT 2.1 sensor words -> event columns on the device (sast_evt2_*; the formats and the decode rule:
// include/sast_hip.h).
//
// The driver is csrc/evt_dec.cuh, shared with k_evt3.hip: the two launches, the scan of the summaries, the piece split, the loads and
// the write of the state, the count and the counters.  This file is the two formats: one policy, Evt2<B>, over the bit layout B of a
// word (Evt2Bits20: 32-bit words, a word is at most one event; Evt2Bits21: 64-bit words, a word is a 32-pixel vector).
// The stream's only state is the time base, and it composes over a range of words, so a range has a SUMMARY (Evt2Sum) and summaries
// combine associatively, in stream order:
//   hfirst, hlast   the range's first and last TIME_HIGH (-1: none), wraps the pairs inside it that descend by >= 2^27; combining two
//                   ranges adds the pair across the seam
//   n, pre, unk     events, events before the range's first TIME_HIGH, unknown words
// The row's state is the summary of everything before the chunk.  With R = state o (the words before word i): word i's events are
// given iff R.hfirst >= 0, at output offset R.n - R.pre (the popcount prefix of the event masks), with R's time base.
#include "evt_dec.cuh"

namespace sast {
namespace {

constexpr int E2_PER_THREAD = SAST_EVT2_THREAD_WORDS;           // words of one thread per step: one (2.0) or two (2.1) 16-byte loads
constexpr int E2_WRAP_STEP = 1 << 27;                           // a TIME_HIGH lower than its predecessor by this much is a wrap
constexpr unsigned E2_UNKNOWN_TYPES = 0x3AFCu;                  // bit `type` set: 0x2-0x7, 0x9, 0xB, 0xC, 0xD

struct Evt2Bits20 {
  using Word = unsigned int;
  static constexpr Word FILLER = 0xF0000000u;                   // CONTINUED: a word without effect
  static constexpr int FANOUT = 1;
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

struct Evt2Bits21 {
  using Word = unsigned long long;
  static constexpr Word FILLER = 0xF000000000000000ull;
  static constexpr int FANOUT = 32;
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
static_assert(E2_PER_THREAD == 4, "the unpack of both layouts takes four words");

struct Evt2Sum {
  int hfirst, hlast, wraps, n, pre, unk;
};

template <class B>
struct Evt2 : B {
  using Word = typename B::Word;
  using Sum = Evt2Sum;
  static constexpr int PER_THREAD = E2_PER_THREAD;
  static constexpr int BLOCK_WORDS = SAST_EVT2_BLOCK_WORDS, MAX_BLOCKS = SAST_EVT2_MAX_BLOCKS, STATE_WORDS = SAST_EVT2_STATE_WORDS;

  static __device__ __forceinline__ Sum identity() { return Sum{-1, -1, 0, 0, 0, 0}; }

  // a then b
  static __device__ __forceinline__ Sum combine(const Sum& a, const Sum& b) {
    Sum r;
    const bool ah = a.hfirst >= 0, bh = b.hfirst >= 0;
    r.hfirst = ah ? a.hfirst : b.hfirst;
    r.hlast = bh ? b.hlast : a.hlast;
    r.wraps = a.wraps + b.wraps + ((ah && bh && a.hlast - b.hfirst >= E2_WRAP_STEP) ? 1 : 0);
    r.n = a.n + b.n;
    r.pre = a.pre + (ah ? 0 : b.pre);                           // without a TIME_HIGH in a, a.pre == a.n
    r.unk = a.unk + b.unk;
    return r;
  }

  // r becomes r o (the one word w)
  static __device__ __forceinline__ void step(Sum& r, Word w) {
    const unsigned type = B::type(w);
    const int c = __popc(B::mask(w));
    r.n += c;
    if (r.hfirst < 0) r.pre += c;
    if (type == 0x8u) {
      const int v = B::high(w);
      if (r.hfirst < 0) r.hfirst = v;
      else if (r.hlast - v >= E2_WRAP_STEP) r.wraps += 1;
      r.hlast = v;
    }
    r.unk += (int)((E2_UNKNOWN_TYPES >> type) & 1u);
  }

  static __device__ __forceinline__ Sum zero_state() { return identity(); }

  static __device__ __forceinline__ Sum load_state(const long long* q) {
    Sum st = identity();
    if (q[2]) st.hfirst = st.hlast = (int)(q[0] & 0x0FFFFFFF);
    st.wraps = (int)min(max(q[1], 0LL), (long long)(INT_MAX / 2));
    return st;
  }

  static __device__ __forceinline__ void store_state(const Sum& R, long long* q) {
    q[0] = R.hfirst >= 0 ? R.hlast : 0;
    q[1] = R.wraps;
    q[2] = R.hfirst >= 0 ? 1 : 0;
    q[3] = 0;
  }

  static __device__ __forceinline__ void emit(const Sum& r, Word w, unsigned m, const DecOut& o, long long orow) {
    const int x0 = B::x0(w);
    const short yy = (short)B::y(w), pol = (short)B::type(w);
    const long long t = (long long)(((unsigned long long)r.wraps << 34) + ((unsigned long long)r.hlast << 6) +
                                    (unsigned long long)B::ts6(w));
    for (long long e = (long long)r.n - r.pre; m && e < o.max_events; m &= m - 1, ++e) {
      o.x[orow + e] = (short)(x0 + __ffs(m) - 1);               // <= 2047 + 31: inside int16
      o.y[orow + e] = yy;
      o.p[orow + e] = pol;
      o.t[orow + e] = t;
    }
  }
};
using Evt2V20 = Evt2<Evt2Bits20>;
using Evt2V21 = Evt2<Evt2Bits21>;

}  // namespace
}  // namespace sast

extern "C" {

size_t sast_evt2_ws_bytes(int S) { return sast::dec_ws_bytes<sast::Evt2V20>(S); }

int sast_evt2_decode(const void* words, const int64_t* counts, int64_t chunk_words, int S, int version, const uint8_t* reset,
                     int64_t* state, void* ws, int16_t* x, int16_t* y, int16_t* p, int64_t* t, int64_t max_events, int64_t* out_counts,
                     int32_t* err, sast_stream_t stream) {
  SAST_ENTRY();
  if (version == SAST_EVT2_V21)
    return sast::dec_launch<sast::Evt2V21>(words, counts, chunk_words, S, reset, state, ws, x, y, p, t, max_events, out_counts, err, stream);
  if (version == SAST_EVT2_V20)
    return sast::dec_launch<sast::Evt2V20>(words, counts, chunk_words, S, reset, state, ws, x, y, p, t, max_events, out_counts, err, stream);
  return SAST_EINVAL;
}

}  // extern "C"
