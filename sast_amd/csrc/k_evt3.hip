// Prophesee EVT 3.0 sensor words -> event columns on the device (sast_evt3_*; the format and the decode rule: include/sast_hip.h).
//
// The driver is csrc/evt_dec.cuh, shared with k_evt2.hip: the two launches, the scan of the summaries, the piece split, the loads and
// the write of the state, the count and the counters.  This file is the format.
// The stream is stateful (a current row, time and vector base address) and one word stands for 0 .. 12 events, but every state field
// composes over a range of words, so a range has a SUMMARY (Evt3::Sum) and summaries combine associatively, in stream order:
//   y, low          last setter wins (-1: the range sets none)
//   vpol, bx        the last VECT_BASE_X (vpol >= 0, bx absolute) or, with none in the range, the increments to add (vpol < 0)
//   hfirst, hlast   the range's first and last TIME_HIGH (-1: none), wraps the descending neighbour pairs inside it; combining two
//                   ranges adds the pair across the seam
//   n, pre, unk     events, events before the range's first TIME_HIGH, unknown words
// The row's state is the summary of everything before the chunk.  With R = state o (the words before word i): word i's events are
// given iff R.hfirst >= 0, at output offset R.n - R.pre, with R's y, bx, vpol and time.
#include "evt_dec.cuh"

namespace sast {
namespace {

constexpr int E3_BX_CAP = 1 << 30;                              // base_x stops growing here: far outside int16, far inside int32

struct Evt3 {
  using Word = unsigned short;
  static constexpr Word FILLER = 0xF000u;                       // a word without effect
  static constexpr int PER_THREAD = 8;                          // words of one thread per step: one 16-byte load
  static constexpr int BLOCK_WORDS = SAST_EVT3_BLOCK_WORDS, MAX_BLOCKS = SAST_EVT3_MAX_BLOCKS, STATE_WORDS = SAST_EVT3_STATE_WORDS;
  static constexpr int FANOUT = 12;

  struct Sum {
    int y, low, vpol, bx, hfirst, hlast, wraps, n, pre, unk;
  };

  static __device__ __forceinline__ Sum identity() { return Sum{-1, -1, -1, 0, -1, -1, 0, 0, 0, 0}; }

  // a then b
  static __device__ __forceinline__ Sum combine(const Sum& a, const Sum& b) {
    Sum r;
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
  static __device__ __forceinline__ unsigned mask(unsigned w) {
    const unsigned type = w >> 12;
    return type == 0x4 ? (w & 0xFFFu) : type == 0x5 ? (w & 0xFFu) : type == 0x2 ? 1u : 0u;
  }

  // r becomes r o (the one word w)
  static __device__ __forceinline__ void step(Sum& r, unsigned w) {
    const unsigned type = w >> 12;
    const int v = (int)(w & 0xFFFu);
    const int c = __popc(mask(w));
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

  static __device__ __forceinline__ void unpack(const uint4* q, Word (&w)[PER_THREAD]) {
    w[0] = q->x & 0xFFFFu; w[1] = q->x >> 16; w[2] = q->y & 0xFFFFu; w[3] = q->y >> 16;
    w[4] = q->z & 0xFFFFu; w[5] = q->z >> 16; w[6] = q->w & 0xFFFFu; w[7] = q->w >> 16;
  }

  // the state after a reset is not the identity: its setters have set 0
  static __device__ __forceinline__ Sum zero_state() { return Sum{0, 0, 0, 0, -1, -1, 0, 0, 0, 0}; }

  static __device__ __forceinline__ Sum load_state(const long long* q) {
    Sum st = zero_state();
    st.y = (int)(q[0] & 0x7FF);
    st.bx = (int)min(max(q[1], 0LL), (long long)E3_BX_CAP);
    st.vpol = (int)(q[2] & 1);
    st.low = (int)(q[3] & 0xFFF);
    if (q[6]) st.hfirst = st.hlast = (int)(q[4] & 0xFFF);
    st.wraps = (int)min(max(q[5], 0LL), (long long)(INT_MAX / 2));
    return st;
  }

  static __device__ __forceinline__ void store_state(const Sum& R, long long* q) {
    q[0] = R.y; q[1] = R.bx; q[2] = R.vpol; q[3] = R.low;
    q[4] = R.hfirst >= 0 ? R.hlast : 0;
    q[5] = R.wraps;
    q[6] = R.hfirst >= 0 ? 1 : 0;
    q[7] = 0;
  }

  static __device__ __forceinline__ short sat16(int v) { return (short)min(v, 32767); }

  // a single event carries its own x and polarity, a vector word takes r's base and polarity
  static __device__ __forceinline__ void emit(const Sum& r, unsigned w, unsigned m, const DecOut& o, long long orow) {
    const bool single = (w >> 12) == 0x2;
    const int x0 = single ? (int)(w & 0x7FFu) : r.bx;
    const short pol = (short)(single ? (w >> 11) & 1u : (unsigned)r.vpol);
    const long long t = ((long long)r.wraps << 24) + ((long long)r.hlast << 12) + r.low;
    for (long long e = (long long)r.n - r.pre; m && e < o.max_events; m &= m - 1, ++e) {
      o.x[orow + e] = sat16(x0 + (single ? 0 : __ffs(m) - 1));
      o.y[orow + e] = (short)r.y;
      o.p[orow + e] = pol;
      o.t[orow + e] = t;
    }
  }
};

}  // namespace
}  // namespace sast

extern "C" {

size_t sast_evt3_ws_bytes(int S) { return sast::dec_ws_bytes<sast::Evt3>(S); }

int sast_evt3_decode(const void* words, const int64_t* counts, int64_t chunk_words, int S, const uint8_t* reset, int64_t* state,
                     void* ws, int16_t* x, int16_t* y, int16_t* p, int64_t* t, int64_t max_events, int64_t* out_counts, int32_t* err,
                     sast_stream_t stream) {
  SAST_ENTRY();
  return sast::dec_launch<sast::Evt3>(words, counts, chunk_words, S, reset, state, ws, x, y, p, t, max_events, out_counts, err, stream);
}

}  // extern "C"
