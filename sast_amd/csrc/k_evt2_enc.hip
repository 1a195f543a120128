// Event columns or packed Event2D records -> Prophesee EVT 2.0 (32-bit) or EVT 2.1 (64-bit) sensor words on the device
// (sast_evt2enc_*; the word tables and the canonical rule: include/sast_hip.h).  The inverse of k_evt2.hip.
//
// The driver is csrc/evt_enc.cuh, shared with k_evt3_enc.hip: the two launches, the source readers, the normalisation, the scans,
// the piece split, the window staged in LDS and the refusal.  This file is the two formats.  The only state a decoder holds is the
// time base, so an event's words depend on the event in front alone (EVT 2.0), and for EVT 2.1 on the up to 31 events behind it that
// its vector word takes in.
#include "evt_enc.cuh"

namespace sast {
namespace {

static_assert(SAST_EVT2_ENC_BLOCK_EVENTS == EN_BLOCK_EVENTS && SAST_EVT2_ENC_MAX_BLOCKS == EN_MAX_BLOCKS, "the header states the driver's sizes");
static_assert(SAST_EVT2_ENC_STATE_WORDS == EN_SUM_WORDS, "slot 0 of a row's ws holds the state");

constexpr long long E2_HIGH_MASK = 0x0FFFFFFF;                   // the 28 bits of a TIME_HIGH
constexpr int E2_KEEP_SHIFT = 26;                                // two neighbouring TIME_HIGHs are at most 2^26 steps apart

// what a leader sends: keep-alive TIME_HIGHs, a TIME_HIGH, then its event word with the mask `valid` (EVT 2.1)
struct E2Words {
  long long ka;
  unsigned flags, valid;
};
constexpr unsigned E2_TH = 1, E2_LEADER = 2;

template <bool V21>
struct Evt2Format {
  using Word = typename std::conditional<V21, unsigned long long, unsigned>::type;
  using Words = E2Words;
  static constexpr int BACK = 1, AHEAD = V21 ? 31 : 0;           // the neighbours an event's words depend on

  // event b continues the group of event a, the one in front of it: both in the chunk, one t, y and p, ascending x inside one block of
  // 32 (EVT 2.1; an EVT 2.0 word is one event)
  static __device__ __forceinline__ bool cont(long long ta, unsigned a, long long tb, unsigned b) {
    if (!V21 || ((a | b) & EN_OUTSIDE)) return false;
    return ta == tb && (a >> 11) == (b >> 11) && en_x(a) < en_x(b) && (en_x(a) >> 5) == (en_x(b) >> 5);
  }

  static __device__ __forceinline__ bool leader(const E2Words& w) { return (w.flags & E2_LEADER) != 0; }
  static __device__ __forceinline__ long long count(const E2Words& w) {
    if (!(w.flags & E2_LEADER)) return 0;
    return w.ka + (w.flags & E2_TH) + 1;
  }
  static __device__ __forceinline__ long long state2(unsigned) { return 0; }

  // the words of event i, entry l = i - b0 + 1 of the normalised window; entries l - 1 .. l + AHEAD are read
  static __device__ __forceinline__ E2Words event(const EnLds<Evt2Format>& w, int l, long long i, const EnRow& r) {
    E2Words o{0, 0, 0};
    const long long t = w.t[l], tp = w.t[l - 1];
    const unsigned e = w.e[l];
    if (cont(tp, w.e[l - 1], t, e)) return o;
    o.flags = E2_LEADER;
    if (i == 0 && !r.have) {
      o.flags |= E2_TH;
    } else {                                                       // entry l - 1 is the event in front, or the state for i == 0
      const long long H = t >> 6, Hp = tp >> 6;
      if (H > Hp) {
        o.ka = (H - Hp - 1) >> E2_KEEP_SHIFT;
        o.flags |= E2_TH;
      }
    }
    o.valid = 1u << (en_x(e) & 31);
    for (int k = 1; k <= AHEAD && cont(w.t[l + k - 1], w.e[l + k - 1], w.t[l + k], w.e[l + k]); ++k) o.valid |= 1u << (en_x(w.e[l + k]) & 31);
    return o;
  }

  static __device__ __forceinline__ Word time_high(long long H) {
    const Word v = (Word)(0x80000000u | (unsigned)(H & E2_HIGH_MASK));
    return V21 ? (Word)((unsigned long long)v << 32) : v;
  }

  // the leader's words at out[pos ..), none at or past max_words
  static __device__ __forceinline__ void put(const E2Words& w, long long t, long long tp, unsigned e, Word* out, long long pos,
                                             long long max_words) {
    const long long Hp = tp >> 6;
    for (long long q = 1; q <= w.ka && pos < max_words; ++q, ++pos) out[pos] = time_high(Hp + (q << E2_KEEP_SHIFT));
    if (w.flags & E2_TH) {
      if (pos < max_words) out[pos] = time_high(t >> 6);
      ++pos;
    }
    if (pos >= max_words) return;
    const unsigned ts6 = (unsigned)(t & 63);
    if (V21) {                                                     // x_base = 32 * (x >> 5), as a sensor aligns it
      const unsigned hi = ((unsigned)en_p(e) << 28) | (ts6 << 22) | ((unsigned)(en_x(e) & ~31) << 11) | (unsigned)en_y(e);
      out[pos] = (Word)(((unsigned long long)hi << 32) | w.valid);
    } else {
      out[pos] = (Word)(((unsigned)en_p(e) << 28) | (ts6 << 22) | ((unsigned)en_x(e) << 11) | (unsigned)en_y(e));
    }
  }
};

bool e2_args_ok(const void* counts, int64_t chunk_events, int S, int version, const void* state, const void* ws, const void* words,
                int64_t max_words, const void* n_words, const void* err) {
  if (version != SAST_EVT2_V20 && version != SAST_EVT2_V21) return false;
  return en_args_ok(counts, chunk_events, S, state, ws, words, max_words, n_words, err, version == SAST_EVT2_V21 ? 8 : 4);
}

template <class Src>
int e2_launch(const Src& src, const int64_t* counts, int64_t chunk_events, int S, int version, const uint8_t* reset, int64_t* state,
              void* ws, void* words, int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream) {
  if (version == SAST_EVT2_V21)
    return en_launch<Evt2Format<true>>(src, counts, chunk_events, S, reset, state, ws, words, max_words, n_words, err, stream);
  return en_launch<Evt2Format<false>>(src, counts, chunk_events, S, reset, state, ws, words, max_words, n_words, err, stream);
}

}  // namespace
}  // namespace sast

extern "C" {

size_t sast_evt2enc_ws_bytes(int S) { return sast::en_ws_bytes(S); }

int sast_evt2enc_encode(const void* x, const void* y, const void* p, const void* t, int x_dtype, int y_dtype, int p_dtype, int t_dtype,
                        const int64_t* counts, int64_t chunk_events, int S, int version, const uint8_t* reset, int64_t* state, void* ws,
                        void* words, int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream) {
  SAST_ENTRY();
  if (!x || !y || !p || !t || !sast::e2_args_ok(counts, chunk_events, S, version, state, ws, words, max_words, n_words, err))
    return SAST_EINVAL;
  if (!sast::en_int_dtype(x_dtype) || !sast::en_int_dtype(y_dtype) || !sast::en_int_dtype(p_dtype) ||
      (t_dtype != SAST_DT_I64 && t_dtype != SAST_DT_I32))
    return SAST_EINVAL;
  const sast::EnColumns src{x, y, p, t, x_dtype, y_dtype, p_dtype, t_dtype};
  return sast::e2_launch(src, counts, chunk_events, S, version, reset, state, ws, words, max_words, n_words, err, stream);
}

int sast_evt2enc_encode_dat(const void* records, const int64_t* counts, int64_t chunk_events, int S, int version, const uint8_t* reset,
                            int64_t* state, void* ws, void* words, int64_t max_words, int64_t* n_words, int32_t* err,
                            sast_stream_t stream) {
  SAST_ENTRY();
  if (!records || ((uintptr_t)records & 7) || !sast::e2_args_ok(counts, chunk_events, S, version, state, ws, words, max_words, n_words, err))
    return SAST_EINVAL;
  const sast::EnRecords src{static_cast<const uint2*>(records)};
  return sast::e2_launch(src, counts, chunk_events, S, version, reset, state, ws, words, max_words, n_words, err, stream);
}

}  // extern "C"
