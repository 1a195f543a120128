// Event columns or packed Event2D records -> Prophesee EVT 3.0 sensor words on the device (sast_evt3enc_*; the word table and the
// canonical rule: include/sast_hip.h).  The inverse of k_evt3.hip.
//
// The driver is csrc/evt_enc.cuh, shared with k_evt2_enc.hip: the two launches, the source readers, the normalisation, the scans,
// the piece split, the window staged in LDS and the refusal.  This file is the format: the words of event i depend on its
// neighbours i-2 .. i+11.
#include "evt_enc.cuh"

namespace sast {
namespace {

static_assert(SAST_EVT3_ENC_BLOCK_EVENTS == EN_BLOCK_EVENTS && SAST_EVT3_ENC_MAX_BLOCKS == EN_MAX_BLOCKS, "the header states the driver's sizes");
static_assert(SAST_EVT3_ENC_STATE_WORDS == EN_SUM_WORDS, "slot 0 of a row's ws holds the state");

// event b continues the group of event a, the one in front of it: both in the chunk, one t, y and p, ascending x inside one block of 12
__device__ __forceinline__ bool en_cont(long long ta, unsigned a, long long tb, unsigned b) {
  if ((a | b) & EN_OUTSIDE) return false;
  return ta == tb && (a >> 11) == (b >> 11) && en_x(a) < en_x(b) && en_x(a) / 12 == en_x(b) / 12;
}

// what a leader sends: keep-alive TIME_HIGHs, then one bit each for TIME_HIGH, TIME_LOW, ADDR_Y, VECT_BASE_X, VECT_12 (else ADDR_X)
struct EnWords {
  long long ka;
  unsigned flags, mask;
};
constexpr unsigned EN_TH = 1, EN_TL = 2, EN_AY = 4, EN_BX = 8, EN_VEC = 16, EN_LEADER = 32;

struct Evt3Format {
  using Word = unsigned short;
  using Words = EnWords;
  static constexpr int BACK = 2, AHEAD = 11;                     // the neighbours an event's words depend on

  static __device__ __forceinline__ bool leader(const EnWords& w) { return (w.flags & EN_LEADER) != 0; }
  static __device__ __forceinline__ long long count(const EnWords& w) {
    if (!(w.flags & EN_LEADER)) return 0;
    return w.ka + __popc(w.flags & (EN_TH | EN_TL | EN_AY | EN_BX)) + 1;
  }
  static __device__ __forceinline__ long long state2(unsigned e) { return en_y(e); }

  // the words of event i, entry l = i - b0 + 2 of the normalised window; entries l - 2 .. l + 11 are read
  static __device__ __forceinline__ EnWords event(const EnLds<Evt3Format>& w, int l, long long i, const EnRow& r) {
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
    for (int k = 1; k <= AHEAD && en_cont(w.t[l + k - 1], w.e[l + k - 1], w.t[l + k], w.e[l + k]); ++k) {
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
  static __device__ __forceinline__ void put(const EnWords& w, long long t, long long tp, unsigned e, unsigned short* out, long long pos,
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
};

}  // namespace
}  // namespace sast

extern "C" {

size_t sast_evt3enc_ws_bytes(int S) { return sast::en_ws_bytes(S); }

int sast_evt3enc_encode(const void* x, const void* y, const void* p, const void* t, int x_dtype, int y_dtype, int p_dtype, int t_dtype,
                     const int64_t* counts, int64_t chunk_events, int S, const uint8_t* reset, int64_t* state, void* ws, void* words,
                     int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream) {
  SAST_ENTRY();
  if (!x || !y || !p || !t || !sast::en_args_ok(counts, chunk_events, S, state, ws, words, max_words, n_words, err, 2)) return SAST_EINVAL;
  if (!sast::en_int_dtype(x_dtype) || !sast::en_int_dtype(y_dtype) || !sast::en_int_dtype(p_dtype) ||
      (t_dtype != SAST_DT_I64 && t_dtype != SAST_DT_I32))
    return SAST_EINVAL;
  const sast::EnColumns src{x, y, p, t, x_dtype, y_dtype, p_dtype, t_dtype};
  return sast::en_launch<sast::Evt3Format>(src, counts, chunk_events, S, reset, state, ws, words, max_words, n_words, err, stream);
}

int sast_evt3enc_encode_dat(const void* records, const int64_t* counts, int64_t chunk_events, int S, const uint8_t* reset, int64_t* state,
                         void* ws, void* words, int64_t max_words, int64_t* n_words, int32_t* err, sast_stream_t stream) {
  SAST_ENTRY();
  if (!records || ((uintptr_t)records & 7) || !sast::en_args_ok(counts, chunk_events, S, state, ws, words, max_words, n_words, err, 2))
    return SAST_EINVAL;
  const sast::EnRecords src{static_cast<const uint2*>(records)};
  return sast::en_launch<sast::Evt3Format>(src, counts, chunk_events, S, reset, state, ws, words, max_words, n_words, err, stream);
}

}  // extern "C"
