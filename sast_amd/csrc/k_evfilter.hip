// Event noise filters on the device: the background-activity filter and the spatio-temporal-contrast filter (sast_evfilter_*; the rule:
// include/sast_hip.h, restated line by line by tests/event_filter_model.py).
//
// The decision for an event depends only on which EVENTS came before it at a handful of pixels, never on earlier decisions, so a
// whole chunk is decided at once:
//   launch 1  every workgroup takes its piece of the row's slots and writes the largest raw time of its events into ws; the workgroups
//             of a row whose reset flag is set sweep that row's surface to -1 (no other row's surface is touched).
//   launch 2  every workgroup folds the maxima of the pieces in front of it onto the row's carry, scans its piece (the running maximum:
//             the corrected times t') and writes, per slot, the value 2 * t' + pbit and the key (row * H * W + pixel) << index_bits |
//             flat index; a slot without an event inside the sensor gets the key S * H * W << index_bits | flat index.
//   the sort  rocprim's device radix sort of the S * chunk_capacity unique keys (fixed size, pre-sized storage).
//   launch 3  one thread per event: the predecessor at pixel q is the largest sorted key below (q's key, own index) if it is q's, else
//             the surface from before the call.  Keep flags, and the kept events of every piece.
//   launch 4  every workgroup folds the kept counts in front of it, scans its flags and scatters its kept events in order; the last key
//             of each pixel's run in the sorted keys writes the surface; the row's last workgroup writes out_counts, t_last, seen, kept.
// A workgroup reads only what an earlier launch wrote.  Every index is formed from device-read counts clamped to their capacities;
// keys of events carry a pixel inside the sensor by construction, so every surface index is below S * H * W.  Integers only.
#include <rocprim/device/device_radix_sort.hpp>
#include "evt_enc.cuh"

namespace sast {
namespace {

constexpr int EF_THREADS = EN_THREADS;
constexpr int EF_PER_THREAD = EN_PER_THREAD;
constexpr int EF_BLOCK_EVENTS = EF_THREADS * EF_PER_THREAD;
constexpr int EF_MAX_BLOCKS = 256;
static_assert(SAST_EVFILTER_BLOCK_EVENTS == EF_BLOCK_EVENTS && SAST_EVFILTER_MAX_BLOCKS == EF_MAX_BLOCKS, "the header states the sizes");
static_assert(EF_MAX_BLOCKS <= EF_THREADS, "the summaries of a row are folded one per thread");

using u64 = unsigned long long;

struct EfGeom {
  long long cap, N, HW;            // slots of a row, of the call (S * cap), pixels of a sensor
  int S, H, W, shift;              // shift: the bits of a flat index
  u64 idx_mask, pad_top;           // pad_top = S * HW: the key's upper part of a slot without an event inside the sensor
  int mode, radius;
  long long thr;
};

struct EfWs {
  u64 *keys, *sorted;              // [N]
  long long* val;                  // [N] 2 * t' + pbit
  long long *pmax, *pcnt;          // [S, EF_MAX_BLOCKS] per workgroup: the largest raw time, the kept events
  unsigned char* flag;             // [N]
  void* sort;
  size_t sort_bytes;
};

__device__ __forceinline__ void ef_xyp(const EnColumns& c, long long i, long long* x, long long* y, long long* p) {
  *x = en_ld(c.x, c.xd, i);
  *y = en_ld(c.y, c.yd, i);
  *p = en_ld(c.p, c.pd, i);
}
__device__ __forceinline__ void ef_xyp(const EnRecords& c, long long i, long long* x, long long* y, long long* p) {
  const unsigned w = c.r[i].y;
  *x = (long long)(w & 16383u);
  *y = (long long)((w >> 14) & 16383u);
  *p = (long long)((w >> 28) & 1u);
}
__device__ __forceinline__ long long ef_pol(const EnColumns& c, long long i) { return en_ld(c.p, c.pd, i); }
__device__ __forceinline__ long long ef_pol(const EnRecords& c, long long i) { return (long long)((c.r[i].y >> 28) & 1u); }

// the row's event count and this workgroup's piece [lo, hi) of the row's SLOTS: every slot of the call belongs to one piece
__device__ __forceinline__ long long ef_piece(const EnIn& in, int s, long long* lo, long long* hi) {
  const long long cap = in.chunk_events;
  const long long per = ((cap + gridDim.x - 1) / gridDim.x + EF_PER_THREAD - 1) / EF_PER_THREAD * EF_PER_THREAD;
  *lo = min((long long)blockIdx.x * per, cap);
  *hi = min(*lo + per, cap);
  return min(max(in.counts[s], 0LL), cap);
}

// launch 1
template <class Src>
__global__ __launch_bounds__(EF_THREADS) void evfilter_max_kernel(Src src, EnIn in, EfGeom g, long long* surface, long long* pmax) {
  __shared__ long long sm[EF_THREADS / 64];
  const int s = blockIdx.y;
  long long lo, hi;
  const long long n = ef_piece(in, s, &lo, &hi);
  const long long row0 = (long long)s * g.cap, end = min(hi, n);
  long long m = LLONG_MIN;
  for (long long i = lo + threadIdx.x; i < end; i += EF_THREADS) m = max(m, en_time(src, row0 + i));
  long long all;
  en_scan<true>(m, sm, &all);
  if (threadIdx.x == 0) pmax[(size_t)s * EF_MAX_BLOCKS + blockIdx.x] = all;
  if (in.reset && in.reset[s]) {
    long long* row = surface + (size_t)s * g.HW;
    for (long long q = (long long)blockIdx.x * EF_THREADS + threadIdx.x; q < g.HW; q += (long long)gridDim.x * EF_THREADS) row[q] = -1;
  }
}

// launch 2
template <class Src>
__global__ __launch_bounds__(EF_THREADS) void evfilter_key_kernel(Src src, EnIn in, EfGeom g, const long long* t_last, EfWs w, int* err) {
  __shared__ long long sm[EF_THREADS / 64];
  const int s = blockIdx.y;
  long long lo, hi;
  const long long n = ef_piece(in, s, &lo, &hi);
  const long long row0 = (long long)s * g.cap;
  long long carry = (in.reset && in.reset[s]) ? 0LL : max(t_last[s], 0LL), front;
  en_scan<true>(threadIdx.x < blockIdx.x ? w.pmax[(size_t)s * EF_MAX_BLOCKS + threadIdx.x] : LLONG_MIN, sm, &front);
  carry = max(carry, front);
  long long outside = 0;
  for (long long b0 = lo; b0 < hi; b0 += EF_BLOCK_EVENTS) {
    const long long i0 = b0 + (long long)threadIdx.x * EF_PER_THREAD;
    long long raw[EF_PER_THREAD], m = LLONG_MIN;
#pragma unroll
    for (int k = 0; k < EF_PER_THREAD; ++k) {
      const long long i = i0 + k;
      raw[k] = (i < hi && i < n) ? en_time(src, row0 + i) : LLONG_MIN;
      m = max(m, raw[k]);
    }
    long long all;
    long long run = max(carry, en_scan<true>(m, sm, &all));
#pragma unroll
    for (int k = 0; k < EF_PER_THREAD; ++k) {
      const long long i = i0 + k;
      if (i >= hi) break;
      const long long flat = row0 + i;
      u64 key = (g.pad_top << g.shift) | (u64)flat;
      long long v = 0;
      if (i < n) {
        run = max(run, raw[k]);
        long long x, y, p;
        ef_xyp(src, flat, &x, &y, &p);
        if (x >= 0 && x < g.W && y >= 0 && y < g.H) {
          key = ((u64)((long long)s * g.HW + y * g.W + x) << g.shift) | (u64)flat;
          v = 2 * run + (p > 0 ? 1 : 0);
        } else {
          ++outside;
        }
      }
      w.keys[flat] = key;
      w.val[flat] = v;
    }
    carry = max(carry, all);
  }
  long long total;
  en_scan<false>(outside, sm, &total);
  if (threadIdx.x == 0 && total > 0) atomicAdd(err, en_sat(total));
}

// the surface value at pixel key pk (row * HW + pixel) as the events in front of the event `flat` left it
__device__ __forceinline__ long long ef_prev(const EfGeom& g, const EfWs& w, const long long* surface, u64 pk, long long flat) {
  const u64 target = (pk << g.shift) | (u64)flat;
  long long a = 0, b = g.N;                                       // the first position whose key is >= target
  while (a < b) {
    const long long mid = (a + b) >> 1;
    if (w.sorted[mid] < target) a = mid + 1; else b = mid;
  }
  if (a > 0) {
    const u64 k = w.sorted[a - 1];
    if ((k >> g.shift) == pk) return w.val[k & g.idx_mask];
  }
  return surface[pk];
}

// launch 3
__global__ __launch_bounds__(EF_THREADS) void evfilter_decide_kernel(EnIn in, EfGeom g, const long long* surface, EfWs w) {
  __shared__ long long sm[EF_THREADS / 64];
  const int s = blockIdx.y;
  long long lo, hi;
  const long long n = ef_piece(in, s, &lo, &hi);
  const long long row0 = (long long)s * g.cap, end = min(hi, n);
  const u64 base = (u64)((long long)s * g.HW);
  long long cnt = 0;
  for (long long i = lo + threadIdx.x; i < end; i += EF_THREADS) {
    const long long flat = row0 + i;
    const u64 top = w.keys[flat] >> g.shift;
    int keep = 0;
    if (top < g.pad_top) {
      const long long v = w.val[flat], tq = v >> 1;
      if (g.mode == SAST_EVFILTER_CONTRAST) {
        const long long u = ef_prev(g, w, surface, top, flat);
        keep = u >= 0 && (u & 1) == (v & 1) && tq - (u >> 1) <= g.thr;
      } else {
        const int pix = (int)(top - base), y = pix / g.W, x = pix - y * g.W;
        const int y0 = max(y - g.radius, 0), y1 = min(y + g.radius, g.H - 1), x0 = max(x - g.radius, 0), x1 = min(x + g.radius, g.W - 1);
        for (int qy = y0; qy <= y1 && !keep; ++qy)
          for (int qx = x0; qx <= x1; ++qx) {
            if (qy == y && qx == x) continue;
            const long long u = ef_prev(g, w, surface, base + (u64)(qy * g.W + qx), flat);
            if (u >= 0 && tq - (u >> 1) <= g.thr) {
              keep = 1;
              break;
            }
          }
      }
    }
    w.flag[flat] = (unsigned char)keep;
    cnt += keep;
  }
  long long all;
  en_scan<false>(cnt, sm, &all);
  if (threadIdx.x == 0) w.pcnt[(size_t)s * EF_MAX_BLOCKS + blockIdx.x] = all;
}

__device__ __forceinline__ short ef_i16(long long v) { return (short)min(max(v, -32768LL), 32767LL); }

// launch 4
template <class Src>
__global__ __launch_bounds__(EF_THREADS) void evfilter_emit_kernel(Src src, EnIn in, EfGeom g, SastEvFilterArgs f, EfWs w) {
  __shared__ long long sm[EF_THREADS / 64];
  const int s = blockIdx.y;
  long long lo, hi;
  const long long n = ef_piece(in, s, &lo, &hi);
  const long long row0 = (long long)s * g.cap, out0 = (long long)s * f.out_capacity;
  const bool mine = threadIdx.x < gridDim.x;
  const size_t slot = (size_t)s * EF_MAX_BLOCKS + (mine ? threadIdx.x : 0);
  long long front, total, tmax;
  en_scan<false>(mine && threadIdx.x < blockIdx.x ? w.pcnt[slot] : 0LL, sm, &front);
  en_scan<false>(mine ? w.pcnt[slot] : 0LL, sm, &total);
  en_scan<true>(mine ? w.pmax[slot] : LLONG_MIN, sm, &tmax);
  const u64 base = (u64)((long long)s * g.HW);
  for (long long b0 = lo; b0 < hi; b0 += EF_BLOCK_EVENTS) {
    const long long i0 = b0 + (long long)threadIdx.x * EF_PER_THREAD;
    int fl[EF_PER_THREAD];
    long long cnt = 0;
#pragma unroll
    for (int k = 0; k < EF_PER_THREAD; ++k) {
      const long long i = i0 + k;
      fl[k] = (i < hi && i < n) ? w.flag[row0 + i] : 0;
      cnt += fl[k];
    }
    long long step;
    long long pos = front + en_scan<false>(cnt, sm, &step);
#pragma unroll
    for (int k = 0; k < EF_PER_THREAD; ++k) {
      const long long i = i0 + k;
      if (i >= hi) break;
      const long long flat = row0 + i;
      if (fl[k]) {
        if (pos < f.out_capacity) {
          const int pix = (int)((w.keys[flat] >> g.shift) - base), y = pix / g.W;
          f.x[out0 + pos] = (short)(pix - y * g.W);
          f.y[out0 + pos] = (short)y;
          f.p[out0 + pos] = ef_i16(ef_pol(src, flat));
          f.t[out0 + pos] = w.val[flat] >> 1;
        }
        ++pos;
      }
      // the sorted key at this slot's position: the last one of a pixel's run is the pixel's last event by arrival order
      const u64 key = w.sorted[flat], top = key >> g.shift;
      if (top < g.pad_top && (flat == g.N - 1 || (w.sorted[flat + 1] >> g.shift) != top)) f.surface[top] = w.val[key & g.idx_mask];
    }
    front += step;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    const bool rst = in.reset && in.reset[s];
    f.out_counts[s] = total;
    f.t_last[s] = max(rst ? 0LL : max(f.t_last[s], 0LL), tmax);
    f.seen[s] = (rst ? 0LL : f.seen[s]) + n;
    f.kept[s] = (rst ? 0LL : f.kept[s]) + total;
  }
}

int ef_bits(u64 v) {
  int b = 0;
  while (v) {
    ++b;
    v >>= 1;
  }
  return b;
}

// the geometry of a call; false: a shape the filter does not take
bool ef_geom(int S, int64_t cap, int H, int W, EfGeom* g) {
  if (S < 1 || S > 65535 || H < 1 || H > 32767 || W < 1 || W > 32767 || cap < 0 || cap > INT_MAX / S) return false;
  g->S = S; g->H = H; g->W = W;
  g->cap = cap;
  g->N = (long long)S * cap;
  g->HW = (long long)H * W;
  g->shift = std::max(ef_bits(g->N > 0 ? (u64)(g->N - 1) : 0), 1);
  g->idx_mask = (1ull << g->shift) - 1;
  g->pad_top = (u64)S * (u64)g->HW;
  return ef_bits(g->pad_top) + g->shift <= 63;
}

size_t ef_align(size_t v) { return (v + 255) & ~(size_t)255; }

// only the bits a key can have are sorted
unsigned ef_end_bit(const EfGeom& g) { return (unsigned)(g.shift + ef_bits(g.pad_top)); }

// the sort's own storage for the call's keys; false: rocprim refused
bool ef_sort_bytes(const EfGeom& g, size_t* bytes) {
  *bytes = 0;
  if (g.N == 0) return true;
  u64* p = nullptr;
  return rocprim::radix_sort_keys(nullptr, *bytes, p, p, (size_t)g.N, 0, ef_end_bit(g), (hipStream_t) nullptr) == hipSuccess;
}

// the workspace carved; returns its size (base may be null: the size alone)
size_t ef_carve(void* base, const EfGeom& g, size_t sort_bytes, EfWs* w) {
  char* p = static_cast<char*>(base);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* q = p ? p + at : nullptr;
    at += ef_align(bytes);
    return q;
  };
  const size_t N = (size_t)g.N;
  w->keys = reinterpret_cast<u64*>(take(N * 8));
  w->sorted = reinterpret_cast<u64*>(take(N * 8));
  w->val = reinterpret_cast<long long*>(take(N * 8));
  w->pmax = reinterpret_cast<long long*>(take((size_t)g.S * EF_MAX_BLOCKS * 8));
  w->pcnt = reinterpret_cast<long long*>(take((size_t)g.S * EF_MAX_BLOCKS * 8));
  w->flag = reinterpret_cast<unsigned char*>(take(N));
  w->sort = take(std::max<size_t>(sort_bytes, 16));
  w->sort_bytes = sort_bytes;
  return at;
}

template <class Src>
int ef_apply(const SastEvFilterArgs* f, const Src& src, const int64_t* counts, int64_t cap, const uint8_t* reset, sast_stream_t stream) {
  EfGeom g;
  if (!f || !counts || !f->surface || !f->t_last || !f->seen || !f->kept || !f->err || !f->ws || !f->x || !f->y || !f->p || !f->t ||
      !f->out_counts || !ef_geom(f->S, cap, f->height, f->width, &g))
    return SAST_EINVAL;
  if (((uintptr_t)f->ws & 7) || f->out_capacity < cap || f->out_capacity < 1 || f->out_capacity > INT_MAX / f->S ||
      (f->mode != SAST_EVFILTER_ACTIVITY && f->mode != SAST_EVFILTER_CONTRAST) || f->radius < 1 || f->radius > 3 || f->threshold_us < 0 ||
      f->threshold_us >= (1ll << 62))
    return SAST_EINVAL;
  g.mode = f->mode;
  g.radius = f->radius;
  g.thr = f->threshold_us;
  size_t sort_bytes;
  EfWs w;
  if (!ef_sort_bytes(g, &sort_bytes) || f->ws_bytes < ef_carve(f->ws, g, sort_bytes, &w)) return SAST_EINVAL;
  const EnIn in{reinterpret_cast<const long long*>(counts), (long long)cap, reinterpret_cast<const unsigned char*>(reset)};
  const long long per = (cap + EF_BLOCK_EVENTS - 1) / EF_BLOCK_EVENTS;
  const dim3 grid((unsigned)std::min<long long>(std::max<long long>(per, 1), EF_MAX_BLOCKS), (unsigned)g.S);
  hipStream_t st = (hipStream_t)stream;
  long long* surface = reinterpret_cast<long long*>(f->surface);
  SAST_LAUNCH((evfilter_max_kernel<Src>), grid, dim3(EF_THREADS), 0, st, src, in, g, surface, w.pmax);
  SAST_LAUNCH((evfilter_key_kernel<Src>), grid, dim3(EF_THREADS), 0, st, src, in, g, reinterpret_cast<const long long*>(f->t_last), w, f->err);
  if (g.N > 0) {
    // unique keys: the sorted order is the arrival order inside every pixel's run
    size_t bytes = std::max<size_t>(sort_bytes, 16);
    if (rocprim::radix_sort_keys(w.sort, bytes, (const u64*)w.keys, w.sorted, (size_t)g.N, 0, ef_end_bit(g), st) !=
        hipSuccess)
      return SAST_ELAUNCH;
  }
  SAST_LAUNCH(evfilter_decide_kernel, grid, dim3(EF_THREADS), 0, st, in, g, (const long long*)surface, w);
  SAST_LAUNCH((evfilter_emit_kernel<Src>), grid, dim3(EF_THREADS), 0, st, src, in, g, *f, w);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // namespace
}  // namespace sast

extern "C" {

size_t sast_evfilter_ws_bytes(int S, int64_t chunk_capacity, int height, int width) {
  sast::EfGeom g;
  sast::EfWs w;
  size_t sort_bytes;
  if (!sast::ef_geom(S, chunk_capacity, height, width, &g) || !sast::ef_sort_bytes(g, &sort_bytes)) return 0;
  return sast::ef_carve(nullptr, g, sort_bytes, &w);
}

int sast_evfilter_apply(const SastEvFilterArgs* f, const void* x, const void* y, const void* p, const void* t, int x_dtype, int y_dtype,
                        int p_dtype, int t_dtype, const int64_t* counts, int64_t chunk_capacity, const uint8_t* reset,
                        sast_stream_t stream) {
  SAST_ENTRY();
  if (!x || !y || !p || !t || !sast::en_int_dtype(x_dtype) || !sast::en_int_dtype(y_dtype) || !sast::en_int_dtype(p_dtype) ||
      (t_dtype != SAST_DT_I64 && t_dtype != SAST_DT_I32))
    return SAST_EINVAL;
  const sast::EnColumns src{x, y, p, t, x_dtype, y_dtype, p_dtype, t_dtype};
  return sast::ef_apply(f, src, counts, chunk_capacity, reset, stream);
}

int sast_evfilter_apply_dat(const SastEvFilterArgs* f, const void* records, const int64_t* counts, int64_t chunk_capacity,
                            const uint8_t* reset, sast_stream_t stream) {
  SAST_ENTRY();
  if (!records || ((uintptr_t)records & 7)) return SAST_EINVAL;
  const sast::EnRecords src{static_cast<const uint2*>(records)};
  return sast::ef_apply(f, src, counts, chunk_capacity, reset, stream);
}

}  // extern "C"
