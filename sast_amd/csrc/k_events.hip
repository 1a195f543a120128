// Raw events (x, y, p, t) -> stacked-histogram frames on the device.
//
// Reference: StackedHistogram.construct (data/utils/representations.py:37-121) and the reader / windowing / downsampling of the offline
// script around it (scripts/genx/preprocess_dataset.py:159-177 time correction and polarity clip, :463-473 nearest-exact downsampling
// by 2, :507-530 window bounds).  Entry points:
//   sast_evstreams_correct_time   S recordings side by side ([S, capacity] buffers, one count / carry per row): per row the running
//                                 maximum of the timestamps with a carry in device memory (two passes over a fixed block count)
//   sast_evstreams_window_bounds  per window two binary searches (duration mode) or one (count mode) inside its row -> int64 [T * S, 2]
//                                 event ranges that index the flattened buffer
//   sast_event_correct_time / sast_event_window_bounds   one recording: the same kernels with S = 1
//   sast_event_frames         the histogram: bucket each window's events by 32-column spatial tile (count -> scan -> scatter of packed
//                             records), then one workgroup per (window, tile) counts its records in LDS and writes the finished uint8 tile
//   sast_mdstack_frames       the mixed-density event stack (MixedDensityEventStack, representations.py:130-218) on the same windows:
//                             the same driver and bucketing passes with the bin taken from the logarithm of the event's age, then one
//                             workgroup per (window, tile) sums the signed polarities per (pixel, bin) in LDS, takes the prefix sum
//                             over the bins and writes the finished int8 tile
// Integer counts do not depend on arrival order: the frames are bitwise reproducible.  Every per-frame size (event count, window
// bounds, carry) is read on the device; the grids are sized from capacities, so a captured graph replays on new events.
#include <climits>
#include "common.cuh"
#include "kernels.h"

namespace sast {
namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_TILE_W = 32;          // tile columns; a record keeps the pixel in 10 bits (tile rows x 32 <= 1024)
constexpr int EV_LDS_WORDS = 20480;    // u32 counters of one (window, tile) workgroup: 80 KiB (32 x 32 px x 20 channels)
constexpr int EV_MAX_TILES = 8192;     // tiles per window: the LDS tile histogram of the bucketing kernels (32 KiB)
constexpr int EV_MAX_CHANNELS = 640;   // 2 * bins: the channel of a record is 10 bits, and one tile row must fit EV_LDS_WORDS
constexpr int EV_MD_MAX_BINS = 512;    // mixed density: the record's channel field holds 2 * bin + polarity
constexpr int EV_EVENTS_PER_BLOCK = 8192;
constexpr int EV_MAX_BLOCKS = 1024;    // bucketing workgroups per window

struct EvGeom {
  int H, W;            // sensor size: events outside it are invalid
  int Ho, Wo;          // frame size (H/2, W/2 with downsample_by_2)
  int bins, C;         // C = 2 * bins channels (mixed density: C = bins)
  int th;              // tile rows
  int tiles_x, tiles;  // tiles per frame row / per frame
  int cutoff, fast, ds, clip_pol;
};

// what the frame kernels read of SastEventArgs / SastMdStackArgs: the fields the two public structs share under the same names
struct EvIn {
  const void *x, *y, *p, *t;
  const int64_t* bounds;
  void* out;           // uint8 (histogram) or int8 (mixed density) frames
  int32_t* err;
  int64_t capacity, window_capacity;
  int32_t x_dtype, y_dtype, p_dtype, t_dtype;
  int32_t B;
};

__device__ __forceinline__ long long ld_int(const void* p, int dt, long long i) {
  if (dt == SAST_DT_I64) return static_cast<const long long*>(p)[i];
  if (dt == SAST_DT_I32) return static_cast<const int*>(p)[i];
  return static_cast<const short*>(p)[i];
}

struct EvWindow {
  long long s, e;      // event range [s, e)
  long long t0;
  float span;          // max(t1 - t0, 1) as the reference's int64 / int division sees it: converted to fp32
};

__device__ __forceinline__ EvWindow ev_window(const EvIn& a, int b) {
  EvWindow w;
  w.s = max(a.bounds[2 * b], 0LL);
  w.e = min(a.bounds[2 * b + 1], (long long)a.capacity);
  w.t0 = 0;
  w.span = 1.0f;
  if (w.e > w.s) {
    w.t0 = ld_int(a.t, a.t_dtype, w.s);
    const long long t1 = ld_int(a.t, a.t_dtype, w.e - 1);
    w.span = (float)max(t1 - w.t0, 1LL);
  }
  return w;
}

// MixedDensityEventStack.construct (representations.py:193-208): t_norm = (t - t0) / max(t1 - t0, 1) in fp32 as above, clamped to
// [1e-6, 1 - 1e-6] (the scalars rounded to fp32), bin = floor(max(bins - log(t_norm) / log(1/2), 0)) = max(bins + floor(log2(t_norm)), 0).
// floor(log2) of a normal fp32 is its exponent field: no logarithm, and no libm whose last bit could decide a bin boundary.
__device__ __forceinline__ int md_bin(long long dt, float span, int bins) {
  float q = __fdiv_rn((float)dt, span);
  q = fminf(fmaxf(q, 1e-6f), (float)(1.0 - 1e-6));
  return max(bins + (int)((__float_as_uint(q) >> 23) & 255u) - 127, 0);     // q < 1: the bin is at most bins - 1
}

// >0: a record (tile in *tile, packed pixel | channel << 10 in *rec);  0: dropped by the downsampling;  <0: an invalid event.
// MD: the mixed-density record, channel field = 2 * bin + polarity
template <bool MD>
__device__ __forceinline__ int ev_record(const EvIn& a, const EvGeom& g, const EvWindow& w, long long i, int* tile,
                                         unsigned* rec) {
  const long long x = ld_int(a.x, a.x_dtype, i), y = ld_int(a.y, a.y_dtype, i);
  long long p = ld_int(a.p, a.p_dtype, i);
  const long long dt = ld_int(a.t, a.t_dtype, i) - w.t0;
  if (p < 0 && g.clip_pol) p = 0;                       // preprocess_dataset.py:177 np.clip(p, a_min=0)
  if (x < 0 || x >= g.W || y < 0 || y >= g.H || p < 0 || p > 1 || dt < 0) return -1;
  int ox = (int)x, oy = (int)y;
  if (g.ds) {                                            // nearest-exact at scale 0.5: output (i, j) is input (2i+1, 2j+1)
    if (!(ox & 1) || !(oy & 1)) return 0;
    ox >>= 1;
    oy >>= 1;
    if (ox >= g.Wo || oy >= g.Ho) return 0;
  }
  int ch;
  if constexpr (MD) {
    ch = 2 * md_bin(dt, w.span, g.bins) + (int)p;
  } else {
    // representations.py:98-104: (t - t0) / max(t1 - t0, 1) is int64 / int64 true division in fp32 (both operands rounded to fp32,
    // one correctly rounded divide), then * bins, floor, clamp(max = bins - 1)
    const float q = __fdiv_rn((float)dt, w.span) * (float)g.bins;
    ch = (int)p * g.bins + min((int)floorf(q), g.bins - 1);
  }
  const int ty = oy / g.th, tx = ox / EV_TILE_W;
  *tile = ty * g.tiles_x + tx;
  *rec = (unsigned)((oy - ty * g.th) * EV_TILE_W + (ox - tx * EV_TILE_W)) | ((unsigned)ch << 10);
  return 1;
}

// the share of window b's events that bucketing workgroup blockIdx.x handles
__device__ __forceinline__ bool ev_chunk(const EvWindow& w, long long* lo, long long* hi) {
  const long long len = w.e - w.s;
  const long long chunk = (len + gridDim.x - 1) / gridDim.x;
  *lo = w.s + blockIdx.x * chunk;
  *hi = min(*lo + chunk, w.e);
  return *lo < *hi;
}

// windows may overlap (count mode, or ends closer than the duration): an invalid event is reported by the first window that holds it
__device__ __forceinline__ bool ev_in_earlier_window(const EvIn& a, int b, long long i) {
  for (int k = 0; k < b; ++k)
    if (i >= max(a.bounds[2 * k], 0LL) && i < min(a.bounds[2 * k + 1], (long long)a.capacity)) return true;
  return false;
}

// pass 1: events per (window, tile) into tile_cnt (zero on entry; the scan clears it again); invalid events into err[0], each once
template <bool MD>
__global__ __launch_bounds__(EV_THREADS) void ev_count_kernel(EvIn a, EvGeom g, int* tile_cnt) {
  extern __shared__ __attribute__((aligned(16))) int hist[];
  __shared__ int s_bad;
  const int b = blockIdx.y;
  const EvWindow w = ev_window(a, b);
  long long lo, hi;
  if (!ev_chunk(w, &lo, &hi)) return;
  for (int k = threadIdx.x; k < g.tiles; k += EV_THREADS) hist[k] = 0;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  int bad = 0;
  for (long long i = lo + threadIdx.x; i < hi; i += EV_THREADS) {
    int tile;
    unsigned rec;
    const int r = ev_record<MD>(a, g, w, i, &tile, &rec);
    if (r > 0) atomicAdd(&hist[tile], 1);
    else if (r < 0 && !ev_in_earlier_window(a, b, i)) ++bad;
  }
  if (bad) atomicAdd(&s_bad, bad);
  __syncthreads();
  for (int k = threadIdx.x; k < g.tiles; k += EV_THREADS)
    if (hist[k]) atomicAdd(&tile_cnt[(size_t)b * g.tiles + k], hist[k]);
  if (threadIdx.x == 0 && s_bad) atomicAdd(&a.err[0], s_bad);
}

// pass 2, one workgroup per window: exclusive scan of the tile counts -> off[b][0..tiles] and the scatter cursors; clears tile_cnt.
// A window with more events than window_capacity is left empty (all-zero frame) and counted in err[1].
__global__ __launch_bounds__(EV_THREADS) void ev_scan_kernel(EvIn a, EvGeom g, int* tile_cnt, int* off, int* cursor, int* ovf) {
  __shared__ long long part[EV_THREADS];
  const int b = blockIdx.x, T = g.tiles;
  int* cnt = tile_cnt + (size_t)b * T;
  int* o = off + (size_t)b * (T + 1);
  int* cur = cursor + (size_t)b * T;
  const int per = (T + EV_THREADS - 1) / EV_THREADS;
  const int k0 = min(threadIdx.x * per, T), k1 = min(k0 + per, T);
  long long sum = 0;
  for (int k = k0; k < k1; ++k) sum += cnt[k];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < EV_THREADS; d <<= 1) {           // inclusive Hillis-Steele scan of the per-thread sums
    const long long v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  const long long total = part[EV_THREADS - 1];
  const bool over = total > a.window_capacity;
  long long run = part[threadIdx.x] - sum;
  for (int k = k0; k < k1; ++k) {
    const int c = cnt[k];
    o[k] = over ? 0 : (int)run;
    cur[k] = over ? 0 : (int)run;
    run += c;
    cnt[k] = 0;
  }
  if (threadIdx.x == 0) {
    o[T] = over ? 0 : (int)total;
    ovf[b] = over ? 1 : 0;
    if (over) atomicAdd(&a.err[1], 1);
  }
}

// pass 3: the same events again; each workgroup reserves one range per tile (one global atomic per (workgroup, tile)), then places
// its records there through LDS cursors
template <bool MD>
__global__ __launch_bounds__(EV_THREADS) void ev_scatter_kernel(EvIn a, EvGeom g, int* cursor, const int* ovf, unsigned* recs) {
  extern __shared__ __attribute__((aligned(16))) int hist[];
  const int b = blockIdx.y;
  if (ovf[b]) return;
  const EvWindow w = ev_window(a, b);
  long long lo, hi;
  if (!ev_chunk(w, &lo, &hi)) return;
  for (int k = threadIdx.x; k < g.tiles; k += EV_THREADS) hist[k] = 0;
  __syncthreads();
  for (long long i = lo + threadIdx.x; i < hi; i += EV_THREADS) {
    int tile;
    unsigned rec;
    if (ev_record<MD>(a, g, w, i, &tile, &rec) > 0) atomicAdd(&hist[tile], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < g.tiles; k += EV_THREADS)
    if (hist[k]) hist[k] = atomicAdd(&cursor[(size_t)b * g.tiles + k], hist[k]);
  __syncthreads();
  unsigned* wr = recs + (size_t)b * (size_t)a.window_capacity;
  for (long long i = lo + threadIdx.x; i < hi; i += EV_THREADS) {
    int tile;
    unsigned rec;
    if (ev_record<MD>(a, g, w, i, &tile, &rec) > 0) {
      const int pos = atomicAdd(&hist[tile], 1);
      if (pos < a.window_capacity) wr[pos] = rec;
    }
  }
}

// representations.py:115-118: fastmode accumulates in uint8 (wraps mod 256), otherwise in int16 (wraps to negative above 32767);
// then clamp(0, count_cutoff)
__device__ __forceinline__ unsigned char ev_finish(unsigned v, int cutoff, int fast) {
  if (fast) return (unsigned char)min((int)(v & 255u), cutoff);
  const int s = (short)(unsigned short)(v & 0xffffu);
  return (unsigned char)min(max(s, 0), cutoff);
}

// pass 4, one workgroup per (tile, window): u32 counters of the tile's th x 32 pixels x C channels in LDS, then the finished uint8
// tile, every pixel of it written once (no clear of the output, no finishing pass)
__global__ __launch_bounds__(EV_THREADS) void ev_accum_kernel(EvIn a, EvGeom g, const int* off, const unsigned* recs) {
  extern __shared__ __attribute__((aligned(16))) unsigned cnt[];
  const int t = blockIdx.x, b = blockIdx.y;
  const int px = g.th * EV_TILE_W, n = px * g.C;
  for (int k = threadIdx.x; k < n; k += EV_THREADS) cnt[k] = 0;
  __syncthreads();
  const int* o = off + (size_t)b * (g.tiles + 1);
  const int beg = o[t], end = min(o[t + 1], (int)min(a.window_capacity, (long long)INT_MAX));
  const unsigned* rd = recs + (size_t)b * (size_t)a.window_capacity;
  for (int i = beg + threadIdx.x; i < end; i += EV_THREADS) {
    const unsigned r = rd[i];
    const unsigned k = (r >> 10) * px + (r & 1023u);
    if (k < (unsigned)n) atomicAdd(&cnt[k], 1u);
  }
  __syncthreads();
  const int oy0 = (t / g.tiles_x) * g.th, ox0 = (t % g.tiles_x) * EV_TILE_W;
  unsigned char* out = static_cast<unsigned char*>(a.out);
  for (int k = threadIdx.x; k < n; k += EV_THREADS) {
    const int c = k / px, l = k - c * px;
    const int oy = oy0 + l / EV_TILE_W, ox = ox0 + (l % EV_TILE_W);
    if (oy < g.Ho && ox < g.Wo)
      out[(((size_t)b * g.C + c) * g.Ho + oy) * g.Wo + ox] = ev_finish(cnt[k], g.cutoff, g.fast);
  }
}

// representations.py:210-217: the sums wrap as int8 (put_ accumulates in int8, the channel sums are stored back to int8), then
// clamp(-count_cutoff, count_cutoff) unless the cutoff is None (< 0 here)
__device__ __forceinline__ signed char md_finish(int v, int cutoff) {
  int s = (signed char)(unsigned char)(v & 255);
  if (cutoff >= 0) s = min(max(s, -cutoff), cutoff);
  return (signed char)s;
}

// pass 4 of the mixed-density stack, one workgroup per (tile, window): signed counters of the tile's th x 32 pixels x bins in LDS
// (+1 / -1 per record), then per pixel the inclusive prefix sum over the bins (representations.py:124-127), every int8 of the tile
// written once (no clear of the output, no finishing pass)
__global__ __launch_bounds__(EV_THREADS) void md_accum_kernel(EvIn a, EvGeom g, const int* off, const unsigned* recs) {
  extern __shared__ __attribute__((aligned(16))) int scnt[];
  const int t = blockIdx.x, b = blockIdx.y;
  const int px = g.th * EV_TILE_W, n = px * g.C;
  for (int k = threadIdx.x; k < n; k += EV_THREADS) scnt[k] = 0;
  __syncthreads();
  const int* o = off + (size_t)b * (g.tiles + 1);
  const int beg = o[t], end = min(o[t + 1], (int)min(a.window_capacity, (long long)INT_MAX));
  const unsigned* rd = recs + (size_t)b * (size_t)a.window_capacity;
  for (int i = beg + threadIdx.x; i < end; i += EV_THREADS) {
    const unsigned r = rd[i];
    const unsigned ch = r >> 10;
    const unsigned k = (ch >> 1) * px + (r & 1023u);
    if (k < (unsigned)n) atomicAdd(&scnt[k], (ch & 1u) ? 1 : -1);
  }
  __syncthreads();
  const int oy0 = (t / g.tiles_x) * g.th, ox0 = (t % g.tiles_x) * EV_TILE_W;
  signed char* out = static_cast<signed char*>(a.out);
  for (int l = threadIdx.x; l < px; l += EV_THREADS) {
    const int oy = oy0 + l / EV_TILE_W, ox = ox0 + (l % EV_TILE_W);
    if (oy >= g.Ho || ox >= g.Wo) continue;
    int run = 0;
    for (int c = 0; c < g.C; ++c) {
      run += scnt[c * px + l];
      out[(((size_t)b * g.C + c) * g.Ho + oy) * g.Wo + ox] = md_finish(run, g.cutoff);
    }
  }
}

// ---- time correction (preprocess_dataset.py:159-168): t[i] = max(t[i], running max), the running max starting at the carry
constexpr int EV_SCAN_BLOCKS = SAST_EVENT_SCAN_BLOCKS;

__device__ __forceinline__ void ev_tchunk(long long n, long long* lo, long long* hi) {
  const long long chunk = (n + gridDim.x - 1) / gridDim.x;
  *lo = min((long long)blockIdx.x * chunk, n);
  *hi = min(*lo + chunk, n);
}

__device__ __forceinline__ long long block_max(long long v, long long* red) {
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
  const int wv = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wv] = v;
  __syncthreads();
  long long m = red[0];
  for (int k = 1; k < EV_THREADS / 64; ++k) m = max(m, red[k]);
  return m;
}

// one EV_THREADS-wide step of a running maximum: *v becomes max(*v, the values of the threads before it, carry); returns the carry out
// (the maximum of the whole step and the carry in).  Every thread of the workgroup calls it.
__device__ __forceinline__ long long block_max_scan(long long* v, long long carry, long long* wtot) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  long long m = *v;
  for (int d = 1; d < 64; d <<= 1) {                      // inclusive max-scan of the wave
    const long long u = __shfl_up(m, d);
    if (lane >= d) m = max(m, u);
  }
  __syncthreads();
  if (lane == 63) wtot[wv] = m;
  __syncthreads();
  long long pre = carry;
  for (int k = 0; k < wv; ++k) pre = max(pre, wtot[k]);
  *v = max(m, pre);
  for (int k = wv; k < EV_THREADS / 64; ++k) pre = max(pre, wtot[k]);
  return pre;
}

// Row blockIdx.y of the [S, cap] buffers is one recording with its own count, carry and windows; a single recording is S = 1.  Two
// passes with gridDim.x blocks per row: a row's partial maxima and its carry live in its own ws row (ws[s][0] = carry in,
// ws[s][1 + blk] = the maximum of block blk's chunk of row s), so no maximum is ever taken across rows.  The results are integer
// maxima: they do not depend on gridDim.x.
constexpr int EV_ROW_WS = EV_SCAN_BLOCKS + 1;
constexpr int EV_ROW_EVENTS_PER_BLOCK = 4096;

__global__ __launch_bounds__(EV_THREADS) void ev_tmax_partial_kernel(const void* t, int dt, const long long* counts, long long cap,
                                                                     const long long* t_last, const unsigned char* reset,
                                                                     long long* ws) {
  __shared__ long long red[EV_THREADS / 64];
  const int s = blockIdx.y;
  const long long n = min(max(counts[s], 0LL), cap), row = (long long)s * cap;
  long long lo, hi;
  ev_tchunk(n, &lo, &hi);
  long long m = LLONG_MIN;
  for (long long i = lo + threadIdx.x; i < hi; i += EV_THREADS) m = max(m, ld_int(t, dt, row + i));
  m = block_max(m, red);
  if (threadIdx.x == 0) {
    long long* w = ws + (size_t)s * EV_ROW_WS;
    w[1 + blockIdx.x] = m;
    if (blockIdx.x == 0) w[0] = (reset && reset[s]) ? 0LL : t_last[s];
  }
}

__global__ __launch_bounds__(EV_THREADS) void ev_tmax_apply_kernel(const void* t, int dt, const long long* counts, long long cap,
                                                                   const long long* ws_all, long long* t_out, long long* t_last) {
  __shared__ long long red[EV_THREADS / 64];
  __shared__ long long wtot[EV_THREADS / 64];
  const int s = blockIdx.y;
  const long long n = min(max(counts[s], 0LL), cap), row = (long long)s * cap;
  const long long* ws = ws_all + (size_t)s * EV_ROW_WS;
  long long lo, hi;
  ev_tchunk(n, &lo, &hi);
  long long carry = LLONG_MIN;
  for (int k = threadIdx.x; k < (int)blockIdx.x + 1; k += EV_THREADS) carry = max(carry, ws[k]);
  carry = block_max(carry, red);
  for (long long base = lo; base < hi; base += EV_THREADS) {
    const long long i = base + threadIdx.x;
    long long v = i < hi ? ld_int(t, dt, row + i) : LLONG_MIN;
    carry = block_max_scan(&v, carry, wtot);
    if (i < hi) t_out[row + i] = v;
  }
  // an empty row has only LLONG_MIN partials: t_last[s] = the carry in (0 after a reset)
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    long long m = ws[0];
    for (int k = 1; k <= (int)gridDim.x; ++k) m = max(m, ws[k]);
    t_last[s] = m;
  }
}

// ---- window bounds (preprocess_dataset.py:507-513): np.searchsorted over the corrected timestamps
__device__ __forceinline__ long long search(const long long* t, long long n, long long v, bool right) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (right ? t[mid] <= v : t[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// rows == nullptr: window w = k * S + s belongs to row s.  Otherwise window w = k * cols + b belongs to row rows[b] (int32 [cols], read
// on the device): several windows of one step may share a row; a row outside [0, S) gives the empty range [0, 0)
__global__ void ev_bounds_kernel(const long long* t, const long long* counts, int S, long long cap, const long long* ends, int B,
                                 int mode, long long value, long long* bounds, const int* rows, int cols) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;     // window k * S + s
  if (w >= B) return;
  const int s = rows ? rows[w % cols] : w % S;
  if (s < 0 || s >= S) {
    bounds[2 * w] = 0;
    bounds[2 * w + 1] = 0;
    return;
  }
  const long long n = min(max(counts[s], 0LL), cap), row = (long long)s * cap;
  const long long e = search(t + row, n, ends[w], true);
  const long long b = mode == SAST_EVENT_WINDOW_COUNT ? max(e - value, 0LL) : search(t + row, n, ends[w] - value, false);
  bounds[2 * w] = row + b;
  bounds[2 * w + 1] = row + e;
}

bool int_dtype(int dt) { return dt == SAST_DT_I64 || dt == SAST_DT_I32 || dt == SAST_DT_I16; }

// geometry of a call, or false for arguments the kernels do not take
bool ev_geom(int B, int bins, int height, int width, int ds, long long wcap, EvGeom* g, bool md = false) {
  if (B < 1 || B > 65535 || bins < 1 || height < 1 || width < 1 || wcap < 0 || wcap > INT_MAX) return false;
  if (md ? bins > EV_MD_MAX_BINS : 2 * bins > EV_MAX_CHANNELS) return false;
  g->H = height;
  g->W = width;
  g->Ho = ds ? height / 2 : height;
  g->Wo = ds ? width / 2 : width;
  if (g->Ho < 1 || g->Wo < 1) return false;
  g->bins = bins;
  g->C = md ? bins : 2 * bins;
  g->th = min(32, EV_LDS_WORDS / (EV_TILE_W * g->C));
  g->tiles_x = (g->Wo + EV_TILE_W - 1) / EV_TILE_W;
  const long long tiles = (long long)g->tiles_x * ((g->Ho + g->th - 1) / g->th);
  if (tiles > EV_MAX_TILES) return false;
  g->tiles = (int)tiles;
  g->ds = ds ? 1 : 0;
  return true;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct EvWs { int* tile_cnt; int* off; int* cursor; int* ovf; unsigned* recs; size_t bytes; };

EvWs ev_ws(void* base, int B, const EvGeom& g, long long wcap) {
  EvWs w;
  char* p = static_cast<char*>(base);
  size_t o = 0;
  w.tile_cnt = reinterpret_cast<int*>(p + o); o += align16(sizeof(int) * (size_t)B * g.tiles);
  w.off = reinterpret_cast<int*>(p + o);      o += align16(sizeof(int) * (size_t)B * (g.tiles + 1));
  w.cursor = reinterpret_cast<int*>(p + o);   o += align16(sizeof(int) * (size_t)B * g.tiles);
  w.ovf = reinterpret_cast<int*>(p + o);      o += align16(sizeof(int) * (size_t)B);
  w.recs = reinterpret_cast<unsigned*>(p + o); o += align16(sizeof(unsigned) * (size_t)B * (size_t)wcap);
  w.bytes = o;
  return w;
}

// the checked fields that SastEventArgs and SastMdStackArgs share, or false for arguments the kernels do not take
template <class Args>
bool ev_in(const Args* a, EvIn* in) {
  if (!a->x || !a->y || !a->p || !a->t || !a->bounds || !a->out || !a->err || !a->ws || a->capacity < 0 || a->capacity > INT_MAX)
    return false;
  if (!int_dtype(a->x_dtype) || !int_dtype(a->y_dtype) || !int_dtype(a->p_dtype) || (a->t_dtype != SAST_DT_I64 && a->t_dtype != SAST_DT_I32))
    return false;
  *in = EvIn{a->x, a->y, a->p, a->t, a->bounds, a->out, a->err, a->capacity, a->window_capacity,
             a->x_dtype, a->y_dtype, a->p_dtype, a->t_dtype, a->B};
  return true;
}

// sast_event_frames (MD = false) / sast_mdstack_frames: count -> scan -> scatter -> accumulate.  g arrives with cutoff, fast and
// clip_pol set by the entry point, which has checked its own cutoff range
template <bool MD, class Args>
int ev_frames(const Args* a, EvGeom g, sast_stream_t stream) {
  EvIn in;
  if (!ev_geom(a->B, a->bins, a->height, a->width, a->downsample_by_2, a->window_capacity, &g, MD) || !ev_in(a, &in)) return SAST_EINVAL;
  const EvWs w = ev_ws(a->ws, in.B, g, in.window_capacity);
  const void* accum = MD ? reinterpret_cast<const void*>(&md_accum_kernel) : reinterpret_cast<const void*>(&ev_accum_kernel);
  if (hipFuncSetAttribute(accum, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(int) * EV_LDS_WORDS)) != hipSuccess)
    return SAST_ELAUNCH;
  hipStream_t st = (hipStream_t)stream;
  const long long per = (in.capacity + EV_EVENTS_PER_BLOCK - 1) / EV_EVENTS_PER_BLOCK;
  const dim3 gb((unsigned)std::min<long long>(std::max<long long>(per, 1), EV_MAX_BLOCKS), (unsigned)in.B);
  const dim3 gt((unsigned)g.tiles, (unsigned)in.B);
  const size_t lds_hist = sizeof(int) * (size_t)g.tiles;
  const size_t lds_acc = sizeof(int) * (size_t)(g.th * EV_TILE_W * g.C);     // both accumulate kernels keep 4-byte counters
  SAST_LAUNCH(ev_count_kernel<MD>, gb, dim3(EV_THREADS), lds_hist, st, in, g, w.tile_cnt);
  SAST_LAUNCH(ev_scan_kernel, dim3((unsigned)in.B), dim3(EV_THREADS), 0, st, in, g, w.tile_cnt, w.off, w.cursor, w.ovf);
  SAST_LAUNCH(ev_scatter_kernel<MD>, gb, dim3(EV_THREADS), lds_hist, st, in, g, w.cursor, (const int*)w.ovf, w.recs);
  if constexpr (MD) SAST_LAUNCH(md_accum_kernel, gt, dim3(EV_THREADS), lds_acc, st, in, g, (const int*)w.off, (const unsigned*)w.recs);
  else SAST_LAUNCH(ev_accum_kernel, gt, dim3(EV_THREADS), lds_acc, st, in, g, (const int*)w.off, (const unsigned*)w.recs);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

// the time correction of S rows with `blocks` workgroups per row
int ev_correct_time(const void* t, int t_dtype, const int64_t* counts, int S, int64_t cap, int64_t* t_out, int64_t* t_last,
                    const uint8_t* reset, int64_t* ws, long long blocks, sast_stream_t stream) {
  if (!t || !counts || !t_out || !t_last || !ws || S < 1 || S > 65535 || cap < 0 || (t_dtype != SAST_DT_I64 && t_dtype != SAST_DT_I32))
    return SAST_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)blocks, (unsigned)S);
  const long long* cd = reinterpret_cast<const long long*>(counts);
  long long* w = reinterpret_cast<long long*>(ws);
  SAST_LAUNCH(ev_tmax_partial_kernel, grid, dim3(EV_THREADS), 0, st, t, t_dtype, cd, (long long)cap,
              reinterpret_cast<const long long*>(t_last), reinterpret_cast<const unsigned char*>(reset), w);
  SAST_LAUNCH(ev_tmax_apply_kernel, grid, dim3(EV_THREADS), 0, st, t, t_dtype, cd, (long long)cap, reinterpret_cast<const long long*>(w),
              reinterpret_cast<long long*>(t_out), reinterpret_cast<long long*>(t_last));
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

// the window search of T windows in each of S rows
int ev_window_bounds(const int64_t* t, const int64_t* counts, int S, int64_t cap, const int64_t* ends_us, int T, int mode, int64_t value,
                     int64_t* bounds, sast_stream_t stream, const int32_t* rows = nullptr, int cols = 0) {
  if (!rows) cols = S;
  if (!t || !counts || !ends_us || !bounds || S < 1 || T < 1 || cols < 1 || (long long)cols * T > INT_MAX || cap < 0 || value < 0 ||
      (mode != SAST_EVENT_WINDOW_DURATION && mode != SAST_EVENT_WINDOW_COUNT))
    return SAST_EINVAL;
  const int B = cols * T;
  SAST_LAUNCH(ev_bounds_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(t),
              reinterpret_cast<const long long*>(counts), S, (long long)cap, reinterpret_cast<const long long*>(ends_us), B, mode,
              (long long)value, reinterpret_cast<long long*>(bounds), rows, cols);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}


// ---- the event queue (sast_evqueue_*): S rows of retained events [head, count) in [S, capacity] storage, fed by chunks of any size.
// Every index into a row is formed from device-read sizes and clamped to capacity / chunk_capacity before it is used.
constexpr int EVQ_ROW_WS = EV_ROW_WS + 5;     // a row's ws: the scan's carry + partial maxima, then the append plan and the move plan
constexpr int EVQ_APPEND_BASE = EV_ROW_WS, EVQ_APPEND_N = EV_ROW_WS + 1, EVQ_DROPPED = EV_ROW_WS + 2, EVQ_MOVE_SRC = EV_ROW_WS + 3,
              EVQ_MOVE_N = EV_ROW_WS + 4;

struct EvqChunk {
  const void *x, *y, *p, *t;     // columns [S, chunk_cap]; packed records: t holds them, x / y / p are not read
  int xd, yd, pd, td;
  const long long* counts;
  long long chunk_cap;
  const unsigned char* reset;
};

// Event2D of the reference's reader (dat_events_tools.py:18-50): word 0 the unsigned 32-bit time, word 1 x | y << 14 | p << 28
__device__ __forceinline__ long long evq_time(const EvqChunk& c, long long i) {
  if (c.td == SAST_EVQUEUE_DT_DAT) return (long long)static_cast<const unsigned*>(c.t)[2 * i];
  return ld_int(c.t, c.td, i);
}

__device__ __forceinline__ short sat16(long long v) { return (short)min(max(v, -32768LL), 32767LL); }

// push, pass 1: the partial maxima of the timestamps that will be stored, and (block 0 of a row) the append plan: where the chunk
// goes and how much of it fits.  Reads the queue's state, writes only ws.
__global__ __launch_bounds__(EV_THREADS) void evq_partial_kernel(SastEvQueueArgs q, EvqChunk c, long long* ws_all) {
  __shared__ long long red[EV_THREADS / 64];
  const int s = blockIdx.y;
  const bool rst = c.reset && c.reset[s];
  const long long cap = q.capacity;
  const long long base = rst ? 0LL : min(max((long long)q.count[s], 0LL), cap);
  const long long want = min(max(c.counts[s], 0LL), c.chunk_cap);
  const long long n = min(want, cap - base), row = (long long)s * c.chunk_cap;
  long long lo, hi;
  ev_tchunk(n, &lo, &hi);
  long long m = LLONG_MIN;
  for (long long i = lo + threadIdx.x; i < hi; i += EV_THREADS) m = max(m, evq_time(c, row + i));
  m = block_max(m, red);
  if (threadIdx.x == 0) {
    long long* w = ws_all + (size_t)s * EVQ_ROW_WS;
    w[1 + blockIdx.x] = m;
    if (blockIdx.x == 0) {
      w[0] = rst ? 0LL : (long long)q.t_last[s];
      w[EVQ_APPEND_BASE] = base;
      w[EVQ_APPEND_N] = n;
      w[EVQ_DROPPED] = want - n;
    }
  }
}

// push, pass 2: the running maximum from the row's carry, the decode / saturating narrowing, the append behind the plan's base; the
// row's last workgroup then writes the new state.  No workgroup reads state that another one writes: sizes come from the plan.
__global__ __launch_bounds__(EV_THREADS) void evq_append_kernel(SastEvQueueArgs q, EvqChunk c, const long long* ws_all) {
  __shared__ long long red[EV_THREADS / 64];
  __shared__ long long wtot[EV_THREADS / 64];
  const int s = blockIdx.y;
  const long long* ws = ws_all + (size_t)s * EVQ_ROW_WS;
  const long long cap = q.capacity;
  const long long base = min(max(ws[EVQ_APPEND_BASE], 0LL), cap);
  const long long n = min(min(max(ws[EVQ_APPEND_N], 0LL), cap - base), c.chunk_cap);
  const long long row = (long long)s * c.chunk_cap, qrow = (long long)s * cap + base;
  long long lo, hi;
  ev_tchunk(n, &lo, &hi);
  long long carry = LLONG_MIN;
  for (int k = threadIdx.x; k < (int)blockIdx.x + 1; k += EV_THREADS) carry = max(carry, ws[k]);
  carry = block_max(carry, red);
  for (long long b0 = lo; b0 < hi; b0 += EV_THREADS) {
    const long long i = b0 + threadIdx.x;
    long long v = LLONG_MIN;
    short x = 0, y = 0, p = 0;
    if (i < hi) {
      if (c.td == SAST_EVQUEUE_DT_DAT) {
        const uint2 r = static_cast<const uint2*>(c.t)[row + i];       // one coalesced 8-byte load per record
        v = (long long)r.x;
        x = (short)(r.y & 16383u);
        y = (short)((r.y >> 14) & 16383u);
        p = (short)((r.y >> 28) & 1u);
      } else {
        v = ld_int(c.t, c.td, row + i);
        x = sat16(ld_int(c.x, c.xd, row + i));
        y = sat16(ld_int(c.y, c.yd, row + i));
        p = sat16(ld_int(c.p, c.pd, row + i));
      }
    }
    carry = block_max_scan(&v, carry, wtot);
    if (i < hi) {
      q.t[qrow + i] = v;
      q.x[qrow + i] = x;
      q.y[qrow + i] = y;
      q.p[qrow + i] = p;
    }
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    long long m = ws[0];
    for (int k = 1; k <= (int)gridDim.x; ++k) m = max(m, ws[k]);
    q.t_last[s] = m;
    q.count[s] = base + n;
    if (c.reset && c.reset[s]) {
      q.head[s] = 0;
      q.retired[s] = 0;
      q.retired_t[s] = 0;
    }
    if (ws[EVQ_DROPPED] > 0) atomicAdd(&q.err[2], (int)min(ws[EVQ_DROPPED], (long long)INT_MAX));
  }
}

// a row's live range [h, c) inside its storage
__device__ __forceinline__ void evq_live(const SastEvQueueArgs& q, int s, long long* h, long long* c) {
  *h = min(max((long long)q.head[s], 0LL), (long long)q.capacity);
  *c = min(max((long long)q.count[s], *h), (long long)q.capacity);
}

// the search of ev_bounds_kernel over a row's live events; a window that needs retired events is counted in err[3]
__global__ void evq_bounds_kernel(SastEvQueueArgs q, const long long* ends, int B, int mode, long long value, long long* bounds) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;     // window k * S + s
  if (w >= B) return;
  const int s = w % q.S;
  long long h, c;
  evq_live(q, s, &h, &c);
  const long long row = (long long)s * q.capacity;
  const long long* t = reinterpret_cast<const long long*>(q.t) + row + h;
  const long long e = h + search(t, c - h, ends[w], true);
  long long b;
  bool late;
  if (mode == SAST_EVENT_WINDOW_COUNT) {
    b = max(e - value, h);
    late = e - h < value && q.retired[s] > 0;
  } else {
    b = h + search(t, c - h, ends[w] - value, false);
    late = q.retired[s] > 0 && (long long)q.retired_t[s] >= ends[w] - value;
  }
  bounds[2 * w] = row + b;
  bounds[2 * w + 1] = row + e;
  if (late) atomicAdd(&q.err[3], 1);
}

// retire, pass 1, one thread per row: everything before the start of the row's last window leaves; the row moves to the front of its
// storage only when the live part fits into the freed part (source and destination disjoint).  Writes the new head / count and the
// move plan.
__global__ void evq_plan_kernel(SastEvQueueArgs q, const long long* bounds, int T, long long* ws_all) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= q.S) return;
  long long h, c;
  evq_live(q, s, &h, &c);
  const long long row = (long long)s * q.capacity;
  const long long start = min(max(bounds[2 * ((long long)(T - 1) * q.S + s)] - row, h), c);
  if (start > h) {
    q.retired[s] += start - h;
    q.retired_t[s] = reinterpret_cast<const long long*>(q.t)[row + start - 1];
  }
  const long long live = c - start;
  const bool move = start > 0 && live <= start;
  long long* w = ws_all + (size_t)s * EVQ_ROW_WS;
  w[EVQ_MOVE_SRC] = start;
  w[EVQ_MOVE_N] = move ? live : 0;
  q.head[s] = move ? 0 : start;
  q.count[s] = move ? live : c;
}

// retire, pass 2: the moves of the plan.  Reads the plan only; n <= src, so no element is read after it was overwritten.
__global__ __launch_bounds__(EV_THREADS) void evq_move_kernel(SastEvQueueArgs q, const long long* ws_all) {
  const int s = blockIdx.y;
  const long long* w = ws_all + (size_t)s * EVQ_ROW_WS;
  const long long cap = q.capacity;
  const long long src = min(max(w[EVQ_MOVE_SRC], 0LL), cap);
  const long long n = min(min(max(w[EVQ_MOVE_N], 0LL), src), cap - src);
  const long long row = (long long)s * cap;
  for (long long i = (long long)blockIdx.x * EV_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * EV_THREADS) {
    q.t[row + i] = q.t[row + src + i];
    q.x[row + i] = q.x[row + src + i];
    q.y[row + i] = q.y[row + src + i];
    q.p[row + i] = q.p[row + src + i];
  }
}

// the scheduler of duration windows, one thread per row: window k of this call ends at e_k = next_end + k * D and is due once an event
// later than e_k was pushed (t_last > e_k), or, when the recording is over, while it still holds an event time (e_k - D < t_last).
// Both are monotone in k, so the due windows are counted in closed form: the k >= 0 with lo + k * D < t_last, lo = next_end or
// next_end - D.  Steps behind the due ones repeat the last end the row gave, which asks the queue for nothing new.
__global__ void evq_schedule_kernel(SastEvQueueArgs q, long long* next_end, long long D, long long first_end, int W,
                                    const unsigned char* reset, const unsigned char* final_flags, long long* ends, unsigned char* due,
                                    long long* backlog) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= q.S) return;
  const long long ne = reset && reset[s] ? first_end : next_end[s];
  const long long tl = (long long)q.t_last[s];
  const long long lo = final_flags && final_flags[s] ? ne - D : ne;
  const long long n_all = tl > lo ? (tl - lo - 1) / D + 1 : 0LL;
  const long long n = min(n_all, (long long)W);
  const long long held = ne + (n - 1) * D;
  for (int k = 0; k < W; ++k) {
    const size_t w = (size_t)k * q.S + s;
    ends[w] = k < n ? ne + k * D : held;
    due[w] = k < n ? 1 : 0;
  }
  backlog[s] = n_all - n;
  next_end[s] = ne + n * D;
}

bool evq_args(const SastEvQueueArgs* q) {
  return q && q->x && q->y && q->p && q->t && q->head && q->count && q->t_last && q->retired && q->retired_t && q->err && q->ws &&
         q->S >= 1 && q->S <= 65535 && q->capacity >= 1 && (long long)q->S * q->capacity <= INT_MAX;
}

long long evq_blocks(long long events) {
  const long long per = (events + EV_ROW_EVENTS_PER_BLOCK - 1) / EV_ROW_EVENTS_PER_BLOCK;
  return std::min<long long>(std::max<long long>(per, 1), EV_SCAN_BLOCKS);
}
}  // namespace
}  // namespace sast

extern "C" {

// one recording is the S = 1 form of the per-row calls: n is its one-element counts, t_last its one-element carry row, no reset flags.
// Each entry point keeps its own grid (here every scan block, per row as many as the capacity needs).
int sast_event_correct_time(const void* t, int t_dtype, const int64_t* n, int64_t capacity, int64_t* t_out, int64_t* t_last, int64_t* ws,
                            sast_stream_t stream) {
  SAST_ENTRY();
  return sast::ev_correct_time(t, t_dtype, n, 1, capacity, t_out, t_last, nullptr, ws, sast::EV_SCAN_BLOCKS, stream);
}

int sast_event_window_bounds(const int64_t* t, const int64_t* n, int64_t capacity, const int64_t* ends_us, int B, int mode, int64_t value,
                             int64_t* bounds, sast_stream_t stream) {
  SAST_ENTRY();
  return sast::ev_window_bounds(t, n, 1, capacity, ends_us, B, mode, value, bounds, stream);
}

size_t sast_evstreams_ws_count(int S) { return S < 1 || S > 65535 ? 0 : (size_t)S * sast::EV_ROW_WS; }

int sast_evstreams_correct_time(const void* t, int t_dtype, const int64_t* counts, int S, int64_t stream_capacity, int64_t* t_out,
                                int64_t* t_last, const uint8_t* reset, int64_t* ws, sast_stream_t stream) {
  SAST_ENTRY();
  const long long per = (stream_capacity + sast::EV_ROW_EVENTS_PER_BLOCK - 1) / sast::EV_ROW_EVENTS_PER_BLOCK;
  const long long blocks = std::min<long long>(std::max<long long>(per, 1), sast::EV_SCAN_BLOCKS);
  return sast::ev_correct_time(t, t_dtype, counts, S, stream_capacity, t_out, t_last, reset, ws, blocks, stream);
}

int sast_evstreams_window_bounds(const int64_t* t, const int64_t* counts, int S, int64_t stream_capacity, const int64_t* ends_us, int T,
                                 int mode, int64_t value, int64_t* bounds, sast_stream_t stream) {
  SAST_ENTRY();
  return sast::ev_window_bounds(t, counts, S, stream_capacity, ends_us, T, mode, value, bounds, stream);
}

int sast_rnd_window_bounds(const int64_t* t, const int64_t* counts, int R, int64_t stream_capacity, const int32_t* rows,
                           const int64_t* ends_us, int B, int T, int mode, int64_t value, int64_t* bounds, sast_stream_t stream) {
  SAST_ENTRY();
  if (!rows || B < 1 || R < 1 || R > 65535 || stream_capacity < 0 || (long long)R * stream_capacity > INT_MAX) return SAST_EINVAL;
  return sast::ev_window_bounds(t, counts, R, stream_capacity, ends_us, T, mode, value, bounds, stream, rows, B);
}

size_t sast_event_frames_ws_bytes(int B, int bins, int height, int width, int downsample_by_2, int64_t window_capacity) {
  sast::EvGeom g;
  if (!sast::ev_geom(B, bins, height, width, downsample_by_2, window_capacity, &g)) return 0;
  return sast::ev_ws(nullptr, B, g, window_capacity).bytes;
}

int sast_event_frames(const SastEventArgs* a, sast_stream_t stream) {
  SAST_ENTRY();
  if (!a || a->count_cutoff < 1 || a->count_cutoff > 255) return SAST_EINVAL;
  sast::EvGeom g = {};
  g.cutoff = a->count_cutoff;
  g.fast = a->fastmode ? 1 : 0;
  g.clip_pol = a->clip_negative_polarity ? 1 : 0;
  return sast::ev_frames<false>(a, g, stream);
}

size_t sast_mdstack_frames_ws_bytes(int B, int bins, int height, int width, int downsample_by_2, int64_t window_capacity) {
  sast::EvGeom g;
  if (!sast::ev_geom(B, bins, height, width, downsample_by_2, window_capacity, &g, true)) return 0;
  return sast::ev_ws(nullptr, B, g, window_capacity).bytes;
}

int sast_mdstack_frames(const SastMdStackArgs* m, sast_stream_t stream) {
  SAST_ENTRY();
  if (!m || m->count_cutoff < -1 || m->count_cutoff > 127) return SAST_EINVAL;
  sast::EvGeom g = {};
  g.cutoff = m->count_cutoff;
  g.fast = 0;
  g.clip_pol = m->clip_negative_polarity ? 1 : 0;
  return sast::ev_frames<true>(m, g, stream);
}

size_t sast_evqueue_ws_count(int S) { return S < 1 || S > 65535 ? 0 : (size_t)S * sast::EVQ_ROW_WS; }

int sast_evqueue_push(const SastEvQueueArgs* q, const void* x, const void* y, const void* p, const void* t, int x_dtype, int y_dtype,
                      int p_dtype, int t_dtype, const int64_t* counts, int64_t chunk_capacity, const uint8_t* reset, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::evq_args(q) || !t || !counts || chunk_capacity < 0 || chunk_capacity > INT_MAX / q->S) return SAST_EINVAL;
  if (t_dtype != SAST_EVQUEUE_DT_DAT) {
    if (!x || !y || !p || !sast::int_dtype(x_dtype) || !sast::int_dtype(y_dtype) || !sast::int_dtype(p_dtype) ||
        (t_dtype != SAST_DT_I64 && t_dtype != SAST_DT_I32))
      return SAST_EINVAL;
  }
  const sast::EvqChunk c{x, y, p, t, x_dtype, y_dtype, p_dtype, t_dtype, reinterpret_cast<const long long*>(counts),
                         (long long)chunk_capacity, reinterpret_cast<const unsigned char*>(reset)};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)sast::evq_blocks(chunk_capacity), (unsigned)q->S);
  long long* ws = reinterpret_cast<long long*>(q->ws);
  SAST_LAUNCH(sast::evq_partial_kernel, grid, dim3(sast::EV_THREADS), 0, st, *q, c, ws);
  SAST_LAUNCH(sast::evq_append_kernel, grid, dim3(sast::EV_THREADS), 0, st, *q, c, (const long long*)ws);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_evqueue_window_bounds(const SastEvQueueArgs* q, const int64_t* ends_us, int T, int mode, int64_t value, int64_t* bounds,
                               sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::evq_args(q) || !ends_us || !bounds || T < 1 || (long long)q->S * T > INT_MAX || value < 0 ||
      (mode != SAST_EVENT_WINDOW_DURATION && mode != SAST_EVENT_WINDOW_COUNT))
    return SAST_EINVAL;
  const int B = q->S * T;
  SAST_LAUNCH(sast::evq_bounds_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, *q, reinterpret_cast<const long long*>(ends_us),
              B, mode, (long long)value, reinterpret_cast<long long*>(bounds));
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_evqueue_retire(const SastEvQueueArgs* q, const int64_t* bounds, int T, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::evq_args(q) || !bounds || T < 1 || (long long)q->S * T > INT_MAX) return SAST_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  long long* ws = reinterpret_cast<long long*>(q->ws);
  SAST_LAUNCH(sast::evq_plan_kernel, dim3((q->S + 63) / 64), dim3(64), 0, st, *q, reinterpret_cast<const long long*>(bounds), T, ws);
  // at most half a row moves (live <= head)
  SAST_LAUNCH(sast::evq_move_kernel, dim3((unsigned)sast::evq_blocks(q->capacity / 2), (unsigned)q->S), dim3(sast::EV_THREADS), 0, st, *q,
              (const long long*)ws);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_evq_schedule(const SastEvQueueArgs* q, int64_t* next_end, int mode, int64_t value, int64_t first_end_us, int W,
                          const uint8_t* reset, const uint8_t* final_flags, int64_t* ends, uint8_t* due, int64_t* backlog,
                          sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::evq_args(q) || !next_end || !ends || !due || !backlog || mode != SAST_EVENT_WINDOW_DURATION || value < 1 ||
      first_end_us < value || W < 1 || (long long)q->S * W > INT_MAX)
    return SAST_EINVAL;
  SAST_LAUNCH(sast::evq_schedule_kernel, dim3((q->S + 63) / 64), dim3(64), 0, (hipStream_t)stream, *q, reinterpret_cast<long long*>(next_end),
              (long long)value, (long long)first_end_us, W, reinterpret_cast<const unsigned char*>(reset),
              reinterpret_cast<const unsigned char*>(final_flags), reinterpret_cast<long long*>(ends), reinterpret_cast<unsigned char*>(due),
              reinterpret_cast<long long*>(backlog));
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
