// Spatial augmentation with rotation: flip, then rotate, then zoom-in or zoom-out, the order of RandomSpatialAugmentorGenX.__call__
// (data/utils/augmentor.py:347-364).  k_augment.hip serves the augmentor without rotation: its map is separable (a column map per
// sample, whole source rows staged in LDS).  A rotated frame is a 2-D gather, so this file has a kernel of its own:
//   sast_rotaug_frames  one composed gather per frame.  Output pixel (y, x) goes through the zoom map (axis_src, unchanged) to (sy, sx)
//                       or to the zero border, the rotation map (rot_src: torchvision's tensor rotate, NEAREST, restated one fp32
//                       rounding at a time) takes (sy, sx) to a source pixel or outside, the flip mirrors the source column.  A
//                       workgroup owns a 64 x 64 tile of one frame and a group of channels: a thread computes the source pixels of
//                       its 16 pixels ONCE (registers, -1 = zero) and the workgroup the box that holds them; then per channel the box
//                       is staged in LDS with 16-byte loads, a thread gathers its 16 bytes from LDS and writes them with one 16-byte
//                       store.  A box too large for LDS is gathered straight from global memory.  No atomics, no workspace.
//   sast_rotaug_labels  sast_augment_labels with rotate_ (data/genx_utils/labels.py:210-248) between flip_lr_ and the zooms.
// A sample whose rot_params row is inactive gets exactly what sast_augment_frames / sast_augment_labels give it.
// build.py compiles this file with -ffp-contract=off (SOURCE_FLAGS): the rules round every product before it is added.
#include "aug_map.cuh"

namespace sast {
namespace {

constexpr int ROT_THREADS = 256;
constexpr int ROT_PX = 16;                         // pixels of one thread: one 16-byte store
constexpr int ROT_TILE = 64;                       // a workgroup owns a 64 x 64 tile of output pixels: 256 threads x 16 pixels
constexpr int ROT_LDS_BYTES = 24576;               // staging area: the source box of a tile rotated by 45 degrees and zoomed out by 1.6 fits
constexpr int ROT_TARGET_WGS = 2048;               // channels are split across workgroups until the grid has about this many

// source pixel of output pixel (y, x) as (row << 12) | column, both < 4096; -1: the pixel is 0
__device__ __forceinline__ int rotaug_src(const AugSample& s, const RotSample& r, int y, int x, int H, int W) {
  int sy = axis_src(y, s.mode, s.y0, s.wh, H);
  int sx = axis_src(x, s.mode, s.x0, s.ww, W);
  if (sy < 0 || sx < 0) return -1;                               // the zero border of zoom-out
  if (r.active && !rot_src(r, sy, sx, H, W, &sy, &sx)) return -1;   // rotated in from outside the frame
  return (sy << 12) | (s.flip ? W - 1 - sx : sx);                // 0 <= sy < H and 0 <= sx < W on both ways here
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
  return v;
}

// VEC: W is a multiple of 16 and out is 16-byte aligned: a thread's 16 pixels are 16 consecutive bytes of one row (row tid / 4 of the
// tile), stored at once.  Otherwise pixel k of thread t is tile pixel k * 256 + t (row 4 k + t / 64, column t % 64), stored byte by byte.
// in_vec: W is a multiple of 16 and in is 16-byte aligned: the source box is staged with 16-byte loads, else byte by byte.
// Per tile, once: the source pixels of the thread's 16 pixels and the box [ylo, yhi] x [xlo, xhi] that holds the tile's sources (shuffle
// reductions, no atomics).  Per channel: the box is staged in LDS (rows of an odd number of dwords, so the rows of a tilted read fall
// into different banks) and the bytes are gathered from there; a box that does not fit the staging area (a large zoom-out factor at a
// large angle) is gathered from global memory instead, with the same offsets.  The choice is workgroup-uniform.
template <bool VEC>
__global__ __launch_bounds__(ROT_THREADS) void rotaug_frames_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                                    const int* __restrict__ params, const int* __restrict__ rot_params, int B,
                                                                    int C, int H, int W, int tiles_x, int ch_per_wg, int in_vec) {
  __shared__ __align__(16) unsigned char stage[ROT_LDS_BYTES];
  __shared__ int wave_box[ROT_THREADS / 64][4];
  const int tid = threadIdx.x;
  const int n = blockIdx.z;
  const AugSample s = aug_sample(params + (size_t)(n % B) * SAST_AUGMENT_PARAM_WORDS, H, W);
  const RotSample r = rot_sample(rot_params + (size_t)(n % B) * SAST_ROTAUG_PARAM_WORDS);
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int y_base = ty * ROT_TILE, x_base = tx * ROT_TILE;      // < H, < W: the grid has ceil(H / 64) * ceil(W / 64) tiles

  int off[ROT_PX];
  int ylo = AUG_MAX_HW, nyhi = 0, xlo = AUG_MAX_HW, nxhi = 0;    // nyhi, nxhi: minus the maxima
#pragma unroll
  for (int k = 0; k < ROT_PX; ++k) {
    const int y = y_base + (VEC ? (tid >> 2) : 4 * k + (tid >> 6));
    const int x = x_base + (VEC ? (tid & 3) * ROT_PX + k : (tid & 63));
    const int o = (y < H && x < W) ? rotaug_src(s, r, y, x, H, W) : -1;
    off[k] = o;
    if (o >= 0) {
      ylo = min(ylo, o >> 12);
      nyhi = min(nyhi, -(o >> 12));
      xlo = min(xlo, o & 4095);
      nxhi = min(nxhi, -(o & 4095));
    }
  }
  ylo = wave_min(ylo);
  nyhi = wave_min(nyhi);
  xlo = wave_min(xlo);
  nxhi = wave_min(nxhi);
  if ((tid & 63) == 0) {
    wave_box[tid >> 6][0] = ylo;
    wave_box[tid >> 6][1] = nyhi;
    wave_box[tid >> 6][2] = xlo;
    wave_box[tid >> 6][3] = nxhi;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < ROT_THREADS / 64; ++w) {
    ylo = min(ylo, wave_box[w][0]);
    nyhi = min(nyhi, wave_box[w][1]);
    xlo = min(xlo, wave_box[w][2]);
    nxhi = min(nxhi, wave_box[w][3]);
  }
  const int yhi = -nyhi, xhi = -nxhi;
  const bool any = ylo <= yhi;                                   // else every pixel of the tile is 0
  // the staged box: rows ylo..yhi, columns xs0..; 0 <= ylo <= yhi < H and 0 <= xs0 <= xlo <= xhi < W where `any`
  const int xs0 = in_vec ? (xlo & ~15) : xlo;
  const int n16 = ((xhi - xs0) >> 4) + 1;                        // 16-byte items of a staged row (in_vec: they end at or before W)
  const int span = xhi - xs0 + 1;                                // bytes of a staged row (byte staging)
  const int pitch = 4 * ((in_vec ? 4 * n16 : (span + 3) >> 2) | 1);
  const int rows = yhi - ylo + 1;
  const bool staged = any && (long long)rows * pitch <= ROT_LDS_BYTES;
#pragma unroll
  for (int k = 0; k < ROT_PX; ++k) {
    const int o = off[k];
    if (o >= 0) off[k] = staged ? ((o >> 12) - ylo) * pitch + ((o & 4095) - xs0) : (o >> 12) * W + (o & 4095);
  }

  const int c_begin = blockIdx.y * ch_per_wg, c_end = min(C, c_begin + ch_per_wg);
  const size_t plane = (size_t)H * W;
  for (int c = c_begin; c < c_end; ++c) {
    const unsigned char* inp = in + ((size_t)n * C + c) * plane;
    unsigned char* outp = out + ((size_t)n * C + c) * plane;
    unsigned v[ROT_PX];
    if (staged) {
      if (c != c_begin) __syncthreads();                         // the previous channel's gather has finished with the staging area
      if (in_vec) {
        for (int it = tid; it < rows * n16; it += ROT_THREADS) {
          const int row = it / n16, j = it - row * n16;
          const uint4 q = *reinterpret_cast<const uint4*>(inp + (size_t)(ylo + row) * W + xs0 + 16 * j);
          unsigned* d = reinterpret_cast<unsigned*>(stage + row * pitch + 16 * j);
          d[0] = q.x;
          d[1] = q.y;
          d[2] = q.z;
          d[3] = q.w;
        }
      } else {
        for (int it = tid; it < rows * span; it += ROT_THREADS) {
          const int row = it / span, j = it - row * span;
          stage[row * pitch + j] = inp[(size_t)(ylo + row) * W + xs0 + j];
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < ROT_PX; ++k) v[k] = off[k] >= 0 ? (unsigned)stage[off[k]] : 0u;
    } else {
#pragma unroll
      for (int k = 0; k < ROT_PX; ++k) v[k] = off[k] >= 0 ? (unsigned)inp[off[k]] : 0u;
    }
    if (VEC) {
      const int y = y_base + (tid >> 2), x = x_base + (tid & 3) * ROT_PX;
      if (y < H && x < W) {                                      // W % 16 == 0: all 16 bytes are inside the row
        uint4 o;
        o.x = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        o.y = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
        o.z = v[8] | (v[9] << 8) | (v[10] << 16) | (v[11] << 24);
        o.w = v[12] | (v[13] << 8) | (v[14] << 16) | (v[15] << 24);
        *reinterpret_cast<uint4*>(outp + (size_t)y * W + x) = o;
      }
    } else {
#pragma unroll
      for (int k = 0; k < ROT_PX; ++k) {
        const int y = y_base + 4 * k + (tid >> 6), x = x_base + (tid & 63);
        if (y < H && x < W) outp[(size_t)y * W + x] = (unsigned char)v[k];
      }
    }
  }
}

__global__ __launch_bounds__(64) void rotaug_labels_kernel(const float* __restrict__ in, const int* __restrict__ counts,
                                                           const int* __restrict__ params, const int* __restrict__ rot_params, int B, int M,
                                                           int H, int W, float* __restrict__ out, int* __restrict__ counts_out,
                                                           float* __restrict__ yolox) {
  aug_labels_frame<true>(in, counts, params, rot_params, B, M, H, W, out, counts_out, yolox);
}

}  // namespace
}  // namespace sast

extern "C" {

int sast_rotaug_frames(const uint8_t* in, uint8_t* out, const int32_t* params, const int32_t* rot_params, int N, int B, int C, int H, int W,
                       sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!in || !out || !params || !rot_params || in == out || N < 1 || B < 1 || C < 1 || H < 1 || W < 1 || H > AUG_MAX_HW || W > AUG_MAX_HW ||
      N > 65535 || C > 65535)
    return SAST_EINVAL;
  const int tiles_x = (W + ROT_TILE - 1) / ROT_TILE, tiles = tiles_x * ((H + ROT_TILE - 1) / ROT_TILE);
  const long long per_c = (long long)N * tiles;
  const int c_groups = (int)std::min<long long>(C, std::max<long long>(1, (ROT_TARGET_WGS + per_c - 1) / per_c));
  const int ch_per_wg = (C + c_groups - 1) / c_groups;
  const dim3 grid((unsigned)tiles, (unsigned)((C + ch_per_wg - 1) / ch_per_wg), (unsigned)N);
  const bool vec = (W % 16 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
  const int in_vec = (W % 16 == 0) && (reinterpret_cast<uintptr_t>(in) % 16 == 0);
  if (vec)
    SAST_LAUNCH(rotaug_frames_kernel<true>, grid, dim3(ROT_THREADS), 0, (hipStream_t)stream, in, out, params, rot_params, B, C, H, W, tiles_x,
                ch_per_wg, in_vec);
  else
    SAST_LAUNCH(rotaug_frames_kernel<false>, grid, dim3(ROT_THREADS), 0, (hipStream_t)stream, in, out, params, rot_params, B, C, H, W, tiles_x,
                ch_per_wg, in_vec);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_rotaug_labels(const float* labels, const int32_t* counts, const int32_t* params, const int32_t* rot_params, int N, int B, int M, int H,
                       int W, float* out, int32_t* counts_out, float* yolox, sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!labels || !counts || !params || !rot_params || !out || !counts_out || labels == out || counts == counts_out || N < 1 || B < 1 ||
      M < 1 || H < 1 || W < 1 || H > AUG_MAX_HW || W > AUG_MAX_HW)
    return SAST_EINVAL;
  SAST_LAUNCH(rotaug_labels_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, labels, counts, params, rot_params, B, M, H, W, out,
              counts_out, yolox);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
