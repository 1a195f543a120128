// Spatial augmentation of event frames and box labels on the device.
//
// Reference: RandomSpatialAugmentorGenX.__call__ (data/utils/augmentor.py:347-364) on uint8 event frames -- horizontal flip
// (th.flip(dims=[-1])), then zoom-in (:203-222: a slice cut at the frame's edge, interpolate(size=(H, W), 'nearest-exact')) or
// zoom-out (:134-153: interpolate of the whole frame to the window, pasted into zeros) -- and the label transforms of ObjectLabels
// (data/genx_utils/labels.py:255-339).  Two entry points:
//   sast_augment_frames  one gather per frame: out[c, y, x] = in[c, sy(y), W-1-sx(x)] (sx(x) without flip), zero outside the zoom-out
//                        window.  A workgroup owns a band of output rows of one frame: it computes the column map once (it depends on
//                        the sample only), then per channel stages the distinct source rows of the band in LDS with 16-byte loads,
//                        gathers bytes from LDS and writes whole rows with 16-byte stores, the zero border included.
//   sast_augment_labels  flip_lr_ / zoom_in_and_rescale_ / zoom_out_and_rescale_ / scale_ / remove_flat_labels_ on [N, M, 7] rows, the
//                        survivors compacted to the front in their order; optionally the head's (class, cx, cy, w, h) layout.
// The per-sample parameters are read from device memory (SAST_AUGMENT_PARAM_WORDS int32 words per sample), so a captured graph is
// replayed with new parameters by rewriting that tensor.  The host validates them; the kernels still clamp every index they form.
#include "aug_map.cuh"

// hipcc contracts a * b + c into an FMA by default (-ffp-contract=fast) and its __fmul_rn / __fadd_rn are plain operators, while the
// label arithmetic (aug_map.cuh) must round every product first, as the reference's separate tensor operations do: build.py compiles this
// file with -ffp-contract=off (SOURCE_FLAGS)

namespace sast {
namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_ROWS = 16;       // output rows of one band (fewer for very wide frames: the LDS budget below)
constexpr int AUG_LDS_BUDGET = 49152;  // bytes of dynamic LDS one workgroup may ask for
constexpr int AUG_TARGET_WGS = 2048;   // channels are split across workgroups until the grid has about this many

// the zoom and flip maps (aug_sample, axis_src, col_src) and the label transforms of one frame: aug_map.cuh

// VEC: W is a multiple of 16 and both bases are 16-byte aligned, so every row starts on a 16-byte boundary.
// Dynamic LDS: [column map: uint16 x Wp][staging: rows x (pitch + 16)], Wp = W rounded up to 16; the 16 bytes after each staged row
// stay zero and are where the map sends the columns of the zero border.
template <bool VEC>
__global__ __launch_bounds__(AUG_THREADS) void aug_frames_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                                 const int* __restrict__ params, int B, int C, int H, int W, int rows_per_wg,
                                                                 int ch_per_wg) {
  extern __shared__ __align__(16) unsigned char aug_lds[];
  __shared__ int src_y[AUG_MAX_ROWS];      // source row of each output row of the band; -1: a zero row
  __shared__ int slot_of[AUG_MAX_ROWS];    // staging slot of each output row
  __shared__ int slot_src[AUG_MAX_ROWS];   // source row held by each slot
  __shared__ int n_slots;

  const int tid = threadIdx.x;
  const int n = blockIdx.z;
  const AugSample s = aug_sample(params + (size_t)(n % B) * SAST_AUGMENT_PARAM_WORDS, H, W);
  const int Wp = (W + 15) & ~15;
  const int W16 = Wp >> 4;
  unsigned short* cmap = reinterpret_cast<unsigned short*>(aug_lds);
  unsigned char* stage = aug_lds + 2 * (size_t)Wp;

  // the span of source columns the band needs: the map is monotone, so its ends are at the first and last non-border columns
  int xa = 0, xb = W - 1;
  if (s.mode == AUG_ZOOM_OUT) {
    xa = s.x0;
    xb = min(s.x0 + s.ww, W) - 1;
  }
  const int ca = col_src(xa, s, W), cb = col_src(xb, s, W);
  const int xs = min(ca, cb), xe = max(ca, cb) + 1;
  const int xs0 = VEC ? (xs & ~15) : xs;
  const int pitch = VEC ? (((xe + 15) & ~15) - xs0) : ((xe - xs0 + 15) & ~15);
  const int stride = pitch + 16;

  for (int x = tid; x < Wp; x += AUG_THREADS) {
    const int c = x < W ? col_src(x, s, W) : -1;
    const unsigned short m = (unsigned short)(c < 0 ? pitch : c - xs0);
    // VEC: the four entries of a 4-byte output group are adjacent, groups of one quarter q of the 16-byte items are contiguous
    const int at = VEC ? ((((x & 15) >> 2) * W16 + (x >> 4)) * 4 + (x & 3)) : x;
    cmap[at] = m;
  }
  const int y_base = blockIdx.x * rows_per_wg;
  const int rows = min(rows_per_wg, H - y_base);
  if (tid < rows) src_y[tid] = axis_src(y_base + tid, s.mode, s.y0, s.wh, H);
  if (tid < rows_per_wg * 16) stage[(size_t)(tid >> 4) * stride + pitch + (tid & 15)] = 0;
  __syncthreads();
  if (tid == 0) {
    int ns = 0, last = -1;
    for (int r = 0; r < rows; ++r) {
      const int sy = src_y[r];
      if (sy < 0) continue;
      if (sy != last) {
        slot_src[ns] = sy;
        last = sy;
        ++ns;
      }
      slot_of[r] = ns - 1;
    }
    n_slots = ns;
  }
  __syncthreads();
  const int ns = n_slots;
  const int c_begin = blockIdx.y * ch_per_wg, c_end = min(C, c_begin + ch_per_wg);
  const size_t plane_bytes = (size_t)H * W;
  const int rot = (tid >> 3) & 3;   // byte reads bank by dword over 32 lanes: each group of 8 lanes starts at another quarter of its item

  for (int c = c_begin; c < c_end; ++c) {
    const unsigned char* inp = in + ((size_t)n * C + c) * plane_bytes;
    unsigned char* outp = out + ((size_t)n * C + c) * plane_bytes;
    if (c != c_begin) __syncthreads();   // the previous channel's gather has finished with the staging area
    if (VEC) {
      const int k16 = pitch >> 4;
      for (int it = tid; it < ns * k16; it += AUG_THREADS) {
        const int sl = it / k16, k = it - sl * k16;
        const uint4 v = *reinterpret_cast<const uint4*>(inp + (size_t)slot_src[sl] * W + xs0 + 16 * k);
        *reinterpret_cast<uint4*>(stage + (size_t)sl * stride + 16 * k) = v;
      }
    } else {
      const int span = xe - xs0;
      for (int it = tid; it < ns * span; it += AUG_THREADS) {
        const int sl = it / span, k = it - sl * span;
        stage[(size_t)sl * stride + k] = inp[(size_t)slot_src[sl] * W + xs0 + k];
      }
    }
    __syncthreads();
    if (VEC) {
      for (int it = tid; it < rows * W16; it += AUG_THREADS) {
        const int r = it / W16, i = it - r * W16;
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (src_y[r] >= 0) {
          const unsigned char* row = stage + (size_t)slot_of[r] * stride;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int q = (qq + rot) & 3;
            const uint2 mm = *reinterpret_cast<const uint2*>(cmap + ((size_t)q * W16 + i) * 4);
            const unsigned v = (unsigned)row[mm.x & 0xffffu] | ((unsigned)row[mm.x >> 16] << 8) | ((unsigned)row[mm.y & 0xffffu] << 16) |
                               ((unsigned)row[mm.y >> 16] << 24);
            o.x = q == 0 ? v : o.x;
            o.y = q == 1 ? v : o.y;
            o.z = q == 2 ? v : o.z;
            o.w = q == 3 ? v : o.w;
          }
        }
        *reinterpret_cast<uint4*>(outp + (size_t)(y_base + r) * W + 16 * i) = o;
      }
    } else {
      for (int it = tid; it < rows * W; it += AUG_THREADS) {
        const int r = it / W, x = it - r * W;
        unsigned char v = 0;
        if (src_y[r] >= 0) v = stage[(size_t)slot_of[r] * stride + cmap[x]];
        outp[(size_t)(y_base + r) * W + x] = v;
      }
    }
  }
}

// one 64-lane workgroup per label frame: aug_labels_frame (aug_map.cuh) without rotation
__global__ __launch_bounds__(64) void aug_labels_kernel(const float* __restrict__ in, const int* __restrict__ counts,
                                                        const int* __restrict__ params, int B, int M, int W, float* __restrict__ out,
                                                        int* __restrict__ counts_out, float* __restrict__ yolox) {
  aug_labels_frame<false>(in, counts, params, nullptr, B, M, 0, W, out, counts_out, yolox);
}

}  // namespace
}  // namespace sast

extern "C" {

int sast_augment_frames(const uint8_t* in, uint8_t* out, const int32_t* params, int N, int B, int C, int H, int W, sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!in || !out || !params || in == out || N < 1 || B < 1 || C < 1 || H < 1 || W < 1 || H > AUG_MAX_HW || W > AUG_MAX_HW || N > 65535 ||
      C > 65535)
    return SAST_EINVAL;
  const int Wp = (W + 15) & ~15;
  const int rows = std::max(1, std::min(AUG_MAX_ROWS, (AUG_LDS_BUDGET - 2 * Wp) / (Wp + 16)));
  const int bands = (H + rows - 1) / rows;
  const long long per_c = (long long)N * bands;
  const int c_groups = (int)std::min<long long>(C, std::max<long long>(1, (AUG_TARGET_WGS + per_c - 1) / per_c));
  const int ch_per_wg = (C + c_groups - 1) / c_groups;
  const dim3 grid((unsigned)bands, (unsigned)((C + ch_per_wg - 1) / ch_per_wg), (unsigned)N);
  const size_t lds = 2 * (size_t)Wp + (size_t)rows * (Wp + 16);
  const bool vec = (W % 16 == 0) && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16 == 0);
  if (vec)
    SAST_LAUNCH(aug_frames_kernel<true>, grid, dim3(AUG_THREADS), lds, (hipStream_t)stream, in, out, params, B, C, H, W, rows, ch_per_wg);
  else
    SAST_LAUNCH(aug_frames_kernel<false>, grid, dim3(AUG_THREADS), lds, (hipStream_t)stream, in, out, params, B, C, H, W, rows, ch_per_wg);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

int sast_augment_labels(const float* labels, const int32_t* counts, const int32_t* params, int N, int B, int M, int W, float* out,
                        int32_t* counts_out, float* yolox, sast_stream_t stream) {
  SAST_ENTRY();
  using namespace sast;
  if (!labels || !counts || !params || !out || !counts_out || labels == out || counts == counts_out || N < 1 || B < 1 || M < 1 || W < 1 ||
      W > AUG_MAX_HW)
    return SAST_EINVAL;
  SAST_LAUNCH(aug_labels_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, labels, counts, params, B, M, W, out, counts_out,
              yolox);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
