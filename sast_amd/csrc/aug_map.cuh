// The per-sample maps of the spatial augmentation, shared by its two sources: k_augment.hip (flip and zoom: a separable map, whole source
// rows staged in LDS) and k_rotaug.hip (flip, rotation, zoom: a 2-D gather).  Both are built with -ffp-contract=off (build.py,
// SOURCE_FLAGS): every product below is rounded before it is added, as the reference's separate tensor operations round it.
//   aug_sample / nearest_exact / axis_src / col_src   the zoom and flip maps of one axis (data/utils/augmentor.py:134-153, :203-222)
//   rot_sample / rot_src                              torchvision's tensor rotate (NEAREST, expand=False, center=None, fill=None) as one
//                                                     fp32 rounding per operation: the rule of include/sast_hip.h
//   aug_labels_frame<ROT>                             the label transforms of one frame (data/genx_utils/labels.py:210-339); ROT = false
//                                                     is sast_augment_labels, ROT = true adds rotate_ between flip_lr_ and the zooms
#pragma once
#include "common.cuh"
#include "kernels.h"

namespace sast {
namespace {

constexpr int AUG_MAX_HW = 4096;

enum { AUG_NONE = 0, AUG_ZOOM_IN = 1, AUG_ZOOM_OUT = 2 };

struct AugSample {
  int flip, mode, x0, y0, wh, ww;
};

__device__ __forceinline__ AugSample aug_sample(const int* p, int H, int W) {
  AugSample s;
  s.flip = p[0] != 0;
  s.mode = (p[1] == AUG_ZOOM_IN || p[1] == AUG_ZOOM_OUT) ? p[1] : AUG_NONE;
  s.x0 = min(max(p[2], 0), W - 1);
  s.y0 = min(max(p[3], 0), H - 1);
  s.wh = min(max(p[4], 1), H);
  s.ww = min(max(p[5], 1), W);
  return s;
}

// ATen's nearest-exact source index (UpSample.h): min(int(floorf((d + 0.5f) * (float(in) / float(out)))), in - 1), all in fp32
__device__ __forceinline__ int nearest_exact(int d, int in, int out) {
  const float scale = __fdiv_rn((float)in, (float)out);
  return min((int)floorf(__fmul_rn(__fadd_rn((float)d, 0.5f), scale)), in - 1);
}

// source index of output index d along one axis of length `full`; -1: the zero border of zoom-out
__device__ __forceinline__ int axis_src(int d, int mode, int o0, int win, int full) {
  int s = d;
  if (mode == AUG_ZOOM_IN) {
    const int canvas = min(win, full - o0);                  // the slice [o0 : o0 + win] is cut at the frame's edge
    s = o0 + nearest_exact(d, canvas, full);
  } else if (mode == AUG_ZOOM_OUT) {
    if (d < o0 || d >= o0 + win) return -1;
    s = nearest_exact(d - o0, full, win);
  }
  return min(max(s, 0), full - 1);
}

__device__ __forceinline__ int col_src(int x, const AugSample& s, int W) {
  const int c = axis_src(x, s.mode, s.x0, s.ww, W);
  return (c >= 0 && s.flip) ? W - 1 - c : c;
}

// one sample's words of rot_params (SAST_ROTAUG_PARAM_WORDS): a, b, c, d map a pixel of the rotated image to grid_sample's
// normalised coordinates; co, si rotate the label corners
struct RotSample {
  int active;
  float a, b, c, d, co, si;
};

__device__ __forceinline__ RotSample rot_sample(const int* p) {
  RotSample r;
  r.active = p[0] != 0;
  r.a = __int_as_float(p[1]);
  r.b = __int_as_float(p[2]);
  r.c = __int_as_float(p[3]);
  r.d = __int_as_float(p[4]);
  r.co = __int_as_float(p[5]);
  r.si = __int_as_float(p[6]);
  return r;
}

// pixel (y, x) of the rotated image -> its source pixel (*sy, *sx); false: outside the frame (also for NaN / Inf parameters: every
// comparison with a NaN is false), the pixel is 0.  affine_grid's base grid, the 2 x 2 product, grid_sample's unnormalisation
// (align_corners=False) and its nearbyint, each operation rounded once
__device__ __forceinline__ bool rot_src(const RotSample& r, int y, int x, int H, int W, int* sy, int* sx) {
  const float fW = (float)W, fH = (float)H;
  const float bx = __fadd_rn((float)x, __fsub_rn(0.5f, __fmul_rn(0.5f, fW)));      // exact: halves below 2^13
  const float by = __fadd_rn((float)y, __fsub_rn(0.5f, __fmul_rn(0.5f, fH)));
  const float gx = __fadd_rn(__fmul_rn(bx, r.a), __fmul_rn(by, r.b));
  const float gy = __fadd_rn(__fmul_rn(bx, r.c), __fmul_rn(by, r.d));
  const float ix = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gx, 1.f), fW), 1.f), 2.f);
  const float iy = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(gy, 1.f), fH), 1.f), 2.f);
  const float rx = rintf(ix), ry = rintf(iy);                                       // ties to even
  if (!(rx >= 0.f && rx < fW && ry >= 0.f && ry < fH)) return false;
  *sx = (int)rx;
  *sy = (int)ry;
  return true;
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }   // ATen: min(max(v, lo), hi)

// one corner of rotate_ (labels.py:233-235): (points - center) through the 2 x 2 matrix, + center
__device__ __forceinline__ void rot_corner(const RotSample& r, float X, float Y, float cx, float cy, float* ox, float* oy) {
  const float px = __fsub_rn(X, cx), py = __fsub_rn(Y, cy);
  *ox = __fadd_rn(__fadd_rn(__fmul_rn(r.co, px), __fmul_rn(r.si, py)), cx);
  *oy = __fadd_rn(__fadd_rn(__fmul_rn(-r.si, px), __fmul_rn(r.co, py)), cy);
}

// The label rows of frame n, by one 64-lane workgroup.  Every operation is the reference's single fp32 operation on a tensor and a
// scalar the host rounded to fp32 once, in the reference's order, with no contraction (w = x1 - x * s rounds x * s first).
// ROT: rot_params row n % B is read and, where active, rotate_ (labels.py:210-248) runs after flip_lr_ and before the zooms; H is
// used by it alone.
template <bool ROT>
__device__ __forceinline__ void aug_labels_frame(const float* __restrict__ in, const int* __restrict__ counts, const int* __restrict__ params,
                                                 const int* __restrict__ rot_params, int B, int M, int H, int W, float* __restrict__ out,
                                                 int* __restrict__ counts_out, float* __restrict__ yolox) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int* p = params + (size_t)(n % B) * SAST_AUGMENT_PARAM_WORDS;
  const int flip = p[0] != 0;
  const int mode = (p[1] == AUG_ZOOM_IN || p[1] == AUG_ZOOM_OUT) ? p[1] : AUG_NONE;
  const float fx0 = (float)p[2], fy0 = (float)p[3];
  const float lox = __int_as_float(p[8]), hix = __int_as_float(p[9]), loy = __int_as_float(p[10]), hiy = __int_as_float(p[11]);
  const float sc = __int_as_float(p[12]), maxx = __int_as_float(p[13]), maxy = __int_as_float(p[14]);
  const float wm1 = (float)(W - 1);
  RotSample rot = {};
  if (ROT) rot = rot_sample(rot_params + (size_t)(n % B) * SAST_ROTAUG_PARAM_WORDS);
  const int cnt = min(max(counts[n], 0), M);
  const float* src = in + (size_t)n * M * 7;
  float* dst = out + (size_t)n * M * 7;
  float* dsty = yolox ? yolox + (size_t)n * M * 5 : nullptr;
  int kept = 0;
  for (int m0 = 0; m0 < cnt; m0 += 64) {
    const int m = m0 + lane;
    bool keep = m < cnt;
    float t = 0.f, x = 0.f, y = 0.f, w = 0.f, h = 0.f, cls = 0.f, conf = 0.f;
    if (keep) {
      const float* r = src + (size_t)m * 7;
      t = r[0]; x = r[1]; y = r[2]; w = r[3]; h = r[4]; cls = r[5]; conf = r[6];
      if (flip) x = __fsub_rn(__fsub_rn(wm1, x), w);                       // labels.py:339
      if (ROT && rot.active) {                                             // labels.py:217-248
        const float cx = (float)(W / 2), cy = (float)(H / 2), hm1 = (float)(H - 1);
        const float xw = __fadd_rn(x, w), yh = __fadd_rn(y, h);
        float ax, ay, bx, by, cx_, cy_, dx, dy;
        rot_corner(rot, x, y, cx, cy, &ax, &ay);
        rot_corner(rot, xw, y, cx, cy, &bx, &by);
        rot_corner(rot, x, yh, cx, cy, &cx_, &cy_);
        rot_corner(rot, xw, yh, cx, cy, &dx, &dy);
        const float x0 = clampf(fminf(fminf(ax, bx), fminf(cx_, dx)), 0.f, wm1), x1 = clampf(fmaxf(fmaxf(ax, bx), fmaxf(cx_, dx)), 0.f, wm1);
        const float y0 = clampf(fminf(fminf(ay, by), fminf(cy_, dy)), 0.f, hm1), y1 = clampf(fmaxf(fmaxf(ay, by), fmaxf(cy_, dy)), 0.f, hm1);
        x = x0;
        y = y0;
        w = __fsub_rn(x1, x0);
        h = __fsub_rn(y1, y0);
        keep = w > 0.f && h > 0.f;
      }
      if (keep && mode == AUG_ZOOM_IN) {                                   // labels.py:277-289
        const float cx0 = clampf(x, lox, hix), cy0 = clampf(y, loy, hiy);
        const float cx1 = clampf(__fadd_rn(x, w), lox, hix), cy1 = clampf(__fadd_rn(y, h), loy, hiy);
        x = __fsub_rn(cx0, fx0);
        y = __fsub_rn(cy0, fy0);
        w = __fsub_rn(cx1, cx0);
        h = __fsub_rn(cy1, cy0);
        keep = w > 0.f && h > 0.f;
      }
      if (keep && mode != AUG_NONE) {                                      // scale_: labels.py:326-334
        const float x1 = fminf(__fmul_rn(__fadd_rn(x, w), sc), maxx), y1 = fminf(__fmul_rn(__fadd_rn(y, h), sc), maxy);
        x = __fmul_rn(x, sc);
        y = __fmul_rn(y, sc);
        w = __fsub_rn(x1, x);
        h = __fsub_rn(y1, y);
        keep = w > 0.f && h > 0.f;
        if (mode == AUG_ZOOM_OUT) {                                        // labels.py:313-314
          x = __fadd_rn(x, fx0);
          y = __fadd_rn(y, fy0);
        }
      }
    }
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const int at = kept + __popcll(mask & ((1ull << lane) - 1ull));
      float* r = dst + (size_t)at * 7;
      r[0] = t; r[1] = x; r[2] = y; r[3] = w; r[4] = h; r[5] = cls; r[6] = conf;
      if (dsty) {                                                          // labels.py:348-352
        float* q = dsty + (size_t)at * 5;
        q[0] = cls;
        q[1] = __fadd_rn(x, __fmul_rn(0.5f, w));
        q[2] = __fadd_rn(y, __fmul_rn(0.5f, h));
        q[3] = w;
        q[4] = h;
      }
    }
    kept += __popcll(mask);
  }
  for (int i = kept * 7 + lane; i < M * 7; i += 64) dst[i] = 0.f;
  if (dsty)
    for (int i = kept * 5 + lane; i < M * 5; i += 64) dsty[i] = 0.f;
  if (lane == 0) counts_out[n] = kept;
}

}  // namespace
}  // namespace sast
