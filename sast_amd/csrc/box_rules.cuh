// The two box rules more than one translation unit applies, each held once: filter_boxes of the Prophesee evaluation (k_eval.hip,
// k_trackeval.hip) and the tracker's fp32 IoU (k_track.hip, k_trackeval.hip).  Every fp32 operation is one rounding: the files that
// include this header are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace sast {

constexpr long long EV_SKIP_US = 500000;   // filter_boxes drops everything at or before 0.5 s (io/box_filtering.py:18-36)

__device__ __forceinline__ bool box_passes(float w, float h, float diag2, float side) {
  const float d = w * w + h * h;   // fp32, one rounding each (box_filtering.py:34)
  return d >= diag2 && w >= side && h >= side;
}

__device__ __forceinline__ bool label_passes(const float* r, float diag2, float side) {
  return (long long)r[0] > EV_SKIP_US && box_passes(r[3], r[4], diag2, side);
}

// NaN when either side is NaN (fminf / fmaxf would drop it): a box with a NaN never passes the threshold
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (b < a ? b : a); }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (b > a ? b : a); }

__device__ __forceinline__ float track_iou(const float4 a, const float4 b) {   // (x, y, w, h) each
  const float ax2 = a.x + a.z, ay2 = a.y + a.w, bx2 = b.x + b.z, by2 = b.y + b.w;
  const float iw = nan_max(0.f, nan_min(ax2, bx2) - nan_max(a.x, b.x));
  const float ih = nan_max(0.f, nan_min(ay2, by2) - nan_max(a.y, b.y));
  const float inter = iw * ih;
  const float uni = a.z * a.w + b.z * b.w - inter;
  return uni > 0.f ? inter / uni : 0.f;
}

}  // namespace sast
