// F.interpolate(..., mode='bilinear', align_corners=False) as ATen evaluates it in fp32: the source tap of a destination index
// and the four-tap blend.  One copy for the kernels that sample a low-resolution map at ground-truth pixels
// (dd_metrics.hip, dd_motion_pr.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace dd {

// source tap of destination index d (ATen: scale = in/out in float, src = max(scale*(d+0.5)-0.5, 0))
__device__ __forceinline__ void dm_tap(int d, float scale, int in_size, int& i0, int& i1, float& w1) {
  float src = scale * (static_cast<float>(d) + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = static_cast<int>(src);
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  w1 = src - static_cast<float>(i0);
}

// ATen's upsample_bilinear2d: w0 = 1 - w1; value = wy0*(wx0*a + wx1*b) + wy1*(wx0*c + wx1*d), (a b) the upper and (c d) the lower taps
__device__ __forceinline__ float dm_blend(float wy, float wx, float a, float b, float c, float d) {
  const float top = (1.f - wx) * a + wx * b;
  const float bot = (1.f - wx) * c + wx * d;
  return (1.f - wy) * top + wy * bot;
}

}  // namespace dd
