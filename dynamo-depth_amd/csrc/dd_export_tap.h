// The source tap of the kernels that export a disparity map at the source resolution (dd_export.hip, dd_cloud.hip): the network's
// disparity, or with the flip post-processing ("PP") the fuse of it with the disparity of the mirrored image.  One copy.
// Include it behind `#pragma clang fp contract(off)`: the fuse is defined unfused (hipops/export.py fuse_host).
#pragma once
#include <hip/hip_runtime.h>

namespace dd {

// the fused disparity of source tap (y, x) of one image
template <bool FUSE>
__device__ __forceinline__ float export_tap(const float* __restrict__ l_img, const float* __restrict__ r_img, const float* __restrict__ l_mask, int w, int y, int x) {
  const float l = l_img[(size_t)y * w + x];
  if (!FUSE) return l;
  const float r = r_img[(size_t)y * w + (w - 1 - x)];
  const float m = 0.5f * (l + r);
  const float lm = l_mask[x], rm = l_mask[w - 1 - x];
  return (rm * l + lm * r) + ((1.f - lm) - rm) * m;
}

}  // namespace dd
