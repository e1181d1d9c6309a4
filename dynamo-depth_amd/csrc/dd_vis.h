// What the kernels that write image bytes share (dd_vis.hip, dd_export.hip): the byte of a unit-range value, the colour-map entry of
// a value, and the four-pixel stores of a lane that owns four horizontally adjacent pixels.  One copy.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace dd {

__device__ __forceinline__ unsigned vis_unit_byte(float x) { return (unsigned)(fminf(fmaxf(x, 0.f), 1.f) * 255.f); }

// matplotlib's Normalize + Colormap.__call__ on fp32 data: the entry of the 256-entry table, -1 for NaN (black)
__device__ __forceinline__ int vis_cmap_index(float x, float vmin, float vmax) {
  const float s = ((x - vmin) / (vmax - vmin)) * 256.f;
  if (s != s) return -1;
  if (s < 0.f) return 0;
  if (s >= 256.f) return 255;
  return (int)s;
}

__device__ __forceinline__ void vis_store4f(float* p, int valid, const float (&v)[4]) {
  if (valid == 4 && ((uintptr_t)p & 15u) == 0u) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < valid) p[k] = v[k];
  }
}

// four pixels r | g << 8 | b << 16 -> 12 bytes at dst
__device__ __forceinline__ void vis_store4px(uint8_t* dst, int valid, const unsigned (&c)[4]) {
  if (valid == 4 && ((uintptr_t)dst & 3u) == 0u) {
    unsigned* d = reinterpret_cast<unsigned*>(dst);
    d[0] = c[0] | (c[1] << 24);
    d[1] = (c[1] >> 8) | (c[2] << 16);
    d[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < valid) dst[3 * k] = (uint8_t)(c[k] & 255u), dst[3 * k + 1] = (uint8_t)((c[k] >> 8) & 255u), dst[3 * k + 2] = (uint8_t)((c[k] >> 16) & 255u);
  }
}

}  // namespace dd
