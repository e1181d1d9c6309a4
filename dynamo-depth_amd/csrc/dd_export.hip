// Full-resolution depth export (predict.py): the network's (B,1,h,w) sigmoid disparity becomes, at the source image's H x W, the float
// depth map, the 16-bit depth image and the colour-mapped disparity in ONE pass over the output -- what the depth metrics define at
// LiDAR points (reference tools.py:42 F.interpolate(bilinear, align_corners=False) of tools.py:291-298 disp_to_depth, then 1 / x;
// dd_metrics.hip) evaluated at every pixel.  Done with torch operators that is five or six full-resolution passes per frame.
// Per output pixel (b, Y, X), fp32, no fused multiply-add (hipops/export.py export_depth_host is the same arithmetic in
// numpy, bit for bit):
//   fuse      only with the disparity of the mirrored image (flip post-processing, "PP" in the literature), per source tap (y, x):
//             l = disp[y,x], r = disp_flipped[y,w-1-x], m = 0.5*(l+r), lm = l_mask[x], rm = l_mask[w-1-x],
//             d = (rm*l + lm*r) + ((1-lm) - rm)*m;  without it d = disp[y,x]
//   scale     s = lo + span*d, lo = 1/max_depth, span = 1/min_depth - 1/max_depth (depth_params of dd_math.h, as dd_ops.hip)
//   upsample  u = dm_blend over the four s taps of dm_tap (dd_bilinear.h), d_up = the same blend of the four d taps
//   outputs   depth = 1/u;  depth16 = min(rint(depth*depth_scale), 65535), 0 for NaN and below 1;  rgb = lut[vis_cmap_index(d_up)]
// dd_export_plane_u8: the same upsample of a plane, then vis_unit_byte (the motion mask).
// The kernel is bound by its stores (13 B per pixel against a source map of a few hundred KB that stays in cache): a lane owns four
// horizontally adjacent pixels = one 16-byte, one 8-byte and three 4-byte stores where the row's address allows, narrow stores else
// (unaligned rows, W % 4 != 0).  A workgroup works on one output row at a time: the vertical taps and weight are wave-uniform.
// No LDS, no atomics: every output byte is the same from run to run.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

// in front of the shared headers: dm_blend and vis_cmap_index are compiled unfused in this file
#pragma clang fp contract(off)

#include "dd_bilinear.h"
#include "dd_export_tap.h"
#include "dd_math.h"
#include "dd_vis.h"

namespace dd {

constexpr int EX_NT = 256;
constexpr int EX_MAX_ROWS = 65535;      // grid.y; more rows than that are walked by a stride loop

struct ExportArgs {
  const float *disp, *flip, *l_mask;
  const uint32_t* lut;
  float* depth;
  uint16_t* depth16;
  uint8_t* rgb;
  int h, w, H, W;
  long long rows;                       // B * H
  float sy, sx, depth_scale, vmin, vmax;
  DepthParams dp;
};

__device__ __forceinline__ void export_store4h(uint16_t* p, int valid, const unsigned (&v)[4]) {
  if (valid == 4 && ((uintptr_t)p & 7u) == 0u) {
    *reinterpret_cast<uint2*>(p) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < valid) p[k] = (uint16_t)v[k];
  }
}

__device__ __forceinline__ void export_store4b(uint8_t* p, int valid, const unsigned (&v)[4]) {
  if (valid == 4 && ((uintptr_t)p & 3u) == 0u) {
    *reinterpret_cast<unsigned*>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < valid) p[k] = (uint8_t)v[k];
  }
}

// grid (ceil(W/4 / EX_NT), min(B*H, EX_MAX_ROWS)): blockIdx.y walks the output rows of the batch
template <bool FUSE>
__global__ __launch_bounds__(EX_NT) void export_depth_kernel(const ExportArgs a) {
  const int X0 = (blockIdx.x * EX_NT + threadIdx.x) * 4;
  if (X0 >= a.W) return;
  const int valid = min(4, a.W - X0);
  const int h = a.h, w = a.w, H = a.H, W = a.W;
  // the horizontal taps do not depend on the row
  int x0[4], x1[4];
  float wx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) dm_tap(min(X0 + k, W - 1), a.sx, w, x0[k], x1[k], wx[k]);
  for (long long row = blockIdx.y; row < a.rows; row += gridDim.y) {
    const int b = (int)(row / H), Y = (int)(row - (long long)b * H);
    int y0, y1;
    float wy;
    dm_tap(Y, a.sy, h, y0, y1, wy);
    const float* l_img = a.disp + (size_t)b * h * w;
    const float* r_img = FUSE ? a.flip + (size_t)b * h * w : nullptr;
    float dep[4];
    unsigned q16[4], px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d00 = export_tap<FUSE>(l_img, r_img, a.l_mask, w, y0, x0[k]), d01 = export_tap<FUSE>(l_img, r_img, a.l_mask, w, y0, x1[k]);
      const float d10 = export_tap<FUSE>(l_img, r_img, a.l_mask, w, y1, x0[k]), d11 = export_tap<FUSE>(l_img, r_img, a.l_mask, w, y1, x1[k]);
      const float u = dm_blend(wy, wx[k], a.dp.lo + a.dp.span * d00, a.dp.lo + a.dp.span * d01, a.dp.lo + a.dp.span * d10, a.dp.lo + a.dp.span * d11);
      dep[k] = 1.f / u;
      const float r = rintf(dep[k] * a.depth_scale);                    // half to even
      q16[k] = r >= 1.f ? (unsigned)fminf(r, 65535.f) : 0u;             // NaN and everything below 1 -> 0
      px[k] = 0u;
      if (a.rgb) {
        const int i = vis_cmap_index(dm_blend(wy, wx[k], d00, d01, d10, d11), a.vmin, a.vmax);
        if (i >= 0) px[k] = a.lut[i];
      }
    }
    const size_t at = (size_t)row * W + X0;
    if (a.depth) vis_store4f(a.depth + at, valid, dep);
    if (a.depth16) export_store4h(a.depth16 + at, valid, q16);
    if (a.rgb) vis_store4px(a.rgb + at * 3, valid, px);
  }
}

__global__ __launch_bounds__(EX_NT) void export_plane_u8_kernel(const float* __restrict__ plane, int h, int w, int H, int W, long long rows, float sy, float sx,
                                                                uint8_t* __restrict__ out) {
  const int X0 = (blockIdx.x * EX_NT + threadIdx.x) * 4;
  if (X0 >= W) return;
  const int valid = min(4, W - X0);
  int x0[4], x1[4];
  float wx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) dm_tap(min(X0 + k, W - 1), sx, w, x0[k], x1[k], wx[k]);
  for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
    const int b = (int)(row / H), Y = (int)(row - (long long)b * H);
    int y0, y1;
    float wy;
    dm_tap(Y, sy, h, y0, y1, wy);
    const float* top = plane + ((size_t)b * h + y0) * w;
    const float* bot = plane + ((size_t)b * h + y1) * w;
    unsigned v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = vis_unit_byte(dm_blend(wy, wx[k], top[x0[k]], top[x1[k]], bot[x0[k]], bot[x1[k]]));
    export_store4b(out + (size_t)row * W + X0, valid, v);
  }
}

// host: the sizes both entry points accept, and their grid
static bool export_sizes(int B, int h, int w, int H, int W) {
  return B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL && (long long)h * w <= 0x7fffffffLL;
}

static dim3 export_grid(int B, int H, int W) {
  const long long rows = (long long)B * H;
  return dim3(((W + 3) / 4 + EX_NT - 1) / EX_NT, (unsigned)(rows < EX_MAX_ROWS ? rows : EX_MAX_ROWS));
}

}  // namespace dd

using namespace dd;

extern "C" int dd_export_depth(const float* disp, const float* disp_flipped, const float* l_mask, int B, int h, int w, int H, int W, float min_depth,
                               float max_depth, float depth_scale, const uint32_t* lut, float vmin, float vmax, float* depth, uint16_t* depth16, uint8_t* rgb,
                               void* stream) {
  if (!disp || (disp_flipped == nullptr) != (l_mask == nullptr) || (lut == nullptr) != (rgb == nullptr) || (!depth && !depth16 && !rgb))
    return (int)hipErrorInvalidValue;
  if (!export_sizes(B, h, w, H, W) || !(min_depth > 0.f) || !(max_depth > 0.f)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)disp & 3u) || ((uintptr_t)disp_flipped & 3u) || ((uintptr_t)l_mask & 3u) || ((uintptr_t)lut & 3u) || ((uintptr_t)depth & 3u) ||
      ((uintptr_t)depth16 & 1u))
    return (int)hipErrorInvalidValue;
  ExportArgs a;
  a.disp = disp, a.flip = disp_flipped, a.l_mask = l_mask, a.lut = lut, a.depth = depth, a.depth16 = depth16, a.rgb = rgb;
  a.h = h, a.w = w, a.H = H, a.W = W, a.rows = (long long)B * H;
  // ATen's area_pixel_compute_scale: the ratio in fp32
  a.sy = (float)h / (float)H, a.sx = (float)w / (float)W;
  a.depth_scale = depth_scale, a.vmin = vmin, a.vmax = vmax;
  a.dp = depth_params(min_depth, max_depth);
  if (disp_flipped)
    hipLaunchKernelGGL(export_depth_kernel<true>, export_grid(B, H, W), dim3(EX_NT), 0, static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(export_depth_kernel<false>, export_grid(B, H, W), dim3(EX_NT), 0, static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

extern "C" int dd_export_plane_u8(const float* plane, int B, int h, int w, int H, int W, uint8_t* out, void* stream) {
  if (!plane || !out || !export_sizes(B, h, w, H, W) || ((uintptr_t)plane & 3u)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(export_plane_u8_kernel, export_grid(B, H, W), dim3(EX_NT), 0, static_cast<hipStream_t>(stream), plane, h, w, H, W, (long long)B * H,
                     (float)h / (float)H, (float)w / (float)W, out);
  return (int)hipGetLastError();
}
