// Segment visualisation panels (reference eval/visualize.py:24-124 get_vis / combine_vis, on Trainer.py:574-605 vis_motion and
// utils.py:103-164 cart2polar / hsv_to_rgb / score_map_vis): per frame the tiles image | disparity | ego flow | independent flow |
// motion mask, as bytes, written where the video frame will be read from.  The reference runs ~60 small torch launches and a
// .max().item() per vis_motion call, keeps every frame's float tensors until the segment ends (the flow brightness is normalised by
// the largest flow magnitude of the whole segment) and then colours every tile on the host.  Here: two streaming kernels.
//   pass 1 (dd_vis_frame, once per frame)      the tiles that do not depend on the segment maximum go straight into the panel; for
//                                              every flow tile the pixel's magnitude and hue go to two fp32 planes of a side buffer,
//                                              and the frame's largest magnitude is folded into device-side running maxima
//   pass 2 (dd_vis_flow_tiles, once per segment) reads the maximum FROM DEVICE MEMORY and colours every frame's flow tiles
// A panel is (N, R*H, C*W, 3) uint8 RGB; a thread owns four adjacent pixels of a tile row = 12 contiguous bytes, stored as three
// dwords where the address allows (the row stride C*W*3 is not generally a multiple of 4: the address is tested), byte-wise else.
// Magnitudes are non-negative, so their order is the order of their bit patterns: per wave a shuffle maximum, then one integer
// atomicMax -- order-independent, hence run-to-run identical.  Floating-point contraction is off in this file: the difference of two
// projections must be exactly zero where both are the same arithmetic on the same numbers (a static scene is white, not noise).
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

#pragma STDC FP_CONTRACT OFF

#include "dd_vis.h"      // after the pragma: the shared helpers are compiled unfused here as well

namespace dd {

constexpr int VIS_NT = 64;          // one wave per workgroup: the maximum is one shuffle tree and one atomic pair
// the constants as torch hands them to fp32 arithmetic: evaluated in double, rounded once
constexpr double VIS_PI_D = 3.141592653589793;
constexpr float VIS_PI = (float)VIS_PI_D, VIS_2PI = (float)(2 * VIS_PI_D), VIS_5PI_2 = (float)(5 * VIS_PI_D / 2), VIS_PI_4 = (float)(VIS_PI_D / 4);

struct VisTiles {
  int n, n_flow;
  unsigned char kind[DD_VIS_MAX_TILES], row[DD_VIS_MAX_TILES], col[DD_VIS_MAX_TILES];
  unsigned char flow_tile[DD_VIS_MAX_TILES];        // flow slot -> tile index (the slots count the flow tiles in list order)
};

struct VisFrameArgs {
  const float *color, *ref_color, *disp, *motion_mask, *complete_flow, *K, *inv_K, *T;
  const unsigned* lut;                              // [2][256] r | g << 8 | b << 16: disparity map, mask map
  float min_disp, disp_range, disp_vmin, disp_vmax, mask_vmin, mask_vmax;
  int H, W, R, C, frame;
  uint8_t* panel;                                   // this frame's (R*H, C*W, 3)
  float* side;                                      // this frame's (n_flow, 2, H, W)
  unsigned* maxima;                                 // [0] the segment's, [1 + frame] the frame's
  VisTiles tiles;
};

// Python's % for a positive modulus (torch.remainder)
__device__ __forceinline__ float vis_mod(float a, float b) {
  float r = fmodf(a, b);
  if (r < 0.f) r += b;
  return r;
}

// four adjacent floats of a plane; lanes past the row's end read nothing
__device__ __forceinline__ void vis_load4(const float* p, int valid, float (&v)[4]) {
  if (valid == 4 && ((uintptr_t)p & 15u) == 0u) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < valid ? p[k] : 0.f;
  }
}

__device__ __forceinline__ uint8_t* vis_tile_row(uint8_t* panel, int row, int col, int y, int x, int H, int W, int C) {
  return panel + (((size_t)row * H + y) * ((size_t)C * W) + (size_t)col * W + x) * 3;
}

// tools.py Project3D without the transform: K[:3, :] . q, pinhole division, to [-1, 1]
__device__ __forceinline__ void vis_project(const float* K, const float (&q)[4], float wm1, float hm1, float& px, float& py) {
  const float cx = K[0] * q[0] + K[1] * q[1] + K[2] * q[2] + K[3] * q[3];
  const float cy = K[4] * q[0] + K[5] * q[1] + K[6] * q[2] + K[7] * q[3];
  const float cz = K[8] * q[0] + K[9] * q[1] + K[10] * q[2] + K[11] * q[3];
  const float z = cz + 1e-7f;
  px = ((cx / z) / wm1 - 0.5f) * 2.f;
  py = ((cy / z) / hm1 - 0.5f) * 2.f;
}

__device__ __forceinline__ void vis_transform(const float* T, const float (&p)[4], float (&q)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = T[4 * r] * p[0] + T[4 * r + 1] * p[1] + T[4 * r + 2] * p[2] + T[4 * r + 3] * p[3];
}

__global__ __launch_bounds__(VIS_NT) void vis_frame_kernel(VisFrameArgs a) {
  const int H = a.H, W = a.W;
  const int G = (W + 3) >> 2;
  const int g = blockIdx.x * VIS_NT + threadIdx.x;
  float tmax = 0.f;
  if (g < H * G) {
    const int y = g / G, x0 = (g - y * G) * 4;
    const int valid = min(4, W - x0);
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x0;

    // the geometry every flow tile shares: the back-projected point, its projection's offset from the identity grid, the ego motion
    float P[4][3], ego[4][3], err[4][2], idn[4][2], mk[4], cf[3][4];
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    if (a.tiles.n_flow > 0) {
      float d[4];
      vis_load4(a.disp + pix, valid, d);
      const bool need_motion = a.motion_mask != nullptr && a.complete_flow != nullptr;
      if (need_motion) {
        vis_load4(a.motion_mask + pix, valid, mk);
#pragma unroll
        for (int c = 0; c < 3; ++c) vis_load4(a.complete_flow + c * plane + pix, valid, cf[c]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) mk[k] = cf[0][k] = cf[1][k] = cf[2][k] = 0.f;
      }
      const float* iK = a.inv_K;
      const float fy = (float)y;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float fx = (float)(x0 + k);
        const float depth = 1.f / (a.min_disp + a.disp_range * d[k]);
        float p4[4], q4[4];
#pragma unroll
        for (int r = 0; r < 3; ++r) p4[r] = P[k][r] = depth * (iK[4 * r] * fx + iK[4 * r + 1] * fy + iK[4 * r + 2] * 1.f);
        p4[3] = 1.f;
        idn[k][0] = fx / (float)W * 2.f - 1.f;
        idn[k][1] = fy / (float)H * 2.f - 1.f;
        float px, py;
        vis_project(a.K, p4, wm1, hm1, px, py);
        err[k][0] = px - idn[k][0], err[k][1] = py - idn[k][1];
        vis_transform(a.T, p4, q4);
#pragma unroll
        for (int r = 0; r < 3; ++r) ego[k][r] = q4[r] - P[k][r];
      }
    }

    int slot = 0;
    for (int t = 0; t < a.tiles.n; ++t) {
      const int kind = a.tiles.kind[t];
      uint8_t* dst = vis_tile_row(a.panel, a.tiles.row[t], a.tiles.col[t], y, x0, H, W, a.C);
      if (kind == DD_VIS_IMG || kind == DD_VIS_REF_IMG) {
        const float* src = (kind == DD_VIS_IMG ? a.color : a.ref_color) + pix;
        float ch[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) vis_load4(src + c * plane, valid, ch[c]);
        unsigned px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = vis_unit_byte(ch[0][k]) | (vis_unit_byte(ch[1][k]) << 8) | (vis_unit_byte(ch[2][k]) << 16);
        vis_store4px(dst, valid, px);
      } else if (kind == DD_VIS_DISP || kind == DD_VIS_MASK) {
        const bool is_disp = kind == DD_VIS_DISP;
        float v[4];
        vis_load4((is_disp ? a.disp : a.motion_mask) + pix, valid, v);
        const unsigned* lut = a.lut + (is_disp ? 0 : 256);
        const float vmin = is_disp ? a.disp_vmin : a.mask_vmin, vmax = is_disp ? a.disp_vmax : a.mask_vmax;
        unsigned px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int i = vis_cmap_index(v[k], vmin, vmax);
          px[k] = i < 0 ? 0u : lut[i];
        }
        vis_store4px(dst, valid, px);
      } else {
        // motion map: none (ego), the complete flow (comp), mask * (complete flow - ego motion) (ind, samp); T for ego and samp
        const bool use_T = kind == DD_VIS_EGO_FLOW || kind == DD_VIS_SAMP_FLOW;
        float mag[4], hue[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float q[4], moved[4];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            float m = 0.f;
            if (kind == DD_VIS_COMP_FLOW) m = cf[r][k];
            if (kind == DD_VIS_IND_FLOW || kind == DD_VIS_SAMP_FLOW) m = mk[k] * (cf[r][k] - ego[k][r]);
            q[r] = kind == DD_VIS_EGO_FLOW ? P[k][r] : P[k][r] + m;
          }
          q[3] = 1.f;
          float px, py;
          if (use_T) {
            vis_transform(a.T, q, moved);
            vis_project(a.K, moved, wm1, hm1, px, py);
          } else {
            vis_project(a.K, q, wm1, hm1, px, py);
          }
          const float rx = (px - idn[k][0]) - err[k][0], ry = (py - idn[k][1]) - err[k][1];
          mag[k] = sqrtf(rx * rx + ry * ry);
          // utils.cart2polar on (x, y): it names them "y, x" and divides the first by the second
          float th = atanf(rx / ry);
          if (th != th) th = 0.f;
          if (ry < 0.f) th = th + VIS_PI;
          th = vis_mod(VIS_5PI_2 - th, VIS_2PI);
          hue[k] = vis_mod(th - VIS_PI_4, VIS_2PI) / VIS_2PI;
          if (k < valid) tmax = fmaxf(tmax, mag[k]);
        }
        float* s = a.side + (size_t)slot * 2 * plane + pix;      // the slots count the flow tiles in list order
        vis_store4f(s, valid, mag);
        vis_store4f(s + plane, valid, hue);
        ++slot;
      }
    }
  }
  if (a.tiles.n_flow > 0) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, off));
    if (threadIdx.x == 0) {
      const unsigned bits = __float_as_uint(tmax);
      atomicMax(a.maxima, bits);
      atomicMax(a.maxima + 1 + a.frame, bits);
    }
  }
}

// grid (row groups, flow slot, frame)
__global__ __launch_bounds__(VIS_NT) void vis_flow_tiles_kernel(const float* __restrict__ side, const unsigned* __restrict__ maxima, VisTiles tiles, int R, int C,
                                                                int H, int W, float factor, int consistent, uint8_t* __restrict__ panel) {
  const int G = (W + 3) >> 2;
  const int g = blockIdx.x * VIS_NT + threadIdx.x;
  if (g >= H * G) return;
  const int slot = blockIdx.y, n = blockIdx.z;
  const int t = tiles.flow_tile[slot];
  const int y = g / G, x0 = (g - y * G) * 4;
  const int valid = min(4, W - x0);
  const size_t plane = (size_t)H * W, pix = (size_t)y * W + x0;
  const float top = factor * (__uint_as_float(maxima[consistent ? 0 : 1 + n]) + 1e-8f);
  const float* s = side + ((size_t)n * tiles.n_flow + slot) * 2 * plane + pix;
  float mag[4], hue[4];
  vis_load4(s, valid, mag);
  vis_load4(s + plane, valid, hue);
  unsigned px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float v = fminf(fmaxf(mag[k] / top, 0.f), 1.f);
    // utils.hsv_to_rgb at saturation 1
    const float h6 = hue[k] * 6.f;
    const float hi = vis_mod(floorf(h6), 6.f);
    const float f = vis_mod(h6, 6.f) - hi;
    const float p = v * (1.f - 1.f), q = v * (1.f - f * 1.f), u = v * (1.f - (1.f - f) * 1.f);
    const int sec = (int)hi;
    const float r = sec == 0 ? v : sec == 1 ? q : sec == 2 ? p : sec == 3 ? p : sec == 4 ? u : v;
    const float gg = sec == 0 ? u : sec == 1 ? v : sec == 2 ? v : sec == 3 ? q : sec == 4 ? p : p;
    const float b = sec == 0 ? p : sec == 1 ? p : sec == 2 ? u : sec == 3 ? v : sec == 4 ? v : q;
    px[k] = (unsigned)((1.f - r) * 255.f) | ((unsigned)((1.f - gg) * 255.f) << 8) | ((unsigned)((1.f - b) * 255.f) << 16);
  }
  uint8_t* frame = panel + (size_t)n * R * H * C * W * 3;
  vis_store4px(vis_tile_row(frame, tiles.row[t], tiles.col[t], y, x0, H, W, C), valid, px);
}

// host: the tile list (kind, row, col triples) into the by-value record; false when it is not a list of tiles inside R x C
static bool vis_tiles(const int* list, int n_tiles, int R, int C, VisTiles* out) {
  if (!list || n_tiles < 1 || n_tiles > DD_VIS_MAX_TILES || R < 1 || C < 1 || R > 255 || C > 255) return false;
  out->n = n_tiles, out->n_flow = 0;
  for (int t = 0; t < DD_VIS_MAX_TILES; ++t) out->kind[t] = out->row[t] = out->col[t] = out->flow_tile[t] = 0;
  for (int t = 0; t < n_tiles; ++t) {
    const int kind = list[3 * t], row = list[3 * t + 1], col = list[3 * t + 2];
    if (kind < DD_VIS_IMG || kind > DD_VIS_SAMP_FLOW || row < 0 || row >= R || col < 0 || col >= C) return false;
    out->kind[t] = (unsigned char)kind, out->row[t] = (unsigned char)row, out->col[t] = (unsigned char)col;
    if (kind >= DD_VIS_EGO_FLOW) out->flow_tile[out->n_flow++] = (unsigned char)t;
  }
  return true;
}

}  // namespace dd

using namespace dd;

extern "C" int dd_vis_frame(const float* color, const float* ref_color, const float* disp, const float* motion_mask, const float* complete_flow,
                            const float* K, const float* inv_K, const float* cam_T_cam, float min_depth, float max_depth, int H, int W, const int* tiles,
                            int n_tiles, int R, int C, const uint32_t* lut, float disp_vmin, float disp_vmax, float mask_vmin, float mask_vmax, int frame,
                            int max_frames, uint8_t* panel, float* side, float* maxima, void* stream) {
  VisFrameArgs a;
  if (!vis_tiles(tiles, n_tiles, R, C, &a.tiles)) return (int)hipErrorInvalidValue;
  if (!panel || !maxima || H < 1 || W < 1 || max_frames < 1 || frame < 0 || frame >= max_frames || !(min_depth > 0.f) || !(max_depth > 0.f))
    return (int)hipErrorInvalidValue;
  if ((long long)H * ((W + 3) / 4) > 0x7fffffffLL - VIS_NT) return (int)hipErrorInvalidValue;
  for (int t = 0; t < n_tiles; ++t) {                    // every plane a listed tile reads
    const int kind = a.tiles.kind[t];
    const bool motion = kind == DD_VIS_IND_FLOW || kind == DD_VIS_COMP_FLOW || kind == DD_VIS_SAMP_FLOW;
    if ((kind == DD_VIS_IMG && !color) || (kind == DD_VIS_REF_IMG && !ref_color) || (kind == DD_VIS_DISP && (!disp || !lut)) ||
        (kind == DD_VIS_MASK && (!motion_mask || !lut)) || (kind >= DD_VIS_EGO_FLOW && (!disp || !K || !inv_K || !cam_T_cam || !side)) ||
        (motion && (!motion_mask || !complete_flow)))
      return (int)hipErrorInvalidValue;
  }
  a.color = color, a.ref_color = ref_color, a.disp = disp, a.motion_mask = motion_mask, a.complete_flow = complete_flow;
  a.K = K, a.inv_K = inv_K, a.T = cam_T_cam, a.lut = lut;
  // tools.disp_to_depth: the two constants in double, the per-pixel arithmetic in fp32
  const double min_disp = 1.0 / (double)max_depth, max_disp = 1.0 / (double)min_depth;
  a.min_disp = (float)min_disp, a.disp_range = (float)(max_disp - min_disp);
  a.disp_vmin = disp_vmin, a.disp_vmax = disp_vmax, a.mask_vmin = mask_vmin, a.mask_vmax = mask_vmax;
  a.H = H, a.W = W, a.R = R, a.C = C, a.frame = frame;
  const size_t plane = (size_t)H * W;
  a.panel = panel + (size_t)frame * R * C * plane * 3;
  a.side = side ? side + (size_t)frame * a.tiles.n_flow * 2 * plane : nullptr;
  a.maxima = reinterpret_cast<unsigned*>(maxima);
  const int groups = H * ((W + 3) / 4);
  hipLaunchKernelGGL(vis_frame_kernel, dim3((groups + VIS_NT - 1) / VIS_NT), dim3(VIS_NT), 0, static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

extern "C" int dd_vis_flow_tiles(const float* side, const float* maxima, const int* tiles, int n_tiles, int R, int C, int H, int W, int n_frames,
                                 float flow_mag_factor, int consistent_flow, uint8_t* panel, void* stream) {
  VisTiles vt;
  if (!vis_tiles(tiles, n_tiles, R, C, &vt)) return (int)hipErrorInvalidValue;
  if (!panel || !maxima || H < 1 || W < 1 || n_frames < 1 || n_frames > 65535) return (int)hipErrorInvalidValue;
  if ((long long)H * ((W + 3) / 4) > 0x7fffffffLL - VIS_NT) return (int)hipErrorInvalidValue;
  if (vt.n_flow == 0) return (int)hipSuccess;           // nothing depends on the maximum
  if (!side) return (int)hipErrorInvalidValue;
  const int groups = H * ((W + 3) / 4);
  hipLaunchKernelGGL(vis_flow_tiles_kernel, dim3((groups + VIS_NT - 1) / VIS_NT, vt.n_flow, n_frames), dim3(VIS_NT), 0, static_cast<hipStream_t>(stream), side,
                     reinterpret_cast<const unsigned*>(maxima), vt, R, C, H, W, flow_mag_factor, consistent_flow ? 1 : 0, panel);
  return (int)hipGetLastError();
}
