// Lens undistortion of a batch of frames that share one calibration (reference prepare_data/waymo.py:10-27: cv2.undistort with the
// new camera matrix equal to the old one).  The definition (hipops/undistort.py undistort_host) for destination pixel
// (u, v) and the intrinsic (f_u, f_v, c_u, c_v, k1, k2, p1, p2, k3), float64, one rounding per operation, in exactly this order:
//   x = (u - c_u) / f_u,  y = (v - c_v) / f_v,  xx = x * x,  yy = y * y,  r2 = xx + yy
//   k = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
//   x_d = (x * k + ((2 * p1) * x) * y) + p2 * (r2 + 2 * xx)
//   y_d = (y * k + p1 * (r2 + 2 * yy)) + ((2 * p2) * x) * y
//   m_x = f_u * x_d + c_u,  m_y = f_v * y_d + c_v
//   i_x = rint(m_x * 32), i_y = rint(m_y * 32), halves to even; a value outside [-2^30, 2^30] or a NaN reads as -2^30
// then in integers: taps at (i_x >> 5, i_y >> 5) and its right, lower and lower-right neighbours with the weights (32 - a)(32 - b),
// a (32 - b), (32 - a) b, a b for a = i_x & 31, b = i_y & 31; a tap outside the image counts as 0; dst = (sum + 512) >> 10.
// The file is compiled without contraction, so the map is the numpy definition's bit for bit, and the rest is exact.
// One launch: a thread computes the map of four neighbouring pixels of a row once and serves them in every frame of the batch (a
// stored map would be 8 bytes per pixel against 3 of image); their 12 bytes leave as three dwords where the width allows it.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

#pragma clang fp contract(off)

namespace dd {

constexpr int UD_BX = 64, UD_BY = 4;

struct UDCal {
  double fu, fv, cu, cv, k1, k2, p1, p2, k3;
};

__device__ __forceinline__ int ud_fix(double t) {
  return (t >= -1073741824.0 && t <= 1073741824.0) ? (int)t : -1073741824;
}

__device__ __forceinline__ void ud_map(const UDCal& k, int u, int v, int& ix, int& iy) {
  const double x = ((double)u - k.cu) / k.fu, y = ((double)v - k.cv) / k.fv;
  const double xx = x * x, yy = y * y;
  const double r2 = xx + yy;
  const double kr = 1.0 + ((k.k3 * r2 + k.k2) * r2 + k.k1) * r2;
  const double xd = (x * kr + ((2.0 * k.p1) * x) * y) + k.p2 * (r2 + 2.0 * xx);
  const double yd = (y * kr + k.p1 * (r2 + 2.0 * yy)) + ((2.0 * k.p2) * x) * y;
  const double mx = k.fu * xd + k.cu, my = k.fv * yd + k.cv;
  ix = ud_fix(rint(mx * 32.0));
  iy = ud_fix(rint(my * 32.0));
}

__global__ __launch_bounds__(UD_BX * UD_BY) void undistort_kernel(const unsigned char* __restrict__ src, int n, int H, int W, UDCal cal,
                                                                  unsigned char* __restrict__ dst, int dwords) {
  const int u0 = 4 * (blockIdx.x * UD_BX + threadIdx.x), v = blockIdx.y * UD_BY + threadIdx.y;
  if (u0 >= W || v >= H) return;
  int off[4], wt[4][4];                                           // first tap's pixel index; weights, 0 for a tap outside the image
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int ix, iy;
    ud_map(cal, u0 + j, v, ix, iy);
    const int sx = ix >> 5, sy = iy >> 5, a = ix & 31, b = iy & 31;
    const bool x0 = sx >= 0 && sx < W, x1 = sx >= -1 && sx < W - 1, y0 = sy >= 0 && sy < H, y1 = sy >= -1 && sy < H - 1;
    wt[j][0] = x0 && y0 ? (32 - a) * (32 - b) : 0;
    wt[j][1] = x1 && y0 ? a * (32 - b) : 0;
    wt[j][2] = x0 && y1 ? (32 - a) * b : 0;
    wt[j][3] = x1 && y1 ? a * b : 0;
    off[j] = (x0 || x1) && (y0 || y1) ? sy * W + sx : 0;          // every read below is guarded by its weight
  }
  const size_t frame = (size_t)H * W * 3;
  for (int f = 0; f < n; ++f) {
    const unsigned char* s = src + (size_t)f * frame;
    unsigned char o[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int acc[3] = {512, 512, 512};
      if (u0 + j < W) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (wt[j][t]) {
            const unsigned char* p = s + 3 * ((long long)off[j] + (t & 1) + (t >> 1) * W);
            acc[0] += wt[j][t] * p[0], acc[1] += wt[j][t] * p[1], acc[2] += wt[j][t] * p[2];
          }
        }
      }
      o[3 * j] = (unsigned char)(acc[0] >> 10), o[3 * j + 1] = (unsigned char)(acc[1] >> 10), o[3 * j + 2] = (unsigned char)(acc[2] >> 10);
    }
    unsigned char* d = dst + (size_t)f * frame + 3 * ((size_t)v * W + u0);
    if (dwords) {
      unsigned* d4 = reinterpret_cast<unsigned*>(d);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        d4[k] = (unsigned)o[4 * k] | ((unsigned)o[4 * k + 1] << 8) | ((unsigned)o[4 * k + 2] << 16) | ((unsigned)o[4 * k + 3] << 24);
    } else {
      for (int k = 0; k < 12 && u0 + k / 3 < W; ++k) d[k] = o[k];
    }
  }
}

}  // namespace dd

using namespace dd;

extern "C" int dd_undistort(const unsigned char* src, int n, int H, int W, const double* intrinsic, unsigned char* dst, void* stream) {
  if (!src || !dst || !intrinsic) return (int)hipErrorInvalidValue;
  if (n < 1 || H < 1 || W < 1 || (long long)H * W * 3 > 2147483647ll || (H + UD_BY - 1) / UD_BY > 65535) return (int)hipErrorInvalidValue;
  if (((uintptr_t)src & 3u) || ((uintptr_t)dst & 3u)) return (int)hipErrorInvalidValue;
  for (int k = 0; k < 9; ++k)
    if (!(intrinsic[k] == intrinsic[k])) return (int)hipErrorInvalidValue;
  if (intrinsic[0] == 0.0 || intrinsic[1] == 0.0) return (int)hipErrorInvalidValue;
  UDCal cal = {intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3], intrinsic[4], intrinsic[5], intrinsic[6], intrinsic[7], intrinsic[8]};
  const int groups = (W + 3) / 4;
  hipLaunchKernelGGL(undistort_kernel, dim3((groups + UD_BX - 1) / UD_BX, (H + UD_BY - 1) / UD_BY), dim3(UD_BX, UD_BY), 0,
                     static_cast<hipStream_t>(stream), src, n, H, W, cal, dst, (W & 3) == 0 ? 1 : 0);
  return (int)hipGetLastError();
}
