// Waymo range images to vehicle-frame points and to the camera's depth list (reference prepare_data/waymo.py:183-186 and 213-241:
// frame_utils.parse_range_image_and_camera_projection, convert_range_image_to_point_cloud, then the projection into one camera).
// The definition (hipops/lidar.py range_image_points_host) for image s of H x W pixels, pixel (r, c) with range rho:
//   direction  the host builds four float64 tables per image: cos and sin of the row's inclination (the calibration's list or the
//              uniform one, reversed so that row 0 looks up) and cos and sin of the column's azimuth
//              ((W - c - 0.5) / W * 2 - 1) * pi - atan2(E[1][0], E[0][0]); the device reads them, so both sides use the same values
//   point      p = ((cos az * cos incl) * rho, (sin az * cos incl) * rho, sin incl * rho); p = E_R p + E_t
//   pose       for the image that carries a per-pixel pose (roll, pitch, yaw, x, y, z; the TOP laser): p = Rz(yaw) Ry(pitch) Rx(roll) p
//              + (x, y, z), then p = F_R p + F_t with F the inverse of the frame pose, inverted on the host in float64
//   valid      rho > 0 (false for NaN)
//   camera     q = C_R p + C_t (C = inv(extrinsic * axis_swap), built on the host), a = K q; kept where a_z > 0, 0 <= a_x / a_z < width
//              and 0 <= a_y / a_z < height; the row is [a_x / a_z, a_y / a_z, a_z]
// All of it in float64, unfused, every dot product left to right.  Per image three ordered compactions, row-major over its pixels:
// points (n, 3) and the first camera projection triple cp (n, 3) of the valid pixels, rows (m, 3) of the kept ones.
// Five launches per RI_CHUNK images, no atomics: count the valid pixels per 256-pixel block; scan; compute every valid pixel's point
// once, write it and its projection triple at its rank, count the kept ones per block; scan; write the rows -- that last pass reads
// the stored float64 point and repeats only the camera step (two 3x3 products), so the trigonometry of the pose runs once per pixel.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

#pragma clang fp contract(off)

namespace dd {

constexpr int RI_NT = 256;
constexpr int RI_CHUNK = 16;        // images per set of launches: their descriptors travel as kernel arguments
constexpr int RI_STRIDE = 64;       // doubles per image: E_R[9] E_t[3] unused F_R[9] F_t[3] C_R[9] C_t[3] K[9] width height, 16 unused

struct RIImages {
  int pix[RI_CHUNK];                // first pixel of the image in range / cp, first row of its segment in the outputs
  int H[RI_CHUNK], W[RI_CHUNK];
  int pose[RI_CHUNK];               // first pixel in `pose`, -1: none
  int trig[RI_CHUNK];               // first double of cos incl [H], sin incl [H], cos az [W], sin az [W]
};

__device__ __forceinline__ void ri_rotate(const double* __restrict__ R, double& x, double& y, double& z) {
  const double a = (R[0] * x + R[1] * y) + R[2] * z;
  const double b = (R[3] * x + R[4] * y) + R[5] * z;
  const double c = (R[6] * x + R[7] * y) + R[8] * z;
  x = a, y = b, z = c;
}

// the camera step of a vehicle-frame point; true where the reference keeps it
__device__ __forceinline__ bool ri_camera(const double* __restrict__ q, double x, double y, double z, double* __restrict__ o) {
  ri_rotate(q + 25, x, y, z);
  x = x + q[34], y = y + q[35], z = z + q[36];
  ri_rotate(q + 37, x, y, z);
  const double u = x / z, v = y / z;
  o[0] = u, o[1] = v, o[2] = z;
  return z > 0.0 && u >= 0.0 && u < q[46] && v >= 0.0 && v < q[47];
}

// rank of a thread among the threads of its block with `flag` set; every thread of the block calls it
__device__ __forceinline__ int ri_rank(bool flag, int* wave_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  __syncthreads();                                                // the previous use of wave_total is over
  if (lane == 0) wave_total[wave] = __popcll(m);
  __syncthreads();
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  for (int k = 0; k < wave; ++k) rank += wave_total[k];
  return rank;
}

__global__ __launch_bounds__(RI_NT) void ri_count_kernel(const float* __restrict__ range, RIImages im, int NBLK, int* __restrict__ blk) {
  const int s = blockIdx.y, n = im.H[s] * im.W[s];
  const long long i = (long long)blockIdx.x * RI_NT + threadIdx.x;
  const bool valid = i < n && range[(size_t)im.pix[s] + i] > 0.f;
  const int total = __syncthreads_count(valid);
  if (threadIdx.x == 0) blk[(size_t)s * NBLK + blockIdx.x] = total;
}

// blk[image] -> its exclusive scan in place; counts[2 * image + column] = the total
__global__ __launch_bounds__(RI_NT) void ri_scan_kernel(int* __restrict__ blk, int NBLK, int* __restrict__ counts, int column) {
  __shared__ int part[RI_NT];
  int* cnt = blk + (size_t)blockIdx.x * NBLK;
  const int t = threadIdx.x;
  int carry = 0;
  for (int b0 = 0; b0 < NBLK; b0 += RI_NT) {
    const int mine = b0 + t < NBLK ? cnt[b0 + t] : 0;
    part[t] = mine;
    __syncthreads();
    for (int step = 1; step < RI_NT; step <<= 1) {
      const int add = t >= step ? part[t - step] : 0;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    if (b0 + t < NBLK) cnt[b0 + t] = carry + part[t] - mine;
    carry += part[RI_NT - 1];
    __syncthreads();
  }
  if (t == 0) counts[2 * blockIdx.x + column] = carry;
}

__global__ __launch_bounds__(RI_NT) void ri_points_kernel(const float* __restrict__ range, const int* __restrict__ cp, const float* __restrict__ pose,
                                                          const double* __restrict__ trig, RIImages im, const double* __restrict__ params, int NBLK,
                                                          const int* __restrict__ blk_a, int* __restrict__ blk_b, double* __restrict__ points,
                                                          int* __restrict__ cp_out) {
  __shared__ int wave_total[RI_NT / 64];
  const int s = blockIdx.y, H = im.H[s], W = im.W[s], n = H * W;
  const double* q = params + (size_t)s * RI_STRIDE;
  const long long il = (long long)blockIdx.x * RI_NT + threadIdx.x;
  const int i = (int)il;                                          // used below only where il < n
  const size_t px = (size_t)im.pix[s] + (size_t)i;
  const float rho_f = il < n ? range[px] : 0.f;
  const bool valid = rho_f > 0.f;
  const int rank = ri_rank(valid, wave_total);
  bool keep = false;
  if (valid) {
    const int r = i / W, c = i - r * W;
    const double* t = trig + im.trig[s];
    const double ci = t[r], si = t[H + r], ca = t[2 * H + c], sa = t[2 * H + W + c];
    const double rho = (double)rho_f;
    double x = (ca * ci) * rho, y = (sa * ci) * rho, z = si * rho;
    ri_rotate(q, x, y, z);
    x = x + q[9], y = y + q[10], z = z + q[11];
    if (im.pose[s] >= 0) {
      const float* e = pose + 6 * ((size_t)im.pose[s] + (size_t)i);
      const double cr = cos((double)e[0]), sr = sin((double)e[0]), cq = cos((double)e[1]), sq = sin((double)e[1]);
      const double cy = cos((double)e[2]), sy = sin((double)e[2]);
      double R[9];
      R[0] = cy * cq, R[1] = (cy * sq) * sr - sy * cr, R[2] = (cy * sq) * cr + sy * sr;
      R[3] = sy * cq, R[4] = (sy * sq) * sr + cy * cr, R[5] = (sy * sq) * cr - cy * sr;
      R[6] = -sq, R[7] = cq * sr, R[8] = cq * cr;
      ri_rotate(R, x, y, z);
      x = x + (double)e[3], y = y + (double)e[4], z = z + (double)e[5];
      ri_rotate(q + 13, x, y, z);
      x = x + q[22], y = y + q[23], z = z + q[24];
    }
    const size_t row = (size_t)im.pix[s] + blk_a[(size_t)s * NBLK + blockIdx.x] + rank;     // < pix + n: an image has at most n points
    points[3 * row] = x, points[3 * row + 1] = y, points[3 * row + 2] = z;
    cp_out[3 * row] = cp[3 * px], cp_out[3 * row + 1] = cp[3 * px + 1], cp_out[3 * row + 2] = cp[3 * px + 2];
    double o[3];
    keep = ri_camera(q, x, y, z, o);
  }
  const int total = __syncthreads_count(keep);
  if (threadIdx.x == 0) blk_b[(size_t)s * NBLK + blockIdx.x] = total;
}

__global__ __launch_bounds__(RI_NT) void ri_rows_kernel(const float* __restrict__ range, RIImages im, const double* __restrict__ params, int NBLK,
                                                        const int* __restrict__ blk_a, const int* __restrict__ blk_b,
                                                        const double* __restrict__ points, double* __restrict__ rows) {
  __shared__ int wave_total[RI_NT / 64];
  const int s = blockIdx.y, n = im.H[s] * im.W[s];
  const long long il = (long long)blockIdx.x * RI_NT + threadIdx.x;
  const bool valid = il < n && range[(size_t)im.pix[s] + (size_t)il] > 0.f;
  const int rank_a = ri_rank(valid, wave_total);
  double o[3] = {0.0, 0.0, 0.0};
  bool keep = false;
  if (valid) {
    const double* p = points + 3 * ((size_t)im.pix[s] + blk_a[(size_t)s * NBLK + blockIdx.x] + rank_a);
    keep = ri_camera(params + (size_t)s * RI_STRIDE, p[0], p[1], p[2], o);
  }
  const int rank_b = ri_rank(keep, wave_total);
  if (keep) {
    double* out = rows + 3 * ((size_t)im.pix[s] + blk_b[(size_t)s * NBLK + blockIdx.x] + rank_b);
    out[0] = o[0], out[1] = o[1], out[2] = o[2];
  }
}

}  // namespace dd

using namespace dd;

extern "C" size_t dd_range_image_points_workspace_bytes(int S, long long hw_max) {
  if (S < 1 || hw_max < 1 || hw_max > 2147483647ll - RI_NT) return 0;
  const long long nblk = (hw_max + RI_NT - 1) / RI_NT;
  return 2 * (size_t)(S < RI_CHUNK ? S : RI_CHUNK) * (size_t)nblk * 4;
}

extern "C" int dd_range_image_points(const float* range, const int32_t* cp, const float* pose, const double* trig, long long n_total, long long n_pose,
                                     long long n_trig, const int32_t* desc, int S, const double* params, int32_t* counts, double* points,
                                     int32_t* cp_out, double* rows, void* workspace, size_t workspace_bytes, void* stream) {
  if (!range || !cp || !trig || !desc || !params || !counts || !points || !cp_out || !rows || !workspace) return (int)hipErrorInvalidValue;
  if (S < 1 || n_total < 1 || n_total > 2147483647ll - RI_NT || n_pose < 0 || n_pose > 2147483647ll || n_trig < 1 || n_trig > 2147483647ll)
    return (int)hipErrorInvalidValue;
  if (n_pose > 0 && !pose) return (int)hipErrorInvalidValue;
  long long end = 0, hw_max = 0;
  for (int s = 0; s < S; ++s) {
    const int32_t* d = desc + 5 * (size_t)s;
    const long long H = d[1], W = d[2], hw = H * W;
    if (H < 1 || W < 1 || hw > 2147483647ll - RI_NT || d[0] < end || d[0] + hw > n_total) return (int)hipErrorInvalidValue;
    if (d[3] < -1 || (d[3] >= 0 && d[3] + hw > n_pose) || d[4] < 0 || d[4] + 2 * (H + W) > n_trig) return (int)hipErrorInvalidValue;
    end = d[0] + hw;
    if (hw > hw_max) hw_max = hw;
  }
  const size_t need = dd_range_image_points_workspace_bytes(S, hw_max);
  if (need == 0 || workspace_bytes < need) return (int)hipErrorInvalidValue;
  if (((uintptr_t)range & 3u) || ((uintptr_t)cp & 3u) || ((uintptr_t)pose & 3u) || ((uintptr_t)trig & 7u) || ((uintptr_t)params & 7u) ||
      ((uintptr_t)counts & 3u) || ((uintptr_t)points & 7u) || ((uintptr_t)cp_out & 3u) || ((uintptr_t)rows & 7u) || ((uintptr_t)workspace & 3u))
    return (int)hipErrorInvalidValue;
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int s0 = 0; s0 < S; s0 += RI_CHUNK) {
    const int ns = S - s0 < RI_CHUNK ? S - s0 : RI_CHUNK;
    RIImages im;
    long long chunk_max = 1;
    for (int k = 0; k < RI_CHUNK; ++k) {
      const int32_t* d = desc + 5 * (size_t)(s0 + (k < ns ? k : ns - 1));
      im.pix[k] = d[0], im.H[k] = d[1], im.W[k] = d[2], im.pose[k] = d[3], im.trig[k] = d[4];
      if ((long long)d[1] * d[2] > chunk_max) chunk_max = (long long)d[1] * d[2];
    }
    const int NBLK = (int)((chunk_max + RI_NT - 1) / RI_NT);
    int* blk_a = static_cast<int*>(workspace);
    int* blk_b = blk_a + (size_t)ns * NBLK;                       // ns * NBLK <= min(S, RI_CHUNK) * nblk(hw_max): inside the workspace
    const double* q = params + (size_t)s0 * RI_STRIDE;
    hipLaunchKernelGGL(ri_count_kernel, dim3(NBLK, ns), dim3(RI_NT), 0, st, range, im, NBLK, blk_a);
    hipLaunchKernelGGL(ri_scan_kernel, dim3(ns), dim3(RI_NT), 0, st, blk_a, NBLK, counts + 2 * (size_t)s0, 0);
    hipLaunchKernelGGL(ri_points_kernel, dim3(NBLK, ns), dim3(RI_NT), 0, st, range, cp, pose, trig, im, q, NBLK, blk_a, blk_b, points, cp_out);
    hipLaunchKernelGGL(ri_scan_kernel, dim3(ns), dim3(RI_NT), 0, st, blk_b, NBLK, counts + 2 * (size_t)s0, 1);
    hipLaunchKernelGGL(ri_rows_kernel, dim3(NBLK, ns), dim3(RI_NT), 0, st, range, im, q, NBLK, blk_a, blk_b, points, rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}
