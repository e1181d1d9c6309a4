// The part of the reference's odometry evaluation that comes after the network (eval/odometry.py:19-41,70-96): snippet
// trajectories from the predicted frame-pair transforms and from the ground-truth global poses, the scale-aligned absolute
// trajectory error (ATE) of every snippet and the ground-truth speed.  The reference copies one pose per frame to the host and
// walks the snippets in numpy; here one thread owns one snippet and nothing leaves the device.
//
// Everything is float64.  Waymo's global translations are ~4e4 m with ~1 m between frames: the relative pose of two
// neighbouring frames is a difference of nearly equal numbers, and fp32 would lose millimetres there.  The relative pose is
// formed as [R0^-1 R1 | R0^-1 (t1 - t0)], so the large translations cancel BEFORE anything multiplies them (the reference's
// inv(G0) . G1 cancels them after; the difference between the two is the reference's own rounding, profiles/eval_accumulators.txt).
// The global poses are taken as affine (last row 0 0 0 1, what odometry.txt holds); their 3x3 blocks are inverted by cofactors,
// not assumed orthonormal, as the reference inverts them in general.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

namespace dd {

constexpr int OD_NT = 64;
constexpr int OD_MAX_TRACK = 16;

// affine 3x4 [R | t], row-major
struct OdAffine {
  double m[3][4];
};

__device__ __forceinline__ OdAffine od_load_global(const double* __restrict__ g) {
  OdAffine a;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) a.m[r][c] = g[r * 4 + c];
  return a;
}

// inverse of the 3x3 block by cofactors
__device__ __forceinline__ void od_inv3(const OdAffine& a, double inv[3][3]) {
  const double c00 = a.m[1][1] * a.m[2][2] - a.m[1][2] * a.m[2][1];
  const double c01 = a.m[1][2] * a.m[2][0] - a.m[1][0] * a.m[2][2];
  const double c02 = a.m[1][0] * a.m[2][1] - a.m[1][1] * a.m[2][0];
  const double det = a.m[0][0] * c00 + a.m[0][1] * c01 + a.m[0][2] * c02;
  const double s = 1.0 / det;
  inv[0][0] = c00 * s;
  inv[1][0] = c01 * s;
  inv[2][0] = c02 * s;
  inv[0][1] = (a.m[0][2] * a.m[2][1] - a.m[0][1] * a.m[2][2]) * s;
  inv[1][1] = (a.m[0][0] * a.m[2][2] - a.m[0][2] * a.m[2][0]) * s;
  inv[2][1] = (a.m[0][1] * a.m[2][0] - a.m[0][0] * a.m[2][1]) * s;
  inv[0][2] = (a.m[0][1] * a.m[1][2] - a.m[0][2] * a.m[1][1]) * s;
  inv[1][2] = (a.m[0][2] * a.m[1][0] - a.m[0][0] * a.m[1][2]) * s;
  inv[2][2] = (a.m[0][0] * a.m[1][1] - a.m[0][1] * a.m[1][0]) * s;
}

// inv(inv(G0) . G1): the local pose the reference chains (eval/odometry.py:79-81)
__device__ OdAffine od_local_pose(const double* __restrict__ g0p, const double* __restrict__ g1p) {
  const OdAffine g0 = od_load_global(g0p), g1 = od_load_global(g1p);
  double i0[3][3];
  od_inv3(g0, i0);
  OdAffine rel;                                              // inv(G0) . G1
  const double d[3] = {g1.m[0][3] - g0.m[0][3], g1.m[1][3] - g0.m[1][3], g1.m[2][3] - g0.m[2][3]};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) rel.m[r][c] = i0[r][0] * g1.m[0][c] + i0[r][1] * g1.m[1][c] + i0[r][2] * g1.m[2][c];
    rel.m[r][3] = i0[r][0] * d[0] + i0[r][1] * d[1] + i0[r][2] * d[2];
  }
  double ir[3][3];
  od_inv3(rel, ir);
  OdAffine loc;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) loc.m[r][c] = ir[r][c];
    loc.m[r][3] = -(ir[r][0] * rel.m[0][3] + ir[r][1] * rel.m[1][3] + ir[r][2] * rel.m[2][3]);
  }
  return loc;
}

// cam <- cam . step, both affine
__device__ __forceinline__ void od_chain(OdAffine& cam, const OdAffine& step) {
  OdAffine out;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      out.m[r][c] = cam.m[r][0] * step.m[0][c] + cam.m[r][1] * step.m[1][c] + cam.m[r][2] * step.m[2][c] + (c == 3 ? cam.m[r][3] : 0.0);
  }
  cam = out;
}

__global__ __launch_bounds__(OD_NT) void odom_snippets_kernel(const float* __restrict__ pred, const double* __restrict__ gt_global, int N,
                                                              int track_length, int S, double* __restrict__ ate, double* __restrict__ speed) {
  const int i = blockIdx.x * OD_NT + threadIdx.x;            // snippet start
  if (i >= S) return;
  // S <= N - track_length + 3, so N - i >= track_length - 2 >= 0 steps; the last kept snippet is one step short
  const int steps = min(track_length - 1, N - i);            // pred[i .. i+steps) and gt_global[i .. i+steps], steps <= N - i
  const int P = steps + 1;
  double gp[OD_MAX_TRACK][3], pp[OD_MAX_TRACK][3];
  gp[0][0] = gp[0][1] = gp[0][2] = 0.0;
  pp[0][0] = pp[0][1] = pp[0][2] = 0.0;

  // predicted points: translations of I . T_i . T_{i+1} ..., the full 4x4 product as np.dot forms it, axes reordered (z, x, y)
  double cam[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) cam[r][c] = r == c ? 1.0 : 0.0;
  for (int k = 0; k < steps; ++k) {
    const float* t = pred + (size_t)(i + k) * 16;
    double m[4][4], out[4][4];
#pragma unroll
    for (int e = 0; e < 16; ++e) m[e >> 2][e & 3] = (double)t[e];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) out[r][c] = cam[r][0] * m[0][c] + cam[r][1] * m[1][c] + cam[r][2] * m[2][c] + cam[r][3] * m[3][c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) cam[r][c] = out[r][c];
    pp[k + 1][0] = cam[2][3];
    pp[k + 1][1] = cam[0][3];
    pp[k + 1][2] = cam[1][3];
  }

  // ground-truth points: the same running product over the local poses
  OdAffine g;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) g.m[r][c] = r == c ? 1.0 : 0.0;
  double dist = 0.0;
  for (int k = 0; k < steps; ++k) {
    const OdAffine loc = od_local_pose(gt_global + (size_t)(i + k) * 16, gt_global + (size_t)(i + k + 1) * 16);
    od_chain(g, loc);
    gp[k + 1][0] = g.m[0][3];
    gp[k + 1][1] = g.m[1][3];
    gp[k + 1][2] = g.m[2][3];
    const double dx = gp[k + 1][0] - gp[k][0], dy = gp[k + 1][1] - gp[k][1], dz = gp[k + 1][2] - gp[k][2];
    dist += sqrt(dx * dx + dy * dy + dz * dz);
  }
  speed[i] = dist / (double)steps;                           // steps >= 1: i < S <= N and N - i >= track_length - 2

  // compute_ate (eval/odometry.py:30-41): align the first points, least-squares scale (unguarded: 0/0 is NaN there too), rmse / P
  const double off[3] = {gp[0][0] - pp[0][0], gp[0][1] - pp[0][1], gp[0][2] - pp[0][2]};
  double sgp = 0.0, spp = 0.0;
  for (int k = 0; k < P; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pp[k][c] += off[c];
      sgp += gp[k][c] * pp[k][c];
      spp += pp[k][c] * pp[k][c];
    }
  }
  const double scale = sgp / spp;
  double err = 0.0;
  for (int k = 0; k < P; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double e = pp[k][c] * scale - gp[k][c];
      err += e * e;
    }
  }
  ate[i] = sqrt(err) / (double)P;
}

}  // namespace dd

using namespace dd;

extern "C" int dd_odom_snippet_count(int N, int track_length) {
  if (N < 1 || track_length < 2 || track_length > OD_MAX_TRACK) return -1;
  const int s = N - track_length + 3;
  return s < 0 ? 0 : (s > N ? N : s);
}

extern "C" int dd_odom_snippets(const float* pred, const double* gt_global, int N, int track_length, double* ate, double* speed, void* stream) {
  const int S = dd_odom_snippet_count(N, track_length);
  if (S < 0) return (int)hipErrorInvalidValue;
  if (S == 0) return (int)hipSuccess;
  if (!pred || !gt_global || !ate || !speed) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(odom_snippets_kernel, dim3((S + OD_NT - 1) / OD_NT), dim3(OD_NT), 0, static_cast<hipStream_t>(stream), pred, gt_global, N,
                     track_length, S, ate, speed);
  return (int)hipGetLastError();
}
