// KITTI LiDAR depth lists (reference prepare_data/kitti.py:104-115 + kitti_util.py generate_depth_map(..., vel_depth=True)): one
// Velodyne scan projected through a 3x4 matrix per camera, z-buffered into an H x W map with the reference's duplicate rule, and the
// pixels with a positive value written as row-major [r, c, d] float64 rows.  The definition (hipops/lidar.py
// depth_points_host) for one scan, one matrix P and W >= 2:
//   kept      point i with x_i >= 0 (false for NaN, true for -0.0)
//   project   float64, unfused, left to right: a_k = ((P[k,0] x + P[k,1] y) + P[k,2] z) + P[k,3]; u = a_0 / a_2, v = a_1 / a_2;
//             c = rint(u) - 1, r = rint(v) - 1 (half to even)
//   valid     c >= 0 && r >= 0 && c < W && r < H, compared in float64; the depth d is x_i (float32, -0.0 read as 0), not a_2
//   map       map[r, c] = d of the valid point with the highest i at that pixel, 0 where there is none
//   buckets   b = r (W - 1) + c - 1 (the reference's sub2ind: pixels (r, W-1) and (r+1, 0) share a bucket); in every bucket with two
//             or more valid points the pixel of the LOWEST-index point gets the minimum d of the bucket, every other pixel keeps its map value
//   rows      the pixels with map > 0 in row-major order as [r, c, d]
// Four launches per chunk of DL_CHUNK scans, after one memset of the chunk's atomic words to 0xff:
//   scatter   one thread per (point, camera): integer atomicMax of i per pixel, and per bucket atomicMin of i, atomicMax of i and
//             atomicMin of the depth's bits (non-negative floats order as unsigned integers).  first != last <=> two or more points.
//   resolve   one thread per pixel: the value of the definition (on the two edge columns, where two pixels share a bucket, the
//             first point is projected again to see which of them it hit), and the number of positive pixels per 256-pixel block
//   scan      one workgroup per job: exclusive scan of the block counts, the job's count
//   rows      one thread per pixel: rank inside the block by ballot, the row at its place
// Integer min / max atomics only: the words, and with them every output byte, do not depend on the order the points arrive in.
// The projection is compiled without contraction and rounds with rint, so it is the host definition bit for bit.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

#pragma clang fp contract(off)

namespace dd {

constexpr int DL_NT = 256;
constexpr int DL_CHUNK = 16;        // scans per set of launches: their offsets travel as kernel arguments
constexpr int DL_MAX_C = 65535;     // cameras are grid.z

struct DLScans {
  int off[DL_CHUNK + 1];            // rows of `points` where the chunk's scans begin; off[k + 1] - off[k] points each
};

// words per job: last[HW] | first[NB] | blast[NB] | bmin[NB], all initialised to 0xffffffff
struct DLShape {
  int H, W, HW, NB, NBLK, C;
};

__device__ __forceinline__ unsigned* dl_job_words(void* ws, const DLShape& g, int job) {
  return static_cast<unsigned*>(ws) + (size_t)job * ((size_t)g.HW + 3 * (size_t)g.NB);
}

// steps 1-3 of the definition; false for a point that is not kept or not valid
__device__ __forceinline__ bool dl_project(const float4 pt, const double* __restrict__ P, int H, int W, int& r, int& c, float& d) {
  if (!(pt.x >= 0.f)) return false;
  const double x = (double)pt.x, y = (double)pt.y, z = (double)pt.z;
  const double a0 = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
  const double a1 = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
  const double a2 = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
  const double cc = rint(a0 / a2) - 1.0, rr = rint(a1 / a2) - 1.0;
  if (!(cc >= 0.0 && rr >= 0.0 && cc < (double)W && rr < (double)H)) return false;
  c = (int)cc, r = (int)rr;
  d = pt.x == 0.f ? 0.f : pt.x;
  return true;
}

__global__ __launch_bounds__(DL_NT) void lidar_scatter_kernel(const float4* __restrict__ points, DLScans sc, const double* __restrict__ P, DLShape g,
                                                              void* ws) {
  const int s = blockIdx.y, base = sc.off[s], n = sc.off[s + 1] - base;
  const long long t = (long long)blockIdx.x * DL_NT + threadIdx.x;
  if (t >= (long long)n * g.C) return;
  const int i = (int)(t / g.C), cam = (int)(t - (long long)i * g.C);
  int r, c;
  float d;
  if (!dl_project(points[(size_t)base + i], P + (size_t)cam * 12, g.H, g.W, r, c, d)) return;
  unsigned* w = dl_job_words(ws, g, s * g.C + cam);
  const int q = r * (g.W - 1) + c;                                // bucket + 1: 0 .. H (W - 1) = NB - 1
  unsigned* first = w + (size_t)g.HW;
  atomicMax(reinterpret_cast<int*>(w) + r * g.W + c, i);
  atomicMin(first + q, (unsigned)i);
  atomicMax(reinterpret_cast<int*>(first + (size_t)g.NB) + q, i);
  atomicMin(first + 2 * (size_t)g.NB + q, __float_as_uint(d));
}

__global__ __launch_bounds__(DL_NT) void lidar_resolve_kernel(const float4* __restrict__ points, DLScans sc, const double* __restrict__ P, DLShape g,
                                                              const void* ws, float* __restrict__ val, float* __restrict__ maps, int first_scan,
                                                              int* __restrict__ blkcnt) {
  const int s = blockIdx.y, cam = blockIdx.z, job = s * g.C + cam, base = sc.off[s];
  const long long pl = (long long)blockIdx.x * DL_NT + threadIdx.x;      // the last block may reach past 2^31
  float v = 0.f;
  if (pl < g.HW) {
    const int p = (int)pl;
    const unsigned* w = dl_job_words(const_cast<void*>(ws), g, job);
    const unsigned* first = w + (size_t)g.HW;
    const int r = p / g.W, c = p - r * g.W;
    const int li = (int)w[p];
    if (li >= 0) {
      const float x = points[(size_t)base + li].x;
      v = x == 0.f ? 0.f : x;
    }
    const int q = r * (g.W - 1) + c;
    const unsigned f = first[q];
    if (f != 0xffffffffu && (int)f != (int)first[(size_t)g.NB + q]) {
      bool mine = true;
      if ((c == 0 && r > 0) || (c == g.W - 1 && r < g.H - 1)) {   // (r, W-1) and (r+1, 0) share the bucket: where did its first point land?
        int rf = -1, cf = -1;
        float df;
        dl_project(points[(size_t)base + f], P + (size_t)cam * 12, g.H, g.W, rf, cf, df);
        mine = rf == r && cf == c;
      }
      if (mine) v = __uint_as_float(first[2 * (size_t)g.NB + q]);
    }
    val[(size_t)job * g.HW + p] = v;
    if (maps) maps[((size_t)(first_scan + s) * g.C + cam) * g.HW + p] = v;
  }
  const int total = __syncthreads_count(v > 0.f);
  if (threadIdx.x == 0) blkcnt[(size_t)job * g.NBLK + blockIdx.x] = total;
}

// blkcnt[job] -> its exclusive scan in place; counts[job] = the total
__global__ __launch_bounds__(DL_NT) void lidar_scan_kernel(int* __restrict__ blkcnt, int NBLK, int* __restrict__ counts) {
  __shared__ int part[DL_NT];
  int* cnt = blkcnt + (size_t)blockIdx.x * NBLK;
  const int t = threadIdx.x;
  int carry = 0;
  for (int b0 = 0; b0 < NBLK; b0 += DL_NT) {
    const int mine = b0 + t < NBLK ? cnt[b0 + t] : 0;
    part[t] = mine;
    __syncthreads();
    for (int step = 1; step < DL_NT; step <<= 1) {
      const int add = t >= step ? part[t - step] : 0;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    if (b0 + t < NBLK) cnt[b0 + t] = carry + part[t] - mine;
    carry += part[DL_NT - 1];
    __syncthreads();
  }
  if (t == 0) counts[blockIdx.x] = carry;
}

__global__ __launch_bounds__(DL_NT) void lidar_rows_kernel(DLScans sc, DLShape g, const float* __restrict__ val, const int* __restrict__ blkoff,
                                                           double* __restrict__ rows) {
  __shared__ int wave_total[DL_NT / 64];
  const int s = blockIdx.y, cam = blockIdx.z, job = s * g.C + cam;
  const int base = sc.off[s], n = sc.off[s + 1] - base;
  const long long pl = (long long)blockIdx.x * DL_NT + threadIdx.x;
  const int p = (int)pl;                                          // used below only where pl < HW
  const float v = pl < g.HW ? val[(size_t)job * g.HW + p] : 0.f;
  const bool keep = v > 0.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_total[wave] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  for (int k = 0; k < wave; ++k) rank += wave_total[k];
  const size_t row = (size_t)g.C * base + (size_t)cam * n + blkoff[(size_t)job * g.NBLK + blockIdx.x] + rank;   // < C * n_total: a job has at most n rows
  const int r = p / g.W;
  double* out = rows + 3 * row;
  out[0] = (double)r, out[1] = (double)(p - r * g.W), out[2] = (double)v;
}

static bool dl_shape(int S, int C, int H, int W, DLShape& g, int& jobs) {
  if (S < 1 || C < 1 || C > DL_MAX_C || H < 1 || W < 2 || (long long)H * W > 2147483647ll) return false;
  g.H = H, g.W = W, g.C = C;
  g.HW = H * W;
  g.NB = H * (W - 1) + 1;
  g.NBLK = (int)(((long long)g.HW + DL_NT - 1) / DL_NT);
  jobs = (S < DL_CHUNK ? S : DL_CHUNK) * C;
  return true;
}

}  // namespace dd

using namespace dd;

extern "C" size_t dd_lidar_depth_points_workspace_bytes(int S, int C, int H, int W) {
  DLShape g;
  int jobs;
  if (!dl_shape(S, C, H, W, g, jobs)) return 0;
  return (size_t)jobs * (2 * (size_t)g.HW + 3 * (size_t)g.NB + (size_t)g.NBLK) * 4;
}

extern "C" int dd_lidar_depth_points(const float* points, long long n_total, const int32_t* offsets, int S, const double* P, int C, int H, int W,
                                     int32_t* counts, double* rows, float* maps, void* workspace, size_t workspace_bytes, void* stream) {
  DLShape g;
  int jobs;
  if (!points || !offsets || !P || !counts || !rows || !workspace) return (int)hipErrorInvalidValue;
  if (!dl_shape(S, C, H, W, g, jobs) || n_total < 0 || n_total > 2147483647ll) return (int)hipErrorInvalidValue;
  if (offsets[0] != 0 || (long long)offsets[S] != n_total) return (int)hipErrorInvalidValue;
  for (int s = 0; s < S; ++s)
    if (offsets[s + 1] < offsets[s]) return (int)hipErrorInvalidValue;
  if (workspace_bytes < dd_lidar_depth_points_workspace_bytes(S, C, H, W)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)points & 15u) || ((uintptr_t)P & 7u) || ((uintptr_t)rows & 7u) || ((uintptr_t)counts & 3u) || ((uintptr_t)maps & 3u) ||
      ((uintptr_t)workspace & 3u))
    return (int)hipErrorInvalidValue;

  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t atomic_words = (size_t)g.HW + 3 * (size_t)g.NB;
  float* val = reinterpret_cast<float*>(static_cast<unsigned*>(workspace) + (size_t)jobs * atomic_words);
  int* blk = reinterpret_cast<int*>(val + (size_t)jobs * g.HW);
  for (int s0 = 0; s0 < S; s0 += DL_CHUNK) {
    const int ns = S - s0 < DL_CHUNK ? S - s0 : DL_CHUNK;
    DLScans sc;
    int n_max = 0;
    for (int k = 0; k <= DL_CHUNK; ++k) sc.off[k] = offsets[s0 + (k < ns ? k : ns)];
    for (int k = 0; k < ns; ++k) n_max = sc.off[k + 1] - sc.off[k] > n_max ? sc.off[k + 1] - sc.off[k] : n_max;
    hipError_t e = hipMemsetAsync(workspace, 0xff, (size_t)ns * C * atomic_words * 4, st);
    if (e != hipSuccess) return (int)e;
    if (n_max > 0) {
      const long long blocks = ((long long)n_max * C + DL_NT - 1) / DL_NT;
      if (blocks > 2147483647ll) return (int)hipErrorInvalidValue;
      hipLaunchKernelGGL(lidar_scatter_kernel, dim3((unsigned)blocks, ns), dim3(DL_NT), 0, st, reinterpret_cast<const float4*>(points), sc, P, g,
                         workspace);
    }
    hipLaunchKernelGGL(lidar_resolve_kernel, dim3(g.NBLK, ns, C), dim3(DL_NT), 0, st, reinterpret_cast<const float4*>(points), sc, P, g, workspace,
                       val, maps, s0, blk);
    hipLaunchKernelGGL(lidar_scan_kernel, dim3(ns * C), dim3(DL_NT), 0, st, blk, g.NBLK, counts + (size_t)s0 * C);
    hipLaunchKernelGGL(lidar_rows_kernel, dim3(g.NBLK, ns, C), dim3(DL_NT), 0, st, sc, g, val, blk, rows);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// nuScenes preparation (reference prepare_data/nuScenes.py:157-244; DESIGN 4.22, hipops/lidar.py pose_points_host / box_fit_host).
//
// dd_lidar_pose_points: every point of a batch of scans carried sensor -> ego (lidar time) -> global -> ego (camera time) -> camera,
// one rigid step after the other as the reference applies them (never folded into one matrix), in float64, unfused, every dot
// product left to right: rotate p' = R p with p'_k = (R[k,0] x + R[k,1] y) + R[k,2] z, translate p' = p + t or p - t.  The global
// point is kept after the second step; pixel u = a_0 / a_2, v = a_1 / a_2 with a = K p_cam summed the same way, depth = z_cam; kept
// where depth > 1, 1 < u < W - 1 and 1 < v < H - 1 (false for NaN).  Kept rows [u, v, depth, gx, gy, gz] are compacted in scan order
// with the scheme of the KITTI rows above: block counts, one scan per job, rank by ballot -- the projection is computed twice with
// the same code instead of being stored between the two launches.  Three launches per DL_CHUNK scans, no atomics.
//
// dd_box_fit: for every movable panoptic label of a key frame (its points contiguous: seg[l] .. seg[l + 1] - 1) and every
// annotation box of the same category, the number of its points strictly inside the box (get_intersect_fraction's three dot-product
// tests), and per label the first box with the strictly greatest count.  One launch, one workgroup per label, its four waves take
// the boxes in turn; counts are sums of ballot popcounts in integers, the four waves' bests combine in box order: no atomics,
// the same words every run.
namespace dd {

constexpr int DP_STRIDE = 64;       // doubles per scan: R1[9] t1[3] R2[9] t2[3] t3[3] R3[9] t4[3] R4[9] K[9] W H, 5 unused
constexpr int BF_STRIDE = 16;       // doubles per box: p1[3] i[3] j[3] k[3] i.i j.j k.k, 1 unused

__device__ __forceinline__ void dp_rotate(const double* __restrict__ R, double& x, double& y, double& z) {
  const double a = (R[0] * x + R[1] * y) + R[2] * z;
  const double b = (R[3] * x + R[4] * y) + R[5] * z;
  const double c = (R[6] * x + R[7] * y) + R[8] * z;
  x = a, y = b, z = c;
}

// the six values of one point; true where the reference's mask keeps it
__device__ __forceinline__ bool dp_point(const float4 pt, const double* __restrict__ q, double* __restrict__ o) {
  double x = (double)pt.x, y = (double)pt.y, z = (double)pt.z;
  dp_rotate(q, x, y, z);
  x = x + q[9], y = y + q[10], z = z + q[11];
  dp_rotate(q + 12, x, y, z);
  x = x + q[21], y = y + q[22], z = z + q[23];
  o[3] = x, o[4] = y, o[5] = z;
  x = x - q[24], y = y - q[25], z = z - q[26];
  dp_rotate(q + 27, x, y, z);
  x = x - q[36], y = y - q[37], z = z - q[38];
  dp_rotate(q + 39, x, y, z);
  const double depth = z;
  dp_rotate(q + 48, x, y, z);
  const double u = x / z, v = y / z;
  o[0] = u, o[1] = v, o[2] = depth;
  return depth > 1.0 && u > 1.0 && u < q[57] - 1.0 && v > 1.0 && v < q[58] - 1.0;
}

__global__ __launch_bounds__(DL_NT) void pose_count_kernel(const float4* __restrict__ points, DLScans sc, const double* __restrict__ params, int NBLK,
                                                           int* __restrict__ blkcnt) {
  const int s = blockIdx.y, base = sc.off[s], n = sc.off[s + 1] - base;
  const int i = blockIdx.x * DL_NT + threadIdx.x;
  double o[6];
  const bool keep = i < n && dp_point(points[(size_t)base + i], params + (size_t)s * DP_STRIDE, o);
  const int total = __syncthreads_count(keep);
  if (threadIdx.x == 0) blkcnt[(size_t)s * NBLK + blockIdx.x] = total;
}

__global__ __launch_bounds__(DL_NT) void pose_rows_kernel(const float4* __restrict__ points, DLScans sc, const double* __restrict__ params, int NBLK,
                                                          const int* __restrict__ blkoff, double* __restrict__ rows) {
  __shared__ int wave_total[DL_NT / 64];
  const int s = blockIdx.y, base = sc.off[s], n = sc.off[s + 1] - base;
  const int i = blockIdx.x * DL_NT + threadIdx.x;
  double o[6];
  const bool keep = i < n && dp_point(points[(size_t)base + i], params + (size_t)s * DP_STRIDE, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_total[wave] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int rank = __popcll(m & ((1ull << lane) - 1ull));
  for (int k = 0; k < wave; ++k) rank += wave_total[k];
  double* out = rows + 6 * ((size_t)base + blkoff[(size_t)s * NBLK + blockIdx.x] + rank);      // < base + n: a scan has at most n rows
#pragma unroll
  for (int k = 0; k < 6; ++k) out[k] = o[k];
}

__global__ __launch_bounds__(DL_NT) void box_fit_kernel(const double* __restrict__ pts, int n_points, const int* __restrict__ seg,
                                                        const int* __restrict__ label_cat, const double* __restrict__ boxes,
                                                        const int* __restrict__ box_cat, int B, int* __restrict__ counts, int* __restrict__ best) {
  __shared__ int s_cnt[DL_NT / 64], s_box[DL_NT / 64];
  const int l = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lo = min(max(seg[l], 0), n_points), n = min(max(seg[l + 1], lo), n_points) - lo;
  const int cat = label_cat[l];
  int bc = 0, bb = -1;
  for (int b = wave; b < B; b += DL_NT / 64) {
    int c = -1;                                                   // a box of another category is not counted
    if (box_cat[b] == cat) {
      const double* q = boxes + (size_t)b * BF_STRIDE;
      c = 0;
      for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        bool in = false;
        if (i < n) {
          const double* p = pts + 3 * ((size_t)lo + i);
          const double x = p[0] - q[0], y = p[1] - q[1], z = p[2] - q[2];
          const double vi = (x * q[3] + y * q[4]) + z * q[5];
          const double vj = (x * q[6] + y * q[7]) + z * q[8];
          const double vk = (x * q[9] + y * q[10]) + z * q[11];
          in = 0.0 < vi && vi < q[12] && 0.0 < vj && vj < q[13] && 0.0 < vk && vk < q[14];
        }
        c += __popcll(__ballot(in));
      }
      if (c > bc) bc = c, bb = b;                                 // ascending b: the first of equal counts stays
    }
    if (lane == 0) counts[(size_t)l * B + b] = c;
  }
  if (lane == 0) s_cnt[wave] = bc, s_box[wave] = bb;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < DL_NT / 64; ++w)
      if (s_box[w] >= 0 && (s_cnt[w] > bc || (s_cnt[w] == bc && s_box[w] < bb))) bc = s_cnt[w], bb = s_box[w];
    best[2 * l] = bb, best[2 * l + 1] = bc;
  }
}

}  // namespace dd

extern "C" size_t dd_lidar_pose_points_workspace_bytes(int S, long long n_max) {
  if (S < 1 || n_max < 0 || n_max > 2147483647ll - DL_NT) return 0;
  const long long nblk = n_max > 0 ? (n_max + DL_NT - 1) / DL_NT : 1;
  return (size_t)(S < DL_CHUNK ? S : DL_CHUNK) * (size_t)nblk * 4;
}

extern "C" int dd_lidar_pose_points(const float* points, long long n_total, const int32_t* offsets, int S, const double* params, int32_t* counts,
                                    double* rows, void* workspace, size_t workspace_bytes, void* stream) {
  if (!points || !offsets || !params || !counts || !rows || !workspace) return (int)hipErrorInvalidValue;
  if (S < 1 || n_total < 0 || n_total > 2147483647ll - DL_NT) return (int)hipErrorInvalidValue;
  if (offsets[0] != 0 || (long long)offsets[S] != n_total) return (int)hipErrorInvalidValue;
  long long longest = 0;
  for (int s = 0; s < S; ++s) {
    if (offsets[s + 1] < offsets[s]) return (int)hipErrorInvalidValue;
    if (offsets[s + 1] - offsets[s] > longest) longest = offsets[s + 1] - offsets[s];
  }
  if (workspace_bytes < dd_lidar_pose_points_workspace_bytes(S, longest)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)points & 15u) || ((uintptr_t)params & 7u) || ((uintptr_t)rows & 7u) || ((uintptr_t)counts & 3u) || ((uintptr_t)workspace & 3u))
    return (int)hipErrorInvalidValue;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* blk = static_cast<int*>(workspace);
  for (int s0 = 0; s0 < S; s0 += DL_CHUNK) {
    const int ns = S - s0 < DL_CHUNK ? S - s0 : DL_CHUNK;
    DLScans sc;
    int n_max = 0;
    for (int k = 0; k <= DL_CHUNK; ++k) sc.off[k] = offsets[s0 + (k < ns ? k : ns)];
    for (int k = 0; k < ns; ++k) n_max = sc.off[k + 1] - sc.off[k] > n_max ? sc.off[k + 1] - sc.off[k] : n_max;
    const int NBLK = n_max > 0 ? (n_max + DL_NT - 1) / DL_NT : 1;
    const double* q = params + (size_t)s0 * DP_STRIDE;
    hipLaunchKernelGGL(pose_count_kernel, dim3(NBLK, ns), dim3(DL_NT), 0, st, reinterpret_cast<const float4*>(points), sc, q, NBLK, blk);
    hipLaunchKernelGGL(lidar_scan_kernel, dim3(ns), dim3(DL_NT), 0, st, blk, NBLK, counts + s0);
    hipLaunchKernelGGL(pose_rows_kernel, dim3(NBLK, ns), dim3(DL_NT), 0, st, reinterpret_cast<const float4*>(points), sc, q, NBLK, blk, rows);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

extern "C" int dd_box_fit(const double* points, int n_points, const int32_t* seg, const int32_t* label_cat, int L, const double* boxes,
                          const int32_t* box_cat, int B, int32_t* counts, int32_t* best, void* stream) {
  if (L < 0 || B < 0 || n_points < 0 || L > 2147483647 / (B > 0 ? B : 1)) return (int)hipErrorInvalidValue;
  if (L == 0) return 0;
  if (!seg || !label_cat || !best || (n_points > 0 && !points) || (B > 0 && (!boxes || !box_cat || !counts))) return (int)hipErrorInvalidValue;
  if (((uintptr_t)points & 7u) || ((uintptr_t)boxes & 7u)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(box_fit_kernel, dim3(L), dim3(DL_NT), 0, static_cast<hipStream_t>(stream), points, n_points, seg, label_cat, boxes, box_cat, B,
                     counts, best);
  return (int)hipGetLastError();
}
