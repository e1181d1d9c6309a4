// Coloured point clouds (predict.py --save cloud / --scene): the network's (B,h,w) disparity becomes, at the H x W source image, the
// back-projected points that pass a range, a depth-edge and a motion filter, optionally moved by a rigid pose, compacted in order
// into 16-byte PLY records.  Done with torch operators that is an up-sample, disp_to_depth, a reciprocal, a back-projection, three
// masks, nonzero (a host synchronisation), gathers and an interleave per frame.
// Candidates are the pixels (Y, X) of the source frame with Y % stride == 0 and X % stride == 0.  Per candidate, fp32, no fused
// multiply-add (hipops/cloud.py export_cloud_host is the same arithmetic in numpy, bit for bit):
//   taps    dm_tap of Y and X (dd_bilinear.h) as dd_export.hip; d = export_tap (the flip fuse with disp_flipped), s = lo + span*d
//   depth   u = dm_blend(s taps), depth = 1/u: the number dd_export_depth writes
//   keep    depth > 0 && depth <= max_range (false for NaN);  with edge > 0: (smax - smin) <= edge*smin over the four taps (fmaxf /
//           fminf, whatever their weights);  with a motion mask: dm_blend(mask taps) < motion_thresh (false for NaN)
//   point   xc = ((float)X - cx)*ifx, yc = ((float)Y - cy)*ify (ifx, ify = 1/fx, 1/fy in double, rounded once on the host);
//           p = (xc*depth, yc*depth, depth);  with a pose p'_k = ((R[k,0]*x + R[k,1]*y) + R[k,2]*z) + t[k]
//   colour  vis_unit_byte(dm_blend(colour taps)) per channel of the network-resolution frame
//   record  three floats, then r, g, b, 255;  the kept candidates of frame 0 in row-major order, then frame 1, ...
// Three launches, no workgroup waits for another (no decoupled look-back: a workgroup that spins on a neighbour's flag can hang):
//   count   a workgroup = 256 candidates of one candidate row (it never straddles two frames): the keep rule, one count per workgroup
//   scan    ONE workgroup loops over the counts, 4096 per pass: exclusive scan in place, offsets[b] at the frame boundaries
//   write   the keep rule again (the source maps stay in cache), the rank inside the workgroup from the wave's 64-bit ballot (mbcnt)
//           plus the wave totals in LDS, one 16-byte store per kept point
// Placement is integer arithmetic, there is no atomic: every output byte is the same from run to run.  A record's index is below
// the number of candidates in front of it, so no store leaves the buffer the caller sized for all candidates.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

// in front of the shared headers: dm_blend and export_tap are compiled unfused in this file
#pragma clang fp contract(off)

#include "dd_bilinear.h"
#include "dd_export_tap.h"
#include "dd_math.h"
#include "dd_vis.h"

namespace dd {

constexpr int CL_NT = 256;              // candidates per workgroup, one per lane
constexpr int CL_ITEMS = 16;            // counts per lane and pass of the scan

struct CloudArgs {
  const float *disp, *flip, *l_mask, *color, *mask, *pose;
  int h, w, stride, Hc, Wc, nseg;       // Hc x Wc candidates per frame, nseg workgroups per candidate row
  float sy, sx, ifx, ify, cx, cy, max_range, edge, thresh;
  DepthParams dp;
};

struct CloudTaps {
  int y0, y1, x0, x1;
  float wy, wx;
};

// the workgroup's frame and candidate row, the lane's candidate column
__device__ __forceinline__ bool cloud_candidate(const CloudArgs& a, int& b, int& Y, int& X) {
  const int row = blockIdx.x / a.nseg, seg = blockIdx.x - row * a.nseg;
  const int Xc = seg * CL_NT + threadIdx.x;
  b = row / a.Hc;
  Y = (row - b * a.Hc) * a.stride;      // <= H - 1
  X = Xc * a.stride;                    // <= W - 1 where Xc < Wc
  return Xc < a.Wc;
}

template <bool FUSE>
__device__ __forceinline__ bool cloud_keep(const CloudArgs& a, int b, int Y, int X, CloudTaps& t, float& depth) {
  const int h = a.h, w = a.w;
  dm_tap(Y, a.sy, h, t.y0, t.y1, t.wy);
  dm_tap(X, a.sx, w, t.x0, t.x1, t.wx);
  const float* l_img = a.disp + (size_t)b * h * w;
  const float* r_img = FUSE ? a.flip + (size_t)b * h * w : nullptr;
  const float s00 = a.dp.lo + a.dp.span * export_tap<FUSE>(l_img, r_img, a.l_mask, w, t.y0, t.x0);
  const float s01 = a.dp.lo + a.dp.span * export_tap<FUSE>(l_img, r_img, a.l_mask, w, t.y0, t.x1);
  const float s10 = a.dp.lo + a.dp.span * export_tap<FUSE>(l_img, r_img, a.l_mask, w, t.y1, t.x0);
  const float s11 = a.dp.lo + a.dp.span * export_tap<FUSE>(l_img, r_img, a.l_mask, w, t.y1, t.x1);
  depth = 1.f / dm_blend(t.wy, t.wx, s00, s01, s10, s11);
  bool keep = depth > 0.f && depth <= a.max_range;
  if (a.edge > 0.f) {
    const float smax = fmaxf(fmaxf(s00, s01), fmaxf(s10, s11)), smin = fminf(fminf(s00, s01), fminf(s10, s11));
    keep = keep && (smax - smin) <= a.edge * smin;
  }
  if (a.mask) {
    const float* top = a.mask + ((size_t)b * h + t.y0) * w;
    const float* bot = a.mask + ((size_t)b * h + t.y1) * w;
    keep = keep && dm_blend(t.wy, t.wx, top[t.x0], top[t.x1], bot[t.x0], bot[t.x1]) < a.thresh;
  }
  return keep;
}

// grid (B * Hc * nseg)
template <bool FUSE>
__global__ __launch_bounds__(CL_NT) void cloud_count_kernel(const CloudArgs a, long long* __restrict__ blk) {
  int b, Y, X;
  CloudTaps t;
  float depth;
  const bool keep = cloud_candidate(a, b, Y, X) && cloud_keep<FUSE>(a, b, Y, X, t, depth);
  const int total = __syncthreads_count(keep);
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// one workgroup: blk[0 .. nblk) -> its exclusive scan in place; offsets[b] = the value at the first workgroup of frame b, offsets[B] = the total
__global__ __launch_bounds__(CL_NT) void cloud_scan_kernel(long long* __restrict__ blk, int nblk, int per_frame, int B, long long* __restrict__ offsets) {
  __shared__ long long part[CL_NT];
  const int t = threadIdx.x;
  long long carry = 0;
  for (long long b0 = 0; b0 < nblk; b0 += CL_NT * CL_ITEMS) {
    const long long i0 = b0 + (long long)t * CL_ITEMS;
    long long v[CL_ITEMS], mine = 0;
#pragma unroll
    for (int k = 0; k < CL_ITEMS; ++k) {
      v[k] = i0 + k < nblk ? blk[i0 + k] : 0;
      mine += v[k];
    }
    part[t] = mine;
    __syncthreads();
    for (int step = 1; step < CL_NT; step <<= 1) {
      const long long add = t >= step ? part[t - step] : 0;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    long long run = carry + part[t] - mine;
#pragma unroll
    for (int k = 0; k < CL_ITEMS; ++k) {
      if (i0 + k < nblk) {
        const int i = (int)(i0 + k);
        blk[i] = run;
        if (i % per_frame == 0) offsets[i / per_frame] = run;
        run += v[k];
      }
    }
    carry += part[CL_NT - 1];
    __syncthreads();
  }
  if (t == 0) offsets[B] = carry;
}

template <bool FUSE>
__global__ __launch_bounds__(CL_NT) void cloud_write_kernel(const CloudArgs a, const long long* __restrict__ blkoff, uint4* __restrict__ records) {
  __shared__ int wave_total[CL_NT / 64];
  int b, Y, X;
  CloudTaps t;
  float depth;
  const bool keep = cloud_candidate(a, b, Y, X) && cloud_keep<FUSE>(a, b, Y, X, t, depth);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_total[wave] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));      // kept lanes below this one
  for (int k = 0; k < wave; ++k) rank += wave_total[k];
  const float xc = ((float)X - a.cx) * a.ifx, yc = ((float)Y - a.cy) * a.ify;
  float px = xc * depth, py = yc * depth, pz = depth;
  if (a.pose) {
    const float* T = a.pose + (size_t)b * 12;
    const float x = px, y = py, z = pz;
    px = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    py = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    pz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
  }
  unsigned rgba = 255u << 24;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* top = a.color + (((size_t)b * 3 + c) * a.h + t.y0) * a.w;
    const float* bot = a.color + (((size_t)b * 3 + c) * a.h + t.y1) * a.w;
    rgba |= vis_unit_byte(dm_blend(t.wy, t.wx, top[t.x0], top[t.x1], bot[t.x0], bot[t.x1])) << (8 * c);
  }
  records[blkoff[blockIdx.x] + rank] = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), rgba);
}

// host: the candidate grid; false for sizes the entry points refuse
struct CloudGrid {
  int Hc, Wc, nseg, per_frame, nblk;
};

static bool cloud_grid(int B, int H, int W, int stride, CloudGrid& g) {
  if (B < 1 || H < 1 || W < 1 || stride < 1 || (long long)H * W > 0x7fffffffLL) return false;
  g.Hc = (int)(((long long)H + stride - 1) / stride), g.Wc = (int)(((long long)W + stride - 1) / stride);
  g.nseg = (g.Wc + CL_NT - 1) / CL_NT;
  const long long per_frame = (long long)g.Hc * g.nseg, nblk = per_frame * B;
  if (nblk * CL_NT > 0xffffffffLL) return false;          // a launch holds fewer than 2^32 lanes
  g.per_frame = (int)per_frame, g.nblk = (int)nblk;
  return true;
}

}  // namespace dd

using namespace dd;

extern "C" size_t dd_export_cloud_workspace_bytes(int B, int H, int W, int stride) {
  CloudGrid g;
  return cloud_grid(B, H, W, stride, g) ? (size_t)g.nblk * sizeof(long long) : 0;
}

extern "C" int dd_export_cloud(const float* disp, const float* disp_flipped, const float* l_mask, const float* color, const float* motion_mask,
                               const float* pose, int B, int h, int w, int H, int W, float fx, float fy, float cx, float cy, float min_depth,
                               float max_depth, float max_range, float edge, float motion_thresh, int stride, void* records, long long* offsets,
                               void* workspace, size_t workspace_bytes, void* stream) {
  CloudGrid g;
  if (!disp || !color || !records || !offsets || !workspace || (disp_flipped == nullptr) != (l_mask == nullptr)) return (int)hipErrorInvalidValue;
  if (h < 1 || w < 1 || (long long)h * w > 0x7fffffffLL || !cloud_grid(B, H, W, stride, g)) return (int)hipErrorInvalidValue;
  if (!(min_depth > 0.f) || !(max_depth > 0.f) || fx == 0.f || fy == 0.f || !(fx - fx == 0.f) || !(fy - fy == 0.f)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)disp & 3u) || ((uintptr_t)disp_flipped & 3u) || ((uintptr_t)l_mask & 3u) || ((uintptr_t)color & 3u) || ((uintptr_t)motion_mask & 3u) ||
      ((uintptr_t)pose & 3u) || ((uintptr_t)records & 15u) || ((uintptr_t)offsets & 7u) || ((uintptr_t)workspace & 7u))
    return (int)hipErrorInvalidValue;
  if (workspace_bytes < (size_t)g.nblk * sizeof(long long)) return (int)hipErrorInvalidValue;
  CloudArgs a;
  a.disp = disp, a.flip = disp_flipped, a.l_mask = l_mask, a.color = color, a.mask = motion_mask, a.pose = pose;
  a.h = h, a.w = w, a.stride = stride, a.Hc = g.Hc, a.Wc = g.Wc, a.nseg = g.nseg;
  // ATen's area_pixel_compute_scale: the ratio in fp32
  a.sy = (float)h / (float)H, a.sx = (float)w / (float)W;
  a.ifx = (float)(1.0 / (double)fx), a.ify = (float)(1.0 / (double)fy), a.cx = cx, a.cy = cy;
  a.max_range = max_range, a.edge = edge, a.thresh = motion_thresh;
  a.dp = depth_params(min_depth, max_depth);
  hipStream_t st = static_cast<hipStream_t>(stream);
  long long* blk = static_cast<long long*>(workspace);
  uint4* rec = static_cast<uint4*>(records);
  if (disp_flipped)
    hipLaunchKernelGGL(cloud_count_kernel<true>, dim3(g.nblk), dim3(CL_NT), 0, st, a, blk);
  else
    hipLaunchKernelGGL(cloud_count_kernel<false>, dim3(g.nblk), dim3(CL_NT), 0, st, a, blk);
  hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(CL_NT), 0, st, blk, g.nblk, g.per_frame, B, offsets);
  if (disp_flipped)
    hipLaunchKernelGGL(cloud_write_kernel<true>, dim3(g.nblk), dim3(CL_NT), 0, st, a, blk, rec);
  else
    hipLaunchKernelGGL(cloud_write_kernel<false>, dim3(g.nblk), dim3(CL_NT), 0, st, a, blk, rec);
  return (int)hipGetLastError();
}
