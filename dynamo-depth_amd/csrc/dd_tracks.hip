// Objects linked across frames (predict.py --save tracks): the vote of the network's own correspondences between the
// label map of frame i and the label map of its predecessor.  hipops/tracks.py link_host is the definition in numpy.
//   per pixel   (b, y, x) with a = labels_src[b, y, x] in 1..M; fp32, unfused: d = export_tap (the flip fuse with disp_flipped),
//               s = lo + span*d, z = 1/s, p = (xc*z, yc*z, z) with xc = ((float)x - cx)*ifx;  c_k = flow[b, k, y, x]*ts[b];  m = p + c: the
//               pixel's point in the predecessor's camera;  un = m0/m2, vn = m1/m2;  u = fx*un + cx, v = fy*vn + cy;
//               uf = floorf(u + 0.5f), vf likewise;  inside = m2 > 0 && 0 <= uf <= w-1 && 0 <= vf <= h-1 (false for NaN)
//   column      M+1 when not inside; else t = labels_dst[b, (int)vf, (int)uf], the column is t where t is in 1..M and 0 otherwise
//   votes       (B, M, M+2): votes[b, a-1, column] = the number of such pixels
//   links       (B, M, 6): dst, votes, dst2, votes2, background, outside -- the largest and the second largest column of 1..M (the
//               smaller column wins a tie; 0, 0 where no count is positive), column 0 and column M+1
// Three launches: a memset of votes, vote, select.  Kernel boundaries are the only ordering between workgroups: nothing spins and
// nothing waits for a flag.  Every sum is an integer atomicAdd, so every output byte is the same from run to run.
//   vote     one lane per pixel; a wave takes TR_SEG consecutive 64-pixel segments.  Per segment the voting lanes are grouped by
//            their word of votes: a pass takes the word of the lowest lane that is left, counts its lanes with a ballot and drops
//            them -- a pass removes at least that lane, and after TR_PASSES passes whatever is left goes lane by lane.  The wave
//            carries one word's running count from segment to segment and adds it only when another word comes up: inside an
//            object that moves as one that is one atomicAdd per 256 pixels.
//   select   one wave per row (b, a): lanes stride over the columns 1..M, wave arg-max twice.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

// in front of the shared header: export_tap and the per-pixel arithmetic are compiled unfused in this file
#pragma clang fp contract(off)

#include "dd_export_tap.h"

namespace dd {

constexpr int TR_NT = 256;              // lanes per workgroup, both kernels
constexpr int TR_SEG = 4;               // vote: 64-pixel segments per wave, so a workgroup covers 1024 consecutive pixels
constexpr int TR_PASSES = 8;            // vote: words a wave groups per segment before the rest go lane by lane
constexpr int TR_LINK = DD_TRACKS_LINK; // 32-bit words per row of links

struct TrackArgs {
  const int *src, *dst;
  const float *disp, *flip, *l_mask, *flow, *ts;
  int B, h, w, hw, n;                   // n = B*h*w
  float fx, fy, cx, cy, ifx, ify, lo, span;
  int M;
};

// grid (ceil(n / 1024))
template <bool FUSE>
__global__ __launch_bounds__(TR_NT) void tracks_vote_kernel(const TrackArgs a, int* __restrict__ votes) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = ((long long)blockIdx.x * (TR_NT / 64) + wave) * (64 * TR_SEG);
  const int cols = a.M + 2;
  const float x_last = (float)(a.w - 1), y_last = (float)(a.h - 1);
  int carry_key = -1, carry_n = 0;      // wave-uniform: a word of votes and the count the wave holds for it
  for (int seg = 0; seg < TR_SEG; ++seg) {
    const long long gi = base + seg * 64 + lane;
    const bool valid = gi < a.n;
    const int i = (int)(valid ? gi : 0);
    const int label = valid ? a.src[i] : 0;
    const bool act = label >= 1 && label <= a.M;                // a source label outside 1..M votes nowhere
    int key = -1;
    if (act) {
      const int b = i / a.hw, rem = i - b * a.hw, y = rem / a.w, x = rem - y * a.w;
      const float* l_img = a.disp + (size_t)b * a.hw;
      const float* r_img = FUSE ? a.flip + (size_t)b * a.hw : nullptr;
      const float d = export_tap<FUSE>(l_img, r_img, a.l_mask, a.w, y, x);
      const float z = 1.f / (a.lo + a.span * d);
      const float xc = ((float)x - a.cx) * a.ifx, yc = ((float)y - a.cy) * a.ify;
      const float* f = a.flow + (size_t)b * 3 * a.hw + rem;
      const float ts = a.ts[b];
      const float m0 = xc * z + f[0] * ts, m1 = yc * z + f[a.hw] * ts, m2 = z + f[2 * (size_t)a.hw] * ts;
      const float un = m0 / m2, vn = m1 / m2;
      const float u = a.fx * un + a.cx, v = a.fy * vn + a.cy;
      const float uf = floorf(u + 0.5f), vf = floorf(v + 0.5f);
      int col = a.M + 1;
      if (m2 > 0.f && uf >= 0.f && uf <= x_last && vf >= 0.f && vf <= y_last) {          // every comparison is false for NaN
        const int ui = (int)uf, vi = (int)vf;                   // converted only behind the range test
        if (ui < a.w && vi < a.h) {     // the guard of the load: 0 <= ui < w and 0 <= vi < h as integers, whatever (float)(w-1) rounded to
          const int t = a.dst[(size_t)b * a.hw + (size_t)vi * a.w + ui];
          col = (t >= 1 && t <= a.M) ? t : 0;                   // a destination label outside 0..M counts as background
        }
      }
      // the guard of the atomic: 0 <= b < B, 0 <= label-1 < M, 0 <= col <= M+1, so 0 <= key < B*M*(M+2) <= 2^31-1
      key = (b * a.M + (label - 1)) * cols + col;
    }
    unsigned long long todo = __ballot(act);                    // wave-uniform, as everything the passes decide on
    for (int pass = 0; todo != 0 && pass < TR_PASSES; ++pass) {
      const int key0 = __shfl(key, __ffsll((long long)todo) - 1);
      const unsigned long long mine = __ballot(act && key == key0);
      const int count = __popcll(mine);
      if (carry_key == key0) {
        carry_n += count;
      } else {
        if (carry_key >= 0 && lane == 0) atomicAdd(votes + carry_key, carry_n);
        carry_key = key0, carry_n = count;
      }
      todo &= ~mine;
    }
    if ((todo >> lane) & 1) atomicAdd(votes + key, 1);          // more than TR_PASSES words in one segment: the rest lane by lane
  }
  if (carry_key >= 0 && lane == 0) atomicAdd(votes + carry_key, carry_n);
}

// the larger count wins, the smaller column among equal counts; all lanes get the result
__device__ __forceinline__ void wave_arg_max(int& count, int& col) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const int oc = __shfl_xor(count, s), ok = __shfl_xor(col, s);
    if (oc > count || (oc == count && ok < col)) count = oc, col = ok;
  }
}

// grid (ceil(B*M / 4)): one wave per row of votes
__global__ __launch_bounds__(TR_NT) void tracks_select_kernel(const int* __restrict__ votes, int rows, int M, int* __restrict__ links) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * (TR_NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;              // wave-uniform
  const int* v = votes + (size_t)row * (M + 2);
  int best = 0, best_col = 0x7fffffff;
  for (int c = 1 + lane; c <= M; c += 64) {
    const int n = v[c];
    if (n > best) best = n, best_col = c;                       // a lane's columns increase: the first of equal counts stays
  }
  wave_arg_max(best, best_col);
  if (best <= 0) best = 0, best_col = 0;
  int second = 0, second_col = 0x7fffffff;
  for (int c = 1 + lane; c <= M; c += 64) {
    const int n = v[c];
    if (c != best_col && n > second) second = n, second_col = c;
  }
  wave_arg_max(second, second_col);
  if (second <= 0) second = 0, second_col = 0;
  if (lane == 0) {
    int* out = links + (size_t)row * TR_LINK;
    out[0] = best_col, out[1] = best, out[2] = second_col, out[3] = second, out[4] = v[0], out[5] = v[M + 1];
  }
}

}  // namespace dd

using namespace dd;

extern "C" int dd_tracks_link(const int* labels_src, const int* labels_dst, const float* disp, const float* disp_flipped, const float* l_mask,
                              const float* complete_flow, const float* ts, int B, int h, int w, float fx, float fy, float cx, float cy, float lo,
                              float span, int max_objects, int* votes, int* links, void* stream) {
  if (!labels_src || !labels_dst || !disp || !complete_flow || !ts || !votes || !links || (disp_flipped == nullptr) != (l_mask == nullptr))
    return (int)hipErrorInvalidValue;
  if (B < 1 || h < 1 || w < 1 || max_objects < 1 || max_objects > DD_TRACKS_MAX_OBJECTS) return (int)hipErrorInvalidValue;
  const long long n = (long long)B * h * w, words = (long long)B * max_objects * (max_objects + 2);
  if (n > 0x7fffffffLL || words > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (fx == 0.f || fy == 0.f || !(fx - fx == 0.f) || !(fy - fy == 0.f)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)labels_src & 3u) || ((uintptr_t)labels_dst & 3u) || ((uintptr_t)disp & 3u) || ((uintptr_t)disp_flipped & 3u) || ((uintptr_t)l_mask & 3u) ||
      ((uintptr_t)complete_flow & 3u) || ((uintptr_t)ts & 3u) || ((uintptr_t)votes & 3u) || ((uintptr_t)links & 3u))
    return (int)hipErrorInvalidValue;
  TrackArgs a;
  a.src = labels_src, a.dst = labels_dst, a.disp = disp, a.flip = disp_flipped, a.l_mask = l_mask, a.flow = complete_flow, a.ts = ts;
  a.B = B, a.h = h, a.w = w, a.hw = h * w, a.n = (int)n;
  a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy, a.ifx = (float)(1.0 / (double)fx), a.ify = (float)(1.0 / (double)fy), a.lo = lo, a.span = span;
  a.M = max_objects;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t cleared = hipMemsetAsync(votes, 0, (size_t)words * sizeof(int), st);
  if (cleared != hipSuccess) return (int)cleared;
  const unsigned wide = (unsigned)((n + TR_NT * TR_SEG - 1) / (TR_NT * TR_SEG));
  if (disp_flipped)
    hipLaunchKernelGGL(tracks_vote_kernel<true>, dim3(wide), dim3(TR_NT), 0, st, a, votes);
  else
    hipLaunchKernelGGL(tracks_vote_kernel<false>, dim3(wide), dim3(TR_NT), 0, st, a, votes);
  const int rows = B * max_objects;
  hipLaunchKernelGGL(tracks_select_kernel, dim3((unsigned)((rows + TR_NT / 64 - 1) / (TR_NT / 64))), dim3(TR_NT), 0, st, votes, rows, max_objects, links);
  return (int)hipGetLastError();
}
