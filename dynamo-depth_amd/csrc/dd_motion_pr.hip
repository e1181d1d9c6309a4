// Motion-segmentation precision/recall counts in one pass (reference eval/motion_segmentation.py:52-95,118-140).
// The reference broadcasts `pred_mask > thrds` to a (B, T, H, W) boolean tensor per batch, sums it three ways per sample, keeps every
// full-resolution prediction on the host and walks the dataset a second time for the false-positive tally.  All of it is one integer
// histogram: a pixel's bin is the number of thresholds its up-sampled prediction exceeds, tp / p_sum per threshold are suffix sums of
// the bins of the moving / the labelled pixels, and the false positives of a class at ANY threshold are a suffix sum of that class's
// bins.  Here: every lane takes a run of 8 consecutive ground-truth pixels (one 8-byte load per label map), samples the
// low-resolution mask through the cache with ATen's bilinear taps, binary-searches the caller's threshold table in LDS, and the
// workgroup's 32-bit LDS histogram is flushed with 64-bit integer atomics: counts are exact and the same on every run.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"
#include "dd_bilinear.h"

namespace dd {

constexpr int MP_NT = 256;
constexpr int MP_RUN = 8;           // pixels per lane and iteration: one 8-byte load of each label map
constexpr int MP_MAX_T = 256;
constexpr int MP_MAX_SEM = 32;
constexpr int MP_MAX_GRID = 2048;
constexpr int MP_PEEL = 4;          // rounds of wave-level grouping before the lanes that are left add on their own

// hist[key] += 1 for every lane with key >= 0.  Trained masks are near 0 almost everywhere, so a wave's lanes mostly share one key:
// the lanes that agree with the first pending lane are counted with a ballot and that lane adds the popcount -- one LDS atomic
// instead of 64 colliding ones.  After MP_PEEL distinct keys (edges of a moving object, noise) each remaining lane adds its own 1.
// Must be called by all lanes of the wave.
__device__ __forceinline__ void mp_add(unsigned* hist, int key, int lane) {
  unsigned long long todo = __ballot(key >= 0);
#pragma unroll 1
  for (int r = 0; r < MP_PEEL && todo != 0ull; ++r) {
    const int leader = __ffsll((long long)todo) - 1;
    const int k0 = __builtin_amdgcn_readlane(key, leader);        // leader is wave-uniform: a register read, no LDS round trip
    const unsigned long long same = __ballot(key == k0) & todo;
    if (lane == leader) atomicAdd(&hist[k0], (unsigned)__popcll(same));
    todo &= ~same;
  }
  if ((todo >> lane) & 1ull) atomicAdd(&hist[key], 1u);
}

// LDS: thr[P - 1] (the table, padded with +inf to one less than a power of two P > T) then hist[(2 + num_sem) * (T + 1)]:
// row 0 = mot == 1, row 1 = mot != 1 && mot != 3 (the flush adds row 0 to it: global row 1 counts mot != 3), row 2+l = class l.
template <bool WIDE>
__global__ __launch_bounds__(MP_NT) void motion_pr_kernel(const float* __restrict__ pred, int h, int w, const uint8_t* __restrict__ mot,
                                                          const uint8_t* __restrict__ sem, int H, int W, long long total,
                                                          const float* __restrict__ thresholds, int T, int P, int num_sem,
                                                          unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned mp_lds[];
  float* thr = reinterpret_cast<float*>(mp_lds);
  unsigned* hist = mp_lds + (P - 1);
  const int nb = T + 1, nhist = (2 + num_sem) * nb;
  for (int i = threadIdx.x; i < P - 1; i += MP_NT) thr[i] = i < T ? thresholds[i] : __uint_as_float(0x7f800000u);
  for (int i = threadIdx.x; i < nhist; i += MP_NT) hist[i] = 0u;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;
  const bool same_size = h == H && w == W;
  const long long hw = (long long)H * W;
  const long long nruns = (total + MP_RUN - 1) / MP_RUN;
  const long long stride = (long long)gridDim.x * MP_NT;
  // wave-uniform trip count: every lane of a wave stays in the loop (the ballots of mp_add need them), idle ones carry no pixel
  for (long long base = (long long)blockIdx.x * MP_NT + (threadIdx.x & ~63); base < nruns; base += stride) {
    const long long p0 = (base + lane) * MP_RUN;
    const long long left = total - p0;
    const int cnt = left >= MP_RUN ? MP_RUN : (left > 0 ? (int)left : 0);
    uint8_t m[MP_RUN], s[MP_RUN];
#pragma unroll
    for (int j = 0; j < MP_RUN; ++j) m[j] = 3, s[j] = 255;
    if (WIDE && cnt == MP_RUN) {                             // mot + p0 is 8-byte aligned: the base is, and p0 is a multiple of 8
      const uint2 mv = *reinterpret_cast<const uint2*>(mot + p0);
#pragma unroll
      for (int j = 0; j < MP_RUN; ++j) m[j] = (uint8_t)(((j < 4 ? mv.x : mv.y) >> (8 * (j & 3))) & 255u);
      if (num_sem > 0) {
        const uint2 sv = *reinterpret_cast<const uint2*>(sem + p0);
#pragma unroll
        for (int j = 0; j < MP_RUN; ++j) s[j] = (uint8_t)(((j < 4 ? sv.x : sv.y) >> (8 * (j & 3))) & 255u);
      }
    } else {
#pragma unroll
      for (int j = 0; j < MP_RUN; ++j)
        if (j < cnt) {
          m[j] = mot[p0 + j];
          if (num_sem > 0) s[j] = sem[p0 + j];
        }
    }
    // (sample, row, column) of the run's first pixel; the run may cross a row or a sample when W is no multiple of 8
    int b = 0, y = 0, x = 0;
    if (cnt > 0) {
      if (total < (1ll << 31)) {
        const unsigned p = (unsigned)p0, uhw = (unsigned)hw;
        b = (int)(p / uhw);
        const unsigned r = p - (unsigned)b * uhw;
        y = (int)(r / (unsigned)W);
        x = (int)(r - (unsigned)y * (unsigned)W);
      } else {
        b = (int)(p0 / hw);
        const long long r = p0 - (long long)b * hw;
        y = (int)(r / W);
        x = (int)(r - (long long)y * W);
      }
    }
    int bin[MP_RUN];
    bool new_row = true;
    const float *row0 = pred, *row1 = pred;
    float wy = 0.f;
#pragma unroll
    for (int j = 0; j < MP_RUN; ++j) {
      bin[j] = 0;
      if (j < cnt) {
        if (new_row) {
          int y0, y1;
          dm_tap(y, sy, h, y0, y1, wy);
          const float* pb = pred + (size_t)b * h * w;
          row0 = pb + (size_t)y0 * w;
          row1 = pb + (size_t)y1 * w;
          new_row = false;
        }
        int x0, x1;
        float wx;
        dm_tap(x, sx, w, x0, x1, wx);
        // at equal sizes ATen copies (its kernels special-case it): the taps are the pixel itself, and a NaN neighbour at weight 0 stays out
        const float v = same_size ? row0[x0] : dm_blend(wy, wx, row0[x0], row0[x1], row1[x0], row1[x1]);
        // bin = #{k : v > thr[k]} on the ascending table: P - 1 slots, the padding is +inf (never exceeded); a NaN exceeds nothing
        int pos = 0;
        for (int step = P >> 1; step > 0; step >>= 1)
          if (v > thr[pos + step - 1]) pos += step;
        bin[j] = pos;
        if (++x == W) {
          x = 0;
          new_row = true;
          if (++y == H) y = 0, ++b;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < MP_RUN; ++j) {
      const int mj = m[j];                                   // idle slots carry 3: no row
      mp_add(hist, mj == 1 ? bin[j] : (mj == 3 ? -1 : nb + bin[j]), lane);
      if (num_sem > 0) mp_add(hist, (mj != 1 && mj != 3 && (int)s[j] < num_sem) ? (2 + (int)s[j]) * nb + bin[j] : -1, lane);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nhist; i += MP_NT) {
    unsigned long long c = hist[i];
    if (i >= nb && i < 2 * nb) c += hist[i - nb];
    if (c != 0ull) atomicAdd(&counts[i], c);
  }
}

}  // namespace dd

using namespace dd;

extern "C" int dd_motion_pr(const float* pred, int B, int h, int w, const uint8_t* mot, const uint8_t* sem, int H, int W,
                            const float* thresholds, int T, int num_sem, unsigned long long* counts, void* stream) {
  if (!pred || !mot || !thresholds || !counts || B < 1 || h < 1 || w < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  if (T < 1 || T > MP_MAX_T || num_sem < 0 || num_sem > MP_MAX_SEM || (num_sem > 0 && !sem)) return (int)hipErrorInvalidValue;
  if ((long long)B * h * w >= (1ll << 40) || (long long)B * H * W >= (1ll << 40)) return (int)hipErrorInvalidValue;
  int P = 2;
  while (P <= T) P <<= 1;                                    // the search takes log2(P) steps over P - 1 >= T slots
  const long long total = (long long)B * H * W;
  const long long nruns = (total + MP_RUN - 1) / MP_RUN;
  const long long want = (nruns + MP_NT - 1) / MP_NT;
  const int grid = (int)(want < MP_MAX_GRID ? want : MP_MAX_GRID);
  const size_t lds = ((size_t)(P - 1) + (size_t)(2 + num_sem) * (T + 1)) * sizeof(unsigned);
  const bool wide = (((uintptr_t)mot | (num_sem > 0 ? (uintptr_t)sem : 0)) & 7u) == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (wide)
    hipLaunchKernelGGL(motion_pr_kernel<true>, dim3(grid), dim3(MP_NT), lds, s, pred, h, w, mot, sem, H, W, total, thresholds, T, P, num_sem, counts);
  else
    hipLaunchKernelGGL(motion_pr_kernel<false>, dim3(grid), dim3(MP_NT), lds, s, pred, h, w, mot, sem, H, W, total, thresholds, T, P, num_sem, counts);
  return (int)hipGetLastError();
}
