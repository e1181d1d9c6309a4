// dd_linear_wgrad.hip -- weight AND bias gradient of LiteMono's point-wise Linears in one pass over their operands (gfx950).
//
//   g_weight[co][ci] = sum over the M = B*H*W rows of g[m][co] * x[m][ci],     g_bias[co] = sum over the rows of g[m][co]
//
// (reference networks/depth_encoder.py:200-203: pwconv1 / pwconv2 of every block, and XCA's qkv / proj), g (M, cout) and x (M, cin)
// dense row-major fp32.  The arithmetic is that of dd_conv_mfma.hip's weight gradient: every operand split exactly into three bf16
// pieces (dd_split.h), six partial products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- with the ROWS as the contraction.
//
//   * A workgroup (4 waves) owns a 64 (co) x 64 (ci) block of the result and a contiguous range of 16-row groups; it writes ONE partial
//     (64 x 64 weights + 64 bias sums), linear_wgrad_fold_kernel adds the partials in a fixed order.  No atomics, no zero-fill: every
//     element of g_weight and g_bias is written by the fold, every result is bit-reproducible.
//   * The four waves split the ROWS, not the block: wave w takes the 16-row groups w, w + 4, ... of the range and keeps the whole block,
//     a 2 x 2 set of 32 x 32 accumulators -- 24 MFMAs per 12 fragments (a 1x1 layer has no taps to get nine accumulators from).
//     A block that holds only 32 valid channels on either side (224 = 7 x 32) skips the MFMAs of its empty half.
//   * The operands want the contraction index contiguous per lane, the tensors have the channels contiguous.  With the rows split among
//     the waves nothing a wave loads is used by another wave, so the tile never goes through LDS: lane l IS channel l & 31 of the
//     fragment and loads its eight rows (l >> 5) * 8 .. + 7 of that channel itself, one dword each -- 32 lanes read 128 contiguous
//     bytes of a row, every cache line is used whole -- and splits them in registers straight into fragment form.  No transposing
//     stores, no bank conflicts, NO barrier and no LDS operation in the main loop.  Measured against it, same decomposition, same box
//     (profiles/linear_wgrad.txt): the tile transposed through a wave-private LDS buffer, two adjacent rows per 32-bit store as
//     conv_wgrad_kernel's `put` (float4 loads, 40-byte channel stride, stores paired on disjoint banks, ds_read_b64 fragments, the
//     split placed between the MFMAs with sched_group_barrier) -- 47.9 / 44.9 / 44.2 us against 43.7 / 41.2 / 41.1 us here at the
//     three stages, with 61 KB of LDS and a good deal more code.  The four accumulator sets meet in LDS, in wave order, at the end.
//   * The rows of step s + 1 are in flight (32 registers) under the MFMAs of step s.  Every global load of the loop is unconditional --
//     a row pointer in scalar registers plus a 32-bit lane offset, no address arithmetic per load (the header of dd_conv_mfma.hip says
//     why unconditional); the one group that crosses M is peeled off behind the loop and clamps its rows there.
//   * Bias: a lane always loads the same two channels of g and keeps fp32 running sums of the raw values; they meet in LDS in a fixed
//     order and only the workgroups of ci block 0 write them.
#include <hip/hip_runtime.h>
#include <cstdlib>

#include "../../include/dynamo_hip.h"
#include "dd_split.h"

namespace dd {
namespace lw {

using cm::bf8;
using cm::f16v;
using cm::split2;

constexpr int NT = 256;
constexpr int KR = 16;                             // rows per wave and step = the K of one MFMA
constexpr int RED_ACC = 3 * 64 * 64 * 4;           // the accumulators of waves 1..3, [wave - 1][register][lane]
constexpr int RED_BIAS = 4 * 2 * 64 * 4;           // bias sums [wave][row half][channel]
constexpr int BLOCK = 64 * 64 + 64;                // floats of one partial: the weights [co][ci], then the bias sums

template <int NP>
__global__ __launch_bounds__(NT, 2) void linear_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, int M, int cout, int cin, int ci_blocks,
                                                             int nblk, int nks, int want_bias, float* __restrict__ partial) {
  __shared__ __align__(16) unsigned char smem[RED_ACC + RED_BIAS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // The nblk * nks work items, row range by row range, are dealt to the eight XCDs (workgroup L runs on XCD L % 8) in eight contiguous
  // runs of equal length: the workgroups that share rows of g and x share an L2, and no XCD gets more than its 64 resident workgroups
  // (two per CU) -- with one item more than that on an XCD the whole kernel waits for a second round.
  const int L = blockIdx.x, xcd = L & 7, total = nblk * nks;
  const int w0 = (int)((long long)total * xcd / 8), w1 = (int)((long long)total * (xcd + 1) / 8), w = w0 + (L >> 3);
  if (w >= w1) return;
  const int ks = w / nblk, blk = w - ks * nblk;
  const int cb = blk / ci_blocks, ib = blk - cb * ci_blocks, co0 = cb * 64, ci0 = ib * 64;
  const int groups = (M + KR - 1) / KR;
  const int u0 = (int)((long long)groups * ks / nks), u1 = (int)((long long)groups * (ks + 1) / nks);
  const bool co_hi = cout - co0 > 32, ci_hi = cin - ci0 > 32;           // the second 32-channel half of the block exists

  // this lane's fragment: channel lane & 31 (+ 32 in the second half), rows (lane >> 5) * 8 .. + 7 of the group
  const int ch = lane & 31, half = lane >> 5;
  // Byte offsets of (first row of this lane in the group, channel) from g / x: M * max(cout, cin) < 2^30.  A channel beyond the layer's
  // reads channel 0 instead and is NOT zeroed: element (co, ci) of the product depends on column co of g and column ci of x alone, and
  // the rows and columns of the block beyond cout / cin are never stored.
  unsigned og[2], ox[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    og[m] = 4u * (co0 + m * 32 + ch < cout ? co0 + m * 32 + ch : 0);
    ox[m] = 4u * (ci0 + m * 32 + ch < cin ? ci0 + m * 32 + ch : 0);
  }
  const unsigned g_last = 4u * (unsigned)(M - 1) * cout, x_last = 4u * (unsigned)(M - 1) * cin;          // the last row
  // Row k of the lane's eight is the wave-uniform pointer g + k * cout plus the lane's 32-bit offset: one scalar base per row, kept for
  // the whole loop, and no 64-bit address arithmetic per load.  Only a group that crosses M (the last one) clamps its rows to the last.
  const char* gk[8];
  const char* xk[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    gk[k] = reinterpret_cast<const char*>(g + (size_t)k * cout);
    xk[k] = reinterpret_cast<const char*>(x + (size_t)k * cin);
  }
  float rg[2][8], rx[2][8];                // [channel half][row]
  auto fetch = [&](int u) {                // a group that lies inside M: 32 loads, none of them conditional
    const unsigned r0 = (unsigned)(u * KR + half * 8);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const unsigned bg = 4u * r0 * cout + og[m], bx = 4u * r0 * cin + ox[m];
#pragma unroll
      for (int k = 0; k < 8; ++k) rg[m][k] = *reinterpret_cast<const float*>(gk[k] + bg);
#pragma unroll
      for (int k = 0; k < 8; ++k) rx[m][k] = *reinterpret_cast<const float*>(xk[k] + bx);
    }
  };
  auto fetch_last = [&](int u) {           // the group that crosses M: rows beyond M re-read the last row and count as zeros
    const int r0 = u * KR + half * 8;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float gv = *reinterpret_cast<const float*>(gk[0] + (min(4u * (unsigned)(r0 + k) * cout, g_last) + og[m]));
        rg[m][k] = r0 + k < M ? gv : 0.f;
        const float xv = *reinterpret_cast<const float*>(xk[0] + (min(4u * (unsigned)(r0 + k) * cin, x_last) + ox[m]));
        rx[m][k] = r0 + k < M ? xv : 0.f;         // (0 * Inf of an unzeroed last row would be a NaN the true sum does not have)
      }
  };
  float bsum[2] = {0.f, 0.f};
  uint4 af[2][3], bfr[2][3];
  // eight rows of one channel -> the three pieces of a fragment; returns their fp32 sum in row order
  auto split8 = [&](const float (&v)[8], uint4 (&f)[3]) -> float {
    unsigned p[3][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) split2(v[2 * q], v[2 * q + 1], p[0][q], p[1][q], p[2][q]);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) f[pc] = make_uint4(p[pc][0], p[pc][1], p[pc][2], p[pc][3]);
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  };
  auto split = [&]() {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      bsum[m] += split8(rg[m], af[m]);
      split8(rx[m], bfr[m]);
    }
  };

  f16v acc[2][2];                          // [co half][ci half]
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

  auto mma = [&]() {
#pragma unroll
    for (int t = 6 - NP; t < 6; ++t)       // the small partial products first; consecutive MFMAs go to different accumulators
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          if ((m == 0 || co_hi) && (n == 0 || ci_hi))
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, af[m][cm::kPieceA[t]]), __builtin_bit_cast(bf8, bfr[n][cm::kPieceB[t]]),
                                                                acc[m][n], 0, 0, 0);
  };
  const int full = M / KR, u1f = min(u1, full);          // the groups of this range that lie inside M
  int u = u0 + wave;
  if (u < u1f) fetch(u);
  for (; u < u1f; u += 4) {
    split();
    fetch(min(u + 4, full - 1));           // in flight under the MFMAs
    mma();
  }
  if (full < groups && u0 <= full && full < u1 && ((full - u0) & 3) == wave) {          // wave-uniform: the last, partial group is this wave's
    fetch_last(full);
    split();
    mma();
  }

  // the four waves' sums meet in LDS in wave order; wave 0 writes the partial
  float* const r_acc = reinterpret_cast<float*>(smem);
  float* const r_bias = reinterpret_cast<float*>(smem + RED_ACC);
  if (wave > 0) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) r_acc[((wave - 1) * 64 + (m * 2 + n) * 16 + r) * 64 + lane] = acc[m][n][r];
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) r_bias[(wave * 2 + half) * 64 + m * 32 + ch] = bsum[m];
  __syncthreads();
  if (wave != 0) return;
  float* const P = partial + ((size_t)blk * nks + ks) * BLOCK;
  // C layout: column (ci) = lane & 31, row (co) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = ((m * 2 + n) * 16 + r) * 64 + lane;
        const float s = (acc[m][n][r] + r_acc[i]) + (r_acc[64 * 64 + i] + r_acc[2 * 64 * 64 + i]);
        const int co = m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), ci = n * 32 + (lane & 31);
        if (co0 + co < cout && ci0 + ci < cin) P[co * 64 + ci] = s;
      }
  if (want_bias && ib == 0 && co0 + lane < cout) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += r_bias[k * 64 + lane];           // (wave, row half) in order
    P[64 * 64 + lane] = s;
  }
}

// g_weight (cout, cin) and g_bias (cout) = the sums over the nks partials of every block, in order.  The shape of conv_wgrad_fold_kernel:
// a workgroup takes 64 consecutive elements of the result (the weights, then the bias), its four waves take the partials k = wave,
// wave + 4, ... (eight loads in flight per lane) and meet in LDS in wave order.
__global__ __launch_bounds__(256) void linear_wgrad_fold_kernel(const float* __restrict__ partial, int nks, int cin, int cout, int ci_blocks, int total,
                                                                float* __restrict__ gw, float* __restrict__ gb) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int idx = blockIdx.x * 64 + lane, nw = cout * cin;
  const bool in = idx < total;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (in) {
    size_t first;                        // this element in the first partial of its block
    if (idx < nw) {
      const int co = idx / cin, ci = idx - co * cin;
      first = ((size_t)(co >> 6) * ci_blocks + (ci >> 6)) * nks * BLOCK + (co & 63) * 64 + (ci & 63);
    } else {
      const int co = idx - nw;
      first = (size_t)(co >> 6) * ci_blocks * nks * BLOCK + 64 * 64 + (co & 63);
    }
    const float* P = partial + first;
    int k = wave;
    for (; k + 28 < nks; k += 32) {
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += P[(size_t)(k + 4 * j) * BLOCK];
    }
    for (; k < nks; k += 4) s[0] += P[(size_t)k * BLOCK];
  }
  red[wave][lane] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (wave == 0 && in) {
    const float v = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    if (idx < nw) gw[idx] = v;
    else gb[idx - nw] = v;
  }
}

static int blocks_of(int cout, int cin) { return ((cout + 63) / 64) * ((cin + 63) / 64); }

static int splits(int M, int cout, int cin) {
  const int groups = (M + KR - 1) / KR;
  const char* env = getenv("DD_LINEAR_WGRAD_SPLITS");
  // FOR TESTS ONLY (more row ranges than row groups: empty ranges; or one), at most 4096.  It is read again by every call, and callers
  // may remember dd_linear_wgrad_workspace_bytes per shape (hipops.functions._ws_bytes does): set it before a process's first call and
  // leave it -- a change in between makes dd_linear_wgrad_n refuse the remembered workspace as too small (hipErrorInvalidValue).
  if (env && atoi(env) >= 1) return atoi(env) < 4096 ? atoi(env) : 4096;
  int n = 512 / blocks_of(cout, cin);                    // two workgroups per CU in all and not one more (a second round doubles the time)
  if (n > groups / 16) n = groups / 16;                  // at least four steps per wave
  return n < 1 ? 1 : n;
}

template <int NP>
static int launch(const float* g, const float* x, int M, int cout, int cin, int nks, int want_bias, float* partial, hipStream_t s) {
  const int ci_blocks = (cin + 63) / 64, nblk = blocks_of(cout, cin);
  hipLaunchKernelGGL(linear_wgrad_kernel<NP>, dim3((nblk * nks + 7) / 8 * 8), dim3(NT), 0, s, g, x, M, cout, cin, ci_blocks, nblk, nks, want_bias, partial);
  return (int)hipGetLastError();
}

}  // namespace lw
}  // namespace dd

extern "C" int dd_linear_wgrad_supported(int M, int cout, int cin) {
  return (M >= 1 && cout >= 4 && cin >= 4 && cout % 4 == 0 && cin % 4 == 0 && cout <= 8192 && cin <= 8192 &&
          (size_t)M * (size_t)(cout > cin ? cout : cin) < (1ull << 30)) ? 1 : 0;
}

extern "C" size_t dd_linear_wgrad_workspace_bytes(int M, int cout, int cin) {
  using namespace dd::lw;
  if (!dd_linear_wgrad_supported(M, cout, cin)) return 0;
  return (size_t)blocks_of(cout, cin) * splits(M, cout, cin) * BLOCK * sizeof(float);
}

extern "C" int dd_linear_wgrad_n(const float* g_out, const float* x, int M, int cout, int cin, int products, float* g_weight, float* g_bias, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  using namespace dd::lw;
  if (!g_out || !x || !g_weight || !workspace || !dd_linear_wgrad_supported(M, cout, cin)) return (int)hipErrorInvalidValue;
  if (products != 6 && products != 3 && products != 1) return (int)hipErrorInvalidValue;
  if (workspace_bytes < dd_linear_wgrad_workspace_bytes(M, cout, cin)) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<unsigned long long>(x) | reinterpret_cast<unsigned long long>(g_out)) & 3ull) return (int)hipErrorInvalidValue;          // dword loads only
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nks = splits(M, cout, cin), want_bias = g_bias ? 1 : 0;
  float* part = static_cast<float*>(workspace);
  const int rc = products == 6 ? launch<6>(g_out, x, M, cout, cin, nks, want_bias, part, s)
               : products == 3 ? launch<3>(g_out, x, M, cout, cin, nks, want_bias, part, s)
                               : launch<1>(g_out, x, M, cout, cin, nks, want_bias, part, s);
  if (rc != 0) return rc;
  const int total = cout * cin + (g_bias ? cout : 0);
  hipLaunchKernelGGL(linear_wgrad_fold_kernel, dim3((total + 63) / 64), dim3(256), 0, s, static_cast<const float*>(workspace), nks, cin, cout, (cin + 63) / 64, total,
                     g_weight, g_bias);
  return (int)hipGetLastError();
}

extern "C" int dd_linear_wgrad(const float* g_out, const float* x, int M, int cout, int cin, float* g_weight, float* g_bias, void* workspace, size_t workspace_bytes,
                               void* stream) {
  return dd_linear_wgrad_n(g_out, x, M, cout, cin, 6, g_weight, g_bias, workspace, workspace_bytes, stream);
}
