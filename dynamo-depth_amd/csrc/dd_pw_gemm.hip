// dd_pw_gemm.hip -- LiteMono's point-wise Linears (reference networks/depth_encoder.py:200-203,216-224,262-272: pwconv1 -> GELU -> pwconv2
// on a channels-last (B,H,W,C) tensor, C = 64 / 128 / 224, hidden 6C) at fp32 accuracy on the bf16 matrix pipe (gfx950).
//
// The BLAS back-end runs these GEMMs on the fp32 MFMA forms and they are short in one dimension (K = C or N = C): 70-100 us each for
// 140 MB of hidden activations, with an element-wise exact-GELU pass (read + write of the hidden tensor) between them.  Here:
//   * y[M,N] = act_in(x[M,K]) . W[N,K]^T + bias with every fp32 operand split exactly into three bf16 pieces and six partial products
//     on v_mfma_f32_32x32x16_bf16 (dd_split.h; the arithmetic of dd_conv_mfma.hip, pinned by tests/test_split_bf16.py);
//   * act_in = the erf GELU applied to the A operand while it is split ("GELU prologue"): the second Linear reads the first one's
//     pre-activation, the activated tensor never exists in memory.  erf is a branch-free two-range polynomial (8e-8 absolute error,
//     fitted and checked against scipy on the CPU: ~25 VALU instructions where the device library's erff takes ~55) -- with the
//     library's the prologue, not HBM, bounded the kernel;
//   * a workgroup (NW waves) owns 32*RB*NW rows and NG 32-column blocks; K goes in chunks of 32: the chunk of A is fetched with
//     coalesced 16-byte loads (eight lanes per row; prefetched one chunk ahead), activated, split ONCE and staged in LDS as three bf16
//     planes with an 80-byte row pitch (conflict-free 16-byte fragment reads); the B fragments come in fragment order from a pack
//     (dd_mlp_pack, once per step) through LDS, each wave fetching its share.  (The first version read every lane's A fragment straight
//     from global memory -- 32 cache lines per load instruction -- and every wave its own B fragments: correct, and bound by the
//     texture addresser at 2-3x the time of this one.)
//   * store tail of both kernels (dd_store_tile.h): the bias is fetched before the main loop, a tile with all of its rows and columns
//     stores straight-line, edge tiles test every store.
// Bound: HBM for the wide side (the 6C-wide tensor is written or read once, 4 bytes per element).
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <type_traits>

#include "../../include/dynamo_hip.h"
#include "dd_attr.h"
#include "dd_split.h"
#include "dd_store_tile.h"

namespace dd {
namespace pw {

using cm::bf8;
using cm::f16v;
using cm::split2;
using cm::store_acc32;
using cm::StoreF32;
using cm::tile_bias;

constexpr int FRAG_U4 = 64;          // uint4 per fragment (64 lanes x 16 bytes)

// pack layout: [n block][k step][piece][lane] x 16 bytes.  lane l of a fragment holds, for output column nb * 32 + (l & 31), the
// inputs ks * 16 + (l >> 5) * 8 + 0..7.  The weight is addressed through two element strides: (s_n, s_k) = (K, 1) packs W (N,K) for
// x . W^T, (1, N') packs the transpose of a (N',N) matrix for the data gradient.
struct PackRegion {
  const float* w;
  long long s_n, s_k;
  int N, K, first;                   // first fragment (n block, k step) of the region inside the launch
  int fused;                         // 1: the second Linear's operand for mlp_fwd_kernel -- [k block of 32][n block][step][piece][lane],
                                     // the lane's eight k in the order in which the first GEMM's accumulator registers hold them
  uint4* out;
};
constexpr int MAX_REGIONS = 5;
struct PackArgs {
  PackRegion r[MAX_REGIONS];
  int count, total;
};

// The C layout of a 32x32 accumulator puts row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) in register r.  mlp_fwd_kernel computes the hidden
// tile TRANSPOSED (hidden index = accumulator row, pixel = column = lane & 31) and feeds registers 8 j .. 8 j + 7 of a lane as the
// eight k values of step j of the second GEMM without moving them: element e of step j of lane-half hh is hidden index
__host__ __device__ inline int fused_k(int j, int hh, int e) { return (e & 3) + 8 * (2 * j + (e >> 2)) + 4 * hh; }

__global__ __launch_bounds__(256) void pw_pack_kernel(const PackArgs a) {
  const int gid = blockIdx.x * 256 + threadIdx.x, lane = gid & 63;
  int f = gid >> 6;
  if (f >= a.total) return;
  int ri = 0;
#pragma unroll
  for (int i = 1; i < MAX_REGIONS; ++i)
    if (i < a.count && f >= a.r[i].first) ri = i;
  PackRegion rg = a.r[0];
#pragma unroll
  for (int i = 1; i < MAX_REGIONS; ++i)
    if (ri == i) rg = a.r[i];
  f -= rg.first;
  const int KS = rg.K >> 4;
  int nb, kk[8];
  if (rg.fused) {
    const int NBLK = (rg.N + 31) >> 5, j = f & 1, hb = (f >> 1) / NBLK;
    nb = (f >> 1) - hb * NBLK;
#pragma unroll
    for (int e = 0; e < 8; ++e) kk[e] = hb * 32 + fused_k(j, lane >> 5, e);
  } else {
    nb = f / KS;
    const int ks = f - nb * KS;
#pragma unroll
    for (int e = 0; e < 8; ++e) kk[e] = ks * 16 + (lane >> 5) * 8 + e;
  }
  const int n = nb * 32 + (lane & 31);
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = n < rg.N ? rg.w[(long long)n * rg.s_n + (long long)kk[e] * rg.s_k] : 0.f;
  unsigned p[3][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) split2(v[2 * q], v[2 * q + 1], p[0][q], p[1][q], p[2][q]);
  uint4* dst = rg.out + ((size_t)f * 3) * FRAG_U4 + lane;
#pragma unroll
  for (int pc = 0; pc < 3; ++pc) dst[pc * FRAG_U4] = make_uint4(p[pc][0], p[pc][1], p[pc][2], p[pc][3]);
}

// erf(a), branch-free: a (1 + P(a^2)) for |a| <= 0.93, sign(a) (1 - exp(t R(t) - t)) beyond, t = min(|a|, 4.05).  Coefficients:
// least squares on Chebyshev nodes in float64, rounded to fp32; evaluated in fp32 the maximum error against scipy.special.erf over
// [-6, 6] is 8.3e-8 absolute (1.0e-7 relative) and the GELU below is within 4.5e-7 of float64 for |x| <= 6.
__device__ __forceinline__ float erf_poly(float a) {
  const float t = fminf(fabsf(a), 4.05f), s = a * a;
  float r = -0.0005972102517262101f;
  r = fmaf(r, s, 0.004989944398403168f);
  r = fmaf(r, s, -0.02676478400826454f);
  r = fmaf(r, s, 0.11281778663396835f);
  r = fmaf(r, s, -0.37612491846084595f);
  r = fmaf(r, s, 0.12837915122509003f);
  const float small = fmaf(r, a, a);
  float q = 9.955634823199944e-07f;
  q = fmaf(q, t, -3.347820893395692e-05f);
  q = fmaf(q, t, 0.0004920329665765166f);
  q = fmaf(q, t, -0.004276696592569351f);
  q = fmaf(q, t, 0.025077397003769875f);
  q = fmaf(q, t, -0.10777396708726883f);
  q = fmaf(q, t, -0.6342049241065979f);
  q = fmaf(q, t, -0.12888674437999725f);
  q = fmaf(q, t, -t);
  const float large = copysignf(1.f - __expf(q), a);
  return t > 0.93f ? large : small;
}

__device__ __forceinline__ float gelu_erf(float v) { return (v * 0.5f) * (1.f + erf_poly(v * 0.70710678118654752440f)); }

constexpr int KC = 32;               // contraction elements per chunk: two MFMA steps
constexpr int RSTR = 80;             // bytes per row and piece in LDS: 32 bf16 + 16 bytes of padding
constexpr int FRAG = 1024;           // bytes per fragment

template <int NW, int RB, int NG>
constexpr int lds_bytes() { return 3 * (32 * RB * NW) * RSTR + NG * 6 * FRAG; }

template <int NW, int RB, int NG, bool GELU_IN>
__global__ __launch_bounds__(NW * 64, 2) void pw_gemm_kernel(const float* __restrict__ x, const uint4* __restrict__ pack, const float* __restrict__ bias,
                                                             int M, int K, int N, float* __restrict__ y) {
  constexpr int NT = NW * 64, MT = 32 * RB * NW;
  constexpr int A_PIECE = MT * RSTR, A_BYTES = 3 * A_PIECE;
  constexpr int BFR = NG * 6;                    // B fragments per chunk: [column block][step][piece]
  constexpr int BR = (BFR + NW - 1) / NW;        // rounds: wave w moves fragment w + NW r
  constexpr int PA = MT * 8 / NT;                // 16-byte loads of A per thread and chunk (eight per row)
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned char* const s_b = smem + A_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = (int)blockIdx.x * MT, nb0 = (int)blockIdx.y * NG;
  const int KS = K >> 4, NCH = K / KC, NBLK = (N + 31) >> 5;

  const float* a_src[PA];
  int a_lds[PA];
#pragma unroll
  for (int p = 0; p < PA; ++p) {
    const int i = tid + p * NT, r = i >> 3, q = i & 7;
    a_src[p] = x + (size_t)min(row0 + r, M - 1) * K + q * 4;          // rows beyond M repeat the last one (never stored)
    a_lds[p] = r * RSTR + q * 8;
  }
  const uint4* b_src[BR];
#pragma unroll
  for (int r = 0; r < BR; ++r) {
    const int f = wave + NW * r < BFR ? wave + NW * r : 0, n = f / 6, j = f - n * 6;
    b_src[r] = pack + (size_t)min(nb0 + n, NBLK - 1) * KS * 192 + j * 64 + lane;
  }
  float4 areg[PA];
  uint4 breg[BR];
  auto fetch = [&](int c) {
#pragma unroll
    for (int p = 0; p < PA; ++p) areg[p] = *reinterpret_cast<const float4*>(a_src[p] + c * KC);
#pragma unroll
    for (int r = 0; r < BR; ++r) breg[r] = b_src[r][(size_t)c * 384];        // two steps x three pieces x 64 lanes
  };
  auto stage = [&]() {
#pragma unroll
    for (int p = 0; p < PA; ++p) {
      float v[4] = {areg[p].x, areg[p].y, areg[p].z, areg[p].w};
      if (GELU_IN) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
      }
      unsigned a1, a2, a3, b1, b2, b3;
      split2(v[0], v[1], a1, a2, a3);
      split2(v[2], v[3], b1, b2, b3);
      *reinterpret_cast<uint2*>(smem + a_lds[p]) = make_uint2(a1, b1);
      *reinterpret_cast<uint2*>(smem + A_PIECE + a_lds[p]) = make_uint2(a2, b2);
      *reinterpret_cast<uint2*>(smem + 2 * A_PIECE + a_lds[p]) = make_uint2(a3, b3);
    }
#pragma unroll
    for (int r = 0; r < BR; ++r)
      if (wave + NW * r < BFR) *reinterpret_cast<uint4*>(s_b + (wave + NW * r) * FRAG + lane * 16) = breg[r];
  };
  // LDS-only barrier: this wave's LDS operations have completed, its global prefetch stays in flight
  auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

  f16v acc[RB][NG];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int n = 0; n < NG; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rb][n][r] = 0.f;

  const unsigned char* a_lane = smem + (wave * 32 * RB + (lane & 31)) * RSTR + (lane >> 5) * 16;
  const unsigned char* b_lane = s_b + lane * 16;
  float bv[NG];          // what the epilogue adds, fetched first (dd_store_tile.h)
#pragma unroll
  for (int n = 0; n < NG; ++n) bv[n] = tile_bias(bias, (nb0 + n) * 32 + (lane & 31), N, pack);
  fetch(0);
  for (int c = 0; c < NCH; ++c) {
    lds_barrier();                         // the previous chunk's fragment reads are done
    stage();
    lds_barrier();
    fetch(min(c + 1, NCH - 1));            // lands under this chunk's MFMAs (the last chunk re-reads itself: no branch)
#pragma unroll
    for (int ksi = 0; ksi < 2; ++ksi) {
      uint4 af[RB][3], bf[NG][3];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) af[rb][pc] = *reinterpret_cast<const uint4*>(a_lane + rb * 32 * RSTR + ksi * 32 + pc * A_PIECE);
#pragma unroll
      for (int n = 0; n < NG; ++n)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) bf[n][pc] = *reinterpret_cast<const uint4*>(b_lane + ((n * 2 + ksi) * 3 + pc) * FRAG);
#pragma unroll
      for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int n = 0; n < NG; ++n)
            acc[rb][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, af[rb][cm::kPieceA[t]]), __builtin_bit_cast(bf8, bf[n][cm::kPieceB[t]]),
                                                                 acc[rb][n], 0, 0, 0);
    }
  }
  // store tail (dd_store_tile.h): a tile with all of its rows and columns stores straight-line, edge tiles test every store
  auto tail = [&](auto full) {
#pragma unroll
    for (int n = 0; n < NG; ++n) {
      const int co = (nb0 + n) * 32 + (lane & 31);
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const int row = row0 + (wave * RB + rb) * 32 + 4 * (lane >> 5);
        store_acc32<decltype(full)::value>(acc[rb][n], bv[n], y + (size_t)row * N + co, (size_t)N, co < N ? M - row : 0, StoreF32{});
      }
    }
  };
  if (row0 + MT <= M && (nb0 + NG) * 32 <= N) tail(std::true_type{});
  else tail(std::false_type{});
}

template <int NW, int RB, int NG, bool GELU_IN>
static int launch(const float* x, const void* pack, const float* bias, int M, int K, int N, float* y, hipStream_t stream) {
  constexpr int MT = 32 * RB * NW;
  auto kern = pw_gemm_kernel<NW, RB, NG, GELU_IN>;
  static dd::LdsAttrOnce lds_attr;          // per instantiation and device (dd_attr.h)
  if (const int rc = lds_attr.ensure(reinterpret_cast<const void*>(kern), (int)((lds_bytes<NW, RB, NG>())))) return rc;
  const int NBLK = (N + 31) / 32;
  constexpr int lds = lds_bytes<NW, RB, NG>();
  hipLaunchKernelGGL(kern, dim3((M + MT - 1) / MT, (NBLK + NG - 1) / NG), dim3(NW * 64), lds, stream, x, static_cast<const uint4*>(pack), bias,
                     M, K, N, y);
  return (int)hipGetLastError();
}

// Which tile a workgroup takes.  Up to two column blocks (N <= 64): 64 rows per wave on two column blocks; more: 32 rows per wave on
// four column blocks (with K > N -- the wide tensor is the operand A -- N <= 128 is then ONE group: A is read, and its GELU evaluated,
// once).  Four waves per workgroup when that still gives ~400 workgroups, two otherwise.
template <bool GELU_IN>
static int dispatch(const float* x, const void* pack, const float* bias, int M, int K, int N, float* y, hipStream_t s) {
  const int NBLK = (N + 31) / 32;
  if (NBLK <= 2) {
    const int groups = 1;
    if ((M + 255) / 256 * groups >= 400) return launch<4, 2, 2, GELU_IN>(x, pack, bias, M, K, N, y, s);
    return launch<2, 2, 2, GELU_IN>(x, pack, bias, M, K, N, y, s);
  }
  const int groups = (NBLK + 3) / 4;
  if ((M + 127) / 128 * groups >= 400) return launch<4, 1, 4, GELU_IN>(x, pack, bias, M, K, N, y, s);
  return launch<2, 1, 4, GELU_IN>(x, pack, bias, M, K, N, y, s);
}

// ---- the whole block forward in one kernel (forward-only passes: the statistics-only side batch, evaluation) -------------------
// out (M,C) = GELU(x . W1^T + b1) . W2^T + b2 without the hidden tensor ever leaving the chip.  A wave owns 32 rows; their x fragments
// are split once and stay in registers.  Per block of 32 hidden units: the first GEMM TRANSPOSED (A operand = W1's fragments, B
// operand = the x fragments: accumulator row = hidden unit, column = pixel), bias + GELU on the sixteen accumulator registers, which
// then ARE the A operand of the second GEMM (pixel = lane & 31 in both layouts; registers 8 j .. 8 j + 7 are the eight k of step j in
// the order fused_k() gives, and dd_mlp_pack lays W2 out in that order) -- no transposition, no LDS round trip for activations.  The
// weight fragments of a hidden block (W1: C/16 x 3, W2: C/32 x 2 x 3 KB) go through LDS, shared by the four waves, prefetched into
// registers one block ahead.  HBM traffic: x once, out once (35 MB at stage 1 against ~600 for two GEMMs and an element-wise pass).
// NP: the partial products kept (6 / 3 / 1, the last NP of cm::kPieceA/B as in mlp_fwd224_kernel).
//
// MODE (the training pass of stages 1 and 2): the loop of mlp_fwd224_kernel's modes at the narrow widths.
//   MLP_TRAIN  besides the output, h = GELU(pre) and d = GELU'(pre) (M, 6C) go to memory straight from the accumulator: registers
//              4 q .. 4 q + 3 of a lane are sixteen contiguous bytes of its pixel's row, lanes l and l + 32 complete 32, the four q of a
//              hidden block a 128-byte line.  The pre-activation is never written; the output's arithmetic is MLP_FWD's, bit for bit.
//   MLP_DGRAD  dx = ((g . W2) * d) . W1: x = g, pack1 = W2^T as first operand, pack2 = W1^T in fused-k order, no bias, no GELU: the
//              accumulator times the d tile is stored as gpre (dd_linear_wgrad's operand) and is the second GEMM's A operand.
// Both keep two workgroups per CU, which at C = 128 (254 VGPRs as MLP_FWD) leaves no register for anything new, so they give up the
// weight prefetch in registers (48 at C = 128): the fragments go global -> LDS directly (global_load_lds_dwordx4), W1's and W2's parts of
// the buffer refilled in turn, each while the other one is being read -- two barriers per hidden block as before.  The d tile (4 KB per
// wave and hidden block, accumulator layout) takes the same road into a buffer of the wave's own, refilled once the wave has read it.
// LDS per workgroup: 25.5 KB (+16 KB d tiles) at C = 64, 51 KB (+16) at C = 128: two workgroups fit the CU's 160 KB in every mode.
// Rows at or beyond M are never stored (their x and d rows are clamped).
constexpr int MLP_FWD = 0, MLP_TRAIN = 1, MLP_DGRAD = 2;
constexpr int MLP_DTILE = 4096;                                 // one wave's d tile of a hidden block: 32 pixels x 32 hidden units

template <int C, int NP, int MODE>
__global__ __launch_bounds__(256, 2) void mlp_fwd_kernel(const float* __restrict__ x, const uint4* __restrict__ pack1, const uint4* __restrict__ pack2,
                                                         const float* __restrict__ b1, const float* __restrict__ b2, int M, float* __restrict__ y,
                                                         const float* __restrict__ aux_in, float* __restrict__ out_a, float* __restrict__ out_b) {
  constexpr int KS1 = C / 16, NB2 = C / 32, HID = 6 * C, NHB = HID / 32;
  constexpr int NF1 = KS1 * 3, NF2 = NB2 * 6, NF = NF1 + NF2;      // fragments per hidden block
  constexpr int BR = MODE == MLP_FWD ? (NF + 3) / 4 : 1;
  static_assert(NF1 % 4 == 0 && NF2 % 4 == 0, "every wave moves the same number of fragments");
  extern __shared__ __align__(16) unsigned char smem[];            // [NF fragments] | b1 (HID floats) | MLP_DGRAD: a d tile per wave
  float* const s_b1 = reinterpret_cast<float*>(smem + NF * FRAG);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hh = lane >> 5;
  const int row0 = (int)blockIdx.x * 128 + wave * 32;
  // this lane's pixel in the (M, 6C) tensors: element offset of its hidden unit 4 hh (the host keeps M * 6C * 4 below 2^32)
  const bool row_ok = row0 + (lane & 31) < M;
  const unsigned aoff = (unsigned)min(row0 + (lane & 31), M - 1) * (unsigned)HID + 4u * hh;

  if (MODE != MLP_DGRAD)
    for (int i = tid; i < HID; i += 256) s_b1[i] = b1[i];
  // x fragments of this wave's 32 rows (B operand of the first GEMM): lane = pixel lane & 31, channels ks * 16 + hh * 8 .. + 7
  uint4 xf[KS1][3];
  {
    const float* xp = x + (size_t)min(row0 + (lane & 31), M - 1) * C + hh * 8;
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
      const float4 v0 = *reinterpret_cast<const float4*>(xp + ks * 16), v1 = *reinterpret_cast<const float4*>(xp + ks * 16 + 4);
      unsigned p[3][4];
      split2(v0.x, v0.y, p[0][0], p[1][0], p[2][0]);
      split2(v0.z, v0.w, p[0][1], p[1][1], p[2][1]);
      split2(v1.x, v1.y, p[0][2], p[1][2], p[2][2]);
      split2(v1.z, v1.w, p[0][3], p[1][3], p[2][3]);
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) xf[ks][pc] = make_uint4(p[pc][0], p[pc][1], p[pc][2], p[pc][3]);
    }
  }
  // weight fragments of hidden block hb: round r moves fragment f = wave + 4 r (W1's first, then W2's)
  typedef unsigned u4v __attribute__((ext_vector_type(4)));        // (HIP's uint4 struct kept this array in scratch)
  u4v breg[BR];
  const u4v* w_src[BR];
  int w_step[BR];                                                   // uint4 between two hidden blocks of the round's source
#pragma unroll
  for (int r = 0; r < BR; ++r) {
    const int f = wave + 4 * r < NF ? wave + 4 * r : 0;             // wave-uniform
    w_src[r] = reinterpret_cast<const u4v*>(f < NF1 ? pack1 + f * 64 : pack2 + (f - NF1) * 64) + lane;
    w_step[r] = (f < NF1 ? NF1 : NF2) * 64;
  }
  auto fetch = [&](int hb) {
#pragma unroll
    for (int r = 0; r < BR; ++r) breg[r] = w_src[r][(size_t)hb * w_step[r]];
  };
  auto store_w = [&]() {
#pragma unroll
    for (int r = 0; r < BR; ++r)
      if (wave + 4 * r < NF) *reinterpret_cast<u4v*>(smem + (wave + 4 * r) * FRAG + lane * 16) = breg[r];
  };
  auto lds_barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

  f16v acc2[NB2];
#pragma unroll
  for (int n = 0; n < NB2; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[n][r] = 0.f;
  const unsigned char* w_lane = smem + lane * 16;

  float bv[NB2];         // the second bias, fetched first (dd_store_tile.h)
#pragma unroll
  for (int n = 0; n < NB2; ++n) bv[n] = tile_bias(b2, n * 32 + (lane & 31), C, pack2);
  // first GEMM, transposed: h^T (32 hidden x 32 pixels) = W1 block . x^T
  auto gemm1 = [&](f16v& acc1) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
      uint4 wf[3];
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) wf[pc] = *reinterpret_cast<const uint4*>(w_lane + (ks * 3 + pc) * FRAG);
#pragma unroll
      for (int t = 6 - NP; t < 6; ++t)
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, wf[cm::kPieceA[t]]), __builtin_bit_cast(bf8, xf[ks][cm::kPieceB[t]]), acc1, 0, 0, 0);
    }
  };
  // what stands between the two GEMMs, on the accumulator: register r holds hidden unit hb * 32 + (r & 3) + 8 (r >> 2) + 4 hh of pixel
  // lane & 31.  MLP_FWD: bias + GELU.  MLP_TRAIN: the same (gelu_erf's arithmetic) and GELU' (gelu_pair_kernel's), both stored a quad at
  // a time.  MLP_DGRAD: times the d tile, stored as gpre.
  auto store_quad = [&](float* __restrict__ out, int hb, int q, const float* v) __attribute__((always_inline)) {
    if (row_ok) *reinterpret_cast<float4*>(out + aoff + hb * 32 + 8 * q) = make_float4(v[0], v[1], v[2], v[3]);
  };
  // quad q: registers 4 q .. 4 q + 3 -> hv (h, or gpre); MLP_TRAIN: GELU' -> dv and h's two factors -> fx, fy; nothing is stored here
  auto act_quad = [&](const f16v& acc1, int hb, int q, float (&hv)[16], float* dv, float* fx, float* fy) __attribute__((always_inline)) {
    if (MODE == MLP_DGRAD) {
      const float4 dq = *reinterpret_cast<const float4*>(smem + NF * FRAG + HID * 4 + wave * MLP_DTILE + q * FRAG + lane * 16);
      hv[4 * q + 0] = acc1[4 * q + 0] * dq.x;
      hv[4 * q + 1] = acc1[4 * q + 1] * dq.y;
      hv[4 * q + 2] = acc1[4 * q + 2] * dq.z;
      hv[4 * q + 3] = acc1[4 * q + 3] * dq.w;
      return;
    }
    const float4 bq = *reinterpret_cast<const float4*>(s_b1 + hb * 32 + 8 * q + 4 * hh);
    const float bqv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = acc1[4 * q + e] + bqv[e];
      if (MODE == MLP_TRAIN) {                       // gelu_erf's expression for h, gelu_pair_kernel's arithmetic for d
        const float er = 1.f + erf_poly(v * 0.70710678118654752440f);
        const float pdf = __expf(-0.5f * v * v) * 0.3989422804014327f;
        fx[e] = v * 0.5f;
        fy[e] = er;
        hv[4 * q + e] = fx[e] * fy[e];
        dv[e] = fmaf(v, pdf, 0.5f * er);
      } else {
        hv[4 * q + e] = gelu_erf(v);
      }
    }
  };
  // second GEMM: out (32 pixels x C) += h (A operand, straight from the registers) . W2 block, in two steps of sixteen hidden units
  auto split_h = [&](const float (&hv)[16], int j, uint4 (&hf)[3]) __attribute__((always_inline)) {
    unsigned p[3][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) split2(hv[8 * j + 2 * q], hv[8 * j + 2 * q + 1], p[0][q], p[1][q], p[2][q]);
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) hf[pc] = make_uint4(p[pc][0], p[pc][1], p[pc][2], p[pc][3]);
  };
  auto gemm2_step = [&](int j, const uint4 (&hf)[3]) __attribute__((always_inline)) {
#pragma unroll
    for (int n = 0; n < NB2; ++n) {
      uint4 wf[3];
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) wf[pc] = *reinterpret_cast<const uint4*>(w_lane + (NF1 + (n * 2 + j) * 3 + pc) * FRAG);
#pragma unroll
      for (int t = 6 - NP; t < 6; ++t)
        acc2[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, hf[cm::kPieceA[t]]), __builtin_bit_cast(bf8, wf[cm::kPieceB[t]]), acc2[n], 0, 0, 0);
    }
  };
  if (MODE == MLP_FWD) {
    fetch(0);
    for (int hb = 0; hb < NHB; ++hb) {
      lds_barrier();                       // the previous block's fragment reads are done (first pass: b1 is in place after the next one)
      store_w();
      lds_barrier();
      fetch(min(hb + 1, NHB - 1));
      f16v acc1;
      float hv[16];
      gemm1(acc1);
#pragma unroll
      for (int q = 0; q < 4; ++q) act_quad(acc1, hb, q, hv, nullptr, nullptr, nullptr);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        uint4 hf[3];
        split_h(hv, j, hf);
        gemm2_step(j, hf);
      }
    }
  } else {
    // `count` fragments of one operand's hidden block hb -> LDS from fragment `first` on, without passing registers (1 KB per
    // wave-instruction, lane l at byte 16 l: the fragment's own order); wave w moves the fragments w, w + 4, ...  The compiler does not
    // count these loads: wait_barrier() waits for them, and nothing reads a buffer between its dma() and the next wait_barrier().
    const unsigned lds0 = (unsigned)reinterpret_cast<size_t>(smem);
    auto dma = [&](const uint4* pack, int count, int first, int hb) __attribute__((always_inline)) {
      const uint4* src = pack + (size_t)hb * (count * 64) + lane;
#pragma unroll
      for (int r = 0; r < count / 4; ++r) {
        const int f = wave + 4 * r;
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((first + f) * FRAG));
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src + f * 64), "s"(dst) : "memory");
      }
    };
    // MLP_DGRAD: this wave's d tile of hidden block hb in accumulator layout: instruction q moves, for every lane, the four hidden units
    // 8 q + 4 hh .. + 3 of its pixel (the accumulator's registers 4 q .. 4 q + 3) to byte q * 1024 + 16 lane of the wave's buffer
    auto dma_d = [&](int hb) __attribute__((always_inline)) {
      const float* src = aux_in + aoff + hb * 32;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(NF * FRAG + HID * 4 + wave * MLP_DTILE + q * FRAG));
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src + 8 * q), "s"(dst) : "memory");
      }
    };
    // every load, store and LDS operation of this wave has completed (what it moved has landed), then the barrier
    auto wait_barrier = [&]() __attribute__((always_inline)) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    dma(pack1, NF1, 0, 0);
    if (MODE == MLP_DGRAD) dma_d(0);
    for (int hb = 0; hb < NHB; ++hb) {
      wait_barrier();                      // the first operand of block hb (and its d tile, and b1) is in place, every wave has left block hb - 1
      dma(pack2, NF2, NF1, hb);            // lands under the first GEMM
      f16v acc1;
      float hv[16];
      gemm1(acc1);
      // Per half of the block: activation, split, stores.  MLP_TRAIN splits h = fx * fy with the first residual taken from the UNROUNDED
      // product (one fma): that is what the compiler makes of gelu_erf + split2 in MLP_FWD (it contracts h's last product into
      // a - bf16(a)), and here the conditional stores between product and split keep it from doing so -- y bit for bit needs the same
      // arithmetic, so it is spelled out; tests/test_mlp_narrow_train_gpu.py holds the two together.
      uint4 hf[2][3];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float dv[8], fx[8], fy[8];
        act_quad(acc1, hb, 2 * j, hv, dv, fx, fy);
        act_quad(acc1, hb, 2 * j + 1, hv, dv + 4, fx + 4, fy + 4);
        if (MODE == MLP_TRAIN) {
          unsigned p[3][4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            p[0][q] = cm::pack_bf16(hv[8 * j + 2 * q], hv[8 * j + 2 * q + 1]);
            const float ra = fmaf(fx[2 * q], fy[2 * q], -cm::lo_f(p[0][q])), rb = fmaf(fx[2 * q + 1], fy[2 * q + 1], -cm::hi_f(p[0][q]));
            p[1][q] = cm::pack_bf16(ra, rb);
            p[2][q] = cm::pack_bf16(ra - cm::lo_f(p[1][q]), rb - cm::hi_f(p[1][q]));
          }
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) hf[j][pc] = make_uint4(p[pc][0], p[pc][1], p[pc][2], p[pc][3]);
        } else {
          split_h(hv, j, hf[j]);
        }
#pragma unroll
        for (int q = 2 * j; q < 2 * j + 2; ++q) {
          store_quad(out_a, hb, q, hv + 4 * q);
          if (MODE == MLP_TRAIN) store_quad(out_b, hb, q, dv + 4 * (q - 2 * j));
        }
      }
      wait_barrier();                      // the second operand is in place, every wave has read the first one (and its own d tile)
      if (hb + 1 < NHB) {                  // lands under the second GEMM
        dma(pack1, NF1, 0, hb + 1);
        if (MODE == MLP_DGRAD) dma_d(hb + 1);
      }
      gemm2_step(0, hf[0]);
      gemm2_step(1, hf[1]);
    }
  }
  auto tail = [&](auto full) {
    const int row = row0 + 4 * hh;
#pragma unroll
    for (int n = 0; n < NB2; ++n)
      store_acc32<decltype(full)::value>(acc2[n], bv[n], y + (size_t)row * C + n * 32 + (lane & 31), (size_t)C, M - row, StoreF32{});
  };
  if ((int)blockIdx.x * 128 + 128 <= M) tail(std::true_type{});
  else tail(std::false_type{});
}

// MLP_FWD / MLP_TRAIN: y = the block's output (out_a = h, out_b = d for MLP_TRAIN).  MLP_DGRAD: x = g, aux_in = d, pack1 = W2^T, pack2 =
// W1^T fused, b1 = b2 = nullptr, y = dx, out_a = gpre.
template <int C, int NP, int MODE>
static int launch_fused(const float* x, const void* pack1, const void* pack2, const float* b1, const float* b2, int M, float* y, hipStream_t stream,
                        const float* aux_in = nullptr, float* out_a = nullptr, float* out_b = nullptr) {
  constexpr int lds = ((C / 16) * 3 + (C / 32) * 6) * FRAG + 6 * C * 4 + (MODE == MLP_DGRAD ? 4 * MLP_DTILE : 0);
  auto kern = mlp_fwd_kernel<C, NP, MODE>;
  static dd::LdsAttrOnce lds_attr;          // per instantiation and device (dd_attr.h)
  if (const int rc = lds_attr.ensure(reinterpret_cast<const void*>(kern), (int)(lds))) return rc;
  hipLaunchKernelGGL(kern, dim3((M + 127) / 128), dim3(256), lds, stream, x, static_cast<const uint4*>(pack1), static_cast<const uint4*>(pack2), b1, b2, M, y,
                     aux_in, out_a, out_b);
  return (int)hipGetLastError();
}

template <int C, int MODE>
static int launch_fused_n(int products, const float* x, const void* pack1, const void* pack2, const float* b1, const float* b2, int M, float* y,
                          hipStream_t stream, const float* aux_in, float* out_a, float* out_b) {
  return products == 6 ? launch_fused<C, 6, MODE>(x, pack1, pack2, b1, b2, M, y, stream, aux_in, out_a, out_b)
       : products == 3 ? launch_fused<C, 3, MODE>(x, pack1, pack2, b1, b2, M, y, stream, aux_in, out_a, out_b)
                       : launch_fused<C, 1, MODE>(x, pack1, pack2, b1, b2, M, y, stream, aux_in, out_a, out_b);
}

// ---- the same block at C = 224 (LiteMono's stage 3: 5 760 / 11 520 rows, hidden 1344 = 42 blocks) -----------------------------------
// mlp_fwd_kernel's arithmetic and operand layouts; what differs is what C = 224 does not fit:
//   * registers: 14 x 3 x fragments (168) + 7 output accumulators (112) want more than half the file, so ONE wave per SIMD
//     (__launch_bounds__(256, 1): 2 x 256 registers per lane, and what a VALU instruction touches must sit in the first 256) and NO
//     weight prefetch in registers (with one, even of 11 fragments per wave, the kernel spilled): the fragments go global -> LDS
//     directly, W1's and W2's halves of the LDS buffer refilled in turn, each while the other one is being read;
//   * parallelism: 128 rows per workgroup are 90 workgroups at 11 520 rows, so blockIdx.y takes one of S contiguous ranges of hidden
//     blocks ([s * 42 / S, (s + 1) * 42 / S): uneven when S does not divide 42, never empty for S <= 42) and stores ONE partial
//     [S][M][224]; mlp_fold224_kernel adds the partials in split order behind b2.  S = 1 stores the result itself.  No atomics, no
//     zero-fill, bit-reproducible for a given S;
//   * one wave per SIMD has nobody to hide its GELU behind, so the loop is skewed by one block: the first GEMM of block hb + 1 is issued
//     beside the bias + GELU + split of block hb (independent instructions in one scheduling region), then the second GEMM of block hb.
constexpr int C3 = 224, KS3 = C3 / 16, NB3 = C3 / 32, NHB3 = 6 * C3 / 32;
constexpr int NF3 = KS3 * 3;                                    // fragments per hidden block and operand: 14 x 3 = 7 x 2 x 3 = 42
constexpr int BR3 = (NF3 + 3) / 4;
constexpr int MLP3_LDS = 2 * NF3 * FRAG + 6 * C3 * 4;           // W1 block | W2 block | b1
static_assert(NF3 == NB3 * 6, "both operands of a hidden block have the same number of fragments");

//
// MODE (the training pass): the same loop with what the slices do exchanged.
//   MLP_TRAIN  the forward of a pass with a tape: besides the output, h = GELU(pre) and d = GELU'(pre) (M, 1344) go to memory straight from
//              the accumulator's slices -- registers 4 q .. 4 q + 3 of a lane are sixteen contiguous bytes of its pixel's row, lanes l and
//              l + 32 complete 32 -- so the backward needs no activation arithmetic.  The arithmetic of the output is MLP_FWD's, bit for bit.
//   MLP_DGRAD  the data gradient dx = ((g . W2) * d) . W1: x = g, pack1 = W2^T as first operand, pack2 = W1^T in fused-k order, no bias and
//              no GELU: the slice multiplies the accumulator by the d tile and stores gpre = (g . W2) * d (dd_linear_wgrad's operand),
//              which is also the second GEMM's A operand.  The d tile (4 KB per wave and hidden block) comes global -> LDS one block ahead
//              (four global_load_lds_dwordx4 per wave, per-lane addresses, two buffers per wave) and is read back in accumulator layout.
// Rows at or beyond M are never stored (their x rows are clamped).  A (row group, hidden block) pair belongs to one split: no fold.
// Stores count in vmcnt, in order, and wait_barrier() waits for all of them: the stores of h and gpre go out from the slices right BEHIND
// the mid-block barrier (the values are held for the split anyway), those of d when a quad is complete (at 252 VGPRs there is no room to
// hold them).
constexpr int MLP3_DTILE = MLP_DTILE;

template <int NP, int MODE>
__global__ __launch_bounds__(256, 1) void mlp_fwd224_kernel(const float* __restrict__ x, const uint4* __restrict__ pack1, const uint4* __restrict__ pack2,
                                                            const float* __restrict__ b1, const float* __restrict__ bias, int M, int S,
                                                            float* __restrict__ dst, const float* __restrict__ aux_in, float* __restrict__ out_a,
                                                            float* __restrict__ out_b) {
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned char* const s_w1 = smem;
  unsigned char* const s_w2 = smem + NF3 * FRAG;
  float* const s_b1 = reinterpret_cast<float*>(smem + 2 * NF3 * FRAG);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3, hh = lane >> 5;
  const int row0 = (int)blockIdx.x * 128 + wave * 32;
  const int split = (int)blockIdx.y, hb0 = split * NHB3 / S, hb1 = (split + 1) * NHB3 / S;
  // this lane's pixel in the (M, 1344) tensors: element offset of its hidden unit 4 hh (the host keeps M * 1344 * 4 below 2^32)
  const bool row_ok = row0 + (lane & 31) < M;
  const unsigned aoff = (unsigned)min(row0 + (lane & 31), M - 1) * (unsigned)(6 * C3) + 4u * hh;
  const unsigned char* const s_d = smem + MLP3_LDS + wave * 2 * MLP3_DTILE + lane * 16;       // MLP_DGRAD: this wave's two d tiles

  if (MODE != MLP_DGRAD)
    for (int i = tid; i < 6 * C3; i += 256) s_b1[i] = b1[i];
  uint4 xf[KS3][3];
  {
    const float* xp = x + (size_t)min(row0 + (lane & 31), M - 1) * C3 + hh * 8;
#pragma unroll
    for (int ks = 0; ks < KS3; ++ks) {
      const float4 v0 = *reinterpret_cast<const float4*>(xp + ks * 16), v1 = *reinterpret_cast<const float4*>(xp + ks * 16 + 4);
      unsigned p[3][4];
      split2(v0.x, v0.y, p[0][0], p[1][0], p[2][0]);
      split2(v0.z, v0.w, p[0][1], p[1][1], p[2][1]);
      split2(v1.x, v1.y, p[0][2], p[1][2], p[2][2]);
      split2(v1.z, v1.w, p[0][3], p[1][3], p[2][3]);
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) xf[ks][pc] = make_uint4(p[pc][0], p[pc][1], p[pc][2], p[pc][3]);
    }
  }
  // One operand's fragments of hidden block hb (both packs: 42 fragments per block) go global -> LDS without passing registers
  // (global_load_lds_dwordx4: 1 KB per wave-instruction, lane l at byte 16 l, which is the fragment's own order); wave w moves the
  // fragments w, w + 4, ...  The compiler does not count these loads: wait_barrier() waits for them, and nothing reads a buffer
  // between its dma() and the next wait_barrier().
  const unsigned lds0 = (unsigned)reinterpret_cast<size_t>(smem);
  auto dma = [&](const uint4* pack, int hb, unsigned char* s_w) __attribute__((always_inline)) {
    const uint4* src = pack + (size_t)hb * (NF3 * 64) + lane;
#pragma unroll
    for (int r = 0; r < BR3; ++r) {
      const int f = min(wave + 4 * r, NF3 - 1);     // 42 = 4 x 10 + 2: in the last round waves 2 and 3 repeat wave 1's (the same bytes; no branch)
      const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(s_w - smem) + f * FRAG);
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(src + f * 64), "s"(dst) : "memory");
    }
  };
  // MLP_DGRAD: this wave's d tile of hidden block hb -> its buffer `buf`, in accumulator layout: instruction q moves, for every lane, the
  // four hidden units 8 q + 4 hh .. + 3 of its pixel (the accumulator's registers 4 q .. 4 q + 3) to byte q * 1024 + 16 lane.  Only this
  // wave reads the tile; like dma() it is complete after the next wait_barrier().
  auto dma_d = [&](int hb, int buf) __attribute__((always_inline)) {
    const float* src = aux_in + aoff + hb * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(MLP3_LDS + (wave * 2 + buf) * MLP3_DTILE + q * FRAG));
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(src + 8 * q), "s"(dst) : "memory");
    }
  };
  // every load and LDS operation of this wave has completed (the weight fragments it moved have landed), then the barrier
  auto wait_barrier = [&]() __attribute__((always_inline)) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

  // One scheduling region per MFMA step (six products on one pair of fragments): the step's MFMAs, the LDS reads of the NEXT step's
  // weight fragments, and one slice of the activation's VALU work.  (Left to itself the scheduler hoists the fragment reads of a whole
  // unrolled GEMM and spills.)
  f16v acc2[NB3];
#pragma unroll
  for (int n = 0; n < NB3; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[n][r] = 0.f;
  auto read_w = [&](const unsigned char* s_w, int f, uint4 (&wf)[3]) __attribute__((always_inline)) {
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) wf[pc] = *reinterpret_cast<const uint4*>(s_w + lane * 16 + (f * 3 + pc) * FRAG);
  };
  // bias + GELU on the first GEMM's accumulator (register r: hidden unit hb * 32 + (r & 3) + 8 (r >> 2) + 4 hh of pixel lane & 31) and
  // the split into the second GEMM's A fragments (registers 8 j .. 8 j + 7 are step j), in 21 slices: 0..10 and 14..18 one GELU each,
  // 11, 12 the fragments of step 0, 19, 20 those of step 1 -- fourteen slices beside the first GEMM of the next block, seven beside
  // step 0 of the second GEMM
  // MLP_TRAIN / MLP_DGRAD: the quads of hv (h, or gpre) are stored from slices 14, 15, 16 and 19, behind the mid-block barrier; d's quad
  // q when its last value exists (slices 3, 7, 14, 18); MLP_DGRAD reads quad q of the d tile in the slice of its first register
  float hv[16];
  float dv[4];
  uint4 hf[2][3];
  int dbuf = 0;                                      // MLP_DGRAD: the buffer that holds the d tile of the block the slices work on
  auto store_quad = [&](float* __restrict__ out, int hb, int q, const float* v) __attribute__((always_inline)) {
    if (row_ok) *reinterpret_cast<float4*>(out + aoff + hb * 32 + 8 * q) = make_float4(v[0], v[1], v[2], v[3]);
  };
  auto slice = [&](const f16v& acc, int hb, int i) __attribute__((always_inline)) {
    const int r = i < 11 ? i : i - 3;
    if (i < 11 || (i >= 14 && i < 19)) {
      if (MODE == MLP_DGRAD) {
        if ((r & 3) == 0) {
          const float4 dq = *reinterpret_cast<const float4*>(s_d + dbuf * MLP3_DTILE + (r >> 2) * FRAG);
          dv[0] = dq.x; dv[1] = dq.y; dv[2] = dq.z; dv[3] = dq.w;
        }
        hv[r] = acc[r] * dv[r & 3];
      } else {
        const float v = acc[r] + s_b1[hb * 32 + 8 * (r >> 2) + 4 * hh + (r & 3)];
        if (MODE == MLP_TRAIN) {                     // gelu_erf's arithmetic for h, gelu_pair_kernel's for d
          const float er = 1.f + erf_poly(v * 0.70710678118654752440f);
          const float pdf = __expf(-0.5f * v * v) * 0.3989422804014327f;
          hv[r] = (v * 0.5f) * er;
          dv[r & 3] = fmaf(v, pdf, 0.5f * er);
          asm volatile("" : "+v"(dv[r & 3]));
        } else {
          hv[r] = gelu_erf(v);
        }
      }
      asm volatile("" : "+v"(hv[r]));              // computed HERE, beside this step's MFMAs (else it sinks to its first use)
      if (MODE == MLP_TRAIN && (r & 3) == 3) store_quad(out_b, hb, r >> 2, dv);
    }
    if (MODE != MLP_FWD && (i == 14 || i == 15 || i == 16 || i == 19)) {
      const int q = i == 19 ? 3 : i - 14;
      store_quad(out_a, hb, q, hv + 4 * q);
    }
    if (i == 11 || i == 12 || i == 19 || i == 20) {
      const int j = i >= 19, q0 = (i == 12 || i == 20) ? 2 : 0;
      unsigned p[3][2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        split2(hv[8 * j + 2 * (q0 + q)], hv[8 * j + 2 * (q0 + q) + 1], p[0][q], p[1][q], p[2][q]);
        asm volatile("" : "+v"(p[0][q]), "+v"(p[1][q]), "+v"(p[2][q]));
      }
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) {
        if (q0 == 0) { hf[j][pc].x = p[pc][0]; hf[j][pc].y = p[pc][1]; }
        else { hf[j][pc].z = p[pc][0]; hf[j][pc].w = p[pc][1]; }
      }
    }
  };
  // first GEMM, transposed: h^T (32 hidden x 32 pixels) = W1 block . x^T, with slices 0..13 of block hb's activation when `act`
  auto gemm1 = [&](f16v& acc, const f16v& prev, int hb, auto act) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    uint4 wf[2][3];
    read_w(s_w1, 0, wf[0]);
#pragma unroll
    for (int ks = 0; ks < KS3; ++ks) {
      if (ks + 1 < KS3) read_w(s_w1, ks + 1, wf[(ks + 1) & 1]);
#pragma unroll
      for (int t = 6 - NP; t < 6; ++t)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, wf[ks & 1][cm::kPieceA[t]]), __builtin_bit_cast(bf8, xf[ks][cm::kPieceB[t]]), acc, 0, 0, 0);
      if (decltype(act)::value) slice(prev, hb, ks);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // second GEMM: out (32 pixels x 224) += h (A operand, straight from the registers) . W2 block, with slices 14..20 beside step 0
  auto gemm2 = [&](const f16v& prev, int hb) __attribute__((always_inline)) {
    uint4 wf[2][3];
    read_w(s_w2, 0, wf[0]);
#pragma unroll
    for (int i = 0; i < 2 * NB3; ++i) {
      const int j = i / NB3, n = i - j * NB3;
      if (i + 1 < 2 * NB3) read_w(s_w2, ((i + 1) % NB3) * 2 + (i + 1) / NB3, wf[(i + 1) & 1]);
#pragma unroll
      for (int t = 6 - NP; t < 6; ++t)
        acc2[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, hf[j][cm::kPieceA[t]]), __builtin_bit_cast(bf8, wf[i & 1][cm::kPieceB[t]]), acc2[n], 0, 0, 0);
      if (j == 0) slice(prev, hb, 14 + n);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  float bv[NB3];         // what the store adds (b2, or nothing to a partial), fetched first (dd_store_tile.h)
#pragma unroll
  for (int n = 0; n < NB3; ++n) bv[n] = tile_bias(bias, n * 32 + (lane & 31), C3, pack2);

  // prologue: W1 of the first block, its first GEMM, then W1 of the second block in place and W2 of the first one on its way
  f16v acc1;
  dma(pack1, hb0, s_w1);
  if (MODE == MLP_DGRAD) dma_d(hb0, 0);
  wait_barrier();                                  // (b1 is in place too)
  gemm1(acc1, acc1, hb0, std::false_type{});
  wait_barrier();                                  // every wave has read W1 of the first block
  dma(pack1, min(hb0 + 1, hb1 - 1), s_w1);
  wait_barrier();
  dma(pack2, hb0, s_w2);
  // here, for every hb: acc1 = the pre-activation of block hb less its bias, s_w1 = W1 of block hb + 1, W2 of block hb on its way to s_w2
  auto block = [&](int hb, auto more) __attribute__((always_inline)) {
    f16v accn;
    dbuf = (hb - hb0) & 1;
    if (decltype(more)::value) gemm1(accn, acc1, hb, std::true_type{});        // block hb + 1, beside the VALU work of block hb
    else {
#pragma unroll
      for (int i = 0; i < KS3; ++i) slice(acc1, hb, i);
    }
    wait_barrier();                                // W2 of block hb is in place, every wave has read s_w1
    if (decltype(more)::value) dma(pack1, min(hb + 2, hb1 - 1), s_w1);
    if (MODE == MLP_DGRAD && decltype(more)::value) dma_d(hb + 1, dbuf ^ 1);   // the other buffer: slices 14..18 still read this one
    gemm2(acc1, hb);
    if (decltype(more)::value) {
      wait_barrier();                              // W1 of block hb + 2 is in place, every wave has read s_w2
      dma(pack2, hb + 1, s_w2);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[r] = accn[r];
    }
  };
  for (int hb = hb0; hb < hb1 - 1; ++hb) block(hb, std::true_type{});
  block(hb1 - 1, std::false_type{});

  float* const out = dst + (size_t)split * M * C3;
  auto tail = [&](auto full) __attribute__((always_inline)) {
    const int row = row0 + 4 * hh;
#pragma unroll
    for (int n = 0; n < NB3; ++n)
      store_acc32<decltype(full)::value>(acc2[n], bv[n], out + (size_t)row * C3 + n * 32 + (lane & 31), (size_t)C3, M - row, StoreF32{});
  };
  if ((int)blockIdx.x * 128 + 128 <= M) tail(std::true_type{});
  else tail(std::false_type{});
}

// y = b2 + partial 0 + partial 1 + ... in that order, four channels per thread (224 = 56 quads per row); the data gradient has no b2
__global__ __launch_bounds__(256) void mlp_fold224_kernel(const float4* __restrict__ partial, const float4* __restrict__ b2, int S, size_t quads, float4* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= quads) return;
  float4 a = b2 ? b2[i % (C3 / 4)] : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < S; ++s) {
    const float4 p = partial[(size_t)s * quads + i];
    a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
  }
  y[i] = a;
}

// S from the row count: 128 rows per workgroup, one workgroup per CU (LDS and registers), and not more workgroups than the 256 CUs:
// a second round doubles the time (the 528-on-512 note of dd_linear_wgrad.hip)
static int mlp224_splits(int M) {
  const int groups = (M + 127) / 128, n = 256 / groups;
  return n < 1 ? 1 : n > NHB3 ? NHB3 : n;
}

// MLP_FWD / MLP_TRAIN: y = the block's output (out_a = h, out_b = d for MLP_TRAIN).  MLP_DGRAD: x = g, aux_in = d, pack1 = W2^T, pack2 =
// W1^T fused, b1 = b2 = nullptr, y = dx, out_a = gpre.
template <int NP, int MODE>
static int launch_fused224(const float* x, const void* pack1, const void* pack2, const float* b1, const float* b2, int M, int S, float* y, float* partial,
                           hipStream_t stream, const float* aux_in = nullptr, float* out_a = nullptr, float* out_b = nullptr) {
  constexpr int lds = MLP3_LDS + (MODE == MLP_DGRAD ? 4 * 2 * MLP3_DTILE : 0);      // two d tiles per wave
  auto kern = mlp_fwd224_kernel<NP, MODE>;
  static dd::LdsAttrOnce lds_attr;          // per instantiation and device (dd_attr.h)
  if (const int rc = lds_attr.ensure(reinterpret_cast<const void*>(kern), lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((M + 127) / 128, S), dim3(256), lds, stream, x, static_cast<const uint4*>(pack1), static_cast<const uint4*>(pack2), b1,
                     S == 1 ? b2 : nullptr, M, S, S == 1 ? y : partial, aux_in, out_a, out_b);
  if (S == 1) return (int)hipGetLastError();
  const size_t quads = (size_t)M * (C3 / 4);
  hipLaunchKernelGGL(mlp_fold224_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const float4*>(partial),
                     reinterpret_cast<const float4*>(b2), S, quads, reinterpret_cast<float4*>(y));
  return (int)hipGetLastError();
}

// backward of the activation between the two Linears, one pass: post = GELU(pre) (the second Linear's weight gradient wants the
// activated tensor, which the forward never wrote) and g <- g * GELU'(pre) in place (cdf + x pdf, ATen's GeluBackwardCUDAKernelImpl formula on erf_poly)
__global__ __launch_bounds__(256) void gelu_pair_kernel(const float4* __restrict__ pre, float4* __restrict__ g, float4* __restrict__ post, size_t quads) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= quads) return;
  const float4 x4 = pre[i], g4 = g[i];
  const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, gv[4] = {g4.x, g4.y, g4.z, g4.w};
  float pv[4], dv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x = xv[e];
    const float er = 1.f + erf_poly(x * 0.70710678118654752440f);
    const float pdf = __expf(-0.5f * x * x) * 0.3989422804014327f;        // M_2_SQRTPI * M_SQRT1_2 * 0.5
    pv[e] = (x * 0.5f) * er;                                              // the forward's arithmetic, bit for bit
    dv[e] = gv[e] * fmaf(x, pdf, 0.5f * er);
  }
  post[i] = make_float4(pv[0], pv[1], pv[2], pv[3]);
  g[i] = make_float4(dv[0], dv[1], dv[2], dv[3]);
}

}  // namespace pw
}  // namespace dd

extern "C" size_t dd_pw_gemm_pack_bytes(int N, int K) { return (size_t)((N + 31) / 32) * (K / 16) * 3 * 1024; }

extern "C" int dd_mlp_pack(const float* w1, long long s1_n, long long s1_k, const float* w2, long long s2_n, long long s2_k, int C, int hidden, void* pack_fwd1,
                           void* pack_fwd2, void* pack_bwd2, void* pack_bwd1, void* pack_fwd2_fused, void* stream) {
  using namespace dd::pw;
  if (!w1 || !w2 || C < 1 || hidden < 1) return (int)hipErrorInvalidValue;
  PackArgs a;
  a.count = 0;
  a.total = 0;
  bool bad = false;
  auto add = [&](const float* w, long long s_n, long long s_k, int N, int K, void* out, int fused = 0) {
    if (!out) return;
    if (K < 16 || K % 16 || (fused && K % 32)) { bad = true; return; }        // the contraction goes in steps of sixteen
    PackRegion& r = a.r[a.count++];
    r.w = w; r.s_n = s_n; r.s_k = s_k; r.N = N; r.K = K; r.first = a.total; r.fused = fused; r.out = static_cast<uint4*>(out);
    a.total += ((N + 31) / 32) * (K / 16);
  };
  add(w1, s1_n, s1_k, hidden, C, pack_fwd1);           // pre  = y . W1^T          W1 (hidden, C)
  add(w2, s2_n, s2_k, C, hidden, pack_fwd2);           // out  = act(pre) . W2^T   W2 (C, hidden)
  add(w2, s2_k, s2_n, hidden, C, pack_bwd2);           // g_post = g . W2          "weight" (n = hidden, k = C) = W2^T
  add(w1, s1_k, s1_n, C, hidden, pack_bwd1);           // g_y  = g_pre . W1        "weight" (n = C, k = hidden) = W1^T
  add(w2, s2_n, s2_k, C, hidden, pack_fwd2_fused, 1);  // dd_mlp_fwd's second operand: W2 by hidden block, k in accumulator-register order
  if (a.count == 0 || bad) return (int)hipErrorInvalidValue;
  for (int i = a.count; i < MAX_REGIONS; ++i) a.r[i] = a.r[0];
  hipLaunchKernelGGL(pw_pack_kernel, dim3((a.total * 64 + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

// ---- the training pass of the block: forward that saves h and d, fused data gradient (C = 224: stage 3; C = 64 / 128: stages 1, 2) ----
static bool mlp_narrow(int C) { return C == 64 || C == 128; }

// the four operands of a training block in one launch; each entry point names the widths it takes
static int mlp_train_pack(bool width_ok, const float* w1, long long s1_n, long long s1_k, const float* w2, long long s2_n, long long s2_k, int C, int hidden,
                          void* pack_fwd1, void* pack_fwd2_fused, void* pack_bwd2, void* pack_bwd1_fused, void* stream) {
  using namespace dd::pw;
  if (!w1 || !w2 || !width_ok || hidden != 6 * C || !pack_fwd1 || !pack_fwd2_fused || !pack_bwd2 || !pack_bwd1_fused) return (int)hipErrorInvalidValue;
  PackArgs a;
  a.count = 0;
  a.total = 0;
  auto add = [&](const float* w, long long s_n, long long s_k, int N, int K, void* out, int fused) {
    PackRegion& r = a.r[a.count++];
    r.w = w; r.s_n = s_n; r.s_k = s_k; r.N = N; r.K = K; r.first = a.total; r.fused = fused; r.out = static_cast<uint4*>(out);
    a.total += ((N + 31) / 32) * (K / 16);
  };
  add(w1, s1_n, s1_k, hidden, C, pack_fwd1, 0);        // pre = x . W1^T: first operand of the forward
  add(w2, s2_n, s2_k, C, hidden, pack_fwd2_fused, 1);  // W2 by hidden block, k in accumulator-register order
  add(w2, s2_k, s2_n, hidden, C, pack_bwd2, 0);        // g . W2: W2^T (n = hidden, k = C) as the data gradient's first operand
  add(w1, s1_k, s1_n, C, hidden, pack_bwd1_fused, 1);  // . W1: W1^T (n = C, k = hidden) by hidden block, fused-k order
  for (int i = a.count; i < MAX_REGIONS; ++i) a.r[i] = a.r[0];
  hipLaunchKernelGGL(pw_pack_kernel, dim3((a.total * 64 + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return (int)hipGetLastError();
}

extern "C" int dd_mlp_train_pack(const float* w1, long long s1_n, long long s1_k, const float* w2, long long s2_n, long long s2_k, int C, int hidden,
                                 void* pack_fwd1, void* pack_fwd2_fused, void* pack_bwd2, void* pack_bwd1_fused, void* stream) {
  return mlp_train_pack(C == dd::pw::C3, w1, s1_n, s1_k, w2, s2_n, s2_k, C, hidden, pack_fwd1, pack_fwd2_fused, pack_bwd2, pack_bwd1_fused, stream);
}

extern "C" int dd_mlp_train_pack_narrow(const float* w1, long long s1_n, long long s1_k, const float* w2, long long s2_n, long long s2_k, int C, int hidden,
                                        void* pack_fwd1, void* pack_fwd2_fused, void* pack_bwd2, void* pack_bwd1_fused, void* stream) {
  return mlp_train_pack(mlp_narrow(C), w1, s1_n, s1_k, w2, s2_n, s2_k, C, hidden, pack_fwd1, pack_fwd2_fused, pack_bwd2, pack_bwd1_fused, stream);
}

extern "C" size_t dd_mlp_train_bwd_workspace_bytes(int M, int C, int splits) {
  if (M < 1 || C != dd::pw::C3 || splits < 0 || splits > dd::pw::NHB3) return 0;
  const int S = splits ? splits : dd::pw::mlp224_splits(M);
  return S > 1 ? (size_t)S * M * C * sizeof(float) : 0;
}

// what both training entry points refuse: another width, rows whose (M, 6C) tensors pass 2^32 bytes (the kernels' 32-bit offsets),
// more splits than hidden blocks (C = 64 / 128: any split, the hidden range stays whole there), an unknown product count
static bool mlp_train_shape_ok(int M, int C, int products, int splits) {
  if (products != 6 && products != 3 && products != 1) return false;
  if (mlp_narrow(C)) return M >= 1 && (long long)M * (6 * C) < (1ll << 30) && splits >= 0 && splits <= 1;
  return C == dd::pw::C3 && M >= 1 && M <= (1 << 19) && splits >= 0 && splits <= dd::pw::NHB3;
}

static bool aligned16(std::initializer_list<const void*> ps) {
  unsigned long long bits = 0;
  for (const void* p : ps) bits |= reinterpret_cast<unsigned long long>(p);
  return (bits & 15ull) == 0;
}

extern "C" int dd_mlp_train_fwd(const float* x, const void* pack_fwd1, const void* pack_fwd2_fused, const float* b1, const float* b2, int M, int C,
                                int products, int splits, float* y, float* h, float* d, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace dd::pw;
  if (!x || !pack_fwd1 || !pack_fwd2_fused || !b1 || !b2 || !y || !h || !d || !mlp_train_shape_ok(M, C, products, splits)) return (int)hipErrorInvalidValue;
  if (!aligned16({x, y, h, d, b2, workspace, pack_fwd1, pack_fwd2_fused})) return (int)hipErrorInvalidValue;
  if (C == 64) return launch_fused_n<64, MLP_TRAIN>(products, x, pack_fwd1, pack_fwd2_fused, b1, b2, M, y, static_cast<hipStream_t>(stream), nullptr, h, d);
  if (C == 128) return launch_fused_n<128, MLP_TRAIN>(products, x, pack_fwd1, pack_fwd2_fused, b1, b2, M, y, static_cast<hipStream_t>(stream), nullptr, h, d);
  const int S = splits ? splits : mlp224_splits(M);
  if (S > 1 && (!workspace || workspace_bytes < dd_mlp_fwd_workspace_bytes(M, C, S))) return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  return products == 6 ? launch_fused224<6, MLP_TRAIN>(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, S, y, part, s, nullptr, h, d)
       : products == 3 ? launch_fused224<3, MLP_TRAIN>(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, S, y, part, s, nullptr, h, d)
                       : launch_fused224<1, MLP_TRAIN>(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, S, y, part, s, nullptr, h, d);
}

extern "C" int dd_mlp_train_bwd(const float* g, const float* d, const void* pack_bwd2, const void* pack_bwd1_fused, int M, int C, int products, int splits,
                                float* dx, float* gpre, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace dd::pw;
  if (!g || !d || !pack_bwd2 || !pack_bwd1_fused || !dx || !gpre || !mlp_train_shape_ok(M, C, products, splits)) return (int)hipErrorInvalidValue;
  if (!aligned16({g, d, dx, gpre, workspace, pack_bwd2, pack_bwd1_fused})) return (int)hipErrorInvalidValue;
  if (C == 64) return launch_fused_n<64, MLP_DGRAD>(products, g, pack_bwd2, pack_bwd1_fused, nullptr, nullptr, M, dx, static_cast<hipStream_t>(stream), d, gpre, nullptr);
  if (C == 128) return launch_fused_n<128, MLP_DGRAD>(products, g, pack_bwd2, pack_bwd1_fused, nullptr, nullptr, M, dx, static_cast<hipStream_t>(stream), d, gpre, nullptr);
  const int S = splits ? splits : mlp224_splits(M);
  if (S > 1 && (!workspace || workspace_bytes < dd_mlp_train_bwd_workspace_bytes(M, C, S))) return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  return products == 6 ? launch_fused224<6, MLP_DGRAD>(g, pack_bwd2, pack_bwd1_fused, nullptr, nullptr, M, S, dx, part, s, d, gpre, nullptr)
       : products == 3 ? launch_fused224<3, MLP_DGRAD>(g, pack_bwd2, pack_bwd1_fused, nullptr, nullptr, M, S, dx, part, s, d, gpre, nullptr)
                       : launch_fused224<1, MLP_DGRAD>(g, pack_bwd2, pack_bwd1_fused, nullptr, nullptr, M, S, dx, part, s, d, gpre, nullptr);
}

extern "C" int dd_mlp_fwd_supported(int C) { return (C == 64 || C == 128 || C == 224) ? 1 : 0; }

extern "C" int dd_mlp_fwd_splits(int M, int C) { return (C == dd::pw::C3 && M >= 1) ? dd::pw::mlp224_splits(M) : 1; }

extern "C" size_t dd_mlp_fwd_workspace_bytes(int M, int C, int splits) {
  if (M < 1 || !dd_mlp_fwd_supported(C) || splits < 0 || splits > dd::pw::NHB3) return 0;
  const int S = splits ? splits : dd_mlp_fwd_splits(M, C);
  return (C == dd::pw::C3 && S > 1) ? (size_t)S * M * C * sizeof(float) : 0;
}

extern "C" int dd_mlp_fwd_n(const float* x, const void* pack_fwd1, const void* pack_fwd2_fused, const float* b1, const float* b2, int M, int C, int products,
                            int splits, float* y, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace dd::pw;
  if (C != C3) return (products == 6 && splits <= 1) ? dd_mlp_fwd(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, C, y, stream) : (int)hipErrorInvalidValue;
  if (!x || !pack_fwd1 || !pack_fwd2_fused || !b1 || !b2 || !y || M < 1 || splits < 0 || splits > NHB3) return (int)hipErrorInvalidValue;
  if (products != 6 && products != 3 && products != 1) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<unsigned long long>(x) | reinterpret_cast<unsigned long long>(y) | reinterpret_cast<unsigned long long>(b2) |
       reinterpret_cast<unsigned long long>(workspace)) & 15ull)
    return (int)hipErrorInvalidValue;
  const int S = splits ? splits : mlp224_splits(M);
  if (S > 1 && (!workspace || workspace_bytes < dd_mlp_fwd_workspace_bytes(M, C, S))) return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  return products == 6 ? launch_fused224<6, MLP_FWD>(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, S, y, part, s)
       : products == 3 ? launch_fused224<3, MLP_FWD>(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, S, y, part, s)
                       : launch_fused224<1, MLP_FWD>(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, S, y, part, s);
}

extern "C" int dd_mlp_fwd(const float* x, const void* pack_fwd1, const void* pack_fwd2_fused, const float* b1, const float* b2, int M, int C, float* y, void* stream) {
  if (!x || !pack_fwd1 || !pack_fwd2_fused || !b1 || !b2 || !y || M < 1 || (reinterpret_cast<unsigned long long>(x) & 15ull)) return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (C) {
    case 64: return dd::pw::launch_fused<64, 6, dd::pw::MLP_FWD>(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, y, s);
    case 128: return dd::pw::launch_fused<128, 6, dd::pw::MLP_FWD>(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, y, s);
    case 224: return dd::pw::launch_fused224<6, dd::pw::MLP_FWD>(x, pack_fwd1, pack_fwd2_fused, b1, b2, M, 1, y, nullptr, s);      // unsplit: dd_mlp_fwd_n fills the chip
    default: return (int)hipErrorInvalidValue;
  }
}

extern "C" int dd_gelu_pair(const float* pre, float* g_inout, float* post, size_t n, void* stream) {
  if (!pre || !g_inout || !post || n == 0 || (n & 3)) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<unsigned long long>(pre) | reinterpret_cast<unsigned long long>(g_inout) | reinterpret_cast<unsigned long long>(post)) & 15ull)
    return (int)hipErrorInvalidValue;
  const size_t quads = n >> 2;
  hipLaunchKernelGGL(dd::pw::gelu_pair_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(pre), reinterpret_cast<float4*>(g_inout), reinterpret_cast<float4*>(post), quads);
  return (int)hipGetLastError();
}

extern "C" int dd_pw_gemm(const float* x, const void* pack, const float* bias, int M, int K, int N, int gelu_in, float* y, void* stream) {
  using namespace dd::pw;
  if (!x || !pack || !y || M < 1 || K < 32 || K % 32 || N < 1) return (int)hipErrorInvalidValue;       // chunks of 32
  if ((reinterpret_cast<unsigned long long>(x) & 15ull) || (size_t)M * K >= (1ull << 40) || (size_t)M * N >= (1ull << 40)) return (int)hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return gelu_in ? dd::pw::dispatch<true>(x, pack, bias, M, K, N, y, s) : dd::pw::dispatch<false>(x, pack, bias, M, K, N, y, s);
}
