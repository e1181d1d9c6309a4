// dd_store_tile.h -- the output store of one 32x32 MFMA accumulator, shared by dd_conv_mfma.hip, dd_pw_gemm.hip and dd_conv_half.hip.
// C layout of v_mfma_f32_32x32x16_*: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) in register r.  Here the column
// is the output channel (contiguous in memory) and the row a pixel / GEMM row, `pitch` elements apart.
//
// Why a helper: on gfx9 stores count in vmcnt like loads, in order.  A load whose first use sits inside conditionally executed store
// blocks (`bias ? bias[co] : 0.f` in the epilogue, used under `if (X < Wo)`) makes the compiler put a full s_waitcnt vmcnt(0) in EVERY
// such block -- it cannot carry "already waited" across the joins -- and each store of the tail then waits for the previous store's
// acknowledgement: 32-96 dependent round trips to L2 per wave.  So: everything the epilogue adds is loaded BEFORE the main loop
// (tile_bias: unconditional, the loop's first counted wait covers it), and a full tile -- a wave-uniform test -- takes the
// straight-line path (FULL) below; only edge tiles keep the per-store bounds checks.  Private to csrc/.
#pragma once

#include <hip/hip_runtime.h>

#include "dd_split.h"

namespace dd {
namespace cm {

// The bias of this lane's output channel `co` (0 without a bias or beyond n_out), to be called BEFORE the main loop.  One
// unconditional load: without a bias (or a column) it reads `valid`, any mapped 4-byte-aligned address, and drops the value.
__device__ __forceinline__ float tile_bias(const float* __restrict__ bias, int co, int n_out, const void* valid) {
  const bool has = bias != nullptr && co < n_out;
  const float v = *(has ? bias + co : static_cast<const float*>(valid));
  return has ? v : 0.f;
}

struct StoreF32 {
  typedef float type;
  __device__ __forceinline__ float operator()(float v) const { return v; }
};

// p: the element of tile row 4 * (lane >> 5), this lane's column.  FULL: all 32 rows and this column exist (sixteen stores, no
// test).  Otherwise rows_left = (rows of the tile that exist) - 4 * (lane >> 5), or <= 0 for a lane whose column does not exist.
template <bool FULL, typename Cvt>
__device__ __forceinline__ void store_acc32(const f16v& acc, float bv, typename Cvt::type* __restrict__ p, size_t pitch, int rows_left, Cvt cvt) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rr = (r & 3) + 8 * (r >> 2);
    if (FULL || rr < rows_left) p[rr * pitch] = cvt(acc[r] + bv);
  }
}

}  // namespace cm
}  // namespace dd
