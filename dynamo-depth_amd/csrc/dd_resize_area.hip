// dd_resize_area.hip -- the area-weighted down-sample of the nuScenes / Waymo preparation (reference prepare_data/nuScenes.py:151-152,
// cv2.resize(..., interpolation=INTER_AREA)) for any down-scale, integer or not.  The definition (hipops/resize.py
// resize_area_host), per axis with scale = S / D: destination d covers [d scale, (d + 1) scale); the source pixels it overlaps are
// weighted by the covered length over cell = min(scale, S - d scale), a partial pixel only where its length exceeds 1e-3
// (OpenCV's computeResizeAreaTab, public source).  The tables (first source index, tap count, fp32 weights padded with zeros to a
// common tap count) are built on the host; the result is the separable weighted sum, columns first, then rows, in fp32 with one
// fused multiply-add per tap in ascending tap order, rounded half to even and saturated.
// One workgroup makes RA_TR destination rows of a strip of at most RA_CW destination columns.  It walks the source rows the tile
// covers once: each row's strip is staged through LDS with 16-byte loads from the 16-byte boundary below its first byte (the
// bytes of a tail chunk that would cross the end of the batch are read one by one), two buffers and one barrier per row, the
// next row's loads in flight under the current row's arithmetic.  Every thread keeps RA_EPT destination bytes of the row being
// summed in registers; a source row that two destination rows share is used for both.  No atomics; every branch is on table values,
// the same in all lanes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dynamo_hip.h"

namespace dd {

constexpr int RA_NT = 256;
constexpr int RA_TR = 8;                              // destination rows per workgroup (1600x900 -> 512x288: 25 source rows, no shared row)
constexpr int RA_CW = 512;                            // destination columns per workgroup at most
constexpr int RA_EPT = RA_CW * 3 / RA_NT;             // destination bytes per thread and row
constexpr int RA_ROW_BYTES = 16384;                   // LDS per staged source row
constexpr int RA_STG = RA_ROW_BYTES / 16 / RA_NT;     // 16-byte chunks per thread and row
constexpr int RA_W_FLOATS = 4096;                     // staged column weights

struct RAShape {
  int Hs, Ws, Hd, Wd, hk, vk, cw;
  long long total;                                    // bytes of src
};

struct RAStage {
  uint4 v[RA_STG];
  int shift;                                          // bytes between the 16-byte boundary the chunks start at and the strip's first byte
};

__device__ __forceinline__ void ra_load(const unsigned char* __restrict__ src, long long total, long long first, int nbytes, int t, RAStage& st) {
  const unsigned char* a = src + first;
  st.shift = (int)(reinterpret_cast<uintptr_t>(a) & 15u);
  const long long base = first - st.shift;            // >= 0: src is 16-byte aligned
  const int nch = (st.shift + nbytes + 15) >> 4;
#pragma unroll
  for (int q = 0; q < RA_STG; ++q) {
    const int ch = t + q * RA_NT;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (ch < nch) {
      const long long o = base + (long long)ch * 16;
      if (o + 16 <= total) {
        v = *reinterpret_cast<const uint4*>(src + o);
      } else {                                        // the chunk that crosses the end of the batch
        unsigned w[4] = {0u, 0u, 0u, 0u};
        for (int b = 0; b < 16; ++b)
          if (o + b < total) w[b >> 2] |= (unsigned)src[o + b] << (8 * (b & 3));
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    st.v[q] = v;
  }
}

__device__ __forceinline__ void ra_store_lds(unsigned char* buf, int nbytes, int t, const RAStage& st) {
  const int nch = (st.shift + nbytes + 15) >> 4;
#pragma unroll
  for (int q = 0; q < RA_STG; ++q) {
    const int ch = t + q * RA_NT;
    if (ch < nch) *reinterpret_cast<uint4*>(buf + ch * 16) = st.v[q];
  }
}

__device__ __forceinline__ unsigned char ra_u8(float a) {
  return (unsigned char)fminf(fmaxf(rintf(a), 0.f), 255.f);
}

__global__ __launch_bounds__(RA_NT) void resize_area_kernel(const unsigned char* __restrict__ src, RAShape g, const int* __restrict__ hstart,
                                                            const int* __restrict__ hcount, const float* __restrict__ hw,
                                                            const int* __restrict__ vstart, const int* __restrict__ vcount,
                                                            const float* __restrict__ vw, unsigned char* __restrict__ dst) {
  __shared__ __align__(16) unsigned char rowbuf[2][RA_ROW_BYTES];
  __shared__ float sw[RA_W_FLOATS];
  const int t = threadIdx.x, img = blockIdx.z;
  const int c0 = blockIdx.x * g.cw, c1 = min(c0 + g.cw, g.Wd), nE = (c1 - c0) * 3;
  const int r0 = blockIdx.y * RA_TR, r1 = min(r0 + RA_TR, g.Hd);
  const int pad = 3 * g.hk + 3;                       // a padded tap may look this far past the strip: zero weight, any byte
  const int s0 = min(max(hstart[c0], 0), g.Ws - 1);
  const int s1 = min(max(hstart[c1 - 1] + hcount[c1 - 1], s0 + 1), g.Ws);
  const int nbytes = min((s1 - s0) * 3, RA_ROW_BYTES - 16 - pad);

  for (int i = t; i < (c1 - c0) * g.hk; i += RA_NT) sw[i] = hw[(size_t)c0 * g.hk + i];
  int eoff[RA_EPT], wb[RA_EPT];
#pragma unroll
  for (int j = 0; j < RA_EPT; ++j) {
    const int e = t + j * RA_NT, x = e / 3;
    const bool live = e < nE;
    eoff[j] = live ? min(max((hstart[c0 + x] - s0) * 3, 0), nbytes - 3) + (e - 3 * x) : 0;
    wb[j] = live ? x * g.hk : 0;
  }

  const int sy0 = min(max(vstart[r0], 0), g.Hs - 1);
  const int sy1 = min(max(vstart[r1 - 1] + vcount[r1 - 1], sy0 + 1), g.Hs);
  const long long row_bytes = (long long)g.Ws * 3;
  const long long first0 = ((long long)img * g.Hs + sy0) * row_bytes + (long long)s0 * 3;
  float acc[RA_EPT];
#pragma unroll
  for (int j = 0; j < RA_EPT; ++j) acc[j] = 0.f;
  int d = r0;
  RAStage st;
  ra_load(src, g.total, first0, nbytes, t, st);
  for (int sy = sy0; sy < sy1; ++sy) {
    unsigned char* buf = rowbuf[(sy - sy0) & 1];
    const int shift = st.shift;
    ra_store_lds(buf, nbytes, t, st);
    __syncthreads();                                  // the other buffer was last read before the previous barrier
    if (sy + 1 < sy1) ra_load(src, g.total, first0 + (long long)(sy + 1 - sy0) * row_bytes, nbytes, t, st);
    float h[RA_EPT];
#pragma unroll
    for (int j = 0; j < RA_EPT; ++j) {
      const unsigned char* p = buf + shift + eoff[j];
      const float* w = sw + wb[j];
      float a = 0.f;
      for (int k = 0; k < g.hk; ++k) a = fmaf(w[k], (float)p[3 * k], a);
      h[j] = a;
    }
    while (d < r1) {                                  // the destination rows this source row belongs to: one, or two at a shared row
      const int k = sy - vstart[d], cnt = min(vcount[d], g.vk);
      if (k < 0 || k >= cnt) break;
      const float wv = vw[(size_t)d * g.vk + k];
#pragma unroll
      for (int j = 0; j < RA_EPT; ++j) acc[j] = fmaf(wv, h[j], acc[j]);
      if (k != cnt - 1) break;
      unsigned char* o = dst + (((size_t)img * g.Hd + d) * g.Wd + c0) * 3;
#pragma unroll
      for (int j = 0; j < RA_EPT; ++j) {
        const int e = t + j * RA_NT;
        if (e < nE) o[e] = ra_u8(acc[j]);
        acc[j] = 0.f;
      }
      ++d;
    }
  }
}

// destination columns per workgroup: the strip's source bytes, the alignment shift and the padded taps fit one LDS row buffer
static int ra_strip(int Ws, int Wd, int hk) {
  const double scale = (double)Ws / (double)Wd;
  const long long px = (RA_ROW_BYTES - 16 - (3 * hk + 3) - 15) / 3 - 2;
  long long cw = (long long)((double)px / scale) - 1;
  if (cw > RA_CW) cw = RA_CW;
  if (cw > RA_W_FLOATS / hk) cw = RA_W_FLOATS / hk;
  return (int)cw;
}

}  // namespace dd

extern "C" int dd_resize_area(const unsigned char* src, int n_images, int Hs, int Ws, unsigned char* dst, int Hd, int Wd, const int32_t* h_start,
                              const int32_t* h_count, const float* h_weight, int h_taps, const int32_t* v_start, const int32_t* v_count,
                              const float* v_weight, int v_taps, void* stream) {
  using namespace dd;
  if (!src || !dst || !h_start || !h_count || !h_weight || !v_start || !v_count || !v_weight) return (int)hipErrorInvalidValue;
  if (n_images < 1 || n_images > 65535 || Hd < 1 || Wd < 1 || Hs < Hd || Ws < Wd || h_taps < 1 || v_taps < 1 || h_taps > 1024)
    return (int)hipErrorInvalidValue;
  if ((long long)Hs * Ws > 2147483647ll / 3 || (reinterpret_cast<uintptr_t>(src) & 15u)) return (int)hipErrorInvalidValue;
  RAShape g;
  g.Hs = Hs, g.Ws = Ws, g.Hd = Hd, g.Wd = Wd, g.hk = h_taps, g.vk = v_taps;
  g.cw = ra_strip(Ws, Wd, h_taps);
  g.total = (long long)n_images * Hs * Ws * 3;
  if (g.cw < 1) return (int)hipErrorInvalidValue;
  const int tiles = (Hd + RA_TR - 1) / RA_TR;
  if (tiles > 65535) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(resize_area_kernel, dim3((Wd + g.cw - 1) / g.cw, tiles, n_images), dim3(RA_NT), 0, static_cast<hipStream_t>(stream), src, g,
                     h_start, h_count, h_weight, v_start, v_count, v_weight, dst);
  return (int)hipGetLastError();
}
