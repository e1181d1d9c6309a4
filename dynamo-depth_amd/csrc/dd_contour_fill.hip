// Motion masks from per-object contour lists (reference datasets/waymo_dataset.py:109-118: cv2.drawContours(mask, contours, -1, label, -1)
// per object on the host, then a (B, 1280, 1920) upload).  The contours come from cv2.findContours(CHAIN_APPROX_SIMPLE): closed, integer
// vertices, every segment between consecutive vertices (and from the last back to the first) horizontal, vertical or a 45 degree
// diagonal.  For such input the fill has an exact integer definition, the one this kernel, hipops/contours.py fill_host and
// tests/contour_fill_case.py implement:
//   edge pixels of an object  every integer pixel on a segment of one of its contours (a one-vertex contour: that pixel)
//   interior                  even-odd over ALL contours of the object: a non-horizontal segment with end rows y0, y1 crosses the rows
//                             min(y0, y1) <= y < max(y0, y1) at its integer x on that row; (x, y) is inside when the number of
//                             crossings of row y at x' <= x is odd
//   covered                   interior or edge
//   mask                      the label of the LAST object in file order that covers the pixel, 0 where none does
// One wave per (sample, row).  The lanes read the sample's contour records 64 at a time and keep those whose row range holds the row;
// for each of them the lanes walk the vertices (one segment per lane and step) and toggle the crossing / set the edge bits of the row in
// two LDS bitmaps with 32-bit integer atomics.  When the object index changes, the crossings become coverage by a prefix xor (in-word
// by shifts, across words by a ballot of the word parities) and the object's label is blended into the row's bytes in LDS, 4 pixels per
// access.  The row leaves in 16-byte stores: every output byte is written once, by its one writer; integers only, so the bytes do not
// depend on the launch geometry.  Bitmaps and row bytes are indexed by q = x + (row base address & 15), which puts the 16-byte
// chunks of LDS and of global memory on the same boundaries whatever the alignment of the row.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

namespace dd {

constexpr int CF_NT = 64;           // one wave: the __syncthreads() below are wave-local
constexpr int CF_REC = 6;           // first vertex, vertex count, object index, label, first row, last row
constexpr int CF_MAX_SIZE = 32768;  // int16 vertices address 0 .. 32767

// LDS: cover/cross bitmap [nw] 64-bit words, edge bitmap [nw], row bytes [nw * 64]
__device__ __forceinline__ void cf_clear(unsigned long long* bits, int nw) {
  for (int i = threadIdx.x; i < 2 * nw; i += CF_NT) bits[i] = 0ull;
}

// crossings -> coverage, and the object's label into the covered bytes of the row
__device__ __forceinline__ void cf_paint(unsigned long long* cross, const unsigned long long* edge, unsigned* row32, int nw, unsigned label) {
  const int lane = threadIdx.x;
  __syncthreads();
  unsigned carry = 0u;
  for (int base = 0; base < nw; base += CF_NT) {
    const int w = base + lane;
    unsigned long long p = w < nw ? cross[w] : 0ull;
    p ^= p << 1, p ^= p << 2, p ^= p << 4, p ^= p << 8, p ^= p << 16, p ^= p << 32;          // bit i = parity of bits 0 .. i
    const unsigned long long odd = __ballot((p >> 63) != 0ull);
    const unsigned before = (__popcll(odd & ((1ull << lane) - 1ull)) & 1u) ^ carry;
    if (w < nw) cross[w] = (before ? ~p : p) | edge[w];
    carry ^= __popcll(odd) & 1u;
  }
  __syncthreads();
  const unsigned char* cover = reinterpret_cast<const unsigned char*>(cross);
  const unsigned lab4 = label * 0x01010101u;
  for (int g = lane; g < nw * 8; g += CF_NT) {                    // 8 pixels: one byte of the bitmap, two words of the row
    const unsigned c = cover[g];
    if (c == 0u) continue;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned n = (c >> (4 * k)) & 15u;
      const unsigned m = ((n & 1u) * 0xffu) | ((n & 2u) * (0xff00u >> 1)) | ((n & 4u) * (0xff0000u >> 2)) | ((n & 8u) * (0xff000000u >> 3));
      if (m != 0u) row32[2 * g + k] = (row32[2 * g + k] & ~m) | (lab4 & m);
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(CF_NT) void contour_fill_kernel(const unsigned* __restrict__ vertices, int v_cap, const int* __restrict__ contours,
                                                             int c_cap, int H, int W, uint8_t* __restrict__ mask) {
  extern __shared__ __align__(16) unsigned long long cf_lds[];
  const int lane = threadIdx.x, y = blockIdx.x, b = blockIdx.y;
  uint8_t* out = mask + ((size_t)b * H + y) * W;
  const int a = (int)((uintptr_t)out & 15u);
  const int nw = (W + a + 63) >> 6;
  unsigned long long* cross = cf_lds;
  unsigned long long* edge = cf_lds + nw;
  unsigned* cross32 = reinterpret_cast<unsigned*>(cross);
  unsigned* edge32 = reinterpret_cast<unsigned*>(edge);
  uint4* row128 = reinterpret_cast<uint4*>(cf_lds + 2 * nw);
  unsigned* row32 = reinterpret_cast<unsigned*>(row128);
  for (int i = lane; i < nw * 4; i += CF_NT) row128[i] = make_uint4(0u, 0u, 0u, 0u);
  cf_clear(cf_lds, nw);
  __syncthreads();

  const unsigned* vtx = vertices + (size_t)b * v_cap;
  const int* rec = contours + (size_t)b * c_cap * CF_REC;
  int cur_obj = -1;
  unsigned cur_label = 0u;
  bool more = true;
  for (int base = 0; base < c_cap && more; base += CF_NT) {
    int first = 0, count = 0, obj = 0, label = 0, ya = 0, yb = -1;
    if (base + lane < c_cap) {
      const int* r = rec + (size_t)(base + lane) * CF_REC;
      first = r[0], count = r[1], obj = r[2], label = r[3], ya = r[4], yb = r[5];
    }
    more = __ballot(count <= 0) == 0ull;                          // the used records come first: an unused slot ends the list
    const bool valid = count > 0 && first >= 0 && first <= v_cap - count;
    unsigned long long todo = __ballot(valid && ya <= y && y <= yb);
    while (todo != 0ull) {
      const int c = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const int c_first = __shfl(first, c), c_count = __shfl(count, c), c_obj = __shfl(obj, c), c_label = __shfl(label, c);
      if (c_obj != cur_obj) {
        if (cur_obj >= 0) {
          cf_paint(cross, edge, row32, nw, cur_label);
          cf_clear(cf_lds, nw);
          __syncthreads();
        }
        cur_obj = c_obj, cur_label = (unsigned)c_label & 255u;
      }
      for (int j = lane; j < c_count; j += CF_NT) {
        const unsigned v0 = vtx[c_first + j], v1 = vtx[c_first + (j + 1 == c_count ? 0 : j + 1)];
        const int x0 = (short)(v0 & 0xffffu), y0 = (short)(v0 >> 16), x1 = (short)(v1 & 0xffffu), y1 = (short)(v1 >> 16);
        if (y0 == y1) {
          if (y0 != y) continue;
          int lo = min(x0, x1), hi = max(x0, x1);                 // a horizontal run (or one pixel): edge only
          lo = max(lo, 0), hi = min(hi, W - 1);
          if (lo > hi) continue;
          lo += a, hi += a;
          for (int w = lo >> 5; w <= hi >> 5; ++w) {
            const unsigned from = w == (lo >> 5) ? (0xffffffffu << (lo & 31)) : 0xffffffffu;
            const unsigned to = w == (hi >> 5) ? (0xffffffffu >> (31 - (hi & 31))) : 0xffffffffu;
            atomicOr(&edge32[w], from & to);
          }
        } else {
          const int top = min(y0, y1), bottom = max(y0, y1);
          if (y < top || y > bottom) continue;
          const int t = abs(y - y0);
          const int x = x0 + (x1 > x0 ? t : (x1 < x0 ? -t : 0));
          if (x < 0 || x >= W) continue;
          const int q = x + a;
          atomicOr(&edge32[q >> 5], 1u << (q & 31));
          if (y < bottom) atomicXor(&cross32[q >> 5], 1u << (q & 31));
        }
      }
    }
  }
  if (cur_obj >= 0) cf_paint(cross, edge, row32, nw, cur_label);
  __syncthreads();

  // chunk k holds q = 16 k .. 16 k + 15, pixel x = q - a; out - a is 16-byte aligned
  uint8_t* aligned = out - a;
  const unsigned char* row8 = reinterpret_cast<const unsigned char*>(row128);
  const int end = W + a;
  for (int k = lane; k * 16 < end; k += CF_NT) {
    const int q0 = k * 16;
    if (q0 >= a && q0 + 16 <= end) {
      *reinterpret_cast<uint4*>(aligned + q0) = row128[k];
    } else {
      for (int q = max(q0, a); q < min(q0 + 16, end); ++q) aligned[q] = row8[q];
    }
  }
}

}  // namespace dd

using namespace dd;

extern "C" int dd_fill_contours(const int16_t* vertices, int v_cap, const int32_t* contours, int c_cap, int B, int H, int W, uint8_t* mask,
                                void* stream) {
  if (!vertices || !contours || !mask || v_cap < 1 || c_cap < 1 || B < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  if (H > CF_MAX_SIZE || W > CF_MAX_SIZE || B > 65535 || ((uintptr_t)vertices & 3u) || ((uintptr_t)contours & 3u)) return (int)hipErrorInvalidValue;
  const int nw = (W + 15 + 63) >> 6;                              // the widest case of the kernel's nw: 41 KB of LDS at W = 32768
  const size_t lds = (size_t)nw * (2 * sizeof(unsigned long long) + 64);
  hipLaunchKernelGGL(contour_fill_kernel, dim3(H, B), dim3(CF_NT), lds, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned*>(vertices), v_cap, contours, c_cap, H, W, mask);
  return (int)hipGetLastError();
}
