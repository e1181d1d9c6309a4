// Moving objects as labelled instances (predict.py --save objects): the connected components of the thresholded motion
// mask of every image, numbered in row-major order of their first pixel, and one table row per object: size, box, depth range and the
// float64 sums of the camera-space point, the object's own motion and the mask.  hipops/objects.py is the definition in numpy.
//   foreground  mask >= thresh in fp32 (false for NaN)
//   component   a maximal 4- or 8-connected set of foreground pixels of ONE image; its anchor is its smallest index y*w + x
//   object      a component of at least min_pixels pixels; objects are numbered 1, 2, ... per image by increasing anchor, the first
//               max_objects of them are kept (counts = kept, found, truncated)
//   per pixel   fp32, unfused: d = export_tap (the flip fuse with disp_flipped), s = lo + span*d, z = 1/s, p = (xc*z, yc*z, z) with
//               xc = ((float)x - cx)*ifx;  q_k = ((R[k,0]*p0 + R[k,1]*p1) + R[k,2]*p2) + t[k];  ego = q - p;  c = flow*ts[b];  r = c - ego
//   row         pixels, x0, y0, x1, y1, anchor, z_min, z_max (over the pixels with 0 < z < inf; +inf and 0 where there is none), then
//               seven doubles: sum p[3], sum r[3], sum mask
// Five launches; no workgroup waits for another, and every loop ends by construction (see uf_find and uf_union):
//   tile     a workgroup = a 16 x 64 tile of one image: union-find over the tile's row-major indices in LDS (a root is the smallest
//            index of its set), then lab[pixel] = the GLOBAL index b*h*w + y*w + x of its root, -1 for background; cnt[pixel] = 0
//   merge    one lane per pixel; a foreground pixel unites itself with each of its W, NW, N, NE neighbours (W, N under 4-connectivity)
//            that lies in another tile -- every adjacent pair across a tile edge or corner is seen from its later pixel
//   flatten  lab[pixel] = its root, cnt[root] += 1 (one atomic per wave where the wave's foreground lanes share a root)
//   number   ONE workgroup per image: zero the image's table, flag the roots with cnt >= min_pixels, exclusive scan of the flags in
//            row-major order -> the object number, kept in cnt[root]; the rows' integer fields are initialised; counts
//   reduce   labels[pixel] = cnt[lab[pixel]]; the per-pixel quantities; the row's box and depth range by integer atomicMin / atomicMax
//            (a positive finite float orders as its bit pattern), the sums by fp64 atomicAdd -- first reduced across the lanes of a
//            wave that carry one row, over the wave's four segments and over the workgroup's waves, then one atomic per quantity
// The workspace is lab and cnt, B*h*w ints each: both are written at every pixel by `tile` before anything reads them.
// Labels of different images never meet: a union joins two pixels of one image, and every parent is a pixel of its child's set.
#include <hip/hip_runtime.h>

#include "../../include/dynamo_hip.h"

// in front of the shared header: export_tap and the per-pixel arithmetic are compiled unfused in this file
#pragma clang fp contract(off)

#include "dd_export_tap.h"

namespace dd {

constexpr int OB_NT = 256;              // lanes per workgroup, every kernel
constexpr int OB_TH = 16, OB_TW = 64;   // the tile: a wave reads one 256-byte row segment, the tile's labels are 4 KB of LDS
constexpr int OB_NUM_NT = 1024;         // lanes of the numbering workgroup: one per image, so it is as wide as a workgroup gets
constexpr int OB_ITEMS = 16;            // pixels per lane and pass of the numbering scan
constexpr int OB_ROW = DD_OBJECTS_ROW;  // 32-bit words per table row
constexpr int OB_SEG = 4;               // reduce: 64-pixel segments per wave, so a workgroup covers 1024 consecutive pixels
constexpr int OB_PASSES = 8;            // reduce: rows a wave groups per segment before the rest go lane by lane

struct ObjectArgs {
  const float *mask, *disp, *flip, *l_mask, *flow, *ts, *pose;
  int B, h, w, hw, n;                   // n = B*h*w
  float ifx, ify, cx, cy, lo, span, thresh;
  int conn8, min_pixels, max_objects;
};

// A forest over pixel indices with L[x] <= x everywhere, at every moment: a parent is written once as L[x] = x and afterwards only
// lowered (atomicMin, or a store of a root below it).  The loads are relaxed atomics: a lane may see an older parent of x, which is
// still a pixel of x's set and still below x.
__device__ __forceinline__ int uf_load(const int* L, int x) { return __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Terminates: every step either returns or replaces x by L[x] < x, and x >= 0.
__device__ __forceinline__ int uf_find(const int* L, int x) {
  for (;;) {
    const int p = uf_load(L, x);
    if (p == x) return x;
    x = p;
  }
}

// Unites the sets of a and b.  Terminates without waiting for any other lane: an iteration either returns, or goes on with the pair
// (old, b) where old < a is what atomicMin found in L[a] and b < a -- max(a, b) is a non-negative integer that every iteration
// strictly lowers, whatever other lanes store meanwhile (their stores only lower parents, which keeps L[x] <= x).
// When atomicMin finds old == a, a was a root and now hangs under b: done.  Otherwise a had been given the parent `old` by another
// lane in the meantime; L[a] is now min(old, b), and the link that is not stored, between old and b, is what the next iteration makes.
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

// grid (B * tiles_y * tiles_x)
__global__ __launch_bounds__(OB_NT) void objects_tile_kernel(const ObjectArgs a, int tiles_y, int tiles_x, int* __restrict__ lab, int* __restrict__ cnt) {
  __shared__ int L[OB_TH * OB_TW];
  const int per = tiles_y * tiles_x;
  const int b = blockIdx.x / per, t = blockIdx.x - b * per;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int lx = threadIdx.x & (OB_TW - 1), wave = threadIdx.x >> 6;
  const int x = tx * OB_TW + lx, y0 = ty * OB_TH;
  const float* m = a.mask + (size_t)b * a.hw;
#pragma unroll
  for (int k = 0; k < OB_TH / 4; ++k) {
    const int ly = wave + 4 * k, y = y0 + ly;
    const bool fg = x < a.w && y < a.h && m[(size_t)y * a.w + x] >= a.thresh;
    L[ly * OB_TW + lx] = fg ? ly * OB_TW + lx : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < OB_TH / 4; ++k) {
    const int ly = wave + 4 * k, i = ly * OB_TW + lx;
    if (L[i] < 0) continue;             // the sign of a label never changes
    if (lx > 0 && L[i - 1] >= 0) uf_union(L, i, i - 1);
    if (ly > 0) {
      if (L[i - OB_TW] >= 0) uf_union(L, i, i - OB_TW);
      if (a.conn8) {
        if (lx > 0 && L[i - OB_TW - 1] >= 0) uf_union(L, i, i - OB_TW - 1);
        if (lx < OB_TW - 1 && L[i - OB_TW + 1] >= 0) uf_union(L, i, i - OB_TW + 1);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < OB_TH / 4; ++k) {
    const int ly = wave + 4 * k, y = y0 + ly, i = ly * OB_TW + lx;
    if (x >= a.w || y >= a.h) continue;
    const int g = b * a.hw + y * a.w + x;
    int root = -1;
    if (L[i] >= 0) {
      const int r = uf_find(L, i);
      root = b * a.hw + (y0 + r / OB_TW) * a.w + (tx * OB_TW + (r & (OB_TW - 1)));
    }
    lab[g] = root;
    cnt[g] = 0;
  }
}

// grid (ceil(n / 256)): the unions across tile edges and corners
__global__ __launch_bounds__(OB_NT) void objects_merge_kernel(const ObjectArgs a, int* __restrict__ lab) {
  const long long gi = (long long)blockIdx.x * OB_NT + threadIdx.x;
  if (gi >= a.n) return;
  const int i = (int)gi;
  if (uf_load(lab, i) < 0) return;
  const int rem = i % a.hw, y = rem / a.w, x = rem - y * a.w;
  const bool left = x > 0 && x % OB_TW == 0, top = y > 0 && y % OB_TH == 0;     // the W / the N neighbour is in another tile
  if (left && uf_load(lab, i - 1) >= 0) uf_union(lab, i, i - 1);
  if (top && uf_load(lab, i - a.w) >= 0) uf_union(lab, i, i - a.w);
  if (a.conn8 && y > 0) {
    if (x > 0 && (left || top) && uf_load(lab, i - a.w - 1) >= 0) uf_union(lab, i, i - a.w - 1);
    if (x < a.w - 1 && (top || (x + 1) % OB_TW == 0) && uf_load(lab, i - a.w + 1) >= 0) uf_union(lab, i, i - a.w + 1);
  }
}

// true where every lane for which `active` holds carries the same key; key0 is that key.  All lanes of the wave call it.
__device__ __forceinline__ bool wave_one_key(bool active, int key, unsigned long long& lanes, int& key0) {
  lanes = __ballot(active);
  if (lanes == 0) return false;
  key0 = __shfl(key, __ffsll((long long)lanes) - 1);
  return __ballot(active && key != key0) == 0;
}

// grid (ceil(n / 256)): no union runs here, so a root is a fixed point and every pixel finds it
__global__ __launch_bounds__(OB_NT) void objects_flatten_kernel(const ObjectArgs a, int* __restrict__ lab, int* __restrict__ cnt) {
  const long long gi = (long long)blockIdx.x * OB_NT + threadIdx.x;
  const int i = (int)(gi < a.n ? gi : 0);
  int root = -1;
  if (gi < a.n && uf_load(lab, i) >= 0) {
    root = uf_find(lab, i);
    __hip_atomic_store(lab + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // a root at or below the parent it replaces
  }
  unsigned long long lanes;
  int root0;
  if (wave_one_key(root >= 0, root, lanes, root0)) {
    if ((threadIdx.x & 63) == __ffsll((long long)lanes) - 1) atomicAdd(cnt + root0, __popcll(lanes));
  } else if (root >= 0) {
    atomicAdd(cnt + root, 1);
  }
}

// grid (B), one workgroup per image: table rows zeroed, roots numbered in row-major order, counts
__global__ __launch_bounds__(OB_NUM_NT) void objects_number_kernel(const ObjectArgs a, const int* __restrict__ lab, int* __restrict__ cnt, int* __restrict__ table,
                                                               int* __restrict__ counts) {
  __shared__ int part[OB_NUM_NT / 64];
  const int t = threadIdx.x, b = blockIdx.x, base = b * a.hw;
  int* rows = table + (size_t)b * a.max_objects * OB_ROW;
  for (int k = t; k < a.max_objects * OB_ROW; k += OB_NUM_NT) rows[k] = 0;
  __syncthreads();
  int carry = 0;
  for (int p0 = 0; p0 < a.hw; p0 += OB_NUM_NT * OB_ITEMS) {     // the pixel index is taken in 64 bits below
    const long long i0 = (long long)p0 + (long long)t * OB_ITEMS;
    int v[OB_ITEMS], mine = 0;
#pragma unroll
    for (int k = 0; k < OB_ITEMS; ++k) {
      const long long i = i0 + k;
      v[k] = 0;
      if (i < a.hw) {
        const int g = base + (int)i, c = cnt[g];
        v[k] = (lab[g] == g && c >= a.min_pixels) ? c : 0;      // the object's size, 0 where no object is anchored
      }
      mine += v[k] != 0;
    }
    int incl = mine;                    // the inclusive scan of the lanes' counts: across the wave, then the four wave totals
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
      const int up = __shfl_up(incl, step);
      if ((t & 63) >= step) incl += up;
    }
    if ((t & 63) == 63) part[t >> 6] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int u = 0; u < OB_NUM_NT / 64; ++u) {
      before += u < (t >> 6) ? part[u] : 0;
      total += part[u];
    }
    int run = carry + before + incl - mine;
#pragma unroll
    for (int k = 0; k < OB_ITEMS; ++k) {
      const long long i = i0 + k;
      if (i < a.hw) {
        int number = 0;
        if (v[k]) {
          ++run;
          if (run <= a.max_objects) {
            number = run;
            int* row = rows + (size_t)(run - 1) * OB_ROW;
            row[0] = v[k];
            row[1] = 0x7fffffff, row[2] = 0x7fffffff, row[3] = -1, row[4] = -1;
            row[5] = (int)i;
            row[6] = 0x7f800000;        // +inf; row[7], z_max, stays 0
          }
        }
        cnt[base + (int)i] = number;
      }
    }
    carry += total;
    __syncthreads();
    if (a.hw - p0 <= OB_NUM_NT * OB_ITEMS) break;               // the last pass: p0 never passes hw, so it cannot wrap
  }
  if (t == 0) {
    counts[b * 3 + 0] = carry < a.max_objects ? carry : a.max_objects;
    counts[b * 3 + 1] = carry;
    counts[b * 3 + 2] = carry > a.max_objects;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s));
  return v;
}

// a row's share of some pixels; wave-uniform where a wave carries it
struct RowAcc {
  int key, x0, y0, x1, y1, zlo, zhi;    // key: the row b * max_objects + number - 1, -1 for none
  double s[7];
};

__device__ __forceinline__ void acc_merge(RowAcc& c, const RowAcc& r) {
  c.x0 = min(c.x0, r.x0), c.y0 = min(c.y0, r.y0), c.x1 = max(c.x1, r.x1), c.y1 = max(c.y1, r.y1);
  c.zlo = min(c.zlo, r.zlo), c.zhi = max(c.zhi, r.zhi);
#pragma unroll
  for (int k = 0; k < 7; ++k) c.s[k] += r.s[k];
}

// one lane: thirteen atomics on the row
__device__ __forceinline__ void acc_flush(const RowAcc& r, int* __restrict__ table) {
  int* row = table + (size_t)r.key * OB_ROW;
  atomicMin(row + 1, r.x0), atomicMin(row + 2, r.y0), atomicMax(row + 3, r.x1), atomicMax(row + 4, r.y1);
  atomicMin(row + 6, r.zlo), atomicMax(row + 7, r.zhi);
  double* sums = reinterpret_cast<double*>(row + 8);
#pragma unroll
  for (int k = 0; k < 7; ++k) unsafeAtomicAdd(sums + k, r.s[k]);    // the hardware's fp64 add: the table is ordinary device memory
}

// grid (ceil(n / 1024)): a wave takes OB_SEG consecutive 64-pixel segments.  Per segment the object lanes are grouped by row: a pass
// takes the row of the lowest lane that is left, reduces its lanes across the wave and drops them from the set -- a pass removes at
// least that lane, and after OB_PASSES passes whatever is left goes lane by lane.  The wave carries one row's running total from
// segment to segment and issues its atomics only when another row comes up; at the end the workgroup's four waves combine the totals
// that belong to one row.  Inside an object that is thirteen atomics per 1024 pixels.
template <bool FUSE>
__global__ __launch_bounds__(OB_NT) void objects_reduce_kernel(const ObjectArgs a, const int* __restrict__ lab, const int* __restrict__ num,
                                                               int* __restrict__ labels, int* __restrict__ table) {
  __shared__ RowAcc slot[OB_NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = ((long long)blockIdx.x * (OB_NT / 64) + wave) * (64 * OB_SEG);
  RowAcc carry;
  carry.key = -1;
  for (int seg = 0; seg < OB_SEG; ++seg) {
    const long long gi = base + seg * 64 + lane;
    const bool valid = gi < a.n;
    const int i = (int)(valid ? gi : 0);
    int number = 0;
    if (valid) {
      const int root = lab[i];
      number = root >= 0 ? num[root] : 0;
      labels[i] = number;
    }
    const bool act = number > 0;
    const int b = i / a.hw, rem = i - b * a.hw, y = rem / a.w, x = rem - y * a.w;
    RowAcc me;
    me.key = b * a.max_objects + number - 1;                // B * max_objects <= 2^31 - 1
    me.x0 = 0x7fffffff, me.y0 = 0x7fffffff, me.x1 = -1, me.y1 = -1, me.zlo = 0x7f800000, me.zhi = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) me.s[k] = 0.0;
    if (act) {
      const float* l_img = a.disp + (size_t)b * a.hw;
      const float* r_img = FUSE ? a.flip + (size_t)b * a.hw : nullptr;
      const float d = export_tap<FUSE>(l_img, r_img, a.l_mask, a.w, y, x);
      const float z = 1.f / (a.lo + a.span * d);
      const float xc = ((float)x - a.cx) * a.ifx, yc = ((float)y - a.cy) * a.ify;
      const float p0 = xc * z, p1 = yc * z, p2 = z;
      const float* T = a.pose + (size_t)b * 12;
      const float* f = a.flow + (size_t)b * 3 * a.hw + rem;
      const float ts = a.ts[b];
      const float q0 = ((T[0] * p0 + T[1] * p1) + T[2] * p2) + T[3];
      const float q1 = ((T[4] * p0 + T[5] * p1) + T[6] * p2) + T[7];
      const float q2 = ((T[8] * p0 + T[9] * p1) + T[10] * p2) + T[11];
      me.s[0] = p0, me.s[1] = p1, me.s[2] = p2;
      me.s[3] = f[0] * ts - (q0 - p0);
      me.s[4] = f[a.hw] * ts - (q1 - p1);
      me.s[5] = f[2 * (size_t)a.hw] * ts - (q2 - p2);
      me.s[6] = a.mask[i];
      me.x0 = me.x1 = x, me.y0 = me.y1 = y;
      if (z > 0.f && z < __int_as_float(0x7f800000)) me.zlo = me.zhi = __float_as_int(z);
    }
    unsigned long long todo = __ballot(act);                // wave-uniform, as everything the passes decide on
    for (int pass = 0; todo != 0 && pass < OB_PASSES; ++pass) {
      RowAcc r;
      r.key = __shfl(me.key, __ffsll((long long)todo) - 1);
      const bool mine = act && me.key == r.key;
      r.x0 = wave_min(mine ? me.x0 : 0x7fffffff), r.y0 = wave_min(mine ? me.y0 : 0x7fffffff), r.zlo = wave_min(mine ? me.zlo : 0x7f800000);
      r.x1 = wave_max(mine ? me.x1 : -1), r.y1 = wave_max(mine ? me.y1 : -1), r.zhi = wave_max(mine ? me.zhi : 0);
#pragma unroll
      for (int k = 0; k < 7; ++k) r.s[k] = wave_sum(mine ? me.s[k] : 0.0);
      if (carry.key == r.key) {
        acc_merge(carry, r);
      } else {
        if (carry.key >= 0 && lane == 0) acc_flush(carry, table);
        carry = r;
      }
      todo &= ~__ballot(mine);
    }
    if ((todo >> lane) & 1) acc_flush(me, table);           // more than OB_PASSES rows in one segment: the rest lane by lane
  }
  if (lane == 0) slot[wave] = carry;
  __syncthreads();
  if (threadIdx.x < OB_NT / 64) {
    RowAcc c = slot[threadIdx.x];
    bool lead = c.key >= 0;
    for (int u = 0; u < (int)threadIdx.x; ++u) lead = lead && slot[u].key != c.key;     // the first wave with this row speaks for it
    if (lead) {
      for (int u = threadIdx.x + 1; u < OB_NT / 64; ++u)
        if (slot[u].key == c.key) acc_merge(c, slot[u]);
      acc_flush(c, table);
    }
  }
}

// grid (ceil(B*H*W / 256))
__global__ __launch_bounds__(OB_NT) void labels_u16_kernel(const int* __restrict__ labels, int h, int w, int H, int W, long long total,
                                                           unsigned short* __restrict__ out) {
  const long long i = (long long)blockIdx.x * OB_NT + threadIdx.x;
  if (i >= total) return;
  const long long HW = (long long)H * W;
  const long long b = i / HW, rem = i - b * HW;
  const int Y = (int)(rem / W), X = (int)(rem - (long long)Y * W);
  const int y = (int)min((long long)h - 1, ((2LL * Y + 1) * h) / (2LL * H)), x = (int)min((long long)w - 1, ((2LL * X + 1) * w) / (2LL * W));
  const int v = labels[(b * h + y) * w + x];
  out[i] = (unsigned short)(v < 0 ? 0 : v > 65535 ? 65535 : v);
}

// host: false for the sizes the entry points refuse
static bool objects_sizes(int B, int h, int w, int max_objects) {
  if (B < 1 || h < 1 || w < 1 || max_objects < 1 || max_objects > 65535) return false;
  if ((long long)B * h * w > 0x7fffffffLL || (long long)h * w > 0x7fffffffLL || (long long)B * max_objects > 0x7fffffffLL) return false;
  const long long tiles = (long long)B * ((h + OB_TH - 1) / OB_TH) * ((w + OB_TW - 1) / OB_TW);
  return tiles <= 0x7fffffffLL;
}

}  // namespace dd

using namespace dd;

extern "C" size_t dd_objects_workspace_bytes(int B, int h, int w, int max_objects) {
  return objects_sizes(B, h, w, max_objects) ? (size_t)B * h * w * 2 * sizeof(int) : 0;      // lab and cnt
}

extern "C" int dd_objects(const float* motion_mask, const float* disp, const float* disp_flipped, const float* l_mask, const float* complete_flow,
                          const float* ts, const float* pose, int B, int h, int w, float fx, float fy, float cx, float cy, float lo, float span,
                          float thresh, int connectivity, int min_pixels, int max_objects, int* labels, void* table, int* counts, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (!motion_mask || !disp || !complete_flow || !ts || !pose || !labels || !table || !counts || !workspace ||
      (disp_flipped == nullptr) != (l_mask == nullptr))
    return (int)hipErrorInvalidValue;
  if (!objects_sizes(B, h, w, max_objects) || (connectivity != 4 && connectivity != 8) || min_pixels < 1) return (int)hipErrorInvalidValue;
  if (fx == 0.f || fy == 0.f || !(fx - fx == 0.f) || !(fy - fy == 0.f)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)motion_mask & 3u) || ((uintptr_t)disp & 3u) || ((uintptr_t)disp_flipped & 3u) || ((uintptr_t)l_mask & 3u) || ((uintptr_t)complete_flow & 3u) ||
      ((uintptr_t)ts & 3u) || ((uintptr_t)pose & 3u) || ((uintptr_t)labels & 3u) || ((uintptr_t)counts & 3u) || ((uintptr_t)table & 7u) ||
      ((uintptr_t)workspace & 7u))
    return (int)hipErrorInvalidValue;
  if (workspace_bytes < dd_objects_workspace_bytes(B, h, w, max_objects)) return (int)hipErrorInvalidValue;
  ObjectArgs a;
  a.mask = motion_mask, a.disp = disp, a.flip = disp_flipped, a.l_mask = l_mask, a.flow = complete_flow, a.ts = ts, a.pose = pose;
  a.B = B, a.h = h, a.w = w, a.hw = h * w, a.n = B * h * w;
  a.ifx = (float)(1.0 / (double)fx), a.ify = (float)(1.0 / (double)fy), a.cx = cx, a.cy = cy, a.lo = lo, a.span = span, a.thresh = thresh;
  a.conn8 = connectivity == 8, a.min_pixels = min_pixels, a.max_objects = max_objects;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int* lab = static_cast<int*>(workspace);
  int* cnt = lab + a.n;
  int* rows = static_cast<int*>(table);
  const int tiles_y = (h + OB_TH - 1) / OB_TH, tiles_x = (w + OB_TW - 1) / OB_TW;
  const unsigned flat = (unsigned)(((long long)a.n + OB_NT - 1) / OB_NT);
  hipLaunchKernelGGL(objects_tile_kernel, dim3((unsigned)(B * tiles_y * tiles_x)), dim3(OB_NT), 0, st, a, tiles_y, tiles_x, lab, cnt);
  hipLaunchKernelGGL(objects_merge_kernel, dim3(flat), dim3(OB_NT), 0, st, a, lab);
  hipLaunchKernelGGL(objects_flatten_kernel, dim3(flat), dim3(OB_NT), 0, st, a, lab, cnt);
  hipLaunchKernelGGL(objects_number_kernel, dim3((unsigned)B), dim3(OB_NUM_NT), 0, st, a, lab, cnt, rows, counts);
  const unsigned wide = (unsigned)(((long long)a.n + OB_NT * OB_SEG - 1) / (OB_NT * OB_SEG));
  if (disp_flipped)
    hipLaunchKernelGGL(objects_reduce_kernel<true>, dim3(wide), dim3(OB_NT), 0, st, a, lab, cnt, labels, rows);
  else
    hipLaunchKernelGGL(objects_reduce_kernel<false>, dim3(wide), dim3(OB_NT), 0, st, a, lab, cnt, labels, rows);
  return (int)hipGetLastError();
}

extern "C" int dd_export_labels_u16(const int* labels, int B, int h, int w, int H, int W, uint16_t* out, void* stream) {
  if (!labels || !out || B < 1 || h < 1 || w < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  if ((long long)h * w > 0x7fffffffLL || (long long)H * W > 0x7fffffffLL || (long long)B * h * w > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const long long total = (long long)B * H * W;
  if ((total + OB_NT - 1) / OB_NT > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (((uintptr_t)labels & 3u) || ((uintptr_t)out & 1u)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(labels_u16_kernel, dim3((unsigned)((total + OB_NT - 1) / OB_NT)), dim3(OB_NT), 0, static_cast<hipStream_t>(stream), labels, h, w, H, W,
                     total, out);
  return (int)hipGetLastError();
}
