// Semantic keypoints: the class of each keypoint straight from the NHWC convSout map, a stable
// per-image compaction of the point set by class, and the class test of the two-way matcher (match_dist_kernel<true>,
// describe_kernels.hip.h).
//   point_class_kernel     one wave per point, lanes = classes: the value sem_predict_kernel gives pixel (y, x) for class c
//                          (semp_interp, sem_eval_kernels.hip.h: the same weights, the same four products and three sums),
//                          then a wave arg-max that keeps (value, lowest index).  ~1000 points x C values per image against
//                          H x W x C for the class map.
//   filter_count_kernel    keep flags (row < count and bit cls of the 256-bit mask) counted per 1024-row block
//   filter_scatter_kernel  every block sums the block counts before it and writes its surviving rows in order: the STABLE
//                          cross-workgroup compaction of track_kernels.hip.h (block_scan_flag / block_base), so the
//                          result does not depend on the order the blocks run in and needs no atomic ticket.  The 1 KiB
//                          descriptor rows are moved by whole waves (16 bytes per lane), not by the thread that owns the row.
#pragma once
#include "geom_blocks.hip.h"
#include "sem_eval_kernels.hip.h"
#include "track_kernels.hip.h"  // TRACK_BLOCK

namespace sspk {

#define POINT_CLASS_NONE 255  // SSP_CLASS_NONE

// sout [B][Hc*Wc][cs] raw logits; pts [B][cap][stride] float rows starting (x, y) = an integer pixel; count [B] (clamped
// to cap); cls [B][cap]: rows < count get the class, the others POINT_CLASS_NONE.  A point outside the image is clamped
// into it.  The classes c < C are scanned in passes of 64; the four corner loads of a pass are consecutive over the lanes.
__global__ __launch_bounds__(256) void point_class_kernel(const float* __restrict__ sout, const float* __restrict__ pts,
                                                          const int32_t* __restrict__ count, uint8_t* __restrict__ cls, int Hc,
                                                          int Wc, int C, int cs, int cap, int stride) {
  const int img = blockIdx.y, r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= cap) return;
  uint8_t* const out = cls + (size_t)img * cap + r;
  if (r >= min(count[img], cap)) {
    if (lane == 0) *out = POINT_CLASS_NONE;
    return;
  }
  const float* q = pts + ((size_t)img * cap + r) * stride;
  const int x = min(max((int)q[0], 0), 8 * Wc - 1), y = min(max((int)q[1], 0), 8 * Hc - 1);
  // pixel (y, x) is lane (ly, lx) of sem_predict_kernel's tile (ty, tx): the 8x8 tile grid shifted by (4, 4)
  const int ty = ((y + 4) >> 3) - 1, ly = (y + 4) & 7, tx = ((x + 4) >> 3) - 1, lx = (x + 4) & 7;
  const int cy0 = max(ty, 0), cy1 = min(ty + 1, Hc - 1), cx0 = max(tx, 0), cx1 = min(tx + 1, Wc - 1);
  const float wy1 = cy0 == cy1 ? 0.f : (float)(2 * ly + 1) * 0.0625f, wx1 = cx0 == cx1 ? 0.f : (float)(2 * lx + 1) * 0.0625f;
  const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
  const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;  // multiples of 1 / 256: exact
  const float* const base = sout + (size_t)img * Hc * Wc * cs;
  const float* const p00 = base + (size_t)(cy0 * Wc + cx0) * cs;
  const float* const p01 = base + (size_t)(cy0 * Wc + cx1) * cs;
  const float* const p10 = base + (size_t)(cy1 * Wc + cx0) * cs;
  const float* const p11 = base + (size_t)(cy1 * Wc + cx1) * cs;
  // strict > walking the lane's classes upward, then between lanes the larger value and, on equal values, the lower index:
  // the first index at which sem_predict_kernel's walk over 0 .. C-1 reaches its maximum (0 when no class beats -inf)
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float l = semp_interp(w00, w01, w10, w11, p00[c], p01[c], p10[c], p11[c]);
    if (l > best) { best = l; idx = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int oi = __shfl_xor(idx, o);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if (lane == 0) *out = (uint8_t)(idx == 0x7fffffff ? 0 : idx);
}

struct ClassMask {  // bit c of word c / 32: class c is kept
  uint32_t w[8];
};

__device__ __forceinline__ bool filter_keep(const ClassMask& m, const uint8_t* __restrict__ cls, int r, int n) {
  if (r >= n) return false;
  const int c = cls[r];
  return (m.w[c >> 5] >> (c & 31)) & 1u;
}

// grid (cdiv(cap, TRACK_BLOCK), n); block_sums [n][gridDim.x]
__global__ __launch_bounds__(TRACK_BLOCK) void filter_count_kernel(const int32_t* __restrict__ count, const uint8_t* __restrict__ cls,
                                                                   ClassMask mask, int cap, int32_t* __restrict__ block_sums) {
  __shared__ int wsum[TRACK_BLOCK / 64];
  const int img = blockIdx.y, r = blockIdx.x * TRACK_BLOCK + threadIdx.x;
  const int n = min(max(count[img], 0), cap);
  int total;
  block_scan_flag<TRACK_BLOCK>(filter_keep(mask, cls + (size_t)img * cap, r, n), wsum, total);
  if (threadIdx.x == 0) block_sums[img * gridDim.x + blockIdx.x] = total;
}

// pts [n][cap][5], desc [n][cap][256], cls [n][cap] -> the kept rows in their order; count_out [n].  cls_out is filled
// with POINT_CLASS_NONE before the launch; pts_out / desc_out rows past the new count are not written.
__global__ __launch_bounds__(TRACK_BLOCK) void filter_scatter_kernel(const float* __restrict__ pts, const int32_t* __restrict__ count,
                                                                     const float* __restrict__ desc, const uint8_t* __restrict__ cls,
                                                                     ClassMask mask, int cap, const int32_t* __restrict__ block_sums,
                                                                     float* __restrict__ pts_out, int32_t* __restrict__ count_out,
                                                                     float* __restrict__ desc_out, uint8_t* __restrict__ cls_out) {
  __shared__ int wsum[TRACK_BLOCK / 64];
  __shared__ int red[TRACK_BLOCK / 64];
  __shared__ int dst[TRACK_BLOCK];
  const int img = blockIdx.y, b = blockIdx.x, r = b * TRACK_BLOCK + threadIdx.x;
  const int n = min(max(count[img], 0), cap);
  const size_t row0 = (size_t)img * cap;
  const int base = block_base<TRACK_BLOCK>(block_sums + img * gridDim.x, b, red);
  const bool keep = filter_keep(mask, cls + row0, r, n);
  int total;
  const int pos = base + block_scan_flag<TRACK_BLOCK>(keep, wsum, total);  // pos <= r < cap
  dst[threadIdx.x] = keep ? pos : -1;
  if (keep) {
    const float* s = pts + (row0 + r) * 5;
    float* d = pts_out + (row0 + pos) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) d[k] = s[k];
    cls_out[row0 + pos] = cls[row0 + r];
  }
  if (b == gridDim.x - 1 && threadIdx.x == 0) count_out[img] = base + total;
  __syncthreads();
  if (total == 0) return;  // (uniform over the block)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < TRACK_BLOCK; k += TRACK_BLOCK / 64) {
    const int p = dst[k];  // wave-uniform
    if (p < 0) continue;
    const float4* s = reinterpret_cast<const float4*>(desc + (row0 + (size_t)b * TRACK_BLOCK + k) * 256);
    reinterpret_cast<float4*>(desc_out + (row0 + p) * 256)[lane] = s[lane];
  }
}

}  // namespace sspk
