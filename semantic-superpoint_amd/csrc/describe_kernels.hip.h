// Descriptor export (export.py:66-190 `export_descriptor`): the sparse-descriptor half and the matcher, after the eval
// forward and the batched keypoint extraction (nms_*_kernel with blockIdx.y = image, export_kernels.hip.h).
//   sample_desc_kernel     models/model_wrap.py:295-313 sample_desc_from_points: grid_sample(bilinear, zeros padding,
//                          align_corners=True) of the coarse descriptor at the INTEGER keypoints, then / its fp32 L2 norm
//   match_dist_kernel      models/model_wrap.py:451-497 nn_match_two_way: D1^T D2 on the fp32 matrix cores
//                          (v_mfma_f32_32x32x2_f32, K = 256), d = sqrt(2 - 2 clip(dot, -1, 1)), row and column argmin of d
//                          as 64-bit atomicMin of (float bits of d) << 32 | index (order-independent: first index on ties,
//                          as np.argmin)
//   match_compact_kernel   keep = d_row < nn_thresh && colargmin[rowargmin[i]] == i, rows ascending -> (i, j, d)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sspk {

// One wave per point; lane l owns channels 4l .. 4l+3.  desc: image k, cell c, channel ch at
// k*img_stride + c*cell_stride + ch*chan_stride (the slot's NHWC rows: cell_stride 256, chan_stride 1; a public NCHW
// tensor: cell_stride 1, chan_stride Hc*Wc).  xy: [n][cap][xy_row] floats, (x, y) first; count: [n] (clamped to cap).
// out: [n][cap][256]; rows >= count are not written.
__global__ __launch_bounds__(256) void sample_desc_kernel(const float* __restrict__ desc, long img_stride, long cell_stride,
                                                          long chan_stride, int Hc, int Wc, const float* __restrict__ xy,
                                                          int xy_row, const int32_t* __restrict__ count, int cap,
                                                          float* __restrict__ out) {
  const int img = blockIdx.y, r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n = min(count[img], cap);
  if (r >= n) return;
  const float* q = xy + ((size_t)img * cap + r) * xy_row;
  // samp_pts = pts / (W/2) - 1 in float64 (the points are a float64 array), then .float() (model_wrap.py:303-307)
  const float xn = (float)((double)q[0] / ((double)(8 * Wc) / 2.0) - 1.0);
  const float yn = (float)((double)q[1] / ((double)(8 * Hc) / 2.0) - 1.0);
  // ATen's CPU grid sampler, align_corners=True: (g + 1) * ((size - 1) / 2), then the four bilinear weights
  const float ix = (xn + 1.f) * ((float)(Wc - 1) / 2.f), iy = (yn + 1.f) * ((float)(Hc - 1) / 2.f);
  const float x0f = floorf(ix), y0f = floorf(iy);
  const float w = ix - x0f, e = 1.f - w, nn = iy - y0f, s = 1.f - nn;
  const float wt[4] = {s * e, s * w, nn * e, nn * w};  // nw, ne, sw, se
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float* base = desc + (size_t)img * img_stride;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xx >= 0 && xx < Wc && yy >= 0 && yy < Hc) {
      const float* p = base + (size_t)(yy * Wc + xx) * cell_stride;
      if (chan_stride == 1) {
        c = *reinterpret_cast<const float4*>(p + 4 * lane);
      } else {
        c.x = p[(4 * lane) * chan_stride]; c.y = p[(4 * lane + 1) * chan_stride];
        c.z = p[(4 * lane + 2) * chan_stride]; c.w = p[(4 * lane + 3) * chan_stride];
      }
    }
    v[0] += c.x * wt[t]; v[1] += c.y * wt[t]; v[2] += c.z * wt[t]; v[3] += c.w * wt[t];
  }
  float ss = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
  const float nrm = __fsqrt_rn(ss);
  float4 o4;
  o4.x = v[0] / nrm; o4.y = v[1] / nrm; o4.z = v[2] / nrm; o4.w = v[3] / nrm;
  *reinterpret_cast<float4*>(out + ((size_t)img * cap + r) * 256 + 4 * lane) = o4;
}

constexpr int MATCH_TILE = 64;  // a block = 2 x 2 waves of 32 x 32 distances

// (spelled out: the HIP `min` overloads do not cover every 64-bit unsigned type exactly)
__device__ __forceinline__ uint64_t min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
  const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
  return ((uint64_t)hi << 32) | lo;
}

// Pair p: descriptors d1[p*pair_stride][cap][256] (n1 = count1[p*pair_stride] rows), d2 likewise.  rowmin: [P][cap] keys
// of each d1 row's nearest d2 column, colmin: [P][cap] the reverse; both start at ~0.
// MFMA operands: lane (r = l & 31, h = l >> 5) loads 4 consecutive k of row r at 8s + 4h and feeds component c as k-pair
// CLASSES (ssp_match_two_way_classes): cls1, cls2 [.][cap] uint8 beside the descriptors; a pair (i, j)
// with cls1[i] != cls2[j] is no candidate of either arg-min.  A row or column without a candidate keeps its ~0 key, which
// match_compact_kernel never keeps (its distance bits are a NaN, its index is >= n2).  CLASSES = false reads neither pointer.
template <bool CLASSES>
__global__ __launch_bounds__(256) void match_dist_kernel(const float* __restrict__ d1, const int32_t* __restrict__ count1,
                                                         const float* __restrict__ d2, const int32_t* __restrict__ count2,
                                                         int cap, int pair_stride, uint64_t* __restrict__ rowmin,
                                                         uint64_t* __restrict__ colmin, const uint8_t* __restrict__ cls1,
                                                         const uint8_t* __restrict__ cls2) {
  const int p = blockIdx.z, ps = p * pair_stride;
  const int n1 = min(count1[ps], cap), n2 = min(count2[ps], cap);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wi = blockIdx.x * MATCH_TILE + (wave >> 1) * 32, wj = blockIdx.y * MATCH_TILE + (wave & 1) * 32;
  if (wi >= n1 || wj >= n2) return;  // (whole waves; no block barrier below)
  const float4* A = reinterpret_cast<const float4*>(d1 + ((size_t)ps * cap + min(wi + r, n1 - 1)) * 256) + h;
  const float4* B = reinterpret_cast<const float4*>(d2 + ((size_t)ps * cap + min(wj + r, n2 - 1)) * 256) + h;
  // the classes of the wave's 32 rows (lane l: row wi + (l & 31)) and of this lane's column, loaded ahead of the MFMA loop
  int ci_rows = 0, cj = 0;
  if (CLASSES) {
    ci_rows = cls1[(size_t)ps * cap + min(wi + r, n1 - 1)];
    cj = cls2[(size_t)ps * cap + min(wj + r, n2 - 1)];
  }
  typedef float floatx16 __attribute__((ext_vector_type(16)));
  floatx16 acc;
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = 0.f;
#pragma unroll 4
  for (int s = 0; s < 32; ++s) {
    const float4 a = A[2 * s], b = B[2 * s];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
  // accumulator t of lane l: row (t & 3) + 8 (t >> 2) + 4h, column r
  const int j = wj + r;
  uint64_t cbest = ~0ull;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int i = wi + (t & 3) + 8 * (t >> 2) + 4 * h;
    bool ok = i < n1 && j < n2;
    if (CLASSES) {  // row (t & 3) + 8 (t >> 2) + 4h of the wave: two wave-uniform lane reads, chosen by h
      const int c0 = __builtin_amdgcn_readlane(ci_rows, (t & 3) + 8 * (t >> 2));
      const int c1 = __builtin_amdgcn_readlane(ci_rows, (t & 3) + 8 * (t >> 2) + 4);
      ok = ok && (h ? c1 : c0) == cj;
    }
    // np.sqrt(2 - 2 * np.clip(dmat, -1, 1)) in fp32: 2 * clip is exact, one rounding for the difference, one for sqrt.
    // sqrtf is the correctly rounded root; __fsqrt_rn compiles to the native one, which may be an ulp off: enough to move a
    // distance across nn_thresh or to order two candidates otherwise than the reference does
    const float dd = sqrtf(2.f - 2.f * fminf(fmaxf(acc[t], -1.f), 1.f));
    const uint64_t hi = (uint64_t)__float_as_uint(dd) << 32;
    uint64_t kr = ok ? hi | (uint32_t)j : ~0ull;
    cbest = min_u64(cbest, ok ? hi | (uint32_t)i : ~0ull);
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) kr = min_u64(kr, shfl_xor_u64(kr, o));
    if (r == 0 && i < n1) atomicMin((unsigned long long*)(rowmin + (size_t)p * cap + i), (unsigned long long)kr);
  }
  cbest = min_u64(cbest, shfl_xor_u64(cbest, 32));
  if (h == 0 && j < n2) atomicMin((unsigned long long*)(colmin + (size_t)p * cap + j), (unsigned long long)cbest);
}

// One block per pair: the order-preserving compaction of the mutual matches.  match: [P][cap][3] = (i, j, d) as floats
// (indices < 2^24 are exact), n_match: [P].
__global__ __launch_bounds__(1024) void match_compact_kernel(const uint64_t* __restrict__ rowmin,
                                                             const uint64_t* __restrict__ colmin,
                                                             const int32_t* __restrict__ count1,
                                                             const int32_t* __restrict__ count2, int cap, int pair_stride,
                                                             float thresh, float* __restrict__ match,
                                                             int32_t* __restrict__ n_match) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n1 = min(count1[p * pair_stride], cap), n2 = min(count2[p * pair_stride], cap);
  if (n1 <= 0 || n2 <= 0) {
    if (tid == 0) n_match[p] = 0;
    return;
  }
  if (tid == 0) base = 0;
  __syncthreads();
  const uint64_t* rm = rowmin + (size_t)p * cap;
  const uint64_t* cm = colmin + (size_t)p * cap;
  float* out = match + (size_t)p * cap * 3;
  for (int i0 = 0; i0 < n1; i0 += 1024) {
    const int i = i0 + tid;
    bool keep = false;
    uint32_t j = 0;
    float dd = 0.f;
    if (i < n1) {
      const uint64_t k = rm[i];
      j = (uint32_t)k;
      dd = __uint_as_float((uint32_t)(k >> 32));
      keep = dd < thresh && j < (uint32_t)n2 && (uint32_t)cm[j] == (uint32_t)i;
    }
    const uint64_t bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (keep) {
      float* o = out + (size_t)(off + before) * 3;
      o[0] = (float)i; o[1] = (float)j; o[2] = dd;
    }
    __syncthreads();
    if (tid == 0) {
      int t = 0;
      for (int w = 0; w < 16; ++w) t += wsum[w];
      base += t;
    }
    __syncthreads();
  }
  if (tid == 0) n_match[p] = base;
}

}  // namespace sspk
