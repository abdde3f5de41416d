// Segmentation head read-out: fused bilinear upsample (x8, align_corners=False) + argmax over the classes + confusion-matrix
// accumulation, straight from the NHWC convSout map - the [B,C,H,W] logits are never materialised (the loss: sem_kernels.hip.h).
//   reference: models/SuperPointNet_gauss2_ssmall.py:87-91 (F.interpolate bilinear, align_corners=False),
//              Train_model_heatmap_all.py:442-443 (images_dict["sem_pred"] / ["warp_sem_pred"]: the logits the class map comes from).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sspk {

constexpr int SEMP_MAX_C = 256;       // the class map is uint8
constexpr int SEMP_WAVES = 4096;      // waves a large launch aims at (256 CUs x 4 SIMDs x 4)
constexpr int SEMP_MIN_TILES = 4;     // tiles per wave at least: the pending list below merges over them

// One wave per 8x8 pixel tile shifted by (4,4), lanes = pixels: all 64 pixels of such a tile interpolate between the same four
// cells with the constant weights (2 i + 1) / 16 (PyTorch's area_pixel_compute_source_index, restated as up_src in
// sem_kernels.hip.h, at scale 1 / 8: source = tile + (2 i + 1) / 16).  The four corner logits of a class are wave-uniform
// loads; every lane interpolates its own pixel on the raw fp32 logits (four products of exact weights, three sums) and keeps a
// running maximum and its index.  Only the classes c < C are scanned: the padding channels C .. cs - 1 are zero in the engine and
// would win over an all-negative pixel.  Ties: strict > while walking the classes upward - the lowest class index wins (torch's
// first-occurrence argmax).  At the image border the two cells of an axis coincide; the weight of the second is set to 0 there,
// which gives the clamped value exactly.
//
// Confusion matrix (row = label, column = prediction; labels outside [0, C) are ignored like in sem_ce_kernel and add to no cell):
// 64-bit integer atomics, so the result does not depend on the order and is bit-identical from run to run.  Pre-aggregation in
// registers, for every C (256^2 counters do not fit LDS):
//   * inside a tile the lanes with equal key = label C + prediction are merged with ballots (one step per DISTINCT key; a
//     segmentation map has one to four per tile);
//   * a wave walks tiles_per_wave consecutive tiles and keeps up to 64 pending (key, count) pairs, one per lane; a key that is
//     already pending only adds to its lane's count.  The pairs go out as ONE atomic instruction at the end of the walk.  A tile key
//     that finds the list full goes out at once from its leading lane (uniformly random labels: still exact, only slower).
// The value of one class at one pixel: four products of exact weights and three sums on the raw fp32 logits, innermost first
// (shared with point_class_kernel, point_class_kernels.hip.h: both must give a pixel the same bits).
__device__ __forceinline__ float semp_interp(float w00, float w01, float w10, float w11, float a, float b, float c, float d) {
  return fmaf(w00, a, fmaf(w01, b, fmaf(w10, c, w11 * d)));
}

// VEC4: cs % 4 == 0 and a 16-byte aligned map - four classes per wave-uniform 16-byte load.
template <bool VEC4>
__global__ __launch_bounds__(256) void sem_predict_kernel(const float* __restrict__ sout, const int64_t* __restrict__ labels,
                                                          uint8_t* __restrict__ pred, unsigned long long* __restrict__ conf, int B,
                                                          int Hc, int Wc, int C, int cs, int tiles_per_wave) {
  const int wave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int TX = Wc + 1, TY = Hc + 1, ntile = B * TX * TY, H = 8 * Hc, W = 8 * Wc;
  const int t0 = wave * tiles_per_wave, t1 = min(ntile, t0 + tiles_per_wave);
  const int ly = lane >> 3, lx = lane & 7;
  const float wy1c = (float)(2 * ly + 1) * 0.0625f, wx1c = (float)(2 * lx + 1) * 0.0625f;
  const bool want_conf = conf != nullptr && labels != nullptr;
  int pend_key = -1, pend_cnt = 0, npend = 0;  // this lane's pending pair; npend is wave-uniform
  for (int tile = t0; tile < t1; ++tile) {
    const int tx = tile % TX - 1, ty = (tile / TX) % TY - 1, n = tile / (TX * TY);
    const int cy0 = max(ty, 0), cy1 = min(ty + 1, Hc - 1), cx0 = max(tx, 0), cx1 = min(tx + 1, Wc - 1);
    const float wy1 = cy0 == cy1 ? 0.f : wy1c, wx1 = cx0 == cx1 ? 0.f : wx1c;
    const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
    const float w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;  // multiples of 1 / 256: exact
    const float* const base = sout + (size_t)n * Hc * Wc * cs;
    const float* const p00 = base + (size_t)(cy0 * Wc + cx0) * cs;
    const float* const p01 = base + (size_t)(cy0 * Wc + cx1) * cs;
    const float* const p10 = base + (size_t)(cy1 * Wc + cx0) * cs;
    const float* const p11 = base + (size_t)(cy1 * Wc + cx1) * cs;
    float best = -INFINITY;
    int idx = 0;
#define SEMP_CLASS(CI, A, B_, C_, D)                                      \
    {                                                                     \
      const float l = semp_interp(w00, w01, w10, w11, A, B_, C_, D);       \
      if (l > best) { best = l; idx = (CI); }                             \
    }
    int c = 0;
    if (VEC4) {
      for (; c + 7 < C; c += 8) {  // 8 wave-uniform 16-byte loads in flight
        float4 v[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          v[u][0] = *reinterpret_cast<const float4*>(p00 + c + 4 * u);
          v[u][1] = *reinterpret_cast<const float4*>(p01 + c + 4 * u);
          v[u][2] = *reinterpret_cast<const float4*>(p10 + c + 4 * u);
          v[u][3] = *reinterpret_cast<const float4*>(p11 + c + 4 * u);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          SEMP_CLASS(c + 4 * u + 0, v[u][0].x, v[u][1].x, v[u][2].x, v[u][3].x)
          SEMP_CLASS(c + 4 * u + 1, v[u][0].y, v[u][1].y, v[u][2].y, v[u][3].y)
          SEMP_CLASS(c + 4 * u + 2, v[u][0].z, v[u][1].z, v[u][2].z, v[u][3].z)
          SEMP_CLASS(c + 4 * u + 3, v[u][0].w, v[u][1].w, v[u][2].w, v[u][3].w)
        }
      }
    } else {
      for (; c + 3 < C; c += 4) {  // 16 wave-uniform 4-byte loads in flight
        float a[4], b[4], cc[4], d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[u] = p00[c + u]; b[u] = p01[c + u]; cc[u] = p10[c + u]; d[u] = p11[c + u]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) SEMP_CLASS(c + u, a[u], b[u], cc[u], d[u])
      }
    }
    for (; c < C; ++c) SEMP_CLASS(c, p00[c], p01[c], p10[c], p11[c])
#undef SEMP_CLASS
    const int y = 8 * ty + 4 + ly, x = 8 * tx + 4 + lx;
    const bool inside = y >= 0 && y < H && x >= 0 && x < W;
    const size_t pix = ((size_t)n * H + (size_t)max(y, 0)) * W + (size_t)max(x, 0);
    if (pred != nullptr && inside) pred[pix] = (uint8_t)idx;
    if (!want_conf) continue;
    int key = -1;
    if (inside) {
      const int64_t lv = labels[pix];
      if ((uint64_t)lv < (uint64_t)C) key = (int)lv * C + idx;  // (the test of sem_count_kernel, on all 64 bits)
    }
    unsigned long long todo = __ballot(key >= 0);
    int direct = 0;
    while (todo != 0ull) {  // one step per distinct key of the tile; everything that steers it is wave-uniform
      const int lead = __ffsll((long long)todo) - 1;
      const int k = __builtin_amdgcn_readlane(key, lead);
      const unsigned long long grp = __ballot(key == k);
      todo &= ~grp;
      const int cnt = __popcll(grp);
      const unsigned long long hit = __ballot(pend_key == k);
      if (hit != 0ull) {
        if (lane == __ffsll((long long)hit) - 1) pend_cnt += cnt;
      } else if (npend < 64) {
        if (lane == npend) { pend_key = k; pend_cnt = cnt; }
        ++npend;
      } else if (lane == lead) {
        direct = cnt;
      }
    }
    if (direct != 0) atomicAdd(conf + key, (unsigned long long)direct);
  }
  if (want_conf && pend_key >= 0) atomicAdd(conf + pend_key, (unsigned long long)pend_cnt);
}

}  // namespace sspk
