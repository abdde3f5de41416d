// Detector evaluation against ground-truth corners (compute_tp_fp / compute_pr / compute_mAP / compute_loc_error of the
// reference, evaluations/detector_evaluation.py:15-136; the rules are restated in DESIGN.md section 19).
//
// Per call (one batch of images) the true / false positive pass is four launches and one memset, without a distance matrix,
// without a cap on the ground-truth points and without a host synchronisation:
//   det_match_kernel    one thread per candidate slot (a pixel of a dense map, or a row of a point list).  A candidate
//                       (prob > remove_zero) scans its clipped (2r+1)^2 window row-major; g = the first label pixel with
//                       dy^2 + dx^2 <= r2 (np.argmax of the reference's match row: first in row-major order, not nearest).
//                       It takes a 64-bit atomicMax of (prob bits << 32 | position) into best[g], and, above prob_thresh,
//                       adds one to the histogram of its minimum d2.  The block's candidate count goes to block_sums.
//                       A point-list row outside the image is no candidate; state word 3 counts such rows.
//                       simplified: best[] only flags EVERY label pixel in range of a candidate (the reference's n_gt).
//   det_offsets_kernel  one workgroup: exclusive scan of the block counts.
//   det_emit_kernel     STABLE compaction (block offset + in-block scan, no ticket counter): candidate k of the call becomes
//                       record state[0] + k and writes the key prob bits << 32 | record << 1 | tp, tp = best[g] == own key
//                       (simplified: any g).  Records past `capacity` set the overflow word and write nothing.
//   det_finish_kernel   n_gt += label pixels (simplified: label pixels some prediction matched); state[0] += candidates.
// Every key is unique (the record index is part of it), so any correct descending sort of the int64 keys gives one order:
// descending probability, among equals the later record first.
//
// The curve over the sorted keys is five launches: tp counts per tile, their scan, precision / recall per record (fp64,
// contraction off) with the tile maxima, the suffix maxima of the tiles, and the right-to-left running maximum with the
// per-tile mAP terms; one workgroup then sums the tile terms in a fixed order (block_sum).
// Needs: geom_blocks.hip.h.
#pragma once

namespace sspk {

#define DET_BLOCK 1024
#define DET_CURVE_TILE 1024  // records per workgroup of the curve kernels (mirrored as lib.DET_CURVE_TILE)
#define DET_MAX_R2 64
#define DET_STATE_RECORDS 0
#define DET_STATE_NGT 1
#define DET_STATE_OVERFLOW 2
#define DET_STATE_OUTSIDE 3                           // point-list rows < count that lie outside the image (skipped)
#define DET_STATE_HIST 8                              // [DET_MAX_R2 + 1] counts of the minimum d2
#define DET_STATE_WORDS (DET_STATE_HIST + DET_MAX_R2 + 1 + 7)  // 80

struct DetParams {
  int H, W, r, r2, simplified, labels_u8;
  float remove_zero, prob_thresh;
};

__device__ __forceinline__ bool det_label(const void* __restrict__ labels, int u8, size_t idx) {
  return u8 ? reinterpret_cast<const uint8_t*>(labels)[idx] != 0 : reinterpret_cast<const float*>(labels)[idx] != 0.f;
}

// Exclusive SUFFIX maximum of v >= 0 over the workgroup's threads (0 for the last) and the workgroup maximum; lds: DET_BLOCK doubles.
__device__ __forceinline__ double det_block_suffix_max(double v, double* lds, double& total) {
  const int t = threadIdx.x;
  __syncthreads();
  lds[t] = v;
  __syncthreads();
  for (int o = 1; o < DET_BLOCK; o <<= 1) {
    const double u = t + o < DET_BLOCK ? lds[t + o] : 0.0;
    __syncthreads();
    lds[t] = fmax(lds[t], u);
    __syncthreads();
  }
  total = lds[0];
  return t + 1 < DET_BLOCK ? lds[t + 1] : 0.0;
}

struct DetItem {
  bool valid, outside;
  int b, pos, y, x;
  unsigned bits;
  float p;
};

// Slot e of the call: POINTS = false: pixel e of prob [B][H*W]; POINTS = true: row e of pts [B][cap][5] (x, y, confidence).
template <bool POINTS>
__device__ __forceinline__ DetItem det_item(const float* __restrict__ src, const int32_t* __restrict__ count, int n_items,
                                            const DetParams& P, long e, long total) {
  DetItem it;
  it.valid = it.outside = false;
  it.b = it.pos = it.y = it.x = 0;
  it.bits = 0u;
  it.p = 0.f;
  if (e >= total) return it;
  it.b = (int)(e / n_items);
  it.pos = (int)(e - (long)it.b * n_items);
  if (POINTS) {
    if (it.pos >= min(max(count[it.b], 0), n_items)) return it;
    const float* r = src + (size_t)e * 5;
    const float fx = r[0], fy = r[1];
    if (!(fx >= 0.f && fx < (float)P.W && fy >= 0.f && fy < (float)P.H)) {  // outside the image (or NaN): skipped and counted
      it.outside = true;
      return it;
    }
    it.x = (int)fx;
    it.y = (int)fy;
    it.p = r[2];
  } else {
    it.y = it.pos / P.W;
    it.x = it.pos - it.y * P.W;
    it.p = src[e];
  }
  it.valid = it.p > P.remove_zero;  // remove_zero >= 0: a candidate is positive, so its bits order like unsigned integers
  it.bits = __float_as_uint(it.p);
  return it;
}

__device__ __forceinline__ unsigned long long det_image_key(const DetItem& it) {
  return ((unsigned long long)it.bits << 32) | (unsigned)it.pos;
}

// gidx [total]: -2 no candidate, -1 candidate without a ground-truth point in range, else g (pixel index in its image)
template <bool POINTS>
__global__ __launch_bounds__(DET_BLOCK) void det_match_kernel(const float* __restrict__ src, const int32_t* __restrict__ count,
                                                              const void* __restrict__ labels, DetParams P, int n_items, long total,
                                                              unsigned long long* __restrict__ best, int32_t* __restrict__ gidx,
                                                              int32_t* __restrict__ block_sums,
                                                              unsigned long long* __restrict__ state) {
  __shared__ int wsum[DET_BLOCK / 64];
  const long e = (long)blockIdx.x * DET_BLOCK + threadIdx.x;
  const DetItem it = det_item<POINTS>(src, count, n_items, P, e, total);
  int g = -2;
  if (it.outside) atomicAdd(state + DET_STATE_OUTSIDE, 1ull);
  if (it.valid) {
    g = -1;
    const size_t img = (size_t)it.b * P.H * P.W;
    const bool loc = it.p > P.prob_thresh;
    int dmin = 0x7fffffff;
    const int y0 = max(it.y - P.r, 0), y1 = min(it.y + P.r, P.H - 1);
    const int x0 = max(it.x - P.r, 0), x1 = min(it.x + P.r, P.W - 1);
    const bool all = loc || P.simplified;  // the whole window: the minimum d2 / every label pixel in range (simplified n_gt)
    for (int yy = y0; yy <= y1 && (all || g < 0); ++yy) {
      const int dy2 = (yy - it.y) * (yy - it.y);
      for (int xx = x0; xx <= x1; ++xx) {
        const int d2 = dy2 + (xx - it.x) * (xx - it.x);
        if (d2 <= P.r2 && det_label(labels, P.labels_u8, img + (size_t)yy * P.W + xx)) {
          if (g < 0) g = yy * P.W + xx;
          dmin = min(dmin, d2);
          if (P.simplified) atomicMax(best + img + (size_t)yy * P.W + xx, 1ull);
          if (!all) break;
        }
      }
    }
    if (g >= 0) {
      if (!P.simplified) atomicMax(best + img + g, det_image_key(it));
      if (loc) atomicAdd(state + DET_STATE_HIST + dmin, 1ull);
    }
  }
  if (e < total) gidx[e] = g;
  int tot;
  block_scan<DET_BLOCK>(g != -2 ? 1 : 0, wsum, tot);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

// One workgroup: offs[k] = sums[0] + .. + sums[k-1], offs[nb] = the total.
__global__ __launch_bounds__(DET_BLOCK) void det_offsets_kernel(const int32_t* __restrict__ sums, int nb, int32_t* __restrict__ offs) {
  __shared__ int wsum[DET_BLOCK / 64];
  int carry = 0;
  for (int k0 = 0; k0 < nb; k0 += DET_BLOCK) {
    const int k = k0 + threadIdx.x;
    const int v = k < nb ? sums[k] : 0;
    int tot;
    const int ex = block_scan<DET_BLOCK>(v, wsum, tot);
    if (k < nb) offs[k] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) offs[nb] = carry;
}

template <bool POINTS>
__global__ __launch_bounds__(DET_BLOCK) void det_emit_kernel(const float* __restrict__ src, const int32_t* __restrict__ count,
                                                             DetParams P, int n_items, long total,
                                                             const unsigned long long* __restrict__ best,
                                                             const int32_t* __restrict__ gidx, const int32_t* __restrict__ block_offs,
                                                             unsigned long long* __restrict__ keys, long long capacity,
                                                             unsigned long long* __restrict__ state) {
  __shared__ int wsum[DET_BLOCK / 64];
  const long e = (long)blockIdx.x * DET_BLOCK + threadIdx.x;
  const DetItem it = det_item<POINTS>(src, count, n_items, P, e, total);
  const int g = e < total ? gidx[e] : -2;
  int tot;
  const int pos = block_offs[blockIdx.x] + block_scan<DET_BLOCK>(g != -2 ? 1 : 0, wsum, tot);
  if (g == -2) return;
  const long long rec = (long long)state[DET_STATE_RECORDS] + pos;  // (no kernel of this launch writes the word)
  if (rec >= capacity) {
    atomicMax(state + DET_STATE_OVERFLOW, 1ull);
    return;
  }
  bool tp = g >= 0;
  if (tp && !P.simplified) tp = best[(size_t)it.b * P.H * P.W + g] == det_image_key(it);
  keys[rec] = ((unsigned long long)it.bits << 32) | ((unsigned long long)rec << 1) | (tp ? 1ull : 0ull);
}

// grid over the B*H*W label pixels
__global__ __launch_bounds__(DET_BLOCK) void det_finish_kernel(const void* __restrict__ labels, DetParams P, long n_pix,
                                                               const unsigned long long* __restrict__ best,
                                                               const int32_t* __restrict__ block_offs, int nb_items,
                                                               unsigned long long* __restrict__ state) {
  __shared__ int wsum[DET_BLOCK / 64];
  const long e = (long)blockIdx.x * DET_BLOCK + threadIdx.x;
  bool f = false;
  if (e < n_pix) f = P.simplified ? best[e] != 0ull : det_label(labels, P.labels_u8, (size_t)e);
  int tot;
  block_scan<DET_BLOCK>(f ? 1 : 0, wsum, tot);
  if (threadIdx.x == 0) {
    if (tot) atomicAdd(state + DET_STATE_NGT, (unsigned long long)tot);
    if (blockIdx.x == 0) state[DET_STATE_RECORDS] += (unsigned long long)block_offs[nb_items];
  }
}

// ---- the curve over the sorted keys (descending) ----
__global__ __launch_bounds__(DET_BLOCK) void det_curve_count_kernel(const unsigned long long* __restrict__ keys, long long n,
                                                                    int32_t* __restrict__ block_sums) {
  __shared__ int wsum[DET_BLOCK / 64];
  const long long e = (long long)blockIdx.x * DET_CURVE_TILE + threadIdx.x;
  int tot;
  block_scan<DET_BLOCK>(e < n ? (int)(keys[e] & 1ull) : 0, wsum, tot);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

// precision / recall [n + 2]; precision holds the un-maximised tp_cum / (tp_cum + fp_cum) after this kernel
__global__ __launch_bounds__(DET_BLOCK) void det_curve_pr_kernel(const unsigned long long* __restrict__ keys, long long n,
                                                                 const unsigned long long* __restrict__ state,
                                                                 const int32_t* __restrict__ block_offs, float* __restrict__ prob,
                                                                 uint8_t* __restrict__ tp_out, double* __restrict__ precision,
                                                                 double* __restrict__ recall, double* __restrict__ block_max) {
#pragma clang fp contract(off)
  __shared__ int wsum[DET_BLOCK / 64];
  __shared__ double lds[DET_BLOCK];
  const long long e = (long long)blockIdx.x * DET_CURVE_TILE + threadIdx.x;
  const unsigned long long key = e < n ? keys[e] : 0ull;
  const int tp = (int)(key & 1ull);
  int tot;
  const long long tp_cum = (long long)block_offs[blockIdx.x] + block_scan<DET_BLOCK>(tp, wsum, tot) + tp;
  double raw = 0.0;
  if (e < n) {
    const long long n_gt = (long long)state[DET_STATE_NGT];
    raw = (double)tp_cum / (double)(e + 1);  // tp_cum + fp_cum = e + 1 > 0
    recall[e + 1] = n_gt != 0 ? (double)tp_cum / (double)n_gt : (tp_cum == 0 ? 1.0 : 0.0);  // div0
    precision[e + 1] = raw;
    prob[e] = __uint_as_float((unsigned)(key >> 32));
    tp_out[e] = (uint8_t)tp;
  }
  double bmax;
  det_block_suffix_max(raw, lds, bmax);
  if (threadIdx.x == 0) {
    block_max[blockIdx.x] = bmax;
    if (blockIdx.x == 0) {
      recall[0] = 0.0;
      recall[n + 1] = 1.0;
      precision[n + 1] = 0.0;
    }
  }
}

// One workgroup: suffix[k] = max(block_max[k+1 ..]) (0 for the last).
__global__ __launch_bounds__(DET_BLOCK) void det_suffix_blocks_kernel(const double* __restrict__ block_max, int nb,
                                                                      double* __restrict__ suffix) {
  __shared__ double lds[DET_BLOCK];
  double carry = 0.0;
  for (int c = (nb - 1) / DET_BLOCK; c >= 0; --c) {
    const int k = c * DET_BLOCK + threadIdx.x;
    const double v = k < nb ? block_max[k] : 0.0;
    double tot;
    const double ex = det_block_suffix_max(v, lds, tot);
    if (k < nb) suffix[k] = fmax(ex, carry);
    carry = fmax(carry, tot);
  }
}

// the right-to-left running maximum and the tile's share of sum(precision[1:] * (recall[1:] - recall[:-1]))
__global__ __launch_bounds__(DET_BLOCK) void det_curve_final_kernel(long long n, const double* __restrict__ suffix,
                                                                    const double* __restrict__ recall, double* __restrict__ precision,
                                                                    double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double lds[DET_BLOCK];
  const long long e = (long long)blockIdx.x * DET_CURVE_TILE + threadIdx.x;
  const double raw = e < n ? precision[e + 1] : 0.0;
  const double rest = n > 0 ? suffix[blockIdx.x] : 0.0;
  double tot;
  const double ex = det_block_suffix_max(raw, lds, tot);
  double term = 0.0;
  if (e < n) {
    const double fin = fmax(raw, fmax(ex, rest));
    precision[e + 1] = fin;
    term = fin * (recall[e + 1] - recall[e]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) precision[0] = fmax(tot, rest);
  const double s = block_sum<DET_BLOCK>(term, lds);  // (the term of the padded last element is 0 * (1 - recall[n]) = 0)
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(DET_BLOCK) void det_sum_kernel(const double* __restrict__ partial, int nb, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double lds[DET_BLOCK / 64];
  double v = 0.0;
  for (int k = threadIdx.x; k < nb; k += DET_BLOCK) v += partial[k];
  const double s = block_sum<DET_BLOCK>(v, lds);
  if (threadIdx.x == 0) out[0] = s;
}

}  // namespace sspk
