// Evaluation of descriptor exports (evaluation.py:86-500 of the reference): repeatability and localisation error
// (evaluations/detector_evaluation.py:153-275), the matching score's unwarped-point count (evaluation.py:194-219), and a
// RANSAC homography (the cv2.findHomography step of evaluations/descriptor_evaluation.py:65-158 and evaluation.py:224-330)
// with the average precision of evaluation.py:318-325 fused into its epilogue.  One workgroup per pair; fp64 throughout
// except the matching-score count, which keeps the reference's float32 warp.  Every function here is compiled with
// contraction off: the reference's numpy arithmetic rounds each product and each sum.  The sums over a workgroup or a wave
// (block_sum, wave_sum), the RANSAC key and the sampler are those of geom_blocks.hip.h.
// Needs: geom_blocks.hip.h.
#pragma once

namespace sspk {

#define EVAL_THREADS 256
#define EVAL_HYPOTHESES 2000
#define EVAL_GN_STEPS 5
#define EVAL_FLT_EPS 1.1920928955078125e-07

// np.dot([x, y, 1], M^T) followed by [:, :2] / [:, 2:] (warp_keypoints, detector_evaluation.py:139-150)
__device__ __forceinline__ void eval_warp(const double* M, double x, double y, double& u, double& v) {
#pragma clang fp contract(off)
  const double w0 = (x * M[0] + y * M[1]) + M[2];
  const double w1 = (x * M[3] + y * M[4]) + M[5];
  const double w2 = (x * M[6] + y * M[7]) + M[8];
  u = w0 / w2;
  v = w1 / w2;
}

// One block per pair.  pts: [P*pair_stride][cap][3] fp64 rows (x, y, confidence); pair p uses entry p * pair_stride of
// pts1 / n1 (the image) and of pts2 / n2 (the warped image).  hom / hom_inv: [P][9] (hom_inv = np.linalg.inv(hom) from
// the host).  out: [P][8] = N1, N2, count1, count2, sum1, sum2, n_unwarped, 0.
// Dynamic LDS: cap doubles (confidence keys) + 2 * kk double2 (the kept points of each side), kk = min(keep_k, cap).
__global__ __launch_bounds__(EVAL_THREADS) void eval_repeat_kernel(const double* __restrict__ pts1,
                                                                   const int32_t* __restrict__ n1_in,
                                                                   const double* __restrict__ pts2,
                                                                   const int32_t* __restrict__ n2_in, int cap,
                                                                   int pair_stride, const double* __restrict__ hom,
                                                                   const double* __restrict__ hom_inv, int height,
                                                                   int width, int kk, double thresh,
                                                                   double* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ double eval_dyn[];
  __shared__ int s_inside[2];
  __shared__ int s_count[2];
  __shared__ int s_unw;
  __shared__ double red[EVAL_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x, ps = p * pair_stride;
  double* key = eval_dyn;
  double2* kept[2] = {reinterpret_cast<double2*>(eval_dyn + ((cap + 1) & ~1)),
                      reinterpret_cast<double2*>(eval_dyn + ((cap + 1) & ~1)) + kk};
  double M[2][9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    M[0][k] = hom[(size_t)p * 9 + k];
    M[1][k] = hom_inv[(size_t)p * 9 + k];
  }
  if (tid < 2) s_inside[tid] = 0, s_count[tid] = 0;
  if (tid == 0) s_unw = 0;
  const double W = (double)width, Hh = (double)height;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    // side 0: the image's points warped by H (true_warped_keypoints); side 1: the warped image's points whose inv(H)
    // image is inside (keep_true_keypoints), at their own coordinates
    const double* P = (s == 0 ? pts1 : pts2) + (size_t)ps * cap * 3;
    const int n = min(s == 0 ? n1_in[ps] : n2_in[ps], cap);
    __syncthreads();
    int inside_local = 0;
    for (int i = tid; i < n; i += EVAL_THREADS) {
      double u, v;
      eval_warp(M[s], P[3 * i], P[3 * i + 1], u, v);
      const bool in = u >= 0.0 && u < W && v >= 0.0 && v < Hh;
      key[i] = in ? P[3 * i + 2] : -INFINITY;
      inside_local += in;
    }
    atomicAdd(&s_inside[s], inside_local);
    __syncthreads();
    // select_k_best: the kk most confident (ties: the lower index) go to the slot of their rank
    for (int i = tid; i < n; i += EVAL_THREADS) {
      const double ki = key[i];
      if (ki == -INFINITY) continue;
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const double kj = key[j];
        rank += (kj > ki) || (kj == ki && j < i);
      }
      if (rank < kk) {
        double u = P[3 * i], v = P[3 * i + 1];
        if (s == 0) eval_warp(M[0], P[3 * i], P[3 * i + 1], u, v);
        kept[s][rank] = make_double2(u, v);
      }
    }
  }
  // matching-score quirk (evaluation.py:194-216): warped_prob[:, [1, 0]] truncated to integers, warped by
  // float32(inv(H)) as if it were (x, y), kept when 0 <= p <= [W, H] - 1
  {
    const double* P = pts2 + (size_t)ps * cap * 3;
    const int n = min(n2_in[ps], cap);
    float F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = (float)M[1][k];
    const float wm1 = (float)width - 1.f, hm1 = (float)height - 1.f;
    int c = 0;
    for (int i = tid; i < n; i += EVAL_THREADS) {
      const float a = (float)(long long)P[3 * i + 1], b = (float)(long long)P[3 * i];
      const float w0 = (F[0] * a + F[1] * b) + F[2];
      const float w1 = (F[3] * a + F[4] * b) + F[5];
      const float w2 = (F[6] * a + F[7] * b) + F[8];
      const float u = __fdiv_rn(w0, w2), v = __fdiv_rn(w1, w2);
      c += (u >= 0.f && u <= wm1 && v >= 0.f && v <= hm1);
    }
    atomicAdd(&s_unw, c);
  }
  __syncthreads();
  const int N[2] = {min(s_inside[0], kk), min(s_inside[1], kk)};
  double sum[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    // row minima (s = 0) / column minima (s = 1) of ||a - b|| over the N1 x N2 pairs
    const double2* A = kept[s];
    const double2* B = kept[1 - s];
    const int na = N[s], nb = N[1 - s];
    double part = 0.0;
    int c = 0;
    if (nb > 0) {
      for (int i = tid; i < na; i += EVAL_THREADS) {
        const double2 a = A[i];
        double m = INFINITY;
        for (int j = 0; j < nb; ++j) {
          const double2 b = B[j];
          const double dx = a.x - b.x, dy = a.y - b.y;
          m = fmin(m, dx * dx + dy * dy);
        }
        const double d = sqrt(m);
        if (d <= thresh) {
          ++c;
          part = part + d;
        }
      }
    }
    atomicAdd(&s_count[s], c);
    sum[s] = block_sum<EVAL_THREADS>(part, red);
  }
  __syncthreads();
  if (tid == 0) {
    double* o = out + (size_t)p * 8;
    o[0] = (double)N[0];
    o[1] = (double)N[1];
    o[2] = (double)s_count[0];
    o[3] = (double)s_count[1];
    o[4] = sum[0];
    o[5] = sum[1];
    o[6] = (double)s_unw;
    o[7] = 0.0;
  }
}

// ---- RANSAC homography ----
__device__ __forceinline__ bool eval_collinear(double ax, double ay, double bx, double by, double cx, double cy) {
#pragma clang fp contract(off)
  const double dx1 = bx - ax, dy1 = by - ay, dx2 = cx - ax, dy2 = cy - ay;
  return fabs(dx2 * dy1 - dy2 * dx1) <= EVAL_FLT_EPS * (((fabs(dx1) + fabs(dy1)) + fabs(dx2)) + fabs(dy2));
}

// Solve the 8x8 system A h = b (A in a[r][0..7], b in a[r][8]) by Gaussian elimination: for every column k, row k is
// swapped with each later row whose |entry| is larger (so the pivot is the largest), then eliminated.  Fully unrolled
// with constant indices: the matrix lives in registers.  Returns false when a pivot is <= 1e-12 in magnitude.
__device__ __forceinline__ bool eval_solve8(double (&a)[8][9], double (&h)[8]) {
#pragma clang fp contract(off)
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int r = k + 1; r < 8; ++r) {
      const bool sw = fabs(a[r][k]) > fabs(a[k][k]);
#pragma unroll
      for (int c = k; c < 9; ++c) {
        const double t = a[k][c];
        a[k][c] = sw ? a[r][c] : t;
        a[r][c] = sw ? t : a[r][c];
      }
    }
    ok = ok && fabs(a[k][k]) > 1e-12;
    const double inv = 1.0 / a[k][k];
#pragma unroll
    for (int r = k + 1; r < 8; ++r) {
      const double f = a[r][k] * inv;
#pragma unroll
      for (int c = k + 1; c < 9; ++c) a[r][c] = a[r][c] - f * a[k][c];
    }
  }
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    double s = a[k][8];
#pragma unroll
    for (int c = k + 1; c < 8; ++c) s = s - a[k][c] * h[c];
    h[k] = s / a[k][k];
  }
  return ok;
}

// Normalisation of a point set: centroid and s = m / sum(|x - cx| + |y - cy|); t = (s, cx, cy).
struct EvalNorm {
  double s, cx, cy;
};

// Pixel homography of the normalised parameters hn (h33 = 1): inv(Tq) * Hn * Tp, scaled to H[8] = 1.
__device__ __forceinline__ void eval_denorm(const double (&hn)[8], EvalNorm tp, EvalNorm tq, double (&H)[9]) {
#pragma clang fp contract(off)
  // Hn * Tp, Tp = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
  const double hv[9] = {hn[0], hn[1], hn[2], hn[3], hn[4], hn[5], hn[6], hn[7], 1.0};
  const double ox = -(tp.s * tp.cx), oy = -(tp.s * tp.cy);
  double B[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    B[3 * r] = hv[3 * r] * tp.s;
    B[3 * r + 1] = hv[3 * r + 1] * tp.s;
    B[3 * r + 2] = (hv[3 * r] * ox + hv[3 * r + 1] * oy) + hv[3 * r + 2];
  }
  // inv(Tq) * B, inv(Tq) = [[1/s, 0, cx], [0, 1/s, cy], [0, 0, 1]]
  const double is = 1.0 / tq.s;
  double C[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    C[c] = B[c] * is + tq.cx * B[6 + c];
    C[3 + c] = B[3 + c] * is + tq.cy * B[6 + c];
    C[6 + c] = B[6 + c];
  }
  const double i8 = 1.0 / C[8];
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = C[k] * i8;
}

__device__ __forceinline__ double eval_resid2(const double (&H)[9], double4 m) {
#pragma clang fp contract(off)
  const double w = (H[6] * m.x + H[7] * m.y) + H[8];
  const double u = ((H[0] * m.x + H[1] * m.y) + H[2]) / w;
  const double v = ((H[3] * m.x + H[4] * m.y) + H[5]) / w;
  const double du = u - m.z, dv = v - m.w;
  return du * du + dv * dv;
}

// The normalised 4-point DLT of hypothesis h: samples 4 distinct indices, rejects a sample with 3 collinear points in
// either set, solves for h33 = 1.  Returns false for an invalid hypothesis.
__device__ __forceinline__ bool eval_hypothesis(const double4* M, int n, uint64_t seed, int h, double (&H)[9]) {
#pragma clang fp contract(off)
  int id[4];
  sample_distinct(seed, h, n, id, [](int) { return true; });  // (n == 4: the direct solve of exactly 4 matches)
  if (id[1] == id[0] || id[2] == id[0] || id[2] == id[1] || id[3] == id[0] || id[3] == id[1] || id[3] == id[2])
    return false;
  double4 q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = M[id[k]];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int a = t < 3 ? 0 : 1, b = t < 2 ? 1 : 2, d = t == 0 ? 2 : 3;  // (0,1,2) (0,1,3) (0,2,3) (1,2,3)
    if (eval_collinear(q[a].x, q[a].y, q[b].x, q[b].y, q[d].x, q[d].y)) return false;
    if (eval_collinear(q[a].z, q[a].w, q[b].z, q[b].w, q[d].z, q[d].w)) return false;
  }
  EvalNorm tp, tq;
  tp.cx = (((q[0].x + q[1].x) + q[2].x) + q[3].x) / 4.0;
  tp.cy = (((q[0].y + q[1].y) + q[2].y) + q[3].y) / 4.0;
  tq.cx = (((q[0].z + q[1].z) + q[2].z) + q[3].z) / 4.0;
  tq.cy = (((q[0].w + q[1].w) + q[2].w) + q[3].w) / 4.0;
  double sp = 0.0, sq = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sp = sp + (fabs(q[k].x - tp.cx) + fabs(q[k].y - tp.cy));
    sq = sq + (fabs(q[k].z - tq.cx) + fabs(q[k].w - tq.cy));
  }
  if (!(sp > 0.0) || !(sq > 0.0)) return false;
  tp.s = 4.0 / sp;
  tq.s = 4.0 / sq;
  double a[8][9];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = (q[k].x - tp.cx) * tp.s, y = (q[k].y - tp.cy) * tp.s;
    const double u = (q[k].z - tq.cx) * tq.s, v = (q[k].w - tq.cy) * tq.s;
    const double r0[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -(x * u), -(y * u), u};
    const double r1[9] = {0.0, 0.0, 0.0, x, y, 1.0, -(x * v), -(y * v), v};
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      a[2 * k][c] = r0[c];
      a[2 * k + 1][c] = r1[c];
    }
  }
  double hn[8];
  if (!eval_solve8(a, hn)) return false;
  eval_denorm(hn, tp, tq, H);
  return isfinite(H[0]) && isfinite(H[1]) && isfinite(H[2]) && isfinite(H[3]) && isfinite(H[4]) && isfinite(H[5]) &&
         isfinite(H[6]) && isfinite(H[7]);
}

// Wave 0 only: the normal equations over the inliers of `mask` in normalised coordinates.  geometric = false: the DLT rows
// (algebraic least squares; the solve of the step from h = 0 is the refit); true: the Jacobian of the forward transfer
// error at hn (one Gauss-Newton step).  Returns the sum of squared residuals; every lane ends with the same sums.
__device__ __forceinline__ double eval_normal_eq(const double4* M, const uint8_t* mask, int n, EvalNorm tp, EvalNorm tq,
                                                 bool geometric, const double (&hn)[8], double (&a)[8][9]) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  double cost = 0.0;
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 9; ++c) a[r][c] = 0.0;
  for (int i = lane; i < n; i += 64) {
    if (!mask[i]) continue;
    const double4 m = M[i];
    const double x = (m.x - tp.cx) * tp.s, y = (m.y - tp.cy) * tp.s;
    const double u = (m.z - tq.cx) * tq.s, v = (m.w - tq.cy) * tq.s;
    double j0[8], j1[8], r0, r1;
    if (geometric) {
      const double iw = 1.0 / ((hn[6] * x + hn[7] * y) + 1.0);
      const double px = ((hn[0] * x + hn[1] * y) + hn[2]) * iw, py = ((hn[3] * x + hn[4] * y) + hn[5]) * iw;
      const double xw = x * iw, yw = y * iw;
      j0[0] = xw; j0[1] = yw; j0[2] = iw; j0[3] = 0.0; j0[4] = 0.0; j0[5] = 0.0; j0[6] = -(xw * px); j0[7] = -(yw * px);
      j1[0] = 0.0; j1[1] = 0.0; j1[2] = 0.0; j1[3] = xw; j1[4] = yw; j1[5] = iw; j1[6] = -(xw * py); j1[7] = -(yw * py);
      r0 = px - u;
      r1 = py - v;
    } else {
      j0[0] = x; j0[1] = y; j0[2] = 1.0; j0[3] = 0.0; j0[4] = 0.0; j0[5] = 0.0; j0[6] = -(x * u); j0[7] = -(y * u);
      j1[0] = 0.0; j1[1] = 0.0; j1[2] = 0.0; j1[3] = x; j1[4] = y; j1[5] = 1.0; j1[6] = -(x * v); j1[7] = -(y * v);
      r0 = -u;
      r1 = -v;
    }
    cost = cost + (r0 * r0 + r1 * r1);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
      for (int c = r; c < 8; ++c) a[r][c] = a[r][c] + (j0[r] * j0[c] + j1[r] * j1[c]);
      a[r][8] = a[r][8] - (j0[r] * r0 + j1[r] * r1);
    }
  }
  cost = wave_sum(cost);
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = r; c < 9; ++c) a[r][c] = wave_sum(a[r][c]);
#pragma unroll
  for (int r = 1; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < r; ++c) a[r][c] = a[c][r];
  return cost;
}

__device__ __forceinline__ EvalNorm eval_norm_of(const double4* M, const uint8_t* mask, int n, bool dst) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  double sx = 0.0, sy = 0.0, cnt = 0.0;
  for (int i = lane; i < n; i += 64) {
    if (!mask[i]) continue;
    const double4 m = M[i];
    sx = sx + (dst ? m.z : m.x);
    sy = sy + (dst ? m.w : m.y);
    cnt = cnt + 1.0;
  }
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  cnt = wave_sum(cnt);
  EvalNorm t;
  t.cx = sx / cnt;
  t.cy = sy / cnt;
  double sa = 0.0;
  for (int i = lane; i < n; i += 64) {
    if (!mask[i]) continue;
    const double4 m = M[i];
    sa = sa + (fabs((dst ? m.z : m.x) - t.cx) + fabs((dst ? m.w : m.y) - t.cy));
  }
  t.s = cnt / wave_sum(sa);
  return t;
}

// Gathers the matched coordinates of each pair: xy[p][k] = (x1, y1, x2, y2) of match k (indices i, j of match row k).
__global__ __launch_bounds__(256) void eval_gather_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2,
                                                          int cap, int pair_stride, const float* __restrict__ match,
                                                          const int32_t* __restrict__ n_match, double4* __restrict__ xy) {
  const int p = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  const int n = min(n_match[p], cap);
  if (k >= n) return;
  const float* m = match + ((size_t)p * cap + k) * 3;
  const int i = min(max((int)m[0], 0), cap - 1), j = min(max((int)m[1], 0), cap - 1);
  const double* a = pts1 + ((size_t)p * pair_stride * cap + i) * 3;
  const double* b = pts2 + ((size_t)p * pair_stride * cap + j) * 3;
  double* o = reinterpret_cast<double*>(xy + (size_t)p * cap + k);
  o[0] = a[0];
  o[1] = a[1];
  o[2] = b[0];
  o[3] = b[1];
}

// One block per pair.  xy: [P][cap] from eval_gather_kernel; staged in LDS when use_lds (dynamic LDS: cap double4 + cap
// floats + cap bytes; otherwise cap floats + cap bytes and xy is read from global memory).  match[p][k][2] is the score
// (distance) of match k, used by the AP when ap != nullptr.
__global__ __launch_bounds__(EVAL_THREADS) void eval_ransac_kernel(const double4* __restrict__ xy,
                                                                   const float* __restrict__ match,
                                                                   const int32_t* __restrict__ n_match, int cap,
                                                                   const uint64_t* __restrict__ seeds, int use_lds,
                                                                   double* __restrict__ h_out, uint8_t* __restrict__ mask_out,
                                                                   int32_t* __restrict__ n_inl_out,
                                                                   int32_t* __restrict__ status_out,
                                                                   double* __restrict__ ap_out) {
#pragma clang fp contract(off)
  extern __shared__ double4 eval_dyn4[];
  __shared__ uint64_t best_key[EVAL_THREADS / 64];
  __shared__ int s_count;
  __shared__ double red[EVAL_THREADS / 64];
  __shared__ double s_h[8];
  __shared__ int s_refit;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(n_match[p], cap);
  const uint64_t seed = seeds[p];
  const double4* G = xy + (size_t)p * cap;
  double4* L = eval_dyn4;
  float* dist = reinterpret_cast<float*>(use_lds ? eval_dyn4 + cap : eval_dyn4);
  uint8_t* mask = reinterpret_cast<uint8_t*>(dist + cap);
  for (int i = tid; i < n; i += EVAL_THREADS) {
    if (use_lds) L[i] = G[i];
    dist[i] = match[((size_t)p * cap + i) * 3 + 2];
  }
  const double4* M = use_lds ? L : G;
  __syncthreads();
  double H[9];
  bool valid = false;
  if (n == 4) {
    valid = eval_hypothesis(M, 4, seed, 0, H);
  } else if (n > 4) {
    // hypotheses tid, tid + 256, ...: score = #(residual^2 <= 9); best = max score, then the lowest index
    uint64_t key = 0;
    for (int h = tid; h < EVAL_HYPOTHESES; h += EVAL_THREADS) {
      double Hh[9];
      if (!eval_hypothesis(M, n, seed, h, Hh)) continue;
      int sc = 0;
      for (int i = 0; i < n; ++i) sc += eval_resid2(Hh, M[i]) <= 9.0;
      const uint64_t k = key_of(sc, h);
      key = k > key ? k : key;
    }
    publish_wave_keys(key, best_key);
    key = max_wave_key<EVAL_THREADS>(best_key);
    if (key != 0) valid = eval_hypothesis(M, n, seed, hypothesis_of(key), H);
  }
  // the best hypothesis's inlier set (n == 4: all four)
  if (tid == 0) s_count = 0, s_refit = 0;
  __syncthreads();
  int c = 0;
  for (int i = tid; i < n; i += EVAL_THREADS) {
    const bool in = valid && (n == 4 || eval_resid2(H, M[i]) <= 9.0);
    mask[i] = in;
    c += in;
  }
  atomicAdd(&s_count, c);
  __syncthreads();
  const int cnt = s_count;
  // refit: algebraic least squares on the inliers, then Gauss-Newton steps on the forward transfer error (wave 0)
  if (valid && n > 4 && cnt >= 4 && wave == 0) {
    const EvalNorm tp = eval_norm_of(M, mask, n, false), tq = eval_norm_of(M, mask, n, true);
    if (tp.s > 0.0 && isfinite(tp.s) && tq.s > 0.0 && isfinite(tq.s)) {
      double a[8][9], h[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) h[k] = 0.0;
      eval_normal_eq(M, mask, n, tp, tq, false, h, a);
      bool ok = eval_solve8(a, h);
      if (ok) {
        double cost = eval_normal_eq(M, mask, n, tp, tq, true, h, a);
        for (int it = 0; it < EVAL_GN_STEPS; ++it) {
          double d[8], hn[8], an[8][9];
          if (!eval_solve8(a, d)) break;
#pragma unroll
          for (int k = 0; k < 8; ++k) hn[k] = h[k] + d[k];
          const double cn = eval_normal_eq(M, mask, n, tp, tq, true, hn, an);
          if (!(cn < cost)) break;
          cost = cn;
#pragma unroll
          for (int k = 0; k < 8; ++k) h[k] = hn[k];
#pragma unroll
          for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int q = 0; q < 9; ++q) a[r][q] = an[r][q];
        }
        double Hr[9];
        eval_denorm(h, tp, tq, Hr);
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) fin = fin && isfinite(Hr[k]);
        if (fin && lane == 0) {
#pragma unroll
          for (int k = 0; k < 8; ++k) s_h[k] = Hr[k];
          s_refit = 1;
        }
      }
    }
  }
  __syncthreads();
  if (s_refit) {
#pragma unroll
    for (int k = 0; k < 8; ++k) H[k] = s_h[k];
    H[8] = 1.0;
  }
  // AP (sklearn average_precision_score of the mask against max(d) - d): sum over the inliers i of
  // tp(d <= d_i) / n(d <= d_i), divided by the inlier count; the same terms as -sum(diff(recall) * precision[:-1])
  double ap = 0.0;
  if (ap_out != nullptr) {
    double part = 0.0;
    if (cnt > 0) {
      for (int i = tid; i < n; i += EVAL_THREADS) {
        if (!mask[i]) continue;
        const float di = dist[i];
        int all = 0, tp = 0;
        for (int j = 0; j < n; ++j) {
          const bool le = dist[j] <= di;
          all += le;
          tp += le && mask[j];
        }
        part = part + (double)tp / (double)all;
      }
    }
    ap = block_sum<EVAL_THREADS>(part, red) / (double)(cnt > 0 ? cnt : 1);
  }
  uint8_t* mo = mask_out + (size_t)p * cap;
  for (int i = tid; i < cap; i += EVAL_THREADS) mo[i] = i < n ? mask[i] : 0;
  if (tid == 0) {
    double* ho = h_out + (size_t)p * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) ho[k] = valid ? H[k] : (k % 4 == 0 ? 1.0 : 0.0);
    n_inl_out[p] = valid ? cnt : 0;
    status_out[p] = valid ? 0 : 1;
    if (ap_out != nullptr) ap_out[p] = (valid && cnt > 0) ? ap : 0.0;
  }
}

// ---- streamed descriptor metrics ----
#define EVAL_ACC_MAX_PAIRS 128
#define EVAL_ROW_WORDS 16
#define EVAL_STATE_WORDS 16

// One lane per pair: the trainer's normalised homography hn (float32, image -> warped image in [-1, 1]^2) to pixels,
// M = Tinv @ (Hn @ T) (utils/utils.py:291-294 homography_scaling in closed form, no division by h33), and its inverse
// adj(M) / det(M).  The inverse is the adjugate, NOT np.linalg.inv's LU solve: the two differ in the last places.
__global__ __launch_bounds__(64) void eval_pixel_hom_kernel(const float* __restrict__ hn, int n_pairs, int height, int width,
                                                            double* __restrict__ hom, double* __restrict__ hom_inv) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n_pairs) return;
  const double W = (double)width, Hh = (double)height;
  const double T[9] = {2.0 / W, 0.0, -1.0, 0.0, 2.0 / Hh, -1.0, 0.0, 0.0, 1.0};
  const double Ti[9] = {W * 0.5, 0.0, W * 0.5, 0.0, Hh * 0.5, Hh * 0.5, 0.0, 0.0, 1.0};
  double h[9], b[9], m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = (double)hn[(size_t)p * 9 + k];
  mat3_mul(h, T, b);
  mat3_mul(Ti, b, m);
  double a[9];
  a[0] = m[4] * m[8] - m[5] * m[7];
  a[1] = m[2] * m[7] - m[1] * m[8];
  a[2] = m[1] * m[5] - m[2] * m[4];
  a[3] = m[5] * m[6] - m[3] * m[8];
  a[4] = m[0] * m[8] - m[2] * m[6];
  a[5] = m[2] * m[3] - m[0] * m[5];
  a[6] = m[3] * m[7] - m[4] * m[6];
  a[7] = m[1] * m[6] - m[0] * m[7];
  a[8] = m[0] * m[4] - m[1] * m[3];
  const double det = (m[0] * a[0] + m[1] * a[3]) + m[2] * a[6];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    hom[(size_t)p * 9 + k] = m[k];
    hom_inv[(size_t)p * 9 + k] = a[k] / det;
  }
}

struct EvalThresholds {
  double t[6];
};

// Mean distance of the four corners of (corner_h, corner_w) under H and under G (compute_homography,
// descriptor_evaluation.py:127-149): corners (0, 0), (0, h - 1), (w - 1, 0), (w - 1, h - 1) as (x, y).
__device__ __forceinline__ double eval_corner_dist(const double* H, const double* G, int corner_h, int corner_w) {
#pragma clang fp contract(off)
  const double xs[2] = {0.0, (double)(corner_w - 1)}, ys[2] = {0.0, (double)(corner_h - 1)};
  double d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double x = xs[k >> 1], y = ys[k & 1];
    double eu, ev, gu, gv;
    eval_warp(H, x, y, eu, ev);
    eval_warp(G, x, y, gu, gv);
    const double dx = gu - eu, dy = gv - ev;
    d[k] = sqrt(dx * dx + dy * dy);
  }
  return (((d[0] + d[1]) + d[2]) + d[3]) / 4.0;
}

// One workgroup of EVAL_ACC_MAX_PAIRS lanes; lane p forms the row of pair p (evaluation.rep_from_counts, correctness_of
// and the mscore / mAP lines of Evaluator.run_points), then lane 0 adds the rows into the state in pair order, so the state
// is the same sequence of fp64 additions however a set is split into calls.  rep == nullptr: repeatability off (and
// n_unwarped = 0); h_est == nullptr: the homography metrics are off; the slots of a group that is off stay 0.
__global__ __launch_bounds__(EVAL_ACC_MAX_PAIRS) void eval_accumulate_kernel(
    const double* __restrict__ rep, const double* __restrict__ h_est, const int32_t* __restrict__ n_inl,
    const int32_t* __restrict__ status, const double* __restrict__ ap, const int32_t* __restrict__ n1, int pair_stride,
    const double* __restrict__ hom, int n_pairs, int corner_h, int corner_w, EvalThresholds thr, long long first_pair,
    double* __restrict__ rows, long long capacity, double* __restrict__ state) {
#pragma clang fp contract(off)
  __shared__ double s_row[EVAL_ACC_MAX_PAIRS][EVAL_ROW_WORDS + 1];
  const int p = threadIdx.x;
  if (p < n_pairs) {
    double r[EVAL_ROW_WORDS];
#pragma unroll
    for (int k = 0; k < EVAL_ROW_WORDS; ++k) r[k] = 0.0;
    double n_unw = 0.0;
    if (rep != nullptr) {
      const double* q = rep + (size_t)p * 8;
      const long long c = (long long)q[2] + (long long)q[3];
      if (c == 0) {
        r[1] = -1.0;
      } else {
        const double cd = (double)c;
        r[0] = cd / (double)((long long)q[0] + (long long)q[1]);
        r[1] = (0.0 + q[4] / cd) + q[5] / cd;
      }
      n_unw = q[6];
    }
    if (h_est != nullptr) {
      const int st = status[p], inl = n_inl[p], np1 = n1[(size_t)p * pair_stride];
      double mean = INFINITY;
      if (st == 0) {
        mean = eval_corner_dist(h_est + (size_t)p * 9, hom + (size_t)p * 9, corner_h, corner_w);
#pragma unroll
        for (int k = 0; k < 6; ++k) r[2 + k] = mean <= thr.t[k] ? 1.0 : 0.0;
      }
      const double den = (double)((long long)np1 + (long long)n_unw);
      r[8] = den > 0.0 ? (double)(2 * (long long)inl) / den : 0.0;
      const double a = ap[p];
      r[9] = a > 0.0 ? a : 0.0;
      r[10] = (double)st;
      r[11] = (double)inl;
      r[12] = (double)np1;
      r[13] = n_unw;
      r[14] = mean;
    }
    r[15] = (double)(first_pair + p);
#pragma unroll
    for (int k = 0; k < EVAL_ROW_WORDS; ++k) s_row[p][k] = r[k];
    if (first_pair + p < capacity) {
      double* o = rows + (size_t)(first_pair + p) * EVAL_ROW_WORDS;
#pragma unroll
      for (int k = 0; k < EVAL_ROW_WORDS; ++k) o[k] = r[k];
    }
  }
  __syncthreads();
  if (p == 0) {
    double s[EVAL_STATE_WORDS];
#pragma unroll
    for (int k = 0; k < EVAL_STATE_WORDS; ++k) s[k] = state[k];
    for (int i = 0; i < n_pairs; ++i) {
      const double* r = s_row[i];
      s[0] = s[0] + 1.0;
      s[1] = s[1] + r[0];
      if (r[1] > 0.0) {
        s[2] = s[2] + r[1];
        s[3] = s[3] + 1.0;
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) s[4 + k] = s[4 + k] + r[2 + k];
      s[10] = s[10] + r[8];
      s[11] = s[11] + r[9];
      if (r[10] != 0.0) s[12] = s[12] + 1.0;
      if (first_pair + i >= capacity) s[13] = s[13] + 1.0;
    }
#pragma unroll
    for (int k = 0; k < EVAL_STATE_WORDS; ++k) state[k] = s[k];
  }
}

}  // namespace sspk
