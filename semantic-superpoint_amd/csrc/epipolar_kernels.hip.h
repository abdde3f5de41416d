// Epipolar check of matches: a fundamental-matrix RANSAC whose 2000 hypotheses of a pair are split
// over several workgroups, and the compaction of the match rows by its mask.  b^T F a = 0 for match (a = pts1[i],
// b = pts2[j]).  The rules are restated in numpy by tests/epipolar_ref.py; everything here is fp64 with contraction off,
// in the parenthesisation of that file.
//   epi_hypotheses_kernel  grid (groups, pairs): workgroup g solves and scores a contiguous slice of the hypotheses over
//                          the pair's matches staged in LDS and writes one (score, hypothesis) key
//   epi_finish_kernel      grid (pairs): the winner over the keys (a maximum: no order to depend on), its mask, the refit on
//                          the inliers with fixed-order sums, the Jacobi rank-2 step, the outputs
//   match_filter_kernel    grid (pairs): stable compaction of the match rows by the mask (wave ballots, no atomic ticket)
// The 8x9 system of a hypothesis lives in registers: every swap of the complete pivoting (pivot_step, geom_blocks.hip.h) is a
// compare-select with constant indices, as in eval_solve8.
// Needs: geom_blocks.hip.h, track_kernels.hip.h (TRACK_BLOCK), eval_kernels.hip.h (EvalNorm, eval_solve8, EVAL_HYPOTHESES).
#pragma once

namespace sspk {

#define EPI_THREADS 256
#define EPI_MAX_GROUPS 64
#define EPI_MIN_SCORE 8
#define EPI_JACOBI_SWEEPS 8

// Matches of pair p -> LDS rows (ax, ay, bx, by).  Indices are clamped to the arrays, as eval_gather_kernel does.
__device__ __forceinline__ void epi_stage(const double* __restrict__ pts1, const double* __restrict__ pts2, int pt_stride,
                                          int cap, const float* __restrict__ match, int n, double4* L) {
  for (int k = threadIdx.x; k < n; k += EPI_THREADS) {
    const float* m = match + (size_t)k * 3;
    const int i = min(max((int)m[0], 0), cap - 1), j = min(max((int)m[1], 0), cap - 1);
    const double* a = pts1 + (size_t)i * pt_stride;
    const double* b = pts2 + (size_t)j * pt_stride;
    L[k] = make_double4(a[0], a[1], b[0], b[1]);
  }
}

// F = T2^T Fn T1, T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
__device__ __forceinline__ void epi_denorm(const double (&fn)[9], EvalNorm t1, EvalNorm t2, double (&F)[9]) {
#pragma clang fp contract(off)
  const double o1x = -(t1.s * t1.cx), o1y = -(t1.s * t1.cy);
  const double o2x = -(t2.s * t2.cx), o2y = -(t2.s * t2.cy);
  double B[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    B[3 * r] = fn[3 * r] * t1.s;
    B[3 * r + 1] = fn[3 * r + 1] * t1.s;
    B[3 * r + 2] = (fn[3 * r] * o1x + fn[3 * r + 1] * o1y) + fn[3 * r + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    F[c] = t2.s * B[c];
    F[3 + c] = t2.s * B[3 + c];
    F[6 + c] = (o2x * B[c] + o2y * B[3 + c]) + B[6 + c];
  }
}

// T2^-T F T1^-1, T^-1 = [[1/s, 0, cx], [0, 1/s, cy], [0, 0, 1]]
__device__ __forceinline__ void epi_carry(const double (&F)[9], EvalNorm t1, EvalNorm t2, double (&G)[9]) {
#pragma clang fp contract(off)
  const double i1 = 1.0 / t1.s, i2 = 1.0 / t2.s;
  double B[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    B[3 * r] = F[3 * r] * i1;
    B[3 * r + 1] = F[3 * r + 1] * i1;
    B[3 * r + 2] = (F[3 * r] * t1.cx + F[3 * r + 1] * t1.cy) + F[3 * r + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    G[c] = i2 * B[c];
    G[3 + c] = i2 * B[3 + c];
    G[6 + c] = (t2.cx * B[c] + t2.cy * B[3 + c]) + B[6 + c];
  }
}

__device__ __forceinline__ void epi_row(double ax, double ay, double bx, double by, double (&r)[9]) {
#pragma clang fp contract(off)
  r[0] = bx * ax; r[1] = bx * ay; r[2] = bx;
  r[3] = by * ax; r[4] = by * ay; r[5] = by;
  r[6] = ax; r[7] = ay; r[8] = 1.0;
}

// Null vector of the 8x9 matrix a by Gaussian elimination with complete pivoting: at step k the pivot is the largest
// |entry| of rows k..7, columns k..8 (row-major scan with a strict comparison: the lowest row, then the lowest column);
// rows and columns are swapped; the unknown of the column left over is 1; back substitution; the column permutation is
// undone.  Constant indices throughout: the matrix lives in registers.  Returns false when a pivot is <= 1e-12 in
// magnitude (or NaN).
__device__ __forceinline__ bool epi_null8x9(double (&a)[8][9], double (&f)[9]) {
#pragma clang fp contract(off)
  bool ok = true;
  int perm[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) perm[c] = c;
  pivot_step<0>(a, perm, ok, 1e-12);
  pivot_step<1>(a, perm, ok, 1e-12);
  pivot_step<2>(a, perm, ok, 1e-12);
  pivot_step<3>(a, perm, ok, 1e-12);
  pivot_step<4>(a, perm, ok, 1e-12);
  pivot_step<5>(a, perm, ok, 1e-12);
  pivot_step<6>(a, perm, ok, 1e-12);
  pivot_step<7>(a, perm, ok, 1e-12);
  double x[9];
  x[8] = 1.0;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    double s = a[k][8];
#pragma unroll
    for (int c = k + 1; c < 8; ++c) s = s + a[k][c] * x[c];
    x[k] = -s / a[k][k];
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) v = perm[c] == j ? x[c] : v;
    f[j] = v;
  }
  return ok;
}

// Hypothesis h of a pair: 8 distinct matches from the counter-based stream (sample_distinct), both
// images normalised over the 8 points, the null vector of the 8x9 system, F in pixels.  false = invalid.
__device__ __forceinline__ bool epi_hypothesis(const double4* M, int n, uint64_t seed, int h, double (&F)[9]) {
#pragma clang fp contract(off)
  int id[8];
  sample_distinct(seed, h, n, id, [](int) { return true; });
  bool distinct = true;
#pragma unroll
  for (int k = 1; k < 8; ++k)
#pragma unroll
    for (int j = 0; j < k; ++j) distinct = distinct && id[k] != id[j];
  if (!distinct) return false;
  double4 q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = M[id[k]];
  double sx = q[0].x, sy = q[0].y, sz = q[0].z, sw = q[0].w;
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    sx = sx + q[k].x;
    sy = sy + q[k].y;
    sz = sz + q[k].z;
    sw = sw + q[k].w;
  }
  EvalNorm t1, t2;
  t1.cx = sx / 8.0;
  t1.cy = sy / 8.0;
  t2.cx = sz / 8.0;
  t2.cy = sw / 8.0;
  double sp = 0.0, sq = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    sp = sp + (fabs(q[k].x - t1.cx) + fabs(q[k].y - t1.cy));
    sq = sq + (fabs(q[k].z - t2.cx) + fabs(q[k].w - t2.cy));
  }
  if (!(sp > 0.0) || !(sq > 0.0)) return false;
  t1.s = 8.0 / sp;
  t2.s = 8.0 / sq;
  double a[8][9];
#pragma unroll
  for (int k = 0; k < 8; ++k)
    epi_row((q[k].x - t1.cx) * t1.s, (q[k].y - t1.cy) * t1.s, (q[k].z - t2.cx) * t2.s, (q[k].w - t2.cy) * t2.s, a[k]);
  double fn[9];
  if (!epi_null8x9(a, fn)) return false;
  epi_denorm(fn, t1, t2, F);
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) fin = fin && isfinite(F[k]);
  return fin;
}

// Squared Sampson distance e^2 / (l0^2 + l1^2 + m0^2 + m1^2), l = F a~, m = F^T b~, e = b~ . l; usable = the
// denominator is finite and positive.
__device__ __forceinline__ double epi_sampson2(const double (&F)[9], double4 m, bool& usable) {
#pragma clang fp contract(off)
  const double l0 = (F[0] * m.x + F[1] * m.y) + F[2];
  const double l1 = (F[3] * m.x + F[4] * m.y) + F[5];
  const double l2 = (F[6] * m.x + F[7] * m.y) + F[8];
  const double m0 = (F[0] * m.z + F[3] * m.w) + F[6];
  const double m1 = (F[1] * m.z + F[4] * m.w) + F[7];
  const double e = (m.z * l0 + m.w * l1) + l2;
  const double den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
  usable = isfinite(den) && den > 0.0;
  return (e * e) / den;
}

__device__ __forceinline__ bool epi_inlier(const double (&F)[9], double4 m, double t2) {
  bool usable;
  const double d2 = epi_sampson2(F, m, usable);
  return usable && d2 <= t2;
}

// Hypotheses tried for n matches: none below 8, the one direct solve at 8, EVAL_HYPOTHESES above.
__device__ __forceinline__ int epi_total(int n) { return n < 8 ? 0 : (n == 8 ? 1 : EVAL_HYPOTHESES); }

// grid (groups, pairs).  keys [pairs][groups]: key_of(score, h) of the best valid hypothesis of the
// slice [g * per, (g + 1) * per), per = ceil(EVAL_HYPOTHESES / groups); 0 = none.  Dynamic LDS: cap double4.
__global__ __launch_bounds__(EPI_THREADS) void epi_hypotheses_kernel(const double* __restrict__ pts1,
                                                                     const double* __restrict__ pts2, int pt_stride, int cap,
                                                                     int pair_stride, const float* __restrict__ match,
                                                                     const int32_t* __restrict__ n_match,
                                                                     const uint64_t* __restrict__ seeds, double thresh,
                                                                     uint64_t* __restrict__ keys) {
#pragma clang fp contract(off)
  extern __shared__ double4 epi_dyn4[];
  __shared__ uint64_t best_key[EPI_THREADS / 64];
  const int g = blockIdx.x, groups = gridDim.x, p = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(n_match[p], 0), cap);
  const int per = (EVAL_HYPOTHESES + groups - 1) / groups;
  const int lo = g * per, hi = min(lo + per, epi_total(n));
  if (lo >= hi) {  // (uniform over the workgroup)
    if (tid == 0) keys[(size_t)p * groups + g] = 0;
    return;
  }
  double4* M = epi_dyn4;
  epi_stage(pts1 + (size_t)p * pair_stride * cap * pt_stride, pts2 + (size_t)p * pair_stride * cap * pt_stride, pt_stride,
            cap, match + (size_t)p * cap * 3, n, M);
  __syncthreads();
  const uint64_t seed = seeds[p];
  const double t2 = thresh * thresh;
  uint64_t key = 0;
  for (int h = lo + tid; h < hi; h += EPI_THREADS) {
    double F[9];
    if (!epi_hypothesis(M, n, seed, h, F)) continue;
    int sc = 0;
    for (int i = 0; i < n; ++i) sc += epi_inlier(F, M[i], t2);
    // key_of and, below, publish_wave_keys / max_wave_key (geom_blocks.hip.h), written out: the same rules, keep them in step
    const uint64_t k = ((uint64_t)(sc + 1) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)h);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t t = __shfl_xor((unsigned long long)key, o);
    key = t > key ? t : key;
  }
  if ((tid & 63) == 0) best_key[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
    key = best_key[0];
#pragma unroll
    for (int w = 1; w < EPI_THREADS / 64; ++w) key = best_key[w] > key ? best_key[w] : key;
    keys[(size_t)p * groups + g] = key;
  }
}

// Normalisation of the inliers of one image (dst = false: a, true: b); sums in block_sum's fixed order.
__device__ __forceinline__ EvalNorm epi_norm_of(const double4* M, const uint8_t* mask, int n, double cnt, bool dst, double* red) {
#pragma clang fp contract(off)
  double sx = 0.0, sy = 0.0;
  for (int i = threadIdx.x; i < n; i += EPI_THREADS) {
    if (!mask[i]) continue;
    const double4 m = M[i];
    sx = sx + (dst ? m.z : m.x);
    sy = sy + (dst ? m.w : m.y);
  }
  EvalNorm t;
  t.cx = block_sum<EPI_THREADS>(sx, red) / cnt;
  t.cy = block_sum<EPI_THREADS>(sy, red) / cnt;
  double sa = 0.0;
  for (int i = threadIdx.x; i < n; i += EPI_THREADS) {
    if (!mask[i]) continue;
    const double4 m = M[i];
    sa = sa + (fabs((dst ? m.z : m.x) - t.cx) + fabs((dst ? m.w : m.y) - t.cy));
  }
  t.s = cnt / block_sum<EPI_THREADS>(sa, red);
  return t;
}

// Fn - (Fn v) v^T, v = the eigenvector of Fn^T Fn of the smallest eigenvalue, by 8 sweeps of cyclic Jacobi.
__device__ __forceinline__ void epi_rank2(double (&f)[9]) {
#pragma clang fp contract(off)
  double G[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      G[i][j] = (f[i] * f[j] + f[3 + i] * f[3 + j]) + f[6 + i] * f[6 + j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < EPI_JACOBI_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(G, V);
    jacobi_rotate<0, 2>(G, V);
    jacobi_rotate<1, 2>(G, V);
  }
  const bool k1 = G[1][1] < G[0][0];
  const double d01 = k1 ? G[1][1] : G[0][0];
  const bool k2 = G[2][2] < d01;
  double v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = k2 ? V[k][2] : (k1 ? V[k][1] : V[k][0]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double w = (f[3 * r] * v[0] + f[3 * r + 1] * v[1]) + f[3 * r + 2] * v[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) f[3 * r + c] = f[3 * r + c] - w * v[c];
  }
}

// Index of the largest |entry| (the lowest index on ties).
__device__ __forceinline__ int epi_argmax_abs(const double (&v)[9]) {
  int k = 0;
  double best = fabs(v[0]);
#pragma unroll
  for (int j = 1; j < 9; ++j) {
    const bool g = fabs(v[j]) > best;
    best = g ? fabs(v[j]) : best;
    k = g ? j : k;
  }
  return k;
}

// grid (pairs).  Dynamic LDS: cap double4 + cap bytes.  winner_out / err_out may be null.
__global__ __launch_bounds__(EPI_THREADS) void epi_finish_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2,
                                                                 int pt_stride, int cap, int pair_stride,
                                                                 const float* __restrict__ match,
                                                                 const int32_t* __restrict__ n_match,
                                                                 const uint64_t* __restrict__ seeds, double thresh, int groups,
                                                                 const uint64_t* __restrict__ keys, double* __restrict__ f_out,
                                                                 uint8_t* __restrict__ mask_out, int32_t* __restrict__ n_inl_out,
                                                                 int32_t* __restrict__ status_out,
                                                                 int32_t* __restrict__ winner_out, double* __restrict__ err_out) {
#pragma clang fp contract(off)
  extern __shared__ double4 epi_dyn4[];
  __shared__ double red[EPI_THREADS / 64];
  __shared__ double s_mom[9][9];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(n_match[p], 0), cap);
  double4* M = epi_dyn4;
  uint8_t* mask = reinterpret_cast<uint8_t*>(epi_dyn4 + cap);
  uint8_t* mo = mask_out + (size_t)p * cap;
  const uint64_t seed = seeds[p];
  const double t2 = thresh * thresh;
  const uint64_t key = max_group_key(keys, p, groups);
  const int winner = hypothesis_of(key);
  bool valid = key != 0 && score_of(key) >= EPI_MIN_SCORE;  // (uniform over the workgroup)
  double F[9], Fd[9];
  double cnt = 0.0, err = 0.0;
  if (valid) {
    epi_stage(pts1 + (size_t)p * pair_stride * cap * pt_stride, pts2 + (size_t)p * pair_stride * cap * pt_stride, pt_stride,
              cap, match + (size_t)p * cap * 3, n, M);
    __syncthreads();
    valid = epi_hypothesis(M, n, seed, winner, F);
  }
  if (valid) {
    double c = 0.0;
    for (int i = tid; i < n; i += EPI_THREADS) {
      const bool in = epi_inlier(F, M[i], t2);
      mask[i] = in;
      c = c + (in ? 1.0 : 0.0);
    }
    cnt = block_sum<EPI_THREADS>(c, red);  // (the barriers inside also publish the mask)
    EvalNorm t1 = epi_norm_of(M, mask, n, cnt, false, red), tq = epi_norm_of(M, mask, n, cnt, true, red);
    if (!(isfinite(t1.s) && t1.s > 0.0 && isfinite(tq.s) && tq.s > 0.0)) {
      t1.s = tq.s = 1.0;
      t1.cx = t1.cy = tq.cx = tq.cy = 0.0;
    }
    double G[9];
    epi_carry(F, t1, tq, G);
    const int ks = epi_argmax_abs(G);
    // moments sum(a_j a_k), j <= k, of the epipolar rows over the inliers
    double mom[45];
#pragma unroll
    for (int e = 0; e < 45; ++e) mom[e] = 0.0;
    for (int i = tid; i < n; i += EPI_THREADS) {
      if (!mask[i]) continue;
      const double4 m = M[i];
      double r[9];
      epi_row((m.x - t1.cx) * t1.s, (m.y - t1.cy) * t1.s, (m.z - tq.cx) * tq.s, (m.w - tq.cy) * tq.s, r);
      int e = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int k = j; k < 9; ++k, ++e) mom[e] = mom[e] + r[j] * r[k];
    }
    {
      int e = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int k = j; k < 9; ++k, ++e) {
          const double s = block_sum<EPI_THREADS>(mom[e], red);
          if (tid == 0) s_mom[j][k] = s_mom[k][j] = s;
        }
    }
    __syncthreads();
    // f[ks] = 1: the other eight entries from the 8x8 normal equations (unknown r is entry r + (r >= ks))
    double a[8][9], gsol[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int jr = r + (r >= ks);
#pragma unroll
      for (int c = 0; c < 8; ++c) a[r][c] = s_mom[jr][c + (c >= ks)];
      a[r][8] = -s_mom[jr][ks];
    }
    bool ok = eval_solve8(a, gsol);
#pragma unroll
    for (int r = 0; r < 8; ++r) ok = ok && isfinite(gsol[r]);
    double fn[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      // entry j is unknown j - (j > ks); unknowns j - 1 and j are the only candidates
      const double lo_v = j > 0 ? gsol[j > 0 ? j - 1 : 0] : 0.0, hi_v = j < 8 ? gsol[j < 8 ? j : 7] : 0.0;
      const double v = j == ks ? 1.0 : (j > ks ? lo_v : hi_v);
      fn[j] = ok ? v : G[j];
    }
    epi_rank2(fn);
    epi_denorm(fn, t1, tq, Fd);
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) ss = ss + Fd[k] * Fd[k];
    const double nrm = sqrt(ss);
    valid = isfinite(nrm) && nrm > 0.0;
    if (valid) {
#pragma unroll
      for (int k = 0; k < 9; ++k) Fd[k] = Fd[k] / nrm;
      const int kb = epi_argmax_abs(Fd);
      double big = Fd[0];
#pragma unroll
      for (int k = 1; k < 9; ++k) big = kb == k ? Fd[k] : big;
      if (big < 0.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) Fd[k] = -Fd[k];
      }
      double part = 0.0;
      for (int i = tid; i < n; i += EPI_THREADS) {
        if (!mask[i]) continue;
        bool usable;
        const double d2 = epi_sampson2(Fd, M[i], usable);
        part = part + (usable ? d2 : 0.0);
      }
      err = sqrt(block_sum<EPI_THREADS>(part, red) / cnt);
    }
  }
  for (int i = tid; i < cap; i += EPI_THREADS) mo[i] = (valid && i < n) ? mask[i] : 0;
  if (tid == 0) {
    double* fo = f_out + (size_t)p * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) fo[k] = valid ? Fd[k] : 0.0;
    n_inl_out[p] = valid ? (int)cnt : 0;
    status_out[p] = valid ? 0 : 1;
    if (winner_out != nullptr) winner_out[p] = valid ? winner : -1;
    if (err_out != nullptr) err_out[p] = valid ? err : 0.0;
  }
}

// grid (pairs), TRACK_BLOCK threads.  Keeps the match rows whose mask byte is set, in order (block_scan_flag: wave ballots
// and popcounts), and writes zero rows behind them.  status != 0 or n_inliers < min_inliers: every row passes.
__global__ __launch_bounds__(TRACK_BLOCK) void match_filter_kernel(const float* __restrict__ match, const int32_t* __restrict__ n_match,
                                                                   const uint8_t* __restrict__ mask,
                                                                   const int32_t* __restrict__ status,
                                                                   const int32_t* __restrict__ n_inliers, int min_inliers,
                                                                   int cap, float* __restrict__ match_out,
                                                                   int32_t* __restrict__ n_match_out) {
  __shared__ int wsum[TRACK_BLOCK / 64];
  const int p = blockIdx.x;
  const int n = min(max(n_match[p], 0), cap);
  const bool pass = status[p] != 0 || n_inliers[p] < min_inliers;
  const float* src = match + (size_t)p * cap * 3;
  const uint8_t* mk = mask + (size_t)p * cap;
  float* dst = match_out + (size_t)p * cap * 3;
  int base = 0;
  for (int i0 = 0; i0 < cap; i0 += TRACK_BLOCK) {  // (uniform trip count: every thread reaches the barriers of the scan)
    const int i = i0 + threadIdx.x;
    const bool keep = i < n && (pass || mk[i] != 0);
    int total;
    const int pos = base + block_scan_flag<TRACK_BLOCK>(keep, wsum, total);
    if (keep) {
      dst[(size_t)pos * 3] = src[(size_t)i * 3];
      dst[(size_t)pos * 3 + 1] = src[(size_t)i * 3 + 1];
      dst[(size_t)pos * 3 + 2] = src[(size_t)i * 3 + 2];
    }
    base += total;
  }
  __syncthreads();
  for (int i = base + threadIdx.x; i < cap; i += TRACK_BLOCK) dst[(size_t)i * 3] = dst[(size_t)i * 3 + 1] = dst[(size_t)i * 3 + 2] = 0.f;
  if (threadIdx.x == 0) n_match_out[p] = base;
}

}  // namespace sspk
