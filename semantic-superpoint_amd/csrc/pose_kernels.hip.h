// Two-view pose: the camera motion of a pair from the fundamental matrix of section 22, its inlier
// mask and the intrinsics of the two views, and the scale chain / trajectory over consecutive pairs.  The rules are restated
// in numpy by tests/pose_ref.py; everything here is fp64 with contraction off, in the parenthesisation of that file.
//   pose_kernel        grid (pairs), 256 threads: E0 = K2^T F K1, the Jacobi sweeps on E0^T E0, U and V without a 3x3 SVD,
//                      the four (R, t) candidates (all redundantly per thread), the in-front counts of the inliers in
//                      block_sum's fixed order, then the per-row outputs under the winner
//   pose_chain_kernel  grid (sequences), 256 threads: depth of frame f's points under pair A in LDS ("the lowest row wins"
//                      by an LDS minimum: no order to depend on), the two sums over the shared points, the state update and
//                      the trajectory row
// The 3x3 work lives in registers: every index is a constant after unrolling, a data-dependent column is a select.
// Needs: geom_blocks.hip.h, epipolar_kernels.hip.h (EPI_JACOBI_SWEEPS).
#pragma once

namespace sspk {

#define POSE_THREADS 256
#define POSE_MIN_FRONT 8
#define POSE_DET_EPS 1e-12
#define POSE_ROW_WORDS 16
#define POSE_STATE_WORDS 16

// (fx, fy, cx, cy) of the two views of a pair
struct PoseIntr {
  double fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
};

// The candidates of a pair: E = u0 v0^T + u1 v1^T, Ra = U W V^T, Rb = U W^T V^T, t = +-u2.  false: a degenerate case.
__device__ __forceinline__ bool pose_candidates(const double* __restrict__ F, PoseIntr K, double (&Em)[9], double (&Ra)[9],
                                                double (&Rb)[9], double (&u2)[3]) {
#pragma clang fp contract(off)
  double B[9], E0[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    B[3 * r] = F[3 * r] * K.fx1;
    B[3 * r + 1] = F[3 * r + 1] * K.fy1;
    B[3 * r + 2] = (F[3 * r] * K.cx1 + F[3 * r + 1] * K.cy1) + F[3 * r + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    E0[c] = K.fx2 * B[c];
    E0[3 + c] = K.fy2 * B[3 + c];
    E0[6 + c] = (K.cx2 * B[c] + K.cy2 * B[3 + c]) + B[6 + c];
  }
  double ss = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) ss = ss + E0[k] * E0[k];
  const double nrm = sqrt(ss);
  bool ok = isfinite(nrm) && nrm > 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) E0[k] = E0[k] / nrm;
  double G[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      G[i][j] = dot3(E0[i], E0[3 + i], E0[6 + i], E0[j], E0[3 + j], E0[6 + j]);
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < EPI_JACOBI_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(G, V);
    jacobi_rotate<0, 2>(G, V);
    jacobi_rotate<1, 2>(G, V);
  }
  // the columns of the largest and the second-largest diagonal entry, the lowest index on ties
  const double d0 = G[0][0], d1 = G[1][1], d2 = G[2][2];
  const int k0 = d2 > (d1 > d0 ? d1 : d0) ? 2 : (d1 > d0 ? 1 : 0);
  const int ra = k0 == 0 ? 1 : 0, rb = k0 == 2 ? 1 : 2;   // the other two, ascending
  const double da = ra == 1 ? d1 : d0, db = rb == 1 ? d1 : d2;
  const int k1 = db > da ? rb : ra;
  double v0[3], v1[3], v2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v0[k] = k0 == 0 ? V[k][0] : (k0 == 1 ? V[k][1] : V[k][2]);
    v1[k] = k1 == 0 ? V[k][0] : (k1 == 1 ? V[k][1] : V[k][2]);
  }
  cross3(v0, v1, v2);
  double w[3], u0[3], u1[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = dot3(E0[3 * r], E0[3 * r + 1], E0[3 * r + 2], v0[0], v0[1], v0[2]);
  const double n0 = sqrt(dot3(w[0], w[1], w[2], w[0], w[1], w[2]));
  ok = ok && isfinite(n0) && n0 > 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) u0[r] = w[r] / n0;
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = dot3(E0[3 * r], E0[3 * r + 1], E0[3 * r + 2], v1[0], v1[1], v1[2]);
  const double pw = dot3(w[0], w[1], w[2], u0[0], u0[1], u0[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = w[r] - pw * u0[r];
  const double n1 = sqrt(dot3(w[0], w[1], w[2], w[0], w[1], w[2]));
  ok = ok && isfinite(n1) && n1 > 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) u1[r] = w[r] / n1;
  cross3(u0, u1, u2);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Em[3 * r + c] = u0[r] * v0[c] + u1[r] * v1[c];
      Ra[3 * r + c] = (u1[r] * v0[c] - u0[r] * v1[c]) + u2[r] * v2[c];
      Rb[3 * r + c] = (u0[r] * v1[c] - u1[r] * v0[c]) + u2[r] * v2[c];
    }
  return ok;
}

// Depths of the rays x1 = (x1x, x1y, 1), x2 = (x2x, x2y, 1) under (R, t): the least-squares meeting point of z1 R x1 + t and
// z2 x2.  Returns "in front of both cameras".
__device__ __forceinline__ bool pose_depths(const double (&R)[9], double t0, double t1, double t2, double x1x, double x1y,
                                            double x2x, double x2y, double& z1, double& z2) {
#pragma clang fp contract(off)
  const double a0 = dot3(R[0], R[1], R[2], x1x, x1y, 1.0);
  const double a1 = dot3(R[3], R[4], R[5], x1x, x1y, 1.0);
  const double a2 = dot3(R[6], R[7], R[8], x1x, x1y, 1.0);
  const double A11 = dot3(a0, a1, a2, a0, a1, a2), A22 = dot3(x2x, x2y, 1.0, x2x, x2y, 1.0);
  const double A12 = dot3(a0, a1, a2, x2x, x2y, 1.0);
  const double b1 = -dot3(a0, a1, a2, t0, t1, t2), b2 = dot3(x2x, x2y, 1.0, t0, t1, t2);
  const double det = A11 * A22 - A12 * A12;
  z1 = (b1 * A22 + A12 * b2) / det;
  z2 = (A11 * b2 + A12 * b1) / det;
  return det > POSE_DET_EPS * (A11 * A22) && isfinite(z1) && isfinite(z2) && z1 > 0.0 && z2 > 0.0;
}

// Rays of match row k of a pair: indices clamped to the arrays as epi_stage clamps them.
__device__ __forceinline__ void pose_rays(const double* __restrict__ pts1, const double* __restrict__ pts2, int pt_stride, int cap,
                                          const float* __restrict__ match, int k, PoseIntr K, double& x1x, double& x1y, double& x2x,
                                          double& x2y) {
#pragma clang fp contract(off)
  const float* m = match + (size_t)k * 3;
  const int i = min(max((int)m[0], 0), cap - 1), j = min(max((int)m[1], 0), cap - 1);
  const double* a = pts1 + (size_t)i * pt_stride;
  const double* b = pts2 + (size_t)j * pt_stride;
  x1x = (a[0] - K.cx1) / K.fx1;
  x1y = (a[1] - K.cy1) / K.fy1;
  x2x = (b[0] - K.cx2) / K.fx2;
  x2y = (b[1] - K.cy2) / K.fy2;
}

// grid (pairs).  intr [n_intr][2][4], n_intr = 1 (shared) or pairs.  Per pair: r_out [9], t_out [3], e_out [9], cand_out,
// counts_out [4], n_front_out, status_out; per match row (aligned with the unfiltered rows, as the mask is): front_out [cap],
// depth_out [cap][2], x_out [cap][3].
__global__ __launch_bounds__(POSE_THREADS) void pose_kernel(const double* __restrict__ f_in, const uint8_t* __restrict__ mask_in,
                                                            const int32_t* __restrict__ n_inl_in, const int32_t* __restrict__ status_in,
                                                            const double* __restrict__ pts1, const double* __restrict__ pts2,
                                                            int pt_stride, int cap, int pair_stride, const float* __restrict__ match,
                                                            const int32_t* __restrict__ n_match, const double* __restrict__ intr,
                                                            int n_intr, double* __restrict__ r_out, double* __restrict__ t_out,
                                                            double* __restrict__ e_out, int32_t* __restrict__ cand_out,
                                                            int32_t* __restrict__ counts_out, int32_t* __restrict__ n_front_out,
                                                            int32_t* __restrict__ status_out, uint8_t* __restrict__ front_out,
                                                            double* __restrict__ depth_out, double* __restrict__ x_out) {
#pragma clang fp contract(off)
  __shared__ double red[POSE_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(n_match[p], 0), cap);
  const int n_inl = n_inl_in[p];
  const double* ik = intr + (size_t)(n_intr == 1 ? 0 : p) * 8;
  const PoseIntr K = {ik[0], ik[1], ik[2], ik[3], ik[4], ik[5], ik[6], ik[7]};
  const double* P1 = pts1 + (size_t)p * pair_stride * cap * pt_stride;
  const double* P2 = pts2 + (size_t)p * pair_stride * cap * pt_stride;
  const float* M = match + (size_t)p * cap * 3;
  const uint8_t* mk = mask_in + (size_t)p * cap;
  uint8_t* fo = front_out + (size_t)p * cap;
  double* dp = depth_out + (size_t)p * cap * 2;
  double* xo = x_out + (size_t)p * cap * 3;
  double Em[9], Ra[9], Rb[9], u2[3];
  bool valid = status_in[p] == 0 && n_inl >= POSE_MIN_FRONT;  // (uniform over the workgroup, as everything that follows from F)
  if (valid) valid = pose_candidates(f_in + (size_t)p * 9, K, Em, Ra, Rb, u2);
  int cnt[4] = {0, 0, 0, 0};
  int win = -1;
  if (valid) {
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    for (int k = tid; k < n; k += POSE_THREADS) {
      if (!mk[k]) continue;
      double x1x, x1y, x2x, x2y, z1, z2;
      pose_rays(P1, P2, pt_stride, cap, M, k, K, x1x, x1y, x2x, x2y);
      c0 = c0 + (pose_depths(Ra, u2[0], u2[1], u2[2], x1x, x1y, x2x, x2y, z1, z2) ? 1.0 : 0.0);
      c1 = c1 + (pose_depths(Ra, -u2[0], -u2[1], -u2[2], x1x, x1y, x2x, x2y, z1, z2) ? 1.0 : 0.0);
      c2 = c2 + (pose_depths(Rb, u2[0], u2[1], u2[2], x1x, x1y, x2x, x2y, z1, z2) ? 1.0 : 0.0);
      c3 = c3 + (pose_depths(Rb, -u2[0], -u2[1], -u2[2], x1x, x1y, x2x, x2y, z1, z2) ? 1.0 : 0.0);
    }
    cnt[0] = (int)block_sum<POSE_THREADS>(c0, red);  // (counts: exact in fp64, and the order is fixed anyway)
    cnt[1] = (int)block_sum<POSE_THREADS>(c1, red);
    cnt[2] = (int)block_sum<POSE_THREADS>(c2, red);
    cnt[3] = (int)block_sum<POSE_THREADS>(c3, red);
    win = 0;
    int best = cnt[0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
      const bool g = cnt[c] > best;
      best = g ? cnt[c] : best;
      win = g ? c : win;
    }
  }
  double R[9], t[3];
  const double sg = (win & 1) ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = valid ? (win >= 2 ? Rb[k] : Ra[k]) : ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0);
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = valid ? (sg < 0.0 ? -u2[k] : u2[k]) : 0.0;
  for (int k = tid; k < cap; k += POSE_THREADS) {
    bool fr = false;
    double z1 = 0.0, z2 = 0.0, x1x = 0.0, x1y = 0.0, x2x, x2y;
    if (valid && k < n && mk[k]) {
      pose_rays(P1, P2, pt_stride, cap, M, k, K, x1x, x1y, x2x, x2y);
      fr = pose_depths(R, t[0], t[1], t[2], x1x, x1y, x2x, x2y, z1, z2);
    }
    fo[k] = fr ? 1 : 0;
    dp[(size_t)k * 2] = fr ? z1 : 0.0;
    dp[(size_t)k * 2 + 1] = fr ? z2 : 0.0;
    xo[(size_t)k * 3] = fr ? z1 * x1x : 0.0;
    xo[(size_t)k * 3 + 1] = fr ? z1 * x1y : 0.0;
    xo[(size_t)k * 3 + 2] = fr ? z1 : 0.0;
  }
  if (tid == 0) {
    const int nf = valid ? cnt[win < 0 ? 0 : win] : 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      r_out[(size_t)p * 9 + k] = R[k];
      e_out[(size_t)p * 9 + k] = valid ? Em[k] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) t_out[(size_t)p * 3 + k] = t[k];
#pragma unroll
    for (int c = 0; c < 4; ++c) counts_out[(size_t)p * 4 + c] = valid ? cnt[c] : 0;
    cand_out[p] = valid ? win : -1;
    n_front_out[p] = nf;
    status_out[p] = !valid ? 1 : ((nf < POSE_MIN_FRONT || 2 * nf < n_inl) ? 2 : 0);
  }
}

// grid (sequences).  Pair A = (f-1, f) ("prev"; front_a == nullptr: there is no such pair) and B = (f, f+1) ("cur").  A point of
// frame f is row j of A's matches and row i of B's.  state [POSE_STATE_WORDS]: n_frames, s, Rw [9], tw [3]; the row
// (Rw [9], C [3], s, n_shared, flags, ratio) is appended to table [capacity][POSE_ROW_WORDS] while it has room.
// Dynamic LDS: max(cap_a, cap_b) * (8 + 4) bytes.
__global__ __launch_bounds__(POSE_THREADS) void pose_chain_kernel(const uint8_t* __restrict__ front_a, const double* __restrict__ depth_a,
                                                                  const int32_t* __restrict__ status_a, const float* __restrict__ match_a,
                                                                  const int32_t* __restrict__ n_match_a, int cap_a,
                                                                  const uint8_t* __restrict__ front_b, const double* __restrict__ depth_b,
                                                                  const int32_t* __restrict__ status_b, const double* __restrict__ r_b,
                                                                  const double* __restrict__ t_b, const float* __restrict__ match_b,
                                                                  const int32_t* __restrict__ n_match_b, int cap_b,
                                                                  double* __restrict__ state, double* __restrict__ table, int capacity) {
#pragma clang fp contract(off)
  extern __shared__ double pose_dyn[];
  __shared__ double red[POSE_THREADS / 64];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int cap_f = cap_a > cap_b ? cap_a : cap_b;   // rows of the per-point table of frame f
  double* zprev = pose_dyn;
  int* owner = reinterpret_cast<int*>(pose_dyn + cap_f);
  const bool have_a = front_a != nullptr;
  for (int k = tid; k < cap_f; k += POSE_THREADS) owner[k] = 0x7FFFFFFF;
  __syncthreads();
  if (have_a) {
    const int na = min(max(n_match_a[q], 0), cap_a);
    const uint8_t* fa = front_a + (size_t)q * cap_a;
    const float* ma = match_a + (size_t)q * cap_a * 3;
    const double* da = depth_a + (size_t)q * cap_a * 2;
    for (int k = tid; k < na; k += POSE_THREADS)
      if (fa[k]) atomicMin(&owner[min(max((int)ma[(size_t)k * 3 + 1], 0), cap_a - 1)], k);   // the lowest row wins
    __syncthreads();
    for (int k = tid; k < na; k += POSE_THREADS) {
      const int j = min(max((int)ma[(size_t)k * 3 + 1], 0), cap_a - 1);
      if (fa[k] && owner[j] == k) zprev[j] = da[(size_t)k * 2 + 1];
    }
    __syncthreads();
  }
  const int nb = min(max(n_match_b[q], 0), cap_b);
  const uint8_t* fb = front_b + (size_t)q * cap_b;
  const float* mb = match_b + (size_t)q * cap_b * 3;
  const double* db = depth_b + (size_t)q * cap_b * 2;
  double sa = 0.0, sb = 0.0, sc = 0.0;
  for (int k = tid; k < nb; k += POSE_THREADS) {
    if (!fb[k]) continue;
    const int i = min(max((int)mb[(size_t)k * 3], 0), cap_b - 1);
    if (owner[i] == 0x7FFFFFFF) continue;
    sa = sa + zprev[i];
    sb = sb + db[(size_t)k * 2];
    sc = sc + 1.0;
  }
  const double SA = block_sum<POSE_THREADS>(sa, red), SB = block_sum<POSE_THREADS>(sb, red);
  const int n_shared = (int)block_sum<POSE_THREADS>(sc, red);
  if (tid != 0) return;
  double* st = state + (size_t)q * POSE_STATE_WORDS;
  const double ratio = n_shared > 0 ? SA / SB : 0.0;
  const bool posed = status_b[q] == 0;
  const bool ok = have_a && status_a[q] == 0 && posed && n_shared >= POSE_MIN_FRONT && isfinite(ratio) && ratio > 0.0;
  const double s = ok ? st[1] * ratio : st[1];
  double R[9], t[3], Rw0[9], tw0[3], Rw[9], tw[3], C[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    R[k] = posed ? r_b[(size_t)q * 9 + k] : ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0);
    Rw0[k] = st[2 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    t[k] = posed ? t_b[(size_t)q * 3 + k] : 0.0;
    tw0[k] = st[11 + k];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Rw[3 * r + c] = dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], Rw0[c], Rw0[3 + c], Rw0[6 + c]);
    tw[r] = dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], tw0[0], tw0[1], tw0[2]) + s * t[r];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) C[c] = -dot3(Rw[c], Rw[3 + c], Rw[6 + c], tw[0], tw[1], tw[2]);
  const int flags = (posed ? 0 : 1) | (ok ? 0 : 2);
  const int row = (int)st[0];
  if (row >= 0 && row < capacity) {
    double* o = table + ((size_t)q * capacity + row) * POSE_ROW_WORDS;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = Rw[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[9 + k] = C[k];
    o[12] = s;
    o[13] = (double)n_shared;
    o[14] = (double)flags;
    o[15] = ratio;
    st[0] = (double)(row + 1);
  }
  st[1] = s;
#pragma unroll
  for (int k = 0; k < 9; ++k) st[2 + k] = Rw[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) st[11 + k] = tw[k];
}

}  // namespace sspk
