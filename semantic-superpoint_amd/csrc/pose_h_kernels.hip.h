// Homography pose and model selection: the camera motion a pair's homography implies (a plane seen twice,
// or a camera that only rotates), and the decision whether a pair obeys its fundamental matrix or its homography.  The rules are
// restated in numpy by tests/pose_h_ref.py; everything here is fp64 with contraction off, in the parenthesisation of that file.
//   pose_h_kernel        grid (pairs), 256 threads: Hn = K2^-1 H K1, its sign from the inliers, the Jacobi sweeps on Hn^T Hn, the
//                        rotation or the four (R, N, T) candidates (all redundantly per thread), the counts of the inliers in
//                        block_sum's fixed order, the choice among the candidates alive, then the per-row outputs under the winner
//   model_select_kernel  grid (pairs), 256 threads: the two robust scores over the unfiltered matches in block_sum's order, the
//                        decision, and the selected model's mask / n_inliers / status in buffers of their own
// The 3x3 work lives in registers: every index is a constant after unrolling, a data-dependent choice is a select.
// Needs: geom_blocks.hip.h, epipolar_kernels.hip.h (EPI_JACOBI_SWEEPS), pose_kernels.hip.h (pose_rays, pose_depths).
#pragma once

namespace sspk {

#define POSE_H_CHI2_H 5.99
#define POSE_H_CHI2_F 3.84

// One (R, N, T) pair of candidates of the normalised Hs: U = [v2, u, v2 x u], W = [Hs v2, Hs u, Hs v2 x Hs u], R = W U^T.
__device__ __forceinline__ void pose_h_candidate(const double (&Hs)[9], const double (&v2)[3], const double (&u)[3], double (&R)[9],
                                                 double (&N)[3], double (&T)[3]) {
#pragma clang fp contract(off)
  double hv[3], hu[3], hw[3];
  cross3(v2, u, N);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    hv[k] = dot3(Hs[3 * k], Hs[3 * k + 1], Hs[3 * k + 2], v2[0], v2[1], v2[2]);
    hu[k] = dot3(Hs[3 * k], Hs[3 * k + 1], Hs[3 * k + 2], u[0], u[1], u[2]);
  }
  cross3(hv, hu, hw);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) R[3 * a + b] = (hv[a] * v2[b] + hu[a] * u[b]) + hw[a] * N[b];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    T[k] = dot3(Hs[3 * k] - R[3 * k], Hs[3 * k + 1] - R[3 * k + 1], Hs[3 * k + 2] - R[3 * k + 2], N[0], N[1], N[2]);
}

// A row under candidate (R, sg N, sg t): on the plane's camera side and in front of both cameras.
__device__ __forceinline__ bool pose_h_front(const double (&R)[9], const double (&N)[3], const double (&t)[3], double sg, double x1x,
                                             double x1y, double x2x, double x2y, double& z1, double& z2) {
#pragma clang fp contract(off)
  const double side = dot3(sg * N[0], sg * N[1], sg * N[2], x1x, x1y, 1.0);
  const bool fr = pose_depths(R, sg * t[0], sg * t[1], sg * t[2], x1x, x1y, x2x, x2y, z1, z2);
  return fr && side > 0.0;
}

// grid (pairs).  The arguments of pose_kernel with h_in for f_in and no e_out; prior [pairs][2][3] or nullptr; use_h [pairs] or
// nullptr: a pair whose use_h is 0 writes model 0, a zero normal and zero normals2 and nothing else.  model_out [pairs],
// normal_out [pairs][3], normals2_out [pairs][2][3].
__global__ __launch_bounds__(POSE_THREADS) void pose_h_kernel(
    const double* __restrict__ h_in, const uint8_t* __restrict__ mask_in, const int32_t* __restrict__ n_inl_in,
    const int32_t* __restrict__ status_in, const double* __restrict__ pts1, const double* __restrict__ pts2, int pt_stride, int cap,
    int pair_stride, const float* __restrict__ match, const int32_t* __restrict__ n_match, const double* __restrict__ intr, int n_intr,
    const double* __restrict__ prior, const int32_t* __restrict__ use_h, double rotation_eps, double normal_margin,
    double* __restrict__ r_out, double* __restrict__ t_out, int32_t* __restrict__ cand_out, int32_t* __restrict__ counts_out,
    int32_t* __restrict__ n_front_out, int32_t* __restrict__ status_out, uint8_t* __restrict__ front_out, double* __restrict__ depth_out,
    double* __restrict__ x_out, int32_t* __restrict__ model_out, double* __restrict__ normal_out, double* __restrict__ normals2_out) {
#pragma clang fp contract(off)
  __shared__ double red[POSE_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (use_h != nullptr && use_h[p] == 0) {   // (uniform over the workgroup)
    if (tid == 0) {
      model_out[p] = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) normal_out[(size_t)p * 3 + k] = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) normals2_out[(size_t)p * 6 + k] = 0.0;
    }
    return;
  }
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
  bool valid = status_in[p] == 0 && n_inl >= POSE_MIN_FRONT;   // (uniform over the workgroup, as everything that follows from H)
  double Hs[9];
  {
    const double* H = h_in + (size_t)p * 9;
    double B[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      B[3 * r] = H[3 * r] * K.fx1;
      B[3 * r + 1] = H[3 * r + 1] * K.fy1;
      B[3 * r + 2] = (H[3 * r] * K.cx1 + H[3 * r + 1] * K.cy1) + H[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Hs[c] = (B[c] - K.cx2 * B[6 + c]) / K.fx2;
      Hs[3 + c] = (B[3 + c] - K.cy2 * B[6 + c]) / K.fy2;
      Hs[6 + c] = B[6 + c];
    }
  }
  int model = 0, win = -1, status = 1;
  int cnt[4] = {0, 0, 0, 0};
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, Nw[3] = {0.0, 0.0, 0.0};
  double n2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double sgw = 1.0;
  double pri[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (prior != nullptr) {
#pragma unroll
    for (int k = 0; k < 6; ++k) pri[k] = prior[(size_t)p * 6 + k];
  }
  const bool have0 = pri[0] != 0.0 || pri[1] != 0.0 || pri[2] != 0.0, have1 = pri[3] != 0.0 || pri[4] != 0.0 || pri[5] != 0.0;
  if (valid) {
    // the sign: b~^T Hn a~ > 0 for at least half of the inliers
    double cp = 0.0;
    for (int k = tid; k < n; k += POSE_THREADS) {
      if (!mk[k]) continue;
      double x1x, x1y, x2x, x2y;
      pose_rays(P1, P2, pt_stride, cap, M, k, K, x1x, x1y, x2x, x2y);
      const double h0 = dot3(Hs[0], Hs[1], Hs[2], x1x, x1y, 1.0), h1 = dot3(Hs[3], Hs[4], Hs[5], x1x, x1y, 1.0);
      const double h2 = dot3(Hs[6], Hs[7], Hs[8], x1x, x1y, 1.0);
      cp = cp + (dot3(x2x, x2y, 1.0, h0, h1, h2) > 0.0 ? 1.0 : 0.0);
    }
    const int pos = (int)block_sum<POSE_THREADS>(cp, red);
    if (2 * pos < n_inl) {
#pragma unroll
      for (int k = 0; k < 9; ++k) Hs[k] = -Hs[k];
    }
    double G[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        G[i][j] = dot3(Hs[i], Hs[3 + i], Hs[6 + i], Hs[j], Hs[3 + j], Hs[6 + j]);
        V[i][j] = i == j ? 1.0 : 0.0;
      }
    for (int sweep = 0; sweep < EPI_JACOBI_SWEEPS; ++sweep) {
      jacobi_rotate<0, 1>(G, V);
      jacobi_rotate<0, 2>(G, V);
      jacobi_rotate<1, 2>(G, V);
    }
    // descending order, the lowest index on ties
    const double d0 = G[0][0], d1 = G[1][1], d2 = G[2][2];
    const int k0 = d2 > (d1 > d0 ? d1 : d0) ? 2 : (d1 > d0 ? 1 : 0);
    const int ra = k0 == 0 ? 1 : 0, rb = k0 == 2 ? 1 : 2;   // the other two, ascending
    const double da = ra == 1 ? d1 : d0, db = rb == 1 ? d1 : d2;
    const int k1 = db > da ? rb : ra, k2 = db > da ? ra : rb;
    double w1 = k0 == 0 ? d0 : (k0 == 1 ? d1 : d2), w3 = k2 == 0 ? d0 : (k2 == 1 ? d1 : d2);
    const double w2 = k1 == 0 ? d0 : (k1 == 1 ? d1 : d2);
    double v1[3], v2[3], v3[3], cr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v1[k] = k0 == 0 ? V[k][0] : (k0 == 1 ? V[k][1] : V[k][2]);
      v2[k] = k1 == 0 ? V[k][0] : (k1 == 1 ? V[k][1] : V[k][2]);
      v3[k] = k2 == 0 ? V[k][0] : (k2 == 1 ? V[k][1] : V[k][2]);
    }
    cross3(v1, v2, cr);
    if (dot3(cr[0], cr[1], cr[2], v3[0], v3[1], v3[2]) < 0.0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) v3[k] = -v3[k];
    }
    valid = isfinite(w1) && isfinite(w3) && isfinite(w2) && w2 > 0.0;
    const double s2 = sqrt(w2);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      Hs[k] = Hs[k] / s2;
      fin = fin && isfinite(Hs[k]);
    }
    w1 = w1 / w2;
    w3 = w3 / w2;
    if (!(w3 > 0.0)) w3 = 0.0;
    valid = valid && fin && isfinite(w1);
    if (valid && sqrt(w1) - sqrt(w3) <= rotation_eps) {
      // a rotation only: Hs made orthonormal
      const double nr0 = sqrt(dot3(Hs[0], Hs[1], Hs[2], Hs[0], Hs[1], Hs[2]));
      const double r0[3] = {Hs[0] / nr0, Hs[1] / nr0, Hs[2] / nr0};
      const double pj = dot3(Hs[3], Hs[4], Hs[5], r0[0], r0[1], r0[2]);
      const double w[3] = {Hs[3] - pj * r0[0], Hs[4] - pj * r0[1], Hs[5] - pj * r0[2]};
      const double nr1 = sqrt(dot3(w[0], w[1], w[2], w[0], w[1], w[2]));
      const double r1[3] = {w[0] / nr1, w[1] / nr1, w[2] / nr1};
      double r2[3];
      cross3(r0, r1, r2);
      bool ok = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) ok = ok && isfinite(r0[k]) && isfinite(r1[k]) && isfinite(r2[k]);
      if (ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          R[k] = r0[k];
          R[3 + k] = r1[k];
          R[6 + k] = r2[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // the priors travel with the camera
          n2[k] = have0 ? dot3(R[3 * k], R[3 * k + 1], R[3 * k + 2], pri[0], pri[1], pri[2]) : 0.0;
          n2[3 + k] = have1 ? dot3(R[3 * k], R[3 * k + 1], R[3 * k + 2], pri[3], pri[4], pri[5]) : 0.0;
        }
        model = 2;
        status = 0;
      }
      valid = false;   // no row is counted and none has a depth
    } else if (valid) {
      const double pp = sqrt(1.0 - w3), qq = sqrt(w1 - 1.0), rr = sqrt(w1 - w3);
      double ua[3], ub[3], Ra[9], Rb[9], Na[3], Nb[3], Ta[3], Tb[3], ta[3], tb[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ua[k] = (pp * v1[k] + qq * v3[k]) / rr;
        ub[k] = (pp * v1[k] - qq * v3[k]) / rr;
      }
      pose_h_candidate(Hs, v2, ua, Ra, Na, Ta);
      pose_h_candidate(Hs, v2, ub, Rb, Nb, Tb);
      const double tna = sqrt(dot3(Ta[0], Ta[1], Ta[2], Ta[0], Ta[1], Ta[2])), tnb = sqrt(dot3(Tb[0], Tb[1], Tb[2], Tb[0], Tb[1], Tb[2]));
      bool ok = isfinite(tna) && tna > 0.0 && isfinite(tnb) && tnb > 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ta[k] = Ta[k] / tna;
        tb[k] = Tb[k] / tnb;
        ok = ok && isfinite(Na[k]) && isfinite(Nb[k]);
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) ok = ok && isfinite(Ra[k]) && isfinite(Rb[k]);
      valid = ok;
      if (valid) {
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
        for (int k = tid; k < n; k += POSE_THREADS) {
          if (!mk[k]) continue;
          double x1x, x1y, x2x, x2y, z1, z2;
          pose_rays(P1, P2, pt_stride, cap, M, k, K, x1x, x1y, x2x, x2y);
          c0 = c0 + (pose_h_front(Ra, Na, ta, 1.0, x1x, x1y, x2x, x2y, z1, z2) ? 1.0 : 0.0);
          c1 = c1 + (pose_h_front(Ra, Na, ta, -1.0, x1x, x1y, x2x, x2y, z1, z2) ? 1.0 : 0.0);
          c2 = c2 + (pose_h_front(Rb, Nb, tb, 1.0, x1x, x1y, x2x, x2y, z1, z2) ? 1.0 : 0.0);
          c3 = c3 + (pose_h_front(Rb, Nb, tb, -1.0, x1x, x1y, x2x, x2y, z1, z2) ? 1.0 : 0.0);
        }
        cnt[0] = (int)block_sum<POSE_THREADS>(c0, red);
        cnt[1] = (int)block_sum<POSE_THREADS>(c1, red);
        cnt[2] = (int)block_sum<POSE_THREADS>(c2, red);
        cnt[3] = (int)block_sum<POSE_THREADS>(c3, red);
        bool alive[4];
        double sc[4], nz[4];
        int n_alive = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          alive[c] = cnt[c] >= POSE_MIN_FRONT && 2 * cnt[c] >= n_inl;
          n_alive += alive[c] ? 1 : 0;
          const double sg = (c & 1) ? -1.0 : 1.0;
          const double N0 = sg * (c >= 2 ? Nb[0] : Na[0]), N1 = sg * (c >= 2 ? Nb[1] : Na[1]), N2 = sg * (c >= 2 ? Nb[2] : Na[2]);
          nz[c] = N2;
          const double s0 = dot3(N0, N1, N2, pri[0], pri[1], pri[2]), s1 = dot3(N0, N1, N2, pri[3], pri[4], pri[5]);
          sc[c] = have0 ? ((have1 && s1 > s0) ? s1 : s0) : s1;
        }
        status = 2;
        if (n_alive == 0) {
          win = 0;
          int best = cnt[0];
#pragma unroll
          for (int c = 1; c < 4; ++c) {
            const bool g = cnt[c] > best;
            best = g ? cnt[c] : best;
            win = g ? c : win;
          }
        } else if (n_alive == 1) {
          win = alive[0] ? 0 : (alive[1] ? 1 : (alive[2] ? 2 : 3));
          status = 0;
        } else {
          if (have0 || have1) {
            int best = -1, second = -1;
            double sbest = 0.0, ssecond = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const bool g = alive[c] && (best < 0 || sc[c] > sbest);
              sbest = g ? sc[c] : sbest;
              best = g ? c : best;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const bool g = alive[c] && c != best && (second < 0 || sc[c] > ssecond);
              ssecond = g ? sc[c] : ssecond;
              second = g ? c : second;
            }
            if (sbest - ssecond >= normal_margin) {
              win = best;
              status = 0;
            }
          }
          if (win < 0) {
            double zbest = 0.0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const bool g = alive[c] && (win < 0 || nz[c] > zbest);
              zbest = g ? nz[c] : zbest;
              win = g ? c : win;
            }
          }
        }
        sgw = (win & 1) ? -1.0 : 1.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = win >= 2 ? Rb[k] : Ra[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          t[k] = sgw * (win >= 2 ? tb[k] : ta[k]);
          Nw[k] = sgw * (win >= 2 ? Nb[k] : Na[k]);
        }
        // the transported normals of the candidates alive, in index order, two at most
        int slot = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double sg = (c & 1) ? -1.0 : 1.0;
          const bool put = alive[c] && slot < 2;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double v = c >= 2 ? dot3(Rb[3 * k], Rb[3 * k + 1], Rb[3 * k + 2], sg * Nb[0], sg * Nb[1], sg * Nb[2])
                                    : dot3(Ra[3 * k], Ra[3 * k + 1], Ra[3 * k + 2], sg * Na[0], sg * Na[1], sg * Na[2]);
            n2[k] = (put && slot == 0) ? v : n2[k];
            n2[3 + k] = (put && slot == 1) ? v : n2[3 + k];
          }
          slot += put ? 1 : 0;
        }
        model = 1;
      }
    }
  }
  const bool rows = valid && model == 1;
  for (int k = tid; k < cap; k += POSE_THREADS) {
    bool fr = false;
    double z1 = 0.0, z2 = 0.0, x1x = 0.0, x1y = 0.0, x2x, x2y;
    if (rows && k < n && mk[k]) {
      pose_rays(P1, P2, pt_stride, cap, M, k, K, x1x, x1y, x2x, x2y);
      const double side = dot3(Nw[0], Nw[1], Nw[2], x1x, x1y, 1.0);
      fr = pose_depths(R, t[0], t[1], t[2], x1x, x1y, x2x, x2y, z1, z2) && side > 0.0;
    }
    fo[k] = fr ? 1 : 0;
    dp[(size_t)k * 2] = fr ? z1 : 0.0;
    dp[(size_t)k * 2 + 1] = fr ? z2 : 0.0;
    xo[(size_t)k * 3] = fr ? z1 * x1x : 0.0;
    xo[(size_t)k * 3 + 1] = fr ? z1 * x1y : 0.0;
    xo[(size_t)k * 3 + 2] = fr ? z1 : 0.0;
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) r_out[(size_t)p * 9 + k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t_out[(size_t)p * 3 + k] = t[k];
      normal_out[(size_t)p * 3 + k] = Nw[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) normals2_out[(size_t)p * 6 + k] = n2[k];
#pragma unroll
    for (int c = 0; c < 4; ++c) counts_out[(size_t)p * 4 + c] = rows ? cnt[c] : 0;
    cand_out[p] = rows ? win : -1;
    n_front_out[p] = rows ? cnt[win < 0 ? 0 : win] : 0;
    status_out[p] = status;
    model_out[p] = model;
  }
}

// The truncated score of a squared distance: 5.99 - d2 below `limit`.  The offset is 5.99 for both models on purpose (so that a
// perfect F row and a perfect H row score alike); only the limit differs, 5.99 for H and 3.84 for F.
__device__ __forceinline__ double pose_h_rho(double d2, double limit) { return d2 < limit ? POSE_H_CHI2_H - d2 : 0.0; }

// Squared distance between (u0, v0) and the image of (x, y) under the 3x3 M.
__device__ __forceinline__ double pose_h_transfer2(const double (&m)[9], double x, double y, double u0, double v0) {
#pragma clang fp contract(off)
  const double w = dot3(m[6], m[7], m[8], x, y, 1.0);
  const double du = dot3(m[0], m[1], m[2], x, y, 1.0) / w - u0, dv = dot3(m[3], m[4], m[5], x, y, 1.0) / w - v0;
  return du * du + dv * dv;
}

// grid (pairs).  scores_out [pairs][2] = (S_H, S_F), use_h_out [pairs]; mask_out [pairs][cap], n_inl_out, status_out: the selected
// model's, copied.
__global__ __launch_bounds__(POSE_THREADS) void model_select_kernel(
    const double* __restrict__ f_in, const uint8_t* __restrict__ f_mask, const int32_t* __restrict__ f_n_inl,
    const int32_t* __restrict__ f_status, const double* __restrict__ h_in, const uint8_t* __restrict__ h_mask,
    const int32_t* __restrict__ h_n_inl, const int32_t* __restrict__ h_status, const double* __restrict__ pts1,
    const double* __restrict__ pts2, int pt_stride, int cap, int pair_stride, const float* __restrict__ match,
    const int32_t* __restrict__ n_match, double model_ratio, double* __restrict__ scores_out, int32_t* __restrict__ use_h_out,
    uint8_t* __restrict__ mask_out, int32_t* __restrict__ n_inl_out, int32_t* __restrict__ status_out) {
#pragma clang fp contract(off)
  __shared__ double red[POSE_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(n_match[p], 0), cap);
  const double* P1 = pts1 + (size_t)p * pair_stride * cap * pt_stride;
  const double* P2 = pts2 + (size_t)p * pair_stride * cap * pt_stride;
  const float* M = match + (size_t)p * cap * 3;
  double h[9], f[9], A[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    h[k] = h_in[(size_t)p * 9 + k];
    f[k] = f_in[(size_t)p * 9 + k];
  }
  A[0] = h[4] * h[8] - h[5] * h[7];
  A[1] = h[2] * h[7] - h[1] * h[8];
  A[2] = h[1] * h[5] - h[2] * h[4];
  A[3] = h[5] * h[6] - h[3] * h[8];
  A[4] = h[0] * h[8] - h[2] * h[6];
  A[5] = h[2] * h[3] - h[0] * h[5];
  A[6] = h[3] * h[7] - h[4] * h[6];
  A[7] = h[1] * h[6] - h[0] * h[7];
  A[8] = h[0] * h[4] - h[1] * h[3];
  const double det = dot3(h[0], h[1], h[2], A[0], A[3], A[6]);
  const bool h_ok = isfinite(det) && det != 0.0;
  double sh = 0.0, sf = 0.0;
  for (int k = tid; k < n; k += POSE_THREADS) {
    const float* m = M + (size_t)k * 3;
    const int i = min(max((int)m[0], 0), cap - 1), j = min(max((int)m[1], 0), cap - 1);
    const double ax = P1[(size_t)i * pt_stride], ay = P1[(size_t)i * pt_stride + 1];
    const double bx = P2[(size_t)j * pt_stride], by = P2[(size_t)j * pt_stride + 1];
    const double th = pose_h_rho(pose_h_transfer2(h, ax, ay, bx, by), POSE_H_CHI2_H) + pose_h_rho(pose_h_transfer2(A, bx, by, ax, ay), POSE_H_CHI2_H);
    sh = sh + (h_ok ? th : 0.0);
    const double l20 = dot3(f[0], f[1], f[2], ax, ay, 1.0), l21 = dot3(f[3], f[4], f[5], ax, ay, 1.0), l22 = dot3(f[6], f[7], f[8], ax, ay, 1.0);
    const double l10 = dot3(f[0], f[3], f[6], bx, by, 1.0), l11 = dot3(f[1], f[4], f[7], bx, by, 1.0);
    const double e = dot3(bx, by, 1.0, l20, l21, l22);
    const double ee = e * e;
    sf = sf + (pose_h_rho(ee / (l20 * l20 + l21 * l21), POSE_H_CHI2_F) + pose_h_rho(ee / (l10 * l10 + l11 * l11), POSE_H_CHI2_F));
  }
  const double SH = block_sum<POSE_THREADS>(sh, red), SF = block_sum<POSE_THREADS>(sf, red);
  const bool use = h_status[p] == 0 && (f_status[p] != 0 || SH >= model_ratio * (SH + SF));
  const uint8_t* src = (use ? h_mask : f_mask) + (size_t)p * cap;
  for (int k = tid; k < cap; k += POSE_THREADS) mask_out[(size_t)p * cap + k] = src[k];
  if (tid == 0) {
    scores_out[(size_t)p * 2] = SH;
    scores_out[(size_t)p * 2 + 1] = SF;
    use_h_out[p] = use ? 1 : 0;
    n_inl_out[p] = use ? h_n_inl[p] : f_n_inl[p];
    status_out[p] = use ? h_status[p] : f_status[p];
  }
}

}  // namespace sspk
