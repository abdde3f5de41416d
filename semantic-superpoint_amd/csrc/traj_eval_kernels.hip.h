// Trajectory evaluation: a trajectory table against ground-truth poses, on the device.  The rules are
// restated in numpy by tests/traj_eval_ref.py.
//   traj_align_kernel         one workgroup per problem: the similarity q ~ s R p + t between the estimated and the true centres
//                             (Umeyama from two passes of moments, the rotation from Jacobi sweeps on H^T H; or the first valid
//                             frame's pose as the origin)
//   traj_ape_kernel           a thread per frame: the absolute translation and rotation error under that similarity
//   traj_rpe_delta_kernel     a thread per frame: the relative pose error between frames f and f + delta
//   traj_rpe_segments_kernel  one workgroup per problem: the cumulative ground-truth path length (an order-defined scan), the
//                             segments of the KITTI devkit by binary search, their errors and the means per length
//   traj_stats_kernel         one workgroup per problem: n, rmse, mean, std, min, max, median, sse of an error array; the median by
//                             a radix select over the bit patterns (eight 8-bit digits, integer LDS histograms), no sort
// fp64 with contraction off.  Every sum runs in one fixed order: thread t takes the rows t, t + TRAJ_THREADS, ..., then block_sums.
// No floating-point atomics, no scratch.  One workgroup per problem wherever a sum is taken, so a problem's result does not depend
// on its batch.
// Needs: geom_blocks.hip.h (dot3, cross3, mat3_mul, jacobi_rotate, block_sum, block_sums).
#pragma once

namespace sspk {

#define TRAJ_THREADS 256
#define TRAJ_ROW_WORDS 16    // a trajectory row: Rw [9], C [3], s, n_shared, flags, ratio
#define TRAJ_GT_WORDS 12     // a ground-truth row: the row-major 3x4 camera-to-world matrix (R | C)
#define TRAJ_SIM_WORDS 16    // s, R [9], t [3], n_valid, status, sigma_p^2
#define TRAJ_STATS_WORDS 8   // n, rmse, mean, std, min, max, median, sse
#define TRAJ_INFO_WORDS 4    // segments counted, with an invalid end, without an end, first frames inside the sequence
#define TRAJ_MAX_LENGTHS 8
#define TRAJ_JACOBI_SWEEPS 8
#define TRAJ_COLLINEAR_EPS 1e-24
#define TRAJ_DEG_PER_RAD 57.29577951308232
#define TRAJ_OK 0
#define TRAJ_FEW 1
#define TRAJ_COLLINEAR 2

// The inputs every kernel shares.  Strides in fp64 words between problems; gt_stride 0: one ground truth for all of them.
struct TrajIn {
  const double* table;
  size_t table_stride;
  const int32_t* n_frames;
  int capacity;
  const double* gt;
  size_t gt_stride;
  int n_gt;
  const int32_t* index;   // [capacity] or null: frame f is ground-truth row f
  int skip_flags;
};

struct TrajFrame {
  double Rw[9], C[3], Rg[9], q[3];   // world-to-camera rotation and centre of the estimate; camera-to-world rotation and centre of the truth
};

__device__ __forceinline__ int traj_frames(const TrajIn& in, int p) { return min(max(in.n_frames[p], 0), in.capacity); }

// The ground-truth row of frame f, or -1.
__device__ __forceinline__ int traj_gt_row(const TrajIn& in, int f) {
  const int g = in.index ? in.index[f] : f;
  return g >= 0 && g < in.n_gt ? g : -1;
}

// Frame f of problem p; false: not valid (outside the sequence, no ground-truth row, a skipped flag, a flag word that is no integer in
// [0, 2^31), or one of the 12 + 12 numbers not finite).
__device__ __forceinline__ bool traj_load(const TrajIn& in, int p, int f, int nf, TrajFrame& o) {
  if (f < 0 || f >= nf) return false;
  const int g = traj_gt_row(in, f);
  if (g < 0) return false;
  const double* row = in.table + (size_t)p * in.table_stride + (size_t)f * TRAJ_ROW_WORDS;
  const double* gr = in.gt + (size_t)p * in.gt_stride + (size_t)g * TRAJ_GT_WORDS;
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    o.Rw[k] = row[k];
    fin = fin && isfinite(o.Rw[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.C[k] = row[9 + k];
    fin = fin && isfinite(o.C[k]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o.Rg[3 * r + c] = gr[4 * r + c];
      fin = fin && isfinite(o.Rg[3 * r + c]);
    }
    o.q[r] = gr[4 * r + 3];
    fin = fin && isfinite(o.q[r]);
  }
  const double fl = row[14];
  const bool flag_ok = fl >= 0.0 && fl < 2147483648.0 && fl == floor(fl) && (((int)fl) & in.skip_flags) == 0;   // (a NaN fails the first comparison)
  return fin && flag_ok;
}

__device__ __forceinline__ void traj_transpose(const double (&a)[9], double (&t)[9]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) t[3 * r + c] = a[3 * c + r];
}

// atan(t) for t >= 0 in operations that are written out here, so that the restatement repeats them bit for bit whatever math
// library either side has: the classic reduction to |x| < 7/16 around the points 1/2, 1, 3/2 and infinity and an odd polynomial of
// eleven terms (the scheme and the constants of the freely distributable fdlibm s_atan.c; error below 1 ulp).
__device__ __forceinline__ double traj_atan_pos(double t) {
#pragma clang fp contract(off)
  if (t >= 73786976294838206464.0) return 1.5707963267948966;   // 2^66 and beyond
  if (t < 1.862645149230957e-09) return t;                       // below 2^-29
  double x = t, hi = 0.0, lo = 0.0;
  const bool reduced = t >= 0.4375;
  if (t >= 2.4375) {
    x = -1.0 / t;
    hi = 1.57079632679489655800e+00;
    lo = 6.12323399573676603587e-17;
  } else if (t >= 1.1875) {
    x = (t - 1.5) / (1.0 + 1.5 * t);
    hi = 9.82793723247329054082e-01;
    lo = 1.39033110312309984516e-17;
  } else if (t >= 0.6875) {
    x = (t - 1.0) / (t + 1.0);
    hi = 7.85398163397448278999e-01;
    lo = 3.06161699786838301793e-17;
  } else if (reduced) {
    x = (2.0 * t - 1.0) / (2.0 + t);
    hi = 4.63647609000806093515e-01;
    lo = 2.26987774529616870924e-17;
  }
  const double z = x * x, w = z * z;
  const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 + w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
  const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 + w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
  if (!reduced) return x - x * (s1 + s2);
  return hi - ((x * (s1 + s2) - lo) - x);
}

// atan2(y, x) for y >= 0: 0 or pi on the axis y = 0, pi / 2 for x = 0, else atan(y / |x|), taken from pi for x < 0.
__device__ __forceinline__ double traj_atan2_pos(double y, double x) {
#pragma clang fp contract(off)
  if (y == 0.0) return x < 0.0 ? 3.1415926535897931160e+00 : 0.0;
  if (x == 0.0) return 1.5707963267948966;
  const double z = traj_atan_pos(y / fabs(x));
  return x > 0.0 ? z : 3.1415926535897931160e+00 - (z - 1.2246467991473531772e-16);
}

// The angle of the rotation E in radians: atan2 of half the length of its antisymmetric part and half its trace less one.
__device__ __forceinline__ double traj_angle(const double (&E)[9]) {
#pragma clang fp contract(off)
  const double a = E[7] - E[5], b = E[2] - E[6], c = E[3] - E[1];
  const double sn = 0.5 * sqrt(dot3(a, b, c, a, b, c));
  const double cs = 0.5 * (((E[0] + E[4]) + E[8]) - 1.0);
  return traj_atan2_pos(sn, cs);
}

// The relative pose error between frames a and b: E = (Pa^-1 Pb)^-1 (Qa^-1 Qb), Q the truth, P the estimate with its centres
// scaled by s.  et = |trans E|, ang = the angle of rot E in radians.
__device__ __forceinline__ void traj_rel_error(const TrajFrame& a, const TrajFrame& b, double s, double& et, double& ang) {
#pragma clang fp contract(off)
  double RgaT[9], RwbT[9], Rq[9], Rp[9], RpT[9], E[9];
  traj_transpose(a.Rg, RgaT);
  mat3_mul(RgaT, b.Rg, Rq);
  const double dq0 = b.q[0] - a.q[0], dq1 = b.q[1] - a.q[1], dq2 = b.q[2] - a.q[2];
  const double dp0 = s * (b.C[0] - a.C[0]), dp1 = s * (b.C[1] - a.C[1]), dp2 = s * (b.C[2] - a.C[2]);
  traj_transpose(b.Rw, RwbT);
  mat3_mul(a.Rw, RwbT, Rp);
  double d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    d[i] = dot3(RgaT[3 * i], RgaT[3 * i + 1], RgaT[3 * i + 2], dq0, dq1, dq2) - dot3(a.Rw[3 * i], a.Rw[3 * i + 1], a.Rw[3 * i + 2], dp0, dp1, dp2);
  traj_transpose(Rp, RpT);
  mat3_mul(RpT, Rq, E);
  const double e0 = dot3(RpT[0], RpT[1], RpT[2], d[0], d[1], d[2]), e1 = dot3(RpT[3], RpT[4], RpT[5], d[0], d[1], d[2]);
  const double e2 = dot3(RpT[6], RpT[7], RpT[8], d[0], d[1], d[2]);
  et = sqrt(dot3(e0, e1, e2, e0, e1, e2));
  ang = traj_angle(E);
}

// grid (P), TRAJ_THREADS threads.  mode 0: SE(3), 1: Sim(3), 2: the first valid frame's pose as the origin, 3: that and a scale.
__global__ __launch_bounds__(TRAJ_THREADS) void traj_align_kernel(TrajIn in, int mode, double* __restrict__ sim) {
#pragma clang fp contract(off)
  __shared__ double red[(TRAJ_THREADS / 64) * 11];
  __shared__ int sh_first;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int nf = traj_frames(in, p);
  TrajFrame fr;
  double s = 1.0, R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, nv = 0.0, sig = 0.0;
  int status = TRAJ_OK;
  if (mode <= 1) {
    double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int f = tid; f < nf; f += TRAJ_THREADS)
      if (traj_load(in, p, f, nf, fr)) {
        a[0] = a[0] + 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          a[1 + k] = a[1 + k] + fr.C[k];
          a[4 + k] = a[4 + k] + fr.q[k];
        }
      }
    block_sums<TRAJ_THREADS, 7>(a, red);
    nv = a[0];
    const double mp[3] = {a[1] / nv, a[2] / nv, a[3] / nv}, mq[3] = {a[4] / nv, a[5] / nv, a[6] / nv};
    double b[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // H = sum (q - mq)(p - mp)^T, sum |p - mp|^2, sum |q - mq|^2
    for (int f = tid; f < nf; f += TRAJ_THREADS)
      if (traj_load(in, p, f, nf, fr)) {
        const double dp[3] = {fr.C[0] - mp[0], fr.C[1] - mp[1], fr.C[2] - mp[2]};
        const double dq[3] = {fr.q[0] - mq[0], fr.q[1] - mq[1], fr.q[2] - mq[2]};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) b[3 * i + j] = b[3 * i + j] + dq[i] * dp[j];
        b[9] = b[9] + dot3(dp[0], dp[1], dp[2], dp[0], dp[1], dp[2]);
        b[10] = b[10] + dot3(dq[0], dq[1], dq[2], dq[0], dq[1], dq[2]);
      }
    block_sums<TRAJ_THREADS, 11>(b, red);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 11; ++k) fin = fin && isfinite(b[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) fin = fin && isfinite(mp[k]) && isfinite(mq[k]);
    if (nv < 3.0 || !fin || !(b[9] > 0.0)) {
      status = TRAJ_FEW;
    } else {
      sig = b[9] / nv;
      double G[3][3], V[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          G[i][j] = dot3(b[i], b[3 + i], b[6 + i], b[j], b[3 + j], b[6 + j]);
          V[i][j] = i == j ? 1.0 : 0.0;
        }
      for (int sweep = 0; sweep < TRAJ_JACOBI_SWEEPS; ++sweep) {
        jacobi_rotate<0, 1>(G, V);
        jacobi_rotate<0, 2>(G, V);
        jacobi_rotate<1, 2>(G, V);
      }
      // the columns of the largest and the second-largest diagonal entry, the lowest index on ties
      const double d0 = G[0][0], d1 = G[1][1], d2 = G[2][2];
      const int k0 = d2 > (d1 > d0 ? d1 : d0) ? 2 : (d1 > d0 ? 1 : 0);
      const int ra = k0 == 0 ? 1 : 0, rb = k0 == 2 ? 1 : 2;
      const double da = ra == 1 ? d1 : d0, db = rb == 1 ? d1 : d2;
      const int k1 = db > da ? rb : ra;
      const double w0 = k0 == 0 ? d0 : (k0 == 1 ? d1 : d2), w1 = k1 == 0 ? d0 : (k1 == 1 ? d1 : d2);
      if (!(w1 > TRAJ_COLLINEAR_EPS * w0)) {
        status = TRAJ_COLLINEAR;
      } else {
        double v0[3], v1[3], v2[3], u0[3], u1[3], u2[3], h0[3], h1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          v0[k] = k0 == 0 ? V[k][0] : (k0 == 1 ? V[k][1] : V[k][2]);
          v1[k] = k1 == 0 ? V[k][0] : (k1 == 1 ? V[k][1] : V[k][2]);
        }
        cross3(v0, v1, v2);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          h0[i] = dot3(b[3 * i], b[3 * i + 1], b[3 * i + 2], v0[0], v0[1], v0[2]);
          h1[i] = dot3(b[3 * i], b[3 * i + 1], b[3 * i + 2], v1[0], v1[1], v1[2]);
        }
        const double n0 = sqrt(dot3(h0[0], h0[1], h0[2], h0[0], h0[1], h0[2]));
#pragma unroll
        for (int i = 0; i < 3; ++i) u0[i] = h0[i] / n0;
        const double pj = dot3(h1[0], h1[1], h1[2], u0[0], u0[1], u0[2]);
        const double w[3] = {h1[0] - pj * u0[0], h1[1] - pj * u0[1], h1[2] - pj * u0[2]};
        const double n1 = sqrt(dot3(w[0], w[1], w[2], w[0], w[1], w[2]));
#pragma unroll
        for (int i = 0; i < 3; ++i) u1[i] = w[i] / n1;
        cross3(u0, u1, u2);
        double Rn[9], tr[3], tn[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
          for (int j = 0; j < 3; ++j) Rn[3 * i + j] = dot3(u0[i], u1[i], u2[i], v0[j], v1[j], v2[j]);
          tr[i] = dot3(Rn[3 * i], Rn[3 * i + 1], Rn[3 * i + 2], b[3 * i], b[3 * i + 1], b[3 * i + 2]);
        }
        const double sn = mode == 1 ? ((tr[0] + tr[1]) + tr[2]) / b[9] : 1.0;
        bool ok = isfinite(sn) && sn > 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          tn[i] = mq[i] - sn * dot3(Rn[3 * i], Rn[3 * i + 1], Rn[3 * i + 2], mp[0], mp[1], mp[2]);
          ok = ok && isfinite(tn[i]);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) ok = ok && isfinite(Rn[k]);
        if (ok) {
          s = sn;
#pragma unroll
          for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
          for (int k = 0; k < 3; ++k) t[k] = tn[k];
        } else {
          status = TRAJ_FEW;
        }
      }
    }
  } else {
    if (tid == 0) sh_first = 0x7FFFFFFF;
    __syncthreads();
    double cnt = 0.0;
    int first = 0x7FFFFFFF;
    for (int f = tid; f < nf; f += TRAJ_THREADS)
      if (traj_load(in, p, f, nf, fr)) {
        cnt = cnt + 1.0;
        first = min(first, f);
      }
    if (first != 0x7FFFFFFF) atomicMin(&sh_first, first);
    nv = block_sum<TRAJ_THREADS>(cnt, red);   // (its barriers also publish sh_first)
    const int f0 = sh_first;
    TrajFrame o;
    if (nv < (mode == 3 ? 2.0 : 1.0) || !traj_load(in, p, f0, nf, o)) {
      status = TRAJ_FEW;   // (uniform over the workgroup: every thread holds the same nv and f0)
    } else {
      double Rn[9], c[2] = {0.0, 0.0};
      mat3_mul(o.Rg, o.Rw, Rn);
      double sn = 1.0;
      if (mode == 3) {
        for (int f = tid; f < nf; f += TRAJ_THREADS)
          if (traj_load(in, p, f, nf, fr)) {
            const double dp[3] = {fr.C[0] - o.C[0], fr.C[1] - o.C[1], fr.C[2] - o.C[2]};
            const double dq[3] = {fr.q[0] - o.q[0], fr.q[1] - o.q[1], fr.q[2] - o.q[2]};
            const double r0 = dot3(Rn[0], Rn[1], Rn[2], dp[0], dp[1], dp[2]), r1 = dot3(Rn[3], Rn[4], Rn[5], dp[0], dp[1], dp[2]);
            const double r2 = dot3(Rn[6], Rn[7], Rn[8], dp[0], dp[1], dp[2]);
            c[0] = c[0] + dot3(dq[0], dq[1], dq[2], r0, r1, r2);
            c[1] = c[1] + dot3(r0, r1, r2, r0, r1, r2);
          }
        block_sums<TRAJ_THREADS, 2>(c, red);
        sn = c[0] / c[1];
        sig = c[1] / nv;
      }
      bool ok = isfinite(sn) && sn > 0.0;
      double tn[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        tn[i] = o.q[i] - sn * dot3(Rn[3 * i], Rn[3 * i + 1], Rn[3 * i + 2], o.C[0], o.C[1], o.C[2]);
        ok = ok && isfinite(tn[i]);
      }
      if (ok) {
        s = sn;
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = tn[k];
      } else {
        status = TRAJ_FEW;
      }
    }
  }
  if (tid == 0) {
    double* out = sim + (size_t)p * TRAJ_SIM_WORDS;
    out[0] = s;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[1 + k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[10 + k] = t[k];
    out[13] = nv;
    out[14] = (double)status;
    out[15] = isfinite(sig) ? sig : 0.0;
  }
}

// grid (cdiv(capacity, TRAJ_THREADS), P).  err_t, err_r, valid [P][capacity]: every entry is written.
__global__ __launch_bounds__(TRAJ_THREADS) void traj_ape_kernel(TrajIn in, const double* __restrict__ sim, double* __restrict__ err_t,
                                                                double* __restrict__ err_r, int32_t* __restrict__ valid) {
#pragma clang fp contract(off)
  const int p = blockIdx.y, f = blockIdx.x * TRAJ_THREADS + threadIdx.x;
  if (f >= in.capacity) return;
  const int nf = traj_frames(in, p);
  const double* S = sim + (size_t)p * TRAJ_SIM_WORDS;
  double et = 0.0, er = 0.0;
  int v = 0;
  TrajFrame fr;
  if (S[14] == 0.0 && traj_load(in, p, f, nf, fr)) {
    const double s = S[0];
    double R[9], RwT[9], M[9], RgT[9], E[9], e[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = S[1 + k];
#pragma unroll
    for (int i = 0; i < 3; ++i) e[i] = fr.q[i] - (s * dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], fr.C[0], fr.C[1], fr.C[2]) + S[10 + i]);
    et = sqrt(dot3(e[0], e[1], e[2], e[0], e[1], e[2]));
    traj_transpose(fr.Rw, RwT);
    mat3_mul(R, RwT, M);
    traj_transpose(fr.Rg, RgT);
    mat3_mul(RgT, M, E);
    er = traj_angle(E) * TRAJ_DEG_PER_RAD;
    v = 1;
  }
  const size_t o = (size_t)p * in.capacity + f;
  err_t[o] = et;
  err_r[o] = er;
  valid[o] = v;
}

// The same grid.  scale [P] at scale_stride words (null: 1).  Frame f holds the error between f and f + delta.
__global__ __launch_bounds__(TRAJ_THREADS) void traj_rpe_delta_kernel(TrajIn in, const double* __restrict__ scale, int scale_stride,
                                                                      int delta, double* __restrict__ err_t, double* __restrict__ err_r,
                                                                      int32_t* __restrict__ valid) {
#pragma clang fp contract(off)
  const int p = blockIdx.y, f = blockIdx.x * TRAJ_THREADS + threadIdx.x;
  if (f >= in.capacity) return;
  const int nf = traj_frames(in, p);
  const double s = scale ? scale[(size_t)p * scale_stride] : 1.0;
  double et = 0.0, er = 0.0;
  int v = 0;
  TrajFrame a, b;
  if (traj_load(in, p, f, nf, a) && traj_load(in, p, f + delta, nf, b)) {   // (delta <= capacity <= 2^20: no overflow)
    double ang;
    traj_rel_error(a, b, s, et, ang);
    er = ang * TRAJ_DEG_PER_RAD;
    v = 1;
  }
  const size_t o = (size_t)p * in.capacity + f;
  err_t[o] = et;
  err_r[o] = er;
  valid[o] = v;
}

// The centre of ground-truth row g of problem p, if it is finite.
__device__ __forceinline__ bool traj_gt_centre(const TrajIn& in, int p, int g, double (&c)[3]) {
  const double* gr = in.gt + (size_t)p * in.gt_stride + (size_t)g * TRAJ_GT_WORDS;
  c[0] = gr[3];
  c[1] = gr[7];
  c[2] = gr[11];
  return isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]);
}

// grid (P), TRAJ_THREADS threads.  lengths [n_len], n_len <= TRAJ_MAX_LENGTHS; n_first = cdiv(capacity, step) first frames.
// dist [P][capacity], seg [P][n_first][n_len][4], summary [P][2 + 3 n_len], info [P][TRAJ_INFO_WORDS].
// The scan: thread t owns the frames [t K, (t + 1) K), K = cdiv(n_frames, TRAJ_THREADS); it adds its steps in order, the totals of
// the threads before it in order, and dist[f] = (that base) + (its own running sum).  A frame whose ground-truth row is missing or
// has a centre that is not finite repeats the value before it.
__global__ __launch_bounds__(TRAJ_THREADS) void traj_rpe_segments_kernel(TrajIn in, const double* __restrict__ scale, int scale_stride,
                                                                         const double* __restrict__ lengths, int n_len, int step,
                                                                         int n_first, double* dist, double* seg,
                                                                         double* __restrict__ summary, int32_t* __restrict__ info) {
#pragma clang fp contract(off)
  __shared__ double part[TRAJ_THREADS];
  __shared__ double red[(TRAJ_THREADS / 64) * 3];
  __shared__ int ired[TRAJ_THREADS / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int nf = traj_frames(in, p);
  const double s = scale ? scale[(size_t)p * scale_stride] : 1.0;
  double* D = dist + (size_t)p * in.capacity;
  double* G = seg + (size_t)p * n_first * n_len * 4;
  // the path length
  const int K = (nf + TRAJ_THREADS - 1) / TRAJ_THREADS;
  const int b0 = min(tid * K, nf), b1 = min(b0 + K, nf);
  bool have = false;
  double c[3] = {0.0, 0.0, 0.0}, q[3];
  for (int f = b0 - 1; f >= 0 && b0 < b1 && !have; --f) {   // the last centre before the thread's frames
    const int g = traj_gt_row(in, f);
    if (g >= 0 && traj_gt_centre(in, p, g, q)) {
      have = true;
      c[0] = q[0];
      c[1] = q[1];
      c[2] = q[2];
    }
  }
  double run = 0.0;
  for (int f = b0; f < b1; ++f) {
    const int g = traj_gt_row(in, f);
    if (g >= 0 && traj_gt_centre(in, p, g, q)) {
      if (have) {
        const double d0 = q[0] - c[0], d1 = q[1] - c[1], d2 = q[2] - c[2];
        run = run + sqrt(dot3(d0, d1, d2, d0, d1, d2));
      }
      have = true;
      c[0] = q[0];
      c[1] = q[1];
      c[2] = q[2];
    }
    D[f] = run;
  }
  part[tid] = run;
  __syncthreads();
  double base = 0.0;
  for (int k = 0; k < tid; ++k) base = base + part[k];
  for (int f = b0; f < b1; ++f) D[f] = base + D[f];
  for (int f = nf + tid; f < in.capacity; f += TRAJ_THREADS) D[f] = 0.0;
  __syncthreads();   // (the segments read entries of dist that other threads wrote)
  // the segments
  int c_ok = 0, c_bad = 0, c_none = 0;
  const int items = n_first * n_len;
  for (int i = tid; i < items; i += TRAJ_THREADS) {
    const int k = i / n_len, l = i - k * n_len;
    const int f0 = k * step;   // (k < n_first = cdiv(capacity, step): f0 < capacity + step)
    const double L = lengths[l];
    int f1 = -1;
    double te = 0.0, re = 0.0, len = 0.0;
    if (f0 < nf) {
      const double target = D[f0] + L;
      int lo = f0 + 1, hi = nf;   // the first f in [lo, hi) with dist[f] > target
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (D[mid] > target) hi = mid;
        else lo = mid + 1;
      }
      if (lo < nf) {
        f1 = lo;
        TrajFrame a, b;
        if (traj_load(in, p, f0, nf, a) && traj_load(in, p, f1, nf, b)) {
          double et, ang;
          traj_rel_error(a, b, s, et, ang);
          te = et / L;
          re = ang / L;
          len = L;
          ++c_ok;
        } else {
          ++c_bad;
        }
      } else {
        ++c_none;
      }
    }
    double* row = G + (size_t)i * 4;
    row[0] = (double)f1;
    row[1] = te;
    row[2] = re;
    row[3] = len;   // (0: the segment does not count)
  }
  __syncthreads();   // (the means read rows of seg that other threads wrote)
  double* sum = summary + (size_t)p * (2 + 3 * n_len);
  double tot[3] = {0.0, 0.0, 0.0};
  for (int l = 0; l < n_len; ++l) {
    double a[3] = {0.0, 0.0, 0.0};
    for (int k = tid; k < n_first; k += TRAJ_THREADS) {
      const double* row = G + ((size_t)k * n_len + l) * 4;
      if (row[3] > 0.0) {
        a[0] = a[0] + 1.0;
        a[1] = a[1] + row[1];
        a[2] = a[2] + row[2];
      }
    }
    block_sums<TRAJ_THREADS, 3>(a, red);
#pragma unroll
    for (int e = 0; e < 3; ++e) tot[e] = tot[e] + a[e];
    if (tid == 0) {
      sum[2 + 3 * l] = a[0];
      sum[3 + 3 * l] = a[0] > 0.0 ? a[1] / a[0] : 0.0;
      sum[4 + 3 * l] = a[0] > 0.0 ? a[2] / a[0] : 0.0;
    }
  }
  const int n_ok = block_sum<TRAJ_THREADS>(c_ok, ired);
  const int n_bad = block_sum<TRAJ_THREADS>(c_bad, ired);
  const int n_none = block_sum<TRAJ_THREADS>(c_none, ired);
  if (tid == 0) {
    sum[0] = tot[0] > 0.0 ? tot[1] / tot[0] : 0.0;
    sum[1] = tot[0] > 0.0 ? tot[2] / tot[0] : 0.0;
    int32_t* o = info + (size_t)p * TRAJ_INFO_WORDS;
    o[0] = n_ok;
    o[1] = n_bad;
    o[2] = n_none;
    o[3] = nf > 0 ? 1 + (nf - 1) / step : 0;
  }
}

// grid (P), TRAJ_THREADS threads.  err, valid [P][capacity]; the errors of valid entries are non-negative and finite, so their bit
// patterns order as they do.  stats [P][TRAJ_STATS_WORDS].
__global__ __launch_bounds__(TRAJ_THREADS) void traj_stats_kernel(const double* __restrict__ err, const int32_t* __restrict__ valid,
                                                                  int capacity, double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double red[(TRAJ_THREADS / 64) * 3];
  __shared__ int hist[256];
  __shared__ unsigned long long sh_prefix, sh_min, sh_max;
  __shared__ int sh_remaining;
  const int p = blockIdx.x, tid = threadIdx.x;
  const double* E = err + (size_t)p * capacity;
  const int32_t* V = valid + (size_t)p * capacity;
  double* out = stats + (size_t)p * TRAJ_STATS_WORDS;
  if (tid == 0) {
    sh_min = ~0ull;
    sh_max = 0ull;
  }
  __syncthreads();
  double a[3] = {0.0, 0.0, 0.0};
  unsigned long long umin = ~0ull, umax = 0ull;
  for (int i = tid; i < capacity; i += TRAJ_THREADS)
    if (V[i]) {
      const double x = E[i];
      a[0] = a[0] + 1.0;
      a[1] = a[1] + x;
      a[2] = a[2] + x * x;
      const unsigned long long u = (unsigned long long)__double_as_longlong(x);
      umin = u < umin ? u : umin;
      umax = u > umax ? u : umax;
    }
  if (a[0] > 0.0) {
    atomicMin(&sh_min, umin);
    atomicMax(&sh_max, umax);
  }
  block_sums<TRAJ_THREADS, 3>(a, red);   // (its barriers also publish sh_min and sh_max)
  const int n = (int)a[0];
  if (n == 0) {   // (uniform)
    if (tid < TRAJ_STATS_WORDS) out[tid] = 0.0;
    return;
  }
  const double mean = a[1] / a[0];
  double b[1] = {0.0};
  for (int i = tid; i < capacity; i += TRAJ_THREADS)
    if (V[i]) {
      const double d = E[i] - mean;
      b[0] = b[0] + d * d;
    }
  block_sums<TRAJ_THREADS, 1>(b, red);
  // the order statistics (n - 1) / 2 and n / 2, counted from 0: most significant digit first
  double med[2];
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const int rank = which == 0 ? (n - 1) / 2 : n / 2;
    if (tid == 0) {
      sh_prefix = 0ull;
      sh_remaining = rank + 1;
    }
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      hist[tid] = 0;   // (TRAJ_THREADS == 256)
      __syncthreads();
      const unsigned long long prefix = sh_prefix;
      for (int i = tid; i < capacity; i += TRAJ_THREADS)
        if (V[i]) {
          const unsigned long long u = (unsigned long long)__double_as_longlong(E[i]);
          if (pass == 0 || (u >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((u >> shift) & 255ull)], 1);
        }
      __syncthreads();
      if (tid == 0) {
        int rem = sh_remaining, d = 0;
        while (d < 255 && hist[d] < rem) rem -= hist[d++];
        sh_remaining = rem;
        sh_prefix = (prefix << 8) | (unsigned long long)d;
      }
      __syncthreads();
    }
    med[which] = __longlong_as_double((long long)sh_prefix);
    __syncthreads();   // (thread 0 resets the prefix for the second statistic)
  }
  if (tid == 0) {
    out[0] = a[0];
    out[1] = sqrt(a[2] / a[0]);
    out[2] = mean;
    out[3] = sqrt(b[0] / a[0]);
    out[4] = __longlong_as_double((long long)sh_min);
    out[5] = __longlong_as_double((long long)sh_max);
    out[6] = 0.5 * (med[0] + med[1]);
    out[7] = a[2];
  }
}

}  // namespace sspk
