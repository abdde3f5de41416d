// Absolute pose from landmarks: the camera of a frame from 3-D to 2-D correspondences (landmark rows of
// section 26 joined with the matches of the next frame) by a P3P RANSAC, a Gauss-Newton refit, and the repair of a trajectory row
// the two-view chain of section 24 could not determine.  Camera model of section 26: y = Rw (X - C), u = fx y0 / y2 + cx.  The
// rules are restated in numpy by tests/pnp_ref.py; everything here is fp64 with contraction off, in the parenthesisation of that
// file.
//   landmark_corr_kernel   one workgroup: "point of the previous frame -> lowest landmark row" in LDS (atomicMin: no order to
//                          depend on), then one correspondence row (X, Y, Z, px, py, landmark row, valid, 0) per match row
//   pnp_hypotheses_kernel  grid (groups, problems): workgroup g solves and scores a contiguous slice of the PNP_HYPOTHESES
//                          hypotheses, one per lane, and writes one (score, hypothesis) key.  Every lane scores the same row at the
//                          same time, so the row's address is uniform over the wavefront: the rows are read where they lie (a
//                          broadcast read served by the scalar cache / L2), not staged
//   pnp_finish_kernel      grid (problems): the winner over the keys (a maximum: no order to depend on), its pose again, its mask,
//                          PNP_GN_STEPS Gauss-Newton steps on (rotation, translation) with 27 moments reduced in
//                          block_sum's fixed order (block_sums: the same order, one pair of barriers for all 27) and a
//                          6x6 solve by complete pivoting, the final mask, rms, status
//   pose_repair_kernel     a thread per sequence: the newest trajectory row and the chain state rewritten from an absolute pose
// The quartic's roots are bracketed by hand: the quadratic g'' by formula, three brackets of the cubic g', four of the quartic;
// every coefficient index is a constant, so the polynomials and the 6x7 system live in registers.
// Needs: geom_blocks.hip.h, pose_kernels.hip.h (POSE_ROW_WORDS), landmark_kernels.hip.h (LM_WORDS).
#pragma once

namespace sspk {

#define PNP_THREADS 256
#define PNP_HYPOTHESES 512
#define PNP_MAX_GROUPS 64
#define PNP_MAX_CAP 4096
#define PNP_V_MAX 32.0
#define PNP_BISECTIONS 64
#define PNP_GN_STEPS 4
#define PNP_PIVOT_EPS 1e-12
#define PNP_FRAME_EPS 1e-12
#define PNP_CORR_WORDS 8       // X, Y, Z, px, py, landmark row, valid, 0
#define PNP_SCALE_FRACTION (1.0 / 64.0)
#define PNP_FLAG_ABSOLUTE 4
#define PNP_NO_OWNER 0x7FFFFFFF

struct PnpIntr {
  double fx, fy, cx, cy;
};

// ---- what the joins and the repairs of the absolute pose, the world map and the loop closure share ----
// The "point of the newest frame -> lowest landmark row" table in LDS: owner [point_cap], PNP_NO_OWNER where no landmark carries the
// point.  Called by every thread of a block of `threads`; the table is complete when it returns.
__device__ __forceinline__ void pnp_owner_table(int* owner, int point_cap, const double* __restrict__ landmarks, int nl, int tid,
                                                int threads) {
  for (int k = tid; k < point_cap; k += threads) owner[k] = PNP_NO_OWNER;
  __syncthreads();
  for (int r = tid; r < nl; r += threads) {
    const double w = landmarks[(size_t)r * LM_WORDS + 7];
    if (isfinite(w) && w >= 0.0 && w < (double)point_cap) atomicMin(&owner[(int)w], r);   // the lowest row wins
  }
  __syncthreads();
}

__device__ __forceinline__ bool pnp_finite5(const double (&v)[5]) {
  return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]) && isfinite(v[4]);
}

// One row of corr [cap][PNP_CORR_WORDS]: (X, Y, Z, px, py), the row they came from and 1 when valid, zeros otherwise.
__device__ __forceinline__ void pnp_store_corr(double* __restrict__ o, const double (&v)[5], int row, bool valid) {
#pragma unroll
  for (int c = 0; c < 5; ++c) o[c] = valid ? v[c] : 0.0;
  o[5] = valid ? (double)row : 0.0;
  o[6] = valid ? 1.0 : 0.0;
  o[7] = 0.0;
}

// Rw [9] and C [3] of one absolute pose; true when all twelve values are finite.
__device__ __forceinline__ bool pnp_load_pose(const double* __restrict__ rw_in, const double* __restrict__ c_in, double (&Rw)[9],
                                              double (&C)[3]) {
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    Rw[k] = rw_in[k];
    fin = fin && isfinite(Rw[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    C[k] = c_in[k];
    fin = fin && isfinite(C[k]);
  }
  return fin;
}

// The rewrite of trajectory row n - 1 (`row`, flags `flags`) and the chain state `st` from the absolute pose (Rw, C): tw = -(Rw C);
// the scale becomes the step from the previous row's centre when that is finite and longer than PNP_SCALE_FRACTION of the carried
// scale (the carried-scale flag is then dropped, otherwise kept); the row's flags become that bit | set_flags.
__device__ __forceinline__ void pnp_rewrite_row(double* __restrict__ st, double* __restrict__ row, int n, int flags,
                                                const double (&Rw)[9], const double (&C)[3], int set_flags) {
#pragma clang fp contract(off)
  double tw[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) tw[i] = -dot3(Rw[3 * i], Rw[3 * i + 1], Rw[3 * i + 2], C[0], C[1], C[2]);
  double s = st[1];
  int keep = flags & 2;
  if (n >= 2) {
    const double* prev = row - POSE_ROW_WORDS;
    const double d0 = C[0] - prev[9], d1 = C[1] - prev[10], d2 = C[2] - prev[11];
    const double len = sqrt(dot3(d0, d1, d2, d0, d1, d2));
    if (isfinite(len) && len > PNP_SCALE_FRACTION * s) {
      s = len;
      keep = 0;
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) row[k] = st[2 + k] = Rw[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    row[9 + k] = C[k];
    st[11 + k] = tw[k];
  }
  row[12] = st[1] = s;
  row[14] = (double)(keep | set_flags);
}

// grid (1), 256 threads, dynamic LDS point_cap ints.  landmarks [row_cap][LM_WORDS], match [cap][3] rows (i, j, d) of the pair
// (previous, new), pts_new [point_cap][pt_stride] rows starting (x, y).  corr [cap][PNP_CORR_WORDS]; n_out [2] = rows, valid rows.
__global__ __launch_bounds__(PNP_THREADS) void landmark_corr_kernel(const double* __restrict__ landmarks,
                                                                    const int32_t* __restrict__ n_landmarks, int row_cap,
                                                                    const float* __restrict__ match, const int32_t* __restrict__ n_match,
                                                                    int cap, const double* __restrict__ pts_new, int pt_stride,
                                                                    int point_cap, double* __restrict__ corr, int32_t* __restrict__ n_out) {
  extern __shared__ int pnp_owner[];
  __shared__ double red[PNP_THREADS / 64];
  const int tid = threadIdx.x;
  pnp_owner_table(pnp_owner, point_cap, landmarks, min(max(n_landmarks[0], 0), row_cap), tid, PNP_THREADS);
  const int n = min(max(n_match[0], 0), cap);
  double cnt = 0.0;
  for (int k = tid; k < cap; k += PNP_THREADS) {
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int r = PNP_NO_OWNER;
    bool valid = false;
    if (k < n) {
      const int i = min(max((int)match[(size_t)k * 3], 0), point_cap - 1), j = min(max((int)match[(size_t)k * 3 + 1], 0), point_cap - 1);
      r = pnp_owner[i];
      if (r != PNP_NO_OWNER) {
        const double* lm = landmarks + (size_t)r * LM_WORDS;
        const double* px = pts_new + (size_t)j * pt_stride;
        v[0] = lm[1];
        v[1] = lm[2];
        v[2] = lm[3];
        v[3] = px[0];
        v[4] = px[1];
        valid = pnp_finite5(v);
      }
    }
    pnp_store_corr(corr + (size_t)k * PNP_CORR_WORDS, v, r, valid);
    cnt = cnt + (valid ? 1.0 : 0.0);
  }
  const double total = block_sum<PNP_THREADS>(cnt, red);   // (a count: exact)
  if (tid == 0) {
    n_out[0] = n;
    n_out[1] = (int)total;
  }
}

__device__ __forceinline__ void pnp_bearing(double px, double py, PnpIntr K, double (&f)[3]) {
#pragma clang fp contract(off)
  const double x = (px - K.cx) / K.fx, y = (py - K.cy) / K.fy;
  const double nrm = sqrt(dot3(x, y, 1.0, x, y, 1.0));
  f[0] = x / nrm;
  f[1] = y / nrm;
  f[2] = 1.0 / nrm;
}

template <int N>
__device__ __forceinline__ double pnp_horner(const double (&c)[N], double v) {
#pragma clang fp contract(off)
  double acc = c[N - 1];
#pragma unroll
  for (int k = N - 2; k >= 0; --k) acc = acc * v + c[k];
  return acc;
}

// PNP_BISECTIONS halvings of [lo, hi], keeping the half with the sign change; change = there was one.
template <int N>
__device__ __forceinline__ double pnp_bisect(const double (&c)[N], double lo, double hi, bool& change) {
#pragma clang fp contract(off)
  const bool slo = pnp_horner(c, lo) < 0.0;
  change = slo != (pnp_horner(c, hi) < 0.0);
#pragma unroll 1
  for (int it = 0; it < PNP_BISECTIONS; ++it) {
    const double mid = 0.5 * (lo + hi);
    const bool same = (pnp_horner(c, mid) < 0.0) == slo;
    lo = same ? mid : lo;
    hi = same ? hi : mid;
  }
  return 0.5 * (lo + hi);
}

__device__ __forceinline__ double pnp_clamp(double x) {
  return isfinite(x) ? (x < 0.0 ? 0.0 : (x > PNP_V_MAX ? PNP_V_MAX : x)) : 0.0;
}

// Orthonormal frame of the triangle with the edges e1, e2 from its first corner.  false: collinear or coincident corners.
__device__ __forceinline__ bool pnp_frame(const double (&e1)[3], const double (&e2)[3], double (&w1)[3], double (&w2)[3], double (&w3)[3]) {
#pragma clang fp contract(off)
  double n[3];
  cross3(e1, e2, n);
  const double l1 = dot3(e1[0], e1[1], e1[2], e1[0], e1[1], e1[2]), l2 = dot3(e2[0], e2[1], e2[2], e2[0], e2[1], e2[2]);
  const double ln = dot3(n[0], n[1], n[2], n[0], n[1], n[2]);
  const double s1 = sqrt(l1), sn = sqrt(ln);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w1[k] = e1[k] / s1;
    w3[k] = n[k] / sn;
  }
  cross3(w3, w1, w2);
  return isfinite(ln) && ln > PNP_FRAME_EPS * (l1 * l2);
}

// Squared reprojection error of X against the pixel under (R, C); front = the depth is finite and positive.  The same arithmetic
// as project (geom_blocks.hip.h), written out: keep the two in step.
__device__ __forceinline__ double pnp_view(const double (&R)[9], const double (&C)[3], double X0, double X1, double X2, double px,
                                           double py, PnpIntr K, bool& front) {
#pragma clang fp contract(off)
  const double q0 = X0 - C[0], q1 = X1 - C[1], q2 = X2 - C[2];
  const double y0 = dot3(R[0], R[1], R[2], q0, q1, q2), y1 = dot3(R[3], R[4], R[5], q0, q1, q2);
  const double y2 = dot3(R[6], R[7], R[8], q0, q1, q2);
  const double r0 = (K.fx * (y0 / y2) + K.cx) - px, r1 = (K.fy * (y1 / y2) + K.cy) - py;
  front = isfinite(y2) && y2 > 0.0;
  return r0 * r0 + r1 * r1;
}

// The pose of a sample: rows 0..2 give up to four solutions, row 3 picks the one with the smallest squared reprojection error
// (the lowest root index on ties).  q[i] = (X, Y, Z, px, py) of row i.  false: no solution.
__device__ __forceinline__ bool pnp_p3p(const double (&q)[4][5], PnpIntr K, double (&Rb)[9], double (&Cb)[3]) {
#pragma clang fp contract(off)
  double f0[3], f1[3], f2[3];
  pnp_bearing(q[0][3], q[0][4], K, f0);
  pnp_bearing(q[1][3], q[1][4], K, f1);
  pnp_bearing(q[2][3], q[2][4], K, f2);
  double d23[3], d13[3], d12[3], e1[3], e2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    d23[c] = q[1][c] - q[2][c];
    d13[c] = q[0][c] - q[2][c];
    d12[c] = q[0][c] - q[1][c];
    e1[c] = q[1][c] - q[0][c];
    e2[c] = q[2][c] - q[0][c];
  }
  const double aa = dot3(d23[0], d23[1], d23[2], d23[0], d23[1], d23[2]);
  const double bb = dot3(d13[0], d13[1], d13[2], d13[0], d13[1], d13[2]);
  const double cc = dot3(d12[0], d12[1], d12[2], d12[0], d12[1], d12[2]);
  const double ca = dot3(f1[0], f1[1], f1[2], f2[0], f2[1], f2[2]);
  const double cb = dot3(f0[0], f0[1], f0[2], f2[0], f2[1], f2[2]);
  const double cg = dot3(f0[0], f0[1], f0[2], f1[0], f1[1], f1[2]);
  // u = s2 / s1 = N(v) / M(v), v = s3 / s1; the quartic g(v) = N^2 - 2 cos(gamma) N M + Q M^2
  const double A = aa / bb, Cc = cc / bb;
  const double Kd = A - Cc;
  const double n0 = -1.0 - Kd, n1 = (2.0 * Kd) * cb, n2 = 1.0 - Kd;
  const double m0 = -2.0 * cg, m1 = 2.0 * ca;
  const double q0 = 1.0 - Cc, q1 = (2.0 * Cc) * cb, q2 = -Cc;
  const double NN[5] = {n0 * n0, 2.0 * (n0 * n1), 2.0 * (n0 * n2) + n1 * n1, 2.0 * (n1 * n2), n2 * n2};
  const double NM[4] = {n0 * m0, n0 * m1 + n1 * m0, n1 * m1 + n2 * m0, n2 * m1};
  const double MM[3] = {m0 * m0, 2.0 * (m0 * m1), m1 * m1};
  const double QM[5] = {q0 * MM[0], q0 * MM[1] + q1 * MM[0], (q0 * MM[2] + q1 * MM[1]) + q2 * MM[0], q1 * MM[2] + q2 * MM[1],
                        q2 * MM[2]};
  const double tc = 2.0 * cg;
  double g[5];
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] = (NN[k] - tc * NM[k]) + QM[k];
  g[4] = NN[4] + QM[4];
  double big = fabs(g[0]);
#pragma unroll
  for (int k = 1; k < 5; ++k) big = fabs(g[k]) > big ? fabs(g[k]) : big;
  const bool ok_q = isfinite(big) && big > 0.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) g[k] = g[k] / big;
  // the roots of g'' by formula, those of g' between them, those of g between those
  const double d[4] = {g[1], 2.0 * g[2], 3.0 * g[3], 4.0 * g[4]};
  const double e0 = d[1], e1q = 2.0 * d[2], e2q = 3.0 * d[3];
  const double sq = sqrt(e1q * e1q - 4.0 * (e2q * e0));
  const double ra = pnp_clamp((-e1q - sq) / (2.0 * e2q)), rb = pnp_clamp((-e1q + sq) / (2.0 * e2q));
  const double c_lo = rb < ra ? rb : ra, c_hi = rb < ra ? ra : rb;
  bool ch;
  double r;
  r = pnp_bisect(d, 0.0, c_lo, ch);
  const double k0 = ch ? r : 0.0;
  r = pnp_bisect(d, c_lo, c_hi, ch);
  const double k1 = ch ? r : c_lo;
  r = pnp_bisect(d, c_hi, PNP_V_MAX, ch);
  const double k2 = ch ? r : c_hi;
  double root[4];
  bool valid[4];
  root[0] = pnp_bisect(g, 0.0, k0, valid[0]);
  root[1] = pnp_bisect(g, k0, k1, valid[1]);
  root[2] = pnp_bisect(g, k1, k2, valid[2]);
  root[3] = pnp_bisect(g, k2, PNP_V_MAX, valid[3]);
  double w1[3], w2[3], w3[3];
  const bool ok_w = pnp_frame(e1, e2, w1, w2, w3);
  double best = __longlong_as_double(0x7ff0000000000000ll);
  bool found = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) Rb[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) Cb[k] = 0.0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const double v = root[s];
    const double D = (1.0 + v * v) - (2.0 * v) * cb;
    const double u = ((n0 + n1 * v) + n2 * (v * v)) / (m0 + m1 * v);
    bool ok = valid[s] && ok_q && ok_w && isfinite(u) && u > 0.0 && isfinite(D) && D > 0.0 && v > 0.0;
    const double s1 = sqrt(bb / D);
    const double s2 = u * s1, s3 = v * s1;
    double Y1[3], a1[3], a2[3], c1[3], c2[3], c3[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Y1[c] = s1 * f0[c];
      a1[c] = s2 * f1[c] - Y1[c];
      a2[c] = s3 * f2[c] - Y1[c];
    }
    ok = pnp_frame(a1, a2, c1, c2, c3) && ok;
    double R[9], C[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[3 * i + j] = (c1[i] * w1[j] + c2[i] * w2[j]) + c3[i] * w3[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) C[j] = q[0][j] - dot3(R[j], R[3 + j], R[6 + j], Y1[0], Y1[1], Y1[2]);
    bool front;
    const double e4 = pnp_view(R, C, q[3][0], q[3][1], q[3][2], q[3][3], q[3][4], K, front);
    const bool take = ok && front && isfinite(e4) && e4 < best;
    best = take ? e4 : best;
    found = found || take;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rb[k] = take ? R[k] : Rb[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Cb[k] = take ? C[k] : Cb[k];
  }
  return found;
}

// Hypotheses tried for n rows: none below 4, the one direct solve at 4, PNP_HYPOTHESES above.
__device__ __forceinline__ int pnp_total(int n) { return n < 4 ? 0 : (n == 4 ? 1 : PNP_HYPOTHESES); }

// Hypothesis h of a problem: 4 distinct valid rows from the counter-based stream (sample_distinct; a draw that hits an
// invalid row is redrawn too), then the minimal solve.  rows [n][PNP_CORR_WORDS].  false = invalid.
__device__ __forceinline__ bool pnp_hypothesis(const double* __restrict__ rows, int n, uint64_t seed, int h, PnpIntr K, double (&R)[9],
                                               double (&C)[3]) {
  int id[4];
  sample_distinct(seed, h, n, id, [rows](int v) { return rows[(size_t)v * PNP_CORR_WORDS + 6] != 0.0; });
  bool usable = true;
  double q[4][5];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double* row = rows + (size_t)id[k] * PNP_CORR_WORDS;
#pragma unroll
    for (int j = 0; j < k; ++j) usable = usable && id[k] != id[j];
    usable = usable && row[6] != 0.0;
#pragma unroll
    for (int c = 0; c < 5; ++c) q[k][c] = row[c];
  }
  const bool found = pnp_p3p(q, K, R, C);
  return usable && found;
}

__device__ __forceinline__ PnpIntr pnp_intr_of(const double* __restrict__ intr, int n_intr, int p) {
  const double* k = intr + (size_t)(n_intr == 1 ? 0 : p) * 4;
  return PnpIntr{k[0], k[1], k[2], k[3]};
}

// grid (groups, problems).  corr [problems][cap][PNP_CORR_WORDS], intr [n_intr][4] (n_intr = 1 or problems).  keys
// [problems][groups]: key_of(score, h) of the best valid hypothesis of the slice [g * per, (g + 1) * per),
// per = ceil(PNP_HYPOTHESES / groups); 0 = none.
__global__ __launch_bounds__(PNP_THREADS) void pnp_hypotheses_kernel(const double* __restrict__ corr, const int32_t* __restrict__ n_in,
                                                                     int cap, const double* __restrict__ intr, int n_intr,
                                                                     const uint64_t* __restrict__ seeds, double thresh,
                                                                     uint64_t* __restrict__ keys) {
#pragma clang fp contract(off)
  __shared__ uint64_t best_key[PNP_THREADS / 64];
  const int g = blockIdx.x, groups = gridDim.x, p = blockIdx.y, tid = threadIdx.x;
  const int n = min(max(n_in[p], 0), cap);
  const int per = (PNP_HYPOTHESES + groups - 1) / groups;
  const int lo = g * per, hi = min(lo + per, pnp_total(n));
  if (lo >= hi) {  // (uniform over the workgroup)
    if (tid == 0) keys[(size_t)p * groups + g] = 0;
    return;
  }
  const double* rows = corr + (size_t)p * cap * PNP_CORR_WORDS;
  const PnpIntr K = pnp_intr_of(intr, n_intr, p);
  const uint64_t seed = seeds[p];
  const double t2 = thresh * thresh;
  uint64_t key = 0;
  for (int base = lo; base < hi; base += PNP_THREADS) {   // (uniform trip count: the scoring loop below is uniform too)
    const int h = base + tid;
    double R[9], C[3];
    const bool ok = pnp_hypothesis(rows, n, seed, h < hi ? h : lo, K, R, C) && h < hi;
    int sc = 0;
#pragma unroll 4
    for (int i = 0; i < n; ++i) {   // (no branch: four rows' divisions are in flight at a time)
      const double* row = rows + (size_t)i * PNP_CORR_WORDS;   // the same address in every lane
      bool front;
      const double e = pnp_view(R, C, row[0], row[1], row[2], row[3], row[4], K, front);
      sc += (row[6] != 0.0 && front && e <= t2) ? 1 : 0;
    }
    // key_of and, below, publish_wave_keys / max_wave_key (geom_blocks.hip.h), written out: the same rules, keep them in step
    const uint64_t k = ((uint64_t)(sc + 1) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)h);
    key = (ok && k > key) ? k : key;
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
    for (int w = 1; w < PNP_THREADS / 64; ++w) key = best_key[w] > key ? best_key[w] : key;
    keys[(size_t)p * groups + g] = key;
  }
}

// x of A x = b (A in a[r][0..5], b in a[r][6]) by complete pivoting over the columns 0..5 (pivot_step).  false: a pivot is <=
// PNP_PIVOT_EPS in magnitude (or NaN) or x is not finite.
__device__ __forceinline__ bool pnp_solve6(double (&a)[6][7], double (&x)[6]) {
#pragma clang fp contract(off)
  bool ok = true;
  int perm[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) perm[c] = c;
  pivot_step<0>(a, perm, ok, PNP_PIVOT_EPS);
  pivot_step<1>(a, perm, ok, PNP_PIVOT_EPS);
  pivot_step<2>(a, perm, ok, PNP_PIVOT_EPS);
  pivot_step<3>(a, perm, ok, PNP_PIVOT_EPS);
  pivot_step<4>(a, perm, ok, PNP_PIVOT_EPS);
  pivot_step<5>(a, perm, ok, PNP_PIVOT_EPS);
  double y[6];
#pragma unroll
  for (int k = 5; k >= 0; --k) {
    double s = a[k][6];
#pragma unroll
    for (int c = k + 1; c < 6; ++c) s = s - a[k][c] * y[c];
    y[k] = s / a[k][k];
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) v = perm[c] == j ? y[c] : v;
    x[j] = v;
    ok = ok && isfinite(v);
  }
  return ok;
}

// The mask of the rows under (R, C) into `mask`, the squared errors of the masked rows summed; returns the count.
__device__ __forceinline__ double pnp_mask_of(const double* __restrict__ rows, int n, const double (&R)[9], const double (&C)[3], PnpIntr K,
                                              double t2, uint8_t* mask, double* red, double& ss) {
#pragma clang fp contract(off)
  double c = 0.0, part = 0.0;
  for (int i = threadIdx.x; i < n; i += PNP_THREADS) {
    const double* row = rows + (size_t)i * PNP_CORR_WORDS;
    bool front;
    const double e = pnp_view(R, C, row[0], row[1], row[2], row[3], row[4], K, front);
    const bool in = row[6] != 0.0 && front && e <= t2;
    mask[i] = in;
    c = c + (in ? 1.0 : 0.0);
    if (in) part = part + e;
  }
  double both[2] = {part, c};
  block_sums<PNP_THREADS>(both, red);  // (the barriers inside also publish the mask)
  ss = both[0];
  return both[1];
}

// grid (problems).  Per problem: rw_out [9], c_out [3], mask_out [cap], n_inl_out, winner_out, rms_out, status_out.
__global__ __launch_bounds__(PNP_THREADS) void pnp_finish_kernel(const double* __restrict__ corr, const int32_t* __restrict__ n_in, int cap,
                                                                 const double* __restrict__ intr, int n_intr,
                                                                 const uint64_t* __restrict__ seeds, double thresh, int min_inliers,
                                                                 int groups, const uint64_t* __restrict__ keys,
                                                                 double* __restrict__ rw_out, double* __restrict__ c_out,
                                                                 uint8_t* __restrict__ mask_out, int32_t* __restrict__ n_inl_out,
                                                                 int32_t* __restrict__ winner_out, double* __restrict__ rms_out,
                                                                 int32_t* __restrict__ status_out) {
#pragma clang fp contract(off)
  __shared__ double red[(PNP_THREADS / 64) * 27];
  __shared__ uint8_t s_mask0[PNP_MAX_CAP];
  __shared__ uint8_t s_mask1[PNP_MAX_CAP];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(n_in[p], 0), cap);
  const double* rows = corr + (size_t)p * cap * PNP_CORR_WORDS;
  const PnpIntr K = pnp_intr_of(intr, n_intr, p);
  const double t2 = thresh * thresh;
  const int need = min_inliers > 4 ? min_inliers : 4;
  const uint64_t key = max_group_key(keys, p, groups);
  const int winner = hypothesis_of(key);
  bool valid = key != 0 && score_of(key) >= need;   // (uniform over the workgroup, as everything below)
  double R0[9], C0[3], R[9], C[3], t[3];
  double k0 = 0.0, k1 = 0.0, ss0 = 0.0, ss1 = 0.0;
  bool refined = false;
  if (valid) valid = pnp_hypothesis(rows, n, seeds[p], winner, K, R0, C0);
  if (valid) {
    k0 = pnp_mask_of(rows, n, R0, C0, K, t2, s_mask0, red, ss0);
    valid = (int)k0 >= need;
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = R0[k];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = -dot3(R0[3 * i], R0[3 * i + 1], R0[3 * i + 2], C0[0], C0[1], C0[2]);
#pragma unroll 1
    for (int step = 0; step < PNP_GN_STEPS; ++step) {
      // the 21 + 6 moments of y <- Cay(w) y + dt over the winner's inliers
      double mom[27];
#pragma unroll
      for (int e = 0; e < 27; ++e) mom[e] = 0.0;
      for (int i = tid; i < n; i += PNP_THREADS) {
        if (!s_mask0[i]) continue;
        const double* row = rows + (size_t)i * PNP_CORR_WORDS;
        const double y0 = dot3(R[0], R[1], R[2], row[0], row[1], row[2]) + t[0];
        const double y1 = dot3(R[3], R[4], R[5], row[0], row[1], row[2]) + t[1];
        const double y2 = dot3(R[6], R[7], R[8], row[0], row[1], row[2]) + t[2];
        const double un = y0 / y2, vn = y1 / y2;
        const double r0 = (K.fx * un + K.cx) - row[3], r1 = (K.fy * vn + K.cy) - row[4];
        const double fa = K.fx / y2, fb = K.fy / y2;
        const double j0[6] = {fa * (0.0 - un * y1), fa * (y2 + un * y0), fa * (0.0 - y1), fa, 0.0, fa * (0.0 - un)};
        const double j1[6] = {fb * ((0.0 - y2) - vn * y1), fb * (vn * y0), fb * y0, 0.0, fb, fb * (0.0 - vn)};
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b, ++e) mom[e] = mom[e] + (j0[a] * j0[b] + j1[a] * j1[b]);
#pragma unroll
        for (int a = 0; a < 6; ++a) mom[21 + a] = mom[21 + a] + (j0[a] * r0 + j1[a] * r1);
      }
      block_sums<PNP_THREADS>(mom, red);
      double a[6][7], delta[6];
      {
        int e = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = r; c < 6; ++c, ++e) a[r][c] = a[c][r] = mom[e];
#pragma unroll
        for (int r = 0; r < 6; ++r) a[r][6] = -mom[21 + r];
      }
      if (pnp_solve6(a, delta)) cayley_update(R, t, delta);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) C[j] = -dot3(R[j], R[3 + j], R[6 + j], t[0], t[1], t[2]);
    k1 = pnp_mask_of(rows, n, R, C, K, t2, s_mask1, red, ss1);
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) fin = fin && isfinite(R[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) fin = fin && isfinite(C[k]);
    refined = fin && k1 >= k0;
  }
  const uint8_t* mask = refined ? s_mask1 : s_mask0;
  uint8_t* mo = mask_out + (size_t)p * cap;
  for (int i = tid; i < cap; i += PNP_THREADS) mo[i] = (valid && i < n) ? mask[i] : 0;
  if (tid == 0) {
    const double cnt = refined ? k1 : k0;
#pragma unroll
    for (int k = 0; k < 9; ++k)
      rw_out[(size_t)p * 9 + k] = valid ? (refined ? R[k] : R0[k]) : ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0);
#pragma unroll
    for (int k = 0; k < 3; ++k) c_out[(size_t)p * 3 + k] = valid ? (refined ? C[k] : C0[k]) : 0.0;
    n_inl_out[p] = valid ? (int)cnt : 0;
    winner_out[p] = valid ? winner : -1;
    rms_out[p] = valid ? sqrt((refined ? ss1 : ss0) / (2.0 * cnt)) : 0.0;
    status_out[p] = valid ? 0 : 1;
  }
}

// grid (cdiv(n_seq, 64)), 64 threads: sequence q's newest trajectory row and chain state from its absolute pose.  Acts when the
// table holds 1 <= n < capacity rows (a full table is left alone: its last row need not be the newest frame's), row n - 1 carries
// flag bit 0 or 1, and the absolute pose has status 0 and is finite; otherwise nothing is written.
__global__ __launch_bounds__(64) void pose_repair_kernel(const double* __restrict__ rw_in, const double* __restrict__ c_in,
                                                         const int32_t* __restrict__ status_in, int n_seq, double* __restrict__ state,
                                                         double* __restrict__ table, int capacity) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_seq) return;
  double* st = state + (size_t)q * POSE_STATE_WORDS;
  const double nf = st[0];
  const int n = (nf >= 0.0 && nf < 2147483647.0) ? (int)nf : 0;
  if (n < 1 || n >= capacity || status_in[q] != 0) return;
  double* row = table + ((size_t)q * capacity + (n - 1)) * POSE_ROW_WORDS;
  const int flags = (int)row[14];
  double Rw[9], C[3];
  const bool fin = pnp_load_pose(rw_in + (size_t)q * 9, c_in + (size_t)q * 3, Rw, C);
  if (!(flags & 3) || !fin) return;
  pnp_rewrite_row(st, row, n, flags, Rw, C, PNP_FLAG_ABSOLUTE);
}

}  // namespace sspk
