// Device building blocks the fp64 geometry headers share: one definition of each, no kernel.  Everything is
// compiled with contraction off, and the operation order of every block is part of the contract with tests/*_ref.py, which restate
// it in numpy: a change of order here changes result bits in every header that calls the block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sspk {

#define GEOM_SAMPLE_DRAWS 64

// ---- 3-vectors and 3x3 matrices ----
__device__ __forceinline__ double dot3(double p0, double p1, double p2, double q0, double q1, double q2) {
#pragma clang fp contract(off)
  return (p0 * q0 + p1 * q1) + p2 * q2;
}

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// c = a @ b for 3x3 row-major matrices: every element ((a0*b0 + a1*b1) + a2*b2), each product and each sum rounded.
__device__ __forceinline__ void mat3_mul(const double (&a)[9], const double (&b)[9], double (&c)[9]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) c[3 * r + k] = dot3(a[3 * r], a[3 * r + 1], a[3 * r + 2], b[k], b[3 + k], b[6 + k]);
}

// ---- sums in a fixed order ----
// Sum over the wave by an xor butterfly from offset 32 down to 1: every lane ends with the same value (each level adds the same
// two operands).
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

// Sum over a workgroup of THREADS (double or int): wave_sum, then the wave partials in wave order.  `red` holds THREADS / 64 values;
// every thread returns the sum.  Two barriers, the first ahead of the write: safe to call again at once.
template <int THREADS, class T>
__device__ __forceinline__ T block_sum(T v, T* red) {
#pragma clang fp contract(off)
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = red[0];
#pragma unroll
  for (int w = 1; w < THREADS / 64; ++w) t = t + red[w];
  return t;
}

// block_sum for N values at once, in its order; one pair of barriers for all of them.  `red` holds (THREADS / 64) * N doubles.
template <int THREADS, int N>
__device__ __forceinline__ void block_sums(double (&v)[N], double* red) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] = wave_sum(v[e]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int e = 0; e < N; ++e) red[(threadIdx.x >> 6) * N + e] = v[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < N; ++e) {
    double t = red[e];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) t = t + red[w * N + e];
    v[e] = t;
  }
}

// ---- exclusive scans over a workgroup of THREADS (all threads call them); wsum holds THREADS / 64 ints ----
// Lane `writer` of each wave holds the wave's total.  Two barriers, the first ahead of the write of wsum, none behind its reads: a
// second call in one kernel waits at its first barrier until every thread has read the totals of the call before.
template <int THREADS>
__device__ __forceinline__ int scan_wave_totals(int wave_total, int writer, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == writer) wsum[wave] = wave_total;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    const int s = wsum[w];
    off += w < wave ? s : 0;
    tot += s;
  }
  total = tot;
  return off;
}

// Position of this thread's flag among the set flags of the workgroup, and their number: wave ballots and popcounts.
template <int THREADS>
__device__ __forceinline__ int block_scan_flag(bool keep, int* wsum, int& total) {
  const unsigned long long bal = __ballot(keep);
  const int before = __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull));
  return scan_wave_totals<THREADS>(__popcll(bal), 0, wsum, total) + before;
}

// Exclusive prefix of v over the workgroup's threads, and the workgroup total.
template <int THREADS>
__device__ __forceinline__ int block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  return scan_wave_totals<THREADS>(incl, 63, wsum, total) + incl - v;
}

// The second half of a stable compaction across workgroups: the sum of the block counts before block b (every thread returns
// it), to which the workgroup adds its own scan.  `red` holds THREADS / 64 ints.
template <int THREADS>
__device__ __forceinline__ int block_base(const int32_t* __restrict__ block_sums, int b, int* red) {
  int v = 0;
  for (int k = threadIdx.x; k < b; k += THREADS) v += block_sums[k];
  return block_sum<THREADS>(v, red);
}

// ---- the key of a RANSAC hypothesis: a maximum of keys is the best score, then the lowest hypothesis; 0 = none ----
__device__ __forceinline__ uint64_t key_of(int score, int h) {
  return ((uint64_t)(score + 1) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)h);
}
__device__ __forceinline__ int hypothesis_of(uint64_t key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }
__device__ __forceinline__ int score_of(uint64_t key) { return (int)(key >> 32) - 1; }

// Maximum over a workgroup (a maximum: no order to depend on) in two halves, so that a kernel whose thread 0 alone stores the key
// reads the wave maxima in that thread only.  publish_wave_keys: the maximum of each wave into best [THREADS / 64], then one barrier
// (a kernel that publishes twice needs a barrier of its own in between); max_wave_key: the maximum of what was published.
__device__ __forceinline__ void publish_wave_keys(uint64_t key, uint64_t* best) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t t = __shfl_xor((unsigned long long)key, o);
    key = t > key ? t : key;
  }
  if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = key;
  __syncthreads();
}
template <int THREADS>
__device__ __forceinline__ uint64_t max_wave_key(const uint64_t* best) {
  uint64_t key = best[0];
#pragma unroll
  for (int w = 1; w < THREADS / 64; ++w) key = best[w] > key ? best[w] : key;
  return key;
}

// The winner over the keys the workgroups of problem p left in keys [problems][groups].
__device__ __forceinline__ uint64_t max_group_key(const uint64_t* __restrict__ keys, int p, int groups) {
  uint64_t key = 0;
  for (int g = 0; g < groups; ++g) {
    const uint64_t k = keys[(size_t)p * groups + g];
    key = k > key ? k : key;
  }
  return key;
}

// ---- the counter-based sampler ----
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// Draw c of hypothesis h: an index in [0, n) from the counter-based stream of the problem's seed.
__device__ __forceinline__ int draw_index(uint64_t seed, int h, int c, int n) {
  const uint64_t r = mix64(seed ^ mix64(((uint64_t)h << 8) | (uint64_t)c));
  return (int)(((r >> 32) * (uint64_t)n) >> 32);
}

// K indices of hypothesis h: n == K gives 0 .. K-1; otherwise position k takes draws until one is valid(index) and differs from
// the positions before it, or GEOM_SAMPLE_DRAWS draws of the hypothesis are spent (the last draw then stays: the caller checks that
// the sample is distinct and usable).
template <int K, class Valid>
__device__ __forceinline__ void sample_distinct(uint64_t seed, int h, int n, int (&id)[K], Valid valid) {
  if (n == K) {
#pragma unroll
    for (int k = 0; k < K; ++k) id[k] = k;
    return;
  }
  int c = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int v;
    bool bad;
    do {
      v = draw_index(seed, h, c++, n);
      bad = !valid(v);
#pragma unroll
      for (int j = 0; j < k; ++j) bad = bad || v == id[j];
    } while (bad && c < GEOM_SAMPLE_DRAWS);
    id[k] = v;
  }
}

// ---- Gaussian elimination with complete pivoting ----
// Step K on the ROWS x COLS matrix a whose first PCOLS columns may be pivots (perm: their permutation): the pivot is the largest
// |entry| of rows K.., columns K..PCOLS-1 (row-major scan with a strict comparison: the lowest row, then the lowest column); rows
// and columns are swapped by compare-selects, then the rows below are eliminated.  ok turns false when the pivot is <= eps in
// magnitude (or NaN).  A template, not a loop: the steps together are beyond the size the compiler unrolls a loop to, and a loop
// that stays rolled puts the matrix into scratch memory; here every index is a constant and the matrix lives in registers.
template <int K, int ROWS, int COLS, int PCOLS>
__device__ __forceinline__ void pivot_step(double (&a)[ROWS][COLS], int (&perm)[PCOLS], bool& ok, double eps) {
#pragma clang fp contract(off)
  double best = -1.0;
  int pr = K, pc = K;
#pragma unroll
  for (int r = K; r < ROWS; ++r) {
#pragma unroll
    for (int c = K; c < PCOLS; ++c) {
      const double v = fabs(a[r][c]);
      const bool g = v > best;
      best = g ? v : best;
      pr = g ? r : pr;
      pc = g ? c : pc;
    }
  }
#pragma unroll
  for (int r = K + 1; r < ROWS; ++r) {
    const bool sw = pr == r;
#pragma unroll
    for (int c = K; c < COLS; ++c) {
      const double t = a[K][c];
      a[K][c] = sw ? a[r][c] : t;
      a[r][c] = sw ? t : a[r][c];
    }
  }
#pragma unroll
  for (int c = K + 1; c < PCOLS; ++c) {
    const bool sw = pc == c;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const double t = a[r][K];
      a[r][K] = sw ? a[r][c] : t;
      a[r][c] = sw ? t : a[r][c];
    }
    const int tp = perm[K];
    perm[K] = sw ? perm[c] : tp;
    perm[c] = sw ? tp : perm[c];
  }
  ok = ok && fabs(a[K][K]) > eps;
  const double inv = 1.0 / a[K][K];
#pragma unroll
  for (int r = K + 1; r < ROWS; ++r) {
    const double m = a[r][K] * inv;
#pragma unroll
    for (int c = K + 1; c < COLS; ++c) a[r][c] = a[r][c] - m * a[K][c];
  }
}

// ---- symmetric 3x3 ----
// One rotation of the cyclic Jacobi on the pair (P, Q) of the symmetric G; V collects the rotations (its columns: the
// eigenvectors).  A template: P, Q and the third index are constants.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&G)[3][3], double (&V)[3][3]) {
#pragma clang fp contract(off)
  constexpr int R = 3 - P - Q;
  const double gpq = G[P][Q];
  if (gpq == 0.0) return;
  const double theta = (G[Q][Q] - G[P][P]) / (2.0 * gpq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  const double gpp = G[P][P] - t * gpq, gqq = G[Q][Q] + t * gpq;
  const double grp = c * G[R][P] - s * G[R][Q], grq = s * G[R][P] + c * G[R][Q];
  G[P][P] = gpp;
  G[Q][Q] = gqq;
  G[P][Q] = G[Q][P] = 0.0;
  G[R][P] = G[P][R] = grp;
  G[R][Q] = G[Q][R] = grq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vp = c * V[k][P] - s * V[k][Q], vq = s * V[k][P] + c * V[k][Q];
    V[k][P] = vp;
    V[k][Q] = vq;
  }
}

// Cofactors and determinant of the symmetric A, and the product of its diagonal.
struct Cof3 {
  double c00, c01, c02, c11, c12, c22, det, diag;
};
__device__ __forceinline__ Cof3 cofactors3(double a00, double a01, double a02, double a11, double a12, double a22) {
#pragma clang fp contract(off)
  Cof3 c;
  c.c00 = a11 * a22 - a12 * a12;
  c.c01 = a02 * a12 - a01 * a22;
  c.c02 = a01 * a12 - a02 * a11;
  c.c11 = a00 * a22 - a02 * a02;
  c.c12 = a01 * a02 - a00 * a12;
  c.c22 = a00 * a11 - a01 * a01;
  c.det = dot3(a00, a01, a02, c.c00, c.c01, c.c02);
  c.diag = (a00 * a11) * a22;
  return c;
}
// x = A^-1 b by the cofactors.  false: the determinant is not finite or not above eps times the product of the diagonal, or the
// solution is not finite.
__device__ __forceinline__ bool cof3_solve(const Cof3& c, double eps, double b0, double b1, double b2, double& x0, double& x1,
                                           double& x2) {
#pragma clang fp contract(off)
  x0 = dot3(c.c00, c.c01, c.c02, b0, b1, b2) / c.det;
  x1 = dot3(c.c01, c.c11, c.c12, b0, b1, b2) / c.det;
  x2 = dot3(c.c02, c.c12, c.c22, b0, b1, b2) / c.det;
  return isfinite(c.det) && c.det > eps * c.diag && isfinite(x0) && isfinite(x1) && isfinite(x2);
}

// ---- the camera model ----
// The view of the point X under (R, C) and (fx, fy, cx, cy): y = R (X - C), u = y0 / y2, v = y1 / y2, the residual against the pixel.
struct View {
  double y0, y1, y2, u, v, r0, r1;
};
__device__ __forceinline__ View project(const double* R, const double* C, double fx, double fy, double cx, double cy, double X0,
                                        double X1, double X2, double px, double py) {
#pragma clang fp contract(off)
  const double q0 = X0 - C[0], q1 = X1 - C[1], q2 = X2 - C[2];
  View o;
  o.y0 = dot3(R[0], R[1], R[2], q0, q1, q2);
  o.y1 = dot3(R[3], R[4], R[5], q0, q1, q2);
  o.y2 = dot3(R[6], R[7], R[8], q0, q1, q2);
  o.u = o.y0 / o.y2;
  o.v = o.y1 / o.y2;
  o.r0 = (fx * o.u + cx) - px;
  o.r1 = (fy * o.v + cy) - py;
  return o;
}
// The same under a camera record: R [9], C [3], fx, fy, cx, cy.
__device__ __forceinline__ View project(const double* cam, double X0, double X1, double X2, double px, double py) {
  return project(cam, cam + 9, cam[12], cam[13], cam[14], cam[15], X0, X1, X2, px, py);
}

// R <- orthonormalised(Cay(w) R), t <- Cay(w) t + dt, delta = (w, dt); Cay(w) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a),
// a = w / 2.  The renormalisation: row 0 scaled to unit length, row 1 made orthogonal to it and scaled, row 2 their cross
// product.  false (nothing changed): the result is not finite.
__device__ __forceinline__ bool cayley_update(double (&R)[9], double (&t)[3], const double (&delta)[6]) {
#pragma clang fp contract(off)
  const double a0 = 0.5 * delta[0], a1 = 0.5 * delta[1], a2 = 0.5 * delta[2];
  const double aa = dot3(a0, a1, a2, a0, a1, a2);
  const double den = 1.0 + aa, om = 1.0 - aa;
  const double Q[9] = {(om + 2.0 * (a0 * a0)) / den,        (2.0 * (a0 * a1) - 2.0 * a2) / den, (2.0 * (a0 * a2) + 2.0 * a1) / den,
                       (2.0 * (a0 * a1) + 2.0 * a2) / den, (om + 2.0 * (a1 * a1)) / den,        (2.0 * (a1 * a2) - 2.0 * a0) / den,
                       (2.0 * (a0 * a2) - 2.0 * a1) / den, (2.0 * (a1 * a2) + 2.0 * a0) / den, (om + 2.0 * (a2 * a2)) / den};
  double M[9], tn[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) M[3 * i + j] = dot3(Q[3 * i], Q[3 * i + 1], Q[3 * i + 2], R[j], R[3 + j], R[6 + j]);
    tn[i] = dot3(Q[3 * i], Q[3 * i + 1], Q[3 * i + 2], t[0], t[1], t[2]) + delta[3 + i];
  }
  const double nr0 = sqrt(dot3(M[0], M[1], M[2], M[0], M[1], M[2]));
  const double r0[3] = {M[0] / nr0, M[1] / nr0, M[2] / nr0};
  const double pj = dot3(M[3], M[4], M[5], r0[0], r0[1], r0[2]);
  const double w[3] = {M[3] - pj * r0[0], M[4] - pj * r0[1], M[5] - pj * r0[2]};
  const double nr1 = sqrt(dot3(w[0], w[1], w[2], w[0], w[1], w[2]));
  const double r1[3] = {w[0] / nr1, w[1] / nr1, w[2] / nr1};
  double r2[3];
  cross3(r0, r1, r2);
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) fin = fin && isfinite(r0[k]) && isfinite(r1[k]) && isfinite(r2[k]) && isfinite(tn[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    R[k] = fin ? r0[k] : R[k];
    R[3 + k] = fin ? r1[k] : R[3 + k];
    R[6 + k] = fin ? r2[k] : R[6 + k];
    t[k] = fin ? tn[k] : t[k];
  }
  return fin;
}

}  // namespace sspk
