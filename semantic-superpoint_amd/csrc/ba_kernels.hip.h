// Windowed bundle adjustment: the cameras of the retained frames inside the newest consistent window and the
// accepted rows of the N-view triangulation (section 26) refined together by Levenberg-Marquardt on the pixel reprojection error,
// the points eliminated by the Schur complement.  The rules are restated in numpy by tests/ba_ref.py; everything here is fp64 with
// contraction off, in the parenthesisation of that file, and every sum over the rows runs in one fixed order (block_sum's
// inside a tile of 256 rows, the tiles ascending), so a result does not depend on row_cap, on the order the workgroups run in or
// on the run.  No floating-point atomics, no grid-wide barrier: every phase is a launch of its own, and what a phase decides
// (accept / reject, done) the next one reads from device memory.
//   ba_init_kernel       x_out <- x, cams_out <- cams (invalid views zeroed), the gauge (a, b, k*) and the first control record
//   ba_linearise_kernel  a track row per thread, 256 rows per workgroup, the ids tile and the camera records staged as in
//                        triangulate_tracks_kernel.  Per row: the damped V_r, its cofactors, g_r; then per view c the 6x6 U_c, g_c
//                        and W V^-1 g_r, and per pair (c, c') of views W_c V^-1 W_c'^T, each summed over the tile.  W is never
//                        stored: a view is recomputed from 16 B of pixel and an LDS camera record whenever it is needed.  A pair no
//                        row of the workgroup sees is a zero store; a wavefront none of whose lanes sees it (ballot) skips the
//                        arithmetic and the butterfly.
//   ba_solve_kernel      one workgroup: the tile partials summed in tile order into the 6L x (6L + 1) system in LDS, damping, the
//                        gauge, Cholesky without pivoting (right-looking: every element's updates come in the order of k), the
//                        step and the candidate cameras (cayley_update: section 27's update and renormalisation)
//   ba_backsub_kernel    per row dX = V^-1 (-g_r - sum W^T d_c), the candidate point, its cost and cheirality under the candidate
//                        cameras, summed per tile
//   ba_accept_kernel     every workgroup reads the same sums and takes the same decision; an accepted step copies the candidates;
//                        workgroup 0 writes the next control record (the records are per iteration: none is read and written in
//                        one launch)
//   ba_finish_kernel     rms_out and info
//   ba_apply_kernel      a thread per sequence: the adjusted cameras written back into the trajectory table and the chain state
// Needs: geom_blocks.hip.h, pose_kernels.hip.h (POSE_ROW_WORDS, POSE_STATE_WORDS), landmark_kernels.hip.h (the staged tile, LM_*),
// pnp_kernels.hip.h (PNP_SCALE_FRACTION, PNP_THREADS).
#pragma once

namespace sspk {

#define BA_THREADS 256
#define BA_WAVES (BA_THREADS / 64)
#define BA_INFO_WORDS 8
#define BA_MAX_ITERATIONS 16
#define BA_FLAG_ADJUSTED 8
#define BA_LAMBDA0 1e-4
#define BA_LAMBDA_MIN 1e-12
#define BA_LAMBDA_MAX 1e6
#define BA_DONE_RELATIVE 1e-10
#define BA_DONE_RESIDUAL 1e-9
#define BA_STATUS_NOTHING 1
#define BA_STATUS_NO_STEP 2
// control record: lambda, cost before, cost now, n_obs, rows used, accepted steps, refused V solves, done, status, a, b, k*
#define BA_CTL_WORDS 12
// after the step in the solve record: solved, the cost the linearisation saw, n_obs, rows used, refused V solves, nothing to adjust
#define BA_SOL_EXTRA 8
static_assert(BA_THREADS == LM_THREADS && BA_THREADS == PNP_THREADS, "one workgroup size for the fp64 geometry kernels");

__host__ __device__ inline int ba_pairs(int L) { return L * (L + 1) / 2; }
// doubles of one tile's partial sums: 36 per pair of views, then per view U (21), g_c (6), W V^-1 g_r (6), then 4 scalars
__host__ __device__ inline int ba_part_words(int L) { return 36 * ba_pairs(L) + 33 * L + 4; }
__host__ __device__ inline size_t ba_stage_bytes(int L) {
  return (size_t)2 * L * LM_CAM_WORDS * sizeof(double) + (size_t)BA_WAVES * 36 * sizeof(double) +
         (size_t)LM_THREADS * lm_ids_pitch(L) * sizeof(int32_t) + (size_t)2 * L * sizeof(int32_t);
}
__host__ __device__ inline size_t ba_solve_lds_bytes(int L) { return (size_t)(6 * L) * (6 * L + 1) * sizeof(double); }

// the workspace, in doubles: control records, the solve record, candidate cameras, candidate points, tile partials, candidate sums
struct BaWs {
  double *ctl, *sol, *cand_cams, *x_cand, *part, *cpart;
};
__host__ __device__ inline size_t ba_ws_words(int L, int row_cap) {
  const size_t tiles = (size_t)(row_cap + BA_THREADS - 1) / BA_THREADS;
  return (size_t)(BA_MAX_ITERATIONS + 1) * BA_CTL_WORDS + (size_t)(6 * L + BA_SOL_EXTRA) + (size_t)L * LM_CAM_WORDS +
         (size_t)row_cap * 3 + tiles * ba_part_words(L) + tiles * 2;
}
__host__ __device__ inline BaWs ba_ws_of(double* base, int L, int row_cap) {
  const size_t tiles = (size_t)(row_cap + BA_THREADS - 1) / BA_THREADS;
  BaWs w;
  w.ctl = base;
  w.sol = w.ctl + (size_t)(BA_MAX_ITERATIONS + 1) * BA_CTL_WORDS;
  w.cand_cams = w.sol + (6 * L + BA_SOL_EXTRA);
  w.x_cand = w.cand_cams + (size_t)L * LM_CAM_WORDS;
  w.part = w.x_cand + (size_t)row_cap * 3;
  w.cpart = w.part + tiles * ba_part_words(L);
  return w;
}

// What a workgroup stages (triangulate_tracks_kernel's tile): two sets of camera records, the reduction scratch, the ids tile at
// an odd pitch, per view the id of its point 0 and its clamped point count.
struct BaStage {
  double *cam, *cam2, *red;
  int32_t *ids, *first, *cnt;
  int pitch;
};
__device__ __forceinline__ BaStage ba_stage(double* dyn, const int32_t* __restrict__ ids, const int32_t* __restrict__ state,
                                            const double* __restrict__ cams, const double* __restrict__ cams2, int L, int point_cap,
                                            int row_cap) {
  BaStage s;
  const int tid = threadIdx.x;
  s.pitch = lm_ids_pitch(L);
  s.cam = dyn;
  s.cam2 = s.cam + (size_t)L * LM_CAM_WORDS;
  s.red = s.cam2 + (size_t)L * LM_CAM_WORDS;
  s.ids = reinterpret_cast<int32_t*>(s.red + BA_WAVES * 36);
  s.first = s.ids + (size_t)LM_THREADS * s.pitch;
  s.cnt = s.first + L;
  const int row0 = blockIdx.x * BA_THREADS;
  const int tile = min(BA_THREADS, row_cap - row0) * L;
  const int32_t* src = ids + (size_t)row0 * L;
  for (int e = tid; e < tile; e += BA_THREADS) {
    const int r = e / L;
    s.ids[r * s.pitch + (e - r * L)] = src[e];
  }
  for (int e = tid; e < L * LM_CAM_WORDS; e += BA_THREADS) {
    s.cam[e] = cams[e];
    s.cam2[e] = cams2[e];
  }
  if (tid < L) {
    int first = 0;
    for (int k = 0; k < tid; ++k) first += min(max(state[2 + k], 0), point_cap);
    s.first[tid] = first;
    s.cnt[tid] = min(max(state[2 + tid], 0), point_cap);
  }
  __syncthreads();
  return s;
}

// the views a live row is observed in, by section 26's id, count and clamp rules
__device__ __forceinline__ unsigned ba_used(const BaStage& s, int L, bool live) {
  unsigned used = 0;
  if (live) {
    const int32_t* my = s.ids + threadIdx.x * s.pitch;
    for (int c = 0; c < L; ++c) {
      const int id = my[c], p = id - s.first[c];
      if (id >= 0 && s.cam[c * LM_CAM_WORDS + 16] != 0.0 && p >= 0 && p < s.cnt[c]) used |= 1u << c;
    }
  }
  return used;
}

__device__ __forceinline__ double2 ba_pixel(const BaStage& s, const double* __restrict__ pts, int first_slot, int c, int L, int point_cap) {
  const int p = s.ids[threadIdx.x * s.pitch + c] - s.first[c];
  return *reinterpret_cast<const double2*>(pts + ((size_t)((first_slot + c) % L) * point_cap + p) * 2);
}

// One view: project's y = Rw (X - C) and residual, the point Jacobians p0, p1 and the camera Jacobians j0, j1 over (w, dC).
struct BaView {
  double y2, r0, r1, p0[3], p1[3], j0[6], j1[6];
};
__device__ __forceinline__ void ba_view(const double* cam, double X0, double X1, double X2, double2 px, BaView& o) {
#pragma clang fp contract(off)
  const View w = project(cam, X0, X1, X2, px.x, px.y);
  const double y0 = w.y0, y1 = w.y1, y2 = w.y2, un = w.u, vn = w.v, fa = cam[12] / y2, fb = cam[13] / y2;
  o.y2 = y2;
  o.r0 = w.r0;
  o.r1 = w.r1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.p0[k] = fa * (cam[k] - un * cam[6 + k]);
    o.p1[k] = fb * (cam[3 + k] - vn * cam[6 + k]);
    o.j0[3 + k] = 0.0 - o.p0[k];
    o.j1[3 + k] = 0.0 - o.p1[k];
  }
  o.j0[0] = fa * (0.0 - un * y1);
  o.j0[1] = fa * (y2 + un * y0);
  o.j0[2] = fa * (0.0 - y1);
  o.j1[0] = fb * ((0.0 - y2) - vn * y1);
  o.j1[1] = fb * (vn * y0);
  o.j1[2] = fb * y0;
}

// the residual alone: squared error and whether the point is in front
__device__ __forceinline__ double ba_error(const double* cam, double X0, double X1, double X2, double2 px, bool& front) {
#pragma clang fp contract(off)
  const View w = project(cam, X0, X1, X2, px.x, px.y);
  front = isfinite(w.y2) && w.y2 > 0.0;
  return w.r0 * w.r0 + w.r1 * w.r1;
}

// The point block of a row under the cameras in s.cam: cofactors and determinant of the damped V_r, g_r, z = V_r^-1 g_r, the sum
// of the squared residuals; ok by cof3_solve's refusal rule.
struct BaPoint {
  Cof3 c;
  double g0, g1, g2, z0, z1, z2, ss;
  bool ok;
};
__device__ __forceinline__ void ba_point(const BaStage& s, const double* __restrict__ pts, int first_slot, int L, int point_cap,
                                         unsigned used, double X0, double X1, double X2, double lambda, BaPoint& o) {
#pragma clang fp contract(off)
  double h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, ss = 0.0;
#pragma unroll 1
  for (int c = 0; c < L; ++c) {
    if (!((used >> c) & 1u)) continue;
    BaView v;
    ba_view(s.cam + c * LM_CAM_WORDS, X0, X1, X2, ba_pixel(s, pts, first_slot, c, L, point_cap), v);
    h00 = h00 + (v.p0[0] * v.p0[0] + v.p1[0] * v.p1[0]);
    h01 = h01 + (v.p0[0] * v.p0[1] + v.p1[0] * v.p1[1]);
    h02 = h02 + (v.p0[0] * v.p0[2] + v.p1[0] * v.p1[2]);
    h11 = h11 + (v.p0[1] * v.p0[1] + v.p1[1] * v.p1[1]);
    h12 = h12 + (v.p0[1] * v.p0[2] + v.p1[1] * v.p1[2]);
    h22 = h22 + (v.p0[2] * v.p0[2] + v.p1[2] * v.p1[2]);
    g0 = g0 + (v.p0[0] * v.r0 + v.p1[0] * v.r1);
    g1 = g1 + (v.p0[1] * v.r0 + v.p1[1] * v.r1);
    g2 = g2 + (v.p0[2] * v.r0 + v.p1[2] * v.r1);
    ss = ss + (v.r0 * v.r0 + v.r1 * v.r1);
  }
  const double damp = 1.0 + lambda;
  o.c = cofactors3(h00 * damp, h01, h02, h11 * damp, h12, h22 * damp);
  o.g0 = g0;
  o.g1 = g1;
  o.g2 = g2;
  o.ok = cof3_solve(o.c, LM_DET_EPS, g0, g1, g2, o.z0, o.z1, o.z2);
  o.ss = ss;
}

// N values summed over the workgroup in block_sum's order (wave_sum inside each wave, the wave partials in wave
// order) and stored by the first N threads.  `wave_has`: some lane of this wave contributes (else the wave's partial is the zero
// its butterfly would give).  The caller has a barrier between two uses of `red`.
template <int N>
__device__ __forceinline__ void ba_block_store(double (&v)[N], bool wave_has, double* red, double* __restrict__ out) {
#pragma clang fp contract(off)
  if (wave_has) {
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = wave_sum(v[e]);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int e = 0; e < N; ++e) red[(threadIdx.x >> 6) * N + e] = wave_has ? v[e] : 0.0;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double t = red[threadIdx.x];
#pragma unroll
    for (int w = 1; w < BA_WAVES; ++w) t = t + red[w * N + threadIdx.x];
    out[threadIdx.x] = t;
  }
}

// grid (cdiv(row_cap, 256)): x_out <- x for every row, cams_out <- cams with the invalid views zeroed, the first control record.
__global__ __launch_bounds__(BA_THREADS) void ba_init_kernel(const double* __restrict__ cams, const double* __restrict__ x_in, int L,
                                                            int row_cap, double* __restrict__ cams_out, double* __restrict__ x_out,
                                                            double* __restrict__ ctl) {
  const int tid = threadIdx.x, row = blockIdx.x * BA_THREADS + tid;
  if (row < row_cap) {
#pragma unroll
    for (int k = 0; k < 3; ++k) x_out[(size_t)row * 3 + k] = x_in[(size_t)row * 3 + k];
  }
  if (blockIdx.x != 0) return;
  for (int e = tid; e < L * LM_CAM_WORDS; e += BA_THREADS) cams_out[e] = cams[(e / LM_CAM_WORDS) * LM_CAM_WORDS + 16] != 0.0 ? cams[e] : 0.0;
  if (tid == 0) {
    int a = -1, b = -1;
    for (int c = 0; c < L; ++c) {
      if (cams[c * LM_CAM_WORDS + 16] == 0.0) continue;
      if (a < 0) a = c;
      b = c;
    }
    int ks = 0;
    if (a >= 0) {
      double best = fabs(cams[b * LM_CAM_WORDS + 9] - cams[a * LM_CAM_WORDS + 9]);
      for (int k = 1; k < 3; ++k) {
        const double d = fabs(cams[b * LM_CAM_WORDS + 9 + k] - cams[a * LM_CAM_WORDS + 9 + k]);
        if (d > best) {
          best = d;
          ks = k;
        }
      }
    }
    for (int e = 0; e < BA_CTL_WORDS; ++e) ctl[e] = 0.0;
    ctl[0] = BA_LAMBDA0;
    ctl[8] = (double)BA_STATUS_NO_STEP;
    ctl[9] = (double)a;
    ctl[10] = (double)b;
    ctl[11] = (double)ks;
  }
}

// grid (cdiv(row_cap, 256)), dynamic LDS ba_stage_bytes(L).  ctl: this iteration's control record.  part: per tile ba_part_words(L).
__global__ __launch_bounds__(BA_THREADS) void ba_linearise_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ state,
                                                                 const double* __restrict__ pts, int first_slot,
                                                                 const double* __restrict__ cams, const double* __restrict__ x,
                                                                 const int32_t* __restrict__ status, int L, int point_cap, int row_cap,
                                                                 const double* __restrict__ ctl, double* __restrict__ part) {
#pragma clang fp contract(off)
  extern __shared__ double ba_dyn[];
  if (ctl[7] != 0.0) return;                                 // done (uniform over the grid)
  const BaStage s = ba_stage(ba_dyn, ids, state, cams, cams, L, point_cap, row_cap);
  const int tid = threadIdx.x, row = blockIdx.x * BA_THREADS + tid;
  const int n_rows = min(max(state[0], 0), row_cap);
  const bool live = row < n_rows && status[row] == 0;
  const unsigned used = ba_used(s, L, live);
  const double lambda = ctl[0];
  double X0 = 0.0, X1 = 0.0, X2 = 0.0;
  if (live) {
    X0 = x[(size_t)row * 3];
    X1 = x[(size_t)row * 3 + 1];
    X2 = x[(size_t)row * 3 + 2];
  }
  BaPoint pt;
  ba_point(s, pts, first_slot, L, point_cap, used, X0, X1, X2, lambda, pt);
  double* out = part + (size_t)blockIdx.x * ba_part_words(L);
  double* out_cam = out + 36 * ba_pairs(L);
  {
    double sc[4] = {live ? pt.ss : 0.0, (double)__popc(used), live ? 1.0 : 0.0, (live && !pt.ok) ? 1.0 : 0.0};
    ba_block_store(sc, true, s.red, out_cam + 33 * L);
  }
#pragma unroll 1
  for (int c = 0; c < L; ++c) {
    const bool act = ((used >> c) & 1u) && pt.ok;
    double* out_pairs = out + (size_t)36 * (c * (c + 1) / 2);
    if (!__syncthreads_or(act)) {                            // no row of the tile: the sums are zeros
      if (tid < 33) out_cam[33 * c + tid] = 0.0;
      for (int e = tid; e < 36 * (c + 1); e += BA_THREADS) out_pairs[e] = 0.0;
      continue;
    }
    const bool wave_act = __ballot(act) != 0ull;
    double Y[6][3];
    {
      double m[33];
#pragma unroll
      for (int e = 0; e < 33; ++e) m[e] = 0.0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) Y[a][k] = 0.0;
      if (act) {
        BaView v;
        ba_view(s.cam + c * LM_CAM_WORDS, X0, X1, X2, ba_pixel(s, pts, first_slot, c, L, point_cap), v);
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b, ++e) m[e] = v.j0[a] * v.j0[b] + v.j1[a] * v.j1[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          m[21 + a] = v.j0[a] * v.r0 + v.j1[a] * v.r1;
          const double w0 = v.j0[a] * v.p0[0] + v.j1[a] * v.p1[0], w1 = v.j0[a] * v.p0[1] + v.j1[a] * v.p1[1];
          const double w2 = v.j0[a] * v.p0[2] + v.j1[a] * v.p1[2];
          m[27 + a] = dot3(w0, w1, w2, pt.z0, pt.z1, pt.z2);
          Y[a][0] = dot3(w0, w1, w2, pt.c.c00, pt.c.c01, pt.c.c02) / pt.c.det;
          Y[a][1] = dot3(w0, w1, w2, pt.c.c01, pt.c.c11, pt.c.c12) / pt.c.det;
          Y[a][2] = dot3(w0, w1, w2, pt.c.c02, pt.c.c12, pt.c.c22) / pt.c.det;
        }
      }
      ba_block_store(m, wave_act, s.red, out_cam + 33 * c);
    }
#pragma unroll 1
    for (int c2 = 0; c2 <= c; ++c2) {
      const bool both = act && ((used >> c2) & 1u);
      if (!__syncthreads_or(both)) {                         // (the barrier also frees `red`)
        if (tid < 36) out_pairs[36 * c2 + tid] = 0.0;
        continue;
      }
      const bool wave_both = __ballot(both) != 0ull;
      double E[36];
#pragma unroll
      for (int e = 0; e < 36; ++e) E[e] = 0.0;
      if (both) {
        BaView v;
        ba_view(s.cam + c2 * LM_CAM_WORDS, X0, X1, X2, ba_pixel(s, pts, first_slot, c2, L, point_cap), v);
#pragma unroll
        for (int b = 0; b < 6; ++b) {
          const double w0 = v.j0[b] * v.p0[0] + v.j1[b] * v.p1[0], w1 = v.j0[b] * v.p0[1] + v.j1[b] * v.p1[1];
          const double w2 = v.j0[b] * v.p0[2] + v.j1[b] * v.p1[2];
#pragma unroll
          for (int a = 0; a < 6; ++a) E[6 * a + b] = dot3(Y[a][0], Y[a][1], Y[a][2], w0, w1, w2);
        }
      }
      ba_block_store(E, wave_both, s.red, out_pairs + 36 * c2);
    }
  }
}

// sum over the tiles of one word of their partials, in tile order; the loads go out eight at a time (one workgroup does this
// alone: it is bound by their latency), the additions stay in order
__device__ __forceinline__ double ba_tile_sum(const double* __restrict__ src, size_t stride, int n_tiles) {
#pragma clang fp contract(off)
  double acc = 0.0;
  int t = 0;
  for (; t + 8 <= n_tiles; t += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = src[(size_t)(t + i) * stride];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = acc + v[i];
  }
  for (; t < n_tiles; ++t) acc = acc + src[(size_t)t * stride];
  return acc;
}

// whether parameter i of the camera system is held: every parameter of an invalid view and of the first valid view a, coordinate k*
// of the centre of the last valid view b
__device__ __forceinline__ bool ba_held(int i, unsigned vmask, int a, int b, int ks) {
  const int c = i / 6, k = i - 6 * c;
  return !((vmask >> c) & 1u) || c == a || (c == b && k == 3 + ks);
}

// one workgroup, dynamic LDS ba_solve_lds_bytes(L).  cams: the current cameras.  sol: the step [6L], then BA_SOL_EXTRA words.
__global__ __launch_bounds__(BA_THREADS) void ba_solve_kernel(const double* __restrict__ part, int n_tiles, const double* __restrict__ cams,
                                                             int L, const double* __restrict__ ctl, double* __restrict__ sol,
                                                             double* __restrict__ cand_cams) {
#pragma clang fp contract(off)
  extern __shared__ double ba_sys[];                         // [N][N + 1]: the lower triangle of S, the right-hand side beside it
  if (ctl[7] != 0.0) return;
  const int tid = threadIdx.x, N = 6 * L, ld = N + 1, P = ba_part_words(L), n_pair_words = 36 * ba_pairs(L);
  const double lambda = ctl[0], damp = 1.0 + lambda;
  const int ga = (int)ctl[9], gb = (int)ctl[10], ks = (int)ctl[11];
  unsigned vmask = 0;
  for (int c = 0; c < L; ++c) vmask |= cams[c * LM_CAM_WORDS + 16] != 0.0 ? 1u << c : 0u;
  // the Schur sums: tile partials in tile order.  An off-diagonal block is stored negated, a diagonal one waits for U.
  for (int e = tid; e < n_pair_words; e += BA_THREADS) {
    const double acc = ba_tile_sum(part + e, P, n_tiles);
    const int p = e / 36, ab = e - 36 * p, a = ab / 6, b = ab - 6 * a;
    int c = 0;
    while ((c + 1) * (c + 2) / 2 <= p) ++c;
    const int c2 = p - c * (c + 1) / 2;
    if (c2 < c || b <= a) ba_sys[(6 * c + a) * ld + 6 * c2 + b] = c2 < c ? 0.0 - acc : acc;
  }
  __syncthreads();
  for (int e = tid; e < 27 * L; e += BA_THREADS) {
    const int c = e / 27, k = e - 27 * c;
    const double* src = part + n_pair_words + 33 * c;
    if (k < 21) {
      const double acc = ba_tile_sum(src + k, P, n_tiles);
      int a = 0, rest = k;
      while (rest >= 6 - a) {
        rest -= 6 - a;
        ++a;
      }
      const int b = a + rest;                                // U[a][b], a <= b, lives at S[6c + b][6c + a]
      double* dst = ba_sys + (6 * c + b) * ld + 6 * c + a;
      *dst = (a == b ? acc * damp : acc) - *dst;
    } else {
      const int a = k - 21;
      const double g = ba_tile_sum(src + 21 + a, P, n_tiles), r = ba_tile_sum(src + 27 + a, P, n_tiles);
      ba_sys[(6 * c + a) * ld + N] = r - g;
    }
  }
  const double* scalars = part + n_pair_words + 33 * L;        // (every thread: 4 * n_tiles loads of the same addresses)
  const double cost = ba_tile_sum(scalars, P, n_tiles), n_obs = ba_tile_sum(scalars + 1, P, n_tiles);
  const double rows = ba_tile_sum(scalars + 2, P, n_tiles), refused = ba_tile_sum(scalars + 3, P, n_tiles);
  const int n_valid = __popc(vmask);
  const bool nothing = n_valid < 2 || rows == 0.0 || 2.0 * n_obs < (double)(6 * (n_valid - 1) - 1) + 3.0 * rows;
  __syncthreads();
  // the gauge
  for (int e = tid; e < N * N; e += BA_THREADS) {
    const int i = e / N, j = e - N * i;
    if (j <= i && (ba_held(i, vmask, ga, gb, ks) || ba_held(j, vmask, ga, gb, ks))) ba_sys[i * ld + j] = i == j ? 1.0 : 0.0;
  }
  if (tid < N && ba_held(tid, vmask, ga, gb, ks)) ba_sys[tid * ld + N] = 0.0;
  __syncthreads();
  // Cholesky, right-looking; the right-hand side is column N
  bool ok = !nothing;
  if (ok) {
#pragma unroll 1
    for (int k = 0; k < N; ++k) {
      const double d = ba_sys[k * ld + k];
      if (!(isfinite(d) && d > 0.0)) {                       // (uniform: every thread reads the same word)
        ok = false;
        break;
      }
      const double r = sqrt(d);
      __syncthreads();
      for (int i = k + 1 + tid; i < N; i += BA_THREADS) ba_sys[i * ld + k] = ba_sys[i * ld + k] / r;
      if (tid == 0) {
        ba_sys[k * ld + k] = r;
        ba_sys[k * ld + N] = ba_sys[k * ld + N] / r;
      }
      __syncthreads();
      const double yk = ba_sys[k * ld + N];
      for (int i = k + 1 + (tid >> 4); i < N; i += BA_THREADS / 16) {   // 16 rows at a time, 16 lanes along each
        const double lik = ba_sys[i * ld + k];
        for (int j = k + 1 + (tid & 15); j <= i; j += 16) ba_sys[i * ld + j] = ba_sys[i * ld + j] - lik * ba_sys[j * ld + k];
        if ((tid & 15) == 0) ba_sys[i * ld + N] = ba_sys[i * ld + N] - lik * yk;
      }
      __syncthreads();
    }
  }
  if (ok) {
#pragma unroll 1
    for (int k = N - 1; k >= 0; --k) {
      __syncthreads();
      const double xk = ba_sys[k * ld + N] / ba_sys[k * ld + k];
      __syncthreads();
      if (tid == 0) ba_sys[k * ld + N] = xk;
      for (int i = tid; i < k; i += BA_THREADS) ba_sys[i * ld + N] = ba_sys[i * ld + N] - ba_sys[k * ld + i] * xk;
    }
    __syncthreads();
    bool fin = true;
    for (int i = tid; i < N; i += BA_THREADS) fin = fin && isfinite(ba_sys[i * ld + N]);
    // the candidate cameras: a view held whole is copied, every other one takes cayley_update
    if (tid < L) {
      const int c = tid;
      const double* cam = cams + c * LM_CAM_WORDS;
      double* o = cand_cams + c * LM_CAM_WORDS;
      for (int e = 0; e < LM_CAM_WORDS; ++e) o[e] = cam[e];
      if (((vmask >> c) & 1u) && c != ga) {
        double R[9], t[3] = {0.0, 0.0, 0.0};
        const double delta[6] = {ba_sys[(6 * c) * ld + N], ba_sys[(6 * c + 1) * ld + N], ba_sys[(6 * c + 2) * ld + N], 0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = cam[e];
        fin = cayley_update(R, t, delta) && fin;
#pragma unroll
        for (int e = 0; e < 9; ++e) o[e] = R[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const double cn = cam[9 + e] + ba_sys[(6 * c + 3 + e) * ld + N];
          fin = fin && isfinite(cn);
          o[9 + e] = cn;
        }
      }
    }
    ok = __syncthreads_and(fin) != 0;
    for (int i = tid; i < N; i += BA_THREADS) sol[i] = ba_sys[i * ld + N];
  }
  if (tid == 0) {
    double* o = sol + N;
    o[0] = ok ? 1.0 : 0.0;
    o[1] = cost;
    o[2] = n_obs;
    o[3] = rows;
    o[4] = refused;
    o[5] = nothing ? 1.0 : 0.0;
    o[6] = o[7] = 0.0;
  }
}

// grid (cdiv(row_cap, 256)), dynamic LDS ba_stage_bytes(L): the candidate points and the candidate cost.  cpart: per tile (cost,
// observations that are not in front).
__global__ __launch_bounds__(BA_THREADS) void ba_backsub_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ state,
                                                               const double* __restrict__ pts, int first_slot,
                                                               const double* __restrict__ cams, const double* __restrict__ x,
                                                               const int32_t* __restrict__ status, int L, int point_cap, int row_cap,
                                                               const double* __restrict__ ctl, const double* __restrict__ sol,
                                                               const double* __restrict__ cand_cams, double* __restrict__ x_cand,
                                                               double* __restrict__ cpart) {
#pragma clang fp contract(off)
  extern __shared__ double ba_dyn[];
  if (ctl[7] != 0.0 || sol[6 * L] == 0.0) return;            // done, or no step to try (uniform over the grid)
  const BaStage s = ba_stage(ba_dyn, ids, state, cams, cand_cams, L, point_cap, row_cap);
  const int tid = threadIdx.x, row = blockIdx.x * BA_THREADS + tid;
  const int n_rows = min(max(state[0], 0), row_cap);
  const bool live = row < n_rows && status[row] == 0;
  const unsigned used = ba_used(s, L, live);
  double X0 = 0.0, X1 = 0.0, X2 = 0.0;
  if (live) {
    X0 = x[(size_t)row * 3];
    X1 = x[(size_t)row * 3 + 1];
    X2 = x[(size_t)row * 3 + 2];
  }
  BaPoint pt;
  ba_point(s, pts, first_slot, L, point_cap, used, X0, X1, X2, ctl[0], pt);
  double ss = 0.0, bad = 0.0;
  if (live) {
    if (pt.ok) {
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll 1
      for (int c = 0; c < L; ++c) {
        if (!((used >> c) & 1u)) continue;
        BaView v;
        ba_view(s.cam + c * LM_CAM_WORDS, X0, X1, X2, ba_pixel(s, pts, first_slot, c, L, point_cap), v);
        const double* d = sol + 6 * c;
        double w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double acc = (v.j0[0] * v.p0[k] + v.j1[0] * v.p1[k]) * d[0] + (v.j0[1] * v.p0[k] + v.j1[1] * v.p1[k]) * d[1];
#pragma unroll
          for (int a = 2; a < 6; ++a) acc = acc + (v.j0[a] * v.p0[k] + v.j1[a] * v.p1[k]) * d[a];
          w[k] = acc;
        }
        t0 = t0 + w[0];
        t1 = t1 + w[1];
        t2 = t2 + w[2];
      }
      const double b0 = (0.0 - pt.g0) - t0, b1 = (0.0 - pt.g1) - t1, b2 = (0.0 - pt.g2) - t2;
      X0 = X0 + dot3(pt.c.c00, pt.c.c01, pt.c.c02, b0, b1, b2) / pt.c.det;
      X1 = X1 + dot3(pt.c.c01, pt.c.c11, pt.c.c12, b0, b1, b2) / pt.c.det;
      X2 = X2 + dot3(pt.c.c02, pt.c.c12, pt.c.c22, b0, b1, b2) / pt.c.det;
    }
    x_cand[(size_t)row * 3] = X0;
    x_cand[(size_t)row * 3 + 1] = X1;
    x_cand[(size_t)row * 3 + 2] = X2;
#pragma unroll 1
    for (int c = 0; c < L; ++c) {
      if (!((used >> c) & 1u)) continue;
      bool front;
      ss = ss + ba_error(s.cam2 + c * LM_CAM_WORDS, X0, X1, X2, ba_pixel(s, pts, first_slot, c, L, point_cap), front);
      bad = bad + (front ? 0.0 : 1.0);
    }
  }
  double both[2] = {ss, bad};
  ba_block_store(both, true, s.red, cpart + (size_t)blockIdx.x * 2);
}

// grid (cdiv(row_cap, 256)).  ctl: this iteration's record, ctl_next: the next one's (written by workgroup 0).
__global__ __launch_bounds__(BA_THREADS) void ba_accept_kernel(const int32_t* __restrict__ state, const int32_t* __restrict__ status, int L,
                                                              int row_cap, int iteration, const double* __restrict__ ctl, double* __restrict__ ctl_next,
                                                              const double* __restrict__ sol, const double* __restrict__ cpart,
                                                              const double* __restrict__ cand_cams, const double* __restrict__ x_cand,
                                                              double* __restrict__ cams_out, double* __restrict__ x_out) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, row = blockIdx.x * BA_THREADS + tid, n_tiles = gridDim.x;
  const bool first = blockIdx.x == 0;
  if (ctl[7] != 0.0) {
    if (first && tid < BA_CTL_WORDS) ctl_next[tid] = ctl[tid];
    return;
  }
  const double* so = sol + 6 * L;
  const bool solved = so[0] != 0.0, nothing = so[5] != 0.0;
  const double cur = so[1], n_obs = so[2];
  double next = 0.0, bad = 0.0;                               // (every thread: the same loads, the same order)
  if (solved) {
    next = ba_tile_sum(cpart, 2, n_tiles);
    bad = ba_tile_sum(cpart + 1, 2, n_tiles);
  }
  const bool accept = solved && isfinite(next) && bad == 0.0 && next < cur;
  if (accept) {
    const int n_rows = min(max(state[0], 0), row_cap);
    if (row < n_rows && status[row] == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) x_out[(size_t)row * 3 + k] = x_cand[(size_t)row * 3 + k];
    }
    if (first)
      for (int e = tid; e < L * LM_CAM_WORDS; e += BA_THREADS) cams_out[e] = cand_cams[e];
  }
  if (first && tid == 0) {
    const bool start = iteration == 0;
    double lambda = ctl[0], done = 0.0, stat = ctl[8], accepted = ctl[5], refused = ctl[6];
    double before = start ? cur : ctl[1], now = start ? cur : ctl[2];
    if (nothing) {
      stat = (double)BA_STATUS_NOTHING;
      done = 1.0;
    } else {
      refused = refused + so[4];
      if (accept) {
        const double by_ten = lambda / 10.0;
        lambda = by_ten > BA_LAMBDA_MIN ? by_ten : BA_LAMBDA_MIN;
        accepted = accepted + 1.0;
        stat = 0.0;
        const double floor_cost = (2.0 * n_obs) * (BA_DONE_RESIDUAL * BA_DONE_RESIDUAL);
        done = (cur - next <= BA_DONE_RELATIVE * cur || next <= floor_cost) ? 1.0 : 0.0;
        now = next;
      } else {
        const double times_ten = lambda * 10.0;
        lambda = times_ten < BA_LAMBDA_MAX ? times_ten : BA_LAMBDA_MAX;
      }
    }
    ctl_next[0] = lambda;
    ctl_next[1] = before;
    ctl_next[2] = now;
    ctl_next[3] = n_obs;
    ctl_next[4] = so[3];
    ctl_next[5] = accepted;
    ctl_next[6] = refused;
    ctl_next[7] = done;
    ctl_next[8] = stat;
    ctl_next[9] = ctl[9];
    ctl_next[10] = ctl[10];
    ctl_next[11] = ctl[11];
  }
}

// grid (cdiv(row_cap, 256)), dynamic LDS ba_stage_bytes(L): rms_out of every row < n_rows under the result, info.
__global__ __launch_bounds__(BA_THREADS) void ba_finish_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ state,
                                                              const double* __restrict__ pts, int first_slot,
                                                              const double* __restrict__ cams_out, const double* __restrict__ x_out,
                                                              const int32_t* __restrict__ status, int L, int point_cap, int row_cap,
                                                              const double* __restrict__ ctl, double* __restrict__ rms_out,
                                                              double* __restrict__ info) {
#pragma clang fp contract(off)
  extern __shared__ double ba_dyn[];
  const BaStage s = ba_stage(ba_dyn, ids, state, cams_out, cams_out, L, point_cap, row_cap);
  const int tid = threadIdx.x, row = blockIdx.x * BA_THREADS + tid;
  const int n_rows = min(max(state[0], 0), row_cap);
  if (blockIdx.x == 0 && tid == 0) {
    info[0] = ctl[8];
    info[1] = ctl[1];
    info[2] = ctl[2];
    info[3] = ctl[3];
    info[4] = ctl[4];
    info[5] = ctl[5];
    info[6] = ctl[6];
    info[7] = ctl[0];
  }
  if (row >= row_cap) return;
  const bool live = row < n_rows && status[row] == 0;
  const unsigned used = ba_used(s, L, live);
  double ss = 0.0;
  if (used) {
    const double X0 = x_out[(size_t)row * 3], X1 = x_out[(size_t)row * 3 + 1], X2 = x_out[(size_t)row * 3 + 2];
#pragma unroll 1
    for (int c = 0; c < L; ++c) {
      if (!((used >> c) & 1u)) continue;
      bool front;
      ss = ss + ba_error(s.cam + c * LM_CAM_WORDS, X0, X1, X2, ba_pixel(s, pts, first_slot, c, L, point_cap), front);
    }
  }
  rms_out[row] = used ? sqrt(ss / (2.0 * (double)__popc(used))) : 0.0;
}

// grid (cdiv(n_seq, 64)), 64 threads: sequence q's trajectory rows and chain state from its adjusted cameras (pose_repair_kernel's
// style).  Acts only when info has status 0.  n_frames_host >= 0 replaces the states' frame counts.
__global__ __launch_bounds__(64) void ba_apply_kernel(const double* __restrict__ info, const double* __restrict__ cams, int L, int n_seq,
                                                     int n_frames_host, double* __restrict__ state, double* __restrict__ table,
                                                     int capacity) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_seq) return;
  if (info[(size_t)q * BA_INFO_WORDS] != 0.0) return;
  double* st = state + (size_t)q * POSE_STATE_WORDS;
  const double* cq = cams + (size_t)q * L * LM_CAM_WORDS;
  const double nf = st[0];
  const int count = (nf >= 0.0 && nf < 2147483647.0) ? (int)nf : 0;
  const int n = n_frames_host >= 0 ? n_frames_host : count;
  bool seen = false;
  for (int c = 0; c < L; ++c) {
    const double* cam = cq + c * LM_CAM_WORDS;
    if (cam[16] == 0.0) continue;
    if (!seen) {                                             // the first valid view is the held one
      seen = true;
      continue;
    }
    const int f = n - L + c;
    if (f < 0 || f >= capacity) continue;
    double* row = table + ((size_t)q * capacity + f) * POSE_ROW_WORDS;
#pragma unroll
    for (int k = 0; k < 12; ++k) row[k] = cam[k];
    row[14] = (double)((int)row[14] | BA_FLAG_ADJUSTED);
    const double* prev = cam - LM_CAM_WORDS;                 // (c >= 1: a valid view came before)
    if (prev[16] != 0.0) {
      const double d0 = cam[9] - prev[9], d1 = cam[10] - prev[10], d2 = cam[11] - prev[11];
      const double len = sqrt(dot3(d0, d1, d2, d0, d1, d2));
      if (isfinite(len) && len > PNP_SCALE_FRACTION * row[12]) row[12] = len;
    }
    if (c == L - 1 && count == n && n < capacity) {
      st[1] = row[12];
#pragma unroll
      for (int k = 0; k < 9; ++k) st[2 + k] = cam[k];
#pragma unroll
      for (int i = 0; i < 3; ++i) st[11 + i] = -dot3(cam[3 * i], cam[3 * i + 1], cam[3 * i + 2], cam[9], cam[10], cam[11]);
    }
  }
}

}  // namespace sspk
