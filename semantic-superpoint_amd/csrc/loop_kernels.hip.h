// Loop closure: a frame's map matches joined with the OLD rows of the world map and the frame's window
// landmarks, the loop edge measured from the pose found against those rows, a Sim(3) pose graph over the trajectory rows since the
// old place was last seen, and the write-back into the trajectory, the chain state and the map.  tests/loop_ref.py restates the
// rules in numpy; everything here is fp64 with contraction off and every sum in the order of that file.
//   loop_corr_kernel        one workgroup: "frame point -> lowest landmark row" in LDS (atomicMin: no order to depend on), then per
//                           match row the correspondence of world_corr_kernel when the map row is old, and the point's landmark
//   loop_edge_kernel        one workgroup: inlier count, anchor (a maximum) and the two depth sums in block_sum's order, then
//                           one thread: sigma, the acceptance rule, the edge row, the counters, the candidate record
//   loop_graph_kernel       ONE persistent workgroup of 512 threads: Levenberg-Marquardt over the free nodes with every phase
//                           (residuals and Jacobians per edge, normal blocks per node row, block cyclic reduction over the 7x7
//                           block tridiagonal system with up to 57 right-hand sides, the Woodbury correction through a Cholesky of
//                           at most 56 x 56 in LDS, the candidate and its cost, accept / reject) separated by workgroup barriers;
//                           all matrices live in the workspace, so no thread holds more than two 7-vectors
//   loop_apply_map_kernel   a thread per map row: rows last seen in (a, f] keep their coordinates in their camera's frame
//   loop_apply_rows_kernel  a thread per trajectory row: rows a + 1 .. f, the chain state
// Needs: geom_blocks.hip.h, pose_kernels.hip.h (POSE_*), landmark_kernels.hip.h (LM_WORDS), pnp_kernels.hip.h (rows, pnp_owner_table).
#pragma once

namespace sspk {

#define LOOP_MAX_EDGES 256
#define LOOP_EDGE_WORDS 16     // i, j, R [9], t [3], log sigma, weight
#define LOOP_STATE_WORDS 8     // edges, frame of the last accepted edge, refused, dropped (full), accepted by the last call, its anchor,
                               // its inliers, map rows left unchanged because the result was not finite
#define LOOP_CAND_WORDS 16     // frame, anchor, inliers, shared depths, sigma, angle of R_c, |t_c|, accepted, reason, 7 spare
#define LOOP_MAX_INNER 8
#define LOOP_INFO_WORDS 8
#define LOOP_FLAG_LOOP 32
#define LOOP_NR (1 + 7 * LOOP_MAX_INNER)   // right-hand sides of the block solve
#define LOOP_THREADS 512
#define LOOP_Q_MAX (7 * LOOP_MAX_INNER)
#define LOOP_LAMBDA0 1e-4
#define LOOP_LAMBDA_MIN 1e-12
#define LOOP_LAMBDA_MAX 1e6
#define LOOP_MAX_ITERATIONS 64

// grid (1), 256 threads, dynamic LDS point_cap ints.  corr [cap][PNP_CORR_WORDS], xnew [cap][4], n_out [3] = rows, valid old rows, those with a landmark.
__global__ __launch_bounds__(256) void loop_corr_kernel(const double* __restrict__ map_x, const int32_t* __restrict__ map_last,
                                                        const int32_t* __restrict__ world_state, int map_cap,
                                                        const float* __restrict__ match, const int32_t* __restrict__ n_match, int cap,
                                                        const double* __restrict__ pts_new, int pt_stride,
                                                        const int32_t* __restrict__ count_new, int point_cap,
                                                        const double* __restrict__ landmarks, const int32_t* __restrict__ n_landmarks,
                                                        int row_cap, int f, int min_gap, double* __restrict__ corr,
                                                        double* __restrict__ xnew, int32_t* __restrict__ n_out) {
  extern __shared__ int loop_owner[];
  const int tid = threadIdx.x;
  pnp_owner_table(loop_owner, point_cap, landmarks, min(max(n_landmarks[0], 0), row_cap), tid, 256);
  const int n_rows = min(max(world_state[0], 0), map_cap), count = min(max(count_new[0], 0), point_cap);
  const int n = min(max(n_match[0], 0), cap);
  const long long newest_old = (long long)f - (long long)min_gap;
  int total = 0, total_lm = 0;
  for (int k0 = 0; k0 < cap; k0 += 256) {
    const int k = k0 + tid;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, x[3] = {0.0, 0.0, 0.0};
    int row = 0;
    bool valid = false, has = false;
    if (k < n) {
      const float fi = match[(size_t)k * 3], fj = match[(size_t)k * 3 + 1];
      if (fi >= 0.f && fi < (float)n_rows && fj >= 0.f && fj < (float)count) {
        row = (int)fi;
        const int j = (int)fj;
        if ((long long)map_last[row] <= newest_old) {
          const double* px = pts_new + (size_t)j * pt_stride;
          v[0] = map_x[(size_t)row * 3];
          v[1] = map_x[(size_t)row * 3 + 1];
          v[2] = map_x[(size_t)row * 3 + 2];
          v[3] = px[0];
          v[4] = px[1];
          valid = pnp_finite5(v);
          const int r = loop_owner[j];
          if (valid && r != PNP_NO_OWNER) {
            const double* lm = landmarks + (size_t)r * LM_WORDS;
            x[0] = lm[1];
            x[1] = lm[2];
            x[2] = lm[3];
            has = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
          }
        }
      }
    }
    if (k < cap) {
      pnp_store_corr(corr + (size_t)k * PNP_CORR_WORDS, v, row, valid);
      double* q = xnew + (size_t)k * 4;
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c] = has ? x[c] : 0.0;
      q[3] = has ? 1.0 : 0.0;
    }
    total += __syncthreads_count(valid);
    total_lm += __syncthreads_count(has);
  }
  if (tid == 0) {
    n_out[0] = n;
    n_out[1] = total;
    n_out[2] = total_lm;
  }
}

// grid (1), 256 threads.  The pose of frame f against the old rows (rw, c, mask [cap], status of ssp_pnp_ransac), corr / xnew / n of
// loop_corr_kernel, the map's last_frame column, the trajectory table.  edges [LOOP_MAX_EDGES][LOOP_EDGE_WORDS], state
// [LOOP_STATE_WORDS], cand [LOOP_CAND_WORDS].
__global__ __launch_bounds__(256) void loop_edge_kernel(const double* __restrict__ rw_in, const double* __restrict__ c_in,
                                                        const uint8_t* __restrict__ mask, const int32_t* __restrict__ status_in,
                                                        const double* __restrict__ corr, const double* __restrict__ xnew,
                                                        const int32_t* __restrict__ n_in, int cap, const int32_t* __restrict__ map_last,
                                                        int map_cap, const double* __restrict__ table, int capacity, int f,
                                                        int min_inliers, int cooldown, double weight, double* __restrict__ edges,
                                                        int32_t* __restrict__ state, double* __restrict__ cand) {
#pragma clang fp contract(off)
  __shared__ double red[256 / 64];
  __shared__ int s_anchor;
  const int tid = threadIdx.x;
  if (tid == 0) s_anchor = -1;
  __syncthreads();
  const int rows = min(max(n_in[0], 0), cap);
  const bool in_table = f >= 0 && f < capacity;
  double Rl[9], Cl[3], Rw[9], C[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    Rl[k] = rw_in[k];
    Rw[k] = in_table ? table[(size_t)f * POSE_ROW_WORDS + k] : ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Cl[k] = c_in[k];
    C[k] = in_table ? table[(size_t)f * POSE_ROW_WORDS + 9 + k] : 0.0;
  }
  int inliers = 0;
  double sa = 0.0, sb = 0.0, sc = 0.0;
  for (int k0 = 0; k0 < cap; k0 += 256) {
    const int k = k0 + tid;
    bool inl = false;
    if (k < rows) {
      const double* o = corr + (size_t)k * PNP_CORR_WORDS;
      inl = mask[k] != 0 && o[6] != 0.0;
      if (inl) {
        const int row = min(max((int)o[5], 0), map_cap - 1);
        atomicMax(&s_anchor, map_last[row]);
        const double* q = xnew + (size_t)k * 4;
        if (q[3] != 0.0) {
          sa = sa + dot3(Rl[6], Rl[7], Rl[8], o[0] - Cl[0], o[1] - Cl[1], o[2] - Cl[2]);
          sb = sb + dot3(Rw[6], Rw[7], Rw[8], q[0] - C[0], q[1] - C[1], q[2] - C[2]);
          sc = sc + 1.0;
        }
      }
    }
    inliers += __syncthreads_count(inl);
  }
  const double SA = block_sum<256>(sa, red), SB = block_sum<256>(sb, red);
  const int shared = (int)block_sum<256>(sc, red);
  if (tid != 0) return;
  const int a = s_anchor;
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) fin = fin && isfinite(Rl[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) fin = fin && isfinite(Cl[k]);
  const bool posed = status_in[0] == 0 && fin && in_table;
  const double sigma = shared > 0 ? SA / SB : 0.0;
  const bool scale_ok = shared >= POSE_MIN_FRONT && isfinite(sigma) && sigma > 0.0;
  const int n_edges = min(max(state[0], 0), LOOP_MAX_EDGES);
  int reason;
  if (!posed) reason = 1;
  else if (inliers < min_inliers) reason = 2;
  else if (!scale_ok) reason = 3;
  else if (!(a >= 0 && a < f)) reason = 4;
  else if (n_edges > 0 && (long long)f - (long long)state[1] < (long long)cooldown) reason = 5;
  else if (n_edges >= LOOP_MAX_EDGES) reason = 6;
  else reason = 0;
#pragma unroll
  for (int k = 0; k < LOOP_CAND_WORDS; ++k) cand[k] = 0.0;
  cand[0] = (double)f;
  cand[1] = (double)a;
  cand[2] = (double)inliers;
  cand[3] = (double)shared;
  cand[8] = (double)reason;
  state[4] = 0;
  state[5] = a;
  state[6] = inliers;
  if (reason >= 1 && reason <= 5) state[2] = state[2] + 1;
  if (reason == 6) state[3] = state[3] + 1;
  if (posed && scale_ok) {
    double Rc[9], tc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) Rc[3 * r + c] = dot3(Rl[r], Rl[3 + r], Rl[6 + r], Rw[c], Rw[3 + c], Rw[6 + c]);
#pragma unroll
    for (int r = 0; r < 3; ++r) tc[r] = Cl[r] - sigma * dot3(Rc[3 * r], Rc[3 * r + 1], Rc[3 * r + 2], C[0], C[1], C[2]);
    const double tr = (Rc[0] + Rc[4]) + Rc[8];
    const double k0 = Rc[7] - Rc[5], k1 = Rc[2] - Rc[6], k2 = Rc[3] - Rc[1];
    cand[4] = sigma;
    cand[5] = atan2(sqrt(dot3(k0, k1, k2, k0, k1, k2)), tr - 1.0);
    cand[6] = sqrt(dot3(tc[0], tc[1], tc[2], tc[0], tc[1], tc[2]));
  }
  if (reason == 0) {
    const double* ra = table + (size_t)a * POSE_ROW_WORDS;
    double* o = edges + (size_t)n_edges * LOOP_EDGE_WORDS;
    const double d0 = Cl[0] - ra[9], d1 = Cl[1] - ra[10], d2 = Cl[2] - ra[11];
    o[0] = (double)a;
    o[1] = (double)f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[2 + 3 * r + c] = dot3(Rl[3 * r], Rl[3 * r + 1], Rl[3 * r + 2], ra[3 * c], ra[3 * c + 1], ra[3 * c + 2]);
      o[11 + r] = dot3(ra[3 * r], ra[3 * r + 1], ra[3 * r + 2], d0, d1, d2);
    }
    o[14] = log(sigma);
    o[15] = weight;
    state[0] = n_edges + 1;
    state[1] = f;
    state[4] = 1;
    cand[7] = 1.0;
  }
}

// ---- the pose graph ----
// Workspace (doubles) of a table of `capacity` rows: M = capacity nodes at most, E = M + LOOP_MAX_EDGES edges.
struct LoopWs {
  double *R, *C, *l, *Rn, *Cn, *ln;    // current and candidate nodes, index 0 = the anchor: [M + 1][9], [M + 1][3], [M + 1]
  double *meas;                        // per edge: Rz [9], tz [3], lz, bz, weight, spare: [E][16]
  double *res, *Ji, *Jj;               // per edge: [E][7], [E][49], [E][49]
  double *D, *Lo, *Up, *F, *B;         // per node: [M][49] x 4, [M][7][LOOP_NR]
};

__host__ __device__ inline size_t loop_ws_words(int capacity) {
  const size_t M = (size_t)capacity, E = M + LOOP_MAX_EDGES;
  return 2 * (M + 1) * 13 + E * (16 + 7 + 98) + M * (4 * 49 + 7 * LOOP_NR);
}

__host__ __device__ inline LoopWs loop_ws_of(double* p, int capacity) {
  const size_t M = (size_t)capacity, E = M + LOOP_MAX_EDGES;
  LoopWs w;
  w.R = p; p += (M + 1) * 9;
  w.C = p; p += (M + 1) * 3;
  w.l = p; p += (M + 1);
  w.Rn = p; p += (M + 1) * 9;
  w.Cn = p; p += (M + 1) * 3;
  w.ln = p; p += (M + 1);
  w.meas = p; p += E * 16;
  w.res = p; p += E * 7;
  w.Ji = p; p += E * 49;
  w.Jj = p; p += E * 49;
  w.D = p; p += M * 49;
  w.Lo = p; p += M * 49;
  w.Up = p; p += M * 49;
  w.F = p; p += M * 49;
  w.B = p;
  return w;
}

// the ends of edge e: a fixed end (node index <= 0) reads the table's row, a free one the node arrays (R, C, l)
struct LoopEnds {
  double Ri[9], Ci[3], li, Rj[9], Cj[3], lj;
};

__device__ __forceinline__ void loop_ends(int e, int m, int a, const int* s_ei, const int* s_ej, const double* table, const double* R,
                                          const double* C, const double* l, LoopEnds& o) {
  const int ni = e < m ? e : s_ei[e - m], nj = e < m ? e + 1 : s_ej[e - m];
  if (ni <= 0) {
    const double* row = table + (size_t)(a + ni) * POSE_ROW_WORDS;
#pragma unroll
    for (int k = 0; k < 9; ++k) o.Ri[k] = row[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.Ci[k] = row[9 + k];
    o.li = 0.0;
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) o.Ri[k] = R[(size_t)ni * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.Ci[k] = C[(size_t)ni * 3 + k];
    o.li = l[ni];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) o.Rj[k] = R[(size_t)nj * 9 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) o.Cj[k] = C[(size_t)nj * 3 + k];
  o.lj = l[nj];
}

// residual of one edge into r [7]; with J: the Jacobians Ji, Jj [49] (row-major, rows = residuals)
__device__ __forceinline__ void loop_residual(const LoopEnds& n, const double* __restrict__ z, double* r, double* Ji, double* Jj) {
#pragma clang fp contract(off)
  double Rr[9], E[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rr[3 * i + j] = dot3(n.Rj[3 * i], n.Rj[3 * i + 1], n.Rj[3 * i + 2], n.Ri[3 * j], n.Ri[3 * j + 1], n.Ri[3 * j + 2]);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) E[3 * i + j] = dot3(z[i], z[3 + i], z[6 + i], Rr[j], Rr[3 + j], Rr[6 + j]);
  const double bz = z[13], ei = exp(-n.li);
  const double d0 = n.Cj[0] - n.Ci[0], d1 = n.Cj[1] - n.Ci[1], d2 = n.Cj[2] - n.Ci[2];
  double tr[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) tr[i] = ei * dot3(n.Ri[3 * i], n.Ri[3 * i + 1], n.Ri[3 * i + 2], d0, d1, d2);
  r[0] = 0.5 * (E[7] - E[5]);
  r[1] = 0.5 * (E[2] - E[6]);
  r[2] = 0.5 * (E[3] - E[1]);
#pragma unroll
  for (int i = 0; i < 3; ++i) r[3 + i] = (tr[i] - z[9 + i]) / bz;
  r[6] = (n.lj - n.li) - z[12];
  if (Ji == nullptr) return;
#pragma unroll
  for (int k = 0; k < 49; ++k) {
    Ji[k] = 0.0;
    Jj[k] = 0.0;
  }
  const double trace = (E[0] + E[4]) + E[8];
  double TmE[9];                                              // trace I - E
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) TmE[3 * i + j] = trace * (i == j ? 1.0 : 0.0) - E[3 * i + j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Ji[7 * i + j] = -0.5 * (trace * (i == j ? 1.0 : 0.0) - E[3 * j + i]);
      Jj[7 * i + j] = 0.5 * dot3(TmE[3 * i], TmE[3 * i + 1], TmE[3 * i + 2], z[3 * j], z[3 * j + 1], z[3 * j + 2]);
    }
  const double ib = 1.0 / bz, eb = ei * ib;
  const double cr[9] = {0.0, -tr[2], tr[1], tr[2], 0.0, -tr[0], -tr[1], tr[0], 0.0};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Ji[7 * (3 + i) + j] = -cr[3 * i + j] * ib;
      const double rs = n.Ri[3 * i + j] * eb;
      Ji[7 * (3 + i) + 3 + j] = -rs;
      Jj[7 * (3 + i) + 3 + j] = rs;
    }
    Ji[7 * (3 + i) + 6] = -tr[i] * ib;
  }
  Ji[48] = -1.0;
  Jj[48] = 1.0;
}

// sum_q A[q][r] B[q][c] over q = 0..6 of two row-major 7x7 blocks, in ascending q
__device__ __forceinline__ double loop_ata(const double* A, int r, const double* B, int c) {
#pragma clang fp contract(off)
  double acc = A[r] * B[c];
#pragma unroll
  for (int q = 1; q < 7; ++q) acc = acc + A[7 * q + r] * B[7 * q + c];
  return acc;
}

__device__ __forceinline__ double loop_atv(const double* A, int r, const double* v) {
#pragma clang fp contract(off)
  double acc = A[r] * v[0];
#pragma unroll
  for (int q = 1; q < 7; ++q) acc = acc + A[7 * q + r] * v[q];
  return acc;
}

// grid (1), LOOP_THREADS threads.  table [capacity][POSE_ROW_WORDS]; edges / state of loop_edge_kernel; f the newest frame.
// rw_out [capacity][9], c_out [capacity][3], sigma_out [capacity], info [LOOP_INFO_WORDS].
__global__ __launch_bounds__(LOOP_THREADS) void loop_graph_kernel(const double* __restrict__ table, int capacity,
                                                                  const double* __restrict__ edges, const int32_t* __restrict__ state,
                                                                  int f, int iterations, double* ws, double* rw_out, double* c_out,
                                                                  double* sigma_out, double* info) {
#pragma clang fp contract(off)
  __shared__ int s_ei[LOOP_MAX_EDGES], s_ej[LOOP_MAX_EDGES], s_row[LOOP_MAX_EDGES];
  __shared__ int s_cnt[4];                // fixed-end edges, both-ends-free edges used, left out, bad
  __shared__ double s_ctl[4];             // lambda, current cost, candidate cost, accepted steps
  __shared__ double s_S[LOOP_Q_MAX * LOOP_Q_MAX], s_z[LOOP_Q_MAX], s_vty[LOOP_Q_MAX];
  const int tid = threadIdx.x;
  const int a = state[5];
  const bool go = state[4] != 0 && a >= 0 && a < f && f < capacity;
  // the copies: every row of the table, sigma 1
  for (int k = tid; k < capacity; k += LOOP_THREADS) {
    const double* row = table + (size_t)k * POSE_ROW_WORDS;
#pragma unroll
    for (int c = 0; c < 9; ++c) rw_out[(size_t)k * 9 + c] = row[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) c_out[(size_t)k * 3 + c] = row[9 + c];
    sigma_out[k] = 1.0;
  }
  if (!go) {
    if (tid < LOOP_INFO_WORDS) info[tid] = tid == 0 ? 1.0 : 0.0;
    return;
  }
  const int m = f - a;
  const LoopWs w = loop_ws_of(ws, capacity);
  if (tid == 0) {
    // the stored edges this graph uses, in table order: fixed-end ones first, then the last LOOP_MAX_INNER both-ends-free ones
    const int ne = min(max(state[0], 0), LOOP_MAX_EDGES);
    int n_inner_all = 0, n_fixed = 0;
    for (int e = 0; e < ne; ++e) {
      const int i = (int)edges[(size_t)e * LOOP_EDGE_WORDS], j = (int)edges[(size_t)e * LOOP_EDGE_WORDS + 1];
      if (!(j > a && j <= f && i >= 0 && i < j)) continue;
      if (i > a) {
        n_inner_all += 1;
      } else {
        s_ei[n_fixed] = i - a;
        s_ej[n_fixed] = j - a;
        s_row[n_fixed] = e;
        n_fixed += 1;
      }
    }
    const int left = max(0, n_inner_all - LOOP_MAX_INNER);
    int seen = 0, n_inner = 0;
    for (int e = 0; e < ne; ++e) {
      const int i = (int)edges[(size_t)e * LOOP_EDGE_WORDS], j = (int)edges[(size_t)e * LOOP_EDGE_WORDS + 1];
      if (!(j > a && j <= f && i >= 0 && i < j) || i <= a) continue;
      seen += 1;
      if (seen <= left) continue;
      s_ei[n_fixed + n_inner] = i - a;
      s_ej[n_fixed + n_inner] = j - a;
      s_row[n_fixed + n_inner] = e;
      n_inner += 1;
    }
    s_cnt[0] = n_fixed;
    s_cnt[1] = n_inner;
    s_cnt[2] = left;
    s_cnt[3] = 0;
    s_ctl[0] = LOOP_LAMBDA0;
    s_ctl[3] = 0.0;
  }
  for (int k = tid; k <= m; k += LOOP_THREADS) {
    const double* row = table + (size_t)(a + k) * POSE_ROW_WORDS;
#pragma unroll
    for (int c = 0; c < 9; ++c) w.R[(size_t)k * 9 + c] = w.Rn[(size_t)k * 9 + c] = row[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) w.C[(size_t)k * 3 + c] = w.Cn[(size_t)k * 3 + c] = row[9 + c];
    w.l[k] = w.ln[k] = 0.0;
  }
  __syncthreads();
  const int n_fixed = s_cnt[0], n_inner = s_cnt[1], n_loops = n_fixed + n_inner, n_e = m + n_loops;
  const int nr = 1 + 7 * n_inner, qn = 7 * n_inner;
  // the measurements
  for (int e = tid; e < n_e; e += LOOP_THREADS) {
    double* z = w.meas + (size_t)e * 16;
    if (e < m) {
      const double* ri = w.R + (size_t)e * 9;
      const double* rj = ri + 9;
      const double* ci = w.C + (size_t)e * 3;
      const double d0 = ci[3] - ci[0], d1 = ci[4] - ci[1], d2 = ci[5] - ci[2];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) z[3 * r + c] = dot3(rj[3 * r], rj[3 * r + 1], rj[3 * r + 2], ri[3 * c], ri[3 * c + 1], ri[3 * c + 2]);
        z[9 + r] = dot3(ri[3 * r], ri[3 * r + 1], ri[3 * r + 2], d0, d1, d2);
      }
      z[12] = 0.0;
      z[14] = 1.0;
    } else {
      const double* o = edges + (size_t)s_row[e - m] * LOOP_EDGE_WORDS;
#pragma unroll
      for (int c = 0; c < 13; ++c) z[c] = o[2 + c];
      z[14] = o[15];
    }
    const double b = sqrt(dot3(z[9], z[10], z[11], z[9], z[10], z[11]));
    z[13] = (isfinite(b) && b > 0.0) ? b : 1.0;
    z[15] = 0.0;
  }
  __syncthreads();
  for (int it = -1; it < iterations; ++it) {
    // residuals (and Jacobians) of the current nodes; iteration -1 only measures the cost before
    for (int e = tid; e < n_e; e += LOOP_THREADS) {
      LoopEnds n;
      loop_ends(e, m, a, s_ei, s_ej, table, w.R, w.C, w.l, n);
      double r[7];
      loop_residual(n, w.meas + (size_t)e * 16, r, it < 0 ? nullptr : w.Ji + (size_t)e * 49, it < 0 ? nullptr : w.Jj + (size_t)e * 49);
#pragma unroll
      for (int c = 0; c < 7; ++c) w.res[(size_t)e * 7 + c] = r[c];
    }
    __syncthreads();
    if (it < 0) {
      if (tid == 0) {
        double c = 0.0;
        for (int e = 0; e < n_e; ++e) {
          const double* r = w.res + (size_t)e * 7;
          c = c + w.meas[(size_t)e * 16 + 14] * ((((((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]) + r[4] * r[4]) + r[5] * r[5]) + r[6] * r[6]);
        }
        s_ctl[1] = c;
        info[1] = c;
      }
      __syncthreads();
      const double c0 = s_ctl[1];
      if (!(c0 > 0.0) || !isfinite(c0)) {
        if (tid == 0) {
          info[0] = 1.0;
          info[2] = c0;
          info[3] = (double)m;
          info[4] = (double)n_e;
          info[5] = 0.0;
          info[6] = (double)s_cnt[2];
          info[7] = 0.0;
        }
        return;
      }
      continue;
    }
    const double lambda = s_ctl[0];
    // normal blocks, a thread per (node, row): chain edge in, chain edge out, the fixed-end loop edges, the free ones (g, diagonal)
    for (int x = tid; x < m * 7; x += LOOP_THREADS) {
      const int k = x / 7, r = x - 7 * k;
      const double* Jin = w.Jj + (size_t)k * 49;                  // edge k = (k - 1, k) in free-node numbering: this node is its j
      const double* Jout_i = w.Ji + (size_t)(k + 1) * 49;         // edge k + 1: this node is its i
      const double* Jout_j = w.Jj + (size_t)(k + 1) * 49;
      const double* Jin_i = w.Ji + (size_t)k * 49;
      const bool out = k + 1 < m;
      double d[7], g;
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        d[c] = loop_ata(Jin, r, Jin, c);
        if (out) d[c] = d[c] + loop_ata(Jout_i, r, Jout_i, c);
        w.Up[(size_t)k * 49 + 7 * r + c] = out ? loop_ata(Jout_i, r, Jout_j, c) : 0.0;
        w.Lo[(size_t)k * 49 + 7 * r + c] = k > 0 ? loop_ata(Jin_i, c, Jin, r) : 0.0;
      }
      g = loop_atv(Jin, r, w.res + (size_t)k * 7);
      if (out) g = g + loop_atv(Jout_i, r, w.res + (size_t)(k + 1) * 7);
      for (int y = 0; y < n_fixed; ++y) {
        if (s_ej[y] - 1 != k) continue;
        const int e = m + y;
        const double wt = w.meas[(size_t)e * 16 + 14];
        const double* J = w.Jj + (size_t)e * 49;
#pragma unroll
        for (int c = 0; c < 7; ++c) d[c] = d[c] + wt * loop_ata(J, r, J, c);
        g = g + wt * loop_atv(J, r, w.res + (size_t)e * 7);
      }
      double dfull = 0.0;
#pragma unroll
      for (int c = 0; c < 7; ++c) dfull = c == r ? d[c] : dfull;
      for (int y = n_fixed; y < n_loops; ++y) {
        const int e = m + y;
        const double wt = w.meas[(size_t)e * 16 + 14];
        if (s_ei[y] - 1 == k) {
          const double* J = w.Ji + (size_t)e * 49;
          g = g + wt * loop_atv(J, r, w.res + (size_t)e * 7);
          dfull = dfull + wt * loop_ata(J, r, J, r);
        }
        if (s_ej[y] - 1 == k) {
          const double* J = w.Jj + (size_t)e * 49;
          g = g + wt * loop_atv(J, r, w.res + (size_t)e * 7);
          dfull = dfull + wt * loop_ata(J, r, J, r);
        }
      }
#pragma unroll
      for (int c = 0; c < 7; ++c) w.D[(size_t)k * 49 + 7 * r + c] = c == r ? d[c] + lambda * dfull : d[c];
      double* b = w.B + ((size_t)k * 7 + r) * LOOP_NR;
      b[0] = -g;
      for (int c = 1; c < nr; ++c) b[c] = 0.0;
    }
    __syncthreads();
    for (int x = tid; x < n_inner * 49; x += LOOP_THREADS) {      // the low-rank columns: sqrt(weight) J^T at the two ends
      const int y = x / 49, c = (x - 49 * y) / 7, r = x - 49 * y - 7 * c;
      const int e = m + n_fixed + y;
      const double sw = sqrt(w.meas[(size_t)e * 16 + 14]);
      w.B[((size_t)(s_ei[n_fixed + y] - 1) * 7 + r) * LOOP_NR + 1 + 7 * y + c] = sw * w.Ji[(size_t)e * 49 + 7 * c + r];
      w.B[((size_t)(s_ej[n_fixed + y] - 1) * 7 + r) * LOOP_NR + 1 + 7 * y + c] = sw * w.Jj[(size_t)e * 49 + 7 * c + r];
    }
    __syncthreads();
    // block cyclic reduction
    int top = 1;
    for (int s = 1; s - 1 < m; s <<= 1) {
      top = s;
      const int nj = (m - (s - 1) + 2 * s - 1) / (2 * s);        // nodes j = s - 1, 3s - 1, ... below m
      for (int x = tid; x < nj; x += LOOP_THREADS) {              // Cholesky of D_j, a thread per node
        const size_t j = (size_t)(s - 1) + (size_t)x * 2 * s;
        const double* A = w.D + j * 49;
        double* L = w.F + j * 49;
        for (int c = 0; c < 7; ++c) {
          double v = A[7 * c + c];
          for (int k = 0; k < c; ++k) v = v - L[7 * c + k] * L[7 * c + k];
          const double dg = sqrt(v);
          L[7 * c + c] = dg;
          for (int r = c + 1; r < 7; ++r) {
            double u = A[7 * r + c];
            for (int k = 0; k < c; ++k) u = u - L[7 * r + k] * L[7 * c + k];
            L[7 * r + c] = u / dg;
          }
        }
      }
      __syncthreads();
      const int ncol = 14 + nr;
      for (int x = tid; x < nj * ncol; x += LOOP_THREADS) {       // D_j^-1 [Lo | Up | B], a thread per (node, column)
        const int xn = x / ncol, col = x - xn * ncol;
        const size_t j = (size_t)(s - 1) + (size_t)xn * 2 * s;
        const double* L = w.F + j * 49;
        double* p;
        int stride;
        if (col < 7) {
          p = w.Lo + j * 49 + col;
          stride = 7;
        } else if (col < 14) {
          p = w.Up + j * 49 + (col - 7);
          stride = 7;
        } else {
          p = w.B + j * 7 * LOOP_NR + (col - 14);
          stride = LOOP_NR;
        }
        double y[7], v[7];
#pragma unroll
        for (int r = 0; r < 7; ++r) {
          double u = p[(size_t)r * stride];
#pragma unroll
          for (int k = 0; k < r; ++k) u = u - L[7 * r + k] * y[k];
          y[r] = u / L[7 * r + r];
        }
#pragma unroll
        for (int r = 6; r >= 0; --r) {
          double u = y[r];
#pragma unroll
          for (int k = r + 1; k < 7; ++k) u = u - L[7 * k + r] * v[k];
          v[r] = u / L[7 * r + r];
        }
#pragma unroll
        for (int r = 0; r < 7; ++r) p[(size_t)r * stride] = v[r];
      }
      __syncthreads();
      const int ni = 2 * s - 1 < m ? (m - (2 * s - 1) + 2 * s - 1) / (2 * s) : 0;   // nodes i = 2s - 1, 4s - 1, ... below m
      for (int x = tid; x < ni * 7; x += LOOP_THREADS) {          // the neighbours eliminated into node i, a thread per (node, row)
        const int xn = x / 7, r = x - 7 * xn;
        const size_t i = (size_t)(2 * s - 1) + (size_t)xn * 2 * s, le = i - s, ri = i + s;
        const bool has = ri < (size_t)m;
        double lo[7], up[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          lo[k] = w.Lo[i * 49 + 7 * r + k];
          up[k] = w.Up[i * 49 + 7 * r + k];
        }
        const double* Lt_le = w.Lo + le * 49;
        const double* Ut_le = w.Up + le * 49;
        const double* Bt_le = w.B + le * 7 * LOOP_NR;
        const double* Lt_ri = w.Lo + (has ? ri : le) * 49;
        const double* Ut_ri = w.Up + (has ? ri : le) * 49;
        const double* Bt_ri = w.B + (has ? ri : le) * 7 * LOOP_NR;
#pragma unroll
        for (int c = 0; c < 7; ++c) {
          double p0 = lo[0] * Ut_le[c], p1 = lo[0] * Lt_le[c], p2 = up[0] * Lt_ri[c], p3 = up[0] * Ut_ri[c];
#pragma unroll
          for (int k = 1; k < 7; ++k) {
            p0 = p0 + lo[k] * Ut_le[7 * k + c];
            p1 = p1 + lo[k] * Lt_le[7 * k + c];
            p2 = p2 + up[k] * Lt_ri[7 * k + c];
            p3 = p3 + up[k] * Ut_ri[7 * k + c];
          }
          double dn = w.D[i * 49 + 7 * r + c] - p0;
          if (has) dn = dn - p2;
          w.D[i * 49 + 7 * r + c] = dn;
          w.Lo[i * 49 + 7 * r + c] = -p1;
          w.Up[i * 49 + 7 * r + c] = has ? -p3 : 0.0;
        }
        double* bi = w.B + (i * 7 + r) * LOOP_NR;
        for (int c = 0; c < nr; ++c) {
          double p0 = lo[0] * Bt_le[c], p2 = up[0] * Bt_ri[c];
#pragma unroll
          for (int k = 1; k < 7; ++k) {
            p0 = p0 + lo[k] * Bt_le[(size_t)k * LOOP_NR + c];
            p2 = p2 + up[k] * Bt_ri[(size_t)k * LOOP_NR + c];
          }
          double bn = bi[c] - p0;
          if (has) bn = bn - p2;
          bi[c] = bn;
        }
      }
      __syncthreads();
    }
    for (int s = top; s >= 1; s >>= 1) {                            // back substitution, a thread per (node, row, column)
      const int nj = (m - (s - 1) + 2 * s - 1) / (2 * s);
      for (int x = tid; x < nj * 7 * nr; x += LOOP_THREADS) {
        const int xn = x / (7 * nr), rem = x - xn * 7 * nr, r = rem / nr, c = rem - r * nr;
        const long long j = (long long)(s - 1) + (long long)xn * 2 * s, le = j - s, ri = j + s;
        double v = w.B[((size_t)j * 7 + r) * LOOP_NR + c];
        if (le >= 0) {
          const double* Lt = w.Lo + (size_t)j * 49 + 7 * r;
          const double* X = w.B + (size_t)le * 7 * LOOP_NR + c;
          double p = Lt[0] * X[0];
#pragma unroll
          for (int k = 1; k < 7; ++k) p = p + Lt[k] * X[(size_t)k * LOOP_NR];
          v = v - p;
        }
        if (ri < m) {
          const double* Ut = w.Up + (size_t)j * 49 + 7 * r;
          const double* X = w.B + (size_t)ri * 7 * LOOP_NR + c;
          double p = Ut[0] * X[0];
#pragma unroll
          for (int k = 1; k < 7; ++k) p = p + Ut[k] * X[(size_t)k * LOOP_NR];
          v = v - p;
        }
        w.B[((size_t)j * 7 + r) * LOOP_NR + c] = v;
      }
      __syncthreads();
    }
    // Woodbury: S = I + V^T Y_V and V^T y_0, Cholesky in LDS, z = S^-1 V^T y_0
    if (qn > 0) {
      for (int x = tid; x < qn * nr; x += LOOP_THREADS) {
        const int row = x / nr, col = x - row * nr, y = row / 7, c = row - 7 * y;
        const int e = m + n_fixed + y;
        const double sw = sqrt(w.meas[(size_t)e * 16 + 14]);
        const double* Jp = w.Ji + (size_t)e * 49 + 7 * c;
        const double* Jq = w.Jj + (size_t)e * 49 + 7 * c;
        const double* Yp = w.B + (size_t)(s_ei[n_fixed + y] - 1) * 7 * LOOP_NR + col;
        const double* Yq = w.B + (size_t)(s_ej[n_fixed + y] - 1) * 7 * LOOP_NR + col;
        double acc = (sw * Jp[0]) * Yp[0];
#pragma unroll
        for (int r = 1; r < 7; ++r) acc = acc + (sw * Jp[r]) * Yp[(size_t)r * LOOP_NR];
#pragma unroll
        for (int r = 0; r < 7; ++r) acc = acc + (sw * Jq[r]) * Yq[(size_t)r * LOOP_NR];
        if (col == 0) s_vty[row] = acc;
        else s_S[row * LOOP_Q_MAX + col - 1] = acc + (col - 1 == row ? 1.0 : 0.0);
      }
      __syncthreads();
      for (int c = 0; c < qn; ++c) {                                // right-looking: each entry loses l l in ascending column
        if (tid == 0) s_S[c * LOOP_Q_MAX + c] = sqrt(s_S[c * LOOP_Q_MAX + c]);
        __syncthreads();
        const double dg = s_S[c * LOOP_Q_MAX + c];
        for (int r = c + 1 + tid; r < qn; r += LOOP_THREADS) s_S[r * LOOP_Q_MAX + c] = s_S[r * LOOP_Q_MAX + c] / dg;
        __syncthreads();
        const int rem = qn - c - 1;
        for (int x = tid; x < rem * rem; x += LOOP_THREADS) {
          const int r = c + 1 + x / rem, k = c + 1 + x % rem;
          if (k <= r) s_S[r * LOOP_Q_MAX + k] = s_S[r * LOOP_Q_MAX + k] - s_S[r * LOOP_Q_MAX + c] * s_S[k * LOOP_Q_MAX + c];
        }
        __syncthreads();
      }
      if (tid == 0) {
        for (int r = 0; r < qn; ++r) {
          double u = s_vty[r];
          for (int k = 0; k < r; ++k) u = u - s_S[r * LOOP_Q_MAX + k] * s_z[k];
          s_z[r] = u / s_S[r * LOOP_Q_MAX + r];
        }
        for (int r = qn - 1; r >= 0; --r) {
          double u = s_z[r];
          for (int k = r + 1; k < qn; ++k) u = u - s_S[k * LOOP_Q_MAX + r] * s_z[k];
          s_z[r] = u / s_S[r * LOOP_Q_MAX + r];
        }
      }
      __syncthreads();
    }
    // the candidate: delta = y_0 - Y_V z, a thread per node
    for (int k = tid; k < m; k += LOOP_THREADS) {
      double delta[6], dl = 0.0;
#pragma unroll
      for (int r = 0; r < 7; ++r) {
        const double* y = w.B + ((size_t)k * 7 + r) * LOOP_NR;
        double v = y[0];
        for (int c = 0; c < qn; ++c) v = v - y[1 + c] * s_z[c];
        if (r < 6) delta[r] = v;
        else dl = v;
      }
      double R[9], t[3] = {0.0, 0.0, 0.0};
      const double rot[6] = {delta[0], delta[1], delta[2], 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < 9; ++c) R[c] = w.R[(size_t)(k + 1) * 9 + c];
      bool fin = cayley_update(R, t, rot);
#pragma unroll
      for (int c = 0; c < 9; ++c) w.Rn[(size_t)(k + 1) * 9 + c] = R[c];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v = w.C[(size_t)(k + 1) * 3 + c] + delta[3 + c];
        fin = fin && isfinite(v);
        w.Cn[(size_t)(k + 1) * 3 + c] = v;
      }
      const double ln = w.l[k + 1] + dl;
      w.ln[k + 1] = ln;
      if (!(fin && isfinite(ln))) atomicOr(&s_cnt[3], 1);
    }
    __syncthreads();
    for (int e = tid; e < n_e; e += LOOP_THREADS) {
      LoopEnds n;
      loop_ends(e, m, a, s_ei, s_ej, table, w.Rn, w.Cn, w.ln, n);
      double r[7];
      loop_residual(n, w.meas + (size_t)e * 16, r, nullptr, nullptr);
#pragma unroll
      for (int c = 0; c < 7; ++c) w.res[(size_t)e * 7 + c] = r[c];
    }
    __syncthreads();
    if (tid == 0) {
      double c = 0.0;
      for (int e = 0; e < n_e; ++e) {
        const double* r = w.res + (size_t)e * 7;
        c = c + w.meas[(size_t)e * 16 + 14] * ((((((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]) + r[4] * r[4]) + r[5] * r[5]) + r[6] * r[6]);
      }
      const bool accept = isfinite(c) && s_cnt[3] == 0 && c < s_ctl[1];
      s_ctl[2] = accept ? 1.0 : 0.0;
      double lam = s_ctl[0];
      if (accept) {
        s_ctl[1] = c;
        s_ctl[3] = s_ctl[3] + 1.0;
        const double by_ten = lam / 10.0;
        lam = by_ten > LOOP_LAMBDA_MIN ? by_ten : LOOP_LAMBDA_MIN;
      } else {
        const double times_ten = lam * 10.0;
        lam = times_ten < LOOP_LAMBDA_MAX ? times_ten : LOOP_LAMBDA_MAX;
      }
      s_ctl[0] = lam;
      s_cnt[3] = 0;
    }
    __syncthreads();
    if (s_ctl[2] != 0.0) {
      for (int k = 1 + tid; k <= m; k += LOOP_THREADS) {
#pragma unroll
        for (int c = 0; c < 9; ++c) w.R[(size_t)k * 9 + c] = w.Rn[(size_t)k * 9 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) w.C[(size_t)k * 3 + c] = w.Cn[(size_t)k * 3 + c];
        w.l[k] = w.ln[k];
      }
    }
    __syncthreads();
  }
  const bool solved = s_ctl[3] > 0.0;
  if (solved) {
    for (int k = 1 + tid; k <= m; k += LOOP_THREADS) {
#pragma unroll
      for (int c = 0; c < 9; ++c) rw_out[(size_t)(a + k) * 9 + c] = w.R[(size_t)k * 9 + c];
#pragma unroll
      for (int c = 0; c < 3; ++c) c_out[(size_t)(a + k) * 3 + c] = w.C[(size_t)k * 3 + c];
      sigma_out[a + k] = exp(w.l[k]);
    }
  }
  if (tid == 0) {
    info[0] = solved ? 0.0 : 2.0;
    info[2] = s_ctl[1];
    info[3] = (double)m;
    info[4] = (double)n_e;
    info[5] = s_ctl[3];
    info[6] = (double)s_cnt[2];
    info[7] = s_ctl[0];
  }
}

// ---- apply ----
// grid (cdiv(map_cap, 256)).  Acts only under status 0.  table still holds the rows as they were; rw_new / c_new / sigma the graph's.
__global__ __launch_bounds__(256) void loop_apply_map_kernel(const double* __restrict__ info, const double* __restrict__ rw_new,
                                                             const double* __restrict__ c_new, const double* __restrict__ sigma,
                                                             int32_t* __restrict__ loop_state, int f, const double* __restrict__ table,
                                                             int capacity, double* __restrict__ map_x,
                                                             const int32_t* __restrict__ map_last, const int32_t* __restrict__ world_state,
                                                             int map_cap) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  const int a = loop_state[5];
  const bool go = info[0] == 0.0 && a >= 0 && a < f && f < capacity;
  const int n_rows = min(max(world_state[0], 0), map_cap);
  bool bad = false;
  if (go && s < n_rows) {
    const int k = map_last[s];
    if (k > a && k <= f) {
      const double* ro = table + (size_t)k * POSE_ROW_WORDS;
      const double* r1 = rw_new + (size_t)k * 9;
      const double* c1 = c_new + (size_t)k * 3;
      double* x = map_x + (size_t)s * 3;
      const double d0 = x[0] - ro[9], d1 = x[1] - ro[10], d2 = x[2] - ro[11];
      double y[3], xn[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) y[r] = dot3(ro[3 * r], ro[3 * r + 1], ro[3 * r + 2], d0, d1, d2);
      const double sg = sigma[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) xn[c] = c1[c] + sg * dot3(r1[c], r1[3 + c], r1[6 + c], y[0], y[1], y[2]);
      if (isfinite(xn[0]) && isfinite(xn[1]) && isfinite(xn[2])) {
        x[0] = xn[0];
        x[1] = xn[1];
        x[2] = xn[2];
      } else {
        bad = true;
      }
    }
  }
  const int n_bad = __syncthreads_count(bad);
  if (threadIdx.x == 0 && n_bad > 0) atomicAdd(&loop_state[7], n_bad);   // (an integer count: no order to depend on)
}

// grid (cdiv(capacity, 256)): after loop_apply_map_kernel.  Row k in a + 1 .. f takes the corrected Rw and C, s by ba_apply_kernel's
// rule and LOOP_FLAG_LOOP; the chain state follows row f when that is its newest frame and the table is not full.
__global__ __launch_bounds__(256) void loop_apply_rows_kernel(const double* __restrict__ info, const double* __restrict__ rw_new,
                                                              const double* __restrict__ c_new, const int32_t* __restrict__ loop_state,
                                                              int f, double* __restrict__ st, double* __restrict__ table, int capacity) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int a = loop_state[5];
  if (!(info[0] == 0.0 && a >= 0 && a < f && f < capacity)) return;
  if (k <= a || k > f) return;
  double* row = table + (size_t)k * POSE_ROW_WORDS;
  const double* r1 = rw_new + (size_t)k * 9;
  const double* c1 = c_new + (size_t)k * 3;
#pragma unroll
  for (int c = 0; c < 9; ++c) row[c] = r1[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) row[9 + c] = c1[c];
  const double d0 = c1[0] - c1[-3], d1 = c1[1] - c1[-2], d2 = c1[2] - c1[-1];
  const double len = sqrt(dot3(d0, d1, d2, d0, d1, d2));
  if (isfinite(len) && len > PNP_SCALE_FRACTION * row[12]) row[12] = len;
  row[14] = (double)((int)row[14] | LOOP_FLAG_LOOP);
  if (k == f) {
    const double nf = st[0];
    const int count = (nf >= 0.0 && nf < 2147483647.0) ? (int)nf : 0;
    if (count == f + 1 && count < capacity) {
      st[1] = row[12];
#pragma unroll
      for (int c = 0; c < 9; ++c) st[2 + c] = r1[c];
#pragma unroll
      for (int i = 0; i < 3; ++i) st[11 + i] = -dot3(r1[3 * i], r1[3 * i + 1], r1[3 * i + 2], c1[0], c1[1], c1[2]);
    }
  }
}

}  // namespace sspk
