// Landmarks from tracks: one point in the world frame per track row, from the row's observations in the
// retained frames and the cameras of the trajectory (section 24).  The rules are restated in numpy by tests/landmarks_ref.py;
// everything here is fp64 with contraction off, in the parenthesisation of that file.
//   map_window_kernel          one workgroup: the cameras of the L retained frames from the pose state, the trajectory table and
//                              the intrinsics; a view is valid inside the newest consistent window only
//   triangulate_tracks_kernel  a track row per thread, 256 rows per workgroup.  The ids tile [256][L] is staged with coalesced
//                              loads into LDS at an odd row pitch, the camera records beside it.  Pass 1 gathers each view's
//                              pixel, turns it into a unit ray, keeps the ray in LDS (three planes [L][256]: the parallax needs
//                              every PAIR of rays) and adds the midpoint system; then the pairs, the closed-form solve, four
//                              Gauss-Newton steps and the residual pass, each of which gathers the pixels again (16 B per view,
//                              L2-resident) instead of holding a per-view private array.  The loop over the views is uniform
//                              across the wavefront: the camera read is an LDS broadcast.
//   landmark_count_kernel /    the stable compaction of the status-0 rows: the ballot / popcount / block-sum pattern of
//   landmark_scatter_kernel    track_kernels.hip.h (block_scan_flag, block_base), so the order is the table's and does not
//                              depend on the order the blocks run in
// Needs: geom_blocks.hip.h, track_kernels.hip.h (TRACK_BLOCK), pose_kernels.hip.h (POSE_ROW_WORDS, POSE_THREADS).
#pragma once

namespace sspk {

#define LM_THREADS 256
#define LM_CAM_WORDS 20        // Rw [9], C [3], fx, fy, cx, cy (project's camera record), valid, 3 spare
#define LM_WORDS 8             // track id, X, Y, Z, n_views, rms, cos_parallax, index of the point in the newest frame (-1)
#define LM_GN_STEPS 4
#define LM_DET_EPS 1e-12
#define LM_STATUS_FEW_VIEWS 1
#define LM_STATUS_DEGENERATE 2
#define LM_STATUS_BEHIND 3
#define LM_STATUS_REPROJ 4
static_assert(LM_THREADS == POSE_THREADS, "one workgroup size for the fp64 geometry kernels");

// ids tile at an odd pitch (lane r reads word r * pitch + c: odd pitch, distinct banks), the rays, the cameras, the counts
__host__ __device__ inline int lm_ids_pitch(int L) { return L | 1; }
__host__ __device__ inline size_t lm_lds_bytes(int L) {
  return (size_t)3 * L * LM_THREADS * sizeof(double) + (size_t)L * LM_CAM_WORDS * sizeof(double) +
         (size_t)LM_THREADS * lm_ids_pitch(L) * sizeof(int32_t) + (size_t)2 * L * sizeof(int32_t);
}

// state [POSE_STATE_WORDS], table [capacity][POSE_ROW_WORDS], intr [n_intr][4] (n_intr = 1 or L), cams [L][LM_CAM_WORDS].
// n_frames_host >= 0 replaces the state's frame count (which stops at `capacity`: a caller that counts its frames knows better).
__global__ __launch_bounds__(64) void map_window_kernel(const double* __restrict__ state, const double* __restrict__ table, int capacity,
                                                        const double* __restrict__ intr, int n_intr, int L, int n_frames_host,
                                                        double* __restrict__ cams) {
  const int c = threadIdx.x;
  if (c >= L) return;
  const double nf = state[0];
  const int n = n_frames_host >= 0 ? n_frames_host : (nf >= 0.0 && nf < 2147483647.0 ? (int)nf : 0);
  // the newest consistent window: w goes down while row w took a pose (bit 0 clear) and row w + 1 chained its scale (bit 1 clear);
  // a row the table does not hold counts as carrying both bits.  Nothing below n - L is retained, so the walk stops there.
  const int lowest = max(n - L, 0);
  int w = n - 1;
  while (w > lowest) {
    const int fw = (w >= 0 && w < capacity) ? (int)table[(size_t)w * POSE_ROW_WORDS + 14] : 3;
    const int fn = w + 1 <= n - 1 ? ((w + 1 < capacity) ? (int)table[(size_t)(w + 1) * POSE_ROW_WORDS + 14] : 3) : 0;
    if ((fw & 1) || (fn & 2)) break;
    --w;
  }
  const int f = n - L + c;
  const double* k = intr + (size_t)(n_intr == 1 ? 0 : c) * 4;
  const double fx = k[0], fy = k[1];
  const bool valid = f >= 0 && f < capacity && f >= w && isfinite(fx) && isfinite(fy) && fx > 0.0 && fy > 0.0;
  double* o = cams + (size_t)c * LM_CAM_WORDS;
  if (valid) {
    const double* row = table + (size_t)f * POSE_ROW_WORDS;
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = row[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[12 + j] = k[j];
    o[16] = 1.0;
  } else {
#pragma unroll
    for (int j = 0; j < 17; ++j) o[j] = 0.0;
  }
  o[17] = o[18] = o[19] = 0.0;
}

// grid (cdiv(row_cap, 256)), 256 threads, dynamic LDS lm_lds_bytes(L).  ids [row_cap][L], state [2 + L], pts [L][point_cap][2] (a
// ring: retained frame c in slot (first_slot + c) % L), cams [L][LM_CAM_WORDS].  Per row < n_rows: x_out [3], n_views_out, rms_out,
// cos_out, status_out.
__global__ __launch_bounds__(LM_THREADS) void triangulate_tracks_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ state,
                                                                        const double* __restrict__ pts, int first_slot,
                                                                        const double* __restrict__ cams, int L, int point_cap,
                                                                        int row_cap, int min_views, double cos_min_parallax,
                                                                        double max_reproj, double* __restrict__ x_out,
                                                                        int32_t* __restrict__ n_views_out, double* __restrict__ rms_out,
                                                                        double* __restrict__ cos_out, int32_t* __restrict__ status_out) {
#pragma clang fp contract(off)
  extern __shared__ double lm_dyn[];
  const int tid = threadIdx.x, pitch = lm_ids_pitch(L);
  double* s_ray = lm_dyn;                                   // [3][L][256]
  double* s_cam = s_ray + (size_t)3 * L * LM_THREADS;       // [L][LM_CAM_WORDS]
  int32_t* s_ids = reinterpret_cast<int32_t*>(s_cam + (size_t)L * LM_CAM_WORDS);   // [256][pitch]
  int32_t* s_first = s_ids + (size_t)LM_THREADS * pitch;    // [L] id of point 0 of retained frame c
  int32_t* s_cnt = s_first + L;                             // [L] its point count, clamped
  const int row0 = blockIdx.x * LM_THREADS;
  const int n_rows = min(max(state[0], 0), row_cap);
  // the tile is one contiguous run of ids: consecutive lanes load consecutive words
  const int tile = min(LM_THREADS, row_cap - row0) * L;
  const int32_t* src = ids + (size_t)row0 * L;
  for (int e = tid; e < tile; e += LM_THREADS) {
    const int r = e / L;
    s_ids[r * pitch + (e - r * L)] = src[e];
  }
  for (int e = tid; e < L * LM_CAM_WORDS; e += LM_THREADS) s_cam[e] = cams[e];
  if (tid < L) {
    int first = 0;
    for (int k = 0; k < tid; ++k) first += min(max(state[2 + k], 0), point_cap);
    s_first[tid] = first;
    s_cnt[tid] = min(max(state[2 + tid], 0), point_cap);
  }
  __syncthreads();
  const int row = row0 + tid;
  if (row >= n_rows) return;                                // (no barrier follows)
  const int32_t* my = s_ids + tid * pitch;

  // pass 1: the observations, their rays and the midpoint system A = sum(I - d d^T), b = sum((I - d d^T) C)
  unsigned used = 0;
  int n_views = 0;
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  for (int c = 0; c < L; ++c) {
    const double* cam = s_cam + c * LM_CAM_WORDS;
    const int id = my[c], p = id - s_first[c];
    if (!(id >= 0 && cam[16] != 0.0 && p >= 0 && p < s_cnt[c])) continue;
    used |= 1u << c;
    ++n_views;
    const double2 px = *reinterpret_cast<const double2*>(pts + ((size_t)((first_slot + c) % L) * point_cap + p) * 2);
    const double x0 = (px.x - cam[14]) / cam[12], x1 = (px.y - cam[15]) / cam[13];
    const double e0 = dot3(cam[0], cam[3], cam[6], x0, x1, 1.0), e1 = dot3(cam[1], cam[4], cam[7], x0, x1, 1.0);
    const double e2 = dot3(cam[2], cam[5], cam[8], x0, x1, 1.0);
    const double nrm = sqrt(dot3(e0, e1, e2, e0, e1, e2));
    const double d0 = e0 / nrm, d1 = e1 / nrm, d2 = e2 / nrm;
    s_ray[(0 * L + c) * LM_THREADS + tid] = d0;
    s_ray[(1 * L + c) * LM_THREADS + tid] = d1;
    s_ray[(2 * L + c) * LM_THREADS + tid] = d2;
    const double m00 = 1.0 - d0 * d0, m11 = 1.0 - d1 * d1, m22 = 1.0 - d2 * d2;
    const double m01 = 0.0 - d0 * d1, m02 = 0.0 - d0 * d2, m12 = 0.0 - d1 * d2;
    a00 = a00 + m00;
    a01 = a01 + m01;
    a02 = a02 + m02;
    a11 = a11 + m11;
    a12 = a12 + m12;
    a22 = a22 + m22;
    b0 = b0 + dot3(m00, m01, m02, cam[9], cam[10], cam[11]);
    b1 = b1 + dot3(m01, m11, m12, cam[9], cam[10], cam[11]);
    b2 = b2 + dot3(m02, m12, m22, cam[9], cam[10], cam[11]);
  }
  n_views_out[row] = n_views;
  double* xo = x_out + (size_t)row * 3;
  if (n_views < min_views) {
    status_out[row] = LM_STATUS_FEW_VIEWS;
    xo[0] = xo[1] = xo[2] = 0.0;
    rms_out[row] = 0.0;
    cos_out[row] = 0.0;
    return;
  }

  // parallax: the smallest d_i . d_j over the pairs of used views (each thread reads its own column of the planes)
  double cosp = __longlong_as_double(0x7ff0000000000000ll);
  for (int i = 0; i + 1 < L; ++i) {
    if (!((used >> i) & 1u)) continue;
    const double p0 = s_ray[(0 * L + i) * LM_THREADS + tid], p1 = s_ray[(1 * L + i) * LM_THREADS + tid];
    const double p2 = s_ray[(2 * L + i) * LM_THREADS + tid];
    for (int j = i + 1; j < L; ++j) {
      if (!((used >> j) & 1u)) continue;
      const double v = dot3(p0, p1, p2, s_ray[(0 * L + j) * LM_THREADS + tid], s_ray[(1 * L + j) * LM_THREADS + tid],
                                s_ray[(2 * L + j) * LM_THREADS + tid]);
      cosp = v < cosp ? v : cosp;
    }
  }
  bool degenerate = cosp > cos_min_parallax;

  // the midpoint, its cheirality
  double X0, X1, X2;
  degenerate |= !cof3_solve(cofactors3(a00, a01, a02, a11, a12, a22), LM_DET_EPS, b0, b1, b2, X0, X1, X2);
  bool behind = false;
  for (int c = 0; c < L; ++c) {
    if (!((used >> c) & 1u)) continue;
    const double* cam = s_cam + c * LM_CAM_WORDS;
    const double z = dot3(cam[6], cam[7], cam[8], X0 - cam[9], X1 - cam[10], X2 - cam[11]);
    behind |= !(isfinite(z) && z > 0.0);
  }

  // Gauss-Newton on the pixel reprojection error: a fixed number of steps, H = sum(J^T J), g = sum(J^T r), X <- X - H^-1 g
  for (int step = 0; step < LM_GN_STEPS; ++step) {
    double h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int c = 0; c < L; ++c) {
      if (!((used >> c) & 1u)) continue;
      const double* cam = s_cam + c * LM_CAM_WORDS;
      const double2 px = *reinterpret_cast<const double2*>(pts + ((size_t)((first_slot + c) % L) * point_cap + (my[c] - s_first[c])) * 2);
      const View w = project(cam, X0, X1, X2, px.x, px.y);
      const double fa = cam[12] / w.y2, fb = cam[13] / w.y2;
      const double j00 = fa * (cam[0] - w.u * cam[6]), j01 = fa * (cam[1] - w.u * cam[7]), j02 = fa * (cam[2] - w.u * cam[8]);
      const double j10 = fb * (cam[3] - w.v * cam[6]), j11 = fb * (cam[4] - w.v * cam[7]), j12 = fb * (cam[5] - w.v * cam[8]);
      h00 = h00 + (j00 * j00 + j10 * j10);
      h01 = h01 + (j00 * j01 + j10 * j11);
      h02 = h02 + (j00 * j02 + j10 * j12);
      h11 = h11 + (j01 * j01 + j11 * j11);
      h12 = h12 + (j01 * j02 + j11 * j12);
      h22 = h22 + (j02 * j02 + j12 * j12);
      g0 = g0 + (j00 * w.r0 + j10 * w.r1);
      g1 = g1 + (j01 * w.r0 + j11 * w.r1);
      g2 = g2 + (j02 * w.r0 + j12 * w.r1);
    }
    double s0, s1, s2;
    degenerate |= !cof3_solve(cofactors3(h00, h01, h02, h11, h12, h22), LM_DET_EPS, g0, g1, g2, s0, s1, s2);
    X0 = X0 - s0;
    X1 = X1 - s1;
    X2 = X2 - s2;
  }

  // the residuals and the cheirality of the result
  double ss = 0.0;
  for (int c = 0; c < L; ++c) {
    if (!((used >> c) & 1u)) continue;
    const double* cam = s_cam + c * LM_CAM_WORDS;
    const double2 px = *reinterpret_cast<const double2*>(pts + ((size_t)((first_slot + c) % L) * point_cap + (my[c] - s_first[c])) * 2);
    const View w = project(cam, X0, X1, X2, px.x, px.y);
    behind |= !(isfinite(w.y2) && w.y2 > 0.0);
    ss = ss + (w.r0 * w.r0 + w.r1 * w.r1);
  }
  const double rms = sqrt(ss / (2.0 * (double)n_views));
  const bool x_ok = isfinite(X0) && isfinite(X1) && isfinite(X2);
  status_out[row] = degenerate ? LM_STATUS_DEGENERATE : (behind ? LM_STATUS_BEHIND : (rms > max_reproj ? LM_STATUS_REPROJ : 0));
  xo[0] = x_ok ? X0 : 0.0;
  xo[1] = x_ok ? X1 : 0.0;
  xo[2] = x_ok ? X2 : 0.0;
  rms_out[row] = isfinite(rms) ? rms : 0.0;
  cos_out[row] = isfinite(cosp) ? cosp : 0.0;
}

__device__ __forceinline__ bool landmark_keep(const int32_t* __restrict__ state, const int32_t* __restrict__ status, int row_cap) {
  const int r = blockIdx.x * TRACK_BLOCK + threadIdx.x;
  return r < min(max(state[0], 0), row_cap) && status[r] == 0;
}

__global__ __launch_bounds__(TRACK_BLOCK) void landmark_count_kernel(const int32_t* __restrict__ state, const int32_t* __restrict__ status,
                                                                     int row_cap, int32_t* __restrict__ block_sums) {
  __shared__ int wsum[TRACK_BLOCK / 64];
  int total;
  block_scan_flag<TRACK_BLOCK>(landmark_keep(state, status, row_cap), wsum, total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// out [row_cap][LM_WORDS], n_out [1]
__global__ __launch_bounds__(TRACK_BLOCK) void landmark_scatter_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ tid,
                                                                       const int32_t* __restrict__ state, const int32_t* __restrict__ status,
                                                                       const double* __restrict__ x, const int32_t* __restrict__ n_views,
                                                                       const double* __restrict__ rms, const double* __restrict__ cosp,
                                                                       const int32_t* __restrict__ block_sums, int L, int point_cap,
                                                                       int row_cap, double* __restrict__ out, int32_t* __restrict__ n_out) {
  __shared__ int wsum[TRACK_BLOCK / 64];
  __shared__ int red[TRACK_BLOCK / 64];
  const int r = blockIdx.x * TRACK_BLOCK + threadIdx.x;
  const int base = block_base<TRACK_BLOCK>(block_sums, blockIdx.x, red);
  const bool keep = landmark_keep(state, status, row_cap);
  int total;
  const int pos = base + block_scan_flag<TRACK_BLOCK>(keep, wsum, total);
  if (keep) {
    int first = 0;
    for (int c = 0; c < L - 1; ++c) first += min(max(state[2 + c], 0), point_cap);
    const int id = ids[(size_t)r * L + L - 1], p = id - first;
    double* o = out + (size_t)pos * LM_WORDS;
    o[0] = (double)tid[r];
    o[1] = x[(size_t)r * 3];
    o[2] = x[(size_t)r * 3 + 1];
    o[3] = x[(size_t)r * 3 + 2];
    o[4] = (double)n_views[r];
    o[5] = rms[r];
    o[6] = cosp[r];
    o[7] = (id >= 0 && p >= 0 && p < min(max(state[2 + L - 1], 0), point_cap)) ? (double)p : -1.0;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) n_out[0] = base + total;
}

}  // namespace sspk
