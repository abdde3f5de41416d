// Point tracks over a frame sequence (PointTracker.update / get_tracks of the reference, models/model_wrap.py:521-615;
// the rules are restated in DESIGN.md section 17).  The table lives in three device arrays of `row_cap` rows:
//   ids [row][L] int32 (point id of frame 0 .. L-1, -1 = none), tid [row] int32 (track id), score [row] fp64 (mean
//   descriptor distance, 9999 = no match yet), and a state vector int32 [2 + L] = n_rows, track_count, point count of
//   the L retained frames (oldest first).  Every count a kernel reads from the device is clamped to its capacity first.
//
// One update is four launches over host-known capacities (no O(matches x rows) search, no host synchronisation):
//   track_shift_kernel     drop the oldest id column, subtract its frame's point count, append -1; scatter
//                          row_of_point[] for the previous frame's column (its ids are dense in one interval)
//   track_match_kernel     one lookup per match: last id, matched flag, the fp64 running mean (contraction off)
//   track_count_kernel     keep flags of the virtual sequence (old rows, then one new row per point) counted per
//                          1024-element block: wave64 ballots + popcounts, no LDS traffic beyond 16 wave totals
//   track_scatter_kernel   every block sums the block counts before it (<= TRACK_MAX_BLOCKS of them), repeats its
//                          ballots and writes the surviving rows in order: a STABLE compaction across workgroups whose
//                          result does not depend on the order the blocks run in.  The last block writes the state.
// get_tracks is the same count / scatter pair with another predicate; it writes the public fp64 [M][2+L] matrix.
// The in-block scan and the sum of the earlier blocks are block_scan_flag and block_base of geom_blocks.hip.h.
// Needs: geom_blocks.hip.h.
#pragma once

namespace sspk {

#define TRACK_BLOCK 1024
#define TRACK_NO_SCORE 9999.0

struct TrackCounts {  // clamped view of a state vector
  int n_rows, track_count, remove_size, n_prev, off2, off1;
};

// state [2 + L]; cnt[c] = points of retained frame c BEFORE the update (frame 0 is the one the update drops).
// off2 / off1: the reference's offsets[-2] / offsets[-1] after the drop = first id of the previous / the new frame.
__device__ __forceinline__ TrackCounts track_counts(const int32_t* __restrict__ state, int L, int point_cap, int row_cap) {
  TrackCounts t;
  t.n_rows = min(max(state[0], 0), row_cap);
  t.track_count = state[1];
  t.remove_size = min(max(state[2], 0), point_cap);
  int s = 0;
  for (int c = 1; c < L - 1; ++c) s += min(max(state[2 + c], 0), point_cap);
  t.off2 = s;
  t.n_prev = min(max(state[2 + L - 1], 0), point_cap);
  t.off1 = s + t.n_prev;
  return t;
}

__global__ __launch_bounds__(256) void track_shift_kernel(const int32_t* __restrict__ ids_in, const double* __restrict__ score_in,
                                                          const int32_t* __restrict__ state_in, int L, int point_cap, int row_cap,
                                                          int32_t* __restrict__ ids_tmp, double* __restrict__ score_tmp,
                                                          int32_t* __restrict__ row_of_point) {
  const TrackCounts t = track_counts(state_in, L, point_cap, row_cap);
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= t.n_rows) return;
  const int32_t* src = ids_in + (size_t)r * L;
  int32_t* dst = ids_tmp + (size_t)r * L;
  int v = -1;
  for (int c = 0; c < L - 1; ++c) {
    v = src[c + 1] - t.remove_size;
    if (v < -1) v = -1;
    dst[c] = v;
  }
  dst[L - 1] = -1;
  score_tmp[r] = score_in[r];
  const int k = v - t.off2;  // v: the previous frame's column
  if (v >= 0 && k >= 0 && k < t.n_prev) row_of_point[k] = r;
}

// match: [.][3] float rows (i, j, distance) as ssp_match_two_way writes them; score64 (may be null): fp64 distances that
// replace column 2.  Mutual matches: no two matches share i or j, so no two threads touch one row.
__global__ __launch_bounds__(256) void track_match_kernel(const float* __restrict__ match, const double* __restrict__ score64,
                                                          const int32_t* __restrict__ n_match, const int32_t* __restrict__ n_points,
                                                          const int32_t* __restrict__ state_in, int L, int point_cap, int row_cap,
                                                          const int32_t* __restrict__ row_of_point, int32_t* __restrict__ ids_tmp,
                                                          double* __restrict__ score_tmp, int32_t* __restrict__ matched) {
#pragma clang fp contract(off)
  const TrackCounts t = track_counts(state_in, L, point_cap, row_cap);
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= min(max(n_match[0], 0), point_cap)) return;
  const int n_new = min(max(n_points[0], 0), point_cap);
  const int i = (int)match[(size_t)m * 3], j = (int)match[(size_t)m * 3 + 1];
  if (i < 0 || i >= t.n_prev || j < 0 || j >= n_new) return;
  const int row = row_of_point[i];
  if (row < 0 || row >= t.n_rows) return;
  const double s = score64 ? score64[m] : (double)match[(size_t)m * 3 + 2];
  int32_t* ids = ids_tmp + (size_t)row * L;
  ids[L - 1] = j + t.off1;
  matched[j] = 1;
  int present = 1;  // the id just written
  for (int c = 0; c < L - 1; ++c) present += ids[c] != -1;
  const double old = score_tmp[row];
  if (old == TRACK_NO_SCORE) {
    score_tmp[row] = s;
  } else {
    const double frac = 1.0 / ((double)present - 1.0);
    score_tmp[row] = (1.0 - frac) * old + frac * s;
  }
}

// update prunes rows without an id >= 0 (get_tracks counts ids != -1: the reference's asymmetry, kept)
__device__ __forceinline__ bool track_row_alive(const int32_t* __restrict__ ids, int L) {
  bool any = false;
  for (int c = 0; c < L; ++c) any |= ids[c] >= 0;
  return any;
}

// get_tracks(min_length): at least min_length ids != -1 and a last id != -1; min_length == 0: every row.
__device__ __forceinline__ bool track_row_selected(const int32_t* __restrict__ ids, int L, int min_length) {
  if (min_length == 0) return true;
  int n = 0;
  for (int c = 0; c < L; ++c) n += ids[c] != -1;
  return n >= min_length && ids[L - 1] != -1;
}

// Blocks [0, nb_old) cover the old rows, blocks [nb_old, nb_old + nb_new) the points of the new frame.
__device__ __forceinline__ bool track_update_flag(int b, int nb_old, int n_rows, int n_new, const int32_t* __restrict__ ids_tmp,
                                                  const int32_t* __restrict__ matched, int L) {
  if (b < nb_old) {
    const int r = b * TRACK_BLOCK + threadIdx.x;
    return r < n_rows && track_row_alive(ids_tmp + (size_t)r * L, L);
  }
  const int j = (b - nb_old) * TRACK_BLOCK + threadIdx.x;
  return j < n_new && !matched[j];
}

__global__ __launch_bounds__(TRACK_BLOCK) void track_count_kernel(const int32_t* __restrict__ ids_tmp, const int32_t* __restrict__ matched,
                                                                  const int32_t* __restrict__ state_in,
                                                                  const int32_t* __restrict__ n_points, int L, int point_cap,
                                                                  int row_cap, int nb_old, int32_t* __restrict__ block_sums) {
  __shared__ int wsum[TRACK_BLOCK / 64];
  const int n_rows = min(max(state_in[0], 0), row_cap), n_new = min(max(n_points[0], 0), point_cap);
  int total;
  block_scan_flag<TRACK_BLOCK>(track_update_flag(blockIdx.x, nb_old, n_rows, n_new, ids_tmp, matched, L), wsum, total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(TRACK_BLOCK) void track_scatter_kernel(const int32_t* __restrict__ ids_tmp, const double* __restrict__ score_tmp,
                                                                    const int32_t* __restrict__ tid_in, const int32_t* __restrict__ matched,
                                                                    const int32_t* __restrict__ state_in,
                                                                    const int32_t* __restrict__ n_points,
                                                                    const int32_t* __restrict__ block_sums, int L, int point_cap,
                                                                    int row_cap, int nb_old, int32_t* __restrict__ ids_out,
                                                                    int32_t* __restrict__ tid_out, double* __restrict__ score_out,
                                                                    int32_t* __restrict__ state_out) {
  __shared__ int wsum[TRACK_BLOCK / 64];
  __shared__ int red[TRACK_BLOCK / 64];
  const TrackCounts t = track_counts(state_in, L, point_cap, row_cap);
  const int n_new = min(max(n_points[0], 0), point_cap);
  const int b = blockIdx.x, nb = gridDim.x;
  const int base = block_base<TRACK_BLOCK>(block_sums, b, red);
  const int kept_old = b < nb_old ? 0 : block_base<TRACK_BLOCK>(block_sums, nb_old, red);  // (uniform per block)
  const bool keep = track_update_flag(b, nb_old, t.n_rows, n_new, ids_tmp, matched, L);
  int total;
  const int pos = base + block_scan_flag<TRACK_BLOCK>(keep, wsum, total);
  if (keep && pos < row_cap) {
    int32_t* dst = ids_out + (size_t)pos * L;
    if (b < nb_old) {
      const int r = b * TRACK_BLOCK + threadIdx.x;
      const int32_t* src = ids_tmp + (size_t)r * L;
      for (int c = 0; c < L; ++c) dst[c] = src[c];
      tid_out[pos] = tid_in[r];
      score_out[pos] = score_tmp[r];
    } else {
      const int j = (b - nb_old) * TRACK_BLOCK + threadIdx.x;
      for (int c = 0; c < L - 1; ++c) dst[c] = -1;
      dst[L - 1] = j + t.off1;
      tid_out[pos] = t.track_count + (pos - kept_old);
      score_out[pos] = TRACK_NO_SCORE;
    }
  }
  if (b == nb - 1 && threadIdx.x == 0) {
    const int rows = base + total;
    state_out[0] = min(rows, row_cap);
    state_out[1] = t.track_count + (rows - kept_old);
    for (int c = 0; c < L - 1; ++c) state_out[2 + c] = min(max(state_in[3 + c], 0), point_cap);
    state_out[2 + L - 1] = n_new;
  }
}

__global__ __launch_bounds__(TRACK_BLOCK) void track_select_count_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ state,
                                                                         int L, int row_cap, int min_length,
                                                                         int32_t* __restrict__ block_sums) {
  __shared__ int wsum[TRACK_BLOCK / 64];
  const int n_rows = min(max(state[0], 0), row_cap);
  const int r = blockIdx.x * TRACK_BLOCK + threadIdx.x;
  int total;
  block_scan_flag<TRACK_BLOCK>(r < n_rows && track_row_selected(ids + (size_t)r * L, L, min_length), wsum, total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// out [row_cap][2 + L] fp64 rows (track id, score, ids), n_out [1]
__global__ __launch_bounds__(TRACK_BLOCK) void track_select_scatter_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ tid,
                                                                           const double* __restrict__ score,
                                                                           const int32_t* __restrict__ state,
                                                                           const int32_t* __restrict__ block_sums, int L, int row_cap,
                                                                           int min_length, double* __restrict__ out,
                                                                           int32_t* __restrict__ n_out) {
  __shared__ int wsum[TRACK_BLOCK / 64];
  __shared__ int red[TRACK_BLOCK / 64];
  const int n_rows = min(max(state[0], 0), row_cap);
  const int r = blockIdx.x * TRACK_BLOCK + threadIdx.x;
  const int base = block_base<TRACK_BLOCK>(block_sums, blockIdx.x, red);
  const bool keep = r < n_rows && track_row_selected(ids + (size_t)r * L, L, min_length);
  int total;
  const int pos = base + block_scan_flag<TRACK_BLOCK>(keep, wsum, total);
  if (keep) {
    double* o = out + (size_t)pos * (2 + L);
    o[0] = (double)tid[r];
    o[1] = score[r];
    for (int c = 0; c < L; ++c) o[2 + c] = (double)ids[(size_t)r * L + c];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) n_out[0] = base + total;
}

// Coordinates of the points a tracks matrix names (the index arithmetic of draw_tracks, models/model_wrap.py:624-641).
// tracks [track_cap][2 + L] fp64 with n_tracks[0] rows; pts [L][point_cap][2] fp64, a ring: retained frame c (0 = oldest)
// lives in slot (first_slot + c) % L; state: the tracker's state vector (frame counts).  xy [track_cap][L][2]: NaN where
// the id is -1 or does not name a point of its frame.
__global__ __launch_bounds__(256) void track_points_kernel(const double* __restrict__ tracks, const int32_t* __restrict__ n_tracks,
                                                           const double* __restrict__ pts, const int32_t* __restrict__ state,
                                                           int L, int point_cap, int track_cap, int first_slot,
                                                           double* __restrict__ xy) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int m = e / L, c = e - m * L;
  if (m >= min(max(n_tracks[0], 0), track_cap)) return;
  int off = 0;
  for (int k = 0; k < c; ++k) off += min(max(state[2 + k], 0), point_cap);
  const int cnt = min(max(state[2 + c], 0), point_cap);
  const double idv = tracks[(size_t)m * (2 + L) + 2 + c];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double x = nan, y = nan;
  if (idv >= 0.0 && idv < 2147483647.0) {
    const int k = (int)idv - off;
    if (k >= 0 && k < cnt) {
      const double* p = pts + ((size_t)((first_slot + c) % L) * point_cap + k) * 2;
      x = p[0];
      y = p[1];
    }
  }
  xy[(size_t)e * 2] = x;
  xy[(size_t)e * 2 + 1] = y;
}

}  // namespace sspk
