// World map: landmarks that outlive their window, a matcher of one frame's descriptors against the whole
// map, the join of its matches with the map's points, and the repair of a trajectory row from the pose found against the map.  The
// rules are restated in numpy by tests/world_ref.py.
//   world_match_kernel     a workgroup of 4 waves owns a strip of 128 map rows.  Wave w keeps its 32 rows' MFMA operands in
//                          registers (lane (r, h): the float4 at 8s + 4h of row r, s = 0..31: 128 registers), read from HBM once.
//                          The frame's rows are swept in tiles of 32, staged through LDS (two buffers; rows padded to 65 float4, so
//                          the ds_read_b128 of 16 rows at one k is conflict-free), each tile read from L2 once per workgroup.  The dot
//                          product is match_dist_kernel's chain: for s, MFMA 32x32x2 on components x, y, z, w, i.e. k = 8s + c and
//                          k = 8s + 4 + c for c = 0..3; a distance depends on its two rows only, and the keys equal that kernel's.
//                          Row minima stay in registers over the sweep and leave by one plain store per map row (one atomicMin
//                          when a small map's sweep is split over several workgroups, decided on the device).  Column minima
//                          cross strips by the 64-bit atomicMin of match_dist_kernel (a minimum of unique keys has no order to
//                          depend on), issued only when the key is below the value already there: a stale read only costs an atomic.
//                          CLASSES (ssp_match_world_classes): a pair (i, j) is a candidate iff the class voted
//                          for map row i's track equals the frame row's, is known, and is kept by the mask; any other pair takes
//                          part in neither arg-min.  The strip's 128 class codes (one byte each, WORLD_CLASS_NONE = never a candidate)
//                          and every tile's 32 frame codes (an unknown frame class becomes 256, which no byte equals) go through
//                          LDS beside the tile; the epilogue reads 4 + 1 words of them.  CLASSES = false reads none of it.
//   world_compact_kernel   one workgroup: thread t owns the map rows [t c, (t + 1) c), c = ceil(n_rows / 1024); count, scan, write:
//                          the mutual matches below the threshold in ascending map row
//   world_anchor_kernel    one thread: the anchor rule (section 29) from the newest trajectory row's flags and the map's state; the
//                          later launches of the call only read what it leaves in the workspace header
//   world_classify_kernel  a thread per landmark row: skipped, found in the map (its slot) or new; counts per block of 1024
//   world_scatter_kernel   the same blocks: a new row's slot = rows before the call + new rows of the earlier blocks + its rank in
//                          the block (stable, independent of block order), the scalar columns, then a wave per row for the 1 KB
//                          descriptor copy; block 0 writes the map's counters
//   world_corr_kernel      one workgroup: a correspondence row (X, Y, Z, px, py, map row, valid, 0) per match row
//   world_repair_kernel    one thread: section 27's repair with the world's firing condition, the streak of repaired frames
// Needs: geom_blocks.hip.h, describe_kernels.hip.h (min_u64, shfl_xor_u64), pose_kernels.hip.h (POSE_ROW_WORDS),
// landmark_kernels.hip.h (LM_WORDS), pnp_kernels.hip.h (the correspondence rows, pnp_load_pose, pnp_rewrite_row).
#pragma once

namespace sspk {

#define WORLD_STATE_WORDS 8     // n_rows, anchored, lost_frames, streak, dropped (full), dropped (tid), appended, updated
#define WORLD_MAX_ROWS 65536
#define WORLD_STRIP 128         // map rows per workgroup of the matcher
#define WORLD_TILE 32           // frame rows per staged tile
#define WORLD_LDS_ROW 65        // float4 per staged row: 64 + 1 of padding
#define WORLD_SPLIT_MAX 16      // workgroups that may share one strip's sweep (grid.y)
#define WORLD_TARGET_GROUPS 512 // two workgroups per CU: a small map splits its sweep until it has that many
#define WORLD_BLOCK 1024
#define WORLD_MAX_BLOCKS 64     // landmark rows / WORLD_BLOCK
#define WORLD_HDR_WORDS 4       // workspace header: rows before the call, anchored, 2 spare
#define WORLD_FLAG_WORLD 16
#define WORLD_CLS_SKIP (-2)
#define WORLD_CLS_NEW (-1)

#define WORLD_CLASS_NONE 255

typedef float world_floatx16 __attribute__((ext_vector_type(16)));

// the class arguments of world_match_kernel<true> (section 42; the votes are kept by world_class_kernels.hip.h)
struct WorldClasses {
  const int32_t* map_tid;   // [map_cap]: the track id of every map slot
  const uint16_t* votes;    // [tid_cap]
  const uint8_t* cls2;      // [cap]: the class of every frame row
  int tid_cap;
  uint32_t keep[8];         // bit c of word c / 32: map rows of class c take part
};

__device__ __forceinline__ int world_class_decode(uint32_t v) { return (v >> 8) ? (int)(v & 255u) : WORLD_CLASS_NONE; }

// the decoded class of track t; an id outside [0, tid_cap) has none
__device__ __forceinline__ int world_class_of(const uint16_t* __restrict__ votes, int t, int tid_cap) {
  return (t >= 0 && t < tid_cap) ? world_class_decode(votes[t]) : WORLD_CLASS_NONE;
}

template <bool CLASSES>
__global__ __launch_bounds__(256, 2) void world_match_kernel(const float* __restrict__ map_desc, const int32_t* __restrict__ world_state,
                                                          int map_cap, const float* __restrict__ d2, const int32_t* __restrict__ count2,
                                                          int cap, uint64_t* __restrict__ rowmin, uint64_t* __restrict__ colmin,
                                                          const WorldClasses wc) {
  __shared__ float4 tile[2][WORLD_TILE * WORLD_LDS_ROW];
  __shared__ uint32_t strip_cls[CLASSES ? WORLD_STRIP / 4 : 1];   // byte k: the class code of map row strip0 + k
  __shared__ int tile_cls[2][CLASSES ? WORLD_TILE : 1];           // the class code of the staged tile's frame rows
  const int n1 = min(max(world_state[0], 0), map_cap), n2 = min(max(count2[0], 0), cap);
  const int strip0 = blockIdx.x * WORLD_STRIP;
  if (strip0 >= n1 || n2 <= 0) return;   // (the whole workgroup: no barrier is left waiting)
  // a map of few strips would leave most CUs idle: its strips' sweeps are split over `split` workgroups (tile y, y + split, ...),
  // decided from the device counts alone.  The minima are of unique keys, so the result does not depend on the split.
  const int n_tiles = (n2 + WORLD_TILE - 1) / WORLD_TILE;
  const int live_strips = (n1 + WORLD_STRIP - 1) / WORLD_STRIP;
  const int split = min(min(WORLD_SPLIT_MAX, n_tiles), max(1, WORLD_TARGET_GROUPS / live_strips));
  const int y = blockIdx.y;
  if (y >= split) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wi = strip0 + wave * 32;
  const bool live = wi < n1;   // a wave past the last row still stages tiles and meets the barriers
  float4 a[32];
  {
    const float4* A = reinterpret_cast<const float4*>(map_desc + (size_t)min(wi + r, n1 - 1) * 256) + h;
#pragma unroll
    for (int s = 0; s < 32; ++s) a[s] = A[2 * s];
  }
  uint64_t kr[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) kr[t] = ~0ull;
  // staging: float4 q * 256 + tid of the tile = row 4q + wave, float4 `lane` of it
#pragma unroll
  for (int q = 0; q < 8; ++q)
    tile[0][(4 * q + wave) * WORLD_LDS_ROW + lane] =
        reinterpret_cast<const float4*>(d2 + (size_t)min(y * WORLD_TILE + 4 * q + wave, n2 - 1) * 256)[lane];
  if (CLASSES) {
    // the classes are loaded under the descriptors' clamp: a copy of row n1 - 1 (n2 - 1) is a candidate exactly where that row is
    if (tid < WORLD_STRIP) {
      const int c = world_class_of(wc.votes, wc.map_tid[min(strip0 + tid, n1 - 1)], wc.tid_cap);
      const bool kept = c != WORLD_CLASS_NONE && ((wc.keep[c >> 5] >> (c & 31)) & 1u);
      reinterpret_cast<uint8_t*>(strip_cls)[tid] = (uint8_t)(kept ? c : WORLD_CLASS_NONE);
    }
    if (tid < WORLD_TILE) {
      const int c = wc.cls2[min(y * WORLD_TILE + tid, n2 - 1)];
      tile_cls[0][tid] = c == WORLD_CLASS_NONE ? 256 : c;
    }
  }
  __syncthreads();
  int buf = 0;
  for (int tl = y; tl < n_tiles; tl += split, buf ^= 1) {
    const int j0 = tl * WORLD_TILE;
    const bool more = tl + split < n_tiles;
    if (live) {
      const float4* B = tile[buf] + r * WORLD_LDS_ROW + h;
      world_floatx16 acc;
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[t] = 0.f;
#pragma unroll
      for (int s = 0; s < 32; ++s) {
        const float4 b = B[2 * s];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].w, b.w, acc, 0, 0, 0);
      }
      // accumulator t of lane l: map row wi + (t & 3) + 8 (t >> 2) + 4h, frame row j0 + r.  No key is masked: a row past n1 - 1 (or
      // a frame row past n2 - 1) is a copy of row n1 - 1 (n2 - 1), which lies in the same wave (tile); its key has that row's
      // distance and a larger index, so it never is a minimum, and its own minimum is never stored.
      const int j = j0 + r;
      uint64_t cbest = ~0ull;
      const int cj = CLASSES ? tile_cls[buf][r] : 0;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int i = wi + (t & 3) + 8 * (t >> 2) + 4 * h;
        const float dd = sqrtf(2.f - 2.f * fminf(fmaxf(acc[t], -1.f), 1.f));   // (the correctly rounded root: describe_kernels.hip.h)
        const uint64_t hi = (uint64_t)__float_as_uint(dd) << 32;
        if (CLASSES) {   // rows 8 (t >> 2) + 4h .. + 3 of the wave: one word, two addresses per wave
          const bool ok = (int)((strip_cls[wave * 8 + 2 * (t >> 2) + h] >> (8 * (t & 3))) & 255u) == cj;
          kr[t] = min_u64(kr[t], ok ? hi | (uint32_t)j : ~0ull);
          cbest = min_u64(cbest, ok ? hi | (uint32_t)i : ~0ull);
        } else {
          kr[t] = min_u64(kr[t], hi | (uint32_t)j);
          cbest = min_u64(cbest, hi | (uint32_t)i);
        }
      }
      cbest = min_u64(cbest, shfl_xor_u64(cbest, 32));
      if (h == 0 && j < n2) {
        unsigned long long* cm = reinterpret_cast<unsigned long long*>(colmin + j);
        if (cbest < __hip_atomic_load(cm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(cm, (unsigned long long)cbest);
      }
    }
    // the next tile goes to the other buffer, which every wave left at the previous barrier; the second workgroup of the CU
    // computes while this one waits for L2
    if (more) {
      float4 stage[8];
#pragma unroll
      for (int q = 0; q < 8; ++q)
        stage[q] = reinterpret_cast<const float4*>(d2 + (size_t)min(j0 + split * WORLD_TILE + 4 * q + wave, n2 - 1) * 256)[lane];
      if (CLASSES && tid < WORLD_TILE) {
        const int c = wc.cls2[min(j0 + split * WORLD_TILE + tid, n2 - 1)];
        tile_cls[buf ^ 1][tid] = c == WORLD_CLASS_NONE ? 256 : c;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) tile[buf ^ 1][(4 * q + wave) * WORLD_LDS_ROW + lane] = stage[q];
    }
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    uint64_t k = kr[t];
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) k = min_u64(k, shfl_xor_u64(k, o));
    const int i = wi + (t & 3) + 8 * (t >> 2) + 4 * h;
    if (r == 0 && i < n1) {
      if (split == 1)
        rowmin[i] = k;
      else
        atomicMin(reinterpret_cast<unsigned long long*>(rowmin + i), (unsigned long long)k);
    }
  }
}

__global__ __launch_bounds__(WORLD_BLOCK) void world_compact_kernel(const uint64_t* __restrict__ rowmin, const uint64_t* __restrict__ colmin,
                                                                    const int32_t* __restrict__ world_state, int map_cap,
                                                                    const int32_t* __restrict__ count2, int cap, float thresh,
                                                                    float* __restrict__ match, int32_t* __restrict__ n_match) {
  __shared__ int wsum[WORLD_BLOCK / 64];
  const int tid = threadIdx.x;
  const int n1 = min(max(world_state[0], 0), map_cap), n2 = min(max(count2[0], 0), cap);
  if (n1 <= 0 || n2 <= 0) {
    if (tid == 0) n_match[0] = 0;
    return;
  }
  const int chunk = (n1 + WORLD_BLOCK - 1) / WORLD_BLOCK;
  const int lo = min(tid * chunk, n1), hi = min(lo + chunk, n1);
  int cnt = 0;
  for (int i = lo; i < hi; ++i) {
    const uint64_t k = rowmin[i];
    const uint32_t j = (uint32_t)k;
    const float dd = __uint_as_float((uint32_t)(k >> 32));
    cnt += (dd < thresh && j < (uint32_t)n2 && (uint32_t)colmin[j] == (uint32_t)i) ? 1 : 0;
  }
  int total;
  int off = block_scan<WORLD_BLOCK>(cnt, wsum, total);
  for (int i = lo; i < hi; ++i) {
    const uint64_t k = rowmin[i];
    const uint32_t j = (uint32_t)k;
    const float dd = __uint_as_float((uint32_t)(k >> 32));
    if (dd < thresh && j < (uint32_t)n2 && (uint32_t)colmin[j] == (uint32_t)i) {   // (each frame row is mutual with one map row: off < n2)
      float* o = match + (size_t)off * 3;
      o[0] = (float)i; o[1] = (float)j; o[2] = dd;
      ++off;
    }
  }
  if (tid == 0) n_match[0] = total;
}

// ---- the store ----
// grid (1), 64 threads.  table [capacity][POSE_ROW_WORDS] of the trajectory, n_frames the caller's frame count: the newest row is
// n_frames - 1 (no such row: the frame counts as flagged).  hdr [WORLD_HDR_WORDS] = (rows before the call, anchored, 0, 0).
__global__ __launch_bounds__(64) void world_anchor_kernel(int32_t* __restrict__ state, int map_cap, const double* __restrict__ table,
                                                          int capacity, int n_frames, int patience, int32_t* __restrict__ hdr) {
  if (threadIdx.x != 0) return;
  int n_rows = min(max(state[0], 0), map_cap), lost = state[2], streak = state[3];
  const bool anchored = state[1] != 0;
  bool ok = false;
  if (n_frames >= 1 && n_frames <= capacity) {
    const double f = table[(size_t)(n_frames - 1) * POSE_ROW_WORDS + 14];
    ok = f >= 0.0 && f < 2147483647.0 && (((int)f) & 3) == 0;
  }
  const bool anch = ok && (n_rows == 0 || anchored || streak >= 2);
  if (n_rows > 0 && !anch) {
    lost += 1;
    if (lost > patience) {
      n_rows = 0;
      lost = 0;
      streak = 0;
      state[4] = 0;
      state[5] = 0;
    }
  } else {
    lost = 0;
  }
  state[0] = n_rows;
  state[1] = anch ? 1 : 0;
  state[2] = lost;
  state[3] = streak;
  state[6] = 0;
  state[7] = 0;
  hdr[0] = n_rows;
  hdr[1] = anch ? 1 : 0;
  hdr[2] = 0;
  hdr[3] = 0;
}

struct WorldRow {
  int tid, p;
  bool part, over;   // takes part; left out because its track id is at or past tid_cap
};

__device__ __forceinline__ WorldRow world_row(const double* __restrict__ lm, int count, int tid_cap) {
  WorldRow o;
  const double t = lm[0], w = lm[7];
  const bool fin = isfinite(lm[1]) && isfinite(lm[2]) && isfinite(lm[3]);
  const bool pok = isfinite(w) && w >= 0.0 && w < (double)count;
  const bool tok = isfinite(t) && t >= 0.0;
  o.part = fin && pok && tok && t < (double)tid_cap;
  o.over = fin && pok && tok && !(t < (double)tid_cap);
  o.tid = o.part ? (int)t : 0;
  o.p = pok ? (int)w : 0;
  return o;
}

// grid (cdiv(row_cap, WORLD_BLOCK)).  cls [row_cap]: WORLD_CLS_SKIP, WORLD_CLS_NEW or the row's slot; bcount [3][WORLD_MAX_BLOCKS] =
// new rows, updated rows, rows whose track id is past tid_cap, per block.
__global__ __launch_bounds__(WORLD_BLOCK) void world_classify_kernel(const int32_t* __restrict__ hdr, const double* __restrict__ landmarks,
                                                                     const int32_t* __restrict__ n_landmarks, int row_cap,
                                                                     const int32_t* __restrict__ count_new, int point_cap,
                                                                     const int32_t* __restrict__ map_tid,
                                                                     const int32_t* __restrict__ slot_of_tid, int tid_cap,
                                                                     int32_t* __restrict__ cls, int32_t* __restrict__ bcount) {
  const int r = blockIdx.x * WORLD_BLOCK + threadIdx.x;
  const int n_rows0 = hdr[0];
  const int nl = hdr[1] ? min(max(n_landmarks[0], 0), row_cap) : 0;
  const int count = min(max(count_new[0], 0), point_cap);
  int code = WORLD_CLS_SKIP;
  bool over = false;
  if (r < nl) {
    const WorldRow w = world_row(landmarks + (size_t)r * LM_WORDS, count, tid_cap);
    over = w.over;
    if (w.part) {
      const int s = slot_of_tid[w.tid];
      code = (s >= 0 && s < n_rows0 && map_tid[s] == w.tid) ? s : WORLD_CLS_NEW;
    }
  }
  if (r < row_cap) cls[r] = code;
  const int n_new = __syncthreads_count(code == WORLD_CLS_NEW);
  const int n_upd = __syncthreads_count(code >= 0);
  const int n_over = __syncthreads_count(over);
  if (threadIdx.x == 0) {
    bcount[blockIdx.x] = n_new;
    bcount[WORLD_MAX_BLOCKS + blockIdx.x] = n_upd;
    bcount[2 * WORLD_MAX_BLOCKS + blockIdx.x] = n_over;
  }
}

__global__ __launch_bounds__(WORLD_BLOCK) void world_scatter_kernel(const int32_t* __restrict__ hdr, const double* __restrict__ landmarks,
                                                                    int row_cap, const float* __restrict__ desc_new, int point_cap,
                                                                    const int32_t* __restrict__ cls, const int32_t* __restrict__ bcount,
                                                                    int n_blocks, int n_frames, int map_cap, double* __restrict__ map_x,
                                                                    float* __restrict__ map_desc, int32_t* __restrict__ map_tid,
                                                                    int32_t* __restrict__ map_views, int32_t* __restrict__ map_first,
                                                                    int32_t* __restrict__ map_last, double* __restrict__ map_rms,
                                                                    int32_t* __restrict__ slot_of_tid, int32_t* __restrict__ state) {
  __shared__ int wsum[WORLD_BLOCK / 64];
  __shared__ int sh_slot[WORLD_BLOCK], sh_p[WORLD_BLOCK];
  if (!hdr[1]) return;   // not anchored: nothing is inserted (the whole grid)
  const int tid = threadIdx.x, r = blockIdx.x * WORLD_BLOCK + tid;
  const int n_rows0 = hdr[0];
  int base = 0;
  for (int b = 0; b < (int)blockIdx.x; ++b) base += bcount[b];
  const int code = r < row_cap ? cls[r] : WORLD_CLS_SKIP;
  int total;
  const int rank = block_scan<WORLD_BLOCK>(code == WORLD_CLS_NEW ? 1 : 0, wsum, total);
  int slot = -1, p = 0;
  if (code != WORLD_CLS_SKIP) {
    const double* lm = landmarks + (size_t)r * LM_WORDS;
    slot = code == WORLD_CLS_NEW ? n_rows0 + base + rank : code;
    if (slot >= map_cap) slot = -1;   // the map is full: dropped, counted by block 0
    p = min(max((int)lm[7], 0), point_cap - 1);
    if (slot >= 0) {
      map_x[(size_t)slot * 3] = lm[1];
      map_x[(size_t)slot * 3 + 1] = lm[2];
      map_x[(size_t)slot * 3 + 2] = lm[3];
      map_views[slot] = (int)lm[4];
      map_rms[slot] = lm[5];
      map_last[slot] = n_frames - 1;
      if (code == WORLD_CLS_NEW) {
        const int t = (int)lm[0];
        map_tid[slot] = t;
        map_first[slot] = n_frames - 1;
        slot_of_tid[t] = slot;
      }
    }
  }
  sh_slot[tid] = slot;
  sh_p[tid] = p;
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int k = wave; k < WORLD_BLOCK; k += WORLD_BLOCK / 64) {
    const int s = sh_slot[k];
    if (s < 0) continue;
    reinterpret_cast<float4*>(map_desc + (size_t)s * 256)[lane] = reinterpret_cast<const float4*>(desc_new + (size_t)sh_p[k] * 256)[lane];
  }
  if (blockIdx.x == 0 && tid == 0) {
    int n_new = 0, n_upd = 0, n_over = 0;
    for (int b = 0; b < n_blocks; ++b) {
      n_new += bcount[b];
      n_upd += bcount[WORLD_MAX_BLOCKS + b];
      n_over += bcount[2 * WORLD_MAX_BLOCKS + b];
    }
    const int appended = min(n_new, map_cap - n_rows0);
    state[0] = n_rows0 + appended;
    state[4] += n_new - appended;
    state[5] += n_over;
    state[6] = appended;
    state[7] = n_upd;
  }
}

// ---- the join ----
// grid (1), 256 threads.  match [cap][3] rows (map row, frame point, d) of world_compact_kernel; pts_new [point_cap][pt_stride] rows
// starting (x, y), count_new [1] its rows.  corr [cap][PNP_CORR_WORDS]; n_out [2] = rows, valid rows.
__global__ __launch_bounds__(256) void world_corr_kernel(const double* __restrict__ map_x, const int32_t* __restrict__ world_state, int map_cap,
                                                         const float* __restrict__ match, const int32_t* __restrict__ n_match, int cap,
                                                         const double* __restrict__ pts_new, int pt_stride,
                                                         const int32_t* __restrict__ count_new, int point_cap, double* __restrict__ corr,
                                                         int32_t* __restrict__ n_out) {
  const int tid = threadIdx.x;
  const int n_rows = min(max(world_state[0], 0), map_cap), count = min(max(count_new[0], 0), point_cap);
  const int n = min(max(n_match[0], 0), cap);
  int total = 0;
  for (int k0 = 0; k0 < cap; k0 += 256) {
    const int k = k0 + tid;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    int row = 0;
    bool valid = false;
    if (k < n) {
      const float fi = match[(size_t)k * 3], fj = match[(size_t)k * 3 + 1];
      if (fi >= 0.f && fi < (float)n_rows && fj >= 0.f && fj < (float)count) {
        row = (int)fi;
        const double* px = pts_new + (size_t)(int)fj * pt_stride;
        v[0] = map_x[(size_t)row * 3];
        v[1] = map_x[(size_t)row * 3 + 1];
        v[2] = map_x[(size_t)row * 3 + 2];
        v[3] = px[0];
        v[4] = px[1];
        valid = pnp_finite5(v);
      }
    }
    if (k < cap) pnp_store_corr(corr + (size_t)k * PNP_CORR_WORDS, v, row, valid);
    total += __syncthreads_count(valid);
  }
  if (tid == 0) {
    n_out[0] = n;
    n_out[1] = total;
  }
}

// ---- the repair ----
// grid (1), 64 threads, one sequence: pose_repair_kernel's rule on row n - 1 (1 <= n < capacity rows in the table), firing when the
// world pose has status 0 and is finite and the row carries flag bit 0 or 1 or the map is lost (rows, not anchored).  Sets
// PNP_FLAG_ABSOLUTE and WORLD_FLAG_WORLD; the streak of consecutive rewritten frames grows by one, or is zeroed when nothing is written.
__global__ __launch_bounds__(64) void world_repair_kernel(const double* __restrict__ rw_in, const double* __restrict__ c_in,
                                                          const int32_t* __restrict__ status_in, double* __restrict__ st,
                                                          double* __restrict__ table, int capacity, int map_cap,
                                                          int32_t* __restrict__ world_state) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  const double nf = st[0];
  const int n = (nf >= 0.0 && nf < 2147483647.0) ? (int)nf : 0;
  const bool lost = min(max(world_state[0], 0), map_cap) > 0 && world_state[1] == 0;
  bool fire = n >= 1 && n < capacity && status_in[0] == 0;
  double Rw[9], C[3];
  int flags = 0;
  double* row = table;
  if (fire) {
    row = table + (size_t)(n - 1) * POSE_ROW_WORDS;
    flags = (int)row[14];
    fire = pnp_load_pose(rw_in, c_in, Rw, C) && ((flags & 3) || lost);
  }
  if (!fire) {
    world_state[3] = 0;
    return;
  }
  pnp_rewrite_row(st, row, n, flags, Rw, C, PNP_FLAG_ABSOLUTE | WORLD_FLAG_WORLD);
  world_state[3] = world_state[3] + 1;
}

}  // namespace sspk
