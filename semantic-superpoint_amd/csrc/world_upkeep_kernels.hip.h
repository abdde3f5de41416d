// World map upkeep: one call per frame, right after the insert.  It merges the row pair of a scene point that
// returned under a new track id, culls rows that never matured, evicts the least valuable rows when the map nears its capacity,
// and compacts the store.  The rules are restated in numpy by tests/world_upkeep_ref.py.
//   upkeep_begin_kernel    a thread per map row / frame point: every row alive, no point owned; thread 0 of block 0 decides whether
//                          the call runs (anchored, rows, a trajectory row for the newest frame) and leaves that in the header
//   upkeep_owner_kernel    a thread per landmark row: the lowest landmark row that names a frame point owns it (integer atomicMin)
//   upkeep_decide_kernel   a thread per match row: the five-part gate (the fp64 reprojection of pnp_view, contraction off) on the
//                          map as the insert left it; the pairs that merge go to the workspace
//   upkeep_merge_kernel    a thread per pair: the survivor's scalar columns, then a wave per pair for the 1 KB descriptor copy.
//                          Pairs are disjoint: a match list is one-to-one and a point belongs to one track, so no two threads
//                          touch one row
//   upkeep_select_kernel   one workgroup: cull, count, the 56-bit eviction keys (thread t takes rows t, t + 1024, ...), a radix select
//                          (seven 8-bit digits, histograms by integer LDS atomics) for the k-th smallest key, and the stable scan
//                          in tiles of 4096 rows that gives every survivor its destination
//   upkeep_gather_kernel   a wave per surviving row at or past the first dead slot: the row into the staging store at its destination
//   upkeep_place_kernel    a wave per destination from the first dead slot on: staging back into the map, slot_of_tid rewritten;
//                          thread 0 of block 0 writes the row count, the report and the running totals
// The compaction never moves a row inside the map: the gather reads the map and writes only staging, the placement reads only
// staging and writes the map, and the kernel boundary orders the two.  No workgroup reads a map row that another one writes.
// Needs: geom_blocks.hip.h (block_scan, block_sum), pose_kernels.hip.h (POSE_ROW_WORDS), landmark_kernels.hip.h (LM_WORDS),
// pnp_kernels.hip.h (pnp_view), world_kernels.hip.h (world_row, WORLD_BLOCK).
#pragma once

namespace sspk {

#define UPKEEP_REPORT_WORDS 8   // rows before, merged, culled, evicted, rows after, eviction fired, rows wanted but protected, skipped
#define UPKEEP_HDR_WORDS 16     // run, rows before, f, merged, culled, evicted, rows after, fired, protected, first dead slot
#define UPKEEP_ALIVE 0
#define UPKEEP_MERGED 1
#define UPKEEP_CULLED 2
#define UPKEEP_EVICTED 3
#define UPKEEP_NO_OWNER 0x7FFFFFFF
#define UPKEEP_NO_KEY (~0ull)
#define UPKEEP_MERGE_THREADS 256
#define UPKEEP_MOVE_THREADS 256
#define UPKEEP_MOVE_BLOCKS_MAX 2048

struct UpkeepParams {
  int merge;
  double merge_thresh;
  int cull_age, cull_min_views, high_water, low_water;
};

// The map's arrays, and the staging copy of the same layout in the workspace.
struct UpkeepStore {
  double* x;
  float* desc;
  int32_t *tid, *views, *first, *last;
  double* rms;
};

__global__ __launch_bounds__(WORLD_BLOCK) void upkeep_begin_kernel(const int32_t* __restrict__ state, int map_cap, int capacity, int n_frames,
                                                                   int point_cap, int32_t* __restrict__ hdr, int32_t* __restrict__ dead,
                                                                   int32_t* __restrict__ owner) {
  const int i = blockIdx.x * WORLD_BLOCK + threadIdx.x;
  if (i < map_cap) dead[i] = UPKEEP_ALIVE;
  if (i < point_cap) owner[i] = UPKEEP_NO_OWNER;
  if (i == 0) {
    const int n_rows = min(max(state[0], 0), map_cap);
    const bool run = state[1] == 1 && n_rows > 0 && n_frames >= 1 && n_frames <= capacity;
    hdr[0] = run ? 1 : 0;
    hdr[1] = n_rows;
    hdr[2] = n_frames - 1;
    for (int k = 3; k < UPKEEP_HDR_WORDS; ++k) hdr[k] = 0;
    hdr[6] = n_rows;
    hdr[9] = n_rows;
  }
}

// grid (cdiv(row_cap, WORLD_BLOCK)).  owner [point_cap]: the lowest landmark row that passes the insert's test and names the point.
__global__ __launch_bounds__(WORLD_BLOCK) void upkeep_owner_kernel(const int32_t* __restrict__ hdr, const double* __restrict__ landmarks,
                                                                   const int32_t* __restrict__ n_landmarks, int row_cap,
                                                                   const int32_t* __restrict__ count_new, int point_cap, int tid_cap,
                                                                   int32_t* __restrict__ owner) {
  if (!hdr[0]) return;
  const int q = blockIdx.x * WORLD_BLOCK + threadIdx.x;
  const int nl = min(max(n_landmarks[0], 0), row_cap);
  const int count = min(max(count_new[0], 0), point_cap);
  if (q >= nl) return;
  const WorldRow w = world_row(landmarks + (size_t)q * LM_WORDS, count, tid_cap);
  if (w.part) atomicMin(owner + w.p, q);   // (w.p < count <= point_cap)
}

// grid (cdiv(cap, UPKEEP_MERGE_THREADS)).  match [cap][3] rows (map row, frame point, d); pts_new [point_cap][pt_stride] rows
// starting (x, y); intr [4] = (fx, fy, cx, cy); table [capacity][POSE_ROW_WORDS].  Reads the map as the insert left it and writes
// pair [2][cap] = (r, r') of a match row that merges, (-1, -1) otherwise: every decision is taken before any row changes.
__global__ __launch_bounds__(UPKEEP_MERGE_THREADS) void upkeep_decide_kernel(
    const int32_t* __restrict__ hdr, const float* __restrict__ match, const int32_t* __restrict__ n_match, int cap,
    const double* __restrict__ landmarks, const int32_t* __restrict__ owner, const double* __restrict__ pts_new, int pt_stride,
    const int32_t* __restrict__ count_new, int point_cap, const double* __restrict__ table, const double* __restrict__ intr,
    UpkeepParams prm, const double* __restrict__ map_x, const int32_t* __restrict__ map_tid, const int32_t* __restrict__ map_last,
    const int32_t* __restrict__ slot_of_tid, int32_t* __restrict__ pair) {
#pragma clang fp contract(off)
  if (!hdr[0] || !prm.merge) return;   // (the whole grid)
  const int k = blockIdx.x * UPKEEP_MERGE_THREADS + threadIdx.x;
  if (k >= cap) return;
  const int n_rows = hdr[1], f = hdr[2];
  const int n = min(max(n_match[0], 0), cap), count = min(max(count_new[0], 0), point_cap);
  int r = -1, r2 = -1;
  if (k < n) {
    const float fi = match[(size_t)k * 3], fj = match[(size_t)k * 3 + 1];
    if (fi >= 0.f && fi < (float)n_rows && fj >= 0.f && fj < (float)count) {
      const int i = (int)fi, p = (int)fj;
      const int q = owner[p];
      if (q != UPKEEP_NO_OWNER) {
        const int t2 = (int)landmarks[(size_t)q * LM_WORDS];   // (the owner passed world_row: 0 <= t2 < tid_cap)
        const int s = slot_of_tid[t2];
        const int j = (s >= 0 && s < n_rows && map_tid[s] == t2) ? s : -1;
        if (j >= 0 && j != i && map_last[i] < f && map_last[j] == f) {
          const double* row = table + (size_t)f * POSE_ROW_WORDS;
          double R[9], C[3];
#pragma unroll
          for (int e = 0; e < 9; ++e) R[e] = row[e];
#pragma unroll
          for (int e = 0; e < 3; ++e) C[e] = row[9 + e];
          const PnpIntr K{intr[0], intr[1], intr[2], intr[3]};
          const double* px = pts_new + (size_t)p * pt_stride;
          bool front;
          const double e2 = pnp_view(R, C, map_x[(size_t)i * 3], map_x[(size_t)i * 3 + 1], map_x[(size_t)i * 3 + 2], px[0], px[1], K, front);
          if (front && e2 <= prm.merge_thresh * prm.merge_thresh) {
            r = i;
            r2 = j;
          }
        }
      }
    }
  }
  pair[k] = r;
  pair[cap + k] = r2;
}

// The same grid.  The survivor is the lower slot: it takes the returning track's row and the smaller first_frame, the other row
// dies.  The pairs are disjoint (a match list is one-to-one and a point belongs to one track), so no two threads touch one row.
__global__ __launch_bounds__(UPKEEP_MERGE_THREADS) void upkeep_merge_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ pair,
                                                                            int cap, UpkeepParams prm, UpkeepStore m,
                                                                            int32_t* __restrict__ slot_of_tid, int32_t* __restrict__ dead) {
  __shared__ int sh_src[UPKEEP_MERGE_THREADS], sh_dst[UPKEEP_MERGE_THREADS];
  if (!hdr[0] || !prm.merge) return;   // (the whole grid)
  const int tid = threadIdx.x, k = blockIdx.x * UPKEEP_MERGE_THREADS + tid;
  const int f = hdr[2];
  int src = -1, dst = -1;
  const int r = k < cap ? pair[k] : -1;
  if (r >= 0) {
    const int r2 = pair[cap + k];
    const int keep = min(r, r2), die = max(r, r2);
    const int first = min(m.first[r], m.first[r2]);
    if (keep == r) {
      const int t2 = m.tid[r2];
      m.x[(size_t)r * 3] = m.x[(size_t)r2 * 3];
      m.x[(size_t)r * 3 + 1] = m.x[(size_t)r2 * 3 + 1];
      m.x[(size_t)r * 3 + 2] = m.x[(size_t)r2 * 3 + 2];
      m.rms[r] = m.rms[r2];
      m.views[r] = m.views[r2];
      m.tid[r] = t2;
      m.last[r] = f;
      slot_of_tid[t2] = r;   // (t2 passed the lookup in upkeep_decide_kernel: 0 <= t2 < tid_cap)
      src = r2;
      dst = r;
    }
    m.first[keep] = first;
    dead[die] = UPKEEP_MERGED;
  }
  sh_src[tid] = src;
  sh_dst[tid] = dst;
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < UPKEEP_MERGE_THREADS; j += UPKEEP_MERGE_THREADS / 64) {
    const int s = sh_src[j];
    if (s < 0) continue;
    reinterpret_cast<float4*>(m.desc + (size_t)sh_dst[j] * 256)[lane] = reinterpret_cast<const float4*>(m.desc + (size_t)s * 256)[lane];
  }
}

// The eviction key of a live, unprotected row: fewest views first, then the oldest, then the higher slot.  56 bits, unique by the slot.
__device__ __forceinline__ uint64_t upkeep_key(int views, int last, int slot) {
  return ((uint64_t)min(max(views, 0), 255) << 48) | ((uint64_t)(uint32_t)max(last, 0) << 16) | (uint64_t)(65535 - slot);
}

// grid (1), WORLD_BLOCK threads.  keys [map_cap], dstslot [map_cap] in the workspace.
__global__ __launch_bounds__(WORLD_BLOCK) void upkeep_select_kernel(int32_t* __restrict__ hdr, const int32_t* __restrict__ views,
                                                                    const int32_t* __restrict__ last, UpkeepParams prm,
                                                                    int32_t* __restrict__ dead, uint64_t* __restrict__ keys,
                                                                    int32_t* __restrict__ dstslot) {
  __shared__ int wsum[WORLD_BLOCK / 64];
  __shared__ int red[WORLD_BLOCK / 64];
  __shared__ int hist[256];
  __shared__ unsigned long long sh_prefix;   // the digits of the k-th smallest key found so far (a valid key's top byte is 0)
  __shared__ int sh_remaining, sh_first_dead;
  if (!hdr[0]) return;
  const int tid = threadIdx.x;
  const int n_rows = hdr[1], f = hdr[2];
  if (tid == 0) sh_first_dead = n_rows;
  // merge (already marked) and cull; the keys of the rows that may be evicted.  Thread t takes the rows t, t + 1024, ...: a wave reads
  // 64 consecutive rows, and no phase but the scan below depends on which thread sees which row
  int c_merged = 0, c_culled = 0, c_alive = 0, c_open = 0;
  for (int i = tid; i < n_rows; i += WORLD_BLOCK) {
    int d = dead[i];
    const int lf = last[i], nv = views[i];
    if (d == UPKEEP_ALIVE && prm.cull_age >= 0 && lf < f - prm.cull_age && nv < prm.cull_min_views) {
      d = UPKEEP_CULLED;
      dead[i] = d;
    }
    c_merged += d == UPKEEP_MERGED;
    c_culled += d == UPKEEP_CULLED;
    const bool alive = d == UPKEEP_ALIVE, open = alive && lf != f;
    c_alive += alive;
    c_open += open;
    keys[i] = open ? upkeep_key(nv, lf, i) : UPKEEP_NO_KEY;
  }
  const int merged = block_sum<WORLD_BLOCK>(c_merged, red);
  const int culled = block_sum<WORLD_BLOCK>(c_culled, red);
  const int alive = block_sum<WORLD_BLOCK>(c_alive, red);
  const int open = block_sum<WORLD_BLOCK>(c_open, red);
  // evict: the k smallest keys die (uniform over the workgroup from here on)
  const bool fire = prm.high_water >= 0 && alive > prm.high_water;
  const int want = fire ? alive - prm.low_water : 0;
  const int k = min(want, open);
  if (k > 0) {
    if (tid == 0) {
      sh_prefix = 0ull;
      sh_remaining = k;
    }
    for (int pass = 0; pass < 7; ++pass) {
      const int shift = 48 - 8 * pass;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const unsigned long long prefix = sh_prefix;
      for (int i = tid; i < n_rows; i += WORLD_BLOCK) {
        const uint64_t key = keys[i];
        if (key != UPKEEP_NO_KEY && (key >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255u)], 1);
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
    const uint64_t kth = sh_prefix;   // the k-th smallest key: the keys are unique, so exactly k of them are <= kth
    for (int i = tid; i < n_rows; i += WORLD_BLOCK)
      if (keys[i] <= kth) dead[i] = UPKEEP_EVICTED;   // (UPKEEP_NO_KEY is above every key)
    __syncthreads();   // (the scan reads marks that other threads wrote)
  }
  // the stable scan, in tiles of 4096 rows, four consecutive rows per thread: a survivor's destination is the number of survivors
  // below it
  int running = 0, first_dead = n_rows;
  for (int base = 0; base < n_rows; base += 4 * WORLD_BLOCK) {
    const int i0 = base + 4 * tid;
    bool a[4];
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = i0 + e < n_rows && dead[i0 + e] == UPKEEP_ALIVE;
      cnt += a[e];
      if (i0 + e < n_rows && !a[e] && first_dead == n_rows) first_dead = i0 + e;
    }
    int total;
    int off = running + block_scan<WORLD_BLOCK>(cnt, wsum, total);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (i0 + e < n_rows) dstslot[i0 + e] = a[e] ? off : -1;
      off += a[e];
    }
    running += total;
  }
  const int total = running;
  if (first_dead < n_rows) atomicMin(&sh_first_dead, first_dead);   // (written before the barriers of the sums above)
  __syncthreads();
  if (tid == 0) {
    hdr[3] = merged;
    hdr[4] = culled;
    hdr[5] = k;
    hdr[6] = total;
    hdr[7] = fire ? 1 : 0;
    hdr[8] = want - k;
    hdr[9] = sh_first_dead;
  }
}

__device__ __forceinline__ void upkeep_copy_row(const UpkeepStore& from, int s, const UpkeepStore& to, int d, int lane) {
  reinterpret_cast<float4*>(to.desc + (size_t)d * 256)[lane] = reinterpret_cast<const float4*>(from.desc + (size_t)s * 256)[lane];
  if (lane < 3) to.x[(size_t)d * 3 + lane] = from.x[(size_t)s * 3 + lane];
  if (lane == 3) to.rms[d] = from.rms[s];
  if (lane == 4) to.tid[d] = from.tid[s];
  if (lane == 5) to.views[d] = from.views[s];
  if (lane == 6) to.first[d] = from.first[s];
  if (lane == 7) to.last[d] = from.last[s];
}

// grid (up to UPKEEP_MOVE_BLOCKS_MAX), UPKEEP_MOVE_THREADS threads, a wave per row, grid-stride.  Reads the map, writes staging.
__global__ __launch_bounds__(UPKEEP_MOVE_THREADS) void upkeep_gather_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ dstslot,
                                                                            UpkeepStore m, UpkeepStore stage) {
  if (!hdr[0]) return;
  const int n_rows = hdr[1], first_dead = hdr[9];
  const int lane = threadIdx.x & 63, waves = UPKEEP_MOVE_THREADS / 64;
  for (int i = first_dead + blockIdx.x * waves + (threadIdx.x >> 6); i < n_rows; i += gridDim.x * waves) {
    const int d = dstslot[i];
    if (d >= 0) upkeep_copy_row(m, i, stage, d, lane);   // (first_dead <= d <= i < n_rows <= map_cap)
  }
}

// The same grid.  Reads staging, writes the map; report [UPKEEP_REPORT_WORDS], totals [4] = merged, culled, evicted, calls (or null).
__global__ __launch_bounds__(UPKEEP_MOVE_THREADS) void upkeep_place_kernel(const int32_t* __restrict__ hdr, UpkeepStore stage, UpkeepStore m,
                                                                           int32_t* __restrict__ slot_of_tid, int tid_cap,
                                                                           int32_t* __restrict__ state, int32_t* __restrict__ report,
                                                                           long long* __restrict__ totals) {
  const bool run = hdr[0] != 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    report[0] = hdr[1];
    report[1] = hdr[3];
    report[2] = hdr[4];
    report[3] = hdr[5];
    report[4] = hdr[6];
    report[5] = hdr[7];
    report[6] = hdr[8];
    report[7] = run ? 0 : 1;
    if (run && hdr[6] != hdr[1]) state[0] = hdr[6];
    if (totals) {
      totals[0] += hdr[3];
      totals[1] += hdr[4];
      totals[2] += hdr[5];
      totals[3] += 1;
    }
  }
  if (!run) return;
  const int n_after = hdr[6], first_dead = hdr[9];
  const int lane = threadIdx.x & 63, waves = UPKEEP_MOVE_THREADS / 64;
  for (int d = first_dead + blockIdx.x * waves + (threadIdx.x >> 6); d < n_after; d += gridDim.x * waves) {
    upkeep_copy_row(stage, d, m, d, lane);
    if (lane == 0) {
      const int t = stage.tid[d];
      if (t >= 0 && t < tid_cap) slot_of_tid[t] = d;
    }
  }
}

}  // namespace sspk
