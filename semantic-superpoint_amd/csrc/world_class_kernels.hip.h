// World map classes: what every landmark lies on.  The rules are restated in numpy by
// tests/world_classes_ref.py.
//   votes [tid_cap] uint16, one entry per TRACK ID (map slots move under the upkeep, a track id names one scene track for its whole
//                          life): the low byte is the class, the high byte the vote count; zeroed memory = no class yet; a count of 0
//                          decodes to WORLD_CLASS_NONE whatever the low byte holds
//   world_vote_kernel      a thread per landmark row: the Boyer-Moore majority step with the class of the row's point in the newest
//                          frame.  Track ids are unique within a call, so no two threads touch one entry: plain loads and stores
//   world_classes_kernel   a thread per map slot: the decoded class of the slot's track below n_rows, WORLD_CLASS_NONE past it
// The class-aware matcher is the CLASSES instance of world_match_kernel.
// Needs: landmark_kernels.hip.h (LM_WORDS), world_kernels.hip.h (WORLD_CLASS_NONE, world_class_of).
#pragma once

namespace sspk {

#define WORLD_VOTE_MAX 255
#define WORLD_CLASS_BLOCK 256

// grid (cdiv(row_cap, WORLD_CLASS_BLOCK)).  landmarks [row_cap][LM_WORDS]: word 0 the track id t, word 7 the newest-frame index p.
// A row takes part iff 0 <= p < count, 0 <= t < tid_cap and cls_new[p] != WORLD_CLASS_NONE: world_row's test without X.
__global__ __launch_bounds__(WORLD_CLASS_BLOCK) void world_vote_kernel(const double* __restrict__ landmarks,
                                                                       const int32_t* __restrict__ n_landmarks, int row_cap,
                                                                       const uint8_t* __restrict__ cls_new,
                                                                       const int32_t* __restrict__ count_new, int point_cap,
                                                                       uint16_t* __restrict__ votes, int tid_cap) {
  const int r = blockIdx.x * WORLD_CLASS_BLOCK + threadIdx.x;
  const int nl = min(max(n_landmarks[0], 0), row_cap), count = min(max(count_new[0], 0), point_cap);
  if (r >= nl) return;
  const double t = landmarks[(size_t)r * LM_WORDS], w = landmarks[(size_t)r * LM_WORDS + 7];
  if (!(isfinite(w) && w >= 0.0 && w < (double)count) || !(isfinite(t) && t >= 0.0 && t < (double)tid_cap)) return;
  const uint32_t c = cls_new[(int)w];
  if (c == WORLD_CLASS_NONE) return;
  const uint32_t v = votes[(int)t];
  const uint32_t n = v >> 8, have = v & 255u;
  uint32_t out;
  if (n == 0)
    out = (1u << 8) | c;
  else if (have == c)
    out = (min(n + 1u, (uint32_t)WORLD_VOTE_MAX) << 8) | c;
  else
    out = ((n - 1u) << 8) | have;
  votes[(int)t] = (uint16_t)out;
}

// grid (cdiv(map_cap, WORLD_CLASS_BLOCK)).  out [map_cap] uint8.
__global__ __launch_bounds__(WORLD_CLASS_BLOCK) void world_classes_kernel(const int32_t* __restrict__ map_tid,
                                                                          const int32_t* __restrict__ world_state, int map_cap,
                                                                          const uint16_t* __restrict__ votes, int tid_cap,
                                                                          uint8_t* __restrict__ out) {
  const int i = blockIdx.x * WORLD_CLASS_BLOCK + threadIdx.x;
  if (i >= map_cap) return;
  const int n_rows = min(max(world_state[0], 0), map_cap);
  out[i] = (uint8_t)(i < n_rows ? world_class_of(votes, map_tid[i], tid_cap) : WORLD_CLASS_NONE);
}

}  // namespace sspk
