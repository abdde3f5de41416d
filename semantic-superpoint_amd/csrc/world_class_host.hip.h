// The C entry points of the world map's classes: ssp_op_track_class_votes, ssp_op_world_classes and
// ssp_match_world_classes.  Included by ssp.hip inside an extern "C" block after world_upkeep_host.hip.h; it keeps the host
// convention of ops_host.hip.h (refuse first: the family check, then scalar ranges, then null pointers; then carve the workspace; then
// launch) and uses its helpers (world_check, match_carve, ROW_CAP_MAX, fail, CHK, HIPCHK, cdiv).  A file of its own for the reason
// world_upkeep_host.hip.h gives: tests/c_refusal_contract.json records the entry points of ops_host.hip.h as they stood.
#pragma once

static_assert(WORLD_CLASS_NONE == SSP_CLASS_NONE, "include/ssp_hip.h and world_class_kernels.hip.h disagree");

int ssp_op_track_class_votes(const double* landmarks_dev, const int32_t* n_landmarks_dev, int row_cap, const uint8_t* cls_new_dev,
                             const int32_t* count_new_dev, int point_cap, uint16_t* votes_dev, int tid_cap, void* stream) {
  if (row_cap < 1 || row_cap > ROW_CAP_MAX || point_cap < 1 || point_cap > SSP_MATCH_MAX_POINTS || tid_cap < 1)
    return fail(-1, "track_class_votes: 1 <= row_cap <= %d, 1 <= point_cap <= %d and tid_cap >= 1 required (row_cap %d, point_cap %d, "
                "tid_cap %d)", ROW_CAP_MAX, SSP_MATCH_MAX_POINTS, row_cap, point_cap, tid_cap);
  if (!landmarks_dev || !n_landmarks_dev || !cls_new_dev || !count_new_dev || !votes_dev) return fail(-1, "track_class_votes: null pointer");
  return launch<world_vote_kernel>(dim3(cdiv(row_cap, WORLD_CLASS_BLOCK)), dim3(WORLD_CLASS_BLOCK), 0, (hipStream_t)stream, landmarks_dev,
                                   n_landmarks_dev, row_cap, cls_new_dev, count_new_dev, point_cap, votes_dev, tid_cap);
}

int ssp_op_world_classes(const int32_t* tid_dev, const int32_t* state_dev, int map_cap, const uint16_t* votes_dev, int tid_cap,
                         uint8_t* out_dev, void* stream) {
  CHK(world_check("world_classes", map_cap, 1));
  if (tid_cap < 1) return fail(-1, "world_classes: tid_cap >= 1 required (tid_cap %d)", tid_cap);
  if (!tid_dev || !state_dev || !votes_dev || !out_dev) return fail(-1, "world_classes: null pointer");
  return launch<world_classes_kernel>(dim3(cdiv(map_cap, WORLD_CLASS_BLOCK)), dim3(WORLD_CLASS_BLOCK), 0, (hipStream_t)stream, tid_dev,
                                      state_dev, map_cap, votes_dev, tid_cap, out_dev);
}

// ssp_match_world with world_match_kernel<true>; the workspace is ssp_match_world_workspace_bytes(map_cap, cap) bytes
int ssp_match_world_classes(const float* desc_dev, const int32_t* tid_dev, const int32_t* state_dev, int map_cap,
                            const uint16_t* votes_dev, int tid_cap, const float* desc2_dev, const uint8_t* cls2_dev,
                            const int32_t* count2_dev, int cap, const uint32_t keep_mask[8], float nn_thresh, void* workspace_dev,
                            float* match_dev, int32_t* n_match_dev, void* stream) {
  CHK(world_check("match_world_classes", map_cap, cap));
  if (tid_cap < 1) return fail(-1, "match_world_classes: tid_cap >= 1 required (tid_cap %d)", tid_cap);
  if (!(nn_thresh >= 0.f)) return fail(-1, "match_world_classes: nn_thresh must be non-negative");
  if (!desc_dev || !tid_dev || !state_dev || !votes_dev || !desc2_dev || !cls2_dev || !count2_dev || !keep_mask || !workspace_dev ||
      !match_dev || !n_match_dev)
    return fail(-1, "match_world_classes: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const MatchWs w = match_carve(map_cap, cap, workspace_dev);
  WorldClasses wc{tid_dev, votes_dev, cls2_dev, tid_cap, {}};
  for (int k = 0; k < 8; ++k) wc.keep[k] = keep_mask[k];
  HIPCHK(hipMemsetAsync(w.rowmin, 0xFF, w.keys * sizeof(uint64_t), st));
  hipLaunchKernelGGL(world_match_kernel<true>, dim3(cdiv(map_cap, WORLD_STRIP), WORLD_SPLIT_MAX), dim3(256), 0, st, desc_dev, state_dev, map_cap,
                     desc2_dev, count2_dev, cap, w.rowmin, w.colmin, wc);
  hipLaunchKernelGGL(world_compact_kernel, dim3(1), dim3(WORLD_BLOCK), 0, st, (const uint64_t*)w.rowmin, (const uint64_t*)w.colmin, state_dev,
                     map_cap, count2_dev, cap, nn_thresh, match_dev, n_match_dev);
  HIPCHK(hipGetLastError());
  return 0;
}
