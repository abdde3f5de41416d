// The C entry points of the world map's upkeep: ssp_world_upkeep_workspace_bytes and ssp_op_world_upkeep.
// Included by ssp.hip inside an extern "C" block right after ops_host.hip.h, whose host convention it keeps (refuse first: the family
// check, then scalar ranges, then null pointers, then the fields of the parameter struct; then carve the workspace; then launch) and
// whose helpers it uses (world_check, ROW_CAP_MAX, Carver, fail, CHK, HIPCHK, cdiv, align_up).  A file of its own: the refusal
// contract of ops_host.hip.h (tests/c_refusal_contract.json) is a record of that file's entry points as they stood; what these two
// answer is held by tests/test_world_upkeep_refusals_cpu.py.
#pragma once

static_assert(UPKEEP_REPORT_WORDS == SSP_WORLD_UPKEEP_REPORT_WORDS && sizeof(UpkeepParams) == sizeof(ssp_world_upkeep_params),
              "include/ssp_hip.h and world_upkeep_kernels.hip.h disagree");
// the header, the rows' marks and destinations, the owners of the frame's points, the merging pairs, the eviction keys, and a
// staging store of map_cap rows in the map's own layout
struct UpkeepWs {
  int32_t *hdr, *dead, *dstslot, *owner, *pair;
  uint64_t* keys;
  UpkeepStore stage;
  size_t bytes;
};
static UpkeepWs upkeep_carve(int map_cap, void* base) {
  Carver c{reinterpret_cast<char*>(base), 0};
  UpkeepWs w;
  const size_t n = (size_t)map_cap;
  w.hdr = c.take<int32_t>(UPKEEP_HDR_WORDS);
  w.dead = c.take<int32_t>(n);
  w.dstslot = c.take<int32_t>(n);
  w.owner = c.take<int32_t>(SSP_MATCH_MAX_POINTS);
  w.pair = c.take<int32_t>(2 * (size_t)SSP_MATCH_MAX_POINTS);
  w.keys = c.take<uint64_t>(n);
  w.stage.x = c.take<double>(3 * n);
  w.stage.rms = c.take<double>(n);
  w.stage.desc = c.take<float>(256 * n);
  w.stage.tid = c.take<int32_t>(n);
  w.stage.views = c.take<int32_t>(n);
  w.stage.first = c.take<int32_t>(n);
  w.stage.last = c.take<int32_t>(n);
  w.bytes = align_up(c.off, 256);
  return w;
}

size_t ssp_world_upkeep_workspace_bytes(int map_cap) {
  if (world_check("world_upkeep_workspace_bytes", map_cap, 1)) return 0;
  return upkeep_carve(map_cap, nullptr).bytes;
}

int ssp_op_world_upkeep(const float* match_dev, const int32_t* n_match_dev, int cap, const double* landmarks_dev,
                        const int32_t* n_landmarks_dev, int row_cap, const double* pts_new_dev, int pt_stride,
                        const int32_t* count_new_dev, int point_cap, const double* table_dev, int capacity, int n_frames,
                        const double* intr_dev, const ssp_world_upkeep_params* params, int map_cap, int tid_cap, double* x_dev,
                        float* desc_dev, int32_t* tid_dev, int32_t* views_dev, int32_t* first_dev, int32_t* last_dev, double* rms_dev,
                        int32_t* slot_of_tid_dev, int32_t* state_dev, int32_t* report_dev, int64_t* totals_dev, void* workspace_dev,
                        void* stream) {
  CHK(world_check("world_upkeep", map_cap, cap));
  if (point_cap < 1 || point_cap > SSP_MATCH_MAX_POINTS || pt_stride < 2)
    return fail(-1, "world_upkeep: 1 <= point_cap <= %d and pt_stride >= 2 required (point_cap %d, pt_stride %d)", SSP_MATCH_MAX_POINTS,
                point_cap, pt_stride);
  if (row_cap < 1 || row_cap > ROW_CAP_MAX || tid_cap < 1 || capacity < 0 || n_frames < 0)
    return fail(-1, "world_upkeep: 1 <= row_cap <= %d, tid_cap >= 1, capacity >= 0 and n_frames >= 0 required (row_cap %d, tid_cap %d, "
                "capacity %d, n_frames %d)", ROW_CAP_MAX, row_cap, tid_cap, capacity, n_frames);
  if (!match_dev || !n_match_dev || !landmarks_dev || !n_landmarks_dev || !pts_new_dev || !count_new_dev || (capacity > 0 && !table_dev) ||
      !intr_dev || !params || !x_dev || !desc_dev || !tid_dev || !views_dev || !first_dev || !last_dev || !rms_dev || !slot_of_tid_dev ||
      !state_dev || !report_dev || !workspace_dev)
    return fail(-1, "world_upkeep: null pointer");
  if (params->merge != 0 && !(params->merge_thresh >= 0.0 && std::isfinite(params->merge_thresh)))
    return fail(-1, "world_upkeep: merge_thresh must be finite and non-negative");
  if (params->high_water >= 0 && !(0 <= params->low_water && params->low_water <= params->high_water && params->high_water <= map_cap))
    return fail(-1, "world_upkeep: 0 <= low_water <= high_water <= map_cap required, or a negative high_water for no eviction "
                "(low_water %d, high_water %d, map_cap %d)", params->low_water, params->high_water, map_cap);
  hipStream_t st = (hipStream_t)stream;
  const UpkeepWs w = upkeep_carve(map_cap, workspace_dev);
  const UpkeepParams prm{params->merge, params->merge_thresh, params->cull_age, params->cull_min_views, params->high_water,
                         params->low_water};
  const UpkeepStore m{x_dev, desc_dev, tid_dev, views_dev, first_dev, last_dev, rms_dev};
  const int move_blocks = std::min(cdiv(map_cap, UPKEEP_MOVE_THREADS / 64), UPKEEP_MOVE_BLOCKS_MAX);
  hipLaunchKernelGGL(upkeep_begin_kernel, dim3(cdiv(std::max(map_cap, point_cap), WORLD_BLOCK)), dim3(WORLD_BLOCK), 0, st,
                     (const int32_t*)state_dev, map_cap, capacity, n_frames, point_cap, w.hdr, w.dead, w.owner);
  if (prm.merge) {
    hipLaunchKernelGGL(upkeep_owner_kernel, dim3(cdiv(row_cap, WORLD_BLOCK)), dim3(WORLD_BLOCK), 0, st, (const int32_t*)w.hdr, landmarks_dev,
                       n_landmarks_dev, row_cap, count_new_dev, point_cap, tid_cap, w.owner);
    hipLaunchKernelGGL(upkeep_decide_kernel, dim3(cdiv(cap, UPKEEP_MERGE_THREADS)), dim3(UPKEEP_MERGE_THREADS), 0, st, (const int32_t*)w.hdr,
                       match_dev, n_match_dev, cap, landmarks_dev, (const int32_t*)w.owner, pts_new_dev, pt_stride, count_new_dev, point_cap,
                       table_dev, intr_dev, prm, (const double*)x_dev, (const int32_t*)tid_dev, (const int32_t*)last_dev,
                       (const int32_t*)slot_of_tid_dev, w.pair);
    hipLaunchKernelGGL(upkeep_merge_kernel, dim3(cdiv(cap, UPKEEP_MERGE_THREADS)), dim3(UPKEEP_MERGE_THREADS), 0, st, (const int32_t*)w.hdr,
                       (const int32_t*)w.pair, cap, prm, m, slot_of_tid_dev, w.dead);
  }
  hipLaunchKernelGGL(upkeep_select_kernel, dim3(1), dim3(WORLD_BLOCK), 0, st, w.hdr, (const int32_t*)views_dev, (const int32_t*)last_dev, prm,
                     w.dead, w.keys, w.dstslot);
  hipLaunchKernelGGL(upkeep_gather_kernel, dim3(move_blocks), dim3(UPKEEP_MOVE_THREADS), 0, st, (const int32_t*)w.hdr,
                     (const int32_t*)w.dstslot, m, w.stage);
  hipLaunchKernelGGL(upkeep_place_kernel, dim3(move_blocks), dim3(UPKEEP_MOVE_THREADS), 0, st, (const int32_t*)w.hdr, w.stage, m,
                     slot_of_tid_dev, tid_cap, state_dev, report_dev, reinterpret_cast<long long*>(totals_dev));
  HIPCHK(hipGetLastError());
  return 0;
}
