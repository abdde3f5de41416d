// The C entry points of the trajectory evaluation: ssp_op_traj_align, ssp_op_traj_ape, ssp_op_traj_rpe_delta,
// ssp_op_traj_rpe_segments and ssp_op_traj_stats.  Included by ssp.hip inside an extern "C" block right after
// world_upkeep_host.hip.h; it keeps the host convention of ops_host.hip.h (refuse first: scalar ranges by name, then null pointers;
// then launch) and uses its helpers (fail, CHK, HIPCHK, cdiv).  A file of its own: the refusal contract of ops_host.hip.h
// (tests/c_refusal_contract.json) is a record of that file's entry points as they stood; what these five answer is held by
// tests/test_traj_eval_refusals_cpu.py.  No call needs a workspace, synchronises with the host or allocates.
#pragma once

static_assert(TRAJ_ROW_WORDS == SSP_POSE_ROW_WORDS && TRAJ_GT_WORDS == SSP_TRAJ_GT_WORDS && TRAJ_SIM_WORDS == SSP_TRAJ_SIM_WORDS &&
                  TRAJ_STATS_WORDS == SSP_TRAJ_STATS_WORDS && TRAJ_INFO_WORDS == SSP_TRAJ_INFO_WORDS &&
                  TRAJ_MAX_LENGTHS == SSP_TRAJ_MAX_LENGTHS,
              "include/ssp_hip.h and traj_eval_kernels.hip.h disagree");

// the scalars every entry point shares
static int traj_check(const char* what, int capacity, int table_stride, int n_gt, int gt_stride, int skip_flags, int n_problems) {
  if (capacity < 1 || capacity > SSP_TRAJ_MAX_FRAMES || table_stride < capacity)
    return fail(-1, "%s: 1 <= capacity <= %d and table_stride >= capacity required (capacity %d, table_stride %d)", what,
                SSP_TRAJ_MAX_FRAMES, capacity, table_stride);
  if (n_gt < 1 || n_gt > SSP_TRAJ_MAX_FRAMES || (gt_stride != 0 && gt_stride < n_gt))
    return fail(-1, "%s: 1 <= n_gt <= %d and gt_stride == 0 or gt_stride >= n_gt required (n_gt %d, gt_stride %d)", what,
                SSP_TRAJ_MAX_FRAMES, n_gt, gt_stride);
  if (skip_flags < 0) return fail(-1, "%s: skip_flags must be non-negative (skip_flags %d)", what, skip_flags);
  if (n_problems < 1 || n_problems > SSP_TRAJ_MAX_PROBLEMS)
    return fail(-1, "%s: 1 <= n_problems <= %d required (n_problems %d)", what, SSP_TRAJ_MAX_PROBLEMS, n_problems);
  return 0;
}

static TrajIn traj_in(const double* table_dev, int table_stride, const int32_t* n_frames_dev, int capacity, const double* gt_dev,
                      int gt_stride, int n_gt, const int32_t* index_dev, int skip_flags) {
  return TrajIn{table_dev, (size_t)table_stride * TRAJ_ROW_WORDS, n_frames_dev, capacity, gt_dev, (size_t)gt_stride * TRAJ_GT_WORDS,
                n_gt,      index_dev, skip_flags};
}

int ssp_op_traj_align(const double* table_dev, int table_stride, const int32_t* n_frames_dev, int capacity, const double* gt_dev,
                      int gt_stride, int n_gt, const int32_t* index_dev, int skip_flags, int mode, int n_problems, double* sim_dev,
                      void* stream) {
  CHK(traj_check("traj_align", capacity, table_stride, n_gt, gt_stride, skip_flags, n_problems));
  if (mode < 0 || mode > 3) return fail(-1, "traj_align: mode must be 0 (SE3), 1 (Sim3), 2 (origin) or 3 (origin and scale) (mode %d)", mode);
  if (!table_dev || !n_frames_dev || !gt_dev || !sim_dev) return fail(-1, "traj_align: null pointer");
  hipLaunchKernelGGL(traj_align_kernel, dim3(n_problems), dim3(TRAJ_THREADS), 0, (hipStream_t)stream,
                     traj_in(table_dev, table_stride, n_frames_dev, capacity, gt_dev, gt_stride, n_gt, index_dev, skip_flags), mode, sim_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_traj_ape(const double* table_dev, int table_stride, const int32_t* n_frames_dev, int capacity, const double* gt_dev,
                    int gt_stride, int n_gt, const int32_t* index_dev, int skip_flags, int n_problems, const double* sim_dev,
                    double* err_t_dev, double* err_r_dev, int32_t* valid_dev, void* stream) {
  CHK(traj_check("traj_ape", capacity, table_stride, n_gt, gt_stride, skip_flags, n_problems));
  if (!table_dev || !n_frames_dev || !gt_dev || !sim_dev || !err_t_dev || !err_r_dev || !valid_dev) return fail(-1, "traj_ape: null pointer");
  hipLaunchKernelGGL(traj_ape_kernel, dim3(cdiv(capacity, TRAJ_THREADS), n_problems), dim3(TRAJ_THREADS), 0, (hipStream_t)stream,
                     traj_in(table_dev, table_stride, n_frames_dev, capacity, gt_dev, gt_stride, n_gt, index_dev, skip_flags), sim_dev,
                     err_t_dev, err_r_dev, valid_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_traj_rpe_delta(const double* table_dev, int table_stride, const int32_t* n_frames_dev, int capacity, const double* gt_dev,
                          int gt_stride, int n_gt, const int32_t* index_dev, int skip_flags, int n_problems, const double* scale_dev,
                          int scale_stride, int delta, double* err_t_dev, double* err_r_dev, int32_t* valid_dev, void* stream) {
  CHK(traj_check("traj_rpe_delta", capacity, table_stride, n_gt, gt_stride, skip_flags, n_problems));
  if (delta < 1 || delta > capacity || scale_stride < 0)
    return fail(-1, "traj_rpe_delta: 1 <= delta <= capacity and scale_stride >= 0 required (delta %d, capacity %d, scale_stride %d)", delta,
                capacity, scale_stride);
  if (!table_dev || !n_frames_dev || !gt_dev || !err_t_dev || !err_r_dev || !valid_dev) return fail(-1, "traj_rpe_delta: null pointer");
  hipLaunchKernelGGL(traj_rpe_delta_kernel, dim3(cdiv(capacity, TRAJ_THREADS), n_problems), dim3(TRAJ_THREADS), 0, (hipStream_t)stream,
                     traj_in(table_dev, table_stride, n_frames_dev, capacity, gt_dev, gt_stride, n_gt, index_dev, skip_flags), scale_dev,
                     scale_stride, delta, err_t_dev, err_r_dev, valid_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_traj_rpe_segments(const double* table_dev, int table_stride, const int32_t* n_frames_dev, int capacity, const double* gt_dev,
                             int gt_stride, int n_gt, const int32_t* index_dev, int skip_flags, int n_problems, const double* scale_dev,
                             int scale_stride, const double* lengths_dev, int n_len, int step, double* dist_dev, double* seg_dev,
                             double* summary_dev, int32_t* info_dev, void* stream) {
  CHK(traj_check("traj_rpe_segments", capacity, table_stride, n_gt, gt_stride, skip_flags, n_problems));
  if (n_len < 1 || n_len > SSP_TRAJ_MAX_LENGTHS || step < 1 || step > SSP_TRAJ_MAX_FRAMES || scale_stride < 0)
    return fail(-1, "traj_rpe_segments: 1 <= n_len <= %d, 1 <= step <= %d and scale_stride >= 0 required (n_len %d, step %d, scale_stride %d)",
                SSP_TRAJ_MAX_LENGTHS, SSP_TRAJ_MAX_FRAMES, n_len, step, scale_stride);
  if (!table_dev || !n_frames_dev || !gt_dev || !lengths_dev || !dist_dev || !seg_dev || !summary_dev || !info_dev)
    return fail(-1, "traj_rpe_segments: null pointer");
  hipLaunchKernelGGL(traj_rpe_segments_kernel, dim3(n_problems), dim3(TRAJ_THREADS), 0, (hipStream_t)stream,
                     traj_in(table_dev, table_stride, n_frames_dev, capacity, gt_dev, gt_stride, n_gt, index_dev, skip_flags), scale_dev,
                     scale_stride, lengths_dev, n_len, step, cdiv(capacity, step), dist_dev, seg_dev, summary_dev, info_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_traj_stats(const double* err_dev, const int32_t* valid_dev, int capacity, int n_problems, double* stats_dev, void* stream) {
  if (capacity < 1 || capacity > SSP_TRAJ_MAX_FRAMES)
    return fail(-1, "traj_stats: 1 <= capacity <= %d required (capacity %d)", SSP_TRAJ_MAX_FRAMES, capacity);
  if (n_problems < 1 || n_problems > SSP_TRAJ_MAX_PROBLEMS)
    return fail(-1, "traj_stats: 1 <= n_problems <= %d required (n_problems %d)", SSP_TRAJ_MAX_PROBLEMS, n_problems);
  if (!err_dev || !valid_dev || !stats_dev) return fail(-1, "traj_stats: null pointer");
  hipLaunchKernelGGL(traj_stats_kernel, dim3(n_problems), dim3(TRAJ_THREADS), 0, (hipStream_t)stream, err_dev, valid_dev, capacity,
                     stats_dev);
  HIPCHK(hipGetLastError());
  return 0;
}
