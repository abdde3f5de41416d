/*
 * ssp_hip.h - C ABI of the MI355X-native Semantic-SuperPoint pair-training path.
 *
 * Every pointer named *_dev is a DEVICE pointer owned by the caller (PyTorch tensors in the
 * Python shims); the library never frees caller memory and keeps no host threads.  All entry
 * points return 0 on success or a negative code; ssp_last_error() gives the message.  `stream`
 * is a hipStream_t passed as void* (0 = default stream).  One handle per GPU / stream.
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   ssp_forward      <- models/SuperPointNet_gauss2.py:42-69, models/SuperPointNet_gauss2_ssmall.py:58-99
 *                       (+ models/unet_parts.py:10-48)
 *   ssp_backward     <- autograd of the above (loss.backward(), Train_model_heatmap_all.py:407)
 *   ssp_pair_step    <- Train_model_heatmap_all.py:195-413 (train_val_sample: 2 forwards, labels2Dto3D
 *                       utils/utils.py:408-440, getMasks Train_model_frontend_all.py:373-386,
 *                       detector_loss :155-179, sem_loss :181-193, batch_descriptor_loss_sparse
 *                       utils/loss_functions/sparse_loss.py:267-284, MultiTaskLoss :46-77, backward)
 *                       or, with ssp_pair_inputs.dense_loss, the dense descriptor_loss utils/utils.py:779-893
 *   ssp_adam_step    <- optimizer.step() of Train_model_frontend_all.py:183-198 (Adam, constant LR)
 *   ssp_sample_indices <- the stochastic half of descriptor_loss_sparse (sparse_loss.py:184-246,
 *                       correspondence_finder.py:191-320), device RNG
 */
#ifndef SSP_HIP_H
#define SSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssp_handle ssp_handle;

enum { SSP_ARCH_GAUSS2 = 0, SSP_ARCH_GAUSS2_SSMALL = 1 };
enum { SSP_NREP = 32 }; /* replicas of each fp64 statistics accumulator (spreads same-address atomics) */

typedef struct {
  int arch;      /* SSP_ARCH_* */
  int n_classes; /* 133 for the ssmall seg head; ignored for gauss2 */
  int max_batch; /* largest N of any forward (1..1024); ssp_pair_step additionally requires batch <= 128
                    (per-image accumulator arrays of the sparse descriptor loss, SSP_MAX_PAIRS) */
  int height;    /* H, multiple of 8 */
  int width;     /* W, multiple of 8 */
  int n_match;   /* num_matching_attempts (1000) */
  int n_non;     /* num_masked_non_matches_per_match (100) */
  int dense_loss; /* 1: reserve the [B, cells, cells] coefficient matrix of the dense descriptor loss
                     (model.dense_loss.enable, utils/utils.py:779-893) in the workspace */
} ssp_config;

/* Device buffers bound once after create (all float32 unless noted).
 * params/grads/adam_m/adam_v: [n_params + 3]  (net.parameters() order = state_dict order without
 * buffers, OIHW conv weights; the 3 trailing floats are MultiTaskLoss.eta).
 * bn_running: [2 * n_bn_channels] = all running_mean (layer order) then all running_var.
 * num_batches_tracked: int64 [n_bn_layers]. */
typedef struct {
  float* params_dev;
  float* grads_dev;
  float* adam_m_dev;
  float* adam_v_dev;
  float* bn_running_dev;
  int64_t* num_batches_tracked_dev;
  void* workspace_dev;
  size_t workspace_bytes;
} ssp_buffers;

/* One micro-batch of pairs (Train_model_heatmap_all.py:212-251 `sample`). NCHW with C==1.
 * warped_image_dev == NULL selects the SINGLE-VIEW step of `data.warped_pair.enable: false` (Train_model_heatmap_all.py:207,
 * 237-262, 330-332; configs/magicpoint_shapes_pair.yaml): one forward, detector (+ segmentation) loss of the image only,
 * loss_det_warp = loss_sem_warp = 0; the other warped_* pointers and homographies_dev are then ignored and lambda_loss must
 * be 0 (the reference asserts "need a pair of images"). */
typedef struct {
  int batch;
  const float* image_dev;             /* [B,1,H,W] */
  const float* warped_image_dev;      /* [B,1,H,W], or NULL: single-view step */
  const float* labels_dev;            /* [B,1,H,W] labels_2D(_gaussian) */
  const float* warped_labels_dev;     /* [B,1,H,W] */
  const float* valid_mask_dev;        /* [B,1,H,W] */
  const float* warped_valid_mask_dev; /* [B,1,H,W] */
  const float* homographies_dev;      /* [B,3,3] normalised coords, image -> warped */
  const int64_t* semantic_dev;        /* [B,H,W] or NULL */
  const int64_t* warped_semantic_dev; /* [B,H,W] or NULL */
  /* sparse-loss indices, either given (parity mode) or sampled on device when match_a_dev==NULL */
  const int32_t* match_a_dev;    /* [B,n_match] cell index u+v*Wc in image a */
  const int32_t* match_b_dev;    /* [B,n_match] cell index in image b */
  const int32_t* nonmatch_b_dev; /* [B,n_match*n_non] cell index in image b */
  uint64_t seed;                 /* device sampler seed (used when match_a_dev == NULL) */
  float lambda_loss;             /* model.lambda_loss; 0 disables the descriptor loss */
  float lamda_d;                 /* sparse_loss.params.lamda_d */
  int multi_task;                /* model.multi_task_loss */
  int train;                     /* 1: accumulate gradients; 0: forward + losses only */
  /* dense descriptor loss instead of the sparse one (Train_model_heatmap_all.py:131-137,348-350): no indices needed.
   * dense_lamda_d: descriptor_loss's `lamda_d` (250: the shipped configs spell it `lambda_d`, which the reference
   * swallows in **config); descriptor_dist: dense_loss.params.descriptor_dist (4) */
  int dense_loss;
  float dense_lamda_d;
  float descriptor_dist;
  /* optional [B,3,3]: the CELL-space homographies scale_homography_torch(H, (Hc, Wc)) (utils/homographies.py:270-276)
   * computed by the caller on the host with the reference's own fp32 op sequence; used by the captured device sampler
   * (ssp_pair_step_graph) - see ssp_sample_indices_cell */
  const float* cell_homographies_dev;
  /* sparse_loss.params.method / dist (sparse_loss.py:76-77, pixelwise_contrastive_loss.py:140): 0 / 0 = "2d" / "cos", what every
   * shipped config selects; method 1 = "1d" (matches by index_select at the cell), dist 1 = "euclidean" (squared distance of the
   * matches, (max(0, ||a - b|| - 0.2))^2 of the non-matches - nearly every non-match of unit descriptors is then a hard one) */
  int sparse_method;
  int sparse_dist;
} ssp_pair_inputs;

/* indices into the float scalars[SSP_N_SCALARS] array filled by ssp_pair_step (the reference's
 * scalar_dict, Train_model_heatmap_all.py:415-441) */
enum {
  SSP_S_LOSS = 0, SSP_S_LOSS_DET, SSP_S_LOSS_DET_WARP, SSP_S_LOSS_DESC, SSP_S_LOSS_SEM, SSP_S_LOSS_SEM_WARP,
  SSP_S_POSITIVE_DIST, SSP_S_NEGATIVE_DIST, SSP_S_ETA_DET, SSP_S_ETA_DESC, SSP_S_ETA_SEM,
  SSP_N_SCALARS = 16
};

const char* ssp_last_error(void);
/* sha256 of the library's source files (csrc/*.hip, csrc/*.hip.h, include/ssp_hip.h) at build time: hipbuild.source_id() */
const char* ssp_build_id(void);
/* Bit-reproducible accumulation (process-wide; also SSP_DETERMINISTIC=1 in the environment): floating-point atomics of the path
 * become order-independent - fp64 accumulators take addends rounded to a fixed quantum (exact sums), fp32 scatter targets go
 * through 64-bit fixed-point shadows (csrc/det.hip.h).  Switch it BEFORE ssp_bind: the shadows are allocated there.  The
 * reference has no counterpart (torch.use_deterministic_algorithms is never set: train4.py). */
int ssp_set_deterministic(int on);
int ssp_get_deterministic(void);
/* Measurement aid (no counterpart in the reference): the shader clock in MHz that the device sustains while every CU runs
 * fp32 matrix-core instructions for ~`ms` milliseconds on `stream` (blocking).  bench.py reports it before and after the timed
 * region: the boxes of a pool differ in the clock their power controller grants. */
int ssp_clock_probe(float ms, double* mhz_out, void* stream);
int ssp_create(const ssp_config* cfg, ssp_handle** out);
void ssp_destroy(ssp_handle* h);
size_t ssp_param_count(const ssp_handle* h);       /* net parameters (without eta) */
size_t ssp_bn_channel_count(const ssp_handle* h);  /* sum of C over BatchNorm layers */
int ssp_bn_layer_count(const ssp_handle* h);
size_t ssp_workspace_bytes(const ssp_handle* h);
int ssp_bind(ssp_handle* h, const ssp_buffers* b, void* stream);

/* forward of one batch into activation slot 0/1; outputs (may be NULL) are NCHW like the reference:
 * semi [N,65,H/8,W/8], desc [N,256,H/8,W/8], sem [N,n_classes,H,W]. train: 1 = batch statistics +
 * running-stat update (module default), 0 = eval() (running statistics). */
int ssp_forward(ssp_handle* h, int slot, const float* x_dev, int n, int height, int width, int train,
                float* semi_dev, float* desc_dev, float* sem_dev, void* stream);
/* backward of slot given dL/d(outputs) in NCHW (NULL = zero); ACCUMULATES into grads_dev. */
int ssp_backward(ssp_handle* h, int slot, const float* dsemi_dev, const float* ddesc_dev, const float* dsem_dev,
                 void* stream);
int ssp_zero_grad(ssp_handle* h, void* stream);
int ssp_pair_step(ssp_handle* h, const ssp_pair_inputs* in, float* scalars_dev, void* stream);
int ssp_adam_step(ssp_handle* h, float lr, int step, void* stream);
/* the same Adam step on grads * grad_scale (data parallel: 1 / world_size after an all-reduce SUM; grads_dev is left
 * untouched, so gradient accumulation over micro-batches keeps working) */
int ssp_adam_step_scaled(ssp_handle* h, float lr, int step, float grad_scale, void* stream);

/* ---- data-parallel overlap ("all-reduce overlapped with encoder backward") ------------------
 * ssp_pair_step_phase: phase 0 = ssp_pair_step.  Phase 1 runs the step up to the point where every gradient from
 * ssp_grad_early_offset(h) to the end of the flat vector (encoder layers >= 2, all heads, eta: 97.7 % of the bytes) is
 * FINAL; phase 2 runs the rest of the backward pass (the two 240x320 layers, 40 % of the backward time).  Between the
 * two calls the host starts the all-reduce of the early bucket on another stream; it overlaps with phase 2. */
int ssp_pair_step_phase(ssp_handle* h, const ssp_pair_inputs* in, float* scalars_dev, int phase, void* stream);
size_t ssp_grad_early_offset(const ssp_handle* h); /* first float of the early-final gradient bucket */

/* ---- hipGraph form of the pair step (north star: "one graph per image pair") --------------------------------------
 * The first call with a given (inputs, phase, algorithm) signature captures the launches of ssp_pair_step_phase into a
 * hipGraph on `stream` (must not be the default stream); later calls replay it with ONE hipGraphLaunch.  With
 * sample_indices != 0 the device index sampler (ssp_sample_indices into in->match_a/match_b/nonmatch_b_dev, which must
 * be caller-owned buffers of the usual sizes) is part of the graph; its seed `in->seed` is kept in device memory and may
 * change from call to call.  Everything else of `in` is part of the signature.  Up to 16 graphs are cached per handle;
 * ssp_bind drops them.  ssp_profile_enable must be off (hipEvents cannot be recorded into the capture). */
int ssp_pair_step_graph(ssp_handle* h, const ssp_pair_inputs* in, float* scalars_dev, int phase, int sample_indices,
                        void* stream);
int ssp_sample_indices(ssp_handle* h, const float* homographies_dev, int batch, uint64_t seed, int32_t* match_a_dev,
                       int32_t* match_b_dev, int32_t* nonmatch_b_dev, void* stream);
/* Index parity: every kernel that warps integer coordinates takes the homography in the space of those coordinates.  With
 * the *_cell / *_px entry points the caller passes T^-1 H T computed on the HOST exactly like the reference
 * (torch.inverse(trans) @ H @ trans: scale_homography_torch / homography_scaling_torch) and the device applies the
 * reference's own fp32 operation order (fma chain of torch's CPU matmul, correctly rounded division, round half to even):
 * warped integer indices are then bit-identical to the reference's.  The plain entry points derive T^-1 H T analytically
 * on the device; coordinates within ~1e-4 of a .5 boundary may then round the other way. */
int ssp_sample_indices_cell(ssp_handle* h, const float* cell_homographies_dev, int batch, uint64_t seed, int32_t* match_a_dev,
                            int32_t* match_b_dev, int32_t* nonmatch_b_dev, void* stream);

/* timing hook for bench.py: when enabled, every launch of the tagged kernel family is bracketed by
 * hipEvents on `stream`; ssp_profile_read returns accumulated milliseconds, launches and FLOPs. */
enum { SSP_PROF_NONE = 0, SSP_PROF_CONV3X3_FWD = 1, SSP_PROF_CONV3X3_DGRAD = 2, SSP_PROF_CONV3X3_WGRAD = 3,
       SSP_PROF_CONV_BIG_FWD = 4, SSP_PROF_CONV3X3_ALL = 5 /* 3x3 forward + data-gradient launches */,
       SSP_PROF_CONV3X3_EVERY = 6 /* 3x3 forward + data-gradient + weight-gradient launches */ };
int ssp_profile_enable(ssp_handle* h, int family);
int ssp_profile_read(ssp_handle* h, double* ms, int64_t* launches, double* flops, double* bytes);
/* The same measurement split by the KERNEL that ran each tagged launch (bench.py's per-kernel roofline entries). */
enum { SSP_PROF_K_CONV_WINO4 = 0 /* conv_wino4_kernel, Winograd F(4x4,3x3) */, SSP_PROF_K_CONV_WINO_PIPE = 1, SSP_PROF_K_CONV_WINO_P2 = 2,
       SSP_PROF_K_WGRAD_WINO = 3 /* wgrad_wino_kernel, F(3x3,2x2) */, SSP_PROF_K_WGRAD_WINO4 = 4 /* wgrad_wino4_kernel, F(3x3,4x4) */,
       SSP_PROF_K_OTHER = 5 /* direct implicit GEMM, bf16-operand Winograd kernels */,
       SSP_PROF_K_CONV_BF16 = 6 /* conv_bf16_kernel (forward + data gradient of the bf16 path) */,
       SSP_PROF_K_WGRAD_BF16 = 7 /* wgrad_bf16_kernel */, SSP_PROF_K_COUNT = 8 };
/* Suspends (paused != 0) / resumes the bracketing without resetting the counters: bench.py brackets every n-th step of the
 * timed region only (the event records of ~30 launches per step cost ~1.7 % of the step when every step carries them). */
int ssp_profile_pause(ssp_handle* h, int paused);
int ssp_profile_read_kernel(ssp_handle* h, int kernel, double* ms, int64_t* launches, double* flops, double* executed_flops,
                            double* bytes);
/* FLOPs the tagged launches since ssp_profile_enable EXECUTED on the matrix cores (ssp_profile_read's `flops` are the
 * algorithmic, direct-convolution FLOPs): x 1/4 for a Winograd F(4x4,3x3) launch, x 16/36 for F(2x2,3x3), x 1 otherwise. */
int ssp_profile_read_executed(ssp_handle* h, double* executed_flops);

/* ---- operator-level entry points (used by the unit parity tests; same kernels as above) ---- */
/* 3x3 / 1x1 convolution, NHWC fp32, stride 1, "same" padding, weights OIHW (reference layout).
 * in_mode: 0 raw input, 1 input = relu(in*scale+shift), 2 = maxpool2(relu(in*scale+shift)) where `in`
 * is [N,2H,2W,Cin]. stats_dev (double [SSP_NREP][2*Cout]: partial sum, sumsq replicas; zeroed by the caller)
 * may be NULL. */
int ssp_op_conv(const float* in_dev, const float* w_oihw_dev, const float* bias_dev, float* out_dev, int n, int h,
                int w, int cin, int cout, int ksize, int in_mode, const float* in_scale_dev,
                const float* in_shift_dev, double* stats_dev, int transpose_flip, void* workspace_dev,
                size_t workspace_bytes, void* stream);
int ssp_op_conv_wgrad(const float* in_dev, const float* dout_dev, float* dw_oihw_dev, int n, int h, int w, int cin,
                      int cout, int ksize, int in_mode, const float* in_scale_dev, const float* in_shift_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- bf16 path (conv algorithm 12, BASELINE configs[3]): bf16 NHWC activations in HBM, v_mfma_f32_32x32x16_bf16 ----
 * Convolution of models/unet_parts.py:14-21 as a direct implicit GEMM (csrc/conv_bf16.hip.h).  in: bf16 (fp32 when in_f32)
 * NHWC [n,h,w,cin]; w: OIHW fp32 (rounded to bf16 when packed; transpose_flip: O = cin, the data-gradient convolution);
 * in_mode 1: operand = bf16(relu(in * scale + shift)); out: bf16 (fp32 when out_f32) NHWC [n,h,w,cout] = round(acc + bias);
 * stats (optional, double [SSP_NREP][2 cout], zeroed by the caller): sum / sum of squares of the STORED output;
 * pool_out (optional, bf16 [n,h/2,w/2,cout]): per-channel max (pool_gamma >= 0) / min (< 0) of every 2x2 window of out.
 * workspace: >= ceil(cout/64) * ceil(cin/32) * ksize^2 * 4096 bytes (the packed bf16 weight image). */
int ssp_op_conv_bf16(const void* in_dev, const float* w_oihw_dev, const float* bias_dev, void* out_dev, int n, int h, int w,
                     int cin, int cout, int ksize, int in_mode, const float* in_scale_dev, const float* in_shift_dev,
                     double* stats_dev, int transpose_flip, int in_f32, int out_f32, void* pool_out_dev,
                     const float* pool_gamma_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Weight gradient of the same convolution (csrc/wgrad_bf16.hip.h): x bf16 NHWC [n,h,w,cin] (in_mode 1: operand =
 * bf16(relu(x * scale + shift))), dy bf16 (fp32 when dy_f32, rounded to bf16 on load) NHWC [n,h,w,cout]; the fp32 OIHW gradient is
 * ACCUMULATED into dw_oihw_dev.  workspace: partial slabs, >= ceil(cin/64) * ceil(cout/64) * ksize^2 * 16 KiB (more = more
 * workgroups, up to 2 per CU). */
int ssp_op_conv_wgrad_bf16(const void* x_dev, const void* dy_dev, float* dw_oihw_dev, int n, int h, int w, int cin, int cout,
                           int ksize, int in_mode, const float* in_scale_dev, const float* in_shift_dev, int dy_f32,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* ssp_op_bn_bwd_strided on bf16 tensors (y, dout, dy: bf16 NHWC, channel stride cs; ReLU layers only). */
int ssp_op_bn_bwd_bf16(const void* y_dev, const void* dout_dev, const float* gamma_dev, const float* stats4_dev, void* dy_dev,
                       float* dgamma_dev, float* dbeta_dev, float* dbias_dev, double* sums_dev, int n, int h, int w, int c, int cs,
                       int relu, int pool, void* stream);

/* labels2Dto3D (utils/utils.py:408-440, add_dustbin=True) -> target [B,65,H/8,W/8] NCHW and getMasks
 * (Train_model_frontend_all.py:373-386) -> cellmask [B,H/8,W/8]; either pair of pointers may be NULL. */
int ssp_op_labels(const float* labels2d_dev, const float* mask2d_dev, float* target_dev, float* cellmask_dev, int b,
                  int h, int w, void* stream);

/* detector_loss (Train_model_heatmap_all.py:155-179, softmax branch) as an operator: semi NHWC [b][h/8*w/8][cs] (65 logits,
 * channel stride cs >= 65), labels2d / mask2d [b,1,h,w] -> loss_dev[0] and (optional) d loss / d semi in the same layout.
 * scratch: 64 KiB + 4 bytes per cell. */
int ssp_op_detector_loss(const float* semi_nhwc_dev, int cs, const float* labels2d_dev, const float* mask2d_dev, int b, int h,
                         int w, void* scratch_dev, size_t scratch_bytes, float* loss_dev, float* dsemi_nhwc_dev, void* stream);

/* sem_loss (Train_model_heatmap_all.py:181-193: CrossEntropyLoss(ignore_index = n_classes) of the bilinear upsample,
 * align_corners=False, models/SuperPointNet_gauss2_ssmall.py:87-91) as an operator, without the [b,n_classes,h,w] logits: convSout NHWC
 * [b][h/8*w/8][cs] (n_classes logits, channel stride cs >= n_classes), labels int64 [b,h,w] (values outside [0, n_classes) are
 * ignored) -> loss_dev[0] = mean NLL over the counted pixels and (optional, OVERWRITTEN) d loss / d convSout in the same layout.
 * algo: 0 = the kernel the training step would take, 1 = pixels-then-classes lanes (any h, w; <= 192 classes), 2 = (x, class) lanes
 * (<= 144 classes).  scratch: 64 KiB. */
int ssp_op_sem_loss(const float* sout_nhwc_dev, int cs, const int64_t* labels_dev, int b, int h, int w, int n_classes, int algo,
                    void* scratch_dev, size_t scratch_bytes, float* loss_dev, float* dsout_nhwc_dev, void* stream);

/* Segmentation head read-out: class map and confusion matrix from convSout NHWC [b][h/8*w/8][cs] (n_classes
 * logits, channel stride cs >= n_classes, 1 <= n_classes <= 256) without the [b,n_classes,h,w] logits: bilinear upsample x8
 * (align_corners=False, models/SuperPointNet_gauss2_ssmall.py:87-91) + argmax over the classes (ties: the lowest class index).
 * pred_dev (nullable): uint8 [b,h,w].  confusion_dev (nullable; needs labels_dev): int64 [n_classes][n_classes], row = label,
 * column = prediction, ACCUMULATED (+=; the caller zeroes it) - labels int64 [b,h,w], values outside [0, n_classes) are ignored
 * (ssp_op_sem_loss).  h and w must be multiples of 8.
 * ssp_sem_predict: the same from the logits the last forward / pair step left in `slot` (like ssp_detector_heatmap). */
int ssp_op_sem_predict(const float* sout_nhwc_dev, int cs, const int64_t* labels_dev, int b, int h, int w, int n_classes,
                       uint8_t* pred_dev, int64_t* confusion_dev, void* stream);
int ssp_sem_predict(ssp_handle* h, int slot, const int64_t* labels_dev, uint8_t* pred_dev, int64_t* confusion_dev, void* stream);

/* ---- pair construction on the device (dataset side of the reference, datasets/Coco.py:341-392) ----
 * ssp_op_warp_image : inv_warp_image_batch (utils/utils.py:347-385): out[p] = sample(img, inv_h * p), p on the
 *                     linspace(-1,1) grid, zeros padding, align_corners=True; nearest != 0 selects mode="nearest".
 * ssp_op_erode      : the erosion of compute_valid_mask (utils/utils.py:737-740): MORPH_ELLIPSE(2r,2r), anchor (r,r).
 * ssp_op_warp_labels: warpLabels (datasets/data_tools.py:37-63) on a keypoint MAP: every non-zero pixel (x,y) is warped
 *                     with T^-1 h T (utils/utils.py:297-300), kept if inside, rounded half-to-even, scattered as 1. */
int ssp_op_warp_image(const float* img_dev, const float* inv_h_dev, float* out_dev, int b, int h, int w, int nearest,
                      void* stream);
int ssp_op_erode(const float* mask_dev, float* out_dev, int b, int h, int w, int radius, void* stream);
int ssp_op_warp_labels(const float* labels_dev, const float* h_dev, float* out_dev, int b, int h, int w, void* stream);
int ssp_op_warp_labels_px(const float* labels_dev, const float* hpx_dev, float* out_dev, int b, int h, int w, void* stream);

/* Pair construction for real data:
 * ssp_op_sample_homographies: sample_homography_np (utils/homographies.py:12-141) with the keys of
 *     `warped_pair.params` + the inversion of datasets/Coco.py:342-350, counter-based device RNG (distribution-level
 *     equivalent of the numpy / scipy streams); h_dev = `homographies` (image -> warped), inv_h_dev = `inv_homographies`.
 * ssp_op_warp_labels_full : warpLabels(..., bilinear=True) (datasets/data_tools.py:37-63) on a keypoint map:
 *     labels [b,1,h,w], res [b,2,h,w] (warped - round(warped) at the rounded position), labels_bi [b,1,h,w]
 *     (get_labels_bi :26-34); any output may be NULL.  Where several key points claim one pixel the winner does not depend on
 *     thread order: points count in row-major order of the map (torch.nonzero); labels / res keep the LAST point that rounds to
 *     the pixel; labels_bi keeps the later of the four neighbour lists (x,y), (x,y+1), (x+1,y), (x+1,y+1) that the reference
 *     concatenates before its single scatter, and within a list the later point.  Two passes (integer atomicMax of a priority
 *     key into the zero-filled maps, then the winner's value in place): no extra memory; h * w < 2^29 or the call is refused.
 * ssp_op_sem_finalize     : datasets/Coco_sem.py:447-448: float class map -> int64, invalid pixels -> n_classes. */
typedef struct ssp_homography_params {
  int32_t perspective, scaling, rotation, translation, allow_artifacts;
  int32_t n_scales, n_angles; /* 5, 25 */
  float scaling_amplitude, perspective_amplitude_x, perspective_amplitude_y, patch_ratio, max_angle, translation_overflow;
} ssp_homography_params;
int ssp_op_sample_homographies(uint64_t seed, const ssp_homography_params* p, int b, float* h_dev, float* inv_h_dev,
                               void* stream);
int ssp_op_warp_labels_full(const float* labels_dev, const float* h_dev, float* labels_out_dev, float* res_out_dev,
                            float* bi_out_dev, int b, int h, int w, void* stream);
int ssp_op_warp_labels_full_px(const float* labels_dev, const float* hpx_dev, float* labels_out_dev, float* res_out_dev,
                               float* bi_out_dev, int b, int h, int w, void* stream);
/* ssp_op_label_quantize : the `*_gaussian` label maps of datasets/Coco.py:378,400 (ImgAugTransform with GaussianBlur sigma 0.2,
 * utils/photometric.py:59-78): uint8 quantisation floor(x * 255) / 255; the sigma-0.2 blur itself is the identity on 8 bits. */
int ssp_op_label_quantize(const float* in_dev, float* out_dev, size_t n, void* stream);
int ssp_op_sem_finalize(const float* sem_warped_dev, const float* valid_dev, int64_t* out_dev, size_t n, int n_classes,
                        void* stream);

/* ---- photometric augmentation of the training images (utils/photometric.py) ----
 * ssp_op_photometric_draw  : every random decision of ImgAugTransform + customizedTransform.additive_shade for b images of
 *     h x w, from ONE seed (counter-based device RNG; the stream differs from numpy's by construction): one row of
 *     SSP_PHOTO_DRAW_STRIDE floats per image, laid out as
 *       [SSP_PHOTO_BRIGHTNESS]    integer delta in [-max_abs_change, +max_abs_change]          (0 when off)
 *       [SSP_PHOTO_CONTRAST]      factor, uniform in strength_range                             (1 when off)
 *       [SSP_PHOTO_SIGMA]         noise sigma on the 0..255 scale, uniform in stddev_range       (0 when off)
 *       [SSP_PHOTO_IMPULSE_P]     impulse probability, uniform in prob_range                     (0 when off)
 *       [SSP_PHOTO_BLUR_FLAG]     1 with probability 1/2, then 9 row-major 3x3 weights (sum 1) at [SSP_PHOTO_BLUR_W]
 *       [SSP_PHOTO_ELLIPSES]      SSP_PHOTO_MAX_ELLIPSES x (cx, cy, ax, ay, angle in degrees); ax < 0 ends the list
 *       [SSP_PHOTO_TRANSPARENCY]  shade transparency
 *       [SSP_PHOTO_KSIZE]         odd shade kernel size                                          (0 when off)
 *       [SSP_PHOTO_KEY]           64-bit key of the per-pixel noise as 4 floats of 16 bits each, low bits first
 *     A neutral value switches its stage off in apply.  Enable fields are COUNTS as the reference's parser produces them
 *     (lib.photometric_params_from_config); a count above 1 (the max_kernel_size quirk) is refused here.
 * ssp_op_photometric_apply : pure function of the image and its row: img / out float [b,1,h,w] in [0, 1] (out may not alias
 *     img).  Stage order, 8-bit semantics and the restated rounding choices: csrc/photo_kernels.hip.h.  Kernel sizes up to
 *     SSP_PHOTO_MAX_KSIZE; h <= 744 (the shade keeps a full-height strip in LDS). */
enum { SSP_PHOTO_MAX_ELLIPSES = 32, SSP_PHOTO_MAX_KSIZE = 351 };
enum { SSP_PHOTO_BRIGHTNESS = 0, SSP_PHOTO_CONTRAST = 1, SSP_PHOTO_SIGMA = 2, SSP_PHOTO_IMPULSE_P = 3, SSP_PHOTO_BLUR_FLAG = 4,
       SSP_PHOTO_BLUR_W = 5, SSP_PHOTO_ELLIPSES = 14, SSP_PHOTO_TRANSPARENCY = 174, SSP_PHOTO_KSIZE = 175, SSP_PHOTO_KEY = 176,
       SSP_PHOTO_DRAW_STRIDE = 180 };
typedef struct ssp_photometric_params {
  uint32_t struct_size; /* sizeof(ssp_photometric_params) of the caller: an unknown size is an error */
  int32_t random_brightness, random_contrast, additive_gaussian_noise, additive_speckle_noise, motion_blur, additive_shade;
  int32_t brightness_max_abs_change;
  float contrast_lo, contrast_hi;         /* random_contrast.strength_range */
  float noise_std_lo, noise_std_hi;       /* additive_gaussian_noise.stddev_range */
  float impulse_prob_lo, impulse_prob_hi; /* additive_speckle_noise.prob_range */
  int32_t shade_nb_ellipses;              /* additive_shade.nb_ellipses (20), <= SSP_PHOTO_MAX_ELLIPSES */
  float shade_transparency_lo, shade_transparency_hi;
  int32_t shade_kernel_lo, shade_kernel_hi; /* kernel_size_range: integer in [lo, hi), made odd by adding 1 */
} ssp_photometric_params;
int ssp_op_photometric_draw(uint64_t seed, const ssp_photometric_params* p, int b, int h, int w, float* draws_dev, void* stream);
int ssp_op_photometric_apply(const float* img_dev, const float* draws_dev, float* out_dev, int b, int h, int w, void* stream);

/* ---- Synthetic Shapes on the device (datasets/synthetic_dataset.py, SyntheticDataset_gaussian.py:125-147) ----
 * ssp_op_shapes_draw   : every random decision of generate_background + one of the nine primitives for b images from one seed:
 *     one scene table row of SSP_SHAPES_ROW int32 words per image (float fields are stored by their bits):
 *       [SSP_SHAPES_PRIM]    primitive 0..8 in the order of `weights`
 *       [SSP_SHAPES_THR]     threshold of the background noise; [SSP_SHAPES_KEY], [+1] its 64-bit noise key (low, high)
 *       [SSP_SHAPES_KSIZE]   box-kernel size of the background; [SSP_SHAPES_NBLOBS] blob count
 *       [SSP_SHAPES_MEAN0]   int(mean) of the thresholded noise; [SSP_SHAPES_MEAN] int(mean) of noise + blobs (the
 *                            `background_color` of every get_random_color of the primitive)
 *       [SSP_SHAPES_NCMDS], [SSP_SHAPES_NPOINTS], [SSP_SHAPES_NVERTS], [SSP_SHAPES_NTEX]  counts
 *       [SSP_SHAPES_BLOBS]   SSP_SHAPES_MAX_BLOBS x (x, y, radius, colour)
 *       [SSP_SHAPES_CMDS]    SSP_SHAPES_MAX_CMDS x 12: (type, colour, bbox x0, y0, x1, y1 clipped to the image, 6 arguments), painted in order:
 *                              1 polygon (first vertex, vertex count)        2 segment (x1, y1, x2, y2, thickness)
 *                              3 ellipse (cx, cy, cos, sin, 1/ax^2, 1/ay^2)  4 textured polygon (first vertex, count, texture)
 *                              5 uniform noise over the image (key low, high)
 *       [SSP_SHAPES_VERTS]   SSP_SHAPES_MAX_VERTS x (x, y); in an ellipse image word c holds max(ax, ay) of command c instead
 *       [SSP_SHAPES_TEX]     SSP_SHAPES_MAX_TEX x 12: (base colour, box-kernel size, key low, key high, centre x, y, radius (float),
 *                              bbox x0, y0, x1, y1, 0): the blobs of a texture are a function of its key
 *       [SSP_SHAPES_POINTS]  SSP_SHAPES_MAX_POINTS x (x, y) float at generation resolution
 * ssp_op_shapes_render : pure function of the table and the parameters: uint8 image [b,1,out_h,out_w], key points scaled to
 *     (out_h, out_w) as float [b, SSP_SHAPES_MAX_POINTS, 2] (x, y; unused slots zero) and their counts int32 [b].
 *     workspace_dev: ssp_shapes_workspace_bytes(p, b) bytes. */
enum { SSP_SHAPES_N_PRIMITIVES = 9, SSP_SHAPES_MAX_BLOBS = 128, SSP_SHAPES_MAX_CMDS = 64, SSP_SHAPES_MAX_VERTS = 256, SSP_SHAPES_MAX_TEX = 32,
       SSP_SHAPES_MAX_POINTS = 256, SSP_SHAPES_MAX_BLUR = 63, SSP_SHAPES_MAX_TEX_BLOBS = 4096 };
enum { SSP_SHAPES_PRIM = 0, SSP_SHAPES_THR = 1, SSP_SHAPES_KEY = 2, SSP_SHAPES_KSIZE = 4, SSP_SHAPES_NBLOBS = 5, SSP_SHAPES_MEAN0 = 6,
       SSP_SHAPES_MEAN = 7, SSP_SHAPES_NCMDS = 8, SSP_SHAPES_NPOINTS = 9, SSP_SHAPES_NVERTS = 10, SSP_SHAPES_NTEX = 11, SSP_SHAPES_BLOBS = 16,
       SSP_SHAPES_CMDS = 528, SSP_SHAPES_VERTS = 1296, SSP_SHAPES_TEX = 1808, SSP_SHAPES_POINTS = 2192, SSP_SHAPES_ROW = 2704 };
typedef struct ssp_shapes_params {
  uint32_t struct_size; /* sizeof(ssp_shapes_params) of the caller: an unknown size is an error */
  int32_t gen_h, gen_w;   /* generation.image_size */
  int32_t out_h, out_w;   /* preprocessing.resize */
  int32_t blur_size;      /* preprocessing.blur_size: odd, <= SSP_SHAPES_MAX_BLUR (0 or 1: no blur) */
  float weights[9];       /* truncate share of draw_lines, draw_polygon, draw_multiple_polygons, draw_ellipses, draw_star,
                             draw_checkerboard, draw_stripes, draw_cube, gaussian_noise (0 = primitive not listed) */
  int32_t bg_nb_blobs, bg_min_kernel, bg_max_kernel;
  float bg_min_rad_ratio, bg_max_rad_ratio;
  int32_t lines_nb_lines, polygon_max_sides, multi_max_sides, multi_nb_polygons, multi_nb_blobs, multi_kernel_lo, multi_kernel_hi;
  int32_t ellipses_nb, star_nb_branches, checker_max_rows, checker_max_cols, stripes_max_nb_cols;
  float checker_transform[2], stripes_transform[2], stripes_min_width_ratio;
  float cube_min_size_ratio, cube_scale[2], cube_trans[2];
  float resize_scale_y, resize_scale_x; /* float32(gen / out): the caller computes the quotient */
  float gauss_w[63];      /* the blur_size normalised Gaussian weights (the caller computes them: lib.shapes_gaussian_weights) */
} ssp_shapes_params;
size_t ssp_shapes_workspace_bytes(const ssp_shapes_params* p, int b);
int ssp_op_shapes_draw(uint64_t seed, const ssp_shapes_params* p, int b, int32_t* table_dev, void* stream);
int ssp_op_shapes_render(const int32_t* table_dev, const ssp_shapes_params* p, int b, void* workspace_dev, uint8_t* image_dev,
                         float* points_dev, int32_t* counts_dev, void* stream);
/* The single-view feed (SyntheticDataset_gaussian.py:342-351, 450-472): float key points [b, stride, 2] (x, y) with counts [b] ->
 * filter_points, warp with the pixel-space homographies hpx_dev [b,3,3] (NULL: no warp), filter_points, round half to even,
 * clamp to (w - 1, h - 1), scatter 1 into labels_dev [b,1,h,w] (zero-filled here). */
int ssp_op_warp_points_scatter(const float* points_dev, const int32_t* counts_dev, const float* hpx_dev, float* labels_dev, int b,
                               int stride, int h, int w, void* stream);

/* ---- homography-adaptation export (export.py:192-352) ------------------------------
 * One image = n_views warped copies that form ONE BatchNorm batch (the reference leaves the net in train mode,
 * models/model_wrap.py:120).  ssp_export_points replaces the body of the export loop (export.py:296-309):
 *   fe.run(img, onlyHeatmap=True)   -> forward (detector head) + flattenDetection (utils/utils.py:515-560)
 *   combine_heatmap                 -> export.py:49-60; unwarp_h = the matrices the reference passes as
 *                                      `inv_homographies`, i.e. sample["homographies"] (export.py:281-284 swaps the keys)
 *   fe.getPtsFromHeatmap            -> models/model_wrap.py:266-293 (threshold, nms_fast :129-192, border removal)
 *   fe.soft_argmax_points           -> models/model_wrap.py:212-249 (when subpixel != 0)
 *   pts[:top_k]                     -> export.py:303-309
 * pts_dev[k]: [ssp_export_max_points][5] rows (x, y, confidence, sx, sy), descending confidence; the reference's
 * float64 point is (x + sx - 2, y + sy - 2, confidence) (sx = sy = 2 when subpixel == 0); count_dev[k]: rows written.
 * Equal confidences are ordered by the lower row-major pixel index (numpy's quicksort order is unspecified there).
 * workspace_dev[k]: ssp_export_workspace_bytes(p) bytes per image.  heatmap_out_dev (or its entries) may be NULL. */
typedef struct ssp_export_params {
  int32_t n_views;       /* data.homography_adaptation.num */
  int32_t height, width; /* multiples of 8 */
  float conf_thresh;     /* model.detection_threshold (compared in fp32, as numpy does) */
  int32_t nms_dist;      /* model.nms */
  int32_t border_remove; /* SuperPointFrontend_torch.border_remove = 4 (models/model_wrap.py:70) */
  int32_t top_k;         /* model.top_k, 0 = all */
  int32_t subpixel;      /* model.subpixel.enable */
} ssp_export_params;

size_t ssp_export_workspace_bytes(const ssp_export_params* p);
int ssp_export_max_points(const ssp_export_params* p);
int ssp_export_points(ssp_handle* h, const ssp_export_params* p, int n_images, const float* const* views_dev,
                      const float* const* masks_dev, const float* const* unwarp_h_dev, void* const* workspace_dev,
                      float* const* heatmap_out_dev, float* const* pts_dev, int32_t* const* count_dev, void* stream);

/* the stages as operators (parity tests):
 * ssp_op_homoadapt_views  : datasets/Coco.py:279-288: n warped copies of ONE [h,w] image (inv_warp_image_batch,
 *                           bilinear) and the nearest-warped all-ones masks (compute_valid_mask before erosion)
 * ssp_op_flatten_detection: flattenDetection on a public NCHW `semi` [n,65,hc,wc] (times mask [n,8hc,8wc] if given)
 * ssp_op_combine_heatmap  : combine_heatmap on heat = heatmap*mask and mask, both [n,h,w]
 * ssp_op_heatmap_points   : getPtsFromHeatmap + soft_argmax_points + top-k on one [h,w] heatmap
 * ssp_op_soft_argmax_points: soft_argmax_points for explicit points xy [n,2] (x, y; truncated to int) -> (sx, sy) [n,2] */
int ssp_op_homoadapt_views(const float* img_dev, const float* inv_h_dev, float* views_dev, float* masks_dev, int n, int h,
                           int w, void* stream);
int ssp_op_flatten_detection(const float* semi_nchw_dev, const float* mask_dev, float* heat_dev, int n, int hc, int wc,
                             void* stream);
int ssp_op_combine_heatmap(const float* heat_dev, const float* mask_dev, const float* unwarp_h_dev, float* out_dev, int n,
                           int h, int w, void* stream);
int ssp_op_heatmap_points(const float* heat_dev, const ssp_export_params* p, void* workspace_dev, float* pts_dev,
                          int32_t* count_dev, void* stream);
int ssp_op_soft_argmax_points(const float* heat_dev, const float* xy_dev, float* out_dev, int n, int h, int w,
                              void* stream);

/* ---- logging branch of train_val_sample (Train_model_heatmap_all.py:447-568) ------
 * ssp_detector_heatmap: get_heatmap (Train_model_frontend_all.py:664-669) = flattenDetection of the detector logits
 *                       of the last forward / pair step in `slot` (0 = image, 1 = warped image) -> heat [n,h,w].
 * ssp_op_heatmap_nms  : heatmap_to_nms / heatmap_nms (Train_model_heatmap_all.py:574-587,693-707) for n_maps heatmaps
 *                       [n_maps,h,w] (p->top_k / subpixel / n_views ignored) and batch_precision_recall's terms
 *                       (:614-622, utils/utils.py:929-941): nms_map_dev [n_maps,h,w] 0/1 (optional),
 *                       pr_dev [n_maps][2] = (precision, recall) against labels_dev [n_maps,h,w] (both optional). */
int ssp_detector_heatmap(ssp_handle* h, int slot, float* heat_dev, void* stream);
int ssp_op_heatmap_nms(const float* heat_dev, const ssp_export_params* p, int n_maps, void* workspace_dev,
                       const float* labels_dev, float* nms_map_dev, float* pr_dev, void* stream);

/* ---- descriptor export (export.py:66-190 export_descriptor; Val_model_heatmap.py:33-186) ------------------------
 * ssp_describe_points: after ssp_forward(slot, train = 0) on n images (eval-mode BatchNorm, Val_model_heatmap.py:65),
 *   the per-image body of get_pts_desc_from_agent (export.py:126-142) for the first n images of the slot:
 *     run                 -> flattenDetection of the slot's detector logits (utils/utils.py:515-560)
 *     heatmap_to_pts      -> getPtsFromHeatmap (models/model_wrap.py:266-293): threshold (fp32), greedy NMS, border
 *                            removal, descending confidence (ties: lower row-major index), top_k when p->top_k > 0
 *     soft_argmax_points  -> models/model_wrap.py:212-249 when p->subpixel (sx, sy of the rows, as ssp_export_points)
 *     desc_to_sparseDesc  -> sample_desc_from_points (models/model_wrap.py:295-313) at the INTEGER points: bilinear
 *                            grid_sample (align_corners=True, zeros padding) of the slot's L2-normalised coarse
 *                            descriptor, x_n = x / (W/2) - 1, then divided by the fp32 L2 norm of the sampled vector.
 *                            Image k samples its OWN map (the reference's grid has batch 1: an extension for n > 1).
 *   p->n_views is ignored (>= 1); p->height / width must equal the slot's forward.  cap = ssp_export_max_points(p):
 *   pts_dev [n][cap][5] rows (x, y, confidence, sx, sy), count_dev [n], desc_dev [n][cap][256] (rows < count written).
 *   Returns -1 for a slot without a forward that computed descriptors, or shapes that do not match it.
 *   workspace_dev: ssp_describe_workspace_bytes(p, n) bytes.
 * ssp_op_sample_descriptors: the sampling step alone on a public NCHW desc [b,256,hc,wc] at explicit points
 *   xy [b][cap][2] (x, y) with counts [b] (clamped to cap) -> out [b][cap][256].
 * ssp_match_two_way: PointTracker.nn_match_two_way (models/model_wrap.py:451-497) for n_pairs pairs.  Pair p matches
 *   desc1 + p*pair_stride*cap*256 (count1[p*pair_stride] rows of 256 unit vectors) against desc2 likewise:
 *   dot = D1^T D2 in fp32 (matrix cores), d = sqrt(2 - 2 clip(dot, -1, 1)), row / column argmin of d (first index on
 *   ties, as np.argmin), keep = d_row < nn_thresh && colargmin[rowargmin[i]] == i.  match_dev [n_pairs][cap][3] =
 *   (i, j, d) as floats in ascending i, n_match_dev [n_pairs]; an empty side gives 0 matches.  pair_stride = 2 matches
 *   the interleaved (image, warped image) output of ssp_describe_points.  cap <= SSP_MATCH_MAX_POINTS; nn_thresh < 0 is
 *   refused (the reference raises ValueError).  workspace_dev: ssp_match_workspace_bytes(cap, n_pairs) bytes. */
#define SSP_MATCH_MAX_POINTS 4096
size_t ssp_describe_workspace_bytes(const ssp_export_params* p, int n);
int ssp_describe_points(ssp_handle* h, int slot, const ssp_export_params* p, int n, void* workspace_dev, float* pts_dev,
                        int32_t* count_dev, float* desc_dev, void* stream);
int ssp_op_sample_descriptors(const float* desc_nchw_dev, int b, int hc, int wc, const float* xy_dev,
                              const int32_t* counts_dev, int cap, float* out_dev, void* stream);
size_t ssp_match_workspace_bytes(int cap, int n_pairs);
int ssp_match_two_way(const float* desc1_dev, const int32_t* count1_dev, const float* desc2_dev, const int32_t* count2_dev,
                      int cap, int n_pairs, int pair_stride, float nn_thresh, void* workspace_dev, float* match_dev,
                      int32_t* n_match_dev, void* stream);

/* ---- semantic keypoints: classes at points, class filter, class-aware matching -------------
 * ssp_op_point_classes: the class of each keypoint without the class map.  sout_nhwc_dev, cs, b, h, w, n_classes: the map
 *   of ssp_op_sem_predict under the same contract (cs >= n_classes, the padding channels are never read), with
 *   1 <= n_classes <= 255 here.  pts_dev [b][cap][pts_stride] float rows whose first two floats are the integer pixel
 *   (x, y), as ssp_describe_points writes them (pts_stride 5); count_dev [b] (clamped to cap).  cls_dev [b][cap] uint8:
 *   row r < count gets exactly the class ssp_op_sem_predict gives pixel (y, x) of its image (the x8 align_corners=False
 *   upsample, the same fp32 operations in the same order, the lowest class on ties); rows >= count get SSP_CLASS_NONE.
 *   A point outside [0, w) x [0, h) is a caller error and is clamped into the image.
 * ssp_point_classes: the same on the logits the last forward / pair step left in `slot`, for its first n images (like
 *   ssp_sem_predict).  Returns -1 without a segmentation head or without a forward that computed it.
 * ssp_op_filter_points: stable per-image compaction of a point set by class.  pts_dev [n][cap][5], count_dev [n],
 *   desc_dev [n][cap][256] (16-byte aligned), cls_dev [n][cap]; keep_mask: 256 bits on the HOST, bit c of word c / 32 set =
 *   rows of class c are kept.  The rows r < count whose class is kept go, in their order (so the descending confidence of
 *   ssp_describe_points survives), to pts_out_dev / desc_out_dev / cls_out_dev, their number to count_out_dev [n].
 *   cls_out rows past the new count are SSP_CLASS_NONE, the other rows past it are unspecified.  Never in place.  The
 *   result is a prefix scan, not an atomic ticket: bit-identical from run to run in every mode.
 *   workspace_dev: ssp_filter_workspace_bytes(n, cap) bytes (0 = bad arguments).
 * ssp_match_two_way_classes: ssp_match_two_way with classes cls1_dev, cls2_dev [n_pairs*pair_stride][cap] beside the
 *   descriptors.  A pair (i, j) with cls1[i] != cls2[j] is no candidate: it takes part in neither the row nor the column
 *   arg-min, and a row or column without a candidate has no match.  Distances, the nn_thresh test, the mutual test, the
 *   tie rule, the order of the output, the limits and the workspace are those of ssp_match_two_way; with all classes equal
 *   the output is bit-identical to it.
 * All of them check their arguments before anything is launched (-1, ssp_last_error), take the caller's stream, can be
 * captured into a graph and never synchronise with the host. */
#define SSP_CLASS_NONE 255
int ssp_op_point_classes(const float* sout_nhwc_dev, int cs, int b, int h, int w, int n_classes, const float* pts_dev,
                         int pts_stride, const int32_t* count_dev, int cap, uint8_t* cls_dev, void* stream);
int ssp_point_classes(ssp_handle* h, int slot, int n, const float* pts_dev, int pts_stride, const int32_t* count_dev, int cap,
                      uint8_t* cls_dev, void* stream);
size_t ssp_filter_workspace_bytes(int n, int cap);
int ssp_op_filter_points(const float* pts_dev, const int32_t* count_dev, const float* desc_dev, const uint8_t* cls_dev,
                         const uint32_t keep_mask[8], int n, int cap, float* pts_out_dev, int32_t* count_out_dev,
                         float* desc_out_dev, uint8_t* cls_out_dev, void* workspace_dev, void* stream);
int ssp_match_two_way_classes(const float* desc1_dev, const int32_t* count1_dev, const float* desc2_dev,
                              const int32_t* count2_dev, const uint8_t* cls1_dev, const uint8_t* cls2_dev, int cap, int n_pairs,
                              int pair_stride, float nn_thresh, void* workspace_dev, float* match_dev, int32_t* n_match_dev,
                              void* stream);

/* ---- evaluation of descriptor exports (evaluation.py:86-500 with -r -homo) ---------------------------------------
 * Points are fp64 rows (x, y, confidence) [n_pairs*pair_stride][cap][3] with int32 counts [n_pairs*pair_stride]; pair p
 * uses entry p*pair_stride of each (pair_stride = 2 matches the interleaved image / warped image of the exporter).
 * 1 <= cap <= SSP_MATCH_MAX_POINTS.  One workgroup per pair: a pair's result does not depend on its batch.
 * ssp_eval_repeatability: compute_repeatability (evaluations/detector_evaluation.py:153-275) in fp64 without contraction:
 *   the warped image's points whose hom_inv image lies in [0, width) x [0, height), the image's points warped by hom and
 *   kept by the same rule, the keep_k (<= 2048) most confident of each (ties: the lower index), then the row / column
 *   minima of the N1 x N2 distances.  hom_dev / hom_inv_dev: [n_pairs][9] (hom_inv = np.linalg.inv(hom), host side).
 *   Also counts the matching score's unwarped points (evaluation.py:194-216): the warped image's (y, x) truncated to
 *   integers, warped as (x, y) by float32(hom_inv) in float32, kept when 0 <= p <= (width - 1, height - 1).
 *   out_dev [n_pairs][8] fp64 = N1, N2, count1, count2, sum1, sum2 (the minima <= dist_thresh and their sums),
 *   n_unwarped, 0.  Needs no workspace.
 * ssp_eval_ransac: a RANSAC homography of each pair's matches (match_dev [n_pairs][cap][3] = (i, j, distance) as
 *   ssp_match_two_way writes them, n_match_dev [n_pairs]) from pts1 row i to pts2 row j: exactly 2000 hypotheses, each 4
 *   distinct matches drawn from a counter-based stream of (seeds_dev[p], hypothesis index); a sample with 3 collinear
 *   points in either image is invalid; normalised 4-point DLT (h33 = 1) in fp64; score = #(squared transfer error <= 9);
 *   the highest score wins, ties to the lowest hypothesis.  H is refitted on the winner's inliers (algebraic least
 *   squares, then up to 5 Gauss-Newton steps on the forward transfer error); mask_dev [n_pairs][cap] is the winner's
 *   inlier set.  4 matches: one direct solve, all inliers.  Fewer than 4 matches, or no valid hypothesis: status 1
 *   ("no model"), H = identity, empty mask, 0 inliers; otherwise status 0.  h_dev [n_pairs][9] fp64 (H[8] = 1).
 *   ap_dev (may be NULL): sklearn's average_precision_score of the mask against max(d) - d, 0 without inliers.
 *   workspace_dev: ssp_eval_ransac_workspace_bytes(cap, n_pairs) bytes. */
int ssp_eval_repeatability(const double* pts1_dev, const int32_t* n1_dev, const double* pts2_dev, const int32_t* n2_dev,
                           int cap, int n_pairs, int pair_stride, const double* hom_dev, const double* hom_inv_dev,
                           int height, int width, int keep_k, double dist_thresh, double* out_dev, void* stream);
size_t ssp_eval_ransac_workspace_bytes(int cap, int n_pairs);
int ssp_eval_ransac(const double* pts1_dev, const double* pts2_dev, int cap, int n_pairs, int pair_stride,
                    const float* match_dev, const int32_t* n_match_dev, const uint64_t* seeds_dev, void* workspace_dev,
                    double* h_dev, uint8_t* mask_dev, int32_t* n_inlier_dev, int32_t* status_dev, double* ap_dev,
                    void* stream);

/* ---- epipolar check of matches -------------------------------------------------------------
 * A fundamental-matrix RANSAC for scenes that are not a plane (b^T F a = 0 for a = pts1 row i, b = pts2 row j of a match),
 * and the compaction of the match rows by its mask.  fp64 without contraction; the rules are DESIGN.md section 22 and are
 * restated in numpy by tests/epipolar_ref.py.  No call synchronises with the host or allocates.
 * ssp_epi_ransac: pts1_dev / pts2_dev: fp64 rows starting (x, y), pt_stride >= 2 doubles per row, cap rows per entry; pair
 *   p reads entry p * pair_stride of each.  match_dev [n_pairs][cap][3] = (i, j, distance) as ssp_match_two_way writes them,
 *   n_match_dev [n_pairs]; seeds_dev [n_pairs].  Exactly 2000 hypotheses: 8 distinct matches from the counter-based stream
 *   of ssp_eval_ransac (the same redraw rule), both images normalised over the 8 points, the null vector of the 8x9
 *   system by Gaussian elimination with complete pivoting (pivot <= 1e-12: invalid), no rank-2 step per hypothesis;
 *   score = #(squared Sampson distance <= thresh^2); the highest score wins, ties to the lowest hypothesis; a winner needs
 *   a score of at least 8.  8 matches: one direct solve.  mask_dev [n_pairs][cap] is the winner's inlier set.  F is
 *   refitted on the inliers (8x8 normal equations with the winner's largest entry held at 1), made rank 2 (Jacobi on
 *   F^T F, F - (F v) v^T), scaled to unit Frobenius norm with its largest |entry| positive.  f_dev [n_pairs][9].
 *   Fewer than 8 matches or no winner: status 1 ("no model"), F = 0, empty mask, 0 inliers, winner -1; otherwise 0.
 *   winner_dev (may be NULL): the winning hypothesis; err_dev (may be NULL): RMS Sampson distance of the inliers under F.
 *   groups: workgroups that share the hypotheses of one pair (1 .. 64; 0 = the library's choice: 32 while 32 * n_pairs
 *   workgroups fit the 256 CUs at one each, else 16).  A pair's result does
 *   not depend on groups, on its batch or on the order the workgroups run in.
 *   workspace_dev: ssp_epi_ransac_workspace_bytes(cap, n_pairs) bytes.
 * ssp_op_filter_matches: match_out_dev [n_pairs][cap][3] = the rows of match_dev whose mask byte is set, in order, zero
 *   rows behind them; n_match_out_dev [n_pairs] their count.  A pair with status != 0 or n_inlier < min_inliers passes
 *   through unchanged (decided on the device).  Never in place. */
size_t ssp_epi_ransac_workspace_bytes(int cap, int n_pairs);
int ssp_epi_ransac(const double* pts1_dev, const double* pts2_dev, int pt_stride, int cap, int n_pairs, int pair_stride,
                   const float* match_dev, const int32_t* n_match_dev, const uint64_t* seeds_dev, double thresh, int groups,
                   void* workspace_dev, double* f_dev, uint8_t* mask_dev, int32_t* n_inlier_dev, int32_t* status_dev,
                   int32_t* winner_dev, double* err_dev, void* stream);
int ssp_op_filter_matches(const float* match_dev, const int32_t* n_match_dev, const uint8_t* mask_dev, const int32_t* status_dev,
                          const int32_t* n_inlier_dev, int min_inliers, int cap, int n_pairs, float* match_out_dev,
                          int32_t* n_match_out_dev, void* stream);

/* ---- two-view pose --------------------------------------------------------------------------
 * The camera motion of a calibrated pair from ssp_epi_ransac's F, mask, n_inlier and status, and the trajectory over
 * consecutive pairs.  Camera model a ~ K1 X1, b ~ K2 X2, X2 = R X1 + t, so F ~ K2^-T [t]x R K1^-1.  fp64 without
 * contraction; the rules are DESIGN.md section 24 and are restated in numpy by tests/pose_ref.py.  No call synchronises with
 * the host or allocates.
 * ssp_pose_from_fundamental: pts / match / n_match / pt_stride / cap / pair_stride as for ssp_epi_ransac (the same gathered
 *   rows, the same clamping); f_dev [n_pairs][9], mask_dev [n_pairs][cap], n_inlier_dev, status_in_dev [n_pairs] as it wrote
 *   them.  intr_dev: fp64 [n_intr][2][4] = (fx, fy, cx, cy) of view 1 and view 2, n_intr = 1 (shared by all pairs) or
 *   n_pairs.  E0 = K2^T F K1 scaled to unit Frobenius norm; V from 8 sweeps of cyclic Jacobi on E0^T E0 (v0, v1: the columns
 *   of the two largest diagonal entries, v2 = v0 x v1), u0 = E0 v0 / |.|, u1 = E0 v1 made orthogonal to u0 and normalised,
 *   u2 = u0 x u1; e_dev [n_pairs][9] = u0 v0^T + u1 v1^T (singular values 1, 1, 0).  Candidates 0..3 = (Ra, +u2),
 *   (Ra, -u2), (Rb, +u2), (Rb, -u2) with Ra = U W V^T, Rb = U W^T V^T.  A match is in front when the least-squares meeting
 *   point of its two rays has finite positive depths z1, z2 and the rays are not parallel (det > 1e-12 A11 A22).  Only rows
 *   whose mask byte is set count; the most in-front rows win, ties to the lowest candidate.  r_dev [n_pairs][9],
 *   t_dev [n_pairs][3] (unit length: the baseline is the unit of every depth), cand_dev [n_pairs] (the winner, -1),
 *   counts_dev [n_pairs][4], n_front_dev [n_pairs].  status_dev [n_pairs]: 0; 1 = no pose (status_in != 0, n_inlier < 8 or a
 *   degenerate matrix: R = I, t = 0, E = 0, counts 0, per-row outputs 0); 2 = ambiguous (fewer than 8 rows in front, or fewer
 *   than half of n_inlier; the winner is still written).  Per match row, aligned with the UNFILTERED rows as the mask is:
 *   front_dev [n_pairs][cap], depth_dev [n_pairs][cap][2] = (z1, z2), x_dev [n_pairs][cap][3] = z1 * ((ax-cx1)/fx1,
 *   (ay-cy1)/fy1, 1), the point in camera 1's frame; zero where front is 0.  One workgroup per pair: a pair's result does
 *   not depend on its batch.
 * ssp_pose_chain: one frame of n_seq sequences.  Pair A = (f-1, f) ("prev": its front / depth / status / match / n_match /
 *   cap; all NULL when there is no such pair) and pair B = (f, f+1) (the same plus r_dev, t_dev).  A point of frame f is row
 *   j of A's matches and row i of B's: zprev[j] = z2 of A's in-front rows (the lowest row wins), the shared points are B's
 *   in-front rows whose i has an entry, ratio = sum(zprev) / sum(z1) over them (sums in a fixed order).  state_dev
 *   [n_seq][SSP_POSE_STATE_WORDS] fp64 = (n_frames, s, Rw [9], tw [3], 2 spare); a new sequence starts from
 *   (0, 1, identity, 0).  s <- s * ratio when both poses have status 0, at least 8 points are shared and the ratio is finite
 *   and positive; otherwise s is carried and flag bit 1 is set.  Rw <- R Rw, tw <- R tw + s t (R = I, t = 0 and flag bit 0
 *   when B's status is not 0), C = -(Rw^T tw).  The row (Rw [9], C [3], s, n_shared, flags, ratio) is written to table_dev
 *   [n_seq][capacity][SSP_POSE_ROW_WORDS] at row n_frames, which then grows by one; a full table stops growing (the state
 *   still advances). */
#define SSP_POSE_ROW_WORDS 16
#define SSP_POSE_STATE_WORDS 16
int ssp_pose_from_fundamental(const double* f_dev, const uint8_t* mask_dev, const int32_t* n_inlier_dev, const int32_t* status_in_dev,
                              const double* pts1_dev, const double* pts2_dev, int pt_stride, int cap, int n_pairs, int pair_stride,
                              const float* match_dev, const int32_t* n_match_dev, const double* intr_dev, int n_intr, double* r_dev,
                              double* t_dev, double* e_dev, int32_t* cand_dev, int32_t* counts_dev, int32_t* n_front_dev,
                              int32_t* status_dev, uint8_t* front_dev, double* depth_dev, double* x_dev, void* stream);
int ssp_pose_chain(const uint8_t* front_prev_dev, const double* depth_prev_dev, const int32_t* status_prev_dev,
                   const float* match_prev_dev, const int32_t* n_match_prev_dev, int cap_prev, const uint8_t* front_dev,
                   const double* depth_dev, const int32_t* status_dev, const double* r_dev, const double* t_dev,
                   const float* match_dev, const int32_t* n_match_dev, int cap, int n_seq, double* state_dev, double* table_dev,
                   int capacity, void* stream);

/* ---- homography pose and model selection ---------------------------------------------------------
 * The camera motion of a calibrated pair from ssp_eval_ransac's H (view 1 pixels to view 2 pixels), mask, n_inlier and status,
 * for the pairs a fundamental matrix does not describe: a plane N . X1 = d seen twice (K2^-1 H K1 ~ R + (t/d) N^T) and a camera
 * that only rotates.  Camera model as above.  fp64 without contraction; restated in numpy by tests/pose_h_ref.py.  No call
 * synchronises with the host or allocates.
 * ssp_pose_from_homography: pts / match / n_match / pt_stride / cap / pair_stride / intr_dev / n_intr and the outputs r_dev ..
 *   x_dev as for ssp_pose_from_fundamental (there is no e_dev).  prior_dev: fp64 [n_pairs][2][3] or NULL, the normals2 of the
 *   pair before (a zero vector is no prior); not the array normals2_dev.  use_h_dev: int32 [n_pairs] or NULL; when given, a pair
 *   whose entry is 0 keeps all its outputs as they are, except model 0 and zero normals.  Valid: status_in == 0 and n_inlier >= 8,
 *   else status 1 with the outputs of ssp_pose_from_fundamental's "no pose" and model 0.  Hn = K2^-1 H K1, negated when fewer
 *   than half of n_inlier mask rows have b~^T Hn a~ > 0.  8 sweeps of cyclic Jacobi on Hn^T Hn, eigenvalues w1 >= w2 >= w3 (the
 *   lowest index on ties) with v1, v2, v3, v3 flipped so that det V = +1; Hn / sqrt(w2), w1 / w2, w3 / w2 (a negative w3 counts
 *   as 0); a non-finite value or w2 <= 0 gives status 1.  sqrt(w1) - sqrt(w3) <= rotation_eps: model 2, R = Hn made orthonormal
 *   (row 0 normalised, row 1 made orthogonal to it and normalised, row 2 their cross product), t = 0, per-row outputs and counts
 *   0, cand -1, status 0, normal 0, normals2 = R prior (the priors travel with the camera).  Otherwise model 1: u_a, u_b =
 *   (sqrt(1 - w3) v1 +- sqrt(w1 - 1) v3) / sqrt(w1 - w3); per u: U = [v2, u, v2 x u], W = [Hn v2, Hn u, Hn v2 x Hn u], R = W U^T,
 *   N = v2 x u, T = (Hn - R) N; candidates 0..3 = (R_a, N_a, T_a), (R_a, -N_a, -T_a), (R_b, N_b, T_b), (R_b, -N_b, -T_b).  A mask
 *   row counts for a candidate when N . a~ > 0 and it is in front under (R, T / |T|) by ssp_pose_from_fundamental's rule.  A
 *   candidate is alive with count >= 8 and 2 count >= n_inlier.  None alive: the highest count wins (ties to the lowest index),
 *   status 2.  One alive: it wins, status 0.  More: each is scored by max_k (N . prior_k) over the non-zero priors; the best wins
 *   with status 0 when it leads the next by at least normal_margin; without a prior or with a smaller lead the largest N_z wins
 *   (ties to the lowest index), status 2.  t = T / |T|; model_dev [n_pairs] (0 = none, 1 = plane, 2 = rotation), normal_dev
 *   [n_pairs][3] = the winner's N, normals2_dev [n_pairs][2][3] = R_c N_c of the candidates alive in index order (two at most),
 *   zeros behind them.  Per-row outputs under the winner (front also needs N . a~ > 0).
 * ssp_model_select: F / H with the mask, n_inlier and status of ssp_epi_ransac / ssp_eval_ransac; the unfiltered matches and the
 *   points as above.  S_H = sum over the match rows of rho(d12^2; 5.99) + rho(d21^2; 5.99), the squared transfer distances under
 *   H and under its inverse (by cofactors; a zero or non-finite determinant gives S_H = 0); S_F the same with the squared
 *   distances to the epipolar lines in both images and 3.84; rho(d2; T) = 5.99 - d2 when d2 < T, else 0; sums in a fixed order.
 *   use_h = status_H == 0 and (status_F != 0 or S_H >= model_ratio (S_H + S_F)).  scores_dev [n_pairs][2] = (S_H, S_F), use_h_dev
 *   [n_pairs]; mask_dev [n_pairs][cap], n_inlier_dev, status_dev [n_pairs]: the selected model's, copied (arrays of their own). */
int ssp_pose_from_homography(const double* h_dev, const uint8_t* mask_dev, const int32_t* n_inlier_dev, const int32_t* status_in_dev,
                             const double* pts1_dev, const double* pts2_dev, int pt_stride, int cap, int n_pairs, int pair_stride,
                             const float* match_dev, const int32_t* n_match_dev, const double* intr_dev, int n_intr,
                             const double* prior_dev, const int32_t* use_h_dev, double rotation_eps, double normal_margin, double* r_dev,
                             double* t_dev, int32_t* cand_dev, int32_t* counts_dev, int32_t* n_front_dev, int32_t* status_dev,
                             uint8_t* front_dev, double* depth_dev, double* x_dev, int32_t* model_dev, double* normal_dev,
                             double* normals2_dev, void* stream);
int ssp_model_select(const double* f_dev, const uint8_t* f_mask_dev, const int32_t* f_n_inlier_dev, const int32_t* f_status_dev,
                     const double* h_dev, const uint8_t* h_mask_dev, const int32_t* h_n_inlier_dev, const int32_t* h_status_dev,
                     const double* pts1_dev, const double* pts2_dev, int pt_stride, int cap, int n_pairs, int pair_stride,
                     const float* match_dev, const int32_t* n_match_dev, double model_ratio, double* scores_dev, int32_t* use_h_dev,
                     uint8_t* mask_dev, int32_t* n_inlier_dev, int32_t* status_dev, void* stream);

/* ---- landmarks from tracks ---------------------------------------------------------------------
 * One point in the world frame per track row: the row's observations in the L retained frames (the track table and the ring
 * of point sets of ssp_op_track_update / ssp_op_track_points) under the cameras of the trajectory (ssp_pose_chain).  World =
 * the first camera of the sequence, unit = the first baseline.  fp64 without contraction; the rules are DESIGN.md section 26
 * and are restated in numpy by tests/landmarks_ref.py.  No call synchronises with the host or allocates.
 * ssp_map_window: state_dev [SSP_POSE_STATE_WORDS] and table_dev [capacity][SSP_POSE_ROW_WORDS] of one sequence; intr_dev fp64
 *   [n_intr][4] = (fx, fy, cx, cy), n_intr = 1 (shared) or max_length (per retained frame).  n_frames >= 0: the number of frames
 *   given so far, as the caller counted them; -1: the state's count, which stops at `capacity`.  Retained frame c (0 = oldest)
 *   is frame f = n_frames - L + c.  cams_dev [max_length][SSP_CAM_WORDS] = (Rw [9], C [3], fx, fy, cx, cy, valid, 3 spare); a
 *   view is valid when 0 <= f < capacity, f >= w and the focal lengths are finite and positive, else its record is zero.  w is
 *   the start of the newest consistent window: the smallest w such that every row in (w, n-1] has flag bit 0 clear and every
 *   row in (w+1, n-1] flag bit 1; a row the table does not hold breaks it.
 * ssp_op_triangulate_tracks: ids_dev [row_cap][max_length], state_dev [2 + max_length], pts_dev [max_length][point_cap][2]
 *   with first_slot as for ssp_op_track_points.  A retained frame gives an observation when its id is >= 0, its camera is
 *   valid and the id names a point of its frame.  Per row below n_rows: n_views_dev, status_dev (int32), x_dev [3], rms_dev,
 *   cos_parallax_dev.  status: SSP_LANDMARK_FEW_VIEWS fewer than min_views (>= 2) observations; SSP_LANDMARK_DEGENERATE the
 *   smallest d_i . d_j over the pairs of unit rays is above cos_min_parallax (the caller's cos(min angle)), or the midpoint
 *   system / a Gauss-Newton step is singular (det not finite or <= 1e-12 * the product of the diagonal) or not finite;
 *   SSP_LANDMARK_BEHIND the depth in a used view is not finite and positive at the midpoint or after the last step;
 *   SSP_LANDMARK_REPROJ rms = sqrt(sum r^2 / (2 n_views)) of the pixel residuals is above max_reproj; in that order, else 0.
 *   The point is the midpoint of the rays (A = sum(I - d d^T), b = sum((I - d d^T) C)) refined by exactly 4 Gauss-Newton steps
 *   on the pixel reprojection error.  x, rms and cos_parallax are written whenever they were computed and are finite (also
 *   under status 2 to 4), else zero.  Rows at or past n_rows are not written.  A row's result depends on nothing but its own
 *   inputs.
 * ssp_op_landmarks_select: the status-0 rows in table order -> landmarks_dev [row_cap][SSP_LANDMARK_WORDS] fp64 rows (track
 *   id, X, Y, Z, n_views, rms, cos_parallax, index of the track's point in the newest frame or -1) and n_landmarks_dev [1];
 *   workspace_dev: ssp_landmark_workspace_bytes(max_length, row_cap) bytes. */
#define SSP_CAM_WORDS 20
#define SSP_LANDMARK_WORDS 8
#define SSP_LANDMARK_FEW_VIEWS 1
#define SSP_LANDMARK_DEGENERATE 2
#define SSP_LANDMARK_BEHIND 3
#define SSP_LANDMARK_REPROJ 4
size_t ssp_landmark_workspace_bytes(int max_length, int row_cap);
int ssp_map_window(const double* state_dev, const double* table_dev, int capacity, const double* intr_dev, int n_intr, int max_length,
                   int n_frames, double* cams_dev, void* stream);
int ssp_op_triangulate_tracks(const int32_t* ids_dev, const int32_t* state_dev, const double* pts_dev, int first_slot,
                              const double* cams_dev, int max_length, int point_cap, int row_cap, int min_views,
                              double cos_min_parallax, double max_reproj, double* x_dev, int32_t* n_views_dev, double* rms_dev,
                              double* cos_parallax_dev, int32_t* status_dev, void* stream);
int ssp_op_landmarks_select(const int32_t* ids_dev, const int32_t* tid_dev, const int32_t* state_dev, const int32_t* status_dev,
                            const double* x_dev, const int32_t* n_views_dev, const double* rms_dev, const double* cos_parallax_dev,
                            int max_length, int point_cap, int row_cap, void* workspace_dev, double* landmarks_dev,
                            int32_t* n_landmarks_dev, void* stream);

/* ---- absolute pose from landmarks -------------------------------------------------------------
 * The camera of a frame from 3-D to 2-D correspondences: landmark rows joined with the matches of the next frame, a P3P RANSAC
 * of 512 hypotheses with a Gauss-Newton refit, and the repair of a trajectory row the two-view chain could not determine.
 * Camera model y = Rw (X - C), u = fx y0 / y2 + cx.  fp64 without contraction; the rules are DESIGN.md section 27 and are
 * restated in numpy by tests/pnp_ref.py.  No call synchronises with the host or allocates.
 * ssp_op_landmark_matches: landmarks_dev [row_cap][SSP_LANDMARK_WORDS] and n_landmarks_dev [1] of ssp_op_landmarks_select for
 *   the window ending at the previous frame; match_dev [cap][3] fp32 rows (i, j, distance) and n_match_dev [1] of the pair
 *   (previous, new), unfiltered; pts_new_dev [point_cap][pt_stride] fp64 rows starting (x, y).  Indices are clamped to
 *   [0, point_cap).  The landmark of point i is the LOWEST landmark row whose eighth word is i.  corr_dev
 *   [cap][SSP_CORR_WORDS] fp64 rows (X, Y, Z, px, py, landmark row, valid, 0), one per match row, zero where the row has no
 *   landmark, lies at or past n_match or holds a non-finite value; n_corr_dev [2] = (rows, valid rows).
 * ssp_pnp_ransac: n_problems problems.  corr_dev [n_problems][cap][SSP_CORR_WORDS], n_dev [n_problems] rows used, intr_dev
 *   fp64 [n_intr][4] = (fx, fy, cx, cy), n_intr = 1 (shared) or n_problems, seeds_dev [n_problems].  Hypothesis h draws 4
 *   distinct valid rows from the counter-based stream of ssp_epi_ransac (4 rows: the one direct solve; fewer: none); three
 *   give up to four P3P solutions, the fourth keeps the one that reprojects it best.  The score counts the valid rows in front
 *   of the camera whose reprojection error is <= thresh pixels; the highest score wins, ties to the lowest h, and needs
 *   max(min_inliers, 4) rows.  4 Gauss-Newton steps over the winner's inliers (Cayley rotation update), then the mask once more:
 *   if it keeps fewer rows the winner's pose and mask stand.  rw_dev [n_problems][9], c_dev [n_problems][3], mask_dev
 *   [n_problems][cap], n_inlier_dev, winner_dev (-1), rms_dev = sqrt(sum e^2 / (2 k)), status_dev (1 = no pose: Rw = I, C = 0,
 *   empty mask).  groups: workgroups per problem (0 = the library's choice, at most 64); a problem's result depends on its
 *   own inputs and seed only.  workspace_dev: ssp_pnp_workspace_bytes(n_problems) bytes (0 = bad arguments).
 * ssp_pose_repair: n_seq sequences; rw_dev [n_seq][9], c_dev [n_seq][3], status_dev [n_seq] of ssp_pnp_ransac; state_dev and
 *   table_dev of ssp_pose_chain.  Acts on row n - 1 of a table holding 1 <= n < capacity rows (a full table is left alone) when
 *   that row carries flag bit 0 or 1 and the absolute pose has status 0 and is finite: Rw and C are replaced in the row and
 *   the state, tw = -(Rw C), s = |C - C of row n - 2| when that is finite and above 1/64 of the previous s (bit 1 is cleared),
 *   else s is kept (bit 1 stays as it was); bit 0 is cleared and SSP_POSE_FLAG_ABSOLUTE set.  Otherwise nothing is written. */
#define SSP_CORR_WORDS 8
#define SSP_POSE_FLAG_ABSOLUTE 4
size_t ssp_pnp_workspace_bytes(int n_problems);
int ssp_op_landmark_matches(const double* landmarks_dev, const int32_t* n_landmarks_dev, int row_cap, const float* match_dev,
                            const int32_t* n_match_dev, int cap, const double* pts_new_dev, int pt_stride, int point_cap,
                            double* corr_dev, int32_t* n_corr_dev, void* stream);
int ssp_pnp_ransac(const double* corr_dev, const int32_t* n_dev, int cap, int n_problems, const double* intr_dev, int n_intr,
                   const uint64_t* seeds_dev, double thresh, int min_inliers, int groups, void* workspace_dev, double* rw_dev,
                   double* c_dev, uint8_t* mask_dev, int32_t* n_inlier_dev, int32_t* winner_dev, double* rms_dev,
                   int32_t* status_dev, void* stream);
int ssp_pose_repair(const double* rw_dev, const double* c_dev, const int32_t* status_dev, int n_seq, double* state_dev,
                    double* table_dev, int capacity, void* stream);

/* ---- windowed bundle adjustment ------------------------------------------------------------------
 * The cameras of the retained frames (ssp_map_window) and the status-0 rows of ssp_op_triangulate_tracks refined together:
 * Levenberg-Marquardt on the pixel reprojection error, the points eliminated by the Schur complement, plain least squares.
 * fp64 without contraction; the rules are DESIGN.md section 28 and are restated in numpy by tests/ba_ref.py.  Every sum over
 * the rows runs in one fixed order, so a result depends on nothing but the call's inputs (not on row_cap, the run or the
 * batch).  No call synchronises with the host or allocates; the number of launches depends on `iterations` alone.
 * ssp_bundle_adjust: the arguments of ssp_op_triangulate_tracks, its x_dev [row_cap][3] and status_dev [row_cap] as inputs.
 *   Unknowns: (w, dC) of every valid view (Rw <- renormalised Cay(w) Rw, C <- C + dC, section 27's update) and X of every row
 *   below n_rows with status 0; the observations are section 26's.  Held: every invalid view, the first valid view a, and
 *   coordinate k* of the centre of the last valid view b (the component of C_b - C_a of largest magnitude, lowest on ties).
 *   lambda starts at 1e-4 and scales the diagonals of U and V by (1 + lambda); V_r is inverted by section 26's cofactor solve
 *   (a refused row contributes nothing in that iteration); the reduced 6L x 6L system is solved by Cholesky without pivoting
 *   (a pivot that is not finite or <= 0 rejects the step).  A step is accepted when its cost is finite, every used view keeps
 *   the point in front and the cost falls: lambda / 10 (at least 1e-12), else lambda * 10 (at most 1e6).  After an accepted
 *   step the loop is done when cur - new <= 1e-10 cur or new <= 2 n_obs (1e-9)^2.  1 <= iterations <= SSP_BA_MAX_ITERATIONS.
 *   cams_out_dev [max_length][SSP_CAM_WORDS] (invalid views zero), x_out_dev [row_cap][3] (rows not used are copies),
 *   rms_out_dev [row_cap] (0 where the row is not used), info_dev [SSP_BA_INFO_WORDS] fp64 = (status, cost before, cost
 *   after, n_obs, rows used, accepted steps, refused V solves, final lambda).  status 0: adjusted; 1: nothing to adjust (fewer
 *   than 2 valid views, no used row, or 2 n_obs < 6 (valid - 1) - 1 + 3 rows); 2: no step accepted.  Under 1 and 2 the outputs
 *   are copies of the inputs.  The outputs must not alias the inputs.  workspace_dev: ssp_ba_workspace_bytes(max_length,
 *   row_cap) bytes (0 = bad arguments).
 * ssp_ba_apply: n_seq sequences; info_dev [n_seq][SSP_BA_INFO_WORDS], cams_dev [n_seq][max_length][SSP_CAM_WORDS] of
 *   ssp_bundle_adjust; state_dev and table_dev of ssp_pose_chain.  n_frames as for ssp_map_window.  Acts only under status 0:
 *   for every valid view c other than a with 0 <= f = n - L + c < capacity, row f takes Rw and C and flag bit 3
 *   (SSP_POSE_FLAG_ADJUSTED); s becomes |C_f - C_(f-1)| when view c - 1 is valid and the length is finite and above 1/64 of
 *   the row's s.  When row n - 1 is the state's newest frame and the table is not full, the state's Rw, tw = -(Rw C) and s
 *   follow it.  Bits 0 and 1 are not touched. */
#define SSP_BA_INFO_WORDS 8
#define SSP_BA_MAX_ITERATIONS 16
#define SSP_POSE_FLAG_ADJUSTED 8
size_t ssp_ba_workspace_bytes(int max_length, int row_cap);
int ssp_bundle_adjust(const int32_t* ids_dev, const int32_t* state_dev, const double* pts_dev, int first_slot, const double* cams_dev,
                      int max_length, int point_cap, int row_cap, const double* x_dev, const int32_t* status_dev, int iterations,
                      double* cams_out_dev, double* x_out_dev, double* rms_out_dev, double* info_dev, void* workspace_dev,
                      void* stream);
int ssp_ba_apply(const double* info_dev, const double* cams_dev, int max_length, int n_seq, int n_frames, double* state_dev,
                 double* table_dev, int capacity, void* stream);

/* ---- world map ---------------------------------------------------------------------------------
 * Landmarks that outlive their window: a store of one sequence (X and a descriptor per track), a matcher of a frame's descriptors
 * against the whole store, the join of its matches with the store's points (the input of ssp_pnp_ransac) and the repair of the
 * newest trajectory row from the pose found.  The rules are restated in numpy by tests/world_ref.py.  No call synchronises with the
 * host or allocates.
 * The store, 1 <= map_cap <= SSP_WORLD_MAX_ROWS rows and tid_cap >= 1 track ids: x_dev fp64 [map_cap][3], desc_dev fp32
 *   [map_cap][256], tid_dev / views_dev / first_dev / last_dev int32 [map_cap], rms_dev fp64 [map_cap], slot_of_tid_dev int32
 *   [tid_cap], state_dev int32 [SSP_WORLD_STATE_WORDS] = (n_rows, anchored, lost_frames, streak, rows dropped because the map was
 *   full, rows dropped because their track id is >= tid_cap, rows appended by the last insert, rows updated by it).  Track t is in
 *   the map iff s = slot_of_tid[t] has 0 <= s < n_rows and tid[s] == t: zeroed memory is an empty map and n_rows = 0 clears it.
 * ssp_op_world_insert: once per frame, after every rewrite of the frame's trajectory row.  landmarks_dev [row_cap]
 *   [SSP_LANDMARK_WORDS] and n_landmarks_dev [1] of ssp_op_landmarks_select for the window ending at the newest frame; desc_new_dev
 *   fp32 [point_cap][256] and count_new_dev [1] of that frame; table_dev [capacity][SSP_POSE_ROW_WORDS] of ssp_pose_chain and the
 *   caller's frame count n_frames (the newest row is n_frames - 1; without such a row the frame counts as flagged).
 *   Anchor rule, from that row's flag word F: ok = (F & 3) == 0; anchored' = ok && (n_rows == 0 || anchored || streak >= 2); while
 *   n_rows > 0 && !anchored', lost_frames counts up, and past `patience` the map is cleared (n_rows, lost_frames, streak and the
 *   two drop counters 0; the next ok frame adopts its own frame of reference); otherwise lost_frames = 0.  Rows are inserted only
 *   when anchored'.  A landmark row takes part iff its newest-frame index p has 0 <= p < count, its track id lies in [0, tid_cap)
 *   and X is finite.  Found in the map: X, n_views, rms, last_frame = n_frames - 1 and the descriptor desc_new[p] are replaced.
 *   Else appended in landmark order (first_frame = last_frame = n_frames - 1) while there is room; past map_cap dropped and counted.
 *   Track ids must be unique within a call.  workspace_dev: ssp_world_insert_workspace_bytes(row_cap) bytes.
 * ssp_match_world: ssp_match_two_way's rules with side 1 = the n_rows (state_dev[0], clamped to map_cap) rows of desc_dev and side
 *   2 = the count2_dev[0] (clamped to cap, 1 <= cap <= SSP_MATCH_MAX_POINTS) rows of desc2_dev [cap][256]: the same fp32 chain per
 *   dot product, the same keys, first index on ties on both sides, keep = d < nn_thresh && mutual; bit-identical to
 *   ssp_match_two_way wherever both apply.  match_dev [cap][3] = (map row, frame row, d) in ascending map row, n_match_dev [1].
 *   workspace_dev: ssp_match_world_workspace_bytes(map_cap, cap) bytes (0 = bad arguments).
 * ssp_op_world_correspondences: corr_dev [cap][SSP_CORR_WORDS] = (X, Y, Z, px, py, map row, valid, 0) per match row, n_corr_dev [2]
 *   = (rows, valid rows).  A row is valid iff it lies below n_match, its map row is < n_rows, its frame point is < count_new_dev[0]
 *   (clamped to point_cap) and the five values are finite; every other row is zero.  pts_new_dev fp64 [point_cap][pt_stride].
 * ssp_world_repair: ssp_pose_repair's rule for one sequence (rw_dev [9], c_dev [3], status_dev [1] of ssp_pnp_ransac), firing when
 *   the pose has status 0 and is finite and either row n - 1 carries flag bit 0 or 1 or the map is lost (n_rows > 0 && !anchored).
 *   Sets SSP_POSE_FLAG_ABSOLUTE and SSP_POSE_FLAG_WORLD; streak += 1 when it rewrites the row, streak = 0 when it does not. */
#define SSP_WORLD_MAX_ROWS 65536
#define SSP_WORLD_STATE_WORDS 8
#define SSP_POSE_FLAG_WORLD 16
size_t ssp_world_insert_workspace_bytes(int row_cap);
size_t ssp_match_world_workspace_bytes(int map_cap, int cap);
int ssp_op_world_insert(const double* landmarks_dev, const int32_t* n_landmarks_dev, int row_cap, const float* desc_new_dev,
                        const int32_t* count_new_dev, int point_cap, const double* table_dev, int capacity, int n_frames, int patience,
                        int map_cap, int tid_cap, double* x_dev, float* desc_dev, int32_t* tid_dev, int32_t* views_dev,
                        int32_t* first_dev, int32_t* last_dev, double* rms_dev, int32_t* slot_of_tid_dev, int32_t* state_dev,
                        void* workspace_dev, void* stream);
int ssp_match_world(const float* desc_dev, const int32_t* state_dev, int map_cap, const float* desc2_dev, const int32_t* count2_dev,
                    int cap, float nn_thresh, void* workspace_dev, float* match_dev, int32_t* n_match_dev, void* stream);
int ssp_op_world_correspondences(const double* x_dev, const int32_t* state_dev, int map_cap, const float* match_dev,
                                 const int32_t* n_match_dev, int cap, const double* pts_new_dev, int pt_stride,
                                 const int32_t* count_new_dev, int point_cap, double* corr_dev, int32_t* n_corr_dev, void* stream);
int ssp_world_repair(const double* rw_dev, const double* c_dev, const int32_t* status_dev, double* state_dev, double* table_dev,
                     int capacity, int map_cap, int32_t* world_state_dev, void* stream);

/* ---- world map upkeep ----------------------------------------------------------------------------
 * One call per frame, right after ssp_op_world_insert and with the arrays that call got: it merges the row pair of a scene point
 * that returned under a new track id, culls rows that never matured, evicts the least valuable rows when the map nears its
 * capacity, and compacts the store, so that no dead row is ever visible between calls.  The rules are restated in numpy by
 * tests/world_upkeep_ref.py.  No call synchronises with the host or allocates.
 *   match_dev [cap][3] / n_match_dev [1]: the frame's ssp_match_world rows, computed before the insert (an anchored insert only
 *   appends and updates, so they still name the same rows); landmarks_dev [row_cap][SSP_LANDMARK_WORDS] / n_landmarks_dev [1],
 *   count_new_dev [1], point_cap: as given to the insert; pts_new_dev fp64 [point_cap][pt_stride]: the frame's points (x, y);
 *   table_dev [capacity][SSP_POSE_ROW_WORDS] and n_frames: the newest row is f = n_frames - 1; intr_dev fp64 [4] = (fx, fy, cx, cy).
 * The call does nothing, and sets report word 7, unless state[1] (anchored) == 1, n_rows > 0 and row f exists.  Four phases, each
 * later one on the rows still alive:
 *   merge (params->merge != 0): for match row (r, p), q = the lowest landmark row that passes the insert's test and names point p,
 *     t' its track id, r' its slot; the pair merges iff r' >= 0, r' != r, last_frame[r] < f, last_frame[r'] == f, X[r] has a finite
 *     positive depth under (Rw, C) of row f and its squared reprojection error against pts_new[p] is <= merge_thresh^2 (fp64,
 *     ssp_pnp_ransac's residual).  The lower slot survives with r''s tid, X, rms, n_views, descriptor, last_frame = f and the
 *     smaller first_frame; slot_of_tid[t'] names it; the other row dies.
 *   cull (cull_age >= 0): a row dies iff last_frame < f - cull_age and n_views < cull_min_views.
 *   evict (high_water >= 0; 0 <= low_water <= high_water <= map_cap): if the rows alive exceed high_water, the k = min(alive -
 *     low_water, rows with last_frame != f) rows of smallest key (min(max(n_views, 0), 255), max(last_frame, 0), 65535 - slot) die.
 *   compact: survivors keep their order; all nine arrays move, slot_of_tid is rewritten for the rows that moved, state[0] becomes the
 *     new count.  When nothing died the store, slot_of_tid and state are left as they were.
 * report_dev int32 [SSP_WORLD_UPKEEP_REPORT_WORDS] = (rows before, merged, culled, evicted, rows after, eviction fired, rows wanted
 * but protected, skipped); totals_dev int64 [4] (or NULL) += (merged, culled, evicted, 1).
 * workspace_dev: ssp_world_upkeep_workspace_bytes(map_cap) bytes (0 = bad arguments). */
#define SSP_WORLD_UPKEEP_REPORT_WORDS 8
typedef struct ssp_world_upkeep_params {
  int merge;            /* 0: no merging */
  double merge_thresh;  /* pixels */
  int cull_age;         /* negative: no culling */
  int cull_min_views;
  int high_water;       /* negative: no eviction */
  int low_water;
} ssp_world_upkeep_params;
size_t ssp_world_upkeep_workspace_bytes(int map_cap);
int ssp_op_world_upkeep(const float* match_dev, const int32_t* n_match_dev, int cap, const double* landmarks_dev,
                        const int32_t* n_landmarks_dev, int row_cap, const double* pts_new_dev, int pt_stride,
                        const int32_t* count_new_dev, int point_cap, const double* table_dev, int capacity, int n_frames,
                        const double* intr_dev, const ssp_world_upkeep_params* params, int map_cap, int tid_cap, double* x_dev,
                        float* desc_dev, int32_t* tid_dev, int32_t* views_dev, int32_t* first_dev, int32_t* last_dev, double* rms_dev,
                        int32_t* slot_of_tid_dev, int32_t* state_dev, int32_t* report_dev, int64_t* totals_dev, void* workspace_dev,
                        void* stream);

/* ---- world map classes ---------------------------------------------------------------------------
 * What every landmark lies on: a class vote per track, the map read out as a labelled point cloud, and ssp_match_world restricted
 * to pairs of one known, kept class.  The rules are restated in numpy by tests/world_classes_ref.py.  No call synchronises with the
 * host or allocates.
 *   votes_dev uint16 [tid_cap], keyed by TRACK ID (map slots move under the upkeep): the low byte is the class, the high byte the
 *   vote count; zeroed memory = no class yet.  The decoded class is SSP_CLASS_NONE when the count is 0, else the low byte.
 * ssp_op_track_class_votes: once per frame, beside ssp_op_world_insert and with its landmarks_dev / n_landmarks_dev / row_cap /
 *   count_new_dev / point_cap; cls_new_dev uint8 [point_cap]: the class of every point of the newest frame.  A landmark row (track
 *   id t, newest-frame index p) takes part iff 0 <= p < count, 0 <= t < tid_cap and c = cls_new[p] != SSP_CLASS_NONE (the insert's
 *   test without X).  Boyer-Moore majority step on votes[t]: count 0 -> (c, 1); the same class -> count = min(count + 1, 255);
 *   another class -> count - 1, the class byte kept.  Track ids must be unique within a call.
 * ssp_op_world_classes: out_dev uint8 [map_cap] = the decoded class of tid_dev[i] for i < n_rows (state_dev[0], clamped),
 *   SSP_CLASS_NONE past that and for a track id outside [0, tid_cap).
 * ssp_match_world_classes: ssp_match_world with one more condition.  With class(i) the decoded class of map row i's track, the pair
 *   (i, j) is a candidate iff class(i) == cls2_dev[j], class(i) != SSP_CLASS_NONE and bit class(i) of keep_mask (256 bits on the
 *   HOST, ssp_op_filter_points' layout) is set; any other pair takes part in neither arg-min, and a row or column without a
 *   candidate gives no match.  With every class equal, known and kept the output is bit-identical to ssp_match_world's.
 *   workspace_dev: ssp_match_world_workspace_bytes(map_cap, cap) bytes. */
int ssp_op_track_class_votes(const double* landmarks_dev, const int32_t* n_landmarks_dev, int row_cap, const uint8_t* cls_new_dev,
                             const int32_t* count_new_dev, int point_cap, uint16_t* votes_dev, int tid_cap, void* stream);
int ssp_op_world_classes(const int32_t* tid_dev, const int32_t* state_dev, int map_cap, const uint16_t* votes_dev, int tid_cap,
                         uint8_t* out_dev, void* stream);
int ssp_match_world_classes(const float* desc_dev, const int32_t* tid_dev, const int32_t* state_dev, int map_cap,
                            const uint16_t* votes_dev, int tid_cap, const float* desc2_dev, const uint8_t* cls2_dev,
                            const int32_t* count2_dev, int cap, const uint32_t keep_mask[8], float nn_thresh, void* workspace_dev,
                            float* match_dev, int32_t* n_match_dev, void* stream);

/* ---- trajectory evaluation -----------------------------------------------------------------------
 * A trajectory table against ground-truth poses: the alignment, the absolute and the relative pose errors, and their statistics.
 * The rules are restated in numpy by tests/traj_eval_ref.py.  fp64 without contraction, no floating-point atomics, every sum in one
 * fixed order (thread t of 256 takes the rows t, t + 256, ..., then the wave butterfly and the waves in order), one workgroup per
 * problem wherever a sum is taken: a problem's result does not depend on its batch or on the run.  No call synchronises with the
 * host, allocates or needs a workspace.
 * The arguments every call shares: n_problems = P tables against one or P ground truths.
 *   table_dev fp64 [P][table_stride][SSP_POSE_ROW_WORDS], table_stride >= capacity rows: rows (Rw [9], C [3], s, n_shared, flags,
 *     ratio), Rw world-to-camera, so that the estimate's camera-to-world rotation is Rw^T; n_frames_dev int32 [P] on the device.
 *   gt_dev fp64 [P or 1][gt_stride][SSP_TRAJ_GT_WORDS]: the row-major 3x4 camera-to-world matrix (R | C) per row, the layout of a
 *     KITTI poses file; n_gt rows; gt_stride 0: one ground truth shared by all problems, else >= n_gt rows per problem.
 *   index_dev int32 [capacity] or NULL: the ground-truth row of frame f, -1 for none; NULL: frame f is row f.
 *   Frame f is valid iff f < min(n_frames, capacity), its ground-truth row g exists (0 <= g < n_gt), its flag word is an integer
 *     in [0, 2^31) with (flags & skip_flags) == 0, and all 12 + 12 numbers (Rw, C; R, C of the truth) are finite.
 * ssp_op_traj_align: sim_dev [P][SSP_TRAJ_SIM_WORDS] = (s, R [9], t [3], n_valid, status, sigma_p^2) of q ~ s R p + t over the valid
 *   frames, p the estimated and q the true centres.  mode 0: SE(3) (s = 1), 1: Sim(3): two passes (the means; H = sum (q - mq)
 *   (p - mp)^T, Sp = sum |p - mp|^2), eight cyclic Jacobi sweeps on H^T H, v0 / v1 the columns of the two largest diagonal
 *   entries (the lowest index on ties), v2 = v0 x v1, u0 = H v0 / |.|, u1 = H v1 made orthogonal to u0 and normalised, u2 = u0 x u1,
 *   R = sum u_k v_k^T, s = sum_ij R_ij H_ij / Sp, t = mq - s R mp; sigma_p^2 = Sp / n_valid.  mode 2: R = R_gt Rw and t = q - R p
 *   of the first valid frame, s = 1; mode 3: the same R and s = sum q'.p' / sum p'.p', q' = q - q0, p' = R (p - p0).
 *   status 1: fewer than 3 valid frames (mode 2: 1, mode 3: 2), Sp <= 0, a moment or a result that is not finite or s <= 0;
 *   status 2: centres collinear (the second-largest diagonal entry <= 1e-24 x the largest).  Both write s = 1, R = I, t = 0.
 * ssp_op_traj_ape: per frame err_t = |q - (s R p + t)|, err_r = the angle of R_gt^T (R Rw^T) in degrees, valid; [P][capacity],
 *   every entry written; 0 / 0 / 0 for an invalid frame or a sim row with status != 0.  The angle of a rotation E is
 *   atan2(0.5 sqrt((E21-E12)^2 + (E02-E20)^2 + (E10-E01)^2), 0.5 (tr E - 1)) everywhere.
 * ssp_op_traj_rpe_delta: for f and f + delta both valid, E = (P_f^-1 P_g)^-1 (Q_f^-1 Q_g), Q the truth, P the estimate with centres
 *   scaled by scale_dev[p * scale_stride] (NULL: 1; sim_dev with stride SSP_TRAJ_SIM_WORDS passes an alignment's s);
 *   err_t = |trans E|, err_r = its angle in degrees, valid; [P][capacity].
 * ssp_op_traj_rpe_segments (the KITTI devkit's rules): dist_dev [P][capacity] = the cumulative path length over the ground-truth
 *   rows of frames 0..f (an order-defined scan; a frame without a row, or whose centre is not finite, repeats the value before it).
 *   For every first frame f0 = 0, step, 2 step, ... below capacity and every length L of lengths_dev fp64 [n_len], f1 = the first
 *   frame with dist[f1] > dist[f0] + L (binary search), -1 if none or f0 >= n_frames.  seg_dev [P][cdiv(capacity, step)][n_len][4]
 *   = (f1, t_err / L, r_err / L, L) for a segment that counts (f1 >= 0, both ends valid; r_err in radians), (f1, 0, 0, 0)
 *   otherwise.  summary_dev [P][2 + 3 n_len] = mean t_err / L, mean r_err / L over all counted segments, then (count, mean, mean)
 *   per length.  info_dev int32 [P][SSP_TRAJ_INFO_WORDS] = (counted, segments whose end exists but an end is invalid, first frames
 *   without an end, first frames inside the sequence).
 * ssp_op_traj_stats: err_dev fp64 / valid_dev int32 [P][capacity] (errors non-negative and finite where valid) ->
 *   stats_dev [P][SSP_TRAJ_STATS_WORDS] = (n, rmse, mean, std (population), min, max, median (numpy's: the mean of the two middle
 *   order statistics), sse); the order statistics by an exact radix select over the bit patterns; n = 0 gives zeros. */
#define SSP_TRAJ_GT_WORDS 12
#define SSP_TRAJ_SIM_WORDS 16
#define SSP_TRAJ_STATS_WORDS 8
#define SSP_TRAJ_INFO_WORDS 4
#define SSP_TRAJ_MAX_LENGTHS 8
#define SSP_TRAJ_MAX_FRAMES (1 << 20)
#define SSP_TRAJ_MAX_PROBLEMS 65535
int ssp_op_traj_align(const double* table_dev, int table_stride, const int32_t* n_frames_dev, int capacity, const double* gt_dev,
                      int gt_stride, int n_gt, const int32_t* index_dev, int skip_flags, int mode, int n_problems, double* sim_dev,
                      void* stream);
int ssp_op_traj_ape(const double* table_dev, int table_stride, const int32_t* n_frames_dev, int capacity, const double* gt_dev,
                    int gt_stride, int n_gt, const int32_t* index_dev, int skip_flags, int n_problems, const double* sim_dev,
                    double* err_t_dev, double* err_r_dev, int32_t* valid_dev, void* stream);
int ssp_op_traj_rpe_delta(const double* table_dev, int table_stride, const int32_t* n_frames_dev, int capacity, const double* gt_dev,
                          int gt_stride, int n_gt, const int32_t* index_dev, int skip_flags, int n_problems, const double* scale_dev,
                          int scale_stride, int delta, double* err_t_dev, double* err_r_dev, int32_t* valid_dev, void* stream);
int ssp_op_traj_rpe_segments(const double* table_dev, int table_stride, const int32_t* n_frames_dev, int capacity, const double* gt_dev,
                             int gt_stride, int n_gt, const int32_t* index_dev, int skip_flags, int n_problems, const double* scale_dev,
                             int scale_stride, const double* lengths_dev, int n_len, int step, double* dist_dev, double* seg_dev,
                             double* summary_dev, int32_t* info_dev, void* stream);
int ssp_op_traj_stats(const double* err_dev, const int32_t* valid_dev, int capacity, int n_problems, double* stats_dev, void* stream);

/* ---- loop closure --------------------------------------------------------------------------------
 * A frame's map matches against the OLD rows of the world map, the loop edge measured from the pose found against them, a Sim(3)
 * pose graph over the trajectory rows since the old place was last seen, and the write-back.  The rules are restated in numpy by
 * tests/loop_ref.py.  fp64 without contraction, no floating-point atomics, every sum in one fixed order.  No call synchronises with
 * the host or allocates.  One sequence per call.
 * ssp_op_loop_correspondences: ssp_op_world_correspondences restricted to match rows whose map row has last_frame <= f - min_gap,
 *   plus xnew_dev [cap][4] = (X of the lowest landmark row whose eighth word is the row's frame point, 1) or zero, and n_dev [3] =
 *   (rows, valid old rows, valid old rows with a landmark).  landmarks_dev [row_cap][SSP_LANDMARK_WORDS] / n_landmarks_dev [1] of
 *   ssp_op_landmarks_select for the window ending at frame f.
 * ssp_loop_edge: one candidate edge from the pose of ssp_pnp_ransac on those rows (rw_dev [9], c_dev [3], mask_dev [cap],
 *   status_dev [1]).  Anchor a = the largest last_frame over the inlier rows; sigma = (sum of the inliers' depths under the loop
 *   pose) / (sum of the depths of their window landmarks under row f), ssp_pose_chain's statistic, accepted when at least 8 inliers
 *   have a landmark and it is finite and positive.  Refused (state word 2) unless status 0 and finite, inliers >= min_inliers, the
 *   scale rule, 0 <= a < f, f - (frame of the last accepted edge) >= cooldown; dropped (word 3) when the table is full.  An accepted
 *   edge (a, f, R [9] = Rw_L Rw_a^T, t [3] = Rw_a (C_L - C_a), log sigma, weight) is appended to edges_dev
 *   [SSP_LOOP_MAX_EDGES][SSP_LOOP_EDGE_WORDS].  state_dev int32 [SSP_LOOP_STATE_WORDS] = (edges, frame of the last accepted edge,
 *   refused, dropped, accepted by this call, its anchor, its inliers, map rows ssp_loop_apply left alone because the result was not
 *   finite); cand_dev fp64 [SSP_LOOP_CAND_WORDS] = (f, a, inliers, shared depths, sigma, angle of R_c, |t_c|, accepted, reason).
 * ssp_pose_graph: Levenberg-Marquardt (`iterations` steps, lambda from 1e-4, /10 on an accepted step, x10 otherwise) over the rows
 *   a + 1 .. f with row a and every earlier row fixed; runs only when the last ssp_loop_edge accepted.  rw_out_dev [capacity][9],
 *   c_out_dev [capacity][3], sigma_out_dev [capacity]: copies of the table (sigma 1) with the free rows replaced under status 0.
 *   info_dev fp64 [SSP_LOOP_INFO_WORDS] = (status, cost before, cost after, nodes, edges used, accepted steps, both-ends-free edges
 *   left out, lambda); status 1: nothing to do, 2: no step accepted.  workspace_dev: ssp_pose_graph_workspace_bytes(capacity).
 * ssp_loop_apply: under status 0, rows a + 1 .. f take the corrected Rw and C, s = |C_k - C_(k-1)| when finite and above 1/64 of
 *   the row's s, and SSP_POSE_FLAG_LOOP; the chain state follows row f when that is its newest frame and the table is not full; a map
 *   row with last_frame = k in (a, f] becomes C'_k + sigma_k R'_k^T R_k (X - C_k). */
#define SSP_LOOP_MAX_EDGES 256
#define SSP_LOOP_EDGE_WORDS 16
#define SSP_LOOP_STATE_WORDS 8
#define SSP_LOOP_CAND_WORDS 16
#define SSP_LOOP_MAX_INNER 8
#define SSP_LOOP_INFO_WORDS 8
#define SSP_LOOP_MAX_ITERATIONS 64
#define SSP_POSE_FLAG_LOOP 32
size_t ssp_pose_graph_workspace_bytes(int capacity);
int ssp_op_loop_correspondences(const double* x_dev, const int32_t* last_dev, const int32_t* state_dev, int map_cap,
                                const float* match_dev, const int32_t* n_match_dev, int cap, const double* pts_new_dev, int pt_stride,
                                const int32_t* count_new_dev, int point_cap, const double* landmarks_dev,
                                const int32_t* n_landmarks_dev, int row_cap, int f, int min_gap, double* corr_dev, double* xnew_dev,
                                int32_t* n_dev, void* stream);
int ssp_loop_edge(const double* rw_dev, const double* c_dev, const uint8_t* mask_dev, const int32_t* status_dev,
                  const double* corr_dev, const double* xnew_dev, const int32_t* n_dev, int cap, const int32_t* last_dev, int map_cap,
                  const double* table_dev, int capacity, int f, int min_inliers, int cooldown, double weight, double* edges_dev,
                  int32_t* state_dev, double* cand_dev, void* stream);
int ssp_pose_graph(const double* table_dev, int capacity, const double* edges_dev, const int32_t* state_dev, int f, int iterations,
                   void* workspace_dev, double* rw_out_dev, double* c_out_dev, double* sigma_out_dev, double* info_dev, void* stream);
int ssp_loop_apply(const double* info_dev, const double* rw_new_dev, const double* c_new_dev, const double* sigma_dev,
                   int32_t* loop_state_dev, int f, double* state_dev, double* table_dev, int capacity, double* x_dev,
                   const int32_t* last_dev, const int32_t* world_state_dev, int map_cap, void* stream);

/* ---- streamed descriptor metrics----------------------------------------------------------
 * The per-pair metrics of evaluation.py -r -homo for a set that is fed batch by batch and never leaves the device, on
 * top of ssp_eval_repeatability, ssp_match_two_way and ssp_eval_ransac.  fp64 without contraction.  No call
 * synchronises with the host.
 * ssp_eval_pixel_homographies: hn_dev float32 [n_pairs][9], the trainer's normalised image-to-warped homographies
 *   (sample["homographies"]), widened to fp64 -> hom_dev = Tinv @ (Hn @ T) with T = [[2/W,0,-1],[0,2/H,-1],[0,0,1]]
 *   (2/W, 2/H correctly rounded) and Tinv = [[W/2,0,W/2],[0,H/2,H/2],[0,0,1]] (utils/utils.py:291-294
 *   homography_scaling in closed form; no division by h33); every element ((a0*b0 + a1*b1) + a2*b2), each product and
 *   each sum rounded.  hom_inv_dev = adj(M) / det(M): each cofactor a rounded p*q - r*s,
 *   det = ((m00*A00 + m01*A10) + m02*A20), nine divisions.  This is NOT np.linalg.inv (an LU solve): the two agree to
 *   about 5e-16 relative, not bit for bit.  Both outputs fp64 [n_pairs][9].
 * ssp_eval_accumulate: one workgroup, 1 <= n_pairs <= SSP_EVAL_ACC_MAX_PAIRS.  rep_dev: the [n_pairs][8] rows of
 *   ssp_eval_repeatability, or NULL (repeatability off; n_unwarped counts as 0).  h_dev / n_inlier_dev / status_dev: the
 *   crossCheck call of ssp_eval_ransac; ap_dev: the nn call's; n1_dev: the image-side point counts (pair p reads entry
 *   p * pair_stride); hom_dev: the true pixel homographies [n_pairs][9]; these six come together, or all NULL (homography
 *   metrics off).  The slots of a group that is off stay 0.  thresholds: 6 doubles (host).  Pair p has the number
 *   first_pair + p and writes the row of that number in rows_dev [capacity][SSP_EVAL_ROW_WORDS] (skipped, and counted in
 *   the state, when the number >= capacity):
 *     0 rep = c / (N1 + N2), c = count1 + count2 (0 when c = 0)   1 loc_err = 0 + sum1 / c + sum2 / c (-1 when c = 0)
 *     2..7 mean corner distance <= threshold k, as 0 / 1 (all 0 with status 1)
 *     8 mscore = 2 n_inliers / (n1 + n_unwarped) (0 for a zero denominator)   9 mAP = ap if ap > 0 else 0
 *     10 status   11 n_inliers   12 n1   13 n_unwarped   14 the mean corner distance (inf without a model)   15 pair number
 *   A corner is ((x*h0 + y*h1) + h2, (x*h3 + y*h4) + h5) / ((x*h6 + y*h7) + h8) for (0, 0), (0, ch - 1), (cw - 1, 0),
 *   (cw - 1, ch - 1); the distance sqrt(dx*dx + dy*dy); the mean (((d0 + d1) + d2) + d3) / 4.
 *   state_dev [SSP_EVAL_STATE_WORDS] fp64, caller-owned, zeroed = empty; one lane adds the rows in pair order, so the state
 *   of a set does not depend on how it was split into calls:
 *     0 pairs   1 sum rep   2 sum loc_err over loc_err > 0   3 their count   4..9 correct counts   10 sum mscore   11 sum mAP
 *     12 pairs without a model   13 rows dropped (pair number >= capacity)   14, 15: 0. */
#define SSP_EVAL_ACC_MAX_PAIRS 128
#define SSP_EVAL_ROW_WORDS 16
#define SSP_EVAL_STATE_WORDS 16
int ssp_eval_pixel_homographies(const float* hn_dev, int n_pairs, int height, int width, double* hom_dev, double* hom_inv_dev,
                                void* stream);
int ssp_eval_accumulate(const double* rep_dev, const double* h_dev, const int32_t* n_inlier_dev, const int32_t* status_dev,
                        const double* ap_dev, const int32_t* n1_dev, int pair_stride, const double* hom_dev, int n_pairs,
                        int corner_h, int corner_w, const double* thresholds, int64_t first_pair, double* rows_dev,
                        int64_t capacity, double* state_dev, void* stream);

/* ---- detector evaluation against ground-truth corners (evaluations/detector_evaluation.py:15-136) --
 * compute_tp_fp / compute_pr / compute_mAP / compute_loc_error for a validation set that is fed batch by batch and never
 * leaves the device.  The caller owns a key buffer int64 [capacity] and a state block int64 [SSP_DET_EVAL_STATE_WORDS]
 * (zeroed = empty): word 0 records fed so far (counts past capacity too), word 1 n_gt, word 2 != 0 after an overflow,
 * word 3 point-list rows that were skipped because they lie outside the image (a mis-scaled list shows here),
 * words 8 .. 8 + SSP_DET_EVAL_MAX_R2: number of predictions above prob_thresh whose nearest ground-truth point is at squared
 * distance d2 (compute_loc_error = sum(count[d2] * sqrt(d2)) / sum(count), formed in fp64 by the caller).
 * Labels are [b][height][width], fp32 (labels_u8 == 0) or uint8, nonzero = ground truth.  r2 is the largest integer d2 with
 * sqrt((double)d2) <= distance_thresh, computed by the caller: the kernels compare integers only.
 * ssp_op_det_tp_fp: candidates are the pixels of prob_dev [b][height][width] with prob > remove_zero (fp32 compare), in
 *   image order, then row-major.  A candidate is assigned to the FIRST label pixel, in row-major order, within r2 (np.argmax of
 *   the reference's match row: not the nearest) and is a true positive iff it has the largest (probability, position) among
 *   the candidates assigned to that pixel.  simplified != 0 (the reference's flag): tp = any label pixel within r2, and n_gt
 *   counts the label pixels within r2 of some candidate.  Candidate k of the call becomes record (word 0) + k and writes
 *   keys_dev[record] = prob bits << 32 | record << 1 | tp; every key is unique, so a descending sort of the keys is the order
 *   "descending probability, among equals the later record first" whatever sort produces it.  Record positions come from a
 *   prefix scan, not an atomic ticket: the keys are bit-identical from run to run and for any split of a set into calls.
 *   A record >= capacity sets word 2 and is not written.
 * ssp_op_det_tp_fp_points: the same for point lists pts_dev [b][cap][5] rows (x, y, confidence, ..) with count_dev [b] (clamped
 *   to cap) as ssp_op_heatmap_points / ssp_describe_points write them: the candidates are the rows < count with confidence >
 *   remove_zero at the integer pixel (x, y), in list order (rows outside the image are skipped).
 * ssp_op_det_pr_curve: compute_pr + compute_mAP over n_records keys sorted in DESCENDING order (as signed or unsigned 64-bit
 *   integers: bit 63 is never set): prob_dev [n] fp32, tp_dev [n] uint8, precision_dev / recall_dev [n + 2] fp64 with the
 *   reference's padding (recall 0 .. 1, precision 0 .. 0), the running maximum of precision from the right, recall by div0's
 *   rule when n_gt == 0 (1 where tp_cum == 0, else 0), and map_dev [1] = sum(precision[1:] * (recall[1:] - recall[:-1])).
 *   fp64 without contraction; every element equals numpy's except map_dev, whose summation order differs.
 *   n_records == 0 gives precision [0, 0], recall [0, 1], mAP 0.
 * Bad arguments (r2 > SSP_DET_EVAL_MAX_R2, remove_zero < 0, prob_thresh < remove_zero, capacity or batch x pixels >= 2^31,
 * ..) return -1 with ssp_last_error before anything is launched.  No call synchronises with the host.  workspace_dev: ssp_det_eval_workspace_bytes(p, b, cap) bytes (cap = 0 for
 * the dense form) / ssp_det_pr_curve_workspace_bytes(n_records) bytes; 0 = bad arguments. */
#define SSP_DET_EVAL_MAX_R2 64
#define SSP_DET_EVAL_STATE_WORDS 80
#define SSP_DET_EVAL_CURVE_TILE 1024 /* records per workgroup of the curve kernels (tests place record counts around it) */
typedef struct ssp_det_eval_params {
  int32_t height, width;
  float remove_zero;  /* compute_tp_fp's remove_zero (1e-4), >= 0 */
  int32_t r2;         /* squared match radius, 0 .. SSP_DET_EVAL_MAX_R2 */
  float prob_thresh;  /* compute_loc_error's prob_thresh (0.5), >= remove_zero: only candidates are measured */
  int32_t simplified; /* compute_tp_fp's simplified */
} ssp_det_eval_params;
size_t ssp_det_eval_workspace_bytes(const ssp_det_eval_params* p, int b, int cap);
int ssp_op_det_tp_fp(const float* prob_dev, const void* labels_dev, int labels_u8, const ssp_det_eval_params* p, int b,
                     void* workspace_dev, int64_t* keys_dev, int64_t capacity, int64_t* state_dev, void* stream);
int ssp_op_det_tp_fp_points(const float* pts_dev, const int32_t* count_dev, int cap, const void* labels_dev, int labels_u8,
                            const ssp_det_eval_params* p, int b, void* workspace_dev, int64_t* keys_dev, int64_t capacity,
                            int64_t* state_dev, void* stream);
size_t ssp_det_pr_curve_workspace_bytes(int64_t n_records);
int ssp_op_det_pr_curve(const int64_t* sorted_keys_dev, int64_t n_records, const int64_t* state_dev, void* workspace_dev,
                        float* prob_dev, uint8_t* tp_dev, double* precision_dev, double* recall_dev, double* map_dev,
                        void* stream);

/* ---- point tracks over a frame sequence (PointTracker.update / get_tracks, models/model_wrap.py:521-615) ----------
 * The track table of max_length = L frames lives in caller-owned arrays of row_cap rows: ids [row_cap][L] int32 (point id
 * of retained frame 0 .. L-1, oldest first, -1 = none), tid [row_cap] int32 (track id), score [row_cap] fp64 (running mean
 * of the match distances, 9999 = no match yet) and a state vector int32 [2 + L] = n_rows, track_count, point count of each
 * retained frame.  An empty tracker is a zeroed state vector.  2 <= L <= SSP_TRACK_MAX_LENGTH, 1 <= point_cap <=
 * SSP_MATCH_MAX_POINTS points per frame, row_cap >= L * point_cap (every point of the retained frames may own a row).
 * The rules are DESIGN.md section 17; results are bit-identical from run to run.
 * ssp_op_track_update: one PointTracker.update from the *_in arrays into the *_out arrays (never in place): n_points_dev [1]
 *   points in the new frame, match_dev [point_cap][3] float rows (i, j, distance) with n_match_dev [1] rows as
 *   ssp_match_two_way writes them (i indexes the previous frame = the last frame of state_in, j the new one);
 *   match_score64_dev (may be NULL): fp64 distances [point_cap] that replace column 2 (a host matcher's float64 scores).
 *   The mean is updated in fp64 as (1 - 1/len) * old + (1/len) * d without contraction.
 * ssp_op_track_select: get_tracks(min_length): the rows with at least min_length ids != -1 and a last id != -1, in table
 *   order, as the reference's fp64 matrix tracks_dev [row_cap][2 + L] = (track id, score, ids), n_tracks_dev [1].
 *   min_length == 0 returns every row (the reference's `tracker.tracks`).
 * ssp_op_track_points: the coordinates a tracks matrix names (the index arithmetic of draw_tracks): tracks_dev
 *   [track_cap][2 + L] fp64 with n_tracks_dev [1] rows, pts_dev [L][point_cap][2] fp64 (x, y) used as a ring: retained frame c
 *   lives in slot (first_slot + c) % L; state_dev gives the frame counts.  xy_dev [track_cap][L][2] fp64, NaN where the id
 *   is -1 (rows >= n_tracks are not written).
 * workspace_dev: ssp_track_workspace_bytes(L, point_cap, row_cap) bytes serve update and select (0 = bad arguments). */
#define SSP_TRACK_MAX_LENGTH 16
size_t ssp_track_workspace_bytes(int max_length, int point_cap, int row_cap);
int ssp_op_track_update(const int32_t* ids_in_dev, const int32_t* tid_in_dev, const double* score_in_dev,
                        const int32_t* state_in_dev, const float* match_dev, const double* match_score64_dev,
                        const int32_t* n_match_dev, const int32_t* n_points_dev, int max_length, int point_cap, int row_cap,
                        void* workspace_dev, int32_t* ids_out_dev, int32_t* tid_out_dev, double* score_out_dev,
                        int32_t* state_out_dev, void* stream);
int ssp_op_track_select(const int32_t* ids_dev, const int32_t* tid_dev, const double* score_dev, const int32_t* state_dev,
                        int max_length, int row_cap, int min_length, void* workspace_dev, double* tracks_dev,
                        int32_t* n_tracks_dev, void* stream);
int ssp_op_track_points(const double* tracks_dev, const int32_t* n_tracks_dev, const double* pts_dev, const int32_t* state_dev,
                        int max_length, int point_cap, int track_cap, int first_slot, double* xy_dev, void* stream);

/* BatchNorm2d(train) (+ReLU (+MaxPool2d(2))) backward. y: raw conv output NHWC; dout: gradient wrt the activated
 * (and pooled) output; stats4 = scale|shift|mean|invstd ([4*C]); dgamma/dbeta/dbias are accumulated;
 * sums_dev: double [SSP_NREP][2*C] scratch. */
int ssp_op_bn_bwd(const float* y_dev, const float* dout_dev, const float* gamma_dev, const float* stats4_dev,
                  float* dy_dev, float* dgamma_dev, float* dbeta_dev, float* dbias_dev, double* sums_dev, int n, int h,
                  int w, int c, int relu, int pool, void* stream);
/* The same on channel-padded NHWC tensors (pixel stride cs >= c, cs % 4 == 0: the 65-channel detector head lives in
 * 68-float pixels); the per-channel vectors stay [c]. */
int ssp_op_bn_bwd_strided(const float* y_dev, const float* dout_dev, const float* gamma_dev, const float* stats4_dev,
                          float* dy_dev, float* dgamma_dev, float* dbeta_dev, float* dbias_dev, double* sums_dev, int n,
                          int h, int w, int c, int cs, int relu, int pool, void* stream);

/* Algorithm of the 3x3 forward / data-gradient convolutions whose input channels are a multiple of 16 (process-wide
 * DEFAULT, copied into a handle at ssp_create; takes effect at the next forward, which re-packs the weights): 1 (default) = Winograd on the fp32 matrix
 * cores, fp32 throughout: F(4x4,3x3) (4x fewer multiplies, conv_wino4_kernel) on maps of >= 60x80 pixels with >= 4 tile
 * blocks per CU, F(2x2,3x3) (2.25x fewer, software-pipelined kernel whose weight fragments come straight from L2)
 * elsewhere; results within ~2e-6 / ~3e-7 relative of the direct form, 6 = the two-workgroups-per-CU F(2x2,3x3) pipeline
 * everywhere, 9 = F(2x2,3x3) only (the default of rounds 1-2), 10 = F(4x4,3x3) wherever legal (tests), 11 = algorithm 1 with
 * the Winograd F(3x3,4x4) weight gradient, 0 = direct implicit GEMM,
 * 12 = the bf16 PATH (BASELINE configs[3], bench.py --dtype bf16): bf16 NHWC activations and activation gradients in HBM, direct
 * bf16 matrix-core 3x3 convolutions, fp32 master weights, BatchNorm statistics, losses and Adam; the handle-less ssp_op_conv
 * refuses a 3x3 convolution with Cin % 16 == 0 under it (-3: that case is ssp_op_conv_bf16's).
 * 2, 3, 5, 7 and 8 (experiments of rounds 1-3) are retired: both setters refuse them (-1). */
int ssp_set_conv_algo(int algo);
/* the same choice for ONE handle (a new handle starts with the process-wide value of ssp_set_conv_algo, which also
 * governs the handle-less ssp_op_conv / ssp_op_conv_wgrad) */
int ssp_handle_set_conv_algo(ssp_handle* h, int algo);

/* perf-debug hook: ablate bits (1 no global loads, 2 no LDS writes, 4 no stores, 8 no MFMA) and grid override of
 * conv_mfma_kernel; (0, 0) restores the product behaviour. */
int ssp_debug_conv_knobs(int ablate, int grid);
/* perf-debug hook: workgroups per CU admitted by hipOccupancyMaxActiveBlocksPerMultiprocessor for a kernel family
 * (0 conv_wino_p2_kernel, 1 conv_wino_pipe_kernel, 2 wgrad_wino_kernel); negative = error */
int ssp_debug_occupancy(int which);

/* test hook: device pointer of an internal buffer ("gP","gQ","dsemi","ddesc","desc","dsout","Y<l>","A<l>" (pooled copy of layer l),
 * "scale<l>","shift<l>","mean<l>","invstd<l>"); under the bf16 path Y<l> / A<l> of the 3x3 layers, gP and gQ hold bf16 elements */
int ssp_debug_buffer(ssp_handle* h, int slot, const char* name, float** ptr, size_t* nfloats);

/* test hook: backward taps.  With a caller-owned device arena (arena_dev != NULL, at least
 * ssp_debug_backward_tap_floats(h, layer_mask) floats) the backward (ssp_pair_step eager, ssp_backward) copies, on the
 * step's stream, per layer l of layer_mask (bit l) and view: which = 0, dOut_l (gradient wrt the layer's (pooled) activation as it
 * enters its BatchNorm backward), which = 1, dY_l (gradient wrt its conv output after the BatchNorm backward APPLY; none for
 * layer 0).  Layer 8 stands for the three 3x3 heads: their whole [cells][256 heads] tensors; layers 9 / 11 (Pb / Db): dY only.
 * NHWC, sized for the handle's max_batch.  Conv algorithm 12 (the bf16 path): the taps of its bf16 tensors (every encoder tap,
 * both layer-8 taps) hold bf16 elements in the first half of their slice; Pb / Db dY stay fp32.  arena_dev == NULL: off (no
 * extra launch).  ssp_pair_step_graph refuses to run with taps on.  ssp_debug_backward_tap: arena offset and size (floats) of
 * one tap's slice (0 / 0 when not tapped) and `route`, the path layer l took in the last backward pass (kept with taps off too):
 * bit 0 pass 1 of the BatchNorm backward (S1 / S2 sums) accumulated by the data gradient above, bit 1 APPLY fused into the
 * weight gradient, bit 2 replica reduction in the weight gradient's prologue, bit 3 (bf16 path) weight-gradient operand read
 * from the activation the forward materialised; bits 4-7 weight-gradient kernel (1 wgrad_wino_fused, 2 wgrad_wino,
 * 3 wgrad_wino4, 4 direct, 5 grouped pointwise, 6 bn_bwd_apply_l0, 7 wgrad_bf16); bits 8-11 data-gradient kernel (1 conv_wino4,
 * 2 conv_wino_pipe, 3 conv_wino_p2, 4 direct, 5 grouped pointwise, 6 conv_bf16, 7 conv_bf16_ws). */
int ssp_debug_backward_taps(ssp_handle* h, float* arena_dev, size_t arena_floats, unsigned layer_mask);
size_t ssp_debug_backward_tap_floats(const ssp_handle* h, unsigned layer_mask);
int ssp_debug_backward_tap(ssp_handle* h, int slot, int layer, int which, size_t* offset, size_t* nfloats, unsigned* route);

/* batch_descriptor_loss_sparse (utils/loss_functions/sparse_loss.py:267-284) on NHWC descriptor maps [B][hc*wc][256] with explicit
 * indices; out2_dev = {mean positive_dist, mean negative_dist}.  method: 0 = "2d" (bilinear grid_sample at normPts), 1 = "1d"
 * (index_select at the cell); dist: 0 = "cos", 1 = "euclidean" (pixelwise_contrastive_loss.py:140,185-210,247-258).  With dd_a /
 * dd_b (both or none; same layout, OVERWRITTEN) also the gradient of coef_pos * positive_dist + coef_neg * negative_dist. */
int ssp_op_sparse_loss(const float* desc_a_nhwc_dev, const float* desc_b_nhwc_dev, const int32_t* match_a_dev,
                       const int32_t* match_b_dev, const int32_t* nonmatch_b_dev, int b, int hc, int wc, int n_match,
                       int n_non, int method, int dist, float coef_pos, float coef_neg, float* dd_a_nhwc_dev, float* dd_b_nhwc_dev,
                       float* out2_dev, void* stream);
/* The same with the path of the match term's gradient chosen by the caller.  gather: 1 = per-cell gather over corner lists (two
 * gradient rows per match, no atomics for the match term: a fixed summation order), 0 = atomic scatter, -1 = the process default
 * (SSP_DESC_GATHER, default 1).  csr_*_dev (all three or none; gather path with gradients only) receive the corner lists: for
 * list = image * 2 + side, csr_off [b * 2][hc * wc + 1] offsets per cell, csr_match / csr_weight [b * 2][4 * n_match] the match
 * index and bilinear weight of every corner with a non-zero weight, sorted by cell and, within a cell, by match index. */
int ssp_op_sparse_loss_path(const float* desc_a_nhwc_dev, const float* desc_b_nhwc_dev, const int32_t* match_a_dev,
                            const int32_t* match_b_dev, const int32_t* nonmatch_b_dev, int b, int hc, int wc, int n_match,
                            int n_non, int method, int dist, float coef_pos, float coef_neg, float* dd_a_nhwc_dev, float* dd_b_nhwc_dev,
                            float* out2_dev, int gather, int32_t* csr_off_dev, int32_t* csr_match_dev, float* csr_weight_dev,
                            void* stream);

/* Dense descriptor loss as an operator (utils/utils.py:779-893) on NHWC descriptor maps [B][hc*wc][256]:
 * out3_dev = {loss_desc, pos_sum, neg_sum}; with dda_dev / ddb_dev (both or none) also the gradients of
 * scale * loss_desc (multi_task == 0) or scale * (pos_sum + neg_sum) (multi_task != 0) wrt both maps.
 * scratch: 64 KiB + B * cells * cells floats when gradients are requested. */
int ssp_op_dense_loss(const float* desc_a_nhwc_dev, const float* desc_b_nhwc_dev, const float* homographies_dev,
                      const float* valid_dev, int b, int hc, int wc, float lamda_d, float descriptor_dist, int multi_task,
                      float scale, void* scratch_dev, size_t scratch_bytes, float* out3_dev, float* dda_dev,
                      float* ddb_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSP_HIP_H */
