// Operator-level C entry points: the handle-less operators and the handle read-outs that forward to them.  Included by ssp.hip
// inside an extern "C" block, after the engine: it uses ssp.hip's helpers (fail, CHK, HIPCHK, launch, launch_lds, DevTemps, Carver,
// cdiv, align_up, device_cu_count) and launchers.  Every entry point refuses first (the family check, then scalar ranges, then null
// pointers, then aliasing), then carves its workspace, then launches: nothing is allocated or launched before the last refusal
// (DESIGN.md section 38).
#pragma once

// ---- argument predicates shared by several families: each names its caller (`what`) and the faulty argument ----
// rows of a track table, and of everything derived from one (landmark lists, world inserts, loop joins)
constexpr int ROW_CAP_MAX = SSP_TRACK_MAX_LENGTH * SSP_MATCH_MAX_POINTS;
// point sets of n_pairs pairs, `cap` rows each, every pair_stride-th set of the point arrays (the matchers, the evaluation)
static int pairs_check(const char* what, int cap, int n_pairs, int pair_stride) {
  if (cap < 1 || cap > SSP_MATCH_MAX_POINTS || n_pairs < 1 || pair_stride < 1)
    return fail(-1, "%s: 1 <= cap <= %d, n_pairs >= 1, pair_stride >= 1 required (cap %d)", what, SSP_MATCH_MAX_POINTS, cap);
  return 0;
}
// one intrinsics row for all n problems (`of_what` names them), or one each
static int intr_check(const char* what, int n_intr, int n, const char* n_name, const char* of_what) {
  if (n_intr != 1 && n_intr != n) return fail(-1, "%s: n_intr must be 1 or %s (got %d for %d %s)", what, n_name, n_intr, n, of_what);
  return 0;
}
static int finite_nonneg_check(const char* what, const char* name, double x) {
  if (!(x >= 0.0) || !std::isfinite(x)) return fail(-1, "%s: a finite %s >= 0 is required", what, name);
  return 0;
}
// n_seq pose chains and the rows of their trajectory tables
static int seq_check(const char* what, int n_seq, int capacity) {
  if (n_seq < 1 || n_seq > 65535 || capacity < 0)
    return fail(-1, "%s: 1 <= n_seq <= 65535 and capacity >= 0 required (n_seq %d, capacity %d)", what, n_seq, capacity);
  return 0;
}

// ---- convolutions ----
int ssp_op_conv(const float* in_dev, const float* w_oihw_dev, const float* bias_dev, float* out_dev, int n, int hh, int w,
                int cin, int cout, int ksize, int in_mode, const float* in_scale_dev, const float* in_shift_dev,
                double* stats_dev, int transpose_flip, void* workspace_dev, size_t workspace_bytes, void* stream) {
  // with transpose_flip the weight tensor is [cin_conv... see header]: w is OIHW with O = (tf ? cin : cout)
  AlgoScope algo(nullptr);
  if (ksize == 1 && in_mode != 2 && g1_enabled() && g1_fits(cin, cout, (long)n * hh * w, cin, cout, 1)) {
    // pointwise layer: the grouped kernel of the heads, one problem set (conv1x1_group.hip.h); workspace = operand image
    const size_t img = g1_image_floats(cin, cout) * sizeof(float);
    if (workspace_bytes >= img) {
      hipStream_t st = (hipStream_t)stream;
      float* wpk = reinterpret_cast<float*>(workspace_dev);
      G1PackJobs G;
      G.n = 0;
      int nb = 0;
      g1_add_pack(G, nb, w_oihw_dev, wpk, transpose_flip ? cin : cout, transpose_flip ? cout : cin, transpose_flip ? 1 : 0);
      hipLaunchKernelGGL(pack_g1_kernel, dim3(nb), dim3(256), 0, st, G);
      HIPCHK(hipGetLastError());
      G1Layer y;
      y.in[0] = in_dev; y.in_cs = cin; y.in_co = 0; y.out[0] = out_dev; y.out_cs = cout; y.out_co = 0; y.wpk = wpk; y.bias = bias_dev;
      y.scale[0] = in_scale_dev; y.shift[0] = in_shift_dev; y.stats[0] = stats_dev; y.K = cin; y.N = cout;
      return launch_g1(&y, 1, 1, (long)n * hh * w, in_mode, device_cu_count(), st);
    }
  }
  const bool wino = wino_ok(ksize, cin) && in_mode != 2;
  const int nchunks = cdiv(cin, CK), ncob = cdiv(cout, NB);
  const size_t need = (size_t)ncob * nchunks * pk_taps(ksize) * CK * NB * sizeof(float);
  if (workspace_bytes < need) return fail(-4, "ssp_op_conv workspace too small (%zu < %zu)", workspace_bytes, need);
  // the bf16 path's convolutions are NHWC bf16 (ssp_op_conv_bf16): its fp32 Winograd-shaped case has no kernel
  if (bf16_path() && ksize == 3 && cin % CK == 0 && in_mode != 2)
    return fail(-3, "ssp_op_conv: conv algorithm 12 has no fp32 3x3 kernel for Cin %% 16 == 0 (use ssp_op_conv_bf16 or another algorithm)");
  hipStream_t st = (hipStream_t)stream;
  float* wpk = reinterpret_cast<float*>(workspace_dev);
  const bool w4 = wino && ksize == 3 && w4_eligible(nullptr, 1, n, hh, w, cin, cout);
  if (!transpose_flip) CHK(launch_pack(w_oihw_dev, wpk, cout, cin, ksize, 0, wino, st, w4));
  else CHK(launch_pack(w_oihw_dev, wpk, cin, cout, ksize, 1, wino, st, w4));
  ConvCall c;
  c.in = in_dev; c.in_cs = cin; c.in_co = 0; c.cin = cin; c.wpk = wpk; c.bias = bias_dev; c.out = out_dev; c.out_cs = cout;
  c.out_co = 0; c.cout = cout; c.in_scale = in_scale_dev; c.in_shift = in_shift_dev; c.stats = stats_dev; c.N = n;
  c.H = hh; c.W = w; c.ks = ksize; c.in_mode = in_mode; c.nchunks = nchunks; c.ncob = ncob; c.wino = wino;
  return launch_conv(nullptr, c, st, 0);
}

int ssp_op_conv_wgrad(const float* in_dev, const float* dout_dev, float* dw_oihw_dev, int n, int hh, int w, int cin,
                      int cout, int ksize, int in_mode, const float* in_scale_dev, const float* in_shift_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream) {
  AlgoScope algo(nullptr);
  if (ksize == 1 && in_mode == 1 && g1_enabled() && g1w_fits(cin, cout, (long)n * hh * w, cin, cout) && cdiv(cdiv(cout, 32), G1_NT) <= G1W_MAXP &&
      workspace_bytes >= (size_t)64 * G1W_SLAB * sizeof(float)) {
    // pointwise layer with 256 input channels under BatchNorm + ReLU on load: the grouped kernel of the heads
    G1WLayer y;
    y.x[0] = in_dev; y.x_cs = cin; y.x_co = 0; y.scale[0] = in_scale_dev; y.shift[0] = in_shift_dev; y.dy[0] = dout_dev;
    y.dy_cs = cout; y.dy_co = 0; y.dw = dw_oihw_dev; y.N = cout;
    return launch_g1_wgrad(&y, 1, 1, (long)n * hh * w, reinterpret_cast<float*>(workspace_dev),
                           (int)std::min<size_t>(workspace_bytes / (G1W_SLAB * sizeof(float)), 512), device_cu_count(), (hipStream_t)stream);
  }
  WgradCall c;
  c.in = in_dev; c.in_cs = cin; c.in_co = 0; c.cin = cin; c.dout = dout_dev; c.dout_cs = cout; c.dout_co = 0; c.cout = cout;
  c.in_scale = in_scale_dev; c.in_shift = in_shift_dev; c.dw = dw_oihw_dev; c.N = n; c.H = hh; c.W = w; c.ks = ksize;
  c.in_mode = in_mode;
  return launch_wgrad(nullptr, c, reinterpret_cast<float*>(workspace_dev), workspace_bytes / sizeof(float), device_cu_count(),
                      (hipStream_t)stream);
}


// ---- pair construction (row a15) ----
int ssp_op_warp_image(const float* img_dev, const float* inv_h_dev, float* out_dev, int b, int hh, int w, int nearest,
                      void* stream) {
  const long n = (long)b * hh * w;
  return launch<warp_image_kernel>(dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, img_dev, inv_h_dev, out_dev, b, hh, w,
                                   nearest ? 1 : 0);
}

int ssp_op_erode(const float* mask_dev, float* out_dev, int b, int hh, int w, int radius, void* stream) {
  if (radius < 0 || radius > 32) return fail(-1, "erosion radius out of range");
  const long n = (long)b * hh * w;
  return launch<erode_ellipse_kernel>(dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, mask_dev, out_dev, b, hh, w, radius);
}

static int warp_labels_impl(const float* labels_dev, const float* h_dev, const float* hpx_dev, float* out_dev, int b, int hh,
                            int w, hipStream_t st) {
  const long n = (long)b * hh * w;
  HIPCHK(hipMemsetAsync(out_dev, 0, n * sizeof(float), st));
  return launch<warp_labels_kernel>(dim3(cdiv(n, 256)), dim3(256), 0, st, labels_dev, h_dev, hpx_dev, out_dev, b, hh, w);
}
int ssp_op_warp_labels(const float* labels_dev, const float* h_dev, float* out_dev, int b, int hh, int w, void* stream) {
  return warp_labels_impl(labels_dev, h_dev, nullptr, out_dev, b, hh, w, (hipStream_t)stream);
}
int ssp_op_warp_labels_px(const float* labels_dev, const float* hpx_dev, float* out_dev, int b, int hh, int w, void* stream) {
  if (!hpx_dev) return fail(-1, "warp_labels_px: pixel-space homographies required");
  return warp_labels_impl(labels_dev, nullptr, hpx_dev, out_dev, b, hh, w, (hipStream_t)stream);
}

// ---- homography-adaptation export ----
static int export_cap(const ssp_export_params* p) {
  const int d = p->nms_dist + 1;
  return cdiv(p->height, d) * cdiv(p->width, d);  // kept points are pairwise more than nms_dist apart (Chebyshev)
}
static int export_cap2(const ssp_export_params* p) {
  int c = 1;
  while (c < export_cap(p)) c <<= 1;
  return c;
}
static int export_check(const ssp_export_params* p) {
  if (!p || p->n_views < 1 || p->height < 8 || p->width < 8 || p->height % 8 || p->width % 8)
    return fail(-1, "export: n_views >= 1 and height/width multiples of 8 are required");
  if (p->nms_dist < 0 || p->nms_dist > 64 || p->border_remove < 0 || p->top_k < 0)
    return fail(-1, "export: nms_dist in [0,64], border_remove >= 0, top_k >= 0 required");
  return 0;
}
struct ExportWs {
  float *heat, *agg, *pts;
  int32_t* count;
  PointsWork pw;
  size_t bytes;
};
static ExportWs export_carve(const ssp_export_params* p, void* base) {
  Carver c{reinterpret_cast<char*>(base), 0};
  const size_t hw = (size_t)p->height * p->width;
  ExportWs w;
  w.heat = c.take<float>(hw * p->n_views);
  w.agg = c.take<float>(hw);
  w.pw.state = c.take<uint8_t>(hw);
  w.pw.cand[0] = c.take<int32_t>(hw);
  w.pw.cand[1] = c.take<int32_t>(hw);
  w.pw.keys = c.take<uint64_t>(export_cap2(p));
  w.pw.counters = c.take<int32_t>(16);
  w.pts = c.take<float>((size_t)export_cap(p) * 5);
  w.count = c.take<int32_t>(16);
  w.bytes = align_up(c.off, 256);
  return w;
}

size_t ssp_export_workspace_bytes(const ssp_export_params* p) {
  if (export_check(p)) return 0;
  return export_carve(p, nullptr).bytes;
}

int ssp_export_max_points(const ssp_export_params* p) {
  if (export_check(p)) return -1;
  const int cap = export_cap(p);
  return p->top_k > 0 ? std::min(cap, p->top_k) : cap;
}

int ssp_op_homoadapt_views(const float* img_dev, const float* inv_h_dev, float* views_dev, float* masks_dev, int n, int hh,
                           int w, void* stream) {
  const long tot = (long)n * hh * w;
  return launch<homoadapt_views_kernel>(dim3(cdiv(tot, 256)), dim3(256), 0, (hipStream_t)stream, img_dev, inv_h_dev, views_dev,
                                        masks_dev, n, hh, w);
}

int ssp_op_flatten_detection(const float* semi_nchw_dev, const float* mask_dev, float* heat_dev, int n, int hc, int wc,
                             void* stream) {
  const int ncells = n * hc * wc;
  return launch<flatten_detection_kernel>(dim3(cdiv(ncells, 4)), dim3(256), 0, (hipStream_t)stream, semi_nchw_dev,
                                          (const float*)nullptr, (const float*)nullptr, mask_dev, heat_dev, ncells, hc, wc,
                                          (long)65 * hc * wc, 1L, (long)hc * wc);
}

int ssp_op_combine_heatmap(const float* heat_dev, const float* mask_dev, const float* unwarp_h_dev, float* out_dev, int n,
                           int hh, int w, void* stream) {
  return launch<combine_heatmap_kernel>(dim3(cdiv((long)hh * w, 64)), dim3(256), 0, (hipStream_t)stream, heat_dev, mask_dev,
                                        unwarp_h_dev, out_dev, n, hh, w);
}

static int heatmap_points(const float* heat, const ssp_export_params* p, const PointsWork& pw, float* pts, int32_t* count,
                          hipStream_t st) {
  const int hw = p->height * p->width;
  HIPCHK(hipMemsetAsync(pw.counters, 0, 16 * sizeof(int32_t), st));
  const int cap2 = export_cap2(p);
  hipLaunchKernelGGL(nms_init_kernel, dim3(cdiv(std::max(hw, cap2), 256)), dim3(256), 0, st, heat, p->conf_thresh, pw, hw,
                     cap2);
  if (p->nms_dist <= NMS_MAX_HALO)
    hipLaunchKernelGGL(nms_tiles_kernel, dim3(cdiv(p->width, NMS_TILE) * cdiv(p->height, NMS_TILE)), dim3(1024), 0, st,
                       heat, pw, p->height, p->width, p->nms_dist, p->border_remove, cap2, 512);
  hipLaunchKernelGGL(nms_points_kernel, dim3(1), dim3(1024), 0, st, heat, pw, p->height, p->width, p->nms_dist,
                     p->border_remove, p->top_k, p->subpixel, export_cap(p), export_cap2(p), pts, count);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_heatmap_points(const float* heat_dev, const ssp_export_params* p, void* workspace_dev, float* pts_dev,
                          int32_t* count_dev, void* stream) {
  CHK(export_check(p));
  if (!heat_dev || !workspace_dev || !pts_dev || !count_dev) return fail(-1, "heatmap_points: null pointer");
  return heatmap_points(heat_dev, p, export_carve(p, workspace_dev).pw, pts_dev, count_dev, (hipStream_t)stream);
}

int ssp_op_heatmap_nms(const float* heat_dev, const ssp_export_params* p, int n_maps, void* workspace_dev,
                       const float* labels_dev, float* nms_map_dev, float* pr_dev, void* stream) {
  CHK(export_check(p));
  if (!heat_dev || !workspace_dev || n_maps < 1) return fail(-1, "heatmap_nms: bad argument");
  hipStream_t st = (hipStream_t)stream;
  ssp_export_params q = *p;
  q.top_k = 0; q.subpixel = 0;
  const ExportWs w = export_carve(&q, workspace_dev);
  const size_t hw = (size_t)p->height * p->width;
  if (nms_map_dev) HIPCHK(hipMemsetAsync(nms_map_dev, 0, hw * n_maps * sizeof(float), st));
  for (int k = 0; k < n_maps; ++k) {
    CHK(heatmap_points(heat_dev + k * hw, &q, w.pw, w.pts, w.count, st));
    hipLaunchKernelGGL(nms_map_pr_kernel, dim3(1), dim3(256), 0, st, w.pts, w.count,
                       labels_dev ? labels_dev + k * hw : nullptr, nms_map_dev ? nms_map_dev + k * hw : nullptr,
                       pr_dev ? pr_dev + 2 * k : nullptr, p->height, p->width);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_detector_heatmap(ssp_handle* h, int slot, float* heat_dev, void* stream) {
  if (!h || !h->bound) return fail(-1, "handle not bound");
  if (slot < 0 || slot > 1 || !heat_dev) return fail(-1, "detector_heatmap: bad argument");
  Slot& S = h->slot[slot];
  if (S.N <= 0) return fail(-1, "detector_heatmap: slot %d holds no forward", slot);
  const int Hc = S.H / 8, Wc = S.W / 8, ncells = S.N * Hc * Wc;
  return launch<flatten_detection_kernel>(dim3(cdiv(ncells, 4)), dim3(256), 0, (hipStream_t)stream, S.Y[L_PB], S.bn[L_PB].scale,
                                          S.bn[L_PB].shift, (const float*)nullptr, heat_dev, ncells, Hc, Wc,
                                          (long)Hc * Wc * S.y_cs[L_PB], (long)S.y_cs[L_PB], 1L);
}

int ssp_op_soft_argmax_points(const float* heat_dev, const float* xy_dev, float* out_dev, int n, int hh, int w,
                              void* stream) {
  if (n <= 0) return 0;
  return launch<soft_argmax_points_kernel>(dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, heat_dev, xy_dev, out_dev, n, hh,
                                           w);
}

int ssp_export_points(ssp_handle* h, const ssp_export_params* p, int n_images, const float* const* views_dev,
                      const float* const* masks_dev, const float* const* unwarp_h_dev, void* const* workspace_dev,
                      float* const* heatmap_out_dev, float* const* pts_dev, int32_t* const* count_dev, void* stream) {
  if (!h || !h->bound) return fail(-1, "handle not bound");
  CHK(export_check(p));
  if (n_images < 1 || n_images > 2) return fail(-1, "export: 1 or 2 images per call");
  AlgoScope algo(h);
  if (p->n_views > h->cfg.max_batch || (size_t)p->n_views * p->height * p->width >
                                           (size_t)h->cfg.max_batch * h->cfg.height * h->cfg.width)
    return fail(-1, "export: %d views of %dx%d exceed the configured engine size", p->n_views, p->height, p->width);
  for (int k = 0; k < n_images; ++k)
    if (!views_dev[k] || !masks_dev[k] || !unwarp_h_dev[k] || !workspace_dev[k] || !pts_dev[k] || !count_dev[k])
      return fail(-1, "export: null pointer for image %d", k);
  hipStream_t st = (hipStream_t)stream;
  SlotSet SS{n_images, {&h->slot[0], n_images == 2 ? &h->slot[1] : nullptr}};
  const float* xs[2] = {views_dev[0], n_images == 2 ? views_dev[1] : nullptr};
  // BatchNorm in train mode over the views of ONE image (models/model_wrap.py:120 leaves net.eval() commented out);
  // only the detector head is evaluated -- the export discards the descriptors (export.py:296)
  CHK(run_forward(h, SS, xs, p->n_views, p->height, p->width, 1, false, st, true));
  const int Hc = p->height / 8, Wc = p->width / 8, ncells = p->n_views * Hc * Wc;
  for (int k = 0; k < n_images; ++k) {
    Slot& S = h->slot[k];
    ExportWs w = export_carve(p, workspace_dev[k]);
    float* agg = heatmap_out_dev && heatmap_out_dev[k] ? heatmap_out_dev[k] : w.agg;
    hipLaunchKernelGGL(flatten_detection_kernel, dim3(cdiv(ncells, 4)), dim3(256), 0, st, S.Y[L_PB], S.bn[L_PB].scale,
                       S.bn[L_PB].shift, masks_dev[k], w.heat, ncells, Hc, Wc, (long)Hc * Wc * S.y_cs[L_PB],
                       (long)S.y_cs[L_PB], 1L);
    hipLaunchKernelGGL(combine_heatmap_kernel, dim3(cdiv((long)p->height * p->width, 64)), dim3(256), 0, st, w.heat,
                       masks_dev[k], unwarp_h_dev[k], agg, p->n_views, p->height, p->width);
    HIPCHK(hipGetLastError());
    CHK(heatmap_points(agg, p, w.pw, pts_dev[k], count_dev[k], st));
  }
  return 0;
}

// ---- descriptor export (export.py:66-190): keypoints, sparse descriptors, two-way matching ----
struct DescribeWs {
  float* heat;  // [n][H*W]
  PointsWork pw;  // state, cand: [n][H*W]; keys: [n][cap2]; counters: [n][16] (points_work_of)
  size_t bytes;
};
static DescribeWs describe_carve(const ssp_export_params* p, int n, void* base) {
  Carver c{reinterpret_cast<char*>(base), 0};
  const size_t hw = (size_t)p->height * p->width;
  DescribeWs w;
  w.heat = c.take<float>(hw * n);
  w.pw.state = c.take<uint8_t>(hw * n);
  w.pw.cand[0] = c.take<int32_t>(hw * n);
  w.pw.cand[1] = c.take<int32_t>(hw * n);
  w.pw.keys = c.take<uint64_t>((size_t)export_cap2(p) * n);
  w.pw.counters = c.take<int32_t>((size_t)16 * n);
  w.bytes = align_up(c.off, 256);
  return w;
}

size_t ssp_describe_workspace_bytes(const ssp_export_params* p, int n) {
  if (export_check(p) || n < 1) return 0;
  return describe_carve(p, n, nullptr).bytes;
}

int ssp_describe_points(ssp_handle* h, int slot, const ssp_export_params* p, int n, void* workspace_dev, float* pts_dev,
                        int32_t* count_dev, float* desc_dev, void* stream) {
  if (!h || !h->bound) return fail(-1, "handle not bound");
  CHK(export_check(p));
  if (slot < 0 || slot > 1) return fail(-1, "describe_points: slot must be 0 or 1");
  if (!workspace_dev || !pts_dev || !count_dev || !desc_dev) return fail(-1, "describe_points: null pointer");
  Slot& S = h->slot[slot];
  if (S.N <= 0 || !S.has_desc) return fail(-1, "describe_points: slot %d holds no forward with descriptors", slot);
  if (n < 1 || n > S.N || p->height != S.H || p->width != S.W)
    return fail(-1, "describe_points: %d images of %dx%d do not match the slot's forward (%d of %dx%d)", n, p->height,
                p->width, S.N, S.H, S.W);
  hipStream_t st = (hipStream_t)stream;
  const DescribeWs w = describe_carve(p, n, workspace_dev);
  const int Hc = S.H / 8, Wc = S.W / 8, ncells = n * Hc * Wc, hw = S.H * S.W;
  const int cap = ssp_export_max_points(p), cap2 = export_cap2(p);
  HIPCHK(hipMemsetAsync(w.pw.counters, 0, (size_t)16 * n * sizeof(int32_t), st));
  hipLaunchKernelGGL(flatten_detection_kernel, dim3(cdiv(ncells, 4)), dim3(256), 0, st, S.Y[L_PB], S.bn[L_PB].scale,
                     S.bn[L_PB].shift, (const float*)nullptr, w.heat, ncells, Hc, Wc, (long)Hc * Wc * S.y_cs[L_PB],
                     (long)S.y_cs[L_PB], 1L);
  hipLaunchKernelGGL(nms_init_kernel, dim3(cdiv(std::max(hw, cap2), 256), n), dim3(256), 0, st, w.heat, p->conf_thresh, w.pw,
                     hw, cap2);
  if (p->nms_dist <= NMS_MAX_HALO)
    hipLaunchKernelGGL(nms_tiles_kernel, dim3(cdiv(p->width, NMS_TILE) * cdiv(p->height, NMS_TILE), n), dim3(1024), 0, st,
                       w.heat, w.pw, p->height, p->width, p->nms_dist, p->border_remove, cap2, 512);
  hipLaunchKernelGGL(nms_points_kernel, dim3(1, n), dim3(1024), 0, st, w.heat, w.pw, p->height, p->width, p->nms_dist,
                     p->border_remove, p->top_k, p->subpixel, cap, cap2, pts_dev, count_dev);
  hipLaunchKernelGGL(sample_desc_kernel, dim3(cdiv(cap, 4), n), dim3(256), 0, st, S.desc, (long)Hc * Wc * 256, 256L, 1L,
                     Hc, Wc, (const float*)pts_dev, 5, (const int32_t*)count_dev, cap, desc_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_sample_descriptors(const float* desc_nchw_dev, int b, int hc, int wc, const float* xy_dev,
                              const int32_t* counts_dev, int cap, float* out_dev, void* stream) {
  if (!desc_nchw_dev || !xy_dev || !counts_dev || !out_dev) return fail(-1, "sample_descriptors: null pointer");
  if (b < 1 || hc < 1 || wc < 1 || cap < 0) return fail(-1, "sample_descriptors: b, hc, wc >= 1 and cap >= 0 required");
  if (cap == 0) return 0;
  return launch<sample_desc_kernel>(dim3(cdiv(cap, 4), b), dim3(256), 0, (hipStream_t)stream, desc_nchw_dev, (long)256 * hc * wc,
                                    1L, (long)hc * wc, hc, wc, xy_dev, 2, counts_dev, cap, out_dev);
}

// best-distance keys per row and per column of a distance matrix (ssp_match_two_way: of every pair's, [n_pairs][cap] each;
// ssp_match_world: [map_cap] and [cap]); rowmin..rowmin + keys is cleared as one range
struct MatchWs {
  uint64_t *rowmin, *colmin;  // back to back
  size_t keys, bytes;
};
static MatchWs match_carve(size_t n_rows, size_t n_cols, void* base) {
  Carver c{reinterpret_cast<char*>(base), 0};
  MatchWs w;
  w.keys = n_rows + n_cols;
  w.rowmin = c.take<uint64_t>(w.keys);
  w.colmin = base ? w.rowmin + n_rows : nullptr;
  w.bytes = align_up(c.off, 256);
  return w;
}

size_t ssp_match_workspace_bytes(int cap, int n_pairs) {
  if (pairs_check("match_two_way", cap, n_pairs, 1)) return 0;
  return match_carve((size_t)n_pairs * cap, (size_t)n_pairs * cap, nullptr).bytes;
}

// cls1_dev == NULL: the plain matcher (match_dist_kernel<false>)
static int match_two_way_impl(const char* what, const float* desc1_dev, const int32_t* count1_dev, const float* desc2_dev,
                              const int32_t* count2_dev, const uint8_t* cls1_dev, const uint8_t* cls2_dev, int cap, int n_pairs,
                              int pair_stride, float nn_thresh, void* workspace_dev, float* match_dev, int32_t* n_match_dev,
                              void* stream) {
  CHK(pairs_check(what, cap, n_pairs, pair_stride));
  if (!(nn_thresh >= 0.f)) return fail(-1, "%s: nn_thresh must be non-negative", what);
  if (!desc1_dev || !count1_dev || !desc2_dev || !count2_dev || !workspace_dev || !match_dev || !n_match_dev)
    return fail(-1, "%s: null pointer", what);
  hipStream_t st = (hipStream_t)stream;
  const MatchWs w = match_carve((size_t)n_pairs * cap, (size_t)n_pairs * cap, workspace_dev);
  HIPCHK(hipMemsetAsync(w.rowmin, 0xFF, w.keys * sizeof(uint64_t), st));
  const int t = cdiv(cap, MATCH_TILE);
  if (cls1_dev != nullptr)
    hipLaunchKernelGGL(match_dist_kernel<true>, dim3(t, t, n_pairs), dim3(256), 0, st, desc1_dev, count1_dev, desc2_dev,
                       count2_dev, cap, pair_stride, w.rowmin, w.colmin, cls1_dev, cls2_dev);
  else
    hipLaunchKernelGGL(match_dist_kernel<false>, dim3(t, t, n_pairs), dim3(256), 0, st, desc1_dev, count1_dev, desc2_dev,
                       count2_dev, cap, pair_stride, w.rowmin, w.colmin, (const uint8_t*)nullptr, (const uint8_t*)nullptr);
  hipLaunchKernelGGL(match_compact_kernel, dim3(n_pairs), dim3(1024), 0, st, (const uint64_t*)w.rowmin, (const uint64_t*)w.colmin,
                     count1_dev, count2_dev, cap, pair_stride, nn_thresh, match_dev, n_match_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_match_two_way(const float* desc1_dev, const int32_t* count1_dev, const float* desc2_dev, const int32_t* count2_dev,
                      int cap, int n_pairs, int pair_stride, float nn_thresh, void* workspace_dev, float* match_dev,
                      int32_t* n_match_dev, void* stream) {
  return match_two_way_impl("match_two_way", desc1_dev, count1_dev, desc2_dev, count2_dev, nullptr, nullptr, cap, n_pairs,
                            pair_stride, nn_thresh, workspace_dev, match_dev, n_match_dev, stream);
}

int ssp_match_two_way_classes(const float* desc1_dev, const int32_t* count1_dev, const float* desc2_dev,
                              const int32_t* count2_dev, const uint8_t* cls1_dev, const uint8_t* cls2_dev, int cap, int n_pairs,
                              int pair_stride, float nn_thresh, void* workspace_dev, float* match_dev, int32_t* n_match_dev,
                              void* stream) {
  if (!cls1_dev || !cls2_dev) return fail(-1, "match_two_way_classes: null class pointer");
  return match_two_way_impl("match_two_way_classes", desc1_dev, count1_dev, desc2_dev, count2_dev, cls1_dev, cls2_dev, cap,
                            n_pairs, pair_stride, nn_thresh, workspace_dev, match_dev, n_match_dev, stream);
}

// ---- semantic keypoints: classes at points, class filter ----
int ssp_op_point_classes(const float* sout_nhwc_dev, int cs, int b, int hh, int w, int n_classes, const float* pts_dev,
                         int pts_stride, const int32_t* count_dev, int cap, uint8_t* cls_dev, void* stream) {
  if (!sout_nhwc_dev || !pts_dev || !count_dev || !cls_dev) return fail(-1, "point_classes: null pointer");
  if (b < 1 || b > 65535 || hh < 8 || w < 8 || hh % 8 || w % 8)
    return fail(-1, "point_classes: 1 <= b <= 65535 and H, W multiples of 8 required (got %d of %dx%d)", b, hh, w);
  if (n_classes < 1 || n_classes > SSP_CLASS_NONE || cs < n_classes)
    return fail(-1, "point_classes: 1 <= n_classes <= %d and channel stride >= n_classes required (got %d, stride %d)",
                SSP_CLASS_NONE, n_classes, cs);
  if (cap < 1 || cap > (1 << 24) || pts_stride < 2)
    return fail(-1, "point_classes: 1 <= cap <= 2^24 rows of at least 2 floats required (cap %d, stride %d)", cap, pts_stride);
  if ((size_t)b * (hh / 8) * (w / 8) * cs > ((size_t)1 << 40)) return fail(-1, "point_classes: shape too large");
  return launch<point_class_kernel>(dim3(cdiv(cap, 4), b), dim3(256), 0, (hipStream_t)stream, sout_nhwc_dev, pts_dev, count_dev,
                                    cls_dev, hh / 8, w / 8, n_classes, cs, cap, pts_stride);
}

int ssp_point_classes(ssp_handle* h, int slot, int n, const float* pts_dev, int pts_stride, const int32_t* count_dev, int cap,
                      uint8_t* cls_dev, void* stream) {
  if (!h || !h->bound) return fail(-1, "handle not bound");
  if (h->nheads != 3) return fail(-1, "point_classes: the model has no segmentation head");
  if (slot < 0 || slot > 1) return fail(-1, "point_classes: slot must be 0 or 1");
  Slot& S = h->slot[slot];
  if (S.N <= 0 || !S.has_desc) return fail(-1, "point_classes: slot %d holds no forward with segmentation logits", slot);
  if (n < 1 || n > S.N) return fail(-1, "point_classes: %d images asked of a forward over %d", n, S.N);
  return ssp_op_point_classes(S.Y[L_SOUT], h->sout_cs, n, S.H, S.W, h->cfg.n_classes, pts_dev, pts_stride, count_dev, cap,
                              cls_dev, stream);
}

static int filter_check(int n, int cap) {
  if (n < 1 || n > 65535 || cap < 1 || cap > (1 << 24))
    return fail(-1, "filter_points: 1 <= n <= 65535 images of 1 <= cap <= 2^24 rows required (got %d of %d)", n, cap);
  return 0;
}

size_t ssp_filter_workspace_bytes(int n, int cap) {
  if (filter_check(n, cap)) return 0;
  return align_up((size_t)n * cdiv(cap, TRACK_BLOCK) * sizeof(int32_t), 256);
}

int ssp_op_filter_points(const float* pts_dev, const int32_t* count_dev, const float* desc_dev, const uint8_t* cls_dev,
                         const uint32_t keep_mask[8], int n, int cap, float* pts_out_dev, int32_t* count_out_dev,
                         float* desc_out_dev, uint8_t* cls_out_dev, void* workspace_dev, void* stream) {
  CHK(filter_check(n, cap));
  if (!pts_dev || !count_dev || !desc_dev || !cls_dev || !keep_mask || !pts_out_dev || !count_out_dev || !desc_out_dev ||
      !cls_out_dev || !workspace_dev)
    return fail(-1, "filter_points: null pointer");
  if (pts_dev == pts_out_dev || count_dev == count_out_dev || desc_dev == desc_out_dev || cls_dev == cls_out_dev)
    return fail(-1, "filter_points: the point set is not filtered in place (pass a second set of arrays)");
  if ((reinterpret_cast<size_t>(desc_dev) | reinterpret_cast<size_t>(desc_out_dev)) & 15)
    return fail(-1, "filter_points: the descriptor arrays must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ClassMask m;
  for (int k = 0; k < 8; ++k) m.w[k] = keep_mask[k];
  int32_t* block_sums = reinterpret_cast<int32_t*>(workspace_dev);
  const dim3 grid(cdiv(cap, TRACK_BLOCK), n);
  HIPCHK(hipMemsetAsync(cls_out_dev, POINT_CLASS_NONE, (size_t)n * cap, st));
  hipLaunchKernelGGL(filter_count_kernel, grid, dim3(TRACK_BLOCK), 0, st, count_dev, cls_dev, m, cap, block_sums);
  hipLaunchKernelGGL(filter_scatter_kernel, grid, dim3(TRACK_BLOCK), 0, st, pts_dev, count_dev, desc_dev, cls_dev, m, cap,
                     (const int32_t*)block_sums, pts_out_dev, count_out_dev, desc_out_dev, cls_out_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- point tracks over a frame sequence (PointTracker.update / get_tracks) ----
struct TrackWs {
  int32_t* ids_tmp;       // [row_cap][L]
  double* score_tmp;      // [row_cap]
  int32_t* row_of_point;  // [point_cap]
  int32_t* matched;       // [point_cap]
  int32_t* block_sums;    // [cdiv(row_cap, TRACK_BLOCK) + cdiv(point_cap, TRACK_BLOCK)]
  size_t bytes;
};
static TrackWs track_carve(int L, int point_cap, int row_cap, void* base) {
  Carver c{reinterpret_cast<char*>(base), 0};
  TrackWs w;
  w.ids_tmp = c.take<int32_t>((size_t)row_cap * L);
  w.score_tmp = c.take<double>((size_t)row_cap);
  w.row_of_point = c.take<int32_t>((size_t)point_cap);
  w.matched = c.take<int32_t>((size_t)point_cap);
  w.block_sums = c.take<int32_t>((size_t)cdiv(row_cap, TRACK_BLOCK) + cdiv(point_cap, TRACK_BLOCK));
  w.bytes = align_up(c.off, 256);
  return w;
}

static int track_check(const char* what, int L, int point_cap, int row_cap) {
  if (L < 2 || L > SSP_TRACK_MAX_LENGTH)
    return fail(-1, "%s: 2 <= max_length <= %d required (got %d)", what, SSP_TRACK_MAX_LENGTH, L);
  if (point_cap < 1 || point_cap > SSP_MATCH_MAX_POINTS)
    return fail(-1, "%s: 1 <= point_cap <= %d points per frame required (got %d)", what, SSP_MATCH_MAX_POINTS, point_cap);
  if (row_cap < 1 || row_cap > ROW_CAP_MAX)
    return fail(-1, "%s: 1 <= row_cap <= %d rows required (got %d)", what, ROW_CAP_MAX, row_cap);
  return 0;
}

size_t ssp_track_workspace_bytes(int max_length, int point_cap, int row_cap) {
  if (track_check("track_workspace_bytes", max_length, point_cap, row_cap)) return 0;
  return track_carve(max_length, point_cap, row_cap, nullptr).bytes;
}

int ssp_op_track_update(const int32_t* ids_in_dev, const int32_t* tid_in_dev, const double* score_in_dev,
                        const int32_t* state_in_dev, const float* match_dev, const double* match_score64_dev,
                        const int32_t* n_match_dev, const int32_t* n_points_dev, int max_length, int point_cap, int row_cap,
                        void* workspace_dev, int32_t* ids_out_dev, int32_t* tid_out_dev, double* score_out_dev,
                        int32_t* state_out_dev, void* stream) {
  CHK(track_check("track_update", max_length, point_cap, row_cap));
  if (row_cap < max_length * point_cap)
    return fail(-1, "track_update: row_cap %d is below max_length * point_cap = %d (every point of the retained frames may own a row)",
                row_cap, max_length * point_cap);
  if (!ids_in_dev || !tid_in_dev || !score_in_dev || !state_in_dev || !match_dev || !n_match_dev || !n_points_dev ||
      !workspace_dev || !ids_out_dev || !tid_out_dev || !score_out_dev || !state_out_dev)
    return fail(-1, "track_update: null pointer");
  if (ids_in_dev == ids_out_dev || tid_in_dev == tid_out_dev || score_in_dev == score_out_dev || state_in_dev == state_out_dev)
    return fail(-1, "track_update: the table is not updated in place (pass a second set of arrays)");
  hipStream_t st = (hipStream_t)stream;
  const int L = max_length;
  const TrackWs w = track_carve(L, point_cap, row_cap, workspace_dev);
  const int nb_old = cdiv(row_cap, TRACK_BLOCK), nb = nb_old + cdiv(point_cap, TRACK_BLOCK);
  HIPCHK(hipMemsetAsync(w.row_of_point, 0xFF, (size_t)point_cap * sizeof(int32_t), st));
  HIPCHK(hipMemsetAsync(w.matched, 0, (size_t)point_cap * sizeof(int32_t), st));
  hipLaunchKernelGGL(track_shift_kernel, dim3(cdiv(row_cap, 256)), dim3(256), 0, st, ids_in_dev, score_in_dev, state_in_dev, L,
                     point_cap, row_cap, w.ids_tmp, w.score_tmp, w.row_of_point);
  hipLaunchKernelGGL(track_match_kernel, dim3(cdiv(point_cap, 256)), dim3(256), 0, st, match_dev, match_score64_dev, n_match_dev,
                     n_points_dev, state_in_dev, L, point_cap, row_cap, (const int32_t*)w.row_of_point, w.ids_tmp, w.score_tmp,
                     w.matched);
  hipLaunchKernelGGL(track_count_kernel, dim3(nb), dim3(TRACK_BLOCK), 0, st, (const int32_t*)w.ids_tmp, (const int32_t*)w.matched,
                     state_in_dev, n_points_dev, L, point_cap, row_cap, nb_old, w.block_sums);
  hipLaunchKernelGGL(track_scatter_kernel, dim3(nb), dim3(TRACK_BLOCK), 0, st, (const int32_t*)w.ids_tmp,
                     (const double*)w.score_tmp, tid_in_dev, (const int32_t*)w.matched, state_in_dev, n_points_dev,
                     (const int32_t*)w.block_sums, L, point_cap, row_cap, nb_old, ids_out_dev, tid_out_dev, score_out_dev,
                     state_out_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_track_select(const int32_t* ids_dev, const int32_t* tid_dev, const double* score_dev, const int32_t* state_dev,
                        int max_length, int row_cap, int min_length, void* workspace_dev, double* tracks_dev,
                        int32_t* n_tracks_dev, void* stream) {
  CHK(track_check("track_select", max_length, 1, row_cap));
  if (min_length < 0) return fail(-1, "track_select: min_length >= 0 required (0 = every row; got %d)", min_length);
  if (!ids_dev || !tid_dev || !score_dev || !state_dev || !workspace_dev || !tracks_dev || !n_tracks_dev)
    return fail(-1, "track_select: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const TrackWs w = track_carve(max_length, 1, row_cap, workspace_dev);
  const int nb = cdiv(row_cap, TRACK_BLOCK);
  hipLaunchKernelGGL(track_select_count_kernel, dim3(nb), dim3(TRACK_BLOCK), 0, st, ids_dev, state_dev, max_length, row_cap,
                     min_length, w.block_sums);
  hipLaunchKernelGGL(track_select_scatter_kernel, dim3(nb), dim3(TRACK_BLOCK), 0, st, ids_dev, tid_dev, score_dev, state_dev,
                     (const int32_t*)w.block_sums, max_length, row_cap, min_length, tracks_dev, n_tracks_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_track_points(const double* tracks_dev, const int32_t* n_tracks_dev, const double* pts_dev, const int32_t* state_dev,
                        int max_length, int point_cap, int track_cap, int first_slot, double* xy_dev, void* stream) {
  CHK(track_check("track_points", max_length, point_cap, track_cap));
  if (first_slot < 0 || first_slot >= max_length)
    return fail(-1, "track_points: 0 <= first_slot < max_length required (got %d)", first_slot);
  if (!tracks_dev || !n_tracks_dev || !pts_dev || !state_dev || !xy_dev) return fail(-1, "track_points: null pointer");
  return launch<track_points_kernel>(dim3(cdiv((long)track_cap * max_length, 256)), dim3(256), 0, (hipStream_t)stream, tracks_dev,
                                     n_tracks_dev, pts_dev, state_dev, max_length, point_cap, track_cap, first_slot, xy_dev);
}

// ---- evaluation of descriptor exports (evaluation.py:86-500): repeatability, RANSAC homography, AP ----
#define EVAL_KEEP_MAX 2048
#define EVAL_LDS_MAX (120 * 1024)

int ssp_eval_repeatability(const double* pts1_dev, const int32_t* n1_dev, const double* pts2_dev, const int32_t* n2_dev,
                           int cap, int n_pairs, int pair_stride, const double* hom_dev, const double* hom_inv_dev,
                           int height, int width, int keep_k, double dist_thresh, double* out_dev, void* stream) {
  CHK(pairs_check("eval_repeatability", cap, n_pairs, pair_stride));
  if (!pts1_dev || !n1_dev || !pts2_dev || !n2_dev || !hom_dev || !hom_inv_dev || !out_dev)
    return fail(-1, "eval_repeatability: null pointer");
  if (height < 1 || width < 1 || keep_k < 1 || keep_k > EVAL_KEEP_MAX || !(dist_thresh >= 0.0))
    return fail(-1, "eval_repeatability: height, width >= 1, 1 <= keep_k <= %d and dist_thresh >= 0 required",
                EVAL_KEEP_MAX);
  const int kk = std::min(keep_k, cap);
  const size_t lds = (size_t)((cap + 1) & ~1) * sizeof(double) + (size_t)2 * kk * 2 * sizeof(double);
  return launch_lds<eval_repeat_kernel>(EVAL_LDS_MAX, dim3(n_pairs), dim3(EVAL_THREADS), lds, (hipStream_t)stream, pts1_dev, n1_dev,
                                        pts2_dev, n2_dev, cap, pair_stride, hom_dev, hom_inv_dev, height, width, kk, dist_thresh, out_dev);
}

size_t ssp_eval_ransac_workspace_bytes(int cap, int n_pairs) {
  if (pairs_check("eval_ransac", cap, n_pairs, 1)) return 0;
  return align_up((size_t)n_pairs * cap * 4 * sizeof(double), 256);
}

int ssp_eval_ransac(const double* pts1_dev, const double* pts2_dev, int cap, int n_pairs, int pair_stride,
                    const float* match_dev, const int32_t* n_match_dev, const uint64_t* seeds_dev, void* workspace_dev,
                    double* h_dev, uint8_t* mask_dev, int32_t* n_inlier_dev, int32_t* status_dev, double* ap_dev,
                    void* stream) {
  CHK(pairs_check("eval_ransac", cap, n_pairs, pair_stride));
  if (!pts1_dev || !pts2_dev || !match_dev || !n_match_dev || !seeds_dev || !workspace_dev || !h_dev || !mask_dev ||
      !n_inlier_dev || !status_dev)
    return fail(-1, "eval_ransac: null pointer");
  hipStream_t st = (hipStream_t)stream;
  double4* xy = reinterpret_cast<double4*>(workspace_dev);
  const size_t small = (size_t)cap * (sizeof(float) + 1);
  const bool use_lds = (size_t)cap * sizeof(double4) + small <= EVAL_LDS_MAX;
  hipLaunchKernelGGL(eval_gather_kernel, dim3(cdiv(cap, 256), n_pairs), dim3(256), 0, st, pts1_dev, pts2_dev, cap, pair_stride,
                     match_dev, n_match_dev, xy);
  return launch_lds<eval_ransac_kernel>(EVAL_LDS_MAX, dim3(n_pairs), dim3(EVAL_THREADS), use_lds ? (size_t)cap * sizeof(double4) + small : small,
                                        st, (const double4*)xy, match_dev, n_match_dev, cap, seeds_dev, (int)use_lds, h_dev, mask_dev,
                                        n_inlier_dev, status_dev, ap_dev);
}

// ---- epipolar check of matches: fundamental-matrix RANSAC over several workgroups per pair ----
// groups = 0: the measured choice (PERF_LOG.md, "Epipolar check").  One pair is fastest with 32 workgroups (120.7 / 208.5 us at
// 500 / 1200 matches against 121.3 / 210.4 with 16 and 121.5 / 213.6 with 8); 16 pairs are fastest with 16 (124.0 / 213.7 us against
// 194.6 / 365.2 with 32: 512 workgroups of more than 256 registers per lane run in two rounds on 256 CUs).  So 32 while
// 32 x n_pairs workgroups fit the CUs at one each, else 16.  The result does not depend on the choice.
#define EPI_GROUPS_FEW_PAIRS 32
#define EPI_GROUPS_MANY_PAIRS 16
#define EPI_CU_COUNT 256
#define EPI_LDS_MAX ((size_t)SSP_MATCH_MAX_POINTS * (sizeof(double4) + 1))
static int epi_check(const char* what, int cap, int n_pairs, int pair_stride, int pt_stride) {
  if (cap < 1 || cap > SSP_MATCH_MAX_POINTS || n_pairs < 1 || n_pairs > 65535 || pair_stride < 1 || pt_stride < 2)
    return fail(-1, "%s: 1 <= cap <= %d, 1 <= n_pairs <= 65535, pair_stride >= 1, pt_stride >= 2 required (cap %d, n_pairs %d)",
                what, SSP_MATCH_MAX_POINTS, cap, n_pairs);
  return 0;
}

size_t ssp_epi_ransac_workspace_bytes(int cap, int n_pairs) {
  if (epi_check("epi_ransac", cap, n_pairs, 1, 2)) return 0;
  return align_up((size_t)n_pairs * EPI_MAX_GROUPS * sizeof(uint64_t), 256);
}

int ssp_epi_ransac(const double* pts1_dev, const double* pts2_dev, int pt_stride, int cap, int n_pairs, int pair_stride,
                   const float* match_dev, const int32_t* n_match_dev, const uint64_t* seeds_dev, double thresh, int groups,
                   void* workspace_dev, double* f_dev, uint8_t* mask_dev, int32_t* n_inlier_dev, int32_t* status_dev,
                   int32_t* winner_dev, double* err_dev, void* stream) {
  CHK(epi_check("epi_ransac", cap, n_pairs, pair_stride, pt_stride));
  if (!pts1_dev || !pts2_dev || !match_dev || !n_match_dev || !seeds_dev || !workspace_dev || !f_dev || !mask_dev ||
      !n_inlier_dev || !status_dev)
    return fail(-1, "epi_ransac: null pointer");
  CHK(finite_nonneg_check("epi_ransac", "thresh", thresh));
  if (groups < 0 || groups > EPI_MAX_GROUPS)
    return fail(-1, "epi_ransac: 0 (the library's choice) <= groups <= %d required (got %d)", EPI_MAX_GROUPS, groups);
  if (groups == 0) groups = n_pairs * EPI_GROUPS_FEW_PAIRS <= EPI_CU_COUNT ? EPI_GROUPS_FEW_PAIRS : EPI_GROUPS_MANY_PAIRS;
  hipStream_t st = (hipStream_t)stream;
  uint64_t* keys = reinterpret_cast<uint64_t*>(workspace_dev);
  CHK(launch_lds<epi_hypotheses_kernel>(EPI_LDS_MAX, dim3(groups, n_pairs), dim3(EPI_THREADS), (size_t)cap * sizeof(double4), st, pts1_dev,
                                        pts2_dev, pt_stride, cap, pair_stride, match_dev, n_match_dev, seeds_dev, thresh, keys));
  return launch_lds<epi_finish_kernel>(EPI_LDS_MAX, dim3(n_pairs), dim3(EPI_THREADS), (size_t)cap * (sizeof(double4) + 1), st, pts1_dev,
                                       pts2_dev, pt_stride, cap, pair_stride, match_dev, n_match_dev, seeds_dev, thresh, groups,
                                       (const uint64_t*)keys, f_dev, mask_dev, n_inlier_dev, status_dev, winner_dev, err_dev);
}

int ssp_op_filter_matches(const float* match_dev, const int32_t* n_match_dev, const uint8_t* mask_dev, const int32_t* status_dev,
                          const int32_t* n_inlier_dev, int min_inliers, int cap, int n_pairs, float* match_out_dev,
                          int32_t* n_match_out_dev, void* stream) {
  if (cap < 1 || cap > SSP_MATCH_MAX_POINTS || n_pairs < 1)
    return fail(-1, "filter_matches: 1 <= cap <= %d and n_pairs >= 1 required (cap %d)", SSP_MATCH_MAX_POINTS, cap);
  if (!match_dev || !n_match_dev || !mask_dev || !status_dev || !n_inlier_dev || !match_out_dev || !n_match_out_dev)
    return fail(-1, "filter_matches: null pointer");
  if (match_dev == match_out_dev || n_match_dev == n_match_out_dev)
    return fail(-1, "filter_matches: the matches are not filtered in place (pass a second set of arrays)");
  return launch<match_filter_kernel>(dim3(n_pairs), dim3(TRACK_BLOCK), 0, (hipStream_t)stream, match_dev, n_match_dev, mask_dev,
                                     status_dev, n_inlier_dev, min_inliers, cap, match_out_dev, n_match_out_dev);
}

// ---- two-view pose: essential matrix, cheirality, scale chain and trajectory ----
static_assert(POSE_ROW_WORDS == SSP_POSE_ROW_WORDS && POSE_STATE_WORDS == SSP_POSE_STATE_WORDS,
              "include/ssp_hip.h and pose_kernels.hip.h disagree");
int ssp_pose_from_fundamental(const double* f_dev, const uint8_t* mask_dev, const int32_t* n_inlier_dev, const int32_t* status_in_dev,
                              const double* pts1_dev, const double* pts2_dev, int pt_stride, int cap, int n_pairs, int pair_stride,
                              const float* match_dev, const int32_t* n_match_dev, const double* intr_dev, int n_intr, double* r_dev,
                              double* t_dev, double* e_dev, int32_t* cand_dev, int32_t* counts_dev, int32_t* n_front_dev,
                              int32_t* status_dev, uint8_t* front_dev, double* depth_dev, double* x_dev, void* stream) {
  CHK(epi_check("pose_from_fundamental", cap, n_pairs, pair_stride, pt_stride));
  if (!f_dev || !mask_dev || !n_inlier_dev || !status_in_dev || !pts1_dev || !pts2_dev || !match_dev || !n_match_dev || !intr_dev ||
      !r_dev || !t_dev || !e_dev || !cand_dev || !counts_dev || !n_front_dev || !status_dev || !front_dev || !depth_dev || !x_dev)
    return fail(-1, "pose_from_fundamental: null pointer");
  CHK(intr_check("pose_from_fundamental", n_intr, n_pairs, "n_pairs", "pairs"));
  return launch<pose_kernel>(dim3(n_pairs), dim3(POSE_THREADS), 0, (hipStream_t)stream, f_dev, mask_dev, n_inlier_dev,
                             status_in_dev, pts1_dev, pts2_dev, pt_stride, cap, pair_stride, match_dev, n_match_dev, intr_dev,
                             n_intr, r_dev, t_dev, e_dev, cand_dev, counts_dev, n_front_dev, status_dev, front_dev, depth_dev,
                             x_dev);
}

int ssp_pose_chain(const uint8_t* front_prev_dev, const double* depth_prev_dev, const int32_t* status_prev_dev,
                   const float* match_prev_dev, const int32_t* n_match_prev_dev, int cap_prev, const uint8_t* front_dev,
                   const double* depth_dev, const int32_t* status_dev, const double* r_dev, const double* t_dev,
                   const float* match_dev, const int32_t* n_match_dev, int cap, int n_seq, double* state_dev, double* table_dev,
                   int capacity, void* stream) {
  if (cap < 1 || cap > SSP_MATCH_MAX_POINTS) return fail(-1, "pose_chain: 1 <= cap <= %d required (got %d)", SSP_MATCH_MAX_POINTS, cap);
  CHK(seq_check("pose_chain", n_seq, capacity));
  if (!front_dev || !depth_dev || !status_dev || !r_dev || !t_dev || !match_dev || !n_match_dev || !state_dev ||
      (capacity > 0 && !table_dev))
    return fail(-1, "pose_chain: null pointer");
  const bool have_prev = front_prev_dev != nullptr;
  if (have_prev && (!depth_prev_dev || !status_prev_dev || !match_prev_dev || !n_match_prev_dev))
    return fail(-1, "pose_chain: the previous pair is given whole or not at all");
  if (have_prev && (cap_prev < 1 || cap_prev > SSP_MATCH_MAX_POINTS))
    return fail(-1, "pose_chain: 1 <= cap_prev <= %d required (got %d)", SSP_MATCH_MAX_POINTS, cap_prev);
  if (!have_prev) cap_prev = 1;
  const size_t lds = (size_t)(cap_prev > cap ? cap_prev : cap) * (sizeof(double) + sizeof(int));   // <= 48 KB
  return launch<pose_chain_kernel>(dim3(n_seq), dim3(POSE_THREADS), lds, (hipStream_t)stream, front_prev_dev, depth_prev_dev,
                                   status_prev_dev, match_prev_dev, n_match_prev_dev, cap_prev, front_dev, depth_dev, status_dev,
                                   r_dev, t_dev, match_dev, n_match_dev, cap, state_dev, table_dev, capacity);
}

// ---- homography pose and model selection ----
int ssp_pose_from_homography(const double* h_dev, const uint8_t* mask_dev, const int32_t* n_inlier_dev, const int32_t* status_in_dev,
                             const double* pts1_dev, const double* pts2_dev, int pt_stride, int cap, int n_pairs, int pair_stride,
                             const float* match_dev, const int32_t* n_match_dev, const double* intr_dev, int n_intr,
                             const double* prior_dev, const int32_t* use_h_dev, double rotation_eps, double normal_margin, double* r_dev,
                             double* t_dev, int32_t* cand_dev, int32_t* counts_dev, int32_t* n_front_dev, int32_t* status_dev,
                             uint8_t* front_dev, double* depth_dev, double* x_dev, int32_t* model_dev, double* normal_dev,
                             double* normals2_dev, void* stream) {
  CHK(epi_check("pose_from_homography", cap, n_pairs, pair_stride, pt_stride));
  if (!h_dev || !mask_dev || !n_inlier_dev || !status_in_dev || !pts1_dev || !pts2_dev || !match_dev || !n_match_dev || !intr_dev ||
      !r_dev || !t_dev || !cand_dev || !counts_dev || !n_front_dev || !status_dev || !front_dev || !depth_dev || !x_dev || !model_dev ||
      !normal_dev || !normals2_dev)
    return fail(-1, "pose_from_homography: null pointer");
  CHK(intr_check("pose_from_homography", n_intr, n_pairs, "n_pairs", "pairs"));
  CHK(finite_nonneg_check("pose_from_homography", "rotation_eps", rotation_eps));
  CHK(finite_nonneg_check("pose_from_homography", "normal_margin", normal_margin));
  if (prior_dev == normals2_dev) return fail(-1, "pose_from_homography: the priors are not updated in place (pass a second array)");
  return launch<pose_h_kernel>(dim3(n_pairs), dim3(POSE_THREADS), 0, (hipStream_t)stream, h_dev, mask_dev, n_inlier_dev,
                               status_in_dev, pts1_dev, pts2_dev, pt_stride, cap, pair_stride, match_dev, n_match_dev, intr_dev,
                               n_intr, prior_dev, use_h_dev, rotation_eps, normal_margin, r_dev, t_dev, cand_dev, counts_dev,
                               n_front_dev, status_dev, front_dev, depth_dev, x_dev, model_dev, normal_dev, normals2_dev);
}

int ssp_model_select(const double* f_dev, const uint8_t* f_mask_dev, const int32_t* f_n_inlier_dev, const int32_t* f_status_dev,
                     const double* h_dev, const uint8_t* h_mask_dev, const int32_t* h_n_inlier_dev, const int32_t* h_status_dev,
                     const double* pts1_dev, const double* pts2_dev, int pt_stride, int cap, int n_pairs, int pair_stride,
                     const float* match_dev, const int32_t* n_match_dev, double model_ratio, double* scores_dev, int32_t* use_h_dev,
                     uint8_t* mask_dev, int32_t* n_inlier_dev, int32_t* status_dev, void* stream) {
  CHK(epi_check("model_select", cap, n_pairs, pair_stride, pt_stride));
  if (!f_dev || !f_mask_dev || !f_n_inlier_dev || !f_status_dev || !h_dev || !h_mask_dev || !h_n_inlier_dev || !h_status_dev ||
      !pts1_dev || !pts2_dev || !match_dev || !n_match_dev || !scores_dev || !use_h_dev || !mask_dev || !n_inlier_dev || !status_dev)
    return fail(-1, "model_select: null pointer");
  if (!(model_ratio >= 0.0) || !(model_ratio <= 1.0)) return fail(-1, "model_select: 0 <= model_ratio <= 1 required");
  if (mask_dev == f_mask_dev || mask_dev == h_mask_dev)
    return fail(-1, "model_select: the selected mask is a copy (pass an array of its own)");
  return launch<model_select_kernel>(dim3(n_pairs), dim3(POSE_THREADS), 0, (hipStream_t)stream, f_dev, f_mask_dev, f_n_inlier_dev,
                                     f_status_dev, h_dev, h_mask_dev, h_n_inlier_dev, h_status_dev, pts1_dev, pts2_dev, pt_stride,
                                     cap, pair_stride, match_dev, n_match_dev, model_ratio, scores_dev, use_h_dev, mask_dev,
                                     n_inlier_dev, status_dev);
}

// ---- landmarks from tracks: cameras of the retained frames, N-view triangulation, the accepted rows ----
static_assert(LM_CAM_WORDS == SSP_CAM_WORDS && LM_WORDS == SSP_LANDMARK_WORDS, "include/ssp_hip.h and landmark_kernels.hip.h disagree");
size_t ssp_landmark_workspace_bytes(int max_length, int row_cap) {
  if (track_check("landmark_workspace_bytes", max_length, 1, row_cap)) return 0;
  return align_up((size_t)cdiv(row_cap, TRACK_BLOCK) * sizeof(int32_t), 256);
}

int ssp_map_window(const double* state_dev, const double* table_dev, int capacity, const double* intr_dev, int n_intr, int max_length,
                   int n_frames, double* cams_dev, void* stream) {
  CHK(track_check("map_window", max_length, 1, 1));
  if (capacity < 0) return fail(-1, "map_window: capacity >= 0 required (got %d)", capacity);
  CHK(intr_check("map_window", n_intr, max_length, "max_length", "retained frames"));
  if (!state_dev || (capacity > 0 && !table_dev) || !intr_dev || !cams_dev) return fail(-1, "map_window: null pointer");
  return launch<map_window_kernel>(dim3(1), dim3(64), 0, (hipStream_t)stream, state_dev, table_dev, capacity, intr_dev, n_intr,
                                   max_length, n_frames, cams_dev);
}

int ssp_op_triangulate_tracks(const int32_t* ids_dev, const int32_t* state_dev, const double* pts_dev, int first_slot,
                              const double* cams_dev, int max_length, int point_cap, int row_cap, int min_views,
                              double cos_min_parallax, double max_reproj, double* x_dev, int32_t* n_views_dev, double* rms_dev,
                              double* cos_parallax_dev, int32_t* status_dev, void* stream) {
  CHK(track_check("triangulate_tracks", max_length, point_cap, row_cap));
  if (first_slot < 0 || first_slot >= max_length)
    return fail(-1, "triangulate_tracks: 0 <= first_slot < max_length required (got %d)", first_slot);
  if (min_views < 2) return fail(-1, "triangulate_tracks: min_views >= 2 required (got %d)", min_views);
  if (!(cos_min_parallax >= -1.0 && cos_min_parallax <= 1.0) || !(max_reproj >= 0.0))
    return fail(-1, "triangulate_tracks: -1 <= cos_min_parallax <= 1 and max_reproj >= 0 required");
  if (!ids_dev || !state_dev || !pts_dev || !cams_dev || !x_dev || !n_views_dev || !rms_dev || !cos_parallax_dev || !status_dev)
    return fail(-1, "triangulate_tracks: null pointer");
  return launch_lds<triangulate_tracks_kernel>(lm_lds_bytes(SSP_TRACK_MAX_LENGTH), dim3(cdiv(row_cap, LM_THREADS)), dim3(LM_THREADS),
                                               lm_lds_bytes(max_length), (hipStream_t)stream, ids_dev, state_dev, pts_dev, first_slot, cams_dev,
                                               max_length, point_cap, row_cap, min_views, cos_min_parallax, max_reproj, x_dev, n_views_dev,
                                               rms_dev, cos_parallax_dev, status_dev);
}

int ssp_op_landmarks_select(const int32_t* ids_dev, const int32_t* tid_dev, const int32_t* state_dev, const int32_t* status_dev,
                            const double* x_dev, const int32_t* n_views_dev, const double* rms_dev, const double* cos_parallax_dev,
                            int max_length, int point_cap, int row_cap, void* workspace_dev, double* landmarks_dev,
                            int32_t* n_landmarks_dev, void* stream) {
  CHK(track_check("landmarks_select", max_length, point_cap, row_cap));
  if (!ids_dev || !tid_dev || !state_dev || !status_dev || !x_dev || !n_views_dev || !rms_dev || !cos_parallax_dev || !workspace_dev ||
      !landmarks_dev || !n_landmarks_dev)
    return fail(-1, "landmarks_select: null pointer");
  hipStream_t st = (hipStream_t)stream;
  int32_t* block_sums = reinterpret_cast<int32_t*>(workspace_dev);
  const int nb = cdiv(row_cap, TRACK_BLOCK);
  hipLaunchKernelGGL(landmark_count_kernel, dim3(nb), dim3(TRACK_BLOCK), 0, st, state_dev, status_dev, row_cap, block_sums);
  hipLaunchKernelGGL(landmark_scatter_kernel, dim3(nb), dim3(TRACK_BLOCK), 0, st, ids_dev, tid_dev, state_dev, status_dev, x_dev,
                     n_views_dev, rms_dev, cos_parallax_dev, (const int32_t*)block_sums, max_length, point_cap, row_cap, landmarks_dev,
                     n_landmarks_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- absolute pose from landmarks: the join, the P3P RANSAC over several workgroups per problem, the repair ----
// groups = 0: the measured choice (PERF_LOG.md, "Absolute pose"): 2 workgroups per problem, one hypothesis per lane.  One problem of 500 /
// 1131 rows takes 215.1 / 364.1 us with 2 against 352.8 / 641.4 with 1 (two hypotheses per lane, one after the other), 217.2 / 367.4 with
// 8, 218.0 / 368.1 with 16 and 219.5 / 370.5 with 32 (more workgroups, each with idle wavefronts); 16 problems 219.2 / 371.0 us with 2
// against 274.9 / 472.1 with 32.  The result does not depend on the choice.
#define PNP_GROUPS_DEFAULT 2
static_assert(PNP_CORR_WORDS == SSP_CORR_WORDS && PNP_FLAG_ABSOLUTE == SSP_POSE_FLAG_ABSOLUTE && PNP_MAX_CAP == SSP_MATCH_MAX_POINTS,
              "include/ssp_hip.h and pnp_kernels.hip.h disagree");
size_t ssp_pnp_workspace_bytes(int n_problems) {
  if (n_problems < 1 || n_problems > 65535) {
    fail(-1, "pnp_workspace_bytes: 1 <= n_problems <= 65535 required (got %d)", n_problems);
    return 0;
  }
  return align_up((size_t)n_problems * PNP_MAX_GROUPS * sizeof(uint64_t), 256);
}

int ssp_op_landmark_matches(const double* landmarks_dev, const int32_t* n_landmarks_dev, int row_cap, const float* match_dev,
                            const int32_t* n_match_dev, int cap, const double* pts_new_dev, int pt_stride, int point_cap,
                            double* corr_dev, int32_t* n_corr_dev, void* stream) {
  if (row_cap < 1 || row_cap > ROW_CAP_MAX || cap < 1 || cap > SSP_MATCH_MAX_POINTS || point_cap < 1 ||
      point_cap > SSP_MATCH_MAX_POINTS || pt_stride < 2)
    return fail(-1, "landmark_matches: 1 <= row_cap <= %d, 1 <= cap, point_cap <= %d and pt_stride >= 2 required (row_cap %d, cap %d, "
                "point_cap %d)", ROW_CAP_MAX, SSP_MATCH_MAX_POINTS, row_cap, cap, point_cap);
  if (!landmarks_dev || !n_landmarks_dev || !match_dev || !n_match_dev || !pts_new_dev || !corr_dev || !n_corr_dev)
    return fail(-1, "landmark_matches: null pointer");
  return launch<landmark_corr_kernel>(dim3(1), dim3(PNP_THREADS), (size_t)point_cap * sizeof(int), (hipStream_t)stream,
                                      landmarks_dev, n_landmarks_dev, row_cap, match_dev, n_match_dev, cap, pts_new_dev, pt_stride,
                                      point_cap, corr_dev, n_corr_dev);
}

int ssp_pnp_ransac(const double* corr_dev, const int32_t* n_dev, int cap, int n_problems, const double* intr_dev, int n_intr,
                   const uint64_t* seeds_dev, double thresh, int min_inliers, int groups, void* workspace_dev, double* rw_dev,
                   double* c_dev, uint8_t* mask_dev, int32_t* n_inlier_dev, int32_t* winner_dev, double* rms_dev,
                   int32_t* status_dev, void* stream) {
  if (cap < 1 || cap > SSP_MATCH_MAX_POINTS || n_problems < 1 || n_problems > 65535)
    return fail(-1, "pnp_ransac: 1 <= cap <= %d and 1 <= n_problems <= 65535 required (cap %d, n_problems %d)", SSP_MATCH_MAX_POINTS,
                cap, n_problems);
  if (!corr_dev || !n_dev || !intr_dev || !seeds_dev || !workspace_dev || !rw_dev || !c_dev || !mask_dev || !n_inlier_dev ||
      !winner_dev || !rms_dev || !status_dev)
    return fail(-1, "pnp_ransac: null pointer");
  CHK(intr_check("pnp_ransac", n_intr, n_problems, "n_problems", "problems"));
  CHK(finite_nonneg_check("pnp_ransac", "thresh", thresh));
  if (min_inliers < 4) return fail(-1, "pnp_ransac: min_inliers >= 4 required (got %d)", min_inliers);
  if (groups < 0 || groups > PNP_MAX_GROUPS)
    return fail(-1, "pnp_ransac: 0 (the library's choice) <= groups <= %d required (got %d)", PNP_MAX_GROUPS, groups);
  if (groups == 0) groups = PNP_GROUPS_DEFAULT;
  hipStream_t st = (hipStream_t)stream;
  uint64_t* keys = reinterpret_cast<uint64_t*>(workspace_dev);
  hipLaunchKernelGGL(pnp_hypotheses_kernel, dim3(groups, n_problems), dim3(PNP_THREADS), 0, st, corr_dev, n_dev, cap, intr_dev, n_intr,
                     seeds_dev, thresh, keys);
  hipLaunchKernelGGL(pnp_finish_kernel, dim3(n_problems), dim3(PNP_THREADS), 0, st, corr_dev, n_dev, cap, intr_dev, n_intr, seeds_dev,
                     thresh, min_inliers, groups, (const uint64_t*)keys, rw_dev, c_dev, mask_dev, n_inlier_dev, winner_dev, rms_dev,
                     status_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_pose_repair(const double* rw_dev, const double* c_dev, const int32_t* status_dev, int n_seq, double* state_dev,
                    double* table_dev, int capacity, void* stream) {
  CHK(seq_check("pose_repair", n_seq, capacity));
  if (!rw_dev || !c_dev || !status_dev || !state_dev || (capacity > 0 && !table_dev)) return fail(-1, "pose_repair: null pointer");
  return launch<pose_repair_kernel>(dim3(cdiv(n_seq, 64)), dim3(64), 0, (hipStream_t)stream, rw_dev, c_dev, status_dev, n_seq,
                                    state_dev, table_dev, capacity);
}

// ---- windowed bundle adjustment: Levenberg-Marquardt over the window's cameras and landmarks, the write-back ----
static_assert(BA_INFO_WORDS == SSP_BA_INFO_WORDS && BA_FLAG_ADJUSTED == SSP_POSE_FLAG_ADJUSTED && BA_MAX_ITERATIONS == SSP_BA_MAX_ITERATIONS,
              "include/ssp_hip.h and ba_kernels.hip.h disagree");
size_t ssp_ba_workspace_bytes(int max_length, int row_cap) {
  if (track_check("ba_workspace_bytes", max_length, 1, row_cap)) return 0;
  return align_up(ba_ws_words(max_length, row_cap) * sizeof(double), 256);
}

int ssp_bundle_adjust(const int32_t* ids_dev, const int32_t* state_dev, const double* pts_dev, int first_slot, const double* cams_dev,
                      int max_length, int point_cap, int row_cap, const double* x_dev, const int32_t* status_dev, int iterations,
                      double* cams_out_dev, double* x_out_dev, double* rms_out_dev, double* info_dev, void* workspace_dev,
                      void* stream) {
  CHK(track_check("bundle_adjust", max_length, point_cap, row_cap));
  if (first_slot < 0 || first_slot >= max_length)
    return fail(-1, "bundle_adjust: 0 <= first_slot < max_length required (got %d)", first_slot);
  if (iterations < 1 || iterations > SSP_BA_MAX_ITERATIONS)
    return fail(-1, "bundle_adjust: 1 <= iterations <= %d required (got %d)", SSP_BA_MAX_ITERATIONS, iterations);
  if (!ids_dev || !state_dev || !pts_dev || !cams_dev || !x_dev || !status_dev || !cams_out_dev || !x_out_dev || !rms_out_dev ||
      !info_dev || !workspace_dev)
    return fail(-1, "bundle_adjust: null pointer");
  if (cams_out_dev == cams_dev || x_out_dev == x_dev) return fail(-1, "bundle_adjust: the outputs must not alias the inputs");
  hipStream_t st = (hipStream_t)stream;
  const int L = max_length, tiles = cdiv(row_cap, BA_THREADS);
  const BaWs w = ba_ws_of(reinterpret_cast<double*>(workspace_dev), L, row_cap);
  const size_t stage = ba_stage_bytes(L);
  hipLaunchKernelGGL(ba_init_kernel, dim3(tiles), dim3(BA_THREADS), 0, st, cams_dev, x_dev, L, row_cap, cams_out_dev, x_out_dev, w.ctl);
  for (int it = 0; it < iterations; ++it) {
    const double* ctl = w.ctl + (size_t)it * BA_CTL_WORDS;
    hipLaunchKernelGGL(ba_linearise_kernel, dim3(tiles), dim3(BA_THREADS), stage, st, ids_dev, state_dev, pts_dev, first_slot,
                       (const double*)cams_out_dev, (const double*)x_out_dev, status_dev, L, point_cap, row_cap, ctl, w.part);
    CHK(launch_lds<ba_solve_kernel>(ba_solve_lds_bytes(SSP_TRACK_MAX_LENGTH), dim3(1), dim3(BA_THREADS), ba_solve_lds_bytes(L), st,
                                    (const double*)w.part, tiles, (const double*)cams_out_dev, L, ctl, w.sol, w.cand_cams));
    hipLaunchKernelGGL(ba_backsub_kernel, dim3(tiles), dim3(BA_THREADS), stage, st, ids_dev, state_dev, pts_dev, first_slot,
                       (const double*)cams_out_dev, (const double*)x_out_dev, status_dev, L, point_cap, row_cap, ctl,
                       (const double*)w.sol, (const double*)w.cand_cams, w.x_cand, w.cpart);
    hipLaunchKernelGGL(ba_accept_kernel, dim3(tiles), dim3(BA_THREADS), 0, st, state_dev, status_dev, L, row_cap, it, ctl,
                       w.ctl + (size_t)(it + 1) * BA_CTL_WORDS, (const double*)w.sol, (const double*)w.cpart,
                       (const double*)w.cand_cams, (const double*)w.x_cand, cams_out_dev, x_out_dev);
  }
  hipLaunchKernelGGL(ba_finish_kernel, dim3(tiles), dim3(BA_THREADS), stage, st, ids_dev, state_dev, pts_dev, first_slot,
                     (const double*)cams_out_dev, (const double*)x_out_dev, status_dev, L, point_cap, row_cap,
                     (const double*)(w.ctl + (size_t)iterations * BA_CTL_WORDS), rms_out_dev, info_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_ba_apply(const double* info_dev, const double* cams_dev, int max_length, int n_seq, int n_frames, double* state_dev,
                 double* table_dev, int capacity, void* stream) {
  CHK(track_check("ba_apply", max_length, 1, 1));
  CHK(seq_check("ba_apply", n_seq, capacity));
  if (!info_dev || !cams_dev || !state_dev || (capacity > 0 && !table_dev)) return fail(-1, "ba_apply: null pointer");
  return launch<ba_apply_kernel>(dim3(cdiv(n_seq, 64)), dim3(64), 0, (hipStream_t)stream, info_dev, cams_dev, max_length, n_seq,
                                 n_frames, state_dev, table_dev, capacity);
}

// ---- world map: the store, the map matcher, the join, the repair ----
static_assert(WORLD_STATE_WORDS == SSP_WORLD_STATE_WORDS && WORLD_MAX_ROWS == SSP_WORLD_MAX_ROWS && WORLD_FLAG_WORLD == SSP_POSE_FLAG_WORLD &&
              WORLD_MAX_BLOCKS * WORLD_BLOCK == SSP_TRACK_MAX_LENGTH * SSP_MATCH_MAX_POINTS && WORLD_MAX_ROWS % WORLD_STRIP == 0,
              "include/ssp_hip.h and world_kernels.hip.h disagree");
static int world_check(const char* what, int map_cap, int cap) {
  if (map_cap < 1 || map_cap > SSP_WORLD_MAX_ROWS || cap < 1 || cap > SSP_MATCH_MAX_POINTS)
    return fail(-1, "%s: 1 <= map_cap <= %d and 1 <= cap <= %d required (map_cap %d, cap %d)", what, SSP_WORLD_MAX_ROWS,
                SSP_MATCH_MAX_POINTS, map_cap, cap);
  return 0;
}

// one int32 array: the header, three counters per block, the class of every landmark row
struct WorldInsertWs {
  int32_t *hdr, *bcount, *cls;  // [WORLD_HDR_WORDS], [3][WORLD_MAX_BLOCKS], [row_cap], back to back
  size_t bytes;
};
static WorldInsertWs world_insert_carve(int row_cap, void* base) {
  Carver c{reinterpret_cast<char*>(base), 0};
  WorldInsertWs w;
  w.hdr = c.take<int32_t>((size_t)WORLD_HDR_WORDS + 3 * WORLD_MAX_BLOCKS + row_cap);
  w.bcount = base ? w.hdr + WORLD_HDR_WORDS : nullptr;
  w.cls = base ? w.bcount + 3 * WORLD_MAX_BLOCKS : nullptr;
  w.bytes = align_up(c.off, 256);
  return w;
}

size_t ssp_world_insert_workspace_bytes(int row_cap) {
  if (row_cap < 1 || row_cap > ROW_CAP_MAX) {
    fail(-1, "world_insert_workspace_bytes: 1 <= row_cap <= %d required (got %d)", ROW_CAP_MAX, row_cap);
    return 0;
  }
  return world_insert_carve(row_cap, nullptr).bytes;
}

size_t ssp_match_world_workspace_bytes(int map_cap, int cap) {
  if (world_check("match_world_workspace_bytes", map_cap, cap)) return 0;
  return match_carve(map_cap, cap, nullptr).bytes;
}

int ssp_op_world_insert(const double* landmarks_dev, const int32_t* n_landmarks_dev, int row_cap, const float* desc_new_dev,
                        const int32_t* count_new_dev, int point_cap, const double* table_dev, int capacity, int n_frames, int patience,
                        int map_cap, int tid_cap, double* x_dev, float* desc_dev, int32_t* tid_dev, int32_t* views_dev,
                        int32_t* first_dev, int32_t* last_dev, double* rms_dev, int32_t* slot_of_tid_dev, int32_t* state_dev,
                        void* workspace_dev, void* stream) {
  CHK(world_check("world_insert", map_cap, point_cap));
  if (row_cap < 1 || row_cap > ROW_CAP_MAX || tid_cap < 1 || capacity < 0 || patience < 0)
    return fail(-1, "world_insert: 1 <= row_cap <= %d, tid_cap >= 1, capacity >= 0 and patience >= 0 required (row_cap %d, tid_cap %d, "
                "capacity %d, patience %d)", ROW_CAP_MAX, row_cap, tid_cap, capacity, patience);
  if (!landmarks_dev || !n_landmarks_dev || !desc_new_dev || !count_new_dev || (capacity > 0 && !table_dev) || !x_dev || !desc_dev ||
      !tid_dev || !views_dev || !first_dev || !last_dev || !rms_dev || !slot_of_tid_dev || !state_dev || !workspace_dev)
    return fail(-1, "world_insert: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const WorldInsertWs w = world_insert_carve(row_cap, workspace_dev);
  const int nb = cdiv(row_cap, WORLD_BLOCK);
  hipLaunchKernelGGL(world_anchor_kernel, dim3(1), dim3(64), 0, st, state_dev, map_cap, table_dev, capacity, n_frames, patience, w.hdr);
  hipLaunchKernelGGL(world_classify_kernel, dim3(nb), dim3(WORLD_BLOCK), 0, st, (const int32_t*)w.hdr, landmarks_dev, n_landmarks_dev,
                     row_cap, count_new_dev, point_cap, (const int32_t*)tid_dev, (const int32_t*)slot_of_tid_dev, tid_cap, w.cls, w.bcount);
  hipLaunchKernelGGL(world_scatter_kernel, dim3(nb), dim3(WORLD_BLOCK), 0, st, (const int32_t*)w.hdr, landmarks_dev, row_cap, desc_new_dev,
                     point_cap, (const int32_t*)w.cls, (const int32_t*)w.bcount, nb, n_frames, map_cap, x_dev, desc_dev, tid_dev, views_dev,
                     first_dev, last_dev, rms_dev, slot_of_tid_dev, state_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_match_world(const float* desc_dev, const int32_t* state_dev, int map_cap, const float* desc2_dev, const int32_t* count2_dev,
                    int cap, float nn_thresh, void* workspace_dev, float* match_dev, int32_t* n_match_dev, void* stream) {
  CHK(world_check("match_world", map_cap, cap));
  if (!(nn_thresh >= 0.f)) return fail(-1, "match_world: nn_thresh must be non-negative");
  if (!desc_dev || !state_dev || !desc2_dev || !count2_dev || !workspace_dev || !match_dev || !n_match_dev)
    return fail(-1, "match_world: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const MatchWs w = match_carve(map_cap, cap, workspace_dev);
  HIPCHK(hipMemsetAsync(w.rowmin, 0xFF, w.keys * sizeof(uint64_t), st));
  hipLaunchKernelGGL(world_match_kernel<false>, dim3(cdiv(map_cap, WORLD_STRIP), WORLD_SPLIT_MAX), dim3(256), 0, st, desc_dev, state_dev, map_cap,
                     desc2_dev, count2_dev, cap, w.rowmin, w.colmin, WorldClasses{});
  hipLaunchKernelGGL(world_compact_kernel, dim3(1), dim3(WORLD_BLOCK), 0, st, (const uint64_t*)w.rowmin, (const uint64_t*)w.colmin, state_dev,
                     map_cap, count2_dev, cap, nn_thresh, match_dev, n_match_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_world_correspondences(const double* x_dev, const int32_t* state_dev, int map_cap, const float* match_dev,
                                 const int32_t* n_match_dev, int cap, const double* pts_new_dev, int pt_stride,
                                 const int32_t* count_new_dev, int point_cap, double* corr_dev, int32_t* n_corr_dev, void* stream) {
  CHK(world_check("world_correspondences", map_cap, cap));
  if (point_cap < 1 || point_cap > SSP_MATCH_MAX_POINTS || pt_stride < 2)
    return fail(-1, "world_correspondences: 1 <= point_cap <= %d and pt_stride >= 2 required (point_cap %d, pt_stride %d)",
                SSP_MATCH_MAX_POINTS, point_cap, pt_stride);
  if (!x_dev || !state_dev || !match_dev || !n_match_dev || !pts_new_dev || !count_new_dev || !corr_dev || !n_corr_dev)
    return fail(-1, "world_correspondences: null pointer");
  return launch<world_corr_kernel>(dim3(1), dim3(256), 0, (hipStream_t)stream, x_dev, state_dev, map_cap, match_dev, n_match_dev,
                                   cap, pts_new_dev, pt_stride, count_new_dev, point_cap, corr_dev, n_corr_dev);
}

int ssp_world_repair(const double* rw_dev, const double* c_dev, const int32_t* status_dev, double* state_dev, double* table_dev,
                     int capacity, int map_cap, int32_t* world_state_dev, void* stream) {
  if (capacity < 0 || map_cap < 1 || map_cap > SSP_WORLD_MAX_ROWS)
    return fail(-1, "world_repair: capacity >= 0 and 1 <= map_cap <= %d required (capacity %d, map_cap %d)", SSP_WORLD_MAX_ROWS, capacity,
                map_cap);
  if (!rw_dev || !c_dev || !status_dev || !state_dev || (capacity > 0 && !table_dev) || !world_state_dev)
    return fail(-1, "world_repair: null pointer");
  return launch<world_repair_kernel>(dim3(1), dim3(64), 0, (hipStream_t)stream, rw_dev, c_dev, status_dev, state_dev, table_dev,
                                     capacity, map_cap, world_state_dev);
}

// ---- loop closure: the join against old rows, the loop edge, the pose graph, the write-back ----
static_assert(LOOP_MAX_EDGES == SSP_LOOP_MAX_EDGES && LOOP_EDGE_WORDS == SSP_LOOP_EDGE_WORDS && LOOP_STATE_WORDS == SSP_LOOP_STATE_WORDS &&
              LOOP_CAND_WORDS == SSP_LOOP_CAND_WORDS && LOOP_MAX_INNER == SSP_LOOP_MAX_INNER && LOOP_INFO_WORDS == SSP_LOOP_INFO_WORDS &&
              LOOP_FLAG_LOOP == SSP_POSE_FLAG_LOOP && LOOP_MAX_ITERATIONS == SSP_LOOP_MAX_ITERATIONS,
              "include/ssp_hip.h and loop_kernels.hip.h disagree");
size_t ssp_pose_graph_workspace_bytes(int capacity) {
  if (capacity < 2 || capacity > (1 << 20)) {
    fail(-1, "pose_graph_workspace_bytes: 2 <= capacity <= %d required (got %d)", 1 << 20, capacity);
    return 0;
  }
  return align_up(loop_ws_words(capacity) * sizeof(double), 256);
}

int ssp_op_loop_correspondences(const double* x_dev, const int32_t* last_dev, const int32_t* state_dev, int map_cap,
                                const float* match_dev, const int32_t* n_match_dev, int cap, const double* pts_new_dev, int pt_stride,
                                const int32_t* count_new_dev, int point_cap, const double* landmarks_dev,
                                const int32_t* n_landmarks_dev, int row_cap, int f, int min_gap, double* corr_dev, double* xnew_dev,
                                int32_t* n_dev, void* stream) {
  CHK(world_check("loop_correspondences", map_cap, cap));
  if (point_cap < 1 || point_cap > SSP_MATCH_MAX_POINTS || pt_stride < 2 || row_cap < 1 || row_cap > ROW_CAP_MAX)
    return fail(-1, "loop_correspondences: 1 <= point_cap <= %d, pt_stride >= 2 and 1 <= row_cap <= %d required (point_cap %d, pt_stride "
                "%d, row_cap %d)", SSP_MATCH_MAX_POINTS, ROW_CAP_MAX, point_cap, pt_stride, row_cap);
  if (f < 0 || min_gap < 1) return fail(-1, "loop_correspondences: f >= 0 and min_gap >= 1 required (f %d, min_gap %d)", f, min_gap);
  if (!x_dev || !last_dev || !state_dev || !match_dev || !n_match_dev || !pts_new_dev || !count_new_dev || !landmarks_dev ||
      !n_landmarks_dev || !corr_dev || !xnew_dev || !n_dev)
    return fail(-1, "loop_correspondences: null pointer");
  return launch<loop_corr_kernel>(dim3(1), dim3(256), (size_t)point_cap * sizeof(int), (hipStream_t)stream, x_dev, last_dev,
                                  state_dev, map_cap, match_dev, n_match_dev, cap, pts_new_dev, pt_stride, count_new_dev, point_cap,
                                  landmarks_dev, n_landmarks_dev, row_cap, f, min_gap, corr_dev, xnew_dev, n_dev);
}

int ssp_loop_edge(const double* rw_dev, const double* c_dev, const uint8_t* mask_dev, const int32_t* status_dev,
                  const double* corr_dev, const double* xnew_dev, const int32_t* n_dev, int cap, const int32_t* last_dev, int map_cap,
                  const double* table_dev, int capacity, int f, int min_inliers, int cooldown, double weight, double* edges_dev,
                  int32_t* state_dev, double* cand_dev, void* stream) {
  CHK(world_check("loop_edge", map_cap, cap));
  if (capacity < 1 || f < 0 || min_inliers < 4 || cooldown < 0)
    return fail(-1, "loop_edge: capacity >= 1, f >= 0, min_inliers >= 4 and cooldown >= 0 required (capacity %d, f %d, min_inliers %d, "
                "cooldown %d)", capacity, f, min_inliers, cooldown);
  if (!(weight > 0.0) || !std::isfinite(weight)) return fail(-1, "loop_edge: a finite weight > 0 is required");
  if (!rw_dev || !c_dev || !mask_dev || !status_dev || !corr_dev || !xnew_dev || !n_dev || !last_dev || !table_dev || !edges_dev ||
      !state_dev || !cand_dev)
    return fail(-1, "loop_edge: null pointer");
  return launch<loop_edge_kernel>(dim3(1), dim3(256), 0, (hipStream_t)stream, rw_dev, c_dev, mask_dev, status_dev, corr_dev,
                                  xnew_dev, n_dev, cap, last_dev, map_cap, table_dev, capacity, f, min_inliers, cooldown, weight,
                                  edges_dev, state_dev, cand_dev);
}

int ssp_pose_graph(const double* table_dev, int capacity, const double* edges_dev, const int32_t* state_dev, int f, int iterations,
                   void* workspace_dev, double* rw_out_dev, double* c_out_dev, double* sigma_out_dev, double* info_dev, void* stream) {
  if (capacity < 2 || capacity > (1 << 20) || f < 0)
    return fail(-1, "pose_graph: 2 <= capacity <= %d and f >= 0 required (capacity %d, f %d)", 1 << 20, capacity, f);
  if (iterations < 1 || iterations > SSP_LOOP_MAX_ITERATIONS)
    return fail(-1, "pose_graph: 1 <= iterations <= %d required (got %d)", SSP_LOOP_MAX_ITERATIONS, iterations);
  if (!table_dev || !edges_dev || !state_dev || !workspace_dev || !rw_out_dev || !c_out_dev || !sigma_out_dev || !info_dev)
    return fail(-1, "pose_graph: null pointer");
  return launch<loop_graph_kernel>(dim3(1), dim3(LOOP_THREADS), 0, (hipStream_t)stream, table_dev, capacity, edges_dev, state_dev,
                                   f, iterations, reinterpret_cast<double*>(workspace_dev), rw_out_dev, c_out_dev, sigma_out_dev,
                                   info_dev);
}

int ssp_loop_apply(const double* info_dev, const double* rw_new_dev, const double* c_new_dev, const double* sigma_dev,
                   int32_t* loop_state_dev, int f, double* state_dev, double* table_dev, int capacity, double* x_dev,
                   const int32_t* last_dev, const int32_t* world_state_dev, int map_cap, void* stream) {
  if (capacity < 2 || f < 0 || map_cap < 1 || map_cap > SSP_WORLD_MAX_ROWS)
    return fail(-1, "loop_apply: capacity >= 2, f >= 0 and 1 <= map_cap <= %d required (capacity %d, f %d, map_cap %d)", SSP_WORLD_MAX_ROWS,
                capacity, f, map_cap);
  if (!info_dev || !rw_new_dev || !c_new_dev || !sigma_dev || !loop_state_dev || !state_dev || !table_dev || !x_dev || !last_dev ||
      !world_state_dev)
    return fail(-1, "loop_apply: null pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loop_apply_map_kernel, dim3(cdiv(map_cap, 256)), dim3(256), 0, st, info_dev, rw_new_dev, c_new_dev, sigma_dev,
                     loop_state_dev, f, (const double*)table_dev, capacity, x_dev, last_dev, world_state_dev, map_cap);
  hipLaunchKernelGGL(loop_apply_rows_kernel, dim3(cdiv(capacity, 256)), dim3(256), 0, st, info_dev, rw_new_dev, c_new_dev,
                     (const int32_t*)loop_state_dev, f, state_dev, table_dev, capacity);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- streamed descriptor metrics: pixel homographies of the trainer's pairs, per-pair rows and running sums ----
static_assert(EVAL_ACC_MAX_PAIRS == SSP_EVAL_ACC_MAX_PAIRS && EVAL_ROW_WORDS == SSP_EVAL_ROW_WORDS && EVAL_STATE_WORDS == SSP_EVAL_STATE_WORDS,
              "include/ssp_hip.h and eval_kernels.hip.h disagree");
int ssp_eval_pixel_homographies(const float* hn_dev, int n_pairs, int height, int width, double* hom_dev, double* hom_inv_dev,
                                void* stream) {
  if (!hn_dev || !hom_dev || !hom_inv_dev) return fail(-1, "eval_pixel_homographies: null pointer");
  if (n_pairs < 1 || height < 1 || width < 1) return fail(-1, "eval_pixel_homographies: n_pairs, height, width >= 1 required");
  return launch<eval_pixel_hom_kernel>(dim3(cdiv(n_pairs, 64)), dim3(64), 0, (hipStream_t)stream, hn_dev, n_pairs, height, width,
                                       hom_dev, hom_inv_dev);
}

int ssp_eval_accumulate(const double* rep_dev, const double* h_dev, const int32_t* n_inlier_dev, const int32_t* status_dev,
                        const double* ap_dev, const int32_t* n1_dev, int pair_stride, const double* hom_dev, int n_pairs,
                        int corner_h, int corner_w, const double* thresholds, int64_t first_pair, double* rows_dev,
                        int64_t capacity, double* state_dev, void* stream) {
  if (n_pairs < 1 || n_pairs > EVAL_ACC_MAX_PAIRS)
    return fail(-1, "eval_accumulate: 1 <= n_pairs <= %d per call (got %d)", EVAL_ACC_MAX_PAIRS, n_pairs);
  if (!rows_dev || !state_dev || !thresholds) return fail(-1, "eval_accumulate: null pointer");
  if (capacity < 1 || first_pair < 0) return fail(-1, "eval_accumulate: capacity >= 1 and first_pair >= 0 required");
  const int n_ransac = (h_dev != nullptr) + (n_inlier_dev != nullptr) + (status_dev != nullptr) + (ap_dev != nullptr) +
                       (n1_dev != nullptr) + (hom_dev != nullptr);
  if (n_ransac != 0 && n_ransac != 6)
    return fail(-1, "eval_accumulate: H, n_inliers, status, ap, n1 and the true homographies come together or not at all");
  if (!rep_dev && n_ransac == 0) return fail(-1, "eval_accumulate: neither the repeatability rows nor the RANSAC results");
  if (n_ransac && (pair_stride < 1 || corner_h < 1 || corner_w < 1))
    return fail(-1, "eval_accumulate: pair_stride, corner_h, corner_w >= 1 required");
  EvalThresholds thr;
  for (int k = 0; k < 6; ++k) thr.t[k] = thresholds[k];
  return launch<eval_accumulate_kernel>(dim3(1), dim3(EVAL_ACC_MAX_PAIRS), 0, (hipStream_t)stream, rep_dev, h_dev, n_inlier_dev,
                                        status_dev, ap_dev, n1_dev, pair_stride, hom_dev, n_pairs, corner_h, corner_w, thr,
                                        (long long)first_pair, rows_dev, (long long)capacity, state_dev);
}

// ---- detector evaluation against ground-truth corners (evaluations/detector_evaluation.py:15-136) ----
static_assert(DET_MAX_R2 == SSP_DET_EVAL_MAX_R2 && DET_STATE_WORDS == SSP_DET_EVAL_STATE_WORDS && DET_CURVE_TILE == SSP_DET_EVAL_CURVE_TILE,
              "include/ssp_hip.h and detector_eval_kernels.hip.h disagree");
struct DetWs {
  unsigned long long* best;  // [b][H*W]
  int32_t* gidx;             // [b][items]
  int32_t* block_sums;       // [nb]
  int32_t* block_offs;       // [nb + 1]
  size_t bytes;
};
static long det_items(const ssp_det_eval_params* p, int b, int cap) { return (long)b * (cap > 0 ? (long)cap : (long)p->height * p->width); }
static DetWs det_carve(const ssp_det_eval_params* p, int b, int cap, void* base) {
  Carver c{reinterpret_cast<char*>(base), 0};
  const long items = det_items(p, b, cap);
  const size_t nb = (size_t)cdiv(items, DET_BLOCK);
  DetWs w;
  w.best = c.take<unsigned long long>((size_t)b * p->height * p->width);
  w.gidx = c.take<int32_t>((size_t)items);
  w.block_sums = c.take<int32_t>(nb);
  w.block_offs = c.take<int32_t>(nb + 1);
  w.bytes = align_up(c.off, 256);
  return w;
}
static int det_check(const char* what, const ssp_det_eval_params* p, int b, int cap) {
  if (!p || p->height < 1 || p->width < 1 || b < 1 || cap < 0)
    return fail(-1, "%s: height, width, batch >= 1 and cap >= 0 required", what);
  if (p->r2 < 0 || p->r2 > SSP_DET_EVAL_MAX_R2)
    return fail(-1, "%s: 0 <= r2 <= %d required (got %d): the squared match radius in pixels", what, SSP_DET_EVAL_MAX_R2, p->r2);
  if (!(p->remove_zero >= 0.f) || !(p->prob_thresh >= 0.f))
    return fail(-1, "%s: remove_zero >= 0 and prob_thresh >= 0 required (candidates are positive probabilities)", what);
  if ((double)b * p->height * p->width >= 2147483648.0 || (double)b * cap >= 2147483648.0)
    return fail(-1, "%s: batch x height x width (or batch x cap) exceeds 2^31: lower the batch", what);
  if (p->prob_thresh < p->remove_zero)
    return fail(-1, "%s: prob_thresh >= remove_zero required (only candidates, prob > remove_zero, reach the localisation histogram)", what);
  return 0;
}

size_t ssp_det_eval_workspace_bytes(const ssp_det_eval_params* p, int b, int cap) {
  if (det_check("det_eval_workspace_bytes", p, b, cap)) return 0;
  return det_carve(p, b, cap, nullptr).bytes;
}

static int det_tp_fp(bool points, const float* src, const int32_t* count, int cap, const void* labels, int labels_u8, const ssp_det_eval_params* p,
                     int b, void* workspace, int64_t* keys, int64_t capacity, int64_t* state, hipStream_t st) {
  const DetWs w = det_carve(p, b, cap, workspace);
  DetParams P;
  P.H = p->height; P.W = p->width; P.r2 = p->r2; P.simplified = p->simplified ? 1 : 0; P.labels_u8 = labels_u8 ? 1 : 0;
  P.remove_zero = p->remove_zero; P.prob_thresh = p->prob_thresh;
  P.r = 0;
  while ((P.r + 1) * (P.r + 1) <= P.r2) ++P.r;
  const long items = det_items(p, b, cap), n_pix = (long)b * p->height * p->width;
  const int n_items = (int)(items / b), nb = cdiv(items, DET_BLOCK);
  unsigned long long* ust = reinterpret_cast<unsigned long long*>(state);
  HIPCHK(hipMemsetAsync(w.best, 0, (size_t)n_pix * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(points ? det_match_kernel<true> : det_match_kernel<false>, dim3(nb), dim3(DET_BLOCK), 0, st, src, count, labels,
                     P, n_items, items, w.best, w.gidx, w.block_sums, ust);
  hipLaunchKernelGGL(det_offsets_kernel, dim3(1), dim3(DET_BLOCK), 0, st, (const int32_t*)w.block_sums, nb, w.block_offs);
  hipLaunchKernelGGL(points ? det_emit_kernel<true> : det_emit_kernel<false>, dim3(nb), dim3(DET_BLOCK), 0, st, src, count, P, n_items, items,
                     (const unsigned long long*)w.best, (const int32_t*)w.gidx, (const int32_t*)w.block_offs,
                     reinterpret_cast<unsigned long long*>(keys), (long long)capacity, ust);
  hipLaunchKernelGGL(det_finish_kernel, dim3(cdiv(n_pix, DET_BLOCK)), dim3(DET_BLOCK), 0, st, labels, P, n_pix,
                     (const unsigned long long*)w.best, (const int32_t*)w.block_offs, nb, ust);
  HIPCHK(hipGetLastError());
  return 0;
}

static int det_buffers_check(const char* what, const void* labels, const void* workspace, const int64_t* keys, int64_t capacity,
                             const int64_t* state) {
  if (!labels || !workspace || !keys || !state) return fail(-1, "%s: null pointer", what);
  if (capacity < 1 || capacity > 2147483647LL)
    return fail(-1, "%s: 1 <= capacity < 2^31 records required (the record index is 31 bits of the key)", what);
  return 0;
}

int ssp_op_det_tp_fp(const float* prob_dev, const void* labels_dev, int labels_u8, const ssp_det_eval_params* p, int b,
                     void* workspace_dev, int64_t* keys_dev, int64_t capacity, int64_t* state_dev, void* stream) {
  CHK(det_check("det_tp_fp", p, b, 0));
  if (!prob_dev) return fail(-1, "det_tp_fp: null pointer");
  CHK(det_buffers_check("det_tp_fp", labels_dev, workspace_dev, keys_dev, capacity, state_dev));
  return det_tp_fp(false, prob_dev, nullptr, 0, labels_dev, labels_u8, p, b, workspace_dev, keys_dev, capacity, state_dev,
                          (hipStream_t)stream);
}

int ssp_op_det_tp_fp_points(const float* pts_dev, const int32_t* count_dev, int cap, const void* labels_dev, int labels_u8,
                            const ssp_det_eval_params* p, int b, void* workspace_dev, int64_t* keys_dev, int64_t capacity,
                            int64_t* state_dev, void* stream) {
  CHK(det_check("det_tp_fp_points", p, b, cap));
  if (cap < 1) return fail(-1, "det_tp_fp_points: cap >= 1 rows per image required");
  if (!pts_dev || !count_dev) return fail(-1, "det_tp_fp_points: null pointer");
  CHK(det_buffers_check("det_tp_fp_points", labels_dev, workspace_dev, keys_dev, capacity, state_dev));
  return det_tp_fp(true, pts_dev, count_dev, cap, labels_dev, labels_u8, p, b, workspace_dev, keys_dev, capacity, state_dev,
                         (hipStream_t)stream);
}

struct DetCurveWs {
  int32_t *block_sums, *block_offs;
  double *block_max, *suffix, *partial;
  size_t bytes;
};
static DetCurveWs det_curve_carve(int64_t n, void* base) {
  Carver c{reinterpret_cast<char*>(base), 0};
  const size_t nb = (size_t)std::max<int64_t>(cdiv(n, (int64_t)DET_CURVE_TILE), 1);
  DetCurveWs w;
  w.block_max = c.take<double>(nb);
  w.suffix = c.take<double>(nb);
  w.partial = c.take<double>(nb);
  w.block_sums = c.take<int32_t>(nb);
  w.block_offs = c.take<int32_t>(nb + 1);
  w.bytes = align_up(c.off, 256);
  return w;
}

size_t ssp_det_pr_curve_workspace_bytes(int64_t n_records) {
  if (n_records < 0 || n_records > 2147483647LL) {
    fail(-1, "det_pr_curve_workspace_bytes: 0 <= n_records < 2^31 required");
    return 0;
  }
  return det_curve_carve(n_records, nullptr).bytes;
}

int ssp_op_det_pr_curve(const int64_t* sorted_keys_dev, int64_t n_records, const int64_t* state_dev, void* workspace_dev,
                        float* prob_dev, uint8_t* tp_dev, double* precision_dev, double* recall_dev, double* map_dev,
                        void* stream) {
  if (n_records < 0 || n_records > 2147483647LL) return fail(-1, "det_pr_curve: 0 <= n_records < 2^31 required");
  if (!state_dev || !workspace_dev || !precision_dev || !recall_dev || !map_dev ||
      (n_records > 0 && (!sorted_keys_dev || !prob_dev || !tp_dev)))
    return fail(-1, "det_pr_curve: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const DetCurveWs w = det_curve_carve(n_records, workspace_dev);
  const long long n = n_records;
  const int nb = (int)std::max<int64_t>(cdiv(n_records, (int64_t)DET_CURVE_TILE), 1);
  const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(sorted_keys_dev);
  const unsigned long long* ust = reinterpret_cast<const unsigned long long*>(state_dev);
  hipLaunchKernelGGL(det_curve_count_kernel, dim3(nb), dim3(DET_BLOCK), 0, st, keys, n, w.block_sums);
  hipLaunchKernelGGL(det_offsets_kernel, dim3(1), dim3(DET_BLOCK), 0, st, (const int32_t*)w.block_sums, nb, w.block_offs);
  hipLaunchKernelGGL(det_curve_pr_kernel, dim3(nb), dim3(DET_BLOCK), 0, st, keys, n, ust, (const int32_t*)w.block_offs, prob_dev,
                     tp_dev, precision_dev, recall_dev, w.block_max);
  hipLaunchKernelGGL(det_suffix_blocks_kernel, dim3(1), dim3(DET_BLOCK), 0, st, (const double*)w.block_max, nb, w.suffix);
  hipLaunchKernelGGL(det_curve_final_kernel, dim3(nb), dim3(DET_BLOCK), 0, st, n, (const double*)w.suffix,
                     (const double*)recall_dev, precision_dev, w.partial);
  hipLaunchKernelGGL(det_sum_kernel, dim3(1), dim3(DET_BLOCK), 0, st, (const double*)w.partial, nb, map_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- pair construction for real data ----
int ssp_op_sample_homographies(uint64_t seed, const ssp_homography_params* p, int b, float* h_dev, float* inv_h_dev,
                               void* stream) {
  if (!p || !h_dev || !inv_h_dev || b < 1) return fail(-1, "sample_homographies: bad argument");
  if (p->n_scales < 0 || p->n_scales > 16 || p->n_angles < 0 || p->n_angles > 63 || p->patch_ratio <= 0.f || p->patch_ratio > 1.f)
    return fail(-1, "sample_homographies: n_scales <= 16, n_angles <= 63, 0 < patch_ratio <= 1 required");
  HomographyParams q;
  q.perspective = p->perspective; q.scaling = p->scaling; q.rotation = p->rotation; q.translation = p->translation;
  q.allow_artifacts = p->allow_artifacts; q.n_scales = p->n_scales; q.n_angles = p->n_angles;
  q.scaling_amplitude = p->scaling_amplitude; q.perspective_amplitude_x = p->perspective_amplitude_x;
  q.perspective_amplitude_y = p->perspective_amplitude_y; q.patch_ratio = p->patch_ratio; q.max_angle = p->max_angle;
  q.translation_overflow = p->translation_overflow;
  return launch<sample_homographies_kernel>(dim3(cdiv(b, 64)), dim3(64), 0, (hipStream_t)stream, seed, q, h_dev, inv_h_dev, b);
}

static int warp_labels_full_impl(const float* labels_dev, const float* h_dev, const float* hpx_dev, float* labels_out_dev,
                                 float* res_out_dev, float* bi_out_dev, int b, int hh, int w, hipStream_t st) {
  if (!labels_dev || b < 1 || hh < 1 || w < 1) return fail(-1, "warp_labels_full: bad argument");
  if ((long)hh * w >= (1L << 29)) return fail(-1, "warp_labels_full: h * w < 2^29 required (29-bit source index in the scatter key)");
  const long n = (long)b * hh * w;
  if (labels_out_dev) HIPCHK(hipMemsetAsync(labels_out_dev, 0, n * sizeof(float), st));
  if (res_out_dev) HIPCHK(hipMemsetAsync(res_out_dev, 0, 2 * n * sizeof(float), st));
  if (bi_out_dev) HIPCHK(hipMemsetAsync(bi_out_dev, 0, n * sizeof(float), st));
  hipLaunchKernelGGL(warp_labels_full_claim_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, labels_dev, h_dev, hpx_dev, labels_out_dev,
                     res_out_dev, bi_out_dev, b, hh, w);
  HIPCHK(hipGetLastError());
  if (res_out_dev || bi_out_dev) {  // the priority keys pass 1 left in the maps become the winners' values
    hipLaunchKernelGGL(warp_labels_full_resolve_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, h_dev, hpx_dev, res_out_dev,
                       bi_out_dev, b, hh, w);
    HIPCHK(hipGetLastError());
  }
  return 0;
}
int ssp_op_warp_labels_full(const float* labels_dev, const float* h_dev, float* labels_out_dev, float* res_out_dev,
                            float* bi_out_dev, int b, int hh, int w, void* stream) {
  return warp_labels_full_impl(labels_dev, h_dev, nullptr, labels_out_dev, res_out_dev, bi_out_dev, b, hh, w, (hipStream_t)stream);
}
int ssp_op_warp_labels_full_px(const float* labels_dev, const float* hpx_dev, float* labels_out_dev, float* res_out_dev,
                               float* bi_out_dev, int b, int hh, int w, void* stream) {
  if (!hpx_dev) return fail(-1, "warp_labels_full_px: pixel-space homographies required");
  return warp_labels_full_impl(labels_dev, nullptr, hpx_dev, labels_out_dev, res_out_dev, bi_out_dev, b, hh, w, (hipStream_t)stream);
}

int ssp_op_label_quantize(const float* in_dev, float* out_dev, size_t n, void* stream) {
  if (!in_dev || !out_dev) return fail(-1, "label_quantize: null pointer");
  return launch<label_quantize_u8_kernel>(dim3(cdiv((long)n, 256)), dim3(256), 0, (hipStream_t)stream, in_dev, out_dev, (long)n);
}

// ---- photometric augmentation (photo_kernels.hip.h) ----
static_assert(SSP_PHOTO_DRAW_STRIDE == PHOTO_DRAW_STRIDE && SSP_PHOTO_ELLIPSES == PHOTO_ELLIPSES && SSP_PHOTO_TRANSPARENCY == PHOTO_TRANSPARENCY &&
                  SSP_PHOTO_KSIZE == PHOTO_KSIZE && SSP_PHOTO_KEY == PHOTO_KEY && SSP_PHOTO_BLUR_W == PHOTO_BLUR_W &&
                  SSP_PHOTO_MAX_ELLIPSES == PHOTO_MAX_ELLIPSES && SSP_PHOTO_MAX_KSIZE == PHOTO_MAX_KSIZE,
              "the draw row of ssp_hip.h and photo_kernels.hip.h differ");
int ssp_op_photometric_draw(uint64_t seed, const ssp_photometric_params* p, int b, int hh, int w, float* draws_dev, void* stream) {
  if (!p || !draws_dev || b < 1 || hh < 1 || w < 1) return fail(-1, "photometric_draw: bad argument");
  if (p->struct_size != sizeof(ssp_photometric_params))
    return fail(-1, "photometric_draw: ssp_photometric_params.struct_size is %u, this library knows %zu", p->struct_size,
                sizeof(ssp_photometric_params));
  const int32_t counts[6] = {p->random_brightness, p->random_contrast, p->additive_gaussian_noise, p->additive_speckle_noise,
                             p->motion_blur, p->additive_shade};
  for (int i = 0; i < 6; ++i)
    if (counts[i] < 0 || counts[i] > 1)
      return fail(-1, "photometric_draw: enable count %d of primitive %d: a primitive applied twice (motion_blur.max_kernel_size != 3) "
                      "is not on the device path", counts[i], i);
  if (p->random_brightness && (p->brightness_max_abs_change < 0 || p->brightness_max_abs_change > 255))
    return fail(-1, "photometric_draw: max_abs_change must be in 0..255");
  if (p->additive_shade && (p->shade_nb_ellipses < 0 || p->shade_nb_ellipses > SSP_PHOTO_MAX_ELLIPSES || p->shade_kernel_lo < 1 ||
                            p->shade_kernel_hi <= p->shade_kernel_lo || p->shade_kernel_hi > SSP_PHOTO_MAX_KSIZE))
    return fail(-1, "photometric_draw: additive_shade needs nb_ellipses <= %d and 1 <= kernel_size_range[0] < kernel_size_range[1] <= %d",
                SSP_PHOTO_MAX_ELLIPSES, SSP_PHOTO_MAX_KSIZE);
  PhotoParams q;
  q.brightness = p->random_brightness; q.contrast = p->random_contrast; q.noise = p->additive_gaussian_noise;
  q.impulse = p->additive_speckle_noise; q.motion_blur = p->motion_blur; q.shade = p->additive_shade;
  q.max_abs_change = p->brightness_max_abs_change; q.nb_ellipses = p->shade_nb_ellipses;
  q.ksize_lo = p->shade_kernel_lo; q.ksize_hi = p->shade_kernel_hi;
  q.contrast_lo = p->contrast_lo; q.contrast_hi = p->contrast_hi; q.std_lo = p->noise_std_lo; q.std_hi = p->noise_std_hi;
  q.p_lo = p->impulse_prob_lo; q.p_hi = p->impulse_prob_hi; q.t_lo = p->shade_transparency_lo; q.t_hi = p->shade_transparency_hi;
  return launch<photo_draw_kernel>(dim3(cdiv(b, 64)), dim3(64), 0, (hipStream_t)stream, seed, q, b, hh, w, draws_dev);
}

int ssp_op_photometric_apply(const float* img_dev, const float* draws_dev, float* out_dev, int b, int hh, int w, void* stream) {
  if (!img_dev || !draws_dev || !out_dev || b < 1 || hh < 1 || w < 1) return fail(-1, "photometric_apply: bad argument");
  if (img_dev == out_dev) return fail(-1, "photometric_apply: out may not alias img (the 3x3 blur reads neighbours)");
  if (b > 65535 || (long)hh * w > (1l << 30)) return fail(-1, "photometric_apply: b <= 65535 and h * w <= 2^30 required");
  const int tx = photo_shade_lds_bytes(hh, 32) <= 65536 ? 32 : 16;
  const size_t lds = photo_shade_lds_bytes(hh, tx);
  if (lds > 65536) return fail(-1, "photometric_apply: h = %d needs %zu bytes of LDS for the shade strip (64 KiB per workgroup)", hh, lds);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(photo_pixel_kernel, dim3(cdiv(hh * w, 256), b), dim3(256), 0, st, img_dev, draws_dev, out_dev, hh, w);
  if (tx == 32) return launch_lds<photo_shade_kernel<32>>(65536, dim3(cdiv(w, 32), b), dim3(256), lds, st, out_dev, draws_dev, hh, w);
  return launch_lds<photo_shade_kernel<16>>(65536, dim3(cdiv(w, 16), b), dim3(256), lds, st, out_dev, draws_dev, hh, w);
}

// ---- Synthetic Shapes (shapes_kernels.hip.h) ----
static_assert(SSP_SHAPES_ROW == SH_ROW && SSP_SHAPES_CMDS == SH_CMDS && SSP_SHAPES_VERTS == SH_VERTS && SSP_SHAPES_TEX == SH_TEX &&
                  SSP_SHAPES_POINTS == SH_POINTS && SSP_SHAPES_BLOBS == SH_BLOBS && SSP_SHAPES_MAX_BLOBS == SH_MAX_BLOBS &&
                  SSP_SHAPES_MAX_CMDS == SH_MAX_CMDS && SSP_SHAPES_MAX_VERTS == SH_MAX_VERTS && SSP_SHAPES_MAX_TEX == SH_MAX_TEX &&
                  SSP_SHAPES_MAX_POINTS == SH_MAX_POINTS && SSP_SHAPES_MAX_BLUR == SH_MAX_BLUR && SSP_SHAPES_MAX_TEX_BLOBS == SH_MAX_TEX_BLOBS,
              "the scene table of ssp_hip.h and shapes_kernels.hip.h differ");
static int shapes_check(const ssp_shapes_params* p, int b, const char* who) {
  if (!p || b < 1 || b > 65535) return fail(-1, "%s: bad argument", who);
  if (p->struct_size != sizeof(ssp_shapes_params))
    return fail(-1, "%s: ssp_shapes_params.struct_size is %u, this library knows %zu", who, p->struct_size, sizeof(ssp_shapes_params));
  if (p->gen_h < 16 || p->gen_w < 16 || p->gen_h > 8192 || p->gen_w > 8192 || p->out_h < 1 || p->out_w < 1 || p->out_h > 8192 || p->out_w > 8192)
    return fail(-1, "%s: image_size 16..8192 and resize 1..8192 required", who);
  if (p->blur_size < 0 || p->blur_size > SSP_SHAPES_MAX_BLUR || (p->blur_size > 1 && !(p->blur_size & 1)))
    return fail(-1, "%s: blur_size must be odd and <= %d", who, SSP_SHAPES_MAX_BLUR);
  float tot = 0.f;
  for (int i = 0; i < 9; ++i) {
    if (!(p->weights[i] >= 0.f)) return fail(-1, "%s: negative primitive weight", who);
    tot += p->weights[i];
  }
  if (!(tot > 0.f)) return fail(-1, "%s: no primitive has a positive weight", who);
  const int dim = p->gen_h > p->gen_w ? p->gen_h : p->gen_w;
  if (p->bg_nb_blobs < 0 || p->bg_nb_blobs > SSP_SHAPES_MAX_BLOBS || p->bg_min_kernel < 1 || p->bg_max_kernel <= p->bg_min_kernel ||
      p->bg_max_kernel > 1024 || !(p->bg_min_rad_ratio >= 0.f) || (int)(dim * (double)p->bg_max_rad_ratio) > 181)
    return fail(-1, "%s: generate_background needs nb_blobs <= %d, 1 <= min_kernel_size < max_kernel_size <= 1024, blob radius <= 181", who,
                SSP_SHAPES_MAX_BLOBS);
  if (p->lines_nb_lines < 2 || p->lines_nb_lines > 33 || p->polygon_max_sides < 4 || p->polygon_max_sides > 17 || p->multi_max_sides < 4 ||
      p->multi_max_sides > 9 || p->multi_nb_polygons < 0 || p->multi_nb_polygons > SSP_SHAPES_MAX_TEX || p->multi_nb_blobs < 0 ||
      p->multi_nb_blobs > SSP_SHAPES_MAX_TEX_BLOBS || p->multi_kernel_lo < 1 || p->multi_kernel_hi <= p->multi_kernel_lo ||
      p->multi_kernel_hi > 1024 || p->ellipses_nb < 0 || p->ellipses_nb > SSP_SHAPES_MAX_CMDS || p->star_nb_branches < 4 ||
      p->star_nb_branches > 17 || p->checker_max_rows < 4 || p->checker_max_rows > 7 || p->checker_max_cols < 4 || p->checker_max_cols > 7 ||
      p->stripes_max_nb_cols < 6 || p->stripes_max_nb_cols > 15)
    return fail(-1, "%s: a primitive's count parameter is outside the scene table's capacity (include/ssp_hip.h)", who);
  return 0;
}
struct ShapesWs {
  unsigned* sums;        // [b][gen_h][gen_w] window sums
  unsigned char* plane;  // [b][gen_h][gen_w] the full-resolution plane, right behind the sums
  size_t bytes;
};
static ShapesWs shapes_carve(const ssp_shapes_params* p, int b, void* base) {
  const size_t px = (size_t)b * p->gen_h * p->gen_w;
  ShapesWs w;
  w.sums = static_cast<unsigned*>(base);
  w.plane = base ? static_cast<unsigned char*>(base) + px * 4 : nullptr;
  w.bytes = px * 4 + align_up(px, 256);
  return w;
}
size_t ssp_shapes_workspace_bytes(const ssp_shapes_params* p, int b) {
  if (!p || b < 1) return 0;
  return shapes_carve(p, b, nullptr).bytes;
}
int ssp_op_shapes_draw(uint64_t seed, const ssp_shapes_params* p, int b, int32_t* table_dev, void* stream) {
  if (int rc = shapes_check(p, b, "shapes_draw")) return rc;
  if (!table_dev) return fail(-1, "shapes_draw: null table");
  return launch<shapes_draw_kernel>(dim3(b), dim3(256), 0, (hipStream_t)stream, seed, *p, b, table_dev);
}
int ssp_op_shapes_render(const int32_t* table_dev, const ssp_shapes_params* p, int b, void* workspace_dev, uint8_t* image_dev,
                         float* points_dev, int32_t* counts_dev, void* stream) {
  if (int rc = shapes_check(p, b, "shapes_render")) return rc;
  if (!table_dev || !workspace_dev || !image_dev || !points_dev || !counts_dev) return fail(-1, "shapes_render: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int H = p->gen_h, W = p->gen_w;
  const int kmax = p->bg_max_kernel > p->multi_kernel_hi ? p->bg_max_kernel : p->multi_kernel_hi;
  const int pre_cap = (W + kmax + 3) & ~3;
  const int cap_bg = SSP_SHAPES_MAX_BLOBS, cap_tex = p->multi_nb_blobs > 0 ? p->multi_nb_blobs : 1;
  const size_t lds_bg = (size_t)4 * pre_cap + (size_t)8 * cap_bg, lds_tex = (size_t)4 * pre_cap + (size_t)8 * cap_tex;
  if (lds_tex > 60 * 1024 || lds_bg > 60 * 1024) return fail(-1, "shapes_render: image width %d with kernel %d needs %zu bytes of LDS", W, kmax, lds_tex);
  const ShapesWs ws = shapes_carve(p, b, workspace_dev);
  // every image has a background; an image of draw_multiple_polygons has up to multi_nb_polygons textures (its workgroups leave at once otherwise)
  for (int layer = -1; layer < p->multi_nb_polygons; ++layer) {
    if (layer >= 0 && !(p->weights[2] > 0.f)) break;
    CHK(launch_lds<shapes_layer_rows_kernel>(60 * 1024, dim3(H, b), dim3(256), layer < 0 ? lds_bg : lds_tex, st, table_dev, layer, H, W,
                                             p->multi_nb_blobs, layer < 0 ? cap_bg : cap_tex, pre_cap, ws.sums));
    hipLaunchKernelGGL(shapes_layer_cols_kernel, dim3(cdiv(W, 256), cdiv(H, 32), b), dim3(256), 0, st, table_dev, layer, H, W, pre_cap, ws.sums, ws.plane);
  }
  hipLaunchKernelGGL(shapes_paint_kernel, dim3(cdiv(W, 64), cdiv(H, 16), b), dim3(256), 0, st, table_dev, H, W, ws.plane);
  hipLaunchKernelGGL(shapes_blur_resize_kernel, dim3(cdiv(p->out_w, 64), cdiv(p->out_h, 4), b), dim3(256), 0, st, ws.plane, *p, image_dev);
  hipLaunchKernelGGL(shapes_points_kernel, dim3(cdiv(b * SSP_SHAPES_MAX_POINTS, 256)), dim3(256), 0, st, table_dev, *p, b, points_dev, counts_dev);
  HIPCHK(hipGetLastError());
  return 0;
}
int ssp_op_warp_points_scatter(const float* points_dev, const int32_t* counts_dev, const float* hpx_dev, float* labels_dev, int b,
                               int stride, int hh, int w, void* stream) {
  if (!points_dev || !counts_dev || !labels_dev || b < 1 || stride < 1 || hh < 1 || w < 1) return fail(-1, "warp_points_scatter: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(labels_dev, 0, (size_t)b * hh * w * sizeof(float), st));
  return launch<warp_points_scatter_kernel>(dim3(cdiv(b * stride, 256)), dim3(256), 0, st, points_dev, counts_dev, hpx_dev,
                                            labels_dev, b, stride, hh, w);
}

int ssp_op_sem_finalize(const float* sem_warped_dev, const float* valid_dev, int64_t* out_dev, size_t n, int n_classes,
                        void* stream) {
  return launch<sem_finalize_kernel>(dim3(cdiv((long)n, 256)), dim3(256), 0, (hipStream_t)stream, sem_warped_dev, valid_dev,
                                     out_dev, (long)n, n_classes);
}

// BatchNorm(+ReLU(+2x2 max-pool)) backward as an operator: y [N,H,W,C] raw conv output, dout = gradient wrt the
// activated (pooled when pool=1: [N,H/2,W/2,C]) output; stats4 = {scale, shift, mean, invstd} each [C].
// Outputs: dy [N,H,W,C], dgamma/dbeta/dbias [C] (accumulated), sums_dev: double[2C] scratch.
int ssp_op_bn_bwd(const float* y_dev, const float* dout_dev, const float* gamma_dev, const float* stats4_dev,
                  float* dy_dev, float* dgamma_dev, float* dbeta_dev, float* dbias_dev, double* sums_dev, int n, int hh,
                  int w, int c, int relu, int pool, void* stream) {
  return ssp_op_bn_bwd_strided(y_dev, dout_dev, gamma_dev, stats4_dev, dy_dev, dgamma_dev, dbeta_dev, dbias_dev, sums_dev, n,
                               hh, w, c, c, relu, pool, stream);
}

// one body for both tensor types (T = float, or uint16_t for bf16 tensors); `what` is the exported name in the messages
extern "C++" template <typename T>
static int bn_bwd_op(const char* what, const void* y_dev, const void* dout_dev, const float* gamma_dev, const float* stats4_dev,
                     void* dy_dev, float* dgamma_dev, float* dbeta_dev, float* dbias_dev, double* sums_dev, int n, int hh, int w, int c,
                     int cs, int relu, int pool, hipStream_t st) {
  constexpr bool bf16 = !std::is_same<T, float>::value;
  if (cs < c || (cs & 3)) return fail(-1, "%s: the channel stride must be a multiple of 4 and >= C", what);
  if (bf16 && !relu) return fail(-3, "%s: only the ReLU layers run on bf16 tensors", what);
  HIPCHK(hipMemsetAsync(sums_dev, 0, 2 * (size_t)c * NREP * sizeof(double), st));
  BnBwdArgs a;
  a.y = reinterpret_cast<const float*>(y_dev); a.dout = reinterpret_cast<const float*>(dout_dev); a.dy = reinterpret_cast<float*>(dy_dev);
  a.scale = stats4_dev; a.shift = stats4_dev + c; a.mean = stats4_dev + 2 * c;
  a.invstd = stats4_dev + 3 * c; a.gamma = gamma_dev; a.sums = sums_dev; a.dbias = dbias_dev; a.N = n; a.H = hh; a.W = w;
  a.C = c; a.y_cs = cs; a.y_co = 0; a.d_cs = cs; a.d_co = 0; a.dy_cs = cs; a.dy_co = 0; a.count = (double)n * hh * w;
  DevTemps tmp(st);
  float* k12 = nullptr;
  CHK(tmp.take(&k12, 2 * (size_t)c));
  a.k12 = k12; a.x = nullptr; a.apool = nullptr; a.beta = nullptr; a.pool_fix = 0;
  if (relu && pool) CHK((launch_bn_bwd<true, true, T>(&a, 1, dgamma_dev, dbeta_dev, st)));
  else if (relu) CHK((launch_bn_bwd<true, false, T>(&a, 1, dgamma_dev, dbeta_dev, st)));
  else if constexpr (!bf16) CHK((launch_bn_bwd<false, false>(&a, 1, dgamma_dev, dbeta_dev, st)));
  return tmp.release();
}

int ssp_op_bn_bwd_strided(const float* y_dev, const float* dout_dev, const float* gamma_dev, const float* stats4_dev,
                          float* dy_dev, float* dgamma_dev, float* dbeta_dev, float* dbias_dev, double* sums_dev, int n,
                          int hh, int w, int c, int cs, int relu, int pool, void* stream) {
  return bn_bwd_op<float>("ssp_op_bn_bwd_strided", y_dev, dout_dev, gamma_dev, stats4_dev, dy_dev, dgamma_dev, dbeta_dev, dbias_dev,
                          sums_dev, n, hh, w, c, cs, relu, pool, (hipStream_t)stream);
}

// the same operator on bf16 tensors (the bf16 path: y, dout, dy are bf16 NHWC with channel stride cs; fp32 arithmetic and parameters)
int ssp_op_bn_bwd_bf16(const void* y_dev, const void* dout_dev, const float* gamma_dev, const float* stats4_dev, void* dy_dev,
                       float* dgamma_dev, float* dbeta_dev, float* dbias_dev, double* sums_dev, int n, int hh, int w, int c, int cs,
                       int relu, int pool, void* stream) {
  return bn_bwd_op<uint16_t>("ssp_op_bn_bwd_bf16", y_dev, dout_dev, gamma_dev, stats4_dev, dy_dev, dgamma_dev, dbeta_dev, dbias_dev,
                             sums_dev, n, hh, w, c, cs, relu, pool, (hipStream_t)stream);
}

int ssp_op_dense_loss(const float* desc_a_nhwc_dev, const float* desc_b_nhwc_dev, const float* homographies_dev,
                      const float* valid_dev, int b, int hc, int wc, float lamda_d, float descriptor_dist, int multi_task,
                      float scale, void* scratch_dev, size_t scratch_bytes, float* out3_dev, float* dda_dev,
                      float* ddb_dev, void* stream) {
  const int pc = hc * wc;
  const bool grad = dda_dev != nullptr && ddb_dev != nullptr;
  const size_t need = align_up(sizeof(StepAccum), 256) + (grad ? (size_t)b * pc * pc * sizeof(float) : 0);
  if (scratch_bytes < need) return fail(-4, "ssp_op_dense_loss scratch too small (%zu < %zu)", scratch_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  StepAccum* acc = reinterpret_cast<StepAccum*>(scratch_dev);
  float* coef = grad ? reinterpret_cast<float*>(reinterpret_cast<char*>(scratch_dev) + align_up(sizeof(StepAccum), 256)) : nullptr;
  hipLaunchKernelGGL(dense_op_prep_kernel, dim3(1), dim3(256), 0, st, acc, valid_dev, b * pc, scale);
  DenseArgs da;
  da.da = desc_a_nhwc_dev; da.db = desc_b_nhwc_dev; da.hn = homographies_dev; da.valid = valid_dev; da.coef = coef;
  da.acc = acc; da.B = b; da.Hc = hc; da.Wc = wc; da.lamda_d = lamda_d; da.dist = descriptor_dist; da.multi_task = multi_task;
  hipLaunchKernelGGL(dense_dots_kernel, dim3(cdiv(pc, 64), cdiv(pc, 64), b), dim3(256), 0, st, da);
  if (grad) {
    hipLaunchKernelGGL((dense_grad_kernel<false>), dim3(4, cdiv(pc, 64), b), dim3(256), 0, st, coef, desc_b_nhwc_dev, dda_dev, pc);
    hipLaunchKernelGGL((dense_grad_kernel<true>), dim3(4, cdiv(pc, 64), b), dim3(256), 0, st, coef, desc_a_nhwc_dev, ddb_dev, pc);
  }
  hipLaunchKernelGGL(dense_op_finish_kernel, dim3(1), dim3(1), 0, st, acc, out3_dev, b, pc);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_sparse_loss(const float* desc_a_nhwc_dev, const float* desc_b_nhwc_dev, const int32_t* match_a_dev,
                       const int32_t* match_b_dev, const int32_t* nonmatch_b_dev, int b, int hc, int wc, int n_match,
                       int n_non, int method, int dist, float coef_pos, float coef_neg, float* dd_a_nhwc_dev, float* dd_b_nhwc_dev,
                       float* out2_dev, void* stream) {
  return ssp_op_sparse_loss_path(desc_a_nhwc_dev, desc_b_nhwc_dev, match_a_dev, match_b_dev, nonmatch_b_dev, b, hc, wc, n_match, n_non, method,
                                 dist, coef_pos, coef_neg, dd_a_nhwc_dev, dd_b_nhwc_dev, out2_dev, -1, nullptr, nullptr, nullptr, stream);
}

int ssp_op_sparse_loss_path(const float* desc_a_nhwc_dev, const float* desc_b_nhwc_dev, const int32_t* match_a_dev,
                            const int32_t* match_b_dev, const int32_t* nonmatch_b_dev, int b, int hc, int wc, int n_match,
                            int n_non, int method, int dist, float coef_pos, float coef_neg, float* dd_a_nhwc_dev, float* dd_b_nhwc_dev,
                            float* out2_dev, int gather, int32_t* csr_off_dev, int32_t* csr_match_dev, float* csr_weight_dev,
                            void* stream) {
  if (b < 1 || b > SSP_MAX_PAIRS) return fail(-1, "batch out of range (1..%d)", SSP_MAX_PAIRS);
  if ((dd_a_nhwc_dev == nullptr) != (dd_b_nhwc_dev == nullptr)) return fail(-1, "sparse_loss: both gradient pointers or none");
  const bool grad = dd_a_nhwc_dev != nullptr;
  const bool use_gather = grad && (gather < 0 ? desc_gather_env() : gather != 0);
  const bool own_csr = csr_off_dev == nullptr || csr_match_dev == nullptr || csr_weight_dev == nullptr;
  if (!own_csr && !use_gather) return fail(-1, "sparse_loss: the corner lists exist on the gather path with gradients only");
  hipStream_t st = (hipStream_t)stream;
  const int dflags = (method != 0 ? DESC_METHOD_1D : 0) | (dist != 0 ? DESC_EUCLIDEAN : 0);
  const size_t ncell_floats = (size_t)b * hc * wc * 256;
  DevTemps tmp(st);
  StepAccum* acc = nullptr;
  float *dots = nullptr, *g_rows = nullptr, *csr_weight = csr_weight_dev;
  int32_t *csr_off = csr_off_dev, *csr_match = csr_match_dev;
  CHK(tmp.take(&acc, 1));
  HIPCHK(hipMemsetAsync(acc, 0, sizeof(StepAccum), st));
  hipLaunchKernelGGL(sparse_op_prep_kernel, dim3(1), dim3(1), 0, st, acc, coef_pos, coef_neg);
  if (grad) {
    CHK(tmp.take(&dots, (size_t)b * n_match * n_non));
    CHK(dev_zero(dd_a_nhwc_dev, ncell_floats * sizeof(float), st));
    CHK(dev_zero(dd_b_nhwc_dev, ncell_floats * sizeof(float), st));
  }
  if (use_gather) {
    if (own_csr) {
      CHK(tmp.take(&csr_off, (size_t)b * 2 * ((size_t)hc * wc + 1)));
      CHK(tmp.take(&csr_match, (size_t)b * 2 * 4 * n_match));
      CHK(tmp.take(&csr_weight, (size_t)b * 2 * 4 * n_match));
    }
    CHK(tmp.take(&g_rows, (size_t)b * n_match * 2 * 256));
    CHK(launch_desc_csr(match_a_dev, match_b_dev, csr_off, csr_match, csr_weight, b, hc, wc, n_match, dflags, st));
  }
  const DescLaunch D(dflags, b, n_match, st);
  float* const none = nullptr;
  if (use_gather)
    D.match<true, true>(desc_a_nhwc_dev, desc_b_nhwc_dev, match_a_dev, match_b_dev, none, none, acc, b, hc, wc, n_match, dflags, g_rows);
  else if (grad)
    D.match<true>(desc_a_nhwc_dev, desc_b_nhwc_dev, match_a_dev, match_b_dev, dd_a_nhwc_dev, dd_b_nhwc_dev, acc, b, hc, wc, n_match, dflags);
  else
    D.match<false>(desc_a_nhwc_dev, desc_b_nhwc_dev, match_a_dev, match_b_dev, none, none, acc, b, hc, wc, n_match, dflags);
  D.nonmatch_fwd(desc_a_nhwc_dev, desc_b_nhwc_dev, match_a_dev, nonmatch_b_dev, dots, acc, b, hc, wc, n_match, n_non, dflags);
  if (grad)
    D.nonmatch_bwd(desc_a_nhwc_dev, desc_b_nhwc_dev, match_a_dev, nonmatch_b_dev, dots, dd_a_nhwc_dev, dd_b_nhwc_dev, acc, b, hc, wc, n_match,
                   n_non, dflags);
  if (use_gather) {   // behind the non-match atomics, as in the pair step (there inside desc_normalize_bwd_kernel)
    const DescGather dg = {csr_off, csr_match, csr_weight, g_rows, hc * wc, n_match};
    hipLaunchKernelGGL(desc_gather_kernel, dim3(cdiv((long)b * hc * wc, 4), 2), dim3(256), 0, st, dd_a_nhwc_dev, dd_b_nhwc_dev, b * hc * wc, dg);
  }
  hipLaunchKernelGGL(sparse_loss_means_kernel, dim3(1), dim3(1), 0, st, acc, out2_dev, b, n_match);
  HIPCHK(hipGetLastError());
  return tmp.release();
}

int ssp_op_detector_loss(const float* semi_nhwc_dev, int cs, const float* labels2d_dev, const float* mask2d_dev, int b, int hh,
                         int w, void* scratch_dev, size_t scratch_bytes, float* loss_dev, float* dsemi_nhwc_dev, void* stream) {
  if (hh % 8 || w % 8 || cs < 65) return fail(-1, "detector_loss: H, W multiples of 8 and channel stride >= 65 required");
  const int ncells = b * (hh / 8) * (w / 8);
  const size_t need = align_up(sizeof(StepAccum), 256) + (size_t)(ncells + 65 * 2) * sizeof(float);
  if (scratch_bytes < need) return fail(-4, "ssp_op_detector_loss scratch too small (%zu < %zu)", scratch_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  StepAccum* acc = reinterpret_cast<StepAccum*>(scratch_dev);
  float* cellmask = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch_dev) + align_up(sizeof(StepAccum), 256));
  float* ones = cellmask + ncells;  // identity BatchNorm affine: scale 1 | shift 0
  hipLaunchKernelGGL(detector_op_prep_kernel, dim3(1), dim3(64), 0, st, acc);
  hipLaunchKernelGGL(fill_affine_identity_kernel, dim3(1), dim3(128), 0, st, ones, 65);
  hipLaunchKernelGGL(cell_mask_kernel, dim3(std::min(cdiv(ncells, 4), 512)), dim3(256), 0, st, mask2d_dev, cellmask,
                     &acc->mask_cnt[0], b, hh, w);
  hipLaunchKernelGGL(detector_loss_kernel, dim3(std::min(cdiv(ncells, 4), 1024)), dim3(256), 0, st, semi_nhwc_dev, ones,
                     ones + 65, labels2d_dev, cellmask, dsemi_nhwc_dev, acc, 0, b, hh, w, cs);
  hipLaunchKernelGGL(detector_op_finish_kernel, dim3(1), dim3(64), 0, st, acc, loss_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_sem_loss(const float* sout_nhwc_dev, int cs, const int64_t* labels_dev, int b, int hh, int w, int n_classes, int algo,
                    void* scratch_dev, size_t scratch_bytes, float* loss_dev, float* dsout_nhwc_dev, void* stream) {
  if (hh % 8 || w % 8 || cs < n_classes || n_classes < 1) return fail(-1, "sem_loss: H, W multiples of 8 and channel stride >= n_classes required");
  if (algo < 0 || algo > 2) return fail(-1, "sem_loss: algo 0 (the step's choice), 1 or 2");
  if (scratch_bytes < sizeof(StepAccum)) return fail(-4, "ssp_op_sem_loss scratch too small (%zu < %zu)", scratch_bytes, sizeof(StepAccum));
  hipStream_t st = (hipStream_t)stream;
  StepAccum* acc = reinterpret_cast<StepAccum*>(scratch_dev);
  const int hc = hh / 8, wc = w / 8;
  hipLaunchKernelGGL(sem_op_prep_kernel, dim3(1), dim3(64), 0, st, acc);
  hipLaunchKernelGGL(sem_count_kernel, dim3(512, 1), dim3(256), 0, st, labels_dev, labels_dev, (long)b * hh * w, n_classes, acc);
  if (dsout_nhwc_dev != nullptr) CHK(dev_zero(dsout_nhwc_dev, (size_t)b * hc * wc * cs * sizeof(float), st));
  CHK(launch_sem_ce(algo, dsout_nhwc_dev != nullptr, sout_nhwc_dev, labels_dev, dsout_nhwc_dev, acc, 0, b, hc, wc, hh, w, n_classes, cs, st));
  hipLaunchKernelGGL(sem_op_finish_kernel, dim3(1), dim3(64), 0, st, acc, loss_dev);
  HIPCHK(hipGetLastError());
  return 0;
}

int ssp_op_sem_predict(const float* sout_nhwc_dev, int cs, const int64_t* labels_dev, int b, int hh, int w, int n_classes,
                       uint8_t* pred_dev, int64_t* confusion_dev, void* stream) {
  if (!sout_nhwc_dev || b < 1 || hh < 8 || w < 8) return fail(-1, "sem_predict: bad argument");
  if (hh % 8 || w % 8) return fail(-1, "sem_predict: H and W must be multiples of 8 (got %dx%d)", hh, w);
  if (n_classes < 1 || n_classes > SEMP_MAX_C || cs < n_classes)
    return fail(-1, "sem_predict: 1 <= n_classes <= %d and channel stride >= n_classes required (got %d, stride %d)", SEMP_MAX_C, n_classes, cs);
  if (!pred_dev && !confusion_dev) return fail(-1, "sem_predict: neither a class map nor a confusion matrix requested");
  if (confusion_dev && !labels_dev) return fail(-1, "sem_predict: a confusion matrix needs labels");
  const int hc = hh / 8, wc = w / 8;
  const long ntile = (long)b * (hc + 1) * (wc + 1);
  if (ntile > (1L << 30) || (size_t)b * hc * wc * cs > ((size_t)1 << 40)) return fail(-1, "sem_predict: shape too large");
  const int tpw = std::max(SEMP_MIN_TILES, cdiv((int)ntile, SEMP_WAVES));
  const dim3 grid(cdiv(cdiv((int)ntile, tpw), 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* conf = reinterpret_cast<unsigned long long*>(confusion_dev);
  if (cs % 4 == 0 && (reinterpret_cast<size_t>(sout_nhwc_dev) & 15) == 0)
    return launch<sem_predict_kernel<true>>(grid, block, 0, st, sout_nhwc_dev, labels_dev, pred_dev, conf, b, hc, wc, n_classes, cs, tpw);
  return launch<sem_predict_kernel<false>>(grid, block, 0, st, sout_nhwc_dev, labels_dev, pred_dev, conf, b, hc, wc, n_classes, cs, tpw);
}

int ssp_sem_predict(ssp_handle* h, int slot, const int64_t* labels_dev, uint8_t* pred_dev, int64_t* confusion_dev, void* stream) {
  if (!h || !h->bound) return fail(-1, "handle not bound");
  if (h->nheads != 3) return fail(-1, "sem_predict: the model has no segmentation head");
  if (slot < 0 || slot > 1) return fail(-1, "sem_predict: slot must be 0 or 1");
  Slot& S = h->slot[slot];
  if (S.N <= 0) return fail(-1, "sem_predict: slot %d holds no forward", slot);
  return ssp_op_sem_predict(S.Y[L_SOUT], h->sout_cs, labels_dev, S.N, S.H, S.W, h->cfg.n_classes, pred_dev, confusion_dev, stream);
}

int ssp_op_labels(const float* labels2d_dev, const float* mask2d_dev, float* target_dev, float* cellmask_dev, int b,
                  int hh, int w, void* stream) {
  if (hh % 8 || w % 8) return fail(-1, "H and W must be multiples of 8");
  hipStream_t st = (hipStream_t)stream;
  const int ncells = b * (hh / 8) * (w / 8);
  if (labels2d_dev && target_dev)
    hipLaunchKernelGGL(labels2dto3d_kernel, dim3(cdiv(ncells, 4)), dim3(256), 0, st, labels2d_dev, target_dev, b, hh, w);
  DevTemps tmp(st);
  if (mask2d_dev && cellmask_dev) {
    double* cnt = nullptr;
    CHK(tmp.take(&cnt, 1));
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(double), st));
    hipLaunchKernelGGL(cell_mask_kernel, dim3(std::min(cdiv(ncells, 4), 512)), dim3(256), 0, st, mask2d_dev, cellmask_dev, cnt, b, hh, w);
  }
  HIPCHK(hipGetLastError());
  return tmp.release();
}
