"""Pair construction for real data on the device: the `warped_pair` branch of
datasets/Coco.py:341-392 / datasets/Coco_sem.py:395-455 for a BATCH that is already resident in HBM.

  homographies      utils/homographies.py:12-141 with `warped_pair.params`, inverted (Coco.py:342-350): device RNG
  warped_img        inv_warp_image_batch, bilinear (utils/utils.py:347-385)
  warped_labels, warped_res, warped_labels_bi   warpLabels(bilinear=True) (datasets/data_tools.py:37-63)
  warped_valid_mask compute_valid_mask (nearest warp of ones + elliptical erosion, utils/utils.py:715-742)
  warped_sem        bilinear warp of the class ids, invalid -> 133 (Coco_sem.py:406-448)

  *_gaussian        ImgAugTransform(GaussianBlur sigma 0.2) of labels_2D / warped_labels_bi (Coco.py:378,400, utils/photometric.py:
                    59-78): float -> uint8 -> blur -> float / 255.  The quantisation floor(x * 255) / 255 is reproduced
                    (`ssp_op_label_quantize`); the blur itself is the identity on 8-bit data (off-centre weights of the 5-tap
                    sigma-0.2 kernel: exp(-12.5) = 3.7e-6) - imgaug / cv2 are absent from the image, so that last statement is
                    restated from the kernel formula, not checked against the binaries.

  image, warped_img with `photometric=`: ImgAugTransform + customizedTransform (utils/photometric.py) as
                    `ssp_op_photometric_draw` / `ssp_op_photometric_apply` in the reference's data flow
                    (Coco.py:249, 355-361): image = photo(raw), warped_img = photo(warp(raw)) - the warp reads the RAW image
                    and the two views draw independently.

The RNG streams differ from numpy / scipy, so the homographies and the photometric draws are a distribution-level
equivalent (like synth.py's host generator)."""
import torch

from . import lib as L


def make_pairs(image, labels_2D, seed, warp_params=None, erosion_radius=3, semantic=None, n_classes=133, photometric=None,
               homographies=None, photometric_draws=None, inv_homographies=None):
    """image, labels_2D: device tensors [B,1,H,W] (keypoint map: non-zero = keypoint); semantic: integer [B,H,W] or None.
    image may be uint8 (scaled by 1/255 here), semantic uint8 / int16 / int64: widening on the device is cheap, the point is
    fewer bytes over PCIe.
    photometric: the `data.augmentation` dict; when its `photometric.enable` is set, both views are augmented with
        independent draws (seeds derived from `seed`).
    homographies: [B,3,3] (image -> warped, normalised coordinates) used instead of sampling; inv_homographies: their
        inverses if the caller has them (otherwise torch.inverse on the host like datasets/Coco.py:350, one small round trip).
    photometric_draws: a pair of draw tables [B, lib.PHOTO_DRAW_STRIDE] (image, warped_img) used instead of drawing.
    With the three at None the output is the same as without them, bit for bit.
    Returns the `sample` dict of Train_model_heatmap_all.py:212-251 (device tensors)."""
    if not image.is_cuda:
        raise RuntimeError("make_pairs needs HIP tensors: there is no CPU fallback")
    B, _, H, W = image.shape
    if image.dtype == torch.uint8:
        # k / 255 from a 256-entry table divided on the HOST: the device's division by a scalar multiplies by the reciprocal,
        # which is not the loader's correctly rounded float32 quotient in the last bit
        image = (torch.arange(256, dtype=torch.float32) / 255.0).to(image.device)[image.contiguous().long()]
    else:
        image = image.contiguous().float()
    labels_2D = labels_2D.contiguous().float()
    if semantic is not None and semantic.dtype != torch.int64:
        semantic = semantic.long()
    if homographies is None:
        hs, inv = L.op_sample_homographies(B, seed, image.device, **(warp_params or {}))
    else:
        hs = homographies.to(image.device, torch.float32).contiguous()
        inv = (torch.inverse(hs.cpu()) if inv_homographies is None else inv_homographies).to(image.device, torch.float32).contiguous()
    warped = L.op_warp_image(image, inv)
    raw = image
    if photometric_draws is None and photometric is not None and (photometric.get("photometric") or {}).get("enable", False):
        pp = L.photometric_params_from_config(photometric)
        photometric_draws = tuple(L.op_photometric_draw(B, H, W, (int(seed) * 2 + 1) * 0x9E3779B1 + v, pp, image.device) for v in (0, 1))
    if photometric_draws is not None:
        # both views in ONE call: 2 B images fill the device twice as well as B (one shade workgroup per image and 32 columns)
        both = L.op_photometric_apply(torch.cat((raw, warped)), torch.cat([d.to(image.device) for d in photometric_draws]).contiguous())
        image, warped = both[:B], both[B:]
    wl, wres, wbi = L.op_warp_labels_full(labels_2D, hs)
    vm = L.op_erode(L.op_warp_image(torch.ones_like(image), inv, nearest=True), erosion_radius)
    s = {"image": image, "warped_img": warped, "labels_2D": labels_2D, "warped_labels": wl, "warped_res": wres,
         "warped_labels_bi": wbi, "labels_2D_gaussian": L.op_label_quantize(labels_2D),
         "warped_labels_gaussian": L.op_label_quantize(wbi),
         "valid_mask": torch.ones_like(image), "warped_valid_mask": vm, "homographies": hs, "inv_homographies": inv,
         # cell-space matrices in the reference's op order: the device sampler's matches then round like the reference's
         "cell_homographies": L.scaled_homographies(hs, H // 8, W // 8).to(image.device)}
    if semantic is not None:
        sw = L.op_warp_image(semantic.float().view(B, 1, H, W).contiguous(), inv)
        s["semantic"] = semantic
        s["warped_sem"] = L.op_sem_finalize(sw.view(B, H, W), vm.view(B, H, W), n_classes)
    return s


def make_single_view(image, points, counts, seed, homographic=None, photometric=None, homographies=None, photometric_draws=None):
    """The single-view branch of the loaders (datasets/SyntheticDataset_gaussian.py:381-480, datasets/Coco.py:307-339) for a
    batch that is resident in HBM: the `sample` dict of the single-view step (`image`, `labels_2D`, `valid_mask`,
    `labels_2D_gaussian`), built in the reference's order:

      1 photometric augmentation of the UNWARPED image (:385-394)
      2 a homography from `augmentation.homographic.params`, inverted (:429-440)
      3 bilinear warp of the image (:442-446)
      4 the key points warped with the pixel-scaled homography (:450)
      5 filter_points, round, clamp to (W - 1, H - 1), scatter (:342-351, 451, 472)
      6 valid mask = nearest warp of ones, eroded by `valid_border_margin` (:463-470)

    image: [B,1,H,W] uint8 or float32; points: float32 [B,N,2] (x, y) at the image's resolution; counts: int32 [B].
    homographic: the `augmentation.homographic` dict (`params`, `valid_border_margin`) or None: labels are the rounded, clamped
        points, the mask is all ones and the image is only augmented photometrically.
    photometric: the `data.augmentation` dict (on when its `photometric.enable` is set) or None; a stage that the reference's
        parser doubles (motion_blur.max_kernel_size != 3) is applied once (lib.photometric_params_single_pass).
    Host work per batch: sampled homographies cost one small D2H copy, the reference's own fp32 `T^-1 H T` per matrix on the host
        (lib.scaled_homographies: bit-identical rounded indices) and one H2D copy - a synchronisation point, as in make_pairs;
        supplied homographies are also inverted on the host.  No image or label map ever leaves the device.
    homographies: [B,3,3] used instead of sampling (the matrix that warps the points; the image is warped with its inverse);
    photometric_draws: one draw table [B, lib.PHOTO_DRAW_STRIDE] used instead of drawing.
    `labels_res` is NOT produced: the heat-map trainer never reads it with `subpixel` off (Train_model_heatmap_all.py).
    `labels_2D_gaussian` is op_label_quantize(labels_2D) as in make_pairs.  The RNG streams differ from numpy's: a
    distribution-level equivalent."""
    if not image.is_cuda:
        raise RuntimeError("make_single_view needs HIP tensors: there is no CPU fallback")
    B, _, H, W = image.shape
    dev = image.device
    if image.dtype == torch.uint8:  # load_as_float: k / 255 from the host's correctly rounded table (see make_pairs)
        image = L.u8_to_unit_float(image)
    else:
        image = image.contiguous().float()
    points = points.contiguous().float()
    counts = counts.contiguous().to(torch.int32)
    if photometric_draws is None and photometric is not None and (photometric.get("photometric") or {}).get("enable", False):
        pp = L.photometric_params_single_pass(photometric)
        photometric_draws = L.op_photometric_draw(B, H, W, (int(seed) * 2 + 1) * 0x9E3779B1, pp, dev)
    if photometric_draws is not None:
        image = L.op_photometric_apply(image, photometric_draws.to(dev).contiguous())
    if homographic is None and homographies is None:
        labels = L.op_warp_points_scatter(points, counts, H, W)
        mask = torch.ones_like(image)
    else:
        if homographies is None:
            hs, inv = L.op_sample_homographies(B, int(seed) ^ 0x53564945, dev, **((homographic or {}).get("params") or {}))
        else:
            hs = homographies.to(dev, torch.float32).contiguous()
            inv = torch.inverse(hs.cpu()).to(dev).contiguous()
        image = L.op_warp_image(image, inv)
        labels = L.op_warp_points_scatter(points, counts, H, W, L.scaled_homographies(hs, H, W).to(dev))
        mask = L.op_erode(L.op_warp_image(torch.ones_like(image), inv, nearest=True), int((homographic or {}).get("valid_border_margin", 0)))
    return {"image": image, "labels_2D": labels, "valid_mask": mask, "labels_2D_gaussian": L.op_label_quantize(labels)}
