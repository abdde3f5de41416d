"""Inputs shared by tests/test_draws_ref_cpu.py and tests/test_gpu_draws_exact.py: the CPU file shows, from the restatement
alone, that the shares the GPU tests may leave out stay inside their caps for exactly these seeds and shapes."""
import functools
import math

import numpy as np

from oracle import cpu_ref as C
from tests import pairs_cases as K
from tests import pairs_ref as R

MARGIN_MIN, MARGIN_CAP = K.MARGIN_MIN, K.MARGIN_CAP
N_MATCH, N_NON = 1000, 100          # the Engine's defaults (sparse_loss.py: num_matching_attempts, num_masked_non_matches_per_match)
SAMPLER_B = 3                       # img << 40 matters from the second image on

# name -> (H, W, seed of the sampler call)
SAMPLER_CASES = {
    "64x96": (64, 96, 1234),                      # 96 cells: cap 2048, nv < n_match on every image, every fill index compared
    "240x320": (240, 320, 0x1234567890ABCDEF),    # 1200 cells: nv = ncell, nv just under n_match, nv = 0; a seed with high bits
    "480x640": (480, 640, 77),                    # 4800 cells: the 8192-key sort, dynamic LDS above 64 KB
}


def _mild(k=1.1, ang=0.05):
    """a magnification by k about the centre, turned by `ang`, with a light perspective: 1 / k^2 of the cells stay inside"""
    c, s = math.cos(ang), math.sin(ang)
    return np.array([[k * c, -k * s, 0.01], [k * s, k * c, -0.02], [0.02, 0.01, 1.0]])


@functools.lru_cache(maxsize=None)
def sampler_homographies(name):
    """float32 [SAMPLER_B, 3, 3]: `homographies` (image -> warped, normalised coordinates) of a sampler case."""
    if name == "240x320":
        far = np.array([[1.0, 0, 3.0], [0, 1.0, 0], [0, 0, 1.0]])     # three image widths to the right: every cell leaves
        hs = np.stack([np.eye(3), _mild(), far])
    else:
        seed = {"64x96": 41, "480x640": 43}[name]
        hs = R.sample_homographies(seed, SAMPLER_B, C.sample_homography, C.get_perspective_transform, **K.f32_params(K.WARP))[0]
    return np.ascontiguousarray(hs, np.float32)


# ------------------------------------------------------------------------------------------------ photometric draw and noise
PHOTO_B = 300                        # the draw runs 64 images per block: five blocks, the last one partly filled
PHOTO_SIZES = ((240, 320), (67, 93))
PHOTO_SEED = 20241018                # every decision margin of the 14 compared draws is above 2e-6 (tests/test_draws_ref_cpu.py)
NOISE_SIZES = ((67, 93), (24, 32))
NOISE_B = 6
# hand-made keys: all four 16-bit words above 32767; zero; and a key under which pixel 669 draws the Gaussian field 0, where
# u1 = (0 + 1) 2^-24 is the largest normal the stream can give (without the + 1: the logarithm of 0)
NOISE_KEYS_BY_HAND = (0x8001_9ABC_FFFF_C000, 0, 10048)
NOISE_EDGE_PIXEL = 5                 # case "impulse_edge": p is set to this pixel's own 24-bit field, so that u1 == p there


def photo_param_sets():
    """name -> parameter dict of photometric_ref.draw: the shipped block and each primitive off in turn"""
    from tests import photometric_ref as P
    sets = {"shipped": dict(P.SHIPPED)}
    for prim in P.PRIMITIVES:
        sets["no_" + prim] = dict(P.SHIPPED, **{prim: 0})
    return sets


@functools.lru_cache(maxsize=None)
def photo_rows(name, H, W):
    """(rows float32 [PHOTO_B, STRIDE], margins [PHOTO_B], [(angle, direction) or None]) of a parameter set"""
    from tests import photometric_ref as P
    out = [P.draw_full(PHOTO_SEED, n, photo_param_sets()[name], H, W) for n in range(PHOTO_B)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), [o[2] for o in out]


def noise_image(kind, H, W):
    """float32 [H, W]: the textured case image, or an image of 0 and 1 only (both clips occur under noise)"""
    from tests import photometric_ref as P
    if kind == "binary":
        return (np.random.RandomState(5).uniform(size=(H, W)) < 0.5).astype(np.float32)
    return P.case_image(H, W, seed=3)


@functools.lru_cache(maxsize=None)
def noise_cases(H, W):
    """name -> (image float32 [H, W], rows float32 [NOISE_B, STRIDE]); three keys come from draw(), three are hand-made"""
    from tests import photometric_ref as P
    keys = [P.row_key(P.draw(PHOTO_SEED, n, P.SHIPPED, H, W)[0]) for n in range(NOISE_B - len(NOISE_KEYS_BY_HAND))]
    keys += list(NOISE_KEYS_BY_HAND)
    col = P.motion_blur_weights(0.0, 0.0)            # a column of thirds: the blur itself has no ties (photometric_ref.exact_cases)
    kinds = {
        "sigma": ("texture", dict(sigma=10.0)),
        "impulse": ("texture", dict(impulse_p=0.0035)),
        "both": ("texture", dict(sigma=10.0, impulse_p=0.0035)),
        "both_blur": ("texture", dict(sigma=10.0, impulse_p=0.0035, blur=col)),
        "both_contrast": ("texture", dict(sigma=10.0, impulse_p=0.0035, contrast=1.4)),
        "sigma_binary": ("binary", dict(sigma=10.0)),
    }
    out = {name: (noise_image(kind, H, W), np.stack([P.make_row(key=k, **kw) for k in keys])) for name, (kind, kw) in kinds.items()}
    # u1 < p is exact: with p = the field of one pixel (a multiple of 2^-24, exact in float32) that pixel must stay, `<=` replaces it
    edge = [int(P.pixel_hash(k, H, W, 1).reshape(-1)[NOISE_EDGE_PIXEL] >> np.uint64(40)) / 16777216.0 for k in keys]
    out["impulse_edge"] = (noise_image("texture", H, W), np.stack([P.make_row(key=k, impulse_p=p) for k, p in zip(keys, edge)]))
    return out


# ------------------------------------------------------------------------------------------------ Synthetic Shapes draw
SHAPES_SINGLE = {k: tuple((300 + 10 * k + j, 8) for j in range(4)) for k in range(9)}   # primitive -> 4 x (seed, B = 8): 32 tables
SHAPES_MIXED_SMALL = (21, 256)       # (seed, B) at the small size of tests/shapes_ref.py (192x256)
SHAPES_MIXED_SHIPPED = (22, 64)      # at the shipped 960x1280


def shapes_config():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_shapes_config.json")) as f:
        return json.load(f)["data"]


def shapes_params(kind):
    """kind: 0..8 = that primitive alone at the small size, "small" = all primitives at the small size, "shipped" = 960x1280"""
    from semantic_superpoint_amd import lib as L
    from tests import shapes_ref as S
    data = shapes_config()
    if kind == "shipped":
        return L.shapes_params_from_config(data)
    return L.shapes_params_from_config(S.small_config(data, None if kind == "small" else L.SHAPES_PRIMITIVES[kind]))


def shapes_batches(kind):
    return SHAPES_SINGLE[kind] if kind in SHAPES_SINGLE else ((SHAPES_MIXED_SMALL,) if kind == "small" else (SHAPES_MIXED_SHIPPED,))


@functools.lru_cache(maxsize=None)
def shapes_tables(kind):
    """[(seed, rows int32 [B, ROW], margins [B], [deviations])] of the restatement for the batches of `kind`"""
    from tests import shapes_ref as S
    p = shapes_params(kind)
    out = []
    for seed, B in shapes_batches(kind):
        rows, margins, devs = zip(*[S.draw(seed, n, p) for n in range(B)])
        out.append((seed, np.stack(rows), np.array(margins), list(devs)))
    return out


def cell_homographies(name):
    """float32 [SAMPLER_B, 3, 3]: the reference's host-scaled cell-space matrices (torch.inverse(trans) @ H @ trans)."""
    import torch
    H, W, _ = SAMPLER_CASES[name]
    hs = torch.from_numpy(sampler_homographies(name))
    return np.stack([C.scale_homography(hs[b], (H // 8, W // 8)).numpy() for b in range(SAMPLER_B)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the draw logic against the reference
REFERENCE_PRIMITIVES = (0, 1, 3, 4, 7)       # draw_lines, draw_polygon, draw_ellipses, draw_star, draw_cube
REFERENCE_BATCH = (31, 32)                   # (seed, B): primitive k draws seed + k (one seed for all would share its 32 backgrounds,
#                                              and with them deviation (a), among the five primitives)
REFERENCE_SIZE = [480, 640]                  # the smallest size at which every thickness range starts at 1 or more (int(480 * 0.003) = 1)


def reference_params(k):
    from semantic_superpoint_amd import lib as L
    from tests import shapes_ref as S
    d = S.small_config(shapes_config(), L.SHAPES_PRIMITIVES[k])
    d["generation"] = dict(d["generation"], image_size=list(REFERENCE_SIZE))
    return L.shapes_params_from_config(d)
