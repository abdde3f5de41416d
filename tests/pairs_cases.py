"""Inputs shared by tests/test_pairs_ref_cpu.py and tests/test_gpu_pairs_exact.py: the CPU file shows that the shares of pixels and
matrices the GPU tests may leave out (tie bands, small decision margins, near-integer class values) stay inside their caps
for exactly these seeds and shapes.  Everything here is computed on the CPU from the oracle and tests/pairs_ref.py."""
import functools
import math

import numpy as np

from oracle import cpu_ref as C
from tests import pairs_ref as R

SHAPES = ((40, 56), (37, 53), (120, 160))   # (37, 53): odd sizes, H * W no multiple of the 256-thread block
BATCH = 3
WARP = dict(translation=True, rotation=True, scaling=True, perspective=True, scaling_amplitude=0.2,
            perspective_amplitude_x=0.2, perspective_amplitude_y=0.2, patch_ratio=0.85, max_angle=1.57, allow_artifacts=True)
WARP_SEEDS = (11, 13)
SW_MIN = 1e-3            # no grid point of any case may have |sw| below this
BAND_CAP = 5e-3          # share of a case's pixels that may lie in the nearest warp's tie band
MARGIN_MIN, MARGIN_CAP = 1e-9, 1e-3   # sampler: matrices with a decision margin below MARGIN_MIN, and their share
SEM_CAP = 1e-2           # chain case of the class ids: share of pixels within 2 e_ref of an integer
SAMPLER_B = 2048


def f32_params(cfg):
    """The operator's C ABI carries its amplitudes as float: the reference is evaluated at those float values."""
    return {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in dict(R.SAMPLER_DEFAULTS, **cfg).items()}


# the sampler's configurations (test 4); every float is the fp32 value the device receives
_TIGHT = dict(WARP, allow_artifacts=False, patch_ratio=0.9, scaling_amplitude=0.3)
SAMPLER_CONFIGS = {
    "warp": (21, dict(WARP)),
    "defaults": (22, {}),
    "tight": (23, _TIGHT),                                   # margin 0.05: few scales and angles keep the corners inside
    "no_perspective": (24, dict(WARP, perspective=False)),
    "no_scaling": (25, dict(WARP, scaling=False)),
    "no_rotation": (26, dict(WARP, rotation=False)),
    "no_translation": (27, dict(WARP, translation=False)),
    "one_angle": (28, dict(WARP, n_angles=1)),
    "overflow": (29, dict(WARP, translation_overflow=0.1)),
}


@functools.lru_cache(maxsize=None)
def sampler_reference(name, B=SAMPLER_B):
    """(homographies, inv_homographies, margins) of pairs_ref.sample_homographies for a named configuration."""
    seed, cfg = SAMPLER_CONFIGS[name]
    return R.sample_homographies(seed, B, C.sample_homography, C.get_perspective_transform, **f32_params(cfg))


def _translation(tx_px, ty_px, H, W):
    """source = output + (tx, ty) pixels, in the normalised coordinates of the linspace(-1, 1) grid"""
    return np.array([[1, 0, 2.0 * tx_px / (W - 1)], [0, 1, 2.0 * ty_px / (H - 1)], [0, 0, 1]])


@functools.lru_cache(maxsize=None)
def warp_cases(H, W):
    """name -> inv_homographies float32 [BATCH, 3, 3] (output grid -> source, normalised coordinates)."""
    cases = {}
    for seed in WARP_SEEDS:   # the training config's WARP: the sampled matrix is `inv_homographies`
        cases["warp%d" % seed] = R.sample_homographies(seed, BATCH, C.sample_homography, C.get_perspective_transform,
                                                       **f32_params(WARP))[1]
    cases["identity_translations"] = np.stack([np.eye(3), _translation(0.3, 0.25, H, W), _translation(-1.7, 2.4, H, W)])
    s = _translation(0.3, -0.2, H, W)
    rot = np.array([[0., -1, 0], [1, 0, 0], [0, 0, 1]])
    cases["scales_rotation"] = np.stack([np.diag([0.5, 0.5, 1.0]) @ s, np.diag([2.0, 2.0, 1.0]) @ s, rot])
    # strong perspective: sw = 1 + 0.9 gx vanishes at gx = -1.11, just left of the image; the second one tilts about both axes
    # (horizon through gy = 1.14 at gx = 0), the third turns the source of the first by 0.3 rad
    c, sn = math.cos(0.3), math.sin(0.3)
    p1 = np.array([[1, 0, 0], [0, 1, 0], [0.9, 0, 1.0]])
    p2 = np.array([[1, 0.1, 0], [0, 1, 0], [0.1, -0.88, 1.0]])
    cases["perspective"] = np.stack([p1, p2, np.array([[c, -sn, 0], [sn, c, 0], [0, 0, 1]]) @ p1])
    out = {}
    for k, m in cases.items():
        m = np.ascontiguousarray(m, np.float32)
        for b in range(BATCH):
            assert np.abs(R.source_coords64(m[b], H, W)[2]).min() >= SW_MIN, (k, b)
        out[k] = m
    return out


def images(kind, H, W, seed=0):
    """float32 [BATCH, 1, H, W]"""
    rs = np.random.RandomState(1000 + seed)
    if kind == "noise":
        a = rs.uniform(0, 1, (BATCH, 1, H, W))
    elif kind == "ramp":      # linear: bilinear interpolation is exact on it, so it checks the coordinates alone
        y, x = np.mgrid[0:H, 0:W]
        a = np.stack([(0.25 + x / 256.0 + y / 512.0), (1.0 - x / 256.0), (y / 128.0)])[:, None]
    elif kind == "corners":   # a single bright pixel in each corner
        a = np.zeros((BATCH, 1, H, W))
        a[:, 0, 0, 0], a[:, 0, 0, W - 1], a[:, 0, H - 1, 0], a[:, 0, H - 1, W - 1] = 1.0, 0.75, 0.5, 0.25
    elif kind == "classes":   # class ids 0..133
        a = rs.randint(0, 134, (BATCH, 1, H, W))
    elif kind == "ones":
        a = np.ones((BATCH, 1, H, W))
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(a, np.float32)


def nearest_tau(inv, H, W):
    """tau of the nearest warp: twice the largest fp32 - fp64 source-coordinate distance over the pixels that can read the
    image; the second figure (all other pixels) must stay below 1/4 so that none of those can round into the image."""
    dev = [R.coord_deviation(inv[b], H, W) for b in range(inv.shape[0])]
    return 2.0 * max(d[0] for d in dev), max(d[1] for d in dev)


def keypoint_maps(H, W, seed):
    """float32 [BATCH, 1, H, W], 5 % key points"""
    return (np.random.RandomState(2000 + seed).uniform(0, 1, (BATCH, 1, H, W)) < 0.05).astype(np.float32)


@functools.lru_cache(maxsize=None)
def label_homographies(H, W):
    """name -> `homographies` float32 [BATCH, 3, 3] (image -> warped, normalised) for the colliding label scatters"""
    half = np.stack([np.diag([0.5, 0.5, 1.0]), np.array([[0.5, 0, 0.1], [0, 0.5, -0.2], [0, 0, 1]]),
                     np.array([[0.5, 0, -0.3], [0, 0.5, 0.3], [0, 0, 1]])])
    # WARP magnifies on average (patch_ratio 0.85), so two of ~100 integer points rarely round to one pixel: draws 48 and 53 of
    # seed 31 compress enough of the image that every 5 % map collides in res as well (tests/test_pairs_ref_cpu.py asserts it)
    warp = R.sample_homographies(31, 54, C.sample_homography, C.get_perspective_transform, **f32_params(WARP))[0][[53, 48, 53]]
    return {"half": np.ascontiguousarray(half, np.float32), "warp": np.ascontiguousarray(warp, np.float32)}
