"""Plain restatement of the device pair feed (csrc/pair_kernels.hip.h) in numpy only: no torch, no import from the product.
Written from the behaviour of the reference's text:

  inv_warp_image_batch    utils/utils.py:347-385      linspace(-1, 1) grid, 3x3 product, division, grid_sample(align_corners=True)
  compute_valid_mask      utils/utils.py:715-742      nearest warp of ones + cv2.erode(MORPH_ELLIPSE (2r, 2r))
  warp_points             utils/utils.py:315-343
  warpLabels / get_labels_bi / extrapolate_points / scatter_points   datasets/data_tools.py:6-63
  sample_homography_np    utils/homographies.py:12-141, inverted as in datasets/Coco.py:342-350
  warped class ids        datasets/Coco_sem.py:406-448

fp64 is the reference for VALUES.  The fixed-order fp32 forms exist only to measure how far fp32 coordinates stray from the
fp64 ones: that distance is what the GPU tests (tests/test_gpu_pairs_exact.py) derive their tie bands from."""
import math

import numpy as np

F32 = np.float32


# ------------------------------------------------------------------------------------------------
# source coordinates of the image warp (utils/utils.py:347-385)
# ------------------------------------------------------------------------------------------------
def source_coords64(inv_h, H, W):
    """Unnormalised source coordinates (ix, iy) [H, W] in fp64 of one matrix (its fp32 entries widened exactly), and the
    homogeneous coordinate sw: grid = linspace(-1, 1), (sx, sy, sw) = inv_h (gx, gy, 1), u = sx / sw,
    ix = ((u + 1) / 2) (W - 1) (grid_sample, align_corners=True)."""
    h = np.asarray(inv_h, np.float64).reshape(3, 3)
    gx = np.linspace(-1.0, 1.0, W)[None, :]
    gy = np.linspace(-1.0, 1.0, H)[:, None]
    sx = h[0, 0] * gx + h[0, 1] * gy + h[0, 2]
    sy = h[1, 0] * gx + h[1, 1] * gy + h[1, 2]
    sw = h[2, 0] * gx + h[2, 1] * gy + h[2, 2]
    return ((sx / sw + 1.0) / 2.0) * (W - 1), ((sy / sw + 1.0) / 2.0) * (H - 1), sw


def linspace32(n):
    """torch.linspace(-1, 1, n) in fp32: step = 2 / (n - 1), the lower half counted up from -1, the upper half down from 1."""
    i = np.arange(n)
    step = F32(2.0) / F32(n - 1)
    lo = F32(-1.0) + step * i.astype(F32)
    hi = F32(1.0) - step * (n - 1 - i).astype(F32)
    return np.where(i < n // 2, lo, hi).astype(F32)


def source_coords32(inv_h, H, W):
    """The same in fp32 in the reference's own sequence, every operation rounded once, the 3x3 product summed left to right:
    linspace, product, division, ((u + 1) / 2) * (W - 1).  Used ONLY to measure the fp32 - fp64 coordinate distance."""
    h = np.asarray(inv_h, F32).reshape(3, 3)
    gx = linspace32(W)[None, :]
    gy = linspace32(H)[:, None]
    sx = (h[0, 0] * gx + h[0, 1] * gy) + h[0, 2]
    sy = (h[1, 0] * gx + h[1, 1] * gy) + h[1, 2]
    sw = (h[2, 0] * gx + h[2, 1] * gy) + h[2, 2]
    assert sx.dtype == F32 and sw.dtype == F32
    ix = ((sx / sw + F32(1)) / F32(2)) * F32(W - 1)
    iy = ((sy / sw + F32(1)) / F32(2)) * F32(H - 1)
    return ix, iy


def coord_deviation(inv_h, H, W):
    """(largest |fp32 - fp64| coordinate distance over the pixels whose fp64 source lies in [-1, W] x [-1, H], the same over
    all other pixels).  Only the first kind of pixel can read the image; for the others every rounding candidate is outside
    as long as the second figure stays below 1/2."""
    ix, iy, _ = source_coords64(inv_h, H, W)
    jx, jy = source_coords32(inv_h, H, W)
    d = np.maximum(np.abs(jx.astype(np.float64) - ix), np.abs(jy.astype(np.float64) - iy))
    near = (ix >= -1) & (ix <= W) & (iy >= -1) & (iy <= H)
    return (float(d[near].max()) if near.any() else 0.0), (float(d[~near].max()) if (~near).any() else 0.0)


def warp_bilinear64(img, inv_h):
    """grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True) of one image [H, W] in fp64.
    Returns (warped, beyond): beyond marks the pixels all four of whose taps lie in the zero padding."""
    img = np.asarray(img, np.float64)
    H, W = img.shape
    ix, iy, _ = source_coords64(inv_h, H, W)
    x0, y0 = np.floor(ix), np.floor(iy)
    ax, ay = ix - x0, iy - y0
    pad = np.zeros((H + 2, W + 2))
    pad[1:-1, 1:-1] = img
    beyond = (x0 < -1) | (x0 > W - 1) | (y0 < -1) | (y0 > H - 1)
    xs = np.clip(x0, -1, W - 1).astype(np.int64) + 1
    ys = np.clip(y0, -1, H - 1).astype(np.int64) + 1
    out = (pad[ys, xs] * (1 - ax) * (1 - ay) + pad[ys, xs + 1] * ax * (1 - ay) + pad[ys + 1, xs] * (1 - ax) * ay +
           pad[ys + 1, xs + 1] * ax * ay)
    out[beyond] = 0.0
    return out, beyond


def warp_nearest64(img, inv_h):
    """grid_sample(mode="nearest", zeros padding, align_corners=True) in fp64: round half to even, zero when outside."""
    img = np.asarray(img, np.float64)
    H, W = img.shape
    ix, iy, _ = source_coords64(inv_h, H, W)
    rx, ry = np.rint(ix), np.rint(iy)
    ok = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
    out = np.zeros((H, W))
    out[ok] = img[ry[ok].astype(np.int64), rx[ok].astype(np.int64)]
    return out


def tie_band(inv_h, H, W, tau):
    """Pixels whose fp64 source coordinate is within tau of a rounding tie (k + 1/2) in x or in y."""
    ix, iy, _ = source_coords64(inv_h, H, W)
    dx = np.abs(ix - np.floor(ix) - 0.5)
    dy = np.abs(iy - np.floor(iy) - 0.5)
    return (dx <= tau) | (dy <= tau)


# ------------------------------------------------------------------------------------------------
# erosion of compute_valid_mask (utils/utils.py:736-740): cv2.erode with MORPH_ELLIPSE (2r, 2r)
# ------------------------------------------------------------------------------------------------
def ellipse_rows_dx(r, height=None):
    """OpenCV's published row formula (getStructuringElement, MORPH_ELLIPSE) in fp64 for a (2r, 2r) element (or (height,
    height)): rr = height // 2, row i: dy = i - rr, dx = round_half_even(rr * sqrt((rr^2 - dy^2) / rr^2))."""
    height = 2 * r if height is None else height
    rr = height // 2
    out = []
    for i in range(height):
        dy = i - rr
        out.append(int(round(rr * math.sqrt((rr * rr - dy * dy) * (1.0 / (rr * rr))))) if abs(dy) <= rr and rr else 0)
    return out


def ellipse(height, width=None):
    """The structuring element [height, width]: row i spans columns c - dx .. c + dx, c = width // 2, clipped."""
    width = height if width is None else width
    k = np.zeros((height, width), np.uint8)
    rr, c = height // 2, width // 2
    for i in range(height):
        dy = i - rr
        if abs(dy) <= rr:
            dx = int(round(c * math.sqrt((rr * rr - dy * dy) * (1.0 / (rr * rr))))) if rr else 0
            k[i, max(c - dx, 0):min(c + dx + 1, width)] = 1
    return k


def ellipse_rows_dx_kernel32(r):
    """The device kernel's fp32 form lrintf(r * sqrtf((r*r - dy*dy) / (r*r))), every operation in np.float32."""
    out = []
    for i in range(2 * r):
        dy = i - r
        q = F32(max(r * r - dy * dy, 0)) / F32(r * r)
        out.append(int(np.rint(F32(r) * np.sqrt(q, dtype=F32))))
    return out


def erode(mask, r):
    """Sliding minimum over the (2r, 2r) ellipse with anchor (r, r); pixels outside the image are ignored (cv2's default
    border of +inf).  mask [H, W], any float values."""
    m = np.asarray(mask)
    if r <= 0:
        return m.copy()
    k = ellipse(2 * r)
    H, W = m.shape
    pad = np.full((H + 2 * r, W + 2 * r), np.inf)               # pixel (y, x) sits at pad[y + r, x + r]
    pad[r:r + H, r:r + W] = m
    out = np.full((H, W), np.inf)
    for i in range(2 * r):
        for j in range(2 * r):
            if k[i, j]:                                          # out[y, x] = min over the element of m[y + i - r, x + j - r]
                out = np.minimum(out, pad[i:i + H, j:j + W])
    return out.astype(m.dtype)                                   # (r, r) belongs to the element: never +inf


# ------------------------------------------------------------------------------------------------
# homography sampler: the kernel's counter RNG; the geometry stays the oracle's
# ------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


def mix(x):
    """The 64-bit finaliser of the device stream (uint64 arithmetic: Python integers reduced modulo 2^64)."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


class DeviceStream:
    """The random numbers homography n of a call with `seed` consumes on the device: key = mix(seed ^ n << 32), draw c is
    (mix(key ^ c * 0xD1342543DE82EF95) >> 11) * 2^-53.  Offers what oracle.cpu_ref.sample_homography asks of its `rs`
    (randn, randint, uniform(lo, hi)) and records the smallest margin of the decisions taken on its numbers:
    | |v| - 2 | of every normal (the truncation test that follows it) and the distance of uniform() * k from an integer."""

    def __init__(self, seed, n):
        self.key = mix((int(seed) ^ (int(n) << 32)) & M64)
        self.ctr = 0
        self.margin = math.inf
        self.normals = 0

    def uniform(self, lo=None, hi=None):
        u = (mix(self.key ^ ((self.ctr * 0xD1342543DE82EF95) & M64)) >> 11) * (1.0 / 9007199254740992.0)
        self.ctr += 1
        return u if lo is None else lo + u * (hi - lo)

    def randn(self):  # Box-Muller, two uniforms per normal
        u1 = max(self.uniform(), 1e-300)
        u2 = self.uniform()
        v = math.sqrt(-2.0 * math.log(u1)) * math.cos(6.283185307179586 * u2)
        self.margin = min(self.margin, abs(abs(v) - 2.0))
        self.normals += 1
        return v

    def randint(self, k):
        x = self.uniform() * k
        self.margin = min(self.margin, abs(x - round(x)))
        return min(int(x), k - 1)


def sample_homography_walk(rs, get_perspective_transform, perspective=True, scaling=True, rotation=True, translation=True,
                           n_scales=5, n_angles=25, scaling_amplitude=0.1, perspective_amplitude_x=0.1,
                           perspective_amplitude_y=0.1, patch_ratio=0.5, max_angle=math.pi / 2, allow_artifacts=False,
                           translation_overflow=0.0):
    """utils/homographies.py:12-141 walked once more on the numbers of `rs`, for two things the oracle's function does not
    hand out: the matrix BEFORE its float32 cast (through the solver passed in: the oracle's get_perspective_transform on
    pts * (2, 2) - 1) and the smallest distance of a candidate corner from 0 and from 1 where allow_artifacts=False turns
    that comparison into a decision.  The caller checks that the cast of this matrix IS the oracle's result."""
    def tn(std):
        while True:
            v = rs.randn()
            if abs(v) <= 2:
                return v * std
    corner = math.inf
    pts1 = np.array([[0., 0.], [0., 1.], [1., 1.], [1., 0.]])
    margin = (1 - patch_ratio) / 2
    pts2 = margin + np.array([[0, 0], [0, patch_ratio], [patch_ratio, patch_ratio], [patch_ratio, 0]])
    if perspective:
        if not allow_artifacts:
            perspective_amplitude_x = min(perspective_amplitude_x, margin)
            perspective_amplitude_y = min(perspective_amplitude_y, margin)
        pd = tn(perspective_amplitude_y / 2)
        hl = tn(perspective_amplitude_x / 2)
        hr = tn(perspective_amplitude_x / 2)
        pts2 += np.array([[hl, pd], [hl, -pd], [hr, pd], [hr, -pd]])
    if scaling:
        scales = np.array([1.0] + [1 + tn(scaling_amplitude / 2) for _ in range(n_scales)])
        center = pts2.mean(axis=0, keepdims=True)
        scaled = (pts2 - center)[None] * scales[:, None, None] + center
        if allow_artifacts:
            valid = np.arange(n_scales)
        else:
            corner = min(corner, float(np.minimum(np.abs(scaled), np.abs(scaled - 1)).min()))
            valid = np.where(((scaled >= 0) & (scaled < 1)).all(axis=(1, 2)))[0]
        pts2 = scaled[valid[rs.randint(valid.shape[0])]]
    if translation:
        t_min, t_max = pts2.min(axis=0), (1 - pts2).min(axis=0)
        if allow_artifacts:
            t_min += translation_overflow
            t_max += translation_overflow
        pts2 += np.array([rs.uniform(-t_min[0], t_max[0]), rs.uniform(-t_min[1], t_max[1])])[None]
    if rotation:
        angles = np.concatenate((np.linspace(-max_angle, max_angle, n_angles), [0.0]))
        center = pts2.mean(axis=0, keepdims=True)
        rot = np.stack([np.cos(angles), -np.sin(angles), np.sin(angles), np.cos(angles)], axis=1).reshape(-1, 2, 2)
        rotated = np.matmul((pts2 - center)[None], rot) + center
        if allow_artifacts:
            valid = np.arange(n_angles)
        else:
            corner = min(corner, float(np.minimum(np.abs(rotated), np.abs(rotated - 1)).min()))
            valid = np.where(((rotated >= 0) & (rotated < 1)).all(axis=(1, 2)))[0]
        pts2 = rotated[valid[rs.randint(valid.shape[0])]]
    return get_perspective_transform(pts1 * 2.0 - 1, pts2 * 2.0 - 1), corner


# the defaults of sample_homography_np (utils/homographies.py:13-16), which the device operator shares; the oracle's own
# defaults are the training config's, so every key is always passed on
SAMPLER_DEFAULTS = dict(perspective=True, scaling=True, rotation=True, translation=True, n_scales=5, n_angles=25,
                        scaling_amplitude=0.1, perspective_amplitude_x=0.1, perspective_amplitude_y=0.1, patch_ratio=0.5,
                        max_angle=math.pi / 2, allow_artifacts=False, translation_overflow=0.0)


def sample_homographies(seed, B, sample_homography, get_perspective_transform, **cfg):
    """What op_sample_homographies(B, seed, **cfg) must return, from the oracle's geometry on the device stream:
    (homographies [B,3,3] fp64 = inv of the sampled matrix, inv_homographies [B,3,3] fp64 = the sampled matrix,
     margins [B] = the smallest margin of any decision behind each matrix)."""
    hs, inv, mg = [], [], []
    cfg = dict(SAMPLER_DEFAULTS, **cfg)
    for n in range(B):
        oracle = sample_homography(DeviceStream(seed, n), shape=(2, 2), shift=-1, **cfg)
        st = DeviceStream(seed, n)
        m64, corner = sample_homography_walk(st, get_perspective_transform, **cfg)
        assert np.array_equal(m64.astype(F32), oracle), "the walk left the oracle's geometry (seed %d, n %d)" % (seed, n)
        inv.append(m64)
        hs.append(np.linalg.inv(m64))
        mg.append(min(st.margin, corner))
    return np.stack(hs), np.stack(inv), np.array(mg)


# ------------------------------------------------------------------------------------------------
# warpLabels(bilinear=True) (datasets/data_tools.py:6-63) with a DEFINED scatter order
# ------------------------------------------------------------------------------------------------
def warp_points32(hpx, pts_xy):
    """warp_points (utils/utils.py:315-343) of integer points with ONE pixel-space matrix in the fp32 operation order the
    reference's `homographies @ points^T` takes on the CPU the goldens were made on (oneMKL sgemm, N >= 12 points):
    fma(p2, 1, fma(p1, y, p0 * x)) per row, then the correctly rounded division.  Evaluated in float64 with an explicit
    float32 rounding after every operation (products of a float32 and a small integer are exact in float64).
    torch on another CPU may pick a kernel that differs in the last bit, so the tests use THIS form on every host and
    tests/test_pairs_ref_cpu.py pins it bit for bit to G11 and to the oracle's warp_points where the goldens were made."""
    p = np.asarray(hpx, F32).reshape(3, 3).astype(np.float64)
    x = np.asarray(pts_xy)[:, 0].astype(np.float64)
    y = np.asarray(pts_xy)[:, 1].astype(np.float64)
    r32 = lambda v: v.astype(F32).astype(np.float64)  # noqa: E731
    rows = [r32(r32(p[r, 1] * y + r32(p[r, 0] * x)) + p[r, 2]) for r in range(3)]
    return np.stack(((rows[0] / rows[2]).astype(F32), (rows[1] / rows[2]).astype(F32)), axis=1)


def map_points(label_map):
    """Key points of a map [H, W] as (x, y) rows in row-major order of the map (torch.nonzero order)."""
    ys, xs = np.nonzero(np.asarray(label_map))
    return np.stack((xs, ys), axis=1).astype(np.int64)


def warp_labels_full(warped, H, W):
    """warped: float32 [N, 2] (x, y), the warped coordinates of the key points in row-major order of the map (warp_points32
    on the host-scaled pixel matrix: the reference's own fp32 operations).  Every scatter is an explicit loop in the order in which the
    reference's single indexed assignment lists its writes, so the LAST write of that list wins:
      labels / res   the last point that rounds (half to even) to the pixel;
      labels_bi      the four neighbour lists (x, y), (x, y+1), (x+1, y), (x+1, y+1) of the truncated points are concatenated
                     (extrapolate_points), filtered and scattered once: the later list wins, within a list the later point.
    Returns (labels [H,W], res [2,H,W], labels_bi [H,W], n_collisions_res, n_collisions_bi), float32."""
    wp = np.asarray(warped, F32).reshape(-1, 2)
    lab = np.zeros((H, W), F32)
    res = np.zeros((2, H, W), F32)
    bi = np.zeros((H, W), F32)
    hit_bi = np.zeros((H, W), np.int64)
    hit_res = np.zeros((H, W), np.int64)
    pi = wp.astype(np.int64).astype(F32)                        # pnts.long(): truncation toward zero
    rx, ry = wp[:, 0] - pi[:, 0], wp[:, 1] - pi[:, 1]
    one = F32(1)
    lists = (((0, 0), (one - rx) * (one - ry)), ((0, 1), (one - rx) * ry), ((1, 0), rx * (one - ry)), ((1, 1), rx * ry))
    for (ox, oy), wts in lists:
        assert wts.dtype == F32
        for p in range(wp.shape[0]):
            x, y = pi[p, 0] + F32(ox), pi[p, 1] + F32(oy)
            if 0 <= x <= W - 1 and 0 <= y <= H - 1:             # filter_points, then quan = round().long()
                bi[int(np.rint(y)), int(np.rint(x))] = wts[p]
                hit_bi[int(np.rint(y)), int(np.rint(x))] += 1
    for p in range(wp.shape[0]):
        x, y = wp[p]
        if 0 <= x <= W - 1 and 0 <= y <= H - 1:
            qx, qy = np.rint(x), np.rint(y)                     # torch.round: half to even
            lab[int(qy), int(qx)] = 1
            res[0, int(qy), int(qx)] = x - qx
            res[1, int(qy), int(qx)] = y - qy
            hit_res[int(qy), int(qx)] += 1
    return lab, res, bi, int((hit_res > 1).sum()), int((hit_bi > 1).sum())


# ------------------------------------------------------------------------------------------------
# class ids (datasets/Coco_sem.py:447-448)
# ------------------------------------------------------------------------------------------------
def sem_finalize(sem_warped, valid, n_classes):
    """float class map -> int64 by truncation toward zero; pixels outside the valid mask -> n_classes."""
    out = np.trunc(np.asarray(sem_warped, np.float64)).astype(np.int64)
    out[np.asarray(valid) == 0] = n_classes
    return out
