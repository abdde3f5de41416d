"""numpy restatement of `ssp_op_photometric_apply` and `ssp_op_photometric_draw` (csrc/photo_kernels.hip.h, DESIGN.md sections 14
and 30) for ONE image and its row of draws, written from the stage list of the design section and from utils/photometric.py -
a helper of tests/test_photometric_cpu.py, tests/test_draws_ref_cpu.py, tests/test_gpu_photometric.py and
tests/test_gpu_draws_exact.py, not a test.  The draw and the per-pixel noise stages (sigma, impulse probability) are restated
on the bits of the device stream (tests/pairs_ref.py::DeviceStream, mix): `draw`, `noise`.

Row layout (include/ssp_hip.h SSP_PHOTO_*): brightness, contrast, sigma, impulse p, blur flag, 9 weights, 32 x (cx, cy, ax, ay,
angle), transparency, kernel size, 4 x 16 key bits."""
import numpy as np

BRIGHTNESS, CONTRAST, SIGMA, IMPULSE_P, BLUR_FLAG, BLUR_W, ELLIPSES, TRANSPARENCY, KSIZE, KEY, STRIDE = 0, 1, 2, 3, 4, 5, 14, 174, 175, 176, 180
MAX_ELLIPSES = 32
TIE_EPS = 1e-3


def gaussian_sigma(k):
    """what cv2.GaussianBlur(..., (k, k), 0) derives from the kernel size"""
    return 0.3 * ((k - 1) * 0.5 - 1) + 0.8


def gaussian_weights(k):
    r = (k - 1) // 2
    j = np.arange(k, dtype=np.float64) - r
    w = np.exp(-(j * j) / (2.0 * gaussian_sigma(k) ** 2))
    return w / w.sum()


def reflect101(p, n):
    """cv2.BORDER_REFLECT_101 index for any distance"""
    p = np.asarray(p).copy()
    if n == 1:
        return np.zeros_like(p)
    for _ in range(64):
        bad = (p < 0) | (p >= n)
        if not bad.any():
            break
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * (n - 1) - p, p)
    return p


def motion_blur_weights(angle_deg, direction, dtype=np.float64):
    """MotionBlur(3): the centre-column line kernel linspace(d, 1 - d, 3), d = (direction + 1) / 2, rotated bilinearly about
    the centre (zeros outside), normalised to sum 1.  dtype=np.longdouble repeats the arithmetic after the double cos / sin
    in extended precision (weight_midpoint_distance)."""
    d = dtype((direction + 1.0) * 0.5)
    line = np.zeros((3, 3), dtype)
    line[:, 1] = [d, dtype(0.5), dtype(1.0) - d]
    a = np.deg2rad(angle_deg)
    c, s = dtype(np.cos(a)), dtype(np.sin(a))
    out = np.zeros((3, 3), dtype)
    for y in range(3):
        for x in range(3):
            dx, dy = x - 1, y - 1
            sx, sy = c * dx + s * dy + 1.0, -s * dx + c * dy + 1.0
            fx, fy = np.floor(sx), np.floor(sy)
            ax, ay = sx - fx, sy - fy

            def at(yy, xx):
                return line[yy, xx] if 0 <= yy < 3 and 0 <= xx < 3 else 0.0
            x0, y0 = int(fx), int(fy)
            out[y, x] = (at(y0, x0) * (1 - ax) * (1 - ay) + at(y0, x0 + 1) * ax * (1 - ay) + at(y0 + 1, x0) * (1 - ax) * ay +
                         at(y0 + 1, x0 + 1) * ax * ay)
    return out / out.sum()


def make_row(brightness=0, contrast=1.0, sigma=0.0, impulse_p=0.0, blur=None, ellipses=(), transparency=0.0, ksize=0, key=0):
    """A hand-made row; the defaults are the neutral values (every stage off).  blur: 3x3 weights or None."""
    r = np.zeros(STRIDE, np.float32)
    r[BRIGHTNESS], r[CONTRAST], r[SIGMA], r[IMPULSE_P] = brightness, contrast, sigma, impulse_p
    r[BLUR_W + 4] = 1.0
    if blur is not None:
        r[BLUR_FLAG] = 1.0
        r[BLUR_W:BLUR_W + 9] = np.asarray(blur, np.float64).reshape(9)
    r[ELLIPSES + 2:ELLIPSES + 5 * MAX_ELLIPSES:5] = -1.0
    r[ELLIPSES + 3:ELLIPSES + 5 * MAX_ELLIPSES:5] = -1.0
    for i, e in enumerate(ellipses):
        r[ELLIPSES + 5 * i:ELLIPSES + 5 * i + 5] = e
    r[TRANSPARENCY], r[KSIZE] = transparency, ksize
    for i in range(4):
        r[KEY + i] = (int(key) >> (16 * i)) & 0xFFFF
    return r


def ellipse_mask(row, H, W):
    """(mask in {0, 1} float64 [H, W], smallest |f - 1| over pixels and ellipses) with f = (x'/ax)^2 + (y'/ay)^2 in the rotated
    frame: a pixel is inside when f <= 1.  The second value tells how close any pixel sits to an ellipse's edge."""
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    mask = np.zeros((H, W), bool)
    margin = np.inf
    for i in range(MAX_ELLIPSES):
        cx, cy, ax, ay, ang = (float(v) for v in row[ELLIPSES + 5 * i:ELLIPSES + 5 * i + 5])
        if ax < 0:
            break
        if ax == 0 or ay == 0:
            continue
        a = np.deg2rad(ang)
        dx, dy = xs - cx, ys - cy
        xr, yr = dx * np.cos(a) + dy * np.sin(a), dy * np.cos(a) - dx * np.sin(a)
        f = (xr / ax) ** 2 + (yr / ay) ** 2
        mask |= f <= 1.0
        margin = min(margin, float(np.abs(f - 1.0).min()))
    return mask.astype(np.float64), margin


def blurred_mask(row, H, W):
    """M / 255: the separable Gaussian blur (reflect_101) of the ellipse mask, in float64"""
    k = int(row[KSIZE]) | 1
    r = (k - 1) // 2
    w = gaussian_weights(k)
    m, _ = ellipse_mask(row, H, W)
    cols = reflect101(np.arange(W)[:, None] + np.arange(k)[None, :] - r, W)   # [W, k]
    rows = reflect101(np.arange(H)[:, None] + np.arange(k)[None, :] - r, H)   # [H, k]
    rp = np.einsum("ywk,k->yw", m[:, cols], w)
    return np.einsum("ykw,k->yw", rp[rows, :], w)


# ------------------------------------------------------------------------------------------------
# the draw (ssp_op_photometric_draw): utils/photometric.py:10-113 on the device stream, DESIGN.md section 14
# ------------------------------------------------------------------------------------------------
PHOTO_TAG = 0x70686F746F6D6574      # "photomet": separates this stream from the homography sampler's of the same seed
PIXEL_MUL = 0xD1342543DE82EF95      # the counter multiplier of the device stream (pairs_ref.DeviceStream.uniform)
DRAW_MUTANTS = ("centre_from_ax", "angle_360", "direction_raw")
NOISE_MUTANTS = ("u1_no_plus_one", "gauss_sin", "gauss_odd_stream", "impulse_cos2", "impulse_le", "noise_before_contrast")
# what the parser makes of the shipped COCO block (tests/golden/g17_photometric_config.json); floats are the float32 values of
# the C ABI.  A primitive that is off writes its neutral values and consumes no uniform.
SHIPPED = dict(brightness=1, contrast=1, noise=1, impulse=1, motion_blur=1, shade=1, max_abs_change=50, contrast_lo=0.5,
               contrast_hi=1.5, std_lo=0.0, std_hi=10.0, p_lo=0.0, p_hi=0.0035, nb_ellipses=20, t_lo=-0.5, t_hi=0.5,
               ksize_lo=100, ksize_hi=150)
PRIMITIVES = ("brightness", "contrast", "noise", "impulse", "motion_blur", "shade")


def f32(x):
    return float(np.float32(x))


def _stream(seed, n):
    from tests.pairs_ref import M64, DeviceStream, mix
    return DeviceStream(mix((int(seed) ^ PHOTO_TAG) & M64), n)


def draw(seed, n, params, H, W, mutant=None):
    """(row float32 [STRIDE], margin) of draw_full."""
    return draw_full(seed, n, params, H, W, mutant)[:2]


def draw_full(seed, n, params, H, W, mutant=None):
    """Row n of ssp_op_photometric_draw(B, H, W, seed, params): (row float32 [STRIDE], margin, (angle_deg, direction) or None).
    Stream key mix(mix(seed ^ PHOTO_TAG) ^ n << 32); the uniforms are consumed in the reference's order: iaa.Add (a discrete
    uniform integer in [-c, c]), LinearContrast, AdditiveGaussianNoise, ImpulseNoise (each float32(lo + u (hi - lo)) in double),
    Sometimes(0.5) / MotionBlur(3) (flag u < 0.5, angle 360 u degrees, direction 2 u - 1), then additive_shade line for line:
    per ellipse ax, ay = int(max(u min_dim, min_dim / 5)), x = randint(max_rad, W - max_rad), y likewise in H, angle 90 u;
    transparency; kernel size randint(lo, hi) made odd.  The four key words are mix(key ^ (0xA5A5 + i)) >> 48.
    margin: the smallest distance from a decision boundary of every truncation, of the flag's u < 0.5 and of the floors
    inside the motion-blur rotation (DeviceStream.randint records its own)."""
    assert mutant is None or mutant in DRAW_MUTANTS, mutant
    from tests.pairs_ref import mix
    p = {k: (f32(v) if isinstance(v, float) else v) for k, v in params.items()}
    rs = _stream(seed, n)
    m = [np.inf]

    def note(x):
        m[0] = min(m[0], abs(x))

    def span(lo, hi):
        return np.float32(lo + rs.uniform() * (hi - lo))

    row = make_row()
    if p["brightness"]:
        c = p["max_abs_change"]
        row[BRIGHTNESS] = rs.randint(2 * c + 1) - c
    if p["contrast"]:
        row[CONTRAST] = span(p["contrast_lo"], p["contrast_hi"])
    if p["noise"]:
        row[SIGMA] = span(p["std_lo"], p["std_hi"])
    if p["impulse"]:
        row[IMPULSE_P] = span(p["p_lo"], p["p_hi"])
    blur = None
    if p["motion_blur"]:
        u = rs.uniform()
        note(u - 0.5)
        row[BLUR_FLAG] = 1.0 if u < 0.5 else 0.0
        angle = rs.uniform() * 360.0
        direction = rs.uniform() * 2.0 - 1.0
        a = np.deg2rad(angle)
        for dx in (-1, 0, 1):            # the floors of the bilinear rotation (continuous across them, recorded all the same)
            for dy in (-1, 0, 1):
                for s in (np.cos(a) * dx + np.sin(a) * dy + 1.0, -np.sin(a) * dx + np.cos(a) * dy + 1.0):
                    if (dx, dy) != (0, 0):
                        note(s - np.rint(s))
        blur = (angle, direction)
        wts = motion_blur_weights(angle, 2.0 * direction - 1.0 if mutant == "direction_raw" else direction)
        row[BLUR_W:BLUR_W + 9] = wts.reshape(9)           # float32(k_i / sum)
    if p["shade"]:
        min_dim = min(H, W) / 4.0

        def axis():
            x = rs.uniform() * min_dim
            if x > min_dim / 5.0:
                note(x - np.rint(x))
            return int(max(x, min_dim / 5.0))

        def randint(lo, hi):             # np.random.randint(lo, hi): [lo, hi)
            return lo + rs.randint(max(hi - lo, 1))

        for e in range(p["nb_ellipses"]):
            ax, ay = axis(), axis()
            max_rad = max(ax, ay)
            x = randint(max_rad, W - (ax if mutant == "centre_from_ax" else max_rad))
            y = randint(max_rad, H - (ay if mutant == "centre_from_ax" else max_rad))
            ang = np.float32(rs.uniform() * (360.0 if mutant == "angle_360" else 90.0))
            row[ELLIPSES + 5 * e:ELLIPSES + 5 * e + 5] = (x, y, ax, ay, ang)
        row[TRANSPARENCY] = span(p["t_lo"], p["t_hi"])
        k = randint(p["ksize_lo"], p["ksize_hi"])
        row[KSIZE] = k + 1 if k % 2 == 0 else k
    for i in range(4):
        row[KEY + i] = mix(rs.key ^ (0xA5A5 + i)) >> 48
    return row, min(m[0], rs.margin), blur


def row_key(row):
    return sum(int(row[KEY + i]) << (16 * i) for i in range(4))


def weight_midpoint_distance(angle_deg, direction):
    """For the nine motion-blur weights: (the relative distance of the double k_i / sum from the nearest float32 rounding
    midpoint, whether the float32 cast of k_i / sum evaluated in numpy.longdouble from the same double cos / sin equals the
    cast of the double).  The device's cos / sin may differ from libm's in the last place, which moves the double quotient
    by a few 1e-16 relative: its float32 cast can then be the neighbour only where this distance is tiny."""
    w = motion_blur_weights(angle_deg, direction).reshape(9)
    wl = motion_blur_weights(angle_deg, direction, np.longdouble).reshape(9)
    dist, agree = np.full(9, np.inf), np.ones(9, bool)
    for i, x in enumerate(w):
        agree[i] = np.float32(wl[i]) == np.float32(x)
        if x == 0.0:
            continue
        f = np.float32(x)
        nb = np.nextafter(f, np.float32(np.inf) if float(f) < x else np.float32(-np.inf))
        mid = (np.longdouble(float(f)) + np.longdouble(float(nb))) / 2
        dist[i] = float(abs(np.longdouble(x) - mid) / np.longdouble(x))
    return dist, agree


# ------------------------------------------------------------------------------------------------
# stages 4 and 5: the per-pixel noise, float64 on the bits the device draws
# ------------------------------------------------------------------------------------------------
TWO_PI_F32, HALF_PI_F32 = f32(6.2831853), f32(1.5707963)     # the float32 constants of the device's evaluation
# Measured on the MI355X (tools/measure_draws_noise.py, profiles/draws_exact_measure.txt): over 14.7 M noisy pixels the device's
# level differs from rint(p_ref) at 65, and the largest e / base that admits one of them is 4.66e-8.  tau = 4 x that, rounded up to
# a power of two.
NOISE_MEASURED = 4.664122e-08
NOISE_TAU = 2.0 ** -22
assert NOISE_TAU / 2 < 4 * NOISE_MEASURED <= NOISE_TAU


def pixel_hash(key, H, W, odd):
    """mix(key ^ (2 pix + odd) * PIXEL_MUL) for every pixel, uint64 [H, W]"""
    from tests.draws_ref import splitmix64_np
    pix = np.arange(H * W, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return splitmix64_np(np.uint64(key) ^ ((np.uint64(2) * pix + np.uint64(odd)) * np.uint64(PIXEL_MUL))).reshape(H, W)


def _fields(h):
    return (h >> np.uint64(40)).astype(np.float64), ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64)


def noise(row, H, W, v=None, tau=0.0, mutant=None):
    """Stages 4 and 5 on the 8-bit levels v (float64 [H, W]; mid-grey 128 when not given), in float64:
      4  sigma > 0:  h = mix(key ^ (2 pix) PIXEL_MUL), u1 = ((h >> 40) + 1) 2^-24, u2 = (h >> 16 & 0xFFFFFF) 2^-24,
                     p = v + sigma sqrt(-2 ln u1) cos(6.2831853f u2), level = clip(rint(p))
      5  prob > 0:   h = mix(key ^ (2 pix + 1) PIXEL_MUL), u1 = (h >> 40) 2^-24 (no + 1), u2 as above; where u1 < prob (both sides
                     exact float32 values) the level becomes clip(rint(255 sin^2(1.5707963f u2)))
    Returns (pre, level, tie, base): pre = the LAST pre-rounding value of each pixel (its input level where no stage touched
    it), tie = a pre-rounding value within tau * base of a .5 boundary between two levels of 0..255, base = sigma |z| + |v|
    for the Gaussian and 255 for the impulse value."""
    assert mutant is None or mutant in NOISE_MUTANTS, mutant
    row = np.asarray(row, np.float32)
    key = row_key(row)
    v = np.full((H, W), 128.0) if v is None else np.asarray(v, np.float64)
    sigma, prob = float(row[SIGMA]), float(row[IMPULSE_P])
    pre, tie, base = v.copy(), np.zeros((H, W), bool), np.zeros((H, W))

    def near_tie(x, e):
        return (np.abs(x - np.floor(x) - 0.5) <= e) & (x > 0.0) & (x < 255.0)      # (beyond 0 and 255 both roundings clip alike)

    if sigma > 0:
        f1, u2 = _fields(pixel_hash(key, H, W, 1 if mutant == "gauss_odd_stream" else 0))
        u1 = (f1 + (0.0 if mutant == "u1_no_plus_one" else 1.0)) / 16777216.0
        with np.errstate(divide="ignore"):
            r = np.sqrt(-2.0 * np.log(u1))
        z = r * (np.sin if mutant == "gauss_sin" else np.cos)(TWO_PI_F32 * (u2 / 16777216.0))
        z = np.where(np.isfinite(z), z, 0.0)     # (only the mutant can take the logarithm of 0)
        pre = v + sigma * z
        base = sigma * np.abs(z) + np.abs(v)
        tie = near_tie(pre, tau * base)
        v = np.clip(np.rint(pre), 0, 255)
    if prob > 0:
        f1, u2 = _fields(pixel_hash(key, H, W, 1))
        u1 = (f1 / 16777216.0).astype(np.float32)
        hit = (u1 <= np.float32(prob)) if mutant == "impulse_le" else (u1 < np.float32(prob))
        sn = (np.cos if mutant == "impulse_cos2" else np.sin)(HALF_PI_F32 * (u2 / 16777216.0))
        val = 255.0 * sn * sn
        pre = np.where(hit, val, pre)
        base = np.where(hit, 255.0, base)
        tie = np.where(hit, near_tie(val, tau * 255.0), tie)
        v = np.where(hit, np.clip(np.rint(val), 0, 255), v)
    return pre, v, tie, base


def noise_samples(img, row, dev_out):
    """The measurement behind NOISE_TAU, for a row without blur and shade: dev_out float32 [H, W] is the device's result.
    For every pixel whose device level differs from rint(p_ref): the smallest e / base that admits it, i.e. the distance of
    p_ref from the .5 boundary over base - or infinity when the device's level is not the one across that boundary.
    Returns (samples, number of pixels)."""
    img, row = np.asarray(img, np.float32), np.asarray(row, np.float32)
    assert row[BLUR_FLAG] == 0 and row[KSIZE] == 0
    H, W = img.shape
    quiet = row.copy()
    quiet[SIGMA] = quiet[IMPULSE_P] = 0
    v, may = apply(img, quiet)
    assert not may.any()
    pre, lvl, _, base = noise(row, H, W, np.rint(v * 255.0), 0.0)
    dev = np.rint(np.asarray(dev_out, np.float64) * 255.0)
    bad = dev != lvl
    fl = np.floor(pre[bad])
    across = np.clip(2 * fl + 1 - np.rint(pre[bad]), 0, 255)       # the level on the other side of the nearest .5 boundary
    s = np.abs(pre[bad] - fl - 0.5) / base[bad]
    return np.where(dev[bad] == across, s, np.inf), H * W


def apply(img, row, tau=None, mutant=None):
    """img: float32 [H, W] in [0, 1]; row: float32 [STRIDE].  Returns (out float64 [H, W], may_differ bool [H, W]): may_differ
    marks the pixels whose pre-rounding value of an 8-bit stage lies within TIE_EPS of a .5 tie (for the noise stages: within
    tau * base, see noise(); for the 3x3 blur: or whose neighbourhood holds such a pixel) - an fp32 evaluation may round those
    the other way, by one level.  Without the shade, float32(out) is the exact expected result."""
    img = np.asarray(img, np.float32)
    row = np.asarray(row, np.float32)
    noisy = row[SIGMA] != 0 or row[IMPULSE_P] != 0
    if noisy and tau is None:
        raise ValueError("a row with noise needs the measured tau of the noise stages (NOISE_TAU)")
    H, W = img.shape
    may = np.zeros((H, W), bool)
    v = np.floor(np.clip(img * np.float32(255.0), 0, 255)).astype(np.float64)         # 1 (float32 product, truncation)
    v = np.clip(v + float(row[BRIGHTNESS]), 0, 255)                                   # 2
    alpha = float(row[CONTRAST])
    if noisy and mutant == "noise_before_contrast":
        _, v, tie, _ = noise(row, H, W, v, tau)
        may |= tie
    if alpha != 1.0:                                                                  # 3
        pre = 127.0 + alpha * (v - 127.0)
        may |= np.abs(pre - np.floor(pre) - 0.5) < TIE_EPS
        v = np.clip(np.rint(pre), 0, 255)
    if noisy and mutant != "noise_before_contrast":                                   # 4, 5
        _, v, tie, _ = noise(row, H, W, v, tau, mutant)
        may |= tie
    if row[BLUR_FLAG] != 0:                                                           # 6
        wts = row[BLUR_W:BLUR_W + 9].astype(np.float64).reshape(3, 3)
        yy, xx = reflect101(np.arange(-1, H + 1), H), reflect101(np.arange(-1, W + 1), W)
        pad, pmay = v[yy][:, xx], may[yy][:, xx]
        pre = sum(wts[dy, dx] * pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
        may = np.any([pmay[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], axis=0)
        may |= np.abs(pre - np.floor(pre) - 0.5) < TIE_EPS
        v = np.clip(np.rint(pre), 0, 255)
    out = (v.astype(np.float32) / np.float32(255.0)).astype(np.float64)               # 7 (float32 division)
    if int(row[KSIZE]) >= 1:                                                          # 8 (no quantisation)
        out = np.clip(out * 255.0 * (1.0 - float(row[TRANSPARENCY]) * blurred_mask(row, H, W)), 0, 255) / 255.0
    return out, may


# ---- the hand-made cases of the exact GPU test; tests/test_photometric_cpu.py checks their tie sets and edge margins ----
# contrast factors 0.6 and 1.4: 127 + alpha * n then lies on a multiple of 1/5 (up to 3e-6 from the float32 factor), never near .5.
# blur: angle 0 / direction 0 gives the column [1/3, 1/3, 1/3], angle 90 / direction -1 the row [0, 1/3, 2/3]-type kernels:
# sums of thirds are never within 1e-3 of .5.
SHADE_ELLIPSES = {(240, 320): [(100.0, 90.0, 40.0, 25.0, 19.0), (220.0, 150.0, 30.0, 55.0, 72.0), (160.0, 120.0, 12.0, 17.0, 33.0)],
                  (67, 93): [(40.0, 30.0, 14.0, 9.0, 17.0), (60.0, 40.0, 7.0, 16.0, 71.0)],
                  # the smallest height whose shade strip takes the 16-column tile (photo_shade_lds_bytes(388, 32) > 64 KiB), one tile wide
                  (388, 16): [(8.0, 200.0, 5.0, 70.0, 19.0), (4.0, 90.0, 3.0, 40.0, 72.0)]}


def _flag_off(row):
    row[BLUR_FLAG] = 0.0
    return row


def exact_cases(H, W):
    """[(name, row)] of the exact test for an H x W image"""
    ell = SHADE_ELLIPSES[(H, W)]
    col, rw = motion_blur_weights(0.0, 0.0), motion_blur_weights(90.0, -1.0)
    return [
        ("all_off", make_row()),
        ("brightness_up", make_row(brightness=37)),
        ("brightness_down", make_row(brightness=-50)),
        ("contrast_low", make_row(contrast=0.6)),
        ("contrast_high", make_row(contrast=1.4)),
        ("blur_column", make_row(blur=col)),
        ("blur_row", make_row(blur=rw)),
        ("blur_weights_flag_off", _flag_off(make_row(blur=rw))),
        ("shade_101_positive", make_row(ellipses=ell, transparency=0.5, ksize=101)),
        ("shade_101_negative", make_row(ellipses=ell, transparency=-0.5, ksize=101)),
        ("shade_351_positive", make_row(ellipses=ell, transparency=0.8, ksize=351)),
        ("shade_351_negative", make_row(ellipses=ell, transparency=-0.5, ksize=351)),
        ("all_together", make_row(brightness=-21, contrast=1.4, blur=col, ellipses=ell, transparency=0.45, ksize=151)),
        ("all_together_no_blur", make_row(brightness=12, contrast=0.6, ellipses=ell, transparency=-0.3, ksize=125)),
    ]


def case_image(H, W, seed=0):
    """a textured float32 image in [0, 1]: a smooth ramp plus noise, so that every 8-bit level and both clips occur"""
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.45 * np.sin(xs / 17.0) * np.cos(ys / 11.0)
    return np.clip(base + 0.1 * rs.randn(H, W), 0, 1).astype(np.float32)
