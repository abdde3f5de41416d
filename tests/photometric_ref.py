"""numpy restatement of `ssp_op_photometric_apply` (csrc/photo_kernels.hip.h) for ONE image and its
row of draws, written from the stage list of the design section - a helper of tests/test_photometric_cpu.py and
tests/test_gpu_photometric.py, not a test.  The per-pixel noise stages (sigma, impulse probability) are not restated: their
random stream lives on the device and is tested statistically; a row with either set is refused here.

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


def motion_blur_weights(angle_deg, direction):
    """MotionBlur(3): the centre-column line kernel linspace(d, 1 - d, 3), d = (direction + 1) / 2, rotated bilinearly about
    the centre (zeros outside), normalised to sum 1."""
    d = (direction + 1.0) * 0.5
    line = np.zeros((3, 3))
    line[:, 1] = [d, 0.5, 1.0 - d]
    a = np.deg2rad(angle_deg)
    c, s = np.cos(a), np.sin(a)
    out = np.zeros((3, 3))
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


def apply(img, row):
    """img: float32 [H, W] in [0, 1]; row: float32 [STRIDE].  Returns (out float64 [H, W], may_differ bool [H, W]): may_differ
    marks the pixels whose pre-rounding value of an 8-bit stage lies within TIE_EPS of a .5 tie (for the 3x3 blur: or whose
    neighbourhood holds such a pixel) - an fp32 evaluation may round those the other way, by one level.
    Without the shade, float32(out) is the exact expected result."""
    img = np.asarray(img, np.float32)
    row = np.asarray(row, np.float32)
    if row[SIGMA] != 0 or row[IMPULSE_P] != 0:
        raise ValueError("the noise stages are not restated on the host")
    H, W = img.shape
    may = np.zeros((H, W), bool)
    v = np.floor(np.clip(img * np.float32(255.0), 0, 255)).astype(np.float64)         # 1 (float32 product, truncation)
    v = np.clip(v + float(row[BRIGHTNESS]), 0, 255)                                   # 2
    alpha = float(row[CONTRAST])
    if alpha != 1.0:                                                                  # 3
        pre = 127.0 + alpha * (v - 127.0)
        may |= np.abs(pre - np.floor(pre) - 0.5) < TIE_EPS
        v = np.clip(np.rint(pre), 0, 255)
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
                  (67, 93): [(40.0, 30.0, 14.0, 9.0, 17.0), (60.0, 40.0, 7.0, 16.0, 71.0)]}


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
