"""numpy restatement of the Synthetic Shapes render rules of DESIGN.md section 15 (scene table -> uint8 image and scaled points)
and the scene-table invariants of the draw.  Written from the rules, not by calling the library: only the table layout
constants and the parameter struct are shared with it."""
import numpy as np

# the scene table row (include/ssp_hip.h, SSP_SHAPES_*)
PRIM, THR, KEY, KSIZE, NBLOBS, MEAN0, MEAN, NCMDS, NPOINTS, NVERTS, NTEX = 0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11
BLOBS, CMDS, VERTS, TEX, POINTS, ROW = 16, 528, 1296, 1808, 2192, 2704
MAX_POINTS, CMD_WORDS, TEX_WORDS = 256, 12, 12
POLY, SEG, ELLIPSE, TEXPOLY, NOISE = 1, 2, 3, 4, 5
PIX_MUL = np.uint64(0xD1342543DE82EF95)
FLIP_EPS = 1e-3


def hs_mix(x):
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def key_of(words):
    return np.uint64(int(words[0]) & 0xFFFFFFFF) | (np.uint64(int(words[1]) & 0xFFFFFFFF) << np.uint64(32))


def noise(key, pix):
    """A byte in 0..254 per pixel index (cv.randu(img, 0, 255) restated)."""
    with np.errstate(over="ignore"):
        h = hs_mix(key ^ (np.asarray(pix, np.uint64) * PIX_MUL))
    return (((h >> np.uint64(32)) * np.uint64(255)) >> np.uint64(32)).astype(np.int64)


def tex_blobs(key, n, H, W, bg):
    with np.errstate(over="ignore"):
        h = hs_mix(key ^ (np.arange(1, n + 1, dtype=np.uint64) * PIX_MUL))
    x = ((h & np.uint64(0xFFFF)) * np.uint64(W)) >> np.uint64(16)
    y = (((h >> np.uint64(16)) & np.uint64(0xFFFF)) * np.uint64(H)) >> np.uint64(16)
    r = (((h >> np.uint64(32)) & np.uint64(0xFF)) * np.uint64(20)) >> np.uint64(8)
    c = ((h >> np.uint64(40)) & np.uint64(0xFF)).astype(np.int64)
    c = np.where(np.abs(c - bg) < 30, (c + 128) % 256, c)
    return x.astype(np.int64), y.astype(np.int64), r.astype(np.int64), c


def reflect101(p, n):
    """cv2.BORDER_REFLECT_101 for any distance."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    m = 2 * (n - 1)
    p = np.mod(p, m)
    return np.where(p >= n, m - p, p)


def gaussian_sigma(ksize):
    return 0.3 * ((ksize - 1) * 0.5 - 1.0) + 0.8


def gaussian_weights(ksize):
    if ksize <= 1:
        return np.ones(1, np.float32)
    s = gaussian_sigma(ksize)
    j = np.arange(ksize, dtype=np.float64) - (ksize - 1) // 2
    w = np.exp(-(j * j) / (2.0 * s * s))
    return (w / w.sum()).astype(np.float32)


def resize_taps(n_out, n_in):
    """(i0, i1, f) of INTER_LINEAR with half-pixel centres, fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    s = (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
    fl = np.floor(s)
    i0 = fl.astype(np.int64)
    f = (s - fl).astype(np.float32)
    f = np.where((i0 < 0) | (i0 >= n_in - 1), np.float32(0), f).astype(np.float32)
    i0 = np.clip(i0, 0, n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), f


def paint_circles(img, xs, ys, rs, cs):
    H, W = img.shape
    for x, y, r, c in zip(xs, ys, rs, cs):
        x0, x1, y0, y1 = max(x - r, 0), min(x + r, W - 1), max(y - r, 0), min(y + r, H - 1)
        if x1 < x0 or y1 < y0:
            continue
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        m = (xx - x) ** 2 + (yy - y) ** 2 <= r * r
        img[y0:y1 + 1, x0:x1 + 1][m] = c


def box_blur(img, k):
    """Integer window sums, anchor k // 2, reflect_101, (sum + k^2 // 2) // k^2."""
    H, W = img.shape
    a = k // 2
    ext = img[reflect101(np.arange(-a, H - a + k - 1), H)][:, reflect101(np.arange(-a, W - a + k - 1), W)].astype(np.int64)
    c = np.zeros((ext.shape[0] + 1, ext.shape[1] + 1), np.int64)
    c[1:, 1:] = ext.cumsum(0).cumsum(1)
    s = c[k:k + H, k:k + W] - c[:H, k:k + W] - c[k:k + H, :W] + c[:H, :W]
    return (s + (k * k) // 2) // (k * k)


def poly_mask(verts, H, W):
    """Integer points inside (even-odd) or on the boundary of the polygon; verts [n,2] integers."""
    v = np.asarray(verts, np.int64)
    x0, x1, y0, y1 = max(v[:, 0].min(), 0), min(v[:, 0].max(), W - 1), max(v[:, 1].min(), 0), min(v[:, 1].max(), H - 1)
    out = np.zeros((H, W), bool)
    if x1 < x0 or y1 < y0:
        return out
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    inside = np.zeros(yy.shape, bool)
    edge = np.zeros(yy.shape, bool)
    n = len(v)
    for i in range(n):
        ax, ay = v[i]
        bx, by = v[(i + 1) % n]
        cr = (xx - ax) * (by - ay) - (yy - ay) * (bx - ax)
        edge |= (cr == 0) & (xx >= min(ax, bx)) & (xx <= max(ax, bx)) & (yy >= min(ay, by)) & (yy <= max(ay, by))
        strad = (ay <= yy) != (by <= yy)
        inside ^= strad & ((cr < 0) if by > ay else (cr > 0))
    out[y0:y1 + 1, x0:x1 + 1] = inside | edge
    return out


def seg_mask(x1, y1, x2, y2, t, H, W):
    """4 d^2 <= t^2, d the distance of the integer point to the segment (round caps)."""
    h = (t + 1) // 2
    bx0, bx1, by0, by1 = max(min(x1, x2) - h, 0), min(max(x1, x2) + h, W - 1), max(min(y1, y2) - h, 0), min(max(y1, y2) + h, H - 1)
    out = np.zeros((H, W), bool)
    if bx1 < bx0 or by1 < by0:
        return out
    yy, xx = np.mgrid[by0:by1 + 1, bx0:bx1 + 1].astype(np.int64)
    ax, ay, px, py = x2 - x1, y2 - y1, xx - x1, yy - y1
    L, s = ax * ax + ay * ay, px * ax + py * ay
    cr = px * ay - py * ax
    qx, qy = xx - x2, yy - y2
    m = np.where((L == 0) | (s <= 0), 4 * (px * px + py * py) <= t * t,
                 np.where(s >= L, 4 * (qx * qx + qy * qy) <= t * t, 4 * cr * cr <= t * t * L))
    out[by0:by1 + 1, bx0:bx1 + 1] = m
    return out


def _f(word):
    return np.array([word], np.int32).view(np.float32)[0]


def ellipse_q(cmd, H, W):
    """The one float test, fp32 with every product and sum rounded: q <= 1 is inside."""
    yy, xx = np.mgrid[0:H, 0:W]
    dx, dy = (xx - int(cmd[6])).astype(np.float32), (yy - int(cmd[7])).astype(np.float32)
    co, si, ia, ib = _f(cmd[8]), _f(cmd[9]), _f(cmd[10]), _f(cmd[11])
    xr = dx * co + dy * si
    yr = dy * co - dx * si
    return (xr * xr) * ia + (yr * yr) * ib


def layer(row, which, H, W, tex_nb_blobs):
    """The blurred blob picture of the background (which = -1) or of texture `which`, over the full image."""
    if which < 0:
        pix = np.arange(H * W, dtype=np.uint64).reshape(H, W)
        img = np.where(noise(key_of(row[KEY:KEY + 2]), pix) > int(row[THR]), 255, 0).astype(np.int64)
        b = row[BLOBS:BLOBS + 4 * int(row[NBLOBS])].reshape(-1, 4).astype(np.int64)
        paint_circles(img, b[:, 0], b[:, 1], b[:, 2], b[:, 3])
        return box_blur(img, int(row[KSIZE]))
    t = row[TEX + TEX_WORDS * which:TEX + TEX_WORDS * (which + 1)]
    img = np.full((H, W), int(t[0]), np.int64)
    paint_circles(img, *tex_blobs(key_of(t[2:4]), tex_nb_blobs, H, W, int(row[MEAN])))
    return box_blur(img, int(t[1]))


def paint(row, H, W, tex_nb_blobs):
    """Steps 1-4: the full-resolution plane and the mask of pixels whose ellipse test is within FLIP_EPS of its boundary."""
    img = layer(row, -1, H, W, tex_nb_blobs)
    near = np.zeros((H, W), bool)
    verts = row[VERTS:VERTS + 512].reshape(-1, 2).astype(np.int64)
    for c in range(int(row[NCMDS])):
        cmd = row[CMDS + CMD_WORDS * c:CMDS + CMD_WORDS * (c + 1)]
        kind, col = int(cmd[0]), int(cmd[1])
        if kind == POLY:
            img[poly_mask(verts[int(cmd[6]):int(cmd[6]) + int(cmd[7])], H, W)] = col
        elif kind == SEG:
            img[seg_mask(int(cmd[6]), int(cmd[7]), int(cmd[8]), int(cmd[9]), int(cmd[10]), H, W)] = col
        elif kind == ELLIPSE:
            q = ellipse_q(cmd, H, W)
            img[q <= np.float32(1)] = col
            near |= np.abs(q.astype(np.float64) - 1.0) < FLIP_EPS
        elif kind == TEXPOLY:
            m = poly_mask(verts[int(cmd[6]):int(cmd[6]) + int(cmd[7])], H, W)
            img[m] = layer(row, int(cmd[8]), H, W, tex_nb_blobs)[m]
        elif kind == NOISE:
            img = noise(key_of(cmd[6:8]), np.arange(H * W, dtype=np.uint64).reshape(H, W))
    return img, near


def gaussian(img, ksize):
    """Separable fp32: rows first, then columns, taps ascending, product and sum rounded separately; (unrounded value)."""
    if ksize <= 1:
        return img.astype(np.float32)
    H, W = img.shape
    w, r = gaussian_weights(ksize), ksize // 2
    ext = img.astype(np.float32)[:, reflect101(np.arange(-r, W + r), W)]
    hs = np.zeros((H, W), np.float32)
    for j in range(ksize):
        hs = hs + w[j] * ext[:, j:j + W]
    ext = hs[reflect101(np.arange(-r, H + r), H)]
    v = np.zeros((H, W), np.float32)
    for i in range(ksize):
        v = v + w[i] * ext[i:i + H]
    return v


def _near_half(v):
    v = v.astype(np.float64)
    return np.abs(v - np.floor(v) - 0.5) < FLIP_EPS


def _dilate(m, r):
    if r <= 0 or not m.any():
        return m
    H, W = m.shape
    ext = np.zeros((H + 2 * r, W + 2 * r), np.int64)
    ext[r:r + H, r:r + W] = m
    c = np.zeros((ext.shape[0] + 1, ext.shape[1] + 1), np.int64)
    c[1:, 1:] = ext.cumsum(0).cumsum(1)
    k = 2 * r + 1
    return (c[k:k + H, k:k + W] - c[:H, k:k + W] - c[k:k + H, :W] + c[:H, :W]) > 0


def render(row, gen_hw, out_hw, blur_size, tex_nb_blobs=3000):
    """(image uint8 [h,w], flip mask bool [h,w], points float32 [n,2] scaled to (h, w)) of one scene table row."""
    row = np.asarray(row, np.int32)
    H, W = gen_hw
    h, w = out_hw
    plane, near = paint(row, H, W, tex_nb_blobs)
    v = gaussian(plane, blur_size)
    g = np.clip(np.rint(v), 0, 255).astype(np.float32)
    gflip = (_near_half(v) if blur_size > 1 else np.zeros((H, W), bool)) | _dilate(near, blur_size // 2)
    y0, y1, fy = resize_taps(h, H)
    x0, x1, fx = resize_taps(w, W)
    fy, fx = fy[:, None], fx[None, :]
    gy, gx = np.float32(1) - fy, np.float32(1) - fx
    top = gx * g[y0][:, x0] + fx * g[y0][:, x1]
    bot = gx * g[y1][:, x0] + fx * g[y1][:, x1]
    val = gy * top + fy * bot
    # the bilinear value can only flip where fp32 did not compute it exactly: with dyadic fractions (an integer reduction gives
    # 1/2) every product and sum is exact, a tie is then a tie for every implementation and rint's half-to-even decides it
    exact = ((gy.astype(np.float64) * (gx.astype(np.float64) * g[y0][:, x0] + fx.astype(np.float64) * g[y0][:, x1])
              + fy.astype(np.float64) * (gx.astype(np.float64) * g[y1][:, x0] + fx.astype(np.float64) * g[y1][:, x1])) == val.astype(np.float64))
    flip = (_near_half(val) & ~exact) | gflip[y0][:, x0] | gflip[y0][:, x1] | gflip[y1][:, x0] | gflip[y1][:, x1]
    n = int(row[NPOINTS])
    p = row[POINTS:POINTS + 2 * n].view(np.float32).reshape(n, 2)
    pts = np.stack([p[:, 0] * np.float32(w) / np.float32(W), p[:, 1] * np.float32(h) / np.float32(H)], 1).astype(np.float32)
    return np.clip(np.rint(val), 0, 255).astype(np.uint8), flip, pts


# ---- invariants of the draw (datasets/synthetic_dataset.py) on one table row ----
def _ccw(a, b, c):
    return (c[1] - a[1]) * (b[0] - a[0]) > (b[1] - a[1]) * (c[0] - a[0])


def segments_intersect(a, b, c, d):
    return (_ccw(a, c, d) != _ccw(b, c, d)) and (_ccw(a, b, c) != _ccw(a, b, d))


def commands(row):
    return [row[CMDS + CMD_WORDS * c:CMDS + CMD_WORDS * (c + 1)].astype(np.int64) for c in range(int(row[NCMDS]))]


def polygon_of(row, cmd):
    return row[VERTS + 2 * int(cmd[6]):VERTS + 2 * (int(cmd[6]) + int(cmd[7]))].reshape(-1, 2).astype(np.int64)


def polygon_ok(v):
    """>= 3 corners, every edge longer than 0.01, every corner angle < 2 pi / 3."""
    n = len(v)
    if n < 3:
        return False
    for i in range(n):
        a, b = (v[(i - 1) % n] - v[i]).astype(np.float64), (v[(i + 1) % n] - v[i]).astype(np.float64)
        na, nb = np.linalg.norm(a), np.linalg.norm(b)
        if not (na > 0.01 and nb > 0.01):
            return False
        if not np.arccos(np.clip(np.dot(a / na, b / nb), -1.0, 1.0)) < 2 * np.pi / 3:
            return False
    return True


def check_row(row, p):
    """Raises AssertionError when a table row breaks a rule of the reference's generator.  p: the parameter struct."""
    row = np.asarray(row, np.int32)
    H, W = p.gen_h, p.gen_w
    prim, bg, md = int(row[PRIM]), int(row[MEAN]), min(H, W)
    cmds = commands(row)
    n = int(row[NPOINTS])
    pts = row[POINTS:POINTS + 2 * n].view(np.float32).reshape(n, 2)
    assert 0 <= prim < 9 and 0 <= int(row[THR]) < 256 and p.bg_min_kernel <= int(row[KSIZE]) < p.bg_max_kernel
    assert ((pts[:, 0] >= 0) & (pts[:, 0] < W) & (pts[:, 1] >= 0) & (pts[:, 1] < H)).all(), "key point outside the image"
    contrast = lambda c: abs(int(c) - bg) >= 30  # noqa: E731  get_random_color

    def thick(lines, lo, hi):  # randint(md * lo, md * hi), at least 1 (deviation d)
        a, b = max(int(md * lo), 1), max(int(md * hi), int(md * lo) + 1, 2)
        return len({int(c[10]) for c in lines}) <= 1 and all(a <= c[10] < b for c in lines)

    blobs = row[BLOBS:BLOBS + 4 * int(row[NBLOBS])].reshape(-1, 4)
    dim = max(H, W)
    assert (np.abs(blobs[:, 3].astype(int) - int(row[MEAN0])) >= 30).all()
    assert ((blobs[:, 2] >= int(dim * p.bg_min_rad_ratio)) & (blobs[:, 2] < max(int(dim * p.bg_max_rad_ratio), int(dim * p.bg_min_rad_ratio) + 1))).all()
    if prim == 0:
        assert 1 <= len(cmds) < p.lines_nb_lines and n == 2 * len(cmds)
        for i, a in enumerate(cmds):
            assert a[0] == SEG and contrast(a[1]) and max(int(md * 0.01), 1) <= a[10] < max(int(md * 0.02), 2)
            for b in cmds[:i]:
                assert not segments_intersect(a[6:8], a[8:10], b[6:8], b[8:10]), "lines intersect"
    elif prim == 1:
        assert len(cmds) == 1 and cmds[0][0] == POLY and contrast(cmds[0][1])
        v = polygon_of(row, cmds[0])
        assert polygon_ok(v) and len(v) < p.polygon_max_sides and n == len(v)
    elif prim == 2:
        assert len(cmds) == int(row[NTEX]) <= p.multi_nb_polygons
        polys = [polygon_of(row, c) for c in cmds]
        tex = [row[TEX + TEX_WORDS * t:TEX + TEX_WORDS * (t + 1)] for t in range(len(cmds))]
        assert n == sum(len(v) for v in polys)
        for i, (c, v, t) in enumerate(zip(cmds, polys, tex)):
            assert c[0] == TEXPOLY and c[8] == i and contrast(t[0]) and polygon_ok(v) and len(v) < p.multi_max_sides
            assert p.multi_kernel_lo <= int(t[1]) < p.multi_kernel_hi
            ci, ri = np.array([int(t[4]), int(t[5])], np.float64), float(_f(t[6]))
            for j in range(i):
                u, tj = polys[j], tex[j]
                for e in range(len(v)):
                    for f in range(len(u)):
                        assert not segments_intersect(v[e], v[(e + 1) % len(v)], u[f], u[(f + 1) % len(u)]), "polygons intersect"
                cj, rj = np.array([int(tj[4]), int(tj[5])], np.float64), float(_f(tj[6]))
                assert not (np.linalg.norm(ci - cj) + min(ri, rj) < max(ri, rj)), "polygons nest (overlap rule)"
    elif prim == 3:
        assert n == 0 and len(cmds) <= p.ellipses_nb
        for i, a in enumerate(cmds):
            assert a[0] == ELLIPSE and contrast(a[1])
            ra = int(row[VERTS + i])
            assert ra == max(round(float(_f(a[10])) ** -0.5), round(float(_f(a[11])) ** -0.5)), "stored max_rad differs from the command's axes"
            assert ra <= a[6] < max(W - ra, ra + 1) and ra <= a[7] < max(H - ra, ra + 1)
            if i:  # :322-324 broadcasts (n,) - (n, 1) to n x n: the nearest previous centre against the LARGEST previous radius
                dmin = min(np.sqrt(float((a[6] - b[6]) ** 2 + (a[7] - b[7]) ** 2)) for b in cmds[:i])
                assert not ra > dmin - max(int(row[VERTS + j]) for j in range(i)), "ellipses too close"
    elif prim == 4:
        assert 3 <= len(cmds) < p.star_nb_branches and n == len(cmds) + 1
        assert all(a[0] == SEG and contrast(a[1]) and (a[6], a[7]) == (cmds[0][6], cmds[0][7]) for a in cmds) and thick(cmds, 0.01, 0.02)
    elif prim == 5:
        cells = [a for a in cmds if a[0] == POLY]
        lines = [a for a in cmds if a[0] == SEG]
        assert 9 <= len(cells) <= (p.checker_max_rows - 1) * (p.checker_max_cols - 1) and 4 <= len(lines) and contrast(cells[0][1])
        assert all(contrast(a[1]) for a in lines) and n <= p.checker_max_rows * p.checker_max_cols and thick(lines, 0.01, 0.015)
        # nb_rows = randint(2, rows + 2), nb_cols = randint(2, cols + 2): at most rows + 1 + cols + 1 lines, rows * cols = len(cells)
        assert any(r * (len(cells) // r) == len(cells) and len(lines) <= r + len(cells) // r + 2
                   for r in range(3, p.checker_max_rows) if 3 <= len(cells) // r < p.checker_max_cols)
    elif prim == 6:
        cells = [a for a in cmds if a[0] == POLY]
        lines = [a for a in cmds if a[0] == SEG]
        assert len(cells) < p.stripes_max_nb_cols and 4 <= len(lines) and all(contrast(a[1]) for a in lines) and n <= 2 * (len(cells) + 1)
        assert len(lines) <= 4 + len(cells) + 1 and thick(lines, 0.01, 0.015)  # nb_rows = randint(2, 5), nb_cols = randint(2, col + 2)
    elif prim == 7:
        assert n <= 7 and len(cmds) == 15 and [int(a[0]) for a in cmds] == [POLY] * 3 + [SEG] * 12 and contrast(cmds[0][1])
        assert thick(cmds[3:], 0.003, 0.015)
        for a in cmds[3:]:
            assert 64 <= (int(a[1]) - int(cmds[0][1])) % 256 < 192  # (col_face + 128 + randint(-64, 64)) % 256
    else:
        assert n == 0 and len(cmds) == 1 and cmds[0][0] == NOISE


# ---- the small case of the exact tests: 192x256 -> 24x32, blur_size 5 (kernel sizes scaled with the image) ----
SMALL = {"generation": {"image_size": [192, 256],
                        "params": {"generate_background": {"min_kernel_size": 30, "max_kernel_size": 100},
                                   "draw_multiple_polygons": {"kernel_boundaries": [10, 20], "nb_blobs": 600}}},
         "preprocessing": {"resize": [24, 32], "blur_size": 5}}
SMALL_TEX_BLOBS = 600
FIXTURE_SEEDS = {"mixed_a": 11, "mixed_b": 12}  # two mixed batches of 4; "prim<k>": one image of primitive k, seed 100 + k


def small_config(data, primitive=None):
    """The fixture's `data:` block at the small size; primitive: only that one."""
    d = dict(data, **SMALL)
    if primitive is not None:
        d["primitives"] = [primitive]
    return d
