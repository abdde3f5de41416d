"""numpy restatement of the Synthetic Shapes render rules of DESIGN.md section 15 (scene table -> uint8 image and scaled points)
and the scene-table invariants of the draw, and (`draw`, below) of the draw itself in the order of
datasets/synthetic_dataset.py on the device stream.  Written from the rules, not by calling the library: only the table layout
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


# ------------------------------------------------------------------------------------------------------------------
# The draw (ssp_op_shapes_draw) restated in the order of datasets/synthetic_dataset.py: generate_background and the nine
# primitives on the device stream, with the stated deviations (a)-(e) of DESIGN.md section 15.  Integer words compare with ==.
# ------------------------------------------------------------------------------------------------------------------
SHAPES_TAG, BG_TAG, TEX_TAG, NOISE_TAG = 0x7368617065733135, 0x6261636B67726E64, 0x7465787475726573, 0x6E6F697365
MAX_BLOBS, MAX_CMDS, MAX_VERTS, MAX_TEX, COORD_MAX = 128, 64, 256, 32, 16383
TWO_PI = 6.283185307179586
DRAW_MUTANTS = ("blob_y_first", "ri_inclusive", "poly_rad_fifth", "centre_x_from_h", "poly_min_03", "filters_once", "overlap_swapped",
                "ellipse_nearest_radius", "persp_alpha", "affine_rows_swapped", "divide_first", "checker_s_w", "stripes_no_unique",
                "cube_faces_order", "cube_edge_30", "mean_after_blur")
# the primitive (index into lib.SHAPES_PRIMITIVES) whose tables can show each mutant; None: every primitive (background)
MUTANT_PRIMITIVE = {"blob_y_first": None, "ri_inclusive": None, "poly_rad_fifth": 1, "centre_x_from_h": 1, "poly_min_03": 1,
                    "filters_once": 2, "overlap_swapped": 2, "ellipse_nearest_radius": 3, "persp_alpha": 5, "affine_rows_swapped": 5,
                    "divide_first": 5, "checker_s_w": 5, "stripes_no_unique": 6, "cube_faces_order": 7, "cube_edge_30": 7,
                    "mean_after_blur": None}


def _fbits(x):
    return int(np.array([x], np.float32).view(np.int32)[0])


def solve_pivoted(A):
    """n x n system [A | b] by Gauss-Jordan elimination with partial pivoting in float64 (deviation e): Python floats."""
    A = [[float(v) for v in r] for r in A]
    n = len(A)
    for c in range(n):
        piv = c
        for r in range(c + 1, n):
            if abs(A[r][c]) > abs(A[piv][c]):
                piv = r
        A[c], A[piv] = A[piv], A[c]
        d = A[c][c]
        for r in range(n):
            if r == c:
                continue
            f = A[r][c] / d
            for k in range(c, n + 1):
                A[r][k] -= f * A[c][k]
    return [A[i][n] / A[i][i] for i in range(n)]


class _Draw:
    def __init__(self, seed, n, p, mutant):
        from tests.pairs_ref import M64, DeviceStream, mix
        self.mix, self.M64 = mix, M64
        self.rs = DeviceStream(mix((int(seed) ^ SHAPES_TAG) & M64), n)
        self.p, self.mutant = p, mutant
        self.H, self.W = int(p.gen_h), int(p.gen_w)
        self.row = np.zeros(ROW, np.int32)
        self.ncmd = self.nvert = self.npts = self.ntex = 0
        self.margin = np.inf
        self.dev = set()
        self.events = []          # what the reference's cv2 calls would receive, in order (section D)

    # ---- the stream
    def note(self, x):
        self.margin = min(self.margin, abs(float(x)))

    def u(self):
        return self.rs.uniform()

    def ri(self, lo, hi):
        """np.random.randint(lo, hi): [lo, hi); an empty range gives lo (deviation d) and still consumes its uniform"""
        n = hi - lo + (1 if self.mutant == "ri_inclusive" else 0)
        if n <= 1:
            self.u()
            if n < 1:
                self.dev.add("d")
            return lo
        v = lo + self.rs.randint(n)
        self.margin = min(self.margin, self.rs.margin)
        return v

    def color(self, bg):
        c = self.ri(0, 256)
        return (c + 128) % 256 if abs(c - bg) < 30 else c

    def toi(self, v):
        """int(): truncation toward zero, clamped to +-COORD_MAX; the margin is the distance from the nearest integer"""
        self.note(v - np.rint(v))
        return int(max(-float(COORD_MAX), min(float(COORD_MAX), v)))

    def trunc(self, v):
        self.note(v - np.rint(v))
        return int(v)

    # ---- the table
    def cmd(self, kind, col):
        if self.ncmd >= MAX_CMDS:
            return None
        c = CMDS + CMD_WORDS * self.ncmd
        self.ncmd += 1
        self.row[c], self.row[c + 1] = kind, col
        return c

    def bbox(self, c, x0, y0, x1, y1):
        self.row[c + 2:c + 6] = (max(x0, 0), max(y0, 0), min(x1, self.W - 1), min(y1, self.H - 1))

    def seg(self, col, x1, y1, x2, y2, t):
        if t < 1:
            self.dev.add("d")
        self.events.append(("line", (x1, y1), (x2, y2), col, t))
        t = max(t, 1)
        c = self.cmd(SEG, col)
        if c is None:
            return
        h = (t + 1) // 2
        self.bbox(c, min(x1, x2) - h, min(y1, y2) - h, max(x1, x2) + h, max(y1, y2) + h)
        self.row[c + 6:c + 12] = (x1, y1, x2, y2, t, 0)

    def poly(self, kind, col, pts):
        n = len(pts)
        if self.nvert + n > MAX_VERTS:
            return None
        c = self.cmd(kind, col)
        if c is None:
            return None
        self.events.append(("fillPoly", [tuple(q) for q in pts], col))
        v = np.asarray(pts, np.int64)
        self.row[VERTS + 2 * self.nvert:VERTS + 2 * (self.nvert + n)] = v.reshape(-1)
        self.bbox(c, v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max())
        self.row[c + 6:c + 12] = (self.nvert, n, 0, 0, 0, 0)
        self.nvert += n
        return c

    def point(self, x, y):
        if self.npts >= MAX_POINTS:
            return
        self.row[POINTS + 2 * self.npts], self.row[POINTS + 2 * self.npts + 1] = _fbits(float(x)), _fbits(float(y))
        self.npts += 1

    def point_inside(self, x, y):
        if 0 <= x < self.W and 0 <= y < self.H:
            self.point(x, y)

    def segments(self):
        out = []
        for c in range(self.ncmd):
            q = self.row[CMDS + CMD_WORDS * c:CMDS + CMD_WORDS * (c + 1)]
            out.append(q)
        return out

    # ---- generate_background :52-79
    def background(self):
        p, H, W = self.p, self.H, self.W
        row = self.row
        tot = sum(float(w) for w in p.weights)
        r = self.u() * tot
        prim, acc = 8, 0.0
        for i in range(9):
            acc += float(p.weights[i])
            self.note(r - acc)
            if r < acc:
                prim = i
                break
        while prim > 0 and not p.weights[prim] > 0:
            prim -= 1
        row[PRIM] = prim
        key = self.mix(self.rs.key ^ BG_TAG)
        row[KEY], row[KEY + 1] = np.array([key & 0xFFFFFFFF, key >> 32], np.uint32).view(np.int32)
        row[THR] = self.ri(0, 256)
        nb = int(p.bg_nb_blobs)
        row[NBLOBS] = nb
        xs = [self.ri(0, W) for _ in range(nb)] if self.mutant != "blob_y_first" else None
        ys = [self.ri(0, H) for _ in range(nb)]
        if xs is None:
            xs = [self.ri(0, W) for _ in range(nb)]
        row[BLOBS:BLOBS + 4 * nb:4], row[BLOBS + 1:BLOBS + 4 * nb:4] = xs, ys
        img = np.where(noise(np.uint64(key), np.arange(H * W, dtype=np.uint64).reshape(H, W)) > int(row[THR]), 255, 0).astype(np.int64)
        mean0 = int(img.sum()) // (H * W)            # int(np.mean(img)): the image holds 0 and 255 only, the integer quotient is exact
        row[MEAN0] = mean0
        dim = max(H, W)
        for i in range(nb):
            row[BLOBS + 4 * i + 3] = self.color(mean0)
            row[BLOBS + 4 * i + 2] = self.ri(int(dim * float(p.bg_min_rad_ratio)), int(dim * float(p.bg_max_rad_ratio)))
        row[KSIZE] = self.ri(int(p.bg_min_kernel), int(p.bg_max_kernel))
        b = row[BLOBS:BLOBS + 4 * nb].reshape(-1, 4).astype(np.int64)
        paint_circles(img, b[:, 0], b[:, 1], b[:, 2], b[:, 3])
        self.plane = img
        mean = int(img.sum()) // (H * W)             # deviation (a): before the box blur
        if self.mutant == "mean_after_blur":
            mean = int(box_blur(img, int(row[KSIZE])).sum()) // (H * W)
        row[MEAN] = mean
        return prim, mean

    def mean_after_blur(self):
        return int(box_blur(self.plane, int(self.row[KSIZE])).sum()) // (self.H * self.W)

    # ---- the corner sampler of draw_polygon :172-199 / draw_multiple_polygons :240-268
    def sample_polygon(self, max_sides):
        H, W, m = self.H, self.W, self.mutant
        n = min(self.ri(3, max_sides), 16)
        md = float(min(H, W))
        lo = md / 5 if m == "poly_rad_fifth" else md / 10
        ur = self.u() * md / 2
        rad = max(ur, lo)
        if ur > lo:
            self.note(rad - np.rint(rad))
            self.note((W - rad) - np.rint(W - rad))
            self.note((H - rad) - np.rint(H - rad))
        cx = self.ri(int(rad), int((H if m == "centre_x_from_h" else W) - rad))
        cy = self.ri(int(rad), int(H - rad))
        ang = []
        for i in range(n):
            s0, s1 = TWO_PI * i / n, TWO_PI * (i + 1) / n
            ang.append(s0 + self.u() * (s1 - s0))
        fmin = 0.3 if m == "poly_min_03" else 0.4
        pts = []
        for a in ang:
            fx, fy = max(self.u(), fmin), max(self.u(), fmin)
            pts.append([self.toi(cx + fx * rad * np.cos(a)), self.toi(cy + fy * rad * np.sin(a))])
        for pas in range(16):
            k = len(pts)
            kept = [pts[i] for i in range(k) if pts[(i - 1) % k] != pts[i]]
            removed = k - len(kept)
            pts, k = kept, len(kept)
            keep = []
            for i in range(k):
                a = (pts[(i - 1) % k][0] - pts[i][0], pts[(i - 1) % k][1] - pts[i][1])
                b = (pts[(i + 1) % k][0] - pts[i][0], pts[(i + 1) % k][1] - pts[i][1])
                na, nb = np.sqrt(float(a[0] * a[0] + a[1] * a[1])), np.sqrt(float(b[0] * b[0] + b[1] * b[1]))
                ok = na > 0 and nb > 0
                if ok:
                    t = np.arccos(max(-1.0, min(1.0, (a[0] / na) * (b[0] / nb) + (a[1] / na) * (b[1] / nb))))
                    self.note(t - TWO_PI / 3)
                    ok = t < TWO_PI / 3
                keep.append(ok)
            kept = [q for q, ok in zip(pts, keep) if ok]
            removed += k - len(kept)
            pts = kept
            if pas >= 1 and removed:
                self.dev.add("b")
            if removed == 0 or len(pts) < 3 or m == "filters_once":
                break
        return pts, cx, cy, rad

    # ---- the affine + perspective pair of draw_checkerboard :379-398 / draw_stripes :512-531
    def sample_warp(self, tp):
        H, W, m = self.H, self.W, self.mutant
        self.dev.add("e")
        alpha = float(max(H, W)) * (float(tp[0]) + self.u() * float(tp[1]))
        c0, c1, sq = float(H // 2), float(W // 2), float(min(H, W) // 3)      # np.float32(img.shape) // 2: (H, W) as written
        p1 = [(c0 + sq, c1 + sq), (c0 + sq, c1 - sq), (c0 - sq, c1 - sq), (c0 - sq, c1 + sq)]
        f32 = lambda v: float(np.float32(v))  # noqa: E731
        p2 = [[f32(p1[i][j] + f32(-alpha + self.u() * 2.0 * alpha)) for j in range(2)] for i in range(4)]
        self.a = []
        for r in ((1, 0) if m == "affine_rows_swapped" else (0, 1)):
            self.a += solve_pivoted([[p1[i][0], p1[i][1], 1.0, p2[i][r]] for i in range(3)])
        if m == "persp_alpha":
            p2 = [[f32(p1[i][j] + f32(-alpha + self.u() * 2.0 * alpha)) for j in range(2)] for i in range(4)]
        else:
            p2 = [[f32(p1[i][j] + f32(-alpha / 2 + self.u() * alpha)) for j in range(2)] for i in range(4)]
        A = []
        for k in range(4):
            (x, y), (uu, v) = p1[k], p2[k]
            A.append([x, y, 1, 0, 0, 0, -uu * x, -uu * y, uu])
            A.append([0, 0, 0, x, y, 1, -v * x, -v * y, v])
        self.pm = solve_pivoted(A) + [1.0]

    def warp(self, x, y):
        a, p = self.a, self.pm
        ax, ay = a[0] * x + a[1] * y + a[2], a[3] * x + a[4] * y + a[5]
        z = ax * p[6] + ay * p[7] + p[8]
        if self.mutant == "divide_first":
            return self.toi((ax / z) * p[0] + (ay / z) * p[1] + p[2]), self.toi((ax / z) * p[3] + (ay / z) * p[4] + p[5])
        return self.toi((ax * p[0] + ay * p[1] + p[2]) / z), self.toi((ax * p[3] + ay * p[4] + p[5]) / z)

    def thickness(self, lo, hi):
        md = min(self.H, self.W)
        return self.ri(int(md * lo), int(md * hi))

    # ---- the nine primitives
    def primitive(self, prim, bg):
        p, H, W, m, row = self.p, self.H, self.W, self.mutant, self.row
        md = min(H, W)
        self.start_ctr = self.rs.ctr
        if prim == 0:                                                     # draw_lines :138-163
            for _ in range(self.ri(1, int(p.lines_nb_lines))):
                s = [self.ri(0, W), self.ri(0, H), self.ri(0, W), self.ri(0, H)]
                if any(segments_intersect(q[6:8].astype(np.int64), q[8:10].astype(np.int64), s[0:2], s[2:4]) for q in self.segments()):
                    continue
                col = self.color(bg)
                self.seg(col, s[0], s[1], s[2], s[3], self.thickness(0.01, 0.02))
                self.point(s[0], s[1])
                self.point(s[2], s[3])
        elif prim == 1:                                                   # draw_polygon :166-206, the recursion as a loop (c)
            for attempt in range(64):
                pts, _, _, _ = self.sample_polygon(int(p.polygon_max_sides))
                if len(pts) < 3:
                    continue
                self.poly(POLY, self.color(bg), pts)
                for q in pts:
                    self.point(q[0], q[1])
                break
            else:
                self.dev.add("c")
        elif prim == 2:                                                   # draw_multiple_polygons :227-301
            for _ in range(int(p.multi_nb_polygons)):
                if self.ntex >= MAX_TEX:
                    break
                pts, cx, cy, rad = self.sample_polygon(int(p.multi_max_sides))
                n = len(pts)
                if n < 3:
                    continue
                hit = False
                for q in self.segments():
                    v = row[VERTS + 2 * int(q[6]):VERTS + 2 * (int(q[6]) + int(q[7]))].reshape(-1, 2).astype(np.int64)
                    for e in range(len(v)):
                        for g in range(n):
                            if segments_intersect(v[e], v[(e + 1) % len(v)], pts[g], pts[(g + 1) % n]):
                                hit = True
                                break
                        if hit:
                            break
                    if hit:
                        break
                for t in range(self.ntex):                                # overlap :209-217
                    if hit:
                        break
                    q = row[TEX + TEX_WORDS * t:TEX + TEX_WORDS * (t + 1)]
                    r2 = float(_f(q[6]))
                    d = np.sqrt(float((cx - int(q[4])) ** 2 + (cy - int(q[5])) ** 2))
                    lhs, rhs = d + min(rad, r2), max(rad, r2)
                    if m == "overlap_swapped":
                        lhs, rhs = d + max(rad, r2), min(rad, r2)
                    self.note(lhs - rhs)
                    hit = lhs < rhs
                if hit:
                    continue
                base = self.color(bg)
                c = self.poly(TEXPOLY, base, pts)
                if c is None:
                    break
                row[c + 8] = self.ntex
                q = TEX + TEX_WORDS * self.ntex
                self.ntex += 1
                key = self.mix(self.rs.key ^ ((TEX_TAG + self.rs.ctr) & self.M64))
                self.rs.ctr += 1                                          # the texture key consumes a counter value
                row[q] = base
                row[q + 1] = self.ri(int(p.multi_kernel_lo), int(p.multi_kernel_hi))
                row[q + 2], row[q + 3] = np.array([key & 0xFFFFFFFF, key >> 32], np.uint32).view(np.int32)
                row[q + 4], row[q + 5], row[q + 6] = cx, cy, _fbits(rad)
                row[q + 7:q + 11] = row[c + 2:c + 6]
                for g in pts:
                    self.point(g[0], g[1])
        elif prim == 3:                                                   # draw_ellipses :304-331
            q4 = float(md) / 4

            def axis():
                x = self.u() * q4
                if x > q4 / 5:
                    self.note(x - np.rint(x))
                return int(max(x, q4 / 5))
            for _ in range(int(p.ellipses_nb)):
                ax, ay = axis(), axis()
                mr = max(ax, ay)
                x, y = self.ri(mr, W - mr), self.ri(mr, H - mr)
                cmds = self.segments()
                if cmds:
                    # (n,) - (n, 1) broadcasts to n x n: ANY pair (distance i, radius j), i.e. the nearest centre against the largest
                    # radius.  max_rad > sqrt(d2) - r  <=>  (max_rad + r)^2 > d2 in integers (both sides are non-negative)
                    d2 = [(int(q[6]) - x) ** 2 + (int(q[7]) - y) ** 2 for q in cmds]
                    rads = [int(row[VERTS + c]) for c in range(len(cmds))]
                    if m == "ellipse_nearest_radius":
                        hit = (mr + rads[int(np.argmin(d2))]) ** 2 > min(d2)
                    else:
                        hit = (mr + max(rads)) ** 2 > min(d2)
                    if hit:
                        continue
                col = self.color(bg)
                deg = self.u() * 90.0
                ang = deg * (3.141592653589793 / 180.0)
                c = self.cmd(ELLIPSE, col)
                if c is None:
                    break
                self.events.append(("ellipse", (x, y), (ax, ay), deg, col))
                row[VERTS + self.ncmd - 1] = mr
                self.bbox(c, x - mr, y - mr, x + mr, y + mr)
                one = np.float32(1)
                ia = one / np.float32(ax * ax) if ax > 0 else np.float32(0)
                ib = one / np.float32(ay * ay) if (ay > 0 and ax > 0) else np.float32(3.0e38)
                row[c + 6:c + 12] = (x, y, _fbits(np.cos(ang)), _fbits(np.sin(ang)), _fbits(ia), _fbits(ib))
        elif prim == 4:                                                   # draw_star :334-359
            nb = min(self.ri(3, int(p.star_nb_branches)), 16)
            t = self.thickness(0.01, 0.02)
            ur = self.u() * md / 2
            rad = max(ur, md / 5)
            if ur > md / 5:
                self.note(rad - np.rint(rad))
                self.note((W - rad) - np.rint(W - rad))
                self.note((H - rad) - np.rint(H - rad))
            x, y = self.ri(int(rad), int(W - rad)), self.ri(int(rad), int(H - rad))
            ang = []
            for i in range(nb):
                s0, s1 = TWO_PI * i / nb, TWO_PI * (i + 1) / nb
                ang.append(s0 + self.u() * (s1 - s0))
            pts = []
            for a in ang:
                fx, fy = max(self.u(), 0.3), max(self.u(), 0.3)
                pts.append((self.toi(x + fx * rad * np.cos(a)), self.toi(y + fy * rad * np.sin(a))))
            self.point(x, y)
            for q in pts:
                self.seg(self.color(bg), x, y, q[0], q[1], t)
                self.point(q[0], q[1])
        elif prim == 5:                                                   # draw_checkerboard :362-478
            rows, cols = min(self.ri(3, int(p.checker_max_rows)), 6), min(self.ri(3, int(p.checker_max_cols)), 6)
            s = (W - 1) // cols if m == "checker_s_w" else min((W - 1) // cols, (H - 1) // rows)
            self.sample_warp(p.checker_transform)
            wp = [self.warp(float(s * j), float(s * i)) for i in range(rows + 1) for j in range(cols + 1)]
            colors = {}
            for i in range(rows):
                for j in range(cols):
                    if i == 0 and j == 0:
                        col = self.color(bg)
                    else:                                                 # get_different_color :24-37
                        near = ([colors[(i - 1, j)]] if i else []) + ([colors[(i, j - 1)]] if j else [])
                        col = self.ri(0, 256)
                        count = 0
                        while any(abs(c - col) < 50 for c in near) and count < 20:
                            count += 1
                            col = self.ri(0, 256)
                    colors[(i, j)] = col
                    a, b = i * (cols + 1) + j, (i + 1) * (cols + 1) + j
                    self.poly(POLY, col, [wp[a], wp[a + 1], wp[b + 1], wp[b]])
            nb_rows, nb_cols = self.ri(2, rows + 2), self.ri(2, cols + 2)
            t = self.thickness(0.01, 0.015)
            for _ in range(nb_rows):
                r, c1, c2 = self.ri(0, rows + 1), self.ri(0, cols + 1), self.ri(0, cols + 1)
                col = self.color(bg)
                self.seg(col, *wp[r * (cols + 1) + c1], *wp[r * (cols + 1) + c2], t)
            for _ in range(nb_cols):
                c, r1, r2 = self.ri(0, cols + 1), self.ri(0, rows + 1), self.ri(0, rows + 1)
                col = self.color(bg)
                self.seg(col, *wp[r1 * (cols + 1) + c], *wp[r2 * (cols + 1) + c], t)
            for q in wp:
                self.point_inside(q[0], q[1])
        elif prim == 6:                                                   # draw_stripes :481-593
            bh, bw = self.trunc(H * (1 + self.u())), self.trunc(W * (1 + self.u()))
            col = min(self.ri(5, int(p.stripes_max_nb_cols)), 14)
            cs = sorted([self.trunc(bw * self.u()) for _ in range(col - 1)] + [0, bw - 1])
            if m != "stripes_no_unique":
                cs = sorted(set(cs))                                      # np.unique
            min_width = float(md) * float(p.stripes_min_width_ratio)
            kept = []
            for i, c in enumerate(cs):
                nxt = float(cs[i + 1]) if i + 1 < len(cs) else float(bw) + min_width
                self.note(nxt - c - min_width)
                if nxt - c >= min_width:
                    kept.append(c)
            col = len(kept) - 1
            self.sample_warp(p.stripes_transform)
            wp = [None] * (2 * (col + 1))
            for i, c in enumerate(kept):
                wp[i] = self.warp(float(c), 0.0)
                wp[i + col + 1] = self.warp(float(c), float(bh - 1))
            color = self.color(bg)
            for i in range(col):
                color = (color + 128 + self.ri(-30, 30)) % 256
                self.poly(POLY, color, [wp[i], wp[i + 1], wp[i + col + 2], wp[i + col + 1]])
            nb_rows, nb_cols = self.ri(2, 5), self.ri(2, col + 2)
            t = self.thickness(0.01, 0.015)
            for _ in range(nb_rows):
                uu = self.u()
                self.note(uu - 0.5)
                r = 0 if uu < 0.5 else col + 1
                c1, c2 = self.ri(0, col + 1), self.ri(0, col + 1)
                color = self.color(bg)
                self.seg(color, *wp[r + c1], *wp[r + c2], t)
            for _ in range(nb_cols):
                c = self.ri(0, col + 1)
                color = self.color(bg)
                self.seg(color, *wp[c], *wp[c + col + 1], t)
            for q in wp:
                self.point_inside(q[0], q[1])
        elif prim == 7:                                                   # draw_cube :596-680
            fmd = float(md)
            min_side = fmd * float(p.cube_min_size_ratio)
            l = [min_side + self.u() * 2 * fmd / 3 for _ in range(3)]
            ra = [self.u() * 3 * 3.141592653589793 / 10. + 3.141592653589793 / 10. for _ in range(3)]
            sc = [float(p.cube_scale[0]) + self.u() * float(p.cube_scale[1]) for _ in range(3)]
            t0, t1 = float(p.cube_trans[0]), float(p.cube_trans[1])
            tx = W * t0 + self.ri(int(-W * t1), int(W * t1))
            ty = H * t0 + self.ri(int(-H * t1), int(H * t1))
            cube = []
            for v in range(8):
                x, y, z = (l[0] if v & 1 else 0.0), (l[1] if v & 2 else 0.0), (l[2] if v & 4 else 0.0)
                x3, z3 = np.cos(ra[2]) * x - np.sin(ra[2]) * z, np.sin(ra[2]) * x + np.cos(ra[2]) * z        # rotation_3
                y2 = np.cos(ra[1]) * y - np.sin(ra[1]) * z3                                                  # rotation_2
                x1, y1 = np.cos(ra[0]) * x3 - np.sin(ra[0]) * y2, np.sin(ra[0]) * x3 + np.cos(ra[0]) * y2    # rotation_1
                if v == 0 and tx == np.rint(tx) and ty == np.rint(ty):
                    cube.append((int(tx), int(ty)))                       # the hidden corner is the translation itself: an exact integer
                    continue
                cube.append((self.toi(tx + sc[0] * x1), self.toi(ty + sc[1] * y1)))
            faces = [[7, 3, 1, 5], [7, 5, 4, 6], [7, 6, 2, 3]]
            if m == "cube_faces_order":
                faces = [faces[1], faces[0], faces[2]]
            col_face = self.color(bg)
            for f in faces:
                self.poly(POLY, col_face, [cube[j] for j in f])
            t = self.thickness(0.003, 0.015)
            for f in faces:
                for j in range(4):
                    col_edge = (col_face + 128 + (self.ri(-30, 30) if m == "cube_edge_30" else self.ri(-64, 64))) % 256
                    a, b = f[j], f[(j + 1) % 4]
                    self.seg(col_edge, *cube[a], *cube[b], t)
            for v in range(1, 8):
                self.point_inside(*cube[v])
        else:                                                             # gaussian_noise :683-686
            c = self.cmd(NOISE, 0)
            key = self.mix(self.rs.key ^ NOISE_TAG)
            self.bbox(c, 0, 0, W - 1, H - 1)
            row[c + 6], row[c + 7] = np.array([key & 0xFFFFFFFF, key >> 32], np.uint32).view(np.int32)
        row[NCMDS], row[NPOINTS], row[NVERTS], row[NTEX] = self.ncmd, self.npts, self.nvert, self.ntex


def draw(seed, n, p, mutant=None, deviation_a=False, full=False):
    """Row n of ssp_op_shapes_draw(B, seed, p): (row int32 [ROW], margin, deviations).  p: the parameter struct (its floats are
    float32 values).  margin: the smallest distance from its boundary of any decision taken on a float (every truncation, every
    u < x, the polygon's angle test, the overlap rule, the stripes' width test).  deviations: which of (a)-(e) of DESIGN.md
    section 15 changed something for this table; (a) costs a box blur and is only evaluated with deviation_a=True; (e) is
    named whenever the solvers ran.  full=True returns the _Draw object (events, counter positions) for section D."""
    assert mutant is None or mutant in DRAW_MUTANTS, mutant
    d = _Draw(seed, n, p, mutant)
    prim, bg = d.background()
    if deviation_a and d.mean_after_blur() != bg:
        d.dev.add("a")
    d.bg = bg
    d.primitive(prim, bg)
    return d if full else (d.row, d.margin, frozenset(d.dev))


def float_words(row):
    """Indices of the row's words that hold float bits cast from a double through libm (the ellipse's cos / sin): the device's
    may be the float32 neighbour.  Key points, the texture radius and 1/ax^2, 1/ay^2 are exact and compare with ==."""
    row = np.asarray(row)
    if int(row[PRIM]) != 3:
        return []
    return [CMDS + CMD_WORDS * c + k for c in range(int(row[NCMDS])) for k in (8, 9)]
