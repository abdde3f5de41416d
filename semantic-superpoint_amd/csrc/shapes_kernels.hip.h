// Synthetic Shapes on the device: the generator of the MagicPoint stage,
//   datasets/synthetic_dataset.py            generate_background + the nine primitives (sampling logic restated)
//   datasets/SyntheticDataset_gaussian.py    dump_primitive_data :125-147 (GaussianBlur, point scaling, INTER_LINEAR resize)
// as two operators: shapes_draw_kernel writes one scene table row (SH_ROW int32 words) per image - every random decision -
// and the render kernels are a pure function of the row and the parameters.
//
// Raster rules (this project's own, cv2 is not available to compare against; DESIGN.md section 15 states them in full):
//   * pixel (x, y) is painted when the integer point (x, y) is inside the shape or on its boundary;
//   * polygon: even-odd crossing rule in integer arithmetic, plus the points on an edge;
//   * thick segment: 4 d^2 <= t^2 with d the distance to the segment (round caps), in 64-bit integers;
//   * circle: dx^2 + dy^2 <= r^2;
//   * ellipse: the one float test, op order fixed with __f*_rn (no contraction), cos / sin / 1/ax^2 / 1/ay^2 in the table;
//   * box blur: integer window sums, anchor k / 2, reflect_101, (sum + k^2 / 2) / k^2;
//   * Gaussian: fp32, rows first then columns, taps in ascending order, multiply and add rounded separately, one rintf;
//   * resize: fp32 bilinear with half-pixel centres, one rintf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "photo_kernels.hip.h"

namespace sspk {

constexpr int SH_MAX_BLOBS = 128, SH_MAX_CMDS = 64, SH_MAX_VERTS = 256, SH_MAX_TEX = 32, SH_MAX_POINTS = 256, SH_MAX_BLUR = 63;
constexpr int SH_CMD_WORDS = 12, SH_TEX_WORDS = 12, SH_MAX_TEX_BLOBS = 4096;
constexpr int SH_PRIM = 0, SH_THR = 1, SH_KEY = 2, SH_KSIZE = 4, SH_NBLOBS = 5, SH_MEAN0 = 6, SH_MEAN = 7, SH_NCMDS = 8, SH_NPOINTS = 9,
              SH_NVERTS = 10, SH_NTEX = 11, SH_BLOBS = 16, SH_CMDS = SH_BLOBS + 4 * SH_MAX_BLOBS, SH_VERTS = SH_CMDS + SH_CMD_WORDS * SH_MAX_CMDS,
              SH_TEX = SH_VERTS + 2 * SH_MAX_VERTS, SH_POINTS = SH_TEX + SH_TEX_WORDS * SH_MAX_TEX, SH_ROW = SH_POINTS + 2 * SH_MAX_POINTS;
constexpr int SH_CMD_POLY = 1, SH_CMD_SEG = 2, SH_CMD_ELLIPSE = 3, SH_CMD_TEXPOLY = 4, SH_CMD_NOISE = 5;
constexpr int SH_COORD_MAX = 16383;  // vertices are clamped here: differences fit 15 bits, their products 31
constexpr uint64_t SH_PIX_MUL = 0xD1342543DE82EF95ull;

// cv.randu(img, 0, 255) restated: a byte in 0..254 from the key and the pixel index
__device__ __forceinline__ int sh_noise(uint64_t key, unsigned pix) {
  return (int)(((hs_mix(key ^ ((uint64_t)pix * SH_PIX_MUL)) >> 32) * 255ull) >> 32);
}
__device__ __forceinline__ uint64_t sh_key(const int* __restrict__ q) { return (uint64_t)(unsigned)q[0] | ((uint64_t)(unsigned)q[1] << 32); }

// blob i of a texture (generate_custom_background: position, radius randint(20), get_random_color) from its key
__device__ __forceinline__ void sh_tex_blob(uint64_t key, int i, int H, int W, int bg, int& x, int& y, int& r, int& c) {
  const uint64_t h = hs_mix(key ^ ((uint64_t)(i + 1) * SH_PIX_MUL));
  x = (int)(((h & 0xFFFFull) * (uint64_t)W) >> 16);
  y = (int)((((h >> 16) & 0xFFFFull) * (uint64_t)H) >> 16);
  r = (int)((((h >> 32) & 0xFFull) * 20ull) >> 8);
  c = (int)((h >> 40) & 0xFFull);
  if (abs(c - bg) < 30) c = (c + 128) % 256;
}

__device__ __forceinline__ bool sh_verts_ok(const int* __restrict__ q) {  // a polygon command's vertex range lies in the pool
  return q[6] >= 0 && q[7] >= 0 && q[6] + q[7] <= SH_MAX_VERTS;
}
// (x, y) inside or on the polygon v[0..n) (integer vertices)
__device__ __forceinline__ bool sh_in_poly(const int* __restrict__ v, int n, int x, int y) {
  bool in = false;
  for (int i = 0; i < n; ++i) {
    const int j = i + 1 == n ? 0 : i + 1;
    const int x1 = v[2 * i], y1 = v[2 * i + 1], x2 = v[2 * j], y2 = v[2 * j + 1];
    const int cr = (x - x1) * (y2 - y1) - (y - y1) * (x2 - x1);
    if (cr == 0 && x >= min(x1, x2) && x <= max(x1, x2) && y >= min(y1, y2) && y <= max(y1, y2)) return true;  // on the edge
    if ((y1 <= y) != (y2 <= y)) {
      if (y2 > y1 ? cr < 0 : cr > 0) in = !in;  // x < x1 + (y - y1) (x2 - x1) / (y2 - y1)
    }
  }
  return in;
}
__device__ __forceinline__ bool sh_in_seg(int x1, int y1, int x2, int y2, int t, int x, int y) {
  const long ax = x2 - x1, ay = y2 - y1, px = x - x1, py = y - y1;
  const long L = ax * ax + ay * ay, s = px * ax + py * ay, tt = (long)t * t;
  if (L == 0 || s <= 0) return 4 * (px * px + py * py) <= tt;
  if (s >= L) { const long qx = x - x2, qy = y - y2; return 4 * (qx * qx + qy * qy) <= tt; }
  const long cr = px * ay - py * ax;
  return 4 * cr * cr <= tt * L;
}
__device__ __forceinline__ float sh_ellipse_q(const int* __restrict__ c, int x, int y) {  // c = the command
  const float dx = (float)(x - c[6]), dy = (float)(y - c[7]);
  const float co = __int_as_float(c[8]), si = __int_as_float(c[9]), ia = __int_as_float(c[10]), ib = __int_as_float(c[11]);
  const float xr = __fadd_rn(__fmul_rn(dx, co), __fmul_rn(dy, si)), yr = __fsub_rn(__fmul_rn(dy, co), __fmul_rn(dx, si));
  return __fadd_rn(__fmul_rn(__fmul_rn(xr, xr), ia), __fmul_rn(__fmul_rn(yr, yr), ib));
}

// ------------------------------------------------------------------------------------------------------------------
// The draw: one workgroup per image.  Thread 0 makes every decision in the reference's order; the whole group only counts
// pixels for the two background means (get_random_color needs int(np.mean(img)) of the thresholded noise and of the
// finished background).  The second mean is taken BEFORE the box blur (the blur changes the mean only through the
// reflected border): stated in DESIGN.md section 15.
// ------------------------------------------------------------------------------------------------------------------
struct ShDraw {
  HsRng rng;
  int* row;
  int H, W, ncmd, nvert, npts, ntex;
  __device__ double u() { return rng.uniform(); }
  __device__ int ri(int lo, int hi) {  // np.random.randint(lo, hi): [lo, hi); an empty range gives lo
    const int n = hi - lo;
    if (n <= 1) { u(); return lo; }
    return lo + min((int)(u() * n), n - 1);
  }
  __device__ int color(int bg) {  // get_random_color :15-21
    int c = ri(0, 256);
    if (abs(c - bg) < 30) c = (c + 128) % 256;
    return c;
  }
  __device__ static int toi(double v) {  // int() / astype(int): truncation; clamped so that the integer tests cannot overflow
    if (!(v == v)) return 0;
    return (int)fmax(-(double)SH_COORD_MAX, fmin((double)SH_COORD_MAX, v));
  }
  __device__ int* cmd(int type, int col) {
    if (ncmd >= SH_MAX_CMDS) return nullptr;
    int* c = row + SH_CMDS + SH_CMD_WORDS * ncmd++;
    c[0] = type; c[1] = col;
    return c;
  }
  __device__ void bbox(int* c, int x0, int y0, int x1, int y1) {
    c[2] = max(x0, 0); c[3] = max(y0, 0); c[4] = min(x1, W - 1); c[5] = min(y1, H - 1);
  }
  __device__ void seg(int col, int x1, int y1, int x2, int y2, int t) {
    t = max(t, 1);
    int* c = cmd(SH_CMD_SEG, col);
    if (!c) return;
    const int h = (t + 1) / 2;
    bbox(c, min(x1, x2) - h, min(y1, y2) - h, max(x1, x2) + h, max(y1, y2) + h);
    c[6] = x1; c[7] = y1; c[8] = x2; c[9] = y2; c[10] = t; c[11] = 0;
  }
  __device__ int* poly(int type, int col, const int (*p)[2], int n) {
    if (nvert + n > SH_MAX_VERTS) return nullptr;
    int* c = cmd(type, col);
    if (!c) return nullptr;
    int x0 = p[0][0], x1 = x0, y0 = p[0][1], y1 = y0;
    for (int i = 0; i < n; ++i) {
      row[SH_VERTS + 2 * (nvert + i)] = p[i][0]; row[SH_VERTS + 2 * (nvert + i) + 1] = p[i][1];
      x0 = min(x0, p[i][0]); x1 = max(x1, p[i][0]); y0 = min(y0, p[i][1]); y1 = max(y1, p[i][1]);
    }
    bbox(c, x0, y0, x1, y1);
    c[6] = nvert; c[7] = n; c[8] = c[9] = c[10] = c[11] = 0;
    nvert += n;
    return c;
  }
  __device__ void point(int x, int y) {
    if (npts >= SH_MAX_POINTS) return;
    row[SH_POINTS + 2 * npts] = __float_as_int((float)x); row[SH_POINTS + 2 * npts + 1] = __float_as_int((float)y);
    ++npts;
  }
  __device__ void point_inside(int x, int y) { if (x >= 0 && x < W && y >= 0 && y < H) point(x, y); }  // keep_points_inside :130-135
};

__device__ __forceinline__ bool sh_ccw(long ax, long ay, long bx, long by, long cx, long cy) { return (cy - ay) * (bx - ax) > (by - ay) * (cx - ax); }
__device__ __forceinline__ bool sh_intersect(const int* a, const int* b) {  // intersect :124-127 for two segments (x1, y1, x2, y2)
  return (sh_ccw(a[0], a[1], b[0], b[1], b[2], b[3]) != sh_ccw(a[2], a[3], b[0], b[1], b[2], b[3])) &&
         (sh_ccw(a[0], a[1], a[2], a[3], b[0], b[1]) != sh_ccw(a[0], a[1], a[2], a[3], b[2], b[3]));
}

// n x n system with partial pivoting (cv.getAffineTransform: 3, cv.getPerspectiveTransform: 8)
template <int N>
__device__ void sh_solve(double (*A)[N + 1], double* out) {
  for (int c = 0; c < N; ++c) {
    int piv = c;
    for (int r = c + 1; r < N; ++r) if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
    for (int k = 0; k <= N; ++k) { const double t = A[c][k]; A[c][k] = A[piv][k]; A[piv][k] = t; }
    const double d = A[c][c];
    for (int r = 0; r < N; ++r) {
      if (r == c) continue;
      const double f = A[r][c] / d;
      for (int k = c; k <= N; ++k) A[r][k] -= f * A[c][k];
    }
  }
  for (int i = 0; i < N; ++i) out[i] = A[i][N] / A[i][i];
}

// the affine + perspective pair of draw_checkerboard :379-398 / draw_stripes :512-531 (17 uniform draws: alpha, 8, 8)
struct ShWarp {
  double a[6], p[9];
  __device__ void sample(ShDraw& d, double tp0, double tp1) {
    const double alpha = (double)max(d.H, d.W) * (tp0 + d.u() * tp1);
    const double c0 = (double)(d.H / 2), c1 = (double)(d.W / 2), sq = (double)(min(d.H, d.W) / 3);  // np.float32(img.shape) // 2: (H, W) order as written
    const double p1[4][2] = {{c0 + sq, c1 + sq}, {c0 + sq, c1 - sq}, {c0 - sq, c1 - sq}, {c0 - sq, c1 + sq}};
    double p2[4][2];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 2; ++j) p2[i][j] = (double)(float)(p1[i][j] + (double)(float)(-alpha + d.u() * 2.0 * alpha));
    for (int r = 0; r < 2; ++r) {
      double A[3][4];
      for (int i = 0; i < 3; ++i) { A[i][0] = p1[i][0]; A[i][1] = p1[i][1]; A[i][2] = 1.0; A[i][3] = p2[i][r]; }
      sh_solve<3>(A, a + 3 * r);
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 2; ++j) p2[i][j] = (double)(float)(p1[i][j] + (double)(float)(-alpha / 2 + d.u() * alpha));
    double A[8][9];
    for (int k = 0; k < 4; ++k) {
      const double x = p1[k][0], y = p1[k][1], uu = p2[k][0], v = p2[k][1];
      const double r0[9] = {x, y, 1, 0, 0, 0, -uu * x, -uu * y, uu}, r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, v};
      for (int c = 0; c < 9; ++c) { A[2 * k][c] = r0[c]; A[2 * k + 1][c] = r1[c]; }
    }
    sh_solve<8>(A, p);
    p[8] = 1.0;
  }
  __device__ void apply(double x, double y, int& ox, int& oy) const {
    const double ax = a[0] * x + a[1] * y + a[2], ay = a[3] * x + a[4] * y + a[5];
    const double z = ax * p[6] + ay * p[7] + p[8];
    ox = ShDraw::toi((ax * p[0] + ay * p[1] + p[2]) / z);
    oy = ShDraw::toi((ax * p[3] + ay * p[4] + p[5]) / z);
  }
};

// the corner sampler and the two filters shared by draw_polygon :172-199 and draw_multiple_polygons :240-268.  The filters are
// repeated until they remove nothing, so that the polygon that is drawn has no zero edge and no angle >= 2 pi / 3 (the
// reference applies each once: DESIGN.md section 15).  Returns the corner count; centre / radius through cx, cy, rad.
__device__ int sh_sample_polygon(ShDraw& d, int max_sides, int (*pts)[2], int& cx, int& cy, double& rad) {
  int n = d.ri(3, max_sides);
  n = min(n, 16);
  const double min_dim = (double)min(d.H, d.W);
  rad = fmax(d.u() * min_dim / 2, min_dim / 10);
  cx = d.ri((int)rad, (int)(d.W - rad));
  cy = d.ri((int)rad, (int)(d.H - rad));
  double ang[16];
  const double two_pi = 6.283185307179586;
  for (int i = 0; i < n; ++i) { const double s0 = two_pi * i / n, s1 = two_pi * (i + 1) / n; ang[i] = s0 + d.u() * (s1 - s0); }
  for (int i = 0; i < n; ++i) {
    const double fx = fmax(d.u(), 0.4), fy = fmax(d.u(), 0.4);
    pts[i][0] = ShDraw::toi(cx + fx * rad * cos(ang[i]));
    pts[i][1] = ShDraw::toi(cy + fy * rad * sin(ang[i]));
  }
  for (int pass = 0; pass < 16; ++pass) {
    bool keep[16];
    int m = 0;
    for (int i = 0; i < n; ++i) { const int j = (i + n - 1) % n; keep[i] = pts[j][0] != pts[i][0] || pts[j][1] != pts[i][1]; }
    for (int i = 0; i < n; ++i) if (keep[i]) { pts[m][0] = pts[i][0]; pts[m][1] = pts[i][1]; ++m; }
    const int removed_a = n - m;
    n = m;
    m = 0;
    for (int i = 0; i < n; ++i) {
      const int j = (i + n - 1) % n, k = (i + 1) % n;
      const double ax = pts[j][0] - pts[i][0], ay = pts[j][1] - pts[i][1], bx = pts[k][0] - pts[i][0], by = pts[k][1] - pts[i][1];
      const double na = sqrt(ax * ax + ay * ay), nb = sqrt(bx * bx + by * by);
      keep[i] = na > 0 && nb > 0 && acos(fmax(-1.0, fmin(1.0, (ax / na) * (bx / nb) + (ay / na) * (by / nb)))) < two_pi / 3;
    }
    for (int i = 0; i < n; ++i) if (keep[i]) { pts[m][0] = pts[i][0]; pts[m][1] = pts[i][1]; ++m; }
    const int removed_b = n - m;
    n = m;
    if (removed_a + removed_b == 0 || n < 3) break;
  }
  return n;
}

__device__ void sh_draw_primitive(ShDraw& d, const ssp_shapes_params& P, int prim, int bg) {
  const int H = d.H, W = d.W, min_dim = min(H, W);
  switch (prim) {
    case 0: {  // draw_lines :138-163
      const int num = d.ri(1, P.lines_nb_lines);
      for (int i = 0; i < num; ++i) {
        int s[4];
        s[0] = d.ri(0, W); s[1] = d.ri(0, H); s[2] = d.ri(0, W); s[3] = d.ri(0, H);
        bool hit = false;
        for (int c = 0; c < d.ncmd && !hit; ++c) hit = sh_intersect(d.row + SH_CMDS + SH_CMD_WORDS * c + 6, s);
        if (hit) continue;
        const int col = d.color(bg);
        const int t = d.ri((int)(min_dim * 0.01), (int)(min_dim * 0.02));
        d.seg(col, s[0], s[1], s[2], s[3], t);
        d.point(s[0], s[1]); d.point(s[2], s[3]);
      }
    } break;
    case 1: {  // draw_polygon :166-206 (the recursion as a loop)
      int pts[16][2], cx, cy;
      double rad;
      for (int attempt = 0; attempt < 64; ++attempt) {
        const int n = sh_sample_polygon(d, P.polygon_max_sides, pts, cx, cy, rad);
        if (n < 3) continue;
        d.poly(SH_CMD_POLY, d.color(bg), pts, n);
        for (int i = 0; i < n; ++i) d.point(pts[i][0], pts[i][1]);
        break;
      }
    } break;
    case 2: {  // draw_multiple_polygons :227-301
      for (int i = 0; i < P.multi_nb_polygons && d.ntex < SH_MAX_TEX; ++i) {
        int pts[16][2], cx, cy;
        double rad;
        const int n = sh_sample_polygon(d, P.multi_max_sides, pts, cx, cy, rad);
        if (n < 3) continue;
        bool hit = false;
        for (int c = 0; c < d.ncmd && !hit; ++c) {
          const int* q = d.row + SH_CMDS + SH_CMD_WORDS * c;
          const int* v = d.row + SH_VERTS + 2 * q[6];
          for (int e = 0; e < q[7] && !hit; ++e) {
            const int f = (e + 1) % q[7];
            const int a[4] = {v[2 * e], v[2 * e + 1], v[2 * f], v[2 * f + 1]};
            for (int g = 0; g < n && !hit; ++g) {
              const int b[4] = {pts[g][0], pts[g][1], pts[(g + 1) % n][0], pts[(g + 1) % n][1]};
              hit = sh_intersect(a, b);
            }
          }
        }
        for (int t = 0; t < d.ntex && !hit; ++t) {  // overlap :209-217
          const int* q = d.row + SH_TEX + SH_TEX_WORDS * t;
          const double r2 = (double)__int_as_float(q[6]), dx = cx - q[4], dy = cy - q[5];
          hit = sqrt(dx * dx + dy * dy) + fmin(rad, r2) < fmax(rad, r2);
        }
        if (hit) continue;
        const int base = d.color(bg);
        int* c = d.poly(SH_CMD_TEXPOLY, base, pts, n);
        if (!c) break;
        c[8] = d.ntex;
        int* q = d.row + SH_TEX + SH_TEX_WORDS * d.ntex++;
        const uint64_t key = hs_mix(d.rng.key ^ (0x7465787475726573ull + (uint64_t)d.rng.ctr++));
        q[0] = base; q[1] = d.ri(P.multi_kernel_lo, P.multi_kernel_hi); q[2] = (int)(unsigned)key; q[3] = (int)(unsigned)(key >> 32);
        q[4] = cx; q[5] = cy; q[6] = __float_as_int((float)rad); q[7] = c[2]; q[8] = c[3]; q[9] = c[4]; q[10] = c[5]; q[11] = 0;
        for (int k = 0; k < n; ++k) d.point(pts[k][0], pts[k][1]);
      }
    } break;
    case 3: {  // draw_ellipses :304-331
      const double md = (double)min_dim / 4;
      for (int i = 0; i < P.ellipses_nb; ++i) {
        const int ax = (int)fmax(d.u() * md, md / 5), ay = (int)fmax(d.u() * md, md / 5);
        const int mr = max(ax, ay);
        const int x = d.ri(mr, W - mr), y = d.ri(mr, H - mr);
        // :322-324: `sqrt(sum(diff^2, axis=1)) - rads` subtracts an (n, 1) array from an (n,) one and broadcasts to n x n, so the
        // candidate is rejected when max_rad > dist_i - rads_j for ANY pair (i, j): nearest centre against the largest radius
        double dmin = 1e30;
        int rmax = 0;
        for (int c = 0; c < d.ncmd; ++c) {
          const int* q = d.row + SH_CMDS + SH_CMD_WORDS * c;
          const double dx = q[6] - x, dy = q[7] - y;
          dmin = fmin(dmin, sqrt(dx * dx + dy * dy));
          rmax = max(rmax, d.row[SH_VERTS + c]);  // rads[c], stored below
        }
        const bool hit = d.ncmd > 0 && (double)mr > dmin - (double)rmax;
        if (hit) continue;
        const int col = d.color(bg);
        const double ang = d.u() * 90.0 * (3.141592653589793 / 180.0);
        int* c = d.cmd(SH_CMD_ELLIPSE, col);
        if (!c) break;
        d.row[SH_VERTS + (d.ncmd - 1)] = mr;  // the vertex pool is free in an ellipse image: max_rad of command c (the separation test reads it)
        d.bbox(c, x - mr, y - mr, x + mr, y + mr);
        c[6] = x; c[7] = y; c[8] = __float_as_int((float)cos(ang)); c[9] = __float_as_int((float)sin(ang));
        c[10] = __float_as_int(ax > 0 ? 1.f / (float)(ax * ax) : 0.f);
        c[11] = __float_as_int(ay > 0 && ax > 0 ? 1.f / (float)(ay * ay) : 3.0e38f);  // a degenerate ellipse covers at most its centre
      }
    } break;
    case 4: {  // draw_star :334-359
      const int nb = min(d.ri(3, P.star_nb_branches), 16);
      const int t = d.ri((int)(min_dim * 0.01), (int)(min_dim * 0.02));
      const double rad = fmax(d.u() * min_dim / 2, (double)min_dim / 5);
      const int x = d.ri((int)rad, (int)(W - rad)), y = d.ri((int)rad, (int)(H - rad));
      double ang[16];
      int pts[16][2];
      for (int i = 0; i < nb; ++i) { const double s0 = 6.283185307179586 * i / nb, s1 = 6.283185307179586 * (i + 1) / nb; ang[i] = s0 + d.u() * (s1 - s0); }
      for (int i = 0; i < nb; ++i) {
        const double fx = fmax(d.u(), 0.3), fy = fmax(d.u(), 0.3);
        pts[i][0] = ShDraw::toi(x + fx * rad * cos(ang[i])); pts[i][1] = ShDraw::toi(y + fy * rad * sin(ang[i]));
      }
      d.point(x, y);
      for (int i = 0; i < nb; ++i) {
        d.seg(d.color(bg), x, y, pts[i][0], pts[i][1], t);
        d.point(pts[i][0], pts[i][1]);
      }
    } break;
    case 5: {  // draw_checkerboard :362-478
      const int rows = min(d.ri(3, P.checker_max_rows), 6), cols = min(d.ri(3, P.checker_max_cols), 6);
      const int s = min((W - 1) / cols, (H - 1) / rows);
      ShWarp w;
      w.sample(d, P.checker_transform[0], P.checker_transform[1]);
      int wp[49][2];
      for (int i = 0; i <= rows; ++i) for (int j = 0; j <= cols; ++j) w.apply((double)(s * j), (double)(s * i), wp[i * (cols + 1) + j][0], wp[i * (cols + 1) + j][1]);
      int colors[36];
      for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) {
          int col;
          if (i == 0 && j == 0) col = d.color(bg);
          else {  // get_different_color :24-37
            col = d.ri(0, 256);
            for (int count = 0; count < 20; ++count) {
              const bool close = (i != 0 && abs(colors[(i - 1) * cols + j] - col) < 50) || (j != 0 && abs(colors[i * cols + j - 1] - col) < 50);
              if (!close) break;
              col = d.ri(0, 256);
            }
          }
          colors[i * cols + j] = col;
          const int a = i * (cols + 1) + j, b = (i + 1) * (cols + 1) + j;
          const int q[4][2] = {{wp[a][0], wp[a][1]}, {wp[a + 1][0], wp[a + 1][1]}, {wp[b + 1][0], wp[b + 1][1]}, {wp[b][0], wp[b][1]}};
          d.poly(SH_CMD_POLY, col, q, 4);
        }
      const int nb_rows = d.ri(2, rows + 2), nb_cols = d.ri(2, cols + 2);
      const int t = d.ri((int)(min_dim * 0.01), (int)(min_dim * 0.015));
      for (int k = 0; k < nb_rows; ++k) {
        const int r = d.ri(0, rows + 1), c1 = d.ri(0, cols + 1), c2 = d.ri(0, cols + 1);
        const int col = d.color(bg);
        d.seg(col, wp[r * (cols + 1) + c1][0], wp[r * (cols + 1) + c1][1], wp[r * (cols + 1) + c2][0], wp[r * (cols + 1) + c2][1], t);
      }
      for (int k = 0; k < nb_cols; ++k) {
        const int c = d.ri(0, cols + 1), r1 = d.ri(0, rows + 1), r2 = d.ri(0, rows + 1);
        const int col = d.color(bg);
        d.seg(col, wp[r1 * (cols + 1) + c][0], wp[r1 * (cols + 1) + c][1], wp[r2 * (cols + 1) + c][0], wp[r2 * (cols + 1) + c][1], t);
      }
      for (int k = 0; k < (rows + 1) * (cols + 1); ++k) d.point_inside(wp[k][0], wp[k][1]);
    } break;
    case 6: {  // draw_stripes :481-593
      const int bh = (int)(H * (1 + d.u())), bw = (int)(W * (1 + d.u()));
      int col = min(d.ri(5, P.stripes_max_nb_cols), 14);
      int cs[16];
      int n = 0;
      for (int i = 0; i < col - 1; ++i) cs[n++] = (int)(bw * d.u());
      cs[n++] = 0; cs[n++] = bw - 1;
      for (int i = 1; i < n; ++i) { const int v = cs[i]; int j = i - 1; while (j >= 0 && cs[j] > v) { cs[j + 1] = cs[j]; --j; } cs[j + 1] = v; }
      int m = 0;
      for (int i = 0; i < n; ++i) if (m == 0 || cs[i] != cs[m - 1]) cs[m++] = cs[i];  // np.unique
      n = m; m = 0;
      const double min_width = (double)min_dim * P.stripes_min_width_ratio;
      int kept[16];
      for (int i = 0; i < n; ++i) {
        const double next = i + 1 < n ? (double)cs[i + 1] : (double)bw + min_width;
        if (next - cs[i] >= min_width) kept[m++] = cs[i];
      }
      col = m - 1;
      ShWarp w;
      w.sample(d, P.stripes_transform[0], P.stripes_transform[1]);
      int wp[32][2];
      for (int i = 0; i <= col; ++i) {
        w.apply((double)kept[i], 0.0, wp[i][0], wp[i][1]);
        w.apply((double)kept[i], (double)(bh - 1), wp[i + col + 1][0], wp[i + col + 1][1]);
      }
      int color = d.color(bg);
      for (int i = 0; i < col; ++i) {
        color = (color + 128 + d.ri(-30, 30)) % 256;
        const int q[4][2] = {{wp[i][0], wp[i][1]}, {wp[i + 1][0], wp[i + 1][1]}, {wp[i + col + 2][0], wp[i + col + 2][1]}, {wp[i + col + 1][0], wp[i + col + 1][1]}};
        d.poly(SH_CMD_POLY, color, q, 4);
      }
      const int nb_rows = d.ri(2, 5), nb_cols = d.ri(2, col + 2);
      const int t = d.ri((int)(min_dim * 0.01), (int)(min_dim * 0.015));
      for (int k = 0; k < nb_rows; ++k) {
        const int r = d.u() < 0.5 ? 0 : col + 1, c1 = d.ri(0, col + 1), c2 = d.ri(0, col + 1);
        color = d.color(bg);
        d.seg(color, wp[r + c1][0], wp[r + c1][1], wp[r + c2][0], wp[r + c2][1], t);
      }
      for (int k = 0; k < nb_cols; ++k) {
        const int c = d.ri(0, col + 1);
        color = d.color(bg);
        d.seg(color, wp[c][0], wp[c][1], wp[c + col + 1][0], wp[c + col + 1][1], t);
      }
      for (int k = 0; k < 2 * (col + 1); ++k) d.point_inside(wp[k][0], wp[k][1]);
    } break;
    case 7: {  // draw_cube :596-680
      const double md = (double)min_dim, min_side = md * P.cube_min_size_ratio;
      const double l[3] = {min_side + d.u() * 2 * md / 3, min_side + d.u() * 2 * md / 3, min_side + d.u() * 2 * md / 3};
      double ra[3], sc[3];
      for (int i = 0; i < 3; ++i) ra[i] = d.u() * 3 * 3.141592653589793 / 10. + 3.141592653589793 / 10.;
      for (int i = 0; i < 3; ++i) sc[i] = P.cube_scale[0] + d.u() * P.cube_scale[1];
      const double tx = W * (double)P.cube_trans[0] + d.ri((int)(-W * (double)P.cube_trans[1]), (int)(W * (double)P.cube_trans[1]));
      const double ty = H * (double)P.cube_trans[0] + d.ri((int)(-H * (double)P.cube_trans[1]), (int)(H * (double)P.cube_trans[1]));
      int cube[8][2];
      for (int v = 0; v < 8; ++v) {
        double x = (v & 1) ? l[0] : 0, y = (v & 2) ? l[1] : 0, z = (v & 4) ? l[2] : 0;
        const double x3 = cos(ra[2]) * x - sin(ra[2]) * z, z3 = sin(ra[2]) * x + cos(ra[2]) * z;  // rotation_3
        const double y2 = cos(ra[1]) * y - sin(ra[1]) * z3;                                       // rotation_2 (z is projected away)
        const double x1 = cos(ra[0]) * x3 - sin(ra[0]) * y2, y1 = sin(ra[0]) * x3 + cos(ra[0]) * y2;  // rotation_1
        cube[v][0] = ShDraw::toi(tx + sc[0] * x1); cube[v][1] = ShDraw::toi(ty + sc[1] * y1);
      }
      const int faces[3][4] = {{7, 3, 1, 5}, {7, 5, 4, 6}, {7, 6, 2, 3}};
      const int col_face = d.color(bg);
      for (int f = 0; f < 3; ++f) {
        int q[4][2];
        for (int j = 0; j < 4; ++j) { q[j][0] = cube[faces[f][j]][0]; q[j][1] = cube[faces[f][j]][1]; }
        d.poly(SH_CMD_POLY, col_face, q, 4);
      }
      const int t = d.ri((int)(md * 0.003), (int)(md * 0.015));
      for (int f = 0; f < 3; ++f)
        for (int j = 0; j < 4; ++j) {
          const int col_edge = (col_face + 128 + d.ri(-64, 64)) % 256;
          const int a = faces[f][j], b = faces[f][(j + 1) % 4];
          d.seg(col_edge, cube[a][0], cube[a][1], cube[b][0], cube[b][1], t);
        }
      for (int v = 1; v < 8; ++v) d.point_inside(cube[v][0], cube[v][1]);
    } break;
    default: {  // gaussian_noise :683-686
      int* c = d.cmd(SH_CMD_NOISE, 0);
      const uint64_t key = hs_mix(d.rng.key ^ 0x6E6F697365ull);
      d.bbox(c, 0, 0, W - 1, H - 1);
      c[6] = (int)(unsigned)key; c[7] = (int)(unsigned)(key >> 32); c[8] = c[9] = c[10] = c[11] = 0;
    } break;
  }
}

__global__ void __launch_bounds__(256) shapes_draw_kernel(uint64_t seed, ssp_shapes_params P, int B, int* __restrict__ table) {
  __shared__ unsigned long long red[256];
  __shared__ unsigned char lst[256][SH_MAX_BLOBS];
  __shared__ int sh_bg;
  const int n = blockIdx.x, tid = threadIdx.x, H = P.gen_h, W = P.gen_w;
  int* row = table + (size_t)n * SH_ROW;
  for (int i = tid; i < SH_ROW; i += 256) row[i] = 0;
  __syncthreads();
  ShDraw d;
  d.rng = HsRng{hs_mix(hs_mix(seed ^ 0x7368617065733135ull) ^ ((uint64_t)n << 32)), 0};
  d.row = row; d.H = H; d.W = W; d.ncmd = d.nvert = d.npts = d.ntex = 0;
  const int dim = max(H, W);
  if (tid == 0) {
    // the primitive: probability proportional to its share of the union of the truncated splits
    double tot = 0, acc = 0;
    for (int i = 0; i < 9; ++i) tot += P.weights[i];
    const double r = d.u() * tot;
    int prim = 8;
    for (int i = 0; i < 9; ++i) { acc += P.weights[i]; if (r < acc) { prim = i; break; } }
    while (prim > 0 && !(P.weights[prim] > 0)) --prim;
    row[SH_PRIM] = prim;
    // generate_background :52-79
    const uint64_t key = hs_mix(d.rng.key ^ 0x6261636B67726E64ull);
    row[SH_KEY] = (int)(unsigned)key; row[SH_KEY + 1] = (int)(unsigned)(key >> 32);
    row[SH_THR] = d.ri(0, 256);
    row[SH_NBLOBS] = P.bg_nb_blobs;
    for (int i = 0; i < P.bg_nb_blobs; ++i) row[SH_BLOBS + 4 * i] = d.ri(0, W);
    for (int i = 0; i < P.bg_nb_blobs; ++i) row[SH_BLOBS + 4 * i + 1] = d.ri(0, H);
  }
  __syncthreads();
  const uint64_t key = sh_key(row + SH_KEY);
  const int thr = row[SH_THR], nb = row[SH_NBLOBS];
  {  // int(np.mean(img)) of the thresholded noise
    unsigned long long cnt = 0;
    for (unsigned p = tid; p < (unsigned)(H * W); p += 256) cnt += sh_noise(key, p) > thr ? 1 : 0;
    red[tid] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    if (tid == 0) {
      const int mean0 = (int)(red[0] * 255ull / (unsigned long long)((long)H * W));
      row[SH_MEAN0] = mean0;
      for (int i = 0; i < nb; ++i) {
        row[SH_BLOBS + 4 * i + 3] = d.color(mean0);
        row[SH_BLOBS + 4 * i + 2] = d.ri((int)(dim * (double)P.bg_min_rad_ratio), (int)(dim * (double)P.bg_max_rad_ratio));
      }
      row[SH_KSIZE] = d.ri(P.bg_min_kernel, P.bg_max_kernel);
    }
    __syncthreads();
  }
  {  // int(np.mean(img)) of noise + blobs (before the box blur)
    unsigned long long sum = 0;
    for (int y = tid; y < H; y += 256) {
      int m = 0;
      for (int i = 0; i < nb; ++i) if (abs(y - row[SH_BLOBS + 4 * i + 1]) <= row[SH_BLOBS + 4 * i + 2]) lst[tid][m++] = (unsigned char)i;
      for (int x = 0; x < W; ++x) {
        int v = sh_noise(key, (unsigned)(y * W + x)) > thr ? 255 : 0;
        for (int k = 0; k < m; ++k) {
          const int* b = row + SH_BLOBS + 4 * lst[tid][k];
          const int dx = x - b[0], dy = y - b[1];
          if (dx * dx + dy * dy <= b[2] * b[2]) v = b[3];
        }
        sum += (unsigned)v;
      }
    }
    __syncthreads();
    red[tid] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    if (tid == 0) sh_bg = (int)(red[0] / (unsigned long long)((long)H * W));
    __syncthreads();
  }
  if (tid == 0) {
    row[SH_MEAN] = sh_bg;
    sh_draw_primitive(d, P, row[SH_PRIM], sh_bg);
    row[SH_NCMDS] = d.ncmd; row[SH_NPOINTS] = d.npts; row[SH_NVERTS] = d.nvert; row[SH_NTEX] = d.ntex;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Render.  A "layer" is a blob picture followed by a box blur: layer -1 is the background over the whole image, layer t >= 0
// the texture of polygon t over that polygon's bounding box.
//   shapes_layer_rows_kernel  one workgroup per row: the row's blobs are culled into LDS, the unblurred row is produced at the
//                             reflected columns, an LDS prefix sum turns it into the k-wide window sums (uint32, HBM)
//   shapes_layer_cols_kernel  one thread per column and 32 rows: sliding k-high sum of the window sums, the one rounding,
//                             uint8 store (textures: only inside the polygon)
//   shapes_paint_kernel       64 x 16 tiles: one ballot over the <= 64 commands' bounding boxes gives the tile's command mask
//   shapes_blur_resize_kernel one thread per OUTPUT pixel: the four Gaussian values its bilinear taps read, nothing else
// ------------------------------------------------------------------------------------------------------------------
struct ShLayer { int k, x0, y0, x1, y1, base, nblobs; uint64_t key; };
__device__ __forceinline__ bool sh_layer(const int* __restrict__ row, int layer, int H, int W, int tex_blobs, ShLayer& L) {
  if (layer < 0) {
    L.k = max(row[SH_KSIZE], 1); L.x0 = 0; L.y0 = 0; L.x1 = W - 1; L.y1 = H - 1; L.base = -1; L.nblobs = min(max(row[SH_NBLOBS], 0), SH_MAX_BLOBS); L.key = sh_key(row + SH_KEY);
    return true;
  }
  if (layer >= min(row[SH_NTEX], SH_MAX_TEX)) return false;
  const int* q = row + SH_TEX + SH_TEX_WORDS * layer;
  L.k = max(q[1], 1); L.x0 = max(q[7], 0); L.y0 = max(q[8], 0); L.x1 = min(q[9], W - 1); L.y1 = min(q[10], H - 1); L.base = q[0] & 255; L.nblobs = tex_blobs; L.key = sh_key(q + 2);
  return L.x1 >= L.x0 && L.y1 >= L.y0;
}

// dynamic LDS: uint32 pre[W + kmax] | int2 list[cap] ; grid (H, B)
__global__ void __launch_bounds__(256) shapes_layer_rows_kernel(const int* __restrict__ table, int layer, int H, int W, int tex_blobs,
                                                                int list_cap, int pre_cap, unsigned* __restrict__ sums) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sh_smem[];
  __shared__ unsigned part[256];
  __shared__ int nlist;
  unsigned* pre = reinterpret_cast<unsigned*>(sh_smem);
  int2* list = reinterpret_cast<int2*>(pre + pre_cap);
  const int n = blockIdx.y, y = blockIdx.x, tid = threadIdx.x;
  const int* row = table + (size_t)n * SH_ROW;
  ShLayer L;
  if (!sh_layer(row, layer, H, W, tex_blobs, L)) return;
  if (L.x1 - L.x0 + L.k > pre_cap) return;  // a table drawn with larger kernel sizes than this call's parameters: not rendered
  const int a = L.k / 2;
  {  // is row y read by the column pass of rows y0..y1 ?  (every row for a window that reflects more than once)
    const int r0 = L.y0 - a, r1 = L.y1 - a + L.k - 1;
    int lo = max(r0, 0), hi = min(r1, H - 1);
    if (r0 < 0) hi = max(hi, min(H - 1, -r0));
    if (r1 > H - 1) lo = min(lo, max(0, 2 * (H - 1) - r1));
    if (r0 < -(H - 1) || r1 > 2 * (H - 1)) { lo = 0; hi = H - 1; }
    if (y < lo || y > hi) return;
  }
  const int bg = row[SH_MEAN];
  if (tid == 0) nlist = 0;
  __syncthreads();
  for (int i = tid; i < L.nblobs; i += 256) {
    int bx, by, br, bc;
    if (layer < 0) { const int* b = row + SH_BLOBS + 4 * i; bx = b[0]; by = b[1]; br = b[2]; bc = b[3]; }
    else sh_tex_blob(L.key, i, H, W, bg, bx, by, br, bc);
    const int dy = y - by, m = br * br - dy * dy;
    if (m >= 0) {
      const int slot = atomicAdd(&nlist, 1);
      if (slot < list_cap) list[slot] = make_int2(bx | (m << 16), (i << 8) | bc);
    }
  }
  __syncthreads();
  const int nl = min(nlist, list_cap);
  const int wr = L.x1 - L.x0 + 1, next = wr + L.k - 1;  // next <= pre_cap (checked by the host)
  const int chunk = (next + 255) / 256;
  const int e0 = tid * chunk, e1 = min(e0 + chunk, next);
  unsigned run = 0;
  for (int e = e0; e < e1; ++e) {
    const int xx = reflect101(L.x0 - a + e, W);
    int v = L.base >= 0 ? L.base : (sh_noise(L.key, (unsigned)(y * W + xx)) > row[SH_THR] ? 255 : 0);
    int best = -1;
    for (int q = 0; q < nl; ++q) {
      const int2 b = list[q];
      const int dx = xx - (b.x & 0xFFFF), idx = b.y >> 8;
      if (dx * dx <= (b.x >> 16) && idx > best) { best = idx; v = b.y & 0xFF; }
    }
    run += (unsigned)v;
    pre[e] = run;
  }
  part[tid] = run;
  __syncthreads();
  unsigned off = 0;
  for (int t = 0; t < tid; ++t) off += part[t];
  for (int e = e0; e < e1; ++e) pre[e] += off;
  __syncthreads();
  unsigned* out = sums + ((size_t)n * H + y) * W;
  for (int i = tid; i < wr; i += 256) out[L.x0 + i] = pre[i + L.k - 1] - (i > 0 ? pre[i - 1] : 0u);
}

// grid (cdiv(W, 256), cdiv(H, 32), B)
__global__ void __launch_bounds__(256) shapes_layer_cols_kernel(const int* __restrict__ table, int layer, int H, int W, int pre_cap,
                                                                const unsigned* __restrict__ sums, unsigned char* __restrict__ plane) {
  const int n = blockIdx.z;
  const int* row = table + (size_t)n * SH_ROW;
  ShLayer L;
  if (!sh_layer(row, layer, H, W, 0, L) || L.x1 - L.x0 + L.k > pre_cap) return;
  const int x = L.x0 + blockIdx.x * 256 + threadIdx.x, ya = L.y0 + blockIdx.y * 32;
  if (x > L.x1 || ya > L.y1) return;
  const int yb = min(ya + 31, L.y1), a = L.k / 2;
  const unsigned* s = sums + (size_t)n * H * W + x;
  const int* verts = nullptr;
  int nv = 0;
  if (layer >= 0) {
    for (int c = 0; c < min(row[SH_NCMDS], SH_MAX_CMDS); ++c) {
      const int* q = row + SH_CMDS + SH_CMD_WORDS * c;
      if (q[0] == SH_CMD_TEXPOLY && q[8] == layer && sh_verts_ok(q)) { verts = row + SH_VERTS + 2 * q[6]; nv = q[7]; }
    }
    if (verts == nullptr) return;
  }
  unsigned acc = 0;
  for (int j = 0; j < L.k; ++j) acc += s[(size_t)reflect101(ya - a + j, H) * W];
  const unsigned kk = (unsigned)(L.k * L.k);
  unsigned char* out = plane + (size_t)n * H * W + x;
  for (int y = ya; y <= yb; ++y) {
    if (layer < 0 || sh_in_poly(verts, nv, x, y)) out[(size_t)y * W] = (unsigned char)((acc + kk / 2) / kk);
    if (y < yb) acc += s[(size_t)reflect101(y + 1 - a + L.k - 1, H) * W] - s[(size_t)reflect101(y - a, H) * W];
  }
}

// grid (cdiv(W, 64), cdiv(H, 16), B); thread = 4 consecutive pixels of one row
__global__ void __launch_bounds__(256) shapes_paint_kernel(const int* __restrict__ table, int H, int W, unsigned char* __restrict__ plane) {
  __shared__ unsigned long long mask_s;
  const int n = blockIdx.z, tid = threadIdx.x;
  const int* row = table + (size_t)n * SH_ROW;
  const int tx0 = blockIdx.x * 64, ty0 = blockIdx.y * 16;
  if (tid < 64) {
    bool hit = false;
    if (tid < min(row[SH_NCMDS], SH_MAX_CMDS)) {
      const int* q = row + SH_CMDS + SH_CMD_WORDS * tid;
      hit = q[0] != SH_CMD_TEXPOLY && (q[0] != SH_CMD_POLY || sh_verts_ok(q)) && q[2] <= tx0 + 63 && q[4] >= tx0 && q[3] <= ty0 + 15 && q[5] >= ty0;
    }
    const unsigned long long m = __ballot(hit);
    if (tid == 0) mask_s = m;
  }
  __syncthreads();
  unsigned long long mask = mask_s;
  if (mask == 0) return;
  const int y = ty0 + tid / 16, xb = tx0 + (tid % 16) * 4;
  if (y >= H || xb >= W) return;
  unsigned char* p = plane + ((size_t)n * H + y) * W;
  int v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = xb + k < W ? p[xb + k] : 0;
  while (mask) {
    const int c = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const int* q = row + SH_CMDS + SH_CMD_WORDS * c;
    if (y < q[3] || y > q[5] || xb + 3 < q[2] || xb > q[4]) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = xb + k;
      bool in;
      switch (q[0]) {
        case SH_CMD_POLY: in = sh_in_poly(row + SH_VERTS + 2 * q[6], q[7], x, y); break;
        case SH_CMD_SEG: in = sh_in_seg(q[6], q[7], q[8], q[9], q[10], x, y); break;
        case SH_CMD_ELLIPSE: in = sh_ellipse_q(q, x, y) <= 1.f; break;
        case SH_CMD_NOISE: in = true; break;
        default: in = false; break;
      }
      if (in) v[k] = q[0] == SH_CMD_NOISE ? sh_noise(sh_key(q + 6), (unsigned)(y * W + x)) : (q[1] & 255);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) if (xb + k < W) p[xb + k] = (unsigned char)v[k];
}

__device__ __forceinline__ void sh_src(int d, float scale, int n, int& i0, int& i1, float& f) {
  const float s = __fsub_rn(__fmul_rn(__fadd_rn((float)d, 0.5f), scale), 0.5f);
  const float fl = floorf(s);
  i0 = (int)fl; f = __fsub_rn(s, fl);
  if (i0 < 0) { i0 = 0; f = 0.f; }
  if (i0 >= n - 1) { i0 = n - 1; f = 0.f; }
  i1 = min(i0 + 1, n - 1);
}

// grid (cdiv(w, 64), cdiv(h, 4), B)
__global__ void __launch_bounds__(256) shapes_blur_resize_kernel(const unsigned char* __restrict__ plane, ssp_shapes_params P,
                                                                 unsigned char* __restrict__ out) {
  __shared__ float wts[SH_MAX_BLUR];
  const int H = P.gen_h, W = P.gen_w, h = P.out_h, w = P.out_w, k = P.blur_size, r = k / 2;
  if (threadIdx.x < SH_MAX_BLUR) wts[threadIdx.x] = P.gauss_w[threadIdx.x];
  __syncthreads();
  const int dx = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6), n = blockIdx.z;
  if (dx >= w || dy >= h) return;
  int x0, x1, y0, y1;
  float fx, fy;
  sh_src(dx, P.resize_scale_x, W, x0, x1, fx);
  sh_src(dy, P.resize_scale_y, H, y0, y1, fy);
  const unsigned char* im = plane + (size_t)n * H * W;
  float g[2][2];
  if (k <= 1) {
    g[0][0] = (float)im[(size_t)y0 * W + x0]; g[0][1] = (float)im[(size_t)y0 * W + x1];
    g[1][0] = (float)im[(size_t)y1 * W + x0]; g[1][1] = (float)im[(size_t)y1 * W + x1];
  } else {
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    const int nrows = k + (y1 - y0);  // y1 is y0 or y0 + 1: the two windows share k - 1 rows
    for (int i = 0; i < nrows; ++i) {
      const unsigned char* rp = im + (size_t)reflect101(y0 - r + i, H) * W;
      float hs0 = 0.f, hs1 = 0.f;
      for (int j = 0; j < k; ++j) {
        const float wj = wts[j];
        hs0 = __fadd_rn(hs0, __fmul_rn(wj, (float)rp[reflect101(x0 - r + j, W)]));
        hs1 = __fadd_rn(hs1, __fmul_rn(wj, (float)rp[reflect101(x1 - r + j, W)]));
      }
      if (i < k) { acc[0][0] = __fadd_rn(acc[0][0], __fmul_rn(wts[i], hs0)); acc[0][1] = __fadd_rn(acc[0][1], __fmul_rn(wts[i], hs1)); }
      if (y1 != y0 && i >= 1) { acc[1][0] = __fadd_rn(acc[1][0], __fmul_rn(wts[i - 1], hs0)); acc[1][1] = __fadd_rn(acc[1][1], __fmul_rn(wts[i - 1], hs1)); }
    }
    if (y1 == y0) { acc[1][0] = acc[0][0]; acc[1][1] = acc[0][1]; }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) g[a][b] = fminf(fmaxf(rintf(acc[a][b]), 0.f), 255.f);
  }
  const float gx = __fsub_rn(1.f, fx), gy = __fsub_rn(1.f, fy);
  const float top = __fadd_rn(__fmul_rn(gx, g[0][0]), __fmul_rn(fx, g[0][1])), bot = __fadd_rn(__fmul_rn(gx, g[1][0]), __fmul_rn(fx, g[1][1]));
  const float v = __fadd_rn(__fmul_rn(gy, top), __fmul_rn(fy, bot));
  out[((size_t)n * h + dy) * w + dx] = (unsigned char)fminf(fmaxf(rintf(v), 0.f), 255.f);
}

// points * resize / image_size (SyntheticDataset_gaussian.py:138-142); unused slots are zero
__global__ void shapes_points_kernel(const int* __restrict__ table, ssp_shapes_params P, int B, float* __restrict__ pts, int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * SH_MAX_POINTS) return;
  const int n = i / SH_MAX_POINTS, k = i - n * SH_MAX_POINTS;
  const int* row = table + (size_t)n * SH_ROW;
  const int cnt = min(max(row[SH_NPOINTS], 0), SH_MAX_POINTS);
  if (k == 0) counts[n] = cnt;
  const bool on = k < cnt;
  pts[2 * i] = on ? __fdiv_rn(__fmul_rn(__int_as_float(row[SH_POINTS + 2 * k]), (float)P.out_w), (float)P.gen_w) : 0.f;
  pts[2 * i + 1] = on ? __fdiv_rn(__fmul_rn(__int_as_float(row[SH_POINTS + 2 * k + 1]), (float)P.out_h), (float)P.gen_h) : 0.f;
}

// ---- the single-view feed: warp float key points, filter_points, round, clamp, scatter (SyntheticDataset_gaussian.py:342-351, 450-472)
// pts [B, stride, 2] (x, y), counts [B]; hpx [B,3,3] pixel-space homographies or nullptr (identity: no warp); labels zero-filled.
__global__ void warp_points_scatter_kernel(const float* __restrict__ pts, const int* __restrict__ counts, const float* __restrict__ hpx,
                                           float* __restrict__ labels, int B, int stride, int H, int W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * stride) return;
  const int n = i / stride, k = i - n * stride;
  if (k >= counts[n]) return;
  float x = pts[2 * i], y = pts[2 * i + 1];
  if (!(x >= 0.f && x <= (float)(W - 1) && y >= 0.f && y <= (float)(H - 1))) return;  // filter_points at :376
  if (hpx != nullptr) {
    float wx, wy;
    warp_point_exact(hpx + n * 9, x, y, wx, wy);
    if (!(wx >= 0.f && wx <= (float)(W - 1) && wy >= 0.f && wy <= (float)(H - 1))) return;
    x = wx; y = wy;
  }
  const int qx = min((int)rintf(x), W - 1), qy = min((int)rintf(y), H - 1);
  labels[((size_t)n * H + qy) * W + qx] = 1.f;
}

}  // namespace sspk
