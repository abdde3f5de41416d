// Photometric augmentation of the training images on the device: the reference's
//   ImgAugTransform.__call__      utils/photometric.py:10-78   (imgaug chain on the uint8 image)
//   customizedTransform.__call__  utils/photometric.py:83-113  (additive_shade on the float image)
// as two operators: photo_draw_kernel writes one row of PHOTO_DRAW_STRIDE floats per image (every random decision
// of the chain), and the apply kernels are a pure function of the image and its row.
//
// Stage order and 8-bit semantics of apply (stages 1-7: photo_pixel_kernel, one pass over the image):
//   1 q = uint8(img * 255)               float32 product, truncation (label_quantize_u8_kernel)
//   2 + brightness delta, saturating     iaa.Add
//   3 127 + alpha * (v - 127)            iaa.LinearContrast
//   4 + N(0, sigma) per pixel            iaa.AdditiveGaussianNoise
//   5 with probability p: 255 sin^2(pi u / 2)   iaa.ImpulseNoise (salt and pepper with a Beta(1/2, 1/2) replacement)
//   6 3x3 correlation, reflect_101       iaa.Sometimes(0.5, iaa.MotionBlur(3))
//   7 / 255
//   8 clip(v * (1 - t * M / 255), 0, 255) / 255 on the FLOAT value (no quantisation), M = GaussianBlur_k(ellipse mask)
// A neutral draw (delta 0, alpha 1, sigma 0, p 0, flag 0, kernel size 0) skips its stage; with all of them neutral the
// result is label_quantize_u8_kernel's bit for bit.
//
// RESTATED, UNPINNED (imgaug and cv2 are not available to compare against; same status as the erosion and the 4-point solve):
//   * every float -> uint8 conversion of stages 3-6 is round-half-to-even followed by the clip to [0, 255];
//   * the motion-blur weights are the bilinear rotation of the float line kernel [d, 1/2, 1-d] (imgaug rotates an 8-bit copy);
//   * the ellipse mask is the analytic inside test (x'/ax)^2 + (y'/ay)^2 <= 1 in the rotated frame (cv2 fills a polygon
//     approximation: edge pixels may differ, and a blur of 100+ taps follows); an ellipse with a zero axis covers nothing;
//   * the Gaussian weights are exp(-(j - r)^2 / (2 sigma^2)) normalised to sum 1 (cv2's fixed tables for k <= 7 are not used);
//   * the per-pixel random numbers are hs_mix(key, pixel index): a different stream from numpy's by construction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pair_kernels.hip.h"

namespace sspk {

// ---- the row of draws (mirrors SSP_PHOTO_* of include/ssp_hip.h) ----
constexpr int PHOTO_MAX_ELLIPSES = 32;
constexpr int PHOTO_BRIGHTNESS = 0, PHOTO_CONTRAST = 1, PHOTO_SIGMA = 2, PHOTO_IMPULSE_P = 3, PHOTO_BLUR_FLAG = 4, PHOTO_BLUR_W = 5,
              PHOTO_ELLIPSES = 14, PHOTO_TRANSPARENCY = PHOTO_ELLIPSES + 5 * PHOTO_MAX_ELLIPSES, PHOTO_KSIZE = PHOTO_TRANSPARENCY + 1,
              PHOTO_KEY = PHOTO_KSIZE + 1, PHOTO_DRAW_STRIDE = PHOTO_KEY + 4;
constexpr int PHOTO_MAX_KSIZE = 351;

struct PhotoParams {
  int brightness, contrast, noise, impulse, motion_blur, shade;
  int max_abs_change, nb_ellipses, ksize_lo, ksize_hi;
  float contrast_lo, contrast_hi, std_lo, std_hi, p_lo, p_hi, t_lo, t_hi;
};

// cv2.BORDER_REFLECT_101 for any distance (a 351-tap kernel is wider than a small image)
__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
  return p;
}

// One thread per image.  Draw order = the reference's: the imgaug chain, then additive_shade line for line
// (utils/photometric.py:88-104).  Neutral values are written for primitives that are off.
__global__ void photo_draw_kernel(uint64_t seed, PhotoParams p, int B, int H, int W, float* __restrict__ draws) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= B) return;
  HsRng rng{hs_mix(hs_mix(seed ^ 0x70686F746F6D6574ull) ^ ((uint64_t)n << 32)), 0};
  float* r = draws + (size_t)n * PHOTO_DRAW_STRIDE;
  // iaa.Add((-c, c)): a discrete uniform integer in [-c, c]
  r[PHOTO_BRIGHTNESS] = p.brightness ? (float)(min((int)(rng.uniform() * (2 * p.max_abs_change + 1)), 2 * p.max_abs_change) - p.max_abs_change) : 0.f;
  r[PHOTO_CONTRAST] = p.contrast ? (float)(p.contrast_lo + rng.uniform() * (p.contrast_hi - p.contrast_lo)) : 1.f;
  r[PHOTO_SIGMA] = p.noise ? (float)(p.std_lo + rng.uniform() * (p.std_hi - p.std_lo)) : 0.f;
  r[PHOTO_IMPULSE_P] = p.impulse ? (float)(p.p_lo + rng.uniform() * (p.p_hi - p.p_lo)) : 0.f;
  float wts[9] = {0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f};
  float flag = 0.f;
  if (p.motion_blur) {
    // iaa.Sometimes(0.5, iaa.MotionBlur(3)): angle in [0, 360), direction in [-1, 1]; the line kernel is the centre column
    // linspace(d, 1 - d, 3) with d = (direction + 1) / 2, rotated about the centre (bilinear, zeros outside), sum 1
    flag = rng.uniform() < 0.5 ? 1.f : 0.f;
    const double ang = rng.uniform() * 360.0 * (3.141592653589793 / 180.0), d = (rng.uniform() * 2.0 - 1.0 + 1.0) * 0.5;
    const double line[3] = {d, 0.5, 1.0 - d};
    const double c = cos(ang), s = sin(ang);
    double sum = 0.0, k[9];
    for (int y = 0; y < 3; ++y)
      for (int x = 0; x < 3; ++x) {
        const double dx = x - 1, dy = y - 1;
        const double sx = c * dx + s * dy + 1.0, sy = -s * dx + c * dy + 1.0;  // source position of the output tap
        const double fx = floor(sx), fy = floor(sy), ax = sx - fx, ay = sy - fy;
        auto at = [&](int yy, int xx) { return (xx == 1 && yy >= 0 && yy < 3) ? line[yy] : 0.0; };
        const int x0 = (int)fx, y0 = (int)fy;
        const double v = at(y0, x0) * (1 - ax) * (1 - ay) + at(y0, x0 + 1) * ax * (1 - ay) + at(y0 + 1, x0) * (1 - ax) * ay +
                         at(y0 + 1, x0 + 1) * ax * ay;
        k[y * 3 + x] = v;
        sum += v;
      }
    for (int i = 0; i < 9; ++i) wts[i] = (float)(k[i] / sum);  // the centre tap is 1/2: sum >= 1/2
  }
  r[PHOTO_BLUR_FLAG] = flag;
  for (int i = 0; i < 9; ++i) r[PHOTO_BLUR_W + i] = wts[i];
  for (int e = 0; e < PHOTO_MAX_ELLIPSES; ++e) {
    float* q = r + PHOTO_ELLIPSES + 5 * e;
    if (p.shade && e < p.nb_ellipses) {
      const double min_dim = (double)min(H, W) / 4.0;
      const int ax = (int)fmax(rng.uniform() * min_dim, min_dim / 5.0), ay = (int)fmax(rng.uniform() * min_dim, min_dim / 5.0);
      const int max_rad = max(ax, ay);
      // np.random.randint(max_rad, size - max_rad): [lo, hi)
      const int nx = max(W - 2 * max_rad, 1), ny = max(H - 2 * max_rad, 1);
      q[0] = (float)(max_rad + min((int)(rng.uniform() * nx), nx - 1));
      q[1] = (float)(max_rad + min((int)(rng.uniform() * ny), ny - 1));
      q[2] = (float)ax;
      q[3] = (float)ay;
      q[4] = (float)(rng.uniform() * 90.0);
    } else {
      q[0] = q[1] = q[4] = 0.f;
      q[2] = q[3] = -1.f;  // unused slot
    }
  }
  float t = 0.f, ks = 0.f;
  if (p.shade) {
    t = (float)(p.t_lo + rng.uniform() * (p.t_hi - p.t_lo));
    const int nk = max(p.ksize_hi - p.ksize_lo, 1);
    int k = p.ksize_lo + min((int)(rng.uniform() * nk), nk - 1);
    if ((k & 1) == 0) k += 1;
    ks = (float)k;
  }
  r[PHOTO_TRANSPARENCY] = t;
  r[PHOTO_KSIZE] = ks;
  for (int i = 0; i < 4; ++i) r[PHOTO_KEY + i] = (float)(unsigned)(hs_mix(rng.key ^ (0xA5A5ull + i)) >> 48);  // 4 x 16 bits
}

__device__ __forceinline__ uint64_t photo_key(const float* __restrict__ r) {
  return (uint64_t)(unsigned)r[PHOTO_KEY] | ((uint64_t)(unsigned)r[PHOTO_KEY + 1] << 16) | ((uint64_t)(unsigned)r[PHOTO_KEY + 2] << 32) |
         ((uint64_t)(unsigned)r[PHOTO_KEY + 3] << 48);
}
__device__ __forceinline__ float photo_u8(float f) { return fminf(fmaxf(rintf(f), 0.f), 255.f); }  // half-to-even, then clip

// stages 1-5 of one pixel: a function of the image, the row and the pixel index only, so that the 3x3 blur can recompute
// its neighbours' post-noise values instead of exchanging them
__device__ __forceinline__ float photo_point(const float* __restrict__ im, int W, int y, int x, float delta, float alpha, float sigma,
                                             float p, uint64_t key) {
  const size_t pix = (size_t)y * W + x;
  const float s = im[pix] * 255.f;
  float v = s >= 255.f ? 255.f : s > 0.f ? floorf(s) : 0.f;
  v = fminf(fmaxf(v + delta, 0.f), 255.f);
  if (alpha != 1.f) v = photo_u8(__fadd_rn(127.f, __fmul_rn(alpha, v - 127.f)));
  if (sigma > 0.f) {
    const uint64_t h = hs_mix(key ^ ((2 * (uint64_t)pix) * 0xD1342543DE82EF95ull));
    const float u1 = ((float)(unsigned)(h >> 40) + 1.f) * (1.f / 16777216.f), u2 = (float)(unsigned)((h >> 16) & 0xFFFFFFu) * (1.f / 16777216.f);
    v = photo_u8(v + sigma * (sqrtf(-2.f * logf(u1)) * cosf(6.2831853f * u2)));
  }
  if (p > 0.f) {
    const uint64_t h = hs_mix(key ^ ((2 * (uint64_t)pix + 1) * 0xD1342543DE82EF95ull));
    const float u1 = (float)(unsigned)(h >> 40) * (1.f / 16777216.f), u2 = (float)(unsigned)((h >> 16) & 0xFFFFFFu) * (1.f / 16777216.f);
    if (u1 < p) {
      const float sn = sinf(1.5707963f * u2);
      v = photo_u8(255.f * sn * sn);
    }
  }
  return v;
}

// stages 1-7; grid (cdiv(H * W, 256), B).  The row is uniform per block (scalar loads).
__global__ void __launch_bounds__(256) photo_pixel_kernel(const float* __restrict__ img, const float* __restrict__ draws,
                                                          float* __restrict__ out, int H, int W) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const float* r = draws + (size_t)n * PHOTO_DRAW_STRIDE;
  const float* im = img + (size_t)n * H * W;
  const float delta = r[PHOTO_BRIGHTNESS], alpha = r[PHOTO_CONTRAST], sigma = r[PHOTO_SIGMA], p = r[PHOTO_IMPULSE_P];
  const uint64_t key = photo_key(r);
  const int y = i / W, x = i - y * W;
  float v;
  if (r[PHOTO_BLUR_FLAG] != 0.f) {
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int yy = reflect101(y + dy - 1, H);
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
        acc += r[PHOTO_BLUR_W + dy * 3 + dx] * photo_point(im, W, yy, reflect101(x + dx - 1, W), delta, alpha, sigma, p, key);
    }
    v = photo_u8(acc);
  } else {
    v = photo_point(im, W, y, x, delta, alpha, sigma, p, key);
  }
  out[(size_t)n * H * W + i] = v / 255.f;
}

// ---- stage 8: the shade.  One workgroup = one image x one strip of TX columns over the FULL height.
// reflect_101 folds the halo of (k - 1) / 2 <= 175 pixels back into the image, and k (100..351) is as large as the image
// itself, so the distinct support of a strip is every row of the image: the strip keeps the row-pass result R[H][TX]
// (fp32) in LDS and runs the column pass from there - nothing of the mask or of R ever reaches HBM.
//   band loop (32 rows at a time):  the ellipse mask is rasterised as BYTES (0 / 1) at the REFLECTED coordinates straight
//       into the extended tile ext[32][TX + 2 * 175] (so the row pass needs no index arithmetic), then
//       R[y][x] = sum_j w[j] * ext[y][x + j]  with RPT rows per thread (one broadcast weight read per RPT products)
//   column pass:  M[y][x] = sum_j w[j] * R[idx[y + j]][x], idx = the reflected row table (uint16, LDS);
//       epilogue  out = clip(v * 255 * (1 - t * M), 0, 255) / 255 in place (a pixel is read and written by its own thread).
// LDS bytes (photo_shade_lds_bytes): 4 H TX + 1408 (weights) + 768 (ellipses) + 2 (H + 352) + 32 (TX + 352):
// 240 x 320 at TX = 32: 46.4 KB (3 workgroups per CU); 480 x 640 takes TX = 16 (46.3 KB); H <= 744 fits the 64 KB a
// workgroup can address at TX = 16.
constexpr int PHOTO_BAND = 32, PHOTO_HALO = (PHOTO_MAX_KSIZE - 1) / 2;
__host__ __device__ constexpr int photo_ext_width(int tx) { return tx + 2 * PHOTO_HALO + 2; }  // multiple of 4 for tx = 16, 32
__host__ __device__ inline size_t photo_shade_lds_bytes(int H, int tx) {
  return (size_t)4 * H * tx + 4 * (PHOTO_MAX_KSIZE + 1) + 4 * 6 * PHOTO_MAX_ELLIPSES + (((size_t)2 * (H + 2 * PHOTO_HALO + 2) + 3) & ~(size_t)3) +
         (size_t)PHOTO_BAND * photo_ext_width(tx);
}

template <int TX>
__global__ void __launch_bounds__(256) photo_shade_kernel(float* __restrict__ io, const float* __restrict__ draws, int H, int W) {
  constexpr int RPT = PHOTO_BAND * TX / 256;  // rows per thread in a band
  constexpr int EXTW = photo_ext_width(TX);
  extern __shared__ __attribute__((aligned(16))) unsigned char photo_smem[];
  const int n = blockIdx.y, x0 = blockIdx.x * TX, tid = threadIdx.x;
  const float* r = draws + (size_t)n * PHOTO_DRAW_STRIDE;
  int k = (int)r[PHOTO_KSIZE];
  if (k < 1) return;  // shade off for this image (uniform per workgroup)
  k = min(k | 1, PHOTO_MAX_KSIZE);
  const int rad = (k - 1) / 2;
  const float t = r[PHOTO_TRANSPARENCY];

  float* R = reinterpret_cast<float*>(photo_smem);
  float* wts = R + (size_t)H * TX;
  float* ell = wts + (PHOTO_MAX_KSIZE + 1);
  unsigned short* idx = reinterpret_cast<unsigned short*>(ell + 6 * PHOTO_MAX_ELLIPSES);
  unsigned char* ext = reinterpret_cast<unsigned char*>(idx) + (((size_t)2 * (H + 2 * PHOTO_HALO + 2) + 3) & ~(size_t)3);

  int n_ell = 0;
  while (n_ell < PHOTO_MAX_ELLIPSES && r[PHOTO_ELLIPSES + 5 * n_ell + 2] >= 0.f) ++n_ell;
  {
    const double sigma = 0.3 * ((k - 1) * 0.5 - 1.0) + 0.8;  // cv2.GaussianBlur(..., 0)
    for (int j = tid; j < k; j += 256) wts[j] = (float)exp(-(double)((j - rad) * (j - rad)) / (2.0 * sigma * sigma));
    if (tid < n_ell) {
      const float* q = r + PHOTO_ELLIPSES + 5 * tid;
      const float a = q[4] * 0.017453292f, ax = q[2], ay = q[3];
      float* e = ell + 6 * tid;
      e[0] = q[0]; e[1] = q[1]; e[2] = cosf(a); e[3] = sinf(a);
      e[4] = ax > 0.f && ay > 0.f ? 1.f / (ax * ax) : 0.f;   // a degenerate ellipse covers nothing
      e[5] = ax > 0.f && ay > 0.f ? 1.f / (ay * ay) : -1.f;
    }
    for (int i = tid; i < H + 2 * rad; i += 256) idx[i] = (unsigned short)reflect101(i - rad, H);
  }
  __syncthreads();
  {
    double s = 0.0;
    for (int j = 0; j < k; ++j) s += (double)wts[j];
    const float inv = (float)(1.0 / s);
    __syncthreads();
    for (int j = tid; j < k; j += 256) wts[j] *= inv;
  }
  const int tx = tid % TX, tg = tid / TX;
  const int extw4 = (TX + 2 * rad + 3) / 4;
  for (int y0 = 0; y0 < H; y0 += PHOTO_BAND) {
    __syncthreads();  // weights ready / the previous band's row pass has finished reading ext
    for (int q = tid; q < PHOTO_BAND * extw4; q += 256) {  // only the TX + 2 * rad columns this kernel size reads
      const int by = q / extw4, i4 = (q - by * extw4) * 4;
      const int y = y0 + by;
      unsigned packed = 0;
      if (y < H) {
        float xs[4];
        bool in[4] = {false, false, false, false};
#pragma unroll
        for (int c = 0; c < 4; ++c) xs[c] = (float)reflect101(x0 - rad + i4 + c, W);
        for (int e = 0; e < n_ell; ++e) {  // one read of the ellipse per four pixels of a row
          const float* el = ell + 6 * e;
          const float cx = el[0], co = el[2], si = el[3], ia = el[4], ib = el[5];
          const float dy = (float)y - el[1];
          const float ys = dy * si, yc = dy * co;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float dx = xs[c] - cx;
            const float xr = dx * co + ys, yr = yc - dx * si;
            in[c] = in[c] || (xr * xr * ia + yr * yr * ib <= 1.f && ib > 0.f);
          }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) packed |= (in[c] ? 1u : 0u) << (8 * c);
      }
      reinterpret_cast<unsigned*>(ext)[by * (EXTW / 4) + (i4 >> 2)] = packed;
    }
    __syncthreads();
    float acc[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) acc[q] = 0.f;
    const unsigned char* e0 = ext + (size_t)(tg * RPT) * EXTW + tx;
#pragma unroll 4
    for (int j = 0; j < k; ++j) {  // (unrolled: several LDS reads in flight per wave - a strip runs at 1-3 waves per SIMD)
      const float wj = wts[j];
#pragma unroll
      for (int q = 0; q < RPT; ++q) acc[q] += wj * (float)e0[q * EXTW + j];
    }
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int y = y0 + tg * RPT + q;
      if (y < H) R[y * TX + tx] = acc[q];
    }
  }
  __syncthreads();
  const int x = x0 + tx;
  float* im = io + (size_t)n * H * W;
  for (int y0 = 0; y0 < H; y0 += PHOTO_BAND) {
    const int yb = y0 + tg * RPT;
    float acc[RPT];
    int row[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      acc[q] = 0.f;
      row[q] = min(yb + q, H - 1);  // rows past the image recompute the last one and are not stored
    }
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
      const float wj = wts[j];
#pragma unroll
      for (int q = 0; q < RPT; ++q) acc[q] += wj * R[(int)idx[row[q] + j] * TX + tx];
    }
    if (x < W) {
#pragma unroll
      for (int q = 0; q < RPT; ++q) {
        const int y = yb + q;
        if (y < H) {
          const float v = im[(size_t)y * W + x] * 255.f;
          im[(size_t)y * W + x] = fminf(fmaxf(v * (1.f - t * acc[q]), 0.f), 255.f) / 255.f;
        }
      }
    }
  }
}

}  // namespace sspk
