// Winograd F(2x2, 3x3) on the fp32 matrix cores: the constants and staging helpers that the forward / data-gradient kernels
// share (conv_wino_pipe.hip.h, conv_wino_p2.hip.h, conv_wino4.hip.h), the F(3x3, 2x2) weight gradient and the reductions of
// its partial slabs.
//
//   Y(2x2) = A^T [ sum_ci (G g G^T) (.) (B^T d B) ] A        d: 4x4 input patch, g: 3x3 filter   (Lavin & Gray 2016)
//
// 16 multiplies per 2x2 outputs instead of 36, i.e. 2.25x fewer MFMA FLOPs than the direct implicit GEMM of conv_mfma_kernel
// for the same (algorithmic) convolution, still in fp32 arithmetic throughout (the transforms only add and halve).
#pragma once
#include <type_traits>
#include "conv_mfma.hip.h"

namespace sspk {

constexpr int WC = 16;                          // Winograd components
constexpr int WTILES = 64;                      // 2x2-output tiles per block
constexpr int WB_FLOATS = WC * CK * NB;         // transformed weights of a 16-channel chunk x 64 output channels (64 KB)
constexpr int WHALO = 340;                      // (8+2) x (32+2) = (32+2) x (8+2) raw halo pixels
constexpr int WINO_THREADS = 512;

// relu(v * scale + shift) of a loaded quad, 0 for zero-padding pixels: two packed fmas + one v_med3 per element
// (clamp to [0, +inf] or, for padding, to [0, 0]) instead of fma + max + select, on the staging path of the MFMA loop
__device__ __forceinline__ f32x4 bn_relu_quad(f32x4 v, f32x4 sc, f32x4 sh, bool padding) {
  const float hi = padding ? 0.f : __builtin_inff();
  v = pk4_fma(v, sc, sh);
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_fmed3f(v[e], 0.f, hi);
  return v;
}

// ------------------------------------------------------------------------------------------------
// Winograd weight gradient F(3x3, 2x2) (the transpose of F(2x2, 3x3)):
//   dW(3x3) = G^T [ sum over 2x2-output tiles (B^T d B) (.) (A dy A^T) ] G      d: 4x4 input patch, dy: 2x2 dY tile
// 16 multiplies per tile and (ci, co) instead of 36.  The 16 component products are GEMMs over K = tiles:
// block = 8 waves, owns a 64 ci x 64 co slab of all 16 components (wave = (co half, component row i): 4 components x
// 2 M-tiles = 128 accumulator registers) and walks a contiguous range of 128-pixel block tiles (32 Winograd tiles) of
// BOTH views.  LDS holds only the RAW input halo and dY tile ([pixel][64 channels], BatchNorm + ReLU of the producer
// applied on the way in); both transforms run in registers between the LDS reads and the MFMAs:
//   lane (li, lh): k = lh selects the tile of the pair, one ds_read_b64 gives channels 2 li, 2 li + 1 = the rows li of
//   M-tiles 0 / 1;  T[i][c] = d[ra][c] +- d[rb][c],  V[i][j] from T[i][0..3];  D[i][j] from the 2x2 dY values of co.
// The partial slabs [block][component][ci][co] are summed over the splits, transformed with G^T . G and accumulated
// into the OIHW gradient by wgrad_wino_reduce_kernel.
// ------------------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <bool WIDE>
struct WgradWinoGeom {
  static constexpr int TH = WIDE ? 4 : 16, TW = WIDE ? 32 : 8;  // 128 output pixels = 32 tiles per step
  static constexpr int TTX = TW / 2;
  static constexpr int HT = TH + 2, WT = TW + 2;
  static constexpr int X_FLOATS = HT * WT * 64, D_FLOATS = TH * TW * 64;
  static constexpr int LDS_BYTES = (X_FLOATS + D_FLOATS + 256) * 4;
};

// The 16 K-steps (32 Winograd tiles, lane half lh = tile of the pair) of one block tile, fully unrolled: every LDS offset
// is base + compile-time constant (the halo rows ra / rb of the wave's component row are folded into the lane bases) and
// all two-wide arithmetic is written on f32x2 so that it compiles to v_pk_fma_f32 / v_pk_add_f32: 13 VALU instructions per
// 8 MFMAs instead of ~34.  On this chip every VALU instruction beside a v_mfma_f32_32x32x2_f32 costs matrix-pipe time one
// for one (the fp32 MFMA executes on the vector ALUs: DESIGN.md section 8, tools/ubench/mfma_overlap.hip).
//   T[c] = d[ra][c] + sg d[rb][c];   (r0, r1) = c0 dy[0][0..1] + c1 dy[1][0..1]
struct WgsNoHook {
  template <typename S> __device__ __forceinline__ void operator()(S) const {}
};
// `hook(std::integral_constant<int, S>)` runs behind the LDS reads of step S, in the shadow of its first MFMA (wgrad_wino_fused_kernel
// issues the next tile's global loads there, two per step)
template <typename G, typename HOOK = WgsNoHook>
__device__ __forceinline__ void wgrad_wino_steps(f32x16 (&acc)[4][2], const float* __restrict__ xa0,
                                                 const float* __restrict__ xb0, const float* __restrict__ db0,
                                                 const f32x2 sg, const f32x2 c0, const f32x2 c1, HOOK&& hook = HOOK()) {
  f32x2 U[4], Wv[4], T[4], top, bot, r;
#define WGS_LOAD(S)                                                                                          \
  {                                                                                                          \
    constexpr int t0_ = 2 * (S);  /* even tile of the pair; the odd one (lh = 1) is folded into the lane bases */ \
    constexpr int ty_ = t0_ / G::TTX, tx_ = t0_ % G::TTX;                                                    \
    constexpr int xo_ = ((2 * ty_) * G::WT + 2 * tx_) * 64, do_ = ((2 * ty_) * G::TW + 2 * tx_) * 64;        \
    _Pragma("unroll") for (int c = 0; c < 4; ++c) {                                                          \
      U[c] = *reinterpret_cast<const f32x2*>(xa0 + xo_ + c * 64);                                            \
      Wv[c] = *reinterpret_cast<const f32x2*>(xb0 + xo_ + c * 64);                                           \
    }                                                                                                        \
    top[0] = db0[do_]; top[1] = db0[do_ + 64];                                                               \
    bot[0] = db0[do_ + G::TW * 64]; bot[1] = db0[do_ + G::TW * 64 + 64];                                     \
  }
  // first half of a step: consumes the raw operands (their registers are free for the next step's LDS reads)
#define WGS_HEAD()                                                                                           \
  {                                                                                                          \
    _Pragma("unroll") for (int c = 0; c < 4; ++c) T[c] = pk_fma(sg, Wv[c], U[c]);                   \
    r = pk_fma(c1, bot, pk_mul(c0, top));                                                                   \
  }
  // second half: the operands of the 8 MFMAs, the first MFMA, then - in ITS shadow - the LDS reads of step s + 1 and the hook's
  // global loads (a non-VALU instruction directly behind an MFMA issues for free while the matrix pipe is busy; in front of the
  // group, where they stood until round 6, each of the 8 cost ~5 cycles: PERF_LOG round 6 section 0), then the other 7 MFMAs.
  // The reads land under those 7 (448 cycles).
#define WGS_STEP(S)                                                                                          \
  WGS_HEAD()                                                                                                 \
  {                                                                                                          \
    const f32x2 V0 = pk_sub(T[0], T[2]), V1 = pk_add(T[1], T[2]), V2 = pk_sub(T[2], T[1]), V3 = pk_sub(T[1], T[3]); \
    const float D0 = r[0], D1 = r[0] + r[1], D2 = r[0] - r[1], D3 = -r[1];                                   \
    /* hipcc does not track the VALU-write -> MFMA-read wait states (2) for registers written by inline asm: */ \
    /* all operands are complete before the fence, the first MFMA reads V0, written >= 3 instructions earlier */ \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(V0[0], D0, acc[0][0], 0, 0, 0);                         \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    if ((S) + 1 < 16) WGS_LOAD(((S) + 1 < 16 ? (S) + 1 : 0))                                                 \
    hook(std::integral_constant<int, (S)>{});                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(V0[1], D0, acc[0][1], 0, 0, 0);                         \
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(V1[0], D1, acc[1][0], 0, 0, 0);                         \
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(V1[1], D1, acc[1][1], 0, 0, 0);                         \
    acc[2][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(V2[0], D2, acc[2][0], 0, 0, 0);                         \
    acc[2][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(V2[1], D2, acc[2][1], 0, 0, 0);                         \
    acc[3][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(V3[0], D3, acc[3][0], 0, 0, 0);                         \
    acc[3][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(V3[1], D3, acc[3][1], 0, 0, 0);                         \
  }                                                                                                          \
  __builtin_amdgcn_sched_barrier(0);
  WGS_LOAD(0)
  WGS_STEP(0) WGS_STEP(1) WGS_STEP(2) WGS_STEP(3) WGS_STEP(4) WGS_STEP(5) WGS_STEP(6) WGS_STEP(7)
  WGS_STEP(8) WGS_STEP(9) WGS_STEP(10) WGS_STEP(11) WGS_STEP(12) WGS_STEP(13) WGS_STEP(14) WGS_STEP(15)
#undef WGS_LOAD
#undef WGS_HEAD
#undef WGS_STEP
}

template <int IN_MODE, bool WIDE>
__global__ __launch_bounds__(512) void wgrad_wino_kernel(const WgradArgs a) {
  using G = WgradWinoGeom<WIDE>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sX = smem;
  float* sD = smem + G::X_FLOATS;
  float* sS = smem + G::X_FLOATS + G::D_FLOATS;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar wave roles
  const int li = lane & 31, lh = lane >> 5;
  const int coh = wave & 1, irow = wave >> 1;

  int bid = blockIdx.x;
  const int split = bid % a.nsplit;
  bid /= a.nsplit;
  const int cob = bid % a.ncob;
  const int cib = bid / a.ncob;
  const int tot_tiles = a.ntiles * a.nprob;
  const int per = (tot_tiles + a.nsplit - 1) / a.nsplit;
  const int t_begin = split * per, t_end = min(tot_tiles, t_begin + per);

  f32x16 acc[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][e][r] = 0.f;

  const int q16 = tid & 15;
  const int ci0 = cib * 64 + q16 * 4;
  const bool civalid = ci0 < a.Cin;
  if (IN_MODE != 0 && tid < 32) {
    const int pr = tid >> 4;
    f32x4 sc0 = {1.f, 1.f, 1.f, 1.f}, sh0 = {0.f, 0.f, 0.f, 0.f};
    if (civalid && pr < a.nprob) {
      sc0 = *reinterpret_cast<const f32x4*>((pr ? a.in_scale2 : a.in_scale) + ci0);
      sh0 = *reinterpret_cast<const f32x4*>((pr ? a.in_shift2 : a.in_shift) + ci0);
    }
    *reinterpret_cast<f32x4*>(sS + pr * 128 + q16 * 4) = sc0;
    *reinterpret_cast<f32x4*>(sS + pr * 128 + 64 + q16 * 4) = sh0;
  }
  const int co0 = cob * 64 + q16 * 4;
  const bool covalid = co0 < a.Cout;

  constexpr int NX = (G::HT * G::WT + 31) / 32;  // halo pixels per thread (pp = (tid >> 4) + 32 i)
  constexpr int ND = G::TH * G::TW / 32;
  f32x4 xreg[NX], dreg[ND];
  unsigned xmask = 0;

  const int xpix = a.in_cs * 4, xrow = a.W * xpix, dpix = a.dout_cs * 4, drow = a.W * dpix;
  const int xq = civalid ? (a.in_co + ci0) * 4 : -1, dq = covalid ? (a.dout_co + co0) * 4 : -1;
  constexpr unsigned OOB = 0x80000000u;
  // byte offsets of this thread's staging slots (slot i = pixel (tid >> 4) + 32 i of the halo / dY raster) relative to
  // the first halo / dY pixel of a tile; OOB for slots past the raster and for channel quads outside the tensor.
  // Tiles whose halo lies inside the image (3/4 of them at 240x320) add the tile origin as the SCALAR offset of the
  // buffer load: no per-slot address arithmetic in the MFMA phase (it cost ~90 VALU instructions per tile and thread).
  unsigned xoffv[NX], doffv[ND];
  unsigned xmask_in = 0;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const int pp = (tid >> 4) + 32 * i, r = pp / G::WT, c = pp - r * G::WT;
    const bool ok = xq >= 0 && pp < G::HT * G::WT;
    xoffv[i] = ok ? (unsigned)(r * xrow + c * xpix + xq) : OOB;
    xmask_in |= (ok ? 1u : 0u) << i;
  }
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    const int pp = (tid >> 4) + 32 * i, r = pp / G::TW, c = pp - r * G::TW;
    doffv[i] = dq >= 0 ? (unsigned)(r * drow + c * dpix + dq) : OOB;
  }
  bool cur_inside = false, nxt_inside = false;  // wave-uniform: the staged / the prefetched tile is an interior tile
  // one buffer descriptor per image (32-bit offsets inside it); an offset beyond num_records returns 0
#define WGW_ISSUE(TILE)                                                                                       \
  if (!(a.ablate & 1)) {                                                                                      \
    const int pr_ = (TILE) >= a.ntiles ? 1 : 0;                                                               \
    const int tl_ = (TILE) - pr_ * a.ntiles;                                                                  \
    const int tx_ = tl_ % a.tiles_x, t2_ = tl_ / a.tiles_x;                                                   \
    const int ty0_ = (t2_ % a.tiles_y) * G::TH, tx0_ = tx_ * G::TW, n_ = t2_ / a.tiles_y;                     \
    const __amdgpu_buffer_rsrc_t rx_ = __builtin_amdgcn_make_buffer_rsrc(                                     \
        const_cast<float*>(pr_ ? a.in2 : a.in) + (size_t)n_ * a.H * a.W * a.in_cs, 0, a.H * xrow, 0x00020000); \
    const __amdgpu_buffer_rsrc_t rd_ = __builtin_amdgcn_make_buffer_rsrc(                                     \
        const_cast<float*>(pr_ ? a.dout2 : a.dout) + (size_t)n_ * a.H * a.W * a.dout_cs, 0, a.H * drow, 0x00020000); \
    nxt_inside = ty0_ >= 1 && ty0_ + G::TH + 1 <= a.H && tx0_ >= 1 && tx0_ + G::TW + 1 <= a.W;               \
    if (nxt_inside) {                                                                                         \
      const int xb_ = (ty0_ - 1) * xrow + (tx0_ - 1) * xpix, db_ = ty0_ * drow + tx0_ * dpix;                 \
      _Pragma("unroll") for (int i = 0; i < NX; ++i)                                                          \
        xreg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx_, xoffv[i], xb_, 0));    \
      _Pragma("unroll") for (int i = 0; i < ND; ++i)                                                          \
        dreg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rd_, doffv[i], db_, 0));    \
      xmask = xmask_in;                                                                                       \
    } else {                                                                                                  \
      xmask = 0;                                                                                              \
      _Pragma("unroll") for (int i = 0; i < NX; ++i) {                                                        \
        const int pp_ = (tid >> 4) + 32 * i, r_ = pp_ / G::WT, c_ = pp_ - r_ * G::WT;                         \
        const int gy = ty0_ - 1 + r_, gx = tx0_ - 1 + c_;                                                     \
        const bool ok = xq >= 0 && pp_ < G::HT * G::WT && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W; \
        xreg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(                            \
            rx_, ok ? (unsigned)(gy * xrow + gx * xpix + xq) : OOB, 0, 0));                                   \
        xmask |= (ok ? 1u : 0u) << i;                                                                         \
      }                                                                                                       \
      _Pragma("unroll") for (int i = 0; i < ND; ++i) {                                                        \
        const int pp_ = (tid >> 4) + 32 * i, r_ = pp_ / G::TW, c_ = pp_ - r_ * G::TW;                         \
        const int gy = ty0_ + r_, gx = tx0_ + c_;                                                             \
        const bool ok = dq >= 0 && gy < a.H && gx < a.W;                                                      \
        dreg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(                            \
            rd_, ok ? (unsigned)(gy * drow + gx * dpix + dq) : OOB, 0, 0));                                   \
      }                                                                                                       \
    }                                                                                                         \
  }

  // per-wave constants of component row i:  T[i][c] = d[ra][c] + sg d[rb][c];  R[q] = c0 dy[0][q] + c1 dy[1][q]
  const int ra = irow == 0 ? 0 : irow == 2 ? 2 : 1;
  const int rb = irow == 2 ? 1 : irow == 3 ? 3 : 2;
  const float sg = irow == 1 ? 1.f : -1.f;
  const float c0 = irow == 3 ? 0.f : 1.f;
  const float c1 = irow == 0 ? 0.f : irow == 1 ? 1.f : -1.f;

  if (t_begin < t_end) WGW_ISSUE(t_begin)
  for (int tile = t_begin; tile < t_end; ++tile) {
    __syncthreads();  // all waves finished reading the previous tile's LDS image
    cur_inside = nxt_inside;
    if (!(a.ablate & 2)) {
      const int cur_prob = tile >= a.ntiles ? 1 : 0;
      f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
      if (IN_MODE != 0) {
        sc = *reinterpret_cast<const f32x4*>(sS + cur_prob * 128 + q16 * 4);
        sh = *reinterpret_cast<const f32x4*>(sS + cur_prob * 128 + 64 + q16 * 4);
      }
      if (IN_MODE != 0 && cur_inside) {
        // interior tile: no zero padding anywhere (channel quads outside the tensor carry scale 1 / shift 0 and load 0)
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          const int pp = (tid >> 4) + 32 * i;
          if (pp < G::HT * G::WT) {
            f32x4 v = pk4_fma(xreg[i], sc, sh);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            *reinterpret_cast<f32x4*>(sX + pp * 64 + q16 * 4) = v;
          }
        }
      } else {
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int pp = (tid >> 4) + 32 * i;
        if (pp < G::HT * G::WT) {
          f32x4 v = xreg[i];  // 0 from the buffer load where the pixel / channel quad is outside
          if (IN_MODE != 0) v = bn_relu_quad(v, sc, sh, !((xmask >> i) & 1u));
          *reinterpret_cast<f32x4*>(sX + pp * 64 + q16 * 4) = v;
        }
      }
      }
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        const int pp = (tid >> 4) + 32 * i;
        *reinterpret_cast<f32x4*>(sD + pp * 64 + q16 * 4) = dreg[i];  // 0 where outside
      }
    }
    __syncthreads();
    {
      const int nxt = min(tile + 1, t_end - 1);  // unconditional prefetch (redundant on the last tile)
      WGW_ISSUE(nxt)
      __builtin_amdgcn_sched_barrier(0);
    }
    if (!(a.ablate & 8)) {
      // lane bases: channel pair 2 li of the raw rows ra / rb, tile column offset of the lane half; dY column of this lane
      const float* xa0 = sX + (ra * G::WT + 2 * lh) * 64 + 2 * li;
      const float* xb0 = sX + (rb * G::WT + 2 * lh) * 64 + 2 * li;
      const float* db0 = sD + (2 * lh) * 64 + coh * 32 + li;
      wgrad_wino_steps<G>(acc, xa0, xb0, db0, f32x2{sg, sg}, f32x2{c0, c0}, f32x2{c1, c1});
    }
  }
#undef WGW_ISSUE
  // partial slab: [blk][component][ci 64][co 64]; M-tile e, row m <-> input channel 2 m + e
  float* dst = a.partial + (size_t)blockIdx.x * WC * 4096;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * lh;
        dst[(irow * 4 + j) * 4096 + (2 * m + e) * 64 + coh * 32 + li] = acc[j][e][r];
      }
}

// Sums the 16-component partial slabs over the splits, applies dW = G^T M G and ACCUMULATES into the OIHW gradient.
// block = 256 threads = 64 consecutive co x 4 split groups, one input channel per block row.
__device__ __forceinline__ void wgrad_wino_reduce_block(const float* __restrict__ partial, float* __restrict__ dw, int Cin,
                                                        int Cout, int ncob, int nsplit, int bid, float (*red)[WC][64]) {
  const int o = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int cob = bid % ncob, ci = bid / ncob;
  const int co = cob * 64 + o, cib = ci >> 6;
  float m[WC];
#pragma unroll
  for (int c = 0; c < WC; ++c) m[c] = 0.f;
  const float* src = partial + (size_t)((cib * ncob + cob) * nsplit) * WC * 4096 + (ci & 63) * 64 + o;
  for (int k = grp; k < nsplit; k += 4)
#pragma unroll
    for (int c = 0; c < WC; ++c) m[c] += src[((size_t)k * WC + c) * 4096];
#pragma unroll
  for (int c = 0; c < WC; ++c) red[grp][c][o] = m[c];
  __syncthreads();
  if (grp != 0 || co >= Cout) return;
#pragma unroll
  for (int c = 0; c < WC; ++c) m[c] = (red[0][c][o] + red[1][c][o]) + (red[2][c][o] + red[3][c][o]);
  float p[3][4];  // P = G^T M
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[0][j] = m[0 * 4 + j] + 0.5f * (m[1 * 4 + j] + m[2 * 4 + j]);
    p[1][j] = 0.5f * (m[1 * 4 + j] - m[2 * 4 + j]);
    p[2][j] = 0.5f * (m[1 * 4 + j] + m[2 * 4 + j]) + m[3 * 4 + j];
  }
  float* out = dw + ((size_t)co * Cin + ci) * 9;
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    out[u * 3 + 0] += p[u][0] + 0.5f * (p[u][1] + p[u][2]);
    out[u * 3 + 1] += 0.5f * (p[u][1] - p[u][2]);
    out[u * 3 + 2] += 0.5f * (p[u][1] + p[u][2]) + p[u][3];
  }
}

__global__ __launch_bounds__(256) void wgrad_wino_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw,
                                                                int Cin, int Cout, int ncob, int nsplit) {
  __shared__ float red[4][WC][64];
  wgrad_wino_reduce_block(partial, dw, Cin, Cout, ncob, nsplit, blockIdx.x, red);
}

// The reductions of ALL Winograd weight-gradient launches of a backward pass in one launch (each wgrad launch keeps its
// own slice of the partial-slab buffer until then): 9 launches of ~20 us less per step.
struct WredJob {
  const float* partial;
  float* dw;
  int cin, cout, ncob, nsplit;
  int nblocks;  // blocks of the job: ncob * cin (f4 == 2: three times as many)
  int block0;
  int f4;  // 0: 16-component slabs of wgrad_wino_kernel (ncob = 64-channel blocks); 1: 9-tap slabs [9][64][32] of
           // wgrad_wino4_kernel, already through G^T . G (ncob = 32-channel blocks); 2: 12-component slabs [4][3][64][64] of
           // wgrad_wino_fused_kernel (right-hand product applied)
};

// wgrad_wino4_kernel's partial slabs [pair * nsplit + k][9 taps][64 ci][32 co] summed over the splits and ACCUMULATED into
// the OIHW gradient.  block = 256 threads = 32 consecutive co x 8 split groups, one input channel per block.
__device__ __forceinline__ void wgrad_wino4_reduce_block(const float* __restrict__ partial, float* __restrict__ dw, int Cin,
                                                         int Cout, int ncob, int nsplit, int bid, float* red) {
  const int o = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int cob = bid % ncob, ci = bid / ncob;
  const int co = cob * 32 + o, cib = ci >> 6;
  float m[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) m[t] = 0.f;
  const float* src = partial + (size_t)((cib * ncob + cob) * nsplit) * (9 * 2048) + (ci & 63) * 32 + o;
  for (int k = grp; k < nsplit; k += 8)
#pragma unroll
    for (int t = 0; t < 9; ++t) m[t] += src[((size_t)k * 9 + t) * 2048];
#pragma unroll
  for (int t = 0; t < 9; ++t) red[(grp * 9 + t) * 32 + o] = m[t];
  __syncthreads();
  if (grp != 0 || co >= Cout) return;
  float* out = dw + ((size_t)co * Cin + ci) * 9;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) s += red[(g * 9 + t) * 32 + o];
    out[t] += s;
  }
}
__global__ __launch_bounds__(256) void wgrad_wino4_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw,
                                                                 int Cin, int Cout, int ncob, int nsplit) {
  __shared__ float red[8 * 9 * 32];
  wgrad_wino4_reduce_block(partial, dw, Cin, Cout, ncob, nsplit, blockIdx.x, red);
}

// wgrad_wino_fused_kernel's slabs [(cib * ncob + cob) * nsplit + k][row i 4][x 3][64 ci][64 co] (the right-hand product of
// dW = G^T M G applied by the workgroup) summed over the splits, the left-hand product, ACCUMULATED into the OIHW gradient.
// block = one input channel, 64 consecutive co, ONE column x of the taps (the left-hand product mixes the rows i of a column only:
// three blocks per (ci, cob) pair without an exchange); 256 threads = 16 co quads (16-byte loads) x 16 split groups - a 64 x 64
// layer has 256 splits and only 64 pairs, so the splits, not the pairs, have to carry the parallelism.
__device__ __forceinline__ void wgrad_fused12_reduce_block(const float* __restrict__ partial, float* __restrict__ dw, int Cin,
                                                           int Cout, int ncob, int nsplit, int rel, float* red) {
  const int q = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int x = rel % 3, bid = rel / 3;
  const int cob = bid % ncob, ci = bid / ncob, cib = ci >> 6;
  float4 m[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* src = partial + (size_t)((cib * ncob + cob) * nsplit) * (12 * 4096) + x * 4096 + (ci & 63) * 64 + q * 4;
  for (int k = grp; k < nsplit; k += 16)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(src + ((size_t)k * 12 + i * 3) * 4096);
      m[i].x += v.x; m[i].y += v.y; m[i].z += v.z; m[i].w += v.w;
    }
#pragma unroll
  for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(red + ((grp * 4 + i) * 16 + q) * 4) = m[i];   // [grp 16][i 4][co 64]
  __syncthreads();
  const int o = threadIdx.x & 63, u = threadIdx.x >> 6, co = cob * 64 + o;
  if (u == 3 || co >= Cout) return;
  float r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int g = 0; g < 16; g += 2) { a0 += red[((g * 4 + i) * 64) + o]; a1 += red[(((g + 1) * 4 + i) * 64) + o]; }
    r[i] = a0 + a1;
  }
  const float v = u == 0 ? r[0] + 0.5f * (r[1] + r[2]) : u == 1 ? 0.5f * (r[1] - r[2]) : 0.5f * (r[1] + r[2]) + r[3];
  dw[((size_t)co * Cin + ci) * 9 + u * 3 + x] += v;
}
__global__ __launch_bounds__(256) void wgrad_fused12_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw,
                                                                   int Cin, int Cout, int ncob, int nsplit) {
  __shared__ __attribute__((aligned(16))) float red[4 * WC * 64];
  wgrad_fused12_reduce_block(partial, dw, Cin, Cout, ncob, nsplit, blockIdx.x, red);
}

constexpr int WRED_MAX_JOBS = 16;
struct WredJobs {
  int n;
  WredJob j[WRED_MAX_JOBS];
};
// (wgrad_wino_reduce_multi_kernel, the launch that runs these jobs, lives in backward_tail.hip.h beside the other tail reductions)

}  // namespace sspk
