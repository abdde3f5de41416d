"""GPU: layer-exact, teacher-forced checks of the fp32 BACKWARD of a training pair step.

After one pair step with the backward taps on (Engine.debug_backward_taps: per layer and view, dOut = the gradient wrt the
layer's (pooled) activation as it enters its BatchNorm backward, dY = the gradient wrt its conv output after the APPLY pass),
every stage of the backward is recomputed in fp64 from the HIP path's OWN inputs to that stage, so a bug shows in the stage
that has it:

  * APPLY (BatchNorm + ReLU (+ 2x2 max-pool) backward): z = fma(Y, scale, shift) in fp32 as the forward test forms it,
    G = route(dOut) * [z > 0], dY = gamma * invstd * (G - S1 / n - xhat * S2 / n), S1 = sum G, S2 = sum G * xhat per view,
    xhat from the engine's own mean / invstd.  Routing rule of every APPLY kernel (bn_bwd_kernel, wgrad_wino_fused_kernel):
    the pooled gradient goes to the FIRST arg-max of relu(z) in window scan order (strictly greater replaces): torch's
    max_pool2d indices on the fp32 activation, which this test uses.  For gamma > 0 that is the raw-Y maximum, for gamma < 0
    the minimum (ties in z aside); for gamma == 0, z == beta in the whole window and the first element takes it (the pool_fix
    scan of bn_bwd_sums_kernel), gated off for beta <= 0.
    Bound per element: tau * |gamma| * invstd * (|G| + sum|G| / n + |xhat| * sum|G * xhat| / n).
  * BatchNorm parameters: grad gamma = sum_v S2_v, grad beta = sum_v S1_v (bound tau * sum of the absolute terms); the conv bias
    of a BatchNorm-fed conv = sum_v sum dY_v of the TAPS (bound tau * sum |dY|).
  * Weight gradient: dW = sum_v conv2d_weight(A_v, dY_v), A_v the forward operand rebuilt from the stored Y of the layer below,
    dY_v the tap; bound tau * sum_v conv2d_weight(|A_v|, |dY_v|).  Layer 0: A = the image, dY = the fp64 APPLY result from the
    dOut_0 tap (dY_0 is never stored), bound from the APPLY bound.  At B = 32 a listed subset of output channels.
  * Data gradient: the dOut tap of the layer below = conv2d_input(W, dY) (the 3x3 heads: one sum over the concatenated
    [Pa | Da | DS] channels), bound tau * conv2d_input(|W|, |dY|), on the images [0, 1, B/2, B-2, B-1] at B = 32.
  * Heads: Pb / Db (BatchNorm without ReLU) from the dsemi / ddesc roots, the grouped pointwise weight and data gradients,
    Sout's bias = the column sums of dsout.  The roots themselves are pinned element by element by
    tests/test_gpu_loss_exact.py.

Every case asserts the per-layer route record of the backward (ssp_debug_backward_tap) against a mirror of the dispatch
predicates, and that taps on / off give bit-identical results under set_deterministic(True).

Algorithm 11 (wgrad_wino4_kernel, F(3x3,4x4)) leaves a map that fits into one 128-pixel block tile to the weight gradient of
algorithm 1 (launch_wgrad): on the 2x3 and 4x6 maps of [ssp-B2-16x24-algo11] F(3x3,4x4) gave non-zero values (<= 1.0e-7, max |dW|
0.45) to 7209 elements whose bound is exactly 0 and ratios up to 2.2e-2, as does a plain numpy fp32 restatement of the transform
(7250 elements, 6.5e-2): the case failed before that change.  DESIGN.md section 33."""
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref as C
from tests.gate_util import _dev, _engine
from tests.exact_sweep_cases import SWEEP_CASES
from tests.test_gpu_layer_exact import _f2x2, _inputs, _kernel, _sd_tensor

pytestmark = pytest.mark.gpu

# tau per family: 4 x the worst ratio |got - fp64| / bound measured on the MI355X over every case of this module (both views)
TAU = {
    "apply_separate": 4 * 2.05e-7,   # bn_bwd_kernel (and the pointwise heads' paired launch): measured 2.042e-7 (convPb, B = 3)
    "apply_fused12": 4 * 1.73e-7,    # wgrad_wino_fused_kernel's APPLY: measured 1.724e-7 (convDS, B = 32)
    "bn_sums": 4 * 3.45e-7,          # grad gamma / beta / conv bias / Sout's column sums: measured 3.443e-7 (convPb.bias, algo 11)
    "dx_wino4": 4 * 1.48e-5,         # conv_wino4_kernel, F(4x4,3x3): measured 1.198e-5 / 1.478e-5 in two runs (atomics order), at
                                     # the maps' last pixels (the output transform's largest coefficients; forward: 4.4e-6)
    "dx_pipe": 4 * 4.25e-7,          # conv_wino_pipe_kernel: measured 4.246e-7
    "dx_p2": 4 * 7.83e-7,            # conv_wino_p2_kernel: measured 7.820e-7 (the 3x3 heads' 768-channel sum)
    "dx_direct": 4 * 8.58e-7,        # conv_mfma_kernel (algorithm 0): measured 8.572e-7
    "dx_grouped": 4 * 7.03e-7,       # conv1x1_group_kernel: measured 7.026e-7
    "dw_fused12": 4 * 4.13e-7,       # wgrad_wino_fused_kernel + the deferred multi-job reduce: measured 4.126e-7 (algo 10)
    # the same kernel on a map that fits into ONE of its tiles (16x8 / 4x32; the 4x6 level of the 16x24 case): a sum of at most
    # 2 B x 32 Winograd tiles per element, whose rounding is relative to the transformed 4x4 tiles, not to the one tap's |A| (*) |dY|
    # (behind a pooling layer three of four dY pixels carry only the small -S1/n - xhat S2/n term).  4 x the worst ratio of a plain
    # numpy fp32 restatement of F(3x3,2x2) on the same tensors, 3.296e-5 (the kernel: 1.40e-5 .. 2.57e-5 in four runs, its atomics'
    # order; there 1.41e-5); plain fp32 accumulation of the nine taps: 2.4e-7.  DESIGN.md section 33
    "dw_fused12_sub_tile": 4 * 3.30e-5,
    "dw_wino_sub_tile": 4 * 3.30e-5,   # wgrad_wino_kernel, the same F(3x3,2x2) without the APPLY: algorithm 11 on such a map (launch_wgrad)
    # wgrad_wino4_kernel, F(3x3,4x4): 4 x the worst ratio of a plain numpy fp32 restatement of the transposed F(4x4,3x3) algorithm on
    # the tensors of the 256x24 case (32x3 cells), 3.517e-5; the kernel there: 2.16e-5 / 3.68e-5 in two runs.  Was 4 x 4.968e-6,
    # the kernel's own ratio at 64x96 (the restatement there: 4.39e-6).  DESIGN.md section 33
    "dw_wino4": 4 * 3.52e-5,
    "dw_direct": 4 * 2.25e-7,        # wgrad_mfma_kernel: measured 2.244e-7
    "dw_grouped": 4 * 3.70e-7,       # wgrad1x1_group_kernel: measured 3.696e-7
    "dw_l0": 4 * 9.81e-9,            # bn_bwd_apply_l0_kernel (bound from the APPLY bound, not |dY_0|): measured 9.810e-9
}
# (the plain wgrad_wino_kernel runs only under algorithm 11 on an even map inside one tile: every even map fuses its APPLY under
# algorithms 1 / 10; a route that names a family without a tau fails with a KeyError)

WG = {1: "fused12", 2: "wino", 3: "wino4", 4: "direct", 5: "grouped", 6: "l0"}
DG = {1: "wino4", 2: "pipe", 3: "p2", 4: "direct", 5: "grouped"}
L_PA, L_PB, L_DA, L_DB, L_DS, L_SOUT = 8, 9, 10, 11, 12, 13
POOLED = (1, 3, 5)


def _cdiv(a, b):
    return -(-a // b)


def _decode(r):
    return (bool(r & 1), bool(r & 2), bool(r & 4), WG.get((r >> 4) & 15), DG.get((r >> 8) & 15))


def _res(l, H, W):
    s = 0 if l < 2 else 1 if l < 4 else 2 if l < 6 else 3
    return H >> s, W >> s


def _predict_routes(arch, algo, B, H, W, n_cu=None):
    """Route record per layer: (bsums_fused, apply_fused, sums_lazy, wgrad kernel, dgrad kernel).  A mirror of csrc/ssp.hip:
    bn_layer_backward's branches, wgrad_can_fuse_apply, setup_bnr / can_fuse_bnr (every Winograd data gradient of the fp32
    pipelined algorithms), launch_wgrad's kernel choice, pack_all's w4_eligible for the data-gradient images (_kernel with the
    channel counts swapped) and conv_uses_p2; the pointwise heads ride the grouped launches whenever the algorithm is not 0."""
    t = C.layer_table(arch)
    nheads = 3 if arch.endswith("ssmall") else 2
    Hc, Wc = H // 8, W // 8
    fuse_ok = lambda h, w, c: algo in (1, 10) and h % 2 == 0 and w % 2 == 0 and c % 4 == 0   # wgrad_can_fuse_apply
    bnr = algo != 0   # can_fuse_bnr
    out = {}

    def wg(h, w, apply):
        one_tile = h <= (4 if w % 32 == 0 else 16) and w <= (32 if w % 32 == 0 else 8)   # launch_wgrad: such a map keeps algorithm 1's
        wino4 = algo == 11 and not one_tile
        wino = wino4 or (algo != 0 and h % 2 == 0 and w % 2 == 0)
        return "fused12" if apply and wino and not wino4 else "wino4" if wino4 else "wino" if wino else "direct"

    out[0] = (bnr, False, False, "l0", None)
    for l in range(1, 8):
        hl, wl = _res(l, H, W)
        cin, cout = t[l][2], t[l][3]
        apply = fuse_ok(hl, wl, cout)
        lazy = bnr and apply and l not in POOLED
        dg = "direct" if algo == 0 else _kernel(algo, l, 3, 2, B, hl, wl, cout, cin, n_cu)
        out[l] = (bnr, apply, lazy, wg(hl, wl, apply), dg)
    heads_dg = "direct" if algo == 0 else _f2x2(B, Hc, Wc, 2, n_cu)   # (allow_w4 = false: the concatenated heads image is F(2x2,3x3))
    for l in (L_PA, L_DA, L_DS)[:nheads]:
        apply = fuse_ok(Hc, Wc, 256)
        out[l] = (bnr, apply, bnr and apply, wg(Hc, Wc, apply), heads_dg)
    g1 = "grouped" if algo != 0 else "direct"
    for l in (L_PB, L_DB, L_SOUT)[:nheads]:
        out[l] = (False, False, False, g1, g1)
    return out


def _nchw(t):
    return t.permute(0, 3, 1, 2)


class _Back:
    def __init__(self, e, arch, sd, B, H, W, algo, imgs, routes, samples):
        self.e, self.arch, self.sd, self.B, self.H, self.W, self.algo, self.imgs = e, arch, sd, B, H, W, algo, imgs
        self.t = C.layer_table(arch)
        self.nheads = 3 if arch.endswith("ssmall") else 2
        self.routes = routes
        self.x = samples   # the two views' images, [B,1,H,W] on the host
        self.grad = {k: v.detach().cpu().double() for k, v in e.grad_dict().items()}
        self.worst = {}
        self.chunk = 4

    def note(self, fam, r, where):
        self.worst[fam] = max(self.worst.get(fam, (0.0, "")), (r, where))
        assert r <= TAU[fam], (fam, where, r, TAU[fam])

    @staticmethod
    def ratio(got, ref, base):
        """max |got - ref| / base; an element with base == 0 must match exactly (ratio inf otherwise); (ratio, flat index)"""
        d = (got.double() - ref).abs()
        r = torch.where(base > 0, d / base.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
        i = int(r.reshape(-1).argmax())
        return float(r.reshape(-1)[i]), i

    def stats(self, v, l, c):
        return [self.e.debug_buffer(v, "%s%d" % (n, l), (c,)).cpu().double() for n in ("scale", "shift", "mean", "invstd")]

    def gamma(self, l):
        return _sd_tensor(self.sd, self.t[l][1] + ".weight").double()

    # ---- APPLY ----
    def apply(self, v, l, y, dout, dy, relu, pool, fam, cb=None):
        """y [B,H,W,C] stored conv output (fp32), dout the gradient wrt the (pooled) activation, dy the dY tap (None: layer 0).
        Returns the per-channel S1, S2, sum |G|, sum |G xhat| of this view.  cb(b0, b1, ref, base) sees the fp64 dY per chunk."""
        C_ = y.shape[-1]
        sc, sh, mean, invstd = self.stats(v, l, C_)
        gam = self.gamma(l)
        n = y.shape[0] * y.shape[1] * y.shape[2]

        def g_of(b0, b1):
            yc = y[b0:b1].double()
            z = (yc * sc + sh).float()   # fma in fp32: exact product, one rounding
            d = dout[b0:b1].double()
            if pool:
                a = _nchw(F.relu(z))
                _, idx = F.max_pool2d(a, 2, return_indices=True)
                d = F.max_unpool2d(_nchw(d).contiguous(), idx, 2, output_size=a.shape[-2:]).permute(0, 2, 3, 1)
            g = d * (z > 0) if relu else d
            return g, (yc - mean) * invstd

        S1, S2, A1, A2 = (torch.zeros(C_, dtype=torch.float64) for _ in range(4))
        for b0 in range(0, y.shape[0], self.chunk):
            g, xh = g_of(b0, b0 + self.chunk)
            gx = g * xh
            S1 += g.sum((0, 1, 2)); S2 += gx.sum((0, 1, 2)); A1 += g.abs().sum((0, 1, 2)); A2 += gx.abs().sum((0, 1, 2))
        k = gam * invstd
        worst = (0.0, None)
        for b0 in range(0, y.shape[0], self.chunk):
            g, xh = g_of(b0, b0 + self.chunk)
            ref = k * (g - S1 / n - xh * (S2 / n))
            base = k.abs() * (g.abs() + A1 / n + xh.abs() * (A2 / n))
            if dy is not None:
                r, i = self.ratio(dy[b0:b0 + self.chunk], ref, base)
                if r > worst[0]:
                    worst = (r, np.unravel_index(i, ref.shape))
            if cb is not None:
                cb(b0, b0 + self.chunk, ref, base)
        if dy is not None:
            (b, yy, xx, c) = worst[1] if worst[1] is not None else (0, 0, 0, 0)
            self.note(fam, worst[0], "%s view %d APPLY dY[%d,%d,%d,c%d]" % (self.t[l][0], v, b, yy, xx, c))
        return S1, S2, A1, A2

    def bn_params(self, l, sums, dy_sum, dy_abs):
        """sums: per view (S1, S2, A1, A2); dy_sum / dy_abs: per-channel sum of dY / |dY| over both views"""
        conv, bn = self.t[l][0], self.t[l][1]
        S1 = sum(s[0] for s in sums); S2 = sum(s[1] for s in sums)
        A1 = sum(s[2] for s in sums); A2 = sum(s[3] for s in sums)
        C_ = S1.shape[0]
        for key, ref, base in ((bn + ".weight", S2, A2), (bn + ".bias", S1, A1), (conv + ".bias", dy_sum, dy_abs)):
            r, i = self.ratio(self.grad[key][:C_], ref, base)
            self.note("bn_sums", r, "%s[%d]" % (key, i))

    # ---- weight gradient ----
    @staticmethod
    def channels(cout):
        """the dW channel subset at B = 32: first and last of every 64-channel block, a few inside, the last (partial) quad"""
        s = set()
        for b in range(0, cout, 64):
            s.update({b, b + 1, b + 31, b + 62, b + 63})
        s.update(range((cout - 1) // 4 * 4, cout))
        return sorted(c for c in s if c < cout)

    def dw_add(self, acc, a, d, sub, pad):
        """acc = [ref, mag] += conv2d_weight of the chunk (a NCHW operand, d NCHW dY), output channels `sub`"""
        d = d[:, sub]
        shape = (len(sub), a.shape[1], 2 * pad + 1, 2 * pad + 1)
        acc[0] += torch.nn.grad.conv2d_weight(a, shape, d, padding=pad)
        acc[1] += torch.nn.grad.conv2d_weight(a.abs(), shape, d.abs(), padding=pad)

    @staticmethod
    def dw_family(wgk, h, w):
        """the tau family of a weight gradient: wgrad_wino_fused_kernel on a map inside one of its tiles has its own"""
        th, tw = (4, 32) if w % 32 == 0 else (16, 8)
        return "dw_%s_sub_tile" % wgk if wgk in ("fused12", "wino") and h <= th and w <= tw else "dw_" + wgk

    def dw_check(self, l, acc, sub, fam):
        key = self.t[l][0] + ".weight"
        r, i = self.ratio(self.grad[key][sub], acc[0], acc[1])
        co, ci, ky, kx = np.unravel_index(i, acc[0].shape)
        self.note(fam, r, "%s[%d,%d,%d,%d]" % (key, sub[co], ci, ky, kx))

    # ---- data gradient ----
    def dx_check(self, v, name, target, dy, w, pad, fam):
        """target [n,H,W,Cin] (the dOut tap below), dy [n,H,W,Cout], w [Cout,Cin,k,k]: target = conv2d_input(w, dy)"""
        dyd, wd = _nchw(dy).double(), w.double()
        ref = F.conv_transpose2d(dyd, wd, padding=pad)
        mag = F.conv_transpose2d(dyd.abs(), wd.abs(), padding=pad)
        r, i = self.ratio(_nchw(target), ref, mag)
        b, c, yy, xx = np.unravel_index(i, ref.shape)
        self.note(fam, r, "%s view %d dX[img %d,%d,%d,c%d]" % (name, v, self.imgs[b], yy, xx, c))

    def operand(self, v, l, y):
        """NCHW fp64 forward operand of layer l + 1: relu(fma(Y_l, scale, shift)) in fp32, 2x2 max-pooled after layers 1, 3, 5,
        from y = (images of) the stored Y_l and the engine's affine"""
        cout = self.t[l][3]
        sc, sh = [self.e.debug_buffer(v, "%s%d" % (n, l), (cout,)).cpu().double() for n in ("scale", "shift")]
        a = _nchw(F.relu((y.cpu().double() * sc + sh).float()))
        return (F.max_pool2d(a, 2) if l in POOLED else a).double()

    # ---- the encoder ----
    def encoder_layer(self, l):
        e, B, H, W, t = self.e, self.B, self.H, self.W, self.t
        conv, bn, cin, cout, k = t[l]
        hl, wl = _res(l, H, W)
        bsums, apply_f, lazy, wgk, dgk = _decode(e.backward_route(l))
        fam_apply = "fused12" if apply_f else "separate"
        pool = l in POOLED
        dh, dw_ = (hl // 2, wl // 2) if pool else (hl, wl)
        sub = self.channels(cout) if B >= 32 else list(range(cout))
        acc = [torch.zeros(len(sub), cin, k, k, dtype=torch.float64) for _ in range(2)]
        sums, dy_sum, dy_abs = [], torch.zeros(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64)
        for v in range(2):
            y = e.debug_buffer(v, "Y%d" % l, (B, hl, wl, cout)).cpu()
            dout = e.backward_tap(v, l, 0, (B, dh, dw_, cout))
            if l == 0:
                x = self.x[v]

                def cb(b0, b1, ref, base):
                    # bn_bwd_apply_l0_kernel forms dY_0 and its weight gradient in one pass: the magnitude of the weight-gradient
                    # bound takes the APPLY bound in place of |dY_0|
                    xc = x[b0:b1].double()
                    acc[0] += torch.nn.grad.conv2d_weight(xc, acc[0].shape, _nchw(ref)[:, sub], padding=1)
                    acc[1] += torch.nn.grad.conv2d_weight(xc.abs(), acc[1].shape, _nchw(base)[:, sub], padding=1)
                    dy_sum.add_(ref.sum((0, 1, 2))); dy_abs.add_(base.sum((0, 1, 2)))
                sums.append(self.apply(v, 0, y, dout, None, True, False, None, cb))
                continue
            dy = e.backward_tap(v, l, 1, (B, hl, wl, cout))
            sums.append(self.apply(v, l, y, dout, dy, True, pool, "apply_" + fam_apply))
            del y, dout
            dy_sum += dy.double().sum((0, 1, 2)); dy_abs += dy.double().abs().sum((0, 1, 2))
            ph, pw = _res(l - 1, H, W)
            yprev = e.debug_buffer(v, "Y%d" % (l - 1), (B, ph, pw, cin))   # (on the device; one chunk at a time to the host)
            for b0 in range(0, B, self.chunk):
                self.dw_add(acc, self.operand(v, l - 1, yprev[b0:b0 + self.chunk]), _nchw(dy[b0:b0 + self.chunk]).double(), sub, k // 2)
            del yprev
            # data gradient: dOut of the layer below
            ph, pw = _res(l, H, W)
            target = e.backward_tap(v, l - 1, 0, (B, ph, pw, cin))[self.imgs]
            self.dx_check(v, conv, target, dy[self.imgs], _sd_tensor(self.sd, conv + ".weight"), k // 2, "dx_" + dgk)
        self.dw_check(l, acc, sub, self.dw_family(wgk, hl, wl))
        self.bn_params(l, sums, dy_sum, dy_abs)

    # ---- the heads ----
    def heads(self):
        e, B, t = self.e, self.B, self.t
        Hc, Wc = self.H // 8, self.W // 8
        hcs = 256 * self.nheads
        h3 = (L_PA, L_DA, L_DS)[:self.nheads]
        p1 = (L_PB, L_DB, L_SOUT)[:self.nheads]
        sout_cs = (t[L_SOUT][3] + 3) // 4 * 4 if self.nheads == 3 else 0
        sub = self.channels(256) if B >= 32 else list(range(256))
        acc3 = {l: [torch.zeros(len(sub), 128, 3, 3, dtype=torch.float64) for _ in range(2)] for l in h3}
        acc1 = {l: [torch.zeros(t[l][3], 256, 1, 1, dtype=torch.float64) for _ in range(2)] for l in p1}
        sums = {l: [] for l in h3 + p1}
        dys = {l: [torch.zeros(t[l][3], dtype=torch.float64) for _ in range(2)] for l in h3 + p1}
        r3 = {l: _decode(e.backward_route(l)) for l in h3}
        r1 = {l: _decode(e.backward_route(l)) for l in p1}
        for v in range(2):
            yh = e.debug_buffer(v, "Y8", (B, Hc, Wc, hcs)).cpu()
            dout3 = e.backward_tap(v, L_PA, 0, (B, Hc, Wc, hcs))
            dy3 = e.backward_tap(v, L_PA, 1, (B, Hc, Wc, hcs))
            # pointwise heads: APPLY (no ReLU) from the roots, weight gradients, data gradients into dOut of the 3x3 heads
            roots = {L_PB: e.debug_buffer(v, "dsemi", (B, Hc, Wc, 80))[..., :65].cpu(),
                     L_DB: e.debug_buffer(v, "ddesc", (B, Hc, Wc, 256)).cpu()}
            dyp = {L_PB: e.backward_tap(v, L_PB, 1, (B, Hc, Wc, 80))[..., :65],
                   L_DB: e.backward_tap(v, L_DB, 1, (B, Hc, Wc, 256))}
            if self.nheads == 3:
                dyp[L_SOUT] = e.debug_buffer(v, "dsout", (B, Hc, Wc, sout_cs))[..., :t[L_SOUT][3]].cpu()
            for hk, l in enumerate(p1):
                conv, bn, cin, cout, _ = t[l]
                if bn is not None:
                    cs = 80 if l == L_PB else 256
                    y = e.debug_buffer(v, "Y%d" % l, (B, Hc, Wc, cs))[..., :cout].cpu()
                    sums[l].append(self.apply(v, l, y, roots[l], dyp[l], False, False, "apply_separate"))
                d = dyp[l].double()
                dys[l][0] += d.sum((0, 1, 2)); dys[l][1] += d.abs().sum((0, 1, 2))
                src = h3[hk]
                a = self.operand_heads(v, src, yh[..., 256 * hk:256 * hk + 256])
                self.dw_add(acc1[l], a, _nchw(d), list(range(cout)), 0)
                w = _sd_tensor(self.sd, conv + ".weight")
                self.dx_check(v, conv, dout3[self.imgs][..., 256 * hk:256 * hk + 256], dyp[l][self.imgs], w, 0, "dx_" + r1[l][4])
            # 3x3 heads: APPLY, weight gradients, ONE data gradient over the concatenated channels
            a7 = self.operand(v, 7, e.debug_buffer(v, "Y7", (B, Hc, Wc, 128)))
            for hk, l in enumerate(h3):
                sl = slice(256 * hk, 256 * hk + 256)
                fam = "apply_" + ("fused12" if r3[l][1] else "separate")
                sums[l].append(self.apply(v, l, yh[..., sl], dout3[..., sl], dy3[..., sl], True, False, fam))
                d = dy3[..., sl].double()
                dys[l][0] += d.sum((0, 1, 2)); dys[l][1] += d.abs().sum((0, 1, 2))
                for b0 in range(0, B, self.chunk):
                    self.dw_add(acc3[l], a7[b0:b0 + self.chunk], _nchw(d[b0:b0 + self.chunk]), sub, 1)
            wcat = torch.cat([_sd_tensor(self.sd, t[l][0] + ".weight") for l in h3], 0)
            target = e.backward_tap(v, 7, 0, (B, Hc, Wc, 128))[self.imgs]
            self.dx_check(v, "heads", target, dy3[self.imgs], wcat, 1, "dx_" + r3[h3[0]][4])
        for l in h3:
            self.dw_check(l, acc3[l], sub, self.dw_family(r3[l][3], Hc, Wc))
            self.bn_params(l, sums[l], *dys[l])
        for l in p1:
            self.dw_check(l, acc1[l], list(range(t[l][3])), "dw_" + r1[l][3])
            if t[l][1] is not None:
                self.bn_params(l, sums[l], *dys[l])
            else:   # Sout: bias gradient = column sums of dsout
                key = t[l][0] + ".bias"
                r, i = self.ratio(self.grad[key], dys[l][0], dys[l][1])
                self.note("bn_sums", r, "%s[%d]" % (key, i))

    def operand_heads(self, v, l, y):
        sc, sh = [self.e.debug_buffer(v, "%s%d" % (n, l), (256,)).cpu().double() for n in ("scale", "shift")]
        return _nchw(F.relu((y.double() * sc + sh).float())).double()


def _edit_gammas(arch, sd):
    """gamma == 0 on three channels of every encoder BatchNorm, with beta > 0, == 0 (z == 0 exactly: the ReLU gate at 0 and the
    pool_fix scan) and < 0 (on top of _inputs' negative gamma on every third channel)"""
    for l, (_, bn, _, _, _) in enumerate(C.layer_table(arch)[:8]):
        g, b = sd[bn + ".weight"].clone(), sd[bn + ".bias"].clone()
        for c, beta in ((1, 0.25), (4, 0.0), (7, -0.25)):
            g[c] = 0.0
            b[c] = beta
        sd[bn + ".weight"], sd[bn + ".bias"] = g, b


TAP_LAYERS = list(range(8)) + [L_PA, L_PB, L_DB]   # every tap: the encoder, the 3x3 heads (one tap pair), Pb and Db


def _transparency(arch, sd, B, H, W, algo, sample):
    """Under set_deterministic(True): one step with every tap on and one with the taps off give bit-identical scalars and
    gradients with equal launch counts per profiled kernel; a graph step with taps on raises."""
    from semantic_superpoint_amd import lib as L
    L.set_deterministic(True)
    try:
        runs = []
        for taps in (False, True):
            e = _engine(arch, B, H, W, sd)
            if algo != 1:
                e.set_conv_algo(algo)
            e.debug_backward_taps(TAP_LAYERS if taps else None)
            e.zero_grad()
            e.profile_enable("conv3x3_every")
            sc = e.pair_step(sample, indices=None, seed=7, train=True)
            torch.cuda.synchronize()
            kern = {k: v["launches"] for k, v in e.profile_read_kernels().items()}
            e.profile_enable("none")
            runs.append((sc.cpu().clone(), e.grads.cpu().clone(), kern))
            if taps:
                with torch.cuda.stream(torch.cuda.Stream()):
                    with pytest.raises(RuntimeError, match="backward taps"):
                        e.pair_step(sample, indices=None, seed=7, train=True, graph=True)
                torch.cuda.synchronize()
            del e
            torch.cuda.empty_cache()
    finally:
        L.set_deterministic(False)
    (s0, g0, k0), (s1, g1, k1) = runs
    same = torch.equal(s0, s1) and torch.equal(g0, g1) and k0 == k1
    print("tap transparency: scalars %s, gradients %s, launches %s (%d kernels), graph step refused" % (
        torch.equal(s0, s1), torch.equal(g0, g1), k0 == k1, len(k0)))
    assert same, (k0, k1)


CASES = [
    # tag, B, H, W, algorithm
    ("sp", 32, 240, 320, 1),    # the benchmark: wino4 / pipe / p2 data gradients with fused sums, fused12 APPLY, l0
    ("ssp", 32, 240, 320, 1),   # the headline configuration: + the segmentation head in the grouped launches
    ("ssp", 2, 240, 320, 1),    # small-batch data-gradient kernels
    ("ssp", 3, 40, 56, 1),      # ragged tiles, 5x7 maps: direct weight gradient and the separate APPLY there
    ("ssp", 2, 64, 96, 0),      # direct everywhere, nothing fused
    ("sp", 2, 64, 96, 10),      # F(4x4,3x3) on every encoder layer
    ("ssp", 2, 64, 96, 11),     # wgrad_wino4_kernel (no fused APPLY)
]


# the tile-edge sweep (tests/exact_sweep_cases.py; what each case adds: its table)
SWEEP_BACK_CASES = [(tag, B, H, W, algo) for tag, B, H, W in SWEEP_CASES
                    for algo in ((1, 10, 0, 11) if (tag, B, H, W) in SWEEP_CASES[:4] else (1,))]
ALL_CASES = CASES + SWEEP_BACK_CASES


@pytest.mark.parametrize("tag,B,H,W,algo", ALL_CASES, ids=["%s-B%d-%dx%d-algo%d" % c for c in ALL_CASES])
def test_fp32_backward_chain_teacher_forced(tag, B, H, W, algo):
    torch.set_num_threads(min(int(os.environ.get("OMP_NUM_THREADS", "16")), 16))
    t0 = time.perf_counter()
    arch, sd, sample = _inputs(tag, B, H, W, flip_gamma=B < 32)
    if B < 32:
        _edit_gammas(arch, sd)
    e = _engine(arch, B, H, W, sd)
    if algo != 1:
        e.set_conv_algo(algo)
    e.debug_backward_taps(TAP_LAYERS)
    e.zero_grad()
    e.pair_step(sample, indices=None, seed=7, train=True)
    torch.cuda.synchronize()
    _check_backward(e, arch, sd, tag, B, H, W, algo, sample, t0)
    del e
    torch.cuda.empty_cache()
    _transparency(arch, sd, B, H, W, algo, sample)


def _check_backward(e, arch, sd, tag, B, H, W, algo, sample, t0):
    """Every stage of the backward of the engine's last pair step (B pairs of HxW, taps on) against fp64, and its route record
    against the mirror of the dispatch."""
    want = _predict_routes(arch, algo, B, H, W)
    got = {l: _decode(e.backward_route(l)) for l in want}
    print("%s B=%d %dx%d algo %d routes: %s" % (tag, B, H, W, algo, {l: got[l] for l in sorted(got)}))
    for l in sorted(want):
        assert got[l] == want[l], ("route of layer", l, "got", got[l], "predicted", want[l])
    imgs = [0, 1, B // 2, B - 2, B - 1] if B >= 32 else list(range(B))
    xs = [sample[k].cpu() for k in ("image", "warped_img")]
    bk = _Back(e, arch, sd, B, H, W, algo, imgs, want, xs)
    bk.heads()
    for l in range(7, -1, -1):
        bk.encoder_layer(l)
    print("%s B=%d %dx%d algo %d: worst |got - fp64| / bound per family: %s (%.1f s)" % (
        tag, B, H, W, algo, ", ".join("%s %.3e [%s]" % (f, r, where) for f, (r, where) in sorted(bk.worst.items())),
        time.perf_counter() - t0))
    return bk.worst
