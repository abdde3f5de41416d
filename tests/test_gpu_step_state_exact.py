"""GPU: the kernels that turn a step into persistent state, each against a closed-form fp64 reference (tests/step_state_ref.py)
on state the test writes or reads back itself: adam_kernel / adam_scaled_kernel, the BatchNorm finalize (bn_finalize_kernel,
bn_finalize_multi_kernel and the consumer-side finalize in the prologue of the Winograd kernels, every BatchNorm layer) and
desc_normalize_kernel.  No whole-step comparison with the oracle happens here (tests/test_gpu_model.py and
tests/test_gpu_single_view.py do that, at tolerances of about 2 lr per parameter, which no Adam can miss).

u = 2^-24 is the unit roundoff of fp32: one rounding to nearest changes a value by at most u relative.

Adam.  The kernel evaluates, per element, in fp32 (gs = g, or fl(g * gscale) in adam_scaled_kernel):
    m1 = 0.9f m + 0.1f gs;   v1 = 0.999f v + 0.001f gs gs;   p1 = p - step_size * (m1 / (sqrtf(v1) / bc2_sqrt + 1e-8f))
with step_size = fl(lr / (1 - 0.9^t)) and bc2_sqrt = fl(sqrt(1 - 0.999^t)) evaluated in double on the host.  Counting roundings
(a constant, a product, a sum, a division or a correctly rounded sqrtf: one u each; a sum of terms of one sign keeps the largest
relative error of its terms, a sum of any signs keeps their absolute errors):
    |m1 - m_ref| <= K_M u A,  A = 0.9 |m| + 0.1 |gs|:  constant + product per term (2 u), the sum (1 u): K_M = 3; the scaled
                   kernel rounds g * gscale first (3 u on that term): K_M = 4
    |v1 - v_ref| <= K_V u v_ref: term 0.001f gs gs = constant + two products (3 u), the sum (1 u): K_V = 4; the scaled kernel
                   squares a rounded gs (5 u on that term, 6 u with the sum when the other term is zero or small), of which the
                   known error of the constant 0.001f (0.8 u) and the exact sum with a zero v leave 4.8 u at t = 1 from zero
                   moments; K_V = 5 is the most this test allows itself there
    |p1 - p_ref| <= u |p_ref| + (lr / bc1) (K_M u A + 8 u |m_ref|) / denom_ref: the final subtraction (u |p|), the error of m1,
                   and 8 u for everything that multiplies it: step_size (1), v1 under the square root (K_V / 2), sqrtf (1), bc2_sqrt
                   (1), the two divisions (2), + eps (1), the product (1).  That count is 9 to 9.5 u if every rounding had its
                   largest size and the same sign; 8 u is the cap this test holds itself to.
The fp32 bias corrections this library used before (1.f - powf(0.999f, t): the cancellation in 1 - 0.999f loses 1.3e-5) put the
whole update off by -112 u at t = 1 and 10, -169 u at t = 2 and -63 u at t = 1000: the p1 assertion fails there by those amounts
on a library built from the earlier sources, and holds with the host-side double evaluation.
Measured on the MI355X over all cases of this file, as the largest error / bound: m 0.80 (plain) and 0.69 (scaled), v 0.55 and
0.44; p 1.00, reached where the update is smaller than an ulp of p and the final rounding alone fills u |p_ref|; the update itself
(parameters that start at zero, no cancellation in m1) is within -7.2 u .. +5.8 u of the reference at every t (the earlier fp32 bias corrections: -117 u at t = 1, -175 u at t = 2,
-119 u at t = 10, -68 u at t = 1000, i.e. 10.5, 15.7, 10.6 and 6.1 times the bound on p1).

BatchNorm finalize.  The convolution epilogues add y and y^2 in fp32 inside a workgroup and commit one fp64 atomic per channel
and workgroup, so the statistics are not exact sums; how far off they are depends on how many values a workgroup visits.  That is
the ONE measured number of this file: with s1, s2 the sums the device used (recovered from its stored mean and invstd) and the
fp64 sums of the device's own fp32 conv output as the reference,
    c1 = |s1_dev - s1_ref| / (u sum |y|),   c2 = |s2_dev - s2_ref| / (u sum y^2).
Measured maxima on the MI355X over every BatchNorm layer and both slots (C_STATS_MEASURED): c1 2.14 / c2 2.98 for both
architectures at B = 2, 64x96, c1 2.63 / c2 3.17 at B = 3, 40x56 (bnDb, 105 values per channel).  The figures barely move with the
count (c2 1.3 .. 1.7 on the 12288-value layers, 1.7 .. 3.2 on the 105-value ones): most of them is the fp32 storage of the mean
and invstd the sums are recovered from (up to 1 in c1; up to 2 (var + eps) / E[y^2] + 2 mean^2 / E[y^2], i.e. 2 .. 4, in c2), not
the fp32 partial sums.  The rule - 4 x the largest, rounded up to a power of two - asks for 16; the cap is sqrt(count) of the
smallest layer, sqrt(105) = 10.2 (the random-walk error of adding everything sequentially in fp32), and it is not raised:
C_STATS = 8, the largest power of two under the cap, 2.5 x the largest measured value.  Everything else follows from C_STATS by
first-order propagation (the derivations are in _bn_bounds).

Descriptor normalisation: |desc - desc_ref| <= (log2(256) + 6) u per element (relative to the unit norm): the fma (1), the square
and the three in-lane additions (log2(4) = 2 of the log2(256) = 8 levels of the sum, the 6-level shuffle tree is the rest), the
sqrtf (1/2 after the root, 1 of its own), the reciprocal (1) and the product (1)."""
import functools
import time

import numpy as np
import pytest
import torch

from tests import step_state_ref as R
from tests.gate_util import _dev

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ARCHS = {"sp": "SuperPointNet_gauss2", "ssp": "SuperPointNet_gauss2_ssmall"}


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)

# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
ADAM_K_M = {False: 3.0, True: 4.0}   # [scaled kernel?]
ADAM_K_V = {False: 4.0, True: 5.0}
ADAM_K_P = 8.0
ADAM_T = (1, 2, 10, 1000, 100000)
ADAM_LR = (1e-3, 1e-4)
ADAM_GS = (None, 1.0, 0.125, 1.0 / 3.0)


@pytest.fixture(scope="module")
def adam_engine():
    from semantic_superpoint_amd.lib import Engine
    return Engine(ARCHS["ssp"], 2, 64, 96, _dev())


@functools.lru_cache(maxsize=None)
def _adam_state(n, zero_moments=False):
    """fp32 p, g, m, v of n elements.  Blocks of 1024 elements cycle through the parameter groups (exact zeros: p1 = -update, so the
    update is visible without ulp(p) in the way; |p| <= 1e-4; weight scale 0.05) and, at another period, through the kinds of
    gradient / moment content: log-uniform magnitudes 1e-12 .. 1e4 of both signs (twice), g == 0 with live moments, m and g of
    opposite signs that cancel to 1e-6 of their magnitude in m1, and all of g, m, v exactly zero.  v >= 0 is tied to the larger of
    m^2 and g^2 (as it is in a run), so the updates stay within a few lr.  The last 1027 elements (the last whole 256-thread block,
    the partial one and eta) are of the generic kind on weight-scale parameters."""
    rs = np.random.RandomState(1234)
    i = np.arange(n)
    sign = lambda: rs.choice([-1.0, 1.0], n)   # noqa: E731
    g = sign() * 10.0 ** rs.uniform(-12, 4, n)
    m = sign() * 10.0 ** rs.uniform(-12, 4, n)
    kind = (i // 3072) % 5
    kind[n - 1027:] = 0
    g[kind == 1] = 0.0
    c = kind == 2
    m[c] = -g[c] / 9.0 * (1.0 + 1e-6 * rs.standard_normal(int(c.sum())))
    v = np.maximum(m * m, g * g) * 10.0 ** rs.uniform(-1, 3, n)
    z = kind == 4
    g[z] = m[z] = v[z] = 0.0
    p = rs.standard_normal(n) * 0.05
    grp = (i // 1024) % 3
    grp[n - 1027:] = 2
    p[grp == 0] = 0.0
    p[grp == 1] = rs.uniform(-1e-4, 1e-4, int((grp == 1).sum()))
    if zero_moments:   # the first step of training
        m[:] = 0.0
        v[:] = 0.0
    out = tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (p, g, m, v))
    assert np.all(out[3] >= 0) and np.all(np.isfinite(out[1])) and (out[0] == 0).sum() > n // 4
    return out


def _adam_load(e, state, t):
    for dst, src in zip((e.params, e.grads, e.adam_m, e.adam_v), state):
        dst.copy_(torch.from_numpy(src))   # in place: the pointers the library is bound to stay valid
    e.adam_t = t - 1


def _adam_read(e):
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy().copy() for a in (e.params, e.grads, e.adam_m, e.adam_v))


def _adam_check(before, after, lr, t, gs, tag):
    """`after` = the device state one step after `before` (both fp32 tuples p, g, m, v) against the fp64 reference of that step."""
    scaled = gs is not None
    # lr and grad_scale cross the C ABI as floats: the reference takes their fp32 images, like those of every other input
    p_ref, m_ref, v_ref, A, denom = R.adam_ref(*before, float(np.float32(lr)), t, 1.0 if gs is None else float(np.float32(gs)))
    bc1 = R.adam_bias_corrections(t)[0]
    p1, g1, m1, v1 = (a.astype(np.float64) for a in after)
    em, ev, ep = np.abs(m1 - m_ref), np.abs(v1 - v_ref), np.abs(p1 - p_ref)
    bm = ADAM_K_M[scaled] * U * A
    bv = ADAM_K_V[scaled] * U * v_ref
    bp = U * np.abs(p_ref) + (lr / bc1) * (ADAM_K_M[scaled] * U * A + ADAM_K_P * U * np.abs(m_ref)) / denom
    upd = np.abs(p_ref - before[0].astype(np.float64))
    zero_p = (before[0] == 0) & (upd > 0) & (A <= 1.01 * np.abs(m_ref))   # p1 = -update, and m1 is no cancelled difference
    rel = float(((p1 - p_ref) / np.where(zero_p, p_ref, 1.0))[zero_p].min() / U) if zero_p.any() else 0.0
    rel_hi = float(((p1 - p_ref) / np.where(zero_p, p_ref, 1.0))[zero_p].max() / U) if zero_p.any() else 0.0
    ratio = lambda err, bound: float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))  # noqa: E731
    print("%s t=%d lr=%g gs=%s: worst error / bound: m %.3f, v %.3f, p %.3f; update error where p == 0: %+.1f u .. %+.1f u"
          % (tag, t, lr, gs, ratio(em, bm), ratio(ev, bv), ratio(ep, bp), rel, rel_hi))
    assert np.array_equal(after[1], before[1]), (tag, "the kernel wrote to the gradient")
    assert np.all(em <= bm), (tag, "m", t, lr, gs, ratio(em, bm))      # constant + product per term, the sum (+ g * gscale)
    assert np.all(ev <= bv), (tag, "v", t, lr, gs, ratio(ev, bv))      # constant + two products, the sum (+ g * gscale twice)
    # subtraction; error of m1; step_size, sqrtf and its argument, bc2_sqrt, two divisions, + eps, product
    assert np.all(ep <= bp), (tag, "p", t, lr, gs, ratio(ep, bp), "update off by %+.1f u .. %+.1f u" % (rel, rel_hi))
    n = before[0].size
    tail = slice(n // 256 * 256 - 256, n)   # the last whole block, the partial one, eta (the last three elements)
    moved = upd > 2 * _ulp32(before[0])   # (an update below an ulp of p may leave p where it was)
    assert n % 256 != 0 and 2 * moved[tail].sum() > moved[tail].size and np.all((after[0] != before[0])[tail][moved[tail]]), (tag, "tail not updated")
    assert np.all(after[2][tail] != before[2][tail]), (tag, "moments of the tail not updated")
    return p_ref, m_ref, v_ref


@pytest.mark.parametrize("gs", ADAM_GS, ids=lambda s: "gs-%s" % (s if s is None else "%.3g" % s))
@pytest.mark.parametrize("lr", ADAM_LR)
@pytest.mark.parametrize("t", ADAM_T)
def test_adam_step_vs_fp64(adam_engine, t, lr, gs):
    e = adam_engine
    before = _adam_state(e.params.numel())
    _adam_load(e, before, t)
    e.adam_step(lr, gs)
    assert e.adam_t == t
    _adam_check(before, _adam_read(e), lr, t, gs, "state")


@pytest.mark.parametrize("gs", ADAM_GS, ids=lambda s: "gs-%s" % (s if s is None else "%.3g" % s))
@pytest.mark.parametrize("lr", ADAM_LR)
def test_adam_first_step_from_zero_moments(adam_engine, lr, gs):
    e = adam_engine
    before = _adam_state(e.params.numel(), zero_moments=True)
    _adam_load(e, before, 1)
    e.adam_step(lr, gs)
    after = _adam_read(e)
    _adam_check(before, after, lr, 1, gs, "zero moments")
    live = np.abs(before[1].astype(np.float64) * (1.0 if gs is None else gs)) > 1e-4   # update = lr g / (|g| + eps): lr sign(g) to 1e-4
    step = (after[0].astype(np.float64) - before[0])[live]
    assert np.allclose(step, -lr * np.sign(before[1][live]), rtol=1e-3, atol=0)


@pytest.mark.parametrize("t", (1, 1000))
def test_adam_unit_grad_scale_gives_the_bits_of_the_plain_step(adam_engine, t):
    e = adam_engine
    before = _adam_state(e.params.numel())
    outs = []
    for gs in (None, 1.0):
        _adam_load(e, before, t)
        e.adam_step(1e-3, gs)
        outs.append(_adam_read(e))
    for a, b, name in zip(outs[0], outs[1], ("p", "g", "m", "v")):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("gs", (None, 1.0 / 3.0), ids=("plain", "scaled"))
@pytest.mark.parametrize("t", (1, 10))
def test_adam_two_consecutive_steps_teacher_forced(adam_engine, t, gs):
    """The second call uses t + 1.  Its reference starts from the device's fp32 state after the first, so the bounds of one
    step hold for it unchanged."""
    e = adam_engine
    before = _adam_state(e.params.numel())
    _adam_load(e, before, t)
    e.adam_step(1e-3, gs)
    mid = _adam_read(e)
    _adam_check(before, mid, 1e-3, t, gs, "first of two")
    e.adam_step(1e-3, gs)
    assert e.adam_t == t + 1
    _adam_check(mid, _adam_read(e), 1e-3, t + 1, gs, "second of two")


# ------------------------------------------------------------------------------------------------
# BatchNorm finalize of every BatchNorm layer, descriptor normalisation
# ------------------------------------------------------------------------------------------------
# measured on the MI355X (max over the BatchNorm layers, both slots): tag, B, H, W -> c1, c2
C_STATS_MEASURED = {("ssp", 2, 64, 96): (2.140, 2.977), ("sp", 2, 64, 96): (2.140, 2.977), ("ssp", 3, 40, 56): (2.629, 3.165)}
C_STATS = 8.0   # the largest power of two below sqrt(105); 4 x max(C_STATS_MEASURED) would round up to 16 (module docstring)
BN_CASES = [("ssp", 2, 64, 96), ("sp", 2, 64, 96), ("ssp", 3, 40, 56)]   # 40x56: 5x7 cells, 105 values per head channel
BN_IDS = ["%s-B%d-%dx%d" % c for c in BN_CASES]


def _state_dict(tag, seed):
    """Default-initialised weights with live BatchNorm parameters and running statistics that are not the defaults (the 0.9 * term
    and the counter's starting value then matter)."""
    from semantic_superpoint_amd import synth
    from semantic_superpoint_amd.lib import layer_table
    sd = synth.default_init_state_dict(layer_table(ARCHS[tag]), seed=seed)
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    for i, (_, bn, _, cout, _) in enumerate(layer_table(ARCHS[tag])):
        if bn is None:
            continue
        gamma = torch.rand(cout, generator=g) + 0.5
        gamma[::5] = -gamma[::5]
        sd[bn + ".weight"] = gamma
        sd[bn + ".bias"] = torch.rand(cout, generator=g) - 0.5
        sd[bn + ".running_mean"] = torch.rand(cout, generator=g) * 2 - 1
        sd[bn + ".running_var"] = torch.rand(cout, generator=g) * 1.5 + 0.5
        sd[bn + ".num_batches_tracked"] = torch.tensor(1000 * i + 17, dtype=torch.int64)
    return sd


def _bn_layers(tag):
    from semantic_superpoint_amd.lib import layer_table
    return [(l, bn, cout) for l, (_, bn, _, cout, _) in enumerate(layer_table(ARCHS[tag])) if bn is not None]


def _raw_output(e, tag, v, l, B, H, W):
    """Y<l> of slot v as [B, h, w, cout] fp32: the pixel stride is the layer's own channel count in the encoder, the concatenated
    [Pa | Da | DS] tensor for the 3x3 heads (layers 8, 10, 12 share "Y8"), 80 for the 65 detector logits, 256 for the descriptors."""
    from semantic_superpoint_amd.lib import layer_table
    cout = layer_table(ARCHS[tag])[l][3]
    if l < 8:
        s = 0 if l < 2 else 1 if l < 4 else 2 if l < 6 else 3
        return e.debug_buffer(v, "Y%d" % l, (B, H >> s, W >> s, cout)).cpu().numpy()
    Hc, Wc = H // 8, W // 8
    if l in (8, 10, 12):
        nheads = 3 if tag == "ssp" else 2
        k = (l - 8) // 2
        return e.debug_buffer(v, "Y%d" % l, (B, Hc, Wc, 256 * nheads)).cpu().numpy()[..., 256 * k:256 * (k + 1)]
    cs = {65: 80, 256: 256}[cout]
    return e.debug_buffer(v, "Y%d" % l, (B, Hc, Wc, cs)).cpu().numpy()[..., :cout]


def _running(e):
    torch.cuda.synchronize()
    sd = e.state_dict()
    return {k: v.cpu().numpy().copy() for k, v in sd.items() if "running_" in k or "num_batches" in k}


def _affine(e, v, l, cout):
    return {k: e.debug_buffer(v, "%s%d" % (k, l), (cout,)).cpu().numpy() for k in ("mean", "invstd", "scale", "shift")}


@functools.lru_cache(maxsize=None)
def _bn_capture(tag, B, H, W):
    """forward(x, slot 0, train), forward(xw, slot 1, train), forward(x, slot 0, eval) on the fp32 path, conv algorithm 1, and
    everything the tests below read, as numpy arrays."""
    from semantic_superpoint_amd import synth
    from semantic_superpoint_amd.lib import Engine
    t0 = time.perf_counter()
    sd = _state_dict(tag, seed=11)
    sample = synth.make_pair(B, H, W, _dev(), seed=23, semantic=(tag == "ssp"))
    e = Engine(ARCHS[tag], B, H, W, _dev(), with_grad=False)
    e.set_conv_algo(1)
    e.load_state_dict(sd)
    cap = {"sd": {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in sd.items()}, "run": [_running(e)], "slot": []}
    x = (sample["image"], sample["warped_img"])
    for v in range(2):
        e.forward(x[v], slot=v, train=True)
        cap["run"].append(_running(e))
    Hc, Wc = H // 8, W // 8
    for v in range(2):   # read after BOTH forwards: the second one must not have touched what the first one left in slot 0
        s = {"Y": {}, "aff": {}}
        for l, bn, cout in _bn_layers(tag):
            s["Y"][l] = _raw_output(e, tag, v, l, B, H, W)
            s["aff"][l] = _affine(e, v, l, cout)
        s["desc"] = e.debug_buffer(v, "desc", (B, Hc, Wc, 256)).cpu().numpy()
        cap["slot"].append(s)
    e.forward(x[0], slot=0, train=False)
    cap["run_eval"] = _running(e)
    cap["aff_eval"] = {l: _affine(e, 0, l, cout) for l, bn, cout in _bn_layers(tag)}
    print("%s B=%d %dx%d: three forwards and the read-back took %.2f s" % (tag, B, H, W, time.perf_counter() - t0))
    return cap


def _stat_ratios(y, aff):
    """c1, c2 per channel: the sums the device used (recovered from its stored mean and invstd) against the fp64 sums of y."""
    y2 = y.reshape(-1, y.shape[-1]).astype(np.float64)
    n = y2.shape[0]
    mean, invstd = aff["mean"].astype(np.float64), aff["invstd"].astype(np.float64)
    s1_dev, s2_dev = mean * n, (1.0 / (invstd * invstd) - R.BN_EPS + mean * mean) * n
    a1, a2 = np.abs(y2).sum(axis=0), (y2 * y2).sum(axis=0)
    return np.abs(s1_dev - y2.sum(axis=0)) / (U * a1), np.abs(s2_dev - a2) / (U * a2)


@pytest.mark.parametrize("tag,B,H,W", BN_CASES, ids=BN_IDS)
def test_bn_statistics_sums_within_c_stats(tag, B, H, W):
    cap = _bn_capture(tag, B, H, W)
    worst = [0.0, 0.0]
    counts = []
    for v in range(2):
        for l, bn, cout in _bn_layers(tag):
            y = cap["slot"][v]["Y"][l]
            c1, c2 = _stat_ratios(y, cap["slot"][v]["aff"][l])
            counts.append(y.size // cout)
            print("%s slot %d layer %2d (%s, count %d): c1 %.3f  c2 %.3f" % (tag, v, l, bn, counts[-1], c1.max(), c2.max()))
            worst = [max(worst[0], float(c1.max())), max(worst[1], float(c2.max()))]
    print("%s B=%d %dx%d: max c1 %.3f, max c2 %.3f (C_STATS %.0f, sqrt(smallest count) %.1f)" % (tag, B, H, W, worst[0], worst[1], C_STATS,
                                                                                                  min(counts) ** 0.5))
    assert C_STATS <= min(counts) ** 0.5
    assert max(worst) <= C_STATS, worst


def _bn_bounds(r, gamma, c=C_STATS):
    """First-order propagation of |s1_dev - s1| <= c u sum |y| and |s2_dev - s2| <= c u sum y^2 (r = bn_finalize_ref's dict):
      mean = s1 / n                        -> d_mean  = c u E|y|
      var = s2 / n - mean^2                -> d_var   = c u E[y^2] + 2 |mean| d_mean (+ d_mean^2)
      invstd = fl((var + eps)^-1/2)        -> d_inv   = invstd^3 d_var / 2 + ulp(invstd)
      scale = fl(gamma invstd)             -> d_scale = |gamma| d_inv + ulp(scale)
      shift = fl(beta - fl(mean scale))    -> d_shift = |scale| d_mean + |mean| d_scale + one ulp at the larger of |shift| and
                                              |mean scale| (half an ulp of the product, half of the difference; an ulp of the
                                              difference alone would not cover a beta that cancels the product)
      running' = fl(0.9 running + 0.1 x)   -> 0.1 d_x + half an ulp (x = mean; x = var n / (n - 1) for the variance)"""
    n = r["count"]
    d_mean = c * U * r["abs_mean"]
    d_var = c * U * r["sq_mean"] + 2 * np.abs(r["mean"]) * d_mean + d_mean ** 2
    d_inv = 0.5 * r["invstd"] ** 3 * d_var + _ulp32(r["invstd"])
    d_scale = np.abs(gamma) * d_inv + _ulp32(r["scale"])
    d_shift = np.abs(r["scale"]) * d_mean + np.abs(r["mean"]) * d_scale + _ulp32(np.maximum(np.abs(r["shift"]), np.abs(r["mean"] * r["scale"])))
    return {"mean": d_mean, "invstd": d_inv, "scale": d_scale, "shift": d_shift,
            "rm1": 0.1 * d_mean + 0.5 * _ulp32(r["rm1"]), "rv1": 0.1 * d_var * n / (n - 1) + 0.5 * _ulp32(r["rv1"])}


@pytest.mark.parametrize("tag,B,H,W", BN_CASES, ids=BN_IDS)
def test_bn_finalize_every_layer_vs_fp64(tag, B, H, W):
    """Slot 0 then slot 1, the reference's order; the update of slot 1 starts from the fp32 running statistics slot 0 left."""
    cap = _bn_capture(tag, B, H, W)
    worst = {}
    for l, bn, cout in _bn_layers(tag):
        gamma, beta = cap["sd"][bn + ".weight"], cap["sd"][bn + ".bias"]
        for v in range(2):
            run0, run1 = cap["run"][v], cap["run"][v + 1]
            r = R.bn_finalize_ref(cap["slot"][v]["Y"][l], gamma, beta, run0[bn + ".running_mean"], run0[bn + ".running_var"],
                                  run0[bn + ".num_batches_tracked"])
            d = _bn_bounds(r, gamma.astype(np.float64))
            got = dict(cap["slot"][v]["aff"][l], rm1=run1[bn + ".running_mean"], rv1=run1[bn + ".running_var"])
            for k in ("mean", "invstd", "scale", "shift", "rm1", "rv1"):
                err = np.abs(got[k].astype(np.float64) - r[k])
                worst[k] = max(worst.get(k, 0.0), float((err / d[k]).max()))
                assert np.all(err <= d[k]), (tag, bn, "slot", v, k, float((err / d[k]).max()))
            assert int(run1[bn + ".num_batches_tracked"]) == r["nbt1"], (tag, bn, v)
        assert int(cap["run"][2][bn + ".num_batches_tracked"]) == int(cap["sd"][bn + ".num_batches_tracked"]) + 2
    print("%s B=%d %dx%d: worst error / bound: %s" % (tag, B, H, W, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("tag,B,H,W", BN_CASES, ids=BN_IDS)
def test_bn_eval_forward_reads_the_running_statistics_and_leaves_them(tag, B, H, W):
    """Eval mode: no sums are involved.  invstd = fl((rv + eps)^-1/2) from a double evaluation (half an ulp), scale = fl(gamma invstd)
    (half an ulp of its own, half inherited): within 2 ulp.  shift = fl(beta - fl(rm scale)): |rm| times the error of scale (one ulp of
    the product), half an ulp of the product, half of the difference: within 2 ulp at the larger of |shift| and |rm scale|."""
    cap = _bn_capture(tag, B, H, W)
    for k, a in cap["run"][2].items():
        assert np.array_equal(a, cap["run_eval"][k]), (tag, k, "changed by an eval forward")
    for l, bn, cout in _bn_layers(tag):
        rm, rv = cap["run"][2][bn + ".running_mean"], cap["run"][2][bn + ".running_var"]
        gamma, beta = cap["sd"][bn + ".weight"], cap["sd"][bn + ".bias"]
        r = R.bn_finalize_ref(np.zeros((2, 1, 1, cout)), gamma, beta, rm, rv)
        got = cap["aff_eval"][l]
        assert np.all(np.abs(got["scale"] - r["eval_scale"]) <= 2 * _ulp32(r["eval_scale"])), (tag, bn, "scale")
        at = np.maximum(np.abs(r["eval_shift"]), np.abs(rm.astype(np.float64) * r["eval_scale"]))
        assert np.all(np.abs(got["shift"] - r["eval_shift"]) <= 2 * _ulp32(at)), (tag, bn, "shift")
        assert np.array_equal(got["mean"], rm) and np.all(np.abs(got["invstd"] - r["eval_invstd"]) <= _ulp32(r["eval_invstd"])), (tag, bn)


@pytest.mark.parametrize("tag,B,H,W", BN_CASES, ids=BN_IDS)
def test_desc_normalize_vs_fp64(tag, B, H, W):
    """desc of each slot after the training forward against the fp64 normalisation of the device's own Y, scale and shift of the
    descriptor head.  B = 3 at 40x56: 105 cells, the last 256-thread block holds one wave of four."""
    cap = _bn_capture(tag, B, H, W)
    l = 11   # convDb / bnDb
    for v in range(2):
        s = cap["slot"][v]
        want, norm = R.desc_normalize_ref(s["Y"][l], s["aff"][l]["scale"], s["aff"][l]["shift"])
        assert np.all(norm > 0)
        got = s["desc"].astype(np.float64)
        err = np.abs(got - want).max()
        nerr = np.abs(np.sqrt((got * got).sum(axis=-1)) - 1.0).max()
        print("%s slot %d: max |desc - ref| %.2f u (bound %d u), max | ||desc|| - 1 | %.2f u (bound 4 u)" % (tag, v, err / U, np.log2(256) + 6, nerr / U))
        assert err <= (np.log2(256) + 6) * U, (tag, v, err / U)
        assert nerr <= 4 * U, (tag, v, nerr / U)


@pytest.mark.parametrize("tag,B,H,W", [BN_CASES[0], BN_CASES[2]], ids=[BN_IDS[0], BN_IDS[2]])
def test_pair_step_leaves_the_running_statistics_of_two_forward_calls(tag, B, H, W):
    """A training pair step (both views in every launch, bn_finalize_kernel / bn_finalize_multi_kernel / the consumer-side finalize
    looping view 0 then view 1) against forward(image, slot 0), forward(warped image, slot 1) on a second engine with the same
    state: running_mean, running_var and num_batches_tracked bit for bit.  Deterministic accumulation, so the fp64 sums do not
    depend on the commit order of the atomics.  At these sizes both engines run the same convolution kernels with the same
    values per workgroup (conv_wino_p2_kernel, at most one tile per workgroup in either launch shape; one workgroup per problem in
    the grouped pointwise kernel; one image row per workgroup in the first layer), so ssp_pair_step_phase is not needed."""
    from semantic_superpoint_amd import lib as L, synth
    sd = _state_dict(tag, seed=31)
    sample = synth.make_pair(B, H, W, _dev(), seed=37, semantic=(tag == "ssp"))
    L.set_deterministic(True)
    try:
        a = L.Engine(ARCHS[tag], B, H, W, _dev())
        b = L.Engine(ARCHS[tag], B, H, W, _dev(), with_grad=False)
        for e in (a, b):
            e.set_conv_algo(1)
            e.load_state_dict(sd)
        a.zero_grad()
        a.pair_step(sample, indices=None, seed=5, train=True)
        b.forward(sample["image"], slot=0, train=True)
        b.forward(sample["warped_img"], slot=1, train=True)
        ra, rb = _running(a), _running(b)
        del a, b
    finally:
        L.set_deterministic(False)
    for k in ra:
        if not np.array_equal(ra[k], rb[k]):
            d = np.abs(ra[k].astype(np.float64) - rb[k].astype(np.float64))
            raise AssertionError("%s: %s differs between the pair step and the two forward calls: %d elements, max |diff| %.3e"
                                 % (tag, k, int((d > 0).sum()), float(d.max())))
        if "num_batches" in k:
            assert int(ra[k]) == int(sd[k]) + 2, k
    assert any(not np.array_equal(ra[k], np.asarray(sd[k])) for k in ra if "running_mean" in k)
