"""Numpy fp64 restatements of the three operations that turn a training step into persistent state: the Adam update
(adam_kernel / adam_scaled_kernel), the BatchNorm statistics -> affine + running-statistics update (bn_finalize_kernel,
bn_finalize_multi_kernel and the consumer-side finalize of the Winograd kernels) and the descriptor head's L2 normalisation
(desc_normalize_kernel).  Written from the definitions (torch.optim.Adam / nn.BatchNorm2d defaults, models/SuperPointNet_gauss2.py:
64-65); tests/test_step_state_cpu.py pins them to torch in float64, tests/test_gpu_step_state_exact.py compares the kernels with them."""
import numpy as np

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def adam_bias_corrections(t):
    """(1 - beta1^t, 1 - beta2^t) in double, as torch.optim.Adam evaluates them."""
    return 1.0 - BETA1 ** int(t), 1.0 - BETA2 ** int(t)


def adam_ref(p, g, m, v, lr, t, grad_scale=1.0):
    """Step t (1-based) of torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False) on the gradient
    g * grad_scale, in fp64 on the fp64 images of the inputs.  Returns (p1, m1, v1, A, denom): the new parameter and moments, and
    the two magnitudes the error bounds of the fp32 kernel are written in: A = 0.9 |m| + 0.1 |g * grad_scale| (what the first
    moment is the signed sum of) and denom = sqrt(v1) / sqrt(1 - beta2^t) + eps."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    gs = g * float(grad_scale)
    bc1, bc2 = adam_bias_corrections(t)
    m1 = BETA1 * m + (1.0 - BETA1) * gs
    v1 = BETA2 * v + (1.0 - BETA2) * gs * gs
    denom = np.sqrt(v1) / np.sqrt(bc2) + ADAM_EPS
    p1 = p - (float(lr) / bc1) * (m1 / denom)
    A = BETA1 * np.abs(m) + (1.0 - BETA1) * np.abs(gs)
    return p1, m1, v1, A, denom


def bn_affine(mean, var, gamma, beta):
    """invstd = 1 / sqrt(var + 1e-5), scale = gamma * invstd, shift = beta - mean * scale."""
    invstd = 1.0 / np.sqrt(_f64(var) + BN_EPS)
    scale = _f64(gamma) * invstd
    return invstd, scale, _f64(beta) - _f64(mean) * scale


def bn_finalize_ref(y, gamma, beta, rm0, rv0, nbt0=0):
    """nn.BatchNorm2d (eps 1e-5, momentum 0.1) on the raw conv output y [N, H, W, C], in fp64.  Returns a dict:
    count; mean, var (biased), unbiased, abs_mean = E|y|, sq_mean = E[y^2] per channel; the training-mode affine invstd, scale,
    shift from the batch statistics; rm1 = 0.9 rm0 + 0.1 mean, rv1 = 0.9 rv0 + 0.1 unbiased, nbt1 = nbt0 + 1; and the eval-mode
    affine eval_invstd, eval_scale, eval_shift computed from the running statistics rm0, rv0 that were passed in."""
    y = _f64(y)
    C = y.shape[-1]
    y2 = y.reshape(-1, C)
    n = y2.shape[0]
    mean = y2.mean(axis=0)
    var = ((y2 - mean) ** 2).mean(axis=0)
    unbiased = var * n / (n - 1) if n > 1 else var
    invstd, scale, shift = bn_affine(mean, var, gamma, beta)
    e_invstd, e_scale, e_shift = bn_affine(rm0, rv0, gamma, beta)
    return {"count": n, "mean": mean, "var": var, "unbiased": unbiased, "abs_mean": np.abs(y2).mean(axis=0),
            "sq_mean": (y2 * y2).mean(axis=0), "invstd": invstd, "scale": scale, "shift": shift,
            "rm1": (1.0 - BN_MOMENTUM) * _f64(rm0) + BN_MOMENTUM * mean,
            "rv1": (1.0 - BN_MOMENTUM) * _f64(rv0) + BN_MOMENTUM * unbiased, "nbt1": int(nbt0) + 1,
            "eval_invstd": e_invstd, "eval_scale": e_scale, "eval_shift": e_shift}


def desc_normalize_ref(y, scale, shift):
    """r = y * scale + shift over the last axis (the descriptor channels), then r / ||r||_2 per cell: no epsilon, like the
    reference.  Returns (desc, norm) in fp64; norm has the shape of y without its last axis."""
    r = _f64(y) * _f64(scale) + _f64(shift)
    norm = np.sqrt((r * r).sum(axis=-1))
    return r / norm[..., None], norm
