"""CPU: tests/step_state_ref.py (the fp64 references of tests/test_gpu_step_state_exact.py) against torch in float64."""
import numpy as np
import torch

from tests import step_state_ref as R


def _adam_case(seed=0, n=4096):
    rs = np.random.RandomState(seed)
    p = rs.standard_normal(n) * 0.05
    m = rs.standard_normal(n) * 1e-2
    v = rs.uniform(0.0, 1.0, n) ** 4 * 1e-2
    g = [rs.standard_normal(n) * 10.0 ** rs.uniform(-6, 1, n) for _ in range(3)]
    return p, m, v, g


def test_adam_ref_equals_torch_adam_in_float64():
    """Three consecutive steps from non-zero state (exp_avg, exp_avg_sq and step preloaded): parameters to 1e-14 relative (of the
    parameter and its update); the moments to 1e-14 of the magnitudes they are sums of (torch evaluates m + (g - m) (1 - beta1), a different rounding of the same
    value, so where m and g cancel the difference is relative to A = 0.9 |m| + 0.1 |g|, not to the result)."""
    p0, m0, v0, grads = _adam_case()
    lr, t0 = 1e-3, 7
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr)
    opt.state[tp] = {"step": torch.tensor(float(t0)), "exp_avg": torch.from_numpy(m0.copy()), "exp_avg_sq": torch.from_numpy(v0.copy())}
    p, m, v = p0, m0, v0
    for k, g in enumerate(grads):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p_prev = p
        p, m, v, A, denom = R.adam_ref(p, g, m, v, lr, t0 + 1 + k)
        st = opt.state[tp]
        got = (tp.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy())
        assert int(st["step"]) == t0 + 1 + k
        assert np.all(np.abs(got[1] - m) <= 1e-14 * A), k
        assert np.all(np.abs(got[2] - v) <= 1e-14 * v), k
        assert np.all(np.abs(got[0] - p) <= 1e-14 * (np.abs(p) + np.abs(p - p_prev))), k
        assert np.all(denom > 0) and np.all(A >= np.abs(m) * (1 - 1e-15))
        p, m, v = got   # the next reference step starts from torch's state: the 1e-14 does not compound through cancellations
    assert np.abs(p - p0).max() > 1e-4   # the three steps moved the parameters


def test_adam_ref_grad_scale_is_a_scaled_gradient():
    p, m, v, grads = _adam_case(seed=1)
    for s in (1.0, 0.125, 1.0 / 3.0):
        a = R.adam_ref(p, grads[0], m, v, 1e-4, 3, grad_scale=s)
        b = R.adam_ref(p, grads[0] * s, m, v, 1e-4, 3)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), s
    assert np.array_equal(R.adam_ref(p, grads[0], m, v, 1e-4, 3)[0], R.adam_ref(p, grads[0], m, v, 1e-4, 3, grad_scale=1.0)[0])


def test_adam_ref_first_step_from_zero_moments_moves_by_lr():
    """t = 1, zero moments: the update is lr * g / (|g| + eps), i.e. lr * sign(g) for |g| >> 1e-8."""
    g = np.array([1e-3, -2.0, 5e3, 0.0])
    p1, m1, v1, A, denom = R.adam_ref(np.zeros(4), g, np.zeros(4), np.zeros(4), 1e-3, 1)
    assert np.allclose(p1[:3], -1e-3 * np.sign(g[:3]), rtol=1e-4, atol=0) and p1[3] == 0.0
    assert np.allclose(m1, 0.1 * g, rtol=1e-15) and np.allclose(v1, 0.001 * g * g, rtol=1e-14)


def _bn_case(seed=2, N=3, H=5, W=7, C=6):
    rs = np.random.RandomState(seed)
    y = rs.standard_normal((N, H, W, C)) * rs.uniform(0.1, 3.0, C) + rs.uniform(-2, 2, C)
    return y, rs.uniform(-1.5, 1.5, C), rs.uniform(-1, 1, C), rs.uniform(-1, 1, C), rs.uniform(0.5, 2.0, C)


def test_bn_finalize_ref_equals_torch_batchnorm_in_float64():
    """One training forward (output, running statistics, num_batches_tracked) and one eval forward from non-default running
    statistics and a non-zero counter."""
    y, gamma, beta, rm0, rv0 = _bn_case()
    C = y.shape[-1]
    bn = torch.nn.BatchNorm2d(C, dtype=torch.float64)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm0))
        bn.running_var.copy_(torch.from_numpy(rv0))
        bn.num_batches_tracked.fill_(41)
    x = torch.from_numpy(y).permute(0, 3, 1, 2).contiguous()
    r = R.bn_finalize_ref(y, gamma, beta, rm0, rv0, nbt0=41)
    # eval forward first (it changes nothing): the affine of the running statistics
    bn.eval()
    with torch.no_grad():
        out = bn(x).permute(0, 2, 3, 1).numpy()
    assert np.allclose(out, y * r["eval_scale"] + r["eval_shift"], rtol=1e-13, atol=1e-13)
    assert int(bn.num_batches_tracked) == 41 and np.array_equal(bn.running_mean.numpy(), rm0)
    bn.train()
    with torch.no_grad():
        out = bn(x).permute(0, 2, 3, 1).numpy()
    assert np.allclose(out, y * r["scale"] + r["shift"], rtol=1e-13, atol=1e-13)
    assert np.allclose(bn.running_mean.numpy(), r["rm1"], rtol=1e-14, atol=1e-15)
    assert np.allclose(bn.running_var.numpy(), r["rv1"], rtol=1e-14, atol=0)
    assert int(bn.num_batches_tracked) == r["nbt1"] == 42
    # the pieces
    assert r["count"] == 3 * 5 * 7
    y2 = y.reshape(-1, C)
    assert np.allclose(r["var"], r["sq_mean"] - r["mean"] ** 2, rtol=1e-12)
    assert np.allclose(r["unbiased"], y2.var(axis=0, ddof=1), rtol=1e-13)
    assert np.allclose(r["abs_mean"], np.abs(y2).mean(axis=0), rtol=1e-15)
    assert np.allclose(r["invstd"], 1.0 / np.sqrt(r["var"] + 1e-5), rtol=1e-15)


def test_desc_normalize_ref_equals_torch():
    rs = np.random.RandomState(3)
    y, sc, sh = rs.standard_normal((2, 3, 4, 256)), rs.uniform(0.5, 2, 256), rs.uniform(-1, 1, 256)
    d, n = R.desc_normalize_ref(y, sc, sh)
    t = torch.from_numpy(y * sc + sh).permute(0, 3, 1, 2)
    dn = torch.norm(t, p=2, dim=1)                      # models/SuperPointNet_gauss2.py:64-65
    want = t.div(torch.unsqueeze(dn, 1)).permute(0, 2, 3, 1).numpy()
    assert np.allclose(d, want, rtol=1e-14, atol=1e-16) and np.allclose(n, dn.numpy(), rtol=1e-14)
    assert np.allclose((d * d).sum(-1), 1.0, rtol=1e-14)
