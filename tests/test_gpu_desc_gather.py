"""GPU: the match term of the sparse descriptor loss as a gather - per-cell corner lists (desc_csr_kernel), two gradient rows per
match (desc_match_kernel<.., GATHER>) and the per-cell sum (desc_gather_cell) - against a NumPy restatement of the bilinear set-up,
against the atomic scatter on identical inputs, against the golden fixtures of the reference, and through the whole pair step.

Shapes: 8x12 and 6x8 cells, B = 3 (not a multiple of the 8 XCD slots of the work split), D = 256, n_match 1 (< 4 waves of a block),
37 (no multiple of 4) and 130 (more matches than cells: long lists).  The g4 fixture adds 1000 matches on 24 cells: lists of more than
64 entries, the chunk size of the gather."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import golden_util as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
VARIANTS = [("2d", "cos"), ("1d", "cos"), ("2d", "euclidean"), ("1d", "euclidean")]
GRIDS = [(8, 12), (6, 8)]
N_MATCH = [1, 37, 130]
SETS = ["mixed", "one_cell"]
B = 3
N_NON = 5


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---- NumPy restatement of bilin_setup / bilin_cell (csrc/loss_kernels.hip.h) as compiled, every operation in fp32 -----------------------------
def bilin_np(cell, Hc, Wc, method):
    """[(corner cell, weight)] of one match in the order nw, ne, sw, se; out-of-range corners carry weight 0."""
    if method == "1d":
        return [(cell, F(1.0))]
    u, v = F(cell % Wc), F(cell // Wc)
    gx = u / F(Wc) * F(2) - F(1)
    gy = v / F(Hc) * F(2) - F(1)
    ix = ((gx + F(1)) / F(2)) * F(Wc - 1)
    iy = ((gy + F(1)) / F(2)) * F(Hc - 1)
    fx, fy = np.floor(ix), np.floor(iy)
    x0, y0 = int(fx), int(fy)
    # `ix - floorf(ix)` is ONE fused multiply-add in the compiled bilin_setup (fp contraction: ix = t * (Wc - 1) is not rounded in front
    # of the subtraction), in the scatter kernel as in the list kernel.  fp64 holds the product of two fp32 exactly, so one rounding
    # of the fp64 expression is that instruction.
    ax = F(np.float64((gx + F(1)) / F(2)) * np.float64(Wc - 1) - np.float64(fx))
    ay = F(np.float64((gy + F(1)) / F(2)) * np.float64(Hc - 1) - np.float64(fy))
    out = []
    for (x, y, w) in ((x0, y0, (F(1) - ax) * (F(1) - ay)), (x0 + 1, y0, ax * (F(1) - ay)),
                      (x0, y0 + 1, (F(1) - ax) * ay), (x0 + 1, y0 + 1, ax * ay)):
        ok = 0 <= x < Wc and 0 <= y < Hc
        out.append((min(max(y, 0), Hc - 1) * Wc + min(max(x, 0), Wc - 1), F(w) if ok else F(0)))
    return out


def csr_np(match, Hc, Wc, method):
    """per-cell lists of one (image, side): {cell: [(match index, weight), ...]} with ascending match index; zero weights dropped."""
    lists = {c: [] for c in range(Hc * Wc)}
    for k, cell in enumerate(match.tolist()):
        for c, w in bilin_np(cell, Hc, Wc, method):
            if w != 0:
                lists[c].append((k, w))
    return lists


# ---- hand-built index sets -----------------------------------------------------------------------------------------------------
def _border_cells(Hc, Wc):
    corners = [0, Wc - 1, (Hc - 1) * Wc, Hc * Wc - 1]
    top = list(range(Wc))
    bottom = [(Hc - 1) * Wc + x for x in range(Wc)]
    left = [y * Wc for y in range(Hc)]
    right = [y * Wc + Wc - 1 for y in range(Hc)]
    return corners + top + bottom + left + right


def index_set(name, Hc, Wc, n):
    """(match_a, match_b) int32 [B, n].
    mixed:    image 0 - side a walks the four corners and the border rows / columns (corner weights 0, cells outside), side b puts three
              consecutive matches into every cell it uses (several matches per cell, the other cells empty);
              image 1 - side a spreads over the grid, side b sits in ONE interior cell with every match;
              image 2 - identical match_a / match_b.
    one_cell: every match of a side in one cell - per image the first corner, an interior cell, the last corner (a) and the reverse (b)."""
    cells = Hc * Wc
    k = np.arange(n)
    if name == "mixed":
        bc = np.array(_border_cells(Hc, Wc))
        a0, b0 = bc[k % len(bc)], (k // 3 * 5 + 2) % cells
        a1, b1 = (k * 7 + 3) % cells, np.full(n, (Hc // 2) * Wc + Wc // 2)
        a2 = (k * 11 + 5) % cells
        ma, mb = np.stack([a0, a1, a2]), np.stack([b0, b1, a2])
    else:
        one = [0, (Hc // 2) * Wc + Wc // 3, cells - 1]
        ma = np.stack([np.full(n, c) for c in one])
        mb = np.stack([np.full(n, c) for c in reversed(one)])
    return ma.astype(np.int32), mb.astype(np.int32)


def descriptors(Hc, Wc, seed):
    """unit descriptors with a shared component: most non-match dot products lie above the 0.2 margin (hard negatives exist)."""
    rs = np.random.RandomState(seed)
    common = rs.randn(1, 256, 1, 1)
    d = rs.randn(B, 256, Hc, Wc) + 0.6 * common
    dw = 0.6 * d + 0.8 * rs.randn(B, 256, Hc, Wc)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dw /= np.linalg.norm(dw, axis=1, keepdims=True)
    return torch.from_numpy(d.astype(np.float32)), torch.from_numpy(dw.astype(np.float32))


def case_inputs(Hc, Wc, n, name, collision_free=False):
    dev = _dev()
    ma, mb = index_set(name, Hc, Wc, n)
    rs = np.random.RandomState(1000 * Hc + 10 * n + len(name))
    if collision_free:   # every address of the non-match scatter receives ONE atomic: see test_gather_is_bit_reproducible
        n_non = 2
        assert n * n_non <= Hc * Wc
        ma = np.stack([rs.permutation(Hc * Wc)[:n] for _ in range(B)]).astype(np.int32)
        nm = np.stack([rs.permutation(Hc * Wc)[:n * n_non] for _ in range(B)]).astype(np.int32)
    else:
        nm = rs.randint(0, Hc * Wc, size=(B, n * N_NON)).astype(np.int32)
    d, dw = descriptors(Hc, Wc, seed=Hc + n)
    return d.to(dev), dw.to(dev), torch.from_numpy(ma).to(dev), torch.from_numpy(mb).to(dev), torch.from_numpy(nm).to(dev)


CASES = [(hc, wc, n, s) for (hc, wc) in GRIDS for n in N_MATCH for s in SETS]


@pytest.mark.parametrize("method", ["2d", "1d"])
@pytest.mark.parametrize("Hc,Wc,n,name", CASES)
def test_corner_lists_match_numpy(Hc, Wc, n, name, method):
    """The CSR arrays of every (image, side): counts per cell, the (match, weight) entries of every cell - integers exact, weights within
    1 ulp - and ascending match order within a cell."""
    from semantic_superpoint_amd import lib as L
    d, dw, ma, mb, nm = case_inputs(Hc, Wc, n, name)
    *_, (off, em, ew) = L.op_sparse_loss(d, dw, ma, mb, nm, method=method, grad=(1.0, 1.0), gather=True, csr=True)
    off, em, ew = off.cpu().numpy(), em.cpu().numpy(), ew.cpu().numpy()
    for img in range(B):
        for side, mt in enumerate((ma, mb)):
            want = csr_np(mt[img].cpu().numpy(), Hc, Wc, method)
            o = off[img, side]
            counts = np.array([len(want[c]) for c in range(Hc * Wc)])
            assert o[0] == 0 and np.array_equal(np.diff(o), counts), (img, side)
            assert o[-1] <= 4 * n
            for c in range(Hc * Wc):
                got_m, got_w = em[img, side, o[c]:o[c + 1]], ew[img, side, o[c]:o[c + 1]]
                assert np.all(np.diff(got_m) > 0), (img, side, c, got_m)                       # ascending, no repeats
                assert got_m.tolist() == [k for k, _ in want[c]], (img, side, c)               # with the line above: the multiset, exactly
                ww = np.array([w for _, w in want[c]], dtype=np.float32)
                assert np.all(np.abs(got_w - ww) <= np.spacing(ww)), (img, side, c, got_w, ww)  # 1 ulp
    if name == "one_cell":   # cells with no entry, and one cell that holds a corner of every match
        assert (np.diff(off[1, 0]) == 0).sum() >= Hc * Wc - 4 and np.diff(off[1, 0]).max() == n


@pytest.mark.parametrize("Hc,Wc,n,name", CASES)
def test_gather_equals_scatter(Hc, Wc, n, name):
    """Loss terms and the full gradients of both sides, gather against scatter on the same inputs, for every (method, dist): the two
    differ in summation order only.  Gradient bound: the one of test_sparse_loss_variants_golden (1e-7 + 2e-5 max|ref|)."""
    from semantic_superpoint_amd import lib as L
    d, dw, ma, mb, nm = case_inputs(Hc, Wc, n, name)
    for method, dist in VARIANTS:
        pg, ng, gag, gbg = L.op_sparse_loss(d, dw, ma, mb, nm, method=method, dist=dist, grad=(0.7, 1.3), gather=True)
        ps, ns, gas, gbs = L.op_sparse_loss(d, dw, ma, mb, nm, method=method, dist=dist, grad=(0.7, 1.3), gather=False)
        assert abs(pg - ps) < 1e-6 and abs(ng - ns) < 1e-6, (method, dist, pg, ps, ng, ns)
        for side, (mine, ref) in enumerate(((gag, gas), (gbg, gbs))):
            assert float(ref.abs().max()) > 0
            err = float((mine - ref).abs().max())
            assert err < 1e-7 + 2e-5 * float(ref.abs().max()), (method, dist, side, err, float(ref.abs().max()))


# (G4 stores the full gradients at the small size only: ("2d", "cos", "mid") has no fixture)
@pytest.mark.parametrize("method,dist,tag", [(m, d, t) for (m, d) in VARIANTS for t in ("small", "mid") if (m, d, t) != ("2d", "cos", "mid")])
def test_gather_golden(method, dist, tag):
    """The gather path against the g4 / g14 fixtures of the real reference, tolerances of test_sparse_loss_variants_golden."""
    from semantic_superpoint_amd import lib as L
    if (method, dist) == ("2d", "cos"):
        g = G.load("g4_sparse_loss_small.npz")
    else:
        g = G.load("g14_sparse_loss_%s_%s_%s.npz" % (method, dist, tag))
    dev = _dev()
    d, dw = torch.from_numpy(g["desc"]), torch.from_numpy(g["desc_w"])
    nb, _, Hc, Wc = d.shape
    idx = G.indices_from(g, "", nb)
    ma = torch.stack([(i["uv_a"][:, 0] + i["uv_a"][:, 1] * Wc) for i in idx]).to(torch.int32).to(dev).contiguous()
    mb = torch.stack([(i["uv_b"][:, 0] + i["uv_b"][:, 1] * Wc) for i in idx]).to(torch.int32).to(dev).contiguous()
    nm = torch.stack([i["nm_b"] for i in idx]).to(torch.int32).to(dev).contiguous()
    w = g["grad_weights"]
    pos, neg, ga, gb = L.op_sparse_loss(d.to(dev), dw.to(dev), ma, mb, nm, method=method, dist=dist,
                                        grad=(float(w[0] + w[1]), float(w[0] + w[2])), gather=True)
    assert abs(pos - float(g["pos"])) < 2e-5 * max(1.0, abs(float(g["pos"])))
    assert abs(neg - float(g["neg"])) < 2e-5 * max(1.0, abs(float(g["neg"])))
    for mine, ref in ((ga, g["ddesc"]), (gb, g["ddesc_w"])):
        ref = torch.from_numpy(ref)
        assert (mine.cpu() - ref).abs().max() < 1e-7 + 2e-5 * float(ref.abs().max())


@pytest.mark.parametrize("Hc,Wc,n,name,free", [c + (False,) for c in CASES] + [(8, 12, 37, "mixed", True), (6, 8, 1, "mixed", True)])
def test_gather_is_bit_reproducible(Hc, Wc, n, name, free):
    """The gather path twice on the same inputs, without deterministic mode: bit-identical gradients of both sides.  The lists fix the
    order of the match term's sum.  The NON-match term keeps its fp32 atomics (not part of the gather), whose order of arrival is free:
    the hand-built cases therefore run with coef_neg = 0 (the non-match atomics add zeros), and the `free` cases run BOTH terms on
    indices where every address of the non-match scatter receives exactly one atomic (distinct match_a, distinct non-matches)."""
    from semantic_superpoint_amd import lib as L
    d, dw, ma, mb, nm = case_inputs(Hc, Wc, n, name, collision_free=free)
    for method, dist in VARIANTS:
        grad = (0.7, 1.3) if free else (0.7, 0.0)
        _, _, ga1, gb1 = L.op_sparse_loss(d, dw, ma, mb, nm, method=method, dist=dist, grad=grad, gather=True)
        _, _, ga2, gb2 = L.op_sparse_loss(d, dw, ma, mb, nm, method=method, dist=dist, grad=grad, gather=True)
        assert float(ga1.abs().max()) > 0 and float(gb1.abs().max()) > 0
        assert torch.equal(ga1, ga2) and torch.equal(gb1, gb2), (method, dist)


_STEP_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from oracle import cpu_ref as C
from tests import golden_util as G
from semantic_superpoint_amd.lib import Engine
dev = torch.device("cuda:0")
arch = "SuperPointNet_gauss2_ssmall"
g = G.load("g6_step_ssp_64x96.npz")
sample = G.sample_from(g)
B, _, H, W = sample["image"].shape
e = Engine(arch, B, H, W, dev)
e.load_state_dict(C.init_state_dict(arch, seed=23))
idx = G.indices_from(g, "idx/", B)
Wc = W // 8
ma = torch.stack([(i["uv_a"][:, 0] + i["uv_a"][:, 1] * Wc) for i in idx]).to(torch.int32).to(dev).contiguous()
mb = torch.stack([(i["uv_b"][:, 0] + i["uv_b"][:, 1] * Wc) for i in idx]).to(torch.int32).to(dev).contiguous()
nm = torch.stack([i["nm_b"] for i in idx]).to(torch.int32).to(dev).contiguous()
e.zero_grad()
sc = e.pair_step({k: v.to(dev).contiguous() for k, v in sample.items()}, indices=(ma, mb, nm), train=True, lambda_loss=1.0, lamda_d=1.0,
                 multi_task=True)
torch.cuda.synchronize()
out = {"scalars": sc.cpu().numpy()}
for k, v in e.grad_dict().items():
    out["grad/" + k] = v.cpu().numpy()
np.savez(sys.argv[2], **out)
"""


def test_pair_step_gather_vs_scatter(tmp_path):
    """A full pair step (64x96, B = 2, the inputs of g6_step_ssp_64x96) with SSP_DESC_GATHER=0 and =1, each in a fresh process (the
    switch is read once): the scalars agree (TOL of the step-golden test, 1e-3 relative) and every gradient tensor agrees within that
    test's bounds - norm within 5e-3, no element off by more than 1e-4 of max|grad| (SLICE_TOL, here over the whole tensor)."""
    from oracle import cpu_ref as C
    runs = {}
    for v in ("0", "1"):
        out = str(tmp_path / ("step%s.npz" % v))
        env = dict(os.environ, SSP_DESC_GATHER=v)
        r = subprocess.run([sys.executable, "-c", _STEP_CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        runs[v] = dict(np.load(out))
    s0, s1 = runs["0"]["scalars"], runs["1"]["scalars"]
    assert np.all(np.isfinite(s1)) and np.all(np.abs(s1 - s0) < 1e-3 * np.maximum(1.0, np.abs(s0))), (s0, s1)
    arch = "SuperPointNet_gauss2_ssmall"
    noisy = {c + ".bias" for c, bn, _, _, _ in C.layer_table(arch) if bn is not None}
    worst = 0.0
    for k in C.param_keys(arch):
        if k in noisy:
            continue
        a, b = runs["0"]["grad/" + k].reshape(-1).astype(np.float64), runs["1"]["grad/" + k].reshape(-1).astype(np.float64)
        na = float(np.linalg.norm(a))
        assert abs(float(np.linalg.norm(b)) - na) < 5e-3 * na + 1e-6, k
        err = float(np.abs(a - b).max()) / (float(np.abs(a).max()) + 1e-30)
        worst = max(worst, err)
        assert err < 1e-4 + 1e-6, (k, err)
    print("pair step, gather vs scatter: worst element difference %.2e of max|grad|" % worst)
