"""CPU: the fp64 restatement of the loss phase (tests/loss_phase_ref.py) against what the project already trusts, and proof that the
bounds of tests/test_gpu_loss_exact.py can fail.

  * fp64 autograd of oracle.cpu_ref's detector_loss, sem_loss, sparse descriptor loss (every (method, dist), through the L2
    normalisation) and multi_task_loss on random tensors of the shapes of case A: agreement within 1e-10 * base;
  * the same for the dense descriptor loss (oracle.cpu_ref.descriptor_loss_dense, multi-task and uniform, through the normalisation);
  * the goldens of the real reference g3_detector_loss, g4_sparse_loss_small, g14_* and g10_dense_loss_small (the fixture of
    tests/test_gpu_dense.py) at the tolerances their GPU tests use;
  * every mutant of the restatement moves at least one element of the case-A inputs by more than TAU_MAX * base (TAU_MAX imported
    from the GPU module: the largest tau it uses);
  * the near-tie cap of the descriptor hinges holds for the index sets of every GPU case on unit descriptors built like
    tests/test_gpu_desc_gather.py::descriptors (the GPU cases assert it again on the descriptors the network produced).

One mutant of the list cannot be expressed on valid indices: "an out-of-range corner given its weight".  normPts followed by
grid_sample(align_corners=True) maps the integer cell u to ix = u (Wc - 1) / Wc, which lies in [0, Wc - 1): both corners of every
match are inside the grid, in fp32 as in fp64 (test_no_corner_is_ever_out_of_range walks every cell of the case grids).  The
zero-padding rule is therefore dead for the indices a step can receive - the branch of bilin_setup is unreachable from pair_step and
from ssp_op_sparse_loss with in-grid cells - and no input can tell the mutant from the reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref as C
from tests import golden_util as G
from tests import loss_phase_ref as R
from tests.test_gpu_loss_exact import TAU_MAX

B, H, W, HC, WC, N_MATCH, N_NON, NC = 3, 64, 96, 8, 12, 130, 5, 133
ETA = R.ETA_TEST
VARIANTS = [("2d", "cos"), ("1d", "cos"), ("2d", "euclidean"), ("1d", "euclidean")]
GPU_GRIDS = [(3, 8, 12, 130), (16, 15, 20, 300)]   # (B, Hc, Wc, n_match) of the GPU cases with a descriptor loss


def _agree(got, ref, base, tol=1e-10):
    r, i = R.ratio(got, ref.double(), base)
    assert r <= tol, (r, i)


@pytest.fixture(scope="module")
def case_a():
    """random stand-ins for the network outputs of case A, and its real label / mask / index inputs"""
    g = torch.Generator().manual_seed(5)
    d = {"labels": [R.make_labels(B, H, W, 11), R.make_labels(B, H, W, 12)],
         "mask": [R.make_mask(B, H, W, 21), R.make_mask(B, H, W, 22, full_image=1)],
         "sem": [R.make_sem_labels(B, H, W, NC, 31), R.make_sem_labels(B, H, W, NC, 32, extra_ignored=True)],
         "idx": R.make_indices(B, HC, WC, N_MATCH, N_NON, 41)}
    d["y9"] = [torch.randn(B, HC, WC, 65, generator=g) * 2 for _ in range(2)]
    d["aff9"] = [(torch.rand(65, generator=g) + 0.5, torch.randn(65, generator=g) * 0.3) for _ in range(2)]
    d["y13"] = [torch.randn(B, HC, WC, NC, generator=g) * 2 for _ in range(2)]
    da, db = R.unit_descriptors(B, HC, WC, 7)
    scale = [torch.rand(B, HC * WC, 1, generator=g) * 3 + 0.5 for _ in range(2)]
    d["raw"] = [da * scale[0], db * scale[1]]   # what the normalisation sees: raw = desc * norm
    return d


def test_inputs_hold_what_the_cases_claim(case_a):
    for v in range(2):
        cm, cnt = R.cell_mask(case_a["mask"][v])
        _, lsum = R.detector_target(case_a["labels"][v])
        assert 0 < cnt < B * HC * WC
        for kind, (cy, cx) in R.LABEL_CELLS.items():
            assert cm[0, cy, cx] == 1
            s = float(lsum[0, cy, cx])
            assert {"zero": s == 0, "below_one": 0 < s < 1, "one": s == 1, "above_one": s > 1}[kind], (kind, s)
        assert ((lsum > 1) & (cm == 1)).sum() > 4
        lab = case_a["labels"][v]
        assert len(torch.unique(lab)) > 3 and torch.equal(lab * 4, (lab * 4).round())   # Gaussian-valued, dyadic
        sem = case_a["sem"][v]
        assert (sem[0, :8] == NC).all() and (sem == 255).any() and (sem == -1).any()
    assert R.cell_mask(case_a["mask"][1])[0][1].sum() == 0                    # image 1 of the warped view: fully masked
    assert R.cell_mask(case_a["mask"][0])[1] != R.cell_mask(case_a["mask"][1])[1]
    assert R.sem_count(case_a["sem"][0], NC) != R.sem_count(case_a["sem"][1], NC)
    ma, mb, nm = case_a["idx"]
    assert torch.equal(ma[2], mb[2]) and len(torch.unique(mb[1])) == 1 and int(nm.max()) < HC * WC


# ---- against fp64 autograd of the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [0, 1])
def test_detector_root_is_the_oracles_gradient(case_a, v):
    sc, sh = case_a["aff9"][v]
    semi = R.fma32(case_a["y9"][v], sc, sh).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    cm, cnt = R.cell_mask(case_a["mask"][v])
    assert torch.equal(C.get_masks(case_a["mask"][v].double()).double(), cm)
    target = C.labels2Dto3D(case_a["labels"][v].double())
    loss = C.detector_loss(semi, target, cm)
    coef = 0.37
    g, = torch.autograd.grad(loss * coef, semi)
    r = R.detector_root(case_a["y9"][v], sc, sh, case_a["labels"][v], cm, coef, cnt)
    _agree(r["d"], g.permute(0, 2, 3, 1), r["d_base"])
    assert abs(r["loss"] - float(loss.detach())) <= 1e-10 * r["loss_base"]
    assert torch.equal(R.detector_target(case_a["labels"][v])[0], target.permute(0, 2, 3, 1))


@pytest.mark.parametrize("v", [0, 1])
def test_sem_root_is_the_oracles_gradient(case_a, v):
    lab = case_a["sem"][v]
    lab_o = torch.where((lab < 0) | (lab >= NC), torch.full_like(lab, NC), lab)   # the oracle ignores the value C only
    sout = case_a["y13"][v].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    loss = C.sem_loss(F.interpolate(sout, (H, W), mode="bilinear", align_corners=False), lab_o)
    coef = 1.9
    g, = torch.autograd.grad(loss * coef, sout)
    cnt = R.sem_count(lab, NC)
    assert cnt == int((lab_o != NC).sum()) < lab.numel()
    r = R.sem_root(case_a["y13"][v], lab, NC, coef, cnt)
    _agree(r["d"], g.permute(0, 2, 3, 1), r["d_base"])
    assert abs(r["loss"] - float(loss.detach())) <= 1e-10 * r["loss_base"]
    sub = R.sem_root(case_a["y13"][v], lab, NC, coef, cnt, images=[0, 2])       # a subset of the images: the same rows, the same loss
    assert torch.equal(sub["d"], r["d"][[0, 2]]) and sub["loss"] == r["loss"]


def _oracle_idx(ma, mb, nm, i):
    uv = lambda m: torch.stack((m[i] % WC, m[i] // WC), 1).double()   # noqa: E731
    return {"uv_a": uv(ma), "uv_b": uv(mb), "nm_b": nm[i].long()}


@pytest.mark.parametrize("method,dist", VARIANTS)
def test_descriptor_root_is_the_oracles_gradient(case_a, method, dist):
    ma, mb, nm = case_a["idx"]
    raw = [r.double().requires_grad_(True) for r in case_a["raw"]]
    unit = [r / r.norm(dim=-1, keepdim=True) for r in raw]
    nchw = [u.reshape(B, HC, WC, 256).permute(0, 3, 1, 2) for u in unit]
    cpos, cneg = 0.8, 1.3
    ps, ns = [], []
    for i in range(B):
        _, p, n = C.descriptor_loss_sparse_given(nchw[0][i], nchw[1][i], _oracle_idx(ma, mb, nm, i), 1.0, N_NON, dist, method)
        ps.append(p), ns.append(n)
    pos, neg = torch.stack(ps), torch.stack(ns)
    ga, gb = torch.autograd.grad(cpos * pos.mean() + cneg * neg.mean(), raw)
    inv = [1.0 / r.detach().norm(dim=-1) for r in raw]
    r = R.sparse_desc_root(unit[0].detach(), unit[1].detach(), inv[0], inv[1], ma, mb, nm, cpos, cneg, HC, WC, method, dist, coords="fp64")
    assert not r["ties"]
    _agree(r["root"][0], ga, r["base"][0])
    _agree(r["root"][1], gb, r["base"][1])
    assert ((r["pos"] - pos.detach()).abs() <= 1e-10 * r["pos_base"]).all()
    assert ((r["neg"] - neg.detach()).abs() <= 1e-10 * r["neg_base"]).all()
    assert float(r["nnz"].min()) > 0
    if dist == "cos":   # active and inactive non-match hinges (two unit vectors of different views are never within 0.2)
        assert float(r["nnz"].max()) < N_MATCH * N_NON


DENSE = dict(B=2, Hc=8, Wc=12, seed=51)   # case D of the GPU module


def _dense_case():
    da, db = R.unit_descriptors(DENSE["B"], DENSE["Hc"], DENSE["Wc"], 10)
    g = torch.Generator().manual_seed(6)
    raw = [(da * (torch.rand(2, 96, 1, generator=g) * 3 + 0.5)).double(), (db * (torch.rand(2, 96, 1, generator=g) * 3 + 0.5)).double()]
    valid = R.cell_mask(R.make_mask(2, 64, 96, 22, full_image=1))[0].reshape(2, 96)
    return raw, R.make_homographies(2, DENSE["seed"]), valid


@pytest.mark.parametrize("multi_task", [True, False])
def test_dense_root_is_the_oracles_gradient(multi_task):
    raw, hm, valid = _dense_case()
    raw = [r.requires_grad_(True) for r in raw]
    unit = [r / r.norm(dim=-1, keepdim=True) for r in raw]
    nchw = [u.reshape(2, 8, 12, 256).permute(0, 3, 1, 2) for u in unit]
    loss, mask, pos, neg = C.descriptor_loss_dense(nchw[0], nchw[1], hm, mask_valid=valid.reshape(2, 1, 8, 12), lamda_d=250.0, descriptor_dist=4.0)
    coef = 0.7
    ga, gb = torch.autograd.grad(coef * ((pos + neg) if multi_task else loss), raw)
    inv = [1.0 / r.detach().norm(dim=-1) for r in raw]
    r = R.dense_desc_root(unit[0].detach(), unit[1].detach(), inv[0], inv[1], hm, valid, coef, multi_task, 8, 12)
    assert not r["ties"] and 0 < valid.sum() < valid.numel()
    assert torch.equal(r["mask"], mask.reshape(2, 96, 96).double()) and 0 < r["mask"].sum() < 400   # the oracle's fp32 mask, no near-tie
    _agree(r["root"][0], ga, r["base"][0])
    _agree(r["root"][1], gb, r["base"][1])
    for k, v in (("ldesc", loss), ("pos", pos), ("neg", neg)):
        assert abs(r[k] - float(v.detach())) <= 1e-10 * r[k + "_base"], k
    assert r["ldesc"] < r["pos"] + r["neg"]   # the valid mask enters loss_desc only


def test_dense_golden_g10_small():
    g = G.load("g10_dense_loss_small.npz")
    d, dw = torch.from_numpy(g["desc"]), torch.from_numpy(g["desc_w"])
    nb, _, hc, wc = d.shape
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(nb, hc * wc, 256)   # noqa: E731
    mv = torch.from_numpy(g["mask_valid"]).reshape(nb, -1)
    for multi_task, scale, key in ((False, 1.0, "g_loss"), (True, 0.5, "g_mt")):
        r = R.dense_desc_root(flat(d), flat(dw), None, None, g["homographies"], mv, scale, multi_task, hc, wc)
        assert torch.equal(r["mask"], torch.from_numpy(g["mask"]).reshape(nb, hc * wc, hc * wc).double())
        assert abs(r["ldesc"] - float(g["loss"])) < 1e-5 and abs(r["pos"] - float(g["pos_sum"])) < 1e-5
        assert abs(r["neg"] - float(g["neg_sum"])) < 1e-7
        for side, nm in enumerate(("_a", "_b")):
            assert (r["root"][side] - flat(torch.from_numpy(g[key + nm])).double()).abs().max() < 1e-6


def test_dense_mutants_and_near_tie_cap():
    raw, hm, valid = _dense_case()
    unit = [(r / r.norm(dim=-1, keepdim=True)).float() for r in raw]
    inv = [1.0 / r.norm(dim=-1) for r in raw]
    cneg = R.coefficients(ETA, True)[2]
    args = (unit[0], unit[1], inv[0], inv[1], hm, valid, cneg, True, 8, 12)
    r = R.dense_desc_root(*args)
    assert len(r["ties"]) <= R.NEAR_TIE_CAP * r["n_terms"]
    cnt0 = R.cell_mask(R.make_mask(2, 64, 96, 21))[1]
    assert cnt0 != float(valid.sum())
    muts = {"normaliser from view 0's mask count": R.dense_desc_root(*args, norm_count=cnt0),
            "normalisation backward without d <g, d>": R.dense_desc_root(*args, drop_projection=True),
            "margin 0.25": R.dense_desc_root(*args, margin_neg=0.25),
            "valid mask in the multi-task gradient": R.dense_desc_root(*args[:7], False, 8, 12)}
    for name, m in muts.items():
        for v in range(2):
            assert _rejected(m["root"][v], r["root"][v], r["base"][v], r["allow"][v]), (name, v)
    m = muts["normaliser from view 0's mask count"]
    for k in ("ldesc", "pos", "neg"):
        assert abs(m[k] - r[k]) > TAU_MAX * r[k + "_base"] + r[k + "_allow"], k


@pytest.mark.parametrize("semantic", [True, False])
def test_scalars_are_the_oracles_multi_task_loss(semantic):
    eta = torch.tensor(ETA, dtype=torch.float64, requires_grad=True)
    det, sem = [(1.7, 1.7), (0.9, 0.9)], [(4.1, 4.1), (3.3, 3.3)]
    desc = {k: torch.tensor(v, dtype=torch.float64) for k, v in (("pos", [0.2, 0.4]), ("neg", [0.1, 0.3]), ("pos_base", [1.0, 1.0]),
                                                                    ("neg_base", [1.0, 1.0]), ("pos_allow", [0.0, 0.0]), ("neg_allow", [0.0, 0.0]))}
    t = lambda x: torch.tensor(x, dtype=torch.float64)   # noqa: E731
    loss = C.multi_task_loss(eta, t(1.7 + 0.9), t(0.3), t(0.2), t(4.1 + 3.3) if semantic else None)
    g, = torch.autograd.grad(loss, eta)
    vals, bases, allow, deta, deta_b, _ = R.step_scalars(ETA, det, sem, desc, True, 1.0, 2.5, semantic)
    assert abs(vals[0] - float(loss.detach())) <= 1e-12 * bases[0]
    assert np.allclose(deta, g.numpy(), rtol=0, atol=1e-12)
    assert vals[1:8] == [1.7, 0.9, pytest.approx(2.5 * 0.3 + 0.2), 4.1 if semantic else 0.0, 3.3 if semantic else 0.0, pytest.approx(0.3),
                         pytest.approx(0.2)]
    assert vals[8:] == list(ETA)
    # the uniform sum and the single-view step
    vals, *_, deta, _, _ = R.step_scalars(ETA, det, sem, desc, False, 0.5, 3.0, semantic)
    assert vals[0] == pytest.approx(2.6 + (7.4 if semantic else 0.0) + 0.5 * (3.0 * 0.3 + 0.2)) and deta == [0.0, 0.0, 0.0]
    vals, *_, deta, _, _ = R.step_scalars(ETA, [det[0], (0.0, 0.0)], [sem[0], (0.0, 0.0)], None, True, 0.0, 1.0, semantic)
    one = C.multi_task_loss(eta, t(1.7), t(0.0), t(0.0), t(4.1) if semantic else None)
    g, = torch.autograd.grad(one, eta)
    assert vals[0] == pytest.approx(float(one.detach()), rel=1e-14) and deta[1] == 0.5 and np.allclose(deta, g.numpy(), rtol=0, atol=1e-12)
    assert vals[2] == vals[3] == vals[5] == vals[6] == vals[7] == 0.0


# ---- against the goldens of the real reference -------------------------------------------------------------------------------------
def test_detector_root_golden_g3():
    g = G.load("g3_detector_loss.npz")
    tgt = torch.from_numpy(g["target"])
    nb, _, hc, wc = tgt.shape
    lab2d = tgt[:, :64].view(nb, 8, 8, hc, wc).permute(0, 3, 1, 4, 2).reshape(nb, 1, hc * 8, wc * 8).contiguous()
    cm = torch.from_numpy(g["mask"]).double()
    y = torch.from_numpy(g["semi"]).permute(0, 2, 3, 1)
    r = R.detector_root(y, torch.ones(65), torch.zeros(65), lab2d, cm, 1.0, float(cm.sum()))
    ref = torch.from_numpy(g["dsemi"]).permute(0, 2, 3, 1).double()
    assert abs(r["loss"] - float(g["loss"])) < 1e-5 * max(1.0, abs(float(g["loss"])))
    assert (r["d"] - ref).abs().max() < 1e-6 + 1e-4 * float(ref.abs().max())


@pytest.mark.parametrize("method,dist,tag", [(m, d, t) for (m, d) in VARIANTS for t in ("small", "mid") if (m, d, t) != ("2d", "cos", "mid")])
def test_descriptor_gradient_goldens_g4_g14(method, dist, tag):
    g = G.load("g4_sparse_loss_small.npz" if (method, dist) == ("2d", "cos") else "g14_sparse_loss_%s_%s_%s.npz" % (method, dist, tag))
    d, dw = torch.from_numpy(g["desc"]), torch.from_numpy(g["desc_w"])
    nb, _, hc, wc = d.shape
    idx = G.indices_from(g, "", nb)
    ma = torch.stack([(i["uv_a"][:, 0] + i["uv_a"][:, 1] * wc) for i in idx]).long()
    mb = torch.stack([(i["uv_b"][:, 0] + i["uv_b"][:, 1] * wc) for i in idx]).long()
    nm = torch.stack([i["nm_b"] for i in idx])
    w = g["grad_weights"]
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(nb, hc * wc, 256)   # noqa: E731
    r = R.sparse_desc_root(flat(d), flat(dw), None, None, ma, mb, nm, float(w[0] + w[1]), float(w[0] + w[2]), hc, wc, method, dist)
    assert abs(float(r["pos"].mean()) - float(g["pos"])) < 2e-5 * max(1.0, abs(float(g["pos"])))
    assert abs(float(r["neg"].mean()) - float(g["neg"])) < 2e-5 * max(1.0, abs(float(g["neg"])))
    for mine, ref in ((r["root"][0], g["ddesc"]), (r["root"][1], g["ddesc_w"])):
        ref = flat(torch.from_numpy(ref)).double()
        assert (mine - ref).abs().max() < 1e-7 + 2e-5 * float(ref.abs().max())


# ---- the bilinear set-up ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hc,wc", [(8, 12), (15, 20), (6, 8), (30, 40)])
def test_no_corner_is_ever_out_of_range(hc, wc):
    """see the module docstring: the zero-padding rule of grid_sample cannot fire for an integer cell of the grid; also the fp32
    set-up against the per-match restatement of tests/test_gpu_desc_gather.py and against the fp64 formulas"""
    from tests.test_gpu_desc_gather import bilin_np
    cells = np.arange(hc * wc)
    assert R.corners_out_of_range(cells, hc, wc) == 0
    i32, w32 = R.bilinear_corners(cells, hc, wc, "2d", "fp32")
    i64, w64 = R.bilinear_corners(cells, hc, wc, "2d", "fp64")
    assert (w32.sum(1) - 1).abs().max() < 1e-6 and (w64.sum(1) - 1).abs().max() < 1e-12
    for c in cells:
        want = bilin_np(int(c), hc, wc, "2d")
        assert [int(x) for x in i32[c]] == [k for k, _ in want] and [float(x) for x in w32[c]] == [float(x) for _, x in want]
    # fp32 and fp64 may floor differently where ix is an integer up to rounding; the sampled value is the same up to 1e-6
    m32, m64 = torch.zeros(hc * wc, hc * wc, dtype=torch.float64), torch.zeros(hc * wc, hc * wc, dtype=torch.float64)
    m32.scatter_add_(1, i32, w32)
    m64.scatter_add_(1, i64, w64)
    assert (m32 - m64).abs().max() < 4e-6


# ---- the bounds can fail --------------------------------------------------------------------------------------------------------------
def _rejected(mut, ref, base, allow=None):
    d = (mut - ref).abs() - (0 if allow is None else allow)
    return bool((d > TAU_MAX * base).any())


def test_tau_max_is_a_tolerance():
    assert 0 < TAU_MAX < 1e-4, TAU_MAX


def test_detector_mutants_are_rejected(case_a):
    cdet = R.coefficients(ETA, True)[0]
    cnts = [R.cell_mask(m)[1] for m in case_a["mask"]]
    for v in range(2):
        sc, sh = case_a["aff9"][v]
        cm, cnt = R.cell_mask(case_a["mask"][v])
        args = (case_a["y9"][v], sc, sh, case_a["labels"][v], cm)
        r = R.detector_root(*args, cdet, cnt)
        muts = {"dustbin missing from the dot": R.detector_root(*args, cdet, cnt, dustbin_in_dot=False),
                "mask factor missing": R.detector_root(*args, cdet, cnt, use_mask=False),
                "labels not renormalised above 1": R.detector_root(*args, cdet, cnt, renorm_over_one=False),
                "exp(-eta[2]) for exp(-eta[0])": R.detector_root(*args, R.coefficients(ETA, True, swap_det_sem=True)[0], cnt)}
        if v == 1:
            muts["view 1 divided by view 0's count"] = R.detector_root(*args, cdet, cnts[0])
        for name, m in muts.items():
            assert _rejected(m["d"], r["d"], r["d_base"]), (name, v)
            if name in ("labels not renormalised above 1", "view 1 divided by view 0's count"):   # (the others leave the loss value alone)
                assert abs(m["loss"] - r["loss"]) > TAU_MAX * r["loss_base"], (name, v)


def test_segmentation_mutants_are_rejected(case_a):
    csem = R.coefficients(ETA, True)[3]
    cnts = [R.sem_count(s, NC) for s in case_a["sem"]]
    v = 1
    args = (case_a["y13"][v], case_a["sem"][v], NC, csem)
    r = R.sem_root(*args, cnts[v])
    muts = {"align_corners=True": R.sem_root(*args, cnts[v], align_corners=True),
            "ignored pixels counted": R.sem_root(*args, R.sem_count(case_a["sem"][v], NC, count_ignored=True)),
            "view 1 divided by view 0's count": R.sem_root(*args, cnts[0])}
    for name, m in muts.items():
        assert _rejected(m["d"], r["d"], r["d_base"]), name
        assert abs(m["loss"] - r["loss"]) > TAU_MAX * r["loss_base"], name


def _desc_case(case_a, cpos, cneg, **kw):
    unit = [r / r.norm(dim=-1, keepdim=True) for r in (x.double() for x in case_a["raw"])]
    inv = [1.0 / r.double().norm(dim=-1) for r in case_a["raw"]]
    return R.sparse_desc_root(unit[0].float(), unit[1].float(), inv[0], inv[1], *case_a["idx"], cpos, cneg, HC, WC, **kw)


def test_descriptor_mutants_are_rejected(case_a):
    _, cpos, cneg, _ = R.coefficients(ETA, True)
    r = _desc_case(case_a, cpos, cneg)
    assert R.near_tie_fraction(r) <= R.NEAR_TIE_CAP
    muts = {"n_match for nnz + 1": _desc_case(case_a, cpos, cneg, nonmatch_norm="n_match"),
            "margin 0.25": _desc_case(case_a, cpos, cneg, margin_neg=0.25),
            "normalisation backward without d <g, d>": _desc_case(case_a, cpos, cneg, drop_projection=True)}
    for name, m in muts.items():
        for v in range(2):
            assert _rejected(m["root"][v], r["root"][v], r["base"][v], r["allow"][v]), (name, v)
    for name in ("n_match for nnz + 1", "margin 0.25"):
        assert ((muts[name]["neg"] - r["neg"]).abs() > TAU_MAX * r["neg_base"] + r["neg_allow"]).all(), name
    # the uniform sum: lamda_d dropped
    _, upos, uneg, _ = R.coefficients(ETA, False, 0.5, 3.0)
    _, mpos, mneg, _ = R.coefficients(ETA, False, 0.5, 3.0, drop_lamda_d=True)
    assert (upos, uneg, mneg) == (1.5, 0.5, 0.5) and mpos == 0.5
    r, m = _desc_case(case_a, upos, uneg), _desc_case(case_a, mpos, mneg)
    for v in range(2):
        assert _rejected(m["root"][v], r["root"][v], r["base"][v], r["allow"][v]), ("lamda_d dropped", v)
    det, sem = [(1.7, 1.7), (0.9, 0.9)], [(4.1, 4.1), (3.3, 3.3)]
    a, ab, aa, *_ = R.step_scalars(ETA, det, sem, r, False, 0.5, 3.0, True)
    b, *_ = R.step_scalars(ETA, det, sem, r, False, 0.5, 3.0, True, drop_lamda_d=True)
    for k in (0, 3):
        assert abs(a[k] - b[k]) > TAU_MAX * ab[k] + aa[k], R.SCALAR_NAMES[k]
    # "an out-of-range corner given its weight": no valid index can tell (module docstring)
    m = _desc_case(case_a, cpos, cneg, oob_weight=True)
    r = _desc_case(case_a, cpos, cneg)
    assert all(torch.equal(m["root"][v], r["root"][v]) for v in range(2))


def test_scalar_mutants_are_rejected(case_a):
    det, sem = [(1.7, 1.7), (0.9, 0.9)], [(4.1, 4.1), (3.3, 3.3)]
    _, cpos, cneg, _ = R.coefficients(ETA, True)
    desc = _desc_case(case_a, cpos, cneg)
    vals, bases, allow, deta, deta_b, deta_a = R.step_scalars(ETA, det, sem, desc)
    m = R.step_scalars(ETA, det, sem, desc, drop_half_eta1=True)
    assert abs(m[0][0] - vals[0]) > TAU_MAX * bases[0] + allow[0]
    assert abs(m[3][1] - deta[1]) > TAU_MAX * deta_b[1] + deta_a[1]
    m = R.step_scalars(ETA, det, sem, desc, deta2_with_eta0=True)
    assert abs(m[3][2] - deta[2]) > TAU_MAX * deta_b[2] + deta_a[2]


# ---- the near-tie cap -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,hc,wc,n,method,dist", [GPU_GRIDS[0] + v for v in VARIANTS] + [GPU_GRIDS[1] + VARIANTS[0]])
def test_near_tie_cap(nb, hc, wc, n, method, dist):
    """(case B runs ("2d", "cos") only)"""
    da, db = R.unit_descriptors(nb, hc, wc, hc + n)
    ma, mb, nm = R.make_indices(nb, hc, wc, n, N_NON, 41)
    r = R.sparse_desc_root(da, db, None, None, ma, mb, nm, 0.5, 0.5, hc, wc, method, dist)
    assert r["n_terms"] == nb * n * ((1 if dist == "cos" else 0) + N_NON)
    assert R.near_tie_fraction(r) <= R.NEAR_TIE_CAP, (len(r["ties"]), r["n_terms"])
    assert float(r["nnz"].min()) > 0
