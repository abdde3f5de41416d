"""GPU: exact checks of the LOSS PHASE of a training step - the roots the backward pass starts from and the step scalars.

After ONE training step with explicit sparse-loss indices and eta = [0.3, 1.7, -0.6] (distinct values, one negative), the stored
buffers of the step are copied out and every root is recomputed in fp64 by tests/loss_phase_ref.py from the step's OWN inputs to
the loss kernels:

  * dsemi (detector_loss_kernel; cell_mask_kernel feeds its mask and divisor) from the stored raw Y9, scale9 / shift9, the 2-D
    labels and the valid mask; pad channels 65..79 and every element of a masked cell must be exactly 0;
  * dsout (sem_count_kernel + sem_ce_xc_kernel) from the stored Y13 and the int64 labels; pad channels n_classes..sout_cs-1 exactly 0;
  * ddesc (desc_csr / desc_match / desc_nonmatch kernels, det_fold, desc_normalize_bwd_kernel) of both views from the stored
    normalised desc, 1 / norm recomputed from Y11, scale11 / shift11, and the indices;
  * the 11 scalars and grad eta (step_begin_kernel / step_end_kernel) from the per-term values of the above.

Acceptance, element by element: |got - ref| <= TAU[family] * base + near-tie allowance, base = the reference expression on the
absolute values of its terms (scale free), the allowance non-zero only where a hinge of the descriptor loss lies within 2^-20 of
its margin in fp64 (at most 0.1 % of a case's hinge terms, asserted).  The logits are whatever the randomised network produces;
min(1 - p) >= 2^-12 is asserted so that the fp64 softmax is a valid reference (saturation stays covered by the G3 golden).

Cases (the smallest shapes at which each path can still go wrong):
  A          ssmall, B = 3, 64x96 (96 cells per image: a single pass of every grid; B odd, no multiple of 8), 130 matches (more
             than cells), 5 non-matches each, multi-task, ("2d", "cos").  Also here: grad eta accumulated over two steps without
             zero_grad, the validation twin (train=False writes no root - they hold a sentinel - nor gradient, and returns the same scalars),
             and a step whose warped view is fully masked (loss_det_warp and its dsemi exactly 0).
  A-det      A under set_deterministic(True): the det_fold route of ddesc and dsout (families *_det).
  A-scatter  A with SSP_DESC_GATHER=0, in a fresh child process (the switch is read when the engine is created).
  A-uniform  multi_task=False, lambda_loss=0.5, lamda_d=3: grad eta exactly 0, coef_pos = lambda_loss * lamda_d.
  A-variants ("1d", "cos"), ("2d", "euclidean"), ("1d", "euclidean"): descriptor root and the two distance scalars.
  A-bf16     A under conv algorithm 12.  That path keeps the pointwise heads' outputs (Y9, Y11, Y13), the roots and the loss
             kernels in fp32 - only the tensors below the heads are bf16 - so it is one more parametrisation of A with the fp32 taus.
  B          ssmall, B = 16, 120x160 (4800 cells per view, Hc = 15 odd), 300 matches: the grid-stride loops of
             detector_loss_kernel (ncells > 4 * 1024) and cell_mask_kernel (ncells > 4 * 512), several row groups of
             sem_ce_xc_kernel.  Segmentation root on the images [0, 1, B/2, B-1]; its loss and everything else on all images.
  D          the dense descriptor loss (Engine(..., dense_loss=True), dense={"descriptor_dist": 4, "lambda_d": 800}: the reference
             swallows that spelling, lamda_d stays 250), SuperPointNet_gauss2, B = 2, 64x96: the three dense sums, ddesc of both views
             through desc_normalize_bwd_kernel WITHOUT its gather argument, the normaliser B * (mask_cnt[1] + 1) * cells (image 1 of the
             warped view is fully masked).  A cell pair whose centre distance lies within 2^-12 px of descriptor_dist is a near-tie of
             the geometric mask and is allowed either way, like a hinge near its margin (none occurs).
  C          single view (no warped image, lambda_loss = 0), B = 3, 64x96, both architectures: the warped scalars are the constants
             0, grad eta[1] == 0.5 exactly, one pointer set.

The profile hooks of the library time the convolution kernels only, so a case asserts through them which conv path ran (the bf16
kernels under algorithm 12, none of them otherwise) and mirrors the launch predicates of the loss kernels
(min(cdiv(ncells, 4), 1024) / 512 workgroups of 4 waves) for the grid-stride claim of case B; that a loss kernel ran shows in its
output being checked element by element.

TAU: 4 x the worst ratio (|got - fp64| - allowance) / base measured on the MI355X over every case of this module, against the fp64
restatement (never against another run of the kernels); the factor covers the order of the atomics and other devices of the
pool.  tests/test_loss_phase_cpu.py imports TAU_MAX and checks that every mutant of the reference is still rejected there."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import loss_phase_ref as R
from tests.gate_util import _dev
from tests.test_gpu_layer_exact import _inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TAU = {
    "det_root": 4 * 2.62e-7,            # detector_loss_kernel: measured 2.610e-7 (A-det; 2.393e-7 in B, the grid-stride loop)
    "sem_root": 4 * 3.61e-6,            # sem_ce_xc_kernel: measured 3.604e-6 (B, image 0, the cells beside the all-ignored rows).  The
                                        # kernel exponentiates in base 2 on operands (l - m) log2 e of magnitude ~30 here: 2-3 ulp of the
                                        # OPERAND per (pixel, class), which the base (softmax + onehot) does not scale with
    "desc_root_gather": 4 * 3.81e-7,    # desc_match_kernel<.., GATHER> + desc_gather_cell + desc_normalize_bwd_kernel: measured 3.802e-7
                                        # (B; 2.0e-5 before bilin_setup's fractions became explicit fmaf)
    "desc_root_scatter": 4 * 3.57e-7,   # the atomic scatter (SSP_DESC_GATHER=0): measured 3.565e-7
    "desc_root_det": 4 * 5.69e-7,       # set_deterministic(True), det_fold of the 2^-40 fixed-point shadow: measured 5.685e-7
    "sem_root_det": 4 * 3.61e-6,        # dsout through det_fold: measured 3.607e-6
    "dense_root": 4 * 3.54e-7,          # dense_dots_kernel + dense_grad_kernel<false / true> (fp32 MFMA) + desc_normalize_bwd_kernel without the
                                        # gather: measured 3.536e-7 (D)
    "scalars": 4 * 1.01e-6,             # step_end_kernel: measured 1.008e-6 (loss_sem_warp, A; the loss sum of the kernel above)
    "scalars_det": 4 * 9.17e-7,         # the loss sums rounded to the 2^-26 quantum: measured 9.164e-7
}
TAU_MAX = max(TAU.values())
N_CLASSES = 133
SOUT_CS = (N_CLASSES + 3) // 4 * 4


def _cdiv(a, b):
    return -(-a // b)


def _f32(x):
    return float(np.float32(x))


ETA = tuple(_f32(x) for x in R.ETA_TEST)


def _cfg(**kw):
    c = dict(tag="ssp", B=3, H=64, W=96, n_match=130, n_non=5, multi_task=True, lambda_loss=1.0, lamda_d=1.0, method="2d", dist="cos",
             det=False, algo=1, single=False, scatter=False, sem_images=None, mask1_all=False, dense=False)
    c.update(kw)
    return c


def _host_inputs(c):
    """the inputs of the loss kernels that do not come from the network, on the host (fixed seeds)"""
    B, H, W = c["B"], c["H"], c["W"]
    host = {"labels": [R.make_labels(B, H, W, 11), R.make_labels(B, H, W, 12)],
            "mask": [R.make_mask(B, H, W, 21), R.make_mask(B, H, W, 22, full_image=1, all_masked=c["mask1_all"])]}
    if c["tag"] == "ssp":
        host["sem"] = [R.make_sem_labels(B, H, W, N_CLASSES, 31), R.make_sem_labels(B, H, W, N_CLASSES, 32, extra_ignored=True)]
    if c["dense"]:
        host["hom"] = R.make_homographies(B, 51)
    elif not c["single"]:
        host["idx"] = R.make_indices(B, H // 8, W // 8, c["n_match"], c["n_non"], 41)
    return host


def _case_inputs(c):
    """(arch, state dict, device sample, device indices or None, host copies of the loss inputs)"""
    arch, sd, sample = _inputs(c["tag"], c["B"], c["H"], c["W"], flip_gamma=True)
    dev = _dev()
    host = _host_inputs(c)
    sample["labels_2D_gaussian"], sample["warped_labels_gaussian"] = (t.to(dev) for t in host["labels"])
    sample["valid_mask"], sample["warped_valid_mask"] = (t.to(dev) for t in host["mask"])
    if c["tag"] == "ssp":
        sample["semantic"], sample["warped_sem"] = (t.to(dev) for t in host["sem"])
    idx = None
    if c["dense"]:
        sample["homographies"] = host["hom"].to(dev).contiguous()
    elif not c["single"]:
        idx = tuple(t.to(dev).contiguous() for t in host["idx"])
    else:
        sample = {k: v for k, v in sample.items() if not k.startswith("warped") and k not in ("homographies", "inv_homographies",
                                                                                             "cell_homographies")}
    return arch, sd, sample, idx, host


def _engine(c, arch, sd):
    from semantic_superpoint_amd.lib import Engine
    e = Engine(arch, c["B"], c["H"], c["W"], _dev(), n_match=c["n_match"], n_non=c["n_non"], dense_loss=c["dense"])
    if c["algo"] != 1:
        e.set_conv_algo(c["algo"])
    e.load_state_dict(sd)
    e.eta.copy_(torch.tensor(ETA, device=_dev()))
    return e


def _step(c, e, sample, idx, train=True):
    sc = e.pair_step(sample, indices=idx, train=train, lambda_loss=0.0 if c["single"] else c["lambda_loss"], lamda_d=c["lamda_d"],
                     multi_task=c["multi_task"], sparse_method=c["method"], sparse_dist=c["dist"],
                     dense={"descriptor_dist": 4, "lambda_d": 800} if c["dense"] else None)
    torch.cuda.synchronize()
    return sc.cpu().clone()


def _copy_out(c, e, scalars):
    """host copies of the stored buffers of the last step"""
    B, Hc, Wc = c["B"], c["H"] // 8, c["W"] // 8
    d = {"scalars": scalars, "deta": e.grad_dict()["eta"].cpu().clone()}
    for v in range(1 if c["single"] else 2):
        for name, ch in (("Y9", 80), ("dsemi", 80), ("Y11", 256), ("desc", 256), ("ddesc", 256)):
            d["%s_%d" % (name, v)] = e.debug_buffer(v, name, (B, Hc, Wc, ch)).cpu()
        for name, ch in (("scale9", 65), ("shift9", 65), ("scale11", 256), ("shift11", 256)):
            d["%s_%d" % (name, v)] = e.debug_buffer(v, name, (ch,)).cpu()
        if c["tag"] == "ssp":
            for name in ("Y13", "dsout"):
                d["%s_%d" % (name, v)] = e.debug_buffer(v, name, (B, Hc, Wc, SOUT_CS)).cpu()
    return d


class _Worst:
    def __init__(self, tau=None):
        self.w, self.tau = {}, TAU if tau is None else tau

    def note(self, fam, r, where):
        self.w[fam] = max(self.w.get(fam, (0.0, "")), (r, where))
        assert r <= self.tau[fam], (fam, where, r, self.tau[fam])

    def __str__(self):
        return ", ".join("%s %.3e [%s]" % (f, r, where) for f, (r, where) in sorted(self.w.items()))


def _check(c, host, d, worst, parts=("det", "sem", "desc", "scalars")):
    """the stored roots and scalars of one step against the fp64 restatement; parts without "det" / "sem": those roots are not
    compared and of the scalars only loss_desc and the two distances are (the variants of the descriptor loss)"""
    full = "det" in parts and "sem" in parts
    nv = 1 if c["single"] else 2
    semantic = c["tag"] == "ssp"
    use_desc = not c["single"] and c["lambda_loss"] > 0
    Hc, Wc = c["H"] // 8, c["W"] // 8
    sfx = "_det" if c["det"] else ""
    cdet, cpos, cneg, csem = R.coefficients(ETA, c["multi_task"], c["lambda_loss"], c["lamda_d"])
    det, sem, desc = [(0.0, 0.0), (0.0, 0.0)], [(0.0, 0.0), (0.0, 0.0)], None
    for v in range(nv):
        cm, cnt = R.cell_mask(host["mask"][v])
        r = R.detector_root(d["Y9_%d" % v], d["scale9_%d" % v], d["shift9_%d" % v], host["labels"][v], cm, cdet, cnt)
        det[v] = (r["loss"], r["loss_base"])
        if "det" in parts:
            assert float((1.0 - r["p"]).min()) >= 2.0 ** -12, ("saturated softmax", v, float((1.0 - r["p"]).min()))
            ds = d["dsemi_%d" % v]
            assert not ds[..., 65:].any(), ("dsemi pad channels", v)
            assert not ds[cm == 0].any(), ("dsemi of masked cells", v)
            assert float(cm.sum()) == 0 or ds[cm == 1].any()
            q, i = R.ratio(ds[..., :65], r["d"], r["d_base"])
            worst.note("det_root", q, "dsemi view %d %s" % (v, np.unravel_index(i, r["d"].shape)))
        if semantic:
            cnt_s = R.sem_count(host["sem"][v], N_CLASSES)
            imgs = c["sem_images"] if "sem" in parts else []
            s = R.sem_root(d["Y13_%d" % v], host["sem"][v], N_CLASSES, csem, cnt_s, imgs)
            sem[v] = (s["loss"], s["loss_base"])
            if "sem" in parts:
                so = d["dsout_%d" % v]
                assert not so[..., N_CLASSES:].any(), ("dsout pad channels", v)
                sel = so if imgs is None else so[imgs]
                q, i = R.ratio(sel[..., :N_CLASSES], s["d"], s["d_base"])
                worst.note("sem_root" + sfx, q, "dsout view %d %s" % (v, np.unravel_index(i, s["d"].shape)))
    if use_desc:
        inv = [R.inv_norm_ref(d["Y11_%d" % v], d["scale11_%d" % v], d["shift11_%d" % v]) for v in range(2)]
        flat = lambda t: t.reshape(c["B"], Hc * Wc, 256)   # noqa: E731
    if use_desc and c["dense"]:
        valid = R.cell_mask(host["mask"][1])[0].reshape(c["B"], Hc * Wc)
        desc = R.dense_desc_root(flat(d["desc_0"]), flat(d["desc_1"]), inv[0], inv[1], host["hom"], valid, cneg, c["multi_task"], Hc, Wc,
                                 lamda_d=250.0, descriptor_dist=4.0)
        assert len(desc["ties"]) <= R.NEAR_TIE_CAP * desc["n_terms"], ("near-ties", len(desc["ties"]), desc["n_terms"])
        assert 0 < float(desc["mask"].sum()) and 0 < float(valid.sum()) < valid.numel()
        for v in range(2):
            got = flat(d["ddesc_%d" % v])
            assert got.any()
            q, i = R.ratio(got, desc["root"][v], desc["base"][v], desc["allow"][v])
            worst.note("dense_root", q, "ddesc view %d %s (%d near-ties)" % (v, np.unravel_index(i, got.shape), len(desc["ties"])))
    elif use_desc:
        desc = R.sparse_desc_root(flat(d["desc_0"]), flat(d["desc_1"]), inv[0], inv[1], *host["idx"], cpos, cneg, Hc, Wc, c["method"],
                                  c["dist"])
        frac = R.near_tie_fraction(desc)
        assert frac <= R.NEAR_TIE_CAP, ("near-ties", len(desc["ties"]), desc["n_terms"])
        if "desc" in parts:
            fam = "desc_root_det" if c["det"] else "desc_root_scatter" if c["scatter"] else "desc_root_gather"
            for v in range(2):
                got = flat(d["ddesc_%d" % v])
                assert got.any()
                q, i = R.ratio(got, desc["root"][v], desc["base"][v], desc["allow"][v])
                worst.note(fam, q, "ddesc view %d %s (%d near-ties)" % (v, np.unravel_index(i, got.shape), len(desc["ties"])))
    vals, bases, allow, deta, deta_b, deta_a = R.step_scalars(ETA, det, sem, desc, c["multi_task"], c["lambda_loss"] if use_desc else 0.0,
                                                              c["lamda_d"], semantic)
    if "scalars" in parts:
        got = d["scalars"].double()
        for k, name in enumerate(R.SCALAR_NAMES):
            if k >= 8:
                assert float(got[k]) == ETA[k - 8], (name, float(got[k]))
            elif full or name in ("loss_desc", "positive_dist", "negative_dist"):
                q, _ = R.ratio(got[k:k + 1], torch.tensor([vals[k]]), torch.tensor([bases[k]]), torch.tensor([allow[k]]))
                worst.note("scalars" + sfx, q, name)
        if full:
            q, i = R.ratio(d["deta"], torch.tensor(deta), torch.tensor(deta_b), torch.tensor(deta_a))
            worst.note("scalars" + sfx, q, "grad eta[%d]" % i)
    return {"vals": vals, "bases": bases, "allow": allow, "deta": deta, "deta_base": deta_b, "deta_allow": deta_a, "det": det}


def _conv_kernels(c, e, sample, idx):
    """names of the profiled convolution kernels one more step of the case launches"""
    e.zero_grad()
    e.profile_enable("conv3x3_every")
    _step(c, e, sample, idx)
    k = e.profile_read_kernels()
    e.profile_enable("none")
    return {n for n, v in k.items() if v["launches"] > 0}


def _run(c, extra=None, parts=("det", "sem", "desc", "scalars")):
    torch.set_num_threads(min(int(os.environ.get("OMP_NUM_THREADS", "16")), 16))
    from semantic_superpoint_amd import lib as L
    t0 = time.perf_counter()
    worst = _Worst()
    L.set_deterministic(c["det"])
    try:
        arch, sd, sample, idx, host = _case_inputs(c)
        e = _engine(c, arch, sd)
        e.zero_grad()
        sc = _step(c, e, sample, idx)
        d = _copy_out(c, e, sc)
        ref = _check(c, host, d, worst, parts)
        if extra is not None:
            extra(c, e, sample, idx, host, d, ref, worst)
        kern = _conv_kernels(c, e, sample, idx)
        bf16 = {k for k in kern if "bf16" in k}
        assert (bf16 == {"conv_bf16_kernel", "wgrad_bf16_kernel"}) if c["algo"] == 12 else not bf16, kern
    finally:
        L.set_deterministic(False)
    print("loss phase %s: worst (|got - fp64| - allowance) / base per family: %s (%.1f s)" % (
        {k: v for k, v in c.items() if _cfg()[k] != v}, worst, time.perf_counter() - t0))
    return worst


SENTINEL = -12345.5


def _root_view(e, slot, name, numel):
    """a VIEW (no copy) of an internal fp32 buffer inside the engine's workspace: the pointer arithmetic of Engine.debug_buffer"""
    import ctypes as C
    p, n = C.c_void_p(), C.c_size_t()
    assert e.lib.ssp_debug_buffer(e.h, slot, name.encode(), C.byref(p), C.byref(n)) == 0
    off = p.value - e.workspace.data_ptr()
    assert 0 <= off and off + numel * 4 <= e.ws_bytes
    return e.workspace[off:off + numel * 4].view(torch.float32)


def _case_a_extras(c, e, sample, idx, host, d, ref, worst):
    # grad eta accumulates: a second step without zero_grad
    sc2 = _step(c, e, sample, idx)
    deta2 = e.grad_dict()["eta"].cpu().double()
    for k in range(3):
        err = abs(float(deta2[k]) - 2.0 * ref["deta"][k])
        base = 2.0 * ref["deta_base"][k]
        worst.note("scalars", max(err - 2.0 * ref["deta_allow"][k], 0.0) / base, "grad eta[%d] over two steps" % k)
    assert torch.allclose(sc2, d["scalars"], rtol=1e-5, atol=0)   # (the same step again: the order of the atomics at the most)
    # the validation twin: roots and gradients untouched, the same scalars
    # (dsemi and dsout are deterministic per element: a validation step that wrongly rewrote them would write the same bits.  The
    # root buffers are therefore filled with a sentinel first; any write shows.)
    names = [("dsemi", 80), ("ddesc", 256), ("dsout", SOUT_CS)]
    ncell = c["B"] * (c["H"] // 8) * (c["W"] // 8)
    views = [_root_view(e, v, n, ncell * ch) for v in range(2) for n, ch in names]
    for t in views:
        t.fill_(SENTINEL)
    grads = e.grads.clone()
    scv = _step(c, e, sample, idx, train=False)
    for t in views:
        assert bool((t == SENTINEL).all()), "train=False wrote a root"
    assert torch.equal(grads, e.grads), "train=False changed the gradients"
    for k, name in enumerate(R.SCALAR_NAMES[:8]):
        q, _ = R.ratio(scv[k:k + 1], torch.tensor([ref["vals"][k]]), torch.tensor([ref["bases"][k]]), torch.tensor([ref["allow"][k]]))
        worst.note("scalars", q, "validation " + name)
    assert torch.equal(scv[8:], d["scalars"][8:])


def test_case_a_every_root_and_scalar():
    _run(_cfg(), _case_a_extras)


def test_case_a_warped_view_fully_masked():
    """mask_cnt[1] == 0: loss_det_warp and dsemi of view 1 are exactly 0 (0 / 1e-5, coefficient times mask 0)"""
    c = _cfg(mask1_all=True)

    def extra(c, e, sample, idx, host, d, ref, worst):
        assert float(d["scalars"][2]) == 0.0
        assert not d["dsemi_1"].any()
        assert d["dsemi_0"].any()
    _run(c, extra)


def test_case_a_deterministic():
    _run(_cfg(det=True))


def test_case_a_bf16_path():
    _run(_cfg(algo=12))


def test_case_a_uniform_sum():
    def extra(c, e, sample, idx, host, d, ref, worst):
        assert not d["deta"].any(), d["deta"]
    _run(_cfg(multi_task=False, lambda_loss=0.5, lamda_d=3.0), extra)


@pytest.mark.parametrize("method,dist", [("1d", "cos"), ("2d", "euclidean"), ("1d", "euclidean")])
def test_case_a_descriptor_variants(method, dist):
    """descriptor root and the two distance scalars of the other (method, dist) pairs"""
    _run(_cfg(method=method, dist=dist), parts=("desc", "scalars"))


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from tests import test_gpu_loss_exact as T
c = T._cfg(scatter=True)
arch, sd, sample, idx, host = T._case_inputs(c)
e = T._engine(c, arch, sd)
e.zero_grad()
d = T._copy_out(c, e, T._step(c, e, sample, idx))
d["ws_bytes"] = torch.tensor(e.ws_bytes)
torch.save(d, sys.argv[2])
"""


def test_case_a_scatter_in_a_fresh_process(tmp_path):
    """SSP_DESC_GATHER=0 is read when the engine is created: the step runs in a child process, the parent checks what it stored.
    No hook names the loss kernels that ran (the profile buckets hold convolution kernels only).  What shows that the child's engine
    read the switch: without the gather it does not carve the corner lists and the gradient rows (csr_off / csr_match / csr_weight /
    g_rows) out of its workspace, so its workspace is smaller than that of an engine of the same configuration made here."""
    out = str(tmp_path / "scatter.pt")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=dict(os.environ, SSP_DESC_GATHER="0"), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = torch.load(out)
    c = _cfg(scatter=True)
    arch, sd, _, _, _ = _case_inputs(c)
    assert os.environ.get("SSP_DESC_GATHER", "1") != "0", "the parent must run the default (gather) path"
    rows = c["B"] * c["n_match"] * 2 * 256 * 4   # g_rows alone
    assert int(d.pop("ws_bytes")) <= _engine(c, arch, sd).ws_bytes - rows, "the child's engine did not take the scatter route"
    worst = _Worst()
    _check(c, _host_inputs(c), d, worst)
    print("loss phase, scatter: %s" % worst)


def test_case_b_grid_stride_loops():
    c = _cfg(B=16, H=120, W=160, n_match=300, sem_images=[0, 1, 8, 15])
    ncells = c["B"] * (c["H"] // 8) * (c["W"] // 8)
    # mirrors of the launches in pair_step_impl: 4 waves (cells) per workgroup
    assert ncells > 4 * min(_cdiv(ncells, 4), 1024), "detector_loss_kernel would not loop"
    assert ncells > 4 * min(_cdiv(ncells, 4), 512), "cell_mask_kernel would not loop"
    _run(c)


def test_case_d_dense_loss():
    _run(_cfg(tag="sp", B=2, dense=True))


@pytest.mark.parametrize("tag", ["ssp", "sp"])
def test_case_c_single_view(tag):
    def extra(c, e, sample, idx, host, d, ref, worst):
        sc = d["scalars"]
        for k in (2, 3, 5, 6, 7):   # loss_det_warp, loss_desc, loss_sem_warp, positive_dist, negative_dist: the constants 0
            assert float(sc[k]) == 0.0, (R.SCALAR_NAMES[k], float(sc[k]))
        assert float(d["deta"][1]) == 0.5
        if c["tag"] == "sp":
            assert float(d["deta"][2]) == 0.0 and float(sc[4]) == 0.0
    _run(_cfg(tag=tag, single=True, lambda_loss=0.0), extra)
