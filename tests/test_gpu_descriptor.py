"""GPU: the descriptor export (export.py:66-190) against the real reference (G15 fixtures, tools/make_golden_descriptor.py).

  1. sparse-descriptor sampling, teacher-forced on the reference's coarse descriptor and integer points
  2. two-way matching on the stored cases (indices exact away from BLAS-order ties, duplicates take the first index)
  3. keypoints, teacher-forced on the reference's heatmaps
  4. end to end through the drop-in names (Val_model_heatmap + PointTracker) with the fixture's weights
  5. a batched DescriptorExporter flush equals single-pair calls; export_descriptor writes the reference's npz layout
  6. refusals: error codes / exceptions instead of faults
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cpu_ref as CR
from tests import golden_util as G
from tests.golden_descriptor import MATCH_CASES, ambiguous_rows, descriptor_case_images, match_case_inputs

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _score_close(a, b):
    """|a - b| <= 1e-6, or the squared distances 2 - 2 dot within 2e-6: near d = 0 the square root amplifies the last
    bit of the fp32 dot product (dot = 1 - 6e-8 gives d = 3.5e-4), which neither summation order decides."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.abs(a - b) <= 1e-6) | (np.abs(a * a - b * b) <= 2e-6)


def _weights_file(tmp_path, arch, seed):
    sd = CR.init_state_dict(arch, seed=seed)
    path = str(tmp_path / "weights.pth")
    torch.save({k: torch.as_tensor(np.array(v)) for k, v in sd.items()}, path)
    return path


def test_sample_descriptors_teacher_forced():
    """The reference's coarse descriptor of the image at its integer points (the fixture keeps the descriptors of the
    `desc_rows` most confident points)."""
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    g = G.load("g15_descriptor_ssp_120x160.npz")
    desc = torch.from_numpy(g["coarse_desc"]).to(dev)
    pts = g["pts_int"]
    n, k = pts.shape[0], g["desc"].shape[0]
    cap = n + 5  # rows past the count stay unread
    xy = torch.zeros(1, cap, 2, dtype=torch.float32)
    xy[0, :n] = torch.from_numpy(pts[:, :2].astype(np.float32))
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    out = L.op_sample_descriptors(desc, xy.to(dev), cnt)
    torch.cuda.synchronize()
    got = out[0, :n].cpu().numpy()
    assert np.abs(got[:k] - g["desc"]).max() < 2e-6
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_sample_descriptors_batch_samples_own_map():
    """The extension: image b of a batch samples its own descriptor map (the reference's grid has batch 1).  Map 1 is the
    negated map 0 at other points: sampling is linear and the norm is even, so its rows are the negated reference rows."""
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    g = G.load("g15_descriptor_ssp_120x160.npz")
    desc = torch.from_numpy(np.concatenate([g["coarse_desc"], -g["coarse_desc"]])).to(dev)
    k = g["desc"].shape[0]
    n0, n1 = g["pts_int"].shape[0], k // 2
    sel = np.arange(k)[::-1][:n1]  # a different subset and order of points for image 1
    cap = max(n0, n1)
    xy = torch.zeros(2, cap, 2, dtype=torch.float32)
    xy[0, :n0] = torch.from_numpy(g["pts_int"][:, :2].astype(np.float32))
    xy[1, :n1] = torch.from_numpy(g["pts_int"][sel, :2].astype(np.float32))
    out = L.op_sample_descriptors(desc, xy.to(dev), torch.tensor([n0, n1], dtype=torch.int32, device=dev)).cpu().numpy()
    assert np.abs(out[0, :k] - g["desc"]).max() < 2e-6
    assert np.abs(out[1, :n1] + g["desc"][sel]).max() < 2e-6


def _device_match(d1, d2, thr, dev):
    from semantic_superpoint_amd import lib as L
    n1, n2 = d1.shape[1], d2.shape[1]
    cap = max(n1, n2, 1)
    a = torch.zeros(1, cap, 256)
    b = torch.zeros(1, cap, 256)
    a[0, :n1] = torch.from_numpy(d1.T.copy())
    b[0, :n2] = torch.from_numpy(d2.T.copy())
    i32 = dict(dtype=torch.int32, device=dev)
    m, nm = L.op_match_two_way(a.to(dev), torch.tensor([n1], **i32), b.to(dev), torch.tensor([n2], **i32), thr)
    k = int(nm.item())
    return m[0, :k].cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("case", [c[0] for c in MATCH_CASES])
def test_match_two_way_golden_cases(case):
    dev = _dev()
    name, seed, n1, n2, thr = next(c for c in MATCH_CASES if c[0] == case)
    ref = G.load("g15_match_cases.npz")[name + "/matches"]
    d1, d2 = match_case_inputs(name, seed, n1, n2)
    got = _device_match(d1, d2, thr, dev)
    if n1 == 0 or n2 == 0:
        assert got.shape[0] == 0 and ref.shape[0] == 0
        return
    assert np.all(np.diff(got[:, 0]) > 0), "rows ascending"
    amb = ambiguous_rows(d1, d2, thr)
    ours = {int(r[0]): r for r in got if not amb[int(r[0])]}
    theirs = {int(r[0]): r for r in ref if not amb[int(r[0])]}
    assert amb.mean() < 0.02, "too many ambiguous rows for a meaningful comparison"
    assert set(ours) == set(theirs)
    for i, r in theirs.items():
        assert int(ours[i][1]) == int(r[1]), (i, ours[i], r)
        assert _score_close(ours[i][2], r[2]), (i, ours[i], r)
    if name == "dup":  # later copies of duplicated columns never win; duplicated rows match only through their first copy
        assert not np.isin(got[:, 1], [17, 40, 9, 61]).any()
        assert not np.isin(got[:, 0], [100, 8, 250]).any()
        np.testing.assert_array_equal(got[:, :2], ref[:, :2])


def test_points_teacher_forced():
    """The NMS / border / sort kernels the batched extraction launches, on the reference's own heatmaps."""
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    g = G.load("g15_descriptor_ssp_120x160.npz")
    for tag in ("", "warped_"):
        hm = torch.from_numpy(g[tag + "heatmap"]).to(dev)
        pi = L.op_heatmap_points(hm, float(g["conf_thresh"]), 4, 4, 0, False)
        np.testing.assert_array_equal(pi, g[tag + "pts_int"])
        ps = L.op_heatmap_points(hm, float(g["conf_thresh"]), 4, 4, 0, True)
        assert np.abs(ps - g[tag + "pts"]).max() < 1e-5


def _get_module(path, name):
    """utils/loader.py:157-164 of the reference."""
    mod = importlib.import_module(name) if path == "" else importlib.import_module("{}.{}".format(path, name))
    return getattr(mod, name)


def test_end_to_end_dropin_names(tmp_path):
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    g = G.load("g15_descriptor_ssp_120x160.npz")
    # the host repository's stub: a top-level module of the front end's name
    (tmp_path / "Val_model_heatmap.py").write_text(
        "from semantic_superpoint_amd.Val_model_heatmap import Val_model_heatmap  # noqa: F401\n")
    sys.path.insert(0, str(tmp_path))
    try:
        sys.modules.pop("Val_model_heatmap", None)
        config = {"front_end_model": "Val_model_heatmap",
                  "model": {"name": str(g["arch"]), "params": {}, "pretrained": _weights_file(tmp_path, str(g["arch"]), int(g["seed"])),
                            "nms": int(g["nms"]), "detection_threshold": float(g["conf_thresh"]),
                            "nn_thresh": float(g["nn_thresh"])}}
        Val_model_heatmap = _get_module("", config["front_end_model"])
        agent = Val_model_heatmap(config["model"], device=dev)
        agent.loadModel()
    finally:
        sys.path.remove(str(tmp_path))
        sys.modules.pop("Val_model_heatmap", None)
    tracker = PointTracker(max_length=2, nn_thresh=agent.nn_thresh)
    ints = {}
    img, warped, _ = descriptor_case_images(int(g["seed"]))
    for tag, im in (("", img), ("warped_", warped)):
        heat = agent.run(torch.from_numpy(im)[None, None].to(dev))   # export.py:126-142
        assert heat.shape == (1, 1, 120, 160)
        pts = agent.heatmap_to_pts()
        pts_int = pts[0].T.copy()
        pts = agent.soft_argmax_points(pts, patch_size=5)
        desc = agent.desc_to_sparseDesc()
        assert desc[0].dtype == np.float32 and desc[0].shape == (256, pts_int.shape[0])
        tracker.update(pts[0], desc[0])
        ref_int = g[tag + "pts_int"]
        key_of = lambda a: [(int(x), int(y)) for x, y in a[:, :2]]  # noqa: E731
        ours = {k: r for r, k in enumerate(key_of(pts_int))}
        theirs = {k: r for r, k in enumerate(key_of(ref_int))}
        common = [k for k in theirs if k in ours]
        assert len(common) >= 0.99 * len(theirs), (len(common), len(theirs))
        io, ir = [ours[k] for k in common], [theirs[k] for k in common]
        kd = g[tag + "desc"].shape[0]  # reference descriptors kept for the kd most confident points
        dsel = [(a, b) for a, b in zip(io, ir) if b < kd]
        assert len(dsel) >= 0.99 * kd
        assert np.abs(desc[0].T[[a for a, _ in dsel]] - g[tag + "desc"][[b for _, b in dsel]]).max() < 1e-4
        assert np.abs(pts[0].T[io, :2] - g[tag + "pts"][ir, :2]).max() < 1e-3
        ints[tag] = (pts_int, ref_int, set(common))
    m = tracker.get_matches()
    assert m.shape[0] == 4
    ms = tracker.get_mscores()
    (o0, r0, c0), (o1, r1, c1) = ints[""], ints["warped_"]

    def pairs(sc, p0, p1):
        out = set()
        for i, j in sc[:, :2].astype(int) if sc.ndim == 2 and sc.shape[1] else []:
            a, b = (int(p0[i, 0]), int(p0[i, 1])), (int(p1[j, 0]), int(p1[j, 1]))
            if a in c0 and b in c1:
                out.add((a, b))
        return out

    mo = pairs(ms.T, o0, o1)
    mr = pairs(g["mscores"], r0, r1)
    assert len(mr) > 20
    assert len(mo & mr) >= 0.99 * len(mo | mr), (len(mo & mr), len(mo), len(mr))


def _pairs_240x320(P, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(P):
        a = rs.uniform(0, 1, (1, 240, 320)).astype(np.float32)
        b = np.roll(a, (2, 3), axis=(1, 2)).copy()
        b[:, :2] = rs.uniform(0, 1, (1, 2, 320))
        out.append((torch.from_numpy(a), torch.from_numpy(b)))
    return out


def test_batched_equals_single_and_export_descriptor(tmp_path):
    from semantic_superpoint_amd import models
    from semantic_superpoint_amd.export import DescriptorExporter, export_descriptor
    dev = _dev()
    arch = "SuperPointNet_gauss2_ssmall"
    net = getattr(models, arch)()
    net.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in CR.init_state_dict(arch, seed=21).items()})
    net = net.to(dev).eval()
    ex = DescriptorExporter(net, dev, conf_thresh=0.0155, nms_dist=4, subpixel=True, nn_thresh=0.7, batch_pairs=8)
    pairs = _pairs_240x320(8, 5)
    batched = ex([(a.to(dev), b.to(dev)) for a, b in pairs])
    n_matches = 0
    for p, (a, b) in enumerate(pairs):
        single = ex([(a.to(dev), b.to(dev))])[0]
        for k in ("prob", "warped_prob", "matches"):
            np.testing.assert_array_equal(batched[p][k], single[k], err_msg="%s of pair %d" % (k, p))
        for k in ("desc", "warped_desc"):
            assert np.abs(batched[p][k] - single[k]).max() <= 1e-6
        assert batched[p]["prob"].shape[0] > 50
        n_matches += batched[p]["matches"].shape[0]
    assert n_matches > 0

    class Loader:
        def __iter__(self):
            for a, b in pairs[:3]:
                yield {"image": a[None], "warped_image": b[None], "homography": torch.eye(3)[None]}

    config = {"data": {"dataset": "in-memory"},
              "model": {"name": arch, "params": {}, "pretrained": _weights_file(tmp_path, arch, 21), "nms": 4,
                        "detection_threshold": 0.0155, "nn_thresh": 0.7, "subpixel": {"enable": True, "patch_size": 5}}}
    out = tmp_path / "export"
    assert export_descriptor(config, str(out), None, test_loader=Loader(), pairs_per_flush=8) == 3
    assert (out / "config.yml").exists()
    for i in range(3):
        d = dict(np.load(out / "predictions" / ("%d.npz" % i)))
        assert set(d) == {"image", "warped_image", "prob", "warped_prob", "desc", "warped_desc", "homography", "matches"}
        assert d["image"].shape == (240, 320) and d["warped_image"].shape == (240, 320)
        for t in ("", "warped_"):
            assert d[t + "prob"].dtype == np.float64 and d[t + "prob"].shape[1] == 3
            assert d[t + "desc"].dtype == np.float32 and d[t + "desc"].shape == (d[t + "prob"].shape[0], 256)
        assert d["homography"].shape == (3, 3)
        m = d["matches"]
        assert m.dtype == np.float64 and m.shape[1] == 4
        np.testing.assert_array_equal(d["prob"], batched[i]["prob"])
        np.testing.assert_array_equal(m, batched[i]["matches"])
        rows0 = {tuple(r) for r in d["prob"][:, :2]}
        rows1 = {tuple(r) for r in d["warped_prob"][:, :2]}
        assert all(tuple(r) in rows0 for r in m[:, :2]) and all(tuple(r) in rows1 for r in m[:, 2:])


def test_refusals():
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.export import DescriptorExporter, PointTracker
    dev = _dev()
    with pytest.raises(ValueError):
        DescriptorExporter(None, dev, 0.015, 4, True, -0.5)
    d = torch.nn.functional.normalize(torch.randn(1, 8, 256, device=dev), dim=2)
    c = torch.tensor([8], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        L.op_match_two_way(d, c, d, c, -0.1)
    with pytest.raises(ValueError):
        PointTracker(2, 0.7).nn_match_two_way(np.eye(256, 4, dtype=np.float32), np.eye(256, 4, dtype=np.float32), -1.0)
    lib = L.load_library()
    st = L._stream()
    # a slot without a forward
    eng = L.Engine("SuperPointNet_gauss2_ssmall", 2, 64, 96, dev, with_grad=False)
    with pytest.raises(RuntimeError):
        eng.describe_points(1, 1)
    p = L.SspExportParams(1, 64, 96, 0.015, 4, 4, 0, 1)
    ws = torch.empty(lib.ssp_describe_workspace_bytes(C.byref(p), 2), dtype=torch.uint8, device=dev)
    cap = lib.ssp_export_max_points(C.byref(p))
    pts = torch.empty(2, cap, 5, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    desc = torch.empty(2, cap, 256, device=dev)
    args = lambda q, n: (eng.h, 0, C.byref(q), n, L._ptr(ws), L._ptr(pts), L._ptr(cnt), L._ptr(desc), st)  # noqa: E731
    assert lib.ssp_describe_points(*args(p, 1)) != 0   # slot 0 holds no forward yet either
    x = torch.rand(2, 1, 64, 96, device=dev)
    eng.forward(x, slot=0, train=False, want=())
    bad = L.SspExportParams(1, 60, 96, 0.015, 4, 4, 0, 1)   # height not a multiple of 8
    assert lib.ssp_describe_workspace_bytes(C.byref(bad), 1) == 0
    assert lib.ssp_describe_points(*args(bad, 1)) != 0
    assert lib.ssp_describe_points(*args(p, 3)) != 0         # more images than the slot's forward
    # the matcher's point cap
    assert lib.ssp_match_workspace_bytes(L.MATCH_MAX_POINTS + 1, 1) == 0
    big = L.MATCH_MAX_POINTS + 1
    assert lib.ssp_match_two_way(L._ptr(d), L._ptr(c), L._ptr(d), L._ptr(c), big, 1, 1, C.c_float(0.7), L._ptr(ws),
                                 L._ptr(desc), L._ptr(cnt), st) != 0
    # and the handle still works
    assert lib.ssp_describe_points(*args(p, 2)) == 0
    torch.cuda.synchronize()
    assert (cnt.cpu() >= 0).all() and (cnt.cpu() <= cap).all()
