"""The epipolar check on the device: ssp_epi_ransac against its numpy restatement
(tests/epipolar_ref.py) and against the truth of synthetic two-view scenes, its independence of groups / batch / repetition,
ssp_op_filter_matches against torch boolean indexing, and the geometric check of PointTracker / SequenceTracker.

Tolerance of F and err (E.TOLERANCE = 2.94e-11): measured, not chosen.  The restatement's refit was evaluated with two
summation orders (ascending and pairwise) on the compared fixtures below; the largest difference of any entry of F or of err
was 1.837e-12 (the err of the 8-match fixture) and the tolerance is 16 times that.  tests/test_epipolar_cpu.py repeats the
measurement.  mask, n_inliers, status and winner are compared for equality.  The planar fixture has no F to compare: every one
of its 2000 systems has rank 6 and is refused by the pivot rule (largest smallest-pivot 5.2e-16 against 1e-12), so the answer
is status 1 (tests/test_epipolar_exact_cpu.py prints the margin).  tests/test_gpu_epipolar_exact.py holds the same kernels
to the restatement in their own summation order, where F and err agree to the last bit."""
import functools

import numpy as np
import pytest
import torch

from tests import epipolar_ref as E

pytestmark = pytest.mark.gpu

KEYS = ("F", "mask", "n_inliers", "status", "winner", "err")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _arrays(names, cap, pair_stride, pt_stride):
    """Host inputs of one call over the named fixtures (pair p at entry p * pair_stride; the other entries hold noise)."""
    P = len(names)
    rng = np.random.RandomState(cap + 7 * pair_stride + 13 * pt_stride)
    pts1 = rng.uniform(0, 300, (P * pair_stride, cap, pt_stride))
    pts2 = rng.uniform(0, 300, (P * pair_stride, cap, pt_stride))
    match = np.zeros((P, cap, 3), dtype=np.float32)
    n_match = np.zeros(P, dtype=np.int32)
    seeds = np.zeros(P, dtype=np.int64)
    for p, nm in enumerate(names):
        c = E.case(nm)
        a, b, m = E.as_arrays(c["m"], cap, pt_stride, rng)
        pts1[p * pair_stride], pts2[p * pair_stride], match[p] = a, b, m
        n_match[p], seeds[p] = c["m"].shape[0], c["seed"]
        assert np.array_equal(E.gather(a, b, m, n_match[p]), c["m"])
    return pts1, pts2, match, n_match, seeds


def _run(names, cap, pair_stride=1, pt_stride=2, groups=0, pairs=None):
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    pts1, pts2, match, n_match, seeds = _arrays(tuple(names), cap, pair_stride, pt_stride)
    if pairs is not None:   # a call over a slice of the pairs
        sl = slice(pairs * pair_stride, (pairs + 1) * pair_stride)
        pts1, pts2, match, n_match, seeds = pts1[sl], pts2[sl], match[pairs:pairs + 1], n_match[pairs:pairs + 1], seeds[pairs:pairs + 1]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    o = L.op_epipolar_ransac(t(pts1), t(pts2), t(match), t(n_match), t(seeds), thresh=1.0, pair_stride=pair_stride, groups=groups)
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in KEYS}


def _sampson(F, m):
    d2, usable = E.sampson2(np.asarray(F, dtype=np.float64).reshape(1, 9), m)
    return np.sqrt(np.where(usable[0], d2[0], np.inf))


def _compare(o, p, name):
    c = E.case(name)
    ref, n = c["ref"], c["m"].shape[0]
    got = {k: o[k][p] for k in KEYS}
    dF = float(np.abs(got["F"] - ref["F"]).max())
    derr = abs(float(got["err"]) - ref["err"])
    print("%s: status %d winner %d inliers %d |dF| %.3e |derr| %.3e (tolerance %.3e)"
          % (name, got["status"], got["winner"], got["n_inliers"], dF, derr, E.TOLERANCE))
    assert got["status"] == ref["status"] and got["winner"] == ref["winner"] and got["n_inliers"] == ref["n_inliers"], name
    assert np.array_equal(got["mask"][:n].astype(bool), ref["mask"]) and not got["mask"][n:].any(), name
    if ref["status"] == 1:
        assert not got["F"].any() and got["err"] == 0.0 and got["winner"] == -1
        return
    if name in E.F_COMPARED:
        assert dF <= E.TOLERANCE and derr <= E.TOLERANCE, (name, dF, derr)
    if name in E.NOISE_FREE:
        assert np.array_equal(got["mask"][:n].astype(bool), c["truth"])
        worst, det = float(_sampson(got["F"], c["m"][c["truth"]]).max()), abs(float(np.linalg.det(got["F"])))
        print("%s: worst true inlier %.3e px, |det F| %.3e" % (name, worst, det))
        assert worst < E.TOLERANCE and det < E.TOLERANCE, (name, worst, det)


FOUR = ("mixed48", "eight", "five", "empty")   # n_match = (48, 8, 5, 0)


@pytest.mark.parametrize("pair_stride,pt_stride", ((1, 2), (1, 3), (2, 2), (2, 3)))
def test_four_pairs_in_one_call(pair_stride, pt_stride):
    assert [E.case(nm)["m"].shape[0] for nm in FOUR] == [48, 8, 5, 0]
    o = _run(FOUR, 64, pair_stride, pt_stride)
    for p, nm in enumerate(FOUR):
        _compare(o, p, nm)


@pytest.mark.parametrize("name,cap", (("n257", 320), ("n4096", 4096), ("noisy", 256), ("planar", 64)))
def test_one_pair(name, cap):
    assert E.case(name)["m"].shape[0] == {"n257": 257, "n4096": 4096, "noisy": 250, "planar": 48}[name]
    _compare(_run((name,), cap, 1, 3), 0, name)


def _same(a, b, pa=slice(None), pb=slice(None)):
    for k in KEYS:
        assert np.array_equal(a[k][pa].view(np.uint8), b[k][pb].view(np.uint8)), k   # bit for bit


def test_result_does_not_depend_on_groups_batch_or_run():
    base = _run(FOUR, 64, 2, 3, groups=0)
    for g in (1, 3, 16):
        _same(base, _run(FOUR, 64, 2, 3, groups=g))
    _same(base, _run(FOUR, 64, 2, 3, groups=0))               # a repeated call
    for p in range(4):                                        # 4 pairs in one call = 4 single calls
        _same(base, _run(FOUR, 64, 2, 3, pairs=p), slice(p, p + 1))
    one = _run(("n257",), 320, 1, 3, groups=0)
    for g in (1, 3, 16):
        _same(one, _run(("n257",), 320, 1, 3, groups=g))


def test_bad_arguments_are_errors():
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    pts = torch.zeros(1, 16, 2, dtype=torch.float64, device=dev)
    m = torch.zeros(1, 16, 3, device=dev)
    nm = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.zeros(1, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError):
        L.op_epipolar_ransac(pts, pts, m, nm, s, groups=65)
    with pytest.raises(RuntimeError):
        L.op_epipolar_ransac(pts, pts, m, nm, s, thresh=-1.0)
    one = torch.zeros(1, 16, 1, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        L.op_epipolar_ransac(one, one, m, nm, s)


# ---- ssp_op_filter_matches ----------------------------------------------------------------------------------------------
def test_filter_matches_against_boolean_indexing():
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    cap = 1100                                   # two 1024-row passes of the workgroup
    ns = (0, 1, 63, 64, 65, cap)
    P = len(ns)
    rng = np.random.RandomState(3)
    match = np.zeros((P, cap, 3), dtype=np.float32)
    for p in range(P):
        match[p, :, 0] = np.sort(rng.choice(4096, cap, replace=False))   # ascending i, as the matcher writes them
        match[p, :, 1] = rng.permutation(cap)
        match[p, :, 2] = rng.rand(cap)
    mask = (rng.rand(P, cap) < 0.6).astype(np.uint8)
    mask[5, 1020:1030] = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1]                  # across the pass boundary
    t = lambda a: torch.from_numpy(a).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    md, kd, nd = t(match), t(mask), i32(list(ns))
    n_inl = i32([int(mask[p, :n].sum()) for p, n in enumerate(ns)])
    out, n_out = L.op_filter_matches(md, nd, kd, i32([0] * P), n_inl, 0)
    for p, n in enumerate(ns):
        want = md[p, :n][kd[p, :n].bool()]
        k = int(n_out[p])
        assert k == want.shape[0] and torch.equal(out[p, :k], want), (p, n)
        assert not out[p, k:].any()
        assert k < 2 or bool((out[p, 1:k, 0] > out[p, :k - 1, 0]).all())  # rows keep ascending i
    # pass-through: no model (status 1), or fewer inliers than min_inliers; decided per pair on the device
    status = i32([0, 1, 1, 0, 0, 0])
    out2, n_out2 = L.op_filter_matches(md, nd, kd, status, n_inl, 40)
    for p, n in enumerate(ns):
        through = int(status[p]) != 0 or int(n_inl[p]) < 40
        want = md[p, :n] if through else md[p, :n][kd[p, :n].bool()]
        assert int(n_out2[p]) == want.shape[0] and torch.equal(out2[p, :want.shape[0]], want), (p, n, through)
    assert int(n_inl[5]) >= 40 and int(n_out2[5]) == int(n_inl[5]) and int(n_out2[2]) == 63   # both branches were taken
    out3, n_out3 = L.op_filter_matches(md, nd, kd, i32([1] * P), n_inl, 0)                     # no model anywhere
    assert torch.equal(n_out3, nd) and torch.equal(out3[5], md[5])
    one, n_one = L.op_filter_matches(md[4], nd[4:5], kd[4:5], i32([0]), n_inl[4:5], 0)     # the [cap, 3] form of one pair
    assert one.shape == (cap, 3) and torch.equal(one, out[4]) and int(n_one) == int(n_out[4])
    with pytest.raises(ValueError):
        L.op_filter_matches(md, nd, kd[:, :cap - 1].contiguous(), i32([0] * P), n_inl, 0)


# ---- the trackers -------------------------------------------------------------------------------------------------------
N_POINTS, N_FRAMES, N_SWAPS, NN_THRESH, MAX_LENGTH = 60, 5, 4, 0.7, 4
# The baseline per frame is wide on purpose: with a short one (a few px of parallax) many matrices fit all true matches
# within 1 px and a sample that contains planted matches can win with them as inliers.  SCENE_SEED / CHECK_SEED were searched
# with the restatements (tests/epipolar_ref.py, tests/eval_restatement.py): in every frame the winner's mask is the truth.
STEP, SCENE_SEED, CHECK_SEED = (0.4, 0.1, 0.16), 41, 9


@functools.lru_cache(maxsize=None)
def sequence(planar):
    """Five frames of a camera translating past N_POINTS fixed points (planar: all on one plane, so consecutive frames are
    related by a homography).  Every point keeps a unit descriptor; from each frame on, N_SWAPS new pairs of points exchange
    their descriptors, so the matcher returns 2 * N_SWAPS wrong matches per frame (exact descriptor matches, geometrically
    wrong by at least E.MARGIN = 25 px).  Returns [(xy [N,2], desc [N,256], wrong [N] bool over the PREVIOUS frame's points)]."""
    rng = np.random.RandomState(SCENE_SEED + planar)
    f, w, h = E.FOCAL, E.WIDTH, E.HEIGHT
    a = np.stack([rng.uniform(30, w - 30, N_POINTS), rng.uniform(30, h - 30, N_POINTS)], axis=1)
    # planar: the plane 0.3 X + 0.2 Y + Z = 6 along the rays of the first frame
    z = 6.0 / (1.0 + 0.3 * (a[:, 0] - w / 2) / f + 0.2 * (a[:, 1] - h / 2) / f) if planar else rng.uniform(4.0, 12.0, N_POINTS)
    X = np.stack([(a[:, 0] - w / 2) * z / f, (a[:, 1] - h / 2) * z / f, z], axis=1)
    step = np.array(STEP)
    desc = rng.randn(N_POINTS, 256)
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(np.float32)
    owner = np.arange(N_POINTS)            # owner[k]: the descriptor point k shows
    used = np.zeros(N_POINTS, dtype=bool)
    frames, prev_xy, prev_order = [], None, None
    for fr in range(N_FRAMES):
        Y = X - fr * step
        xy = np.stack([f * Y[:, 0] / Y[:, 2] + w / 2, f * Y[:, 1] / Y[:, 2] + h / 2], axis=1)
        wrong_pts = np.zeros(N_POINTS, dtype=bool)
        if fr > 0:
            pairs = 0
            for u in range(N_POINTS):
                for v in range(u + 1, N_POINTS):
                    if pairs == N_SWAPS or used[u] or used[v]:
                        continue
                    far = np.hypot(*(xy[u] - xy[v])) >= E.MARGIN
                    if not planar and far:   # (the wrong matches are u -> v and v -> u)
                        d = np.concatenate(E.line_dist(_F_const(step), prev_xy[[u, v]], xy[[v, u]]))
                        far = d.min() >= E.MARGIN
                    if far:
                        owner[u], owner[v] = owner[v], owner[u]
                        used[u] = used[v] = True
                        wrong_pts[[u, v]] = True
                        pairs += 1
            assert pairs == N_SWAPS
        order = rng.permutation(N_POINTS)          # the rows of a frame are in another order every frame
        wrong_prev = np.zeros(N_POINTS, dtype=bool)
        if fr > 0:
            wrong_prev[np.argsort(prev_order)[np.nonzero(wrong_pts)[0]]] = True
        frames.append((np.ascontiguousarray(xy[order]), np.ascontiguousarray(desc[owner[order]]), wrong_prev))
        prev_xy, prev_order = xy, order
    return frames


def _F_const(t):
    """F between consecutive frames of `sequence`: one focal length, translation t."""
    K = np.array([[E.FOCAL, 0.0, E.WIDTH / 2], [0.0, E.FOCAL, E.HEIGHT / 2], [0.0, 0.0, 1.0]])
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ki = np.linalg.inv(K)
    return Ki.T @ (-tx) @ Ki


def _table(L, table):
    return L.tracks_to_numpy(*L.op_track_select(table, 0)), table["state"].cpu().numpy()


def _device_frame(xy, desc, dev):
    return (torch.from_numpy(xy).to(dev), torch.tensor([xy.shape[0]], dtype=torch.int32, device=dev), torch.from_numpy(desc).to(dev))


def _reference(mode, planar, dev, check_seed, min_inliers=16, thresh=1.0):
    """Per frame: (table, state, filtered matches [k,3], mask over the unfiltered matches, unfiltered matches) from the
    operators: matcher -> RANSAC -> torch boolean indexing -> op_track_update."""
    from semantic_superpoint_amd import lib as L
    cap = 1024
    table = L.track_table(MAX_LENGTH, cap, dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    prev = None
    out = []
    for fr, (xy, desc, _) in enumerate(sequence(planar)):
        n = xy.shape[0]
        p = torch.zeros(1, cap, 2, dtype=torch.float64, device=dev)
        d = torch.zeros(1, cap, 256, device=dev)
        p[0, :n], d[0, :n] = torch.from_numpy(xy).to(dev), torch.from_numpy(desc).to(dev)
        cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        pp, pd, pc = prev if prev is not None else (torch.zeros_like(p), torch.zeros_like(d), zero)
        m, nm = L.op_match_two_way(pd, pc, d, cnt, NN_THRESH)
        seed = torch.tensor([check_seed + fr], dtype=torch.int64, device=dev)
        if mode == "fundamental":
            g = L.op_epipolar_ransac(pp, p, m, nm, seed, thresh=thresh)
        else:
            pad = torch.zeros(1, cap, 1, dtype=torch.float64, device=dev)
            g = L.op_eval_ransac(torch.cat([pp, pad], 2), torch.cat([p, pad], 2), m, nm, seed)
        k = int(nm)
        keep = g["mask"][0, :k].bool()
        if int(g["status"]) != 0 or int(g["n_inliers"]) < min_inliers:
            keep = torch.ones(k, dtype=torch.bool, device=dev)
        filt = torch.zeros(cap, 3, device=dev)
        kept = m[0, :k][keep]                                # torch boolean indexing
        filt[:kept.shape[0]] = kept
        table = L.op_track_update(table, filt, torch.tensor([kept.shape[0]], dtype=torch.int32, device=dev), cnt)
        out.append(_table(L, table) + (kept.cpu().numpy(), g["mask"][0, :k].cpu().numpy().astype(bool), m[0, :k].cpu().numpy()))
        prev = (p, d, cnt)
    return out


@pytest.mark.parametrize("mode", ("fundamental", "homography"))
def test_tracker_with_geometric_check(mode):
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    planar = mode == "homography"
    ref = _reference(mode, planar, dev, check_seed=CHECK_SEED)
    tr = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check=mode, check_seed=CHECK_SEED)
    host = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check=mode, check_seed=CHECK_SEED)
    cc = PointTracker(MAX_LENGTH, NN_THRESH, dev, class_consistent=True, geometric_check=mode, check_seed=CHECK_SEED)
    plain = PointTracker(MAX_LENGTH, NN_THRESH, dev)
    removed = 0
    for fr, (xy, desc, wrong_prev) in enumerate(sequence(planar)):
        tr.update_device(*_device_frame(xy, desc, dev))
        plain.update_device(*_device_frame(xy, desc, dev))
        cc.update_device(*_device_frame(xy, desc, dev), cls=torch.zeros(xy.shape[0], dtype=torch.uint8, device=dev))
        host.update(np.concatenate([xy.T, np.ones((1, xy.shape[0]))]), desc.T.copy())
        rows, state, kept, mask, unfiltered = ref[fr]
        for t in (tr, host, cc):
            got_rows, got_state = _table(L, t.table)
            assert np.array_equal(got_rows, rows) and np.array_equal(got_state, state), (mode, fr)
        g = tr.last_geometry()
        assert np.array_equal(g["mask"][0, :mask.shape[0]].cpu().numpy().astype(bool), mask)
        # the scene: the matcher returned every point, the planted matches among them, and the check removed exactly those
        if fr > 0:
            assert unfiltered.shape[0] == N_POINTS and int(g["status"]) == 0
            planted = wrong_prev[unfiltered[:, 0].astype(int)]
            assert planted.sum() == 2 * N_SWAPS and np.array_equal(mask, ~planted), (mode, fr)
            removed += int((~mask).sum())
            assert not np.array_equal(_table(L, plain.table)[0], rows)     # without the check the wrong matches continue tracks
        got = host.get_matches()
        if fr > 0:
            prev_xy = sequence(planar)[fr - 1][0]
            want = np.concatenate([prev_xy[kept[:, 0].astype(int)].T, xy[kept[:, 1].astype(int)].T])
            assert np.array_equal(got, want) and np.array_equal(tr.get_matches(), want)
            assert np.array_equal(host.get_mscores(), kept.T.astype(np.float64))
    assert removed == 2 * N_SWAPS * (N_FRAMES - 1)


def test_tracker_without_check_is_unchanged():
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    old = PointTracker(MAX_LENGTH, NN_THRESH, dev)
    new = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check=None, check_thresh=2.0, min_inliers=3, check_seed=5)
    for xy, desc, _ in sequence(False):
        old.update_device(*_device_frame(xy, desc, dev))
        new.update_device(*_device_frame(xy, desc, dev))
        for k in ("ids", "tid", "score", "state"):
            n = int(old.table["state"][0]) if k != "state" else None
            assert torch.equal(old.table[k][:n], new.table[k][:n]), k     # bit for bit
        assert new.last_geometry() is None
    with pytest.raises(ValueError):
        PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="essential")


def test_tracker_keeps_everything_below_min_inliers():
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.export import PointTracker
    dev = _dev()
    plain = PointTracker(MAX_LENGTH, NN_THRESH, dev)
    loose = PointTracker(MAX_LENGTH, NN_THRESH, dev, geometric_check="fundamental", min_inliers=N_POINTS + 1, check_seed=CHECK_SEED)
    for xy, desc, _ in sequence(False):
        plain.update_device(*_device_frame(xy, desc, dev))
        loose.update_device(*_device_frame(xy, desc, dev))
    assert np.array_equal(_table(L, plain.table)[0], _table(L, loose.table)[0])
    assert int(loose.last_geometry()["status"]) == 0 and int(loose.last_geometry()["n_inliers"]) == N_POINTS - 2 * N_SWAPS


@pytest.mark.parametrize("mode", ("fundamental", "homography"))
def test_sequence_tracker_step_does_not_synchronise(tmp_path, mode):
    from semantic_superpoint_amd import lib as L
    from semantic_superpoint_amd.export import SequenceTracker
    from tests.test_gpu_tracks import _agent, _no_host_sync, _shifted_frames
    dev = _dev()
    agent = _agent(tmp_path, dev)
    args = (agent.net, dev, agent.conf_thresh, agent.nms_dist, False, agent.nn_thresh, 3)
    seq = SequenceTracker(*args, geometric_check=mode, check_thresh=1.0, min_inliers=8)
    loose = SequenceTracker(*args, geometric_check=mode, min_inliers=10 ** 6)    # the check runs, every match passes
    plain = SequenceTracker(*args)
    assert plain.tracker.geometric_check is None and seq.tracker.min_inliers == 8
    for f, im in enumerate(_shifted_frames()):            # 64x96 frames
        on_dev = torch.from_numpy(im).to(dev)
        if f == 0:
            seq.step(on_dev)                              # (the first step allocates)
        else:
            with _no_host_sync():
                seq.step(on_dev)
        loose.step(on_dev)
        plain.step(on_dev)
        assert np.array_equal(_table(L, loose.tracker.table)[0], _table(L, plain.tracker.table)[0])
        g = seq.tracker.last_geometry()
        k = seq.tracker.get_matches().shape[1]
        k_plain = plain.tracker.get_matches().shape[1]
        if f > 0:
            filtered = int(g["status"]) == 0 and int(g["n_inliers"]) >= 8
            assert k == (int(g["n_inliers"]) if filtered else k_plain) and k <= k_plain
    assert plain.tracker.get_matches().shape[1] >= 1
