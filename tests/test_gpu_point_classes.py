"""GPU: semantic keypoints - the class of each keypoint without the class map (ssp_op_point_classes /
ssp_point_classes), the stable class filter (ssp_op_filter_points), the class-aware two-way matcher
(ssp_match_two_way_classes) and their use in Engine.describe_points, PointTracker, SequenceTracker and DescriptorExporter.

The yardsticks: tests/point_classes_ref.py (fp64 numpy restatement, checked by hand in tests/test_point_classes_cpu.py), the
existing class-map kernel (op_sem_predict, bit for bit) and the existing matcher (op_match_two_way, bit for bit when all
classes are equal).  Tolerance of the random-logit check: DESIGN section 16's 8 * 2^-24 * max|logit| - a class value is four
products and three sums of magnitude <= max|logit| in fp32, and the winner is compared with the true maximum."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as C
from tests import point_classes_ref as R

pytestmark = pytest.mark.gpu
ARCH = "SuperPointNet_gauss2_ssmall"
NC = 133


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _all_pixels(B, h, w, stride=5):
    """every pixel of a B x h x w image as a point row (x, y, ...): cap = h * w"""
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    pts = np.zeros((B, h * w, stride), dtype=np.float32)
    pts[:, :, 0], pts[:, :, 1] = xs.reshape(-1), ys.reshape(-1)
    pts[:, :, 2:] = 0.5
    return pts


# ---- classes ----

@pytest.mark.parametrize("hc,wc", [(2, 3), (4, 5)])
def test_integer_logits_equal_the_restatement_at_every_pixel(hc, wc):
    """Integer logits in {-2..2}: every interpolant is a multiple of 2^-8, exact in fp32 in any order, and ties are everywhere.
    16x24: every pixel touches a border clamp; 32x40: interior as well.  Every pixel is a point."""
    from semantic_superpoint_amd import lib as L
    g = torch.Generator().manual_seed(7 + hc)
    B, h, w = 2, 8 * hc, 8 * wc
    sout = torch.randint(-2, 3, (B, NC, hc, wc), generator=g).float()
    pts = _all_pixels(B, h, w)
    count = np.array([h * w, h * w], dtype=np.int32)
    want = R.point_classes(sout.numpy(), pts, count)
    l0 = np.stack([R.logits_at(sout.numpy(), 0, x, y) for x, y in pts[0, :, :2]])
    ties = float(((l0 == l0.max(1, keepdims=True)).sum(1) > 1).mean())
    cls = L.op_point_classes(sout.to(_dev()), torch.from_numpy(pts).to(_dev()), torch.from_numpy(count).to(_dev()))
    assert cls.dtype == torch.uint8 and tuple(cls.shape) == (B, h * w)
    print("share of pixels with an exact tie at the top: %.3f, mismatches %d" % (ties, int((cls.cpu().numpy() != want).sum())))
    assert ties > 0.25          # (a property of the inputs alone: 0.73 at 16x24, 0.40 at 32x40)
    assert np.array_equal(cls.cpu().numpy(), want)
    pred, _ = L.op_sem_predict(sout.to(_dev()))
    assert torch.equal(cls.view(B, h, w), pred)


@pytest.mark.parametrize("n_classes,cs", [(5, 8), (64, 64), (65, 72), (133, 136)])
def test_class_counts_and_poisoned_padding(n_classes, cs):
    """5 classes, one full lane pass, one class into the second pass, and the engine's 133 / 136.  All class logits are negative
    and the padding channels hold 1e9: a padding channel read by mistake would win everywhere."""
    from semantic_superpoint_amd import lib as L
    g = torch.Generator().manual_seed(n_classes)
    B, hc, wc = 2, 2, 3
    sout = torch.randint(-2, 3, (B, n_classes, hc, wc), generator=g).float() - 20.0
    sout[:, n_classes - 1, 0, 0] = 5.0   # the last class wins around the first cell
    x = torch.cat([sout, torch.full((B, cs - n_classes, hc, wc), 1e9)], 1) if cs > n_classes else sout
    pts = _all_pixels(B, 16, 24, stride=2)
    count = np.array([16 * 24, 16 * 24], dtype=np.int32)
    cls = L.op_point_classes(x.to(_dev()), torch.from_numpy(pts).to(_dev()), torch.from_numpy(count).to(_dev()),
                             n_classes=n_classes).cpu().numpy()
    assert int(cls.max()) == n_classes - 1 and int(cls[0, 0]) == n_classes - 1
    assert np.array_equal(cls, R.point_classes(sout.numpy(), pts, count))


@pytest.fixture(scope="module")
def random_case():
    """3 randn logits, 133 classes, B = 2 at 40x56 (5x7 cells), every pixel a point; the class map of the existing kernel and
    the fp64 logits at the points: shared, never modified"""
    from semantic_superpoint_amd import lib as L
    g = torch.Generator().manual_seed(11)
    B, hc, wc = 2, 5, 7
    sout = 3.0 * torch.randn(B, NC, hc, wc, generator=g)
    pts = _all_pixels(B, 8 * hc, 8 * wc)
    dev = _dev()
    pred, _ = L.op_sem_predict(sout.to(dev))
    s = sout.numpy()
    l64 = np.stack([[R.logits_at(s, k, x, y) for x, y in pts[k, :, :2]] for k in range(B)])
    return {"sout": sout, "pts": pts, "pred": pred, "l64": l64, "B": B, "h": 8 * hc, "w": 8 * wc}


def test_random_logits_equal_the_class_map_and_meet_the_fp64_bound(random_case):
    from semantic_superpoint_amd import lib as L
    rc, dev = random_case, _dev()
    B, h, w = rc["B"], rc["h"], rc["w"]
    count = torch.full((B,), h * w, dtype=torch.int32, device=dev)
    cls = L.op_point_classes(rc["sout"].to(dev), torch.from_numpy(rc["pts"]).to(dev), count)
    assert torch.equal(cls.view(B, h, w), rc["pred"])              # the existing kernel, bit for bit
    got, l64 = cls.cpu().numpy().astype(np.int64), rc["l64"]
    tol = 8.0 * 2.0 ** -24 * float(rc["sout"].abs().max())
    top = np.sort(l64, axis=2)
    chosen = np.take_along_axis(l64, got[:, :, None], 2)[:, :, 0]
    clear = top[:, :, -1] - top[:, :, -2] > 2 * tol
    print("tol %.3e  clear share %.6f  worst shortfall %.3e" % (tol, clear.mean(), float((top[:, :, -1] - chosen).max())))
    assert clear.mean() >= 0.99
    assert (chosen >= top[:, :, -1] - tol).all()
    assert np.array_equal(got[clear], l64.argmax(2)[clear])


def test_counts_and_rows_past_the_count(random_case):
    """counts 0, 1, cap and one image shorter than the other; a shuffled point order; a point outside the image is clamped"""
    from semantic_superpoint_amd import lib as L
    rc, dev = random_case, _dev()
    B, h, w = rc["B"], rc["h"], rc["w"]
    cap = 300
    rs = np.random.RandomState(3)
    sel = rs.permutation(h * w)[:cap]
    pts = np.ascontiguousarray(rc["pts"][:, sel])
    pts[0, 0, :2] = (-7, h + 20)                                    # clamps to (0, h - 1)
    flat = rc["pred"].cpu().numpy().reshape(B, h * w)
    want_full = flat[:, sel].copy()
    want_full[0, 0] = flat[0, (h - 1) * w]
    sout = rc["sout"].to(dev)
    for counts in ((0, 1), (cap, 137), (1, cap + 50)):            # (a count above cap is clamped to it)
        cls = L.op_point_classes(sout, torch.from_numpy(pts).to(dev), torch.tensor(counts, dtype=torch.int32, device=dev))
        got = cls.cpu().numpy()
        for k in range(B):
            n = min(counts[k], cap)
            assert np.array_equal(got[k, :n], want_full[k, :n]), (counts, k)
            assert (got[k, n:] == L.CLASS_NONE).all(), (counts, k)


def _engine(arch, B, H, W):
    from semantic_superpoint_amd.lib import Engine
    e = Engine(arch, B, H, W, _dev())
    e.load_state_dict(C.init_state_dict(arch, seed=1))
    return e


def test_engine_point_classes():
    """Engine.point_classes on a real eval forward equals the operator on the slot's logits rearranged to NCHW, the class map
    of Engine.sem_predict at the points, and (within section 16's bound) the arg-max of forward(want=("sem",))'s logits."""
    from semantic_superpoint_amd import lib as L
    B, H, W = 2, 64, 96
    dev = _dev()
    eng = _engine(ARCH, B, H, W)
    img = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(4)).to(dev)
    rs = np.random.RandomState(5)
    cap = 500
    pts = np.zeros((B, cap, 5), dtype=np.float32)
    pts[:, :, 0], pts[:, :, 1] = rs.randint(0, W, (B, cap)), rs.randint(0, H, (B, cap))
    count = torch.tensor([cap, 321], dtype=torch.int32, device=dev)
    p = torch.from_numpy(pts).to(dev)
    with pytest.raises(RuntimeError, match="no forward"):
        eng.point_classes(0, p, count)
    out = eng.forward(img, train=False, want=("sem",))
    cls = eng.point_classes(0, p, count)
    cs = (NC + 3) // 4 * 4
    logits = eng.debug_buffer(0, "Y13", (B, H // 8, W // 8, cs))[..., :NC].permute(0, 3, 1, 2).contiguous()
    assert torch.equal(cls, L.op_point_classes(logits, p, count))
    pred, _ = eng.sem_predict(0, B, H, W)
    xs, ys = torch.from_numpy(pts[:, :, 0]).long().to(dev), torch.from_numpy(pts[:, :, 1]).long().to(dev)
    at = torch.stack([pred[k, ys[k], xs[k]] for k in range(B)])
    assert torch.equal(cls[0], at[0]) and torch.equal(cls[1, :321], at[1, :321]) and bool((cls[1, 321:] == 255).all())
    sem = out["sem"].double()
    tol = 8.0 * 2.0 ** -24 * float(logits.abs().max())
    for k, n in ((0, cap), (1, 321)):
        l = sem[k][:, ys[k, :n], xs[k, :n]]                        # [C, n]
        chosen = l.gather(0, cls[k, :n].long()[None])[0]
        assert bool((chosen >= l.max(0).values - tol).all())
    assert len(torch.unique(cls[0])) > 1
    # describe_points(classes=True) = describe_points + point_classes; classes=False is the dict of old
    a = eng.describe_points(0, B)
    b = eng.describe_points(0, B, classes=True)
    assert sorted(a) == ["count", "desc", "pts"] and sorted(b) == ["cls", "count", "desc", "pts"]
    assert torch.equal(a["count"], b["count"]) and b["cls"].dtype == torch.uint8
    n0 = int(b["count"][0])
    assert n0 > 0 and torch.equal(b["desc"][0, :n0], a["desc"][0, :n0]) and torch.equal(b["pts"][0, :n0], a["pts"][0, :n0])
    assert torch.equal(b["cls"], eng.point_classes(0, b["pts"], b["count"]))
    assert bool((b["cls"][0, n0:] == 255).all()) and int(b["cls"][0, :n0].max()) < NC


def test_engine_without_segmentation_head_is_refused():
    import ctypes
    B, H, W = 1, 64, 96
    dev = _dev()
    eng = _engine("SuperPointNet_gauss2", B, H, W)
    eng.forward(torch.rand(B, 1, H, W, device=dev), train=False)
    p, c = torch.zeros(B, 8, 5, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    cls = torch.zeros(B, 8, dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    assert eng.lib.ssp_point_classes(eng.h, 0, B, vp(p.data_ptr()), 5, vp(c.data_ptr()), 8, vp(cls.data_ptr()), None) == -1
    with pytest.raises(RuntimeError, match="segmentation head"):
        eng.point_classes(0, p, c)
    with pytest.raises(RuntimeError, match="segmentation head"):
        eng.describe_points(0, B, classes=True)


# ---- filter ----

@pytest.fixture(scope="module")
def filter_case():
    """n = 3, cap = 1500, counts (1300, 0, 1500): the rows cross every workgroup boundary of the scan (1024 rows per block)"""
    rs = np.random.RandomState(21)
    n, cap = 3, 1500
    pts = rs.uniform(0, 100, (n, cap, 5)).astype(np.float32)
    desc = rs.standard_normal((n, cap, 256)).astype(np.float32)
    cls = rs.randint(0, NC, (n, cap)).astype(np.uint8)
    count = np.array([1300, 0, 1500], dtype=np.int32)
    dev = _dev()
    return {"np": (pts, count, desc, cls), "dev": tuple(torch.from_numpy(a).to(dev) for a in (pts, count, desc, cls))}


@pytest.mark.parametrize("which", ["keep_all", "drop_all", "random"])
def test_filter_equals_boolean_indexing(filter_case, which):
    from semantic_superpoint_amd import lib as L
    pts, count, desc, cls = filter_case["dev"]
    n, cap = cls.shape
    if which == "keep_all":
        mask = L.class_mask(drop=[], n_classes=NC)
    elif which == "drop_all":
        mask = L.class_mask(keep=[], n_classes=NC)
    else:
        mask = L.class_mask(keep=np.random.RandomState(2).permutation(NC)[:60], n_classes=NC)
    before = [t.clone() for t in (pts, count, desc, cls)]
    o = L.op_filter_points(pts, count, desc, cls, mask)
    again = L.op_filter_points(pts, count, desc, cls, mask)
    assert all(torch.equal(a, b) for a, b in zip(before, (pts, count, desc, cls)))      # out of place
    bits = torch.from_numpy(R.mask_bits(mask)).to(cls.device)
    new = o["count"].cpu().tolist()
    for k in range(n):
        keep = bits[cls[k].long()] & (torch.arange(cap, device=cls.device) < count[k])
        m = int(keep.sum())
        assert new[k] == m, (which, k)
        assert torch.equal(o["pts"][k, :m], pts[k][keep]) and torch.equal(o["desc"][k, :m], desc[k][keep])   # order preserved
        assert torch.equal(o["cls"][k, :m], cls[k][keep]) and bool((o["cls"][k, m:] == L.CLASS_NONE).all())
        assert torch.equal(again["pts"][k, :m], o["pts"][k, :m]) and torch.equal(again["desc"][k, :m], o["desc"][k, :m])
    assert torch.equal(again["count"], o["count"]) and torch.equal(again["cls"], o["cls"])  # bit-identical on a repeat call
    if which == "keep_all":
        assert new == [1300, 0, 1500]
    if which == "drop_all":
        assert new == [0, 0, 0]
    if which == "random":
        assert 0 < new[0] < 1300 and 0 < new[2] < 1500
        rp, rn, rd, rc = R.filter_points(*filter_case["np"], mask)                          # the numpy restatement
        assert np.array_equal(rn, o["count"].cpu().numpy()) and np.array_equal(rc, o["cls"].cpu().numpy())
        assert np.array_equal(rp[0, :rn[0]], o["pts"][0, :rn[0]].cpu().numpy())


# ---- matcher ----

MATCH_SEEDS = (0, 3, 5)          # one per pair; checked on the CPU (tests/test_point_classes_cpu.py)
MATCH_THRESH = 1.3


def match_case(seed, n1=70, n2=130):
    """Unit descriptors with three classes: the first 50 rows of side 2 are noisy copies of rows of side 1 (a fifth of them with
    another class than their original, which the class test must keep apart), the rest is random.  Random pairs lie near
    sqrt(2); MATCH_THRESH admits the nearest of them, so the masked arg-mins decide matches beyond the copies."""
    rng = np.random.default_rng(1000 + seed)
    d1 = R.unit_rows(rng, n1)
    d2 = R.unit_rows(rng, n2)
    src = rng.permutation(n1)[:50]
    noisy = d1[src] + 0.35 * R.unit_rows(rng, 50)
    d2[:50] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
    c1 = rng.integers(0, 3, n1).astype(np.uint8)
    c2 = rng.integers(0, 3, n2).astype(np.uint8)
    c2[:50] = c1[src]
    c2[:50:5] = (c2[:50:5] + 1) % 3
    return d1, d2, c1, c2


def _match_tensors(cases, cap, dev, pair_stride=2):
    """pair p at entry p * pair_stride; the other entries and the rows past the counts hold descriptors that would match"""
    P = len(cases)
    rs = np.random.RandomState(9)
    d1 = np.zeros((P * pair_stride, cap, 256), dtype=np.float32)
    d2 = np.zeros_like(d1)
    c1 = rs.randint(0, 3, (P * pair_stride, cap)).astype(np.uint8)
    c2 = rs.randint(0, 3, (P * pair_stride, cap)).astype(np.uint8)
    n1 = np.zeros(P * pair_stride, dtype=np.int32)
    n2 = np.zeros(P * pair_stride, dtype=np.int32)
    for p, (a, b, ca, cb) in enumerate(cases):
        e = p * pair_stride
        d1[e:e + pair_stride], d2[e:e + pair_stride] = b[0], a[0]          # decoys everywhere ...
        d1[e, :len(a)], d2[e, :len(b)] = a, b                               # ... then the pair's rows below its counts
        c1[e, :len(a)], c2[e, :len(b)] = ca, cb
        n1[e], n2[e] = len(a), len(b)
        n1[e + 1:e + pair_stride], n2[e + 1:e + pair_stride] = cap, cap
    return tuple(torch.from_numpy(t).to(dev) for t in (d1, n1, d2, n2, c1, c2))


def _decided(d1, d2, c1, c2, thresh):
    """the restatement's arg-mins and threshold tests are decided by more than 1e-5 (fp32 distances differ from fp64 by ~1e-7)"""
    assert R.best_second_gaps(d1, d2, c1, c2) > 1e-5
    d = R.distances(d1, d2)
    d[c1[:, None] != c2[None, :]] = np.inf
    rowmin = d.min(1)
    assert np.abs(rowmin[np.isfinite(rowmin)] - thresh).min() > 1e-5


def test_class_matcher_equals_the_masked_restatement():
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    cases = [match_case(s) for s in MATCH_SEEDS]
    d1, n1, d2, n2, c1, c2 = _match_tensors(cases, 130, dev)
    match, n_match = L.op_match_two_way(d1, n1, d2, n2, MATCH_THRESH, pair_stride=2, cls1=c1, cls2=c2)
    plain, n_plain = L.op_match_two_way(d1, n1, d2, n2, MATCH_THRESH, pair_stride=2)
    assert tuple(match.shape) == (3, 130, 3) and tuple(n_match.shape) == (3,)
    for p, (a, b, ca, cb) in enumerate(cases):
        _decided(a, b, ca, cb, MATCH_THRESH)
        want = R.match_two_way_classes(a, b, ca, cb, MATCH_THRESH)
        m = int(n_match[p])
        got = match[p, :m].cpu().numpy().astype(np.float64)
        assert m == len(want) and m > 20, (p, m, len(want))
        assert np.array_equal(got[:, :2], want[:, :2]), p
        assert np.abs(got[:, 2] - want[:, 2]).max() < 1e-5            # fp32 dot products of 256 terms, then sqrt (d >= 0.3 here)
        assert (ca[got[:, 0].astype(int)] == cb[got[:, 1].astype(int)]).all()
        assert (np.diff(got[:, 0]) > 0).all()                          # ascending i
        # the class test changed something: the plain matcher pairs rows of different classes
        pm = plain[p, :int(n_plain[p])].cpu().numpy()
        assert (ca[pm[:, 0].astype(int)] != cb[pm[:, 1].astype(int)]).any()


def test_class_matcher_with_equal_classes_is_the_plain_matcher():
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    d1, n1, d2, n2, c1, c2 = _match_tensors([match_case(s) for s in MATCH_SEEDS], 130, dev)
    for thresh in (MATCH_THRESH, 0.7):
        plain, n_plain = L.op_match_two_way(d1, n1, d2, n2, thresh, pair_stride=2)
        for c in (0, 7, 254):
            same = torch.full_like(c1, c)
            match, n_match = L.op_match_two_way(d1, n1, d2, n2, thresh, pair_stride=2, cls1=same, cls2=same)
            assert torch.equal(n_match, n_plain) and int(n_plain.min()) > 0
            for p in range(3):
                assert torch.equal(match[p, :int(n_plain[p])], plain[p, :int(n_plain[p])])


def test_class_matcher_edge_cases():
    from semantic_superpoint_amd import lib as L
    dev = _dev()
    a, b, ca, cb = match_case(MATCH_SEEDS[0])
    # class 2 on side 1 only: those rows get no match, the others match as if the rows were absent
    cb2 = np.where(cb == 2, 1, cb).astype(np.uint8)
    d1, n1, d2, n2, c1, c2 = _match_tensors([(a, b, ca, cb2)], 130, dev, pair_stride=1)
    _decided(a, b, ca, cb2, MATCH_THRESH)
    match, n_match = L.op_match_two_way(d1, n1, d2, n2, MATCH_THRESH, cls1=c1, cls2=c2)
    got = match[0, :int(n_match[0])].cpu().numpy()
    assert (ca == 2).sum() > 10 and len(got) > 10 and not (ca[got[:, 0].astype(int)] == 2).any()
    assert np.array_equal(got[:, :2], R.match_two_way_classes(a, b, ca, cb2, MATCH_THRESH)[:, :2])
    # disjoint class sets: no match at all
    match, n_match = L.op_match_two_way(d1, n1, d2, n2, 2.5, cls1=torch.full_like(c1, 3), cls2=torch.full_like(c2, 4))
    assert int(n_match[0]) == 0
    # an empty side
    zero = torch.zeros_like(n1)
    for x, y in ((zero, n2), (n1, zero), (zero, zero)):
        match, n_match = L.op_match_two_way(d1, x, d2, y, 2.5, cls1=c1, cls2=c2)
        assert int(n_match[0]) == 0
    with pytest.raises(ValueError, match="both or neither"):
        L.op_match_two_way(d1, n1, d2, n2, 1.0, cls1=c1)
    with pytest.raises(ValueError, match="uint8"):
        L.op_match_two_way(d1, n1, d2, n2, 1.0, cls1=c1.int(), cls2=c2)
    with pytest.raises(RuntimeError, match="HIP device"):
        L.op_match_two_way(d1, n1, d2, n2, 1.0, cls1=c1.cpu(), cls2=c2)


# ---- front end ----

def _frames():
    big = np.random.RandomState(1900).uniform(0, 1, (64, 96 + 8)).astype(np.float32)
    return [torch.from_numpy(big[:, 2 * k:2 * k + 96].copy()) for k in range(5)]   # a fixed image shifted by 2 px per frame


def _class_shares(net, dev, image, conf_thresh, nms_dist):
    eng = net.engine(1, 64, 96, dev)
    with torch.no_grad():
        eng.forward(image.to(dev)[None, None].contiguous(), slot=0, train=False, want=())
    o = eng.describe_points(0, 1, conf_thresh=conf_thresh, nms_dist=nms_dist, subpixel=False, classes=True)
    n = int(o["count"][0])
    ids, cnt = np.unique(o["cls"][0, :n].cpu().numpy(), return_counts=True)
    return n, {int(i): c / n for i, c in zip(ids, cnt)}


@pytest.fixture(scope="module")
def front(tmp_path_factory):
    """A random-init Semantic-SuperPoint whose keypoints spread over at least three classes: convSout is perturbed with fixed
    seeds until three classes hold 10 % of frame 0's points each (a random-init head puts every keypoint into one class)."""
    from tests.test_gpu_tracks import _agent
    dev = _dev()
    agent = _agent(tmp_path_factory.mktemp("w"), dev)
    net, frames = agent.net, _frames()
    w0 = net.convSout.weight.detach().clone()
    big, attempt = [], 0
    while True:
        n, shares = _class_shares(net, dev, frames[0], agent.conf_thresh, agent.nms_dist)
        big = sorted((c for c, s in shares.items() if s >= 0.1), key=lambda c: -shares[c])
        print("attempt %d: %d points, shares %s" % (attempt, n, {c: round(shares[c], 3) for c in big}))
        if len(big) >= 3 or attempt == 8:
            break
        noise = np.random.RandomState(1000 + attempt).normal(0, 1.0, tuple(w0.shape)).astype(np.float32)
        with torch.no_grad():
            net.convSout.weight.copy_(w0 + (2 * float(w0.abs().max())) * torch.from_numpy(noise).to(dev))
        attempt += 1
    assert len(big) >= 3 and n >= 30, (n, shares)
    return {"agent": agent, "frames": frames, "big": big, "dev": dev}


def _xy(o, subpixel):
    pts = o["pts"][0]
    xy = pts[:, :2].to(torch.float64)
    return xy + pts[:, 3:5].to(torch.float64) - 2 if subpixel else xy


def test_sequence_tracker_drop_classes(front):
    """SequenceTracker(drop_classes=...) leaves exactly the track table of a plain PointTracker fed the same frames' tensors
    filtered with torch boolean indexing; the steps after the first queue no host synchronisation."""
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    from tests.test_gpu_tracks import _no_host_sync
    agent, dev, frames = front["agent"], front["dev"], front["frames"]
    drop = [front["big"][0], front["big"][2]]
    ml = 3
    for subpixel in (False, True):
        seq = SequenceTracker(agent.net, dev, agent.conf_thresh, agent.nms_dist, subpixel, agent.nn_thresh, ml, drop_classes=drop)
        plain = SequenceTracker(agent.net, dev, agent.conf_thresh, agent.nms_dist, subpixel, agent.nn_thresh, ml)
        host = PointTracker(ml, agent.nn_thresh, dev)
        dropped = 0
        for f, im in enumerate(frames):
            if f == 0:
                o = seq.step(im)
            else:
                on_dev = im.to(dev)              # (the upload of a host image synchronises; the step must not)
                with _no_host_sync():
                    o = seq.step(on_dev)
            full = plain.describe(im)
            eng = agent.net.engine(1, 64, 96, dev)
            cls = eng.point_classes(0, full["pts"], full["count"])[0]
            n = int(full["count"][0])
            keep = torch.ones(n, dtype=torch.bool, device=dev)
            for c in drop:
                keep &= cls[:n] != c
            m = int(keep.sum())
            dropped += n - m
            assert int(o["count"][0]) == m and torch.equal(o["pts"][0, :m], full["pts"][0, :n][keep])
            assert torch.equal(o["desc"][0, :m], full["desc"][0, :n][keep]) and torch.equal(o["cls"][0, :m], cls[:n][keep])
            host.update_device(_xy(full, subpixel)[:n][keep].contiguous(), torch.tensor([m], dtype=torch.int32, device=dev),
                               full["desc"][0, :n][keep].contiguous())
        assert dropped > 20
        tracks = seq.get_tracks(2)
        assert tracks.shape[0] > 0 and np.array_equal(tracks, host.get_tracks(2))
        assert np.array_equal(seq.tracker.tracks, host.tracks)
        assert np.array_equal(seq.track_points(tracks), host.track_points(tracks), equal_nan=True)
    keep_seq = SequenceTracker(agent.net, dev, agent.conf_thresh, agent.nms_dist, False, agent.nn_thresh, ml,
                               keep_classes=[front["big"][1]])
    o = keep_seq.step(frames[0])
    n = int(o["count"][0])
    assert n > 0 and bool((o["cls"][0, :n] == front["big"][1]).all())


def test_class_consistent_tracking(front):
    from semantic_superpoint_amd.export import PointTracker, SequenceTracker
    agent, dev, frames = front["agent"], front["dev"], front["frames"]
    ml = 3
    seq = SequenceTracker(agent.net, dev, agent.conf_thresh, agent.nms_dist, False, agent.nn_thresh, ml, class_consistent=True)
    plain = PointTracker(ml, agent.nn_thresh, dev)
    forced = PointTracker(ml, agent.nn_thresh, dev, class_consistent=True)      # every point forced to one class
    prev, checked, differs = None, 0, 0
    for im in frames:
        o = seq.step(im)
        n = int(o["count"][0])
        cls = o["cls"][0, :n].cpu().numpy()
        xy, cnt, desc = _xy(o, False), o["count"][0:1], o["desc"][0]
        plain.update_device(xy, cnt, desc)
        forced.update_device(xy, cnt, desc, cls=torch.full_like(o["cls"][0], 9))
        m = seq.tracker.get_matches()                                            # [4, K] = x0, y0, x1, y1
        if prev is not None:
            assert m.shape[1] > 0
            lut_prev = {(x, y): c for (x, y), c in zip(prev[0], prev[1])}
            lut_now = {(x, y): c for (x, y), c in zip(map(tuple, xy[:n].cpu().numpy()), cls)}
            for x0, y0, x1, y1 in m.T:
                assert lut_prev[(x0, y0)] == lut_now[(x1, y1)]
                checked += 1
            differs += int(not np.array_equal(m, plain.get_matches()))
        else:
            plain.get_matches()
        prev = (list(map(tuple, xy[:n].cpu().numpy())), cls)
        assert np.array_equal(forced.tracks, plain.tracks)
    print("matches checked: %d; frames whose matches differ from the plain tracker's: %d" % (checked, differs))
    assert checked >= 4
    assert np.array_equal(forced.get_tracks(2), plain.get_tracks(2)) and np.array_equal(forced.get_matches(), plain.get_matches())
    with pytest.raises(ValueError, match="cls"):
        forced.update_device(xy, cnt, desc)


def test_defaults_do_not_touch_the_new_path(front):
    """With every new argument at its default, describe_points / SequenceTracker.step / DescriptorExporter.run_device give what
    a second engine gives that never ran the new code."""
    from semantic_superpoint_amd.export import DescriptorExporter, SequenceTracker
    from semantic_superpoint_amd.lib import Engine
    agent, dev, frames = front["agent"], front["dev"], front["frames"]
    seq = SequenceTracker(agent.net, dev, agent.conf_thresh, agent.nms_dist, True, agent.nn_thresh, 3)
    fresh = Engine(ARCH, 1, 64, 96, dev, with_grad=False)
    fresh.load_state_dict({k: v.detach().clone() for k, v in agent.net.state_dict().items()})
    for im in frames[:3]:
        o = seq.step(im)
        assert sorted(o) == ["count", "desc", "pts"]
        fresh.forward(im.to(dev)[None, None].contiguous(), slot=0, train=False, want=())
        want = fresh.describe_points(0, 1, conf_thresh=agent.conf_thresh, nms_dist=agent.nms_dist, subpixel=True)
        n = int(want["count"][0])
        assert n > 0 and torch.equal(o["count"], want["count"])
        assert torch.equal(o["pts"][0, :n], want["pts"][0, :n]) and torch.equal(o["desc"][0, :n], want["desc"][0, :n])
    pairs = [(frames[0], frames[1])]
    a = DescriptorExporter(agent.net, dev, agent.conf_thresh, agent.nms_dist, True, agent.nn_thresh, batch_pairs=1).run_device(pairs)
    b = DescriptorExporter(agent.net, dev, agent.conf_thresh, agent.nms_dist, True, agent.nn_thresh, batch_pairs=1,
                           classes=True).run_device(pairs)
    assert sorted(a) == ["count", "desc", "match", "n_match", "pts"] and sorted(b) == ["cls"] + sorted(a)
    assert torch.equal(a["count"], b["count"]) and torch.equal(a["n_match"], b["n_match"])
    for k in range(2):
        n = int(a["count"][k])
        assert n > 0 and torch.equal(a["pts"][k, :n], b["pts"][k, :n]) and torch.equal(a["desc"][k, :n], b["desc"][k, :n])
    assert torch.equal(a["match"][0, :int(a["n_match"][0])], b["match"][0, :int(a["n_match"][0])])
    eng = agent.net.engine(2, 64, 96, dev)
    assert torch.equal(b["cls"], eng.point_classes(0, b["pts"], b["count"]))


def test_segmentation_head_is_required(front):
    from semantic_superpoint_amd.export import DescriptorExporter, SequenceTracker
    from semantic_superpoint_amd.models.SuperPointNet_gauss2 import SuperPointNet_gauss2
    net = SuperPointNet_gauss2()
    for kw in ({"drop_classes": [1]}, {"keep_classes": [1]}, {"class_consistent": True}):
        with pytest.raises(ValueError, match="segmentation head"):
            SequenceTracker(net, front["dev"], 0.015, 4, False, 0.7, 3, **kw)
    with pytest.raises(ValueError, match="segmentation head"):
        DescriptorExporter(net, front["dev"], 0.015, 4, False, 0.7, classes=True)
    with pytest.raises(ValueError, match="exactly one"):
        SequenceTracker(front["agent"].net, front["dev"], 0.015, 4, False, 0.7, 3, keep_classes=[1], drop_classes=[2])
    with pytest.raises(ValueError, match="outside"):
        SequenceTracker(front["agent"].net, front["dev"], 0.015, 4, False, 0.7, 3, drop_classes=[133])
