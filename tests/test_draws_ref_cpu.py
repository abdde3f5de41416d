"""CPU: the restatements of the kernels that take random decisions on the device are pinned here, without a GPU:
  index sampler (tests/draws_ref.py)            the oracle's cell correspondences, published splitmix64 outputs, mutants
  photometric draw and noise (photometric_ref)  row 0 by hand, neutral columns, float64 against longdouble weight casts, mutants
  Synthetic Shapes draw (shapes_ref.draw)       the committed device tables g18 word for word, check_row, mutants
  the draw logic against the reference itself   datasets/synthetic_dataset.py imported in place with a recording cv2 (skipped
                                                where the reference is absent)
A wrong rule must change a value of the compared cases, or the GPU comparison could not see it.  The shares the GPU tests may
leave out are asserted here, from the restatements alone, for exactly the cases tests/test_gpu_draws_exact.py runs
(tests/draws_cases.py)."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref as C
from tests import draws_cases as DC
from tests import draws_ref as D

F32 = np.float32


def test_splitmix64_published_outputs():
    """The first three outputs of splitmix64 seeded with 0 (Vigna's splitmix64.c; the values every xoshiro seeding test quotes):
    output k is the finaliser of the state k * 0x9E3779B97F4A7C15, the scalar and the vectorised form alike."""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    states = [(k * D.GOLDEN) & D.M64 for k in range(3)]
    assert [D.splitmix64(s) for s in states] == want
    assert D.splitmix64_np(np.array(states, np.uint64)).tolist() == want
    rs = np.random.RandomState(0)
    x = rs.randint(0, 2 ** 63, 1000).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, 1000).astype(np.uint64)
    assert D.splitmix64_np(x).tolist() == [D.splitmix64(int(v)) for v in x]


@pytest.mark.parametrize("name", list(DC.SAMPLER_CASES))
def test_sampler_targets_equal_the_oracles_cell_matches(name):
    """The valid set and match_b of the restatement == oracle.cpu_ref.cell_matches (sparse_loss.py:184-207) for the host-scaled
    matrices; every sampled pair is one of them, the matches are distinct up to nv, and the fill repeats sorted positions."""
    H, W, seed = DC.SAMPLER_CASES[name]
    Hc, Wc = H // 8, W // 8
    hs, ch = DC.sampler_homographies(name), DC.cell_homographies(name)
    nvs = []
    for b in range(DC.SAMPLER_B):
        uv_a, uv_b = C.cell_matches(torch.from_numpy(hs[b]), Hc, Wc)
        ia = (uv_a[:, 0] + uv_a[:, 1] * Wc).long().numpy()
        ib = (uv_b[:, 0] + uv_b[:, 1] * Wc).long().numpy()
        valid, cb = D.cell_targets(ch[b], Hc, Wc)
        assert np.array_equal(np.nonzero(valid)[0], ia), (name, b)
        assert np.array_equal(cb[valid], ib), (name, b)
        ma, mb = D.sampler_matches(ch[b], seed, b, Hc, Wc, DC.N_MATCH)
        nv = int(valid.sum())
        nvs.append(nv)
        if nv == 0:
            assert not ma.any() and not mb.any()
            continue
        assert valid[ma].all() and np.array_equal(cb[ma], mb)
        assert len(set(ma[:nv].tolist())) == min(nv, DC.N_MATCH)
        assert set(ma[nv:].tolist()) <= set(ma[:nv].tolist())
    print("sampler %s: nv %s of %d cells" % (name, nvs, Hc * Wc))
    if name == "64x96":
        assert all(0 < nv < DC.N_MATCH for nv in nvs)                 # every image fills with replacement
    elif name == "240x320":
        assert nvs[0] == Hc * Wc and nvs[2] == 0 and DC.N_MATCH - 50 <= nvs[1] < DC.N_MATCH
    else:
        assert all(nv >= DC.N_MATCH for nv in nvs) and Hc * Wc > 4096     # the 8192-key sort, no fill


def test_sampler_mutants_change_an_index():
    """Each wrong rule changes at least one index of the compared cases (over the three cases; `fill_ncell` can only show where
    nv < n_match, so it is also checked on such a case alone)."""
    moved = {m: 0 for m in D.MATCH_MUTANTS + D.NONMATCH_MUTANTS}
    for name, (H, W, seed) in DC.SAMPLER_CASES.items():
        Hc, Wc = H // 8, W // 8
        ch = DC.cell_homographies(name)
        for b in range(DC.SAMPLER_B):
            valid, cb = D.cell_targets(ch[b], Hc, Wc)
            ma, mb = D.matches_from_targets(valid, cb, seed, b, DC.N_MATCH)
            for m in D.MATCH_MUTANTS:
                xa, xb = D.matches_from_targets(valid, cb, seed, b, DC.N_MATCH, mutant=m)
                d = int((xa != ma).sum() + (xb != mb).sum())
                if m == "img32" and b == 0:
                    assert d == 0            # image 0: the shift cannot matter
                if m == "fill_ncell" and name == "64x96":
                    assert d > 0
                moved[m] += d
        total = DC.SAMPLER_B * DC.N_MATCH * DC.N_NON
        nm = D.sampler_nonmatches(seed, total, Hc, Wc)
        assert nm.min() >= 0 and nm.max() < Hc * Wc
        for m in D.NONMATCH_MUTANTS:
            d = int((D.sampler_nonmatches(seed, total, Hc, Wc, mutant=m) != nm).sum())
            assert d > total // 2, (name, m, d)
            moved[m] += d
    print("indices moved by each mutant:", moved)
    assert all(v > 0 for v in moved.values()), moved


def test_sampler_nonmatch_scalar_form():
    """The vectorised non-match draw == the rule written out with Python integers and one float32 product per coordinate."""
    seed, Hc, Wc = 0x1234567890ABCDEF, 30, 40
    nm = D.sampler_nonmatches(seed, 500, Hc, Wc)
    for i in range(500):
        r = D.splitmix64(seed ^ 0x5EED5EED ^ ((i * D.GOLDEN) & D.M64))
        u1, u2 = F32((r >> 40) / 16777216.0), F32(((r >> 16) & 0xFFFFFF) / 16777216.0)
        u, v = min(int(np.floor(u1 * F32(Wc))), Wc - 1), min(int(np.floor(u2 * F32(Hc))), Hc - 1)
        assert nm[i] == u + v * Wc, i


def analytic_cell_warp32(hn, Hc, Wc):
    """pixel_homography_analytic followed by warp_points32, every operation rounded once to float32 in the written order (no
    contraction): ONE of the float32 evaluations the bound of draws_ref.analytic_cell_warp64 must cover."""
    h = np.asarray(hn, F32).reshape(3, 3)
    a, b = F32(2) / F32(Wc), F32(2) / F32(Hc)
    M = np.stack((h[:, 0] * a, h[:, 1] * b, (-h[:, 0] - h[:, 1]) + h[:, 2]), axis=1)
    P = np.stack(((M[0] + M[2]) / a, (M[1] + M[2]) / b, M[2]))
    assert P.dtype == F32
    from tests import pairs_ref as R
    return R.warp_points32(P, D.cell_grid(Hc, Wc))


def test_sampler_analytic_margin_covers_fp32_and_stays_small():
    """The analytic path: (1) the uncontracted float32 evaluation stays inside the derived bound of the float64 one at every
    cell with a finite bound; (2) over the compared cases the undecided share stays below MARGIN_CAP; (3) every decided cell
    of the float64 form agrees with the host-scaled float32 form (two independent routes to the same correspondence)."""
    cells = undecided = 0
    worst = 0.0
    for name, (H, W, seed) in DC.SAMPLER_CASES.items():
        Hc, Wc = H // 8, W // 8
        hs, ch = DC.sampler_homographies(name), DC.cell_homographies(name)
        for b in range(DC.SAMPLER_B):
            wu, wv, bound = D.analytic_cell_warp64(hs[b], Hc, Wc)
            w32 = analytic_cell_warp32(hs[b], Hc, Wc).astype(np.float64)
            ok = np.isfinite(bound)
            dev = np.maximum(np.abs(w32[:, 0] - wu), np.abs(w32[:, 1] - wv))
            assert (dev[ok] <= bound[ok]).all(), (name, b, float((dev[ok] / bound[ok]).max()))
            worst = max(worst, float((dev[ok] / bound[ok]).max()))
            valid, cb, decided = D.analytic_targets(hs[b], Hc, Wc)
            v32, c32 = D.cell_targets(ch[b], Hc, Wc)
            assert np.array_equal(valid[decided], v32[decided]) and np.array_equal(cb[decided], c32[decided]), (name, b)
            cells += Hc * Wc
            undecided += int((~decided).sum())
    print("analytic path: %d cells, %d undecided (share %.2e), largest fp32 deviation / bound %.3f" %
          (cells, undecided, undecided / cells, worst))
    assert undecided / cells < DC.MARGIN_CAP


# ------------------------------------------------------------------------------------------------ photometric draw and noise
def test_photometric_draw_margins_and_neutral_columns():
    """For exactly the seed, sizes and parameter sets of the GPU test: no row's decision margin is below MARGIN_MIN (the
    share left out is asserted below MARGIN_CAP); a primitive that is off leaves its neutral values; the draw obeys the
    reference's ranges; switching a primitive off moves every LATER primitive's draw (it consumes no uniform) and none
    before it."""
    from tests import photometric_ref as P
    for H, W in DC.PHOTO_SIZES:
        full = DC.photo_rows("shipped", H, W)[0]
        left = 0
        for name in DC.photo_param_sets():
            rows, margin, _ = DC.photo_rows(name, H, W)
            left += int((margin < DC.MARGIN_MIN).sum())
            assert (margin < DC.MARGIN_MIN).mean() < DC.MARGIN_CAP, (name, H, W)
            neutral = P.make_row()
            cols = {"no_brightness": [P.BRIGHTNESS], "no_contrast": [P.CONTRAST], "no_noise": [P.SIGMA], "no_impulse": [P.IMPULSE_P],
                    "no_motion_blur": list(range(P.BLUR_FLAG, P.BLUR_W + 9)), "no_shade": list(range(P.ELLIPSES, P.KEY))}.get(name, [])
            assert np.array_equal(rows[:, cols], np.tile(neutral[cols], (DC.PHOTO_B, 1))), name
            order = [[P.BRIGHTNESS], [P.CONTRAST], [P.SIGMA], [P.IMPULSE_P], list(range(P.BLUR_FLAG, P.BLUR_W + 9)), list(range(P.ELLIPSES, P.KEY))]
            if cols:
                k = order.index(cols)
                for before in order[:k]:
                    assert np.array_equal(rows[:, before], full[:, before]), (name, before[0])
                for after in order[k + 1:]:
                    assert not np.array_equal(rows[:, after], full[:, after]), (name, after[0])
            assert np.array_equal(rows[:, P.KEY:], full[:, P.KEY:])          # the key words come from the stream key alone
        print("photometric draw %dx%d: %d rows over 7 parameter sets, %d left out for a margin" % (H, W, 7 * DC.PHOTO_B, left))
        ell = full[:, P.ELLIPSES:P.ELLIPSES + 5 * P.MAX_ELLIPSES].reshape(DC.PHOTO_B, P.MAX_ELLIPSES, 5)[:, :20]
        cx, cy, ax, ay, ang = (ell[..., i] for i in range(5))
        md = min(H, W) / 4
        rad = np.maximum(ax, ay)
        assert ax.min() >= int(md / 5) and ax.max() <= md and (cx >= rad).all() and (cx < np.maximum(W - rad, rad + 1)).all()
        assert (cy >= rad).all() and (cy < np.maximum(H - rad, rad + 1)).all() and ang.min() >= 0 and ang.max() < 90
        assert set(np.unique(full[:, P.KSIZE] % 2)) == {1.0} and full[:, P.KSIZE].min() >= 101 and full[:, P.KSIZE].max() <= 151
        assert np.abs(full[:, P.BLUR_W:P.BLUR_W + 9].astype(np.float64).sum(axis=1) - 1).max() < 1e-6
        assert len({P.row_key(r) for r in full}) == DC.PHOTO_B


def test_photometric_draw_first_row_by_hand():
    """Row 0 of the shipped block written out once more from the uniforms, in the reference's order."""
    from tests import photometric_ref as P
    from tests.pairs_ref import M64, DeviceStream, mix
    H, W = 67, 93
    row = DC.photo_rows("shipped", H, W)[0][0]
    rs = DeviceStream(mix((DC.PHOTO_SEED ^ 0x70686F746F6D6574) & M64), 0)
    u = [rs.uniform() for _ in range(7 + 5 * 20 + 2)]
    assert row[P.BRIGHTNESS] == min(int(u[0] * 101), 100) - 50
    assert row[P.CONTRAST] == np.float32(0.5 + u[1]) and row[P.SIGMA] == np.float32(u[2] * 10.0)
    assert row[P.IMPULSE_P] == np.float32(u[3] * float(np.float32(0.0035)))
    assert row[P.BLUR_FLAG] == (1.0 if u[4] < 0.5 else 0.0)
    assert np.array_equal(row[P.BLUR_W:P.BLUR_W + 9], P.motion_blur_weights(u[5] * 360.0, u[6] * 2.0 - 1.0).reshape(9).astype(np.float32))
    md = min(H, W) / 4.0
    ax, ay = int(max(u[7] * md, md / 5)), int(max(u[8] * md, md / 5))
    r = max(ax, ay)
    first = (r + int(u[9] * (W - 2 * r)), r + int(u[10] * (H - 2 * r)), ax, ay, np.float32(u[11] * 90.0))
    assert tuple(row[P.ELLIPSES:P.ELLIPSES + 5]) == first
    assert row[P.TRANSPARENCY] == np.float32(-0.5 + u[107]) and row[P.KSIZE] == (100 + int(u[108] * 50)) | 1
    assert [int(row[P.KEY + i]) for i in range(4)] == [mix(rs.key ^ (0xA5A5 + i)) >> 48 for i in range(4)]


def test_photometric_weight_casts():
    """float(k_i / sum) of the compared rows: evaluated once more in numpy.longdouble from the same double cos / sin, the float32
    cast changes only where the double lies within 1e-12 relative of a float32 rounding midpoint - so the device's double
    evaluation (its cos / sin may differ from libm's in the last place) can give the float32 neighbour there and nowhere else."""
    from tests import photometric_ref as P
    n = close = 0
    for H, W in DC.PHOTO_SIZES[:1]:                       # the weights do not depend on the size
        for name in ("shipped", "no_brightness"):
            rows, margin, blur = DC.photo_rows(name, H, W)
            for b in range(DC.PHOTO_B):
                if margin[b] < DC.MARGIN_MIN:
                    continue
                dist, agree = P.weight_midpoint_distance(*blur[b])
                n += 9
                close += int((dist < 1e-12).sum())
                assert (agree | (dist < 1e-12)).all(), (name, b, dist[~agree])
    print("blur weights: %d compared, %d within 1e-12 relative of a float32 rounding midpoint" % (n, close))


def test_photometric_draw_mutants():
    """Each wrong rule changes a column of the compared rows."""
    from tests import photometric_ref as P
    H, W = DC.PHOTO_SIZES[1]
    ref = DC.photo_rows("shipped", H, W)[0]
    for m in P.DRAW_MUTANTS:
        rows = np.stack([P.draw(DC.PHOTO_SEED, n, P.SHIPPED, H, W, mutant=m)[0] for n in range(32)])
        d = int((rows != ref[:32]).sum())
        print("draw mutant %-15s moves %d values of 32 rows" % (m, d))
        assert d > 0, m


@pytest.mark.parametrize("hw", DC.NOISE_SIZES)
def test_photometric_noise_ties_and_mutants(hw):
    """For exactly the GPU cases: the tie set at NOISE_TAU stays below MARGIN_CAP of the pixels (under the 3x3 blur a tie excuses
    its neighbourhood: nine times that), both clips occur on the image of 0 and 1, and every mutant moves more pixels
    outside the tie set than the tie set holds - the comparison cannot hide it."""
    from tests import photometric_ref as P
    H, W = hw
    cases = DC.noise_cases(H, W)
    moved = {m: 0 for m in P.NOISE_MUTANTS}
    ties = 0
    for name, (img, rows) in cases.items():
        ref, may = zip(*[P.apply(img, r, tau=P.NOISE_TAU) for r in rows])
        ref, may = np.stack(ref), np.stack(may)
        ties += int(may.sum())
        assert may.mean() < (9 if rows[0][P.BLUR_FLAG] else 1) * DC.MARGIN_CAP, name
        if name == "sigma_binary":
            assert (ref == 0).any() and (ref == 1).any() and ((ref > 0) & (ref < 1)).any()
        for m in P.NOISE_MUTANTS:
            mut = np.stack([P.apply(img, r, tau=P.NOISE_TAU, mutant=m)[0] for r in rows])
            moved[m] += int(((mut != ref) & ~may).sum())
    print("noise %dx%d: %d pixels in tie sets; pixels moved outside them by each mutant: %s" % (H, W, ties, moved))
    for m, d in moved.items():
        # a pixel outside the tie set cannot be excused: one is enough.  The two mutants that differ on single 24-bit values
        # (u1 <= p: the field equal to p, case impulse_edge; u1 without the + 1: the field 0 under the hand-made key) move few
        # pixels by nature; every other one moves more than all tie sets together hold
        assert d > 0, (m, d)
        if m not in ("impulse_le", "u1_no_plus_one"):
            assert d > ties, (m, d, ties)


def test_photometric_noise_edge_pixels():
    """The purpose-made pixels: under the hand-made key pixel 669 draws the Gaussian field 0 (u1 = 2^-24, |z| up to 5.77); in the
    case impulse_edge the edge pixel's field equals p, so `<` keeps it and `<=` would replace it."""
    from tests import photometric_ref as P
    H, W = 24, 32
    key = DC.NOISE_KEYS_BY_HAND[2]
    assert int(P.pixel_hash(key, H, W, 0).reshape(-1)[669] >> np.uint64(40)) == 0
    pre, lvl, tie, _ = P.noise(P.make_row(sigma=10.0, key=key), H, W, tau=P.NOISE_TAU)
    assert abs(pre.reshape(-1)[669] - 128.0) > 50 and not tie.reshape(-1)[669]
    img, rows = DC.noise_cases(H, W)["impulse_edge"]
    for r in rows:
        f1 = int(P.pixel_hash(P.row_key(r), H, W, 1).reshape(-1)[DC.NOISE_EDGE_PIXEL] >> np.uint64(40))
        assert float(r[P.IMPULSE_P]) * 16777216.0 == f1
        quiet = P.apply(img, P.make_row(key=P.row_key(r)))[0]
        keep, mut = P.apply(img, r, tau=P.NOISE_TAU)[0], P.apply(img, r, tau=P.NOISE_TAU, mutant="impulse_le")[0]
        assert keep.reshape(-1)[DC.NOISE_EDGE_PIXEL] == quiet.reshape(-1)[DC.NOISE_EDGE_PIXEL]
        assert (keep != mut).sum() >= 1 and (f1 == 0 or (keep != quiet).any())


# ------------------------------------------------------------------------------------------------ Synthetic Shapes draw
def test_shapes_draw_reproduces_the_committed_tables():
    """tests/golden/g18_shapes_tables.npz was drawn on the device: the restatement reproduces every word of its 17 tables
    (FIXTURE_SEEDS and seeds 100 + k) and each restated row passes check_row."""
    import os
    from semantic_superpoint_amd import lib as L
    from tests import shapes_ref as S
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_shapes_tables.npz"))
    jobs = [("prim%d" % k, 100 + k, DC.shapes_params(k)) for k in range(9)]
    jobs += [(key, seed, DC.shapes_params("small")) for key, seed in S.FIXTURE_SEEDS.items()]
    n_tab = 0
    for key, seed, p in jobs:
        for n in range(g[key].shape[0]):
            row, margin, _ = S.draw(seed, n, p)
            assert margin >= DC.MARGIN_MIN, (key, n, margin)
            fw = S.float_words(row)
            plain = np.ones(S.ROW, bool)
            plain[fw] = False
            assert np.array_equal(row[plain], g[key][n][plain]), (key, n, np.nonzero(row != g[key][n])[0][:8])
            a, b = row[fw].view(np.float32), g[key][n][fw].view(np.float32)
            assert ((a == b) | (b == np.nextafter(a, np.float32(2))) | (b == np.nextafter(a, np.float32(-2)))).all(), (key, n)
            S.check_row(row, p)
            n_tab += 1
    assert n_tab == 17


@pytest.mark.parametrize("kind", list(range(9)) + ["small", "shipped"])
def test_shapes_draw_margins_and_rules(kind):
    """For exactly the batches of the GPU test: the share of tables with a decision margin below MARGIN_MIN stays below
    MARGIN_CAP, every restated row passes check_row, the unused tail of every section is zero."""
    from tests import shapes_ref as S
    p = DC.shapes_params(kind)
    left = total = 0
    for seed, rows, margins, devs in DC.shapes_tables(kind):
        left += int((margins < DC.MARGIN_MIN).sum())
        total += len(rows)
        for row in rows:
            S.check_row(row, p)
            assert not row[12:S.BLOBS].any() and not row[S.BLOBS + 4 * int(row[S.NBLOBS]):S.CMDS].any()
            assert not row[S.CMDS + S.CMD_WORDS * int(row[S.NCMDS]):S.VERTS].any()
            assert not row[S.TEX + S.TEX_WORDS * int(row[S.NTEX]):S.POINTS].any() and not row[S.POINTS + 2 * int(row[S.NPOINTS]):].any()
            if int(row[S.PRIM]) != 3:
                assert not row[S.VERTS + 2 * int(row[S.NVERTS]):S.TEX].any()
        if kind in range(9):
            assert (rows[:, S.PRIM] == kind).all()
    print("shapes draw %s: %d tables, %d left out for a margin" % (kind, total, left))
    assert left / total < DC.MARGIN_CAP
    if kind == "small":
        assert set(np.concatenate([r[:, S.PRIM] for _, r, _, _ in DC.shapes_tables(kind)]).tolist()) == set(range(9))


def test_shapes_draw_mutants():
    """Each wrong rule changes a word of at least one compared table (the 32 tables of the primitive it concerns; the
    background's mutants are tried on the polygon's tables)."""
    from tests import shapes_ref as S
    moved = {}
    for m in S.DRAW_MUTANTS:
        kind = S.MUTANT_PRIMITIVE[m] if S.MUTANT_PRIMITIVE[m] is not None else 1
        p = DC.shapes_params(kind)
        d = 0
        for seed, rows, _, _ in DC.shapes_tables(kind):
            for n in range(len(rows)):
                d += int(not np.array_equal(S.draw(seed, n, p, mutant=m)[0], rows[n]))
        moved[m] = d
    print("tables changed by each mutant (of 32):", moved)
    # `stripes without the unique` is an EQUIVALENT mutant: a repeated column has the gap 0 < min_width, so the min-width pass
    # that follows drops it exactly as np.unique would have; no table can tell the two apart while min_width > 0
    assert moved.pop("stripes_no_unique") == 0 and float(DC.shapes_params(6).stripes_min_width_ratio) > 0
    assert all(v > 0 for v in moved.values()), moved


# ------------------------------------------------------------------------------------------------ D the draw logic against the reference
class _StreamState:
    """What datasets/synthetic_dataset.py asks of its random_state, on the device stream: randint(lo[, hi]) truncates its bounds
    like numpy's legacy randint does and maps one uniform to [lo, hi); rand() is one uniform, rand(n) n of them in order."""

    def __init__(self, stream):
        self.s = stream

    def randint(self, lo, hi=None):
        lo, hi = (0, int(lo)) if hi is None else (int(lo), int(hi))
        n = hi - lo
        assert n >= 1, "an empty range: such a table carries deviation (d) and is not compared"
        u = self.s.uniform()
        return lo + min(int(u * n), n - 1)

    def rand(self, *shape):
        return self.s.uniform() if not shape else np.array([self.s.uniform() for _ in range(int(np.prod(shape)))]).reshape(shape)


def test_draw_logic_against_the_reference_itself():
    """The reference's own draw_lines, draw_polygon, draw_ellipses, draw_star and draw_cube, imported in place with a cv2 that only
    records its calls, driven by the device stream of the same (seed, image) positioned where the restatement's primitive
    starts, on a constant image of the restatement's background mean: the recorded commands (endpoints, corners, centres,
    axes, angle, colours, thicknesses) and the returned key points equal the restatement's for every table without a stated
    deviation; fewer than one table in ten carries one."""
    from oracle import ref_harness as RH
    if not RH.available():
        pytest.skip("the reference is not present")
    from semantic_superpoint_amd import lib as L
    from tests import shapes_ref as S
    from tests.pairs_ref import M64, DeviceStream, mix
    mod, rec = RH.synthetic_dataset_recording()
    seed0, B = DC.REFERENCE_BATCH
    total = deviating = compared = 0
    for k in DC.REFERENCE_PRIMITIVES:
        seed = seed0 + k
        p = DC.reference_params(k)
        H, W = int(p.gen_h), int(p.gen_w)
        kwargs = {0: dict(nb_lines=int(p.lines_nb_lines)), 1: dict(max_sides=int(p.polygon_max_sides)), 3: dict(nb_ellipses=int(p.ellipses_nb)),
                  4: dict(nb_branches=int(p.star_nb_branches)),
                  7: dict(min_size_ratio=float(p.cube_min_size_ratio), scale_interval=tuple(float(v) for v in p.cube_scale),
                          trans_interval=tuple(float(v) for v in p.cube_trans))}[k]
        for n in range(B):
            d = S.draw(seed, n, p, deviation_a=True, full=True)
            total += 1
            if d.dev:
                deviating += 1
                continue
            stream = DeviceStream(mix((seed ^ S.SHAPES_TAG) & M64), n)
            stream.ctr = d.start_ctr
            mod.set_random_state(_StreamState(stream))
            del rec.calls[:]
            pts = getattr(mod, L.SHAPES_PRIMITIVES[k])(np.full((H, W), d.bg, np.uint8), **kwargs)
            mine = [(e[0], e[1], e[2], e[3], max(e[4], 1)) if e[0] == "line" else e for e in d.events]
            assert rec.calls == mine, (L.SHAPES_PRIMITIVES[k], n, rec.calls[:3], mine[:3])
            assert stream.ctr == d.rs.ctr, "the reference consumed another number of uniforms"
            mp = d.row[S.POINTS:S.POINTS + 2 * d.npts].view(np.float32).reshape(-1, 2)
            assert np.array_equal(np.asarray(pts, np.float64).reshape(-1, 2), mp.astype(np.float64)), (L.SHAPES_PRIMITIVES[k], n)
            compared += 1
    print("draw logic against the reference: %d tables, %d compared, %d with a stated deviation (share %.3f)" %
          (total, compared, deviating, deviating / total))
    assert deviating / total < 0.1
