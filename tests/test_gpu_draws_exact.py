"""GPU: the kernels that take random decisions on the device, index by index against the plain restatement tests/draws_ref.py.

Index sampler (csrc/sem_kernels.hip.h: sample_matches_kernel, sample_nonmatches_kernel): every index is an integer, the
comparison is torch.equal over the whole buffers.  tests/test_draws_ref_cpu.py pins the restatement (the oracle's cell
correspondences, published splitmix64 outputs, mutants) and shows that the share the analytic path may leave out stays
inside its cap for exactly these cases (tests/draws_cases.py).

Photometric draw and per-pixel noise (csrc/photo_kernels.hip.h: photo_draw_kernel, stages 4 and 5 of photo_point) against
tests/photometric_ref.py::draw / noise: the rows column by column, the noisy images level by level.

Synthetic Shapes draw (csrc/shapes_kernels.hip.h: shapes_draw_kernel, sh_draw_primitive, sh_sample_polygon, ShWarp) against
tests/shapes_ref.py::draw: the scene tables word by word."""
import numpy as np
import pytest
import torch

from tests import draws_cases as DC
from tests import draws_ref as D

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _sampler_engine(name):
    from semantic_superpoint_amd.lib import Engine
    H, W, seed = DC.SAMPLER_CASES[name]
    return Engine("SuperPointNet_gauss2", DC.SAMPLER_B, H, W, _dev(), with_grad=False), H // 8, W // 8, seed


# ------------------------------------------------------------------------------------------------ A index sampler
@pytest.mark.parametrize("name", list(DC.SAMPLER_CASES))
def test_sampler_host_scaled_every_index(name):
    """Engine.sample_indices with the reference's cell-space matrices: match_a, match_b and nonmatch_b equal the restatement in
    full, position by position: which cells are chosen, in which order (the bitonic sort of 2048 / 8192 keys), the fill with
    replacement where nv < n_match, the zeros of nv == 0, and every single non-match."""
    e, Hc, Wc, seed = _sampler_engine(name)
    hs, ch = DC.sampler_homographies(name), DC.cell_homographies(name)
    ma, mb, nm = e.sample_indices(t(hs).to(_dev()), seed=seed, cell_homographies=t(ch))
    torch.cuda.synchronize()
    ref = [D.sampler_matches(ch[b], seed, b, Hc, Wc, DC.N_MATCH) for b in range(DC.SAMPLER_B)]
    ra, rb = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    rn = D.sampler_nonmatches(seed, DC.SAMPLER_B * DC.N_MATCH * DC.N_NON, Hc, Wc).reshape(DC.SAMPLER_B, -1)
    eq = (torch.equal(ma.cpu(), t(ra)), torch.equal(mb.cpu(), t(rb)), torch.equal(nm.cpu(), t(rn)))
    print("sampler %s host-scaled: compared %d match pairs and %d non-matches, left out 0, bit-equal %s" %
          (name, ra.size, rn.size, eq))
    assert ma.dtype == torch.int32 and nm.dtype == torch.int32
    assert eq[0], ("match_a", int((ma.cpu() != t(ra)).sum()))
    assert eq[1], ("match_b", int((mb.cpu() != t(rb)).sum()))
    assert eq[2], ("nonmatch_b", int((nm.cpu() != t(rn)).sum()))


@pytest.mark.parametrize("name", list(DC.SAMPLER_CASES))
def test_sampler_analytic_path(name):
    """Engine.sample_indices without host matrices: the device derives T^-1 H T itself (pixel_homography_analytic) in float32.
    Reference: the same product in float64 (draws_ref.analytic_cell_warp64).  A cell is compared unless a warped coordinate
    lies within `bound` of a rounding tie k + 1/2 (the range limits -1/2 and Wc - 1/2 are such ties).  Derivation of `bound`,
    u = 2^-24, first order, for ANY association or contraction of the written operations (an fma only removes a rounding):
      a = fl(2 / Wc): relative u.   M[r][0] = fl(h a): 2 u |h a|;  M[r][2] = fl(fl(-h0 - h1) + h2): 2 u (|h0| + |h1| + |h2|).
      P[0][c] = fl(fl(M0c + M2c) / a): (eM0c + eM2c + u (|M0c| + |M2c|)) / a + 2 u |P0c|  - the division by a = 2 / Wc is what
      scales absolute errors of order u up by Wc / 2.   P[2][c] = M[2][c].
      X = fl(fl(P1 y + fl(P0 x)) + P2): eP0 x + eP1 y + eP2 + 3 u (|P0| x + |P1| y + |P2|); the same for Y and Z.
      wu = fl(X / Z): (eX + |wu| eZ) / |Z| + u |wu|.
    At these magnitudes (coordinates up to 80, |P2| up to 80, Z near 1) that is 1e-5 (8x12 cells) to 1.4e-4 (60x80 cells); a cell
    whose Z is not determined to 1e-3 relative counts as undecided.  The CPU test shows the uncontracted float32 evaluation at
    a fifth of the bound and the undecided share below MARGIN_CAP.  With k undecided cells in an image match_a must equal the
    restatement for one of the 2^k settlements, and match_b at every decided cell (draws_ref.check_analytic_matches).
    The non-matches do not depend on the matrices: equal in full."""
    e, Hc, Wc, seed = _sampler_engine(name)
    hs = DC.sampler_homographies(name)
    ma, mb, nm = e.sample_indices(t(hs).to(_dev()), seed=seed)
    torch.cuda.synchronize()
    ma, mb = ma.cpu().numpy(), mb.cpu().numpy()
    left = [int((~D.analytic_targets(hs[b], Hc, Wc)[2]).sum()) for b in range(DC.SAMPLER_B)]
    rn = D.sampler_nonmatches(seed, DC.SAMPLER_B * DC.N_MATCH * DC.N_NON, Hc, Wc).reshape(DC.SAMPLER_B, -1)
    share = sum(left) / (DC.SAMPLER_B * Hc * Wc)
    print("sampler %s analytic: compared %d cells and %d non-matches, left out %d cells for the margin (share %.2e), non-matches "
          "bit-equal %s" % (name, DC.SAMPLER_B * Hc * Wc - sum(left), rn.size, sum(left), share, torch.equal(nm.cpu(), t(rn))))
    assert share < DC.MARGIN_CAP
    assert torch.equal(nm.cpu(), t(rn))
    assert left == [D.check_analytic_matches(ma[b], mb[b], hs[b], seed, b, Hc, Wc, DC.N_MATCH) for b in range(DC.SAMPLER_B)]
    print("sampler %s analytic: match_a equals the restatement for a settlement of the undecided cells, match_b at every decided cell" % name)


# ------------------------------------------------------------------------------------------------ B photometric draw and noise
def _photo_struct(L, p):
    import ctypes
    s = L.SspPhotometricParams()
    s.struct_size = ctypes.sizeof(L.SspPhotometricParams)
    s.random_brightness, s.random_contrast, s.additive_gaussian_noise = p["brightness"], p["contrast"], p["noise"]
    s.additive_speckle_noise, s.motion_blur, s.additive_shade = p["impulse"], p["motion_blur"], p["shade"]
    s.brightness_max_abs_change = p["max_abs_change"]
    s.contrast_lo, s.contrast_hi, s.noise_std_lo, s.noise_std_hi = p["contrast_lo"], p["contrast_hi"], p["std_lo"], p["std_hi"]
    s.impulse_prob_lo, s.impulse_prob_hi = p["p_lo"], p["p_hi"]
    s.shade_nb_ellipses, s.shade_transparency_lo, s.shade_transparency_hi = p["nb_ellipses"], p["t_lo"], p["t_hi"]
    s.shade_kernel_lo, s.shade_kernel_hi = p["ksize_lo"], p["ksize_hi"]
    return s


@pytest.mark.parametrize("hw", DC.PHOTO_SIZES)
@pytest.mark.parametrize("name", list(DC.photo_param_sets()))
def test_photometric_draw_every_column(name, hw):
    """ssp_op_photometric_draw, 300 rows (five blocks of 64, the last partly filled), the shipped block and each primitive off
    in turn (an off primitive writes its neutral values and consumes no uniform, so every later column moves up the stream):
    every column `==` as float32 - the ellipse angle too, one product in double cast once - except the nine blur weights,
    float(k_i / sum) from double cos / sin, which must equal the restatement's value or its float32 neighbour.  Rows whose
    smallest decision margin is below MARGIN_MIN are left out (none for this seed: tests/test_draws_ref_cpu.py)."""
    from semantic_superpoint_amd import lib as L
    from tests import photometric_ref as P
    H, W = hw
    ref, margin, _ = DC.photo_rows(name, H, W)
    got = L.op_photometric_draw(DC.PHOTO_B, H, W, DC.PHOTO_SEED, _photo_struct(L, DC.photo_param_sets()[name]), _dev()).cpu().numpy()
    keep = margin >= DC.MARGIN_MIN
    wcols = np.zeros(P.STRIDE, bool)
    wcols[P.BLUR_W:P.BLUR_W + 9] = True
    exact = np.array_equal(got[keep][:, ~wcols], ref[keep][:, ~wcols])
    gw, rw = got[keep][:, wcols], ref[keep][:, wcols]
    near = (gw == np.nextafter(rw, np.float32(2))) | (gw == np.nextafter(rw, np.float32(-2)))
    print("photometric draw %-15s %dx%d: compared %d rows x %d columns, left out %d rows for a margin, bit-equal %s; weights: %d "
          "compared, %d equal, %d the float32 neighbour" % (name, H, W, int(keep.sum()), P.STRIDE, int((~keep).sum()),
                                                            exact and bool((gw == rw).all()), gw.size, int((gw == rw).sum()), int(near.sum())))
    assert (~keep).mean() < DC.MARGIN_CAP
    bad = np.argwhere(got[keep][:, ~wcols] != ref[keep][:, ~wcols])
    assert exact, ("first differing (row, column of the non-weight columns)", bad[:5].tolist())
    assert ((gw == rw) | near).all()


@pytest.mark.parametrize("hw", DC.NOISE_SIZES)
def test_photometric_noise_every_pixel(hw):
    """ssp_op_photometric_apply with stages 4 and 5: sigma 10 alone, p = 0.0035 alone, both, both under the 3x3 blur, both after
    contrast 1.4, and sigma 10 on an image of 0 and 1 (both clips); six keys per case, three drawn and three hand-made (one with
    all four 16-bit words above 32767).  Every pixel outside the tie set equals the float64 restatement's level exactly;
    a pixel of the tie set (pre-rounding value within NOISE_TAU * base of a .5 boundary; under the blur: such a pixel in the
    3x3 neighbourhood) may differ by one level.  NOISE_TAU = 4 x the measured ratio (photometric_ref.NOISE_MEASURED)."""
    from semantic_superpoint_amd import lib as L
    from tests import photometric_ref as P
    H, W = hw
    for name, (img, rows) in DC.noise_cases(H, W).items():
        x = torch.from_numpy(img).view(1, 1, H, W).repeat(len(rows), 1, 1, 1).contiguous().to(_dev())
        got = L.op_photometric_apply(x, t(rows).to(_dev())).cpu().numpy()[:, 0]
        ref, may = zip(*[P.apply(img, r, tau=P.NOISE_TAU) for r in rows])
        ref, may = np.stack(ref).astype(np.float32), np.stack(may)
        equal = got == ref
        print("photometric noise %dx%d %-14s compared %d pixels, left out %d for a tie, bit-equal %s (inside the tie set %d differ)" %
              (H, W, name, int((~may).sum()), int(may.sum()), bool(equal[~may].all()), int((~equal[may]).sum())))
        assert may.mean() < (9 if rows[0][P.BLUR_FLAG] else 1) * DC.MARGIN_CAP, name
        assert equal[~may].all(), (name, int((~equal[~may]).sum()))
        assert (np.abs(got.astype(np.float64) - ref)[may] <= 1 / 255 + 1e-7).all(), name
        assert len({got[b].tobytes() for b in range(len(rows))}) == len(rows), name     # another key, another noise


# ------------------------------------------------------------------------------------------------ C Synthetic Shapes draw
@pytest.mark.parametrize("kind", list(range(9)) + ["small", "shipped"])
def test_shapes_draw_every_word(kind):
    """ssp_op_shapes_draw against tests/shapes_ref.py::draw: 32 tables of each primitive alone and a mixed batch of 256 at the
    small size (192x256), a mixed batch of 64 at the shipped 960x1280.  Every int32 word of the row `==` (the unused tails are
    zeros), the float-bit words included - key points, texture radius, 1/ax^2 and 1/ay^2 are exact - except the ellipses' cos and
    sin, casts of a double libm result, which may be the float32 neighbour.  Tables whose smallest decision margin is below
    MARGIN_MIN are left out (none for these seeds: tests/test_draws_ref_cpu.py)."""
    from semantic_superpoint_amd import lib as L
    from tests import shapes_ref as S
    p = DC.shapes_params(kind)
    n_tab = left = n_float = n_near = 0
    equal = True
    for seed, rows, margins, _ in DC.shapes_tables(kind):
        got = L.op_shapes_draw(len(rows), seed, p, _dev()).cpu().numpy()
        for n in range(len(rows)):
            if margins[n] < DC.MARGIN_MIN:
                left += 1
                continue
            n_tab += 1
            fw = S.float_words(rows[n])
            plain = np.ones(S.ROW, bool)
            plain[fw] = False
            same = np.array_equal(got[n][plain], rows[n][plain])
            equal &= same and np.array_equal(got[n][fw], rows[n][fw])
            assert same, (kind, seed, n, "first differing words", np.nonzero(got[n] != rows[n])[0][:8].tolist())
            a, b = rows[n][fw].view(np.float32), got[n][fw].view(np.float32)
            near = (b == np.nextafter(a, np.float32(2))) | (b == np.nextafter(a, np.float32(-2)))
            n_float += len(fw)
            n_near += int(near.sum())
            assert ((a == b) | near).all(), (kind, seed, n)
    print("shapes draw %-7s compared %d tables x %d words, left out %d for a margin, bit-equal %s (%d cos / sin words, %d the float32 "
          "neighbour)" % (kind, n_tab, S.ROW, left, equal, n_float, n_near))
    assert left / (n_tab + left) < DC.MARGIN_CAP
