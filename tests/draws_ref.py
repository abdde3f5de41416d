"""Plain restatement of the kernels that take random decisions on the device, numpy only, no import from the product.
(The photometric draw and noise live in tests/photometric_ref.py, the Synthetic Shapes draw in tests/shapes_ref.py.)

Section "sampler": the index sampler of the sparse descriptor loss (csrc/sem_kernels.hip.h, Engine.sample_indices and
pair_step(indices=None, seed=...)), written from its stated rules:

  matches      cell i = u + v Wc of image `img` is warped with the cell-space matrix in the fp32 operation order of warp_points
               (pairs_ref.warp_points32), rounded half to even, and is VALID when both rounded coordinates are in range
               (sparse_loss.py:184-207).  The valid cells are ordered by the key
                   (splitmix64(seed ^ img << 40 ^ i) >> 33) << 32 | i          ascending,
               the first n_match are taken; position j >= nv (nv = number of valid cells) repeats the sorted position
                   splitmix64(seed ^ 0xA5A5A5A5 ^ img << 40 ^ j) % nv;
               nv == 0 gives zeros.
  non-matches  element i of the flat [B, n_match * n_non] buffer: r = splitmix64(seed ^ 0x5EED5EED ^ i * 0x9E3779B97F4A7C15),
               u1 = (r >> 40) 2^-24, u2 = (r >> 16 & 0xFFFFFF) 2^-24, cell = min(floor(u1 Wc), Wc - 1) + min(floor(u2 Hc), Hc - 1) Wc
               with the two products rounded to float32.

Every index is an integer: the comparison with the device is `==`.  `mutant=` switches ONE rule to a plausible wrong form;
tests/test_draws_ref_cpu.py shows that each of them changes an index of the compared cases (the comparison can see it)."""
import numpy as np

from tests import pairs_ref as R

F32 = np.float32
M64 = R.M64
GOLDEN = 0x9E3779B97F4A7C15
splitmix64 = R.mix   # the device stream's finaliser IS splitmix64's output function of the state x + GOLDEN

MATCH_MUTANTS = ("descending", "low31", "img32", "fill_ncell")
NONMATCH_MUTANTS = ("u2_low24", "hw_swapped")


def splitmix64_np(x):
    """splitmix64 of a uint64 array (numpy's uint64 products wrap modulo 2^64)."""
    with np.errstate(over="ignore"):
        x = x.astype(np.uint64) + np.uint64(GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


# ------------------------------------------------------------------------------------------------ sampler: matches
def cell_grid(Hc, Wc):
    """(u, v) of cell i = u + v Wc, int64 [Hc * Wc, 2]"""
    i = np.arange(Hc * Wc)
    return np.stack((i % Wc, i // Wc), axis=1)


def cell_targets(cell_h_fp32, Hc, Wc):
    """(valid bool [ncell], cell_b int64 [ncell]) of one cell-space matrix, float32 [3, 3]: warp_points32 (product, fma, add and
    the division, each rounded to float32), rint, both coordinates in range.  A NaN or infinite coordinate is not valid."""
    w = R.warp_points32(np.asarray(cell_h_fp32, F32), cell_grid(Hc, Wc))
    with np.errstate(invalid="ignore"):
        ub, vb = np.rint(w[:, 0]), np.rint(w[:, 1])
        valid = (ub >= 0) & (ub <= Wc - 1) & (vb >= 0) & (vb <= Hc - 1)
    cb = np.where(valid, ub + vb * Wc, 0).astype(np.int64)
    return valid, cb


def matches_from_targets(valid, cell_b, seed, img, n_match, mutant=None):
    """The ordering and the fill, from the per-cell validity and target: (match_a, match_b) int32 [n_match]."""
    assert mutant is None or mutant in MATCH_MUTANTS, mutant
    seed, img = int(seed) & M64, int(img)
    ncell = len(valid)
    shift = 32 if mutant == "img32" else 40
    keys = []
    for i in np.nonzero(valid)[0].tolist():
        r = splitmix64(seed ^ ((img << shift) & M64) ^ i)
        r = (r & 0x7FFFFFFF) if mutant == "low31" else (r >> 33)
        keys.append((r << 32) | i)
    keys.sort(reverse=(mutant == "descending"))
    nv = len(keys)
    ma = np.zeros(n_match, np.int32)
    mb = np.zeros(n_match, np.int32)
    if nv == 0:
        return ma, mb
    for j in range(n_match):
        src = j
        if j >= nv:
            src = splitmix64(seed ^ 0xA5A5A5A5 ^ ((img << shift) & M64) ^ j) % (ncell if mutant == "fill_ncell" else nv)
            src = min(src, nv - 1) if mutant == "fill_ncell" else src   # (the mutant must still name a sorted position)
        ma[j] = keys[src] & 0xFFFFFFFF
        mb[j] = cell_b[ma[j]]
    return ma, mb


def sampler_matches(cell_h_fp32, seed, img, Hc, Wc, n_match, mutant=None):
    """(match_a, match_b) int32 [n_match] of image `img` of a batch, from its cell-space matrix (float32 [3, 3])."""
    valid, cb = cell_targets(cell_h_fp32, Hc, Wc)
    return matches_from_targets(valid, cb, seed, img, n_match, mutant)


# ------------------------------------------------------------------------------------------------ sampler: non-matches
def sampler_nonmatches(seed, total, Hc, Wc, mutant=None):
    """int32 [total]: the flat non-match buffer of a whole batch (the element index runs over the batch)."""
    assert mutant is None or mutant in NONMATCH_MUTANTS, mutant
    i = np.arange(total, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = splitmix64_np(np.uint64((int(seed) & M64) ^ 0x5EED5EED) ^ (i * np.uint64(GOLDEN)))
    f1 = r >> np.uint64(40)
    f2 = (r & np.uint64(0xFFFFFF)) if mutant == "u2_low24" else ((r >> np.uint64(16)) & np.uint64(0xFFFFFF))
    u1 = f1.astype(F32) * F32(1.0 / 16777216.0)     # 24 bits: exact in float32
    u2 = f2.astype(F32) * F32(1.0 / 16777216.0)
    nu, nv = (Hc, Wc) if mutant == "hw_swapped" else (Wc, Hc)
    pu, pv = u1 * F32(nu), u2 * F32(nv)
    assert pu.dtype == F32 and pv.dtype == F32
    u = np.minimum(np.floor(pu).astype(np.int64), Wc - 1)
    v = np.minimum(np.floor(pv).astype(np.int64), Hc - 1)
    return (u + v * Wc).astype(np.int32)


# ------------------------------------------------------------------------------------------------ sampler: analytic path
U24 = 2.0 ** -24   # unit roundoff of float32


def analytic_cell_warp64(hn_fp32, Hc, Wc):
    """T^-1 H T in float64 (T = [[2/Wc, 0, -1], [0, 2/Hc, -1], [0, 0, 1]], the float32 entries of H widened exactly) applied to
    the cell centres, and a first-order bound on how far the device's float32 evaluation (pixel_homography_analytic followed by
    warp_point_exact) may lie from it.  Returns (wu, wv, bound) float64 [ncell]; the derivation of `bound` is in the
    docstring of tests/test_gpu_draws_exact.py::test_sampler_analytic_path."""
    h = np.asarray(hn_fp32, F32).astype(np.float64).reshape(3, 3)
    a, b = 2.0 / Wc, 2.0 / Hc
    T = np.array([[a, 0, -1], [0, b, -1], [0, 0, 1]])
    P = np.linalg.inv(T) @ h @ T
    # |error| of the float32 M = H T: columns 0, 1 are h * fl(a): two roundings; column 2 is (-h0 - h1) + h2: two roundings
    ah = np.abs(h)
    eM = np.stack((2 * U24 * ah[:, 0] * a, 2 * U24 * ah[:, 1] * b, 2 * U24 * ah.sum(axis=1)), axis=1)
    M = h @ T
    eP = np.empty((3, 3))
    for c in range(3):   # P0 = (M0 + M2) / fl(a): the sum rounds, fl(a) and the division round
        eP[0, c] = (eM[0, c] + eM[2, c] + U24 * (abs(M[0, c]) + abs(M[2, c]))) / a + 2 * U24 * abs(P[0, c])
        eP[1, c] = (eM[1, c] + eM[2, c] + U24 * (abs(M[1, c]) + abs(M[2, c]))) / b + 2 * U24 * abs(P[1, c])
        eP[2, c] = eM[2, c]
    g = cell_grid(Hc, Wc).astype(np.float64)
    x, y = g[:, 0], g[:, 1]
    rows, erow = [], []
    for r in range(3):   # fl(fl(P1 y + fl(P0 x)) + P2): three roundings of partial sums no larger than the sum of magnitudes
        mag = abs(P[r, 0]) * x + abs(P[r, 1]) * y + abs(P[r, 2])
        rows.append(P[r, 0] * x + P[r, 1] * y + P[r, 2])
        erow.append(eP[r, 0] * x + eP[r, 1] * y + eP[r, 2] + 3 * U24 * mag)
    with np.errstate(divide="ignore", invalid="ignore"):
        wu, wv = rows[0] / rows[2], rows[1] / rows[2]
        z = np.abs(rows[2])
        bu = (erow[0] + np.abs(wu) * erow[2]) / z + U24 * np.abs(wu)
        bv = (erow[1] + np.abs(wv) * erow[2]) / z + U24 * np.abs(wv)
        bound = np.where(erow[2] < 1e-3 * z, np.maximum(bu, bv), np.inf)   # first order holds only for a well-determined z
    return wu, wv, bound


def analytic_targets(hn_fp32, Hc, Wc):
    """(valid, cell_b, decided) of the analytic path from the float64 warp: `decided` marks the cells whose two coordinates lie
    farther than their bound from every rounding tie k + 1/2 (the range limits -1/2 and Wc - 1/2 are such ties).  A cell whose
    bound is not small against 1/2 (|z| near 0) is undecided."""
    wu, wv, bound = analytic_cell_warp64(hn_fp32, Hc, Wc)
    with np.errstate(invalid="ignore"):
        ub, vb = np.rint(wu), np.rint(wv)
        valid = (ub >= 0) & (ub <= Wc - 1) & (vb >= 0) & (vb <= Hc - 1)
        tie = np.minimum(np.abs(np.abs(wu - np.floor(wu)) - 0.5), np.abs(np.abs(wv - np.floor(wv)) - 0.5))
        decided = np.isfinite(bound) & (bound < 0.25) & (tie > bound)
        # far outside the grid every candidate is invalid whatever the rounding: decided although the bound is large
        far = np.isfinite(bound) & ((wu < -0.5 - bound) | (wu > Wc - 0.5 + bound) | (wv < -0.5 - bound) | (wv > Hc - 0.5 + bound))
    decided = decided | (far & ~valid)
    cb = np.where(valid, ub + vb * Wc, 0).astype(np.int64)
    return valid, cb, decided


def check_analytic_matches(ma_dev, mb_dev, hn_fp32, seed, img, Hc, Wc, n_match, max_undecided=6):
    """Position by position: the device's (match_a, match_b) int arrays [n_match] of the analytic path against the restatement.
    The order of match_a depends on the valid SET alone, so with k undecided cells the device's match_a must equal the
    restatement's for one of the 2^k ways to settle them; match_b must equal the float64 target wherever match_a names a
    decided cell.  Returns k."""
    valid, cb, decided = analytic_targets(hn_fp32, Hc, Wc)
    und = np.nonzero(~decided)[0]
    assert len(und) <= max_undecided, ("too many undecided cells", len(und))
    ma_dev, mb_dev = np.asarray(ma_dev).astype(np.int64), np.asarray(mb_dev).astype(np.int64)
    for bits in range(1 << len(und)):
        v = valid.copy()
        v[und] = [(bits >> k) & 1 for k in range(len(und))]
        ma, mb = matches_from_targets(v, cb, seed, img, n_match)
        if np.array_equal(ma, ma_dev):
            if not v.any():
                assert not mb_dev.any(), "nv == 0 leaves zeros"
                return len(und)
            sure = decided[ma_dev]
            assert np.array_equal(mb_dev[sure], mb[sure]), ("match_b differs at a decided cell", img)
            return len(und)
    raise AssertionError("match_a of image %d equals the restatement for no settlement of its %d undecided cells" % (img, len(und)))
