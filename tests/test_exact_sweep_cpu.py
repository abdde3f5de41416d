"""CPU: what the tile-edge sweep of the layer-exact chains covers, asserted from the dispatch mirrors for a 256-CU device.

tests/exact_sweep_cases.py classifies every tile-based launch a chain case checks at rounding level: tile shape, the state of the
tile grid (full tiles only / ragged last row / ragged last column / both / map smaller than one tile), whole or partial Winograd
tiles, parity of the cell map, interior or border tiles of wgrad_bf16_kernel, one unit per workgroup or several.  The test prints
the table (classes x old / new cases: run with -s) and asserts
  * every class the sweep was written for (REQUIRED) is reached by a new case and by no old one;
  * every class the mirror can produce for maps up to 256x256 and batches up to 48 is reached by some case or listed, with its
    reason, in NOT_COVERED."""
import itertools

from tests import exact_sweep_cases as S
from tests import test_gpu_backward_exact as BE
from tests import test_gpu_bf16_backward_exact as BB
from tests import test_gpu_bf16_path as BP
from tests import test_gpu_exact_subbatch as SB
from tests import test_gpu_layer_exact as LE

N_CU = 256
TAGS = {v: k for k, v in S.ARCHS.items()}


def _old_cases():
    out = [("f32_fwd", tag, B, H, W, dict(algo=algo)) for tag, B, H, W, algo, _ in LE.CHAIN_CASES]
    out += [("f32_bwd", tag, B, H, W, dict(algo=algo)) for tag, B, H, W, algo in BE.CASES]
    out += [("bf16_fwd", TAGS[arch], B, H, W, dict(nprob=1)) for arch, H, W, B in BP.FORWARD_CASES]
    out += [("bf16_fwd", "ssp", 32, 240, 320, {})]   # test_bf16_forward_chain_teacher_forced_at_the_benchmark_size
    out += [("bf16_bwd", tag, B, H, W, dict(fuse=fuse)) for tag, B, H, W, fuse in BB.CASES]
    return out


def _new_cases():
    out = [("f32_fwd", tag, B, H, W, dict(algo=algo)) for tag, B, H, W, algo, _ in LE.SWEEP_CHAIN_CASES]
    out += [("f32_bwd", tag, B, H, W, dict(algo=algo)) for tag, B, H, W, algo in BE.SWEEP_BACK_CASES]
    out += [("bf16_fwd", TAGS[arch], B, H, W, dict(nprob=1)) for arch, H, W, B in BP.SWEEP_FORWARD_CASES]
    out += [("bf16_bwd", tag, B, H, W, dict(fuse=fuse)) for tag, B, H, W, fuse in BB.SWEEP_BACK_CASES]
    # tests/test_gpu_exact_subbatch.py: the chains at B = 2 on the engine of 3, the forwards below the configured size
    tag, _, H, W = SB.SUBBATCH_ENGINE
    out += [(k, tag, SB.SUBBATCH_B, H, W, {}) for k in ("f32_fwd", "f32_bwd", "bf16_fwd", "bf16_bwd")]
    out += [(k, SB.FORWARD_ENGINE[0], n, h, w, dict(nprob=1)) for n, h, w in SB.FORWARD_SHAPES for k in ("f32_fwd", "bf16_fwd")]
    return out


def _case_id(c):
    kind, tag, B, H, W, kw = c
    return "%s %s B%d %dx%d%s" % (kind, tag, B, H, W, "".join(" %s%s" % kv for kv in sorted(kw.items())))


def _coverage(cases):
    """{(family, direction, class, value): [case ids]}"""
    cov = {}
    for c in cases:
        kind, tag, B, H, W, kw = c
        for rec in S.launches(kind, tag, B, H, W, n_cu=N_CU, **kw):
            for key in S.class_keys(rec):
                ids = cov.setdefault(key, [])
                if _case_id(c) not in ids:
                    ids.append(_case_id(c))
    return cov


def _universe():
    """every class the mirror produces: maps up to 256x256 (multiples of 8), batches up to 48, both models, every algorithm a
    chain runs, one and two views per forward launch"""
    seen = set()
    sizes = range(8, 257, 8)
    kinds = [("f32_fwd", dict(algo=a, nprob=p)) for a in (0, 1, 10) for p in (1, 2)]
    kinds += [("f32_bwd", dict(algo=a)) for a in (0, 1, 10, 11)]
    kinds += [("bf16_fwd", dict(nprob=p)) for p in (1, 2)] + [("bf16_bwd", dict(fuse=f)) for f in (0, 1)]
    for (kind, kw), tag, B in itertools.product(kinds, ("sp", "ssp"), (1, 2, 3, 8, 24, 48)):
        for H in sizes:
            for W in sizes:
                for rec in S.launches(kind, tag, B, H, W, n_cu=N_CU, **kw):
                    seen.update(S.class_keys(rec))
    return seen


# what the sweep was written for: (family, direction, class, value); each must be reached by a new case and by no old one
PIPE, P2, W4, MFMA = "conv_wino_pipe_kernel", "conv_wino_p2_kernel", "conv_wino4_kernel", "conv_mfma_kernel"
WS, WGB = "conv_bf16_ws_kernel", "wgrad_bf16_kernel<FUSE %d>"
REQUIRED = [
    # W % 32 == 0 below the first pyramid level: the 8x32 tile of the pipe kernel (the 3x3 heads at 5x32; level 2 stays on the
    # 8x16 tile of the p2 kernel at every swept batch: NOT_COVERED has no entry for it because the class is per kernel, not per level),
    # the 8x16 tile of the p2 kernel on 6x64 / 3x32, 8x32 tiles with H % 8 != 0
    (PIPE, "forward", "edge", "8x32: map smaller than one tile"),
    (P2, "forward", "edge", "8x16: map smaller than one tile"), (P2, "dgrad", "edge", "8x16: map smaller than one tile"),
    (PIPE, "forward", "edge", "8x32: ragged last row"), (PIPE, "dgrad", "edge", "8x32: ragged last row"),
    (MFMA, "forward", "edge", "8x32: ragged last row"), (MFMA, "dgrad", "edge", "8x32: ragged last row"),
    ("wgrad_wino_fused_kernel", "wgrad", "edge", "4x32: ragged last row"),
    # the tall twin: a ragged last column of the narrow tiles
    (P2, "forward", "edge", "16x8: ragged last column"), (P2, "dgrad", "edge", "16x8: ragged last column"),
    (MFMA, "forward", "edge", "32x8: ragged last column"), ("wgrad_wino_fused_kernel", "wgrad", "edge", "16x8: ragged last column"),
    # cell maps odd in one direction only
    ("wgrad_mfma_kernel", "wgrad", "cell map", "odd x even"), ("wgrad_mfma_kernel", "wgrad", "cell map", "even x odd"),
    ("wgrad_wino4_kernel", "wgrad", "cell map", "even x odd"),
    (P2, "forward", "cell map", "odd x even"), (P2, "forward", "cell map", "even x odd"),
    (P2, "dgrad", "cell map", "odd x even"), (P2, "dgrad", "cell map", "even x odd"),
    (PIPE, "forward", "cell map", "odd x even"), (PIPE, "forward", "winograd", "partial 2x2 tiles"),
    # maps smaller than one tile block (the rest of the families: the old 40x56 and 64x96 cases reach theirs at 5x7 / 8x12)
    (MFMA, "forward", "edge", "8x32: map smaller than one tile"), (W4, "forward", "edge", "32x16: map smaller than one tile"),
    (W4, "dgrad", "edge", "32x16: map smaller than one tile"), ("wgrad_wino_kernel", "wgrad", "edge", "16x8: map smaller than one tile"),
    (WGB % 2, "wgrad", "edge", "16x16: map smaller than one tile"),
    # partial F(4x4,3x3) tiles (4x6, 6x64, 22x18 ...), forward, data gradient and the F(3x3,4x4) weight gradient
    (W4, "forward", "winograd", "partial 4x4 tiles"), (W4, "dgrad", "winograd", "partial 4x4 tiles"),
    ("wgrad_wino4_kernel", "wgrad", "winograd", "partial 4x4 tiles"),
    (W4, "forward", "edge", "16x32: ragged row and column"), (W4, "forward", "edge", "32x16: ragged row and column"),
    # the bf16 kernels on those widths
    (WS, "forward", "cell map", "even x odd"), (WS, "dgrad", "cell map", "odd x even"), (WS, "dgrad", "cell map", "even x odd"),
    (WGB % 1, "wgrad", "cell map", "odd x even"), (WGB % 1, "wgrad", "cell map", "even x odd"),
    (WGB % 2, "wgrad", "edge", "16x16: ragged last column"), (WGB % 0, "wgrad", "edge", "16x16: ragged row and column"),
]
# (conv_wino4_kernel under the DEFAULT predicate with a ragged tile-block row is not in REQUIRED: the 120x160 level of the old
# B = 32 cases is already "16x32: ragged last row" (120 = 7.5 x 16); the 40x256 level of the fifth case is a second, cheaper one.)

# classes the mirror can produce (maps up to 256x256, B up to 48) that no case of the chains reaches, each with its reason
_R_ALGO0_UNITS = ("needs more than 64 tiles per view and XCD slice under algorithm 0 (512 workgroups): only the B >= 32 cases are that "
                  "large, and they run the default algorithm")
_R_W4_COL = ("a ragged last block column alone needs W % 32 (W % 16) != 0 with H a multiple of the block height, e.g. 64x72; the "
             "sweep has the column bound only together with the row bound (88x72, 44x36: ragged row and column)")
_R_PIPE_NARROW = ("the 32x8 tile of the pipe kernel needs >= 1024 first-generation items on a map with W % 32 != 0: the 240x320 cases "
                  "reach it at 120x160 / 30x40 in the states listed as covered; every further state of that grid needs another "
                  "B >= 32 case at a size with W % 32 != 0, about the cost of the fifth case again")
_R_PIPE_CELLS = "the 3x3 heads reach the pipe kernel only at B >= 32; the one such swept case has 5x32 cells (odd x even)"
_R_FUSE0 = ("the separate APPLY pass (SSP_BF16_FUSE_APPLY=0) runs at 64x96 and, in the sweep, at 88x72 only; the tile code of "
            "wgrad_bf16_kernel<FUSE 0> is the one FUSE 1 / 2 run on every other case")
_R_FUSE1_FULL = ("FUSE 1 (the unpooled layers: levels 1 .. 3) has a full or column-ragged 16x16 grid only when H % 32 == 0: among the "
                 "fused cases only 256x24, whose level maps are narrower than a tile; the same grid states run as FUSE 2 on level 0 "
                 "and as FUSE 0 at 64x96")
_R_WG_DIRECT = ("a 2x32 tile larger than the map needs a 1-row cell map with Wc % 32 == 0 (8x256 images); a row-ragged 8x8 grid needs "
                "W % 8 == 0, W % 32 != 0 and H % 8 != 0 on a map this kernel takes (algorithm 0, or odd cells), e.g. 12x8 cells: no "
                "case has either")
_R_WGF_SMALL = "needs a 2-row even map with W % 32 == 0 (level 2 of an 8x128 image); no case has it"
_R_A11_ONE_TILE = ("under algorithm 11 a map inside one 128-pixel block tile keeps algorithm 1's weight gradient (launch_wgrad): the "
                   "plain wgrad_wino_kernel sees only such maps, of which the sweep has the 4x6 one (B = 2); wgrad_wino4_kernel keeps a "
                   "4x32 tile larger than the map, or odd x even cells, only beyond one tile, e.g. a 2x64 level (8x256 images) or 17x8 "
                   "cells (136x64): no case has them")
NOT_COVERED = {
    ("wgrad_wino4_kernel", "wgrad", "cell map", "odd x even"): _R_A11_ONE_TILE,
    ("wgrad_wino4_kernel", "wgrad", "edge", "4x32: map smaller than one tile"): _R_A11_ONE_TILE,
    ("wgrad_wino_kernel", "wgrad", "cell map", "even x even"): _R_A11_ONE_TILE,
    ("wgrad_wino_kernel", "wgrad", "edge", "16x8: full tiles only"): _R_A11_ONE_TILE,
    ("wgrad_wino_kernel", "wgrad", "edge", "4x32: full tiles only"): _R_A11_ONE_TILE,
    ("wgrad_wino_kernel", "wgrad", "edge", "4x32: map smaller than one tile"): _R_A11_ONE_TILE,
    ("wgrad_wino_kernel", "wgrad", "tile", "4x32 (wide)"): _R_A11_ONE_TILE,
    ("wgrad_wino_kernel", "wgrad", "units", "several units per workgroup"): _R_A11_ONE_TILE,
    (MFMA, "forward", "units", "several units per workgroup"): _R_ALGO0_UNITS,
    (MFMA, "dgrad", "units", "several units per workgroup"): _R_ALGO0_UNITS,
    (W4, "forward", "edge", "16x32: ragged last column"): _R_W4_COL, (W4, "forward", "edge", "32x16: ragged last column"): _R_W4_COL,
    (W4, "dgrad", "edge", "16x32: ragged last column"): _R_W4_COL, (W4, "dgrad", "edge", "32x16: ragged last column"): _R_W4_COL,
    (PIPE, "dgrad", "edge", "32x8: full tiles only"): _R_PIPE_NARROW, (PIPE, "dgrad", "edge", "32x8: map smaller than one tile"): _R_PIPE_NARROW,
    (PIPE, "dgrad", "edge", "32x8: ragged last column"): _R_PIPE_NARROW, (PIPE, "dgrad", "edge", "32x8: ragged row and column"): _R_PIPE_NARROW,
    (PIPE, "forward", "edge", "32x8: full tiles only"): _R_PIPE_NARROW, (PIPE, "forward", "edge", "32x8: ragged last column"): _R_PIPE_NARROW,
    (PIPE, "forward", "edge", "32x8: ragged last row"): _R_PIPE_NARROW, (PIPE, "forward", "edge", "32x8: ragged row and column"): _R_PIPE_NARROW,
    (PIPE, "forward", "cell map", "even x odd"): _R_PIPE_CELLS, (PIPE, "forward", "cell map", "odd x odd"): _R_PIPE_CELLS,
    (WGB % 0, "wgrad", "cell map", "even x odd"): _R_FUSE0, (WGB % 0, "wgrad", "cell map", "odd x even"): _R_FUSE0,
    (WGB % 0, "wgrad", "edge", "16x16: ragged last row"): _R_FUSE0, (WGB % 0, "wgrad", "units", "several units per workgroup"): _R_FUSE0,
    (WGB % 1, "wgrad", "edge", "16x16: full tiles only"): _R_FUSE1_FULL, (WGB % 1, "wgrad", "edge", "16x16: ragged last column"): _R_FUSE1_FULL,
    ("wgrad_mfma_kernel", "wgrad", "edge", "2x32: map smaller than one tile"): _R_WG_DIRECT,
    ("wgrad_mfma_kernel", "wgrad", "edge", "8x8: ragged last row"): _R_WG_DIRECT,
    ("wgrad_wino_fused_kernel", "wgrad", "edge", "4x32: map smaller than one tile"): _R_WGF_SMALL,
}


def test_the_fifth_case_reaches_its_three_kernels_on_256_cus():
    """(ssp, 48, 40, 256) under the default predicate: 40x256 on conv_wino4_kernel with a ragged 16x32 block row, 20x128 on
    conv_wino_pipe_kernel (8x32 tiles, H % 8 != 0) which also writes the raw pooled copy, the 3x3 heads on the pipe kernel at 5x32"""
    tag, B, H, W = S.SWEEP_CASES[4]
    assert (B, H, W) == (48, 40, 256)
    assert LE._kernel(1, 1, 3, 2, B, 40, 256, 64, 64, N_CU) == "wino4"
    assert LE._kernel(1, 2, 3, 2, B, 20, 128, 64, 64, N_CU) == "pipe" and LE._kernel(1, 3, 3, 2, B, 20, 128, 64, 64, N_CU) == "pipe"
    assert LE._kernel(1, 8, 3, 2, B, 5, 32, 128, 768, N_CU) == "pipe"
    recs = {r["layer"]: r for r in S.launches("f32_fwd", tag, B, H, W, algo=1, n_cu=N_CU)}
    assert recs[1]["cls"]["edge"] == "16x32: ragged last row"
    assert recs[3]["cls"]["edge"] == "8x32: ragged last row"
    assert recs[8]["cls"]["edge"] == "8x32: map smaller than one tile"


def test_sweep_coverage_table():
    old, new = _coverage(_old_cases()), _coverage(_new_cases())
    universe = _universe()
    assert set(old) <= universe and set(new) <= universe
    print("\nfamily | direction | class | value | old cases | new cases   (n_cu = %d)" % N_CU)
    for key in sorted(universe):
        mark = "NOT COVERED: " + NOT_COVERED[key] if key in NOT_COVERED else ""
        print("%s | %s | %s | %s | %d | %d %s%s" % (key + (len(old.get(key, ())), len(new.get(key, ())),
                                                 "" if key in old or key not in new else "[new: %s]" % new[key][0], mark)))
    for key in REQUIRED:
        assert key in new and key not in old, (key, "old cases", old.get(key), "new cases", new.get(key))
    missing = sorted(k for k in universe if k not in old and k not in new and k not in NOT_COVERED)
    assert not missing, ("classes no case reaches and NOT_COVERED does not list", missing)
    stale = sorted(k for k in NOT_COVERED if k in old or k in new or k not in universe)
    assert not stale, ("NOT_COVERED lists classes that are covered or cannot occur", stale)
