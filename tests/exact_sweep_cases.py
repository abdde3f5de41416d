"""The tile-edge sweep of the four teacher-forced, layer-exact chains (not a test module): the case table, and a pure-Python
classifier of the tile-edge classes a configuration reaches in every tile-based kernel family.

The chains (tests/test_gpu_layer_exact.py, test_gpu_backward_exact.py, test_gpu_bf16_path.py::test_bf16_forward_chain_teacher_forced,
test_gpu_bf16_backward_exact.py) extend their parameter lists from SWEEP_CASES; tests/test_exact_sweep_cpu.py runs `launches` over
the old and the new cases for a 256-CU device and asserts what the sweep adds.

The classifier restates the HOST side of the launches: which kernel the dispatch picks (the chains' own mirrors, which every GPU
case asserts against the engine's route record or profiled kernel set), the tile shape launch_conv / launch_wgrad /
launch_conv_bf16 / launch_wgrad_bf16 derive from the map, and how the persistent grids deal their units (the "work assignment"
blocks at the top of the kernels).  Families without spatial tiles are not classified: the row-based first-layer kernels
(conv0_direct_kernel, bn_bwd_*_l0_kernel: grid from an occupancy query) and the pointwise heads (flat pixel lists)."""

# (tag, B, H, W): SSp unless noted; all tensors from seeds, negative / zero BatchNorm scales as in the chains' small cases
SWEEP_CASES = [
    # level maps 16x24, 8x12, 4x6, 2x3: every family gets one partial unit per image, W < 32, H < 8; the smallest pair step (2x3
    # cells, n = 12 per channel on the cell maps)
    ("ssp", 2, 16, 24),
    # 24x256, 12x128, 6x64, 3x32: W % 32 == 0 on all four levels, H % 8 != 0 on level 1, H < 8 on level 2; odd x even cells
    ("ssp", 2, 24, 256),
    # 256x24, 128x12, 64x6, 32x3: the tall twin: 32x8 and 16x8 tiles with a ragged last column; even x odd cells
    ("sp", 2, 256, 24),
    # 88x72, 44x36, 22x18, 11x9: maps of size 2 mod 4 on level 2 (partial F(4x4,3x3) tiles), odd x odd cells, odd batch; the only
    # small case with interior 16x16 tiles (wgrad_bf16_kernel's staging without bounds)
    ("ssp", 3, 88, 72),
    # 40x256, 20x128, 10x64, 5x32, conv checks on the images [0, 1, 24, 46, 47]: on 256 CUs the default predicate sends 40x256 to
    # conv_wino4_kernel (16x32 tile blocks, ragged block row), 20x128 to conv_wino_pipe_kernel (8x32 tiles, H % 8 != 0, the raw
    # pooled copy from a ragged tile row) and the 3x3 heads to the pipe kernel on a 5x32 map (test_exact_sweep_cpu asserts it)
    ("ssp", 48, 40, 256),
]
ARCHS = {"sp": "SuperPointNet_gauss2", "ssp": "SuperPointNet_gauss2_ssmall"}
# (cin, cout) of the 3x3 encoder layers 1 .. 7 (oracle/cpu_ref.py's layer table) and the level of their maps
ENC = {1: (64, 64), 2: (64, 64), 3: (64, 64), 4: (64, 128), 5: (128, 128), 6: (128, 128), 7: (128, 128)}
POOLED = (1, 3, 5)


def _cdiv(a, b):
    return -(-a // b)


def _level(l):
    return 0 if l < 2 else 1 if l < 4 else 2 if l < 6 else 3


def _edge(h, w, th, tw):
    """the tile grid of an h x w map under th x tw tiles"""
    if h < th or w < tw:
        return "map smaller than one tile"
    rr, rc = h % th != 0, w % tw != 0
    return "ragged row and column" if rr and rc else "ragged last row" if rr else "ragged last column" if rc else "full tiles only"


def _parity(h, w):
    return "%s x %s" % ("odd" if h & 1 else "even", "odd" if w & 1 else "even")


def _per_wg(n):
    return "at most one unit per workgroup" if n <= 1 else "several units per workgroup"


def _conv_f32(kernel, direction, layer, h, w, N, nprob, ncob, n_cu):
    """One fp32 3x3 launch (launch_conv of csrc/ssp.hip): tile shape, Winograd tile completeness, units per workgroup of the
    XCD-aware persistent grid (conv_mfma_kernel's work assignment, shared by the Winograd kernels)."""
    if kernel == "wino4":
        wide = _cdiv(h, 16) * 16 * _cdiv(w, 32) * 32 <= _cdiv(h, 32) * 32 * _cdiv(w, 16) * 16   # w4_geometry
        th, tw = (16, 32) if wide else (32, 16)
    elif kernel == "p2":
        wide = w % 16 == 0
        th, tw = (8, 16) if wide else (16, 8)
    else:   # pipe, direct
        wide = w % 32 == 0
        th, tw = (8, 32) if wide else (32, 8)
    cls = {"tile": "%dx%d (%s)" % (th, tw, "wide" if wide else "narrow"), "edge": "%dx%d: %s" % (th, tw, _edge(h, w, th, tw))}
    if kernel == "wino4":
        cls["winograd"] = "partial 4x4 tiles" if h % 4 or w % 4 else "whole 4x4 tiles"
    elif kernel in ("pipe", "p2"):
        cls["winograd"] = "partial 2x2 tiles" if h % 2 or w % 2 else "whole 2x2 tiles"
    nblocks = max(8, ((1 if kernel in ("pipe", "wino4") else 2) * n_cu) // 8 * 8)
    per_cob = max(1, nblocks // 8 // ncob)
    per_t = _cdiv(N * _cdiv(h, th) * _cdiv(w, tw), 8 // nprob)
    cls["units"] = _per_wg(_cdiv(per_t, per_cob))
    if layer >= 6:
        cls["cell map"] = _parity(h, w)
    return {"family": {"wino4": "conv_wino4_kernel", "pipe": "conv_wino_pipe_kernel", "p2": "conv_wino_p2_kernel",
                       "direct": "conv_mfma_kernel"}[kernel], "dir": direction, "layer": layer, "h": h, "w": w, "cls": cls}


def _wgrad_f32(kernel, layer, h, w, N, cin, cout, n_cu):
    """One fp32 weight-gradient launch (launch_wgrad): kernel = fused12 / wino / wino4 / direct"""
    wide = w % 32 == 0
    wino = kernel != "direct"
    th, tw = ((4 if wide else 16) if wino else (2 if wide else 8)), (32 if wide else 8)
    cls = {"tile": "%dx%d (%s)" % (th, tw, "wide" if wide else "narrow"), "edge": "%dx%d: %s" % (th, tw, _edge(h, w, th, tw))}
    if kernel == "wino4":
        cls["winograd"] = "partial 4x4 tiles" if h % 4 or w % 4 else "whole 4x4 tiles"
    pairs = _cdiv(cin, 64) * _cdiv(cout, 32 if kernel == "wino4" else 64)
    ntiles = 2 * N * _cdiv(h, th) * _cdiv(w, tw)
    nsplit = min(max(1, ((1 if wino else 2) * n_cu) // pairs // 8 * 8), ntiles)
    cls["units"] = _per_wg(_cdiv(ntiles, nsplit))
    if layer >= 6:
        cls["cell map"] = _parity(h, w)
    fam = {"fused12": "wgrad_wino_fused_kernel", "wino": "wgrad_wino_kernel", "wino4": "wgrad_wino4_kernel", "direct": "wgrad_mfma_kernel"}
    return {"family": fam[kernel], "dir": "wgrad", "layer": layer, "h": h, "w": w, "cls": cls}


def _conv_bf16(direction, layer, h, w, N, nviews, ncob, n_cu):
    """One 3x3 launch of conv_bf16_ws_kernel (launch_conv_bf16; every 3x3 layer of this network has whole pairs of 32-channel
    chunks): 16x16 tiles, contiguous unit range per XCD, its workgroups interleaved"""
    cls = {"edge": "16x16: %s" % _edge(h, w, 16, 16)}
    units = nviews * ncob * N * _cdiv(h, 16) * _cdiv(w, 16)
    nb = max(8, min(n_cu, _cdiv(units, 8) * 8) // 8 * 8)
    cls["units"] = _per_wg(_cdiv(_cdiv(units, 8), nb // 8))
    if layer >= 6:
        cls["cell map"] = _parity(h, w)
    return {"family": "conv_bf16_ws_kernel", "dir": direction, "layer": layer, "h": h, "w": w, "cls": cls}


def _wgrad_bf16(layer, h, w, N, cin, cout, fuse, n_cu):
    """One 3x3 launch of wgrad_bf16_kernel<.., FUSE> (launch_wgrad_bf16): 16x16 tiles; a tile whose halo lies inside the map
    stages without coordinates or bounds"""
    cls = {"edge": "16x16: %s" % _edge(h, w, 16, 16)}
    cls["tiles"] = ("interior tiles", "border tiles") if h >= 33 and w >= 33 else ("border tiles",)
    ntiles = 2 * N * _cdiv(h, 16) * _cdiv(w, 16)
    nsplit = max(1, min(ntiles, 2 * n_cu // (_cdiv(cin, 64) * _cdiv(cout, 64))))
    cls["units"] = _per_wg(_cdiv(ntiles, nsplit))
    if layer >= 6:
        cls["cell map"] = _parity(h, w)
    return {"family": "wgrad_bf16_kernel<FUSE %d>" % fuse, "dir": "wgrad", "layer": layer, "h": h, "w": w, "cls": cls}


def launches(kind, tag, B, H, W, algo=1, n_cu=256, nprob=2, fuse=1):
    """The tile-based launches one case of a chain checks at rounding level, each with its edge classes.  kind: "f32_fwd" (the
    forward chain), "f32_bwd" (data and weight gradients), "bf16_fwd", "bf16_bwd"; nprob: views per launch (Engine.forward: 1)."""
    from tests.test_gpu_backward_exact import _predict_routes   # (here: the test modules import this one)
    from tests.test_gpu_layer_exact import _kernel
    arch = ARCHS[tag]
    nheads = 3 if tag == "ssp" else 2
    Hc, Wc = H // 8, W // 8
    out = []
    if kind == "f32_fwd":
        for l, (cin, cout) in ENC.items():
            h, w = H >> _level(l), W >> _level(l)
            out.append(_conv_f32(_kernel(algo, l, 3, nprob, B, h, w, cin, cout, n_cu), "forward", l, h, w, B, nprob, _cdiv(cout, 64), n_cu))
        out.append(_conv_f32(_kernel(algo, 8, 3, nprob, B, Hc, Wc, 128, 256 * nheads, n_cu), "forward", 8, Hc, Wc, B, nprob, 4 * nheads, n_cu))
    elif kind == "f32_bwd":
        routes = _predict_routes(arch, algo, B, H, W, n_cu)
        for l, (cin, cout) in ENC.items():
            h, w = H >> _level(l), W >> _level(l)
            out.append(_conv_f32(routes[l][4], "dgrad", l, h, w, B, 2, _cdiv(cin, 64), n_cu))
            out.append(_wgrad_f32(routes[l][3], l, h, w, B, cin, cout, n_cu))
        out.append(_conv_f32(routes[8][4], "dgrad", 8, Hc, Wc, B, 2, 2, n_cu))
        for k in range(nheads):
            out.append(_wgrad_f32(routes[8][3], 8, Hc, Wc, B, 128, 256, n_cu))
    elif kind == "bf16_fwd":
        for l, (cin, cout) in ENC.items():
            h, w = H >> _level(l), W >> _level(l)
            out.append(_conv_bf16("forward", l, h, w, B, nprob, _cdiv(cout, 64), n_cu))
        out.append(_conv_bf16("forward", 8, Hc, Wc, B, nprob, 4 * nheads, n_cu))
    elif kind == "bf16_bwd":
        for l, (cin, cout) in ENC.items():
            h, w = H >> _level(l), W >> _level(l)
            out.append(_conv_bf16("dgrad", l, h, w, B, 2, _cdiv(cin, 64), n_cu))
            apply = bool(fuse) and (l not in POOLED or (h | w) & 1 == 0)   # (the chains' _predict_routes)
            out.append(_wgrad_bf16(l, h, w, B, cin, cout, (2 if l in POOLED else 1) if apply else 0, n_cu))
        out.append(_conv_bf16("dgrad", 8, Hc, Wc, B, 2, 2, n_cu))
        out.append(_wgrad_bf16(8, Hc, Wc, B, 128, 256, 1 if fuse else 0, n_cu))
    else:
        raise KeyError(kind)
    return out


def class_keys(rec):
    """(family, direction, class name, value) of one launch"""
    for name, v in rec["cls"].items():
        for x in (v if isinstance(v, tuple) else (v,)):
            yield (rec["family"], rec["dir"], name, x)
