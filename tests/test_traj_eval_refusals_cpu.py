"""What the five C entry points of the trajectory evaluation (csrc/traj_eval_host.hip.h) answer before they touch a device, in the
convention of csrc/ops_host.hip.h: scalar ranges by name, then null pointers; a refusal returns -1 and a
message that names the faulty argument.  Every call here must be refused ahead of the first launch; its pointers are host memory,
which a call that was let through would hand to a kernel, so the module is skipped where there is a device, as
tests/test_world_upkeep_refusals_cpu.py is."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="a call let through would launch on host pointers: CPU only")

BIG = (1 << 20) + 1
SHARED = ("table", "table_stride", "n_frames", "capacity", "gt", "gt_stride", "n_gt", "index", "skip_flags")
SHARED_BASE = dict(table_stride=8, capacity=8, gt_stride=0, n_gt=8, skip_flags=1, n_problems=2)
SHARED_BAD = [("capacity", (-1, 0, BIG)), ("table_stride", (-1, 0, 7)), ("n_gt", (-1, 0, BIG)), ("gt_stride", (-1, 1, 7)),
              ("skip_flags", (-1,)), ("n_problems", (-1, 0, 65536))]
# entry point -> (its arguments in the header's order, the scalars' good values, the scalars' bad values, the pointers that may be NULL)
ENTRIES = {
    "traj_align": (SHARED + ("mode", "n_problems", "sim", "stream"), dict(SHARED_BASE, mode=1), SHARED_BAD + [("mode", (-1, 4))],
                   ("index", "stream")),
    "traj_ape": (SHARED + ("n_problems", "sim", "err_t", "err_r", "valid", "stream"), SHARED_BASE, SHARED_BAD, ("index", "stream")),
    "traj_rpe_delta": (SHARED + ("n_problems", "scale", "scale_stride", "delta", "err_t", "err_r", "valid", "stream"),
                       dict(SHARED_BASE, scale_stride=16, delta=1), SHARED_BAD + [("delta", (-1, 0, 9)), ("scale_stride", (-1,))],
                       ("index", "scale", "stream")),
    "traj_rpe_segments": (SHARED + ("n_problems", "scale", "scale_stride", "lengths", "n_len", "step", "dist", "seg", "summary", "info",
                                    "stream"),
                          dict(SHARED_BASE, scale_stride=16, n_len=8, step=10),
                          SHARED_BAD + [("n_len", (-1, 0, 9)), ("step", (-1, 0, BIG)), ("scale_stride", (-1,))], ("index", "scale", "stream")),
    "traj_stats": (("err", "valid", "capacity", "n_problems", "stats", "stream"), dict(capacity=8, n_problems=2),
                   [("capacity", (-1, 0, BIG)), ("n_problems", (-1, 0, 65536))], ("stream",)),
}


@pytest.fixture(scope="module")
def lib():
    from semantic_superpoint_amd import lib as L
    return L, L.load_library()


def _call(so, entry, **over):
    """The entry point with every pointer at a host buffer that no refusal reads (NULL where `over` says None) -> (rc, message)"""
    order, base, _, may_be_null = ENTRIES[entry]
    dummy = (C.c_double * 8)()
    args = []
    for name in order:
        if name in base:
            args.append(over.get(name, base[name]))
        else:
            args.append(over.get(name, None if name in may_be_null else C.c_void_p(C.addressof(dummy))))
    rc = getattr(so, "ssp_op_" + entry)(*args)
    assert rc == -1, "every call of this module must be refused ahead of the first launch (got %d)" % rc
    return rc, so.ssp_last_error().decode()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_signature_matches_the_header_order(lib, entry):
    L, _ = lib
    order, base, _, _ = ENTRIES[entry]
    argtypes = L.SIGNATURES["ssp_op_" + entry][0]
    assert len(argtypes) == len(order)
    assert sorted(n for n, t in zip(order, argtypes) if t is C.c_int) == sorted(base)


@pytest.mark.parametrize("entry,name,values", [(e, n, v) for e in ENTRIES for n, v in ENTRIES[e][2]])
def test_scalar_ranges_are_refused_by_name(lib, entry, name, values):
    _, so = lib
    first_pointer = next(n for n in ENTRIES[entry][0] if n not in ENTRIES[entry][1])
    for v in values:
        rc, msg = _call(so, entry, **{name: v})
        assert rc == -1 and msg.startswith(entry + ": ") and name in msg, (entry, name, v, msg)
        # the scalar refusal stands ahead of the pointer test
        rc, msg = _call(so, entry, **{name: v, first_pointer: None})
        assert rc == -1 and name in msg and "null pointer" not in msg, (entry, name, v, msg)


@pytest.mark.parametrize("entry,name", [(e, n) for e in ENTRIES for n in ENTRIES[e][0] if n not in ENTRIES[e][1] and n not in ENTRIES[e][3]])
def test_null_pointers_are_refused(lib, entry, name):
    _, so = lib
    assert _call(so, entry, **{name: None}) == (-1, entry + ": null pointer")


def test_constants_follow_the_header(lib):
    L, _ = lib
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssp_hip.h")).read()
    for name in ("GT_WORDS", "SIM_WORDS", "STATS_WORDS", "INFO_WORDS", "MAX_LENGTHS", "MAX_PROBLEMS"):
        assert int(re.search(r"#define SSP_TRAJ_%s (\d+)" % name, hdr).group(1)) == getattr(L, "TRAJ_" + name), name
    assert re.search(r"#define SSP_TRAJ_MAX_FRAMES \(1 << 20\)", hdr) and L.TRAJ_MAX_FRAMES == 1 << 20
