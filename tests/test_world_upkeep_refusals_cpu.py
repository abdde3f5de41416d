"""What the two C entry points of the world map's upkeep (csrc/world_upkeep_host.hip.h) answer before they touch a device, in the
convention of csrc/ops_host.hip.h: the family check, then scalar ranges, then null pointers, then the fields
of the parameter struct; a refusal returns -1 (a byte count: 0) and a message that names the faulty argument.  Every call here must be
refused ahead of the first launch; its pointers are host memory, which a call that was let through would hand to a kernel, so the
module is skipped where there is a device, as tests/test_c_refusals_cpu.py is."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="a call let through would launch on host pointers: CPU only")

BASE = dict(cap=8, row_cap=8, pt_stride=2, point_cap=4, capacity=4, n_frames=3, map_cap=8, tid_cap=16)
ORDER = ("match", "n_match", "cap", "landmarks", "n_landmarks", "row_cap", "pts_new", "pt_stride", "count_new", "point_cap", "table",
         "capacity", "n_frames", "intr", "params", "map_cap", "tid_cap", "x", "desc", "tid", "views", "first", "last", "rms", "slot_of_tid",
         "state", "report", "totals", "workspace", "stream")
MAY_BE_NULL = ("totals", "stream")
BIG = (1 << 30) + 1


@pytest.fixture(scope="module")
def lib():
    from semantic_superpoint_amd import lib as L
    return L, L.load_library()


def _call(L, lib, struct=None, **over):
    """ssp_op_world_upkeep with every pointer at a host buffer that no refusal reads (NULL where `over` says None) -> (rc, message)"""
    dummy = (C.c_double * 8)()
    prm = struct if struct is not None else L.SspWorldUpkeepParams(1, 2.0, 4, 3, 6, 4)
    args = []
    for name in ORDER:
        if name in BASE:
            args.append(over.get(name, BASE[name]))
        elif name == "params":
            args.append(over.get(name, C.c_void_p(C.addressof(prm))))
        else:
            args.append(over.get(name, None if name in MAY_BE_NULL else C.c_void_p(C.addressof(dummy))))
    rc = lib.ssp_op_world_upkeep(*args)
    assert rc == -1, "every call of this module must be refused ahead of the first launch (got %d)" % rc
    return rc, lib.ssp_last_error().decode()


def test_signature_matches_the_header_order(lib):
    L, _ = lib
    argtypes = L.SIGNATURES["ssp_op_world_upkeep"][0]
    assert len(argtypes) == len(ORDER)
    assert [n for n, t in zip(ORDER, argtypes) if t is C.c_int] == list(BASE)


@pytest.mark.parametrize("name,values", [("cap", (-1, 0, BIG)), ("map_cap", (-1, 0, BIG)), ("point_cap", (-1, 0, BIG)),
                                         ("pt_stride", (-1, 0, 1)), ("row_cap", (-1, 0, BIG)), ("tid_cap", (-1, 0)), ("capacity", (-1,)),
                                         ("n_frames", (-1,))])
def test_scalar_ranges_are_refused_by_name(lib, name, values):
    L, so = lib
    for v in values:
        rc, msg = _call(L, so, **{name: v})
        assert rc == -1 and msg.startswith("world_upkeep: ") and name in msg, (name, v, msg)
        # the scalar refusal stands ahead of the pointer test
        rc, msg = _call(L, so, match=None, **{name: v})
        assert rc == -1 and name in msg and "null pointer" not in msg, (name, v, msg)


@pytest.mark.parametrize("name", [n for n in ORDER if n not in BASE and n not in MAY_BE_NULL])
def test_null_pointers_are_refused(lib, name):
    L, so = lib
    assert _call(L, so, **{name: None}) == (-1, "world_upkeep: null pointer")


def test_a_table_may_be_null_only_without_rows(lib):
    L, so = lib
    bad = L.SspWorldUpkeepParams(1, -1.0, 4, 3, 6, 4)       # (a struct fault, so that the accepted pointer test still ends in a refusal)
    rc, msg = _call(L, so, struct=bad, table=None, capacity=0)
    assert rc == -1 and "merge_thresh" in msg
    assert _call(L, so, struct=bad, table=None, capacity=4) == (-1, "world_upkeep: null pointer")


@pytest.mark.parametrize("fields,word", [((1, -1.0, 4, 3, 6, 4), "merge_thresh"), ((1, float("nan"), 4, 3, 6, 4), "merge_thresh"),
                                         ((1, float("inf"), 4, 3, 6, 4), "merge_thresh"), ((0, 2.0, 4, 3, 3, 4), "low_water"),
                                         ((0, 2.0, 4, 3, 9, 4), "high_water"), ((0, 2.0, 4, 3, 6, -1), "low_water")])
def test_parameter_struct_is_refused_by_field(lib, fields, word):
    L, so = lib
    rc, msg = _call(L, so, struct=L.SspWorldUpkeepParams(*fields))
    assert rc == -1 and word in msg, msg


def test_workspace_bytes(lib):
    """0 and a message for a bad map_cap; else the stated layout: the header, two int32 and one 64-bit word per row, the owners and
    pairs of a frame's 4096 points, and a staging row of 1072 B, each array rounded up to 256 B."""
    L, so = lib
    for v in (-1, 0, 65537, BIG):
        assert so.ssp_world_upkeep_workspace_bytes(v) == 0 and "map_cap" in so.ssp_last_error().decode()
    up = lambda n: -(-n // 256) * 256
    for n in (1, 8, 1000, 65536):
        want = (up(64) + 2 * up(4 * n) + up(4 * 4096) + up(8 * 4096) + up(8 * n) + up(24 * n) + up(8 * n) + up(1024 * n) + 4 * up(4 * n))
        assert so.ssp_world_upkeep_workspace_bytes(n) == want, n
    assert so.ssp_world_upkeep_workspace_bytes(8) == 59904
