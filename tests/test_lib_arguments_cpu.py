"""The argument contract of the read-out and geometry wrappers of lib.py (op_match_two_way .. op_eval_accumulate), on the CPU.

The wrappers refuse CPU tensors, so the harness replaces three things: lib.load_library by a stub whose *_workspace_bytes
return 256 and whose other entries raise AssertionError("device entry reached"), lib._need_gpu by a version that keeps only
its contiguity RuntimeError, and torch.cuda.device by a guard that raises `Reached`.  A call is "accepted" when it gets as far
as that guard (or returns before it); otherwise its outcome is the exception's class and message.

cases() yields one accepted call per operator at the smallest sizes and single-fault mutations of it: for every tensor argument
and dict member the operator reads a wrong dtype, one rank more and less, every dimension off by one, a strided view, a missing key,
None (at P = 2 where the operator has a P: P = 1 is the accepted call and its special forms); for the scalars their bounds and one
step outside.  The buffer dicts are written out here with literal shapes: they restate the layouts
independently of lib.py's tables.  tests/lib_argument_contract.json holds the outcomes recorded from the commit before the
wrappers were rewritten (tools/record_lib_contract.py); the test holds every later lib.py to them."""
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = os.path.join(ROOT, "tests", "lib_argument_contract.json")
CAP = 8  # the builders below spell the other sizes out: L = 2, point_cap = 4, row_cap = 8, map_cap = 8, tid_cap = 16, capacity = 4
MAX_POINTS = 4096  # lib.MATCH_MAX_POINTS, restated


class Reached(Exception):
    """the device guard: every check of the wrapper has passed"""


class _StubLibrary:
    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return lambda *a: 256
        raise AssertionError("device entry reached")


class _Guard:
    def __init__(self, device):
        pass

    def __enter__(self):
        raise Reached()

    def __exit__(self, *a):
        return False


def _contiguous_only(t, name):
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


def install(lib, setattr_):
    """puts the three replacements in place through setattr_(object, name, value) (monkeypatch.setattr or a recorder)"""
    stub = _StubLibrary()
    setattr_(lib, "load_library", lambda path=None: stub)
    setattr_(lib, "_need_gpu", _contiguous_only)
    setattr_(torch.cuda, "device", _Guard)


def load_contract(path=CONTRACT):
    """{case id: "accepted" or [exception class, message]}; the file groups the ids "operator/case" by operator"""
    with open(path) as f:
        return {"%s/%s" % (op, case): v for op, group in json.load(f).items() for case, v in group.items()}


def dump_contract(contract):
    """the file's text: one block per operator, one case per line"""
    groups = {}
    for cid in sorted(contract):
        op, case = cid.split("/", 1)
        groups.setdefault(op, []).append(" %s: %s" % (json.dumps(case), json.dumps(contract[cid])))
    return "{\n" + ",\n".join("%s: {\n%s\n}" % (json.dumps(op), ",\n".join(rows)) for op, rows in groups.items()) + "\n}\n"


def outcome(fn, kwargs):
    try:
        fn(**kwargs)
    except Reached:
        return "accepted"
    except Exception as e:  # noqa: BLE001 - the class is what is recorded
        return [type(e).__name__, str(e)]
    return "accepted"


# ---- literal tensors and buffer dicts ----
def f64(*s):
    return torch.zeros(*s, dtype=torch.float64)


def f32(*s):
    return torch.zeros(*s, dtype=torch.float32)


def i32(*s):
    return torch.zeros(*s, dtype=torch.int32)


def i64(*s):
    return torch.zeros(*s, dtype=torch.int64)


def u8(*s):
    return torch.zeros(*s, dtype=torch.uint8)


def track_table():
    return {"ids": i32(8, 2), "tid": i32(8), "score": f64(8), "state": i32(4), "L": 2, "point_cap": 4, "row_cap": 8, "ws": u8(256)}


def landmark_dict():
    return {"cams": f64(2, 20), "X": f64(8, 3), "n_views": i32(8), "rms": f64(8), "cos_parallax": f64(8), "status": i32(8),
            "landmarks": f64(8, 8), "n_landmarks": i32(1), "ws": u8(256)}


def landmark_rows():
    return {"X": f64(8, 3), "n_views": i32(8), "rms": f64(8), "cos_parallax": f64(8), "status": i32(8)}


def pnp_dict(P, cap):
    return {"corr": f64(P, cap, 8), "n": i32(P, 2), "Rw": f64(P, 3, 3), "C": f64(P, 3), "mask": u8(P, cap), "n_inliers": i32(P),
            "winner": i32(P), "rms": f64(P), "status": i32(P), "ws": u8(256)}


def ba_dict():
    return {"cams": f64(2, 20), "X": f64(8, 3), "rms": f64(8), "info": f64(8), "ws": u8(256)}


def world_dict(map_cap=8, tid_cap=16):
    return {"X": f64(map_cap, 3), "desc": f32(map_cap, 256), "tid": i32(map_cap), "n_views": i32(map_cap), "first_frame": i32(map_cap),
            "last_frame": i32(map_cap), "rms": f64(map_cap), "slot_of_tid": i32(tid_cap), "state": i32(8), "ws": u8(256),
            "map_cap": map_cap, "tid_cap": tid_cap}


def loop_dict(cap, capacity=4):
    return {"corr": f64(cap, 8), "xnew": f64(cap, 4), "n": i32(3), "edges": f64(256, 16), "state": i32(8), "cand": f64(16),
            "Rw": f64(capacity, 9), "C": f64(capacity, 3), "sigma": f64(capacity), "info": f64(8), "ws": u8(256), "cap": cap,
            "capacity": capacity}


def pose_dict(P, cap):
    return {"R": f64(P, 3, 3), "t": f64(P, 3), "E": f64(P, 3, 3), "cand": i32(P), "counts": i32(P, 4), "n_front": i32(P),
            "status": i32(P), "front": u8(P, cap), "depth": f64(P, cap, 2), "X": f64(P, cap, 3)}


def ransac_dict(key, P, cap):
    return {key: f64(P, 3, 3), "mask": u8(P, cap), "n_inliers": i32(P), "status": i32(P)}


def pair(P, cap, stride=2):
    return dict(pts1=f64(P, cap, stride), pts2=f64(P, cap, stride), match=f32(P, cap, 3), n_match=i32(P))


def absolute(P, cap):
    return {"Rw": f64(P, 3, 3), "C": f64(P, 3), "mask": u8(P, cap), "n_inliers": i32(P), "winner": i32(P), "rms": f64(P),
            "status": i32(P)}


# ---- one accepted call per operator: name -> (builder(P, cap, **sizes) -> kwargs, sizes it takes, scalar cases) ----
def _b_match_two_way(P, cap):
    return dict(desc1=f32(P, cap, 256), count1=i32(P), desc2=f32(P, cap, 256), count2=i32(P), nn_thresh=0.7, cls1=u8(P, cap),
                cls2=u8(P, cap))


def _b_track_update(P, cap):
    return dict(table=track_table(), match=f32(4, 3), n_match=i32(1), n_points=i32(1), match_score64=f64(4), out=track_table())


def _b_track_select(P, cap):
    return dict(table=track_table(), min_length=2)


def _b_track_points(P, cap):
    return dict(tracks=f64(8, 4), n_tracks=i32(1), pts=f64(2, 4, 2), state=i32(4))


def _b_det_tp_fp(P, cap):
    return dict(prob=f32(2, 8, 8), labels=f32(2, 8, 8), keys=i64(16), state=i64(80))


def _b_det_tp_fp_points(P, cap):
    return dict(pts=f32(2, cap, 5), count=i32(2), labels=u8(2, 8, 8), keys=i64(16), state=i64(80))


def _b_det_pr_curve(P, cap):
    return dict(sorted_keys=i64(16), state=i64(80))


def _b_eval_repeatability(P, cap):
    return dict(pts1=f64(P, cap, 3), n1=i32(P), pts2=f64(P, cap, 3), n2=i32(P), hom=f64(P, 3, 3), hom_inv=f64(P, 3, 3), height=8,
                width=8)


def _b_eval_ransac(P, cap):
    return dict(pair(P, cap, 3), seeds=i64(P), want_ap=True)


def _b_epipolar_ransac(P, cap):
    return dict(pair(P, cap), seeds=i64(P))


def _b_filter_matches(P, cap):
    return dict(match=f32(P, cap, 3), n_match=i32(P), mask=u8(P, cap), status=i32(P), n_inliers=i32(P), min_inliers=8)


def _b_two_view_pose(P, cap):
    return dict(geometry=ransac_dict("F", P, cap), intrinsics=f64(P, 2, 4), **pair(P, cap))


def _b_pose_chain(P, cap):
    return dict(prev=pose_dict(P, cap), cur=pose_dict(P, cap), match_prev=f32(P, cap, 3), match_cur=f32(P, cap, 3), n_match_prev=i32(P),
                n_match_cur=i32(P), state=f64(P, 16), table=f64(P, 4, 16))


def _b_homography_pose(P, cap):
    return dict(geometry_h=ransac_dict("H", P, cap), intrinsics=f64(P, 2, 4), prior=f64(P, 2, 3), use_h=i32(P), out=pose_dict(P, cap),
                **pair(P, cap))


def _b_model_select(P, cap):
    return dict(geometry_f=ransac_dict("F", P, cap), geometry_h=ransac_dict("H", P, cap), **pair(P, cap))


def _b_map_window(P, cap, L=2):
    return dict(state=f64(16), table=f64(4, 16), intrinsics=f64(L, 4), max_length=L, n_frames=3, out={"cams": f64(L, 20)})


def _b_triangulate(P, cap):
    return dict(table=track_table(), pts=f64(2, 4, 2), first_slot=0, cams=f64(2, 20), out=landmark_dict())


def _b_landmarks_select(P, cap):
    return dict(table=track_table(), rows=landmark_rows(), out=landmark_dict())


def _b_landmark_matches(P, cap):
    return dict(landmarks=f64(8, 8), n_landmarks=i32(1), match=f32(cap, 3), n_match=i32(1), pts_new=f64(4, 2), out=pnp_dict(1, cap))


def _b_pnp_ransac(P, cap):
    return dict(corr=f64(P, cap, 8), n=i32(P), intrinsics=f64(P, 4), seeds=i64(P), out=pnp_dict(P, cap))


def _b_pose_repair(P, cap):
    return dict(absolute=absolute(P, cap), state=f64(P, 16), table=f64(P, 4, 16))


def _b_bundle_adjust(P, cap):
    return dict(table=track_table(), pts=f64(2, 4, 2), first_slot=0, cams=f64(2, 20), rows=landmark_rows(), iterations=10, out=ba_dict())


def _b_ba_apply(P, cap, L=2):
    return dict(adjusted={"cams": f64(P, L, 20), "X": f64(8, 3), "rms": f64(8), "info": f64(P, 8)}, state=f64(P, 16), table=f64(P, 4, 16),
                max_length=L, n_frames=3)


def _b_world_insert(P, cap, map_cap=8, tid_cap=16):
    return dict(world=world_dict(map_cap, tid_cap), landmarks=f64(8, 8), n_landmarks=i32(1), desc_new=f32(4, 256), count_new=i32(1),
                table=f64(4, 16), n_frames=3)


def _b_match_world(P, cap):
    return dict(world=world_dict(), desc2=f32(cap, 256), count2=i32(1), nn_thresh=0.7, out=(f32(cap, 3), i32(1)))


def _b_world_correspondences(P, cap):
    return dict(world=world_dict(), match=f32(cap, 3), n_match=i32(1), pts_new=f64(4, 2), count_new=i32(1), out=pnp_dict(1, cap))


def _b_world_repair(P, cap):
    return dict(world=world_dict(), absolute=absolute(1, cap), state=f64(16), table=f64(4, 16))


def _b_loop_correspondences(P, cap, capacity=4):
    return dict(world=world_dict(), match=f32(cap, 3), n_match=i32(1), pts_new=f64(4, 2), count_new=i32(1), landmarks=f64(8, 8),
                n_landmarks=i32(1), frame=3, min_gap=1, loop=loop_dict(cap, capacity))


def _b_loop_edge(P, cap):
    return dict(world=world_dict(), absolute=absolute(1, cap), table=f64(4, 16), frame=3, loop=loop_dict(cap))


def _b_pose_graph(P, cap):
    return dict(table=f64(4, 16), frame=3, loop=loop_dict(cap), iterations=10)


def _b_loop_apply(P, cap):
    return dict(world=world_dict(), state=f64(16), table=f64(4, 16), frame=3, loop=loop_dict(cap))


def _b_pixel_homographies(P, cap):
    return dict(hn=f32(P, 3, 3), height=8, width=8)


def _b_eval_accumulate(P, cap):
    return dict(rows=f64(4, 16), state=f64(16), first_pair=0, rep=f64(P, 8), ransac={"H": f64(P, 3, 3), "n_inliers": i32(P), "status": i32(P)},
                ap=f64(P), n1=i32(P), hom=f64(P, 3, 3))


INF = float("inf")
# operator -> (builder, takes P, takes cap, {scalar: values}, {builder size: values})
OPERATORS = {
    "op_match_two_way": (_b_match_two_way, True, True, {"nn_thresh": (0.0, -0.5), "pair_stride": (2,), "n_pairs": (0, 1, 3)}, {}),
    "op_track_update": (_b_track_update, False, False, {}, {}),
    "op_track_select": (_b_track_select, False, False, {}, {}),
    "op_track_points": (_b_track_points, False, False, {}, {}),
    "op_detector_tp_fp": (_b_det_tp_fp, False, False, {}, {}),
    "op_detector_tp_fp_points": (_b_det_tp_fp_points, False, True, {}, {}),
    "op_detector_pr_curve": (_b_det_pr_curve, False, False, {}, {}),
    "op_eval_repeatability": (_b_eval_repeatability, True, True, {"n_pairs": (0, 1, 3), "pair_stride": (2,)}, {}),
    "op_eval_ransac": (_b_eval_ransac, True, True, {"pair_stride": (2,), "want_ap": (False,)}, {}),
    "op_epipolar_ransac": (_b_epipolar_ransac, True, True, {"pair_stride": (2,)}, {}),
    "op_filter_matches": (_b_filter_matches, True, True, {}, {}),
    "op_two_view_pose": (_b_two_view_pose, True, True, {"pair_stride": (2,)}, {}),
    "op_pose_chain": (_b_pose_chain, True, True, {}, {}),
    "op_homography_pose": (_b_homography_pose, True, True,
                           {"pair_stride": (2,), "rotation_eps": (0.0, -1e-3), "normal_margin": (0.0, -1e-3)}, {}),
    "op_model_select": (_b_model_select, True, True, {"pair_stride": (2,), "model_ratio": (0.0, 1.0, -0.01, 1.01)}, {}),
    "op_map_window": (_b_map_window, False, False, {"n_frames": (0, -1, None)}, {"L": (2, 16, 1, 17)}),
    "op_triangulate_tracks": (_b_triangulate, False, False, {"first_slot": (1, -1, 2), "min_views": (2, 1),
                                                             "min_parallax_deg": (0.0, 180.0, -1.0, 181.0), "max_reproj": (0.0, -1.0)}, {}),
    "op_landmarks_select": (_b_landmarks_select, False, False, {}, {}),
    "op_landmark_matches": (_b_landmark_matches, False, True, {}, {}),
    "op_pnp_ransac": (_b_pnp_ransac, True, True, {"min_inliers": (4, 3)}, {}),
    "op_pose_repair": (_b_pose_repair, True, False, {}, {}),
    "op_bundle_adjust": (_b_bundle_adjust, False, False, {"first_slot": (1, -1, 2), "iterations": (1, 16, 0, 17)}, {}),
    "op_ba_apply": (_b_ba_apply, True, False, {"n_frames": (0, -1, None)}, {"L": (2, 16, 1, 17)}),
    "op_world_insert": (_b_world_insert, False, False, {"n_frames": (0, -1), "patience": (0, -1)},
                        {"map_cap": (1, 0, 65537), "tid_cap": (1, 0)}),
    "op_match_world": (_b_match_world, False, True, {"nn_thresh": (0.0, -0.5)}, {}),
    "op_world_correspondences": (_b_world_correspondences, False, True, {}, {}),
    "op_world_repair": (_b_world_repair, False, False, {}, {}),
    "op_loop_correspondences": (_b_loop_correspondences, False, True, {"frame": (0, -1), "min_gap": (1, 0)}, {"capacity": (2, 1)}),
    "op_loop_edge": (_b_loop_edge, False, True, {"frame": (0, -1), "min_inliers": (4, 3), "cooldown": (0, -1),
                                                 "weight": (1e-9, 0.0, INF)}, {}),
    "op_pose_graph": (_b_pose_graph, False, False, {"frame": (0, -1), "iterations": (1, 64, 0, 65)}, {}),
    "op_loop_apply": (_b_loop_apply, False, False, {"frame": (0, -1)}, {}),
    "op_eval_pixel_homographies": (_b_pixel_homographies, True, False, {}, {}),
    "op_eval_accumulate": (_b_eval_accumulate, True, False, {"first_pair": (0, -1), "pair_stride": (0, 2), "thresholds": ((1, 3, 5, 10, 20),),
                                                             "corner_shape": ((240, 320, 3),)}, {}),
}


# ---- mutations ----
_OTHER = {torch.float64: torch.float32, torch.float32: torch.float64, torch.int32: torch.int64, torch.int64: torch.int32,
          torch.uint8: torch.int32}


def _mutations(t):
    """(tag, tensor) single faults of a tensor"""
    s = tuple(t.shape)
    yield "dtype", t.to(_OTHER[t.dtype])
    yield "rank+1", t[None]
    yield "rank-1", t[0]
    for i, n in enumerate(s):
        yield "dim%d+1" % i, torch.zeros(s[:i] + (n + 1,) + s[i + 1:], dtype=t.dtype)
    if all(n >= 2 for n in s):  # no size-1 dimension: the view below really is strided
        v = torch.zeros(s[:-1] + (2 * s[-1],), dtype=t.dtype)[..., ::2]
        assert not v.is_contiguous() and tuple(v.shape) == s
        yield "strided", v


# The dict members an operator reads (a dict that is not named: all of them).  The world and loop dicts go through one checker
# whichever operator takes them: every member is mutated under op_world_insert resp. op_loop_correspondences, one elsewhere.
_ABSOLUTE, _ONE = ("Rw", "C", "status"), ("state", "ws")
READS = {
    "op_pose_chain": {"prev": ("front", "depth", "status"), "cur": ("front", "depth", "status", "R", "t")},
    "op_homography_pose": {"out": ("R", "t", "cand", "counts", "n_front", "status", "front", "depth", "X")},
    "op_triangulate_tracks": {"table": ("ids", "state"), "out": ("X", "n_views", "rms", "cos_parallax", "status")},
    "op_landmarks_select": {"table": ("ids", "tid", "state"), "out": ("landmarks", "n_landmarks", "ws")},
    "op_landmark_matches": {"out": ("corr", "n")},
    "op_pnp_ransac": {"out": ("Rw", "C", "mask", "n_inliers", "winner", "rms", "status", "ws")},
    "op_pose_repair": {"absolute": _ABSOLUTE},
    "op_bundle_adjust": {"table": ("ids", "state"), "rows": ("X", "status")},
    "op_ba_apply": {"adjusted": ("info", "cams")},
    "op_match_world": {"world": _ONE},
    "op_world_correspondences": {"world": _ONE, "out": ("corr", "n")},
    "op_world_repair": {"world": _ONE, "absolute": _ABSOLUTE},
    "op_loop_correspondences": {"world": _ONE},
    "op_loop_edge": {"world": _ONE, "loop": _ONE, "absolute": ("Rw", "C", "mask", "status")},
    "op_pose_graph": {"loop": _ONE},
    "op_loop_apply": {"world": _ONE, "loop": _ONE},
}


def _leaves(name, kwargs):
    """(argument, key or None, tensor) of every tensor a call is given and the operator reads"""
    for a, v in kwargs.items():
        if torch.is_tensor(v):
            yield a, None, v
        elif isinstance(v, dict):
            for k, m in v.items():
                if torch.is_tensor(m) and k in READS.get(name, {}).get(a, v):
                    yield a, k, m
        elif isinstance(v, tuple):
            for k, m in enumerate(v):
                if torch.is_tensor(m):
                    yield a, k, m


def _replaced(kwargs, a, k, value):
    out = dict(kwargs)
    if k is None:
        out[a] = value
    elif isinstance(kwargs[a], tuple):
        out[a] = tuple(value if i == k else m for i, m in enumerate(kwargs[a]))
    else:
        out[a] = dict(kwargs[a])
        out[a][k] = value
    return out


def _special(name, P, cap):
    """the acceptances and refusals that are no mutation of one tensor"""
    b = OPERATORS[name][0]
    if name == "op_match_two_way":
        kw = b(P, cap)
        yield "no_classes", dict(kw, cls1=None, cls2=None), "cls1"
        yield "one_class_side", dict(kw, cls2=None), "cls2"
    if name == "op_filter_matches" and P == 1:
        kw = b(1, cap)
        yield "match2d", dict(kw, match=kw["match"][0]), "match"
    if name == "op_pnp_ransac" and P == 1:
        kw = b(1, cap)
        yield "corr2d", dict(kw, corr=kw["corr"][0]), "corr"
        yield "no_ws", dict(kw, out={k: v for k, v in kw["out"].items() if k != "ws"}), "out"
    if name in ("op_eval_ransac", "op_epipolar_ransac", "op_two_view_pose", "op_homography_pose", "op_model_select", "op_filter_matches"):
        kw = b(P, cap)
        yield "n_match_column", dict(kw, n_match=kw["n_match"][:, None]), "n_match"
    if name in ("op_epipolar_ransac", "op_two_view_pose", "op_homography_pose", "op_model_select"):
        kw = b(P, cap)
        yield "pt_stride3", dict(kw, pts1=f64(P, cap, 3), pts2=f64(P, cap, 3)), "pts1"
        yield "pt_stride1", dict(kw, pts1=f64(P, cap, 1), pts2=f64(P, cap, 1)), "pts1"
        yield "longer_pts", dict(kw, pts1=f64(P + 3, cap, 2), pts2=f64(P + 3, cap, 2), pair_stride=2), "pts1"
    if name in ("op_two_view_pose", "op_homography_pose"):
        kw = b(P, cap)
        yield "shared_intrinsics", dict(kw, intrinsics=f64(1, 2, 4)), "intrinsics"
    if name in ("op_pnp_ransac", "op_map_window"):
        kw = b(P, cap)
        yield "shared_intrinsics", dict(kw, intrinsics=f64(1, 4)), "intrinsics"
    if name == "op_pose_chain":
        kw = b(P, cap)
        yield "no_prev", dict(kw, prev=None, match_prev=None, n_match_prev=None), "prev"
        yield "prev_other_cap", dict(kw, prev=pose_dict(P, cap + 3), match_prev=f32(P, cap + 3, 3)), "prev"
        if P == 1:
            yield "one_sequence_flat", dict(kw, state=f64(16), table=f64(4, 16)), "state"
    if name == "op_homography_pose":
        kw = b(P, cap)
        yield "use_h_without_out", dict(kw, out=None), "use_h"
        yield "new_tensors", dict(kw, out=None, use_h=None), "out"
        yield "no_prior", dict(kw, prior=None), "prior"
    if name in ("op_pose_repair", "op_ba_apply") and P == 1:
        kw = b(1, cap)
        yield "one_sequence_flat", dict(kw, state=f64(16), table=f64(4, 16)), "state"
    if name == "op_ba_apply" and P == 1:
        kw = b(1, cap)
        yield "adjusted_flat", dict(kw, adjusted=dict(kw["adjusted"], info=f64(8), cams=f64(2, 20))), "adjusted"
    if name == "op_bundle_adjust":
        kw = b(P, cap)
        yield "out_shares_cams", dict(kw, out=dict(kw["out"], cams=kw["cams"])), "out"
        yield "out_shares_X", dict(kw, out=dict(kw["out"], X=kw["rows"]["X"])), "out"
    if name == "op_track_update":
        kw = b(P, cap)
        yield "out_is_table", dict(kw, out=kw["table"]), "out"
        yield "no_score64", dict(kw, match_score64=None), "match_score64"
        yield "longer_match", dict(kw, match=f32(9, 3)), "match"
    if name == "op_match_world":
        kw = b(P, cap)
        yield "small_ws", dict(kw, world=dict(kw["world"], ws=u8(255))), "world['ws']"
    if name == "op_eval_accumulate":
        kw = b(P, cap)
        yield "rep_only", dict(kw, ransac=None, ap=None, n1=None, hom=None), "ransac"
        yield "ransac_only", dict(kw, rep=None), "rep"
        yield "nothing", dict(kw, rep=None, ransac=None, ap=None, n1=None, hom=None), "rep"
        yield "half_group", dict(kw, ap=None), "ap"
        if P == 1:
            yield "P128", b(128, cap), "rep"
            yield "P129", b(129, cap), "rep"
    if name == "op_detector_tp_fp":
        kw = b(P, cap)
        yield "four_dims", dict(kw, prob=f32(2, 1, 8, 8), labels=u8(2, 1, 8, 8)), "labels"


def cases():
    """(id, operator, kwargs, the mutated argument's name as a message should spell it) of every case of the contract"""
    for name, (b, has_P, has_cap, scalars, sizes) in OPERATORS.items():
        for P in ((1, 2) if has_P else (1,)):
            tag = "%s/P%d" % (name, P) if has_P else name
            kw = b(P, CAP)
            yield tag + "/valid", name, kw, None
            for a, k, t in (_leaves(name, kw) if P == 2 or not has_P else ()):  # the faults of a tensor: at P = 2 where there is a P
                where = a if k is None else "%s[%r]" % (a, k)
                for m, v in _mutations(t):
                    yield "%s/%s/%s" % (tag, where, m), name, _replaced(kw, a, k, v), where
                if k is None:
                    yield "%s/%s/None" % (tag, where), name, _replaced(kw, a, k, None), where
                elif isinstance(kw[a], dict):
                    yield "%s/%s/missing" % (tag, where), name, dict(kw, **{a: {q: m for q, m in kw[a].items() if q != k}}), a
            for a, v in kw.items():
                if isinstance(v, (dict, tuple)) and (P == 2 or not has_P):
                    yield "%s/%s/None" % (tag, a), name, dict(kw, **{a: None}), a
            for m, kw2, where in _special(name, P, CAP):
                yield "%s/%s" % (tag, m), name, kw2, where
        for a, values in scalars.items():
            for v in values:
                yield "%s/%s=%r" % (name, a, v), name, dict(b(2 if has_P else 1, CAP), **{a: v}), a
        for a, values in sizes.items():
            for v in values:
                yield "%s/size:%s=%r" % (name, a, v), name, b(1, CAP, **{a: v}), {"L": "max_length", "map_cap": "world", "tid_cap": "world",
                                                                                    "capacity": "loop"}[a]
        if has_cap:
            for cap in (0, 1, MAX_POINTS, MAX_POINTS + 1):
                yield "%s/size:cap=%d" % (name, cap), name, b(1, cap), "cap"


MATCHED = {"op_match_two_way": ("uint8", "both or neither")}  # what tests/test_gpu_point_classes.py matches in a message stays in it


@pytest.fixture()
def lib(monkeypatch):
    from semantic_superpoint_amd import lib as L
    install(L, monkeypatch.setattr)
    return L


def test_argument_contract(lib):
    """Every case that is generated is recorded and the other way round; an accepted call stays accepted; a refusal stays a refusal
    of the same exception class; a ValueError or RuntimeError either keeps its recorded text or names the mutated argument as the
    signature spells it (a dict member as name['key']; a size by the argument or dict that sets it).  One allowance: an IndexError
    recorded for a tensor one rank short was Python's, raised inside a shape test, not a wrapper's answer; it may become the
    ValueError that names the argument (pts2 of op_epipolar_ransac and op_two_view_pose, table of op_world_repair)."""
    recorded = load_contract()
    seen, wrong = set(), []
    for cid, name, kwargs, where in cases():
        assert cid not in seen, "case id %s twice" % cid
        seen.add(cid)
        want = recorded.get(cid)
        if want is None:
            continue
        got = outcome(getattr(lib, name), kwargs)
        if want == "accepted" or got == "accepted":
            if got != want:
                wrong.append((cid, want, got))
            continue
        if got[0] != want[0]:
            if not (want[0] == "IndexError" and cid.endswith("/rank-1") and got[0] == "ValueError" and where in got[1]):
                wrong.append((cid, want, got))
        elif got[0] in ("ValueError", "RuntimeError") and got[1] != want[1]:
            # a reworded message names the mutated argument as the signature spells it (dict members as name['key'])
            if where not in got[1] or any(w in want[1] and w not in got[1] for w in MATCHED.get(name, ())):
                wrong.append((cid, want, got))
    assert seen == set(recorded), "cases generated and recorded differ: %s" % sorted(seen ^ set(recorded))[:10]
    assert not wrong, "%d of %d cases moved, e.g. %s" % (len(wrong), len(seen), wrong[:10])


def test_constants_mirror_the_header():
    """Every constant of lib.py whose comment names an SSP_* define equals that define in include/ssp_hip.h."""
    src = open(os.path.join(ROOT, "semantic-superpoint_amd", "lib.py")).read()
    hdr = open(os.path.join(ROOT, "include", "ssp_hip.h")).read()
    mirrored = {m.group(3): (m.group(1), int(m.group(2))) for m in re.finditer(r"^([A-Z][A-Z0-9_]*) = (\d+)  # (SSP_\w+)", src, re.M)}
    checked = set()
    for m in re.finditer(r"^#define (SSP_\w+)[ \t]+\(?(-?\d+|0x[0-9a-fA-F]+)\)?[ \t]*(?:/[/*].*)?$|^enum \{ (SSP_\w+) = (\d+) \};", hdr, re.M):
        define, value = (m.group(1) or m.group(3)), int(m.group(2) or m.group(4), 0)
        if define in mirrored:
            name, mine = mirrored[define]
            assert mine == value, "%s = %d but %s is %d" % (name, mine, define, value)
            checked.add(define)
    assert checked == set(mirrored), "include/ssp_hip.h has no integer %s" % sorted(set(mirrored) - checked)
    assert len(checked) >= 25, "only %d mirrored constants found: the pattern no longer reads lib.py" % len(checked)
