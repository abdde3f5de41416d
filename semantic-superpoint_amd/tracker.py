"""The trackers of the descriptor export (DESIGN.md sections 17, 18, 22, 24, 26-29, 31): PointTracker, the reference's
models/model_wrap.py:416-615 on the device with the geometric stages behind it, and SequenceTracker, which feeds it from a model
frame by frame.  export.py re-exports both classes: `from semantic_superpoint_amd.export import PointTracker, SequenceTracker`.

Every arithmetic step runs in libssp_hip.so; tensors must live on a HIP device (no CPU fallback)."""
import numpy as np
import torch

from . import lib as L


def _check_mode(option, value, *modes):
    """ValueError unless `value` is None or one of `modes`."""
    if value is not None and value not in modes:
        raise ValueError("%s must be None, %s or %r (got %r)" % (option, ", ".join(repr(m) for m in modes[:-1]), modes[-1], value))


def _check_one_camera(intrinsics, message):
    """ValueError(message) when `intrinsics` is a (previous, new) pair of two different cameras."""
    k = np.asarray(intrinsics, dtype=np.float64)
    if k.shape == (2, 4) and not np.array_equal(k[0], k[1]):
        raise ValueError(message)


def _check_stage(option, source, intrinsics, geometric_check, landmark_params, *own):
    """What every stage that works on the window's landmarks needs, in this order: intrinsics with the fundamental or auto check
    (the stages read the trajectory, the matches and front / depth, never F), ONE
    camera, the stage's own options (`own`: pairs of a test that returns True when refused, and its message), landmark_params."""
    if intrinsics is None or geometric_check not in ("fundamental", "auto"):
        raise ValueError("%s needs intrinsics and geometric_check='fundamental': %s" % (option, source))   # (or 'auto': section 36)
    _check_one_camera(intrinsics, "%s needs ONE camera: a fixed (previous, new) pair of different intrinsics cannot describe "
                                  "more than two views" % option)
    for refused, message in own:
        if refused():
            raise ValueError(message)
    if len(landmark_params) != 3 or int(landmark_params[0]) < 2:
        raise ValueError("landmark_params must be (min_views >= 2, min_parallax_deg, max_reproj)")


def _pnp_no_pose(a):
    """The result of a frame without a pose in the lib.pnp_buffers `a`: status 1, Rw = I, C = 0, no correspondence."""
    for k in ("corr", "n", "C", "mask", "n_inliers", "rms"):
        a[k].zero_()
    a["Rw"].copy_(torch.eye(3, dtype=torch.float64, device=a["Rw"].device)[None])
    a["winner"].fill_(-1)
    a["status"].fill_(1)
    return {k: a[k] for k in L.PNP_KEYS}


def _write_pose_row(table, f, res, n_corr):
    """A P3P result (lib.op_pnp_ransac) and its number of correspondences into row f of a [rows, POSE_ROW_WORDS] table, if it has one."""
    if f < table.shape[0]:
        row = table[f]
        row[0:9] = res["Rw"].reshape(9)
        row[9:12] = res["C"].reshape(3)
        row[12:13] = res["n_inliers"]
        row[13:14] = res["rms"]
        row[14:15] = res["status"]
        row[15:16] = n_corr


class PointTracker(object):
    """models/model_wrap.py:416-615 on the device for 2 <= max_length <= lib.TRACK_MAX_LENGTH: the two-way nearest-neighbour
    matcher (ssp_match_two_way) and the track bookkeeping (ssp_op_track_update / _select / _points).
    The table, the running track count, the last max_length point sets and the previous frame's descriptors stay in HBM;
    `update` uploads one frame and reads the matches back (get_matches is a numpy contract), `update_device` takes device
    tensors and synchronises with the host only to allocate.  Descriptors are 256-dimensional.  draw_tracks is not provided
    (no drawing here): `track_points` returns the coordinates it would connect.
    class_consistent=True: every frame comes with the class of each point (`cls`); the previous
    frame's classes are kept beside its descriptors and only points of equal class are matched
    (ssp_match_two_way_classes).  The track table logic is the same.
    geometric_check: None accepts every mutual match below nn_thresh (the reference).  "fundamental"
    fits a fundamental matrix to the frame's matches (lib.op_epipolar_ransac, inliers within check_thresh pixels of Sampson
    distance) and "homography" a homography (lib.op_eval_ransac with its own 3 px rule); only the inliers continue tracks and
    are reported by get_matches / get_mscores.  A frame with no model or fewer than min_inliers inliers keeps all its
    matches; that is decided on the device.  Frame f (0-based) uses seed check_seed + f.  last_geometry() is the newest
    frame's result.  "auto" (needs intrinsics) runs both with the frame's seed, decides per frame which model
    the frame obeys (lib.op_model_select, model_ratio) and takes the pose from that model (lib.op_homography_pose with rotation_eps,
    normal_margin and the previous frame's normals2 as the prior): planar scenes and a camera that only rotates get a pose and a
    trajectory row.  last_geometry() gains "model" (0 fundamental, 1 plane, 2 rotation), "scores", "H", "h_mask", "h_n_inliers",
    "h_status", "normal", "normals2"; "mask", "n_inliers", "status" are the selected model's, "F", "winner", "err" the F fit's.
    intrinsics (needs geometric_check="fundamental" or "auto"): (fx, fy, cx, cy) of the camera, or a pair of such
    tuples (the camera of the previous frame, the camera of the new frame).  Every frame's fundamental matrix then gives the
    camera motion from the previous frame (lib.op_two_view_pose: last_geometry() gains its keys, "status" as "pose_status")
    and one row of the trajectory (lib.op_pose_chain), read with trajectory(); trajectory_rows sizes that table.  All of it is
    queued on the device like the check itself.  None runs none of it.
    landmarks / landmarks_device / landmark_rows_device (need intrinsics of ONE camera): one point in the
    world frame per track, from its observations in the retained frames under the trajectory's cameras.  On demand: update /
    update_device run none of it.
    absolute_pose (needs intrinsics of ONE camera): None runs none of it.  "observe": after every frame the
    tracker keeps the landmarks of the window ending there (landmark_params = (min_views, min_parallax_deg, max_reproj), in buffers
    of its own: landmarks_device neither sees nor disturbs them); the next frame's unfiltered matches join them to its points
    (lib.op_landmark_matches) and a P3P RANSAC (lib.op_pnp_ransac, absolute_thresh pixels, absolute_min_inliers, the frame's
    check seed) places its camera in the window's frame and scale: last_geometry() gains the "abs_*" keys and
    absolute_trajectory() one row.  "repair" also rewrites the frame's trajectory row and the chain state from that pose
    (lib.op_pose_repair) when the two-view chain could not determine them, so a frame without a two-view pose no longer breaks the
    window.  All of it is queued on the device.
    bundle_adjust (needs intrinsics of ONE camera): None runs none of it.  "observe": after the track update
    of every bundle_every-th frame the cameras of the newest consistent window and the landmarks triangulated under them
    (landmark_params, buffers of the tracker's own) are refined together (lib.op_bundle_adjust, bundle_iterations);
    bundle_adjusted() returns the result and last_geometry() gains "ba_info".  "apply" also writes the refined cameras back into
    the trajectory and the chain state (lib.op_ba_apply), so the next frame's chain, the kept landmarks of absolute_pose and
    landmarks_device see them.  All of it is queued on the device.
    world_map (needs intrinsics of ONE camera): None runs none of it.  "observe": the landmarks of every
    frame's window (landmark_params, buffers of the tracker's own) enter a map of world_cap rows that keeps X and the newest
    descriptor of every track after the track has left the window (lib.op_world_insert, while the map is anchored to the
    trajectory; world_patience frames without an anchor clear it).  Every frame's unfiltered descriptors are matched against the
    whole map (lib.op_match_world with nn_thresh; class_consistent does not reach the map matcher: world_classes="match" does), joined
    with its points (lib.op_world_correspondences) and given to the P3P RANSAC (world_thresh pixels, world_min_inliers, the frame's
    check seed): last_geometry() gains the "world_*" keys and world_trajectory() one row.  "relocalise" also rewrites the frame's
    trajectory row and the chain state from that pose (lib.op_world_repair) when the two-view chain could not determine them or
    the map has lost its anchor, so a frame without points no longer restarts the map.  All of it is queued on the device.
    loop_closure (needs world_map): None runs none of it.  "observe": after the window's landmarks are
    selected and before they enter the map, the frame's map matches whose map row was last seen loop_min_gap frames ago or earlier
    are joined with the frame's points and window landmarks (lib.op_loop_correspondences) and given to the P3P RANSAC (world_thresh,
    loop_min_inliers, the frame's check seed); lib.op_loop_edge measures the similarity between the chained frame and the old map
    and appends an edge when its rule holds (at most one per loop_cooldown frames); lib.op_pose_graph distributes it over the rows
    since the old place was last seen (loop_iterations Levenberg-Marquardt steps, loop edges weighted loop_weight).  Nothing is
    written into the trajectory or the map.  "apply" also writes the corrected rows, the chain state and the map rows of that span
    (lib.op_loop_apply; POSE_FLAG_LOOP) and selects the window's landmarks once more before the insert.  last_geometry() gains the
    "loop_*" keys; loop_closures() and loop_edges_device() read the accepted edges.
    world_upkeep (needs world_map): None runs none of it.  "on": right after every insert (and so after loop
    closure and its write-back) lib.op_world_upkeep merges the row pair of a scene point that came back under a new track id
    (world_merge, within world_merge_thresh pixels, default world_thresh), removes rows last seen more than world_cull_age frames
    ago (default max_length) with fewer than world_cull_min_views views, and, once more than world_high_water rows are alive
    (default world_cap - world_cap // 16), evicts the least seen, then oldest rows down to world_low_water (default world_cap -
    world_cap // 8); a negative world_cull_age or world_high_water switches that phase off.  The map is compacted, so map rows
    change their slots: last_geometry()["world_match"] indexes the map as it stood before the frame's upkeep.  last_geometry() gains
    "world_upkeep_report"; world_upkeep_report() reads the running totals.
    world_classes (needs world_map, and every frame's classes `cls` as class_consistent does; the two options
    are independent): None runs none of it.  "observe": after every frame's landmark selection, beside the insert and before the
    upkeep, each landmark's track takes a vote on its class from the class of its point in the newest frame
    (lib.op_track_class_votes; votes per track id, so they survive the upkeep's moves and a cleared map); world_classes_device()
    and world_map(classes=True) read the map as a labelled point cloud; every other output stays as it was.  "match": the frame is
    also matched against the map by lib.op_match_world_classes: a map row takes part only with frame points of its own voted class,
    and only when that class is known and kept by world_keep_classes / world_drop_classes (one of them, ids below 255; neither: all
    classes), so the world pose, relocalisation, loop closure and the upkeep's merge, which all read these match rows, never join
    across classes.  reset_world_classes() zeroes the votes.
    ground_truth (needs intrinsics): float64 [N, 12] camera-to-world rows (R | C), the layout of a KITTI poses
    file; gt_index: int32 [trajectory_rows], the ground-truth row of each frame (-1: none), or None when frame f is row f.
    evaluate_trajectory(which, **options) scores trajectory(), absolute_trajectory() or world_trajectory() on demand (alignment, ATE,
    RPE, the KITTI segments; trajectory_evaluation.TrajectoryEvaluator).  trajectory_eval="observe": every frame, after all of its
    write-backs, appends a row (ATE rmse, mean, max of the frames so far under their own eval_align alignment, s, n_valid, status,
    two spare) to a device log [trajectory_rows, 8] for eval_table = "trajectory" or "world", with no host copy or synchronisation;
    trajectory_eval_log() reads it and last_geometry() gains "trajectory_eval".  With trajectory_eval=None no new code runs."""

    def __init__(self, max_length, nn_thresh, device=None, class_consistent=False, geometric_check=None, check_thresh=1.0,
                 min_inliers=16, check_seed=0, intrinsics=None, trajectory_rows=4096, absolute_pose=None, absolute_thresh=2.0,
                 absolute_min_inliers=6, landmark_params=(2, 1.0, 2.0), bundle_adjust=None, bundle_iterations=10, bundle_every=1,
                 world_map=None, world_cap=65536, world_patience=30, world_thresh=2.0, world_min_inliers=6,
                 loop_closure=None, loop_min_gap=32, loop_min_inliers=12, loop_cooldown=32, loop_iterations=10, loop_weight=1.0,
                 model_ratio=0.40, rotation_eps=0.02, normal_margin=0.01, world_upkeep=None, world_merge=True, world_merge_thresh=None,
                 world_cull_age=None, world_cull_min_views=3, world_high_water=None, world_low_water=None, ground_truth=None,
                 gt_index=None, trajectory_eval=None, eval_align="sim3", eval_table="trajectory", world_classes=None,
                 world_keep_classes=None, world_drop_classes=None):
        stage = (intrinsics, geometric_check, landmark_params)
        _check_mode("world_classes", world_classes, "observe", "match")
        if world_classes is None:
            if world_keep_classes is not None or world_drop_classes is not None:
                raise ValueError("world_keep_classes / world_drop_classes need world_classes='match'")
        else:
            if world_map is None:
                raise ValueError("world_classes needs world_map: the votes are on that map's landmarks")
            if world_keep_classes is not None or world_drop_classes is not None:
                if world_classes != "match":
                    raise ValueError("world_keep_classes / world_drop_classes need world_classes='match'")
                world_keep_classes = L.class_mask(keep=world_keep_classes, drop=world_drop_classes, n_classes=L.CLASS_NONE)
        _check_mode("trajectory_eval", trajectory_eval, "observe")
        if eval_table not in ("trajectory", "world"):
            raise ValueError("eval_table must be 'trajectory' or 'world' (got %r)" % (eval_table,))
        if eval_align not in L.TRAJ_MODES:
            raise ValueError("eval_align must be one of %s (got %r)" % (sorted(L.TRAJ_MODES), eval_align))
        if trajectory_eval is not None or ground_truth is not None:
            if intrinsics is None:
                raise ValueError("trajectory evaluation needs intrinsics: it scores the trajectory of a calibrated camera")
            if ground_truth is None:
                raise ValueError("trajectory_eval needs ground_truth: float64 [N, 12] camera-to-world rows (R | C)")
            ground_truth = np.ascontiguousarray(ground_truth, dtype=np.float64)
            if ground_truth.ndim != 2 or ground_truth.shape[1] != L.TRAJ_GT_WORDS or ground_truth.shape[0] < 1:
                raise ValueError("ground_truth must be [N >= 1, %d] (got %s)" % (L.TRAJ_GT_WORDS, list(ground_truth.shape)))
            if gt_index is not None:
                gt_index = np.ascontiguousarray(gt_index, dtype=np.int32)
                if gt_index.shape != (int(trajectory_rows),):
                    raise ValueError("gt_index must hold trajectory_rows = %d entries (got %s)" % (int(trajectory_rows),
                                                                                                 list(gt_index.shape)))
            if trajectory_eval is not None and eval_table == "world" and world_map is None:
                raise ValueError("eval_table='world' needs world_map: it scores world_trajectory()")
        elif gt_index is not None:
            raise ValueError("gt_index needs ground_truth")
        _check_mode("geometric_check", geometric_check, "fundamental", "homography", "auto")
        if geometric_check == "auto":
            if intrinsics is None:
                raise ValueError("geometric_check='auto' needs intrinsics: it chooses between two poses, not two filters")
            if not (0.0 <= model_ratio <= 1.0 and rotation_eps >= 0.0 and normal_margin >= 0.0):
                raise ValueError("0 <= model_ratio <= 1 and non-negative rotation_eps and normal_margin required")
        _check_mode("world_map", world_map, "observe", "relocalise")
        if world_map is not None:
            _check_stage("world_map", "the landmarks come from the trajectory's cameras", *stage, (
                lambda: not (world_thresh >= 0.0 and np.isfinite(world_thresh)) or int(world_min_inliers) < 4,
                "world_thresh must be finite and non-negative, world_min_inliers at least 4"), (
                lambda: not 1 <= int(world_cap) <= L.WORLD_MAX_ROWS or int(world_patience) < 0,
                "1 <= world_cap <= %d and world_patience >= 0 required" % L.WORLD_MAX_ROWS))
        _check_mode("world_upkeep", world_upkeep, "on")
        if world_upkeep is not None:
            if world_map is None:
                raise ValueError("world_upkeep needs world_map: it is the upkeep of that map")
            if world_merge_thresh is None:
                world_merge_thresh = world_thresh
            if world_cull_age is None:
                world_cull_age = max_length
            if world_high_water is None:
                world_high_water = int(world_cap) - int(world_cap) // 16
            if world_low_water is None:
                world_low_water = min(int(world_cap) - int(world_cap) // 8, int(world_high_water)) if world_high_water >= 0 else 0
            _check_stage("world_upkeep", "the merge reprojects the map's points into the trajectory's newest camera", *stage, (
                lambda: bool(world_merge) and not (world_merge_thresh >= 0.0 and np.isfinite(world_merge_thresh)),
                "world_merge_thresh must be finite and non-negative"), (
                lambda: world_high_water >= 0 and not 0 <= int(world_low_water) <= int(world_high_water) <= int(world_cap),
                "0 <= world_low_water <= world_high_water <= world_cap required (or a negative world_high_water for no eviction)"))
        _check_mode("loop_closure", loop_closure, "observe", "apply")
        if loop_closure is not None:
            if world_map is None:
                raise ValueError("loop_closure needs world_map: the closure is detected from the frame's matches against the map")
            if int(loop_min_gap) < 1 or int(loop_min_inliers) < 4 or int(loop_cooldown) < 0:
                raise ValueError("loop_min_gap must be at least 1, loop_min_inliers at least 4, loop_cooldown non-negative")
            if not 1 <= int(loop_iterations) <= L.LOOP_MAX_ITERATIONS:
                raise ValueError("1 <= loop_iterations <= %d required" % L.LOOP_MAX_ITERATIONS)
            if not (loop_weight > 0.0 and np.isfinite(loop_weight)):
                raise ValueError("loop_weight must be finite and positive")
            if int(trajectory_rows) < 2:
                raise ValueError("loop_closure needs trajectory_rows >= 2")
        _check_mode("absolute_pose", absolute_pose, "observe", "repair")
        if absolute_pose is not None:
            _check_stage("absolute_pose", "the landmarks come from the trajectory's cameras", *stage, (
                lambda: not (absolute_thresh >= 0.0 and np.isfinite(absolute_thresh)) or int(absolute_min_inliers) < 4,
                "absolute_thresh must be finite and non-negative, absolute_min_inliers at least 4"))
        _check_mode("bundle_adjust", bundle_adjust, "observe", "apply")
        if bundle_adjust is not None:
            _check_stage("bundle_adjust", "the cameras come from the trajectory", *stage, (
                lambda: not 1 <= int(bundle_iterations) <= L.BA_MAX_ITERATIONS or int(bundle_every) < 1,
                "1 <= bundle_iterations <= %d and bundle_every >= 1 required" % L.BA_MAX_ITERATIONS))
        if intrinsics is not None:
            if geometric_check not in ("fundamental", "auto"):
                raise ValueError("intrinsics need geometric_check='fundamental' or 'auto': the pose is read off the fundamental "
                                 "matrix (or, with 'auto', the homography where the frame obeys that)")
            k = np.asarray(intrinsics, dtype=np.float64)
            if k.shape == (4,):
                k = np.stack([k, k])
            if k.shape != (2, 4) or not np.all(np.isfinite(k)) or not np.all(k[:, :2] > 0.0):
                raise ValueError("intrinsics must be (fx, fy, cx, cy), or a pair of them, with positive focal lengths")
            if trajectory_rows < 1:
                raise ValueError("trajectory_rows must be positive")
            intrinsics = k
        if geometric_check is not None and not (check_thresh >= 0.0 and min_inliers >= 0):
            raise ValueError("check_thresh and min_inliers must be non-negative")
        if max_length < 2:
            raise ValueError("max_length must be greater than or equal to 2.")
        if max_length > L.TRACK_MAX_LENGTH:
            raise ValueError("max_length must be at most %d (SSP_TRACK_MAX_LENGTH)." % L.TRACK_MAX_LENGTH)
        self.maxl = int(max_length)
        self.nn_thresh = nn_thresh
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.last_desc = None
        self.max_score = 9999
        self.matches = None
        self.last_pts = None
        self.mscores = None
        self._host_pts = [np.zeros((2, 0)) for _ in range(self.maxl)]  # None = only on the device (update_device)
        self._frames = 0          # updates so far: frame f lives in ring slot f % maxl
        self._cap = 0             # points per frame the device buffers hold
        self._table = self._spare = None
        self._pts = None          # float64 [maxl, cap, 2] ring of (x, y)
        self._desc = None         # float32 [2, cap, 256]: the descriptors of frame f in slot f % 2
        self._counts = None       # int32 [2]: their counts; a cleared / missing previous frame reads _zero instead
        self._zero = None
        self._prev_ok = False     # the previous frame's descriptors take part in the next match
        self._pending = None      # device (match, n_match, had_prev) whose numpy form get_matches() has not been asked for yet
        self.class_consistent = bool(class_consistent)
        self._cls = None          # uint8 [2, cap] beside _desc (class_consistent only)
        self.geometric_check = geometric_check
        self.check_thresh, self.min_inliers, self.check_seed = float(check_thresh), int(min_inliers), int(check_seed)
        self._seed = None         # int64 [1] on the device: the seed of the next frame's check
        self._geometry = None
        self.intrinsics = intrinsics     # float64 [2, 4] (numpy) or None
        self.trajectory_rows = int(trajectory_rows)
        self._intr = None         # float64 [1, 2, 4] on the device
        self._traj_state = self._traj_table = None
        self._pose_prev = None    # (pose dict, unfiltered match [1, cap, 3], n_match) of the previous frame's pair
        self.model_ratio, self.rotation_eps, self.normal_margin = float(model_ratio), float(rotation_eps), float(normal_margin)
        self._normals_prev = None # float64 [1, 2, 3]: the previous frame's normals2 ("auto": the next frame's prior)
        self._lm = None           # lib.landmark_buffers of the table's row_cap (landmarks_device; allocated on first use)
        self.absolute_pose = absolute_pose
        self.absolute_thresh, self.absolute_min_inliers = float(absolute_thresh), int(absolute_min_inliers)
        self.landmark_params = (int(landmark_params[0]), float(landmark_params[1]), float(landmark_params[2]))
        self._abs_lm = None       # lib.landmark_buffers of the tracker's own: the landmarks of the window ending at the previous frame
        self._abs_have = False    # _abs_lm holds such landmarks
        self._abs = None          # lib.pnp_buffers of one problem
        self._abs_table = None    # float64 [trajectory_rows, POSE_ROW_WORDS]: absolute_trajectory()
        self.bundle_adjust = bundle_adjust
        self.bundle_iterations, self.bundle_every = int(bundle_iterations), int(bundle_every)
        self._ba_lm = None        # lib.landmark_buffers of the tracker's own: what the bundle adjustment starts from
        self._ba = None           # lib.ba_buffers: its result
        self._ba_ran = False
        self.world_map_mode = world_map
        self.world_cap, self.world_patience = int(world_cap), int(world_patience)
        self.world_thresh, self.world_min_inliers = float(world_thresh), int(world_min_inliers)
        self._world = None        # lib.world_buffers: the map
        self._world_lm = None     # lib.landmark_buffers of the tracker's own: the landmarks of the window ending at the newest frame
        self._world_pnp = None    # lib.pnp_buffers of one problem
        self._world_match = None  # (match [cap, 3], n_match [1]) of the newest frame against the map
        self._world_table = None  # float64 [trajectory_rows, POSE_ROW_WORDS]: world_trajectory()
        self.world_upkeep = world_upkeep
        if world_upkeep is not None:
            self.world_upkeep_params = dict(merge=bool(world_merge), merge_thresh=float(world_merge_thresh), cull_age=int(world_cull_age),
                                            cull_min_views=int(world_cull_min_views), high_water=int(world_high_water),
                                            low_water=int(world_low_water))
        self._upkeep = None       # lib.world_upkeep_buffers: the scratch, the last report, the running totals
        self.world_classes = world_classes
        self.world_keep_mask = world_keep_classes      # eight 32-bit words (lib.class_mask), or None: every class
        self._world_votes = None  # lib.world_class_buffers: the class votes per track id
        self._world_cls = None    # uint8 [cap]: the classes of the newest frame's points (world_classes only)
        self.loop_closure = loop_closure
        self.loop_min_gap, self.loop_min_inliers, self.loop_cooldown = int(loop_min_gap), int(loop_min_inliers), int(loop_cooldown)
        self.loop_iterations, self.loop_weight = int(loop_iterations), float(loop_weight)
        self._loop = None         # lib.loop_buffers: the edge table, its state, the pose graph's outputs
        self._loop_pnp = None     # lib.pnp_buffers of one problem: the pose against the old rows
        self._loop_log = None     # float64 [trajectory_rows, 11]: the candidate record and the graph's costs and status per frame
        self._loop_seed = None    # the frame's check seed
        self.ground_truth, self.gt_index = ground_truth, gt_index   # numpy, or None
        self.trajectory_eval, self.eval_align, self.eval_table = trajectory_eval, eval_align, eval_table
        self._evaluators = {}     # trajectory_evaluation.TrajectoryEvaluator per option set of evaluate_trajectory
        self._eval = None         # the buffers of the per-frame log under trajectory_eval="observe"
        self._eval_log = None     # float64 [trajectory_rows, 8]: ATE rmse, mean, max, s, n_valid, status, two spare

    # ---- device buffers -------------------------------------------------------------------------------------------
    def _ensure(self, n):
        """Buffers for frames of at least n points (grown by copying: the table's rows keep their places)."""
        if n <= self._cap:
            return
        if n > L.MATCH_MAX_POINTS:
            raise ValueError("at most %d points per frame (got %d)" % (L.MATCH_MAX_POINTS, n))
        cap = min(L.MATCH_MAX_POINTS, max(n, 2 * self._cap, 1024))
        dev = self.device
        table, spare = L.track_table(self.maxl, cap, dev), L.track_table(self.maxl, cap, dev)
        pts = torch.zeros(self.maxl, cap, 2, dtype=torch.float64, device=dev)
        desc = torch.zeros(2, cap, 256, dtype=torch.float32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        if self._cap:
            rows = self._table["row_cap"]
            for k in ("ids", "tid", "score"):
                table[k][:rows] = self._table[k]
            table["state"].copy_(self._table["state"])
            pts[:, :self._cap] = self._pts
            desc[:, :self._cap] = self._desc
            counts.copy_(self._counts)
        if self.class_consistent:
            cls = torch.full((2, cap), L.CLASS_NONE, dtype=torch.uint8, device=dev)
            if self._cap:
                cls[:, :self._cap] = self._cls
            self._cls = cls
        if self.world_classes is not None:
            self._world_cls = torch.full((cap,), L.CLASS_NONE, dtype=torch.uint8, device=dev)
        self._table, self._spare, self._pts, self._desc, self._counts, self._cap = table, spare, pts, desc, counts, cap
        self._zero = torch.zeros(1, dtype=torch.int32, device=dev)

    def _slots(self):
        """(ring slot of the newest frame, desc slot of the newest frame)."""
        return (self._frames - 1) % self.maxl, (self._frames - 1) % 2

    def _advance(self, xy, count, desc, cls=None):
        """The device half of an update: xy float64 [n, 2], count int32 [1], desc float32 [n, 256] device tensors (rows past
        the count are ignored), cls uint8 [n] with class_consistent.  Returns the device (match, n_match) of the new frame
        against the previous one and whether the previous frame's descriptors took part."""
        n = xy.shape[0]
        if n > L.MATCH_MAX_POINTS:  # a capacity, not a count: the matcher takes the first MATCH_MAX_POINTS rows at most
            n = L.MATCH_MAX_POINTS
            xy, desc, count = xy[:n], desc[:n], count.clamp(max=n)
            cls = cls[:n] if cls is not None else None
        self._ensure(max(n, 1))
        self._frames += 1
        slot, dslot = self._slots()
        self._pts[slot, :n] = xy
        self._desc[dslot, :n] = desc
        self._counts[dslot:dslot + 1] = count
        if self.class_consistent:
            self._cls[dslot, :n] = cls
        if self.world_classes is not None:
            self._world_cls[:n] = cls
        m, nm = self._match_device()
        if self.geometric_check is not None:
            m, nm = self._check_device(m, nm)
        self._track_device(m, nm)
        if self.bundle_adjust is not None:
            self._bundle_device()
        if self.absolute_pose is not None:
            self._keep_landmarks_device()
        if self.world_map_mode is not None:
            self._world_insert_device()
        if self.trajectory_eval is not None:
            self._eval_observe_device()
        had_prev, self._prev_ok = self._prev_ok, True
        return m, nm, had_prev

    def _match_device(self):
        _, dslot = self._slots()
        prev = self._counts[1 - dslot:2 - dslot] if self._prev_ok else self._zero
        if self.class_consistent:
            m, nm = L.op_match_two_way(self._desc[1 - dslot:2 - dslot], prev, self._desc[dslot:dslot + 1],
                                       self._counts[dslot:dslot + 1], self.nn_thresh, cls1=self._cls[1 - dslot:2 - dslot],
                                       cls2=self._cls[dslot:dslot + 1])
            return m[0], nm
        m, nm = L.op_match_two_way(self._desc[1 - dslot:2 - dslot], prev, self._desc[dslot:dslot + 1],
                                   self._counts[dslot:dslot + 1], self.nn_thresh)
        return m[0], nm

    def _check_device(self, m, nm):
        """The geometric check of the newest frame's matches against the previous frame: (match, n_match) of the inliers."""
        if self._seed is None:
            self._seed = torch.full((1,), self.check_seed + self._frames - 1, dtype=torch.int64, device=self.device)
        slot, _ = self._slots()
        pslot = (slot - 1) % self.maxl
        p1, p2 = self._pts[pslot:pslot + 1], self._pts[slot:slot + 1]
        gh = None
        if self.geometric_check in ("fundamental", "auto"):
            g = L.op_epipolar_ransac(p1, p2, m[None], nm, self._seed, thresh=self.check_thresh)
        if self.geometric_check in ("homography", "auto"):
            pad = torch.zeros(2, self._cap, 1, dtype=torch.float64, device=self.device)
            p12 = torch.cat([torch.cat([p1, p2]), pad], dim=2)
            gh = L.op_eval_ransac(p12[0:1], p12[1:2], m[None], nm, self._seed)
            if self.geometric_check == "homography":
                g, gh = gh, None
        seed, self._seed = self._seed, self._seed + 1
        if self.intrinsics is not None:
            g = self._pose_device(g, p1, p2, m[None], nm, gh)
        if self.absolute_pose is not None:
            g = self._absolute_device(g, m, nm, p2[0], seed)
        if self.world_map_mode is not None:
            g = self._world_device(g, p2[0], seed)
        self._geometry = g
        return L.op_filter_matches(m, nm, g["mask"], g["status"], g["n_inliers"], self.min_inliers)

    def _pose_device(self, g, p1, p2, m, nm, gh=None):
        """The pose of the newest frame against the previous one and its trajectory row; returns g with the pose keys.  gh: the
        homography RANSAC of the frame ("auto"): the model is selected, a frame that obeys the homography gets its pose written
        over the fundamental matrix's, and mask / n_inliers / status become the selected model's."""
        if self._intr is None:
            self._intr = torch.from_numpy(self.intrinsics[None].copy()).to(self.device)
            self._traj_state = L.pose_state(self.device)
            self._traj_table = L.pose_table(self.trajectory_rows, self.device)
        pose = L.op_two_view_pose(g, p1, p2, m, nm, self._intr)
        if gh is not None:
            sel = L.op_model_select(g, gh, p1, p2, m, nm, model_ratio=self.model_ratio)
            L.op_homography_pose(gh, p1, p2, m, nm, self._intr, prior=self._normals_prev, rotation_eps=self.rotation_eps,
                                 normal_margin=self.normal_margin, use_h=sel["use_h"], out=pose)
            self._normals_prev = pose["normals2"]
            g = dict(g, mask=sel["mask"], n_inliers=sel["n_inliers"], status=sel["status"], scores=sel["scores"], H=gh["H"],
                     h_mask=gh["mask"], h_n_inliers=gh["n_inliers"], h_status=gh["status"])
        prev, m_prev, nm_prev = self._pose_prev if self._pose_prev is not None else (None, None, None)
        L.op_pose_chain(prev, pose, m_prev, m, nm_prev, nm, self._traj_state, self._traj_table)
        self._pose_prev = (pose, m, nm)
        g = dict(g)
        g.update(("pose_status" if k == "status" else k, v) for k, v in pose.items())
        return g

    def _absolute_device(self, g, m, nm, pts_new, seed):
        """The absolute pose of the newest frame from the landmarks kept after the previous one, its row of absolute_trajectory()
        and, with "repair", the repair of the newest trajectory row; returns g with the abs_* keys."""
        if self._abs_table is None:
            self._abs_table = L.pose_table(self.trajectory_rows, self.device)
        a = self._pnp_one("_abs", m.shape[0])
        g = dict(g)
        if self._abs_have:            # (kept at the row_cap of the frame before: a landmark names its point by index, not by row)
            corr, n = L.op_landmark_matches(self._abs_lm["landmarks"], self._abs_lm["n_landmarks"], m, nm, pts_new, out=a)
            res = L.op_pnp_ransac(a["corr"], n[0:1], self._intr[0, 1:2], seed, thresh=self.absolute_thresh,
                                  min_inliers=self.absolute_min_inliers, out=a)
            if self.absolute_pose == "repair":
                L.op_pose_repair(res, self._traj_state, self._traj_table)
        else:                         # no landmarks yet: the row of a frame without a pose
            res = _pnp_no_pose(a)
        _write_pose_row(self._abs_table, self._frames - 1, res, a["n"][0, 1:2])
        g.update(("abs_" + k, v) for k, v in res.items())
        g["abs_corr"], g["abs_n_corr"] = a["corr"][0], a["n"][0]
        return g

    def _pnp_one(self, name, cap):
        """The tracker's lib.pnp_buffers `name` of one problem with room for cap correspondences (allocated again when cap changed)."""
        a = getattr(self, name)
        if a is None or a["corr"].shape[1] != cap:
            a = L.pnp_buffers(1, cap, self.device)
            setattr(self, name, a)
        return a

    def _window_rows(self, name, min_views, min_parallax_deg, max_reproj):
        """The window ending at the newest frame into the tracker's lib.landmark_buffers `name` (allocated again when the table's
        row_cap changed): its cameras from the trajectory and the triangulation of every track under them.  Returns (cams, rows)."""
        lm = getattr(self, name)
        if lm is None or lm["status"].shape[0] != self._table["row_cap"]:
            lm = L.landmark_buffers(self.maxl, self._table["row_cap"], self.device)
            setattr(self, name, lm)
        cams = L.op_map_window(self._traj_state, self._traj_table, self._intr[0, 1:2], self.maxl, n_frames=self._frames, out=lm)
        rows = L.op_triangulate_tracks(self._table, self._pts, self._frames % self.maxl, cams, min_views, min_parallax_deg, max_reproj,
                                       out=lm)
        return cams, rows

    def _window_landmarks(self, name, min_views, min_parallax_deg, max_reproj):
        """_window_rows and the selection of the accepted rows into the same buffers: (landmarks, n_landmarks)."""
        _, rows = self._window_rows(name, min_views, min_parallax_deg, max_reproj)
        return L.op_landmarks_select(self._table, rows, out=getattr(self, name))

    def _keep_landmarks_device(self):
        """The landmarks of the window ending at the newest frame into the tracker's own buffers (after _track_device)."""
        self._abs_have = self._frames >= 2 and self._traj_table is not None
        if self._abs_have:
            self._window_landmarks("_abs_lm", *self.landmark_params)

    def _world_device(self, g, pts_new, seed):
        """The newest frame against the world map: match, join, P3P, its row of world_trajectory() and, with "relocalise", the
        repair of the newest trajectory row; returns g with the world_* keys.  An empty map gives the status-1 row."""
        _, dslot = self._slots()
        cap = self._cap
        if self._world is None:
            self._world = L.world_buffers(self.world_cap, device=self.device)
            self._world_table = L.pose_table(self.trajectory_rows, self.device)
            if self.world_classes is not None:
                self._world_votes = L.world_class_buffers(self._world["tid_cap"], self.device)
        if self._world_match is None or self._world_match[0].shape[0] != cap:
            old, self._world_match = self._world_match, (torch.zeros(cap, 3, dtype=torch.float32, device=self.device),
                                                         torch.zeros(1, dtype=torch.int32, device=self.device))
            if old is not None:       # grown by copying: the matcher leaves the rows past n_match as they were
                self._world_match[0][:old[0].shape[0]] = old[0]
        w, a, count = self._world, self._pnp_one("_world_pnp", cap), self._counts[dslot:dslot + 1]
        self._loop_seed = seed
        if self.world_classes == "match":
            m, nm = L.op_match_world_classes(w, self._world_votes, self._desc[dslot], self._world_cls, count, self.nn_thresh,
                                             map_keep=self.world_keep_mask, out=self._world_match)
        else:
            m, nm = L.op_match_world(w, self._desc[dslot], count, self.nn_thresh, out=self._world_match)
        corr, n = L.op_world_correspondences(w, m, nm, pts_new, count, out=a)
        res = L.op_pnp_ransac(a["corr"], n[0:1], self._intr[0, 1:2], seed, thresh=self.world_thresh,
                              min_inliers=self.world_min_inliers, out=a)
        if self.world_map_mode == "relocalise":
            L.op_world_repair(w, res, self._traj_state, self._traj_table)
        _write_pose_row(self._world_table, self._frames - 1, res, a["n"][0, 1:2])
        g = dict(g)
        g.update(("world_" + k, v) for k, v in res.items())
        g["world_corr"], g["world_n_corr"], g["world_match"], g["world_n_match"] = a["corr"][0], a["n"][0], m, nm
        return g

    def _world_insert_device(self):
        """The landmarks of the window ending at the newest frame into the world map (after _track_device and the bundle
        adjustment): map window, triangulate, select, insert."""
        if self._frames < 2 or self._traj_table is None or self._world is None:
            return
        slot, dslot = self._slots()
        lms, n_lms = self._window_landmarks("_world_lm", *self.landmark_params)
        if self.loop_closure is not None:
            self._loop_device(lms, n_lms)
            if self.loop_closure == "apply":      # once more, unconditionally: the rows inserted stand under the corrected cameras
                lms, n_lms = self._window_landmarks("_world_lm", *self.landmark_params)
        L.op_world_insert(self._world, lms, n_lms, self._desc[dslot], self._counts[dslot:dslot + 1], self._traj_table, self._frames,
                          self.world_patience)
        if self.world_classes is not None:        # beside the insert, before the upkeep: the votes are per track id, not per slot
            L.op_track_class_votes(self._world_votes, lms, n_lms, self._world_cls, self._counts[dslot:dslot + 1])
        if self.world_upkeep is not None:         # after loop closure and its write-back: both saw the map the frame was matched with
            if self._upkeep is None:
                self._upkeep = L.world_upkeep_buffers(self.world_cap, self.device)
            m, nm = self._world_match
            L.op_world_upkeep(self._world, m, nm, lms, n_lms, self._pts[slot], self._counts[dslot:dslot + 1], self._traj_table,
                              self._frames, self._intr[0, 1:2], self._upkeep, **self.world_upkeep_params)
            self._geometry = dict(self._geometry, world_upkeep_report=self._upkeep["report"])

    def _loop_device(self, lms, n_lms):
        """Loop closure of the newest frame, between the select and the insert: the frame's map matches
        against the old rows, P3P, the edge, the pose graph and, with "apply", the write-back.  last_geometry() gains loop_* keys."""
        f = self._frames - 1
        slot, dslot = self._slots()
        cap = self._cap
        if self._loop is None or self._loop["cap"] != cap:
            new = L.loop_buffers(cap, self.trajectory_rows, self.device)
            if self._loop is not None:          # the match tables grew: the edges and the counters stay
                new["edges"].copy_(self._loop["edges"])
                new["state"].copy_(self._loop["state"])
            self._loop = new
        if self._loop_log is None:
            self._loop_log = torch.zeros(self.trajectory_rows, 11, dtype=torch.float64, device=self.device)
        lp, w, count = self._loop, self._world, self._counts[dslot:dslot + 1]
        m, nm = self._world_match
        L.op_loop_correspondences(w, m, nm, self._pts[slot], count, lms, n_lms, f, self.loop_min_gap, lp)
        res = L.op_pnp_ransac(lp["corr"], lp["n"][0:1], self._intr[0, 1:2], self._loop_seed, thresh=self.world_thresh,
                              min_inliers=self.loop_min_inliers, out=self._pnp_one("_loop_pnp", cap))
        g = dict(self._geometry)
        g.update(("loop_" + k, v) for k, v in res.items())
        g["loop_corr"], g["loop_xnew"], g["loop_n_corr"] = lp["corr"], lp["xnew"], lp["n"]
        g["loop_cand"], g["loop_info"], g["loop_state"] = lp["cand"], lp["info"], lp["state"]
        self._geometry = g
        if f >= self.trajectory_rows:           # no row in the table: nothing to close
            return
        L.op_loop_edge(w, res, self._traj_table, f, lp, self.loop_min_inliers, self.loop_cooldown, self.loop_weight)
        L.op_pose_graph(self._traj_table, f, lp, self.loop_iterations)
        if self.loop_closure == "apply":
            L.op_loop_apply(w, self._traj_state, self._traj_table, f, lp)
        row = self._loop_log[f]
        row[0:8] = lp["cand"][0:8]
        row[8:10] = lp["info"][1:3]
        row[10:11] = lp["info"][0:1]

    def loop_edges_device(self):
        """(edges float64 [LOOP_MAX_EDGES, LOOP_EDGE_WORDS] rows (i, j, R [9], t [3], log sigma, weight), state int32
        [LOOP_STATE_WORDS]; state[0] rows are in use) on the device; None without loop_closure or before the third frame.  No
        synchronisation."""
        if self._loop is None:
            return None
        return self._loop["edges"], self._loop["state"]

    def loop_closures(self):
        """One numpy row per accepted edge: (frame, anchor, inliers, sigma, angle of R_c in radians, |t_c|, cost before, cost
        after, status of the pose graph); one host synchronisation.  Zero rows without loop_closure."""
        if self._loop_log is None:
            return np.zeros((0, 9))
        log = self._loop_log[:min(self._frames, self.trajectory_rows)].cpu().numpy()
        log = log[log[:, 7] != 0.0]
        return np.ascontiguousarray(log[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]])

    def world_trajectory(self):
        """(table, n_frames) on the device in absolute_trajectory()'s layout: rows (Rw [9], C [3], n_inliers, rms, status, n_corr),
        one per frame given so far: the camera of that frame against the world map as it stood before the frame (status 1, Rw = I,
        C = 0 where there was no pose).  None without world_map or before the first frame.  No synchronisation."""
        if self._world_table is None:
            return None
        return self._world_table, self._traj_state[0:1]

    def world_map_device(self):
        """The map's device buffers (the dict of lib.world_buffers; "state"[0] rows are in use), None without world_map or before
        the first frame.  No synchronisation."""
        return self._world

    def world_upkeep_report(self):
        """The running totals of the map's upkeep as numpy int64 [4] = (rows merged, culled, evicted, calls); one host
        synchronisation.  Zeros without world_upkeep or before its first call."""
        if self._upkeep is None:
            return np.zeros(4, dtype=np.int64)
        return self._upkeep["totals"].cpu().numpy()

    def world_map(self, classes=False):
        """The map as numpy: (rows float64 [n_rows, 8] = (tid, X, Y, Z, n_views, rms, first_frame, last_frame), descriptors float32
        [n_rows, 256]); one host synchronisation.  Zero rows without world_map or before the first frame.  classes=True (needs
        world_classes): the rows get a ninth column, the class voted for the row's track (lib.CLASS_NONE while it has none)."""
        if classes and self.world_classes is None:
            raise ValueError("world_map(classes=True) needs world_classes")
        if self._world is None:
            return np.zeros((0, 9 if classes else 8)), np.zeros((0, 256), dtype=np.float32)
        w = self._world
        n = min(max(int(w["state"][0].item()), 0), w["map_cap"])
        cols = [w["tid"][:n].double()[:, None], w["X"][:n], w["n_views"][:n].double()[:, None], w["rms"][:n, None],
                w["first_frame"][:n].double()[:, None], w["last_frame"][:n].double()[:, None]]
        if classes:
            cols.append(self.world_classes_device()[:n].double()[:, None])
        return torch.cat(cols, dim=1).cpu().numpy(), w["desc"][:n].cpu().numpy()

    def world_classes_device(self):
        """uint8 [world_cap] on the device: the class voted for the track of every map row in use, lib.CLASS_NONE while it has none and
        past the rows in use (lib.op_world_classes); None without world_classes or before the first frame.  No synchronisation."""
        if self._world_votes is None:
            return None
        return L.op_world_classes(self._world, self._world_votes)

    def reset_world_classes(self):
        """Zeroes the class votes (a cleared or re-anchored map keeps them: a track id names one scene track for its whole life)."""
        if self._world_votes is not None:
            self._world_votes["votes"].zero_()

    def _bundle_device(self):
        """The bundle adjustment of the window ending at the newest frame (after _track_device): map window, triangulate, adjust
        and, with "apply", the write-back into the trajectory."""
        row_cap = self._table["row_cap"]
        if self._ba is None:
            self._ba = L.ba_buffers(self.maxl, row_cap, self.device)
            self._ba["info"][0:1] = L.BA_NOTHING
            self._ba["info"][7:8] = 1e-4
        elif self._ba["rms"].shape[0] != row_cap:   # the table grew (_ensure): so does the newest adjustment, its rows in their places
            old, self._ba = self._ba, L.ba_buffers(self.maxl, row_cap, self.device)
            rows = old["rms"].shape[0]
            self._ba["info"].copy_(old["info"])
            self._ba["cams"].copy_(old["cams"])
            self._ba["X"][:rows] = old["X"]
            self._ba["rms"][:rows] = old["rms"]
        if self._frames >= 2 and self._traj_table is not None and self._frames % self.bundle_every == 0:
            cams, rows = self._window_rows("_ba_lm", *self.landmark_params)
            res = L.op_bundle_adjust(self._table, self._pts, self._frames % self.maxl, cams, rows, self.bundle_iterations, out=self._ba)
            if self.bundle_adjust == "apply":
                L.op_ba_apply(res, self._traj_state, self._traj_table, self.maxl, n_frames=self._frames)
            self._ba_ran = True
        if self._geometry is not None:
            self._geometry = dict(self._geometry, ba_info=self._ba["info"])

    def bundle_adjusted(self):
        """(cams float64 [max_length, lib.CAM_WORDS], X float64 [row_cap, 3], rms float64 [row_cap], info float64
        [lib.BA_INFO_WORDS]) of the newest bundle adjustment on the device (lib.op_bundle_adjust; X and rms are aligned with the
        track table's rows at that frame), None without bundle_adjust or before it first ran.  No synchronisation."""
        if not self._ba_ran:
            return None
        return self._ba["cams"], self._ba["X"], self._ba["rms"], self._ba["info"]

    def absolute_trajectory(self):
        """(table, n_frames) on the device: float64 [trajectory_rows, lib.POSE_ROW_WORDS] rows (Rw [9], C [3], n_inliers, rms,
        status, n_corr), one per frame given so far: the camera of that frame against the landmarks of the window ending at the
        frame before it (status 1, Rw = I, C = 0 where there was none), and trajectory()'s float64 [1] number of rows.  None
        without absolute_pose or before the first frame.  No synchronisation."""
        if self._abs_table is None:
            return None
        return self._abs_table, self._traj_state[0:1]

    def trajectory(self):
        """(table, n_frames) on the device: float64 [trajectory_rows, lib.POSE_ROW_WORDS] rows (Rw [9], C [3], s, n_shared, flags,
        ratio), one per frame given so far (row 0, the first frame, is the world: identity, flag bit 0), and the float64 [1]
        number of rows written.  World = the first camera; C is the camera centre with the first baseline as the unit.  None
        without intrinsics or before the first frame.  No synchronisation."""
        if self._traj_table is None:
            return None
        return self._traj_table, self._traj_state[0:1]

    # ---- landmarks ------------------------------------------------------------------------------
    def landmark_rows_device(self, min_views=2, min_parallax_deg=1.0, max_reproj=2.0):
        """The N-view triangulation of every row of the track table (lib.op_map_window + lib.op_triangulate_tracks): the device
        dict {"X": float64 [row_cap, 3], "n_views": int32, "rms": float64, "cos_parallax": float64, "status": int32 [row_cap]}
        aligned with `table`'s rows (rows at or past its n_rows are stale).  World = the first camera of the sequence, unit = the
        first baseline.  After a break in the chain (a frame without a pose, a carried scale) only the frames of the newest
        consistent window are used, and the points are in that window's own scale.  Needs `intrinsics`, and one camera: a fixed
        (previous, new) pair of two different cameras cannot describe more than two views (ValueError; lib.op_map_window takes
        per-frame intrinsics).  Before the second frame every array has zero rows.  No host copy, no synchronisation; the
        buffers are allocated once per capacity and overwritten by the next call."""
        if not self._landmarks_wanted(min_views):
            f64, i32 = dict(dtype=torch.float64, device=self.device), dict(dtype=torch.int32, device=self.device)
            return {"X": torch.zeros(0, 3, **f64), "n_views": torch.zeros(0, **i32), "rms": torch.zeros(0, **f64),
                    "cos_parallax": torch.zeros(0, **f64), "status": torch.zeros(0, **i32)}
        return self._window_rows("_lm", min_views, min_parallax_deg, max_reproj)[1]

    def _landmarks_wanted(self, min_views):
        """The checks of the landmark calls; False before the second frame (nothing to triangulate yet)."""
        if self.intrinsics is None:
            raise ValueError("landmarks need intrinsics (and geometric_check='fundamental'): the cameras come from the trajectory")
        _check_one_camera(self.intrinsics, "landmarks need ONE camera: a fixed (previous, new) pair of different intrinsics cannot "
                                           "describe more than two views (lib.op_map_window takes per-frame intrinsics)")
        if int(min_views) < 2:
            raise ValueError("min_views >= 2 required (got %d)" % min_views)
        return self._frames >= 2 and self._traj_table is not None

    def landmarks_device(self, min_views=2, min_parallax_deg=1.0, max_reproj=2.0):
        """The accepted landmarks on the device: (landmarks float64 [row_cap, lib.LANDMARK_WORDS] rows (track id, X, Y, Z,
        n_views, rms, cos_parallax, index of the track's point in the newest frame or -1) in table order, n_landmarks int32 [1]).
        A track is accepted when at least min_views retained frames of the newest consistent window see it, two of its rays are
        at least min_parallax_deg apart, it lies in front of every camera that sees it and its rms reprojection error is at most
        max_reproj pixels.  Frame, unit, errors and cost: landmark_rows_device.  Before the second frame: zero rows, n = 0."""
        if not self._landmarks_wanted(min_views):
            return (torch.zeros(0, L.LANDMARK_WORDS, dtype=torch.float64, device=self.device),
                    torch.zeros(1, dtype=torch.int32, device=self.device))
        return self._window_landmarks("_lm", min_views, min_parallax_deg, max_reproj)

    def landmarks(self, min_views=2, min_parallax_deg=1.0, max_reproj=2.0):
        """landmarks_device as numpy: float64 [M, lib.LANDMARK_WORDS] (one host synchronisation)."""
        return L.landmarks_to_numpy(*self.landmarks_device(min_views, min_parallax_deg, max_reproj))

    # ---- trajectory evaluation ---------------------------------------------------------------------
    def _eval_tables(self, which):
        """(table, rows given so far) of trajectory() / absolute_trajectory() / world_trajectory(), or None before it exists"""
        got = {"trajectory": self.trajectory, "absolute": self.absolute_trajectory, "world": self.world_trajectory}[which]()
        return None if got is None else (got[0], min(self._frames, self.trajectory_rows))

    def _eval_observe_device(self):
        """One row of the log for the newest frame, after all of its write-backs: the alignment of the frames so far, their
        absolute errors and the statistics of those (three launches and two small gathers; the first frame allocates, after it
        there is no host copy or synchronisation).  A frame before the table exists, or past trajectory_rows, leaves no row."""
        f = self._frames - 1
        e = self._eval
        if e is None:
            dev, rows = self.device, self.trajectory_rows
            e = self._eval = dict(traj=L.traj_eval_buffers(rows, 1, 1, rows, dev, n_stat=1),
                                  gt=torch.as_tensor(self.ground_truth).to(dev),
                                  index=None if self.gt_index is None else torch.as_tensor(self.gt_index).to(dev),
                                  n_frames=torch.zeros(1, dtype=torch.int32, device=dev),
                                  stat_words=torch.tensor([1, 2, 5], device=dev), sim_words=torch.tensor([0, 13, 14], device=dev))
            self._eval_log = torch.zeros(rows, 8, dtype=torch.float64, device=dev)
        got = self._eval_tables(self.eval_table)
        if got is None or f >= self.trajectory_rows:
            return
        table, n = got
        traj = e["traj"]
        e["n_frames"].fill_(n)
        sim = L.op_traj_align(table, e["n_frames"], e["gt"], traj, e["index"], self.eval_align)
        err_t, _, valid = L.op_traj_ape(table, e["n_frames"], e["gt"], traj, e["index"])
        stats = L.op_traj_stats(err_t, valid, traj["stats"][0])
        row = self._eval_log[f]
        row[0:3] = stats[0].index_select(0, e["stat_words"])
        row[3:6] = sim[0].index_select(0, e["sim_words"])
        if self._geometry is not None:
            self._geometry = dict(self._geometry, trajectory_eval=row)

    def trajectory_eval_log(self):
        """The per-frame log of trajectory_eval="observe" as numpy float64 [frames, 8]: (ATE rmse, mean, max of the frames so far
        under their own alignment, s, n_valid, status, two spare) per frame given so far; one host synchronisation.  Zero rows
        without it or before the first frame."""
        if self._eval_log is None:
            return np.zeros((0, 8))
        return self._eval_log[:min(self._frames, self.trajectory_rows)].cpu().numpy()

    def evaluate_trajectory(self, which=None, **options):
        """The trajectory so far against ground_truth, on demand: which = "trajectory" (default: eval_table), "absolute" or "world";
        options are TrajectoryEvaluator's (align: default eval_align; lengths, step, deltas, skip_flags).  Returns
        TrajectoryEvaluator.result()'s dict (one host copy), None before the table exists."""
        from .trajectory_evaluation import TrajectoryEvaluator
        if self.ground_truth is None:
            raise ValueError("evaluate_trajectory needs ground_truth (and intrinsics)")
        which = self.eval_table if which is None else which
        if which not in ("trajectory", "absolute", "world"):
            raise ValueError("which must be 'trajectory', 'absolute' or 'world' (got %r)" % (which,))
        got = self._eval_tables(which)
        if got is None:
            return None
        options.setdefault("align", self.eval_align)
        key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in options.items()))
        ev = self._evaluators.get(key)
        if ev is None:
            ev = self._evaluators[key] = TrajectoryEvaluator(self.ground_truth, self.gt_index, capacity=self.trajectory_rows,
                                                             device=self.device, **options)
        ev.evaluate(got[0], got[1])
        return ev.result()

    def last_geometry(self):
        """The device dict of the newest frame's geometric check (lib.op_epipolar_ransac or lib.op_eval_ransac), None before
        the first checked frame or without a check.  Its mask indexes the UNFILTERED matches of that frame.  With bundle_adjust
        it also holds "ba_info" (float64 [lib.BA_INFO_WORDS]) of the newest adjustment (status lib.BA_NOTHING before the first).
        With world_upkeep it holds "world_upkeep_report" (int32 [lib.WORLD_UPKEEP_REPORT_WORDS]) once the upkeep has been called, and
        the rows of "world_match" index the map as it stood before the frame's upkeep, which may have moved or removed them.
        With trajectory_eval it holds "trajectory_eval" (float64 [8]): the frame's row of the log."""
        return self._geometry

    def _track_device(self, m, nm):
        _, dslot = self._slots()
        out = L.op_track_update(self._table, m, nm, self._counts[dslot:dslot + 1], out=self._spare)
        self._table, self._spare = out, self._table

    # ---- the reference's interface --------------------------------------------------------------------------------
    def nn_match_two_way(self, desc1, desc2, nn_thresh):
        """desc1 [D,N1], desc2 [D,N2] unit columns -> float64 [3,L] (index in desc1, index in desc2, distance), rows of
        desc1 ascending.  Same checks and order as models/model_wrap.py:451-497 (an empty side returns before the
        nn_thresh check)."""
        assert desc1.shape[0] == desc2.shape[0]
        if desc1.shape[1] == 0 or desc2.shape[1] == 0:
            return np.zeros((3, 0))
        if nn_thresh < 0.0:
            raise ValueError("'nn_thresh' should be non-negative")
        if desc1.shape[0] != 256:
            raise ValueError("the device matcher takes 256-dimensional descriptors")
        n1, n2 = desc1.shape[1], desc2.shape[1]
        cap = max(n1, n2)
        if cap > L.MATCH_MAX_POINTS:
            raise ValueError("at most %d descriptors per side (got %d)" % (L.MATCH_MAX_POINTS, cap))
        f32 = dict(dtype=torch.float32, device=self.device)
        d1 = torch.zeros(1, cap, 256, **f32)
        d2 = torch.zeros(1, cap, 256, **f32)
        d1[0, :n1] = torch.from_numpy(np.ascontiguousarray(desc1.T, dtype=np.float32)).to(self.device)
        d2[0, :n2] = torch.from_numpy(np.ascontiguousarray(desc2.T, dtype=np.float32)).to(self.device)
        c1 = torch.tensor([n1], dtype=torch.int32, device=self.device)
        c2 = torch.tensor([n2], dtype=torch.int32, device=self.device)
        m, nm = L.op_match_two_way(d1, c1, d2, c2, nn_thresh)
        matches = _matches_to_numpy(m[0], int(nm.item()))
        self.mscores = matches
        return matches

    @property
    def all_pts(self):
        """The last max_length point sets, oldest first (numpy; a frame given to update_device is read back as [2,N])."""
        if any(p is None for p in self._host_pts):
            counts = self._table["state"][2:].cpu().numpy()
            first = self._frames % self.maxl  # ring slot of the oldest retained frame
            for c, p in enumerate(self._host_pts):
                if p is None:
                    self._host_pts[c] = self._pts[(first + c) % self.maxl, :int(counts[c])].cpu().numpy().T.copy()
        return self._host_pts

    @property
    def table(self):
        """The device track table (the dict of lib.track_table; None before the first frame).  Read it, e.g. with
        lib.op_track_select or as the input of lib.op_track_update with another `out`; the tracker owns its arrays."""
        return self._table

    @property
    def track_count(self):
        return int(self._table["state"][1].item()) if self._table is not None else 0

    @property
    def tracks(self):
        """The whole table as the reference keeps it: float64 [M, 2 + max_length] (track id, mean score, point ids)."""
        if self._table is None:
            return np.zeros((0, self.maxl + 2))
        return L.tracks_to_numpy(*L.op_track_select(self._table, 0))

    def get_offsets(self):
        """models/model_wrap.py:496-510: the id of point 0 of every retained frame."""
        return np.cumsum(np.array([0] + [p.shape[1] for p in self.all_pts[:-1]]))

    def _materialize(self):
        if self._pending is None:
            return
        (m, nm, had_prev), self._pending = self._pending, None
        matches = _matches_to_numpy(m, int(nm.item()))
        pts = self.all_pts
        if had_prev and pts[-2].shape[1] and pts[-1].shape[1]:
            self.mscores = matches   # (an empty side returns before the reference stores them)
        self.matches = matches
        if self._frames > 1:
            self.matches = np.concatenate((pts[-2][:2, matches[0].astype(int)], pts[-1][:2, matches[1].astype(int)]), axis=0)

    def get_matches(self):
        self._materialize()
        return self.matches

    def get_mscores(self):
        self._materialize()
        return self.mscores

    def clear_desc(self):
        self.last_desc = None
        self._prev_ok = False

    def update(self, pts, desc):
        """pts [3,N] points, desc [256,N] descriptors of the next frame (numpy).  After it, get_matches() is [4,K]
        (x0, y0, x1, y1) of the mutual matches with the previous frame and get_tracks() follows them over the last
        max_length frames (models/model_wrap.py:521-597)."""
        if pts is None or desc is None:
            print("PointTracker: Warning, no points were added to tracker.")
            return
        if self.class_consistent or self.world_classes is not None:
            raise ValueError("a class-consistent tracker and one with world_classes take their frames, with their classes, through "
                             "update_device")
        assert pts.shape[1] == desc.shape[1]
        n = pts.shape[1]
        if self.nn_thresh < 0.0 and n and self._prev_ok and self.all_pts[-1].shape[1]:
            raise ValueError("'nn_thresh' should be non-negative")
        if n and desc.shape[0] != 256:
            raise ValueError("the device matcher takes 256-dimensional descriptors")
        if n > L.MATCH_MAX_POINTS:
            raise ValueError("at most %d descriptors per side (got %d)" % (L.MATCH_MAX_POINTS, n))
        self._materialize()
        dev = self.device
        xy = torch.from_numpy(np.ascontiguousarray(pts[:2].T, dtype=np.float64)).to(dev)
        d = torch.from_numpy(np.ascontiguousarray(desc.T, dtype=np.float32)).to(dev).reshape(n, 256)
        self._host_pts = self.all_pts[1:] + [pts]
        self._pending = self._advance(xy, torch.tensor([n], dtype=torch.int32, device=dev), d)
        self._materialize()
        self.last_desc = desc.copy()
        self.last_pts = pts[:2, :].copy()

    def update_device(self, pts, count, desc, cls=None):
        """The same update from device tensors, e.g. one image's slice of Engine.describe_points: pts [cap, >= 2] rows
        starting (x, y), count int32 [1] (or 0-d), desc float32 [cap, 256] unit rows.  Matching and the track update are
        queued on the current stream; nothing is copied to the host and the host is not synchronised (the first call, and a
        call with a larger cap than any before, allocate).  A frame whose cap makes the buffers grow gives the results of a tracker
        that had that capacity from the start: the table, the kept landmarks of absolute_pose, the newest bundle adjustment and the
        loop edges are carried into the larger buffers, and no result depends on the capacity.  A cap above
        lib.MATCH_MAX_POINTS is cut to that many rows (and the count with it).  get_matches / get_mscores / all_pts read back on
        demand and describe the NEWEST frame: matches of earlier frames that were never asked for are dropped, so get_mscores()
        is the last non-empty match set among the frames it was asked about, not among all frames as after `update`.
        cls: uint8 [cap] classes of the rows (Engine.describe_points(classes=True)); required by a class-consistent tracker and
        by one with world_classes, ignored by a plain one."""
        if self.class_consistent or self.world_classes is not None:
            if cls is None:
                raise ValueError("a class-consistent tracker and one with world_classes need the classes of every frame (cls)")
            if not cls.is_cuda:
                raise RuntimeError("cls must live on a HIP device: the MI355X path has no CPU fallback")
            if cls.dtype != torch.uint8 or tuple(cls.shape) != (pts.shape[0],):
                raise ValueError("cls must be uint8 [cap] beside pts")
        else:
            cls = None
        for t, nm in ((pts, "pts"), (count, "count"), (desc, "desc")):
            if not t.is_cuda:
                raise RuntimeError("%s must live on a HIP device: the MI355X path has no CPU fallback" % nm)
        if pts.dim() != 2 or pts.shape[1] < 2 or desc.shape != (pts.shape[0], 256) or count.dtype != torch.int32:
            raise ValueError("pts [cap, >= 2], desc [cap, 256] and an int32 count are required")
        if self.nn_thresh < 0.0:
            raise ValueError("'nn_thresh' should be non-negative")
        self._pending = None  # the previous frame's matches were not asked for: they are dropped, not read back
        self._host_pts = self._host_pts[1:] + [None]
        self._pending = self._advance(pts[:, :2].to(torch.float64), count.reshape(1), desc, cls)
        self.last_desc = self.last_pts = None  # (host copies exist for frames given to update only)

    def get_tracks_device(self, min_length):
        """get_tracks on the device: (tracks float64 [row_cap, 2 + max_length], n_tracks int32 [1]); no synchronisation."""
        if min_length < 1:
            raise ValueError("'min_length' too small.")
        if self._table is None:
            raise RuntimeError("no frame yet")
        return L.op_track_select(self._table, int(min_length))

    def get_tracks(self, min_length):
        """models/model_wrap.py:599-615: float64 [M, 2 + max_length] rows (track id, mean score, point ids) of the tracks
        with at least min_length points and a point in the newest frame."""
        if min_length < 1:
            raise ValueError("'min_length' too small.")
        if self._table is None:
            return np.zeros((0, self.maxl + 2))
        return L.tracks_to_numpy(*L.op_track_select(self._table, int(min_length)))

    def track_points_device(self, tracks, n_tracks):
        """Device (tracks, n_tracks) as get_tracks_device returns them -> float64 [row_cap, max_length, 2] coordinates in
        the retained frames (NaN where a track has no point); no synchronisation."""
        return L.op_track_points(tracks, n_tracks, self._pts, self._table["state"], self._frames % self.maxl)

    def track_points(self, tracks):
        """The coordinates a tracks matrix (get_tracks) names: float64 [M, max_length, 2], NaN where the id is -1.  This is
        the read-out draw_tracks would connect with lines (models/model_wrap.py:617-648)."""
        tracks = np.ascontiguousarray(tracks, dtype=np.float64)
        if tracks.shape[0] == 0 or self._table is None:
            return np.zeros((tracks.shape[0], self.maxl, 2))
        t = torch.from_numpy(tracks).to(self.device)
        n = torch.tensor([tracks.shape[0]], dtype=torch.int32, device=self.device)
        return self.track_points_device(t, n).cpu().numpy()

    def draw_tracks(self, out, tracks):
        raise NotImplementedError("PointTracker draws nothing here: track_points(tracks) returns the [M, max_length, 2] "
                                  "coordinates of the tracks (NaN where a track has no point) for the caller's own drawing")


class SequenceTracker:
    """Point tracks over an image sequence on one GPU: per frame one eval forward, keypoints + sparse descriptors
    (ssp_describe_points), the two-way matcher against the previous frame and the track update, all on the device with no
    host copy of points, descriptors or matches.  `net` is one of this package's model drop-ins; the vocabulary is
    DescriptorExporter's.  Read the result with get_tracks / track_points (or `tracker`, the PointTracker).
    Semantic keypoints (the model needs a segmentation head): keep_classes / drop_classes (one of them)
    remove the keypoints of unwanted classes on the device before they enter the track table; class_consistent matches only
    points of equal class.  Neither adds a host copy or a synchronisation.
    geometric_check / check_thresh / min_inliers / check_seed: PointTracker's epipolar or homography check of every frame's
    matches, also without a host copy or a synchronisation.
    intrinsics / trajectory_rows: PointTracker's two-view pose and trajectory of a calibrated camera (DESIGN.md section 24;
    needs geometric_check="fundamental" or "auto"); read them with tracker.last_geometry() and trajectory().
    landmarks / landmarks_device / landmark_rows_device: PointTracker's, on demand.
    absolute_pose / absolute_thresh / absolute_min_inliers / landmark_params: PointTracker's absolute pose of every frame from the
    landmarks of the window before it, and with "repair" the repair of the trajectory; read it with
    tracker.last_geometry() and absolute_trajectory().  A step stays free of host copies and synchronisation.
    bundle_adjust / bundle_iterations / bundle_every: PointTracker's windowed bundle adjustment of the cameras and the landmarks,
    and with "apply" its write-back into the trajectory; read it with bundle_adjusted().  A step stays
    free of host copies and synchronisation.
    world_map / world_cap / world_patience / world_thresh / world_min_inliers: PointTracker's world map of landmarks that outlive
    their window, every frame's pose against it and, with "relocalise", the repair of the trajectory from it (DESIGN.md section
    29); read it with tracker.last_geometry(), world_trajectory(), world_map_device() and world_map().  A step stays free of host
    copies and synchronisation once allocated.
    world_classes / world_keep_classes / world_drop_classes: PointTracker's class votes on the map's landmarks and, with "match",
    its class-aware map matcher (needs world_map and a model with a segmentation head); read them with
    world_classes_device() and world_map(classes=True).  No host copy or synchronisation per step.
    loop_closure / loop_min_gap / loop_min_inliers / loop_cooldown / loop_iterations / loop_weight: PointTracker's loop closure
    over the world map (needs world_map); read it with tracker.last_geometry(), loop_closures() and
    loop_edges_device().
    world_upkeep / world_merge / world_merge_thresh / world_cull_age / world_cull_min_views / world_high_water / world_low_water:
    PointTracker's upkeep of the world map after every insert (needs world_map): revisits merged, weak rows
    culled, the least valuable rows evicted before the map is full; read it with tracker.last_geometry() and world_upkeep_report().
    ground_truth / gt_index / trajectory_eval / eval_align / eval_table: PointTracker's trajectory evaluation against ground-truth
    poses (needs intrinsics): evaluate_trajectory() on demand and, with "observe", a per-frame log on the
    device; read it with trajectory_eval_log() and tracker.last_geometry().
    Everything from geometric_check on is given by keyword (`**tracker_options`) and goes to PointTracker as it is: its names,
    defaults and checks are PointTracker's."""

    def __init__(self, net, device, conf_thresh, nms_dist, subpixel, nn_thresh, max_length, border_remove=4,
                 keep_classes=None, drop_classes=None, class_consistent=False, **tracker_options):
        if nn_thresh < 0.0:
            raise ValueError("'nn_thresh' should be non-negative")
        self.class_consistent = bool(class_consistent)
        self._mask = None
        self._with_cls = self.class_consistent or tracker_options.get("world_classes") is not None   # the tracker takes cls
        if keep_classes is not None or drop_classes is not None or self._with_cls:
            if not hasattr(net, "convSout"):
                raise ValueError("keep_classes / drop_classes / class_consistent / world_classes need a model with a segmentation head")
            if keep_classes is not None or drop_classes is not None:
                self._mask = L.class_mask(keep=keep_classes, drop=drop_classes, n_classes=net.n_classes)
        self.net, self.device = net, torch.device(device)
        self.conf_thresh, self.nms_dist, self.subpixel = conf_thresh, nms_dist, bool(subpixel)
        self.border_remove = border_remove
        self.tracker = PointTracker(max_length, nn_thresh, self.device, class_consistent=self.class_consistent, **tracker_options)

    def describe(self, image):
        """image [H,W] / [1,H,W] / [1,1,H,W] -> the device tensors of Engine.describe_points for this one image (with "cls",
        and already filtered, when the tracker was built with class arguments)."""
        x = _image_2d(image).to(self.device, torch.float32)[None, None].contiguous()
        eng = self.net.engine(1, x.shape[2], x.shape[3], self.device)
        with torch.no_grad():
            eng.forward(x, slot=0, train=False, want=())
        if self._mask is None and not self._with_cls:
            return eng.describe_points(0, 1, conf_thresh=self.conf_thresh, nms_dist=self.nms_dist, subpixel=self.subpixel,
                                       border_remove=self.border_remove)
        o = eng.describe_points(0, 1, conf_thresh=self.conf_thresh, nms_dist=self.nms_dist, subpixel=self.subpixel,
                                border_remove=self.border_remove, classes=True)
        return o if self._mask is None else L.op_filter_points(o["pts"], o["count"], o["desc"], o["cls"], self._mask)

    def step(self, image):
        """The next frame: forward -> points / descriptors (-> classes -> class filter) -> PointTracker.update_device.
        Returns describe()'s tensors."""
        o = self.describe(image)
        pts = o["pts"][0]
        xy = pts[:, :2].to(torch.float64)
        if self.subpixel:  # the same float64 sum as lib.points_to_numpy
            xy = xy + pts[:, 3:5].to(torch.float64) - 2
        self.tracker.update_device(xy, o["count"][0:1], o["desc"][0], o["cls"][0] if self._with_cls else None)
        return o

    def get_tracks(self, min_length):
        return self.tracker.get_tracks(min_length)

    def track_points(self, tracks):
        return self.tracker.track_points(tracks)

    def trajectory(self):
        return self.tracker.trajectory()

    def absolute_trajectory(self):
        return self.tracker.absolute_trajectory()

    def bundle_adjusted(self):
        return self.tracker.bundle_adjusted()

    def world_trajectory(self):
        return self.tracker.world_trajectory()

    def world_map_device(self):
        return self.tracker.world_map_device()

    def world_map(self, classes=False):
        return self.tracker.world_map(classes)

    def world_classes_device(self):
        return self.tracker.world_classes_device()

    def world_upkeep_report(self):
        return self.tracker.world_upkeep_report()

    def loop_edges_device(self):
        return self.tracker.loop_edges_device()

    def loop_closures(self):
        return self.tracker.loop_closures()

    def evaluate_trajectory(self, which=None, **options):
        return self.tracker.evaluate_trajectory(which, **options)

    def trajectory_eval_log(self):
        return self.tracker.trajectory_eval_log()

    def landmarks_device(self, min_views=2, min_parallax_deg=1.0, max_reproj=2.0):
        return self.tracker.landmarks_device(min_views, min_parallax_deg, max_reproj)

    def landmarks(self, min_views=2, min_parallax_deg=1.0, max_reproj=2.0):
        return self.tracker.landmarks(min_views, min_parallax_deg, max_reproj)

    def landmark_rows_device(self, min_views=2, min_parallax_deg=1.0, max_reproj=2.0):
        return self.tracker.landmark_rows_device(min_views, min_parallax_deg, max_reproj)


def _matches_to_numpy(m, n):
    """Device rows (i, j, score) -> the reference's float64 [3,L]."""
    a = m[:n].cpu().numpy().astype(np.float64)
    return a.T.copy() if n else np.zeros((3, 0))


def _image_2d(t):
    t = torch.as_tensor(t)
    while t.dim() > 2:
        assert t.shape[0] == 1, "one image per entry"
        t = t[0]
    return t
