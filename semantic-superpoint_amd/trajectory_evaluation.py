"""Trajectory evaluation on the device: a trajectory table against ground-truth poses -> the Sim(3) / SE(3)
alignment, ATE, the rotation error, RPE per frame distance and the KITTI devkit's segment errors, each with its statistics.

  read_kitti_poses / read_tum_trajectory / associate   the host steps, once per sequence: pose files and the frame-to-row map
  TrajectoryEvaluator                                  queues the operators of lib.op_traj_* and reads everything in one copy

A table row is (Rw [9], C [3], s, n_shared, flags, ratio) with Rw world-to-camera, as PointTracker.trajectory(),
absolute_trajectory() and world_trajectory() give it; a ground-truth row is the row-major 3x4 camera-to-world matrix (R | C), the
layout of a KITTI poses file.  There is no CPU fallback: the evaluator needs a HIP device."""
import numpy as np
import torch

from . import lib as L

STAT_NAMES = ("n", "rmse", "mean", "std", "min", "max", "median", "sse")


def read_kitti_poses(path):
    """A KITTI odometry poses file (a row-major 3x4 camera-to-world matrix per line) -> float64 [N, 12]"""
    rows = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if rows.shape[1] != L.TRAJ_GT_WORDS:
        raise ValueError("%s: a KITTI poses file has 12 numbers per line (got %d)" % (path, rows.shape[1]))
    return np.ascontiguousarray(rows)


def read_tum_trajectory(path):
    """A TUM trajectory file (lines `t tx ty tz qx qy qz qw`, `#` comments) -> (stamps float64 [N], poses float64 [N, 12]): the
    rotation of the unit quaternion (normalised here) and the translation, as camera-to-world rows."""
    rows = np.loadtxt(path, dtype=np.float64, comments="#", ndmin=2)
    if rows.shape[1] != 8:
        raise ValueError("%s: a TUM trajectory file has 8 numbers per line (got %d)" % (path, rows.shape[1]))
    q = rows[:, 4:8]
    norm = np.linalg.norm(q, axis=1, keepdims=True)
    if not (norm > 0).all():
        raise ValueError("%s: a zero quaternion" % path)
    x, y, z, w = (q / norm).T
    poses = np.empty((len(rows), 3, 4))
    poses[:, 0, 0], poses[:, 0, 1], poses[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    poses[:, 1, 0], poses[:, 1, 1], poses[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    poses[:, 2, 0], poses[:, 2, 1], poses[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    poses[:, :, 3] = rows[:, 1:4]
    return rows[:, 0].copy(), poses.reshape(-1, L.TRAJ_GT_WORDS)


def associate(stamps_est, stamps_gt, max_diff=0.02):
    """The ground-truth row of each estimated frame by time stamp -> int32 [len(stamps_est)], -1 for none.  All pairs within
    max_diff, sorted by difference, then by the estimate's index, then by the truth's, are taken greedily and one-to-one."""
    a, b = np.asarray(stamps_est, np.float64).ravel(), np.asarray(stamps_gt, np.float64).ravel()
    if not max_diff >= 0:
        raise ValueError("max_diff must be non-negative")
    index = np.full(len(a), -1, dtype=np.int32)
    if len(a) == 0 or len(b) == 0:
        return index
    order = np.argsort(b, kind="stable")
    lo, hi = np.searchsorted(b[order], a - max_diff, "left"), np.searchsorted(b[order], a + max_diff, "right")
    i = np.repeat(np.arange(len(a)), hi - lo)
    j = order[np.concatenate([np.arange(l, h) for l, h in zip(lo, hi)]).astype(np.int64)] if len(i) else np.zeros(0, np.int64)
    d = np.abs(a[i] - b[j])
    keep = d <= max_diff
    i, j, d = i[keep], j[keep], d[keep]
    used = np.zeros(len(b), dtype=bool)
    for k in np.lexsort((j, i, d)):
        if index[i[k]] < 0 and not used[j[k]]:
            index[i[k]] = j[k]
            used[j[k]] = True
    return index


class TrajectoryEvaluator(object):
    """gt: float64 [N, 12] (numpy or a tensor), the ground truth of one sequence; index: int32 [capacity] (numpy or a tensor), the
    ground-truth row of each frame (-1: none), or None when frame f is row f; capacity: the rows of the tables to come; align: "se3",
    "sim3", "origin" or "origin_scale"; skip_flags: frames whose flag word has one of these bits are left out; lengths / step: the
    KITTI segment lengths in metres (at most 8) and the distance between first frames; deltas: the frame distances of the RPE.

    evaluate(table, n_frames) queues the evaluation of one table [capacity, 16] and returns its device tensors; evaluate_many takes a
    stack [K, capacity, 16] against the one ground truth in the same launches.  result() copies the numbers of the last call to the
    host, once, and names them.  Nothing else synchronises with the host; the buffers of a batch size are allocated at its first
    use."""

    def __init__(self, gt, index=None, capacity=None, device="cuda", align="sim3", skip_flags=L.POSE_FLAG_NO_POSE,
                 lengths=L.KITTI_LENGTHS, step=10, deltas=(1,)):
        if align not in L.TRAJ_MODES:
            raise ValueError("align must be one of %s (got %r)" % (sorted(L.TRAJ_MODES), align))
        gt = torch.as_tensor(gt)
        if gt.dim() != 2 or gt.shape[1] != L.TRAJ_GT_WORDS or gt.shape[0] < 1:
            raise ValueError("gt must be [N >= 1, %d]: a row-major 3x4 camera-to-world matrix per row (got %s)" % (L.TRAJ_GT_WORDS,
                                                                                                           list(gt.shape)))
        if capacity is None:
            raise ValueError("capacity (the rows of the trajectory tables) is required")
        self.capacity, self.align, self.skip_flags, self.step = int(capacity), align, int(skip_flags), int(step)
        self.lengths = tuple(float(x) for x in lengths)
        self.deltas = tuple(int(d) for d in deltas)
        if not 1 <= len(self.lengths) <= L.TRAJ_MAX_LENGTHS or not all(np.isfinite(x) and x > 0 for x in self.lengths):
            raise ValueError("1 to %d finite positive lengths required (got %r)" % (L.TRAJ_MAX_LENGTHS, lengths))
        if not all(1 <= d <= self.capacity for d in self.deltas) or len(set(self.deltas)) != len(self.deltas):
            raise ValueError("deltas must be distinct and in 1..capacity (got %r)" % (deltas,))
        if self.step < 1 or not 1 <= self.capacity <= L.TRAJ_MAX_FRAMES:
            raise ValueError("step >= 1 and 1 <= capacity <= %d required" % L.TRAJ_MAX_FRAMES)
        if index is not None:
            index = torch.as_tensor(index)
            if index.dim() != 1 or index.shape[0] != self.capacity:
                raise ValueError("index must hold capacity = %d entries (got %s)" % (self.capacity, list(index.shape)))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TrajectoryEvaluator needs a HIP device: the MI355X path has no CPU fallback")
        self.gt = gt.to(self.device, torch.float64).contiguous()
        self.index = None if index is None else index.to(self.device, torch.int32).contiguous()
        self._sets = {}
        self._last = None

    def _set(self, P):
        """The buffers of a batch of P tables: the family of lib.traj_eval_buffers, whose err_t / err_r / valid hold the absolute
        errors, and a view of it per delta with per-frame arrays of its own.  Stats slots: ATE, rotation, then two per delta."""
        s = self._sets.get(P)
        if s is None:
            traj = L.traj_eval_buffers(self.capacity, P, len(self.lengths), self.step, self.device, n_stat=2 + 2 * len(self.deltas))
            traj["lengths"].copy_(torch.tensor(self.lengths, dtype=torch.float64))
            rpe = [dict(traj, **L._alloc(L.TRAJ_SPEC, L._traj_dims(traj), self.device, L.TRAJ_PAIR_KEYS)) for _ in self.deltas]
            n_frames = torch.zeros(P, dtype=torch.int32, device=self.device)
            packed = torch.zeros(P, L.TRAJ_SIM_WORDS + traj["stats"].shape[0] * L.TRAJ_STATS_WORDS + traj["summary"].shape[1]
                                 + L.TRAJ_INFO_WORDS, dtype=torch.float64, device=self.device)
            s = self._sets[P] = dict(traj=traj, rpe=rpe, n_frames=n_frames, packed=packed)
        return s

    def evaluate_many(self, tables, n_frames):
        """tables float64 [K, capacity, 16] on the device; n_frames: an int, an int32 device tensor of K entries, or K ints (a list
        is copied from the host, which may wait for the device; an int or a device tensor does not) ->
        dict of device tensors: sim [K, 16]; err_t / err_r / valid [K, capacity], the absolute errors per frame; rpe {delta: (err_t,
        err_r, valid)}; dist, seg, summary, info of the segments; stats [2 + 2 len(deltas), K, 8]: ATE, rotation, then translation and
        rotation per delta.  The tensors belong to the evaluator and are rewritten by its next call."""
        L._need_gpu(tables, "tables")
        if tables.dim() != 3:
            raise ValueError("tables must be float64 [K, %d, %d] (got %s)" % (self.capacity, L.POSE_ROW_WORDS, list(tables.shape)))
        P = int(tables.shape[0])
        s = self._set(P)
        traj, nf = s["traj"], s["n_frames"]
        if torch.is_tensor(n_frames):
            nf = L._count(n_frames, "n_frames", P, hint="one per table")
        elif np.ndim(n_frames) == 0:
            nf.fill_(int(n_frames))
        else:
            if len(n_frames) != P:
                raise ValueError("n_frames must hold one count per table (%d, got %d)" % (P, len(n_frames)))
            nf.copy_(torch.tensor([int(n) for n in n_frames], dtype=torch.int32))
        kw = dict(index=self.index, skip_flags=self.skip_flags)
        L.op_traj_align(tables, nf, self.gt, traj, mode=self.align, **kw)
        L.op_traj_ape(tables, nf, self.gt, traj, **kw)
        L.op_traj_stats(traj["err_t"], traj["valid"], traj["stats"][0])
        L.op_traj_stats(traj["err_r"], traj["valid"], traj["stats"][1])
        for k, (d, r) in enumerate(zip(self.deltas, s["rpe"])):
            L.op_traj_rpe_delta(tables, nf, self.gt, r, delta=d, scale=traj["sim"], **kw)
            L.op_traj_stats(r["err_t"], r["valid"], traj["stats"][2 + 2 * k])
            L.op_traj_stats(r["err_r"], r["valid"], traj["stats"][3 + 2 * k])
        L.op_traj_rpe_segments(tables, nf, self.gt, traj, scale=traj["sim"], **kw)
        self._last = (P, tables.dim())
        out = {k: traj[k] for k in ("sim", "err_t", "err_r", "valid", "dist", "seg", "summary", "info", "stats")}
        out["rpe"] = {d: (r["err_t"], r["err_r"], r["valid"]) for d, r in zip(self.deltas, s["rpe"])}
        return out

    def evaluate(self, table, n_frames):
        """One table float64 [capacity, 16]: evaluate_many of a stack of one"""
        L._need_gpu(table, "table")
        if table.dim() != 2:
            raise ValueError("table must be float64 [%d, %d] (got %s)" % (self.capacity, L.POSE_ROW_WORDS, list(table.shape)))
        out = self.evaluate_many(table[None], n_frames)
        self._last = (1, 2)
        return out

    def result(self):
        """The numbers of the last evaluate (a dict) or evaluate_many (a list of dicts), in one copy to the host: ate_* and ape_rot_*
        (rmse, mean, median, std, min, max; metres and degrees), rpe_trans_* / rpe_rot_* of the first delta and "rpe" {delta: {...}} of
        all, kitti_t_rel_percent, kitti_r_rel_deg_per_100m, kitti_segments, kitti_lengths [(L, segments, percent, deg per 100 m)],
        kitti_info, scale, rotation, translation, n_valid, status."""
        if self._last is None:
            raise RuntimeError("result() needs an evaluate() or evaluate_many() before it")
        P, dim = self._last
        s = self._sets[P]
        traj = s["traj"]
        n_stat, n_sum = traj["stats"].shape[0], traj["summary"].shape[1]
        torch.cat([traj["sim"], traj["stats"].permute(1, 0, 2).reshape(P, -1), traj["summary"], traj["info"].to(torch.float64)], dim=1,
                  out=s["packed"])
        host = s["packed"].cpu().numpy()
        out = []
        for row in host:
            sim, rest = row[:L.TRAJ_SIM_WORDS], row[L.TRAJ_SIM_WORDS:]
            stats = rest[:n_stat * L.TRAJ_STATS_WORDS].reshape(n_stat, L.TRAJ_STATS_WORDS)
            summary, info = rest[n_stat * L.TRAJ_STATS_WORDS:][:n_sum], rest[n_stat * L.TRAJ_STATS_WORDS + n_sum:]
            named = lambda prefix, st: {"%s_%s" % (prefix, n): float(v) for n, v in zip(STAT_NAMES[1:7], st[1:7])}
            r = dict(scale=float(sim[0]), rotation=sim[1:10].reshape(3, 3).copy(), translation=sim[10:13].copy(), n_valid=int(sim[13]),
                     status=int(sim[14]), align=self.align)
            r.update(named("ate", stats[0]))
            r.update(named("ape_rot", stats[1]))
            r["rpe"] = {}
            for k, d in enumerate(self.deltas):
                e = dict(n=int(stats[2 + 2 * k][0]))
                e.update(named("trans", stats[2 + 2 * k]))
                e.update(named("rot", stats[3 + 2 * k]))
                r["rpe"][d] = e
                if k == 0:
                    r.update(named("rpe_trans", stats[2]))
                    r.update(named("rpe_rot", stats[3]))
            deg = 180.0 / np.pi
            r["kitti_t_rel_percent"] = 100.0 * float(summary[0])
            r["kitti_r_rel_deg_per_100m"] = 100.0 * deg * float(summary[1])
            r["kitti_lengths"] = [(Lm, int(summary[2 + 3 * k]), 100.0 * float(summary[3 + 3 * k]), 100.0 * deg * float(summary[4 + 3 * k]))
                                  for k, Lm in enumerate(self.lengths)]
            r["kitti_segments"] = int(info[0])
            r["kitti_info"] = tuple(int(v) for v in info)
            out.append(r)
        return out[0] if dim == 2 else out
