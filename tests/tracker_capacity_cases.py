"""Padding for tests/test_gpu_tracker_capacity.py: a PointTracker sizes its buffers by the row count of the
tensors update_device is given, so three trackers fed the same frames at different row counts have different capacities, and one
whose row count rises grows.  Padding rows are copies of the frame's first row (point, descriptor, class), never zeros: a kernel that
read them would count them."""
import torch

FIRST_CAP = 1024            # PointTracker._ensure: cap = min(MATCH_MAX_POINTS, max(n, 2 * cap, 1024))
TIGHT_EXTRA, WIDE_ROWS = 64, 2048
GROW_ROWS = (1025, 2049)    # the row counts that take the capacity 1024 -> 2048 -> 4096


def pad_rows(t, rows):
    """t [n >= 1, ...] -> [rows >= n, ...]: the rows past n are copies of row 0."""
    n = t.shape[0]
    assert 1 <= n <= rows
    out = t[:1].repeat(rows, *([1] * (t.dim() - 1)))
    out[:n] = t
    return out.contiguous()


def padded(frame, rows):
    """frame: (pts, count, desc) or (pts, count, desc, cls) of update_device -> the same frame in tensors of `rows` rows."""
    pts, count, desc = frame[:3]
    out = (pad_rows(pts, rows), count, pad_rows(desc, rows))
    return out + ((pad_rows(frame[3], rows),) if len(frame) > 3 and frame[3] is not None else ())


def plans(counts, g, g2=None):
    """Rows per frame of the three trackers: {"tight", "wide", "growing"}; growing = tight except frame g (GROW_ROWS[0]) and, where
    there is one, frame g2 (default g + 1; GROW_ROWS[1]).  And the capacity each tracker has after every frame."""
    frames = len(counts)
    assert max(counts) + TIGHT_EXTRA <= FIRST_CAP and 1 <= g < frames
    g2 = g + 1 if g2 is None else g2
    tight = [n + TIGHT_EXTRA for n in counts]
    growing = list(tight)
    growing[g] = GROW_ROWS[0]
    if g2 < frames:
        assert g2 > g
        growing[g2] = GROW_ROWS[1]
    rows = {"tight": tight, "wide": [WIDE_ROWS] * frames, "growing": growing}
    caps = {}
    for name, per_frame in rows.items():
        cap, caps[name] = 0, []
        for r in per_frame:
            if r > cap:
                cap = max(r, 2 * cap, FIRST_CAP)
            caps[name].append(cap)
    return rows, caps


def slice_to_common(a, b, cap_a, cap_b):
    """Two entries of last_geometry() from trackers of capacities cap_a and cap_b: (a over the common rows, b over the common rows,
    what the wider one holds behind them), or None when their shapes differ in a dimension that is no capacity."""
    if a.dim() != b.dim():
        return None
    rest = []
    for d, (sa, sb) in enumerate(zip(a.shape, b.shape)):
        if sa == sb:
            continue
        if sa * cap_b != sb * cap_a:          # (cap rows, or max_length * cap rows)
            return None
        m = min(sa, sb)
        wide = a if sa > sb else b
        rest.append(wide.narrow(d, m, max(sa, sb) - m))
        a, b = a.narrow(d, 0, m), b.narrow(d, 0, m)
    return a, b, rest


def same_bytes(a, b):
    a, b = a.contiguous().cpu().numpy(), b.contiguous().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def all_zero(t):
    return not bool(torch.count_nonzero(t.contiguous().view(torch.uint8) if t.dtype != torch.bool else t))


def chain_step_block_order(prev, cur, match_prev, match_cur, n_match_prev, n_match_cur, state, cap_prev, cap_cur):
    """pose_ref.chain_step with the two sums of the shared depths taken as pose_chain_kernel takes them (csrc/pose_kernels.hip.h:
    "sa = sa + zprev[i]" per thread over its rows k = tid, tid + 256, ..., then block_sum<256>), not in ascending order: the only
    place where the kernel's order of addition differs from pose_ref's.  Everything else is chain_step's, in float64."""
    import numpy as np

    from tests import epipolar_ref as E
    from tests import pose_ref as P
    rows_k, shared_prev, shared_cur = [], [], []
    if prev is not None:
        _, jA = P._indices(match_prev, n_match_prev, cap_prev)
        zprev = {}
        for k in range(jA.shape[0]):
            if prev["front"][k] and int(jA[k]) not in zprev:       # the lowest row wins
                zprev[int(jA[k])] = prev["depth"][k, 1]
        iB, _ = P._indices(match_cur, n_match_cur, cap_cur)
        for k in range(iB.shape[0]):
            if cur["front"][k] and int(iB[k]) in zprev:
                rows_k.append(k)
                shared_prev.append(zprev[int(iB[k])])
                shared_cur.append(cur["depth"][k, 0])
    n_shared = len(rows_k)
    sa = float(E.block_sum(np.array(shared_prev), np.array(rows_k), 256)) if n_shared else 0.0
    sb = float(E.block_sum(np.array(shared_cur), np.array(rows_k), 256)) if n_shared else 0.0
    with np.errstate(all="ignore"):
        ratio = np.float64(sa) / np.float64(sb) if n_shared > 0 else np.float64(0.0)
    ok = (prev is not None and prev["status"] == 0 and cur["status"] == 0 and n_shared >= P.MIN_FRONT and P._usable(ratio))
    s = state["s"] * ratio if ok else state["s"]
    posed = cur["status"] == 0
    R = np.asarray(cur["R"], dtype=np.float64) if posed else np.eye(3)
    t = np.asarray(cur["t"], dtype=np.float64) if posed else np.zeros(3)
    Rw0, tw0 = state["Rw"], state["tw"]
    Rw, tw = np.zeros((3, 3)), np.zeros(3)
    for r in range(3):
        for c in range(3):
            Rw[r, c] = P._dot(R[r], Rw0[:, c])
        tw[r] = P._dot(R[r], tw0) + s * t[r]
    C = np.array([-P._dot(Rw[:, c], tw) for c in range(3)])
    flags = (0 if posed else P.FLAG_NO_POSE) | (0 if ok else P.FLAG_SCALE_CARRIED)
    row = np.concatenate([Rw.reshape(9), C, [s, float(n_shared), float(flags), ratio]])
    return row, {"n_frames": state["n_frames"] + 1, "s": s, "Rw": Rw, "tw": tw}
