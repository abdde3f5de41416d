"""The fixtures of the trajectory evaluation, shared by tests/test_traj_eval_cpu.py and
tests/test_gpu_traj_eval.py: ground truths, planted similarity transforms, invalid rows, hand-made error arrays and the analytic
KITTI cases, all small by construction, and the measured float64 / longdouble difference of the restatement on each of them.
    python -m tests.traj_eval_cases        prints WAY_DIFFERENCE as it is recorded below"""
import functools

import numpy as np

from tests import traj_eval_ref as R

MARGIN_MIN = 1e-9          # no fixture rests on a decision closer than this, relative (segment ends, collinearity)
FRAME_COUNTS = (0, 1, 2, 3, 4, 63, 64, 65, 257, 1025, 4097)   # around the wave, the workgroup and the rows-per-thread boundaries
LENGTHS = (20.0, 50.0, 100.0, 200.0)   # of the 300 m circuits


def rot(axis, angle):
    """Rodrigues"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def truth(n, kind="circuit", length=300.0):
    """gt [n, 12]: a camera on a closed 3-D circuit of about `length` metres ("planar": in the plane y = 0; "line": along z),
    heading along the path with a small pitch"""
    u = np.arange(n) / max(n, 1)
    r = length / (2 * np.pi)
    if kind == "line":
        c = np.stack([np.zeros(n), np.zeros(n), length * u], axis=1)
    else:
        c = np.stack([r * np.cos(2 * np.pi * u), (0.0 if kind == "planar" else 2.0) * np.sin(4 * np.pi * u), r * np.sin(2 * np.pi * u)], axis=1)
    gt = np.zeros((n, 3, 4))
    for k in range(n):
        gt[k, :, :3] = rot((0, 1, 0), -2 * np.pi * u[k]) @ rot((1, 0, 0), 0.05 * np.sin(6 * np.pi * u[k]))
        gt[k, :, 3] = c[k]
    return gt.reshape(n, 12)


def estimate(gt, s=1.0, Rot=None, t=(0.0, 0.0, 0.0), noise=0.0, noise_rot=0.0, seed=0, capacity=None, mirror=False):
    """table [capacity, 16] whose centres p satisfy q = s Rot p + t (+ noise) and whose rotations are Rot^T R_gt (+ noise_rot radians)"""
    rng = np.random.default_rng(seed)
    n = len(gt)
    Rot = np.eye(3) if Rot is None else Rot
    G = gt.reshape(n, 3, 4)
    table = np.zeros((capacity or max(n, 1), R.ROW_WORDS))
    for k in range(n):
        p = Rot.T @ (G[k, :, 3] - np.asarray(t)) / s + noise * rng.standard_normal(3)
        if mirror:
            p = p * np.array([1.0, 1.0, -1.0])
        c2w = Rot.T @ G[k, :, :3] @ rot(rng.standard_normal(3) + 1e-3, noise_rot * rng.standard_normal())
        table[k, :9], table[k, 9:12], table[k, 12] = c2w.T.ravel(), p, 1.0
    return table


def sequence_truth(seq):
    """gt [frames, 12] of a sequence of pose_ref / world_ref / loop_ref: (Rw^T | C) per frame.  Where the sequence keeps no "Rw", the
    world-to-camera rotations are chained from its pairs' R (camera 0 is the world)."""
    frames = len(seq["centres"])
    if "Rw" in seq:
        Rw = np.asarray(seq["Rw"], np.float64)
    else:
        Rw = [np.eye(3)]
        for pr in seq["pairs"]:
            Rw.append(pr["R"] @ Rw[-1])
        Rw = np.stack(Rw)
    gt = np.zeros((frames, 3, 4))
    gt[:, :, :3], gt[:, :, 3] = np.swapaxes(Rw, 1, 2), seq["centres"]
    return gt.reshape(frames, 12)


def observe_log(table, frames, gt, mode="sim3", index=None):
    """The restated per-frame log of PointTracker(trajectory_eval="observe"): row f = (ATE rmse, mean, max, s, n_valid, status, 0, 0)
    of rows 0..f of the table as it stands (a table that is rewritten in later frames gives the log of its final state)."""
    log = np.zeros((frames, 8))
    for f in range(frames):
        log[f] = observe_row(table, f + 1, gt, mode, index)
    return log


def observe_row(table, n, gt, mode="sim3", index=None):
    sim = R.align(table, n, gt, index, mode)
    et, _, v = R.ape(table, n, gt, sim, index)
    st = R.stats(et, v)
    return np.array([st[1], st[2], st[5], sim[0], sim[13], sim[14], 0.0, 0.0])


ROT_A = rot((1.0, 2.0, -0.5), 0.7)
ROT_180 = rot((0.3, -1.0, 0.2), np.pi - 1e-3)


def _case(table, n_frames, gt, index=None, mode="sim3", lengths=LENGTHS, step=10, deltas=(1,), status=R.OK):
    return dict(table=table, n_frames=n_frames, gt=gt, index=index, mode=mode, lengths=tuple(lengths), step=step, deltas=tuple(deltas),
                status=status)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: dict(table [capacity, 16], n_frames, gt [n_gt, 12], index or None, mode, lengths, step, deltas, status)}"""
    out = {}
    for n in FRAME_COUNTS:   # a planted Sim(3) with noise at every frame count; a ground truth is never empty
        gt = truth(max(n, 1))
        out["n%d" % n] = _case(estimate(gt[:n], 0.037, ROT_A, (5.0, -3.0, 2.0), 0.02, 0.01, seed=n), n, gt,
                               status=R.FEW if n < 3 else R.OK, deltas=(1, 7) if n == 65 else (1,))
    gt = truth(257)
    for name, s, Rt in (("s0037", 0.037, ROT_A), ("s41", 41.0, ROT_A), ("rot180", 1.7, ROT_180)):
        out[name] = _case(estimate(gt, s, Rt, (1.0, 2.0, 3.0)), 257, gt)
        out[name + "_noise"] = _case(estimate(gt, s, Rt, (1.0, 2.0, 3.0), 0.05 / s, 0.02, seed=7), 257, gt)
    out["mirror"] = _case(estimate(gt[:65], 1.0, ROT_A, noise=0.01, seed=3, mirror=True), 65, gt[:65])   # det H < 0
    for k in (4, 5):
        out["mirror%d" % k] = _case(estimate(gt[:64 * k:64], 1.0, ROT_A, noise=0.01, seed=k, mirror=True), k, gt[:64 * k:64].copy())
    gp = truth(257, "planar")
    out["planar"] = _case(estimate(gp, 2.5, rot((0, 1, 0), 1.1), (4.0, 0.0, -2.0)), 257, gp)
    gl = truth(65, "line")
    # centres on a line along z on both sides, scaled and shifted but not turned: every product off H[2][2] is an exact zero, so the
    # collinearity test is decided with the whole margin (a line in general position leaves the second eigenvalue at rounding level)
    out["collinear"] = _case(estimate(gl, 2.0, None, (1.0, 1.0, 1.0)), 65, gl, status=R.COLLINEAR)
    for mode in ("se3", "origin", "origin_scale"):
        out["mode_" + mode] = _case(estimate(gt, 1.0 if mode != "origin_scale" else 0.2, ROT_A, (1.0, 2.0, 3.0), 0.03, 0.01, seed=11), 257, gt,
                                    mode=mode)
    # invalid rows interleaved: flags, NaN in the table and in the truth, a -1 index, other flag bits that do not skip
    table = estimate(gt, 0.5, ROT_A, (0.0, 1.0, 0.0), 0.02, 0.01, seed=5)
    g2 = gt.copy()
    index = np.arange(257, dtype=np.int32)
    table[::9, 14] = 1.0
    table[1::9, 14] = 2.0 + 4.0 + 8.0 + 32.0
    table[5::31, 10] = np.nan
    table[6::37, 3] = np.inf
    table[100, 14] = np.nan
    table[101, 14] = 0.5   # (no integer)
    g2[7::41, 5] = np.nan
    index[3::23] = -1
    index[250] = 400
    out["invalid"] = _case(table, 257, g2, index)
    perm = np.random.default_rng(1).permutation(257)   # the truth stored in another order, the index map undoing it
    inv = np.empty(257, dtype=np.int32)
    inv[perm] = np.arange(257, dtype=np.int32)
    out["permuted"] = _case(estimate(gt, 3.0, ROT_A, noise=0.01, seed=2), 257, gt[perm], inv)
    out["overlong"] = _case(estimate(gt, 3.0, ROT_A, noise=0.01, seed=2, capacity=257)[:200].copy(), 257, gt)   # n_frames > capacity
    # the analytic KITTI cases (a straight line: the alignment is status 2, the identity, and the segments take the scale 1):
    # 1 m steps along z, the estimate 1.1 times the truth / a constant yaw drift; a short sequence; an
    # invalid end
    line = np.zeros((1000, 3, 4))
    line[:, :, :3] = np.eye(3)
    line[:, 2, 3] = np.arange(1000.0)
    line = line.reshape(1000, 12)
    scaled = estimate(line)
    scaled[:, 9:12] *= 1.1
    out["kitti_scale"] = _case(scaled, 1000, line, mode="se3", lengths=R.KITTI_LENGTHS, status=R.COLLINEAR)
    yaw = estimate(line)
    for k in range(1000):
        yaw[k, :9] = rot((0, 1, 0), YAW_DRIFT * k).T.ravel()
    out["kitti_yaw"] = _case(yaw, 1000, line, mode="origin", lengths=R.KITTI_LENGTHS)
    out["kitti_short"] = _case(scaled[:90].copy(), 90, line[:90].copy(), mode="se3", lengths=R.KITTI_LENGTHS, status=R.COLLINEAR)
    bad = scaled.copy()
    bad[101, 14] = 1.0   # the end of the 100 m segment from frame 0
    out["kitti_bad_end"] = _case(bad, 1000, line, mode="se3", lengths=R.KITTI_LENGTHS, status=R.COLLINEAR)
    return out


YAW_DRIFT = 1e-3   # radians per frame of kitti_yaw


@functools.lru_cache(maxsize=None)
def stats_cases():
    """{name: (err [capacity], valid int32 [capacity])}: hand-made error arrays"""
    rng = np.random.default_rng(4)
    out = {}
    for n in (0, 1, 2, 3):
        out["n%d" % n] = (np.array([3.0, 1.0, 2.0, 9.0])[:max(n, 1)], np.array([1, 1, 1, 1], np.int32)[:max(n, 1)] * (n > 0))
    out["equal"] = (np.full(100, 0.125), np.ones(100, np.int32))
    base = np.float64(1.5).view(np.uint64)
    out["mantissa_byte"] = ((base + (rng.permutation(200).astype(np.uint64) << np.uint64(16))).view(np.float64), np.ones(200, np.int32))
    out["exponent"] = (np.ldexp(1.0, rng.permutation(np.arange(-60, 61))), np.ones(121, np.int32))
    ties = np.concatenate([np.full(100, 0.5), np.full(57, 0.75), np.full(100, 2.0)])
    out["ties257"] = (rng.permutation(ties), np.ones(257, np.int32))
    ties2 = np.concatenate([np.full(128, 0.5), np.full(128, 0.75)])
    out["ties256"] = (rng.permutation(ties2), np.ones(256, np.int32))
    x = np.abs(rng.standard_normal(1025))
    v = (rng.random(1025) < 0.7).astype(np.int32)
    x[v == 0] = np.nan   # what an invalid entry holds is never read into a result
    out["masked1025"] = (x, v)
    out["zeros"] = (np.zeros(65), np.ones(65, np.int32))
    return out


# ---- the float64 / longdouble difference of the restatement, per fixture and output ----
OUTPUTS = ("scale", "rotation", "translation", "sigma", "err_t", "err_r", "ate", "ate_sse", "ape_rot", "ape_rot_sse", "rpe_t", "rpe_r",
           "rpe_t_stats", "rpe_t_sse", "rpe_r_stats", "rpe_r_sse", "dist", "seg_t", "seg_r", "summary_t", "summary_r")


def flatten(ev):
    """{output: flat array} of a traj_eval_ref.evaluate result (the integers left out).  Numbers of one kind and size share an
    output, so that a bound is never set by a larger neighbour: the statistics of a kind (rmse, mean, std, min, max, median) apart
    from its sum of squares, the translation errors of the segments apart from the rotation errors."""
    d = sorted(ev["rpe"])
    sim, seg, summary = ev["sim"], ev["seg"], ev["summary"]
    return {"scale": sim[0:1], "rotation": sim[1:10], "translation": sim[10:13], "sigma": sim[15:], "err_t": ev["ape"][0],
            "err_r": ev["ape"][1], "ate": ev["ate"][1:7], "ate_sse": ev["ate"][7:], "ape_rot": ev["ape_rot"][1:7],
            "ape_rot_sse": ev["ape_rot"][7:],
            "rpe_t": np.concatenate([ev["rpe"][k][0] for k in d]), "rpe_r": np.concatenate([ev["rpe"][k][1] for k in d]),
            "rpe_t_stats": np.concatenate([ev["rpe"][k][3][1:7] for k in d]), "rpe_t_sse": np.concatenate([ev["rpe"][k][3][7:] for k in d]),
            "rpe_r_stats": np.concatenate([ev["rpe"][k][4][1:7] for k in d]), "rpe_r_sse": np.concatenate([ev["rpe"][k][4][7:] for k in d]),
            "dist": ev["dist"], "seg_t": seg[:, :, 1].ravel(), "seg_r": seg[:, :, 2].ravel(),
            "summary_t": np.concatenate([summary[0:1], summary[3::3]]), "summary_r": np.concatenate([summary[1:2], summary[4::3]])}


@functools.lru_cache(maxsize=None)
def reference(name, wide=False):
    """traj_eval_ref.evaluate of a fixture, computed once and shared"""
    c = cases()[name]
    return R.evaluate(c["table"], c["n_frames"], c["gt"], c["index"], c["mode"], R.FLAG_NO_POSE, c["lengths"], c["step"], c["deltas"],
                      way=R.WAY2 if wide else R.WAY1)


def way_difference(name):
    """{output: the largest |float64 - longdouble| of the restatement on the fixture}"""
    a, b = flatten(reference(name)), flatten(reference(name, True))
    return {k: float(np.abs(a[k].astype(np.longdouble) - b[k]).max()) if a[k].size else 0.0 for k in OUTPUTS}


def stats_way_difference(name):
    """(the statistics rmse .. median, the sum of squares): the largest |float64 - longdouble| of each"""
    e, v = stats_cases()[name]
    d = np.abs(R.stats(e, v).astype(np.longdouble) - R.stats(e, v, R.WAY2))
    return float(d[1:7].max()), float(d[7])


def bound(name, output):
    """16 times the recorded difference: the tolerance of a floating output of a fixture"""
    return 16.0 * WAY_DIFFERENCE[name][OUTPUTS.index(output)]


# Recorded from `python -m tests.traj_eval_cases` (numpy.longdouble is the 80-bit format here); tests/test_traj_eval_cpu.py
# repeats the measurement.  Per fixture, in the order of OUTPUTS.
WAY_DIFFERENCE = {
    'n0': (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    'n1': (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    'n2': (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.225508831723346e-13, 7.660430449696332e-16, 4.225508831723346e-13, 1.940861693583429e-09, 7.660430449696332e-16, 5.506391783510756e-16, 0.0, 2.3966939544095567e-14, 6.483507815639635e-19, 2.3966939544095567e-14, 6.483507815639635e-19),
    'n3': (5.421010862427522e-19, 1.6376873815393544e-16, 8.667112166849122e-16, 6.673417374258861e-11, 2.4189929278971056e-15, 4.807786113669721e-15, 2.4189929278971056e-15, 1.4783004070669066e-18, 4.807786113669721e-15, 9.306899868832819e-15, 2.7111559525172524e-15, 2.554082162778415e-15, 2.7111559525172524e-15, 6.048113398993138e-15, 2.554082162778415e-15, 4.179490954714371e-15, 7.577272143066693e-15, 1.3278088481158412e-16, 7.619061360552432e-19, 1.3278088481158412e-16, 7.619061360552432e-19),
    'n4': (1.112662479513249e-17, 2.397713104451693e-16, 1.9741153156616065e-15, 1.9326762412674725e-12, 1.2786199243331099e-14, 5.2069893535788836e-15, 1.2786199243331099e-14, 1.868698631749086e-17, 3.641292996292567e-15, 1.0765802312129313e-14, 6.2765276916815216e-15, 6.762507762970993e-16, 6.2765276916815216e-15, 5.104965929147998e-15, 6.762507762970993e-16, 4.1991150140363587e-16, 2.2412627309620348e-14, 2.2582321890273274e-17, 5.886878983417387e-19, 2.2582321890273274e-17, 5.886878983417387e-19),
    'n63': (9.063252535621014e-18, 3.6374982886888674e-16, 2.076464000744238e-15, 1.4995293895481154e-10, 2.7802141357783337e-14, 9.930804008989602e-15, 1.2608648273273711e-14, 1.5375593521466276e-17, 6.536058586720239e-15, 3.585326480148865e-14, 1.602364519452074e-15, 3.2371024263899706e-15, 1.602364519452074e-15, 2.2724877535296173e-16, 1.6361152883892505e-15, 4.440892098500626e-15, 7.291389714225716e-14, 9.145372379857318e-17, 2.470371590667167e-18, 1.8342074956318247e-17, 1.0583676675942483e-18),
    'n64': (6.030874584450618e-19, 2.3922920935892655e-16, 1.3363875978056328e-15, 1.3596945791505277e-10, 1.2820421756680337e-14, 1.1322567232754932e-14, 8.275302254020069e-15, 1.0667037952842107e-16, 5.193111565771069e-15, 9.498651865058605e-14, 7.492290174501617e-16, 3.424723612338587e-15, 6.732170219173896e-16, 4.0101927854807595e-17, 1.9325903724554117e-15, 1.2443171493181637e-14, 8.31279489688086e-14, 7.524871296817753e-17, 4.512462147378878e-18, 2.820069142941105e-17, 2.1535812683940586e-19),
    'n65': (6.583140066060422e-18, 1.9217483507305566e-16, 2.1600559882428705e-15, 2.7000623958883807e-10, 1.4031761562845462e-14, 1.5708544491219167e-14, 8.932862824819528e-15, 9.701297970241547e-17, 1.2472745648535021e-14, 1.4129149239483496e-13, 4.4155488727187775e-15, 4.3241370770510934e-15, 2.6076146450448867e-15, 1.0771765424077984e-14, 4.07176191635078e-15, 2.7630675525358583e-14, 1.85268467234323e-13, 1.2709051747192973e-16, 1.5570053757310142e-18, 3.59667130063121e-17, 2.599067659090617e-19),
    'n257': (5.400682071693419e-18, 1.7119552303546115e-16, 2.5191437477700696e-15, 8.93578544491902e-11, 1.4643735349819287e-14, 1.0351528662022602e-14, 7.59130663196975e-15, 1.030409492285548e-16, 6.508221695941674e-15, 1.2961853812498703e-13, 4.242161228415822e-16, 3.0161420236374248e-15, 2.601746400786309e-17, 2.558039500707987e-17, 6.049373784018652e-16, 3.660960423701454e-14, 1.4718781748968013e-13, 1.349191136078092e-16, 3.174983888774537e-18, 1.553585480206475e-17, 1.5140713932170619e-19),
    'n1025': (6.105413483808997e-18, 2.3071822230491534e-16, 8.179221189230645e-16, 1.921307557495311e-10, 1.787305163759986e-14, 8.812069997310434e-15, 3.840014125498477e-15, 1.2701555505609773e-16, 6.7975139406151186e-15, 9.325873406851315e-15, 1.5001197017845995e-16, 3.900444420570914e-15, 1.683512393381404e-17, 8.216219588366713e-18, 1.0197328008040851e-15, 1.4432899320127035e-15, 9.336975637097567e-14, 1.6398325255655005e-16, 5.921819092491627e-18, 1.230061246002695e-17, 2.4961002164400163e-19),
    'n4097': (3.1712913545201005e-18, 2.854704320154333e-16, 2.224349177071261e-15, 1.956550477189012e-10, 2.13796618424769e-14, 1.5512439423270852e-14, 1.4016856641709983e-14, 9.838935662563348e-16, 3.619311377926213e-15, 2.6201263381153694e-13, 3.270584791761986e-17, 3.805386995098248e-15, 2.0383847875674738e-18, 4.186036825330752e-18, 1.1158608759220812e-15, 9.614531393253856e-14, 2.415012634315872e-13, 2.1272808953818126e-16, 5.005805899595305e-18, 3.888728260844493e-18, 6.728617974751348e-20),
    's0037': (7.514876308040153e-18, 2.4736072565256784e-16, 2.068007223798851e-15, 1.1232259566895664e-10, 2.5257298298195097e-14, 1.7295468863400847e-14, 1.8037854571206188e-14, 5.370958685677463e-26, 1.3990424841775125e-14, 5.032691811713677e-26, 5.421345326301528e-16, 4.0030690232683375e-15, 1.026805507221012e-16, 4.135662441713743e-29, 4.904511021287362e-16, 6.736408251315513e-28, 1.4718781748968013e-13, 4.859945881698704e-16, 2.3741148138888464e-18, 1.5684423554504254e-16, 4.05808833836766e-19),
    's0037_noise': (5.248216141187645e-18, 2.1071469222255779e-16, 2.4017246524898894e-15, 1.8849277694243938e-10, 1.8696500646503758e-14, 8.723328049492496e-15, 2.3702353556427636e-15, 6.271025365656158e-16, 2.419397147901403e-15, 9.14823772291129e-14, 4.3895280205791254e-16, 3.3163033950900367e-15, 5.648693318649478e-17, 1.3697810247181863e-15, 2.3935050447697337e-15, 1.1302070390684094e-13, 1.4718781748968013e-13, 2.0955933928250292e-16, 2.0873009402714096e-18, 3.256079352540256e-17, 1.3880752423129847e-19),
    's41': (6.581540867856006e-15, 2.7538735181131813e-16, 2.389202117397682e-15, 6.938893903907228e-18, 2.6308625411641052e-14, 1.0634165587605008e-14, 2.0679808167662332e-14, 5.547076062114792e-26, 7.404851244032016e-15, 1.0266000915372164e-26, 4.350875935435224e-16, 4.0030690232683375e-15, 9.584367780722725e-17, 1.4987145376557527e-29, 4.904511021287362e-16, 6.736408251315513e-28, 1.4718781748968013e-13, 3.2326795913010094e-16, 2.3741148138888464e-18, 7.287918722910053e-17, 4.05808833836766e-19),
    's41_noise': (3.3792413312028202e-15, 2.104436416794364e-16, 2.357706044286978e-15, 2.2833297752544723e-16, 1.1442666340280225e-14, 7.210076584168376e-15, 2.349605868212385e-15, 4.1222450800071364e-15, 5.605113473513244e-15, 2.3869795029440866e-14, 3.7176614868170144e-16, 3.3163033950900367e-15, 9.359714067160019e-17, 1.0633854907737827e-15, 2.3935050447697337e-15, 1.1302070390684094e-13, 1.4718781748968013e-13, 1.7424484164557663e-16, 2.0873009402714096e-18, 7.618214327605177e-18, 1.3880752423129847e-19),
    'rot180': (2.7668839441830073e-16, 2.056731521205002e-16, 4.315341486926805e-15, 3.3306690738754696e-15, 2.8838926041369056e-14, 5.246180434152758e-15, 1.7402550785405005e-14, 7.708387540332165e-26, 2.715891118538795e-15, 6.889007236559403e-27, 4.3943504056784294e-16, 3.3781248056327213e-15, 1.708270475444284e-16, 4.05789485329037e-29, 6.822196454785424e-16, 1.0093699204008243e-27, 1.4718781748968013e-13, 4.934662585500264e-16, 3.522868382554655e-18, 1.4155784275934694e-16, 1.101660141896925e-18),
    'rot180_noise': (4.1514101184469965e-16, 6.591949208711867e-16, 3.7529658200585736e-15, 7.049916206369744e-15, 3.488133176396402e-14, 8.999582763041802e-15, 2.0430847192819037e-14, 4.1750457258071805e-15, 4.848768955789673e-15, 2.1926904736346842e-14, 5.270577810995158e-16, 3.26258117744338e-15, 4.956667400742715e-17, 1.9285788244172153e-15, 2.8977335938748516e-15, 3.197442310920451e-14, 1.4718781748968013e-13, 4.2487638502396695e-16, 2.2697306612863045e-18, 4.1330972661273585e-17, 6.405686663610646e-20),
    'mirror': (3.060702732926579e-16, 1.7294108853316281e-15, 8.194226547297845e-14, 5.1431081615760377e-14, 2.3888768567459362e-14, 1.1837753000065732e-13, 2.3888768567459362e-14, 7.11263730204803e-16, 1.1837753000065732e-13, 1.836326646298403e-09, 5.844933911869354e-16, 4.0030690232683375e-15, 3.773955296491535e-16, 1.5064338665382593e-14, 6.559989728826571e-16, 1.660261654380296e-28, 1.969951979319262e-14, 3.1295495708794085e-16, 1.907160146159579e-18, 1.7328261221749575e-16, 8.844271138169668e-19),
    'mirror4': (5.909986042218485e-16, 6.007022136655937e-16, 1.5434973178046762e-16, 1.5942802633617248e-13, 1.1366694261175092e-14, 7.147060721024445e-15, 8.034473422940253e-15, 1.5513747242141412e-16, 7.147060721024445e-15, 1.0622613899613498e-11, 4.6379566853715914e-14, 1.479201478687849e-15, 4.6379566853715914e-14, 9.85345138815319e-12, 1.1042775103311026e-15, 5.526358438745504e-30, 3.493039191226899e-14, 3.168038748002644e-16, 2.70716313453451e-19, 3.168038748002644e-16, 2.70716313453451e-19),
    'mirror5': (5.892638807458717e-17, 2.5560066216345767e-16, 1.9524041671575842e-15, 2.0117241206207837e-13, 6.521049162894893e-15, 1.0796918914479647e-14, 2.0728014302803105e-15, 3.5973828083069037e-16, 1.0796918914479647e-14, 1.099209612220875e-11, 6.890321646579878e-15, 1.479201478687849e-15, 9.353628982466944e-15, 4.1104897263721796e-12, 4.955470828831561e-16, 2.3740503488743156e-30, 3.493039191226899e-14, 1.1340754724198376e-16, 2.70716313453451e-19, 1.1340754724198376e-16, 2.70716313453451e-19),
    'planar': (4.2912721986976265e-16, 2.2199039481640703e-16, 2.5804011705155006e-15, 1.4210854715202004e-14, 1.8693804905113863e-14, 7.273769880663525e-15, 1.6999374709668764e-14, 2.5066951754634502e-26, 5.110965178362173e-15, 1.3336631484184875e-27, 5.109223398430123e-16, 5.741137963784395e-15, 1.3061284448041627e-16, 2.2104850364908904e-29, 2.7967389302818588e-15, 4.058843396819596e-28, 1.499356194756274e-13, 4.0172877010046267e-16, 2.9559617558227508e-18, 1.3112063826327155e-16, 5.121545117980279e-19),
    'collinear': (0.0, 0.0, 0.0, 2.3780977187470853e-13, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 5.986964396464955e-16, 0.0, 3.727487069005164e-16, 3.1308289294429414e-14, 0.0, 0.0, 0.0, 1.2533377113932431e-16, 0.0, 8.310409652101391e-17, 0.0),
    'mode_se3': (0.0, 2.673100456263011e-16, 2.669305748659312e-15, 2.0961010704922955e-13, 2.1663646896340205e-14, 7.560900690262162e-15, 8.354262665363115e-15, 1.6836412906201526e-14, 2.1386569713799115e-15, 5.338091080275831e-14, 2.883977778811442e-16, 2.526299482108474e-15, 9.787635112112891e-17, 1.222980050563649e-16, 5.856860135766695e-16, 3.469446951953614e-16, 1.4718781748968013e-13, 1.4126434329480957e-16, 2.5467104350384608e-18, 1.9663446354034955e-17, 2.288047748770679e-19),
    'mode_origin': (0.0, 0.0, 5.009881398621019e-15, 0.0, 1.2320595661318573e-14, 5.151369782130377e-15, 4.817110252353096e-15, 8.23126289350995e-14, 1.2377252001094519e-15, 5.946632075648495e-15, 2.883977778811442e-16, 2.526299482108474e-15, 9.787635112112891e-17, 1.222980050563649e-16, 5.856860135766695e-16, 3.469446951953614e-16, 1.4718781748968013e-13, 1.4126434329480957e-16, 2.5467104350384608e-18, 1.9663446354034955e-17, 2.288047748770679e-19),
    'mode_origin_scale': (2.5221253037444047e-17, 0.0, 1.0826842894440247e-15, 2.1046275833214168e-11, 1.0392992618856595e-14, 5.151369782130377e-15, 3.4413932207405518e-15, 4.1348868773383174e-14, 1.2377252001094519e-15, 5.946632075648495e-15, 4.976759022251587e-16, 2.526299482108474e-15, 9.144906511736328e-17, 1.0448998437329049e-17, 5.856860135766695e-16, 3.469446951953614e-16, 1.4718781748968013e-13, 1.3371706797653694e-16, 2.5467104350384608e-18, 1.6472673241728006e-17, 2.288047748770679e-19),
    'invalid': (9.638557313396134e-17, 1.9662006398024623e-16, 2.6944863441152878e-15, 5.924150059399835e-13, 2.5573076642415593e-14, 6.101510355988049e-15, 1.903209319438178e-14, 2.1443282804782526e-15, 1.864502476023322e-15, 3.035072193569022e-14, 4.1467344965781527e-16, 3.1714539848459733e-15, 1.3857797830259255e-16, 8.027161834539553e-17, 7.567731163948821e-16, 4.719141744047306e-14, 6.600275881396556e-14, 1.417655750413473e-16, 2.2865786760027846e-18, 1.393369198233324e-17, 2.2737540677857625e-19),
    'permuted': (4.501607420159814e-16, 1.1416648876272362e-16, 2.7410729444560375e-15, 3.372302437298913e-15, 2.03135847986341e-14, 7.55514171325378e-15, 9.769041044854765e-15, 4.157806911264661e-15, 4.07441355299216e-15, 7.866321289284276e-15, 3.9997573395705865e-16, 4.0030690232683375e-15, 9.078837941850493e-17, 3.959506333917062e-16, 4.904511021287362e-16, 6.736408251315513e-28, 1.4718781748968013e-13, 3.0814380994753643e-16, 2.3741148138888464e-18, 4.93678330230592e-17, 4.05808833836766e-19),
    'overlong': (2.7755575615628914e-16, 3.9519169187096637e-16, 2.192690473634684e-15, 9.076073226310655e-15, 1.3543973817367432e-14, 1.0299890568942665e-14, 5.3624758035745665e-15, 8.298158167552305e-15, 8.153576843236048e-15, 1.581436685841849e-14, 3.6414624028820175e-16, 4.0030690232683375e-15, 1.4796522094053834e-16, 6.917209860457518e-17, 5.060574859617795e-16, 5.501827612771014e-28, 7.098488463697095e-14, 3.2456333187182423e-16, 2.3741148138888464e-18, 3.3323970210878684e-17, 3.8274085195185163e-19),
    'kitti_scale': (0.0, 0.0, 0.0, 1.06368247543287e-11, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.1655173354219173e-17, 1.5629858518551032e-15, 0.0, 0.0, 0.0, 1.157995682850299e-16, 0.0, 2.4015078120553923e-17, 0.0),
    'kitti_yaw': (0.0, 0.0, 0.0, 0.0, 0.0, 1.1428358259735205e-14, 0.0, 0.0, 8.489736691430494e-15, 2.7284841053187847e-11, 2.028000163634136e-16, 4.607483150434813e-15, 4.6458063091003865e-17, 5.245803791353865e-15, 1.654529784662559e-15, 3.8489177123235407e-16, 0.0, 2.0025214125807267e-16, 7.281306972834779e-19, 7.139471305817047e-17, 2.1736983008913482e-19),
    'kitti_short': (0.0, 0.0, 0.0, 2.2426505097428162e-14, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.1072414686508214e-17, 9.768661574094395e-17, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    'kitti_bad_end': (0.0, 0.0, 0.0, 1.13473674900888e-11, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 6.776263578034403e-20, 2.8449465006019636e-16, 0.0, 0.0, 0.0, 1.157995682850299e-16, 0.0, 2.4015078120553923e-17, 0.0),
}
STATS_WAY_DIFFERENCE = {'n0': (0.0, 0.0), 'n1': (0.0, 0.0), 'n2': (1.0863705768304754e-16, 0.0), 'n3': (1.973247953923618e-16, 0.0), 'equal': (0.0, 0.0), 'mantissa_byte': (2.168404344971009e-19, 5.828670879282072e-16), 'exponent': (16.703125, 9.82865582677337e+19), 'ties257': (6.76000054544712e-17, 0.0), 'ties256': (4.228388472693467e-17, 0.0), 'masked1025': (7.535205098774256e-17, 1.9206858326015208e-14), 'zeros': (0.0, 0.0)}

if __name__ == "__main__":
    print("WAY_DIFFERENCE = {")
    for name in cases():
        print("    %r: (%s)," % (name, ", ".join(repr(way_difference(name)[k]) for k in OUTPUTS)))
    print("}")
    print("STATS_WAY_DIFFERENCE = {%s}" % ", ".join("%r: %r" % (n, stats_way_difference(n)) for n in stats_cases()))
