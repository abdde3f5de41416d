"""evaluation.py of the reference (evaluate(), evaluation.py:86-500) on the device: repeatability and localisation error
(-r), homography correctness, matching score and mean AP (-homo) of descriptor exports.

  python -m semantic_superpoint_amd.evaluation <predictions dir> [-r] [-homo]

reads the exporter's `<int>.npz` files in numeric order, evaluates them in batches of pairs on one GPU and appends the
reference's summary to `<dir>/result.txt` and writes `<dir>/result.npz`.  Evaluator.run_device evaluates the device
tensors of DescriptorExporter.run_device without a host copy of points or descriptors.  StreamingEvaluator keeps the
per-pair metrics and their sums on the device as well and reads them once per set (a validation round, an export).  The RANSAC step restates
cv2.findHomography; there is no CPU fallback.
"""
import argparse
import os

import numpy as np
import torch

from . import lib as L

HOMOGRAPHY_THRESH = [1, 3, 5, 10, 20, 50]
TOP_K = 1000          # evaluation.py:101 top_K
REP_THD = 3           # evaluation.py:96 rep_thd
NN_THRESH = 1.2       # evaluation.py:231 getMatches
CORNER_SHAPE = (240, 320)  # compute_homography's default `shape` (evaluate never passes one)
BATCH_PAIRS = 16


def pair_seeds(file_numbers):
    """RANSAC seeds of pairs named by their file numbers: (crossCheck call, mAP call)."""
    f = np.asarray(file_numbers, dtype=np.int64)
    return 2 * f, 2 * f + 1


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("the evaluation needs a HIP device: there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def correctness_of(H, real_H, shape=CORNER_SHAPE, thresh=HOMOGRAPHY_THRESH):
    """descriptor_evaluation.py:127-149: mean corner distance of H against real_H <= each threshold; H None = no model."""
    if H is None:
        return np.zeros(len(thresh), dtype=bool)
    corners = np.array([[0, 0, 1], [0, shape[0] - 1, 1], [shape[1] - 1, 0, 1], [shape[1] - 1, shape[0] - 1, 1]])
    real_w = np.dot(corners, np.transpose(real_H))
    real_w = real_w[:, :2] / real_w[:, 2:]
    est_w = np.dot(corners, np.transpose(H))
    est_w = est_w[:, :2] / est_w[:, 2:]
    mean_dist = np.mean(np.linalg.norm(real_w - est_w, axis=1))
    return mean_dist <= np.asarray(thresh)


def rep_from_counts(row):
    """(repeatability, localization_err) of compute_repeatability from the device row N1, N2, count1, count2, sum1, sum2:
    repeatability 0 (an int, as the reference) when nothing repeats, localization_err -1 then."""
    n1, n2, c1, c2, s1, s2 = (row[k] for k in range(6))
    c = np.int64(c1) + np.int64(c2)
    if c == 0:
        return 0, -1
    rep = c / (np.int64(n1) + np.int64(n2))
    return rep, 0 + s1 / c + s2 / c


class Evaluator:
    """Batched -r -homo evaluation of export pairs on one GPU.  height / width: the images' shape."""

    def __init__(self, height, width, repeatability=True, homography=True, keep_k=TOP_K, rep_thd=REP_THD,
                 nn_thresh=NN_THRESH):
        self.height, self.width = int(height), int(width)
        self.repeatability, self.homography = bool(repeatability), bool(homography)
        self.keep_k, self.rep_thd, self.nn_thresh = int(keep_k), float(rep_thd), float(nn_thresh)

    def run_points(self, pts, count, desc, homographies, seeds):
        """pts: float64 [2P,cap,3] rows (x, y, conf) interleaved (image 2p, warped image 2p + 1), count int32 [2P],
        desc float32 [2P,cap,256] unit rows, homographies [P,3,3] (host), seeds: per-pair ints (pair_seeds of its file
        number).  Returns one dict of metrics per pair (the reference's per-file values)."""
        P = count.numel() // 2
        dev = pts.device
        Hs = np.asarray(homographies, dtype=np.float64).reshape(P, 3, 3)
        out = {}
        if self.repeatability or self.homography:
            Hd = torch.from_numpy(Hs).to(dev)
            Hi = torch.from_numpy(np.stack([np.linalg.inv(h) for h in Hs])).to(dev)
            out["rep"] = L.op_eval_repeatability(pts, count, pts[1:], count[1:], Hd, Hi, self.height, self.width,
                                                 self.keep_k, self.rep_thd, pair_stride=2, n_pairs=P)
        if self.homography:
            s_cc, s_nn = pair_seeds(seeds)
            m, nm = L.op_match_two_way(desc, count, desc[1:], count[1:], float("inf"), pair_stride=2, n_pairs=P)
            out["cc"] = L.op_eval_ransac(pts, pts[1:], m, nm, torch.from_numpy(s_cc).to(dev), pair_stride=2)
            m, nm = L.op_match_two_way(desc, count, desc[1:], count[1:], self.nn_thresh, pair_stride=2, n_pairs=P)
            out["nn"] = L.op_eval_ransac(pts, pts[1:], m, nm, torch.from_numpy(s_nn).to(dev), pair_stride=2,
                                         want_ap=True)
        # the only host round trip: per-pair scalars and the estimated H
        host = {}
        if "rep" in out:
            host["rep"] = out["rep"].cpu().numpy()
        if self.homography:
            host["H"] = out["cc"]["H"].cpu().numpy()
            host["n_inl"] = out["cc"]["n_inliers"].cpu().numpy()
            host["status"] = out["cc"]["status"].cpu().numpy()
            host["ap"] = out["nn"]["ap"].cpu().numpy()
            host["n1"] = count[0::2].cpu().numpy()
        res = []
        for p in range(P):
            r = {}
            if self.repeatability:
                r["rep"], r["loc_err"] = rep_from_counts(host["rep"][p])
            if self.homography:
                ok = host["status"][p] == 0
                r["correctness"] = correctness_of(host["H"][p] if ok else None, Hs[p])
                r["homography"] = host["H"][p]
                n_unw = int(host["rep"][p][6])
                den = int(host["n1"][p]) + n_unw
                r["mscore"] = np.float64(2 * int(host["n_inl"][p])) / np.float64(den) if den > 0 else np.float64(0.0)
                ap = float(host["ap"][p])
                r["mAP"] = ap if ap > 0 else 0
            res.append(r)
        return res

    def run_device(self, o, homographies, seeds, subpixel=True):
        """Evaluates the dict of DescriptorExporter.run_device (device tensors pts [2P,cap,5] rows (x, y, conf, sx, sy),
        count [2P], desc [2P,cap,256]) with no host copy of points or descriptors.  subpixel: the exporter's setting
        (prob = x + sx - 2 in float64, as export.py stores it)."""
        pts5 = o["pts"]
        pts = pts5[:, :, :3].double()
        if subpixel:
            pts[:, :, :2] = pts[:, :, :2] + pts5[:, :, 3:5].double() - 2
        return self.run_points(pts.contiguous(), o["count"], o["desc"], homographies, seeds)


class StreamingEvaluator:
    """The -r -homo metrics of a set of pairs that is fed batch by batch and never leaves the device (DESIGN.md section
    21): every update queues op_eval_repeatability, the two matchers, the two RANSACs and op_eval_accumulate on the
    current stream and reads nothing back; result() makes the one read of the state block and the per-pair rows.
    height / width: the images' shape; capacity: pairs whose rows are kept (pairs past it still count in the sums and
    in `rows_dropped`); corner_shape: the (height, width) whose corners measure homography correctness -
    compute_homography's default (240, 320) as `evaluate` uses it, or the images' own shape.  Pairs are numbered in
    feeding order from 0 and pair f draws its RANSAC seeds from pair_seeds(f), like the file numbers of `evaluate`.
    With repeatability off and homography on, the repeatability rows are still computed (the matching score needs their
    unwarped-point count) and result() leaves the repeatability keys out."""

    def __init__(self, height, width, device, capacity, repeatability=True, homography=True, keep_k=TOP_K, rep_thd=REP_THD,
                 nn_thresh=NN_THRESH, corner_shape=CORNER_SHAPE):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("StreamingEvaluator needs a HIP device (got %s): no CPU fallback exists" % self.device)
        self.height, self.width, self.capacity = int(height), int(width), int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity >= 1 pairs required (got %d)" % self.capacity)
        self.repeatability, self.homography = bool(repeatability), bool(homography)
        if not (self.repeatability or self.homography):
            raise ValueError("repeatability or homography (or both) must be on")
        self.keep_k, self.rep_thd, self.nn_thresh = int(keep_k), float(rep_thd), float(nn_thresh)
        self.corner_shape = (int(corner_shape[0]), int(corner_shape[1]))
        self.rows, self.state = L.eval_metrics_state(self.capacity, self.device)
        self.pairs = 0  # pairs fed since reset(): the next pair's number (host side; nothing is read back for it)

    def reset(self):
        self.rows.zero_()
        self.state.zero_()
        self.pairs = 0

    def _pixel(self, t, name, P):
        if torch.is_tensor(t) and t.is_cuda:
            if t.dtype != torch.float64 or tuple(t.shape) != (P, 3, 3):
                raise ValueError("%s on the device must be float64 [%d,3,3] (got %s %s)" % (name, P, t.dtype, tuple(t.shape)))
            return t.contiguous()
        a = t.detach().numpy() if torch.is_tensor(t) else np.asarray(t)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(P, 3, 3)).to(self.device)

    def update_points(self, pts, count, desc, homographies=None, pair_stride=2, pts2=None, count2=None, desc2=None,
                      hom_inv=None, normalised=None):
        """The next P pairs.  pts float64 [P*pair_stride,cap,3] rows (x, y, conf), count int32, desc float32
        [..,cap,256] unit rows: pair p's image is entry p * pair_stride; its warped image is that entry of pts2 / count2 /
        desc2, or entry p * pair_stride + 1 of the same arrays when they are None (the exporter's interleaved layout).
        homographies: the true pixel matrices [P,3,3], host (any array) or device float64, with hom_inv beside them
        (default for host matrices: np.linalg.inv, as Evaluator; device matrices need it) - or normalised=hn, the
        trainer's device float32 [P,3,3] (sample["homographies"]), converted by op_eval_pixel_homographies.
        No host read."""
        for t, nm in ((pts, "pts"), (count, "count"), (desc, "desc")):
            L._need_gpu(t, nm)
        if pts.dim() != 3 or pts.shape[1] > L.MATCH_MAX_POINTS:
            raise ValueError("at most %d points per image (the arrays hold %s)" % (L.MATCH_MAX_POINTS, tuple(pts.shape)))
        if (homographies is None) == (normalised is None):
            raise ValueError("update_points(homographies=pixel matrices) or update_points(normalised=hn)")
        if (pts2 is None) != (count2 is None) or (pts2 is None) != (desc2 is None):
            raise ValueError("pts2, count2 and desc2 come together")
        pair_stride = int(pair_stride)
        if normalised is not None:
            if not torch.is_tensor(normalised) or normalised.dtype != torch.float32 or normalised.dim() != 3 \
                    or tuple(normalised.shape[1:]) != (3, 3):
                raise ValueError("normalised must be a device float32 [P,3,3] tensor")
            if hom_inv is not None:
                raise ValueError("hom_inv belongs to pixel homographies, not to normalised ones")
            P = normalised.shape[0]
        else:
            P = (homographies.numel() if torch.is_tensor(homographies) else np.asarray(homographies).size) // 9
        if pts2 is None:
            if pair_stride < 2:
                raise ValueError("interleaved pairs need pair_stride >= 2")
            pts2, count2, desc2 = pts[1:], count[1:], desc[1:]
            n2 = pts.shape[0] - 1
        else:
            n2 = pts2.shape[0]
            if pts2.shape[1:] != pts.shape[1:]:
                raise ValueError("pts2 must have the cap of pts")
        if P < 1 or pts.shape[0] != P * pair_stride or count.numel() != pts.shape[0] or desc.shape[:2] != pts.shape[:2] \
                or n2 < (P - 1) * pair_stride + 1:
            raise ValueError("%d homographies do not match point arrays of %d entries at stride %d"
                             % (P, pts.shape[0], pair_stride))
        if normalised is not None:
            Hd, Hi = L.op_eval_pixel_homographies(normalised, self.height, self.width)
        else:
            if hom_inv is None:
                if torch.is_tensor(homographies) and homographies.is_cuda:
                    raise ValueError("device homographies need hom_inv (or pass normalised=hn)")
                Hs = np.asarray(homographies, dtype=np.float64).reshape(P, 3, 3)
                hom_inv = np.stack([np.linalg.inv(h) for h in Hs])
            Hd, Hi = self._pixel(homographies, "homographies", P), self._pixel(hom_inv, "hom_inv", P)
        f0 = self.pairs
        rep = L.op_eval_repeatability(pts, count, pts2, count2, Hd, Hi, self.height, self.width, self.keep_k, self.rep_thd,
                                      pair_stride=pair_stride, n_pairs=P)
        cc = nn = None
        if self.homography:
            s_cc, s_nn = pair_seeds(np.arange(f0, f0 + P))
            m, nm = L.op_match_two_way(desc, count, desc2, count2, float("inf"), pair_stride=pair_stride, n_pairs=P)
            cc = L.op_eval_ransac(pts, pts2, m, nm, torch.from_numpy(s_cc).to(self.device), pair_stride=pair_stride)
            m, nm = L.op_match_two_way(desc, count, desc2, count2, self.nn_thresh, pair_stride=pair_stride, n_pairs=P)
            nn = L.op_eval_ransac(pts, pts2, m, nm, torch.from_numpy(s_nn).to(self.device), pair_stride=pair_stride,
                                  want_ap=True)
        for a in range(0, P, L.EVAL_ACC_MAX_PAIRS):
            b = min(P, a + L.EVAL_ACC_MAX_PAIRS)
            kw = {}
            if self.homography:
                kw = dict(ransac={k: cc[k][a:b] for k in ("H", "n_inliers", "status")}, ap=nn["ap"][a:b],
                          n1=count[a * pair_stride:], pair_stride=pair_stride, hom=Hd[a:b])
            L.op_eval_accumulate(self.rows, self.state, f0 + a, rep=rep[a:b], corner_shape=self.corner_shape,
                                 thresholds=HOMOGRAPHY_THRESH, **kw)
        self.pairs = f0 + P

    @staticmethod
    def _points64(pts5, subpixel):
        pts = pts5[:, :, :3].double()
        if subpixel:  # prob = x + sx - 2 in float64, as export.py stores it (Evaluator.run_device)
            pts[:, :, :2] = pts[:, :, :2] + pts5[:, :, 3:5].double() - 2
        return pts.contiguous()

    def update_device(self, o, homographies, subpixel=True, hom_inv=None):
        """The dict of DescriptorExporter.run_device (interleaved pts [2P,cap,5], count [2P], desc [2P,cap,256]) with the
        pairs' true pixel homographies; subpixel: the exporter's setting."""
        self.update_points(self._points64(o["pts"], subpixel), o["count"], o["desc"], homographies, hom_inv=hom_inv)

    def update_views(self, d0, d1, hn, subpixel=True):
        """Two Engine.describe_points dicts over the B images of a training pair's two views (image b of d0 against image
        b of d1) and the step's normalised homographies hn (device float32 [B,3,3])."""
        self.update_points(self._points64(d0["pts"], subpixel), d0["count"], d0["desc"], pair_stride=1,
                           pts2=self._points64(d1["pts"], subpixel), count2=d1["count"], desc2=d1["desc"], normalised=hn)

    def result(self):
        """The one host read (state block and rows, in one copy) -> the summary: summarize's keys as means over the pairs
        fed (sum / count, formed here in fp64), plus `pairs`, `no_model`, `rows_dropped` and `rows`, the float64
        [min(pairs, capacity), 16] per-pair rows (include/ssp_hip.h).  repeatability is 0 and localization_err NaN when
        no pair counts towards them."""
        n = min(self.pairs, self.capacity)
        host = torch.cat([self.state, self.rows[:n].reshape(-1)]).cpu().numpy()
        st, rows = host[:L.EVAL_STATE_WORDS], host[L.EVAL_STATE_WORDS:].reshape(n, L.EVAL_ROW_WORDS)
        pairs = st[0]
        out = {"pairs": int(pairs), "rows_dropped": int(st[13]), "rows": rows}
        if self.repeatability:
            out["repeatability"] = st[1] / pairs if pairs > 0 else np.float64(0.0)
            out["localization_err"] = st[2] / st[3] if st[3] > 0 else np.float64("nan")
        if self.homography:
            nan = np.float64("nan")
            out["correctness"] = st[4:10] / pairs if pairs > 0 else np.full(6, nan)
            out["homography_thresh"] = HOMOGRAPHY_THRESH
            out["mscore"] = st[10] / pairs if pairs > 0 else nan
            out["mAP"] = st[11] / pairs if pairs > 0 else nan
            out["no_model"] = int(st[12])
        return out

    def per_file(self, rows=None):
        """The rows as the per-pair dicts of Evaluator.run_points (without the estimated homography)."""
        rows = self.result()["rows"] if rows is None else rows
        res = []
        for r in rows:
            d = {}
            if self.repeatability:
                d["rep"], d["loc_err"] = (0, -1) if r[1] == -1 else (r[0], r[1])
            if self.homography:
                d["correctness"] = r[2:8] != 0
                d["mscore"] = r[8]
                d["mAP"] = r[9] if r[9] > 0 else 0
            res.append(d)
        return res

    def write(self, path, files):
        """result.txt / result.npz of `evaluate` for the pairs fed (named `files`, in feeding order) -> summarize's dict."""
        per_file = self.per_file()
        if len(files) != len(per_file):
            raise ValueError("%d names for %d kept rows" % (len(files), len(per_file)))
        return summarize(path, list(files), per_file, self.repeatability, self.homography, output_img=False)


def _upload(datas, dev):
    """Pads a batch of npz pairs into the interleaved device layout."""
    counts = []
    for d in datas:
        counts += [d["prob"].shape[0], d["warped_prob"].shape[0]]
    cap = max(1, max(counts))
    if cap > L.MATCH_MAX_POINTS:
        raise ValueError("a file holds %d points; the device evaluation takes at most %d per image"
                         % (cap, L.MATCH_MAX_POINTS))
    n = len(counts)
    pts = np.zeros((n, cap, 3))
    desc = np.zeros((n, cap, 256), dtype=np.float32)
    for p, d in enumerate(datas):
        for k, tag in ((2 * p, ""), (2 * p + 1, "warped_")):
            c = counts[k]
            pts[k, :c] = d[tag + "prob"][:, :3]
            desc[k, :c] = d[tag + "desc"]
    return (torch.from_numpy(pts).to(dev), torch.tensor(counts, dtype=torch.int32, device=dev),
            torch.from_numpy(desc).to(dev))


def _single(data, repeatability, homography, keep_k=TOP_K, rep_thd=REP_THD):
    img = np.asarray(data["image"])
    ev = Evaluator(img.shape[0], img.shape[1], repeatability, homography, keep_k=keep_k, rep_thd=rep_thd)
    d = {k: np.asarray(data[k]) for k in ("prob", "warped_prob", "desc", "warped_desc", "homography") if k in data}
    if "desc" not in d:
        d["desc"] = np.zeros((d["prob"].shape[0], 256), np.float32)
        d["warped_desc"] = np.zeros((d["warped_prob"].shape[0], 256), np.float32)
    pts, cnt, desc = _upload([d], _device())
    return ev.run_points(pts, cnt, desc, d["homography"][None], [0])[0]


def compute_repeatability(data, keep_k_points=300, distance_thresh=3, verbose=False):
    """evaluations/detector_evaluation.py:153-275 for one pair on the device -> (repeatability, localization_err).
    Unlike the reference, data["prob"] is not overwritten with the warped points."""
    r = _single(data, True, False, keep_k=keep_k_points, rep_thd=distance_thresh)
    return r["rep"], r["loc_err"]


def compute_homography(data, keep_k_points=1000, correctness_thresh=3, orb=False, shape=CORNER_SHAPE, seed=0):
    """evaluations/descriptor_evaluation.py:65-158 for one pair on the device: crossCheck matches, the device RANSAC
    (seeded) and correctness of the corners of `shape`.  Returns the reference's keys correctness, keypoints1,
    keypoints2, matches ([L,4] = x1, y1, x2, y2), mscores, inliers and homography."""
    if orb:
        raise ValueError("orb (Hamming) descriptors are not supported")
    dev = _device()
    pts, cnt, desc = _upload([{k: np.asarray(data[k]) for k in ("prob", "warped_prob", "desc", "warped_desc")}], dev)
    m, nm = L.op_match_two_way(desc, cnt, desc[1:], cnt[1:], float("inf"), pair_stride=2, n_pairs=1)
    r = L.op_eval_ransac(pts, pts[1:], m, nm, torch.tensor([int(seed)], dtype=torch.int64, device=dev), pair_stride=2)
    k = int(nm.item())
    mm = m[0, :k].cpu().numpy()
    i, j, dist = mm[:, 0].astype(int), mm[:, 1].astype(int), mm[:, 2].astype(np.float64)
    kp, wkp = np.asarray(data["prob"])[:, [1, 0]], np.asarray(data["warped_prob"])[:, [1, 0]]
    ok = int(r["status"].item()) == 0
    H = r["H"][0].cpu().numpy() if ok else np.identity(3)
    corr = correctness_of(H if ok else None, np.asarray(data["homography"]), shape, np.atleast_1d(correctness_thresh))
    return {
        "correctness": corr if np.ndim(correctness_thresh) else corr[0],
        "keypoints1": kp,
        "keypoints2": wkp,
        "matches": np.hstack((kp[i][:, [1, 0]], wkp[j][:, [1, 0]])),
        "mscores": dist / dist.max() if k else dist,
        "inliers": r["mask"][0, :k].cpu().numpy(),
        "homography": H,
    }


def find_files_with_ext(directory, extension=".npz"):
    """evaluation.py:64-79: the `<number>.npz` files of a directory."""
    def isfloat(v):
        try:
            float(v)
            return True
        except ValueError:
            return False
    return [f for f in os.listdir(directory) if f.endswith(extension) and isfloat(f[:-4])]


def summarize(path, files, per_file, repeatability, homography, output_img=False):
    """evaluation.py:402-500: appends the summary and the details to <path>/result.txt, writes <path>/result.npz.
    per_file: one metrics dict per file (Evaluator.run_points).  Returns the dict stored in result.npz."""
    rep = [r["rep"] for r in per_file] if repeatability else []
    loc = [r["loc_err"] for r in per_file if repeatability and r["loc_err"] > 0]
    correctness = [r["correctness"] for r in per_file] if homography else []
    mscore = [r["mscore"] for r in per_file] if homography else []
    mAP = [r["mAP"] for r in per_file] if homography else []
    with open(path + "/result.txt", "a") as f:
        f.write("path: " + path + "\n")
        f.write("output Images: " + str(output_img) + "\n")
        if repeatability:
            f.write("repeatability threshold: " + str(REP_THD) + "\n")
            f.write("repeatability: " + str(np.array(rep).mean()) + "\n")
            f.write("localization error: " + str(np.array(loc).mean()) + "\n")
        if homography:
            f.write("Homography estimation: " + "\n")
            f.write("Homography threshold: " + str(HOMOGRAPHY_THRESH) + "\n")
            f.write("Average correctness: " + str(np.array(correctness).mean(axis=0)) + "\n")
            f.write("nn mean AP: " + str(np.array(mAP).mean()) + "\n")
            f.write("matching score: " + str(np.array(mscore).mean(axis=0)) + "\n")
        f.write("====== details =====" + "\n")
        for i in range(len(files)):
            f.write("file: " + files[i])
            if repeatability:
                f.write("; rep: " + str(rep[i]))
            if homography:
                f.write("; correct: " + str(correctness[i]))
                f.write("; mscore: " + str(mscore[i]))
                f.write(":, mean AP: " + str(mAP[i]))
            f.write("\n")
        f.write("======== end ========" + "\n")
    out = {"repeatability": rep, "localization_err": loc, "correctness": np.array(correctness),
           "homography_thresh": HOMOGRAPHY_THRESH, "mscore": mscore, "mAP": np.array(mAP)}
    np.savez(path + "/result.npz", **out)
    return out


REFUSED = (("sift", "--sift (SIFT exports)"), ("outputImg", "--outputImg (OpenCV drawing)"),
           ("plotMatching", "--plotMatching (match drawing)"), ("split", "--split"))


def evaluate(args, batch_pairs=BATCH_PAIRS, **options):
    """evaluation.py:86-500 with the reference's args (path, repeatibility, homography; sift, outputImg, plotMatching
    and split are refused).  Returns the dict written to result.npz.  Every pair needs at least one point per image
    only for the homography's matches; a pair whose RANSAC finds no model scores six False, mscore 0 and AP 0."""
    for name, what in REFUSED:
        if getattr(args, name, False):
            raise ValueError("%s is not supported by the device evaluation" % what)
    path = args.path
    rep_on, homo_on = bool(args.repeatibility), bool(args.homography)
    files = find_files_with_ext(path)
    files.sort(key=lambda x: int(x[:-4]))
    dev = _device()
    per_file = []
    k = 0
    while k < len(files):
        datas, nums = [], []
        shape = None
        while k < len(files) and len(datas) < batch_pairs:
            d = np.load(os.path.join(path, files[k]))
            d = {n: d[n] for n in ("image", "prob", "warped_prob", "desc", "warped_desc", "homography")}
            if shape is not None and d["image"].shape != shape:
                break
            shape = d["image"].shape
            datas.append(d)
            nums.append(int(files[k][:-4]))
            k += 1
        ev = Evaluator(shape[0], shape[1], rep_on, homo_on)
        pts, cnt, desc = _upload(datas, dev)
        per_file += ev.run_points(pts, cnt, desc, np.stack([d["homography"] for d in datas]), nums)
    return summarize(path, files, per_file, rep_on, homo_on, output_img=False)


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("path", type=str)
    parser.add_argument("--sift", action="store_true", help="use sift matches (not supported)")
    parser.add_argument("-o", "--outputImg", action="store_true")
    parser.add_argument("-r", "--repeatibility", action="store_true")
    parser.add_argument("-homo", "--homography", action="store_true")
    parser.add_argument("-plm", "--plotMatching", action="store_true")
    parser.add_argument("-s", "--split", action="store_true", help="split in ilumination and viewpoint changes")
    args = parser.parse_args(argv)
    try:
        out = evaluate(args)
    except ValueError as e:
        parser.error(str(e))
    if args.repeatibility:
        print("repeatability: ", np.array(out["repeatability"]).mean())
        print("localization error over ", len(out["localization_err"]), " images : ",
              np.array(out["localization_err"]).mean())
    if args.homography:
        print("homography estimation threshold", HOMOGRAPHY_THRESH)
        print("correctness_ave", out["correctness"].mean(axis=0))
        print("matching score", np.array(out["mscore"]).mean(axis=0))
        print("mean AP", out["mAP"].mean())
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
