"""Seeded frames for the PoseOptimization tests: map points in front of a camera with a known pose,
their mono or stereo observations through synthetic.KITTI_CAM with pixel noise and planted gross
outliers, and a start pose that is the truth perturbed. A problem is indexed by the frame's keypoints
(valid[i] = the keypoint has a map point), as include/orbfe_poseopt.h takes it."""
import numpy as np

from orb_slam2_2021_amd.synthetic import KITTI_CAM


def axis_rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


class Problem:
    """n keypoints, n_valid of them with a map point (scattered when n_valid < n).
    stereo: the share of valid keypoints with a right coordinate. outliers: the share of valid
    keypoints moved by 30..80 px. rot_deg / trans: the start pose's distance from the truth.
    garbage: every observation is a uniform pixel of the image (no pose explains them).
    at_origin: identity start pose, three points behind the camera, two at z = 0 exactly and one at
    the camera centre, so that 1/z is inf and 0/0 is NaN."""

    def __init__(self, n, seed, n_valid=None, stereo=0.5, noise=0.5, outliers=0.0, rot_deg=1.0, trans=0.03,
                 garbage=False, at_origin=False, one_sided=False):
        rng = np.random.default_rng(seed)
        cam = KITTI_CAM
        self.n = n
        self.k = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
        self.bf = np.float32(cam["bf"])
        fx, fy, cx, cy = [float(v) for v in self.k]
        bf = float(self.bf)
        n_valid = n if n_valid is None else n_valid
        self.valid = np.zeros(n, np.uint8)
        self.valid[np.sort(rng.choice(n, n_valid, replace=False))] = 1
        R = np.eye(3) if at_origin else axis_rotation(rng.normal(size=3), rng.uniform(-0.3, 0.3))
        t = np.zeros(3) if at_origin else rng.uniform(-1.0, 1.0, 3)
        pc = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(4, 20, n)], 1)
        self.xw = np.ascontiguousarray((pc - t) @ R, np.float32)
        pc = self.xw.astype(np.float64) @ R.T + t  # the float map points, projected exactly
        uv = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], 1)
        ur = uv[:, 0] - bf / pc[:, 2]
        is_stereo = rng.random(n) < stereo
        if noise > 0:
            uv = uv + rng.normal(0, noise, uv.shape)
            ur = ur + rng.normal(0, noise, n)
        bad = (rng.random(n) < outliers) & (self.valid == 1)
        shift = rng.uniform(30, 80, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
        if one_sided:  # every outlier pulls the same way: the robust first round is biased by them
            shift = np.abs(shift)
        uv[bad] += shift[bad]
        if garbage:
            uv = np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 376, n)], 1)
            bad = self.valid == 1
        self.planted_outlier = bad
        self.kp_un = np.ascontiguousarray(uv, np.float32)
        self.u_right = np.where(is_stereo, ur, -1.0).astype(np.float32)
        sigma2 = (np.float32(1.2) ** (2 * rng.integers(0, 4, n))).astype(np.float32)
        self.inv_sigma2 = (np.float32(1.0) / sigma2).astype(np.float32)  # mvInvLevelSigma2
        self.R_true, self.t_true = R, t
        dR = axis_rotation(rng.normal(size=3), np.deg2rad(rot_deg))
        dt = rng.normal(size=3)
        dt = dt / np.linalg.norm(dt) * trans
        Rs, ts = dR @ R, dR @ t + dt
        if at_origin:
            Rs, ts = np.eye(3), np.zeros(3)
            v = np.flatnonzero(self.valid)
            self.xw[v[0:3], 2] = [-3.0, -7.5, -1.0]
            self.xw[v[3:5], 2] = 0.0
            self.xw[v[5]] = 0.0
            self.u_right[v[3]] = -1.0  # one of the z = 0 edges mono (x / 0), one as drawn
            self.u_right[v[5]] = -1.0  # 0 / 0
            self.nan_edge = int(v[5])
        self.tcw = np.ascontiguousarray(np.hstack([Rs, ts[:, None]]), np.float32).reshape(12)
        self.R_start, self.t_start = Rs, ts
        # the valid-only invalid entries carry no data the solver may read
        inv = self.valid == 0
        self.xw[inv] = 0
        self.kp_un[inv] = 0
        self.u_right[inv] = -1
        self.inv_sigma2[inv] = 0


# name -> (Problem arguments, why the case exists)
CASES = {
    "n2": (dict(n=2, seed=1, stereo=0.0), "< 3 correspondences: returns 0, the pose bits untouched"),
    "n3": (dict(n=3, seed=2, stereo=0.0), "one round only (edges < 10)"),
    "n9": (dict(n=9, seed=3, stereo=0.0), "one round only, the largest such size"),
    "n10": (dict(n=10, seed=4), "the first size with four rounds"),
    "mono30": (dict(n=30, seed=5, stereo=0.0), "the monocular edge alone"),
    "stereo30": (dict(n=30, seed=6, stereo=1.0), "the stereo edge alone"),
    "n63": (dict(n=63, seed=7), "one short of a full set of lanes"),
    "n64": (dict(n=64, seed=8), "every lane owns exactly one edge"),
    "n65": (dict(n=65, seed=9), "lane 0 owns a second edge"),
    "n129": (dict(n=129, seed=10), "a third mask word with one bit"),
    "sparse": (dict(n=200, seed=11, n_valid=40), "valid[] handling: mask bits at their frame indices"),
    "outliers30": (dict(n=120, seed=20, noise=1.0, outliers=0.3, rot_deg=2.0, trans=0.05, one_sided=True),
                   "levels change between rounds; an edge flagged early is an inlier at the end"),
    "clean": (dict(n=80, seed=13, noise=0.0, rot_deg=2.0, trans=0.05), "ends by the _nBad rule"),
    "far": (dict(n=80, seed=14, rot_deg=20.0, trans=1.0), "a rejected trial: lambda *= ni"),
    "all_out": (dict(n=20, seed=15, garbage=True), "a round with no active edge (stop == 3)"),
    "behind": (dict(n=20, seed=16, at_origin=True), "z <= 0: inf / NaN stay bounded; NaN chi2 is an inlier"),
}
OUTLIER_SEEDS = (20, 22, 25)     # outliers30 and two more seeds of its shape
CLEAN_SEEDS = (13, 113, 213, 313)  # clean and three more noise-free scenes


def case(name):
    return Problem(**CASES[name][0])


def outlier_scene(seed):
    return Problem(**dict(CASES["outliers30"][0], seed=seed))


def clean_scene(seed):
    return Problem(**dict(CASES["clean"][0], seed=seed))
