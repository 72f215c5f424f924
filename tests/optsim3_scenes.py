"""Seeded loop-closure candidates for the OptimizeSim3 tests: points in front of camera 2, a known Sim3
S12 that takes them to camera 1, their observations in both keyframes with pixel noise and planted
gross outliers, and a start Sim3 that is the truth perturbed. A problem is indexed by KF1's keypoints
(valid[i] = the correspondence enters the optimisation), as include/orbfe_optsim3.h takes it."""
import numpy as np

from orb_slam2_2021_amd.synthetic import KITTI_CAM
from poseopt_scenes import axis_rotation

OTHER_CAM = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3)


class Problem:
    """n keypoints of KF1, n_valid of them with a correspondence (scattered when n_valid < n).
    scale: the true s12. outliers: the share of correspondences with one observation moved by 30..80 px.
    rot_deg / trans / scale_err: the start's distance from the truth. garbage: every observation is a
    uniform pixel (no Sim3 explains them). behind: one point lies behind camera 2's mapped view.
    nan_in: one observation is NaN. kf2_pose: the problem carries r2w / t2w (the result's scw)."""

    def __init__(self, n, seed, n_valid=None, scale=1.0, noise=0.5, outliers=0.0, n_outliers=None, rot_deg=1.0,
                 trans=0.03, scale_err=0.0, fix_scale=True, garbage=False, two_cameras=False, behind=False,
                 nan_in=False, kf2_pose=True, th2=10.0):
        rng = np.random.default_rng(seed)
        self.n = n
        cam1 = KITTI_CAM
        cam2 = OTHER_CAM if two_cameras else KITTI_CAM
        self.k1 = np.array([cam1["fx"], cam1["fy"], cam1["cx"], cam1["cy"]], np.float32)
        self.k2 = np.array([cam2["fx"], cam2["fy"], cam2["cx"], cam2["cy"]], np.float32)
        self.th2 = np.float32(th2)
        self.fix_scale = int(fix_scale)
        n_valid = n if n_valid is None else n_valid
        self.valid = np.zeros(n, np.uint8)
        self.valid[np.sort(rng.choice(n, n_valid, replace=False))] = 1
        R = axis_rotation(rng.normal(size=3), rng.uniform(-0.2, 0.2))
        t = rng.uniform(-0.5, 0.5, 3)
        p2 = np.stack([rng.uniform(-5, 5, n), rng.uniform(-2, 2, n), rng.uniform(6, 20, n)], 1)
        self.p3d2c = np.ascontiguousarray(p2, np.float32)
        p1 = scale * (self.p3d2c.astype(np.float64) @ R.T) + t
        self.p3d1c = np.ascontiguousarray(p1, np.float32)

        def project(k, p):
            p = p.astype(np.float64)
            return np.stack([float(k[0]) * p[:, 0] / p[:, 2] + float(k[2]), float(k[1]) * p[:, 1] / p[:, 2] + float(k[3])], 1)

        uv1, uv2 = project(self.k1, self.p3d1c), project(self.k2, self.p3d2c)
        if noise > 0:
            uv1 = uv1 + rng.normal(0, noise, uv1.shape)
            uv2 = uv2 + rng.normal(0, noise, uv2.shape)
        bad = (rng.random(n) < outliers) & (self.valid == 1)
        if n_outliers is not None:
            bad = np.zeros(n, bool)
            bad[rng.choice(np.flatnonzero(self.valid), n_outliers, replace=False)] = True
        shift = rng.uniform(30, 80, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
        in_first = rng.random(n) < 0.5
        uv1[bad & in_first] += shift[bad & in_first]
        uv2[bad & ~in_first] += shift[bad & ~in_first]
        if garbage:
            uv1 = np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 376, n)], 1)
            uv2 = np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 376, n)], 1)
            bad = self.valid == 1
        v = np.flatnonzero(self.valid)
        if behind:  # S12 maps it behind camera 1; camera 2 sees P3D1c as usual
            self.p3d2c[v[1], 2] = -3.0
            bad[v[1]] = True
        self.planted_outlier = bad
        self.kp_un1 = np.ascontiguousarray(uv1, np.float32)
        self.kp_un2 = np.ascontiguousarray(uv2, np.float32)
        if nan_in:
            self.kp_un2[v[2], 1] = np.nan
            self.nan_entry = int(v[2])
        sigma2 = (np.float32(1.2) ** (2 * rng.integers(0, 4, (n, 2)))).astype(np.float32)
        inv = (np.float32(1.0) / sigma2).astype(np.float32)  # mvInvLevelSigma2
        self.inv_sigma2_1 = np.ascontiguousarray(inv[:, 0])
        self.inv_sigma2_2 = np.ascontiguousarray(inv[:, 1])
        self.R_true, self.t_true, self.s_true = R, t, scale
        dR = axis_rotation(rng.normal(size=3), np.deg2rad(rot_deg))
        dt = rng.normal(size=3)
        dt = dt / np.linalg.norm(dt) * trans
        self.r12 = np.ascontiguousarray(dR @ R, np.float32).reshape(9)
        self.t12 = np.ascontiguousarray(dR @ t + dt, np.float32)
        self.s12 = np.float32(scale * (1.0 + scale_err))
        self.r2w = self.t2w = None
        if kf2_pose:
            self.r2w = np.ascontiguousarray(axis_rotation(rng.normal(size=3), rng.uniform(-1.0, 1.0)), np.float32).reshape(9)
            self.t2w = rng.uniform(-3.0, 3.0, 3).astype(np.float32)
        # the invalid entries carry no data the solver may read
        inv = self.valid == 0
        for a in (self.p3d1c, self.p3d2c, self.kp_un1, self.kp_un2, self.inv_sigma2_1, self.inv_sigma2_2):
            a[inv] = 0


# name -> (Problem arguments, why the case exists)
CASES = {
    "n0": (dict(n=12, seed=1, n_valid=0), "no valid entry: no step, returns 0"),
    "n9": (dict(n=9, seed=2), "9 correspondences: round 1 runs, returns 0, Sim3 untouched"),
    "n10": (dict(n=10, seed=3), "the first size with two rounds"),
    "n64": (dict(n=64, seed=4), "every lane owns exactly one correspondence"),
    "n65": (dict(n=65, seed=5), "lane 0 owns a second correspondence"),
    "n130_sparse": (dict(n=130, seed=6, n_valid=40, kf2_pose=False), "valid entries scattered; a third mask word; no scw"),
    "clean": (dict(n=80, seed=7, noise=0.0, rot_deg=0.5, trans=0.02), "nBad == 0: 5 more iterations"),
    "outliers": (dict(n=120, seed=20, noise=0.5, outliers=0.3, rot_deg=2.0, trans=0.05), "nBad > 0: 10 more iterations"),
    "drops_below_10": (dict(n=14, seed=9, n_outliers=6), "14 correspondences, 8 after round 1: returns 0"),
    "all_out": (dict(n=20, seed=10, garbage=True), "every correspondence fails the gate"),
    "free_scale": (dict(n=100, seed=11, scale=1.3, scale_err=0.05, fix_scale=False), "fix_scale = 0, true scale 1.3"),
    "fix_scale": (dict(n=100, seed=11, scale=1.3, scale_err=0.05, fix_scale=True), "the same scene, scale fixed"),
    "two_cameras": (dict(n=90, seed=12, two_cameras=True), "K1 != K2"),
    "far_start": (dict(n=80, seed=13, rot_deg=25.0, trans=1.5), "a start far off: a round has rejected trials"),
    "behind": (dict(n=40, seed=14, behind=True), "a point mapped to z < 0 in camera 1"),
    "nan_in": (dict(n=30, seed=15, nan_in=True, rot_deg=0.01, trans=0.0005),
               "one NaN observation: NONFINITE, loops run their caps; the NaN chi2 keeps its correspondence"),
    "cap5": (dict(n=80, seed=40, rot_deg=60.0, trans=3.0, th2=1e6), "nBad == 0 and round 2 ends at its cap of 5"),
    "cap10": (dict(n=80, seed=25, rot_deg=60.0, trans=3.0, th2=1e6), "nBad > 0 and round 2 ends at its cap of 10"),
}
OUTLIER_SEEDS = (20, 21, 22)       # outliers and two more seeds of its shape
CLEAN_SEEDS = (7, 107, 207, 307)   # clean and three more noise-free scenes


def case(name):
    return Problem(**CASES[name][0])


def outlier_scene(seed):
    return Problem(**dict(CASES["outliers"][0], seed=seed))


def clean_scene(seed, fix_scale=True, scale=1.0):
    return Problem(**dict(CASES["clean"][0], seed=seed, fix_scale=fix_scale, scale=scale))
