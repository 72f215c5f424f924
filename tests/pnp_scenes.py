"""Seeded relocalisation scenes for the PnP solver tests: map points in front of a camera with a
known pose, their projections through a KITTI-like K with pixel noise, and a share of outliers."""
import numpy as np

KITTI_K = (718.856, 718.856, 607.1928, 185.2157)  # fx, fy, cx, cy
RELOC = (0.99, 10, 300, 4, 0.5, 5.991)            # Tracking::Relocalization's SetRansacParameters


def rotation(rng, max_angle=0.3):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-max_angle, max_angle)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


class Scene:
    def __init__(self, n, seed, noise=0.5, outliers=0.3, planar=False, duplicate=False):
        rng = np.random.default_rng(seed)
        self.n = n
        self.R = rotation(rng)
        self.t = rng.uniform(-1.0, 1.0, 3)
        pc = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(4, 20, n)], 1)
        if planar:  # all map points on one world plane: the third PCA singular value is ~0
            pw = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), np.full(n, 3.0)], 1)
            pc = pw @ self.R.T + self.t + np.array([0, 0, 8.0])
            self.t = self.t + np.array([0, 0, 8.0])
        else:
            pw = (pc - self.t) @ self.R
        if duplicate and n >= 2:
            pw[1] = pw[0]
            pc[1] = pc[0]
        fx, fy, cx, cy = KITTI_K
        uv = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], 1)
        uv += rng.normal(0, noise, uv.shape) if noise > 0 else 0
        if duplicate and n >= 2:
            uv[1] = uv[0]
        bad = rng.random(n) < outliers
        uv[bad] += rng.uniform(-80, 80, (int(bad.sum()), 2))
        self.outlier = bad
        self.p3dw = np.ascontiguousarray(pw, np.float32)
        self.p2d = np.ascontiguousarray(uv, np.float32)
        self.sigma2 = (np.float32(1.2) ** (2 * rng.integers(0, 4, n))).astype(np.float32)
        self.k = np.array(KITTI_K, np.float32)


def draws(n, n_hyp, seed):
    """RandomInt(0, size - 1) of the four picks of n_hyp iterations: (n_hyp, 4) int32."""
    rng = np.random.default_rng(seed)
    hi = np.array([n, n - 1, n - 2, n - 3], np.int64)
    return rng.integers(0, hi, (n_hyp, 4)).astype(np.int32)


# The cases the GPU test solves and tests/test_pnp_ref.py's coverage test inspects:
# name -> (Scene arguments, SetRansacParameters arguments, hypotheses drawn, draw seed)
CASES = {
    "n4": (dict(n=4, seed=11, noise=0.0, outliers=0.0), (0.99, 4, 300, 4, 0.5, 5.991), 3, 1),
    "n5": (dict(n=5, seed=12, noise=0.2, outliers=0.0), (0.99, 4, 300, 4, 0.5, 5.991), 5, 2),
    "n63": (dict(n=63, seed=13, noise=0.5, outliers=0.3), (0.99, 10, 300, 4, 0.3, 5.991), 4, 3),
    "n64": (dict(n=64, seed=14, noise=0.3, outliers=0.0), (0.99, 10, 300, 4, 0.3, 5.991), 3, 4),
    "n65": (dict(n=65, seed=15, noise=0.3, outliers=0.0), (0.99, 10, 300, 4, 0.3, 5.991), 5, 5),
    "h1": (dict(n=30, seed=16, noise=0.5, outliers=0.2), (0.99, 10, 300, 4, 0.3, 5.991), 1, 6),
    "h24": (dict(n=30, seed=17, noise=0.7, outliers=0.4), (0.99, 8, 300, 4, 0.2, 5.991), 24, 7),
    "strict": (dict(n=40, seed=18, noise=1.5, outliers=0.5), (0.99, 12, 300, 4, 0.3, 5.991), 24, 8),
    "refail": (dict(n=24, seed=133, noise=0.3, outliers=0.6), (0.99, 5, 300, 4, 0.2, 5.991), 16, 134),
    "small": (dict(n=3, seed=19), (0.99, 10, 300, 4, 0.5, 5.991), 0, 9),
    "degenerate_planar": (dict(n=20, seed=20, noise=0.3, outliers=0.1, planar=True),
                          (0.99, 6, 300, 4, 0.3, 5.991), 5, 10),
    "degenerate_duplicate": (dict(n=12, seed=21, noise=0.3, outliers=0.0, duplicate=True),
                             (0.99, 5, 300, 4, 0.3, 5.991), 4, 11),
    "workload": (dict(n=100, seed=22, noise=0.5, outliers=0.2), RELOC, 24, 12),
}


def case(name):
    """-> (Scene, params, draws)"""
    args, params, n_hyp, dseed = CASES[name]
    sc = Scene(**args)
    d = draws(sc.n, n_hyp, dseed) if sc.n >= 4 else np.zeros((0, 4), np.int32)
    if name == "degenerate_duplicate" and len(d):
        d[0] = (0, 0, 0, 0)   # picks 0, n-1, n-2, n-3
        d[1] = (0, 1, 5, 2)   # picks both copies of the duplicated point
    if name == "h24" and len(d):
        d[2] = (3, 3, 3, 3)   # colliding draws: the swapped-in values are picked
        d[3] = (sc.n - 1, sc.n - 2, sc.n - 3, sc.n - 4)
    return sc, params, d
