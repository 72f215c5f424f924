"""Seeded two-view scenes for the Initializer tests: points in front of a first camera, a second
camera at a known pose, both projections through a small-sensor K with pixel noise, a share of gross
outliers among the matches and keypoints that no match uses. Small on purpose: the scalar
restatement (tests/initializer_ref.py) runs every case in a few seconds."""
import functools

import numpy as np

CAM_K = (458.654, 457.296, 367.215, 248.375)  # fx, fy, cx, cy


def rotation(axis, angle):
    axis = np.asarray(axis, float)
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


class Scene:
    """N matches among n1 = N + extra1 and n2 = N + extra2 keypoints. kind: "general" (a depth range),
    "planar" (one slanted plane), "collinear" (one 3-D line). keys2 is shuffled so that matches12
    is not the identity."""

    def __init__(self, N, seed, kind="general", t=(0.4, 0.05, 0.1), angle=0.08, noise=0.3, outliers=0.0,
                 extra1=5, extra2=7, duplicate=0, k=CAM_K, sigma=1.0, depth=(3.0, 9.0), tilt=0.6):
        rng = np.random.default_rng(seed)
        fx, fy, cx, cy = CAM_K
        self.R = rotation(rng.normal(size=3), angle) if angle else np.eye(3)
        self.t = np.asarray(t, float)
        u = rng.uniform(40, 700, N)
        v = rng.uniform(40, 440, N)
        if kind == "collinear":
            v = 100 + 0.5 * u
        z = rng.uniform(depth[0], depth[1], N)
        if kind in ("planar", "collinear"):  # the plane Z = 5 + tilt * X + 0.2 * tilt * Y
            z = 5.0 / (1.0 - tilt * (u - cx) / fx - 0.2 * tilt * (v - cy) / fy)
        if kind == "same":
            u, v = np.full(N, 300.0), np.full(N, 200.0)
        X1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
        X2 = X1 @ self.R.T + self.t
        p1 = np.stack([u, v], 1)
        p2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
        if noise > 0:
            p1 = p1 + rng.normal(0, noise, p1.shape)
            p2 = p2 + rng.normal(0, noise, p2.shape)
        bad = rng.random(N) < outliers
        p2[bad] += rng.uniform(-120, 120, (int(bad.sum()), 2))
        for d in range(duplicate):  # pairs of identical matches: point 2d+1 repeats point 2d
            p1[2 * d + 1], p2[2 * d + 1] = p1[2 * d], p2[2 * d]
        self.outlier = bad
        self.X1 = X1
        n1, n2 = N + extra1, N + extra2
        slot1 = np.sort(rng.permutation(n1)[:N])
        slot2 = rng.permutation(n2)[:N]
        keys1 = np.stack([rng.uniform(0, 752, n1), rng.uniform(0, 480, n1)], 1)
        keys2 = np.stack([rng.uniform(0, 752, n2), rng.uniform(0, 480, n2)], 1)
        keys1[slot1] = p1
        keys2[slot2] = p2
        self.keys1 = np.ascontiguousarray(keys1, np.float32)
        self.keys2 = np.ascontiguousarray(keys2, np.float32)
        self.matches12 = np.full(n1, -1, np.int32)
        self.matches12[slot1] = slot2
        self.N, self.n1, self.n2 = N, n1, n2
        self.k = np.array(k, np.float32)
        self.sigma = float(sigma)


def draws(N, n_hyp, seed):
    """RandomInt(0, size - 1) of the eight picks of n_hyp iterations: (n_hyp, 8) int32."""
    if N < 8:
        return np.zeros((n_hyp, 8), np.int32)
    rng = np.random.default_rng(seed)
    hi = np.array([N - j for j in range(8)], np.int64)
    return rng.integers(0, hi, (n_hyp, 8)).astype(np.int32)


# name -> (Scene arguments, hypotheses drawn, draw seed)
CASES = {
    "n8": (dict(N=8, seed=1, noise=0.0), 4, 101),
    "n9": (dict(N=9, seed=2, noise=0.1), 5, 102),
    "n63": (dict(N=63, seed=3, outliers=0.1), 4, 103),
    "n64": (dict(N=64, seed=4), 3, 104),
    "n65": (dict(N=65, seed=5, kind="planar"), 5, 105),
    "general": (dict(N=120, seed=6, noise=0.2), 12, 106),
    "planar": (dict(N=120, seed=7, kind="planar", noise=0.2, t=(0.5, 0.1, 0.0), tilt=0.9), 8, 107),
    "rotation": (dict(N=100, seed=8, t=(0, 0, 0), angle=0.1, noise=0.0), 6, 108),
    "rotation_noisy": (dict(N=100, seed=8, t=(0, 0, 0), angle=0.1, noise=0.01), 6, 108),
    "low_parallax": (dict(N=110, seed=30, t=(0.03, 0.005, 0.0), angle=0.05, noise=0.03, depth=(2.2, 4.5), sigma=0.3),
                     8, 130),
    "outliers": (dict(N=130, seed=9, outliers=0.3, noise=0.4), 16, 109),
    "few": (dict(N=40, seed=10, noise=0.2), 6, 110),
    "similar": (dict(N=120, seed=11, kind="planar", noise=0.2, t=(0.1, 0.02, 0.3), tilt=0.1), 8, 111),
    "unmatched": (dict(N=70, seed=12, extra1=60, extra2=45, noise=0.2), 6, 112),
    "n7": (dict(N=7, seed=13), 4, 113),
    "duplicated": (dict(N=12, seed=15, duplicate=6, noise=0.0), 4, 115),
    "collinear": (dict(N=30, seed=16, kind="collinear", noise=0.0), 4, 116),
    "same": (dict(N=10, seed=20, kind="same", noise=0.0), 3, 120),
    "sigma0": (dict(N=20, seed=21, sigma=0.0), 3, 121),
    "nan_calibration": (dict(N=70, seed=17, noise=0.2, k=(float("nan"), 457.296, 367.215, 248.375)), 4, 117),
    "workload": (dict(N=128, seed=18, outliers=0.15, noise=0.3, extra1=40, extra2=40), 16, 118),
}


@functools.lru_cache(None)
def case(name):
    """-> (Scene, draws)"""
    args, n_hyp, dseed = CASES[name]
    sc = Scene(**args)
    d = draws(sc.N, n_hyp, dseed)
    if name == "n9":
        d[0] = (0, 0, 0, 0, 0, 0, 0, 0)   # each removal brings the last element to slot 0
        d[1] = (8, 7, 6, 5, 4, 3, 2, 1)   # always the last element
    if name == "duplicated":
        d[0] = (0, 1, 2, 2, 2, 2, 2, 2)   # the first two picks are the two copies of one match
    return sc, d


@functools.lru_cache(None)
def reference(name):
    """The restatement's result of a case, computed once and shared by the tests."""
    import initializer_ref as I
    sc, d = case(name)
    return I.initialize(sc.keys1, sc.keys2, sc.matches12, sc.k, sc.sigma, d)


def bits32(x):
    return "%08x" % int(np.array([x], np.float32).view(np.uint32)[0])


def dump(path, problems):
    """Writes (keys1, keys2, matches12, k, sigma, draws) problems as the text the stand-alone host
    program tests/cpp/initializer_core_main.cpp reads: every real as the bits of a float."""
    lines = [str(len(problems))]
    for keys1, keys2, m12, k, sigma, d in problems:
        lines.append("%d %d %d %s %s" % (len(keys1), len(keys2), len(d), bits32(sigma), " ".join(bits32(v) for v in k)))
        for (x, y), m in zip(keys1, m12):
            lines.append("%s %s %d" % (bits32(x), bits32(y), int(m)))
        for x, y in keys2:
            lines.append("%s %s" % (bits32(x), bits32(y)))
        for row in d:
            lines.append(" ".join(str(int(v)) for v in row))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
