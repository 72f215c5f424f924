"""Synthetic correspondence sets for the Sim3Solver tests (tests/test_sim3_ref.py on the CPU,
tests/test_gpu_sim3.py on the GPU). Plain numpy; shares no code with the product."""
import numpy as np

K_KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
K_OTHER = np.array([520.9, 521.0, 325.1, 249.7], np.float32)


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    x, y, z = axis
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


class Scene:
    """n correspondences X1 = s*R*X2 + t (+ noise); `outliers` of them scrambled."""

    def __init__(self, n, seed, scale=1.0, noise=0.002, outlier_frac=0.0, k1=K_KITTI, k2=K_KITTI):
        rng = np.random.default_rng(seed)
        self.R = rotation(rng.normal(size=3), rng.uniform(0.1, 0.6))
        self.s = float(scale)
        self.t = rng.uniform(-0.5, 0.5, 3)
        X2 = np.stack([rng.uniform(-4, 4, n), rng.uniform(-1.5, 1.5, n), rng.uniform(5, 14, n)], axis=1)
        X1 = self.s * X2 @ self.R.T + self.t + rng.normal(0, noise, (n, 3))
        self.consistent = np.ones(n, bool)
        n_out = int(round(outlier_frac * n))
        if n_out:
            out = rng.choice(n, n_out, replace=False)
            self.consistent[out] = False
            X1[out] = np.stack([rng.uniform(-4, 4, n_out), rng.uniform(-1.5, 1.5, n_out),
                                rng.uniform(5, 14, n_out)], axis=1)
        self.x1 = X1.astype(np.float32)
        self.x2 = X2.astype(np.float32)
        octave1 = rng.integers(0, 8, n)
        octave2 = rng.integers(0, 8, n)
        sigma2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2
        self.sigma2_1 = sigma2[octave1].astype(np.float32)
        self.sigma2_2 = sigma2[octave2].astype(np.float32)
        self.k1 = np.asarray(k1, np.float32)
        self.k2 = np.asarray(k2, np.float32)
        self.n = n


def draws(n, n_hyp, seed):
    """n_hyp iterations of raw RandomInt(0, size - 1) values: draw i in 0 .. n-1-i."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.array([n, n - 1, n - 2]), (n_hyp, 3)).astype(np.int32)


# The three swap-remove collisions, for N = 6 (hand-worked in tests/test_sim3_ref.py):
#   r1 == r0: the second draw lands on the slot that now holds the former last element
#   r0 == N-1: the first draw takes the last element itself
#   r2 on a moved slot: the third draw lands on the slot the second removal refilled
COLLISION_DRAWS = {
    "r1_eq_r0": ([2, 2, 0], [2, 5, 0]),
    "r0_is_last": ([5, 4, 0], [5, 4, 0]),
    "r2_on_moved": ([1, 3, 3], [1, 3, 4]),
    "r1_r2_chain": ([0, 0, 0], [0, 5, 4]),
}


def quirk_inputs(err_sq):
    """One correspondence whose reprojection error under the identity Sim3 is about err_sq in both
    images (fx = fy = 100, z = 1), padded with two exact correspondences; sigma2 = 1.44 gives the
    threshold 9.210 * 1.44 = 13.26, truncated to 13."""
    k = np.array([100.0, 100.0, 50.0, 50.0], np.float32)
    d = np.sqrt(err_sq) / 100.0
    x2 = np.array([[0.1, 0.2, 1.0], [0.3, -0.1, 1.0], [-0.2, 0.1, 1.0]], np.float32)
    x1 = x2.copy()
    x1[0, 0] += np.float32(d)
    sig = np.full(3, 1.44, np.float32)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    return x1, x2, sig, k, eye
