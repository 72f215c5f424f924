"""Named synthetic pose graphs for the OptimizeEssentialGraph tests, seeded: the smallest at which each
path can go wrong. A scene is the problem orbfe_essgraph_solve reads (tests/essgraph_ref.py solves the
same object): keyframes on a ring looking inwards, odometry drift accumulated along it, the loop keyframe
fixed, the current keyframe and its neighbours carrying a CorrectedSim3 (and their uncorrected pose in
NonCorrectedSim3), loop-connection edges (kind 0) from the corrected end to the loop end, spanning-tree
and covisibility edges (kind 1) along the band."""
import functools
from types import SimpleNamespace

import numpy as np


def rot(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def quat(R):
    """x y z w of a rotation matrix, w >= 0"""
    w = np.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1e-300)) / 2
    if w > 1e-6:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) / 2
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = t, (R[j, i] + R[i, j]) / (4 * t), (R[k, i] + R[i, k]) / (4 * t), (R[k, j] - R[j, k]) / (4 * t)
    return q / np.linalg.norm(q)


def sim3_row(R, t, s):
    return np.concatenate([quat(R), np.asarray(t, np.float64), [s]])


def ring_truth(n, radius=5.0):
    """world-to-camera (R, t) of n keyframes on a circle"""
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        Rwc = rot([0.0, a, 0.0])
        c = np.array([radius * np.sin(a), 0.1 * np.sin(3 * a), radius * np.cos(a)])
        out.append((Rwc.T, -Rwc.T @ c))
    return out


def graph(n, band=1, fixed=0, n_corr=2, loop_rows=1, fix_scale=True, seed=0, drift=(0.01, 0.02), corr_rot=0.0,
          corr_scale=1.0, extra_edges=(), orphan=False, n_points=0, points_on_fixed=False, per_vertex_corr=None):
    """The keyframes 0 .. n-1 ascending in mnId; the loop keyframe `fixed`; the last n_corr keyframes
    corrected: the truth turned by corr_rot and scaled by corr_scale, or per_vertex_corr's (rotation vector,
    scale) applied to the keyframe's own pose. orphan: one more keyframe without an edge."""
    rng = np.random.default_rng(seed)
    truth = ring_truth(n)
    # odometry: the relative motions with a small error each, chained from keyframe 0
    est = [truth[0]]
    for k in range(1, n):
        Rrel = truth[k][0] @ truth[k - 1][0].T
        trel = truth[k][1] - Rrel @ truth[k - 1][1]
        dR = rot(rng.normal(0, drift[0], 3))
        dt = rng.normal(0, drift[1], 3)
        Rk = dR @ Rrel @ est[k - 1][0]
        tk = dR @ (Rrel @ est[k - 1][1] + trel) + dt
        est.append((Rk, tk))
    nv = n + (1 if orphan else 0)
    tcw = np.zeros((nv, 12), np.float32)
    for k in range(n):
        tcw[k] = np.hstack([est[k][0], est[k][1].reshape(3, 1)]).reshape(-1)
    if orphan:
        tcw[n] = np.hstack([rot([0.1, 0.2, 0.3]), np.array([[1.0], [2.0], [3.0]])]).reshape(-1)
    corrected_idx, corrected, noncorrected = [], [], []
    for k in range(n - n_corr, n):
        Rf, tf = tcw[k].reshape(3, 4)[:, :3].astype(np.float64), tcw[k].reshape(3, 4)[:, 3].astype(np.float64)
        if per_vertex_corr is not None:
            w, sc = per_vertex_corr[k - (n - n_corr)]
            Rc, tc, s = rot(w) @ Rf, rot(w) @ tf * sc, sc
        else:
            w = rng.normal(0, 1, 3)
            w = w / np.linalg.norm(w) * corr_rot
            Rc, tc, s = rot(w) @ truth[k][0], truth[k][1] * corr_scale + rng.normal(0, 0.01, 3), corr_scale
        corrected_idx.append(k)
        corrected.append(sim3_row(Rc, tc, s))
        noncorrected.append(sim3_row(Rf, tf, 1.0))
    edges = []
    for r in range(loop_rows):  # LoopConnections: the corrected end sees the loop end
        edges.append((n - 1 - r, (fixed + r) % n if r == 0 else r, 0))
    for k in range(1, n):
        edges.append((k, k - 1, 1))  # the spanning tree
        for j in range(max(0, k - band), k - 1):
            edges.append((k, j, 1))  # covisibility, the later keyframe is vertex 0
    edges += list(extra_edges)
    xw, ref = np.zeros((n_points, 3), np.float32), np.zeros(n_points, np.int32)
    for i in range(n_points):
        ref[i] = fixed if (points_on_fixed and i % 5 == 0) else int(rng.integers(0, nv))
        R, t = tcw[ref[i]].reshape(3, 4)[:, :3].astype(np.float64), tcw[ref[i]].reshape(3, 4)[:, 3].astype(np.float64)
        xc = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 6)])
        xw[i] = R.T @ (xc - t)
    noncorrected_idx = list(corrected_idx)
    return SimpleNamespace(
        n_vertices=nv, tcw=tcw, fixed_vertex=fixed, fix_scale=1 if fix_scale else 0,
        n_corrected=len(corrected_idx), corrected_idx=np.array(corrected_idx, np.int32),
        corrected_sim3=np.array(corrected, np.float64).reshape(-1, 8),
        n_noncorrected=len(noncorrected_idx), noncorrected_idx=np.array(noncorrected_idx, np.int32),
        noncorrected_sim3=np.array(noncorrected, np.float64).reshape(-1, 8),
        n_edges=len(edges), edge_i=np.array([e[0] for e in edges], np.int32), edge_j=np.array([e[1] for e in edges], np.int32),
        edge_kind=np.array([e[2] for e in edges], np.uint8), n_points=n_points, xw=xw, point_ref=ref,
        truth=truth)


# A seed at which trials are rejected and a later trial of the same iteration is accepted: found by a
# search over seeds 0 .. 39 of this generator with tests/essgraph_ref.py (the first hit of three).
REJECTED_SEED = 14

def _nonfinite():
    """The corrected keyframe's translation is 1e160: finite, but the squares of the residuals of its two
    edges are not, so chi2 is +inf and H has non-finite entries from the third block row on. Every trial's
    factorisation passes two pivot blocks, fails at the third and is rejected."""
    p = graph(5, n_corr=1, seed=12, corr_rot=0.03)
    p.corrected_sim3 = p.corrected_sim3.copy()
    p.corrected_sim3[0, 4:7] = [1e160, -1e160, 1e160]
    return p


CASES = {
    # 2 vertices, 1 edge, one fixed: a 1-block system; one point
    "pair": lambda: graph(2, n_corr=1, seed=1, corr_rot=0.05, n_points=1),
    "chain3": lambda: graph(3, n_corr=1, seed=2, corr_rot=0.05, loop_rows=0),
    # a drifted ring with a loop-connection edge between free vertices (and one to the fixed one): one long
    # envelope row with fill; points130
    "ring12": lambda: graph(12, n_corr=2, loop_rows=2, seed=3, corr_rot=0.02, n_points=130, points_on_fixed=True),
    "fixed_mid": lambda: graph(9, fixed=4, n_corr=2, seed=4, corr_rot=0.02),
    "fix_scale": lambda: graph(12, n_corr=3, loop_rows=2, seed=5, corr_rot=0.02, corr_scale=1.15, fix_scale=True),
    "free_scale": lambda: graph(12, n_corr=3, loop_rows=2, seed=5, corr_rot=0.02, corr_scale=1.15, fix_scale=False),
    "orphan": lambda: graph(6, n_corr=1, seed=6, corr_rot=0.03, orphan=True, n_points=7),
    # the same pair as a kind-0 and a kind-1 edge
    "dup_edge": lambda: graph(6, n_corr=2, seed=7, corr_rot=0.03, extra_edges=[(5, 0, 1), (0, 5, 1)]),
    # the current keyframe's neighbours corrected, the rest not: kind-1 edges with both ends in the map
    "noncorrected": lambda: graph(10, band=3, n_corr=4, seed=8, corr_rot=0.03, corr_scale=0.9, fix_scale=False),
    # 80 vertices, band 6, two long loop rows: past a wavefront in every per-vertex and per-edge stage
    "ring80_band": lambda: graph(80, band=6, n_corr=3, loop_rows=3, seed=9, corr_rot=0.01, drift=(0.002, 0.004)),
    # the start residuals of the four kind-1 edges into the corrected tail land in log()'s four branches
    "log_branches": lambda: graph(7, n_corr=3, seed=10, fix_scale=False, loop_rows=0, drift=(0.0, 0.0),
                                  per_vertex_corr=[([0.0, 0.0, 0.0], 1.3), ([0.0, 0.3, 0.0], 1.0), ([0.2, 0.0, 0.1], 1.0)]),
    "rejected": lambda: graph(6, n_corr=2, seed=REJECTED_SEED, corr_rot=3.0, corr_scale=0.3, fix_scale=False),
    "nonfinite": _nonfinite,
}

GPU_CASES = list(CASES)


@functools.lru_cache(None)
def case(name):
    return CASES[name]()


def recovery_scene(n=12):
    """Noise-free: every uncorrected pose and every NonCorrectedSim3 is the truth, so every kind-1
    measurement (the loop edge included) is an exact relative motion; the tail's CorrectedSim3 is a
    planted wrong pose. The optimum is the ring itself, chi2 = 0."""
    return graph(n, n_corr=2, seed=11, drift=(0.0, 0.0), corr_rot=0.05, loop_rows=0, extra_edges=[(n - 1, 0, 1)])
