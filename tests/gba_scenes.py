"""Synthetic maps for the global BundleAdjustment tests, each named for the branch it takes
(test_gba_ref.py asserts from the restatement that it does): the smallest shapes at which the plan, the
sparse Schur complement and the envelope factorisation can go wrong. Keyframe 0 is the mnId-0 keyframe
(fixed) unless a scene says otherwise; keyframes stand in a row as in lba_scenes and each point of a
chain is seen by `obs` consecutive ones. Every array is float32 / int32 as the C ABI takes it."""
import functools

import numpy as np

from lba_scenes import add_point, edit, finish, project, rot


def chain(seed, nk, per_link, obs=3, mode="mixed", noise=0.3, perturb=True, fix0=True, loop_points=0, outlier_frac=0.0,
          n_iterations=10, robust=1, stop_at_poll=-1):
    """nk keyframes; link i (0 .. nk - obs) has per_link points seen by keyframes i .. i + obs - 1; then
    loop_points points seen by keyframe 1 and the last one (the first and the last free keyframe)"""
    rng = np.random.default_rng(seed)
    true_T = np.zeros((nk, 3, 4))
    step = min(0.3, 4.0 / nk)
    for i in range(nk):
        R = rot(*(rng.uniform(-0.05, 0.05, 3)))
        c = np.array([step * i - 0.5 * step * nk, rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3)])
        true_T[i, :, :3], true_T[i, :, 3] = R, -R @ c
    fixed = np.zeros(nk, np.uint8)
    fixed[0] = 1 if fix0 else 0
    seen_by = [list(range(i, min(i + obs, nk))) for i in range(max(nk - obs + 1, 1)) for _ in range(per_link)]
    seen_by += [[1, nk - 1]] * loop_points
    true_X = np.zeros((len(seen_by), 3))
    for p, seen in enumerate(seen_by):  # inside its observers' images, the right-image coordinate included
        for _ in range(1000):
            X = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 12)])
            uv = np.array([project(true_T[kf], X)[0] for kf in seen])
            if (uv > 5).all() and (uv[:, [0, 2]] < 635).all() and (uv[:, 1] < 475).all():
                break
        true_X[p] = X
    tcw0 = true_T.copy()
    if perturb:
        for i in range(nk):
            if fixed[i]:
                continue
            dR = rot(*(rng.uniform(-0.004, 0.004, 3)))
            tcw0[i, :, :3] = dR @ true_T[i, :, :3]
            tcw0[i, :, 3] = dR @ true_T[i, :, 3] + rng.uniform(-0.01, 0.01, 3)
    xw0 = true_X + (rng.uniform(-0.03, 0.03, true_X.shape) if perturb else 0.0)
    edge_begin, e_kf, kp, ur, is2, planted = [0], [], [], [], [], []
    for p, seen in enumerate(seen_by):
        moved = int(rng.choice(seen)) if rng.random() < outlier_frac * len(seen) else -1
        for kf in seen:
            u, _ = project(true_T[kf], true_X[p])
            u = u + rng.normal(0, noise, 3) if noise else u
            stereo = mode == "stereo" or (mode == "mixed" and rng.random() < 0.5)
            bad = kf == moved
            if bad:
                ang, d = rng.uniform(0, 2 * np.pi), rng.uniform(50, 90)
                u = u + np.array([d * np.cos(ang), d * np.sin(ang), d * np.cos(ang)])
            e_kf.append(kf), kp.append(u[:2]), ur.append(u[2] if stereo else -1.0)
            is2.append(1.0 / 1.2 ** (2 * int(rng.integers(0, 4)))), planted.append(bad)
        edge_begin.append(len(e_kf))
    q = finish(true_T, true_X, tcw0, xw0, fixed, edge_begin, e_kf, kp, ur, is2, planted, stop_at_poll)
    return edit(q, n_iterations=n_iterations, robust=robust)


def add_keyframe(p, T, fixed):
    """a copy of p with one more keyframe (3x4 pose T, true and initial) that observes nothing yet"""
    row = np.asarray(T, float).reshape(1, 12)
    return edit(p, n_kf=p.n_kf + 1, tcw=np.vstack([p.tcw, row.astype(np.float32)]), true_tcw=np.vstack([p.true_tcw, row]),
                k=np.vstack([p.k, p.k[:1]]), bf=np.append(p.bf, p.bf[0]).astype(np.float32),
                fixed=np.append(p.fixed, np.uint8(1 if fixed else 0)).astype(np.uint8))


def _orphan_kf():
    p = chain(15, 5, 4)
    T = p.true_tcw[2].reshape(3, 4).copy()
    T[:, 3] += [0.05, -0.02, 0.03]
    return add_keyframe(p, T, False)


def _nonfinite():
    # a fixed camera at z = 6 with identity rotation; the last point has z = 0 in it
    p = add_keyframe(chain(17, 4, 5), np.hstack([np.eye(3), [[0.0], [0.0], [-6.0]]]), True)
    X = np.array([0.25, 0.5, 6.0])
    T = p.true_tcw.reshape(-1, 3, 4)
    return add_point(p, X, X, [1, 2, 4], obs_px=[tuple(project(T[1], X)[0][:2]), tuple(project(T[2], X)[0][:2]), (300.0, 200.0)])


BUILDERS = {
    "pair_mono": lambda: chain(11, 2, 30, obs=2, mode="mono", n_iterations=20),
    "chain": lambda: chain(12, 12, 4),
    "loop": lambda: chain(12, 12, 4, loop_points=3),
    "past_lba": lambda: chain(13, 131, 2, n_iterations=3),
    "not_robust": lambda: chain(14, 6, 8, outlier_frac=0.10, robust=0),
    "mixed": lambda: chain(16, 5, 24),
    "no_fixed": lambda: chain(18, 4, 6, mode="stereo", fix0=False),
    "orphan_kf": _orphan_kf,
    "orphan_point": lambda: add_point(chain(19, 5, 4), [0.1, -0.2, 9.0], [0.11, -0.2, 9.02], []),
    "fixed_only_point": lambda: add_point(chain(20, 5, 4), [-0.4, 0.3, 6.0], [-0.42, 0.31, 6.05], [0], mono=False),
    "nonfinite": _nonfinite,
    "stop0": lambda: chain(21, 4, 5, stop_at_poll=0),
    "stop_mid": lambda: chain(21, 4, 5, stop_at_poll=2),
    "empty": lambda: edit(chain(22, 3, 4), fixed=np.ones(3, np.uint8)),
}
CASES = list(BUILDERS)
CLEAN_SEEDS = (31, 32, 33)


@functools.lru_cache(None)
def case(name):
    return BUILDERS[name]()


def clean_scene(seed):
    return chain(seed, 6, 8, mode="stereo", noise=0.0)


def lba_like_scene():
    """within LocalBundleAdjustment's caps, every keyframe but the mnId-0 one free: both solvers' first
    linearisation can be compared"""
    return chain(23, 7, 5, loop_points=2)
