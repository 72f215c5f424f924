"""Pins tests/sim3_ref.py, the plain-Python restatement of the reference's Sim3Solver that the GPU
tests compare against: hand-worked sample selection, the truncated error threshold, the
iteration-count formula, the acceptance rules, and ComputeSim3 against a float64 Horn solution."""
import math

import numpy as np
import pytest

import sim3_ref as R
from sim3_scenes import COLLISION_DRAWS, K_KITTI, Scene, draws, quirk_inputs, rotation


# ---- swap-remove selection ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLLISION_DRAWS))
def test_swap_remove_collisions(name):
    d, want = COLLISION_DRAWS[name]
    assert R.select3(6, d) == want


def test_swap_remove_hand_worked():
    # [0..5]: take slot 2 (-> 2), slot 2 now holds 5; take slot 2 again (-> 5), it now holds 4
    assert R.select3(6, [2, 2, 2]) == [2, 5, 4]
    # r0 == N-1 removes the last element without moving anything
    assert R.select3(4, [3, 2, 1]) == [3, 2, 1]
    # N == 3: the only list, any admissible draws give a permutation
    assert sorted(R.select3(3, [0, 0, 0])) == [0, 1, 2] and R.select3(3, [0, 0, 0]) == [0, 2, 1]
    with pytest.raises(AssertionError):
        R.select3(6, [0, 5, 0])  # the second draw's range is 0..4


# ---- threshold truncation ---------------------------------------------------------------------
def test_threshold_is_truncated():
    assert R.max_error(np.float32(1.44)) == 13  # 9.210 * 1.44 = 13.26
    assert R.max_error(np.float32(1.0)) == 9
    for err_sq, inlier in ((13.1, False), (12.9, True)):
        x1, x2, sig, k, eye = quirk_inputs(err_sq)
        s = R.Sim3Solver(x1, x2, sig, sig, k, k, True)
        u, v = R.project(s.X2, eye, k)
        e1 = R.sq_err(s.p1im1[0], s.p1im1[1], u, v)
        assert abs(float(e1[0]) - err_sq) < 0.05 and 13.0 < 13.1 < 9.210 * 1.44
        inl = s.check_inliers(eye, eye)
        assert bool(inl[0]) is inlier and inl[1] and inl[2]


# ---- SetRansacParameters -------------------------------------------------------------------------
def test_iteration_count_formula():
    # minInliers == N: one iteration
    assert R.ransac_max_its(20, 20, 300, 0.99) == 1
    # epsilon = 0.5f: ceil(log(0.01) / log(1 - 0.125)) = ceil(34.49) = 35
    assert R.ransac_max_its(12, 6, 300, 0.99) == 35
    assert R.ransac_max_its(12, 6, 20, 0.99) == 20
    # epsilon = (float)6 / 100: log(0.01) / log(1 - 0.06f^3) = 21318.2..., capped by maxIterations
    eps = float(np.float32(6) / np.float32(100))
    want = math.ceil(math.log(1 - 0.99) / math.log(1 - eps ** 3))
    assert want > 300 and R.ransac_max_its(100, 6, 300, 0.99) == 300
    assert R.ransac_max_its(100, 6, 10 ** 6, 0.99) == want
    # the float epsilon matters: 20 / 30 in float is not 2/3 in double
    eps = float(np.float32(20) / np.float32(30))
    assert R.ransac_max_its(30, 20, 300, 0.99) == math.ceil(math.log(0.01) / math.log(1 - eps ** 3))
    # never below 1; a quotient outside int converts to INT_MIN (x86) and ends as 1
    assert R.ransac_max_its(10, 9, 0, 0.99) == 1
    assert R.ransac_max_its(10, 0, 300, 0.99) == 1
    assert R.ransac_max_its(10, 6, 300, 1.0) == 1


# ---- acceptance -----------------------------------------------------------------------------------
def test_acceptance_rules():
    n, mi = 50, 20
    # a tie takes the later hypothesis; count == minInliers is not accepted
    counts = [5, 12, 12, 20, 3]
    assert R.find_counts(counts, n, mi, 5) == (-1, 0, 3, 20, True)
    assert R.find_counts([5, 12, 12, 3, 3], n, mi, 5) == (-1, 0, 2, 12, True)
    # the first count > minInliers returns, later (better) ones are never looked at
    assert R.find_counts([5, 21, 40], n, mi, 5) == (1, 21, 1, 21, False)
    # fewer draws than mRansacMaxIts and no acceptance: not bNoMore
    assert R.find_counts([5, 6], n, mi, 5) == (-1, 0, 1, 6, False)
    # N < minInliers: bNoMore, nothing else
    assert R.find_counts([], 10, 20, 5) == (-1, 0, -1, 0, True)
    assert R.iterate_counts([30], 10, 20, 5, 5, [0, 0, -1]) == (-1, True, 0)
    # zero counts still replace the best (0 >= 0): the last of them stays
    assert R.find_counts([0, 0, 0], n, mi, 3) == (-1, 0, 2, 0, True)


def test_iterate_5_repeated_equals_find():
    rng = np.random.default_rng(5)
    for trial in range(40):
        max_its = int(rng.integers(1, 40))
        counts = rng.integers(0, 24, max_its).tolist()
        want = R.find_counts(counts, 50, 20, max_its)
        state = [0, 0, -1]
        for step in range(100):
            acc, no_more, n_in = R.iterate_counts(counts, 50, 20, max_its, 5, state)
            if acc >= 0 or no_more:
                break
        assert (acc, n_in, state[2], state[1], no_more) == want
        assert state[0] <= max_its and step <= max_its // 5 + 1


# ---- ComputeSim3 against float64 Horn -------------------------------------------------------------
def horn64(P1, P2, fix_scale):
    """Horn 1987 in float64 with numpy's symmetric eigensolver: -> (R, s, t, N, q)."""
    P1 = np.asarray(P1, np.float64)
    P2 = np.asarray(P2, np.float64)
    O1, O2 = P1.mean(axis=1), P2.mean(axis=1)
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, -1]
    ang = math.atan2(np.linalg.norm(q[1:]), q[0])
    axis = q[1:] / np.linalg.norm(q[1:])
    Rm = rotation(axis, 2 * ang)
    P3 = Rm @ Pr2
    s = 1.0 if fix_scale else float((Pr1 * P3).sum() / (P3 * P3).sum())
    return Rm, s, O1 - s * Rm @ O2, N, q


HORN_P2 = np.array([[1.0, -2.0, 0.5], [0.25, 1.5, -1.0], [6.0, 8.0, 10.0]])  # one point per column
HORN_R = rotation([0.3, -0.5, 0.8], 0.7)
HORN_S, HORN_T = 1.25, np.array([0.5, -0.25, 0.75])
# Measured on this fixture (float32 restatement against horn64, the larger of fix_scale 0 / 1):
# max |R - R64| = 9.62e-8, |s - s64| = 7.98e-10, max |t - t64| = 9.49e-7. The bounds are 10x those.
HORN_TOL_R, HORN_TOL_S, HORN_TOL_T = 9.62e-7, 7.98e-9, 9.49e-6


@pytest.mark.parametrize("fix_scale", [False, True])
def test_compute_sim3_against_float64_horn(fix_scale):
    s_true = 1.0 if fix_scale else HORN_S
    P1 = (s_true * HORN_R @ HORN_P2 + HORN_T[:, None]).astype(np.float32)
    P2 = HORN_P2.astype(np.float32)
    h = R.compute_sim3(P1, P2, fix_scale)
    R64, s64, t64, N64, q64 = horn64(P1, P2, fix_scale)
    eR = float(np.abs(h["R"] - R64).max())
    eS = abs(float(h["s"]) - s64)
    eT = float(np.abs(h["t"] - t64).max())
    print(f"fix_scale={fix_scale}: |R-R64|={eR:.3g} |s-s64|={eS:.3g} |t-t64|={eT:.3g} "
          f"rotations={h['rotations']}")
    # N q = lambda q for the restatement's own N, eigenvalue and eigenvector (float32 Jacobi)
    N = h["N"].astype(np.float64)
    q = h["q"].astype(np.float64)
    lam = float(h["eval"][0])
    assert np.abs(N @ q - lam * q).max() <= 8 * np.finfo(np.float32).eps * np.abs(N).max()
    assert abs(np.linalg.norm(q) - 1) < 1e-6
    assert np.all(np.diff(h["eval"]) <= 0)  # descending
    # R orthonormal, a proper rotation
    Rm = h["R"].astype(np.float64)
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-6 and np.linalg.det(Rm) > 0.999
    assert eR <= HORN_TOL_R and eS <= HORN_TOL_S and eT <= HORN_TOL_T
    # and the solution is the true one (noise-free fixture)
    assert np.abs(Rm - HORN_R).max() < 1e-5 and abs(float(h["s"]) - s_true) < 1e-5
    # T12 / T21 are consistent: T21 * T12 = identity
    T12 = np.vstack([h["T12"], [0, 0, 0, 1]]).astype(np.float64)
    T21 = np.vstack([h["T21"], [0, 0, 0, 1]]).astype(np.float64)
    assert np.abs(T21 @ T12 - np.eye(4)).max() < 1e-5


def test_degenerate_triples_terminate():
    base = np.array([[1.0, -2.0, 0.5], [0.25, 1.5, -1.0], [6.0, 8.0, 10.0]], np.float32)
    coincident = base.copy()
    coincident[:, 1] = coincident[:, 0]
    collinear = base.copy()
    collinear[:, 2] = 2 * collinear[:, 1] - collinear[:, 0]
    nan = base.copy()
    nan[0, 0] = np.nan
    for P in (coincident, collinear, nan, np.zeros((3, 3), np.float32)):
        h = R.compute_sim3(P, P, False)
        assert h["rotations"] <= 4 * 4 * 30
    # identical sets: the quaternion's imaginary part is 0, 2*ang/norm is 0/0 and the reference's
    # hypothesis is NaN (kept)
    h = R.compute_sim3(base, base, True)
    if float(np.abs(h["q"][1:]).max()) == 0.0:
        assert np.isnan(h["R"]).all()


def test_restatement_end_to_end_recovers_the_loop():
    sc = Scene(60, seed=3, scale=1.1, outlier_frac=0.3)
    s = R.Sim3Solver(sc.x1, sc.x2, sc.sigma2_1, sc.sigma2_2, sc.k1, sc.k2, False)
    s.set_ransac_parameters(0.99, 20, 300)
    hyp = s.evaluate(draws(sc.n, 300, seed=4))
    acc, n_in, best, best_in, no_more = R.find_counts(s.counts(), s.N, s.min_inliers, s.max_its)
    assert acc >= 0 and n_in > 20
    inl = hyp[acc]["inliers"]
    assert not np.any(inl & ~sc.consistent)
    assert abs(float(hyp[acc]["s"]) - 1.1) < 0.05
    assert K_KITTI.dtype == np.float32
