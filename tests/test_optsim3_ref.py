"""tests/optsim3_ref.py pinned on its own (no GPU): hand-worked Sim3 values, the numeric Jacobians against
the analytic ones, exp against libm, the 7x7 LDLT against numpy, recovery of the truth, planted outliers,
the branch each named scene takes, the stale-error rule, and the core header built for the host under
sanitizers against the restatement bit for bit."""
import functools
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import optsim3_ref as O
from optsim3_scenes import CASES, CLEAN_SEEDS, OUTLIER_SEEDS, case, clean_scene, outlier_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured with this file (printed by the tests); the assertions allow 4x for other seeds.
MEASURED_EXP_ULP = 1.000         # worst |exp - math.exp| in ulp over the grid of test_exp_within_two_ulp
MEASURED_JACOBIAN_GAP = 1.23e-07  # worst |J_numeric - J_analytic| / max |J_analytic| of an edge
MEASURED_ROT, MEASURED_TRANS, MEASURED_SCALE = 5.03e-06, 2.36e-04, 7.9e-05  # noise-free recovery, float32 inputs

IDENTITY = ([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], 1.0)


@functools.lru_cache(None)
def ref(name):
    return O.optimize(case(name))


# ---- Sim3 by hand ----------------------------------------------------------------------------------
def test_sim3_update_small_theta_small_sigma():
    (q, t, s), flags = O.sim3_from_update([0.0, 0.0, 0.0, 1.5, -2.0, 0.25, 0.0])
    assert (q, t, s, flags) == ([0.0, 0.0, 0.0, 1.0], [1.5, -2.0, 0.25], 1.0, 0)
    # R = I + Omega + Omega^2 with omega = (0, 0, 2^-20); W = 0.5 Omega + Omega^2 / 6 + I
    w = 2.0 ** -20
    (q, t, s), _ = O.sim3_from_update([0.0, 0.0, w, 1.0, 0.0, 0.0, 0.0])
    R = [1.0 - w * w, -w, 0.0, w, 1.0 - w * w, 0.0, 0.0, 0.0, 1.0]
    assert q == O.quat_from_matrix(R) and s == 1.0
    assert t == [0.5 * 0.0 + (1.0 / 6.0) * (-(w * w)) + 1.0, 0.5 * w, 0.0]
    assert abs(((q[0] ** 2 + q[1] ** 2) + q[2] ** 2) + q[3] ** 2 - 1.0) < 1e-11  # not normalised, only close


def test_sim3_update_small_theta_large_sigma():
    sigma = 0.5
    (q, t, s), _ = O.sim3_from_update([0.0, 0.0, 0.0, 2.0, 0.0, -4.0, sigma])
    assert q == [0.0, 0.0, 0.0, 1.0] and s == O.exp(0.5)
    C = (s - 1) / sigma
    assert t == [C * 2.0, 0.0, C * -4.0]


def test_sim3_update_large_theta_both_sigma_branches():
    th = 0.5
    sn, cs, _ = O.sincos(th)
    (q, t, s), flags = O.sim3_from_update([0.0, 0.0, th, 0.0, 0.0, 3.0, 0.0])
    assert flags == 0 and s == 1.0 and t == [0.0, 0.0, 3.0]  # W e_z = C e_z
    assert abs(q[2] - math.sin(0.25)) < 1e-15 and abs(q[3] - math.cos(0.25)) < 1e-15
    (q2, t2, s2), _ = O.sim3_from_update([0.0, 0.0, th, 1.0, 0.0, 0.0, 0.25])
    assert q2 == q and s2 == O.exp(0.25)
    a, b, c = s2 * sn, s2 * cs, th * th + 0.25 * 0.25
    A = (a * 0.25 + (1 - b) * th) / (th * c)
    C = (s2 - 1) / 0.25
    B = (C - ((b - 1) * 0.25 + a * th) / c) * 1. / (th * th)
    assert t2 == [(A * 0.0 + B * -(th * th)) + C, (A * th + B * 0.0) + 0.0, 0.0]
    assert O.sim3_from_update([0.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0])[1] == O.FLAG_LARGE_STEP


def test_inverse_map_and_product_on_exact_values():
    S = ([0.0, 0.0, 1.0, 0.0], [1.0, 2.0, 4.0], 2.0)  # half a turn about z, scale 2
    assert O.sim3_map(S, [1.0, 0.5, 3.0]) == [-1.0, 1.0, 10.0]
    Si = O.sim3_inverse(S)
    assert Si == ([-0.0, -0.0, -1.0, 0.0], [0.5, 1.0, -2.0], 0.5)
    assert O.sim3_map(Si, [-1.0, 1.0, 10.0]) == [1.0, 0.5, 3.0]
    T = ([0.0, 0.0, 0.0, 1.0], [0.25, 0.0, -1.0], 4.0)
    assert O.sim3_mul(S, T) == ([0.0, 0.0, 1.0, 0.0], [0.5, 2.0, 2.0], 8.0)
    assert O.sim3_mul(IDENTITY, S) == S


def test_oplus_zeroes_the_scale_increment_in_place():
    u = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.3]
    S, _ = O.oplus(u, True, IDENTITY)
    assert u[6] == 0.0 and S[2] == 1.0
    u = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.3]
    S, _ = O.oplus(u, False, IDENTITY)
    assert u[6] == 0.3 and S[2] == O.exp(0.3)


# ---- exp -------------------------------------------------------------------------------------------
def ulps(got, want):
    return abs(got - want) / math.ulp(want)


def exp_grid():
    xs = [float(x) for x in np.linspace(-1.0, 1.0, 100001)]
    for start in (0.0, 1e-9, -1e-9):
        for toward in (math.inf, -math.inf):
            x = start
            for _ in range(1000):
                x = math.nextafter(x, toward)
                xs.append(x)
    return xs


def test_exp_within_two_ulp():
    """the project's condition for restated libm functions: at most 2 ulp against libm, over 100,001
    equally spaced points of [-1, 1] and the 1,000 doubles above and below 0, 1e-9 and -1e-9"""
    worst = max(ulps(O.exp(x), math.exp(x)) for x in exp_grid())
    print("exp: worst deviation from libm %.3f ulp" % worst)
    assert worst <= 2.0
    assert worst <= MEASURED_EXP_ULP * 1.01
    assert O.exp(0.0) == 1.0 and O.exp(-0.0) == 1.0


def test_exp_outside_the_stated_range():
    for x in (-700.0, -30.0, -5.0, 3.0, 20.0, 700.0, 709.7, -744.0):
        assert abs(O.exp(x) - math.exp(x)) <= 4 * math.ulp(math.exp(x)) or math.exp(x) < 1e-300, x
    assert O.exp(710.0) == math.inf and O.exp(-746.0) == 0.0 and O.exp(math.inf) == math.inf and O.exp(-math.inf) == 0.0
    assert O.exp(math.nan) != O.exp(math.nan)


# ---- the numeric Jacobians -------------------------------------------------------------------------
def analytic_jacobian(e, S):
    """d error / d update for the left increment exp(u) * S (the formulas of the commented-out
    linearizeOplus, derived by hand): e12: -dproj(p) [-[p]x | I | p], p = S.map(X);
    e21: +dproj(p') (1 / s) R^T [-[X]x | I | X], p' = S^-1.map(X)"""
    R = np.array(O.quat_to_matrix(S[0])).reshape(3, 3)
    X = np.array(e.X)

    def skew(v):
        return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])

    if e.inverse:
        p = np.array(O.sim3_map(O.sim3_inverse(S), e.X))
        dp = -(1.0 / S[2]) * R.T @ np.hstack([-skew(X), np.eye(3), X[:, None]])
    else:
        p = np.array(O.sim3_map(S, e.X))
        dp = np.hstack([-skew(p), np.eye(3), p[:, None]])
    fx, fy = e.cam[0], e.cam[1]
    dproj = np.array([[fx / p[2], 0, -fx * p[0] / p[2] ** 2], [0, fy / p[2], -fy * p[1] / p[2] ** 2]])
    return -dproj @ dp


def test_numeric_jacobian_against_the_analytic_one():
    worst = 0.0
    for name, fix in (("n64", False), ("free_scale", False), ("two_cameras", False), ("fix_scale", True)):
        p = case(name)
        S = O.sim3_from_floats(p.r12, p.t12, float(p.s12))
        tab = O.build_table(S, fix)
        for i in np.flatnonzero(p.valid)[:12]:
            for e in (O.Edge(p.p3d2c[i], p.kp_un1[i], p.inv_sigma2_1[i], p.k1, False),
                      O.Edge(p.p3d1c[i], p.kp_un2[i], p.inv_sigma2_2[i], p.k2, True)):
                Jn = np.array(O.numeric_jacobian(e, tab))
                Ja = analytic_jacobian(e, S)
                if fix:
                    assert (Jn[:, 6] == 0.0).all() and not np.signbit(Jn[:, 6]).any()  # column 6 is exactly +0
                    Ja[:, 6] = 0.0
                worst = max(worst, float(np.max(np.abs(Jn - Ja)) / np.max(np.abs(Ja))))
    print("numeric vs analytic Jacobian: worst relative gap %.3g" % worst)
    assert worst <= 4 * MEASURED_JACOBIAN_GAP


def test_fix_scale_gives_h66_equal_to_lambda():
    seen = []
    O.optimize(case("fix_scale"), hook=lambda it, i, S, lam: seen.append((S[O.H_IDX[6][6]], S[34], [S[O.H_IDX[6][c]] for c in range(6)])))
    assert seen and all(h66 == 0.0 and b6 == 0.0 and row == [0.0] * 6 for h66, b6, row in seen)
    seen = []
    O.optimize(case("free_scale"), hook=lambda it, i, S, lam: seen.append(S[O.H_IDX[6][6]]))
    assert all(h > 0.0 for h in seen)


# ---- the 7x7 solve ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_ldlt_against_numpy(name):
    seen = []
    O.optimize(case(name), hook=lambda it, i, S, lam: seen.append((S, lam)))
    if not seen:
        assert name == "n0"
        return
    S, lam = seen[0]
    ok, x, flags = O.solve_step(S, lam, [0.0] * 7)
    if not all(O.finite(v) for v in S[:35]):
        assert name == "nan_in" and not ok and flags == O.FLAG_NONFINITE and x == [0.0] * 7
        return
    assert ok and flags == 0
    A, b = O.system_of(S, lam)
    H = np.array(A)
    H = H + np.tril(H, -1).T
    if case(name).fix_scale:
        assert H[6, 6] == lam
    want = np.linalg.solve(H, np.array(b))
    assert np.max(np.abs(np.array(x) - want)) <= 1e-10 * np.max(np.abs(want)), name


def test_ldlt_pivots_and_sign():
    A = [[-float(3 + r) if r == c else 0.25 for c in range(7)] for r in range(7)]
    tr, positive = O.ldlt([row[:] for row in A])
    assert not positive and tr[0] == 6  # negative definite; the largest |diagonal| is pivoted first
    A = [[float(2 + r) if r == c else 0.25 for c in range(7)] for r in range(7)]
    B = [row[:] for row in A]
    tr, positive = O.ldlt(B)
    assert positive and tr[0] == 6
    x = O.ldlt_solve(B, tr, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    assert np.allclose(np.array(A) @ np.array(x), [1, 2, 3, 4, 5, 6, 7], atol=1e-13)
    Z = [[0.0] * 7 for _ in range(7)]
    tr, positive = O.ldlt(Z)
    assert positive and tr == list(range(7))  # ZeroSign
    assert O.ldlt_solve(Z, tr, [1.0] * 7) == [0.0] * 7


# ---- the optimisation ------------------------------------------------------------------------------
def test_classification_reads_the_last_evaluated_state():
    """rule 5 on a hand-made state. No scene was found that ends on a rejected trial which decides a flag:
    Result.stale (flags that would differ at the final estimate) is 0 in every named case and in 5,000
    further seeded scenes run through the host build (444 of them end a round on a rejected trial, none
    changes a flag; test_optimize_classifies_at_the_last_evaluated_trial says why). So the step is pinned
    here, and the state optimize() hands to it there: the final estimate puts the
    pair inside the gate, the last evaluated trial outside it."""
    pair = (O.Edge([0.0, 0.0, 4.0], [0.0, 0.0], 1.0, [100.0, 100.0, 0.0, 0.0], False),
            O.Edge([0.0, 0.0, 4.0], [0.0, 0.0], 1.0, [100.0, 100.0, 0.0, 0.0], True))
    trial = ([0.0, 0.0, 0.0, 1.0], [0.2, 0.0, 0.0], 1.0)  # 5 px off in both cameras: chi2 = 25
    assert O.classify(pair, trial, O.sim3_inverse(trial), 10.0) is True
    assert O.classify(pair, IDENTITY, O.sim3_inverse(IDENTITY), 10.0) is False
    assert O.classify(pair, trial, O.sim3_inverse(trial), 25.0) is False  # compared with >
    assert O.classify(pair, IDENTITY, O.sim3_inverse(trial), 10.0) is True  # either edge removes the pair
    nan = ([0.0, 0.0, 0.0, 1.0], [math.nan, 0.0, 0.0], 1.0)
    assert O.classify(pair, nan, O.sim3_inverse(nan), 10.0) is False  # a NaN chi2 keeps the correspondence
    assert all(ref(name).stale == 0 for name in CASES)


def test_optimize_classifies_at_the_last_evaluated_trial(monkeypatch):
    """rule 5 inside optimize(): the state handed to the classification is the one the round's last
    activeRobustChi2 saw, also when that trial was rejected and the estimate stayed behind. A round ends on
    a rejected trial only after ten rejections in a row, when lambda has grown by 2^45 and the step has all
    but vanished: of the named cases that end so, four have a last trial equal to the estimate in every
    bit, and `clean` differs in two doubles by 4e-19. So the rule cannot decide a flag against a float
    th2 in practice (none in 5,000 seeded scenes run through the host build, 444 of which end a round on a
    rejected trial); what can be pinned is the state that is handed over, and `clean` shows it."""
    trials, classified = [], []
    real_chi, real_classify = O.sums_chi, O.classify

    def spy_chi(pairs, active, S, Si, delta, dsqr):
        trials.append(S)
        return real_chi(pairs, active, S, Si, delta, dsqr)

    def spy_classify(pair, S, Si, th2):
        classified.append((len(trials), S, Si))
        return real_classify(pair, S, Si, th2)

    monkeypatch.setattr(O, "sums_chi", spy_chi)
    monkeypatch.setattr(O, "classify", spy_classify)
    r = O.optimize(case("clean"))
    assert r.rounds[1].stop == O.STOP_TERMINATE and r.rounds[1].last_rejected
    per_round = sorted({n for n, _, _ in classified})
    assert per_round == [r.rounds[0].trials, r.rounds[0].trials + r.rounds[1].trials]
    for n, S, Si in classified:
        assert O.flat(S) == O.flat(trials[n - 1]) and O.flat(Si) == O.flat(O.sim3_inverse(trials[n - 1]))
    last = O.flat(trials[-1])
    assert [O.bits64(v) for v in last] != [O.bits64(v) for v in r.sim3]  # the rejected trial, not the estimate


def sim3_error(p, r):
    R = np.array(O.quat_to_matrix(r.sim3[:4])).reshape(3, 3)
    return (float(np.max(np.abs(R - p.R_true))), float(np.max(np.abs(np.array(r.sim3[4:7]) - p.t_true))),
            abs(r.sim3[7] - p.s_true))


def test_recovers_the_true_sim3_without_noise():
    rot = trans = scale = 0.0
    for seed in CLEAN_SEEDS:
        for fix, s in ((True, 1.0), (False, 1.3)):
            p = clean_scene(seed, fix, s)
            r = O.optimize(p)
            assert r.n_bad == 0 and r.rounds_run == 2 and r.n_inliers == p.n
            dr, dt, ds = sim3_error(p, r)
            rot, trans, scale = max(rot, dr), max(trans, dt), max(scale, ds)
    print("noise-free recovery: max |R - R_true| = %.3g, |t - t_true| = %.3g, |s - s_true| = %.3g" % (rot, trans, scale))
    assert rot <= 4 * MEASURED_ROT and trans <= 4 * MEASURED_TRANS and scale <= 4 * MEASURED_SCALE


@pytest.mark.parametrize("seed", OUTLIER_SEEDS)
def test_planted_outliers_are_the_removal_mask(seed):
    p = outlier_scene(seed)
    r = O.optimize(p)
    assert p.planted_outlier.sum() > 10
    assert np.array_equal(r.removed, p.planted_outlier)
    assert r.n_inliers == p.n - int(p.planted_outlier.sum())


def test_scenes_take_the_branch_they_are_named_for():
    zero = O.Round().key()
    p, r = case("n0"), ref("n0")
    assert (r.n_correspondences, r.rounds_run, r.n_inliers, r.n_bad) == (0, 1, 0, 0)
    assert r.rounds[0].stop == O.STOP_NO_EDGE and r.rounds[0].iterations == 0 and r.rounds[1].key() == zero
    for name in ("n0", "n9", "drops_below_10", "all_out"):  # the early return: the start as constructed
        p, r = case(name), ref(name)
        assert r.rounds_run == 1 and r.n_inliers == 0 and r.rounds[1].key() == zero, name
        assert r.sim3 == O.flat(O.sim3_from_floats(p.r12, p.t12, float(p.s12))), name
    assert ref("n9").n_correspondences == 9 and ref("n9").rounds[0].iterations >= 1 and ref("n9").n_bad == 0
    assert ref("n10").rounds_run == 2 and ref("n10").n_correspondences == 10
    assert ref("n64").n_correspondences == 64 and ref("n65").n_correspondences == 65
    p, r = case("n130_sparse"), ref("n130_sparse")
    assert r.n_correspondences == 40 and p.n == 130 and np.flatnonzero(p.valid)[-1] >= 128 and not r.scw.any()
    assert ref("n64").scw.any()
    r = ref("clean")
    assert r.rounds[0].n_bad == 0 and r.rounds[1].iterations <= 5 and r.rounds_run == 2
    r = ref("cap5")  # nBad == 0 -> optimize(5): round 2 ends at 5 iterations with no stop rule met
    assert r.rounds[0].n_bad == 0 and r.rounds[1].iterations == 5 and r.rounds[1].stop == O.STOP_ALL
    r = ref("cap10")  # nBad > 0 -> optimize(10)
    assert r.rounds[0].n_bad > 0 and r.rounds[1].iterations == 10 and r.rounds[1].stop == O.STOP_ALL
    r = ref("outliers")
    assert r.rounds[0].n_bad > 0 and r.rounds_run == 2 and r.rounds[1].n_active == 120 - r.rounds[0].n_bad
    p, r = case("drops_below_10"), ref("drops_below_10")
    assert r.n_correspondences >= 10 and r.n_correspondences - r.n_bad < 10 and np.array_equal(r.removed, p.planted_outlier)
    p, r = case("all_out"), ref("all_out")
    assert r.n_bad == r.n_correspondences == 20 and r.removed.all()
    rf, rx = ref("free_scale"), ref("fix_scale")
    assert abs(rf.sim3[7] - 1.3) < 0.01 and rx.sim3[7] == float(np.float32(1.3 * 1.05))
    steps = []
    O.optimize(case("free_scale"), hook=lambda it, i, S, lam: steps.append(O.solve_step(S, lam, [0.0] * 7)[1]))
    assert abs(steps[0][6]) >= 1e-5  # the sigma >= 1e-5 branches of Sim3(update)
    assert (case("two_cameras").k1 != case("two_cameras").k2).all()
    assert any(rd.rejected_trials > 0 for rd in ref("far_start").rounds)
    p, r = case("behind"), ref("behind")
    i = int(np.flatnonzero(p.valid)[1])
    S = O.sim3_from_floats(p.r12, p.t12, float(p.s12))
    assert O.sim3_map(S, [float(v) for v in p.p3d2c[i]])[2] < 0 and r.removed[i] and r.flags == 0
    p, r = case("nan_in"), ref("nan_in")
    assert r.flags & O.FLAG_NONFINITE and not r.removed[p.nan_entry] and r.rounds_run == 2
    for name in CASES:
        assert all(rd.iterations <= 10 and rd.trials <= 10 * rd.iterations for rd in ref(name).rounds), name


# ---- the stand-alone host program ------------------------------------------------------------------
def nan_insensitive(row):
    """NaN payloads and signs are not part of the comparison"""
    out = []
    for tok in row.split():
        if len(tok) == 16 and (int(tok, 16) & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000:
            tok = "nan64"
        elif len(tok) == 8 and (int(tok, 16) & 0x7FFFFFFF) > 0x7F800000:
            tok = "nan32"
        out.append(tok)
    return out


def build_host_program():
    exe = os.path.join(ROOT, "tests", "cpp", "build", "optsim3_core_main")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "optsim3_core_main.cpp")], check=True)
    return exe


def test_core_header_on_the_host_matches_the_restatement_under_sanitizers(tmp_path):
    exe = build_host_program()
    problems = [case(name) for name in CASES]
    path = tmp_path / "problems.txt"
    O.write_problems(str(path), problems)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = out.stdout.strip().split("\n")
    assert len(rows) == len(problems)
    for name, p, row in zip(CASES, problems, rows):
        assert nan_insensitive(row) == nan_insensitive(O.expected_row(p, ref(name))), name
    # os_exp against the restated exp, bit for bit, over the grid of the ulp test and beyond
    xs = exp_grid()[::7] + [-745.0, -744.0, -700.5, -37.25, 11.0, 300.125, 709.5, 710.0, -746.0, math.inf, -math.inf]
    path = tmp_path / "exp.txt"
    path.write_text("\n".join("%016x" % struct.unpack("<Q", struct.pack("<d", x))[0] for x in xs) + "\n")
    out = subprocess.run([exe, "exp", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.split()
    assert got == ["%016x" % O.bits64(O.exp(x)) for x in xs]
