"""tests/essgraph_ref.py pinned on its own, without the library: log and acos against libm, Sim3::log()
against exp and a hand-worked value, the 3x3 LU and the envelope LDL^T against numpy and against the
dense LDL^T, the numeric Jacobians against a second difference, noise-free recovery, the branch each scene
of the GPU test is named for, the point correction, and the stand-alone host program over
orbfe_essgraph_core.h (built with ASan + UBSan) against the restatement, bit for bit."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import essgraph_ref as R
import optsim3_ref as O
import poseopt_ref as P
from essgraph_scenes import CASES, case, recovery_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured with this file (the tests print them) and asserted with a factor 4: the margin covers other
# seeds, not other platforms -- the arithmetic is IEEE double throughout.
MEASURED_JAC_GAP = 3.2e-7      # the +-1e-9 Jacobians vs a +-1e-6 difference, worst gap relative to max(1, |J|)
MEASURED_LDLT_GAP = 7.7e-13    # the envelope step vs numpy.linalg.solve of the densified system, relative
MEASURED_ROT = 8.7e-8          # noise-free recovery, float32 inputs: max |R - R*|
MEASURED_TRANS = 5.8e-7        # max |t - t*|
MEASURED_ROUNDTRIP = 1.4e-15   # log(exp(v)) - v, worst absolute


@functools.lru_cache(None)
def ref(name):
    return R.solve(case(name))


def ulps(a, b):
    return abs(P.bits64(a) - P.bits64(b)) if (a >= 0) == (b >= 0) else P.bits64(abs(a)) + P.bits64(abs(b))


def test_log_within_2_ulp_of_libm():
    """The domain in use is a scale: a dense grid over [1e-3, 1e3], the neighbourhood of 1 down to single
    ulps, and the reduction's boundaries."""
    xs = list(np.exp(np.linspace(math.log(1e-3), math.log(1e3), 40001)))
    xs += [1.0 + k * 2.0 ** -e for e in range(10, 53) for k in (-3, -2, -1, 1, 2, 3)]
    xs += list(np.linspace(1 - 1e-4, 1 + 1e-4, 20001))
    xs += list(np.linspace(0.70, 0.72, 4001)) + list(np.linspace(1.37, 1.43, 4001)) + [1.0, 2.0, 0.5, 1e-300, 1e300]
    worst = max(ulps(R.log(float(x)), math.log(float(x))) for x in xs)
    print("log: worst ulp gap", worst)
    assert worst <= 2
    assert R.log(1.0) == 0.0 and R.log(0.0) == -math.inf and math.isnan(R.log(-1.0)) and R.log(math.inf) == math.inf


def test_acos_within_2_ulp_of_libm():
    xs = list(np.linspace(-1.0, 1.0, 80001))
    xs += [s * (1.0 - k * 2.0 ** -e) for e in range(8, 54) for k in (1, 2, 3) for s in (-1.0, 1.0)]
    xs += [s * k * 2.0 ** -e for e in range(2, 70) for k in (1, 3) for s in (-1.0, 1.0)]
    xs += list(np.linspace(-0.51, -0.49, 4001)) + list(np.linspace(0.49, 0.51, 4001)) + [0.0, 1.0, -1.0]
    worst = max(ulps(R.acos(float(x)), math.acos(float(x))) for x in xs)
    print("acos: worst ulp gap", worst)
    assert worst <= 2
    assert R.acos(1.0) == 0.0 and R.acos(-1.0) == math.pi and math.isnan(R.acos(1.5))


BRANCH_VECTORS = {
    (True, True): [1e-7, -2e-7, 3e-7, 0.3, -0.2, 0.5, 2e-6],
    (True, False): [0.3, -0.4, 0.2, 0.3, -0.2, 0.5, -3e-6],
    (False, True): [2e-7, 1e-7, -1e-7, 0.3, -0.2, 0.5, 0.4],
    (False, False): [0.5, 0.1, -0.7, 1.0, 2.0, -3.0, -0.6],
}


def test_log_of_exp_round_trip_in_each_branch():
    worst = 0.0
    for branch, v in BRANCH_VECTORS.items():
        S, _ = O.sim3_from_update(list(v))
        assert R.log_branch(S) == branch
        worst = max(worst, max(abs(a - b) for a, b in zip(R.sim3_log(S), v)))
    print("log(exp(v)) worst gap", worst)
    assert worst <= 4 * MEASURED_ROUNDTRIP


def test_hand_worked_log_of_an_exact_sim3():
    """A quarter turn about z, scale 2: omega = (0, 0, pi/2), sigma = ln 2; with t = W (1, 0, 0) for the
    branch's A, B, C the translation part is (1, 0, 0)."""
    h = math.sqrt(0.5)
    theta, sigma, s = math.pi / 2, math.log(2.0), 2.0
    a, b, c = s * 1.0, s * 0.0, theta * theta + sigma * sigma
    C = (s - 1) / sigma
    A = (a * sigma + (1 - b) * theta) / (theta * c)
    B = (C - ((b - 1) * sigma + a * theta) / c) / (theta * theta)
    # W = A Omega + B Omega^2 + C I with Omega = skew(0, 0, theta): first column (C - B theta^2, A theta, 0)
    t = [C - B * theta * theta, A * theta, 0.0]
    out = R.sim3_log(([0.0, 0.0, h, h], t, s))
    assert np.allclose(out, [0.0, 0.0, theta, 1.0, 0.0, 0.0, sigma], atol=1e-14)
    assert R.sim3_log(([0.0, 0.0, 0.0, 1.0], [1.0, 2.0, 3.0], 1.0)) == [0.0, 0.0, 0.0, 1.0, 2.0, 3.0, 0.0]


def test_lu3_against_numpy():
    rng = np.random.default_rng(0)
    for _ in range(200):
        W, t = rng.normal(0, 1, (3, 3)), rng.normal(0, 1, 3)
        x = R.lu3_solve(list(W.reshape(-1)), list(t))
        assert np.allclose(x, np.linalg.solve(W, t), rtol=1e-9, atol=1e-11)
    # the pivot: the first of two equal maxima, and a zero leading entry
    assert R.lu3_solve([0.0, 1.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 4.0], [1.0, 2.0, 4.0]) == [1.0, 1.0, 1.0]


def test_numeric_jacobians_against_a_second_difference():
    rng = np.random.default_rng(1)
    worst, h = 0.0, 1e-6
    for fix_scale in (False, True):
        for _ in range(6):
            Si, _ = O.sim3_from_update(list(rng.uniform(-0.5, 0.5, 7)))
            Sj, _ = O.sim3_from_update(list(rng.uniform(-0.5, 0.5, 7)))
            C, _ = O.sim3_from_update(list(rng.uniform(-0.1, 0.1, 7)))
            C = O.sim3_mul(C, O.sim3_mul(Sj, O.sim3_inverse(Si)))
            _, J = R.jacobian(C, Si, Sj, fix_scale, -1)
            for side in (0, 1):
                for d in range(7):
                    es = []
                    for delta in (h, -h):
                        u = [0.0] * 7
                        u[d] = delta
                        Pp, _ = O.oplus(u, fix_scale, Sj if side else Si)
                        es.append(np.array(R.edge_error(C, Si, Pp) if side else R.edge_error(C, Pp, Sj)))
                    num = (es[0] - es[1]) / (2 * h)
                    ana = np.array([J[k][7 * side + d] for k in range(7)])
                    worst = max(worst, float(np.max(np.abs(num - ana)) / max(1.0, np.max(np.abs(ana)))))
                    if fix_scale and d == 6:
                        assert all(P.bits64(v) == 0 for v in ana)  # exactly +0
    print("worst relative Jacobian gap", worst)
    assert worst <= 4 * MEASURED_JAC_GAP


def test_fixed_vertex_has_no_jacobian():
    S = R.Solver(case("pair"))
    _, J = R.jacobian(S.meas[0], S.est[1], S.est[0], True, 1)
    assert all(J[k][7 + d] == 0.0 for k in range(7) for d in range(7)) and any(J[k][0] != 0.0 for k in range(7))


def densify(S, lam):
    n = 7 * S.ns
    A = np.zeros((n, n))
    for i in range(n):
        for k, v in enumerate(S.rows[i]):
            A[i, S.c0[i] + k] = A[S.c0[i] + k, i] = v
        A[i, i] += lam
    return A


FINITE_CASES = [n for n in CASES if n != "nonfinite"]  # that scene's system has no solution to compare


def test_envelope_step_against_numpy_and_dense_ldlt():
    worst = 0.0
    for name in FINITE_CASES:
        S = R.Solver(case(name))
        S.linearize()
        lam = 1e-16 if not case(name).fix_scale else 1e-6  # H66 = lambda: keep numpy's solve conditioned
        A = densify(S, lam)
        rows = [list(r) for r in S.rows]
        for i in range(len(rows)):
            rows[i][-1] = rows[i][-1] + lam
        ok, x, _ = R.ldlt_envelope(rows, S.c0, S.b, None)
        assert ok
        xn = np.linalg.solve(A, np.array(S.b))
        worst = max(worst, float(np.max(np.abs(np.array(x) - xn)) / max(np.max(np.abs(xn)), 1e-300)))
        if name != "ring80_band":  # the dense restatement is cubic: the small scenes pin the identity
            xd = R.ldlt_dense([list(r) for r in A], S.b)
            assert [P.bits64(v) for v in x] == [P.bits64(v) for v in xd], name
    print("worst relative gap of an envelope step", worst)
    assert worst <= 4 * MEASURED_LDLT_GAP


def test_noise_free_recovery():
    p = recovery_scene()
    r = R.solve(p)
    assert r.trace.chi2 < 1e-12
    rot = trans = 0.0
    for v, (Rt, tt) in enumerate(p.truth):
        T = r.tcw[v].reshape(3, 4).astype(np.float64)
        rot = max(rot, float(np.max(np.abs(T[:, :3] - Rt))))
        trans = max(trans, float(np.max(np.abs(T[:, 3] - tt))))
    print("recovery: max |R - R*|", rot, "max |t - t*|", trans)
    assert rot <= 4 * MEASURED_ROT and trans <= 4 * MEASURED_TRANS


@pytest.mark.parametrize("name", list(CASES))
def test_accepted_iterations_never_raise_chi2(name):
    for ini, cur in ref(name).trace.chis:
        assert cur <= ini


def test_each_scene_takes_its_branch():
    assert ref("pair").solver.ns == 1 and ref("pair").trace.env_blocks == 1
    assert ref("chain3").solver.ns == 2
    S = ref("ring12").solver
    assert S.first[9] == 0 and S.first[10] == 9 and ref("ring12").trace.env_blocks == 1 + 16 + 10 + 2  # one long row with fill
    S = ref("fixed_mid").solver
    assert S.slot_of_v[4] == -1 and S.slot_of_v[5] == 4 and S.slot_of_v[3] == 3
    a, b = ref("fix_scale"), ref("free_scale")
    assert all(a.solver.est[v][2] == a.solver.scw[v][2] for v in range(12))  # no scale moves
    assert any(b.solver.est[v][2] != b.solver.scw[v][2] for v in range(9))
    S = ref("orphan").solver
    assert S.slot_of_v[6] == -1 and S.est[6] == S.scw[6]
    p = case("dup_edge")
    pairs = [(min(i, j), max(i, j)) for i, j in zip(p.edge_i, p.edge_j)]
    assert pairs.count((0, 5)) == 3 and set(p.edge_kind[[k for k, q in enumerate(pairs) if q == (0, 5)]]) == {0, 1}
    p = case("noncorrected")
    inmap = set(int(i) for i in p.noncorrected_idx)
    assert any(int(i) in inmap and int(j) in inmap and k == 1 for i, j, k in zip(p.edge_i, p.edge_j, p.edge_kind))
    S = ref("ring80_band").solver
    assert S.ns == 79 and S.ne > 64 and S.first[77] == 0 and S.first[76] == 1  # two long rows
    S = R.Solver(case("log_branches"))
    seen = set()
    for e in range(S.ne):
        seen.add(R.log_branch(O.sim3_mul(O.sim3_mul(S.meas[e], S.est[S.ei[e]]), O.sim3_inverse(S.est[S.ej[e]]))))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    t = ref("rejected").trace
    assert 0 < t.rejected_trials < t.trials and t.rejected_trials % 10 != 0 and t.stop != P.STOP_TERMINATE
    assert all(ref(n).trace.flags == 0 for n in FINITE_CASES)
    r = ref("nonfinite")
    t = r.trace
    assert t.flags & R.FLAG_NONFINITE and t.rejected_trials >= 1 and t.rejected_trials == t.trials
    assert t.chi2 == math.inf and all(cur == ini for ini, cur in t.chis)  # no trial was accepted
    S = R.Solver(case("nonfinite"))
    S.linearize()
    bad = [i // 7 for i in range(7 * S.ns) if not all(math.isfinite(v) for v in S.rows[i])]
    assert S.ns == 4 and min(bad) == 2  # two pivot blocks factor before the failing one


def test_point_correction_against_numpy():
    p, r = case("ring12"), ref("ring12")
    S = r.solver

    def mat(Sm):
        q, t, s = Sm
        M = np.eye(4)
        M[:3, :3] = s * np.array(P.quat_to_matrix(q)).reshape(3, 3)
        M[:3, 3] = t
        return M

    assert p.n_points == 130 and (p.point_ref == p.fixed_vertex).sum() >= 26
    for i in range(p.n_points):
        v = int(p.point_ref[i])
        x = np.linalg.inv(mat(S.est[v])) @ mat(S.scw[v]) @ np.append(p.xw[i].astype(np.float64), 1.0)
        assert np.allclose(r.xw[i], x[:3], rtol=1e-6, atol=1e-6)
    assert case("chain3").n_points == 0 and ref("chain3").xw.shape == (0, 3) and case("pair").n_points == 1


# ---- the host build of orbfe_essgraph_core.h --------------------------------------------------------
def f32hex(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def write_problems(path, problems):
    with open(path, "w") as f:
        f.write(f"{len(problems)}\n")
        for p in problems:
            f.write(f"{p.n_vertices} {p.fixed_vertex} {p.fix_scale} {p.n_corrected} {p.n_noncorrected} {p.n_edges} {p.n_points}\n")
            for row in np.asarray(p.tcw, np.float32).reshape(-1, 12):
                f.write(" ".join(f32hex(v) for v in row) + "\n")
            for idx, arr in ((p.corrected_idx, p.corrected_sim3), (p.noncorrected_idx, p.noncorrected_sim3)):
                for i, row in zip(idx, np.asarray(arr, np.float64).reshape(-1, 8)):
                    f.write(f"{int(i)} " + " ".join("%016x" % P.bits64(float(v)) for v in row) + "\n")
            for i, j, k in zip(p.edge_i, p.edge_j, p.edge_kind):
                f.write(f"{int(i)} {int(j)} {int(k)}\n")
            for ref_v, x in zip(p.point_ref, np.asarray(p.xw, np.float32).reshape(-1, 3)):
                f.write(f"{int(ref_v)} " + " ".join(f32hex(v) for v in x) + "\n")


def expected_line(r):
    t = r.trace
    out = [str(t.iterations), str(t.trials), str(t.rejected_trials), str(t.stop), str(t.flags), str(t.env_blocks),
           "%016x" % P.bits64(t.lam), "%016x" % P.bits64(t.chi2)]
    out += [f32hex(v) for v in r.tcw.reshape(-1)] + [f32hex(v) for v in r.xw.reshape(-1)]
    return " ".join(out)


def test_host_program_matches_the_restatement_bit_for_bit(tmp_path):
    exe = tmp_path / "essgraph_core_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "essgraph_core_main.cpp")],
                   check=True)
    names = list(CASES)
    write_problems(tmp_path / "in.txt", [case(n) for n in names])
    out = subprocess.run([str(exe), str(tmp_path / "in.txt")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(names)
    for name, line in zip(names, out):
        assert line.strip() == expected_line(ref(name)), name
