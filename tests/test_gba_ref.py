"""tests/gba_ref.py pinned on its own, without the library: the branch each scene of the GPU test is named
for, the Huber constant, the envelope LDL^T against lba_ref's dense one bit for bit, the sparse Schur
complement against lba_ref's dense one bit for bit, one Schur step against numpy's solve of the full
system, recovery on noise-free scenes, and the stand-alone host program over orbfe_gba_core.h (built with
ASan + UBSan) against the restatement, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import gba_ref as G
import lba_ref as R
import poseopt_ref as P
from gba_scenes import CASES, CLEAN_SEEDS, case, clean_scene, lba_like_scene
from test_lba_ref import bits32, full_system, nan_insensitive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Measured with this file (the tests print them) and asserted with a factor 4: the margin covers other
# seeds, not other platforms -- the arithmetic is IEEE double throughout.
MEASURED_SCHUR_GAP = 5.4e-13  # a Schur step vs numpy.linalg.solve of the full system, worst relative gap
MEASURED_ROT = 3.9e-5         # noise-free recovery over a chain with one fixed keyframe, float32 inputs: max |R - R*|
MEASURED_TRANS = 2.4e-4       # max |t - t*|
MEASURED_POINT = 2.1e-3       # max |X - X*|

ref = G.solve_case


def test_the_mono_delta_is_5_99():
    assert G.DELTA_MONO == float(np.float32(np.sqrt(5.99))) and G.DELTA_MONO != P.DELTA_MONO
    assert G.DELTA_STEREO == float(np.float32(np.sqrt(7.815))) == P.DELTA_STEREO
    S = G.Solver(case("pair_mono"))
    assert S.deltas == (G.DELTA_MONO, G.DELTA_STEREO)


def test_each_scene_takes_the_branch_it_is_named_for():
    r, p = ref("pair_mono"), case("pair_mono")
    assert p.n_kf == 2 and list(p.fixed) == [1, 0] and (p.u_right < 0).all() and p.n_iterations == 20 and p.robust == 1
    assert r.solver.nslot == 1 and r.trace.iterations > 0
    r, p = ref("chain"), case("chain")
    env = r.solver.env
    assert p.n_kf == 12 and env.ns == 11 and max(env.row_first) > 0 and r.env_blocks == r.schur_blocks
    assert all(s - env.row_first[s] <= 2 for s in range(env.ns))  # banded: three consecutive keyframes per point
    r = ref("loop")
    env = r.solver.env
    assert r.env_blocks > r.schur_blocks and env.row_first[env.ns - 1] == 0
    # the blocks without a structural pair start as +0.0 and fill in
    assert (env.ns - 1, 3) not in {(b, a) for a, b in env.pairs}
    blk = (env.row_off[env.ns - 1] + 3) * 36
    assert all(v == 0.0 and np.copysign(1.0, v) == 1.0 for v in r.solver.last["S"][blk:blk + 36])
    assert any(v != 0.0 for v in r.solver.last["L"][blk:blk + 36])
    r = ref("past_lba")
    assert r.solver.nslot == 130 > 128 and 6 * r.solver.nslot > 256
    r, p = ref("not_robust"), case("not_robust")
    assert p.robust == 0 and p.n_iterations == 10 and p.planted.sum() > 0 and not r.solver.kernel_on
    assert r.trace.rejected_trials >= 1
    p = case("mixed")
    assert p.n_points >= 64 and (p.u_right < 0).any() and (p.u_right >= 0).any()
    r, p = ref("no_fixed"), case("no_fixed")
    assert not p.fixed.any() and r.solver.nslot == p.n_kf
    r, p = ref("orphan_kf"), case("orphan_kf")
    last = p.n_kf - 1
    assert not (p.edge_kf == last).any() and not p.fixed[last] and r.solver.slot_of_free[r.solver.kf_free[last]] == -1
    assert np.array_equal(r.tcw[last], P.se3_to_tcw(P.se3_from_tcw(p.tcw[last])))  # written out, through the quaternion
    r, p = ref("orphan_point"), case("orphan_point")
    assert not r.included[-1] and r.included[:-1].all() and not r.solver.p_active[-1]
    assert np.array_equal(r.xw[-1].view(np.uint32), p.xw[-1].view(np.uint32))
    r, p = ref("fixed_only_point"), case("fixed_only_point")
    assert all(p.fixed[k] for k in p.edge_kf[p.edge_begin[-2]:]) and r.included[-1]
    assert not np.array_equal(r.xw[-1], p.xw[-1])  # it is in the system: Hll and b only
    r = ref("nonfinite")
    assert r.flags & G.FLAG_NONFINITE and any(r.trace.fail_trace) and r.trace.rejected_trials > 0
    r, p = ref("stop0"), case("stop0")
    assert r.trace.iterations == 0 and r.trace.stop == G.STOP_FLAG and r.polls == 1
    assert np.array_equal(r.xw.view(np.uint32), p.xw.view(np.uint32))
    r, p = ref("stop_mid"), case("stop_mid")
    assert r.trace.stop == G.STOP_FLAG and 0 < r.trace.iterations < p.n_iterations
    r, p = ref("empty"), case("empty")
    assert r.polls == 0 and r.trace.iterations == 0 and r.solver is None
    assert np.array_equal(r.tcw.view(np.uint32), p.tcw.view(np.uint32))


def linearized(p, **kw):
    S = G.Solver(p, **kw)
    S.set_active(None, bool(p.robust))
    chi, maxdiag = S.linearize()
    return S, 1e-5 * maxdiag


@pytest.mark.parametrize("name", ["chain", "loop"])
def test_envelope_ldlt_equals_the_dense_one_bit_for_bit(name):
    S, lam = linearized(case(name))
    S.trial(lam)
    env, n = S.env, 6 * S.env.ns
    A = env.dense(S.last["S"])  # lower triangle; lba_ref reads the upper one
    dense = [float(v) for v in A.T.reshape(-1)]
    Lm, d, fail, _ = R.ldlt_factor(dense, n)
    assert not fail
    L = list(S.last["S"])
    d_env, fail_env, _ = G.env_factor(env, L)
    assert not fail_env
    assert [P.bits64(v) for v in d_env] == [P.bits64(v) for v in d]
    inside = 0
    for i in range(n):
        for j in range(i):
            if j >= 6 * env.row_first[i // 6]:
                assert P.bits64(L[env.at(i, j)]) == P.bits64(Lm[j][i]), (i, j)
                inside += 1
            else:
                assert Lm[j][i] == 0.0, (i, j)  # outside the envelope: exact zeros
    assert inside == 36 * env.nblk - 21 * env.ns
    x = R.ldlt_solve(Lm, d, S.last["bs"], n)
    assert [P.bits64(v) for v in G.env_solve(env, L, d_env, S.last["bs"])] == [P.bits64(v) for v in x]
    assert [P.bits64(v) for v in S.xp] == [P.bits64(v) for v in x]


def test_sparse_schur_equals_lba_refs_dense_one_bit_for_bit():
    p = lba_like_scene()
    assert list(p.fixed) == [1] + [0] * (p.n_kf - 1)
    S, lam = linearized(p, deltas=(P.DELTA_MONO, P.DELTA_STEREO))  # the Huber deltas made equal
    D = R.Solver(p)
    D.set_active(None, True)
    chi, maxdiag = D.linearize()
    assert 1e-5 * maxdiag == lam
    S.trial(lam), D.trial(lam)
    n, env = D.last["n"], S.env
    assert n == 6 * env.ns and env.nblk > len(env.pairs)
    A = env.dense(S.last["S"])
    for i in range(n):
        for j in range(i + 1):
            assert P.bits64(float(A[i, j])) == P.bits64(D.last["S"][j * n + i]), (i, j)
    assert [P.bits64(v) for v in S.last["bs"]] == [P.bits64(v) for v in D.last["bs"]]
    assert [P.bits64(v) for v in S.xp] == [P.bits64(v) for v in D.xp]


FINITE_CASES = [n for n in CASES if n not in ("nonfinite", "empty", "stop0", "past_lba")]


def test_schur_step_against_numpy_solve_of_the_full_system():
    worst = 0.0
    for name in FINITE_CASES:
        S, lam = linearized(case(name))
        S.trial(lam)
        act = [pt for pt in range(S.np_) if S.p_active[pt]]
        H, b = full_system(S, lam)
        n = 6 * S.nslot
        keep = list(range(n)) + [n + 3 * pt + k for pt in act for k in range(3)]
        want = np.linalg.solve(H[np.ix_(keep, keep)], b[keep])
        got = np.array(list(S.xp) + [v for pt in act for v in S.p_xl[pt]])
        worst = max(worst, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
    print("worst relative Schur step gap", worst)
    assert worst <= 4 * MEASURED_SCHUR_GAP


def test_noise_free_recovery():
    rot = trans = point = 0.0
    for seed in CLEAN_SEEDS:
        p = clean_scene(seed)
        o = G.solve(p)
        assert o.flags == 0 and o.trace.iterations > 0
        free = p.fixed == 0
        got, want = o.tcw.reshape(-1, 3, 4)[free].astype(float), p.true_tcw.reshape(-1, 3, 4)[free]
        rot = max(rot, float(np.max(np.abs(got[:, :, :3] - want[:, :, :3]))))
        trans = max(trans, float(np.max(np.abs(got[:, :, 3] - want[:, :, 3]))))
        point = max(point, float(np.max(np.abs(o.xw.astype(float) - p.true_xw))))
    print("recovery: rot", rot, "trans", trans, "point", point)
    assert rot <= 4 * MEASURED_ROT and trans <= 4 * MEASURED_TRANS and point <= 4 * MEASURED_POINT


@pytest.mark.parametrize("name", CASES)
def test_accepted_iterations_never_raise_chi2(name):
    for before, temp, accepted in ref(name).trace.chi_trace:
        if accepted:
            assert temp < before or not (before == before), (name, before, temp)


# ---- the core header on the host --------------------------------------------------------------------
def write_problems(path, problems):
    with open(path, "w") as f:
        f.write("%d\n" % len(problems))
        for p in problems:
            f.write("%d %d %d %d %d %d\n" % (p.n_kf, p.n_points, p.n_edges, p.stop_at_poll, p.n_iterations, p.robust))
            for i in range(p.n_kf):
                vals = list(p.tcw[i]) + list(p.k[i]) + [p.bf[i]]
                f.write("%d %s\n" % (p.fixed[i], " ".join(bits32(v) for v in vals)))
            for pt in range(p.n_points):
                b, e = p.edge_begin[pt], p.edge_begin[pt + 1]
                f.write("%d %s\n" % (e - b, " ".join(bits32(v) for v in p.xw[pt])))
                for j in range(b, e):
                    vals = [p.kp_un[j, 0], p.kp_un[j, 1], p.u_right[j], p.inv_sigma2[j]]
                    f.write("%d %s\n" % (p.edge_kf[j], " ".join(bits32(v) for v in vals)))


def expected_row(r):
    k = G.trace_key(r)
    f = ["%d %d %d %d %d %016x %016x %d %d %d %d" % k]
    f += [bits32(v) for v in r.tcw.reshape(-1)]
    f += [bits32(v) for v in r.xw.reshape(-1)]
    return " ".join(f)


def build_host_program():
    exe = os.path.join(ROOT, "tests", "cpp", "build", "gba_core_main")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "gba_core_main.cpp")], check=True)
    return exe


def test_core_header_on_the_host_matches_the_restatement_under_sanitizers(tmp_path):
    exe = build_host_program()
    problems = [case(name) for name in CASES]
    path = tmp_path / "problems.txt"
    write_problems(path, problems)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = out.stdout.strip().split("\n")
    assert len(rows) == len(problems)
    for name, row in zip(CASES, rows):
        assert nan_insensitive(row) == nan_insensitive(expected_row(ref(name))), name
