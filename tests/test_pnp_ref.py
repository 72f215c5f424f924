"""tests/pnp_ref.py pinned on its own, without the library: the selection, SetRansacParameters, the
iterate() loop condition, the record rule, each Jacobi SVD against numpy, EPnP against the true pose
on noise-free scenes, the branch coverage of the scenes the GPU test uses, and the stand-alone host
program over orbfe_pnp_core.h (built with ASan + UBSan) against the restatement, bit for bit."""
import os
import struct
import subprocess

import numpy as np

import pnp_ref as P
from pnp_scenes import CASES, RELOC, Scene, case, draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest deviation of EPnP over all points from the true pose on the noise-free scenes below,
# measured with this file (float32 inputs, KITTI-like K), and asserted with a factor 4: the margin
# covers other seeds, not other platforms -- the arithmetic is IEEE double throughout.
MEASURED_ROT = 3.4e-8    # max |R - R_true|
MEASURED_TRANS = 2.5e-7  # max |t - t_true|


def test_swap_remove_selection_by_hand():
    # n = 6: list 0 1 2 3 4 5
    assert P.select4(6, (0, 0, 0, 0)) == [0, 5, 4, 3]     # each removal brings the last element to slot 0
    assert P.select4(6, (5, 4, 3, 2)) == [5, 4, 3, 2]     # always the last element
    assert P.select4(6, (2, 2, 2, 2)) == [2, 5, 4, 3]     # colliding draws pick the swapped-in values
    assert P.select4(6, (1, 4, 1, 0)) == [1, 4, 5, 0]     # 0 5 2 3 4 -> 0 5 2 3 -> 0 3 2
    assert P.select4(4, (3, 0, 1, 0)) == [3, 0, 1, 2]     # 0 1 2 -> 2 1 -> 2
    assert P.select4(7, (3, 3, 4, 0)) == [3, 6, 4, 0]     # 0 1 2 6 4 5 -> 0 1 2 5 4 -> 0 1 2 5
    for n in (4, 5, 9):
        for d in draws(n, 50, n):
            idx = P.select4(n, d)
            assert len(set(idx)) == 4 and all(0 <= i < n for i in idx)


def test_set_ransac_parameters_steps():
    s2 = np.ones(100, np.float32)
    # Relocalization's own call on 100 matches: 0.5 * 100 = 50 inliers, epsilon stays, 35 iterations
    mi, eps, its, me = P.ransac_parameters(100, *RELOC, s2)
    assert (mi, its) == (50, 35) and eps == 0.5
    assert me.dtype == np.float32 and me[0] == np.float32(5.991)
    # N * epsilon truncates: 15 * 0.5 = 7.5 -> 7, raised to minInliers 10; epsilon raised to 10/15 in float
    mi, eps, its, _ = P.ransac_parameters(15, *RELOC, s2[:15])
    assert mi == 10 and eps == float(np.float32(10) / np.float32(15))
    assert its == int(np.ceil(np.log(1 - 0.99) / np.log(1 - eps ** 3)))
    # N == minInliers -> one iteration
    assert P.ransac_parameters(10, *RELOC, s2[:10])[2] == 1
    assert P.ransac_parameters(4, 0.99, 2, 300, 4, 0.1, 5.991, s2[:4])[:3] == (4, 1.0, 1)   # minSet lifts it
    # N < minInliers: epsilon > 1, log of a negative number, NaN -> INT_MIN -> 1
    assert P.ransac_parameters(5, *RELOC, s2[:5])[2] == 1
    # maxIterations caps; probability 1 -> log(0) = -inf -> -inf / negative = +inf -> INT_MIN -> 1
    assert P.ransac_parameters(100, 0.99, 10, 20, 4, 0.5, 5.991, s2)[2] == 20
    assert P.ransac_parameters(100, 1.0, 10, 300, 4, 0.5, 5.991, s2)[2] == 1
    # mvMaxError is a float product
    s = np.array([1.44, 2.0736], np.float32)
    assert np.array_equal(P.ransac_parameters(2, *RELOC, s)[3], s * np.float32(5.991))


def test_loop_condition_runs_the_first_iterate_to_max_its():
    counts = [0] * 40
    state = [0, 0, -1]
    o = P.iterate_counts(counts, {}, 10, 35, 5, state)
    assert state[0] == 35 and o["no_more"] == 1 and o["returned"] == 0   # || : on to mRansacMaxIts
    o = P.iterate_counts(counts, {}, 10, 35, 5, state)
    assert state[0] == 40 and o["no_more"] == 1                          # afterwards five at a time
    # with an unrefined best at the end: returned == 2
    counts = [0, 12, 0, 11]
    state = [0, 0, -1]
    o = P.iterate_counts(counts, {1: 10}, 10, 4, 5, state)
    assert o == dict(accepted=-1, returned=2, no_more=1, n_inliers=12) and state == [4, 12, 1]
    # the evaluated hypotheses run out below max_its: no bNoMore
    state = [0, 0, -1]
    o = P.iterate_counts([0, 0], {}, 10, 35, 5, state)
    assert o["no_more"] == 0 and state[0] == 2


def sequential_transcription(counts, refine, min_inliers, max_its, n_iterations, st):
    """:193-250 literally: Refine is called at every qualifying iteration, on the best set so far.
    st = dict(it, best_inliers, best). refine(best) -> refined count."""
    cur = 0
    while (st["it"] < max_its or cur < n_iterations) and st["it"] < len(counts):
        cur += 1
        k = st["it"]
        st["it"] += 1
        if counts[k] >= min_inliers:
            if counts[k] > st["best_inliers"]:
                st["best_inliers"], st["best"] = counts[k], k
            n_refined = refine(st["best"])
            if n_refined > min_inliers:
                return (1, st["best"], n_refined, k)
    return (0, -1, 0, -1)


def test_record_rule_against_the_sequential_transcription():
    rng = np.random.default_rng(5)
    for trial in range(300):
        n_hyp = int(rng.integers(1, 30))
        min_inl = int(rng.integers(4, 9))
        counts = [int(c) for c in rng.integers(0, 14, n_hyp)]
        refined_of = {k: int(rng.integers(0, 14)) for k in range(n_hyp)}   # Refine is a function of the best set
        rec = P.records_of(counts, min_inl)
        refined = {k: refined_of[k] for k in rec}
        max_its = int(rng.integers(1, 35))
        st, state = dict(it=0, best_inliers=0, best=-1), [0, 0, -1]
        for _ in range(8):
            n_it = int(rng.integers(0, 7))
            lit = sequential_transcription(counts, lambda b: refined_of[b], min_inl, max_its, n_it, st)
            o = P.iterate_counts(counts, refined, min_inl, max_its, n_it, state)
            assert (o["returned"] == 1) == (lit[0] == 1)
            if lit[0]:
                assert o["accepted"] == lit[1] and o["n_inliers"] == lit[2]
            assert state == [st["it"], st["best_inliers"], st["best"]]
        # find() from a fresh state: qualifying non-records never change the outcome -- the literal walk
        # accepts at a record's own iteration, the first record whose refinement succeeds
        st = dict(it=0, best_inliers=0, best=-1)
        lit = sequential_transcription(counts, lambda b: refined_of[b], min_inl, max_its, max_its, st)
        first = [k for k in rec if k < max_its and refined[k] > min_inl][:1]
        assert (lit[1], lit[3]) == ((first[0], first[0]) if first else (-1, -1))
        assert P.find_counts(counts, refined, min_inl, max_its)["accepted"] == lit[1]


def test_jacobi_svd_against_numpy():
    rng = np.random.default_rng(7)
    for n in (12, 3):
        for trial in range(4):
            A = rng.normal(size=(n, n)) * 10
            if trial % 2 == 0:
                A = A.T @ A                                  # the symmetric case compute_pose feeds it
            At = [[float(v) for v in row] for row in A.T]    # At = the transposed input
            flags = [0]
            W, Vt = P.jacobi_svd(At, n, n, flags)
            assert flags[0] == 0
            sv = np.linalg.svd(A, compute_uv=False)
            assert np.allclose(W, sv, rtol=1e-12, atol=1e-12 * sv[0])
            U = np.array(At).T
            rec = (U * np.array(W)) @ np.array(Vt)
            assert np.allclose(rec, A, rtol=0, atol=1e-11 * sv[0])
    # 6 x N systems of find_betas_approx: cvSolve(CV_SVD) against the least-squares solution
    for nn in (3, 4, 5):
        A = rng.normal(size=(6, nn))
        b = rng.normal(size=6)
        x = P.solve_svd([[float(v) for v in A[:, c]] for c in range(nn)], [float(v) for v in b], [0])
        assert np.allclose(x, np.linalg.lstsq(A, b, rcond=None)[0], atol=1e-12)


def noise_free_deviation():
    rot = trans = 0.0
    for seed in range(40, 48):
        sc = Scene(n=30 + seed, seed=seed, noise=0.0, outliers=0.0)
        R, t, N, flags = P.pose_of(sc.p3dw, sc.p2d, [float(v) for v in sc.k], range(sc.n))
        assert flags == 0
        rot = max(rot, float(np.abs(np.array(R).reshape(3, 3) - sc.R).max()))
        trans = max(trans, float(np.abs(np.array(t) - sc.t).max()))
    return rot, trans


def test_epnp_recovers_the_true_pose_without_noise():
    rot, trans = noise_free_deviation()
    print("measured", rot, trans)
    assert rot <= 4 * MEASURED_ROT and trans <= 4 * MEASURED_TRANS


def test_scenes_cover_the_branches():
    solvers = {}
    for name in CASES:
        sc, params, d = case(name)
        solvers[name] = P.Solver(sc.p3dw, sc.p2d, sc.sigma2, sc.k, params, d)
    launched = {n: s for n, s in solvers.items() if s.launched}
    assert any(len(s.records) >= 2 for s in launched.values())
    assert any(len(s.records) >= 2 and s.refined[s.records[0]].count <= s.min_inliers
               and s.find()["accepted"] in s.records[1:] for s in launched.values())
    # no acceptance, the unrefined best returned
    outs = {n: P.iterate_counts(s.counts, s.refined_counts, s.min_inliers, s.max_its, s.max_its, [0, 0, -1])
            for n, s in launched.items()}
    assert any(o["returned"] == 2 for o in outs.values())
    assert any(o["returned"] == 1 for o in outs.values())
    assert any(not s.launched and s.n < s.min_inliers for s in solvers.values())
    chosen = {h.N for s in launched.values() for h in s.hyp}
    assert chosen == {1, 2, 3}
    for n, s in launched.items():
        fl = {h.flags for h in s.hyp} | {r.flags for r in s.refined.values()}
        if not n.startswith("degenerate"):
            assert fl <= {0}, n
    assert any(h.flags & P.FLAG_SVD_NULL for h in solvers["degenerate_planar"].hyp)
    # the sizes the kernels can go wrong at
    assert {s.n for s in solvers.values()} >= {3, 4, 5, 63, 64, 65, 100}
    assert {len(s.hyp) for s in launched.values()} >= {1, 3, 4, 5, 24}
    refined_over = {len(r.idx) for s in launched.values() for r in s.refined.values()}
    assert refined_over >= {4, 64, 65}
    assert len(solvers["workload"].hyp) == 24 and solvers["workload"].params == RELOC


def bits32(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def test_core_header_on_the_host_matches_the_restatement_under_sanitizers(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "build", "pnp_core_main")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pnp_core_main.cpp")],
                   check=True)
    samples = []
    for name in ("n4", "n5", "h24", "degenerate_planar", "degenerate_duplicate", "n65"):
        sc, params, d = case(name)
        for dr in d[:3]:
            samples.append((sc, P.select4(sc.n, dr)))
        samples.append((sc, list(range(sc.n))))           # the refinement's shape: EPnP over many points
    lines = [str(len(samples))]
    for sc, idx in samples:
        lines.append("%d %s" % (len(idx), " ".join(bits32(v) for v in sc.k)))
        for i in idx:
            lines.append(" ".join(bits32(v) for v in list(sc.p3dw[i]) + list(sc.p2d[i])))
    path = tmp_path / "samples.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = out.stdout.strip().split("\n")
    assert len(rows) == len(samples)
    for (sc, idx), row in zip(samples, rows):
        R, t, N, flags = P.pose_of(sc.p3dw, sc.p2d, [float(v) for v in sc.k], idx)
        f = row.split()
        assert (int(f[0]), int(f[1])) == (N, flags)
        got = np.array([int(x, 16) for x in f[2:]], np.uint64).view(np.float64)
        want = np.array(R + t, np.float64)
        same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (len(idx), got, want)
