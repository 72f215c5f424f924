"""tests/initializer_ref.py pinned on its own, without the library: the selection and Normalize by
hand, each Jacobi SVD (the fill-in of ComputeF21's row 8 included) against numpy, the recovered pose
against the true one on noise-free scenes, the branch coverage of the scenes the GPU test uses, and
the stand-alone host program over orbfe_init_core.h (built with ASan + UBSan) against the
restatement, bit for bit on every case."""
import os
import subprocess

import numpy as np

import initializer_ref as I
from initializer_scenes import CASES, Scene, bits32, case, draws, dump, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

# The largest deviations on the well-conditioned sets below, measured with this file (float32 inputs)
# and asserted with a factor 4: the margin covers other seeds, not other platforms -- the arithmetic
# is IEEE float / double throughout.
MEASURED_F_NORM = 4.2e-8         # | |row 8| - 1 |
MEASURED_F_ANNIHILATE = 6.7e-8   # max |A row 8| / |A|_2
MEASURED_F_NULL = 2.1e-5         # max |row 8 -+ numpy's null vector|
MEASURED_H_NULL = 3.4e-7         # max |vt.row(8) -+ numpy's last right vector| of the 16x9 system
MEASURED_SVD3 = 1.9e-7           # max |u diag(w) vt - M| / |M|_2 and max |w - numpy's| / w[0]
MEASURED_ROT = 1.1e-6            # max |R21 - R_true| on noise-free scenes
MEASURED_TRANS = 1.2e-5          # max |t21 - t_true / |t_true||


def test_swap_remove_selection_by_hand():
    assert I.select8(8, (0, 0, 0, 0, 0, 0, 0, 0)) == [0, 7, 6, 5, 4, 3, 2, 1]   # every set of N = 8 is the whole list
    assert I.select8(9, (8, 7, 6, 5, 4, 3, 2, 1)) == [8, 7, 6, 5, 4, 3, 2, 1]   # always the last element
    assert I.select8(9, (2, 2, 2, 2, 2, 2, 2, 1)) == [2, 8, 7, 6, 5, 4, 3, 1]   # colliding draws pick the swapped-in values
    assert I.select8(10, (1, 4, 1, 0, 5, 0, 3, 2)) == [1, 4, 9, 0, 5, 6, 3, 2]
    # 0 9 2 3 4 5 6 7 8 -> 0 9 2 3 8 5 6 7 -> 0 7 2 3 8 5 6 -> 6 7 2 3 8 5 -> 6 7 2 3 8 -> 8 7 2 3 -> 8 7 2
    for n in (8, 9, 30):
        for d in draws(n, 40, n):
            idx = I.select8(n, d)
            assert len(set(idx)) == 8 and all(0 <= i < n for i in idx)


def test_normalize_by_hand_on_three_points():
    mx, my, sx, sy = I.normalize(np.array([[1, 2], [3, 10], [8, 6]], F32))
    assert (mx, my) == (F32(4), F32(6))                      # 12 / 3, 18 / 3
    assert sx == F32(1.0 / float(F32(8) / F32(3)))           # |1-4| + |3-4| + |8-4| = 8
    assert sy == F32(1.0 / float(F32(8) / F32(3)))           # 4 + 4 + 0
    T = I.t_of((mx, my, sx, sy))
    assert T[2] == F32(-4) * sx and T[5] == F32(-6) * sy and T[8] == 1
    assert I.norm_point((1, 2), (mx, my, sx, sy)) == (F32(-3) * sx, F32(-4) * sy)


def well_conditioned_sets():
    for seed in range(60, 68):
        sc = Scene(N=8, seed=seed, noise=0.0, extra1=0, extra2=0)
        m1 = [i for i in range(sc.n1) if sc.matches12[i] >= 0]
        n1, n2 = I.normalize(sc.keys1), I.normalize(sc.keys2)
        yield ([I.norm_point(sc.keys1[i], n1) for i in m1],
               [I.norm_point(sc.keys2[sc.matches12[i]], n2) for i in m1])


def f_system(p1, p2):
    return np.array([[u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1] for (u1, v1), (u2, v2) in zip(p1, p2)],
                    np.float64)


def f_deviation():
    norm = ann = null = 0.0
    for p1, p2 in well_conditioned_sets():
        A = f_system(p1, p2)
        At = [[F32(v) for v in row] for row in A] + [[F32(0)] * 9]
        Vt = [[F32(0)] * 8 for _ in range(8)]
        stats = {}
        I.jacobi_svd(At, Vt, 9, 8, 9, stats)
        assert not stats                                    # no row i < n refilled: row 8 is the fill-in alone
        row = np.array(At[8], np.float64)
        nv = np.linalg.svd(A)[2][8]
        norm = max(norm, abs(np.linalg.norm(row) - 1))
        ann = max(ann, np.abs(A.dot(row)).max() / np.linalg.norm(A, 2))
        null = max(null, min(np.abs(row - nv).max(), np.abs(row + nv).max()))
    return norm, ann, null


def test_f21_fill_in_row_is_the_null_vector():
    norm, ann, null = f_deviation()
    print("measured", norm, ann, null)
    assert norm <= 4 * MEASURED_F_NORM and ann <= 4 * MEASURED_F_ANNIHILATE and null <= 4 * MEASURED_F_NULL


def h_deviation():
    dev = 0.0
    for p1, p2 in well_conditioned_sets():
        h = np.array(I.compute_h21(p1, p2), np.float64)
        rows = []
        for (u1, v1), (u2, v2) in zip(p1, p2):
            rows.append([0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2])
            rows.append([u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2])
        nv = np.linalg.svd(np.array(rows, np.float64))[2][8]
        dev = max(dev, min(np.abs(h - nv).max(), np.abs(h + nv).max()))
    return dev


def test_h21_against_numpy():
    dev = h_deviation()
    print("measured", dev)
    assert dev <= 4 * MEASURED_H_NULL


def svd3_deviation():
    rng = np.random.default_rng(3)
    dev = 0.0
    for _ in range(12):
        M = rng.normal(size=(3, 3)).astype(F32)
        w, u, vt = I.svd3([F32(v) for v in M.reshape(9)])
        w64, U, V = np.array(w, np.float64), np.array(u, np.float64).reshape(3, 3), np.array(vt, np.float64).reshape(3, 3)
        sv = np.linalg.svd(M.astype(np.float64), compute_uv=False)
        dev = max(dev, np.abs((U * w64) @ V - M).max() / sv[0], np.abs(w64 - sv).max() / sv[0])
    return dev


def test_svd3_against_numpy():
    dev = svd3_deviation()
    print("measured", dev)
    assert dev <= 4 * MEASURED_SVD3


def test_rng_and_small_rules():
    s = I.rng_next(0x12345678)
    assert s == 0x12345678 * 4164903690 and I.rng_next(s) == ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32))
    M = [F32(v) for v in (2, 0, 1, 0, 4, 3, 0, 0, 1)]
    assert I.det3_d(M) == 8.0
    inv = np.array(I.inv3(M), np.float64).reshape(3, 3)
    assert np.allclose(inv @ np.array(M, np.float64).reshape(3, 3), np.eye(3), atol=1e-7)
    assert I.inv3([F32(0)] * 9) == [F32(0)] * 9             # a singular matrix inverts to zeros
    assert I.key_value(I.order_key(F32(-0.0))).view(np.uint32) == 0x80000000
    keys = [I.order_key(F32(v)) for v in (-np.inf, -1.5, -0.0, 0.0, 1e-30, 2.0, np.inf)]
    assert keys == sorted(keys) and len(set(keys)) == 7


def pose_deviation():
    rot = trans = 0.0
    for seed in range(70, 74):
        sc = Scene(N=90, seed=seed, noise=0.0)
        r = I.initialize(sc.keys1, sc.keys2, sc.matches12, sc.k, 1.0, draws(sc.N, 6, seed))
        assert r.ok and r.model == I.MODEL_F
        rot = max(rot, float(np.abs(r.R21.reshape(3, 3) - sc.R).max()))
        trans = max(trans, float(np.abs(r.t21 - sc.t / np.linalg.norm(sc.t)).max()))
        assert r.vbTriangulated.sum() >= 0.9 * sc.N and not r.vbTriangulated[sc.matches12 < 0].any()
    return rot, trans


def test_initialize_recovers_the_true_pose_without_noise():
    rot, trans = pose_deviation()
    print("measured", rot, trans)
    assert rot <= 4 * MEASURED_ROT and trans <= 4 * MEASURED_TRANS


def test_scenes_cover_the_branches():
    res = {n: reference(n) for n in CASES}
    reached = set().union(*(r.branches for r in res.values()))
    # each return false, both models, both depth gates, the isfinite gate, both flags
    assert reached >= {"too_few", "no_model", "h_degenerate", "h_reject", "f_reject", "f_low_parallax", "model_h",
                       "model_f", "depth1", "depth2", "nonfinite", "reproj1", "reproj2", "ngood0", "size_minus_1",
                       "index_50", "pass_high_cos"}
    assert res["n7"].flags == I.FLAG_TOO_FEW and res["sigma0"].flags == I.FLAG_NO_MODEL
    assert np.isnan(res["sigma0"].RH) and res["sigma0"].model == I.MODEL_F   # NaN > 0.40 is false: the F branch
    assert res["general"].ok and res["general"].model == I.MODEL_F
    assert res["planar"].ok and res["planar"].model == I.MODEL_H and res["planar"].RH > 0.40
    assert not res["rotation"].ok and not res["rotation_noisy"].ok and not res["low_parallax"].ok
    assert res["low_parallax"].candidate >= 0 and 0 < res["low_parallax"].parallax < 1
    assert res["duplicated"].stats.get("refill", 0) >= 1      # the fill-in of a row i < n
    assert all(r.stats.get("refill", 0) == 0 for n, r in res.items() if n != "duplicated")
    assert res["outliers"].mask_f.sum() < res["outliers"].N
    sim = res["similar"]
    assert sim.model == I.MODEL_H and sorted(sim.n_good)[-2] >= 0.75 * max(sim.n_good)
    assert {r.N for r in res.values()} >= {7, 8, 9, 63, 64, 65}
    assert all(r.N <= 130 and r.n_hyp <= 16 for r in res.values())
    sc, _ = case("unmatched")
    assert sc.n1 - sc.N == 60 and sc.n2 - sc.N == 45
    sub = I.normalize(sc.keys1[sc.matches12 >= 0])
    assert sub != I.normalize(sc.keys1)                        # Normalize sees the unmatched keys
    for n, r in res.items():                                   # the sets of N = 8 are the whole list
        if r.N == 8:
            assert all(sorted(s) == list(range(8)) for s in r.sets)


def rows_of(r, n1):
    words = max((r.N + 63) // 64, 0)

    def mask(m):
        out = []
        for w in range(words):
            bits = m[64 * w:64 * w + 64]
            out.append("%016x" % sum(1 << i for i, b in enumerate(bits) if b))
        return " ".join(out)

    def fl(v):
        return " ".join(bits32(x) for x in np.asarray(v, F32).reshape(-1))

    return [" ".join(str(int(v)) for v in (r.flags, r.ok, r.model, r.best_h, r.best_f, r.n_motions, r.candidate,
                                           r.motion, r.stats.get("refill", 0))),
            fl([r.SH, r.SF, r.RH, r.parallax]), fl(r.score_h), fl(r.score_f), fl(r.H21), fl(r.F21),
            mask(r.mask_h), mask(r.mask_f), " ".join(str(int(v)) for v in r.n_good), fl(r.cos), fl(r.R21), fl(r.t21),
            fl(r.vP3D), " ".join(str(int(v)) for v in r.vbTriangulated)]


def same_row(got, want):
    """Equal token by token; two floats also when both are NaN."""
    g, w = got.split(), want.split()
    if len(g) != len(w):
        return False
    for a, b in zip(g, w):
        if a != b:
            if len(a) != 8 or len(b) != 8:
                return False
            x = np.array([int(a, 16), int(b, 16)], np.uint32).view(F32)
            if not (np.isnan(x[0]) and np.isnan(x[1])):
                return False
    return True


def test_core_header_on_the_host_matches_the_restatement_under_sanitizers(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "build", "initializer_core_main")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "tests", "cpp", "hipstub"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "initializer_core_main.cpp")], check=True)
    names = list(CASES)
    problems = []
    for n in names:
        sc, d = case(n)
        problems.append((sc.keys1, sc.keys2, sc.matches12, sc.k, sc.sigma, d))
    path = tmp_path / "problems.txt"
    dump(str(path), problems)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    rows = out.stdout.split("\n")
    assert len(rows) >= 14 * len(names)
    for i, n in enumerate(names):
        want = rows_of(reference(n), case(n)[0].n1)
        got = rows[14 * i:14 * i + 14]
        for j, (g, w) in enumerate(zip(got, want)):
            assert same_row(g, w), (n, j, g[:200], w[:200])
