"""GPU parity of the batched Sim3Solver (k_sim3_hypotheses + k_sim3_inliers + k_sim3_select,
liborbfe.so) against tests/sim3_ref.py, the reference's Sim3Solver.cc restated in Python.

Everything is exact. Per hypothesis: R, t, s, T12, T21 bit-equal (NaN equal to NaN), the inlier
count and the inlier mask. Per solver: the outcome of find() and every iterate(5) step.

The one excuse: atan2 / cos / sin run in double before a narrowing to float, and the device's math
library may differ from the host's in the last bit of the double. A hypothesis whose floats differ
is excused only if one of the restatement's pre-narrowing doubles lies within 2 double-ulps of a
float rounding midpoint; it is then skipped for the inlier comparison and named in the output. At
most 1 hypothesis in 10,000 of a run may be excused (test_excused_budget, last in this file).

Shapes: N = 3 (one iteration), 6, 63 / 64 / 65 (the wavefront chunk of the mask), 300 x 300
hypotheses; both fix_scale values; draws that collide in the swap-remove; degenerate triples."""
import numpy as np
import pytest

from orb_slam2_2021_amd import ORBmatcher, Sim3Batch, Sim3Solver, solve_batch
from orb_slam2_2021_amd import synthetic as S

import sim3_ref as R
from sim3_scenes import COLLISION_DRAWS, K_KITTI, K_OTHER, Scene, draws, quirk_inputs

pytestmark = pytest.mark.gpu

COMPARED = [0]   # hypotheses compared in this run
EXCUSED = []     # (tag, hypothesis) excused by the midpoint rule


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    b = np.ascontiguousarray(b, np.float32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na],
                                                                            b.view(np.uint32)[~nb])


def near_float_midpoint(d):
    """Is the double d within 2 double-ulps of the midpoint of two adjacent floats?"""
    if not np.isfinite(d):
        return False
    f = np.float32(d)
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    mids = [(float(lo) + float(f)) / 2, (float(f) + float(hi)) / 2]
    return min(abs(d - m) for m in mids) <= 2 * float(np.spacing(np.float64(d)))


def make_pair(sc, fix_scale, min_inliers, max_iterations, rand_idx, probability=0.99, hyp=None):
    g = Sim3Solver(sc.x1, sc.x2, sc.sigma2_1, sc.sigma2_2, sc.k1, sc.k2, fix_scale)
    g.SetRansacParameters(probability, min_inliers, max_iterations)
    r = R.Sim3Solver(sc.x1, sc.x2, sc.sigma2_1, sc.sigma2_2, sc.k1, sc.k2, fix_scale)
    r.set_ransac_parameters(probability, min_inliers, max_iterations)
    if rand_idx is not None:
        g.set_draws(rand_idx)
        r.evaluate(rand_idx)
    return g, r


def compare(g, r, tag):
    """Per hypothesis, then find(), then every iterate(5) step. -> hypotheses excused"""
    assert g.n_evaluated == len(r.hyp), tag
    if r.N >= r.min_inliers:
        assert g.mRansacMaxIts == r.max_its, tag
    excused = []
    for k, h in enumerate(r.hyp):
        COMPARED[0] += 1
        same = (bits_equal(g.r12[k], h["R"]) and bits_equal(g.tr12[k], h["t"]) and bits_equal(g.s12[k], h["s"])
                and bits_equal(g.t12[k], h["T12"]) and bits_equal(g.t21[k], h["T21"]))
        if not same:
            if any(near_float_midpoint(float(d)) for d in h["dbl"]):
                print(f"EXCUSED {tag} hypothesis {k}: a pre-narrowing double sits on a float midpoint")
                EXCUSED.append((tag, k))
                excused.append(k)
                continue
            raise AssertionError(f"{tag} hypothesis {k} (samples {h['idx']}): R {g.r12[k].ravel()} vs "
                                 f"{h['R'].ravel()}, t {g.tr12[k]} vs {h['t']}, s {g.s12[k]} vs {h['s']}")
        assert int(g.n_inliers[k]) == h["count"], (tag, k, int(g.n_inliers[k]), h["count"])
        assert np.array_equal(g.inliers_of(k), h["inliers"]), (tag, k)
    if excused:
        return excused
    counts = r.counts()
    acc, n_in, best, best_in, no_more = R.find_counts(counts, r.N, r.min_inliers, r.max_its)
    assert g.found == dict(accepted=acc, nInliers=n_in, best=best, mnBestInliers=best_in, bNoMore=no_more), tag
    state = [0, 0, -1]
    for step in range(len(counts) // 5 + 2):
        T, g_no_more, g_inl, g_n = g.iterate(5)
        w_acc, w_no_more, w_n = R.iterate_counts(counts, r.N, r.min_inliers, r.max_its, 5, state)
        assert (T is not None) == (w_acc >= 0) and g_no_more == w_no_more and g_n == w_n, (tag, step)
        if w_acc >= 0:
            assert bits_equal(T[:3], r.hyp[w_acc]["T12"]) and np.array_equal(T[3], [0, 0, 0, 1]), (tag, step)
            assert np.array_equal(g_inl, r.hyp[w_acc]["inliers"]), (tag, step)
            assert bits_equal(g.GetEstimatedRotation(), r.hyp[w_acc]["R"])
            assert bits_equal(g.GetEstimatedTranslation(), r.hyp[w_acc]["t"])
            assert bits_equal(g.GetEstimatedScale(), r.hyp[w_acc]["s"])
        else:
            assert not g_inl.any(), (tag, step)
        assert (g._state.iterations, g._state.best_inliers, g._state.best) == tuple(state), (tag, step)
        if w_acc >= 0 or w_no_more or state[0] >= len(counts):
            break
    return excused


@pytest.fixture(scope="module")
def batch(require_gpu):
    b = Sim3Batch(max_solvers=4, max_corr=320, max_hyp=300)
    yield b
    b.close()


# ---- sizes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n,min_inliers,n_hyp", [(3, 3, 5), (6, 4, 20), (63, 20, 40), (64, 20, 40), (65, 20, 40)])
def test_sizes(batch, n, min_inliers, n_hyp, fix_scale):
    sc = Scene(n, seed=100 + n, scale=1.0 if fix_scale else 1.15, outlier_frac=0.3 if n > 6 else 0.0,
               k2=K_OTHER)
    g, r = make_pair(sc, fix_scale, min_inliers, 300, draws(n, n_hyp, seed=n))
    batch.solve([g])
    compare(g, r, f"n={n} fix_scale={fix_scale}")
    if n == 3:
        assert g.n_evaluated == 1 and g.mRansacMaxIts == 1  # minInliers == N: one iteration
    # bits past N in the last mask word are clear
    if g.n_evaluated and n % 64:
        assert not (g.inlier_words[:, -1] >> np.uint64(n % 64)).any()


def test_300_correspondences_300_hypotheses(batch):
    # 66 consistent correspondences against minInliers 73 (epsilon 0.243: mRansacMaxIts is capped at
    # 300): find() never stops early, so all 300 hypotheses matter to the best and to bNoMore
    sc = Scene(300, seed=7, scale=0.9, outlier_frac=0.78)
    g, r = make_pair(sc, False, 73, 300, draws(300, 300, seed=8))
    batch.solve([g])
    assert g.n_evaluated == 300 and g.mRansacMaxIts == 300
    compare(g, r, "n=300")
    assert g.found["accepted"] == -1 and g.found["bNoMore"] and g.found["mnBestInliers"] > 50


def test_fewer_correspondences_than_min_inliers(batch):
    sc = Scene(10, seed=9)
    g, r = make_pair(sc, False, 20, 300, draws(10, 30, seed=1))
    batch.solve([g])
    assert g.n_evaluated == 0 and r.hyp == []
    assert g.found == dict(accepted=-1, nInliers=0, best=-1, mnBestInliers=0, bNoMore=True)
    T, no_more, inl, n_in = g.iterate(5)
    assert T is None and no_more and n_in == 0 and not inl.any()
    T, inl, n_in = g.find()
    assert T is None and n_in == 0


# ---- sample selection -------------------------------------------------------------------------------
def test_swap_remove_collision_draws(batch):
    sc = Scene(6, seed=21, scale=1.05)
    names = sorted(COLLISION_DRAWS)
    rand_idx = np.array([COLLISION_DRAWS[k][0] for k in names], np.int32)
    g, r = make_pair(sc, False, 6, 300, None)
    # minInliers == N would give one iteration: use 5 so that all four triples run
    g.SetRansacParameters(0.99, 5, 300)
    r.set_ransac_parameters(0.99, 5, 300)
    g.set_draws(rand_idx)
    r.evaluate(rand_idx)
    batch.solve([g])
    assert g.n_evaluated == len(names)
    for k, name in enumerate(names):
        assert r.hyp[k]["idx"] == COLLISION_DRAWS[name][1]
    compare(g, r, "collisions")


# ---- threshold truncation ------------------------------------------------------------------------------
@pytest.mark.parametrize("err_sq,inlier", [(13.1, False), (12.9, True)])
def test_truncated_threshold(batch, err_sq, inlier):
    x1, x2, sig, k, eye = quirk_inputs(err_sq)
    g = Sim3Solver(x1, x2, sig, sig, k, k, True)
    g.SetRansacParameters(0.99, 2, 300)
    g.set_hypotheses(eye[None], eye[None])
    batch.solve([g])
    r = R.Sim3Solver(x1, x2, sig, sig, k, k, True)
    want = r.check_inliers(eye, eye)
    assert bool(want[0]) is inlier
    assert np.array_equal(g.inliers_of(0), want) and int(g.n_inliers[0]) == int(want.sum())


# ---- a synthetic loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("fix_scale", [False, True])
def test_synthetic_loop(batch, fix_scale):
    sc = Scene(100, seed=31, scale=1.0 if fix_scale else 1.2, outlier_frac=0.3)
    g, r = make_pair(sc, fix_scale, 20, 300, draws(100, 300, seed=32))
    batch.solve([g])
    excused = compare(g, r, f"loop fix_scale={fix_scale}")
    acc = g.found["accepted"]
    assert acc >= 0 and g.found["nInliers"] > 20
    if not excused:
        assert np.array_equal(g.inliers_of(acc), r.hyp[acc]["inliers"])
    assert not np.any(g.inliers_of(acc) & ~sc.consistent)
    assert abs(float(g.s12[acc]) - sc.s) < 0.05


# ---- degenerate triples ------------------------------------------------------------------------------
def test_degenerate_triples(batch):
    sc = Scene(12, seed=41, scale=1.1)
    sc.x1[1] = sc.x1[0]                       # two coincident points (both sets)
    sc.x2[1] = sc.x2[0]
    sc.x1[4] = 2 * sc.x1[3] - sc.x1[2]        # three collinear points
    sc.x2[4] = 2 * sc.x2[3] - sc.x2[2]
    sc.x1[5, 2] = 0.0                         # a point with z = 0
    sc.x2[6, 2] = 0.0
    sc.x1[8] = sc.x2[8]                       # identical triples: the quaternion has no imaginary part
    sc.x1[9] = sc.x2[9]
    sc.x1[10] = sc.x2[10]
    sc.x1[11] = np.nan
    # draws that select (0, 1, 7), (2, 3, 4), (5, 6, 7), (8, 9, 10), (11, 0, 7) and an ordinary triple
    # (10 has moved to slot 9 by the third draw of the fourth row)
    rand_idx = np.array([[0, 1, 7], [2, 3, 4], [5, 6, 7], [8, 9, 9], [11, 0, 7], [7, 2, 0]], np.int32)
    for row, want in zip(rand_idx, [[0, 1, 7], [2, 3, 4], [5, 6, 7], [8, 9, 10], [11, 0, 7], [7, 2, 0]]):
        assert R.select3(12, row) == want
    for fix_scale in (False, True):
        g, r = make_pair(sc, fix_scale, 4, 300, rand_idx)
        batch.solve([g])  # returns: the Jacobi loop is capped
        compare(g, r, f"degenerate fix_scale={fix_scale}")
        for k, h in enumerate(r.hyp):
            if np.isnan(h["T12"]).any():
                assert int(g.n_inliers[k]) == 0 and not g.inliers_of(k).any()
        assert np.isnan(r.hyp[4]["T12"]).any() and np.isnan(g.t12[4]).any()


# ---- batches ---------------------------------------------------------------------------------------
def three_solvers():
    specs = [(Scene(40, seed=51, scale=1.1, outlier_frac=0.2), False, 12, 60),
             (Scene(130, seed=52, outlier_frac=0.4, k2=K_OTHER), True, 20, 25),
             (Scene(7, seed=53, scale=0.8), False, 4, 9)]
    return [make_pair(sc, fs, mi, 300, draws(sc.n, nh, seed=sc.n)) for sc, fs, mi, nh in specs]


def snapshot(g):
    return [a.copy() for a in (g.n_inliers, g.t12, g.t21, g.r12, g.tr12, g.s12, g.inlier_words)] + [dict(g.found)]


def same_snapshot(a, b):
    return all(bits_equal(x, y) if getattr(x, "dtype", None) == np.float32 else
               (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y) for x, y in zip(a, b))


def test_batch_of_three_equals_one_by_one(batch):
    pairs = three_solvers()
    batch.solve([g for g, _ in pairs])
    together = [snapshot(g) for g, _ in pairs]
    for i, (g, r) in enumerate(pairs):
        compare(g, r, f"batch solver {i}")
    # one inactive solver (n < minInliers) in the middle does not shift the others
    idle, _ = make_pair(Scene(5, seed=54), False, 20, 300, draws(5, 4, seed=1))
    batch.solve([pairs[0][0], idle, pairs[1][0], pairs[2][0]])
    assert idle.n_evaluated == 0 and idle.found["bNoMore"]
    for (g, _), want in zip(pairs, together):
        assert same_snapshot(snapshot(g), want)
    for (g, _), want in zip(pairs, together):
        batch.solve([g])
        assert same_snapshot(snapshot(g), want)


def test_back_to_back_batches_equal_fresh_handles(batch):
    first = three_solvers()
    second = [make_pair(Scene(90, seed=61, outlier_frac=0.3), False, 20, 300, draws(90, 50, seed=2)),
              make_pair(Scene(20, seed=62), True, 8, 300, draws(20, 30, seed=3))]
    batch.solve([g for g, _ in first])
    batch.solve([g for g, _ in second])       # a smaller batch over the first one's buffers
    reused = [snapshot(g) for g, _ in second]
    batch.solve([g for g, _ in first])
    reused_first = [snapshot(g) for g, _ in first]
    for pairs, got in ((second, reused), (first, reused_first)):
        fresh = solve_batch([g for g, _ in pairs])
        for (g, _), want in zip(pairs, got):
            assert same_snapshot(snapshot(g), want)
        fresh.close()
    # a solver replays only the solve it took part in
    batch.solve([first[0][0]])
    stale = second[0][0]
    stale._batch, stale._epoch = batch, batch.epoch - 1
    with pytest.raises(RuntimeError):
        stale.iterate(5)


def test_caller_supplied_hypotheses(batch):
    sc = Scene(70, seed=71, scale=1.1, outlier_frac=0.3)
    g, r = make_pair(sc, False, 20, 300, draws(70, 40, seed=72))
    t12 = np.stack([h["T12"] for h in r.hyp])
    t21 = np.stack([h["T21"] for h in r.hyp])
    g.set_hypotheses(t12, t21)
    batch.solve([g])
    assert g.n_evaluated == len(r.hyp)
    for k, h in enumerate(r.hyp):
        assert bits_equal(g.t12[k], h["T12"]) and bits_equal(g.t21[k], h["T21"])
        assert bits_equal(g.tr12[k], h["T12"][:, 3])
        assert int(g.n_inliers[k]) == h["count"] and np.array_equal(g.inliers_of(k), h["inliers"]), k
    acc, n_in, best, best_in, no_more = R.find_counts(r.counts(), r.N, r.min_inliers, r.max_its)
    assert g.found == dict(accepted=acc, nInliers=n_in, best=best, mnBestInliers=best_in, bNoMore=no_more)


# ---- the chain: solver -> SearchBySim3 ---------------------------------------------------------------
def test_chain_into_search_by_sim3(batch):
    rng = np.random.default_rng(81)
    sc = S.make_keyframe_scene(rng, n_points=300, n_clutter=100)
    # the constructor's filter: KF1 keypoints with a MapPoint that KF2 observes too
    kp2_of_point = {int(p): i for i, p in enumerate(sc.point_of_kp2) if p >= 0}
    i1 = [i for i, p in enumerate(sc.point_of_kp1) if p >= 0 and int(p) in kp2_of_point]
    i2 = [kp2_of_point[int(sc.point_of_kp1[i])] for i in i1]
    Xw = sc.world[sc.point_of_kp1[i1]].astype(np.float64)
    x1 = (Xw @ sc.kf1.tcw[:, :3].T.astype(np.float64) + sc.kf1.tcw[:, 3]).astype(np.float32)
    x2 = (Xw @ sc.kf2.tcw[:, :3].T.astype(np.float64) + sc.kf2.tcw[:, 3]).astype(np.float32)
    sig1 = sc.kf1.level_sigma2[sc.kf1.keys_un["octave"][i1]]
    sig2 = sc.kf2.level_sigma2[sc.kf2.keys_un["octave"][i2]]
    k = np.array([sc.kf1.fx, sc.kf1.fy, sc.kf1.cx, sc.kf1.cy], np.float32)

    class Corr:
        pass
    c = Corr()
    c.x1, c.x2, c.sigma2_1, c.sigma2_2, c.k1, c.k2, c.n = x1, x2, sig1, sig2, k, k, len(x1)
    assert c.n > 100
    g, r = make_pair(c, False, 20, 300, draws(c.n, 300, seed=82))
    batch_big = Sim3Batch(1, c.n, 300)
    batch_big.solve([g])
    excused = compare(g, r, "chain")
    acc = g.found["accepted"]
    assert acc >= 0 and not excused and g._state.best == acc  # compare()'s iterate(5) steps stopped there
    m = ORBmatcher(0.75, True)
    n_g, m_g = m.SearchBySim3(sc.kf1, sc.kf2, sc.mps1, sc.mps2, g.GetEstimatedScale(), g.GetEstimatedRotation(),
                              g.GetEstimatedTranslation(), 7.5)
    h = r.hyp[acc]
    n_r, m_r = m.SearchBySim3(sc.kf1, sc.kf2, sc.mps1, sc.mps2, float(h["s"]), h["R"], h["t"], 7.5)
    assert n_g == n_r and np.array_equal(m_g, m_r) and n_g > 20
    batch_big.close()


# ---- a handle with no room to spare ---------------------------------------------------------------------
@pytest.mark.parametrize("supplied", [False, True], ids=["draws", "hypotheses"])
def test_handles_filled_to_every_bound(require_gpu, supplied):
    """Two solvers with n == max_corr and n_hyp == max_hyp on a handle made for exactly two: every byte of its
    buffers is planned. Bit for bit what each solver gives alone on a fresh handle with generous bounds."""
    solvers = []
    for seed in (91, 96):
        sc = Scene(65, seed=seed, scale=1.1, outlier_frac=0.1, k2=K_OTHER)
        g, r = make_pair(sc, False, 20, 300, draws(65, 3, seed=seed))
        if supplied:
            g.set_hypotheses(np.stack([h["T12"] for h in r.hyp]), np.stack([h["T21"] for h in r.hyp]))
        solvers.append(g)
    full = Sim3Batch(max_solvers=2, max_corr=65, max_hyp=3)
    full.solve(solvers)
    together = [snapshot(g) for g in solvers]
    full.close()
    assert all(g.n_evaluated == 3 and g.inlier_words.shape == (3, 2) for g in solvers)
    assert all(int(g.n_inliers.max()) > 20 and g.inliers_of(2)[64] for g in solvers)  # bits in both mask words
    for g, want in zip(solvers, together):
        alone = Sim3Batch(max_solvers=4, max_corr=320, max_hyp=300)
        alone.solve([g])
        assert same_snapshot(snapshot(g), want)
        alone.close()


def test_excused_budget():
    """Last: at most 1 hypothesis in 10,000 of this run was excused by the midpoint rule."""
    print(f"compared {COMPARED[0]} hypotheses, excused {len(EXCUSED)}: {EXCUSED}")
    assert len(EXCUSED) * 10000 <= COMPARED[0]
    assert K_KITTI.dtype == np.float32
