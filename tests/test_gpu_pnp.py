"""PnPsolver on the GPU (include/orbfe_pnp.h) against tests/pnp_ref.py: every value compared with ==
on its bits (NaN equal to NaN), nothing excused -- no transcendental runs on the device.

Per hypothesis: R, t as double bits, tcw as float bits, N, the inlier count, the mask, the flags.
Per record: the refined set. Per solver: find() and every iterate(5) step, its state included.
The cases are tests/pnp_scenes.CASES; tests/test_pnp_ref.py checks on the restatement alone that
they cover the branches."""
import functools

import numpy as np
import pytest

import pnp_ref as P
from pnp_scenes import CASES, case

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def ref(name):
    sc, params, d = case(name)
    return P.Solver(sc.p3dw, sc.p2d, sc.sigma2, sc.k, params, d)


def make(name):
    from orb_slam2_2021_amd import PnPsolver
    sc, params, d = case(name)
    s = PnPsolver(sc.p3dw, sc.p2d, sc.sigma2, sc.k)
    s.SetRansacParameters(*params)
    s.set_draws(d)
    return s


def same_bits(got, want, what):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(np.asarray(want, got.dtype).reshape(got.shape))
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    eq = got.view(u) == want.view(u)
    if got.dtype.kind == "f":
        eq |= np.isnan(got) & np.isnan(want)
    assert eq.all(), (what, got, want)


def check_pose(tag, g_r, g_t, g_tcw, g_n, g_flags, g_count, g_inl, h):
    same_bits(g_r.reshape(9), np.array(h.R, np.float64), tag + " R")
    same_bits(g_t, np.array(h.t, np.float64), tag + " t")
    same_bits(g_tcw.reshape(12), h.tcw, tag + " tcw")
    assert int(g_n) == h.N, tag
    assert int(g_flags) == h.flags, tag
    assert int(g_count) == h.count, tag
    assert np.array_equal(g_inl, h.inliers), tag


def check(name, s):
    r = ref(name)
    assert s.mRansacMinInliers == r.min_inliers and s.mRansacMaxIts == r.max_its, name
    same_bits(np.float32(s.mRansacEpsilon).reshape(1), np.float32(r.epsilon).reshape(1), name + " epsilon")
    assert s.n_evaluated == len(r.hyp), name
    for k, h in enumerate(r.hyp):
        check_pose(f"{name} hyp {k}", s.r[k], s.t[k], s.tcw[k], s.n_chosen[k], s.flags[k], s.n_inliers[k],
                   s.inliers_of(k), h)
    assert list(s.records) == r.records, name
    for j, k in enumerate(r.records):
        check_pose(f"{name} record {j}", s.refined_r[j], s.refined_t[j], s.refined_tcw[j], s.refined_n_chosen[j],
                   s.refined_flags[j], s.refined_inliers[j], s.refined_inliers_of(j), r.refined[k])
    assert s.found == r.find(), name
    # every iterate(5) step from a fresh state
    state = [0, 0, -1]
    for _ in range(len(r.hyp) // 5 + 3):
        T, no_more, inl, n_inl = s.iterate(5)
        if not r.launched:
            assert T is None and no_more and n_inl == 0 and not inl.any()
            break
        o = P.iterate_counts(r.counts, r.refined_counts, r.min_inliers, r.max_its, 5, state)
        assert s.last_iterate == o, (name, s.last_iterate, o)
        assert [s._state.iterations, s._state.best_inliers, s._state.best] == state, name
        if o["returned"] == 1:
            want = r.refined[o["accepted"]]
            same_bits(T[:3].reshape(12), want.tcw, name + " iterate tcw")
            assert np.array_equal(inl, want.inliers)
        elif o["returned"] == 2:
            same_bits(T[:3].reshape(12), r.hyp[state[2]].tcw, name + " iterate best tcw")
            assert np.array_equal(inl, r.hyp[state[2]].inliers)
        else:
            assert T is None and not inl.any()
        if no_more or state[0] >= len(r.counts):
            break


@pytest.mark.parametrize("name", [n for n in CASES if n not in ("small",)])
def test_one_solver(name):
    from orb_slam2_2021_amd.pnp_solver import solve_batch
    s = make(name)
    batch = solve_batch([s])
    check(name, s)
    batch.close()


def test_batch_of_three_and_one_unlaunched():
    from orb_slam2_2021_amd import PnPBatch
    names = ["n63", "small", "n5", "refail"]
    solvers = [make(n) for n in names]
    batch = PnPBatch(max_solvers=4, max_corr=64, max_hyp=16)
    batch.solve(solvers)
    assert solvers[1].n_evaluated == 0 and solvers[1].found["no_more"] == 1
    for n, s in zip(names, solvers):
        check(n, s)
    # the same handle again, other solvers at other offsets
    names = ["refail", "n4"]
    solvers = [make(n) for n in names]
    batch.solve(solvers)
    for n, s in zip(names, solvers):
        check(n, s)
    batch.close()


def test_handles_filled_to_every_bound():
    """Two solvers with n == max_corr and n_hyp == max_hyp on a handle made for exactly two: every byte of its
    buffers and of the refinement workspace is planned. Bit for bit what each solver gives alone on a fresh
    handle with generous bounds."""
    from orb_slam2_2021_amd import PnPBatch, PnPsolver
    from pnp_scenes import Scene, draws

    def snapshot(s):
        arrays = (s.n_inliers, s.inlier_words, s.r, s.t, s.tcw, s.n_chosen, s.flags, s.records, s.refined_inliers,
                  s.refined_words, s.refined_r, s.refined_t, s.refined_tcw, s.refined_n_chosen, s.refined_flags)
        return [np.array(a).copy() for a in arrays] + [dict(s.found)]

    solvers = []
    for seed in (43, 44):
        sc = Scene(65, seed=seed, noise=0.3, outliers=0.0)
        s = PnPsolver(sc.p3dw, sc.p2d, sc.sigma2, sc.k)
        s.SetRansacParameters(0.99, 10, 300, 4, 0.3, 5.991)
        s.set_draws(draws(65, 3, seed))
        solvers.append(s)
    full = PnPBatch(max_solvers=2, max_corr=65, max_hyp=3)
    full.solve(solvers)
    together = [snapshot(s) for s in solvers]
    full.close()
    assert all(s.n_evaluated == 3 and s.inlier_words.shape == (3, 2) for s in solvers)
    assert all(s.n_records >= 1 and int(s.refined_inliers.max()) > 19 for s in solvers)  # the workspace was used
    for s, want in zip(solvers, together):
        alone = PnPBatch(max_solvers=4, max_corr=320, max_hyp=300)
        alone.solve([s])
        got = snapshot(s)
        for a, b in zip(got[:-1], want[:-1]):
            assert a.shape == b.shape
            same_bits(a, b, "alone against the full handle")
        assert got[-1] == want[-1]
        alone.close()


def test_find_and_scatter_through_key_point_indices():
    from orb_slam2_2021_amd import PnPsolver
    sc, params, d = case("h24")
    idx = np.arange(sc.n) * 3 + 1
    s = PnPsolver(sc.p3dw, sc.p2d, sc.sigma2, sc.k, key_point_indices=idx, n_keypoints=3 * sc.n + 5)
    s.SetRansacParameters(*params)
    s.set_draws(d)
    T, vb, n_inl = s.find()
    r = ref("h24")
    f = r.find()
    assert f["accepted"] >= 0 and n_inl == f["accepted_inliers"]
    want = np.zeros(3 * sc.n + 5, bool)
    want[idx[r.refined[f["accepted"]].inliers]] = True
    assert np.array_equal(vb, want)
    same_bits(T[:3].reshape(12), r.refined[f["accepted"]].tcw, "find tcw")
    assert np.array_equal(T[3], [0, 0, 0, 1])
