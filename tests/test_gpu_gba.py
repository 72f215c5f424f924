"""Global BundleAdjustment on the GPU (include/orbfe_gba.h) against tests/gba_ref.py: every value compared
with == on its bits (NaN equal to NaN), nothing excused -- no transcendental and no unordered reduction
runs on either side.

Per scene: the poses as float bits, the points, and every field of the trace with lambda and chi2 as
double bits. The scenes are tests/gba_scenes.CASES; tests/test_gba_ref.py checks on the restatement alone
that each takes the branch it is named for."""
import numpy as np
import pytest

import gba_ref as G
from gba_scenes import CASES, case

pytestmark = pytest.mark.gpu

ref = G.solve_case


def same_bits(got, want, what):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(np.asarray(want, got.dtype).reshape(got.shape))
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    eq = got.view(u) == want.view(u)
    eq |= np.isnan(got) & np.isnan(want)
    assert eq.all(), (what, got[~eq], want[~eq])


def check(name, g, r):
    t = r.trace
    want = dict(n_active=t.n_active, iterations=t.iterations, trials=t.trials, rejected_trials=t.rejected_trials, stop=t.stop,
                env_blocks=r.env_blocks, schur_blocks=r.schur_blocks, flags=r.flags, polls=r.polls)
    for field, v in want.items():
        print(name, field, getattr(g, field), v)
        assert getattr(g, field) == v, (name, field)
    print(name, "lambda, chi2", g.lam, g.chi2)
    same_bits(np.array([g.lam, g.chi2]), np.array([t.lam, t.chi2]), name + " lambda, chi2")
    same_bits(g.tcw, r.tcw, name + " tcw")
    same_bits(g.xw, r.xw, name + " xw")


def adjuster_for(*problems):
    from orb_slam2_2021_amd import GlobalBundleAdjuster
    return GlobalBundleAdjuster(max(p.n_kf for p in problems), max(p.n_points for p in problems),
                                max(p.n_edges for p in problems), max(max(G.plan_counts(p)[0] for p in problems), 1))


@pytest.mark.parametrize("name", list(CASES))
def test_one_scene(name):
    p = case(name)
    adj = adjuster_for(p)
    check(name, adj.solve(p), ref(name))
    adj.close()


def test_two_scenes_alternating_on_one_handle():
    """a stale envelope or a stale plan would show: loop's envelope is wider than chain's, orphan_kf's
    slots differ from both"""
    a, b, c = case("loop"), case("chain"), case("orphan_kf")
    adj = adjuster_for(a, b, c)
    check("loop", adj.solve(a), ref("loop"))
    check("chain", adj.solve(b), ref("chain"))
    check("loop", adj.solve(a), ref("loop"))
    check("orphan_kf", adj.solve(c), ref("orphan_kf"))
    check("chain", adj.solve(b), ref("chain"))
    adj.close()


def test_global_bundle_adjustment_on_keyframes():
    """GlobalBundleAdjustment(...) over the package's KeyFrame class: the gather, the write-back and the
    points not included, against the restatement on the gathered problem; a bad keyframe, a bad point and
    an unobserved point in the input"""
    from orb_slam2_2021_amd import KEYPOINT_DTYPE, GlobalBundleAdjustment, KeyFrame, problem_of_map
    p = case("loop")
    ids = [0, 2, 3, 5, 8, 9, 11, 12, 14, 17, 20, 21]  # mnId per scene keyframe
    sigma2 = np.array([1.2 ** (2 * l) for l in range(8)], np.float32)
    inv = np.float32(1.0) / sigma2
    kfs, obs = {}, {}

    def keyframe(i, edges):
        keys = np.zeros(len(edges), KEYPOINT_DTYPE)
        keys["x"], keys["y"] = p.kp_un[edges, 0], p.kp_un[edges, 1]
        keys["octave"] = [int(np.argmin(np.abs(inv - v))) for v in p.inv_sigma2[edges]]
        return KeyFrame(keys_un=keys, descriptors=np.zeros((len(edges), 32), np.uint8), u_right=p.u_right[edges].copy(),
                        mp_state=np.zeros(len(edges), np.uint8), scale_factors=np.sqrt(sigma2), level_sigma2=sigma2,
                        fx=float(p.k[i, 0]), fy=float(p.k[i, 1]), cx=float(p.k[i, 2]), cy=float(p.k[i, 3]),
                        bf=float(p.bf[i]), tcw=p.tcw[i].reshape(3, 4).copy())

    for kid, i in zip(ids, range(p.n_kf)):
        edges = np.flatnonzero(p.edge_kf == i)
        kfs[kid] = keyframe(i, edges)
        for j, e in enumerate(edges):
            pt = int(np.searchsorted(p.edge_begin, e, side="right") - 1)
            obs.setdefault(100 + 2 * pt, {})[kid] = j
    points = {100 + 2 * pt: p.xw[pt].copy() for pt in range(p.n_points)}
    # a bad keyframe that observes the first three points: neither a vertex nor an edge
    kfs[6] = keyframe(3, np.flatnonzero(p.edge_kf == 3))
    kfs[6].bad = True
    for pt in range(3):
        obs[100 + 2 * pt][6] = 0
    points[51] = None  # a bad point
    obs[51] = {0: 0, 2: 0}
    points[999] = np.array([0.3, 0.2, 7.0], np.float32)  # no observation: not included
    gathered = problem_of_map(kfs, points, obs, n_iterations=7, robust=True)
    assert gathered.kf_ids == ids and list(gathered.fixed) == [1] + [0] * 11
    assert gathered.point_ids == sorted(100 + 2 * pt for pt in range(p.n_points)) + [999]
    assert gathered.n_edges == p.n_edges and gathered.n_iterations == 7
    want = G.solve(gathered)
    assert want.trace.iterations > 0 and want.env_blocks > want.schur_blocks
    before = {kid: np.array(kf.tcw, np.float32).copy() for kid, kf in kfs.items()}
    not_included = GlobalBundleAdjustment(kfs, points, obs, n_iterations=7)
    assert not_included == [999] and points[51] is None
    same_bits(np.asarray(points[999], np.float32), np.array([0.3, 0.2, 7.0], np.float32), "the unobserved point")
    same_bits(np.asarray(kfs[6].tcw, np.float32), before[6], "the bad keyframe")
    for i, kid in enumerate(gathered.kf_ids):
        same_bits(np.asarray(kfs[kid].tcw, np.float32).reshape(12), want.tcw[i], "tcw of %d" % kid)
    for i, pid in enumerate(gathered.point_ids):
        same_bits(np.asarray(points[pid], np.float32), want.xw[i], "point %d" % pid)
