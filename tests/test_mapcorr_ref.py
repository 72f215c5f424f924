"""tests/mapcorr_ref.py pinned on its own (CPU, no library): against float64 definitions on generated maps,
and on hand-built cases whose results are worked here.

Bounds against the float64 definitions, with u = 2^-24 and the inputs (float32) taken as exact. They come
from the operation counts below, not from a run.

update_normal_depth, per component of the normal (|component| <= 1), n observers:
  d = X - O is one rounding (u); cv::norm is double (nothing); a = (float)(1 / nrm) sees the rounded d (u) and
  is narrowed (u); d * a is rounded (u): a term is off by at most 4u. The i-th addition rounds a partial sum of
  size <= i: u n (n + 1) / 2 over the chain. The mean multiplies by (float)(1 / n) (u) and rounds (u).
  |error| <= (4 u n + u n (n + 1) / 2) / n + 2u = (6 + (n + 1) / 2) u; the test allows (7 + (n + 1) / 2) u.
  dist = (float)norm(d): u from d, u from the narrowing; max_dist one product more, min_dist one quotient
  more: relative 3u and 4u; the test allows 3.5u and 4.5u for the second-order terms.

correct_loop, per coordinate of a corrected point, m = 32 a bound on every coordinate along the chain
(|X| <= 13, camera centres within 3.5, scale <= 1.1): a pose's float32 rotation is within u per entry of a
rotation, so Quaterniond(R) acts within 6u m of R (Siw.map); Twc built by transposition is within 10u m of the
inverse (9 entries of R^-1 - R^T at u each, Ow's rounding); the gemm of Tic rounds 4 terms (4u m); Tic's
quaternion, of a product of two such rotations, acts within 8u m; the narrowing is u m. The double
operations are 2^-53 each and do not count. 29u m in CorrectedSiw and Siw together; the inverse similarity
has gain 1 / s <= 1.12: 33u m. The test allows 40u m = 7.7e-5.

apply_gba, per entry of a propagated pose, mt = 16 a bound on a translation entry along the chain: the
transposed inverse (10u mt), two gemms of 4 terms each (8u mt), the parent's own error carried over (linear in
the run length L): 20 L u mt; the test allows 24 L u mt. A point that moves with its reference keyframe:
two gemms with C and the transposed inverse (12u m, m = 16), plus the pose's error on three rotation entries
times |Xc| <= m and one translation entry: the test allows 12u m + 4 m (24 L u mt).
"""
from types import SimpleNamespace

import numpy as np

import mapcorr_ref as R
import mapcorr_scenes as S
from optsim3_ref import sim3_inverse, sim3_map

F32 = np.float32
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def T4(t):
    return np.vstack([np.asarray(t, np.float64).reshape(3, 4), [0, 0, 0, 1]])


def scale_table(n):
    s = [F32(1.0)]
    for _ in range(1, n):
        s.append(s[-1] * F32(1.2))
    return np.array(s, F32)


def points(xw, bad, segs, ref_kf, ref_level, n_levels=8):
    obs_begin = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int32)
    obs_kf = np.array([k for s in segs for k in s], np.int32)
    n = len(segs)
    return SimpleNamespace(n_points=n, n_obs=len(obs_kf), n_levels=n_levels, scale_factors=scale_table(n_levels),
                           xw=np.array(xw, F32).reshape(n, 3), bad=np.array(bad, np.uint8), obs_begin=obs_begin, obs_kf=obs_kf,
                           ref_kf=np.array(ref_kf, np.int32), ref_level=np.array(ref_level, np.int32))


# ---- against float64 definitions ------------------------------------------------------------------------
def test_normals_against_the_mean_of_unit_vectors():
    p = S.normals_problem(1, 12, 120, [0, 1, 2, 3, 5, 8])
    r = R.update_normal_depth(p)
    ow, xw, sc = p.ow.astype(np.float64), p.xw.astype(np.float64), p.scale_factors.astype(np.float64)
    seen = 0
    for i in range(p.n_points):
        b, e = p.obs_begin[i], p.obs_begin[i + 1]
        if p.bad[i] or e == b:
            assert not r.updated[i]
            assert np.array_equal(bits(r.normal[i]), bits(p.normal[i])) and bits(r.max_dist[i]) == bits(p.max_dist[i])
            continue
        d = xw[i] - ow[p.obs_kf[b:e]]
        assert np.linalg.norm(d, axis=1).min() >= 1.0
        want = (d / np.linalg.norm(d, axis=1)[:, None]).mean(0)
        n = e - b
        assert np.abs(r.normal[i].astype(np.float64) - want).max() <= (7 + (n + 1) / 2) * U, (i, n)
        dist = np.linalg.norm(xw[i] - ow[p.ref_kf[i]])
        mx = dist * sc[p.ref_level[i]]
        assert abs(float(r.max_dist[i]) - mx) <= 3.5 * U * mx and abs(float(r.min_dist[i]) - mx / sc[-1]) <= 4.5 * U * mx / sc[-1]
        assert r.updated[i]
        seen += 1
    assert seen > 60


def sim_matrix(s8):
    q = np.asarray(s8[:4], np.float64)
    x, y, z, w = q / np.linalg.norm(q)
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s8[7] * Rm, s8[4:7]
    return M


def test_loop_points_against_similarity_matrices():
    p = S.loop_problem(3, 8, 5, [40, 0, 25], 80, [0, 1, 2, 4])
    r = R.correct_loop(p)
    Mscw, Tcur = sim_matrix(p.scw), T4(p.tcw[p.connected_kf[p.cur]])
    corrected = 0
    for i in range(p.n_points):
        pos = int(r.corrected_by[i])
        if pos < 0:
            assert np.array_equal(bits(r.xw_out[i]), bits(p.xw[i])) and not r.updated[i]
            continue
        Tiw = T4(p.tcw[p.connected_kf[pos]])
        corr = Mscw if pos == p.cur else Tiw @ np.linalg.inv(Tcur) @ Mscw
        want = np.linalg.inv(corr) @ Tiw @ np.append(p.xw[i].astype(np.float64), 1.0)
        assert np.abs(want[:3]).max() < 32 and np.abs(r.xw_out[i].astype(np.float64) - want[:3]).max() <= 40 * U * 32, i
        assert not p.bad[i] and any(i in p.row_point[p.row_begin[k]:p.row_begin[k + 1]] for k in range(pos + 1))
        assert not any(i in p.row_point[p.row_begin[k]:p.row_begin[k + 1]] for k in range(pos))  # the first row that holds it
        corrected += 1
    assert corrected > 30
    # the Sim3 outputs as matrices, and the poses as [R | t / s]
    for pos in range(p.n_connected):
        Tiw = T4(p.tcw[p.connected_kf[pos]])
        assert np.abs(sim_matrix(r.noncorrected_sim3[pos]) - Tiw).max() <= 40 * U * 4
        corr = Mscw if pos == p.cur else Tiw @ np.linalg.inv(Tcur) @ Mscw
        assert np.abs(sim_matrix(r.corrected_sim3[pos]) - corr).max() <= 40 * U * 32
        s = r.corrected_sim3[pos][7]
        assert np.abs(r.tcw_out[pos].reshape(3, 4)[:, 3] - corr[:3, 3] / s).max() <= 40 * U * 32
        assert np.abs(r.tcw_out[pos].reshape(3, 4)[:, :3] - corr[:3, :3] / s).max() <= 40 * U


def test_gba_against_homogeneous_products():
    parent, optimised = S.tree_with_runs(14, [1, 2, 3])
    p = S.gba_problem(4, parent, optimised, 90)
    r = R.apply_gba(p)
    assert r.levels == 4
    L, mt, m = 3, 16.0, 16.0
    pose_tol = 24 * L * U * mt
    want = {}
    for k in range(p.n_kf):  # the chain ascends in index
        want[k] = T4(p.tcw_gba[k]) if optimised[k] else T4(p.tcw[k]) @ np.linalg.inv(T4(p.tcw[parent[k]])) @ want[parent[k]]
        assert np.abs(want[k][:3, 3]).max() < mt
        if optimised[k]:
            assert np.array_equal(bits(r.tcw_out[k]), bits(p.tcw_gba[k])) and not r.propagated[k]
        else:
            assert r.propagated[k] and np.abs(r.tcw_out[k].reshape(3, 4) - want[k][:3]).max() <= pose_tol
    moved = 0
    for i in range(p.n_points):
        if p.bad[i] or (not p.pt_optimised[i] and p.ref_kf[i] < 0):
            assert np.array_equal(bits(r.xw_out[i]), bits(p.xw[i])) and not r.pt_changed[i]
        elif p.pt_optimised[i]:
            assert np.array_equal(bits(r.xw_out[i]), bits(p.xw_gba[i])) and r.pt_changed[i]
        else:
            k = p.ref_kf[i]
            x = np.linalg.inv(want[k]) @ T4(p.tcw[k]) @ np.append(p.xw[i].astype(np.float64), 1.0)
            assert np.abs(r.xw_out[i] - x[:3]).max() <= 12 * U * m + 4 * m * pose_tol and r.pt_changed[i]
            moved += 1
    assert moved > 20


# ---- hand-built cases -----------------------------------------------------------------------------------
def test_one_observer_on_an_axis():
    """The centre at the origin, the point at (0, 0, 5): d = (0, 0, 5), norm 5, a = (float)0.2, 5 * a = 1.00000001
    rounds to 1; n = 1 so the mean multiplies by 1. dist = 5; max_dist = 5 * 1.2^3 in float, min_dist = max_dist /
    1.2^7 in float."""
    p = points([[0, 0, 5]], [0], [[0]], [0], [3])
    p.n_kf, p.ow = 1, np.zeros((1, 3), F32)
    r = R.update_normal_depth(p)
    s = scale_table(8)
    assert r.updated[0] and np.array_equal(bits(r.normal[0]), bits([0, 0, 1]))
    assert bits(r.max_dist[0]) == bits(F32(5) * s[3]) and bits(r.min_dist[0]) == bits((F32(5) * s[3]) / s[7])


def test_a_point_at_an_observers_centre():
    """Observer 0 sits on the point: d = 0, norm 0, 1 / 0 = inf, 0 * inf = NaN in all three components and it stays
    through the second observer and the mean. The reference keyframe is observer 1: finite distances."""
    p = points([[1, 2, 3]], [0], [[0, 1]], [1], [0])
    p.n_kf, p.ow = 2, np.array([[1, 2, 3], [1, 2, 0]], F32)
    r = R.update_normal_depth(p)
    assert r.updated[0] and np.isnan(r.normal[0]).all()
    assert bits(r.max_dist[0]) == bits(F32(3)) and bits(r.min_dist[0]) == bits(F32(3) / scale_table(8)[7])


def test_an_empty_segment_and_a_bad_point_are_left_alone():
    p = points([[0, 0, 5], [0, 0, 6], [0, 0, 7]], [0, 1, 0], [[], [0], [0]], [0, 0, 0], [0, 0, 0])
    p.n_kf, p.ow = 1, np.zeros((1, 3), F32)
    p.normal = np.arange(9, dtype=F32).reshape(3, 3)
    p.max_dist, p.min_dist = np.array([70, 71, 72], F32), np.array([7, 8, 9], F32)
    r = R.update_normal_depth(p)
    assert r.updated.tolist() == [0, 0, 1]
    for i in (0, 1):
        assert np.array_equal(bits(r.normal[i]), bits(p.normal[i]))
        assert bits(r.max_dist[i]) == bits(p.max_dist[i]) and bits(r.min_dist[i]) == bits(p.min_dist[i])
    assert np.array_equal(bits(r.normal[2]), bits([0, 0, 1])) and bits(r.max_dist[2]) == bits(F32(7))


def three_keyframes():
    rng = np.random.default_rng(8)
    tcw = S.poses(rng, 3)
    T = tcw[0].astype(np.float64).reshape(3, 4)
    D = S.rot([0.02, -0.03, 0.01])
    scw = np.concatenate([S.quat(D @ T[:, :3]), 1.08 * (D @ T[:, 3]) + [0.2, -0.1, 0.3], [1.08]])
    return tcw, scw


def test_the_first_keyframe_in_list_order_corrects_a_shared_point():
    """Keyframes 0, 1, 2 are connected and the tie keys reverse the mnIds: the list is 2, 1, 0. Point 0 is in
    all three rows: position 0 (keyframe 2) corrects it, with keyframe 2's two Sim3."""
    tcw, scw = three_keyframes()
    p = points([[0.5, -0.2, 8.0]], [0], [[0, 1, 2]], [0], [2])
    p.n_kf, p.tcw, p.n_connected, p.connected_kf, p.cur, p.scw = 3, tcw, 3, np.array([2, 1, 0], np.int32), 2, scw
    p.n_slots, p.row_begin, p.row_point = 5, np.array([0, 2, 3, 5], np.int32), np.array([-1, 0, 0, 0, 0], np.int32)
    r = R.correct_loop(p)
    assert r.corrected_by.tolist() == [0] and r.updated[0]
    flat = lambda s: (list(s[:4]), list(s[4:7]), s[7])
    c = sim3_map(sim3_inverse(flat(r.corrected_sim3[0])), sim3_map(flat(r.noncorrected_sim3[0]), [float(v) for v in p.xw[0]]))
    assert np.array_equal(bits(r.xw_out[0]), bits(c))
    other = sim3_map(sim3_inverse(flat(r.corrected_sim3[1])), sim3_map(flat(r.noncorrected_sim3[1]), [float(v) for v in p.xw[0]]))
    assert np.abs(np.array(other) - np.array(c)).max() < 1e-4  # the same correction up to rounding, whoever applies it
    assert np.array_equal(r.corrected_sim3[2], scw)  # the current keyframe's entry is mg2oScw itself


def test_the_timing_of_update_normal_and_depth_inside_the_loop():
    """The list is keyframes 0, 1, 2 and point 0 sits only in keyframe 1's row: it is corrected at position 1.
    Its observers are keyframe 0 (position 0: SetPose has run, the new centre counts) and keyframe 2 (position 2:
    still its old centre); the reference keyframe is keyframe 1 itself (old centre). Swapping old and new gives
    other bits."""
    tcw, scw = three_keyframes()
    p = points([[0.5, -0.2, 8.0]], [0], [[0, 2]], [1], [1])
    p.n_kf, p.tcw, p.n_connected, p.connected_kf, p.cur, p.scw = 3, tcw, 3, np.array([0, 1, 2], np.int32), 0, scw
    p.n_slots, p.row_begin, p.row_point = 1, np.array([0, 0, 1, 1], np.int32), np.array([0], np.int32)
    r = R.correct_loop(p)
    assert r.corrected_by.tolist() == [1] and r.updated[0]
    old = [R.centre(tcw[k]) for k in range(3)]
    new = [R.centre(r.tcw_out[k]) for k in range(3)]
    assert max(abs(float(a) - float(b)) for a, b in zip(old[0], new[0])) > 0.01
    s = scale_table(8)
    with np.errstate(all="ignore"):
        n, mx, mn = R.normal_and_depth(r.xw_out[0], [new[0], old[2]], old[1], s[1], s[7])
        swapped = R.normal_and_depth(r.xw_out[0], [old[0], new[2]], new[1], s[1], s[7])
    assert np.array_equal(bits(r.normal[0]), bits(n)) and bits(r.max_dist[0]) == bits(mx) and bits(r.min_dist[0]) == bits(mn)
    assert not np.array_equal(bits(swapped[0]), bits(n)) and bits(swapped[1]) != bits(mx)


def test_the_propagation_along_a_chain():
    """origin(optimised) -> a -> b -> c(optimised) -> d: a and b are propagated from the origin, c keeps its
    tcw_gba, d hangs off c. Each propagated pose is (Tcw_child * Twc_parent(old)) * TcwGBA_parent(new)."""
    rng = np.random.default_rng(9)
    p = S.gba_problem(9, [-1, 0, 1, 2, 3], [1, 0, 0, 1, 0], 6, bad_every=0, stray_ref_every=0, optimised_every=2)
    p.ref_kf = np.array([0, 4, 2, -1, 1, 3], np.int32)
    p.bad[4] = 1
    r = R.apply_gba(p)
    assert r.propagated.tolist() == [0, 1, 1, 0, 1] and r.levels == 3
    a = R.gemm44(R.gemm44(p.tcw[1], R.pose_inverse(p.tcw[0])), p.tcw_gba[0])
    b = R.gemm44(R.gemm44(p.tcw[2], R.pose_inverse(p.tcw[1])), a)
    d = R.gemm44(R.gemm44(p.tcw[4], R.pose_inverse(p.tcw[3])), p.tcw_gba[3])
    for k, want in ((0, p.tcw_gba[0]), (1, a), (2, b), (3, p.tcw_gba[3]), (4, d)):
        assert np.array_equal(bits(r.tcw_out[k]), bits(want)), k
    # points 0, 2 (and bad 4): pt_optimised; point 1 moves with d; point 3 has no listed reference; point 5 with c
    assert r.pt_changed.tolist() == [1, 1, 1, 0, 0, 1]
    for i in (0, 2):
        assert np.array_equal(bits(r.xw_out[i]), bits(p.xw_gba[i]))
    for i in (3, 4):
        assert np.array_equal(bits(r.xw_out[i]), bits(p.xw[i]))
    for i, k in ((1, 4), (5, 3)):
        B, X = p.tcw[k], p.xw[i]
        xc = [F32(R.dot3(B[4 * q:4 * q + 3], X) + float(B[4 * q + 3])) for q in range(3)]
        twc = R.pose_inverse(r.tcw_out[k])
        want = [F32(R.dot3(twc[4 * q:4 * q + 3], xc) + float(twc[4 * q + 3])) for q in range(3)]
        assert np.array_equal(bits(r.xw_out[i]), bits(want)), i
        assert np.abs(r.xw_out[i] - p.xw[i]).max() > 1e-3
    del rng


def test_every_opencv_rule_of_the_restatement_appears_in_the_core_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "orb_slam2_2021_amd", "csrc", "orbfe_mapcorr_core.h")).read()
    rules = re.findall(r"# (OPENCV: .*)", open(os.path.join(root, "tests", "mapcorr_ref.py")).read())
    assert len(rules) >= 7
    for rule in rules:
        assert rule.strip() in header, rule
