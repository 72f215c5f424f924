"""tests/culling_ref.py held to account on the CPU: against a second definition (incidence matrices) for a pass with
no culls, on hand-built cases worked out below, and the random-scene generator against the conditions that make
the GPU comparisons bite (a cull, a cascade, a decision that depends on the order)."""
import numpy as np
import pytest

import culling_ref as C
from culling_ref import keyframe as K


def case(name, kfs, cand, mono, want, not_erase=(), bad=(), want_bad=None, want_counts=None):
    return dict(name=name, kfs=kfs, cand=cand, mono=mono, want=want, not_erase=not_erase, bad=bad, want_bad=want_bad,
                want_counts=want_counts)


def line_case(n_mps, n_red):
    """Candidate 1 holds n_mps points; the first n_red are held by 2, 3, 4 too (Observations() 4, three others in
    the same octave: redundant), the rest by nobody else."""
    pts = list(range(n_mps))
    return [K(1, pts)] + [K(i, pts[:n_red]) for i in (2, 3, 4)]


def hand_cases():
    cs = []
    # -- Observations() around > 3. One slot, so redundant means 1 > 0.9 * 1.
    # 1 mono + 2, 3, 4 mono: nObs 4, three others: culled. p0 keeps nObs 3 afterwards: nothing goes bad.
    cs.append(case("obs4_mono", [K(1, [0]), K(2, [0]), K(3, [0]), K(4, [0])], [1], True, [1], want_bad=[[]],
                   want_counts=[(1, 1)]))
    # 1 stereo + 2, 3 mono: nObs 4 > 3, but only two others: kept
    cs.append(case("obs4_two_others", [K(1, [0], stereo=[True]), K(2, [0]), K(3, [0])], [1], True, [0],
                   want_counts=[(1, 0)]))
    # 1 mono + 2 stereo: nObs 3, not > 3: kept
    cs.append(case("obs3", [K(1, [0]), K(2, [0], stereo=[True])], [1], True, [0], want_counts=[(1, 0)]))
    # 1 mono + 2, 3, 4 stereo: nObs 7; culled; 6 left
    cs.append(case("obs7_stereo", [K(1, [0])] + [K(i, [0], stereo=[True]) for i in (2, 3, 4)], [1], True, [1]))
    # -- the octave gate: the slot is in octave 2; observers in octave 3 pass, one in octave 4 does not
    cs.append(case("octave_plus1", [K(1, [0], [2])] + [K(i, [0], [3]) for i in (2, 3, 4)], [1], True, [1]))
    cs.append(case("octave_plus2", [K(1, [0], [2]), K(2, [0], [3]), K(3, [0], [3]), K(4, [0], [4])], [1], True, [0],
                   want_counts=[(1, 0)]))
    # -- FAR: p0 redundant and near, p1 private and far. Stereo run: nMPs 1, nRed 1: culled. Mono run: 1 of 2: kept.
    far = [K(1, [0, 1], far=[False, True]), K(2, [0]), K(3, [0]), K(4, [0])]
    cs.append(case("far_stereo_run", far, [1], False, [1], want_counts=[(1, 1)]))
    cs.append(case("far_mono_run", far, [1], True, [0], want_counts=[(2, 1)]))
    # -- nMPs 0: 0 > 0.0 is false
    cs.append(case("no_points", [K(1, [-1, -1, -1]), K(2, [0])], [1], True, [0], want_counts=[(0, 0)]))
    cs.append(case("empty_row", [K(1, []), K(2, [0])], [1], True, [0], want_counts=[(0, 0)]))
    # -- 0.9 * nMPs: 9.0, 18.0, 27.0 in double (asserted below); equal is kept, one more is culled
    for n_mps in (10, 20, 30):
        n_red = 9 * n_mps // 10
        cs.append(case(f"line_{n_mps}_at", line_case(n_mps, n_red), [1], True, [0], want_counts=[(n_mps, n_red)]))
        cs.append(case(f"line_{n_mps}_over", line_case(n_mps, n_red + 1), [1], True, [1],
                       want_counts=[(n_mps, n_red + 1)]))
    # -- A (1) and B (2) hold ten points that 3 and 4 hold too: nObs 4. Whoever comes first is culled (nObs 3), the
    #    other then has nothing redundant.
    pts = list(range(10))
    pair = [K(i, pts) for i in (1, 2, 3, 4)]
    cs.append(case("pair_ab", pair, [1, 2], True, [1, 0], want_counts=[(10, 10), (10, 0)]))
    cs.append(case("pair_ba", pair, [2, 1], True, [1, 0], want_counts=[(10, 10), (10, 0)]))
    # -- not_erase: A is redundant but stays (mbToBeErased); B still sees it: culled
    cs.append(case("not_erase", pair, [1, 2], True, [2, 1], not_erase=[1], want_counts=[(10, 10), (10, 10)]))
    # -- mnId 0 is passed over, however redundant
    cs.append(case("id0", [K(i, pts) for i in (0, 2, 3, 4)], [0, 2], True, [3, 1], want_counts=[(0, 0), (10, 10)]))
    # -- cascade. A (1): 19 points that 3, 4, 5 hold and point 100 that only X (2, stereo there) holds: nObs 3.
    #    19 > 0.9 * 20: culled. Point 100 drops to nObs 2: bad, and leaves X's row. X: 100 and 9 points that 6, 7, 8
    #    hold: before 9 of 10 (kept), after 9 of 9 (culled). Its cull makes nothing bad (the nine keep nObs 3).
    red = list(range(19))
    xs = list(range(200, 209))
    casc = [K(1, red + [100]), K(2, [100] + xs, stereo=[True] + [False] * 9)] + [K(i, red) for i in (3, 4, 5)] + \
           [K(i, xs) for i in (6, 7, 8)]
    cs.append(case("cascade", casc, [1, 2], True, [1, 1], want_bad=[[100], []], want_counts=[(20, 19), (9, 9)]))
    cs.append(case("cascade_reversed", casc, [2, 1], True, [0, 1], want_bad=[[], [100]],
                   want_counts=[(10, 9), (20, 19)]))
    # -- a point in two slots: 19 redundant points and point 100 twice; nMPs 21 (both slots count), 19 > 18.9;
    #    100 is erased once, at the first of its slots, and listed once
    two = [K(1, red + [100, 100]), K(2, [100], stereo=[True])] + [K(i, red) for i in (3, 4, 5)]
    cs.append(case("two_slots", two, [1], True, [1], want_bad=[[100]], want_counts=[(21, 19)]))
    # -- a point that was bad before the call is not counted and not listed
    cs.append(case("bad_before", [K(1, [0, 1])] + [K(i, [0]) for i in (2, 3, 4)], [1], True, [1], bad=[1],
                   want_bad=[[]], want_counts=[(1, 1)]))
    return cs


CASES = hand_cases()


def run_case(c):
    ref = C.build_ref(c["kfs"], c["bad"])
    out = ref.keyframe_culling(c["cand"], c["mono"], c["not_erase"])
    return ref, out


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_hand_built_keyframe_cases(c):
    before = {k.mn_id: k.points.tolist() for k in c["kfs"]}
    ref, out = run_case(c)
    assert out.decision == c["want"]
    if c["want_bad"] is not None:
        assert out.bad_points == c["want_bad"]
    if c["want_counts"] is not None:
        assert list(zip(out.n_mps, out.n_redundant)) == c["want_counts"]
    culled = [i for i, d in zip(c["cand"], out.decision) if d == C.CULLED]
    assert sorted(ref.kfs) == sorted(set(before) - set(culled))
    gone = {p for lst in out.bad_points for p in lst}
    assert gone <= ref.bad
    for i, kf in ref.kfs.items():  # only the bad points' recorded slots changed
        for s, (was, now) in enumerate(zip(before[i], kf.mvpMapPoints)):
            assert now == was or (now == -1 and was in gone and before[i].index(was) == s)


def test_the_line_is_exact_in_double():
    assert 0.9 * 10 == 9.0 and 0.9 * 20 == 18.0 and 0.9 * 30 == 27.0
    assert not 9 > 0.9 * 10 and 10 > 0.9 * 10


def test_not_erase_leaves_everything_as_it_was():
    c = next(c for c in CASES if c["name"] == "not_erase")
    ref, out = run_case(c)
    assert 1 in ref.kfs and ref.to_be_erased == {1} and 2 not in ref.kfs


def test_cascade_edits_the_observer_row():
    c = next(c for c in CASES if c["name"] == "cascade")
    ref = C.build_ref(c["kfs"])
    assert ref.points[100].nObs == 3
    ref.keyframe_culling([1], True)
    assert ref.points[100].mbBad and ref.points[100].nObs == 2 and ref.kfs[2].mvpMapPoints[0] == -1


# ---- a second definition for a pass without culls -----------------------------------------------------------------
def matrices(kfs, n_points):
    n = len(kfs)
    A = np.zeros((n, n_points), np.int64)
    st = np.zeros((n, n_points), np.int64)
    oc = np.zeros((n, n_points), np.int64)
    for k, kf in enumerate(kfs):
        for s in range(len(kf.points) - 1, -1, -1):  # the lowest slot is written last
            p = kf.points[s]
            if p >= 0:
                A[k, p] = 1
                st[k, p] = kf.u_right[s] >= 0
                oc[k, p] = kf.octaves[s]
    return A, st, oc


@pytest.mark.parametrize("seed,mono", [(5, True), (6, False)])
def test_evaluation_equals_the_incidence_definition(seed, mono):
    kfs, _, _ = C.random_scene(seed, n_kf=40, slots=24, n_candidates=10)
    ref = C.build_ref(kfs)
    n_points = 1 + max(int(k.points.max()) for k in kfs)
    A, st, oc = matrices(kfs, n_points)
    W = (A * (1 + st)).sum(0)
    some = 0
    for c, kf in enumerate(kfs):
        n_mps = n_red = 0
        for s, p in enumerate(kf.points):
            if p < 0 or (not mono and (kf.depth[s] > kf.th_depth or kf.depth[s] < 0)):
                continue
            n_mps += 1
            G = A[:, p] * (oc[:, p] <= kf.octaves[s] + 1)
            if W[p] > 3 and G.sum() - G[c] >= 3:
                n_red += 1
        got = ref.evaluate(kf.mn_id, mono)
        assert got[:2] == (n_mps, n_red), kf.mn_id
        assert got[2] == (10 * n_red > 9 * n_mps)  # the line in integers
        some += n_red
    assert some > 0
    for p, mp in ref.points.items():  # nObs, kept incrementally, against the weighted column sum
        assert mp.nObs == W[p]


# ---- MapPointCulling ------------------------------------------------------------------------------------------------
def point_scene():
    """Point p has p mono observers, p = 0..5; point 6 has a stereo and a mono observer (nObs 3)."""
    kfs = [K(10 + k, [p if p > k else -1 for p in range(6)] + [6], stereo=[False] * 6 + [k == 0]) for k in range(5)]
    kfs[2].points[6] = kfs[3].points[6] = kfs[4].points[6] = -1
    return kfs


POINT_CASES = [
    # (point, found, visible, first, current, mono, action)
    (4, 1, 4, 10, 10, True, 0),     # ratio exactly 0.25 is not < 0.25; age 0: stays
    (4, 249999, 1000000, 10, 10, True, 2),
    (4, 0, 0, 10, 10, True, 0),     # 0 / 0 is NaN
    (4, 1, 0, 10, 13, True, 4),     # +inf
    (4, 0, 1, 10, 10, True, 2),
    (2, 1, 1, 10, 11, True, 0),     # age 1: the observations are not looked at
    (2, 1, 1, 10, 12, True, 3),     # age 2, nObs 2 <= 2
    (3, 1, 1, 10, 12, True, 0),     # nObs 3 > 2 (mono)
    (3, 1, 1, 10, 12, False, 3),    # nObs 3 <= 3 (stereo)
    (4, 1, 1, 10, 12, False, 0),    # nObs 4
    (4, 1, 1, 10, 13, False, 4),    # age 3
    (6, 1, 1, 10, 12, False, 3),    # weighted: 2 + 1
    (6, 1, 1, 10, 12, True, 0),
    (3, 1, 1, 12, 10, True, 0),     # negative age
    (0, 1, 1, 10, 12, True, 3),     # no observers
]


@pytest.mark.parametrize("p,found,visible,first,cur,mono,want", POINT_CASES)
def test_map_point_culling_branches(p, found, visible, first, cur, mono, want):
    ref = C.build_ref(point_scene())
    assert ref.map_point_culling([p], [found], [visible], [first], cur, mono) == [want]
    if want in (2, 3):
        assert p in ref.bad and all(p not in kf.mvpMapPoints for kf in ref.kfs.values())
    else:
        assert p not in ref.bad
    bad = C.build_ref(point_scene(), bad=[p])
    assert bad.map_point_culling([p], [found], [visible], [first], cur, mono) == [1]


# ---- re-parenting -----------------------------------------------------------------------------------------------
def graph(links, parents):
    """Keyframes with the given symmetric weights {(a, b): w} and parents {child: parent}."""
    ids = sorted({i for ab in links for i in ab} | set(parents) | set(parents.values()))
    ref = C.build_ref([K(i, []) for i in ids])
    for (a, b), w in links.items():
        ref.kfs[a].mConnectedKeyFrameWeights[b] = w
        ref.kfs[b].mConnectedKeyFrameWeights[a] = w
    for kf in ref.kfs.values():
        ref._update_best_covisibles(kf)
        kf.mbFirstConnection = False
    for c, p in parents.items():
        ref.kfs[c].mpParent = p
        ref.kfs[p].mspChildrens.add(c)
    return ref


REPARENT = {
    # 5 is erased; its parent is 1. Child 6 sees candidates... only 1 at first.
    # two candidate parents at equal weight: after 6 joins 1, child 7 sees 1 and 6 with weight 20 each; the ordered
    # list of 7 is descending in (weight, key), so 6 comes first and the strict > keeps it: parent 6
    "equal_weight": (dict(links={(5, 6): 50, (5, 7): 50, (6, 1): 30, (7, 1): 20, (7, 6): 20, (5, 1): 40},
                          parents={5: 1, 6: 5, 7: 5}), {6: 1, 7: 6}),
    # a chain: 6 is linked to the old parent, 7 only to 6, 8 only to 7: each re-parented child is the next one's parent
    "chain": (dict(links={(5, 6): 50, (5, 7): 50, (5, 8): 50, (6, 1): 30, (7, 6): 25, (8, 7): 20, (5, 1): 40},
                   parents={5: 1, 6: 5, 7: 5, 8: 5}), {6: 1, 7: 6, 8: 7}),
    # 9 has no link to any candidate: it goes to the old parent
    "no_link": (dict(links={(5, 6): 50, (5, 9): 50, (6, 1): 30, (5, 1): 40}, parents={5: 1, 6: 5, 9: 5}),
                {6: 1, 9: 1}),
}


@pytest.mark.parametrize("name", sorted(REPARENT))
def test_reparenting(name):
    spec, want = REPARENT[name]
    ref = graph(**spec)
    ref.set_bad_flag(5)
    assert 5 not in ref.kfs and ref.kfdb_erased == [5]
    for child, parent in want.items():
        assert ref.GetParent(child) == parent, child
        assert child in ref.GetChilds(parent)
    assert 5 not in ref.GetChilds(1)
    for kf in ref.kfs.values():
        assert 5 not in kf.mConnectedKeyFrameWeights and 5 not in kf.mvpOrderedConnectedKeyFrames


# ---- the generator ------------------------------------------------------------------------------------------------
SCENE_SEEDS = (0, 1, 2, 3)


@pytest.mark.parametrize("seed", SCENE_SEEDS)
def test_the_generator_makes_the_order_matter(seed):
    kfs, cand, mono = C.random_scene(seed)
    assert len(kfs) == 300 and len(cand) == 65 and len(set(cand)) == 65
    ref = C.build_ref(kfs)
    free = ref.order_free_decisions(cand, mono)
    out = ref.keyframe_culling(cand, mono)
    assert out.decision.count(C.CULLED) >= 1
    assert sum(len(b) for b in out.bad_points) >= 1
    assert any(a != b for a, b in zip(free, out.decision))
    counts = sorted({len(mp.mObservations) for mp in C.build_ref(kfs).points.values()})
    assert counts[0] == 1 and counts[-1] >= 6
