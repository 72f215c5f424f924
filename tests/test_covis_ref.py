"""tests/covis_ref.py (the reference's UpdateConnections, vote and LocalBundleAdjustment gather restated with its
own containers) held to a second, independent definition and to hand-built cases. CPU only.

The second definition is linear algebra: with A the keyframe x point incidence matrix (A[k, p] = 1 when row k
holds p at least once and p is not bad) and Q_k the counts of keyframe k's slots per point (duplicates included,
bad points zero), KFcounter of k is Q_k . A^T with entry k removed and zeros dropped. The vote of a point list is
its count vector times A^T; the local map's points are the columns any local row of Q touches, its fixed keyframes
the rows of A those columns touch outside the local set."""
import numpy as np
import pytest

from covis_ref import RefCovisibility


def random_world(seed, n_kf=25, n_slots=80, n_points=150, null_frac=0.2):
    rng = np.random.default_rng(seed)
    ref = RefCovisibility()
    ids = rng.permutation(3 * n_kf)[:n_kf].tolist()
    keys = (rng.permutation(n_kf) + 500).tolist()  # not monotone in mnId
    for kid, key in zip(ids, keys):
        row = rng.integers(0, n_points, int(rng.integers(0, n_slots))).tolist()
        row = [-1 if rng.random() < null_frac else p for p in row]
        ref.set_keyframe(kid, row, key)
    ref.set_points_bad(rng.choice(n_points, n_points // 10, replace=False).tolist())
    return ref, ids, dict(zip(ids, keys)), n_points


def matrices(ref, ids, n_points):
    Q = np.zeros((len(ids), n_points), np.int64)
    for r, kid in enumerate(ids):
        for p in ref.kfs[kid].mvpMapPoints:
            if p >= 0 and p not in ref.bad:
                Q[r, p] += 1
    A = (Q > 0).astype(np.int64)
    for p in ref.bad:          # a bad point is skipped on the query side only: its observers still hold it
        for r, kid in enumerate(ids):
            A[r, p] = 1 if p in ref.kfs[kid].mvpMapPoints else 0
    return Q, A


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_counter_is_a_matrix_product(seed):
    ref, ids, key, n_points = random_world(seed)
    Q, A = matrices(ref, ids, n_points)
    W = Q @ A.T
    for th in (1, 4, 15):
        for r, kid in enumerate(ids):
            c = ref.count_connections(kid, th)
            want = {ids[j]: int(W[r, j]) for j in range(len(ids)) if j != r and W[r, j] > 0}
            assert dict(zip(c.counter_ids, c.counter_weights)) == want
            assert c.counter_ids == sorted(want, key=key.get)                      # the map's iteration order
            assert c.unchanged == (not want)
            if not want:
                continue
            assert c.nmax == max(want.values())
            assert c.kf_max == min((k for k in want if want[k] == c.nmax), key=key.get)  # first maximum, strict >
            over = [k for k in want if want[k] >= th]
            if over:
                assert c.ordered_ids == sorted(over, key=lambda k: (want[k], key[k]), reverse=True)
                assert c.ordered_weights == [want[k] for k in c.ordered_ids]
            else:
                assert (c.ordered_ids, c.ordered_weights) == ([c.kf_max], [c.nmax])


@pytest.mark.parametrize("seed", [4, 5])
def test_vote_and_gather_are_matrix_products(seed):
    ref, ids, key, n_points = random_world(seed)
    Q, A = matrices(ref, ids, n_points)
    rng = np.random.default_rng(seed)
    for pts in (rng.integers(-1, n_points, 60).tolist(), [], sorted(ref.bad), [3, 3, 3, -1]):
        q = np.zeros(n_points, np.int64)
        for p in pts:
            if p >= 0 and p not in ref.bad:
                q[p] += 1
        w = A @ q
        v = ref.vote(pts)
        want = {ids[j]: int(w[j]) for j in range(len(ids)) if w[j] > 0}
        assert dict(zip(v.kf_ids, v.counts)) == want and v.kf_ids == sorted(want, key=key.get)
        assert v.max == max(want.values(), default=0)
        assert v.kf_max == (min((k for k in want if want[k] == v.max), key=key.get) if want else -1)
    for n_local in (1, 2, 10):
        local = ids[:n_local]
        rows = [ids.index(k) for k in local]
        cols = np.flatnonzero(Q[rows].sum(axis=0) > 0)
        g = ref.gather_local_map(local)
        assert g.point_ids == cols.tolist()
        seen = np.flatnonzero(A[:, cols].sum(axis=1) > 0)
        assert g.fixed_ids == sorted(ids[j] for j in seen if ids[j] not in local)
        order = sorted(local) + g.fixed_ids
        assert g.edge_begin == [0] + np.cumsum(A[:, cols].sum(axis=0)).tolist()
        for i, p in enumerate(g.point_ids):
            edges = [order[k] for k in g.edge_kf[g.edge_begin[i]:g.edge_begin[i + 1]]]
            assert edges == sorted(ids[j] for j in np.flatnonzero(A[:, p]))       # ascending mnId
            for kid, slot in zip(edges, g.edge_slot[g.edge_begin[i]:g.edge_begin[i + 1]]):
                assert ref.kfs[kid].mvpMapPoints.index(p) == slot                  # the lowest slot


def hand_world():
    """Keyframe 0 holds points 0..59; keyframes 1..4 share 14 / 15 / 16 / 15 of them; tie keys reverse mnId."""
    ref = RefCovisibility()
    ref.set_keyframe(0, list(range(60)), 500)
    ref.set_keyframe(1, list(range(0, 14)), 40)
    ref.set_keyframe(2, list(range(14, 29)), 30)
    ref.set_keyframe(3, list(range(29, 45)), 20)
    ref.set_keyframe(4, list(range(45, 60)), 10)
    return ref


def test_weights_around_th():
    c = hand_world().count_connections(0, 15)
    assert c.counter_ids == [4, 3, 2, 1] and c.counter_weights == [15, 16, 15, 14]
    # 14 stays out; the two 15s are ordered by tie key, the larger (keyframe 2, key 30) first after push_front
    assert c.ordered_ids == [3, 2, 4] and c.ordered_weights == [16, 15, 15]
    assert (c.nmax, c.kf_max) == (16, 3)


def test_nothing_reaches_th_with_a_tie_at_the_maximum():
    ref = hand_world()
    ref.set_slots(3, [15], [-1])  # 15 / 15 / 15 / 14
    c = ref.count_connections(0, 16)
    # strict > while iterating ascending in tie key: keyframe 4 (key 10) is met first and kept
    assert (c.ordered_ids, c.ordered_weights, c.nmax, c.kf_max) == ([4], [15], 15, 4)
    assert c.counter_ids == [4, 3, 2, 1]  # KFcounter is kept whole
    # a sort by mnId would have chosen keyframe 2
    assert min(k for k, w in zip(c.counter_ids, c.counter_weights) if w == 15) == 2


def test_empty_counter_leaves_the_state():
    ref = hand_world()
    ref.set_keyframe(9, [100, 101, -1], 5)
    ref.update_connections([0, 9])
    assert ref.count_connections(9).unchanged
    assert ref.state(9) == ({}, [], [], None, set(), True)  # not even mbFirstConnection moves (:339)
    ref.set_points_bad(list(range(60)))
    before = ref.state(0)
    ref.update_connections([0])   # every shared point is bad now: the early return keeps the old connections
    assert ref.state(0) == before and before[0] == {1: 14, 2: 15, 3: 16, 4: 15}


def test_add_connection_resorts_the_whole_map():
    """UpdateConnections gives a keyframe the ordered entries >= th only; a later AddConnection from another
    keyframe runs UpdateBestCovisibles over the whole weight map, so the entries below th enter the ordered list
    (KeyFrame.cc:122-157)."""
    ref = hand_world()
    ref.update_connections([0])
    assert ref.GetVectorCovisibleKeyFrames(0) == [3, 2, 4] and ref.GetOrderedWeights(0) == [16, 15, 15]
    assert ref.GetConnectedKeyFrames(0) == {1, 2, 3, 4} and ref.GetWeight(0, 1) == 14
    assert ref.GetParent(0) is None                        # never for mnId 0
    assert ref.GetVectorCovisibleKeyFrames(3) == [0] and ref.GetVectorCovisibleKeyFrames(1) == []
    ref.update_connections([1])                            # 14 < th: the fallback connects 1 -> 0 and calls
    assert ref.GetVectorCovisibleKeyFrames(1) == [0]       # keyframe 0's AddConnection(1, 14): same weight, no re-sort
    assert ref.GetVectorCovisibleKeyFrames(0) == [3, 2, 4]
    assert ref.GetParent(1) == 0 and ref.GetChilds(0) == {1}
    ref.set_slots(2, [0], [-1])                            # keyframe 2 now shares 14
    ref.update_connections([2])                            # AddConnection(2, 14) on keyframe 0 differs: re-sort
    assert ref.GetVectorCovisibleKeyFrames(0) == [3, 4, 1, 2] and ref.GetOrderedWeights(0) == [16, 15, 14, 14]
    assert ref.GetBestCovisibilityKeyFrames(0, 2) == [3, 4] and ref.GetBestCovisibilityKeyFrames(0, 10) == [3, 4, 1, 2]
    assert ref.GetCovisiblesByWeight(0, 15) == [3, 4]
    assert ref.GetCovisiblesByWeight(0, 14) == []          # upper_bound reaches end(): the reference returns nothing
    # keyframe 2's own list is [0] before and after (only its weight moved): nothing to mirror for it
    assert ref.kfdb_calls[-2:] == [(1, [0]), (0, [3, 4, 1, 2])]


def test_loop_connections_and_erase():
    ref = hand_world()
    ref.update_connections([0, 1, 2, 3, 4])
    ref.set_keyframe(7, list(range(0, 40)), 7)             # a keyframe from the other side of a loop
    got = ref.loop_connections([0, 3])
    # GetConnectedKeyFrames is the whole weight map, the previous neighbours only the ordered list: keyframe 1
    # (weight 14, never in keyframe 0's ordered list) counts as new along with 7
    assert got == {0: {1, 7}, 3: {7}}
    assert ref.GetWeight(7, 0) == 40 and ref.GetVectorCovisibleKeyFrames(7) == [0]  # by AddConnection alone
    ref.erase(0)
    assert ref.GetVectorCovisibleKeyFrames(7) == [] and ref.GetConnectedKeyFrames(3) == {7}
    assert ref.GetParent(1) == 0                            # the re-parenting is not restated
    assert 0 not in ref.observations().get(5, {})
