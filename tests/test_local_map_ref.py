"""tests/local_map_ref.py (the reference's walks with its stamps and push_backs) held to a second definition -- the
named rows concatenated, filtered, np.unique ordered by first index -- and to hand-built cases with the expected
lists written out; CPU only. The GPU tests compare the library against the restatement these tests pin."""
import numpy as np
import pytest

import local_map_ref as R


def walk_case(name, rows, kf_list, want, bad=()):
    return dict(name=name, rows=rows, list=kf_list, want=want, bad=list(bad))


# rows: {mnId: row}; list: the keyframe list; want: the expected push_back order
WALK_CASES = [
    walk_case("a point in two slots of one row", {0: [5, 3, 5, 7]}, [0], [5, 3, 7]),
    walk_case("a point in three rows", {0: [1, 2], 1: [2, 3], 2: [3, 2, 4]}, [0, 1, 2], [1, 2, 3, 4]),
    walk_case("the list order decides, not mnId", {0: [1, 2], 1: [2, 3], 2: [3, 2, 4]}, [2, 0, 1], [3, 2, 4, 1]),
    walk_case("a keyframe named twice", {0: [1, 2], 1: [9, 2]}, [0, 1, 0], [1, 2, 9]),
    walk_case("an all -1 row", {0: [-1, -1, -1], 1: [4, -1, 6]}, [0, 1], [4, 6]),
    walk_case("a length-0 row", {0: [], 1: [4, 6]}, [0, 1], [4, 6]),
    walk_case("a length-0 row alone", {0: [], 1: [4]}, [0], []),
    walk_case("every point bad", {0: [1, 2], 1: [2, 3]}, [0, 1], [], bad=[1, 2, 3]),
    walk_case("a bad point between good ones", {0: [1, 2, 3], 1: [2, 5]}, [0, 1], [1, 3, 5], bad=[2]),
    walk_case("an empty result", {0: [-1], 1: [-1, -1]}, [1, 0], []),
]


def build(c):
    rows = {k: np.asarray(v, np.int32) for k, v in c["rows"].items()}
    return R.build_ref(rows, {k: k for k in rows}, c["bad"])


@pytest.mark.parametrize("c", WALK_CASES, ids=[c["name"] for c in WALK_CASES])
def test_hand_built_walks(c):
    ref = build(c)
    assert ref.update_local_points(c["list"], 7) == c["want"]
    second = R.distinct_by_unique([c["rows"][k] for k in c["list"]], c["bad"])
    assert second.tolist() == c["want"]
    # the stamp holds: the same Frame again collects nothing, the next Frame collects the same list
    assert ref.update_local_points(c["list"], 7) == []
    assert ref.update_local_points(c["list"], 8) == c["want"]


def test_a_bad_flag_set_and_then_cleared():
    ref = build(walk_case("", {0: [1, 2, 3], 1: [2, 5]}, [0, 1], None))
    ref.set_points_bad([2, 5])
    assert ref.update_local_points([0, 1], 1) == [1, 3]
    ref.set_points_bad([2], False)
    assert ref.update_local_points([0, 1], 2) == [1, 2, 3]
    ref.set_points_bad([5], False)
    assert ref.update_local_points([0, 1], 3) == [1, 2, 3, 5]


def test_stamp_zero_is_the_reference_artefact():
    ref = build(WALK_CASES[1])
    assert ref.update_local_points([0, 1, 2], 0) == []  # every member starts at 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_three_walks_equal_the_second_definition(seed):
    rows, tie, bad, _ = R.random_scene(seed)
    ref = R.build_ref(rows, tie, bad, connect_th=3)
    rng = np.random.default_rng(100 + seed)
    for frame in range(1, 6):
        kf_list = rng.integers(0, len(rows), rng.integers(1, 30)).tolist()  # repeats included
        want = R.distinct_by_unique([rows[k] for k in kf_list], bad).tolist()
        assert ref.update_local_points(kf_list, frame) == want
        assert len(set(want)) == len(want) and not set(want) & set(bad) and -1 not in want
    for k, mono in ((5, False), (20, True), (33, False)):  # a keyframe passes through SearchInNeighbors once
        targets, cands = ref.fuse_candidates(k, mono)
        assert cands == R.distinct_by_unique([rows[t] for t in targets], bad).tolist()
        loop = ref.loop_map_points(k, 500 + k)
        order = ref.GetVectorCovisibleKeyFrames(k) + [k]
        assert loop == R.distinct_by_unique([rows[t] for t in order], bad).tolist()


def test_fuse_targets_keep_a_second_neighbour_twice():
    ref = R.hand_graph(6)
    R.link(ref, 5, ordered=[1, 2])
    R.link(ref, 1, ordered=[5, 3, 4])
    R.link(ref, 2, ordered=[3, 5, 1])
    # 1, its seconds 3 and 4 (5 is the keyframe itself); 2, its seconds 3 again (never stamped), 1 is stamped
    assert ref.fuse_targets(5, False) == [1, 3, 4, 2, 3]
    ref = R.hand_graph(6)
    R.link(ref, 5, ordered=[1, 2])
    R.link(ref, 1, ordered=[5, 3, 4])
    R.link(ref, 2, ordered=[3, 5, 1])
    targets, cands = ref.fuse_candidates(5, False)
    assert targets == [1, 3, 4, 2, 3] and cands == [1, 3, 4, 2]


# ---- UpdateLocalKeyFrames, the second half ----------------------------------------------------------
def keyframe_cases():
    out = []
    ref = R.hand_graph(8)
    R.link(ref, 0, ordered=[1, 6], parent=5)
    R.link(ref, 1, ordered=[7])
    out.append(("a parent on the first turn ends the loop", ref, [0, 1, 2], ([0, 1, 2, 6, 5], 0)))
    ref = R.hand_graph(14)
    R.link(ref, 0, ordered=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])
    out.append(("the first nine are included: the tenth is taken", ref, list(range(10)), (list(range(10)) + [10], 0)))
    ref = R.hand_graph(14)
    R.link(ref, 0, ordered=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11])
    out.append(("the first ten are included: the eleventh is out of reach", ref, list(range(11)),
                (list(range(11)), 0)))
    tie = {k: 100 - k for k in range(8)}  # pointer order is the reverse of mnId order
    ref = R.hand_graph(8, tie)
    R.link(ref, 7, children=[3, 4, 5])
    out.append(("children by tie key, not mnId", ref, [7], ([7, 5], 7)))
    ref = R.hand_graph(8, tie)
    R.link(ref, 7, children=[3, 4, 5])
    out.append(("an included child is passed over", ref, [7, 5], ([7, 5, 4], 7)))  # voted in tie order: 7 (93), 5 (95)
    ref = R.hand_graph(8)
    R.link(ref, 2, ordered=[3], children=[4], parent=1)
    out.append(("neighbour, child and parent in one turn", ref, [2], ([2, 3, 4, 1], 2)))
    ref = R.hand_graph(8)
    R.link(ref, 1, parent=0)
    R.link(ref, 2, ordered=[5])
    out.append(("an included parent does not end the loop", ref, [0, 1, 2], ([0, 1, 2, 5], 0)))
    for n, want_len in ((79, 81), (80, 81), (81, 81)):
        ref = R.hand_graph(2 * n)
        for k in range(n):
            R.link(ref, k, ordered=[n + k])
        want = list(range(n)) + [n + k for k in range(want_len - n)]
        out.append((f"{n} voted keyframes", ref, list(range(n)), (want, 0)))
    return out


KEYFRAME_CASES = keyframe_cases()


@pytest.mark.parametrize("name,ref,frame,want", KEYFRAME_CASES, ids=[c[0] for c in KEYFRAME_CASES])
def test_hand_built_keyframe_half(name, ref, frame, want):
    got = ref.update_local_keyframes(frame, 3)
    assert got == want
    assert len(set(got[0])) == len(got[0])


def test_an_empty_vote_returns_none():
    ref = R.hand_graph(4)
    assert ref.update_local_keyframes([], 1) is None
    assert ref.update_local_keyframes([-1, -1], 2) is None
    ref.set_points_bad([2])
    assert ref.update_local_keyframes([2, -1], 3) is None
    assert ref.update_local_keyframes([77], 4) is None  # a point nobody observes
    assert ref.update_local_map([77], 5) is None


@pytest.mark.parametrize("seed", [4, 5])
def test_the_first_half_is_the_vote_and_the_whole_is_bounded(seed):
    rows, tie, bad, n_points = R.random_scene(seed, n_kf=60)
    ref = R.build_ref(rows, tie, bad, connect_th=3)
    rng = np.random.default_rng(seed)
    for frame in range(1, 8):
        pts = rng.integers(-1, n_points, 40).tolist()
        v = ref.vote(pts)
        got = ref.update_local_map(pts, frame)
        if not v.kf_ids:
            assert got is None
            continue
        local, kf_max, points = got
        assert local[:len(v.kf_ids)] == v.kf_ids and kf_max == v.kf_max
        assert len(set(local)) == len(local) and len(local) <= max(len(v.kf_ids), 80) + 3
        extra = local[len(v.kf_ids):]
        assert len(extra) <= 3 * len(v.kf_ids)  # the reserve at :1284 is never outgrown
        assert points == R.distinct_by_unique([rows[k] for k in local], bad).tolist()
