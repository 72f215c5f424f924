"""CPU side of the matcher edge tests: every hand-worked case of tests/edge_scenes.py on the oracle,
and the conditions that keep the low-entropy GPU tests from being vacuous -- the numpy-only event
counters (inputs alone) and the oracle's match counts on the ~300-feature scenes."""
import numpy as np
import pytest

import edge_scenes as E
import match_edge_runs as R


@pytest.mark.parametrize("case", E.EXISTING_CASES + E.NEW_CASES, ids=lambda c: c.__name__)
def test_hand_case_on_the_oracle(case):
    case(E.Oracle())


def test_counters_on_a_hand_case():
    """Four rows (targets, distances), threshold 50, ratio 3 : 4:
      row 0: targets 0, 1, 2 at 5, 5, 9 -- best == second (5, 5); first minimum is target 0 at 5;
      row 1: targets 0, 2 at 5, 8       -- first minimum is target 0 at 5 again: with row 0 that is
                                           one contested target; 4 * 5 != 3 * 8;
      row 2: targets 3, 4 at 6, 8       -- 4 * 6 == 3 * 8: on the ratio boundary;
      row 3: target 5 at 50             -- best on the threshold."""
    rows = [(np.array([0, 1, 2]), np.array([5, 5, 9])), (np.array([0, 2]), np.array([5, 8])),
            (np.array([3, 4]), np.array([6, 8])), (np.array([5]), np.array([50]))]
    ev = E.count_events(rows, 50)
    assert ev == dict(rows=4, best_eq_second=1, on_threshold=1, on_ratio=1, contested=1)


def test_flips_are_distances():
    code = np.random.default_rng(0).integers(0, 256, (4, 32), dtype=np.uint8)
    d = E.hamming(code, E.flip_leading(code, [0, 30, 50, 100]))
    assert np.diag(d).tolist() == [0, 30, 50, 100]
    d = E.hamming(E.flip_leading(code, [36] * 4), E.flip_trailing(code, [12] * 4))
    assert np.diag(d).tolist() == [48] * 4


@pytest.mark.parametrize("vocab", R.VOCABS, ids=str)
def test_low_entropy_scene_reaches_the_edges(vocab):
    """At 300 features per side every event that applies to a search occurs at least 20 times in
    that search's own candidate sets (nodes or windows) and
    the oracle matches at least 20 -- on the random scenes of the other tests the first three
    events occur 0 times in 6,771 rows."""
    sc = R.scene(R.BIG, vocab)
    assert sc.kf1.N == sc.kf2.N == R.BIG
    ev = R.assert_events(sc)
    print(vocab, ev)
    counts = R.oracle_counts(sc)
    print(vocab, counts)
    for search, n in counts.items():
        assert n >= R.MIN_EVENTS, (search, n)


@pytest.mark.parametrize("n", R.SIZES)
def test_scene_sizes_are_exact(n):
    sc = R.scene(n, (10, 2))
    assert sc.kf1.N == sc.f1.N == sc.kf2.N == sc.f2.N == n
    assert len(sc.mps1.flags) == len(sc.mps2.flags) == n


def test_big_node_layout_reaches_the_edges():
    """The 520-node SearchForTriangulation layout: big nodes on both sides of the 256-node chunk,
    at least 20 of each event inside them, at least 20 oracle matches."""
    from oracle import orbref
    K1, K2, F12, positions = R.big_node_trig()
    print(positions, R.check_big_layout(K1, K2, positions))
    assert orbref.search_for_triangulation(K1, K2, F12, *E.FAR_EPIPOLE, False, True)[0] >= R.MIN_EVENTS
