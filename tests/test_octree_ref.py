"""DistributeOctTree's hand-built key sets (tests/octree_scenes.py) against the second reference
(tests/octree_ref.py), and the oracle (oracle/orbref.cpp) held to that reference.

The hand-written survivor lists are the fixed point: octree_ref must give them, with the stop rule and
the trace figures each scene claims, and the oracle must give what octree_ref gives from the oracle's
own candidates, on every hand-built, large-node and random scene. tests/test_gpu_octree_edges.py
makes the same comparison with k_octree in the oracle's place.
"""
import functools

import numpy as np
import pytest

import definition_ref as D
import octree_ref as O
import octree_scenes as S
from oracle.orbref import RefExtractor

HAND = S.hand_scenes()
LARGE = S.large_scenes()
RANDOM = S.random_scenes()
ALL = HAND + LARGE + RANDOM


def ids(scenes):
    return [s.name for s in scenes]


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """(candidates in the oracle's order, survivors in list order), border-relative."""
    sc = next(s for s in ALL if s.name == name)
    ref = RefExtractor(sc.N, 1.2, 1, 20, 7)
    kps, _ = ref(sc.image())
    cand = D.unpack_keys(ref.candidates(0))
    keys = [(x - S.BORDER, y - S.BORDER, r) for x, y, r in D.unpack_keys(ref.level_keys(0))]
    assert len(kps) == len(keys)
    return cand, keys


@pytest.mark.parametrize("sc", HAND, ids=ids(HAND))
def test_hand_built_expectations(sc):
    """octree_ref gives the written-out survivors, by the stop rule and through the branch the scene
    claims, from the scene's key order and from the FAST cell order of the same keys."""
    got, tr = O.distribute_traced(sc.keys, sc.w, sc.h, sc.N)
    assert got == sc.expect
    assert tr.stop == sc.stop
    for name, want in sc.trace.items():
        assert getattr(tr, name) == want, f"trace.{name}: {getattr(tr, name)} vs {want}"
    assert O.distribute(oracle_run(sc.name)[0], sc.w, sc.h, sc.N) == sc.expect
    assert O.tie_sensitive(sc.keys, sc.w, sc.h, sc.N) == sc.tie
    if sc.tie:  # the case must keep testing the rule
        assert O.distribute(sc.keys, sc.w, sc.h, sc.N, "reverse") != sc.expect


@pytest.mark.parametrize("sc", HAND, ids=ids(HAND))
def test_oracle_gives_hand_built_expectations(sc):
    cand, keys = oracle_run(sc.name)
    assert set(cand) == set(sc.keys) and len(cand) == len(sc.keys)
    assert keys == sc.expect


@pytest.mark.parametrize("sc", ALL, ids=ids(ALL))
def test_oracle_held_to_second_reference(sc):
    """The scene's image gives exactly the designed keys as candidates, and the oracle's survivors
    equal, in order, octree_ref's from the oracle's candidates."""
    cand, keys = oracle_run(sc.name)
    assert len(cand) == len(sc.keys) and set(cand) == set(sc.keys), \
        f"only oracle {sorted(set(cand) - set(sc.keys))[:5]}, only scene {sorted(set(sc.keys) - set(cand))[:5]}"
    want, tr = O.distribute_traced(cand, sc.w, sc.h, sc.N)
    for name, claimed in sc.trace.items():
        assert getattr(tr, name) == claimed, f"trace.{name}: {getattr(tr, name)} vs {claimed}"
    assert keys == want, f"first difference at {next(i for i, (a, b) in enumerate(zip(keys + [None], want + [None])) if a != b)}"


def test_owner_disagreements_are_occupied():
    """The x where (int)(hX * i) and (size_t)(x / hX) name different initial nodes exist for the
    fractional hX of the two sweep scenes, are the ones the scenes state, and hold a dot each; the
    hand-written first-owned x are the reference expressions' own."""
    for name, firsts, bad in (("ini8_boundary_sweep", S._INI8_B, [31, 62, 93, 156, 187, 218]),
                              ("ini9_boundary_sweep", S._INI9_B, [33, 66, 133, 166, 233, 266])):
        sc = next(s for s in HAND if s.name == name)
        assert O.owner_disagreements(sc.w, sc.h) == bad
        xs = {k[0] for k in sc.keys}
        assert set(bad) <= xs
        hx = np.float32(sc.w) / np.float32(len(firsts) + 1)
        for i, b in enumerate(firsts, 1):
            assert int(np.float32(b) / hx) == i and int(np.float32(b - 1) / hx) == i - 1
            assert {b - 2, b - 1, b, b + 1, b + 2} <= xs
    assert O.owner_disagreements(1920, 30) == [] and O.owner_disagreements(384, 32) == []


def test_scene_coverage():
    """The scene sets reach what they are there for: every stop rule, every overshoot 0..3, the
    initial-node counts on both sides of the kernel's placement switch and at the upper limit,
    divided nodes of every size around the thread-serial threshold and the 64-lane step, a node one
    pixel wide; and the number of tie-sensitive random scenes (compared under the creation
    rule like the rest)."""
    traces = {s.name: O.distribute_traced(s.keys, s.w, s.h, s.N)[1] for s in ALL}
    hand = [traces[s.name] for s in HAND]
    assert {t.stop for t in hand} == {O.PASS_N, O.PASS_STALL, O.REFINE_N, O.REFINE_STALL}
    assert {0, 1, 2, 3} <= {t.overshoot for t in hand}
    assert {1, 2, 3, 8, 9, 12, 64} <= {t.nIni for t in hand}
    divided = {traces[s.name].max_divided for s in LARGE}
    assert set(S.LARGE_COUNTS[1:]) <= divided and max(divided) > 256
    assert min(t.min_w for t in hand) == 1
    assert {traces[s.name].stop for s in RANDOM} == {O.PASS_N, O.PASS_STALL, O.REFINE_N, O.REFINE_STALL}
    assert max(traces[s.name].rounds for s in LARGE + RANDOM) >= 2
    sens = [s.name for s in LARGE + RANDOM if O.tie_sensitive(s.keys, s.w, s.h, s.N)]
    print(f"tie-sensitive: {len([n for n in sens if n.startswith('random')])} of {len(RANDOM)} random scenes, "
          f"{len([n for n in sens if n.startswith('large')])} of {len(LARGE)} large-node scenes")
    assert [s.name for s in HAND if s.tie] == ["tie_equal_sizes_creation_order_decision"]
