"""orbfe_covis_* on the host-only handle (device < 0): every error path, the capacities, duplicate tie keys, ids
past max_point_id, erase and re-add. No GPU; the queries stop at ORBFE_ERR_STATE after their argument checks."""
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

from orb_slam2_2021_amd import CovisibilityGraph, OrbfeError
from orb_slam2_2021_amd import _lib as L


def status(fn):
    with pytest.raises(OrbfeError) as e:
        fn()
    return e.value.status


def test_create_bounds():
    lib, h = L.lib(), c_void_p()
    for args in ((0, 16, 100), (4097, 16, 100), (8, 0, 100), (8, 8193, 100), (8, 16, 0), (8, 16, (1 << 24) + 1)):
        assert lib.orbfe_covis_create(-1, *args, byref(h)) == L.ORBFE_ERR_ARG, args
        assert not h.value
    assert lib.orbfe_covis_create(-1, 8, 16, 100, None) == L.ORBFE_ERR_ARG
    assert lib.orbfe_covis_create(-1, 4096, 8192, 1 << 24, byref(h)) == L.ORBFE_OK  # host-only: no table allocated
    assert lib.orbfe_covis_destroy(h) == L.ORBFE_OK
    assert lib.orbfe_covis_destroy(None) == L.ORBFE_OK
    n = c_int()
    assert lib.orbfe_covis_size(None, byref(n)) == L.ORBFE_ERR_ARG
    for call in (lambda: lib.orbfe_covis_set_keyframe(None, 1, 1, 0, None), lambda: lib.orbfe_covis_clear(None),
                 lambda: lib.orbfe_covis_set_slots(None, 1, 0, None, None),
                 lambda: lib.orbfe_covis_erase_keyframe(None, 1),
                 lambda: lib.orbfe_covis_set_points_bad(None, 0, None, 1),
                 lambda: lib.orbfe_covis_update_connections(None, 0, None, 15, None),
                 lambda: lib.orbfe_covis_vote(None, 0, None, None, None),
                 lambda: lib.orbfe_covis_local_map(None, 0, None, None)):
        assert call() == L.ORBFE_ERR_ARG


def test_mutations_and_their_errors():
    g = CovisibilityGraph(4, 8, 100, device=-1)
    g.set_keyframe(30, [1, 2, -1, 99], tie_key=5)
    g.set_keyframe(10, [2], tie_key=9)
    g.set_keyframe(20, [])
    assert len(g) == 3 and 20 in g and 40 not in g
    assert status(lambda: g.set_keyframe(40, [1], tie_key=5)) == L.ORBFE_ERR_ARG        # duplicate tie key
    assert status(lambda: g.set_keyframe(10, [1], tie_key=20)) == L.ORBFE_ERR_ARG       # 20's default key
    assert status(lambda: g.set_keyframe(40, [100])) == L.ORBFE_ERR_CAPACITY            # id at max_point_id
    assert status(lambda: g.set_keyframe(40, [-2])) == L.ORBFE_ERR_ARG
    assert status(lambda: g.set_keyframe(40, [1] * 9)) == L.ORBFE_ERR_CAPACITY          # more than max_slots
    assert len(g) == 3 and 40 not in g
    g.set_keyframe(40, [3])
    assert status(lambda: g.set_keyframe(50, [3])) == L.ORBFE_ERR_CAPACITY              # the table is full
    g.set_keyframe(10, [4, 5, 6])                                                        # a whole row replaced
    g.set_slots(10, [0, 2, 0], [7, -1, 9])
    g.set_slots(10, [], [])
    assert status(lambda: g.set_slots(10, [3], [1])) == L.ORBFE_ERR_ARG                 # outside the row
    assert status(lambda: g.set_slots(10, [-1], [1])) == L.ORBFE_ERR_ARG
    assert status(lambda: g.set_slots(10, [0], [100])) == L.ORBFE_ERR_CAPACITY
    assert status(lambda: g.set_slots(10, [0], [-2])) == L.ORBFE_ERR_ARG
    assert status(lambda: g.set_slots(77, [0], [1])) == L.ORBFE_ERR_STATE               # not stored
    g.set_points_bad([1, 99])
    g.set_points_bad([1], False)
    g.set_points_bad([])
    assert status(lambda: g.set_points_bad([100])) == L.ORBFE_ERR_CAPACITY
    assert status(lambda: g.set_points_bad([-1])) == L.ORBFE_ERR_ARG
    with pytest.raises(ValueError):
        g.set_slots(10, [0, 1], [1])
    # erase and re-add
    assert status(lambda: L.check(g._lib.orbfe_covis_erase_keyframe(g._h, 77), "erase")) == L.ORBFE_ERR_STATE
    g.erase(30)
    assert len(g) == 3 and 30 not in g
    g.set_keyframe(50, [3], tie_key=5)   # the erased keyframe's tie key is free again
    assert status(lambda: g.set_keyframe(30, [1, 2], tie_key=6)) == L.ORBFE_ERR_CAPACITY  # and its row is taken
    g.erase(20)
    g.set_keyframe(30, [1, 2], tie_key=20)
    assert len(g) == 4 and 30 in g and 20 not in g
    g.clear()
    assert len(g) == 0
    g.set_keyframe(1, [0])
    assert len(g) == 1
    g.close()


def test_queries_check_arguments_then_refuse_without_a_device():
    g = CovisibilityGraph(8, 16, 100, device=-1)
    for kid in (1, 2, 3):
        g.set_keyframe(kid, [kid, 50, -1])
    assert status(lambda: g.count_connections([1, 2])) == L.ORBFE_ERR_STATE
    assert status(lambda: g.count_connections([1, 9])) == L.ORBFE_ERR_ARG               # 9 is not stored
    assert status(lambda: g.update_connections([3])) == L.ORBFE_ERR_STATE
    assert status(lambda: g.vote([[1, 2, -1]])) == L.ORBFE_ERR_STATE
    assert status(lambda: g.vote([[1, 100]])) == L.ORBFE_ERR_CAPACITY                   # id at max_point_id
    assert status(lambda: g.vote([[-2]])) == L.ORBFE_ERR_ARG
    assert status(lambda: g.vote([[1] * 8193])) == L.ORBFE_ERR_CAPACITY                 # longer than a row can be
    assert status(lambda: g.gather_local_map([1, 2])) == L.ORBFE_ERR_STATE
    assert status(lambda: g.gather_local_map([1, 9])) == L.ORBFE_ERR_ARG
    assert status(lambda: g.gather_local_map([1, 1])) == L.ORBFE_ERR_ARG                # named twice
    # raw calls: missing result arrays, a broken CSR
    lib, ids = g._lib, np.array([1, 2], np.int64)
    r = L.covis_connections(capacity=4)
    assert lib.orbfe_covis_update_connections(g._h, 2, L.ptr(ids), 15, byref(r)) == L.ORBFE_ERR_ARG
    r = L.covis_connections(capacity=-1)
    assert lib.orbfe_covis_update_connections(g._h, 0, L.ptr(ids), 15, byref(r)) == L.ORBFE_ERR_ARG
    v = L.covis_votes(capacity=4)
    begin, pts = np.array([0, 1], np.int32), np.array([1], np.int32)
    assert lib.orbfe_covis_vote(g._h, 1, L.ptr(begin), L.ptr(pts), byref(v)) == L.ORBFE_ERR_ARG
    n, mx, kmax = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int64)
    kids, cnt = np.zeros(8, np.int64), np.zeros(8, np.int32)
    v = L.covis_votes(capacity=4, n=L.ptr(n), kf_ids=L.ptr(kids), counts=L.ptr(cnt), max=L.ptr(mx), kf_max=L.ptr(kmax))
    for bad_begin in ([1, 1], [0, 2, 1]):
        b = np.array(bad_begin, np.int32)
        assert lib.orbfe_covis_vote(g._h, len(b) - 1, L.ptr(b), L.ptr(np.array([1, 2], np.int32)), byref(v)) == L.ORBFE_ERR_ARG
    m = L.covis_local_map(point_capacity=4, fixed_capacity=4, edge_capacity=4)
    assert lib.orbfe_covis_local_map(g._h, 1, L.ptr(ids), byref(m)) == L.ORBFE_ERR_ARG  # no arrays
    assert b"orbfe_covis_local_map" in lib.orbfe_last_error()
    g.close()


def test_readers_of_an_unconnected_keyframe():
    g = CovisibilityGraph(8, 16, 100, device=-1)
    g.set_keyframe(4, [1, 2])
    assert g.GetVectorCovisibleKeyFrames(4) == [] and g.GetBestCovisibilityKeyFrames(4, 10) == []
    assert g.GetCovisiblesByWeight(4, 1) == [] and g.GetConnectedKeyFrames(4) == set()
    assert g.GetWeight(4, 5) == 0 and g.GetParent(4) is None and g.GetChilds(4) == set()
    g.close()
