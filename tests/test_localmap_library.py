"""include/orbfe_localmap.h on the host-only handle (device < 0): every error path and capacity rule, with "nothing
touched" checked where it is promised, the bounds the header states, and the host half of UpdateLocalKeyFrames'
wrappers that need no device. No GPU; the device calls stop at ORBFE_ERR_STATE after their argument checks."""
from ctypes import byref

import numpy as np
import pytest

import local_map_ref as R
from orb_slam2_2021_amd import CovisibilityGraph, OrbfeError, ResidentLocalMap
from orb_slam2_2021_amd import _lib as L


def status(fn):
    with pytest.raises(OrbfeError) as e:
        fn()
    return e.value.status


def graph():
    g = CovisibilityGraph(4096, 8192, 1000, device=-1)
    g.set_keyframe(3, [1, 2, -1])
    g.set_keyframe(5, [2, 7])
    g.set_keyframe(9, [])
    return g


def points_call(g, ids, capacity=8, buf=None, n_points=-5):
    ids = np.ascontiguousarray(ids, np.int64)
    buf = np.full(max(capacity, 1), -7, np.int32) if buf is None else buf
    r = L.covis_points(point_capacity=capacity, n_points=n_points, point_ids=L.ptr(buf))
    st = g._lib.orbfe_covis_distinct_points(g._h, len(ids), L.ptr(ids), byref(r))
    return st, r, buf


def test_the_symbols_are_exported_and_declared():
    lib = L.lib()
    for name in ("orbfe_covis_distinct_points", "orbfe_covis_set_point_geometry", "orbfe_covis_local_geometry"):
        assert name in L.EXPORTED and getattr(lib, name)


def test_distinct_points_argument_checks():
    g = graph()
    lib = g._lib
    ids = np.asarray([3, 5], np.int64)
    r = L.covis_points(point_capacity=0, n_points=0, point_ids=None)
    assert lib.orbfe_covis_distinct_points(None, 2, L.ptr(ids), byref(r)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_covis_distinct_points(g._h, 2, L.ptr(ids), None) == L.ORBFE_ERR_ARG
    assert lib.orbfe_covis_distinct_points(g._h, 2, None, byref(r)) == L.ORBFE_ERR_ARG
    r = L.covis_points(point_capacity=4, n_points=0, point_ids=None)       # a capacity without an array
    assert lib.orbfe_covis_distinct_points(g._h, 2, L.ptr(ids), byref(r)) == L.ORBFE_ERR_ARG
    r = L.covis_points(point_capacity=-1, n_points=0, point_ids=None)
    assert lib.orbfe_covis_distinct_points(g._h, 2, L.ptr(ids), byref(r)) == L.ORBFE_ERR_ARG
    for bad_list in ([], [3, 4], [4], [3, 5, -1]):                           # empty; an id that is not stored
        st, r, buf = points_call(g, bad_list)
        assert st == L.ORBFE_ERR_ARG, bad_list
        assert r.n_points == -5 and (buf == -7).all()                        # nothing touched
    # well-formed lists reach the host-only refusal: repeats, an empty row, a capacity of 0
    for ok_list, cap in (([3], 8), ([3, 5, 3, 3], 8), ([9], 8), ([5, 9], 0)):
        st, r, buf = points_call(g, ok_list, cap)
        assert st == L.ORBFE_ERR_STATE, ok_list
        assert "host-only" in L.last_error() and (buf == -7).all()
    g.erase(5)
    assert points_call(g, [3, 5])[0] == L.ORBFE_ERR_ARG                      # erased: no longer stored
    assert points_call(g, [3])[0] == L.ORBFE_ERR_STATE


def test_the_list_bound_is_4096_entries_and_nothing_else():
    """The header's bounds: 1..4096 list entries of at most 8192 slots; the 2^25 slots that allows are all accepted
    (a key is position << 13 | slot), so there is no separate bound on the total."""
    g = CovisibilityGraph(4096, 8192, 1000, device=-1)
    g.set_keyframe(1, np.full(8192, -1, np.int32))
    assert points_call(g, [1] * 4096)[0] == L.ORBFE_ERR_STATE               # 2^25 named slots: accepted
    st, r, buf = points_call(g, [1] * 4097)
    assert st == L.ORBFE_ERR_CAPACITY and r.n_points == -5 and (buf == -7).all()
    assert status(lambda: g.distinct_points([1] * 4097)) == L.ORBFE_ERR_CAPACITY
    assert status(lambda: g.distinct_points([1])) == L.ORBFE_ERR_STATE
    assert g.distinct_points([]).tolist() == []                              # the wrapper never sends an empty list


def geometry_args(n, ids=None, flags=0):
    rng = np.random.default_rng(n)
    return dict(point_ids=np.arange(n) if ids is None else ids, world_pos=rng.random((n, 3)), normal=rng.random((n, 3)),
                min_distance=rng.random(n), max_distance=rng.random(n) + 1, descriptors=rng.integers(0, 256, (n, 32)),
                flags=flags)


def test_set_point_geometry_checks():
    g = graph()
    g.set_point_geometry(**geometry_args(5))                                 # host-only: checked, nothing stored
    g.set_point_geometry(**geometry_args(0))
    g.set_point_geometry(**geometry_args(3, flags=[L.MPF_OBSERVED, L.MPF_PRESENT | L.MPF_OUTLIER, L.MPF_SKIP | 128]))
    g.set_point_geometry(**geometry_args(2, ids=[0, 999]))
    for f in (L.MPF_BAD, L.MPF_SEEN, L.MPF_TRACK_IN_VIEW, L.MPF_OBSERVED | L.MPF_SEEN):
        assert status(lambda: g.set_point_geometry(**geometry_args(2, flags=[0, f]))) == L.ORBFE_ERR_ARG
    assert status(lambda: g.set_point_geometry(**geometry_args(2, ids=[0, 1000]))) == L.ORBFE_ERR_ARG
    assert status(lambda: g.set_point_geometry(**geometry_args(2, ids=[-1, 4]))) == L.ORBFE_ERR_ARG
    assert status(lambda: g.set_point_geometry(**geometry_args(3, ids=[4, 6, 4]))) == L.ORBFE_ERR_ARG
    lib, ids, f = g._lib, np.asarray([1, 2], np.int32), np.zeros(2, np.uint8)
    x3, x1, d = np.zeros((2, 3), np.float32), np.zeros(2, np.float32), np.zeros((2, 32), np.uint8)
    full = [L.ptr(ids), L.ptr(f), L.ptr(x3), L.ptr(x3), L.ptr(x1), L.ptr(x1), L.ptr(d)]
    assert lib.orbfe_covis_set_point_geometry(None, 2, *full) == L.ORBFE_ERR_ARG
    assert lib.orbfe_covis_set_point_geometry(g._h, -1, *full) == L.ORBFE_ERR_ARG
    for k in range(7):                                                       # each array is required when n > 0
        args = list(full)
        args[k] = None
        assert lib.orbfe_covis_set_point_geometry(g._h, 2, *args) == L.ORBFE_ERR_ARG, k
    assert lib.orbfe_covis_set_point_geometry(g._h, 2, *full) == L.ORBFE_OK


def geometry_call(g, ids, seen, capacity=8):
    ids, seen = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(seen, np.int32)
    buf = np.full(max(capacity, 1), -7, np.int32)
    r = L.covis_local_geometry(point_capacity=capacity, n_points=-5, n_missing=-5, point_ids=L.ptr(buf))
    r.geometry.m = -5
    st = g._lib.orbfe_covis_local_geometry(g._h, len(ids), L.ptr(ids), len(seen), L.ptr(seen), byref(r))
    untouched = r.n_points == -5 and r.n_missing == -5 and r.geometry.m == -5 and (buf == -7).all()
    return st, untouched


def test_local_geometry_argument_checks():
    g = graph()
    assert geometry_call(g, [3, 5], [1, -1, 2, 2]) == (L.ORBFE_ERR_STATE, True)   # host-only, after the checks
    assert geometry_call(g, [3, 5], []) == (L.ORBFE_ERR_STATE, True)
    assert geometry_call(g, [], [1]) == (L.ORBFE_ERR_ARG, True)
    assert geometry_call(g, [3, 4], [1]) == (L.ORBFE_ERR_ARG, True)               # 4 is not stored
    assert geometry_call(g, [3] * 4097, [1]) == (L.ORBFE_ERR_CAPACITY, True)
    assert geometry_call(g, [3], [-2]) == (L.ORBFE_ERR_ARG, True)
    assert geometry_call(g, [3], [1000]) == (L.ORBFE_ERR_CAPACITY, True)          # at max_point_id, as in a vote list
    assert geometry_call(g, [3], [999]) == (L.ORBFE_ERR_STATE, True)
    assert geometry_call(g, [3], [1] * 8192) == (L.ORBFE_ERR_STATE, True)
    assert geometry_call(g, [3], [1] * 8193) == (L.ORBFE_ERR_CAPACITY, True)
    lib, ids = g._lib, np.asarray([3], np.int64)
    assert lib.orbfe_covis_local_geometry(g._h, 1, L.ptr(ids), 0, None, None) == L.ORBFE_ERR_ARG
    r = L.covis_local_geometry(point_capacity=0, point_ids=None)
    assert lib.orbfe_covis_local_geometry(None, 1, L.ptr(ids), 0, None, byref(r)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_covis_local_geometry(g._h, 1, L.ptr(ids), 2, None, byref(r)) == L.ORBFE_ERR_ARG  # a count, no list
    assert lib.orbfe_covis_local_geometry(g._h, 1, L.ptr(ids), -1, None, byref(r)) == L.ORBFE_ERR_ARG
    assert status(lambda: g.local_geometry([3], [1])) == L.ORBFE_ERR_STATE


def test_an_empty_list_gives_an_empty_map_and_staleness_is_an_error():
    g = graph()
    ids, lm = g.local_geometry([], [1, 2])
    assert ids.tolist() == [] and isinstance(lm, ResidentLocalMap) and len(lm) == 0 and lm.view().m == 0
    ids2, lm2 = g.local_geometry([])
    with pytest.raises(RuntimeError):
        lm.view()
    with pytest.raises(RuntimeError):
        lm.descriptors.data_ptr()
    assert lm2.view().m == 0
    g.close()
    with pytest.raises(RuntimeError):
        lm2.view()


def test_the_host_half_needs_the_vote():
    """update_local_keyframes starts with the device vote: on a host-only graph it stops there; the wrappers that only
    build a keyframe list run, and stop at the device walk."""
    g = graph()
    assert status(lambda: g.update_local_keyframes([1, 2])) == L.ORBFE_ERR_STATE
    assert status(lambda: g.update_local_map([1, 2])) == L.ORBFE_ERR_STATE
    ref = R.hand_graph(6)
    R.link(ref, 5, ordered=[1, 2])
    R.link(ref, 1, ordered=[5, 3, 4])
    R.link(ref, 2, ordered=[3, 5, 1])
    g = CovisibilityGraph(8, 4, 100, device=-1)
    for k in range(6):
        g.set_keyframe(k, [k])
    R.mirror_graph(ref, g)
    assert g.fuse_targets(5, False) == ref.fuse_targets(5, False) == [1, 3, 4, 2, 3]
    assert g.fuse_targets(5, True) == [1, 3, 4, 2, 3]
    assert g.fuse_targets(0, False) == []
    assert g.fuse_candidates(0, False).tolist() == []                       # no targets: no device call
    assert status(lambda: g.fuse_candidates(5, False)) == L.ORBFE_ERR_STATE
    assert status(lambda: g.loop_map_points(5)) == L.ORBFE_ERR_STATE
