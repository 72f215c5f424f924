"""The culling entry points of include/orbfe_covis.h on a host-only handle (device -1): every error path, each time
with nothing touched, and the attributes' life cycle; CovisibilityGraph.set_bad_flag's re-parenting on a host-only
graph against tests/culling_ref.py. CPU only."""
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

from orb_slam2_2021_amd import _lib as L
from orb_slam2_2021_amd import CovisibilityGraph

import culling_ref as C
from test_culling_ref import REPARENT, graph


class Handle:
    def __init__(self, max_keyframes=8, max_slots=16, max_point_id=100):
        self.lib = L.lib()
        self.h = c_void_p()
        assert self.lib.orbfe_covis_create(-1, max_keyframes, max_slots, max_point_id, byref(self.h)) == 0

    def __del__(self):
        self.lib.orbfe_covis_destroy(self.h)

    def size(self):
        n = c_int()
        assert self.lib.orbfe_covis_size(self.h, byref(n)) == 0
        return n.value

    def set_keyframe(self, kid, pts, key=None):
        a = np.ascontiguousarray(pts, np.int32)
        return self.lib.orbfe_covis_set_keyframe(self.h, kid, kid if key is None else key, len(a), L.ptr(a))

    def attrs(self, kid, attrs):
        a = np.ascontiguousarray(attrs, np.uint8)
        return self.lib.orbfe_covis_set_keyframe_attrs(self.h, kid, len(a), L.ptr(a))

    def cull(self, ids, not_erase=None, cap=None, mono=1):
        ids = np.ascontiguousarray(ids, np.int64)
        n = len(ids)
        ne = np.zeros(max(n, 1), np.uint8) if not_erase is None else np.ascontiguousarray(not_erase, np.uint8)
        cap = 16 * max(n, 1) if cap is None else cap
        self.out = [np.full(max(n, 1), 77, np.uint8), np.full(max(n, 1), 77, np.int32), np.full(max(n, 1), 77, np.int32),
                    np.full(n + 1, 77, np.int32), np.full(max(cap, 1), 77, np.int32)]
        r = L.covis_cull(decision=L.ptr(self.out[0]), n_mps=L.ptr(self.out[1]), n_redundant=L.ptr(self.out[2]),
                         bad_begin=L.ptr(self.out[3]), bad_points=L.ptr(self.out[4]), bad_capacity=cap)
        return self.lib.orbfe_covis_cull_keyframes(self.h, n, L.ptr(ids), L.ptr(ne), mono, byref(r))

    def untouched(self):
        return all((a == 77).all() for a in self.out)

    def cull_points(self, pts, first=None, cur=10, found=None, visible=None):
        p = np.ascontiguousarray(pts, np.int32)
        n = len(p)
        f = np.ones(max(n, 1), np.int32) if found is None else np.ascontiguousarray(found, np.int32)
        v = np.ones(max(n, 1), np.int32) if visible is None else np.ascontiguousarray(visible, np.int32)
        k = np.full(max(n, 1), 9, np.int64) if first is None else np.ascontiguousarray(first, np.int64)
        self.action = np.full(max(n, 1), 77, np.uint8)
        return self.lib.orbfe_covis_cull_points(self.h, n, L.ptr(p), L.ptr(f), L.ptr(v), L.ptr(k), cur, 1,
                                                L.ptr(self.action))


@pytest.fixture
def h():
    t = Handle()
    for kid in (1, 2, 3):
        assert t.set_keyframe(kid, [0, 1, 2, -1]) == 0
        assert t.attrs(kid, [0, 0x21, 0x47, 0]) == 0
    return t


def test_attrs_argument_rules(h):
    assert h.attrs(1, [0, 0, 0]) == L.ORBFE_ERR_ARG          # not the row's length
    assert h.attrs(1, [0, 0, 0, 0, 0]) == L.ORBFE_ERR_ARG
    assert h.attrs(9, [0, 0, 0, 0]) == L.ORBFE_ERR_STATE     # not stored
    assert h.attrs(1, [0, 0x80, 0, 0]) == L.ORBFE_ERR_ARG    # bit 7
    assert h.attrs(1, [0x7f, 0x7f, 0x7f, 0x7f]) == 0
    assert h.lib.orbfe_covis_set_keyframe_attrs(None, 1, 0, None) == L.ORBFE_ERR_ARG
    assert h.lib.orbfe_covis_set_keyframe_attrs(h.h, 1, 4, None) == L.ORBFE_ERR_ARG
    assert h.cull([1]) == L.ORBFE_ERR_STATE and h.size() == 3  # every check passed: host-only


def test_attrs_follow_the_keyframe(h):
    host_only = "host-only"

    def state():
        st = h.cull([1, 2])
        return "none" if st == L.ORBFE_ERR_STATE and host_only not in L.last_error() else st

    assert h.cull([1, 2]) == L.ORBFE_ERR_STATE and host_only in L.last_error()
    assert h.set_keyframe(2, [5, 6, 7, 8]) == 0               # same length: kept
    assert host_only in (h.cull([1, 2]), L.last_error())[1]
    assert h.set_keyframe(2, [5, 6, 7]) == 0                  # another length: dropped
    assert state() == "none" and h.untouched()
    assert h.cull_points([1]) == L.ORBFE_ERR_STATE and host_only not in L.last_error()
    assert h.attrs(2, [1, 2, 3]) == 0
    assert host_only in (h.cull([1, 2]), L.last_error())[1]
    assert h.lib.orbfe_covis_erase_keyframe(h.h, 2) == 0
    assert h.set_keyframe(2, [5, 6, 7]) == 0                  # erased and stored again: dropped
    assert state() == "none"
    assert h.lib.orbfe_covis_clear(h.h) == 0
    assert h.set_keyframe(1, [0, 1, 2, -1]) == 0 and h.set_keyframe(2, [0]) == 0
    assert state() == "none"


def test_cull_keyframes_argument_rules(h):
    assert h.cull([1, 9]) == L.ORBFE_ERR_ARG and h.untouched()        # not stored
    assert h.cull([1, 2, 1]) == L.ORBFE_ERR_ARG and h.untouched()     # named twice
    assert h.cull([1, 2], cap=7) == L.ORBFE_ERR_CAPACITY and h.untouched()
    assert h.cull([1, 2], cap=8) == L.ORBFE_ERR_STATE and "host-only" in L.last_error() and h.untouched()
    assert h.cull([], cap=0) == L.ORBFE_ERR_STATE and "host-only" in L.last_error()
    assert h.lib.orbfe_covis_cull_keyframes(h.h, 1, None, None, 1, None) == L.ORBFE_ERR_ARG
    assert h.set_keyframe(4, [3]) == 0                                # a stored keyframe without attributes
    assert h.cull([1, 2]) == L.ORBFE_ERR_STATE and "host-only" not in L.last_error() and h.untouched()
    assert h.cull([1, 9]) == L.ORBFE_ERR_ARG                          # the argument comes first
    assert h.size() == 4


def test_cull_points_argument_rules(h):
    assert h.cull_points([1, 2, 1]) == L.ORBFE_ERR_ARG and (h.action == 77).all()   # named twice
    assert h.cull_points([-1]) == L.ORBFE_ERR_ARG and (h.action == 77).all()
    assert h.cull_points([100]) == L.ORBFE_ERR_ARG                                   # max_point_id
    assert h.cull_points([1], first=[1 << 31]) == L.ORBFE_ERR_ARG
    assert h.cull_points([1], first=[-1]) == L.ORBFE_ERR_ARG
    assert h.cull_points([1], cur=1 << 31) == L.ORBFE_ERR_ARG
    assert h.cull_points([1], first=[(1 << 31) - 1], cur=(1 << 31) - 1) == L.ORBFE_ERR_STATE
    assert "host-only" in L.last_error() and (h.action == 77).all()
    assert h.cull_points([99, 0]) == L.ORBFE_ERR_STATE and "host-only" in L.last_error()
    assert h.lib.orbfe_covis_cull_points(h.h, 1, None, None, None, None, 1, 1, None) == L.ORBFE_ERR_ARG
    assert h.set_keyframe(4, [3]) == 0
    assert h.cull_points([1]) == L.ORBFE_ERR_STATE and "host-only" not in L.last_error()


def test_pack_attrs_compares_in_float32():
    th = np.float32(40.0)
    above = np.nextafter(th, np.float32(100))
    a = CovisibilityGraph.pack_attrs([0, 31, 5, 5, 5], [-1.0, 0.0, -0.0, 3.5, np.float32(-1e-30)],
                                     [th, above, -0.0, np.float32(-1e-30), 40.0000001], th)
    # 40.0000001 rounds to 40 in float32: not far; -0.0 is not < 0; -1e-30 is
    assert a.tolist() == [0, 31 | 0x20 | 0x40, 5 | 0x20, 5 | 0x20 | 0x40, 5]
    with pytest.raises(ValueError):
        CovisibilityGraph.pack_attrs([32], [0], [0], 1)


def host_graph(ref):
    g = CovisibilityGraph(16, 4, 10, device=-1)
    for i, kf in ref.kfs.items():
        g.set_keyframe(i, [])
    for i, kf in ref.kfs.items():
        n = g._nodes[i]
        n.weights = dict(kf.mConnectedKeyFrameWeights)
        n.ordered = list(kf.mvpOrderedConnectedKeyFrames)
        n.ordered_weights = list(kf.mvOrderedWeights)
        n.parent = kf.mpParent
        n.children = set(kf.mspChildrens)
        n.first_connection = False
    return g


@pytest.mark.parametrize("name", sorted(REPARENT))
def test_set_bad_flag_on_the_graph(name):
    spec, want = REPARENT[name]
    ref = graph(**spec)
    g = host_graph(ref)
    ref.set_bad_flag(5)
    g.set_bad_flag(5)
    assert 5 not in g and len(g) == len(ref)
    for i in ref.kfs:
        got = ({k: g.GetWeight(i, k) for k in g.GetConnectedKeyFrames(i)}, g.GetVectorCovisibleKeyFrames(i),
               g.GetOrderedWeights(i), g.GetParent(i), g.GetChilds(i), g._nodes[i].first_connection)
        assert got == ref.state(i), i
    for child, parent in want.items():
        assert g.GetParent(child) == parent


def test_set_bad_flag_leaves_keyframe_0_and_erase_keeps_its_contract():
    ref = graph(links={(0, 1): 20, (1, 2): 20, (0, 2): 10}, parents={1: 0, 2: 1})
    g = host_graph(ref)
    g.set_bad_flag(0)
    assert 0 in g and len(g) == 3
    g.erase(1)  # no re-parenting: 2 keeps naming 1
    assert g.GetParent(2) == 1 and 1 not in g.GetChilds(0)
    with pytest.raises(KeyError):
        g.set_bad_flag(1)
