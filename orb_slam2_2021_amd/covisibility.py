"""The covisibility graph on MI355X (include/orbfe_covis.h): the keyframes' mvpMapPoints rows stay on
the device, and KeyFrame::UpdateConnections, Tracking::UpdateLocalKeyFrames' vote and
LocalBundleAdjustment's gather run over them there.

`CovisibilityGraph` owns the device table and the graph state the reference keeps in KeyFrame
(mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights, mpParent, mspChildrens,
mbFirstConnection). The device returns the counts and orders of src/KeyFrame.cc:304-378; the side
effects (:360-392, AddConnection / UpdateBestCovisibles at :122-157) are applied here on the host,
keyframe by keyframe. LocalMapping::KeyFrameCulling and MapPointCulling run over the same table
(keyframe_culling, map_point_culling); what KeyFrame::SetBadFlag does to the graph and the spanning
tree is applied here (set_bad_flag). Keyframes are named by mnId; every order among equal weights is the tie
key's (the reference's KeyFrame* value; mnId unless given).

The local map (include/orbfe_localmap.h): distinct_points is the walk of Tracking::UpdateLocalPoints,
SearchInNeighbors' vpFuseCandidates and ComputeSim3's mvpLoopMapPoints on the device; set_point_geometry feeds the
per-point store and local_geometry gathers the walk's points from it into a ResidentLocalMap that stays in HBM;
update_local_keyframes adds the host half of Tracking::UpdateLocalKeyFrames (Tracking.cc:1306-1365) to the vote, and
update_local_map runs them for one Frame.
"""
from __future__ import annotations

from ctypes import byref, c_int, c_void_p
from types import SimpleNamespace
from typing import Dict, Iterable, List, Optional, Sequence, Set, Tuple

import numpy as np

from . import _lib as L
from .frames import ResidentLocalMap


class _Node:
    """One keyframe's graph state."""

    __slots__ = ("tie_key", "weights", "ordered", "ordered_weights", "parent", "children", "first_connection")

    def __init__(self, tie_key: int):
        self.tie_key = tie_key
        self.weights: Dict[int, int] = {}      # mConnectedKeyFrameWeights
        self.ordered: List[int] = []           # mvpOrderedConnectedKeyFrames
        self.ordered_weights: List[int] = []   # mvOrderedWeights
        self.parent: Optional[int] = None      # mpParent
        self.children: Set[int] = set()        # mspChildrens
        self.first_connection = True           # mbFirstConnection


class CovisibilityGraph:
    def __init__(self, max_keyframes: int = 4096, max_slots: int = 2048, max_point_id: int = 1 << 20, kfdb=None,
                 device: int = 0):
        self._lib = L.lib()
        h = c_void_p()
        L.check(self._lib.orbfe_covis_create(int(device), int(max_keyframes), int(max_slots), int(max_point_id),
                                             byref(h)), "orbfe_covis_create")
        self._h = h
        self._max_slots = int(max_slots)
        self._max_point_id = int(max_point_id)
        self._local_generation = 0  # local_geometry calls so far: a ResidentLocalMap of an earlier one is stale
        self._pt_buf = np.zeros(65536, np.int32)
        self._kfdb = kfdb
        self._nodes: Dict[int, _Node] = {}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_covis_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = c_int()
        L.check(self._lib.orbfe_covis_size(self._h, byref(n)), "orbfe_covis_size")
        return n.value

    def __contains__(self, kf_id: int) -> bool:
        return int(kf_id) in self._nodes

    # ---- the table ----------------------------------------------------------------------------
    def set_keyframe(self, kf_id: int, point_ids, tie_key: Optional[int] = None) -> None:
        """Adds a keyframe with its mvpMapPoints (point mnId per keypoint, -1 for none), or replaces a stored
        keyframe's whole row. tie_key stands for the reference's KeyFrame* (default: mnId)."""
        kf_id = int(kf_id)
        ids = np.ascontiguousarray(point_ids, np.int32)
        node = self._nodes.get(kf_id)
        key = int(tie_key) if tie_key is not None else (node.tie_key if node else kf_id)
        L.check(self._lib.orbfe_covis_set_keyframe(self._h, kf_id, key, len(ids), L.ptr(ids)),
                "orbfe_covis_set_keyframe")
        if node is None:
            self._nodes[kf_id] = _Node(key)
        else:
            node.tie_key = key

    def set_slots(self, kf_id: int, slots, point_ids) -> None:
        """AddMapPoint / EraseMapPointMatch (-1) / ReplaceMapPointMatch on the given slots."""
        s = np.ascontiguousarray(slots, np.int32)
        p = np.ascontiguousarray(point_ids, np.int32)
        if len(s) != len(p):
            raise ValueError("slots / point_ids differ in length")
        L.check(self._lib.orbfe_covis_set_slots(self._h, int(kf_id), len(s), L.ptr(s), L.ptr(p)),
                "orbfe_covis_set_slots")

    def set_points_bad(self, point_ids, bad: bool = True) -> None:
        p = np.ascontiguousarray(point_ids, np.int32)
        L.check(self._lib.orbfe_covis_set_points_bad(self._h, len(p), L.ptr(p), 1 if bad else 0),
                "orbfe_covis_set_points_bad")

    def erase(self, kf_id: int) -> None:
        """Removes the keyframe's row and applies EraseConnection on every connected keyframe
        (KeyFrame.cc:482-484, :570-584); the keyframe leaves its parent's children (:555). The spanning-tree
        re-parenting of KeyFrame::SetBadFlag (:496-553) is out of scope: the erased keyframe's children keep naming
        it as their parent until the caller assigns another."""
        kf_id = int(kf_id)
        L.check(self._lib.orbfe_covis_erase_keyframe(self._h, kf_id), "orbfe_covis_erase_keyframe")
        node = self._nodes.pop(kf_id)
        before = {}
        for other in sorted(node.weights, key=lambda i: self._nodes[i].tie_key if i in self._nodes else i):
            o = self._nodes.get(other)
            if o is not None and kf_id in o.weights:  # EraseConnection
                before.setdefault(other, list(o.ordered))
                del o.weights[kf_id]
                self._update_best_covisibles(o)
        if node.parent is not None and node.parent in self._nodes:
            self._nodes[node.parent].children.discard(kf_id)
        self._mirror(before)

    def clear(self) -> None:
        L.check(self._lib.orbfe_covis_clear(self._h), "orbfe_covis_clear")
        self._nodes.clear()

    # ---- culling ------------------------------------------------------------------------------
    @staticmethod
    def pack_attrs(octaves, u_right, depth, th_depth) -> np.ndarray:
        """The attribute byte per keypoint: octave | STEREO (mvuRight[i] >= 0) | FAR (mvDepth[i] > mThDepth ||
        mvDepth[i] < 0), the compares in float32 as the reference makes them."""
        o = np.asarray(octaves, np.int64).reshape(-1)
        if len(o) and (o.min() < 0 or o.max() > 31):
            raise ValueError("octave outside 0..31")
        ur = np.asarray(u_right, np.float32).reshape(-1)
        d = np.asarray(depth, np.float32).reshape(-1)
        if not len(o) == len(ur) == len(d):
            raise ValueError("octaves / u_right / depth differ in length")
        th = np.float32(th_depth)
        far = (d > th) | (d < np.float32(0))
        return np.ascontiguousarray(o.astype(np.uint8) | (np.uint8(0x20) * (ur >= np.float32(0)))
                                    | (np.uint8(0x40) * far), np.uint8)

    def set_keyframe_attrs(self, kf_id: int, octaves, u_right, depth, th_depth) -> None:
        """What the cullings read of a stored keyframe's keypoints (mvKeysUn[i].octave, mvuRight, mvDepth against
        mThDepth), one byte per slot. A keyframe's keypoints never change: once per keyframe is enough."""
        a = self.pack_attrs(octaves, u_right, depth, th_depth)
        L.check(self._lib.orbfe_covis_set_keyframe_attrs(self._h, int(kf_id), len(a), L.ptr(a)),
                "orbfe_covis_set_keyframe_attrs")

    def map_point_culling(self, point_ids, found, visible, first_kf_ids, current_kf_id: int,
                          monocular: bool) -> np.ndarray:
        """LocalMapping::MapPointCulling (LocalMapping.cc:174-209) over mlpRecentAddedMapPoints: per point 0 stays in
        the list, 1 leaves (was bad), 2 set bad (found ratio), 3 set bad (observations), 4 leaves (age). Points set
        bad are flagged in the table and erased from their observers' rows."""
        p = np.ascontiguousarray(point_ids, np.int32)
        f = np.ascontiguousarray(found, np.int32)
        v = np.ascontiguousarray(visible, np.int32)
        k = np.ascontiguousarray(first_kf_ids, np.int64)
        if not len(p) == len(f) == len(v) == len(k):
            raise ValueError("point_ids / found / visible / first_kf_ids differ in length")
        action = np.zeros(max(len(p), 1), np.uint8)
        L.check(self._lib.orbfe_covis_cull_points(self._h, len(p), L.ptr(p), L.ptr(f), L.ptr(v), L.ptr(k),
                                                  int(current_kf_id), 1 if monocular else 0, L.ptr(action)),
                "orbfe_covis_cull_points")
        return action[:len(p)]

    def cull_keyframes(self, kf_ids: Sequence[int], monocular: bool, not_erase=None) -> SimpleNamespace:
        """orbfe_covis_cull_keyframes over the candidates in the given order, the table pruned and no graph state
        touched: decision, n_mps, n_redundant per candidate and bad_points, one list per candidate."""
        ids = np.ascontiguousarray(list(kf_ids), np.int64)
        n = len(ids)
        ne = np.zeros(max(n, 1), np.uint8) if not_erase is None else np.ascontiguousarray(not_erase, np.uint8)
        if not_erase is not None and len(ne) != n:
            raise ValueError("kf_ids / not_erase differ in length")
        m = max(n, 1)
        cap = max(n * self._max_slots, 1)
        dec, mps, red = np.zeros(m, np.uint8), np.zeros(m, np.int32), np.zeros(m, np.int32)
        beg, pts = np.zeros(m + 1, np.int32), np.zeros(cap, np.int32)
        r = L.covis_cull(decision=L.ptr(dec), n_mps=L.ptr(mps), n_redundant=L.ptr(red), bad_begin=L.ptr(beg),
                         bad_points=L.ptr(pts), bad_capacity=cap)
        L.check(self._lib.orbfe_covis_cull_keyframes(self._h, n, L.ptr(ids), L.ptr(ne), 1 if monocular else 0,
                                                     byref(r)), "orbfe_covis_cull_keyframes")
        return SimpleNamespace(decision=dec[:n].tolist(), n_mps=mps[:n].tolist(), n_redundant=red[:n].tolist(),
                               bad_points=[pts[beg[i]:beg[i + 1]].tolist() for i in range(n)])

    def keyframe_culling(self, kf_id: int, monocular: bool, not_erase=()) -> SimpleNamespace:
        """LocalMapping::KeyFrameCulling (LocalMapping.cc:640-706) for mpCurrentKeyFrame = kf_id: the candidates are
        GetVectorCovisibleKeyFrames(kf_id), `not_erase` the ids among them with mbNotErase. One device call decides
        them in order and prunes the table; then, for each culled keyframe in order, the rest of
        KeyFrame::SetBadFlag runs on the host graph (set_bad_flag's graph part). Returns the device's result with
        kf_ids, culled (ids, in order) and to_be_erased (redundant but not_erase: the reference's mbToBeErased).
        Poses are not graph state: mTcp = Tcw * parent's Twc (KeyFrame.cc:556) stays with the caller, who reads
        GetParent before this call."""
        cand = self.GetVectorCovisibleKeyFrames(kf_id)
        hold = {int(i) for i in not_erase}
        res = self.cull_keyframes(cand, monocular, [1 if i in hold else 0 for i in cand])
        res.kf_ids = cand
        res.culled = [i for i, d in zip(cand, res.decision) if d == 1]
        res.to_be_erased = [i for i, d in zip(cand, res.decision) if d == 2]
        before: Dict[int, List[int]] = {}
        for i in res.culled:
            self._set_bad_flag_graph(i, before)
        self._mirror(before)
        return res

    def set_bad_flag(self, kf_id: int) -> None:
        """KeyFrame::SetBadFlag (KeyFrame.cc:469-562) on the graph: EraseConnection on the connected keyframes, the
        spanning-tree re-parenting of :496-553 in the reference's iteration orders, EraseChild, the database's
        erase and the mirror. The keyframe's row leaves the table as by orbfe_covis_erase_keyframe; the
        EraseObservation cascade on the points (:486-488) belongs to keyframe_culling, which runs it on the device.
        mnId 0 is left alone (:473). mbNotErase and mTcp stay with the caller."""
        kf_id = int(kf_id)
        if kf_id == 0:
            return
        if kf_id not in self._nodes:
            raise KeyError(kf_id)
        L.check(self._lib.orbfe_covis_erase_keyframe(self._h, kf_id), "orbfe_covis_erase_keyframe")
        before: Dict[int, List[int]] = {}
        self._set_bad_flag_graph(kf_id, before)
        self._mirror(before)

    def _set_bad_flag_graph(self, kf_id: int, before: Dict[int, List[int]]) -> None:
        node = self._nodes.pop(kf_id)
        for other in sorted(node.weights, key=self._tie):  # :482-484, the map's iteration order
            o = self._nodes.get(other)
            if o is not None and kf_id in o.weights:
                before.setdefault(other, list(o.ordered))
                del o.weights[kf_id]
                self._update_best_covisibles(o)
        # :496-553. A set<KeyFrame*> iterates in tie-key order.
        candidates = set() if node.parent is None else {node.parent}
        children = {c for c in node.children if c in self._nodes}  # isBad() children are passed over for good
        while children:
            best, child, parent = -1, None, None
            for c in sorted(children, key=self._tie):
                cn = self._nodes[c]
                for v in cn.ordered:
                    for pc in sorted(candidates, key=self._tie):
                        if v == pc:
                            w = cn.weights.get(v, 0)
                            if w > best:
                                best, child, parent = w, c, v
            if child is None:
                break
            self._change_parent(child, parent)
            candidates.add(child)
            children.discard(child)
        for c in sorted(children, key=self._tie):  # :549-553
            self._change_parent(c, node.parent)
        if node.parent is not None and node.parent in self._nodes:
            self._nodes[node.parent].children.discard(kf_id)  # :555
        if self._kfdb is not None:  # :561
            try:
                self._kfdb.erase(kf_id)
            except L.OrbfeError as e:
                if e.status != L.ORBFE_ERR_STATE:  # the database never held it
                    raise

    def _change_parent(self, child: int, parent: Optional[int]) -> None:
        """KeyFrame.cc:412-417"""
        self._nodes[child].parent = parent
        if parent is not None and parent in self._nodes:
            self._nodes[parent].children.add(child)

    # ---- device queries -----------------------------------------------------------------------
    def count_connections(self, kf_ids: Sequence[int], th: int = 15) -> List[SimpleNamespace]:
        """orbfe_covis_update_connections for a batch, no side effects: per keyframe counter_ids /
        counter_weights (KFcounter, ascending tie key), ordered_ids / ordered_weights, nmax, kf_max, unchanged."""
        ids = np.ascontiguousarray(list(kf_ids), np.int64)
        n, cap = len(ids), max(len(self) - 1, 1)
        m = max(n, 1)
        n_counter, n_ordered, nmax = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        kf_max, unchanged = np.zeros(m, np.int64), np.zeros(m, np.uint8)
        c_ids, c_w = np.zeros(m * cap, np.int64), np.zeros(m * cap, np.int32)
        o_ids, o_w = np.zeros(m * cap, np.int64), np.zeros(m * cap, np.int32)
        r = L.covis_connections(capacity=cap, n_counter=L.ptr(n_counter), counter_ids=L.ptr(c_ids),
                                counter_weights=L.ptr(c_w), n_ordered=L.ptr(n_ordered), ordered_ids=L.ptr(o_ids),
                                ordered_weights=L.ptr(o_w), nmax=L.ptr(nmax), kf_max=L.ptr(kf_max),
                                unchanged=L.ptr(unchanged))
        L.check(self._lib.orbfe_covis_update_connections(self._h, n, L.ptr(ids), int(th), byref(r)),
                "orbfe_covis_update_connections")
        out = []
        for q in range(n):
            b, nc, no = q * cap, int(n_counter[q]), int(n_ordered[q])
            out.append(SimpleNamespace(counter_ids=c_ids[b:b + nc].tolist(), counter_weights=c_w[b:b + nc].tolist(),
                                       ordered_ids=o_ids[b:b + no].tolist(), ordered_weights=o_w[b:b + no].tolist(),
                                       nmax=int(nmax[q]), kf_max=int(kf_max[q]), unchanged=bool(unchanged[q])))
        return out

    def vote(self, point_lists: Sequence[Iterable[int]]) -> List[SimpleNamespace]:
        """The first half of Tracking::UpdateLocalKeyFrames (Tracking.cc:1257-1303) for a batch of Frames, each given
        as its mvpMapPoints (point mnIds; -1 and bad points are skipped): per Frame kf_ids (ascending tie key:
        mvpLocalKeyFrames' initial content), counts, max, kf_max (-1 when nothing was voted)."""
        lists = [np.asarray(list(p), np.int32).reshape(-1) for p in point_lists]
        nq = len(lists)
        begin = np.zeros(nq + 1, np.int32)
        if nq:
            begin[1:] = np.cumsum([len(p) for p in lists])
        pts = np.ascontiguousarray(np.concatenate(lists) if nq and begin[-1] else np.zeros(1, np.int32), np.int32)
        cap, m = max(len(self), 1), max(nq, 1)
        n, mx, kf_max = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int64)
        ids, counts = np.zeros(m * cap, np.int64), np.zeros(m * cap, np.int32)
        r = L.covis_votes(capacity=cap, n=L.ptr(n), kf_ids=L.ptr(ids), counts=L.ptr(counts), max=L.ptr(mx),
                          kf_max=L.ptr(kf_max))
        L.check(self._lib.orbfe_covis_vote(self._h, nq, L.ptr(begin), L.ptr(pts), byref(r)), "orbfe_covis_vote")
        return [SimpleNamespace(kf_ids=ids[q * cap:q * cap + int(n[q])].tolist(),
                                counts=counts[q * cap:q * cap + int(n[q])].tolist(), max=int(mx[q]),
                                kf_max=int(kf_max[q])) for q in range(nq)]

    def gather_local_map(self, local_ids: Iterable[int]) -> SimpleNamespace:
        """orbfe_covis_local_map: point_ids (ascending), fixed_ids (ascending mnId), edge_begin, edge_kf (index into
        sorted(local_ids) + fixed_ids), edge_slot. The capacities grow to what the gather reports."""
        ids = np.ascontiguousarray(list(local_ids), np.int64)
        pc, fc, ec = 4096, max(len(self), 1), 32768
        for _ in range(2):
            pts, fixed = np.zeros(max(pc, 1), np.int32), np.zeros(max(fc, 1), np.int64)
            ebeg, ekf, esl = np.zeros(pc + 1, np.int32), np.zeros(max(ec, 1), np.int32), np.zeros(max(ec, 1), np.int32)
            r = L.covis_local_map(point_capacity=pc, fixed_capacity=fc, edge_capacity=ec, point_ids=L.ptr(pts),
                                  fixed_ids=L.ptr(fixed), edge_begin=L.ptr(ebeg), edge_kf=L.ptr(ekf),
                                  edge_slot=L.ptr(esl))
            st = self._lib.orbfe_covis_local_map(self._h, len(ids), L.ptr(ids), byref(r))
            if st == L.ORBFE_ERR_CAPACITY and (r.n_points > pc or r.n_fixed > fc or r.n_edges > ec):
                pc, fc, ec = max(pc, r.n_points), max(fc, r.n_fixed), max(ec, r.n_edges)
                continue
            L.check(st, "orbfe_covis_local_map")
            break
        else:
            L.check(st, "orbfe_covis_local_map")
        return SimpleNamespace(point_ids=pts[:r.n_points].copy(), fixed_ids=fixed[:r.n_fixed].copy(),
                               edge_begin=ebeg[:r.n_points + 1].copy(), edge_kf=ekf[:r.n_edges].copy(),
                               edge_slot=esl[:r.n_edges].copy())

    # ---- the local map (include/orbfe_localmap.h) ------------------------------------------------
    def _point_buffer(self, need: int) -> np.ndarray:
        if need > len(self._pt_buf):
            self._pt_buf = np.zeros(max(need, 2 * len(self._pt_buf)), np.int32)
        return self._pt_buf

    def distinct_points(self, kf_ids: Iterable[int]) -> np.ndarray:
        """orbfe_covis_distinct_points: the non-bad points in the rows of kf_ids (repeats allowed), each once, in
        first-occurrence order over (list position, slot) -- the reference's push_back order at Tracking.cc:1228-1252,
        LocalMapping.cc:500-521 and LoopClosing.cc:371-391. An empty list gives an empty result."""
        ids = np.ascontiguousarray(list(kf_ids), np.int64)
        if len(ids) == 0:
            return np.zeros(0, np.int32)
        for _ in range(2):
            buf = self._pt_buf
            r = L.covis_points(point_capacity=len(buf), n_points=0, point_ids=L.ptr(buf))
            st = self._lib.orbfe_covis_distinct_points(self._h, len(ids), L.ptr(ids), byref(r))
            if st == L.ORBFE_ERR_CAPACITY and r.n_points > len(buf):
                self._point_buffer(r.n_points)
                continue
            break
        L.check(st, "orbfe_covis_distinct_points")
        return buf[:r.n_points].copy()

    def set_point_geometry(self, point_ids, world_pos, normal, min_distance, max_distance, descriptors,
                           flags=0) -> None:
        """Creates or overwrites the stored geometry of the given points (SetWorldPos, UpdateNormalAndDepth,
        ComputeDistinctiveDescriptors as the caller mirrors them). flags: the bits handed on with each point
        (MPF_OBSERVED, ...), one per point or one for all; MPF_BAD, MPF_SEEN and MPF_TRACK_IN_VIEW are refused."""
        p = np.ascontiguousarray(point_ids, np.int32).reshape(-1)
        n = len(p)
        f = np.ascontiguousarray(np.broadcast_to(np.asarray(flags, np.uint8), (n,)))
        wp = np.ascontiguousarray(world_pos, np.float32).reshape(n, 3)
        nr = np.ascontiguousarray(normal, np.float32).reshape(n, 3)
        mn = np.ascontiguousarray(min_distance, np.float32).reshape(n)
        mx = np.ascontiguousarray(max_distance, np.float32).reshape(n)
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(n, 32)
        L.check(self._lib.orbfe_covis_set_point_geometry(self._h, n, L.ptr(p), L.ptr(f), L.ptr(wp), L.ptr(nr),
                                                         L.ptr(mn), L.ptr(mx), L.ptr(d)),
                "orbfe_covis_set_point_geometry")

    def local_geometry(self, kf_ids: Iterable[int], seen_point_ids=()) -> Tuple[np.ndarray, ResidentLocalMap]:
        """orbfe_covis_local_geometry: distinct_points(kf_ids) and, gathered on the device from the store, the
        MapPointGeometry of those points with MPF_SEEN on the ones in seen_point_ids (the Frame's mvpMapPoints; -1
        and bad points skipped). Returns (point_ids, ResidentLocalMap); entry i of the map is point_ids[i]. Earlier
        ResidentLocalMaps of this graph become stale. A point whose geometry was never set: OrbfeError with status
        ORBFE_ERR_STATE and the attribute n_missing."""
        ids = np.ascontiguousarray(list(kf_ids), np.int64)
        seen = np.ascontiguousarray(seen_point_ids, np.int32).reshape(-1)
        self._local_generation += 1
        if len(ids) == 0:
            return np.zeros(0, np.int32), ResidentLocalMap(self, self._local_generation, L.mappoint_geometry())
        for _ in range(2):
            buf = self._pt_buf
            r = L.covis_local_geometry(point_capacity=len(buf), point_ids=L.ptr(buf))
            st = self._lib.orbfe_covis_local_geometry(self._h, len(ids), L.ptr(ids), len(seen), L.ptr(seen),
                                                      byref(r))
            if st == L.ORBFE_ERR_CAPACITY and r.n_points > len(buf):
                self._point_buffer(r.n_points)
                continue
            break
        if st < 0:
            e = L.OrbfeError(st, "orbfe_covis_local_geometry")
            e.n_missing = int(r.n_missing)
            raise e
        return buf[:r.n_points].copy(), ResidentLocalMap(self, self._local_generation, r.geometry)

    def update_local_keyframes(self, frame_point_ids) -> Optional[Tuple[List[int], int]]:
        """Tracking::UpdateLocalKeyFrames (Tracking.cc:1254-1366) for a Frame given as its mvpMapPoints: the vote on
        the device, then :1306-1365 on the host from the graph state. Returns (local_kf_ids in mvpLocalKeyFrames'
        order, reference_kf = pKFmax), or None when nothing was voted (:1277-1278: the caller keeps its lists).
        The loop runs over the voted keyframes only (itEndKF is taken before the pushes); the > 80 test comes first in
        each turn; per turn the first not-yet-included of GetBestCovisibilityKeyFrames(10), then the first
        not-yet-included child in tie-key order (set<KeyFrame*>), then the parent, whose break (:1355) ends the whole
        loop. Bad keyframes are in neither the table nor the graph, so the reference's isBad() tests are vacuous
        here; a parent id that erase() left dangling is passed over like a NULL parent."""
        v = self.vote([frame_point_ids])[0]
        if not v.kf_ids:
            return None
        local = list(v.kf_ids)
        included = set(local)  # mnTrackReferenceForFrame == mCurrentFrame.mnId
        for kf in v.kf_ids:
            if len(local) > 80:
                break
            node = self._nodes[kf]
            for nb in node.ordered[:10]:
                if nb in self._nodes and nb not in included:
                    local.append(nb)
                    included.add(nb)
                    break
            for ch in sorted(node.children, key=self._tie):
                if ch in self._nodes and ch not in included:
                    local.append(ch)
                    included.add(ch)
                    break
            par = node.parent
            if par is not None and par in self._nodes and par not in included:
                local.append(par)
                included.add(par)
                break
        return local, v.kf_max

    def update_local_map(self, frame_point_ids) -> Optional[SimpleNamespace]:
        """Tracking::UpdateLocalMap for one Frame (its mvpMapPoints as point ids): update_local_keyframes, then
        UpdateLocalPoints with the geometry (local_geometry, the Frame's own points marked MPF_SEEN). Returns
        local_kf_ids, reference_kf, point_ids and local_map (a ResidentLocalMap for ORBmatcher.SearchLocalPoints), or
        None when nothing was voted."""
        r = self.update_local_keyframes(frame_point_ids)
        if r is None:
            return None
        point_ids, local_map = self.local_geometry(r[0], frame_point_ids)
        return SimpleNamespace(local_kf_ids=r[0], reference_kf=r[1], point_ids=point_ids, local_map=local_map)

    def fuse_targets(self, kf_id: int, monocular: bool) -> List[int]:
        """vpTargetKFs of LocalMapping::SearchInNeighbors (LocalMapping.cc:463-486): the best 20 (monocular) or 10
        neighbours, each followed by its own best 5 that are neither stamped nor the keyframe itself. Second
        neighbours are not stamped (mnFuseTargetForKF is set at :473 only), so one can appear more than once: the
        repeats are kept."""
        kf_id = int(kf_id)
        targets: List[int] = []
        stamped: Set[int] = set()
        for k in self.GetBestCovisibilityKeyFrames(kf_id, 20 if monocular else 10):
            if k not in self._nodes or k in stamped:
                continue
            targets.append(k)
            stamped.add(k)
            for k2 in self.GetBestCovisibilityKeyFrames(k, 5):
                if k2 not in self._nodes or k2 in stamped or k2 == kf_id:
                    continue
                targets.append(k2)
        return targets

    def fuse_candidates(self, kf_id: int, monocular: bool) -> np.ndarray:
        """vpFuseCandidates (LocalMapping.cc:500-521): distinct_points over fuse_targets."""
        return self.distinct_points(self.fuse_targets(kf_id, monocular))

    def loop_map_points(self, matched_kf_id: int) -> np.ndarray:
        """mvpLoopMapPoints (LoopClosing.cc:372-391): distinct_points over the matched keyframe's
        GetVectorCovisibleKeyFrames() followed by the keyframe itself."""
        k = int(matched_kf_id)
        return self.distinct_points(self.GetVectorCovisibleKeyFrames(k) + [k])

    # ---- the reference's side effects ----------------------------------------------------------
    def _update_best_covisibles(self, node: _Node) -> None:
        """KeyFrame.cc:137-157: sort the pairs (weight, KeyFrame*) ascending, push_front each."""
        pairs = sorted((w, self._tie(i), i) for i, w in node.weights.items())
        pairs.reverse()
        node.ordered = [i for _, _, i in pairs]
        node.ordered_weights = [w for w, _, _ in pairs]

    def _tie(self, kf_id: int) -> int:
        n = self._nodes.get(kf_id)
        return n.tie_key if n is not None else kf_id

    def _add_connection(self, node: _Node, other: int, weight: int) -> bool:
        """KeyFrame.cc:122-135; True when the ordered list was rebuilt."""
        if node.weights.get(other) == weight:
            return False
        node.weights[other] = weight
        self._update_best_covisibles(node)  # the whole map, entries below th included
        return True

    def _mirror(self, before: Dict[int, List[int]]) -> None:
        """GetBestCovisibilityKeyFrames(10) of every keyframe whose ordered list differs from `before` to the
        KeyFrameDatabase, in the order the lists were first touched. A keyframe the database does not hold yet is
        skipped: mirror() it after KeyFrameDatabase.add."""
        if self._kfdb is None:
            return
        for kid, old in before.items():
            node = self._nodes.get(kid)
            if node is not None and node.ordered != old:
                self.mirror(kid)

    def mirror(self, kf_id: int) -> bool:
        """kfdb.set_covisible(kf_id, GetBestCovisibilityKeyFrames(10)); False when the database does not hold it."""
        try:
            self._kfdb.set_covisible(int(kf_id), self.GetBestCovisibilityKeyFrames(kf_id, 10))
        except L.OrbfeError as e:
            if e.status != L.ORBFE_ERR_STATE:
                raise
            return False
        return True

    def _apply(self, kf_id: int, c: SimpleNamespace, before: Dict[int, List[int]]) -> None:
        node = self._nodes[kf_id]
        if c.unchanged:  # :339
            return
        # :360 / :367, in KFcounter's iteration order (ascending tie key)
        for other, w in sorted(zip(c.ordered_ids, c.ordered_weights), key=lambda t: self._tie(t[0])):
            o = self._nodes[other]
            before.setdefault(other, list(o.ordered))
            self._add_connection(o, kf_id, w)
        before.setdefault(kf_id, list(node.ordered))
        node.weights = dict(zip(c.counter_ids, c.counter_weights))  # :383-385
        node.ordered = list(c.ordered_ids)
        node.ordered_weights = list(c.ordered_weights)
        if node.first_connection and kf_id != 0:  # :387-392
            node.parent = node.ordered[0]
            self._nodes[node.parent].children.add(kf_id)
            node.first_connection = False

    def update_connections(self, kf_ids, th: int = 15) -> None:
        """KeyFrame::UpdateConnections of each keyframe: one device call for the counts, then the side effects on the
        host in the given order."""
        ids = [int(kf_ids)] if np.isscalar(kf_ids) else [int(i) for i in kf_ids]
        before: Dict[int, List[int]] = {}
        for kid, c in zip(ids, self.count_connections(ids, th)):
            self._apply(kid, c, before)
        self._mirror(before)

    def loop_connections(self, connected_ids: Sequence[int], th: int = 15) -> Dict[int, Set[int]]:
        """LoopClosing.cc:565-587 over mvpCurrentConnectedKFs: UpdateConnections of each, and per keyframe its new
        connected set minus its previous ordered neighbours and minus the list itself (the LoopConnections that
        essential_graph.py takes)."""
        ids = [int(i) for i in connected_ids]
        before: Dict[int, List[int]] = {}
        out: Dict[int, Set[int]] = {}
        for kid, c in zip(ids, self.count_connections(ids, th)):
            previous = self.GetVectorCovisibleKeyFrames(kid)  # :571, before this keyframe's update
            self._apply(kid, c, before)
            out[kid] = self.GetConnectedKeyFrames(kid) - set(previous) - set(ids)
        self._mirror(before)
        return out

    def local_map(self, kf_id: int) -> Tuple[List[int], List[int], Dict[int, Dict[int, int]]]:
        """Optimizer.cc:456-506 for pKF: local_ids (pKF and GetVectorCovisibleKeyFrames()), fixed_ids, and point
        mnId -> {keyframe mnId -> keypoint index} over the local points, as problem_of_local_map takes them."""
        kf_id = int(kf_id)
        local = [kf_id] + [i for i in self.GetVectorCovisibleKeyFrames(kf_id) if i != kf_id]
        g = self.gather_local_map(local)
        order = sorted(local) + g.fixed_ids.tolist()
        obs: Dict[int, Dict[int, int]] = {}
        for i, pid in enumerate(g.point_ids.tolist()):
            b, e = int(g.edge_begin[i]), int(g.edge_begin[i + 1])
            obs[pid] = {order[k]: int(s) for k, s in zip(g.edge_kf[b:e].tolist(), g.edge_slot[b:e].tolist())}
        return local, g.fixed_ids.tolist(), obs

    # ---- readers (KeyFrame.cc:159-210, :419-434) -------------------------------------------------
    def GetConnectedKeyFrames(self, kf_id: int) -> Set[int]:
        return set(self._nodes[int(kf_id)].weights)

    def GetVectorCovisibleKeyFrames(self, kf_id: int) -> List[int]:
        return list(self._nodes[int(kf_id)].ordered)

    def GetBestCovisibilityKeyFrames(self, kf_id: int, n: int) -> List[int]:
        return list(self._nodes[int(kf_id)].ordered[:int(n)])

    def GetCovisiblesByWeight(self, kf_id: int, w: int) -> List[int]:
        """KeyFrame.cc:185-201, its upper_bound included: when no ordered weight is below w the iterator is end()
        and the reference returns an empty vector, not the whole list."""
        node = self._nodes[int(kf_id)]
        n = sum(1 for wi in node.ordered_weights if wi >= w)  # descending: a prefix
        return [] if n == len(node.ordered) else list(node.ordered[:n])

    def GetWeight(self, kf_id: int, other: int) -> int:
        return self._nodes[int(kf_id)].weights.get(int(other), 0)

    def GetParent(self, kf_id: int) -> Optional[int]:
        return self._nodes[int(kf_id)].parent

    def GetChilds(self, kf_id: int) -> Set[int]:
        return set(self._nodes[int(kf_id)].children)

    def GetOrderedWeights(self, kf_id: int) -> List[int]:
        return list(self._nodes[int(kf_id)].ordered_weights)
