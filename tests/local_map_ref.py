"""The reference's local-map walks restated on the CPU with its own containers and stamps (test infrastructure):
Tracking::UpdateLocalKeyFrames, both halves, and UpdateLocalPoints (src/Tracking.cc:1228-1366), vpTargetKFs and
vpFuseCandidates of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:463-521) and mvpLoopMapPoints of
LoopClosing::ComputeSim3 (src/LoopClosing.cc:371-391), over the graph state of covis_ref.RefCovisibility.

A vector is a list grown by append (push_back); a set<KeyFrame*> is iterated in sorted tie-key order; the
"already taken" tests are the reference's stamp members (mnTrackReferenceForFrame, mnFuseTargetForKF,
mnFuseCandidateForKF, mnLoopPointForKF), which start at 0: the caller passes Frame / KeyFrame stamps >= 1 that it has
not used before (a stamp of 0 finds everything taken, the reference's artefact, which the library does not model).
"""
import numpy as np

from covis_ref import RefCovisibility


class RefMapPoint:
    def __init__(self):
        self.mnTrackReferenceForFrame = 0
        self.mnFuseCandidateForKF = 0
        self.mnLoopPointForKF = 0


class RefLocalMap(RefCovisibility):
    def __init__(self):
        super().__init__()
        self.mps = {}           # point id -> RefMapPoint
        self.kf_track = {}      # tie key -> KeyFrame::mnTrackReferenceForFrame
        self.kf_fuse = {}       # tie key -> KeyFrame::mnFuseTargetForKF

    def mp(self, p):
        return self.mps.setdefault(p, RefMapPoint())

    def _walk(self, kf_ids, member, stamp):
        """for each keyframe, for each slot: skip NULL, skip stamped, push_back and stamp the rest that are not bad.
        The three sites differ in the order of the isBad() and stamp tests, which cannot change the list."""
        out = []
        for mn_id in kf_ids:
            for p in list(self.kfs[mn_id].mvpMapPoints):  # GetMapPointMatches() copies
                if p < 0:
                    continue
                pmp = self.mp(p)
                if getattr(pmp, member) == stamp:
                    continue
                if p not in self.bad:
                    out.append(p)
                    setattr(pmp, member, stamp)
        return out

    # ---- Tracking.cc:1228-1252 -----------------------------------------------------------------
    def update_local_points(self, local_kf_ids, frame_id):
        return self._walk(local_kf_ids, "mnTrackReferenceForFrame", frame_id)

    # ---- Tracking.cc:1254-1366 -----------------------------------------------------------------
    def update_local_keyframes(self, frame_points, frame_id):
        """Returns (mvpLocalKeyFrames as mnIds, pKFmax's mnId), or None at the early return of :1277-1278."""
        counter = {}
        for p in frame_points:
            if p >= 0:
                if p not in self.bad:
                    for key, _ in self._observers_by_key(p):
                        counter[key] = counter.get(key, 0) + 1
        if not counter:
            return None
        mx, kf_max, local = 0, None, []
        for key in sorted(counter):  # map<KeyFrame*, int>
            if counter[key] > mx:
                mx, kf_max = counter[key], key
            local.append(key)
            self.kf_track[key] = frame_id
        it_end = len(local)  # itEndKF, taken before the pushes below
        for i in range(it_end):
            if len(local) > 80:
                break
            kf = self.by_key[local[i]]
            v = kf.mvpOrderedConnectedKeyFrames
            for nkey in (v if len(v) < 10 else v[:10]):
                if nkey in self.by_key:  # !isBad()
                    if self.kf_track.get(nkey, 0) != frame_id:
                        local.append(nkey)
                        self.kf_track[nkey] = frame_id
                        break
            for ckey in sorted(kf.mspChildrens):  # set<KeyFrame*>
                if ckey in self.by_key:
                    if self.kf_track.get(ckey, 0) != frame_id:
                        local.append(ckey)
                        self.kf_track[ckey] = frame_id
                        break
            pkey = kf.mpParent
            if pkey is not None and pkey in self.by_key:
                if self.kf_track.get(pkey, 0) != frame_id:
                    local.append(pkey)
                    self.kf_track[pkey] = frame_id
                    break  # :1355 leaves the outer loop
        return self._ids(local), self.by_key[kf_max].mnId

    def update_local_map(self, frame_points, frame_id):
        r = self.update_local_keyframes(frame_points, frame_id)
        if r is None:
            return None
        return r[0], r[1], self.update_local_points(r[0], frame_id)

    # ---- LocalMapping.cc:463-521 ---------------------------------------------------------------
    def fuse_targets(self, kf_id, monocular):
        cur = self.kfs[kf_id]
        targets = []
        for mn in self.GetBestCovisibilityKeyFrames(kf_id, 20 if monocular else 10):
            kfi = self.kfs.get(mn)
            if kfi is None or self.kf_fuse.get(kfi.key, 0) == cur.mnId:
                continue
            targets.append(mn)
            self.kf_fuse[kfi.key] = cur.mnId
            for mn2 in self.GetBestCovisibilityKeyFrames(mn, 5):
                kf2 = self.kfs.get(mn2)
                if kf2 is None or self.kf_fuse.get(kf2.key, 0) == cur.mnId or mn2 == cur.mnId:
                    continue
                targets.append(mn2)
        return targets

    def fuse_candidates(self, kf_id, monocular):
        targets = self.fuse_targets(kf_id, monocular)
        return targets, self._walk(targets, "mnFuseCandidateForKF", kf_id)

    # ---- LoopClosing.cc:371-391 ----------------------------------------------------------------
    def loop_map_points(self, matched_kf_id, current_kf_id):
        kfs = self.GetVectorCovisibleKeyFrames(matched_kf_id)
        kfs.append(matched_kf_id)
        return self._walk(kfs, "mnLoopPointForKF", current_kf_id)


def distinct_by_unique(rows, bad):
    """The second definition: the named rows concatenated, -1 and bad entries dropped, np.unique with the index of
    each value's first occurrence, ordered by that index."""
    flat = np.concatenate([np.asarray(r, np.int64).reshape(-1) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    keep = flat >= 0
    if len(bad):
        keep &= ~np.isin(flat, np.asarray(sorted(bad), np.int64))
    flat = flat[keep]
    values, index = np.unique(flat, return_index=True)
    return values[np.argsort(index, kind="stable")].astype(np.int32)


# ---- scenes --------------------------------------------------------------------------------------
def random_scene(seed, n_kf=40, slots=24, observers=4, p_none=0.15, p_bad=0.05, tie_shuffle=True):
    """A track: keyframe k sees a window of the points that slides with k, so neighbours share points; some slots
    are empty, some points repeat inside a row, a few are bad. Tie keys are a shuffle of the mnIds, so pointer order
    and mnId order disagree. Returns (rows: {mnId: int32 row}, tie: {mnId: key}, bad: sorted ids, n_points)."""
    rng = np.random.default_rng(seed)
    n_points = max(8, n_kf * slots // observers)
    window = max(4, observers * slots // 2)
    rows, tie = {}, {}
    keys = rng.permutation(n_kf) + 1000 if tie_shuffle else np.arange(n_kf)
    for k in range(n_kf):
        base = k * n_points // n_kf
        row = ((base + rng.integers(0, window, slots)) % n_points).astype(np.int32)
        row[rng.random(slots) < p_none] = -1
        rows[k] = row
        tie[k] = int(keys[k])
    bad = sorted(int(p) for p in np.flatnonzero(rng.random(n_points) < p_bad))
    return rows, tie, bad, n_points


def build_ref(rows, tie, bad, connect_th=None):
    """A RefLocalMap of the scene; connect_th: UpdateConnections of every keyframe in mnId order with that th."""
    ref = RefLocalMap()
    for k in sorted(rows):
        ref.set_keyframe(k, [int(p) for p in rows[k]], tie[k])
    ref.set_points_bad(bad)
    if connect_th is not None:
        for k in sorted(rows):
            ref.update_connections(k, connect_th)
    return ref


def hand_graph(n, tie=None):
    """n keyframes with one private point each (so every one can be voted for) and no graph state: the tests set
    mvpOrderedConnectedKeyFrames, mspChildrens and mpParent by hand. Point id = mnId."""
    ref = RefLocalMap()
    for k in range(n):
        ref.set_keyframe(k, [k], tie[k] if tie else k)
    return ref


def link(ref, mn_id, ordered=(), children=(), parent=None):
    kf = ref.kfs[mn_id]
    kf.mvpOrderedConnectedKeyFrames = [ref.kfs[i].key for i in ordered]
    kf.mvOrderedWeights = list(range(len(ordered), 0, -1))
    kf.mConnectedKeyFrameWeights = dict(zip(kf.mvpOrderedConnectedKeyFrames, kf.mvOrderedWeights))
    kf.mspChildrens = {ref.kfs[i].key for i in children}
    kf.mpParent = None if parent is None else ref.kfs[parent].key
    kf.mbFirstConnection = False


def mirror_graph(ref, graph):
    """The restatement's graph state copied into a CovisibilityGraph whose table already holds the keyframes."""
    for mn_id, kf in ref.kfs.items():
        node = graph._nodes[mn_id]
        node.weights = {ref.id_of_key[k]: w for k, w in kf.mConnectedKeyFrameWeights.items()}
        node.ordered = ref._ids(kf.mvpOrderedConnectedKeyFrames)
        node.ordered_weights = list(kf.mvOrderedWeights)
        node.parent = None if kf.mpParent is None else ref.id_of_key[kf.mpParent]
        node.children = set(ref._ids(kf.mspChildrens))
        node.first_connection = kf.mbFirstConnection
