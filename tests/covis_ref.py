"""The reference's covisibility code restated on the CPU with its own containers (test infrastructure):
KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles / EraseConnection and the readers
(src/KeyFrame.cc:122-210, :304-395, :570-584), the vote of Tracking::UpdateLocalKeyFrames
(src/Tracking.cc:1257-1303), the gather of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:456-506) and the
LoopConnections loop of LoopClosing::CorrectLoop (src/LoopClosing.cc:565-587).

A std::map<KeyFrame*, T> is a dict iterated in sorted tie-key order (the tie key stands for the pointer); a
vector<pair<int, KeyFrame*>> is a list of (weight, tie key) tuples, sorted and then reversed by push_front.
MapPoint::mObservations is derived from the keyframes' rows by the rules of include/orbfe_covis.h: the observers
are the live keyframes whose row holds the point, ascending in mnId, each with its lowest slot.
"""
from types import SimpleNamespace


class RefKeyFrame:
    def __init__(self, mn_id, tie_key, points):
        self.mnId = mn_id
        self.key = tie_key                 # the KeyFrame* value
        self.mvpMapPoints = list(points)   # point mnId or -1
        self.mConnectedKeyFrameWeights = {}     # tie key -> weight
        self.mvpOrderedConnectedKeyFrames = []  # tie keys
        self.mvOrderedWeights = []
        self.mpParent = None               # tie key
        self.mspChildrens = set()          # tie keys
        self.mbFirstConnection = True


class RefCovisibility:
    def __init__(self):
        self.kfs = {}       # mnId -> RefKeyFrame
        self.by_key = {}    # tie key -> RefKeyFrame (dereferencing the pointer)
        self.id_of_key = {}  # tie key -> mnId, erased keyframes included (a dangling pointer still names one)
        self.bad = set()    # point ids with isBad()
        self._obs = None    # point id -> {mnId -> slot}, ascending mnId
        self.kfdb_calls = []  # (mnId, GetBestCovisibilityKeyFrames(10)) in call order

    # ---- the table -----------------------------------------------------------------------------
    def set_keyframe(self, mn_id, points, tie_key=None):
        old = self.kfs.get(mn_id)
        key = tie_key if tie_key is not None else (old.key if old else mn_id)
        assert key not in self.by_key or self.by_key[key] is old, "duplicate tie key"
        if old is None:
            kf = RefKeyFrame(mn_id, key, points)
            self.kfs[mn_id] = kf
            self.by_key[key] = kf
            self.id_of_key[key] = mn_id
        else:
            assert key == old.key, "the restatement's graph state is keyed by the pointer"
            old.mvpMapPoints = list(points)
        self._obs = None

    def set_slots(self, mn_id, slots, points):
        for s, p in zip(slots, points):
            self.kfs[mn_id].mvpMapPoints[s] = p
        self._obs = None

    def set_points_bad(self, points, bad=True):
        for p in points:
            (self.bad.add if bad else self.bad.discard)(p)

    def erase(self, mn_id):
        """SetBadFlag's EraseConnection loop (:482-484), EraseObservation (:486-488) and EraseChild (:555); not
        the re-parenting."""
        kf = self.kfs.pop(mn_id)
        del self.by_key[kf.key]
        self._obs = None
        before = {}
        for key in sorted(kf.mConnectedKeyFrameWeights):
            other = self.by_key.get(key)
            if other is not None:
                self._snapshot(before, other)
                self._erase_connection(other, kf.key)
        if kf.mpParent in self.by_key:
            self.by_key[kf.mpParent].mspChildrens.discard(kf.key)
        self._mirror(before)

    def __len__(self):
        return len(self.kfs)

    def observations(self):
        if self._obs is None:
            obs = {}
            for mn_id in sorted(self.kfs):
                for slot, p in enumerate(self.kfs[mn_id].mvpMapPoints):
                    if p >= 0:
                        obs.setdefault(p, {}).setdefault(mn_id, slot)
            self._obs = obs
        return self._obs

    def _observers_by_key(self, p):
        """map<KeyFrame*, size_t>: iteration in pointer order"""
        o = self.observations().get(p, {})
        return sorted((self.kfs[i].key, slot) for i, slot in o.items())

    # ---- KeyFrame.cc ---------------------------------------------------------------------------
    def _update_best_covisibles(self, kf):
        v_pairs = [(w, key) for key, w in sorted(kf.mConnectedKeyFrameWeights.items())]
        v_pairs.sort()
        l_kfs, l_ws = [], []
        for w, key in v_pairs:
            l_kfs.insert(0, key)
            l_ws.insert(0, w)
        kf.mvpOrderedConnectedKeyFrames = l_kfs
        kf.mvOrderedWeights = l_ws

    def _add_connection(self, kf, key, weight):
        if key not in kf.mConnectedKeyFrameWeights:
            kf.mConnectedKeyFrameWeights[key] = weight
        elif kf.mConnectedKeyFrameWeights[key] != weight:
            kf.mConnectedKeyFrameWeights[key] = weight
        else:
            return
        self._update_best_covisibles(kf)

    def _erase_connection(self, kf, key):
        if key in kf.mConnectedKeyFrameWeights:
            del kf.mConnectedKeyFrameWeights[key]
            self._update_best_covisibles(kf)

    def _snapshot(self, before, kf):
        before.setdefault(kf.mnId, list(kf.mvpOrderedConnectedKeyFrames))

    def _mirror(self, before):
        for mn_id, old in before.items():
            kf = self.kfs.get(mn_id)
            if kf is not None and kf.mvpOrderedConnectedKeyFrames != old:
                self.kfdb_calls.append((mn_id, self.GetBestCovisibilityKeyFrames(mn_id, 10)))

    def count_connections(self, mn_id, th=15):
        """:304-378 without the side effects, in the shape of CovisibilityGraph.count_connections."""
        kf = self.kfs[mn_id]
        counter = {}
        for p in kf.mvpMapPoints:
            if p < 0:
                continue
            if p in self.bad:
                continue
            for key, _ in self._observers_by_key(p):
                if self.by_key[key].mnId == kf.mnId:
                    continue
                counter[key] = counter.get(key, 0) + 1
        if not counter:
            return SimpleNamespace(counter_ids=[], counter_weights=[], ordered_ids=[], ordered_weights=[], nmax=0,
                                   kf_max=-1, unchanged=True, counter=counter, pairs=[])
        nmax, kf_max = 0, None
        v_pairs = []
        for key in sorted(counter):
            if counter[key] > nmax:
                nmax, kf_max = counter[key], key
            if counter[key] >= th:
                v_pairs.append((counter[key], key))
        if not v_pairs:
            v_pairs.append((nmax, kf_max))
        v_pairs.sort()
        l_kfs, l_ws = [], []
        for w, key in v_pairs:
            l_kfs.insert(0, key)
            l_ws.insert(0, w)
        ids = lambda keys: [self.by_key[k].mnId for k in keys]
        return SimpleNamespace(counter_ids=ids(sorted(counter)), counter_weights=[counter[k] for k in sorted(counter)],
                               ordered_ids=ids(l_kfs), ordered_weights=l_ws, nmax=nmax, kf_max=self.by_key[kf_max].mnId,
                               unchanged=False, counter=counter, pairs=list(zip(l_ws, l_kfs)))

    def _update_connections(self, mn_id, th, before):
        kf = self.kfs[mn_id]
        c = self.count_connections(mn_id, th)
        if c.unchanged:
            return
        for w, key in sorted(c.pairs, key=lambda t: t[1]):  # :350-362 iterates KFcounter: ascending pointer
            other = self.by_key[key]
            self._snapshot(before, other)
            self._add_connection(other, kf.key, w)
        self._snapshot(before, kf)
        kf.mConnectedKeyFrameWeights = dict(c.counter)
        kf.mvpOrderedConnectedKeyFrames = [k for _, k in c.pairs]
        kf.mvOrderedWeights = [w for w, _ in c.pairs]
        if kf.mbFirstConnection and kf.mnId != 0:
            kf.mpParent = kf.mvpOrderedConnectedKeyFrames[0]
            self.by_key[kf.mpParent].mspChildrens.add(kf.key)
            kf.mbFirstConnection = False

    def update_connections(self, mn_ids, th=15):
        before = {}
        for mn_id in ([mn_ids] if isinstance(mn_ids, int) else mn_ids):
            self._update_connections(mn_id, th, before)
        self._mirror(before)

    def loop_connections(self, connected, th=15):
        """LoopClosing.cc:565-587"""
        before, out = {}, {}
        for mn_id in connected:
            previous = self.GetVectorCovisibleKeyFrames(mn_id)
            self._update_connections(mn_id, th, before)
            s = self.GetConnectedKeyFrames(mn_id)
            for p in previous:
                s.discard(p)
            for c in connected:
                s.discard(c)
            out[mn_id] = s
        self._mirror(before)
        return out

    # ---- readers, in mnIds ---------------------------------------------------------------------
    def _ids(self, keys):
        return [self.id_of_key[k] for k in keys]

    def GetConnectedKeyFrames(self, mn_id):
        return set(self._ids(self.kfs[mn_id].mConnectedKeyFrameWeights))

    def GetVectorCovisibleKeyFrames(self, mn_id):
        return self._ids(self.kfs[mn_id].mvpOrderedConnectedKeyFrames)

    def GetOrderedWeights(self, mn_id):
        return list(self.kfs[mn_id].mvOrderedWeights)

    def GetBestCovisibilityKeyFrames(self, mn_id, n):
        v = self.kfs[mn_id].mvpOrderedConnectedKeyFrames
        return self._ids(v if len(v) < n else v[:n])

    def GetCovisiblesByWeight(self, mn_id, w):
        kf = self.kfs[mn_id]
        if not kf.mvpOrderedConnectedKeyFrames:
            return []
        it = len(kf.mvOrderedWeights)  # upper_bound(begin, end, w, a > b): the first weight with w > weight
        for i, wi in enumerate(kf.mvOrderedWeights):
            if w > wi:
                it = i
                break
        if it == len(kf.mvOrderedWeights):
            return []
        return self._ids(kf.mvpOrderedConnectedKeyFrames[:it])

    def GetWeight(self, mn_id, other):
        key = self.kfs[other].key if other in self.kfs else other
        return self.kfs[mn_id].mConnectedKeyFrameWeights.get(key, 0)

    def GetParent(self, mn_id):
        p = self.kfs[mn_id].mpParent
        return None if p is None else self._ids([p])[0]

    def GetChilds(self, mn_id):
        return set(self._ids(self.kfs[mn_id].mspChildrens))

    def state(self, mn_id):
        """Everything CovisibilityGraph keeps for one keyframe, for whole-state comparisons."""
        kf = self.kfs[mn_id]
        return (dict(zip(self._ids(kf.mConnectedKeyFrameWeights), kf.mConnectedKeyFrameWeights.values())),
                self.GetVectorCovisibleKeyFrames(mn_id), self.GetOrderedWeights(mn_id), self.GetParent(mn_id),
                self.GetChilds(mn_id), kf.mbFirstConnection)

    # ---- Tracking.cc:1257-1303 -----------------------------------------------------------------
    def vote(self, points):
        counter = {}
        for p in points:
            if p >= 0:
                if p not in self.bad:
                    for key, _ in self._observers_by_key(p):
                        counter[key] = counter.get(key, 0) + 1
        mx, kf_max, local = 0, None, []
        for key in sorted(counter):
            if counter[key] > mx:
                mx, kf_max = counter[key], key
            local.append(key)
        return SimpleNamespace(kf_ids=self._ids(local), counts=[counter[k] for k in local], max=mx,
                               kf_max=-1 if kf_max is None else self.by_key[kf_max].mnId)

    # ---- Optimizer.cc:456-506 ------------------------------------------------------------------
    def gather_local_map(self, local_ids):
        """lLocalMapPoints, lFixedCameras and the observations, then put in the order orbfe_lba_problem_t wants:
        points ascending, keyframes local ascending then fixed ascending, a point's edges ascending in mnId."""
        local_ids = list(local_ids)
        l_points, marked = [], set()
        for mn_id in local_ids:
            for p in self.kfs[mn_id].mvpMapPoints:
                if p >= 0 and p not in self.bad and p not in marked:
                    l_points.append(p)
                    marked.add(p)
        l_fixed, fixed_mark = [], set()
        for p in l_points:
            for key, _ in self._observers_by_key(p):
                i = self.by_key[key].mnId
                if i not in local_ids and i not in fixed_mark:
                    fixed_mark.add(i)
                    l_fixed.append(i)
        order = sorted(local_ids) + sorted(l_fixed)
        index = {i: k for k, i in enumerate(order)}
        edge_begin, edge_kf, edge_slot = [0], [], []
        for p in sorted(l_points):
            for i, slot in sorted(self.observations()[p].items()):
                edge_kf.append(index[i])
                edge_slot.append(slot)
            edge_begin.append(len(edge_kf))
        return SimpleNamespace(point_ids=sorted(l_points), fixed_ids=sorted(l_fixed), edge_begin=edge_begin,
                               edge_kf=edge_kf, edge_slot=edge_slot)

    def local_map(self, mn_id):
        local = [mn_id] + [i for i in self.GetVectorCovisibleKeyFrames(mn_id) if i != mn_id]
        g = self.gather_local_map(local)
        return local, g.fixed_ids, {p: dict(self.observations()[p]) for p in g.point_ids}
