"""LocalMapping::KeyFrameCulling (src/LocalMapping.cc:640-706), LocalMapping::MapPointCulling (:174-209) and
KeyFrame::SetBadFlag (src/KeyFrame.cc:469-562) restated on the CPU with the reference's own containers (test
infrastructure), on top of covis_ref's graph:

  - a MapPoint has mObservations, a std::map<KeyFrame*, size_t> (a dict iterated in sorted tie-key order), and nObs,
    kept incrementally by AddObservation / EraseObservation (MapPoint.cc:128-167): the weighted count is never
    derived here;
  - MapPoint::SetBadFlag (:181-198) clears mObservations and erases the match at the recorded index of every observer;
  - KeyFrame::SetBadFlag erases the connections, then the observations in slot order, then re-parents the children.

RefCulling keeps covis_ref's rows (point ids) in step with what the objects do, so its UpdateConnections and
local-map gather can be held against the device's table after a culling. The scene generator at the end is shared
by the CPU and GPU tests.
"""
from types import SimpleNamespace

import numpy as np

from covis_ref import RefCovisibility

KEPT, CULLED, NOT_ERASE, SKIPPED = 0, 1, 2, 3


class MapPoint:
    def __init__(self, mn_id):
        self.mnId = mn_id
        self.mObservations = {}   # tie key -> idx
        self.nObs = 0
        self.mbBad = False

    def AddObservation(self, kf, idx):
        if kf.key in self.mObservations:
            return
        self.mObservations[kf.key] = idx
        if kf.mvuRight[idx] >= np.float32(0):
            self.nObs += 2
        else:
            self.nObs += 1


class RefCulling(RefCovisibility):
    def __init__(self):
        super().__init__()
        self.points = {}         # point id -> MapPoint
        self.kfdb_erased = []    # mnIds, in call order
        self.to_be_erased = set()

    # ---- building ----------------------------------------------------------------------------------------
    def point(self, p):
        if p not in self.points:
            self.points[p] = MapPoint(p)
        return self.points[p]

    def add_keyframe(self, mn_id, points, octaves, u_right, depth, th_depth, tie_key=None):
        """A new keyframe with its keypoints' attributes; AddObservation on every slot in slot order."""
        assert mn_id not in self.kfs
        self.set_keyframe(mn_id, [int(p) for p in points], tie_key)
        kf = self.kfs[mn_id]
        kf.octave = [int(o) for o in octaves]
        kf.mvuRight = np.asarray(u_right, np.float32)
        kf.mvDepth = np.asarray(depth, np.float32)
        kf.mThDepth = np.float32(th_depth)
        assert len(kf.octave) == len(kf.mvuRight) == len(kf.mvDepth) == len(kf.mvpMapPoints)
        for idx, p in enumerate(kf.mvpMapPoints):
            if p >= 0:
                mp = self.point(p)
                if p in self.bad:
                    continue  # a bad point has no observations
                mp.AddObservation(kf, idx)

    def set_points_bad(self, points, bad=True):
        """MapPoint::SetBadFlag without the row edits (orbfe_covis_set_points_bad's contract)."""
        assert bad
        super().set_points_bad(points, True)
        for p in points:
            mp = self.point(p)
            mp.mbBad = True
            mp.mObservations = {}

    # ---- MapPoint.cc ---------------------------------------------------------------------------------------
    def _erase_match(self, kf, idx):
        kf.mvpMapPoints[idx] = -1
        self._obs = None

    def _point_set_bad(self, mp):
        obs = dict(mp.mObservations)
        mp.mbBad = True
        mp.mObservations = {}
        self.bad.add(mp.mnId)
        for key in sorted(obs):
            self._erase_match(self.by_key[key], obs[key])

    def _erase_observation(self, mp, kf):
        b_bad = False
        if kf.key in mp.mObservations:
            idx = mp.mObservations[kf.key]
            if kf.mvuRight[idx] >= np.float32(0):
                mp.nObs -= 2
            else:
                mp.nObs -= 1
            del mp.mObservations[kf.key]
            if mp.nObs <= 2:
                b_bad = True
        if b_bad:
            self._point_set_bad(mp)
        return b_bad

    # ---- KeyFrame::SetBadFlag ------------------------------------------------------------------------------
    def set_bad_flag(self, mn_id, not_erase=False, before=None):
        """Returns the points EraseObservation made bad, in slot order (None when nothing was erased)."""
        kf = self.kfs[mn_id]
        if kf.mnId == 0:
            return None
        if not_erase:
            self.to_be_erased.add(mn_id)
            return None
        own = before is None
        before = {} if own else before
        for key in sorted(kf.mConnectedKeyFrameWeights):
            other = self.by_key.get(key)
            if other is not None:
                self._snapshot(before, other)
                self._erase_connection(other, kf.key)
        went_bad = []
        for p in list(kf.mvpMapPoints):
            if p >= 0:
                if self._erase_observation(self.points[p], kf):
                    went_bad.append(p)
        kf.mConnectedKeyFrameWeights = {}
        kf.mvpOrderedConnectedKeyFrames = []
        s_parent_candidates = set()
        if kf.mpParent is not None:
            s_parent_candidates.add(kf.mpParent)
        while kf.mspChildrens:
            b_continue = False
            mx, p_c, p_p = -1, None, None
            for ckey in sorted(kf.mspChildrens):
                child = self.by_key.get(ckey)
                if child is None:  # isBad()
                    continue
                for vkey in child.mvpOrderedConnectedKeyFrames:
                    for pkey in sorted(s_parent_candidates):
                        if self.id_of_key[vkey] == self.id_of_key[pkey]:
                            w = child.mConnectedKeyFrameWeights.get(vkey, 0)
                            if w > mx:
                                p_c, p_p, mx = child, vkey, w
                                b_continue = True
            if b_continue:
                self._change_parent(p_c, p_p)
                s_parent_candidates.add(p_c.key)
                kf.mspChildrens.discard(p_c.key)
            else:
                break
        for ckey in sorted(kf.mspChildrens):
            child = self.by_key.get(ckey)
            if child is not None:
                self._change_parent(child, kf.mpParent)
        if kf.mpParent in self.by_key:
            self.by_key[kf.mpParent].mspChildrens.discard(kf.key)
        del self.kfs[mn_id]   # mpMap->EraseKeyFrame
        del self.by_key[kf.key]
        self._obs = None
        self.kfdb_erased.append(mn_id)
        if own:
            self._mirror(before)
        return went_bad

    def _change_parent(self, child, pkey):
        child.mpParent = pkey
        if pkey in self.by_key:
            self.by_key[pkey].mspChildrens.add(child.key)

    # ---- LocalMapping::KeyFrameCulling ---------------------------------------------------------------------
    def evaluate(self, mn_id, monocular):
        """:654-703 for one candidate: (nMPs, nRedundantObservations, redundant)."""
        kf = self.kfs[mn_id]
        th_obs = 3
        n_red, n_mps = 0, 0
        for i, p in enumerate(kf.mvpMapPoints):
            if p >= 0:
                mp = self.points[p]
                if not mp.mbBad:
                    if not monocular:
                        if kf.mvDepth[i] > kf.mThDepth or kf.mvDepth[i] < np.float32(0):
                            continue
                    n_mps += 1
                    if mp.nObs > th_obs:
                        scale_level = kf.octave[i]
                        n_obs = 0
                        for key in sorted(mp.mObservations):
                            kfi = self.by_key[key]
                            if kfi is kf:
                                continue
                            if kfi.octave[mp.mObservations[key]] <= scale_level + 1:
                                n_obs += 1
                                if n_obs >= th_obs:
                                    break
                        if n_obs >= th_obs:
                            n_red += 1
        return n_mps, n_red, n_red > 0.9 * n_mps

    def keyframe_culling(self, candidates, monocular, not_erase=()):
        """The loop at :648-705 over `candidates` (vpLocalKeyFrames) in order."""
        hold = set(not_erase)
        out = SimpleNamespace(decision=[], n_mps=[], n_redundant=[], bad_points=[])
        before = {}
        for mn_id in candidates:
            if mn_id == 0:
                out.decision.append(SKIPPED)
                out.n_mps.append(0)
                out.n_redundant.append(0)
                out.bad_points.append([])
                continue
            n_mps, n_red, redundant = self.evaluate(mn_id, monocular)
            out.n_mps.append(n_mps)
            out.n_redundant.append(n_red)
            went_bad = []
            if redundant:
                r = self.set_bad_flag(mn_id, mn_id in hold, before)
                out.decision.append(NOT_ERASE if r is None else CULLED)
                went_bad = r or []
            else:
                out.decision.append(KEPT)
            out.bad_points.append(went_bad)
        self._mirror(before)
        return out

    def order_free_decisions(self, candidates, monocular, not_erase=()):
        """Every candidate judged against the map as it is now, nothing applied."""
        hold = set(not_erase)
        out = []
        for mn_id in candidates:
            if mn_id == 0:
                out.append(SKIPPED)
            else:
                red = self.evaluate(mn_id, monocular)[2]
                out.append((NOT_ERASE if mn_id in hold else CULLED) if red else KEPT)
        return out

    # ---- LocalMapping::MapPointCulling ---------------------------------------------------------------------
    def map_point_culling(self, point_ids, found, visible, first_kf_ids, current_kf_id, monocular):
        """:187-208 over the list in order; the action per point (the codes of orbfe_covis_cull_points)."""
        cn_th_obs = 2 if monocular else 3
        actions = []
        for p, f, v, first in zip(point_ids, found, visible, first_kf_ids):
            mp = self.point(int(p))
            act = point_action(mp.mbBad, f, v, current_kf_id, first, mp.nObs, cn_th_obs)
            if act in (2, 3):
                self._point_set_bad(mp)
            actions.append(act)
        return actions


def point_action(is_bad, found, visible, current_kf_id, first_kf_id, n_obs, cn_th_obs):
    """One turn of the loop at LocalMapping.cc:187-208; GetFoundRatio is one float32 divide."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.float32(found) / np.float32(visible)
    if is_bad:
        return 1
    elif ratio < np.float32(0.25):
        return 2
    elif int(current_kf_id) - int(first_kf_id) >= 2 and n_obs <= cn_th_obs:
        return 3
    elif int(current_kf_id) - int(first_kf_id) >= 3:
        return 4
    return 0


# ---- scenes ----------------------------------------------------------------------------------------------------
def keyframe(mn_id, points, octaves=None, stereo=None, far=None, tie_key=None):
    """One keyframe of a scene. stereo / far: bools per slot, turned into mvuRight / mvDepth against mThDepth 40
    (test data: the two bits are set independently of each other)."""
    n = len(points)
    octaves = [0] * n if octaves is None else list(octaves)
    stereo = [False] * n if stereo is None else list(stereo)
    far = [False] * n if far is None else list(far)
    u_right = np.where(np.asarray(stereo, bool), np.float32(12.5), np.float32(-1)).astype(np.float32)
    depth = np.where(np.asarray(far, bool), np.float32(41), np.float32(7)).astype(np.float32)
    if n > 1 and far[n - 1]:
        depth[n - 1] = np.float32(-1)  # the other way to be FAR
    return SimpleNamespace(mn_id=int(mn_id), points=np.asarray(points, np.int32).reshape(-1), octaves=octaves,
                           u_right=u_right.reshape(-1), depth=depth.reshape(-1), th_depth=np.float32(40.0),
                           tie_key=tie_key)


def build_ref(kfs, bad=()):
    ref = RefCulling()
    if len(bad):
        ref.set_points_bad([int(p) for p in bad])
    for k in kfs:
        ref.add_keyframe(k.mn_id, k.points.tolist(), k.octaves, k.u_right, k.depth, k.th_depth, k.tie_key)
    return ref


def random_scene(seed, n_kf=300, slots=64, n_candidates=65):
    """A map of n_kf keyframes x `slots` slots with 1 to 6 observers per background point and mixed
    stereo flags, in which the order of the candidates matters. Planted, all in octave 0 and mono:
      - A and B hold the same 60 points, C and D hold them too: each of A, B is redundant only while the other
        lives (Observations() 4 -> 3);
      - A also holds 3 points that only X (there with stereo keypoints) shares: nObs 3 -> 2 when A goes, so they
        go bad by cascade and leave X's row;
      - X holds those 3 and 27 points that E, F, G hold too: 27 of 30 is not > 27.0, 27 of 27 is > 24.3: X is culled
        only after the cascade.
    The candidates hold A before B and X, among background keyframes; odd seeds are stereo runs (the background's
    FAR slots are skipped). Returns (keyframes, candidates, monocular)."""
    rng = np.random.default_rng(seed)
    ids = (rng.permutation(3 * n_kf)[:n_kf] + 1).tolist()          # never mnId 0
    keys = (rng.permutation(n_kf) + 1000).tolist()
    n_bg = n_kf - 8
    n_points = max(n_bg * slots // 3, 8)
    kfs = []
    for i in range(n_bg):
        row = rng.integers(0, n_points, slots).astype(np.int32)
        row[rng.random(slots) < 0.2] = -1
        if slots > 4:
            row[slots - 1] = row[1]                                 # a point in two slots
        kfs.append(keyframe(ids[i], row, rng.integers(0, 8, slots), rng.random(slots) < 0.4, rng.random(slots) < 0.1,
                            keys[i]))
    base = n_points
    shared = np.arange(base, base + 60, dtype=np.int32)
    casc = np.arange(base + 60, base + 63, dtype=np.int32)
    xs = np.arange(base + 63, base + 90, dtype=np.int32)
    a, b, c, d, x, e, f, g = ids[n_bg:]
    ka, kb, kc, kd, kx, ke, kf_, kg = keys[n_bg:]
    kfs.append(keyframe(a, np.concatenate([shared, casc]), tie_key=ka))
    kfs.append(keyframe(b, shared, tie_key=kb))
    kfs.append(keyframe(c, shared, tie_key=kc))
    kfs.append(keyframe(d, shared, tie_key=kd))
    kfs.append(keyframe(x, np.concatenate([casc, xs]), stereo=[True] * 3 + [False] * 27, tie_key=kx))
    for i, k in ((e, ke), (f, kf_), (g, kg)):
        kfs.append(keyframe(i, xs, tie_key=k))
    order = rng.permutation(len(kfs)).tolist()
    kfs = [kfs[i] for i in order]
    pool = [i for i in ids[:n_bg]]
    rng.shuffle(pool)
    cand = pool[:max(n_candidates - 3, 0)]
    ia = int(rng.integers(0, len(cand) // 3 + 1))  # a first, then b and x somewhere behind it
    cand.insert(ia, a)
    cand.insert(int(rng.integers(ia + 1, len(cand) + 1)), b)
    cand.insert(int(rng.integers(ia + 1, len(cand) + 1)), x)
    return kfs, cand, seed % 2 == 0
