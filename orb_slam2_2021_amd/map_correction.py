"""The map corrections that follow an optimiser, on MI355X (include/orbfe_mapcorr.h): new poses applied to a
map's points, and the points' viewing normal and scale-invariance distances refreshed.

Mirrors MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:360-401), LoopClosing::CorrectLoop's pose and point
correction (src/LoopClosing.cc:453-535) and RunGlobalBundleAdjustment's map update (:705-766) of the
reference. `MapCorrector` is the device handle with the three calls; `normals_problem_of_map`,
`loop_problem_of_map` and `gba_update_problem_of_map` perform the gathers over the dict-based map objects
`problem_of_map` takes; `UpdateNormalAndDepth`, `CorrectLoopPoses` and `ApplyGlobalBundleAdjustment` write
the results back in place. The mnCorrectedByKF / mnBAGlobalForKF bookkeeping, UpdateConnections, the fusion
and InformNewBigChange stay with the caller.
"""
from __future__ import annotations

from ctypes import byref, c_void_p
from types import SimpleNamespace
from typing import Dict, Iterable, List, Mapping, Optional, Sequence

import numpy as np

from . import _lib as L
from .frames import camera_center

MAX_KF, MAX_POINTS, MAX_EDGES, MAX_LEVELS = L.MAPCORR_MAX_KF, L.MAPCORR_MAX_POINTS, L.MAPCORR_MAX_EDGES, L.MAPCORR_MAX_LEVELS


def _good_keyframes(keyframes):
    kf_ids = sorted(int(i) for i, kf in keyframes.items() if not getattr(kf, "bad", False))
    return kf_ids, {kid: i for i, kid in enumerate(kf_ids)}


def _tcw_of(keyframes, kf_ids):
    tcw = np.zeros((len(kf_ids), 12), np.float32)
    for i, kid in enumerate(kf_ids):
        tcw[i] = np.asarray(keyframes[kid].tcw, np.float32).reshape(-1)[:12]
    return tcw


def _points_of_map(keyframes, index, points, observations, point_ids, point_refs):
    """The points' side of calls 1 and 2. The observers ascend in mnId (the reference's std::map follows
    KeyFrame*); an observation by a keyframe that is not listed is skipped. Without point_refs a point's
    reference keyframe is its first observer. ref_level is the octave of the reference keyframe's keypoint,
    keypoint 0's when the reference keyframe is not an observer (what operator[] yields)."""
    n = len(point_ids)
    xw, bad = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    ref_kf, ref_level = np.zeros(n, np.int32), np.zeros(n, np.int32)
    obs_begin, obs_kf = [0], []
    for i, pid in enumerate(point_ids):
        x = points.get(pid)
        obs = observations.get(pid, {})
        seen = [int(k) for k in sorted(obs) if int(k) in index]
        if x is None:
            bad[i] = 1
        else:
            xw[i] = np.asarray(x, np.float32).reshape(3)
            obs_kf += [index[k] for k in seen]
            ref = point_refs.get(pid) if point_refs is not None else None
            if ref is None and seen:
                ref = seen[0]
            if ref is not None and int(ref) in index:
                kf = keyframes[int(ref)]
                ref_kf[i] = index[int(ref)]
                ref_level[i] = int(kf.keys_un["octave"][int(obs[ref]) if ref in obs else 0])
            elif seen:
                raise ValueError(f"the reference keyframe of point {pid} is not among the good keyframes")
        obs_begin.append(len(obs_kf))
    scale = (np.asarray(keyframes[next(iter(index))].scale_factors, np.float32) if index else np.ones(1, np.float32))
    return SimpleNamespace(n_points=n, n_obs=len(obs_kf), n_levels=len(scale), scale_factors=scale, xw=xw, bad=bad,
                           obs_begin=np.array(obs_begin, np.int32), obs_kf=np.array(obs_kf, np.int32), ref_kf=ref_kf,
                           ref_level=ref_level)


def normals_problem_of_map(keyframes: Mapping[int, object], points: Mapping[int, Optional[np.ndarray]],
                           observations: Mapping[int, Mapping[int, int]], point_ids: Optional[Iterable[int]] = None,
                           point_refs: Optional[Mapping[int, int]] = None) -> SimpleNamespace:
    """keyframes: mnId -> KeyFrame (tcw, keys_un, scale_factors; an optional `bad`); points: mnId ->
    GetWorldPos(), None for a bad point; observations: point mnId -> {keyframe mnId -> keypoint index};
    point_ids: the points to update (all by default, ascending); point_refs: point mnId -> mnId of mpRefKF.
    The keyframes share one mvScaleFactors table. The problem carries kf_ids and point_ids."""
    kf_ids, index = _good_keyframes(keyframes)
    point_ids = sorted(int(i) for i in points) if point_ids is None else [int(i) for i in point_ids]
    tcw = _tcw_of(keyframes, kf_ids)
    ow = np.array([camera_center(t) for t in tcw], np.float32).reshape(-1, 3)
    p = _points_of_map(keyframes, index, points, observations, point_ids, point_refs)
    p.n_kf, p.ow, p.kf_ids, p.point_ids = len(kf_ids), ow, kf_ids, point_ids
    return p


def loop_problem_of_map(keyframes: Mapping[int, object], points: Mapping[int, Optional[np.ndarray]],
                        observations: Mapping[int, Mapping[int, int]], connected_ids: Iterable[int], cur_kf: int,
                        scw: Sequence[float], rows: Mapping[int, Sequence[Optional[int]]],
                        point_refs: Optional[Mapping[int, int]] = None,
                        tie_keys: Optional[Mapping[int, int]] = None) -> SimpleNamespace:
    """connected_ids: mvpCurrentConnectedKFs, the current keyframe included; cur_kf: mpCurrentKF's mnId; scw:
    mg2oScw (q x y z w, t, s); rows: keyframe mnId -> GetMapPointMatches() as point mnIds (None or -1: no
    point); tie_keys: mnId -> the key that stands for KeyFrame* (the mnId by default): CorrectedSim3 is
    iterated in its order. Every point of `points` is listed, ascending. The problem carries kf_ids,
    point_ids and connected_ids (in list order)."""
    kf_ids, index = _good_keyframes(keyframes)
    key = (lambda k: (tie_keys[k], k)) if tie_keys is not None else (lambda k: k)
    connected = sorted((int(k) for k in connected_ids), key=key)
    point_ids = sorted(int(i) for i in points)
    pindex = {pid: i for i, pid in enumerate(point_ids)}
    row_begin, row_point = [0], []
    for kid in connected:
        row_point += [pindex[int(q)] if q is not None and int(q) >= 0 else -1 for q in rows.get(kid, ())]
        row_begin.append(len(row_point))
    p = _points_of_map(keyframes, index, points, observations, point_ids, point_refs)
    p.n_kf, p.tcw, p.n_connected = len(kf_ids), _tcw_of(keyframes, kf_ids), len(connected)
    p.connected_kf = np.array([index[k] for k in connected], np.int32)
    p.cur, p.scw = connected.index(int(cur_kf)), np.asarray(scw, np.float64).reshape(8).copy()
    p.n_slots, p.row_begin, p.row_point = len(row_point), np.array(row_begin, np.int32), np.array(row_point, np.int32)
    p.kf_ids, p.point_ids, p.connected_ids = kf_ids, point_ids, connected
    return p


def gba_update_problem_of_map(keyframes: Mapping[int, object], tcw_gba: Mapping[int, np.ndarray],
                              points: Mapping[int, Optional[np.ndarray]], pos_gba: Mapping[int, np.ndarray],
                              parents: Mapping[int, Optional[int]], point_refs: Mapping[int, int]) -> SimpleNamespace:
    """tcw_gba: mnId -> mTcwGBA of the keyframes with mnBAGlobalForKF == nLoopKF; pos_gba: point mnId ->
    mPosGBA of the points with mnBAGlobalForKF == nLoopKF; parents: mnId -> GetParent(), None for a keyframe of
    mvpKeyFrameOrigins; point_refs: point mnId -> GetReferenceKeyFrame(), -1 in the problem when it is not a
    listed keyframe. The problem carries kf_ids and point_ids."""
    kf_ids, index = _good_keyframes(keyframes)
    nk = len(kf_ids)
    gba, optimised, parent = np.zeros((nk, 12), np.float32), np.zeros(nk, np.uint8), np.full(nk, -1, np.int32)
    for i, kid in enumerate(kf_ids):
        if kid in tcw_gba:
            gba[i], optimised[i] = np.asarray(tcw_gba[kid], np.float32).reshape(-1)[:12], 1
        q = parents.get(kid)
        parent[i] = index[int(q)] if q is not None else -1
    point_ids = sorted(int(i) for i in points)
    n = len(point_ids)
    xw, xg = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    bad, popt, ref = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.full(n, -1, np.int32)
    for i, pid in enumerate(point_ids):
        if points[pid] is None:
            bad[i] = 1
            continue
        xw[i] = np.asarray(points[pid], np.float32).reshape(3)
        if pid in pos_gba:
            xg[i], popt[i] = np.asarray(pos_gba[pid], np.float32).reshape(3), 1
        ref[i] = index.get(int(point_refs[pid]), -1) if point_refs.get(pid) is not None else -1
    return SimpleNamespace(n_kf=nk, tcw=_tcw_of(keyframes, kf_ids), tcw_gba=gba, optimised=optimised, parent=parent,
                           n_points=n, xw=xw, bad=bad, pt_optimised=popt, xw_gba=xg, ref_kf=ref, kf_ids=kf_ids,
                           point_ids=point_ids)


def _fill(S, fields, keep):
    for name, (src, dtype, count) in fields.items():
        arr = np.ascontiguousarray(src, dtype).reshape(-1)
        if len(arr) != count:
            raise ValueError(f"{name} must hold {count} values")
        keep[name] = arr if count else np.zeros(1, dtype)
        setattr(S, name, L.ptr(keep[name]))


def _c_points(P, p, keep):
    npt, no = int(p.n_points), int(p.n_obs)
    P.n_points, P.n_obs, P.n_levels = npt, no, int(p.n_levels)
    _fill(P, dict(scale_factors=(p.scale_factors, np.float32, max(int(p.n_levels), 0)), xw=(p.xw, np.float32, 3 * npt),
                  bad=(p.bad, np.uint8, npt), obs_begin=(p.obs_begin, np.int32, npt + 1), obs_kf=(p.obs_kf, np.int32, no),
                  ref_kf=(p.ref_kf, np.int32, npt), ref_level=(p.ref_level, np.int32, npt)), keep)


def _c_normals(R, p, npt):
    """The three in/out arrays start as the problem's normal / max_dist / min_dist where it carries them."""
    normal = np.array(getattr(p, "normal", np.zeros((npt, 3))), np.float32).reshape(-1)
    max_dist = np.array(getattr(p, "max_dist", np.zeros(npt)), np.float32).reshape(-1)
    min_dist = np.array(getattr(p, "min_dist", np.zeros(npt)), np.float32).reshape(-1)
    if (len(normal), len(max_dist), len(min_dist)) != (3 * npt, npt, npt):
        raise ValueError("normal, max_dist and min_dist must hold one entry per point")
    out = dict(normal=np.append(normal, np.float32(0)), max_dist=np.append(max_dist, np.float32(0)),
               min_dist=np.append(min_dist, np.float32(0)), updated=np.zeros(npt + 1, np.uint8))
    for name, arr in out.items():
        setattr(R, name, L.ptr(arr))
    return out


def _normals_result(out, npt):
    return dict(normal=out["normal"][:3 * npt].reshape(npt, 3), max_dist=out["max_dist"][:npt],
                min_dist=out["min_dist"][:npt], updated=out["updated"][:npt])


class MapCorrector:
    """The device handle: staging and workspace for maps up to the given bounds; reused from call to call.
    device < 0 gives a host-only handle (argument checks only). Not thread-safe."""

    def __init__(self, max_kf: int = 1024, max_points: int = 131072, max_edges: int = 1048576, device: int = 0):
        self._lib = L.lib()
        h = c_void_p()
        L.check(self._lib.orbfe_mapcorr_create(int(device), int(max_kf), int(max_points), int(max_edges), byref(h)),
                "orbfe_mapcorr_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_mapcorr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update_normal_depth(self, p) -> SimpleNamespace:
        """orbfe_mapcorr_update_normal_depth -> normal (n_points, 3), max_dist, min_dist (float32) and updated
        (uint8). Where updated is 0 the three hold what p.normal / p.max_dist / p.min_dist held (zeros without)."""
        nk, npt = int(p.n_kf), int(p.n_points)
        P, R, keep = L.mapcorr_normals_problem(), L.mapcorr_normals(), {}
        P.n_kf = nk
        _fill(P, dict(ow=(p.ow, np.float32, 3 * nk)), keep)
        _c_points(P.points, p, keep)
        out = _c_normals(R, p, npt)
        L.check(self._lib.orbfe_mapcorr_update_normal_depth(self._h, byref(P), byref(R)), "orbfe_mapcorr_update_normal_depth")
        return SimpleNamespace(**_normals_result(out, npt))

    def correct_loop(self, p) -> SimpleNamespace:
        """orbfe_mapcorr_correct_loop -> noncorrected_sim3, corrected_sim3 (n_connected, 8) float64, tcw_out
        (n_connected, 12), xw_out (n_points, 3), corrected_by (n_points) int32 and call 1's four outputs."""
        nk, nc, ns, npt = int(p.n_kf), int(p.n_connected), int(p.n_slots), int(p.n_points)
        P, R, keep = L.mapcorr_loop_problem(), L.mapcorr_loop_result(), {}
        P.n_kf, P.n_connected, P.cur, P.n_slots = nk, nc, int(p.cur), ns
        _fill(P, dict(tcw=(p.tcw, np.float32, 12 * nk), connected_kf=(p.connected_kf, np.int32, max(nc, 0)),
                      scw=(p.scw, np.float64, 8), row_begin=(p.row_begin, np.int32, max(nc, 0) + 1),
                      row_point=(p.row_point, np.int32, ns)), keep)
        _c_points(P.points, p, keep)
        out = _c_normals(R.normals, p, npt)
        m = max(nc, 1)
        nonc, corr, tcw = np.zeros(8 * m, np.float64), np.zeros(8 * m, np.float64), np.zeros(12 * m, np.float32)
        xw, by = np.zeros(3 * npt + 1, np.float32), np.zeros(npt + 1, np.int32)
        R.noncorrected_sim3, R.corrected_sim3, R.tcw_out, R.xw_out, R.corrected_by = (L.ptr(nonc), L.ptr(corr), L.ptr(tcw),
                                                                                      L.ptr(xw), L.ptr(by))
        L.check(self._lib.orbfe_mapcorr_correct_loop(self._h, byref(P), byref(R)), "orbfe_mapcorr_correct_loop")
        nc = max(nc, 0)
        return SimpleNamespace(noncorrected_sim3=nonc[:8 * nc].reshape(nc, 8), corrected_sim3=corr[:8 * nc].reshape(nc, 8),
                               tcw_out=tcw[:12 * nc].reshape(nc, 12), xw_out=xw[:3 * npt].reshape(npt, 3),
                               corrected_by=by[:npt], **_normals_result(out, npt))

    def apply_gba(self, p) -> SimpleNamespace:
        """orbfe_mapcorr_apply_gba -> tcw_out (n_kf, 12), propagated (n_kf) uint8, xw_out (n_points, 3),
        pt_changed (n_points) uint8 and levels, the dependent steps the propagation took."""
        nk, npt = int(p.n_kf), int(p.n_points)
        P, R, keep = L.mapcorr_gba_problem(), L.mapcorr_gba_result(), {}
        P.n_kf, P.n_points = nk, npt
        _fill(P, dict(tcw=(p.tcw, np.float32, 12 * nk), tcw_gba=(p.tcw_gba, np.float32, 12 * nk),
                      optimised=(p.optimised, np.uint8, nk), parent=(p.parent, np.int32, nk), xw=(p.xw, np.float32, 3 * npt),
                      bad=(p.bad, np.uint8, npt), pt_optimised=(p.pt_optimised, np.uint8, npt),
                      xw_gba=(p.xw_gba, np.float32, 3 * npt), ref_kf=(p.ref_kf, np.int32, npt)), keep)
        tcw, prop = np.zeros(12 * nk + 1, np.float32), np.zeros(nk + 1, np.uint8)
        xw, changed = np.zeros(3 * npt + 1, np.float32), np.zeros(npt + 1, np.uint8)
        R.tcw_out, R.propagated, R.xw_out, R.pt_changed = L.ptr(tcw), L.ptr(prop), L.ptr(xw), L.ptr(changed)
        L.check(self._lib.orbfe_mapcorr_apply_gba(self._h, byref(P), byref(R)), "orbfe_mapcorr_apply_gba")
        return SimpleNamespace(tcw_out=tcw[:12 * nk].reshape(nk, 12), propagated=prop[:nk], xw_out=xw[:3 * npt].reshape(npt, 3),
                               pt_changed=changed[:npt], levels=int(R.levels))


def _with_corrector(corrector, device, sizes, fn):
    own = corrector is None
    if own:
        corrector = MapCorrector(*(max(int(s), 1) for s in sizes), device)
    try:
        return fn(corrector)
    finally:
        if own:
            corrector.close()


def _write_geometry(geometry, point_ids, r):
    done = []
    for i, pid in enumerate(point_ids):
        if r.updated[i]:
            geometry[pid] = SimpleNamespace(normal=r.normal[i].copy(), max_dist=np.float32(r.max_dist[i]),
                                            min_dist=np.float32(r.min_dist[i]))
            done.append(pid)
    return done


def UpdateNormalAndDepth(keyframes: Mapping[int, object], points: Mapping[int, Optional[np.ndarray]],
                         observations: Mapping[int, Mapping[int, int]], geometry: Dict[int, object],
                         point_ids: Optional[Iterable[int]] = None, point_refs: Optional[Mapping[int, int]] = None,
                         corrector: Optional[MapCorrector] = None, device: int = 0) -> List[int]:
    """void MapPoint::UpdateNormalAndDepth() for the listed points: sets geometry[mnId] (normal, max_dist,
    min_dist: mNormalVector, mfMaxDistance, mfMinDistance) of every point that is not bad and has an
    observation, and returns their mnIds. Without `corrector` a handle sized for the call is created."""
    p = normals_problem_of_map(keyframes, points, observations, point_ids, point_refs)
    r = _with_corrector(corrector, device, (p.n_kf, p.n_points, p.n_obs), lambda c: c.update_normal_depth(p))
    return _write_geometry(geometry, p.point_ids, r)


def CorrectLoopPoses(keyframes: Dict[int, object], points: Dict[int, Optional[np.ndarray]],
                     observations: Mapping[int, Mapping[int, int]], connected_ids: Iterable[int], cur_kf: int,
                     scw: Sequence[float], rows: Mapping[int, Sequence[Optional[int]]], geometry: Dict[int, object],
                     point_refs: Optional[Mapping[int, int]] = None, tie_keys: Optional[Mapping[int, int]] = None,
                     corrector: Optional[MapCorrector] = None, device: int = 0) -> SimpleNamespace:
    """LoopClosing::CorrectLoop, :453-535: sets tcw of every connected keyframe (SetPose), the position of
    every corrected point (SetWorldPos) and its geometry in place. Returns non_corrected and corrected (mnId ->
    q x y z w, t, s: NonCorrectedSim3 and CorrectedSim3, ready for problem_of_essential_graph) and corrected_by
    (point mnId -> the mnId of the correcting keyframe: mnCorrectedReference)."""
    p = loop_problem_of_map(keyframes, points, observations, connected_ids, cur_kf, scw, rows, point_refs, tie_keys)
    r = _with_corrector(corrector, device, (p.n_kf, p.n_points, max(p.n_obs, p.n_slots)), lambda c: c.correct_loop(p))
    for i, kid in enumerate(p.connected_ids):
        keyframes[kid].tcw = r.tcw_out[i].reshape(3, 4).copy()
    by = {}
    for i, pid in enumerate(p.point_ids):
        if r.corrected_by[i] >= 0:
            points[pid] = r.xw_out[i].copy()
            by[pid] = p.connected_ids[int(r.corrected_by[i])]
    _write_geometry(geometry, p.point_ids, r)
    return SimpleNamespace(non_corrected={k: r.noncorrected_sim3[i].copy() for i, k in enumerate(p.connected_ids)},
                           corrected={k: r.corrected_sim3[i].copy() for i, k in enumerate(p.connected_ids)}, corrected_by=by)


def ApplyGlobalBundleAdjustment(keyframes: Dict[int, object], tcw_gba: Mapping[int, np.ndarray],
                                points: Dict[int, Optional[np.ndarray]], pos_gba: Mapping[int, np.ndarray],
                                parents: Mapping[int, Optional[int]], point_refs: Mapping[int, int],
                                corrector: Optional[MapCorrector] = None, device: int = 0) -> SimpleNamespace:
    """LoopClosing::RunGlobalBundleAdjustment, :705-766: sets tcw of every keyframe (SetPose) and the position
    of every changed point (SetWorldPos) in place. Returns tcw_bef (mnId -> mTcwBefGBA), propagated (the mnIds
    whose mTcwGBA came from their parent) and changed (the mnIds of the points that moved)."""
    p = gba_update_problem_of_map(keyframes, tcw_gba, points, pos_gba, parents, point_refs)
    r = _with_corrector(corrector, device, (p.n_kf, p.n_points, 1), lambda c: c.apply_gba(p))
    bef = {}
    for i, kid in enumerate(p.kf_ids):
        bef[kid] = p.tcw[i].reshape(3, 4).copy()
        keyframes[kid].tcw = r.tcw_out[i].reshape(3, 4).copy()
    changed = []
    for i, pid in enumerate(p.point_ids):
        if r.pt_changed[i]:
            points[pid] = r.xw_out[i].copy()
            changed.append(pid)
    return SimpleNamespace(tcw_bef=bef, propagated=[k for i, k in enumerate(p.kf_ids) if r.propagated[i]], changed=changed)
