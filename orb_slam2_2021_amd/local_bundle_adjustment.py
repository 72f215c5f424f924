"""Optimizer::LocalBundleAdjustment on MI355X (include/orbfe_lba.h): the Levenberg-Marquardt of one local
map, points marginalised by a Schur complement over the free keyframes.

Mirrors src/Optimizer.cc:508-781 of the reference. `problem_of_local_map` performs the gather of
:525-656 from KeyFrame objects, map point positions and the observation table; `LocalBundleAdjuster`
is the device handle; `LocalBundleAdjustment(...)` writes the poses and positions back and returns the
(keyframe, point) pairs the reference would erase. UpdateNormalAndDepth stays with the caller.
"""
from __future__ import annotations

from ctypes import byref, c_void_p
from types import SimpleNamespace
from typing import Dict, Iterable, List, Mapping, Optional, Tuple

import numpy as np

from . import _lib as L

MAX_FREE_KF, MAX_KF, MAX_POINTS, MAX_EDGES = L.LBA_MAX_FREE_KF, L.LBA_MAX_KF, L.LBA_MAX_POINTS, L.LBA_MAX_EDGES


def problem_of_local_map(keyframes: Mapping[int, object], points: Mapping[int, np.ndarray],
                         observations: Mapping[int, Mapping[int, int]], local_ids: Iterable[int],
                         fixed_ids: Iterable[int] = (), stop_at_poll: int = -1) -> SimpleNamespace:
    """keyframes: mnId -> KeyFrame (tcw, fx fy cx cy, bf, keys_un, u_right, level_sigma2); points: mnId ->
    GetWorldPos(); observations: point mnId -> {keyframe mnId -> keypoint index} (GetObservations());
    local_ids: lLocalKeyFrames, fixed_ids: lFixedCameras. Keyframes are listed local first, then fixed,
    each ascending in mnId, and points ascending in mnId: g2o's Hessian order. A local keyframe with
    mnId 0 is fixed (:531). An observation by a keyframe in neither list (a bad one, :592) is skipped.
    The problem carries kf_ids, point_ids and edge_pairs ((keyframe mnId, point mnId) per edge)."""
    local = sorted(int(i) for i in local_ids)
    fixed_cams = sorted(int(i) for i in fixed_ids if int(i) not in set(local))
    kf_ids = local + fixed_cams
    index = {kid: i for i, kid in enumerate(kf_ids)}
    nk = len(kf_ids)
    tcw = np.zeros((nk, 12), np.float32)
    k = np.zeros((nk, 4), np.float32)
    bf = np.zeros(nk, np.float32)
    fixed = np.zeros(nk, np.uint8)
    inv_level = []
    for i, kid in enumerate(kf_ids):
        kf = keyframes[kid]
        tcw[i] = np.asarray(kf.tcw, np.float32).reshape(-1)[:12]
        k[i] = [kf.fx, kf.fy, kf.cx, kf.cy]
        bf[i] = kf.bf
        fixed[i] = 1 if (i >= len(local) or kid == 0) else 0
        inv_level.append((np.float32(1.0) / np.asarray(kf.level_sigma2, np.float32)).astype(np.float32))
    point_ids = sorted(int(i) for i in points)
    xw = np.array([np.asarray(points[pid], np.float32).reshape(3) for pid in point_ids], np.float32).reshape(-1, 3)
    edge_begin, edge_kf, kp_un, u_right, inv_sigma2, pairs = [0], [], [], [], [], []
    for pid in point_ids:
        obs = observations.get(pid, {})
        for kid in sorted(obs):
            if kid not in index:
                continue
            kf, idx = keyframes[kid], int(obs[kid])
            edge_kf.append(index[kid])
            kp_un.append((kf.keys_un["x"][idx], kf.keys_un["y"][idx]))
            u_right.append(kf.u_right[idx])
            inv_sigma2.append(inv_level[index[kid]][int(kf.keys_un["octave"][idx])])
            pairs.append((kid, pid))
        edge_begin.append(len(edge_kf))
    ne = len(edge_kf)
    return SimpleNamespace(n_kf=nk, n_points=len(point_ids), n_edges=ne, tcw=tcw, k=k, bf=bf, fixed=fixed, xw=xw,
                           edge_begin=np.array(edge_begin, np.int32), edge_kf=np.array(edge_kf, np.int32),
                           kp_un=np.array(kp_un, np.float32).reshape(ne, 2), u_right=np.array(u_right, np.float32),
                           inv_sigma2=np.array(inv_sigma2, np.float32), stop_at_poll=int(stop_at_poll),
                           kf_ids=kf_ids, point_ids=point_ids, edge_pairs=pairs)


class LocalBundleAdjuster:
    """The device handle: a workspace for local maps up to the given bounds; reused from call to call.
    device < 0 gives a host-only handle (argument checks only)."""

    def __init__(self, max_free_kf: int = 32, max_kf: int = 128, max_points: int = 4096, max_edges: int = 32768,
                 device: int = 0):
        self._lib = L.lib()
        h = c_void_p()
        L.check(self._lib.orbfe_lba_create(int(device), int(max_free_kf), int(max_kf), int(max_points), int(max_edges),
                                           byref(h)), "orbfe_lba_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_lba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, p, stop_flag=None) -> SimpleNamespace:
        """orbfe_lba_solve -> tcw (n_kf, 12) float32, xw (n_points, 3) float32, erase / level1 (bool per
        edge), erase_words / level1_words, n_erase, rounds_run, flags, polls, rounds (n_active, iterations,
        trials, rejected_trials, stop, n_flagged, lam, chi2). stop_flag: an optional ctypes c_int."""
        nk, npt, ne = int(p.n_kf), int(p.n_points), int(p.n_edges)
        a = dict(tcw=(p.tcw, np.float32, 12 * nk), k=(p.k, np.float32, 4 * nk), bf=(p.bf, np.float32, nk),
                 fixed=(p.fixed, np.uint8, nk), xw=(p.xw, np.float32, 3 * npt), edge_begin=(p.edge_begin, np.int32, npt + 1),
                 edge_kf=(p.edge_kf, np.int32, ne), kp_un=(p.kp_un, np.float32, 2 * ne), u_right=(p.u_right, np.float32, ne),
                 inv_sigma2=(p.inv_sigma2, np.float32, ne))
        P, R, keep = L.lba_problem(), L.lba_result(), {}
        P.n_kf, P.n_points, P.n_edges = nk, npt, ne
        for name, (src, dtype, count) in a.items():
            arr = np.ascontiguousarray(src, dtype).reshape(-1)
            if len(arr) != count:
                raise ValueError(f"{name} must hold {count} values")
            keep[name] = arr if count else np.zeros(1, dtype)
            setattr(P, name, L.ptr(keep[name]))
        P.stop_flag = c_void_p(0) if stop_flag is None else c_void_p(int(np.uintp(_address(stop_flag))))
        P.stop_at_poll = int(getattr(p, "stop_at_poll", -1))
        words = max((ne + 63) // 64, 1)
        tcw, xw = np.zeros(max(12 * nk, 1), np.float32), np.zeros(max(3 * npt, 1), np.float32)
        erase, level1 = np.zeros(words, np.uint64), np.zeros(words, np.uint64)
        R.tcw, R.xw, R.mask_words, R.erase_mask, R.level1_mask = L.ptr(tcw), L.ptr(xw), words, L.ptr(erase), L.ptr(level1)
        L.check(self._lib.orbfe_lba_solve(self._h, byref(P), byref(R)), "orbfe_lba_solve")
        bits = lambda w: np.unpackbits(w.view(np.uint8), bitorder="little")[:ne].astype(bool)
        rounds = [SimpleNamespace(n_active=t.n_active, iterations=t.iterations, trials=t.trials,
                                  rejected_trials=t.rejected_trials, stop=t.stop, n_flagged=t.n_flagged,
                                  lam=float(t.lam), chi2=float(t.chi2)) for t in R.rounds]
        return SimpleNamespace(tcw=tcw[:12 * nk].reshape(nk, 12), xw=xw[:3 * npt].reshape(npt, 3), erase=bits(erase),
                               level1=bits(level1), erase_words=erase, level1_words=level1, n_erase=R.n_erase,
                               rounds_run=R.rounds_run, flags=int(R.flags), polls=R.polls, rounds=rounds)


def _address(c_obj) -> int:
    import ctypes
    return ctypes.addressof(c_obj)


def LocalBundleAdjustment(keyframes: Dict[int, object], points: Dict[int, np.ndarray],
                          observations: Mapping[int, Mapping[int, int]], local_ids: Iterable[int],
                          fixed_ids: Iterable[int] = (), adjuster: Optional[LocalBundleAdjuster] = None,
                          device: int = 0, stop_flag=None) -> List[Tuple[int, int]]:
    """void Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap) from :508 on: sets tcw of every local
    keyframe (SetPose) and every point's position (SetWorldPos) in place and returns vToErase as (keyframe
    mnId, point mnId) pairs for the caller's EraseMapPointMatch / EraseObservation. Without `adjuster` a
    handle sized for this map is created for the call."""
    p = problem_of_local_map(keyframes, points, observations, local_ids, fixed_ids)
    own = adjuster is None
    if own:
        n_free = max(int((p.fixed == 0).sum()), 1)
        adjuster = LocalBundleAdjuster(n_free, max(p.n_kf, n_free), max(p.n_points, 1), max(p.n_edges, 1), device)
    try:
        r = adjuster.solve(p, stop_flag)
    finally:
        if own:
            adjuster.close()
    if r.rounds_run > 0:
        for i, kid in enumerate(p.kf_ids):
            if not p.fixed[i]:
                keyframes[kid].tcw = r.tcw[i].reshape(3, 4).copy()
        for i, pid in enumerate(p.point_ids):
            points[pid] = r.xw[i].copy()
    return [p.edge_pairs[e] for e in np.flatnonzero(r.erase)]
