"""Optimizer::BundleAdjustment / GlobalBundleAdjustemnt on MI355X (include/orbfe_gba.h): the Levenberg-
Marquardt of a whole map, the points marginalised by a Schur complement over the covisible keyframe
pairs, the reduced pose system a 6x6 block envelope.

Mirrors src/Optimizer.cc:51-240 of the reference. `problem_of_map` performs the gather of :70-186 from
KeyFrame objects, map point positions and the observation table; `GlobalBundleAdjuster` is the device
handle; `GlobalBundleAdjustment(...)` writes the poses and positions back (:192-238) and returns the ids
of the points that were not included. The nLoopKF bookkeeping, RunGlobalBundleAdjustment's propagation
and UpdateNormalAndDepth stay with the caller.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_int, c_void_p
from types import SimpleNamespace
from typing import Dict, List, Mapping, Optional

import numpy as np

from . import _lib as L

MAX_KF, MAX_POINTS, MAX_EDGES, MAX_ENV_BLOCKS = L.GBA_MAX_KF, L.GBA_MAX_POINTS, L.GBA_MAX_EDGES, L.GBA_MAX_ENV_BLOCKS


def problem_of_map(keyframes: Mapping[int, object], points: Mapping[int, Optional[np.ndarray]],
                   observations: Mapping[int, Mapping[int, int]], n_iterations: int = 10, robust: bool = True,
                   stop_at_poll: int = -1) -> SimpleNamespace:
    """keyframes: mnId -> KeyFrame (tcw, fx fy cx cy, bf, keys_un, u_right, level_sigma2; an optional `bad`);
    points: mnId -> GetWorldPos(), None for a bad point; observations: point mnId -> {keyframe mnId ->
    keypoint index} (GetObservations()). Bad keyframes (:76) and bad points (:94) are skipped, and so is an
    observation by a keyframe that is not listed (:111). Keyframes and points ascend in mnId: g2o's
    Hessian order. The keyframe with mnId 0 is fixed (:81). The problem carries kf_ids and point_ids."""
    kf_ids = sorted(int(i) for i, kf in keyframes.items() if not getattr(kf, "bad", False))
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
        fixed[i] = 1 if kid == 0 else 0
        inv_level.append((np.float32(1.0) / np.asarray(kf.level_sigma2, np.float32)).astype(np.float32))
    point_ids = sorted(int(i) for i, x in points.items() if x is not None)
    xw = np.array([np.asarray(points[pid], np.float32).reshape(3) for pid in point_ids], np.float32).reshape(-1, 3)
    edge_begin, edge_kf, kp_un, u_right, inv_sigma2 = [0], [], [], [], []
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
        edge_begin.append(len(edge_kf))
    ne = len(edge_kf)
    return SimpleNamespace(n_kf=nk, n_points=len(point_ids), n_edges=ne, tcw=tcw, k=k, bf=bf, fixed=fixed, xw=xw,
                           edge_begin=np.array(edge_begin, np.int32), edge_kf=np.array(edge_kf, np.int32),
                           kp_un=np.array(kp_un, np.float32).reshape(ne, 2), u_right=np.array(u_right, np.float32),
                           inv_sigma2=np.array(inv_sigma2, np.float32), n_iterations=int(n_iterations),
                           robust=1 if robust else 0, stop_at_poll=int(stop_at_poll), kf_ids=kf_ids, point_ids=point_ids)


def _c_problem(p, stop_flag=None):
    """-> (L.gba_problem, the arrays it points into)"""
    nk, npt, ne = int(p.n_kf), int(p.n_points), int(p.n_edges)
    a = dict(tcw=(p.tcw, np.float32, 12 * nk), k=(p.k, np.float32, 4 * nk), bf=(p.bf, np.float32, nk),
             fixed=(p.fixed, np.uint8, nk), xw=(p.xw, np.float32, 3 * npt), edge_begin=(p.edge_begin, np.int32, npt + 1),
             edge_kf=(p.edge_kf, np.int32, ne), kp_un=(p.kp_un, np.float32, 2 * ne), u_right=(p.u_right, np.float32, ne),
             inv_sigma2=(p.inv_sigma2, np.float32, ne))
    P, keep = L.gba_problem(), {}
    P.n_kf, P.n_points, P.n_edges = nk, npt, ne
    for name, (src, dtype, count) in a.items():
        arr = np.ascontiguousarray(src, dtype).reshape(-1)
        if len(arr) != count:
            raise ValueError(f"{name} must hold {count} values")
        keep[name] = arr if count else np.zeros(1, dtype)
        setattr(P, name, L.ptr(keep[name]))
    P.n_iterations, P.robust = int(getattr(p, "n_iterations", 10)), int(getattr(p, "robust", 1))
    P.stop_flag = c_void_p(0) if stop_flag is None else c_void_p(ctypes.addressof(stop_flag))
    P.stop_at_poll = int(getattr(p, "stop_at_poll", -1))
    return P, keep


def envelope(p) -> SimpleNamespace:
    """orbfe_gba_envelope: the argument checks and the plan on the host -> env_blocks, schur_blocks"""
    P, keep = _c_problem(p)
    env, schur = c_int(0), c_int(0)
    L.check(L.lib().orbfe_gba_envelope(byref(P), byref(env), byref(schur)), "orbfe_gba_envelope")
    return SimpleNamespace(env_blocks=env.value, schur_blocks=schur.value)


class GlobalBundleAdjuster:
    """The device handle: a workspace for maps up to the given bounds; reused from call to call.
    device < 0 gives a host-only handle (argument checks and the plan only)."""

    def __init__(self, max_kf: int = 512, max_points: int = 32768, max_edges: int = 262144, max_env_blocks: int = 65536,
                 device: int = 0):
        self._lib = L.lib()
        h = c_void_p()
        L.check(self._lib.orbfe_gba_create(int(device), int(max_kf), int(max_points), int(max_edges), int(max_env_blocks),
                                           byref(h)), "orbfe_gba_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_gba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, p, stop_flag=None) -> SimpleNamespace:
        """orbfe_gba_solve -> tcw (n_kf, 12) float32, xw (n_points, 3) float32 and the trace's fields
        (n_active, iterations, trials, rejected_trials, stop, lam, chi2, env_blocks, schur_blocks, flags,
        polls). stop_flag: an optional ctypes c_int."""
        nk, npt = int(p.n_kf), int(p.n_points)
        P, keep = _c_problem(p, stop_flag)
        R = L.gba_result()
        tcw, xw = np.zeros(max(12 * nk, 1), np.float32), np.zeros(max(3 * npt, 1), np.float32)
        R.tcw, R.xw = L.ptr(tcw), L.ptr(xw)
        L.check(self._lib.orbfe_gba_solve(self._h, byref(P), byref(R)), "orbfe_gba_solve")
        t = R.trace
        return SimpleNamespace(tcw=tcw[:12 * nk].reshape(nk, 12), xw=xw[:3 * npt].reshape(npt, 3), n_active=t.n_active,
                               iterations=t.iterations, trials=t.trials, rejected_trials=t.rejected_trials, stop=t.stop,
                               lam=float(t.lam), chi2=float(t.chi2), env_blocks=t.env_blocks, schur_blocks=t.schur_blocks,
                               flags=int(t.flags), polls=t.polls)


def GlobalBundleAdjustment(keyframes: Dict[int, object], points: Dict[int, Optional[np.ndarray]],
                           observations: Mapping[int, Mapping[int, int]], n_iterations: int = 10, stop_flag=None,
                           robust: bool = True, adjuster: Optional[GlobalBundleAdjuster] = None,
                           device: int = 0) -> List[int]:
    """void Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust): sets tcw
    of every keyframe that is not bad and the position of every included point in place, and returns the
    mnIds of the points that were not included (vbNotIncludedMP: no observation by a listed keyframe).
    Without `adjuster` a handle sized by orbfe_gba_envelope is created for the call."""
    p = problem_of_map(keyframes, points, observations, n_iterations, robust)
    own = adjuster is None
    if own:
        adjuster = GlobalBundleAdjuster(max(p.n_kf, 1), max(p.n_points, 1), max(p.n_edges, 1),
                                        max(envelope(p).env_blocks, 1), device)
    try:
        r = adjuster.solve(p, stop_flag)
    finally:
        if own:
            adjuster.close()
    included = np.diff(p.edge_begin) > 0
    for i, kid in enumerate(p.kf_ids):
        keyframes[kid].tcw = r.tcw[i].reshape(3, 4).copy()
    for i, pid in enumerate(p.point_ids):
        if included[i]:
            points[pid] = r.xw[i].copy()
    return [pid for i, pid in enumerate(p.point_ids) if not included[i]]
