"""Optimizer::OptimizeSim3 on MI355X (include/orbfe_optsim3.h): the 7-DoF Levenberg-Marquardt of a loop
candidate's Sim3, or of a batch of candidates, in one launch.

Mirrors src/Optimizer.cc:1050-1250 of the reference. A problem is indexed by KF1's keypoints: valid[i]
says whether correspondence i enters the optimisation, and bit i of the result's removal flags is
"vpMatches1[i] was set to NULL". `Sim3Optimizer.optimize` takes problems (anything with the fields n,
valid, p3d1c, p3d2c, kp_un1, kp_un2, inv_sigma2_1, inv_sigma2_2, k1, k2, r12, t12, s12, th2, fix_scale
and optionally r2w, t2w); `problem_of_keyframes` gathers one from two KeyFrames that carry `world_pos`
(GetWorldPos() per keypoint); `OptimizeSim3(KF1, KF2, matches12, ...)` keeps the reference's signature.
"""
from __future__ import annotations

from ctypes import c_void_p, byref
from types import SimpleNamespace
from typing import List, Optional, Sequence

import numpy as np

from . import _lib as L
from .frames import Frame, gemv_f32_double

MAX_PROBLEMS, MAX_OBS = 64, 4096


def problem_of_keyframes(KF1: Frame, KF2: Frame, matches12, R12, t12, s12, th2, fix_scale) -> SimpleNamespace:
    """What the caller gathers (:1068-1187). matches12[i] is the index in KF2 of the map point
    vpMatches1[i] (GetIndexInKeyFrame(pKF2)), or -1. A correspondence is valid when both keypoints carry
    a map point that is not bad. P3DNc = RNw * P3DNw + tNw by the CV_32F gemm rule (double accumulation,
    one rounding)."""
    for kf in (KF1, KF2):
        if getattr(kf, "world_pos", None) is None or kf.tcw is None:
            raise ValueError("OptimizeSim3 needs each keyframe's pose (tcw) and its map points' world_pos")
    n = KF1.N
    m = np.asarray(matches12, np.int64).reshape(n)
    good1 = (KF1.mp_state != L.ORBFE_MP_NONE) & (KF1.mp_state != L.ORBFE_MP_BAD)
    good2 = (KF2.mp_state != L.ORBFE_MP_NONE) & (KF2.mp_state != L.ORBFE_MP_BAD)
    i2 = np.where((m >= 0) & (m < KF2.N), m, 0)
    valid = (m >= 0) & (m < KF2.N) & good1 & good2[i2]
    inv1 = (np.float32(1.0) / KF1.level_sigma2.astype(np.float32)).astype(np.float32)
    inv2 = (np.float32(1.0) / KF2.level_sigma2.astype(np.float32)).astype(np.float32)
    p1, p2 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    kp1, kp2 = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
    is1, is2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    T1, T2 = np.asarray(KF1.tcw, np.float32).reshape(3, 4), np.asarray(KF2.tcw, np.float32).reshape(3, 4)
    w1, w2 = np.asarray(KF1.world_pos, np.float32).reshape(-1, 3), np.asarray(KF2.world_pos, np.float32).reshape(-1, 3)
    for i in np.flatnonzero(valid):
        j = int(i2[i])
        p1[i] = gemv_f32_double(T1[:, :3], w1[i], T1[:, 3])
        p2[i] = gemv_f32_double(T2[:, :3], w2[j], T2[:, 3])
        kp1[i] = KF1.keys_un["x"][i], KF1.keys_un["y"][i]
        kp2[i] = KF2.keys_un["x"][j], KF2.keys_un["y"][j]
        is1[i] = inv1[KF1.keys_un["octave"][i]]
        is2[i] = inv2[KF2.keys_un["octave"][j]]
    return SimpleNamespace(
        n=n, valid=valid.astype(np.uint8), p3d1c=p1, p3d2c=p2, kp_un1=kp1, kp_un2=kp2, inv_sigma2_1=is1, inv_sigma2_2=is2,
        k1=np.array([KF1.fx, KF1.fy, KF1.cx, KF1.cy], np.float32), k2=np.array([KF2.fx, KF2.fy, KF2.cx, KF2.cy], np.float32),
        r12=np.ascontiguousarray(R12, np.float32).reshape(9), t12=np.ascontiguousarray(t12, np.float32).reshape(3),
        s12=np.float32(s12), th2=np.float32(th2), fix_scale=int(bool(fix_scale)),
        r2w=np.ascontiguousarray(T2[:, :3]).reshape(9), t2w=np.ascontiguousarray(T2[:, 3]))


class Sim3Optimizer:
    """The device handle: buffers for up to max_problems problems of max_obs keypoints each.
    device < 0 gives a host-only handle (argument checks only)."""

    def __init__(self, max_problems: int = 8, max_obs: int = 2048, device: int = 0):
        self._lib = L.lib()
        self.max_problems, self.max_obs = int(max_problems), int(max_obs)
        h = c_void_p()
        L.check(self._lib.orbfe_optsim3_create(int(device), self.max_problems, self.max_obs, byref(h)),
                "orbfe_optsim3_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_optsim3_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def optimize(self, problems: Sequence) -> List[SimpleNamespace]:
        """orbfe_optsim3_batch -> one result per problem: removed (bool[n]), removed_words,
        n_correspondences, n_bad, n_inliers, rounds_run, flags, sim3_q_t_s (8 float64: q xyzw, t, s),
        s12_rt and scw (3x4 float32) and rounds (the per-round trace, as PoseOptimizer's)."""
        n = len(problems)
        Pa = (L.optsim3_problem * max(n, 1))()
        Ra = (L.optsim3_result * max(n, 1))()
        keep = []
        fields = (("valid", np.uint8, 1), ("p3d1c", np.float32, 3), ("p3d2c", np.float32, 3), ("kp_un1", np.float32, 2),
                  ("kp_un2", np.float32, 2), ("inv_sigma2_1", np.float32, 1), ("inv_sigma2_2", np.float32, 1))
        for i, p in enumerate(problems):
            pn = int(p.n)
            arrays = {}
            for name, dtype, per in fields:
                arrays[name] = np.ascontiguousarray(getattr(p, name), dtype).reshape(-1)
                if len(arrays[name]) != per * pn:
                    raise ValueError(f"problem {i}: {name} must hold {per} value(s) per keypoint")
                setattr(Pa[i], name, L.ptr(arrays[name]))
            words = np.zeros(max((pn + 63) // 64, 1), np.uint64)
            Pa[i].n = pn
            Pa[i].k1[:] = [float(v) for v in np.asarray(p.k1, np.float32).reshape(4)]
            Pa[i].k2[:] = [float(v) for v in np.asarray(p.k2, np.float32).reshape(4)]
            Pa[i].r12[:] = [float(v) for v in np.asarray(p.r12, np.float32).reshape(9)]
            Pa[i].t12[:] = [float(v) for v in np.asarray(p.t12, np.float32).reshape(3)]
            Pa[i].s12 = float(np.float32(p.s12))
            Pa[i].th2 = float(np.float32(p.th2))
            Pa[i].fix_scale = int(bool(p.fix_scale))
            r2w = getattr(p, "r2w", None)
            Pa[i].has_kf2 = int(r2w is not None)
            if r2w is not None:
                Pa[i].r2w[:] = [float(v) for v in np.asarray(r2w, np.float32).reshape(9)]
                Pa[i].t2w[:] = [float(v) for v in np.asarray(p.t2w, np.float32).reshape(3)]
            Ra[i].mask_words = len(words)
            Ra[i].removed_mask = L.ptr(words)
            keep.append((arrays, words))
        L.check(self._lib.orbfe_optsim3_batch(self._h, Pa, n, Ra), "orbfe_optsim3_batch")
        out = []
        for i, p in enumerate(problems):
            r, words = Ra[i], keep[i][1]
            bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:int(p.n)].astype(bool)
            rounds = [SimpleNamespace(n_active=t.n_active, iterations=t.iterations, trials=t.trials,
                                      rejected_trials=t.rejected_trials, stop=t.stop, n_bad=t.n_bad,
                                      lam=float(t.lam), chi2=float(t.chi2)) for t in r.rounds]
            out.append(SimpleNamespace(removed=bits, removed_words=words, n_correspondences=r.n_correspondences,
                                       n_bad=r.n_bad, n_inliers=r.n_inliers, rounds_run=r.rounds_run, flags=int(r.flags),
                                       sim3_q_t_s=np.array(r.sim3_q_t_s, np.float64),
                                       s12_rt=np.array(r.s12_rt, np.float32).reshape(3, 4),
                                       scw=np.array(r.scw, np.float32).reshape(3, 4), rounds=rounds))
        return out


def OptimizeSim3(KF1: Frame, KF2: Frame, matches12, R12, t12, s12, th2, fix_scale,
                 optimizer: Optional[Sim3Optimizer] = None, device: int = 0, result: Optional[dict] = None) -> int:
    """int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale): sets the removed
    entries of matches12 (an int array, KF2's keypoint index per KF1 keypoint) to -1 in place and returns
    nIn. g2oS12 is R12 / t12 / s12 as the Sim3Solver returns them; the refined Sim3 (sim3_q_t_s, s12_rt,
    scw) and the rest of the result are written into `result` when a dict is given. Without `optimizer`
    a handle sized for this keyframe is created for the call."""
    own = optimizer is None
    if own:
        optimizer = Sim3Optimizer(1, max(KF1.N, 1), device)
    try:
        r = optimizer.optimize([problem_of_keyframes(KF1, KF2, matches12, R12, t12, s12, th2, fix_scale)])[0]
    finally:
        if own:
            optimizer.close()
    matches12[r.removed] = -1
    if result is not None:
        result.update(vars(r))
    return r.n_inliers
