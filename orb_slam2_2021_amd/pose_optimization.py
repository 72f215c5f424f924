"""Optimizer::PoseOptimization on MI355X (include/orbfe_poseopt.h): the motion-only Levenberg-Marquardt
of one frame, or of a batch of frames (Relocalization's surviving candidates), in one launch.

Mirrors src/Optimizer.cc:242-452 of the reference. A problem is indexed by the frame's keypoints:
valid[i] says whether keypoint i has a map point, and bit i of the result's outlier flags is
mvbOutlier[i]. `PoseOptimizer.optimize` takes problems (anything with the fields n, valid, xw, kp_un,
u_right, inv_sigma2, k, bf, tcw) or Frame objects that carry `world_pos` (GetWorldPos() per keypoint);
`PoseOptimization(frame)` keeps the reference's signature.
"""
from __future__ import annotations

from ctypes import c_void_p, byref
from types import SimpleNamespace
from typing import List, Optional, Sequence

import numpy as np

from . import _lib as L
from .frames import Frame

MAX_PROBLEMS, MAX_OBS = 64, 4096


def problem_of_frame(frame: Frame, world_pos=None) -> SimpleNamespace:
    """What the caller gathers from a Frame: mvpMapPoints[i] != NULL, GetWorldPos(), mvKeysUn[i].pt,
    mvuRight, mvInvLevelSigma2[octave] (1.0f / mvLevelSigma2, Frame.cc's table), the camera and mTcw."""
    xw = world_pos if world_pos is not None else getattr(frame, "world_pos", None)
    if xw is None or frame.tcw is None:
        raise ValueError("PoseOptimization needs the frame's pose (tcw) and its map points' world_pos")
    n = frame.N
    inv_level = (np.float32(1.0) / frame.level_sigma2.astype(np.float32)).astype(np.float32)
    return SimpleNamespace(
        n=n, valid=(frame.mp_state != L.ORBFE_MP_NONE).astype(np.uint8),
        xw=np.ascontiguousarray(xw, np.float32).reshape(n, 3),
        kp_un=np.ascontiguousarray(np.stack([frame.keys_un["x"], frame.keys_un["y"]], 1), np.float32),
        u_right=frame.u_right, inv_sigma2=np.ascontiguousarray(inv_level[frame.keys_un["octave"]]),
        k=np.array([frame.fx, frame.fy, frame.cx, frame.cy], np.float32), bf=np.float32(frame.bf),
        tcw=np.ascontiguousarray(frame.tcw, np.float32).reshape(12))


class PoseOptimizer:
    """The device handle: buffers for up to max_problems problems of max_obs keypoints each.
    device < 0 gives a host-only handle (argument checks only)."""

    def __init__(self, max_problems: int = 8, max_obs: int = 2048, device: int = 0):
        self._lib = L.lib()
        self.max_problems, self.max_obs = int(max_problems), int(max_obs)
        h = c_void_p()
        L.check(self._lib.orbfe_poseopt_create(int(device), self.max_problems, self.max_obs, byref(h)),
                "orbfe_poseopt_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_poseopt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def optimize(self, frames_or_problems: Sequence) -> List[SimpleNamespace]:
        """orbfe_poseopt_batch -> one result per problem: tcw (3x4 float32), pose_q_t (7 float64),
        outlier (bool[n], mvbOutlier), outlier_words, n_initial, n_bad, n_inliers, rounds_run, flags and
        rounds (the per-round trace: n_active, iterations, trials, rejected_trials, stop, n_bad, lam,
        chi2)."""
        probs = [problem_of_frame(p) if isinstance(p, Frame) else p for p in frames_or_problems]
        n = len(probs)
        Pa = (L.poseopt_problem * max(n, 1))()
        Ra = (L.poseopt_result * max(n, 1))()
        keep = []
        for i, p in enumerate(probs):
            arrays = dict(valid=np.ascontiguousarray(p.valid, np.uint8).reshape(-1),
                          xw=np.ascontiguousarray(p.xw, np.float32).reshape(-1),
                          kp_un=np.ascontiguousarray(p.kp_un, np.float32).reshape(-1),
                          u_right=np.ascontiguousarray(p.u_right, np.float32).reshape(-1),
                          inv_sigma2=np.ascontiguousarray(p.inv_sigma2, np.float32).reshape(-1))
            pn = int(p.n)
            for name, per in (("valid", 1), ("xw", 3), ("kp_un", 2), ("u_right", 1), ("inv_sigma2", 1)):
                if len(arrays[name]) != per * pn:
                    raise ValueError(f"problem {i}: {name} must hold {per} value(s) per keypoint")
            words = np.zeros(max((pn + 63) // 64, 1), np.uint64)
            Pa[i].n = pn
            for name, a in arrays.items():
                setattr(Pa[i], name, L.ptr(a))
            Pa[i].k[:] = [float(v) for v in np.asarray(p.k, np.float32).reshape(4)]
            Pa[i].bf = float(np.float32(p.bf))
            Pa[i].tcw[:] = [float(v) for v in np.asarray(p.tcw, np.float32).reshape(-1)[:12]]
            Ra[i].mask_words = len(words)
            Ra[i].outlier_mask = L.ptr(words)
            keep.append((arrays, words))
        L.check(self._lib.orbfe_poseopt_batch(self._h, Pa, n, Ra), "orbfe_poseopt_batch")
        out = []
        for i, p in enumerate(probs):
            r, words = Ra[i], keep[i][1]
            bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:int(p.n)].astype(bool)
            rounds = [SimpleNamespace(n_active=t.n_active, iterations=t.iterations, trials=t.trials,
                                      rejected_trials=t.rejected_trials, stop=t.stop, n_bad=t.n_bad,
                                      lam=float(t.lam), chi2=float(t.chi2)) for t in r.rounds]
            out.append(SimpleNamespace(tcw=np.array(r.tcw, np.float32).reshape(3, 4),
                                       pose_q_t=np.array(r.pose_q_t, np.float64), outlier=bits, outlier_words=words,
                                       n_initial=r.n_initial, n_bad=r.n_bad, n_inliers=r.n_inliers,
                                       rounds_run=r.rounds_run, flags=int(r.flags), rounds=rounds))
        return out


def PoseOptimization(frame: Frame, optimizer: Optional[PoseOptimizer] = None, device: int = 0) -> int:
    """int Optimizer::PoseOptimization(Frame* pFrame): sets frame.tcw (SetPose) and frame.outlier
    (mvbOutlier, bool per keypoint) and returns nInitialCorrespondences - nBad. The frame carries its map
    points' positions as frame.world_pos, (N, 3) float32. Without `optimizer` a handle sized for this
    frame is created for the call."""
    own = optimizer is None
    if own:
        optimizer = PoseOptimizer(1, max(frame.N, 1), device)
    try:
        r = optimizer.optimize([frame])[0]
    finally:
        if own:
            optimizer.close()
    outlier = getattr(frame, "outlier", None)
    if outlier is None or len(outlier) != frame.N:
        outlier = np.zeros(frame.N, bool)
    valid = frame.mp_state != L.ORBFE_MP_NONE
    outlier = np.array(outlier, bool)
    outlier[valid] = r.outlier[valid]  # :291, :325: only keypoints with a map point are written
    frame.outlier = outlier
    if r.n_initial >= 3:
        frame.tcw = r.tcw.copy()
    return r.n_inliers
