"""Sim3Solver on MI355X (include/orbfe_sim3.h): the RANSAC hypotheses of one or several
loop-closure candidates are generated, checked and selected in one device pass.

Mirrors src/Sim3Solver.cc:113-420 of the reference. `Sim3Solver` keeps the reference's interface
(SetRansacParameters, iterate, find, GetEstimated*); `solve_batch` evaluates several solvers in one
call, after which their iterate() / find() only replay the acceptance rules on the host.

The caller does the constructor's filtering (:61-101) and passes mvX3Dc1 / mvX3Dc2 and the
keypoints' mvLevelSigma2 entries. The draws of DUtils::Random::RandomInt are the caller's too
(`set_draws`); without them a numpy generator draws, which follows the reference's distribution
but not its rand() sequence.
"""
from __future__ import annotations

from ctypes import byref, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

MAX_SOLVERS, MAX_CORR, MAX_HYP = 64, 4096, 1024


class Sim3Batch:
    """The device handle: buffers for up to max_solvers solvers of max_corr correspondences and
    max_hyp hypotheses each. device < 0 gives a host-only handle (argument checks only)."""

    def __init__(self, max_solvers: int = 8, max_corr: int = 1024, max_hyp: int = 300, device: int = 0):
        self._lib = L.lib()
        self.max_solvers, self.max_corr, self.max_hyp = int(max_solvers), int(max_corr), int(max_hyp)
        h = c_void_p()
        L.check(self._lib.orbfe_sim3_create(int(device), self.max_solvers, self.max_corr, self.max_hyp,
                                            byref(h)), "orbfe_sim3_create")
        self._h = h
        self.epoch = 0  # solves so far: a solver replays only the solve it took part in

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_sim3_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, solvers: Sequence["Sim3Solver"]) -> None:
        """orbfe_sim3_solve_batch over `solvers`; each then holds its per-hypothesis results and
        the outcome of find(), and its iterate() starts from iteration 0."""
        n = len(solvers)
        S = (L.sim3_solver * max(n, 1))()
        R = (L.sim3_result * max(n, 1))()
        keep = []
        for i, s in enumerate(solvers):
            keep.append(s._fill(S[i], R[i]))
        L.check(self._lib.orbfe_sim3_solve_batch(self._h, S, n, R), "orbfe_sim3_solve_batch")
        self.epoch += 1
        for i, s in enumerate(solvers):
            s._take(self, i, R[i], keep[i])


class Sim3Solver:
    """Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) after its constructor's filter.

    x3dc1 / x3dc2: (n, 3) mvX3Dc1 / mvX3Dc2; sigma2_1 / sigma2_2: (n,) mvLevelSigma2[kp.octave] of
    the two keypoints; K1 / K2: (fx, fy, cx, cy) or a 3x3 calibration matrix."""

    def __init__(self, x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, bFixScale: bool, seed: int = 0):
        self.x3dc1 = np.ascontiguousarray(x3dc1, np.float32).reshape(-1, 3)
        self.x3dc2 = np.ascontiguousarray(x3dc2, np.float32).reshape(-1, 3)
        self.N = len(self.x3dc1)
        self.sigma2_1 = np.ascontiguousarray(sigma2_1, np.float32).reshape(-1)
        self.sigma2_2 = np.ascontiguousarray(sigma2_2, np.float32).reshape(-1)
        if not (len(self.x3dc2) == len(self.sigma2_1) == len(self.sigma2_2) == self.N):
            raise ValueError("correspondence arrays differ in length")
        self.K1, self.K2 = self._k(K1), self._k(K2)
        self.mbFixScale = bool(bFixScale)
        self._rng = np.random.default_rng(seed)
        self._draws = None
        self._hyp = None
        self._batch = None
        self.SetRansacParameters()

    @staticmethod
    def _k(K):
        K = np.asarray(K, np.float32)
        if K.shape == (3, 3):
            K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
        return np.ascontiguousarray(K.reshape(4))

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 6, maxIterations: int = 300):
        self.mRansacProb, self.mRansacMinInliers = float(probability), int(minInliers)
        self.max_iterations = int(maxIterations)
        self._batch = None  # mnIterations = 0: the next iterate() solves again
        self._state = L.sim3_state(0, 0, -1)

    def set_draws(self, rand_idx) -> None:
        """The raw RandomInt values, three per iteration: (n_hyp, 3), draw i in 0 .. N-1-i."""
        self._draws = np.ascontiguousarray(rand_idx, np.int32).reshape(-1, 3)
        self._hyp = None
        self._batch = None

    def set_hypotheses(self, t12, t21) -> None:
        """Caller-computed hypotheses (n_hyp, 3, 4) each: only the inlier check and selection run."""
        a = np.ascontiguousarray(t12, np.float32).reshape(-1, 12)
        b = np.ascontiguousarray(t21, np.float32).reshape(-1, 12)
        if len(a) != len(b):
            raise ValueError("t12 / t21 differ in length")
        self._hyp = (a, b)
        self._batch = None

    # ---- orbfe_sim3_solve_batch plumbing --------------------------------------------------------
    def _fill(self, s: L.sim3_solver, r: L.sim3_result):
        if self._hyp is None and self._draws is None and self.N >= 3:
            hi = np.array([self.N, self.N - 1, self.N - 2], np.int64)
            self._draws = self._rng.integers(0, hi, (self.max_iterations, 3)).astype(np.int32)
        n_hyp = len(self._hyp[0]) if self._hyp is not None else (len(self._draws) if self._draws is not None else 0)
        s.n = self.N
        s.x3dc1, s.x3dc2 = L.ptr(self.x3dc1), L.ptr(self.x3dc2)
        s.sigma2_1, s.sigma2_2 = L.ptr(self.sigma2_1), L.ptr(self.sigma2_2)
        s.k1[:] = [float(v) for v in self.K1]
        s.k2[:] = [float(v) for v in self.K2]
        s.fix_scale = int(self.mbFixScale)
        s.min_inliers, s.max_iterations, s.probability = self.mRansacMinInliers, self.max_iterations, self.mRansacProb
        s.n_hyp = n_hyp
        if self._hyp is not None:
            s.hyp_t12, s.hyp_t21 = L.ptr(self._hyp[0]), L.ptr(self._hyp[1])
        elif self._draws is not None:
            s.rand_idx = L.ptr(self._draws)
        cap = max(min(n_hyp, max(self.max_iterations, 1)), 1)
        words = max((self.N + 63) // 64, 1)
        out = dict(n_inliers=np.zeros(cap, np.int32), t12=np.zeros((cap, 3, 4), np.float32),
                   t21=np.zeros((cap, 3, 4), np.float32), r12=np.zeros((cap, 3, 3), np.float32),
                   tr12=np.zeros((cap, 3), np.float32), s12=np.zeros(cap, np.float32),
                   inlier_mask=np.zeros((cap, words), np.uint64))
        r.hyp_capacity, r.mask_words = cap, words
        for name, a in out.items():
            setattr(r, name, L.ptr(a))
        return out

    def _take(self, batch: Sim3Batch, index: int, r: L.sim3_result, out) -> None:
        e = r.n_evaluated
        self.n_evaluated, self.mRansacMaxIts = e, r.ransac_max_its
        self.n_inliers = out["n_inliers"][:e]
        self.t12, self.t21 = out["t12"][:e], out["t21"][:e]
        self.r12, self.tr12, self.s12 = out["r12"][:e], out["tr12"][:e], out["s12"][:e]
        self.inlier_words = out["inlier_mask"][:e]
        self.found = dict(accepted=r.accepted, nInliers=r.accepted_inliers, best=r.best,
                          mnBestInliers=r.best_inliers, bNoMore=bool(r.no_more))
        self._batch, self._index, self._epoch = batch, index, batch.epoch
        self._state = L.sim3_state(0, 0, -1)

    def inliers_of(self, k: int) -> np.ndarray:
        """mvbInliersi of hypothesis k as bool[N]."""
        return self._bits(self.inlier_words[k])

    def _bits(self, words: np.ndarray) -> np.ndarray:
        return np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")[:self.N].astype(bool)

    # ---- the reference's interface --------------------------------------------------------------
    def iterate(self, nIterations: int) -> Tuple[Optional[np.ndarray], bool, np.ndarray, int]:
        """-> (T12 as 4x4 or None, bNoMore, vbInliers over the N correspondences, nInliers)"""
        if self._batch is None:
            solve_batch([self])
        if self._batch.epoch != self._epoch:
            raise RuntimeError("the handle has solved another batch since: solve this solver again")
        words = np.zeros(max((self.N + 63) // 64, 1), np.uint64)
        out = L.sim3_iterate(mask_words=len(words), inlier_mask=L.ptr(words))
        L.check(self._batch._lib.orbfe_sim3_iterate(self._batch._h, self._index, int(nIterations),
                                                    byref(self._state), byref(out)), "orbfe_sim3_iterate")
        T = None
        if out.accepted >= 0:
            T = np.eye(4, dtype=np.float32)
            T[:3, :] = np.array(out.t12, np.float32).reshape(3, 4)
        return T, bool(out.no_more), self._bits(words), out.n_inliers

    def find(self) -> Tuple[Optional[np.ndarray], np.ndarray, int]:
        """-> (T12 or None, vbInliers12, nInliers)"""
        if self._batch is None:
            solve_batch([self])
        T, _, inl, n = self.iterate(self.mRansacMaxIts)
        return T, inl, n

    def _best(self) -> int:
        if self._batch is None or self._state.best < 0:
            raise RuntimeError("no hypothesis has been evaluated yet")
        return self._state.best

    def GetEstimatedRotation(self) -> np.ndarray:
        return self.r12[self._best()].copy()

    def GetEstimatedTranslation(self) -> np.ndarray:
        return self.tr12[self._best()].copy()

    def GetEstimatedScale(self) -> float:
        return float(self.s12[self._best()])


def solve_batch(solvers: List[Sim3Solver], batch: Optional[Sim3Batch] = None, device: int = 0) -> Sim3Batch:
    """Evaluates every solver's hypotheses in one device pass. Without `batch` a handle sized for
    these solvers is created; it is returned and stays alive while the solvers replay from it."""
    if batch is None:
        n = max([s.N for s in solvers] + [3])
        hyp = max([min(s.max_iterations, MAX_HYP) for s in solvers] + [1])
        batch = Sim3Batch(max(len(solvers), 1), n, hyp, device)
    batch.solve(solvers)
    return batch
