"""PnPsolver on MI355X (include/orbfe_pnp.h): the EPnP RANSAC hypotheses of one or several
relocalisation candidates are generated, checked, refined and selected in one device pass.

Mirrors src/PnPsolver.cc:66-349 of the reference. `PnPsolver` keeps the reference's interface
(SetRansacParameters, iterate, find); `PnPBatch.solve` evaluates several solvers in one call, after
which their iterate() / find() only replay the acceptance rules on the host.

The caller does the constructor's filtering (:66-117) and passes mvP3Dw, mvP2D, the keypoints'
mvLevelSigma2 entries and, optionally, mvKeyPointIndices with the number of the frame's keypoints.
The draws of DUtils::Random::RandomInt are the caller's too (`set_draws`); without them a numpy
generator draws, which follows the reference's distribution but not its rand() sequence.
"""
from __future__ import annotations

from ctypes import byref, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

MAX_SOLVERS, MAX_CORR, MAX_HYP, MAX_RECORDS = 64, 4096, 1024, 16


class PnPBatch:
    """The device handle: buffers for up to max_solvers solvers of max_corr correspondences and
    max_hyp hypotheses each. device < 0 gives a host-only handle (argument checks only)."""

    def __init__(self, max_solvers: int = 8, max_corr: int = 1024, max_hyp: int = 300, device: int = 0):
        self._lib = L.lib()
        self.max_solvers, self.max_corr, self.max_hyp = int(max_solvers), int(max_corr), int(max_hyp)
        h = c_void_p()
        L.check(self._lib.orbfe_pnp_create(int(device), self.max_solvers, self.max_corr, self.max_hyp,
                                           byref(h)), "orbfe_pnp_create")
        self._h = h
        self.epoch = 0  # solves so far: a solver replays only the solve it took part in

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_pnp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, solvers: Sequence["PnPsolver"]) -> None:
        """orbfe_pnp_solve_batch over `solvers`; each then holds its per-hypothesis and per-record
        results and the outcome of find(), and its iterate() starts from iteration 0."""
        n = len(solvers)
        S = (L.pnp_solver * max(n, 1))()
        R = (L.pnp_result * max(n, 1))()
        keep = [s._fill(S[i], R[i]) for i, s in enumerate(solvers)]
        L.check(self._lib.orbfe_pnp_solve_batch(self._h, S, n, R), "orbfe_pnp_solve_batch")
        self.epoch += 1
        for i, s in enumerate(solvers):
            s._take(self, i, R[i], keep[i])


class PnPsolver:
    """PnPsolver(F, vpMapPointMatches) after its constructor's filter.

    p3dw: (n, 3) mvP3Dw; p2d: (n, 2) mvP2D; sigma2: (n,) mvSigma2; K: (fx, fy, cx, cy) or a 3x3
    calibration matrix. key_point_indices / n_keypoints: mvKeyPointIndices and
    mvpMapPointMatches.size(); when given, vbInliers is scattered through them as :240-245 does."""

    def __init__(self, p3dw, p2d, sigma2, K, key_point_indices=None, n_keypoints: Optional[int] = None, seed: int = 0):
        self.p3dw = np.ascontiguousarray(p3dw, np.float32).reshape(-1, 3)
        self.p2d = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        self.N = len(self.p3dw)
        if not (len(self.p2d) == len(self.sigma2) == self.N):
            raise ValueError("correspondence arrays differ in length")
        K = np.asarray(K, np.float32)
        if K.shape == (3, 3):
            K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
        self.K = np.ascontiguousarray(K.reshape(4))
        self.mvKeyPointIndices = None
        if key_point_indices is not None:
            self.mvKeyPointIndices = np.ascontiguousarray(key_point_indices, np.int64).reshape(-1)
            if len(self.mvKeyPointIndices) != self.N:
                raise ValueError("key_point_indices must have one entry per correspondence")
            self.n_keypoints = int(n_keypoints) if n_keypoints is not None else int(self.mvKeyPointIndices.max(initial=-1)) + 1
        self._rng = np.random.default_rng(seed)
        self._draws = None
        self._batch = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 8, maxIterations: int = 300,
                            minSet: int = 4, epsilon: float = 0.4, th2: float = 5.991):
        self.params = (float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon), float(th2))
        self._batch = None  # mnIterations = 0: the next iterate() solves again
        self._state = L.pnp_state(0, 0, -1)

    def set_draws(self, rand_idx) -> None:
        """The raw RandomInt values, four per iteration: (n_hyp, 4), draw i in 0 .. N-1-i."""
        self._draws = np.ascontiguousarray(rand_idx, np.int32).reshape(-1, 4)
        self._batch = None

    # ---- orbfe_pnp_solve_batch plumbing ---------------------------------------------------------
    def _fill(self, s: L.pnp_solver, r: L.pnp_result):
        if self._draws is None:
            if self.N >= 4:
                hi = np.array([self.N, self.N - 1, self.N - 2, self.N - 3], np.int64)
                self._draws = self._rng.integers(0, hi, (min(self.params[2], MAX_HYP), 4)).astype(np.int32)
            else:
                self._draws = np.zeros((0, 4), np.int32)
        n_hyp = len(self._draws)
        s.n = self.N
        s.p3dw, s.p2d, s.sigma2 = L.ptr(self.p3dw), L.ptr(self.p2d), L.ptr(self.sigma2)
        s.k[:] = [float(v) for v in self.K]
        (s.probability, s.min_inliers, s.max_iterations, s.min_set, s.epsilon, s.th2) = self.params
        s.n_hyp = n_hyp
        s.rand_idx = L.ptr(self._draws) if n_hyp else None
        cap, rc = max(n_hyp, 1), MAX_RECORDS
        words = max((self.N + 63) // 64, 1)
        out = dict(n_inliers=np.zeros(cap, np.int32), inlier_mask=np.zeros((cap, words), np.uint64),
                   r=np.zeros((cap, 3, 3), np.float64), t=np.zeros((cap, 3), np.float64),
                   tcw=np.zeros((cap, 3, 4), np.float32), n_chosen=np.zeros(cap, np.int32),
                   flags=np.zeros(cap, np.uint32),
                   records=np.zeros(rc, np.int32), refined_inliers=np.zeros(rc, np.int32),
                   refined_mask=np.zeros((rc, words), np.uint64), refined_r=np.zeros((rc, 3, 3), np.float64),
                   refined_t=np.zeros((rc, 3), np.float64), refined_tcw=np.zeros((rc, 3, 4), np.float32),
                   refined_n_chosen=np.zeros(rc, np.int32), refined_flags=np.zeros(rc, np.uint32))
        r.hyp_capacity, r.rec_capacity, r.mask_words = cap, rc, words
        for name, a in out.items():
            setattr(r, name, L.ptr(a))
        return out

    def _take(self, batch: PnPBatch, index: int, r: L.pnp_result, out) -> None:
        e, nr = r.n_evaluated, r.n_records
        self.n_evaluated, self.n_records = e, nr
        self.mRansacMaxIts, self.mRansacMinInliers, self.mRansacEpsilon = (r.ransac_max_its, r.ransac_min_inliers,
                                                                           float(r.ransac_epsilon))
        self.n_inliers, self.inlier_words = out["n_inliers"][:e], out["inlier_mask"][:e]
        self.r, self.t, self.tcw = out["r"][:e], out["t"][:e], out["tcw"][:e]
        self.n_chosen, self.flags = out["n_chosen"][:e], out["flags"][:e]
        self.records, self.refined_inliers = out["records"][:nr], out["refined_inliers"][:nr]
        self.refined_words = out["refined_mask"][:nr]
        self.refined_r, self.refined_t, self.refined_tcw = out["refined_r"][:nr], out["refined_t"][:nr], out["refined_tcw"][:nr]
        self.refined_n_chosen, self.refined_flags = out["refined_n_chosen"][:nr], out["refined_flags"][:nr]
        self.found = dict(accepted=r.accepted, accepted_inliers=r.accepted_inliers, best=r.best,
                          best_inliers=r.best_inliers, no_more=int(r.no_more))
        self._batch, self._index, self._epoch = batch, index, batch.epoch
        self._state = L.pnp_state(0, 0, -1)

    def inliers_of(self, k: int) -> np.ndarray:
        """mvbInliersi of hypothesis k as bool[N]."""
        return self._bits(self.inlier_words[k])

    def refined_inliers_of(self, j: int) -> np.ndarray:
        """mvbRefinedInliers of record j as bool[N]."""
        return self._bits(self.refined_words[j])

    def _bits(self, words: np.ndarray) -> np.ndarray:
        return np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")[:self.N].astype(bool)

    def _scatter(self, inl: np.ndarray, returned: int) -> np.ndarray:
        if self.mvKeyPointIndices is None:
            return inl
        if not returned:
            return np.zeros(0, bool)  # vbInliers.clear()
        vb = np.zeros(self.n_keypoints, bool)
        vb[self.mvKeyPointIndices[inl]] = True
        return vb

    # ---- the reference's interface --------------------------------------------------------------
    def iterate(self, nIterations: int) -> Tuple[Optional[np.ndarray], bool, np.ndarray, int]:
        """-> (Tcw as 4x4 or None, bNoMore, vbInliers, nInliers)"""
        if self._batch is None:
            solve_batch([self])
        if self._batch.epoch != self._epoch:
            raise RuntimeError("the handle has solved another batch since: solve this solver again")
        words = np.zeros(max((self.N + 63) // 64, 1), np.uint64)
        out = L.pnp_iterate(mask_words=len(words), inlier_mask=L.ptr(words))
        L.check(self._batch._lib.orbfe_pnp_iterate(self._batch._h, self._index, int(nIterations),
                                                   byref(self._state), byref(out)), "orbfe_pnp_iterate")
        self.last_iterate = dict(returned=out.returned, accepted=out.accepted, no_more=out.no_more,
                                 n_inliers=out.n_inliers)
        T = None
        if out.returned:
            T = np.eye(4, dtype=np.float32)
            T[:3, :] = np.array(out.tcw, np.float32).reshape(3, 4)
        return T, bool(out.no_more), self._scatter(self._bits(words), out.returned), out.n_inliers

    def find(self) -> Tuple[Optional[np.ndarray], np.ndarray, int]:
        """-> (Tcw or None, vbInliers, nInliers)"""
        if self._batch is None:
            solve_batch([self])
        T, _, inl, n = self.iterate(self.mRansacMaxIts)
        return T, inl, n


def solve_batch(solvers: List[PnPsolver], batch: Optional[PnPBatch] = None, device: int = 0) -> PnPBatch:
    """Evaluates every solver's hypotheses in one device pass. Without `batch` a handle sized for
    these solvers is created; it is returned and stays alive while the solvers replay from it."""
    if batch is None:
        n = max([s.N for s in solvers] + [4])
        hyp = max([len(s._draws) if s._draws is not None else min(s.params[2], MAX_HYP) for s in solvers] + [1])
        batch = PnPBatch(max(len(solvers), 1), n, hyp, device)
    batch.solve(solvers)
    return batch
