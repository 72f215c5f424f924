"""Initializer on MI355X (include/orbfe_init.h): the homography / fundamental RANSAC of the monocular
bootstrap and the reconstruction from the winning model, for one or several frame pairs, in one
device pass.

Mirrors src/Initializer.cc of the reference. `Initializer` keeps the reference's interface
(constructor, Initialize); `InitializerBatch.solve` evaluates several of them in one call.

The caller passes mvKeysUn[i].pt of both frames and vMatches12. The draws of
DUtils::Random::RandomInt are the caller's too (`set_draws`); without them a numpy generator draws,
which follows the reference's distribution but not its rand() sequence.
"""
from __future__ import annotations

from ctypes import byref, c_void_p
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

MAX_PROBLEMS, MAX_KEYS, MAX_MATCHES, MAX_HYP = 16, 8192, 8192, 1024


class InitializerBatch:
    """The device handle: buffers for up to max_problems problems of max_keys keypoints per frame,
    max_matches matches and max_hyp hypotheses each. device < 0 gives a host-only handle (argument
    checks only)."""

    def __init__(self, max_problems: int = 1, max_keys: int = 2048, max_matches: Optional[int] = None,
                 max_hyp: int = 200, device: int = 0):
        self._lib = L.lib()
        max_matches = max_keys if max_matches is None else max_matches
        h = c_void_p()
        L.check(self._lib.orbfe_init_create(int(device), int(max_problems), int(max_keys), int(max_matches),
                                            int(max_hyp), byref(h)), "orbfe_init_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_init_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, initializers: Sequence["Initializer"]) -> None:
        """orbfe_init_solve_batch over initializers on which prepare(keys2, vMatches12) was called; each
        then holds its outputs (`result`) and diagnostics."""
        n = len(initializers)
        P = (L.init_problem * max(n, 1))()
        R = (L.init_result * max(n, 1))()
        keep = [s._fill(P[i], R[i]) for i, s in enumerate(initializers)]
        L.check(self._lib.orbfe_init_solve_batch(self._h, P, n, R), "orbfe_init_solve_batch")
        for i, s in enumerate(initializers):
            s._take(R[i], keep[i])


class Initializer:
    """Initializer(ReferenceFrame, sigma, iterations): keys1 is (n1, 2) mvKeysUn[i].pt of the reference
    frame, K (fx, fy, cx, cy) or a 3x3 calibration matrix."""

    def __init__(self, keys1, K, sigma: float = 1.0, iterations: int = 200, seed: int = 0,
                 batch: Optional[InitializerBatch] = None, device: int = 0):
        self.keys1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        K = np.asarray(K, np.float32)
        if K.shape == (3, 3):
            K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
        self.K = np.ascontiguousarray(K.reshape(4))
        self.sigma, self.iterations = float(sigma), int(iterations)
        self.min_parallax = 1.0  # Initialize's argument to ReconstructH / ReconstructF
        self._rng = np.random.default_rng(seed)
        self._draws = None
        self._batch, self._device = batch, device
        self.keys2 = self.matches12 = None

    def set_draws(self, rand_idx) -> None:
        """The raw RandomInt values, eight per iteration: (n_hyp, 8), draw j in 0 .. N-1-j."""
        self._draws = np.ascontiguousarray(rand_idx, np.int32).reshape(-1, 8)

    def prepare(self, keys2, vMatches12) -> "Initializer":
        self.keys2 = np.ascontiguousarray(keys2, np.float32).reshape(-1, 2)
        self.matches12 = np.ascontiguousarray(vMatches12, np.int32).reshape(-1)
        if len(self.matches12) != len(self.keys1):
            raise ValueError("vMatches12 must have one entry per keypoint of the reference frame")
        return self

    # ---- orbfe_init_solve_batch plumbing --------------------------------------------------------
    def _fill(self, p: L.init_problem, r: L.init_result):
        if self.keys2 is None:
            raise RuntimeError("prepare(keys2, vMatches12) first")
        N = int((self.matches12 >= 0).sum())
        draws = self._draws
        if draws is None:
            if N >= 8:
                hi = np.array([N - j for j in range(8)], np.int64)
                draws = self._rng.integers(0, hi, (min(self.iterations, MAX_HYP), 8)).astype(np.int32)
            else:
                draws = np.zeros((0, 8), np.int32)
        n_hyp, n1 = len(draws), len(self.keys1)
        p.n1, p.n2 = n1, len(self.keys2)
        p.keys1, p.keys2, p.matches12 = L.ptr(self.keys1), L.ptr(self.keys2), L.ptr(self.matches12)
        p.k[:] = [float(v) for v in self.K]
        p.sigma, p.min_parallax, p.n_hyp = self.sigma, self.min_parallax, n_hyp
        p.rand_idx = L.ptr(draws) if n_hyp else None
        words = max((N + 63) // 64, 1)
        out = dict(p3d=np.zeros((max(n1, 1), 3), np.float32), triangulated=np.zeros(max(n1, 1), np.uint8),
                   score_h=np.zeros(max(n_hyp, 1), np.float32), score_f=np.zeros(max(n_hyp, 1), np.float32),
                   mask_h=np.zeros(words, np.uint64), mask_f=np.zeros(words, np.uint64))
        r.hyp_capacity, r.mask_words = max(n_hyp, 1), words
        for name, a in out.items():
            setattr(r, name, L.ptr(a))
        out["draws"] = draws
        return out

    def _take(self, r: L.init_result, out) -> None:
        n1, e, N = len(self.keys1), len(out["draws"]), r.n_matches
        self.N, self.n_hyp, self.flags = N, e, int(r.flags)
        self.score_h, self.score_f = out["score_h"][:e], out["score_f"][:e]
        self.mask_h, self.mask_f = self._bits(out["mask_h"], N), self._bits(out["mask_f"], N)
        self.SH, self.SF, self.RH = np.float32(r.sh), np.float32(r.sf), np.float32(r.rh)
        self.model, self.best_h, self.best_f = r.model, r.best_h, r.best_f
        self.H21, self.F21 = np.array(r.h21, np.float32).reshape(3, 3), np.array(r.f21, np.float32).reshape(3, 3)
        self.n_motions = r.n_motions
        self.n_good, self.cos_parallax = np.array(r.n_good, np.int32), np.array(r.cos_parallax, np.float32)
        self.candidate, self.motion, self.parallax = r.candidate, r.motion, np.float32(r.parallax)
        self.result = (bool(r.ok), np.array(r.r21, np.float32).reshape(3, 3), np.array(r.t21, np.float32),
                       out["p3d"][:n1], out["triangulated"][:n1].astype(bool))

    @staticmethod
    def _bits(words: np.ndarray, n: int) -> np.ndarray:
        return np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")[:n].astype(bool)

    # ---- the reference's interface --------------------------------------------------------------
    def Initialize(self, keys2, vMatches12) -> Tuple[bool, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """-> (ok, R21 3x3, t21, vP3D (n1, 3), vbTriangulated (n1,)); the last four are zero when not ok."""
        self.prepare(keys2, vMatches12)
        if self._batch is None:
            hyp = len(self._draws) if self._draws is not None else min(self.iterations, MAX_HYP)
            keys = max(len(self.keys1), len(self.keys2), 8)
            self._batch = InitializerBatch(1, keys, keys, max(hyp, 1), self._device)
        self._batch.solve([self])
        return self.result
