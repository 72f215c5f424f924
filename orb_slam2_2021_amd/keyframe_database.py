"""KeyFrameDatabase on MI355X (include/orbfe_kfdb.h): the keyframes' BowVectors stay on the
device, DetectRelocalizationCandidates / DetectLoopCandidates run there.

Mirrors src/KeyFrameDatabase.cc:33-315 of the reference: add / erase / clear and the two queries,
which return the reference's candidate list (same keyframes, same order) together with the
sharing list they were computed from.
"""
from __future__ import annotations

from ctypes import byref, c_int, c_void_p
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .vocabulary import BowVector, ORBVocabulary

RELOC, LOOP = 0, 1


@dataclass
class SharingList:
    """lKFsSharingWords of one query, in the reference's discovery order."""

    kf_ids: np.ndarray        # int64
    common_words: np.ndarray  # int32: mnRelocWords / mnLoopWords
    scored: np.ndarray        # bool: common_words > min_common
    scores: np.ndarray        # float32: si where scored, else 0
    max_common: int
    min_common: int


class KeyFrameDatabase:
    def __init__(self, voc: ORBVocabulary, max_keyframes: int = 4096, max_words: int = 2048,
                 device: int = 0):
        self._lib = L.lib()
        self._voc = voc  # the handle reads the vocabulary at creation only; kept for callers
        self.max_keyframes, self.max_words = int(max_keyframes), int(max_words)
        h = c_void_p()
        L.check(self._lib.orbfe_kfdb_create(voc._h, self.max_keyframes, self.max_words, int(device),
                                            byref(h)), "orbfe_kfdb_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = c_int()
        L.check(self._lib.orbfe_kfdb_size(self._h, byref(n)), "orbfe_kfdb_size")
        return n.value

    @staticmethod
    def _vec(bow):
        words = np.ascontiguousarray(bow.words, np.uint32)
        weights = np.ascontiguousarray(bow.weights, np.float64)
        if len(words) != len(weights):
            raise ValueError("BowVector words / weights differ in length")
        return words, weights

    def add(self, kf_id: int, bow: BowVector) -> None:
        words, weights = self._vec(bow)
        L.check(self._lib.orbfe_kfdb_add(self._h, int(kf_id), L.ptr(words), L.ptr(weights), len(words)),
                "orbfe_kfdb_add")

    def add_batch_device(self, kf_ids, d_bow_words: int, d_bow_weights: int, d_bow_n: int, cap: int,
                         stream: int = 0) -> None:
        """The BowVectors ORBVocabulary.transform_batch_device wrote (stride `cap`, device counts),
        one per id, without a host copy."""
        ids = np.ascontiguousarray(kf_ids, np.int64)
        L.check(self._lib.orbfe_kfdb_add_batch_device(self._h, len(ids), L.ptr(ids), c_void_p(d_bow_words),
                                                      c_void_p(d_bow_weights), c_void_p(d_bow_n), int(cap),
                                                      c_void_p(stream)), "orbfe_kfdb_add_batch_device")

    def erase(self, kf_id: int) -> None:
        L.check(self._lib.orbfe_kfdb_erase(self._h, int(kf_id)), "orbfe_kfdb_erase")

    def clear(self) -> None:
        L.check(self._lib.orbfe_kfdb_clear(self._h), "orbfe_kfdb_clear")

    def set_covisible(self, kf_id: int, ids) -> None:
        """pKF->GetBestCovisibilityKeyFrames(10), in that order."""
        a = np.ascontiguousarray(ids, np.int64)
        L.check(self._lib.orbfe_kfdb_set_covisible(self._h, int(kf_id), L.ptr(a), len(a)),
                "orbfe_kfdb_set_covisible")

    def _query(self, q: L.kfdb_query, keep):
        cap = max(len(self), 1)
        ids = np.zeros(cap, np.int64)
        common = np.zeros(cap, np.int32)
        scored = np.zeros(cap, np.uint8)
        scores = np.zeros(cap, np.float32)
        cand = np.zeros(cap, np.int64)
        r = L.kfdb_result(capacity=cap, kf_ids=L.ptr(ids), common_words=L.ptr(common), scored=L.ptr(scored),
                          scores=L.ptr(scores), candidates=L.ptr(cand))
        L.check(self._lib.orbfe_kfdb_query(self._h, byref(q), byref(r)), "orbfe_kfdb_query")
        del keep
        s = r.n_sharing
        return (cand[:r.n_candidates].copy(),
                SharingList(ids[:s].copy(), common[:s].copy(), scored[:s].astype(bool), scores[:s].copy(),
                            r.max_common, r.min_common))

    def query(self, mode: int, bow: BowVector, min_score: float = 0.0, connected=()):
        words, weights = self._vec(bow)
        ex = np.ascontiguousarray(list(connected), np.int64)
        q = L.kfdb_query(mode=int(mode), n=len(words), words=L.ptr(words), weights=L.ptr(weights),
                         on_device=0, min_score=float(min_score), excluded=L.ptr(ex), n_excluded=len(ex))
        return self._query(q, (words, weights, ex))

    def query_device(self, mode: int, d_words: int, d_weights: int, n: int, d_n: int = 0,
                     stream: int = 0, min_score: float = 0.0, connected=()):
        """The query BowVector in device memory (`n` words, or at most `n` with the count at `d_n`)."""
        ex = np.ascontiguousarray(list(connected), np.int64)
        q = L.kfdb_query(mode=int(mode), n=int(n), words=c_void_p(d_words), weights=c_void_p(d_weights),
                         on_device=1, d_n=c_void_p(d_n), stream=c_void_p(stream),
                         min_score=float(min_score), excluded=L.ptr(ex), n_excluded=len(ex))
        return self._query(q, (ex,))

    def DetectRelocalizationCandidates(self, bow: BowVector):
        """-> (candidate ids, SharingList)   (KeyFrameDatabase.cc:201-315)"""
        return self.query(RELOC, bow)

    def DetectLoopCandidates(self, bow: BowVector, min_score: float, connected=()):
        """-> (candidate ids, SharingList); `connected` = pKF->GetConnectedKeyFrames()
        (KeyFrameDatabase.cc:74-199)"""
        return self.query(LOOP, bow, min_score, connected)
