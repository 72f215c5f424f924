"""The reference's KeyFrameDatabase restated in plain Python -- the yardstick of the GPU
KeyFrameDatabase tests. It shares no code with the product.

Restates, statement by statement and with the reference's own containers:
  src/KeyFrameDatabase.cc:33-72    ctor / add / erase / clear: mvInvertedFile is a list per word
  :74-199                          DetectLoopCandidates
  :201-315                         DetectRelocalizationCandidates
  Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68   L1Scoring::score (the lower_bound walk)
Every `double` of the reference is a Python float, every `float` a numpy.float32 (si, accScore,
bestScore, bestAccScore, 0.75f * ..., maxCommonWords * 0.8f).

Two things are defined here as include/orbfe_kfdb.h defines them: mRelocScore starts at 0.0f when
a keyframe is added (the reference leaves it uninitialised), and every query takes a fresh query
id (so the reference's mnId == 0 artefact does not occur).
"""
import bisect

import numpy as np

F32 = np.float32

# Five common words whose terms fabs(vi - wi) - fabs(vi) - fabs(wi) are exact: with vi == wi the
# term is -2 * vi. a = -(1 + 2^-24), then four times -2^-53 (half an ulp of a).
#   left to right: a + (-2^-53) is a tie and rounds to even = a, four times: sum = a,
#                  score = (1 + 2^-24) / 2 = 0.5 + 2^-25: a float tie, to even: 0.5f
#   right to left: the small terms add exactly to -2^-51, a - 2^-51 is exact,
#                  score = 0.5 + 2^-25 + 2^-52: above the tie: 0.5f + 2^-24
# A pairwise tree gives a - 2^-52 - 2^-52: above the tie as well.
ORDER_WORDS = [3, 10, 11, 40, 77]
ORDER_WEIGHTS = [0.5 + 2.0 ** -25, 2.0 ** -54, 2.0 ** -54, 2.0 ** -54, 2.0 ** -54]


def l1_score(v1, v2, order="forward"):
    """L1Scoring::score(v1, v2); v = (ascending word list, weight list). `order="reverse"` sums
    the same terms right to left (for the tests that show the order matters)."""
    w1, x1 = v1
    w2, x2 = v2
    i1 = i2 = 0
    terms = []
    while i1 != len(w1) and i2 != len(w2):
        vi, wi = float(x1[i1]), float(x2[i2])
        if w1[i1] == w2[i2]:
            terms.append(abs(vi - wi) - abs(vi) - abs(wi))
            i1 += 1
            i2 += 1
        elif w1[i1] < w2[i2]:
            i1 = bisect.bisect_left(w1, w2[i2])  # v1.lower_bound(v2_it->first)
        else:
            i2 = bisect.bisect_left(w2, w1[i1])
    score = 0.0
    for t in (terms if order == "forward" else reversed(terms)):
        score += t
    return -score / 2.0


class RefKeyFrame:
    def __init__(self, mnId, words, weights):
        self.mnId = mnId
        self.words = [int(w) for w in words]        # mBowVec keys (std::map order)
        self.weights = [float(x) for x in weights]  # mBowVec values
        self.covisible = []                         # GetBestCovisibilityKeyFrames(10)
        self.mnRelocQuery = self.mnLoopQuery = -1
        self.mnRelocWords = self.mnLoopWords = 0
        self.mRelocScore = F32(0.0)
        self.mLoopScore = F32(0.0)

    @property
    def bow(self):
        return self.words, self.weights


class RefSharing:
    """What one query saw: lKFsSharingWords and the threshold."""

    def __init__(self):
        self.kf_ids, self.common_words, self.scored, self.scores = [], [], [], []
        self.max_common = self.min_common = 0


class RefKeyFrameDatabase:
    def __init__(self, n_words):
        self.n_words = n_words
        self.mvInvertedFile = [[] for _ in range(n_words)]
        self.kfs = {}        # id -> RefKeyFrame, for the tests' convenience
        self._query_id = 0

    def __len__(self):
        return len(self.kfs)

    def add(self, mnId, words, weights):
        assert mnId not in self.kfs
        kf = RefKeyFrame(mnId, words, weights)
        self.kfs[mnId] = kf
        for w in kf.words:
            self.mvInvertedFile[w].append(kf)
        return kf

    def erase(self, mnId):
        kf = self.kfs.pop(mnId)
        for w in kf.words:
            lKFs = self.mvInvertedFile[w]
            for k, other in enumerate(lKFs):
                if other is kf:
                    del lKFs[k]
                    break

    def clear(self):
        self.mvInvertedFile = [[] for _ in range(self.n_words)]
        self.kfs = {}

    def set_covisible(self, mnId, ids):
        assert len(ids) <= 10
        self.kfs[mnId].covisible = list(ids)

    def _neighbours(self, kf):
        return [self.kfs[i] for i in kf.covisible if i in self.kfs]

    def _new_query(self):
        self._query_id += 1
        return self._query_id

    @staticmethod
    def _sharing(lKFs, words_of, min_common, max_common, score_of):
        s = RefSharing()
        s.max_common, s.min_common = max_common, min_common
        for kf in lKFs:
            c = words_of(kf)
            s.kf_ids.append(kf.mnId)
            s.common_words.append(c)
            s.scored.append(c > min_common)
            s.scores.append(score_of(kf) if c > min_common else F32(0.0))
        return s

    def DetectRelocalizationCandidates(self, words, weights):
        F_bow = ([int(w) for w in words], [float(x) for x in weights])
        F_mnId = self._new_query()
        lKFsSharingWords = []
        for w in F_bow[0]:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != F_mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F_mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            return [], RefSharing()
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnRelocWords > maxCommonWords:
                maxCommonWords = kf.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(l1_score(F_bow, pKFi.bow))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
        sharing = self._sharing(lKFsSharingWords, lambda k: k.mnRelocWords, minCommonWords,
                                maxCommonWords, lambda k: k.mRelocScore)
        if not lScoreAndMatch:
            return [], sharing
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for first, pKFi in lScoreAndMatch:
            bestScore = first
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnRelocQuery != F_mnId:
                    continue
                accScore = F32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi.mnId not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi.mnId)
        return vpRelocCandidates, sharing

    def DetectLoopCandidates(self, words, weights, minScore, connected=()):
        pKF_bow = ([int(w) for w in words], [float(x) for x in weights])
        pKF_mnId = self._new_query()
        minScore = F32(minScore)
        spConnectedKeyFrames = set(connected)
        lKFsSharingWords = []
        for w in pKF_bow[0]:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnLoopQuery != pKF_mnId:
                    pKFi.mnLoopWords = 0
                    if pKFi.mnId not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = pKF_mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        if not lKFsSharingWords:
            return [], RefSharing()
        lScoreAndMatch = []
        maxCommonWords = 0
        for kf in lKFsSharingWords:
            if kf.mnLoopWords > maxCommonWords:
                maxCommonWords = kf.mnLoopWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = F32(l1_score(pKF_bow, pKFi.bow))
                pKFi.mLoopScore = si
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        sharing = self._sharing(lKFsSharingWords, lambda k: k.mnLoopWords, minCommonWords,
                                maxCommonWords, lambda k: k.mLoopScore)
        if not lScoreAndMatch:
            return [], sharing
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for first, pKFi in lScoreAndMatch:
            bestScore = first
            accScore = first
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):
                if pKF2.mnLoopQuery == pKF_mnId and pKF2.mnLoopWords > minCommonWords:
                    accScore = F32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpLoopCandidates = []
        for first, pKFi in lAccScoreAndMatch:
            if first > minScoreToRetain:
                if pKFi.mnId not in spAlreadyAddedKF:
                    vpLoopCandidates.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi.mnId)
        return vpLoopCandidates, sharing
