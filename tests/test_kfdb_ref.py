"""Pins of tests/kfdb_ref.py (the restated KeyFrameDatabase the GPU tests compare against) with
hand-worked answers, and the KeyFrameDatabase C ABI on a host-only handle: argument checks,
bookkeeping, no query without a device. No GPU needed."""
import os
import re
import subprocess
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

from kfdb_ref import F32, ORDER_WEIGHTS, ORDER_WORDS, RefKeyFrameDatabase, l1_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_l1_score_order_matters_in_the_last_bit():
    v = (ORDER_WORDS, ORDER_WEIGHTS)
    fwd, rev = l1_score(v, v), l1_score(v, v, order="reverse")
    assert fwd == 0.5 + 2.0 ** -25
    assert rev == 0.5 + 2.0 ** -25 + 2.0 ** -52
    assert fwd != rev
    assert F32(fwd) == F32(0.5) and F32(rev) == F32(0.5) + F32(2.0 ** -24)
    assert F32(fwd).view(np.uint32) + 1 == F32(rev).view(np.uint32)


def test_l1_score_known_answers():
    # |0.25-0.5| - 0.25 - 0.5 = -0.5 ; |0.75-0.125| - 0.75 - 0.125 = -0.25 ; word 9 / 4 not shared
    a = ([1, 4, 7], [0.25, 1.0, 0.75])
    b = ([1, 7, 9], [0.5, 0.125, 3.0])
    assert l1_score(a, b) == 0.375
    assert l1_score(b, a) == 0.375
    assert l1_score(a, ([2, 3], [1.0, 1.0])) == 0.0
    assert l1_score(a, ([], [])) == 0.0
    assert l1_score(a, a) == 2.0  # not normalised here: (0.25 + 1 + 0.75) * 2 / 2


def db_with(n_words, kfs):
    db = RefKeyFrameDatabase(n_words)
    for kf_id, words in kfs:
        db.add(kf_id, words, [0.125] * len(words))
    return db


@pytest.mark.parametrize("max_common,min_common", [(5, 4), (6, 4), (10, 8)])
def test_min_common_words_threshold(max_common, min_common):
    """int minCommonWords = maxCommonWords * 0.8f, compared with strict >."""
    db = db_with(32, [(0, range(max_common)), (1, range(min_common)), (2, range(min_common + 1)),
                      (3, range(20, 25))])
    q = list(range(max_common))
    for cand, sh in (db.DetectRelocalizationCandidates(q, [0.125] * len(q)),
                     db.DetectLoopCandidates(q, [0.125] * len(q), 0.0)):
        assert (sh.max_common, sh.min_common) == (max_common, min_common)
        assert sh.kf_ids == [0, 1, 2]
        assert sh.common_words == [max_common, min_common, min_common + 1]
        assert sh.scored == [True, False, True]  # exactly at the threshold: excluded
        assert sh.scores[1] == 0 and sh.scores[0] == F32(0.125 * max_common)
        # 0.125 * (min + 1) > 0.75 * 0.125 * max in all three cases: 2 is retained, 1 never scored
        assert sh.scores[2] == F32(0.125 * (min_common + 1))
        assert cand == [0, 2]


def test_discovery_order_and_erase_readd():
    # order = (smallest common word, add order)
    db = db_with(16, [(7, [5, 6]), (3, [2, 6]), (9, [2, 5]), (1, [6])])
    q = ([2, 5, 6], [0.125] * 3)
    assert db.DetectRelocalizationCandidates(*q)[1].kf_ids == [3, 9, 7, 1]
    db.erase(3)
    assert db.DetectRelocalizationCandidates(*q)[1].kf_ids == [9, 7, 1]
    db.add(3, [2, 6], [0.125] * 2)  # back, with a later sequence number: now behind 9 on word 2
    assert db.DetectRelocalizationCandidates(*q)[1].kf_ids == [9, 3, 7, 1]
    assert len(db) == 4
    db.clear()
    assert len(db) == 0 and db.DetectRelocalizationCandidates(*q)[0] == []


def test_stale_reloc_score_is_reused():
    """:278-281: a neighbour in the sharing list adds its mRelocScore even when this query did not
    score it -- the value of the last query that did."""
    db = db_with(32, [(0, range(0, 10)), (1, range(10, 20)), (2, [0, 10])])
    db.set_covisible(0, [1])
    db.set_covisible(1, [0, 99])  # 99 is not stored: ignored
    q1 = (list(range(10, 20)), [0.25] * 10)
    cand, sh = db.DetectRelocalizationCandidates(*q1)
    assert sh.kf_ids == [1, 2] and sh.scored == [True, False] and cand == [1]
    assert db.kfs[1].mRelocScore == F32(1.25) and db.kfs[0].mRelocScore == 0
    # second query: 0 is scored (10 words), 1 only shares word 10 (1 <= min 8) but adds its 1.25
    q2 = (list(range(0, 11)), [0.25] * 11)
    cand, sh = db.DetectRelocalizationCandidates(*q2)
    assert sh.kf_ids == [0, 2, 1] and sh.scored == [True, False, False]
    assert sh.scores[0] == F32(1.25) and sh.scores[2] == 0
    # acc(0) = 1.25 + stale 1.25; pBestKF stays 0 (strict >)
    assert cand == [0]
    db.kfs[1].mRelocScore = F32(5.0)  # were the stale score larger, the neighbour would be pBestKF
    assert db.DetectRelocalizationCandidates(*q2)[0] == [1]


def test_loop_exclusions_and_min_score():
    kfs = [(0, range(0, 10)), (1, range(0, 9)), (2, range(0, 10)), (3, range(0, 9)), (4, [30])]
    db = RefKeyFrameDatabase(40)
    w = {0: 0.25, 1: 0.0625, 2: 0.25, 3: 0.125}
    for kf_id, words in kfs:
        db.add(kf_id, words, [w.get(kf_id, 0.25)] * len(words))
    db.set_covisible(3, [1, 2, 0])
    db.set_covisible(1, [3])
    q = (list(range(0, 10)), [0.25] * 10)
    # connected {2}: never in the sharing list, not a neighbour. scores: 0 -> 2.5, 1 -> 0.5625,
    # 3 -> 1.125. minScore 1.0 drops 1 from lScoreAndMatch; it still adds to 3's accScore.
    cand, sh = db.DetectLoopCandidates(*q, 1.0, connected=[2, 77])
    assert sh.kf_ids == [0, 1, 3] and sh.max_common == 10 and sh.min_common == 8
    assert sh.scored == [True, True, True]
    assert sh.scores == [F32(2.5), F32(0.5625), F32(1.125)]
    # acc(0) = 2.5 -> best 0; acc(3) = 1.125 + 0.5625 + 2.5 = 4.1875 -> pBestKF 0 (2 is excluded)
    # retain > 0.75 * 4.1875 = 3.14: only 3's entry, whose pBestKF is 0
    assert cand == [0]
    # without the exclusion 2 is in the list and the first neighbour with the top score wins
    cand, sh = db.DetectLoopCandidates(*q, 1.0)
    assert sh.kf_ids == [0, 1, 2, 3]
    assert cand == [2]  # acc(3) = 1.125 + 0.5625 + 2.5 + 2.5, pBestKF = 2 (met first, strict >)
    # a minScore above everything: empty lScoreAndMatch
    assert db.DetectLoopCandidates(*q, 3.0)[0] == []
    # every sharing keyframe connected: empty sharing list
    cand, sh = db.DetectLoopCandidates(*q, 0.0, connected=[0, 1, 2, 3])
    assert cand == [] and sh.kf_ids == []


def test_duplicate_best_is_returned_once():
    db = db_with(32, [(0, range(0, 10)), (1, range(0, 10)), (2, range(0, 9))])
    db.kfs[0].weights = [0.25] * 10  # 0 scores highest
    db.set_covisible(1, [0])
    db.set_covisible(2, [0])
    cand, sh = db.DetectRelocalizationCandidates(list(range(10)), [0.25] * 10)
    assert sh.scored == [True, True, True]
    assert cand == [0]  # pBestKF of all three entries


# ---- the C ABI on a host-only handle -------------------------------------------------------------

def declared_functions():
    src = open(os.path.join(ROOT, "include", "orbfe_kfdb.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(orbfe_\w+)\s*\(", src))


def test_header_functions_are_exported_and_bound():
    from orb_slam2_2021_amd import _lib as L
    lib = L.lib()
    names = declared_functions()
    assert {"orbfe_kfdb_create", "orbfe_kfdb_destroy", "orbfe_kfdb_add", "orbfe_kfdb_add_batch_device",
            "orbfe_kfdb_erase", "orbfe_kfdb_clear", "orbfe_kfdb_size", "orbfe_kfdb_set_covisible",
            "orbfe_kfdb_query"} == names
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (orbfe_\w+)", out))
    assert names <= exported
    assert names <= set(L.EXPORTED)
    for n in names:
        getattr(lib, n)
    blob = open(L.LIB_PATH, "rb").read()
    assert b"k_kfdb_sweep" in blob and b"k_kfdb_finish" in blob and b"k_kfdb_add" in blob


@pytest.fixture()
def host_db():
    from orb_slam2_2021_amd import KeyFrameDatabase
    from orb_slam2_2021_amd import synthetic as S
    from orb_slam2_2021_amd.vocabulary import ORBVocabulary
    voc = ORBVocabulary.from_tree(S.Vocabulary.synthetic(k=10, levels=2), device=-1)
    assert voc.n_words == 100
    return KeyFrameDatabase(voc, max_keyframes=3, max_words=8, device=-1)


def test_host_only_handle_bookkeeping_and_argument_checks(host_db):
    from orb_slam2_2021_amd import _lib as L
    from orb_slam2_2021_amd.vocabulary import BowVector
    db = host_db
    lib = L.lib()

    def add(kf_id, words):
        w = np.asarray(words, np.uint32)
        return lib.orbfe_kfdb_add(db._h, kf_id, L.ptr(w), L.ptr(np.full(len(w), 0.5)), len(w))

    assert len(db) == 0
    assert add(5, [1, 2, 99]) == L.ORBFE_OK
    assert add(2, []) == L.ORBFE_OK  # an empty BowVector is a keyframe too
    assert len(db) == 2
    assert add(7, [3, 2]) == L.ORBFE_ERR_ARG and b"ascending" in lib.orbfe_last_error()
    assert add(7, [2, 2]) == L.ORBFE_ERR_ARG
    assert add(7, [1, 100]) == L.ORBFE_ERR_ARG and b"n_words" in lib.orbfe_last_error()
    assert add(5, [4]) == L.ORBFE_ERR_STATE  # already stored
    assert add(7, list(range(9))) == L.ORBFE_ERR_CAPACITY  # max_words = 8
    assert len(db) == 2
    assert add(7, list(range(8))) == L.ORBFE_OK
    assert add(8, [1]) == L.ORBFE_ERR_CAPACITY  # max_keyframes = 3
    assert lib.orbfe_kfdb_erase(db._h, 6) == L.ORBFE_ERR_STATE
    db.erase(5)
    assert len(db) == 2
    assert add(8, [1]) == L.ORBFE_OK and len(db) == 3
    ids = np.arange(11, dtype=np.int64)
    assert lib.orbfe_kfdb_set_covisible(db._h, 8, L.ptr(ids), 11) == L.ORBFE_ERR_ARG
    assert lib.orbfe_kfdb_set_covisible(db._h, 8, L.ptr(ids), 10) == L.ORBFE_OK
    assert lib.orbfe_kfdb_set_covisible(db._h, 5, L.ptr(ids), 1) == L.ORBFE_ERR_STATE  # erased
    db.clear()
    assert len(db) == 0
    assert add(5, [1]) == L.ORBFE_OK and len(db) == 1
    # positions are renumbered when the add counter passes 2 * max_keyframes: many cycles are fine
    for i in range(20):
        db.erase(5)
        assert add(5, [1]) == L.ORBFE_OK
    assert len(db) == 1
    # queries need the device; their arguments are checked first
    bow = BowVector(np.array([1, 2], np.uint32), np.array([0.5, 0.5]))
    with pytest.raises(L.OrbfeError) as e:
        db.DetectRelocalizationCandidates(bow)
    assert e.value.status == L.ORBFE_ERR_STATE
    with pytest.raises(L.OrbfeError) as e:
        db.DetectLoopCandidates(bow, 0.1, [5])
    assert e.value.status == L.ORBFE_ERR_STATE
    with pytest.raises(L.OrbfeError) as e:
        db.DetectRelocalizationCandidates(BowVector(np.array([2, 1], np.uint32), np.array([0.5, 0.5])))
    assert e.value.status == L.ORBFE_ERR_ARG
    with pytest.raises(L.OrbfeError) as e:
        db.query(2, bow)
    assert e.value.status == L.ORBFE_ERR_ARG
    one = np.zeros(1, np.int64)
    assert lib.orbfe_kfdb_add_batch_device(db._h, 1, L.ptr(one), c_void_p(16), c_void_p(16), c_void_p(16),
                                           8, None) == L.ORBFE_ERR_STATE
    n = c_int()
    assert lib.orbfe_kfdb_size(None, byref(n)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_kfdb_destroy(None) == L.ORBFE_OK


def test_create_rejects_non_l1_vocabulary_and_bad_bounds():
    from orb_slam2_2021_amd import _lib as L
    from orb_slam2_2021_amd import synthetic as S
    from orb_slam2_2021_amd.vocabulary import ORBVocabulary
    lib = L.lib()
    h = c_void_p()
    for scoring in (1, 2, 3, 4, 5):
        tree = S.Vocabulary.synthetic_orbvoc(k=4, levels=2, scoring=scoring)
        voc = ORBVocabulary.from_tree(tree, device=-1)
        assert lib.orbfe_kfdb_create(voc._h, 8, 8, -1, byref(h)) == L.ORBFE_ERR_ARG
        assert b"L1" in lib.orbfe_last_error()
    voc = ORBVocabulary.from_tree(S.Vocabulary.synthetic_orbvoc(k=4, levels=2), device=-1)
    assert lib.orbfe_kfdb_create(None, 8, 8, -1, byref(h)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_kfdb_create(voc._h, 0, 8, -1, byref(h)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_kfdb_create(voc._h, 16385, 8, -1, byref(h)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_kfdb_create(voc._h, 8, 8193, -1, byref(h)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_kfdb_create(voc._h, 8, 8, -1, byref(h)) == L.ORBFE_OK
    assert lib.orbfe_kfdb_destroy(h) == L.ORBFE_OK
