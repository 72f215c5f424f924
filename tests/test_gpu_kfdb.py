"""GPU parity of the resident KeyFrameDatabase (k_kfdb_sweep + k_kfdb_finish + k_kfdb_add,
liborbfe.so) against tests/kfdb_ref.py, the reference's KeyFrameDatabase.cc / L1Scoring::score
restated with its own containers. Everything is exact: the sharing list (ids in discovery order,
common-word counts, scored flags, float scores bit-equal, max / min common words) and the
candidate list, for DetectRelocalizationCandidates and DetectLoopCandidates.

Shapes: 0 / 1 / 2 / 64 / 65 / 300 keyframes (wave and workgroup boundaries of the sweep, more
than one pass of the finish workgroup's 64-entry sort floor), BowVectors of 0 / 1 / 63 / 64 / 65 /
~1000 words (the sweep's 64-word chunks), a 100-word vocabulary for dense sharing and an
ORBvoc-shaped one (10^6 words, levelsup 4).

Past one key per finish thread: stores of 1,023 .. 16,384 keyframes whose sharing list is the whole
store (big_store below), so k_kfdb_finish's strided compare-exchange, its candidate emission past
the first 1,024-entry chunk and the dynamic LDS above 64 KiB all run."""
import numpy as np
import pytest

from orb_slam2_2021_amd import KeyFrameDatabase
from orb_slam2_2021_amd import synthetic as S
from orb_slam2_2021_amd.keyframe_database import LOOP, RELOC
from orb_slam2_2021_amd.vocabulary import BowVector, ORBVocabulary

from kfdb_ref import ORDER_WEIGHTS, ORDER_WORDS, RefKeyFrameDatabase

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small_voc(require_gpu):
    tree = S.Vocabulary.synthetic(k=10, levels=2)
    return tree, ORBVocabulary.from_tree(tree)


@pytest.fixture(scope="module")
def orbvoc(require_gpu):
    tree = S.Vocabulary.synthetic_orbvoc()
    return tree, ORBVocabulary.from_tree(tree)


def bow_of(words, weights):
    return BowVector(np.asarray(words, np.uint32), np.asarray(weights, np.float64))


class Pair:
    """The product and the restated reference, driven together."""

    def __init__(self, voc, max_keyframes=512, max_words=2048):
        self.gpu = KeyFrameDatabase(voc, max_keyframes=max_keyframes, max_words=max_words)
        self.ref = RefKeyFrameDatabase(voc.n_words)

    def add(self, kf_id, bow):
        self.gpu.add(kf_id, bow)
        self.ref.add(kf_id, bow.words.tolist(), bow.weights.tolist())

    def erase(self, kf_id):
        self.gpu.erase(kf_id)
        self.ref.erase(kf_id)

    def set_covisible(self, kf_id, ids):
        self.gpu.set_covisible(kf_id, ids)
        self.ref.set_covisible(kf_id, ids)

    def check(self, mode, bow, min_score=0.0, connected=()):
        assert len(self.gpu) == len(self.ref)
        got = self.gpu.query(mode, bow, min_score, connected)
        if mode == RELOC:
            want = self.ref.DetectRelocalizationCandidates(bow.words.tolist(), bow.weights.tolist())
        else:
            want = self.ref.DetectLoopCandidates(bow.words.tolist(), bow.weights.tolist(), min_score, connected)
        same(got, want)
        return want


def same(got, want):
    cand, sh = got
    rcand, rsh = want
    assert sh.kf_ids.tolist() == rsh.kf_ids, "sharing list (discovery order)"
    assert sh.common_words.tolist() == rsh.common_words
    assert (sh.max_common, sh.min_common) == (rsh.max_common, rsh.min_common)
    assert sh.scored.tolist() == rsh.scored
    want_scores = np.array(rsh.scores, np.float32)
    assert np.array_equal(sh.scores.view(np.uint32), want_scores.view(np.uint32)), "scores differ in bits"
    assert cand.tolist() == rcand, "candidate list"


def random_descriptors(rng, tree, n):
    """Half near word centroids, half random (as tests/test_gpu_vocab.py)."""
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    leaves = np.nonzero(tree.is_leaf)[0]
    near = tree.descriptors[rng.choice(leaves, n // 2)].copy()
    near ^= (rng.integers(0, 256, near.shape, dtype=np.uint8) & rng.integers(0, 256, near.shape, dtype=np.uint8)
             & rng.integers(0, 256, near.shape, dtype=np.uint8))
    d[: n // 2] = near
    return d


def random_covisibility(rng, pair, ids):
    for i in ids:
        k = int(rng.integers(0, 11))
        pool = [j for j in ids if j != i] + [10 ** 6 + 1, 10 ** 6 + 2]  # two ids that are not stored
        pair.set_covisible(i, rng.choice(pool, min(k, len(pool)), replace=False).tolist())


def median_scored(want):
    sc = sorted(float(s) for s, f in zip(want[1].scores, want[1].scored) if f)
    return sc[len(sc) // 2] if sc else 0.0


@pytest.mark.parametrize("n_kf", [0, 1, 2, 64, 65, 300])
def test_keyframe_counts(small_voc, n_kf):
    """Descriptor sets of 0 / 1 / 80 / 2000 over the 100-word tree; ids added out of order."""
    tree, voc = small_voc
    rng = np.random.default_rng(1000 + n_kf)
    pair = Pair(voc, max_keyframes=max(n_kf, 1), max_words=100)
    ids = rng.permutation(n_kf * 3)[:n_kf].tolist()
    sizes = [0, 1, 80, 2000]
    for k, i in enumerate(ids):
        n = sizes[k % 4] if k < 8 else int(rng.choice([20, 80, 80, 200]))
        pair.add(i, voc.transform(random_descriptors(rng, tree, n), 1)[0])
    random_covisibility(rng, pair, ids)
    for n in (80, 2000, 1, 0):
        q = voc.transform(random_descriptors(rng, tree, n), 1)[0]
        want = pair.check(RELOC, q)
        if n_kf >= 64 and n >= 80:  # not a vacuous case
            assert len(want[1].kf_ids) >= n_kf // 2 and len(want[0]) >= 1
        want = pair.check(LOOP, q, 0.0)
        connected = ids[: n_kf // 4] + [10 ** 6 + 1]
        pair.check(LOOP, q, median_scored(want), connected)


def test_words_per_keyframe_orbvoc(orbvoc):
    """BowVectors of 0, 1, 63, 64, 65 and ~1000+ words over the ORBvoc-shaped tree, levelsup 4."""
    tree, voc = orbvoc
    rng = np.random.default_rng(7)
    pool = random_descriptors(rng, tree, 2600)  # keyframes draw 2000 of these: ~77 % overlap
    pair = Pair(voc, max_keyframes=64, max_words=2048)
    full = voc.transform(pool[:2000], 4)[0]
    assert len(full.words) >= 1000
    mid = voc.transform(pool[1000:1080], 4)[0]
    assert len(mid.words) >= 65
    vecs = [bow_of([], []), bow_of(full.words[:1], full.weights[:1]), bow_of(mid.words[:63], mid.weights[:63]),
            bow_of(mid.words[:64], mid.weights[:64]), bow_of(mid.words[:65], mid.weights[:65]), full]
    for k in range(24):
        vecs.append(voc.transform(pool[rng.choice(2600, 2000, replace=False)], 4)[0])
    ids = list(range(100, 100 + len(vecs)))
    for i, v in zip(ids, vecs):
        pair.add(i, v)
    random_covisibility(rng, pair, ids)
    for sel in (rng.choice(2600, 2000, replace=False), rng.choice(2600, 700, replace=False), slice(1000, 1080)):
        q = voc.transform(pool[sel], 4)[0]
        want = pair.check(RELOC, q)
        assert len(want[1].kf_ids) >= 20
        pair.check(LOOP, q, median_scored(want), ids[6:9])
    want = pair.check(RELOC, full)  # the query is a stored keyframe: it has the top score
    assert want[1].kf_ids[int(np.argmax(want[1].scores))] == 105


def test_no_overlap_and_self_query(small_voc):
    _, voc = small_voc
    pair = Pair(voc, 8, 100)
    pair.add(1, bow_of(range(0, 50), [0.02] * 50))
    pair.add(2, bow_of(range(10, 40), [0.03] * 30))
    for mode in (RELOC, LOOP):
        want = pair.check(mode, bow_of(range(50, 100), [0.02] * 50))
        assert want[0] == [] and want[1].kf_ids == []
        want = pair.check(mode, bow_of(range(0, 50), [0.02] * 50))
        assert want[0] == [1] and want[1].scores[0] == np.float32(1.0)


def test_summation_order_decides_the_float(small_voc):
    """The five-word vector of test_kfdb_ref: summed left to right the score is 0.5f, in any
    other order 0.5f + 2^-24."""
    _, voc = small_voc
    pair = Pair(voc, 4, 100)
    v = bow_of(ORDER_WORDS, ORDER_WEIGHTS)
    pair.add(0, v)
    want = pair.check(RELOC, v)
    assert want[1].scores == [np.float32(0.5)]
    pair.check(LOOP, v, 0.25)


def test_erase_and_readd_moves_the_keyframe(small_voc):
    _, voc = small_voc
    pair = Pair(voc, 4, 100)  # a full store: the re-added keyframe takes the freed slot
    for kf_id, words in [(7, [5, 6]), (3, [2, 6]), (9, [2, 5]), (1, [6])]:
        pair.add(kf_id, bow_of(words, [0.5] * len(words)))
    q = bow_of([2, 5, 6], [0.25, 0.25, 0.5])
    assert pair.check(RELOC, q)[1].kf_ids == [3, 9, 7, 1]
    pair.erase(3)
    assert pair.check(RELOC, q)[1].kf_ids == [9, 7, 1]
    pair.add(3, bow_of([2, 6], [0.5, 0.5]))
    assert pair.check(RELOC, q)[1].kf_ids == [9, 3, 7, 1]
    for _ in range(12):  # past 2 * max_keyframes adds: the order positions are renumbered
        pair.erase(9)
        pair.add(9, bow_of([2, 5], [0.5, 0.5]))
    assert pair.check(LOOP, q, 0.0)[1].kf_ids == [3, 9, 7, 1]
    pair.gpu.clear()
    pair.ref.clear()
    assert pair.check(RELOC, q)[1].kf_ids == []
    pair.add(5, bow_of([6], [1.0]))
    assert pair.check(RELOC, q)[0] == [5]


def test_stale_reloc_score(small_voc):
    """Two relocalisation queries in a row: keyframe 1 is scored by the first and only shares a
    word in the second, where it still adds its old mRelocScore (:278-281)."""
    _, voc = small_voc
    pair = Pair(voc, 8, 100)
    pair.add(0, bow_of(range(0, 10), [0.1] * 10))
    pair.add(1, bow_of(range(10, 20), [0.1] * 10))
    pair.add(2, bow_of([0, 10], [0.5, 0.5]))
    pair.add(3, bow_of(range(0, 10), [0.07] * 10))
    pair.set_covisible(0, [1])
    pair.set_covisible(1, [0, 99])
    pair.set_covisible(3, [2, 1, 0])
    want = pair.check(RELOC, bow_of(range(10, 20), [0.1] * 10))
    assert want[1].kf_ids == [1, 2] and want[1].scored == [True, False] and want[0] == [1]
    want = pair.check(RELOC, bow_of(range(0, 11), [0.09] * 10 + [0.1]))
    assert want[1].kf_ids == [0, 2, 3, 1] and want[1].scored == [True, False, True, False]
    assert pair.ref.kfs[1].mRelocScore > pair.ref.kfs[0].mRelocScore  # the stale score is the best
    assert want[0] == [1]


def test_loop_mode(small_voc):
    """A connected set, a min_score that drops some scored keyframes, and a dropped keyframe that
    still contributes to a neighbour's accumulated score."""
    _, voc = small_voc
    pair = Pair(voc, 8, 100)
    w = {0: 0.25, 1: 0.0625, 2: 0.25, 3: 0.125}
    for kf_id, words in [(0, range(0, 10)), (1, range(0, 9)), (2, range(0, 10)), (3, range(0, 9)), (4, [30])]:
        pair.add(kf_id, bow_of(words, [w.get(kf_id, 0.25)] * len(words)))
    pair.set_covisible(3, [1, 2, 0])
    pair.set_covisible(1, [3])
    q = bow_of(range(0, 10), [0.25] * 10)
    want = pair.check(LOOP, q, 1.0, [2, 77])
    assert want[1].kf_ids == [0, 1, 3] and want[0] == [0]
    assert want[1].scores[1] < 1.0 <= want[1].scores[2]  # 1 is dropped, 3 is kept and adds 1's score
    assert pair.check(LOOP, q, 1.0)[0] == [2]
    assert pair.check(LOOP, q, 3.0)[0] == []
    want = pair.check(LOOP, q, 0.0, [0, 1, 2, 3])
    assert want[1].kf_ids == [] and want[0] == []


def test_duplicate_best_is_returned_once(small_voc):
    _, voc = small_voc
    pair = Pair(voc, 8, 100)
    pair.add(0, bow_of(range(0, 10), [0.25] * 10))
    pair.add(1, bow_of(range(0, 10), [0.125] * 10))
    pair.add(2, bow_of(range(0, 9), [0.125] * 9))
    pair.set_covisible(1, [0])
    pair.set_covisible(2, [0])
    want = pair.check(RELOC, bow_of(range(0, 10), [0.25] * 10))
    assert want[1].scored == [True, True, True] and want[0] == [0]


def test_device_add_and_device_query(small_voc):
    """add_batch_device fed straight from transform_batch_device for 8 images answers like host
    adds of the same vectors; a query vector may stay on the device too."""
    import torch
    tree, voc = small_voc
    rng = np.random.default_rng(8)
    n_img, cap = 8, 300
    counts = np.array([0, 1, cap, 80, 200, 37, 64, 129], np.int32)
    desc = np.stack([random_descriptors(rng, tree, cap) for _ in range(n_img)])
    dev = torch.device("cuda", 0)
    dd, dc = torch.from_numpy(desc).to(dev), torch.from_numpy(counts).to(dev)
    ids_t = torch.empty(n_img * cap, dtype=torch.int32, device=dev)
    offs = torch.empty(n_img * (cap + 1), dtype=torch.int32, device=dev)
    idx = torch.empty(n_img * cap, dtype=torch.int32, device=dev)
    nn = torch.zeros(n_img, dtype=torch.int32, device=dev)
    bw = torch.empty(n_img * cap, dtype=torch.int32, device=dev)
    bwt = torch.empty(n_img * cap, dtype=torch.float64, device=dev)
    bn = torch.zeros(n_img, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()  # the transform runs here; the database orders itself behind it
    stream = side.cuda_stream
    voc.transform_batch_device(n_img, dd.data_ptr(), cap * 32, dc.data_ptr(), 1, ids_t.data_ptr(),
                               offs.data_ptr(), idx.data_ptr(), nn.data_ptr(), cap, stream=stream,
                               d_bow_words=bw.data_ptr(), d_bow_weights=bwt.data_ptr(), d_bow_n=bn.data_ptr())
    kf_ids = [40, 3, 17, 5, 99, 0, 63, 12]
    on_dev = KeyFrameDatabase(voc, max_keyframes=8, max_words=100)
    on_dev.add_batch_device(kf_ids, bw.data_ptr(), bwt.data_ptr(), bn.data_ptr(), cap, stream=stream)
    assert len(on_dev) == 8
    BW, BT, BN = bw.cpu().numpy().view(np.uint32), bwt.cpu().numpy(), bn.cpu().numpy()
    pair = Pair(voc, 8, 100)
    for i, kf_id in enumerate(kf_ids):
        pair.add(kf_id, bow_of(BW[i * cap:i * cap + BN[i]], BT[i * cap:i * cap + BN[i]]))
    cov = {40: [3, 17], 5: [99, 12, 40], 63: [0]}
    for k, v in cov.items():
        on_dev.set_covisible(k, v)
        pair.set_covisible(k, v)
    for n in (150, 30):
        q = voc.transform(random_descriptors(rng, tree, n), 1)[0]
        want = pair.check(RELOC, q)
        same(on_dev.query(RELOC, q), want)
        min_score = median_scored(want)
        want = pair.check(LOOP, q, min_score, [17])
        same(on_dev.query(LOOP, q, min_score, [17]), want)
    # image 4's BowVector as a device-resident query, its count read on the device
    i = 4
    q = bow_of(BW[i * cap:i * cap + BN[i]], BT[i * cap:i * cap + BN[i]])
    want = pair.check(RELOC, q)
    got = on_dev.query_device(RELOC, bw.data_ptr() + 4 * i * cap, bwt.data_ptr() + 8 * i * cap, cap,
                              d_n=bn.data_ptr() + 4 * i, stream=stream)
    same(got, want)
    # a store too small for the batch's BowVectors refuses all of it
    tight = KeyFrameDatabase(voc, max_keyframes=8, max_words=int(BN.max()) - 1)
    from orb_slam2_2021_amd import OrbfeError
    with pytest.raises(OrbfeError):
        tight.add_batch_device(kf_ids, bw.data_ptr(), bwt.data_ptr(), bn.data_ptr(), cap)
    assert len(tight) == 0
    assert tight.query(RELOC, q)[1].kf_ids.tolist() == []


def test_back_to_back_queries(small_voc):
    """Queries on one handle with nothing in between: each returns its own result."""
    tree, voc = small_voc
    rng = np.random.default_rng(21)
    pair = Pair(voc, 128, 100)
    ids = list(range(100))
    for i in ids:
        pair.add(i, voc.transform(random_descriptors(rng, tree, 60), 1)[0])
    random_covisibility(rng, pair, ids)
    qs = [voc.transform(random_descriptors(rng, tree, n), 1)[0] for n in (60, 25, 60, 8)]
    got = [pair.gpu.query(RELOC, q) for q in qs] + [pair.gpu.query(LOOP, q, 0.05, ids[:7]) for q in qs]
    want = [pair.ref.DetectRelocalizationCandidates(q.words.tolist(), q.weights.tolist()) for q in qs]
    want += [pair.ref.DetectLoopCandidates(q.words.tolist(), q.weights.tolist(), 0.05, ids[:7]) for q in qs]
    for g, w in zip(got, want):
        same(g, w)
    assert len({tuple(w[1].kf_ids) for w in want}) > 1


# ---- stores past one sort key per finish thread ---------------------------------------------------
BIG_SIZES = [1023, 1024, 1025, 2049, 8192, 8193, 16384]
BIG_W = 8                       # max_words of the big stores
COMMON_WORD = 99                # in every keyframe and in the query: the sharing list is the store
Q_WORDS = [7, 23, 41, 58, 76, COMMON_WORD]
Q_WEIGHTS = [0.125, 0.25, 0.125, 0.125, 0.125, 0.25]  # exact in binary, sum 1: a clone scores 1.0f


def big_store(n_kf, seed):
    """Hand-built BowVectors of 1-6 words for `n_kf` keyframes over the 100-word vocabulary.

    A sixth are clones of the query (score exactly 1.0f each) and a sixth near-clones, the query
    without its smallest word (score exactly 0.875f; their first common word is the query's
    second, so they sit behind every keyframe holding word 7 in the list). The others hold
    COMMON_WORD and 0-5 seeded words, each of the query's own words with probability 0.7 and
    otherwise any word below 99, with weights in [1/128, 3/128]: their score is
    sum(min(vi, wi)) <= 6 * 3/128 < 0.15. The smallest common word -- the high half of the finish
    kernel's sort key -- so takes the values 7, 23, 41, 58, 76 and 99, each shared by hundreds of
    keyframes whose order then rests on the add sequence alone. Returns (ids, words[n, BIG_W]
    uint32, weights[n, BIG_W] float64, counts int32, mask of clones and near-clones, mask of
    clones); ids are a seeded permutation, so id order is not add order."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(3 * n_kf)[:n_kf].astype(np.int64)
    words = np.zeros((n_kf, BIG_W), np.uint32)
    weights = np.zeros((n_kf, BIG_W), np.float64)
    counts = np.zeros(n_kf, np.int32)
    kind = rng.random(n_kf)
    clone, full = kind < 1.0 / 3.0, kind < 1.0 / 6.0
    for i in range(n_kf):
        if full[i]:
            w, x = Q_WORDS, Q_WEIGHTS
        elif clone[i]:
            w, x = Q_WORDS[1:], Q_WEIGHTS[1:]
        else:
            k = int(rng.integers(0, 6))
            pick = set()
            while len(pick) < k:
                pick.add(int(rng.choice(Q_WORDS[:5])) if rng.random() < 0.7 else int(rng.integers(0, COMMON_WORD)))
            w = sorted(pick) + [COMMON_WORD]
            x = (rng.integers(1, 4, len(w)) / 128.0).tolist()
        counts[i] = len(w)
        words[i, :len(w)] = w
        weights[i, :len(w)] = x
    return ids, words, weights, counts, clone, full


def big_covisibility(rng, ids, scored, clone, full, n_set=300):
    """Neighbour lists for `n_set` keyframes, kept so that no accumulated score passes 1.15 (every
    clone and near-clone then clears 0.75 * bestAccScore < 0.8625, and the candidate list is long):
      - a clone or near-clone entry gets up to 3 unscored neighbours and at most one scored
        non-clone (< 0.15);
      - a scored non-clone entry gets one of 8 hub clones first (its pBestKF: several entries name
        the same hub, which is also a candidate by itself -- the deduplication) and unscored ones.
    Neighbours are drawn from the whole store, so their list indices lie on either side of every
    1,024 boundary. Returns {id: [neighbour ids]}."""
    idx = np.arange(len(ids))
    unscored, low = idx[~scored], idx[scored & ~clone]
    hubs = rng.choice(idx[full], min(8, int(full.sum())), replace=False)
    cov = {}
    for i in rng.choice(idx[scored], min(n_set, int(scored.sum())), replace=False):
        nb = rng.choice(unscored, min(int(rng.integers(0, 4)), len(unscored)), replace=False).tolist()
        if clone[i]:
            if len(low) and rng.random() < 0.5:
                nb.insert(int(rng.integers(0, len(nb) + 1)), int(rng.choice(low)))
        else:
            nb.insert(0, int(rng.choice(hubs)))
        nb = [j for j in nb if j != i] + ([10 ** 6 + 1] if rng.random() < 0.2 else [])  # one id not stored
        cov[int(ids[i])] = [int(ids[j]) if j < len(ids) else int(j) for j in nb]
    return cov


class BigPair(Pair):
    """A Pair whose product side is filled by add_batch_device from hand-built device arrays."""

    def __init__(self, voc, n_kf):
        super().__init__(voc, max_keyframes=n_kf, max_words=BIG_W)

    def add_batch(self, ids, words, weights, counts, launches=1):
        import torch
        dev = torch.device("cuda", 0)
        for part in np.array_split(np.arange(len(ids)), launches):
            if len(part) == 0:
                continue
            dw = torch.from_numpy(np.ascontiguousarray(words[part]).view(np.int32)).to(dev)
            dx = torch.from_numpy(np.ascontiguousarray(weights[part])).to(dev)
            dn = torch.from_numpy(np.ascontiguousarray(counts[part])).to(dev)
            torch.cuda.synchronize()
            self.gpu.add_batch_device(ids[part], dw.data_ptr(), dx.data_ptr(), dn.data_ptr(), BIG_W)
            for i in part:
                self.ref.add(int(ids[i]), words[i, :counts[i]].tolist(), weights[i, :counts[i]].tolist())


def list_index_of_candidates(want):
    where = {k: i for i, k in enumerate(want[1].kf_ids)}
    return [where[c] for c in want[0]]


def big_queries(pair, ids):
    """RELOC, then LOOP at the reference's median score with an excluded set from both halves of
    the slots, then LOOP at 0 (the low scorers stay in lScoreAndMatch: hubs are named twice).
    Returns the RELOC answer of the reference."""
    q = bow_of(Q_WORDS, Q_WEIGHTS)
    reloc = pair.check(RELOC, q)
    n = len(ids)
    excluded = [int(i) for i in ids[:5]] + [int(i) for i in ids[n // 2 - 3:n // 2 + 3]] + [int(i) for i in ids[-5:]]
    excluded = [i for i in excluded if i in pair.ref.kfs] + [10 ** 6 + 7]
    loop = pair.check(LOOP, q, median_scored(reloc), excluded)
    assert not set(excluded) & set(loop[1].kf_ids)
    pair.check(LOOP, q, 0.0, excluded[:3])
    return reloc


@pytest.mark.parametrize("n_kf", BIG_SIZES)
def test_big_store(small_voc, n_kf):
    """The sharing list is the whole store: 1,023 / 1,024 / 1,025 (one key per finish thread, and
    one more), 2,049 (three keys for some threads, a 4,096-key sort), 8,192 / 8,193 (64 KiB of
    dynamic LDS, and the first size above it) and 16,384 (the bound: 128 KiB)."""
    _, voc = small_voc
    ids, words, weights, counts, clone, full = big_store(n_kf, 5000 + n_kf)
    pair = BigPair(voc, n_kf)
    pair.add_batch(ids, words, weights, counts, launches=1 if n_kf != 2049 else 3)
    assert len(pair.gpu) == n_kf
    q = bow_of(Q_WORDS, Q_WEIGHTS)
    dry = pair.ref.DetectLoopCandidates(q.words.tolist(), q.weights.tolist(), 0.0)  # who is scored (no mRelocScore written)
    scored = np.zeros(n_kf, bool)
    at = {int(k): i for i, k in enumerate(ids)}
    for k, f in zip(dry[1].kf_ids, dry[1].scored):
        scored[at[k]] = f
    rng = np.random.default_rng(n_kf)
    cov = big_covisibility(rng, ids, scored, clone, full)
    for k, v in cov.items():
        pair.set_covisible(k, v)
    want = big_queries(pair, ids)
    assert len(want[1].kf_ids) == n_kf                       # every keyframe shares COMMON_WORD
    assert len(set(np.asarray(want[1].common_words))) >= 5   # and the first-word key is tied widely
    where = {k: i for i, k in enumerate(want[1].kf_ids)}
    crossing = sum(1 for k, v in cov.items() for j in v if j in where and where[k] // 1024 != where[j] // 1024)
    at_idx = list_index_of_candidates(want)
    assert len(want[0]) > n_kf // 4
    if n_kf >= 2049:
        assert crossing >= 20                                # neighbours across a 1,024 boundary
    if n_kf >= 2049:  # the emission loop's second chunk runs with s_base carried over from the first
        assert max(at_idx) >= 1024 and min(at_idx) < 1024
    # more candidates than one chunk holds: from 8,192 on. At 2,049 a third of the store are clones
    # and near-clones, about 690 candidates, so only their list indices past 1,024 can be asked for
    if n_kf >= 8192:
        assert len(want[0]) > 1024
    if n_kf != 2049:
        return
    # holes, renumbered order positions (more than 2 * max_keyframes adds in all), hi > live count
    gone = [int(i) for i in ids[::3]]
    for i in gone:
        pair.erase(i)
    back = gone[::2]
    sel = np.array([at[i] for i in back])
    for _ in range(6):  # 2,049 + 7 * 342 adds in all: past 4,098
        pair.add_batch(ids[sel], words[sel], weights[sel], counts[sel])
        for i in back:
            pair.erase(i)
    pair.add_batch(ids[sel], words[sel], weights[sel], counts[sel], launches=2)
    assert n_kf + 7 * len(back) > 2 * n_kf and len(pair.gpu) == n_kf - len(gone) + len(back) < n_kf
    for k, v in list(cov.items())[::2]:
        if k in pair.ref.kfs:
            pair.set_covisible(k, v)
    want = big_queries(pair, ids)
    assert len(want[1].kf_ids) == len(pair.ref) and max(list_index_of_candidates(want)) >= 1024


def test_readded_keyframe_has_a_fresh_reloc_score(small_voc):
    """Keyframe 1 is scored by a RELOC query (mRelocScore = 1.0f), erased and re-added under the
    same id. In the next RELOC query it shares one word (unscored) and is keyframe 0's neighbour:
    the accumulation adds the 0.0f of a new keyframe (orbfe_kfdb.h), not the 1.0f of the old one --
    with the stale score it would be pBestKF and the candidate list would be [1]."""
    _, voc = small_voc
    pair = Pair(voc, 4, 100)
    pair.add(0, bow_of(range(0, 10), [0.1] * 10))
    pair.add(1, bow_of(range(10, 20), [0.1] * 10))
    pair.add(2, bow_of([0, 10], [0.5, 0.5]))
    pair.set_covisible(0, [1])
    want = pair.check(RELOC, bow_of(range(10, 20), [0.1] * 10))
    assert want[1].kf_ids == [1, 2] and want[1].scored == [True, False] and want[0] == [1]
    pair.erase(1)
    pair.add(1, bow_of(range(10, 20), [0.1] * 10))
    want = pair.check(RELOC, bow_of(range(0, 11), [0.09] * 10 + [0.1]))
    assert want[1].kf_ids == [0, 2, 1] and want[1].scored == [True, False, False]
    assert pair.ref.kfs[1].mRelocScore == 0.0
    assert want[0] == [0]


def test_result_capacity_below_the_sharing_list(small_voc):
    """orbfe_kfdb_query with room for fewer entries than the sharing list: ORBFE_ERR_CAPACITY, and
    the next query on the handle answers as usual."""
    from ctypes import byref
    from orb_slam2_2021_amd import _lib as L
    _, voc = small_voc
    pair = Pair(voc, 8, 100)
    for i in range(5):
        pair.add(i, bow_of([3, 10 + i], [0.5, 0.5]))
    q = bow_of([3, 12], [0.5, 0.5])
    words, weights = pair.gpu._vec(q)
    cap = 3
    arrs = [np.zeros(cap, t) for t in (np.int64, np.int32, np.uint8, np.float32, np.int64)]
    r = L.kfdb_result(capacity=cap, kf_ids=L.ptr(arrs[0]), common_words=L.ptr(arrs[1]), scored=L.ptr(arrs[2]),
                      scores=L.ptr(arrs[3]), candidates=L.ptr(arrs[4]))
    kq = L.kfdb_query(mode=RELOC, n=len(words), words=L.ptr(words), weights=L.ptr(weights), on_device=0,
                      min_score=0.0, excluded=L.ptr(np.zeros(0, np.int64)), n_excluded=0)
    assert L.lib().orbfe_kfdb_query(pair.gpu._h, byref(kq), byref(r)) == L.ORBFE_ERR_CAPACITY
    assert all(not a.any() for a in arrs)  # nothing was written past or into the short arrays
    # the reference ran no query meanwhile; the failed one assigned mRelocScore as a full one does
    want = pair.ref.DetectRelocalizationCandidates(q.words.tolist(), q.weights.tolist())
    assert len(want[1].kf_ids) == 5 > cap
    pair.check(RELOC, q)
    pair.check(LOOP, q, 0.0, [1])


@pytest.mark.parametrize("d_count,used", [(9, 4), (4, 4), (2, 2), (-3, 0), (-2 ** 31, 0), (2 ** 31 - 1, 4)])
def test_device_count_is_clamped(small_voc, d_count, used):
    """query_device's count at d_n is clamped to 0..n as k_kfdb_sweep states: the answer is the
    reference's on the first `used` words."""
    import torch
    _, voc = small_voc
    pair = Pair(voc, 8, 100)
    vecs = [([1, 5, 9], [0.3, 0.3, 0.4]), ([5, 9, 20, 30], [0.25] * 4), ([1, 30], [0.5, 0.5]), ([40], [1.0])]
    for i, (w, x) in enumerate(vecs):
        pair.add(10 + i, bow_of(w, x))
    pair.set_covisible(10, [11, 12])
    words = np.array([1, 5, 9, 30, 40, 41], np.int32)   # the bound n = 4 stops before word 40
    weights = np.array([0.2, 0.3, 0.3, 0.2, 0.5, 0.5], np.float64)
    dev = torch.device("cuda", 0)
    dw, dx = torch.from_numpy(words).to(dev), torch.from_numpy(weights).to(dev)
    dn = torch.tensor([d_count], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for mode in (RELOC, LOOP):
        got = pair.gpu.query_device(mode, dw.data_ptr(), dx.data_ptr(), 4, d_n=dn.data_ptr(), connected=[13])
        w, x = words[:used].tolist(), weights[:used].tolist()
        want = (pair.ref.DetectRelocalizationCandidates(w, x) if mode == RELOC
                else pair.ref.DetectLoopCandidates(w, x, 0.0, [13]))
        same(got, want)
        assert (len(want[1].kf_ids) > 0) == (used > 0)
