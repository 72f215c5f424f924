"""GPU parity of the resident KeyFrameDatabase (k_kfdb_sweep + k_kfdb_finish + k_kfdb_add,
liborbfe.so) against tests/kfdb_ref.py, the reference's KeyFrameDatabase.cc / L1Scoring::score
restated with its own containers. Everything is exact: the sharing list (ids in discovery order,
common-word counts, scored flags, float scores bit-equal, max / min common words) and the
candidate list, for DetectRelocalizationCandidates and DetectLoopCandidates.

Shapes: 0 / 1 / 2 / 64 / 65 / 300 keyframes (wave and workgroup boundaries of the sweep, more
than one pass of the finish workgroup's 64-entry sort floor), BowVectors of 0 / 1 / 63 / 64 / 65 /
~1000 words (the sweep's 64-word chunks), a 100-word vocabulary for dense sharing and an
ORBvoc-shaped one (10^6 words, levelsup 4)."""
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
