"""bench.py's reporting helpers on CPU: the roofline object carries the contract's keys with
consistent arithmetic, the committed PMC summary is found for the benchmark workload, and the
CLI defaults are N=1 with a short run."""
import os
import sys

from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

# level geometry of 1241x376 / 8 levels / 1.2 (w, h, ncells per level; other columns unused here)
GEO = np.array([[1241, 376, 429], [1034, 313, 297], [862, 261, 196], [718, 218, 138],
                [598, 181, 95], [499, 151, 64], [416, 126, 42], [346, 105, 30]])
GEO = np.hstack([GEO, np.zeros((8, 4), np.int64)])


def test_roofline_object():
    counts = np.full(64, 2007, np.int32)
    kt = {"k_fast": (50 * 0.25, 100)}  # 50 steps, 2 launches per step, 0.25 ms per step
    pipe = SimpleNamespace(n_vocab=32, pair_idx=[(i, i + 1) for i in range(31)], n_pairs=31)
    r = bench.roofline(kt, "k_fast", GEO, counts, 13_000 * 64, 64, 50, pipe)  # 50 sub-batches
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["launches_per_subbatch"] == 2
    per_step = r["algorithmic_bytes_per_subbatch"]
    assert abs(r["achieved"] - per_step / 0.25e-3 / 1e9) < 0.05
    assert abs(r["frac"] - r["achieved"] / 8000.0) < 1e-5
    px = sum(int(w) * int(h) for w, h in GEO[:, :2])
    assert per_step == 64 * (px + 4 * int(GEO[:, 2].sum())) + 4 * 13_000 * 64
    # SearchForTriangulation bytes follow the pairing: 31 KeyFrame pairs (t, t+1) of 2007 keypoints
    kt = {"k_sft_nodes": (50 * 0.1, 50)}
    r = bench.roofline(kt, "k_sft_nodes", GEO, counts, 0, 64, 50, pipe)
    assert r["algorithmic_bytes_per_subbatch"] == 31 * (64 * 2 * 2007 + 4 * 2007)
    # every kernel of the C3 step has algorithmic bytes (the dominant one is chosen by device time)
    for k in ("k_copy0", "k_resize_win", "k_fast", "k_octree", "k_blur", "k_describe", "k_stereo_rows",
              "k_stereo_match", "k_stereo_median", "k_vocab_descend", "k_vocab", "k_sft_nodes", "k_sft_finish"):
        r = bench.roofline({k: (50 * 0.1, 50)}, k, GEO, counts, 13_000 * 64, 64, 50, pipe)
        assert r["algorithmic_bytes_per_subbatch"] > 0 and 0 < r["frac"] < 1, k


def test_committed_pmc_traffic_matches_workload():
    a = SimpleNamespace(pairs="kf", stereo=True)  # the bench default
    t, src = bench.pmc_traffic("k_fast", 1241, 376, 32, a)
    assert t is not None and t > 0 and "FETCH_SIZE" in src
    assert bench.pmc_traffic("k_fast", 640, 480, 32, a) == (None, None)  # other workload: not reported
    assert bench.pmc_traffic("k_fast", 1241, 376, 32, SimpleNamespace(pairs="stereo", stereo=False)) == (None, None)
    # the stereo leg's traffic: all three ComputeStereoMatches kernels are in the summary
    assert bench.stereo_traffic(a, 1241, 376, 32) > 0
    # C5: the search's kernels for the 50k-MapPoint map
    assert bench.c5_pmc_traffic(50000) > 0 and bench.c5_pmc_traffic(1000) is None


def test_cli_defaults():
    saved = sys.argv
    sys.argv = ["bench.py"]
    try:
        a = bench.parse()
    finally:
        sys.argv = saved
    assert a.gpus == 1 and 0 < a.steps <= 100 and 0 <= a.warmup <= 20 and a.batch == 32
    assert a.input_batches >= 4 and a.vocab_levels == 6 and a.levelsup == 4
    # two extractor handles, two output sets each
    assert a.extractors == 2 and a.handles_per_stream == 2 and bench.pipe_depth(a) == 8 and not a.stereo_on_extract
    # SURVEY 8(d)'s KeyFrame pairs with the stereo Frame's ComputeStereoMatches
    assert a.pairs == "kf" and a.stereo
    # a step is long enough to be seen (>= 1024 sub-batches of 32 stereo frames)
    assert a.batches_per_step * a.batch >= 32 * 1024


def test_plain_run_is_the_default():
    """--full is off by default, and the measurements beside the headline figure only run with it."""
    assert bench.parse([]).full is False and bench.parse(["--full"]).full is True
    assert bench.parse([]).dump_outputs == "" and bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"


def test_dump_outputs_writes_float_arrays(tmp_path):
    """--dump-outputs: one float32 / float64 .npy per output of a sub-batch, values exact, the same
    files for the same outputs, and a seeded row sample once the whole exceeds the size limit."""
    from orb_slam2_2021_amd import _lib as L
    rng = np.random.default_rng(5)
    n = [3, 0, 5, 2]
    kps = []
    for m in n:
        k = np.zeros(m, L.KEYPOINT_DTYPE)
        k["x"], k["y"], k["octave"] = rng.random(m, np.float32), rng.random(m, np.float32), rng.integers(0, 8, m)
        kps.append(k)
    h = {"keypoints": kps, "descriptors": [rng.integers(0, 256, (m, 32), np.uint8) for m in n],
         "bow": [(np.arange(m, dtype=np.uint32) * 400_000, rng.random(m)) for m in n[:2]],
         "fv": [(np.arange(2, dtype=np.uint32), np.array([0, 1, m], np.int32), np.arange(m, dtype=np.int32))
                for m in n[:2]],
         "match12": [rng.integers(-1, 5, m, np.int32) for m in n[:3]], "nmatches": np.array([1, 0, 2], np.int32),
         "u_right": [rng.random(m, np.float32) for m in n[:2]]}
    bench.dump_outputs(str(tmp_path / "a"), h)
    bench.dump_outputs(str(tmp_path / "b"), h)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "keypoints.npy" in names and "u_right.npy" in names
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and a.tobytes() == b.tobytes(), f
    a = tmp_path / "a"
    assert np.load(a / "keypoint_counts.npy").tolist() == n
    assert np.array_equal(np.load(a / "keypoints.npy")[:, 0], np.concatenate([k["x"] for k in kps]))
    assert np.array_equal(np.load(a / "keypoints.npy")[:, 5], np.concatenate([k["octave"] for k in kps]))
    assert np.array_equal(np.load(a / "descriptors.npy"), np.concatenate(h["descriptors"]))
    assert np.array_equal(np.load(a / "bow_words.npy"), np.concatenate([w for w, _ in h["bow"]]))
    assert np.array_equal(np.load(a / "bow_weights.npy"), np.concatenate([t for _, t in h["bow"]]))
    assert np.array_equal(np.load(a / "match12.npy"), np.concatenate(h["match12"]))
    # over the limit: the large arrays keep a seeded sample of their rows, in order, within the limit
    saved, bench.DUMP_MAX_BYTES = bench.DUMP_MAX_BYTES, 64 << 10
    try:
        big = dict(h, keypoints=[np.zeros(4000, L.KEYPOINT_DTYPE)],
                   descriptors=[rng.integers(0, 256, (4000, 32), np.uint8)])
        bench.dump_outputs(str(tmp_path / "c"), big)
        bench.dump_outputs(str(tmp_path / "d"), big)
        for r in range(2):  # several ranks share the limit
            bench.dump_outputs(str(tmp_path / "e"), big, rank=r, world=2)
    finally:
        bench.DUMP_MAX_BYTES = saved
    c = {f: np.load(tmp_path / "c" / f) for f in names}
    assert sum(v.nbytes for v in c.values()) <= 64 << 10
    assert 0 < len(c["descriptors.npy"]) < 4000 and len(c["descriptors.npy"]) == len(c["keypoints.npy"])
    assert all(c[f].tobytes() == np.load(tmp_path / "d" / f).tobytes() for f in names)
    ranks = sorted(os.listdir(tmp_path / "e"))
    assert ranks == sorted(f"rank{r}_{f}" for r in range(2) for f in names)
    assert sum(np.load(tmp_path / "e" / f).nbytes for f in ranks) <= 64 << 10


def test_hw_queue_setting():
    # several ranks: RCCL's stream gets a hardware queue of its own beside the four pipeline streams
    assert bench.hw_queue_setting(-1, 1) == 0
    assert bench.hw_queue_setting(-1, 2) == bench.HW_QUEUES_MULTI_RANK >= 5
    assert bench.hw_queue_setting(-1, 8) == bench.HW_QUEUES_MULTI_RANK
    assert bench.hw_queue_setting(0, 8) == 0  # the environment's
    assert bench.hw_queue_setting(4, 1) == 4
    assert bench.parse([]).hw_queues == -1 and bench.parse([]).c5_workers >= 1


def test_root_share_schedule():
    """C4's rank-0 share: the model and the slot schedule."""
    import bench
    assert bench.root_share(-1, 1) == 1.0
    assert abs(bench.root_share(-1, 8) - (1 - 7 * bench.ROOT_INGEST_PER_PEER)) < 1e-12
    assert bench.root_share(0.3, 8) == 0.3 and bench.root_share(2.0, 8) == 1.0
    for n, f in [(1024, 0.809), (1024, 1.0), (7, 0.5), (3, 0.97), (100, 0.0)]:
        own = bench.own_slots(n, f)
        assert len(own) == n and sum(own) == int(n * f + 0.5)
        if f > 0:
            assert own[0]  # the first slot runs rank 0's own sub-batch
    # the whole-job loss the share leaves at N = 8 (rank 0 and the peers finish together)
    f = bench.root_share(-1, 8)
    assert (1 - f) / 8 <= 0.05
