"""The exact sequence bench.py times (orb_slam2_2021_amd.pipeline.C3Pipeline, config C3):
extract_batch_device on 2B = 64 images [-> ComputeStereoMatches] -> vocabulary
transform_batch_device (ORBvoc-shaped k=10/L=6 tree, levelsup 4, BowVector + FeatureVector) ->
search_for_triangulation_batch_device with device-side counts (kf*_n_dev / fv*_nodes_dev), output
sets in flight -- every image's keypoints, descriptors, BowVector and FeatureVector, mvuRight and
every pair's match12 against the oracle chain (oracle/c3_check.py). Both pairings: "kf" (the
bench default: KeyFrame t vs t+1 of the driving sequence, SURVEY 8(d), LocalMapping.cc:211-272)
and "stereo" (left vs right of one frame)."""
import numpy as np
import pytest

from orb_slam2_2021_amd import ORBextractor, synth_frame, synth_sequence_frame
from orb_slam2_2021_amd import synthetic as S
from orb_slam2_2021_amd.pipeline import build_c3
from orb_slam2_2021_amd.vocabulary import ORBVocabulary
from oracle.c3_check import check_c3
from oracle.orbref import RefVocabulary

pytestmark = pytest.mark.gpu

H, W = 376, 1241


@pytest.fixture(scope="module")
def vocab():
    tree = S.Vocabulary.synthetic_orbvoc()
    ref = RefVocabulary.from_table(tree.k, tree.levels, tree.scoring, tree.weighting, tree.parent,
                                   tree.is_leaf, tree.descriptors, tree.weights)
    return tree, ORBVocabulary.from_tree(tree), ref


def frames(B, base, pairs="stereo"):
    imgs = np.zeros((2 * B, H, W), np.uint8)
    for i in range(B):
        if pairs == "kf":  # consecutive frames of the bench's driving sequence
            imgs[i], imgs[B + i] = synth_sequence_frame(0x0C3, base + i, H, W, right=True)
        else:
            imgs[i], imgs[B + i] = synth_frame(base + i, H, W, right=True)
    return imgs


@pytest.mark.parametrize("pairs,stereo", [("stereo", False), ("stereo", True), ("kf", True), ("kf", False)])
def test_c3_batch32_bit_exact(require_gpu, vocab, pairs, stereo):
    import torch
    tree, voc, ref = vocab
    B = 32
    ext = ORBextractor(2000, 1.2, 8, 20, 7)
    pipe, st = build_c3(ext, tree, voc, B, H, W, 0, stereo=stereo, pairs=pairs)
    batches = [frames(B, 0, pairs), frames(B, 1000, pairs)]
    d = [torch.from_numpy(b).to("cuda") for b in batches]
    # four sub-batches through both output sets; check the last one of each input batch
    for j in range(4):
        pipe.run(d[j % 2].data_ptr())
    out_b = pipe.to_host(pipe.sets[1])  # sub-batch 3: batch 1
    out_a = pipe.to_host(pipe.sets[0])  # sub-batch 2: batch 0
    for imgs, out in ((batches[0], out_a), (batches[1], out_b)):
        r = check_c3(imgs, out, ref, st["u_right"], st["mp_state"], st["scale"], st["sigma2"], st["cam"],
                     st["F12"], st["epipole"], levelsup=4, stereo=stereo, mb=st["mb"], pairs=pairs)
        assert r["all"], r
        assert min(len(k) for k in out["keypoints"]) >= 2000
        assert len(out["nmatches"]) == (31 if pairs == "kf" else 32)
        assert int(np.sum(out["nmatches"])) > len(out["nmatches"]) * (40 if pairs == "kf" else 50)
        assert len(out["bow"]) == (32 if pairs == "kf" else 64)
        assert all(len(b[0]) > 100 for b in out["bow"])
        if pairs == "kf":  # the epipole is the principal point (forward motion)
            assert abs(st["epipole"][0] - st["cam"]["cx"]) < 1e-3 and abs(st["epipole"][1] - st["cam"]["cy"]) < 1e-3


@pytest.mark.parametrize("match_inline,stereo,blur_mode,pairs,stereo_on_match,handles,fast_side",
                         [(False, False, 1, "stereo", True, 2, 0), (True, False, 0, "stereo", True, 2, 0),
                          (False, True, 0, "stereo", False, 2, 0), (False, True, 1, "kf", True, 2, 0),
                          (True, True, 1, "kf", True, 2, 0), (False, True, 1, "kf", False, 2, 0),
                          (False, True, 1, "kf", True, 4, 0), (False, True, 1, "kf", True, 4, 4)])
@pytest.mark.parametrize("native", [True, False])
def test_c3_two_extractors_bit_exact(require_gpu, vocab, match_inline, stereo, blur_mode, pairs, stereo_on_match,
                                     handles, fast_side, native):
    """bench.py's schedules: extractor handles extract consecutive sub-batches on two extraction
    streams (handle k on stream k mod 2; side-stream work on one shared high-priority stream),
    matching on its own stream or inline after each extraction (then two vocabulary transforms run
    concurrently on the one handle: per-stream scratch), 4+ output sets; ComputeStereoMatches on the
    matching stream (with 2 handles the handle's next extraction waits for it; with 4 -- bench.py's
    default -- nothing waits) or right after the extraction. fast_side 4: FAST of levels 0-3 on the
    shared side stream, bench.py's setting (0 keeps the library default, 3). native: each sub-batch
    enqueued by one orbfe_c3_run call (include/orbfe_c3.h), or stage by stage from Python."""
    import torch
    from orb_slam2_2021_amd.pipeline import PipelineStreams
    tree, voc, ref = vocab
    B = 32
    exts = [ORBextractor(2000, 1.2, 8, 20, 7) for _ in range(handles)]
    for e in exts:
        e.debug_set_blur_mode(blur_mode)
        if fast_side > 0:
            e.debug_set_fast_side_levels(fast_side)
    streams = PipelineStreams(0, 2, match_inline=match_inline)
    pipe, st = build_c3(exts, tree, voc, B, H, W, 0, stereo=stereo, depth=4, streams=streams, pairs=pairs,
                        stereo_on_match=stereo_on_match, native=native)
    assert (pipe._c3 is not None) == native
    batches = [frames(B, 0, pairs), frames(B, 1000, pairs), frames(B, 2000, pairs)]
    d = [torch.from_numpy(b).to("cuda") for b in batches]
    nsets = len(pipe.sets)
    for j in range(7):  # sub-batch j: input j % 3, set j % nsets, handle j % handles
        pipe.run(d[j % 3].data_ptr())
    torch.cuda.synchronize()
    for j in (4, 5, 6):
        out = pipe.to_host(pipe.sets[j % nsets])
        r = check_c3(batches[j % 3], out, ref, st["u_right"], st["mp_state"], st["scale"], st["sigma2"],
                     st["cam"], st["F12"], st["epipole"], levelsup=4, stereo=stereo, mb=st["mb"], pairs=pairs)
        assert r["all"], (j, r)
    pipe.close()
    streams.close()


@pytest.mark.parametrize("slots", ["0", "4", "5"])
def test_bench_host_fed_parity(require_gpu, slots):
    """bench.py --feed host: every sub-batch's images copied from pinned host memory into a ring of
    device slots on the copy stream, a slot reused only after the extraction that read it (its
    consumed event). Default ring (2 per handle: 8), one slot per handle (4) and a ring that is not a
    multiple of the handle count (5): the timed line's last sub-batch is bit-exact against the oracle
    chain, and the line reports the ring it used."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--feed", "host", "--input-slots", slots, "--steps", "1",
           "--warmup", "1", "--batches-per-step", "24", "--full", "--no-cpu", "--no-legs", "--event-every", "1000000"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["parity_bit_exact"] is True
    assert line["feed"]["device_slots"] == (8 if slots == "0" else int(slots))
