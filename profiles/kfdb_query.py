"""Relocalisation query time of the resident KeyFrameDatabase (include/orbfe_kfdb.h) on one GPU.

Fills the database with 1,000 and 10,000 keyframes of about 1,000 words each over the
ORBvoc-shaped vocabulary (10^6 words), then times DetectRelocalizationCandidates for query vectors
that are noisy copies of stored keyframes. Prints one JSON line:
  us_per_query      host wall time of the whole call (upload, two kernels, result copy, one
                    synchronise): median, p10, p90 over --repeats calls after --warmup calls
  kernels_us        per-kernel device time from the library's kernel timer, taken in a separate
                    pass (the timer adds host work per launch)
  sweep_bytes       forward-index bytes one query has to read: 4 B per stored word, 8 B per common
                    word (its weight); sweep_gbps = that over k_kfdb_sweep's time, against the
                    6.3 TB/s an MI355X streams from HBM (8 TB/s spec)

    python profiles/kfdb_query.py [--sizes 1000,10000] [--repeats 300] [--warmup 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orb_slam2_2021_amd import KeyFrameDatabase  # noqa: E402
from orb_slam2_2021_amd import _lib as L  # noqa: E402
from orb_slam2_2021_amd import synthetic as S  # noqa: E402
from orb_slam2_2021_amd.vocabulary import BowVector, ORBVocabulary  # noqa: E402

HBM_ACHIEVABLE_GBPS = 6300.0


def bow(rng, words):
    words = np.unique(words).astype(np.uint32)
    w = rng.uniform(0.5, 10.0, len(words))
    return BowVector(words, w / w.sum())


def run(voc, n_kf, words_per_kf, repeats, warmup, rng):
    db = KeyFrameDatabase(voc, max_keyframes=n_kf, max_words=words_per_kf + 64)
    # the places' words come from a 20,000-word part of the vocabulary: two keyframes share ~50
    scene = rng.choice(voc.n_words, 20000, replace=False)
    stored = []
    total_words = 0
    for i in range(n_kf):
        v = bow(rng, rng.choice(scene, words_per_kf, replace=False))
        db.add(i, v)
        stored.append(v.words)
        total_words += len(v.words)
        db.set_covisible(i, [j for j in range(i - 5, i + 6) if j != i and 0 <= j < n_kf][:10])
    queries = []
    for k in range(16):  # a revisit: 70 % of a stored keyframe's words, the rest new
        src = stored[int(rng.integers(n_kf))]
        keep = rng.choice(src, int(0.7 * len(src)), replace=False)
        queries.append(bow(rng, np.concatenate([keep, rng.choice(scene, words_per_kf - len(keep))])))
    common = 0
    for k in range(warmup):
        cand, sh = db.DetectRelocalizationCandidates(queries[k % 16])
    t = np.zeros(repeats)
    for k in range(repeats):
        t0 = time.perf_counter()
        cand, sh = db.DetectRelocalizationCandidates(queries[k % 16])
        t[k] = time.perf_counter() - t0
        common += int(sh.common_words.sum())
    L.ktimer_select(["k_kfdb_sweep", "k_kfdb_finish"])
    L.ktimer_reset()
    n_timed = min(repeats, 64)
    for k in range(n_timed):
        db.DetectRelocalizationCandidates(queries[k % 16])
    kt = {name: 1e3 * ms / launches for name, (ms, launches) in L.ktimer_read().items()}
    L.ktimer_select(None)
    L.ktimer_reset()
    sweep_bytes = 4 * total_words + 8 * common // repeats
    sweep_us = kt.get("k_kfdb_sweep", float("nan"))
    out = {"keyframes": n_kf, "words_per_kf": total_words / max(n_kf, 1),
           "sharing": int(len(sh.kf_ids)), "scored": int(sh.scored.sum()), "candidates": int(len(cand)),
           "us_per_query": {"median": 1e6 * float(np.median(t)), "p10": 1e6 * float(np.percentile(t, 10)),
                            "p90": 1e6 * float(np.percentile(t, 90))},
           "kernels_us": kt, "sweep_bytes": int(sweep_bytes),
           "sweep_gbps": sweep_bytes / (sweep_us * 1e-6) / 1e9,
           "sweep_share_of_hbm": sweep_bytes / (sweep_us * 1e-6) / 1e9 / HBM_ACHIEVABLE_GBPS}
    db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000")
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    rng = np.random.default_rng(2021)
    voc = ORBVocabulary.from_tree(S.Vocabulary.synthetic_orbvoc())
    rows = [run(voc, int(n), a.words, a.repeats, a.warmup, rng) for n in a.sizes.split(",")]
    print(json.dumps({"profile": "kfdb_query", "mode": "reloc", "gpus": 1,
                      "timer_overhead_us": L.ktimer_calibrate(0), "sizes": rows}))


if __name__ == "__main__":
    main()
