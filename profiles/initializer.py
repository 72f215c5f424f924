"""Initializer time (include/orbfe_init.h) on one GPU, beside the host build of the same arithmetic on
this machine's CPU.

The workload is the reference's own: 200 iterations over the matches ORBmatcher(0.9, True)
.SearchForInitialization returns on bench.py's synthetic monocular pair (2000 features per frame,
window 100). Prints one JSON line:
  matches        N, the matches of the pair
  us_per_call    host wall time of orbfe_init_solve_batch (staging, the upload, six launches, the
                 copy-out, the host's parallax decision): median, p10, p90 over --repeats calls
  kernel_us      device time per kernel of one call, from the library's kernel timer, taken in a
                 separate pass (the timer adds host work per launch)
  host_core_us   orbfe_init_core.h compiled for the host (g++ -O2 -ffp-contract=off, one thread,
                 tests/cpp/initializer_core_main.cpp) over the same problem
  batch          the same problem 1, 4 and 16 times in one call

    python profiles/initializer.py [--repeats 30] [--warmup 3]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from orb_slam2_2021_amd import Initializer, InitializerBatch, ORBmatcher  # noqa: E402
from orb_slam2_2021_amd import _lib as L  # noqa: E402
from orb_slam2_2021_amd import synthetic as S  # noqa: E402
from initializer_scenes import draws, dump  # noqa: E402

KERNELS = ["k_init_normalize", "k_init_hypotheses", "k_init_score", "k_init_select", "k_init_checkrt",
           "k_init_decide"]


def bench_pair():
    """bench.py's SearchForInitialization case: (keys1, keys2, vMatches12, K)."""
    rng = np.random.default_rng(0x0B0C)
    sc = S.make_keyframe_scene(rng, n_points=1500, n_clutter=500, vocab=S.Vocabulary.synthetic())
    cur = sc.f1
    prev = np.stack([cur.keys_un["x"], cur.keys_un["y"]], 1).astype(np.float32)
    n, m12, _ = ORBmatcher(0.9, True).SearchForInitialization(cur, sc.f2, prev, 100)
    keys2 = np.stack([sc.f2.keys_un["x"], sc.f2.keys_un["y"]], 1).astype(np.float32)
    cam = S.KITTI_CAM
    return prev, keys2, np.asarray(m12, np.int32), (cam["fx"], cam["fy"], cam["cx"], cam["cy"]), int(n)


def host_core_us(problem, tmp, passes=3):
    exe = os.path.join(tmp, "initializer_core_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "hipstub"),
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "initializer_core_main.cpp")], check=True)
    path = os.path.join(tmp, "problem.txt")
    dump(path, [problem])
    out = subprocess.run([exe, path, str(passes)], check=True, capture_output=True, text=True).stdout
    return 1e3 * float(out.split()[1])  # the program times its own passes: parsing and start-up excluded


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=200)
    a = ap.parse_args()
    keys1, keys2, m12, K, n = bench_pair()
    N = int((m12 >= 0).sum())
    d = draws(N, a.iterations, 2021)
    rows = {}
    first = None
    for copies in (1, 4, 16):
        batch = InitializerBatch(copies, max(len(keys1), len(keys2)), max(N, 8), a.iterations)
        inits = []
        for _ in range(copies):
            s = Initializer(keys1, K, 1.0, a.iterations)
            s.set_draws(d)
            inits.append(s.prepare(keys2, m12))
        for _ in range(a.warmup):
            batch.solve(inits)
        t = np.zeros(a.repeats)
        for k in range(a.repeats):
            t0 = time.perf_counter()
            batch.solve(inits)
            t[k] = time.perf_counter() - t0
        row = {"us_per_call": {"median": 1e6 * float(np.median(t)), "p10": 1e6 * float(np.percentile(t, 10)),
                               "p90": 1e6 * float(np.percentile(t, 90))}}
        if copies == 1:
            first = inits[0]
            L.ktimer_select(KERNELS)
            L.ktimer_reset()
            calls = min(a.repeats, 5)
            for _ in range(calls):
                batch.solve(inits)
            row["kernel_us"] = {name: 1e3 * ms / calls for name, (ms, launches) in L.ktimer_read().items()}
            L.ktimer_select(None)
            L.ktimer_reset()
        rows[str(copies)] = row
        batch.close()
    with tempfile.TemporaryDirectory() as tmp:
        cpu = host_core_us((keys1, keys2, m12, K, 1.0, d), tmp)
    print(json.dumps({"profile": "initializer", "gpus": 1, "timer_overhead_us": L.ktimer_calibrate(0),
                      "keys": [len(keys1), len(keys2)], "matches": N, "iterations": a.iterations,
                      "ok": bool(first.result[0]), "model": first.model, "n_good": [int(v) for v in first.n_good],
                      "batch": rows, "host_core_us": cpu,
                      "cpu_over_gpu": cpu / rows["1"]["us_per_call"]["median"]}))


if __name__ == "__main__":
    main()
