"""LocalBundleAdjustment time (include/orbfe_lba.h) on one GPU, beside the host build of the same
arithmetic on this machine's CPU.

Times orbfe_lba_solve for three local maps, as free / fixed keyframes x points x observations per point:
5/5 x 300 x 4, 20/30 x 2000 x 6 and 64/128 x 8000 x 8 (tests/lba_scenes.make: mixed mono / stereo, 0.3 px of
noise, 5 % of the points with one gross outlier). Prints one JSON line:
  us_per_call    host wall time of the whole call (plan, uploads, every launch and record read-back of
                 the host-side Levenberg loop, the copy-out): median, p10, p90 over --repeats calls
  kernel_us      device time per stage, summed over one call, from the library's kernel timer, taken in
                 a separate pass (the timer adds host work per launch)
  iterations, trials   per round
  host_core_us   orbfe_lba_core.h compiled for the host (g++ -O2 -ffp-contract=off, one thread,
                 tests/cpp/lba_core_main.cpp) over the same problem

    python profiles/lba.py [--shapes 5/5x300x4,20/30x2000x6,64/128x8000x8] [--repeats 20] [--warmup 3]
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

from orb_slam2_2021_amd import LocalBundleAdjuster  # noqa: E402
from orb_slam2_2021_amd import _lib as L  # noqa: E402
from lba_scenes import make  # noqa: E402
from test_lba_ref import write_problems  # noqa: E402

KERNELS = ["k_lba_edge", "k_lba_point", "k_lba_pose", "k_lba_dinv", "k_lba_schur", "k_lba_ldlt", "k_lba_update",
           "k_lba_edge_trial", "k_lba_point_chi", "k_lba_reduce", "k_lba_classify"]


def host_core_us(problem, tmp, passes=3):
    exe = os.path.join(tmp, "lba_core_main")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "lba_core_main.cpp")], check=True)
    path = os.path.join(tmp, "problem.txt")
    write_problems(path, [problem])

    def wall(reps):
        t0 = time.perf_counter()
        subprocess.run([exe, path, str(reps)], check=True, stdout=subprocess.DEVNULL)
        return time.perf_counter() - t0

    wall(1)
    return 1e6 * (wall(1 + passes) - wall(1)) / passes  # parsing and start-up cancel


def run(shape, repeats, warmup, seed, tmp):
    kfs, n_points, obs = shape.split("x")
    n_free, n_fixed = (int(v) for v in kfs.split("/"))
    p = make(seed, n_free, 0, n_fixed, int(n_points), int(obs), noise=0.3, outlier_frac=0.05 / int(obs))
    adj = LocalBundleAdjuster(n_free, p.n_kf, p.n_points, p.n_edges)
    for _ in range(warmup):
        r = adj.solve(p)
    t = np.zeros(repeats)
    for k in range(repeats):
        t0 = time.perf_counter()
        r = adj.solve(p)
        t[k] = time.perf_counter() - t0
    L.ktimer_select(KERNELS)
    L.ktimer_reset()
    calls = min(repeats, 5)
    for _ in range(calls):
        adj.solve(p)
    kt = {name: 1e3 * ms / calls for name, (ms, launches) in L.ktimer_read().items()}
    L.ktimer_select(None)
    L.ktimer_reset()
    adj.close()
    return {"free": n_free, "fixed": n_fixed, "points": p.n_points, "edges": p.n_edges, "n_erase": int(r.n_erase),
            "iterations": [rd.iterations for rd in r.rounds], "trials": [rd.trials for rd in r.rounds],
            "us_per_call": {"median": 1e6 * float(np.median(t)), "p10": 1e6 * float(np.percentile(t, 10)),
                            "p90": 1e6 * float(np.percentile(t, 90))},
            "kernel_us": kt, "host_core_us": host_core_us(p, tmp)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5/5x300x4,20/30x2000x6,64/128x8000x8")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        rows = [run(shape, a.repeats, a.warmup, 2021 + 100 * k, tmp) for k, shape in enumerate(a.shapes.split(","))]
    print(json.dumps({"profile": "lba", "gpus": 1, "timer_overhead_us": L.ktimer_calibrate(0), "shapes": rows}))


if __name__ == "__main__":
    main()
