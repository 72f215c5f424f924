"""Batched OptimizeSim3 time (include/orbfe_optsim3.h) on one GPU, beside the host build of the same
arithmetic on this machine's CPU.

Times orbfe_optsim3_batch for three shapes: 1 problem x 100 correspondences, 5 x 100 (ComputeSim3's
usual handful of loop candidates) and 64 x 1000. The candidates are tests/optsim3_scenes.Problem: half
a pixel of noise, 20 % gross outliers, the start 2 degrees / 5 cm off, the scale fixed. Prints one JSON
line:
  us_per_batch   host wall time of the whole call (staging, one upload, one kernel, one result copy,
                 one synchronise, the copy-out): median, p10, p90 over --repeats calls after --warmup
  kernel_us      k_optsim3's device time per launch from the library's kernel timer, taken in a
                 separate pass (the timer adds host work per launch)
  host_core_us   orbfe_optsim3_core.h compiled for the host (g++ -O2 -ffp-contract=off, one thread,
                 tests/cpp/optsim3_core_main.cpp) over the same problems: time per pass over the batch

    python profiles/optsim3.py [--shapes 1x100,5x100,64x1000] [--repeats 200] [--warmup 20]
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

from orb_slam2_2021_amd import Sim3Optimizer  # noqa: E402
from orb_slam2_2021_amd import _lib as L  # noqa: E402
from optsim3_ref import write_problems  # noqa: E402
from optsim3_scenes import Problem  # noqa: E402


def host_core_us(problems, tmp, passes=20):
    exe = os.path.join(tmp, "optsim3_core_main")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "optsim3_core_main.cpp")], check=True)
    path = os.path.join(tmp, "problems.txt")
    write_problems(path, problems)

    def wall(reps):
        t0 = time.perf_counter()
        subprocess.run([exe, path, str(reps)], check=True, stdout=subprocess.DEVNULL)
        return time.perf_counter() - t0

    wall(1)
    return 1e6 * (wall(1 + passes) - wall(1)) / passes  # parsing and start-up cancel


def run(n_problems, n, repeats, warmup, seed, tmp):
    problems = [Problem(n=n, seed=seed + i, noise=0.5, outliers=0.2, rot_deg=2.0, trans=0.05) for i in range(n_problems)]
    opt = Sim3Optimizer(n_problems, n)
    for _ in range(warmup):
        res = opt.optimize(problems)
    t = np.zeros(repeats)
    for k in range(repeats):
        t0 = time.perf_counter()
        res = opt.optimize(problems)
        t[k] = time.perf_counter() - t0
    L.ktimer_select(["k_optsim3"])
    L.ktimer_reset()
    for _ in range(min(repeats, 64)):
        opt.optimize(problems)
    kt = {name: 1e3 * ms / launches for name, (ms, launches) in L.ktimer_read().items()}
    L.ktimer_select(None)
    L.ktimer_reset()
    opt.close()
    return {"problems": n_problems, "correspondences": n,
            "inliers": [int(r.n_inliers) for r in res][:8],
            "iterations": [[rd.iterations for rd in r.rounds] for r in res][:2],
            "us_per_batch": {"median": 1e6 * float(np.median(t)), "p10": 1e6 * float(np.percentile(t, 10)),
                             "p90": 1e6 * float(np.percentile(t, 90))},
            "kernel_us": kt.get("k_optsim3"), "host_core_us": host_core_us(problems, tmp)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x100,5x100,64x1000")
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        rows = [run(*(int(v) for v in shape.split("x")), a.repeats, a.warmup, 2021 + 100 * k, tmp)
                for k, shape in enumerate(a.shapes.split(","))]
    print(json.dumps({"profile": "optsim3", "gpus": 1, "timer_overhead_us": L.ktimer_calibrate(0), "shapes": rows}))


if __name__ == "__main__":
    main()
