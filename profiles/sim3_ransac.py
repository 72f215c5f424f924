"""Batched Sim3Solver RANSAC time (include/orbfe_sim3.h) on one GPU.

Times orbfe_sim3_solve_batch for loop-closure-shaped inputs: 5 candidates x 100 correspondences x
300 hypotheses (LoopClosing::ComputeSim3 with five candidates) and 1 x 30 x 300. Prints one JSON line:
  us_per_solve_batch  host wall time of the whole call (staging, one upload, three kernels, one
                      result copy, one synchronise, the copy-out): median, p10, p90 over --repeats
                      calls after --warmup calls
  kernels_us          per-kernel device time from the library's kernel timer, taken in a separate
                      pass (the timer adds host work per launch)

    python profiles/sim3_ransac.py [--shapes 5x100x300,1x30x300] [--repeats 300] [--warmup 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orb_slam2_2021_amd import Sim3Batch, Sim3Solver  # noqa: E402
from orb_slam2_2021_amd import _lib as L  # noqa: E402

KERNELS = ["k_sim3_hypotheses", "k_sim3_inliers", "k_sim3_select"]
K = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)


def make_solver(rng, n, n_hyp):
    """70 % of the correspondences follow one Sim3, the rest are scrambled."""
    ang = rng.uniform(0.1, 0.5)
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    x2 = np.stack([rng.uniform(-4, 4, n), rng.uniform(-1.5, 1.5, n), rng.uniform(5, 14, n)], axis=1)
    x1 = 1.1 * x2 @ R.T + rng.uniform(-0.5, 0.5, 3) + rng.normal(0, 0.002, (n, 3))
    out = rng.choice(n, int(0.3 * n), replace=False)
    x1[out] = x1[rng.permutation(out)] + rng.normal(0, 0.5, (len(out), 3))
    sigma2 = (1.2 ** rng.integers(0, 8, (2, n))) ** 2
    s = Sim3Solver(x1, x2, sigma2[0], sigma2[1], K, K, False)
    # minInliers / n = 0.2 keeps mRansacMaxIts at the 300 cap (LoopClosing's 20 would leave 14
    # iterations at 30 correspondences)
    s.SetRansacParameters(0.99, min(20, n // 5), 300)
    s.set_draws(rng.integers(0, np.array([n, n - 1, n - 2]), (n_hyp, 3)))
    return s


def run(n_solvers, n, n_hyp, repeats, warmup, rng):
    batch = Sim3Batch(n_solvers, n, n_hyp)
    solvers = [make_solver(rng, n, n_hyp) for _ in range(n_solvers)]
    for _ in range(warmup):
        batch.solve(solvers)
    t = np.zeros(repeats)
    for k in range(repeats):
        t0 = time.perf_counter()
        batch.solve(solvers)
        t[k] = time.perf_counter() - t0
    L.ktimer_select(KERNELS)
    L.ktimer_reset()
    for _ in range(min(repeats, 64)):
        batch.solve(solvers)
    kt = {name: 1e3 * ms / launches for name, (ms, launches) in L.ktimer_read().items()}
    L.ktimer_select(None)
    L.ktimer_reset()
    out = {"solvers": n_solvers, "correspondences": n, "hypotheses": n_hyp,
           "evaluated": [int(s.n_evaluated) for s in solvers],
           "accepted": [int(s.found["accepted"]) for s in solvers],
           "us_per_solve_batch": {"median": 1e6 * float(np.median(t)), "p10": 1e6 * float(np.percentile(t, 10)),
                                  "p90": 1e6 * float(np.percentile(t, 90))},
           "kernels_us": kt}
    batch.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5x100x300,1x30x300")
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    rng = np.random.default_rng(2021)
    rows = [run(*(int(v) for v in shape.split("x")), a.repeats, a.warmup, rng) for shape in a.shapes.split(",")]
    print(json.dumps({"profile": "sim3_ransac", "gpus": 1, "timer_overhead_us": L.ktimer_calibrate(0),
                      "shapes": rows}))


if __name__ == "__main__":
    main()
