"""Batched PnPsolver RANSAC time (include/orbfe_pnp.h) on one GPU.

Times orbfe_pnp_solve_batch for relocalisation-shaped inputs: 5 candidates x 100 correspondences x
300 hypotheses with Tracking::Relocalization's SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), and
1 x 30 x 300. Prints one JSON line:
  us_per_solve_batch  host wall time of the whole call (staging, one upload, six kernels, one result
                      copy, one synchronise, the copy-out): median, p10, p90 over --repeats calls
                      after --warmup calls
  kernels_us          per-kernel device time per launch from the library's kernel timer, taken in a
                      separate pass (the timer adds host work per launch); k_pnp_inliers is launched
                      twice per call (hypotheses, refined poses)

    python profiles/pnp_ransac.py [--shapes 5x100x300,1x30x300] [--repeats 300] [--warmup 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orb_slam2_2021_amd import PnPBatch, PnPsolver  # noqa: E402
from orb_slam2_2021_amd import _lib as L  # noqa: E402

KERNELS = ["k_pnp_hypotheses", "k_pnp_inliers", "k_pnp_records", "k_pnp_refine", "k_pnp_select"]
K = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
RELOC = (0.99, 10, 300, 4, 0.5, 5.991)


def make_solver(rng, n, n_hyp):
    """75 % of the matches project through one pose with half a pixel of noise, the rest are off."""
    ang = rng.uniform(-0.3, 0.3)
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    t = rng.uniform(-1, 1, 3)
    pc = np.stack([rng.uniform(-6, 6, n), rng.uniform(-2, 2, n), rng.uniform(4, 20, n)], axis=1)
    pw = (pc - t) @ R
    uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], axis=1)
    uv += rng.normal(0, 0.5, uv.shape)
    out = rng.choice(n, int(0.25 * n), replace=False)
    uv[out] += rng.uniform(-80, 80, (len(out), 2))
    sigma2 = (1.2 ** rng.integers(0, 8, n)) ** 2
    s = PnPsolver(pw, uv, sigma2, K)
    s.SetRansacParameters(*RELOC)
    s.set_draws(rng.integers(0, np.array([n, n - 1, n - 2, n - 3]), (n_hyp, 4)))
    return s


def run(n_solvers, n, n_hyp, repeats, warmup, rng):
    batch = PnPBatch(n_solvers, n, n_hyp)
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
           "evaluated": [int(s.n_evaluated) for s in solvers], "records": [int(s.n_records) for s in solvers],
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
    print(json.dumps({"profile": "pnp_ransac", "gpus": 1, "timer_overhead_us": L.ktimer_calibrate(0),
                      "shapes": rows}))


if __name__ == "__main__":
    main()
