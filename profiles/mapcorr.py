"""Device and wall time of the three map corrections (include/orbfe_mapcorr.h) on one GPU at a map-sized shape:
1,000 keyframes on a track, 100,000 points with 8 observers each, the last 40 keyframes connected to the
current one (their rows hold about 32,000 slots), the last 8 keyframes and every tenth point not optimised.

The map is the one tests/cpp/mapcorr_core_test.cpp --bench generates for the host figure (the same shape and
structure; the random draws differ). Prints one JSON line:
  *_kernel_us   the sum of the call's kernels (kernel timer: each dispatch's own begin/end)
  *_call_us     host wall time of the whole call through the Python handle (packing, upload, kernels, copy back)
each as median / min / max over --repeats after --warmup, and `host`: the --bench line of the core header
composed serially on this machine's CPU (built -O2 without sanitizers into profile_out/).

    python profiles/mapcorr.py [--keyframes 1000] [--points 100000] [--observers 8] [--connected 40] [--repeats 20]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam2_2021_amd import MapCorrector  # noqa: E402
from orb_slam2_2021_amd import _lib as L  # noqa: E402

KERNELS = {"update_normal_depth": ["k_mc_normals"],
           "correct_loop": ["k_mc_centres", "k_mc_loop_kf", "k_mc_loop_mark", "k_mc_loop_point"],
           "apply_gba": ["k_mc_gba_kf", "k_mc_gba_point"]}


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def track(nk, npt, nobs, ncon, rng):
    a = 0.02 * (rng.random(nk) - 0.5)
    c, s, x = np.cos(a), np.sin(a), 0.1 * np.arange(nk)
    z, o = np.zeros(nk), np.ones(nk)
    tcw = np.stack([c, z, s, -x * c, z, o, z, z, -s, z, c, x * s], 1).astype(np.float32)
    first = np.minimum(np.arange(npt) * nk // npt, nk - nobs)
    xw = np.stack([0.1 * first + 4 * (rng.random(npt) - 0.5), 2 * (rng.random(npt) - 0.5), 4 + 8 * rng.random(npt)], 1).astype(np.float32)
    obs_kf = (first[:, None] + np.arange(nobs)[None, :]).astype(np.int32).reshape(-1)
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    pts = dict(n_points=npt, n_obs=npt * nobs, n_levels=8, scale_factors=scale, xw=xw, bad=np.zeros(npt, np.uint8),
               obs_begin=(np.arange(npt + 1) * nobs).astype(np.int32), obs_kf=obs_kf, ref_kf=first.astype(np.int32),
               ref_level=rng.integers(0, 8, npt).astype(np.int32))
    R = tcw.reshape(nk, 3, 4)
    ow = -np.einsum("kji,kj->ki", R[:, :, :3].astype(np.float64), R[:, :, 3].astype(np.float64)).astype(np.float32)
    normals = SimpleNamespace(n_kf=nk, ow=ow, **pts)
    conn = np.arange(nk - ncon, nk)
    rows = [np.flatnonzero((first <= k) & (k < first + nobs)).astype(np.int32) for k in conn]
    T = R[nk - 1].astype(np.float64)
    w = np.sqrt(max(1.0 + T[0, 0] + T[1, 1] + T[2, 2], 1e-12)) / 2
    q = np.array([(T[2, 1] - T[1, 2]) / (4 * w), (T[0, 2] - T[2, 0]) / (4 * w), (T[1, 0] - T[0, 1]) / (4 * w), w])
    loop = SimpleNamespace(n_kf=nk, tcw=tcw, n_connected=ncon, connected_kf=conn.astype(np.int32), cur=ncon - 1,
                           scw=np.concatenate([q, 1.05 * T[:, 3] + [0.3, 0.0, -0.2], [1.05]]),
                           n_slots=int(sum(len(r) for r in rows)),
                           row_begin=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32),
                           row_point=np.concatenate(rows).astype(np.int32), **pts)
    optimised = np.ones(nk, np.uint8)
    optimised[max(nk - 8, 1):] = 0
    gba_pose = tcw.copy()
    gba_pose[:, 3::4] += np.float32(0.01)
    pt_opt = np.ones(npt, np.uint8)
    pt_opt[::10] = 0
    gba = SimpleNamespace(n_kf=nk, tcw=tcw, tcw_gba=gba_pose, optimised=optimised, parent=(np.arange(nk) - 1).astype(np.int32),
                          n_points=npt, xw=xw, bad=pts["bad"], pt_optimised=pt_opt, xw_gba=xw, ref_kf=pts["ref_kf"])
    return normals, loop, gba


def host_figure(a):
    out_dir = os.path.join(ROOT, "profile_out")
    exe = os.path.join(out_dir, "mapcorr_core_bench")
    if not os.path.exists(exe):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "mapcorr_core_test.cpp")], check=True)
    out = subprocess.run([exe, "--bench", str(a.keyframes), str(a.points), str(a.observers), str(a.connected), str(a.repeats)],
                         check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--observers", type=int, default=8)
    ap.add_argument("--connected", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    problems = dict(zip(KERNELS, track(a.keyframes, a.points, a.observers, a.connected, np.random.default_rng(1))))
    h = MapCorrector(a.keyframes, a.points, max(a.points * a.observers, problems["correct_loop"].n_slots))
    out = {"profile": "mapcorr", "gpus": 1, "keyframes": a.keyframes, "points": a.points, "observers": a.observers,
           "connected": a.connected, "row_slots": problems["correct_loop"].n_slots, "repeats": a.repeats, "warmup": a.warmup,
           "timer_overhead_us": L.ktimer_calibrate(0)}
    for name, kernels in KERNELS.items():
        call, p = getattr(h, name), problems[name]
        kernel, wall = [], []
        for it in range(a.warmup + a.repeats):
            L.ktimer_select(kernels)
            L.ktimer_reset()
            r = call(p)
            kt = L.ktimer_read()
            L.ktimer_select(None)
            t0 = time.perf_counter()
            call(p)
            t1 = time.perf_counter()
            if it >= a.warmup:
                kernel.append(1e3 * sum(kt[k][0] for k in kernels if k in kt))
                wall.append(1e6 * (t1 - t0))
        out[name + "_kernel_us"], out[name + "_call_us"] = spread(kernel), spread(wall)
        if name == "correct_loop":
            out["corrected_points"] = int((r.corrected_by >= 0).sum())
        if name == "apply_gba":
            out["gba_levels"] = r.levels
    h.close()
    out["host"] = host_figure(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
