"""Measures the local map on the device (include/orbfe_localmap.h) at Tracking's shape: 80 local
keyframes x 2000 slots, about 8 observers per point. Prints one JSON object.

  python profiles/local_map.py [--kf 80] [--slots 2000] [--observers 8] [--repeats 20]

Device time per kernel comes from the library's kernel timer (mean over the repeats: the timer keeps totals), host
time is wall time around the whole call with the timer off (median, min..max over the repeats, after warm-up).
Baselines, never the code under test: (a) tests/cpp/localmap_core_test --bench, the walk through vector<MapPoint*>
rows and stamp members on one core, built here with -O2; (b) the path without this feature for the same Frame: the
MapPointGeometry gathered on the host by the walk's ids and staged through SearchLocalPoints, against the
ResidentLocalMap through SearchLocalPoints, interleaved in one process."""
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

from orb_slam2_2021_amd import CovisibilityGraph, MapPointGeometry, ORBextractor, ORBmatcher, synth_frame  # noqa: E402
from orb_slam2_2021_amd import _lib as L  # noqa: E402
from orb_slam2_2021_amd import synthetic as S  # noqa: E402


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def kernels(fn, repeats):
    fn()
    L.ktimer_select("*")
    L.ktimer_reset()
    for _ in range(repeats):
        fn()
    r = L.ktimer_read()
    L.ktimer_select(None)
    return {k: {"mean_us": round(1e3 * t / repeats, 2), "launches_per_call": n / repeats} for k, (t, n) in sorted(r.items())}


def host_walk_bench(n_kf, slots, observers, repeats):
    src = os.path.join(ROOT, "tests", "cpp", "localmap_core_test.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "localmap_core_bench")
        subprocess.run(["g++", "-std=c++17", "-O2", "-o", exe, src], check=True)
        out = subprocess.run([exe, "--bench", str(n_kf), str(slots), str(observers), str(repeats)], check=True,
                             capture_output=True, text=True)
    return json.loads(out.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=80)
    ap.add_argument("--slots", type=int, default=2000)
    ap.add_argument("--observers", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(27)
    n_points = a.kf * a.slots // a.observers
    ext = ORBextractor(2000, 1.2, 8, 20, 7)
    k, d = ext(synth_frame(5, 376, 1241))
    F = S.make_frame(k, d, ext.GetScaleFactors(), ext.GetScaleSigmaSquares(), 376, 1241, S.KITTI_CAM, rng,
                     tcw=S.pose(tx=0.2, yaw=0.03))
    G = S.make_local_map(F, n_points, rng)
    stored = (G.flags & ~np.uint8(L.MPF_BAD | L.MPF_SEEN | L.MPF_TRACK_IN_VIEW)).astype(np.uint8)
    g = CovisibilityGraph(max(a.kf, 8), a.slots, n_points)
    window = max(1, a.observers * a.slots // 2)
    for kf in range(a.kf):
        base = kf * n_points // a.kf
        row = ((base + rng.integers(0, window, a.slots)) % n_points).astype(np.int32)
        row[rng.random(a.slots) < 0.1] = -1
        g.set_keyframe(kf, row)
        g.update_connections(kf)
    g.set_point_geometry(np.arange(n_points), G.world_pos, G.normal, G.min_distance, G.max_distance, G.descriptors,
                         flags=stored)
    frame_points = rng.integers(0, n_points, 1500).astype(np.int32)
    local = list(range(a.kf))
    m = ORBmatcher(0.8, True)
    ids = g.distinct_points(local)

    def host_path():  # the parent's path for this Frame, the walk itself excluded (baseline (a) times it)
        flags = stored[ids] | (L.MPF_SEEN * np.isin(ids, frame_points)).astype(np.uint8)
        H = MapPointGeometry(flags, G.world_pos[ids], G.normal[ids], G.min_distance[ids], G.max_distance[ids],
                             G.descriptors[ids])
        return m.SearchLocalPoints(F, H, 1.0)

    def resident_path():
        _, lm = g.local_geometry(local, frame_points)
        return m.SearchLocalPoints(F, lm, 1.0)

    nh, bh, _, _ = host_path()
    nd, bd, _, _ = resident_path()
    assert nh == nd and np.array_equal(bh, bd)
    out = {"shape": {"keyframes": a.kf, "slots": a.slots, "observers": a.observers, "point_ids": n_points,
                     "result_points": int(len(ids)), "repeats": a.repeats},
           "ktimer_overhead_us": round(L.ktimer_calibrate(0), 2),
           "device_distinct_points": kernels(lambda: g.distinct_points(local), a.repeats),
           "device_local_geometry": kernels(lambda: g.local_geometry(local, frame_points), a.repeats),
           "host_distinct_points": timed(lambda: g.distinct_points(local), a.repeats),
           "host_local_geometry": timed(lambda: g.local_geometry(local, frame_points), a.repeats),
           "host_update_local_map": timed(lambda: g.update_local_map(frame_points), a.repeats)}
    r = g.update_local_map(frame_points)
    out["update_local_map_keyframes"] = len(r.local_kf_ids)
    hp, rp = [], []
    for fn in (host_path, resident_path) * 3:
        fn()
    for _ in range(a.repeats):  # interleaved
        for fn, acc in ((host_path, hp), (resident_path, rp)):
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)
    out["baseline_b_host_geometry_search_local_points"] = stats(hp)
    out["resident_local_geometry_search_local_points"] = stats(rp)
    out["search_local_points_matches"] = int(nh)
    try:
        out["baseline_a_host_walk_one_core"] = host_walk_bench(a.kf, a.slots, a.observers, a.repeats)
    except (OSError, subprocess.CalledProcessError) as e:
        out["baseline_a_host_walk_one_core"] = f"not taken: {e}"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
