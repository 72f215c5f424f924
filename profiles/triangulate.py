"""Triangulation of SearchForTriangulation's matches (include/orbfe_triangulate.h) on one GPU.

Prints one JSON line:
  k_triangulate_us      device time of k_triangulate per launch, from the library's kernel timer
                        (32 pairs of ~2,000 keypoints with ~45 matches each: the bench's counts)
  batch32_us            host wall time of orbfe_triangulate_batch_device for those 32 pairs, enqueue
                        to stream idle: median, p10, p90 over --repeats calls after --warmup calls
  create10_us           the same for orbfe_create_new_mappoints_device, one KF1 of 2,000 keypoints
                        against 10 neighbours (search + triangulation + marking per neighbour); the
                        KeyFrames' mp_state is restored on the device before every call
The scenes are the tests' seeded ones (tests/triangulate_scenes.py).

    python profiles/triangulate.py [--repeats 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import triangulate_scenes as S  # noqa: E402
from orb_slam2_2021_amd import ORBmatcher  # noqa: E402
from orb_slam2_2021_amd import _lib as L  # noqa: E402


def stats(t):
    return {"median": 1e6 * float(np.median(t)), "p10": 1e6 * float(np.percentile(t, 10)),
            "p90": 1e6 * float(np.percentile(t, 90))}


def timed(fn, sync, repeats, warmup, before=None):
    for _ in range(warmup):
        if before:
            before()
        fn()
        sync()
    t = np.zeros(repeats)
    for k in range(repeats):
        if before:
            before()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        sync()
        t[k] = time.perf_counter() - t0
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    m = ORBmatcher(0.6, False)
    # 32 pairs, 2,000 keypoints, ~45 matches each
    hold, pairs, nmatch = [], [], []
    for k in range(32):
        sc = S.Scene("mixed", 2000, 900 + k, match_frac=45 / 2000)
        d1, d2 = sc.kf1.to_device(dev), sc.kf2.to_device(dev)
        t = dict(m12=torch.from_numpy(sc.match12).to(dev), status=torch.zeros(2000, dtype=torch.int8, device=dev),
                 x3d=torch.zeros(2000, 3, device=dev), nnew=torch.zeros(1, dtype=torch.int32, device=dev))
        p = L.tri_pair()
        p.kf1, p.kf2, p.t1, p.t2 = d1.view(), d2.view(), d1.tri_view(), d2.tri_view()
        p.match12, p.status, p.x3d, p.nnew = (L.ptr(t[f]) for f in ("m12", "status", "x3d", "nnew"))
        hold.append((d1, d2, t))
        pairs.append(p)
        nmatch.append(int((sc.match12 >= 0).sum()))
    arr = (L.tri_pair * 32)(*pairs)
    torch.cuda.synchronize()
    t32 = timed(lambda: m.TriangulateBatchDevice(arr), m.synchronize, a.repeats, a.warmup)
    nnew32 = [int(h[2]["nnew"].item()) for h in hold]
    L.ktimer_select(["k_triangulate", "k_tri_zero"])
    L.ktimer_reset()
    for _ in range(min(a.repeats, 64)):
        m.TriangulateBatchDevice(arr)
    m.synchronize()
    kt = {name: 1e3 * ms / launches for name, (ms, launches) in L.ktimer_read().items()}
    L.ktimer_select(None)
    L.ktimer_reset()
    # one KF1 against 10 neighbours
    ch = S.ChainScene(10, n=2000, seed=31)
    d1 = ch.kf1.to_device(dev)
    dn = [nb.to_device(dev) for nb in ch.nbs]
    saved = [d.mp_state.clone() for d in [d1] + dn]

    def restore():
        for d, s in zip([d1] + dn, saved):
            d.mp_state.copy_(s)

    res = {}

    def create():
        res["out"] = m.CreateNewMapPointsDevice(d1, dn, ch.f12, ch.epipole)

    t10 = timed(create, m.synchronize, a.repeats, a.warmup, before=restore)
    print(json.dumps({"profile": "triangulate", "gpus": 1, "timer_overhead_us": L.ktimer_calibrate(0),
                      "batch32": {"pairs": 32, "keypoints": 2000, "matches_mean": float(np.mean(nmatch)),
                                  "nnew_mean": float(np.mean(nnew32)), "batch32_us": stats(t32), "kernels_us": kt},
                      "create10": {"neighbours": 10, "keypoints": 2000,
                                   "nmatches": [int(v) for v in res["out"][3].cpu()],
                                   "nnew": [int(v) for v in res["out"][4].cpu()], "create10_us": stats(t10)}}))
    m.close()


if __name__ == "__main__":
    main()
