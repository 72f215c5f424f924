"""orb_slam2_2021_amd/csrc/orbfe_localmap_core.h composed serially on the host, in a stand-alone program built with
ASan + UBSan (tests/cpp/localmap_core_test.cpp), against tests/local_map_ref.py on a case file the restatement
writes; CPU only. The cases: the hand-built walks, random scenes, rows whose lengths straddle the 256-slot block,
the argument and capacity checks, and the plan (grid and bound) the library launches from."""
import json
import os
import subprocess

import numpy as np
import pytest

import local_map_ref as R
from test_local_map_ref import WALK_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
OK, ERR_ARG, ERR_CAPACITY = 0, -1, -2


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(CPP, "build")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "localmap_core_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", path,
                    os.path.join(CPP, "localmap_core_test.cpp")], check=True)
    return path


def walk_line(rows, kf_list, bad, seen, n_points):
    """One D case and the line the program must print, from the restatement."""
    tok = ["D", n_points, len(kf_list), len(bad), len(seen)]
    for k in kf_list:
        tok += [len(rows[k])] + [int(p) for p in rows[k]]
    tok += list(bad) + list(seen)
    ref = R.build_ref({k: np.asarray(v, np.int32) for k, v in rows.items()}, {k: k for k in rows}, bad)
    want = ref.update_local_points(kf_list, 1)
    flags = np.isin(np.asarray(want, np.int64), np.asarray(seen, np.int64)).astype(int).tolist() if want else []
    return " ".join(map(str, tok)), " ".join(map(str, [len(want)] + want + ["|"] + flags))


def walk_cases():
    out = []
    for c in WALK_CASES:
        seen = [c["want"][0], -1, 0] if c["want"] else [-1, 1]
        out.append(walk_line(c["rows"], c["list"], c["bad"], seen, 16))
    for seed in (11, 12):
        rows, _, bad, n_points = R.random_scene(seed)
        rng = np.random.default_rng(seed)
        kf_list = rng.integers(0, len(rows), 25).tolist()
        out.append(walk_line(rows, kf_list, bad, rng.integers(-1, n_points, 60).tolist(), n_points))
    rng = np.random.default_rng(13)
    for n in (255, 256, 257, 511, 513):  # one block, its edge, and the next one
        rows = {0: rng.integers(-1, 300, n).tolist(), 1: rng.integers(-1, 300, 3).tolist(),
                2: rng.integers(-1, 300, n + 1).tolist()}
        out.append(walk_line(rows, [1, 0, 2, 0], [7, 8], [5, 6, 7], 300))
    return out


def check_cases():
    stored = [(3, 0), (5, 7), (9, 256), (11, 257), (12, 8192)]
    head = f"C 4096 8192 1000 {len(stored)} " + " ".join(f"{i} {n}" for i, n in stored)
    plan = lambda ids: (lambda lens: (max(lens), -(-max(lens) // 256), -(-max(lens) // 256) * len(ids), sum(lens),
                                      min(sum(lens), 1000)))([dict(stored)[i] for i in ids])
    out = []
    for ids in ([3], [5], [9], [11], [5, 9, 5], [12, 11], [3, 3]):
        out.append((f"{head} {len(ids)} " + " ".join(map(str, ids)), " ".join(map(str, (OK,) + plan(ids)))))
    out.append((f"{head} 0", f"{ERR_ARG} 0 0 0 0 0"))
    out.append((f"{head} 2 5 6", f"{ERR_ARG} 0 0 0 0 0"))  # 6 is not stored
    out.append((f"{head} 4097 " + " ".join(["5"] * 4097), f"{ERR_CAPACITY} 0 0 0 0 0"))
    ids = [12] * 4096  # the largest call there is: 2^25 slots, one block count per 256 of them
    out.append((f"{head} 4096 " + " ".join(map(str, ids)), f"{OK} 8192 32 131072 {1 << 25} 1000"))
    out.append(("G 100 3 0 0 5 4 99 216", str(OK)))       # every bit the store hands on: 4 | 8 | 16 | 64 | 128
    out.append(("G 100 0", str(OK)))
    for f in (1, 2, 32, 3):
        out.append((f"G 100 2 4 0 5 {f}", str(ERR_ARG)))  # TRACK_IN_VIEW, BAD, SEEN
    out.append(("G 100 2 4 0 100 0", str(ERR_ARG)))
    out.append(("G 100 2 4 0 -1 0", str(ERR_ARG)))
    out.append(("G 100 3 4 0 5 0 4 0", str(ERR_ARG)))     # named twice
    out.append(("S 100 4 -1 0 99 0", str(OK)))            # repeats and -1 are fine
    out.append(("S 100 1 -2", str(ERR_ARG)))
    out.append(("S 100 1 100", str(ERR_CAPACITY)))
    out.append(("S 100 8192 " + " ".join(["1"] * 8192), str(OK)))
    out.append(("S 100 8193 " + " ".join(["1"] * 8193), str(ERR_CAPACITY)))
    return out


def test_core_equals_the_restatement(exe, tmp_path):
    cs = walk_cases() + check_cases()
    (tmp_path / "cases.txt").write_text("\n".join(c for c, _ in cs) + "\n")
    out = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln.strip() for ln in out.stdout.splitlines()]
    assert len(lines) == len(cs)
    wrong = [(c[:200], w[:200], g[:200]) for (c, w), g in zip(cs, lines) if w != g]
    assert not wrong, wrong[:5]
    assert any(w.startswith("0 |") for c, w in cs if c[0] == "D")       # an empty result
    assert any(" 1" in w.split("|")[1] for c, w in cs if c[0] == "D")   # a seen point


def test_a_refused_case_file_is_an_error(exe, tmp_path):
    (tmp_path / "bad.txt").write_text("D 4 1 0 0 2 1 9\n")  # point 9 of 4
    out = subprocess.run([exe, str(tmp_path / "bad.txt")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2, out.stdout + out.stderr


def test_bench_mode_prints_the_host_time(exe):
    out = subprocess.run([exe, "--bench", "20", "200", "8", "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout)
    assert r["host_update_local_points_ms"] > 0 and r["keyframes"] == 20 and 0 < r["points"] <= 20 * 200
