"""orb_slam2_2021_amd/csrc/orbfe_cull_core.h composed serially on the host, in a stand-alone program built with
ASan + UBSan (tests/cpp/cull_core_test.cpp), bit for bit against tests/culling_ref.py on a case file the restatement
writes; CPU only. The cases: every (nRedundantObservations, nMPs) within 2 of the 0.9 line for nMPs <= 8192, every
found / visible pair up to 64 at every age and threshold edge, the hand-built scenes and random ones."""
import json
import os
import subprocess

import numpy as np
import pytest

import culling_ref as C
from test_culling_ref import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(CPP, "build")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "cull_core_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", path,
                    os.path.join(CPP, "cull_core_test.cpp")], check=True)
    return path


def line_cases():
    out = []
    for n_mps in range(0, 8193):
        at = 9 * n_mps // 10
        for n_red in range(max(at - 2, 0), min(at + 3, n_mps + 1)):
            out.append((f"L {n_red} {n_mps}", "1" if n_red > 0.9 * n_mps else "0"))
    return out


def point_cases():
    out = []
    for found in range(65):
        for visible in range(65):
            for age, obs, mono in ((0, 9, 1), (2, 2, 1), (2, 3, 1), (2, 3, 0), (2, 4, 0), (3, 9, 0)):
                want = C.point_action(False, found, visible, 100 + age, 100, obs, 2 if mono else 3)
                out.append((f"P 0 {found} {visible} {100 + age} 100 {obs} {mono}", str(want)))
    out.append(("P 1 0 1 5 5 0 1", "1"))
    out.append((f"P 0 1 1 {2 ** 31 - 1} 0 9 1", "4"))
    out.append((f"P 0 1 1 0 {2 ** 31 - 1} 0 1", "0"))
    return out


def attr_bytes(k):
    far = (k.depth > k.th_depth) | (k.depth < np.float32(0))
    return (np.asarray(k.octaves, np.int64) | (0x20 * (k.u_right >= np.float32(0))) | (0x40 * far)).tolist()


def scene_case(kfs, cand, mono, not_erase=(), bad=()):
    kfs = sorted(kfs, key=lambda k: k.mn_id)
    row = {k.mn_id: r for r, k in enumerate(kfs)}
    n_points = 1 + max([int(k.points.max()) for k in kfs if len(k.points)] + list(bad) + [0])
    tok = ["S", int(bool(mono)), len(kfs), n_points, len(bad), len(cand)]
    for k in kfs:
        tok += [k.mn_id, len(k.points)]
        for p, a in zip(k.points.tolist(), attr_bytes(k)):
            tok += [p, a]
    tok += list(bad)
    for i in cand:
        tok += [row[i], 1 if i in set(not_erase) else 0]
    out = C.build_ref(kfs, bad).keyframe_culling(cand, mono, not_erase)
    want = " | ".join(" ".join(map(str, [d, m, r, len(b)] + b)) for d, m, r, b in
                      zip(out.decision, out.n_mps, out.n_redundant, out.bad_points))
    return " ".join(map(str, tok)), want


def scene_cases():
    out = [scene_case(c["kfs"], c["cand"], c["mono"], c["not_erase"], c["bad"]) for c in CASES]
    for seed in (30, 31):
        out.append(scene_case(*C.random_scene(seed, n_kf=40, slots=24, n_candidates=20)))
    return out


def test_core_equals_the_restatement(exe, tmp_path):
    cs = line_cases() + point_cases() + scene_cases()
    (tmp_path / "cases.txt").write_text("\n".join(c for c, _ in cs) + "\n")
    out = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln.strip() for ln in out.stdout.splitlines()]
    assert len(lines) == len(cs)
    wrong = [(c, w, g) for (c, w), g in zip(cs, lines) if w != g]
    assert not wrong, wrong[:5]
    assert {w for c, w in cs if c[0] == "P"} == {"0", "1", "2", "3", "4"}
    assert any("1 " in w[:2] and w.split()[3] != "0" for c, w in cs if c[0] == "S")  # a cull with a cascade


def test_a_refused_case_file_is_an_error(exe, tmp_path):
    (tmp_path / "bad.txt").write_text("S 1 1 4 0 1 7 2 0 0 9 0 0 0\n")  # point 9 of 4
    out = subprocess.run([exe, str(tmp_path / "bad.txt")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2, out.stdout + out.stderr


def test_bench_mode_prints_the_host_time(exe):
    out = subprocess.run([exe, "--bench", "60", "100", "8", "10", "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout)
    assert r["host_keyframe_culling_ms"] > 0 and r["candidates"] == 10 and r["culled"] >= 1
