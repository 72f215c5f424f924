"""orb_slam2_2021_amd/csrc/orbfe_mapcorr_core.h composed serially on the host, in a stand-alone program built
with ASan + UBSan (tests/cpp/mapcorr_core_test.cpp), bit for bit against tests/mapcorr_ref.py on case files the
restatement writes; CPU only. The cases cover the three calls: empty and bad points, strayed reference
keyframes, a point at a camera centre (NaN), rows with -1 and repeats, a point in every row, the current
keyframe alone, runs of keyframes that are not optimised, two origins."""
import json
import os
import subprocess

import numpy as np
import pytest

import mapcorr_ref as R
import mapcorr_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(CPP, "build")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "mapcorr_core_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", path,
                    os.path.join(CPP, "mapcorr_core_test.cpp")], check=True)
    return path


def cases():
    at_centre = S.normals_problem(5, 3, 4, [2, 1])
    at_centre.bad[:] = 0
    at_centre.xw[1] = at_centre.ow[at_centre.obs_kf[at_centre.obs_begin[1]]]
    two_origins = np.array([-1, 0, 1, -1, 3, 3, 5], np.int32), np.array([1, 0, 0, 1, 1, 0, 0], np.uint8)
    return [
        (1, S.normals_problem(1, 5, 40, [0, 1, 2, 3, 8])),
        (1, S.normals_problem(2, 1, 3, [1], n_levels=1)),
        (1, S.normals_problem(3, 2, 0, [1])),
        (1, at_centre),
        (2, S.loop_problem(10, 6, 4, [30, 0, 12], 50, [0, 1, 2, 5], in_every_row=(3, 4))),
        (2, S.loop_problem(11, 1, 1, [7], 9, [1, 0])),
        (2, S.loop_problem(12, 9, 9, [25], 30, [3, 9], n_levels=1)),
        (2, S.loop_problem(13, 3, 2, [0], 5, [2])),
        (3, S.gba_problem(20, *S.tree_with_runs(12, [0, 1, 2, 3]), 40)),
        (3, S.gba_problem(21, *two_origins, 25)),
        (3, S.gba_problem(22, np.full(1, -1), np.ones(1), 3)),
        (3, S.gba_problem(23, [], [], 2)),
    ]


def test_core_equals_the_restatement_bit_for_bit(exe, tmp_path):
    cs = cases()
    R.write_cases(tmp_path / "cases.txt", cs)
    out = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cs)
    seen_nan = False
    for i, ((kind, p), line) in enumerate(zip(cs, lines)):
        want = R.expected_line(kind, p).split()
        got = line.split()
        assert len(got) == len(want), (i, kind, len(got), len(want))
        bad = [j for j, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (i, kind, bad[:8], [got[j] for j in bad[:8]], [want[j] for j in bad[:8]])
        seen_nan |= kind == 1 and any(w.startswith("7fc0") or w.startswith("ffc0") for w in want)
    assert seen_nan  # the point at a camera centre


def test_a_refused_case_file_is_an_error(exe, tmp_path):
    p = S.normals_problem(1, 5, 4, [2])
    p.obs_kf[0] = 5
    R.write_cases(tmp_path / "bad.txt", [(1, p)])
    out = subprocess.run([exe, str(tmp_path / "bad.txt")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2, out.stdout + out.stderr


def test_bench_mode_prints_the_three_host_times(exe):
    out = subprocess.run([exe, "--bench", "12", "200", "4", "5", "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout)
    assert {"host_update_normal_depth_ms", "host_correct_loop_ms", "host_apply_gba_ms"} <= set(r)
    assert r["corrected_points"] > 0 and r["row_slots"] > 0
