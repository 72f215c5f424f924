"""orb_slam2_2021_amd/csrc/orbfe_frame_core.h through the host entry points of include/orbfe_frame.h, in a
stand-alone program built with ASan + UBSan (tests/cpp/frame_core_main.cpp), bit for bit against
tests/sensor_ref.py; CPU only. The cases: the TUM fr1 camera with 5 and with 4 coefficients and a camera with
k1 = -1.5 on a 9 x 7 lattice over 640 x 480 (fractional coordinates included), the two k1 == 0 early-outs, the
bounds of each camera, and the depth maps and edge keys of tests/sensor_cases.py."""
import os
import subprocess

import numpy as np
import pytest

import sensor_ref as R
from sensor_cases import (CAMERAS, COLS, DEPTH_CASES, EDGE_KEYS, LATTICE, MAP_CAM, MAP_COLS, MAP_ROWS, ROWS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "orb_slam2_2021_amd", "csrc")


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(CPP, "build")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "frame_core_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DORBFE_FRAME_STANDALONE",
                    "-o", path, os.path.join(CPP, "frame_core_main.cpp"),
                    os.path.join(CSRC, "orbfe_frame_host.cpp")], check=True)
    return path


def hx(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def cam_line(cam):
    d = list(cam["dist"]) + [0.0] * (5 - len(cam["dist"]))
    return " ".join(["C"] + [hx(cam[f]) for f in ("fx", "fy", "cx", "cy")] + [str(len(cam["dist"]))] +
                    [hx(v) for v in d] + [hx(cam["bf"])])


def key_lines(keys):
    return ["K %s %s %s %s %s %d %d" % (hx(k["x"]), hx(k["y"]), hx(k["size"]), hx(k["angle"]), hx(k["response"]),
                                        k["octave"], k["class_id"]) for k in keys]


def map_line(m, factor, extra):
    t = 0 if m.dtype == np.uint16 else 1
    vals = m.astype(np.uint32) if t == 0 else m.view(np.uint32)
    return "M %d %d %d %d %s %s" % (t, m.shape[0], m.shape[1], m.shape[1] + extra, hx(factor),
                                    " ".join("%x" % v for v in vals.reshape(-1)))


def want_keys(cam, keys, m, factor):
    un = R.undistort_keys(cam, keys)
    ur, dep = R.stereo_from_depth(cam, keys, un, m, factor)
    return ["K %s %s %s %s %s %d %d %s %s" % (hx(u["x"]), hx(u["y"]), hx(u["size"]), hx(u["angle"]),
                                              hx(u["response"]), u["octave"], u["class_id"], hx(a), hx(b))
            for u, a, b in zip(un, ur, dep)]


def run(exe, tmp_path, lines):
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return [ln.strip() for ln in out.stdout.splitlines()]


def test_k1_negative_takes_the_icdist_exit_for_some_points_only():
    trace = []
    R.undistort_keys(CAMERAS["k1_neg"], LATTICE, trace)
    assert len(trace) == len(LATTICE) == 63 and 0 < sum(trace) < len(trace)
    trace = []
    R.undistort_keys(CAMERAS["fr1"], LATTICE, trace)
    assert not any(trace)
    assert (LATTICE["x"] != np.floor(LATTICE["x"])).any() and (LATTICE["y"] != np.floor(LATTICE["y"])).any()


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_lattice_and_bounds_equal_the_reference(exe, tmp_path, name):
    cam = CAMERAS[name]
    lines = [cam_line(cam), "B %d %d" % (ROWS, COLS), "M none"] + key_lines(LATTICE) + ["E"]
    want = ["B " + " ".join(hx(v) for v in R.image_bounds(cam, ROWS, COLS))] + want_keys(cam, LATTICE, None, 1.0)
    got = run(exe, tmp_path, lines)
    assert len(got) == len(want)
    wrong = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not wrong, wrong[:5]
    if name in ("fr1", "fr1_4", "k1_neg"):
        assert want[1:] != want_keys(CAMERAS["k1_zero"], LATTICE, None, 1.0)  # the points do move


@pytest.mark.parametrize("case", DEPTH_CASES, ids=[c[0] for c in DEPTH_CASES])
def test_stereo_from_depth_equals_the_reference(exe, tmp_path, case):
    _, m, factor = case
    assert m.shape == (MAP_ROWS, MAP_COLS)
    lines = [cam_line(MAP_CAM), map_line(m, factor, 3)] + key_lines(EDGE_KEYS) + ["E"]
    want = want_keys(MAP_CAM, EDGE_KEYS, m, factor)
    got = run(exe, tmp_path, lines)
    assert got == want
    dep = [w.split()[-1] for w in want]
    assert hx(-1.0) in dep and any(d != hx(-1.0) for d in dep)  # both branches of d > 0


def test_gray_rule_equals_the_reference(exe, tmp_path):
    rng = np.random.default_rng(3)
    px = np.concatenate([rng.integers(0, 256, (200, 3)), [[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0],
                                                          [0, 0, 255]]]).astype(np.uint8)
    lines, want = [], []
    for mode in (R.GRAY_SHIFT15, R.GRAY_SHIFT14):
        for rgb in (1, 0):
            g = R.gray(px[None], bool(rgb), mode)[0]
            for p, v in zip(px, g):
                lines.append("G %d %d %d %d %d" % (mode, rgb, p[0], p[1], p[2]))
                want.append("G %d" % v)
    assert run(exe, tmp_path, lines) == want


def test_bad_arguments_are_refused(exe, tmp_path):
    (tmp_path / "bad.txt").write_text(cam_line(dict(CAMERAS["fr1"], dist=CAMERAS["fr1"]["dist"][:3])) + "\nB 4 4\n")
    out = subprocess.run([exe, str(tmp_path / "bad.txt")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3, out.stdout + out.stderr
