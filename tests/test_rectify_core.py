"""orb_slam2_2021_amd/csrc/orbfe_rectify_core.h through the host entry points of include/orbfe_rectify.h, in a
stand-alone program built with ASan + UBSan (tests/cpp/rectify_core_main.cpp) and run directly, bit for bit
against tests/rectify_ref.py; CPU only. The maps as float bit patterns, the fixed-point entries and the remapped
images for both arducam cameras at 640 x 480; a calibration that leaves its 600 x 440 source, with 5 and with 4
coefficients and a null R; the hand-built maps; 1, 3 and 4 channels, both gray modes and channel orders, padded
pitches, a row range with row0 > 0; bad arguments."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rectify_ref as R
from rectify_cases import hand_maps, random_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "orb_slam2_2021_amd", "csrc")
ERR_ARG = -1


@pytest.fixture(scope="module")
def exe():
    out_dir = os.path.join(CPP, "build")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "rectify_core_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DORBFE_RECTIFY_STANDALONE",
                    "-o", path, os.path.join(CPP, "rectify_core_main.cpp"),
                    os.path.join(CSRC, "orbfe_rectify_host.cpp")], check=True)
    return path


def run(exe, tmp_path, records):
    (tmp_path / "cases.bin").write_bytes(b"".join(records))
    out = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return (tmp_path / "answers.bin").read_bytes()


class Answers:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, dtype, n):
        a = np.frombuffer(self.data, dtype, n, self.at)
        self.at += a.nbytes
        return a

    def status(self):
        return int(self.take("<i4", 1)[0])

    def done(self):
        return self.at == len(self.data)


def maps_case(cam, size):
    d = [float(v) for v in cam["D"]]
    r = cam.get("R")
    return b"".join([struct.pack("<5i", 1, len(d), 0 if r is None else 1, size[1], size[0]),
                     np.asarray(cam["K"], "<f8").reshape(9).tobytes(), np.asarray(d + [0.0] * (5 - len(d)), "<f8").tobytes(),
                     (np.eye(3) if r is None else np.asarray(r, "<f8")).reshape(9).tobytes(),
                     np.asarray(cam["P"], "<f8").reshape(3, -1)[:, :3].tobytes()])


def entries_case(m1, m2, src_size):
    return struct.pack("<5i", 2, m1.shape[0], m1.shape[1], src_size[1], src_size[0]) + m1.tobytes() + m2.tobytes()


def remap_case(src, m1, m2, rows, gray_out, rgb, mode, src_pad, map_pad_floats, dst_pad):
    ch = 1 if src.ndim == 2 else src.shape[2]
    oc = 1 if (gray_out and ch != 1) else ch
    head = struct.pack("<14i", 3, src.shape[0], src.shape[1], src.shape[1] * ch + src_pad, ch, m1.shape[0], m1.shape[1],
                       4 * (m1.shape[1] + map_pad_floats), rows[0], rows[1], int(rgb), mode, int(gray_out),
                       m1.shape[1] * oc + dst_pad)
    return head + np.ascontiguousarray(src).tobytes() + m1.tobytes() + m2.tobytes()


def check_remap(ans, src, m1, m2, rows, gray_out, rgb, mode, dst_pad, tag):
    want = R.rectify(src, m1, m2, rows, gray_out, rgb, mode)
    want = want.reshape(want.shape[0], -1)
    pitch = want.shape[1] + dst_pad
    assert ans.status() == 0, tag
    got = ans.take(np.uint8, (want.shape[0] - 1) * pitch + want.shape[1])
    full = np.full(want.shape[0] * pitch, 0xA5, np.uint8)
    np.lib.stride_tricks.as_strided(full, want.shape, (pitch, 1))[...] = want
    assert np.array_equal(got, full[:len(got)]), (tag, np.nonzero(got != full[:len(got)])[0][:8])


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def colour_source(rng, rows, cols, ch):
    return rng.integers(0, 256, (rows, cols) + ((ch,) if ch != 1 else ()), dtype=np.uint8)


def test_arducam_cameras_at_vga(exe, tmp_path):
    A = R.arducam()
    size = (A["width"], A["height"])
    rng = np.random.default_rng(7)
    src = colour_source(rng, 480, 640, 3)
    cams = [A["left"], A["right"]]
    ref = [R.rectify_maps(c["K"], c["D"], c["R"], c["P"], size) for c in cams]
    records = []
    for c, (m1, m2) in zip(cams, ref):
        records += [maps_case(c, size), entries_case(m1, m2, size),
                    remap_case(src, m1, m2, (0, 400), True, True, R.GRAY_SHIFT15, 0, 0, 0)]
    ans = Answers(run(exe, tmp_path, records))
    for name, (m1, m2) in zip(("left", "right"), ref):
        assert ans.status() == 0
        assert same_bits(ans.take("<f4", m1.size), m1.reshape(-1)), name
        assert same_bits(ans.take("<f4", m2.size), m2.reshape(-1)), name
        assert ans.status() == 0
        want = R.fixed_point(m1, m2, size)
        assert ans.take(R.ENTRY_DTYPE, m1.size).tobytes() == want.tobytes(), name
        assert R.classify(want, size) == (0, 0, 640 * 480)
        check_remap(ans, src, m1, m2, (0, 400), True, True, R.GRAY_SHIFT15, 0, name)
    assert ans.done()


def test_a_calibration_that_leaves_the_source(exe, tmp_path):
    S = R.synthetic_camera()
    full = dict(K=S["K"], D=S["D"], R=S["R"], P=S["P"])
    short = dict(K=S["K"], D=S["D"][:4], R=None, P=S["P"])
    rng = np.random.default_rng(8)
    src = colour_source(rng, S["src_size"][1], S["src_size"][0], 3)
    ref = [R.rectify_maps(c["K"], c["D"], c["R"], c["P"], S["size"]) for c in (full, short)]
    records = []
    for c, (m1, m2) in zip((full, short), ref):
        records += [maps_case(c, S["size"]), entries_case(m1, m2, S["src_size"]),
                    remap_case(src, m1, m2, (3, 470), False, True, R.GRAY_SHIFT15, 5, 3, 2)]
    ans = Answers(run(exe, tmp_path, records))
    for tag, (m1, m2) in zip(("5 coefficients", "4 coefficients, R = NULL"), ref):
        assert ans.status() == 0
        assert same_bits(ans.take("<f4", m1.size), m1.reshape(-1)), tag
        assert same_bits(ans.take("<f4", m2.size), m2.reshape(-1)), tag
        assert ans.status() == 0
        want = R.fixed_point(m1, m2, S["src_size"])
        assert ans.take(R.ENTRY_DTYPE, m1.size).tobytes() == want.tobytes(), tag
        n_out, n_part, n_in = R.classify(want, S["src_size"])
        assert n_out > 0 and n_part > 0 and n_in > 0, (tag, n_out, n_part, n_in)
        check_remap(ans, src, m1, m2, (3, 470), False, True, R.GRAY_SHIFT15, 2, tag)
    assert ans.done()
    assert not same_bits(ref[0][0], ref[1][0])


def test_hand_built_maps(exe, tmp_path):
    src, m1, m2 = hand_maps()
    size = (src.shape[1], src.shape[0])
    ans = Answers(run(exe, tmp_path, [entries_case(m1, m2, size),
                                      remap_case(src, m1, m2, (0, m1.shape[0]), False, True, 0, 0, 0, 0)]))
    assert ans.status() == 0
    assert ans.take(R.ENTRY_DTYPE, m1.size).tobytes() == R.fixed_point(m1, m2, size).tobytes()
    check_remap(ans, src, m1, m2, (0, m1.shape[0]), False, True, 0, 0, "hand")
    assert ans.done()


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_channels_gray_modes_orders_pitches_and_row_ranges(exe, tmp_path, channels):
    rng = np.random.default_rng(20 + channels)
    srows, scols, drows, dcols = 13, 17, 11, 23
    src = colour_source(rng, srows, scols, channels)
    m1, m2 = random_maps(rng, drows, dcols, srows, scols)
    assert min(R.classify(R.fixed_point(m1, m2, (scols, srows)), (scols, srows))) > 0
    cases = [(rows, g, rgb, mode, pads) for rows in ((0, drows), (4, 9)) for g in (False, True)
             for rgb in (True, False) for mode in (R.GRAY_SHIFT15, R.GRAY_SHIFT14) for pads in ((0, 0, 0), (5, 2, 3))]
    ans = Answers(run(exe, tmp_path, [remap_case(src, m1, m2, rows, g, rgb, mode, *pads)
                                      for rows, g, rgb, mode, pads in cases]))
    for rows, g, rgb, mode, pads in cases:
        check_remap(ans, src, m1, m2, rows, g, rgb, mode, pads[2], (rows, g, rgb, mode, pads))
    assert ans.done()


def test_bad_arguments_are_refused(exe, tmp_path):
    ans = Answers(run(exe, tmp_path, [struct.pack("<i", 4)]))
    n = ans.status()
    assert n >= 20
    assert ans.take("<i4", n).tolist() == [ERR_ARG] * n
    assert ans.done()
