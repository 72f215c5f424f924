"""tests/sensor_ref.py held to values worked out by hand from the rules it restates (DESIGN.md "Monocular and
RGB-D Frames"); CPU only. The library is compared with sensor_ref in test_frame_core.py and the GPU tests."""
import numpy as np
import pytest

import sensor_ref as R
from sensor_cases import CAMERAS


def px(c0, c1, c2, *alpha):
    return np.array([[[c0, c1, c2, *alpha]]], np.uint8)


# pure colours: 255 * coefficient + half, shifted. 15 bits: R (2498490 + 16384) >> 15 = 76,
# G (4904925 + 16384) >> 15 = 150, B (952425 + 16384) >> 15 = 29; 14 bits: R (1249245 + 8192) >> 14 = 76,
# G (2452335 + 8192) >> 14 = 150, B (476340 + 8192) >> 14 = 29. White: the coefficients sum to 1 << shift, so
# (255 << shift + half) >> shift = 255.
@pytest.mark.parametrize("mode", [R.GRAY_SHIFT15, R.GRAY_SHIFT14])
def test_gray_of_pure_colours(mode):
    for rgb in (True, False):
        assert R.gray(px(255, 255, 255), rgb, mode)[0, 0] == 255
        assert R.gray(px(0, 0, 0), rgb, mode)[0, 0] == 0
        assert R.gray(px(0, 255, 0), rgb, mode)[0, 0] == 150
    assert R.gray(px(255, 0, 0), True, mode)[0, 0] == 76    # channel 0 is R
    assert R.gray(px(0, 0, 255), True, mode)[0, 0] == 29
    assert R.gray(px(255, 0, 0), False, mode)[0, 0] == 29   # channel 0 is B
    assert R.gray(px(0, 0, 255), False, mode)[0, 0] == 76
    assert R.gray(px(255, 0, 0, 9), True, mode)[0, 0] == 76  # alpha ignored
    assert R.gray(px(255, 0, 0, 200), True, mode)[0, 0] == 76


def test_gray_modes_differ_where_the_tables_do():
    # B = 9: 15 bits (33615 + 16384) >> 15 = 1; 14 bits (16812 + 8192) >> 14 = 1; as channel 0 = B of (0, 0, 9):
    # R = 9 instead: (88182 + 16384) >> 15 = 3, (44091 + 8192) >> 14 = 3
    assert R.gray(px(0, 0, 9), True, R.GRAY_SHIFT15)[0, 0] == 1
    assert R.gray(px(0, 0, 9), False, R.GRAY_SHIFT15)[0, 0] == 3
    # 19235 = 2 * 9617 + 1 and 3735 = 2 * 1868 - 1: the two generations round some pixels differently
    rgb = np.stack(np.meshgrid(np.arange(0, 256, 5), np.arange(256), np.arange(0, 256, 5), indexing="ij"), -1)
    a, b = R.gray(rgb, True, R.GRAY_SHIFT15), R.gray(rgb, True, R.GRAY_SHIFT14)
    assert (a != b).any() and np.abs(a.astype(int) - b.astype(int)).max() == 1


@pytest.mark.parametrize("name", ["fr1", "fr1_4", "k1_neg"])
def test_the_principal_point_stays(name):
    # x = (cx - cx) * ifx = 0: r2 = 0, icdist = 1 / 1, both deltas 0, and fx * 0 + 0 * 0 + cx = cx
    cam = CAMERAS[name]
    x, y = R.undistort_point(cam, cam["cx"], cam["cy"])
    assert x == cam["cx"] and y == cam["cy"]


@pytest.mark.parametrize("name", ["k1_zero", "k1_negzero"])
def test_k1_zero_is_the_early_out(name):
    cam = CAMERAS[name]
    assert np.count_nonzero(cam["dist"]) == 4 and not R.distorted(cam)
    keys = R.lattice_keys(480, 640)
    assert R.undistort_keys(cam, keys).tobytes() == keys.tobytes()
    assert R.image_bounds(cam, 480, 640).tolist() == [0.0, 640.0, 0.0, 480.0]
    # the same coefficients behind a non-zero k1 do move the points
    other = R.camera(**dict(R.FR1, dist=(1e-3, *cam["dist"][1:])))
    assert R.undistort_keys(other, keys).tobytes() != keys.tobytes()


def test_depth_is_sampled_at_the_truncated_distorted_key():
    cam = CAMERAS["k1_zero"]
    keys = np.zeros(1, R.KEYPOINT_DTYPE)
    keys["x"], keys["y"] = 10.8, 5.9
    un = keys.copy()
    un["x"] = 100.0
    m = np.zeros((30, 40), np.float32)
    m[5, 10], m[6, 11], m[5, 11], m[6, 10] = 2.0, 3.0, 4.0, 5.0
    ur, dep = R.stereo_from_depth(cam, keys, un, m, 1.0)
    assert dep[0] == 2.0 and ur[0] == np.float32(100.0) - np.float32(40.0) / np.float32(2.0)  # kpU.x - mbf / d
    for bad in (0.0, -1.0, np.nan):
        m[5, 10] = bad
        ur, dep = R.stereo_from_depth(cam, keys, un, m, 1.0)
        assert ur[0] == -1 and dep[0] == -1
    ur, dep = R.stereo_from_depth(cam, keys, un, None, 1.0)
    assert ur[0] == -1 and dep[0] == -1


def test_depth_conversion():
    # uint16 is always converted: 5000 * float(1 / 5000); float at factor 1 is not; 1 + 2e-5 is, 1 + 5e-6 is not
    f = np.float32(1.0) / np.float32(5000.0)
    assert R.depth_value(np.uint16(5000), f) == np.float32(5000.0) * f
    assert R.depth_value(np.uint16(7), np.float32(1.0)) == np.float32(7.0)
    v = np.float32(3.0000002)
    assert R.depth_value(v, np.float32(1.0)) == v
    assert R.depth_value(v, np.float32(1.000005)) == v
    assert R.depth_value(v, np.float32(1.00002)) == np.float32(v * np.float32(1.00002)) != v
    assert R.depth_value(v, np.float32(0.5)) == np.float32(1.5000001)
