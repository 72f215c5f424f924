"""tests/rectify_ref.py held to hand-computed values; CPU only. The identity calibration, a half-pixel shift, the
float ties of the 1/32 grid, -0.5, each "fully outside" condition at equality and one step short of it, taps
outside on each side and at a corner, map values with no int conversion, and the argument that the exact weight
32768 of a = b = 0 gives what OpenCV's stored 32767 + 1 gives."""
import numpy as np

import rectify_ref as R
from rectify_cases import SRC_COLS, SRC_ROWS, hand_maps


def entry(x, y, size=(SRC_COLS, SRC_ROWS)):
    e = R.fixed_point(np.array([[x]], np.float32), np.array([[y]], np.float32), size)[0, 0]
    return int(e["ix"]), int(e["iy"]), int(e["alpha"]), int(e["outside"])


def pixel(src, x, y):
    m1, m2 = np.array([[x]], np.float32), np.array([[y]], np.float32)
    return int(R.rectify(src, m1, m2)[0, 0])


def test_identity_calibration_returns_the_input():
    K = [[500.0, 0.0, 319.5], [0.0, 480.0, 239.5], [0.0, 0.0, 1.0]]
    m1, m2 = R.rectify_maps(K, [0.0, 0.0, 0.0, 0.0], np.eye(3), K, (40, 30))
    e = R.fixed_point(m1, m2, (40, 30))
    i, j = np.mgrid[0:30, 0:40]
    sx = e["ix"].astype(np.int64) * 32 + (e["alpha"] & 31)
    sy = e["iy"].astype(np.int64) * 32 + (e["alpha"] >> 5)
    assert np.array_equal(sx, 32 * j) and np.array_equal(sy, 32 * i) and not e["alpha"].any()
    assert not e["outside"].any()
    src = np.random.default_rng(0).integers(0, 256, (30, 40, 3), dtype=np.uint8)
    assert np.array_equal(R.remap(src, e), src)  # last row and column included: their outside taps weigh 0
    assert np.array_equal(R.rectify(src[..., 0], m1, m2), src[..., 0])
    # R None is the identity; D with 5 entries, the fifth zero, is D with 4
    m1b, m2b = R.rectify_maps(K, [0.0, 0.0, 0.0, 0.0, 0.0], None, K, (40, 30))
    assert np.array_equal(m1.view(np.uint32), m1b.view(np.uint32)) and np.array_equal(m2.view(np.uint32), m2b.view(np.uint32))


def test_hand_source_identity_rows():
    src, m1, m2 = hand_maps()
    out = R.rectify(src, m1, m2)
    assert np.array_equal(out[:SRC_ROWS], src)


def test_half_pixel_shift():
    src, _, _ = hand_maps()
    p, q = int(src[2, 3]), int(src[2, 4])
    assert entry(3.5, 2.0) == (3, 2, 16, 0)
    assert pixel(src, 3.5, 2.0) == (p + q + 1) >> 1
    p, q = int(src[2, 3]), int(src[3, 3])
    assert entry(3.0, 2.5) == (3, 2, 16 * 32, 0)
    assert pixel(src, 3.0, 2.5) == (p + q + 1) >> 1


def test_float_ties_round_to_even():
    big = (4000, 4000)
    assert entry(10 + 1 / 64, 0.0, big)[:3] == (10, 0, 0)        # 320.5 -> 320
    assert entry(10 + 3 / 64, 0.0, big)[:3] == (10, 0, 2)        # 321.5 -> 322
    assert entry(0.0, 10 + 1 / 64, big)[:3] == (0, 10, 0)
    assert entry(0.0, 10 + 3 / 64, big)[:3] == (0, 10, 2 * 32)
    assert entry(-1 / 64, 0.0, big)[:3] == (0, 0, 0)             # -0.5 -> -0
    assert entry(-3 / 64, 0.0, big)[:3] == (-1, 0, 30)           # -1.5 -> -2


def test_minus_one_half():
    src, _, _ = hand_maps()
    assert entry(-0.5, 0.0) == (-1, 0, 16, 0)
    assert pixel(src, -0.5, 0.0) == (16384 * int(src[0, 0]) + 16384) >> 15
    assert entry(0.0, -0.5) == (0, -1, 16 * 32, 0)
    assert pixel(src, 0.0, -0.5) == (16384 * int(src[0, 0]) + 16384) >> 15


def test_fully_outside_conditions_at_equality_and_one_short():
    src, _, _ = hand_maps()
    assert entry(SRC_COLS, 2.0) == (SRC_COLS, 2, 0, 1)                      # ix >= cols
    assert entry(SRC_COLS - 1 / 32, 2.0) == (SRC_COLS - 1, 2, 31, 0)
    assert entry(-1 - 1 / 32, 2.0) == (-2, 2, 31, 1)                        # ix + 1 < 0
    assert entry(-1.0, 2.0) == (-1, 2, 0, 0)
    assert entry(3.0, SRC_ROWS) == (3, SRC_ROWS, 0, 1)                      # iy >= rows
    assert entry(3.0, SRC_ROWS - 1 / 32) == (3, SRC_ROWS - 1, 31 * 32, 0)
    assert entry(3.0, -1 - 1 / 32) == (3, -2, 31 * 32, 1)                   # iy + 1 < 0
    assert entry(3.0, -1.0) == (3, -1, 0, 0)
    for x, y in ((SRC_COLS, 2.0), (-1 - 1 / 32, 2.0), (3.0, SRC_ROWS), (3.0, -1 - 1 / 32)):
        assert pixel(src, x, y) == 0
    # one short of it: only the inside taps count, with their own weights
    assert pixel(src, SRC_COLS - 1 / 32, 2.0) == (32 * 1 * 32 * int(src[2, SRC_COLS - 1]) + 16384) >> 15
    assert pixel(src, -1.0, 2.0) == 0                                       # the inside tap weighs 0
    assert pixel(src, 3.0, SRC_ROWS - 1 / 32) == (32 * 32 * 1 * int(src[SRC_ROWS - 1, 3]) + 16384) >> 15


def test_taps_outside_on_each_side_and_at_a_corner():
    src, _, _ = hand_maps()
    r, c = SRC_ROWS - 1, SRC_COLS - 1
    w = lambda a, b: 32 * a * b
    # right edge: x = c + 0.5, y = 2.25 (b = 8): taps (2, c) and (3, c) inside
    assert pixel(src, c + 0.5, 2.25) == (w(16, 24) * int(src[2, c]) + w(16, 8) * int(src[3, c]) + 16384) >> 15
    # bottom edge: x = 3.25 (a = 8), y = r + 0.5
    assert pixel(src, 3.25, r + 0.5) == (w(24, 16) * int(src[r, 3]) + w(8, 16) * int(src[r, 4]) + 16384) >> 15
    # left and top edges
    assert pixel(src, -0.5, 2.0) == (w(16, 32) * int(src[2, 0]) + 16384) >> 15
    assert pixel(src, 3.0, -0.5) == (w(32, 16) * int(src[0, 3]) + 16384) >> 15
    # the four corners: one tap inside, a quarter of it
    for x, y, p in ((-0.5, -0.5, src[0, 0]), (c + 0.5, -0.5, src[0, c]), (-0.5, r + 0.5, src[r, 0]),
                    (c + 0.5, r + 0.5, src[r, c])):
        assert pixel(src, x, y) == (w(16, 16) * int(p) + 16384) >> 15
    # three channels are blended one by one
    rgb = np.stack([src, 255 - src, src // 2], -1)
    m1, m2 = np.array([[c + 0.5]], np.float32), np.array([[2.25]], np.float32)
    got = R.rectify(rgb, m1, m2)[0, 0]
    for ch in range(3):
        assert int(got[ch]) == pixel(np.ascontiguousarray(rgb[..., ch]), c + 0.5, 2.25)
    g = R.rectify(rgb, m1, m2, gray_out=True)[0, 0]
    assert int(g) == (9798 * int(got[0]) + 19235 * int(got[1]) + 3735 * int(got[2]) + 16384) >> 15


def test_values_without_an_int_conversion_are_the_constant():
    src, _, _ = hand_maps()
    for x, y in ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf), (1e30, 1.0), (1.0, -1e30),
                 (7e7, 1.0)):
        assert entry(x, y) == (0, 0, 0, 1), (x, y)
        assert pixel(src, x, y) == 0
    assert entry(6e7, 1.0) == (32767, 1, 0, 1)            # fits an int, saturates the short: outside
    assert entry(-67108864.0, 1.0) == (-32768, 1, 0, 1)   # the product is -2^31 exactly
    assert entry(1.0, -6e7) == (1, -32768, 0, 1)


def test_exact_weight_equals_the_stored_one_for_every_byte():
    """a = b = 0: OpenCV stores 32767 for the first tap and adds the missing 1 to another tap (value q)."""
    p, q = np.mgrid[0:256, 0:256].astype(np.int64)
    assert np.array_equal((32767 * p + q + 16384) >> 15, p)
    assert np.array_equal((32768 * p + 16384) >> 15, p)
    a, b = np.mgrid[0:32, 0:32]
    assert np.all(32 * (32 - a) * (32 - b) + 32 * a * (32 - b) + 32 * (32 - a) * b + 32 * a * b == 32768)
    assert np.count_nonzero(32 * (32 - a) * (32 - b) > 32767) == 1


def test_row_range_and_counts():
    src, m1, m2 = hand_maps()
    full = R.rectify(src, m1, m2)
    assert np.array_equal(R.rectify(src, m1, m2, rows=(3, 9)), full[3:9])
    n_out, n_part, n_in = R.classify(R.fixed_point(m1, m2, (SRC_COLS, SRC_ROWS)), (SRC_COLS, SRC_ROWS))
    assert n_out > 0 and n_part > 0 and n_in > 0 and n_out + n_part + n_in == m1.size


def test_arducam_maps_stay_inside_the_source():
    A = R.arducam()
    for name, lo, hi in (("left", 19.29, 638.73), ("right", -0.002, 621.06)):
        c = A[name]
        m1, m2 = R.rectify_maps(c["K"], c["D"], c["R"], c["P"], (A["width"], A["height"]))
        assert abs(float(m1.min()) - lo) < 0.01 and abs(float(m1.max()) - hi) < 0.01
        assert R.classify(R.fixed_point(m1, m2, (640, 480)), (640, 480)) == (0, 0, 640 * 480)
    S = R.synthetic_camera()
    m1, m2 = R.rectify_maps(S["K"], S["D"], S["R"], S["P"], S["size"])
    assert min(R.classify(R.fixed_point(m1, m2, S["src_size"]), S["src_size"])) > 0
