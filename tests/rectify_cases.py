"""Inputs shared by the rectification tests (tests/test_rectify_ref.py, test_rectify_core.py, test_gpu_rectify.py)."""
import numpy as np

SRC_ROWS, SRC_COLS = 6, 8

# (x, y) map values on the 8 x 6 source beyond the identity grid: half-pixel shifts, the float ties of the
# 1/32 grid (k + 1/64 rounds to even), -0.5, each "fully outside" condition at equality and one step short of
# it, taps outside on each side and at the corners, and values with no int conversion.
SPECIAL = [(0.5, 0.0), (0.0, 0.5), (3.5, 2.5), (2 + 1 / 64, 1.0), (2 + 3 / 64, 1.0), (10 + 1 / 64, 1.0),
           (10 + 3 / 64, 1.0), (1.0, 2 + 1 / 64), (1.0, 2 + 3 / 64), (-0.5, 0.0), (0.0, -0.5), (-0.5, -0.5),
           (8.0, 2.0), (8 - 1 / 32, 2.0), (-1 - 1 / 32, 2.0), (-1.0, 2.0), (3.0, 6.0), (3.0, 6 - 1 / 32),
           (3.0, -1 - 1 / 32), (3.0, -1.0), (7.5, 2.25), (3.25, 5.5), (7.5, 5.5), (-0.5, 5.5), (7.5, -0.5),
           (7.0, 5.0), (6.96875, 4.96875), (np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf),
           (1e30, 1.0), (1.0, -1e30), (7e7, 1.0), (6e7, 1.0), (1.0, -6e7), (-67108864.0, 1.0), (1000.0, 1.0),
           (-1000.0, -1000.0), (1023.99, 2.0), (-1024.5, 2.0)]


def hand_maps():
    """(src, map1, map2): an 8 x 6 source of distinct non-zero bytes; maps of 8 columns whose first 6 rows are
    the identity (K = P, D = 0, R = I) and whose further rows hold SPECIAL, padded with (0, 0)."""
    src = (np.arange(SRC_ROWS * SRC_COLS, dtype=np.int64) * 5 + 9).astype(np.uint8).reshape(SRC_ROWS, SRC_COLS)
    y, x = np.mgrid[0:SRC_ROWS, 0:SRC_COLS].astype(np.float32)
    pts = SPECIAL + [(0.0, 0.0)] * (-len(SPECIAL) % SRC_COLS)
    sp = np.asarray(pts, np.float32).reshape(-1, SRC_COLS, 2)
    return src, np.concatenate([x, sp[..., 0]]), np.concatenate([y, sp[..., 1]])


def random_maps(rng, rows, cols, src_rows, src_cols):
    """Float maps on the 1/64 grid (so that ties of the 1/32 grid occur) from two pixels outside the source on
    each side: fully-outside, partly-outside and inside pixels."""
    m1 = rng.integers(-2 * 64, (src_cols + 1) * 64, (rows, cols)).astype(np.float32) / np.float32(64)
    m2 = rng.integers(-2 * 64, (src_rows + 1) * 64, (rows, cols)).astype(np.float32) / np.float32(64)
    return m1, m2
