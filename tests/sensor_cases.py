"""The cameras, keypoints and depth maps the sensor-Frame tests share (tests/test_frame_core.py on the host
entry points, tests/test_gpu_frame_finish.py on the kernel): built once, never modified."""
import numpy as np

import sensor_ref as R

ROWS, COLS = 480, 640

CAMERAS = {
    "fr1": R.camera(**R.FR1),
    "fr1_4": R.camera(**dict(R.FR1, dist=R.FR1["dist"][:4])),
    # strong barrel distortion: 1 + k1 r^2 < 0 towards the corners (the icdist < 0 exit), not at the centre
    "k1_neg": R.camera(**dict(R.FR1, dist=(-1.5, 0.0, 0.0, 0.0, 0.0))),
    # the early-outs: k1 == 0 / -0 with every other coefficient set
    "k1_zero": R.camera(**dict(R.FR1, dist=(0.0, -0.953104, -0.005358, 0.002628, 1.163314))),
    "k1_negzero": R.camera(**dict(R.FR1, dist=(-0.0, -0.953104, -0.005358, 0.002628, 1.163314))),
}

LATTICE = R.lattice_keys(ROWS, COLS)

# 40 x 30 depth maps and the keys that sample their edge values
MAP_ROWS, MAP_COLS = 30, 40


def edge_keys():
    k = np.zeros(8, R.KEYPOINT_DTYPE)
    xy = [(MAP_COLS - 0.4, MAP_ROWS - 0.4), (0.9, 0.9), (10.8, 5.9), (1.0, 0.0), (2.5, 0.5), (3.0, 1.0),
          (4.2, 1.7), (20.0, 15.0)]
    for i, (x, y) in enumerate(xy):
        k[i] = (x, y, 31.0, 10.0 * i, 20.0 + i, i % 8, i)
    return k


EDGE_KEYS = edge_keys()


def depth_u16():
    rng = np.random.default_rng(11)
    m = rng.integers(300, 40000, (MAP_ROWS, MAP_COLS)).astype(np.uint16)
    m[0, 0], m[0, 1], m[0, 2] = 0, 1, 65535
    m[MAP_ROWS - 1, MAP_COLS - 1] = 65535
    m[5, 10] = 12345
    return m


def depth_f32():
    rng = np.random.default_rng(12)
    m = rng.uniform(0.3, 8.0, (MAP_ROWS, MAP_COLS)).astype(np.float32)
    m[0, 0], m[0, 1], m[0, 2] = 0.0, -1.0, np.nan
    m[1, 3], m[1, 4] = np.inf, -0.0
    m[5, 10] = 2.5
    return m


# (name, map, factor)
DEPTH_CASES = [
    ("u16_5000", depth_u16(), np.float32(1.0) / np.float32(5000.0)),
    ("f32_1", depth_f32(), np.float32(1.0)),
    ("f32_half", depth_f32(), np.float32(0.5)),
]

# the camera of the 40 x 30 maps: fr1 scaled to that image
MAP_CAM = R.scaled(CAMERAS["fr1"], 1.0 / 16.0)


def padded(m, extra):
    """m in a buffer whose rows are `extra` elements longer: (the contiguous buffer, the pitch in bytes)."""
    buf = np.full((m.shape[0], m.shape[1] + extra), 0x7f, m.dtype)
    buf[:, :m.shape[1]] = m
    return buf, buf.strides[0]
