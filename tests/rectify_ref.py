"""Stereo rectification a second way, in NumPy / Python (float64, float32 and integer arithmetic), sharing no
code with the library: cv::initUndistortRectifyMap(K, D, R, P, size, CV_32F), cv::remap's float-to-fixed-point
conversion, its 8-bit bilinear blend with BORDER_CONSTANT 0, the row crop and cvtColor's gray
(Examples/Stereo/arducam_images.cpp:123-133, 229-275 and Tracking.cc:183-208 of the reference; OpenCV 4.5.x's
calib3d / imgproc as DESIGN.md section 30 records them). Every operation is one IEEE operation of the stated
type, in the stated order, so the library must equal it bit for bit. The maps are evaluated for all rows at once
and serially along the columns (the running sums); the blend gathers from a zero-padded copy of the source."""
import json
import os

import numpy as np

from sensor_ref import GRAY_SHIFT14, GRAY_SHIFT15, gray  # noqa: F401  (gray rule 1, held by test_sensor_ref.py)

ENTRY_DTYPE = np.dtype([("ix", "<i2"), ("iy", "<i2"), ("alpha", "<u2"), ("outside", "<u2")])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arducam_stereo.json")


def arducam():
    """The reference's Examples/Stereo/arducam.yaml numbers: {"width", "height", "left": {K, D, R, P}, "right"}."""
    with open(GOLDEN) as f:
        return json.load(f)


def synthetic_camera():
    """A calibration whose rectified view leaves the source: a 7 degree roll, a 4 degree pan, k1 = 0.35 and a
    new focal length well under the old one, for a 600 x 440 source and a 640 x 480 destination."""
    a, b = np.deg2rad(7.0), np.deg2rad(4.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[np.cos(b), 0.0, np.sin(b)], [0.0, 1.0, 0.0], [-np.sin(b), 0.0, np.cos(b)]])
    return dict(K=[[410.5, 0.0, 301.25], [0.0, 409.75, 218.5], [0.0, 0.0, 1.0]], D=[0.35, -0.08, 0.0015, -0.002, 0.01],
                R=(rz @ ry).tolist(), P=[[300.0, 0.0, 322.0, 0.0], [0.0, 300.0, 237.0, 0.0], [0.0, 0.0, 1.0, 0.0]],
                size=(640, 480), src_size=(600, 440))


def inverse_of_product(P3, R):
    """inv(P3 * R) as a list of 9 Python floats (IEEE doubles): the product's sums left to right, then the
    cofactors over the determinant."""
    A = [[float(v) for v in row] for row in np.asarray(P3, np.float64).reshape(3, 3)]
    B = [[float(v) for v in row] for row in np.asarray(R, np.float64).reshape(3, 3)]
    m = [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]
    det = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    d = 1.0 / det
    return [(m[1][1] * m[2][2] - m[1][2] * m[2][1]) * d, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * d,
            (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * d, (m[1][2] * m[2][0] - m[1][0] * m[2][2]) * d,
            (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * d, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * d,
            (m[1][0] * m[2][1] - m[1][1] * m[2][0]) * d, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * d,
            (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * d]


def rectify_maps(K, D, R, P, size):
    """(map1, map2), float32 (rows, cols), for size = (cols, rows). D: 4 or 5 entries; R None: the identity."""
    cols, rows = size
    K = np.asarray(K, np.float64).reshape(3, 3)
    P3 = np.asarray(P, np.float64).reshape(3, -1)[:, :3]
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    d = [np.float64(v) for v in np.asarray(D, np.float64).reshape(-1)]
    assert len(d) in (4, 5)
    k1, k2, p1, p2 = d[:4]
    k3 = d[4] if len(d) == 5 else np.float64(0.0)
    zero, one, two = np.float64(0.0), np.float64(1.0), np.float64(2.0)
    fx, fy, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ir = [np.float64(v) for v in inverse_of_product(P3, R)]
    i = np.arange(rows, dtype=np.float64)
    X, Y, W = i * ir[1] + ir[2], i * ir[4] + ir[5], i * ir[7] + ir[8]
    map1 = np.empty((rows, cols), np.float32)
    map2 = np.empty((rows, cols), np.float32)
    with np.errstate(all="ignore"):
        for j in range(cols):
            w = one / W
            x, y = X * w, Y * w
            x2, y2 = x * x, y * y
            r2, xy2 = x2 + y2, two * x * y
            kr = (one + ((k3 * r2 + k2) * r2 + k1) * r2) / (one + ((zero * r2 + zero) * r2 + zero) * r2)
            xd = x * kr + p1 * xy2 + p2 * (r2 + two * x2) + zero * r2 + zero * r2 * r2
            yd = y * kr + p1 * (r2 + two * y2) + p2 * xy2 + zero * r2 + zero * r2 * r2
            map1[:, j] = (fx * one * xd + u0).astype(np.float32)
            map2[:, j] = (fy * one * yd + v0).astype(np.float32)
            X, Y, W = X + ir[0], Y + ir[3], W + ir[6]
    return map1, map2


def fixed_point(map1, map2, src_size):
    """The entries remap derives from float maps for a source of src_size = (cols, rows): ENTRY_DTYPE, the maps'
    shape. A product that is not finite or lies beyond int is the constant, with zero fields."""
    scols, srows = src_size
    out = np.zeros(np.shape(map1), ENTRY_DTYPE)
    with np.errstate(all="ignore"):
        px = np.asarray(map1, np.float32) * np.float32(32.0)
        py = np.asarray(map2, np.float32) * np.float32(32.0)
        assert px.dtype == np.float32
        lo, hi = np.float32(-2.0 ** 31), np.float32(2.0 ** 31)  # NaN fails every comparison
        ok = (px >= lo) & (px < hi) & (py >= lo) & (py < hi)
        sx = np.where(ok, np.rint(px.astype(np.float64)), 0).astype(np.int64)  # rint: half to even
        sy = np.where(ok, np.rint(py.astype(np.float64)), 0).astype(np.int64)
    ix = np.clip(sx >> 5, -32768, 32767)
    iy = np.clip(sy >> 5, -32768, 32767)
    outside = ~ok | (ix >= scols) | (ix + 1 < 0) | (iy >= srows) | (iy + 1 < 0)
    out["ix"] = np.where(ok, ix, 0)
    out["iy"] = np.where(ok, iy, 0)
    out["alpha"] = np.where(ok, (sy & 31) * 32 + (sx & 31), 0)
    out["outside"] = outside
    return out


def remap(src, entries):
    """src (rows, cols) or (rows, cols, C) uint8 through `entries`: the same number of channels out."""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    img = src.reshape(src.shape[0], src.shape[1], -1).astype(np.int64)
    rows, cols, _ = img.shape
    assert rows <= 32766 and cols <= 32766
    pad = np.zeros((rows + 2, cols + 2, img.shape[2]), np.int64)  # taps at -1 and at rows / cols read 0
    pad[1:-1, 1:-1] = img
    inside = entries["outside"] == 0
    x = np.where(inside, entries["ix"].astype(np.int64), 0) + 1
    y = np.where(inside, entries["iy"].astype(np.int64), 0) + 1
    a = (entries["alpha"].astype(np.int64) & 31)[..., None]
    b = (entries["alpha"].astype(np.int64) >> 5)[..., None]
    acc = (32 * (32 - a) * (32 - b) * pad[y, x] + 32 * a * (32 - b) * pad[y, x + 1] +
           32 * (32 - a) * b * pad[y + 1, x] + 32 * a * b * pad[y + 1, x + 1] + (1 << 14)) >> 15
    acc = np.where(inside[..., None], acc, 0)
    assert acc.min() >= 0 and acc.max() <= 255
    out = acc.astype(np.uint8)
    return out[..., 0] if src.ndim == 2 else out


def rectify(src, map1, map2, rows=(0, None), gray_out=False, rgb=True, mode=GRAY_SHIFT15):
    """remap on the image as it comes, the crop to destination rows [rows[0], rows[1]), then gray when the
    image has 3 or 4 channels and gray_out is set."""
    src = np.asarray(src)
    ent = fixed_point(map1, map2, (src.shape[1], src.shape[0]))
    out = remap(src, ent)[rows[0]:rows[1]]
    if gray_out and src.ndim == 3 and src.shape[2] in (3, 4):
        return gray(out, rgb, mode)
    return out


def classify(entries, src_size):
    """(fully outside, partly outside, inside) pixel counts of a plan."""
    scols, srows = src_size
    out = entries["outside"] != 0
    ix, iy = entries["ix"].astype(np.int64), entries["iy"].astype(np.int64)
    part = ~out & ((ix < 0) | (ix + 1 >= scols) | (iy < 0) | (iy + 1 >= srows))
    return int(out.sum()), int(part.sum()), int((~out & ~part).sum())
