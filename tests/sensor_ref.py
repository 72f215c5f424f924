"""The monocular and RGB-D Frames' per-frame rules a second way, in NumPy (float64 / float32 / integer
arithmetic), sharing no code with the library: cvtColor's 8-bit gray in its two table generations,
convertTo's depth value, cv::undistortPoints(src, dst, K, D, noArray(), K), Frame::UndistortKeyPoints,
Frame::ComputeImageBounds and Frame::ComputeStereoFromRGBD (Tracking.cc:226-283, Frame.cc:456-520,
702-723 of the reference; OpenCV 4.5.x's calib3d / imgproc as DESIGN.md records them). Every operation
is one IEEE operation of the stated type, in the stated order, so the library must equal it bit for bit."""
import numpy as np

GRAY_SHIFT15, GRAY_SHIFT14 = 0, 1
DEPTH_U16, DEPTH_F32 = 0, 1

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

# TUM RGB-D freiburg1 (the reference's Examples/RGB-D/TUM1.yaml values, as the issue lists them)
FR1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989,
           dist=(0.262383, -0.953104, -0.005358, 0.002628, 1.163314), bf=40.0)


def camera(fx, fy, cx, cy, dist, bf):
    """The camera as the Frame holds it: float32 K, float32 mDistCoef (4 or 5 entries), float32 mbf."""
    return dict(fx=np.float32(fx), fy=np.float32(fy), cx=np.float32(cx), cy=np.float32(cy),
                dist=np.asarray(dist, np.float32), bf=np.float32(bf))


def scaled(cam, s):
    """A camera for an image s times the size (float32 products), distortion unchanged."""
    c = camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["dist"], cam["bf"])
    for f in ("fx", "fy", "cx", "cy"):
        c[f] = np.float32(c[f] * np.float32(s))
    return c


def gray(img, rgb, mode):
    """(rows, cols, 3 or 4) uint8 -> (rows, cols) uint8; channel 0 is R when rgb else B; alpha ignored."""
    a = np.asarray(img).astype(np.int32)  # 255 * 32768 + 16384 < 2^31
    r, g, b = (a[..., 0], a[..., 1], a[..., 2]) if rgb else (a[..., 2], a[..., 1], a[..., 0])
    if mode == GRAY_SHIFT15:
        v = (9798 * r + 19235 * g + 3735 * b + (1 << 14)) >> 15
    elif mode == GRAY_SHIFT14:
        v = (4899 * r + 9617 * g + 1868 * b + (1 << 13)) >> 14
    else:
        raise ValueError(mode)
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def distorted(cam):
    return not (cam["dist"][0] == np.float32(0.0))  # -0.0 == 0.0


def undistort_point(cam, px, py, trace=None):
    """One point through cvUndistortPointsInternal with R = I, P = K: python floats are IEEE doubles and
    each operator below is one correctly rounded operation. trace (a list) receives True when the
    icdist < 0 exit is taken."""
    fx, fy, cx, cy = (float(cam[f]) for f in ("fx", "fy", "cx", "cy"))
    k = [0.0] * 12
    for i, d in enumerate(cam["dist"]):
        k[i] = float(d)
    ifx = 1.0 / fx
    ify = 1.0 / fy
    x = float(np.float32(px))
    y = float(np.float32(py))
    u, v = x, y
    x = (x - cx) * ifx
    y = (y - cy) * ify
    x0, y0 = x, y
    bailed = False
    with np.errstate(all="ignore"):
        for _ in range(5):
            r2 = x * x + y * y
            num = np.float64(1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
            den = np.float64(1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            icdist = float(num / den)  # numpy: IEEE division by zero
            if icdist < 0:
                x = (u - cx) * ifx
                y = (v - cy) * ify
                bailed = True
                break
            dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = (x0 - dx) * icdist
            y = (y0 - dy) * icdist
        xx = fx * x + 0.0 * y + cx
        yy = 0.0 * x + fy * y + cy
        ww = 1.0 / (0.0 * x + 0.0 * y + 1.0)
        out = np.float32(xx * ww), np.float32(yy * ww)
    if trace is not None:
        trace.append(bailed)
    return out


def undistort_keys(cam, keys, trace=None):
    keys = np.asarray(keys, KEYPOINT_DTYPE)
    out = keys.copy()
    if not distorted(cam):
        return out
    for i in range(len(keys)):
        out["x"][i], out["y"][i] = undistort_point(cam, keys["x"][i], keys["y"][i], trace)
    return out


def image_bounds(cam, rows, cols):
    """(mnMinX, mnMaxX, mnMinY, mnMaxY) as float32."""
    if not distorted(cam):
        return np.array([0, cols, 0, rows], np.float32)
    p = [undistort_point(cam, x, y) for x, y in ((0, 0), (cols, 0), (0, rows), (cols, rows))]
    return np.array([min(p[0][0], p[2][0]), max(p[1][0], p[3][0]),
                     min(p[0][1], p[1][1]), max(p[2][1], p[3][1])], np.float32)


def depth_value(raw, factor):
    """convertTo(CV_32F, factor) of one raw value where Tracking.cc:246 applies it."""
    f = np.float32(factor)
    converts = float(abs(np.float32(f - np.float32(1.0)))) > 1e-5 or raw.dtype != np.float32
    with np.errstate(all="ignore"):
        return np.float32(np.float32(raw) * f) if converts else np.float32(raw)


def stereo_from_depth(cam, keys, keys_un, depth_map, factor):
    """(mvuRight, mvDepth); depth_map None is the monocular Frame."""
    n = len(keys)
    ur = np.full(n, -1, np.float32)
    dep = np.full(n, -1, np.float32)
    if depth_map is None:
        return ur, dep
    for i in range(n):
        d = depth_value(depth_map[int(keys["y"][i]), int(keys["x"][i])], factor)
        if d > 0:
            dep[i] = d
            with np.errstate(all="ignore"):
                ur[i] = np.float32(keys_un["x"][i] - np.float32(cam["bf"] / d))
    return ur, dep


def lattice_keys(rows, cols, nx=9, ny=7, frac=True):
    """An nx x ny lattice over the image, fractional coordinates included, every field distinct."""
    k = np.zeros(nx * ny, KEYPOINT_DTYPE)
    i = 0
    for iy in range(ny):
        for ix in range(nx):
            x = ix * (cols - 1) / (nx - 1) + (0.37 * ((ix + iy) % 3) if frac and ix < nx - 1 else 0.0)
            y = iy * (rows - 1) / (ny - 1) + (0.61 * ((ix + 2 * iy) % 2) if frac and iy < ny - 1 else 0.0)
            k[i] = (x, y, 31.0 + i, 0.5 * i, 7.0 + i, i % 8, i - 3)
            i += 1
    return k


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
