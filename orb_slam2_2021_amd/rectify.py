"""Stereo rectification of raw camera pairs -- host mirror of include/orbfe_rectify.h over liborbfe.so.

The reference's stereo programs (Examples/Stereo/arducam_images.cpp:119-153, 229-275) build four float maps
with cv::initUndistortRectifyMap once and then, per frame, cut the side-by-side image in two, cv::remap each
half, crop and (Tracking.cc:183-208) convert both to gray. StereoRectifier holds the maps as a fixed-point
plan on the device; rectify_batch and ORBextractor.rectified_stereo_frame run the per-frame part in one
kernel launch.
"""
from __future__ import annotations

from ctypes import byref, c_size_t, c_void_p
from typing import Optional, Tuple

import numpy as np

from . import _lib as L


def rectify_maps_host(K, D, R, P, size: Tuple[int, int]) -> Tuple[np.ndarray, np.ndarray]:
    """cv::initUndistortRectifyMap(K, D, R, P, size, CV_32F): K 3 x 3, D with 4 or 5 entries (k1 k2 p1 p2[ k3]),
    R 3 x 3 or None (identity), P 3 x 3 or 3 x 4 (its left 3 x 3 is used), size = (cols, rows) as cv::Size.
    Returns (map1, map2), float32 (rows, cols). Host only."""
    cols, rows = int(size[0]), int(size[1])
    k = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
    d = np.ascontiguousarray(np.asarray(D, np.float64).reshape(-1))
    p = np.ascontiguousarray(np.asarray(P, np.float64).reshape(3, -1)[:, :3])
    r = None if R is None or np.size(R) == 0 else np.ascontiguousarray(np.asarray(R, np.float64).reshape(3, 3))
    m1 = np.zeros((max(rows, 0), max(cols, 0)), np.float32)
    m2 = np.zeros_like(m1)
    L.check(L.lib().orbfe_rectify_maps_host(L.ptr(k), L.ptr(d), len(d), L.ptr(r), L.ptr(p), rows, cols, L.ptr(m1),
                                            L.ptr(m2)), "orbfe_rectify_maps_host")
    return m1, m2


def _maps(map1, map2):
    m1 = np.ascontiguousarray(np.asarray(map1, np.float32))
    m2 = np.ascontiguousarray(np.asarray(map2, np.float32))
    if m1.ndim != 2 or m1.shape != m2.shape:
        raise ValueError("map1 and map2 are float32 (rows, cols) arrays of one shape")
    return m1, m2


def remap_host(src: np.ndarray, map1, map2, rows: Tuple[int, Optional[int]] = (0, None), gray_out: bool = False,
               rgb: bool = True, gray_mode: int = L.GRAY_SHIFT15) -> np.ndarray:
    """cv::remap(src, map1, map2, INTER_LINEAR, BORDER_CONSTANT 0), the crop to destination rows
    [rows[0], rows[1]) and, with gray_out, cvtColor(*2GRAY) of a 3- or 4-channel result. src is uint8
    (rows, cols) or (rows, cols, 1 | 3 | 4) with any row stride. Host only."""
    img = np.asarray(src)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3, 4)):
        raise ValueError("a CV_8UC1, CV_8UC3 or CV_8UC4 image is expected")
    ch = 1 if img.ndim == 2 else img.shape[2]
    if img.strides[-1] != 1 or (img.ndim == 3 and img.strides[1] != ch) or img.strides[0] < 0:
        img = np.ascontiguousarray(img)
    m1, m2 = _maps(map1, map2)
    row0, row1 = int(rows[0]), m1.shape[0] if rows[1] is None else int(rows[1])
    oc = 1 if (gray_out and ch != 1) else ch
    out = np.zeros((max(row1 - row0, 0), m1.shape[1]) + ((oc,) if oc != 1 else ()), np.uint8)
    L.check(L.lib().orbfe_remap_host(c_void_p(img.ctypes.data), img.shape[0], img.shape[1], c_size_t(img.strides[0]),
                                     ch, L.ptr(m1), L.ptr(m2), c_size_t(m1.strides[0]), m1.shape[0], m1.shape[1],
                                     row0, row1, int(bool(rgb)), int(gray_mode), int(bool(gray_out)), L.ptr(out),
                                     c_size_t(m1.shape[1] * oc)), "orbfe_remap_host")
    return out


def rectify_entries_host(map1, map2, src_size: Tuple[int, int]) -> np.ndarray:
    """The fixed-point entries (RECTIFY_ENTRY_DTYPE, shape of the maps) cv::remap derives from float maps for a
    source of src_size = (cols, rows). Host only."""
    m1, m2 = _maps(map1, map2)
    out = np.zeros(m1.shape, L.RECTIFY_ENTRY_DTYPE)
    L.check(L.lib().orbfe_rectify_entries_host(L.ptr(m1), L.ptr(m2), m1.shape[0], m1.shape[1], int(src_size[1]),
                                               int(src_size[0]), L.ptr(out)), "orbfe_rectify_entries_host")
    return out


class StereoRectifier:
    """A stereo calibration's rectification plan on the extractor's device: built once, where the reference
    calls rectification() (arducam_images.cpp:229-275), and shared by every frame and batch.

    left / right: dicts of K, D, R (or None) and P as the settings file holds them. size = (cols, rows) of the
    rectified image, src_size = (cols, rows) of each raw image (default: size)."""

    def __init__(self, extractor, left: dict, right: dict, size: Tuple[int, int],
                 src_size: Optional[Tuple[int, int]] = None):
        ml = rectify_maps_host(left["K"], left["D"], left.get("R"), left["P"], size)
        mr = rectify_maps_host(right["K"], right["D"], right.get("R"), right["P"], size)
        self._init(extractor, ml + mr, src_size if src_size is not None else size)

    @classmethod
    def from_maps(cls, extractor, map1_l, map2_l, map1_r, map2_r, src_size: Tuple[int, int]) -> "StereoRectifier":
        """From the caller's own CV_32F maps (e.g. their OpenCV's initUndistortRectifyMap)."""
        self = cls.__new__(cls)
        self._init(extractor, _maps(map1_l, map2_l) + _maps(map1_r, map2_r), src_size)
        return self

    def _init(self, extractor, maps, src_size) -> None:
        self._plan = None
        if any(m.shape != maps[0].shape for m in maps):
            raise ValueError("the four maps have one shape")
        self._lib = L.lib()
        self.extractor = extractor
        self.maps = tuple(maps)  # (map1_l, map2_l, map1_r, map2_r), float32 (rows, cols)
        self.rows, self.cols = maps[0].shape
        self.src_cols, self.src_rows = int(src_size[0]), int(src_size[1])
        plan = c_void_p()
        L.check(self._lib.orbfe_rectify_plan_create(extractor._h, *[L.ptr(m) for m in maps], self.rows, self.cols,
                                                    self.src_rows, self.src_cols, byref(plan)),
                "orbfe_rectify_plan_create")
        self._plan = plan

    def close(self) -> None:
        if getattr(self, "_plan", None):
            self._lib.orbfe_rectify_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def entries(self, right: bool = False) -> np.ndarray:
        """The plan's fixed-point entries of one camera read back (RECTIFY_ENTRY_DTYPE, (rows, cols))."""
        out = np.zeros((self.rows, self.cols), L.RECTIFY_ENTRY_DTYPE)
        L.check(self._lib.orbfe_rectify_plan_read(self._plan, int(bool(right)), L.ptr(out)), "orbfe_rectify_plan_read")
        return out

    def rectify_batch(self, src, dst, rows: Tuple[int, Optional[int]] = (0, None), gray_out: bool = True,
                      rgb: bool = True, gray_mode: int = L.GRAY_SHIFT15, stream: Optional[int] = None) -> None:
        """remap + crop + gray on device tensors. src: a batch of side-by-side images, (n, src_rows, 2 * src_cols)
        or (n, src_rows, 2 * src_cols, 1 | 3 | 4) uint8, or a pair (lefts, rights) of (n, src_rows, src_cols[, ch])
        tensors with the same strides; pixels contiguous within a row, any row and image strides.
        dst: (2n, row1 - row0, cols) uint8, or (2n, row1 - row0, cols, channels) for colour out (gray_out False):
        the lefts, then the rights, as extract_batch_device and compute_stereo_matches_batch_device take them.
        Async on `stream` (default: the handle's)."""
        if isinstance(src, (tuple, list)):
            src_left, src_right = src
        else:
            if src.dim() not in (3, 4) or src.shape[2] != 2 * self.src_cols:
                raise ValueError("rectify_batch: a side-by-side src is (n, src_rows, 2 * src_cols[, channels])")
            src_left, src_right = src[:, :, :self.src_cols], src[:, :, self.src_cols:]
        if src_left.dim() not in (3, 4) or src_left.shape != src_right.shape or \
                tuple(src_left.stride()) != tuple(src_right.stride()):
            raise ValueError("rectify_batch: lefts / rights (n, rows, cols[, channels]) of one shape and stride")
        ch = 1 if src_left.dim() == 3 else src_left.shape[3]
        n = src_left.shape[0]
        if ch not in (1, 3, 4) or tuple(src_left.shape[1:3]) != (self.src_rows, self.src_cols):
            raise ValueError("rectify_batch: the sources have the plan's source size and 1, 3 or 4 channels")
        if src_left.stride(2) != ch or (src_left.dim() == 4 and src_left.stride(3) != 1):
            raise ValueError("rectify_batch: pixels must be contiguous within a row")
        row0, row1 = int(rows[0]), self.rows if rows[1] is None else int(rows[1])
        oc = 1 if (gray_out or ch == 1) else ch
        want = (2 * n, row1 - row0, self.cols) + ((oc,) if oc != 1 else ())
        if tuple(dst.shape) != want and not (oc == 1 and tuple(dst.shape) == want + (1,)):
            raise ValueError("rectify_batch: dst is %r" % (want,))
        if dst.stride(2) != oc or (dst.dim() == 4 and dst.stride(3) != 1):
            raise ValueError("rectify_batch: pixels must be contiguous within a row")
        if src_left.element_size() != 1 or dst.element_size() != 1:
            raise ValueError("rectify_batch: uint8 tensors")
        L.check(self._lib.orbfe_rectify_batch_device(
            self.extractor._h, self._plan, n, c_void_p(src_left.data_ptr()), c_void_p(src_right.data_ptr()),
            c_size_t(src_left.stride(0)), c_size_t(src_left.stride(1)), ch, int(bool(rgb)), int(gray_mode),
            int(bool(gray_out)), row0, row1, c_void_p(dst.data_ptr()), c_size_t(dst.stride(0)),
            c_size_t(dst.stride(1)), c_void_p(stream or 0)), "orbfe_rectify_batch_device")
