"""ORBextractor on MI355X -- host mirror of include/ORBextractor.h over liborbfe.so.

Same constructor arguments, getters and call semantics as the reference class
(include/ORBextractor.h:56-100, src/ORBextractor.cc:413-473, 1041-1103): calling the extractor on
an 8-bit grayscale image returns its keypoints (cv::KeyPoint fields, level order) and the N x 32
descriptor matrix. All work runs in the HIP kernels of liborbfe.so.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_int, c_size_t, c_void_p
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

KeyPoints = np.ndarray  # structured, dtype KEYPOINT_DTYPE


class ORBextractor:
    HARRIS_SCORE = 0  # ORBextractor.h:51-54 (enum kept for API parity)
    FAST_SCORE = 1

    def __init__(self, nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int,
                 minThFAST: int, device: int = 0):
        self._lib = L.lib()
        h = c_void_p()
        L.check(self._lib.orbfe_extractor_create(int(nfeatures), float(scaleFactor), int(nlevels),
                                                 int(iniThFAST), int(minThFAST), int(device),
                                                 byref(h)), "orbfe_extractor_create")
        self._h = h
        self.nfeatures = int(nfeatures)
        self.scaleFactor = float(scaleFactor)
        self.nlevels = int(nlevels)
        self.iniThFAST = int(iniThFAST)
        self.minThFAST = int(minThFAST)
        self.device = int(device)
        n = self.nlevels
        self._scale = np.zeros(n, np.float32)
        self._inv = np.zeros(n, np.float32)
        self._s2 = np.zeros(n, np.float32)
        self._is2 = np.zeros(n, np.float32)
        self._fpl = np.zeros(n, np.int32)
        L.check(self._lib.orbfe_get_scale_tables(self._h, L.ptr(self._scale), L.ptr(self._inv),
                                                 L.ptr(self._s2), L.ptr(self._is2),
                                                 L.ptr(self._fpl)), "orbfe_get_scale_tables")
        self._last_shape: Optional[Tuple[int, int]] = None

    # ---- lifetime -------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_extractor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- getters (ORBextractor.h:70-98) ---------------------------------------------------
    def GetLevels(self) -> int:
        return self.nlevels

    def GetScaleFactor(self) -> float:
        return self.scaleFactor

    def GetScaleFactors(self) -> np.ndarray:
        return self._scale.copy()

    def GetInverseScaleFactors(self) -> np.ndarray:
        return self._inv.copy()

    def GetScaleSigmaSquares(self) -> np.ndarray:
        return self._s2.copy()

    def GetInverseScaleSigmaSquares(self) -> np.ndarray:
        return self._is2.copy()

    @property
    def mnFeaturesPerLevel(self) -> np.ndarray:
        return self._fpl.copy()

    def set_resize_mode(self, mode: int) -> None:
        L.check(self._lib.orbfe_extractor_set_resize_mode(self._h, int(mode)), "set_resize_mode")

    def max_keypoints(self, rows: int, cols: int) -> int:
        return L.check(self._lib.orbfe_max_keypoints(self._h, int(rows), int(cols)),
                       "orbfe_max_keypoints")

    # ---- operator() -----------------------------------------------------------------------
    def __call__(self, image: np.ndarray, mask=None) -> Tuple[KeyPoints, Optional[np.ndarray]]:
        """operator()(image, mask, keypoints, descriptors). The mask is ignored, as in the
        reference (ORBextractor.h:65). Returns (keypoints, descriptors); descriptors is None when
        no keypoint was found (the reference releases the Mat, ORBextractor.cc:1062-1063)."""
        img = np.asarray(image)
        if img.size == 0:
            return np.zeros(0, L.KEYPOINT_DTYPE), None
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("ORBextractor expects a CV_8UC1 image")  # assert at :1048
        img = np.ascontiguousarray(img)
        rows, cols = img.shape
        cap = self.max_keypoints(rows, cols)
        kps = np.zeros(cap, L.KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = c_int()
        L.check(self._lib.orbfe_extract(self._h, L.ptr(img), rows, cols, c_size_t(img.strides[0]),
                                        L.ptr(kps), cap, L.ptr(desc), byref(n)), "orbfe_extract")
        self._last_shape = (rows, cols)
        k = n.value
        return kps[:k].copy(), (desc[:k].copy() if k else None)

    def extract_batch(self, images: Sequence[np.ndarray]) -> List[Tuple[KeyPoints, np.ndarray]]:
        """Independent operator() calls on same-shaped images in one launch sequence."""
        imgs = [np.ascontiguousarray(np.asarray(i, np.uint8)) for i in images]
        if not imgs:
            return []
        rows, cols = imgs[0].shape
        if any(i.shape != (rows, cols) for i in imgs):
            raise ValueError("extract_batch needs same-shaped images")
        cap = self.max_keypoints(rows, cols)
        B = len(imgs)
        kps = np.empty(B * cap, L.KEYPOINT_DTYPE)
        desc = np.empty((B * cap, 32), np.uint8)
        counts = np.zeros(B, np.int32)
        arr = (c_void_p * B)(*[i.ctypes.data for i in imgs])
        L.check(self._lib.orbfe_extract_batch(self._h, B, ctypes.cast(arr, c_void_p), rows, cols,
                                              c_size_t(cols), L.ptr(kps), L.ptr(desc), cap,
                                              L.ptr(counts)), "orbfe_extract_batch")
        self._last_shape = (rows, cols)
        out = []
        for b in range(B):
            k = int(counts[b])
            out.append((kps[b * cap:b * cap + k].copy(), desc[b * cap:b * cap + k].copy()))
        return out

    def extract_batch_device(self, n_images: int, d_imgs: int, image_stride: int, rows: int,
                             cols: int, pitch: int, d_kps: int, d_desc: int, cap: int,
                             d_counts: int, stream: Optional[int] = None) -> None:
        """Device-resident batch (all int arguments are device addresses); async on `stream`."""
        L.check(self._lib.orbfe_extract_batch_device(
            self._h, int(n_images), c_void_p(d_imgs), c_size_t(image_stride), int(rows), int(cols),
            c_size_t(pitch), c_void_p(d_kps), c_void_p(d_desc), int(cap), c_void_p(d_counts),
            c_void_p(stream or 0)), "orbfe_extract_batch_device")
        self._last_shape = (rows, cols)

    # ---- Frame::ComputeStereoMatches (src/Frame.cc:522-700) -------------------------------
    def compute_stereo_matches(self, kps_l: KeyPoints, desc_l: np.ndarray, kps_r: KeyPoints,
                               desc_r: np.ndarray, mbf: float, mb: float, right: "ORBextractor" = None,
                               image_left: int = 0, image_right: Optional[int] = None
                               ) -> Tuple[np.ndarray, np.ndarray]:
        """Frame::ComputeStereoMatches (Frame.cc:522-700): (mvuRight, mvDepth) of the left keypoints.
        The left pyramid is image `image_left` of this extractor's last call; the right pyramid is
        image `image_right` of `right`'s last call (default: this extractor, image 1 -- e.g. after
        extract_batch([left, right]); with a separate right extractor, its image 0).
        mb: the reference uses the Frame's mb before assigning it (Frame.cc:125 vs :149); pass
        mbf / fx, or 0 for an unbounded disparity range."""
        other = self if right is None else right
        if image_right is None:
            image_right = 1 if other is self else 0
        kl = np.ascontiguousarray(kps_l, L.KEYPOINT_DTYPE)
        kr = np.ascontiguousarray(kps_r, L.KEYPOINT_DTYPE)
        dl = np.ascontiguousarray(desc_l if desc_l is not None else np.zeros((0, 32)), np.uint8)
        dr = np.ascontiguousarray(desc_r if desc_r is not None else np.zeros((0, 32)), np.uint8)
        n = len(kl)
        ur = np.full(n, -1.0, np.float32)
        dep = np.full(n, -1.0, np.float32)
        L.check(self._lib.orbfe_compute_stereo_matches(
            self._h, int(image_left), other._h, int(image_right), L.ptr(kl), L.ptr(dl), n,
            L.ptr(kr), L.ptr(dr), len(kr), float(mbf), float(mb), L.ptr(ur), L.ptr(dep)),
            "orbfe_compute_stereo_matches")
        return ur, dep

    def stereo_frame(self, left: np.ndarray, right: np.ndarray, mbf: float, mb: float):
        """The stereo Frame constructor's hot path (Frame.cc:113-125): ExtractORB(0, left),
        ExtractORB(1, right), ComputeStereoMatches. Returns (kps_l, desc_l, kps_r, desc_r,
        u_right, depth)."""
        l = np.ascontiguousarray(np.asarray(left, np.uint8))
        r = np.ascontiguousarray(np.asarray(right, np.uint8))
        if l.shape != r.shape or l.ndim != 2:
            raise ValueError("stereo_frame needs two same-shaped CV_8UC1 images")
        rows, cols = l.shape
        if l.size == 0:
            e = np.zeros(0, L.KEYPOINT_DTYPE)
            return e, None, e.copy(), None, np.zeros(0, np.float32), np.zeros(0, np.float32)
        cap = self.max_keypoints(rows, cols)
        kl = np.zeros(cap, L.KEYPOINT_DTYPE)
        kr = np.zeros(cap, L.KEYPOINT_DTYPE)
        dl = np.zeros((cap, 32), np.uint8)
        dr = np.zeros((cap, 32), np.uint8)
        ur = np.zeros(cap, np.float32)
        dep = np.zeros(cap, np.float32)
        nl, nr = c_int(), c_int()
        L.check(self._lib.orbfe_stereo_frame(self._h, L.ptr(l), L.ptr(r), rows, cols, c_size_t(cols),
                                             float(mbf), float(mb), L.ptr(kl), L.ptr(dl), byref(nl),
                                             L.ptr(kr), L.ptr(dr), byref(nr), cap, L.ptr(ur),
                                             L.ptr(dep)), "orbfe_stereo_frame")
        self._last_shape = (rows, cols)
        a, b = nl.value, nr.value
        return (kl[:a].copy(), dl[:a].copy() if a else None, kr[:b].copy(),
                dr[:b].copy() if b else None, ur[:a].copy(), dep[:a].copy())

    def rectified_stereo_frame(self, left: np.ndarray, right: np.ndarray, rectifier, mbf: float, mb: float,
                               rgb: bool = True, gray_mode: int = L.GRAY_SHIFT15,
                               rows: Tuple[int, Optional[int]] = (0, None)):
        """The stereo Frame from a raw, distorted pair (arducam_images.cpp:119-153, Tracking.cc:183-208,
        Frame.cc:113-125): remap with `rectifier` (a rectify.StereoRectifier), crop to rectified rows
        [rows[0], rows[1]), gray, ExtractORB of both planes, ComputeStereoMatches. left / right: CV_8UC1,
        CV_8UC3 or CV_8UC4 of the rectifier's source size; the two halves of one side-by-side array go up in
        one copy. Returns what stereo_frame returns."""
        l, r = np.asarray(left), np.asarray(right)
        if l.dtype != np.uint8 or r.dtype != np.uint8 or l.shape != r.shape or l.ndim not in (2, 3) or \
                (l.ndim == 3 and l.shape[2] not in (1, 3, 4)):
            raise ValueError("rectified_stereo_frame needs two same-shaped CV_8UC1, CV_8UC3 or CV_8UC4 images")
        channels = 1 if l.ndim == 2 else l.shape[2]
        dense = (channels, 1) if l.ndim == 3 else (1,)
        if l.size and (l.strides[1:] != dense or r.strides != l.strides or l.strides[0] < l.shape[1] * channels):
            l, r = np.ascontiguousarray(l), np.ascontiguousarray(r)
        row0, row1 = int(rows[0]), rectifier.rows if rows[1] is None else int(rows[1])
        e = np.zeros(0, L.KEYPOINT_DTYPE)
        if l.size == 0 or row1 == row0:
            return e, None, e.copy(), None, np.zeros(0, np.float32), np.zeros(0, np.float32)
        cap = self.max_keypoints(max(row1 - row0, 1), rectifier.cols)
        kl = np.zeros(cap, L.KEYPOINT_DTYPE)
        kr = np.zeros(cap, L.KEYPOINT_DTYPE)
        dl = np.zeros((cap, 32), np.uint8)
        dr = np.zeros((cap, 32), np.uint8)
        ur = np.zeros(cap, np.float32)
        dep = np.zeros(cap, np.float32)
        nl, nr = c_int(), c_int()
        L.check(self._lib.orbfe_rectified_stereo_frame(
            self._h, rectifier._plan, c_void_p(l.ctypes.data), c_void_p(r.ctypes.data), l.shape[0], l.shape[1],
            c_size_t(l.strides[0]), channels, int(bool(rgb)), int(gray_mode), row0, row1, float(mbf), float(mb),
            L.ptr(kl), L.ptr(dl), byref(nl), L.ptr(kr), L.ptr(dr), byref(nr), cap, L.ptr(ur), L.ptr(dep)),
            "orbfe_rectified_stereo_frame")
        self._last_shape = (row1 - row0, rectifier.cols)
        a, b = nl.value, nr.value
        return (kl[:a].copy(), dl[:a].copy() if a else None, kr[:b].copy(),
                dr[:b].copy() if b else None, ur[:a].copy(), dep[:a].copy())

    # ---- the monocular and RGB-D Frames (src/Frame.cc:154-277; include/orbfe_frame.h) --------
    def _sensor_frame(self, image, camera, depth_map, depth_factor, rgb, gray_mode):
        from .frames import Frame
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3, 4)):
            raise ValueError("a CV_8UC1, CV_8UC3 or CV_8UC4 image is expected")  # Tracking.cc:229-244
        img = np.ascontiguousarray(img)
        rows, cols = img.shape[:2]
        channels = 1 if img.ndim == 2 else img.shape[2]
        cam = camera if isinstance(camera, L.camera) else L.make_camera(**camera)
        bounds = np.zeros(4, np.float32)
        L.check(self._lib.orbfe_image_bounds(byref(cam), rows, cols, L.ptr(bounds)), "orbfe_image_bounds")
        cap = self.max_keypoints(rows, cols) if img.size else 1
        kps = np.zeros(cap, L.KEYPOINT_DTYPE)
        un = np.zeros(cap, L.KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        ur = np.zeros(cap, np.float32)
        dep = np.zeros(cap, np.float32)
        n = c_int()
        step = c_size_t(img.strides[0] if img.size else cols * channels)
        if depth_map is None:
            L.check(self._lib.orbfe_mono_frame(self._h, L.ptr(img), rows, cols, step, channels, int(bool(rgb)),
                                               int(gray_mode), byref(cam), L.ptr(kps), L.ptr(desc), byref(n), cap,
                                               L.ptr(un), L.ptr(ur), L.ptr(dep)), "orbfe_mono_frame")
        else:
            dm = np.asarray(depth_map)
            if dm.dtype not in (np.uint16, np.float32) or dm.shape != (rows, cols):
                raise ValueError("the depth map is uint16 or float32 and has the image's shape")
            dm = np.ascontiguousarray(dm)
            dtype = L.DEPTH_U16 if dm.dtype == np.uint16 else L.DEPTH_F32
            L.check(self._lib.orbfe_rgbd_frame(self._h, L.ptr(img), rows, cols, step, channels, int(bool(rgb)),
                                               int(gray_mode), L.ptr(dm), c_size_t(dm.strides[0]), dtype,
                                               float(depth_factor), byref(cam), L.ptr(kps), L.ptr(desc), byref(n),
                                               cap, L.ptr(un), L.ptr(ur), L.ptr(dep)), "orbfe_rgbd_frame")
        if img.size:
            self._last_shape = (rows, cols)
        k = n.value
        return Frame(keys_un=un[:k].copy(), descriptors=desc[:k].copy(), u_right=ur[:k].copy(),
                     mp_state=np.zeros(k, np.uint8), scale_factors=self._scale.copy(), level_sigma2=self._s2.copy(),
                     min_x=float(bounds[0]), max_x=float(bounds[1]), min_y=float(bounds[2]), max_y=float(bounds[3]),
                     fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, bf=cam.bf, keys=kps[:k].copy(),
                     depth=dep[:k].copy())

    def mono_frame(self, image: np.ndarray, camera, rgb: bool = True, gray_mode: int = L.GRAY_SHIFT15):
        """The monocular Frame (Frame.cc:216-277 behind Tracking::GrabImageMonocular's cvtColor): `image` is
        CV_8UC1, or CV_8UC3 / CV_8UC4 with channel 0 = R when `rgb` (mbRGB) else B. `camera` is an
        _lib.camera or a dict of fx, fy, cx, cy, dist, bf. Returns a frames.Frame with keys (mvKeys),
        keys_un, the image bounds and grid inverses, and u_right = depth = -1."""
        return self._sensor_frame(image, camera, None, 1.0, rgb, gray_mode)

    def rgbd_frame(self, image: np.ndarray, depth_map: np.ndarray, camera, depth_factor: float = 1.0,
                   rgb: bool = True, gray_mode: int = L.GRAY_SHIFT15):
        """The RGB-D Frame (Frame.cc:154-214 behind Tracking::GrabImageRGBD): as mono_frame, plus
        ComputeStereoFromRGBD on the raw uint16 / float32 `depth_map`; `depth_factor` is mDepthMapFactor
        already inverted (Tracking.cc:148-152)."""
        return self._sensor_frame(image, camera, depth_map, depth_factor, rgb, gray_mode)

    def to_gray_batch(self, src, dst, rgb: bool = True, gray_mode: int = L.GRAY_SHIFT15,
                      stream: Optional[int] = None) -> None:
        """cvtColor(*2GRAY) on device tensors: src (n, rows, cols, 3 or 4) uint8, dst (n, rows, cols) uint8,
        both with contiguous pixels (any row and image strides). Async on `stream` (default: the handle's)."""
        if src.dim() != 4 or dst.dim() != 3 or src.shape[:3] != dst.shape or src.shape[3] not in (3, 4):
            raise ValueError("to_gray_batch: src (n, rows, cols, 3|4), dst (n, rows, cols)")
        if src.stride(3) != 1 or src.stride(2) != src.shape[3] or dst.stride(2) != 1:
            raise ValueError("to_gray_batch: pixels must be contiguous within a row")
        n, rows, cols, ch = src.shape
        L.check(self._lib.orbfe_gray_batch_device(
            self._h, n, c_void_p(src.data_ptr()), c_size_t(src.stride(0)), c_size_t(src.stride(1)), ch,
            int(bool(rgb)), int(gray_mode), rows, cols, c_void_p(dst.data_ptr()), c_size_t(dst.stride(0)),
            c_size_t(dst.stride(1)), c_void_p(stream or 0)), "orbfe_gray_batch_device")

    def frame_finish_batch(self, n_images: int, camera, d_kps: int, d_counts: int, cap: int, rows: int, cols: int,
                           d_keys_un: int, d_u_right: int, d_depth: int, depth_maps=None,
                           depth_factor: float = 1.0, stream: Optional[int] = None) -> None:
        """UndistortKeyPoints + ComputeStereoFromRGBD of a device batch (orbfe_frame_finish_batch_device): the
        int arguments are device addresses laid out as extract_batch_device's outputs; depth_maps is a
        (n, rows, cols) uint16 / float32 device tensor (any row and image strides) or None (monocular)."""
        cam = camera if isinstance(camera, L.camera) else L.make_camera(**camera)
        dm, ist, pitch, dtype = 0, 0, 0, L.DEPTH_F32
        if depth_maps is not None:
            es = depth_maps.element_size()
            if depth_maps.dim() != 3 or depth_maps.stride(2) != 1 or es not in (2, 4) or \
                    (es == 4 and not depth_maps.is_floating_point()):
                raise ValueError("frame_finish_batch: depth_maps (n, rows, cols) of 16-bit raw values or float32")
            dm, ist, pitch = depth_maps.data_ptr(), depth_maps.stride(0) * es, depth_maps.stride(1) * es
            dtype = L.DEPTH_U16 if es == 2 else L.DEPTH_F32
        L.check(self._lib.orbfe_frame_finish_batch_device(
            self._h, int(n_images), byref(cam), c_void_p(d_kps), c_void_p(d_counts), int(cap), c_void_p(dm),
            c_size_t(ist), c_size_t(pitch), dtype, float(depth_factor), int(rows), int(cols), c_void_p(d_keys_un),
            c_void_p(d_u_right), c_void_p(d_depth), c_void_p(stream or 0)), "orbfe_frame_finish_batch_device")

    def compute_stereo_matches_batch_device(self, n_pairs: int, left0: int, right0: int, d_kps: int,
                                            d_desc: int, d_counts: int, cap: int, mbf: float,
                                            mb: float, d_u_right: int, d_depth: int,
                                            stream: Optional[int] = None) -> None:
        """Device-resident ComputeStereoMatches over pairs (left0 + p, right0 + p) of the last
        extract_batch_device call; outputs at p*cap + i. Async on `stream`."""
        L.check(self._lib.orbfe_compute_stereo_matches_batch_device(
            self._h, int(n_pairs), int(left0), int(right0), c_void_p(d_kps), c_void_p(d_desc),
            c_void_p(d_counts), int(cap), float(mbf), float(mb), c_void_p(d_u_right),
            c_void_p(d_depth), c_void_p(stream or 0)), "orbfe_compute_stereo_matches_batch_device")

    @property
    def stream(self) -> int:
        return self._lib.orbfe_extractor_stream(self._h) or 0

    def wait_pyramid(self, stream: int) -> None:
        """Make `stream` wait for the pyramid of this handle's last extract call
        (orbfe_extractor_pyramid_event): call right after the extract call."""
        L.check(self._lib.orbfe_stream_wait_event(c_void_p(stream or 0),
                                                  c_void_p(self._lib.orbfe_extractor_pyramid_event(self._h))),
                "orbfe_stream_wait_event")

    # ---- mvImagePyramid (ORBextractor.h:100) --------------------------------------------
    def level_view(self, level: int, image: int = 0) -> np.ndarray:
        """mvImagePyramid[level] of image `image` of the last call as a view of the handle's host
        block (no copy): valid until the next extract call, like the reference's cv::Mat headers."""
        p = c_void_p()
        r, c, s = c_int(), c_int(), c_size_t()
        L.check(self._lib.orbfe_get_level(self._h, image, level, byref(p), byref(r), byref(c),
                                          byref(s)), "orbfe_get_level")
        buf = (ctypes.c_uint8 * ((r.value - 1) * s.value + c.value)).from_address(p.value)
        return np.lib.stride_tricks.as_strided(np.frombuffer(buf, np.uint8), (r.value, c.value), (s.value, 1))

    def level(self, level: int, image: int = 0) -> np.ndarray:
        return self.level_view(level, image).copy()

    def set_host_pyramid(self, on: bool = True) -> None:
        """orbfe_extractor_set_host_pyramid: later host-buffer calls copy each pyramid to the host
        beside the extraction, so mvImagePyramid costs no copy of its own."""
        L.check(self._lib.orbfe_extractor_set_host_pyramid(self._h, 1 if on else 0), "set_host_pyramid")

    def set_graphs(self, on: bool) -> None:
        """orbfe_extractor_set_graphs: replay each extract call's launch sequence as a hipGraph
        captured per argument set; off (the default) launches every kernel directly."""
        L.check(self._lib.orbfe_extractor_set_graphs(self._h, 1 if on else 0), "set_graphs")

    def debug_graph_stats(self) -> tuple:
        """(graph captures, graph replays, graphs held) of this handle."""
        import numpy as np
        out = np.zeros(3, np.int64)
        L.check(self._lib.orbfe_debug_graph_stats(self._h, out.ctypes.data), "graph_stats")
        return tuple(int(x) for x in out)

    @property
    def mvImagePyramid(self) -> List[np.ndarray]:
        return [self.level(l) for l in range(self.nlevels)]

    # ---- instrumentation ----------------------------------------------------------------
    def debug_candidates(self, level: int, image: int = 0) -> np.ndarray:
        n = c_int()
        L.check(self._lib.orbfe_debug_get_candidates(self._h, image, level, None, 0, byref(n)),
                "debug_candidates")
        out = np.zeros(max(n.value, 1), np.uint32)
        L.check(self._lib.orbfe_debug_get_candidates(self._h, image, level, L.ptr(out), len(out),
                                                     byref(n)), "debug_candidates")
        return out[:n.value]
    def debug_candidate_total(self) -> int:
        """FAST candidates over every image and level of the last call."""
        t = ctypes.c_longlong()
        L.check(self._lib.orbfe_debug_candidate_total(self._h, byref(t)), "debug_candidate_total")
        return t.value

    def debug_level_keys(self, level: int, image: int = 0) -> np.ndarray:
        n = c_int()
        L.check(self._lib.orbfe_debug_get_level_keys(self._h, image, level, None, 0, byref(n)),
                "debug_level_keys")
        out = np.zeros(max(n.value, 1), np.uint32)
        L.check(self._lib.orbfe_debug_get_level_keys(self._h, image, level, L.ptr(out), len(out),
                                                     byref(n)), "debug_level_keys")
        return out[:n.value]

    def debug_blurred(self, level: int, image: int = 0) -> np.ndarray:
        ref = self.level(level, image)
        out = np.zeros(ref.shape, np.uint8)
        L.check(self._lib.orbfe_debug_get_blurred(self._h, image, level, L.ptr(out), out.size),
                "debug_blurred")
        return out

    def debug_set_octree_key_cap(self, cap: int) -> None:
        """Limit the keys DistributeOctTree keeps in LDS (0: global-memory path; <0: auto)."""
        L.check(self._lib.orbfe_debug_set_octree_key_cap(self._h, int(cap)), "set_octree_key_cap")

    def debug_set_fast_side_levels(self, k: int) -> None:
        """FAST of levels 0..k-1 on the side stream as each level is built (k <= 0: the default, 3)."""
        L.check(self._lib.orbfe_debug_set_fast_side_levels(self._h, int(k)), "set_fast_side_levels")

    def debug_set_octree_split(self, k: int) -> None:
        """DistributeOctTree in two launches for batches of 8+ images, levels 0..k-1 at 80 KiB of LDS
        per block and k.. at 40 KiB (default 5; k <= 0: one launch of every level at 80 KiB)."""
        L.check(self._lib.orbfe_debug_set_octree_split(self._h, int(k)), "set_octree_split")

    def debug_set_octree_threads(self, small_calls: int, batches: int = 256) -> None:
        """DistributeOctTree's block size (256 / 512 / 1024) for calls of fewer than 8 images (512
        default) and for batches of 8+ (256 default)."""
        L.check(self._lib.orbfe_debug_set_octree_threads(self._h, int(small_calls), int(batches)),
                "set_octree_threads")

    def debug_set_octree_serial(self, small_calls: int, batches: int = 48) -> None:
        """DistributeOctTree: nodes of at most this many keys split by one thread, larger ones by a
        wavefront (1..128), for calls of fewer than 8 images / batches of 8+."""
        L.check(self._lib.orbfe_debug_set_octree_serial(self._h, int(small_calls), int(batches)),
                "set_octree_serial")

    def debug_set_fast_side_merge(self, on: bool) -> None:
        """Batches: the side stream's FAST levels 1..k-1 in one launch after level k-1 is built."""
        L.check(self._lib.orbfe_debug_set_fast_side_merge(self._h, int(bool(on))), "set_fast_side_merge")

    def debug_set_schedule_autotune(self, on: bool) -> None:
        """Calls of fewer than 8 images: time the latency schedule on two streams against one stream
        over the first host-buffer calls and keep the faster (default on); off: always two."""
        L.check(self._lib.orbfe_debug_set_schedule_autotune(self._h, int(bool(on))), "set_schedule_autotune")

    def debug_schedule_choice(self, n_images: int = 1) -> int:
        """-1 still timing, 0 two streams, 1 the launch stream alone (calls of n_images images)."""
        return int(self._lib.orbfe_debug_schedule_choice(self._h, int(n_images)))

    def debug_set_zero_copy(self, inp: bool, out: Optional[bool] = None) -> None:
        """Host-buffer calls of fewer than 8 images: k_copy0 reads the staged image from pinned host
        memory, and the kernels write the results into the pinned host mirror (both default) instead
        of H2D / D2H copies (out defaults to inp)."""
        out = inp if out is None else out
        L.check(self._lib.orbfe_debug_set_zero_copy(self._h, int(bool(inp)), int(bool(out))), "set_zero_copy")

    def debug_set_pyramid_tiles(self, small=(0, 0), batch=(0, 0)) -> None:
        """ComputePyramid's levels 1.. in one k_pyramid launch of tx x ty tiles per image for calls of
        fewer than 8 images / batches of 8+ ((0, 0): one resize launch per level)."""
        L.check(self._lib.orbfe_debug_set_pyramid_tiles(self._h, int(small[0]), int(small[1]), int(batch[0]),
                                                        int(batch[1])), "set_pyramid_tiles")

    def debug_set_latency_schedule(self, k: int) -> None:
        """Calls of fewer than 8 images: FAST and DistributeOctTree of levels 0..k-1 on the side stream
        beside the main stream's levels k.. (default 1; k <= 0: the throughput schedule)."""
        L.check(self._lib.orbfe_debug_set_latency_schedule(self._h, int(k)), "set_latency_schedule")

    def debug_set_octree_lds(self, hi_kb: int, lo_kb: int) -> None:
        """LDS budgets (KiB per block) of the octree launches below / from the split (80 / 40)."""
        L.check(self._lib.orbfe_debug_set_octree_lds(self._h, int(hi_kb), int(lo_kb)), "set_octree_lds")

    def debug_set_fast_wpb(self, side_wpb: int, main_wpb: int) -> None:
        """k_fast cells per workgroup: side-stream launches (default 4), the rest (default 1)."""
        L.check(self._lib.orbfe_debug_set_fast_wpb(self._h, int(side_wpb), int(main_wpb)), "set_fast_wpb")

    def debug_set_blur_mode(self, mode: int) -> None:
        """GaussianBlur placement: 0 side stream beside DistributeOctTree (default), 1 launch stream
        after it (several handles sharing one side stream)."""
        L.check(self._lib.orbfe_debug_set_blur_mode(self._h, int(mode)), "set_blur_mode")

    def set_side_stream(self, stream: int) -> None:
        """Run the side-stream work on `stream` (a hipStream_t address; 0 restores the handle's own)."""
        L.check(self._lib.orbfe_set_side_stream(self._h, c_void_p(stream or 0)), "set_side_stream")

    def debug_set_inline_side(self, on: bool = True) -> None:
        """Run the side-stream work (k_blur, early FAST levels) on the launch stream."""
        L.check(self._lib.orbfe_debug_set_inline_side(self._h, 1 if on else 0), "set_inline_side")

    def geometry(self, rows: int, cols: int) -> np.ndarray:
        info = np.zeros(7 * self.nlevels, np.int32)
        L.check(self._lib.orbfe_debug_geometry(self._h, rows, cols, L.ptr(info), len(info)),
                "geometry")
        return info.reshape(self.nlevels, 7)


def image_bounds(camera, rows: int, cols: int) -> np.ndarray:
    """Frame::ComputeImageBounds (Frame.cc:488-520): float32 (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    cam = camera if isinstance(camera, L.camera) else L.make_camera(**camera)
    out = np.zeros(4, np.float32)
    L.check(L.lib().orbfe_image_bounds(byref(cam), int(rows), int(cols), L.ptr(out)), "orbfe_image_bounds")
    return out


def undistort_keypoints_host(camera, keys: KeyPoints) -> KeyPoints:
    """Frame::UndistortKeyPoints (Frame.cc:456-486) on host arrays: mvKeysUn of mvKeys."""
    cam = camera if isinstance(camera, L.camera) else L.make_camera(**camera)
    k = np.ascontiguousarray(keys, L.KEYPOINT_DTYPE)
    out = np.zeros(len(k), L.KEYPOINT_DTYPE)
    L.check(L.lib().orbfe_undistort_keypoints_host(byref(cam), L.ptr(k), len(k), L.ptr(out)),
            "orbfe_undistort_keypoints_host")
    return out


def stereo_from_depth_host(camera, keys: KeyPoints, keys_un: KeyPoints, depth_map: Optional[np.ndarray],
                           depth_factor: float = 1.0):
    """Frame::ComputeStereoFromRGBD (Frame.cc:702-723) on host arrays: (mvuRight, mvDepth). depth_map is the raw
    uint16 / float32 map (contiguous within a row; any row stride) or None."""
    cam = camera if isinstance(camera, L.camera) else L.make_camera(**camera)
    k = np.ascontiguousarray(keys, L.KEYPOINT_DTYPE)
    u = np.ascontiguousarray(keys_un, L.KEYPOINT_DTYPE)
    ur = np.zeros(len(k), np.float32)
    dep = np.zeros(len(k), np.float32)
    rows = cols = pitch = address = 0
    dtype = L.DEPTH_F32
    if depth_map is not None:
        if depth_map.dtype not in (np.uint16, np.float32) or depth_map.ndim != 2 or \
                depth_map.strides[1] != depth_map.itemsize:
            raise ValueError("the depth map is a 2-D uint16 or float32 array with contiguous rows")
        rows, cols = depth_map.shape
        dtype = L.DEPTH_U16 if depth_map.dtype == np.uint16 else L.DEPTH_F32
        pitch, address = depth_map.strides[0], depth_map.ctypes.data
    L.check(L.lib().orbfe_stereo_from_depth_host(byref(cam), L.ptr(k), L.ptr(u), len(k), c_void_p(address),
                                                 c_size_t(pitch), dtype, float(depth_factor), rows, cols,
                                                 L.ptr(ur), L.ptr(dep)), "orbfe_stereo_from_depth_host")
    return ur, dep


def register_host(a: np.ndarray) -> None:
    """orbfe_host_register: page-lock a (C-contiguous) numpy buffer the host-buffer entry points
    then DMA from / to directly (images; keypoint and descriptor outputs with cap equal to
    max_keypoints). Keep the array alive and call unregister_host before dropping it."""
    if not a.flags["C_CONTIGUOUS"]:
        raise ValueError("register_host needs a C-contiguous array")
    L.check(L.lib().orbfe_host_register(c_void_p(a.ctypes.data), c_size_t(a.nbytes)), "orbfe_host_register")


def unregister_host(a: np.ndarray) -> None:
    L.check(L.lib().orbfe_host_unregister(c_void_p(a.ctypes.data)), "orbfe_host_unregister")


def synth_frame(index: int, rows: int = 376, cols: int = 1241, n_rects: int = 0,
                right: bool = False):
    """Seeded synthetic KITTI-shaped frame (orbfe_synth.h). Returns left or (left, right)."""
    lib = L.lib()
    left = np.zeros((rows, cols), np.uint8)
    r = np.zeros((rows, cols), np.uint8) if right else None
    L.check(lib.orbfe_synth_frame(int(index), rows, cols, int(n_rects), L.ptr(left),
                                  L.ptr(r) if right else None, c_size_t(cols)), "orbfe_synth_frame")
    return (left, r) if right else left


def synth_sequence_frame(seq: int, t: int, rows: int = 376, cols: int = 1241, cam: dict = None,
                         step_z: float = 1.0, right: bool = False):
    """Frame t of a seeded driving sequence (orbfe_synth_sequence_frame): the camera moves step_z m
    along +z per frame, so frames t and t+1 are the C3 KeyFrame pair of SURVEY 8(d). `cam` holds
    fx, fy, cx, cy and bf (baseline = bf / fx); KITTI-like by default. Returns left or (left, right)."""
    from .synthetic import KITTI_CAM
    cam = cam or KITTI_CAM
    lib = L.lib()
    left = np.zeros((rows, cols), np.uint8)
    r = np.zeros((rows, cols), np.uint8) if right else None
    L.check(lib.orbfe_synth_sequence_frame(int(seq), int(t), rows, cols, cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                                           cam["bf"] / cam["fx"], float(step_z), L.ptr(left),
                                           L.ptr(r) if right else None, c_size_t(cols)),
            "orbfe_synth_sequence_frame")
    return (left, r) if right else left
