"""The occupancy grid of the reference's GridMapping thread on MI355X (include/orbfe_gridmap.h): one
Bresenham beam per map point of a keyframe into a visit counter, one increment per point into an
occupied counter, and the int8 grid message built from the two (src/GridMapping.cpp:72-154, 232-270).

`OccupancyGrid` owns the device counters and the int8 grid. update() takes the keyframes' camera
centres and their points' world positions (GetMPs order); update_resident() reads the points from a
CovisibilityGraph's rows and geometry store, so nothing but the centres crosses the bus. The
loop-closure rebuild (ResetGridMap, then UpdateGridMap of every keyframe) is reset() followed by one
update over all keyframes. host_update / host_build apply the same rules on numpy arrays with no
device. Two rule sets: REFERENCE (the default: what the reference's code does, its chained beam starts
and its early return included) and INTENDED (what its header documents).
"""
from __future__ import annotations

from ctypes import byref, c_float, c_int32, c_void_p
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

REFERENCE, INTENDED = L.GRIDMAP_REFERENCE, L.GRIDMAP_INTENDED


class GridStats(NamedTuple):
    """What one update did (orbfe_gridmap_stats). rows: the dirty row range [row0, row1)."""
    beams: int
    visits: int
    dropped: int
    points_cut: int
    kf_outside: int
    rows: Tuple[int, int]


def _stats(s: L.gridmap_stats) -> GridStats:
    return GridStats(int(s.beams), int(s.visits), int(s.dropped), int(s.points_cut), int(s.kf_outside),
                     (int(s.row0), int(s.row1)))


def geometry(scale_factor: int = 3, min_x: Optional[float] = None, max_x: Optional[float] = None,
             min_z: Optional[float] = None, max_z: Optional[float] = None, visit_threshold: int = 0) -> L.gridmap_geometry:
    """An orbfe_gridmap_geometry; the ends default to the reference's -1000, 1000, -500 and 1600 times the scale."""
    s = int(scale_factor)
    return L.gridmap_geometry(scale_factor=s, min_x=float(-1000 * s if min_x is None else min_x),
                              max_x=float(1000 * s if max_x is None else max_x),
                              min_z=float(-500 * s if min_z is None else min_z),
                              max_z=float(1600 * s if max_z is None else max_z), visit_threshold=int(visit_threshold))


def dims(geo: L.gridmap_geometry) -> Tuple[int, int, float, float]:
    """rows, cols, norm_x, norm_z of a geometry (raises OrbfeError on one the library refuses)."""
    r, c, nx, nz = c_int32(), c_int32(), c_float(), c_float()
    L.check(L.lib().orbfe_gridmap_dims(byref(geo), byref(r), byref(c), byref(nx), byref(nz)), "orbfe_gridmap_dims")
    return r.value, c.value, nx.value, nz.value


def _csr(centres, points: Sequence):
    """centres [n_kf, 3] and one [n_i, 3] array per keyframe -> contiguous centres, begin, positions."""
    c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
    if len(points) != len(c):
        raise ValueError("one point array per keyframe")
    parts = [np.asarray(p, np.float32).reshape(-1, 3) for p in points]
    begin = np.zeros(len(parts) + 1, np.int32)
    if parts:
        begin[1:] = np.cumsum([len(p) for p in parts])
    pos = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 3), np.float32))
    return c, begin, pos


def host_update(geo: L.gridmap_geometry, rules: int, occupied: np.ndarray, visits: np.ndarray, centres,
                points: Sequence) -> GridStats:
    """orbfe_gridmap_host_update: increments the two int32 [rows, cols] arrays in place."""
    for a in (occupied, visits):
        if a.dtype != np.int32 or not a.flags["C_CONTIGUOUS"]:
            raise ValueError("counters are C-contiguous int32 arrays")
    c, begin, pos = _csr(centres, points)
    s = L.gridmap_stats()
    L.check(L.lib().orbfe_gridmap_host_update(byref(geo), int(rules), L.ptr(occupied), L.ptr(visits), len(c), L.ptr(c),
                                              L.ptr(begin), L.ptr(pos), byref(s)), "orbfe_gridmap_host_update")
    return _stats(s)


def host_build(geo: L.gridmap_geometry, occupied: np.ndarray, visits: np.ndarray, row0: int = 0,
               row1: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """orbfe_gridmap_host_build: the int8 grid and the float data grid of rows [row0, row1)."""
    rows, cols, _, _ = dims(geo)
    row1 = rows if row1 is None else int(row1)
    occ = np.ascontiguousarray(occupied, np.int32)
    vis = np.ascontiguousarray(visits, np.int32)
    grid = np.zeros((max(row1 - row0, 0), cols), np.int8)
    data = np.zeros((max(row1 - row0, 0), cols), np.float32)
    L.check(L.lib().orbfe_gridmap_host_build(byref(geo), L.ptr(occ), L.ptr(vis), int(row0), row1, L.ptr(grid),
                                             L.ptr(data)), "orbfe_gridmap_host_build")
    return grid, data


class OccupancyGrid:
    def __init__(self, geo: Optional[L.gridmap_geometry] = None, rules: int = REFERENCE, device: int = 0):
        self._lib = L.lib()
        self.geometry = geo if geo is not None else geometry()
        self.rules = int(rules)
        self.rows, self.cols, self.norm_x, self.norm_z = dims(self.geometry)
        h = c_void_p()
        L.check(self._lib.orbfe_gridmap_create(int(device), byref(self.geometry), self.rules, byref(h)),
                "orbfe_gridmap_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_gridmap_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """ResetGridMap: both counters (and the grid) to zero."""
        L.check(self._lib.orbfe_gridmap_reset(self._h), "orbfe_gridmap_reset")

    def update(self, centres, points: Sequence) -> GridStats:
        """UpdateGridMap of len(centres) keyframes: centres [n_kf, 3] (Ow), points[k] the [n, 3] world positions of
        keyframe k's GetMPs()."""
        c, begin, pos = _csr(centres, points)
        return self.update_csr(c, begin, pos)

    def update_csr(self, centres: np.ndarray, begin: np.ndarray, world_pos: np.ndarray) -> GridStats:
        c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(begin, np.int32)
        p = np.ascontiguousarray(world_pos, np.float32)
        if len(b) != len(c) + 1:
            raise ValueError("begin holds one entry per keyframe and the total")
        s = L.gridmap_stats()
        L.check(self._lib.orbfe_gridmap_update(self._h, len(c), L.ptr(c), L.ptr(b), L.ptr(p), byref(s)),
                "orbfe_gridmap_update")
        return _stats(s)

    def update_resident(self, graph, kf_ids, centres) -> GridStats:
        """The same update over the rows and the geometry store of a CovisibilityGraph. A point without geometry
        raises OrbfeError (ORBFE_ERR_STATE) with .n_missing set; no counter is touched then."""
        ids = np.ascontiguousarray(kf_ids, np.int64)
        c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
        if len(ids) != len(c):
            raise ValueError("one centre per keyframe id")
        s = L.gridmap_stats()
        missing = c_int32()
        st = self._lib.orbfe_gridmap_update_resident(self._h, graph._h, len(ids), L.ptr(ids), L.ptr(c), byref(s),
                                                     byref(missing))
        if st < 0:
            e = L.OrbfeError(st, "orbfe_gridmap_update_resident")
            e.n_missing = missing.value
            raise e
        return _stats(s)

    def build(self, all_rows: bool = False) -> None:
        """BuildOccupancyGridMsg over the dirty rows (or all of them); clears the dirty range."""
        L.check(self._lib.orbfe_gridmap_build(self._h, 1 if all_rows else 0), "orbfe_gridmap_build")

    def _range(self, row0, row1):
        return int(row0), self.rows if row1 is None else int(row1)

    def download(self, row0: int = 0, row1: Optional[int] = None) -> np.ndarray:
        """Rows [row0, row1) of the int8 grid message."""
        r0, r1 = self._range(row0, row1)
        out = np.zeros((max(r1 - r0, 0), self.cols), np.int8)
        L.check(self._lib.orbfe_gridmap_download(self._h, r0, r1, L.ptr(out)), "orbfe_gridmap_download")
        return out

    def download_counters(self, row0: int = 0, row1: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(occupied, visits) of rows [row0, row1)."""
        r0, r1 = self._range(row0, row1)
        occ = np.zeros((max(r1 - r0, 0), self.cols), np.int32)
        vis = np.zeros_like(occ)
        L.check(self._lib.orbfe_gridmap_download_counters(self._h, r0, r1, L.ptr(occ), L.ptr(vis)),
                "orbfe_gridmap_download_counters")
        return occ, vis

    def upload_counters(self, row0: int, occupied, visits) -> None:
        """Overwrites rows row0 .. row0 + len(occupied) of both counters and marks them dirty."""
        occ = np.ascontiguousarray(occupied, np.int32).reshape(-1, self.cols)
        vis = np.ascontiguousarray(visits, np.int32).reshape(-1, self.cols)
        if occ.shape != vis.shape:
            raise ValueError("occupied / visits differ in shape")
        L.check(self._lib.orbfe_gridmap_upload_counters(self._h, int(row0), int(row0) + len(occ), L.ptr(occ), L.ptr(vis)),
                "orbfe_gridmap_upload_counters")

    def probability(self, row0: int = 0, row1: Optional[int] = None) -> np.ndarray:
        """Rows [row0, row1) of the float data grid (gmap_.data)."""
        r0, r1 = self._range(row0, row1)
        out = np.zeros((max(r1 - r0, 0), self.cols), np.float32)
        L.check(self._lib.orbfe_gridmap_probability(self._h, r0, r1, L.ptr(out)), "orbfe_gridmap_probability")
        return out
