"""A second statement of the occupancy grid's rules (include/orbfe_gridmap.h; the reference's
src/GridMapping.cpp:72-154, 232-270) in plain scalar Python and NumPy float32, sharing no code with the
library. Counters are sparse dicts (flat index -> count), so the 6300 x 6000 default grid costs nothing.

  cell      g = p * float(scale); c = (g - min) * norm; floor; int; outside when < 0 or >= size, and
            (decision) when NaN or beyond the int range.
  beam      CastLaserBeam literally: the steep swap, the ordering swap, deltaerr = dy / dx in double, error
            accumulated in double step by step and tested >= 0.5, both ends visited; dx == 0 gives a NaN
            deltaerr and one cell.
  REFERENCE the swaps rewrite the keyframe's cell (arguments by reference), so beam i starts where the swaps
            of beams 0..i-1 left it; the first outside point ends the keyframe; a visit goes to the flat
            index row * cols + col, dropped (and counted) when >= rows * cols.
  INTENDED  every beam starts at the keyframe's cell; an outside point is skipped.
  build     data = vc <= thr ? 1 : 1 - float(oc) / float(vc); msg = trunc((1 - data) * 100) clamped to int8.
"""
import numpy as np

REFERENCE, INTENDED = 0, 1
F = np.float32


class Stats(dict):
    __getattr__ = dict.__getitem__


def beam(x0, y0, x1, y1):
    """-> (visits as (a, b) = at<int>(a, b), x0, y0 after the swaps, steep)."""
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0 = y0, x0
        x1, y1 = y1, x1
    if x0 > x1:
        x0, x1 = x1, x0
        y0, y1 = y1, y0
    dx = x1 - x0
    dy = abs(y1 - y0)
    error = 0.0
    deltaerr = float(dy) / float(dx) if dx != 0 else float("nan")  # 0 / 0 in C
    y = y0
    ystep = 1 if y0 < y1 else -1
    out = []
    for x in range(x0, x1 + 1):
        out.append((x, y) if steep else (y, x))
        error = error + deltaerr
        if error >= 0.5:
            y = y + ystep
            error = error - 1.0
    return out, x0, y0, steep


def beam_exact(x0, y0, x1, y1, ties_step=True):
    """The same walk with the exact rational error (integer Bresenham); a tie (error == 1/2) steps or not."""
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0 = y0, x0
        x1, y1 = y1, x1
    if x0 > x1:
        x0, x1 = x1, x0
        y0, y1 = y1, y0
    dx = x1 - x0
    dy = abs(y1 - y0)
    num = 0  # error * dx
    y = y0
    ystep = 1 if y0 < y1 else -1
    out = []
    for x in range(x0, x1 + 1):
        out.append((x, y) if steep else (y, x))
        num += dy
        if dx and (2 * num > dx or (ties_step and 2 * num == dx)):
            y += ystep
            num -= dx
    return out


class RefGrid:
    def __init__(self, scale=3, min_x=None, max_x=None, min_z=None, max_z=None, visit_threshold=0, rules=REFERENCE):
        self.scale = int(scale)
        self.min_x = F(-1000 * scale if min_x is None else min_x)
        self.max_x = F(1000 * scale if max_x is None else max_x)
        self.min_z = F(-500 * scale if min_z is None else min_z)
        self.max_z = F(1600 * scale if max_z is None else max_z)
        self.cols = int(self.max_x - self.min_x)
        self.rows = int(self.max_z - self.min_z)
        assert F(self.cols) == self.max_x - self.min_x and F(self.rows) == self.max_z - self.min_z
        self.norm_x = F(self.cols - 1) / F(self.cols)
        self.norm_z = F(self.rows - 1) / F(self.rows)
        self.thr = int(visit_threshold)
        self.rules = rules
        self.reset()
        # what the chained rules did, over the grid's life (the tests assert these are exercised)
        self.changed_starts = 0   # beams whose start differed from the keyframe's own cell
        self.wrapped_writes = 0   # visits with col >= cols that stayed inside the buffer

    def reset(self):
        self.occ, self.vis = {}, {}
        self.touched = set()  # rows an increment touched since the last take_dirty()

    def coord(self, p, lo, norm):
        with np.errstate(all="ignore"):
            g = F(p) * F(self.scale)
            return (g - lo) * norm

    def cell1(self, p, lo, norm, size):
        with np.errstate(all="ignore"):
            f = np.floor(self.coord(p, lo, norm))
        if not (f >= 0 and f < 2147483648.0):
            return None
        i = int(f)
        return i if i < size else None

    def cell(self, pos):
        x = self.cell1(pos[0], self.min_x, self.norm_x, self.cols)
        z = self.cell1(pos[2], self.min_z, self.norm_z, self.rows)
        return None if x is None or z is None else (x, z)

    def update(self, centres, points):
        s = Stats(beams=0, visits=0, dropped=0, points_cut=0, kf_outside=0)
        size = self.rows * self.cols
        for centre, pts in zip(centres, points):
            kf = self.cell(centre)
            if kf is None:
                s["kf_outside"] += 1
                continue
            kx, kz = kf
            for i, p in enumerate(pts):
                c = self.cell(p)
                if c is None:
                    if self.rules == REFERENCE:
                        s["points_cut"] += len(pts) - i
                        break
                    s["points_cut"] += 1
                    continue
                px, pz = c
                flat = pz * self.cols + px
                self.occ[flat] = self.occ.get(flat, 0) + 1
                self.touched.add(pz)
                if (kx, kz) != kf:
                    self.changed_starts += 1
                cells, nx, nz, _ = beam(kx, kz, px, pz)
                if self.rules == REFERENCE:
                    kx, kz = nx, nz
                s["beams"] += 1
                for a, b in cells:
                    flat = a * self.cols + b
                    if flat >= size:
                        s["dropped"] += 1
                        continue
                    if b >= self.cols:
                        self.wrapped_writes += 1
                    self.vis[flat] = self.vis.get(flat, 0) + 1
                    s["visits"] += 1
                    self.touched.add(flat // self.cols)
        return s

    def dirty(self):
        """[row0, row1) of the rows touched since the last take_dirty(); (0, 0) when none."""
        return (min(self.touched), max(self.touched) + 1) if self.touched else (0, 0)

    def take_dirty(self):
        d = self.dirty()
        self.touched = set()
        return d

    def counters(self, row0=0, row1=None):
        row1 = self.rows if row1 is None else row1
        occ = np.zeros((row1 - row0, self.cols), np.int32)
        vis = np.zeros_like(occ)
        lo, hi = row0 * self.cols, row1 * self.cols
        for d, a in ((self.occ, occ), (self.vis, vis)):
            for flat, n in d.items():
                if lo <= flat < hi:
                    a.reshape(-1)[flat - lo] = n
        return occ, vis

    def sparse(self):
        """(occupied, visits) as sorted [(flat, count)] lists."""
        return sorted(self.occ.items()), sorted(self.vis.items())

    def build(self, row0=0, row1=None):
        occ, vis = self.counters(row0, row1)
        return build(occ, vis, self.thr)


def build(occ, vis, thr):
    """-> (msg int8, data float32) of two int32 arrays."""
    occ = np.asarray(occ, np.int32)
    vis = np.asarray(vis, np.int32)
    with np.errstate(all="ignore"):
        ratio = occ.astype(np.float32) / vis.astype(np.float32)
        data = np.where(vis <= thr, F(1), F(1) - ratio).astype(np.float32)
        v = (F(1) - data) * F(100)
    msg = np.clip(np.trunc(v.astype(np.float64)), -128, 127).astype(np.int8)
    return msg, data
