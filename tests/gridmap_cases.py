"""The inputs of the occupancy-grid tests (tests/test_gridmap_core.py on the host entry points,
tests/test_gpu_gridmap.py on the device), built once per process. A case is a dict: geo (keyword arguments
of gridmap_ref.RefGrid and of the library's geometry), rules, centres [n_kf, 3] float32 and points (one
[n, 3] float32 array per keyframe). World positions are chosen per cell and checked against the
reference's own cell rule when the case is built."""
import functools

import numpy as np

import gridmap_ref as R

SEGMENT = 64  # ORBFE_GRIDMAP_SEGMENT


def unit_geo(rows, cols, **kw):
    return dict(scale=1, min_x=0.0, max_x=float(cols), min_z=0.0, max_z=float(rows), **kw)


def pos_of_cell(ref, x, z):
    """A world position in the middle of cell (x, z)."""
    px = ((x + 0.5) / float(ref.norm_x) + float(ref.min_x)) / ref.scale
    pz = ((z + 0.5) / float(ref.norm_z) + float(ref.min_z)) / ref.scale
    p = np.array([px, 0.25, pz], np.float32)
    assert ref.cell(p) == (x, z), (x, z, ref.cell(p))
    return p


def positions(ref, cells):
    return np.array([pos_of_cell(ref, x, z) for x, z in cells], np.float32).reshape(-1, 3)


def case(geo, rules, centres, points):
    return dict(geo=geo, rules=rules, centres=np.asarray(centres, np.float32).reshape(-1, 3),
                points=[np.asarray(p, np.float32).reshape(-1, 3) for p in points])


@functools.lru_cache(None)
def star():
    """Case 1: 129 x 129, INTENDED, one beam from (64, 64) to every cell, over three keyframes."""
    geo = unit_geo(129, 129)
    ref = R.RefGrid(rules=R.INTENDED, **geo)
    cells = [(x, z) for z in range(129) for x in range(129)]
    pts = positions(ref, cells)
    c = pos_of_cell(ref, 64, 64)
    return case(geo, R.INTENDED, [c, c, c], [pts[:5547], pts[5547:11094], pts[11094:]])


def segment_dxs():
    S = SEGMENT
    # the issue's lengths as visited cells (dx + 1) and as steps taken (dx)
    return sorted({v for n in (1, 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 4 * S + 1) for v in (n - 1, n)})


@functools.lru_cache(None)
def segment_edges():
    """Case 2: every length around the segment size along a row, a column, a diagonal and at slope 3/10, both ways;
    one keyframe per beam."""
    geo = unit_geo(320, 320)
    ref = R.RefGrid(rules=R.INTENDED, **geo)
    centres, points = [], []
    for d in segment_dxs():
        for ex, ez in ((d, 0), (0, d), (d, d), (d, 3 * d // 10), (3 * d // 10, d)):
            a, b = (20, 30), (20 + ex, 30 + ez)
            for s, e in ((a, b), (b, a)):
                centres.append(pos_of_cell(ref, *s))
                points.append(positions(ref, [e]))
    return case(geo, R.INTENDED, centres, points)


CHAIN_GRIDS = ((8, 5), (5, 8), (8, 8))  # rows x cols
CHAIN_SEED = 29


@functools.lru_cache(None)
def chain(rows, cols):
    """Case 3: REFERENCE rules, 2,000 keyframes of 6 random in-grid points."""
    geo = unit_geo(rows, cols)
    ref = R.RefGrid(rules=R.REFERENCE, **geo)
    rng = np.random.default_rng(CHAIN_SEED)
    centres, points = [], []
    for _ in range(2000):
        centres.append(pos_of_cell(ref, int(rng.integers(cols)), int(rng.integers(rows))))
        points.append(positions(ref, [(int(rng.integers(cols)), int(rng.integers(rows))) for _ in range(6)]))
    return case(geo, R.REFERENCE, centres, points)


@functools.lru_cache(None)
def return_against_skip(rules):
    """Case 4: [in, in, out, in]; a keyframe outside the grid; NaN and 1e30 coordinates; an empty keyframe."""
    geo = unit_geo(16, 20)
    ref = R.RefGrid(rules=rules, **geo)
    inn = positions(ref, [(3, 4), (10, 2), (7, 13), (19, 15), (0, 0)])
    out = np.array([25.0, 0.0, 3.0], np.float32)
    nan = np.array([np.nan, 0.0, 5.0], np.float32)
    big = np.array([4.0, 0.0, 1e30], np.float32)
    neg = np.array([4.0, 0.0, -0.5], np.float32)
    c = pos_of_cell(ref, 9, 8)
    assert ref.cell(out) is None and ref.cell(nan) is None and ref.cell(big) is None and ref.cell(neg) is None
    centres = [c, np.array([-3.0, 0.0, 4.0], np.float32), c, c, nan, c]
    points = [[inn[0], inn[1], out, inn[2]], [inn[0], inn[1]], [inn[3], nan, inn[4], big, inn[0], neg, inn[1]],
              np.zeros((0, 3), np.float32), [inn[0]], [inn[2]]]
    return case(geo, rules, centres, points)


def single_keyframe(rules):
    c = return_against_skip(rules)
    return case(c["geo"], rules, c["centres"][:1], c["points"][:1])


def _neighbours(p, k=4):
    out = [np.float32(p)]
    lo = hi = np.float32(p)
    for _ in range(k):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return sorted(set(float(v) for v in out))


@functools.lru_cache(None)
def cell_rule():
    """Case 5: the default geometry; per axis, the floats around the positions whose coordinate lands on 0, 1,
    size - 1 and size. Each probe is a point of one keyframe at the grid's middle (INTENDED: outside probes are
    skipped) and the centre of a keyframe of its own with one point."""
    geo = {}
    ref = R.RefGrid(rules=R.INTENDED)
    mid = pos_of_cell(ref, 3000, 3150)
    probes = []
    for axis, (lo, norm, size) in enumerate(((ref.min_x, ref.norm_x, ref.cols), (ref.min_z, ref.norm_z, ref.rows))):
        for k in (0, 1, size - 1, size):
            p0 = (k / float(norm) + float(lo)) / ref.scale
            for v in _neighbours(p0):
                p = mid.copy()
                p[2 * axis] = v
                probes.append(p)
    probes = np.array(probes, np.float32)
    centres = [mid] + list(probes)
    points = [probes] + [mid.reshape(1, 3)] * len(probes)
    return case(geo, R.INTENDED, centres, points)


def build_counters(cols=50):
    """Case 8: every 0 <= oc <= vc <= 64, oc > vc up to and past the clamp, vc = 0; as [rows, cols] arrays."""
    pairs = [(oc, vc) for vc in range(65) for oc in range(vc + 1)]
    pairs += [(oc, 100) for oc in range(100, 135)] + [(oc, 1) for oc in (2, 3, 100, 127, 128, 129, 200, 1000, 2 ** 31 - 1)]
    pairs += [(oc, 0) for oc in (0, 1, 5)] + [(3, 2), (5, 2), (2, 2), (1, 3), (-1, 1), (-2, 1), (-5, 2), (-(2 ** 31), 1), (-4, 3),
                                                   (-(2 ** 31), 7)]
    n = -(-len(pairs) // cols) * cols
    pairs += [(0, 0)] * (n - len(pairs))
    a = np.array(pairs, np.int32)
    return a[:, 0].reshape(-1, cols).copy(), a[:, 1].reshape(-1, cols).copy()


def default_beams():
    """Case 10: the default geometry under REFERENCE rules; one beam ends in the last cell."""
    ref = R.RefGrid(rules=R.REFERENCE)
    c = pos_of_cell(ref, 5900, 6200)
    pts = positions(ref, [(5999, 6299), (5950, 6100), (5800, 6250), (5900, 6200)])
    c2 = pos_of_cell(ref, 5990, 6290)
    pts2 = positions(ref, [(5999, 6299), (5920, 6280)])
    return case({}, R.REFERENCE, [c, c2], [pts, pts2])
