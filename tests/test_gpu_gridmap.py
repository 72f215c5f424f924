"""The occupancy grid on the device (include/orbfe_gridmap.h, orb_slam2_2021_amd/occupancy_grid.py), every case
bit for bit against tests/gridmap_ref.py: counters, the stats record, the dirty row range, the int8 grid and the
float grid. The cases are those of tests/gridmap_cases.py plus the ones only a device has: contention on one
line, batching against single calls, the resident path over a CovisibilityGraph, and the default 6300 x 6000
geometry (one handle shared by the two cases that need it)."""
import numpy as np
import pytest

import gridmap_cases as C
import gridmap_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(require_gpu):
    from orb_slam2_2021_amd import occupancy_grid
    return occupancy_grid


def geo_of(G, ref):
    return G.geometry(ref.scale, float(ref.min_x), float(ref.max_x), float(ref.min_z), float(ref.max_z), ref.thr)


def make(G, case, **kw):
    ref = R.RefGrid(rules=case["rules"], **dict(case["geo"], **kw))
    grid = G.OccupancyGrid(geo_of(G, ref), case["rules"])
    assert (grid.rows, grid.cols) == (ref.rows, ref.cols)
    assert np.float32(grid.norm_x) == ref.norm_x and np.float32(grid.norm_z) == ref.norm_z
    return ref, grid


def same_stats(got, want, dirty):
    assert (got.beams, got.visits, got.dropped, got.points_cut, got.kf_outside) == \
        (want.beams, want.visits, want.dropped, want.points_cut, want.kf_outside)
    assert got.rows == dirty


def same_counters(grid, ref):
    occ, vis = grid.download_counters()
    rocc, rvis = ref.counters()
    assert np.array_equal(occ, rocc)
    assert np.array_equal(vis, rvis)


def same_sparse(grid, ref):
    """The counters of a large grid, compared through their non-zero entries."""
    occ, vis = grid.download_counters()
    for a, want in zip((occ, vis), ref.sparse()):
        flat = np.flatnonzero(a)
        assert [(int(i), int(a.reshape(-1)[i])) for i in flat] == want


def check_case(G, case):
    ref, grid = make(G, case)
    want = ref.update(case["centres"], case["points"])
    got = grid.update(case["centres"], case["points"])
    same_stats(got, want, ref.dirty())
    same_counters(grid, ref)
    grid.build()
    msg, data = ref.build()
    assert np.array_equal(grid.download(), msg)
    assert np.array_equal(grid.probability().view(np.uint32), data.view(np.uint32))
    grid.close()
    return ref, want


def test_star(G):
    ref, s = check_case(G, C.star())
    assert s.beams == 129 * 129 and ref.vis[64 * 129 + 64] == 129 * 129


def test_segment_edges(G):
    _, s = check_case(G, C.segment_edges())
    assert s.beams == len(C.segment_dxs()) * 10


@pytest.mark.parametrize("rows,cols", C.CHAIN_GRIDS)
def test_chain(G, rows, cols):
    ref, s = check_case(G, C.chain(rows, cols))
    assert ref.changed_starts > 0
    if (rows, cols) == (8, 5):
        assert ref.wrapped_writes > 0
    if (rows, cols) == (5, 8):
        assert s.dropped > 0


@pytest.mark.parametrize("rules", [R.REFERENCE, R.INTENDED])
def test_return_against_skip(G, rules):
    _, s = check_case(G, C.return_against_skip(rules))
    assert s.kf_outside == 2
    _, one = check_case(G, C.single_keyframe(rules))  # n_kf = 1
    assert one.beams == (2 if rules == R.REFERENCE else 3)


@pytest.fixture(scope="module")
def default_grids(G):
    """One handle per rule set on the default geometry (340 MB of device memory each, made once)."""
    grids = {r: G.OccupancyGrid(rules=r) for r in (R.REFERENCE, R.INTENDED)}
    yield grids
    for g in grids.values():
        g.close()


def test_cell_rule(G, default_grids):
    case = C.cell_rule()
    ref = R.RefGrid(rules=R.INTENDED)
    grid = default_grids[R.INTENDED]
    assert (grid.rows, grid.cols) == (6300, 6000)
    grid.reset()
    want = ref.update(case["centres"], case["points"])
    got = grid.update(case["centres"], case["points"])
    assert want.kf_outside > 0 and want.points_cut > 0 and ref.dirty() == (0, 6300)
    same_stats(got, want, ref.dirty())
    same_sparse(grid, ref)


def test_default_geometry(G, default_grids):
    case = C.default_beams()
    ref = R.RefGrid(rules=R.REFERENCE)
    grid = default_grids[R.REFERENCE]
    grid.reset()
    want = ref.update(case["centres"], case["points"])
    got = grid.update(case["centres"], case["points"])
    same_stats(got, want, ref.dirty())
    r0, r1 = got.rows
    assert r1 == 6300 and r0 > 5900  # the last cell is touched; only a few hundred rows are dirty
    occ, vis = grid.download_counters(r0, r1)
    rocc, rvis = ref.counters(r0, r1)
    assert np.array_equal(occ, rocc) and np.array_equal(vis, rvis)
    assert occ[-1, -1] == 2 and vis[-1, -1] >= 2
    grid.build()
    assert np.array_equal(grid.download(r0, r1), ref.build(r0, r1)[0])
    assert not grid.download(0, r0).any()  # nothing outside the dirty rows was written


def test_contention(G):
    geo = C.unit_geo(64, 64)
    ref = R.RefGrid(rules=R.INTENDED, **geo)
    c = C.pos_of_cell(ref, 3, 5)
    p = C.pos_of_cell(ref, 60, 41)
    one = R.RefGrid(rules=R.INTENDED, **geo)
    one.update([c], [[p]])
    grid = G.OccupancyGrid(geo_of(G, ref), R.INTENDED)
    s = grid.update([c], [np.tile(p, (4096, 1))])
    occ, vis = grid.download_counters()
    rocc, rvis = one.counters()
    assert s.beams == 4096 and s.visits == 4096 * int(rvis.sum())
    assert np.array_equal(vis, 4096 * rvis) and np.array_equal(occ, 4096 * rocc)
    assert occ[41, 60] == 4096 and vis[41, 60] == 4096 and vis[5, 3] == 4096
    grid.close()


def test_batching_reset_and_dirty_build(G):
    rows, cols = 40, 50
    geo = C.unit_geo(rows, cols)
    rng = np.random.default_rng(7)
    ref = R.RefGrid(rules=R.REFERENCE, **geo)
    centres, points = [], []
    for k in range(5):
        centres.append(C.pos_of_cell(ref, int(rng.integers(10, 30)), int(rng.integers(10, 30))))  # transposed states stay in 10..29
        points.append(C.positions(ref, [(int(rng.integers(10, 30)), int(rng.integers(10, 30))) for _ in range(40 + 13 * k)]))
    batch = G.OccupancyGrid(geo_of(G, ref), R.REFERENCE)
    single = G.OccupancyGrid(geo_of(G, ref), R.REFERENCE)
    want = ref.update(centres, points)
    got = batch.update(centres, points)
    same_stats(got, want, ref.dirty())
    parts = [single.update([c], [p]) for c, p in zip(centres, points)]
    assert sum(s.beams for s in parts) == want.beams and sum(s.visits for s in parts) == want.visits
    assert sum(s.dropped for s in parts) == want.dropped
    assert parts[-1].rows == ref.dirty()  # accumulated over the calls since the last build
    same_counters(batch, ref)
    same_counters(single, ref)
    r0, r1 = ref.dirty()
    assert 0 < r0 and r1 < rows  # some rows stay clean, so the dirty build is a part of the grid
    batch.build()
    assert np.array_equal(batch.download(), ref.build()[0])  # dirty rows only, equal to the full message
    assert batch.update(centres[:1], [points[0][:0]]).rows == (0, 0)  # the build cleared the range
    batch.reset()
    ref.reset()
    same_counters(batch, ref)
    assert not batch.download().any()
    got = batch.update(centres[::-1], points[::-1])
    same_stats(got, ref.update(centres[::-1], points[::-1]), ref.dirty())
    same_counters(batch, ref)
    batch.build(all_rows=True)
    assert np.array_equal(batch.download(), ref.build()[0])
    batch.close()
    single.close()


@pytest.mark.parametrize("thr", [0, 2])
def test_build(G, thr):
    occ, vis = C.build_counters()
    rows, cols = occ.shape
    ref = R.RefGrid(visit_threshold=thr, **C.unit_geo(rows + 2, cols))
    grid = G.OccupancyGrid(geo_of(G, ref))
    grid.upload_counters(1, occ, vis)
    o2, v2 = grid.download_counters(1, rows + 1)
    assert np.array_equal(o2, occ) and np.array_equal(v2, vis)
    grid.build()
    msg, data = R.build(occ, vis, thr)
    assert np.array_equal(grid.download(1, rows + 1), msg)
    assert np.array_equal(grid.probability(1, rows + 1).view(np.uint32), data.view(np.uint32))
    assert not grid.download(0, 1).any() and not grid.download(rows + 1, rows + 2).any()
    assert {127, -128, 0, 100} <= set(int(m) for m in msg.reshape(-1))
    grid.close()


def test_resident(G):
    from orb_slam2_2021_amd import CovisibilityGraph, OrbfeError
    from orb_slam2_2021_amd import _lib as L
    rows, cols = 30, 36
    geo = C.unit_geo(rows, cols)
    rng = np.random.default_rng(11)
    ref = R.RefGrid(rules=R.REFERENCE, **geo)
    n_points = 400
    pos = C.positions(ref, [(int(rng.integers(cols)), int(rng.integers(rows))) for _ in range(n_points)])
    pos[17] = [99.0, 0.0, 3.0]  # one point outside the grid: REFERENCE rules end a keyframe there
    graph = CovisibilityGraph(8, 320, n_points + 1)
    rows_of = {}
    for kf, n_slots in ((3, 300), (5, 257), (9, 64)):
        row = rng.integers(0, n_points, n_slots).astype(np.int32)
        row[rng.random(n_slots) < 0.2] = -1
        if kf == 9:
            row[40] = 17
        row[row == n_points] = -1
        rows_of[kf] = row
        graph.set_keyframe(kf, row)
    bad = int(rows_of[3][rows_of[3] >= 0][5])
    graph.set_points_bad([bad])
    ids = np.arange(n_points)
    graph.set_point_geometry(ids, pos, np.zeros((n_points, 3)), np.ones(n_points), np.ones(n_points),
                             np.zeros((n_points, 32), np.uint8))
    kf_ids = [5, 3, 9]
    centres = [C.pos_of_cell(ref, int(rng.integers(cols)), int(rng.integers(rows))) for _ in kf_ids]
    points = []
    for kf in kf_ids:
        r = rows_of[kf]
        points.append(pos[[p for p in r if p >= 0 and p != bad]])
    assert any(bad in rows_of[k] for k in kf_ids) and any((r == -1).any() for r in rows_of.values())
    want = ref.update(centres, points)
    assert want.points_cut > 0
    for rules in (R.REFERENCE,):
        host = G.OccupancyGrid(geo_of(G, ref), rules)
        res = G.OccupancyGrid(geo_of(G, ref), rules)
        same_stats(host.update(centres, points), want, ref.dirty())
        same_stats(res.update_resident(graph, kf_ids, centres), want, ref.dirty())
        same_counters(res, ref)
        same_counters(host, ref)
        # a point without geometry: the call is refused before any counter is touched
        extra = rows_of[9].copy()
        extra[3] = n_points
        graph.set_keyframe(9, extra)
        with pytest.raises(OrbfeError) as e:
            res.update_resident(graph, kf_ids, centres)
        assert e.value.status == L.ORBFE_ERR_STATE and e.value.n_missing == 1
        same_counters(res, ref)
        with pytest.raises(OrbfeError) as e:
            res.update_resident(graph, [5, 4], centres[:2])  # 4 is not stored
        assert e.value.status == L.ORBFE_ERR_ARG
        host.close()
        res.close()
    graph.close()


def test_bounds_are_checked_before_any_device_work(G):
    from orb_slam2_2021_amd import OrbfeError
    from orb_slam2_2021_amd import _lib as L
    ref = R.RefGrid(**C.unit_geo(8, 8))
    grid = G.OccupancyGrid(geo_of(G, ref))
    c = C.pos_of_cell(ref, 1, 1)
    for centres, points, status in (([c] * 4097, [np.zeros((0, 3))] * 4097, L.ORBFE_ERR_CAPACITY),
                                    ([c], [np.tile(c, (8193, 1))], L.ORBFE_ERR_CAPACITY),
                                    (np.zeros((0, 3)), [], L.ORBFE_ERR_ARG)):
        with pytest.raises(OrbfeError) as e:
            grid.update(centres, points)
        assert e.value.status == status
    occ, vis = grid.download_counters()
    assert not occ.any() and not vis.any()
    assert grid.update([c], [np.tile(c, (8192, 1))]).beams == 8192  # the bound itself is served
    grid.close()


def repeated(G, grid, ref_kw, rules, centre_cell, spread, times, seed):
    """One keyframe of 8,192 random points near its centre, named `times` times in one call: the counters are `times`
    times one keyframe's (a keyframe's beams depend on nothing outside it under either rule set)."""
    one = R.RefGrid(rules=rules, **ref_kw)
    rng = np.random.default_rng(seed)
    cx, cz = centre_cell
    c = C.pos_of_cell(one, cx, cz)
    pts = C.positions(one, [(cx + int(rng.integers(-spread, spread + 1)), cz + int(rng.integers(-spread, spread + 1)))
                            for _ in range(8192)])
    want = one.update([c], [pts])
    got = grid.update([c] * times, [pts] * times)
    assert (got.beams, got.visits, got.dropped, got.points_cut, got.kf_outside) == \
        (times * want.beams, times * want.visits, times * want.dropped, 0, 0)
    assert got.rows == one.dirty()
    r0, r1 = got.rows
    occ, vis = grid.download_counters(r0, r1)
    rocc, rvis = one.counters(r0, r1)
    assert np.array_equal(occ, times * rocc) and np.array_equal(vis, times * rvis)
    assert int(grid.download_counters()[1].sum(dtype=np.int64)) == times * want.visits  # nothing outside those rows


def test_more_points_than_one_group(G):
    """33 x 8,192 points: the first 32 keyframes fill a group of 2^18 points exactly, the last starts another."""
    geo = C.unit_geo(64, 64)
    ref = R.RefGrid(rules=R.REFERENCE, **geo)
    grid = G.OccupancyGrid(geo_of(G, ref), R.REFERENCE)
    repeated(G, grid, geo, R.REFERENCE, (30, 33), 20, 33, 5)
    grid.close()


def test_more_beams_than_one_sub_range(G, default_grids):
    """6 x 8,192 beams on the default grid, whose longest beam has 99 segments: a sub-range holds 2^22 / 99 = 42,366
    beams, so the group is scattered in two passes and the cut falls inside a keyframe."""
    grid = default_grids[R.INTENDED]
    grid.reset()
    repeated(G, grid, {}, R.INTENDED, (5000, 400), 40, 6, 6)
