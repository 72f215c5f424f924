"""k_frustum and k_proj_queries on the edges of their visibility rules (tests/frustum_scenes.py):
ORBmatcher.isInFrustum / SearchLocalPoints against tests/frustum_ref.py on all six outputs, once more
with the geometry resident on the device, and the five projection searches through the probe target
against frustum_ref's expected best_idx and against the oracle -- on every hand-built case, on the
tiled sizes and on the near-threshold maps, bit for bit."""
import numpy as np
import pytest

from orb_slam2_2021_amd import MPF_TRACK_IN_VIEW, ORBmatcher
from orb_slam2_2021_amd.frames import DeviceMapPointGeometry

import frustum_ref as FR
import frustum_scenes as FS
from test_frustum_ref import FIELDS, sized
from test_gpu_match_edges import Gpu

pytestmark = pytest.mark.gpu

RIGS = {r.name: r for r in FS.rigs()}
GENERAL = {r.name: r for r in FS.rigs(general=True)}
FRUSTUM = [n for n, r in RIGS.items() if r.func == "frustum"]
SEARCHES = [n for n, r in RIGS.items() if r.func != "frustum"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.itemsize}")


def check_frustum(rig, G, cos_limit=0.5, resident=False):
    """isInFrustum and SearchLocalPoints' frustum half against frustum_ref; where the reference
    writes nothing (not in view) the five members are not compared."""
    want = FR.is_in_frustum(rig.target, G, rig.tcw, rig.lsf, cos_limit)
    inv = (want["flags"] & MPF_TRACK_IN_VIEW) > 0
    m = ORBmatcher(0.8, True)
    arg = G
    if resident:
        import torch
        arg = DeviceMapPointGeometry(G, device=torch.device("cuda", 0))
    sf = rig.cfg[0]
    nv, lm = m.isInFrustum(rig.target, arg, cos_limit, scale_factor=sf)
    _, _, nv2, lm2 = m.SearchLocalPoints(rig.target, arg, 3.0, cos_limit, scale_factor=sf)
    for n, got in ((nv, lm), (nv2, lm2)):
        assert n == want["n_in_view"]
        assert np.array_equal(got.flags, want["flags"]), np.flatnonzero(got.flags != want["flags"])[:5]
        for f in FIELDS:
            bad = np.flatnonzero(bits(getattr(got, f))[inv] != bits(want[f])[inv])
            assert len(bad) == 0, f"{rig.name} {f}: {len(bad)} differ, first {bad[:5].tolist()}"


def check_searches(rig, G):
    gpu = Gpu()   # every call is also compared with the oracle
    for part, up, down in FS.probe_searches(rig, G):
        for s in (up, down):
            got = s.run(gpu)
            bad = np.flatnonzero(got != s.expect)
            assert len(bad) == 0, f"{rig.name}: best_idx differs at MapPoints {part[bad[:5]].tolist()}: " \
                                  f"{got[bad[:5]]} / {s.expect[bad[:5]]}"


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("cos_limit", [0.5, FS.QUARTER_LIMIT])
@pytest.mark.parametrize("name", FRUSTUM)
def test_frustum_cases(require_gpu, name, cos_limit, resident):
    rig = RIGS[name]
    check_frustum(rig, FS.build(rig, FS.cases(rig.cfg)), cos_limit, resident)


def test_frustum_one_level(require_gpu):
    rig = FS._rigid("frustum_one_level", "frustum", (1.2, 1), True)
    check_frustum(rig, FS.build(rig, FS.cases(FS.CFG_A)))


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("share", ["mixed", "all", "none", "last"])
def test_frustum_sizes(require_gpu, share, resident):
    rig = RIGS["frustum"]
    for m in FS.SIZES:
        if m == 0 and resident:
            continue
        G, want_n = sized(rig, m, share)
        check_frustum(rig, G, 0.5, resident)
        assert FR.is_in_frustum(rig.target, G, rig.tcw, rig.lsf)["n_in_view"] == want_n


@pytest.mark.parametrize("name", SEARCHES)
def test_search_cases(require_gpu, name):
    rig = RIGS[name]
    check_searches(rig, FS.build(rig, FS.cases(rig.cfg)))


@pytest.mark.parametrize("name", [n for n in SEARCHES if RIGS[n].cfg == FS.CFG_B])
def test_window_edge_at_level_three(require_gpu, name):
    gpu = Gpu()
    for s, want in FS.window_searches(RIGS[name]):
        assert s.run(gpu).tolist() == [want] == s.expect.tolist()


@pytest.mark.parametrize("name", list(GENERAL))
def test_near_threshold_map(require_gpu, name):
    rig = GENERAL[name]
    G, _ = FS.near_map(rig)
    if rig.func == "frustum":
        check_frustum(rig, G)
        check_frustum(rig, G, resident=True)
    else:
        check_searches(rig, G)
