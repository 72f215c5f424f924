"""The two CPU statements of Frame::ComputeStereoMatches (src/Frame.cc:522-700) against each other
on the hand-built cases of tests/stereo_scenes.py: tests/stereo_ref.py (NumPy, written from the
routine's steps) and oracle/orbref.cpp's orbref_compute_stereo_matches (the restatement every GPU
stereo test compares with), over RefExtractor pyramids of each case's images.

  * bit for bit equal (u_right, depth) on every case;
  * each case produces the outcome, winner, distance, shift and SADs it is named for;
  * every outcome code of stereo_ref is produced somewhere, or is proven unreachable in writing.
"""
import functools

import numpy as np
import pytest

import stereo_ref
import stereo_scenes as scenes
from oracle import orbref
from oracle.orbref import RefExtractor

CASES = scenes.single_cases() + scenes.batch_pairs()


@functools.lru_cache(maxsize=None)
def solved(i):
    c = CASES[i]
    E1, E2 = RefExtractor(500, c.sf, c.nlevels, 20, 7), RefExtractor(500, c.sf, c.nlevels, 20, 7)
    E1(c.left)
    E2(c.right)
    T = E1.tables()
    pl = [E1.level(l) for l in range(c.nlevels)]
    pr = [E2.level(l) for l in range(c.nlevels)]
    assert np.array_equal(np.asarray(T["scale"], np.float32).view(np.uint32), c.scale.view(np.uint32))
    assert np.array_equal(np.asarray(T["inv_scale"], np.float32).view(np.uint32), c.inv_scale.view(np.uint32))
    ref = stereo_ref.compute_stereo_matches(c.kl, c.dl, c.kr, c.dr, pl, pr, c.scale, c.inv_scale, c.mb, c.mbf)
    ora = orbref.compute_stereo_matches(c.kl, c.dl, c.kr, c.dr, pl, pr, T["scale"], T["inv_scale"], c.mb, c.mbf)
    return ref, ora


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c in CASES])
def test_the_two_references_agree_on_the_bits(i):
    ref, (ur, dep) = solved(i)
    for name, a, b in (("u_right", ref["u_right"], ur), ("depth", ref["depth"], dep)):
        bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
        assert len(bad) == 0, f"{CASES[i].name} {name}: keypoints {bad[:8].tolist()} stereo_ref " \
                              f"{a[bad[:8]].tolist()} oracle {b[bad[:8]].tolist()} " \
                              f"({[ref['outcome'][k] for k in bad[:8]]})"


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c in CASES])
def test_each_case_takes_the_branch_it_is_named_for(i):
    assert CASES[i].expect or len(CASES[i].kl) == 0
    scenes.check_expect(CASES[i], solved(i)[0])


def test_every_outcome_code_is_reached():
    hit = set()
    for i in range(len(CASES)):
        hit.update(solved(i)[0]["outcome"])
    assert None not in hit
    missing = set(stereo_ref.OUTCOMES) - hit - set(scenes.EXEMPT)
    assert not missing, f"no case reaches {sorted(missing)}"
    assert not (hit & set(scenes.EXEMPT)), "an outcome listed as unreachable was reached"
    assert set(scenes.EXEMPT) == {"delta_out"}


def test_sad_totals_on_both_sides_of_two_to_the_15():
    i = [c.name for c in CASES].index("sad_binary")
    s = solved(i)[0]["sads"]
    s = s[s >= 0]
    assert s.max() == 120 * 510 and ((s > 2 ** 15) & (s < 2 ** 15 + 256)).any() and \
        ((s < 2 ** 15) & (s > 2 ** 15 - 256)).any()


def test_median_cases_cover_the_counts():
    got = {}
    for i, c in enumerate(CASES):
        if c.name.startswith("median_"):
            o = solved(i)[0]["outcome"]
            got[c.name] = sum(x in ("accepted", "median_rejected") for x in o)
    assert got["median_M0"] == 0 and got["median_M1_sad0"] == 1 and got["median_M2"] == 2
    assert got["median_odd"] % 2 == 1 and got["median_even"] % 2 == 0 and got["median_high_byte"] > 256


def test_table_shapes_sit_where_they_are_named():
    by = {c.name: c for c in CASES}
    n = lambda c: c.nlevels * (c.left.shape[0] + 1)
    assert n(by["band_row_only_table"]) > 16384 and n(by["band_table_at_16384"]) == 16384
    assert n(by["band_8_levels"]) < 16384 - 16
