"""The extractor kernels' stage outputs held to the stages' definitions (tests/definition_ref.py).

The same assertions as tests/test_definition_oracle.py with the kernels in the oracle's place, and no
import of the oracle: k_copy0 / k_pyramid / k_resize_win through ext.level(l), k_blur through
ext.debug_blurred(l), k_fast through ext.debug_candidates(l), k_describe through the angles and
descriptors ext(img) returns. Each stage is fed what the kernel consumed (the definition's resize of
the kernel's own previous level, the blur of its own level, the descriptor from its own blurred level
and angle), so a failure names its stage and does not compound.

Paths: a single-image call builds levels 1.. in one k_pyramid launch; a batch of 8 builds them with
one k_resize_win launch per level; both in both resize rounding forms. The two figures taken from the
oracle (blur mean difference, fast_atan2 sweep error) are definition_ref's recorded constants, pinned
to the oracle by the CPU suite.
"""
import functools

import numpy as np
import pytest

import definition_ref as D
from orb_slam2_2021_amd import ORBextractor, synth_frame, ORBFE_RESIZE_SCALAR, ORBFE_RESIZE_SIMD128
from orb_slam2_2021_amd import _lib as L

pytestmark = pytest.mark.gpu

PARAMS = {"noise": (500, D.PYRAMID[0], D.PYRAMID[1], 20, 7),
          "texture": (500, D.PYRAMID[0], D.PYRAMID[1], 20, 7),
          "plateau": (500, 1.2, 1, 20, 7)}
CASES = [("small", ORBFE_RESIZE_SIMD128), ("small", ORBFE_RESIZE_SCALAR),
         ("batch", ORBFE_RESIZE_SIMD128), ("batch", ORBFE_RESIZE_SCALAR)]
BATCH = 8  # the smallest call that takes the batch plan


def names(mode):
    # the plateau image has one level: nothing of it depends on the resize form
    return ("noise", "texture", "plateau") if mode == ORBFE_RESIZE_SIMD128 else ("noise", "texture")


@functools.lru_cache(maxsize=None)
def image(name):
    if name == "noise":
        return D.noise_image()
    if name == "plateau":
        return D.plateau_image()
    return np.ascontiguousarray(synth_frame(0, 376, 1241)[50:50 + D.NOISE_SHAPE[0], 600:600 + D.NOISE_SHAPE[1]])


def _batch(name):
    """(images, index of `name` in them): the image under test last or first, other images between."""
    if name == "plateau":
        other = np.ascontiguousarray(image("plateau")[::-1, ::-1])
        return [other] * (BATCH - 1) + [image("plateau")], BATCH - 1
    rng = np.random.default_rng(5)
    fill = [rng.integers(0, 256, D.NOISE_SHAPE, dtype=np.uint8) for _ in range(BATCH - 2)]
    return [image("texture")] + fill + [image("noise")], (BATCH - 1 if name == "noise" else 0)


@functools.lru_cache(maxsize=None)
def _extract(path, mode, group):
    ext = ORBextractor(*PARAMS[group])
    ext.set_resize_mode(mode)
    if path == "small":
        return ext, [ext(image(group))]
    return ext, ext.extract_batch(_batch(group)[0])


@functools.lru_cache(maxsize=None)
def run(path, mode, name):
    """The stage outputs of one image of one call, per level."""
    if path == "small":
        ext, outs = _extract(path, mode, name)
        idx = 0
        # the handle keeps the last call's stages only: one handle per image on this path
    else:
        ext, outs = _extract(path, mode, "plateau" if name == "plateau" else "noise")
        idx = _batch(name)[1]
    kps, desc = outs[idx]
    umax = np.zeros(16, np.int32)
    L.check(ext._lib.orbfe_debug_get_umax(ext._h, L.ptr(umax)), "debug_get_umax")
    n = ext.nlevels
    out = {"levels": [ext.level(l, image=idx) for l in range(n)],
           "blurred": [ext.debug_blurred(l, image=idx) for l in range(n)],
           "cand": [ext.debug_candidates(l, image=idx) for l in range(n)],
           "keys": [ext.debug_level_keys(l, image=idx) for l in range(n)],
           "umax": umax, "kps": [], "desc": []}
    for l in range(n):
        sel = kps["octave"] == l
        out["kps"].append(kps[sel])
        out["desc"].append(desc[sel] if desc is not None else np.zeros((0, 32), np.uint8))
        assert len(out["keys"][l]) == int(sel.sum()), f"level {l}: octree survivors vs keypoints"
    return out


@functools.lru_cache(maxsize=None)
def _candidates_of(shape, data, ini_th, min_th):
    return D.fast_cell_candidates(np.frombuffer(data, np.uint8).reshape(shape), ini_th, min_th)


def test_umax_is_the_circle(require_gpu):
    ext = ORBextractor(*PARAMS["plateau"])
    umax = np.zeros(16, np.int32)
    L.check(ext._lib.orbfe_debug_get_umax(ext._h, L.ptr(umax)), "debug_get_umax")
    # ORBextractor.cc:457-472: the half-widths of the rows of a discretised circle of radius 15
    assert umax.tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


@pytest.mark.parametrize("path,mode", CASES)
def test_pyramid(require_gpu, path, mode):
    """k_copy0: level 0 is the image. k_pyramid / k_resize_win: every further level against the exact
    bilinear resize of the kernel's own previous level, within definition_ref.resize_bounds."""
    for name in ("noise", "texture"):
        r = run(path, mode, name)
        assert np.array_equal(r["levels"][0], image(name)), f"{name}: level 0 is not the image"
        for l in range(1, len(r["levels"])):
            src = r["levels"][l - 1]
            dh, dw = D.level_shape(image(name).shape, PARAMS[name][1], l)
            assert r["levels"][l].shape == (dh, dw), f"{name}: level {l} shape"
            d = r["levels"][l].astype(np.float64) - D.resize_bilinear(src, dw, dh)
            lo, hi = D.resize_bounds(mode == ORBFE_RESIZE_SIMD128, src.shape)
            print(f"resize {path} mode {mode} {name} level {l}: kernel - exact in [{d.min():.4f}, {d.max():.4f}], "
                  f"bound ({lo:.4f}, {hi:.4f})")
            assert lo < d.min() and d.max() < hi, \
                f"{name} level {l}: first at {np.argwhere((d <= lo) | (d >= hi))[:5].tolist()}"


@pytest.mark.parametrize("path,mode", CASES)
def test_blur(require_gpu, path, mode):
    """k_blur against the exact Gaussian of the kernel's own level: the derived per-pixel bound on
    every level, and on the noise image's level 0 a mean difference of at most 1.5 x the oracle's."""
    bound = D.blur_bound()
    for name in names(mode):
        r = run(path, mode, name)
        for l, (lev, bl) in enumerate(zip(r["levels"], r["blurred"])):
            d = np.abs(bl.astype(np.float64) - D.gaussian_blur(lev))
            print(f"blur {path} mode {mode} {name} level {l}: max {d.max():.4f} mean {d.mean():.5f}")
            assert d.max() <= bound, f"{name} level {l}: {d.max()} at {np.argwhere(d > bound)[:5].tolist()}"
            if name == "noise" and l == 0:
                assert d.mean() <= 1.5 * D.ORACLE_BLUR_MEAN_ABS, f"mean difference {d.mean()}"


@pytest.mark.parametrize("path,mode", CASES)
def test_fast_candidates(require_gpu, path, mode):
    """k_fast: the decoded (x, y, response) candidates of every level equal, as a set, the definition's
    per-cell FAST with strict non-maximum suppression on the kernel's own level."""
    for name in names(mode):
        r = run(path, mode, name)
        _, _, _, ini_th, min_th = PARAMS[name]
        for l, lev in enumerate(r["levels"]):
            want = _candidates_of(lev.shape, lev.tobytes(), ini_th, min_th)
            got = D.unpack_keys(r["cand"][l])
            assert len(want) > 20 and len(set(got)) == len(got)
            assert set(got) == set(want), (f"{name} level {l}: {len(got)} vs {len(want)}; only kernel "
                                           f"{sorted(set(got) - set(want))[:5]}, only definition "
                                           f"{sorted(set(want) - set(got))[:5]}")


@pytest.mark.parametrize("path,mode", CASES)
def test_angles(require_gpu, path, mode):
    """k_describe's orientation: within twice the oracle's fast_atan2 sweep error of atan2(m01, m10)
    of the exact moments of the kernel's own level."""
    bound = 2.0 * D.ORACLE_ATAN2_SWEEP_MAX_DEG
    for name in names(mode):
        r = run(path, mode, name)
        n = 0
        for l, lev in enumerate(r["levels"]):
            xs, ys, _ = (np.array(v, np.int64) for v in zip(*D.unpack_keys(r["keys"][l])))
            d = D.angle_diff_deg(r["kps"][l]["angle"], D.ic_angle_deg(lev, xs, ys, r["umax"]))
            assert d.max() <= bound, f"{name} level {l}: {d.max()} degrees at key {int(d.argmax())}"
            n += len(xs)
        assert n >= 30


@pytest.mark.parametrize("path,mode", CASES)
def test_descriptors(require_gpu, path, mode):
    """k_describe's bits: every test not within 1e-3 of a rounding tie equals the steered BRIEF of the
    kernel's own blurred level at the kernel's own angle; at most 2 % of a run's tests are ties."""
    pat = D.pattern31()
    for name in names(mode):
        r = run(path, mode, name)
        tests = masked = wrong = 0
        for l in range(len(r["levels"])):
            got = D.descriptor_bits(r["desc"][l])
            for k, (x, y, _) in enumerate(D.unpack_keys(r["keys"][l])):
                desc, mask = D.steered_brief(r["blurred"][l], x, y, float(r["kps"][l]["angle"][k]), pat)
                wrong += int(((got[k] != D.descriptor_bits(desc)[0]) & ~mask).sum())
                masked += int(mask.sum())
                tests += 256
        print(f"descriptors {path} mode {mode} {name}: {tests} tests, {100.0 * masked / tests:.3f} % masked, "
              f"{wrong} wrong")
        assert tests >= 30 * 256
        assert masked <= 0.02 * tests, f"{name}: {masked} of {tests} tests masked"
        assert wrong == 0, f"{name}: {wrong} bits differ"
