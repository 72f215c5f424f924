"""k_octree held to the hand-built key sets (tests/octree_scenes.py) and the second reference
(tests/octree_ref.py): the assertions of tests/test_octree_ref.py with the kernel in the oracle's
place, and no import of the oracle.

Each scene is an image of isolated dots, extracted with one pyramid level, so the level's budget is
nfeatures and k_fast hands k_octree exactly the scene's keys. debug_candidates(0) is checked as a set
against the scene and fed, in the kernel's own order, to octree_ref.distribute; the result is compared
in order with debug_level_keys(0) and with the keypoints, and for the hand-built scenes with the
written-out survivors. Every arm runs all hand-built and large-node scenes and a third of the
random ones (those whose budget the kernel's LDS plan takes: see MAX_N).
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import definition_ref as D
import octree_ref as O
import octree_scenes as S
from orb_slam2_2021_amd import ORBextractor
from orb_slam2_2021_amd import _lib as L

pytestmark = pytest.mark.gpu

# k_octree keeps its node arena in LDS, sized by the level's budget: a single level takes a budget of
# about 1900 at the most, above that the extract call returns ORBFE_ERR_ARG ("image too large for the
# octree LDS plan"). The scenes with N = 5000 therefore stay with the CPU suite (oracle against
# octree_ref); N = 1500 is their stand-in here: like 5000 it exceeds every scene's key count, so the
# same branch runs (no node is left with two keys).
MAX_N = 1500
HAND = S.hand_scenes()
SCENES = HAND + [s for s in S.large_scenes() if s.N <= MAX_N] + [s for s in S.random_scenes() if s.N <= MAX_N][::3]

# settings of one handle, and how the scene's image reaches it
ARMS = {
    "default": dict(),
    "global_keys": dict(key_cap=0),
    "threads_256": dict(threads=(256, 256)),
    "threads_1024": dict(threads=(1024, 1024)),
    "serial_1": dict(serial=(1, 1)),
    "serial_128": dict(serial=(128, 128)),
    "batch_of_3": dict(call="batch3"),
    "device_batch_of_8": dict(call="device8"),
    "device_batch_of_8_one_launch": dict(call="device8", split=0),
}


def make_extractor(n, arm):
    ext = ORBextractor(n, 1.2, 1, 20, 7)
    if "key_cap" in arm:
        ext.debug_set_octree_key_cap(arm["key_cap"])
    if "threads" in arm:
        ext.debug_set_octree_threads(*arm["threads"])
    if "serial" in arm:
        ext.debug_set_octree_serial(*arm["serial"])
    if "split" in arm:
        ext.debug_set_octree_split(arm["split"])
    return ext


def device_batch(ext, imgs):
    import torch
    imgs = np.stack(imgs)
    n, rows, cols = imgs.shape
    cap = ext.max_keypoints(rows, cols)
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(imgs).to(dev)
    kps = torch.empty(n * cap * L.KEYPOINT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    desc = torch.empty(n * cap * 32, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    ext.extract_batch_device(n, d_in.data_ptr(), rows * cols, rows, cols, cols, kps.data_ptr(), desc.data_ptr(),
                             cap, cnt.data_ptr())
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    k = kps.cpu().numpy().view(L.KEYPOINT_DTYPE).reshape(n, cap)
    return [k[i, :c[i]] for i in range(n)]


def check_image(ext, idx, kps, sc, keys_of_image=None, expect=None):
    """One image of the handle's last call: candidates vs the designed keys, survivors and keypoints vs
    octree_ref from the kernel's own candidates, and vs the written-out survivors where there are any."""
    tag = f"{sc.name} image {idx}"
    cand = D.unpack_keys(ext.debug_candidates(0, image=idx))
    if keys_of_image is not None:
        assert len(cand) == len(keys_of_image) and set(cand) == set(keys_of_image), f"{tag}: candidates are not the scene's keys"
    want = O.distribute(cand, sc.w, sc.h, sc.N)
    got = [(x - S.BORDER, y - S.BORDER, r) for x, y, r in D.unpack_keys(ext.debug_level_keys(0, image=idx))]
    assert got == want, (f"{tag}: {len(got)} survivors vs {len(want)}, first difference at "
                         f"{next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))}")
    if expect is not None:
        assert got == expect, f"{tag}: not the written-out survivors"
    assert len(kps) == len(want), f"{tag}: keypoint count"
    assert [(int(k["x"]) - S.BORDER, int(k["y"]) - S.BORDER, int(k["response"])) for k in kps] == want, f"{tag}: keypoints"
    assert not np.any(kps["octave"]), f"{tag}: octave"


def flips(sc):
    """The scene's image mirrored three ways with the keys of each: other key sets of the same shape."""
    w, h = sc.w, sc.h
    img = sc.image()
    return [(img[:, ::-1], [(w - 1 - x, y, r) for x, y, r in sc.keys]),
            (img[::-1, :], [(x, h - 1 - y, r) for x, y, r in sc.keys]),
            (img[::-1, ::-1], [(w - 1 - x, h - 1 - y, r) for x, y, r in sc.keys])]


@pytest.mark.parametrize("arm", list(ARMS), ids=list(ARMS))
def test_octree_scenes(require_gpu, arm):
    cfg = ARMS[arm]
    handles = {}
    try:
        for sc in SCENES:
            ext = handles.get(sc.N)
            if ext is None:
                ext = handles[sc.N] = make_extractor(sc.N, cfg)
            img = sc.image()
            call = cfg.get("call")
            if call is None:
                check_image(ext, 0, ext(img)[0], sc, sc.keys, sc.expect)
                continue
            other = flips(sc)
            if call == "batch3":
                between = other[:1]
                imgs = [img] + [np.ascontiguousarray(o[0]) for o in between] + [img]
                outs = [o[0] for o in ext.extract_batch(imgs)]
            else:
                between = other + other
                imgs = [img] + [np.ascontiguousarray(o[0]) for o in between] + [img]
                outs = device_batch(ext, imgs)
            last = len(imgs) - 1
            for i in reversed(range(len(imgs))):
                if i in (0, last):
                    check_image(ext, i, outs[i], sc, sc.keys, sc.expect)
                else:
                    check_image(ext, i, outs[i], sc, between[i - 1][1])
    finally:
        for ext in handles.values():
            ext.close()


def test_designated_tie_case_is_the_creation_rule(require_gpu):
    """Equal sizes in the refinement's sort: the kernel divides the later-created node first (the
    project's decision), and the opposite order would give another answer."""
    sc = next(s for s in HAND if s.tie)
    with make_extractor(sc.N, {}) as ext:
        kps, _ = ext(sc.image())
        got = [(x - S.BORDER, y - S.BORDER, r) for x, y, r in D.unpack_keys(ext.debug_level_keys(0))]
    assert got == sc.expect and len(kps) == len(got)
    assert got != O.distribute(sc.keys, sc.w, sc.h, sc.N, "reverse")


@pytest.mark.parametrize("shape", [(200, 90), (48, 1100), (62, 1968)])
def test_rejected_aspect_ratios(require_gpu, shape):
    """Shapes the octree cannot take return ORBFE_ERR_ARG from the extract call: 200 x 90 has a border
    area of 58 x 168, ratio 0.35, nIni = 0; 62 x 1968 one of 1936 x 30, ratio 64.53, nIni = 65; the
    48 x 1100 strip (ratio 66.75) is refused one line earlier, because its border area is 16 high, under
    the 30 px a FAST cell needs. The entry points call compute_geometry right after their argument
    checks and return its status; it refuses these shapes inside its first loop over the levels, before
    it allocates, copies or plans anything, and no launch comes before it -- read from the source,
    nothing here runs such a shape any other way."""
    rows, cols = shape
    img = np.zeros(shape, np.uint8)
    with ORBextractor(100, 1.2, 1, 20, 7) as ext:
        cap = 4096
        kps = np.zeros(cap, L.KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = ctypes.c_int(-1)
        st = ext._lib.orbfe_extract(ext._h, L.ptr(img), rows, cols, ctypes.c_size_t(cols), L.ptr(kps), cap,
                                    L.ptr(desc), ctypes.byref(n))
        assert st == L.ORBFE_ERR_ARG
        if shape != (48, 1100):
            assert "aspect ratio" in L.last_error()
        with pytest.raises(L.OrbfeError) as e:
            ext(img)
        assert e.value.status == L.ORBFE_ERR_ARG
        ok = dataclasses.replace(HAND[0], N=100)  # the handle still serves a shape it can take
        check_image(ext, 0, ext(ok.image())[0], ok, ok.keys)
