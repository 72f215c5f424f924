"""k_rectify_plan and k_rectify (orbfe_rectify_plan_create, orbfe_rectify_batch_device) on every byte: the device,
the host entry points (orbfe_remap_host, orbfe_rectify_entries_host) and tests/rectify_ref.py must agree bit
for bit. Hand-built maps on an 8 x 6 source; small destination widths around the kernel's four-byte groups and
64-lane waves with unaligned pitches, a side-by-side source and a sentinel around every destination row, for
1, 3 and 4 channels with gray fused and with colour out, in a batch of 3 pairs on one plan with row0 > 0; the
arducam cameras at 640 x 480 and a calibration that leaves the source."""
import numpy as np
import pytest

import rectify_ref as R
from rectify_cases import hand_maps, random_maps

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ext(require_gpu):
    from orb_slam2_2021_amd import ORBextractor
    e = ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    yield e
    e.close()


def same_entries(got, want):
    return all(np.array_equal(got[f], want[f]) for f in ("ix", "iy", "alpha", "outside"))


def test_hand_built_maps(ext):
    import torch
    from orb_slam2_2021_amd import StereoRectifier, rectify_entries_host, remap_host
    src, m1, m2 = hand_maps()
    srows, scols = src.shape
    want_e = R.fixed_point(m1, m2, (scols, srows))
    assert sum(R.classify(want_e, (scols, srows))[:2]) > 0
    want = R.remap(src, want_e)
    with StereoRectifier.from_maps(ext, m1, m2, m1, m2, (scols, srows)) as rect:
        assert same_entries(rect.entries(False), want_e) and same_entries(rect.entries(True), want_e)
        assert same_entries(rectify_entries_host(m1, m2, (scols, srows)), want_e)
        d_src = torch.from_numpy(src).cuda().unsqueeze(0)
        d_dst = torch.full((2,) + m1.shape, SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()  # the fill ran on torch's stream, the call runs on the handle's
        rect.rectify_batch((d_src, d_src), d_dst)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    assert np.array_equal(remap_host(src, m1, m2), want)


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("cols", [1, 3, 63, 64, 65, 257])
def test_small_widths_unaligned_pitches_and_padding(ext, cols, channels):
    """3 side-by-side pairs of 9 x 11 pixels per half; the source starts at byte 1 of its buffer with rows an odd
    number of bytes apart; destination rows are their bytes + 3 apart and start at byte 2, so every alignment of
    the four-byte groups occurs. Rows 2..7 of a 7-row map."""
    import torch
    from orb_slam2_2021_amd import StereoRectifier, remap_host
    n, srows, scols, drows, row0, row1 = 3, 9, 11, 7, 2, 7
    rng = np.random.default_rng(1000 * cols + channels)
    img = rng.integers(0, 256, (n, srows, 2 * scols, channels), dtype=np.uint8)
    maps = random_maps(rng, drows, cols, srows, scols) + random_maps(rng, drows, cols, srows, scols)
    for side in range(2):
        counts = R.classify(R.fixed_point(maps[2 * side], maps[2 * side + 1], (scols, srows)), (scols, srows))
        assert cols < 63 or min(counts) > 0, counts
    spitch = 2 * scols * channels + (7 if (2 * scols * channels + 7) % 4 else 5)
    assert spitch % 4 != 0
    sstride = srows * spitch + 3
    src = np.full(1 + n * sstride, 0x3C, np.uint8)
    np.lib.stride_tricks.as_strided(src[1:], img.shape, (sstride, spitch, channels, 1))[...] = img
    d_src = torch.from_numpy(src).cuda()
    sview = torch.as_strided(d_src, img.shape, (sstride, spitch, channels, 1), 1)
    if channels == 1:
        sview = sview[..., 0]
    with StereoRectifier.from_maps(ext, *maps, (scols, srows)) as rect:
        for gray_out in ((True,) if channels == 1 else (True, False)):
            oc = 1 if gray_out else channels
            for mode, rgb in ((R.GRAY_SHIFT15, True), (R.GRAY_SHIFT14, False)):
                dpitch = cols * oc + 3
                dstride = (row1 - row0) * dpitch + 1
                shape = (2 * n, row1 - row0, cols) + ((oc,) if oc != 1 else ())
                strides = (dstride, dpitch, oc) + ((1,) if oc != 1 else ())
                d_dst = torch.full((2 + 2 * n * dstride,), SENTINEL, dtype=torch.uint8, device="cuda")
                torch.cuda.current_stream().synchronize()  # the fill ran on torch's stream, the call runs on the handle's
                rect.rectify_batch(sview, torch.as_strided(d_dst, shape, strides, 2), rows=(row0, row1),
                                   gray_out=gray_out, rgb=rgb, gray_mode=mode)
                torch.cuda.synchronize()
                got = d_dst.cpu().numpy()
                want = np.full(2 + 2 * n * dstride, SENTINEL, np.uint8)
                wv = np.lib.stride_tricks.as_strided(want[2:], shape, strides)
                for side in range(2):
                    for p in range(n):
                        half = img[p, :, side * scols:(side + 1) * scols]
                        half = half[..., 0] if channels == 1 else half
                        ref = R.rectify(half, maps[2 * side], maps[2 * side + 1], (row0, row1), gray_out, rgb, mode)
                        wv[side * n + p] = ref
                        if p == 0:
                            host = remap_host(half, maps[2 * side], maps[2 * side + 1], (row0, row1), gray_out, rgb,
                                              mode)
                            assert np.array_equal(host, ref), (side, gray_out, mode)
                assert np.array_equal(got, want), (gray_out, mode, rgb, np.nonzero(got != want)[0][:8])
    assert np.array_equal(d_src.cpu().numpy(), src)


@pytest.fixture(scope="module")
def vga_source(require_gpu):
    from orb_slam2_2021_amd import synth_frame
    left, right = synth_frame(4, 480, 640, right=True)
    g = np.concatenate([left, right], axis=1)
    return np.stack([g, 255 - g, (g.astype(np.uint16) * 5 // 7).astype(np.uint8)], -1)  # (480, 1280, 3)


def test_arducam_cameras_at_vga(ext, vga_source):
    import torch
    from orb_slam2_2021_amd import StereoRectifier, remap_host
    A = R.arducam()
    with StereoRectifier(ext, A["left"], A["right"], (640, 480)) as rect:
        d_src = torch.from_numpy(vga_source).cuda().unsqueeze(0)
        d_dst = torch.zeros((2, 400, 640), dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()  # the fill ran on torch's stream, the call runs on the handle's
        rect.rectify_batch(d_src, d_dst, rows=(0, 400), rgb=bool(A["rgb"]))
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        for side, name in enumerate(("left", "right")):
            c = A[name]
            m1, m2 = R.rectify_maps(c["K"], c["D"], c["R"], c["P"], (640, 480))
            assert np.array_equal(rect.maps[2 * side].view(np.uint32), m1.view(np.uint32))
            assert np.array_equal(rect.maps[2 * side + 1].view(np.uint32), m2.view(np.uint32))
            assert same_entries(rect.entries(bool(side)), R.fixed_point(m1, m2, (640, 480)))
            half = vga_source[:, side * 640:(side + 1) * 640]
            want = R.rectify(half, m1, m2, (0, 400), True, bool(A["rgb"]))
            assert np.array_equal(got[side], want), name
            assert np.array_equal(remap_host(half, m1, m2, (0, 400), True, bool(A["rgb"])), want), name


def test_a_calibration_that_leaves_the_source(ext, vga_source):
    """600 x 440 sources, a 640 x 480 destination; fully-outside, partly-outside and inside pixels all occur."""
    import torch
    from orb_slam2_2021_amd import StereoRectifier, remap_host
    S = R.synthetic_camera()
    cam = dict(K=S["K"], D=S["D"], R=S["R"], P=S["P"])
    cam4 = dict(K=S["K"], D=S["D"][:4], R=None, P=S["P"])
    src = np.ascontiguousarray(vga_source[20:460, 30:1230])  # (440, 1200, 3): two 600-pixel halves
    with StereoRectifier(ext, cam, cam4, S["size"], S["src_size"]) as rect:
        d_src = torch.from_numpy(src).cuda().unsqueeze(0)
        d_dst = torch.zeros((2, 480, 640, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.current_stream().synchronize()  # the fill ran on torch's stream, the call runs on the handle's
        rect.rectify_batch(d_src, d_dst, gray_out=False)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        for side, c in enumerate((cam, cam4)):
            m1, m2 = R.rectify_maps(c["K"], c["D"], c["R"], c["P"], S["size"])
            ent = R.fixed_point(m1, m2, S["src_size"])
            assert min(R.classify(ent, S["src_size"])) > 0
            assert same_entries(rect.entries(bool(side)), ent)
            half = src[:, side * 600:(side + 1) * 600]
            want = R.remap(half, ent)
            assert np.array_equal(got[side], want), side
            assert np.array_equal(remap_host(half, m1, m2), want), side


def test_bad_arguments_are_refused(ext):
    import torch
    from orb_slam2_2021_amd import OrbfeError, StereoRectifier
    src, m1, m2 = hand_maps()
    with pytest.raises(OrbfeError):
        StereoRectifier.from_maps(ext, m1, m2, m1, m2, (40000, 6))
    with StereoRectifier.from_maps(ext, m1, m2, m1, m2, (src.shape[1], src.shape[0])) as rect:
        d_src = torch.from_numpy(src).cuda().unsqueeze(0)
        d_dst = torch.zeros((2,) + m1.shape, dtype=torch.uint8, device="cuda")
        with pytest.raises(OrbfeError):
            rect.rectify_batch((d_src, d_src), d_dst, gray_mode=7)
        with pytest.raises(ValueError):
            rect.rectify_batch((d_src, d_src), d_dst[:, :, :3])
        with pytest.raises(OrbfeError):
            rect.rectify_batch((d_src, d_src), d_dst[:, :2], rows=(m1.shape[0] - 1, m1.shape[0] + 1))
