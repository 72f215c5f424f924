"""k_gray (orbfe_gray_batch_device) against tests/sensor_ref.py on every byte: every RGB triple once in both table
generations and both channel orders, and small widths around the kernel's four-pixel groups and 64-lane waves
with unaligned pitches, where nothing outside the rows' pixels may be written."""
import numpy as np
import pytest

import sensor_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ext(require_gpu):
    from orb_slam2_2021_amd import ORBextractor
    e = ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def all_triples(require_gpu):
    import torch
    idx = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    return img, torch.from_numpy(img).cuda().unsqueeze(0)


@pytest.mark.parametrize("rgb", [True, False])
@pytest.mark.parametrize("mode", [R.GRAY_SHIFT15, R.GRAY_SHIFT14])
def test_every_rgb_triple(ext, all_triples, mode, rgb):
    import torch
    img, d_img = all_triples
    d_out = torch.zeros((1, 4096, 4096), dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()  # the fill ran on torch's stream, the call runs on the handle's
    ext.to_gray_batch(d_img, d_out, rgb=rgb, gray_mode=mode)
    torch.cuda.synchronize()
    got = d_out[0].cpu().numpy()
    want = R.gray(img, rgb, mode)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("cols", [1, 3, 63, 64, 65, 257])
def test_small_widths_unaligned_pitches_and_padding(ext, cols, channels):
    """A batch of 3 images of 5 rows. The source rows are 7 (or 5) bytes longer than their pixels, so no row
    but the first starts on a dword; the source starts at byte 1 of its buffer; the destination rows are
    cols + 3 bytes apart and start at byte 2, so every alignment of the four-pixel groups occurs."""
    import torch
    n, rows = 3, 5
    rng = np.random.default_rng(100 * cols + channels)
    img = rng.integers(0, 256, (n, rows, cols, channels), dtype=np.uint8)
    spitch = cols * channels + (7 if (cols * channels + 7) % 4 else 5)
    assert spitch % 4 != 0 and spitch > cols * channels
    sstride = rows * spitch + 3
    src = np.full(1 + n * sstride, 0x3C, np.uint8)
    sv = np.lib.stride_tricks.as_strided(src[1:], (n, rows, cols, channels), (sstride, spitch, channels, 1))
    sv[...] = img
    dpitch = cols + 3
    dstride = rows * dpitch + 1
    d_src = torch.from_numpy(src).cuda()
    for mode in (R.GRAY_SHIFT15, R.GRAY_SHIFT14):
        for rgb in (True, False):
            d_dst = torch.full((2 + n * dstride,), SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.current_stream().synchronize()  # the fill ran on torch's stream, the call runs on the handle's
            ext.to_gray_batch(torch.as_strided(d_src, (n, rows, cols, channels), (sstride, spitch, channels, 1), 1),
                              torch.as_strided(d_dst, (n, rows, cols), (dstride, dpitch, 1), 2), rgb=rgb,
                              gray_mode=mode)
            torch.cuda.synchronize()
            got = d_dst.cpu().numpy()
            want = np.full(2 + n * dstride, SENTINEL, np.uint8)
            np.lib.stride_tricks.as_strided(want[2:], (n, rows, cols), (dstride, dpitch, 1))[...] = \
                R.gray(img, rgb, mode)
            assert np.array_equal(got, want), (mode, rgb, np.nonzero(got != want)[0][:8])
    assert np.array_equal(d_src.cpu().numpy(), src)


def test_bad_arguments_are_refused(ext):
    import torch
    from orb_slam2_2021_amd import OrbfeError
    src = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((1, 4, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(OrbfeError):
        ext.to_gray_batch(src, dst, gray_mode=7)
    with pytest.raises(ValueError):
        ext.to_gray_batch(src[..., :2], dst)
