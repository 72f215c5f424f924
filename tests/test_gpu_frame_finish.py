"""k_frame_finish (orbfe_frame_finish_batch_device) on hand-built keypoints, no extractor involved, bit for bit
against tests/sensor_ref.py and against the host entry points: the cameras and lattice of the CPU test, a batch
with counts 0, 1, 63, 64, 65 and cap = 128 whose outputs hold a sentinel beyond each count, uint16 and float32
depth maps with padded rows, keys on the maps' edge values, and the monocular null depth pointer."""
import numpy as np
import pytest

import sensor_ref as R
from sensor_cases import (CAMERAS, DEPTH_CASES, EDGE_KEYS, LATTICE, MAP_CAM, MAP_COLS, MAP_ROWS, padded)

pytestmark = pytest.mark.gpu

CAP = 128
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ext(require_gpu):
    from orb_slam2_2021_amd import ORBextractor
    e = ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    yield e
    e.close()


def finish(ext, cam, key_sets, maps=None, factor=1.0, extra=3, rows=MAP_ROWS, cols=MAP_COLS):
    """Runs the kernel on a batch (key_sets[i] = image i's keys; maps[i] its raw depth map, rows `extra` elements
    longer than the map). Returns per image (keys_un, u_right, depth) as full cap-long arrays, sentinel included."""
    import torch
    n = len(key_sets)
    kps = np.zeros(n * CAP, R.KEYPOINT_DTYPE)
    kps["x"] = -12345.0  # a key beyond a count would sample far outside a map
    counts = np.zeros(n, np.int32)
    for i, k in enumerate(key_sets):
        kps[i * CAP:i * CAP + len(k)] = k
        counts[i] = len(k)
    d_kps = torch.from_numpy(kps.view(np.uint8)).cuda()
    d_counts = torch.from_numpy(counts).cuda()
    d_un = torch.full((n * CAP * 28,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ur = torch.full((n * CAP * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_dep = torch.full((n * CAP * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_maps = None
    if maps is not None:
        buf = np.stack([padded(m, extra)[0] for m in maps])
        raw = torch.from_numpy(buf.view(np.int16) if buf.dtype == np.uint16 else buf).cuda()
        d_maps = raw[:, :, :maps[0].shape[1]]
        assert d_maps.stride(1) == maps[0].shape[1] + extra
    ext.frame_finish_batch(n, R_to_lib(cam), d_kps.data_ptr(), d_counts.data_ptr(), CAP, rows, cols, d_un.data_ptr(),
                           d_ur.data_ptr(), d_dep.data_ptr(), depth_maps=d_maps, depth_factor=float(factor))
    torch.cuda.synchronize()
    un = d_un.cpu().numpy().view(R.KEYPOINT_DTYPE).reshape(n, CAP)
    ur = d_ur.cpu().numpy().view(np.float32).reshape(n, CAP)
    dep = d_dep.cpu().numpy().view(np.float32).reshape(n, CAP)
    return un, ur, dep


def R_to_lib(cam):
    return dict(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], dist=cam["dist"], bf=cam["bf"])


def check(cam, key_sets, got, maps=None, factor=1.0, extra=3):
    from orb_slam2_2021_amd.extractor import stereo_from_depth_host, undistort_keypoints_host
    un, ur, dep = got
    sent_f = np.frombuffer(bytes([SENTINEL] * 4), np.uint32)[0]
    for i, keys in enumerate(key_sets):
        k = len(keys)
        m = None if maps is None else maps[i]
        want_un = R.undistort_keys(cam, keys)
        want_ur, want_dep = R.stereo_from_depth(cam, keys, want_un, m, factor)
        assert un[i, :k].tobytes() == want_un.tobytes(), (i, "keys_un")  # all seven fields
        assert np.array_equal(R.bits(ur[i, :k]), R.bits(want_ur)), (i, "u_right")
        assert np.array_equal(R.bits(dep[i, :k]), R.bits(want_dep)), (i, "depth")
        # nothing at or beyond the count is touched
        assert (un[i, k:].view(np.uint8) == SENTINEL).all(), i
        assert (R.bits(ur[i, k:]) == sent_f).all() and (R.bits(dep[i, k:]) == sent_f).all(), i
        # the host entry points give the same bits
        host_un = undistort_keypoints_host(R_to_lib(cam), keys)
        assert host_un.tobytes() == un[i, :k].tobytes(), (i, "host keys_un")
        if m is None:
            h_ur, h_dep = stereo_from_depth_host(R_to_lib(cam), keys, host_un, None)
        else:
            buf, _ = padded(m, extra)
            h_ur, h_dep = stereo_from_depth_host(R_to_lib(cam), keys, host_un, buf[:, :m.shape[1]], factor)
        assert np.array_equal(R.bits(h_ur), R.bits(ur[i, :k])) and np.array_equal(R.bits(h_dep), R.bits(dep[i, :k])), i


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_cameras_on_the_lattice_monocular(ext, name):
    cam = CAMERAS[name]
    got = finish(ext, cam, [LATTICE], rows=480, cols=640)
    check(cam, [LATTICE], got)
    assert (got[1][0, :len(LATTICE)] == -1).all() and (got[2][0, :len(LATTICE)] == -1).all()
    if name == "k1_neg":
        trace = []
        R.undistort_keys(cam, LATTICE, trace)
        assert 0 < sum(trace) < len(trace)


def batch_keys(seed):
    """Counts 0, 1, 63, 64, 65 and cap in one batch, keys anywhere on the 40 x 30 map, every field set."""
    rng = np.random.default_rng(seed)
    sets = []
    for c in (0, 1, 63, 64, 65, CAP):
        k = np.zeros(c, R.KEYPOINT_DTYPE)
        k["x"] = rng.uniform(0, MAP_COLS, c).astype(np.float32).clip(0, np.float32(MAP_COLS - 0.01))
        k["y"] = rng.uniform(0, MAP_ROWS, c).astype(np.float32).clip(0, np.float32(MAP_ROWS - 0.01))
        k["size"], k["angle"], k["response"] = rng.uniform(1, 400, (3, c)).astype(np.float32)
        k["octave"], k["class_id"] = rng.integers(-1, 8, (2, c))
        sets.append(k)
    return sets


@pytest.mark.parametrize("case", DEPTH_CASES, ids=[c[0] for c in DEPTH_CASES])
def test_batch_counts_and_depth_maps(ext, case):
    _, m, factor = case
    sets = batch_keys(5)
    maps = [np.roll(m, 3 * i, axis=1) for i in range(len(sets))]  # a different map per image
    got = finish(ext, MAP_CAM, sets, maps, factor)
    check(MAP_CAM, sets, got, maps, factor)
    dep = np.concatenate([got[2][i, :len(k)] for i, k in enumerate(sets)])
    assert (dep == -1).any() and (dep > 0).any()


@pytest.mark.parametrize("case", DEPTH_CASES, ids=[c[0] for c in DEPTH_CASES])
def test_edge_keys_sample_the_edge_values(ext, case):
    name, m, factor = case
    got = finish(ext, MAP_CAM, [EDGE_KEYS], [m], factor)
    check(MAP_CAM, [EDGE_KEYS], got, [m], factor)
    dep = got[2][0]
    # key 0 at (cols - 0.4, rows - 0.4) reads the last value, key 1 at (0.9, 0.9) reads [0][0], key 2 at
    # (10.8, 5.9) reads [5][10]; keys 3.. read [0][1], [0][2], [1][3], [1][4]
    assert R.bits(dep[0:1])[0] == R.bits(R.depth_value(m[MAP_ROWS - 1, MAP_COLS - 1], factor))[0]
    assert dep[1] == -1  # the zero at [0][0]
    assert R.bits(dep[2:3])[0] == R.bits(R.depth_value(m[5, 10], factor))[0]
    if name == "u16_5000":
        assert dep[3] == np.float32(1.0) * factor and dep[4] == np.float32(65535.0) * factor
    else:
        assert dep[3] == -1 and dep[4] == -1 and dep[6] == -1   # -1, NaN, -0
        assert np.isposinf(dep[5]) and got[1][0][5] == got[0][0]["x"][5]  # +inf: uRight = x - bf / inf


def test_null_depth_is_monocular(ext):
    sets = batch_keys(6)
    got = finish(ext, MAP_CAM, sets)
    check(MAP_CAM, sets, got)
    for i, k in enumerate(sets):
        assert (got[1][i, :len(k)] == -1).all() and (got[2][i, :len(k)] == -1).all()


def test_bad_arguments_are_refused(ext):
    from orb_slam2_2021_amd import OrbfeError
    with pytest.raises(OrbfeError):
        ext.frame_finish_batch(1, R_to_lib(MAP_CAM), 0, 16, CAP, 30, 40, 16, 16, 16)
    with pytest.raises(ValueError):
        ext.frame_finish_batch(1, dict(R_to_lib(MAP_CAM), dist=[0.1, 0.2]), 16, 16, CAP, 30, 40, 16, 16, 16)
