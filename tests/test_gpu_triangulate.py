"""k_triangulate on the GPU against tests/triangulate_ref.py: status, the bits of x3d where
status > 0, and nnew compare with ==. No tolerance and no excuse rule: test_triangulate_ref.py shows
that no decision of these scenes can hang on the last bits of cosf / atan2f."""
import numpy as np
import pytest

import triangulate_ref as R
import triangulate_scenes as S

pytestmark = pytest.mark.gpu
KEEP = np.float32(-123.25)   # x3d entries without a point must come back as they went in


@pytest.fixture(scope="module")
def matcher(require_gpu):
    from orb_slam2_2021_amd import ORBmatcher
    m = ORBmatcher(0.6, False)
    yield m
    m.close()


def same(got, want, tag=""):
    st, x, nnew = got
    rst, rx, rn = want
    assert np.array_equal(st, rst), (tag, np.nonzero(st != rst)[0][:8], st[st != rst][:8], rst[st != rst][:8])
    assert nnew == rn == int((rst > 0).sum()), tag
    acc = rst > 0
    assert np.array_equal(x[acc].view(np.uint32), rx[acc].view(np.uint32)), tag
    assert np.all(x[~acc] == KEEP), tag


def host_run(matcher, kf1, kf2, m12):
    keep = np.full((kf1.kf.N, 3), KEEP, np.float32)
    return matcher.TriangulateMatches(kf1, kf2, m12, keep), R.triangulate_ref(kf1, kf2, m12, keep)


# ---- shapes: the smallest at which the compaction can go wrong ------------------------------------
def pattern(sc, which):
    """match12 thinned out of a scene in which every KF1 keypoint has its true match."""
    m = np.full(sc.n1, -1, np.int32)
    if which == "all":
        m[:] = sc.match12
    elif which == "last":        # exactly one match, in the last lane of the last block
        m[-1] = sc.match12[-1]
    elif which == "wave4":       # every match of the first block in its fourth wavefront
        m[192:256] = sc.match12[192:256]
    return m


@pytest.mark.parametrize("n1", S.SHAPE_N1)
@pytest.mark.parametrize("which", ["none", "last", "all"])
def test_shapes(matcher, n1, which):
    sc = S.shape_scene(n1)
    m = pattern(sc, which)
    got, want = host_run(matcher, sc.kf1, sc.kf2, m)
    same(got, want, (n1, which))
    if which == "none":
        assert got[2] == 0 and not got[0].any()
    if which == "last":
        assert np.count_nonzero(got[0]) == 1 and got[0][-1] != 0
    if which == "all":
        assert np.all(got[0] != 0) and got[2] >= 0.3 * n1


def test_matches_only_in_the_fourth_wavefront(matcher):
    sc = S.wave4_scene()
    m = pattern(sc, "wave4")
    got, want = host_run(matcher, sc.kf1, sc.kf2, m)
    same(got, want)
    assert np.count_nonzero(got[0]) == 64 and not got[0][:192].any() and not got[0][256:].any()


@pytest.mark.parametrize("idx", range(len(S.SCENES)), ids=[s[0] for s in S.SCENES])
def test_scene_kinds(matcher, idx):
    sc = S.scenes()[idx]
    got, want = host_run(matcher, sc.kf1, sc.kf2, sc.match12)
    same(got, want, sc.kind)
    assert got[2] > 20


CASES = S.status_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_status_cases(matcher, case):
    name, kf1, kf2, want = case
    got, ref = host_run(matcher, kf1, kf2, np.zeros(1, np.int32))
    same(got, ref, name)
    assert got[0][0] != want[1] if isinstance(want, tuple) else got[0][0] == want


def test_out_of_range_match_and_octave(matcher):
    sc = S.range_scene()
    m = sc.match12.copy()
    m[3], m[70], m[129], m[5] = sc.n2, 2 ** 30, sc.n2 + 1, -7
    sc.kf1.kf.keys_un["octave"][10] = 8
    sc.kf1.kf.keys_un["octave"][11] = -1
    sc.kf2.kf.keys_un["octave"][m[12]] = 8
    got, want = host_run(matcher, sc.kf1, sc.kf2, m)
    same(got, want)
    st = got[0]
    assert list(st[[3, 70, 129]]) == [R.REJ_BAD_MATCH] * 3 and st[5] == R.NO_MATCH
    assert list(st[[10, 11, 12]]) == [R.REJ_BAD_OCTAVE] * 3


# ---- device entry points ----------------------------------------------------------------------------
def device_batch(matcher, items, pad=5):
    """items: (kf1, kf2, match12). Every pair's kf1.n is `pad` above its real count, which the
    kernel reads from device memory (kf1_n_dev). -> per pair ((status, x3d, nnew), status tail)."""
    import torch
    from orb_slam2_2021_amd import _lib as L
    dev = torch.device("cuda", 0)
    hold, pairs = [], []
    for kf1, kf2, m12 in items:
        d1, d2 = kf1.to_device(dev), kf2.to_device(dev)
        n1 = kf1.kf.N
        t = dict(m12=torch.from_numpy(np.concatenate([m12, np.zeros(pad, np.int32)])).to(dev),
                 n=torch.tensor([n1], dtype=torch.int32, device=dev),
                 status=torch.full((n1 + pad,), 77, dtype=torch.int8, device=dev),
                 x3d=torch.full((n1 + pad, 3), float(KEEP), dtype=torch.float32, device=dev),
                 nnew=torch.full((1,), -5, dtype=torch.int32, device=dev))
        p = L.tri_pair()
        p.kf1, p.kf2, p.t1, p.t2 = d1.view(), d2.view(), d1.tri_view(), d2.tri_view()
        p.kf1.n = n1 + pad
        p.match12, p.kf1_n_dev, p.status = L.ptr(t["m12"]), L.ptr(t["n"]), L.ptr(t["status"])
        p.x3d, p.nnew = L.ptr(t["x3d"]), L.ptr(t["nnew"])
        hold.append((d1, d2, t))
        pairs.append(p)
    torch.cuda.synchronize()
    matcher.TriangulateBatchDevice(pairs)
    matcher.synchronize()
    out = []
    for (kf1, _, _), (_, _, t) in zip(items, hold):
        n1 = kf1.kf.N
        st = t["status"].cpu().numpy()
        out.append(((st[:n1], t["x3d"].cpu().numpy()[:n1], int(t["nnew"].item())), st[n1:]))
    return out


@pytest.mark.parametrize("n_pairs", S.BATCH_PAIRS)
def test_batches_with_unequal_sizes_and_device_counts(matcher, n_pairs):
    items = [(sc.kf1, sc.kf2, sc.match12) for sc in S.batch_scenes(n_pairs)]
    for (kf1, kf2, m12), (got, tail) in zip(items, device_batch(matcher, items)):
        keep = np.full((kf1.kf.N, 3), KEEP, np.float32)
        same(got, R.triangulate_ref(kf1, kf2, m12, keep), kf1.kf.N)
        assert np.all(tail == 77)    # nothing past the device-side count is touched


def test_search_then_triangulate_on_one_stream_with_marking(matcher):
    """orbfe_search_for_triangulation_batch_device -> orbfe_triangulate_batch_device on the matcher's
    stream, no host copy in between, equals the host-buffer path run on the copied-back match12;
    mark1 / mark2 afterwards are the input mp_state with OBSERVED at exactly the accepted indices."""
    import ctypes
    import torch
    from orb_slam2_2021_amd import _lib as L
    sc = S.ChainScene(1)
    kf1, kf2 = sc.kf1, sc.nbs[0]
    dev = torch.device("cuda", 0)
    d1, d2 = kf1.to_device(dev), kf2.to_device(dev)
    n1 = kf1.kf.N
    m12 = torch.full((n1,), -9, dtype=torch.int32, device=dev)
    nm = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(n1, dtype=torch.int8, device=dev)
    x3d = torch.full((n1, 3), float(KEEP), dtype=torch.float32, device=dev)
    nnew = torch.zeros(1, dtype=torch.int32, device=dev)
    sp = (L.sft_pair * 1)()
    sp[0].kf1, sp[0].kf2, sp[0].fv1, sp[0].fv2 = d1.view(), d2.view(), d1.fv_view(), d2.fv_view()
    for k, v in enumerate(sc.f12[0].reshape(9)):
        sp[0].f12[k] = float(v)
    sp[0].ex, sp[0].ey = sc.epipole[0]
    sp[0].match12, sp[0].nmatches = L.ptr(m12), L.ptr(nm)
    tp = L.tri_pair()
    tp.kf1, tp.kf2, tp.t1, tp.t2 = d1.view(), d2.view(), d1.tri_view(), d2.tri_view()
    tp.match12, tp.status, tp.x3d, tp.nnew = L.ptr(m12), L.ptr(status), L.ptr(x3d), L.ptr(nnew)
    tp.mark1, tp.mark2 = L.ptr(d1.mp_state), L.ptr(d2.mp_state)
    torch.cuda.synchronize()
    L.check(L.lib().orbfe_search_for_triangulation_batch_device(matcher._h, 1, ctypes.addressof(sp), 0, None), "sft")
    matcher.TriangulateBatchDevice([tp])
    matcher.synchronize()
    m12h = m12.cpu().numpy()
    assert int(nm.item()) == int((m12h >= 0).sum()) > 30
    got = (status.cpu().numpy(), x3d.cpu().numpy(), int(nnew.item()))
    keep = np.full((n1, 3), KEEP, np.float32)
    host = matcher.TriangulateMatches(kf1, kf2, m12h, keep)
    same(got, host)
    same(got, R.triangulate_ref(kf1, kf2, m12h, keep))
    acc = got[0] > 0
    assert acc.sum() > 20
    want1, want2 = kf1.kf.mp_state.copy(), kf2.kf.mp_state.copy()
    want1[acc] = L.ORBFE_MP_OBSERVED
    want2[m12h[acc]] = L.ORBFE_MP_OBSERVED
    assert np.array_equal(d1.mp_state_host(), want1) and np.array_equal(d2.mp_state_host(), want2)


@pytest.mark.parametrize("n_nb", [1, 2, 5])
def test_create_new_mappoints_equals_the_python_loop(matcher, n_nb):
    import torch
    sc = S.ChainScene(n_nb)
    want, s1, s2s = S.chain_reference(sc)
    dev = torch.device("cuda", 0)
    d1 = sc.kf1.to_device(dev)
    dn = [nb.to_device(dev) for nb in sc.nbs]
    m12, status, x3d, nm, nnew = matcher.CreateNewMapPointsDevice(d1, dn, sc.f12, sc.epipole)
    matcher.synchronize()
    m12, status, x3d, nm, nnew = (t.cpu().numpy() for t in (m12, status, x3d, nm, nnew))
    for j, (rm, rst, rx, rnm, rnn) in enumerate(want):
        assert np.array_equal(m12[j], rm), j
        assert nm[j] == rnm and nnew[j] == rnn, j
        assert np.array_equal(status[j], rst), j
        acc = rst > 0
        assert np.array_equal(x3d[j][acc].view(np.uint32), rx[acc].view(np.uint32)), j
        assert np.array_equal(dn[j].mp_state_host(), s2s[j]), j
    assert np.array_equal(d1.mp_state_host(), s1)
    if n_nb > 1:
        assert nnew[1] > 0 and not np.any(m12[1][status[0] > 0] >= 0)


def test_create_new_mappoints_rejects_a_repeated_neighbour(matcher):
    import torch
    from orb_slam2_2021_amd import OrbfeError
    sc = S.ChainScene(2, n=30)
    dev = torch.device("cuda", 0)
    d1 = sc.kf1.to_device(dev)
    dn = [nb.to_device(dev) for nb in sc.nbs]
    with pytest.raises(OrbfeError, match="appears twice"):
        matcher.CreateNewMapPointsDevice(d1, [dn[0], dn[1], dn[0]], sc.f12 + [sc.f12[0]], sc.epipole + [sc.epipole[0]])
    with pytest.raises(OrbfeError, match="equals KF1"):
        matcher.CreateNewMapPointsDevice(d1, [dn[0], d1], sc.f12, sc.epipole)
    assert np.array_equal(d1.mp_state_host(), sc.kf1.kf.mp_state)   # nothing was launched
