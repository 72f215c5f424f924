"""orbfe_pnp_* without a GPU: the symbols are exported, a host-only handle (device < 0) checks every
argument before it would touch a device, and a solve on it fails loudly (ORBFE_ERR_STATE)."""
import os
import re
import subprocess
from ctypes import byref, c_void_p

import numpy as np
import pytest

from pnp_scenes import Scene, draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = (0.99, 10, 300, 4, 0.3, 5.991)


def test_pnp_symbols_declared_and_exported():
    from orb_slam2_2021_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "orbfe_pnp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(orbfe_pnp_\w+)\s*\(", src))
    assert declared == {"orbfe_pnp_create", "orbfe_pnp_destroy", "orbfe_pnp_solve_batch", "orbfe_pnp_iterate"}
    L.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (orbfe_\w+)", out))
    assert declared <= exported and declared <= set(L.EXPORTED)
    blob = open(L.LIB_PATH, "rb").read()
    for k in (b"k_pnp_hypotheses", b"k_pnp_inliers", b"k_pnp_records", b"k_pnp_refine", b"k_pnp_select"):
        assert k in blob


def test_create_bounds():
    from orb_slam2_2021_amd import _lib as L
    lib = L.lib()
    h = c_void_p()
    for args in ((0, 100, 300), (65, 100, 300), (4, 3, 300), (4, 4097, 300), (4, 100, 0), (4, 100, 1025)):
        assert lib.orbfe_pnp_create(-1, *args, byref(h)) == L.ORBFE_ERR_ARG, args
        assert not h.value
    assert b"1..64" in lib.orbfe_last_error()
    assert lib.orbfe_pnp_create(-1, 4, 100, 300, None) == L.ORBFE_ERR_ARG
    assert lib.orbfe_pnp_create(-1, 64, 4096, 1024, byref(h)) == L.ORBFE_OK and h.value
    assert lib.orbfe_pnp_destroy(h) == L.ORBFE_OK
    assert lib.orbfe_pnp_destroy(None) == L.ORBFE_OK


class HostOnly:
    def __init__(self, max_solvers=2, max_corr=64, max_hyp=16):
        from orb_slam2_2021_amd import PnPBatch
        self.batch = PnPBatch(max_solvers, max_corr, max_hyp, device=-1)

    def status(self, solvers):
        from orb_slam2_2021_amd import OrbfeError
        try:
            self.batch.solve(solvers)
        except OrbfeError as e:
            return e.status, str(e)
        return 0, ""


def make_solver(n=20, n_hyp=8, seed=1, params=PARAMS):
    from orb_slam2_2021_amd import PnPsolver
    sc = Scene(n, seed)
    s = PnPsolver(sc.p3dw, sc.p2d, sc.sigma2, sc.k)
    s.SetRansacParameters(*params)
    if n >= 4:
        s.set_draws(draws(n, n_hyp, seed + 1))
    return s


def test_host_only_solve_is_a_state_error_after_the_checks():
    from orb_slam2_2021_amd import _lib as L
    ho = HostOnly()
    st, msg = ho.status([make_solver()])
    assert st == L.ORBFE_ERR_STATE and "host-only" in msg
    # n < mRansacMinInliers is a valid request (bNoMore): still the state error, not an argument error
    assert ho.status([make_solver(n=5)])[0] == L.ORBFE_ERR_STATE
    assert ho.status([make_solver(n=0)])[0] == L.ORBFE_ERR_STATE


def test_capacity_checks():
    from orb_slam2_2021_amd import _lib as L
    ho = HostOnly(max_solvers=2, max_corr=64, max_hyp=16)
    assert ho.status([make_solver(), make_solver(), make_solver()])[0] == L.ORBFE_ERR_CAPACITY
    assert ho.status([make_solver(n=65)])[0] == L.ORBFE_ERR_CAPACITY
    st, msg = ho.status([make_solver(n_hyp=17)])
    assert st == L.ORBFE_ERR_CAPACITY and "max_hyp" in msg
    assert ho.status([make_solver(n=64, n_hyp=16)])[0] == L.ORBFE_ERR_STATE


def test_min_set_must_be_four():
    from orb_slam2_2021_amd import _lib as L
    ho = HostOnly()
    for min_set in (3, 5, 0):
        st, msg = ho.status([make_solver(params=(0.99, 10, 300, min_set, 0.3, 5.991))])
        assert st == L.ORBFE_ERR_ARG and "min_set" in msg


@pytest.mark.parametrize("pos,value", [(0, 20), (0, -1), (1, 19), (2, 18), (3, 17), (7, 17)])
def test_rand_idx_out_of_range_for_its_position(pos, value):
    from orb_slam2_2021_amd import _lib as L
    ho = HostOnly()
    s = make_solver(n=20, n_hyp=8)
    d = draws(20, 8, 3)
    d.reshape(-1)[pos] = value
    s.set_draws(d)
    st, msg = ho.status([s])
    assert st == L.ORBFE_ERR_ARG and "rand_idx" in msg
    # the largest admissible value of that position passes the check
    d.reshape(-1)[pos] = 19 - pos % 4
    s.set_draws(d)
    assert ho.status([s])[0] == L.ORBFE_ERR_STATE


def test_null_arrays_and_bad_parameters():
    from orb_slam2_2021_amd import _lib as L
    lib = L.lib()
    h = c_void_p()
    assert lib.orbfe_pnp_create(-1, 2, 64, 16, byref(h)) == L.ORBFE_OK
    sc = Scene(20, 1)
    d = draws(20, 8, 2)
    cnt = np.zeros(16, np.int32)
    mask = np.zeros((16, 1), np.uint64)

    def solver(**over):
        f = dict(n=20, p3dw=L.ptr(sc.p3dw), p2d=L.ptr(sc.p2d), sigma2=L.ptr(sc.sigma2), probability=0.99,
                 min_inliers=10, max_iterations=300, min_set=4, epsilon=0.3, th2=5.991, n_hyp=8, rand_idx=L.ptr(d))
        f.update(over)
        s = L.pnp_solver(**f)
        s.k[:] = [float(v) for v in sc.k]
        return s

    def run(s, r=None):
        S = (L.pnp_solver * 1)(s)
        R = (L.pnp_result * 1)(r if r is not None else L.pnp_result(hyp_capacity=16, rec_capacity=16, mask_words=1))
        return lib.orbfe_pnp_solve_batch(h, S, 1, R)

    assert run(solver()) == L.ORBFE_ERR_STATE
    for name in ("p3dw", "p2d", "sigma2", "rand_idx"):
        assert run(solver(**{name: None})) == L.ORBFE_ERR_ARG, name
    assert run(solver(n=-1)) == L.ORBFE_ERR_ARG
    assert run(solver(n_hyp=-1)) == L.ORBFE_ERR_ARG
    assert run(solver(probability=1.5)) == L.ORBFE_ERR_ARG
    assert run(solver(epsilon=float("nan"))) == L.ORBFE_ERR_ARG
    assert run(solver(th2=float("inf"))) == L.ORBFE_ERR_ARG
    bad_sigma = sc.sigma2.copy()
    bad_sigma[3] = np.nan
    assert run(solver(sigma2=L.ptr(bad_sigma))) == L.ORBFE_ERR_ARG
    assert run(solver(), L.pnp_result(hyp_capacity=7, rec_capacity=16, mask_words=1, n_inliers=L.ptr(cnt))) \
        == L.ORBFE_ERR_CAPACITY
    assert run(solver(), L.pnp_result(hyp_capacity=16, rec_capacity=7, mask_words=1, records=L.ptr(cnt))) \
        == L.ORBFE_ERR_CAPACITY
    assert run(solver(), L.pnp_result(hyp_capacity=16, rec_capacity=16, mask_words=0, inlier_mask=L.ptr(mask))) \
        == L.ORBFE_ERR_CAPACITY
    assert lib.orbfe_pnp_solve_batch(None, None, 1, None) == L.ORBFE_ERR_ARG
    assert lib.orbfe_pnp_solve_batch(h, None, 1, None) == L.ORBFE_ERR_ARG
    # iterate: nothing solved on this handle
    st, out = L.pnp_state(0, 0, -1), L.pnp_iterate()
    assert lib.orbfe_pnp_iterate(h, 0, 5, byref(st), byref(out)) == L.ORBFE_ERR_STATE
    assert lib.orbfe_pnp_iterate(h, 0, 5, None, byref(out)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_pnp_iterate(None, 0, 5, byref(st), byref(out)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_pnp_destroy(h) == L.ORBFE_OK
