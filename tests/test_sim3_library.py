"""orbfe_sim3_* without a GPU: the symbols are exported, a host-only handle (device < 0) checks
every argument before it would touch a device, and a solve on it fails loudly (ORBFE_ERR_STATE)."""
import os
import re
import subprocess
from ctypes import byref, c_void_p

import numpy as np
import pytest

from sim3_scenes import Scene, draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sim3_symbols_declared_and_exported():
    from orb_slam2_2021_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "orbfe_sim3.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(orbfe_sim3_\w+)\s*\(", src))
    assert declared == {"orbfe_sim3_create", "orbfe_sim3_destroy", "orbfe_sim3_solve_batch", "orbfe_sim3_iterate"}
    L.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (orbfe_\w+)", out))
    assert declared <= exported and declared <= set(L.EXPORTED)
    blob = open(L.LIB_PATH, "rb").read()
    for k in (b"k_sim3_hypotheses", b"k_sim3_inliers", b"k_sim3_select"):
        assert k in blob


def test_create_bounds():
    from orb_slam2_2021_amd import _lib as L
    lib = L.lib()
    h = c_void_p()
    for args in ((0, 100, 300), (65, 100, 300), (4, 2, 300), (4, 4097, 300), (4, 100, 0), (4, 100, 1025)):
        assert lib.orbfe_sim3_create(-1, *args, byref(h)) == L.ORBFE_ERR_ARG, args
        assert not h.value
    assert b"1..64" in lib.orbfe_last_error()
    assert lib.orbfe_sim3_create(-1, 4, 100, 300, None) == L.ORBFE_ERR_ARG
    assert lib.orbfe_sim3_create(-1, 64, 4096, 1024, byref(h)) == L.ORBFE_OK and h.value
    assert lib.orbfe_sim3_destroy(h) == L.ORBFE_OK
    assert lib.orbfe_sim3_destroy(None) == L.ORBFE_OK


class HostOnly:
    def __init__(self, max_solvers=2, max_corr=64, max_hyp=16):
        from orb_slam2_2021_amd import Sim3Batch
        self.batch = Sim3Batch(max_solvers, max_corr, max_hyp, device=-1)

    def status(self, solvers):
        from orb_slam2_2021_amd import OrbfeError
        try:
            self.batch.solve(solvers)
        except OrbfeError as e:
            return e.status, str(e)
        return 0, ""


def make_solver(n=20, n_hyp=8, seed=1, min_inliers=6, max_iterations=300):
    from orb_slam2_2021_amd import Sim3Solver
    sc = Scene(n, seed)
    s = Sim3Solver(sc.x1, sc.x2, sc.sigma2_1, sc.sigma2_2, sc.k1, sc.k2, False)
    s.SetRansacParameters(0.99, min_inliers, max_iterations)
    if n >= 3:
        s.set_draws(draws(n, n_hyp, seed + 1))
    return s


def test_host_only_solve_is_a_state_error_after_the_checks():
    from orb_slam2_2021_amd import _lib as L
    ho = HostOnly()
    st, msg = ho.status([make_solver()])
    assert st == L.ORBFE_ERR_STATE and "host-only" in msg
    # n < min_inliers is a valid request (bNoMore): still the state error, not an argument error
    assert ho.status([make_solver(n=4, min_inliers=6)])[0] == L.ORBFE_ERR_STATE


def test_capacity_checks():
    from orb_slam2_2021_amd import _lib as L
    ho = HostOnly(max_solvers=2, max_corr=64, max_hyp=16)
    assert ho.status([make_solver(), make_solver(), make_solver()])[0] == L.ORBFE_ERR_CAPACITY
    assert ho.status([make_solver(n=65)])[0] == L.ORBFE_ERR_CAPACITY
    # 17 evaluated hypotheses against max_hyp = 16
    st, msg = ho.status([make_solver(n_hyp=17)])
    assert st == L.ORBFE_ERR_CAPACITY and "max_hyp" in msg
    # 40 drawn but mRansacMaxIts = 16 caps the evaluated count: accepted (then the state error)
    assert ho.status([make_solver(n_hyp=40, max_iterations=16)])[0] == L.ORBFE_ERR_STATE
    # n == min_inliers evaluates one hypothesis however many were drawn
    assert ho.status([make_solver(n=20, n_hyp=40, min_inliers=20)])[0] == L.ORBFE_ERR_STATE


@pytest.mark.parametrize("pos,value", [(0, 20), (0, -1), (1, 19), (2, 18), (5, 18)])
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
    d.reshape(-1)[pos] = 19 - pos % 3
    s.set_draws(d)
    assert ho.status([s])[0] == L.ORBFE_ERR_STATE


def test_null_arrays_and_bad_parameters():
    from orb_slam2_2021_amd import _lib as L
    lib = L.lib()
    h = c_void_p()
    assert lib.orbfe_sim3_create(-1, 2, 64, 16, byref(h)) == L.ORBFE_OK
    sc = Scene(20, 1)
    d = draws(20, 8, 2)
    res_arrays = dict(hyp_capacity=16, mask_words=1)

    def solver(**over):
        f = dict(n=20, x3dc1=L.ptr(sc.x1), x3dc2=L.ptr(sc.x2), sigma2_1=L.ptr(sc.sigma2_1),
                 sigma2_2=L.ptr(sc.sigma2_2), fix_scale=0, min_inliers=6, max_iterations=300, probability=0.99,
                 n_hyp=8, rand_idx=L.ptr(d))
        f.update(over)
        return L.sim3_solver(**f)

    def run(s, r=None):
        S = (L.sim3_solver * 1)(s)
        R = (L.sim3_result * 1)(r if r is not None else L.sim3_result(**res_arrays))
        return lib.orbfe_sim3_solve_batch(h, S, 1, R)

    assert run(solver()) == L.ORBFE_ERR_STATE
    for name in ("x3dc1", "x3dc2", "sigma2_1", "sigma2_2", "rand_idx"):
        assert run(solver(**{name: None})) == L.ORBFE_ERR_ARG, name
    t = np.zeros((8, 12), np.float32)
    assert run(solver(hyp_t12=L.ptr(t))) == L.ORBFE_ERR_ARG           # one without the other
    assert run(solver(hyp_t12=L.ptr(t), hyp_t21=L.ptr(t), rand_idx=None)) == L.ORBFE_ERR_STATE
    assert run(solver(n=-1)) == L.ORBFE_ERR_ARG
    assert run(solver(n_hyp=-1)) == L.ORBFE_ERR_ARG
    assert run(solver(probability=1.5)) == L.ORBFE_ERR_ARG
    assert run(solver(n=2, min_inliers=2)) == L.ORBFE_ERR_ARG          # a hypothesis needs three points
    bad_sigma = sc.sigma2_1.copy()
    bad_sigma[3] = np.nan
    assert run(solver(sigma2_1=L.ptr(bad_sigma))) == L.ORBFE_ERR_ARG
    assert run(solver(), L.sim3_result(hyp_capacity=7, mask_words=1)) == L.ORBFE_ERR_CAPACITY
    mask = np.zeros((16, 1), np.uint64)
    assert run(solver(), L.sim3_result(hyp_capacity=16, mask_words=0, inlier_mask=L.ptr(mask))) == L.ORBFE_ERR_CAPACITY
    assert lib.orbfe_sim3_solve_batch(None, None, 1, None) == L.ORBFE_ERR_ARG
    assert lib.orbfe_sim3_solve_batch(h, None, 1, None) == L.ORBFE_ERR_ARG
    # iterate: nothing solved on this handle
    st, out = L.sim3_state(0, 0, -1), L.sim3_iterate()
    assert lib.orbfe_sim3_iterate(h, 0, 5, byref(st), byref(out)) == L.ORBFE_ERR_STATE
    assert lib.orbfe_sim3_iterate(h, 0, 5, None, byref(out)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_sim3_iterate(None, 0, 5, byref(st), byref(out)) == L.ORBFE_ERR_ARG
    assert lib.orbfe_sim3_destroy(h) == L.ORBFE_OK
