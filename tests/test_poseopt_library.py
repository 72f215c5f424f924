"""orbfe_poseopt_* without a GPU: the symbols are exported, k_poseopt is in the code object, a
host-only handle (device < 0) checks every argument before it would touch a device, and a solve on it
fails loudly (ORBFE_ERR_STATE)."""
import os
import re
import subprocess
from ctypes import byref, c_void_p

import numpy as np

from poseopt_scenes import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_poseopt_symbols_declared_and_exported():
    from orb_slam2_2021_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "orbfe_poseopt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(orbfe_poseopt_\w+)\s*\(", src))
    assert declared == {"orbfe_poseopt_create", "orbfe_poseopt_destroy", "orbfe_poseopt_batch"}
    L.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (orbfe_poseopt_\w+)", out))
    assert declared == exported and declared <= set(L.EXPORTED)
    assert {s for s in L.EXPORTED if s.startswith("orbfe_poseopt_")} == declared
    assert b"k_poseopt" in open(L.LIB_PATH, "rb").read()


def test_flag_and_stop_values_match_the_header():
    from orb_slam2_2021_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "orbfe_poseopt.h")).read()
    for name, value in (("FLAG_LARGE_STEP", L.POSEOPT_FLAG_LARGE_STEP), ("FLAG_NONFINITE", L.POSEOPT_FLAG_NONFINITE),
                        ("STOP_ALL", L.POSEOPT_STOP_ALL), ("STOP_TERMINATE", L.POSEOPT_STOP_TERMINATE),
                        ("STOP_NBAD", L.POSEOPT_STOP_NBAD), ("STOP_NO_EDGE", L.POSEOPT_STOP_NO_EDGE)):
        m = re.search(r"#define ORBFE_POSEOPT_%s (\d+)" % name, src)
        assert m and int(m.group(1)) == value, name


def test_create_bounds():
    from orb_slam2_2021_amd import _lib as L
    lib = L.lib()
    h = c_void_p()
    for args in ((0, 100), (65, 100), (4, 0), (4, 4097), (-1, 100)):
        assert lib.orbfe_poseopt_create(-1, *args, byref(h)) == L.ORBFE_ERR_ARG, args
        assert not h.value
    assert b"1..64" in lib.orbfe_last_error()
    assert lib.orbfe_poseopt_create(-1, 4, 100, None) == L.ORBFE_ERR_ARG
    assert lib.orbfe_poseopt_create(-1, 64, 4096, byref(h)) == L.ORBFE_OK and h.value
    assert lib.orbfe_poseopt_destroy(h) == L.ORBFE_OK
    assert lib.orbfe_poseopt_destroy(None) == L.ORBFE_OK


def status(opt, problems):
    from orb_slam2_2021_amd import OrbfeError
    try:
        opt.optimize(problems)
    except OrbfeError as e:
        return e.status, str(e)
    return 0, ""


def test_host_only_solve_is_a_state_error_after_the_checks():
    from orb_slam2_2021_amd import PoseOptimizer, _lib as L
    opt = PoseOptimizer(2, 64, device=-1)
    st, msg = status(opt, [case("n10")])
    assert st == L.ORBFE_ERR_STATE and "host-only" in msg
    assert status(opt, [case("n2")])[0] == L.ORBFE_ERR_STATE  # < 3 correspondences is a valid request
    assert status(opt, [case("n64"), case("n3")])[0] == L.ORBFE_ERR_STATE
    opt.close()


def test_capacity_checks():
    from orb_slam2_2021_amd import PoseOptimizer, _lib as L
    opt = PoseOptimizer(2, 64, device=-1)
    assert status(opt, [case("n3"), case("n9"), case("n10")])[0] == L.ORBFE_ERR_CAPACITY
    st, msg = status(opt, [case("n65")])
    assert st == L.ORBFE_ERR_CAPACITY and "max_obs" in msg
    opt.close()


def test_null_arrays_and_bad_arguments():
    from orb_slam2_2021_amd import _lib as L
    lib = L.lib()
    h = c_void_p()
    assert lib.orbfe_poseopt_create(-1, 2, 128, byref(h)) == L.ORBFE_OK
    p = case("n65")
    mask = np.zeros(2, np.uint64)

    def problem(**over):
        f = dict(n=p.n, valid=L.ptr(p.valid), xw=L.ptr(p.xw), kp_un=L.ptr(p.kp_un), u_right=L.ptr(p.u_right),
                 inv_sigma2=L.ptr(p.inv_sigma2), bf=float(p.bf))
        f.update(over)
        s = L.poseopt_problem(**f)
        s.k[:] = [float(v) for v in p.k]
        s.tcw[:] = [float(v) for v in p.tcw]
        return s

    def run(s, r=None, count=1):
        S = (L.poseopt_problem * 1)(s)
        R = (L.poseopt_result * 1)(r if r is not None else L.poseopt_result(mask_words=2, outlier_mask=L.ptr(mask)))
        return lib.orbfe_poseopt_batch(h, S, count, R)

    assert run(problem()) == L.ORBFE_ERR_STATE
    assert run(problem(), L.poseopt_result()) == L.ORBFE_ERR_STATE  # no mask asked for
    for name in ("valid", "xw", "kp_un", "u_right", "inv_sigma2"):
        assert run(problem(**{name: None})) == L.ORBFE_ERR_ARG, name
    assert run(problem(n=0, valid=None, xw=None, kp_un=None, u_right=None, inv_sigma2=None)) == L.ORBFE_ERR_STATE
    assert run(problem(n=-1)) == L.ORBFE_ERR_ARG
    assert run(problem(n=129)) == L.ORBFE_ERR_CAPACITY
    assert run(problem(), L.poseopt_result(mask_words=1, outlier_mask=L.ptr(mask))) == L.ORBFE_ERR_CAPACITY
    assert run(problem(), L.poseopt_result(mask_words=-1)) == L.ORBFE_ERR_ARG
    assert run(problem(), count=0) == L.ORBFE_ERR_ARG
    assert run(problem(), count=3) == L.ORBFE_ERR_CAPACITY
    assert lib.orbfe_poseopt_batch(None, None, 1, None) == L.ORBFE_ERR_ARG
    assert lib.orbfe_poseopt_batch(h, None, 1, None) == L.ORBFE_ERR_ARG
    S = (L.poseopt_problem * 1)(problem())
    assert lib.orbfe_poseopt_batch(h, S, 1, None) == L.ORBFE_ERR_ARG
    assert lib.orbfe_poseopt_destroy(h) == L.ORBFE_OK
