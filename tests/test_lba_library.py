"""orbfe_lba.h at the boundary, without a GPU: a host-only handle, the hard caps, every ORBFE_ERR_ARG
and ORBFE_ERR_CAPACITY path of orbfe_lba_solve, and the struct layouts of _lib.py against the header."""
import ctypes
import os
import re

import numpy as np
import pytest

from lba_scenes import case, edit
from orb_slam2_2021_amd import LocalBundleAdjuster, OrbfeError
from orb_slam2_2021_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -2, -4


def status_of(fn):
    with pytest.raises(OrbfeError) as e:
        fn()
    return int(re.search(r"status (-?\d+)", str(e.value)).group(1))


def host(p, **kw):
    a = dict(max_free_kf=max(int((p.fixed == 0).sum()), 1), max_kf=p.n_kf, max_points=p.n_points, max_edges=p.n_edges)
    a.update(kw)
    return LocalBundleAdjuster(device=-1, **a)


def test_host_only_handle_checks_arguments_and_refuses_to_solve():
    p = case("tiny")
    adj = host(p)
    assert status_of(lambda: adj.solve(p)) == ERR_STATE
    adj.close()
    adj.close()


@pytest.mark.parametrize("args", [(0, 4, 10, 10), (129, 512, 10, 10), (4, 513, 10, 10), (4, 3, 10, 10), (4, 8, 0, 10),
                                  (4, 8, 16385, 10), (4, 8, 10, 0), (4, 8, 10, 131073)])
def test_create_refuses_bounds_outside_the_hard_caps(args):
    assert status_of(lambda: LocalBundleAdjuster(*args, device=-1)) == ERR_ARG


def test_the_hard_caps_themselves_are_accepted():
    LocalBundleAdjuster(L.LBA_MAX_FREE_KF, L.LBA_MAX_KF, L.LBA_MAX_POINTS, L.LBA_MAX_EDGES, device=-1).close()


def test_capacity_past_the_handles_bounds():
    p = case("tiny")
    for kw in (dict(max_kf=p.n_kf - 1, max_free_kf=1), dict(max_points=p.n_points - 1), dict(max_edges=p.n_edges - 1),
               dict(max_free_kf=1)):
        adj = host(p, **kw)
        assert status_of(lambda: adj.solve(p)) == ERR_CAPACITY, kw
        adj.close()


def test_every_err_arg_path():
    p = case("tiny")
    adj = host(p)
    bad_kf = p.edge_kf.copy()
    bad_kf[3] = p.n_kf
    neg_kf = p.edge_kf.copy()
    neg_kf[0] = -1
    twice = p.edge_kf.copy()
    twice[p.edge_begin[2] + 1] = twice[p.edge_begin[2]]
    not_csr = p.edge_begin.copy()
    not_csr[-1] -= 1
    first = p.edge_begin.copy()
    first[0] = 1
    backwards = p.edge_begin.copy()
    backwards[4], backwards[5] = backwards[5], backwards[4]
    for what, q in (("index past n_kf", edit(p, edge_kf=bad_kf)), ("negative index", edit(p, edge_kf=neg_kf)),
                    ("keyframe twice under a point", edit(p, edge_kf=twice)), ("last != n_edges", edit(p, edge_begin=not_csr)),
                    ("first != 0", edit(p, edge_begin=first)), ("descending", edit(p, edge_begin=backwards)),
                    ("stop_at_poll", edit(p, stop_at_poll=-2))):
        assert status_of(lambda: adj.solve(q)) == ERR_ARG, what
    lib = L.lib()
    P, R = L.lba_problem(), L.lba_result()
    assert lib.orbfe_lba_solve(None, ctypes.byref(P), ctypes.byref(R)) == ERR_ARG
    assert lib.orbfe_lba_solve(adj._h, None, ctypes.byref(R)) == ERR_ARG
    P.n_kf, P.n_points, P.n_edges = 1, 1, 1
    assert lib.orbfe_lba_solve(adj._h, ctypes.byref(P), ctypes.byref(R)) == ERR_ARG  # null arrays
    P.n_kf = -1
    assert lib.orbfe_lba_solve(adj._h, ctypes.byref(P), ctypes.byref(R)) == ERR_ARG
    adj.close()


def test_mask_words_below_the_edges_is_a_capacity_error():
    p = case("lanes")
    adj = host(p)
    lib = L.lib()
    keep = {n: np.ascontiguousarray(getattr(p, n)) for n in ("tcw", "k", "bf", "fixed", "xw", "edge_begin", "edge_kf", "kp_un",
                                                              "u_right", "inv_sigma2")}
    P, R = L.lba_problem(), L.lba_result()
    P.n_kf, P.n_points, P.n_edges, P.stop_at_poll = p.n_kf, p.n_points, p.n_edges, -1
    for n, a in keep.items():
        setattr(P, n, L.ptr(a))
    tcw, xw, mask = np.zeros(12 * p.n_kf, np.float32), np.zeros(3 * p.n_points, np.float32), np.zeros(64, np.uint64)
    R.tcw, R.xw, R.erase_mask, R.mask_words = L.ptr(tcw), L.ptr(xw), L.ptr(mask), (p.n_edges + 63) // 64 - 1
    assert lib.orbfe_lba_solve(adj._h, ctypes.byref(P), ctypes.byref(R)) == ERR_CAPACITY
    R.mask_words = (p.n_edges + 63) // 64
    assert lib.orbfe_lba_solve(adj._h, ctypes.byref(P), ctypes.byref(R)) == ERR_STATE  # past every check
    adj.close()


def header_fields(text, name):
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = [re.sub(r"\[.*?\]", "", n).replace("*", "").strip() for n in decl.split(",")]
        names[0] = names[0].split()[-1]
        out += names
    return out


def test_struct_layouts_match_the_header():
    text = open(os.path.join(ROOT, "include", "orbfe_lba.h")).read()
    rename = {"lambda": "lam"}
    for cname, cls in (("orbfe_lba_problem_t", L.lba_problem), ("orbfe_lba_round_t", L.lba_round),
                       ("orbfe_lba_result_t", L.lba_result)):
        want = [rename.get(n, n) for n in header_fields(text, cname)]
        assert [f[0] for f in cls._fields_] == want, cname
    assert ctypes.sizeof(L.lba_round) == 40 and ctypes.sizeof(L.lba_result) == 5 * 8 + 4 * 4 + 2 * 40
    assert ctypes.sizeof(L.lba_problem) == 3 * 4 + 4 + 11 * 8 + 8
    for n in ("MAX_FREE_KF", "MAX_KF", "MAX_POINTS", "MAX_EDGES", "FLAG_LARGE_STEP", "FLAG_NONFINITE", "STOP_ALL",
              "STOP_TERMINATE", "STOP_NBAD", "STOP_NO_EDGE", "STOP_FLAG"):
        value = int(re.search(r"#define ORBFE_LBA_%s (\d+)" % n, text).group(1))
        assert getattr(L, "LBA_" + n) == value, n
