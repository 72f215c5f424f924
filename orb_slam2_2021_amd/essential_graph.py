"""Optimizer::OptimizeEssentialGraph on MI355X (include/orbfe_essgraph.h): the pose-graph Levenberg-
Marquardt over Sim3 keyframe vertices that LoopClosing::CorrectLoop runs after a loop is accepted.

Mirrors src/Optimizer.cc:784-1048 of the reference. `problem_of_essential_graph` performs the gather of
:800-988 from KeyFrame objects and the covisibility / spanning-tree / loop-edge tables;
`EssentialGraphOptimizer` is the device handle; `OptimizeEssentialGraph(...)` writes the poses and the
point positions back. UpdateNormalAndDepth stays with the caller.
"""
from __future__ import annotations

from ctypes import byref, c_void_p
from types import SimpleNamespace
from typing import Dict, Iterable, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

MAX_VERTICES, MAX_EDGES, MAX_ENV_BLOCKS, MAX_POINTS = (L.ESSGRAPH_MAX_VERTICES, L.ESSGRAPH_MAX_EDGES,
                                                       L.ESSGRAPH_MAX_ENV_BLOCKS, L.ESSGRAPH_MAX_POINTS)
MIN_FEAT = 100  # const int minFeat = 100


def problem_of_essential_graph(keyframes: Mapping[int, object], loop_kf: int, cur_kf: int,
                               non_corrected: Mapping[int, Sequence[float]], corrected: Mapping[int, Sequence[float]],
                               loop_connections: Mapping[int, Iterable[int]], parents: Mapping[int, Optional[int]],
                               children: Mapping[int, Iterable[int]], loop_edges: Mapping[int, Iterable[int]],
                               covisibles_by_weight: Mapping[int, Sequence[Tuple[int, int]]],
                               points: Mapping[int, np.ndarray], point_refs: Mapping[int, int],
                               fix_scale: bool) -> SimpleNamespace:
    """keyframes: mnId -> KeyFrame (tcw; an optional `bad`); loop_kf / cur_kf: the mnIds of pLoopKF / pCurKF;
    non_corrected / corrected: mnId -> (q x y z w, t, s); loop_connections: mnId -> the mnIds of its set;
    parents: mnId -> GetParent() or None; children: mnId -> GetChilds(); loop_edges: mnId -> GetLoopEdges();
    covisibles_by_weight: mnId -> [(mnId, weight)] in GetCovisiblesByWeight's order (GetWeight reads it, 0 when
    absent); points: mnId -> GetWorldPos(); point_refs: point mnId -> the keyframe of :1025-1034.

    Bad keyframes are no vertices and no edge reaches them. The edges come in a fixed order (the
    reference's follows pointer-ordered containers): the loop connections by ascending (mnId, mnId), then
    per keyframe ascending in mnId its spanning-tree edge, its loop edges ascending, its covisibility
    edges in by-weight order. The problem carries kf_ids, point_ids and edge_pairs (mnId of vertex 0,
    mnId of vertex 1, kind)."""
    kf_ids = sorted(int(k) for k, kf in keyframes.items() if not getattr(kf, "bad", False))
    index = {kid: i for i, kid in enumerate(kf_ids)}
    if int(loop_kf) not in index:
        raise ValueError("the loop keyframe is not among the good keyframes")
    weight = {kid: {int(o): int(w) for o, w in covisibles_by_weight.get(kid, ())} for kid in kf_ids}
    tcw = np.zeros((len(kf_ids), 12), np.float32)
    for i, kid in enumerate(kf_ids):
        tcw[i] = np.asarray(keyframes[kid].tcw, np.float32).reshape(-1)[:12]
    edges, inserted = [], set()
    for kid in sorted(int(k) for k in loop_connections):  # :853-885
        if kid not in index:
            continue
        for other in sorted(int(o) for o in loop_connections[kid]):
            if other not in index:
                continue
            if (kid != int(cur_kf) or other != int(loop_kf)) and weight[kid].get(other, 0) < MIN_FEAT:
                continue
            edges.append((kid, other, 0))
            inserted.add((min(kid, other), max(kid, other)))
    for kid in kf_ids:  # :887-988
        parent = parents.get(kid)
        parent = int(parent) if parent is not None else None
        if parent is not None and parent in index:
            edges.append((kid, parent, 1))
        loops = set(int(o) for o in loop_edges.get(kid, ()))
        for other in sorted(loops):
            if other < kid and other in index:
                edges.append((kid, other, 1))
        kids = set(int(o) for o in children.get(kid, ()))
        for other, w in covisibles_by_weight.get(kid, ()):
            other = int(other)
            if int(w) < MIN_FEAT or other == parent or other in kids or other in loops:
                continue
            if other not in index or not other < kid:
                continue
            if (min(kid, other), max(kid, other)) in inserted:
                continue
            edges.append((kid, other, 1))

    def table(m):
        ids = sorted(int(k) for k in m if int(k) in index)
        return (np.array([index[k] for k in ids], np.int32),
                np.array([np.asarray(m[k], np.float64).reshape(8) for k in ids], np.float64).reshape(-1, 8))

    corrected_idx, corrected_sim3 = table(corrected)
    noncorrected_idx, noncorrected_sim3 = table(non_corrected)
    point_ids = sorted(int(i) for i in points)
    xw = np.array([np.asarray(points[i], np.float32).reshape(3) for i in point_ids], np.float32).reshape(-1, 3)
    point_ref = np.array([index[int(point_refs[i])] for i in point_ids], np.int32)
    return SimpleNamespace(
        n_vertices=len(kf_ids), tcw=tcw, fixed_vertex=index[int(loop_kf)], fix_scale=1 if fix_scale else 0,
        n_corrected=len(corrected_idx), corrected_idx=corrected_idx, corrected_sim3=corrected_sim3,
        n_noncorrected=len(noncorrected_idx), noncorrected_idx=noncorrected_idx, noncorrected_sim3=noncorrected_sim3,
        n_edges=len(edges), edge_i=np.array([index[e[0]] for e in edges], np.int32),
        edge_j=np.array([index[e[1]] for e in edges], np.int32), edge_kind=np.array([e[2] for e in edges], np.uint8),
        n_points=len(point_ids), xw=xw, point_ref=point_ref, kf_ids=kf_ids, point_ids=point_ids, edge_pairs=edges)


def envelope_blocks(p) -> int:
    """The 7x7 blocks the problem's envelope holds (what max_env_blocks bounds)"""
    used = np.zeros(int(p.n_vertices), bool)
    used[np.asarray(p.edge_i, np.int64)] = True
    used[np.asarray(p.edge_j, np.int64)] = True
    used[int(p.fixed_vertex)] = False
    slot = np.cumsum(used) - 1
    first = np.arange(int(used.sum()))
    for i, j in zip(np.asarray(p.edge_i), np.asarray(p.edge_j)):
        if used[i] and used[j]:
            a, b = int(slot[i]), int(slot[j])
            first[max(a, b)] = min(first[max(a, b)], min(a, b))
    return int((np.arange(len(first)) - first + 1).sum())


class EssentialGraphOptimizer:
    """The device handle: a workspace for pose graphs up to the given bounds; reused from call to call.
    device < 0 gives a host-only handle (argument checks only)."""

    def __init__(self, max_vertices: int = 1024, max_edges: int = 8192, max_env_blocks: int = 65536,
                 max_points: int = 131072, device: int = 0):
        self._lib = L.lib()
        h = c_void_p()
        L.check(self._lib.orbfe_essgraph_create(int(device), int(max_vertices), int(max_edges), int(max_env_blocks),
                                                int(max_points), byref(h)), "orbfe_essgraph_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.orbfe_essgraph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, p) -> SimpleNamespace:
        """orbfe_essgraph_solve -> tcw (n_vertices, 12) float32, xw (n_points, 3) float32 and trace
        (iterations, trials, rejected_trials, stop, lam, chi2, env_blocks, flags)."""
        nv, ne, npt = int(p.n_vertices), int(p.n_edges), int(p.n_points)
        nc, nn = int(p.n_corrected), int(p.n_noncorrected)
        a = dict(tcw=(p.tcw, np.float32, 12 * nv), corrected_idx=(p.corrected_idx, np.int32, nc),
                 corrected_sim3=(p.corrected_sim3, np.float64, 8 * nc), noncorrected_idx=(p.noncorrected_idx, np.int32, nn),
                 noncorrected_sim3=(p.noncorrected_sim3, np.float64, 8 * nn), edge_i=(p.edge_i, np.int32, ne),
                 edge_j=(p.edge_j, np.int32, ne), edge_kind=(p.edge_kind, np.uint8, ne), xw=(p.xw, np.float32, 3 * npt),
                 point_ref=(p.point_ref, np.int32, npt))
        P, R, keep = L.essgraph_problem(), L.essgraph_result(), {}
        P.n_vertices, P.fixed_vertex, P.fix_scale = nv, int(p.fixed_vertex), int(p.fix_scale)
        P.n_corrected, P.n_noncorrected, P.n_edges, P.n_points = nc, nn, ne, npt
        for name, (src, dtype, count) in a.items():
            arr = np.ascontiguousarray(src, dtype).reshape(-1)
            if len(arr) != count:
                raise ValueError(f"{name} must hold {count} values")
            keep[name] = arr if count else np.zeros(1, dtype)
            setattr(P, name, L.ptr(keep[name]))
        tcw, xw = np.zeros(max(12 * nv, 1), np.float32), np.zeros(max(3 * npt, 1), np.float32)
        R.tcw, R.xw = L.ptr(tcw), L.ptr(xw)
        L.check(self._lib.orbfe_essgraph_solve(self._h, byref(P), byref(R)), "orbfe_essgraph_solve")
        t = R.trace
        trace = SimpleNamespace(iterations=t.iterations, trials=t.trials, rejected_trials=t.rejected_trials, stop=t.stop,
                                lam=float(t.lam), chi2=float(t.chi2), env_blocks=t.env_blocks, flags=int(t.flags))
        return SimpleNamespace(tcw=tcw[:12 * nv].reshape(nv, 12), xw=xw[:3 * npt].reshape(npt, 3), trace=trace)


def OptimizeEssentialGraph(keyframes: Dict[int, object], loop_kf: int, cur_kf: int,
                           non_corrected: Mapping[int, Sequence[float]], corrected: Mapping[int, Sequence[float]],
                           loop_connections: Mapping[int, Iterable[int]], parents: Mapping[int, Optional[int]],
                           children: Mapping[int, Iterable[int]], loop_edges: Mapping[int, Iterable[int]],
                           covisibles_by_weight: Mapping[int, Sequence[Tuple[int, int]]], points: Dict[int, np.ndarray],
                           point_refs: Mapping[int, int], fix_scale: bool,
                           optimizer: Optional[EssentialGraphOptimizer] = None, device: int = 0) -> SimpleNamespace:
    """void Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
    LoopConnections, bFixScale): sets tcw of every good keyframe (SetPose) and every point's position
    (SetWorldPos) in place and returns the trace. Without `optimizer` a handle sized for this graph is
    created for the call."""
    p = problem_of_essential_graph(keyframes, loop_kf, cur_kf, non_corrected, corrected, loop_connections, parents,
                                   children, loop_edges, covisibles_by_weight, points, point_refs, fix_scale)
    own = optimizer is None
    if own:
        optimizer = EssentialGraphOptimizer(max(p.n_vertices, 1), max(p.n_edges, 1), max(envelope_blocks(p), 1),
                                            p.n_points, device)
    try:
        r = optimizer.solve(p)
    finally:
        if own:
            optimizer.close()
    for i, kid in enumerate(p.kf_ids):
        keyframes[kid].tcw = r.tcw[i].reshape(3, 4).copy()
    for i, pid in enumerate(p.point_ids):
        points[pid] = r.xw[i].copy()
    return r.trace
