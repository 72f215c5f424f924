"""Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:784-1048 of the reference) restated in Python floats,
with numpy.float32 only where the reference narrows: the yardstick for orbfe_essgraph_core.h on the host
and for the kernels of orbfe_essgraph.hip on the GPU, compared bit for bit.

One function per rule, the same code as the core header. The quaternion rules, sin / cos, IEEE division
and sqrt and the lane tree are those of tests/poseopt_ref.py, Sim3, exp and oplus
those of tests/optsim3_ref.py (section 19); what is new is log and acos from + - * / sqrt, Sim3::log()
with its 3x3 partial-pivot LU, EdgeSim3, the pose-graph system and the LDL^T over the block envelope
(section 21). EIGEN: and DEVIATION: mark lines as they do there.

Summation: a vertex's H_ii and b_i run over its incident edges in ascending edge index from +0.0, an
off-diagonal block over its edges likewise; for the total chi2 edge e, and for computeScale slot s,
belongs to lane index % 64, a lane adds in ascending index from +0.0, the lanes are combined by
s[l] += s[l + stride], stride = 32 .. 1.
"""
from types import SimpleNamespace

import numpy as np

from lm_ref import (DBL_MAX, FLAG_LARGE_STEP, FLAG_NONFINITE, NAN, PO_LANES, STOP_ALL, STOP_NBAD,  # noqa: F401
                    STOP_NO_EDGE, STOP_TERMINATE, div, finite, levenberg, tree)
from optsim3_ref import exp, flat, oplus, sim3_inverse, sim3_map, sim3_mul  # noqa: F401
from poseopt_ref import bits64, c_sqrt, quat_from_matrix, quat_rotate, quat_to_matrix, sincos  # noqa: F401

DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
MAX_ITER = 20
INF = float("inf")

LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
LG = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
      1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)


def log(x):
    """DEVIATION: replaces std::log. x = m 2^k with m in [sqrt(1/2), sqrt(2)) by exact halvings /
    doublings, then fdlibm's e_log.c on f = m - 1."""
    if x != x:
        return x
    if x < 0.0:
        return NAN
    if x == 0.0:
        return -INF
    if x > DBL_MAX:
        return x
    m, k = x, 0
    it = 0
    while it < 1100 and m >= 1.4142135623730951:
        m, k, it = m * 0.5, k + 1, it + 1
    it = 0
    while it < 1100 and m < 0.70710678118654757:
        m, k, it = m * 2.0, k - 1, it + 1
    f = m - 1.0
    dk = float(k)
    if abs(f) < 9.5367431640625e-07:
        if f == 0.0:
            return 0.0 if k == 0 else dk * LN2_HI + dk * LN2_LO
        R = f * f * (0.5 - 0.33333333333333333 * f)
        return f - R if k == 0 else dk * LN2_HI - ((R - dk * LN2_LO) - f)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (LG[1] + w * (LG[3] + w * LG[5]))
    t2 = z * (LG[0] + w * (LG[2] + w * (LG[4] + w * LG[6])))
    R = t2 + t1
    mo = m * 2.0 if m < 1.0 else m
    if mo >= 1.3799991607666016 and mo < 1.4200000762939453:
        hfsq = 0.5 * f * f
        return f - (hfsq - s * (hfsq + R)) if k == 0 else dk * LN2_HI - ((hfsq - (s * (hfsq + R) + dk * LN2_LO)) - f)
    return f - s * (f - R) if k == 0 else dk * LN2_HI - ((s * (f - R) - dk * LN2_LO) - f)


PIO2_HI, PIO2_LO, PI = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00
PS = (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
      7.91534994289814532176e-04, 3.47933107596021167570e-05)
QS = (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)


def _acos_r(z):
    p = z * (PS[0] + z * (PS[1] + z * (PS[2] + z * (PS[3] + z * (PS[4] + z * PS[5])))))
    q = 1.0 + z * (QS[0] + z * (QS[1] + z * (QS[2] + z * QS[3])))
    return p / q


def acos(x):
    """DEVIATION: replaces std::acos. fdlibm's e_acos.c; the head of sqrt(z) by Veltkamp's split."""
    if x != x:
        return x
    ax = abs(x)
    if ax >= 1.0:
        if ax == 1.0:
            return 0.0 if x > 0 else PI + 2.0 * PIO2_LO
        return NAN
    if ax < 0.5:
        if ax <= 6.938893903907228e-18:
            return PIO2_HI + PIO2_LO
        r = _acos_r(x * x)
        return PIO2_HI - (x - (PIO2_LO - x * r))
    if x < 0:
        z = (1.0 + x) * 0.5
        r = _acos_r(z)
        s = c_sqrt(z)
        w = r * s - PIO2_LO
        return PI - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = c_sqrt(z)
    t = s * 134217729.0
    df = t - (t - s)
    c = (z - df * df) / (s + df)
    r = _acos_r(z)
    w = r * s + c
    return 2.0 * (df + w)


def lu3_solve(W, t):
    """EIGEN: PartialPivLU<Matrix3d>::compute (unblocked) and solve: the first largest |entry| of the
    column is the pivot, a non-zero pivot divides the column below, the rank-1 update; P b, the unit
    lower solve by columns, the upper solve by columns from the last."""
    a = list(W)
    x = list(t)
    for k in range(3):
        big, best = k, abs(a[4 * k])
        for i in range(k + 1, 3):
            if abs(a[3 * i + k]) > best:
                big, best = i, abs(a[3 * i + k])
        if big != k:
            for c in range(3):
                a[3 * k + c], a[3 * big + c] = a[3 * big + c], a[3 * k + c]
            x[k], x[big] = x[big], x[k]
        if best != 0.0:
            for i in range(k + 1, 3):
                a[3 * i + k] = div(a[3 * i + k], a[4 * k])
        for i in range(k + 1, 3):
            for c in range(k + 1, 3):
                a[3 * i + c] = a[3 * i + c] - a[3 * i + k] * a[3 * k + c]
    x[1] = x[1] - x[0] * a[3]
    x[2] = x[2] - x[0] * a[6]
    x[2] = x[2] - x[1] * a[7]
    x[2] = div(x[2], a[8])
    x[0] = x[0] - x[2] * a[2]
    x[1] = x[1] - x[2] * a[5]
    x[1] = div(x[1], a[4])
    x[0] = x[0] - x[1] * a[1]
    x[0] = div(x[0], a[0])
    return x


def log_branch(S):
    """-> (|sigma| < eps, d > 1 - eps): which of the four branches Sim3::log() takes"""
    R = quat_to_matrix(S[0])
    d = 0.5 * (((R[0] + R[4]) + R[8]) - 1)
    return abs(log(S[2])) < 0.00001, d > 1 - 0.00001


def sim3_log(S):
    """Sim3::log() (sim3.h:148-230) -> 7 doubles"""
    q, t, s = S
    sigma = log(s)
    R = quat_to_matrix(q)
    d = 0.5 * (((R[0] + R[4]) + R[8]) - 1)
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    eps = 0.00001
    near = d > 1 - eps
    theta, sn, cs = 0.0, 0.0, 1.0
    if near:
        om = [0.5 * dR[0], 0.5 * dR[1], 0.5 * dR[2]]
    else:
        theta = acos(d)
        f = div(theta, 2 * c_sqrt(1 - d * d))
        om = [f * dR[0], f * dR[1], f * dR[2]]
        sn, cs, _ = sincos(theta)
    if abs(sigma) < eps:
        C = 1.0
        if near:
            A = 1. / 2.
            B = 1. / 6.
        else:
            theta2 = theta * theta
            A = div(1 - cs, theta2)
            B = div(theta - sn, theta2 * theta)
    else:
        C = div(s - 1, sigma)
        if near:
            sigma2 = sigma * sigma
            A = div((sigma - 1) * s + 1, sigma2)
            B = div((0.5 * sigma2 - sigma + 1) * s, sigma2 * sigma)
        else:
            theta2 = theta * theta
            a = s * sn
            b = s * cs
            c = theta2 + sigma * sigma
            A = div(a * sigma + (1 - b) * theta, theta * c)
            B = div((C - div((b - 1) * sigma + a * theta, c)) * 1., theta2)
    O = [0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0]
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    W = [0.0] * 9
    for r in range(3):
        for c in range(3):
            bo2 = ((B * O[3 * r]) * O[c] + (B * O[3 * r + 1]) * O[3 + c]) + (B * O[3 * r + 2]) * O[6 + c]
            W[3 * r + c] = (A * O[3 * r + c] + bo2) + C * I[3 * r + c]
    up = lu3_solve(W, t)
    return [om[0], om[1], om[2], up[0], up[1], up[2], sigma]


def edge_error(C, Si, Sj):
    """EdgeSim3::computeError: (C * v0.estimate() * v1.estimate().inverse()).log()"""
    return sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inverse(Sj)))


def chi2_of(e):
    s = e[0] * e[0]
    for k in range(1, 7):
        s = s + e[k] * e[k]
    return s


def sim3_of(a):
    return ([float(v) for v in a[0:4]], [float(v) for v in a[4:7]], float(a[7]))


def start_states(p):
    """Optimizer.cc:812-847 -> (vScw, the measurement-side states)"""
    corr = {int(i): sim3_of(s) for i, s in zip(p.corrected_idx, np.asarray(p.corrected_sim3, np.float64).reshape(-1, 8))}
    nonc = {int(i): sim3_of(s) for i, s in zip(p.noncorrected_idx, np.asarray(p.noncorrected_sim3, np.float64).reshape(-1, 8))}
    tcw = np.asarray(p.tcw, np.float32).reshape(-1, 12)
    scw, mst = [], []
    for v in range(p.n_vertices):
        if v in corr:
            S = corr[v]
        else:
            T = [float(x) for x in tcw[v]]
            S = (quat_from_matrix([T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]]), [T[3], T[7], T[11]], 1.0)
        scw.append(S)
        mst.append(nonc.get(v, S))
    return scw, mst


def jacobian(C, Si, Sj, fix_scale, fixed_side):
    """BaseBinaryEdge::linearizeOplus -> (the error, J: 7 rows of 14; a fixed vertex's columns are zero)"""
    err = edge_error(C, Si, Sj)
    J = [[0.0] * 14 for _ in range(7)]
    for side in (0, 1):
        if side == fixed_side:
            continue
        for d in range(7):
            es = []
            for delta in (DELTA, -DELTA):
                u = [0.0] * 7
                u[d] = delta
                P, _ = oplus(u, fix_scale, Sj if side else Si)
                es.append(edge_error(C, Si, P) if side else edge_error(C, P, Sj))
            for k in range(7):
                J[k][7 * side + d] = SCALAR * (es[0][k] - es[1][k])
    return err, J


def edge_products(J, err):
    """EIGEN: (J^T J)_rc = sum_k J_kr J_kc, b_r = sum_k J_kr (-e_k), k ascending -> (ii, jj, ij, bi, bj)"""
    def dot(a, b):
        s = J[0][a] * J[0][b]
        for k in range(1, 7):
            s = s + J[k][a] * J[k][b]
        return s

    def bdot(a):
        s = J[0][a] * -err[0]
        for k in range(1, 7):
            s = s + J[k][a] * -err[k]
        return s

    ii = [[dot(r, c) for c in range(7)] for r in range(7)]
    jj = [[dot(7 + r, 7 + c) for c in range(7)] for r in range(7)]
    ij = [[dot(r, 7 + c) for c in range(7)] for r in range(7)]
    return ii, jj, ij, [bdot(r) for r in range(7)], [bdot(7 + r) for r in range(7)]


def envelope(p):
    """-> (slot_of_v, v_of_slot, row_first, blocks): the free vertices that have an edge, renumbered in
    order; row s holds the block columns row_first[s] .. s"""
    used = [False] * p.n_vertices
    for i, j in zip(p.edge_i, p.edge_j):
        used[int(i)] = used[int(j)] = True
    slot_of_v, v_of_slot = [-1] * p.n_vertices, []
    for v in range(p.n_vertices):
        if used[v] and v != p.fixed_vertex:
            slot_of_v[v] = len(v_of_slot)
            v_of_slot.append(v)
    first = list(range(len(v_of_slot)))
    for i, j in zip(p.edge_i, p.edge_j):
        a, b = slot_of_v[int(i)], slot_of_v[int(j)]
        if a >= 0 and b >= 0:
            first[max(a, b)] = min(first[max(a, b)], min(a, b))
    return slot_of_v, v_of_slot, first, sum(s - first[s] + 1 for s in range(len(first)))


def ldlt_envelope(rows, c0, b, x_prev):
    """DEVIATION: the unpivoted LDL^T in natural order over the envelope. rows[i]: the entries of scalar
    row i from column c0[i] to i (H + lambda I); entry (i, j): v = A_ij; v -= (L_ik d_k) L_jk for k
    ascending inside both envelopes; L_ij = v / d_j. A d_i that is 0, or not finite (FLAG_NONFINITE),
    fails. -> (ok, x, flags); x keeps its previous value after a failure."""
    n = len(rows)
    Lr = [list(r) for r in rows]
    d = [0.0] * n
    for i in range(n):
        ci, Li = c0[i], Lr[i]
        for j in range(ci, i + 1):
            cj, Lj = c0[j], Lr[j]
            v = Li[j - ci]
            for k in range(max(ci, cj), j):
                v = v - (Li[k - ci] * d[k]) * Lj[k - cj]
            if j < i:
                Li[j - ci] = v / d[j]
            else:
                d[i] = v
                if not finite(v):
                    return False, x_prev, FLAG_NONFINITE
                if v == 0.0:
                    return False, x_prev, 0
    y = [0.0] * n
    for i in range(n):
        v = b[i]
        for k in range(c0[i], i):
            v = v - Lr[i][k - c0[i]] * y[k]
        y[i] = v
    for i in range(n):
        y[i] = div(y[i], d[i])
    for k in range(n - 1, -1, -1):
        for i in range(c0[k], k):
            y[i] = y[i] - Lr[k][i - c0[k]] * y[k]
    return True, y, 0


def ldlt_dense(A, b):
    """Section 20's dense unpivoted LDL^T on the full lower triangle A (list of rows) -> x, or None"""
    n = len(A)
    L = [[0.0] * n for _ in range(n)]
    d = [0.0] * n
    for j in range(n):
        for i in range(j, n):
            v = A[i][j]
            for k in range(j):
                v = v - (L[i][k] * d[k]) * L[j][k]
            if i == j:
                d[j] = v
                if not finite(v) or v == 0.0:
                    return None
            else:
                L[i][j] = v / d[j]
    y = list(b)
    for k in range(n):
        for i in range(k + 1, n):
            y[i] = y[i] - L[i][k] * y[k]
    y = [div(y[i], d[i]) for i in range(n)]
    for k in range(n - 1, -1, -1):
        for i in range(k):
            y[i] = y[i] - L[k][i] * y[k]
    return y


class Solver:
    """The workspace of one solve: states, the structure, linearize / trial / accept as the backends of
    the core header have them."""

    def __init__(self, p):
        self.p = p
        self.fix_scale = bool(p.fix_scale)
        self.ne = int(p.n_edges)
        self.ei = [int(v) for v in p.edge_i]
        self.ej = [int(v) for v in p.edge_j]
        self.scw, mst = start_states(p)
        self.est = list(self.scw)
        self.tri = list(self.scw)
        self.meas = []
        for e in range(self.ne):
            src = self.scw if int(p.edge_kind[e]) == 0 else mst
            self.meas.append(sim3_mul(src[self.ej[e]], sim3_inverse(src[self.ei[e]])))
        self.slot_of_v, self.v_of_slot, self.first, self.env_blocks = envelope(p)
        self.ns = len(self.v_of_slot)
        self.c0 = [7 * self.first[i // 7] for i in range(7 * self.ns)]
        self.x = [0.0] * (7 * self.ns)  # DEVIATION: zero before the first successful solve
        self.flags = 0

    def total_chi(self, est):
        lanes = [[0.0] for _ in range(PO_LANES)]
        self.e_chi = [chi2_of(edge_error(self.meas[e], est[self.ei[e]], est[self.ej[e]])) for e in range(self.ne)]
        for e in range(self.ne):
            lanes[e % PO_LANES][0] = lanes[e % PO_LANES][0] + self.e_chi[e]
        return tree(lanes)[0]

    def linearize(self):
        """-> chi2 at the accepted estimates; builds the envelope rows (lambda not added) and b"""
        ns, fixed = self.ns, int(self.p.fixed_vertex)
        n = 7 * ns
        rows = [[0.0] * (i - self.c0[i] + 1) for i in range(n)]
        b = [0.0] * n
        lanes = [[0.0] for _ in range(PO_LANES)]
        off = {}
        self.errors = []
        for e in range(self.ne):
            vi, vj = self.ei[e], self.ej[e]
            err, J = jacobian(self.meas[e], self.est[vi], self.est[vj], self.fix_scale,
                              0 if vi == fixed else (1 if vj == fixed else -1))
            self.errors.append(err)
            lanes[e % PO_LANES][0] = lanes[e % PO_LANES][0] + chi2_of(err)
            ii, jj, ij, bi, bj = edge_products(J, err)
            a, c = self.slot_of_v[vi], self.slot_of_v[vj]
            for s, blk, bb in ((a, ii, bi), (c, jj, bj)):
                if s < 0:
                    continue
                for r in range(7):
                    row = rows[7 * s + r]
                    base = 7 * s - self.c0[7 * s + r]
                    for cc in range(r + 1):  # the lower triangle is what the factorisation reads
                        row[base + cc] = row[base + cc] + blk[r][cc]
                    b[7 * s + r] = b[7 * s + r] + bb[r]
            if a >= 0 and c >= 0:
                hi, lo = max(a, c), min(a, c)
                for r in range(7):
                    row = rows[7 * hi + r]
                    base = 7 * lo - self.c0[7 * hi + r]
                    for cc in range(7):
                        row[base + cc] = row[base + cc] + (ij[r][cc] if a > c else ij[cc][r])
        self.rows, self.b = rows, b
        return tree(lanes)[0]

    def trial(self, lam):
        """-> (chi2 at the trial estimates, computeScale, fail)"""
        n = 7 * self.ns
        rows = [list(r) for r in self.rows]
        for i in range(n):
            rows[i][-1] = rows[i][-1] + lam
        ok, x, fl = ldlt_envelope(rows, self.c0, self.b, self.x)
        self.flags |= fl
        self.x = list(x)
        for v in range(self.p.n_vertices):
            s = self.slot_of_v[v]
            if s < 0:
                self.tri[v] = self.est[v]
                continue
            u = self.x[7 * s:7 * s + 7]
            self.tri[v], fl = oplus(u, self.fix_scale, self.est[v])
            self.x[7 * s + 6] = u[6]  # oplusImpl zeroes the solver's x_6 in place with _fix_scale
            self.flags |= fl
        chi = self.total_chi(self.tri)
        lanes = [[0.0] for _ in range(PO_LANES)]
        for s in range(self.ns):
            v = 0.0
            for j in range(7):
                xj = self.x[7 * s + j]
                v = v + xj * (lam * xj + self.b[7 * s + j])
            lanes[s % PO_LANES][0] = lanes[s % PO_LANES][0] + v
        return chi, tree(lanes)[0], not ok

    def accept(self):
        self.est = list(self.tri)


def optimize(S, on_iteration=None):
    """SparseOptimizer::optimize(20) with OptimizationAlgorithmLevenberg::solve, lambda from
    setUserLambdaInit(1e-16), no stop flag -> the trace. on_iteration(i, ini, current), if given, sees
    every iteration's chi2 before and after its trials (tr.chis keeps them)."""
    tr = SimpleNamespace(iterations=0, trials=0, rejected_trials=0, stop=STOP_NO_EDGE, lam=0.0, chi2=0.0,
                         env_blocks=S.env_blocks, flags=0, chis=[])
    if S.ne == 0:
        return tr

    def each(i, ini, current):
        tr.chis.append((ini, current))
        if on_iteration:
            on_iteration(i, ini, current)

    t = levenberg(lambda: (S.linearize(), 0.0), S.trial, S.accept, MAX_ITER, user_lambda=1e-16, on_iteration=each)
    tr.iterations, tr.trials, tr.rejected_trials, tr.stop = t.iterations, t.trials, t.rejected_trials, t.stop
    tr.lam, tr.chi2, tr.flags = t.lam, t.chi2, S.flags
    return tr


def finish(S):
    """:997-1047 -> (tcw (nv, 12) float32, xw (np, 3) float32)"""
    p = S.p
    tcw = np.zeros((p.n_vertices, 12), np.float32)
    for v in range(p.n_vertices):
        q, t, s = S.est[v]
        m = quat_to_matrix(q)
        c = div(1., s)
        tcw[v] = [m[0], m[1], m[2], t[0] * c, m[3], m[4], m[5], t[1] * c, m[6], m[7], m[8], t[2] * c]
    xw_in = np.asarray(p.xw, np.float32).reshape(-1, 3)
    xw = np.zeros((int(p.n_points), 3), np.float32)
    inv = {}
    for i in range(int(p.n_points)):
        v = int(p.point_ref[i])
        if v not in inv:
            inv[v] = sim3_inverse(S.est[v])
        xw[i] = sim3_map(inv[v], sim3_map(S.scw[v], [float(x) for x in xw_in[i]]))
    return tcw, xw


def solve(p):
    S = Solver(p)
    tr = optimize(S)
    tcw, xw = finish(S)
    return SimpleNamespace(tcw=tcw, xw=xw, trace=tr, solver=S)
