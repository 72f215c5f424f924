"""Optimizer::OptimizeSim3 (src/Optimizer.cc:1050-1250 of the reference) restated in Python floats, with
numpy.float32 only where the reference narrows: the yardstick for orbfe_optsim3_core.h on the host and
for k_optsim3 on the GPU, compared bit for bit.

One function per rule, the same code as the core header. The quaternion rules, sin / cos, IEEE division
and sqrt, the lane tree and the Levenberg driver's conventions are those of tests/poseopt_ref.py
 and are imported from it; what is new is Sim3 (sim3.h), exp from + - * /, the
numeric Jacobians of BaseBinaryEdge::linearizeOplus, the binary edge's constructQuadraticForm and the
7x7 LDLT. EIGEN: and DEVIATION: mark lines as they do there.

The sum over edges is fixed: correspondence i (KF1's keypoint index) belongs to lane i % 64, a lane adds
e12 then e21 of its active correspondences in ascending i from +0.0, and the lanes are combined by
s[l] += s[l + stride], stride = 32 .. 1.
"""
from types import SimpleNamespace

import numpy as np

from lm_ref import (DBL_MAX, DBL_MIN, FLAG_LARGE_STEP, FLAG_NONFINITE, NAN, PO_LANES, STOP_ALL, STOP_NBAD,  # noqa: F401
                    STOP_NO_EDGE, STOP_TERMINATE, div, finite, ldlt, ldlt_solve, levenberg, tree)
from poseopt_ref import (Round, bits64, c_sqrt, mat3_mul, quat_from_matrix, quat_mul, quat_rotate,  # noqa: F401
                         quat_to_matrix, sincos)

ACC = 36  # 28 lower entries of H (row-major over r >= c), 7 of b, the robust chi2
H_IDX = [[r * (r + 1) // 2 + c if c <= r else -1 for c in range(7)] for r in range(7)]
DELTA = 1e-9  # BaseBinaryEdge::linearizeOplus
SCALAR = 1.0 / (2 * DELTA)

# ---- exp from + - * / ------------------------------------------------------------------------------
INV_LN2 = 1.44269504088896338700e+00
LN2_HI = 6.93147180369123816490e-01  # the low 32 bits are zero: k * LN2_HI is exact for |k| < 2^11
LN2_LO = 1.90821492927058770002e-10
P1, P2, P3 = 1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05
P4, P5 = -1.65339022054652515390e-06, 4.13813679705723846039e-08
TWO_512, TWO_M512 = 1.3407807929942597e+154, 7.458340731200207e-155


def exp(x):
    """DEVIATION: replaces std::exp. Cody-Waite reduction by ln 2, the rational form of fdlibm's
    e_exp.c on the reduced argument, then k exact doublings or halvings."""
    if x != x:
        return x
    if x > 709.782712893384:
        return DBL_MAX * 2.0  # +inf
    if x < -745.2:
        return 0.0
    kk = int(x * INV_LN2 + (-0.5 if x < 0 else 0.5))  # truncation, as a C conversion
    k = float(kk)
    hi = x - k * LN2_HI
    lo = k * LN2_LO
    r = hi - lo
    t = r * r
    c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
    y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
    neg = kk < 0
    a = -kk if neg else kk
    p = 0.5 if neg else 2.0
    for j in range(11):
        if j < 10:
            if (a >> j) & 1:
                y = y * p
            p = p * p
        elif (a >> j) & 1:
            h = TWO_M512 if neg else TWO_512
            y = y * h
            y = y * h
    return y


# ---- Sim3: (q, t, s) -------------------------------------------------------------------------------
def sim3_from_update(u):
    """Sim3(const Vector7d&) (sim3.h:70-142) -> ((q, t, s), flags). EIGEN: norm() is
    sqrt((x^2 + y^2) + z^2); a sum of three matrices is taken left to right per entry."""
    om, up, sigma = u[0:3], u[3:6], u[6]
    theta = c_sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    O = [0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0]
    O2 = mat3_mul(O, O)
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    s = exp(sigma)
    eps = 0.00001
    small_theta = theta < eps
    flags = 0
    sn, cs = 0.0, 1.0
    if not small_theta:
        sn, cs, flags = sincos(theta)
    if abs(sigma) < eps:
        C = 1.0
        if small_theta:
            A = 1. / 2.
            B = 1. / 6.
        else:
            theta2 = theta * theta
            A = div(1 - cs, theta2)
            B = div(theta - sn, theta2 * theta)
    else:
        C = div(s - 1, sigma)
        if small_theta:
            sigma2 = sigma * sigma
            A = div((sigma - 1) * s + 1, sigma2)
            B = div((0.5 * sigma2 - sigma + 1) * s, sigma2 * sigma)
        else:
            a = s * sn
            b = s * cs
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = div(a * sigma + (1 - b) * theta, theta * c)
            B = div((C - div((b - 1) * sigma + a * theta, c)) * 1., theta2)
    if small_theta:
        R = [(I[i] + O[i]) + O2[i] for i in range(9)]
    else:
        ra = div(sn, theta)
        rb = div(1 - cs, theta * theta)
        R = [(I[i] + ra * O[i]) + rb * O2[i] for i in range(9)]
    q = quat_from_matrix(R)  # r = Quaterniond(R): no normalisation
    W = [(A * O[i] + B * O2[i]) + C * I[i] for i in range(9)]
    t = [(W[3 * r] * up[0] + W[3 * r + 1] * up[1]) + W[3 * r + 2] * up[2] for r in range(3)]
    return (q, t, s), flags


def sim3_mul(a, b):
    """Sim3::operator*: r = a.r * b.r; t = a.s * (a.r * b.t) + a.t; s = a.s * b.s"""
    r = quat_rotate(a[0], b[1])
    return quat_mul(a[0], b[0]), [a[2] * r[i] + a[1][i] for i in range(3)], a[2] * b[2]


def sim3_inverse(a):
    """Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)"""
    q = [-a[0][0], -a[0][1], -a[0][2], a[0][3]]
    c = div(-1., a[2])
    return q, quat_rotate(q, [c * a[1][0], c * a[1][1], c * a[1][2]]), div(1., a[2])


def sim3_map(S, X):
    """s * (r * xyz) + t"""
    r = quat_rotate(S[0], X)
    return [S[2] * r[i] + S[1][i] for i in range(3)]


def sim3_from_floats(r9, t3, s):
    """Sim3(toMatrix3d(R), toVector3d(t), s): r = Quaterniond(R) of the widened floats"""
    return (quat_from_matrix([float(np.float32(v)) for v in r9]), [float(np.float32(v)) for v in t3], s)


def oplus(u, fix_scale, est):
    """VertexSim3Expmap::oplusImpl: update[6] = 0 in place with _fix_scale -> (estimate, flags)"""
    if fix_scale:
        u[6] = 0.0
    d, flags = sim3_from_update(u)
    return sim3_mul(d, est), flags


def sim3_to_rt(S):
    """Converter::toCvMat(g2o::Sim3): float(s * R | t) -> 12 float32"""
    R = quat_to_matrix(S[0])
    sR = [S[2] * v for v in R]
    return np.array([sR[0], sR[1], sR[2], S[1][0], sR[3], sR[4], sR[5], S[1][1], sR[6], sR[7], sR[8], S[1][2]],
                    np.float32)


def flat(S):
    return list(S[0]) + list(S[1]) + [S[2]]


# ---- one edge --------------------------------------------------------------------------------------
class Edge:
    """One of the two edges of a correspondence: the fixed point, the observation, invSigma2 and the
    camera as the doubles the reference widens to. inverse: EdgeInverseSim3ProjectXYZ (e21)."""

    def __init__(self, X, obs, inv_sigma2, cam, inverse):
        self.X = [float(np.float32(v)) for v in X]
        self.obs = [float(np.float32(obs[0])), float(np.float32(obs[1]))]
        self.w = float(np.float32(inv_sigma2))
        self.cam = [float(np.float32(v)) for v in cam]  # fx fy cx cy
        self.inverse = inverse


def edge_error(e, S):
    """computeError at the state S (the estimate for e12, its inverse for e21):
    obs - cam_map(project(S.map(X)))"""
    p = sim3_map(S, e.X)
    return [e.obs[0] - (div(p[0], p[2]) * e.cam[0] + e.cam[2]), e.obs[1] - (div(p[1], p[2]) * e.cam[1] + e.cam[3])]


def edge_chi2(e, err):
    """EIGEN: _error.dot(information() * _error) with a diagonal information"""
    return err[0] * (e.w * err[0]) + err[1] * (e.w * err[1])


def huber_delta(th2):
    """const float deltaHuber = sqrt(th2); setDelta widens"""
    return float(np.float32(c_sqrt(th2)))


def huber(chi2, delta, dsqr):
    """RobustKernelHuber::robustify -> rho[0], rho[1]"""
    if chi2 <= dsqr:
        return chi2, 1.0
    sq = c_sqrt(chi2)
    return 2 * sq * delta - dsqr, div(delta, sq)


def build_table(est, fix_scale):
    """The 15 states of one linearisation, each with its inverse: the estimate, then oplus(+delta e_d),
    oplus(-delta e_d) for d = 0 .. 6. They do not depend on the edge."""
    tab = [(est, sim3_inverse(est))]
    for d in range(7):
        for sign in (DELTA, -DELTA):
            u = [0.0] * 7
            u[d] = sign
            S, _ = oplus(u, fix_scale, est)
            tab.append((S, sim3_inverse(S)))
    return tab


def numeric_jacobian(e, tab):
    """BaseBinaryEdge::linearizeOplus for the Sim3 vertex: column d = (1 / (2 delta)) * (e(+d) - e(-d))
    -> 2 rows of 7"""
    side = 1 if e.inverse else 0
    J = [[0.0] * 7, [0.0] * 7]
    for d in range(7):
        ep = edge_error(e, tab[1 + 2 * d][side])
        em = edge_error(e, tab[2 + 2 * d][side])
        J[0][d] = SCALAR * (ep[0] - em[0])
        J[1][d] = SCALAR * (ep[1] - em[1])
    return J


def edge_accumulate(acc, e, tab, delta, dsqr):
    """computeError, linearizeOplus and the robust constructQuadraticForm of one edge.
    EIGEN: omega_r = -(w * e_k), omega_r *= rho1; b_r += B_0r * omega_r0 + B_1r * omega_r1;
           H_rc += (B_0r * (rho1 * w)) * B_0c + (B_1r * (rho1 * w)) * B_1c, lower triangle only."""
    err = edge_error(e, tab[0][1 if e.inverse else 0])
    rho0, rho1 = huber(edge_chi2(e, err), delta, dsqr)
    acc[35] = acc[35] + rho0
    J = numeric_jacobian(e, tab)
    or0, or1 = -(e.w * err[0]) * rho1, -(e.w * err[1]) * rho1
    ww = rho1 * e.w
    for r in range(7):
        acc[28 + r] = acc[28 + r] + (J[0][r] * or0 + J[1][r] * or1)
        for c in range(r + 1):
            acc[H_IDX[r][c]] = acc[H_IDX[r][c]] + ((J[0][r] * ww) * J[0][c] + (J[1][r] * ww) * J[1][c])


def sums_full(pairs, active, tab, delta, dsqr):
    """pairs: {i: (e12, e21)}; active: ascending KF1 indices -> the 36 sums"""
    lanes = [[0.0] * ACC for _ in range(PO_LANES)]
    for i in active:
        edge_accumulate(lanes[i % PO_LANES], pairs[i][0], tab, delta, dsqr)
        edge_accumulate(lanes[i % PO_LANES], pairs[i][1], tab, delta, dsqr)
    return tree(lanes)


def sums_chi(pairs, active, S, Si, delta, dsqr):
    """activeRobustChi2 at the state S and its inverse Si"""
    lanes = [[0.0] for _ in range(PO_LANES)]
    for i in active:
        for e, T in ((pairs[i][0], S), (pairs[i][1], Si)):
            rho0, _ = huber(edge_chi2(e, edge_error(e, T)), delta, dsqr)
            lanes[i % PO_LANES][0] = lanes[i % PO_LANES][0] + rho0
    return tree(lanes)[0]


# ---- the 7x7 solve (lm_ref.ldlt / ldlt_solve) ------------------------------------------------------
def system_of(S, lam):
    """H + lambda I (lower triangle) and b of the sums S"""
    A = [[0.0] * 7 for _ in range(7)]
    for r in range(7):
        for c in range(r + 1):
            A[r][c] = S[H_IDX[r][c]] + lam if r == c else S[H_IDX[r][c]]
    return A, list(S[28:35])


def solve_step(S, lam, x_prev):
    """setLambda + LinearSolverDense::solve on the sums S -> (ok2, x, flags).
    DEVIATION: a non-finite entry of H + lambda I or b gives ok2 = false (FLAG_NONFINITE) without a
    factorisation; x keeps its previous value whenever ok2 is false."""
    A, b = system_of(S, lam)
    ok = finite(lam) and all(finite(v) for v in S[0:35]) and all(finite(A[j][j]) for j in range(7))
    if not ok:
        return False, x_prev, FLAG_NONFINITE
    tr, positive = ldlt(A)
    if not positive:
        return False, x_prev, 0
    return True, ldlt_solve(A, tr, b), 0


# ---- the optimisation ------------------------------------------------------------------------------
def classify(pair, S, Si, th2):
    """:1202, :1236: e12->chi2() > th2 || e21->chi2() > th2, unrobustified doubles against the widened
    float; a NaN chi2 keeps the correspondence"""
    c12 = edge_chi2(pair[0], edge_error(pair[0], S))
    c21 = edge_chi2(pair[1], edge_error(pair[1], Si))
    return bool(c12 > th2 or c21 > th2)


_classify_at = classify  # for Result.stale: not the classification step itself


class Result:
    pass


def optimize(p, hook=None):
    """OptimizeSim3 over a problem (optsim3_scenes.Problem, or anything with its fields) -> Result.
    hook(round, iteration, S, lam), if given, sees every linearisation's sums."""
    n = int(p.n)
    th2 = float(np.float32(p.th2))
    fix_scale = bool(p.fix_scale)
    delta = huber_delta(th2)
    dsqr = delta * delta
    pairs = {i: (Edge(p.p3d2c[i], p.kp_un1[i], p.inv_sigma2_1[i], p.k1, False),
                 Edge(p.p3d1c[i], p.kp_un2[i], p.inv_sigma2_2[i], p.k2, True)) for i in range(n) if p.valid[i]}
    idx = sorted(pairs)
    start = sim3_from_floats(np.asarray(p.r12).reshape(9), np.asarray(p.t12).reshape(3), float(np.float32(p.s12)))
    res = Result()
    res.n_correspondences = len(idx)
    res.removed = np.zeros(n, bool)
    res.rounds = [Round() for _ in range(2)]
    res.rounds_run = 0
    res.flags = 0
    res.n_bad = 0
    est = start
    T_eval = est
    for it in range(2):
        if it == 1 and res.n_correspondences - res.n_bad < 10:
            break  # :1220: return 0, g2oS12 untouched
        max_iter = 5 if it == 0 else (10 if res.n_bad > 0 else 5)
        active = [i for i in idx if not res.removed[i]]
        R = res.rounds[it]
        R.n_active = len(active)
        if not active:
            R.stop = STOP_NO_EDGE
        else:
            # DEVIATION: x is zero before a round's first successful solve
            st = SimpleNamespace(x=[0.0] * 7, S=None, trial=None)

            def linearize():
                st.S = sums_full(pairs, active, build_table(est, fix_scale), delta, dsqr)
                mx = 0.0
                for j in range(7):
                    a = abs(st.S[H_IDX[j][j]])
                    mx = mx if a < mx else a  # std::max(fabs(H_jj), maxDiagonal)
                return st.S[35], mx

            def trial(lam):
                nonlocal T_eval
                ok2, x, fl = solve_step(st.S, lam, st.x)
                res.flags |= fl
                st.x = list(x)
                st.trial, fl = oplus(st.x, fix_scale, est)  # zeroes x[6] with fix_scale: computeScale reads it so
                res.flags |= fl
                T_eval = st.trial
                temp = sums_chi(pairs, active, st.trial, sim3_inverse(st.trial), delta, dsqr)
                scale = 0.0
                for j in range(7):
                    scale = scale + st.x[j] * (lam * st.x[j] + st.S[28 + j])
                return temp, scale, not ok2

            def accept():
                nonlocal est
                est = st.trial

            t = levenberg(linearize, trial, accept, max_iter,
                          on_lambda=(lambda i, lam: hook(it, i, st.S, lam)) if hook else None)
            R.iterations, R.trials, R.rejected_trials, R.stop = t.iterations, t.trials, t.rejected_trials, t.stop
            R.lam, R.chi2, R.last_rejected = t.lam, t.chi2, t.last_rejected
        T_inv = sim3_inverse(T_eval)
        for i in active:
            res.removed[i] = classify(pairs[i], T_eval, T_inv, th2)
        R.removed = res.removed.copy()
        R.n_bad = res.n_bad = int(res.removed.sum())
        res.rounds_run = it + 1
    out = est if res.rounds_run == 2 else start
    res.n_inliers = res.n_correspondences - res.n_bad if res.rounds_run == 2 else 0
    # correspondences whose flag would differ had the last round classified them at the final estimate
    res.stale = 0
    if res.rounds_run:
        last = res.rounds[res.rounds_run - 1]
        before = res.rounds[0].removed if res.rounds_run == 2 else np.zeros(n, bool)
        fin = (est, sim3_inverse(est))
        res.stale = sum(1 for i in idx if not before[i] and _classify_at(pairs[i], fin[0], fin[1], th2) != bool(last.removed[i]))
    res.sim3 = flat(out)
    res.s12_rt = sim3_to_rt(out)
    res.scw = np.zeros(12, np.float32)
    if getattr(p, "r2w", None) is not None:
        smw = sim3_from_floats(np.asarray(p.r2w).reshape(9), np.asarray(p.t2w).reshape(3), 1.0)
        res.scw = sim3_to_rt(sim3_mul(out, smw))
    return res


# ---- the stand-alone host program's text format (tests/cpp/optsim3_core_main.cpp) -------------------
def bits32(x):
    import struct
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def write_problems(path, problems):
    lines = [str(len(problems))]
    for p in problems:
        has_kf2 = getattr(p, "r2w", None) is not None
        head = list(p.k1) + list(p.k2) + list(np.asarray(p.r12).reshape(9)) + list(p.t12) + [p.s12, p.th2]
        head += (list(np.asarray(p.r2w).reshape(9)) + list(p.t2w)) if has_kf2 else [0.0] * 12
        lines.append("%d %d %d %s" % (p.n, int(p.fix_scale), int(has_kf2), " ".join(bits32(v) for v in head)))
        for i in range(p.n):
            vals = (list(p.p3d1c[i]) + list(p.p3d2c[i]) + list(p.kp_un1[i]) + list(p.kp_un2[i])
                    + [p.inv_sigma2_1[i], p.inv_sigma2_2[i]])
            lines.append("%d %s" % (p.valid[i], " ".join(bits32(v) for v in vals)))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def expected_row(p, r):
    """the host program's output line for problem p with the restatement's result r"""
    f = ["%d %d %d %d %d" % (r.n_correspondences, r.n_bad, r.n_inliers, r.rounds_run, r.flags)]
    f += ["%016x" % bits64(v) for v in r.sim3]
    f += [bits32(v) for v in r.s12_rt]
    f += [bits32(v) for v in r.scw]
    words = np.packbits(np.concatenate([r.removed, np.zeros(-p.n % 64, bool)]), bitorder="little").view("<u8")
    f += ["%016x" % int(w) for w in words]
    for rd in r.rounds:
        f.append("%d %d %d %d %d %d %016x %016x" % rd.key())
    return " ".join(f)
