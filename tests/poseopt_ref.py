"""Optimizer::PoseOptimization (src/Optimizer.cc:242-452 of the reference) restated in Python floats,
with numpy.float32 only where the reference narrows: the yardstick for orbfe_poseopt_core.h on the
host and for k_poseopt on the GPU, compared bit for bit.

One function per rule. A line marked EIGEN: restates an Eigen 3.4 operation from knowledge of that
library (its source is not available here); where its vectorised order depends on the build the plain
left-to-right scalar order is taken. A line marked DEVIATION: departs from the reference on purpose
(DESIGN.md section 18 lists them). No libm transcendental is used: sin and cos are restated from
+ - * / alone, so every platform that rounds those four (and sqrt) as IEEE 754 does gives these bits.

The sum over edges is fixed here, because g2o's own order (a std::set of pointers) is not defined:
edge i (the frame's keypoint index) belongs to lane i % PO_LANES, a lane adds its active edges in
ascending i from +0.0, and the lanes are combined by s[l] += s[l + stride], stride = 32 .. 1.
"""
import math
import struct
from types import SimpleNamespace

import numpy as np

from lm_ref import (DBL_MAX, DBL_MIN, FLAG_LARGE_STEP, FLAG_NONFINITE, NAN, PO_LANES, STOP_ALL, STOP_NBAD,  # noqa: F401
                    STOP_NO_EDGE, STOP_TERMINATE, div, finite, ldlt, ldlt_solve, levenberg, tree)

DELTA_MONO = float(np.float32(math.sqrt(5.991)))    # const float deltaMono = sqrt(5.991), setDelta widens
DELTA_STEREO = float(np.float32(math.sqrt(7.815)))
CHI2_MONO = np.float32(5.991)
CHI2_STEREO = np.float32(7.815)

# ---- sin / cos from + - * / ------------------------------------------------------------------------
PI = 3.141592653589793
INV_PIO2 = 6.36619772367581382433e-01
PIO2_1 = 1.57079632673412561417e+00   # pi/2 in three pieces of 33 bits, so that k * piece is exact
PIO2_2 = 6.07710050630396597660e-11   # for a small k, and what is left of it
PIO2_3 = 2.02226624871116645580e-21
PIO2_3T = 8.47842766036889956997e-32
TRIG_MAX = 2147483648.0
S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11


def kernel_sin(x, y):
    """sin(x + y) on [-pi/4, pi/4], y the tail of x: an odd polynomial of degree 13"""
    z = x * x
    w = z * z
    r = (S2 + z * (S3 + z * S4)) + (z * w) * (S5 + z * S6)
    v = z * x
    return x - ((z * (0.5 * y - v * r) - y) - v * S1)


def kernel_cos(x, y):
    """cos(x + y) on [-pi/4, pi/4]: 1 - z/2 + z^2 * (an even polynomial), the 1 - z/2 step compensated"""
    z = x * x
    w = z * z
    r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6))
    hz = 0.5 * z
    w = 1.0 - hz
    return w + (((1.0 - w) - hz) + (z * r - x * y))


def sincos(theta):
    """-> (sin, cos, flags). DEVIATION: replaces libm's sin / cos. Cody-Waite reduction by pi/2 with
    the constant split in pieces (each subtraction's rounding error is carried into a tail), then the
    kernels by quadrant. Defined for every finite theta; above pi it sets FLAG_LARGE_STEP, from 2^31
    on it returns (0, 1). A non-finite theta gives NaN."""
    if theta - theta != 0.0:
        return NAN, NAN, 0
    flags = FLAG_LARGE_STEP if theta > PI else 0
    if not (theta < TRIG_MAX and theta > -TRIG_MAX):
        return 0.0, 1.0, flags
    kk = int(theta * INV_PIO2 + 0.5)  # truncation, as a C conversion
    k = float(kk)
    r0 = theta - k * PIO2_1
    w1 = k * PIO2_2
    r1 = r0 - w1
    e1 = (r0 - r1) - w1
    w2 = k * PIO2_3
    r2 = r1 - w2
    e2 = (r1 - r2) - w2
    tail = (e1 + e2) - k * PIO2_3T
    r = r2 + tail
    y = (r2 - r) + tail
    s, c = kernel_sin(r, y), kernel_cos(r, y)
    q = kk & 3
    if q == 0:
        return s, c, flags
    if q == 1:
        return c, -s, flags
    if q == 2:
        return -s, -c, flags
    return -c, s, flags


# ---- Eigen's quaternion and 3x3 operations ---------------------------------------------------------
def quat_from_matrix(m):
    """EIGEN: Quaterniond(Matrix3d): the trace branch if the trace (m00 + m11 + m22) is > 0, else the
    branch of the largest diagonal entry (a later entry wins only if strictly greater).
    m: 9 row-major; -> [x, y, z, w]"""
    q = [0.0] * 4
    t = m[0] + m[4] + m[8]
    if t > 0.0:
        t = c_sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = div(0.5, t)
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = c_sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0)
        q[i] = 0.5 * t
        t = div(0.5, t)
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q


def c_sqrt(a):
    """IEEE sqrt: NaN below zero (math.sqrt raises there)"""
    if a != a or a < 0:
        return NAN
    if a == float("inf"):
        return a
    return math.sqrt(a)


def normalize_rotation(q):
    """SE3Quat::normalizeRotation: w < 0 flips every coefficient (times -1), then
    EIGEN: normalize() divides each coefficient by sqrt(((x^2 + y^2) + z^2) + w^2) when that sum is > 0"""
    if q[3] < 0:
        q = [c * -1.0 for c in q]
    z = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    if z > 0.0:
        nrm = c_sqrt(z)
        q = [c / nrm for c in q]
    return q


def cross(a, b):
    """EIGEN: cross(): (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)"""
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def quat_rotate(q, v):
    """EIGEN: Quaterniond * Vector3d: uv = qv x v; uv += uv; v + w * uv + qv x uv"""
    uv = cross(q, v)
    uv = [u + u for u in uv]
    c2 = cross(q, uv)
    return [(v[i] + q[3] * uv[i]) + c2[i] for i in range(3)]


def quat_mul(a, b):
    """EIGEN: the scalar quaternion product, term by term, left to right"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def quat_to_matrix(q):
    """EIGEN: toRotationMatrix()"""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def mat3_mul(a, b):
    """EIGEN: a 3x3 product sums k ascending"""
    return [(a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c] for r in range(3) for c in range(3)]


def mat3_vec(a, v):
    return [(a[3 * r] * v[0] + a[3 * r + 1] * v[1]) + a[3 * r + 2] * v[2] for r in range(3)]


# ---- SE3Quat: (q, t) -------------------------------------------------------------------------------
def se3_from_tcw(tcw):
    """Converter::toSE3Quat: float -> double, SE3Quat(R, t)"""
    m = [float(np.float32(tcw[4 * (i // 3) + i % 3])) for i in range(9)]
    t = [float(np.float32(tcw[4 * i + 3])) for i in range(3)]
    return normalize_rotation(quat_from_matrix(m)), t


def se3_exp(u):
    """SE3Quat::exp (se3quat.h). DEVIATION: sin / cos from sincos(); pow(theta, 3) is
    theta * theta * theta. -> (q, t, flags)"""
    om, up = u[0:3], u[3:6]
    theta = c_sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    O = [0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0]
    O2 = mat3_mul(O, O)
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    flags = 0
    if theta < 0.00001:
        R = [(I[i] + O[i]) + O2[i] for i in range(9)]
        V = R
    else:
        s, c, flags = sincos(theta)
        a = s / theta
        b = (1.0 - c) / (theta * theta)
        d = (theta - s) / (theta * theta * theta)
        R = [(I[i] + a * O[i]) + b * O2[i] for i in range(9)]
        V = [(I[i] + b * O[i]) + d * O2[i] for i in range(9)]
    return normalize_rotation(quat_from_matrix(R)), mat3_vec(V, up), flags


def se3_mul(a, b):
    """SE3Quat::operator*: t = a.t + a.q * b.t; q = a.q * b.q; normalizeRotation"""
    r = quat_rotate(a[0], b[1])
    return normalize_rotation(quat_mul(a[0], b[0])), [a[1][i] + r[i] for i in range(3)]


def se3_map(T, X):
    r = quat_rotate(T[0], X)
    return [r[i] + T[1][i] for i in range(3)]


def se3_to_tcw(T):
    """to_homogeneous_matrix narrowed by Converter::toCvMat -> 12 float32"""
    R = quat_to_matrix(T[0])
    return np.array([R[0], R[1], R[2], T[1][0], R[3], R[4], R[5], T[1][1], R[6], R[7], R[8], T[1][2]], np.float32)


# ---- one edge --------------------------------------------------------------------------------------
class Edge:
    """One correspondence: Xw, obs, the camera and invSigma2 as the doubles the reference widens to."""

    def __init__(self, xw, kp, ur, inv_sigma2, k, bf):
        self.X = [float(np.float32(v)) for v in xw]
        self.stereo = not (np.float32(ur) < 0)  # mvuRight[i] < 0: monocular
        self.obs = [float(np.float32(kp[0])), float(np.float32(kp[1]))] + ([float(np.float32(ur))] if self.stereo else [])
        self.w = float(np.float32(inv_sigma2))
        self.fx, self.fy, self.cx, self.cy = [float(np.float32(v)) for v in k]
        self.bf = float(np.float32(bf))
        self.delta = DELTA_STEREO if self.stereo else DELTA_MONO
        self.dsqr = self.delta * self.delta


def edge_error(e, T):
    """computeError of the two *OnlyPose edges: obs - cam_project(T.map(Xw))"""
    p = se3_map(T, e.X)
    if e.stereo:
        invz = float(np.float32(div(1.0, p[2])))  # const float invz = 1.0f / z: divided in double, narrowed
        r0 = p[0] * invz * e.fx + e.cx
        r1 = p[1] * invz * e.fy + e.cy
        r2 = r0 - e.bf * invz
        return [e.obs[0] - r0, e.obs[1] - r1, e.obs[2] - r2]
    r0 = div(p[0], p[2]) * e.fx + e.cx  # project2d divides in double
    r1 = div(p[1], p[2]) * e.fy + e.cy
    return [e.obs[0] - r0, e.obs[1] - r1]


def edge_chi2(e, err):
    """EIGEN: _error.dot(information() * _error) with a diagonal information: sum_k e_k * (w * e_k)"""
    s = err[0] * (e.w * err[0]) + err[1] * (e.w * err[1])
    if e.stereo:
        s = s + err[2] * (e.w * err[2])
    return s


def huber(chi2, delta, dsqr):
    """RobustKernelHuber::robustify -> rho[0], rho[1]"""
    if chi2 <= dsqr:
        return chi2, 1.0
    sq = c_sqrt(chi2)
    return 2 * sq * delta - dsqr, div(delta, sq)


def edge_jacobian(e, T):
    """linearizeOplus of the two *OnlyPose edges -> rows of 6"""
    p = se3_map(T, e.X)
    x, y = p[0], p[1]
    invz = div(1.0, p[2])
    invz_2 = invz * invz
    fx, fy = e.fx, e.fy
    J = [[x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, 0.0, x * invz_2 * fx],
         [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, 0.0, -invz * fy, y * invz_2 * fy]]
    if e.stereo:
        bf = e.bf
        J.append([J[0][0] - bf * y * invz_2, J[0][1] + bf * x * invz_2, J[0][2], J[0][3], 0.0, J[0][5] - bf * invz_2])
    return J


H_IDX = [[r * (r + 1) // 2 + c if c <= r else -1 for c in range(6)] for r in range(6)]
ACC = 28  # 21 lower entries of H (row-major over r >= c), 6 of b, the robust chi2


def edge_accumulate(acc, e, T, kernel_on, full):
    """computeError + activeRobustChi2's term and, with `full`, linearizeOplus + constructQuadraticForm
    of one active edge into a lane's accumulators.
    EIGEN: b_r -= sum_k ((rho1 * A_kr) * w) * e_k (without a kernel: (A_kr * w) * e_k);
           H_rc += sum_k (A_kr * (rho1 * w)) * A_kc (without: A_kr * w), lower triangle only."""
    err = edge_error(e, T)
    chi2 = edge_chi2(e, err)
    rho0, rho1 = huber(chi2, e.delta, e.dsqr) if kernel_on else (chi2, 1.0)
    acc[27] = acc[27] + rho0
    if not full:
        return
    J = edge_jacobian(e, T)
    D = len(J)
    ww = rho1 * e.w if kernel_on else e.w
    for r in range(6):
        if kernel_on:
            s = ((rho1 * J[0][r]) * e.w) * err[0]
            for k in range(1, D):
                s = s + ((rho1 * J[k][r]) * e.w) * err[k]
        else:
            s = (J[0][r] * e.w) * err[0]
            for k in range(1, D):
                s = s + (J[k][r] * e.w) * err[k]
        acc[21 + r] = acc[21 + r] - s
        for c in range(r + 1):
            s = (J[0][r] * ww) * J[0][c]
            for k in range(1, D):
                s = s + (J[k][r] * ww) * J[k][c]
            acc[H_IDX[r][c]] = acc[H_IDX[r][c]] + s


def sums(edges, active, T, kernel_on, full):
    """edges: {i: Edge}; active: ascending keypoint indices -> the 28 sums"""
    lanes = [[0.0] * ACC for _ in range(PO_LANES)]
    for i in active:
        edge_accumulate(lanes[i % PO_LANES], edges[i], T, kernel_on, full)
    return tree(lanes)


# ---- the 6x6 solve (lm_ref.ldlt / ldlt_solve) ------------------------------------------------------
def solve_step(S, lam, x_prev):
    """setLambda + LinearSolverDense::solve on the sums S -> (ok2, x, flags).
    DEVIATION: a non-finite entry of H + lambda I or b gives ok2 = false (FLAG_NONFINITE) without a
    factorisation; x keeps its previous value whenever ok2 is false."""
    A = [[0.0] * 6 for _ in range(6)]
    ok = True
    for r in range(6):
        for c in range(r + 1):
            A[r][c] = S[H_IDX[r][c]] + lam if r == c else S[H_IDX[r][c]]
            ok = ok and finite(A[r][c])
        ok = ok and finite(S[21 + r])
    if not ok:
        return False, x_prev, FLAG_NONFINITE
    tr, positive = ldlt(A)
    if not positive:
        return False, x_prev, 0
    return True, ldlt_solve(A, tr, S[21:27]), 0


# ---- the optimisation ------------------------------------------------------------------------------
class Round:
    def __init__(self):
        self.n_active = self.iterations = self.trials = self.rejected_trials = self.stop = self.n_bad = 0
        self.lam = self.chi2 = 0.0
        self.last_rejected = False  # the round's last evaluated trial was rejected (not part of the C trace)

    def key(self):
        return (self.n_active, self.iterations, self.trials, self.rejected_trials, self.stop, self.n_bad,
                bits64(self.lam), bits64(self.chi2))


def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def classify(e, T_final, T_eval, was_outlier):
    """The classification of one edge after a round: an edge flagged before is recomputed at the final
    estimate, an active one keeps the error of the last evaluated trial (accepted or not); chi2 is
    narrowed to float and compared with >, so a NaN is an inlier. -> outlier"""
    err = edge_error(e, T_final if was_outlier else T_eval)
    chi2 = np.float32(edge_chi2(e, err))
    return bool(chi2 > (CHI2_STEREO if e.stereo else CHI2_MONO))


class Result:
    pass


def optimize(n, valid, xw, kp_un, u_right, inv_sigma2, k, bf, tcw):
    """PoseOptimization over a frame's n keypoints -> Result"""
    tcw = np.asarray(tcw, np.float32).reshape(12)
    edges = {i: Edge(xw[i], kp_un[i], u_right[i], inv_sigma2[i], k, bf) for i in range(n) if valid[i]}
    idx = sorted(edges)
    T0 = se3_from_tcw(tcw)
    res = Result()
    res.n_initial = len(idx)
    res.outlier = np.zeros(n, bool)
    res.rounds = [Round() for _ in range(4)]
    res.rounds_run = 0
    res.flags = 0
    res.n_bad = 0
    est = T0
    if len(idx) < 3:
        res.n_inliers = 0
        res.stale = 0
        res.tcw = tcw.copy()
        res.pose = list(T0[0]) + list(T0[1])
        return res
    for it in range(4):
        est = T0  # every round restarts from the frame's pose
        kernel_on = it < 3
        active = [i for i in idx if not res.outlier[i]]
        T_eval = est
        R = res.rounds[it]
        R.n_active = len(active)
        if not active:
            R.stop = STOP_NO_EDGE
        else:
            # DEVIATION: x is zero before a round's first successful solve
            st = SimpleNamespace(x=[0.0] * 6, S=None, trial=None)

            def linearize():
                st.S = sums(edges, active, est, kernel_on, True)
                mx = 0.0
                for j in range(6):
                    a = abs(st.S[H_IDX[j][j]])
                    mx = mx if a < mx else a  # std::max(fabs(H_jj), maxDiagonal)
                return st.S[27], mx

            def trial(lam):
                nonlocal T_eval
                ok2, st.x, fl = solve_step(st.S, lam, st.x)
                res.flags |= fl
                dq, dt, fl = se3_exp(st.x)
                res.flags |= fl
                st.trial = T_eval = se3_mul((dq, dt), est)
                temp = sums(edges, active, st.trial, kernel_on, False)[27]
                scale = 0.0
                for j in range(6):
                    scale = scale + st.x[j] * (lam * st.x[j] + st.S[21 + j])
                return temp, scale, not ok2

            def accept():
                nonlocal est
                est = st.trial

            t = levenberg(linearize, trial, accept, 10)
            R.iterations, R.trials, R.rejected_trials, R.stop = t.iterations, t.trials, t.rejected_trials, t.stop
            R.lam, R.chi2, R.last_rejected = t.lam, t.chi2, t.last_rejected
        for i in idx:
            res.outlier[i] = classify(edges[i], est, T_eval, bool(res.outlier[i]))
        R.outlier = res.outlier.copy()
        R.n_bad = int(res.outlier.sum())
        res.n_bad = R.n_bad
        res.rounds_run = it + 1
        if len(idx) < 10:
            break
    res.n_inliers = res.n_initial - res.n_bad
    # edges whose flag would differ had the last round classified them at the final estimate
    res.stale = sum(1 for i in idx if classify(edges[i], est, est, True) != bool(res.outlier[i]))
    res.tcw = se3_to_tcw(est)
    res.pose = list(est[0]) + list(est[1])
    return res


def optimize_problem(p):
    """p: a poseopt_scenes.Problem (or anything with its fields)"""
    return optimize(p.n, p.valid, p.xw, p.kp_un, p.u_right, p.inv_sigma2, p.k, p.bf, p.tcw)
