"""The reference's Sim3Solver restated in plain Python / numpy -- the yardstick of the GPU
Sim3Solver tests. It shares no code with the product.

Restates src/Sim3Solver.cc:113-420 of the reference:
  :113-137   SetRansacParameters
  :139-212   iterate / find (the swap-remove sample selection, the acceptance rules)
  :214-336   ComputeCentroid / ComputeSim3 (Horn 1987)
  :338-420   CheckInliers / Project / FromCameraToImage
Every `float` of the reference is a numpy.float32 and every operation on it is rounded separately;
every `double` is a Python float (numpy.float64 in the vectorised inlier check).

The OpenCV calls inside ComputeSim3 are restated from a reading of OpenCV 3.x/4.x that could not be
checked against an OpenCV build. Each such rule is one line marked `# OPENCV:` so that it can be
corrected in one place.

The caller supplies the raw draws DUtils::Random::RandomInt would have returned (three per
iteration), so the generator stays outside.
"""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
FLT_EPSILON = F32(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
INT_MIN = -(1 << 31)


# ---- SetRansacParameters (:113-137) ---------------------------------------------------------------
def ransac_max_its(n, min_inliers, max_iterations, probability):
    """mRansacMaxIts after SetRansacParameters. A quotient that does not fit an int converts as
    x86's cvttsd2si does (INT_MIN), which max(1, min(...)) turns into 1."""
    epsilon = F32(min_inliers) / F32(n)
    if min_inliers == n:
        n_it = 1
    else:
        try:
            with np.errstate(all="ignore"):
                num = float(np.log(F64(1.0 - probability)))
                den = float(np.log(F64(1.0 - math.pow(float(epsilon), 3))))
                q = float(np.ceil(np.divide(F64(num), F64(den))))
        except (ValueError, OverflowError):  # pragma: no cover
            q = float("nan")
        n_it = int(q) if (q == q and -2147483649.0 < q < 2147483648.0) else INT_MIN
    return max(1, min(n_it, max_iterations))


def max_error(sigma2):
    """mvnMaxError entry: std::vector<size_t>::push_back(9.210 * sigmaSquare) truncates."""
    return int(9.210 * float(F32(sigma2)))


# ---- sample selection (:162-176) -------------------------------------------------------------------
def select3(n, draws):
    """The three correspondence indices of one iteration: swap-remove on a fresh 0..n-1 list."""
    avail = list(range(n))
    out = []
    for i in range(3):
        r = int(draws[i])
        assert 0 <= r <= len(avail) - 1, "draw outside RandomInt(0, size - 1)"
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


# ---- cv::Mat algebra --------------------------------------------------------------------------------
def gemm(A, B, alpha=None, C=None):
    """OPENCV: CV_32F gemm alpha*A*B (+ C): each element accumulates its products in double, left
    to right, alpha is applied in double, C is added in double, one rounding to float."""
    m, kk = A.shape
    n = B.shape[1]
    out = np.zeros((m, n), F32)
    with np.errstate(all="ignore"):
        for i in range(m):
            for j in range(n):
                s = F64(A[i, 0]) * F64(B[0, j])
                for k in range(1, kk):
                    s = s + F64(A[i, k]) * F64(B[k, j])
                if alpha is not None:
                    s = F64(alpha) * s
                if C is not None:
                    s = s + F64(C[i, j])
                out[i, j] = F32(s)
    return out


def hypot32(a, b):
    # OPENCV: std::hypot(float, float) as sqrt of the double sum of squares, narrowed once
    with np.errstate(all="ignore"):
        return F32(np.sqrt(F64(a) * F64(a) + F64(b) * F64(b)))


def jacobi4(N):
    """OPENCV: cv::eigen on a symmetric 4x4 CV_32F: JacobiImpl_<float> (max-pivot indices indR /
    indC, at most n*n*30 rotations, stop at |p| <= FLT_EPSILON), eigenvalues sorted descending,
    eigenvectors as rows, signs as the rotations leave them. -> (W[4], V[4][4], rotations)"""
    n = 4
    A = [[F32(N[i, j]) for j in range(n)] for i in range(n)]
    V = [[F32(1.0) if i == j else F32(0.0) for j in range(n)] for i in range(n)]
    W = [A[k][k] for k in range(n)]
    indR = [0] * n
    indC = [0] * n

    def row_max(k):
        m = k + 1
        mv = abs(A[k][m])
        for i in range(k + 2, n):
            val = abs(A[k][i])
            if mv < val:
                mv, m = val, i
        return m

    def col_max(k):
        m = 0
        mv = abs(A[0][k])
        for i in range(1, k):
            val = abs(A[i][k])
            if mv < val:
                mv, m = val, i
        return m

    for k in range(n):
        if k < n - 1:
            indR[k] = row_max(k)
        if k > 0:
            indC[k] = col_max(k)
    iters = 0
    with np.errstate(all="ignore"):
        for iters in range(n * n * 30):
            k = 0
            mv = abs(A[0][indR[0]])
            for i in range(1, n - 1):
                val = abs(A[i][indR[i]])
                if mv < val:
                    mv, k = val, i
            l = indR[k]
            for i in range(1, n):
                val = abs(A[indC[i]][i])
                if mv < val:
                    mv, k, l = val, indC[i], i
            p = A[k][l]
            if abs(p) <= FLT_EPSILON:
                break
            y = F32((W[l] - W[k]) * F32(0.5))
            t = abs(y) + hypot32(p, y)
            s = hypot32(p, t)
            c = t / s
            s = p / s
            t = (p / t) * p
            if y < 0:
                s, t = -s, -t
            A[k][l] = F32(0.0)
            W[k] = W[k] - t
            W[l] = W[l] + t

            def rot(a0, b0):
                return a0 * c - b0 * s, a0 * s + b0 * c

            for i in range(0, k):
                A[i][k], A[i][l] = rot(A[i][k], A[i][l])
            for i in range(k + 1, l):
                A[k][i], A[i][l] = rot(A[k][i], A[i][l])
            for i in range(l + 1, n):
                A[k][i], A[l][i] = rot(A[k][i], A[l][i])
            for i in range(n):
                V[k][i], V[l][i] = rot(V[k][i], V[l][i])
            for idx in (k, l):
                if idx < n - 1:
                    indR[idx] = row_max(idx)
                if idx > 0:
                    indC[idx] = col_max(idx)
        else:
            iters = n * n * 30
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return np.array(W, F32), np.array(V, F32), iters


def centroid(P):
    """ComputeCentroid (:214-223): -> (Pr, C)."""
    with np.errstate(all="ignore"):
        C = (P[:, 0] + P[:, 1]) + P[:, 2]  # OPENCV: cv::reduce(SUM) of a CV_32F row: float, left to right
        C = C * F32(1.0 / 3)               # OPENCV: C / P.cols multiplies by (float)(1.0 / 3)
        Pr = (P - C[:, None]).astype(F32)
    return Pr, C.astype(F32)


def rodrigues(v):
    """OPENCV: cv::Rodrigues, vector -> matrix, evaluated in double: identity below DBL_EPSILON,
    else (c*I + (1-c)*r*rT) + s*[r]x element by element. -> the nine doubles before narrowing"""
    x, y, z = float(v[0]), float(v[1]), float(v[2])
    with np.errstate(all="ignore"):
        theta = float(np.sqrt(F64(x * x + y * y + z * z)))  # (x*x + y*y) + z*z, as Python evaluates it
    if theta < DBL_EPSILON:
        return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if theta != theta or math.isinf(theta):
        c = s = float("nan")
    else:
        c, s = math.cos(theta), math.sin(theta)
    c1 = 1.0 - c
    with np.errstate(all="ignore"):
        it = float(F64(1.0) / F64(theta))
        r = [float(F64(x) * it), float(F64(y) * it), float(F64(z) * it)]
        eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        rx = [0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0]
        out = []
        for i in range(3):
            for j in range(3):
                e = F64(c) * F64(eye[3 * i + j]) + F64(c1) * (F64(r[i]) * F64(r[j]))
                e = e + F64(s) * F64(rx[3 * i + j])
                out.append(float(e))
    return out


def compute_sim3(P1, P2, fix_scale):
    """ComputeSim3 (:225-336). P1, P2: 3x3 float32, one point per column.
    -> dict R (3x3), t (3), s, T12 (3x4), T21 (3x4), q (evec row 0), N (4x4), eval, rotations,
       dbl: the doubles that are narrowed to float after a double transcendental:
            [alpha = 2*ang/norm(vec), R00 .. R22]"""
    P1 = np.asarray(P1, F32)
    P2 = np.asarray(P2, F32)
    with np.errstate(all="ignore"):
        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M = gemm(Pr2, Pr1.T)
        N11 = M[0, 0] + M[1, 1] + M[2, 2]
        N12 = M[1, 2] - M[2, 1]
        N13 = M[2, 0] - M[0, 2]
        N14 = M[0, 1] - M[1, 0]
        N22 = M[0, 0] - M[1, 1] - M[2, 2]
        N23 = M[0, 1] + M[1, 0]
        N24 = M[2, 0] + M[0, 2]
        N33 = -M[0, 0] + M[1, 1] - M[2, 2]
        N34 = M[1, 2] + M[2, 1]
        N44 = -M[0, 0] - M[1, 1] + M[2, 2]
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34],
                      [N14, N24, N34, N44]], F32)
        ev, evec, rotations = jacobi4(N)
        q = evec[0]
        vec = q[1:4].copy()
        # OPENCV: cv::norm of CV_32F accumulates the squares in double; its double result is used as is
        nrm = float(np.sqrt(F64(vec[0]) * F64(vec[0]) + F64(vec[1]) * F64(vec[1]) + F64(vec[2]) * F64(vec[2])))
        ang = math.atan2(nrm, float(q[0])) if nrm == nrm and q[0] == q[0] else float("nan")
        alpha = float(np.divide(F64(2.0 * ang), F64(nrm)))
        vec = vec * F32(alpha)  # OPENCV: 2*ang*vec/norm(vec) is one double alpha applied as a float scale
        Rd = rodrigues(vec)
        R = np.array(Rd, F64).astype(F32).reshape(3, 3)
        P3 = gemm(R, Pr2)
        if not fix_scale:
            nom = F64(0.0)
            den = F64(0.0)
            for i in range(3):
                for j in range(3):
                    nom = nom + F64(Pr1[i, j]) * F64(P3[i, j])  # OPENCV: Mat::dot: double sum of the float pairs' products, row-major
                    den = den + F64(P3[i, j] * P3[i, j])
            s = F32(np.divide(nom, den))
        else:
            s = F32(1.0)
        t = gemm(R, O2.reshape(3, 1), alpha=-float(s), C=O1.reshape(3, 1)).reshape(3)
        sR = (R * s).astype(F32)                                # OPENCV: s*R multiplies by (float)alpha
        a_inv = F32(np.divide(F64(1.0), F64(s)))
        sRinv = (R.T * a_inv).astype(F32)                       # OPENCV: (1.0/s)*R.t() multiplies by (float)alpha
        tinv = gemm(sRinv, t.reshape(3, 1), alpha=-1.0).reshape(3)
    T12 = np.concatenate([sR, t.reshape(3, 1)], axis=1).astype(F32)
    T21 = np.concatenate([sRinv, tinv.reshape(3, 1)], axis=1).astype(F32)
    return dict(R=R, t=t.astype(F32), s=F32(s), T12=T12, T21=T21, q=q, N=N, eval=ev, rotations=rotations,
                dbl=np.array([alpha] + Rd, F64))


# ---- CheckInliers (:338-420) ------------------------------------------------------------------------
def camera_to_image(X, K):
    fx, fy, cx, cy = (F32(v) for v in K)
    with np.errstate(all="ignore"):
        invz = F32(1.0) / X[:, 2]
        x = X[:, 0] * invz
        y = X[:, 1] * invz
        return fx * x + cx, fy * y + cy


def project(X, T, K):
    """Project (:379-400): Rcw * X + tcw by the double-accumulating gemm, then the float pinhole."""
    X = np.asarray(X, F32)
    P = np.zeros_like(X)
    with np.errstate(all="ignore"):
        for r in range(3):
            s = F64(T[r, 0]) * X[:, 0].astype(F64)
            s = s + F64(T[r, 1]) * X[:, 1].astype(F64)
            s = s + F64(T[r, 2]) * X[:, 2].astype(F64)
            s = s + F64(T[r, 3])
            P[:, r] = s.astype(F32)
    return camera_to_image(P, K)


def sq_err(u0, v0, u1, v1):
    with np.errstate(all="ignore"):
        d0 = (u0 - u1).astype(F64)
        d1 = (v0 - v1).astype(F64)
        return (d0 * d0 + d1 * d1).astype(F32)


class Sim3Solver:
    """One solver over the n correspondences that survived the constructor's filter (:61-101)."""

    def __init__(self, x3dc1, x3dc2, sigma2_1, sigma2_2, k1, k2, fix_scale):
        self.X1 = np.ascontiguousarray(x3dc1, F32).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(x3dc2, F32).reshape(-1, 3)
        self.N = len(self.X1)
        self.max1 = np.array([max_error(v) for v in np.asarray(sigma2_1, F32).reshape(-1)], np.int64)
        self.max2 = np.array([max_error(v) for v in np.asarray(sigma2_2, F32).reshape(-1)], np.int64)
        self.K1 = np.asarray(k1, F32)
        self.K2 = np.asarray(k2, F32)
        self.fix_scale = bool(fix_scale)
        self.p1im1 = camera_to_image(self.X1, self.K1) if self.N else (np.zeros(0, F32),) * 2
        self.p2im2 = camera_to_image(self.X2, self.K2) if self.N else (np.zeros(0, F32),) * 2
        self.set_ransac_parameters()
        self.hyp = []

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.min_inliers = int(min_inliers)
        self.max_its = (ransac_max_its(self.N, min_inliers, max_iterations, probability)
                        if self.N >= min_inliers else max(1, int(max_iterations)))
        self.iterations = 0
        self.best_inliers = 0
        self.best = -1

    def check_inliers(self, T12, T21):
        """-> bool[N]"""
        if self.N == 0:
            return np.zeros(0, bool)
        u21, v21 = project(self.X2, T12, self.K1)
        u12, v12 = project(self.X1, T21, self.K2)
        e1 = sq_err(self.p1im1[0], self.p1im1[1], u21, v21)
        e2 = sq_err(u12, v12, self.p2im2[0], self.p2im2[1])
        with np.errstate(all="ignore"):
            return (e1 < self.max1.astype(F32)) & (e2 < self.max2.astype(F32))

    def hypothesis(self, draws):
        idx = select3(self.N, draws)
        h = compute_sim3(self.X1[idx].T, self.X2[idx].T, self.fix_scale)
        h["idx"] = idx
        return h

    def evaluate(self, rand_idx):
        """Every hypothesis the draws allow, min(len(rand_idx) / 3, mRansacMaxIts) of them, each with
        its inlier mask and count."""
        self.hyp = []
        if self.N < self.min_inliers:
            return self.hyp
        rand_idx = np.asarray(rand_idx).reshape(-1, 3)
        for k in range(min(len(rand_idx), self.max_its)):
            h = self.hypothesis(rand_idx[k])
            h["inliers"] = self.check_inliers(h["T12"], h["T21"])
            h["count"] = int(h["inliers"].sum())
            self.hyp.append(h)
        return self.hyp

    def counts(self):
        return [h["count"] for h in self.hyp]


def iterate_counts(counts, n, min_inliers, max_its, n_iterations, state):
    """iterate() (:139-206) over precomputed per-hypothesis inlier counts. state = [mnIterations,
    mnBestInliers, best index] and is updated in place.
    -> (accepted hypothesis index or -1, bNoMore, nInliers)"""
    if n < min_inliers:
        return -1, True, 0
    cur = 0
    while state[0] < max_its and cur < n_iterations and state[0] < len(counts):
        cur += 1
        k = state[0]
        state[0] += 1
        if counts[k] >= state[1]:
            state[1] = counts[k]
            state[2] = k
            if counts[k] > min_inliers:
                return k, False, counts[k]
    return -1, state[0] >= max_its, 0


def find_counts(counts, n, min_inliers, max_its):
    """find() (:208-212): -> (accepted, nInliers, best index, mnBestInliers, bNoMore)"""
    state = [0, 0, -1]
    acc, no_more, n_in = iterate_counts(counts, n, min_inliers, max_its, max_its, state)
    if n < min_inliers:
        return -1, 0, -1, 0, True
    return acc, n_in, state[2], state[1], no_more
