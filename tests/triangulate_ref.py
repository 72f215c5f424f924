"""The per-match loop of LocalMapping::CreateNewMapPoints restated in plain Python / numpy -- the
yardstick of the GPU triangulation tests. It shares no code with the product.

Restates, of the reference:
  src/LocalMapping.cc:290-438   the match loop (parallax, linear triangulation, the eight gates)
  src/KeyFrame.cc:632-648       KeyFrame::UnprojectStereo
Every `float` of the reference is a numpy.float32 and every operation on it is rounded separately;
every `double` is a numpy.float64.

The OpenCV calls are restated from a reading of OpenCV 3.x/4.x that could not be checked against an
OpenCV build; each such rule is one line marked `# OPENCV:`, and each C library call one line marked
`# LIBM:`, so that it can be corrected in one place. orbfe_triangulate_core.h mirrors every marked
line and DESIGN.md section 16 lists them.

A KeyFrame here is any object with: keys_un (x, y, octave), u_right, scale_factors, level_sigma2,
fx, fy, cx, cy, bf, mb, tcw (3x4), ow (3), depth, keys_xy (None = the undistorted keys).
"""
import ctypes
import ctypes.util

import numpy as np

F32 = np.float32
F64 = np.float64
FLT_EPSILON = F32(np.finfo(np.float32).eps)

NO_MATCH, TRIANGULATED, STEREO1, STEREO2 = 0, 1, 2, 3
REJ_PARALLAX, REJ_W_ZERO, REJ_Z1, REJ_Z2, REJ_REPROJ1, REJ_REPROJ2 = -1, -2, -3, -4, -5, -6
REJ_DIST_ZERO, REJ_SCALE, REJ_UNPROJECT, REJ_BAD_MATCH, REJ_BAD_OCTAVE = -7, -8, -9, -10, -11
MP_OBSERVED = 2

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f, _n in (("cosf", 1), ("atan2f", 2)):
    getattr(_libm, _f).restype = ctypes.c_float
    getattr(_libm, _f).argtypes = [ctypes.c_float] * _n


def cosf(x):
    return F32(_libm.cosf(float(F32(x))))        # LIBM: std::cos(float) is cosf


def atan2f(y, x):
    return F32(_libm.atan2f(float(F32(y)), float(F32(x))))  # LIBM: std::atan2(float, float) is atan2f


def dot3_d(a, b):
    # OPENCV: CV_32F gemm element / Mat::dot of three float pairs: double accumulation left to right
    s = F64(a[0]) * F64(b[0])
    s = s + F64(a[1]) * F64(b[1])
    s = s + F64(a[2]) * F64(b[2])
    return s


def norm3_d(a):
    # OPENCV: cv::norm (NORM_L2) of a CV_32F 3x1: the squares accumulate in double; the double result
    return np.sqrt(dot3_d(a, a))


def hypot_d(a, b):
    # OPENCV: lapack.cpp's own hypot template, instantiated for double by JacobiSVDImpl_'s hypot((double)p, beta)
    a, b = abs(F64(a)), abs(F64(b))
    if a > b:
        b = b / a
        return a * np.sqrt(F64(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(F64(1) + a * a)
    return F64(0)


def svd4(A):
    """OPENCV: cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a 4x4 CV_32F is
    JacobiSVDImpl_<float> on the transpose (At row i = column i of A) without LAPACK.
    -> (w[4] float32, vt[4][4] float32, sweeps)"""
    n = 4
    A = np.asarray(A, F32)
    At = [[F32(A[k, i]) for k in range(n)] for i in range(n)]
    Vt = [[F32(1.0) if i == k else F32(0.0) for k in range(n)] for i in range(n)]
    W = [F64(0)] * n
    with np.errstate(all="ignore"):
        for i in range(n):
            sd = F64(0)
            for k in range(n):
                sd = sd + F64(At[i][k]) * F64(At[i][k])  # OPENCV: row norms of At accumulate in double
            W[i] = sd
        eps = FLT_EPSILON * F32(2)  # OPENCV: JacobiSVD(float*) passes eps = FLT_EPSILON * 2
        sweeps = 0
        for sweeps in range(1, 31):  # OPENCV: JacobiSVDImpl_ runs at most max(m, 30) sweeps (m = 4)
            changed = False
            for i in range(n - 1):
                for j in range(i + 1, n):  # OPENCV: column pairs in the fixed order i < j
                    a, b, p = W[i], W[j], F64(0)
                    for k in range(n):
                        p = p + F64(At[i][k]) * F64(At[j][k])
                    if abs(p) <= F64(eps) * np.sqrt(a * b):  # OPENCV: the skip test, eps * sqrt(a * b) in double
                        continue
                    p = p * F64(2)
                    beta = a - b
                    gamma = hypot_d(p, beta)
                    if beta < 0:
                        delta = (gamma - beta) * F64(0.5)
                        s = F32(np.sqrt(delta / gamma))
                        c = F32(p / (gamma * F64(s) * F64(2)))
                    else:
                        c = F32(np.sqrt((gamma + beta) / (gamma * F64(2))))
                        s = F32(p / (gamma * F64(c) * F64(2)))
                    a = b = F64(0)
                    for k in range(n):
                        t0 = c * At[i][k] + s * At[j][k]
                        t1 = (-s) * At[i][k] + c * At[j][k]
                        At[i][k], At[j][k] = t0, t1
                        a = a + F64(t0) * F64(t0)
                        b = b + F64(t1) * F64(t1)
                    W[i], W[j] = a, b
                    changed = True
                    for k in range(n):
                        t0 = c * Vt[i][k] + s * Vt[j][k]
                        t1 = (-s) * Vt[i][k] + c * Vt[j][k]
                        Vt[i][k], Vt[j][k] = t0, t1
            if not changed:
                break
        for i in range(n):
            sd = F64(0)
            for k in range(n):
                sd = sd + F64(At[i][k]) * F64(At[i][k])
            W[i] = np.sqrt(sd)
        # OPENCV: singular values sorted descending by selection (W[j] < W[k] on the doubles), rows of Vt
        # swapped with them, signs as the rotations left them
        for i in range(n - 1):
            j = i
            for k in range(i + 1, n):
                if W[j] < W[k]:
                    j = k
            if i != j:
                W[i], W[j] = W[j], W[i]
                Vt[i], Vt[j] = Vt[j], Vt[i]
    return np.array(W, F64).astype(F32), np.array(Vt, F32), sweeps


def unproject_stereo(kf, i):
    """KeyFrame::UnprojectStereo (KeyFrame.cc:632-648): -> float32[3], or None for the empty Mat."""
    z = F32(kf.depth[i])
    if not z > 0:
        return None
    xy = kf.keys_xy if kf.keys_xy is not None else None
    u = F32(xy[i, 0]) if xy is not None else F32(kf.keys_un["x"][i])
    v = F32(xy[i, 1]) if xy is not None else F32(kf.keys_un["y"][i])
    with np.errstate(all="ignore"):
        invfx, invfy = F32(1.0) / F32(kf.fx), F32(1.0) / F32(kf.fy)
        x = (u - F32(kf.cx)) * z * invfx
        y = (v - F32(kf.cy)) * z * invfy
        T = np.asarray(kf.tcw, F32).reshape(3, 4)
        O = np.asarray(kf.ow, F32)
        # OPENCV: Rwc * x3Dc + twc is one gemm with C: the double sum plus C in double, one rounding
        return np.array([F32(dot3_d(T[:, r], (x, y, z)) + F64(O[r])) for r in range(3)], F32)


def _reproj_rejects(kf, i, stereo, bf, X, z):
    T = np.asarray(kf.tcw, F32).reshape(3, 4)
    fx, fy, cx, cy = F32(kf.fx), F32(kf.fy), F32(kf.cx), F32(kf.cy)
    sigma2 = F32(kf.level_sigma2[int(kf.keys_un["octave"][i])])
    x = F32(dot3_d(T[0, :3], X) + F64(T[0, 3]))
    y = F32(dot3_d(T[1, :3], X) + F64(T[1, 3]))
    invz = F32(F64(1.0) / F64(z))  # invz = 1.0 / z: a double quotient, narrowed
    u = fx * x * invz + cx
    v = fy * y * invz + cy
    ex = u - F32(kf.keys_un["x"][i])
    ey = v - F32(kf.keys_un["y"][i])
    if not stereo:
        return bool(F64(ex * ex + ey * ey) > F64(5.991) * F64(sigma2))  # a double comparison
    u_r = u - F32(bf) * invz
    er = u_r - F32(kf.u_right[i])
    return bool(F64(ex * ex + ey * ey + er * er) > F64(7.8) * F64(sigma2))  # a double comparison


def parallax(kf1, kf2, idx1, idx2):
    """The cosines of :304-320 alone. -> dict(cos_rays, cos_st1, cos_st2, st1, st2, xn1, xn2)"""
    with np.errstate(all="ignore"):
        k1, k2 = kf1.keys_un, kf2.keys_un
        T1 = np.asarray(kf1.tcw, F32).reshape(3, 4)
        T2 = np.asarray(kf2.tcw, F32).reshape(3, 4)
        st1 = bool(F32(kf1.u_right[idx1]) >= 0)
        st2 = bool(F32(kf2.u_right[idx2]) >= 0)
        invfx1, invfy1 = F32(1.0) / F32(kf1.fx), F32(1.0) / F32(kf1.fy)
        invfx2, invfy2 = F32(1.0) / F32(kf2.fx), F32(1.0) / F32(kf2.fy)
        # OPENCV: Mat_<float>(3,1) << a, b, 1.0 stores each operand converted to float
        xn1 = ((F32(k1["x"][idx1]) - F32(kf1.cx)) * invfx1, (F32(k1["y"][idx1]) - F32(kf1.cy)) * invfy1, F32(1.0))
        xn2 = ((F32(k2["x"][idx2]) - F32(kf2.cx)) * invfx2, (F32(k2["y"][idx2]) - F32(kf2.cy)) * invfy2, F32(1.0))
        ray1 = [F32(dot3_d(T1[:, r], xn1)) for r in range(3)]  # Rwc = Rcw^T exactly
        ray2 = [F32(dot3_d(T2[:, r], xn2)) for r in range(3)]
        cos_rays = F32(dot3_d(ray1, ray2) / (norm3_d(ray1) * norm3_d(ray2)))
        cos_st1 = cos_st2 = cos_rays + F32(1)
        if st1:
            cos_st1 = cosf(F32(2) * atan2f(F32(kf1.mb) / F32(2), F32(kf1.depth[idx1])))
        elif st2:
            cos_st2 = cosf(F32(2) * atan2f(F32(kf2.mb) / F32(2), F32(kf2.depth[idx2])))
    return dict(cos_rays=cos_rays, cos_st1=cos_st1, cos_st2=cos_st2, st1=st1, st2=st2, xn1=xn1, xn2=xn2)


def triangulate_match(kf1, kf2, idx1, idx2, detail=None):
    """One match of :290-438. -> (status, float32[3] or None). With a dict `detail`, the parallax
    cosines and (on the SVD path) A and vt.row(3) are left in it."""
    with np.errstate(all="ignore"):
        k1, k2 = kf1.keys_un, kf2.keys_un
        o1, o2 = int(k1["octave"][idx1]), int(k2["octave"][idx2])
        if not (0 <= o1 < len(kf1.scale_factors) and 0 <= o2 < len(kf2.scale_factors)):
            return REJ_BAD_OCTAVE, None
        T1 = np.asarray(kf1.tcw, F32).reshape(3, 4)
        T2 = np.asarray(kf2.tcw, F32).reshape(3, 4)
        O1, O2 = np.asarray(kf1.ow, F32), np.asarray(kf2.ow, F32)
        par = parallax(kf1, kf2, idx1, idx2)
        st1, st2, xn1, xn2 = par["st1"], par["st2"], par["xn1"], par["xn2"]
        cos_rays, cos_st1, cos_st2 = par["cos_rays"], par["cos_st1"], par["cos_st2"]
        cos_st = cos_st2 if cos_st2 < cos_st1 else cos_st1  # std::min(a, b): b < a ? b : a
        if detail is not None:
            detail.update(cos_rays=cos_rays, cos_st1=cos_st1, cos_st2=cos_st2, st1=st1, st2=st2)
        if cos_rays < cos_st and cos_rays > 0 and (st1 or st2 or F64(cos_rays) < F64(0.9998)):
            A = np.zeros((4, 4), F32)
            # OPENCV: a * M.row(r) - M.row(q) is one scaled add on floats: fl(fl(a * m_r) - m_q)
            A[0] = xn1[0] * T1[2] - T1[0]
            A[1] = xn1[1] * T1[2] - T1[1]
            A[2] = xn2[0] * T2[2] - T2[0]
            A[3] = xn2[1] * T2[2] - T2[1]
            _, vt, _ = svd4(A)
            v = vt[3]
            if detail is not None:
                detail.update(A=A, v=v)
            if v[3] == 0:
                return REJ_W_ZERO, None
            inv = F32(F64(1.0) / F64(v[3]))  # OPENCV: Mat / scalar multiplies by (float)(1.0 / s)
            X = np.array([v[0] * inv, v[1] * inv, v[2] * inv], F32)
            status = TRIANGULATED
        elif st1 and cos_st1 < cos_st2:
            X = unproject_stereo(kf1, idx1)
            status = STEREO1
            if X is None:
                return REJ_UNPROJECT, None
        elif st2 and cos_st2 < cos_st1:
            X = unproject_stereo(kf2, idx2)
            status = STEREO2
            if X is None:
                return REJ_UNPROJECT, None
        else:
            return REJ_PARALLAX, None
        z1 = F32(dot3_d(T1[2, :3], X) + F64(T1[2, 3]))
        if z1 <= 0:
            return REJ_Z1, None
        z2 = F32(dot3_d(T2[2, :3], X) + F64(T2[2, 3]))
        if z2 <= 0:
            return REJ_Z2, None
        if _reproj_rejects(kf1, idx1, st1, kf1.bf, X, z1):
            return REJ_REPROJ1, None
        if _reproj_rejects(kf2, idx2, st2, kf1.bf, X, z2):  # mpCurrentKeyFrame->mbf (:411)
            return REJ_REPROJ2, None
        dist1 = F32(norm3_d(X - O1))
        dist2 = F32(norm3_d(X - O2))
        if dist1 == 0 or dist2 == 0:
            return REJ_DIST_ZERO, None
        ratio_dist = dist2 / dist1
        ratio_octave = F32(kf1.scale_factors[o1]) / F32(kf2.scale_factors[o2])
        ratio_factor = F32(1.5) * F32(kf1.scale_factors[1]) if len(kf1.scale_factors) > 1 else F32(1.5)
        if ratio_dist * ratio_factor < ratio_octave or ratio_dist > ratio_octave * ratio_factor:
            return REJ_SCALE, None
        return status, X


def triangulate_ref(kf1, kf2, match12, x3d=None):
    """The loop over (idx1, match12[idx1]) in ascending idx1. -> (status int8[n1], x3d float32[n1,3],
    nnew). x3d (or zeros) is kept wherever status <= 0."""
    n1 = len(kf1.keys_un)
    n2 = len(kf2.keys_un)
    status = np.zeros(n1, np.int8)
    out = np.zeros((n1, 3), F32) if x3d is None else np.array(x3d, F32).reshape(n1, 3).copy()
    for i in range(n1):
        m = int(match12[i])
        if m < 0:
            continue
        if m >= n2:
            status[i] = REJ_BAD_MATCH
            continue
        st, X = triangulate_match(kf1, kf2, i, m)
        status[i] = st
        if st > 0:
            out[i] = X
    return status, out, int((status > 0).sum())


def ulps32(a, b):
    """Distance of two finite float32 in units in the last place (of the ordered-integer line)."""
    def key(x):
        v = int(np.array([x], F32).view(np.int32)[0])
        return v if v >= 0 else -(v & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def libm_band(kf1, kf2, idx1, idx2):
    """The smallest ulp distance between two quantities that :323-349 compare and of which one came
    out of cosf / atan2f, or None when the match calls neither. A decision can differ between two
    C libraries only where this is small."""
    d = parallax(kf1, kf2, idx1, idx2)
    if not (d["st1"] or d["st2"]):
        return None
    return min(ulps32(d["cos_rays"], d["cos_st1"]), ulps32(d["cos_rays"], d["cos_st2"]),
               ulps32(d["cos_st1"], d["cos_st2"]))
