"""A second reference for Frame::isInFrustum and for the query stage of the five projection searches,
NumPy only, written from the reference text and sharing no code with oracle/.

  is_in_frustum   Frame.cc:318-374 + MapPoint::PredictScale (MapPoint.cc:403-447), with the skip rules
                  of Tracking::SearchLocalPoints (Tracking.cc:1193-1196)
  queries         what each search computes per MapPoint before it walks the window:
                    "reloc"     SearchByProjection(Frame&, KeyFrame*, set, th, ORBdist)  ORBmatcher.cc:1493-1625
                    "sbp_scw"   SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)          :295-412
                    "fuse"      Fuse(KeyFrame*, vpMapPoints, th)                                      :841-991
                    "fuse_scw"  Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint)                    :993-1120
                    "by_sim3"   one direction of SearchBySim3                                         :1122-1346
  search          the window walk of those searches over a target frame (GetFeaturesInArea,
                  Frame.cc:376-433 / KeyFrame.cc:586-625, the level test, Fuse's chi-square gate, the
                  claim of a matched keypoint), enough to turn queries into an expected best_idx

Arithmetic: operands are float32; a cv::Mat gemm row, cv::norm and Mat::dot
accumulate in float64 and round once; everything else is float32 in the reference's own association
(isInFrustum and "reloc": fx*xc*invz + cx; the KeyFrame kinds: x = xc*invz, u = fx*x + cx). A
Mat / float and a float * Mat are MatExpr scalings by a float factor (1/scw is rounded to float
before it multiplies). PredictScale is ceil(logf(ratio) / lsf) with the C library's logf: the
float overloads the reference gets under `using namespace std`.

Unpinned by decision: inputs whose reference behaviour is undefined -- a NaN projection (zc == 0
with xc == 0, or "reloc" at zc == 0) reaching GetFeaturesInArea's float-to-int casts, a log scale
factor of 0. The scenes hold none.
"""
import ctypes
import ctypes.util

import numpy as np

F32, F64 = np.float32, np.float64
TRACK_IN_VIEW, BAD, OBSERVED, PRESENT, OUTLIER, SEEN, SKIP = 1, 2, 4, 8, 16, 32, 64
KINDS = ("reloc", "sbp_scw", "fuse", "fuse_scw", "by_sim3")
GRID_COLS, GRID_ROWS = 64, 48   # Frame.h:38-39

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x):
    x = np.asarray(x, F32)
    return np.array([_libm.logf(float(v)) for v in x.ravel()], F32).reshape(x.shape)


def gemv(A, X, add=None):
    """Rows of A (3x3 float32) times the rows of X (N, 3), plus `add`: float64 sums, one rounding."""
    A, X = np.asarray(A, F32).astype(F64), np.asarray(X, F32).reshape(-1, 3).astype(F64)
    s = X[:, 0:1] * A[None, :, 0]
    s = s + X[:, 1:2] * A[None, :, 1]
    s = s + X[:, 2:3] * A[None, :, 2]
    if add is not None:
        s = s + np.asarray(add, F32).astype(F64)[None, :]
    return s.astype(F32)


def norm3(V):
    V = np.asarray(V, F32).astype(F64)
    s = V[:, 0] * V[:, 0]
    s = s + V[:, 1] * V[:, 1]
    s = s + V[:, 2] * V[:, 2]
    return np.sqrt(s).astype(F32)


def dot3(A, B):
    """Mat::dot: float64, not rounded."""
    A, B = np.asarray(A, F32).astype(F64), np.asarray(B, F32).astype(F64)
    s = A[:, 0] * B[:, 0]
    s = s + A[:, 1] * B[:, 1]
    return s + A[:, 2] * B[:, 2]


def camera_centre(R, t):
    """Ow = -Rcw.t() * tcw: a gemm with alpha = -1."""
    return -gemv(np.asarray(R, F32).T, np.asarray(t, F32).reshape(1, 3))[0]


def split_pose(T):
    T = np.asarray(T, F32).reshape(-1, 4)[:3]
    return T[:, :3].copy(), T[:, 3].copy()


def split_scw(S):
    """:308-312 / :1006-1010. scw = sqrt(row0 . row0); Rcw = sRcw / scw; tcw = col(3) / scw."""
    S = np.asarray(S, F32).reshape(-1, 4)[:3]
    scw = F32(np.sqrt(dot3(S[0:1, :3], S[0:1, :3])[0]))
    f = F32(F64(1.0) / F64(scw))
    T = (S * f).astype(F32)
    return T[:, :3].copy(), T[:, 3].copy()


def predict_scale(max_d, dist, lsf, nlevels):
    with np.errstate(all="ignore"):
        ratio = np.asarray(max_d, F32) / np.asarray(dist, F32)
        n = np.ceil(logf(ratio) / F32(lsf))
    return np.clip(n, 0, nlevels - 1).astype(np.int32), ratio


def _cam(c):
    return tuple(F32(getattr(c, k)) for k in ("fx", "fy", "cx", "cy", "bf"))


def _bounds(f):
    return tuple(F32(getattr(f, k)) for k in ("min_x", "max_x", "min_y", "max_y"))


def geometry(kind, G, R, t, ow, cam, target, lsf, cos_limit=0.5, R2=None, t2=None):
    """Every intermediate of one function for every MapPoint, whatever its flags: zc, u, v, ur,
    dist, dot, view_cos, ratio, pred and the outcome of each test. kind is "frustum" or one of KINDS."""
    fx, fy, cx, cy, bf = _cam(cam)
    min_x, max_x, min_y, max_y = _bounds(target)
    nlevels = len(target.scale_factors)
    P = np.asarray(G.world_pos, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        Pc = gemv(R, P, t)
        if kind == "by_sim3":
            Pc = gemv(R2, Pc, t2)
        xc, yc, zc = Pc[:, 0], Pc[:, 1], Pc[:, 2]
        if kind == "frustum":
            invz = F32(1.0) / zc
        elif kind in ("sbp_scw", "fuse"):
            invz = F32(1) / zc                           # `1 / p3Dc.at<float>(2)`: a float division
        else:
            invz = (F64(1.0) / zc.astype(F64)).astype(F32)  # `1.0 / ...` rounded into a float
        if kind in ("frustum", "reloc"):
            u = fx * xc * invz + cx
            v = fy * yc * invz + cy
            in_image = ~((u < min_x) | (u > max_x)) & ~((v < min_y) | (v > max_y))
        else:
            x, y = xc * invz, yc * invz
            u = fx * x + cx
            v = fy * y + cy
            in_image = (u >= min_x) & (u < max_x) & (v >= min_y) & (v < max_y)   # KeyFrame::IsInImage
        depth_ok = np.ones(len(P), bool) if kind == "reloc" else ~(zc < F32(0.0))
        ur = u - bf * invz if kind in ("frustum", "fuse") else np.zeros(len(P), F32)
        PO = Pc if kind == "by_sim3" else P - np.asarray(ow, F32)[None, :]
        dist = norm3(PO)
        max_dist = F32(1.2) * np.asarray(G.max_distance, F32)
        min_dist = F32(0.8) * np.asarray(G.min_distance, F32)
        dist_ok = ~((dist < min_dist) | (dist > max_dist))
        dot = dot3(PO, G.normal)
        view_cos = (dot / dist.astype(F64)).astype(F32)
        if kind == "frustum":
            angle_ok = ~(view_cos < F32(cos_limit))
        elif kind in ("sbp_scw", "fuse", "fuse_scw"):
            angle_ok = ~(dot < 0.5 * dist.astype(F64))
        else:
            angle_ok = np.ones(len(P), bool)
        pred, ratio = predict_scale(G.max_distance, dist, lsf, nlevels)
    return dict(zc=zc, u=u, v=v, ur=ur.astype(F32), dist=dist, dot=dot, view_cos=view_cos, ratio=ratio, pred=pred,
                depth_ok=depth_ok, in_image=in_image, dist_ok=dist_ok, angle_ok=angle_ok,
                geo_ok=depth_ok & in_image & dist_ok & angle_ok, min_dist=min_dist, max_dist=max_dist)


def is_in_frustum(F, G, tcw, lsf, cos_limit=0.5):
    """-> dict(flags, proj_x, proj_y, proj_xr, level, view_cos, n_in_view). The five members are
    written only for the MapPoints in view (zero elsewhere, as nothing is written there)."""
    R, t = split_pose(tcw)
    g = geometry("frustum", G, R, t, camera_centre(R, t), F, F, lsf, cos_limit)
    fl = np.asarray(G.flags, np.uint8)
    cleared = fl & np.uint8(0xFF ^ TRACK_IN_VIEW)
    in_view = ((fl & (BAD | SEEN)) == 0) & g["geo_ok"]
    z = np.zeros(len(fl), F32)
    return dict(flags=np.where(in_view, cleared | np.uint8(TRACK_IN_VIEW), cleared).astype(np.uint8),
                proj_x=np.where(in_view, g["u"], z), proj_y=np.where(in_view, g["v"], z),
                proj_xr=np.where(in_view, g["ur"], z), level=np.where(in_view, g["pred"], 0).astype(np.int32),
                view_cos=np.where(in_view, g["view_cos"], z), n_in_view=int(in_view.sum()))


def sim3_between(s12, R12, t12):
    """:1139-1141 -> (sR12, t12, sR21, t21)."""
    R12 = np.asarray(R12, F32).reshape(3, 3)
    t12 = np.asarray(t12, F32).reshape(3)
    sR12 = (R12 * F32(s12)).astype(F32)
    sR21 = (R12.T * F32(F64(1.0) / F64(F32(s12)))).astype(F32)
    t21 = -gemv(sR21, t12.reshape(1, 3))[0]
    return sR12, t12, sR21, t21


def queries(kind, target, G, lsf, th, tcw=None, ow=None, scw=None, cam=None, R2=None, t2=None):
    """Per MapPoint (valid, u, v, ur, radius, min_level, max_level) of one search into `target`.
    "reloc": tcw (the Frame's pose). "fuse": tcw and the KeyFrame's own ow. The Scw kinds: scw.
    "by_sim3": tcw is the pose of the KeyFrame that owns the MapPoints, (R2, t2) takes its camera
    frame to the target's, cam is KF1 (both directions project with KF1's intrinsics), and lsf is
    the target's."""
    if kind in ("sbp_scw", "fuse_scw"):
        R, t = split_scw(scw)
    else:
        R, t = split_pose(tcw)
    if kind != "fuse":
        ow = camera_centre(R, t)
    g = geometry(kind, G, R, t, ow, cam if cam is not None else target, target, lsf, R2=R2, t2=t2)
    fl = np.asarray(G.flags, np.uint8)
    ok = (fl & (BAD | SKIP)) == 0
    if kind not in ("sbp_scw", "fuse_scw"):
        ok &= (fl & PRESENT) != 0
    valid = ok & g["geo_ok"]
    pred = g["pred"]
    radius = F32(th) * np.asarray(target.scale_factors, F32)[pred]
    return dict(valid=valid, u=g["u"], v=g["v"], ur=g["ur"], radius=radius, min_level=pred - 1,
                max_level=pred + 1 if kind == "reloc" else pred, pred=pred)


def by_sim3_queries(K1, K2, g1, g2, s12, R12, t12, lsf1, lsf2, th):
    """(queries of KF1's MapPoints into KF2, of KF2's into KF1)."""
    sR12, t12, sR21, t21 = sim3_between(s12, R12, t12)
    return (queries("by_sim3", K2, g1, lsf2, th, tcw=K1.tcw, cam=K1, R2=sR21, t2=t21),
            queries("by_sim3", K1, g2, lsf1, th, tcw=K2.tcw, cam=K1, R2=sR12, t2=t12))


# ---- the window walk ------------------------------------------------------------------------------
def _round_half_away(a):
    a = np.asarray(a, F64)
    return np.sign(a) * np.floor(np.abs(a) + 0.5)


def in_grid(target):
    """PosInGrid (Frame.cc:435-445): a keypoint outside the 64 x 48 cells is in no cell and is never
    returned by GetFeaturesInArea. A KeyFrame keeps the grid of the Frame it was made from."""
    origin = getattr(target, "grid_origin", None) or (target.min_x, target.min_y)
    kx, ky = target.keys_un["x"].astype(F32), target.keys_un["y"].astype(F32)
    px = _round_half_away((kx - F32(origin[0])) * F32(target.grid_inv_w))
    py = _round_half_away((ky - F32(origin[1])) * F32(target.grid_inv_h))
    return (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)


def hamming(a, B):
    return np.unpackbits(np.asarray(a, np.uint8)[None, :] ^ np.asarray(B, np.uint8), axis=1).sum(axis=1)


THRESHOLD = dict(sbp_scw=50, fuse=50, fuse_scw=50, by_sim3=100)   # TH_LOW / TH_HIGH; "reloc" takes ORBdist


def search(kind, q, target, desc, threshold=None):
    """best_idx per MapPoint: the first minimum over the keypoints of the window at the allowed
    levels, accepted at `<= threshold`. "reloc" and "sbp_scw" skip a keypoint that has a MapPoint and
    give a matched keypoint to no later MapPoint. Ties between candidates are not modelled (the cell
    order decides them): a tie raises."""
    threshold = THRESHOLD[kind] if threshold is None else threshold
    kx, ky = target.keys_un["x"].astype(F32), target.keys_un["y"].astype(F32)
    lvl = target.keys_un["octave"].astype(np.int64)
    usable = in_grid(target)
    if kind in ("reloc", "sbp_scw"):
        usable &= np.asarray(target.mp_state) == 0
    if kind == "fuse":
        assert np.all(np.asarray(target.u_right, F32) < 0), "the stereo gate is not modelled"
        inv_sigma2 = (F32(1.0) / np.asarray(target.level_sigma2, F32))[lvl]
    best = np.full(len(q["valid"]), -1, np.int32)
    for i in np.flatnonzero(q["valid"]):
        u, v, r = q["u"][i], q["v"][i], q["radius"][i]
        ex, ey = kx - u, ky - v
        c = usable & (np.abs(ex) < r) & (np.abs(ey) < r) & (lvl >= q["min_level"][i]) & (lvl <= q["max_level"][i])
        if kind == "fuse":   # :946-953: e2 * invSigma2 > 5.99 in double
            ex, ey = u - kx, v - ky
            e2 = ex * ex + ey * ey
            c &= ~((e2 * inv_sigma2).astype(F64) > 5.99)
        c = np.flatnonzero(c)
        if len(c) == 0:
            continue
        d = hamming(desc[i], target.descriptors[c])
        k = int(np.argmin(d))
        if (d == d[k]).sum() > 1:
            raise ValueError(f"MapPoint {i}: candidates tie at distance {d[k]}")
        if d[k] <= threshold:
            best[i] = c[k]
            if kind in ("reloc", "sbp_scw"):
                usable[c[k]] = False
    return best


def agree(m1, m2):
    """SearchBySim3's agreement (:1328-1343) -> (nFound, match12)."""
    out = np.full(len(m1), -1, np.int32)
    for i1, i2 in enumerate(m1):
        if i2 >= 0 and m2[i2] == i1:
            out[i1] = i2
    return int((out >= 0).sum()), out
