"""Frame::ComputeStereoMatches (src/Frame.cc:522-700) in plain NumPy: the second reference.

Written from what the routine does, step by step, with none of the shortcuts the HIP kernels or
the C++ restatement take. It imports nothing from oracle/ or from the package.

  * the row table is a list per image row; right keypoint iR is appended to every row from
    floor(y - r) to ceil(y + r), r = 2 * scale[octave], in iR order;
  * the candidates of a left keypoint are that list, scanned front to back, and a candidate wins
    only on a strictly smaller Hamming distance than the best so far, which starts at 100;
  * the two 11x11 windows become float32 arrays with their centre pixel subtracted, and the
    distance at each of the 11 shifts is the L1 norm of their difference;
  * the first strictly smallest shift wins; the parabola, the re-scaled coordinate, the disparity
    and the depth are float32 operations in the order the source writes them;
  * the median is element M/2 of the sorted (SAD, iL) pairs, and the sorted list is walked from
    its end, dropping matches until one has SAD < 1.5f * 1.4f * median.

Every `float` of the source is a numpy.float32 here and each operation rounds once, as the C++
does on x86-64 (no excess precision, no contraction on these expressions).

Three places where the source has no defined behaviour are decided, not derived:
  * windows that leave the level image. cv::Mat::rowRange / colRange would throw there (or, built
    without checks, read out of bounds). This reference SKIPS such a keypoint, by the same rule the
    C++ restatement and the kernel use: the left window needs 0 <= x-5, x+5 < cols, 0 <= y-5,
    y+5 < rows, and the right sweep needs 0 <= xR0-10 (its right end is the source's own
    `endu >= cols` test). This one rule is shared with the code under test by decision.
  * row-table rows outside [0, nRows) (the source indexes the vector unchecked) are dropped, and a
    left keypoint whose (int)y is outside the table has no row.
  * an empty match list (the source indexes element 0 of an empty vector): nothing is rejected.

Besides (u_right, depth) every left keypoint gets an outcome code naming where it left the routine.
"""
import numpy as np

F = np.float32

OUTCOMES = ("no_row", "no_candidate", "orb_dist", "window_off_image", "min_at_shift_edge", "delta_out",
            "disparity_negative", "disparity_ge_maxD", "median_rejected", "accepted",
            "accepted_zero_disparity")

TH_HIGH, TH_LOW = 100, 50  # ORBmatcher.h
W, L = 5, 5                # Frame.cc:618, :628

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _round_half_away(x):
    """C round() of a float32, as a float32 (exact: |x| + 0.5 is exact in float64)."""
    x = float(x)
    m = np.floor(abs(x) + 0.5)
    return F(m if x >= 0 else -m)


def _window(img, yc, xc):
    """rowRange(yc-5, yc+6).colRange(xc-5, xc+6), converted to float32, minus its centre pixel."""
    a = img[yc - W:yc + W + 1, xc - W:xc + W + 1].astype(np.float32)
    return a - a[W, W]


def compute_stereo_matches(kl, dl, kr, dr, pyr_l, pyr_r, scale, inv_scale, mb, mbf):
    """kl, kr: structured arrays with x, y, octave; dl, dr: n x 32 uint8; pyr_l, pyr_r: level images.
    Returns a dict: u_right, depth (float32), outcome (list of str), best_iR (-1: none), best_dist
    (100: none), sads (n x 11, -1 where the sweep did not run), best_shift (-99: none)."""
    n, nr = len(kl), len(kr)
    scale = np.asarray(scale, np.float32)
    inv_scale = np.asarray(inv_scale, np.float32)
    mb, mbf = F(mb), F(mbf)
    u_right = np.full(n, -1.0, np.float32)
    depth = np.full(n, -1.0, np.float32)
    outcome = [None] * n
    best_iR = np.full(n, -1, np.int64)
    best_dist = np.full(n, TH_HIGH, np.int64)
    sads = np.full((n, 2 * L + 1), -1, np.int64)
    best_shift = np.full(n, -99, np.int64)
    dl = np.asarray(dl, np.uint8).reshape(-1, 32)
    dr = np.asarray(dr, np.uint8).reshape(-1, 32)

    th_orb = (TH_HIGH + TH_LOW) // 2
    n_rows = pyr_l[0].shape[0]
    table = [[] for _ in range(n_rows)]
    for iR in range(nr):
        y = F(kr["y"][iR])
        r = F(2.0) * scale[int(kr["octave"][iR])]
        maxr = int(np.ceil(F(y + r)))
        minr = int(np.floor(F(y - r)))
        for yi in range(minr, maxr + 1):
            if 0 <= yi < n_rows:
                table[yi].append(iR)

    with np.errstate(divide="ignore", invalid="ignore"):
        maxD = F(mbf / mb)
    minD = F(0)
    matches = []  # (SAD, iL)
    for iL in range(n):
        levelL = int(kl["octave"][iL])
        vL, uL = F(kl["y"][iL]), F(kl["x"][iL])
        if not (vL >= 0 and vL < n_rows):
            outcome[iL] = "no_row"
            continue
        cand = table[int(vL)]
        if not cand:
            outcome[iL] = "no_row"
            continue
        minU, maxU = F(uL - maxD), F(uL - minD)
        if maxU < 0:
            outcome[iL] = "no_candidate"
            continue
        best, best_r, tried = TH_HIGH, 0, 0
        for iR in cand:
            o = int(kr["octave"][iR])
            if o < levelL - 1 or o > levelL + 1:
                continue
            uR = F(kr["x"][iR])
            if uR >= minU and uR <= maxU:
                tried += 1
                d = int(_POP[np.bitwise_xor(dl[iL], dr[iR])].sum())
                if d < best:
                    best, best_r = d, iR
        best_dist[iL] = best
        if best < TH_HIGH:
            best_iR[iL] = best_r
        if not best < th_orb:
            outcome[iL] = "orb_dist" if tried else "no_candidate"
            continue

        uR0 = F(kr["x"][best_r])
        sf = inv_scale[levelL]
        su = _round_half_away(F(uL * sf))
        sv = _round_half_away(F(vL * sf))
        sr = _round_half_away(F(uR0 * sf))
        IMG_L, IMG_R = pyr_l[levelL], pyr_r[levelL]
        rows, cols = IMG_L.shape
        xL, yL, xR0 = int(su), int(sv), int(sr)
        iniu = F(F(sr + F(L)) - F(W))
        endu = F(F(F(sr + F(L)) + F(W)) + F(1))
        if iniu < 0 or endu >= IMG_R.shape[1]:
            outcome[iL] = "window_off_image"
            continue
        if (yL - W < 0 or yL + W >= rows or yL + W >= IMG_R.shape[0] or xL - W < 0 or xL + W >= cols
                or xR0 - L - W < 0):
            outcome[iL] = "window_off_image"  # the shared skip rule (module docstring)
            continue
        IL = _window(IMG_L, yL, xL)
        best_sad, best_inc = 2 ** 31 - 1, 0
        dists = np.zeros(2 * L + 1, np.float32)
        for inc in range(-L, L + 1):
            IR = _window(IMG_R, yL, xR0 + inc)
            dist = F(np.abs(IL - IR).astype(np.float64).sum())
            if dist < F(best_sad):
                best_sad, best_inc = int(dist), inc
            dists[L + inc] = dist
        sads[iL] = dists.astype(np.int64)
        best_shift[iL] = best_inc
        if best_inc == -L or best_inc == L:
            outcome[iL] = "min_at_shift_edge"
            continue
        d1, d2, d3 = dists[L + best_inc - 1], dists[L + best_inc], dists[L + best_inc + 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = F(F(d1 - d3) / F(F(2.0) * F(F(d1 + d3) - F(F(2.0) * d2))))
        if delta < -1 or delta > 1:
            outcome[iL] = "delta_out"
            continue
        best_u = F(scale[levelL] * F(F(F(sr) + F(best_inc)) + delta))
        disparity = F(uL - best_u)
        if disparity >= minD and disparity < maxD:
            zero = bool(disparity <= 0)
            if zero:
                disparity = F(0.01)
                best_u = F(np.float64(uL) - 0.01)
            depth[iL] = F(mbf / disparity)
            u_right[iL] = best_u
            matches.append((best_sad, iL))
            outcome[iL] = "accepted_zero_disparity" if zero else "accepted"
        else:
            outcome[iL] = "disparity_negative" if disparity < minD else "disparity_ge_maxD"

    if matches:
        matches.sort()
        median = F(matches[len(matches) // 2][0])
        th = F(F(F(1.5) * F(1.4)) * median)
        for sad, iL in reversed(matches):
            if F(sad) < th:
                break
            u_right[iL] = -1
            depth[iL] = -1
            outcome[iL] = "median_rejected"
    return {"u_right": u_right, "depth": depth, "outcome": outcome, "best_iR": best_iR,
            "best_dist": best_dist, "sads": sads, "best_shift": best_shift}
