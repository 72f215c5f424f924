"""Hand-built inputs for Frame::ComputeStereoMatches (src/Frame.cc:522-700), each named for the
branch it drives. Pure NumPy; imports neither the package nor oracle/.

A case is two level-0 images, the extractor parameters that build their pyramids, hand-written
keypoint / descriptor arrays, (mbf, mb), and `expect`: {left index: {key: value}} with keys
  outcome   stereo_ref outcome code          winner  best iR (-1: none)
  dist      best Hamming distance (100: none) shift  best SAD shift
  sad       SAD at the best shift             sads   all 11 SADs
  swept     True: the SAD sweep ran (the windows were inside the level)
tests/test_stereo_ref.py proves on the CPU that every case produces what it is named for;
tests/test_gpu_stereo_edges.py re-asserts it on the levels the kernels read.

How the cases isolate one keypoint pair from the next
  * descriptors are rows of the 256 x 256 Sylvester-Hadamard matrix: two different rows differ in
    exactly 128 bits. A pair is a row and the same row with d <= 28 leading bits flipped, so its own
    distance is d and every foreign distance is >= 100 and can never become a best distance;
  * probes with larger d (74, 75, 99, 100, the stride probes) sit on rows no other probe's span
    reaches, or further apart in x than the disparity window maxD = 32;
  * SADs are set by pasting a shifted copy of the left texture into an unrelated right texture
    (wrong shifts cost thousands) and then adding a known total to non-centre-row pixels of the
    left window, so the SAD at the matching shift is exactly that total.

Unreachable, and therefore not built
  * outcome `delta_out`. The first strict minimum at an interior shift has d1 > d2 and d3 >= d2,
    all integers below 2^17 and exact in float32. With a = d1 - d2 > 0 and b = d3 - d2 >= 0,
    deltaR = (a - b) / (2 (a + b)) and |a - b| <= a + b, so |deltaR| <= 0.5 (division rounds
    monotonically, 0.5 is representable). `deltaR < -1 || deltaR > 1` can never hold; the
    `sad_binary` case reaches the extreme 0.5 exactly.
  * a left window at xL = 5 (or 4): a candidate has uR <= uL, rounding is monotonic, so xR0 <= xL,
    and the right sweep needs xR0 >= 10. The left-edge test of the left window cannot fire before
    the right one; the cases hold yL at 4 / 5 / rows-6 / rows-5 and xL at cols-6 / cols-5 instead.
"""
from types import SimpleNamespace

import numpy as np

F = np.float32
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
               ("octave", "<i4"), ("class_id", "<i4")])
EXEMPT = {"delta_out": "|deltaR| <= 0.5 at a first strict interior minimum (module docstring)"}
INF = F(np.inf)


def scale_tables(sf, nlevels):
    """mvScaleFactor / mvInvScaleFactor as ORBextractor.cc:422-433 builds them (float products)."""
    s = np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        s[i] = F(s[i - 1] * F(sf))
    return s, (F(1.0) / s).astype(np.float32)


def level_shape(rows, cols, inv):
    return int(np.rint(F(F(rows) * inv))), int(np.rint(F(F(cols) * inv)))


def hadamard(i):
    bits = np.array([bin(i & j).count("1") & 1 for j in range(256)], np.uint8)
    return np.packbits(bits)


def flipped(desc, bits):
    b = np.unpackbits(desc)
    b[list(bits)] ^= 1
    return np.packbits(b)


def texture(rows, cols, seed):
    return np.random.RandomState(seed).randint(64, 192, (rows, cols)).astype(np.uint8)


def up(x):
    return np.nextafter(F(x), INF)


def down(x):
    return np.nextafter(F(x), -INF)


def last_y_reaching_from_below(v, r):
    """Largest float32 y with floor(y - r) == v: the next float up starts its span at v + 1."""
    y = F(F(v + 1) + r)
    while np.floor(F(y - r)) > v:
        y = down(y)
    while np.floor(F(up(y) - r)) <= v:
        y = up(y)
    return y


def first_y_reaching_from_above(v, r):
    """Smallest float32 y with ceil(y + r) == v: the next float down ends its span at v - 1."""
    y = F(F(v - 1) - r)
    while np.ceil(F(y + r)) < v:
        y = up(y)
    while np.ceil(F(down(y) + r)) >= v:
        y = down(y)
    return y


class Builder:
    def __init__(self, name, sf, nlevels, rows, cols, mbf=16.0, mb=0.5, seed=1, shift=None, flat=None):
        self.name, self.sf, self.nlevels, self.rows, self.cols = name, sf, nlevels, rows, cols
        self.mbf, self.mb = mbf, mb
        self.scale, self.inv = scale_tables(sf, nlevels)
        if flat is not None:
            self.left = np.full((rows, cols), flat, np.uint8)
            self.right = self.left.copy()
        else:
            self.left = texture(rows, cols, seed)
            self.right = texture(rows, cols, seed + 1000)
            if shift is not None:  # right[x] = left[x + shift]: disparity `shift` everywhere
                self.right[:, :cols - shift] = self.left[:, shift:]
        self.kl, self.dl, self.kr, self.dr = [], [], [], []
        self.expect, self.word = {}, 1
        self.injections = []

    def new_word(self):
        w = hadamard(self.word)
        self.word += 1
        assert self.word <= 256
        return w

    def add_left(self, x, y, octave, desc):
        self.kl.append((F(x), F(y), octave))
        self.dl.append(desc)
        return len(self.kl) - 1

    def add_right(self, x, y, octave, desc):
        self.kr.append((F(x), F(y), octave))
        self.dr.append(desc)
        return len(self.kr) - 1

    def pair(self, xl, yl, ol, xr, yr, orr, d=10, word=None):
        w = self.new_word() if word is None else word
        iL = self.add_left(xl, yl, ol, w)
        iR = self.add_right(xr, yr, orr, flipped(w, range(d)))
        return iL, iR

    def want(self, iL, **kw):
        self.expect.setdefault(iL, {}).update(kw)

    def paste(self, yc, xc, dd, hw=24, hh=7):
        """right[y, x] = left[y, x + dd] around (yc, xc): the left content at column c shows at c - dd."""
        for y in range(max(0, yc - hh), min(self.rows, yc + hh + 1)):
            for x in range(max(0, xc - hw), min(self.cols, xc + hw + 1)):
                if 0 <= x + dd < self.cols:
                    self.right[y, x] = self.left[y, x + dd]

    def inject(self, yc, xc, total, symmetric=False):
        """Raise non-centre-row pixels of the left window at (yc, xc) by `total` in all (applied when
        the case is finished, after every paste has copied the untouched texture)."""
        self.injections.append((yc, xc, total, symmetric))

    def _apply(self, yc, xc, total, symmetric):
        left = total
        for dy in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5):
            for dx in (range(1, 6) if symmetric else range(-5, 6)):
                if left <= 0:
                    return
                if symmetric:
                    a = min(60, left // 2)
                    self.left[yc + dy, xc + dx] += a
                    self.left[yc + dy, xc - dx] += a
                    left -= 2 * a
                else:
                    a = min(60, left)
                    self.left[yc + dy, xc + dx] += a
                    left -= a
        assert left == 0

    def done(self):
        for j in self.injections:
            self._apply(*j)

        def kps(lst):
            a = np.zeros(len(lst), KP)
            for i, (x, y, o) in enumerate(lst):
                a[i]["x"], a[i]["y"], a[i]["octave"] = x, y, o
                a[i]["size"], a[i]["angle"], a[i]["class_id"] = 31.0, 0.0, -1
            return a

        def descs(lst):
            return np.array(lst, np.uint8).reshape(-1, 32)

        return SimpleNamespace(name=self.name, sf=self.sf, nlevels=self.nlevels, left=self.left,
                               right=self.right, kl=kps(self.kl), dl=descs(self.dl), kr=kps(self.kr),
                               dr=descs(self.dr), mbf=self.mbf, mb=self.mb, expect=self.expect,
                               scale=self.scale, inv_scale=self.inv)


# ---- row band, octave filter, disparity window, Hamming thresholds, 16-lane stride, ties -----------
BALLAST_SAD = 40


def band_case(name, sf, nlevels, rows, cols):
    """maxD = 32, right image == left image, so every level of the two pyramids is equal and a right
    keypoint one level-pixel left of the left keypoint is an exact match (SAD 0) at shift +1. Every
    probe whose candidate must be found is therefore `accepted` -- a kernel that misses the candidate
    writes -1 instead -- and every probe whose candidate must be refused would be accepted if it were
    taken. 64 level-0 matches with SAD 40 in columns >= 320, outside every probe's disparity window,
    hold the median at 40 so that the SAD-0 matches survive it.

    Rows (every block of probes is more than two of the widest spans from the next): 0 and rows-1
    span edges whose windows cannot fit (see below) | a row near 6 reached by a span with minr = -1 |
    48, 72.75 span edges | 96, 120 octave filter | 144, 168, 192 ties | 216 Hamming thresholds |
    240 candidate counts | 264 an empty row | 288 disparity window.

    A left keypoint on row 0 or rows-1 has its window centre within a pixel of the level's edge, so
    it always ends in `window_off_image` whether or not its candidate was found: those probes name
    the reference's winner only, and nothing the kernels return can observe them. The packed int16
    minr < 0, maxr >= rows and the bucket clamp are observed by the minr = -1 probe here and by
    clamp_case()."""
    assert rows >= 400 and cols >= 528 and nlevels >= 7
    b = Builder(name, sf, nlevels, rows, cols, seed=7, shift=0)
    top = nlevels - 1

    def level_x(o, u):
        return int(np.floor(F(F(u) * b.inv[o]) + 0.5))

    def coords(o, u, back=1.0):
        """Left x a little right of level column xl, right x `back` level columns left of it."""
        xl = level_x(o, u)
        s, inv = b.scale[o], b.inv[o]
        uL, uR = F(s * F(xl + 0.3)), F(s * F(xl - back))
        assert np.floor(F(uL * inv) + 0.5) == xl and np.floor(F(uR * inv) + 0.5) == xl - back
        assert 0 <= uL - uR < 32
        return uL, uR

    def fits(o, vL):
        h = level_shape(rows, cols, b.inv[o])[0]
        return 5 <= np.floor(F(F(vL) * b.inv[o]) + 0.5) <= h - 6

    def probe(ol, vL, orr, yR, u, found, d=10, refused="orb_dist"):
        uL, uR = coords(ol, u)
        iL, iR = b.pair(uL, vL, ol, uR, yR, orr, d=d)
        if found and fits(ol, vL):
            b.want(iL, winner=iR, dist=d, outcome="accepted", shift=1, sad=0)
        elif found:
            b.want(iL, winner=iR, dist=d, outcome="window_off_image")
        else:
            b.want(iL, winner=-1, dist=100)
            if refused:
                b.want(iL, outcome=refused)
        return iL, iR

    k = 0
    full_band = ulp_close = 0
    for vL in (0.0, 48.0, 72.75, float(rows - 1)):
        v = int(vL)
        for o in (0, 1, top):
            r = F(F(2.0) * b.scale[o])
            y_hi = last_y_reaching_from_below(v, r)
            y_lo = first_y_reaching_from_above(v, r)
            # y -+ r within an ulp of y of the integer where the span test flips
            assert abs(F(up(y_hi) - r) - (v + 1)) <= np.spacing(y_hi) and np.floor(F(up(y_hi) - r)) == v + 1
            assert abs(F(down(y_lo) + r) - (v - 1)) <= np.spacing(abs(y_lo)) and np.ceil(F(down(y_lo) + r)) == v - 1
            ulp_close += 2
            # the bucket row of y_lo is the full band distance ceil(r) + 1 above v
            assert np.floor(y_lo) == v - (int(np.ceil(r)) + 1)
            full_band += 1
            for y, reach in ((y_hi, True), (up(y_hi), False), (y_lo, True), (down(y_lo), False)):
                probe(o, vL, o, y, 60.0 + 4 * (k % 40), reach, refused=None)
                k += 1
    assert full_band == 12 and ulp_close == 24
    # a span that starts at row -1 (packed as 0xffff) and ends on the row of a window that fits
    for o in range(1, nlevels):
        r = F(F(2.0) * b.scale[o])
        y = F(r - F(0.06))
        maxr = int(np.ceil(F(y + r)))
        if fits(o, maxr + 0.8):
            break
    assert np.floor(F(y - r)) == -1 and fits(o, maxr + 0.8)
    iL, iR = probe(o, maxr + 0.8, o, y, 230.0, True)
    assert b.expect[iL]["outcome"] == "accepted"
    mid = 3
    for v, probes in ((96.0, ((0, 1, True), (0, 2, False), (top, top - 1, True), (top, top - 2, False))),
                      (120.0, ((mid, mid - 1, True), (mid, mid + 1, True), (mid, mid - 2, False),
                               (mid, mid + 2, False)))):
        for s, (ol, orr, ok) in enumerate(probes):
            probe(ol, v, orr, v, 60.0 + 50 * s, ok, refused="no_candidate")
    # equal best distance at several iR: the smallest iR sits at row v+1 of octave t, the others one
    # row earlier in every octave of the filter -- earlier in bucket order, later in iR order -- and
    # 12 or more level columns further left, where the SAD sweep cannot reach the exact match
    for v, t in ((144.0, 1), (168.0, 2), (192.0, 3)):
        w = b.new_word()
        uL, uR = coords(2, 120.0)
        iL = b.add_left(uL, v, 2, w)
        first = b.add_right(uR, v + 1, t, flipped(w, range(10)))
        for n, o in enumerate((1, 2, 3, t)):
            _, far = coords(2, 120.0, back=13.0 + 2 * n)
            b.add_right(far, v - 1, o, flipped(w, range(10 * (n + 1), 10 * (n + 2))))
        b.want(iL, winner=first, dist=10, outcome="accepted", shift=1, sad=0)
    for s, d in enumerate((74, 75, 99, 100)):
        iL, iR = probe(0, 216.0, 0, 216.0, 60.0 + 50 * s, d == 74, d=d)
        if d in (75, 99):
            b.want(iL, winner=iR, dist=d)
    # 15, 16, 17 and 33 candidates; the best is the last one in iR order and the only one whose
    # sweep reaches the match
    for s, n in enumerate((15, 16, 17, 33)):
        xl = 60 + 50 * s
        w = b.new_word()
        iL = b.add_left(xl + 0.3, 240.0, 0, w)
        for c in range(n - 1):
            b.add_right(xl - 12 - (c % 19) - 0.25 * (c // 19), 240.0, 0, flipped(w, range(60 + c % 9)))
        iR = b.add_right(xl - 1.0, 240.0, 0, flipped(w, range(20)))
        b.want(iL, winner=iR, dist=20, outcome="accepted", shift=1, sad=0)
    iL = b.add_left(100.0, 264.0, 0, b.new_word())
    b.want(iL, winner=-1, dist=100, outcome="no_row")
    # disparity window [uL - 32, uL], both ends inclusive. At the lower end the left content is
    # pasted 30 columns to the left, two shifts right of the candidate: disparity 30.25 - deltaR.
    for s, (lower, inside) in enumerate(((True, True), (True, False), (False, True), (False, False))):
        uL = F(60.25 + 50 * s)
        if lower:
            uR = F(uL - 32) if inside else down(F(uL - 32))
            b.paste(288, int(uL) - 32, 30)
        else:
            uR = uL if inside else up(uL)
        iL, iR = b.pair(uL, 288.0, 0, uR, 288.0, 0)
        if inside:
            b.want(iL, winner=iR, dist=10, outcome="accepted", shift=2 if lower else 0, sad=0)
        else:
            b.want(iL, winner=-1, dist=100, outcome="no_candidate")
    for i in range(64):
        x, y = 320 + 12 * (i % 16), 150 + 12 * (i // 16)
        iL, iR = b.pair(x + 0.3, y, 0, x - 1.0, y, 0, word=hadamard(255 - i % 16))
        b.inject(y, x, BALLAST_SAD)
        b.want(iL, winner=iR, outcome="accepted", shift=1, sad=BALLAST_SAD)
    return b.done()


def clamp_case():
    """Scale factor 3, two levels: a level-1 right keypoint spans 6 rows each way, enough to reach a
    level-0 window that still fits from outside the image. Right y = rows + 0.5 covers row rows-6
    (maxr = rows + 7 >= rows, bucket row clamped to rows-1); right y = -0.5 covers row 5 (minr = -7,
    bucket row clamped to 0). One row further out each way, the span misses."""
    R, C = 192, 256
    b = Builder("clamp_scale3", 3.0, 2, R, C, seed=15, shift=0)
    r = F(F(2.0) * b.scale[1])
    assert r == 6
    for x, vL, y, reach in ((60, R - 6.0, R + 0.5, True), (100, R - 7.0, R + 0.5, False),
                            (140, 5.0, -0.5, True), (180, 7.0, -0.5, False)):
        assert (np.floor(F(F(y) - r)) <= vL <= np.ceil(F(F(y) + r))) == reach
        iL, iR = b.pair(x + 0.3, vL, 0, x - 1.0, y, 1)
        if reach:
            b.inject(int(vL), x, 9 + x // 40)
            b.want(iL, winner=iR, dist=10, outcome="accepted", shift=1, sad=9 + x // 40)
        else:
            b.want(iL, winner=-1, dist=100)
    return b.done()


def mb_zero_case():
    """mb = 0: maxD = +inf, minU = -inf; only uR <= uL bounds the window. The match is pasted two
    shifts right of a candidate 88 columns left of uL."""
    b = Builder("mb_zero", 1.2, 1, 64, 128, mbf=16.0, mb=0.0, seed=11)
    b.paste(30, 12, 86)
    iL, iR = b.pair(100.0, 30.0, 0, 12.0, 30.0, 0)
    b.inject(30, 100, 9)
    b.want(iL, winner=iR, dist=10, outcome="accepted", shift=2, sad=9)
    iL, iR = b.pair(60.0, 50.0, 0, up(F(60.0)), 50.0, 0)
    b.want(iL, winner=-1, dist=100, outcome="no_candidate")
    return b.done()


# ---- window placement ---------------------------------------------------------------------------
def placement_case():
    """Level 0 of a one-level pyramid, right[x] = left[x + 3]. Windows one pixel inside and one
    pixel outside every reachable image edge, and coordinates at .5 (round half away from zero)."""
    R, C = 96, 160
    b = Builder("placement", 1.2, 1, R, C, seed=21, shift=3)
    sad = iter(range(12, 40))

    def ok(xl, yl, xr, shift=0):
        s = next(sad)
        iL, iR = b.pair(xl, yl, 0, xr, yl, 0)
        b.inject(int(np.floor(yl + 0.5)), int(np.floor(xl + 0.5)), s)
        b.want(iL, winner=iR, outcome="accepted", shift=shift, sad=s)

    def off(xl, yl, xr):
        iL, iR = b.pair(xl, yl, 0, xr, yl, 0)
        b.want(iL, winner=iR, outcome="window_off_image")

    ok(13.0, 20.0, 10.0)             # xR0 = 10
    off(12.0, 40.0, 9.0)             # xR0 = 9
    ok(C - 9.0, 20.0, C - 12.0)      # xR0 = cols - 12: endu = cols - 1
    off(C - 8.0, 40.0, C - 11.0)     # xR0 = cols - 11: endu = cols
    ok(60.0, 5.0, 57.0)              # yL = 5
    off(100.0, 4.0, 97.0)            # yL = 4
    ok(60.0, R - 6.0, 57.0)          # yL = rows - 6
    off(100.0, R - 5.0, 97.0)        # yL = rows - 5
    ok(C - 6.0, 60.0, C - 12.0, 3)   # xL = cols - 6; the match is 3 shifts right of the candidate
    off(C - 5.0, 76.0, C - 12.0)     # xL = cols - 5
    ok(70.5, 30.5, 67.5)             # round(70.5) = 71, round(30.5) = 31, round(67.5) = 68
    return b.done()


def align_case(level):
    """All 16 combinations of (xL - 5) mod 4 and (xR0 - 10) mod 4 -- the byte offsets of the two
    window rows in their dwords -- on level 0, or on the resized level 1 of a two-level pyramid."""
    R, C = 96, 160
    b = Builder(f"align_level{level}", 1.2, level + 1, R, C, seed=31 + level, shift=3)
    s, inv = b.scale[level], b.inv[level]
    n = 0
    residues = set()
    for a in range(4):
        for d in (3, 4, 5, 6):
            if level == 0:
                xs, ys = 32 + 32 * (d - 3) + a, 14 + 20 * a
            else:
                xs, ys = 28 + 24 * (d - 3) + a, 12 + 16 * a
            x, y, xr = F(xs * s), F(ys * s), F((xs - d) * s)
            assert np.floor(F(x * inv) + 0.5) == xs and np.floor(F(xr * inv) + 0.5) == xs - d
            assert np.floor(F(y * inv) + 0.5) == ys
            residues.add(((xs - 5) % 4, (xs - d - 10) % 4))
            iL, iR = b.pair(x, y, level, xr, y, level)
            if level == 0:
                b.inject(ys, xs, 10 + n)
                b.want(iL, winner=iR, outcome="accepted", shift=d - 3, sad=10 + n)
            else:
                b.want(iL, winner=iR, swept=True)
            n += 1
    assert len(residues) == 16
    return b.done()


# ---- SAD arithmetic -----------------------------------------------------------------------------
def sad_binary_case():
    """0 / 255 windows on a flat background: per-pixel terms of 510, shift totals of 61,200 (the
    largest possible is 121 * 510 = 61,710), totals on both sides of 2^15, and deltaR = 0.5."""
    b = Builder("sad_binary", 1.2, 1, 96, 160, flat=128)
    Lm, Rm = b.left, b.right
    # every non-centre pixel 255 against 0, centres 0 against 255: 120 * 510 at shift 0
    x, y = 40, 24
    Lm[y - 5:y + 6, x - 5:x + 6] = 255
    Lm[y, x] = 0
    Rm[y - 5:y + 6, x - 10:x + 11] = 0
    Rm[y, x] = 255
    iL, iR = b.pair(x, y, 0, x, y, 0)
    b.want(iL, winner=iR, outcome="min_at_shift_edge", sads=[30345] * 5 + [61200] + [30345] * 5)
    # checkerboard against its inverse: odd shifts coincide (0), even shifts oppose (60 * 510)
    x, y = 100, 24
    for dy in range(-5, 6):
        for dx in range(-10, 11):
            if abs(dx) <= 5:
                Lm[y + dy, x + dx] = 255 if (dy + dx) % 2 else 0
            Rm[y + dy, x + dx] = 0 if (dy + dx) % 2 else 255
    iL, iR = b.pair(x, y, 0, x, y, 0)
    b.want(iL, winner=iR, outcome="min_at_shift_edge", sads=[0, 30600] * 5 + [0])
    # left 255 around a 0 centre; right 255 with 9 zeros only shift -5 sees and 8 only +5 sees:
    # 32,895 (> 2^15), nine times 30,600, then 32,640 (< 2^15). First minimum at -4, deltaR = 0.5.
    x, y = 40, 56
    Lm[y - 5:y + 6, x - 5:x + 6] = 255
    Lm[y, x] = 0
    Rm[y - 5:y + 6, x - 10:x + 11] = 255
    Rm[y - 5:y + 4, x - 10] = 0
    Rm[y - 5:y + 3, x + 10] = 0
    iL, iR = b.pair(x, y, 0, x, y, 0)
    b.want(iL, winner=iR, outcome="accepted", shift=-4, sads=[32895] + [30600] * 9 + [32640])
    return b.done()


def sad_texture_case():
    """Textured windows with the match pasted at a chosen shift: minima at -5 / +5 (rejected) and
    -4 / +4 (kept), a flat pair, two equal minima, and the three disparity outcomes."""
    R, C = 128, 256
    b = Builder("sad_texture", 1.2, 1, R, C, seed=41)

    def probe(x, y, c, s):  # candidate c columns left of uL, match pasted at shift s
        b.paste(y, x - c, c - s)
        return b.pair(x, y, 0, x - c, y, 0)

    for x, s in ((40, -5), (104, 5)):
        iL, iR = probe(x, 16, 8, s)
        b.want(iL, winner=iR, outcome="min_at_shift_edge", shift=s)
    for x, s, sad in ((168, -4, 11), (232, 4, 12)):
        iL, iR = probe(x, 16, 8, s)
        b.inject(16, x, sad)
        b.want(iL, winner=iR, outcome="accepted", shift=s, sad=sad)
    # flat pair: every SAD is 0, the first of them is shift -5
    b.left[33:48, 16:65] = 100
    b.right[33:48, 16:65] = 100
    iL, iR = b.pair(40, 40, 0, 32, 40, 0)
    b.want(iL, winner=iR, outcome="min_at_shift_edge", sads=[0] * 11)
    # columns of period 7 in both images: the candidate 3 left of uL matches at +3 and at -4
    for xx in range(90, 151):
        b.left[33:48, xx] = b.left[33:48, 90 + (xx - 90) % 7]
    b.right[33:48, 90:151] = b.left[33:48, 90:151]
    iL, iR = b.pair(120, 40, 0, 117, 40, 0)
    b.inject(40, 120, 13)
    b.want(iL, winner=iR, outcome="accepted", shift=-4, sad=13)
    # mirror-symmetric about x = 200, right = left, candidate at uL: d1 == d3, disparity exactly 0
    for kk in range(1, 21):
        b.left[33:48, 200 + kk] = b.left[33:48, 200 - kk]
    b.right[33:48, 180:221] = b.left[33:48, 180:221]
    iL, iR = b.pair(200, 40, 0, 200, 40, 0)
    b.inject(40, 200, 14, symmetric=True)
    b.want(iL, winner=iR, outcome="accepted_zero_disparity", shift=0, sad=14)
    # candidate at uR == uL, the match two shifts right of it: bestuR > uL
    iL, iR = probe(40, 64, 0, 2)
    b.want(iL, winner=iR, outcome="disparity_negative", shift=2)
    # candidate at uR == uL - maxD (inside the window), the match two shifts left of it
    iL, iR = probe(120, 64, 32, -2)
    b.want(iL, winner=iR, outcome="disparity_ge_maxD", shift=-2)
    return b.done()


# ---- median filter ------------------------------------------------------------------------------
TH_FACTOR = F(F(1.5) * F(1.4))


def median_case(name, sads, seed):
    """One left keypoint per entry of `sads` on a 12-pixel grid, right[x] = left[x + 3], the SAD at
    the matching shift set by injection; None makes a keypoint whose best distance is 80."""
    per_row = 20
    nrow = (len(sads) + per_row - 1) // per_row
    R, C = max(64, 32 + 12 * (nrow - 1)), 272
    b = Builder(name, 1.2, 1, R, C, seed=seed, shift=3)
    kept = sorted(s for s in sads if s is not None)
    th = F(TH_FACTOR * F(kept[len(kept) // 2])) if kept else None
    for i, s in enumerate(sads):
        x, y = 16 + 12 * (i % per_row), 16 + 12 * (i // per_row)
        w = hadamard(1 + i % per_row)  # rows are further apart than any span
        if s is None:
            iL, iR = b.pair(x, y, 0, x - 3, y, 0, d=80, word=w)
            b.want(iL, dist=80, outcome="orb_dist")
            continue
        iL, iR = b.pair(x, y, 0, x - 3, y, 0, word=w)
        b.inject(y, x, s)
        b.want(iL, winner=iR, shift=0, sad=s, outcome="accepted" if F(s) < th else "median_rejected")
    return b.done()


def median_cases():
    mix = np.random.RandomState(5)
    runs = [50] * 10 + [100] * 20 + [209, 210, 211] + [120] * 7
    mix.shuffle(runs)
    big = [255] * 150 + [256] + [257] * 147 + [537, 538]
    mix.shuffle(big)
    return [
        median_case("median_M0", [None, None, None], 51),
        median_case("median_M1_sad0", [0], 52),
        median_case("median_M1_sad7", [7], 53),
        median_case("median_M2", [10, 30], 54),
        median_case("median_odd", [22, 1, 21, 2, 10, 3, 20], 55),          # median 10, threshold 21
        median_case("median_even", [22, 1, 21, 2, 10, 9, 3, 20], 56),      # element 4 of 8 is 10, not 9
        median_case("median_equal_runs", runs, 57),                        # rank 20 inside twenty 100s
        median_case("median_high_byte", big, 58),                          # M = 300: 255 | 256 | 257
    ]


# ---- batches ------------------------------------------------------------------------------------
def batch_pairs():
    """Five pairs of one batch (two levels, 96 x 160): 15, 16 and 17 left keypoints, a pair without
    right keypoints, a pair without left keypoints. The last pair is the one whose right image is
    the last of the batch; its last left keypoint has its window on the last rows of the last level
    with the right sweep ending at the last column the reference allows."""
    R, C = 96, 160
    out = []
    for p, (nl, nr) in enumerate(((15, 15), (16, 16), (5, 0), (0, 5), (16, 16))):
        b = Builder(f"batch_pair{p}", 1.2, 2, R, C, seed=61 + p, shift=3)
        for i in range(max(nl, nr)):
            x, y = 20 + 24 * (i % 6), 14 + 14 * (i // 6)
            w = b.new_word()
            if i < nl:
                iL = b.add_left(x, y, 0, w)
            if i < nr:
                iR = b.add_right(x - 3, y, 0, flipped(w, range(10)))
            if i < nl and i < nr:
                b.inject(y, x, 10 + i)
                b.want(iL, winner=iR, outcome="accepted", shift=0, sad=10 + i)
            elif i < nl:
                b.want(iL, winner=-1, outcome="no_row")
        if p == 4:
            h1, w1 = level_shape(R, C, b.inv[1])
            s1, i1 = b.scale[1], b.inv[1]
            ys, xr, xl = h1 - 6, w1 - 12, w1 - 9
            y, ul, ur = F(ys * s1), F(xl * s1), F(xr * s1)
            assert np.floor(F(y * i1) + 0.5) == ys and np.floor(F(ul * i1) + 0.5) == xl
            assert np.floor(F(ur * i1) + 0.5) == xr
            iL, iR = b.pair(ul, y, 1, ur, y, 1)
            b.want(iL, winner=iR, swept=True)
        out.append(b.done())
    return out


# ---- the cases ----------------------------------------------------------------------------------
# 32 levels at 1.05 need 62 * 1.05^31 = 282 rows, and the extractor needs every level's
# (width - 32) / (height - 32) to round to at least 1. nlevels * (rows + 1) is 16,416 at 512 rows
# (one bucket per row for all octaves) and exactly 16,384 at 511 rows: the last shape with a bucket
# per octave and row, and the one whose row table needs more than 64 KiB of LDS.
def single_cases():
    return [
        band_case("band_8_levels", 1.2, 8, 400, 528),
        band_case("band_row_only_table", 1.05, 32, 512, 528),
        band_case("band_table_at_16384", 1.05, 32, 511, 528),
        clamp_case(),
        mb_zero_case(),
        placement_case(),
        align_case(0),
        align_case(1),
        sad_binary_case(),
        sad_texture_case(),
    ] + median_cases()


def check_expect(case, ref):
    """Assert every expectation of `case` on a stereo_ref result."""
    for iL, e in case.expect.items():
        tag = f"{case.name}[{iL}]"
        if "outcome" in e:
            assert ref["outcome"][iL] == e["outcome"], f"{tag}: {ref['outcome'][iL]}, named {e['outcome']}"
        if "winner" in e:
            assert ref["best_iR"][iL] == e["winner"], f"{tag}: iR {ref['best_iR'][iL]}, named {e['winner']}"
        if "dist" in e:
            assert ref["best_dist"][iL] == e["dist"], f"{tag}: distance {ref['best_dist'][iL]}"
        if "shift" in e:
            assert ref["best_shift"][iL] == e["shift"], f"{tag}: shift {ref['best_shift'][iL]}"
        if "sad" in e:
            got = ref["sads"][iL][5 + ref["best_shift"][iL]]
            assert got == e["sad"], f"{tag}: SAD {got}, named {e['sad']}"
        if "sads" in e:
            assert ref["sads"][iL].tolist() == list(e["sads"]), f"{tag}: SADs {ref['sads'][iL].tolist()}"
        if e.get("swept"):
            assert ref["sads"][iL][0] >= 0, f"{tag}: {ref['outcome'][iL]}, the sweep did not run"
