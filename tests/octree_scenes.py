"""Key sets for DistributeOctTree, fed through the public call as images of isolated dots.

On a flat background b a single pixel of value b + r + 1 (or b - r - 1) is a FAST corner of response
r and nothing around it is: its 16-pixel ring is b everywhere, and a ring that holds the dot has one
differing pixel where a corner needs nine in a row. With dots at Chebyshev distance >= 4 no ring holds
two dots, so every dot with r >= iniThFAST is exactly one candidate. The cell detector looks 3 px
inside each cell's region, so a candidate's border-relative coordinates (level coordinates minus 16)
lie in [3, w - 4] x [3, h - 4], w x h being the border area (cols - 32, rows - 32). With one pyramid
level the level's budget is nfeatures, so any such key set and any N reach DistributeOctTree.

Every hand-built Scene carries the survivors it must give, written out, in list order, and the
stop rule that ends it; the derivations are beside each case. Notation: a node is
[x0, x1) x [y0, y1); DivideNode cuts it at mx = x0 + ceil((x1 - x0) / 2), my likewise, into
n1 (x < mx, y < my), n2 (x >= mx, y < my), n3 (x < mx, y >= my), n4; non-empty children are pushed
to the FRONT of the list in the order n1..n4, then the parent is erased. A pass visits the nodes that
were in the list at its start, front to back. The cases on equal responses list their keys in
candidate order: cell by cell (cells of about 30 px, row-major), and by (y, x) inside a cell.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

import octree_ref as O

Key = Tuple[int, int, int]
BORDER = 16  # EDGE_THRESHOLD - 3: level coordinate = border-relative coordinate + 16


@dataclass
class Scene:
    name: str
    shape: Tuple[int, int]          # image rows, cols
    keys: List[Key]                 # border-relative (x, y, response)
    N: int
    expect: Optional[List[Key]] = None   # hand-built scenes: the survivors in list order
    stop: Optional[str] = None
    trace: Dict[str, int] = field(default_factory=dict)  # Trace fields the scene claims
    tie: bool = False               # the one scene that pins the equal-size order
    background: int = 60

    @property
    def w(self) -> int:
        return self.shape[1] - 2 * BORDER

    @property
    def h(self) -> int:
        return self.shape[0] - 2 * BORDER

    def image(self) -> np.ndarray:
        return dot_image(self.shape, self.keys, self.background)


def dot_image(shape, keys, background=60) -> np.ndarray:
    """The image whose level-0 FAST candidates are exactly `keys` (border-relative x, y, response)."""
    rows, cols = shape
    w, h = cols - 2 * BORDER, rows - 2 * BORDER
    img = np.full(shape, background, np.uint8)
    pts = np.array([(k[0], k[1]) for k in keys], np.int64).reshape(-1, 2)
    for x, y, r in keys:
        assert 3 <= x <= w - 4 and 3 <= y <= h - 4, f"dot ({x}, {y}) outside the detector's area {w}x{h}"
        assert 20 <= r <= 254, f"response {r}"
        v = background + r + 1 if background + r + 1 <= 255 else background - r - 1
        assert 0 <= v <= 255, f"response {r} does not fit around background {background}"
        img[y + BORDER, x + BORDER] = v
    if len(pts) > 1:
        order = np.lexsort((pts[:, 1], pts[:, 0]))
        p = pts[order]
        for i in range(len(p)):  # dots sorted by x: only those within 3 columns can be too close
            j = i + 1
            while j < len(p) and p[j, 0] - p[i, 0] < 4:
                assert abs(p[j, 1] - p[i, 1]) >= 4, f"dots {p[i].tolist()} and {p[j].tolist()} closer than 4 px"
                j += 1
    return img


# --------------------------------------------------------------------------------------------------
# Hand-built cases. S64 is a 96 x 96 image: border area 64 x 64, nIni = round(1.0) = 1, root
# [0,64) x [0,64) cut at (32, 32) into Q1 [0,32)x[0,32), Q2 [32,64)x[0,32), Q3 [0,32)x[32,64), Q4.
S64 = (96, 96)
S65 = (97, 97)  # border area 65 x 65: root cut at ceil(32.5) = 33

# The keys shared by the stop-rule cases: a, b, f (and g) in Q1, one per child of Q1 (cut at 16, 16);
# c alone in Q2; d, e in Q4, in n1 and n2 of Q4 (cut at 48, 48).
_a, _b, _f, _g = (8, 8, 50), (24, 8, 60), (8, 24, 55), (24, 24, 52)
_c, _d, _e = (40, 8, 45), (40, 40, 70), (56, 40, 65)
# After pass 1 of [a, b, c, f, d, e] the list is [Q4{d,e}, Q2{c}, Q1{a,b,f}]: size 3, nToExpand 2.
_STOP_KEYS = [_a, _b, _c, _f, _d, _e]

_INI8_B = [32, 63, 94, 125, 157, 188, 219]        # first x owned by initial node 1..7 of a 250-wide area
_INI9_B = [34, 67, 100, 134, 167, 200, 234, 267]  # ... by node 1..8 of a 300-wide area


def _boundary_sweep(firsts):
    """Five dots over four rows around each first-owned x B: (B-2, 30) and (B-1, 40) belong to the
    node on the left, (B, 60), (B+1, 50), (B+2, 35) to the node on the right."""
    keys = []
    for b in firsts:
        keys += [(b - 2, 3, 30), (b + 2, 3, 35), (b - 1, 7, 40), (b, 11, 60), (b + 1, 15, 50)]
    return keys


def _sweep_expect(firsts):
    # Every initial node is about 32 wide and 32 high and is cut near (lo + 16, 16); all dots have
    # y < 16. Node i holds the right-hand group of boundary i in its n1 and the left-hand group of
    # boundary i + 1 in its n2. One pass (N = 1) creates, in order, n2 of node 0, n1 and n2 of node 1,
    # ..., n1 of the last node; pushed to the front, the list is that order reversed, and each child's
    # best key is (B, 60) for a right-hand group and (B - 1, 40) for a left-hand one.
    out = []
    for b in reversed(firsts):
        out += [(b, 11, 60), (b - 1, 7, 40)]
    return out


def hand_scenes() -> List[Scene]:
    P, PS, RN, RS = O.PASS_N, O.PASS_STALL, O.REFINE_N, O.REFINE_STALL
    s = []
    # ---- 1. a key on a split line --------------------------------------------------------------
    # (32, 8) has x == mx = 32: not < 32, so it goes right, to n2 = Q2 with (40, 12, 60). Pass 1
    # leaves [Q2{(32,8),(40,12)}, Q1{(28,8)}], size 2 >= N = 1.
    s.append(Scene("split_x_equal_even", S64, [(28, 8, 40), (32, 8, 50), (40, 12, 60)], 1,
                   [(40, 12, 60), (28, 8, 40)], P, dict(nIni=1, passes=1, rounds=0)))
    # (8, 32) has y == my = 32: it goes down, to n3 = Q3 with (12, 40, 60): [Q3, Q1{(8,28)}].
    s.append(Scene("split_y_equal_even", S64, [(8, 28, 40), (8, 32, 50), (12, 40, 60)], 1,
                   [(12, 40, 60), (8, 28, 40)], P, dict(nIni=1, passes=1, rounds=0)))
    # Width 65: half = ceil(32.5) = 33, so (32, 8) is left (n1, with (20, 12)) and (36, 8) alone in
    # n2: [n2{(36,8)}, n1{(32,8),(20,12)}]. A floor half (32) would send (32, 8) right.
    s.append(Scene("split_x_odd_ceil", S65, [(32, 8, 50), (36, 8, 60), (20, 12, 40)], 1,
                   [(36, 8, 60), (32, 8, 50)], P, dict(nIni=1, passes=1)))
    # The same on y: (8, 32) is above my = 33 (n1, with (12, 20)), (8, 36) alone in n3.
    s.append(Scene("split_y_odd_ceil", S65, [(12, 20, 40), (8, 32, 50), (8, 36, 60)], 1,
                   [(8, 36, 60), (8, 32, 50)], P, dict(nIni=1, passes=1)))
    # Width 65 again, a key ON the odd cut: (33, 20) has x == mx = 33 and goes right, to n2 with
    # (44, 8, 30); (28, 12, 40) stays alone in n1: [n2{(44,8),(33,20)}, n1{(28,12)}].
    s.append(Scene("split_x_equal_odd", S65, [(44, 8, 30), (28, 12, 40), (33, 20, 50)], 1,
                   [(33, 20, 50), (28, 12, 40)], P, dict(nIni=1, passes=1)))

    # A node one pixel wide. 151 x 92 image, area 60 x 119, nIni = round(0.504) = 1. One key peels off
    # in every pass, so the list keeps growing and the pair (29,8), (29,12) is followed down:
    #   pass 1 root cut (30,60):            [n4{(40,70)}, n1{the other five}]
    #   pass 2 [0,30)x[0,60) cut (15,30):   [n2{four}, n1{(8,20)}, (40,70)]
    #   pass 3 [15,30)x[0,30) cut (23,15):  [n2{(24,4),(29,8),(29,12)}, n1{(18,5)}, ...]
    #   pass 4 [23,30)x[0,15) cut (27,8):   [n4{(29,8),(29,12)}, n1{(24,4)}, ...]
    #   pass 5 [27,30)x[8,15), 3 wide, cut (27 + ceil(1.5), 8 + ceil(3.5)) = (29,12): (29,8) in n2,
    #          (29,12) in n4, both [29,30) wide;  pass 6 divides nothing.
    s.append(Scene("width_1_after_repeated_splits", (151, 92),
                   [(40, 70, 50), (8, 20, 55), (18, 5, 60), (24, 4, 65), (29, 8, 70), (29, 12, 75)], 20,
                   [(29, 12, 75), (29, 8, 70), (24, 4, 65), (18, 5, 60), (8, 20, 55), (40, 70, 50)], PS,
                   dict(nIni=1, passes=6, rounds=0, min_w=1)))

    # ---- 2. initial nodes ----------------------------------------------------------------------
    # 140 x 100 image, area 68 x 108: nIni = round(0.63) = 1. The root [0,68)x[0,108) is cut at
    # (34, 54): x = 34 equals the cut and goes right, so all three keys (y < 54) land in n2. The list
    # stays at one node: no progress, and the best of the three survives.
    s.append(Scene("ini1_all_in_one_child", (140, 100), [(34, 24, 50), (38, 24, 60), (54, 44, 70)], 50,
                   [(54, 44, 70)], PS, dict(nIni=1, passes=1, rounds=0)))
    # 100 x 140 image, area 108 x 68: nIni = round(1.59) = 2, hX = 54. x = 54 is owned by node 1
    # (54 / 54 = 1), alone there (bNoMore). Node 0 [0,54)x[0,68) is cut at (27, 34): both its keys go
    # to n2, so the list [n2{(34,24),(38,24)}, node1] is as long as before: no progress.
    s.append(Scene("ini2_no_progress_multi_key", (100, 140), [(34, 24, 50), (38, 24, 60), (54, 44, 70)], 50,
                   [(38, 24, 60), (54, 44, 70)], PS, dict(nIni=2, passes=1, rounds=0)))
    # Area 48 x 32: ratio 1.5 rounds away from zero to nIni = 2, hX = 24. One key per node, both
    # bNoMore: nothing to divide, list [node0, node1]. (Truncation would make one root and give the
    # opposite order.)
    s.append(Scene("ini_round_1p5_up", (64, 80), [(8, 8, 50), (28, 8, 60)], 5,
                   [(8, 8, 50), (28, 8, 60)], PS, dict(nIni=2, passes=1)))
    # Area 80 x 32: ratio 2.5 rounds to nIni = 3, hX = 26.67: owners of x = 8, 32, 60 are 0, 1, 2.
    s.append(Scene("ini_round_2p5_up", (64, 112), [(8, 8, 50), (32, 8, 60), (60, 8, 70)], 5,
                   [(8, 8, 50), (32, 8, 60), (60, 8, 70)], PS, dict(nIni=3, passes=1)))
    # Area 250 x 32: nIni = round(7.81) = 8 (the last count the kernel places by its threshold table),
    # hX = 31.25. (int)(hX * i) and x / hX disagree at x = 31, 62, 93, 156, 187, 218: each is the last
    # x owned by the node on its left although that node's UR.x equals it. All of them are occupied.
    s.append(Scene("ini8_boundary_sweep", (64, 282), _boundary_sweep(_INI8_B), 1, _sweep_expect(_INI8_B), P,
                   dict(nIni=8, passes=1, nodes=14)))
    # Area 300 x 32: nIni = round(9.38) = 9 (the first count placed by the float division),
    # hX = 33.33...; the two forms disagree at x = 33, 66, 133, 166, 233, 266, all occupied.
    s.append(Scene("ini9_boundary_sweep", (64, 332), _boundary_sweep(_INI9_B), 1, _sweep_expect(_INI9_B), P,
                   dict(nIni=9, passes=1, nodes=16)))
    # Area 384 x 32: nIni = 12, hX = 32. Nodes 1 and 11 hold one key (bNoMore), node 6 two, the other
    # nine none (erased): [node1, node6, node11]. Node 6 [192,224)x[0,32) is cut at (208, 16): both
    # keys in n1, pushed to the front: [n1{(200,8),(204,12)}, node1, node11], no progress.
    s.append(Scene("ini12_empty_nodes_erased", (64, 416), [(40, 8, 50), (200, 8, 60), (204, 12, 55), (380, 8, 70)], 10,
                   [(200, 8, 60), (40, 8, 50), (380, 8, 70)], PS, dict(nIni=12, passes=1)))
    # Area 1920 x 30: nIni = 64, the most the library accepts; hX = 30. Owners 0, 33, 33, 63. Node 33
    # [990,1020)x[0,30) is cut at (1005, 15): both keys in n1.
    s.append(Scene("ini64_upper_limit", (62, 1952), [(8, 8, 50), (1000, 8, 60), (1004, 12, 55), (1916, 8, 70)], 10,
                   [(1000, 8, 60), (8, 8, 50), (1916, 8, 70)], PS, dict(nIni=64, passes=1)))

    # ---- 3. stop rules at equality -------------------------------------------------------------
    # One key in each of Q1, Q2, Q3: pass 1 pushes n1, n2, n3 -> [Q3, Q2, Q1], size 3 == N.
    s.append(Scene("stop_exactly_N_after_pass", S64, [(8, 8, 50), (40, 8, 60), (8, 40, 70)], 3,
                   [(8, 40, 70), (40, 8, 60), (8, 8, 50)], P, dict(passes=1, rounds=0, overshoot=0)))
    # One key per quadrant and N = 1: the first pass is unchecked and gives 4 nodes = N + 3.
    s.append(Scene("stop_overshoot_3_N1", S64, [(8, 8, 50), (40, 8, 60), (8, 40, 70), (40, 40, 65)], 1,
                   [(40, 40, 65), (8, 40, 70), (40, 8, 60), (8, 8, 50)], P, dict(passes=1, overshoot=3)))
    # _STOP_KEYS, N = 9: size + 3 * nToExpand = 3 + 6 == N does NOT start the refinement. Pass 2
    # walks [Q4, Q2, Q1]: Q4 -> [e, d, Q2, Q1]; Q2 is bNoMore; Q1 -> [f, b, a, e, d, Q2], size 6 < 9,
    # nToExpand 0. Pass 3 divides nothing: no progress.
    s.append(Scene("trigger_equal_N_no_refinement", S64, _STOP_KEYS, 9,
                   [_f, _b, _a, _e, _d, _c], PS, dict(passes=3, rounds=0)))
    # N = 8: 9 == N + 1 starts it. Sizes differ (Q1 3, Q4 2): Q1 is divided first -> [f, b, a, Q4,
    # Q2], then Q4 -> [e, d, f, b, a, Q2], size 6 < 8. Round 2 has nothing to divide: no progress.
    # The order differs from the full pass above, which walks the list instead of the sizes.
    s.append(Scene("trigger_N_plus_1_refines_by_size", S64, _STOP_KEYS, 8,
                   [_e, _d, _f, _b, _a, _c], RS, dict(passes=1, rounds=2)))
    # N = 5: the refinement divides Q1 -> size 5 == N: break, Q4 is left whole (best key d).
    s.append(Scene("refine_break_exactly_N", S64, _STOP_KEYS, 5,
                   [_f, _b, _a, _d, _c], RN, dict(passes=1, rounds=1, overshoot=0, left_in_round=1)))
    # N = 4: the same division passes N by one.
    s.append(Scene("refine_overshoot_1", S64, _STOP_KEYS, 4,
                   [_f, _b, _a, _d, _c], RN, dict(passes=1, rounds=1, overshoot=1, left_in_round=1)))
    # With g, Q1 holds one key per child; N = 4: size 3 -> 6 = N + 2 in one division.
    s.append(Scene("refine_overshoot_2", S64, [_a, _b, _c, _f, _g, _d, _e], 4,
                   [_g, _f, _b, _a, _d, _c], RN, dict(passes=1, rounds=1, overshoot=2, left_in_round=1)))
    # N above the key count: pass 1 -> [Q4{(40,40)}, Q1{(8,8),(24,8)}]; pass 2 cuts Q1 at 16 ->
    # [(24,8), (8,8), Q4]; pass 3 divides nothing. Every node a singleton.
    s.append(Scene("N_above_key_count", S64, [(8, 8, 50), (24, 8, 60), (40, 40, 70)], 10,
                   [(24, 8, 60), (8, 8, 50), (40, 40, 70)], PS, dict(passes=3, rounds=0, nodes=3)))
    s.append(Scene("one_key", S64, [(20, 20, 50)], 5, [(20, 20, 50)], PS, dict(passes=1, nodes=1)))
    s.append(Scene("no_key", S64, [], 5, [], PS, dict(passes=1, nodes=0)))

    # ---- 4. best key of a node: strict >, first in the node's key order wins ---------------------
    # All keys in Q1 and N = 1: pass 1 leaves [Q1] and its first maximum survives.
    s.append(Scene("best_two_equal_before_weaker", S64, [(20, 8, 80), (8, 12, 40), (12, 20, 80)], 1,
                   [(20, 8, 80)], P, dict(passes=1, nodes=1)))
    s.append(Scene("best_two_equal_after_weaker", S64, [(8, 8, 40), (20, 12, 80), (12, 20, 80)], 1,
                   [(20, 12, 80)], P, dict(passes=1, nodes=1)))
    s.append(Scene("best_three_equal", S64, [(8, 8, 90), (16, 12, 90), (24, 16, 40), (12, 20, 90)], 1,
                   [(8, 8, 90)], P, dict(passes=1, nodes=1)))
    # Input order alternates Q1, Q2, Q1, Q2 (x = 33, 34 are right of the cut at 32 but still in the
    # first FAST cell): the stable partition keeps (8,8) before (12,16) and (33,12) before (34,20).
    s.append(Scene("best_equal_across_partition", S64, [(8, 8, 80), (33, 12, 80), (12, 16, 80), (34, 20, 80)], 2,
                   [(33, 12, 80), (8, 8, 80)], P, dict(passes=1, nodes=2)))

    # ---- 5. refinement order -------------------------------------------------------------------
    # (different sizes: trigger_N_plus_1_refines_by_size above.)
    # THE PROJECT'S DECISION. Q1{a,b} and Q4{d,e} both hold 2 keys; the reference orders
    # them by heap address, the project by creation number: Q4, created later, is divided first ->
    # [e, d, Q2, Q1], size 4 == N: break, Q1 left whole (best key b). The opposite order gives
    # [b, a, d, c].
    s.append(Scene("tie_equal_sizes_creation_order_decision", S64, [_a, _b, _c, _d, _e], 4,
                   [_e, _d, _c, _b], RN, dict(passes=1, rounds=1, overshoot=0, left_in_round=1), tie=True))
    return s


# --------------------------------------------------------------------------------------------------
# Large nodes: k dots of a 4-px lattice packed into initial node 0 of a 120 x 200 image (area
# 168 x 88, nIni 2, node 0 = [0, 84)), one more in node 1, so the first division splits exactly k keys;
# and the full lattice (41 x 21 = 861 dots). Responses are random in 20..254 (dark background).
LARGE_SHAPE = (120, 200)
LARGE_COUNTS = (1, 47, 48, 49, 63, 64, 65, 128, 129)
LARGE_N = (5, 37, 200, 1500, 5000)  # the last two exceed every key count: every node ends a singleton


def _lattice(shape):
    w, h = shape[1] - 2 * BORDER, shape[0] - 2 * BORDER
    return [(x, y) for y in range(3, h - 3, 4) for x in range(3, w - 3, 4)]


def large_scenes() -> List[Scene]:
    out = []
    rng = np.random.default_rng(20240611)
    for k in LARGE_COUNTS + (0,):
        if k:
            side = int(np.ceil(np.sqrt(k)))
            pts = [(3 + 4 * (i % side), 3 + 4 * (i // side)) for i in range(k)] + [(123, 43)]
            assert max(p[0] for p in pts[:-1]) < 84
        else:
            pts = _lattice(LARGE_SHAPE)
        keys = [(x, y, int(r)) for (x, y), r in zip(pts, rng.integers(20, 255, len(pts)))]
        for n in LARGE_N:
            out.append(Scene(f"large_{k or len(pts)}_N{n}", LARGE_SHAPE, keys, n, background=0,
                             trace=dict(max_divided=k) if k > 1 else {}))
    return out


RANDOM_SHAPES = ((100, 140), (140, 100), (97, 141), (101, 250), (120, 200), (64, 282), (64, 332), (62, 1952))
RANDOM_N = (1, 2, 3, 5, 8, 13, 21, 37, 60, 100, 200, 500, 1000, 5000)


def random_scenes(count: int = 40) -> List[Scene]:
    out = []
    rng = np.random.default_rng(77)
    for i in range(count):
        shape = RANDOM_SHAPES[i % len(RANDOM_SHAPES)]
        lat = _lattice(shape)
        p = float(rng.choice([0.03, 0.1, 0.3, 0.6, 1.0]))
        pts = [q for q in lat if rng.random() < p]
        keys = [(x, y, int(r)) for (x, y), r in zip(pts, rng.integers(20, 255, len(pts)))]
        out.append(Scene(f"random_{i}", shape, keys, int(rng.choice(RANDOM_N)), background=0))
    return out
