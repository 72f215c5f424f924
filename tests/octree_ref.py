"""DistributeOctTree in plain Python, from the reference text alone.

A second restatement of ORBextractor::DistributeOctTree (ORBextractor.cc:542-766) and
ExtractorNode::DivideNode (:484-540) that imports nothing from oracle/ and shares no code with it.
The std::list is a Python list whose index 0 is the list's front; every statement of the reference
that decides an integer keeps its float expression, evaluated in numpy float32:

    nIni  = round((float)w / h)                       :546   (C round: halves away from zero)
    hX    = (float)w / nIni                           :548
    UL.x  = (int)(hX * (float)i)                      :558-559
    owner = (size_t)(kp.pt.x / hX)                    :572
    half  = (int)ceil((float)(UR.x - UL.x) / 2)       :486-487

The one thing the text does not fix is the order of equal-size nodes in the refinement's sort, which
compares (size, node address) pairs (:687). `tie` chooses it: "creation" is the project's rule
(ascending creation number stands for ascending address, so the walk from the back of the
sorted vector meets the later-created of two equal nodes first); "reverse" is the opposite order.
"""
import math
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

Key = Tuple[int, int, int]  # (x, y, response), x and y relative to the level's 16-px border

f32 = np.float32

# why the outer loop ended (:672 and :737)
PASS_N = "pass: size >= N"              # after a full pass
PASS_STALL = "pass: size == prevSize"   # a full pass added no node
REFINE_N = "refine: size >= N"          # in or after a refinement round
REFINE_STALL = "refine: size == prevSize"


@dataclass
class Trace:
    nIni: int = 0
    passes: int = 0        # full passes (iterations of the outer loop, :597)
    rounds: int = 0        # refinement rounds (iterations of the inner loop, :679)
    stop: str = ""
    nodes: int = 0         # final list size = number of survivors
    left_in_round: int = 0  # nodes of the last refinement round not divided because of the break (:733)
    overshoot: int = 0     # nodes - N
    min_w: int = 1 << 30   # the narrowest / lowest node that received a key
    min_h: int = 1 << 30
    max_divided: int = 0   # most keys in a node that was divided


@dataclass(eq=False)
class _Node:
    ulx: int = 0
    uly: int = 0
    urx: int = 0
    bry: int = 0
    keys: List[Key] = field(default_factory=list)
    no_more: bool = False
    seq: int = 0


def _c_round(v) -> int:
    """C round() of a non-negative float32: halves away from zero."""
    return int(math.floor(float(v) + 0.5))


def _divide(p: _Node, tr: "Trace" = None):
    """ExtractorNode::DivideNode (:484-540): the four children n1..n4 (top-left, top-right,
    bottom-left, bottom-right), empty ones included."""
    half_x = int(math.ceil(f32(p.urx - p.ulx) / f32(2)))
    half_y = int(math.ceil(f32(p.bry - p.uly) / f32(2)))
    mx, my = p.ulx + half_x, p.uly + half_y  # n1.UR.x, n1.BR.y
    if tr is not None:
        tr.max_divided = max(tr.max_divided, len(p.keys))
    n1 = _Node(p.ulx, p.uly, mx, my)
    n2 = _Node(mx, p.uly, p.urx, my)
    n3 = _Node(p.ulx, my, mx, p.bry)
    n4 = _Node(mx, my, p.urx, p.bry)
    for k in p.keys:
        if k[0] < mx:
            if k[1] < my:
                n1.keys.append(k)
            else:
                n3.keys.append(k)
        elif k[1] < my:
            n2.keys.append(k)
        else:
            n4.keys.append(k)
    for c in (n1, n2, n3, n4):
        c.no_more = len(c.keys) == 1
    return n1, n2, n3, n4


def distribute_traced(keys: Sequence[Key], w: int, h: int, N: int, tie: str = "creation"):
    """DistributeOctTree over `keys` (input order) in a w x h border area with budget N.
    Returns (survivors in list order, Trace)."""
    if tie not in ("creation", "reverse"):
        raise ValueError(tie)
    tr = Trace()
    n_ini = _c_round(f32(w) / f32(h))
    tr.nIni = n_ini
    hx = f32(w) / f32(n_ini)
    seq = 0
    nodes: List[_Node] = []  # index 0 = front of the std::list
    ini = []
    for i in range(n_ini):
        nd = _Node(int(hx * f32(i)), 0, int(hx * f32(i + 1)), h)
        nd.seq = seq
        seq += 1
        nodes.append(nd)
        ini.append(nd)
    for k in keys:
        ini[int(f32(k[0]) / hx)].keys.append(tuple(int(v) for v in k))
    kept = []
    for nd in nodes:
        if len(nd.keys) == 1:
            nd.no_more = True
            kept.append(nd)
        elif nd.keys:
            kept.append(nd)
    nodes = kept

    expand: List[_Node] = []  # vSizeAndPointerToNode: the size is len(node.keys)

    def push_children(children):
        nonlocal seq
        n_exp = 0
        for c in children:
            if not c.keys:
                continue
            tr.min_w = min(tr.min_w, c.urx - c.ulx)
            tr.min_h = min(tr.min_h, c.bry - c.uly)
            c.seq = seq
            seq += 1
            nodes.insert(0, c)
            if len(c.keys) > 1:
                n_exp += 1
                expand.append(c)
        return n_exp

    finish = False
    while not finish:
        tr.passes += 1
        prev_size = len(nodes)
        n_to_expand = 0
        expand.clear()
        for nd in list(nodes):  # the pass visits the nodes present at its start, front to back
            if nd.no_more:
                continue
            n_to_expand += push_children(_divide(nd, tr))
            nodes.remove(nd)
        if len(nodes) >= N or len(nodes) == prev_size:
            finish = True
            tr.stop = PASS_N if len(nodes) >= N else PASS_STALL
        elif len(nodes) + n_to_expand * 3 > N:
            while not finish:
                tr.rounds += 1
                prev_size = len(nodes)
                prev = list(expand)
                expand.clear()
                if tie == "creation":
                    prev.sort(key=lambda nd: (len(nd.keys), nd.seq))
                else:
                    prev.sort(key=lambda nd: (len(nd.keys), -nd.seq))
                tr.left_in_round = 0
                for j in range(len(prev) - 1, -1, -1):
                    push_children(_divide(prev[j], tr))
                    nodes.remove(prev[j])
                    if len(nodes) >= N:
                        tr.left_in_round = j
                        break
                if len(nodes) >= N or len(nodes) == prev_size:
                    finish = True
                    tr.stop = REFINE_N if len(nodes) >= N else REFINE_STALL

    out = []
    for nd in nodes:
        best = nd.keys[0]
        for k in nd.keys[1:]:
            if k[2] > best[2]:
                best = k
        out.append(best)
    tr.nodes = len(out)
    tr.overshoot = len(out) - N
    return out, tr


def distribute(keys: Sequence[Key], w: int, h: int, N: int, tie: str = "creation") -> List[Key]:
    return distribute_traced(keys, w, h, N, tie)[0]


def tie_sensitive(keys: Sequence[Key], w: int, h: int, N: int) -> bool:
    """Whether the order of equal-size nodes in the refinement's sort changes the result."""
    return distribute(keys, w, h, N, "creation") != distribute(keys, w, h, N, "reverse")


def owner_disagreements(w: int, h: int) -> List[int]:
    """The integer x in [0, w) whose initial node by (size_t)(x / hX) (:572) is not the node whose
    [(int)(hX * i), (int)(hX * (i + 1))) bounds (:558-559) contain it."""
    n_ini = _c_round(f32(w) / f32(h))
    hx = f32(w) / f32(n_ini)
    bad = []
    for x in range(w):
        o = int(f32(x) / hx)
        if not (int(hx * f32(o)) <= x < int(hx * f32(o + 1))):
            bad.append(x)
    return bad
