"""The contract of shared-border simplification (csrc/ring_coverage.hip, ops.ring_coverage) as a sequential
definition on a dense label map in plain Python integers -- no kernel, no run table, no floating point.

LABELS.  L int [H, W]: the instance of every pixel, -1 for background; owner(x, y) = L[y, x], -1 outside the canvas.
NODES.  A lattice point p = (px, py) in [0, W] x [0, H] with the pixels a = (px - 1, py - 1), b = (px, py - 1), c = (px - 1,
py), d = (px, py) around it is a node iff [a != b] + [b != d] + [d != c] + [c != a] >= 3 on owners.
NODED RING.  The ring of §14.7 (tests/_mask_polygons_ref.py trace: corners only, from its smallest vertex) with every node
that lies strictly inside one of its straight segments inserted in order, then rotated to begin at its first node visit
counted from that start (no node: it stays).  Every vertex carries a node flag and `other`, the owner on the far side of the
unit step that leaves it.  Rings run clockwise on screen around the set pixel, so travelling right at row Y the far pixels
are row Y - 1, down at column X column X, left row Y, up column X - 1; the inside owner is asserted at every step.
ARCS.  Every node visit is kept and index 0 is kept; the chains between consecutive kept vertices are the arcs, the last one
closes to v_m := v_0.  A chain (a, b) with b - a >= 2 takes num_i / den of §14.8 (tests/_ring_simplify_ref.seg_dist2) for its
inner vertices, s = argmax num_i -- among equals the vertex with the smallest (x, y) --, and splits at s iff the two ends are
the same point or 256 num_s > tol2_q8 den.  Both rules are symmetric under reversal of the chain.
SURVIVAL and OUTPUT.  As _ring_simplify_ref.simplify with min_ring_area = 0, on the noded rings; vert_other = `other` of the
kept vertices of the survivors."""
from fractions import Fraction

import numpy as np

import _mask_polygons_ref as pref
import _ring_simplify_ref as sref

# what the reference met since reset_stats(): ties (chains whose largest num several vertices share), ties in which the
# lowest index and the smallest point are different vertices, chains whose two ends are one point, nodes inserted into straight
# segments, rings dropped
STATS = dict(ties=0, ties_differ=0, closed_chains=0, inserted_nodes=0, dropped_rings=0)


def reset_stats():
    for key in STATS:
        STATS[key] = 0


def labels_of(masks, H, W):
    """k disjoint boolean masks -> the label map"""
    L = np.full((H, W), -1, np.int64)
    for i, m in enumerate(masks):
        m = np.asarray(m, bool)
        assert (L[m] == -1).all(), 'the masks overlap'
        L[m] = i
    return L


def masks_of(L, k):
    return [np.asarray(L) == i for i in range(k)]


def _owner(rows, H, W, x, y):
    return rows[y][x] if 0 <= x < W and 0 <= y < H else -1


def is_node(rows, H, W, px, py):
    a, b = _owner(rows, H, W, px - 1, py - 1), _owner(rows, H, W, px, py - 1)
    c, d = _owner(rows, H, W, px - 1, py), _owner(rows, H, W, px, py)
    return (a != b) + (b != d) + (d != c) + (c != a) >= 3


def noded_ring(rows, H, W, inst, corners):
    """the corners of one ring of instance `inst` -> (points, flags, others) of the rotated noded ring"""
    pts, flags, others = [], [], []
    m = len(corners)
    for t in range(m):
        (x0, y0), (x1, y1) = corners[t], corners[(t + 1) % m]
        assert (x0 == x1) != (y0 == y1)
        sx, sy = (x1 > x0) - (x1 < x0), (y1 > y0) - (y1 < y0)
        x, y = x0, y0
        while (x, y) != (x1, y1):
            # the pixels on either side of the unit step that leaves (x, y)
            if sx > 0:
                inside, far = (x, y), (x, y - 1)
            elif sx < 0:
                inside, far = (x - 1, y - 1), (x - 1, y)
            elif sy > 0:
                inside, far = (x - 1, y), (x, y)
            else:
                inside, far = (x, y - 1), (x - 1, y - 1)
            assert _owner(rows, H, W, *inside) == inst
            node = is_node(rows, H, W, x, y)
            if (x, y) == (x0, y0) or node:
                if (x, y) != (x0, y0):
                    STATS['inserted_nodes'] += 1
                pts.append((x, y))
                flags.append(bool(node))
                others.append(_owner(rows, H, W, *far))
            x, y = x + sx, y + sy
    if True in flags:
        f = flags.index(True)
        pts, flags, others = pts[f:] + pts[:f], flags[f:] + flags[:f], others[f:] + others[:f]
    return pts, flags, others


def simplify_arcs(ring, flags, q8):
    """the noded ring -> (sorted kept indices, rounds): rounds = the levels of the split trees of its arcs that kept a vertex"""
    m = len(ring)
    keep = [bool(f) for f in flags]
    if m:
        keep[0] = True
    ends = [i for i in range(m) if keep[i]] + [m]
    stack = [(a, b, 1) for a, b in zip(ends[:-1], ends[1:])]
    rounds = 0
    while stack:
        a, b, level = stack.pop()
        if b - a < 2:
            continue
        va, vb = ring[a], ring[b % m]
        nums = [sref.seg_dist2(ring[i], va, vb) for i in range(a + 1, b)]
        den = nums[0][1]
        vals = [v for v, _ in nums]
        top = max(vals)
        closed = va == vb
        STATS['closed_chains'] += closed
        if closed or 256 * top > q8 * den:
            tied = [a + 1 + j for j, v in enumerate(vals) if v == top]
            s = min(tied, key=lambda i: (ring[i], i))
            STATS['ties'] += len(tied) > 1
            STATS['ties_differ'] += s != tied[0]
            keep[s] = True
            rounds = max(rounds, level)
            stack.append((a, s, level + 1))
            stack.append((s, b, level + 1))
    return [i for i in range(m) if keep[i]], rounds


def noded(L, k):
    """label map -> (the six arrays of the noded rings (numpy, the layout of ops.mask_polygons), flags, others: per ring lists)"""
    L = np.asarray(L)
    H, W = L.shape
    rows = L.tolist()
    per_instance, flags, others = [], [], []
    for i in range(k):
        rings = []
        for ring, par, a2 in pref.trace(L == i):
            pts, fl, ot = noded_ring(rows, H, W, i, [tuple(v) for v in ring.tolist()])
            assert sref.area2_of(pts) == a2
            rings.append((np.asarray(pts, np.int32).reshape(-1, 2), par, a2))
            flags.append(fl)
            others.append(ot)
        per_instance.append(rings)
    return pref.flatten(per_instance), flags, others


def coverage(L, k, q8, pre=None):
    """label map -> (the six arrays of the survivors, ring_src, vert_other, rounds int32 [R] of every traced ring), numpy;
    pre = noded(L, k) of an earlier call"""
    arrays, flags, others = pre if pre is not None else noded(L, k)
    V, ro = arrays[0].tolist(), arrays[1].tolist()
    kept, rounds = [], []
    for r in range(len(flags)):
        ring = [tuple(v) for v in V[ro[r]:ro[r + 1]]]
        idx, nr = simplify_arcs(ring, flags[r], q8)
        kept.append(idx)
        rounds.append(nr)
    out, src, rnd, _ = sref.simplify(arrays, q8, 0, pre=(kept, rounds))
    STATS['dropped_rings'] += len(flags) - len(src)
    other = [others[r][i] for r in src.tolist() for i in kept[r]]
    return out + (src, np.asarray(other, np.int32), rnd)


def lists(result):
    """coverage()'s result (or the device's, as numpy) -> per instance a list of (ring [m, 2], parent, area2, other [m])"""
    v, ro, _, par, a2, io = (np.asarray(x) for x in result[:6])
    other = np.asarray(result[7])
    ro, io = ro.tolist(), io.tolist()
    return [[(v[ro[r]:ro[r + 1]], int(par[r]), int(a2[r]), other[ro[r]:ro[r + 1]]) for r in range(io[i], io[i + 1])]
            for i in range(len(io) - 1)]


# ------------------------------------------------------------------------------------------------------------ properties
def directed_edges(verts, ring_offs, ring_inst, vert_other):
    """(u, w, instance, other) of every kept edge"""
    v = np.asarray(verts).reshape(-1, 2)
    ro, inst, other = np.asarray(ring_offs).tolist(), np.asarray(ring_inst).tolist(), np.asarray(vert_other).tolist()
    out = []
    for r in range(len(inst)):
        pts = [tuple(p) for p in v[ro[r]:ro[r + 1]].tolist()]
        for t in range(len(pts)):
            out.append((pts[t], pts[(t + 1) % len(pts)], inst[r], other[ro[r] + t]))
    return out


def unmatched_twins(edges, lost=()):
    """the directed edges (u -> w, i, other >= 0) whose twin (w -> u, other, i) is missing, as a multiset difference;
    pairs with an instance in `lost` (it lost a ring) are left out"""
    from collections import Counter
    c = Counter(e for e in edges if e[3] >= 0 and e[2] not in lost and e[3] not in lost)
    bad = 0
    for (u, w, i, o), cnt in c.items():
        bad += max(0, cnt - c.get((w, u, o, i), 0))
    return bad


def lost_instances(n_rings_in, result):
    """the instances that lost a ring: inst_ring_offs of the traced rings against the result's"""
    a, b = np.diff(np.asarray(n_rings_in)), np.diff(np.asarray(result[5]))
    return set(np.flatnonzero(a != b).tolist())


def check_properties(L, k, nod, result, q8):
    """every node is kept; every dropped vertex of a surviving ring lies within the tolerance of its kept segment (fractions)
    unless the chain around it has one point for both ends; the twin edges match"""
    arrays, flags, _ = nod
    V, ro = arrays[0].tolist(), arrays[1].tolist()
    ov, oo = np.asarray(result[0]).tolist(), np.asarray(result[1]).tolist()
    eps2 = Fraction(q8, 256)
    for r2, r in enumerate(np.asarray(result[6]).tolist()):
        ring = [tuple(v) for v in V[ro[r]:ro[r + 1]]]
        got = [tuple(v) for v in ov[oo[r2]:oo[r2 + 1]]]
        idx, j = [], 0
        for p in got:                                                    # the kept vertices are a subsequence from v_0 on
            while ring[j] != p:
                j += 1
            idx.append(j)
            j += 1
        assert idx[0] == 0 and all(i in idx for i in range(len(ring)) if flags[r][i])
        ends = idx + [len(ring)]
        for a, b in zip(ends[:-1], ends[1:]):
            for i in range(a + 1, b):
                num, den = sref.seg_dist2(ring[i], ring[a], ring[b % len(ring)])
                assert Fraction(num, den) <= eps2, (r, i, a, b)
    edges = directed_edges(result[0], result[1], result[2], result[7])
    assert unmatched_twins(edges, lost_instances(arrays[5], result)) == 0
    return len(edges)
