"""The contract of polygon simplification (csrc/ring_simplify.hip, ops.ring_simplify) as a sequential definition
in plain Python integers -- no kernel, no floating point, an explicit stack.

A ring is v_0 .. v_{m-1}, closed by v_m := v_0.  Index 0 is kept, and so is f = argmax_{0<i<m} |v_i - v_0|^2 (lowest i among
equals).  A chain (a, b) of kept indices with b - a >= 2 takes for every a < i < b the squared distance num_i / den of v_i to
the SEGMENT v_a v_b; s = argmax num_i (lowest index among equals) is kept, and (a, s), (s, b) go on, iff
256 num_s > tol2_q8 den, tol2_q8 = round(256 tolerance^2).  Rings then survive in this order: |old area2| >= 2 min_ring_area,
at least 3 kept vertices, a new doubled area that is not 0 and has the old one's sign, and for a hole a surviving parent."""
from fractions import Fraction

import numpy as np

# what the reference met since reset_stats(): ties the lowest-index rule decided, chains whose two ends are one point (every
# ring has one: the closing chain (0, m) the anchor is taken from; inner_zero_chords counts the later ones), the largest
# numerator, the deepest split tree
STATS = dict(ties=0, zero_chords=0, inner_zero_chords=0, max_num=0, depth=0)


def reset_stats():
    STATS.update(ties=0, zero_chords=0, inner_zero_chords=0, max_num=0, depth=0)


def tol2_q8(tolerance):
    return int(round(float(tolerance) ** 2 * 256))


def seg_dist2(p, a, b):
    """(num, den) of the squared distance from p to the segment a b, integers"""
    dx, dy = b[0] - a[0], b[1] - a[1]
    ex, ey = p[0] - a[0], p[1] - a[1]
    L = dx * dx + dy * dy
    if L == 0:
        return ex * ex + ey * ey, 1
    t = ex * dx + ey * dy
    if t <= 0:
        return (ex * ex + ey * ey) * L, L
    if t >= L:
        fx, fy = p[0] - b[0], p[1] - b[1]
        return (fx * fx + fy * fy) * L, L
    c = ex * dy - ey * dx
    return c * c, L


def simplify_ring(ring, q8):
    """ring: list of (x, y) Python ints -> (sorted kept indices, rounds): rounds = the levels of the split tree that kept a
    vertex (the anchor is level 1), which is the number of rounds the kernels take"""
    m = len(ring)
    if m == 0:
        return [], 0
    keep = [False] * m
    keep[0] = True
    if m < 2:
        return [0], 0
    d0 = [seg_dist2(ring[i], ring[0], ring[0])[0] for i in range(1, m)]      # the chain (0, m): its ends are one point
    STATS['zero_chords'] += 1
    best = max(d0)
    STATS['ties'] += d0.count(best) - 1
    f = 1 + d0.index(best)
    keep[f] = True
    rounds = 1
    stack = [(0, f, 2), (f, m, 2)]
    while stack:
        a, b, level = stack.pop()
        if b - a < 2:
            continue
        va, vb = ring[a], ring[b % m]
        nums = [seg_dist2(ring[i], va, vb) for i in range(a + 1, b)]
        den = nums[0][1]
        if va == vb:
            STATS['zero_chords'] += 1
            STATS['inner_zero_chords'] += 1
        vals = [n for n, _ in nums]
        top = max(vals)
        STATS['max_num'] = max(STATS['max_num'], top)
        if 256 * top > q8 * den:
            STATS['ties'] += vals.count(top) - 1
            s = a + 1 + vals.index(top)
            keep[s] = True
            rounds = max(rounds, level)
            stack.append((a, s, level + 1))
            stack.append((s, b, level + 1))
    STATS['depth'] = max(STATS['depth'], rounds)
    return [i for i in range(m) if keep[i]], rounds


def area2_of(pts):
    return sum(pts[t][0] * pts[(t + 1) % len(pts)][1] - pts[(t + 1) % len(pts)][0] * pts[t][1] for t in range(len(pts)))


def simplify(arrays, q8, min_ring_area=0, pre=None):
    """the six arrays of ops.mask_polygons (numpy) -> (the six arrays of the survivors, ring_src int32 [R'], rounds int32 [R]
    of every INPUT ring, kept: per input ring the kept indices).  pre = (kept, rounds) of an earlier call on the same rings
    at the same q8: the rings are not simplified again"""
    verts, ring_offs, ring_inst, ring_parent, ring_area2, inst_ring_offs = (np.asarray(a) for a in arrays)
    V = verts.reshape(-1, 2).tolist()
    ro, inst, par, a2, io = (x.tolist() for x in (ring_offs, ring_inst, ring_parent, ring_area2, inst_ring_offs))
    R, k = len(inst), len(io) - 1
    kept, rounds, new_a2, alive = [], [], [], []
    for r in range(R):
        ring = [tuple(v) for v in V[ro[r]:ro[r + 1]]]
        idx, nr = (pre[0][r], pre[1][r]) if pre is not None else simplify_ring(ring, q8)
        kept.append(idx)
        rounds.append(nr)
        na = area2_of([ring[i] for i in idx]) if idx else 0
        new_a2.append(na)
        ok = abs(a2[r]) >= 2 * min_ring_area
        ok = ok and len(idx) >= 3
        ok = ok and na != 0 and (na > 0) == (a2[r] > 0)
        alive.append(ok)
    for r in range(R):
        if par[r] >= 0 and not alive[io[inst[r]] + par[r]]:
            alive[r] = False
    new_index, c = [], 0
    for r in range(R):
        new_index.append(c if alive[r] else -1)
        c += alive[r]
    o_verts, o_offs, o_inst, o_par, o_a2, o_src = [], [0], [], [], [], []
    o_io = [0] * (k + 1)
    for r in range(R):
        if not alive[r]:
            continue
        ring = V[ro[r]:ro[r + 1]]
        o_verts += [ring[i] for i in kept[r]]
        o_offs.append(len(o_verts))
        o_inst.append(inst[r])
        o_a2.append(new_a2[r])
        o_src.append(r)
        o_io[inst[r] + 1] += 1
    o_io = np.cumsum(o_io).tolist()
    for r in range(R):
        if alive[r]:
            o_par.append(-1 if par[r] < 0 else new_index[io[inst[r]] + par[r]] - o_io[inst[r]])
    out = (np.asarray(o_verts, np.int32).reshape(-1, 2), np.asarray(o_offs, np.int64), np.asarray(o_inst, np.int32),
           np.asarray(o_par, np.int32), np.asarray(o_a2, np.int64), np.asarray(o_io, np.int64))
    return out, np.asarray(o_src, np.int32), np.asarray(rounds, np.int32), kept


def simplify_lists(per_instance, q8, min_ring_area=0):
    """per-instance ring lists (ring [m, 2], parent, area2) -> the same form, simplified"""
    import _mask_polygons_ref as pref
    out, _, _, _ = simplify(pref.flatten(per_instance), q8, min_ring_area)
    v, ro, _, par, a2, io = (x.tolist() for x in out)
    v = np.asarray(v, np.int32).reshape(-1, 2)
    return [[(v[ro[r]:ro[r + 1]], par[r], a2[r]) for r in range(io[i], io[i + 1])] for i in range(len(io) - 1)]


def check_ring(ring, idx, q8):
    """what must hold for the kept indices of one ring: a subsequence with v_0, and every dropped vertex within the
    tolerance of the segment between the kept pair around it (exact, fractions)"""
    m = len(ring)
    assert idx == sorted(set(idx)) and (m == 0 or idx[0] == 0) and all(0 <= i < m for i in idx)
    eps2 = Fraction(q8, 256)
    ends = idx + [m]
    for a, b in zip(ends[:-1], ends[1:]):
        for i in range(a + 1, b):
            num, den = seg_dist2(ring[i], ring[a], ring[b % m])
            assert Fraction(num, den) <= eps2, (i, a, b)
