"""The sequential statement of the oriented-box contract, in Python integers and fractions; it imports nothing
from the package.

Pixel (x, y) covers [x, x + 1] x [y, y + 1], y down.  An instance is the union of the closed squares of ALL its set pixels.
  hull       Andrew's monotone chain over the pixel corners: strictly convex, from the smallest vertex by (x, y) on, clockwise on
             screen (area2 = sum x_i y_{i+1} - x_{i+1} y_i > 0), first vertex not repeated.
  rectangle  hull edge j from vertex j to j + 1 (cyclic): e = (ex, ey), nrm = (-ey, ex) (points inside), L = ex^2 + ey^2; over
             the hull vertices p: a = p . e, b = p . nrm, U = amax - amin, V = bmax - bmin.  Area U V / L as a Fraction; the
             smallest wins, the lowest j among equals.  q = (ex, ey, amin, amax, bmin, bmax).
  corners    C0..C3 = (amin, bmin), (amax, bmin), (amax, bmax), (amin, bmax) in the (e, nrm) frame, pixel coordinates
             (a e + b nrm) / L: clockwise on screen, C0 -> C1 on the hull edge.
  xywha      centre = mean of the corners, sides U / sqrt L along e and V / sqrt L along nrm, w the longer (e on U == V), the
             angle of the w side from +x towards +y in [-pi / 2, pi / 2)."""
import math
from fractions import Fraction

import numpy as np


def pixels_of(mask):
    ys, xs = np.nonzero(np.asarray(mask, bool))
    return list(zip(xs.tolist(), ys.tolist()))


def corner_points(pixels):
    pts = set()
    for x, y in pixels:
        pts.update(((x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)))
    return sorted(pts)


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def area2_of(ring):
    return sum(ring[i][0] * ring[(i + 1) % len(ring)][1] - ring[(i + 1) % len(ring)][0] * ring[i][1] for i in range(len(ring)))


def canonical(ring):
    """from the smallest vertex on, positive area2"""
    ring = list(ring)
    if area2_of(ring) < 0:
        ring.reverse()
    i = ring.index(min(ring))
    return ring[i:] + ring[:i]


def hull_of_points(pts):
    """Andrew's monotone chain on sorted distinct points; collinear points are dropped"""
    if not pts:
        return []
    first, second = [], []
    for p in pts:
        while len(first) >= 2 and _cross(first[-2], first[-1], p) <= 0:
            first.pop()
        first.append(p)
    for p in reversed(pts):
        while len(second) >= 2 and _cross(second[-2], second[-1], p) <= 0:
            second.pop()
        second.append(p)
    return canonical(first[:-1] + second[:-1])


def hull_of_pixels(pixels):
    return hull_of_points(corner_points(pixels))


def hull(mask):
    return hull_of_pixels(pixels_of(mask))


def edge_frame(ring, j):
    """(q, L) of the rectangle flush with edge j"""
    p0, p1 = ring[j], ring[(j + 1) % len(ring)]
    ex, ey = p1[0] - p0[0], p1[1] - p0[1]
    r = np.asarray(ring, np.int64)                       # coordinates below 2^16: a and b stay below 2^34
    a, b = r[:, 0] * ex + r[:, 1] * ey, r[:, 1] * ex - r[:, 0] * ey
    return (ex, ey, int(a.min()), int(a.max()), int(b.min()), int(b.max())), ex * ex + ey * ey


def rect_area(q, L):
    return Fraction((q[3] - q[2]) * (q[5] - q[4]), L)


def min_rect(ring):
    """(edge, q, area) of a canonical strictly convex ring; (-1, zeros, 0) of an empty one"""
    if not ring:
        return -1, (0,) * 6, Fraction(0)
    best = None
    for j in range(len(ring)):
        q, L = edge_frame(ring, j)
        area = rect_area(q, L)
        if best is None or area < best[2]:
            best = (j, q, area)
    return best


def uvl_bits(ring):
    """the bits of the largest U V L over the edges: what the exact comparison multiplies"""
    most = 0
    for j in range(len(ring)):
        q, L = edge_frame(ring, j)
        most = max(most, ((q[3] - q[2]) * (q[5] - q[4]) * L).bit_length())
    return most


def corners(q):
    """[4][2] Fractions: C0..C3 in pixel coordinates"""
    ex, ey, amin, amax, bmin, bmax = q
    L = ex * ex + ey * ey
    return [[Fraction(a * ex - b * ey, L), Fraction(a * ey + b * ex, L)] for a, b in
            ((amin, bmin), (amax, bmin), (amax, bmax), (amin, bmax))]


def xywha(q):
    """(cx, cy, w, h, angle) as floats computed from exact values"""
    ex, ey, amin, amax, bmin, bmax = q
    L = ex * ex + ey * ey
    c = corners(q)
    cx, cy = sum(p[0] for p in c) / 4, sum(p[1] for p in c) / 4
    U, V = amax - amin, bmax - bmin
    su, sv = math.sqrt(Fraction(U * U, L)), math.sqrt(Fraction(V * V, L))
    if U >= V:
        w, h, ang = su, sv, math.atan2(ey, ex)
    else:
        w, h, ang = sv, su, math.atan2(ex, -ey)
    if ang >= math.pi / 2:
        ang -= math.pi
    elif ang < -math.pi / 2:
        ang += math.pi
    return float(cx), float(cy), w, h, ang


def obb(pixels_or_mask):
    """(hull as a list of (x, y), area2, edge, q) of a dense mask or a list of (x, y) pixels"""
    pixels = pixels_or_mask if isinstance(pixels_or_mask, list) else pixels_of(pixels_or_mask)
    ring = hull_of_pixels(pixels)
    edge, q, _ = min_rect(ring)
    return ring, (area2_of(ring) if ring else 0), edge, q


# ------------------------------------------------------------------------------------------------------------ properties
def check(pixels_or_mask):
    """obb() with the properties of the issue asserted: every pixel corner on or inside the hull, strict convexity, area2 >= 2
    popcount, the rectangle around every hull vertex and no larger than the axis-aligned box, no rectangle flush with another
    edge smaller (and none equal at a lower index)"""
    pixels = pixels_or_mask if isinstance(pixels_or_mask, list) else pixels_of(pixels_or_mask)
    ring, a2, edge, q = obb(pixels)
    if not pixels:
        assert ring == [] and edge == -1 and a2 == 0
        return ring, a2, edge, q
    m = len(ring)
    assert m >= 4 and a2 > 0 and ring[0] == min(ring) and len(set(ring)) == m
    for i in range(m):
        assert _cross(ring[i], ring[(i + 1) % m], ring[(i + 2) % m]) > 0, 'not strictly convex / not clockwise on screen'
    pts = np.array(corner_points(pixels), np.int64)
    r = np.array(ring, np.int64)
    rn = np.roll(r, -1, 0)
    cr = (rn[None, :, 0] - r[None, :, 0]) * (pts[:, None, 1] - r[None, :, 1]) - \
        (rn[None, :, 1] - r[None, :, 1]) * (pts[:, None, 0] - r[None, :, 0])
    assert (cr >= 0).all(), 'a pixel corner outside the hull'
    assert set(ring) <= set(map(tuple, pts.tolist()))
    assert a2 >= 2 * len(set(pixels))
    ex, ey, amin, amax, bmin, bmax = q
    fq, L = edge_frame(ring, edge)
    assert fq == q and L > 0
    for p in ring:
        assert amin <= p[0] * ex + p[1] * ey <= amax and bmin <= p[1] * ex - p[0] * ey <= bmax
    assert bmin == ring[edge][1] * ex - ring[edge][0] * ey
    area = rect_area(q, L)
    xs, ys = [p[0] for p in ring], [p[1] for p in ring]
    assert area <= (max(xs) - min(xs)) * (max(ys) - min(ys)) and 2 * area >= a2
    for j in range(m):
        other = rect_area(*edge_frame(ring, j))
        assert other > area or (other == area and j >= edge)
    c = corners(q)
    assert area2_of(c) == 2 * area                                      # clockwise on screen, the rectangle's own area
    p0, p1 = ring[edge], ring[(edge + 1) % m]
    assert (c[1][0] - c[0][0]) * (p1[1] - p0[1]) == (c[1][1] - c[0][1]) * (p1[0] - p0[0])          # C0 -> C1 along the hull edge
    return ring, a2, edge, q
