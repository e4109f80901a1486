"""The ring contract of polygon export as a sequential definition on dense numpy masks, and the checks of
that definition against scipy.ndimage -- no kernel, no run table.

Pixel (x, y) covers [x, x + 1] x [y, y + 1], y points down.  Every unit side between a set pixel and an unset one (or the
canvas border) is a directed edge, clockwise on screen around the set pixel.  The successor of an edge is the edge leaving
its end vertex; at a saddle (two set pixels touching only diagonally) two edges leave and the successor is the one of the
OTHER set pixel, which makes the foreground 8-connected and the background 4-connected.  A ring is a closed walk, stored as
its corners from its smallest vertex by (x, y) on, without repeating it; area2 = sum(x_i y_{i+1} - x_{i+1} y_i) is positive
for outer rings and negative for holes; rings are ordered by first vertex; the parent of a hole is the outer ring of
smallest area2 that contains the centre of the pixel left of the hole's first vertex."""
import numpy as np


def _edges(mask):
    """the directed unit edges: arrays (sx, sy, ex, ey, px, py)"""
    m = np.asarray(mask).astype(bool)
    p = np.pad(m, 1)
    ys, xs = np.nonzero(m)
    up, down = ~p[ys, xs + 1], ~p[ys + 2, xs + 1]
    left, right = ~p[ys + 1, xs], ~p[ys + 1, xs + 2]
    out = []
    for sel, (sx, sy, ex, ey) in ((up, (0, 0, 1, 0)), (right, (1, 0, 1, 1)), (down, (1, 1, 0, 1)), (left, (0, 1, 0, 0))):
        x, y = xs[sel], ys[sel]
        out.append(np.stack([x + sx, y + sy, x + ex, y + ey, x, y], 1))
    return np.concatenate(out, 0) if out else np.zeros((0, 6), np.int64)


def trace(mask):
    """one [H, W] mask -> list of (ring int32 [m, 2] = (x, y), parent, area2), the contract above"""
    edges = _edges(mask).tolist()
    leaving = {}
    for i, (sx, sy, ex, ey, px, py) in enumerate(edges):
        leaving.setdefault((sx, sy), []).append(i)
    seen = [False] * len(edges)
    rings = []
    for i0 in range(len(edges)):
        if seen[i0]:
            continue
        walk, i = [], i0
        while not seen[i]:
            seen[i] = True
            walk.append(i)
            sx, sy, ex, ey, px, py = edges[i]
            cand = leaving[(ex, ey)]
            if len(cand) == 1:
                i = cand[0]
            else:
                assert len(cand) == 2
                other = [j for j in cand if (edges[j][4], edges[j][5]) != (px, py)]
                assert len(other) == 1
                i = other[0]
        assert i == i0                                                   # a closed walk
        dirs = [(edges[j][2] - edges[j][0], edges[j][3] - edges[j][1]) for j in walk]
        corners = [(edges[j][0], edges[j][1]) for t, j in enumerate(walk) if dirs[t] != dirs[t - 1]]
        s = corners.index(min(corners))
        assert corners.count(corners[s]) == 1
        corners = corners[s:] + corners[:s]
        area2 = sum(corners[t][0] * corners[(t + 1) % len(corners)][1] - corners[(t + 1) % len(corners)][0] * corners[t][1]
                    for t in range(len(corners)))
        rings.append((corners, area2))
    rings.sort(key=lambda r: r[0][0])
    starts = [r[0][0] for r in rings]
    assert len(set(starts)) == len(starts)                               # two rings of one mask never share a first vertex
    # parents: even-odd count of every outer ring's vertical edges left of the test point
    outer = [t for t, r in enumerate(rings) if r[1] > 0]
    seg_x, seg_lo, seg_hi, seg_ring = [], [], [], []
    for oi, t in enumerate(outer):
        c = np.asarray(rings[t][0])
        nx = np.roll(c, -1, 0)
        v = c[:, 0] == nx[:, 0]
        seg_x.append(c[v, 0])
        seg_lo.append(np.minimum(c[v, 1], nx[v, 1]))
        seg_hi.append(np.maximum(c[v, 1], nx[v, 1]))
        seg_ring.append(np.full(int(v.sum()), oi))
    if outer:
        seg_x, seg_lo, seg_hi, seg_ring = (np.concatenate(a) for a in (seg_x, seg_lo, seg_hi, seg_ring))
    out = []
    for t, (corners, area2) in enumerate(rings):
        parent = -1
        if area2 < 0:
            x0, y0 = corners[0]
            hit = (seg_x <= x0 - 1) & (seg_lo <= y0) & (y0 < seg_hi)     # left of (x0 - 0.5, y0 + 0.5)
            inside = np.flatnonzero(np.bincount(seg_ring[hit], minlength=len(outer)) & 1)
            assert inside.size
            parent = min((rings[outer[oi]][1], outer[oi]) for oi in inside.tolist())[1]
        out.append((np.asarray(corners, np.int32).reshape(-1, 2), parent, int(area2)))
    return out


def flatten(per_instance):
    """list (one entry per instance: trace()'s list, or None / [] for no rings) -> the six arrays of ops.mask_polygons"""
    verts, offs, inst, parent, area2, ioffs = [], [0], [], [], [], [0]
    for i, rings in enumerate(per_instance):
        for ring, par, a2 in (rings or []):
            verts.append(np.asarray(ring, np.int32).reshape(-1, 2))
            offs.append(offs[-1] + len(ring))
            inst.append(i)
            parent.append(par)
            area2.append(a2)
        ioffs.append(len(inst))
    v = np.concatenate(verts, 0) if verts else np.zeros((0, 2), np.int32)
    return (v.astype(np.int32), np.asarray(offs, np.int64), np.asarray(inst, np.int32), np.asarray(parent, np.int32),
            np.asarray(area2, np.int64), np.asarray(ioffs, np.int64))


def refill(verts, ring_offs, H, W):
    """even-odd refill of ONE instance's rings: a signed count of the vertical edges (+1 upward = foreground on the right,
    -1 downward) into an [H, W + 1] array, summed along x"""
    verts, ring_offs = np.asarray(verts, np.int64).reshape(-1, 2), np.asarray(ring_offs, np.int64)
    d = np.zeros((H + 1, W + 1), np.int64)
    if len(verts):
        nxt = np.arange(1, len(verts) + 1)
        nxt[ring_offs[1:] - 1] = ring_offs[:-1]
        a, b = verts, verts[nxt]
        v = a[:, 0] == b[:, 0]
        sign = np.where(a[v, 1] > b[v, 1], 1, -1)
        lo, hi = np.minimum(a[v, 1], b[v, 1]), np.maximum(a[v, 1], b[v, 1])
        np.add.at(d, (lo, a[v, 0]), sign)
        np.add.at(d, (hi, a[v, 0]), -sign)
    return np.cumsum(np.cumsum(d, 0)[:H], 1)[:, :W]


def check_properties(mask, verts, ring_offs, ring_parent, ring_area2):
    """what must hold for the rings of ONE mask whoever made them, against the mask and scipy.ndimage.label (vectorised:
    usable at 1024 x 1024).  Returns (outer rings, holes)."""
    from scipy import ndimage
    mask = np.asarray(mask).astype(bool)
    H, W = mask.shape
    verts = np.asarray(verts, np.int64).reshape(-1, 2)
    ring_offs, ring_parent, ring_area2 = (np.asarray(a, np.int64) for a in (ring_offs, ring_parent, ring_area2))
    assert int(ring_area2.sum()) == 2 * int(mask.sum())                  # the area identity
    lab8, n8 = ndimage.label(mask, structure=np.ones((3, 3), int))
    _, n4 = ndimage.label(~np.pad(mask, 1))
    outer, holes = ring_area2 > 0, ring_area2 < 0
    assert int(outer.sum()) == n8 and int(holes.sum()) == n4 - 1 and not (ring_area2 == 0).any()
    assert (ring_parent[outer] == -1).all()
    starts = verts[ring_offs[:-1]]
    if len(starts) > 1:                                                  # ordered by first vertex, all different
        key = starts[:, 0] * (H + 1) + starts[:, 1]
        assert (np.diff(key) > 0).all()
    if holes.any():
        hp = ring_parent[holes]
        assert (hp >= 0).all() and (hp < len(ring_area2)).all() and outer[hp].all()
        hs, ps = starts[holes], starts[hp]
        assert (lab8[hs[:, 1], hs[:, 0] - 1] == lab8[ps[:, 1], ps[:, 0]]).all() and (lab8[ps[:, 1], ps[:, 0]] > 0).all()
    assert np.array_equal(refill(verts, ring_offs, H, W), mask.astype(np.int64))
    return int(outer.sum()), int(holes.sum())


def check_traced(mask):
    """trace(mask) + check_properties on it; returns trace's list"""
    rings = trace(mask)
    v, o, _, p, a, _ = flatten([rings])
    check_properties(mask, v, o, p, a)
    for ring, _, _ in rings:                                             # corners only: the direction changes at every vertex
        d = np.roll(ring, -1, 0) - ring
        assert ((d[:, 0] == 0) != (d[:, 1] == 0)).all() and ((d[:, 0] == 0) != (np.roll(d, 1, 0)[:, 0] == 0)).all()
    return rings
