"""Bodies of the shared-border simplification tests (csrc/ring_coverage.hip, ops.ring_coverage, rle.simplify_coverage,
apis.masks_to_polygons(topology='shared'), large_image polygon_topology), shared by both tiers:
tests/test_ring_coverage_cpu.py calls them with the emulated `ops` on CPU tensors, tests/test_gpu_ring_coverage.py with the
real ones on cuda:0.  The reference is tests/_ring_coverage_ref.py, the sequential definition on a dense label map in Python
integers; all nine arrays (the six of the rings, ring_src, vert_other and the rounds every traced ring took) are compared by
exact equality."""
import numpy as np
import torch

import _mask_polygons_ref as pref
import _ring_coverage_ref as cref
import _ring_simplify_cases as scases
import _ring_simplify_ref as sref
import _run_flatten_cases as fcases
import _seam_merge_cases as seam_cases

NAMES = ('verts', 'ring_offs', 'ring_inst', 'ring_parent', 'ring_area2', 'inst_ring_offs', 'ring_src', 'vert_other', 'rounds')
TOLERANCES = (0, 0.5, 1, 1.5, 2, 5)
NESTED = (0, 0.5, 1, 2, 5)
ReadCounter, Poison = fcases.ReadCounter, fcases.Poison


# --------------------------------------------------------------------------------------------------------------- maps
def diagonal_split(side=16):
    """two instances along x + y < side: a staircase border of 2 side - 1 shared vertices"""
    return np.where(np.add.outer(np.arange(side), np.arange(side)) < side, 0, 1)


def slope2_split():
    yy, xx = np.mgrid[:32, :16]
    return np.where(2 * xx + yy < 32, 0, 1)


def t_junction():
    """A = rows 0-3, B = rows 4-7 with x < 5, C = rows 4-7 with x >= 5 on 8 x 12: (5, 4) lies inside A's bottom wall"""
    L = np.zeros((8, 12), np.int64)
    L[4:, :5] = 1
    L[4:, 5:] = 2
    return L


def framed(island, pad=2, bg=1):
    """instance 1 = the island, instance 0 = a frame `pad` pixels thick around it, `bg` background pixels around the frame"""
    island = np.asarray(island, bool)
    h, w = island.shape
    L = np.full((h + 2 * (pad + bg), w + 2 * (pad + bg)), -1, np.int64)
    L[bg:-bg, bg:-bg] = 0
    inner = L[bg + pad:bg + pad + h, bg + pad:bg + pad + w]
    inner[island] = 1
    return L


def touching_islands():
    """islands B and C inside A that touch each other at one lattice point: B's ring is a closed arc with one node"""
    L = np.zeros((8, 8), np.int64)
    L[2:4, 2:4] = 1
    L[4:6, 4:6] = 2
    return L


def notch():
    """A = rows 0-4, C = rows 5-8 on 9 x 10, B = row 4, x in 3..6, cut out of A on the border: B's ring holds two nodes, (3, 5)
    and (7, 5), and the arc over it lies 1 px from the chord between them"""
    L = np.zeros((9, 10), np.int64)
    L[5:] = 2
    L[4, 3:7] = 1
    return L


def pinned_hole():
    """a 6 x 6 frame A, one pixel thick, alone in the background; inside it B (top), C and D (bottom left and right): the hole
    ring of A holds three nodes that are not collinear, so it stays at any tolerance -- until A's outer ring, a closed arc
    without a node, collapses (a corner is 6 / sqrt 2 = 4.24 from the diagonal) and takes the hole with it"""
    L = np.full((8, 8), -1, np.int64)
    L[1:7, 1:7] = 0
    L[2:4, 2:6] = 1
    L[4:6, 2:4] = 2
    L[4:6, 4:6] = 3
    return L


def long_wall(horizontal=True):
    """A over five instances of widths 7, 20, 1, 30, 22 along an 80-step wall: four nodes inside one straight segment"""
    L = np.zeros((8, 80), np.int64)
    for i, (a, b) in enumerate(((0, 7), (7, 27), (27, 28), (28, 58), (58, 80))):
        L[4:, a:b] = i + 1
    return L if horizontal else np.ascontiguousarray(L.T)


def stairs_with_tee(n, tee):
    """instance 0 = the staircase of n steps (2 n + 2 corners) one column into an n x (n + 1) canvas; tee: instance 1 in column
    0 from the top down to row n // 2, whose lower end is a T-junction inside the staircase's straight left wall: 2 n + 3"""
    L = np.full((n, n + 1), -1, np.int64)
    L[:, 1:][np.tri(n, n, dtype=bool)] = 0
    if tee:
        L[:n // 2, 0] = 1
    return L, 2 if tee else 1


def orientations(L):
    L = np.asarray(L)
    return [L, L[::-1], L.T, L.T[:, ::-1]]


def hand_maps():
    """(name, label map, k) of every hand-built case"""
    out = [('two rectangles', np.repeat([[0, 1]], 6, 0).repeat(4, 1), 2)]
    out += [(f'two rectangles, free-standing {i}', np.pad(m, 1, constant_values=-1), 2)
            for i, m in enumerate(orientations(np.repeat([[0, 1]], 3, 0).repeat(5, 1))[:3:2])]
    out += [(f'T-junction {i}', m, 3) for i, m in enumerate(orientations(t_junction()))]            # inside above, below, left, right
    out += [(f'border T {i}', m, 2) for i, m in enumerate(orientations(np.repeat([[0, 0, 1]], 5, 0).repeat(2, 1)))]
    out.append(('four regions', np.repeat(np.repeat([[0, 1], [2, 3]], 3, 0), 4, 1), 4))
    out.append(('saddle A / B', np.repeat(np.repeat([[0, 1], [1, 0]], 3, 0), 3, 1), 2))
    out.append(('saddle A / background', np.repeat(np.repeat([[0, -1], [-1, 0]], 3, 0), 3, 1), 1))
    out.append(('square island', framed(np.ones((4, 4), bool)), 2))
    out.append(('diamond island', framed(scases.diamond(4)), 2))
    out.append(('disc island', framed(scases.disc(6)), 2))
    out.append(('touching islands', touching_islands(), 3))
    out.append(('diagonal', diagonal_split(), 2))
    out.append(('slope 2', slope2_split(), 2))
    out.append(('notch', notch(), 3))
    out.append(('pinned hole', pinned_hole(), 4))
    out.append(('full canvas', np.zeros((5, 7), np.int64), 1))
    out.append(('empty rows', np.where(np.arange(6)[None] < 3, 1, 3).repeat(4, 0), 5))              # rows 0, 2, 4 have no pixel
    out.append(('H = 1', np.asarray([[0, 0, 1, -1, 2, 2, 2]]), 3))
    out.append(('W = 1', np.asarray([[0, 0, 1, -1, 2, 2, 2]]).T.copy(), 3))
    out.append(('1 x 1', np.zeros((1, 1), np.int64), 1))
    out.append(('long wall', long_wall(True), 6))
    out.append(('long wall, vertical', long_wall(False), 6))
    return out


def random_map(rng):
    """the prototype's maps: 2 .. 19 a side, 1-5 Voronoi regions plus background, 15 % of the pixels relabelled"""
    H, W, k = int(rng.integers(2, 20)), int(rng.integers(2, 20)), int(rng.integers(1, 6))
    pts = rng.integers(0, [H, W], (k + 1, 2))
    yy, xx = np.mgrid[:H, :W]
    L = ((yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2).argmin(-1) - 1
    flip = rng.random((H, W)) < 0.15
    L[flip] = rng.integers(-1, k, int(flip.sum()))
    return L, k


def voronoi(H, W, k, seed, noise=0.15):
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, [H, W], (k, 2))
    yy, xx = np.mgrid[:H, :W]
    L = ((yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2).argmin(-1)
    flip = rng.random((H, W)) < noise
    L[flip] = rng.integers(0, k, int(flip.sum()))
    return L


# -------------------------------------------------------------------------------------------------------------- helpers
_NODED, _WANT = {}, {}


def noded_of(key, L, k):
    if key is None:
        return cref.noded(L, k)
    if key not in _NODED:
        _NODED[key] = cref.noded(L, k)
    return _NODED[key]


def want_of(key, L, k, tolerance):
    """the reference's nine arrays, computed once per (key, tolerance) and shared between the tests"""
    q8 = sref.tol2_q8(tolerance)
    if key is None or (key, q8) not in _WANT:
        want = cref.coverage(L, k, q8, pre=noded_of(key, L, k))
        if key is None:
            return want
        _WANT[(key, q8)] = want
    return _WANT[(key, q8)]


def table(L, k, dev, cap=None):
    return seam_cases.rows_from_masks(cref.masks_of(L, k), dev, cap)


def assert_equal(got, want, what=''):
    assert len(got) == len(want) == 9, what
    for name, g, w in zip(NAMES, got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert g.dtype == w.dtype, f'{what}: {name} is {g.dtype}, expected {w.dtype}'
        assert tuple(g.shape) == tuple(w.shape), f'{what}: {name} has shape {tuple(g.shape)}, expected {tuple(w.shape)}'
        assert torch.equal(g.cpu(), w), f'{what}: {name} differs'


def check(ops, dev, key, L, k, tolerances=TOLERANCES, variants=(0,)):
    L = np.asarray(L)
    H, W = L.shape
    counts, n = table(L, k, dev)
    for tol in tolerances:
        want = want_of(key, L, k, tol)
        for v in variants:
            got = ops.ring_coverage(counts, n, H, W, sref.tol2_q8(tol), with_rounds=True, variant=v)
            assert_equal(got, want, f'{key} at tolerance {tol}, variant {v}')
            assert all(g.device.type == torch.device(dev).type for g in got)
    return want


def twins_unmatched(result, lost=()):
    return cref.unmatched_twins(cref.directed_edges(result[0], result[1], result[2], result[7]), lost)


# ---------------------------------------------------------------------------------------------------- the reference itself
def check_reference_on(key, L, k):
    """twin edges (between instances that lost no ring), every node kept, every dropped vertex within the tolerance (fractions),
    kept sets nested over the tolerances, tolerance 0 minus the non-corner nodes = the traced rings"""
    nod = noded_of(key, L, k)
    arrays, flags, _ = nod
    last = None
    for tol in reversed(NESTED):
        q8 = sref.tol2_q8(tol)
        res = want_of(key, L, k, tol)
        cref.check_properties(L, k, nod, res, q8)
        pts = {(r, tuple(p)) for r, a, b in zip(res[6].tolist(), res[1][:-1].tolist(), res[1][1:].tolist())
               for p in res[0][a:b].tolist()}
        assert last is None or last <= pts, (key, tol)
        last = pts
    exact = want_of(key, L, k, 0)
    assert all(np.array_equal(a, b) for a, b in zip(exact[:6], arrays)) and exact[6].tolist() == list(range(len(flags)))
    v, ro = arrays[0].tolist(), arrays[1].tolist()
    r = 0
    for i in range(k):
        for ring, par, a2 in pref.trace(np.asarray(L) == i):
            corners = [tuple(p) for p in ring.tolist()]
            mine = [tuple(p) for p in v[ro[r]:ro[r + 1]]]
            m = len(mine)
            keep = [p for t, p in enumerate(mine)                          # a corner: the direction changes there
                    if (mine[t - 1][0] == p[0]) != (mine[(t + 1) % m][0] == p[0])]
            s = keep.index(min(keep))
            assert keep[s:] + keep[:s] == corners and (arrays[3][r], arrays[4][r]) == (par, a2), (key, i)
            r += 1
    assert r == len(flags)


def check_reference():
    for name, L, k in hand_maps():
        check_reference_on(name, L, k)
    rng = np.random.default_rng(20261021)
    for t in range(300):
        L, k = random_map(rng)
        check_reference_on(('random', t), L, k)
    return len(_WANT)


# ------------------------------------------------------------------------------------------------------- discriminating
def check_shared_borders_match(apis, rle, dev):
    """the diagonal split and the T-junction: rings simplified one by one do not fit together, topology='shared' ones do"""
    import inspect
    assert 'topology' in inspect.signature(apis.masks_to_polygons).parameters
    for L, k, tols in ((diagonal_split(), 2, (0.5, 1.0, 1.5, 2.0)), (t_junction(), 3, (1.0,))):
        H, W = L.shape
        dense = torch.from_numpy(np.stack(cref.masks_of(L, k))).to(dev)
        counts, n, size, _ = rle.masks_to_runs(dense, dev, 'test')
        for tol in tols:
            alone, _ = rle.simplify_polygons(rle.runs_to_polygons(counts, n, size), size, tol)
            edges = {}
            v, ro, inst = alone[0].cpu().tolist(), alone[1].cpu().tolist(), alone[2].cpu().tolist()
            for r, i in enumerate(inst):                                   # an inner edge of the layer has a twin in another ring
                pts = [tuple(p) for p in v[ro[r]:ro[r + 1]]]
                for t, p in enumerate(pts):
                    q = pts[(t + 1) % len(pts)]
                    on_border = (p[0] == q[0] and p[0] in (0, W)) or (p[1] == q[1] and p[1] in (0, H))
                    if not on_border:
                        edges[(p, q)] = edges.get((p, q), 0) + 1
            assert any(edges.get((q, p), 0) != c for (p, q), c in edges.items()), (L.shape, tol)     # gaps or slivers
            polys, src, other = rle.simplify_coverage(counts, n, size, tol)
            got = tuple(t.cpu().numpy() for t in polys) + (src.cpu().numpy(), other.cpu().numpy())
            assert twins_unmatched(got) == 0 and len(src) == k
            rings = apis.masks_to_polygons(dense, tolerance=tol, topology='shared')
            assert [r[0].tolist() for inst_ in rings for r in inst_] == [got[0][a:b].tolist() for a, b in zip(got[1][:-1], got[1][1:])]
    rings = apis.masks_to_polygons(torch.from_numpy(np.stack(cref.masks_of(t_junction(), 3))).to(dev), tolerance=0, topology='shared')
    assert [5, 4] in rings[0][0][0].tolist() and len(rings[0][0][0]) == 5                            # A follows B and C there
    assert [5, 4] not in apis.masks_to_polygons(torch.from_numpy(np.stack(cref.masks_of(t_junction(), 3))).to(dev))[0][0][0].tolist()


# -------------------------------------------------------------------------------------------------------------- kernels
def check_hand_maps(ops, dev):
    for name, L, k in hand_maps():
        check(ops, dev, name, L, k, variants=(0, 3))


def check_closed_arcs(ops, dev):
    """islands in a frame: closed arcs without a node, as outer ring and as the hole around it -- both are anchored at the same
    point and keep the same vertices.  A four-vertex square has no tie (the corner opposite its anchor is the one farthest
    vertex), so the diamond and the disc decide the ties on which lowest-index and smallest-point differ"""
    cref.reset_stats()
    for name, island in (('square island', np.ones((4, 4), bool)), ('diamond island', scases.diamond(4)),
                         ('disc island', scases.disc(6))):
        L = framed(island)
        for tol in TOLERANCES:
            want = cref.coverage(L, 2, sref.tol2_q8(tol))
            assert_equal(ops.ring_coverage(*table(L, 2, dev), *L.shape, sref.tol2_q8(tol), with_rounds=True), want, name)
            per = cref.lists(want)
            if len(per[0]) == 2 and len(per[1]) == 1:                      # frame outer + hole, island
                hole, isl = per[0][1][0].tolist(), per[1][0][0].tolist()
                assert hole[0] == isl[0] == min(isl) and hole[1:] == isl[1:][::-1], (name, tol)
                assert set(per[1][0][3].tolist()) == {0} and set(per[0][1][3].tolist()) == {1}
    assert cref.STATS['closed_chains'] > 0 and cref.STATS['ties_differ'] > 0, cref.STATS
    return dict(cref.STATS)


def check_one_node_arc(ops, dev):
    L = touching_islands()
    arrays, flags, _ = noded_of('touching islands', L, 3)
    # A's foreground is 8-connected, so B and C sit in a hole each: A's outer ring has no node, the four others one, and begin there
    assert [sum(f) for f in flags] == [0, 1, 1, 1, 1] and arrays[3].tolist() == [-1, 0, 0, -1, -1]
    assert [arrays[0][s].tolist() for s in arrays[1][1:-1]] == [[4, 4]] * 4
    check(ops, dev, 'touching islands', L, 3, variants=(0, 3))


def check_collapse(ops, dev):
    """the notch: at tolerance 1 B keeps its two nodes only and goes; A and C stay and follow each other over the chord"""
    L = notch()
    want = check(ops, dev, 'notch', L, 3, variants=(0, 3))
    w = want_of('notch', L, 3, 1)
    assert w[6].tolist() == [0, 2] and w[5].tolist() == [0, 1, 1, 2]
    assert w[0].tolist() == [[10, 5], [7, 5], [3, 5], [0, 5], [0, 0], [10, 0],
                             [0, 5], [3, 5], [7, 5], [10, 5], [10, 9], [0, 9]]
    assert w[7].tolist() == [2, 1, 2, -1, -1, -1, 0, 1, 0, -1, -1, -1]
    assert twins_unmatched(w, lost={1}) == 0
    w = want_of('notch', L, 3, 0.5)                                        # below 1 px everything stays
    assert w[6].tolist() == [0, 1, 2] and len(w[0]) == 8 + 4 + 6           # C: four corners and the two nodes in its top wall
    return want


def check_hole_loses_parent(ops, dev):
    L = pinned_hole()
    check(ops, dev, 'pinned hole', L, 4, variants=(0, 3))
    arrays, flags, _ = noded_of('pinned hole', L, 4)
    assert arrays[3].tolist()[:2] == [-1, 0] and sum(flags[0]) == 0 and sum(flags[1]) == 3
    hole = [tuple(p) for p in arrays[0][arrays[1][1]:arrays[1][2]].tolist()]
    assert len(cref.simplify_arcs(hole, flags[1], sref.tol2_q8(5))[0]) == 3                            # it would stay on its own
    w = want_of('pinned hole', L, 4, 5)
    assert 0 not in w[2].tolist() and w[5].tolist()[:2] == [0, 0] and 1 not in w[6].tolist()
    w = want_of('pinned hole', L, 4, 2)
    assert w[6].tolist()[:2] == [0, 1] and w[3].tolist()[:2] == [-1, 0]


def check_empty_calls(ops, dev):
    z = torch.zeros((0, 4), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev)
    got = ops.ring_coverage(*z, 5, 6, 256, with_rounds=True)
    assert [tuple(g.shape) for g in got] == [(0, 2), (1,), (0,), (0,), (0,), (1,), (0,), (0,), (0,)]
    counts, n = seam_cases.rows_from_counts([[30], None, [30]], dev)       # rows without a pixel only
    with ReadCounter(dev) as rc:
        got = ops.ring_coverage(counts, n, 5, 6, 256, with_rounds=True)
    assert rc.n == 1 and got[5].cpu().tolist() == [0, 0, 0, 0] and got[0].shape[0] == 0 and got[7].shape[0] == 0
    L = np.zeros((3, 3), np.int64)                                         # every ring collapses
    got = ops.ring_coverage(*table(L, 1, dev), 3, 3, sref.tol2_q8(100), with_rounds=True)
    assert_equal(got, want_of(None, L, 1, 100))
    assert got[0].shape[0] == 0 and got[8].cpu().tolist() == [1]


def check_lengths(ops, dev):
    """noded ring lengths on both sides of the wave path's end (64) and of the block path's chunk boundary (256), and one that
    does not fit LDS (above 2048): staircases, the odd lengths by a T-junction in the straight wall"""
    lengths = []
    for n_, tee in ((30, True), (31, False), (31, True), (126, True), (127, False), (127, True), (1030, False)):
        L, k = stairs_with_tee(n_, tee)
        arrays, _, _ = noded_of(('stairs', n_, tee), L, k)
        lengths.append(int(arrays[1][1]))
        check(ops, dev, ('stairs', n_, tee), L, k, tolerances=(0.5, 2) if n_ < 1000 else (1,),
              variants=(0, 1, 2, 3) if n_ < 1000 else (0,))
    assert lengths == [63, 64, 65, 255, 256, 257, 2062], lengths
    return lengths


def check_long_wall(ops, dev):
    for horizontal in (True, False):
        L = long_wall(horizontal)
        key = 'long wall' if horizontal else 'long wall, vertical'
        arrays, flags, others = noded_of(key, L, 6)
        assert int(arrays[1][1]) == 4 + 4 and sum(flags[0]) == 4 + 2      # A: four corners, four inserted nodes; two corners are nodes
        assert sorted(set(others[0])) == [-1, 1, 2, 3, 4, 5]
        check(ops, dev, key, L, 6, variants=(0, 3))
    # the same wall between two instances only: 79 unit steps without a node
    L = np.zeros((8, 80), np.int64)
    L[4:] = 1
    check(ops, dev, None, L, 2, tolerances=(0, 1))
    check(ops, dev, None, np.ascontiguousarray(L.T), 2, tolerances=(0, 1))


def check_random(ops, dev, count=300):
    """the prototype's label maps at its tolerances; every counter of the reference moves"""
    cref.reset_stats()
    rng = np.random.default_rng(20261021)
    edges = 0
    for t in range(count):
        L, k = random_map(rng)
        check(ops, dev, ('random', t), L, k, tolerances=NESTED)
        edges += sum(len(want_of(('random', t), L, k, tol)[0]) for tol in NESTED)
    return edges


def check_random_stats(count=300):
    """the counters of the reference over the random maps, on a pass of its own (the shared results are cached)"""
    cref.reset_stats()
    rng = np.random.default_rng(20261021)
    for t in range(count):
        L, k = random_map(rng)
        nod = cref.noded(L, k)                                             # (inserted nodes are counted while noding)
        for tol in NESTED:
            cref.coverage(L, k, sref.tol2_q8(tol), pre=nod)
    stats = dict(cref.STATS)
    assert all(v > 0 for v in stats.values()), stats
    return stats


def check_protocol(ops, rle, dev):
    """poisoned output buffers and a second launch: the same bits; the documented host reads; a table wider than its rows"""
    L = voronoi(40, 37, 7, 3)
    H, W = L.shape
    counts, n = table(L, 7, dev)
    q8 = sref.tol2_q8(1)
    want = want_of('protocol', L, 7, 1)
    outs = []
    for byte in (0xFF, 0x55):
        with Poison(byte):
            outs.append(ops.ring_coverage(counts, n, H, W, q8, with_rounds=True))
        assert_equal(outs[-1], want, f'poison {byte:#x}')
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    with ReadCounter(dev) as rc:
        got = ops.ring_coverage(counts, n, H, W, q8)
    assert rc.n == 5 and len(got) == 8, rc.n                               # the documented five
    with ReadCounter(dev) as rc:
        polys, src, other = rle.simplify_coverage(counts, n, (H, W), 1.0)
    assert rc.n == 5 and len(polys) == 6 and torch.equal(src, got[6]) and torch.equal(other, got[7])
    wide, _ = table(L, 7, dev, cap=3000)
    assert_equal(ops.ring_coverage(wide, n, H, W, q8, with_rounds=True), want, 'wide table')
    assert_equal(ops.ring_coverage(wide, n, H, W, q8, with_rounds=True, variant=3), want, 'block path')


def check_refusals(ops, rle, apis, dev, pytest):
    L = t_junction()
    counts, n = table(L, 3, dev)
    assert len(ops.ring_coverage(counts, n, 8, 12, 256)) == 8
    for bad in (-1, 2 ** 40 + 1, 1.5, None, True):
        with pytest.raises(ValueError, match='tol2_q8'):
            ops.ring_coverage(counts, n, 8, 12, bad)
    over = [m.copy() for m in cref.masks_of(L, 3)]
    over[0][4, 2] = True                                                  # one pixel of B also in A
    oc, on = seam_cases.rows_from_masks(over, dev)
    with pytest.raises(ValueError, match='overlap.*flatten_masks'):
        ops.ring_coverage(oc, on, 8, 12, 256)
    with pytest.raises(ValueError, match='overlap'):
        rle.simplify_coverage(oc, on, (8, 12), 1.0)
    with pytest.raises(ValueError, match='overlap'):
        apis.masks_to_polygons(torch.from_numpy(np.stack(over)).to(dev), tolerance=1.0, topology='shared')
    nc, nn = seam_cases.rows_from_counts([[2, 3, 0, 2, 89], [40, 8, 48]], dev)     # a zero count inside row 0
    with pytest.raises(ValueError, match='canonical'):
        ops.ring_coverage(nc, nn, 8, 12, 256)
    with pytest.raises(ValueError, match='canonical|zero'):
        apis.masks_to_polygons([dict(size=[8, 12], counts=[2, 3, 0, 2, 89])], tolerance=1.0, topology='shared', device=dev)
    dense = torch.from_numpy(np.stack(cref.masks_of(L, 3))).to(dev)
    for bad in (1, 2.0, 30):
        with pytest.raises(ValueError, match='min_ring_area == 0.*nobody'):
            apis.masks_to_polygons(dense, tolerance=1.0, min_ring_area=bad, topology='shared')
    with pytest.raises(ValueError, match='requires a tolerance'):
        apis.masks_to_polygons(dense, topology='shared')
    for bad in ('arcs', None, 1, 'Shared'):
        with pytest.raises(ValueError, match='topology'):
            apis.masks_to_polygons(dense, tolerance=1.0, topology=bad)
    for bad in (-1.0, float('nan'), 65536.5):
        with pytest.raises(ValueError, match='tolerance'):
            apis.masks_to_polygons(dense, tolerance=bad, topology='shared')
    big, bn = seam_cases.rows_from_counts([[0, 2 ** 20 + 1]], dev)
    with pytest.raises(ValueError, match='2\\^20'):
        ops.ring_coverage(big, bn, 1, 2 ** 20 + 1, 256)
    with pytest.raises(ValueError, match='2\\^20'):
        rle.simplify_coverage(big, bn, (2 ** 20 + 1, 1), 1.0)
    with pytest.raises(ValueError, match='32-bit'):
        ops.ring_coverage(big, bn, 65536, 32768, 256)
    # the C entry points, without a launch that reads anything
    lib = ops._lib.load()
    buf = torch.zeros((64,), dtype=torch.int64, device=dev)
    p, side = buf.data_ptr(), 2 ** 20
    BIG = ops.CONST['RSP_RUN_PIECES_MAX_PIECES'] + 1
    chk = lambda *a: lib.rsp_ring_coverage_check(*a, 0)                              # noqa: E731
    assert chk(p, 0, 3, 4, p) == 0 and chk(p, 1, 3, 4, p) == 0
    assert chk(p, 1, side + 1, 4, p) != 0 and chk(p, 1, 3, side + 1, p) != 0 and chk(p, 1, 65536, 32768, p) != 0
    assert chk(p, -1, 3, 4, p) != 0 and chk(p, BIG, 3, 4, p) != 0 and chk(0, 1, 3, 4, p) != 0 and chk(p, 1, 3, 4, 0) != 0
    assert chk(p, 1, 0, 4, p) != 0
    cnt = lambda *a: lib.rsp_ring_coverage_nodes_count(*a, 0)                        # noqa: E731
    ok = [p, p, 1, 0, p, p, 1, 1, 3, 4, p, p]                                          # V = 0: nothing to do
    assert cnt(*ok) == 0
    for at, bad in ((2, -1), (3, -1), (5, 0), (6, -1), (6, BIG), (7, -1), (8, side + 1), (9, side + 1), (8, 0)):
        v = list(ok)
        v[at] = bad
        assert cnt(*v) != 0, at
    ok[3] = 1
    for at in (0, 1, 4, 10, 11):
        v = list(ok)
        v[at] = 0
        assert cnt(*v) != 0, at
    wr = lambda *a: lib.rsp_ring_coverage_nodes_write(*a, 0)                         # noqa: E731
    ok = [p, p, 1, 0, p, p, 1, 1, 3, 4, p, p, 0, p, p, p]
    assert wr(*ok) == 0
    ok[3], ok[12] = 1, 1
    for at, bad in ((0, 0), (1, 0), (10, 0), (11, 0), (13, 0), (14, 0), (15, 0), (12, 0), (12, 2 ** 31), (8, side + 1), (7, -1)):
        v = list(ok)
        v[at] = bad
        assert wr(*v) != 0, at
    mark = lambda *a: lib.rsp_ring_coverage_mark(*a, 0)                              # noqa: E731
    assert mark(p, p, 1, 4, 256, 9, 9, 0, p, p, p, p, p) == 0                         # one ring without vertices
    assert mark(p, p, 1, 4, -1, 9, 9, 0, p, p, p, p, p) != 0 and mark(p, p, 1, 4, 2 ** 40 + 1, 9, 9, 0, p, p, p, p, p) != 0
    assert mark(p, p, 1, 4, 256, side + 1, 9, 0, p, p, p, p, p) != 0 and mark(p, p, 1, 4, 256, 9, 9, 4, p, p, p, p, p) != 0
    assert mark(p, 0, 1, 4, 256, 9, 9, 0, p, p, p, p, p) != 0 and mark(p, p, 1, 4, 256, 9, 9, 0, 0, p, p, p, p) != 0
    oth = lambda *a: lib.rsp_ring_coverage_other(*a, 0)                              # noqa: E731
    assert oth(p, 1, 4, p, p, p, p, 0, p, p) == 0
    for at, bad in ((1, -1), (2, -1), (7, 5), (7, -1)):
        v = [p, 1, 4, p, p, p, p, 1, p, p]
        v[at] = bad
        assert oth(*v) != 0, at
    for at in (0, 3, 4, 5, 6, 8, 9):
        v = [p, 1, 4, p, p, p, p, 1, p, p]
        v[at] = 0
        assert oth(*v) != 0, at
    if torch.device(dev).type != 'cpu':
        torch.cuda.synchronize()
    del buf


# ------------------------------------------------------------------------------------------------------------------ API
def _lists_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for (gr, gp, ga), (wr, wp, wa, _) in zip(g, w):
            assert gr.dtype == np.int32 and np.array_equal(gr, wr) and (gp, ga) == (wp, wa)


def check_api_forms(apis, rle, dev):
    """the three input forms and the three output forms; the defaults are the calls without the new argument"""
    import _large_image_ref as lref
    L = voronoi(24, 30, 5, 9)
    L[10:14, 12:18] = -1
    H, W = L.shape
    masks = cref.masks_of(L, 5)
    dense = torch.from_numpy(np.stack(masks)).to(dev)
    lists = [dict(size=[H, W], counts=lref.rle_counts_np(m)) for m in masks]
    strings = [dict(size=[H, W], counts=rle.counts_to_string(lref.rle_counts_np(m))) for m in masks]
    for form in ('rings', 'coco', 'geojson'):
        for kw in (dict(), dict(tolerance=1.0), dict(tolerance=2, min_ring_area=3)):
            a, b = apis.masks_to_polygons(dense, form=form, **kw), apis.masks_to_polygons(dense, form=form, topology='rings', **kw)
            assert (a == b) if form != 'rings' else all(np.array_equal(x[0], y[0]) and x[1:] == y[1:]
                                                        for p, q in zip(a, b) for x, y in zip(p, q))
    for tol in (0, 1.0, 2):
        want = cref.lists(want_of(('api', 0), L, 5, tol))
        for src in (dense, lists, strings):
            _lists_equal(apis.masks_to_polygons(src, device=dev, tolerance=tol, topology='shared'), want)
        coco = apis.masks_to_polygons(dense, form='coco', tolerance=tol, topology='shared')
        for entry, w in zip(coco, want):
            assert entry['polygons'] == [[float(c) for c in ring.reshape(-1).tolist()] for ring, _, a2, _ in w if a2 > 0]
        geo = apis.masks_to_polygons(dense, form='geojson', tolerance=tol, topology='shared', transform=(10.0, 2.0, 0.0, 5.0, 0.0, -2.0))
        edges = {}
        for i, g in enumerate(geo):                                       # neighbouring features share their border coordinates
            for poly in ([g['coordinates']] if g['type'] == 'Polygon' else g['coordinates']):
                for ring in poly:
                    assert ring[0] == ring[-1]
                    for p, q in zip(ring[:-1], ring[1:]):
                        edges[(tuple(p), tuple(q))] = edges.get((tuple(p), tuple(q)), 0) + 1
        res = want_of(('api', 0), L, 5, tol)
        lost = cref.lost_instances(noded_of(('api', 0), L, 5)[0][5], res)
        if not lost:
            inner = sum(1 for o in res[7].tolist() if o >= 0)
            assert sum(c for (p, q), c in edges.items() if edges.get((q, p), 0) == c) == inner and inner > 0


# ------------------------------------------------------------------------------------------------------------- pipeline
def check_pipeline(li, dev, model, merge, region):
    """inference_large_image(masks='polygons', flatten='score', polygon_topology='shared') against the reference applied to
    the label map of the same call with masks='rle'; the defaults; the refusals that come before the first tile"""
    scene = np.random.default_rng(16).integers(0, 256, (45, 70, 3)).astype(np.uint8)
    kw = dict(patch_size=32, batch_size=2, merge_iou_thr=0.25, merge_nms_type=merge, min_mask_region_area=region)
    if merge == 'seam_mask':
        kw['seam_iou_thr'] = 0.3
    flat = li.inference_large_image(model, scene, flatten='score', **kw).pred_instances
    K = len(flat.scores)
    dense = fcases._dense_of(flat.masks, 'strings', 45, 70)
    L = cref.labels_of(list(dense), 45, 70)
    for tol in (0, 1.0):
        out = li.inference_large_image(model, scene, masks='polygons', flatten='score', polygon_tolerance=tol,
                                       polygon_topology='shared', **kw).pred_instances
        want = want_of(('pipeline', merge, region), L, K, tol)
        _lists_equal(out.masks, cref.lists(want))
        assert torch.equal(out.bboxes, flat.bboxes) and torch.equal(out.flatten_kept, flat.flatten_kept)
        assert twins_unmatched(want, cref.lost_instances(noded_of(('pipeline', merge, region), L, K)[0][5], want)) == 0
    a = li.inference_large_image(model, scene, masks='polygons', flatten='score', polygon_tolerance=1.0, **kw).pred_instances
    b = li.inference_large_image(model, scene, masks='polygons', flatten='score', polygon_tolerance=1.0, polygon_topology='rings',
                                 **kw).pred_instances
    assert all(np.array_equal(x[0], y[0]) and x[1:] == y[1:] for p, q in zip(a.masks, b.masks) for x, y in zip(p, q))
    return K


def check_pipeline_refusals(li, model, pytest):
    scene = np.random.default_rng(16).integers(0, 256, (45, 70, 3)).astype(np.uint8)

    class Never(type(model)):
        def test_step(self, data):
            raise AssertionError('a tile ran before the refusal')
    never = Never((32, 32))
    kw = dict(patch_size=32, polygon_topology='shared')
    with pytest.raises(ValueError, match="masks='polygons'"):
        li.inference_large_image(never, scene, flatten='score', **kw)
    with pytest.raises(ValueError, match='flatten'):
        li.inference_large_image(never, scene, masks='polygons', polygon_tolerance=1.0, **kw)
    with pytest.raises(ValueError, match='requires a tolerance'):
        li.inference_large_image(never, scene, masks='polygons', flatten='score', **kw)
    with pytest.raises(ValueError, match='min_ring_area == 0'):
        li.inference_large_image(never, scene, masks='polygons', flatten='score', polygon_tolerance=1.0, polygon_min_ring_area=2, **kw)
    with pytest.raises(ValueError, match='topology'):
        li.inference_large_image(never, scene, masks='polygons', flatten='score', polygon_tolerance=1.0, patch_size=32,
                                 polygon_topology='arcs')


# ------------------------------------------------------------------------------------------------------- properties only
def scene_600(rle, dev):
    """the 600-row scene of DESIGN §14.14 (300 blobs of 128 x 128 on 8 192 x 9 000 and their copies moved by up to six
    pixels), flattened by a random rank -> (counts, n, size)"""
    from scipy import ndimage
    rng = np.random.default_rng(300)
    th, tw, H, W, k = 128, 128, 8192, 9000, 300
    f = ndimage.gaussian_filter(rng.random((k, th, tw)), (0, 3, 3))
    tiles = torch.from_numpy(f > np.quantile(f, 0.55)).to(dev)
    offs = np.stack([rng.integers(0, W - tw + 1, k), rng.integers(0, H - th + 1, k)], 1).astype(np.int32)
    jit = np.clip(offs + rng.integers(-6, 7, offs.shape), 0, [W - tw, H - th]).astype(np.int32)
    counts, n, _, _ = rle.encode_runs(tiles)
    parts = [rle.shift_runs(counts, n, torch.from_numpy(o).to(dev), (th, tw), (H, W))[:2] for o in (offs, jit)]
    sc, sn = rle.concat_runs([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    rank = np.random.default_rng(1).permutation(2 * k).astype(np.int32)
    fc, fn = rle.flatten_runs(sc, sn, (H, W), rank)[:2]
    return fc, fn, (H, W)


def check_scene_properties(result, exact, labels, k):
    """a result on the device too large for the sequential reference, with `exact` = the call at tolerance 0 (the noded rings)
    and the label map of the table (0: background, i + 1): offsets consistent, twin edges matched through vert_other between
    instances without a dropped ring, every node of a surviving ring kept, fewer vertices than noded (all vectorised)
    -> (V', twin edges, nodes)"""
    v, ro, inst, par, a2, io, src, other = (t.cpu().numpy() for t in result[:8])
    ev, ero, eio, esrc = (exact[i].cpu().numpy() for i in (0, 1, 5, 6))
    noded_total = len(ev)
    assert esrc.tolist() == list(range(len(esrc)))                        # tolerance 0 drops nothing
    lab = torch.nn.functional.pad(labels, (1, 1, 1, 1))
    a, b, c, d = lab[:-1, :-1], lab[:-1, 1:], lab[1:, :-1], lab[1:, 1:]
    node = ((a != b).to(torch.uint8) + (b != d) + (d != c) + (c != a)) >= 3
    is_node = node[torch.from_numpy(ev[:, 1].astype(np.int64)).to(node.device),
                   torch.from_numpy(ev[:, 0].astype(np.int64)).to(node.device)].cpu().numpy()
    pack = lambda r, p: (r.astype(np.int64) << 42) | (p[:, 0].astype(np.int64) << 21) | p[:, 1]       # noqa: E731
    e_ring = np.repeat(np.arange(len(esrc)), np.diff(ero))
    need = pack(e_ring, ev)[is_node & np.isin(e_ring, src)]
    have = pack(np.repeat(src, np.diff(ro)), v)
    assert len(need) > 0 and np.isin(need, have).all()
    lost = np.flatnonzero(np.diff(eio) != np.diff(io))
    R2, V2 = len(inst), len(v)
    assert ro[0] == 0 and ro[-1] == V2 and (np.diff(ro) >= 3).all() and len(ro) == R2 + 1 and len(other) == V2
    assert io[0] == 0 and io[-1] == R2 and (np.diff(io) >= 0).all() and len(io) == k + 1
    assert (np.diff(inst) >= 0).all() and (np.diff(src) > 0).all() and (a2 != 0).all() and ((par >= 0) == (a2 < 0)).all()
    assert (inst == np.repeat(np.arange(k), np.diff(io))).all() and ((other >= -1) & (other < k)).all()
    assert V2 < noded_total
    ring_of = np.repeat(np.arange(R2), np.diff(ro))
    nxt = np.arange(1, V2 + 1)
    nxt[ro[1:] - 1] = ro[:-1]
    vi = inst[ring_of].astype(np.int64)
    assert (other != vi).all()
    key = lambda p: p[:, 0].astype(np.int64) * (1 << 21) + p[:, 1]                   # noqa: E731
    u, w = key(v), key(v[nxt])
    sel = (other >= 0) & ~np.isin(vi, lost) & ~np.isin(other, lost)
    fwd = np.stack([u[sel], w[sel], vi[sel], other[sel].astype(np.int64)], 1)
    bwd = np.stack([w[sel], u[sel], other[sel].astype(np.int64), vi[sel]], 1)
    order = lambda e: e[np.lexsort(e.T[::-1])]                                       # noqa: E731
    assert len(fwd) > 0 and np.array_equal(order(fwd), order(bwd))        # the multiset of edges is the multiset of twins
    return V2, len(fwd), len(need)
