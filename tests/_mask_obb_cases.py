"""Bodies of the oriented-box tests (csrc/mask_obb.hip, ops.mask_hull / ops.hull_min_rect, rle.runs_to_obb, apis.masks_to_obb,
large_image oriented_boxes=True), shared by both tiers: tests/test_mask_obb_cpu.py calls them with the emulated
`ops` on CPU tensors, tests/test_gpu_mask_obb.py with the real ones on cuda:0.  The reference is tests/_mask_obb_ref.py, the
sequential definition in Python integers and fractions; the five integer arrays are compared with torch.equal, the float forms
against the Fraction reference at rtol = 1e-12.  The run tables come from tests/_large_image_ref.py's numpy encoder (or are
written by hand), not from the kernels under test."""
import math

import numpy as np
import torch

import _large_image_ref as lref
import _mask_obb_ref as oref
import _mask_polygons_cases as pcases
import _seam_merge_cases as seam_cases

NAMES = ('hull_verts', 'hull_offs', 'hull_area2', 'edge', 'q')
RTOL = 1e-12
# the path boundaries of csrc/mask_obb.hip: MO_THREADS records / points a chunk, MO_LDS_PTS / 2 records a chain in LDS,
# MO_RECT_LDS hull vertices in LDS
THREADS, LDS_RECORDS, RECT_LDS = 256, 2048, 1024


# ----------------------------------------------------------------------------------------------------------- the masks
def _pix(h, w, pixels):
    m = np.zeros((h, w), bool)
    for x, y in pixels:
        m[y, x] = True
    return m


def known_answers():
    """(name, mask, hull, edge, q or None, area) as the issue states them"""
    blk = np.zeros((5, 6), bool)
    blk[1:4, 2:5] = True
    return [
        ('single pixel', _pix(3, 3, [(0, 0)]), [(0, 0), (1, 0), (1, 1), (0, 1)], 0, (1, 0, 0, 1, 0, 1), 1),
        ('two diagonal pixels', _pix(3, 3, [(0, 0), (1, 1)]), [(0, 0), (1, 0), (2, 1), (2, 2), (1, 2), (0, 1)], 0,
         (1, 0, 0, 2, 0, 2), 4),
        ('five diagonal pixels', _pix(6, 5, [(i, i) for i in range(5)]), [(0, 0), (1, 0), (5, 4), (5, 5), (4, 5), (0, 1)], 1,
         (4, 4, 0, 40, -4, 4), 10),
        ('anti-diagonal', _pix(3, 4, [(2, 0), (1, 1), (0, 2)]), [(0, 2), (2, 0), (3, 0), (3, 1), (1, 3), (0, 3)], 0,
         (2, -2, -6, 6, 4, 8), 6),
        ('an L', _pix(4, 3, [(0, 0), (0, 1), (0, 2), (1, 2), (2, 2)]), [(0, 0), (1, 0), (3, 2), (3, 3), (0, 3)], 0,
         (1, 0, 0, 3, 0, 3), 9),
        ('3 x 3 block', blk, [(2, 1), (5, 1), (5, 4), (2, 4)], 0, None, 9),
    ]


WIDE = dict(H=32767, W=65535, pixels=[(0, 0), (40000, 100), (65534, 32766)])


def counts_of_pixels(pixels, H, W):
    """canonical COCO counts of single pixels no two of which touch in the stream"""
    out, at = [], 0
    for s in sorted(x * H + y for x, y in pixels):
        out += [s - at, 1]
        at = s + 1
    return out + [H * W - at] if at < H * W else out


def plus_sign():
    m = np.zeros((9, 9), bool)
    m[3:6, :] = True
    m[:, 3:6] = True
    return m


def lattice_octagon():
    m = np.zeros((10, 10), bool)
    for y in range(10):
        for x in range(10):
            m[y, x] = 3 <= x + y <= 15 and -6 <= x - y <= 6
    return m


def extra_masks():
    rng = np.random.default_rng(149)
    out = [('H = 1', np.array([[0, 1, 1, 0, 1, 0]], bool)), ('W = 1', np.array([[0], [1], [0], [1]], bool)),
           ('1 x 1', np.ones((1, 1), bool)), ('full canvas', np.ones((7, 5), bool))]
    m = np.zeros((6, 9), bool)                           # runs across column ends with full columns in between
    m[4:, 1] = True
    m[:, 2:7] = True
    m[:2, 7] = True
    out.append(('a run across six column ends', m))
    m = np.zeros((5, 8), bool)
    m[3:, 0] = True
    m[:, 1:3] = True
    m[:1, 3] = True
    m[2:4, 3] = True                                     # a second piece in the column the long run ends in
    m[4, 5] = True
    m[:, 6] = True
    m[0, 7] = True
    out.append(('long runs and more pieces in their end columns', m))
    m = np.zeros((40, 60), bool)
    m[2:5, 1:4] = True
    m[30:38, 50:59] = True
    out.append(('two far components', m))
    for d in (0.02, 0.1, 0.5, 0.9):
        out.append((f'noise 64 x 64 at {d}', rng.random((64, 64)) < d))
    out.append(('square', _pix(8, 8, [(x, y) for x in range(2, 6) for y in range(1, 5)])))
    out.append(('plus sign', plus_sign()))
    out.append(('lattice octagon', lattice_octagon()))
    return out


def quarter_disc_with_spike(r=100):
    """a convex arc with one far outlier beside it: the columns' tops climb the upper left quarter of a disc in the lower half
    of the canvas, the next column is set over the full height.  Every point of the arc is a strict convex turn between its
    neighbours and none is a hull vertex: the pruning takes the arc apart from the spike's side, about one point a round"""
    m = np.zeros((2 * r + 1, r + 2), bool)
    for x in range(r + 1):
        top = 2 * r - int(round(math.sqrt(r * r - (x - r) ** 2)))
        m[top:, x] = True
    m[:, r + 1] = True
    return m


def column_profile(ncols, spread, two_pieces, seed):
    """ncols occupied columns, `spread` columns apart, on a canvas 48 rows high: the tops follow a noisy parabola, the bottoms
    another; two_pieces: only the first and the last pixel of a column are set (two runs a column), else all between them"""
    rng = np.random.default_rng(seed)
    H, W = 48, spread * ncols
    x = np.arange(ncols)
    u = (x - ncols / 2) / (ncols / 2)
    top = np.clip(np.round(16 * u * u + rng.integers(0, 3, ncols)), 0, 20).astype(int)
    bot = np.clip(np.round(46 - 14 * u * u - rng.integers(0, 3, ncols)), 26, 47).astype(int)
    m = np.zeros((H, W), bool)
    for i in range(ncols):
        if two_pieces:
            m[top[i], spread * i] = m[bot[i], spread * i] = True
        else:
            m[top[i]:bot[i] + 1, spread * i] = True
    return m


def boundary_masks():
    """occupied-column counts around every path boundary: one chunk of records (spread 2: a record and two points a column),
    one chunk of points, the LDS capacity of a chain"""
    out = []
    for ncols in (THREADS // 2 - 1, THREADS // 2, THREADS // 2 + 1, THREADS - 1, THREADS, THREADS + 1):
        out.append((f'{ncols} columns apart', column_profile(ncols, 2, ncols % 2 == 0, ncols)))
        out.append((f'{ncols} columns side by side', column_profile(ncols, 1, ncols % 2 == 1, ncols)))
    for ncols in (LDS_RECORDS - 1, LDS_RECORDS, LDS_RECORDS + 1):
        out.append((f'{ncols} columns apart', column_profile(ncols, 2, True, ncols)))
    out.append((f'{2 * LDS_RECORDS + 1} columns side by side', column_profile(2 * LDS_RECORDS + 1, 1, True, 7)))
    return out


def all_cases():
    return [(nm, m) for nm, m, *_ in known_answers()] + pcases.all_cases() + extra_masks()


_WANT = {}


def want_of(name, mask):
    """the reference's (hull, area2, edge, q) of a case mask, made and self-checked once and shared"""
    key = (name, mask.shape)
    if key not in _WANT:
        _WANT[key] = oref.check(mask)
    return _WANT[key]


def flatten(wants):
    """[(hull, area2, edge, q)] -> the five arrays"""
    verts = np.array([v for w in wants for v in w[0]], np.int32).reshape(-1, 2)
    offs = np.cumsum([0] + [len(w[0]) for w in wants]).astype(np.int64)
    return (verts, offs, np.array([w[1] for w in wants], np.int64).reshape(-1), np.array([w[2] for w in wants], np.int32).reshape(-1),
            np.array([w[3] for w in wants], np.int64).reshape(-1, 6))


def assert_arrays_equal(got, want, what=''):
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert g.dtype == w.dtype, f'{what}: {name} is {g.dtype}, expected {w.dtype}'
        assert tuple(g.shape) == tuple(w.shape), f'{what}: {name} has shape {tuple(g.shape)}, expected {tuple(w.shape)}'
        assert torch.equal(g.cpu(), w), f'{what}: {name} differs: {g.cpu().tolist()[:12]} != {w.tolist()[:12]}'


def obb_of_table(ops, counts, n, H, W):
    hull = ops.mask_hull(counts, n, H, W)
    return tuple(hull) + tuple(ops.hull_min_rect(hull[0], hull[1]))


def run(ops, dev, masks, H, W):
    counts, n = seam_cases.rows_from_masks(masks, dev)
    return obb_of_table(ops, counts, n, H, W)


# -------------------------------------------------------------------------------------------------------------- kernels
def check_known_answers(ops, dev):
    for name, m, hull, edge, q, area in known_answers():
        got = run(ops, dev, [m], *m.shape)
        assert [tuple(v) for v in got[0].cpu().tolist()] == hull, name
        assert got[1].cpu().tolist() == [0, len(hull)] and got[2].cpu().tolist() == [oref.area2_of(hull)], name
        assert got[3].cpu().tolist() == [edge], name
        gq = tuple(got[4].cpu().tolist()[0])
        assert q is None or gq == q, (name, gq)
        assert oref.rect_area(gq, gq[0] ** 2 + gq[1] ** 2) == area, name
        assert_arrays_equal(got, flatten([want_of(name, m)]), name)


def check_single_masks(ops, dev):
    """every case mask alone (k = 1) on its own canvas"""
    for name, m in all_cases():
        H, W = m.shape
        got = run(ops, dev, [m], H, W)
        assert_arrays_equal(got, flatten([want_of(name, m)]), name)
        assert all(g.device.type == torch.device(dev).type for g in got)


def check_ties(ops, dev):
    """equal rectangles: the lowest edge wins"""
    cases = dict(extra_masks())
    sq = run(ops, dev, [cases['square']], 8, 8)
    assert sq[3].cpu().tolist() == [0] and sq[0].shape[0] == 4 and tuple(sq[4].cpu().tolist()[0]) == (4, 0, 8, 24, 4, 20)
    for nm in ('plus sign', 'lattice octagon'):
        m = cases[nm]
        ring, _, edge, q = want_of(nm, m)
        areas = [oref.rect_area(*oref.edge_frame(ring, j)) for j in range(len(ring))]
        assert areas.count(min(areas)) >= 2 and edge == areas.index(min(areas)) and len(ring) == 8
        assert_arrays_equal(run(ops, dev, [m], *m.shape), flatten([want_of(nm, m)]), nm)


def check_path_boundaries(ops, dev):
    """the column counts around a chunk of records, a chunk of points and the LDS capacity, in one batch per canvas; the
    pruning rounds are reported"""
    rounds = {}
    for name, m in boundary_masks():
        H, W = m.shape
        counts, n = seam_cases.rows_from_masks([m], dev)
        hull = ops.mask_hull(counts, n, H, W, with_rounds=True)
        got = tuple(hull[:3]) + tuple(ops.hull_min_rect(hull[0], hull[1]))
        assert_arrays_equal(got, flatten([want_of(name, m)]), name)
        rounds[name] = (hull[3].cpu().view(-1).tolist(), int(hull[0].shape[0]))
    return rounds


def check_slow_pruning(ops, dev, r=100):
    m = quarter_disc_with_spike(r)
    H, W = m.shape
    counts, n = seam_cases.rows_from_masks([m], dev)
    hull = ops.mask_hull(counts, n, H, W, with_rounds=True)
    got = tuple(hull[:3]) + tuple(ops.hull_min_rect(hull[0], hull[1]))
    assert_arrays_equal(got, flatten([want_of(f'quarter disc {r}', m)]), 'quarter disc with a spike')
    return hull[3].cpu().view(-1).tolist()


def check_wide_coordinates(ops, dev):
    """H = 32 767, W = 65 535: the rectangle comparison multiplies beyond 64 bits"""
    H, W, pixels = WIDE['H'], WIDE['W'], WIDE['pixels']
    ring, a2, edge, q = oref.check(pixels)
    assert len(ring) == 7 and edge == 5 and q == (-65534, -32766, -5368414212, 0, -65534, 1304119366)
    from fractions import Fraction
    assert oref.rect_area(q, q[0] ** 2 + q[1] ** 2) == Fraction(875175594029474850, 671039489)
    assert oref.uvl_bits(ring) > 64 and oref.uvl_bits(ring) == 95
    counts, n = seam_cases.rows_from_counts([counts_of_pixels(pixels, H, W), None], dev)
    got = obb_of_table(ops, counts, n, H, W)
    assert_arrays_equal(got, flatten([(ring, a2, edge, q), ([], 0, -1, (0,) * 6)]), 'wide coordinates')


def batch_case():
    """every case mask placed on one 66 x 70 canvas (tests/_mask_polygons_cases.py batch_case's canvas)"""
    H, W = 66, 70
    rng = np.random.default_rng(19)
    masks, want = [], []
    for name, m in all_cases():
        ox, oy = int(rng.integers(0, W - m.shape[1] + 1)), int(rng.integers(0, H - m.shape[0] + 1))
        masks.append(pcases.embed(m, H, W, ox, oy))
        ring, a2, edge, q = want_of(name, m)
        moved = [(x + ox, y + oy) for x, y in ring]
        if ring:                                            # a moved hull keeps its edge; its frame moves with the offset
            ex, ey = q[0], q[1]
            da, db = ox * ex + oy * ey, oy * ex - ox * ey
            q = (ex, ey, q[2] + da, q[3] + da, q[4] + db, q[5] + db)
        want.append((moved, a2, edge, q))
    return H, W, masks, want


def check_batch(ops, dev):
    H, W, masks, want = batch_case()
    for i in (0, 7, len(masks) - 1):                        # the moved expectations are the reference's own
        assert oref.obb(masks[i]) == want[i]
    rows = [lref.rle_counts_np(m) for m in masks]
    cap = max(len(r) for r in rows)
    widest = max(range(len(rows)), key=lambda i: len(rows[i]))
    counts, n = seam_cases.rows_from_counts(rows, 'cpu', cap)
    empty = ([], 0, -1, (0,) * 6)
    order = list(range(len(rows)))
    order.insert(3, 'zero')
    order.insert(11, 'negative')
    order.insert(len(rows) // 2, 'beyond')
    out_c = torch.zeros((len(order), cap), dtype=torch.int32)
    out_n = torch.zeros((len(order),), dtype=torch.int32)
    want_all = []
    for j, o in enumerate(order):
        if o == 'zero':
            out_c[j] = counts[0]
            want_all.append(empty)
        elif o == 'negative':
            out_c[j], out_n[j] = counts[1], -(cap + 5)
            want_all.append(empty)
        elif o == 'beyond':
            out_c[j], out_n[j] = counts[widest], cap + 7
            want_all.append(want[widest])
        else:
            out_c[j], out_n[j] = counts[o], n[o]
            want_all.append(want[o])
    got = obb_of_table(ops, out_c.to(dev), out_n.to(dev), H, W)
    assert_arrays_equal(got, flatten(want_all), 'batch')
    again = obb_of_table(ops, out_c.to(dev), out_n.to(dev), H, W)              # a second launch is bit-identical
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    return got, want_all


def check_no_rows_and_no_pixels(ops, dev):
    z = obb_of_table(ops, torch.zeros((0, 4), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev), 5, 6)
    assert_arrays_equal(z, flatten([]), 'k = 0')
    got = run(ops, dev, [np.zeros((4, 3), bool), None, np.zeros((4, 3), bool)], 4, 3)
    assert_arrays_equal(got, flatten([([], 0, -1, (0,) * 6)] * 3), 'empty masks')


def primitive_polygon(r):
    """a strictly convex lattice polygon with one edge per primitive vector inside the disc of radius r, canonical"""
    vecs = [(a, b) for a in range(-r, r + 1) for b in range(-r, r + 1) if (a or b) and a * a + b * b <= r * r and math.gcd(a, b) == 1]
    vecs.sort(key=lambda v: math.atan2(v[1], v[0]))
    pts, x, y = [], 0, 0
    for a, b in vecs:
        pts.append((x, y))
        x, y = x + a, y + b
    x0, y0 = min(p[0] for p in pts), min(p[1] for p in pts)
    return oref.canonical([(px - x0, py - y0) for px, py in pts])


def hand_made_polygons():
    top = 65535
    return [[(0, 0), (4, 0), (0, 3)], [(0, 0), (top, 0), (top, top), (0, top)], [(0, 1), (1, 0), (top, top - 1), (top - 1, top)],
            [], [(3, 5), (9, 2), (12, 4), (13, 9), (7, 12), (4, 10)], primitive_polygon(6), [(2, 2), (3, 2), (3, 3), (2, 3)],
            primitive_polygon(14), primitive_polygon(24)]


def check_hull_min_rect(ops, dev):
    """the calipers alone on hand-made convex polygons: small, at the coordinate bound, empty, more edges than a block has
    threads, more vertices than are staged in LDS"""
    rings = hand_made_polygons()
    assert len(rings[5]) < THREADS < len(rings[-2]) <= RECT_LDS < len(rings[-1])
    for ring in rings:
        m = len(ring)
        assert not ring or ring == oref.canonical(ring)
        assert all(oref._cross(ring[i], ring[(i + 1) % m], ring[(i + 2) % m]) > 0 for i in range(m))
    want = [oref.min_rect(ring) for ring in rings]
    assert oref.uvl_bits(rings[2]) > 64
    verts = torch.tensor([v for ring in rings for v in ring], dtype=torch.int32).reshape(-1, 2).to(dev)
    offs = torch.tensor(np.cumsum([0] + [len(ring) for ring in rings]), dtype=torch.int64).to(dev)
    edge, q = ops.hull_min_rect(verts, offs)
    assert edge.dtype == torch.int32 and q.dtype == torch.int64
    assert edge.cpu().tolist() == [w[0] for w in want], (edge.cpu().tolist(), [w[0] for w in want])
    assert [tuple(r) for r in q.cpu().tolist()] == [tuple(w[1]) for w in want], (q.cpu().tolist(), [w[1] for w in want])
    e2, q2 = ops.hull_min_rect(verts, offs)
    assert torch.equal(edge, e2) and torch.equal(q, q2)


def check_refuses_bad_arguments(ops, dev, pytest):
    counts, n = seam_cases.rows_from_counts([[4]], dev)
    with pytest.raises(ValueError, match='32-bit'):
        ops.mask_hull(counts, n, 65536, 32768)
    with pytest.raises(ValueError, match='65535'):
        ops.mask_hull(counts, n, 2, 65536)
    with pytest.raises(ValueError, match='65535'):
        ops.mask_hull(counts, n, 65536, 2)
    with pytest.raises(ValueError, match='int32'):
        ops.mask_hull(counts.to(torch.int64), n, 2, 2)
    with pytest.raises(ValueError, match='empty'):
        ops.mask_hull(counts, n, 0, 4)
    v, o = torch.zeros((4, 2), dtype=torch.int32, device=dev), torch.tensor([0, 4], dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match='hull_verts'):
        ops.hull_min_rect(v.to(torch.int64), o)
    with pytest.raises(ValueError, match='hull_offs'):
        ops.hull_min_rect(v, o.to(torch.int32))
    with pytest.raises(ValueError, match=r'\[Vh, 2\]'):
        ops.hull_min_rect(torch.zeros((4, 3), dtype=torch.int32, device=dev), o)
    assert ops.MASK_OBB_MAX_SIDE == 65535
    lib = ops._lib.load()
    p = torch.zeros((64,), dtype=torch.int64, device=dev).data_ptr()
    assert lib.rsp_mask_hull_chains(p, p, 1, 4, 65536, 32768, p, 1, p, p, p, 0) != 0
    assert lib.rsp_mask_hull_chains(p, p, 1, 4, 2, 65536, p, 1, p, p, p, 0) != 0
    assert lib.rsp_mask_hull_chains(p, p, 1, 4, 65536, 2, p, 1, p, p, p, 0) != 0
    assert lib.rsp_mask_hull_chains(0, p, 1, 4, 4, 4, p, 1, p, p, p, 0) != 0
    assert lib.rsp_mask_hull_chains(p, p, 1, 4, 4, 4, p, 2 ** 30, p, p, p, 0) != 0
    assert lib.rsp_mask_hull_write(p, 1, 4, p, 1, p, p, p, 2 ** 31, p, p, 0) != 0
    assert lib.rsp_mask_hull_write(p, 1, 4, p, 1, p, p, 0, 4, p, p, 0) != 0
    assert lib.rsp_hull_min_rect(p, p, 1, 2 ** 31, p, p, 0) != 0 and lib.rsp_hull_min_rect(p, 0, 1, 4, p, p, 0) != 0
    assert lib.rsp_mask_hull_workspace_bytes(-1) == 0 and lib.rsp_mask_hull_workspace_bytes(2 ** 30) == 0
    assert lib.rsp_mask_hull_workspace_bytes(3) == 3 * 32


# ------------------------------------------------------------------------------------------------------------------ API
def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(np.all(np.isnan(got) == np.isnan(want))) and \
        bool(np.all(np.abs(got - want)[~np.isnan(want)] <= RTOL * np.abs(want)[~np.isnan(want)]))


def want_floats(wants):
    """(corners [k, 4, 2], xywha [k, 5]) of reference results as float64, NaN rows for empty ones"""
    c = np.full((len(wants), 4, 2), np.nan)
    x = np.full((len(wants), 5), np.nan)
    for i, (ring, _, edge, q) in enumerate(wants):
        if edge >= 0:
            c[i] = [[float(v) for v in p] for p in oref.corners(q)]
            x[i] = oref.xywha(q)
    return c, x


def api_masks():
    cases = dict(all_cases())
    names = ('five diagonal pixels', 'anti-diagonal', 'comb', 'nested frames', 'two diagonal pixels', 'noise 64 x 64 at 0.1',
             'lattice octagon')
    H, W = 66, 67
    masks = [pcases.embed(cases[nm], H, W, 1, 2) for nm in names] + [np.zeros((H, W), bool)]
    tall = np.zeros((H, W), bool)
    tall[5:40, 7:10] = True                              # V > U on edge 0: w runs along nrm, the angle is -pi / 2
    return H, W, masks + [tall]


def check_api_forms(apis, rle, dev):
    """the three input forms and the four output forms of masks_to_obb against the Fraction reference"""
    H, W, masks = api_masks()
    wants = [oref.check(m) for m in masks]
    wc, wx = want_floats(wants)
    assert wx[-1][2] > wx[-1][3] and wx[-1][4] == -math.pi / 2 and np.isnan(wc[-2]).all()
    assert all(-math.pi / 2 <= a < math.pi / 2 for a in wx[:, 4] if not math.isnan(a)) and len({round(a, 6) for a in wx[:-2, 4]}) >= 3
    dense = torch.from_numpy(np.stack(masks)).to(dev)
    lists = [dict(size=[H, W], counts=lref.rle_counts_np(m)) for m in masks]
    strings = [dict(size=[H, W], counts=rle.counts_to_string(lref.rle_counts_np(m))) for m in masks]
    inputs = [(dense, {}), (lists, dict(device=dev)), (strings, dict(device=dev)),
              ([dict(d, counts=d['counts'].decode()) for d in strings], dict(device=dev))]
    for src, kw in inputs:
        c = apis.masks_to_obb(src, **kw)
        assert isinstance(c, np.ndarray) and c.dtype == np.float64 and close(c, wc)
        x = apis.masks_to_obb(src, form='xywha', **kw)
        assert isinstance(x, np.ndarray) and x.dtype == np.float64 and close(x, wx)
        hulls = apis.masks_to_obb(src, form='hull', **kw)
        assert len(hulls) == len(wants)
        for h, w in zip(hulls, wants):
            assert h.dtype == np.int32 and h.shape == (len(w[0]), 2) and [tuple(v) for v in h.tolist()] == w[0]
    geo = apis.masks_to_obb(dense, form='geojson')
    assert [g['type'] for g in geo] == ['Polygon'] * len(masks) and geo[-2]['coordinates'] == []
    for g, c in zip(geo, wc):
        if not np.isnan(c).any():
            ring = g['coordinates'][0]
            assert len(ring) == 5 and ring[0] == ring[-1] and close(ring[:4], c)
    t = (500000.0, 0.5, 0.0, 4000000.0, 0.0, -0.5)
    tc = apis.masks_to_obb(dense, transform=t)
    assert close(tc, np.stack([500000.0 + 0.5 * wc[..., 0], 4000000.0 - 0.5 * wc[..., 1]], -1))
    tg = apis.masks_to_obb(dense[:1], form='geojson', transform=t)
    assert close(tg[0]['coordinates'][0][:4], tc[0])
    assert apis.masks_to_obb(torch.zeros((0, 4, 4), dtype=torch.bool, device=dev)).shape == (0, 4, 2)
    assert apis.masks_to_obb(torch.zeros((0, 4, 4), dtype=torch.bool, device=dev), form='xywha').shape == (0, 5)
    # rle.obb_to_numpy is the one transfer behind both float forms
    counts, n = seam_cases.rows_from_masks(masks, dev)
    out = rle.runs_to_obb(counts, n, (H, W))
    assert len(out) == 5 and close(rle.obb_to_numpy(out[3], out[4]), wc) and close(rle.obb_to_numpy(out[3], out[4], 'xywha'), wx)
    assert all(torch.equal(a, b) for a, b in zip(rle.runs_to_hulls(counts, n, (H, W)), out[:3]))


def check_api_refusals(apis, rle, dev, pytest):
    m = torch.zeros((1, 2, 2), dtype=torch.bool, device=dev)
    with pytest.raises(ValueError, match='xywha'):
        apis.masks_to_obb(m, form='xywha', transform=(0, 1, 0, 0, 0, 1))
    with pytest.raises(ValueError, match='form'):
        apis.masks_to_obb(m, form='le90')
    with pytest.raises(ValueError, match='canonical'):
        apis.masks_to_obb([dict(size=[2, 2], counts=[2, 1, 0, 1])], device=dev)
    with pytest.raises(ValueError, match='form'):
        rle.obb_to_numpy(torch.zeros((0,), dtype=torch.int32), torch.zeros((0, 6), dtype=torch.int64), 'hull')


# ------------------------------------------------------------------------------------------------------------- pipeline
def check_pipeline(li, scene, model, patch, dense_masks_of, **kw):
    """inference_large_image(oriented_boxes=True) against the reference applied to the dense result of the same call, for
    masks='rle' and 'polygons'; the defaults leave no obb field; masks='dense' is refused before the model runs"""
    base = dict(patch_size=patch, batch_size=3, **kw)
    dense = dense_masks_of(li.inference_large_image(model, scene, masks='dense', **base))
    wc, _ = want_floats([oref.obb(m) for m in dense])
    plain = li.inference_large_image(model, scene, masks='rle', **base)
    assert 'obb' not in plain.pred_instances and 'obb' not in li.pred2dict(plain)
    for form in ('rle', 'polygons'):
        out = li.inference_large_image(model, scene, masks=form, oriented_boxes=True, **base)
        p = out.pred_instances
        assert isinstance(p.obb, np.ndarray) and p.obb.dtype == np.float64 and p.obb.shape == (len(dense), 4, 2)
        assert close(p.obb, wc)
        js = li.pred2dict(out, 0.5)
        sel = (p.scores >= 0.5).nonzero().view(-1).tolist()
        assert close(np.asarray(js['obb'], np.float64).reshape(-1, 4, 2), wc[sel]) and len(js['obb']) == len(js['labels'])
        assert {k: v for k, v in js.items() if k != 'obb'} == li.pred2dict(
            li.inference_large_image(model, scene, masks=form, **base), 0.5)
    fc = li.pred2geojson(out, 0.5)
    assert all(close(f['properties']['obb'], wc[i]) for f, i in zip(fc['features'], sel))
    assert len(dense) > 0 and not np.isnan(wc).all()
    return len(dense)
