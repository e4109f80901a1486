"""Bodies of the polygon-export tests (csrc/mask_polygons.hip, rsprompter_amd/rle.py runs_to_polygons, apis.masks_to_polygons,
large_image masks='polygons'), shared by both tiers: tests/test_mask_polygons_cpu.py calls them with the
emulated `ops` on CPU tensors, tests/test_gpu_mask_polygons.py with the real ones on cuda:0.  The reference is
tests/_mask_polygons_ref.py, the sequential definition on dense masks; all six arrays are compared by exact equality.  The
run tables come from tests/_large_image_ref.py's numpy encoder, not from the kernels under test."""
import numpy as np
import torch

import _large_image_ref as lref
import _mask_polygons_ref as pref
import _seam_merge_cases as seam_cases

NAMES = ('verts', 'ring_offs', 'ring_inst', 'ring_parent', 'ring_area2', 'inst_ring_offs')


# ----------------------------------------------------------------------------------------------------------- the masks
def _frame(h, w, t=1):
    m = np.ones((h, w), bool)
    m[t:h - t, t:w - t] = False
    return m


def arm_spiral(n=33):
    """a one-pixel-wide arm that winds inwards on n x n: ONE long ring.  Segment lengths n-1, n-1, n-1, n-3, n-3, n-5, ..."""
    m = np.zeros((n, n), bool)
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = True
    lengths = [n - 1, n - 1, n - 1]
    v = n - 3
    while v > 0:
        lengths += [v, v]
        v -= 2
    for run in lengths:
        for _ in range(run):
            x, y = x + dx, y + dy
            m[y, x] = True
        dx, dy = -dy, dx
    return m


def named_masks():
    """(name, mask) for the shapes the issue lists; small canvases"""
    out = []
    out.append(('row H=1', np.array([[1, 0, 1, 1, 0, 1]], bool)))
    out.append(('column W=1', np.array([[1], [1], [0], [1]], bool)))
    out.append(('1 x 1 set', np.ones((1, 1), bool)))
    out.append(('1 x 1 clear', np.zeros((1, 1), bool)))
    for name, (y, x) in (('top left', (0, 0)), ('top right', (0, 4)), ('bottom left', (3, 0)), ('bottom right', (3, 4))):
        m = np.zeros((4, 5), bool)
        m[y, x] = True
        out.append((f'one pixel {name}', m))
    m = np.zeros((5, 4), bool)
    m[:, 2] = True
    out.append(('full column', m))
    m = np.zeros((5, 4), bool)
    m[4, 1] = m[0, 2] = True
    out.append(('run across a column end', m))
    m = np.zeros((5, 4), bool)
    m[2:, 0] = True
    m[:, 1] = True
    m[:3, 2] = True
    out.append(('run across two column ends', m))
    out.append(('full', np.ones((3, 4), bool)))
    out.append(('checkerboard', (np.add.outer(np.arange(6), np.arange(7)) % 2 == 0)))
    out.append(('checkerboard odd', (np.add.outer(np.arange(5), np.arange(5)) % 2 == 1)))
    m = np.zeros((9, 10), bool)
    m[1:8, 1:9] = _frame(7, 8)
    m[2, 2] = True                                   # an island that touches the frame's inner corner only diagonally
    m[4, 5] = True                                   # and a free one in the same hole
    out.append(('frame with a diagonal-touching island in its hole', m))
    m = np.zeros((13, 14), bool)
    m[0:13, 0:13] = _frame(13, 13)
    m[2:11, 2:11] |= _frame(9, 9)
    m[4:9, 4:9] |= _frame(5, 5)
    m[6, 6] = True
    out.append(('nested frames', m))
    out.append(('spiral 33 x 33', arm_spiral(33)))
    m = np.zeros((9, 15), bool)
    m[0, :] = True
    m[:, ::2] = True
    out.append(('comb', m))
    m = np.zeros((15, 9), bool)
    m[:, 0] = True
    m[::2, :] = True
    out.append(('comb sideways', m))
    m = np.zeros((6, 6), bool)                       # a hole whose ring passes a saddle twice
    m[0:5, 0:5] = _frame(5, 5)
    m[2, 2] = True
    m[1, 1] = False
    m[0, 0] = True
    out.append(('holes meeting at saddles', m))
    return out


def random_masks(count=28, seed=5):
    rng = np.random.default_rng(seed)
    out = [('random 1 x 1', rng.random((1, 1)) < 0.6)]
    for i in range(count):
        H, W = int(rng.integers(1, 15)), int(rng.integers(1, 15))
        d = (0.0, 0.2, 0.6, 1.0)[i % 4]
        out.append((f'random {H} x {W} at {d}', rng.random((H, W)) < d))
    return out


def noise64():
    return np.random.default_rng(64).random((64, 64)) < 0.5


_WANT = {}


def want_of(name, mask):
    """the reference's rings of a case mask, traced and self-checked once and shared"""
    if name not in _WANT:
        _WANT[name] = pref.check_traced(mask)
    return _WANT[name]


def all_cases():
    return named_masks() + random_masks() + [('noise 64 x 64', noise64())]


# ------------------------------------------------------------------------------------------------------------- helpers
def assert_arrays_equal(got, want, what=''):
    assert len(got) == len(want) == 6
    for name, g, w in zip(NAMES, got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert g.dtype == w.dtype, f'{what}: {name} is {g.dtype}, expected {w.dtype}'
        assert tuple(g.shape) == tuple(w.shape), f'{what}: {name} has shape {tuple(g.shape)}, expected {tuple(w.shape)}'
        assert torch.equal(g.cpu(), w), f'{what}: {name} differs'


def run(ops, dev, masks, H, W):
    counts, n = seam_cases.rows_from_masks(masks, dev)
    return ops.mask_polygons(counts, n, H, W)


def embed(mask, H, W, ox, oy):
    out = np.zeros((H, W), bool)
    out[oy:oy + mask.shape[0], ox:ox + mask.shape[1]] = mask
    return out


# -------------------------------------------------------------------------------------------------------------- kernels
def check_single_masks(ops, dev):
    """every case mask alone (k = 1) on its own canvas"""
    for name, m in all_cases():
        H, W = m.shape
        got = run(ops, dev, [m], H, W)
        assert_arrays_equal(got, pref.flatten([want_of(name, m)]), name)
        assert all(g.device.type == torch.device(dev).type for g in got)


def check_known_answers(ops, dev):
    """a few answers written out by hand, independent of the reference tracer"""
    got = run(ops, dev, [np.ones((3, 4), bool)], 3, 4)
    assert got[0].cpu().tolist() == [[0, 0], [4, 0], [4, 3], [0, 3]] and got[4].cpu().tolist() == [24]
    assert got[1].cpu().tolist() == [0, 4] and got[3].cpu().tolist() == [-1] and got[5].cpu().tolist() == [0, 1]
    got = run(ops, dev, [_frame(3, 3)], 3, 3)
    assert got[0].cpu().tolist() == [[0, 0], [3, 0], [3, 3], [0, 3], [1, 1], [1, 2], [2, 2], [2, 1]]
    assert got[4].cpu().tolist() == [18, -2] and got[3].cpu().tolist() == [-1, 0]
    d = np.array([[1, 0], [0, 1]], bool)                  # two pixels touching diagonally: ONE ring through the saddle twice
    got = run(ops, dev, [d], 2, 2)
    assert got[0].cpu().tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]] and got[4].cpu().tolist() == [4]
    got = run(ops, dev, [~d], 2, 2)
    assert got[0].cpu().tolist() == [[0, 1], [1, 1], [1, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]] and got[4].cpu().tolist() == [4]


def batch_case():
    """every case mask, the 64 x 64 noise included, placed on one 66 x 70 canvas; check_batch puts rows of n = 0, n < 0 and
    n beyond cap in between"""
    H, W = 66, 70
    rng = np.random.default_rng(9)
    masks, want = [], []
    for name, m in all_cases():
        ox, oy = int(rng.integers(0, W - m.shape[1] + 1)), int(rng.integers(0, H - m.shape[0] + 1))
        masks.append(embed(m, H, W, ox, oy))
        want.append([(ring + np.array([ox, oy], np.int32), par, a2) for ring, par, a2 in want_of(name, m)])
    return H, W, masks, want


def check_batch(ops, dev):
    H, W, masks, want = batch_case()
    rows = [lref.rle_counts_np(m) for m in masks]
    cap = max(len(r) for r in rows)
    widest = max(range(len(rows)), key=lambda i: len(rows[i]))
    counts, n = seam_cases.rows_from_counts(rows, 'cpu', cap)
    # in between: an empty row (n = 0), a row reported as not fitting (n < 0), and the widest row with n beyond cap, which
    # is read up to cap
    k0 = len(rows)
    at = [3, 11, k0 // 2]
    order = list(range(k0))
    order.insert(at[0], 'zero')
    order.insert(at[1], 'negative')
    order.insert(at[2], 'beyond')
    out_c = torch.zeros((len(order), cap), dtype=torch.int32)
    out_n = torch.zeros((len(order),), dtype=torch.int32)
    want_all = []
    for j, o in enumerate(order):
        if o == 'zero':
            out_c[j] = counts[0]
            want_all.append([])
        elif o == 'negative':
            out_c[j], out_n[j] = counts[1], -(cap + 5)
            want_all.append([])
        elif o == 'beyond':
            out_c[j], out_n[j] = counts[widest], cap + 7
            want_all.append(want[widest])
        else:
            out_c[j], out_n[j] = counts[o], n[o]
            want_all.append(want[o])
    got = ops.mask_polygons(out_c.to(dev), out_n.to(dev), H, W)
    assert_arrays_equal(got, pref.flatten(want_all), 'batch')
    again = ops.mask_polygons(out_c.to(dev), out_n.to(dev), H, W)              # a second launch is bit-identical
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    return got, want_all


def check_no_rows_and_no_rings(ops, dev):
    z = ops.mask_polygons(torch.zeros((0, 4), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev), 5, 6)
    assert_arrays_equal(z, pref.flatten([]), 'k = 0')
    got = run(ops, dev, [np.zeros((4, 3), bool), None, np.zeros((4, 3), bool)], 4, 3)
    assert_arrays_equal(got, pref.flatten([[], [], []]), 'empty masks')


def check_refuses_bad_arguments(ops, dev, pytest):
    counts, n = seam_cases.rows_from_counts([[4]], dev)
    with pytest.raises(ValueError, match='32-bit'):
        ops.mask_polygons(counts, n, 65536, 32768)
    with pytest.raises(ValueError, match='int32'):
        ops.mask_polygons(counts.to(torch.int64), n, 2, 2)
    with pytest.raises(ValueError, match='empty'):
        ops.mask_polygons(counts, n, 0, 4)
    lib = ops._lib.load()
    p = torch.zeros((64,), dtype=torch.int64, device=dev).data_ptr()
    assert lib.rsp_run_pieces_count(p, p, 1, 4, 65536, 32768, p, 0) != 0
    assert lib.rsp_mask_polygon_edges(1, 65536, 32768, p, 1, p, p, p, p, 0) != 0
    assert lib.rsp_run_pieces_count(0, p, 1, 4, 4, 4, p, 0) != 0
    assert lib.rsp_mask_polygon_edges(1, 4, 4, p, 2 ** 31 // 6 + 1, p, p, p, p, 0) != 0
    assert lib.rsp_mask_polygon_rank(1, 4, 63, p, p, p, p, p, p, p, p, p, 0) != 0
    assert lib.rsp_mask_polygon_rank_workspace_bytes(-1) == 0 and lib.rsp_mask_polygon_rank_workspace_bytes(2) == 6 * 2 * 28


# ---------------------------------------------------------------------------------------------------------- piece table
def pieces_of_counts(rows, ns, cap, H):
    """the column-piece table as a statement on the counts alone: every ones-run [s, e) of the first min(n, cap) counts of a
    row, cut at the multiples of H -> ([(x, y0, y1, instance)] in stream order, piece_offs)"""
    out, offs = [], [0]
    for m, (row, n) in enumerate(zip(rows, ns)):
        s = 0
        for i in range(max(min(n, cap), 0)):
            e = s + row[i]
            if i & 1 and e > s:
                out += [(x, max(s, x * H) - x * H, min(e, (x + 1) * H) - x * H, m) for x in range(s // H, (e - 1) // H + 1)]
            s = e
        offs.append(len(out))
    return out, offs


def piece_tables():
    """[(H, W, rows, ns)]: per H in 1, 3, 7 a ones-run over four columns, rows with n = 0, n < 0 and n beyond the capacity,
    a non-canonical row (zero counts between ones-runs, a ones-run of no pixel) and noise; the 24 x 24 checkerboard, whose 553
    runs cross two chunks of the walk"""
    rng = np.random.default_rng(41)
    out = []
    for H in (1, 3, 7):
        W = 40
        noise = [lref.rle_counts_np(rng.random((H, W)) < d) for d in (0.5, 0.3)]
        rows = [[2, 3 * H + 1, H * W - 3 * H - 3], noise[1], noise[1], noise[0], [1, 2, 0, 3, 0, 0, 4, 1, 1, 0, 2, 2], noise[0], [H * W]]
        cap = max(len(r) for r in rows)
        ns = [len(r) for r in rows]
        ns[1], ns[2], ns[3] = 0, -(cap + 5), cap + 7
        rows[3] = (rows[3] + [1] * cap)[:cap]                  # every slot of the row that is read up to cap holds a count
        out.append((H, W, rows, ns))
    board = (np.add.outer(np.arange(24), np.arange(24)) & 1).astype(bool)
    row = lref.rle_counts_np(board)
    assert len(row) > 2 * 256
    out.append((24, 24, [[5, 7, 564], row], [3, len(row)]))
    return out


def _table_on(rows, ns, dev):
    counts, _ = seam_cases.rows_from_counts(rows, dev)
    return counts, torch.tensor(ns, dtype=torch.int32).to(dev)


def check_run_pieces(ops, dev):
    """ops.run_pieces and the two C entries behind it against pieces_of_counts, everything by ==; the tables its two consumers
    work on are the same bits; the documented host reads of the callers that share the run-domain intermediates"""
    from _run_morphology_cases import ReadCounter
    i32 = dict(dtype=torch.int32, device=dev)
    lib = ops._lib.load()
    for H, W, rows, ns in piece_tables():
        counts, n = _table_on(rows, ns, dev)
        cap = int(counts.shape[1])
        want, want_offs = pieces_of_counts(rows, ns, cap, H)
        assert max(x for x, _, _, _ in want) - min(x for x, _, _, _ in want[:4]) >= 3 or H == 24
        got = ops.run_pieces(counts, n, H, W)
        assert (got.P, got.widest) == (len(want), max(b - a for a, b in zip(want_offs, want_offs[1:])))
        assert got.pieces.dtype == torch.int32 and got.piece_offs.dtype == torch.int64 and got.pieces.is_contiguous()
        assert got.piece_offs.cpu().tolist() == want_offs
        assert [tuple(p) for p in got.pieces.cpu().t().tolist()] == want, (H, W)
        # the tables of the two consumers: the one mask_polygons works on (what its call of run_pieces returned) and the one
        # rle_components returns
        seen, inner = [], ops.run_pieces
        ops.run_pieces = lambda *a, **kw: seen.append(inner(*a, **kw)) or seen[-1]
        try:
            ops.mask_polygons(counts, n, H, W)
            comps = ops.rle_components(counts, n, H, W)
        finally:
            ops.run_pieces = inner
        assert len(seen) == 2 and seen[1].pieces is comps.pieces and seen[1].piece_offs is comps.piece_offs
        for t in seen:
            assert torch.equal(t.pieces, got.pieces) and torch.equal(t.piece_offs, got.piece_offs) and t.P == got.P
        # a piece_offs that overstates rows: the slots behind a row's pieces keep instance -1 and nothing else is written
        k, pad, mark = len(rows), 5, 0x5a5a5a5a
        cnt = torch.zeros((k,), **i32)
        assert lib.rsp_run_pieces_count(counts.data_ptr(), n.data_ptr(), k, cap, H, W, cnt.data_ptr(), ops._stream()) == 0
        assert cnt.cpu().tolist() == [b - a for a, b in zip(want_offs, want_offs[1:])]
        extra = [(3 * m + 1) % 4 for m in range(k)]
        offs = [0]
        for c, x in zip(cnt.cpu().tolist(), extra):
            offs.append(offs[-1] + c + x)
        P = offs[-1]
        buf = torch.full((4 * P + 2 * pad,), mark, **i32)
        offs_t = torch.tensor(offs, dtype=torch.int64).to(dev)
        assert lib.rsp_run_pieces(counts.data_ptr(), n.data_ptr(), k, cap, H, W, offs_t.data_ptr(), P, buf[pad:].data_ptr(),
                                  ops._stream()) == 0
        host = buf.cpu().tolist()
        expect = [mark] * pad + [mark] * (3 * P) + [-1] * P + [mark] * pad
        for m in range(k):
            for j, p in enumerate(want[want_offs[m]:want_offs[m + 1]]):
                for plane in range(4):
                    expect[pad + plane * P + offs[m] + j] = p[plane]
        assert host == expect, (H, W)
    # no rows; rows without a piece
    z = ops.run_pieces(torch.zeros((0, 4), **i32), torch.zeros((0,), **i32), 5, 6)
    assert (z.P, z.widest, tuple(z.pieces.shape), z.piece_offs.cpu().tolist()) == (0, 0, (4, 0), [0])
    counts, n = _table_on([[12], [3, 4, 5]], [1, -3], dev)
    z = ops.run_pieces(counts, n, 3, 4)
    assert (z.P, z.widest, tuple(z.pieces.shape), z.piece_offs.cpu().tolist()) == (0, 0, (4, 0), [0, 0, 0])
    C = ops.CONST
    assert C['RSP_RUN_COMPONENTS_MAX_PIECES'] == C['RSP_RUN_PIECES_MAX_PIECES'] == ops.RUN_PIECES_MAX_PIECES == 0x7fffff00
    assert C['RSP_MASK_POLYGON_MAX_PIECES'] == (2 ** 31 - 1) // 6 < C['RSP_RUN_PIECES_MAX_PIECES'] and C['RSP_ABI_VERSION'] == 6
    # host reads
    H, W, rows, ns = piece_tables()[2]
    counts, n = _table_on([rows[0], rows[3], rows[5]], [ns[0], len(rows[5]), ns[5]], dev)
    reads = {}
    for name, call in (('run_pieces', lambda: ops.run_pieces(counts, n, H, W)),
                       ('mask_polygons', lambda: ops.mask_polygons(counts, n, H, W)),
                       ('rle_components', lambda: ops.rle_components(counts, n, H, W)),
                       ('mask_hull', lambda: ops.mask_hull(counts, n, H, W)),
                       ('rle_union', lambda: ops.rle_union(counts, n, H, W, torch.tensor([0, 2, 3], **i32), torch.arange(3, **i32), 64))):
        with ReadCounter(dev) as rc:
            call()
        reads[name] = rc.n
    assert reads == dict(run_pieces=1, mask_polygons=3, rle_components=2, mask_hull=2, rle_union=1), reads


# ------------------------------------------------------------------------------------------------------------------ API
def _coco_counts(entry, H, W):
    from rsprompter_amd import datasets
    merged = datasets.rle_merge([datasets.rle_from_poly(p, H, W) for p in entry['polygons']])
    return merged if merged else [H * W]


def _fill_holes(mask):
    from scipy import ndimage
    lab, _ = ndimage.label(~np.pad(mask, 1))
    return (lab != lab[0, 0])[1:-1, 1:-1]


def check_api_forms(apis, rle, dev):
    """the three input forms give equal rings; coco reproduces hole-free masks through rleFrPoly + rleMerge; geojson"""
    names = ('comb', 'nested frames', 'checkerboard', 'full column', 'frame with a diagonal-touching island in its hole')
    cases = dict(all_cases())
    H, W = 16, 17
    masks = [embed(cases[nm], H, W, 1, 1) for nm in names] + [np.zeros((H, W), bool)]
    want = [pref.trace(m) for m in masks]
    dense = torch.from_numpy(np.stack(masks)).to(dev)
    by_tensor = apis.masks_to_polygons(dense)
    lists = [dict(size=[H, W], counts=lref.rle_counts_np(m)) for m in masks]
    by_list = apis.masks_to_polygons(lists, device=dev)
    strings = [dict(size=[H, W], counts=rle.counts_to_string(lref.rle_counts_np(m))) for m in masks]
    by_bytes = apis.masks_to_polygons(strings, device=dev)
    by_str = apis.masks_to_polygons([dict(d, counts=d['counts'].decode()) for d in strings], device=dev)
    for got in (by_tensor, by_list, by_bytes, by_str):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert len(g) == len(w)
            for (gr, gp, ga), (wr, wp, wa) in zip(g, w):
                assert gr.dtype == np.int32 and np.array_equal(gr, wr) and (gp, ga) == (wp, wa)
    # coco: outer rings only
    coco = apis.masks_to_polygons(dense, form='coco')
    for m, entry in zip(masks, coco):
        holes = any(a2 < 0 for _, _, a2 in pref.trace(m))
        assert entry['holes_dropped'] == holes
        assert all(isinstance(v, float) for p in entry['polygons'] for v in p)
        assert _coco_counts(entry, H, W) == lref.rle_counts_np(_fill_holes(m) if holes else m)
    assert [c['holes_dropped'] for c in coco] == [False, True, True, False, True, False]     # a checkerboard encloses its zeros
    rng = np.random.default_rng(3)
    free = [m for m in (rng.random((9, 11)) < 0.35 for _ in range(40)) if all(a2 > 0 for _, _, a2 in pref.trace(m))][:8]
    assert len(free) == 8
    for m, entry in zip(free, apis.masks_to_polygons(torch.from_numpy(np.stack(free)).to(dev), form='coco')):
        assert not entry['holes_dropped'] and _coco_counts(entry, 9, 11) == lref.rle_counts_np(m)
    # geojson
    geo = apis.masks_to_polygons(dense, form='geojson')
    assert [g['type'] for g in geo] == ['Polygon', 'MultiPolygon', 'Polygon', 'Polygon', 'MultiPolygon', 'MultiPolygon']
    assert geo[5]['coordinates'] == [] and len(geo[2]['coordinates']) == 11 and len(geo[4]['coordinates']) == 2
    assert [len(poly) for poly in geo[4]['coordinates']] == [2, 1]        # the frame with its hole, the free island
    nested = geo[1]['coordinates']                       # three frames, each with its hole, and the pixel in the middle
    assert [len(poly) for poly in nested] == [2, 2, 2, 1] and all(r[0] == r[-1] and len(r) == 5 for poly in nested for r in poly)
    assert nested[0][0][:-1] == [[float(x), float(y)] for x, y in want[1][0][0].tolist()]
    for g, w in zip(geo, want):                          # every hole sits in the polygon of its parent
        polys = [g['coordinates']] if g['type'] == 'Polygon' else g['coordinates']
        outer = [r for r, (_, par, a2) in enumerate(w) if a2 > 0]
        assert len(polys) == len(outer)
        for poly, o in zip(polys, outer):
            rings = [w[o][0]] + [ring for ring, par, a2 in w if par == o]
            assert [r[:-1] for r in poly] == [[[float(x), float(y)] for x, y in ring.tolist()] for ring in rings]
    t = apis.masks_to_polygons(dense[3:4], form='geojson', transform=(500000.0, 0.5, 0.0, 4000000.0, 0.0, -0.5))
    col = cases['full column']
    x0 = 1 + int(np.flatnonzero(col.any(0))[0])
    assert t[0] == dict(type='Polygon', coordinates=[[[500000.0 + 0.5 * x0, 4000000.0 - 0.5], [500000.0 + 0.5 * (x0 + 1), 4000000.0 - 0.5],
                                                     [500000.0 + 0.5 * (x0 + 1), 4000000.0 - 0.5 * 6], [500000.0 + 0.5 * x0, 4000000.0 - 0.5 * 6],
                                                     [500000.0 + 0.5 * x0, 4000000.0 - 0.5]]])


def check_api_refusals(apis, dev, pytest):
    for counts in ([2, 1, 0, 1], [0, 0, 4], [2, 1], [2, 1, 2], [2 ** 32 + 2, 2], [2 ** 31, 4 - 2 ** 31], [-1, 5]):
        # touching runs, two zeros, short, long, counts that would wrap in 32 bits, a negative count
        with pytest.raises(ValueError, match='canonical'):
            apis.masks_to_polygons([dict(size=[2, 2], counts=[4]), dict(size=[2, 2], counts=counts)], device=dev)
    assert len(apis.masks_to_polygons([dict(size=[2, 2], counts=[0, 4]), dict(size=[2, 2], counts=[4])], device=dev)[0]) == 1
    with pytest.raises(ValueError, match='canonical'):                            # "2 1 0 1" as a compressed string
        from rsprompter_amd import rle
        apis.masks_to_polygons([dict(size=[2, 2], counts=rle.counts_to_string([2, 1, 0, 1]))], device=dev)
    with pytest.raises(ValueError, match='form'):
        apis.masks_to_polygons(torch.zeros((1, 2, 2), dtype=torch.bool, device=dev), form='wkt')
    with pytest.raises(ValueError, match='transform'):
        apis.masks_to_polygons(torch.zeros((1, 2, 2), dtype=torch.bool, device=dev), transform=(0, 1, 0, 0, 0, 1))
    with pytest.raises(ValueError, match='one size'):
        apis.masks_to_polygons([dict(size=[2, 2], counts=[4]), dict(size=[2, 3], counts=[6])], device=dev)
    with pytest.raises(ValueError, match='empty list'):
        apis.masks_to_polygons([], device=dev)
    assert apis.masks_to_polygons(torch.zeros((0, 4, 4), dtype=torch.bool, device=dev)) == []


# ------------------------------------------------------------------------------------------------------------- pipeline
def refill_rings(rings, H, W):
    v, o, _, _, _, _ = pref.flatten([rings])
    return pref.refill(v, o, H, W).astype(bool)


def check_pipeline(li, dev, scene, model, patch, dense_masks_of, **kw):
    """inference_large_image(masks='polygons') against the reference applied to the dense result of the same call"""
    H, W = scene.shape[:2]
    out = li.inference_large_image(model, scene, patch_size=patch, batch_size=3, masks='polygons', **kw)
    dense = dense_masks_of(li.inference_large_image(model, scene, patch_size=patch, batch_size=3, masks='dense', **kw))
    p = out.pred_instances
    assert len(p.masks) == len(dense) == len(p.scores) > 0
    for rings, m in zip(p.masks, dense):
        want = pref.trace(m)
        assert len(rings) == len(want)
        for (gr, gp, ga), (wr, wp, wa) in zip(rings, want):
            assert np.array_equal(gr, wr) and (gp, ga) == (wp, wa)
    # pred2dict of the dense result and of the 'rle' result of the same call are one document, as before this feature
    dense_sample = li.inference_large_image(model, scene, patch_size=patch, batch_size=3, masks='dense', **kw)
    rle_sample = li.inference_large_image(model, scene, patch_size=patch, batch_size=3, masks='rle', **kw)
    assert isinstance(dense_sample.pred_instances.masks, torch.Tensor)
    for thr in (0.0, 0.5):
        jd, jr = li.pred2dict(dense_sample, thr), li.pred2dict(rle_sample, thr)
        assert jd == jr and all(isinstance(m['counts'], str) for m in jd['masks']) and len(jd['masks']) == len(jd['labels'])
    assert len(li.pred2dict(dense_sample, 0.0)['masks']) == len(dense) > 0
    js = li.pred2dict(out, 0.5)
    assert len(js['masks']) == int((p.scores >= 0.5).sum()) and set(js) == {'labels', 'scores', 'bboxes', 'masks'}
    assert all(set(r) == {'ring', 'parent', 'area2'} for inst in js['masks'] for r in inst)
    fc = li.pred2geojson(out, 0.5, (10.0, 2.0, 0.0, 20.0, 0.0, -2.0))
    assert fc['type'] == 'FeatureCollection' and len(fc['features']) == len(js['masks'])
    assert all(f['type'] == 'Feature' and set(f['properties']) == {'label', 'score', 'bbox'} and
               f['geometry']['type'] in ('Polygon', 'MultiPolygon') for f in fc['features'])
    return len(dense), sum(len(r) for r in p.masks)
