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
    assert lib.rsp_mask_polygon_pieces(p, p, 1, 4, 65536, 32768, p, 0) != 0
    assert lib.rsp_mask_polygon_edges(p, p, 1, 4, 65536, 32768, p, 1, p, p, p, p, 0) != 0
    assert lib.rsp_mask_polygon_pieces(0, p, 1, 4, 4, 4, p, 0) != 0
    assert lib.rsp_mask_polygon_edges(p, p, 1, 4, 4, 4, p, 2 ** 31 // 6 + 1, p, p, p, p, 0) != 0
    assert lib.rsp_mask_polygon_rank(1, 4, 63, p, p, p, p, p, p, p, p, p, 0) != 0
    assert lib.rsp_mask_polygon_rank_workspace_bytes(-1) == 0 and lib.rsp_mask_polygon_rank_workspace_bytes(2) == 6 * 2 * 28


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
