"""Bodies of the polygon-simplification tests (csrc/ring_simplify.hip, ops.ring_simplify, rle.simplify_polygons,
apis.masks_to_polygons(tolerance=...), large_image polygon_tolerance), shared by both tiers:
tests/test_ring_simplify_cpu.py calls them with the emulated `ops` on CPU tensors, tests/test_gpu_ring_simplify.py with the
real ones on cuda:0.  The reference is tests/_ring_simplify_ref.py, the sequential definition in Python integers; all seven
arrays (and the rounds every input ring took) are compared by exact equality.  The rings come from the reference tracer
tests/_mask_polygons_ref.py or are written out directly, not from the tracing kernels."""
import math

import numpy as np
import torch

import _mask_polygons_cases as mcases
import _mask_polygons_ref as pref
import _ring_simplify_ref as sref

NAMES = mcases.NAMES + ('ring_src', 'rounds')
TOLERANCES = (0, 0.5, 1, 1.5, 2, 5)
AREAS = (0, 2, 9)
NESTED = (0.5, 1, 1.5, 2, 5)


# --------------------------------------------------------------------------------------------------------------- shapes
def disc(rad):
    yy, xx = np.mgrid[:2 * rad + 1, :2 * rad + 1]
    return (yy - rad) ** 2 + (xx - rad) ** 2 <= rad * rad


def staircase(leg=16):
    """the pixels on and below the diagonal of a leg x leg square"""
    return np.tri(leg, leg, dtype=bool)


def l_shape():
    m = np.ones((4, 4), bool)
    m[:2, 2:] = False
    return m


def plus_sign(arm=3, width=3):
    n = 2 * arm + width
    m = np.zeros((n, n), bool)
    m[arm:arm + width, :] = True
    m[:, arm:arm + width] = True
    return m


def diamond(rad=6):
    yy, xx = np.mgrid[:2 * rad + 1, :2 * rad + 1]
    return abs(yy - rad) + abs(xx - rad) <= rad


def diagonal_blobs():
    """a 10 x 10 blob and a 2 x 2 one that touch only diagonally: ONE ring through the saddle vertex twice"""
    m = np.zeros((12, 12), bool)
    m[2:12, 0:10] = True
    m[0:2, 10:12] = True
    return m


def star_ring(count, seed, radius=None):
    """a synthetic simple ring of `count` vertices around a centre (any count, odd ones included): (x, y) Python ints"""
    rng = np.random.default_rng(seed)
    radius = radius or max(40, 2 * count)
    out = []
    for i in range(count):
        t = 2 * math.pi * i / count
        r = radius * (0.55 + 0.45 * float(rng.random()))
        out.append((int(round(radius + r * math.cos(t))), int(round(radius + r * math.sin(t)))))
    return out


def zigzag_ring(teeth=40, side=2 ** 20):
    """a synthetic ring that spans [0, 2^20]^2: a sawtooth along the top from corner to corner and back along the bottom"""
    step = side // teeth
    top = [(i * step, 0 if i % 2 == 0 else side // 3 + 7 * i) for i in range(teeth)] + [(side, 1)]
    return top + [(side, side), (side // 2 + 1, side - 12345), (0, side)]


def rings_as_arrays(rings):
    """synthetic rings (lists of (x, y)), one instance each, all outer -> the six arrays"""
    return pref.flatten([[(np.asarray(r, np.int64).reshape(-1, 2), -1, sref.area2_of(r))] for r in rings])


def traced(mask):
    return pref.flatten([pref.trace(mask)])


# -------------------------------------------------------------------------------------------------------------- helpers
_KEPT = {}


def want_of(key, arrays, tolerance, area=0):
    """the reference's answer; the kept sets of (key, tolerance) are computed once and shared between the areas"""
    q8 = sref.tol2_q8(tolerance)
    pre = _KEPT.get((key, q8)) if key is not None else None
    out, src, rounds, kept = sref.simplify(arrays, q8, area, pre=pre)
    if key is not None:
        _KEPT[(key, q8)] = (kept, rounds.tolist())
    return out + (src, rounds)


def call(ops, dev, arrays, tolerance, area=0, H=None, W=None, variant=0):
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    if H is None:
        side = int(arrays[0].max()) + 1 if len(arrays[0]) else 1
        H = W = side
    return ops.ring_simplify(*t, sref.tol2_q8(tolerance), area, H, W, with_rounds=True, variant=variant)


def assert_equal(got, want, what=''):
    assert len(got) == len(want) == 8
    for name, g, w in zip(NAMES, got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert g.dtype == w.dtype, f'{what}: {name} is {g.dtype}, expected {w.dtype}'
        assert tuple(g.shape) == tuple(w.shape), f'{what}: {name} has shape {tuple(g.shape)}, expected {tuple(w.shape)}'
        assert torch.equal(g.cpu(), w), f'{what}: {name} differs'


def check(ops, dev, key, arrays, tolerance, area=0, H=None, W=None, variants=(0,)):
    want = want_of(key, arrays, tolerance, area)
    for v in variants:
        got = call(ops, dev, arrays, tolerance, area, H, W, v)
        assert_equal(got, want, f'{key} at tolerance {tolerance}, area {area}, variant {v}')
        assert all(g.device.type == torch.device(dev).type for g in got)
    return want


# ---------------------------------------------------------------------------------------------------- the reference itself
def check_reference():
    """on every case mask: kept vertices are a subsequence with v_0, every dropped vertex is within the tolerance of the
    segment between the kept pair around it (fractions), kept sets are nested in the tolerance, tolerance 0 is the identity"""
    shapes = mcases.all_cases() + [('disc 9', disc(9)), ('staircase', staircase()), ('diamond', diamond()),
                                   ('plus', plus_sign()), ('diagonal blobs', diagonal_blobs())]
    rings = 0
    for name, m in shapes:
        for ring, _, _ in pref.trace(m):
            pts = [tuple(v) for v in ring.tolist()]
            assert sref.simplify_ring(pts, 0)[0] == list(range(len(pts))), name          # traced rings: corners only
            last = None
            for tol in reversed(NESTED):                                                   # 5, 2, 1.5, 1, 0.5
                q8 = sref.tol2_q8(tol)
                idx, _ = sref.simplify_ring(pts, q8)
                sref.check_ring(pts, idx, q8)
                assert last is None or set(last) <= set(idx), (name, tol)
                last = idx
            rings += 1
    for count in (3, 5, 65, 257):
        pts = star_ring(count, count)
        for tol in NESTED:
            sref.check_ring(pts, sref.simplify_ring(pts, sref.tol2_q8(tol))[0], sref.tol2_q8(tol))
    return rings


def known_answers():
    """(name, ring, tolerance, kept vertices or None for a dropped ring), worked out by hand"""
    out = []
    for w, h in ((4, 3), (30, 2), (7, 7)):
        rect = [(0, 0), (w, 0), (w, h), (0, h)]
        d = w * h / math.hypot(w, h)                       # from a corner to the diagonal
        out.append((f'{w} x {h} rectangle below', rect, 0.99 * d, rect))
        out.append((f'{w} x {h} rectangle above', rect, 1.01 * d, None))      # two vertices are left: dropped
    out.append(('1 x 1 pixel', [(0, 0), (1, 0), (1, 1), (0, 1)], 1, None))
    stairs = [tuple(v) for v in pref.trace(staircase(16))[0][0].tolist()]
    assert len(stairs) == 34 and stairs[0] == (0, 0) and (16, 16) in stairs and (0, 16) in stairs
    out.append(('staircase at 1', stairs, 1, [(0, 0), (16, 16), (0, 16)]))
    # every step corner is 1 / sqrt 2 = 0.707 from the diagonal and stays at 0.5 -- but for the last step: once (15, 14) is kept,
    # (15, 15) and (16, 15) are 1 / sqrt 5 = 0.447 from the chord (15, 14) - (16, 16).  Below 0.447 the ring stays as it is.
    out.append(('staircase at 0.5', stairs, 0.5, [v for v in stairs if v not in ((15, 15), (16, 15))]))
    out.append(('staircase at 0.44', stairs, 0.44, stairs))
    ell = [(0, 0), (2, 0), (2, 2), (4, 2), (4, 4), (0, 4)]
    assert [tuple(v) for v in pref.trace(l_shape())[0][0].tolist()] == ell
    out.append(('L at 0.8', ell, 0.8, ell))
    out.append(('L at 1', ell, 1, [(0, 0), (2, 0), (4, 4), (0, 4)]))       # (2, 2), (4, 2) are 0.894 from (2, 0) - (4, 4)
    out.append(('L at 1.5', ell, 1.5, [(0, 0), (4, 4), (0, 4)]))           # (2, 0) is 1.414 from the diagonal
    return out


def check_known_answers_of_the_reference():
    for name, ring, tol, want in known_answers():
        idx, _ = sref.simplify_ring(ring, sref.tol2_q8(tol))
        got = [ring[i] for i in idx]
        assert got == (want if want is not None else got) and (want is not None or len(got) < 3), name


# -------------------------------------------------------------------------------------------------------------- kernels
def check_known_answers(ops, dev):
    for name, ring, tol, want in known_answers():
        got = call(ops, dev, rings_as_arrays([ring]), tol)
        if want is None:
            assert got[0].shape[0] == 0 and got[1].cpu().tolist() == [0] and got[5].cpu().tolist() == [0, 0], name
        else:
            assert got[0].cpu().tolist() == [list(v) for v in want] and got[1].cpu().tolist() == [0, len(want)], name
            assert got[4].cpu().tolist() == [sref.area2_of(want)] and got[6].cpu().tolist() == [0], name


def check_case_masks(ops, dev):
    """every mask of the polygon-export cases, traced by the reference tracer, at every tolerance and area"""
    for name, m in mcases.all_cases():
        arrays = pref.flatten([mcases.want_of(name, m)])
        for tol in TOLERANCES:
            for area in AREAS:
                want = check(ops, dev, name, arrays, tol, area, m.shape[0], m.shape[1])
                if tol == 0 and area == 0:                   # the identity on traced rings
                    assert all(np.array_equal(a, b) for a, b in zip(want[:6], arrays))


def check_batch(ops, dev):
    """the batch case (every case mask on one canvas) with rows that have no rings in between; a second launch"""
    H, W, masks, want = mcases.batch_case()
    per_instance = []
    for i, w in enumerate(want):
        if i in (3, 11, len(want) // 2):
            per_instance.append([])
        per_instance.append(w)
    per_instance.append([])
    arrays = pref.flatten(per_instance)
    assert sum(1 for w in per_instance if not w) >= 10 and len(arrays[2]) > 350
    for tol in TOLERANCES:
        for area in (0, 2):
            check(ops, dev, 'batch', arrays, tol, area, H, W)
    a, b = call(ops, dev, arrays, 1, 2, H, W), call(ops, dev, arrays, 1, 2, H, W)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    return arrays


def check_empty_calls(ops, dev):
    z = pref.flatten([[], [], []])                                       # R = 0, k = 3
    assert_equal(call(ops, dev, z, 1, 0, 5, 6), want_of(None, z, 1))
    z = pref.flatten([])                                                 # k = 0
    got = call(ops, dev, z, 1, 0, 5, 6)
    assert_equal(got, want_of(None, z, 1))
    assert got[5].cpu().tolist() == [0] and got[6].shape[0] == 0
    arrays = pref.flatten([pref.trace(mcases.noise64()), [], pref.trace(plus_sign())])
    want = check(ops, dev, None, arrays, 1, 10 ** 6, 64, 64)             # every ring is dropped
    assert want[0].shape == (0, 2) and want[5].tolist() == [0, 0, 0, 0] and want[1].tolist() == [0]
    check(ops, dev, None, arrays, 100, 0, 64, 64)                        # ... and by collapse


def length_rings():
    """ring lengths on both sides of every boundary of the kernels: 64 | 65 (a wave per ring, a block per ring), 128 | 129,
    256 | 257, 512 | 513 (a thread's chunk grows beyond one vertex at 128, 256 or 512 threads), 2048 | 2049 (coordinates in
    LDS, in memory), and rings of several thousand vertices"""
    rings = [star_ring(c, c) for c in (3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049,
                                       5000)]
    per_instance = [[(np.asarray(r, np.int64), -1, sref.area2_of(r))] for r in rings]
    per_instance += [pref.trace(mcases.arm_spiral(n)) for n in (31, 33, 127, 129)]      # 64, 68, 256, 260 vertices
    per_instance += [pref.trace(disc(r)) for r in (1, 13, 60, 520)]
    return pref.flatten(per_instance)


def check_lengths(ops, dev):
    arrays = length_rings()
    lengths = np.diff(arrays[1]).tolist()
    assert {4, 63, 64, 65, 255, 256, 257} <= set(lengths) and max(lengths) >= 5000 and sum(x > 2048 for x in lengths) >= 3
    for tol in (0.5, 2):
        check(ops, dev, 'lengths', arrays, tol, 0, variants=(0, 1, 2, 3))
    return lengths


def check_deep_spiral(ops, dev):
    """arm spirals: the split tree is about as deep as the ring is long"""
    sref.reset_stats()
    arrays = pref.flatten([pref.trace(mcases.arm_spiral(n)) for n in (31, 65)])
    want = check(ops, dev, None, arrays, 1, 0, 65, 65, variants=(0, 3))
    assert sref.STATS['depth'] >= 64 and int(want[7].max()) == sref.STATS['depth']
    return sref.STATS['depth']


def check_ties(ops, dev):
    """shapes whose symmetric vertices are equally far: the lowest index decides"""
    sref.reset_stats()
    comb = np.zeros((9, 15), bool)
    comb[0, :] = True
    comb[:, ::2] = True
    shapes = [np.ones((5, 5), bool), np.ones((8, 8), bool), plus_sign(), plus_sign(5, 1), diamond(6), diamond(9), comb]
    arrays = pref.flatten([pref.trace(m) for m in shapes])
    for tol in (0.5, 1, 2):
        check(ops, dev, None, arrays, tol, 0, 32, 32, variants=(0, 3))
    assert sref.STATS['ties'] >= 10
    return sref.STATS['ties']


def check_zero_chords(ops, dev):
    """chains whose two ends are one point (den = 1, num = |v_i - v_a|^2).  On a closed ring that is the chain (0, m) the
    anchor is taken from -- every ring has it, here the ring of two blobs that touch diagonally, which passes its saddle
    vertex twice.  A later chain (a, b) with v_a = v_b cannot come up unless every vertex between is the same point as well
    (v_b was kept as the farthest vertex of a chain that starts behind a, or ends in front of it, so a kept vertex lies
    between): the synthetic rings below repeat points to take that path too."""
    sref.reset_stats()
    blobs = pref.trace(diagonal_blobs())
    assert len(blobs) == 1 and len({tuple(v) for v in blobs[0][0].tolist()}) == len(blobs[0][0]) - 1
    arrays = pref.flatten([blobs, pref.trace(~diagonal_blobs())])
    for tol in (0, 0.5, 1, 2):
        check(ops, dev, None, arrays, tol, 0, 12, 12, variants=(0, 3))
    assert sref.STATS['zero_chords'] >= 1
    sref.reset_stats()
    same = [[(7, 7)] * 4, [(7, 7)] * 70, [(0, 0), (5, 0), (5, 0), (5, 5), (0, 0), (0, 5)], [(3, 3)], [(1, 1), (9, 9)]]
    arrays = rings_as_arrays(same)
    for tol in (0, 1):
        check(ops, dev, None, arrays, tol, 0, 16, 16, variants=(0, 3))
    assert sref.STATS['inner_zero_chords'] >= 1
    return sref.STATS['inner_zero_chords']


def check_dropped_parents(ops, dev):
    """nested frames: an outer ring that goes takes its holes with it, the parents that stay are re-indexed"""
    nested = dict(mcases.all_cases())['nested frames']
    rings = pref.trace(nested)
    assert [p for _, p, _ in rings] == [-1, 0, -1, 2, -1, 4, -1]
    arrays = pref.flatten([rings, rings])
    # |area2| / 2 of the rings: 169, 121, 81, 49, 25, 9, 1.  At 30 pixels the frames of 25 and less go with their holes.
    want = check(ops, dev, None, arrays, 0.5, 30, 13, 14)
    assert want[6].tolist() == [0, 1, 2, 3, 7, 8, 9, 10] and want[3].tolist() == [-1, 0, -1, 2] * 2
    # at 100 pixels the hole of 81 pixels' outer ring (81) goes, and the hole (49) with it; the outer frame keeps its hole (121)
    want = check(ops, dev, None, arrays, 0.5, 100, 13, 14)
    assert want[6].tolist() == [0, 1, 7, 8] and want[3].tolist() == [-1, 0, -1, 0] and want[5].tolist() == [0, 2, 4]
    # a tolerance that collapses the inner frames: the small square rings (side 1, 3) lose two vertices
    want = check(ops, dev, None, arrays, 2.2, 0, 13, 14)
    par, inst, io = want[3].tolist(), want[2].tolist(), want[5].tolist()
    assert 0 < len(par) < 14 and all(p == -1 or (want[4][io[i] + p] > 0 and want[3][io[i] + p] == -1) for p, i in zip(par, inst))
    for tol in TOLERANCES:
        for area in (0, 9, 30, 100):
            check(ops, dev, 'nested x 2', arrays, tol, area, 13, 14)


def check_wide_coordinates(ops, dev):
    """a ring across [0, 2^20]^2: numerators beyond 2^64"""
    sref.reset_stats()
    ring = zigzag_ring()
    assert min(min(p) for p in ring) == 0 and max(max(p) for p in ring) == 2 ** 20
    arrays = rings_as_arrays([ring, star_ring(300, 1, 2 ** 19)])
    for tol in (0, 1, 1000.5, 65536):
        check(ops, dev, None, arrays, tol, 0, 2 ** 20, 2 ** 20, variants=(0, 3))
    assert sref.STATS['max_num'] > 2 ** 64
    return sref.STATS['max_num']


def check_refusals(ops, dev, pytest):
    arrays = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in traced(plus_sign())]
    ok = ops.ring_simplify(*arrays, 256, 0, 9, 9)
    assert len(ok) == 7
    for bad in (-1, 2 ** 40 + 1, 1.5, None, True):
        with pytest.raises(ValueError, match='tol2_q8'):
            ops.ring_simplify(*arrays, bad, 0, 9, 9)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError, match='min_ring_area'):
            ops.ring_simplify(*arrays, 256, bad, 9, 9)
    with pytest.raises(ValueError, match='2\\^20'):
        ops.ring_simplify(*arrays, 256, 0, 2 ** 20 + 1, 9)
    with pytest.raises(ValueError, match='2\\^20'):
        ops.ring_simplify(*arrays, 256, 0, 9, 0)
    for i, wrong in ((0, arrays[0].to(torch.int64)), (1, arrays[1].to(torch.int32)), (0, arrays[0].reshape(-1)),
                     (4, arrays[4].to(torch.int32)), (2, arrays[2][None])):
        a = list(arrays)
        a[i] = wrong
        with pytest.raises(ValueError, match=NAMES[i]):
            ops.ring_simplify(*a, 256, 0, 9, 9)
    with pytest.raises(ValueError, match='expected verts'):
        ops.ring_simplify(arrays[0], arrays[1][:-1], *arrays[2:], 256, 0, 9, 9)
    with pytest.raises(ValueError, match='expected verts'):
        ops.ring_simplify(arrays[0][:, :1], *arrays[1:], 256, 0, 9, 9)
    # the C entry points, without a launch
    lib = ops._lib.load()
    buf = torch.zeros((64,), dtype=torch.int64, device=dev)            # one ring without vertices; kept alive to the end
    p = buf.data_ptr()
    assert lib.rsp_ring_simplify_mark(p, p, 1, 4, 256, 9, 9, 0, p, p, p, p, p, 0) == 0
    assert lib.rsp_ring_simplify_mark(p, p, 1, 4, -1, 9, 9, 0, p, p, p, p, p, 0) != 0
    assert lib.rsp_ring_simplify_mark(p, p, 1, 4, 2 ** 40 + 1, 9, 9, 0, p, p, p, p, p, 0) != 0
    assert lib.rsp_ring_simplify_mark(p, p, 1, 4, 256, 2 ** 20 + 1, 9, 0, p, p, p, p, p, 0) != 0
    assert lib.rsp_ring_simplify_mark(p, p, 1, 4, 256, 9, 2 ** 20 + 1, 0, p, p, p, p, p, 0) != 0
    assert lib.rsp_ring_simplify_mark(p, p, -1, 4, 256, 9, 9, 0, p, p, p, p, p, 0) != 0
    assert lib.rsp_ring_simplify_mark(p, p, 1, -4, 256, 9, 9, 0, p, p, p, p, p, 0) != 0
    assert lib.rsp_ring_simplify_mark(p, p, 1, 4, 256, 9, 9, 4, p, p, p, p, p, 0) != 0
    assert lib.rsp_ring_simplify_mark(p, 0, 1, 4, 256, 9, 9, 0, p, p, p, p, p, 0) != 0
    assert lib.rsp_ring_simplify_mark(0, p, 1, 4, 256, 9, 9, 0, p, p, p, p, p, 0) != 0
    assert lib.rsp_ring_simplify_mark(p, p, 1, 4, 256, 9, 9, 0, p, p, 0, p, p, 0) != 0
    assert lib.rsp_ring_simplify_survive(p, p, p, p, 1, 1, 0, p, p, p, 0) == 0
    for at, bad in ((4, -1), (5, -1), (6, -1), (0, 0), (3, 0), (7, 0), (9, 0)):
        v = [p, p, p, p, 1, 1, 0, p, p, p, 0]
        v[at] = bad
        assert lib.rsp_ring_simplify_survive(*v) != 0, at
    w = [p] * 5 + [1, 4, 1] + [p] * 5 + [1, 4] + [p] * 7 + [0]
    assert lib.rsp_ring_simplify_write(*w) == 0
    for at, bad in ((5, -1), (6, -1), (7, -1), (13, 2), (14, 5), (0, 0), (8, 0), (12, 0), (16, 0), (21, 0)):
        v = list(w)
        v[at] = bad
        assert lib.rsp_ring_simplify_write(*v) != 0, at
    if torch.device(dev).type != 'cpu':
        torch.cuda.synchronize()
    del buf


# ------------------------------------------------------------------------------------------------------------------ API
def _lists_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for (gr, gp, ga), (wr, wp, wa) in zip(g, w):
            assert gr.dtype == np.int32 and np.array_equal(gr, wr) and (gp, ga) == (wp, wa)


def api_masks():
    cases = dict(mcases.all_cases())
    H, W = 40, 44
    shapes = [cases['comb'], cases['nested frames'], disc(13), staircase(16), plus_sign(), np.zeros((3, 3), bool), ~disc(9)]
    return H, W, [mcases.embed(m, H, W, 2, 1) for m in shapes]


def check_api_forms(apis, rle, dev):
    """the three forms of apis.masks_to_polygons with a tolerance, from all input forms; the defaults are today's output"""
    import _large_image_ref as lref
    H, W, masks = api_masks()
    exact = [pref.trace(m) for m in masks]
    dense = torch.from_numpy(np.stack(masks)).to(dev)
    lists = [dict(size=[H, W], counts=lref.rle_counts_np(m)) for m in masks]
    strings = [dict(size=[H, W], counts=rle.counts_to_string(lref.rle_counts_np(m))) for m in masks]
    for form in ('rings', 'coco', 'geojson'):                        # defaults: what a call without the arguments returns
        a, b = apis.masks_to_polygons(dense, form=form), apis.masks_to_polygons(dense, form=form, tolerance=None, min_ring_area=0)
        if form == 'rings':
            _lists_equal(a, exact)
            _lists_equal(b, exact)
        else:
            assert a == b
    for tol, area in ((1.0, 0), (2, 9), (None, 30), (0.5, 0)):
        want = sref.simplify_lists(exact, sref.tol2_q8(tol or 0), area)
        assert sum(len(r[0]) for w in want for r in w) < sum(len(r[0]) for w in exact for r in w)
        for src in (dense, lists, strings):
            _lists_equal(apis.masks_to_polygons(src, device=dev, tolerance=tol, min_ring_area=area), want)
        coco = apis.masks_to_polygons(dense, form='coco', tolerance=tol, min_ring_area=area)
        for entry, w in zip(coco, want):
            assert entry['holes_dropped'] == any(a2 < 0 for _, _, a2 in w)
            assert entry['polygons'] == [[float(c) for c in ring.reshape(-1).tolist()] for ring, _, a2 in w if a2 > 0]
        geo = apis.masks_to_polygons(dense, form='geojson', tolerance=tol, min_ring_area=area, transform=(10.0, 2.0, 0.0, 5.0, 0.0, -2.0))
        for g, w in zip(geo, want):
            polys = [g['coordinates']] if g['type'] == 'Polygon' else g['coordinates']
            outer = [r for r, (_, par, a2) in enumerate(w) if a2 > 0]
            assert len(polys) == len(outer) and (g['type'] == 'Polygon') == (len(outer) == 1)
            for poly, o in zip(polys, outer):
                rings = [w[o][0]] + [ring for ring, par, a2 in w if par == o]
                assert all(r[0] == r[-1] for r in poly)
                assert [r[:-1] for r in poly] == [[[10.0 + 2.0 * x, 5.0 - 2.0 * y] for x, y in ring.tolist()] for ring in rings]
    want = sref.simplify_lists(exact, sref.tol2_q8(1.0), 0)
    assert len(want[2][0][0]) < len(exact[2][0][0]) // 2                # the disc's staircase
    got = rle.simplify_polygons(tuple(torch.from_numpy(a).to(dev) for a in pref.flatten(exact)), (H, W), 1.0)
    assert len(got) == 2 and len(got[0]) == 6 and got[1].dtype == torch.int32
    _lists_equal(rle.polygons_to_lists(*got[0]), want)


def check_api_refusals(apis, rle, dev, pytest):
    m = torch.zeros((1, 4, 4), dtype=torch.bool, device=dev)
    for bad in (-0.5, float('nan'), float('inf'), -float('inf'), 65536.5, 'wide', True):
        with pytest.raises(ValueError, match='tolerance'):
            apis.masks_to_polygons(m, tolerance=bad)
    for bad in (-1, 2.5, float('nan'), None, 'big', True):
        with pytest.raises(ValueError, match='min_ring_area'):
            apis.masks_to_polygons(m, tolerance=1.0, min_ring_area=bad)
    with pytest.raises(ValueError, match='min_ring_area'):
        apis.masks_to_polygons(m, min_ring_area=-3)
    assert rle.polygon_tolerance_q8(65536) == 2 ** 40 and rle.polygon_tolerance_q8(0.0625) == 1 and rle.polygon_tolerance_q8(0) == 0
    assert apis.masks_to_polygons(m, tolerance=65536.0, min_ring_area=2.0) == [[]]
    polys = tuple(torch.from_numpy(a).to(dev) for a in traced(plus_sign()))
    with pytest.raises(ValueError, match='ring_offs'):
        rle.simplify_polygons((polys[0], polys[1].to(torch.int32)) + polys[2:], (9, 9), 1.0)
    with pytest.raises(ValueError, match='2\\^20'):
        rle.simplify_polygons(polys, (9, 2 ** 20 + 1), 1.0)
    if torch.device(dev).type != 'cpu':                               # arrays of the wrong device
        with pytest.raises(ValueError, match='device'):
            rle.simplify_polygons((polys[0].cpu(),) + polys[1:], (9, 9), 1.0)


# ------------------------------------------------------------------------------------------------------------- pipeline
def check_pipeline(li, dev, scene, model, patch, **kw):
    """inference_large_image(masks='polygons', polygon_tolerance=1.0) against the reference applied to the unsimplified call"""
    exact = li.inference_large_image(model, scene, patch_size=patch, batch_size=3, masks='polygons', **kw)
    again = li.inference_large_image(model, scene, patch_size=patch, batch_size=3, masks='polygons', polygon_tolerance=None,
                                     polygon_min_ring_area=0, **kw)
    _lists_equal(again.pred_instances.masks, exact.pred_instances.masks)
    out = li.inference_large_image(model, scene, patch_size=patch, batch_size=3, masks='polygons', polygon_tolerance=1.0, **kw)
    assert torch.equal(out.keep, exact.keep) and torch.equal(out.pred_instances.bboxes, exact.pred_instances.bboxes)
    want = sref.simplify_lists(exact.pred_instances.masks, sref.tol2_q8(1.0), 0)
    _lists_equal(out.pred_instances.masks, want)
    out2 = li.inference_large_image(model, scene, patch_size=patch, batch_size=3, masks='polygons', polygon_tolerance=2,
                                    polygon_min_ring_area=4, **kw)
    _lists_equal(out2.pred_instances.masks, sref.simplify_lists(exact.pred_instances.masks, sref.tol2_q8(2), 4))
    fc = li.pred2geojson(out, 0.0)
    assert len(fc['features']) == len(want)
    before = sum(len(r[0]) for w in exact.pred_instances.masks for r in w)
    after = sum(len(r[0]) for w in want for r in w)
    assert 0 < after < before
    return len(want), before, after
