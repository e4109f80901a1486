"""Case bodies of polygon rasterisation (csrc/poly_raster.hip, ops.poly_raster, rle.polygons_to_runs, datasets.anns_to_rle,
apis.polygons_to_masks, CocoMetric(gt_raster=...), large_image --from-geojson), shared by the emulator tier
(tests/test_poly_raster_cpu.py) and the device tier (tests/test_gpu_poly_raster.py).

The oracle is tests/_cocoeval_ref.py: rle_fr_poly / rle_fr_bbox / rle_merge / rle_decode / rle_encode, the literal restatement
of cocoapi's maskApi.c.  Every comparison is == on run counts; there is no tolerance in this file.  The even-odd fill of
several rings has no function in cocoapi: its oracle is the XOR of the rings' decoded rle_fr_poly masks, encoded again (the
boundaries of the joint crossing multiset are the symmetric difference of the rings' boundaries: DESIGN §14.11)."""
import json
import os

import numpy as np
import torch

import _cocoeval_ref as ref
import _coco_cases as cc
import _mask_polygons_cases as mp_cases

THREADS = 256                       # PR_THREADS of csrc/poly_raster.hip


# ------------------------------------------------------------------------------------------------------------- helpers
def ring(*xy):
    return np.asarray(xy, np.float64).reshape(-1, 2)


def square(x0, y0, x1, y1):
    return ring(x0, y0, x1, y0, x1, y1, x0, y1)


def walk_points(rings):
    """the walk points rleFrPoly makes of these rings: max(|dx|, |dy|) + 1 per edge of every closed ring"""
    total = 0
    for r in rings:
        s = [(int(5.0 * float(x) + .5), int(5.0 * float(y) + .5)) for x, y in np.asarray(r).reshape(-1, 2)]
        for j in range(len(s)):
            e = s[(j + 1) % len(s)]
            total += max(abs(e[0] - s[j][0]), abs(e[1] - s[j][1])) + 1
    return total


def tensors(groups, hws, dev):
    """groups: per group a list of float64 [m, 2] rings; hws: (h, w) per group -> the four arrays of ops.poly_raster"""
    rings = [np.asarray(r, np.float64).reshape(-1, 2) for g in groups for r in g]
    offs = np.cumsum([0] + [len(r) for r in rings]).astype(np.int64)
    verts = np.concatenate(rings + [np.zeros((0, 2))]).reshape(-1, 2)
    group = np.repeat(np.arange(len(groups), dtype=np.int32), [len(g) for g in groups])
    return (torch.from_numpy(verts).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(group).to(dev),
            torch.tensor([list(hw) for hw in hws], dtype=torch.int32, device=dev).view(len(hws), 2))


def rows(counts, n):
    """a run table -> per row the list of its counts"""
    c, m = counts.cpu().numpy().astype(np.int64) & 0xffffffff, n.cpu().tolist()
    assert all(v > 0 for v in m), f'rows that did not fit or are empty: {m}'
    return [c[i, :m[i]].tolist() for i in range(len(m))]


def raster(ops, dev, groups, hws, cap=64):
    counts, n, n_host, cap = ops.poly_raster(*tensors(groups, hws, dev), cap)
    assert counts.dtype == torch.int32 and n.dtype == torch.int32 and counts.shape == (len(groups), cap)
    assert counts.device.type == torch.device(dev).type and n_host.tolist() == n.cpu().tolist()
    return rows(counts, n)


def want_ring(r, h, w):
    r = np.asarray(r, np.float64).reshape(-1, 2)
    return ref.rle_fr_poly(r.reshape(-1).tolist(), h, w) if len(r) else [h * w]


def want_evenodd(group, h, w):
    if len(group) == 1:
        return want_ring(group[0], h, w)
    m = np.zeros((h, w), np.uint8)
    for r in group:
        m ^= ref.rle_decode(want_ring(r, h, w), h, w)
    return ref.rle_encode(m)


def want_union(group, h, w):
    return ref.rle_merge([want_ring(r, h, w) for r in group]) if group else [h * w]


def assert_canonical(cnts, h, w, what=''):
    assert sum(cnts) == h * w and all(c > 0 for c in cnts[1:]) and cnts[0] >= 0, f'{what}: {cnts} on {h} x {w}'


def check_groups(ops, dev, groups, hws, what, cap=64):
    got = raster(ops, dev, groups, hws, cap)
    for i, (g, (h, w)) in enumerate(zip(groups, hws)):
        assert_canonical(got[i], h, w, f'{what} [{i}]')
        assert got[i] == want_evenodd(g, h, w), f'{what} [{i}]: {[r.tolist() for r in g]} on {h} x {w}'
    return got


# -------------------------------------------------------------------------------------------------------- hand-checked
def check_hand_checked(ops, dev):
    """answers worked out by hand, asserted on the oracle and on the kernels"""
    cases = [
        ('unit square', square(0, 0, 1, 1), (2, 2), [0, 1, 3]),                      # pixel (0, 0) alone
        ('triangle with a 45 degree edge', ring(0, 0, 4, 0, 0, 4), (4, 4), [0, 3, 1, 2, 2, 1, 7]),   # columns of 3, 2, 1 pixels
        ('one-pixel-wide sliver', square(2, 0, 3, 5), (5, 5), [10, 5, 10]),          # column 2 from top to bottom
        ('the whole canvas', square(0, 0, 2, 2), (2, 2), [0, 4]),
    ]
    for name, r, (h, w), counts in cases:
        assert want_ring(r, h, w) == counts, name
    got = raster(ops, dev, [[r] for _, r, _, _ in cases], [hw for _, _, hw, _ in cases])
    assert got == [c for _, _, _, c in cases]
    for name, r, hw, counts in cases:                                               # and each alone
        assert raster(ops, dev, [[r]], [hw]) == [counts], name


# ------------------------------------------------------------------------------------------------- committed annotations
_NWPU = {}


def nwpu():
    """the 26 committed NWPU annotations -> (segmentations, sizes, the oracle's counts per annotation), made once"""
    if not _NWPU:
        with open(cc.FIXTURE_JSON) as f:
            d = json.load(f)
        hw = {im['id']: (im['height'], im['width']) for im in d['images']}
        segms = [a['segmentation'] for a in d['annotations']]
        sizes = [hw[a['image_id']] for a in d['annotations']]
        want = [ref.rle_merge([ref.rle_fr_bbox(p, h, w) if len(p) == 4 else ref.rle_fr_poly(p, h, w) for p in s])
                for s, (h, w) in zip(segms, sizes)]
        _NWPU.update(segms=segms, sizes=sizes, want=want, json=d)
    return _NWPU['segms'], _NWPU['sizes'], _NWPU['want']


def check_nwpu_annotations(ops, datasets, dev):
    """one batched call with mixed group_hw; then datasets.anns_to_rle against the oracle's strings and datasets.ann_to_rle"""
    segms, sizes, want = nwpu()
    assert len(segms) == 26 and len(set(sizes)) == 6 and sum(len(p) // 2 for s in segms for p in s) == 518
    groups = [[ring(*p) for p in s] for s in segms]
    assert all(len(g) == 1 for g in groups)
    assert raster(ops, dev, groups, sizes) == want
    got = datasets.anns_to_rle(segms, sizes, dev)
    assert got == [dict(size=[h, w], counts=ref.rle_to_string(c)) for c, (h, w) in zip(want, sizes)]
    assert got == [datasets.ann_to_rle(s, h, w) for s, (h, w) in zip(segms, sizes)]


# ------------------------------------------------------------------------------------------------ seeded random polygons
_RANDOM = {}


def random_polygons(count=2000, seed=2000):
    """count polygons of 3 .. 12 float vertices on canvases from 1 x 1 to 64 x 64; a third of the vertices on the .5 and .1
    grids (rounding ties of (int)(5 x + .5) and of the walk), a fifth outside the canvas on every side (negative values:
    truncation toward zero) -> (rings, sizes, oracle counts), made once and shared"""
    key = (count, seed)
    if key not in _RANDOM:
        rng = np.random.default_rng(seed)
        rings, sizes = [], []
        for i in range(count):
            h, w = (1, 1) if i == 0 else (int(rng.integers(1, 65)), int(rng.integers(1, 65)))
            k = int(rng.integers(3, 13))
            xy = rng.uniform(0.0, 1.0, (k, 2))
            axes = rng.integers(1, 4, (k, 1))                                 # bit 0: x leaves the canvas, bit 1: y
            out = (rng.random((k, 1)) < 0.2) & ((axes & [1, 2]) != 0)         # a fifth of the vertices outside, on every side
            far = rng.uniform(0.02, 0.6, (k, 2)) * np.where(rng.random((k, 2)) < 0.5, -1.0, 1.0)
            xy = np.where(out, np.where(far < 0, far, 1.0 + far), xy) * [w, h]
            grid = rng.random((k, 1))                                         # a third of the vertices on the .5 and .1 grids
            xy = np.where(grid < 1 / 6, np.round(xy * 2) / 2, np.where(grid < 1 / 3, np.round(xy * 10) / 10, xy))
            rings.append(xy)
            sizes.append((h, w))
        _RANDOM[key] = (rings, sizes, [want_ring(r, h, w) for r, (h, w) in zip(rings, sizes)])
    return _RANDOM[key]


def check_random_polygons(ops, dev, count=2000):
    rings, sizes, want = random_polygons(count)
    v = np.concatenate(rings)
    lim = np.concatenate([np.tile([w, h], (len(r), 1)) for r, (h, w) in zip(rings, sizes)])
    outside = ((v < 0) | (v > lim)).any(1).mean()
    on_grid = (np.abs(v * 10 - np.round(v * 10)) < 1e-9).all(1).mean()
    assert 0.17 < outside < 0.23 and 0.3 < on_grid < 0.37 and (v < 0).any() and sizes[0] == (1, 1)
    got = raster(ops, dev, [[r] for r in rings], sizes, cap=16)
    bad = [i for i in range(count) if got[i] != want[i]]
    assert not bad, f'{len(bad)} of {count} polygons differ, first {bad[0]}: {rings[bad[0]].tolist()} on {sizes[bad[0]]}: ' \
                    f'{got[bad[0]]} != {want[bad[0]]}'
    assert len({tuple(c) for c in want}) > count // 2 and sum(len(c) > 1 for c in want) > count // 2


# ------------------------------------------------------------------------------------------------------ degenerate rings
def degenerate_groups():
    g = [
        ('no vertices', [ring()], (5, 7)),
        ('one vertex', [ring(2.3, 1.7)], (5, 7)),
        ('two vertices', [ring(1, 1, 4.5, 3)], (5, 7)),
        ('two equal vertices', [ring(2, 2, 2, 2)], (5, 7)),
        ('repeated vertices', [ring(1, 1, 1, 1, 4, 1, 4, 1, 4, 4, 4, 4, 1, 4, 1, 4, 1, 1)], (6, 6)),
        ('zero-length edge at the start', [ring(1, 1, 1, 1, 4, 1, 4, 4)], (6, 6)),
        ('collinear edges', [ring(0, 0, 2, 0, 5, 0, 5, 2.5, 5, 5, 0, 5)], (6, 6)),
        ('collinear on a slope', [ring(0, 0, 2, 1, 4, 2, 6, 3, 0, 3)], (4, 7)),
        ('axis-only ring', [ring(1, 1, 3, 1, 3, 2, 5, 2, 5, 5, 1, 5)], (6, 6)),
        ('horizontal line', [ring(0, 2, 6, 2)], (5, 6)),
        ('vertical line', [ring(3, 0, 3, 5)], (5, 6)),
        ('wholly right of the canvas', [square(10, 1, 14, 4)], (5, 6)),
        ('wholly left of the canvas', [square(-14, 1, -10, 4)], (5, 6)),
        ('wholly above', [square(1, -9, 4, -3)], (5, 6)),
        ('wholly below', [square(1, 7, 4, 12)], (5, 6)),
        ('around the canvas', [square(-3, -3, 9, 9)], (5, 6)),
        ('H = 1', [ring(0.4, -1, 6.2, 0.3, 3, 2)], (1, 7)),
        ('H = 1, a box', [square(1, 0, 4, 1)], (1, 7)),
        ('W = 1', [ring(-1, 0.4, 0.3, 6.2, 2, 3)], (7, 1)),
        ('W = 1, a box', [square(0, 1, 1, 4)], (7, 1)),
        ('1 x 1 covered', [square(-1, -1, 2, 2)], (1, 1)),
        ('1 x 1 missed', [square(0.6, 0.6, 3, 3)], (1, 1)),
        ('negative ties', [ring(-0.1, -0.1, -0.3, 4.1, 3.1, 4.5, 2.9, -0.5)], (5, 4)),
    ]
    return g


def check_degenerate(ops, dev):
    g = degenerate_groups()
    got = check_groups(ops, dev, [x[1] for x in g], [x[2] for x in g], 'degenerate rings, batched')
    for (name, group, hw), batched in zip(g, got):
        assert check_groups(ops, dev, [group], [hw], name) == [batched], name
    by = {name: c for (name, _, _), c in zip(g, got)}
    assert by['no vertices'] == by['one vertex'] == by['two equal vertices'] == [35]
    assert by['wholly right of the canvas'] == by['wholly left of the canvas'] == by['wholly above'] == [30]
    assert by['around the canvas'] == [0, 30] and by['1 x 1 covered'] == [0, 1] and by['1 x 1 missed'] == [1]
    assert by['H = 1, a box'] == [1, 3, 3] and by['W = 1, a box'] == [1, 3, 3]
    assert by['repeated vertices'] == want_ring(square(1, 1, 4, 4), 6, 6)
    # no rings at all, and nothing at all
    assert raster(ops, dev, [[], []], [(3, 4), (1, 1)]) == [[12], [1]]
    counts, n, n_host, _ = ops.poly_raster(*tensors([], [], dev))
    assert counts.shape[0] == 0 and n.shape[0] == 0 and n_host.numel() == 0


# ------------------------------------------------------------------------------------------------------------ tail rule
def check_tail_rule(ops, dev):
    """the closed form of rleFrPoly's tail: multiplicity parity below h w, h w always"""
    a, b = square(1, 1, 3, 3), square(3, 1, 5, 3)
    spike = ring(1, 1, 3, 1, 3, 3, 5, 3, 3, 3, 1, 3)                       # the edge (3, 3) -> (5, 3) and back
    cases = [
        ('two rings touching along an edge: even multiplicity on it', [a, b], (6, 6)),
        ('the same ring twice cancels', [a, a], (6, 6)),
        ('three times the same ring', [a, a, a], (6, 6)),
        ('a spike traversed twice', [spike], (6, 6)),
        ('odd multiplicity at position 0', [square(0, 0, 2, 1)], (2, 2)),
        ('even multiplicity at position 0', [square(0, 0, 2, 1), square(0, 0, 1, 2)], (2, 2)),
        ('crossings exactly at h w: a vertex at (w, h)', [square(2, 1, 4, 3)], (3, 4)),
        ('crossings at h w, twice', [square(2, 1, 4, 3), square(3, 2, 4, 3)], (3, 4)),
        ('no crossing at all: a vertical line', [ring(2, 0, 2, 3)], (3, 4)),
        ('no crossing at all: outside', [square(9, 9, 12, 12)], (3, 4)),
        ('a hole', [square(0, 0, 6, 6), square(2, 2, 4, 4)], (6, 6)),
    ]
    got = check_groups(ops, dev, [c[1] for c in cases], [c[2] for c in cases], 'tail rule')
    by = {name.split(':')[0]: c for (name, _, _), c in zip(cases, got)}
    assert by['two rings touching along an edge'] == want_ring(square(1, 1, 5, 3), 6, 6) == [7, 2, 4, 2, 4, 2, 4, 2, 9]
    assert by['the same ring twice cancels'] == [36] and by['three times the same ring'] == want_ring(a, 6, 6)
    assert by['a spike traversed twice'] == want_ring(square(1, 1, 3, 3), 6, 6)
    assert by['odd multiplicity at position 0'] == [0, 1, 1, 1, 1] and by['even multiplicity at position 0'] == [1, 2, 1]
    assert by['crossings exactly at h w'] == [7, 2, 1, 2] and by['crossings at h w, twice'] == [7, 2, 1, 1, 1]
    assert by['no crossing at all'] == [12]
    # the rule itself against the sequential loop, on random multisets of positions (host only: the oracle of the oracle)
    rng = np.random.default_rng(7)
    for _ in range(300):
        hw = int(rng.integers(1, 40))
        pos = rng.integers(0, hw + 1, int(rng.integers(0, 30))).tolist()
        srt = sorted(pos + [hw])
        diffs = [srt[0]] + [srt[i] - srt[i - 1] for i in range(1, len(srt))]
        seq, j = [diffs[0]], 1
        while j < len(diffs):
            if diffs[j] > 0:
                seq.append(diffs[j])
                j += 1
            else:
                j += 1
                if j < len(diffs):
                    seq[-1] += diffs[j]
                    j += 1
        bounds = sorted(p for p in set(pos) if p < hw and pos.count(p) % 2 == 1) + [hw]
        assert seq == [bounds[0]] + [bounds[i] - bounds[i - 1] for i in range(1, len(bounds))], (pos, hw)


# ------------------------------------------------------------------------------------------------------ launch geometry
def _corner(a, b):
    """a ring of 2 a + b + 3 walk points (b <= a, in fifths of a pixel): (0, 0) -> (a, 0) -> (a, b)"""
    return ring(0, 0, a / 5, 0, a / 5, b / 5)


def check_launch_geometry(ops, dev):
    for total, (a, b) in ((63, (25, 10)), (64, (25, 11)), (65, (25, 12)), (THREADS - 1, (120, 12)), (THREADS, (120, 13)),
                          (THREADS + 1, (120, 14))):
        r = _corner(a, b)
        assert walk_points([r]) == total
        check_groups(ops, dev, [[r]], [(4, 30)], f'{total} walk points')
    # one edge far longer than a block's share of the points
    long = ring(0, 1, 1999.8, 30)
    assert walk_points([long]) == 2 * 10000
    check_groups(ops, dev, [[long], [ring(0, 35, 1999.8, 2, 700, 39)]], [(40, 2000), (40, 2000)], '10 000-point edges')
    # 4 096 one-edge rings (one vertex each: one zero-length edge, no crossing), one group each and all in one group
    dots = [ring(i % 64 + 0.5, i // 64 + 0.5) for i in range(4096)]
    assert walk_points(dots) == 4096
    assert raster(ops, dev, [[d] for d in dots], [(64, 64)] * 4096) == [[4096]] * 4096
    assert raster(ops, dev, [dots], [(64, 64)]) == [[4096]]
    # ... and 4 096 two-vertex rings (two edges, there and back: crossings of even multiplicity wherever they land)
    rng = np.random.default_rng(4096)
    segs = [ring(*rng.uniform(-1, 9, 4)) for _ in range(4096)]
    assert raster(ops, dev, [[s] for s in segs], [(8, 8)] * 4096) == [want_ring(s, 8, 8) for s in segs]
    # empty groups between full ones, rings without vertices between rings with, and a second launch on the same buffers
    groups = [[], [square(1, 1, 4, 4)], [], [], [ring(), square(0, 0, 2, 2), ring(), square(1, 1, 3, 3)], [ring()], [],
              [ring(0.5, 0.5, 7.5, 3, 2, 6.5)], []]
    hws = [(3, 3), (5, 6), (1, 1), (9, 2), (4, 4), (2, 2), (7, 7), (8, 8), (6, 5)]
    check_groups(ops, dev, groups, hws, 'empty groups between full ones')
    launch = ops.poly_raster_launcher(*tensors(groups, hws, dev))
    first, second = launch(16), launch(16)
    sorted_along = ops.poly_raster_launcher(*tensors(groups, hws, dev), compact=False)      # the empty slots sorted along
    assert rows(*sorted_along(16)) == rows(*first) and sorted_along.walk_points == launch.walk_points == walk_points(
        [r for g in groups for r in g]) and int(sorted_along.crossings) == int(launch.crossings) > 0
    assert rows(*first) == rows(*second) == [want_evenodd(g, h, w) for g, (h, w) in zip(groups, hws)]


# ------------------------------------------------------------------------------------------------------------- capacity
def check_capacity(ops, dev):
    groups = [[square(1, 1, 3, 3)], [ring(0.5, 0.5, 15.5, 3, 2, 14.5, 9, 9)], []]
    hws = [(6, 6), (16, 16), (2, 2)]
    want = [want_evenodd(g, h, w) for g, (h, w) in zip(groups, hws)]
    need = max(len(c) for c in want)
    assert need > 8 and [len(c) for c in want][::2] == [5, 1]
    launch = ops.poly_raster_launcher(*tensors(groups, hws, dev))
    counts, n = launch(need - 1)                                   # one short: the widest row reports -(needed), the others fit
    assert n.cpu().tolist() == [5, -need, 1]
    counts, n = launch(need)
    assert rows(counts, n) == want
    counts, n, n_host, cap = ops.fit_runs(launch, 2)               # the retry: up from a capacity nothing but [h w] fits
    assert cap == ops.grown_cap(need) and counts.shape[1] == cap and rows(counts, n) == want
    assert rows(*ops.poly_raster(*tensors(groups, hws, dev), 1)[:2]) == want


# --------------------------------------------------------------------------------------------------------------- limits
def check_limits(ops, dev, pytest):
    """out-of-range coordinates, canvases of 2^31 pixels and more, and too many walk points: RSP_EINVAL from the C entry (-1),
    a ValueError that names the limit from the wrapper; NaN and inf before any launch"""
    lib = ops._lib.load()
    EINVAL = ops.CONST['RSP_EINVAL']
    assert EINVAL == -1 and ops.POLY_RASTER_MAX_COORD == 1 << 24
    verts, offs, group, hw = tensors([[square(1, 1, 3, 3)]], [(6, 6)], dev)
    scaled = torch.zeros((4, 2), dtype=torch.int32, device=dev)
    edge_pts = torch.zeros((4,), dtype=torch.int64, device=dev)
    px = torch.zeros((1,), dtype=torch.int64, device=dev)
    assert lib.rsp_poly_raster_edges(verts.data_ptr(), offs.data_ptr(), hw.data_ptr(), 1, 4, 1, scaled.data_ptr(),
                                     edge_pts.data_ptr(), px.data_ptr(), ops._stream()) == 0
    edge_offs = torch.cat([edge_pts.new_zeros((1,)), torch.cumsum(edge_pts, 0)]).contiguous()
    T = int(edge_offs[-1])
    assert T == 44 and int(px[0]) == 36 and int(scaled.abs().max()) == 15
    keys = torch.empty((T,), dtype=torch.int64, device=dev)

    def crossings(T=T, coord_max=15, pixels_max=36):
        return lib.rsp_poly_raster_crossings(scaled.data_ptr(), offs.data_ptr(), group.data_ptr(), hw.data_ptr(),
                                             edge_offs.data_ptr(), 1, 4, 1, T, coord_max, pixels_max, keys.data_ptr(),
                                             ops._stream())
    assert crossings() == 0
    assert crossings(coord_max=1 << 24) == 0 and crossings(coord_max=(1 << 24) + 1) == EINVAL
    assert crossings(pixels_max=2 ** 31 - 1) == 0 and crossings(pixels_max=2 ** 31) == EINVAL
    assert crossings(T=2 ** 31) == EINVAL and crossings(T=3) == EINVAL and crossings(T=-1) == EINVAL
    counts = torch.empty((1, 8), dtype=torch.int32, device=dev)
    n = torch.zeros((1,), dtype=torch.int32, device=dev)
    offs1 = torch.tensor([0, 0], dtype=torch.int64, device=dev)

    def runs(pixels_max=36, cap=8, K=0):
        return lib.rsp_poly_raster_runs(keys.data_ptr(), K, offs1.data_ptr(), hw.data_ptr(), 1, pixels_max, counts.data_ptr(),
                                        n.data_ptr(), cap, ops._stream())
    assert runs() == 0 and rows(counts, n) == [[36]]
    assert runs(pixels_max=2 ** 31) == EINVAL and runs(cap=0) == EINVAL and runs(K=-1) == EINVAL and runs(K=2 ** 31) == EINVAL
    # the edges call pins what is out of range (and tells through group_px), so that nothing behind it can fault
    far = torch.tensor([[4e6, -4e6], [1e300, 0.0], [0.0, 0.0]], dtype=torch.float64, device=dev)
    big = torch.tensor([[65536, 32768], [0, 5], [46341, 46341]], dtype=torch.int32, device=dev)
    sc, ep, gp = torch.zeros((3, 2), dtype=torch.int32, device=dev), torch.zeros((3,), dtype=torch.int64, device=dev), \
        torch.zeros((3,), dtype=torch.int64, device=dev)
    o3 = torch.tensor([0, 3], dtype=torch.int64, device=dev)
    assert lib.rsp_poly_raster_edges(far.data_ptr(), o3.data_ptr(), big.data_ptr(), 1, 3, 3, sc.data_ptr(), ep.data_ptr(),
                                     gp.data_ptr(), ops._stream()) == 0
    assert sc.cpu().tolist() == [[(1 << 24) + 2, -(1 << 24) - 2], [(1 << 24) + 2, 0], [0, 0]]
    assert gp.cpu().tolist() == [2 ** 31, 2 ** 31, 2 ** 31] and ep.cpu().tolist() == [(1 << 24) + 3] * 3
    # the wrapper
    one = [[square(1, 1, 3, 3)]]
    for bad_hw in ((65536, 32768), (46341, 46341), (0, 5), (5, -1)):
        with pytest.raises(ValueError, match='2\\^31 pixels'):
            ops.poly_raster(*tensors(one, [bad_hw], dev))
    assert raster(ops, dev, [[]], [(46340, 46340)]) == [[46340 * 46340]]
    with pytest.raises(ValueError, match='scales beyond'):
        ops.poly_raster(*tensors([[square(1, 1, 3.4e6, 3)]], [(6, 6)], dev))
    with pytest.raises(ValueError, match='scales beyond'):
        ops.poly_raster(*tensors([[square(-3.4e6, 1, 3, 3)]], [(6, 6)], dev))
    edge = (1 << 24) / 5.0                                         # the largest coordinate that is taken
    assert raster(ops, dev, [[ring(edge, 1, edge, 3)]], [(6, 6)]) == [[36]]
    for bad in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='NaN or infinite'):
            ops.poly_raster(*tensors([[ring(1, 1, bad, 2, 3, 3)]], [(6, 6)], dev))
    v, o, g, h = tensors([[square(1, 1, 3, 3)], [square(0, 0, 1, 1)]], [(6, 6), (2, 2)], dev)
    with pytest.raises(ValueError, match='ring_group'):
        ops.poly_raster(v, o, torch.tensor([1, 0], dtype=torch.int32, device=dev), h)
    with pytest.raises(ValueError, match='ring_group'):
        ops.poly_raster(v, o, torch.tensor([0, 2], dtype=torch.int32, device=dev), h)
    with pytest.raises(ValueError, match='ring_offs'):
        ops.poly_raster(v, torch.tensor([0, 5, 8], dtype=torch.int64, device=dev)[[0, 2, 1]].contiguous(), g, h)
    with pytest.raises(ValueError, match='float64'):
        ops.poly_raster(v.to(torch.float32), o, g, h)


# ----------------------------------------------------------------------------------------------------------- fill rules
def check_fill_rules(rle, apis, datasets, dev, pytest):
    a, b = square(1, 1, 5, 5), square(3, 3, 8, 7)
    h, w = 9, 10
    ma, mb = ref.rle_decode(want_ring(a, h, w), h, w), ref.rle_decode(want_ring(b, h, w), h, w)
    assert (ma & mb).sum() == 4 and ma.sum() == 16 and mb.sum() == 20
    t = tensors([[a, b], [], [b], [a, a]], [(h, w), (3, 3), (h, w), (4, 4)], dev)
    got = {f: rows(*rle.polygons_to_runs(*t, fill=f)) for f in rle.POLYGON_FILLS}
    assert got['union'] == [ref.rle_encode(ma | mb), [9], want_ring(b, h, w), want_ring(a, 4, 4)]
    assert got['evenodd'] == [ref.rle_encode(ma ^ mb), [9], want_ring(b, h, w), [16]]
    assert got['union'][0] == want_union([a, b], h, w) and got['union'][0] != got['evenodd'][0]
    with pytest.raises(ValueError, match='fill'):
        rle.polygons_to_runs(*t, fill='nonzero')
    # union over instances of several canvas sizes: one rsp_rle_union call per size, single-part rows untouched
    groups = [[a, b], [b], [a, b, square(0, 0, 2, 2)], [], [b, a], [square(0, 0, 1, 1), square(1, 1, 2, 2)]]
    hws = [(9, 10), (9, 10), (12, 12), (5, 5), (9, 10), (2, 2)]
    got = rows(*rle.polygons_to_runs(*tensors(groups, hws, dev), fill='union', cap=2))
    assert got == [want_union(g, *hw) for g, hw in zip(groups, hws)]
    # the API: COCO lists default to union (= ann_to_rle), a 4-number entry is an xywh box, flat and nested lists
    flat = a.reshape(-1).tolist()
    polys = [[flat, b.reshape(-1).tolist()], flat, [[3, 3, 5, 4]], [flat, [3, 3, 5, 4]], dict(polygons=[flat]), []]
    out = apis.polygons_to_masks(polys, (h, w), device=dev)
    assert out[:4] == [datasets.ann_to_rle(p, h, w) for p in polys[:4]]
    assert out[2] == dict(size=[h, w], counts=ref.rle_to_string(ref.rle_fr_bbox([3, 3, 5, 4], h, w))) and out[4] == out[1]
    assert out[5] == dict(size=[h, w], counts=ref.rle_to_string([h * w]))
    assert out[3] == dict(size=[h, w], counts=ref.rle_to_string(ref.rle_encode(ma | mb)))
    xor = apis.polygons_to_masks(polys[:1], (h, w), fill='evenodd', device=dev)
    assert xor == [dict(size=[h, w], counts=ref.rle_to_string(ref.rle_encode(ma ^ mb)))]
    counts, n = apis.polygons_to_masks(polys[:1], (h, w), form='runs', device=dev)
    assert rows(counts, n) == [ref.rle_encode(ma | mb)]
    dense = apis.polygons_to_masks(polys[:2] + [[]], (h, w), form='dense', device=dev)
    assert dense.dtype == torch.bool and dense.shape == (3, h, w)
    assert np.array_equal(dense.cpu().numpy(), np.stack([ma | mb, ma, np.zeros_like(ma)]).astype(bool))
    assert datasets.anns_to_rle(polys[:4] + [out[0], dict(size=[h, w], counts=[h * w])], (h, w), dev) == \
        out[:4] + [out[0], dict(size=[h, w], counts=ref.rle_to_string([h * w]))]
    assert datasets.anns_to_rle([], [], dev) == [] and datasets.anns_to_rle([[]], [(3, 3)], dev) == [datasets.ann_to_rle([], 3, 3)]


def check_api_refusals(apis, dev, pytest):
    sq = [[1, 1, 3, 1, 3, 3, 1, 3]]
    gj = dict(type='Polygon', coordinates=[[[1, 1], [3, 1], [3, 3], [1, 3], [1, 1]]])
    with pytest.raises(ValueError, match='mask form'):
        apis.polygons_to_masks([sq], (5, 5), form='png', device=dev)
    with pytest.raises(ValueError, match='fill'):
        apis.polygons_to_masks([sq], (5, 5), fill='winding', device=dev)
    with pytest.raises(ValueError, match='pass fill'):
        apis.polygons_to_masks([sq, gj], (5, 5), device=dev)
    assert len(apis.polygons_to_masks([sq, gj], (5, 5), fill='evenodd', device=dev)) == 2
    with pytest.raises(ValueError, match='singular'):
        apis.polygons_to_masks([gj], (5, 5), transform=(0, 1, 2, 0, 2, 4), device=dev)
    with pytest.raises(ValueError, match='2\\^31'):
        apis.polygons_to_masks([sq], (65536, 32768), device=dev)
    with pytest.raises(ValueError, match='NaN or infinite'):
        apis.polygons_to_masks([[[1, 1, float('nan'), 1, 3, 3]]], (5, 5), device=dev)
    with pytest.raises(ValueError, match='GeoJSON'):
        apis.polygons_to_masks([dict(type='Point', coordinates=[1, 1])], (5, 5), device=dev)
    from rsprompter_amd import large_image as li
    with pytest.raises(ValueError, match='dense masks'):
        apis.polygons_to_masks([sq] * 8, (40000, 40000), form='dense', device=dev)
    assert li.DENSE_MASK_LIMIT_BYTES < 8 * 40000 * 40000


# ----------------------------------------------------------------------------------------------------------- round trip
GEO = (500000.0, 0.25, 0.0, 4649776.0, 0.0, -0.25)     # power-of-two scales, a large integer origin: exactly invertible


def check_round_trip(apis, rle, dev, cases=None):
    """every mask -> masks_to_polygons -> polygons_to_masks: the same run table bit for bit, for 'rings' and for 'geojson'"""
    cases = mp_cases.all_cases() if cases is None else cases
    for name, m in cases:
        H, W = m.shape
        masks = torch.from_numpy(np.ascontiguousarray(m[None])).to(dev)
        counts, n, n_host, _ = rle.encode_runs(masks)
        want = rows(counts, n)
        rings = apis.masks_to_polygons(masks, form='rings', device=dev)
        c, k = apis.polygons_to_masks(rings, (H, W), form='runs', device=dev)
        assert rows(c, k) == want, f'{name}: rings'
        gj = apis.masks_to_polygons(masks, form='geojson', transform=GEO, device=dev)
        c, k = apis.polygons_to_masks(gj, (H, W), form='runs', transform=GEO, device=dev)
        assert rows(c, k) == want, f'{name}: geojson'
        assert want[0] == ref.rle_encode(m), name


def check_round_trip_batch(apis, rle, dev, masks, what):
    """k masks of one canvas in one call each way; 'rle' strings equal to the encoder's"""
    k, H, W = masks.shape
    t = torch.from_numpy(masks).to(dev)
    counts, n, n_host, _ = rle.encode_runs(t)
    want = rle.runs_to_strings(counts, n, (H, W))
    polys = rle.runs_to_polygons(counts, n, (H, W))
    c, m = rle.polygons_to_runs(polys[0].to(torch.float64), polys[1], polys[2],
                                torch.tensor([[H, W]] * k, dtype=torch.int32, device=dev), fill='evenodd')
    assert torch.equal(m, n), what
    live = torch.arange(c.shape[1], device=c.device)[None] < m[:, None]
    width = min(int(c.shape[1]), int(counts.shape[1]))
    assert int(m.max()) <= width, what
    assert torch.equal(torch.where(live, c, 0)[:, :width], torch.where(live[:, :width], counts[:, :width], 0)), what
    assert rle.runs_to_strings(c.contiguous(), m, (H, W)) == want, what
    return int(polys[1].shape[0]) - 1, int(polys[0].shape[0])


# ----------------------------------------------------------------------------------------------------------- CocoMetric
def check_coco_metric_parity(evaluation, datasets, dev):
    """CocoMetric(gt_raster='device') on the NWPU golden subset: the ground-truth RLE strings of 'host', and its stats"""
    segms, sizes, want = nwpu()
    d = _NWPU['json']
    hw = {im['id']: (im['height'], im['width']) for im in d['images']}
    rng = np.random.default_rng(26)
    per_img = {}
    classes, cat_ids = [c['name'] for c in d['categories']], [c['id'] for c in d['categories']]    # labels index the JSON's order
    for a, c in zip(d['annotations'], want):
        h, w = hw[a['image_id']]
        x, y, bw, bh = a['bbox']
        jit = rng.uniform(-3, 3, 4)
        box = [x + jit[0], y + jit[1], x + bw + jit[2], y + bh + jit[3]]
        per_img.setdefault(a['image_id'], []).append((box, float(rng.uniform(0.3, 1.0)), cat_ids.index(a['category_id']),
                                                      dict(size=[h, w], counts=ref.rle_to_string(c))))
    out = {}
    for how in ('host', 'device'):
        m = evaluation.CocoMetric(ann_file=cc.FIXTURE_JSON, metric=['bbox', 'segm'], device=str(dev), gt_raster=how)
        assert m.gt_raster == how
        m.dataset_meta = dict(classes=classes)
        samples = []
        for im in d['images']:
            p = per_img.get(im['id'], [])
            pi = dict(bboxes=torch.tensor([q[0] for q in p], dtype=torch.float32).view(-1, 4),
                      scores=torch.tensor([q[1] for q in p], dtype=torch.float32),
                      labels=torch.tensor([q[2] for q in p], dtype=torch.int64), masks=[q[3] for q in p])
            samples.append(dict(pred_instances=pi, img_id=im['id'], ori_shape=(im['height'], im['width'])))
        m.process(None, samples)
        res = m.evaluate(len(samples))
        gt = m._gt_with_rles(m.coco_gt, dev)
        out[how] = (res, [a['segmentation'] for a in gt['annotations']],
                    {t: m.eval_results[t].stats.copy() for t in ('bbox', 'segm')})
    assert out['host'][1] == out['device'][1] and len(out['host'][1]) == 26
    assert out['host'][1] == [dict(size=list(s), counts=ref.rle_to_string(c)) for s, c in zip(sizes, want)]
    assert out['host'][0] == out['device'][0] and len(out['host'][0]) == 12
    for t in ('bbox', 'segm'):
        assert np.array_equal(out['host'][2][t], out['device'][2][t], equal_nan=True), t
    # the predictions carry the ground truth's own masks and jittered boxes: a run that matches, not one of all zeros
    # (the ann_file path counts the detection matched to annotation id 0 as a false positive, so segm is not 1 either)
    assert 0.5 < out['host'][2]['bbox'][0] < out['host'][2]['segm'][0] <= 1.0
    import pytest
    with pytest.raises(ValueError, match='gt_raster'):
        evaluation.CocoMetric(gt_raster='gpu')


# ------------------------------------------------------------------------------------------------------------------ CLI
def check_cli(li, apis, dev, tmp_path, monkeypatch, model, scene_path, argv_tail):
    """--from-geojson on the output of --mask-format geojson gives the RLE strings of --mask-format rle"""
    monkeypatch.setattr(apis, 'init_detector', lambda cfg, ckpt, device=None: model)
    argv = [scene_path, 'cfg.py', 'none'] + argv_tail + ['--device', str(dev)]
    li.main(argv + ['--out-dir', str(tmp_path / 'rle')])
    geo = [str(v) for v in GEO]
    li.main(argv + ['--out-dir', str(tmp_path / 'geo'), '--mask-format', 'geojson', '--geo-transform'] + geo)
    name = os.path.splitext(os.path.basename(scene_path))[0]
    want = json.loads((tmp_path / 'rle' / f'{name}.json').read_text())
    layer = tmp_path / 'geo' / f'{name}.geojson'
    H, W = want['masks'][0]['size']
    li.main(['--from-geojson', str(layer), '--size', str(H), str(W), '--out-dir', str(tmp_path / 'back'), '--device', str(dev),
             '--geo-transform'] + geo)
    got = json.loads((tmp_path / 'back' / f'{name}.json').read_text())
    assert len(want['masks']) > 3 and got['masks'] == want['masks']
    assert got['labels'] == want['labels'] and got['scores'] == want['scores'] and got['bboxes'] == want['bboxes']
    # without the transform the layer is in pixel coordinates
    li.main(argv + ['--out-dir', str(tmp_path / 'px'), '--mask-format', 'geojson'])
    li.main(['--from-geojson', str(tmp_path / 'px' / f'{name}.geojson'), '--size', str(H), str(W), '--out-dir',
             str(tmp_path / 'back_px'), '--device', str(dev)])
    assert json.loads((tmp_path / 'back_px' / f'{name}.json').read_text())['masks'] == want['masks']
    import pytest
    with pytest.raises(SystemExit):
        li.main(['--from-geojson', str(layer), '--out-dir', str(tmp_path / 'x')])          # --size is required
    return len(want['masks'])
