"""The host side of the run-table protocol (rsprompter_amd/rle.py over ops.fit_runs), shared by the emulator suite and the
device suite: every pipeline stage started from a capacity that is too small must retry and end with the table -- and the
strings -- of a generous first guess.  The raw kernels' overflow reports have their own tests; this is the loop around
them, which a real scene reaches only when it overflows a generous guess."""
import numpy as np
import torch

import _large_image_ref as ref

TILE_HW, SCENE_HW = (16, 12), (40, 36)
OFFSETS = [(3, 5), (10, 9), (24, 24)]                 # (ox, oy): the column crosses the checkerboard, the empty mask in a corner
GROUPS = [[0, 1], [2]]


def tile_masks():
    """checkerboard, one full column, empty"""
    h, w = TILE_HW
    yy, xx = np.mgrid[:h, :w]
    column = np.zeros((h, w), bool)
    column[:, 7] = True
    return np.stack([(yy + xx) % 2 == 1, column, np.zeros((h, w), bool)])


def _rows(counts, n_host):
    return [counts[i, :int(n_host[i])].tolist() for i in range(len(n_host))]


def check_capacity_retries(ops, dev):
    """encode_runs -> shift_runs -> union_runs -> runs_to_strings from cap = 2 / flat_cap = 1 against the same calls with the
    default capacities, and the strings against the restatement on the dense paste"""
    from oracle import rle as orle
    from rsprompter_amd import rle
    masks = tile_masks()
    (h, w), (H, W) = TILE_HW, SCENE_HW
    md = torch.from_numpy(masks).to(dev)
    off = torch.tensor(OFFSETS, dtype=torch.int32).to(dev)
    goffs = torch.tensor(np.cumsum([0] + [len(g) for g in GROUPS]).astype(np.int32)).to(dev)
    members = torch.tensor([i for g in GROUPS for i in g], dtype=torch.int32).to(dev)
    canvas = np.stack([ref.shift_masks(masks[i:i + 1], OFFSETS[i], SCENE_HW)[0] for i in range(len(masks))])
    want_tile = [ref.rle_counts(m) for m in masks]
    want_scene = [ref.rle_counts(c) for c in canvas]
    want_union = [ref.rle_counts(np.logical_or.reduce(canvas[g], 0)) for g in GROUPS]
    assert len(want_scene[0]) == 193 and len(want_tile[0]) > 2 and len(want_union[0]) > 2

    # the launchers, recorded: how often each ran and what its FIRST attempt reported
    seen = {}

    def record(name, n_of):
        f = getattr(ops, name)

        def g(*a, **k):
            r = f(*a, **k)
            seen.setdefault(name, []).append(n_of(a, r).cpu().tolist())
            return r
        setattr(ops, name, g)
        return name, f
    saved = [record('mask_rle_into', lambda a, r: a[3]), record('rle_shift', lambda a, r: r[1]),
             record('rle_union', lambda a, r: r[1]), record('rle_to_string', lambda a, r: r[1][-1:])]
    try:
        tc, tn, tn_h, tcap = rle.encode_runs(md, cap=2)
        sc, sn, sn_h, scap = rle.shift_runs(tc, tn, off, TILE_HW, SCENE_HW, cap=2)
        uc, un, un_h, ucap = rle.union_runs(sc, sn, SCENE_HW, goffs, members, cap=2)
        s_scene = rle.runs_to_strings(sc, sn, SCENE_HW, flat_cap=1)
        s_union = rle.runs_to_strings(uc, un, SCENE_HW, flat_cap=1)
        tight = {k: [len(v), v[0]] for k, v in seen.items()}
        seen.clear()
        g_tc, g_tn, g_tn_h, _ = rle.encode_runs(md)
        g_sc, g_sn, g_sn_h, _ = rle.shift_runs(g_tc, g_tn, off, TILE_HW, SCENE_HW)
        g_uc, g_un, g_un_h, _ = rle.union_runs(g_sc, g_sn, SCENE_HW, goffs, members)
        g_scene = rle.runs_to_strings(g_sc, g_sn, SCENE_HW)
        g_union = rle.runs_to_strings(g_uc, g_un, SCENE_HW)
        generous = {k: len(v) for k, v in seen.items()}
    finally:
        for name, f in saved:
            setattr(ops, name, f)
    print('attempts and first reports from cap = 2:', tight, '| attempts with the default capacities:', generous)
    # every stage retried, and its first attempt reported the row that needs most
    assert tight['mask_rle_into'] == [2, [-len(c) if len(c) > 2 else len(c) for c in want_tile]]
    assert tight['rle_shift'] == [2, [-193, -3, 1]]
    assert tight['rle_union'] == [2, [-len(want_union[0]), 1]]
    assert tight['rle_to_string'][0] == 4 and tight['rle_to_string'][1][0] > 1          # two tables, two attempts each
    assert generous == dict(mask_rle_into=1, rle_shift=1, rle_union=1, rle_to_string=2)
    assert (tcap, scap, ucap) == (ops.grown_cap(len(want_tile[0])), 256, ops.grown_cap(len(want_union[0])))
    # bit for bit the generous calls' results (a row's entries beyond its n are not written: rows are compared up to n)
    assert tc.shape == g_tc.shape == (3, len(want_tile[0])) and _rows(tc.cpu(), tn_h) == _rows(g_tc.cpu(), g_tn_h)
    for a, b in ((tn, g_tn), (tn_h, g_tn_h), (sn, g_sn), (sn_h, g_sn_h), (un, g_un), (un_h, g_un_h), (tn.cpu(), tn_h),
                 (sn.cpu(), sn_h), (un.cpu(), un_h)):
        assert torch.equal(a, b)
    assert _rows(sc.cpu(), sn_h) == _rows(g_sc.cpu(), g_sn_h) and _rows(uc.cpu(), un_h) == _rows(g_uc.cpu(), g_un_h)
    assert s_scene == g_scene and s_union == g_union
    # and the restatement's on the dense paste
    assert _rows(tc.cpu(), tn_h) == want_tile and _rows(sc.cpu(), sn_h) == want_scene and _rows(uc.cpu(), un_h) == want_union
    size = [H, W]
    assert s_scene == [dict(size=size, counts=orle.rle_to_string(c)) for c in want_scene]
    assert s_union == [dict(size=size, counts=orle.rle_to_string(c)) for c in want_union]
    assert rle.runs_to_dicts(uc, un_h, SCENE_HW) == [dict(size=size, counts=c) for c in want_union]


# ------------------------------------------------------------------------------------------------------------ mask forms
FORM_CANVASES = [(1, 1), (5, 7), (8, 8), (9, 15)]     # one pixel; fewer than 64; exactly one word; three words, the last partial
# device-to-host reads (ReadCounter), measured before the conversions moved into rle.py: the intake of a dense tensor and of
# compressed strings reads n once per attempt, that of lists nothing; check_canonical reads the bad rows (nonzero + tolist);
# one_size=False gathers the rows of every counts form into list order (one nonzero per form)
READS_INTAKE = dict(dense=1, strings=1, lists=0)
READS_CANONICAL = 2
READS_GATHER = 1


def form_masks(H, W, rng):
    """empty, full, pixel 0 only, the last pixel only, the checkerboard of the column-major stream (every other pixel of it:
    every run has length 1, which (y + x) % 2 gives for odd H only), a seeded blob"""
    from scipy import ndimage as ndi
    first, last = np.zeros((H, W), bool), np.zeros((H, W), bool)
    first[0, 0], last[-1, -1] = True, True
    checker = (np.arange(H * W) % 2 == 1).reshape(W, H).T
    blob = ndi.gaussian_filter(rng.standard_normal((H, W)), 1) > 0
    return np.stack([np.zeros((H, W), bool), np.ones((H, W), bool), first, last, checker, blob])


def check_mask_forms(ops, rle, dev, pytest):
    """every conversion between a caller's masks (dense, bytes / str dicts, list dicts) and the run table, both ways, exact"""
    from _run_morphology_cases import ReadCounter
    from oracle import rle as orle
    rng = np.random.default_rng(23)

    def rows(counts, n):
        return _rows(counts.cpu(), n.cpu())

    def reads(fn, *a, **k):
        with ReadCounter(dev) as rc:
            out = fn(*a, **k)
        return rc.n, out
    every = []                                                     # (size, counts) of every mask, for the tables of many sizes
    for H, W in FORM_CANVASES:
        masks = form_masks(H, W, rng)
        want = [ref.rle_counts(m) for m in masks]
        k, size = len(masks), [H, W]
        assert want[0] == [H * W] and want[1] == [0, H * W] and len(want[3]) == 2 and all(c == 1 for c in want[4])
        every += [((H, W), c) for c in want]
        t = torch.from_numpy(masks).to(dev)
        # dense -> table -> dense
        r, (counts, n, sz, form) = reads(rle.masks_to_runs, t, dev, 'frobnicate', canonical=True)
        assert (r, sz, form) == (READS_INTAKE['dense'], (H, W), 'dense') and rows(counts, n) == want
        for back in (rle.runs_to_dense(counts, n, sz), rle.runs_to_masks(counts, n, sz, form)):
            assert back.dtype == torch.bool and back.device == t.device and torch.equal(back, t)
        # table -> dicts of either counts form -> table; str counts are the bytes' table
        packed = rle.runs_to_masks(counts, n, sz, 'strings')
        plain = rle.runs_to_masks(counts, n, sz, 'lists', n.cpu())
        assert packed == [dict(size=size, counts=orle.rle_to_string(c)) for c in want]
        assert plain == [dict(size=size, counts=c) for c in want] == rle.runs_to_masks(counts, n, sz, 'lists')
        text = [dict(size=size, counts=p['counts'].decode()) for p in packed]
        for dicts, kind in ((packed, 'strings'), (text, 'strings'), (plain, 'lists')):
            for canonical in (False, True):
                r, (c2, n2, sz2, form2) = reads(rle.masks_to_runs, dicts, dev, 'frobnicate', canonical=canonical)
                assert (r, sz2, form2) == (READS_INTAKE[kind] + READS_CANONICAL * canonical, (H, W), kind)
                assert rows(c2, n2) == want
            out = rle.runs_to_masks(c2, n2, sz2, form2)            # the form that came in (bytes for str)
            assert out == (packed if kind == 'strings' else plain)
        assert reads(rle.check_canonical, counts, n, sz, 'frobnicate')[0] == READS_CANONICAL
        # the bit planes: ops.rle_to_bits at word offsets made by hand
        nw = (H * W + 63) // 64
        woff = torch.tensor([i * nw for i in range(k + 1)], dtype=torch.int64).to(dev)
        bits, word_offs, area, wrange = rle.runs_to_bits(counts, n, [size] * k)
        b2, a2, w2 = ops.rle_to_bits(counts, n, woff)
        assert torch.equal(word_offs, woff) and torch.equal(bits, b2) and torch.equal(area, a2) and torch.equal(wrange, w2)
        assert area.cpu().tolist() == [int(m.sum()) for m in masks]
        # capacity retry: the checkerboard from cap = 2 is the default's table
        chk = want[4]
        r, (c3, n3, _, _) = reads(rle.masks_to_runs, t[4:5], dev, 'frobnicate', cap=2)
        assert rows(c3, n3) == [chk] and r == READS_INTAKE['dense'] * (2 if len(chk) > 2 else 1)
        r, (c3, n3) = reads(rle.strings_to_runs, [packed[4]['counts']], dev, cap=2)
        assert rows(c3, n3) == [chk] and r == READS_INTAKE['strings'] * (2 if len(chk) > 2 else 1)
        assert rows(*rle.masks_to_runs(packed[4:5], dev, 'frobnicate', cap=2)[:2]) == [chk]
        # k = 0 through every direction
        c0, n0, sz0, form0 = rle.masks_to_runs(t[:0], dev, 'frobnicate')
        assert (int(n0.shape[0]), sz0, form0) == (0, (H, W), 'dense')
        assert tuple(rle.runs_to_dense(c0, n0, sz0).shape) == (0, H, W)
        assert rle.runs_to_masks(c0, n0, sz0, 'strings') == [] and rle.runs_to_masks(c0, n0, sz0, 'lists') == []
        assert rle.runs_to_bits(c0, n0, [])[1].cpu().tolist() == [0] and rle.runs_to_bits(c0, n0, [])[2].shape[0] == 0
        assert reads(rle.check_canonical, c0, n0, sz0, 'frobnicate')[0] == 0
    for empty in (rle.strings_to_runs([], dev), rle.lists_to_runs([], dev)):
        assert tuple(empty[1].shape) == (0,) and empty[0].shape[0] == 0 and empty[0].dtype == empty[1].dtype == torch.int32
    # one_size=False: sizes of their own, packed and plain counts side by side, rows in list order
    a, b = dict(size=[2, 3], counts=[1, 2, 3]), dict(size=[4, 1], counts=orle.rle_to_string([0, 3, 1]))
    r, (counts, n, sizes, form) = reads(rle.masks_to_runs, [a, b, a], dev, 'frobnicate', one_size=False)
    assert sizes == [(2, 3), (4, 1), (2, 3)] and n.cpu().tolist() == [3, 3, 3] and form == 'mixed'
    assert counts.cpu()[:, :3].tolist() == [[1, 2, 3], [0, 3, 1], [1, 2, 3]]
    assert r == READS_INTAKE['strings'] + READS_INTAKE['lists'] + 2 * READS_GATHER == 3
    assert reads(rle.masks_to_runs, [a, a], dev, 'frobnicate', one_size=False)[0] == READS_INTAKE['lists'] + READS_GATHER
    assert reads(rle.masks_to_runs, [b], dev, 'frobnicate', one_size=False)[0] == READS_INTAKE['strings'] + READS_GATHER
    r, (c0, n0, sizes, _) = reads(rle.masks_to_runs, [], dev, 'frobnicate', one_size=False)
    assert (r, c0.shape[0], tuple(n0.shape), sizes) == (0, 0, (0,), [])
    # every mask of every canvas in one table, alternating counts forms: the rows, and bit planes at offsets of many sizes
    dicts = [dict(size=list(s), counts=orle.rle_to_string(c) if i % 2 else c) for i, (s, c) in enumerate(every)]
    counts, n, sizes, form = rle.masks_to_runs(dicts, dev, 'frobnicate', one_size=False)
    assert rows(counts, n) == [c for _, c in every] and sizes == [s for s, _ in every] and form == 'mixed'
    woff = torch.tensor(np.cumsum([0] + [(h * w + 63) // 64 for (h, w), _ in every]), dtype=torch.int64).to(dev)
    bits, word_offs, area, wrange = rle.runs_to_bits(counts, n, sizes)
    b2, a2, w2 = ops.rle_to_bits(counts, n, woff)
    assert torch.equal(word_offs, woff) and torch.equal(bits, b2) and torch.equal(area, a2) and torch.equal(wrange, w2)
    assert area.cpu().tolist() == [sum(c[1::2]) for _, c in every]
    # refusals: `what` heads every message
    t = torch.zeros((2, 5, 7), dtype=torch.bool).to(dev)
    with pytest.raises(ValueError, match=r'frobnicate: .*\[k, H, W\]'):
        rle.masks_to_runs(t[0], dev, 'frobnicate')
    with pytest.raises(ValueError, match='frobnicate: an empty list'):
        rle.masks_to_runs([], dev, 'frobnicate')
    with pytest.raises(ValueError, match='frobnicate: .*share one size'):
        rle.masks_to_runs([a, b], dev, 'frobnicate')
    with pytest.raises(ValueError, match='frobnicate: compressed .* and uncompressed'):
        rle.masks_to_runs([a, dict(b, size=[2, 3])], dev, 'frobnicate')
    with pytest.raises(ValueError, match="mask form 'mixed'"):
        rle.runs_to_masks(counts, n, (5, 7), 'mixed')
    for bad in ([3, 0, 32], [3, 4], [0, 0, 35]):                   # a zero count after the first (twice); a sum other than H W
        for cnts in (bad, orle.rle_to_string(bad)):
            dicts = [dict(size=[5, 7], counts=cnts)]
            assert rle.masks_to_runs(dicts, dev, 'frobnicate')[3] in ('strings', 'lists')          # refused on request only
            with pytest.raises(ValueError, match='frobnicate: the counts of mask 0 are not canonical'):
                rle.masks_to_runs(dicts, dev, 'frobnicate', canonical=True)
    for bad in ([36, -1], [2 ** 31, 1]):                           # a negative count; a count of 32 bits and more in a list
        for one_size in (True, False):
            with pytest.raises(ValueError, match='frobnicate: not canonical .* 32 bits'):
                rle.masks_to_runs([dict(size=[5, 7], counts=bad)], dev, 'frobnicate', one_size=one_size)
    with pytest.raises(ValueError, match='lists_to_runs: not canonical'):
        rle.lists_to_runs([[36, -1]], dev)
    good, zero = dict(size=[5, 7], counts=[35]), dict(size=[5, 7], counts=[3, 0, 32])
    with pytest.raises(ValueError, match='frobnicate: the counts of mask 1 .*; 2 masks in all'):
        rle.masks_to_runs([good, zero, zero], dev, 'frobnicate', canonical=True)
