"""Bodies of the tests of the device-side run-table reader (csrc/run_table.h: the row, the walk, the columns of a
ones-run), shared by both tiers: tests/test_run_walk_cpu.py calls them with the emulated `ops` on CPU tensors,
tests/test_gpu_run_walk.py with the real ones on cuda:0.

ONE table aims at the chunk edges of the walk (256 runs per chunk): rows of n in ROW_LENGTHS and one row with a negative n
(an overflow report, read as empty) on a canvas of height 5.  Run lengths come from RUN_LENGTHS (the last run of a row
is lengthened to the end of the canvas), so ones-runs cross column ends and the runs of 11 span three columns; the row of 257
starts with a zero count (pixel 0 set).  cap = the longest row + 7 and every slot at or beyond a row's n holds POISON: a
lane that read one would move every pixel start behind it.  Every consumer of the walk runs on that table and on the same
table with those slots zeroed; both must give the dense numpy answer.  Everything is compared exactly."""
import functools

import numpy as np
import torch

import _large_image_ref as lref
import _mask_polygons_cases as poly_cases
import _mask_polygons_ref as pref
import _seam_merge_ref as sref

ROW_LENGTHS = (0, 1, 2, 3, 255, 256, 257, 511, 512, 513)
RUN_LENGTHS = (1, 2, 3, 7, 11)
H = 5
POISON = 0x7fffffff
ZERO_FIRST = 257                     # the row of this length starts with a zero count


@functools.lru_cache(maxsize=None)
def table():
    """-> dict(W, cap, rows = run-count lists (None: the row with a negative n), n = list, dense = bool [H, W] per row)"""
    rng = np.random.default_rng(21)
    drawn = []
    for length in ROW_LENGTHS:
        c = rng.choice(RUN_LENGTHS, length).tolist()
        if length == ZERO_FIRST:
            c[0] = 0
        drawn.append(c)
    W = -(-max(sum(c) for c in drawn) // H)
    rows = []
    for c in drawn:
        if c:
            c[-1] += H * W - sum(c)                                   # the last run reaches the end of the canvas
        rows.append(c)
    rows.insert(5, None)                                              # in between: the overflow report
    n = [-(len(ROW_LENGTHS) + 600) if r is None else len(r) for r in rows]
    dense = [lref.counts_to_mask(r or [H * W], H, W) for r in rows]
    cap = max(ROW_LENGTHS) + 7
    assert 300 < W < 1000 and dense[ROW_LENGTHS.index(ZERO_FIRST) + 1][0, 0]
    spans = []                                                        # columns touched by every drawn ones-run
    for r in rows:
        s = np.cumsum([0] + (r or [0])[:-1])[1:-1:2]
        spans += ((s + np.asarray((r or [0])[1:-1:2]) - 1) // H - s // H + 1).tolist()
    assert spans.count(2) > 100 and spans.count(3) > 10
    return dict(W=W, cap=cap, rows=rows, n=n, dense=dense)


def tensors(dev, fill):
    """the table on `dev` with `fill` in every slot at or beyond a row's n"""
    t = table()
    counts = torch.full((len(t['rows']), t['cap']), fill, dtype=torch.int32)
    for i, r in enumerate(t['rows']):
        if r:
            counts[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return counts.to(dev), torch.tensor(t['n'], dtype=torch.int32, device=dev)


def both(dev):
    """[(name, counts, n)]: the poisoned table and the zeroed one"""
    return [('poisoned',) + tensors(dev, POISON), ('zeroed',) + tensors(dev, 0)]


def check_rle_bbox(ops, dev):
    t = table()
    want = [sref.bbox_area_dense(m) for m in t['dense']]
    assert want[0] == want[5] == ([0, 0, 0, 0], 0)                   # n = 0 and n < 0
    for name, counts, n in both(dev):
        boxes, area = ops.rle_bbox(counts, n, H, t['W'])
        got = list(zip(boxes.cpu().tolist(), area.cpu().tolist()))
        assert got == want, (name, [i for i in range(len(want)) if got[i] != want[i]])


def check_rle_pair_overlap(ops, dev):
    """every row with its neighbour; the rectangle of pair i cuts columns (and rows), at another place for every pair"""
    t = table()
    k, W = len(t['rows']), t['W']
    pairs = [(i, (i + 1) % k) for i in range(k)]
    rects = [(7 * i + 1, i % 3, W - 11 * i - 2, 3 + i % 3) for i in range(k)]
    want = [list(sref.pair_overlap_dense(t['dense'][i], t['dense'][j], r)) for (i, j), r in zip(pairs, rects)]
    assert sum(w[0] > 0 for w in want) >= 4 and sum(0 < w[1] < int(t['dense'][i].sum()) for (i, _), w in zip(pairs, want)) >= 4
    for name, counts, n in both(dev):
        got = ops.rle_pair_overlap(counts, n, H, W, torch.tensor(pairs, dtype=torch.int32, device=dev),
                                   torch.tensor(rects, dtype=torch.int32, device=dev)).cpu().tolist()
        assert got == want, (name, [i for i in range(k) if got[i] != want[i]])


def check_rle_union(ops, dev):
    """groups of one return the row's own counts (an empty row: the empty canvas); neighbouring pairs the dense OR"""
    t = table()
    k, W = len(t['rows']), t['W']
    groups = [[i] for i in range(k)] + [[i, (i + 1) % k] for i in range(k)]
    want = [r or [H * W] for r in t['rows']]
    want += [lref.rle_counts_np(t['dense'][i] | t['dense'][j]) for i, j in groups[k:]]
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(g) for g in groups])]), dtype=torch.int32, device=dev)
    mem = torch.tensor([i for g in groups for i in g], dtype=torch.int32, device=dev)
    for name, counts, n in both(dev):
        out, no = ops.rle_union(counts, n, H, W, offs, mem, 2 * t['cap'])
        out, no = out.cpu(), no.cpu().tolist()
        assert no == [len(w) for w in want], name
        bad = [g for g, w in enumerate(want) if out[g, :no[g]].tolist() != w]
        assert not bad, (name, bad)


def check_mask_polygons(ops, dev):
    t = table()
    want = pref.flatten([pref.check_traced(m) if r else [] for r, m in zip(t['rows'], t['dense'])])
    assert len(want[2]) > 100                                         # rings
    for name, counts, n in both(dev):
        poly_cases.assert_arrays_equal(ops.mask_polygons(counts, n, H, t['W']), want, name)


def check_rle_shift(ops, dev):
    """the rows as 5-row tiles placed into a scene of height 9 (every ones-run splits at its column ends) and of height 5
    (columns stay adjacent: runs are not split), against the dense paste, re-encoded"""
    t = table()
    k, W = len(t['rows']), t['W']
    for SH in (9, 5):
        SW = W + 3
        offsets = [(i % 4, (2 * i + 1) % (SH - H + 1)) for i in range(k)]
        want = [lref.rle_counts_np(lref.shift_masks(m[None], o, (SH, SW))[0]) if r else []
                for r, m, o in zip(t['rows'], t['dense'], offsets)]
        cap_out = max(len(w) for w in want) + 1
        for name, counts, n in both(dev):
            out, no = ops.rle_shift(counts, n, torch.tensor(offsets, dtype=torch.int32, device=dev), (H, W), (SH, SW), cap_out)
            out, no = out.cpu(), no.cpu().tolist()
            assert no == [len(w) for w in want], (SH, name)
            bad = [i for i, w in enumerate(want) if out[i, :no[i]].tolist() != w]
            assert not bad, (SH, name, bad)
