"""Bodies of the run-domain mask IoU tests (csrc/coco_iou_runs.hip, ops.run_prefix / ops.coco_iou_runs, CocoMetric's
iou_domain, apis.mask_iou, evaluate(large_image=...)), shared by both tiers: tests/test_coco_iou_runs_cpu.py
calls them with the emulated `ops` on CPU tensors, tests/test_gpu_coco_iou_runs.py with the real ones on cuda:0.

The oracle is tests/_cocoeval_ref.py: `rle_iou`, cocoapi's rleIou loop by loop (LITERAL_IOU below is that function whatever
`use_numpy_forms` did to the module since), `rle_area`, `coco_stats`, `rle_encode`.  Every comparison is ==.

One property of the literal walk matters for non-canonical counts: rleIou's loop ends when BOTH cursors hold a count of
zero after their refill (`ct == 0`), which happens in the middle of a stream exactly when both rows hold a zero count at one
stream position.  Its answer is then the IoU of the prefix.  The kernel counts pixels; the cases below make one row of a
pair non-canonical where they are compared with the literal walk (no such coincidence can arise), and compare pairs of two
non-canonical rows with the pixel count of the decoded streams and with the bits route."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _cocoeval_ref as ref  # noqa: E402
import _seam_merge_cases as seam_cases  # noqa: E402

LITERAL_IOU = ref.rle_iou
assert LITERAL_IOU.__name__ == 'rle_iou'

rows_from_counts = seam_cases.rows_from_counts


# ------------------------------------------------------------------------------------------------------------ references
def stream(c):
    """run counts -> the 0 / 1 stream they describe (any counts)"""
    out = np.zeros(int(sum(c)), bool)
    p = 0
    for i, v in enumerate(c):
        if i & 1:
            out[p:p + v] = True
        p += v
    return out


def prefix_np(c):
    """(workspace entries [2 * ones-runs], area, extent) of one row"""
    starts = np.concatenate([[0], np.cumsum(np.asarray(c, np.int64))])[:len(c)] if len(c) else np.zeros(0, np.int64)
    ws, ones, lo, hi = [], 0, None, 0
    for i in range(1, len(c), 2):
        ws += [ones, int(starts[i])]
        ones += int(c[i])
        if c[i] > 0:
            lo = int(starts[i]) if lo is None else lo
            hi = int(starts[i]) + int(c[i])
    return ws, ones, (lo or 0, hi) if hi else (0, 0)


def check_prefix(ops, dev, rows, cap=None):
    """ops.run_prefix on a table of these rows (None = the empty row) against prefix_np"""
    counts, n = rows_from_counts(rows, dev, cap)
    ws, area, ext = ops.run_prefix(counts, n)
    assert ws.shape == counts.shape and ws.dtype == torch.int32 and area.dtype == torch.int64 and ext.dtype == torch.int32
    assert area.shape == (len(rows),) and ext.shape == (len(rows), 2)
    ws, area, ext = ws.cpu().numpy(), area.cpu().tolist(), ext.cpu().tolist()
    for i, r in enumerate(rows):
        w, a, e = prefix_np(r or [])
        assert ws[i, :len(w)].tolist() == w, (i, r)
        assert area[i] == a == ref.rle_area(r or []), (i, r)
        assert tuple(ext[i]) == e, (i, r, ext[i], e)
    return counts, n


def literal(d, g, hw, crowd):
    """rleIou of one pair on an (h, w) canvas; an empty ROW shares no pixel with anything"""
    if not d or not g:
        return 0.0
    return float(LITERAL_IOU([(list(d), hw[0], hw[1])], [(list(g), hw[0], hw[1])], [crowd])[0, 0])


def pixel_iou(d, g, crowd):
    """the definition on the decoded streams: what the kernel must give for ANY counts"""
    if not d or not g:
        return 0.0
    a, b = stream(d), stream(g)
    m = min(len(a), len(b))
    inter = int((a[:m] & b[:m]).sum())
    if inter == 0:
        return 0.0
    return inter / (int(a.sum()) if crowd else int(a.sum()) + int(b.sum()) - inter)


def units_of(blocks):
    """[(nd, ng)] -> the unit columns, blocks back to back in all three arrays"""
    nd = np.array([b[0] for b in blocks], np.int64)
    ng = np.array([b[1] for b in blocks], np.int64)
    z = lambda v: np.concatenate([[0], np.cumsum(v)[:-1]]).astype(np.int64)          # noqa: E731
    return z(nd), z(ng), z(nd * ng), nd, ng


def run_units(ops, dev, dt_rows, gt_rows, blocks, crowd, hws=None, dt_cap=None, gt_cap=None, want='literal', bits=False):
    """The units `blocks` over the two row lists through ops.coco_iou_runs, every pair against the reference (`want`:
    'literal' needs hws = the canvas of every unit, 'pixels' does not), the prefixes against numpy, a second launch for the
    same bits; bits=True: the same units through rsp_rle_to_bits + rsp_coco_iou as well.  -> (iou, info)"""
    dt0, gt0, out0, nd, ng = units_of(blocks)
    n_iou = int((nd * ng).sum())
    dc, dn = check_prefix(ops, dev, dt_rows, dt_cap)
    gc, gn = check_prefix(ops, dev, gt_rows, gt_cap)
    units = ops.coco_units(dt0, gt0, out0, nd, ng, np.zeros(len(nd), np.int64), dev)
    g_crowd = torch.tensor(list(crowd) + [0], dtype=torch.uint8, device=dev)
    info = {}
    iou = ops.coco_iou_runs(units, n_iou, (dc, dn), (gc, gn), g_crowd, info=info)
    assert iou.dtype == torch.float64 and iou.shape == (n_iou,)
    again = ops.coco_iou_runs(units, n_iou, (dc, dn), (gc, gn), g_crowd)
    assert torch.equal(iou.view(torch.int64), again.view(torch.int64))
    got = iou.cpu().numpy()
    for u in range(len(nd)):
        for d in range(nd[u]):
            for g in range(ng[u]):
                a, b, c = dt_rows[dt0[u] + d], gt_rows[gt0[u] + g], crowd[gt0[u] + g]
                w = literal(a, b, hws[u], c) if want == 'literal' else pixel_iou(a, b, c)
                assert got[out0[u] + d * ng[u] + g] == w, (u, d, g, got[out0[u] + d * ng[u] + g], w, a, b)
    if bits:
        nwords = np.array([(h * w + 63) // 64 for h, w in hws], np.int64)

        def words(rows, first, cnt):
            per = np.zeros(len(rows), np.int64)
            for u in range(len(cnt)):
                per[first[u]:first[u] + cnt[u]] = nwords[u]
            return torch.from_numpy(np.concatenate([[0], np.cumsum(per)])).to(dev)
        dwo, gwo = words(dt_rows, dt0, nd), words(gt_rows, gt0, ng)
        db, da, dwr = ops.rle_to_bits(dc, dn, dwo)
        gb, ga, gwr = ops.rle_to_bits(gc, gn, gwo)
        ub = ops.coco_units(dt0, gt0, out0, nd, ng, nwords, dev)
        via_bits = ops.coco_iou(ub, n_iou, ops.COCO_IOU_SEGM, gt_crowd=g_crowd, dt_bits=db, gt_bits=gb, dt_woff=dwo,
                                gt_woff=gwo, dt_wrange=dwr, gt_wrange=gwr, dt_area=da, gt_area=ga)
        assert torch.equal(iou.view(torch.int64), via_bits.view(torch.int64))
    return got, info


def enc(mask):
    return [int(v) for v in ref.rle_encode(mask)]


# ------------------------------------------------------------------------------------------------------- hand-checked pairs
def check_hand_checked(ops, dev):
    H, W = 7, 9
    z = lambda: np.zeros((H, W), bool)                                               # noqa: E731
    outer, inner = z(), z()
    outer[1:6, 2:7] = True                                                           # 25 pixels
    inner[2:4, 3:6] = True                                                           # 6 of them

    def of_stream(sl):                                                               # pixels of the column-major stream
        flat = np.zeros(H * W, bool)
        flat[sl] = True
        return flat.reshape(W, H).T
    left = of_stream(slice(5, 20))                                                   # stream [5, 20): crosses two column ends
    right = of_stream(slice(20, 33))                                                 # starts where `left` ends: touching
    even = of_stream(slice(10, 40, 2))                                               # interleaved single-pixel stripes:
    odd = of_stream(slice(11, 41, 2))                                                # overlapping extents, no common pixel
    first, last = z(), z()
    first[:3, 0] = True                                                              # pixel 0 set: a leading zero count
    last[4:, W - 1] = True                                                           # the last pixel set: an even n
    far = of_stream(slice(50, 60))
    masks = dict(outer=outer, inner=inner, left=left, right=right, even=even, odd=odd, first=first, last=last, far=far,
                 ones=np.ones((H, W), bool), zeros=z())
    names = list(masks) + ['empty row']
    rows = [enc(m) for m in masks.values()] + [None]
    assert rows[names.index('first')][0] == 0 and len(rows[names.index('last')]) % 2 == 0
    assert rows[names.index('ones')] == [0, 63] and rows[names.index('zeros')] == [63] and rows[names.index('left')] == [5, 15, 43]
    k = len(rows)
    for crowd in (0, 1):
        got, info = run_units(ops, dev, rows, rows, [(k, k)], [crowd] * k, [(H, W)], bits=False)
        iou = got.reshape(k, k)
        at = lambda a, b: iou[names.index(a), names.index(b)]                        # noqa: E731
        for nm in names[:-2]:
            if nm != 'zeros':
                assert at(nm, nm) == 1.0, nm
        assert at('zeros', 'zeros') == 0.0 and at('empty row', 'ones') == 0.0 and at('ones', 'empty row') == 0.0
        assert at('inner', 'outer') == (6 / 6 if crowd else 6 / 25) and at('outer', 'inner') == 6 / 25
        assert at('left', 'right') == 0.0 and at('right', 'left') == 0.0 and at('left', 'far') == 0.0
        assert at('even', 'odd') == 0.0 and at('odd', 'even') == 0.0
        assert at('ones', 'outer') == (25 / 63) and at('outer', 'ones') == (1.0 if crowd else 25 / 63)
        assert at('first', 'ones') == (1.0 if crowd else 3 / 63) and at('last', 'ones') == (1.0 if crowd else 3 / 63)
        # the filter: touching and disjoint extents never reach the walk; the stripes do
        ext = [prefix_np(r or [])[2] for r in rows]
        alive = sum(1 for a in ext for b in ext if max(a[0], b[0]) < min(a[1], b[1]))
        assert info == dict(pairs=k * k, survivors=alive) and alive < k * k
    # the same rows through the bits route (an empty row has no bits: without it)
    run_units(ops, dev, rows[:-1], rows[:-1], [(k - 1, k - 1)], [0, 1] * 5 + [0], [(H, W)], bits=True)


# ------------------------------------------------------------------------------------------------- wave and chunk boundaries
RUNS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)


def alternating(R, off, total):
    """R ones-runs of one pixel, every other pixel from `off` on"""
    if R == 0:
        return [total]
    c = [off] + [1] * (2 * R - 1)
    rest = total - sum(c)
    assert rest >= 0
    return c + ([rest] if rest else [])


def check_wave_boundaries(ops, dev):
    H, W = 40, 37
    N = H * W
    rng = np.random.default_rng(41)
    rows = [alternating(R, (7 * i) % 23 + (0 if i % 3 else 1), N) for i, R in enumerate(RUNS)]
    rows[3] = alternating(63, 0, N)                                                  # pixel 0 set
    rows[-1] = alternating(513, N - 2 * 513 + 1, N)                                  # the last pixel set
    assert len(rows[-1]) % 2 == 0
    dense = enc(rng.random((H, W)) < 0.5)                                            # about 370 ones-runs
    sparse = [431, 3, 400, 2, 644]                                                   # two short runs
    block = [100, 1100, 280]                                                         # one run over most of the canvas
    inside = [300, 131, 1049]                                                        # a window that begins and ends inside a chunk
    tail = [1479, 1]                                                                 # the last pixel alone
    partners = [dense, sparse, block, inside, tail, alternating(200, 301, N)]
    for r in rows + partners:
        assert sum(r) == N
    assert max(len(r) for r in rows) > 1024
    for crowd in (0, 1):
        run_units(ops, dev, rows, partners, [(len(rows), len(partners))], [crowd] * len(partners), [(H, W)], bits=not crowd)
        run_units(ops, dev, partners, rows, [(len(partners), len(rows))], [crowd] * len(rows), [(H, W)])
    # every row against every row: windows that begin and end at every phase of a wave's 64 lanes
    run_units(ops, dev, rows, rows, [(len(rows), len(rows))], [0] * len(rows), [(H, W)])


# ------------------------------------------------------------------------------------------------------- non-canonical counts
def with_zeros(c, rng, times=None):
    """the same stream with zero counts at random places: a pair (0, 0) in front of any count (in front of a ones-run: two
    ones-runs that share a start; at 0: leading zeros), and runs cut in two by a zero count of the other value"""
    c = list(c)
    for _ in range(times or int(rng.integers(1, 5))):
        i = int(rng.integers(0, len(c) + 1))
        if rng.random() < 0.5 or not c:
            c[i:i] = [0, 0]
        else:
            i = min(i, len(c) - 1)
            a = int(rng.integers(0, c[i] + 1))
            c[i:i + 1] = [a, 0, c[i] - a]
    return c


def check_non_canonical(ops, dev):
    rng = np.random.default_rng(43)
    # pinned: ones-runs sharing a start (a zero-pixel run in front of a real one), an adjacent pair of ones-runs, leading
    # and trailing zero counts -- 20 pixels each
    tie = [3, 0, 0, 4, 5, 0, 0, 0, 0, 6, 2]                   # ones: [3,3) [3,7) | [12,12) [12,12) [12,18)
    split = [3, 2, 0, 2, 5, 6, 2]                             # ones: [3,5) [5,7) [12,18): the same pixels
    plain = [3, 4, 5, 6, 2]
    lead = [0, 0, 0, 0, 3, 4, 5, 6, 2, 0, 0]                  # the same pixels behind two empty pairs, an empty pair at the end
    other = [5, 10, 5]
    assert all(sum(r) == 20 for r in (tie, split, plain, lead, other))
    assert all(np.array_equal(stream(r), stream(plain)) for r in (tie, split, lead))
    rows = [tie, split, plain, lead, other]
    for crowd in (0, 1):
        got, _ = run_units(ops, dev, rows, rows, [(5, 5)], [crowd] * 5, want='pixels')
        iou = got.reshape(5, 5)
        assert (iou[:4, :4] == 1.0).all()                     # four spellings of one mask
        assert (iou[:4, 4] == (5 / 10 if crowd else 5 / 15)).all() and (iou[4, :4] == (5 / 10 if crowd else 5 / 15)).all()
    # one row of a pair non-canonical: the literal walk is the reference (module docstring)
    for H, W in ((7, 9), (40, 37)):
        canon = [enc(rng.random((H, W)) < d) for d in (0.05, 0.3, 0.5, 0.9) for _ in range(3)]
        canon += [[0, H * W], [H * W]]
        bent = [with_zeros(c, rng) for c in canon] + [with_zeros(canon[0], rng, 40)]
        for r, s in zip(bent, canon):
            assert np.array_equal(stream(r), stream(s))
        crowd = [int(i % 3 == 0) for i in range(len(canon))]
        run_units(ops, dev, bent, canon, [(len(bent), len(canon))], crowd, [(H, W)], bits=(H == 7))
        run_units(ops, dev, canon, bent, [(len(canon), len(bent))], crowd + [0], [(H, W)], gt_cap=256 if H == 7 else None)
        # both rows non-canonical: the pixel count and the bits route
        run_units(ops, dev, bent, bent, [(len(bent), len(bent))], crowd + [1], [(H, W)], want='pixels', bits=True)
    # the coincidence the literal walk stops at: both rows hold a zero count at pixel 2; the kernel counts the pixels behind it
    a = [2, 0, 0, 3]
    assert LITERAL_IOU([(a, 1, 5)], [(a, 1, 5)], [0])[0, 0] == 0.0
    got, _ = run_units(ops, dev, [a], [a], [(1, 1)], [0], [(1, 5)], want='pixels', bits=True)
    assert got[0] == 1.0


# --------------------------------------------------------------------------------------------------------- crowd ground truths
def check_crowd(ops, dev):
    H, W = 7, 9
    d = np.zeros((H, W), bool)
    d[1:5, 1:5] = True                                        # 16 pixels
    g = np.zeros((H, W), bool)
    g[3:7, 3:9] = True                                        # 24 pixels, 4 of them in d
    got, _ = run_units(ops, dev, [enc(d)], [enc(g), enc(g)], [(1, 2)], [1, 0], [(H, W)], bits=True)
    assert got.tolist() == [4 / 16, 4 / 36]


# ------------------------------------------------------------------------------------------------------------- unit geometry
def check_unit_geometry(ops, dev):
    rng = np.random.default_rng(47)
    canvases = [(1, 1), (1, 9), (9, 1), (7, 9), (40, 37), (1, 1), (7, 9)]
    blocks = [(1, 1), (3, 2), (2, 3), (0, 4), (5, 0), (0, 0), (4, 5)]
    dt_rows, gt_rows, crowd, hws = [], [], [], []
    for (h, w), (a, b) in zip(canvases, blocks):
        hws.append((h, w))
        dt_rows += [enc(rng.random((h, w)) < 0.5) for _ in range(a)]
        gt_rows += [enc(rng.random((h, w)) < 0.5) for _ in range(b)]
        crowd += [int(rng.random() < 0.3) for _ in range(b)]
    dt_rows[0], gt_rows[0] = [0, 1], [0, 1]                                          # the 1 x 1 unit: one pixel, set in both
    got, info = run_units(ops, dev, dt_rows, gt_rows, blocks, crowd, hws, bits=True)
    assert got[0] == 1.0 and info['pairs'] == sum(a * b for a, b in blocks)
    # capacities of their own: the dt table exactly as wide as its widest row, the gt table far wider than any row needs
    widest = max(len(r) for r in dt_rows)
    got2, _ = run_units(ops, dev, dt_rows, gt_rows, blocks, crowd, hws, dt_cap=widest, gt_cap=4096)
    assert np.array_equal(got, got2)
    # nothing to do
    none = ops.coco_units(*units_of([(0, 0), (0, 3)])[:5], np.zeros(2, np.int64), dev)
    gc, gn = rows_from_counts(gt_rows[:3], dev)
    out = ops.coco_iou_runs(none, 0, (gc[:0], gn[:0]), (gc, gn), torch.zeros((4,), dtype=torch.uint8, device=dev))
    assert out.shape == (0,) and out.dtype == torch.float64
    ws, area, ext = ops.run_prefix(gc[:0], gn[:0])
    assert ws.shape == (0, gc.shape[1]) and area.shape == (0,) and ext.shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------- seeded random pairs
def random_pairs(seed=53, count=300):
    rng = np.random.default_rng(seed)
    dens = (0.0, 0.05, 0.3, 0.5, 0.9, 1.0)
    dt_rows, gt_rows, hws, crowd = [], [], [], []
    for i in range(count):
        h, w = (1, 1) if i == 0 else (64, 64) if i == 1 else (int(rng.integers(1, 65)), int(rng.integers(1, 65)))
        d = enc(rng.random((h, w)) < dens[int(rng.integers(6))])
        g = enc(rng.random((h, w)) < dens[int(rng.integers(6))])
        if i % 3 == 0:                                       # a third of the rows non-canonical, one row of a pair at most
            d = with_zeros(d, rng)
        elif i % 3 == 1:
            g = with_zeros(g, rng)
        dt_rows.append(d)
        gt_rows.append(g)
        hws.append((h, w))
        crowd.append(int(rng.random() < 0.25))
    return dt_rows, gt_rows, hws, crowd


def check_random_pairs(ops, dev):
    dt_rows, gt_rows, hws, crowd = random_pairs()
    got, info = run_units(ops, dev, dt_rows, gt_rows, [(1, 1)] * len(hws), crowd, hws, bits=True)
    assert (got > 0).sum() > 100 and (got == 0).sum() > 30 and info['survivors'] < info['pairs']


# ------------------------------------------------------------------------------------------------------------------ 64-bit union
def check_union_64bit(ops, dev):
    """46 340 x 46 340 = 2 147 395 600 pixels fit COCO's counts; area_d + area_g does not fit 32 bits"""
    side = 46340
    N = side * side
    d = [10, 2147395000 - 10, N - 2147395000]
    g = [2000000000, N - 2000000000]
    assert N < 2 ** 31 and sum(d) == N and sum(g) == N and d[1] + g[1] > 2 ** 31
    got, info = run_units(ops, dev, [d], [g, g], [(1, 2)], [0, 1], [(side, side)])
    assert got[0] == 147395000 / 2147395590 and got[1] == 147395000 / 2147394990
    assert info == dict(pairs=2, survivors=2)


# ---------------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(ops, dev, pytest):
    from rsprompter_amd import _lib
    lib = _lib.load()
    EINVAL, OK = ops.CONST['RSP_EINVAL'], ops.CONST['RSP_OK']
    rows = [[3, 4, 5], [12]]
    c, n = rows_from_counts(rows, dev)
    ws, area, ext = ops.run_prefix(c, n)
    p = lambda t: t.data_ptr()                                                       # noqa: E731
    assert lib.rsp_run_prefix_workspace_bytes(2, 3) == 24 and lib.rsp_run_prefix_workspace_bytes(-1, 3) == 0
    assert lib.rsp_run_prefix_workspace_bytes(2, 0) == 0
    assert lib.rsp_run_prefix(p(c), p(n), 2, 0, p(ws), p(area), p(ext), None) == EINVAL           # cap < 1
    assert lib.rsp_run_prefix(p(c), p(n), -1, 3, p(ws), p(area), p(ext), None) == EINVAL          # a negative size
    assert lib.rsp_run_prefix(None, p(n), 2, 3, p(ws), p(area), p(ext), None) == EINVAL           # null arrays
    assert lib.rsp_run_prefix(p(c), p(n), 2, 3, None, p(area), p(ext), None) == EINVAL
    assert lib.rsp_run_prefix(p(c), p(n), 2, 3, p(ws), None, p(ext), None) == EINVAL
    assert lib.rsp_run_prefix(None, None, 0, 3, None, None, None, None) == OK                     # k == 0: nothing to do
    units = ops.coco_units(*units_of([(2, 2)])[:5], np.zeros(1, np.int64), dev)
    up = ops._units_ptr(units)
    alive = torch.full((4,), -1, dtype=torch.int64, device=dev)
    iou = torch.zeros((4,), dtype=torch.float64, device=dev)
    crowd = torch.zeros((2,), dtype=torch.uint8, device=dev)
    assert lib.rsp_coco_iou_runs_filter(up, -1, 4, p(ext), 2, p(ext), 2, p(alive), p(iou), None) == EINVAL
    assert lib.rsp_coco_iou_runs_filter(up, 1, -4, p(ext), 2, p(ext), 2, p(alive), p(iou), None) == EINVAL
    assert lib.rsp_coco_iou_runs_filter(up, 1, 4, p(ext), -2, p(ext), 2, p(alive), p(iou), None) == EINVAL
    assert lib.rsp_coco_iou_runs_filter(None, 1, 4, p(ext), 2, p(ext), 2, p(alive), p(iou), None) == EINVAL
    assert lib.rsp_coco_iou_runs_filter(up, 1, 4, None, 2, p(ext), 2, p(alive), p(iou), None) == EINVAL
    assert lib.rsp_coco_iou_runs_filter(up, 1, 4, p(ext), 2, p(ext), 2, None, p(iou), None) == EINVAL
    assert lib.rsp_coco_iou_runs_filter(up, 1, 4, p(ext), 2, p(ext), 2, p(alive), None, None) == EINVAL
    assert lib.rsp_coco_iou_runs_filter(None, 0, 4, None, 2, None, 2, None, None, None) == OK     # n_units == 0
    slots = torch.arange(4, dtype=torch.int64, device=dev)

    def walk(slots_p=p(slots), n_slots=4, n_iou=4, alive_p=p(alive), dc=p(c), k=2, cap=3, gt_cap=3, iou_p=p(iou), crowd_p=p(crowd)):
        return lib.rsp_coco_iou_runs(slots_p, n_slots, n_iou, alive_p, dc, p(n), k, cap, p(ws), p(area), p(ext),
                                     p(c), p(n), 2, gt_cap, p(ws), p(area), p(ext), crowd_p, iou_p, None)
    assert walk(cap=0) == EINVAL and walk(gt_cap=0) == EINVAL and walk(n_slots=-1) == EINVAL and walk(k=-2) == EINVAL
    assert walk(n_iou=-1) == EINVAL
    assert walk(slots_p=None) == EINVAL and walk(alive_p=None) == EINVAL and walk(dc=None) == EINVAL
    assert walk(iou_p=None) == EINVAL and walk(crowd_p=None) == EINVAL
    assert walk(slots_p=None, n_slots=0) == OK and walk(dc=None, k=0) == OK
    assert walk() == OK                                        # every slot dead (-1): walked over, nothing written
    assert iou.cpu().tolist() == [0.0] * 4
    # the wrappers: a row that did not fit its producer
    bad = n.clone()
    bad[1] = -5
    with pytest.raises(ValueError, match='did not fit'):
        ops.run_prefix(c, bad)
    with pytest.raises(ValueError, match='did not fit'):
        ops.coco_iou_runs(units, 4, (c, bad), (c, n), crowd)
    with pytest.raises(ValueError, match='did not fit'):
        ops.coco_iou_runs(units, 4, (c, n), (c, bad), crowd)
    with pytest.raises(ValueError, match='int32'):
        ops.run_prefix(c.to(torch.int64), n)
    # n > cap is read up to cap, as everywhere else
    wide = n.clone()
    wide[0] = 7
    _, a2, e2 = ops.run_prefix(c, wide)
    assert a2.cpu().tolist() == [4, 0] and e2.cpu().tolist() == [[3, 7], [0, 0]]


# ================================================================================================== metric and API (host + device)
def _stats_and_tables(m):
    return ({t: m.eval_results[t].stats.copy() for t in ('bbox', 'segm')},
            {k: m.eval_results['segm'].tables[k] for k in ('dtm', 'dtig', 'npig')})


def _run_metric(evaluation, dev, classes, images, per_img, prefix, ann_file=None, samples_gt=None, **kw):
    """CocoMetric through process / evaluate; per_img: {img_id: [(xyxy, score, label, rle dict)]} -> the metric"""
    m = evaluation.CocoMetric(ann_file=ann_file, metric=['bbox', 'segm'], device=str(dev), outfile_prefix=prefix, **kw)
    m.dataset_meta = dict(classes=classes)
    samples = []
    for im in images:
        p = per_img.get(im['id'], [])
        pi = dict(bboxes=torch.tensor([q[0] for q in p], dtype=torch.float32).view(-1, 4),
                  scores=torch.tensor([q[1] for q in p], dtype=torch.float32),
                  labels=torch.tensor([q[2] for q in p], dtype=torch.int64), masks=[q[3] for q in p])
        s = dict(pred_instances=pi, img_id=im['id'], ori_shape=(im['height'], im['width']))
        if samples_gt is not None:
            s['gt_instances'] = samples_gt[im['id']]
        samples.append(s)
    m.process(None, samples)
    m.evaluate(len(samples))
    return m


def _oracle_stats(m, prefix):
    """the restatement on the metric's own ground truth and its written result files (tests/test_gpu_coco_eval.py)"""
    return {t: ref.coco_stats(m.coco_gt, json.load(open(f'{prefix}.{t}.json')), t)[0] for t in ('bbox', 'segm')}


def _check_domains(evaluation, dev, classes, images, per_img, tmp_path, name, **kw):
    """'bits' and 'runs' through the metric: all 24 stats and the tables equal, and equal to coco_stats"""
    got = {}
    for domain in ('bits', 'runs'):
        prefix = str(tmp_path / f'{name}_{domain}' / 'r')
        m = _run_metric(evaluation, dev, classes, images, per_img, prefix, iou_domain=domain, **kw)
        assert m.iou_domain == domain and m.timings['segm']['iou_domain'] == domain
        got[domain] = _stats_and_tables(m) + (m, prefix)
    for t in ('bbox', 'segm'):
        assert np.array_equal(got['bits'][0][t], got['runs'][0][t]), (name, t, got['bits'][0][t], got['runs'][0][t])
    for k in ('dtm', 'dtig', 'npig'):
        assert np.array_equal(got['bits'][1][k], got['runs'][1][k]), (name, k)
    want = _oracle_stats(got['runs'][2], got['runs'][3])
    for t in ('bbox', 'segm'):
        assert np.array_equal(got['runs'][0][t], want[t]), (name, t, got['runs'][0][t], want[t])
    tm = got['runs'][2].timings['segm']
    assert 0 < tm['survivors'] <= tm['pairs']
    return got['runs'][0], tm


def nwpu_detections():
    """the committed NWPU subset with detections made as tests/_poly_raster_cases.py makes them (jittered boxes, the ground
    truth's own masks), plus for every annotation its mask moved by three columns at a lower score: IoUs between 0 and 1"""
    import _coco_cases as cc
    import _large_image_ref as lref
    import _poly_raster_cases as prc
    segms, sizes, want = prc.nwpu()
    d = prc._NWPU['json']
    hw = {im['id']: (im['height'], im['width']) for im in d['images']}
    rng = np.random.default_rng(26)
    classes, cat_ids = [c['name'] for c in d['categories']], [c['id'] for c in d['categories']]
    per_img, samples_gt = {}, {im['id']: dict(bboxes=[], labels=[], masks=[]) for im in d['images']}
    for a, c in zip(d['annotations'], want):
        h, w = hw[a['image_id']]
        x, y, bw, bh = a['bbox']
        jit = rng.uniform(-3, 3, 4)
        box = [x + jit[0], y + jit[1], x + bw + jit[2], y + bh + jit[3]]
        lab = cat_ids.index(a['category_id'])
        rle = dict(size=[h, w], counts=ref.rle_to_string(c))
        moved = np.roll(ref.rle_decode(c, h, w), 3, axis=1)
        per_img.setdefault(a['image_id'], []).append((box, float(rng.uniform(0.5, 1.0)), lab, rle))
        per_img[a['image_id']].append(([v + 3 for v in box], float(rng.uniform(0.1, 0.5)), lab,
                                       dict(size=[h, w], counts=ref.rle_to_string(lref.rle_counts_np(moved)))))
        g = samples_gt[a['image_id']]
        g['bboxes'].append([x, y, x + bw, y + bh])
        g['labels'].append(lab)
        g['masks'].append(rle)
    for g in samples_gt.values():
        g['bboxes'] = np.asarray(g['bboxes'], np.float32).reshape(-1, 4)
        g['labels'] = np.asarray(g['labels'], np.int64)
    return cc.FIXTURE_JSON, classes, d['images'], per_img, samples_gt


def check_metric_nwpu(evaluation, dev, tmp_path):
    ref.use_numpy_forms()
    ann_file, classes, images, per_img, samples_gt = nwpu_detections()
    s_file, _ = _check_domains(evaluation, dev, classes, images, per_img, tmp_path, 'ann_file', ann_file=ann_file)
    s_def, _ = _check_domains(evaluation, dev, classes, images, per_img, tmp_path, 'default', samples_gt=samples_gt)
    assert 0.3 < s_file['segm'][0] < 1.0 and 0.3 < s_def['segm'][0] <= 1.0


def scene_set(apis, dev, sizes, seed=61):
    """Two scenes of different sizes, two categories, 30 ground-truth ellipses each as 32-vertex polygons and one crowd
    ground truth as uncompressed RLE; 45 detections each (jittered ground truths and spurious ellipses) rasterised with
    apis.polygons_to_masks -> (gt json, classes, per_img)"""
    rng = np.random.default_rng(seed)
    th = np.linspace(0, 2 * np.pi, 32, endpoint=False)

    def ellipse(h, w, scale):
        cx, cy = rng.uniform(0.1 * w, 0.9 * w), rng.uniform(0.1 * h, 0.9 * h)
        rx, ry = rng.uniform(0.02, 0.08) * scale, rng.uniform(0.02, 0.08) * scale
        return cx, cy, rx, ry

    def ring(cx, cy, rx, ry, h, w):
        xy = np.stack([np.clip(cx + rx * np.cos(th), 0, w), np.clip(cy + ry * np.sin(th), 0, h)], 1)
        return np.round(xy, 2).reshape(-1).tolist()
    images, anns, per_img = [], [], {}
    for img_id, (h, w) in enumerate(sizes, start=1):
        images.append(dict(id=img_id, height=h, width=w, file_name=f'scene{img_id}.png'))
        scale = min(h, w)
        gts = [ellipse(h, w, scale) for _ in range(30)]
        for j, e in enumerate(gts):
            poly = ring(*e, h, w)
            xs, ys = poly[0::2], poly[1::2]
            bb = [min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys)]
            anns.append(dict(id=len(anns) + 1, image_id=img_id, category_id=1 + j % 2, segmentation=[poly], bbox=bb,
                             area=float(np.pi * e[2] * e[3]), iscrowd=0))
        x0, x1 = int(0.3 * w), int(0.6 * w)                                           # the crowd region: whole columns
        anns.append(dict(id=len(anns) + 1, image_id=img_id, category_id=1, iscrowd=1, bbox=[x0, 0, x1 - x0, h],
                         area=float((x1 - x0) * h), segmentation=dict(size=[h, w], counts=[x0 * h, (x1 - x0) * h, (w - x1) * h])))
        dets, polys = [], []
        for j in range(45):
            if j < 32:
                cx, cy, rx, ry = gts[j % 30]
                e = (cx + rng.normal(0, 0.3 * rx), cy + rng.normal(0, 0.3 * ry), rx * rng.uniform(0.8, 1.2), ry * rng.uniform(0.8, 1.2))
                lab = (j % 30) % 2 if rng.random() < 0.9 else 1 - (j % 30) % 2
            else:
                e, lab = ellipse(h, w, scale), int(rng.integers(2))
            poly = ring(*e, h, w)
            xs, ys = poly[0::2], poly[1::2]
            polys.append([poly])
            dets.append(([min(xs), min(ys), max(xs), max(ys)], float(np.round(rng.uniform(0.05, 1.0), 2)), lab))
        rles = apis.polygons_to_masks(polys, (h, w), form='rle', device=dev)
        per_img[img_id] = [d + (r,) for d, r in zip(dets, rles)]
    gt = dict(images=images, annotations=anns, categories=[dict(id=1, name='a'), dict(id=2, name='b')])
    return gt, ['a', 'b'], per_img


def check_metric_scenes(evaluation, apis, dev, tmp_path, sizes, monkeypatch, memory=None):
    """the scene set through 'bits' and 'runs', against coco_stats; 'auto' on both sides of the budget; apis.mask_iou on the
    scene-sized RLE (memory: a callable -> peak bytes since its reset, on the device tier)"""
    ref.use_numpy_forms()
    monkeypatch.setattr(ref, 'rle_iou', LITERAL_IOU)              # the literal walk skips the pairs rleIou's bbIou skips
    gt, classes, per_img = scene_set(apis, dev, sizes)
    ann = tmp_path / 'scenes.json'
    ann.write_text(json.dumps(gt))
    stats, tm = _check_domains(evaluation, dev, classes, gt['images'], per_img, tmp_path, 'scenes', ann_file=str(ann))
    assert 0.05 < stats['segm'][0] < 1.0 and tm['survivors'] < tm['pairs']
    assert evaluation.BITS_BUDGET_BYTES == 1 << 30
    for budget, route in ((1, 'runs'), (1 << 40, 'bits')):
        monkeypatch.setattr(evaluation, 'BITS_BUDGET_BYTES', budget)
        m = _run_metric(evaluation, dev, classes, gt['images'], per_img, str(tmp_path / f'auto_{route}' / 'r'),
                        ann_file=str(ann), iou_domain='auto')
        assert m.timings['segm']['iou_domain'] == route
        for t in ('bbox', 'segm'):
            assert np.array_equal(m.eval_results[t].stats, stats[t]), (route, t)
    # mask_iou on the first scene: every detection against every ground truth of the metric's own RLE
    m_gt = m._gt_with_rles(m.coco_gt, dev)
    h, w = sizes[0]
    g = [a for a in m_gt['annotations'] if a['image_id'] == 1]
    d_rles, g_rles = [q[3] for q in per_img[1]], [a['segmentation'] for a in g]
    crowd = [bool(a['iscrowd']) for a in g]
    if memory is not None:
        memory(reset=True)
    iou = apis.mask_iou(d_rles, g_rles, crowd, device=dev)
    if memory is not None:
        peak, plane = memory(), h * w // 8
        print(f'mask_iou on {len(d_rles)} x {len(g_rles)} masks of {h} x {w}: peak {peak} bytes, one bit plane {plane} bytes')
        assert peak < (len(d_rles) + len(g_rles)) * plane // 8                    # far below one bit plane per mask
    assert iou.dtype == torch.float64 and iou.shape == (len(d_rles), len(g_rles)) and iou.device.type == torch.device(dev).type
    want = LITERAL_IOU([ref.segm_to_cnts(r, h, w) for r in d_rles], [ref.segm_to_cnts(r, h, w) for r in g_rles], crowd)
    assert np.array_equal(iou.cpu().numpy(), want) and (want > 0).sum() > 30 and any(crowd)


def check_metric_refusals(evaluation, pytest):
    with pytest.raises(ValueError, match='iou_domain'):
        evaluation.CocoMetric(iou_domain='rle')
    with pytest.raises(ValueError, match='iou_domain'):
        evaluation.device_evaluate(dict(images=[], annotations=[]), [], 'segm', [], [], [0.5], [1, 10, 100], 'cpu', iou_domain='x')
    assert evaluation.CocoMetric().iou_domain == 'bits' and evaluation.IOU_DOMAINS == ('bits', 'runs', 'auto')


def check_mask_iou(apis, dev, pytest):
    import _coco_cases as cc
    import _large_image_ref as lref
    rng = np.random.default_rng(67)
    for h, w in ((20, 36), (64, 50)):
        masks = [cc.random_mask(rng, h, w, k) for k in ('blob', 'blob', 'noise', 'full', 'empty', 'pixel', 'blob')]
        cnts = [[int(v) for v in lref.rle_counts_np(m.astype(bool))] for m in masks]
        packed = [dict(size=[h, w], counts=ref.rle_to_string(c)) for c in cnts]
        plain = [dict(size=[h, w], counts=list(c)) for c in cnts]
        text = [dict(size=[h, w], counts=ref.rle_to_string(c).decode()) for c in cnts]
        mixed = [packed[0], plain[1], text[2], plain[3], packed[4], plain[5], text[6]]
        crowd = [True, False, False, True, False, False, True]
        want = LITERAL_IOU([(c, h, w) for c in cnts[:5]], [(c, h, w) for c in cnts], crowd)
        for dt, gt in ((packed[:5], packed), (plain[:5], plain), (mixed[:5], mixed), (mixed[:5], packed)):
            got = apis.mask_iou(dt, gt, crowd, device=dev)
            assert got.dtype == torch.float64 and got.shape == (5, 7) and np.array_equal(got.cpu().numpy(), want)
        t = torch.from_numpy(np.stack(masks)).to(dev).bool()
        assert np.array_equal(apis.mask_iou(t[:5], t, crowd).cpu().numpy(), want)
        assert np.array_equal(apis.mask_iou(t[:5], mixed, crowd, device=dev).cpu().numpy(), want)
        none = LITERAL_IOU([(c, h, w) for c in cnts[:5]], [(c, h, w) for c in cnts], [False] * 7)
        assert np.array_equal(apis.mask_iou(packed[:5], packed, device=dev).cpu().numpy(), none) and not np.array_equal(none, want)
        assert apis.mask_iou([], packed, device=dev).shape == (0, 7) and apis.mask_iou(packed, [], device=dev).shape == (7, 0)
        assert apis.mask_iou(t[:0], t).shape == (0, 7)
    # sizes of their own: one table, the rows in the order of the list
    a, b = dict(size=[2, 3], counts=[1, 2, 3]), dict(size=[4, 1], counts=ref.rle_to_string([0, 3, 1]))
    from rsprompter_amd import rle
    counts, n, sizes, _ = rle.masks_to_runs([a, b, a], dev, 'mask_iou', one_size=False)
    assert sizes == [(2, 3), (4, 1), (2, 3)] and n.cpu().tolist() == [3, 3, 3]
    assert counts.cpu()[:, :3].tolist() == [[1, 2, 3], [0, 3, 1], [1, 2, 3]]
    with pytest.raises(ValueError, match='different sizes'):
        apis.mask_iou([a], [b], device=dev)
    with pytest.raises(ValueError, match='different sizes'):
        apis.mask_iou([a, b], [a], device=dev)
    with pytest.raises(ValueError, match='iscrowd'):
        apis.mask_iou([a], [a, a], [True], device=dev)
    assert apis.mask_iou([a], [a], device=dev).cpu().tolist() == [[1.0]]
