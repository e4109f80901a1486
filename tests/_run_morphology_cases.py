"""Case bodies of the run-domain morphology and Boundary IoU (csrc/run_morphology.hip, ops.rle_erode / rle_boundary,
rle.*_runs, apis.mask_morphology / mask_boundary / boundary_iou, CocoMetric(metric='boundary')), run on the
lane emulator by tests/test_run_morphology_cpu.py and on the device by tests/test_gpu_run_morphology.py.  The oracle is
tests/_run_morphology_ref.py (dense numpy, two forms that must agree); Boundary AP is checked against COCOeval of
tests/_cocoeval_ref.py with computeIoU replaced by min(mask IoU, band IoU).  Every comparison is ==."""
import json
import os
import sys

import numpy as np
import torch
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _coco_iou_runs_cases as cic  # noqa: E402
import _cocoeval_ref as ref  # noqa: E402
import _run_morphology_ref as mref  # noqa: E402
import _seam_merge_cases as seam_cases  # noqa: E402

rows_from_counts = seam_cases.rows_from_counts
rows_from_masks = seam_cases.rows_from_masks
OK, EINVAL = 0, -1


# -------------------------------------------------------------------------------------------------------------- helpers
def decode(counts, n_host, H, W):
    """a run table -> dense masks, after checking that every row is canonical COCO: only count 0 may be zero, sum H * W"""
    counts = counts.cpu().numpy()
    out = []
    for i, m in enumerate(n_host.tolist()):
        c = counts[i, :m].tolist()
        assert m >= 1 and sum(c) == H * W and all(v > 0 for v in c[1:]) and c[0] >= 0, (i, c[:12])
        out.append(ref.rle_decode(c, H, W).astype(bool))
    return out


def erode_table(ops, counts, n, H, W, r, border=0, cap=None):
    c, m, n_host, cap2 = ops.rle_erode(counts, n, H, W, r, border, cap)
    assert c.dtype == torch.int32 and m.dtype == torch.int32 and tuple(c.shape) == (n.shape[0], cap2)
    assert np.array_equal(m.cpu().numpy(), n_host.numpy())
    return decode(c, n_host, H, W)


def boundary_table(ops, counts, n, H, W, r, cap=None):
    c, m, n_host, cap2 = ops.rle_boundary(counts, n, H, W, r, cap)
    assert tuple(c.shape) == (n.shape[0], cap2) and np.array_equal(m.cpu().numpy(), n_host.numpy())
    return decode(c, n_host, H, W)


def check_masks(ops, dev, masks, r, borders=(0, 1), band=True, what=''):
    """erosion (both borders) and band of dense masks of one size against the oracle"""
    H, W = masks[0].shape
    counts, n = rows_from_masks(masks, dev)
    for b in borders:
        got = erode_table(ops, counts, n, H, W, r, b)
        for i, m in enumerate(masks):
            assert np.array_equal(got[i], mref.erode(m, r, b)), (what, 'erode', i, r, b, H, W)
    if band:
        got = boundary_table(ops, counts, n, H, W, r)
        for i, m in enumerate(masks):
            assert np.array_equal(got[i], mref.boundary(m, r)), (what, 'boundary', i, r, H, W)
            assert got[i].any() == m.any() or r == 0             # the band of a non-empty mask is never empty


def blob(rng, h, w, thr=-0.02):
    return ndi.gaussian_filter(rng.standard_normal((h, w)), 3) > thr


class ReadCounter:
    """counts the calls through which the package's host code reads from `dev`: Tensor.item / nonzero / cpu / tolist (the
    counter of tests/test_gpu_sam_multicrop.py, for tensors of the device under test: the emulator's are CPU tensors)"""

    def __init__(self, dev):
        self.dev = torch.device(dev).type

    def __enter__(self):
        self.n = 0
        self.saved = {k: getattr(torch.Tensor, k) for k in ('item', 'nonzero', 'cpu', 'tolist')}
        for k, fn in self.saved.items():
            def wrap(t, *a, _fn=fn, **kw):
                if t.device.type == self.dev:
                    self.n += 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, wrap)
        return self

    def __exit__(self, *a):
        for k, fn in self.saved.items():
            setattr(torch.Tensor, k, fn)


def check_oracle():
    """the literal form and scipy agree (mref.erode asserts it), and dilation is the complement's erosion with the outside set"""
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (1, 9), (9, 1), (7, 5), (40, 37), (33, 64)):
        for r in (1, 2, 3, 5, 8, 13):
            for m in (np.ones((h, w), bool), rng.random((h, w)) < 0.9, blob(rng, h, w, 0.0), blob(rng, h, w, -0.05)):
                mref.dilate(m, r)
                for b in (0, 1):
                    assert np.array_equal(mref.erode(m, r, b), mref.erode_separable(m, r, b)), (h, w, r, b)
                assert np.array_equal(mref.boundary_cropped(m, r, separable=True), mref.boundary(m, r))
                assert not (mref.boundary(m, r) & ~m).any() and mref.boundary(m, r).any() == m.any()
    assert [mref.radius(s) for s in ((1024, 1024), (512, 512), (8192, 9000))] == [29, 14, 243]


# --------------------------------------------------------------------------------------------------------- hand-checked
def check_hand_checked(ops, dev):
    def one(mask, r, b=0):
        H, W = mask.shape
        counts, n = rows_from_masks([mask], dev)
        got = erode_table(ops, counts, n, H, W, r, b)[0]
        assert np.array_equal(got, mref.erode(mask, r, b))
        return got
    z = lambda h, w: np.zeros((h, w), bool)                                          # noqa: E731
    # one pixel: gone at r = 1; the 1 x 1 canvas keeps it under border 1 only
    m = z(7, 9)
    m[3, 4] = True
    assert not one(m, 1).any() and one(m, 0)[3, 4] and one(m, 0).sum() == 1
    assert not one(np.ones((1, 1), bool), 1, 0).any() and one(np.ones((1, 1), bool), 1, 1).all()
    # the full canvas: r = 1 leaves the interior, r >= ceil(min / 2) nothing
    full = np.ones((7, 9), bool)
    want = z(7, 9)
    want[1:-1, 1:-1] = True
    assert np.array_equal(one(full, 1), want)
    assert one(full, 3).sum() == 3 and not one(full, 4).any() and one(full, 4, 1).all()
    for r in (1, 2, 3):
        # a (2r+1)^2 square away from the border leaves one pixel, a (2r)^2 square none
        m = z(12, 13)
        m[2:2 + 2 * r + 1, 3:3 + 2 * r + 1] = True
        e = one(m, r)
        assert e.sum() == 1 and e[2 + r, 3 + r]
        m = z(12, 13)
        m[2:2 + 2 * r, 3:3 + 2 * r] = True
        assert not one(m, r).any()
        # the same square in a corner: border 0 leaves its centre as anywhere, border 1 keeps the (r + 1)^2 corner of it
        m = z(12, 13)
        m[:2 * r + 1, :2 * r + 1] = True
        e = one(m, r, 0)
        assert e.sum() == 1 and e[r, r]
        e = one(m, r, 1)
        assert e.sum() == (r + 1) ** 2 and e[:r + 1, :r + 1].all()
        m = z(12, 13)
        m[-(2 * r + 1):, -(2 * r + 1):] = True
        e = one(m, r, 1)
        assert e.sum() == (r + 1) ** 2 and e[-(r + 1):, -(r + 1):].all()
        # a one-pixel hole removes its (2r+1)^2 neighbourhood
        m = np.ones((15, 16), bool)
        m[7, 8] = False
        e = one(m, r, 1)
        assert (~e).sum() == (2 * r + 1) ** 2 and not e[7 - r:8 + r, 8 - r:9 + r].any()
    # a ones-run crossing several column ends: stream [5, 40) of a 7-row canvas = part of column 0, columns 1..4, part of 5
    flat = np.zeros(7 * 9, bool)
    flat[5:40] = True
    m = flat.reshape(9, 7).T
    assert cic.enc(m) == [5, 35, 23]
    e = one(m, 1)
    want = z(7, 9)
    want[1:6, 2:4] = True                                                            # columns 1..4 are full ...
    want[1:4, 4] = True                                                              # ... and column 5 holds rows 0..4
    assert np.array_equal(e, want)
    one(m, 1, 1), one(m, 2, 0), one(m, 2, 1)
    # canvases of 1 x 9 and 9 x 1
    for shape in ((1, 9), (9, 1)):
        m = np.ones(shape, bool)
        assert not one(m, 1, 0).any() and one(m, 1, 1).all()
        m = m.copy()
        m.reshape(-1)[4] = False
        e = one(m, 1, 1).reshape(-1)
        assert e.tolist() == [True, True, True, False, False, False, True, True, True]
    # W < 2r + 1: empty under border 0, the full mask stays full under border 1
    full = np.ones((20, 4), bool)
    assert not one(full, 2, 0).any() and one(full, 2, 1).all() and one(full, 1, 0).sum() == 18 * 2
    # r = 0 is the identity; r far beyond the canvas equals r = max(H, W)
    rng = np.random.default_rng(5)
    m = rng.random((9, 11)) < 0.7
    assert np.array_equal(one(m, 0), m) and np.array_equal(one(m, 0, 1), m)
    for b in (0, 1):
        assert np.array_equal(one(m, 10 ** 6, b), one(m, 11, b))
    assert one(np.ones((9, 11), bool), 10 ** 6, 1).all()
    # the empty row, the empty mask, all ones -- in one table
    counts, n = rows_from_counts([None, [99], [0, 99]], dev)
    for b in (0, 1):
        got = erode_table(ops, counts, n, 9, 11, 2, b)
        assert not got[0].any() and not got[1].any()
        assert got[2].all() if b else (got[2].sum() == 5 * 7 and got[2][2:7, 2:9].all())
    got = boundary_table(ops, counts, n, 9, 11, 2)
    assert not got[0].any() and not got[1].any() and got[2].sum() == 99 - 35 and not got[2][2:7, 2:9].any()
    # the band: mask pixels at the image border belong to it
    m = z(10, 10)
    m[:6, :6] = True
    counts, n = rows_from_masks([m], dev)
    band = boundary_table(ops, counts, n, 10, 10, 2)[0]
    assert np.array_equal(band, mref.boundary(m, 2)) and band[0, 0] and band[:6, 0].all() and not band[2:4, 2:4].any()


# ------------------------------------------------------------------------------------------- every digit pattern of 2r + 1
RADII = (1, 2, 3, 4, 7, 8, 15, 16, 31)


def check_digit_patterns(ops, dev):
    rng = np.random.default_rng(20261020)
    m = blob(rng, 64, 64)
    big = np.ones((64, 64), bool)                                # three pixels survive r = 31 under border 0
    big[0, 0] = False
    assert mref.erode(big, 31, 0).sum() == 3 and m.any() and not m.all()
    for r in RADII:
        check_masks(ops, dev, [m, ~m, big], r, what=f'digits r={r}')


# ------------------------------------------------------------------------------------------------- list and wave boundaries
PIECES = (0, 1, 63, 64, 65, 129, 130)


def check_list_boundaries(ops, dev):
    """columns of 0 .. 130 pieces (alternating rows) beside columns of one long piece, both ways round"""
    H, W = 260, 12
    comb = lambda p: np.isin(np.arange(H), 2 * np.arange(p))                         # noqa: E731  p one-pixel pieces
    thick = lambda p: np.isin(np.arange(H) % 4, (0, 1, 2)) & (np.arange(H) < 4 * p)   # noqa: E731  p three-pixel pieces
    masks = []
    for make in (comb, thick):
        for swap in (0, 1):
            m = np.zeros((H, W), bool)
            for j, p in enumerate(PIECES):
                x = j + 2 if not swap else W - 3 - j
                m[:, x] = make(min(p, H // 4 if make is thick else p))
            long_cols = [0, 1, W - 2, W - 1] if not swap else [0, W - 1]
            for x in long_cols:
                m[3:H - 2, x] = True
            masks.append(m)
    # pieces beside one long piece in every column pair: long pieces in the even columns
    m = np.zeros((H, W), bool)
    for j, p in enumerate(PIECES[:6]):
        m[:, 2 * j] = True
        m[:, 2 * j + 1] = thick(min(p, 65))
    masks += [m, ~m, ~masks[0], ~masks[2]]
    for r in (1, 2):
        check_masks(ops, dev, masks, r, what=f'lists r={r}')


# ------------------------------------------------------------------------------------------------------- non-canonical counts
def check_non_canonical(ops, dev):
    rng = np.random.default_rng(43)
    tie = [3, 0, 0, 4, 5, 0, 0, 0, 0, 6, 2]
    split = [3, 2, 0, 2, 5, 6, 2]
    plain = [3, 4, 5, 6, 2]
    lead = [0, 0, 0, 0, 3, 4, 5, 6, 2, 0, 0]
    rows = [tie, split, plain, lead]
    for H, W in ((20, 1), (10, 2), (4, 5), (2, 10)):
        counts, n = rows_from_counts(rows, dev)
        dense = cic.stream(plain).reshape(W, H).T
        for r in (0, 1):
            for b in (0, 1):
                got = erode_table(ops, counts, n, H, W, r, b)
                assert all(np.array_equal(g, mref.erode(dense, r, b)) for g in got), (H, W, r, b)
            got = boundary_table(ops, counts, n, H, W, r)
            assert all(np.array_equal(g, mref.boundary(dense, r)) for g in got), (H, W, r)
    for H, W in ((7, 9), (40, 37)):
        canon = [cic.enc(rng.random((H, W)) < d) for d in (0.5, 0.9, 0.97) for _ in range(2)] + [[0, H * W], [H * W]]
        canon += [cic.enc(blob(rng, H, W))]
        bent = [cic.with_zeros(c, rng) for c in canon] + [cic.with_zeros(canon[0], rng, 40)]
        dense = [cic.stream(c).reshape(W, H).T for c in bent]
        counts, n = rows_from_counts(bent, dev)
        for r, b in ((1, 0), (1, 1), (2, 1)):
            got = erode_table(ops, counts, n, H, W, r, b)
            for i, d in enumerate(dense):
                assert np.array_equal(got[i], mref.erode(d, r, b)), (H, W, r, b, i)
        got = boundary_table(ops, counts, n, H, W, 1)
        for i, d in enumerate(dense):
            assert np.array_equal(got[i], mref.boundary(d, 1)), (H, W, i)


# -------------------------------------------------------------------------------------------------------------- seeded random
def random_masks(seed=20261020, count=300):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        h, w, r = int(rng.integers(8, 65)), int(rng.integers(8, 65)), int(rng.integers(1, 5))
        out.append((blob(rng, h, w), r))
    return out


def check_random(ops, apis, dev):
    """300 masks, every operation of mask_morphology, in the three mask forms; at most a quarter of the erosions may be
    empty (asserted of the oracle), so the test does not compare empties"""
    cases = random_masks()
    want = [{op: fn(m, r) for op, fn in mref.OPS.items()} for m, r in cases]
    assert sum(1 for w in want if w['erode'].any()) >= 225 and all(w['boundary'].any() for w in want)
    groups = {}
    for i, (m, r) in enumerate(cases):
        groups.setdefault((m.shape, r), []).append(i)
    for j, ((shape, r), idx) in enumerate(sorted(groups.items())):
        H, W = shape
        masks = [cases[i][0] for i in idx]
        form = j % 3
        if form == 0:
            arg = torch.from_numpy(np.stack(masks)).to(dev)
        elif form == 1:
            arg = [dict(size=[H, W], counts=ref.rle_to_string(cic.enc(m))) for m in masks]
        else:
            arg = [dict(size=[H, W], counts=cic.enc(m)) for m in masks]
        for op in apis.MORPHOLOGY_OPS:
            got = apis.mask_morphology(arg, op, r, device=dev)
            if form == 0:
                assert got.dtype == torch.bool and tuple(got.shape) == (len(idx), H, W)
                dense = list(got.cpu().numpy())
            else:
                assert all(g['size'] == [H, W] and isinstance(g['counts'], bytes if form == 1 else list) for g in got)
                dense = [ref.rle_decode(ref.rle_fr_string(g['counts']) if form == 1 else g['counts'], H, W).astype(bool)
                         for g in got]
            for i, d in zip(idx, dense):
                assert np.array_equal(d, want[i][op]), (op, i, shape, r, form)


# ------------------------------------------------------------------------------------------------------------------ protocol
def check_protocol(ops, rle, dev):
    rng = np.random.default_rng(77)
    H, W = 40, 37
    masks = [blob(rng, H, W), rng.random((H, W)) < 0.9, np.ones((H, W), bool), np.zeros((H, W), bool)]
    want_e = [mref.erode(m, 2, 0) for m in masks]
    want_b = [mref.boundary(m, 2) for m in masks]
    counts, n = rows_from_masks(masks, dev)
    # capacities of their own, a table far wider than its rows
    wide, _ = rows_from_masks(masks, dev, cap=4000)
    for c in (counts, wide):
        assert all(np.array_equal(g, w) for g, w in zip(erode_table(ops, c, n, H, W, 2, 0, cap=1024), want_e))
        assert all(np.array_equal(g, w) for g, w in zip(boundary_table(ops, c, n, H, W, 2, cap=777), want_b))
    # a cap too small for the band: the retry grows it (fit_runs), and the number of host reads is the documented one
    need = max(len(cic.enc(w)) for w in want_b)
    assert need > 8
    L = ops.run_morph_levels(2, W)
    assert L == 2 and ops.run_morph_levels(243, 9000) == 8 and ops.run_morph_levels(10 ** 6, 5) == 3
    with ReadCounter(dev) as rc:
        c2, n2, n_host, cap2 = ops.rle_boundary(counts, n, H, W, 2, cap=2)
    assert cap2 == ops.grown_cap(need) and rc.n == 3 + L + 2, (rc.n, cap2, need)
    assert all(np.array_equal(g, w) for g, w in zip(decode(c2, n_host, H, W), want_b))
    with ReadCounter(dev) as rc:
        c3, n3, n_host3, cap3 = ops.rle_erode(counts, n, H, W, 2, 0, cap=4096)
    assert cap3 == 4096 and rc.n == 2 + L + 1, rc.n
    with ReadCounter(dev) as rc:
        ops.rle_erode(counts, n, H, W, 31, 1, cap=4096)
    assert rc.n == 2 + ops.run_morph_levels(31, W) + 1 == 2 + 5 + 1, rc.n
    # n > cap is read up to cap: the row cut after `cut` counts describes a shorter stream; what it holds is eroded
    row = cic.enc(masks[0])
    cut = 7
    c_cut, n_cut = rows_from_counts([row[:cut]], dev)
    n_cut[0] = len(row)
    short = np.zeros(H * W, bool)
    short[:sum(row[:cut])] = cic.stream(row[:cut])
    got = erode_table(ops, c_cut, n_cut, H, W, 1, 0)[0]
    assert np.array_equal(got, mref.erode(short.reshape(W, H).T, 1, 0))
    # a second launch gives the same bits
    again = ops.rle_erode(counts, n, H, W, 2, 0, cap=4096)
    assert torch.equal(again[1], n3) and all(torch.equal(again[0][i, :m], c3[i, :m]) for i, m in enumerate(n_host3.tolist()))
    again = ops.rle_boundary(counts, n, H, W, 2, cap=cap2)
    assert torch.equal(again[1], n2) and all(torch.equal(again[0][i, :m], c2[i, :m]) for i, m in enumerate(n_host.tolist()))
    # k = 0
    c0, n0 = counts[:0], n[:0]
    for out in (ops.rle_erode(c0, n0, H, W, 2), ops.rle_boundary(c0, n0, H, W, 2)):
        assert out[0].shape[0] == 0 and out[1].shape[0] == 0 and out[2].shape[0] == 0
    # the derived operations and the radius
    for fn, name in ((rle.dilate_runs, 'dilate'), (rle.open_runs, 'open'), (rle.close_runs, 'close'), (rle.boundary_runs, 'boundary')):
        c, m, n_host, _ = fn(counts, n, (H, W), 2)
        assert all(np.array_equal(g, mref.OPS[name](w, 2)) for g, w in zip(decode(c, n_host, H, W), masks)), name
    ce, ne = rows_from_counts([None, cic.enc(masks[0])], dev)
    c, m, n_host, _ = rle.dilate_runs(ce, ne, (H, W), 1)
    got = decode(c, n_host, H, W)
    assert not got[0].any() and np.array_equal(got[1], mref.dilate(masks[0], 1))
    assert [rle.boundary_radius(s) for s in ((1024, 1024), (512, 512), (8192, 9000), (3, 3))] == [29, 14, 243, 1]
    assert rle.boundary_radius((512, 512), 0.05) == 36 == mref.radius((512, 512), 0.05)


def check_refusals(ops, rle, dev, pytest):
    from rsprompter_amd import _lib
    lib = _lib.load()
    counts, n = rows_from_counts([[3, 4, 5]], dev)
    for bad in (-1, 1.5, True, None):
        with pytest.raises((ValueError, TypeError)):
            ops.rle_erode(counts, n, 3, 4, bad)
    for border in (2, -1):
        with pytest.raises(ValueError, match='border'):
            ops.rle_erode(counts, n, 3, 4, 1, border)
    with pytest.raises(ValueError, match='32-bit'):
        ops.rle_erode(counts, n, 65536, 32768, 1)
    with pytest.raises(ValueError, match='32-bit'):
        ops.rle_boundary(counts, n, 46341, 46341, 1)
    with pytest.raises(ValueError, match='expected counts'):
        ops.rle_erode(counts.to(torch.int64), n, 3, 4, 1)
    for bad in (0, -0.02, float('inf'), float('nan'), True):
        with pytest.raises(ValueError, match='dilation_ratio'):
            rle.boundary_radius((10, 10), bad)
    # the entry points themselves
    p = counts.data_ptr()
    pieces = lambda *a: lib.rsp_run_morph_pieces_count(*a, 0)                        # noqa: E731
    assert pieces(p, p, 1, 4, 3, 4, 1, 0, 0, p) == OK
    assert pieces(p, p, 0, 4, 3, 4, 1, 0, 0, 0) == OK                               # k == 0: a no-op
    assert pieces(p, p, 1, 4, 65536, 32768, 1, 0, 0, p) == EINVAL                   # H * W >= 2^31
    assert pieces(p, p, 1, 0, 3, 4, 1, 0, 0, p) == EINVAL                           # cap < 1
    assert pieces(p, p, 1, 4, 3, 4, -1, 0, 0, p) == EINVAL                          # a negative radius
    assert pieces(p, p, 1, 4, 3, 4, 1, -1, 0, p) == EINVAL
    assert pieces(p, p, 1, 4, 3, 4, 1, 0, 2, p) == EINVAL                           # a border other than 0 / 1
    assert pieces(0, p, 1, 4, 3, 4, 1, 0, 0, p) == EINVAL and pieces(p, 0, 1, 4, 3, 4, 1, 0, 0, p) == EINVAL
    assert pieces(p, p, 1, 4, 3, 4, 1, 0, 0, 0) == EINVAL
    assert pieces(p, p, 2 ** 20, 4, 3, 2048, 1, 0, 0, p) == EINVAL                  # k * W >= 2^31
    assert lib.rsp_run_morph_pieces(p, p, 0, 4, 3, 4, 1, 0, 0, p, 0, p, p, p, 0) == OK
    assert lib.rsp_run_morph_pieces(p, p, 1, 4, 3, 4, 1, 0, 0, 0, 1, p, p, p, 0) == EINVAL
    assert lib.rsp_run_morph_pieces(p, p, 1, 4, 3, 4, 1, 0, 0, p, -1, p, p, p, 0) == EINVAL
    jc = lambda *a: lib.rsp_run_morph_join_count(*a, 0)                              # noqa: E731
    assert jc(0, p, p, p, 0, 4, p, p, p, 0, 1, 4, 1, 2, 0, 4, p) == OK              # no interval: a no-op
    assert jc(2, p, p, p, 1, 4, p, p, p, 1, 1, 4, 1, 2, 0, 4, p) == EINVAL          # op
    assert jc(0, 0, p, p, 1, 4, p, p, p, 1, 1, 4, 1, 2, 0, 4, p) == EINVAL
    assert jc(0, p, p, p, 1, 4, 0, p, p, 1, 1, 4, 1, 2, 0, 4, p) == EINVAL
    assert jc(0, p, p, p, 1, 4, p, p, p, 1, 1, 4, -1, 2, 0, 4, p) == EINVAL
    assert jc(0, p, p, p, 1, 0, p, p, p, 1, 1, 4, 1, 2, 0, 4, p) == EINVAL
    assert jc(0, p, p, p, 1, 4, p, p, p, 1, 1, 4, 1, 2, 0, 4, 0) == EINVAL
    jw = lambda *a: lib.rsp_run_morph_join(*a, 0)                                    # noqa: E731
    assert jw(0, p, p, p, 0, 4, p, p, p, 0, 1, 4, 1, 2, p, 0, 0, 4, 3, 0, p, p, p, 0, 0) == OK
    assert jw(0, p, p, p, 1, 4, p, p, p, 1, 1, 4, 1, 2, 0, 1, 0, 4, 3, 0, p, p, p, 0, 0) == EINVAL
    assert jw(0, p, p, p, 1, 4, p, p, p, 1, 1, 4, 1, 2, p, 1, 0, 4, 3, 1, p, p, p, 0, 0) == EINVAL     # keys asked, none given
    assert jw(0, p, p, p, 1, 4, p, p, p, 1, 1, 4, 1, 2, p, 1, 0, 4, 3, 0, 0, p, p, 0, 0) == EINVAL
    assert jw(0, p, p, p, 1, 4, p, p, p, 1, 1, 4, 1, 2, p, -1, 0, 4, 3, 0, p, p, p, 0, 0) == EINVAL


# -------------------------------------------------------------------------------------------------------------- boundary_iou
PAIR_SIZES = ((33, 47), (64, 64), (40, 37), (56, 29), (48, 64), (64, 35))


def boundary_pairs(seed=20261021, per_size=50):
    """per canvas size 50 pairs: gt = a thresholded smooth field, dt = the same field shifted and thresholded again"""
    rng = np.random.default_rng(seed)
    out = {}
    for h, w in PAIR_SIZES:
        pairs = []
        for _ in range(per_size):
            f = ndi.gaussian_filter(rng.standard_normal((h, w)), 3)
            dy, dx = int(rng.integers(1, 3)), int(rng.integers(0, 3))
            pairs.append((np.roll(f, (dy, dx), (0, 1)) > -0.02 + rng.uniform(-0.01, 0.01), f > -0.02))
        out[h, w] = pairs
    return out


def check_boundary_iou(apis, dev, pytest):
    import _large_image_ref as lref
    enc = lambda m: [int(v) for v in lref.rle_counts_np(m)]                          # noqa: E731
    n_pairs = 0
    for j, ((h, w), pairs) in enumerate(boundary_pairs().items()):
        r = mref.radius((h, w))
        dts, gts = [p[0] for p in pairs], [p[1] for p in pairs]
        db, gb = [mref.boundary(m, r) for m in dts], [mref.boundary(m, r) for m in gts]
        assert all(np.array_equal(b, mref.boundary_cropped(m, r)) for b, m in zip(db + gb, dts + gts))
        crowd = [bool(i % 4 == 0) for i in range(len(gts))]
        for i in range(len(pairs)):                          # of the oracle: min() is exercised by every pair
            assert 0 < mref.iou(db[i], gb[i]) < mref.iou(dts[i], gts[i]), (h, w, i)
            n_pairs += 1
        want = {c: np.array([[mref.iou(a, b, cr and c) for b, cr in zip(gb, crowd)] for a in db]) for c in (False, True)}
        mask = {c: np.array([[mref.iou(a, b, cr and c) for b, cr in zip(gts, crowd)] for a in dts]) for c in (False, True)}
        packed = lambda ms: [dict(size=[h, w], counts=ref.rle_to_string(enc(m))) for m in ms]   # noqa: E731
        plain = lambda ms: [dict(size=[h, w], counts=enc(m)) for m in ms]                       # noqa: E731
        if j % 3 == 0:
            d_arg, g_arg = torch.from_numpy(np.stack(dts)).to(dev), torch.from_numpy(np.stack(gts)).to(dev)
        elif j % 3 == 1:
            d_arg, g_arg = packed(dts), plain(gts)
        else:                                                # mixed counts forms in one list
            d_arg = [(packed if i % 2 else plain)([m])[0] for i, m in enumerate(dts)]
            g_arg = packed(gts)
        got = apis.boundary_iou(d_arg, g_arg, device=dev)
        assert got.dtype == torch.float64 and tuple(got.shape) == (len(dts), len(gts))
        assert got.device.type == torch.device(dev).type
        assert np.array_equal(got.cpu().numpy(), want[False]), (h, w)
        got = apis.boundary_iou(d_arg, g_arg, crowd, device=dev)
        assert np.array_equal(got.cpu().numpy(), want[True]) and not np.array_equal(want[True], want[False])
        got = apis.boundary_iou(d_arg, g_arg, crowd, min_with_mask=True, device=dev)
        assert np.array_equal(got.cpu().numpy(), np.minimum(want[True], mask[True]))
        # a radius of its own, a ratio of its own
        got = apis.boundary_iou(d_arg[:3], g_arg[:4], radius=3, device=dev)
        assert np.array_equal(got.cpu().numpy(), np.array([[mref.boundary_iou(a, b, r=3) for b in gts[:4]] for a in dts[:3]]))
        got = apis.boundary_iou(d_arg[:3], g_arg[:4], dilation_ratio=0.1, device=dev)
        assert np.array_equal(got.cpu().numpy(),
                              np.array([[mref.boundary_iou(a, b, dilation_ratio=0.1) for b in gts[:4]] for a in dts[:3]]))
        # mask_boundary in the form of its input
        src = d_arg[:5] if j % 3 != 2 else packed(dts[:5])      # one counts form per call, as remove_small_regions asks
        bands = apis.mask_boundary(src, device=dev)
        if isinstance(bands, torch.Tensor):
            assert bands.dtype == torch.bool and np.array_equal(bands.cpu().numpy(), np.stack(db[:5]))
        else:
            for b, a, want_b in zip(bands, src, db[:5]):
                assert type(b['counts']) is type(a['counts']) and b['size'] == [h, w]
                c = ref.rle_fr_string(b['counts']) if isinstance(b['counts'], bytes) else b['counts']
                assert np.array_equal(ref.rle_decode(c, h, w).astype(bool), want_b)
    assert n_pairs == 300
    # the other way round: a square against its own outline -- the bands agree, the masks do not
    sq = np.zeros((40, 40), bool)
    sq[5:35, 5:35] = True
    frame = sq & ~mref.erode(sq, 1, 0)
    pair = torch.from_numpy(np.stack([sq, frame])).to(dev)
    assert apis.boundary_iou(pair[:1], pair[1:], radius=1).cpu().tolist() == [[1.0]]
    assert apis.boundary_iou(pair[:1], pair[1:], radius=1, min_with_mask=True).cpu().tolist() == [[int(frame.sum()) / 900]]
    a, b = dict(size=[2, 3], counts=[1, 2, 3]), dict(size=[4, 1], counts=ref.rle_to_string([0, 3, 1]))
    with pytest.raises(ValueError, match='different sizes'):
        apis.boundary_iou([a], [b], device=dev)
    with pytest.raises(ValueError, match='iscrowd'):
        apis.boundary_iou([a], [a, a], [True], device=dev)
    with pytest.raises(ValueError, match='dilation_ratio'):
        apis.boundary_iou([a], [a], dilation_ratio=0, device=dev)
    with pytest.raises(ValueError, match='op must be'):
        apis.mask_morphology([a], 'buffer', 1, device=dev)
    with pytest.raises(ValueError, match='radius'):
        apis.mask_morphology([a], 'erode', -1, device=dev)
    assert apis.boundary_iou([a], [a], device=dev).cpu().tolist() == [[1.0]]
    assert apis.boundary_iou([], [a], device=dev).shape == (0, 1) and apis.boundary_iou([a], [], device=dev).shape == (1, 0)


# -------------------------------------------------------------------------------------------------------------------- metric
class BoundaryEval(ref.COCOeval):
    """COCOeval(iouType='segm') with the IoU of every pair replaced by min(mask IoU, IoU of the bands); the bands come from
    the numpy oracle, per annotation, with the radius of the annotation's image"""
    dilation_ratio = 0.02

    def _band(self, ann):
        if '_band' not in ann:
            import _large_image_ref as lref
            c, h, w = ann['_rle']
            band = mref.boundary_cropped(ref.rle_decode(c, h, w).astype(bool), mref.radius((h, w), self.dilation_ratio),
                                         separable=h * w > 1 << 16)     # scene-sized: the form that does not grow with r
            ann['_band'] = ([int(v) for v in lref.rle_counts_np(band)], h, w)
        return ann['_band']

    def computeIoU(self, imgId, catId):
        p = self.params
        gt, dt = self._gts[imgId, catId], self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        dt = [dt[i] for i in np.argsort([-d['score'] for d in dt], kind='mergesort')][:p.maxDets[-1]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        if len(dt) == 0 or len(gt) == 0:
            return []
        mask = ref.rle_iou([d['_rle'] for d in dt], [g['_rle'] for g in gt], iscrowd)
        band = ref.rle_iou([self._band(d) for d in dt], [self._band(g) for g in gt], iscrowd)
        return np.minimum(mask, band)


def boundary_oracle(m, prefix, dilation_ratio=0.02):
    """the subclassed restatement on the metric's own ground truth and its written segm results -> (stats, COCOeval)"""
    gt = ref.COCO(m.coco_gt)
    dt = gt.loadRes([{k: v for k, v in r.items() if k != 'bbox'} for r in json.load(open(f'{prefix}.segm.json'))])
    ev = BoundaryEval(gt, dt, 'segm')
    ev.dilation_ratio = dilation_ratio
    ev.params.catIds, ev.params.imgIds, ev.params.maxDets = gt.getCatIds(), gt.getImgIds(), [100, 300, 1000]
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev.stats, ev


def run_boundary_metric(evaluation, dev, classes, images, per_img, tmp_path, name, **kw):
    """CocoMetric(metric=['segm', 'boundary']) on both routes against the oracle and against a call without 'boundary'"""
    import _coco_cases as cc
    got = {}
    for domain in ('bits', 'runs'):
        prefix = str(tmp_path / f'{name}_{domain}' / 'r')
        m = evaluation.CocoMetric(metric=['segm', 'boundary'], device=str(dev), outfile_prefix=prefix, iou_domain=domain, **kw)
        cic_run(m, classes, images, per_img)
        assert m.timings['boundary']['iou_domain'] == domain and m.timings['boundary']['band'] > 0
        got[domain] = m, prefix
    b, r = got['bits'][0], got['runs'][0]
    for t in ('segm', 'boundary'):
        assert np.array_equal(b.eval_results[t].stats, r.eval_results[t].stats), (name, t)
        for k in ('dtm', 'dtig', 'npig'):
            assert np.array_equal(b.eval_results[t].tables[k], r.eval_results[t].tables[k]), (name, t, k)
    want, rev = boundary_oracle(r, got['runs'][1], kw.get('dilation_ratio', 0.02))
    stats = r.eval_results['boundary'].stats
    assert np.array_equal(stats, want), (name, stats, want)
    cc.check_tables_equal(r.eval_results['boundary'].tables, rev)
    # the segm stats of the same call equal those of a call without 'boundary'
    plain = evaluation.CocoMetric(metric='segm', device=str(dev), iou_domain='runs',
                                  **{k: v for k, v in kw.items() if k != 'dilation_ratio'})
    cic_run(plain, classes, images, per_img)
    assert np.array_equal(plain.eval_results['segm'].stats, r.eval_results['segm'].stats)
    assert list(plain.eval_results) == ['segm'] and list(r.eval_results) == ['segm', 'boundary']
    assert stats[0] <= r.eval_results['segm'].stats[0]                               # boundary_mAP <= segm_mAP
    table = r.summary_table()
    assert '*boundary*' in table and table.count('Average Precision') == 12 and table.count('Average Recall') == 12
    return r


def cic_run(m, classes, images, per_img):
    """process / evaluate as _coco_iou_runs_cases._run_metric does them, on a metric built by the caller"""
    m.dataset_meta = dict(classes=classes)
    samples = []
    for im in images:
        p = per_img.get(im['id'], [])
        pi = dict(bboxes=torch.tensor([q[0] for q in p], dtype=torch.float32).view(-1, 4),
                  scores=torch.tensor([q[1] for q in p], dtype=torch.float32),
                  labels=torch.tensor([q[2] for q in p], dtype=torch.int64), masks=[q[3] for q in p])
        samples.append(dict(pred_instances=pi, img_id=im['id'], ori_shape=(im['height'], im['width'])))
    m.process(None, samples)
    m.last_result = m.evaluate(len(samples))
    return m


def check_metric_nwpu(evaluation, dev, tmp_path, pytest):
    ref.use_numpy_forms()
    ann_file, classes, images, per_img, samples_gt = cic.nwpu_detections()
    assert len({(im['height'], im['width']) for im in images}) > 1                   # several sizes: the grouping is exercised
    m = run_boundary_metric(evaluation, dev, classes, images, per_img, tmp_path, 'ann_file', ann_file=ann_file)
    keys = [k for k in m.last_result if 'boundary' in k]
    assert keys == [f'coco/boundary_{s}' for s in ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l')]
    # without the detections that ARE the ground truth's masks: only the moved copies, whose band IoU lies below their mask IoU
    moved = {k: v[1::2] for k, v in per_img.items()}
    m = run_boundary_metric(evaluation, dev, classes, images, moved, tmp_path, 'moved', ann_file=ann_file)
    b, s = m.eval_results['boundary'].stats, m.eval_results['segm'].stats
    print('NWPU subset, moved masks: boundary', b[:3], 'segm', s[:3])
    assert 0.0 < b[0] < s[0]
    # a ratio of its own moves the numbers and the oracle with them
    thin = run_boundary_metric(evaluation, dev, classes, images, moved, tmp_path, 'thin', ann_file=ann_file,
                               dilation_ratio=0.005)
    assert not np.array_equal(thin.eval_results['boundary'].stats, b)
    with pytest.raises(KeyError):
        evaluation.CocoMetric(metric='edges')
    for bad in (0, -0.02, float('inf'), float('nan'), '0.02', True):
        with pytest.raises(ValueError, match='dilation_ratio'):
            evaluation.CocoMetric(metric='boundary', dilation_ratio=bad)
    assert evaluation.CocoMetric().metrics == ['bbox'] and evaluation.CocoMetric().dilation_ratio == 0.02


def check_metric_scenes(evaluation, apis, dev, tmp_path, sizes):
    ref.use_numpy_forms()
    saved = ref.rle_iou
    ref.rle_iou = cic.LITERAL_IOU                                 # the literal walk skips the pairs rleIou's bbIou skips
    try:
        gt, classes, per_img = cic.scene_set(apis, dev, sizes)
        ann = tmp_path / 'scenes.json'
        ann.write_text(json.dumps(gt))
        m = run_boundary_metric(evaluation, dev, classes, gt['images'], per_img, tmp_path, 'scenes', ann_file=str(ann))
        assert 0.0 < m.eval_results['boundary'].stats[0] < m.eval_results['segm'].stats[0]
    finally:
        ref.rle_iou = saved
