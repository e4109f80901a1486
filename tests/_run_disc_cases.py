"""Case bodies of the Euclidean buffers (csrc/run_disc.hip, ops.rle_dilate_disc / rle_erode_disc / rle_minus,
rle.half_heights / *_runs(element=...) / buffer_runs, apis.mask_morphology(element=...) / buffer_masks,
inference_large_image(buffer=...)), run on the lane emulator by tests/test_run_disc_cpu.py and on the device by
tests/test_gpu_run_disc.py.  The oracle is tests/_run_disc_ref.py (dense numpy: scipy's footprint morphology and the
thresholded integer distance transform, which must agree).  Every comparison is ==."""
import fractions
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _coco_iou_runs_cases as cic  # noqa: E402
import _cocoeval_ref as ref  # noqa: E402
import _run_disc_ref as dref  # noqa: E402
import _run_morphology_cases as mcases  # noqa: E402

rows_from_counts = mcases.rows_from_counts
rows_from_masks = mcases.rows_from_masks
decode = mcases.decode
ReadCounter = mcases.ReadCounter
OK, EINVAL = 0, -1
R2S = (0, 1, 2, 3, 4, 5, 8, 9, 10, 24, 25, 26)


def hh_of(r2, shape=None):
    from rsprompter_amd import rle
    return rle.half_heights('disc', r2=r2, size=shape)[0]


def dilate_table(ops, counts, n, H, W, hh, cap=None):
    c, m, n_host, cap2 = ops.rle_dilate_disc(counts, n, H, W, hh, cap)
    assert c.dtype == torch.int32 and m.dtype == torch.int32 and tuple(c.shape) == (n.shape[0], cap2)
    assert np.array_equal(m.cpu().numpy(), n_host.numpy())
    return decode(c, n_host, H, W)


def erode_table(ops, counts, n, H, W, hh, border=0, cap=None):
    c, m, n_host, cap2 = ops.rle_erode_disc(counts, n, H, W, hh, border, cap)
    assert c.dtype == torch.int32 and m.dtype == torch.int32 and tuple(c.shape) == (n.shape[0], cap2)
    assert np.array_equal(m.cpu().numpy(), n_host.numpy())
    return decode(c, n_host, H, W)


def check_masks(ops, dev, masks, r2, what=''):
    """dilation and erosion (both borders) of dense masks of one size against the oracle"""
    H, W = masks[0].shape
    counts, n = rows_from_masks(masks, dev)
    hh = hh_of(r2, (H, W))
    got = dilate_table(ops, counts, n, H, W, hh)
    for i, m in enumerate(masks):
        assert np.array_equal(got[i], dref.dilate(m, r2)), (what, 'dilate', i, r2, H, W)
    for b in (0, 1):
        got = erode_table(ops, counts, n, H, W, hh, b)
        for i, m in enumerate(masks):
            assert np.array_equal(got[i], dref.erode(m, r2, b)), (what, 'erode', i, r2, b, H, W)


# ------------------------------------------------------------------------------------------------------------------ oracle
def check_oracle(rle):
    """the two forms agree (every call of dref asserts it), the cropped forms equal the full ones, and the half-heights are
    the footprint's columns"""
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (1, 9), (9, 1), (7, 5), (40, 37), (33, 64)):
        for r2 in (1, 2, 4, 5, 8, 9, 13, 25, 50):
            for m in (np.ones((h, w), bool), rng.random((h, w)) < 0.9, mcases.blob(rng, h, w, 0.0), mcases.blob(rng, h, w, -0.05)):
                d = dref.dilate(m, r2)
                assert np.array_equal(d, dref.dilate_cropped(m, r2))
                for b in (0, 1):
                    e = dref.erode(m, r2, b)
                    assert np.array_equal(e, dref.erode_cropped(m, r2, b)), (h, w, r2, b)
                    assert not (e & ~m).any() and not (m & ~d).any()
                assert np.array_equal(~dref.erode(~m, r2, 1), d)
    for r in (0, 1, 2, 5):
        m = mcases.blob(rng, 30, 31)
        assert np.array_equal(~dref.diamond_erode(~m, r, 1), dref.diamond_dilate(m, r))
    for r2 in list(range(0, 60)) + [10 ** 4, 10 ** 6 + 1]:
        hh, R = rle.half_heights('disc', r2=r2)
        assert R == math.isqrt(r2) == len(hh) - 1 == hh[0] and all(a >= b for a, b in zip(hh, hh[1:]))
        if r2 < 60:
            fp = dref.footprint(r2)
            assert [int(fp[R:, R + dx].sum()) - 1 for dx in range(R + 1)] == hh
    assert rle.half_heights('disc', r2=25)[0] == [5, 4, 4, 4, 3, 0] and rle.half_heights('disc', r2=24)[0] == [4, 4, 4, 3, 2]
    assert rle.half_heights('disc', r2=0) == ([0], 0) and rle.half_heights('disc', r2=1) == ([1, 0], 1)
    assert rle.half_heights('disc', r2=2) == ([1, 1], 1) and rle.half_heights('diamond', 3) == ([3, 2, 1, 0], 3)
    # a real radius: floor(d^2) in exact arithmetic
    assert [rle.disc_r2(d) for d in (0, 1, 1.5, 2.9, 3, '1.5', fractions.Fraction(3, 2), 1.4142135623730951)] == \
        [0, 1, 2, 8, 9, 2, 2, 2]
    assert rle.disc_r2(0.1 + 0.2) == 0 and rle.disc_r2(2.23606797749979) == 5 and rle.disc_r2(2.2360679774997) == 4
    assert rle.disc_r2(10 ** 6) == 10 ** 12 and rle.disc_r2(1e6) == 10 ** 12
    assert rle.half_heights('disc', radius=2.9) == rle.half_heights('disc', r2=8)
    assert rle.half_heights('disc', r2=10 ** 12, size=(5, 7))[1] == math.isqrt(74)


# --------------------------------------------------------------------------------------------------------- hand-checked
def check_hand_checked(ops, dev):
    z = lambda h, w: np.zeros((h, w), bool)                                          # noqa: E731

    def dil(mask, r2):
        H, W = mask.shape
        counts, n = rows_from_masks([mask], dev)
        got = dilate_table(ops, counts, n, H, W, hh_of(r2, (H, W)))[0]
        assert np.array_equal(got, dref.dilate(mask, r2)), (r2, mask.shape)
        return got

    def ero(mask, r2, b=0):
        H, W = mask.shape
        counts, n = rows_from_masks([mask], dev)
        got = erode_table(ops, counts, n, H, W, hh_of(r2, (H, W)), b)[0]
        assert np.array_equal(got, dref.erode(mask, r2, b)), (r2, b, mask.shape)
        return got
    # one pixel in the middle of 15 x 15: the footprint itself; eroded back (outside set) it is the pixel again
    for r2 in R2S:
        R = math.isqrt(r2)
        m = z(15, 15)
        m[7, 7] = True
        d = dil(m, r2)
        want = z(15, 15)
        want[7 - R:8 + R, 7 - R:8 + R] = dref.footprint(r2)
        assert np.array_equal(d, want)
        assert np.array_equal(ero(d, r2, 1), m)
        # the same pixel in every corner and on every edge: clipped on all four sides, sources whose targets leave [0, W)
        for y in (0, 7, 14):
            for x in (0, 7, 14):
                m = z(15, 15)
                m[y, x] = True
                assert np.array_equal(ero(dil(m, r2), r2, 1), m)
    d = dil(np.pad(np.ones((1, 1), bool), 7), 25)
    assert d[7 + 4, 7 + 3] and d[7 + 3, 7 + 4] and d[7 + 5, 7] and not d[7 + 4, 7 + 4] and d.sum() == 81
    d = dil(np.pad(np.ones((1, 1), bool), 7), 24)
    assert not d[7 + 4, 7 + 3] and not d[7 + 5, 7] and d.sum() == 69
    assert dil(np.pad(np.ones((1, 1), bool), 7), 1).sum() == 5 and dil(np.pad(np.ones((1, 1), bool), 7), 2).sum() == 9
    # all ones: border 1 keeps it, border 0 leaves [R, W - R) x [R, H - R), nothing on 5 x 5 with R = 3
    full = np.ones((11, 13), bool)
    for r2 in (1, 2, 4, 5, 9, 10, 16):
        R = math.isqrt(r2)
        want = z(11, 13)
        want[R:11 - R, R:13 - R] = True
        assert ero(full, r2, 1).all() and np.array_equal(ero(full, r2, 0), want)
    assert not ero(np.ones((5, 5), bool), 9, 0).any() and ero(np.ones((5, 5), bool), 9, 1).all()
    assert ero(np.ones((5, 5), bool), 4, 0).sum() == 1
    # two pixels 2R + 1 and 2R columns apart: the dilations touch in neighbouring columns, then overlap in one
    for r2 in (1, 4, 5, 9):
        R = math.isqrt(r2)
        for gap in (2 * R + 1, 2 * R):
            m = z(2 * R + 3, 4 * R + 5)
            m[R + 1, R + 1] = m[R + 1, R + 1 + gap] = True
            d = dil(m, r2)
            shared = 2 * hh_of(r2)[R] + 1 if gap == 2 * R else 0      # the one column both reach: dx = R from either
            assert d[R + 1, R + 1:R + 2 + gap].all() and d.sum() == 2 * dref.footprint(r2).sum() - shared
    # a one-pixel hole under dilate and under close
    for r2 in (1, 2, 5):
        m = np.ones((15, 16), bool)
        m[7, 8] = False
        assert dil(m, r2).all()
        e = ero(m, r2, 1)
        assert (~e).sum() == dref.footprint(r2).sum()
        assert ero(dil(m, r2), r2, 1).all()
    # canvases of 1 x 9 and 9 x 1, W < 2R + 1, H < 2R + 1
    for shape in ((1, 9), (9, 1)):
        m = np.zeros(shape, bool)
        m.reshape(-1)[4] = True
        assert dil(m, 4).reshape(-1).tolist() == [False, False, True, True, True, True, True, False, False]
        assert dil(m, 3).sum() == 3 and dil(m, 100).all()
        assert not ero(np.ones(shape, bool), 1, 0).any() and ero(np.ones(shape, bool), 1, 1).all()
        assert ero(~m, 1, 1).sum() == 6 and ero(~m, 1, 0).sum() == 0
    for shape in ((20, 4), (4, 20)):
        full = np.ones(shape, bool)
        assert not ero(full, 4, 0).any() and ero(full, 4, 1).all() and ero(full, 1, 0).sum() == 18 * 2
        m = z(*shape)
        m[1, 1] = True
        dil(m, 4), dil(m, 9), dil(m, 50), ero(~m, 4, 0), ero(~m, 9, 1)
    # a huge radius on a small canvas
    rng = np.random.default_rng(5)
    m = rng.random((9, 11)) < 0.3
    assert dil(m, 10 ** 12).all() and not ero(m, 10 ** 12, 0).any() and not ero(m, 10 ** 12, 1).any()
    assert ero(np.ones((9, 11), bool), 10 ** 12, 1).all() and not dil(z(9, 11), 10 ** 12).any()
    assert np.array_equal(dil(m, 0), m) and np.array_equal(ero(m, 0, 0), m) and np.array_equal(ero(m, 0, 1), m)
    # an unclamped table of half-heights far longer than the canvas is wide
    counts, n = rows_from_masks([m], dev)
    assert dilate_table(ops, counts, n, 9, 11, hh_of(10 ** 6))[0].all()
    assert not erode_table(ops, counts, n, 9, 11, hh_of(10 ** 6), 0)[0].any()
    # the empty row, the empty mask, all ones -- in one table
    counts, n = rows_from_counts([None, [99], [0, 99]], dev)
    got = dilate_table(ops, counts, n, 9, 11, hh_of(5))
    assert not got[0].any() and not got[1].any() and got[2].all()
    for b in (0, 1):
        got = erode_table(ops, counts, n, 9, 11, hh_of(5), b)
        assert not got[0].any() and not got[1].any()
        assert got[2].all() if b else (got[2].sum() == 5 * 7 and got[2][2:7, 2:9].all())
    # a ones-run crossing several column ends
    flat = np.zeros(7 * 9, bool)
    flat[5:40] = True
    m = flat.reshape(9, 7).T
    assert cic.enc(m) == [5, 35, 23]
    for r2 in (1, 2, 5):
        dil(m, r2), ero(m, r2, 0), ero(m, r2, 1)


# ----------------------------------------------------------------------------------------------------------------- the pruning
def pruning_masks():
    H, W = 24, 30
    comb = np.zeros((H, W), bool)
    comb[3:-3, ::2] = True                                       # every piece exposed on both sides
    checker = (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(bool)
    stair = np.zeros((H, W), bool)
    for x in range(W):
        stair[min(x * H // W, H - 1):, x] = True
    notch = np.zeros((H, W), bool)
    notch[4:20, 2:27] = True
    notch[11, 26] = False                                        # a one-pixel notch in the right side
    right = np.zeros((H, W), bool)
    right[5:15, 20:] = True                                      # touches column W - 1: E+ is empty inside the canvas
    left = right[:, ::-1].copy()
    return [comb, checker, stair, notch, right, left]


def check_pruning(ops, dev):
    masks = pruning_masks()
    for r2 in (1, 2, 5, 9, 26):
        check_masks(ops, dev, masks + [~m for m in masks], r2, what=f'pruning r2={r2}')
    # the intervals emitted are the pieces plus R times the exposed parts: a wide rectangle exposes two columns only
    rect = np.zeros((64, 64), bool)
    rect[10:50, 4:60] = True
    counts, n = rows_from_masks([rect], dev)
    seen = []
    real = torch.sort

    def spy(t, *a, **kw):
        seen.append(int(t.numel()))
        return real(t, *a, **kw)
    torch.sort = spy
    try:
        ops.rle_dilate_disc(counts, n, 64, 64, hh_of(9))
    finally:
        torch.sort = real
    assert seen == [56 + 3 * 2], seen


# ------------------------------------------------------------------------------------------------- list and wave boundaries
def check_list_boundaries(ops, dev):
    """columns of 0 .. 130 pieces beside columns of one long piece, both ways round (mcases.check_list_boundaries' masks)"""
    H, W = 260, 12
    comb = lambda p: np.isin(np.arange(H), 2 * np.arange(p))                         # noqa: E731
    thick = lambda p: np.isin(np.arange(H) % 4, (0, 1, 2)) & (np.arange(H) < 4 * p)   # noqa: E731
    masks = []
    for make in (comb, thick):
        for swap in (0, 1):
            m = np.zeros((H, W), bool)
            for j, p in enumerate(mcases.PIECES):
                x = j + 2 if not swap else W - 3 - j
                m[:, x] = make(min(p, H // 4 if make is thick else p))
            for x in ([0, 1, W - 2, W - 1] if not swap else [0, W - 1]):
                m[3:H - 2, x] = True
            masks.append(m)
    m = np.zeros((H, W), bool)
    for j, p in enumerate(mcases.PIECES[:6]):
        m[:, 2 * j] = True
        m[:, 2 * j + 1] = thick(min(p, 65))
    masks += [m, ~m, ~masks[0], ~masks[2]]
    for r2 in (1, 5):
        check_masks(ops, dev, masks, r2, what=f'lists r2={r2}')


# ------------------------------------------------------------------------------------------------------- non-canonical counts
def check_non_canonical(ops, dev):
    rng = np.random.default_rng(43)
    tie = [3, 0, 0, 4, 5, 0, 0, 0, 0, 6, 2]
    split = [3, 2, 0, 2, 5, 6, 2]
    plain = [3, 4, 5, 6, 2]
    lead = [0, 0, 0, 0, 3, 4, 5, 6, 2, 0, 0]
    for H, W in ((20, 1), (10, 2), (4, 5), (2, 10)):
        counts, n = rows_from_counts([tie, split, plain, lead], dev)
        dense = cic.stream(plain).reshape(W, H).T
        for r2 in (0, 1, 2):
            hh = hh_of(r2)
            assert all(np.array_equal(g, dref.dilate(dense, r2)) for g in dilate_table(ops, counts, n, H, W, hh)), (H, W, r2)
            for b in (0, 1):
                got = erode_table(ops, counts, n, H, W, hh, b)
                assert all(np.array_equal(g, dref.erode(dense, r2, b)) for g in got), (H, W, r2, b)
    for H, W in ((7, 9), (40, 37)):
        canon = [cic.enc(rng.random((H, W)) < d) for d in (0.5, 0.9, 0.97) for _ in range(2)] + [[0, H * W], [H * W]]
        canon += [cic.enc(mcases.blob(rng, H, W))]
        bent = [cic.with_zeros(c, rng) for c in canon] + [cic.with_zeros(canon[0], rng, 40)]
        dense = [cic.stream(c).reshape(W, H).T for c in bent]
        counts, n = rows_from_counts(bent, dev)
        for r2 in (1, 5):
            hh = hh_of(r2)
            got = dilate_table(ops, counts, n, H, W, hh)
            assert all(np.array_equal(g, dref.dilate(d, r2)) for g, d in zip(got, dense)), (H, W, r2)
            for b in (0, 1):
                got = erode_table(ops, counts, n, H, W, hh, b)
                assert all(np.array_equal(g, dref.erode(d, r2, b)) for g, d in zip(got, dense)), (H, W, r2, b)


# ------------------------------------------------------------------------------------------------------------------ diamond
def check_diamond(ops, rle, apis, dev):
    rng = np.random.default_rng(9)
    masks = pruning_masks() + [mcases.blob(rng, 24, 30), np.ones((24, 30), bool)]
    one = np.zeros((24, 30), bool)
    one[12, 15] = True
    masks.append(one)
    H, W = 24, 30
    counts, n = rows_from_masks(masks, dev)
    for r in (1, 2, 5):
        hh = rle.half_heights('diamond', r)[0]
        got = dilate_table(ops, counts, n, H, W, hh)
        assert all(np.array_equal(g, dref.diamond_dilate(m, r)) for g, m in zip(got, masks)), r
        for b in (0, 1):
            got = erode_table(ops, counts, n, H, W, hh, b)
            assert all(np.array_equal(g, dref.diamond_erode(m, r, b)) for g, m in zip(got, masks)), (r, b)
        t = torch.from_numpy(np.stack(masks)).to(dev)
        got = apis.mask_morphology(t, 'boundary', r, device=dev, element='diamond').cpu().numpy()
        assert all(np.array_equal(g, m & ~dref.diamond_erode(m, r, 0)) for g, m in zip(got, masks))
        got = apis.mask_morphology(t, 'close', r, device=dev, element='diamond').cpu().numpy()
        assert all(np.array_equal(g, dref.diamond_erode(dref.diamond_dilate(m, r), r, 1)) for g, m in zip(got, masks))
    assert dilate_table(ops, counts[-1:], n[-1:], H, W, rle.half_heights('diamond', 2)[0])[0].sum() == 13


# -------------------------------------------------------------------------------------------------------------- seeded random
R2_DRAW = [1, 2, 4, 5, 8, 9, 10, 13, 16, 18, 25]


def random_masks(seed=20261022, count=240):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        h, w = int(rng.integers(8, 65)), int(rng.integers(8, 65))
        r2 = R2_DRAW[int(rng.integers(0, 11))]
        out.append((mcases.blob(rng, h, w), r2))
    return out


def _radius_of(r2, j):
    """a radius that gives r2: the integer r2 through its exact square root where there is one, else a float above sqrt(r2)"""
    R = math.isqrt(r2)
    if R * R == r2:
        return R
    d = math.sqrt(r2) + 1e-9                                     # floor(d^2) == r2: checked, not assumed
    assert math.floor(fractions.Fraction(repr(d)) ** 2) == r2
    return d


def check_random(ops, apis, dev):
    """240 masks, every operation of mask_morphology(element='disc'), in the three mask forms"""
    cases = random_masks()
    want = [{op: fn(m, r2) for op, fn in dref.OPS.items()} for m, r2 in cases]
    assert sum(1 for w in want if w['erode'].any()) >= 180 and all(w['boundary'].any() for w in want)
    groups = {}
    for i, (m, r2) in enumerate(cases):
        groups.setdefault((m.shape, r2), []).append(i)
    for j, ((shape, r2), idx) in enumerate(sorted(groups.items())):
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
            got = apis.mask_morphology(arg, op, _radius_of(r2, j), device=dev, element='disc')
            if form == 0:
                assert got.dtype == torch.bool and tuple(got.shape) == (len(idx), H, W)
                dense = list(got.cpu().numpy())
            else:
                assert all(g['size'] == [H, W] and isinstance(g['counts'], bytes if form == 1 else list) for g in got)
                dense = [ref.rle_decode(ref.rle_fr_string(g['counts']) if form == 1 else g['counts'], H, W).astype(bool)
                         for g in got]
            for i, d in zip(idx, dense):
                assert np.array_equal(d, want[i][op]), (op, i, shape, r2, form)


# -------------------------------------------------------------------------------------------------------------- buffer_masks
def check_buffer_masks(apis, dev):
    rng = np.random.default_rng(12)
    H, W = 40, 37
    masks = [mcases.blob(rng, H, W), rng.random((H, W)) < 0.9, np.ones((H, W), bool), np.zeros((H, W), bool)]
    t = torch.from_numpy(np.stack(masks)).to(dev)
    for d, r2 in ((1.5, 2), (2.9, 8), (3, 9), (1, 1), ('2.5', 6)):
        assert dref.buffer is not None
        got = apis.buffer_masks(t, d, device=dev)
        assert got.dtype == torch.bool and torch.equal(got, apis.mask_morphology(t, 'dilate', float(d), device=dev, element='disc'))
        assert all(np.array_equal(g, dref.dilate(m, r2)) for g, m in zip(got.cpu().numpy(), masks)), d
        neg = -d if not isinstance(d, str) else '-' + d
        got = apis.buffer_masks(t, neg, device=dev).cpu().numpy()
        assert all(np.array_equal(g, dref.erode(m, r2, 1)) for g, m in zip(got, masks)), d
    assert torch.equal(apis.buffer_masks(t, 0, device=dev), t) and torch.equal(apis.buffer_masks(t, -0.0, device=dev), t)
    assert torch.equal(apis.buffer_masks(t, 0.9, device=dev), t)                     # floor(0.81) = 0
    assert apis.buffer_masks(t[:0], 2, device=dev).shape == (0, H, W)
    for packed in (True, False):
        arg = [dict(size=[H, W], counts=ref.rle_to_string(cic.enc(m)) if packed else cic.enc(m)) for m in masks]
        for d, r2 in ((2.9, 8), (-2.9, -8), (0, 0)):
            got = apis.buffer_masks(arg, d, device=dev)
            assert all(g['size'] == [H, W] and isinstance(g['counts'], bytes if packed else list) for g in got)
            dense = [ref.rle_decode(ref.rle_fr_string(g['counts']) if packed else g['counts'], H, W).astype(bool) for g in got]
            assert all(np.array_equal(g, dref.buffer(m, r2)) for g, m in zip(dense, masks)), (packed, d)


# ------------------------------------------------------------------------------------------------------------------ protocol
def check_protocol(ops, rle, dev, monkeypatch):
    rng = np.random.default_rng(77)
    H, W = 40, 37
    masks = [mcases.blob(rng, H, W), rng.random((H, W)) < 0.9, np.ones((H, W), bool), np.zeros((H, W), bool),
             mcases.blob(rng, H, W, 0.0)]
    r2 = 5
    hh = hh_of(r2)
    want_d = [dref.dilate(m, r2) for m in masks]
    want_e = [dref.erode(m, r2, 0) for m in masks]
    counts, n = rows_from_masks(masks, dev)
    # capacities of their own, a table far wider than its rows
    wide, _ = rows_from_masks(masks, dev, cap=4000)
    for c in (counts, wide):
        assert all(np.array_equal(g, w) for g, w in zip(dilate_table(ops, c, n, H, W, hh, cap=1024), want_d))
        assert all(np.array_equal(g, w) for g, w in zip(erode_table(ops, c, n, H, W, hh, 0, cap=777), want_e))
    # a cap too small: the retry grows it (fit_runs), and the number of host reads is the documented one
    need = max(len(cic.enc(w)) for w in want_d)
    assert need > 8
    with ReadCounter(dev) as rc:
        c2, n2, n_host2, cap2 = ops.rle_dilate_disc(counts, n, H, W, hh, cap=2)
    assert cap2 == ops.grown_cap(need) and rc.n == 2 + 2, (rc.n, cap2, need)
    assert all(np.array_equal(g, w) for g, w in zip(decode(c2, n_host2, H, W), want_d))
    with ReadCounter(dev) as rc:
        c3, n3, n_host3, cap3 = ops.rle_dilate_disc(counts, n, H, W, hh, cap=4096)
    assert cap3 == 4096 and rc.n == 2 + 1, rc.n
    with ReadCounter(dev) as rc:
        c4, n4, n_host4, cap4 = ops.rle_erode_disc(counts, n, H, W, hh, 0, cap=4096)
    assert cap4 == 4097 and rc.n == 2 + 1 + 1, rc.n
    with ReadCounter(dev) as rc:
        ops.rle_dilate_disc(counts, n, H, W, [0], cap=4096)                           # the identity: no exposed parts to count
        ops.rle_dilate_disc(counts[3:4], n[3:4], H, W, hh, cap=4096)                  # no piece
    assert rc.n == 2 * (1 + 1), rc.n
    with ReadCounter(dev) as rc:
        cb, nb, nb_host, _ = ops.rle_minus(counts, n, c4, n4, H, W, cap=4096)
    assert rc.n == 2 + 1, rc.n
    assert all(np.array_equal(g, dref.boundary(m, r2)) for g, m in zip(decode(cb, nb_host, H, W), masks))
    # n > cap is read up to cap: the row cut after `cut` counts describes a shorter stream; what it holds is dilated
    row = cic.enc(masks[0])
    cut = 7
    c_cut, n_cut = rows_from_counts([row[:cut]], dev)
    n_cut[0] = len(row)
    short = np.zeros(H * W, bool)
    short[:sum(row[:cut])] = cic.stream(row[:cut])
    short = short.reshape(W, H).T
    assert np.array_equal(dilate_table(ops, c_cut, n_cut, H, W, hh)[0], dref.dilate(short, r2))
    assert np.array_equal(erode_table(ops, c_cut, n_cut, H, W, hh, 1)[0], dref.erode(short, r2, 1))
    # a second launch gives the same bits
    again = ops.rle_dilate_disc(counts, n, H, W, hh, cap=4096)
    assert torch.equal(again[1], n3) and all(torch.equal(again[0][i, :m], c3[i, :m]) for i, m in enumerate(n_host3.tolist()))
    again = ops.rle_erode_disc(counts, n, H, W, hh, 0, cap=4096)
    assert torch.equal(again[1], n4) and all(torch.equal(again[0][i, :m], c4[i, :m]) for i, m in enumerate(n_host4.tolist()))
    # k = 0 launches nothing and reads nothing from the device
    c0, n0 = counts[:0], n[:0]
    for out in (ops.rle_dilate_disc(c0, n0, H, W, hh), ops.rle_erode_disc(c0, n0, H, W, hh), ops.rle_minus(c0, n0, c0, n0, H, W)):
        assert out[0].shape[0] == 0 and out[1].shape[0] == 0 and out[2].shape[0] == 0
    # the row chunking: six blobs of one size, a budget of half their intervals -- several passes, none above the budget, the
    # results those of the one pass
    blobs = [mcases.blob(rng, H, W) for _ in range(6)]
    bc, bn = rows_from_masks(blobs, dev)
    real = torch.sort
    seen = []

    def spy(t, *a, **kw):
        seen.append(int(t.numel()))
        return real(t, *a, **kw)
    monkeypatch.setattr(torch, 'sort', spy)
    for fn in (lambda: ops.rle_dilate_disc(bc, bn, H, W, hh, cap=4096), lambda: ops.rle_erode_disc(bc, bn, H, W, hh, 0, cap=4096)):
        del seen[:]
        whole = fn()
        assert len(seen) == 1
        total, budget = seen[0], seen[0] // 2
        monkeypatch.setattr(ops, 'DISC_MAX_INTERVALS', budget)
        del seen[:]
        parts = fn()
        assert len(seen) >= 2 and sum(seen) == total and all(v <= budget for v in seen), (budget, seen)
        monkeypatch.setattr(ops, 'DISC_MAX_INTERVALS', 1 << 26)
        assert torch.equal(parts[1], whole[1]) and torch.equal(parts[2], whole[2])
        assert all(torch.equal(parts[0][i, :m], whole[0][i, :m]) for i, m in enumerate(whole[2].tolist()))
    monkeypatch.setattr(torch, 'sort', real)
    # a single row above the budget is refused by its number and its count
    monkeypatch.setattr(ops, 'DISC_MAX_INTERVALS', 50)
    import pytest
    zc, zn = rows_from_masks([np.zeros((H, W), bool), blobs[0], np.zeros((H, W), bool)], dev)
    with pytest.raises(ValueError, match=r'row 1 alone emits \d+ intervals'):
        ops.rle_dilate_disc(zc, zn, H, W, hh)
    monkeypatch.setattr(ops, 'DISC_MAX_INTERVALS', 1 << 26)
    # the derived operations
    for fn, name in ((rle.erode_runs, 'erode'), (rle.dilate_runs, 'dilate'), (rle.open_runs, 'open'), (rle.close_runs, 'close'),
                     (rle.boundary_runs, 'boundary')):
        c, m, n_host, _ = fn(counts, n, (H, W), math.sqrt(5) + 1e-9, element='disc')
        assert all(np.array_equal(g, dref.OPS[name](w, 5)) for g, w in zip(decode(c, n_host, H, W), masks)), name
        c, m, n_host, _ = fn(counts, n, (H, W), 2)                                   # the default stays the square
        assert all(np.array_equal(g, mcases.mref.OPS[name](w, 2)) for g, w in zip(decode(c, n_host, H, W), masks)), name
    for d, r2s in ((2.9, 8), (-1.5, -2), (0, 0)):
        c, m, n_host, _ = rle.buffer_runs(counts, n, (H, W), d)
        assert all(np.array_equal(g, dref.buffer(w, r2s)) for g, w in zip(decode(c, n_host, H, W), masks)), d


def check_refusals(ops, rle, apis, dev, pytest):
    from rsprompter_amd import _lib
    lib = _lib.load()
    counts, n = rows_from_counts([[3, 4, 5]], dev)
    for bad in (None, [], [1, 2], [-1], [2, 1, -1], 'ab', 3):
        with pytest.raises(ValueError, match='hh must be'):
            ops.rle_dilate_disc(counts, n, 3, 4, bad)
    for border in (2, -1):
        with pytest.raises(ValueError, match='border'):
            ops.rle_erode_disc(counts, n, 3, 4, [1, 0], border)
    with pytest.raises(ValueError, match='32-bit'):
        ops.rle_dilate_disc(counts, n, 65536, 32768, [1, 0])
    with pytest.raises(ValueError, match='expected counts'):
        ops.rle_erode_disc(counts.to(torch.int64), n, 3, 4, [1, 0])
    with pytest.raises(ValueError, match='row by row'):
        ops.rle_minus(counts, n, counts[:0], n[:0], 3, 4)
    for kw in (dict(element='square', radius=1), dict(element='disc'), dict(element='disc', radius=1, r2=1),
               dict(element='disc', r2=-1), dict(element='disc', r2=1.5), dict(element='disc', r2=True),
               dict(element='disc', radius=-1), dict(element='disc', radius=float('nan')), dict(element='disc', radius=float('inf')),
               dict(element='disc', radius='x'), dict(element='disc', radius=True), dict(element='diamond', radius=1.5),
               dict(element='diamond', radius=-1), dict(element='diamond', r2=4), dict(element='diamond', radius=True)):
        with pytest.raises(ValueError):
            rle.half_heights(**kw)
    a = dict(size=[2, 3], counts=[1, 2, 3])
    assert apis.MORPHOLOGY_ELEMENTS == ('square', 'disc', 'diamond')
    assert apis.MORPHOLOGY_OPS == ('erode', 'dilate', 'open', 'close', 'boundary')
    with pytest.raises(ValueError, match='element must be'):
        apis.mask_morphology([a], 'erode', 1, device=dev, element='ellipse')
    with pytest.raises(ValueError, match='element must be'):
        apis.mask_boundary([a], radius=1, device=dev, element='ellipse')
    with pytest.raises(ValueError, match='op must be'):
        apis.mask_morphology([a], 'buffer', 1, device=dev, element='disc')
    for element, bad in (('disc', -1), ('disc', -0.5), ('disc', float('nan')), ('disc', float('inf')), ('disc', None),
                         ('disc', True), ('square', 1.5), ('diamond', 1.5), ('diamond', -1), ('square', -1)):
        with pytest.raises((ValueError, TypeError)):
            apis.mask_morphology([a], 'dilate', bad, device=dev, element=element)
    for bad in (float('nan'), float('inf'), None, 'far', True):
        with pytest.raises(ValueError, match='distance'):
            apis.buffer_masks([a], bad, device=dev)
    dense = cic.stream(a['counts']).reshape(3, 2).T
    assert apis.mask_morphology([a], 'dilate', 1.0, device=dev, element='disc')[0]['counts'] == cic.enc(dref.dilate(dense, 1))
    assert apis.mask_boundary([a], radius=1, device=dev, element='disc')[0]['counts'] == cic.enc(dref.boundary(dense, 1))
    # the entry point itself
    p = counts.data_ptr()
    hh = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    offs = torch.zeros((2,), dtype=torch.int64, device=dev)
    col = torch.zeros((4,), dtype=torch.int32, device=dev)
    keys = torch.zeros((4,), dtype=torch.int64, device=dev)
    c, h, o, q = col.data_ptr(), hh.data_ptr(), offs.data_ptr(), keys.data_ptr()
    emit = lambda *a: lib.rsp_run_disc_emit(*a, 0)                                   # noqa: E731
    assert emit(c, c, c, 0, 1, 3, 4, h, 1, 0, 0, 0, 1, q, q) == OK                   # no interval: a no-op
    assert emit(c, c, c, 1, 0, 3, 4, h, 1, 0, 0, 0, 1, q, q) == OK                   # k == 0
    assert emit(c, c, c, 1, 1, 3, 4, h, 1, 0, 0, 0, 0, 0, 0) == OK                   # no slot
    assert emit(c, c, c, 1, 1, 3, 4, h, 0, 1, 0, 0, 1, q, q) == OK                   # no neighbour column to reach
    assert emit(c, c, c, 1, 1, 3, 4, h, 1, 0, 0, 0, 1, q, q) == OK                   # y0 = y1 = 0: the lane stores nothing
    assert keys.cpu().tolist() == [0, 0, 0, 0]
    assert emit(c, c, c, -1, 1, 3, 4, h, 1, 0, 0, 0, 1, q, q) == EINVAL
    assert emit(c, c, c, 1, -1, 3, 4, h, 1, 0, 0, 0, 1, q, q) == EINVAL
    assert emit(c, c, c, 1, 1, 65536, 32768, h, 1, 0, 0, 0, 1, q, q) == EINVAL       # H * W >= 2^31
    assert emit(c, c, c, 1, 2 ** 20, 3, 2048, h, 1, 0, 0, 0, 1, q, q) == EINVAL      # k * W >= 2^31
    assert emit(c, c, c, 1, 1, 3, 4, h, -1, 0, 0, 0, 1, q, q) == EINVAL
    assert emit(c, c, c, 1, 1, 3, 4, h, 4, 0, 0, 0, 1, q, q) == EINVAL               # R > W - 1
    assert emit(c, c, c, 1, 1, 3, 4, h, 1, 2, o, 0, 1, q, q) == EINVAL and emit(c, c, c, 1, 1, 3, 4, h, 1, -2, o, 0, 1, q, q) == EINVAL
    assert emit(c, c, c, 1, 1, 3, 4, h, 1, 0, 0, -1, 1, q, q) == EINVAL and emit(c, c, c, 1, 1, 3, 4, h, 1, 0, 0, 2, 1, q, q) == EINVAL
    assert emit(c, c, c, 1, 1, 3, 4, h, 1, 0, 0, 0, 2 ** 31, q, q) == EINVAL and emit(c, c, c, 1, 1, 3, 4, h, 1, 0, 0, 0, -1, q, q) == EINVAL
    assert emit(0, c, c, 1, 1, 3, 4, h, 1, 0, 0, 0, 1, q, q) == EINVAL and emit(c, 0, c, 1, 1, 3, 4, h, 1, 0, 0, 0, 1, q, q) == EINVAL
    assert emit(c, c, 0, 1, 1, 3, 4, h, 1, 0, 0, 0, 1, q, q) == EINVAL and emit(c, c, c, 1, 1, 3, 4, 0, 1, 0, 0, 0, 1, q, q) == EINVAL
    assert emit(c, c, c, 1, 1, 3, 4, h, 1, 0, 0, 0, 1, 0, q) == EINVAL and emit(c, c, c, 1, 1, 3, 4, h, 1, 0, 0, 0, 1, q, 0) == EINVAL
    assert emit(c, c, c, 1, 1, 3, 4, h, 1, 1, 0, 0, 1, q, q) == EINVAL               # a side without its slot ranges
    # the join takes a negative shift for the difference only; what it took before it takes as before
    jc = lambda *a: lib.rsp_run_morph_join_count(*a, 0)                              # noqa: E731
    assert jc(1, c, c, c, 1, 4, c, c, c, 1, 1, 4, -1, 1, 0, 4, c) == OK
    assert jc(0, c, c, c, 1, 4, c, c, c, 1, 1, 4, -1, 1, 0, 4, c) == EINVAL


# ------------------------------------------------------------------------------------------------------------- large_image
def check_large_image_refusals(li, pytest):
    """the signature and what is refused before the first tile runs, without a model"""
    import inspect
    sig = inspect.signature(li.inference_large_image).parameters
    assert sig['buffer'].default == 0.0
    with pytest.raises(ValueError, match="buffer works on the scene run table"):
        li.inference_large_image(None, np.zeros((8, 8, 3), np.uint8), masks='dense', buffer=2.0)
    for bad in (float('nan'), float('inf'), 'wide', None, True):
        with pytest.raises(ValueError, match='buffer must be'):
            li.inference_large_image(None, np.zeros((8, 8, 3), np.uint8), buffer=bad)
    for argv in (['img.png', 'cfg.py', 'none', '--buffer', 'nan'], ['img.png', 'cfg.py', 'none', '--buffer', 'inf'],
                 ['img.png', 'cfg.py', 'none', '--buffer']):
        with pytest.raises(SystemExit):
            li.main(argv)


def _dense(masks, H, W):
    return np.stack([ref.rle_decode(ref.rle_fr_string(m['counts']), H, W).astype(bool) for m in masks]) if len(masks) else \
        np.zeros((0, H, W), bool)


def check_scene_buffer(dev, plain, grown, shrunk, flat, d, H, W):
    """pred_instances of inference_large_image without a buffer, with buffer=+d, with buffer=-d and with buffer=+d and
    flatten='score' (masks='rle', the same other arguments) -> K"""
    r2 = math.floor(fractions.Fraction(repr(float(d))) ** 2)
    K = len(plain.scores)
    base = _dense(plain.masks, H, W)
    assert 'buffer_area' not in plain
    for out, sign in ((grown, 1), (shrunk, -1)):
        assert len(out.masks) == K
        for key in ('bboxes', 'scores', 'labels'):
            assert torch.equal(getattr(plain, key), getattr(out, key))
        got = _dense(out.masks, H, W)
        want = np.stack([dref.buffer(m, sign * r2) for m in base]) if K else base
        assert np.array_equal(got, want), sign
        assert out.buffer_area.dtype == torch.int32 and tuple(out.buffer_area.shape) == (K, 2)
        assert out.buffer_area.cpu().numpy().tolist() == [[int(a.sum()), int(b.sum())] for a, b in zip(base, want)]
    got = _dense(flat.masks, H, W)
    want = np.stack([dref.dilate(m, r2) for m in base]) if K else base
    assert (got.sum(0) <= 1).all() and np.array_equal(got.any(0), want.any(0))      # pairwise disjoint, the same union
    assert not (got & ~want).any()
    assert flat.buffer_area.cpu().numpy()[:, 1].tolist() == want.reshape(K, -1).sum(1).tolist()
    assert flat.flatten_area.cpu().numpy()[:, 0].tolist() == want.reshape(K, -1).sum(1).tolist()
    return K


def check_pipeline(li, dev, model, merge):
    """inference_large_image around a stub detector on a 45 x 70 scene of 32 x 32 tiles -> K"""
    scene = np.random.default_rng(16).integers(0, 256, (45, 70, 3)).astype(np.uint8)
    kw = dict(patch_size=32, batch_size=2, merge_iou_thr=0.25, merge_nms_type=merge)
    if merge == 'seam_mask':
        kw['seam_iou_thr'] = 0.3
    run = lambda **k: li.inference_large_image(model, scene, **kw, **k).pred_instances   # noqa: E731
    K = check_scene_buffer(dev, run(), run(buffer=1.5), run(buffer=-1.5), run(buffer=1.5, flatten='score'), 1.5, 45, 70)
    rings = run(buffer=1.5, masks='polygons', flatten='score', oriented_boxes=True)
    assert sum(int(a2) for inst in rings.masks for _, _, a2 in inst) == 2 * int(rings.flatten_area[:, 1].sum())
    assert rings.obb.shape == (K, 4, 2)
    return K
