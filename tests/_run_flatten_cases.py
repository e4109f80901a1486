"""Case bodies of planar instance layers (csrc/run_flatten.hip, ops.rle_flatten / rle_label_map, rle.flatten_runs /
runs_to_labels, apis.flatten_masks / masks_to_label_map), run on the lane emulator by
tests/test_run_flatten_cpu.py and on the device by tests/test_gpu_run_flatten.py.  The oracle is tests/_run_flatten_ref.py
(dense numpy, two forms that must agree).  Every comparison is ==."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _coco_iou_runs_cases as cic  # noqa: E402
import _cocoeval_ref as ref  # noqa: E402
import _run_flatten_ref as fref  # noqa: E402
import _run_morphology_cases as mcases  # noqa: E402
import _seam_merge_cases as seam_cases  # noqa: E402

rows_from_counts = seam_cases.rows_from_counts
rows_from_masks = seam_cases.rows_from_masks
decode = mcases.decode
ReadCounter = mcases.ReadCounter
OK, EINVAL = 0, -1


# -------------------------------------------------------------------------------------------------------------- helpers
def rank_tensor(rank, dev):
    return torch.tensor([int(r) for r in rank], dtype=torch.int32).to(dev)


def flatten_table(ops, counts, n, H, W, rank, cap=None):
    """ops.rle_flatten -> dense masks, every row checked to be canonical COCO counts"""
    c, m, cap2 = ops.rle_flatten(counts, n, H, W, rank_tensor(rank, counts.device), cap)
    assert c.dtype == torch.int32 and m.dtype == torch.int32 and tuple(c.shape) == (n.shape[0], cap2)
    return decode(c, m.cpu(), H, W)


def check_partition(masks, flat, rank):
    """what follows from the definition, asserted of a result: pairwise disjoint, the union kept, the rank-0 row unchanged"""
    masks, flat = np.asarray(masks, bool), np.asarray(flat, bool)
    if not len(masks):
        return
    assert flat.sum(0).max() <= 1
    assert np.array_equal(flat.any(0), masks.any(0))
    top = int(np.argmin(rank))
    assert np.array_equal(flat[top], masks[top])
    assert int(flat.sum()) == int(masks.any(0).sum())
    assert not (flat & ~masks).any()


def check_masks(ops, dev, masks, rank, what=''):
    """ops.rle_flatten and ops.rle_label_map on dense masks of one size against the oracle -> the flattened masks"""
    masks = [np.asarray(m, bool) for m in masks]
    H, W = masks[0].shape
    counts, n = rows_from_masks(masks, dev)
    c, m, cap = ops.rle_flatten(counts, n, H, W, rank_tensor(rank, dev))
    assert c.dtype == torch.int32 and m.dtype == torch.int32 and tuple(c.shape) == (len(masks), cap)
    got = np.stack(decode(c, m.cpu(), H, W))
    want = fref.flatten(np.stack(masks), rank)
    assert np.array_equal(got, want), (what, H, W, list(rank))
    check_partition(masks, got, rank)
    lab = ops.rle_label_map(c, m, H, W)
    assert lab.dtype == torch.int32 and tuple(lab.shape) == (H, W)
    assert np.array_equal(lab.cpu().numpy(), fref.label_map(want)), (what, 'labels')
    return got


def column(H, *intervals):
    """an H x 1 mask set on the row intervals [a, b)"""
    m = np.zeros((H, 1), bool)
    for a, b in intervals:
        m[a:b] = True
    return m


def check_oracle():
    """the definition and the restatement of panoptic_postprocess agree, and the two derived ranks are what they say"""
    rng = np.random.default_rng(5)
    for h, w, k in ((1, 1, 2), (1, 9, 3), (9, 1, 4), (7, 5, 1), (24, 31, 9), (39, 39, 12)):
        for d in (0.2, 0.5, 0.9):
            masks = rng.random((k, h, w)) < d
            rank = rng.permutation(k)
            scores = fref.scores_of_rank(rank)
            assert len(set(scores.tolist())) == k and 0 < scores.min() and scores.max() <= 1
            a, b = fref.flatten(masks, rank), fref.flatten_fusion(masks, scores)
            assert np.array_equal(a, b), (h, w, k, d)
            check_partition(masks, a, rank)
            assert np.array_equal(fref.rank_of_scores(scores), rank)
    assert fref.rank_of_scores([0.5, 0.9, 0.5, 0.1]).tolist() == [1, 0, 2, 3]
    m = np.zeros((3, 2, 2), bool)
    m[0], m[1, 0, 0], m[2, 0, 0] = True, True, True
    assert fref.rank_of_areas(m).tolist() == [2, 0, 1]
    assert fref.flatten(m[:0], []).shape == (0, 2, 2) and fref.flatten_fusion(m[:0], []).shape == (0, 2, 2)


# --------------------------------------------------------------------------------------------------------- hand-checked
def check_hand_checked(ops, rle, dev):
    one = lambda masks, rank, what='': check_masks(ops, dev, masks, rank, what)      # noqa: E731
    rng = np.random.default_rng(9)
    # 1 x 1: the better one keeps the pixel
    full = np.ones((1, 1), bool)
    got = one([full, full], [1, 0], '1x1')
    assert not got[0].any() and got[1].all()
    # 1 x W (every pixel its own column) and H x 1 (one column)
    for shape in ((1, 9), (9, 1), (1, 70), (70, 1)):
        masks = rng.random((4,) + shape) < 0.6
        for _ in range(3):
            one(masks, rng.permutation(4), str(shape))
    # k = 1: the row comes back; an all-empty row and a row with n < 0 / n = 0 are empty masks, one count H * W
    m = rng.random((7, 9)) < 0.5
    assert np.array_equal(one([m], [0])[0], m)
    counts, n = rows_from_counts([cic.enc(m), [63], None, cic.enc(~m), [0, 63]], dev)
    n[2] = -5
    rank = [2, 0, 1, 4, 3]
    c, nn, _ = ops.rle_flatten(counts, n, 7, 9, rank_tensor(rank, dev))
    got = decode(c, nn.cpu(), 7, 9)
    assert np.array_equal(np.stack(got), fref.flatten(np.stack([m, m & False, m & False, ~m, m | True]), rank))
    assert nn.cpu().tolist()[1:3] == [1, 1] and c[1:3, 0].cpu().tolist() == [63, 63]
    assert np.array_equal(got[0], m) and not got[3].any() and np.array_equal(got[4], ~m)
    # a piece cut into four survivors; the blockers touch neither each other nor the ends
    low = column(20, (0, 20))
    got = one([low, column(20, (2, 4)), column(20, (7, 9)), column(20, (12, 13))], [3, 0, 2, 1], 'four survivors')
    assert cic.enc(got[0]) == [0, 2, 2, 3, 2, 3, 1, 7]
    # a piece fully covered (the instance keeps its other piece), an instance fully covered: one count H * W, kept False
    two = column(20, (1, 5), (10, 15))
    got = one([two, column(20, (0, 6))], [1, 0], 'piece covered')
    assert cic.enc(got[0]) == [10, 5, 5]
    masks = [two, column(20, (0, 6)), column(20, (9, 16))]
    counts, n = rows_from_masks(masks, dev)
    c, nn, cap, before, after, kept = rle.flatten_runs(counts, n, (20, 1), [2, 1, 0])
    assert nn.cpu().tolist()[0] == 1 and int(c[0, 0]) == 20
    assert kept.cpu().tolist() == [False, True, True] and before.cpu().tolist() == [9, 6, 7] and after.cpu().tolist() == [0, 6, 7]
    assert kept.dtype == torch.bool and before.dtype == torch.int32 and after.dtype == torch.int32
    # blockers that only touch: y1_j == y0 and y0_j == y1
    mid = column(20, (5, 10))
    got = one([mid, column(20, (0, 5)), column(20, (10, 15))], [2, 0, 1], 'touching')
    assert np.array_equal(got[0], mid)
    # the nesting case `reach` exists for: in column order [0, 100) (better), [10, 20) (worse), then the piece [50, 60): y1
    # alone is not sorted (100, 20, 60), the running maximum is
    piece = column(100, (50, 60))
    got = one([piece, column(100, (0, 100)), column(100, (10, 20))], [1, 0, 2], 'nesting')
    assert not got[0].any() and cic.enc(got[2]) == [100]
    got = one([piece, column(100, (0, 55)), column(100, (10, 20))], [1, 0, 2], 'nesting, part')
    assert cic.enc(got[0]) == [55, 5, 40]
    got = one([piece, column(100, (0, 100)), column(100, (10, 20))], [1, 2, 0], 'nesting, the long one worse')
    assert np.array_equal(got[0], piece) and cic.enc(got[1]) == [0, 10, 10, 30, 10, 40]
    # overlapping blockers of different instances (cur = max), one of them inside another
    got = one([column(20, (0, 20)), column(20, (3, 10)), column(20, (6, 14)), column(20, (8, 9))], [3, 1, 0, 2], 'overlapping')
    assert cic.enc(got[0]) == [0, 3, 11, 6] and cic.enc(got[1]) == [3, 3, 14] and not got[3].any()
    got = one([column(20, (0, 20)), column(20, (3, 14)), column(20, (6, 10))], [2, 0, 1], 'inside')
    assert cic.enc(got[0]) == [0, 3, 11, 6]
    # equal y0 in one column from several instances, every order of the three
    trio = [column(20, (4, 8)), column(20, (4, 12)), column(20, (4, 6)), column(20, (0, 20))]
    for perm in ([0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]):
        one(trio, perm + [3], 'equal y0')
        one(trio, [p + 1 for p in perm] + [0], 'equal y0 under a cover')
    # runs that cross column ends: stream slices of a 7 x 9 canvas
    def of_stream(*slices):
        flat = np.zeros(63, bool)
        for a, b in slices:
            flat[a:b] = True
        return flat.reshape(9, 7).T
    masks = [of_stream((5, 40)), of_stream((0, 8), (20, 30)), of_stream((13, 15), (27, 29), (34, 50)), of_stream((0, 63))]
    assert cic.enc(masks[0]) == [5, 35, 23]
    for perm in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1], [1, 3, 0, 2]):
        one(masks, perm, 'column ends')
    got = one(masks, [1, 0, 2, 3])
    assert cic.enc(got[0]) == [8, 12, 10, 10, 23]


def check_tied_scores(apis, dev):
    """duplicate masks with tied scores: the lower index keeps everything (the argmax of torch CPU)"""
    rng = np.random.default_rng(10)
    m = rng.random((9, 11)) < 0.5
    other = rng.random((9, 11)) < 0.5
    masks = torch.from_numpy(np.stack([other, m, m, m])).to(dev)
    got, info = apis.flatten_masks(masks, scores=[0.25, 0.5, 0.5, 0.5], device=dev)
    got = got.cpu().numpy()
    assert np.array_equal(got[1], m) and not got[2].any() and not got[3].any() and np.array_equal(got[0], other & ~m)
    assert info['rank'].tolist() == [3, 0, 1, 2] and info['kept'].cpu().tolist() == [bool((other & ~m).any()), True, False, False]
    got, info = apis.flatten_masks(masks, scores=torch.tensor([0.5, 0.5, 0.5, 0.5]), device=dev)
    assert info['rank'].tolist() == [0, 1, 2, 3] and np.array_equal(got[0].cpu().numpy(), other)
    # order='area': the smaller mask on top, ties to the lower index
    small = np.zeros((9, 11), bool)
    small[2:4, 3:5] = True
    big = np.ones((9, 11), bool)
    got, info = apis.flatten_masks(torch.from_numpy(np.stack([big, small, small])).to(dev), order='area', device=dev)
    assert info['rank'].tolist() == [2, 0, 1]
    got = got.cpu().numpy()
    assert np.array_equal(got[0], ~small) and np.array_equal(got[1], small) and not got[2].any()


# ------------------------------------------------------------------------------------------------- wave and chunk boundaries
PIECES = (63, 64, 65, 128, 129)


def check_wave_boundaries(ops, dev):
    """a 260 x 3 canvas whose columns hold p one-pixel pieces of p instances, beside two instances that cover the columns
    from end to end: the carry of `reach` over the chunks of a column, and walks that cross a chunk"""
    H, W = 260, 3
    rng = np.random.default_rng(64)
    for p in PIECES:
        masks = []
        for i in range(p):
            m = np.zeros((H, W), bool)
            m[2 * i, :] = True
            if i % 7 == 0:
                m[2 * i:2 * i + 2, 1] = True                       # some two pixels long: they touch the next instance
            masks.append(m)
        long1 = np.zeros((H, W), bool)
        long1[:, 1] = True
        long1[3:200, 0] = True
        masks += [long1, np.ones((H, W), bool)]
        k = len(masks)
        for trial in range(2):
            rank = rng.permutation(k)
            if trial == 0:                                          # the long ones in the middle and at the bottom
                rank = np.argsort(np.argsort(np.concatenate([rng.random(p), [0.5, 2.0]])))
            check_masks(ops, dev, masks, rank, f'p={p}')


# ------------------------------------------------------------------------------------------------------- non-canonical counts
def check_non_canonical(ops, dev):
    rng = np.random.default_rng(43)
    for H, W in ((20, 1), (4, 5), (7, 9), (24, 17)):
        k = 5
        dense = rng.random((k, H, W)) < 0.6
        canon = [cic.enc(m) for m in dense]
        bent = [cic.with_zeros(c, rng) for c in canon[:-1]] + [cic.with_zeros(canon[-1], rng, 30)]
        assert all(np.array_equal(cic.stream(b).reshape(W, H).T, m) for b, m in zip(bent, dense))
        assert any(0 in b[1:] for b in bent)
        counts, n = rows_from_counts(bent, dev)
        for _ in range(3):
            rank = rng.permutation(k)
            got = flatten_table(ops, counts, n, H, W, rank)
            assert np.array_equal(np.stack(got), fref.flatten(dense, rank)), (H, W)


# -------------------------------------------------------------------------------------------------------------- seeded random
def random_case(rng):
    h, w, k = int(rng.integers(1, 49)), int(rng.integers(1, 41)), int(rng.integers(1, 13))
    kind = int(rng.integers(0, 3))
    masks = np.zeros((k, h, w), bool)
    for i in range(k):
        if kind == 0:
            masks[i] = rng.random((h, w)) < rng.uniform(0.1, 0.9)
        else:
            for _ in range(int(rng.integers(1, 4))):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
                y1, x1 = int(rng.integers(y0, h)) + 1, int(rng.integers(x0, w)) + 1
                masks[i, y0:y1, x0:x1] = True
                if kind == 2 and y1 - y0 > 2 and x1 - x0 > 2:                       # a rectangle with a hole
                    masks[i, y0 + 1:y1 - 1, x0 + 1:int(rng.integers(x0 + 2, x1))] = False
    return masks, rng.permutation(k)


def _dense_of(got, form, H, W):
    if form == 'dense':
        assert got.dtype == torch.bool
        return got.cpu().numpy()
    if form == 'runs':
        return np.stack(decode(got[0], got[1].cpu(), H, W))
    out = []
    for g in got:
        assert g['size'] == [H, W] and isinstance(g['counts'], bytes if form == 'strings' else list)
        out.append(ref.rle_decode(ref.rle_fr_string(g['counts']) if form == 'strings' else g['counts'], H, W).astype(bool))
    return np.stack(out)


def check_random(apis, dev, count=300, seed=20261020):
    """300 seeded cases through apis.flatten_masks and masks_to_label_map: every input form (dense, compressed, uncompressed)
    against every output form (as it came, 'rle', 'runs', 'dense'), an explicit rank; every fifth case by score, every
    seventh by area; min_ratio on every third"""
    rng = np.random.default_rng(seed)
    covered = set()
    for j in range(count):
        masks, rank = random_case(rng)
        k, H, W = masks.shape
        scores, order = None, rank
        if j % 5 == 4:
            scores = rng.integers(0, 4, k) / 4.0                                     # ties
            order, rank = 'score', fref.rank_of_scores(scores)
        elif j % 7 == 6:
            order, rank = 'area', fref.rank_of_areas(masks)
        ratio = 0.0 if j % 3 else float(rng.choice([0.25, 0.5, 0.9, 1.0]))
        part = fref.flatten(masks, rank)
        check_partition(masks, part, rank)
        want, want_kept = fref.apply_min_ratio(masks, part, ratio)
        in_form, out_form = ('dense', 'strings', 'lists')[j % 3], (None, 'rle', 'runs', 'dense')[(j // 3) % 4]
        covered.add((in_form, out_form))
        if in_form == 'dense':
            arg = torch.from_numpy(masks).to(dev)
        elif in_form == 'strings':
            arg = [dict(size=[H, W], counts=ref.rle_to_string(cic.enc(m))) for m in masks]
        else:
            arg = [dict(size=[H, W], counts=cic.enc(m)) for m in masks]
        got, info = apis.flatten_masks(arg, scores=scores, order=order, min_ratio=ratio, form=out_form, device=dev)
        form = in_form if out_form is None else {'rle': 'strings'}.get(out_form, out_form)
        got = _dense_of(got, form, H, W)
        assert np.array_equal(got, want), (j, H, W, k, in_form, out_form, ratio)
        assert info['rank'].tolist() == [int(r) for r in rank] and info['kept'].cpu().tolist() == want_kept.tolist()
        assert info['area_before'].cpu().tolist() == masks.reshape(k, -1).sum(1).tolist()
        assert info['area_after'].cpu().tolist() == want.reshape(k, -1).sum(1).tolist()
        if ratio == 0.0:
            assert int(info['area_after'].sum()) == int(masks.any(0).sum())
        ids = None if j % 2 else rng.integers(1, 1000, k)
        lab = apis.masks_to_label_map(arg, scores=scores, order=order, ids=ids, min_ratio=ratio, device=dev)
        assert lab.dtype == torch.int32 and tuple(lab.shape) == (H, W)
        assert np.array_equal(lab.cpu().numpy(), fref.label_map(want, ids)), (j, 'labels')
    assert len(covered) == 12


# ------------------------------------------------------------------------------------------------------------------ protocol
class Poison:
    """inside, every torch.empty starts as `byte`: an output slot nobody stored shows as that pattern"""

    def __init__(self, byte):
        self.byte = byte

    def __enter__(self):
        self.saved = torch.empty

        def empty(*a, **kw):
            t = self.saved(*a, **kw)
            if t.numel() and t.is_contiguous() and not t.dtype.is_complex and t.dtype != torch.bool:
                t.view(torch.uint8).fill_(self.byte)
            return t
        torch.empty = empty

    def __exit__(self, *a):
        torch.empty = self.saved


def check_protocol(ops, rle, dev):
    rng = np.random.default_rng(77)
    H, W, k = 40, 37, 6
    masks = np.stack([mcases.blob(rng, H, W) for _ in range(k - 1)] + [np.ones((H, W), bool)])
    rank = [3, 1, 4, 0, 2, 5]
    want = fref.flatten(masks, rank)
    counts, n = rows_from_masks(list(masks), dev)
    rt = rank_tensor(rank, dev)
    # poisoned output buffers, two patterns: the same bits, the oracle's
    outs = []
    for byte in (0xFF, 0x55):
        with Poison(byte):
            c, m, cap = ops.rle_flatten(counts, n, H, W, rt, cap=512)
            lab = ops.rle_label_map(c, m, H, W)
        assert cap == 512 and np.array_equal(np.stack(decode(c, m.cpu(), H, W)), want)
        assert np.array_equal(lab.cpu().numpy(), fref.label_map(want))
        outs.append((c, m, lab))
    m_host = outs[0][1].cpu().tolist()
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    assert all(torch.equal(outs[0][0][i, :v], outs[1][0][i, :v]) for i, v in enumerate(m_host))
    # a table far wider than its rows, a capacity of its own
    wide, _ = rows_from_masks(list(masks), dev, cap=3000)
    assert np.array_equal(np.stack(flatten_table(ops, wide, n, H, W, rank, cap=777)), want)
    # a result row that needs more counts than the input's capacity: five lines across the canvas (75 counts each) cut the
    # full row (two counts) into six pieces per column, 372 counts
    masks = np.zeros((k, H, W), bool)
    for i in range(5):
        masks[i, 3 + 6 * i] = True
    masks[5] = True
    rank = [3, 1, 4, 0, 2, 5]
    want = fref.flatten(masks, rank)
    counts, n = rows_from_masks(list(masks), dev)
    need = max(len(cic.enc(w)) for w in want)
    assert int(counts.shape[1]) == 75 and need == len(cic.enc(want[5])) == 372 and ops.grown_cap(need) == 512
    with ReadCounter(dev) as rc:
        c2, n2, cap2 = ops.rle_flatten(counts, n, H, W, rt)
    assert cap2 == ops.grown_cap(need) and rc.n == 3 + 1, (rc.n, cap2, need)      # the documented three and one retry
    assert np.array_equal(np.stack(decode(c2, n2.cpu(), H, W)), want)
    with ReadCounter(dev) as rc:
        c3, n3, cap3 = ops.rle_flatten(counts, n, H, W, rt, cap=2)
    assert cap3 == cap2 and rc.n == 4
    with ReadCounter(dev) as rc:
        c4, n4, cap4 = ops.rle_flatten(counts, n, H, W, rt, cap=4096)
    assert cap4 == 4096 and rc.n == 3, rc.n
    with ReadCounter(dev) as rc:
        ops.rle_label_map(c4, n4, H, W)
    assert rc.n == 1, rc.n
    # a table without a piece: two reads
    ce, ne = rows_from_counts([[H * W], None], dev)
    with ReadCounter(dev) as rc:
        c5, n5, _ = ops.rle_flatten(ce, ne, H, W, rank_tensor([1, 0], dev))
    assert rc.n == 2 and n5.cpu().tolist() == [1, 1] and c5[:, 0].cpu().tolist() == [H * W, H * W]
    assert not ops.rle_label_map(c5, n5, H, W).cpu().numpy().any()
    # a second launch gives the same bits
    again = ops.rle_flatten(counts, n, H, W, rt, cap=4096)
    n_host = n4.cpu().tolist()
    assert torch.equal(again[1], n4) and all(torch.equal(again[0][i, :v], c4[i, :v]) for i, v in enumerate(n_host))
    assert torch.equal(ops.rle_label_map(c4, n4, H, W), ops.rle_label_map(*again[:2], H, W))
    # k = 0
    c0, n0, _ = ops.rle_flatten(counts[:0], n[:0], H, W, rt[:0])
    assert c0.shape[0] == 0 and n0.shape[0] == 0
    lab = ops.rle_label_map(counts[:0], n[:0], H, W)
    assert tuple(lab.shape) == (H, W) and not lab.cpu().numpy().any()
    # min_ratio against its definition, ids of the caller's
    for ratio in (0.0, 0.5, 0.9, 1.0):
        c, m, _, before, after, kept = rle.flatten_runs(counts, n, (H, W), rank, ratio)
        w2, k2 = fref.apply_min_ratio(masks, want, ratio)
        assert np.array_equal(np.stack(decode(c, m.cpu(), H, W)), w2) and kept.cpu().tolist() == k2.tolist()
        assert after.cpu().tolist() == w2.reshape(k, -1).sum(1).tolist() and before.cpu().tolist() == masks.reshape(k, -1).sum(1).tolist()
        ids = [7, 7, 900, 2 ** 31 - 1, 5, 1]
        assert np.array_equal(rle.runs_to_labels(c, m, (H, W), ids).cpu().numpy(), fref.label_map(w2, ids))
    assert not fref.apply_min_ratio(masks, want, 0.9)[1].all() and fref.apply_min_ratio(masks, want, 0.0)[1].all()


def check_refusals(ops, rle, apis, dev, pytest, monkeypatch):
    from rsprompter_amd import _lib, large_image
    lib = _lib.load()
    counts, n = rows_from_counts([[3, 4, 5], [0, 12]], dev)
    masks = [dict(size=[3, 4], counts=[3, 4, 5]), dict(size=[3, 4], counts=[0, 12])]
    for bad in ([0, 0], [0, 2], [1, 2], [-1, 0], [0], [0, 1, 2], [0.0, 1.0]):
        with pytest.raises(ValueError, match='permutation|entries'):
            rle.flatten_runs(counts, n, (3, 4), bad)
        with pytest.raises(ValueError, match='permutation|entries'):
            apis.flatten_masks(masks, order=bad, device=dev)
    for bad in ([float('nan'), 0.5], torch.tensor([0.5, float('nan')])):
        with pytest.raises(ValueError, match='NaN'):
            apis.flatten_masks(masks, scores=bad, device=dev)
    with pytest.raises(ValueError, match='needs scores'):
        apis.flatten_masks(masks, device=dev)
    with pytest.raises(ValueError, match='order'):
        apis.flatten_masks(masks, scores=[1, 2], order='size', device=dev)
    for bad in (-0.1, 1.5, float('nan'), float('inf'), True, None, '0.5'):
        with pytest.raises(ValueError, match='min_ratio'):
            apis.flatten_masks(masks, scores=[1, 2], min_ratio=bad, device=dev)
        with pytest.raises(ValueError, match='min_ratio'):
            rle.flatten_runs(counts, n, (3, 4), [0, 1], bad)
    with pytest.raises(ValueError, match='mask form'):
        apis.flatten_masks(masks, scores=[1, 2], form='bits', device=dev)
    # a label map over the limit (4 bytes per pixel), in the message style of the dense masks
    monkeypatch.setattr(large_image, 'DENSE_MASK_LIMIT_BYTES', 47)
    with pytest.raises(ValueError, match='needs 48 bytes .limit large_image.DENSE_MASK_LIMIT_BYTES = 47'):
        apis.masks_to_label_map(masks, scores=[1, 2], device=dev)
    monkeypatch.setattr(large_image, 'DENSE_MASK_LIMIT_BYTES', 48)
    assert apis.masks_to_label_map(masks, scores=[2, 1], device=dev).cpu().numpy().T.reshape(-1).tolist() == [2] * 3 + [1] * 4 + [2] * 5
    monkeypatch.undo()
    # H * W >= 2^31
    big = [dict(size=[65536, 32768], counts=[2 ** 31 - 1, 1])]
    for fn in (lambda: ops.rle_flatten(counts, n, 65536, 32768, rank_tensor([0, 1], dev)),
               lambda: ops.rle_label_map(counts, n, 46341, 46341),
               lambda: apis.flatten_masks(big, order=[0], device=dev),
               lambda: apis.masks_to_label_map(big, order=[0], device=dev)):
        with pytest.raises(ValueError, match='32-bit'):
            fn()
    with pytest.raises(ValueError, match='rank must be int32'):
        ops.rle_flatten(counts, n, 3, 4, torch.tensor([0, 1]).to(dev))
    with pytest.raises(ValueError, match='ids'):
        ops.rle_label_map(counts, n, 3, 4, torch.tensor([1, 2, 3], dtype=torch.int32).to(dev))
    with pytest.raises(ValueError, match='empty list'):
        apis.masks_to_label_map([], device=dev)
    # the entry points themselves, without a launch that reads anything
    p = counts.data_ptr()
    BIG = _lib.CONST['RSP_RUN_PIECES_MAX_PIECES'] + 1
    cols = lambda *a: lib.rsp_run_flatten_columns(*a, 0)                             # noqa: E731
    assert cols(p, p, 1, 65536, 32768, p, p) == EINVAL                              # H * W >= 2^31
    assert cols(p, p, BIG, 3, 4, p, p) == EINVAL and cols(p, p, -1, 3, 4, p, p) == EINVAL
    assert cols(0, p, 1, 3, 4, p, p) == EINVAL and cols(p, 0, 1, 3, 4, p, p) == EINVAL
    assert cols(p, p, 1, 3, 4, 0, p) == EINVAL and cols(p, p, 1, 3, 4, p, 0) == EINVAL
    assert cols(p, p, 1, 0, 4, p, p) == EINVAL
    cnt = lambda *a: lib.rsp_run_flatten_count(*a, 0)                                # noqa: E731
    assert cnt(p, p, p, p, p, 0, 1, 3, 4, 0) == OK and cnt(p, p, p, p, p, 1, 0, 3, 4, 0) == OK      # nothing to do
    assert cnt(p, p, p, p, p, 1, -1, 3, 4, p) == EINVAL                             # k < 0
    assert cnt(p, p, p, p, p, BIG, 1, 3, 4, p) == EINVAL
    assert cnt(p, p, p, p, p, 1, 1, 65536, 32768, p) == EINVAL
    for hole in range(5):
        a = [p] * 5
        a[hole] = 0
        assert cnt(*a, 1, 1, 3, 4, p) == EINVAL
    assert cnt(p, p, p, p, p, 1, 1, 3, 4, 0) == EINVAL
    wr = lambda *a: lib.rsp_run_flatten_write(*a, 0)                                 # noqa: E731
    assert wr(p, p, p, p, p, 1, 1, 3, 4, p, 0, p, p) == OK
    assert wr(p, p, p, p, p, 1, 1, 3, 4, p, -1, p, p) == EINVAL and wr(p, p, p, p, p, 1, 1, 3, 4, p, 2 ** 31, p, p) == EINVAL
    assert wr(p, p, p, p, p, 1, 1, 3, 4, 0, 1, p, p) == EINVAL and wr(p, p, p, p, p, 1, 1, 3, 4, p, 1, 0, p) == EINVAL
    assert wr(p, p, p, p, p, 1, 1, 3, 4, p, 1, p, 0) == EINVAL and wr(p, p, p, p, p, 1, -1, 3, 4, p, 1, p, p) == EINVAL
    assert wr(p, p, p, p, p, BIG, 1, 3, 4, p, 1, p, p) == EINVAL
    paint = lambda *a: lib.rsp_run_flatten_paint(*a, 0)                              # noqa: E731
    assert paint(p, p, 1, p, 1, 3, 4, 0) == EINVAL and paint(p, p, 1, p, -1, 3, 4, p) == EINVAL
    assert paint(0, p, 1, p, 1, 3, 4, p) == EINVAL and paint(p, 0, 1, p, 1, 3, 4, p) == EINVAL
    assert paint(p, p, 1, 0, 1, 3, 4, p) == EINVAL and paint(p, p, -1, p, 1, 3, 4, p) == EINVAL
    assert paint(p, p, 1, p, 1, 65536, 32768, p) == EINVAL


# --------------------------------------------------------------------------------------------------------------- integration
def check_scene_pair(dev, plain, flat, region, overlapping=True):
    """pred_instances of inference_large_image without and with flatten='score' (masks='rle', the same other arguments): K,
    boxes, scores and labels are the same; no two flattened instances share a pixel (apis.mask_iou exactly 0 off the
    diagonal); flatten_kept / flatten_area say what the masks hold; without region cleaning the result is apis.flatten_masks
    of the plain masks (with it, cleaning comes after the flatten here and before it there) -> K"""
    from rsprompter_amd import apis, ops, rle
    K = len(plain.scores)
    assert len(flat.scores) == K and len(flat.masks) == K and len(plain.masks) == K
    for key in ('bboxes', 'scores', 'labels'):
        assert torch.equal(getattr(plain, key), getattr(flat, key))
    assert 'flatten_kept' not in plain and 'flatten_area' not in plain
    assert flat.flatten_kept.dtype == torch.bool and tuple(flat.flatten_kept.shape) == (K,)
    assert flat.flatten_area.dtype == torch.int32 and tuple(flat.flatten_area.shape) == (K, 2)
    if K == 0:
        return 0
    off = ~np.eye(K, dtype=bool)
    iou = apis.mask_iou(flat.masks, flat.masks, device=dev).cpu().numpy()
    assert (iou[off] == 0).all(), int((iou[off] != 0).sum())
    if overlapping:                                                      # the layer was not planar before
        assert (apis.mask_iou(plain.masks, plain.masks, device=dev).cpu().numpy()[off] > 0).any()
    c, n, size, _ = rle.masks_to_runs(flat.masks, dev, 'test')
    assert torch.equal(ops.rle_bbox(c, n, *size)[1], flat.flatten_area[:, 1])
    assert torch.equal(flat.flatten_kept, flat.flatten_area[:, 1] > 0)
    if region == 0:
        again, info = apis.flatten_masks(plain.masks, scores=plain.scores, device=dev)
        assert [m['counts'] for m in again] == [m['counts'] for m in flat.masks]
        assert torch.equal(info['kept'], flat.flatten_kept)
        assert torch.equal(torch.stack([info['area_before'], info['area_after']], 1), flat.flatten_area)
        c0, n0, _, _ = rle.masks_to_runs(plain.masks, dev, 'test')
        assert torch.equal(ops.rle_bbox(c0, n0, *size)[1], flat.flatten_area[:, 0])
        want = fref.flatten(_dense_of(plain.masks, 'strings', *size), fref.rank_of_scores(plain.scores.cpu().numpy())) \
            if size[0] * size[1] * K <= 1 << 22 else None
        if want is not None:                                             # small scenes: the numpy oracle as well
            assert np.array_equal(_dense_of(flat.masks, 'strings', *size), want)
    return K


def check_pipeline(li, dev, model, merge, region):
    """inference_large_image around a stub detector on a 45 x 70 scene of 32 x 32 tiles: check_scene_pair, the area order,
    min_ratio, polygons whose ring areas sum to the union, and the refusals that come before the first tile -> K"""
    scene = np.random.default_rng(16).integers(0, 256, (45, 70, 3)).astype(np.uint8)
    kw = dict(patch_size=32, batch_size=2, merge_iou_thr=0.25, merge_nms_type=merge, min_mask_region_area=region)
    if merge == 'seam_mask':
        kw['seam_iou_thr'] = 0.3
    plain = li.inference_large_image(model, scene, **kw).pred_instances
    flat = li.inference_large_image(model, scene, flatten='score', **kw).pred_instances
    K = check_scene_pair(dev, plain, flat, region)
    from rsprompter_amd import apis
    dense = _dense_of(plain.masks, 'strings', 45, 70)
    union = int(dense.any(0).sum())
    for order in ('score', 'area'):
        rings = li.inference_large_image(model, scene, masks='polygons', flatten=order, **kw).pred_instances
        area2 = sum(int(a2) for inst in rings.masks for _, _, a2 in inst)
        assert area2 == 2 * int(rings.flatten_area[:, 1].sum())
        if region == 0:
            assert area2 == 2 * union                                    # every covered pixel once, holes negative
    if region == 0:
        by_area = li.inference_large_image(model, scene, flatten='area', **kw).pred_instances
        want = fref.flatten(dense, fref.rank_of_areas(dense))
        assert np.array_equal(_dense_of(by_area.masks, 'strings', 45, 70), want)
        thin = li.inference_large_image(model, scene, flatten='score', flatten_min_ratio=0.5, **kw).pred_instances
        part = fref.flatten(dense, fref.rank_of_scores(plain.scores.cpu().numpy()))
        want, kept = fref.apply_min_ratio(dense, part, 0.5)
        assert np.array_equal(_dense_of(thin.masks, 'strings', 45, 70), want) and thin.flatten_kept.cpu().tolist() == kept.tolist()
        assert not kept.all() and kept.any()
    return K
