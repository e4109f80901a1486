"""Bodies of the panoptic-quality tests (csrc/panoptic_quality.hip, ops.pq_image / pq_reduce), shared by tests/test_pq_cpu.py
(the lane-level emulator) and tests/test_gpu_pq.py (the device); each takes (ops, device).  The reference is tests/_pq_ref.py:
two numpy forms that must agree.  Every comparison is ==, the doubles included: counts are integers, an IoU is one IEEE
division of integers and the sums have a fixed order.

Classes of the generated and hand-checked cases: labels 0, 1, 2 things, 3 stuff, num_classes = 4 (so 4 is void); a thing's
id is label + 1000 * instance, the stuff id is 3."""
import numpy as np
import pytest
import torch

import _pq_ref as pr

NC = 4
CATS = {0: dict(isthing=1), 1: dict(isthing=1), 2: dict(isthing=1), 3: dict(isthing=0)}
V = NC                                  # a void pixel of a prediction
# (H, W, segments a side): 1 x 1; 3 x 5; W % 4 = 1, 2, 3; 75 x 110 = 8250 pixels = two blocks of 256 strips of 16 and a third
# with three whole strips and one of 10 pixels
GEN_SHAPES = ((1, 1, 1), (3, 5, 3), (37, 53, 12), (5, 6, 4), (9, 7, 5), (75, 110, 40))
NOISE_SHAPE = (37, 53, 40)


def seg(id, cat, crowd=0, area=None):
    return dict(id=id, category_id=cat, iscrowd=crowd, area=area)


def _cells(H, W, sy, sx):
    out = np.empty((H, W), dtype=np.int64)
    xs = np.arange(W)[None, :, None]
    for y0 in range(0, H, 64):
        ys = np.arange(y0, min(y0 + 64, H))[:, None, None]
        out[y0:y0 + 64] = ((ys - sy) ** 2 + (xs - sx) ** 2).argmin(-1)
    return out


def generate(H, W, n, seed, noise=False):
    """(pan, gt, segments): nearest-seed cells (or per-pixel noise: every pixel a new run) with, on the gt side, void and
    unlisted cells, crowd segments, JSON order shuffled, ids up to 2^24 and listed areas on even seeds; on the predicted
    side the gt's seeds moved by a pixel, labels mostly the gt's, void cells with and without an instance part, one shared
    stuff id"""
    rng = np.random.RandomState(seed)
    sy, sx = rng.randint(0, H, n), rng.randint(0, W, n)
    if noise:
        gcell, pcell = rng.randint(0, n, (H, W)), rng.randint(0, n, (H, W))
    else:
        gcell = _cells(H, W, sy, sx)
        pcell = _cells(H, W, sy + rng.randint(-1, 2, n), sx + rng.randint(-1, 2, n))
    gid = rng.choice(np.arange(1, 1 << 24), size=n, replace=False)
    gid[: n // 2] = rng.choice(np.arange(1, 4000), size=n // 2, replace=False)
    cat = rng.randint(0, NC, n)
    role = np.arange(n) % 7                                 # 5: VOID, 6: unlisted
    gt_of_cell = np.where(role == 5, 0, gid)
    gt = gt_of_cell[gcell]
    segments = [seg(int(gid[k]), int(cat[k]), int(k % 5 == 2 and cat[k] < 3)) for k in range(n) if role[k] < 5 or n < 3]
    if n < 3:
        gt = gid[gcell]
    segments = [segments[k] for k in rng.permutation(len(segments))]
    if seed % 2 == 0:
        for s in segments:
            s['area'] = int((gt == s['id']).sum())
    label = np.where(rng.rand(n) < 0.2, rng.randint(0, NC, n), cat)
    pid = np.where(label == 3, 3, label + 1000 * (np.arange(n) + 1))
    pid = np.where(np.arange(n) % 6 == 3, V + 1000 * (np.arange(n) % 2) * (np.arange(n) + 1), pid)
    return pid[pcell].astype(np.int32), gt.astype(np.int64), segments


def to_host(row, cats=CATS):
    """a row of ops.pq_image as the reference's result"""
    n = int(row['n_pred'].cpu())
    cat_ids = list(cats)
    tp, fp, fn, iou = (row[k].cpu().tolist() for k in ('tp', 'fp', 'fn', 'iou'))
    assert row['iou'].dtype == torch.float64 and all(row[k].dtype == torch.int32 for k in ('tp', 'fp', 'fn', 'status', 'n_pred'))
    ids, pc, ar = (row[k].cpu().tolist() for k in ('pred_ids', 'pred_cat', 'pred_area'))
    assert ids[n:] == [-1] * (len(ids) - n) and pc[n:] == [-1] * (len(ids) - n) and ar[n:] == [0] * (len(ids) - n)
    return dict(stat={c: [tp[i], fp[i], fn[i], iou[i]] for i, c in enumerate(cat_ids)}, status=int(row['status'].cpu()),
                segments=[(ids[k], cat_ids[pc[k]] if pc[k] >= 0 else None, ar[k]) for k in range(n)])


def run(ops, dev, pan, gt, segments, cats=CATS, nc=NC, ign=None, l2c=None, rgb=False):
    pan = torch.as_tensor(np.asarray(pan), dtype=torch.int32).contiguous().to(dev)
    g = torch.from_numpy(pr.id2rgb(gt)).contiguous() if rgb else torch.as_tensor(np.asarray(gt), dtype=torch.int32).contiguous()
    return ops.pq_image(pan, g.to(dev), segments, cats, nc, ignore_index=ign, label2cat=l2c)


def reference(pan, gt, segments, cats=CATS, nc=NC, ign=None, l2c=None):
    """both forms of the reference, asserted equal"""
    a = pr.image_loop(pan, gt, segments, list(cats), nc, ign, l2c)
    b = pr.image_arrays(pan, gt, segments, list(cats), nc, ign, l2c)
    assert a == b, (a, b)
    return a


def check(ops, dev, pan, gt, segments, what, **kw):
    """the id form and the rgb form of the gt give the reference, ==; returns the reference's result"""
    want = reference(pan, gt, segments, **kw)
    for rgb in (False, True):
        got = to_host(run(ops, dev, pan, gt, segments, rgb=rgb, **kw), kw.get('cats', CATS))
        assert got['status'] == 0, (what, rgb, got['status'])
        assert got['segments'] == want['segments'], (what, rgb, 'segments')
        assert got['stat'] == want['stat'], (what, rgb, got['stat'], want['stat'])
    return want


# ------------------------------------------------------------------------------------------------------------- generated
def check_generated(ops, dev, shape, seed=0):
    H, W, n = shape
    pan, gt, segments = generate(H, W, n, seed + 31 * H + W)
    want = check(ops, dev, pan, gt, segments, shape)
    if H * W >= 1000:                                       # the case means something: all four outcomes occur
        tot = [sum(want['stat'][c][k] for c in CATS) for k in range(3)]
        assert min(tot) > 0, tot


def check_noise(ops, dev):
    H, W, n = NOISE_SHAPE
    pan, gt, segments = generate(H, W, n, 7, noise=True)
    assert (np.diff(pan, axis=1) != 0).mean() > 0.9         # nearly every pixel starts a run
    check(ops, dev, pan, gt, segments, 'noise')


# ---------------------------------------------------------------------------------------------------------- hand-checked
def _stat(tp=(), fp=(), fn=(), iou=()):
    s = {c: [0, 0, 0, 0.0] for c in CATS}
    for k, d in enumerate((tp, fp, fn, iou)):
        for c, v in dict(d).items():
            s[c][k] = v
    return s


def check_iou_half_is_no_match(ops, dev):
    """gt 1 {0, 1, 2} x pred 1000 {1, 2, 3}: 2 / 4 = 0.5 exactly, no TP; gt 2 {4..7} x pred 1001 {5..8}: 3 / 5, a TP"""
    gt = [[1, 1, 1, 9, 2, 2, 2, 2, 3, 3]]
    pan = [[V, 1000, 1000, 1000, V, 1001, 1001, 1001, 1001, V]]
    want = check(ops, dev, pan, gt, [seg(1, 0), seg(2, 1), seg(3, 2), seg(9, 3)], 'half')
    assert want['stat'] == _stat(tp={1: 1}, fp={0: 1}, fn={0: 1, 2: 1, 3: 1}, iou={1: 3 / 5})


def check_void_overlap_decides(ops, dev):
    """pred 1000 has 2 of its 4 pixels on gt 1 (3 pixels) and 2 on VOID: 2 / (4 + 3 - 2 - 2) = 2 / 3 is a TP; without the
    void term it would be 2 / 5"""
    want = check(ops, dev, [[V, 1000, 1000, 1000, 1000, V]], [[1, 1, 1, 0, 0, 0]], [seg(1, 0)], 'void overlap')
    assert want['stat'] == _stat(tp={0: 1}, iou={0: 2 / 3})


def check_fp_ratio_half_is_fp(ops, dev):
    """pred 1000: 2 of 4 pixels on VOID = 0.5 exactly, an FP; pred 1001: 2 of 3, ignored; gt 5 has no pixel: an FN"""
    want = check(ops, dev, [[1000] * 4 + [1001] * 3], [[0, 0, 7, 7, 0, 0, 7]], [seg(5, 2)], 'fp ratio')
    assert want['stat'] == _stat(fp={0: 1}, fn={2: 1})


def check_last_crowd_in_json_order(ops, dev):
    """crowd segments 20 and 10 of category 0; pred 1000 lies 3 / 4 on gt 10, pred 2000 only 1 / 4 on gt 20 (both 0 on VOID).
    JSON order 20, 30, 10: crowd_of[0] = 10 (the last; also the lowest id, but not the first) -- 1000 is ignored, 2000 an FP.
    JSON order 10, 30, 20: crowd_of[0] = 20 (the last; neither the first nor the lowest id) -- 1000 has nothing on gt 20 and
    2000 a quarter: two FPs.  A first-crowd rule gives 2 and 1, a lowest-id rule 1 and 1.  Crowds are no FN; gt 30 is"""
    gt = [[10, 10, 10, 30, 20, 30, 30, 30]]
    pan = [[1000] * 4 + [2000] * 4]
    want = check(ops, dev, pan, gt, [seg(20, 0, 1), seg(30, 1), seg(10, 0, 1)], 'crowd')
    assert want['stat'] == _stat(fp={0: 1}, fn={1: 1})
    flipped = check(ops, dev, pan, gt, [seg(10, 0, 1), seg(30, 1), seg(20, 0, 1)], 'crowd flipped')
    assert flipped['stat'] == _stat(fp={0: 2}, fn={1: 1}) and flipped['segments'] == want['segments']


def check_unlisted_gt_adds_to_area_only(ops, dev):
    """pred 1000 = 3 pixels of gt 1 + 2 of the unlisted gt id 99: 3 / (5 + 3 - 3) = 3 / 5 (as VOID or as nothing: 1.0)"""
    want = check(ops, dev, [[1000] * 5 + [V]], [[1, 1, 1, 99, 99, 0]], [seg(1, 0)], 'unlisted')
    assert want['stat'] == _stat(tp={0: 1}, iou={0: 3 / 5}) and want['segments'] == [(1000, 0, 5)]


def check_gt_without_pixel_is_fn(ops, dev):
    want = check(ops, dev, [[1001, 1001]], [[4, 4]], [seg(4, 1), seg(77, 1), seg(78, 3, area=12)], 'absent gt')
    assert want['stat'] == _stat(tp={1: 1}, fn={1: 1, 3: 1}, iou={1: 1.0})


def check_all_void_and_no_gt(ops, dev):
    """P = 0: every gt segment an FN; G = 0: predictions over unlisted ids are FPs, over VOID they are ignored"""
    want = check(ops, dev, [[V, V + 1000, V]], [[1, 1, 2]], [seg(1, 0), seg(2, 3)], 'P = 0')
    assert want['stat'] == _stat(fn={0: 1, 3: 1}) and want['segments'] == []
    want = check(ops, dev, [[1000, 1000, 3, 2002]], [[8, 8, 0, 8]], [], 'G = 0')
    assert want['stat'] == _stat(fp={0: 1, 2: 1}) and want['segments'] == [(3, 3, 1), (1000, 0, 2), (2002, 2, 1)]
    want = check(ops, dev, [[V]], [[0]], [], 'nothing')
    assert want['stat'] == _stat()


def check_word_edge_ids(ops, dev):
    """predicted ids at the edges of the bitmap's words and at its end"""
    ids = [31, 32, 63, 64, 1031, 2047, 2048, ops.PQ_MAX_PRED_ID - 1]
    cats = {c: dict(isthing=1) for c in range(200)}
    gt = [list(range(1, len(ids) + 1))]
    segments = [seg(k + 1, i % 1000) for k, i in enumerate(ids)]
    want = check(ops, dev, [ids], gt, segments, 'word edges', cats=cats, nc=200)
    assert [s[0] for s in want['segments']] == ids and sum(v[0] for v in want['stat'].values()) == len(ids)
    assert want['stat'][31] == [2, 0, 0, 2.0]               # 31 and 1031


def _distinct(P, W):
    """a map of P pixels (padded with void to a multiple of W), every pixel its own thing segment"""
    k = np.arange(P)
    pan = np.concatenate([k % 3 + 1000 * (k + 1), np.full((-P) % W, V)]).reshape(-1, W)
    gt = np.repeat(np.arange(1, pan.size // 8 + 2), 8)[:pan.size].reshape(pan.shape)
    segments = [seg(int(i), int(i % 3)) for i in np.unique(gt)]
    return pan, gt, segments


def check_many_segments(ops, dev, P):
    """P = 70: more than a wave of columns; P = 1024: the limit"""
    pan, gt, segments = _distinct(P, 32)
    want = check(ops, dev, pan, gt, segments, P)
    assert len(want['segments']) == P


def check_too_many_segments(ops, dev):
    pan, gt, segments = _distinct(ops.PQ_MAX_SEGMENTS + 1, 25)
    row = run(ops, dev, pan, gt, segments)
    got = to_host(row)
    assert got['status'] == 1 and got['segments'] == [] and got['stat'] == _stat()
    # ... and the raise: the row through the reduce and the one host read, as compute_metrics does it
    from rsprompter_amd.evaluation import pq_stat_from_packed
    good = run(ops, dev, [[1000]], [[1]], [seg(1, 0)])
    with pytest.raises(RuntimeError, match=r"'second'.*too_many_segments"):
        pq_stat_from_packed(ops.pq_reduce([good, row])['packed'], list(CATS), ['first', 'second'])


def check_ignore_index(ops, dev):
    """ignore_index = 2: label 2 is void next to label 4, with and without an instance part"""
    pan = [[2, 3002, V, 1000, 1000, 1001]]
    gt = [[1, 1, 1, 2, 2, 3]]
    segments = [seg(1, 2), seg(2, 0), seg(3, 1)]
    want = check(ops, dev, pan, gt, segments, 'ignore_index', ign=2)
    assert want['stat'] == _stat(tp={0: 1, 1: 1}, fn={2: 1}, iou={0: 1.0, 1: 1.0}) and len(want['segments']) == 2
    other = check(ops, dev, pan, gt, segments, 'default ignore_index')
    assert len(other['segments']) == 4 and other['stat'][2][:3] == [0, 2, 1]


def check_label2cat(ops, dev):
    """category ids 7, 11, 20 for labels 0, 1, 2 and a JSON category 33 that no label maps to"""
    cats = {7: dict(isthing=1), 33: dict(isthing=1), 11: dict(isthing=1), 20: dict(isthing=0)}
    l2c = {0: 7, 1: 11, 2: 20}
    pan = [[1000, 1000, 2, 2, 1001, 3]]
    gt = [[5, 5, 6, 6, 7, 8]]
    want = check(ops, dev, pan, gt, [seg(8, 33), seg(7, 11), seg(6, 20), seg(5, 7)], 'label2cat', cats=cats, nc=3, l2c=l2c)
    assert want['stat'] == {7: [1, 0, 0, 1.0], 33: [0, 0, 1, 0.0], 11: [1, 0, 0, 1.0], 20: [1, 0, 0, 1.0]}
    assert want['segments'] == [(2, 20, 2), (1000, 7, 2), (1001, 11, 1)]


# ------------------------------------------------------------------------------------------------- the order of the sums
ORDER_FRACTIONS = (((7, 10), (3, 5), (2, 3)), ((5, 7), (7, 11), (5, 9)), ((7, 13), (7, 12), (4, 5)))


def order_images():
    """three one-row images with three TPs of category 0 each (ORDER_FRACTIONS, found by a search over small fractions).  A
    pair with IoU a / b is a gt of a pixels inside a prediction of b pixels whose other pixels lie on an unlisted gt id.
    Fraction k of an image sits k-th along the row with gt id first - 10 k, and the JSON lists 2, 0, 1.  So the three orders a
    per-image kernel could sum in start with three different pairs: ascending id (f2 + f1) + f0, the map's (f0 + f1) + f2,
    the JSON's (f2 + f0) + f1"""
    images = []
    for first, fracs in zip((100, 200, 300), ORDER_FRACTIONS):
        gt, pan, segments = [], [], []
        for k, (a, b) in enumerate(fracs):
            gid = first - 10 * k
            gt += [gid] * a + [999] * (b - a)
            pan += [1000 * (k + 1)] * b
            segments.append(seg(gid, 0))
        images.append(([pan], [gt], [segments[2], segments[0], segments[1]]))
    return images


def order_sums():
    """per image the sums of category 0 in ascending-id, map and JSON order, from the fractions alone; and the totals of the
    ascending-id sums over the images in processing order and in the orders that start with another pair of images"""
    per_image = []
    for fracs in ORDER_FRACTIONS:
        f = [a / b for a, b in fracs]
        per_image.append(dict(ascending=(f[2] + f[1]) + f[0], map=(f[0] + f[1]) + f[2], json=(f[2] + f[0]) + f[1]))
    s = [p['ascending'] for p in per_image]
    totals = dict(processing=((0.0 + s[0]) + s[1]) + s[2], last_two_first=((0.0 + s[1]) + s[2]) + s[0],
                  outer_two_first=((0.0 + s[0]) + s[2]) + s[1])
    return per_image, totals


def check_sum_order(ops, dev):
    per_image, totals = order_sums()
    ims = [reference(*im) for im in order_images()]
    assert [im['stat'][0][3] for im in ims] == [p['ascending'] for p in per_image]
    rows = [run(ops, dev, *im) for im in order_images()]
    for row, want in zip(rows, ims):
        assert to_host(row)['stat'] == want['stat']         # within an image: ascending gt id
    red = ops.pq_reduce(rows)
    assert red['iou'].dtype == torch.float64 and red['iou'].cpu().tolist()[0] == totals['processing']
    assert pr.add_stats(ims, list(CATS))[0][3] == totals['processing']
    assert red['tp'].cpu().tolist() == [9, 0, 0, 0] and red['status'].cpu().tolist() == [0, 0, 0]


def check_reduce_three_images(ops, dev):
    """three generated images reduced in order, one read of `packed`"""
    ims = [generate(37, 53, 12, s) for s in (3, 4, 5)]
    want = pr.add_stats([reference(*im) for im in ims], list(CATS))
    red = ops.pq_reduce([run(ops, dev, *im, rgb=(k == 1)) for k, im in enumerate(ims)])
    packed = red['packed'].cpu().numpy()
    n = len(CATS)
    assert packed.shape == (4 * n + 3,) and packed[4 * n:].tolist() == [0, 0, 0]
    got = {c: [int(packed[i]), int(packed[n + i]), int(packed[2 * n + i]), float(packed[3 * n:4 * n].view(np.float64)[i])]
           for i, c in enumerate(CATS)}
    assert got == want
    assert sum(v[0] for v in want.values()) > 0


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(ops, dev, other_dev):
    pan = torch.full((4, 6), 1000, dtype=torch.int32, device=dev)
    gt = torch.ones((4, 6), dtype=torch.int32, device=dev)
    ok = [seg(1, 0)]
    bad_calls = dict(
        sizes=lambda: ops.pq_image(pan, gt[:, :5].contiguous(), ok, CATS, NC),
        rgb_sizes=lambda: ops.pq_image(pan, torch.zeros((6, 4, 3), dtype=torch.uint8, device=dev), ok, CATS, NC),
        duplicate=lambda: ops.pq_image(pan, gt, [seg(1, 0), seg(1, 1)], CATS, NC),
        gt_id_zero=lambda: ops.pq_image(pan, gt, [seg(0, 0)], CATS, NC),
        category=lambda: ops.pq_image(pan, gt, ok, CATS, NC, label2cat={0: 0, 1: 9}),
        too_many_gt=lambda: ops.pq_image(pan, gt, [seg(k + 1, 0) for k in range(ops.PQ_MAX_SEGMENTS + 1)], CATS, NC),
        too_many_cats=lambda: ops.pq_image(pan, gt, ok, list(range(ops.PQ_MAX_CATEGORIES + 1)), NC),
        no_cats=lambda: ops.pq_image(pan, gt, ok, [], NC),
        dtype=lambda: ops.pq_image(pan.long(), gt, ok, CATS, NC),
        gt_dtype=lambda: ops.pq_image(pan, gt.float(), ok, CATS, NC),
        rank=lambda: ops.pq_image(pan[None], gt, ok, CATS, NC),
        strided=lambda: ops.pq_image(pan.t(), gt.t().contiguous(), ok, CATS, NC),
        misaligned=lambda: ops.pq_image(torch.zeros(25, dtype=torch.int32, device=dev)[1:].view(4, 6), gt, ok, CATS, NC),
        area=lambda: ops.pq_image(pan, gt, [seg(1, 0, area=-3)], CATS, NC),
        device=lambda: ops.pq_image(pan, torch.ones((4, 6), dtype=torch.int32, device=other_dev), ok, CATS, NC),
        no_rows=lambda: ops.pq_reduce([]),
    )
    for name, call in bad_calls.items():
        with pytest.raises(ValueError):
            call()
    # what only the map can tell arrives as the row's status, and the row is zero
    for name, first, status in (('zero', 0, 4), ('negative', -5, 2), ('beyond', ops.PQ_MAX_PRED_ID, 2), ('label', 1007, 8)):
        p = pan.clone()
        p[2, 3] = first
        got = to_host(ops.pq_image(p, gt, ok, CATS, NC))
        assert got['status'] == status and got['stat'] == _stat() and got['segments'] == [], name
    got = to_host(ops.pq_image(pan, gt, [seg(1, 0, area=23)], CATS, NC))       # 24 pixels in the map
    assert got['status'] == 16 and got['stat'] == _stat()
    assert to_host(ops.pq_image(pan, gt, [seg(1, 0, area=24)], CATS, NC))['stat'] == _stat(tp={0: 1}, iou={0: 1.0})
    # the C entry points themselves
    lib = ops._lib.load()
    assert lib.rsp_pq_workspace_bytes(ops.PQ_MAX_SEGMENTS + 1) == -1 and lib.rsp_pq_workspace_bytes(0) > 0
    row = ops.pq_image(pan, gt, ok, CATS, NC)
    tab = torch.zeros(4 + 1000 + 4, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.rsp_pq_workspace_bytes(1), dtype=torch.uint8, device=dev)
    out = [row[k].data_ptr() for k in ('tp', 'fp', 'fn', 'iou', 'status', 'n_pred', 'pred_ids', 'pred_cat', 'pred_area')]

    def c_call(pred=pan.data_ptr(), rgb=0, ids=gt.data_ptr(), H=4, W=6, G=1, n_cat=4, w=ws.data_ptr()):
        return lib.rsp_pq_image(pred, rgb, ids, H, W, NC, NC, tab.data_ptr(), G, n_cat, w, *out, 0)
    assert c_call() == 0
    for kw in (dict(rgb=gt.data_ptr()), dict(ids=0), dict(H=1 << 16, W=1 << 15), dict(G=ops.PQ_MAX_SEGMENTS + 1), dict(G=-1),
               dict(n_cat=ops.PQ_MAX_CATEGORIES + 1), dict(n_cat=0), dict(pred=0), dict(w=0), dict(pred=pan.data_ptr() + 4),
               dict(ids=gt.data_ptr() + 4), dict(w=ws.data_ptr() + 8), dict(H=0)):
        assert c_call(**kw) == -1, kw


HAND_CHECKED = (check_iou_half_is_no_match, check_void_overlap_decides, check_fp_ratio_half_is_fp, check_last_crowd_in_json_order,
                check_unlisted_gt_adds_to_area_only, check_gt_without_pixel_is_fn, check_all_void_and_no_gt, check_word_edge_ids,
                check_too_many_segments, check_ignore_index, check_label2cat, check_sum_order, check_reduce_three_images)
