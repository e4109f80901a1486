"""Bodies of the detection-selection tests, in the style of tests/_sampler_props.py: the kernels of csrc/det.hip and
query_topk_kernel of csrc/query.hip decide which boxes every model returns, and each entry point is held here to ONE plain
restatement of the reference's lines at the places where a decision is cut.

    rsp_rpn_topk       rpn_head.py:193-212: sigmoid, stable descending sort, first nms_pre; natural order when n <= nms_pre
    rsp_rpn_decode     anchors + delta2bbox (delta_xywh_bbox_coder.py:264-361) + the min_bbox_size filter of _bbox_post_process
    rsp_bbox_post      bbox_head.py:525-571 + bbox_nms.py:40-76: softmax, per-class decode, > score_thr, * fp32(1 / scale_factor)
    rsp_batched_nms    mmcv batched_nms + nms: offset id * (max + 1) in fp32, stable order, IoU > thr   (also ops.nms_flat)
    rsp_query_topk     maskformer_fusion_head.py:149-162

Every restatement takes a dtype and a mutation switch.  dtype = float32 with every operation rounded on its own is the FP32
SEQUENCE: what the reference's eager code computes and what det.hip's header promises ("bit-for-bit in index space", "every
operation is its own fp32 rounding step").  dtype = float64 is the oracle of the exact tier and the yardstick of the tolerance
tier.  With a mutation the fp32 sequence is the stand-in of tests/test_kernel_props_selfcheck_cpu.py (FakeOps below).  The
restatements are plain torch / numpy on the CPU; nothing goes through `ops`, torch_ops_mock or a kernel.

Exact tier.  Dyadic anchors, deltas, means and stds with dw = dh = 0 (or dw so far below zero that the size vanishes beside the
centre); logits in {-100, -0.0, 0, 100}; softmax rows with j logits at 0 (or 100) and the rest 200 below, j a power of two;
integer boxes whose IoU is a short dyadic fraction.  Every fp32 operation of any correct evaluation order is exact, so the fp64
oracle is the kernel's answer bit for bit -- boxes, scores, ids, src, counts and order.  Each body first asserts, on the
reference alone, that the fp32 and fp64 restatements agree bit for bit.  One reading note: 1 / (1 + exp(100)) and
exp(-200) / j are 0 in every fp32 evaluation (the exponential overflows / underflows) and 3.7e-44 / 1.4e-87 in fp64, below
fp32's normal range; the oracle's scores below 2^-126 are read as 0 (`flush`), as _sampler_props does with its paste field.
An IoU equal to fp32(0.7) cannot be made exact in every order: fp32(0.7) = 11744051 / 2^24 with an odd numerator, so the union
is a multiple of 2^24 and area + area = union + inter is not an fp32 number.  The exact tier therefore cuts at 1/2, at
5/16 and at 717/1024; the cut at fp32(0.3), fp32(0.5) and fp32(0.7) itself is the sequence tier's threshold pool.

Sequence tier.  Non-dyadic inputs with no transcendental on the path (dw = dh = 0 in the decode, exact softmax rows, given
boxes and scores for the NMS).  The kernel must equal the fp32 sequence bit for bit; this is what guards -ffp-contract=off, the
rounding of id * (max + 1) and of box + offset, and the correctly rounded division.  Per case the body asserts on the reference
alone that the case discriminates: the fp64 restatement and every mutation named for the case differ from the fp32 sequence in
at least one output.  Softmax rows with 3, 5, 6, 7 ... maxima belong here too: exp(0) = 1 and expf(-200) = 0 are exact, so the score
is fp32(1 / j) if and only if the kernel's division is correctly rounded (the exact tier's 1 / 2^k comes out of any reciprocal).
gx +- gw * 0.5 has no contracted form that differs (a product by 1/2 is exact), so there is no such
mutation.

Tolerance tier.  expf in the decode, sigmoid, softmax, a real coder.  Value outputs: err <= max(F, 2 E32) (_sampler_props.Report).
Decisions may differ from the fp64 restatement only for candidates whose fp64 quantity lies within NEAR_* of a cut; each
NEAR_* is twice the largest fp32-from-fp64 distance of that quantity over the tier's cases, measured on the reference on the
CPU (tools of this module: `measure_near`), and each body re-measures its case and asserts 2 x distance <= the constant.

    NEAR_SCORE = 4e-7    measured: the fp32 sigmoid / softmax score is at most 1.94e-7 from the fp64 one (QUERY_TOL[0], 100
                         queries x 80 classes; BBOX_TOL[0] 1.91e-7, the sigmoid of RPN_TOL 8.8e-8); twice that is 3.9e-7
    NEAR_SIDE  = 1.8e-3  measured: a decoded side length is at most 8.73e-4 from the fp64 one (DECODE_TOL 'tol-no-clip', whose
                         sides reach 62.5 x 512 pixels; 'tol-real' 7.9e-5, 'tol-ctr' 4.3e-5); twice that is 1.75e-3
    NEAR_IOU   = 8e-6    measured: the IoU of two offset candidates, decode and offsets in fp32, is at most 3.73e-6 from the
                         all-fp64 one (BBOX_TOL[0], ten classes: coordinates up to 9 x 421; the others stay below 9e-7);
                         twice that is 7.5e-6

Seeds were chosen on the reference alone so that at most 2 candidates of a case are that near to a cut (none for the IoU and
for the order of the NMS, whose greedy walk would carry one flip to later rows); a body fails the CASE, not the kernel, when
that no longer holds.

tests/test_gpu_det_props.py runs these on the device, tests/test_det_props_cpu.py the census and a subset on the lane-level
emulator, tests/test_kernel_props_selfcheck_cpu.py the mutations."""
import collections
import functools
import math

import numpy as np
import torch

from _sampler_props import Report, _first_diff, case_id  # noqa: F401


class DetReport(Report):
    """the max(F, 2 E32) rule of _sampler_props.Report under this module's line prefix"""
    prefix = 'det'

F64, F32 = torch.float64, torch.float32
NEAR_SCORE = 4e-7
NEAR_SIDE = 1.8e-3
NEAR_IOU = 8e-6
TINY = 2.0 ** -126
IDS = (0, 1, 7, 79)


def _f32(v, dtype):
    """a host float as the kernel receives it (fp32), in the working dtype"""
    return torch.tensor(float(v), dtype=F32).to(dtype)


def _fma(a, b, c, dtype):
    """a * b + c with ONE rounding in fp32 (the product of two fp32 numbers is exact in fp64); the plain form in fp64"""
    if dtype == F64:
        return a * b + c
    return (a.double() * b.double() + c.double()).float()


def flush(x):
    """an fp64 score below fp32's normal range read as 0 (see the module docstring)"""
    return torch.where(x.abs() < TINY, torch.zeros_like(x), x)


def _below(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def _above(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def _same(got, want, what):
    got = got.cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    assert torch.equal(got, want), (what, _first_diff(got, want))


def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _softmax_fg(logits, mut=None):
    """[n, nc + 1] -> the softmax over nc + 1 with the sum taken column by column (the kernels' order)"""
    x = logits if mut == 'softmax_without_max' else logits - logits.max(-1, keepdim=True).values
    e = torch.exp(x)
    s = torch.zeros_like(e[:, 0])
    for j in range(e.shape[1]):
        s = s + e[:, j]
    if mut == 'division_by_truncated_reciprocal' and e.dtype == F32:        # e * rcp(s) with a reciprocal that is not rounded to nearest
        exact = 1.0 / s.double()
        r = exact.float()
        r = torch.where(r.double() > exact, torch.nextafter(r, torch.zeros_like(r)), r)
        return e * r[:, None]
    return e / s[:, None]


# ======================================================================================================================= NMS
NMS_MUTATIONS = ('iou_ge', 'iou_cross_multiplied', 'iou_fp64', 'offset_contracted', 'offset_unit_without_plus_one',
                 'max_over_capacity_rows', 'count_ignored', 'ties_by_index_descending', 'suppressed_box_suppresses',
                 'max_out_counts_suppressed', 'zero_area_suppressed')


def _offset_boxes(boxes, ids, n, dt, mut):
    """mmcv batched_nms: boxes[:n] + ids * (max + 1), each step rounded in `dt`; boxes is the whole capacity"""
    b = boxes.astype(dt)
    mx = (b if mut == 'max_over_capacity_rows' else b[:n]).max()
    unit = mx if mut == 'offset_unit_without_plus_one' else mx + dt(1)
    idf = ids[:n].astype(dt)
    if mut == 'offset_contracted' and dt == np.float32:
        return (idf.astype(np.float64)[:, None] * np.float64(unit) + b[:n].astype(np.float64)).astype(np.float32)
    return b[:n] + (idf * unit)[:, None]


def _suppressed(bi, rest, thr, dt, mut):
    """mmcv nms: the rows of `rest` that box `bi` suppresses; thr is the fp32 threshold in `dt`"""
    if mut == 'iou_fp64':
        bi, rest, thr = bi.astype(np.float64), rest.astype(np.float64), np.float64(thr)
        dt = np.float64
    w = np.maximum(dt(0), np.minimum(bi[2], rest[:, 2]) - np.maximum(bi[0], rest[:, 0]))
    h = np.maximum(dt(0), np.minimum(bi[3], rest[:, 3]) - np.maximum(bi[1], rest[:, 1]))
    inter = w * h
    ia = (bi[2] - bi[0]) * (bi[3] - bi[1])
    ja = (rest[:, 2] - rest[:, 0]) * (rest[:, 3] - rest[:, 1])
    union = ia + ja - inter
    if mut == 'iou_cross_multiplied':
        return inter > thr * union
    ovr = inter / union
    if mut == 'iou_ge':
        return ovr >= thr
    if mut == 'zero_area_suppressed':
        return ~(ovr <= thr)
    return ovr > thr                                                        # 0 / 0 is not > thr


def nms_keep(boxes, scores, ids, n, thr, max_out, dtype=F64, mut=None):
    """one image: numpy [cap, 4], [cap], [cap], the count -> the kept original positions in score order"""
    dt = np.float64 if dtype == F64 else np.float32
    if mut == 'count_ignored':
        n = boxes.shape[0]
    if n == 0:
        return []
    with np.errstate(all='ignore'):
        ob = _offset_boxes(boxes, ids, n, dt, mut)
        sc = scores[:n]
        if mut == 'ties_by_index_descending':
            order = (n - 1 - np.argsort(-sc[::-1], kind='stable'))
        else:
            order = np.argsort(-sc, kind='stable')
        s = ob[order]
        t = dt(np.float32(thr))
        dead = np.zeros(n, bool)
        keep, seen = [], 0
        for i in range(n):
            seen += 1
            if dead[i] and mut != 'suppressed_box_suppresses':
                continue
            if not dead[i]:
                keep.append(int(order[i]))
                if len(keep) >= max_out:
                    break
            if mut == 'max_out_counts_suppressed' and seen >= max_out:
                break
            if i + 1 < n:
                dead[i + 1:] |= _suppressed(s[i], s[i + 1:], t, dt, mut)
    return keep


def nms_ref(boxes, scores, ids, src, cnt, thr, max_out, dtype=F64, mut=None):
    """the outputs of ops.batched_nms: [B, max_out] rows gathered through the keep lists, 0 / -1 behind the count"""
    B = boxes.shape[0]
    ob = torch.zeros(B, max_out, 4, dtype=F32)
    os_ = torch.zeros(B, max_out, dtype=F32)
    oi = torch.full((B, max_out), -1, dtype=torch.int32)
    osrc = torch.full((B, max_out), -1, dtype=torch.int32)
    keep = torch.full((B, max_out), -1, dtype=torch.int32)
    count = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        k = nms_keep(boxes[b].numpy(), scores[b].numpy(), ids[b].numpy(), int(cnt[b]), thr, max_out, dtype, mut)
        kk = torch.tensor(k, dtype=torch.long)
        m = len(k)
        count[b] = m
        ob[b, :m], os_[b, :m], oi[b, :m], osrc[b, :m], keep[b, :m] = boxes[b][kk], scores[b][kk], ids[b][kk], src[b][kk], kk.int()
    return dict(boxes=ob, scores=os_, ids=oi, src=osrc, count=count, keep=keep)


def _nms_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in ('boxes', 'scores', 'ids', 'src', 'count', 'keep'))


def assert_nms_output(got, want, what):
    """every output of ops.batched_nms against a restatement; `keep` is defined up to the count"""
    _same(got['count'], want['count'], (what, 'count'))
    for key in ('boxes', 'scores', 'ids', 'src'):
        _same(got[key], want[key], (what, key))
    kg = got['keep'].cpu()
    for b in range(kg.shape[0]):
        m = int(want['count'][b])
        assert torch.equal(kg[b, :m], want['keep'][b, :m]), (what, 'keep', b)


class NmsCase:
    """name, tier ('exact' | 'seq'), the candidate buffers [B, cap, ...] + cnt [B], thr, max_out, and the mutations the case
    must show (asserted on the reference alone by the body)"""

    def __init__(self, name, tier, boxes, scores, ids, cnt, thr, max_out, kills=(), emu=True):
        B, cap = scores.shape
        self.name, self.tier, self.thr, self.max_out, self.kills, self.emu = name, tier, thr, max_out, tuple(kills), emu
        self.boxes, self.scores, self.ids = boxes.float().contiguous(), scores.float().contiguous(), ids.to(torch.int32).contiguous()
        self.cnt = torch.tensor(cnt, dtype=torch.int32)
        g = torch.Generator().manual_seed(cap)
        self.src = torch.stack([torch.randperm(cap, generator=g) for _ in range(B)]).to(torch.int32) + 1000    # not the position
        self.B, self.cap = B, cap

    def cand(self):
        return (self.boxes, self.scores, self.ids, self.src, self.cnt)

    def ref(self, dtype, mut=None):
        return nms_ref(self.boxes, self.scores, self.ids, self.src, self.cnt, self.thr, self.max_out, dtype, mut)


def _pack(images, cap=None, poison=True):
    """[(boxes [n, 4], scores [n], ids [n])] -> buffers [B, cap, ...] + counts; the rows behind a count are poisoned with 1e30
    coordinates, the top score and a large id: they must enter neither the max nor the sort"""
    cap = cap or max(b.shape[0] for b, _, _ in images) + 3
    B = len(images)
    boxes = torch.full((B, cap, 4), 1e30 if poison else 0.0)
    scores = torch.full((B, cap), 1e3 if poison else 0.0)
    ids = torch.full((B, cap), 5 if poison else 0, dtype=torch.int32)
    cnt = []
    for i, (b, s, d) in enumerate(images):
        n = b.shape[0]
        boxes[i, :n], scores[i, :n], ids[i, :n] = b, s, d.to(torch.int32)
        cnt.append(n)
    return boxes, scores, ids, cnt


def _nested_pairs(areas):
    """integer pairs (A, B) on rows of their own, B inside A: A is 1024 x 1, B is area x 1, so IoU = area / 1024 exactly"""
    boxes = []
    for i, area in enumerate(areas):
        y0 = 2.0 * i
        boxes += [[0.0, y0, 1024.0, y0 + 1], [0.0, y0, float(area), y0 + 1]]
    return torch.tensor(boxes, dtype=F32)


def _exact_threshold_image(num, g, n_pairs=24):
    """pairs with IoU exactly num / 1024 (strict >: both kept), 1 / 1024 above (suppressed) and below, every id of IDS"""
    boxes = _nested_pairs([num + (i % 3 - 1) for i in range(n_pairs)])
    n = boxes.shape[0]
    ids = torch.tensor([IDS[(i // 2) % 4] for i in range(n)])
    scores = torch.rand(n, generator=g).mul(64).floor() / 64 + 0.25         # dyadic, with ties
    scores[0::2] += 1.0                                                      # A before B
    perm = torch.randperm(n, generator=g)
    return boxes[perm], scores[perm], ids[perm]


def _chain_image(n, places, g, thr_gap=True):
    """n integer boxes, all kept but for the chains: A = [0, 10), B = [4, 14), C = [8, 18) (x; 10 high): IoU(A, B) = IoU(B, C)
    = 6/14 > 1/4 >= IoU(A, C) = 2/18 -- A suppresses B, B is dead and must not suppress C.  places: (pos A, pos B, pos C) in
    the sorted order.  The fillers are disjoint unit-spaced boxes on a grid; runs of equal scores straddle the 64-row blocks"""
    side = int(math.ceil(math.sqrt(n)))
    idx = torch.arange(n)
    x0, y0 = (idx % side) * 24.0, (idx // side) * 16.0
    boxes = torch.stack([x0, y0, x0 + 10, y0 + 10], 1)
    rank = torch.arange(n)                                                   # the sorted position of row i is rank[i]
    for a, b, c in places:
        base = boxes[a].clone()
        boxes[b] = base + torch.tensor([4.0, 0, 4.0, 0])
        boxes[c] = base + torch.tensor([8.0, 0, 8.0, 0])
    # scores fall in runs of 100 equal values (longer than a 64-row block): inside a run the index decides
    scores = 1.0 - (rank // 100).float() / 256
    ids = torch.zeros(n, dtype=torch.int32)
    return boxes, scores, ids


def _dup_image(n, g, nid=3):
    """integer boxes on a coarse grid with duplicates, dyadic scores with ties, zero-area boxes and identical twins"""
    xy = (torch.rand(n, 2, generator=g) * 6).floor() * 16
    wh = (torch.rand(n, 2, generator=g) * 3).floor() * 16 + 16
    boxes = torch.cat([xy, xy + wh], 1)
    scores = (torch.rand(n, generator=g) * 8).floor() / 8
    ids = torch.randint(0, nid, (n,), generator=g)
    if n >= 8:
        boxes[1] = torch.tensor([8.0, 8.0, 8.0, 24.0])                     # zero width
        boxes[3] = boxes[1]                                                  # ... twice: 0 / 0
        boxes[5] = torch.tensor([40.0, 40.0, 40.0, 40.0])                  # a point inside others
        boxes[7], scores[7], ids[7] = boxes[2], scores[2], ids[2]          # identical twins: the lower index survives
        ids[3] = ids[1]
        scores[3] = scores[1]
    return boxes, scores, ids


# -------------------------------------------------------------------------------------------------- the threshold pool
def _pair_decisions(ax, ay, w, h, dx, off32, off64, thr):
    """vectorised over pairs: A = (ax, ay, ax + w, ay + h), B = A shifted by dx, both moved by the id's offset.
    -> (fp32-sequence IoU, fp64 IoU of the fp64-offset boxes, inter and union of the fp32 sequence)"""
    def iou(dt, off):
        x1, y1, x2, y2 = (v.astype(dt) + off.astype(dt) for v in (ax, ay, ax + w, ay + h))
        u1, u2 = (ax + dx).astype(dt) + off.astype(dt), (ax + dx + w).astype(dt) + off.astype(dt)
        iw = np.maximum(dt(0), np.minimum(x2, u2) - np.maximum(x1, u1))
        ih = np.maximum(dt(0), y2 - y1)
        inter = iw * ih
        union = (x2 - x1) * (y2 - y1) + (u2 - u1) * (y2 - y1) - inter
        return inter / union, inter, union
    o32, i32, u32 = iou(np.float32, off32)
    o64, _, _ = iou(np.float64, off64)
    return o32, o64, i32, u32


@functools.lru_cache(maxsize=None)
def threshold_pool(thr, seed, n_pairs=64, origin=0.0, tries=8):
    """n_pairs disjoint pairs whose IoU sits on the cut (and eight that overlap by far): the shift of B is bisected to the threshold, then 81 neighbouring
    shifts (steps of one ulp of the offset coordinate) are scanned for one where the fp32 sequence and the fp64 IoU decide
    differently ('differ'), where the fp32 IoU equals fp32(thr) ('equal'), or where inter > thr * union decides differently
    ('cross'); a third of the pairs prefers each, and a pair tries up to `tries` geometries for its preference.
    The set's largest coordinate is origin + 1333.37 (a sentinel box), so that id * (max + 1) and box + offset both round.
    -> (boxes [2 (n + 8) + 1, 4], scores, ids), census {kind: [count per id]}"""
    rng = np.random.default_rng(seed)
    t32 = np.float32(thr)
    cols = 11
    top = origin + 1333.37
    cell = 1293.0 / cols
    n_cut, n_pairs = n_pairs, n_pairs + 8                                   # eight more pairs that overlap by far: suppressed for sure
    k = np.arange(n_pairs)[:, None].repeat(tries, 1)
    ids = np.array(IDS)[k % 4]
    shape = (n_pairs, tries)
    ax = (origin + (k % cols) * cell + rng.random(shape) * 10 + 3).astype(np.float32)
    ay = (origin + (k // cols) * cell + rng.random(shape) * 10 + 3).astype(np.float32)
    w = (rng.random(shape) * 30 + 30).astype(np.float32)
    h = (rng.random(shape) * 30 + 30).astype(np.float32)
    unit32 = np.float32(top) + np.float32(1)
    off32 = ids.astype(np.float32) * unit32
    off64 = ids.astype(np.float64) * (np.float64(np.float32(top)) + 1.0)
    lo, hi = np.zeros(shape, np.float64), w.astype(np.float64)
    for _ in range(50):                                                     # IoU falls with the shift
        mid = (lo + hi) / 2
        above = _pair_decisions(ax, ay, w, h, mid.astype(np.float32), off32, off64, thr)[0] > t32
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    dx0 = hi.astype(np.float32)
    far = np.abs(ax + dx0 + w + off32)
    ulp = np.nextafter(far, np.float32(np.inf)) - far                       # one ulp of the offset coordinate
    steps = np.arange(-40, 41, dtype=np.float32)
    b = lambda v: v[..., None].repeat(81, -1)
    dx = (b(dx0) + steps * b(ulp)).astype(np.float32)
    o32, o64, i32, u32 = _pair_decisions(b(ax), b(ay), b(w), b(h), dx, b(off32), b(off64), thr)
    ok = (dx > 0) & (dx < b(w))
    kinds = dict(differ=ok & ((o32 > t32) != (o64 > np.float64(t32))), equal=ok & (o32 == t32), cross=ok & ((i32 > t32 * u32) != (o32 > t32)))
    pick_t, pick_s = np.zeros(n_pairs, int), np.full(n_pairs, 40)
    census = {name: [0] * 4 for name in kinds}
    prefer = ('differ', 'equal', 'cross')
    for p in range(n_cut):
        for name in (prefer[(p // 4) % 3],) + prefer:
            hit = np.argwhere(kinds[name][p])
            if hit.size:
                pick_t[p], pick_s[p] = hit[np.argmin(np.abs(hit[:, 1] - 40))]
                break
        for name in kinds:
            census[name][p % 4] += int(kinds[name][p, pick_t[p], pick_s[p]])
    r = np.arange(n_pairs)
    ax, ay, w, h, d = ax[r, pick_t], ay[r, pick_t], w[r, pick_t], h[r, pick_t], dx[r, pick_t, pick_s]
    d[n_cut:] = w[n_cut:] * np.float32(0.03125)
    ids = ids[:, 0]
    A = np.stack([ax, ay, ax + w, ay + h], 1)
    Bx = np.stack([ax + d, ay, ax + d + w, ay + h], 1)
    boxes = np.concatenate([A, Bx, np.array([[top - 30, top - 30, top, top]], np.float32)]).astype(np.float32)
    assert float(boxes.max()) == float(np.float32(top))
    sc = rng.permutation(2 * n_pairs + 1).astype(np.float32) / 512 + 0.125
    sc[:n_pairs] += 1.0                                                     # every A before its B
    allids = np.concatenate([ids, ids, [0]])
    perm = rng.permutation(2 * n_pairs + 1)
    return (torch.from_numpy(boxes[perm]), torch.from_numpy(sc[perm]), torch.from_numpy(allids[perm].astype(np.int32))), census


POOL_THRESHOLDS = (0.3, 0.5, 0.7)
_SEQ_NMS_KILLS = ('iou_ge', 'iou_fp64', 'offset_contracted', 'max_over_capacity_rows', 'count_ignored')


@functools.lru_cache(maxsize=None)
def nms_cases():
    g = torch.Generator().manual_seed(5)
    cases = []
    # ---- exact tier: the cut at a short dyadic IoU, every id, poisoned rows behind the counts
    for name, num in (('half', 512), ('five-16ths', 320), ('717-1024ths', 717)):
        thr = num / 1024
        imgs = [_exact_threshold_image(num, g), _exact_threshold_image(num, g, n_pairs=17)]
        cases.append(NmsCase(f'cut-{name}', 'exact', *_pack(imgs), thr, 64, kills=('iou_ge', 'max_over_capacity_rows', 'count_ignored')))
    # ---- exact tier: degenerate boxes, twins, n in {0, 1, 63, 64, 65, 130}
    for na, nb in ((0, 130), (1, 65), (63, 64)):
        imgs = [_dup_image(na, g), _dup_image(nb, g)]
        cases.append(NmsCase(f'sizes-{na}-{nb}', 'exact', *_pack(imgs, cap=133), 0.5, 140,
                             kills=('zero_area_suppressed', 'ties_by_index_descending') if nb == 130 else ()))
    # ---- exact tier: chains and runs of equal scores; max_out mid-block, at a block end, beyond n
    places = ((3, 9, 20), (40, 70, 100), (50, 127, 128))
    img = _chain_image(300, places, g)
    for mo in (37, 63, 64, 128, 400):                                       # 63: reached on the last row of block 0 (row 9 is suppressed)
        cases.append(NmsCase(f'walk-300-max{mo}', 'exact', *_pack([img, _chain_image(131, places[:2], g)]), 0.25, mo,
                             kills=('suppressed_box_suppresses', 'max_out_counts_suppressed') if mo < 400 else ('suppressed_box_suppresses',)))
    big = _chain_image(4300, places + ((5, 4100, 4150), (4000, 4097, 4290)), g)
    cases.append(NmsCase('walk-4300', 'exact', *_pack([big, img], cap=4303), 0.25, 4303, kills=('suppressed_box_suppresses',), emu=False))
    # ---- sequence tier: the threshold pool, ids in IDS, fractional coordinates up to 1333
    for thr in POOL_THRESHOLDS:
        (p0, c0), (p1, c1) = threshold_pool(thr, 11), threshold_pool(thr, 12, 48)
        cross = sum(c0['cross']) + sum(c1['cross'])                         # none at 1/2: thr * union is exact there
        cases.append(NmsCase(f'pool-{thr}', 'seq', *_pack([p0, p1]), thr, 200,
                             kills=_SEQ_NMS_KILLS + (('iou_cross_multiplied',) if cross else ())))
    # ---- sequence tier: n in {63, 64, 65, 130} with the pool embedded: its sentinel (the largest coordinate) and its first rows
    (pb, ps, pi), _ = threshold_pool(0.7, 16, 64)
    top = int(pb.max(1).values.argmax())
    rows = [top] + [i for i in range(pb.shape[0]) if i != top]
    cut = lambda n: (pb[rows[:n]], ps[rows[:n]], pi[rows[:n]])
    for na, nb, kills in ((63, 64, ('iou_fp64',)), (65, 130, ('iou_fp64', 'offset_contracted'))):
        cases.append(NmsCase(f'pool-sizes-{na}-{nb}', 'seq', *_pack([cut(na), cut(nb)], cap=133), 0.7, 140, kills=kills))
    # ---- sequence tier: every coordinate below -1 (clip_border=False boxes): the unit is <= 0 and the classes overlap
    (neg, ps, pi), _ = threshold_pool(0.5, 13, 32, origin=-2800.0)
    assert float(neg.max()) < -1
    cases.append(NmsCase('negative-unit', 'seq', *_pack([(neg, ps, pi), (neg.flip(0), ps.flip(0), pi.flip(0))]), 0.5, 100,
                         kills=('offset_contracted', 'iou_fp64')))
    # ... and the same in the exact tier: the largest coordinate is -1.5, so the unit is -1/2 -- without the + 1 it is -3/2 and
    # the box of id 2 moves two pixels further: IoU 64/136 instead of 60/140 on either side of 7/16
    nb = torch.tensor([[-20.0, -20, -10, -10], [-15.0, -19, -5, -9], [-3.0, -3, -1.5, -1.5], [-40.0, -40, -30, -30], [-36.0, -39, -26, -29]])
    ns, ni = torch.tensor([0.875, 0.75, 0.5, 0.625, 0.25]), torch.tensor([0, 2, 1, 0, 2])
    cases.append(NmsCase('negative-unit-exact', 'exact', *_pack([(nb, ns, ni), (nb.flip(0), ns.flip(0), ni.flip(0))]), 0.4375, 8,
                         kills=('offset_unit_without_plus_one',)))
    # ---- sequence tier: the LDS-to-memory sort switch and the 4-to-32-word reduce switch, the pool embedded
    for cap in (16384, 16385):
        (p0, _), (p1, _) = threshold_pool(0.7, 14, 32), threshold_pool(0.7, 15, 64)
        cases.append(NmsCase(f'pool-cap{cap}', 'seq', *_pack([p0, p1], cap=cap), 0.7, 150, kills=('iou_fp64', 'max_over_capacity_rows'),
                             emu=False))
    return tuple(cases)


def nms_case(name):
    return next(c for c in nms_cases() if c.name == name)


def assert_nms_case_holds(case):
    """on the reference alone: an exact case is exact, a sequence case discriminates, the named mutations show -> the oracle"""
    r32, r64 = case.ref(F32), case.ref(F64)
    if case.tier == 'exact':
        assert _nms_equal(r32, r64), ('not an exact case: fp32 and fp64 differ', case.name)
    else:
        assert not _nms_equal(r32, r64), ('the case does not discriminate: fp64 gives the fp32 sequence', case.name)
    for m in case.kills:
        assert not _nms_equal(case.ref(F32, m), r32), ('the case does not show the mutation', case.name, m)
    return r64 if case.tier == 'exact' else r32


def check_nms(ops, dev, case):
    want = assert_nms_case_holds(case)
    got = ops.batched_nms(tuple(t.to(dev) for t in case.cand()), case.B, case.cap, case.thr, case.max_out)
    assert_nms_output(got, want, ('batched_nms', case.name))


def check_nms_flat(ops, dev, case):
    """the same lists, image by image, through ops.nms_flat (B = 1, no capacity rows, no max_out)"""
    dtype = F64 if case.tier == 'exact' else F32
    for b in range(case.B):
        n = int(case.cnt[b])
        bx, sc, ids = case.boxes[b, :n], case.scores[b, :n], case.ids[b, :n]
        want = nms_keep(bx.numpy(), sc.numpy(), ids.numpy(), n, case.thr, max(n, 1), dtype)
        got = ops.nms_flat(bx.to(dev), sc.to(dev), ids.to(dev), case.thr).cpu()
        assert got.dtype == torch.int64 and got.tolist() == want, ('nms_flat', case.name, b, len(want), got.numel())


# ==================================================================================================================== decode
DECODE_MUTATIONS = ('delta_contracted', 'centre_contracted', 'size_clamped_from_both_sides_under_ctr_clamp', 'ctr_clamp_skipped',
                    'clip_to_size_minus_one', 'min_size_ge', 'min_size_zero_disables')
Coder = collections.namedtuple('Coder', 'means stds max_ratio ctr_clamp clip_border add_ctr_clamp')
MAX_RATIO = abs(math.log(16 / 1000))


def decode_boxes(an, d, coder, img_h, img_w, dtype=F64, mut=None):
    """delta2bbox of anchors / rois [m, 4] and deltas [m, 4] (both already in `dtype`) -> [m, 4]; img_h / img_w: 0-dim"""
    means = torch.tensor(coder.means, dtype=F32).to(dtype)
    stds = torch.tensor(coder.stds, dtype=F32).to(dtype)
    dd = _fma(d, stds, means, dtype) if mut == 'delta_contracted' else d * stds + means
    dxy, dwh = dd[:, :2], dd[:, 2:]
    pxy = (an[:, :2] + an[:, 2:]) * 0.5
    pwh = an[:, 2:] - an[:, :2]
    mr, cc = _f32(coder.max_ratio, dtype), _f32(coder.ctr_clamp, dtype)
    if coder.add_ctr_clamp:
        shift = pwh * dxy
        if mut != 'ctr_clamp_skipped':
            shift = torch.minimum(torch.maximum(shift, -cc), cc)
        dwh = torch.minimum(dwh, mr)
        if mut == 'size_clamped_from_both_sides_under_ctr_clamp':
            dwh = torch.maximum(dwh, -mr)
        gxy = pxy + shift
    else:
        dwh = torch.minimum(torch.maximum(dwh, -mr), mr)
        gxy = _fma(pwh, dxy, pxy, dtype) if mut == 'centre_contracted' else pxy + pwh * dxy
    gwh = pwh * torch.exp(dwh)
    out = torch.cat([gxy - gwh * 0.5, gxy + gwh * 0.5], 1)
    if coder.clip_border:
        hi = torch.stack([img_w, img_h, img_w, img_h]).to(dtype) - (1.0 if mut == 'clip_to_size_minus_one' else 0.0)
        out = torch.minimum(torch.maximum(out, torch.zeros_like(out)), hi.expand_as(out))
    return out


def rpn_decode_ref(heads, sizes, strides, ld, A, k, base, coder, min_size, sel_idx, sel_score, sel_cnt, img_hw, cap, dtype=F64, mut=None):
    """-> the candidate buffers of rsp_rpn_decode: boxes [B, cap, 4] (in `dtype`), scores, ids, src, cnt, compacted level-major in
    the order of sel_idx; rows behind the count are 0 / -1"""
    B, L = sel_cnt.shape
    boxes = torch.zeros(B, cap, 4, dtype=dtype)
    scores = torch.zeros(B, cap, dtype=F32)
    ids = torch.full((B, cap), -1, dtype=torch.int32)
    src = torch.full((B, cap), -1, dtype=torch.int32)
    cnt = torch.zeros(B, dtype=torch.int32)
    ms = _f32(min_size, dtype)
    for b in range(B):
        o = 0
        for lvl in range(L):
            n = int(sel_cnt[b, lvl])
            if n == 0:
                continue
            H, W = sizes[lvl]
            c = sel_idx[b, lvl, :n].long()
            pos, a = c // A, c % A
            y, x = pos // W, pos % W
            st = _f32(strides[lvl], dtype)
            sh = torch.stack([x.to(dtype) * st, y.to(dtype) * st], 1).repeat(1, 2)
            an = base[lvl][a].to(dtype) + sh
            rows = heads[lvl][b * H * W + pos]
            d = torch.stack([rows[torch.arange(n), A + 4 * a + j] for j in range(4)], 1).to(dtype)
            bx = decode_boxes(an, d, coder, img_hw[b, 0].to(dtype), img_hw[b, 1].to(dtype), dtype, mut)
            w, h = bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]
            off = (min_size <= 0) if mut == 'min_size_zero_disables' else (min_size < 0)
            if off:
                valid = torch.ones(n, dtype=torch.bool)
            elif mut == 'min_size_ge':
                valid = (w >= ms) & (h >= ms)
            else:
                valid = (w > ms) & (h > ms)
            m = int(valid.sum())
            boxes[b, o:o + m], scores[b, o:o + m] = bx[valid], sel_score[b, lvl, :n][valid]
            ids[b, o:o + m], src[b, o:o + m] = lvl, c[valid].int()
            o += m
        cnt[b] = o
    return boxes, scores, ids, src, cnt


def _rpn_desc(ops, heads, sizes, strides, ld, A, k, base, coder, min_size):
    d = ops._lib.RspRpnDesc()
    for i, (hd, (H, W)) in enumerate(zip(heads, sizes)):
        d.head[i] = hd.data_ptr()
        d.H[i], d.W[i], d.stride[i] = H, W, float(strides[i])
    d.ld, d.A, d.nms_pre, d.num_levels = ld, A, k, len(heads)
    d.base_anchors = base.data_ptr()
    d.coder, d.min_bbox_size = ops.box_coder(coder), float(min_size)
    return d


_DEFAULT_CODER = Coder((0.0,) * 4, (1.0,) * 4, MAX_RATIO, 32.0, True, False)


def rpn_topk(ops, dev, heads, sizes, ld, A, k, B):
    """rsp_rpn_topk through the library the wrappers use (ops.RpnSelector chains it with the decode and the NMS); a stand-in
    without a library answers with its own rpn_topk.  The outputs start poisoned: rows behind a count stay -7"""
    if not hasattr(ops, '_lib'):
        return ops.rpn_topk(heads, sizes, ld, A, k, B)
    lib = ops._lib.load()
    hd = [h.to(dev) for h in heads]
    L = len(heads)
    base = torch.zeros(L, A, 4, device=dev)
    d = _rpn_desc(ops, hd, sizes, [1.0] * L, ld, A, k, base, _DEFAULT_CODER, 0.0)
    sel_idx = torch.full((B, L, k), -7, dtype=torch.int32, device=dev)
    sel_score = torch.full((B, L, k), -7.0, dtype=F32, device=dev)
    sel_cnt = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    ops._lib.check(lib.rsp_rpn_topk(d, B, sel_idx.data_ptr(), sel_score.data_ptr(), sel_cnt.data_ptr(), ops._stream()), 'rsp_rpn_topk')
    return sel_idx.cpu(), sel_score.cpu(), sel_cnt.cpu()


def rpn_decode(ops, dev, heads, sizes, strides, ld, A, k, base, coder, min_size, sel_idx, sel_score, sel_cnt, img_hw, cap):
    """rsp_rpn_decode on hand-built selections, as rpn_topk above"""
    if not hasattr(ops, '_lib'):
        return ops.rpn_decode(heads, sizes, strides, ld, A, k, base, coder, min_size, sel_idx, sel_score, sel_cnt, img_hw, cap)
    lib = ops._lib.load()
    hd = [h.to(dev) for h in heads]
    bs = torch.stack(list(base)).float().contiguous().to(dev)
    d = _rpn_desc(ops, hd, sizes, strides, ld, A, k, bs, coder, min_size)
    B = sel_cnt.shape[0]
    si, ss, sc, ih = _to(dev, sel_idx.contiguous(), sel_score.contiguous(), sel_cnt.contiguous(), img_hw.contiguous())
    boxes = torch.zeros(B, cap, 4, dtype=F32, device=dev)
    scores = torch.zeros(B, cap, dtype=F32, device=dev)
    ids = torch.full((B, cap), -1, dtype=torch.int32, device=dev)
    src = torch.full((B, cap), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
    ops._lib.check(lib.rsp_rpn_decode(d, B, si.data_ptr(), ss.data_ptr(), sc.data_ptr(), ih.data_ptr(), cap, boxes.data_ptr(),
                                      scores.data_ptr(), ids.data_ptr(), src.data_ptr(), cnt.data_ptr(), ops._stream()), 'rsp_rpn_decode')
    return tuple(t.cpu() for t in (boxes, scores, ids, src, cnt))


class DecodeCase:
    """one call of rsp_rpn_decode: a pyramid of heads whose delta columns are set per selected candidate"""

    def __init__(self, name, tier, coder, min_size, sizes, strides, A, k, per_level, img_hw, kills=(), emu=True, cap=None, real_anchors=False):
        """per_level[b][lvl] = deltas [n, 4] of n candidates at random (cell, anchor) places, or (deltas, anchor, cells or None):
        all on one anchor shape, at the given cells or at random cells off the first row and column"""
        self.name, self.tier, self.coder, self.min_size, self.sizes, self.strides = name, tier, coder, min_size, sizes, strides
        self.A, self.k, self.kills, self.emu = A, k, tuple(kills), emu
        self.ld = 5 * A + 3                                                  # ld > 5 A
        B, L = len(per_level), len(sizes)
        self.B, self.L = B, L
        self.cap = cap or L * k
        self.img_hw = torch.tensor(img_hw, dtype=F32)
        g = torch.Generator().manual_seed(len(name))
        self.base = [torch.tensor([[-(2.0 ** (a + 2)), -(2.0 ** (a + 1)), 2.0 ** (a + 2), 2.0 ** (a + 1)] for a in range(A)]) * s
                     for s in strides]                                       # dyadic base anchors, none square
        if real_anchors:                                                     # AnchorGenerator(scales=[8], ratios=[0.5, 1, 2]): sides 8 s sqrt(2)^(-1, 0, 1)
            hr = torch.tensor([0.5, 1.0, 2.0]).sqrt()
            self.base = [torch.stack([-0.5 * (8 * s / hr), -0.5 * (8 * s * hr), 0.5 * (8 * s / hr), 0.5 * (8 * s * hr)], 1) for s in strides]
        self.heads = [torch.full((B * H * W, self.ld), 77.0) for H, W in sizes]
        self.sel_idx = torch.full((B, L, k), -7, dtype=torch.int32)
        self.sel_score = torch.full((B, L, k), -7.0)
        self.sel_cnt = torch.zeros(B, L, dtype=torch.int32)
        for b in range(B):
            for lvl, entry in enumerate(per_level[b]):
                H, W = sizes[lvl]
                deltas, fixed_a, fixed_pos = entry if isinstance(entry, tuple) else (entry, None, None)
                n = deltas.shape[0]
                assert n <= k and n <= H * W * A, (name, n, k, H * W * A)
                if fixed_a is None:
                    c = torch.randperm(H * W * A, generator=g)[:n]           # any order: the decode keeps it
                else:                                                        # one anchor shape, cells off the first row and column
                    inner = torch.tensor([y * W + x for y in range(1, H) for x in range(1, W)])
                    pos = inner[torch.randperm(inner.numel(), generator=g)[:n]] if fixed_pos is None else torch.tensor(fixed_pos)
                    c = pos * A + fixed_a
                pos, a = c // A, c % A
                for j in range(4):
                    self.heads[lvl][b * H * W + pos, A + 4 * a + j] = deltas[:, j]
                self.sel_idx[b, lvl, :n] = c.int()
                self.sel_score[b, lvl, :n] = torch.rand(n, generator=g)
                self.sel_cnt[b, lvl] = n

    def ref(self, dtype, mut=None):
        return rpn_decode_ref(self.heads, self.sizes, self.strides, self.ld, self.A, self.k, self.base, self.coder, self.min_size,
                              self.sel_idx, self.sel_score, self.sel_cnt, self.img_hw, self.cap, dtype, mut)

    def run(self, ops, dev):
        return rpn_decode(ops, dev, self.heads, self.sizes, self.strides, self.ld, self.A, self.k, self.base, self.coder, self.min_size,
                          self.sel_idx, self.sel_score, self.sel_cnt, self.img_hw, self.cap)


def _dyadic_deltas(n, g, dwh=0.0, scale=8):
    d = torch.randint(-scale, scale + 1, (n, 4), generator=g).float() / 16
    d[:, 2:] = dwh
    return d


def _edge_deltas(coder, pw, below=True):
    """deltas for an anchor of width pw: the centre shift exactly at +-ctr_clamp, one ulp beyond and (below: the sum with the
    centre rounds, so the sequence tier only) one ulp inside, zero, and dw far below -max_ratio (the size vanishes beside the
    centre: exact); stds / means are undone so that the de-normalised delta is the target"""
    rows = []
    cc = coder.ctr_clamp
    for target in (cc, _above(cc), -cc, -_above(cc), 0.0) + ((_below(cc), -_below(cc)) if below else ()):
        dx = (target / pw - coder.means[0]) / coder.stds[0]
        rows.append([dx, (0.25 - coder.means[1]) / coder.stds[1], (0.0 - coder.means[2]) / coder.stds[2], (0.0 - coder.means[3]) / coder.stds[3]])
    rows.append([0.0, 0.0, (-128.0 - coder.means[2]) / coder.stds[2], (-128.0 - coder.means[3]) / coder.stds[3]])
    return torch.tensor(rows, dtype=F32)


_CODER_DYADIC = Coder((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0), MAX_RATIO, 32.0, True, False)
_CODER_MEANS = Coder((0.25, -0.5, 1.0, -2.0), (0.5, 0.25, 0.5, 2.0), MAX_RATIO, 32.0, True, False)        # dw = -2 * 0.5 + 1 = 0
_CODER_NOCLIP = Coder((0.0, 0.0, 0.0, 0.0), (0.5, 0.5, 1.0, 1.0), MAX_RATIO, 32.0, False, False)
_CODER_CTR = Coder((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0), MAX_RATIO, 8.0, True, True)
_CODER_REAL = Coder((0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2), MAX_RATIO, 32.0, True, False)
_CODER_REAL_NOCLIP = _CODER_REAL._replace(clip_border=False)
_CODER_REAL_CTR = _CODER_REAL._replace(add_ctr_clamp=True, ctr_clamp=8.0)
COMPACTION_COUNTS = (0, 1, 1023, 1024, 1025)


def _zero_size(d, coder):
    """deltas with dw = dh = 0 after de-normalisation"""
    d = d.clone()
    d[:, 2] = (0.0 - coder.means[2]) / coder.stds[2]
    d[:, 3] = (0.0 - coder.means[3]) / coder.stds[3]
    return d


@functools.lru_cache(maxsize=None)
def decode_cases():
    """level 0 (stride 4), anchor 0 is 32 x 16 around (4 x, 4 y): the hand-placed rows below use it"""
    g = torch.Generator().manual_seed(9)
    sizes, strides = ((12, 16), (6, 8), (3, 4)), (4.0, 8.0, 16.0)
    img = [[40.0, 56.0], [48.0, 64.0]]
    cases = []
    for name, coder in (('dyadic', _CODER_DYADIC), ('means-stds', _CODER_MEANS), ('no-clip', _CODER_NOCLIP)):
        per = [[_zero_size(_dyadic_deltas(n, g), coder) for n in (50, 0, 30)], [_zero_size(_dyadic_deltas(n, g), coder) for n in (1, 60, 36)]]
        # 16 is a side that anchors have exactly (strict: dropped); the float below 16 keeps them
        for ms, kills in ((0.0, ('min_size_zero_disables',) if coder.clip_border else ()), (-1.0, ()), (16.0, ('min_size_ge',)), (_below(16.0), ())):
            cases.append(DecodeCase(f'{name}-min{ms:.9g}', 'exact', coder, ms, sizes, strides, 3, 64, per, img, kills=kills))
    # the centre clamp: shifts exactly at +-ctr_clamp and one ulp either side; dw far below -max_ratio (clamped from above only)
    for tier in ('exact', 'seq'):
        per = [[(_edge_deltas(_CODER_CTR, 32.0, below=tier == 'seq'), 0, None), _dyadic_deltas(0, g), _zero_size(_dyadic_deltas(9, g, 0.0, 64), _CODER_CTR)]] * 2
        cases.append(DecodeCase(f'ctr-clamp-{tier}', tier, _CODER_CTR, -1.0, sizes, strides, 6, 16, per, [[400.0, 400.0]] * 2,
                                kills=('size_clamped_from_both_sides_under_ctr_clamp', 'ctr_clamp_skipped')))
    # the clip: x1 < 0, x2 / y2 exactly on the image's side and one ulp above, boxes wholly outside (zero size after the clip:
    # min_size 0 drops them, -1 keeps them)
    placed = torch.tensor([[0.0, 0, 0, 0], [2.0 ** -23, 0, 0, 0], [0.0, 0, 0, 0], [0.0, 0, 0, 0], [0.0, 2.0 ** -22, 0, 0], [-64.0, 0, 0, 0], [64.0, 0, 0, 0]])
    at = [3 * 16 + 10, 4 * 16 + 10, 5 * 16 + 1, 8 * 16 + 5, 8 * 16 + 6, 2 * 16 + 3, 2 * 16 + 4]
    far = torch.tensor([[-64.0, 0.0, 0.0, 0.0], [64.0, 0.0, 0.0, 0.0], [0.0, -64.0, 0.0, 0.0], [0.0, 64.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    per = [[(placed, 0, at), far.repeat(4, 1), far.repeat(2, 1)]] * 2
    for ms in (0.0, -1.0):
        cases.append(DecodeCase(f'clip-min{ms:g}', 'exact', _CODER_DYADIC, ms, sizes, strides, 3, 64, per, [[40.0, 56.0]] * 2,
                                kills=('clip_to_size_minus_one',) + (('min_size_zero_disables',) if ms == 0.0 else ())))
    # compaction: per-level survivors of 0, 1, 1023, 1024, 1025; a level that loses everything between two that keep theirs;
    # cap = L * nms_pre exactly.  A candidate dies by a shift far out of the image (zero size after the clip, min_size 0)
    big_sizes, big_strides = ((32, 36), (32, 36), (32, 36)), (4.0, 4.0, 4.0)

    def level(n_alive, n):
        d = _dyadic_deltas(n, g, scale=2)
        dead = torch.randperm(n, generator=g)[:n - n_alive]
        d[dead, 0] = -64.0
        return d
    per = [[level(1023, 1030), level(0, 1030), level(1025, 1030)], [level(1024, 1030), level(1, 7), level(1030, 1030)]]
    cases.append(DecodeCase('compaction', 'exact', _CODER_DYADIC, 0.0, big_sizes, big_strides, 3, 1030, per, [[200.0, 200.0]] * 2,
                            kills=('min_size_zero_disables',)))
    # ---- sequence tier: random non-dyadic deltas, stds (0.1, 0.1, 0.2, 0.2), dw = dh = 0.  d * std + 0 has no contracted form
    # that differs, so one coder carries non-zero means for dx and dy
    for name, coder, kills in (('real', _CODER_REAL, ('centre_contracted',)), ('real-no-clip', _CODER_REAL_NOCLIP, ('centre_contracted',)),
                               ('means', _CODER_REAL_NOCLIP._replace(means=(0.013, -0.027, 0.0, 0.0)), ('delta_contracted', 'centre_contracted'))):
        per = [[_zero_size(torch.randn(n, 4, generator=g) * 4, coder) for n in (64, 48, 36)] for _ in range(2)]
        cases.append(DecodeCase(f'seq-{name}', 'seq', coder, 0.0, sizes, strides, 3, 64, per, [[3000.0, 3000.0]] * 2, kills=kills, real_anchors=True))
    return tuple(cases)


def decode_case(name):
    return next(c for c in decode_cases() if c.name == name)


def _cand_equal(a, b):
    return all(torch.equal(x.double() if x.is_floating_point() else x, y.double() if y.is_floating_point() else y) for x, y in zip(a, b))


def _changed_fraction(a, b):
    """the fraction of the decoded coordinates (of the rows both kept) that differ"""
    n = min(int(a[4].min()), int(b[4].min()))
    return float((a[0][:, :n].double() != b[0][:, :n].double()).float().mean()) if n else 0.0


def assert_decode_case_holds(case):
    r32, r64 = case.ref(F32), case.ref(F64)
    if case.tier == 'exact':
        assert r32[0].dtype == F32 and _cand_equal(r32, r64), ('not an exact case: fp32 and fp64 differ', case.name)
    else:
        assert not _cand_equal(r32, r64), ('the case does not discriminate', case.name)
    for m in case.kills:
        mm = case.ref(F32, m)
        assert not _cand_equal(mm, r32), ('the case does not show the mutation', case.name, m)
        if m in ('delta_contracted', 'centre_contracted'):                   # a contraction moves a coordinate in twenty at least
            assert _changed_fraction(mm, r32) >= 0.05, (case.name, m, _changed_fraction(mm, r32))
    return r64 if case.tier == 'exact' else r32


def assert_cand(got, want, what):
    """candidate buffers (boxes, scores, ids, src, cnt) up to the counts, bit for bit; boxes compared in fp64"""
    _same(got[4], want[4], (what, 'cnt'))
    for b in range(want[4].shape[0]):
        n = int(want[4][b])
        gb = got[0][b, :n].cpu()
        assert gb.dtype == F32 and torch.equal(gb.double(), want[0][b, :n].double()), (what, 'boxes', b, _first_diff(gb.double(), want[0][b, :n].double()))
        for i, key in ((1, 'scores'), (2, 'ids'), (3, 'src')):
            assert torch.equal(got[i][b, :n].cpu(), want[i][b, :n]), (what, key, b)


def check_decode(ops, dev, case):
    want = assert_decode_case_holds(case)
    assert_cand(case.run(ops, dev), want, ('rpn_decode', case.name))


def _delta_for(target, std):
    """the fp32 delta whose fp32 product with fp32(std) IS fp32(target) (the mean is 0): a neighbour of target / std"""
    t32, s32 = np.float32(target), np.float32(std)
    d = np.float32(target / std)
    for cand in [d] + [f(d, np.float32(sgn * np.inf)) for sgn in (1, -1) for f in (np.nextafter, lambda a, b: np.nextafter(np.nextafter(a, b), b))]:
        if np.float32(cand * s32) == t32:
            return float(cand)
    raise AssertionError(('no fp32 delta gives the target', target, std))


def decode_tol_case():
    """the real coder with dw, dh != 0: deltas beyond +-max_ratio / at it and one ulp either side, shifts at the ctr clamp"""
    g = torch.Generator().manual_seed(21)
    sizes, strides = ((12, 16), (6, 8), (3, 4)), (4.0, 8.0, 16.0)
    out = []
    for name, coder in (('tol-real', _CODER_REAL), ('tol-ctr', _CODER_REAL_CTR), ('tol-no-clip', _CODER_REAL_NOCLIP)):
        per = []
        for b in range(2):
            lv = []
            for n in (60, 40, 30):
                d = torch.randn(n, 4, generator=g) * 3
                for j, t in enumerate((MAX_RATIO, _below(MAX_RATIO), _above(MAX_RATIO), -MAX_RATIO, 100.0, -100.0)):
                    d[j, 2] = _delta_for(t, 0.2)
                    d[j + 6, 3] = _delta_for(t, 0.2)
                lv.append(d)
            per.append(lv)
        out.append(DecodeCase(name, 'tol', coder, 4.0, sizes, strides, 3, 64, per, [[800.0, 1333.0]] * 2))
    return tuple(out)


DECODE_TOL = decode_tol_case()


def _near_allowed(n_near, case):
    assert n_near <= 2, ('the reference has', n_near, 'candidates near a cut (at most 2): another seed', case)


def check_decode_tolerance(ops, dev, report=print, cases=None):
    rep = DetReport('rpn_decode', report)
    for case in (cases or DECODE_TOL):
        # the filter off: every candidate's box and side, for the measure and the near set
        all64 = DecodeCase.ref(_with(case, min_size=-1.0), F64)
        all32 = DecodeCase.ref(_with(case, min_size=-1.0), F32)
        side64 = torch.cat([all64[0][..., 2] - all64[0][..., 0], all64[0][..., 3] - all64[0][..., 1]])
        side32 = torch.cat([all32[0][..., 2] - all32[0][..., 0], all32[0][..., 3] - all32[0][..., 1]]).double()
        e_side = float((side32 - side64).abs().max())
        assert 2 * e_side <= NEAR_SIDE, ('NEAR_SIDE is below twice the fp32 restatement distance', case.name, e_side)
        near = ((all64[0][..., 2] - all64[0][..., 0] - case.min_size).abs() < NEAR_SIDE) | ((all64[0][..., 3] - all64[0][..., 1] - case.min_size).abs() < NEAR_SIDE)
        _near_allowed(int(near.sum(1).max()), case.name)
        w64, w32 = case.ref(F64), case.ref(F32)
        got = case.run(ops, dev)
        for b in range(case.B):
            n = int(w64[4][b])
            near_src = {(int(all64[2][b, i]), int(all64[3][b, i])) for i in near[b].nonzero()[:, 0].tolist()}
            gk = [(int(got[2][b, i]), int(got[3][b, i])) for i in range(int(got[4][b]))]
            wk = [(int(w64[2][b, i]), int(w64[3][b, i])) for i in range(n)]
            assert set(gk) ^ set(wk) <= near_src, ('rpn_decode keeps another set away from min_bbox_size', case.name, b)
            assert [k for k in gk if k not in near_src] == [k for k in wk if k not in near_src], ('order', case.name, b)
            if gk == wk:
                n32 = int(w32[4][b])
                r32 = w32[0][b, :n] if n32 == n else w64[0][b, :n].float()
                rep.add(f'{case.name} image {b} n={n}', got[0][b, :n], w64[0][b, :n], r32)
                assert torch.equal(got[1][b, :n], w64[1][b, :n])
        report(f'det rpn_decode {case.name}: side E32 {e_side:.3e} NEAR_SIDE {NEAR_SIDE:.1e}; near min_bbox_size: {int(near.sum())}')
    return rep.finish()


def _with(case, **kw):
    import copy
    c = copy.copy(case)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ================================================================================================================== bbox_post
POST_MUTATIONS = ('score_ge', 'background_is_a_candidate', 'softmax_without_max', 'scale_by_division', 'division_by_truncated_reciprocal')


def bbox_post_cand(head, ld, rois, roi_start, img_hw, nc, score_thr, coder, scale_factors=None, dtype=F64, mut=None, exact=False,
                   want_scores=False):
    """-> candidate buffers (boxes [B, cap, 4] in `dtype`, scores fp32 [B, cap], ids, src, cnt) with cap = max RoIs x classes, in
    (roi, class) order.  exact: the fp64 scores are flushed (module docstring).  want_scores: also the full score table"""
    B = img_hw.shape[0]
    rs = [int(v) for v in roi_start]
    ncand = nc + 1 if mut == 'background_is_a_candidate' else nc
    cap = max(max((rs[b + 1] - rs[b]) for b in range(B)) * ncand, 1)
    boxes = torch.zeros(B, cap, 4, dtype=dtype)
    scores = torch.zeros(B, cap, dtype=dtype)
    ids = torch.full((B, cap), -1, dtype=torch.int32)
    src = torch.full((B, cap), -1, dtype=torch.int32)
    cnt = torch.zeros(B, dtype=torch.int32)
    thr = _f32(score_thr, dtype)
    table = []
    for b in range(B):
        rows = head[rs[b]:rs[b + 1]]
        n = rows.shape[0]
        if n == 0:
            table.append(torch.zeros(0, nc, dtype=dtype))
            continue
        sc = _softmax_fg(rows[:, :nc + 1].to(dtype), mut)[:, :ncand]
        if exact and dtype == F64:
            sc = flush(sc)
        table.append(sc[:, :nc])
        valid = ((sc >= thr) if mut == 'score_ge' else (sc > thr)).reshape(-1)
        cls = torch.arange(ncand).repeat(n)
        dcls = torch.where(cls < nc, cls, torch.zeros_like(cls))                 # (the background has no deltas: class 0's)
        r = torch.arange(n).repeat_interleave(ncand)
        d = torch.stack([rows[r, nc + 1 + 4 * dcls + j] for j in range(4)], 1).to(dtype)
        an = rois[rs[b]:rs[b + 1], 1:][r].to(dtype)
        bx = decode_boxes(an, d, coder, img_hw[b, 0].to(dtype), img_hw[b, 1].to(dtype), dtype)
        if scale_factors is not None:
            sf = scale_factors[b]
            if mut == 'scale_by_division':
                bx = bx / torch.stack([_f32(sf[0], dtype), _f32(sf[1], dtype)]).repeat(2)
            else:
                bx = bx * torch.stack([_f32(1 / float(sf[0]), dtype), _f32(1 / float(sf[1]), dtype)]).repeat(2)
        m = int(valid.sum())
        boxes[b, :m], scores[b, :m] = bx[valid], sc.reshape(-1)[valid]
        ids[b, :m], src[b, :m] = cls[valid].int(), torch.arange(n * ncand)[valid].int()
        cnt[b] = m
    out = (boxes, scores, ids, src, cnt)
    return (out, table) if want_scores else out


def bbox_post_ref(case_args, iou_thr, max_out, dtype=F64, mut=None, exact=False):
    """rsp_bbox_post + rsp_batched_nms as ops.bbox_post chains them -> the dict of ops.batched_nms + cand_count.  Everything runs in
    `dtype`; the outputs are stored as fp32"""
    boxes, scores, ids, src, cnt = bbox_post_cand(*case_args, dtype=dtype, mut=mut if mut in POST_MUTATIONS else None, exact=exact)
    out = nms_ref(boxes, scores, ids, src, cnt, iou_thr, max_out, dtype, mut if mut in NMS_MUTATIONS else None)
    out['cand_count'] = cnt
    return out


class PostCase:
    def __init__(self, name, tier, nc, rois_per_image, score_thr, coder, iou_thr, scale_factors=None, kills=(), seed=1, emu=True,
                 hot=100.0, dyadic=True, maxima=(1, 2, 4)):
        """exact softmax rows: per RoI j in {1, 2, 4} logits at 0 (or at `hot`: the max is subtracted) and the rest 200 below"""
        g = torch.Generator().manual_seed(seed)
        self.name, self.tier, self.nc, self.score_thr, self.coder, self.iou_thr = name, tier, nc, score_thr, coder, iou_thr
        self.scale_factors, self.kills, self.emu = scale_factors, tuple(kills), emu
        n = sum(rois_per_image)
        self.ld = (5 * nc + 1 + 3) // 4 * 4 + 4
        self.roi_start = torch.tensor([0] + list(np.cumsum(rois_per_image)), dtype=torch.int32)
        B = len(rois_per_image)
        self.B = B
        self.img_hw = torch.tensor([[96.0, 128.0]] * B)
        head = torch.full((n, self.ld), 55.0)
        js = [j for j in maxima if j <= nc + 1]
        for r in range(n):
            j = js[r % len(js)]
            top = hot if r % 5 == 0 else 0.0
            head[r, :nc + 1] = top - 200.0
            cols = torch.randperm(nc + 1, generator=g)[:j]
            if r % 7 == 0 and nc not in cols.tolist():
                cols[0] = nc                                                 # the background among the maxima
            head[r, cols] = top
        if dyadic:
            xy = torch.randint(0, 12, (n, 2), generator=g).float() * 8
            wh = torch.randint(1, 5, (n, 2), generator=g).float() * 8
            d = torch.randint(-8, 9, (n, 4 * nc), generator=g).float() / 16
        else:
            xy = torch.rand(n, 2, generator=g) * 90
            wh = torch.rand(n, 2, generator=g) * 30 + 4
            d = torch.randn(n, 4 * nc, generator=g)
        d = d.view(n, nc, 4)
        d[:, :, 2] = (0.0 - coder.means[2]) / coder.stds[2]
        d[:, :, 3] = (0.0 - coder.means[3]) / coder.stds[3]
        head[:, nc + 1:5 * nc + 1] = d.reshape(n, 4 * nc)
        bidx = torch.repeat_interleave(torch.arange(B), torch.tensor(rois_per_image)).float()
        self.rois = torch.cat([bidx[:, None], xy, xy + wh], 1).contiguous()
        self.head = head.contiguous()
        self.max_out = max(max(rois_per_image) * nc, 1)

    def args(self):
        return (self.head, self.ld, self.rois, self.roi_start, self.img_hw, self.nc, self.score_thr, self.coder, self.scale_factors)

    def ref(self, dtype, mut=None, iou_thr=None):
        return bbox_post_ref(self.args(), self.iou_thr if iou_thr is None else iou_thr, self.max_out, dtype, mut, exact=True)

    def run(self, ops, dev, iou_thr=None):
        h, r, ih = _to(dev, self.head, self.rois, self.img_hw)
        return ops.bbox_post(h, self.ld, r, self.roi_start, ih, self.nc, self.score_thr, self.coder,
                             self.iou_thr if iou_thr is None else iou_thr, self.max_out, scale_factors=self.scale_factors)


@functools.lru_cache(maxsize=None)
def post_cases():
    cases = []
    seed = 30
    for nc in (1, 3, 7, 10):
        for thr, kills in ((0.5, ('score_ge', 'background_is_a_candidate', 'softmax_without_max', 'ties_by_index_descending')), (_below(0.5), ('background_is_a_candidate',)),
                           (0.25, ('score_ge',)), (_below(0.25), ())):
            if nc == 1 and thr < 0.3:
                continue                                                     # nc + 1 = 2: no row with four maxima
            seed += 1
            cases.append(PostCase(f'nc{nc}-thr{thr:.9g}', 'exact', nc, (23, 0, 40), thr, _CODER_DYADIC, 0.5, kills=kills, seed=seed))
    cases.append(PostCase('ragged-0-first', 'exact', 3, (0, 17, 0), 0.25, _CODER_MEANS, 0.5, kills=('score_ge',), seed=50))
    # more than 1024 candidates in an image: the scan loop takes several trips with a ragged last one
    cases.append(PostCase('many-nc10', 'exact', 10, (5, 0, 1100), _below(0.25), _CODER_DYADIC, 0.5, seed=51, emu=False,
                          kills=('iou_ge', 'ties_by_index_descending')))                   # ... and the NMS behind them cuts at IoU = 1/2
    # sequence tier: non-dyadic RoIs and deltas (dw = dh = 0), a non-dyadic scale factor: a product by fp32(1 / sf)
    sfs = [(1.3, 0.7), (1.0, 1.0), (800 / 1333, 1333 / 800)]
    cases.append(PostCase('seq-scaled', 'seq', 3, (30, 0, 41), 0.25, _CODER_REAL, 0.5, scale_factors=sfs,
                          kills=('scale_by_division', 'score_ge'), seed=52, dyadic=False))
    # sequence tier: rows with 3, 5, 6, 7 ... maxima: exp(0) = 1 and expf(-200) = 0 exactly, so the score is fp32(1 / j) if and only
    # if the softmax division is correctly rounded; score_thr sits on fp32(1 / 3) and on the float below it
    third = float(np.float32(1.0) / np.float32(3.0))
    for nc, thr, kills in ((3, third, ('score_ge',)), (3, _below(third), ('division_by_truncated_reciprocal',)),
                           (10, _below(third), ('division_by_truncated_reciprocal',))):
        cases.append(PostCase(f'seq-odd-maxima-nc{nc}-thr{thr:.9g}', 'seq', nc, (29, 0, 44), thr, _CODER_REAL, 0.5, kills=kills, seed=54 + nc,
                              maxima=(1, 3, 5, 6, 7, 9, 10, 11), dyadic=False))
    cases.append(PostCase('seq-unscaled', 'seq', 7, (25, 3, 0), _below(0.5), _CODER_REAL_NOCLIP, 0.5, seed=53, dyadic=False))
    return tuple(cases)


def post_case(name):
    return next(c for c in post_cases() if c.name == name)


def _post_equal(a, b):
    return _nms_equal(a, b) and torch.equal(a['cand_count'], b['cand_count'])


def assert_post_case_holds(case):
    """-> the oracles without and with the NMS (iou_thr = 1: nothing is suppressed, every candidate comes out in score order)"""
    wants, r32s = [], {}
    for iou in (1.0, case.iou_thr):
        r32, r64 = case.ref(F32, iou_thr=iou), case.ref(F64, iou_thr=iou)
        if case.tier == 'exact':
            assert _post_equal(r32, r64), ('not an exact case: fp32 and fp64 differ', case.name, iou)
        else:
            assert not _post_equal(r32, r64), ('the case does not discriminate', case.name, iou)
        r32s[iou] = r32
        wants.append(r64 if case.tier == 'exact' else r32)
    for m in case.kills:
        iou = case.iou_thr if m in NMS_MUTATIONS else 1.0
        assert not _post_equal(case.ref(F32, m, iou_thr=iou), r32s[iou]), ('the case does not show the mutation', case.name, m)
    return wants


def check_post(ops, dev, case):
    w_all, w_nms = assert_post_case_holds(case)
    for iou, want in ((1.0, w_all), (case.iou_thr, w_nms)):
        got = case.run(ops, dev, iou)
        _same(got['cand_count'], want['cand_count'], ('bbox_post', case.name, 'cand_count'))
        assert_nms_output(got, want, ('bbox_post', case.name, iou))


PostTol = collections.namedtuple('PostTol', 'nc rois score_thr coder sf seed')
BBOX_TOL = (PostTol(10, (60, 0, 90), 0.05, _CODER_REAL, None, 0), PostTol(3, (70, 40, 1), 0.3, _CODER_REAL_CTR, ((1.3, 0.7),) * 3, 0),
            PostTol(1, (50, 64, 0), 0.5, _CODER_REAL_NOCLIP, None, 0))


def post_tol_inputs(c, seed=None):
    g = torch.Generator().manual_seed(c.seed if seed is None else seed)
    n, nc = sum(c.rois), c.nc
    ld = (5 * nc + 1 + 3) // 4 * 4
    head = torch.zeros(n, ld)
    head[:, :nc + 1] = torch.randn(n, nc + 1, generator=g) * 2.5
    head[:, nc + 1:5 * nc + 1] = torch.randn(n, 4 * nc, generator=g)
    head[0, :nc + 1] += 100.0                                                # no overflow: the max is subtracted
    xy = torch.rand(n, 2, generator=g) * 300
    bidx = torch.repeat_interleave(torch.arange(len(c.rois)), torch.tensor(c.rois)).float()
    rois = torch.cat([bidx[:, None], xy, xy + torch.rand(n, 2, generator=g) * 120 + 2], 1)
    roi_start = torch.tensor([0] + list(np.cumsum(c.rois)), dtype=torch.int32)
    img_hw = torch.tensor([[400.0, 420.0]] * len(c.rois))
    return (head, ld, rois, roi_start, img_hw, nc, c.score_thr, c.coder, c.sf)


def _pair_iou_near(boxes64, boxes32, ids, n, thr):
    """the IoU of every pair of the offset candidates of one image, all in fp64 and all in fp32 (decode included)
    -> (largest distance, pairs whose fp64 IoU is within NEAR_IOU of thr)"""
    if n < 2:
        return 0.0, 0
    out = []
    for dt, boxes in ((np.float64, boxes64), (np.float32, boxes32)):
        ob = _offset_boxes(boxes, ids, n, dt, None)
        x1, y1, x2, y2 = (ob[:, j] for j in range(4))
        w = np.maximum(dt(0), np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]))
        h = np.maximum(dt(0), np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]))
        inter = w * h
        a = (x2 - x1) * (y2 - y1)
        with np.errstate(all='ignore'):
            out.append((inter / (a[:, None] + a[None] - inter)).astype(np.float64))
    iu = np.triu_indices(n, 1)
    d = np.nan_to_num(np.abs(out[0] - out[1])[iu])
    return float(d.max()), int((np.abs(out[0][iu] - float(np.float32(thr))) < NEAR_IOU).sum())


def post_tol_figures(c, seed=None, iou_thr=0.5):
    """on the reference alone -> dict(e_score, near_thr, near_order, e_iou, near_iou) of a tolerance case"""
    args = post_tol_inputs(c, seed)
    (c64, t64) = bbox_post_cand(*args, dtype=F64, want_scores=True)
    (c32, t32) = bbox_post_cand(*args, dtype=F32, want_scores=True)
    e_score = max([float((a.double() - b).abs().max()) for a, b in zip(t32, t64) if b.numel()] + [0.0])
    near_thr = max(int(((b - float(np.float32(c.score_thr))).abs() < NEAR_SCORE).sum()) for b in t64)
    near_order, e_iou, near_iou = 0, 0.0, 0
    for b in range(len(c.rois)):
        n = int(c64[4][b])
        s = c64[1][b, :n].sort(descending=True).values
        near_order = max(near_order, int(((s[:-1] - s[1:]) < NEAR_SCORE).sum()) if n > 1 else 0)
        same = int(c32[4][b]) == n and torch.equal(c32[3][b], c64[3][b])      # (else a score sits on score_thr: near_thr says so)
        e, k = _pair_iou_near(c64[0][b].numpy(), (c32 if same else c64)[0][b].float().numpy(), c64[2][b].numpy(), n, iou_thr)
        e_iou, near_iou = max(e_iou, e), max(near_iou, k)
    return dict(e_score=e_score, near_thr=near_thr, near_order=near_order, e_iou=e_iou, near_iou=near_iou)


def check_post_tolerance(ops, dev, report=print, cases=None):
    rep = DetReport('bbox_post', report)
    for c in (cases or BBOX_TOL):
        args = post_tol_inputs(c)
        fig = post_tol_figures(c)
        assert 2 * fig['e_score'] <= NEAR_SCORE and 2 * fig['e_iou'] <= NEAR_IOU, ('a NEAR_* is below twice the fp32 distance', c, fig)
        assert fig['near_thr'] <= 2 and fig['near_order'] == 0 and fig['near_iou'] == 0, ('candidates near a cut: another seed', c, fig)
        c64 = bbox_post_cand(*args, dtype=F64)
        t64 = bbox_post_cand(*args, dtype=F64, want_scores=True)[1]
        max_out = int(c64[0].shape[1])
        head, ld, rois, roi_start, img_hw = args[:5]
        h, r, ih = _to(dev, head, rois, img_hw)
        for iou in (1.0, 0.5):
            got = {k: v.cpu() for k, v in ops.bbox_post(h, ld, r, roi_start, ih, c.nc, c.score_thr, c.coder, iou, max_out, scale_factors=c.sf).items()}
            w64 = bbox_post_ref(args, iou, max_out, F64)
            w32 = bbox_post_ref(args, iou, max_out, F32)
            for b in range(len(c.rois)):
                thr = float(np.float32(c.score_thr))
                near = {i for i in range(t64[b].numel()) if abs(float(t64[b].reshape(-1)[i]) - thr) < NEAR_SCORE}
                gk = got['src'][b, :int(got['count'][b])].tolist()
                wk = w64['src'][b, :int(w64['count'][b])].tolist()
                assert set(gk) ^ set(wk) <= near, ('bbox_post keeps another set away from a cut', c, iou, b, sorted(set(gk) ^ set(wk))[:8])
                assert [k for k in gk if k not in near] == [k for k in wk if k not in near], ('order', c, iou, b)
                if gk == wk and len(gk):
                    m = len(gk)
                    same32 = w32['src'][b, :m].tolist() == wk and int(w32['count'][b]) == m
                    cand64 = {int(s_): i for i, s_ in enumerate(c64[3][b, :int(c64[4][b])].tolist())}
                    rows = torch.tensor([cand64[k] for k in gk])
                    ref_b, ref_s = c64[0][b][rows], c64[1][b][rows]
                    rep.add(f'nc={c.nc} iou={iou} image {b} boxes', got['boxes'][b, :m], ref_b, w32['boxes'][b, :m] if same32 else ref_b.float())
                    rep.add(f'nc={c.nc} iou={iou} image {b} scores', got['scores'][b, :m], ref_s, w32['scores'][b, :m] if same32 else ref_s.float())
                    assert torch.equal(got['ids'][b, :m], w64['ids'][b, :m])
        report(f'det bbox_post nc={c.nc}: score E32 {fig["e_score"]:.3e} NEAR_SCORE {NEAR_SCORE:.1e}, IoU E32 {fig["e_iou"]:.3e} NEAR_IOU {NEAR_IOU:.1e}; '
               f'near score_thr {fig["near_thr"]}, near ties {fig["near_order"]}, near iou_thr {fig["near_iou"]}')
    return rep.finish()


# ====================================================================================================================== top-k
TOPK_MUTATIONS = ('negative_zero_below_zero', 'ties_by_index_descending', 'kth_ties_from_the_end', 'sorted_when_n_le_k')
QUERY_MUTATIONS = ('ties_by_index_descending', 'kth_ties_from_the_end', 'flat_index_class_major', 'division_by_truncated_reciprocal')


def _select(score, k, mut=None, signbit=None):
    """the first k of a stable descending sort of a 1-d score vector -> indices, in that order"""
    n = score.numel()
    idx = torch.arange(n)
    if mut == 'ties_by_index_descending':
        order = (n - 1 - torch.sort(score.flip(0), descending=True, stable=True)[1])
    elif mut == 'negative_zero_below_zero' and signbit is not None:
        first = torch.sort(signbit.to(torch.int8), stable=True)[1]                 # +0 logits before -0 logits at one score
        order = first[torch.sort(score[first], descending=True, stable=True)[1]]
    else:
        order = torch.sort(score, descending=True, stable=True)[1]
    if mut == 'kth_ties_from_the_end' and k < n:
        kth = score[order[k - 1]]
        gt = order[score[order] > kth]
        eq = idx[score == kth]
        return torch.cat([gt, eq[eq.numel() - (k - gt.numel()):]])
    return order[:k]


def rpn_topk_ref(heads, sizes, ld, A, k, B, dtype=F64, mut=None, exact=False):
    """-> sel_idx int32 [B, L, k], sel_score [B, L, k] in `dtype`, sel_cnt [B, L]; rows behind a count stay -7"""
    L = len(heads)
    sel_idx = torch.full((B, L, k), -7, dtype=torch.int32)
    sel_score = torch.full((B, L, k), -7.0, dtype=dtype)
    sel_cnt = torch.zeros(B, L, dtype=torch.int32)
    for b in range(B):
        for lvl, (H, W) in enumerate(sizes):
            logit = heads[lvl][b * H * W:(b + 1) * H * W, :A].reshape(-1)
            sc = _sigmoid(logit.to(dtype))
            if exact and dtype == F64:
                sc = flush(sc)
            n = sc.numel()
            if n <= k and mut != 'sorted_when_n_le_k':
                sel = torch.arange(n)
            else:
                sel = _select(sc, min(k, n), mut, torch.signbit(logit))
            m = sel.numel()
            sel_idx[b, lvl, :m], sel_score[b, lvl, :m], sel_cnt[b, lvl] = sel.int(), sc[sel], m
    return sel_idx, sel_score, sel_cnt


TopkCase = collections.namedtuple('TopkCase', 'name A ld k levels emu')


def topk_kills(case):
    """the mutations an exact top-k case must show: the three tie rules everywhere (every case has +-0.0 ties at its cut), the sorted
    natural order where a level has n <= nms_pre"""
    le = any(H * W * case.A <= case.k for (H, W), *_ in case.levels)
    return TOPK_MUTATIONS[:3] + (('sorted_when_n_le_k',) if le else ())

# levels: ((H, W), pattern of image 0, pattern of image 1); a pattern is ('mix',) -- logits drawn from {-100, -0.0, 0, 100} --,
# ('equal', v) -- one value (v = 0: +0.0 and -0.0 mixed) -- or ('kth', n_gt, n_eq): n_gt logits at 100, n_eq at +-0.0, the rest
# at -100, with n_gt < k < n_gt + n_eq: the k-th score lies inside the run of ties
RPN_TOPK = (
    TopkCase('k1-A3', 3, 18, 1, (((2, 1), ('kth', 0, 2), ('equal', 0)), ((1, 1), ('mix',), ('equal', 100)), ((5, 7), ('mix',), ('kth', 0, 2))), True),
    TopkCase('k5-A6', 6, 33, 5, (((1, 1), ('mix',), ('kth', 3, 3)), ((4, 4), ('kth', 2, 30), ('mix',))), True),                 # n = k + 1
    TopkCase('k1000-A3', 3, 16, 1000, (((20, 16), ('mix',), ('equal', 0)), ((41, 13), ('kth', 500, 1025), ('kth', 999, 2)),
                                      ((32, 24), ('kth', 0, 1024), ('kth', 100, 1025)), ((2765, 1), ('kth', 999, 1025), ('mix',))), False),
    TopkCase('k1022-A3', 3, 16, 1022, (((341, 1), ('mix',), ('kth', 1021, 2)), ((31, 11), ('equal', -100), ('equal', 0))), False),   # n = k + 1
    TopkCase('k1024-A6', 6, 31, 1024, (((10, 17), ('mix',), ('equal', 0)), ((20, 30), ('kth', 1, 1024), ('kth', 1023, 1025)),
                                      ((1400, 1), ('equal', 0), ('kth', 0, 1025))), False),
    TopkCase('k64-A3-emu', 3, 16, 64, (((5, 4), ('mix',), ('equal', 0)), ((8, 11), ('kth', 40, 30), ('kth', 63, 2)), ((30, 12), ('kth', 0, 1025), ('mix',))), True),
)


def topk_inputs(case, seed=3):
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor([-100.0, -0.0, 0.0, 100.0])
    heads, B = [], 2
    for (H, W), *pats in case.levels:
        n = H * W * case.A
        hd = torch.full((B * H * W, case.ld), 100.0)                        # the other columns would win if they were read
        for b, pat in enumerate(pats):
            if pat[0] == 'mix':
                v = vals[torch.randint(0, 4, (n,), generator=g)]
            elif pat[0] == 'equal':
                v = torch.full((n,), float(pat[1]))
                if pat[1] == 0:
                    v = vals[torch.randint(1, 3, (n,), generator=g)]
            else:
                _, n_gt, n_eq = pat
                assert n_gt < case.k < n_gt + n_eq <= n, (case.name, pat, n)
                v = torch.full((n,), -100.0)
                p = torch.randperm(n, generator=g)
                v[p[:n_gt]] = 100.0
                v[p[n_gt:n_gt + n_eq]] = vals[torch.randint(1, 3, (n_eq,), generator=g)]
            hd[b * H * W:(b + 1) * H * W, :case.A] = v.view(H * W, case.A)
        heads.append(hd.contiguous())
    return heads, [s for s, *_ in case.levels], B


def _sel_equal(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].double(), b[1].double()) and torch.equal(a[2], b[2])


def assert_sel(got, want, what):
    _same(got[2], want[2], (what, 'sel_cnt'))
    _same(got[0], want[0], (what, 'sel_idx'))
    g = got[1].cpu()
    assert g.dtype == F32 and torch.equal(g.double(), want[1].double()), (what, 'sel_score', _first_diff(g.double(), want[1].double()))


def check_exact_rpn_topk(ops, dev, case):
    heads, sizes, B = topk_inputs(case)
    ref = rpn_topk_ref(heads, sizes, case.ld, case.A, case.k, B, F64, exact=True)
    r32 = rpn_topk_ref(heads, sizes, case.ld, case.A, case.k, B, F32)
    assert r32[1].dtype == F32 and _sel_equal(r32, ref), ('not an exact case: fp32 and fp64 differ', case.name)
    for m in topk_kills(case):
        assert not _sel_equal(rpn_topk_ref(heads, sizes, case.ld, case.A, case.k, B, F32, m), r32), ('the case does not show the mutation', case.name, m)
    assert_sel(rpn_topk(ops, dev, heads, sizes, case.ld, case.A, case.k, B), ref, ('rpn_topk', case.name))


def _assert_selection_near(got_idx, got_n, ref_idx, q64, k_cut, what):
    """a top-k decision of the tolerance tier: the sets differ only by candidates within NEAR_SCORE of the k-th score, and the
    order follows the fp64 scores up to NEAR_SCORE (exact ties by index)"""
    g, r = got_idx[:got_n].tolist(), ref_idx[:got_n].tolist()
    assert len(set(g)) == got_n
    if k_cut is not None:
        near = {i for i in set(g) ^ set(r) if abs(float(q64[i]) - k_cut) < NEAR_SCORE}
        assert set(g) ^ set(r) == near, (what, 'a candidate away from the k-th score trades places', sorted(set(g) ^ set(r))[:8])
    else:
        assert set(g) == set(r), what
    if k_cut is not None:                                                    # exact ties with the k-th score: the lowest indices
        tied = (q64 == k_cut).nonzero()[:, 0].tolist()
        took = sorted(i for i in g if float(q64[i]) == k_cut)
        assert took == tied[:len(took)], (what, 'ties with the k-th score are not taken from the front')
    qs = q64[torch.tensor(g, dtype=torch.long)] if g else q64[:0]
    assert bool((qs[:-1] - qs[1:] > -NEAR_SCORE).all()), (what, 'order')
    tie = (qs[:-1] == qs[1:]).nonzero()[:, 0].tolist()
    assert all(g[i] < g[i + 1] for i in tie), (what, 'equal scores out of index order')


RpnTol = collections.namedtuple('RpnTol', 'A ld k sizes seed')
RPN_TOL = (RpnTol(3, 16, 200, ((24, 20), (12, 10), (5, 6)), 0), RpnTol(6, 40, 1000, ((40, 30), (9, 20)), 0))


def rpn_tol_inputs(c, seed=None):
    g = torch.Generator().manual_seed(c.seed if seed is None else seed)
    heads, B = [], 2
    for H, W in c.sizes:
        hd = torch.randn(B * H * W, c.ld, generator=g) * 3
        hd[::17, :c.A] = hd[3, :c.A]                                        # exact ties between positions
        heads.append(hd.contiguous())
    return heads, B


def rpn_tol_figures(c, seed=None):
    heads, B = rpn_tol_inputs(c, seed)
    r64 = rpn_topk_ref(heads, c.sizes, c.ld, c.A, c.k, B, F64)
    e, near = 0.0, 0
    for lvl, (H, W) in enumerate(c.sizes):
        for b in range(B):
            logit = heads[lvl][b * H * W:(b + 1) * H * W, :c.A].reshape(-1)
            s64, s32 = _sigmoid(logit.double()), _sigmoid(logit)
            e = max(e, float((s32.double() - s64).abs().max()))
            if logit.numel() > c.k:
                kth = float(r64[1][b, lvl, c.k - 1])
                near = max(near, int((((s64 - kth).abs() < NEAR_SCORE) & (s64 != kth)).sum()))
    return e, near


def check_rpn_topk_tolerance(ops, dev, report=print, cases=None):
    rep = DetReport('rpn_topk', report)
    for c in (cases or RPN_TOL):
        heads, B = rpn_tol_inputs(c)
        e, near = rpn_tol_figures(c)
        assert 2 * e <= NEAR_SCORE, ('NEAR_SCORE is below twice the fp32 restatement distance', c, e)
        _near_allowed(near, c)
        r64 = rpn_topk_ref(heads, c.sizes, c.ld, c.A, c.k, B, F64)
        r32 = rpn_topk_ref(heads, c.sizes, c.ld, c.A, c.k, B, F32)
        got = rpn_topk(ops, dev, heads, c.sizes, c.ld, c.A, c.k, B)
        _same(got[2], r64[2], ('rpn_topk tolerance', 'sel_cnt'))
        for lvl, (H, W) in enumerate(c.sizes):
            for b in range(B):
                logit = heads[lvl][b * H * W:(b + 1) * H * W, :c.A].reshape(-1)
                q64 = _sigmoid(logit.double())
                m = int(r64[2][b, lvl])
                if logit.numel() <= c.k:
                    assert got[0][b, lvl, :m].tolist() == list(range(m)), ('natural order', c, lvl, b)
                else:
                    _assert_selection_near(got[0][b, lvl], m, r64[0][b, lvl], q64, float(r64[1][b, lvl, c.k - 1]), ('rpn_topk', c, lvl, b))
                gi = got[0][b, lvl, :m].long()
                rep.add(f'A={c.A} k={c.k} level {lvl} image {b} scores', got[1][b, lvl, :m], q64[gi], _sigmoid(logit)[gi])
        report(f'det rpn_topk A={c.A} k={c.k}: score E32 {e:.3e} NEAR_SCORE {NEAR_SCORE:.1e}; near the k-th score: {near}')
    return rep.finish()


# ---------------------------------------------------------------------------------------------------------------- query top-k
def query_topk_ref(cls, k, dtype=F64, mut=None, exact=False):
    """maskformer_fusion_head.py:149-162: softmax over nc + 1, the background column dropped, top-k of the Nq nc scores by (score
    descending, flat index ascending) -> (scores [B, k] in `dtype`, flat int32 [B, k])"""
    B, Nq, nc1 = cls.shape
    nc = nc1 - 1
    out_s = torch.zeros(B, k, dtype=dtype)
    out_f = torch.zeros(B, k, dtype=torch.int32)
    for b in range(B):
        sc = _softmax_fg(cls[b].to(dtype), mut)[:, :nc]
        if exact and dtype == F64:
            sc = flush(sc)
        if mut == 'flat_index_class_major':
            flat = sc.t().reshape(-1)
        else:
            flat = sc.reshape(-1)
        sel = _select(flat, k, mut)
        out_s[b], out_f[b] = flat[sel], sel.int()
    return out_s, out_f


QueryCase = collections.namedtuple('QueryCase', 'Nq nc k')


def query_kills(case):
    """the mutations an exact query case must show: ties by descending index everywhere, the ties at the cut taken from the end
    where there is a cut (k < Nq nc), the class-major flat index where there is more than one class"""
    return ('ties_by_index_descending',) + (('kth_ties_from_the_end',) if case.k < case.Nq * case.nc else ()) + \
        (('flat_index_class_major',) if case.nc > 1 else ())

QUERY_EXACT = (QueryCase(128, 8, 1), QueryCase(128, 8, 1024), QueryCase(128, 8, 100), QueryCase(205, 5, 100), QueryCase(205, 5, 1025),
               QueryCase(64, 1, 10), QueryCase(65, 1, 65), QueryCase(65, 1, 1), QueryCase(100, 80, 100), QueryCase(7, 3, 21))


def query_exact_inputs(case, seed=29, maxima=(1, 2, 4)):
    """rows with j in {1, 2, 4} logits at 0 (every fifth row: at 100) and the rest 200 below: scores 1/j or 0, tied across queries
    and across the classes of one query; image 1 is image 0 with its queries reversed"""
    g = torch.Generator().manual_seed(seed)
    Nq, nc = case.Nq, case.nc
    js = [j for j in maxima if j <= nc + 1]
    cls = torch.zeros(2, Nq, nc + 1)
    for q in range(Nq):
        j = js[int(torch.randint(0, len(js), (1,), generator=g))]
        top = 100.0 if q % 5 == 0 else 0.0
        cls[0, q] = top - 200.0
        cols = torch.randperm(nc + 1, generator=g)[:j]
        if q % 3 == 0 and nc not in cols.tolist():
            cols[0] = nc                                                     # the background among the maxima
        cls[0, q, cols] = top
    cls[1] = cls[0].flip(0)
    return cls.contiguous()


def check_exact_query_topk(ops, dev, case):
    cls = query_exact_inputs(case)
    ref = query_topk_ref(cls, case.k, F64, exact=True)
    r32 = query_topk_ref(cls, case.k, F32)
    assert r32[0].dtype == F32 and torch.equal(r32[0].double(), ref[0]) and torch.equal(r32[1], ref[1]), ('not an exact case', case)
    for m in query_kills(case):
        bad = query_topk_ref(cls, case.k, F32, m)
        assert not (torch.equal(bad[0], r32[0]) and torch.equal(bad[1], r32[1])), ('the case does not show the mutation', case, m)
    sc, fl = ops.query_topk(cls.to(dev), case.k)
    _same(fl, ref[1], ('query_topk', case, 'flat'))
    assert sc.dtype == F32 and torch.equal(sc.cpu().double(), ref[0]), ('query_topk', case, 'scores', _first_diff(sc.cpu().double(), ref[0]))


QUERY_SEQ = (QueryCase(40, 10, 400), QueryCase(33, 6, 50), QueryCase(100, 80, 100))


def check_seq_query_topk(ops, dev, case):
    """rows with 1, 3, 5, 6, 7 ... maxima: scores fp32(1 / j), the correctly rounded quotient of two exact numbers; the kernel must
    equal the fp32 sequence, which the fp64 restatement and a reciprocal that is not rounded to nearest do not"""
    cls = query_exact_inputs(case, maxima=(1, 3, 5, 6, 7, 9, 10, 11))
    r32 = query_topk_ref(cls, case.k, F32)
    r64 = query_topk_ref(cls, case.k, F64, exact=True)
    assert not torch.equal(r32[0].double(), r64[0]), ('the case does not discriminate', case)
    bad = query_topk_ref(cls, case.k, F32, 'division_by_truncated_reciprocal')
    assert not torch.equal(bad[0], r32[0]), ('the case does not show the mutation', case)
    sc, fl = ops.query_topk(cls.to(dev), case.k)
    _same(fl, r32[1], ('query_topk', case, 'flat'))
    _same(sc, r32[0], ('query_topk', case, 'scores'))


QUERY_TOL = (QueryCase(100, 80, 100), QueryCase(33, 5, 64), QueryCase(50, 1, 50))


def query_tol_inputs(c, seed=0):
    g = torch.Generator().manual_seed(seed + c.Nq)
    cls = torch.randn(2, c.Nq, c.nc + 1, generator=g) * 2
    cls[:, c.Nq - 1] = cls[:, 0]                                            # an exact tie between the first and the last query
    return cls.contiguous()


def query_tol_figures(c, seed=0):
    cls = query_tol_inputs(c, seed)
    e, near = 0.0, 0
    for b in range(2):
        s64 = _softmax_fg(cls[b].double())[:, :c.nc].reshape(-1)
        s32 = _softmax_fg(cls[b])[:, :c.nc].reshape(-1)
        e = max(e, float((s32.double() - s64).abs().max()))
        if c.k < s64.numel():
            kth = float(s64.sort(descending=True).values[c.k - 1])
            near = max(near, int((((s64 - kth).abs() < NEAR_SCORE) & (s64 != kth)).sum()))
    return e, near


def check_query_topk_tolerance(ops, dev, report=print, cases=None):
    rep = DetReport('query_topk', report)
    for c in (cases or QUERY_TOL):
        cls = query_tol_inputs(c)
        e, near = query_tol_figures(c)
        assert 2 * e <= NEAR_SCORE, ('NEAR_SCORE is below twice the fp32 restatement distance', c, e)
        _near_allowed(near, c)
        r64 = query_topk_ref(cls, c.k, F64)
        sc, fl = ops.query_topk(cls.to(dev), c.k)
        sc, fl = sc.cpu(), fl.cpu()
        for b in range(2):
            q64 = _softmax_fg(cls[b].double())[:, :c.nc].reshape(-1)
            cut = float(r64[0][b, c.k - 1]) if c.k < q64.numel() else None
            _assert_selection_near(fl[b], c.k, r64[1][b], q64, cut, ('query_topk', c, b))
            rep.add(f'Nq={c.Nq} nc={c.nc} k={c.k} image {b}', sc[b], q64[fl[b].long()], _softmax_fg(cls[b])[:, :c.nc].reshape(-1)[fl[b].long()])
        report(f'det query_topk Nq={c.Nq} nc={c.nc} k={c.k}: score E32 {e:.3e} NEAR_SCORE {NEAR_SCORE:.1e}; near the k-th score: {near}')
    return rep.finish()


def measure_near():
    """the figures behind NEAR_*: (score, side, IoU) fp32-from-fp64 distances per tolerance case, on the reference alone"""
    rows = [('rpn_topk', c, rpn_tol_figures(c)[0]) for c in RPN_TOL] + [('query_topk', c, query_tol_figures(c)[0]) for c in QUERY_TOL]
    for c in BBOX_TOL:
        f = post_tol_figures(c)
        rows += [('bbox_post score', c, f['e_score']), ('bbox_post iou', c, f['e_iou'])]
    for case in DECODE_TOL:
        a64, a32 = _with(case, min_size=-1.0).ref(F64), _with(case, min_size=-1.0).ref(F32)
        s = lambda a: torch.cat([a[0][..., 2] - a[0][..., 0], a[0][..., 3] - a[0][..., 1]]).double()
        rows.append(('rpn_decode side', case.name, float((s(a32) - s(a64)).abs().max())))
    return rows


# ========================================================================================================= failure signatures
class FakeOps:
    """the entry points of rsprompter_amd.ops for the detection selection, computed by the fp32-sequence restatements on the CPU
    with at most one mutation (tests/test_kernel_props_selfcheck_cpu.py)"""

    def __init__(self, mutation=None):
        known = NMS_MUTATIONS + DECODE_MUTATIONS + POST_MUTATIONS + TOPK_MUTATIONS + QUERY_MUTATIONS
        assert mutation is None or mutation in known, mutation
        self.mut = mutation

    def _m(self, family):
        return self.mut if self.mut in family else None

    def batched_nms(self, cand, B, cap, iou_thr, max_out):
        boxes, scores, ids, src, cnt = cand
        out = nms_ref(boxes, scores, ids, src, cnt, iou_thr, max_out, F32, self._m(NMS_MUTATIONS))
        out['cand_count'] = cnt
        return out

    def nms_flat(self, boxes, scores, labels, iou_thr):
        n = boxes.shape[0]
        return torch.tensor(nms_keep(boxes.numpy(), scores.numpy(), labels.numpy(), n, iou_thr, max(n, 1), F32, self._m(NMS_MUTATIONS)),
                            dtype=torch.int64)

    def bbox_post(self, head, ld, rois, roi_start, img_hw, num_classes, score_thr, coder, iou_thr, max_out, scale_factors=None):
        return bbox_post_ref((head, ld, rois, roi_start, img_hw, num_classes, score_thr, coder, scale_factors), iou_thr, max_out, F32,
                             self._m(POST_MUTATIONS + NMS_MUTATIONS))

    def rpn_topk(self, heads, sizes, ld, A, k, B):
        return rpn_topk_ref(heads, sizes, ld, A, k, B, F32, self._m(TOPK_MUTATIONS))

    def rpn_decode(self, heads, sizes, strides, ld, A, k, base, coder, min_size, sel_idx, sel_score, sel_cnt, img_hw, cap):
        return rpn_decode_ref(heads, sizes, strides, ld, A, k, base, coder, min_size, sel_idx, sel_score, sel_cnt, img_hw, cap, F32,
                              self._m(DECODE_MUTATIONS))

    def query_topk(self, cls, k):
        return query_topk_ref(cls, k, F32, self._m(QUERY_MUTATIONS))
