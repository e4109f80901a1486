"""Case bodies of the oriented-box comparison (csrc/obb_iou.hip), shared by the emulator tier
(tests/test_obb_iou_cpu.py) and the device tier (tests/test_gpu_obb_iou.py).  The oracle is tests/_obb_iou_ref.py: the exact
IoU in fractions; decisions (keep lists, dtm) are compared for EQUALITY with the reference run on the exact IoUs, values
against the exact IoU within BOUND."""
import functools
import json
from fractions import Fraction

import numpy as np
import torch

import _cocoeval_ref as cref
import _mask_obb_cases as ocases
import _mask_obb_ref as oref
import _obb_iou_ref as ref
import _seam_merge_cases as seam_cases

# THE TOLERANCE of every value that is not exactly representable.  It is measured against the EXACT reference, never against
# the kernel: the largest |twin - exact| over the committed generator `families()` below is 1.97e-13, held here as 2.0e-13
# (the far slivers: a 5 000 x 1 pixel box 60 000 pixels from the origin; ordinary boxes 2.5e-16, lattice rectangles 2.3e-16,
# near-identical boxes 1.1e-15: tests/test_obb_iou_cpu.py prints them), times 16: the kernel may order its sums otherwise
# than the twin, which is worth a small constant; nothing in the method is worth more.
# test_the_twin_stays_within_a_sixteenth_of_the_bound holds the measurement to it.
TWIN_WORST = 2.0e-13
BOUND = 16 * TWIN_WORST
# no exact IoU of a decision case lies this close to a threshold in use (asserted on the CPU, without product code)
DECISION_MARGIN = 1e-9
NMS_SIZES = (0, 1, 2, 63, 64, 65, 129, 1000)


# ---------------------------------------------------------------------------------------------------------- generators
def box(cx, cy, w, h, ang):
    """float64 [4, 2], clockwise on screen from (-w / 2, -h / 2) in the box's frame"""
    ux, uy = np.cos(ang), np.sin(ang)
    sa, sb = np.array([-1.0, 1.0, 1.0, -1.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    return np.stack([cx + sa * (w / 2) * ux - sb * (h / 2) * uy, cy + sa * (w / 2) * uy + sb * (h / 2) * ux], 1)


def ordinary(seed, n):
    """pairs of random boxes of 1-80 pixels at arbitrary angles, the second near the first"""
    rng = np.random.default_rng(seed)
    a = [box(rng.uniform(0, 200), rng.uniform(0, 200), rng.uniform(1, 80), rng.uniform(1, 80), rng.uniform(-np.pi, np.pi))
         for _ in range(n)]
    b = [box(x[:, 0].mean() + rng.uniform(-30, 30), x[:, 1].mean() + rng.uniform(-30, 30), rng.uniform(1, 80),
             rng.uniform(1, 80), rng.uniform(-np.pi, np.pi)) for x in a]
    return np.stack(a), np.stack(b)


def slivers(seed, n):
    """5 000 x 1 pixel slivers 60 000 pixels from the origin whose angles differ by less than 0.01 rad"""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for _ in range(n):
        cx, cy, ang = rng.uniform(59000, 61000), rng.uniform(59000, 61000), rng.uniform(-np.pi, np.pi)
        a.append(box(cx, cy, 5000.0, 1.0, ang))
        b.append(box(cx + rng.uniform(-2, 2), cy + rng.uniform(-2, 2), 5000.0, 1.0, ang + rng.uniform(-0.01, 0.01)))
    return np.stack(a), np.stack(b)


def near_identical(seed, n):
    """a box against itself with its corners moved by 0, 1e-9 or 1e-6.  THIS FAMILY IS HERE BECAUSE IT BREAKS THE
    BOUNDARY-INTEGRAL FORM of the intersection (clip every edge of each box by the other box and sum p x q without a vertex
    list): the crossing of two almost parallel edges is then computed twice, independently, the boundary does not close by
    ~1e-3 px, and the shoelace sum turns the gap into an IoU error of 1.4e-5.  The closed Sutherland-Hodgman polygon is
    within 2e-15 on the same inputs."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for i in range(n):
        x = box(rng.uniform(0, 2000), rng.uniform(0, 2000), rng.uniform(20, 300), rng.uniform(20, 300),
                rng.uniform(-np.pi, np.pi))
        eps = (0.0, 1e-9, 1e-6)[i % 3]
        a.append(x)
        b.append(x + eps * rng.uniform(-1, 1, (4, 2)))
    return np.stack(a), np.stack(b)


def _rect_of_q(ex, ey, amin, amax, bmin, bmax):
    """the expression of rle.obb_to_numpy(form='corners'), restated"""
    ex, ey, L = float(ex), float(ey), float(ex) * float(ex) + float(ey) * float(ey)
    a, b = np.array([amin, amax, amax, amin], np.float64), np.array([bmin, bmin, bmax, bmax], np.float64)
    return np.stack([(a * ex - b * ey) / L, (a * ey + b * ex) / L], 1)


def lattice(seed, n):
    """rectangles as the merge produces them: obb_to_numpy's corners of random q (|e| <= 40, extents to 3 000 pixels) at
    integer offsets, the second rectangle in the first one's frame or in one of its own"""
    rng = np.random.default_rng(seed)

    def rect(near=None):
        while True:
            ex, ey = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))
            if ex or ey:
                break
        L = ex * ex + ey * ey
        root = L ** 0.5
        U, V = int(rng.uniform(1, 3000) * root), int(rng.uniform(1, 3000) * root)
        ox, oy = (int(rng.integers(0, 60000)), int(rng.integers(0, 60000))) if near is None else \
            (near[0] + int(rng.integers(-800, 800)), near[1] + int(rng.integers(-800, 800)))
        a0, b0 = ox * ex + oy * ey, -ox * ey + oy * ex
        return _rect_of_q(ex, ey, a0, a0 + max(U, 1), b0, b0 + max(V, 1)), (ox, oy)
    a, b = [], []
    for _ in range(n):
        ra, at = rect()
        a.append(ra)
        b.append(rect(at)[0])
    return np.stack(a), np.stack(b)


FAMILIES = (('ordinary', ordinary, (0, 1), 300), ('slivers', slivers, (2, 3), 150), ('near-identical', near_identical, (4, 5), 150),
            ('lattice', lattice, (6, 7), 300))


@functools.lru_cache(maxsize=None)
def families():
    """[(name, a [n, 4, 2], b [n, 4, 2], exact IoUs as Fractions)] of the committed generator, made once and shared"""
    out = []
    for name, fn, seeds, n in FAMILIES:
        parts = [fn(s, n) for s in seeds]
        a, b = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        out.append((name, a, b, [ref.exact_iou(x, y) for x, y in zip(a, b)]))
    return out


def twin_errors():
    """{family: the largest |twin - exact|}"""
    return {name: max(abs(Fraction(ref.twin_iou(x, y)) - e) for x, y, e in zip(a, b, ex)) for name, a, b, ex in families()}


# ------------------------------------------------------------------------------------------------------------- helpers
def pair_units(ops, dev, n):
    """n units of one pair each: dt i against gt i"""
    idx = np.arange(n, dtype=np.int64)
    return ops.coco_units(idx, idx, idx, np.ones(n, np.int64), np.ones(n, np.int64), np.zeros(n, np.int64), dev)


def dev_quads(q, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1, 4, 2))).to(dev)


def pair_iou(ops, dev, a, b, crowd=None):
    """device IoU of a[i] with b[i] -> list of floats"""
    n = len(a)
    c = torch.zeros((n,), dtype=torch.uint8) if crowd is None else torch.tensor(crowd, dtype=torch.uint8)
    return ops.obb_iou(pair_units(ops, dev, n), n, dev_quads(a, dev), dev_quads(b, dev), c.to(dev)).cpu().tolist()


def matrix_iou(ops, dev, a, b, crowd=None):
    D, G = len(a), len(b)
    c = torch.zeros((G,), dtype=torch.uint8) if crowd is None else torch.tensor(crowd, dtype=torch.uint8)
    units = ops.coco_units([0], [0], [0], [D], [G], [0], dev)
    return ops.obb_iou(units, D * G, dev_quads(a, dev), dev_quads(b, dev), c.to(dev)).view(D, G).cpu().numpy()


def assert_within_bound(got, exact, what):
    worst = 0.0
    for i, (g, e) in enumerate(zip(got, exact)):
        err = abs(Fraction(float(g)) - e)
        worst = max(worst, float(err))
        assert err <= Fraction(BOUND), f'{what}: pair {i}: device {g!r}, exact {float(e)!r}, off by {float(err):.3e} > {BOUND:.3e}'
    return worst


# --------------------------------------------------------------------------------------------------------- exact answers
def sq(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


DIAMOND = np.array([[2, -2], [6, 2], [2, 6], [-2, 2]], np.float64)


def exact_table():
    """(name, a, b, crowd, expected Fraction): small integer corners, every fp64 operation exact"""
    S = sq(0, 0, 4, 4)
    nan = np.full((4, 2), np.nan)
    inf = S.copy()
    inf[2, 0] = np.inf
    return [
        ('identical squares', S, S, 0, Fraction(1)),
        ('half-shifted squares', S, sq(2, 0, 6, 4), 0, Fraction(1, 3)),
        ('square and diamond', S, DIAMOND, 0, Fraction(1, 2)),
        ('sharing an edge', S, sq(4, 0, 8, 4), 0, Fraction(0)),
        ('sharing a corner', S, sq(4, 4, 8, 8), 0, Fraction(0)),
        ('a vertex on an edge', S, np.array([[4, 2], [6, 0], [8, 2], [6, 4]], np.float64), 0, Fraction(0)),
        ('a vertex on a slanted edge', DIAMOND, sq(5, -3, 9, 1), 0, Fraction(0)),
        ('sharing part of a slanted edge', DIAMOND, np.array([[4, 0], [8, -4], [10, -2], [6, 2]], np.float64), 0, Fraction(0)),
        ('inside, apart from the edges', S, sq(1, 1, 2, 2), 0, Fraction(1, 16)),
        ('inside, flush with an edge', S, sq(0, 1, 1, 2), 0, Fraction(1, 16)),
        ('plus-shaped crossing', sq(0, 4, 9, 5), sq(4, 0, 5, 9), 0, Fraction(1, 17)),
        ('plus-shaped crossing, wide arms', sq(0, 3, 10, 5), sq(4, 0, 6, 9), 0, Fraction(2, 17)),
        ('rotated 45 degrees, identical', DIAMOND, DIAMOND, 0, Fraction(1)),
        ('zero-area box', S, np.array([[0, 0], [4, 4], [8, 8], [2, 2]], np.float64), 0, Fraction(0)),
        ('a point', S, sq(1, 1, 1, 1), 0, Fraction(0)),
        ('NaN box', S, nan, 0, Fraction(0)),
        ('infinite corner', S, inf, 0, Fraction(0)),
        ('crowd gt around the dt', sq(1, 1, 2, 2), S, 1, Fraction(1)),
        ('crowd gt half over the dt', S, sq(2, 0, 6, 4), 1, Fraction(1, 2)),
    ]


def check_exact_table(ops, dev):
    """the device double == the expected value, in either orientation of either box, and with the operands swapped"""
    rows = exact_table()
    for name, a, b, crowd, want in rows:                                         # the table is the reference's own
        assert ref.exact_iou(a, b, bool(crowd)) == want, name
    A, B, C, W = [], [], [], []
    for name, a, b, crowd, want in rows:
        for ra in (a, a[::-1]):
            for rb in (b, b[::-1]):
                A.append(ra), B.append(rb), C.append(crowd), W.append((name, float(want)))
                if not crowd:
                    A.append(rb), B.append(ra), C.append(0), W.append((name + ' (swapped)', float(want)))
    got = pair_iou(ops, dev, A, B, C)
    for g, (name, want) in zip(got, W):
        assert g == want, f'{name}: {g!r} != {want!r}'
    return len(got)


def check_families(ops, dev):
    """every family of the committed generator within BOUND of the exact value"""
    worst = {}
    for name, a, b, exact in families():
        worst[name] = assert_within_bound(pair_iou(ops, dev, a, b), exact, name)
        swapped = pair_iou(ops, dev, b[:50], a[:50])
        assert_within_bound(swapped, exact[:50], name + ' (swapped)')
    return worst


# ------------------------------------------------------------------------------------------------------------ IoU units
UNIT_SHAPES = ((0, 3), (3, 0), (1, 1), (3, 5), (65, 70))


@functools.lru_cache(maxsize=None)
def unit_case():
    """boxes of the five units (clustered, so that most pairs overlap), crowd flags, and the exact IoU blocks"""
    rng = np.random.default_rng(11)
    def mk(k):
        return np.array([box(rng.uniform(0, 120), rng.uniform(0, 120), rng.uniform(5, 80), rng.uniform(5, 80),
                             rng.uniform(-np.pi, np.pi)) for _ in range(k)], np.float64).reshape(-1, 4, 2)
    dts, gts = [mk(d) for d, _ in UNIT_SHAPES], [mk(g) for _, g in UNIT_SHAPES]
    crowds = [(rng.random(g) < 0.2).astype(np.uint8) for _, g in UNIT_SHAPES]
    exact = [ref.exact_iou_matrix(d, g, c) for d, g, c in zip(dts, gts, crowds)]
    return dts, gts, crowds, exact


def check_unit_shapes(ops, dev):
    dts, gts, crowds, exact = unit_case()
    nd, ng = np.array([d for d, _ in UNIT_SHAPES], np.int64), np.array([g for _, g in UNIT_SHAPES], np.int64)
    dt0, gt0 = np.concatenate([[0], np.cumsum(nd)[:-1]]), np.concatenate([[0], np.cumsum(ng)[:-1]])
    out0 = np.concatenate([[0], np.cumsum(nd * ng)[:-1]])
    n_iou = int((nd * ng).sum())
    units = ops.coco_units(dt0, gt0, out0, nd, ng, np.zeros(len(nd), np.int64), dev)
    crowd = torch.from_numpy(np.concatenate(crowds)).to(dev)
    got = ops.obb_iou(units, n_iou, dev_quads(np.concatenate(dts), dev), dev_quads(np.concatenate(gts), dev), crowd)
    assert got.shape == (n_iou,) and got.dtype == torch.float64
    again = ops.obb_iou(units, n_iou, dev_quads(np.concatenate(dts), dev), dev_quads(np.concatenate(gts), dev), crowd)
    assert torch.equal(got, again)                                                # a second launch: the same bits
    got = got.cpu().numpy()
    live = 0
    for u, (d, g) in enumerate(UNIT_SHAPES):
        blk = got[out0[u]:out0[u] + d * g]
        flat = [e for row in exact[u] for e in row]
        assert_within_bound(blk, flat, f'unit {d} x {g}')
        assert all((float(x) == 0.0) == (e == 0) for x, e in zip(blk, flat))     # disjoint pairs are 0.0, the others are not
        live += sum(1 for e in flat if e > 0)
    assert live > 1000
    return n_iou, live


# ----------------------------------------------------------------------------------------------------------------- NMS
def nms_boxes(n, seed):
    """n boxes spread so that a box overlaps a handful of others; scores in steps of 1 / 64 so that many tie; 3 labels"""
    rng = np.random.default_rng(seed)
    side = 40.0 * max(n, 1) ** 0.5
    q = np.array([box(rng.uniform(0, side), rng.uniform(0, side), rng.uniform(20, 90), rng.uniform(8, 40),
                      rng.uniform(-np.pi, np.pi)) for _ in range(n)], np.float64).reshape(-1, 4, 2)
    if n >= 10:                                                                   # exact duplicates and a NaN row
        q[n // 2] = q[n // 3]
        q[n - 2] = np.nan
    scores = (rng.integers(1, 64, n) / 64.0).astype(np.float32)
    labels = rng.integers(0, 3, n).astype(np.int32)
    return q, scores, labels


@functools.lru_cache(maxsize=None)
def nms_case(n, seed=0):
    """(quads, scores, labels, exact IoU matrix as Fractions) of nms_boxes, the reference made once and shared"""
    q, s, lab = nms_boxes(n, 1000 * seed + n)
    return q, s, lab, ref.exact_iou_matrix(q, q)


NMS_THRS = (0.1, 0.5)


def decision_margin(iou_rows, thrs):
    """the smallest distance of a non-trivial exact IoU to a threshold"""
    return min([abs(e - Fraction(float(t))) for row in iou_rows for e in row if e is not ref.ZERO and e != 1 for t in thrs]
               + [Fraction(1)])


def run_nms(ops, dev, q, s, lab, thr, agnostic=False):
    keep = ops.obb_nms(dev_quads(q, dev), torch.from_numpy(s).to(dev), torch.from_numpy(lab).to(dev), thr, class_agnostic=agnostic)
    assert keep.dtype == torch.int64
    return keep.cpu().tolist()


def check_nms_sizes(ops, dev, sizes=NMS_SIZES):
    kept = {}
    for n in sizes:
        q, s, lab, iou = nms_case(n)
        for thr in NMS_THRS:
            for agnostic in (False, True):
                want = ref.nms(q, s, lab, thr, agnostic, iou)
                got = run_nms(ops, dev, q, s, lab, thr, agnostic)
                assert got == want, (n, thr, agnostic, got[:10], want[:10])
            one = ref.nms(q, s, np.zeros(n, np.int32), thr, False, iou)            # one label = class_agnostic
            assert run_nms(ops, dev, q, s, np.zeros(n, np.int32), thr) == one == ref.nms(q, s, lab, thr, True, iou)
        kept[n] = len(want)
        assert run_nms(ops, dev, q, s, lab, NMS_THRS[-1], True) == got            # a second launch: the same bits
    return kept


# Sizes the exact reference cannot reach (it is quadratic in fractions): a construction whose keep lists are known in O(n).
# n = 4097 is 65 mask words, a second removal word per lane of the walk; n = 16449 is 258 > 256 words, the large form
# (csrc/nms_core.h).
NMS_GRID_SIZES = (4097, 16449)
NMS_GRID_TAIL = 100


@functools.lru_cache(maxsize=None)
def nms_grid_case(n, m=None):
    """(quads, scores, labels, keep class-aware, keep class-agnostic).  Positions 0 .. m - 1 (the head, m = n - 100) are the
    same box in distinct cells of a grid of pitch 100, position i >= m (the tail) is the box of i - m again: two boxes are
    identical or their bounds are disjoint, so every IoU is 0 or 1.  Scores do not increase with the position, in plateaus of
    130 equal values (ties across mask-word edges); a tail box scores below its twin.  Labels are i % 3 in the head; in the
    tail an even i has its twin's label and is suppressed, an odd i another one and is kept unless class_agnostic.  More
    than half of all boxes are kept, so every block of the walk propagates, and the last words of the mask hold kept boxes
    beside boxes that a box of the first two words suppresses."""
    m = n - NMS_GRID_TAIL if m is None else m
    assert NMS_GRID_TAIL <= m < n <= 2 * m
    head = np.stack([box(100.0 * (k % 128) + 50.0, 100.0 * (k // 128) + 50.0, 40, 16, 0.3) for k in range(m)])
    pos = np.arange(n)
    q = np.concatenate([head, head[:n - m]])
    scores = (1.0 - (pos // 130) / 256.0).astype(np.float32)
    assert n // 130 < 256 and m > 130                       # positive, exact in float32; a twin is on a lower plateau
    labels = (pos % 3).astype(np.int32)
    tail = pos[m:]
    labels[m:] = np.where(tail % 2 == 0, labels[tail - m], (labels[tail - m] + 1) % 3)
    aware = list(range(m)) + [int(i) for i in tail if i % 2 == 1]
    return q, scores, labels, aware, list(range(m))


def nms_grid_permuted(n, m=None, seed=5):
    """the same case with one fixed permutation applied to the inputs, so that the sort does the ordering: new position j
    holds old position perm[j]; the kept set is mapped through it and put into the canonical order of the new inputs"""
    q, s, lab, aware, agnostic = nms_grid_case(n, m)
    perm = np.random.default_rng(seed).permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    s2 = s[perm]

    def mapped(keep):
        new = inv[np.asarray(keep, np.int64)]
        return [int(j) for j in new[np.lexsort((new, -s2[new].astype(np.float64)))]]
    return q[perm], s2, lab[perm], mapped(aware), mapped(agnostic)


def check_nms_grid(ops, dev, n):
    """both input orders, both thresholds, both label modes against the known keep lists"""
    for q, s, lab, aware, agnostic in (nms_grid_case(n), nms_grid_permuted(n)):
        assert 2 * len(agnostic) > n and len(aware) == len(agnostic) + NMS_GRID_TAIL // 2
        for thr in NMS_THRS:
            got = run_nms(ops, dev, q, s, lab, thr, False)
            assert got == aware, (n, thr, len(got), len(aware), [(a, b) for a, b in zip(got, aware) if a != b][:5])
            got = run_nms(ops, dev, q, s, lab, thr, True)
            assert got == agnostic, (n, thr, len(got), len(agnostic), [(a, b) for a, b in zip(got, agnostic) if a != b][:5])
    return len(aware), len(agnostic)


def check_nms_rules(ops, dev):
    S = sq(0, 0, 4, 4)
    one = np.zeros(8, np.int32)
    f32 = lambda *v: np.array(v, np.float32)                                      # noqa: E731
    # the exact-0.5 pair: strict comparison keeps both at 0.5, one below it
    pair = np.stack([S, DIAMOND])
    assert run_nms(ops, dev, pair, f32(0.9, 0.8), one[:2], 0.5) == [0, 1]
    assert run_nms(ops, dev, pair, f32(0.9, 0.8), one[:2], 0.4999999999999999) == [0]
    assert run_nms(ops, dev, pair, f32(0.8, 0.9), one[:2], 0.25) == [1]
    # tied scores: by position
    three = np.stack([S, S + 0.5, S + 100.0])
    assert run_nms(ops, dev, three, f32(0.5, 0.5, 0.5), one[:3], 0.3) == [0, 2]
    assert run_nms(ops, dev, three[[2, 1, 0]], f32(0.5, 0.5, 0.5), one[:3], 0.3) == [0, 1]
    # a chain: A suppresses B, B would have suppressed C, so C stays
    chain = np.stack([sq(0, 0, 10, 4), sq(4, 0, 14, 4), sq(8, 0, 18, 4)])         # IoU 6 / 14, 6 / 14 and 2 / 18
    assert run_nms(ops, dev, chain, f32(0.9, 0.8, 0.7), one[:3], 0.3) == [0, 2]
    assert run_nms(ops, dev, chain, f32(0.7, 0.9, 0.8), one[:3], 0.3) == [1]
    # labels part the boxes unless class_agnostic
    assert run_nms(ops, dev, chain, f32(0.9, 0.8, 0.7), np.array([0, 1, 0], np.int32), 0.3) == [0, 1, 2]
    assert run_nms(ops, dev, chain, f32(0.9, 0.8, 0.7), np.array([0, 1, 0], np.int32), 0.3, True) == [0, 2]
    # all boxes identical: one is kept, across a mask-word edge; the first by position among equal scores
    same = np.repeat(box(30, 30, 20, 8, 0.3)[None], 130, 0)
    assert run_nms(ops, dev, same, np.full(130, 0.5, np.float32), np.zeros(130, np.int32), 0.5) == [0]
    sc = np.full(130, 0.5, np.float32)
    sc[97] = 0.75
    assert run_nms(ops, dev, same, sc, np.zeros(130, np.int32), 0.5) == [97]
    # degenerate boxes suppress nothing and are kept, in score order
    deg = np.stack([S, np.full((4, 2), np.nan), S, sq(1, 1, 1, 1), np.full((4, 2), np.nan)])
    assert run_nms(ops, dev, deg, f32(0.5, 0.9, 0.4, 0.95, 0.1), one[:5], 0.5) == [3, 1, 0, 4]


def check_refusals(ops, dev, pytest):
    S = dev_quads(np.stack([sq(0, 0, 4, 4)] * 3), dev)
    s, lab = torch.ones(3, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    crowd = torch.zeros(3, dtype=torch.uint8, device=dev)
    units = ops.coco_units([0], [0], [0], [3], [3], [0], dev)
    with pytest.raises(ValueError, match='float64'):
        ops.obb_nms(S.float(), s, lab, 0.5)
    with pytest.raises(ValueError, match=r'\[n, 4, 2\]'):
        ops.obb_nms(S.view(3, 8), s, lab, 0.5)
    with pytest.raises(ValueError, match='scores'):
        ops.obb_nms(S, s[:2], lab, 0.5)
    with pytest.raises(ValueError, match='labels'):
        ops.obb_nms(S, s, lab.long(), 0.5)
    for bad in (-0.1, float('nan')):
        with pytest.raises(ValueError, match='iou_thr'):
            ops.obb_nms(S, s, lab, bad)
    with pytest.raises(ValueError, match='float64'):
        ops.obb_iou(units, 9, S.float(), S, crowd)
    with pytest.raises(ValueError, match='gt_crowd'):
        ops.obb_iou(units, 9, S, S, crowd[:2])
    with pytest.raises(ValueError, match='units'):
        ops.obb_iou(units[:5], 9, S, S, crowd)
    edge, q = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros((2, 6), dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match='edge'):
        ops.obb_corners(edge.long(), q)
    with pytest.raises(ValueError, match='q must'):
        ops.obb_corners(edge, q[:, :5])
    with pytest.raises(ValueError, match='offsets'):
        ops.obb_corners(edge, q, torch.zeros((2, 2), dtype=torch.int64, device=dev))
    # beyond the cap: refused by the wrapper before a launch, by the entry point, and the size function says -1
    cap = ops.OBB_NMS_MAX
    assert cap == 32768
    big = torch.zeros((cap + 1, 4, 2), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match=str(cap)):
        ops.obb_nms(big, torch.zeros(cap + 1, device=dev), torch.zeros(cap + 1, dtype=torch.int32, device=dev), 0.5)
    lib = ops._lib.load()
    assert lib.rsp_obb_nms_workspace_bytes(cap + 1) == -1 and lib.rsp_obb_nms_workspace_bytes(-1) == -1
    assert lib.rsp_obb_nms_workspace_bytes(cap) >= cap * (cap // 64) * 8
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    assert lib.rsp_obb_nms(big.data_ptr(), s.data_ptr(), lab.data_ptr(), cap + 1, 0.5, 0, big.data_ptr(), big.data_ptr(),
                           cnt.data_ptr(), 0) != 0
    assert lib.rsp_obb_nms(S.data_ptr(), s.data_ptr(), lab.data_ptr(), 3, -1.0, 0, big.data_ptr(), big.data_ptr(),
                           cnt.data_ptr(), 0) != 0


def check_refuses_host_tensors(ops, pytest):
    """the wrappers refuse CPU tensors before a launch (the real ops._is_device: not under the emulator)"""
    S = torch.zeros((2, 4, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match='HIP device'):
        ops.obb_nms(S, torch.zeros(2), torch.zeros(2, dtype=torch.int32), 0.5)
    with pytest.raises(ValueError, match='HIP device'):
        ops.obb_iou(torch.zeros(32, dtype=torch.uint8), 4, S, S, torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(ValueError, match='HIP device'):
        ops.obb_corners(torch.zeros(2, dtype=torch.int32), torch.zeros((2, 6), dtype=torch.int64))


# ------------------------------------------------------------------------------------------------------------- corners
def same_doubles(got, want):
    """bit-equal float64 arrays, NaN rows in the same places"""
    g, w = got.cpu().numpy(), np.asarray(want, np.float64)
    assert g.shape == w.shape and g.dtype == np.float64, (g.shape, w.shape, g.dtype)
    assert np.array_equal(np.isnan(g), np.isnan(w))
    live = ~np.isnan(w)
    return np.array_equal(g[live].view(np.int64), w[live].view(np.int64))


def check_corners(ops, rle, dev):
    """rsp_obb_corners is bit-equal with obb_to_numpy on §14.9's case tables, without offsets and with them; the offsets
    against the rectangles of the rsp_rle_shift-ed tables"""
    H, W, masks, _ = ocases.batch_case()
    counts, n = seam_cases.rows_from_masks(masks, dev)
    edge, q = rle.runs_to_obb(counts, n, (H, W))[3:]
    k = int(edge.shape[0])
    assert int((edge < 0).sum()) >= 3 and k > 40
    want = rle.obb_to_numpy(edge, q, 'corners')
    assert same_doubles(ops.obb_corners(edge, q), want)
    assert same_doubles(rle.runs_to_obb_corners(counts, n, (H, W)), want)
    rng = np.random.default_rng(5)
    SH, SW = 8192, 9000
    offs = np.stack([rng.integers(0, SW - W + 1, k), rng.integers(0, SH - H + 1, k)], 1).astype(np.int32)
    offs[0], offs[1] = (0, 0), (SW - W, SH - H)
    off_d = torch.from_numpy(offs).to(dev)
    sc, sn, _, _ = rle.shift_runs(counts, n, off_d, (H, W), (SH, SW))
    se, sq_ = rle.runs_to_obb(sc, sn, (SH, SW))[3:]
    want = rle.obb_to_numpy(se, sq_, 'corners')
    got = ops.obb_corners(edge, q, off_d)
    assert same_doubles(got, want)
    assert same_doubles(rle.runs_to_obb_corners(counts, n, (H, W), off_d), want)
    assert ops.obb_corners(edge[:0], q[:0]).shape == (0, 4, 2)
    # the corner form is the one the IoU reads: positive orientation
    g = got.cpu().numpy()
    live = ~np.isnan(g[:, 0, 0])
    a2 = (g[:, :, 0] * np.roll(g[:, :, 1], -1, 1) - np.roll(g[:, :, 0], -1, 1) * g[:, :, 1]).sum(1)
    assert (a2[live] > 0).all()
    return k


# ----------------------------------------------------------------------------------------------------------------- API
def check_api(apis, rle, dev):
    H, W, masks, _ = ocases.batch_case()
    masks = masks[:40]
    dense = torch.from_numpy(np.stack(masks)).to(dev)
    corners = apis.masks_to_obb(dense, 'corners', device=dev)
    xywha = apis.masks_to_obb(dense, 'xywha', device=dev)
    on_masks = apis.obb_iou(dense[:10], dense[5:], device=dev)
    on_corners = apis.obb_iou(corners[:10], corners[5:], device=dev)
    assert on_masks.shape == (10, 35) and on_masks.dtype == torch.float64 and on_masks.device.type == torch.device(dev).type
    assert torch.equal(on_masks, on_corners)
    rles = rle.runs_to_masks(*rle.encode_runs(dense)[:2], (H, W), 'strings')
    assert torch.equal(apis.obb_iou(rles[:10], corners[5:], device=dev), on_masks)
    exact = ref.exact_iou_matrix(corners[:10], corners[5:])
    assert_within_bound(on_corners.cpu().numpy().reshape(-1), [e for r in exact for e in r], 'apis.obb_iou')
    d = np.diagonal(on_corners.cpu().numpy()[5:10, :5])
    live = ~np.isnan(corners[5:10, 0, 0])
    assert (np.abs(d[live] - 1.0) <= BOUND).all() and (d[~live] == 0.0).all()       # a box with itself; an empty mask with itself
    # xywha is one cos / sin away from exact: close, not equal
    on_xywha = apis.obb_iou(xywha[:10], corners[5:], device=dev).cpu().numpy()
    assert np.allclose(on_xywha, on_corners.cpu().numpy(), rtol=0, atol=1e-9)
    c2 = apis.xywha_to_corners(xywha[live.nonzero()[0] + 5])                       # the same rectangle, from another corner on
    orient = (c2[:, :, 0] * np.roll(c2[:, :, 1], -1, 1) - np.roll(c2[:, :, 0], -1, 1) * c2[:, :, 1]).sum(1)
    assert (orient > 0).all()
    for x, y in zip(c2, corners[5:10][live]):
        assert min(np.abs(np.roll(x, r, 0) - y).max() for r in range(4)) < 1e-9
    crowd = np.zeros(35, bool)
    crowd[::2] = True
    got = apis.obb_iou(corners[:10], corners[5:], iscrowd=crowd, device=dev).cpu().numpy().reshape(-1)
    exact = ref.exact_iou_matrix(corners[:10], corners[5:], crowd)
    assert_within_bound(got, [e for r in exact for e in r], 'apis.obb_iou crowd')
    assert apis.obb_iou(corners[:0], corners, device=dev).shape == (0, 40)
    # nms_rotated: the forms agree, labels part the boxes
    scores = np.linspace(0.9, 0.1, 40).astype(np.float32)
    iou = ref.exact_iou_matrix(corners, corners)
    assert decision_margin(iou, (0.05,)) > Fraction(DECISION_MARGIN)
    want = ref.nms(corners, scores, np.zeros(40, np.int32), 0.05, True, iou)
    for form in (dense, corners, torch.from_numpy(corners).to(dev), rles):
        keep = apis.nms_rotated(form, scores, iou_thr=0.05, device=dev)
        assert keep.dtype == torch.int64 and keep.cpu().tolist() == want
    lab = np.arange(40) % 2
    by_label = ref.nms(corners, scores, lab, 0.05, False, iou)
    assert apis.nms_rotated(corners, torch.from_numpy(scores), labels=lab, iou_thr=0.05, device=dev).cpu().tolist() == by_label
    assert len(want) < len(by_label) < 40
    return on_masks


def check_api_refusals(apis, dev, pytest):
    with pytest.raises(ValueError, match='corners'):
        apis.obb_iou(np.zeros((3, 4)), np.zeros((3, 4, 2)), device=dev)
    with pytest.raises(ValueError, match='iscrowd'):
        apis.obb_iou(np.zeros((3, 4, 2)), np.zeros((3, 4, 2)), iscrowd=[0, 1], device=dev)
    with pytest.raises(ValueError, match='scores'):
        apis.nms_rotated(np.zeros((3, 4, 2)), [0.5, 0.4], device=dev)


# ------------------------------------------------------------------------------------------------------------ pipeline
class OwnerStub(torch.nn.Module):
    """a detector of planted objects as tests/_seam_merge_cases.py PlantedStub, one that reports an object only from the
    tile that owns it: channel 0 of the scene holds the object id per pixel, channel 1 the owning tile's index + 1 (0: every
    tile that sees the object reports it); score = 0.9 - 0.1 id - 0.01 tile, label 0"""

    def __init__(self, scale):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.cfg = seam_cases._stub_cfg(scale)
        self.calls = 0

    def test_step(self, data):
        from rsprompter_amd.structures import InstanceData
        import _seam_merge_ref as sref
        self.calls += 1
        for x, s in zip(data['inputs'], data['data_samples']):
            th, tw = s.metainfo['ori_shape']
            tile = int(s.metainfo['img_id'])
            ids = x[0, :th, :tw].round().to(torch.int64).cpu().numpy()
            owner = x[1, :th, :tw].round().to(torch.int64).cpu().numpy()
            boxes, scores, masks = [], [], []
            for i in sorted(set(ids.reshape(-1).tolist()) - {0}):
                m = ids == i
                if int(owner[m].max()) not in (0, tile + 1):
                    continue
                boxes.append(sref.bbox_area_dense(m)[0])
                scores.append(0.9 - 0.1 * i - 0.01 * tile)
                masks.append(m)
            dev = x.device
            s.pred_instances = InstanceData(
                bboxes=torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4).to(dev),
                scores=torch.tensor(scores, dtype=torch.float32).to(dev), labels=torch.zeros(len(boxes), dtype=torch.int64).to(dev),
                masks=torch.from_numpy(np.asarray(masks, bool).reshape(-1, th, tw)).to(dev))
        return data['data_samples']


def bars_scene(duplicate=False):
    """uint8 [32, 48, 3]: 32-pixel tiles at overlap 0.5 start at x = 0 and x = 16.  Two bars at 45 degrees, three pixels
    thick, moored side by side: bar 1 on x - y = 0 inside tile 0, bar 2 on x - y = 15 inside tile 1, each owned by its tile.
    Their axis-aligned boxes have IoU 1 / 3, their oriented boxes do not meet.  duplicate=True: one short bar inside the
    band both tiles see, owned by neither: both report it in full."""
    H, W = 32, 48
    yy, xx = np.mgrid[:H, :W]
    scene = np.zeros((H, W, 3), np.uint8)
    rows = (yy >= 2) & (yy < 30)
    if duplicate:
        scene[..., 0][rows & (np.abs(xx - 18 - yy // 3) <= 1)] = 1
        return scene
    for i, (c, tile) in enumerate(((0, 0), (15, 1)), start=1):
        m = rows & (np.abs(xx - yy - c) <= 1)
        scene[..., 0][m], scene[..., 1][m] = i, tile + 1
    return scene


def check_bars(li, dev):
    """'nms' drops one of two ships moored side by side at 45 degrees -- today's behaviour, which must not change --,
    'nms_rotated' keeps both; a bar both tiles report is suppressed in both modes"""
    kw = dict(patch_size=32, patch_overlap_ratio=0.5, merge_iou_thr=0.25, batch_size=2)
    scene = bars_scene()
    ids = scene[..., 0]
    model = OwnerStub((32, 32)).to(dev)
    plain = li.inference_large_image(model, scene, merge_nms_type='nms', **kw)
    import _seam_merge_ref as sref
    b = [[float(v) for v in sref.bbox_area_dense(ids == i)[0]] for i in (1, 2)]     # the bars' tight boxes
    assert plain.pred_instances.bboxes.cpu().tolist() == b[:1] and plain.keep.cpu().tolist() == [0]
    rot, patches, start = li.inference_large_image(model, scene, merge_nms_type='nms_rotated', return_patches=True, **kw)
    assert start == [(0, 0), (16, 0)] and [len(p.pred_instances.scores) for p in patches] == [1, 1]
    p = rot.pred_instances
    assert rot.keep.cpu().tolist() == [0, 1] and p.bboxes.cpu().tolist() == b                 # both; the boxes stay axis-aligned
    assert p.scores.cpu().tolist() == patches[0].pred_instances.scores.cpu().tolist() + patches[1].pred_instances.scores.cpu().tolist()
    import _large_image_ref as lref
    from rsprompter_amd import datasets
    for i, r in enumerate(p.masks):                                                           # downstream of keep: 'nms''s
        assert np.array_equal(lref.counts_to_mask(datasets.rle_from_string(r['counts']), 32, 48), ids == i + 1)
    # the premise, on the reference: box IoU above the threshold, rotated IoU exactly 0
    quads = [np.array([[float(v) for v in c] for c in oref.corners(oref.obb(ids == i)[3])]) for i in (1, 2)]
    assert ref.exact_iou(quads[0], quads[1]) == 0
    inter = (min(b[0][2], b[1][2]) - max(b[0][0], b[1][0])) * (min(b[0][3], b[1][3]) - max(b[0][1], b[1][1]))
    area = [(v[2] - v[0]) * (v[3] - v[1]) for v in b]
    assert inter / (area[0] + area[1] - inter) > 0.3 > 0.25
    # with oriented_boxes=True the scene-table rectangles are still reported, for both
    both = li.inference_large_image(model, scene, merge_nms_type='nms_rotated', oriented_boxes=True, masks='polygons', **kw)
    assert both.pred_instances.obb.shape == (2, 4, 2) and np.allclose(both.pred_instances.obb, np.stack(quads), rtol=0, atol=1e-9)
    # merge_results_by_nms on the patch results: the same two modes
    m1 = li.merge_results_by_nms(patches, start, (32, 48), dict(type='nms', iou_threshold=0.25))
    m2 = li.merge_results_by_nms(patches, start, (32, 48), dict(type='nms_rotated', iou_threshold=0.25))
    assert len(m1.pred_instances.scores) == 1 and len(m2.pred_instances.scores) == 2
    assert m2.pred_instances.bboxes.cpu().tolist() == b and bool(m2.pred_instances.masks[1].cpu().numpy()[ids == 2].all())
    # a duplicated bar across the seam goes in both modes
    dup = bars_scene(duplicate=True)
    for mode in ('nms', 'nms_rotated'):
        out, patches, _ = li.inference_large_image(model, dup, merge_nms_type=mode, return_patches=True, **kw)
        assert [len(q.pred_instances.scores) for q in patches] == [1, 1], mode
        assert out.keep.cpu().tolist() == [0], mode


def check_pipeline_refusals(li, dev, pytest):
    class Never(OwnerStub):
        def test_step(self, data):
            raise AssertionError('the model ran')
    with pytest.raises(ValueError, match='nms_rotated'):
        li.inference_large_image(Never((32, 32)).to(dev), bars_scene(), 32, masks='dense', merge_nms_type='nms_rotated')
    never = Never((32, 32)).to(dev)
    never.with_mask = False
    with pytest.raises(ValueError, match='no masks'):
        li.inference_large_image(never, bars_scene(), 32, merge_nms_type='nms_rotated')

    class NoMasks(OwnerStub):
        def test_step(self, data):
            out = super().test_step(data)
            for s in out:
                del s.pred_instances.masks
            return out
    with pytest.raises(ValueError, match='returned none'):
        li.inference_large_image(NoMasks((32, 32)).to(dev), bars_scene(), 32, patch_overlap_ratio=0.5, merge_nms_type='nms_rotated')
    with pytest.raises(NotImplementedError, match='soft_nms'):
        li.inference_large_image(Never((32, 32)).to(dev), bars_scene(), 32, merge_nms_type='soft_nms')
    with pytest.raises(NotImplementedError):
        li.merge_results_by_nms([], [], (32, 48), dict(type='soft_nms'))


# -------------------------------------------------------------------------------------------------------------- metric
def _quad_of_ann(ann):
    """the rectangle of an annotation's mask by the sequential reference, once per annotation"""
    if '_quad' not in ann:
        c, h, w = ann['_rle']
        q = oref.obb(cref.rle_decode(c, h, w).astype(bool))[3]
        e = oref.obb(cref.rle_decode(c, h, w).astype(bool))[2]
        ann['_quad'] = np.full((4, 2), np.nan) if e < 0 else np.array([[float(v) for v in p] for p in oref.corners(q)])
    return ann['_quad']


PAIR_LOG = []                    # (exact IoU, both boxes have integer corners) of every pair that was asked for


def obb_pair_iou(dts, gts):
    out = []
    for d in dts:
        qd = _quad_of_ann(d)
        row = []
        for g in gts:
            qg = _quad_of_ann(g)
            e = ref.exact_iou(qd, qg, bool(g['iscrowd']))
            PAIR_LOG.append((e, bool(np.isfinite(qd).all() and np.isfinite(qg).all() and (qd == np.round(qd)).all()
                                     and (qg == np.round(qg)).all())))
            row.append(float(e))
        out.append(row)
    return out


def metric_margin_ok(thrs):
    """every logged exact IoU is farther than DECISION_MARGIN from every threshold (the exactly representable ties are
    check_metric_tie's and the exact table's, not this set's)"""
    for e, _ in PAIR_LOG:
        for t in thrs:
            assert abs(e - Fraction(float(t))) > Fraction(DECISION_MARGIN), (float(e), float(t))
    return 0


@functools.lru_cache(maxsize=None)
def metric_set():
    """A small set made by hand, WITHOUT product code: two image sizes, two categories, per image 14 ground truths (rotated
    ellipses drawn with numpy, compressed with the restated cocoapi) and one crowd region of whole columns, 24 detections
    (jittered ground truths, some with the other label, and spurious ellipses) -> (gt json, classes, per_img, dense masks:
    {'gt' | 'dt': [(image id, category id, iscrowd, bool [h, w])]})"""
    import _large_image_ref as lref
    rng = np.random.default_rng(42)          # (a seed whose set metric_precondition accepts: no exact IoU near a threshold)

    def rle_of(m, h, w):
        return dict(size=[h, w], counts=cref.rle_to_string([int(v) for v in lref.rle_counts_np(m)]).decode())
    images, anns, per_img, dense = [], [], {}, dict(gt=[], dt=[])
    for img_id, (h, w) in enumerate(((60, 80), (72, 64)), start=1):
        yy, xx = np.mgrid[:h, :w]

        def ellipse(cx, cy, rx, ry, ang):
            u = (xx + 0.5 - cx) * np.cos(ang) + (yy + 0.5 - cy) * np.sin(ang)
            v = -(xx + 0.5 - cx) * np.sin(ang) + (yy + 0.5 - cy) * np.cos(ang)
            return (u / rx) ** 2 + (v / ry) ** 2 <= 1.0

        def params():
            return [rng.uniform(8, w - 8), rng.uniform(8, h - 8), rng.uniform(4, 12), rng.uniform(2, 5), rng.uniform(-np.pi, np.pi)]
        images.append(dict(id=img_id, height=h, width=w, file_name=f'{img_id}.png'))
        gts = [params() for _ in range(14)]
        for j, e in enumerate(gts):
            m = ellipse(*e)
            ys, xs = np.nonzero(m)
            anns.append(dict(id=len(anns) + 1, image_id=img_id, category_id=1 + j % 2, iscrowd=0, area=float(m.sum()),
                             bbox=[int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)],
                             segmentation=rle_of(m, h, w)))
            dense['gt'].append((img_id, 1 + j % 2, 0, m))
        x0, x1 = int(0.3 * w), int(0.6 * w)
        crowd = (xx >= x0) & (xx < x1)
        anns.append(dict(id=len(anns) + 1, image_id=img_id, category_id=1, iscrowd=1, area=float(crowd.sum()),
                         bbox=[x0, 0, x1 - x0, h], segmentation=rle_of(crowd, h, w)))
        dense['gt'].append((img_id, 1, 1, crowd))
        dets = []
        for j in range(24):
            if j < 16:
                e = list(gts[j % 14])
                e[0] += rng.normal(0, 1.0)
                e[1] += rng.normal(0, 1.0)
                e[2] *= rng.uniform(0.85, 1.15)
                e[4] += rng.normal(0, 0.1)
                lab = (j % 14) % 2 if rng.random() < 0.85 else 1 - (j % 14) % 2
            else:
                e, lab = params(), int(rng.integers(2))
            m = ellipse(*e)
            ys, xs = np.nonzero(m)
            r = rle_of(m, h, w)
            dets.append(([float(xs.min()), float(ys.min()), float(xs.max() + 1), float(ys.max() + 1)],
                         float(np.round(rng.uniform(0.05, 1.0), 2)), lab, dict(size=r['size'], counts=r['counts'].encode())))
            dense['dt'].append((img_id, 1 + lab, 0, m))
        per_img[img_id] = dets
    gt = dict(images=images, annotations=anns, categories=[dict(id=1, name='a'), dict(id=2, name='b')])
    return gt, ['a', 'b'], per_img, dense


def _ref_quad(mask):
    _, _, e, q = oref.obb(mask)
    return np.full((4, 2), np.nan) if e < 0 else np.array([[float(v) for v in p] for p in oref.corners(q)])


def metric_precondition(thrs=tuple(np.linspace(.5, 0.95, 10))):
    """On the CPU, before any product call: the rectangles of the hand-made masks by the sequential reference, the exact IoU of
    every detection with every ground truth of its image and category, and the distance of each to every threshold
    (metric_margin_ok) -> (pairs, pairs inside the margin: none)"""
    dense = metric_set()[3]
    gq = [(i, c, crowd, _ref_quad(m)) for i, c, crowd, m in dense['gt']]
    dq = [(i, c, _ref_quad(m)) for i, c, _, m in dense['dt']]
    del PAIR_LOG[:]
    for i, c, qd in dq:
        for gi, gc, crowd, qg in gq:
            if (i, c) == (gi, gc):
                e = ref.exact_iou(qd, qg, bool(crowd))
                PAIR_LOG.append((e, bool(np.isfinite(qd).all() and np.isfinite(qg).all() and (qd == np.round(qd)).all()
                                         and (qg == np.round(qg)).all())))
    pairs = len(PAIR_LOG)
    return pairs, metric_margin_ok(thrs)


def check_metric(evaluation, apis, dev, tmp_path):
    import _coco_cases as cc
    import _run_morphology_cases as mcases
    cref.use_numpy_forms()
    gt, classes, per_img, _ = metric_set()
    assert len({(im['height'], im['width']) for im in gt['images']}) > 1
    ann = tmp_path / 'set.json'
    ann.write_text(json.dumps(gt))
    prefix = str(tmp_path / 'obb' / 'r')
    m = evaluation.CocoMetric(metric=['bbox', 'segm', 'obb'], device=str(dev), outfile_prefix=prefix, ann_file=str(ann),
                              iou_domain='runs')
    mcases.cic_run(m, classes, gt['images'], per_img)
    assert list(m.eval_results) == ['bbox', 'segm', 'obb']
    keys = [k for k in m.last_result if 'obb' in k]
    assert keys == [f'coco/obb_{s}' for s in ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l')]
    results = [{k: v for k, v in r.items() if k != 'bbox'} for r in json.load(open(f'{prefix}.segm.json'))]
    del PAIR_LOG[:]
    want, rev = ref.coco_stats_with_iou(cref, m.coco_gt, results, obb_pair_iou)
    got = m.eval_results['obb']
    # (test_no_exact_iou_of_the_metric_set_is_near_a_threshold holds the set clear of the thresholds, without product code)
    assert len(PAIR_LOG) > 300
    assert np.array_equal(got.stats, want), (got.stats, want)
    cc.check_tables_equal(got.tables, rev)
    assert 0.0 < got.stats[0] < 1.0
    # segm and bbox beside it are those of a call without 'obb'
    plain = evaluation.CocoMetric(metric=['bbox', 'segm'], device=str(dev), ann_file=str(ann), iou_domain='runs')
    mcases.cic_run(plain, classes, gt['images'], per_img)
    for t in ('bbox', 'segm'):
        assert np.array_equal(plain.eval_results[t].stats, m.eval_results[t].stats), t
        for k in ('dtm', 'dtig', 'npig'):
            assert np.array_equal(plain.eval_results[t].tables[k], m.eval_results[t].tables[k]), (t, k)
    assert not np.array_equal(got.stats, m.eval_results['segm'].stats)
    table = m.summary_table()
    assert '*obb*' in table and table.count('Average Precision') == 18
    return got.stats


def check_metric_tie(evaluation, dev):
    """a detection whose rectangle has IoU exactly 0.5 with the ground truth's is a match at threshold 0.5 (rsp_coco_match
    compares with >=, as pycocotools does) and none at 0.55"""
    H, W = 12, 16
    gt_m, dt_m = np.zeros((H, W), bool), np.zeros((H, W), bool)
    gt_m[2:6, 3:7] = True                                                        # [3, 7] x [2, 6]: area 16
    dt_m[2:6, 3:11] = True                                                       # [3, 11] x [2, 6]: area 32 around it
    assert ref.exact_iou(sq(3, 2, 7, 6), sq(3, 2, 11, 6)) == Fraction(1, 2)
    import _large_image_ref as lref
    rle_of = lambda m: dict(size=[H, W], counts=[int(v) for v in lref.rle_counts_np(m)])   # noqa: E731
    gt = dict(images=[dict(id=1, height=H, width=W, file_name='a.png')], categories=[dict(id=1, name='a')],
              annotations=[dict(id=1, image_id=1, category_id=1, iscrowd=0, area=16.0, bbox=[3, 2, 4, 4], segmentation=rle_of(gt_m))])
    dts = [dict(id=1, image_id=1, category_id=1, score=0.9, iscrowd=0,
                segmentation=dict(size=[H, W], counts=cref.rle_to_string(rle_of(dt_m)['counts'])))]
    gt_rle = dict(gt, annotations=[dict(gt['annotations'][0], segmentation=dict(
        size=[H, W], counts=cref.rle_to_string(rle_of(gt_m)['counts'])))])
    ev = evaluation.device_evaluate(gt_rle, dts, 'obb', [1], [1], np.array([0.5, 0.55]), [1, 10, 100], dev, keep_iou=True)
    assert ev.tables['iou'].cpu().tolist() == [0.5]
    assert ev.tables['dtm'][0].tolist() == [[1], [0]]
    segm = evaluation.device_evaluate(gt_rle, dts, 'segm', [1], [1], np.array([0.5, 0.55]), [1, 10, 100], dev, keep_iou=True)
    assert segm.tables['iou'].cpu().tolist() == [0.5] and segm.tables['dtm'][0].tolist() == [[1], [0]]
