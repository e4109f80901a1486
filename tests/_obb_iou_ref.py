"""The reference of the oriented-box comparison.  Imports nothing from rsprompter_amd.

THE DEFINITION is `exact_iou`: a box is four float64 corners, a float64 is a rational, so the intersection of two convex
quadrilaterals (Sutherland-Hodgman, one box clipped by the four half-planes of the other, then the shoelace sum) and the
quotient inter / union are computed in fractions.Fraction without any rounding; float(exact_iou) rounds once.

`twin_iou` is the same procedure in float64, operation by operation as csrc/obb_iou.hip orders it (Python floats are IEEE
doubles and never fuse).  It exists ONLY to size the tolerance of the tests (tests/_obb_iou_cases.py BOUND): how far a
float64 evaluation of this method lies from the exact value.  Nothing is ever compared with the twin.

A box whose corners are not all finite or whose area is zero is DEGENERATE: IoU 0 with everything, suppresses nothing, kept.
`nms` is mmcv's nms_rotated rule stated sequentially, `coco_stats_with_iou` pycocotools' evaluation (tests/_cocoeval_ref.py)
fed IoU blocks of the caller's."""
import math
from fractions import Fraction

import numpy as np


# ------------------------------------------------------------------------------------------------------------- exact
def _frac_box(box):
    """float64 [4, 2] -> (corners as Fractions in positive orientation, doubled area) or None when degenerate"""
    b = np.asarray(box, np.float64).reshape(4, 2)
    if not np.isfinite(b).all():
        return None
    p = [(Fraction(float(x)), Fraction(float(y))) for x, y in b.tolist()]
    a2 = sum(p[i][0] * p[(i + 1) % 4][1] - p[(i + 1) % 4][0] * p[i][1] for i in range(4))
    if a2 == 0:
        return None
    if a2 < 0:
        p = [p[0], p[3], p[2], p[1]]
        a2 = -a2
    return p, a2


def _clip(poly, p, q):
    """the part of the convex polygon on the left of (or on) the line p -> q"""
    ex, ey = q[0] - p[0], q[1] - p[1]
    out = []
    m = len(poly)
    for i in range(m):
        v, u = poly[i - 1], poly[i]
        dv = ex * (v[1] - p[1]) - ey * (v[0] - p[0])
        du = ex * (u[1] - p[1]) - ey * (u[0] - p[0])
        if (du >= 0) != (dv >= 0):
            den = dv - du
            out.append(((u[0] * dv - v[0] * du) / den, (u[1] * dv - v[1] * du) / den))
        if du >= 0:
            out.append(u)
    return out


def exact_inter2(A, B):
    """the doubled area of the intersection of two boxes as _frac_box returns them"""
    poly = list(B[0])
    for i in range(4):
        if not poly:
            return Fraction(0)
        poly = _clip(poly, A[0][i], A[0][(i + 1) % 4])
    if len(poly) < 3:
        return Fraction(0)
    return sum(poly[i - 1][0] * poly[i][1] - poly[i][0] * poly[i - 1][1] for i in range(len(poly)))


def exact_iou(a, b, crowd=False):
    """the IoU of two boxes float64 [4, 2] as a Fraction: inter / (area_a + area_b - inter), inter / area_a for a crowd b"""
    A, B = _frac_box(a), _frac_box(b)
    if A is None or B is None:
        return Fraction(0)
    inter2 = exact_inter2(A, B)
    if inter2 <= 0:
        return Fraction(0)
    un2 = A[1] if crowd else A[1] + B[1] - inter2
    return inter2 / un2 if un2 > 0 else Fraction(0)


ZERO = Fraction(0)


def exact_iou_matrix(a, b, crowd=None):
    """[len(a)][len(b)] Fractions.  Pairs whose axis-aligned bounds do not overlap (float comparisons are exact) share no
    area and are ZERO without clipping; with a is b and no crowd the matrix is symmetric and half of it is computed."""
    same = a is b and crowd is None
    a, b = np.asarray(a, np.float64).reshape(-1, 4, 2), np.asarray(b, np.float64).reshape(-1, 4, 2)
    crowd = [False] * len(b) if crowd is None else list(crowd)
    A, B = [_frac_box(x) for x in a], ([_frac_box(y) for y in b] if not same else None)
    B = A if same else B
    with np.errstate(invalid='ignore'):
        alo, ahi, blo, bhi = a.min(1), a.max(1), b.min(1), b.max(1)
    out = [[ZERO] * len(b) for _ in range(len(a))]
    for i in range(len(a)):
        if A[i] is None:
            continue
        with np.errstate(invalid='ignore'):
            hit = (ahi[i, 0] > blo[:, 0]) & (bhi[:, 0] > alo[i, 0]) & (ahi[i, 1] > blo[:, 1]) & (bhi[:, 1] > alo[i, 1])
        for j in np.nonzero(hit)[0].tolist():
            if B[j] is None:
                continue
            if same and j < i:
                out[i][j] = out[j][i]
                continue
            inter2 = exact_inter2(A[i], B[j])
            if inter2 > 0:
                un2 = A[i][1] if crowd[j] else A[i][1] + B[j][1] - inter2
                out[i][j] = inter2 / un2
    return out


# -------------------------------------------------------------------------------------------------------- float64 twin
def _twin_box(box):
    b = [float(v) for v in np.asarray(box, np.float64).reshape(-1)]
    finite = all(math.isfinite(v) for v in b)
    x, y = b[0::2], b[1::2]
    d1x, d1y, d2x, d2y, d3x, d3y = x[1] - x[0], y[1] - y[0], x[2] - x[0], y[2] - y[0], x[3] - x[0], y[3] - y[0]
    if not finite:
        return x, y, 0.0
    a2 = (d1x * d2y - d1y * d2x) + (d2x * d3y - d2y * d3x)
    if a2 < 0.0:
        x[1], x[3], y[1], y[3] = x[3], x[1], y[3], y[1]
        a2 = -a2
    return x, y, (a2 if a2 > 0.0 else 0.0)


def twin_iou(a, b, crowd=False):
    """float64, in the kernel's order of operations (csrc/obb_iou.hip oi_iou); sizes the tolerance, nothing else"""
    ax, ay, a2 = _twin_box(a)
    bx, by, b2 = _twin_box(b)
    if a2 == 0.0 or b2 == 0.0:
        return 0.0
    if max(ax) <= min(bx) or max(bx) <= min(ax) or max(ay) <= min(by) or max(by) <= min(ay):
        return 0.0
    cx, cy = (ax[0] + ax[1] + ax[2] + ax[3]) * 0.25, (ay[0] + ay[1] + ay[2] + ay[3]) * 0.25
    ax, ay = [v - cx for v in ax], [v - cy for v in ay]
    poly = [(bx[i] - cx, by[i] - cy) for i in range(4)]
    for e in range(4):
        px, py = ax[e], ay[e]
        ex, ey = ax[(e + 1) & 3] - px, ay[(e + 1) & 3] - py
        out = []
        if poly:
            vx, vy = poly[-1]
            dv = ex * (vy - py) - ey * (vx - px)
            for ux, uy in poly:
                du = ex * (uy - py) - ey * (ux - px)
                if (du >= 0.0) != (dv >= 0.0):
                    den = dv - du
                    out.append(((ux * dv - vx * du) / den, (uy * dv - vy * du) / den))
                if du >= 0.0:
                    out.append((ux, uy))
                vx, vy, dv = ux, uy, du
        poly = out[:8]
    if len(poly) < 3:
        return 0.0
    s = 0.0
    vx, vy = poly[-1]
    for ux, uy in poly:
        s += vx * uy - ux * vy
        vx, vy = ux, uy
    inter = 0.5 * s
    if not inter > 0.0:
        return 0.0
    aa, ab = 0.5 * a2, 0.5 * b2
    un = aa if crowd else aa + ab - inter
    return inter / un if un > 0.0 else 0.0


# ----------------------------------------------------------------------------------------------------------------- NMS
def nms(quads, scores, labels, thr, class_agnostic=False, iou=None):
    """mmcv nms_rotated stated sequentially: order by score descending, position ascending; a box is dropped iff a KEPT box
    ahead of it has its label (or class_agnostic) and iou > thr (strict, compared exactly: thr is a float, so a rational).
    iou: a matrix of Fractions over the input positions (exact_iou_matrix), made here when None.  -> kept input positions"""
    n = len(quads)
    if iou is None:
        iou = exact_iou_matrix(quads, quads)
    s = np.asarray(scores, np.float32)
    order = sorted(range(n), key=lambda i: (-float(s[i]), i))
    t = thr if isinstance(thr, Fraction) else Fraction(float(thr))
    keep = []
    for j in order:
        if not any((class_agnostic or int(labels[i]) == int(labels[j])) and iou[i][j] > t for i in keep):
            keep.append(j)
    return keep


# -------------------------------------------------------------------------------------------------------------- metric
def coco_stats_with_iou(cref, gt_json, results, pair_iou, **kw):
    """tests/_cocoeval_ref.py's COCOeval on `results` (segm results) with computeIoU replaced: the IoU block of (image,
    category) is pair_iou(dts, gts) -> [len(dts)][len(gts)] floats for the score-sorted, truncated detections and the
    ground truths as COCOeval hands them over (annotation dicts).  Everything else -- evaluateImg, accumulate, summarize --
    is the restated pycocotools.  -> stats"""
    class Swapped(cref.COCOeval):
        def computeIoU(self, imgId, catId):
            p = self.params
            gt = self._gts[imgId, catId]
            dt = self._dts[imgId, catId]
            if len(gt) == 0 and len(dt) == 0:
                return []
            inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
            dt = [dt[i] for i in inds]
            if len(dt) > p.maxDets[-1]:
                dt = dt[0:p.maxDets[-1]]
            if len(dt) == 0 or len(gt) == 0:
                return []
            return np.asarray(pair_iou(dt, gt), np.float64).reshape(len(dt), len(gt))
    orig = cref.COCOeval
    cref.COCOeval = Swapped
    try:
        return cref.coco_stats(gt_json, results, 'segm', **kw)
    finally:
        cref.COCOeval = orig
