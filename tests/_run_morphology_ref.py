"""TEST ORACLE of the run-domain morphology: square erosion and what is built from it on DENSE numpy masks,
in two independent forms that must agree before either is used (`erode` asserts it on every call):
  the literal form -- the mask inside a ring of `border`, then `r` times the 3 x 3 minimum with +inf (all ones) outside;
  scipy.ndimage.binary_erosion / binary_dilation with a 3 x 3 structuring element, `iterations=r`.
Boundary IoU is the paper's (Cheng et al., CVPR 2021): the IoU of the bands M & ~erode(M, d, border=0), d from the image
diagonal.  Nothing here is on the product path."""
import math

import numpy as np
from scipy import ndimage as ndi

ONES3 = np.ones((3, 3), bool)


def erode_literal(mask, r, border=0):
    m = np.asarray(mask, bool)
    h, w = m.shape
    r = min(int(r), max(h, w))                                 # beyond the canvas nothing changes
    pad = np.full((h + 2 * r, w + 2 * r), bool(border))      # a ring as wide as the radius: what happens outside stays outside
    pad[r:r + h, r:r + w] = m
    for _ in range(r):
        p = np.ones((pad.shape[0] + 2, pad.shape[1] + 2), bool)
        p[1:-1, 1:-1] = pad
        out = np.ones_like(pad)
        for dy in range(3):
            for dx in range(3):
                out &= p[dy:dy + pad.shape[0], dx:dx + pad.shape[1]]
        pad = out
    return pad[r:r + h, r:r + w]


def erode(mask, r, border=0):
    m = np.asarray(mask, bool)
    if r == 0:
        return m.copy()
    a = ndi.binary_erosion(m, ONES3, iterations=int(min(r, max(m.shape))), border_value=int(border))
    b = erode_literal(m, r, border)
    assert np.array_equal(a, b), 'the two forms of the oracle disagree'
    return a


def erode_separable(mask, r, border=0):
    """a third form, linear in the pixels whatever r is: the running minimum over 2 r + 1 rows, then over 2 r + 1 columns,
    `border` outside.  For scene-sized masks; the oracle cases compare it with `erode` before anything uses it."""
    m = np.asarray(mask, np.uint8)
    if r == 0:
        return m.astype(bool)
    for axis in (0, 1):
        m = ndi.minimum_filter1d(m, 2 * int(min(r, max(m.shape))) + 1, axis=axis, mode='constant', cval=int(border))
    return m.astype(bool)


def dilate(mask, r):
    m = np.asarray(mask, bool)
    if r == 0:
        return m.copy()
    a = ndi.binary_dilation(m, ONES3, iterations=int(min(r, max(m.shape))))
    assert np.array_equal(a, ~erode(~m, r, 1)), 'dilation is not the complement of the erosion of the complement'
    return a


def opening(mask, r):
    return dilate(erode(mask, r, 0), r)


def closing(mask, r):
    return erode(dilate(mask, r), r, 1)


def boundary(mask, r):
    m = np.asarray(mask, bool)
    return m & ~erode(m, r, 0)


OPS = dict(erode=lambda m, r: erode(m, r, 0), dilate=dilate, open=opening, close=closing, boundary=boundary)


def radius(hw, dilation_ratio=0.02):
    return max(1, int(round(dilation_ratio * math.sqrt(hw[0] * hw[0] + hw[1] * hw[1]))))


def iou(a, b, crowd=False):
    """maskUtils.iou of two dense masks: 0.0 without a common pixel, / |a| for a crowd b"""
    inter = int((a & b).sum())
    if inter == 0:
        return 0.0
    return inter / (int(a.sum()) if crowd else int(a.sum()) + int(b.sum()) - inter)


def boundary_iou(dt, gt, crowd=False, dilation_ratio=0.02, r=None):
    r = radius(dt.shape, dilation_ratio) if r is None else r
    return iou(boundary(dt, r), boundary(gt, r), crowd)


def boundary_cropped(mask, r, separable=False):
    """`boundary` computed on the mask's bounding box alone: outside it there is background or the image border, which the
    erosion with border 0 reads alike, so the result is the same (the boundary_iou cases compare them); for scene-sized masks"""
    m = np.asarray(mask, bool)
    out = np.zeros_like(m)
    ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
    if ys.size:
        sl = (slice(ys[0], ys[-1] + 1), slice(xs[0], xs[-1] + 1))
        out[sl] = m[sl] & ~erode_separable(m[sl], r, 0) if separable else boundary(m[sl], r)
    return out
