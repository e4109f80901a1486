"""TEST ORACLE of the Euclidean buffers: morphology by the exact disc dx^2 + dy^2 <= r2 (and the diamond
|dx| + |dy| <= r) on DENSE numpy masks, in two independent forms that must agree before either is used (every call asserts
it):
  scipy.ndimage.binary_dilation / binary_erosion with the boolean footprint;
  the integer squared distances to the nearest set (unset) pixel, from the indices of distance_transform_edt, thresholded
  at r2 (the diamond: r iterations of the 4-neighbour cross).
Nothing here is on the product path."""
import math

import numpy as np
from scipy import ndimage as ndi

CROSS = ndi.generate_binary_structure(2, 1)


def clamp_r2(r2, shape):
    return min(int(r2), shape[0] ** 2 + shape[1] ** 2)          # beyond the diagonal nothing changes


def footprint(r2):
    R = math.isqrt(int(r2))
    d = np.arange(-R, R + 1)
    return d[:, None] ** 2 + d[None, :] ** 2 <= int(r2)


def diamond_footprint(r):
    d = np.arange(-int(r), int(r) + 1)
    return np.abs(d)[:, None] + np.abs(d)[None, :] <= int(r)


def dist2(mask):
    """the squared Euclidean distance of every pixel to the nearest SET pixel of mask, in integers; None for an empty mask"""
    m = np.asarray(mask, bool)
    if not m.any():
        return None
    iy, ix = ndi.distance_transform_edt(~m, return_distances=False, return_indices=True)
    yy, xx = np.indices(m.shape)
    return (iy - yy).astype(np.int64) ** 2 + (ix - xx).astype(np.int64) ** 2


def dilate(mask, r2):
    m = np.asarray(mask, bool)
    r2 = clamp_r2(r2, m.shape)
    a = ndi.binary_dilation(m, footprint(r2))
    d2 = dist2(m)
    b = np.zeros_like(m) if d2 is None else d2 <= r2
    assert np.array_equal(a, b), 'the two forms of the oracle disagree (dilate)'
    return a


def erode(mask, r2, border=0):
    m = np.asarray(mask, bool)
    r2 = clamp_r2(r2, m.shape)
    R = math.isqrt(r2)
    a = ndi.binary_erosion(m, footprint(r2), border_value=int(border))
    pad = np.pad(m, R, constant_values=bool(border))           # a ring as wide as the radius: what lies farther cannot matter
    d2 = dist2(~pad)                                           # to the nearest pixel outside the mask
    b = (np.ones_like(pad) if d2 is None else d2 > r2)[R:R + m.shape[0], R:R + m.shape[1]]
    assert np.array_equal(a, b), 'the two forms of the oracle disagree (erode)'
    return a


def opening(mask, r2):
    return dilate(erode(mask, r2, 0), r2)


def closing(mask, r2):
    return erode(dilate(mask, r2), r2, 1)


def boundary(mask, r2):
    m = np.asarray(mask, bool)
    return m & ~erode(m, r2, 0)


OPS = dict(erode=lambda m, r2: erode(m, r2, 0), dilate=dilate, open=opening, close=closing, boundary=boundary)


def diamond_dilate(mask, r):
    m = np.asarray(mask, bool)
    if r == 0:
        return m.copy()
    a = ndi.binary_dilation(m, diamond_footprint(r))
    assert np.array_equal(a, ndi.binary_dilation(m, CROSS, iterations=int(r))), 'the two forms disagree (diamond dilate)'
    return a


def diamond_erode(mask, r, border=0):
    m = np.asarray(mask, bool)
    if r == 0:
        return m.copy()
    a = ndi.binary_erosion(m, diamond_footprint(r), border_value=int(border))
    pad = np.pad(m, int(r), constant_values=bool(border))
    b = ndi.binary_erosion(pad, CROSS, iterations=int(r), border_value=int(border))[r:r + m.shape[0], r:r + m.shape[1]]
    assert np.array_equal(a, b), 'the two forms disagree (diamond erode)'
    return a


def buffer(mask, d2):
    """the signed buffer by a distance given as its SIGNED squared radius: > 0 dilate, < 0 erode with the outside set"""
    return dilate(mask, d2) if d2 >= 0 else erode(mask, -d2, 1)


def dilate_cropped(mask, r2):
    """`dilate` on the mask's bounding box grown by R alone (scene-sized masks): farther away nothing is reached"""
    m = np.asarray(mask, bool)
    out = np.zeros_like(m)
    R = math.isqrt(int(r2))
    ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
    if ys.size:
        sl = (slice(max(ys[0] - R, 0), ys[-1] + 1 + R), slice(max(xs[0] - R, 0), xs[-1] + 1 + R))
        out[sl] = dilate(m[sl], r2)
    return out


def erode_cropped(mask, r2, border):
    """`erode` on the bounding box: inside it the outside of the box is background unless it is the outside of the canvas"""
    m = np.asarray(mask, bool)
    out = np.zeros_like(m)
    R = math.isqrt(int(r2))
    ys, xs = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
    if ys.size:
        y0, y1, x0, x1 = max(ys[0] - R, 0), min(ys[-1] + 1 + R, m.shape[0]), max(xs[0] - R, 0), min(xs[-1] + 1 + R, m.shape[1])
        pad = np.full((y1 - y0 + 2 * R, x1 - x0 + 2 * R), False)
        if border:                                               # the sides of the box that ARE the canvas edge count as set
            pad[:R if y0 == 0 else 0, :] = True
            pad[pad.shape[0] - R if y1 == m.shape[0] else pad.shape[0]:, :] = True
            pad[:, :R if x0 == 0 else 0] = True
            pad[:, pad.shape[1] - R if x1 == m.shape[1] else pad.shape[1]:] = True
        pad[R:R + y1 - y0, R:R + x1 - x0] = m[y0:y1, x0:x1]
        e = ndi.binary_erosion(pad, footprint(r2), border_value=0)[R:R + y1 - y0, R:R + x1 - x0]
        out[y0:y1, x0:x1] = e & m[y0:y1, x0:x1]
    return out
