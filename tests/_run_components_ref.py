"""The sequential definition behind the run-domain component tests (csrc/run_components.hip): a flood fill over
a dense numpy mask with the 3 x 3 structure (8-connectivity).  Nothing here imports the package.

  components(mask)  -> (labels int32 [H, W] with -1 for background, comps): the components in STREAM order (by their first
                       pixel in column-major order x H + y), each dict(area, box=(x0, y0, x1, y1) end-exclusive, first = the
                       lowest row-major index y W + x of its pixels)
  pieces(mask)      -> the column pieces [(x, y0, y1)] sorted by (x, y0)
  remove_small_regions(mask, min_area, mode) -> (mask, changed by holes, changed by islands): segment-anything's function
                       with the tie rule of rsprompter_amd.ops.remove_small_regions (all islands small: the largest stays,
                       among equals the one with the lowest row-major first pixel)
  check(mask)       -> components(mask) after its own checks: the areas sum to the population, every pixel lies in exactly one
                       component, no two components have 8-adjacent pixels; where scipy imports, the count and the sizes
                       agree with scipy.ndimage.label."""
import numpy as np

MODES = {'holes': 1, 'islands': 2, 'both': 3}
_DONE = {}                                                  # the fill of one mask is made once and shared, never changed


def components(mask):
    m = np.asarray(mask, bool)
    key = (m.shape, m.tobytes())
    if key not in _DONE:
        _DONE[key] = _fill(m)
    return _DONE[key]


def _fill(m):
    H, W = m.shape
    labels = np.full((H, W), -1, np.int32)
    comps = []
    for x in range(W):
        for y in np.flatnonzero(m[:, x] & (labels[:, x] < 0)).tolist():
            if labels[y, x] >= 0:
                continue
            c = len(comps)
            labels[y, x] = c
            stack, xs, ys = [(x, y)], [], []
            while stack:
                px, py = stack.pop()
                xs.append(px)
                ys.append(py)
                for qx in (px - 1, px, px + 1):
                    for qy in (py - 1, py, py + 1):
                        if 0 <= qx < W and 0 <= qy < H and m[qy, qx] and labels[qy, qx] < 0:
                            labels[qy, qx] = c
                            stack.append((qx, qy))
            xs, ys = np.array(xs), np.array(ys)
            comps.append(dict(area=len(xs), box=(int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1),
                              first=int((ys * W + xs).min())))
    return labels, comps


def pieces(mask):
    m = np.asarray(mask, bool)
    H, W = m.shape
    out = []
    for x in range(W):
        col = np.concatenate([[0], m[:, x].astype(np.int8), [0]])
        d = np.diff(col)
        out += [(x, int(a), int(b)) for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))]
    return out


def _pass(m, min_area, holes):
    labels, comps = components(~m if holes else m)
    small = [c for c, d in enumerate(comps) if d['area'] < min_area]
    if not small:
        return m, False
    if holes:
        return m | np.isin(labels, small), True
    keep = [c for c, d in enumerate(comps) if d['area'] >= min_area]
    if not keep:
        keep = [max(range(len(comps)), key=lambda c: (comps[c]['area'], -comps[c]['first']))]
    return np.isin(labels, keep), True


def remove_small_regions(mask, min_area, mode='both'):
    m = np.asarray(mask, bool).copy()
    bits = MODES[mode]
    ch = cs = False
    if bits & 1:
        m, ch = _pass(m, min_area, True)
    if bits & 2:
        m, cs = _pass(m, min_area, False)
    return m, ch, cs


def check(mask):
    m = np.asarray(mask, bool)
    H, W = m.shape
    labels, comps = components(m)
    assert sum(d['area'] for d in comps) == int(m.sum())
    assert ((labels >= 0) == m).all() and (np.bincount(labels[m], minlength=len(comps)) == [d['area'] for d in comps]).all()
    firsts = [min(x * H + y for y, x in zip(*np.nonzero(labels == c))) for c in range(len(comps))] if len(comps) <= 64 else None
    assert firsts is None or firsts == sorted(firsts)
    pad = np.full((H + 2, W + 2), -1, np.int32)
    pad[1:-1, 1:-1] = labels
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            nb = pad[dy:dy + H, dx:dx + W]
            both = (labels >= 0) & (nb >= 0)
            assert (labels[both] == nb[both]).all()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        lab, cnt = ndimage.label(m, structure=np.ones((3, 3), int))
        assert cnt == len(comps)
        assert sorted(np.bincount(lab[m], minlength=cnt + 1)[1:].tolist()) == sorted(d['area'] for d in comps)
    return labels, comps
