"""Evaluation hand-off: `encode_mask_results` of the reference
(mmdet/structures/mask/utils.py:38-53 -> pycocotools.mask.encode): run-length counting (`rsp_mask_rle`) and the
compression of the counts to COCO's ASCII string (cocoapi maskApi.c rleToString -> `rsp_rle_to_string`) both run on the
GPU; the host receives finished strings.  The result is what CocoMetric.process stores per instance
(coco_metric.py:346-391): dict(size=[h, w], counts=bytes).

This module is also the one home of the RUN TABLE that every mask leaves the device as: counts int32
[k, cap] + n int32 [k], the column-major COCO stream with zeros as the first run, written by producers that never read the
host and report a row that did not fit as n[i] = -(slots needed).  The retry on run capacity is `ops.fit_runs`, the retry on
string bytes (offs[k] > flat_cap: again with flat_cap = offs[k]) is `_string_bytes`; the features call the pipelines below
and hold no capacity loop of their own.  The run table is also where the VECTOR form starts: runs_to_polygons
turns it into exact rings on the device, simplify_polygons thins them there, polygons_to_lists brings them
to the host in one transfer.

The section "mask forms" below is the one home of the conversions between a CALLER'S masks (a dense bool tensor, RLE dicts
with compressed or with uncompressed counts) and the run table, in both directions (DESIGN §14 "Mask forms"): masks_to_runs
(over encode_runs, strings_to_runs, lists_to_runs, check_canonical) on the way in, runs_to_masks (over runs_to_dense,
runs_to_strings, runs_to_dicts) on the way out, runs_to_bits for the bit planes of the COCO IoU.  The caller-facing
functions of apis.py and evaluation.py check their own arguments and call these; ops.rle_from_string and ops.rle_to_bits
have no other caller in the package."""
import math

import numpy as np
import torch

from . import ops


def counts_to_string(cnts):
    """rleToString on a Python list (the definition the device kernel is tested against; not on the product path)."""
    out = bytearray()
    for i, x in enumerate(cnts):
        if i > 2:
            x -= cnts[i - 2]
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(c + 48)
    return bytes(out)


_counts_to_string = counts_to_string      # round-2 name


def encode_runs(masks, cap=4096):
    """bool [k, H, W] on the device -> (counts int32 [k, widest row] (a copy: the [k, cap] buffer goes; two columns at least,
    which rsp_rle_to_string asks for), n int32 [k], n on the host, the capacity that fit): rsp_mask_rle, one device-to-host
    read (n) per attempt."""
    ops.require_device(masks.device)
    counts, n, n_host, cap = ops.fit_runs(ops.mask_rle_launcher(masks), cap)
    width = max(int(n_host.max()) if n_host.numel() else 0, 2)
    return counts[:, :width].clone(), n, n_host, cap


def shift_runs(counts, n, offsets, tile_hw, scene_hw, cap=None):
    """tile run tables placed at offsets (int32 [k, 2] = (ox, oy), device) in the scene (rsp_rle_shift) -> (scene counts,
    scene n, n on the host, cap); one device-to-host read per attempt."""
    if cap is None:     # a column end inside a run adds at most one ones-run and one zero run: n_in + 2 w bounds the scene's runs
        cap = int(counts.shape[1]) + 2 * int(tile_hw[1]) + 2
    return ops.fit_runs(lambda cap: ops.rle_shift(counts, n, offsets, tile_hw, scene_hw, cap), cap)


def union_runs(counts, n, scene_hw, group_offs, members, cap=None):
    """the union of the member rows of every group as one run table (ops.rle_union's arguments) -> (counts, n, n on the
    host, cap); per attempt one device-to-host read and the one inside ops.rle_union.  cap=None reads the bound once."""
    if cap is None:     # the union of a group has at most as many runs as its members together
        runs = n[members.to(torch.int64)].clamp(min=1).to(torch.int64)
        csum = torch.cat([runs.new_zeros((1,)), torch.cumsum(runs, 0)])
        o64 = group_offs.to(torch.int64)
        cap = max(int((csum[o64[1:]] - csum[o64[:-1]]).max().item()) + 1, 2) if o64.shape[0] > 1 else 2
    return ops.fit_runs(lambda cap: ops.rle_union(counts, n, scene_hw[0], scene_hw[1], group_offs, members, cap), cap)


def concat_runs(tables, rows=None, device=None):
    """run tables int32 [k_i, w_i] -> one zero-padded table [sum k_i, widest] (at least one column), or with `rows` (int64,
    device: row numbers of the concatenation, any order) only those rows, gathered table by table.  `device` places the
    result of an empty list."""
    dev = tables[0].device if tables else device
    width = max([int(t.shape[1]) for t in tables] + [1])
    total = sum(int(t.shape[0]) for t in tables)
    out = torch.zeros((total if rows is None else int(rows.shape[0]), width), dtype=torch.int32, device=dev)
    r0 = 0
    for t in tables:
        if rows is None:
            out[r0:r0 + t.shape[0], :t.shape[1]] = t
        else:
            sel = ((rows >= r0) & (rows < r0 + t.shape[0])).nonzero().view(-1)
            out[sel, :t.shape[1]] = t[rows[sel] - r0]
        r0 += t.shape[0]
    return out


def _string_bytes(counts, n, flat_cap):
    """run table -> (flat uint8, offs int64 [k + 1]) on the HOST: string i is flat[offs[i]:offs[i + 1]]
    (rsp_rle_to_string).  One device-to-host read (offs) per attempt, then the bytes."""
    k = int(n.shape[0])
    while True:
        _, offs, flat = ops.rle_to_string(counts, n, k, flat_cap)
        offs_h = offs.cpu()
        total = int(offs_h[-1])
        if total <= flat_cap:
            return flat[:total].cpu(), offs_h
        flat_cap = total


def runs_to_strings(counts, n, size, flat_cap=None):
    """run table -> list of dict(size=[H, W], counts=bytes), COCO's compressed form.  `flat_cap`: the first guess of the
    strings' bytes (two per table entry when None)."""
    k = int(n.shape[0])
    if k == 0:
        return []
    flat, offs = _string_bytes(counts, n, flat_cap or 2 * k * int(counts.shape[1]) + 16)
    buf, o = flat.numpy().tobytes(), offs.tolist()
    return [dict(size=[int(size[0]), int(size[1])], counts=buf[o[i]:o[i + 1]]) for i in range(k)]


def runs_to_polygons(counts, n, size):
    """run table of k masks on one size = (H, W) canvas -> (verts int32 [V, 2], ring_offs int64 [R + 1], ring_inst int32 [R],
    ring_parent int32 [R], ring_area2 int64 [R], inst_ring_offs int64 [k + 1]) on the device: the rings of DESIGN §14.7
    (ops.mask_polygons).  Three device-to-host reads, whatever k is."""
    return ops.mask_polygons(counts, n, size[0], size[1])


def polygon_tolerance_q8(tolerance):
    """a simplification tolerance in pixels -> tol2_q8 = round(256 tolerance^2), the integer every distance is compared with
    (DESIGN §14.8); refuses what is negative, not finite, or above 2^40 (65 536 px)"""
    try:
        t = float(tolerance)
    except (TypeError, ValueError):
        raise ValueError(f'a simplification tolerance is a number of pixels, got {tolerance!r}') from None
    if isinstance(tolerance, bool) or not math.isfinite(t) or t < 0:
        raise ValueError(f'a simplification tolerance is a finite number of pixels >= 0, got {tolerance!r}')
    q8 = int(round(t * t * 256))
    if q8 > ops.RING_SIMPLIFY_MAX_TOL2_Q8:
        raise ValueError(f'a simplification tolerance of {tolerance!r} px: 256 tolerance^2 is at most 2^40 (65 536 px)')
    return q8


def polygon_min_ring_area(min_ring_area):
    """min_ring_area as the non-negative integer of pixels ops.ring_simplify takes (a float with an integer value passes)"""
    a = min_ring_area
    if isinstance(a, bool) or not isinstance(a, (int, float, np.integer, np.floating)) or not math.isfinite(a) or a < 0 \
            or a != int(a):
        raise ValueError(f'min_ring_area is a non-negative integer number of pixels, got {min_ring_area!r}')
    return int(a)


def simplify_polygons(polys, size, tolerance, min_ring_area=0):
    """what runs_to_polygons returns, on a size = (H, W) canvas -> (the six arrays of the simplified rings, ring_src int32
    [R']) on the device: exact Douglas-Peucker at `tolerance` pixels (distance to the segment between the kept vertices
    around a vertex; tolerance^2 is quantised to 1 / 256 px^2), rings of less than min_ring_area pixels (before
    simplification) dropped, with the holes of a dropped outer ring (ops.ring_simplify).  ring_src[r] = the
    input ring that output ring r was.  One device-to-host read."""
    out = ops.ring_simplify(*polys, polygon_tolerance_q8(tolerance), polygon_min_ring_area(min_ring_area), size[0], size[1])
    return out[:6], out[6]


POLYGON_TOPOLOGIES = ('rings', 'shared')


def polygon_topology(topology, tolerance, min_ring_area):
    """the `topology` of the polygon outputs with the options that go with it -> True for 'shared' (DESIGN §14.15), which
    requires a tolerance (0 is legal: the noded exact rings) and min_ring_area == 0"""
    if topology not in POLYGON_TOPOLOGIES:
        raise ValueError(f'polygon topology {topology!r}: one of {POLYGON_TOPOLOGIES}')
    if topology == 'rings':
        return False
    if tolerance is None:
        raise ValueError("topology='shared' simplifies shared borders and requires a tolerance (0 gives the exact rings "
                         'with their nodes)')
    polygon_tolerance_q8(tolerance)
    if polygon_min_ring_area(min_ring_area) != 0:
        raise ValueError("topology='shared' requires min_ring_area == 0: a ring dropped by its area would leave its pixels "
                         'to nobody, and the layer would have a gap again')
    return True


def simplify_coverage(counts, n, size, tolerance):
    """run table of k masks on one size = (H, W) canvas whose rows are pairwise disjoint and canonical (what flatten_runs
    returns) -> (the six arrays of the simplified rings, ring_src int32 [R'], vert_other int32 [V']) on the device:
    shared-border simplification at `tolerance` pixels (ops.ring_coverage).  A border between two instances
    keeps the same vertices in both rings, every node (T-junctions, points where three or four regions or two and the canvas
    border meet, saddles) is a vertex, and a ring begins at its first node visit, not at its smallest vertex (a ring without a
    node stays there).  vert_other[v] = the instance on the far side of the edge that leaves vertex v, -1 for background.
    Arcs of different borders may still cross each other at large tolerances.  Overlapping or non-canonical rows raise
    ValueError.  Five device-to-host reads (one when the table has no piece)."""
    out = ops.ring_coverage(counts, n, size[0], size[1], polygon_tolerance_q8(tolerance))
    return out[:6], out[6], out[7]


def polygons_to_lists(verts, ring_offs, ring_inst, ring_parent, ring_area2, inst_ring_offs):
    """what runs_to_polygons returns -> per instance a list of (ring int32 ndarray [m, 2] = (x, y), parent, area2) on the
    host, after ONE transfer (the five arrays that are read, packed into one int64 buffer)."""
    sizes = [int(verts.numel()), int(ring_offs.numel()), int(ring_parent.numel()), int(ring_area2.numel()),
             int(inst_ring_offs.numel())]
    buf = torch.cat([verts.reshape(-1).to(torch.int64), ring_offs, ring_parent.to(torch.int64), ring_area2,
                     inst_ring_offs]).cpu().numpy()
    v, ro, par, a2, io = np.split(buf, np.cumsum(sizes)[:-1])
    v = v.astype(np.int32).reshape(-1, 2)
    ro, par, a2, io = ro.tolist(), par.tolist(), a2.tolist(), io.tolist()
    return [[(v[ro[r]:ro[r + 1]], par[r], a2[r]) for r in range(io[i], io[i + 1])] for i in range(len(io) - 1)]


POLYGON_FILLS = ('union', 'evenodd')


def polygons_to_runs(verts, ring_offs, ring_group, group_hw, fill='union', cap=None):
    """Rings -> the run table of G masks, every one on its own canvas (ops.poly_raster): verts float64 [V, 2] =
    (x, y), ring_offs int64 [R + 1], ring_group int32 [R] (the instance of each ring, non-decreasing), group_hw int32 [G, 2] =
    (h, w) per instance, on one device -> (counts int32 [G, cap'], n int32 [G]).  Every ring is rasterised as maskApi.c
    rleFrPoly does it; an instance without rings is the empty mask.
    fill='evenodd': all rings of an instance on one canvas, a pixel is set when an odd number of rings covers it: holes
      subtract.  The inverse of runs_to_polygons, bit for bit.
    fill='union': pycocotools' COCO.annToRLE: every ring on its own, then rleMerge: the instances of more than one ring are
      unioned with union_runs, one call per distinct canvas size among them; the rows of the others pass through untouched.
    cap: the first run capacity (ops.fit_runs grows it)."""
    if fill not in POLYGON_FILLS:
        raise ValueError(f'polygon fill {fill!r}: one of {POLYGON_FILLS}')
    cap = 64 if cap is None else max(int(cap), 2)
    if fill == 'evenodd':
        return ops.poly_raster(verts, ring_offs, ring_group, group_hw, cap)[:2]
    dev = verts.device
    R, G = int(ring_group.shape[0]), int(group_hw.shape[0])
    parts = torch.arange(R, dtype=torch.int32, device=dev)
    part_hw = group_hw[ring_group.to(torch.int64).clamp(0, max(G - 1, 0))].contiguous() if R else group_hw[:0]
    counts, n, _, _ = ops.poly_raster(verts, ring_offs, parts, part_hw, cap)
    hw = group_hw.cpu().numpy().astype(np.int64)
    inst_offs = np.searchsorted(ring_group.cpu().numpy(), np.arange(G + 1))               # the rings of instance g
    per = inst_offs[1:] - inst_offs[:-1]
    multi, single = np.flatnonzero(per > 1), np.flatnonzero(per == 1)
    tables = []                                                                           # (rows of the result, counts, n)
    for h, w in sorted({(int(a), int(b)) for a, b in hw[multi]}):
        rows = multi[(hw[multi, 0] == h) & (hw[multi, 1] == w)]
        members = np.concatenate([np.arange(inst_offs[g], inst_offs[g + 1]) for g in rows])
        offs = np.concatenate([[0], np.cumsum(per[rows])])
        c, m, _, _ = union_runs(counts, n, (h, w), torch.from_numpy(offs.astype(np.int32)).to(dev),
                                torch.from_numpy(members.astype(np.int32)).to(dev))
        tables.append((rows, c, m))
    # two columns at least: rsp_rle_to_string
    width = max([int(t[1].shape[1]) for t in tables] + [int(counts.shape[1]) if single.size else 2, 2])
    out = torch.zeros((G, width), dtype=torch.int32, device=dev)
    out[:, 0] = (group_hw[:, 0].to(torch.int64) * group_hw[:, 1]).to(torch.int32)          # no ring: one count h w
    n_out = torch.ones((G,), dtype=torch.int32, device=dev)
    if single.size:
        rows, src = torch.from_numpy(single).to(dev), torch.from_numpy(inst_offs[single]).to(dev)
        out[rows, :counts.shape[1]] = counts[src]
        n_out[rows] = n[src]
    for rows, c, m in tables:
        rows = torch.from_numpy(rows).to(dev)
        out[rows, :c.shape[1]] = c
        n_out[rows] = m
    return out, n_out


def runs_to_hulls(counts, n, size):
    """run table of k masks on one size = (H, W) canvas -> (hull_verts int32 [Vh, 2], hull_offs int64 [k + 1], hull_area2
    int64 [k]) on the device: the convex hull of every mask, all its components together (ops.mask_hull).
    Two device-to-host reads, whatever k is."""
    return ops.mask_hull(counts, n, size[0], size[1])


def runs_to_obb(counts, n, size):
    """run table -> (hull_verts, hull_offs, hull_area2, edge int32 [k], q int64 [k, 6]) on the device: the hulls and the
    minimum-area rectangle of each (ops.hull_min_rect: flush with hull edge `edge`, -1 for an empty mask; q = (ex, ey, amin,
    amax, bmin, bmax) in that edge's frame).  Exact integers; the two device-to-host reads of runs_to_hulls."""
    hull_verts, hull_offs, hull_area2 = runs_to_hulls(counts, n, size)
    edge, q = ops.hull_min_rect(hull_verts, hull_offs)
    return hull_verts, hull_offs, hull_area2, edge, q


def runs_to_obb_corners(counts, n, size, offsets=None):
    """run table of k masks on one size = (H, W) canvas -> float64 [k, 4, 2] ON THE DEVICE: the corners of every mask's
    minimum-area rectangle, the doubles of obb_to_numpy(form='corners') bit for bit, NaN rows for empty masks
    (ops.obb_corners).  offsets int32 [k, 2] = (ox, oy): each rectangle moved by its offset in integers first
    (a tile's rectangle at its place in the scene: the rectangle of the shifted table).  The two device-to-host reads of
    runs_to_hulls; the rectangles themselves stay on the device."""
    edge, q = runs_to_obb(counts, n, size)[3:]
    return ops.obb_corners(edge, q, offsets)


OBB_FORMS = ('corners', 'xywha')


def obb_to_numpy(edge, q, form='corners'):
    """what runs_to_obb returns -> float64 numpy on the host after ONE transfer (edge and q in one int64 buffer).
    form='corners': [k, 4, 2] = C0..C3 in pixel coordinates, clockwise on screen, C0 -> C1 on the hull edge: (amin, bmin),
      (amax, bmin), (amax, bmax), (amin, bmax) in the frame e = (ex, ey), nrm = (-ey, ex), divided by L = |e|^2.
    form='xywha': [k, 5] = centre x, y (the mean of the corners), w >= h (the sides U / sqrt L along e and V / sqrt L along
      nrm; w is e's on U == V) and the angle of the w side from +x towards +y in [-pi / 2, pi / 2), radians.
    Empty masks (edge = -1) give NaN rows."""
    if form not in OBB_FORMS:
        raise ValueError(f'oriented-box form {form!r}: one of {OBB_FORMS}')
    k = int(edge.shape[0])
    buf = torch.cat([edge.to(torch.int64).view(-1, 1), q.view(k, 6)], 1).cpu().numpy()
    live = buf[:, 0] >= 0
    ex, ey, amin, amax, bmin, bmax = (buf[:, i].astype(np.float64) for i in range(1, 7))
    L = np.where(live, ex * ex + ey * ey, 1.0)
    a = np.stack([amin, amax, amax, amin], 1)
    b = np.stack([bmin, bmin, bmax, bmax], 1)
    c = np.stack([a * ex[:, None] - b * ey[:, None], a * ey[:, None] + b * ex[:, None]], 2) / L[:, None, None]
    c[~live] = np.nan
    if form == 'corners':
        return c
    U, V = amax - amin, bmax - bmin
    along_e = U >= V
    root = np.sqrt(L)
    w, h = np.where(along_e, U, V) / root, np.where(along_e, V, U) / root
    ang = np.where(along_e, np.arctan2(ey, ex), np.arctan2(ex, -ey))
    ang = np.where(ang >= np.pi / 2, ang - np.pi, np.where(ang < -np.pi / 2, ang + np.pi, ang))
    out = np.stack([c[:, :, 0].mean(1), c[:, :, 1].mean(1), w, h, ang], 1)
    out[~live] = np.nan
    return out


def runs_components(counts, n, size):
    """run table of k masks on one size = (H, W) canvas -> ops.RunComponents on the device: the 8-connected components of
    every mask (comp_offs, piece_comp, comp_area, comp_box, comp_first, comp_inst, pieces, piece_offs, status; DESIGN §14.10,
    ops.rle_components).  Two device-to-host reads, whatever k is."""
    return ops.rle_components(counts, n, size[0], size[1])


def split_runs(counts, n, size, comps=None, cap=None):
    """run table -> (counts, n, n on the host, cap, comp_offs int64 [k + 1]): a run table with ONE ROW PER COMPONENT, C rows
    in component order (instance, then first pixel in stream order); rows comp_offs[i] .. comp_offs[i + 1] are the components
    of instance i.  A row holding one component comes back bit for bit.  comps: what runs_components returned for the table;
    cap: the first capacity (the input's plus two when None); the retry is ops.fit_runs'."""
    if comps is None:
        comps = runs_components(counts, n, size)
    if cap is None:
        cap = int(counts.shape[1]) + 2
    out = ops.fit_runs(lambda cap: ops.components_union(comps, size[0], size[1], cap), max(int(cap), 2))
    return out + (comps.comp_offs,)


def clean_runs(counts, n, size, min_area, mode='both', cap=None):
    """segment-anything's `remove_small_regions` in the run domain, with the semantics of ops.remove_small_regions (DESIGN §15
    "Small regions"): mode 'holes' (the 8-connected components of the complement with fewer than min_area pixels are set;
    the outer background is a component like any other), 'islands' (components of the mask that small are cleared; if all
    are, the largest stays, among equals the one with the lowest row-major first pixel) or 'both' (holes, then islands of the
    filled mask) -> (counts, n, n on the host, cap, changed int32 [k, 2] = a small hole / a small island existed).  A row
    with n <= 0 comes back as n = 0.  min_area = 0 returns the input table itself, without a launch.  Every pass labels the
    pieces (runs_components), selects components (ops.components_select) and writes the rows again through rsp_rle_union
    under ops.fit_runs; the complement of a row is the same counts with a leading zero added or removed."""
    if mode not in ops.MASK_REGION_MODES:
        raise ValueError(f'clean_runs: mode must be one of {sorted(ops.MASK_REGION_MODES)}, got {mode!r}')
    if isinstance(min_area, bool) or int(min_area) != min_area or not 0 <= int(min_area) < 2 ** 31:
        raise ValueError(f'clean_runs: min_area must be an integer in [0, 2^31), got {min_area!r}')
    k = int(n.shape[0])
    changed = torch.zeros((k, 2), dtype=torch.int32, device=n.device)
    if int(min_area) == 0 or k == 0:
        return counts, n, n.cpu(), int(counts.shape[1]), changed
    H, W = int(size[0]), int(size[1])
    live = n > 0
    cap = max(int(cap), 2) if cap is not None else int(counts.shape[1]) + 2
    bits = ops.MASK_REGION_MODES[mode]

    def filtered(c, m, keep_largest, slot, cap):
        comps = runs_components(c, m, (H, W))
        keep = ops.components_select(comps, int(min_area), keep_largest, slot, changed)
        return ops.fit_runs(lambda cap: ops.components_union(comps, H, W, cap, keep), cap)
    if bits & 1:                                   # the complement's small components go: what is left is the new background
        c, m, _, cap = filtered(*ops.rle_complement(counts, n), False, 0, cap)
        counts, n = ops.rle_complement(c, m)
    if bits & 2:
        counts, n, _, cap = filtered(counts, n, True, 1, cap)
    n = torch.where(live, n, torch.zeros_like(n))
    changed *= live[:, None].to(torch.int32)
    return counts, n, n.cpu(), int(counts.shape[1]), changed


MORPHOLOGY_ELEMENTS = ('square', 'disc', 'diamond')


def _exact_fraction(x, what):
    """a real number as the exact fractions.Fraction of what the caller wrote: an int, a Fraction, a Decimal, a string, or a
    float through its shortest repr (1.1 is 11/10, not the binary fraction next to it)"""
    import decimal
    import fractions
    if isinstance(x, bool) or x is None:
        raise ValueError(f'{what} must be a real number, got {x!r}')
    try:
        if isinstance(x, (int, fractions.Fraction, decimal.Decimal)):
            f = fractions.Fraction(x)
        elif isinstance(x, str):
            f = fractions.Fraction(x.strip())
        else:
            x = float(x)
            if not math.isfinite(x):
                raise ValueError
            f = fractions.Fraction(repr(x))
    except (ValueError, TypeError, ZeroDivisionError, OverflowError):
        raise ValueError(f'{what} must be a finite real number, got {x!r}') from None
    return f


def disc_r2(radius):
    """a real radius d >= 0 in pixels -> the squared radius floor(d^2) of the exact disc, in exact arithmetic (1.5 -> 2, 2.9 -> 8)"""
    f = _exact_fraction(radius, 'radius')
    if f < 0:
        raise ValueError(f'radius must be non-negative, got {radius!r}')
    return math.floor(f * f)


def half_heights(element, radius=None, r2=None, size=None):
    """the structuring element of the Euclidean buffers -> (hh, R): hh a list of R + 1 ints, hh[dx] = the rows
    the element reaches above and below its centre at column offset dx, non-increasing, hh[0] = R.  element='disc': the exact
    disc dx^2 + dy^2 <= r2, hh[dx] = isqrt(r2 - dx^2), R = isqrt(r2); give an integer r2 >= 0, or a real radius >= 0 for r2 =
    floor(radius^2) (disc_r2).  element='diamond': |dx| + |dy| <= radius, an integer, hh[dx] = radius - dx.  size = (H, W):
    r2 is cut at H^2 + W^2 (the diamond's radius at H + W), beyond which nothing changes on that canvas."""
    if element == 'disc':
        if (radius is None) == (r2 is None):
            raise ValueError("half_heights: 'disc' takes a radius or r2, one of them")
        if r2 is None:
            r2 = disc_r2(radius)
        elif isinstance(r2, bool) or not isinstance(r2, (int, np.integer)) or int(r2) < 0:
            raise ValueError(f'half_heights: r2 must be a non-negative integer, got {r2!r}')
        r2 = int(r2)
        if size is not None:
            r2 = min(r2, int(size[0]) ** 2 + int(size[1]) ** 2)
        R = math.isqrt(r2)
        return [math.isqrt(r2 - dx * dx) for dx in range(R + 1)], R
    if element == 'diamond':
        if r2 is not None or radius is None or isinstance(radius, bool) or int(radius) != radius or int(radius) < 0:
            raise ValueError(f"half_heights: 'diamond' takes a non-negative integer radius, got {radius!r}")
        R = int(radius) if size is None else min(int(radius), int(size[0]) + int(size[1]))
        return [R - dx for dx in range(R + 1)], R
    raise ValueError(f"half_heights: element must be 'disc' or 'diamond', got {element!r}")


def _element(element, radius, size):
    """element, radius of the *_runs below -> None for the square (the code of DESIGN §14.13), else the half-heights"""
    if element not in MORPHOLOGY_ELEMENTS:
        raise ValueError(f'element must be one of {MORPHOLOGY_ELEMENTS}, got {element!r}')
    return None if element == 'square' else half_heights(element, radius, size=size)[0]


def erode_runs(counts, n, size, radius, border=0, cap=None, element='square'):
    """run table of k masks on one size = (H, W) canvas -> (counts, n, n on the host, cap): every mask eroded by the
    (2 radius + 1)^2 square, the outside of the canvas counting as `border` (ops.rle_erode); element='disc'
    (radius a real number: the exact disc of floor(radius^2)) or 'diamond': ops.rle_erode_disc, DESIGN §14.16"""
    hh = _element(element, radius, size)
    if hh is not None:
        return ops.rle_erode_disc(counts, n, size[0], size[1], hh, border, cap)
    return ops.rle_erode(counts, n, size[0], size[1], radius, border, cap)


def dilate_runs(counts, n, size, radius, cap=None, element='square'):
    """every mask dilated by the square: the complement of the erosion of the complement with the outside set.  A row with
    n <= 0 stays the empty mask.  element='disc' | 'diamond': ops.rle_dilate_disc."""
    hh = _element(element, radius, size)
    if hh is not None:
        return ops.rle_dilate_disc(counts, n, size[0], size[1], hh, cap)
    live = n > 0
    c, m, _, cap = ops.rle_erode(*ops.rle_complement(counts, n), size[0], size[1], radius, 1, cap)
    c, m = ops.rle_complement(c, m)
    hw = int(size[0]) * int(size[1])
    c[:, 0] = torch.where(live, c[:, 0], torch.full_like(c[:, 0], hw))
    m = torch.where(live, m, torch.ones_like(m))
    return c, m, m.cpu(), int(c.shape[1])


def open_runs(counts, n, size, radius, cap=None, element='square'):
    """opening: dilation of the erosion (border 0); removes what the element does not fit into"""
    c, m, _, cap = erode_runs(counts, n, size, radius, 0, cap, element)
    return dilate_runs(c, m, size, radius, cap, element)


def close_runs(counts, n, size, radius, cap=None, element='square'):
    """closing: erosion (border 1) of the dilation; fills what the element does not fit into"""
    c, m, _, cap = dilate_runs(counts, n, size, radius, cap, element)
    return erode_runs(c, m, size, radius, 1, cap, element)


def boundary_runs(counts, n, size, radius, cap=None, element='square'):
    """the boundary band of every mask, M & ~erode(M, radius) (ops.rle_boundary): Boundary IoU's G_d & G; with
    element='disc' | 'diamond' the mask minus its erosion by that element (ops.rle_erode_disc, ops.rle_minus)"""
    if _element(element, radius, size) is not None:
        c, m, _, cap = erode_runs(counts, n, size, radius, 0, cap, element)
        return ops.rle_minus(counts, n, c, m, size[0], size[1], cap)
    return ops.rle_boundary(counts, n, size[0], size[1], radius, cap)


def buffer_runs(counts, n, size, distance, cap=None):
    """the GIS buffer of every mask by a signed real distance in pixels: > 0 the dilation by the exact disc
    of floor(distance^2), < 0 the erosion by the disc of |distance| with the outside of the canvas set (the edge of a scene is
    not an object boundary), 0 the canonical rows -> (counts, n, n on the host, cap)"""
    d = _exact_fraction(distance, 'distance')
    if d < 0:
        return erode_runs(counts, n, size, -d, 1, cap, 'disc')
    return dilate_runs(counts, n, size, d, cap, 'disc')


def boundary_radius(size, dilation_ratio=0.02):
    """Boundary IoU's band width for a size = (H, W) image: max(1, round(dilation_ratio * diagonal)), Python's round on a
    Python float, on the host (boundary-iou-api mask_to_boundary)"""
    r = float(dilation_ratio)
    if isinstance(dilation_ratio, bool) or not (r > 0 and math.isfinite(r)):
        raise ValueError(f'dilation_ratio must be a positive finite number, got {dilation_ratio!r}')
    H, W = int(size[0]), int(size[1])
    return max(1, int(round(r * math.sqrt(H * H + W * W))))


FLATTEN_ORDERS = ('score', 'area')


def _flatten_min_ratio(min_ratio):
    r = min_ratio
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not 0.0 <= float(r) <= 1.0:
        raise ValueError(f'min_ratio is a number in [0, 1], got {min_ratio!r}')
    return float(r)


def flatten_rank(k, order='score', scores=None, areas=None):
    """the priority of planar layers -> rank int32 numpy [k], a permutation of 0 .. k - 1 where 0 wins, on the
    host.  order='score': descending `scores`, ties to the lower index (the argmax of score x mask on torch CPU); NaN scores
    are refused.  order='area': ascending `areas`, small masks on top, ties to the lower index.  Anything else is taken as
    the rank itself and checked to be a permutation.  Tensors are brought to the host (a read where they are on the device)."""
    def host(v, name):
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if v.reshape(-1).shape[0] != k:
            raise ValueError(f'flatten: {name} has {v.reshape(-1).shape[0]} entries for {k} masks')
        return v.reshape(-1)
    if isinstance(order, str):
        if order not in FLATTEN_ORDERS:
            raise ValueError(f'flatten: order must be one of {FLATTEN_ORDERS} or a permutation, got {order!r}')
        if order == 'score':
            if scores is None:
                raise ValueError("flatten: order='score' needs scores")
            s = host(scores, 'scores').astype(np.float64)
            if np.isnan(s).any():
                raise ValueError('flatten: a score is NaN')
            first = np.argsort(-s, kind='stable')
        else:
            first = np.argsort(host(areas, 'areas').astype(np.int64), kind='stable')
        rank = np.empty(k, np.int32)
        rank[first] = np.arange(k, dtype=np.int32)
        return rank
    r = host(order, 'rank')
    if r.dtype.kind not in 'iu' or not np.array_equal(np.sort(r.astype(np.int64)), np.arange(k)):
        raise ValueError(f'flatten: rank must be a permutation of 0 .. {k - 1} (integers, 0 wins)')
    return r.astype(np.int32)


def flatten_runs(counts, n, size, rank, min_ratio=0.0, cap=None):
    """run table of k masks on one size = (H, W) canvas -> (counts, n, cap, area_before int32 [k], area_after int32 [k], kept
    bool [k]), all on the device: the rows made pairwise disjoint, F_i = M_i minus every M_j with rank[j] < rank[i]
    (ops.rle_flatten).  rank: a permutation of 0 .. k - 1, 0 wins -- a list, a numpy array or a tensor
    (flatten_rank checks it on the host: a device tensor costs a read); any counts that describe the canvas are legal input.
    min_ratio in [0, 1]: an instance with area(F_i) < min_ratio * area(M_i) is emptied AFTER the partition is made, so its
    pixels are not handed to the instances below it (the iou_thr branch of panoptic_postprocess); the comparison is made in
    float64 on the device (both areas are below 2^31, so only the product rounds).  kept[i] is False for such an instance
    and for one whose F_i is empty; area_after is the area of the row that is returned.  Reads: those of ops.rle_flatten."""
    k, dev = int(n.shape[0]), n.device
    ratio = _flatten_min_ratio(min_ratio)
    rank = torch.from_numpy(flatten_rank(k, rank)).to(dev)
    H, W = int(size[0]), int(size[1])
    out, n_out, cap = ops.rle_flatten(counts, n, H, W, rank, cap)
    before, after = ops.rle_bbox(counts, n, H, W)[1], ops.rle_bbox(out, n_out, H, W)[1]
    kept = (after > 0) & (after.to(torch.float64) >= ratio * before.to(torch.float64))
    if k:
        out[:, 0] = torch.where(kept, out[:, 0], torch.full_like(out[:, 0], H * W))
        n_out = torch.where(kept, n_out, torch.ones_like(n_out))
        after = torch.where(kept, after, torch.zeros_like(after))
    return out, n_out, cap, before, after, kept


def runs_to_labels(counts, n, size, ids=None):
    """run table of k pairwise DISJOINT masks (flatten_runs) on one size = (H, W) canvas -> int32 [H, W] on the device: ids[i]
    on the pixels of row i (i + 1 when None; a list, a numpy array or an int32 tensor), 0 for the background
    (ops.rle_label_map: one device-to-host read)."""
    k = int(n.shape[0])
    if ids is not None:
        ids = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.asarray(ids, np.int64).reshape(-1))
        if ids.dim() != 1 or ids.shape[0] != k or ids.dtype.is_floating_point:
            raise ValueError(f'runs_to_labels: ids holds one integer per mask ({k})')
        ids = ids.to(device=n.device, dtype=torch.int32)
    return ops.rle_label_map(counts, n, size[0], size[1], ids)


def runs_to_dicts(counts, n_host, size):
    """run table -> list of dict(size=[H, W], counts=list), the uncompressed form (HF `_mask_to_rle`).  n_host: the row
    lengths on the host (what fit_runs returned); one transfer, the table."""
    counts, n_host = counts.cpu().numpy(), n_host.tolist()
    return [dict(size=[int(size[0]), int(size[1])], counts=counts[i, :n_host[i]].tolist()) for i in range(len(n_host))]


# ---------------------------------------------------------------------------------------------------- mask forms
# A caller's masks are a bool [k, H, W] tensor ('dense'), RLE dicts with compressed counts (bytes / str: 'strings') or with
# uncompressed counts (list: 'lists').  Every conversion between these and the run table is here, in both directions.
def strings_to_runs(strings, device, cap=1024):
    """COCO's compressed counts (bytes as they are, str encoded) -> (counts, n) on `device` (ops.rle_from_string under
    ops.fit_runs: one device-to-host read per attempt)"""
    strings = [s if type(s) is bytes else s.encode() if isinstance(s, str) else bytes(s) for s in strings]
    offs = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, strings), dtype=np.int64, count=len(strings)), out=offs[1:])
    flat = np.frombuffer(b''.join(strings) or b'\0', dtype=np.uint8).copy()
    return ops.rle_from_string(torch.from_numpy(flat).to(device), torch.from_numpy(offs).to(device), cap)


def lists_to_runs(lists, device, what='lists_to_runs'):
    """uncompressed counts -> (counts zero-padded, n) on `device`; no device-to-host read"""
    table = np.zeros((len(lists), max([len(c) for c in lists] + [1])), np.int64)
    for i, c in enumerate(lists):
        table[i, :len(c)] = c
    if table.size and (int(table.max()) >= 2 ** 31 or int(table.min()) < 0):
        raise ValueError(f'{what}: not canonical COCO run counts: a count is negative or does not fit 32 bits')
    n = torch.tensor([len(c) for c in lists], dtype=torch.int32)
    return torch.from_numpy(table.astype(np.int32)).to(device), n.to(device)


def check_canonical(counts, n, size, what):
    """RLE dicts come from outside: the tracer reads canonical COCO counts only (a zero count anywhere but in front would
    make two runs of one value touch, counts that do not sum to H * W describe another canvas).  One device-to-host read."""
    k, cap = int(counts.shape[0]), int(counts.shape[1])
    if k == 0:
        return
    live = torch.arange(cap, device=counts.device)[None] < n[:, None]
    c = torch.where(live, counts, 0).to(torch.int64)
    bad = ((c[:, 1:] <= 0) & live[:, 1:]).any(1) | (c[:, :1] < 0).any(1) | ((c.sum(1) != size[0] * size[1]) & (n > 0))
    rows = bad.nonzero().view(-1).tolist()
    if rows:
        raise ValueError(f'{what}: the counts of mask {rows[0]} are not canonical COCO run counts of a '
                         f'{size[0]} x {size[1]} canvas (a zero or negative count after the first, or a sum other than H * W)'
                         + (f'; {len(rows)} masks in all' if len(rows) > 1 else ''))


def masks_to_runs(masks, device, what, *, one_size=True, canonical=False, cap=None):
    """A caller's masks -> (counts, n, size, form) on the device: a bool [k, H, W] tensor (form 'dense', on its own device;
    encode_runs) or a list of RLE dicts dict(size=[H, W], counts=...) ('strings' / 'lists'; `device` places the table).
    `what` names the public function that was called and heads every refusal.
    one_size=True: the dicts share one size = (H, W) and one counts form; an empty list carries no size and is refused.
    one_size=False: size is the list of every row's own (H, W); compressed and uncompressed counts may stand side by side
      ('mixed'): one table, the rows in list order (the run-domain IoU takes no canvas size); an empty list is an empty table.
    canonical=True: check_canonical on what came as dicts (one more read).  cap: the first run capacity of the producer."""
    if isinstance(masks, torch.Tensor):
        if masks.dim() != 3:
            raise ValueError(f'{what}: a mask tensor is bool [k, H, W]')
        counts, n, _, _ = encode_runs(masks.to(torch.bool), cap or 4096)
        size = (int(masks.shape[1]), int(masks.shape[2]))
        return counts, n, size if one_size else [size] * int(n.shape[0]), 'dense'
    masks = list(masks)
    sizes = [(int(m['size'][0]), int(m['size'][1])) for m in masks]
    packed = [isinstance(m['counts'], (bytes, str)) for m in masks]
    if one_size:
        if not masks:
            raise ValueError(f'{what}: an empty list carries no canvas size; pass a bool [0, H, W] tensor instead')
        if len(set(sizes)) != 1:
            raise ValueError(f'{what}: the RLE dicts of one call share one size, got {sorted(set(sizes))}')
        if len(set(packed)) != 1:
            raise ValueError(f'{what}: compressed (bytes / str) and uncompressed (list) counts in one call')
    dev = torch.device(device)
    ops.require_device(dev)
    if not masks:
        return torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev), [], 'lists'
    form = 'mixed' if len(set(packed)) > 1 else 'strings' if packed[0] else 'lists'
    order, tables, ns = [], [], []
    for is_packed in (True, False):                                     # a table per counts form: the compressed rows first
        idx = [i for i, p in enumerate(packed) if p == is_packed]
        if idx:
            rows = [masks[i]['counts'] for i in idx]
            c, n = strings_to_runs(rows, dev, cap or 1024) if is_packed else lists_to_runs(rows, dev, what)
            order, tables, ns = order + idx, tables + [c], ns + [n]
    if one_size:                                                        # one counts form: its table as it is
        if canonical:
            check_canonical(tables[0], ns[0], sizes[0], what)
        return tables[0], ns[0], sizes[0], form
    back = torch.tensor(np.argsort(np.asarray(order, np.int64), kind='stable'), dtype=torch.int64, device=dev)
    return concat_runs(tables, rows=back).contiguous(), torch.cat(ns)[back].contiguous(), sizes, form


def word_offsets(sizes):
    """(H, W) per mask -> int64 [k + 1] on the host: mask i holds words word_offsets[i] .. [i + 1] of the bit planes, one
    bit per pixel in 64-bit words, every mask from a word of its own"""
    offs = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(((int(h) * int(w) + 63) // 64 for h, w in sizes), dtype=np.int64, count=len(sizes)), out=offs[1:])
    return offs


def runs_to_bits(counts, n, sizes):
    """run table, (H, W) per row -> (bits int64, word_offs int64 [k + 1], area int64 [k], wrange int32 [k, 2]) on the device:
    the bit planes rsp_coco_iou reads (ops.rle_to_bits; one device-to-host read, the number of words)"""
    word_offs = torch.from_numpy(word_offsets(sizes)).to(n.device)
    bits, area, wrange = ops.rle_to_bits(counts, n, word_offs)
    return bits, word_offs, area, wrange


def runs_to_dense(counts, n, size):
    """run table of k masks on one size = (H, W) canvas -> bool [k, H, W] on the device, through the bit planes of
    ops.rle_to_bits (one size: the word offsets are made on the device)"""
    (H, W), k, dev = size, int(n.shape[0]), n.device
    nw = int(word_offsets([size])[1])
    bits = ops.rle_to_bits(counts.contiguous(), n, torch.arange(k + 1, dtype=torch.int64, device=dev) * nw)[0]
    # pixel j of the column-major stream is bit j & 7 of byte j >> 3 (little-endian words): one byte per pixel,
    # then [W, H] -> [H, W]
    px = (bits[:k * nw].view(torch.uint8).view(k, nw * 8, 1) >> torch.arange(8, dtype=torch.uint8, device=dev)) & 1
    return px.view(k, nw * 64)[:, :H * W].reshape(k, W, H).transpose(1, 2).to(torch.bool).contiguous()


def runs_to_masks(counts, n, size, form, n_host=None):
    """run table -> the masks in the form they came in (masks_to_runs' `form`): 'dense' a bool [k, H, W] tensor, 'strings'
    runs_to_strings (bytes, also for str input), 'lists' runs_to_dicts (n_host: the row lengths, where the host has them)"""
    if form == 'dense':
        return runs_to_dense(counts, n, size)
    if form == 'strings':
        return runs_to_strings(counts.contiguous(), n, size)
    if form == 'lists':
        return runs_to_dicts(counts, n.cpu() if n_host is None else n_host, size)
    raise ValueError(f"mask form {form!r}: one of 'dense', 'strings', 'lists'")


def encode_rle_strings(masks, cap=4096, flat_cap=None):
    """bool [k, H, W] on the device -> (flat uint8 tensor, offsets int64 [k + 1]) on the HOST: string i is
    flat[offs[i]:offs[i + 1]].  Two device kernels and three transfers (n, offs, flat); grows its capacities and retries
    when a mask has more runs / the strings more bytes than assumed."""
    k = int(masks.shape[0])
    counts, n, _, cap = encode_runs(masks, cap)
    if k == 0:
        return torch.zeros((0,), dtype=torch.uint8), torch.zeros((1,), dtype=torch.int64)
    return _string_bytes(counts, n, flat_cap or 2 * cap * k)


def encode_mask_results(masks):
    """masks: bool tensor [k, H, W] on the HIP device -> list of k RLE dicts (same as the reference's function)."""
    k, h, w = masks.shape
    counts, n, _, cap = encode_runs(masks)
    return runs_to_strings(counts, n, (h, w), 2 * cap * k)


def encode_mask_dicts(masks):
    """encode_mask_results in the uncompressed form: bool [k, H, W] on the device -> list of k dict(size, counts=list)."""
    counts, _, n_host, _ = encode_runs(masks)
    return runs_to_dicts(counts, n_host, masks.shape[1:])
