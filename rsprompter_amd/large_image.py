"""Sliced inference on large scenes: the reference's `demo/large_image_demo.py` +
`mmdet/utils/large_image.py` (`shift_predictions`, `merge_results_by_nms`) over `sahi.slicing`
(`get_slice_bboxes`, `slice_image`, `shift_bboxes`, `shift_masks`) and `mmcv.ops.batched_nms`.

The reference cuts the scene into overlapping patches on the host, runs the detector patch by patch, pads every instance
mask to the full scene as a dense array and merges with a class-aware NMS.  Here the decoded scene is uploaded once;
tiles are cut by a kernel straight into the model's input batch (`rsp_slice_resize_pad`); a batch's tile masks are
reduced to run counts as soon as it is done (`rsp_mask_rle`); the merge is `rsp_batched_nms`; and the scene-sized COCO
RLE of the kept instances is produced in the run domain from the tile-sized runs (`rsp_rle_shift` ->
`rsp_rle_to_string`), so a scene-sized dense mask exists only when the caller asks for one.  merge_nms_type='seam_mask'
first joins the fragments of objects cut by tile seams by their mask IoU inside the tiles' common rectangle, also in the run
domain (`rsp_rle_bbox`, `rsp_rle_pair_overlap`, `rsp_rle_union`: DESIGN §14.6).

CLI: `python -m rsprompter_amd.large_image IMG_OR_DIR CONFIG CHECKPOINT --out-dir DIR` writes one `<name>.json` per scene.
"""
import json
import os

import numpy as np
import torch

from . import _lib, ops, rle
from .structures import DetDataSample, InstanceData

# masks='dense' materialises bool [K, H, W]; a request beyond this many bytes is refused with the figure in the message
# (settable, like ops.NMS_WORKSPACE_LIMIT_BYTES)
DENSE_MASK_LIMIT_BYTES = 8 << 30
MAX_PATCH_WIDTH = _lib.CONST['RSP_RLE_MAX_WIDTH']          # rsp_mask_rle is specified for widths up to here


# ----------------------------------------------------------------------------------------------------------------- host
def slice_bboxes(height, width, slice_height, slice_width, overlap_height_ratio=0.2, overlap_width_ratio=0.2):
    """sahi.slicing.get_slice_bboxes(auto_slice_resolution=False): [xmin, ymin, xmax, ymax] per tile, row-major.  A tile
    that would cross the right / bottom edge is moved back inside, so all tiles have the size
    (min(slice_height, height), min(slice_width, width))."""
    slice_bboxes_ = []
    y_max = y_min = 0
    y_overlap = int(overlap_height_ratio * slice_height)
    x_overlap = int(overlap_width_ratio * slice_width)
    if slice_height <= y_overlap or slice_width <= x_overlap or slice_height <= 0 or slice_width <= 0:
        raise ValueError('the overlap must be smaller than the slice')
    while y_max < height:
        x_min = x_max = 0
        y_max = y_min + slice_height
        while x_max < width:
            x_max = x_min + slice_width
            if y_max > height or x_max > width:
                xmax = min(width, x_max)
                ymax = min(height, y_max)
                xmin = max(0, xmax - slice_width)
                ymin = max(0, ymax - slice_height)
                slice_bboxes_.append([xmin, ymin, xmax, ymax])
            else:
                slice_bboxes_.append([x_min, y_min, x_max, y_max])
            x_min = x_max - x_overlap
        y_min = y_max - y_overlap
    return slice_bboxes_


def shift_bboxes(bboxes, offset):
    """sahi.slicing.shift_bboxes: boxes [n, 4] + (ox, oy, ox, oy) in the boxes' dtype (fp32)."""
    if bboxes.shape[-1] != 4:
        raise NotImplementedError(f'boxes with {bboxes.shape[-1]} columns (rotated boxes) are not supported')
    return bboxes + bboxes.new_tensor([offset[0], offset[1], offset[0], offset[1]])


def _offsets_tensor(offsets, counts, dev):
    """per-instance (ox, oy) int32 [sum(counts), 2] on the device from per-tile offsets and per-tile instance counts"""
    off = torch.tensor([[int(o[0]), int(o[1])] for o in offsets], dtype=torch.int32).reshape(-1, 2)
    rep = torch.repeat_interleave(off, torch.tensor(list(counts), dtype=torch.int64), dim=0)
    return rep.to(dev)


def shift_predictions(det_data_samples, offsets, src_image_shape):
    """mmdet/utils/large_image.py:27-72: the patch results moved into the scene and concatenated (tile order, then the
    tile's own order) -> InstanceData(bboxes, scores, labels[, masks bool [n, H, W] dense, as the reference])."""
    assert len(det_data_samples) == len(offsets), 'The `results` should has the same length with `offsets`.'
    insts = [s.pred_instances for s in det_data_samples]
    for p in insts:
        if p.bboxes.shape[-1] != 4:
            raise NotImplementedError(f'boxes with {p.bboxes.shape[-1]} columns (rotated boxes) are not supported')
    out = InstanceData()
    out.bboxes = torch.cat([shift_bboxes(p.bboxes, o) for p, o in zip(insts, offsets)], 0)
    out.scores = torch.cat([p.scores for p in insts], 0)
    out.labels = torch.cat([p.labels for p in insts], 0)
    if all('masks' in p and p.masks is not None for p in insts) and insts:
        shapes = {tuple(p.masks.shape[1:]) for p in insts}
        if len(shapes) != 1:
            raise ValueError(f'the patches must have one size, got masks of {sorted(shapes)}')
        masks = torch.cat([p.masks for p in insts], 0)
        off = _offsets_tensor(offsets, [len(p.scores) for p in insts], masks.device)
        H, W = int(src_image_shape[0]), int(src_image_shape[1])
        _check_dense(masks.shape[0], H, W)
        out.masks = ops.paste_tiles(masks.to(torch.bool), off, (H, W))
    return out


def _check_nms_cfg(nms_cfg):
    """-> (type, box IoU threshold, seam IoU threshold)"""
    cfg = dict(nms_cfg)
    typ = cfg.pop('type', 'nms')
    if typ not in ('nms', 'seam_mask', 'nms_rotated'):
        raise NotImplementedError(f"merge nms type {typ!r}: only 'nms' (mmcv.ops.nms through batched_nms), 'seam_mask' and "
                                  "'nms_rotated' are implemented")
    if cfg.get('class_agnostic', False):
        raise NotImplementedError('class_agnostic merging is not implemented')
    return typ, float(cfg.get('iou_threshold', cfg.get('iou_thr', 0.5))), float(cfg.get('seam_iou_threshold', 0.5))


def merge_results_by_nms(results, offsets, src_image_shape, nms_cfg):
    """mmdet/utils/large_image.py:75-104: shift, then mmcv.ops.batched_nms over all instances of the scene; returns a
    DetDataSample with the metainfo of results[0] and the kept instances in batched_nms' order (descending score).
    nms_cfg = dict(type='seam_mask', iou_threshold=..., seam_iou_threshold=...): fragments of one object are first joined
    by their mask IoU at the tile seams (the tile size is the masks' shape, as in shift_predictions); the
    sample then also carries `keep` and `members` like inference_large_image's.
    nms_cfg = dict(type='nms_rotated', iou_threshold=...): mmcv.ops.nms_rotated in place of the box NMS, on the minimum-area
    rectangles of the patch masks moved to their place in the scene; every patch result needs masks, the
    boxes stay axis-aligned."""
    typ, thr, seam_thr = _check_nms_cfg(nms_cfg)
    if typ == 'seam_mask':
        return _merge_results_by_seam_mask(results, offsets, src_image_shape, thr, seam_thr)
    if typ == 'nms_rotated':
        insts = [s.pred_instances for s in results]
        if not insts or not all('masks' in p and p.masks is not None for p in insts):
            raise ValueError("merge type 'nms_rotated' compares the masks' rectangles: every patch result needs "
                             'pred_instances.masks')
    inst = shift_predictions(results, offsets, src_image_shape)
    if typ == 'nms_rotated':
        tile = torch.cat([p.masks for p in insts], 0).to(torch.bool)
        off = _offsets_tensor(offsets, [len(p.scores) for p in insts], tile.device)
        counts, n, _, _ = rle.encode_runs(tile)
        keep = _rotated_keep(counts, n, tuple(tile.shape[1:]), off, inst.scores, inst.labels, thr)
    else:
        keep = ops.nms_flat(inst.bboxes, inst.scores, inst.labels, thr)
    merged = DetDataSample(metainfo=results[0].metainfo)
    merged.pred_instances = inst[keep]
    return merged


def _rotated_keep(counts, n, tile_hw, offsets, scores, labels, thr):
    """merge type 'nms_rotated' (DESIGN §14.17): the minimum-area rectangle of every tile instance from the tile run table,
    moved by its tile origin in integers (offsets int32 [k, 2] = (ox, oy)), then ONE rotated NMS over the scene -> keep int64,
    indices in kept order like ops.nms_flat's.  An instance with an empty mask has no rectangle: it suppresses nothing and
    is kept."""
    if int(n.shape[0]) == 0:
        return torch.zeros((0,), dtype=torch.int64, device=n.device)
    quad = rle.runs_to_obb_corners(counts, n, tile_hw, offsets.to(torch.int32).contiguous())
    return ops.obb_nms(quad, scores.to(torch.float32), labels.to(torch.int32), thr)


def _check_dense(k, H, W):
    need = int(k) * int(H) * int(W)
    if need > DENSE_MASK_LIMIT_BYTES:
        raise ValueError(f'dense masks of {k} instances on a {H} x {W} scene need {need} bytes (limit '
                         f'large_image.DENSE_MASK_LIMIT_BYTES = {DENSE_MASK_LIMIT_BYTES}): use masks="rle"')


# ------------------------------------------------------------------------------------------------------------- pipeline
def _runs_out(counts, n, scene_hw, polygons, obb_out=None):
    """the scene run table in the form the caller asked for: COCO strings (rsp_rle_to_string), or with polygons (True, or
    (tolerance, min_ring_area) to simplify them on the device, DESIGN §14.8, or (tolerance, 0, 'shared') to simplify the
    shared borders of a flattened table once) the per-instance ring lists of DESIGN §14.7
    (csrc/mask_polygons.hip), traced on the table before any string is made.  obb_out: a list that receives the oriented
    boxes of the table, float64 [k, 4, 2] (csrc/mask_obb.hip), made from the same table first"""
    if obb_out is not None:
        obb_out.append(rle.obb_to_numpy(*rle.runs_to_obb(counts, n, scene_hw)[3:], form='corners'))
    if polygons is not True and polygons and len(polygons) == 3:        # (tolerance, 0, 'shared'): DESIGN §14.15
        return rle.polygons_to_lists(*rle.simplify_coverage(counts, n, scene_hw, polygons[0])[0])
    if polygons:
        polys = rle.runs_to_polygons(counts, n, scene_hw)
        if polygons is not True:
            polys, _ = rle.simplify_polygons(polys, scene_hw, polygons[0], polygons[1])
        return rle.polygons_to_lists(*polys)
    return rle.runs_to_strings(counts, n, scene_hw)


def _clean_scene(counts, n, scene_hw, region):
    """region = (min_mask_region_area, a list that receives changed bool [K]) or None: the scene run table with holes and
    islands of fewer pixels than that removed (rle.clean_runs, mode 'both': DESIGN §14.10), before it takes any output form"""
    if region is None:
        return counts, n
    counts, n, _, _, changed = rle.clean_runs(counts, n, scene_hw, region[0], 'both')
    region[1].append((changed != 0).any(1))
    return counts, n


def _check_flatten(flatten, min_ratio):
    """flatten=False | 'score' | 'area' and flatten_min_ratio of inference_large_image -> (order or None, min_ratio)"""
    if flatten is not False and flatten is not None and flatten not in rle.FLATTEN_ORDERS:
        raise ValueError(f"flatten must be False, 'score' or 'area', got {flatten!r}")
    ratio = rle._flatten_min_ratio(min_ratio)
    if not flatten and ratio != 0.0:
        raise ValueError("flatten_min_ratio applies with flatten='score' or flatten='area'")
    return (flatten or None), ratio


def _check_buffer(buffer):
    """buffer of inference_large_image: a signed finite real number of pixels -> it, or None for 0"""
    try:
        d = rle._exact_fraction(buffer, 'buffer')
    except ValueError:
        raise ValueError(f'buffer must be a finite real number of pixels (signed), got {buffer!r}') from None
    return buffer if d != 0 else None


def _finish_scene(counts, n, scene_hw, region, planar, buf=None):
    """the scene run table before it takes any output form.  buf = (distance, a list that receives area int32 [K, 2]) or
    None: every mask buffered by the signed distance first (rle.buffer_runs) -- growth may create overlaps,
    which the flatten below resolves, so a planar layer stays planar.  planar = (order, min_ratio, scores float [K], a list that receives
    (kept bool [K], area int32 [K, 2])) or None: the instances made pairwise disjoint first (rle.flatten_runs),
    so that the slivers a subtraction leaves are cleaned with everything else (_clean_scene).  Cleaning fills small holes, and
    a hole of one instance may be where a better one lives: where both are asked for the cleaned table is flattened once
    more, by the same rank, so the result is disjoint whatever was filled."""
    if buf is not None:
        area0 = ops.rle_bbox(counts, n, scene_hw[0], scene_hw[1])[1]
        counts, n, _, _ = rle.buffer_runs(counts, n, scene_hw, buf[0])
        buf[1].append(torch.stack([area0, ops.rle_bbox(counts, n, scene_hw[0], scene_hw[1])[1]], 1))
    if planar is None:
        return _clean_scene(counts, n, scene_hw, region)
    order, ratio, scores, out = planar
    areas = ops.rle_bbox(counts, n, scene_hw[0], scene_hw[1])[1] if order == 'area' else None
    rank = rle.flatten_rank(int(n.shape[0]), order, scores, areas)
    counts, n, _, before, after, kept = rle.flatten_runs(counts, n, scene_hw, rank, ratio)
    if region is not None:
        counts, n = _clean_scene(counts, n, scene_hw, region)
        counts, n, _, _, after, again = rle.flatten_runs(counts, n, scene_hw, rank)
        kept = kept & again
    out.append((kept, torch.stack([before, after], 1)))
    return counts, n


def _scene_rle(counts, n, offsets, tile_hw, scene_hw, polygons=False, obb_out=None, region=None, planar=None, buf=None):
    """tile run counts of the kept instances -> list of dict(size=[H, W], counts=bytes) (rsp_rle_shift, rsp_rle_to_string)"""
    if int(n.shape[0]) == 0:
        if obb_out is not None:
            obb_out.append(np.zeros((0, 4, 2), np.float64))
        return []
    sc, sn, _, _ = rle.shift_runs(counts, n, offsets, tile_hw, scene_hw)
    sc, sn = _finish_scene(sc, sn, scene_hw, region, planar, buf)
    return _runs_out(sc, sn, scene_hw, polygons, obb_out)


# ------------------------------------------------------------------------------------------------------- seam merge
SEAM_PAIR_CHUNK_ELEMS = 1 << 24     # box tests materialised at once while pairing the instances of overlapping tiles


def _seam_pairs(tile_rects, cand_tile, tight, labels, dev):
    """candidate pairs of the seam merge.  tile_rects: host [T, 4]; cand_tile: host int [nc] (ascending) = the tile of each
    candidate; tight int32 [nc, 4] / labels [nc] on the device.  Per pair of tiles whose rectangles overlap, the pairs of
    their candidates with one label and intersecting TIGHT boxes (exact: disjoint tight boxes imply an empty intersection)
    -> (pairs int32 [P, 2] candidate rows, first < second; rects int32 [P, 4] = the tiles' common rectangle)."""
    empty = (torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros((0, 4), dtype=torch.int32, device=dev))
    T, nc = len(tile_rects), len(cand_tile)
    if nc == 0 or T < 2:
        return empty
    r = np.asarray(tile_rects, np.int64).reshape(T, 4)
    first = np.searchsorted(cand_tile, np.arange(T), 'left')
    cnt = np.searchsorted(cand_tile, np.arange(T), 'right') - first
    live = np.flatnonzero(cnt > 0)
    ix0, iy0 = np.maximum(r[live, None, 0], r[None, live, 0]), np.maximum(r[live, None, 1], r[None, live, 1])
    ix1, iy1 = np.minimum(r[live, None, 2], r[None, live, 2]), np.minimum(r[live, None, 3], r[None, live, 3])
    a, b = np.nonzero(np.triu((ix1 > ix0) & (iy1 > iy0), 1))
    if a.size == 0:
        return empty
    tp_rect = torch.from_numpy(np.stack([ix0[a, b], iy0[a, b], ix1[a, b], iy1[a, b]], 1).astype(np.int32)).to(dev)
    kmax = int(cnt.max())
    table = np.full((T, kmax), -1, np.int64)
    for t in live.tolist():
        table[t, :cnt[t]] = np.arange(first[t], first[t] + cnt[t])
    table = torch.from_numpy(table).to(dev)
    ta, tb = torch.from_numpy(live[a]).to(dev), torch.from_numpy(live[b]).to(dev)
    lab = labels.to(torch.int64)
    pairs, rects = [], []
    step = max(1, SEAM_PAIR_CHUNK_ELEMS // (kmax * kmax))
    for c0 in range(0, int(ta.shape[0]), step):
        ia, ib = table[ta[c0:c0 + step]], table[tb[c0:c0 + step]]                       # [C, kmax]
        A, B = tight[ia.clamp(min=0)][:, :, None, :], tight[ib.clamp(min=0)][:, None, :, :]
        hit = (ia >= 0)[:, :, None] & (ib >= 0)[:, None, :] & (lab[ia.clamp(min=0)][:, :, None] == lab[ib.clamp(min=0)][:, None, :])
        hit &= (A[..., 0] < B[..., 2]) & (B[..., 0] < A[..., 2]) & (A[..., 1] < B[..., 3]) & (B[..., 1] < A[..., 3])
        c, p, q = hit.nonzero(as_tuple=True)
        pairs.append(torch.stack([ia[c, p], ib[c, q]], 1).to(torch.int32))
        rects.append(tp_rect[c0:c0 + step][c])
    return torch.cat(pairs, 0).contiguous(), torch.cat(rects, 0).contiguous()


def _seam_components(n, edges, scores):
    """connected components of the edge graph on the host (union-find; the edge list is small) -> list of (representative,
    members ascending), ascending by representative: the member with the highest score, the lowest index among equals"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for i, j in edges:
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    groups = {}
    for i in range(n):
        groups.setdefault(find(i), []).append(i)
    out = []
    for mem in groups.values():
        rep = mem[0]
        for i in mem[1:]:
            if scores[i] > scores[rep]:
                rep = i
        out.append((rep, mem))
    out.sort(key=lambda g: g[0])
    return out


def _seam_merge(boxes, scores, labels, tile_of, tile_rects, counts, n, tile_hw, scene_hw, seam_iou_thr, merge_iou_thr):
    """The 'seam_mask' merge over the tile-ordered concatenation: boxes fp32 [N, 4] in the scene, scores,
    labels, tile_of int64 [N] (ascending), tile_rects host [T, 4], counts / n = the TILE run counts of all N instances.
    Returns (InstanceData(bboxes, scores, labels) of the merged instances in nms_flat's keep order, keep = their
    representatives, members = list of index lists, (member rows int64 [M], group offsets int32 [K + 1]) on the device)."""
    dev = boxes.device
    N = int(scores.shape[0])
    H, W = scene_hw
    th, tw = tile_hw
    rect_d = torch.tensor(np.asarray(tile_rects, np.int64).reshape(-1, 4), dtype=torch.int32, device=dev)
    origin = rect_d[tile_of][:, :2] if N else torch.zeros((0, 2), dtype=torch.int32, device=dev)
    edges = []
    if N:
        # tight boxes of the tile runs, moved into the scene: an instance whose mask stays outside every other tile's
        # rectangle cannot share a pixel with another tile's instance and stays a singleton without being shifted
        tb, area = ops.rle_bbox(counts, n, th, tw)
        tb = tb + torch.cat([origin, origin], 1)
        reach = (tb[:, None, 0] < rect_d[None, :, 2]) & (rect_d[None, :, 0] < tb[:, None, 2]) \
            & (tb[:, None, 1] < rect_d[None, :, 3]) & (rect_d[None, :, 1] < tb[:, None, 3])
        reach[torch.arange(N, device=dev), tile_of] = False
        cand = ((area > 0) & reach.any(1)).nonzero().view(-1)
        cand_h = cand.cpu().numpy()
        if cand_h.size:
            sc, sn, _, _ = rle.shift_runs(counts[cand], n[cand].contiguous(), origin[cand].contiguous(), tile_hw, scene_hw)
            tight, _ = ops.rle_bbox(sc, sn, H, W)
            pairs, rects = _seam_pairs(tile_rects, tile_of.cpu().numpy()[cand_h], tight, labels[cand], dev)
            if pairs.shape[0]:
                ov = ops.rle_pair_overlap(sc, sn, H, W, pairs, rects).to(torch.int64)
                inter, union = ov[:, 0], ov[:, 1] + ov[:, 2] - ov[:, 0]
                is_edge = (inter > 0) & (inter.double() >= float(seam_iou_thr) * union.double())
                e = pairs[is_edge].cpu().numpy()
                edges = np.stack([cand_h[e[:, 0]], cand_h[e[:, 1]]], 1).tolist() if e.size else []
            del sc, sn
    comps = _seam_components(N, edges, scores.cpu().tolist())
    K = len(comps)
    reps = torch.tensor([c[0] for c in comps], dtype=torch.int64, device=dev)
    gid_h = np.zeros((N,), np.int64)
    for g, (_, mem) in enumerate(comps):
        gid_h[mem] = g
    gid = torch.from_numpy(gid_h).to(dev)
    g2 = gid[:, None].expand(-1, 2)
    mb = torch.empty((K, 4), dtype=boxes.dtype, device=dev)
    if K:
        mb[:, :2] = torch.zeros((K, 2), dtype=boxes.dtype, device=dev).scatter_reduce(0, g2, boxes[:, :2], 'amin', include_self=False)
        mb[:, 2:] = torch.zeros((K, 2), dtype=boxes.dtype, device=dev).scatter_reduce(0, g2, boxes[:, 2:], 'amax', include_self=False)
    ms, ml = scores[reps], labels[reps]
    keep_m = ops.nms_flat(mb, ms, ml, merge_iou_thr)
    out = InstanceData(bboxes=mb[keep_m], scores=ms[keep_m], labels=ml[keep_m])
    members = [comps[g][1] for g in keep_m.tolist()]
    flat = torch.tensor([i for mem in members for i in mem], dtype=torch.int64, device=dev)
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(mem) for mem in members])]).astype(np.int32), device=dev)
    return out, reps[keep_m], members, (flat, offs)


def _seam_rle(counts, n, origin, groups, tile_hw, scene_hw, polygons=False, obb_out=None, region=None, planar=None,
              buf=None):
    """the merged instances' scene RLE: the members' tile runs shifted into the scene (rsp_rle_shift), joined per group
    (rsp_rle_union) and written as strings (rsp_rle_to_string)"""
    flat, offs = groups
    K = int(offs.shape[0]) - 1
    if K == 0:
        if obb_out is not None:
            obb_out.append(np.zeros((0, 4, 2), np.float64))
        return []
    sc, sn, _, _ = rle.shift_runs(counts[flat], n[flat].contiguous(), origin[flat].contiguous(), tile_hw, scene_hw)
    members = torch.arange(flat.shape[0], dtype=torch.int32, device=flat.device)
    uc, un, _, _ = rle.union_runs(sc, sn, scene_hw, offs, members)
    uc, un = _finish_scene(uc, un, scene_hw, region, planar, buf)
    return _runs_out(uc, un, scene_hw, polygons, obb_out)


def _seam_dense(tile_masks, origin, groups, scene_hw):
    """the merged instances' dense masks: the members pasted (rsp_paste_tiles) and OR-reduced per group"""
    flat, offs = groups
    K, M = int(offs.shape[0]) - 1, int(flat.shape[0])
    H, W = scene_hw
    _check_dense(M, H, W)
    out = torch.zeros((K, H, W), dtype=torch.uint8, device=flat.device)
    if M:
        o64 = offs.to(torch.int64)
        gid = torch.repeat_interleave(torch.arange(K, device=flat.device), o64[1:] - o64[:-1], output_size=M)
        pasted = ops.paste_tiles(tile_masks[flat].to(torch.bool), origin[flat].contiguous(), (H, W))
        out.index_add_(0, gid, pasted.to(torch.uint8))                 # a group is a handful of fragments: no overflow
    return out > 0


def _merge_results_by_seam_mask(results, offsets, src_image_shape, thr, seam_thr):
    insts = [s.pred_instances for s in results]
    assert len(results) == len(offsets), 'The `results` should has the same length with `offsets`.'
    if not insts or not all('masks' in p and p.masks is not None for p in insts):
        raise ValueError("merge type 'seam_mask' compares masks: every patch result needs pred_instances.masks")
    for p in insts:
        if p.bboxes.shape[-1] != 4:
            raise NotImplementedError(f'boxes with {p.bboxes.shape[-1]} columns (rotated boxes) are not supported')
    shapes = {tuple(p.masks.shape[1:]) for p in insts}
    if len(shapes) != 1:
        raise ValueError(f'the patches must have one size, got masks of {sorted(shapes)}')
    th, tw = shapes.pop()
    H, W = int(src_image_shape[0]), int(src_image_shape[1])
    if H * W >= 2 ** 31:
        raise ValueError(f'a {H} x {W} scene has {H * W} pixels; COCO run counts are 32-bit (< 2^31 pixels)')
    masks = torch.cat([p.masks for p in insts], 0).to(torch.bool)
    dev = masks.device
    boxes = torch.cat([shift_bboxes(p.bboxes, o) for p, o in zip(insts, offsets)], 0)
    scores, labels = torch.cat([p.scores for p in insts], 0), torch.cat([p.labels for p in insts], 0)
    tile_of = torch.repeat_interleave(torch.arange(len(insts)), torch.tensor([len(p.scores) for p in insts])).to(dev)
    rects = [[int(o[0]), int(o[1]), int(o[0]) + tw, int(o[1]) + th] for o in offsets]
    counts, n, _, _ = rle.encode_runs(masks)
    out, keep, members, groups = _seam_merge(boxes, scores, labels, tile_of, rects, counts, n, (th, tw), (H, W), seam_thr, thr)
    origin = torch.tensor(rects, dtype=torch.int32, device=dev).reshape(-1, 4)[tile_of][:, :2]
    out.masks = _seam_dense(masks, origin, groups, (H, W))
    merged = DetDataSample(metainfo=results[0].metainfo)
    merged.pred_instances = out
    merged.keep, merged.members = keep, members
    return merged


@torch.no_grad()
def inference_large_image(model, img, patch_size=640, patch_overlap_ratio=0.25, merge_iou_thr=0.25, merge_nms_type='nms',
                          batch_size=1, masks='rle', return_patches=False, seam_iou_thr=0.5, polygon_tolerance=None,
                          polygon_min_ring_area=0, oriented_boxes=False, min_mask_region_area=0, flatten=False,
                          flatten_min_ratio=0.0, polygon_topology='rings', buffer=0.0):
    """demo/large_image_demo.py:105-170 as one call.  img: path, ndarray or tensor [H, W, 3] (BGR like TestPipeline);
    patch_size: int or (h, w).  Returns a DetDataSample with ori_shape = (H, W) and pred_instances.{bboxes, scores,
    labels} on the device in batched_nms' keep order; pred_instances.masks is a list of dict(size=[H, W], counts=bytes)
    (masks='rle'), a bool [K, H, W] device tensor (masks='dense'), or per instance the list of (ring int32 [m, 2], parent,
    area2) of DESIGN §14.7 (masks='polygons': traced on the device from the scene run table; polygon_tolerance in pixels and
    polygon_min_ring_area in pixels simplify the rings there first, DESIGN §14.8 -- apis.masks_to_polygons says how; they
    apply to masks='polygons' only; polygon_topology='shared', DESIGN §14.15, simplifies every border between two instances
    once, to the same vertices in both rings: it requires masks='polygons', flatten on, a polygon_tolerance -- 0 is legal --
    and polygon_min_ring_area 0; with min_mask_region_area the last step is a flatten, so the table is disjoint).
    oriented_boxes=True (masks='rle' or 'polygons'): pred_instances.obb is float64 numpy
    [K, 4, 2], the corners of the minimum-area rectangle around each instance's scene mask (clockwise on screen,
    NaN for an empty mask), made on the device from the scene run table before any string is made.  min_mask_region_area > 0
    (masks='rle' or 'polygons'): holes and islands of fewer pixels than that are removed from every scene mask
    (segment-anything's remove_small_regions, 'both', in the run domain; with 'seam_mask' after the union), before strings,
    rings and oriented boxes are made; bboxes, scores and labels stay the detector's, no mask is emptied, and
    pred_instances.region_changed is bool [K].  flatten='score' | 'area' (masks='rle' or 'polygons'): the scene
    masks are made pairwise disjoint, a planar layer -- every pixel stays with the covering instance of highest score ('score',
    ties to the lower index) or smallest scene mask ('area') -- on the scene run table, after the shift or union and before
    the min_mask_region_area cleaning, strings, rings and oriented boxes; where the cleaning is on, the cleaned table is
    flattened once more so that a filled hole cannot overlap the instance inside it.  flatten_min_ratio in [0, 1] empties an
    instance that keeps less than that share of its pixels (apis.flatten_masks).  K, bboxes, scores and labels stay the
    detector's; pred_instances.flatten_kept is bool [K] (False: the instance kept no pixel or was emptied) and flatten_area
    int32 [K, 2], the pixels of each scene mask before and in the result.  buffer (masks='rle' or 'polygons'): a
    signed real number of pixels; every scene mask is grown (> 0) or shrunk (< 0, the outside of the scene counting as set) by
    the exact Euclidean disc (apis.buffer_masks) as the first step on the scene run table, before flatten and cleaning, so
    overlaps that growth creates are resolved by flatten; bboxes, scores and labels stay the detector's, polygons, oriented
    boxes and strings are made from the buffered table, and pred_instances.buffer_area is int32 [K, 2] (before, after).
    return_patches=True: (sample, per-tile samples,
    starting_pixels).  merge_nms_type='seam_mask' (DESIGN §14.6): instances of different tiles with one label whose masks
    agree inside the tiles' common rectangle (IoU there >= seam_iou_thr) are fragments of one object and come back as ONE
    instance -- mask = the union, score = the maximum, box = the hull of the members' boxes -- before the same box NMS;
    `sample.keep` then holds the representatives (the best-scored member) and `sample.members` the index lists.
    merge_nms_type='nms_rotated' (masks='rle' or 'polygons'): the merge suppresses by the IoU of the instances'
    ORIENTED boxes -- the minimum-area rectangle of every tile instance, from the tile run tables the loop makes, moved by its
    tile origin in integers -- with mmcv.ops.nms_rotated's rule at merge_iou_thr (two ships moored side by side at 45 degrees
    overlap as axis-aligned boxes and not at all as oriented ones); everything downstream of `keep` is 'nms''s,
    pred_instances.bboxes stay axis-aligned and oriented_boxes=True still reports the scene-table rectangles.  One rotated NMS
    holds ops.OBB_NMS_MAX = 32 768 boxes (its suppression mask has n^2 / 8 bytes): a scene whose tiles return more instances
    than that in all is refused with a ValueError when the merge starts, after the tiles have run -- raise the detector's score
    threshold or lower its max_per_img, or merge with 'nms'."""
    from .apis import TestPipeline, get_test_pipeline_cfg
    if merge_nms_type not in ('nms', 'seam_mask', 'nms_rotated'):
        raise NotImplementedError(f"merge_nms_type {merge_nms_type!r}: only 'nms', 'seam_mask' and 'nms_rotated' are "
                                  'implemented (soft_nms and the other mmcv variants are not)')
    seam = merge_nms_type == 'seam_mask'
    rotated = merge_nms_type == 'nms_rotated'
    if rotated and masks == 'dense':                                    # refused before the first tile runs
        raise ValueError("merge_nms_type='nms_rotated' reads the tile run tables: use masks='rle' or masks='polygons'")
    if rotated and getattr(model, 'with_mask', True) is False:          # refused before the first tile runs
        raise ValueError("merge_nms_type='nms_rotated' compares the masks' rectangles: the detector returns no masks")
    if masks not in ('rle', 'dense', 'polygons'):
        raise ValueError("masks must be 'rle', 'dense' or 'polygons'")
    poly = masks == 'polygons'
    if oriented_boxes and masks == 'dense':                             # refused before the first tile runs
        raise ValueError("oriented_boxes=True reads the scene run table: use masks='rle' or masks='polygons'")
    obb = [] if oriented_boxes else None
    from .sam_prompts import _check_region_area
    region_area = _check_region_area(min_mask_region_area)              # refused before the first tile runs
    region = (region_area, []) if region_area else None
    if region is not None and masks == 'dense':                         # refused before the first tile runs
        raise ValueError("min_mask_region_area cleans the scene run table: use masks='rle' or masks='polygons' (dense masks "
                         'are cleaned by apis.remove_small_regions)')
    flat_order, flat_ratio = _check_flatten(flatten, flatten_min_ratio)  # refused before the first tile runs
    if flat_order is not None and masks == 'dense':
        raise ValueError("flatten works on the scene run table: use masks='rle' or masks='polygons' (dense masks go through "
                         'apis.flatten_masks)')
    flat_out = []
    buf_dist = _check_buffer(buffer)                                    # refused before the first tile runs
    if buf_dist is not None and masks == 'dense':
        raise ValueError("buffer works on the scene run table: use masks='rle' or masks='polygons' (dense masks go through "
                         'apis.buffer_masks)')
    buf = (buf_dist, []) if buf_dist is not None else None
    if polygon_tolerance is not None or polygon_min_ring_area != 0:
        if not poly:
            raise ValueError("polygon_tolerance and polygon_min_ring_area apply to masks='polygons'")
        poly = (0 if polygon_tolerance is None else polygon_tolerance, polygon_min_ring_area)
        rle.polygon_tolerance_q8(poly[0])                               # refused before the first tile runs
        rle.polygon_min_ring_area(poly[1])
    if rle.polygon_topology(polygon_topology, polygon_tolerance if poly else 0, polygon_min_ring_area if poly else 0):
        if not poly:                                                    # refused before the first tile runs
            raise ValueError("polygon_topology='shared' applies to masks='polygons'")
        if flat_order is None:
            raise ValueError("polygon_topology='shared' needs pairwise disjoint instances: turn flatten on (flatten='score' "
                             "or flatten='area')")
        poly = (polygon_tolerance, 0, 'shared')
    ph_, pw_ = (int(patch_size), int(patch_size)) if isinstance(patch_size, (int, float)) else (int(patch_size[0]), int(patch_size[1]))
    if pw_ > MAX_PATCH_WIDTH:
        raise ValueError(f'a patch {pw_} pixels wide: the tile RLE kernel is specified for widths up to {MAX_PATCH_WIDTH}')
    dev = next(model.parameters()).device
    ops.require_device(dev)
    pipe = TestPipeline(get_test_pipeline_cfg(model.cfg), device=dev)
    img_path = None
    if isinstance(img, (str, os.PathLike)):
        img_path = str(img)
        img = pipe._decode(img_path)
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError('expected an [H, W, 3] image')
    H, W = int(img.shape[0]), int(img.shape[1])
    if H * W >= 2 ** 31:
        raise ValueError(f'a {H} x {W} scene has {H * W} pixels; COCO run counts are 32-bit (< 2^31 pixels)')
    scene = img.to(dev).contiguous()                                    # the one upload
    tiles = slice_bboxes(H, W, ph_, pw_, patch_overlap_ratio, patch_overlap_ratio)
    starting_pixels = [(t[0], t[1]) for t in tiles]
    th, tw = min(ph_, H), min(pw_, W)
    nh, nw, ph, pw, meta = pipe.geometry(th, tw)
    origins = torch.tensor(starting_pixels, dtype=torch.int32).reshape(-1, 2).to(dev)

    boxes, scores, labels, tile_of, runs, run_n, dense_tiles, patch_samples = [], [], [], [], [], [], [], []
    cap = 4096
    for b0 in range(0, len(tiles), batch_size):
        nb = min(batch_size, len(tiles) - b0)
        inputs = ops.slice_resize_pad(scene, origins[b0:b0 + nb], (th, tw), (nh, nw), (ph, pw), pipe.pad_val)
        samples = [DetDataSample(metainfo={k: v for k, v in dict(meta, img_id=b0 + j, img_path=img_path).items()
                                           if k in pipe.meta_keys}) for j in range(nb)]
        res = model.test_step(dict(inputs=[inputs[j] for j in range(nb)], data_samples=samples))
        insts = [r.pred_instances for r in res]
        for j, p in enumerate(insts):
            if p.bboxes.shape[-1] != 4:
                raise NotImplementedError(f'boxes with {p.bboxes.shape[-1]} columns (rotated boxes) are not supported')
            boxes.append(p.bboxes)
            scores.append(p.scores)
            labels.append(p.labels)
            tile_of.append(torch.full((int(p.scores.shape[0]),), b0 + j, dtype=torch.int64, device=dev))
        if all('masks' in p and p.masks is not None for p in insts):
            bm = torch.cat([p.masks for p in insts], 0).to(torch.bool)
            if masks == 'dense':
                dense_tiles.append(bm)
            if masks != 'dense' or seam:                                # the seam merge compares runs in either form
                c, n, _, cap = rle.encode_runs(bm, cap)                 # the batch's dense masks go once the runs fit
                runs.append(c)
                run_n.append(n)
            del bm
        elif seam:
            raise ValueError("merge_nms_type='seam_mask' compares masks: the detector returned none")
        elif rotated:
            raise ValueError("merge_nms_type='nms_rotated' compares the masks' rectangles: the detector returned none")
        if return_patches:
            patch_samples.extend(res)
        del res, insts

    cat = (lambda xs, dt: torch.cat(xs, 0) if xs else torch.zeros((0,), dtype=dt, device=dev))
    tile_of = cat(tile_of, torch.int64)
    off_all = origins.to(torch.int64)[tile_of]                          # [n, 2] = (ox, oy)
    all_boxes = (torch.cat(boxes, 0) if boxes else torch.zeros((0, 4), device=dev))
    all_boxes = all_boxes + torch.cat([off_all, off_all], 1).to(all_boxes.dtype)       # sahi shift_bboxes, fp32
    all_scores, all_labels = cat(scores, torch.float32), cat(labels, torch.int64)
    members = None
    if seam:
        ac = rle.concat_runs(runs, device=dev)
        an = torch.cat(run_n, 0) if run_n else torch.zeros((0,), dtype=torch.int32, device=dev)
        out, keep, members, groups = _seam_merge(all_boxes, all_scores, all_labels, tile_of, tiles, ac, an, (th, tw), (H, W),
                                                 seam_iou_thr, merge_iou_thr)
        origin = off_all.to(torch.int32)
        if masks == 'dense':
            tm = torch.cat(dense_tiles, 0) if dense_tiles else torch.zeros((0, th, tw), dtype=torch.bool, device=dev)
            out.masks = _seam_dense(tm, origin, groups, (H, W))
        else:
            planar = (flat_order, flat_ratio, out.scores, flat_out) if flat_order else None
            out.masks = _seam_rle(ac, an, origin, groups, (th, tw), (H, W), poly, obb, region, planar, buf)
    else:
        all_runs = None
        if rotated:
            all_runs = rle.concat_runs(runs, device=dev)                # every tile instance's runs: the rectangles read them
            keep = _rotated_keep(all_runs, cat(run_n, torch.int32), (th, tw), off_all, all_scores, all_labels, merge_iou_thr)
        else:
            keep = ops.nms_flat(all_boxes, all_scores, all_labels, merge_iou_thr)
        out = InstanceData(bboxes=all_boxes[keep], scores=all_scores[keep], labels=all_labels[keep])
        koff = off_all[keep].to(torch.int32).contiguous()
        if masks == 'dense' and dense_tiles:
            _check_dense(keep.shape[0], H, W)
            out.masks = ops.paste_tiles(torch.cat(dense_tiles, 0)[keep], koff, (H, W))
        elif runs:
            # only the kept instances' runs are gathered ('nms_rotated' has the whole table already)
            kc = rle.concat_runs(runs, keep) if all_runs is None else all_runs[keep].contiguous()
            planar = (flat_order, flat_ratio, out.scores, flat_out) if flat_order else None
            out.masks = _scene_rle(kc, torch.cat(run_n, 0)[keep].contiguous(), koff, (th, tw), (H, W), poly, obb, region, planar,
                                   buf)
    if obb:
        out.obb = obb[0]
    if region is not None:
        out.region_changed = region[1][0] if region[1] else torch.zeros((len(out.scores),), dtype=torch.bool, device=dev)
    if flat_order is not None:
        K = len(out.scores)
        out.flatten_kept = flat_out[0][0] if flat_out else torch.zeros((K,), dtype=torch.bool, device=dev)
        out.flatten_area = flat_out[0][1] if flat_out else torch.zeros((K, 2), dtype=torch.int32, device=dev)
    if buf is not None:
        out.buffer_area = buf[1][0] if buf[1] else torch.zeros((len(out.scores), 2), dtype=torch.int32, device=dev)
    sample = DetDataSample(metainfo=dict(img_path=img_path, ori_shape=(H, W), img_shape=(H, W), img_id=0))
    sample.pred_instances = out
    sample.keep = keep                                                  # indices into the tile-ordered concatenation
    if members is not None:
        sample.members = members                                        # per output instance, its fragments
    if return_patches:
        return sample, patch_samples, starting_pixels
    return sample


def _is_rings(masks):
    return isinstance(masks, list) and all(isinstance(m, list) for m in masks)


def pred2dict(sample, score_thr=0.0):
    """DetInferencer.pred2dict form (det_inferencer.py:573-627): labels, scores, bboxes, masks as RLE with `counts` as str;
    the rings of masks='polygons' as dict(ring=[[x, y], ...], parent, area2) per ring; with oriented boxes an "obb" key, the
    four corners of each (NaN for an empty mask, which json writes as NaN)"""
    p = sample.pred_instances
    sel = (p.scores >= score_thr).nonzero().view(-1).tolist()
    lab, sc, bb = p.labels.tolist(), p.scores.tolist(), p.bboxes.tolist()
    out = dict(labels=[lab[i] for i in sel], scores=[sc[i] for i in sel], bboxes=[bb[i] for i in sel])
    if 'obb' in p and p.obb is not None:                               # oriented_boxes=True: [[x, y] x 4] per instance
        corners = np.asarray(p.obb).tolist()
        out['obb'] = [corners[i] for i in sel]
    if 'masks' in p and p.masks is not None:
        rles = p.masks
        if _is_rings(rles) and rles:                                   # a tensor (masks='dense') is no list: falls through
            out['masks'] = [[dict(ring=r.tolist(), parent=int(par), area2=int(a2)) for r, par, a2 in rles[i]] for i in sel]
            return out
        if isinstance(rles, torch.Tensor):
            rles = rle.encode_mask_results(rles) if rles.shape[0] else []
        out['masks'] = [dict(size=rles[i]['size'], counts=rles[i]['counts'].decode()) for i in sel]
    return out


def pred2geojson(sample, score_thr=0.0, transform=None):
    """a masks='polygons' result as a GeoJSON FeatureCollection: one feature per instance at or above score_thr, geometry
    from apis.rings_to_geojson (holes attached, rings closed, `transform` applied), properties label, score, bbox"""
    from .apis import rings_to_geojson
    p = sample.pred_instances
    if 'masks' not in p or p.masks is None:
        if len(p.scores):
            raise ValueError('pred2geojson: the detector returned no masks, so there are no geometries to write')
        return dict(type='FeatureCollection', features=[])
    if not _is_rings(p.masks):
        raise ValueError("pred2geojson needs the rings of inference_large_image(..., masks='polygons')")
    sel = (p.scores >= score_thr).nonzero().view(-1).tolist()
    lab, sc, bb = p.labels.tolist(), p.scores.tolist(), p.bboxes.tolist()
    feats = [dict(type='Feature', geometry=rings_to_geojson(p.masks[i], transform),
                  properties=dict(label=lab[i], score=sc[i], bbox=bb[i])) for i in sel]
    if 'obb' in p and p.obb is not None:                               # the corners in pixel coordinates, like bbox
        corners = np.asarray(p.obb).tolist()
        for f, i in zip(feats, sel):
            f['properties']['obb'] = corners[i]
    return dict(type='FeatureCollection', features=feats)


def geojson2dict(collection, size, transform=None, device='cuda:0'):
    """the reverse of pred2geojson: a GeoJSON FeatureCollection (or a list of features / geometries) of Polygon / MultiPolygon
    geometries -> the pred2dict form with the masks as COCO RLE on a size = (H, W) canvas, rasterised on the device with the
    even-odd rule (apis.polygons_to_masks); `transform` is the forward transform the layer was written with.
    labels / scores / bboxes come from the features' properties where every feature has them."""
    from .apis import polygons_to_masks
    feats = collection['features'] if isinstance(collection, dict) and 'features' in collection else list(collection)
    geoms = [f['geometry'] if isinstance(f, dict) and f.get('type') == 'Feature' else f for f in feats]
    rles = polygons_to_masks(geoms, size, form='rle', fill='evenodd', transform=transform, device=device) if geoms else []
    out = {}
    props = [f.get('properties') or {} if isinstance(f, dict) and f.get('type') == 'Feature' else {} for f in feats]
    for key, name in (('labels', 'label'), ('scores', 'score'), ('bboxes', 'bbox')):
        if all(name in p for p in props):
            out[key] = [p[name] for p in props]
    out['masks'] = [dict(size=r['size'], counts=r['counts'].decode()) for r in rles]
    return out


def _main_from_geojson(argv):
    import argparse
    ap = argparse.ArgumentParser(description='Rasterise a GeoJSON vector layer to COCO RLE masks on the device '
                                 '(the reverse of --mask-format geojson)')
    ap.add_argument('--from-geojson', required=True, metavar='FILE', help='a FeatureCollection of Polygon / MultiPolygon features')
    ap.add_argument('--size', type=int, nargs=2, required=True, metavar=('H', 'W'), help='the canvas of the masks in pixels')
    ap.add_argument('--geo-transform', type=float, nargs=6, default=None, metavar=('A', 'B', 'C', 'D', 'E', 'F'),
                    help='the forward transform the layer was written with: pixel corner (x, y) -> (A + B x + C y, D + E x + F y)')
    ap.add_argument('--out-dir', default='./output', help='<name>.json is written here')
    ap.add_argument('--device', default='cuda:0')
    a = ap.parse_args(argv)
    with open(a.from_geojson) as f:
        layer = json.load(f)
    try:
        out = geojson2dict(layer, a.size, a.geo_transform, a.device)
    except ValueError as e:
        ap.error(str(e))
    os.makedirs(a.out_dir, exist_ok=True)
    dst = os.path.join(a.out_dir, os.path.splitext(os.path.basename(a.from_geojson))[0] + '.json')
    with open(dst, 'w') as f:
        json.dump(out, f)
    print(f'{a.from_geojson}: {len(out["masks"])} instances -> {dst}')


def main(argv=None):
    import argparse
    import sys
    if any(str(t).split('=')[0] == '--from-geojson' for t in (sys.argv[1:] if argv is None else argv)):
        return _main_from_geojson(argv)                                # no model: --from-geojson FILE --size H W [--geo-transform ...]
    from .apis import DetInferencer, init_detector
    ap = argparse.ArgumentParser(description='Sliced inference on large images (demo/large_image_demo.py without drawing)')
    ap.add_argument('img', help='Image path or a directory of images')
    ap.add_argument('config', help='Config file')
    ap.add_argument('checkpoint', help='Checkpoint file')
    ap.add_argument('--out-dir', default='./output', help='one <name>.json per scene is written here')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--score-thr', type=float, default=0.3, help='Bbox score threshold')
    ap.add_argument('--patch-size', type=int, default=640, help='The size of patches')
    ap.add_argument('--patch-overlap-ratio', type=float, default=0.25, help='Ratio of overlap between two patches')
    ap.add_argument('--merge-iou-thr', type=float, default=0.25, help='IoU threshould for merging results')
    ap.add_argument('--merge-nms-type', default='nms', help="NMS type for merging results: 'nms', 'seam_mask' to join "
                    "the fragments of objects cut by tile seams first, or 'nms_rotated' to suppress by the IoU of the "
                    "instances' oriented boxes")
    ap.add_argument('--seam-iou-thr', type=float, default=0.5, help="mask IoU inside the tiles' overlap above which two "
                    "fragments are one object (--merge-nms-type seam_mask)")
    ap.add_argument('--batch-size', type=int, default=1, help='Batch size of patches')
    ap.add_argument('--mask-format', default='rle', choices=('rle', 'polygons', 'geojson'),
                    help="masks in <name>.json as COCO RLE (default) or as exact rings ('polygons'), or <name>.geojson: a "
                    "FeatureCollection with label, score and bbox properties ('geojson')")
    ap.add_argument('--geo-transform', type=float, nargs=6, default=None, metavar=('A', 'B', 'C', 'D', 'E', 'F'),
                    help='--mask-format geojson: pixel corner (x, y) -> (A + B x + C y, D + E x + F y)')
    ap.add_argument('--simplify-tolerance', type=float, default=None, metavar='T',
                    help='--mask-format polygons|geojson: Douglas-Peucker on the device, dropped vertices lie within T pixels '
                    'of the kept outline (default: the exact rings)')
    ap.add_argument('--min-ring-area', type=int, default=0, metavar='A',
                    help='--mask-format polygons|geojson: drop rings of less than A pixels (a dropped hole is filled)')
    ap.add_argument('--oriented-boxes', action='store_true',
                    help='add "obb": the four corners of the minimum-area rectangle around each mask, made on the device')
    ap.add_argument('--min-mask-region-area', type=int, default=0, metavar='A',
                    help='remove holes and islands of less than A pixels from every scene mask, on the device')
    ap.add_argument('--simplify-topology', default='rings', choices=rle.POLYGON_TOPOLOGIES,
                    help="'shared': simplify every border between two instances once, to the same vertices on both sides "
                         '(needs --flatten, --simplify-tolerance and --mask-format polygons or geojson; DESIGN 14.15)')
    ap.add_argument('--flatten', nargs='?', const='score', default=None, choices=('score', 'area'),
                    help="make the instances of a scene pairwise disjoint, a planar layer: every pixel stays with the covering "
                    "instance of highest score ('score', the default) or smallest mask ('area'), on the device")
    ap.add_argument('--flatten-min-ratio', type=float, default=0.0, metavar='R',
                    help='--flatten: empty an instance that keeps less than the share R of its pixels')
    ap.add_argument('--buffer', type=float, default=0.0, metavar='D',
                    help='grow (D > 0) or shrink (D < 0) every scene mask by the Euclidean disc of |D| pixels, on the device, '
                         'before --flatten and the cleaning (DESIGN 14.16)')
    a = ap.parse_args(argv)
    if a.geo_transform is not None and a.mask_format != 'geojson':
        ap.error('--geo-transform applies to --mask-format geojson')
    if (a.simplify_tolerance is not None or a.min_ring_area != 0) and a.mask_format == 'rle':
        ap.error('--simplify-tolerance and --min-ring-area apply to --mask-format polygons and geojson')
    try:
        rle.polygon_tolerance_q8(0 if a.simplify_tolerance is None else a.simplify_tolerance)
        rle.polygon_min_ring_area(a.min_ring_area)
        if a.min_mask_region_area < 0:
            raise ValueError(f'--min-mask-region-area must be a non-negative integer, got {a.min_mask_region_area}')
        _check_flatten(a.flatten or False, a.flatten_min_ratio)
        _check_buffer(a.buffer)
        if rle.polygon_topology(a.simplify_topology, a.simplify_tolerance, a.min_ring_area):
            if a.mask_format == 'rle':
                raise ValueError('--simplify-topology shared applies to --mask-format polygons and geojson')
            if not a.flatten:
                raise ValueError('--simplify-topology shared needs pairwise disjoint instances: add --flatten')
    except ValueError as e:
        ap.error(str(e))
    model = init_detector(a.config, None if a.checkpoint in ('', 'none', 'None') else a.checkpoint, device=a.device)
    os.makedirs(a.out_dir, exist_ok=True)
    for path in DetInferencer._inputs_to_list(a.img):
        s = inference_large_image(model, path, a.patch_size, a.patch_overlap_ratio, a.merge_iou_thr, a.merge_nms_type,
                                  a.batch_size, masks='rle' if a.mask_format == 'rle' else 'polygons',
                                  seam_iou_thr=a.seam_iou_thr, polygon_tolerance=a.simplify_tolerance,
                                  polygon_min_ring_area=a.min_ring_area, oriented_boxes=a.oriented_boxes,
                                  min_mask_region_area=a.min_mask_region_area, flatten=a.flatten or False,
                                  flatten_min_ratio=a.flatten_min_ratio, polygon_topology=a.simplify_topology,
                                  buffer=a.buffer)
        geo = a.mask_format == 'geojson'
        dst = os.path.join(a.out_dir, os.path.splitext(os.path.basename(path))[0] + ('.geojson' if geo else '.json'))
        with open(dst, 'w') as f:
            json.dump(pred2geojson(s, a.score_thr, a.geo_transform) if geo else pred2dict(s, a.score_thr), f)
        print(f'{path}: {len(s.pred_instances.scores)} instances -> {dst}')


if __name__ == '__main__':
    main()
