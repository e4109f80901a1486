"""TEST ORACLE: merging instances cut by tile seams, restated on numpy / plain Python.

The definition works on scene-frame masks M of instances that carry a label, a score, an fp32 box and the tile they came
from.  For i, j of DIFFERENT tiles with ONE label whose tiles' rectangles meet in R = rect(A) & rect(B) of positive area:
    inter = |M_i & M_j|        a_i = |M_i & R|        a_j = |M_j & R|        union_R = a_i + a_j - inter
    (i, j) is an edge  iff  inter > 0 and float(inter) >= float(thr) * float(union_R)
Connected components of the edges are merged: mask = OR, label = the common one, score = max, box = element-wise min / max,
representative = highest score (lowest index among equals); merged instances in ascending order of the representative;
then the class-aware box NMS that is handed in.

Two forms: dense (`*_dense`, boolean arrays; the definition itself) and an interval-domain twin (`iv_*`: a mask is the
sorted array of the [start, end) intervals of its ones in the column-major stream) for scenes whose dense form does not fit;
the CPU tier checks the twin against the dense form.  Nothing here imports the package under test."""
import numpy as np

from _large_image_ref import rle_counts_np, shift_bboxes, shift_masks


# ------------------------------------------------------------------------------------------------------------- dense
def bbox_area_dense(mask):
    """tight (x0, y0, x1, y1) end-exclusive (zeros when empty), area"""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return [0, 0, 0, 0], 0
    return [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1], int(ys.size)


def clip_rect(rect, H, W):
    x0, y0, x1, y1 = (int(v) for v in rect)
    return min(max(x0, 0), W), min(max(y0, 0), H), min(max(x1, 0), W), min(max(y1, 0), H)


def pair_overlap_dense(mi, mj, rect):
    H, W = mi.shape
    x0, y0, x1, y1 = clip_rect(rect, H, W)
    inr = np.zeros((H, W), bool)
    if x1 > x0 and y1 > y0:
        inr[y0:y1, x0:x1] = True
    return int((mi & mj).sum()), int((mi & inr).sum()), int((mj & inr).sum())


def is_edge(inter, a_i, a_j, thr):
    return inter > 0 and float(inter) >= float(thr) * float(a_i + a_j - inter)


def rect_intersection(ra, rb):
    x0, y0, x1, y1 = max(ra[0], rb[0]), max(ra[1], rb[1]), min(ra[2], rb[2]), min(ra[3], rb[3])
    return (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else None


def components(n, edges, scores):
    """-> list of (representative, members ascending), ascending by representative"""
    label = list(range(n))
    changed = True
    while changed:                                             # label propagation: no union-find, another algorithm
        changed = False
        for i, j in edges:
            m = min(label[i], label[j])
            if label[i] != m or label[j] != m:
                label[i] = label[j] = m
                changed = True
    out = []
    for root in sorted(set(label)):
        mem = [i for i in range(n) if label[i] == root]
        best = max(float(scores[i]) for i in mem)
        out.append(([i for i in mem if float(scores[i]) == best][0], mem))
    out.sort(key=lambda g: g[0])
    return out


def _merge(n, overlap, boxes, scores, labels, tile, tile_rects, seam_thr, batched_nms, nms_thr):
    """the graph part, shared by the two forms; overlap(i, j, rect) -> (inter, a_i, a_j)"""
    import torch
    edges, rejected, evaluated = [], [], []
    by_tile = {}
    for i in range(n):
        by_tile.setdefault(tile[i], []).append(i)
    tiles = sorted(by_tile)
    for a, ta in enumerate(tiles):
        for tb in tiles[a + 1:]:
            rect = rect_intersection(tile_rects[ta], tile_rects[tb])
            if rect is None:
                continue
            for i in by_tile[ta]:
                for j in by_tile[tb]:
                    if labels[i] != labels[j]:
                        continue
                    inter, ai, aj = overlap(i, j, rect)
                    evaluated.append((i, j, rect, inter, ai, aj))
                    if is_edge(inter, ai, aj, seam_thr):
                        edges.append((i, j))
                    elif inter > 0:
                        rejected.append((i, j))
    comps = components(n, edges, scores)
    mb = np.zeros((len(comps), 4), np.float32)
    for g, (_, mem) in enumerate(comps):
        mb[g, :2] = boxes[mem][:, :2].min(0)
        mb[g, 2:] = boxes[mem][:, 2:].max(0)
    ms = np.asarray([scores[r] for r, _ in comps], np.float32)
    ml = np.asarray([labels[r] for r, _ in comps], np.int64)
    if len(comps):
        _, keep = batched_nms(torch.from_numpy(mb), torch.from_numpy(ms), torch.from_numpy(ml), nms_thr)
        keep = keep.numpy().tolist()
    else:
        keep = []
    return dict(edges=edges, rejected=rejected, evaluated=evaluated, comps=comps, n_merged=len(comps), kept=keep,
                keep=[comps[g][0] for g in keep], members=[comps[g][1] for g in keep],
                bboxes=mb[keep].reshape(-1, 4), scores=ms[keep], labels=ml[keep])


def concat_tiles(tile_results, offsets):
    """tile-ordered concatenation: scene-frame fp32 boxes, scores, labels, tile index"""
    boxes = np.concatenate([shift_bboxes(r['bboxes'], o) for r, o in zip(tile_results, offsets)], 0)
    scores = np.concatenate([np.asarray(r['scores'], np.float32) for r in tile_results], 0)
    labels = np.concatenate([np.asarray(r['labels'], np.int64) for r in tile_results], 0)
    tile = np.concatenate([np.full(len(r['scores']), i, np.int64) for i, r in enumerate(tile_results)], 0)
    return boxes, scores, labels, tile


def seam_merge_dense(tile_results, offsets, tile_rects, full_shape, seam_thr, batched_nms, nms_thr):
    """tile_results: per tile dict(bboxes fp32 [n, 4], scores, labels, masks bool [n, h, w]).  Returns the dict of _merge
    plus masks (dense union per kept instance) and counts (their COCO run counts)."""
    boxes, scores, labels, tile = concat_tiles(tile_results, offsets)
    scene = [shift_masks(m[None], offsets[t], full_shape)[0] for t, r in enumerate(tile_results) for m in r['masks']]
    out = _merge(len(scene), lambda i, j, rect: pair_overlap_dense(scene[i], scene[j], rect), boxes, scores, labels,
                 tile.tolist(), tile_rects, seam_thr, batched_nms, nms_thr)
    out['masks'] = [np.logical_or.reduce([scene[i] for i in mem]) for mem in out['members']]
    out['counts'] = [rle_counts_np(m) for m in out['masks']]
    return out


# ---------------------------------------------------------------------------------------------------------- intervals
def counts_to_iv(counts):
    """COCO run counts -> int64 [r, 2] = [start, end) of the ones-runs"""
    c = np.asarray(counts, np.int64)
    ends = np.cumsum(c)
    starts = ends - c
    iv = np.stack([starts[1::2], ends[1::2]], 1)
    return iv[iv[:, 1] > iv[:, 0]]


def _coverage(ivs):
    """sweep over the boundaries of several interval sets -> (positions sorted, how many sets cover [pos[t], pos[t + 1]))"""
    pos = np.concatenate([iv.reshape(-1) for iv in ivs] + [np.zeros(0, np.int64)])
    delta = np.concatenate([np.tile([1, -1], len(iv)) for iv in ivs] + [np.zeros(0, np.int64)])
    order = np.argsort(pos, kind='stable')
    return pos[order], np.cumsum(delta[order])


def iv_inter(a, b):
    pos, cov = _coverage([a, b])
    return int((np.diff(pos) * (cov[:-1] == 2)).sum()) if pos.size else 0


def iv_rect(rect, H, W):
    x0, y0, x1, y1 = clip_rect(rect, H, W)
    if x1 <= x0 or y1 <= y0:
        return np.zeros((0, 2), np.int64)
    x = np.arange(x0, x1, dtype=np.int64)
    return np.stack([x * H + y0, x * H + y1], 1)


def iv_pair_overlap(a, b, rect, H, W):
    r = iv_rect(rect, H, W)
    return iv_inter(a, b), iv_inter(a, r), iv_inter(b, r)


def iv_union_counts(ivs, H, W):
    """canonical COCO run counts of the union of several interval sets on an (H, W) canvas"""
    pos, cov = _coverage(list(ivs))
    counts, at, val = [], 0, 0
    for t in range(len(pos) - 1):
        v = 1 if cov[t] > 0 else 0
        if pos[t + 1] == pos[t]:
            continue
        if v != val:
            counts.append(int(pos[t]) - at)
            at, val = int(pos[t]), v
    if val == 1:                                              # close the last ones-run at the last boundary
        counts.append(int(pos[-1]) - at)
        at = int(pos[-1])
    if at < H * W or not counts:
        counts.append(H * W - at)
    return counts


def iv_bbox_area(iv, H):
    if len(iv) == 0:
        return [0, 0, 0, 0], 0
    s, e1 = iv[:, 0], iv[:, 1] - 1
    xa, xb = s // H, e1 // H
    one = xa == xb
    y0 = np.where(one, s - xa * H, 0).min()
    y1 = np.where(one, e1 - xb * H + 1, H).max()
    return [int(xa.min()), int(y0), int(xb.max()) + 1, int(y1)], int((iv[:, 1] - iv[:, 0]).sum())


def seam_merge_iv(ivs, boxes, scores, labels, tile, tile_rects, full_shape, seam_thr, batched_nms, nms_thr):
    """the interval-domain twin: ivs = scene-frame interval arrays of the tile-ordered instances, boxes already in the
    scene frame.  Pairs are pruned by the tight boxes first (exact).  Returns the dict of _merge plus counts."""
    H, W = full_shape
    tight = [iv_bbox_area(iv, H)[0] for iv in ivs]

    def overlap(i, j, rect):
        a, b = tight[i], tight[j]
        if not (a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]):
            return 0, 0, 0                                    # inter == 0: never an edge, never a rejected pair
        return iv_pair_overlap(ivs[i], ivs[j], rect, H, W)
    out = _merge(len(ivs), overlap, np.asarray(boxes, np.float32), scores, labels, list(tile), tile_rects, seam_thr,
                 batched_nms, nms_thr)
    out['counts'] = [iv_union_counts([ivs[i] for i in mem], H, W) for mem in out['members']]
    return out
