"""The dense numpy oracle of planar instance layers (csrc/run_flatten.hip), in two independent forms that
must agree (tests/_run_flatten_cases.check_oracle):

* `flatten`: the definition.  Over the masks that cover a pixel the one of smallest rank keeps it.
* `flatten_fusion`: a restatement of the loop of MaskFormerFusionHead.panoptic_postprocess (mmdet
  maskformer_fusion_head.py:70-104) for binary masks and distinct scores in (0, 1], with filter_low_score=True and
  iou_thr=0: float32 scores x masks, argmax over the queries, then per query `ids == k & masks[k] >= 0.5`.

min_ratio is NOT the reference's iou_thr (its mask_area is taken before filter_low_score and counts every uncovered pixel
for query 0); `apply_min_ratio` is the definition of the issue: area(F_i) < min_ratio * area(M_i) empties F_i after the
partition is made."""
import numpy as np


def flatten(masks, rank):
    """masks bool [k, H, W], rank a permutation (0 wins) -> bool [k, H, W]"""
    masks = np.asarray(masks, bool)
    k = masks.shape[0]
    if k == 0:
        return masks.copy()
    rank = np.asarray(rank, np.int64)
    cost = np.where(masks, rank[:, None, None], k)                       # k: not covered
    win = cost.argmin(0)                                                 # ranks are distinct: no tie among covering masks
    return masks & (win[None] == np.arange(k)[:, None, None])


def scores_of_rank(rank):
    """distinct float32 scores in (0, 1], the smaller the rank the larger"""
    k = len(rank)
    return ((k - np.asarray(rank, np.int64)) / np.float32(k)).astype(np.float32)


def flatten_fusion(masks, scores):
    """panoptic_postprocess' loop on binary masks -> bool [k, H, W]"""
    masks = np.asarray(masks, bool)
    k = masks.shape[0]
    if k == 0:
        return masks.copy()
    cur_masks = masks.astype(np.float32)
    cur_prob_masks = np.asarray(scores, np.float32).reshape(-1, 1, 1) * cur_masks
    cur_mask_ids = cur_prob_masks.argmax(0)
    out = np.zeros_like(masks)
    for q in range(k):
        mask = cur_mask_ids == q
        mask_area = int(mask.sum())
        original_area = int((cur_masks[q] >= 0.5).sum())
        mask = mask & (cur_masks[q] >= 0.5)                              # filter_low_score=True
        if mask_area > 0 and original_area > 0:                          # iou_thr = 0: no ratio test
            out[q] = mask
    return out


def rank_of_scores(scores):
    """descending score, ties to the lower index"""
    first = np.argsort(-np.asarray(scores, np.float64), kind='stable')
    rank = np.empty(len(first), np.int64)
    rank[first] = np.arange(len(first))
    return rank


def rank_of_areas(masks):
    """ascending area, ties to the lower index"""
    first = np.argsort(np.asarray(masks, bool).reshape(len(masks), -1).sum(1), kind='stable')
    rank = np.empty(len(first), np.int64)
    rank[first] = np.arange(len(first))
    return rank


def apply_min_ratio(masks, flat, min_ratio):
    """-> (flat with the instances of area(F_i) < min_ratio * area(M_i) emptied, kept bool [k]); float64 comparison"""
    masks, flat = np.asarray(masks, bool), np.asarray(flat, bool).copy()
    k = masks.shape[0]
    before = masks.reshape(k, -1).sum(1).astype(np.float64)
    after = flat.reshape(k, -1).sum(1).astype(np.float64)
    kept = (after > 0) & (after >= np.float64(min_ratio) * before)
    flat[~kept] = False
    return flat, kept


def label_map(flat, ids=None):
    """sum_i ids[i] * F_i, int64 [H, W]"""
    flat = np.asarray(flat, bool)
    k = flat.shape[0]
    ids = np.arange(1, k + 1) if ids is None else np.asarray(ids, np.int64)
    return (ids[:, None, None] * flat.astype(np.int64)).sum(0) if k else np.zeros(flat.shape[1:], np.int64)
