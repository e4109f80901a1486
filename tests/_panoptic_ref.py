"""The reference of the panoptic-fusion tests (csrc/panoptic_fuse.hip): MaskFormerFusionHead.panoptic_postprocess
(mmdet maskformer_fusion_head.py:41-106) on the dense fp64 mask field of tests/_mask_field_props.py, twice:

* `fuse_loop`: a restatement of the reference's loop (fp64 softmax and sigmoid, argmax(0), the Python loop over the kept
  queries with its float division);
* `fuse_arrays`: the definition the kernels implement, as array operations (argmax, bincount, cumsum).

`reference()` evaluates both, asserts that they agree (==) and returns the second with the per-pixel figures the tolerance
rules need: the fp64 gap between the two largest products, the scores of those two, and whether they are exact duplicates (the
same class row and the same field value: the device computes the same bits for both, the lower index wins).  Nothing here
goes through a kernel, `ops` or `torch_ops_mock`."""
import numpy as np
import torch

import _mask_field_props as mf

INSTANCE_OFFSET = 1000            # mmdet/evaluation/functional/panoptic_utils.py:18


def select(cls, nc, object_mask_thr):
    """(score fp64 [Nq], label [Nq], keep bool [Nq]): maskformer_fusion_head.py:62-65 in fp64"""
    p = torch.softmax(cls.detach().cpu().double(), -1)
    score, label = torch.from_numpy(p.numpy().max(-1)), torch.from_numpy(p.numpy().argmax(-1))      # numpy: the first maximum
    return score, label, (label != nc) & (score > object_mask_thr)


def fuse_loop(cls, field, num_things, nc, object_mask_thr=0.8, iou_thr=0.8, filter_low_score=False):
    """the reference's procedure, step by step, on the fp64 fields [Nq, oh, ow] of ALL queries: one pass over the kept queries
    in order, each painting over the void map -> (sem int32 [oh, ow], segment [Nq], mask_area [Nq], original_area [Nq])"""
    score, label, keep = select(cls, nc, object_mask_thr)
    Nq = cls.shape[0]
    oh, ow = field.shape[-2:]
    sem = torch.full((oh, ow), nc, dtype=torch.int32)
    segment, m_area, o_area = [-1] * Nq, [0] * Nq, [0] * Nq
    qs = [q for q in range(Nq) if bool(keep[q])]
    if not qs:
        return sem, segment, m_area, o_area
    prob = field[qs].sigmoid()                                                   # [K, oh, ow]
    leader = torch.from_numpy((score[qs].view(-1, 1, 1) * prob).numpy().argmax(0))
    next_id = 1
    for k, q in enumerate(qs):
        won = leader == k
        inside = prob[k] >= 0.5
        m_area[q], o_area[q] = int(won.sum()), int(inside.sum())
        if m_area[q] == 0 or o_area[q] == 0:
            continue
        if m_area[q] / o_area[q] < iou_thr:                                      # Python's float division, as the reference's
            continue
        c = int(label[q])
        if c < num_things:
            segment[q] = c + next_id * INSTANCE_OFFSET
            next_id += 1
        else:
            segment[q] = c                                                       # stuff of one class shares the bare label
        sem[won & inside if filter_low_score else won] = segment[q]
    return sem, segment, m_area, o_area


def fuse_arrays(cls, field, num_things, nc, object_mask_thr=0.8, iou_thr=0.8, filter_low_score=False):
    """the definition: select, argmax, bincount, the ratio test, cumsum over the painted things, a lookup.  Returns a dict:
    sem int32 [oh, ow], segment / mask_area / original_area lists [Nq], kept (query indices), score fp64 [Nq], winner int64
    [oh, ow] (kept index, -1 without kept queries), gap fp64 [oh, ow], pair_scores fp64 [oh, ow], duplicate bool [oh, ow],
    near_zero [K] (pixels of every kept field with |v| < mf.NEAR)."""
    cls64 = cls.detach().cpu().double()
    score, label, keep = select(cls, nc, object_mask_thr)
    kept = keep.nonzero()[:, 0]
    K, Nq = int(kept.numel()), cls.shape[0]
    oh, ow = field.shape[-2:]
    res = dict(kept=kept.tolist(), score=score, winner=torch.full((oh, ow), -1, dtype=torch.int64),
               gap=torch.full((oh, ow), float('inf'), dtype=torch.float64), pair_scores=torch.zeros(oh, ow, dtype=torch.float64),
               duplicate=torch.zeros(oh, ow, dtype=torch.bool), near_zero=[])
    segment, m_area, o_area = np.full(Nq, -1), np.zeros(Nq, dtype=np.int64), np.zeros(Nq, dtype=np.int64)
    sem = torch.full((oh, ow), nc, dtype=torch.int32)
    if K:
        v = field[kept]
        prod = (score[kept].view(-1, 1, 1) * v.sigmoid()).numpy()
        win = prod.argmax(0)                                                    # the lowest kept index on an exact tie
        res['winner'] = torch.from_numpy(win)
        ma = np.bincount(win.ravel(), minlength=K)
        pos = (v >= 0).numpy()
        oa = pos.reshape(K, -1).sum(1)
        res['near_zero'] = (v.abs() < mf.NEAR).flatten(1).sum(1).tolist()
        if K > 1:
            order = np.argsort(-prod, axis=0, kind='stable')[:2]
            top = np.take_along_axis(prod, order, 0)
            res['gap'] = torch.from_numpy(top[0] - top[1])
            sk = score[kept].numpy()
            res['pair_scores'] = torch.from_numpy(sk[order[0]] + sk[order[1]])
            rows = cls64[kept]
            same_row = (rows[:, None, :] == rows[None, :, :]).all(-1).numpy()
            vn = v.numpy()
            res['duplicate'] = torch.from_numpy((top[0] == top[1]) & same_row[order[0], order[1]] &
                                                (np.take_along_axis(vn, order[:1], 0)[0] == np.take_along_axis(vn, order[1:2], 0)[0]))
        with np.errstate(divide='ignore', invalid='ignore'):
            painted = (ma > 0) & (oa > 0) & ~(ma.astype(np.float64) / oa.astype(np.float64) < iou_thr)
        lab = label[kept].numpy()
        thing = painted & (lab < num_things)
        ids = np.cumsum(thing)                                                   # instance ids from 1, painted things only
        seg = np.where(thing, lab + ids * INSTANCE_OFFSET, lab)
        lut = np.where(painted, seg, nc)
        out = lut[win]
        if filter_low_score:
            out = np.where(np.take_along_axis(pos, win[None], 0)[0], out, nc)
        sem = torch.from_numpy(out.astype(np.int32))
        segment[kept.numpy()] = np.where(painted, seg, -1)
        m_area[kept.numpy()], o_area[kept.numpy()] = ma, oa
    res.update(sem=sem, segment=segment.tolist(), mask_area=m_area.tolist(), original_area=o_area.tolist())
    return res


def reference(cls, low, geo, num_things, nc, **cfg):
    """both forms on field_f64 of all queries (geo = (img, crop, out)); they must agree"""
    field = mf.field_f64(low, *geo)
    a = fuse_arrays(cls, field, num_things, nc, **cfg)
    sem, segment, m_area, o_area = fuse_loop(cls, field, num_things, nc, **cfg)
    assert torch.equal(sem, a['sem']), 'the two forms of the reference disagree on the map'
    assert segment == a['segment'] and m_area == a['mask_area'] and o_area == a['original_area'], \
        ('the two forms of the reference disagree', segment, a['segment'], m_area, a['mask_area'], o_area, a['original_area'])
    a['field'] = field
    return a
