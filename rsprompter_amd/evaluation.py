"""`METRICS` registry and `CocoMetric`: box and mask mAP with mmdet's surface (mmdet/evaluation/metrics/coco_metric.py),
without pycocotools.  The per-pair and per-(image, category) work of COCOeval.evaluate runs on the device
(csrc/cocoeval.hip: string decode, bits, IoU, greedy matching); accumulate / summarize stay on the host in float64 numpy
with pycocotools' arithmetic.

The segm IoU has two routes with the same doubles (`iou_domain`): bit planes (`'bits'`, the default) and run tables
(`'runs'`, csrc/coco_iou_runs.hip: scenes whose masks never exist as bits); `'auto'` chooses by size.

Both ground-truth paths of the reference work and give the reference's (different) numbers:
  * no `ann_file` (every RSPrompter config): the ground truth of the data samples, converted as `gt_to_coco_json` does
    (annotation ids from 1, category ids 0..C-1, every instance non-crowd, area = float32 box area w * h);
  * `ann_file`: the JSON as it is (crowd flags, the JSON's areas and annotation ids).

`CocoPanopticMetric` (mmdet/evaluation/metrics/coco_panoptic_metric.py) is at the end: PQ / SQ / RQ of panoptic maps with
the per-image confusion and matching on the device (csrc/panoptic_quality.hip), without panopticapi.
"""
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from . import ops, rle
from .datasets import ann_to_rle, anns_to_rle
from .registry import Registry

METRICS = Registry('metric')

AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
AREA_LBL = ('all', 'small', 'medium', 'large')
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
STAT_NAMES = ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l', 'AR@100', 'AR@300', 'AR@1000', 'AR_s@1000',
              'AR_m@1000', 'AR_l@1000')


def _get(obj, key, default=None):
    return obj.get(key, default) if isinstance(obj, dict) else getattr(obj, key, default)


def _np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _segm_runs(segms, device):
    """the run table (counts, n) of compressed segmentations, for masks of any size"""
    return rle.strings_to_runs([s['counts'] for s in segms], device)


def _segm_sizes(segms):
    return [s['size'] for s in segms]


IOU_DOMAINS = ('bits', 'runs', 'auto')
# iou_domain='auto': the run route when the bit words of one device_evaluate call (every dt and gt mask at one bit per
# pixel) would pass this; one 8 192 x 9 000 mask is 9.2 MB of them
BITS_BUDGET_BYTES = 1 << 30


class CocoEvalResult:
    """What COCOeval leaves behind that the metric reads: eval['precision'] / ['recall'] and stats."""

    def __init__(self, precision, recall, stats, tables=None):
        self.eval = dict(precision=precision, recall=recall)
        self.stats = stats
        self.tables = tables            # the device's evaluateImg tables (dtm, dtig [A, T, n_dt], npig [units, A], ...)


def _band_runs(runs, sizes, dilation_ratio):
    """the boundary bands of a run table whose rows lie on canvases of their own (sizes: (H, W) per row): the rows grouped
    by size, one rle.boundary_runs call per size with that size's radius, the groups put back in row order"""
    counts, n = runs
    groups = {}
    for i, s in enumerate(sizes):
        groups.setdefault((int(s[0]), int(s[1])), []).append(i)
    if not groups:
        return counts, n
    tables, ns, order = [], [], []
    for size, idx in groups.items():
        sel = torch.tensor(idx, dtype=torch.int64, device=n.device)
        c, m, _, _ = rle.boundary_runs(counts[sel].contiguous(), n[sel].contiguous(), size,
                                       rle.boundary_radius(size, dilation_ratio))
        tables.append(c)
        ns.append(m)
        order += idx
    back = torch.tensor(np.argsort(np.asarray(order, np.int64), kind='stable'), dtype=torch.int64, device=n.device)
    return rle.concat_runs(tables, rows=back).contiguous(), torch.cat(ns)[back].contiguous()


def _obb_quads(runs, sizes):
    """the oriented boxes of a run table whose rows lie on canvases of their own (sizes: (H, W) per row): the rows grouped by
    size as in _band_runs, one rle.runs_to_obb_corners call per size -> float64 [k, 4, 2] on the device, in row order (NaN
    rows for empty masks)"""
    counts, n = runs
    out = torch.full((len(sizes), 4, 2), float('nan'), dtype=torch.float64, device=n.device)
    groups = {}
    for i, s in enumerate(sizes):
        groups.setdefault((int(s[0]), int(s[1])), []).append(i)
    for size, idx in groups.items():
        sel = torch.tensor(idx, dtype=torch.int64, device=n.device)
        out[sel] = rle.runs_to_obb_corners(counts[sel].contiguous(), n[sel].contiguous(), size)
    return out


def _band_iou(units, n_iou, d_runs, g_runs, d_sizes, g_sizes, g_crowd, dilation_ratio, iou_domain):
    """the IoU blocks of the boundary bands, through the route the mask IoU took: the bit route gets its words from the band
    tables"""
    d_band, g_band = _band_runs(d_runs, d_sizes, dilation_ratio), _band_runs(g_runs, g_sizes, dilation_ratio)
    if iou_domain == 'runs':
        return ops.coco_iou_runs(units, n_iou, d_band, g_band, g_crowd)
    (db, dwo, da, dwr), (gb, gwo, ga, gwr) = rle.runs_to_bits(*d_band, d_sizes), rle.runs_to_bits(*g_band, g_sizes)
    return ops.coco_iou(units, n_iou, ops.COCO_IOU_SEGM, gt_crowd=g_crowd, dt_bits=db, gt_bits=gb, dt_woff=dwo, gt_woff=gwo,
                        dt_wrange=dwr, gt_wrange=gwr, dt_area=da, gt_area=ga)


def device_evaluate(gt, dt, iou_type, img_ids, cat_ids, iou_thrs, max_dets, device, timings=None, iou_domain='bits',
                    keep_iou=False, dilation_ratio=0.02):
    """COCOeval(gt, dt, iou_type) with params imgIds / catIds / iouThrs / maxDets -> evaluate + accumulate + summarize.

    gt: dict(images, annotations) (annotations with id, image_id, category_id, area, iscrowd, bbox, segmentation);
    dt: list of loadRes'd detections (id from 1, image_id, category_id, score, area, bbox or segmentation RLE).
    iou_domain (segm only): 'bits' expands every mask to one bit per pixel (rsp_rle_to_bits + rsp_coco_iou), 'runs' keeps
    the run tables (ops.coco_iou_runs: the same doubles, for scenes), 'auto' takes 'runs' when the bits of this call would
    pass BITS_BUDGET_BYTES.  timings['iou_domain'] tells which one ran.  keep_iou: tables['iou'] = the IoU blocks, on the
    device (tools/bench_coco_iou_runs.py compares the routes on them).
    iou_type 'boundary'  is 'segm' with the IoU of every pair replaced by min(mask IoU, Boundary IoU): the
    bands M & ~erode(M, d) of detections and ground truths are made in the run domain (one rle.boundary_runs call per image
    size, d = rle.boundary_radius(size, dilation_ratio)) and their IoU goes through the same route as the mask IoU; areas,
    crowds, matching and accumulation are segm's.
    iou_type 'obb'  is 'segm' with the IoU of every pair replaced by the IoU of the masks' minimum-area
    rectangles (rle.runs_to_obb_corners per image size, ops.obb_iou); areas (the mask areas), crowds, area ranges, matching
    and accumulation are segm's, so the two APs differ by the IoU alone.  It reads the run tables (iou_domain is not used)."""
    import time
    segm = iou_type in ('segm', 'boundary', 'obb')
    if iou_domain not in IOU_DOMAINS:
        raise ValueError(f'device_evaluate: iou_domain {iou_domain!r}: one of {IOU_DOMAINS}')
    t0 = time.perf_counter()
    img_ids = np.unique(np.asarray(img_ids))
    cat_ids = np.unique(np.asarray(cat_ids))
    thrs = np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    max_dets = list(max_dets)
    I, K, A, T, M = len(img_ids), len(cat_ids), len(AREA_RNG), len(thrs), len(max_dets)
    img_pos = {int(v): i for i, v in enumerate(img_ids.tolist())}
    cat_pos = {int(v): i for i, v in enumerate(cat_ids.tolist())}
    img_hw = {im['id']: (im.get('height'), im.get('width')) for im in gt['images']}
    # ---- units = (category, image), category-major; gts in annotation order, dts by score (stable), truncated
    gts = [g for g in gt['annotations'] if g['image_id'] in img_pos and g['category_id'] in cat_pos]
    g_unit = np.fromiter((cat_pos[g['category_id']] * I + img_pos[g['image_id']] for g in gts), dtype=np.int64,
                         count=len(gts))
    g_ord = np.argsort(g_unit, kind='mergesort')
    gts = [gts[i] for i in g_ord]
    g_unit = g_unit[g_ord]
    dts = [d for d in dt if d['image_id'] in img_pos and d['category_id'] in cat_pos]
    d_unit = np.fromiter((cat_pos[d['category_id']] * I + img_pos[d['image_id']] for d in dts), dtype=np.int64,
                         count=len(dts))
    d_score = np.fromiter((d['score'] for d in dts), dtype=np.float64, count=len(dts))
    d_ord = np.lexsort((-d_score, d_unit))                  # per unit: argsort(-score, kind='mergesort')
    d_unit = d_unit[d_ord]
    U = K * I
    nd_all = np.bincount(d_unit, minlength=U)
    first = np.concatenate([[0], np.cumsum(nd_all)[:-1]])
    rank = np.arange(len(d_unit)) - first[d_unit] if len(d_unit) else np.zeros(0, dtype=np.int64)
    keep = rank < max_dets[-1]
    d_ord, d_unit, rank = d_ord[keep], d_unit[keep], rank[keep]
    dts = [dts[i] for i in d_ord]
    d_score = d_score[d_ord]
    nd = np.bincount(d_unit, minlength=U).astype(np.int64)
    ng = np.bincount(g_unit, minlength=U).astype(np.int64)
    dt0 = np.concatenate([[0], np.cumsum(nd)[:-1]]).astype(np.int64)
    gt0 = np.concatenate([[0], np.cumsum(ng)[:-1]]).astype(np.int64)
    npair = nd * ng
    out0 = np.concatenate([[0], np.cumsum(npair)[:-1]]).astype(np.int64)
    n_iou = int(npair.sum())
    n_dt, n_gt = len(dts), len(gts)
    unit_img = np.tile(img_ids, K)
    nwords = np.array([((img_hw.get(int(i), (0, 0))[0] or 0) * (img_hw.get(int(i), (0, 0))[1] or 0) + 63) // 64
                       for i in unit_img.tolist()], dtype=np.int64)
    if segm:
        for d in dts:
            if tuple(d['segmentation']['size']) != tuple(img_hw[d['image_id']]):
                raise ValueError('segm: a detection mask does not have the size of its image')
    units = ops.coco_units(dt0, gt0, out0, nd, ng, nwords if segm else np.zeros(U, np.int64), device)

    def dev(a, dtype):
        a = np.asarray(a, dtype=dtype)
        if a.size == 0:
            a = np.zeros((1,) + a.shape[1:], dtype=dtype)
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    g_crowd = dev([int(bool(g.get('iscrowd', 0))) for g in gts], np.uint8)
    g_area = dev([g['area'] for g in gts], np.float64)
    g_id = dev([g['id'] for g in gts], np.int64)
    t1 = time.perf_counter()
    d_segm, g_segm = ([x['segmentation'] for x in dts], [x['segmentation'] for x in gts]) if segm else ([], [])
    by_mask = segm and iou_type != 'obb'                       # the IoU reads the masks themselves
    if by_mask and iou_domain == 'auto':
        words = int(rle.word_offsets(_segm_sizes(d_segm))[-1] + rle.word_offsets(_segm_sizes(g_segm))[-1])
        iou_domain = 'runs' if 8 * words > BITS_BUDGET_BYTES else 'bits'
    if by_mask and iou_domain == 'runs':
        d_runs, g_runs = _segm_runs(d_segm, device), _segm_runs(g_segm, device)
        d_pre = ops.run_prefix(*d_runs, check=False)           # rle_from_string's retry left no negative n
        info = {}
        iou = ops.coco_iou_runs(units, n_iou, d_runs, g_runs, g_crowd, dt_prefix=d_pre, info=info)
        d_area = d_pre[1].to(torch.float64) if n_dt else dev([0.0], np.float64)
        if timings is not None:
            timings.update(pairs=info['pairs'], survivors=info['survivors'])
    elif by_mask:
        db, dwo, da, dwr = rle.runs_to_bits(*_segm_runs(d_segm, device), _segm_sizes(d_segm))
        gb, gwo, ga, gwr = rle.runs_to_bits(*_segm_runs(g_segm, device), _segm_sizes(g_segm))
        iou = ops.coco_iou(units, n_iou, ops.COCO_IOU_SEGM, gt_crowd=g_crowd, dt_bits=db, gt_bits=gb, dt_woff=dwo,
                           gt_woff=gwo, dt_wrange=dwr, gt_wrange=gwr, dt_area=da, gt_area=ga)
        d_area = da.to(torch.float64) if n_dt else dev([0.0], np.float64)
    elif segm:                                                 # 'obb': the rectangles of the run tables, segm's areas
        iou_domain = 'runs'
        d_runs, g_runs = _segm_runs(d_segm, device), _segm_runs(g_segm, device)
        d_area = ops.run_prefix(*d_runs, check=False)[1].to(torch.float64) if n_dt else dev([0.0], np.float64)
        iou = ops.obb_iou(units, n_iou, _obb_quads(d_runs, _segm_sizes(d_segm)), _obb_quads(g_runs, _segm_sizes(g_segm)),
                          g_crowd[:n_gt])
    else:
        d_box = dev(np.asarray([d['bbox'] for d in dts], np.float64).reshape(-1, 4), np.float64)
        g_box = dev(np.asarray([g['bbox'] for g in gts], np.float64).reshape(-1, 4), np.float64)
        iou = ops.coco_iou(units, n_iou, ops.COCO_IOU_BBOX, gt_crowd=g_crowd, dt_box=d_box, gt_box=g_box)
        d_area = dev([d['area'] for d in dts], np.float64)
    if iou_type == 'boundary' and n_iou:
        tb = time.perf_counter()
        if iou_domain != 'runs':
            d_runs, g_runs = _segm_runs(d_segm, device), _segm_runs(g_segm, device)
        band = _band_iou(units, n_iou, d_runs, g_runs, _segm_sizes(d_segm), _segm_sizes(g_segm), g_crowd, dilation_ratio,
                         iou_domain)
        iou = torch.minimum(iou[:n_iou], band)
        if timings is not None:
            timings['band'] = timings.get('band', 0.0) + (time.perf_counter() - tb)     # inside 'device'
    if n_iou == 0:
        iou = torch.zeros((1,), dtype=torch.float64, device=device)
    dtm, dtig, npig = ops.coco_match(units, iou, g_area, g_crowd, g_id, d_area, dev(AREA_RNG, np.float64),
                                     dev(thrs, np.float64), n_dt)
    dtm, dtig, npig = dtm.cpu().numpy(), dtig.cpu().numpy().astype(bool), npig.cpu().numpy()
    t2 = time.perf_counter()
    precision, recall = accumulate(dtm, dtig, npig, d_score, d_unit, rank, nd, ng, K, I, thrs, max_dets)
    stats = summarize(precision, recall, thrs, max_dets)
    t3 = time.perf_counter()
    if timings is not None:
        timings['host_prepare'] = timings.get('host_prepare', 0.0) + (t1 - t0)
        timings['device'] = timings.get('device', 0.0) + (t2 - t1)
        timings['host_accumulate'] = timings.get('host_accumulate', 0.0) + (t3 - t2)
        if segm:
            timings['iou_domain'] = iou_domain
    tables = dict(dtm=dtm, dtig=dtig, npig=npig, dt_ids=np.array([d['id'] for d in dts], dtype=np.int64), dt0=dt0,
                  nd=nd, ng=ng, n_img=I, n_cat=K)
    if keep_iou:
        tables['iou'] = iou[:n_iou]
    return CocoEvalResult(precision, recall, stats, tables)


def accumulate(dtm, dtig, npig, d_score, d_unit, rank, nd, ng, K, I, thrs, max_dets):
    """COCOeval.accumulate, vectorised over thresholds.  dtm / dtig [A, T, n_dt] in unit order (category-major, images
    sorted, dts by score within a unit); npig [K * I, A]."""
    T, R, A, M = len(thrs), len(REC_THRS), len(AREA_RNG), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    # a unit that has neither gt nor dt is evaluateImg's None: it contributes nothing either way
    d_cat = d_unit // I if len(d_unit) else d_unit
    cat_has = (nd + ng).reshape(K, I).sum(1) > 0
    for k in range(K):
        if not cat_has[k]:
            continue
        sel_k = np.nonzero(d_cat == k)[0]
        for m, max_det in enumerate(max_dets):
            sel = sel_k[rank[sel_k] < max_det]
            inds = np.argsort(-d_score[sel], kind='mergesort')
            idx = sel[inds]
            for a in range(A):
                n_pos = int(npig[k * I:(k + 1) * I, a].sum())
                if n_pos == 0:
                    continue
                m_ = dtm[a][:, idx] != 0
                ig = dtig[a][:, idx]
                tps = np.logical_and(m_, np.logical_not(ig))
                fps = np.logical_and(np.logical_not(m_), np.logical_not(ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                nd_ = tp_sum.shape[1]
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    rc = tp / n_pos
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd_ else 0
                    q = np.zeros((R,))
                    if nd_:
                        pr = np.maximum.accumulate(pr[::-1])[::-1]
                        pi = np.searchsorted(rc, REC_THRS, side='left')
                        ok = pi < nd_
                        q[ok] = pr[pi[ok]]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize(precision, recall, thrs, max_dets):
    """COCOeval.summarize / _summarizeDets with mmdet's maxDets = proposal_nums."""
    thrs = np.asarray(thrs)

    def _s(ap, iou_thr=None, area='all', md=100):
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, m in enumerate(max_dets) if m == md]
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == thrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if iou_thr is not None:
                s = s[np.where(iou_thr == thrs)[0]]
            s = s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    md = max_dets
    stats = np.zeros((12,))
    stats[0] = _s(1, md=md[2])
    stats[1] = _s(1, iou_thr=.5, md=md[2])
    stats[2] = _s(1, iou_thr=.75, md=md[2])
    stats[3] = _s(1, area='small', md=md[2])
    stats[4] = _s(1, area='medium', md=md[2])
    stats[5] = _s(1, area='large', md=md[2])
    stats[6] = _s(0, md=md[0])
    stats[7] = _s(0, md=md[1])
    stats[8] = _s(0, md=md[2])
    stats[9] = _s(0, area='small', md=md[2])
    stats[10] = _s(0, area='medium', md=md[2])
    stats[11] = _s(0, area='large', md=md[2])
    return stats


def load_res(gt, results, iou_type):
    """COCO.loadRes for a list of result dicts: ids from 1, iscrowd 0, area = w * h (bbox) or the mask area (segm,
    computed on the device with the IoU's bits; filled in by device_evaluate)."""
    img_set = {im['id'] for im in gt['images']}
    out = []
    for i, r in enumerate(results):
        if r['image_id'] not in img_set:
            raise AssertionError('Results do not correspond to current coco set')
        d = dict(r)
        d['id'] = i + 1
        d['iscrowd'] = 0
        if iou_type == 'bbox':
            bb = d['bbox']
            d['area'] = bb[2] * bb[3]
        out.append(d)
    return out


GT_RASTERS = ('host', 'device')


@METRICS.register_module()
class CocoMetric:
    """mmdet CocoMetric (bbox / segm) -- `process`, `compute_metrics`, `evaluate(size)`, `dataset_meta`.  metric 'boundary'
    adds Boundary AP (LVIS iouType='boundary', boundary-iou-api): segm with min(mask IoU, Boundary IoU) per pair, band width
    dilation_ratio * the image diagonal; keys boundary_mAP, boundary_mAP_50, ....  metric 'obb' adds
    oriented-box AP: segm with the IoU of the masks' minimum-area rectangles per pair; keys obb_mAP, obb_mAP_50, ... (DESIGN
    §14.17)."""
    default_prefix = 'coco'

    def __init__(self, ann_file=None, metric='bbox', classwise=False, proposal_nums=(100, 300, 1000), iou_thrs=None,
                 metric_items=None, format_only=False, outfile_prefix=None, file_client_args=None, backend_args=None,
                 collect_device='cpu', prefix=None, sort_categories=False, use_mp_eval=False, device=None, gt_raster='host',
                 iou_domain='bits', dilation_ratio=0.02):
        self.metrics = metric if isinstance(metric, list) else [metric]
        for m in self.metrics:
            if m in ('proposal', 'proposal_fast'):
                raise NotImplementedError(f'CocoMetric: metric {m!r} is not implemented (bbox and segm are)')
            if m not in ('bbox', 'segm', 'boundary', 'obb'):
                raise KeyError(f"metric should be one of 'bbox', 'segm', 'proposal', 'proposal_fast', but got {m}.")
        if file_client_args is not None:
            raise RuntimeError('The `file_client_args` is deprecated, please use `backend_args` instead')
        if backend_args is not None:
            raise NotImplementedError('backend_args: only local files are supported (backend_args=None)')
        self.classwise = classwise
        self.use_mp_eval = use_mp_eval                      # same numbers: accepted and ignored
        self.proposal_nums = list(proposal_nums)
        if iou_thrs is None:
            iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.iou_thrs = iou_thrs
        self.metric_items = metric_items
        self.format_only = format_only
        if format_only:
            assert outfile_prefix is not None, 'outfile_prefix must be not None when format_only is True'
        self.outfile_prefix = outfile_prefix
        self.prefix = prefix or self.default_prefix
        self.device = device
        if gt_raster not in GT_RASTERS:
            raise ValueError(f'CocoMetric: gt_raster {gt_raster!r}: one of {GT_RASTERS}')
        self.gt_raster = gt_raster                          # who rasterises ground-truth polygons
        if iou_domain not in IOU_DOMAINS:
            raise ValueError(f'CocoMetric: iou_domain {iou_domain!r}: one of {IOU_DOMAINS}')
        self.iou_domain = iou_domain                        # how the segm IoU reads the masks
        if isinstance(dilation_ratio, bool) or not isinstance(dilation_ratio, (int, float)) \
                or not (dilation_ratio > 0 and np.isfinite(dilation_ratio)):
            raise ValueError(f'CocoMetric: dilation_ratio must be a positive finite number, got {dilation_ratio!r}')
        self.dilation_ratio = float(dilation_ratio)         # the band width of metric 'boundary' 
        self._coco_api = None
        if ann_file is not None:
            with open(ann_file) as f:
                self._coco_api = json.load(f)
            self._coco_api.setdefault('annotations', [])
            if sort_categories:
                self._coco_api['categories'] = sorted(self._coco_api['categories'], key=lambda c: c['id'])
        self.cat_ids = None
        self.img_ids = None
        self._dataset_meta = None
        self.results = []
        self.eval_results = {}                              # iou type -> CocoEvalResult (unrounded stats)
        self.timings = {}

    @property
    def dataset_meta(self):
        return self._dataset_meta

    @dataset_meta.setter
    def dataset_meta(self, meta):
        self._dataset_meta = meta

    # ------------------------------------------------------------------ mmengine BaseMetric surface
    def process(self, data_batch, data_samples):
        """store (gt, result) per sample as coco_metric.py:346-391; masks may be a device bool tensor (encoded with the
        device RLE codec) or a list of COCO RLE dicts (what `dist.gather_results` delivers)."""
        from .rle import encode_mask_results
        for s in data_samples:
            pred = _get(s, 'pred_instances')
            result = dict(img_id=_get(s, 'img_id'), bboxes=_np(_get(pred, 'bboxes')).astype(np.float32).reshape(-1, 4),
                          scores=_np(_get(pred, 'scores')).astype(np.float32).reshape(-1),
                          labels=_np(_get(pred, 'labels')).astype(np.int64).reshape(-1))
            masks = _get(pred, 'masks')
            if masks is not None:
                result['masks'] = encode_mask_results(masks) if isinstance(masks, torch.Tensor) else list(masks)
            ms = _get(pred, 'mask_scores')
            if ms is not None:
                result['mask_scores'] = _np(ms).astype(np.float32).reshape(-1)
            ori = _get(s, 'ori_shape')
            gt = dict(width=int(ori[1]), height=int(ori[0]), img_id=_get(s, 'img_id'))
            if self._coco_api is None:
                gi = _get(s, 'gt_instances')
                g_masks = _get(gi, 'masks')
                if isinstance(g_masks, torch.Tensor):
                    g_masks = encode_mask_results(g_masks)
                gt['anns'] = [dict(bbox_label=int(lb), bbox=bb, mask=mk) for bb, mk, lb in
                              zip(_np(_get(gi, 'bboxes')).astype(np.float32).reshape(-1, 4), g_masks,
                                  _np(_get(gi, 'labels')).reshape(-1))]
            self.results.append((gt, result))

    def evaluate(self, size):
        """mmengine BaseMetric.evaluate: the results of `size` samples -> metrics with the `coco/` prefix."""
        results = self.results[:size]
        metrics = self.compute_metrics(results)
        self.results = []
        return {f'{self.prefix}/{k}': v for k, v in metrics.items()}

    # ------------------------------------------------------------------ conversions
    def gt_to_coco_json(self, gt_dicts):
        """coco_metric.py:274-344 (in memory): ids from 1, categories 0..C-1, iscrowd = ignore_flag (never set), area =
        float32 w * h of the float32 xyxy box."""
        categories = [dict(id=i, name=n) for i, n in enumerate(self.dataset_meta['classes'])]
        images, annotations = [], []
        for idx, g in enumerate(gt_dicts):
            img_id = g.get('img_id', idx)
            images.append(dict(id=img_id, width=g['width'], height=g['height'], file_name=''))
            for ann in g['anns']:
                bbox = ann['bbox']
                coco_bbox = [bbox[0], bbox[1], bbox[2] - bbox[0], bbox[3] - bbox[1]]       # float32 arithmetic
                a = dict(id=len(annotations) + 1, image_id=img_id, bbox=[float(v) for v in coco_bbox],
                         iscrowd=ann.get('ignore_flag', 0), category_id=int(ann['bbox_label']),
                         area=float(coco_bbox[2] * coco_bbox[3]))
                mask = ann.get('mask', None)
                if mask:
                    a['segmentation'] = mask
                annotations.append(a)
        return dict(images=images, categories=categories, annotations=annotations)

    @staticmethod
    def xyxy2xywh(bbox):
        b = bbox.tolist()
        return [b[0], b[1], b[2] - b[0], b[3] - b[1]]

    def results2json(self, results, outfile_prefix=None):
        """coco_metric.py:209-272: bbox and segm result lists (written to <prefix>.bbox.json / .segm.json when a prefix
        is given)."""
        bbox_json, segm_json = [], []
        for r in results:
            image_id = r.get('img_id')
            labels, bboxes, scores = r['labels'], r['bboxes'], r['scores']
            for i in range(len(labels)):
                bbox_json.append(dict(image_id=image_id, bbox=self.xyxy2xywh(bboxes[i]), score=float(scores[i]),
                                      category_id=self.cat_ids[labels[i]]))
            if 'masks' not in r:
                continue
            mask_scores = r.get('mask_scores', scores)
            for i in range(len(labels)):
                m = r['masks'][i]
                c = m['counts']
                segm_json.append(dict(image_id=image_id, bbox=self.xyxy2xywh(bboxes[i]), score=float(mask_scores[i]),
                                      category_id=self.cat_ids[labels[i]],
                                      segmentation=dict(size=list(m['size']),
                                                        counts=c.decode() if isinstance(c, bytes) else c)))
        files = {}
        if outfile_prefix is not None:
            os.makedirs(os.path.dirname(os.path.abspath(outfile_prefix)), exist_ok=True)
            files['bbox'] = f'{outfile_prefix}.bbox.json'
            with open(files['bbox'], 'w') as f:
                json.dump(bbox_json, f)
            if segm_json:
                files['segm'] = f'{outfile_prefix}.segm.json'
                with open(files['segm'], 'w') as f:
                    json.dump(segm_json, f)
        return dict(bbox=bbox_json, segm=segm_json) if segm_json else dict(bbox=bbox_json), files

    # ------------------------------------------------------------------ metrics
    def _gt_with_rles(self, coco, device=None):
        """annToRLE of every gt segmentation (polygons rasterised + merged, uncompressed RLE compressed).  gt_raster='host'
        walks every polygon in Python (datasets.ann_to_rle); 'device' rasterises all of them in one call on `device`
        (datasets.anns_to_rle, csrc/poly_raster.hip) and gives the same strings."""
        hw = {im['id']: (im['height'], im['width']) for im in coco['images']}
        anns = []
        if self.gt_raster == 'device':
            anns = [dict(a) for a in coco['annotations']]
            todo = [a for a in anns if a['image_id'] in hw and 'segmentation' in a and a['segmentation'] is not None]
            rles = anns_to_rle([a['segmentation'] for a in todo], [hw[a['image_id']] for a in todo],
                               device if device is not None else (self.device or 'cuda:0'))
            for a, r in zip(todo, rles):
                a['segmentation'] = r
            return dict(coco, annotations=anns)
        for a in coco['annotations']:
            a = dict(a)
            if a['image_id'] in hw and 'segmentation' in a and a['segmentation'] is not None:
                h, w = hw[a['image_id']]
                a['segmentation'] = ann_to_rle(a['segmentation'], h, w)
            anns.append(a)
        return dict(coco, annotations=anns)

    def compute_metrics(self, results):
        import time
        gts, preds = zip(*results) if results else ((), ())
        coco = self._coco_api if self._coco_api is not None else self.gt_to_coco_json(gts)
        self.coco_gt = coco                                 # the ground truth the numbers were computed against
        classes = list(self.dataset_meta['classes'])
        if self.cat_ids is None:
            self.cat_ids = [c['id'] for c in coco['categories'] if c['name'] in classes]
        if self.img_ids is None:
            self.img_ids = list(dict.fromkeys(im['id'] for im in coco['images']))
        result_lists, _ = self.results2json(preds, self.outfile_prefix)
        eval_results = OrderedDict()
        if self.format_only:
            return eval_results
        device = torch.device(self.device) if self.device is not None else torch.device('cuda', torch.cuda.current_device())
        names = {n: i for i, n in enumerate(STAT_NAMES)}
        gt_rle = None
        for metric in self.metrics:
            masks = metric in ('segm', 'boundary', 'obb')   # 'boundary' and 'obb' read the segm results and ground-truth RLEs
            preds_m = result_lists.get('segm' if masks else metric)
            if preds_m is None:
                raise KeyError(f'{metric} is not in results')
            if len(preds_m) == 0:                       # pycocotools loadRes indexes anns[0]: mmdet logs and stops
                break
            t0 = time.perf_counter()
            if masks:
                preds_m = [{k: v for k, v in x.items() if k != 'bbox'} for x in preds_m]
                if gt_rle is None:
                    gt_rle = self._gt_with_rles(coco, device)
                gt_m = gt_rle
            else:
                gt_m = coco
            dts = load_res(gt_m, preds_m, metric)
            for d in dts:
                if masks:
                    c = d['segmentation']['counts']
                    d['segmentation'] = dict(size=d['segmentation']['size'], counts=c.encode() if isinstance(c, str) else c)
            tm = {}
            ev = device_evaluate(gt_m, dts, metric, self.img_ids, self.cat_ids, self.iou_thrs, self.proposal_nums,
                                 device, timings=tm, iou_domain=self.iou_domain, dilation_ratio=self.dilation_ratio)
            tm['total'] = time.perf_counter() - t0
            self.timings[metric] = tm
            self.eval_results[metric] = ev
            if self.metric_items is not None:
                for item in self.metric_items:
                    if item not in names:
                        raise KeyError(f'metric item "{item}" is not supported')
            if self.classwise:
                precisions = ev.eval['precision']
                assert len(self.cat_ids) == precisions.shape[2]
                cname = {c['id']: c['name'] for c in coco['categories']}
                for idx, cat_id in enumerate(self.cat_ids):
                    p = precisions[:, :, idx, 0, -1]
                    p = p[p > -1]
                    ap = np.mean(p) if p.size else float('nan')
                    eval_results[f'{cname[cat_id]}_precision'] = round(ap, 3)
            items = self.metric_items if self.metric_items is not None else list(STAT_NAMES[:6])
            for item in items:
                val = ev.stats[names[item]]
                eval_results[f'{metric}_{item}'] = float(f'{round(val, 3)}')
        return eval_results

    def summary_table(self):
        """mmdet's printed summary: pycocotools' 12 lines per iou type."""
        lines = []
        spec = [(1, None, 'all', 2), (1, .5, 'all', 2), (1, .75, 'all', 2), (1, None, 'small', 2), (1, None, 'medium', 2),
                (1, None, 'large', 2), (0, None, 'all', 0), (0, None, 'all', 1), (0, None, 'all', 2),
                (0, None, 'small', 2), (0, None, 'medium', 2), (0, None, 'large', 2)]
        for metric, ev in self.eval_results.items():
            lines.append(f'Evaluate annotation type *{metric}*')
            for v, (ap, thr, area, mi) in zip(ev.stats, spec):
                title = 'Average Precision' if ap == 1 else 'Average Recall'
                typ = '(AP)' if ap == 1 else '(AR)'
                iou = '0.50:0.95' if thr is None else f'{thr:0.2f}'
                lines.append(f' {title:<18} {typ} @[ IoU={iou:<9} | area={area:>6s} | '
                             f'maxDets={self.proposal_nums[mi]:>3d} ] = {v:0.3f}')
        return '\n'.join(lines)


# ------------------------------------------------------------------------------------------------------------ panoptic
PQ_KEYS = ('PQ', 'SQ', 'RQ', 'PQ_th', 'SQ_th', 'RQ_th', 'PQ_st', 'SQ_st', 'RQ_st')


def pq_average(stat, categories, isthing=None):
    """panopticapi's PQStat.pq_average on stat = {category id: (tp, fp, fn, iou_sum)}, categories = {id: dict(isthing=...)}:
    (dict(pq, sq, rq, n), per class).  A category with tp + fp + fn == 0 is not counted.  A group without a counted
    category gives pq = sq = rq = 0.0, n = 0 (panopticapi divides by n; every RSPrompter dataset has no stuff class, so the
    Stuff group would fail there every time: DESIGN §16.1)."""
    pq = sq = rq = 0.0
    n = 0
    per_class = {}
    for c, info in categories.items():
        if isthing is not None and isthing != (info['isthing'] == 1):
            continue
        tp, fp, fn, iou = stat[c]
        if tp + fp + fn == 0:
            per_class[c] = dict(pq=0.0, sq=0.0, rq=0.0)
            continue
        n += 1
        pq_c = iou / (tp + 0.5 * fp + 0.5 * fn)
        sq_c = iou / tp if tp != 0 else 0
        rq_c = tp / (tp + 0.5 * fp + 0.5 * fn)
        per_class[c] = dict(pq=pq_c, sq=sq_c, rq=rq_c)
        pq, sq, rq = pq + pq_c, sq + sq_c, rq + rq_c
    if n == 0:
        return dict(pq=0.0, sq=0.0, rq=0.0, n=0), per_class
    return dict(pq=pq / n, sq=sq / n, rq=rq / n, n=n), per_class


def pq_results(stat, categories):
    """{'All' | 'Things' | 'Stuff': dict(pq, sq, rq, n), 'classwise': per class of All} (coco_panoptic_metric.py:533-540)"""
    out = {}
    for name, isthing in (('All', None), ('Things', True), ('Stuff', False)):
        out[name], per_class = pq_average(stat, categories, isthing)
        if name == 'All':
            out['classwise'] = per_class
    return out


def parse_pq_results(res):
    """coco_panoptic_metric.py:556-575"""
    return {k.upper() + s: 100 * res[g][k] for g, s in (('All', ''), ('Things', '_th'), ('Stuff', '_st')) for k in ('pq', 'sq', 'rq')}


def _text_table(rows):
    width = [max(len(str(r[i])) for r in rows) for i in range(len(rows[0]))]
    line = '+' + '+'.join('-' * (w + 2) for w in width) + '+'
    body = ['| ' + ' | '.join(str(v).ljust(w) for v, w in zip(r, width)) + ' |' for r in rows]
    return '\n'.join([line, body[0], line] + body[1:] + [line])


def panoptic_table(res, classwise=None):
    """print_panoptic_table (coco_panoptic_metric.py:578-618) as plain text"""
    rows = [['', 'PQ', 'SQ', 'RQ', 'categories']]
    for name in ('All', 'Things', 'Stuff'):
        rows.append([name] + [f'{res[name][k] * 100:0.3f}' for k in ('pq', 'sq', 'rq')] + [res[name]['n']])
    text = 'Panoptic Evaluation Results:\n' + _text_table(rows)
    if classwise is not None:
        rows = [['category', 'PQ', 'SQ', 'RQ']] + [[name] + [f'{m[k] * 100:0.3f}' for k in ('pq', 'sq', 'rq')]
                                                  for name, m in classwise.items()]
        text += '\nClasswise Panoptic Evaluation Results:\n' + _text_table(rows)
    return text


def pq_stat_from_packed(packed, cat_ids, names=None):
    """the one host read of ops.pq_reduce -> {category id: (tp, fp, fn, iou_sum)}; a row with a status raises, naming it"""
    buf = packed.cpu().numpy()
    n = len(cat_ids)
    for k, st in enumerate(buf[4 * n:].tolist()):
        if st:
            who = names[k] if names is not None else k
            raise RuntimeError(f'panoptic quality: image {who!r} was refused: {ops.pq_status_text(st)} (status {st})')
    iou = buf[3 * n:4 * n].view(np.float64)
    return {c: (int(buf[i]), int(buf[n + i]), int(buf[2 * n + i]), float(iou[i])) for i, c in enumerate(cat_ids)}


def _segments_as_json(segments_info, categories):
    """segments_info in the JSON's form: the dataset's form (id, category, is_thing) converted as
    coco_panoptic_metric.py:355-372 does -- iscrowd = a thing class whose segment is not a thing; the area is counted"""
    out = []
    for s in segments_info:
        if 'category_id' in s:
            out.append(dict(id=int(s['id']), category_id=s['category_id'], iscrowd=int(s.get('iscrowd', 0)), area=s.get('area')))
        else:
            label = s['category']
            crowd = 1 if categories[label]['isthing'] and not s['is_thing'] else 0
            out.append(dict(id=int(s['id']), category_id=label, iscrowd=crowd, area=None))
    return out


@METRICS.register_module()
class CocoPanopticMetric:
    """mmdet CocoPanopticMetric (mmdet/evaluation/metrics/coco_panoptic_metric.py): PQ / SQ / RQ of `pred_panoptic_seg`
    with the per-image work -- void mapping, np.unique, the confusion of the two maps, matching -- on the device
    (ops.pq_image, csrc/panoptic_quality.hip): the predicted map is never copied to the host or written to a
    file to be scored.  `process` keeps one small row per image; `compute_metrics` reduces them on the device in processing
    order, reads the host once and averages as PQStat.pq_average.  Needs neither panopticapi nor terminaltables.

    The ground truth of a sample comes from, in this order: an in-memory id map `gt_panoptic` with `segments_info`; with
    `ann_file` the JSON's segments_info (areas as listed) and the PNG `seg_prefix/<name>.png`; else the sample's
    `segments_info` with `seg_map_path` (or `seg_prefix/<name>.png`), areas counted.  `outfile_prefix` additionally writes
    `<prefix>.panoptic/<name>.png` and `<prefix>.panoptic.json` (`format_only`: only that); PQ itself always comes from the
    maps.  `nproc` is accepted and ignored: the sums are the in-order ones."""
    default_prefix = 'coco_panoptic'

    def __init__(self, ann_file=None, seg_prefix=None, classwise=False, format_only=False, outfile_prefix=None, nproc=32,
                 file_client_args=None, backend_args=None, collect_device='cpu', prefix=None, device=None):
        if file_client_args is not None:
            raise RuntimeError('The `file_client_args` is deprecated, please use `backend_args` instead')
        if backend_args is not None:
            raise NotImplementedError('backend_args: only local files are supported (backend_args=None)')
        self.classwise = classwise
        self.format_only = format_only
        if format_only:
            assert outfile_prefix is not None, 'outfile_prefix must be not None when format_only is True'
        self.outfile_prefix = outfile_prefix
        self.seg_out_dir = None if outfile_prefix is None else f'{outfile_prefix}.panoptic'
        self.nproc = nproc
        self.seg_prefix = seg_prefix
        self.collect_device = collect_device
        self.prefix = prefix or self.default_prefix
        self.device = device
        self._coco_api = None
        self.categories = None
        if ann_file:
            with open(ann_file) as f:
                self._coco_api = json.load(f)
            self.categories = {c['id']: c for c in self._coco_api['categories']}
            self._img_to_segments = {a['image_id']: a['segments_info'] for a in self._coco_api.get('annotations', [])}
        self._dataset_meta = None
        self.results = []
        self.pq_results = None
        self.table = None

    @property
    def dataset_meta(self):
        return self._dataset_meta

    @dataset_meta.setter
    def dataset_meta(self, meta):
        self._dataset_meta = meta

    def _categories(self):
        """(categories, label2cat) as coco_panoptic_metric.py:316-327: without an ann_file the labels are the ids; with
        one, label i is the i-th JSON category whose name is a class (get_cat_ids keeps the JSON's order)"""
        classes = list(self.dataset_meta['classes'])
        if self._coco_api is None:
            things = set(self.dataset_meta.get('thing_classes', classes))
            return {i: dict(id=i, name=n, isthing=1 if n in things else 0) for i, n in enumerate(classes)}, None
        cat_ids = [c['id'] for c in self._coco_api['categories'] if c['name'] in classes]
        return self.categories, {i: c for i, c in enumerate(cat_ids)}

    @staticmethod
    def _read_png(path, device):
        from PIL import Image
        with Image.open(path) as im:
            return torch.from_numpy(np.array(im.convert('RGB'), dtype=np.uint8)).to(device)

    def process(self, data_batch, data_samples):
        device = torch.device(self.device) if self.device is not None else torch.device('cuda', torch.cuda.current_device())
        ops.require_device(device)                          # the kernels have no CPU form: refused before a map is moved
        categories, label2cat = self._categories()
        num_classes = len(self.dataset_meta['classes'])
        for s in data_samples:
            pred = _get(s, 'pred_panoptic_seg')
            sem = torch.as_tensor(_get(pred, 'sem_seg'))
            sem = (sem[0] if sem.dim() == 3 else sem).to(device=device, dtype=torch.int32).contiguous()
            ignore_index = _get(pred, 'ignore_index', num_classes)
            img_id = _get(s, 'img_id')
            name = os.path.basename(_get(s, 'img_path') or f'{img_id}.png').replace('jpg', 'png')
            gt_map = _get(s, 'gt_panoptic')
            if gt_map is not None:
                gt = torch.as_tensor(gt_map).to(device)
                segments = _segments_as_json(_get(s, 'segments_info'), categories)
            elif self._coco_api is not None:
                gt = self._read_png(os.path.join(self.seg_prefix, name), device)
                segments = self._img_to_segments[img_id]
            else:
                path = _get(s, 'seg_map_path') or os.path.join(self.seg_prefix, name)
                gt = self._read_png(path, device)
                segments = _segments_as_json(_get(s, 'segments_info'), categories)
            try:
                row = ops.pq_image(sem, gt, segments, categories, num_classes, ignore_index=ignore_index, label2cat=label2cat)
            except ValueError as e:
                raise ValueError(f'CocoPanopticMetric: image {name!r}: {e}') from e
            kept = dict(name=name, img_id=img_id, row={k: row[k] for k in ('tp', 'fp', 'fn', 'iou', 'status')})
            if self.outfile_prefix is not None:
                kept['annotation'] = self._write_prediction(sem, row, name, img_id, categories, num_classes, ignore_index)
            self.results.append(kept)

    def _write_prediction(self, sem, row, name, img_id, categories, num_classes, ignore_index):
        """_parse_predictions' file (coco_panoptic_metric.py:295-305) and result2json's entry (:231-242); this path reads
        the segment list of the image from the device, and with it the status: a refused image raises here, before a file
        with an empty segment list is written (format_only never reaches the check of compute_metrics)"""
        from .apis import write_panoptic_png
        status, n = torch.cat([row['status'], row['n_pred']]).cpu().tolist()
        if status:
            raise RuntimeError(f'panoptic quality: image {name!r} was refused: {ops.pq_status_text(status)} (status {status})')
        os.makedirs(self.seg_out_dir, exist_ok=True)
        write_panoptic_png(sem, os.path.join(self.seg_out_dir, name), void=(num_classes, ignore_index))
        cat_ids = list(categories)
        ids, cats, areas = (row[k][:n].cpu().tolist() for k in ('pred_ids', 'pred_cat', 'pred_area'))
        info = [dict(id=i, category_id=cat_ids[c], area=a, isthing=categories[cat_ids[c]]['isthing'])
                for i, c, a in zip(ids, cats, areas) if c >= 0]
        return dict(image_id=img_id, segments_info=info, file_name=name)

    def evaluate(self, size):
        results = self.results[:size]
        metrics = self.compute_metrics(results)
        self.results = []
        return {f'{self.prefix}/{k}': v for k, v in metrics.items()}

    def compute_metrics(self, results):
        import logging
        logger = logging.getLogger('rsprompter_amd')
        if self.outfile_prefix is not None:
            os.makedirs(os.path.dirname(os.path.abspath(self.outfile_prefix)), exist_ok=True)
            with open(f'{self.outfile_prefix}.panoptic.json', 'w') as f:
                json.dump(dict(annotations=[r['annotation'] for r in results]), f)
            if self.format_only:
                logger.info(f'results are saved in {os.path.dirname(self.outfile_prefix)}')
                return dict()
        categories, _ = self._categories()
        self.categories = categories
        cat_ids = list(categories)
        if results:
            red = ops.pq_reduce([r['row'] for r in results])
            stat = pq_stat_from_packed(red['packed'], cat_ids, [r['name'] for r in results])
        else:
            stat = {c: (0, 0, 0, 0.0) for c in cat_ids}
        self.pq_stat = stat
        res = pq_results(stat, categories)
        classwise = None
        if self.classwise:
            classwise = {k: v for k, v in zip(self.dataset_meta['classes'], res['classwise'].values())}
        self.pq_results, self.classwise_results = res, classwise
        self.table = panoptic_table(res, classwise)
        logger.info(self.table)
        return parse_pq_results(res)
