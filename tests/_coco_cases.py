"""Test bodies of the COCO evaluation (csrc/cocoeval.hip + rsprompter_amd/evaluation.py), shared by the emulator tier
(tests/test_coco_eval_cpu.py, CPU tensors under tests/wave_emu) and the device tier (tests/test_gpu_coco_eval.py).
Everything is compared EXACTLY (==) with the cocoapi restatement tests/_cocoeval_ref.py."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _cocoeval_ref as ref  # noqa: E402

FIXTURE = os.path.join(HERE, 'golden', 'coco_nwpu')
FIXTURE_JSON = os.path.join(FIXTURE, 'NWPU_instances_val_subset.json')
NWPU_CLASSES = ('airplane', 'ship', 'storage_tank', 'baseball_diamond', 'tennis_court', 'basketball_court',
                'ground_track_field', 'harbor', 'bridge', 'vehicle')


def random_mask(rng, h, w, kind='blob'):
    m = np.zeros((h, w), dtype=np.uint8)
    if kind == 'empty':
        return m
    if kind == 'full':
        return m + 1
    if kind == 'pixel':
        m[rng.integers(h), rng.integers(w)] = 1
        return m
    if kind == 'noise':
        return (rng.random((h, w)) < 0.3).astype(np.uint8)
    cy, cx = rng.integers(0, h), rng.integers(0, w)
    ry, rx = rng.integers(1, max(2, h // 4)), rng.integers(1, max(2, w // 4))
    yy, xx = np.ogrid[:h, :w]
    m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = 1
    return m


def rle_dict(mask):
    h, w = mask.shape
    return dict(size=[h, w], counts=ref.rle_to_string(ref.rle_encode(mask)))


# ----------------------------------------------------------------------------- string codec
def check_string_roundtrip(ops, dev, masks, cap=None):
    """device encoder (rsp_mask_rle + rsp_rle_to_string) -> device decoder (rsp_rle_from_string) -> device encoder:
    identical bytes; decoded counts == the restatement's; areas of rsp_rle_to_bits == rleArea"""
    from rsprompter_amd import rle
    t = torch.from_numpy(np.stack(masks)).to(dev).bool()
    flat, offs = rle.encode_rle_strings(t)
    k = len(masks)
    o = offs.tolist()
    strings = [flat[o[i]:o[i + 1]].numpy().tobytes() for i in range(k)]
    want = [ref.rle_encode(m) for m in masks]
    for s, c in zip(strings, want):
        assert ref.rle_fr_string(s) == c
    counts, n = ops.rle_from_string(flat.to(dev), offs.to(dev), **({} if cap is None else dict(cap=cap)))
    nh = n.cpu().tolist()
    ch = counts.cpu()
    for i in range(k):
        assert nh[i] == len(want[i])
        assert ch[i, :nh[i]].to(torch.int64).tolist() == [int(v) for v in want[i]]
    lens, offs2, flat2 = ops.rle_to_string(counts, n, k, int(o[-1]) + 16)
    o2 = offs2.cpu().tolist()
    assert o2 == o
    assert flat2.cpu()[:o[-1]].numpy().tobytes() == flat.numpy().tobytes()
    h, w = masks[0].shape
    nw = (h * w + 63) // 64
    woff = torch.arange(k + 1, dtype=torch.int64, device=dev) * nw
    bits, area, wrange = ops.rle_to_bits(counts, n, woff)
    assert area.cpu().tolist() == [ref.rle_area(c) for c in want]
    b = bits.cpu().numpy().view(np.uint64).reshape(k, nw)
    for i in range(k):
        col = masks[i].T.reshape(-1).astype(np.uint64)                 # column-major stream
        packed = np.zeros(nw * 64, dtype=np.uint64)
        packed[:h * w] = col
        words = (packed.reshape(nw, 64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
        assert np.array_equal(b[i], words)
        lo, hi = wrange[i].tolist()
        nz = np.nonzero(words)[0]
        assert (lo, hi) == ((int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0))
    return strings


# ----------------------------------------------------------------------------- IoU
def check_iou(ops, dev, rng, n_img, nd, ng, h, w, crowd_frac=0.2, mode='segm'):
    """rsp_coco_iou over a batch of images (one unit each), exactly equal to rleIou / bbIou of the restatement"""
    from rsprompter_amd import rle
    dt_rles, gt_rles, dt_box, gt_box, crowd, nds, ngs = [], [], [], [], [], [], []
    for i in range(n_img):
        a, b = int(rng.integers(0, nd + 1)) if i % 3 == 2 else nd, ng if i % 4 != 3 else int(rng.integers(0, ng + 1))
        nds.append(a)
        ngs.append(b)
        for _ in range(a):
            dt_rles.append(rle_dict(random_mask(rng, h, w, 'blob')))
            x, y = rng.integers(0, w), rng.integers(0, h)
            dt_box.append([float(x), float(y), float(rng.integers(1, w // 2)) + 0.5, float(rng.integers(1, h // 2))])
        for _ in range(b):
            gt_rles.append(rle_dict(random_mask(rng, h, w, 'blob')))
            x, y = rng.integers(0, w), rng.integers(0, h)
            gt_box.append([float(x), float(y), float(rng.integers(1, w // 2)), float(rng.integers(1, h // 2)) + 0.25])
            crowd.append(int(rng.random() < crowd_frac))
    # exact-threshold and identical pairs: a dt that equals a gt
    if nds[0] and ngs[0]:
        dt_rles[0] = gt_rles[0]
        dt_box[0] = list(gt_box[0])
    nd_a, ng_a = np.array(nds), np.array(ngs)
    dt0 = np.concatenate([[0], np.cumsum(nd_a)[:-1]])
    gt0 = np.concatenate([[0], np.cumsum(ng_a)[:-1]])
    out0 = np.concatenate([[0], np.cumsum(nd_a * ng_a)[:-1]])
    n_iou = int((nd_a * ng_a).sum())
    units = ops.coco_units(dt0, gt0, out0, nd_a, ng_a, np.full(n_img, (h * w + 63) // 64), dev)
    g_crowd = torch.tensor(crowd + [0], dtype=torch.uint8, device=dev)
    if mode == 'segm':
        db, dwo, da, dwr = rle.runs_to_bits(*rle.strings_to_runs([r['counts'] for r in dt_rles], dev), [r['size'] for r in dt_rles])
        gb, gwo, ga, gwr = rle.runs_to_bits(*rle.strings_to_runs([r['counts'] for r in gt_rles], dev), [r['size'] for r in gt_rles])
        iou = ops.coco_iou(units, n_iou, ops.COCO_IOU_SEGM, gt_crowd=g_crowd, dt_bits=db, gt_bits=gb, dt_woff=dwo,
                           gt_woff=gwo, dt_wrange=dwr, gt_wrange=gwr, dt_area=da, gt_area=ga)
    else:
        iou = ops.coco_iou(units, n_iou, ops.COCO_IOU_BBOX, gt_crowd=g_crowd,
                           dt_box=torch.tensor(dt_box + [[0.0] * 4], dtype=torch.float64, device=dev),
                           gt_box=torch.tensor(gt_box + [[0.0] * 4], dtype=torch.float64, device=dev))
    got = iou.cpu().numpy()
    n_checked = 0
    for i in range(n_img):
        if nds[i] == 0 or ngs[i] == 0:
            continue
        dsl = slice(dt0[i], dt0[i] + nds[i])
        gsl = slice(gt0[i], gt0[i] + ngs[i])
        if mode == 'segm':
            d = [(ref.rle_fr_string(r['counts']), h, w) for r in dt_rles[dsl]]
            g = [(ref.rle_fr_string(r['counts']), h, w) for r in gt_rles[gsl]]
            want = ref.rle_iou(d, g, crowd[gsl])
        else:
            want = ref.bb_iou(dt_box[dsl], gt_box[gsl], crowd[gsl])
        blk = got[out0[i]:out0[i] + nds[i] * ngs[i]].reshape(nds[i], ngs[i])
        assert np.array_equal(blk, want), (i, np.abs(blk - want).max())
        n_checked += int((want > 0).sum())
    return n_checked


# ----------------------------------------------------------------------------- matching + accumulate (through the metric)
def synth_eval_case(rng, n_img, n_cat, nd, ng, h, w, mode='bbox', ties=True, boundary=True, crowd_frac=0.1,
                    img_id_zero=True):
    """a COCO gt dict + a result list: forced score ties within and across images, IoUs exactly at thresholds, areas
    exactly on range boundaries, images without gt / without dt, gt id 0"""
    images, anns, res = [], [], []
    ids = list(rng.permutation(np.arange(n_img) * 3 + 1))              # unsorted image ids
    scores_pool = np.round(rng.random(8), 2)
    ann_id = 0 if img_id_zero else 1
    for ii, img_id in enumerate(ids):
        img_id = int(img_id)
        images.append(dict(id=img_id, height=h, width=w, file_name=f'{img_id}.jpg'))
        n_g = 0 if ii % 5 == 4 else int(rng.integers(1, ng + 1))
        n_d = 0 if ii % 7 == 6 else int(rng.integers(1, nd + 1))
        gboxes = []
        for _ in range(n_g):
            side = int(rng.choice([32, 96, 16, 50, 120])) if boundary else int(rng.integers(4, w // 2))
            x, y = int(rng.integers(0, w - side)), int(rng.integers(0, h - side))
            bb = [float(x), float(y), float(side), float(side)]
            gboxes.append(bb)
            cat = int(rng.integers(1, n_cat + 1))
            a = dict(id=ann_id, image_id=img_id, category_id=cat, bbox=bb, area=float(side * side),
                     iscrowd=int(rng.random() < crowd_frac))
            if mode == 'segm':
                m = np.zeros((h, w), dtype=np.uint8)
                m[y:y + side, x:x + side] = 1
                a['segmentation'] = dict(size=[h, w], counts=ref.rle_to_string(ref.rle_encode(m)).decode())
            anns.append(a)
            ann_id += 1
        for j in range(n_d):
            if gboxes and rng.random() < 0.6:
                g = gboxes[int(rng.integers(len(gboxes)))]
                # shrink the height so that IoU hits 0.75 / 0.5 exactly, or keep it (1.0)
                f = float(rng.choice([1.0, 0.75, 0.5, 0.9]))
                bb = [g[0], g[1], g[2], g[3] * f]
            else:
                side = int(rng.integers(4, w // 3))
                bb = [float(rng.integers(0, w - side)), float(rng.integers(0, h - side)), float(side), float(side)]
            cat = int(rng.integers(1, n_cat + 1))
            score = float(scores_pool[int(rng.integers(len(scores_pool)))]) if ties else float(rng.random())
            r = dict(image_id=img_id, category_id=cat, bbox=bb, score=score)
            if mode == 'segm':
                m = np.zeros((h, w), dtype=np.uint8)
                x0, y0 = int(bb[0]), int(bb[1])
                m[y0:y0 + int(round(bb[3])), x0:x0 + int(round(bb[2]))] = 1
                r['segmentation'] = dict(size=[h, w], counts=ref.rle_to_string(ref.rle_encode(m)).decode())
            res.append(r)
    cats = [dict(id=c, name=f'c{c}') for c in range(1, n_cat + 1)]
    return dict(images=images, annotations=anns, categories=cats), res


def product_stats(gt, res, iou_type, dev, max_dets=(100, 300, 1000)):
    """rsprompter_amd.evaluation.device_evaluate on the loadRes'd results, with CocoMetric's parameters"""
    from rsprompter_amd import evaluation as E
    gt_m = gt
    results = res
    if iou_type == 'segm':
        results = [{k: v for k, v in r.items() if k != 'bbox'} for r in res]
        gt_m = dict(gt, annotations=[dict(a, segmentation=E.ann_to_rle(a['segmentation'], gt_img['height'],
                                                                         gt_img['width']))
                                     for a in gt['annotations']
                                     for gt_img in [next(i for i in gt['images'] if i['id'] == a['image_id'])]])
    dts = E.load_res(gt_m, results, iou_type)
    for d in dts:
        if iou_type == 'segm':
            c = d['segmentation']['counts']
            d['segmentation'] = dict(size=d['segmentation']['size'], counts=c.encode() if isinstance(c, str) else c)
    thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    img_ids = [im['id'] for im in gt['images']]
    cat_ids = [c['id'] for c in gt['categories']]
    return E.device_evaluate(gt_m, dts, iou_type, img_ids, cat_ids, thrs, list(max_dets), dev)


def check_stats_equal(gt, res, iou_type, dev, max_dets=(100, 300, 1000)):
    ev = product_stats(gt, res, iou_type, dev, max_dets)
    want, rev = ref.coco_stats(gt, res, iou_type, max_dets=max_dets)
    assert np.array_equal(ev.stats, want), (ev.stats, want)
    assert np.array_equal(ev.eval['precision'], rev.eval['precision'])
    assert np.array_equal(ev.eval['recall'], rev.eval['recall'])
    check_tables_equal(ev.tables, rev)
    return ev.stats


def check_tables_equal(tb, rev):
    """dt matched (gt ids), dt ignored and the non-ignored gt count of every (category, area range, image) unit against
    the restatement's evaluateImg records"""
    I, K = tb['n_img'], tb['n_cat']
    A = tb['dtm'].shape[0]
    n = 0
    for k in range(K):
        for a in range(A):
            for i in range(I):
                e = rev.evalImgs[k * A * I + a * I + i]
                u = k * I + i
                if e is None:
                    assert tb['nd'][u] == 0 and tb['ng'][u] == 0
                    continue
                sl = slice(tb['dt0'][u], tb['dt0'][u] + tb['nd'][u])
                assert tb['dt_ids'][sl].tolist() == list(e['dtIds'])
                assert np.array_equal(tb['dtm'][a][:, sl], e['dtMatches'])
                assert np.array_equal(tb['dtig'][a][:, sl], e['dtIgnore'])
                assert tb['npig'][u, a] == np.count_nonzero(e['gtIgnore'] == 0)
                n += 1
    assert n > 0
