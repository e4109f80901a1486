"""TEST ORACLE: a literal restatement of cocoapi (pycocotools coco.py / cocoeval.py and maskApi.c), written loop by loop
from the published definitions, because pycocotools is not installed.  Imports nothing from rsprompter_amd.

Covers COCO.loadRes, COCOeval.evaluate / computeIoU / evaluateImg / accumulate / summarize and maskApi's rleFrPoly,
rleFrString, rleToString, rleMerge, rleArea, rleToBbox, rleIou, bbIou.  Annotation ids are match markers exactly as in
pycocotools (a detection matched to the gt with id 0 counts as unmatched)."""
import copy
import itertools
import math
from collections import defaultdict

import numpy as np


# ----------------------------------------------------------------------------- maskApi.c
def rle_fr_string(s):
    if isinstance(s, str):
        s = s.encode()
    cnts = []
    p = 0
    m = 0
    while p < len(s) and s[p]:
        x = 0
        k = 0
        more = 1
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << 5 * k
            more = c & 0x20
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << 5 * k
        if m > 2:
            x += cnts[m - 2]
        cnts.append(x % (1 << 32))
        m += 1
    return cnts


def rle_to_string(cnts):
    out = bytearray()
    for i in range(len(cnts)):
        x = int(cnts[i])
        if i > 2:
            x -= int(cnts[i - 2])
        more = 1
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            c += 48
            out.append(c)
    return bytes(out)


def rle_fr_poly(xy, h, w):
    scale = 5.0
    k = len(xy) // 2
    x = [0] * (k + 1)
    y = [0] * (k + 1)
    for j in range(k):
        x[j] = int(scale * xy[j * 2 + 0] + .5)
    x[k] = x[0]
    for j in range(k):
        y[j] = int(scale * xy[j * 2 + 1] + .5)
    y[k] = y[0]
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx = abs(xe - xs)
        dy = abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            t = xs; xs = xe; xe = t                       # noqa: E702
            t = ys; ys = ye; ye = t                       # noqa: E702
        if dx >= dy:
            s = (ye - ys) / dx if dx != 0 else float('nan')
        else:
            s = (xe - xs) / dy
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                vv = ys + s * t + .5
                v.append(int(vv) if vv == vv else -(1 << 31))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    xs_, ys_ = [], []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / scale - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / scale - .5
            if yd < 0:
                yd = 0
            elif yd > h:
                yd = h
            yd = math.ceil(yd)
            xs_.append(int(xd))
            ys_.append(int(yd))
    k = len(xs_)
    a = [(xs_[j] * h + ys_[j]) % (1 << 32) for j in range(k)]
    a.append(h * w)
    k += 1
    a.sort()
    p = 0
    for j in range(k):
        t = a[j]
        a[j] -= p
        p = t
    b = []
    j = 0
    b.append(a[j])
    j += 1
    while j < k:
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < k:
                b[-1] += a[j]
                j += 1
    return b


def rle_fr_bbox(bb, h, w):
    xs = bb[0]; ys = bb[1]; xe = xs + bb[2]; ye = ys + bb[3]  # noqa: E702
    return rle_fr_poly([xs, ys, xs, ye, xe, ye, xe, ys], h, w)


def rle_merge(R, intersect=0):
    if len(R) == 0:
        return []
    if len(R) == 1:
        return list(R[0])
    cnts = list(R[0])
    for i in range(1, len(R)):
        A, B = cnts, R[i]
        cnts = []
        ca = A[0]
        cb = B[0]
        v = va = vb = 0
        a = b = 1
        cc = 0
        ct = 1
        while ct > 0:
            c = min(ca, cb)
            cc += c
            ct = 0
            ca -= c
            if not ca and a < len(A):
                ca = A[a]; a += 1; va = not va            # noqa: E702
            ct += ca
            cb -= c
            if not cb and b < len(B):
                cb = B[b]; b += 1; vb = not vb            # noqa: E702
            ct += cb
            vp = v
            v = (va and vb) if intersect else (va or vb)
            if v != vp or ct == 0:
                cnts.append(cc)
                cc = 0
    return cnts


def rle_area(cnts):
    a = 0
    for j in range(1, len(cnts), 2):
        a += cnts[j]
    return a


def rle_to_bbox(cnts, h, w):
    m = (len(cnts) // 2) * 2
    if m == 0:
        return [0.0, 0.0, 0.0, 0.0]
    xs, ys, xe, ye = w, h, 0, 0
    cc = 0
    xp = 0
    for j in range(m):
        cc += cnts[j]
        t = cc - j % 2
        y = t % h
        x = (t - y) // h
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys = 0
            ye = h - 1
        xs = min(xs, x)
        xe = max(xe, x)
        ys = min(ys, y)
        ye = max(ye, y)
    return [float(xs), float(ys), float(xe - xs + 1), float(ye - ys + 1)]


def rle_decode(cnts, h, w):
    flat = np.zeros(h * w, dtype=np.uint8)
    p, v = 0, 0
    for c in cnts:
        flat[p:p + c] = v
        p += c
        v = 1 - v
    return flat.reshape(w, h).T


def rle_encode(mask):
    flat = np.asarray(mask, dtype=np.uint8).T.reshape(-1)
    cnts, p, c = [], 0, 0
    for val in flat:
        if val != p:
            cnts.append(c)
            c = 0
            p = val
        c += 1
    cnts.append(c)
    return cnts


def bb_iou(dt, gt, iscrowd):
    m, n = len(dt), len(gt)
    o = np.zeros((m, n))
    for g in range(n):
        G = gt[g]
        ga = G[2] * G[3]
        crowd = iscrowd is not None and iscrowd[g]
        for d in range(m):
            D = dt[d]
            da = D[2] * D[3]
            o[d, g] = 0
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            u = da if crowd else da + ga - i
            o[d, g] = i / u
    return o


def rle_iou(dt, gt, iscrowd):
    """dt / gt: lists of (cnts, h, w)"""
    m, n = len(dt), len(gt)
    db = [rle_to_bbox(c, h, w) for c, h, w in dt]
    gb = [rle_to_bbox(c, h, w) for c, h, w in gt]
    o = bb_iou(db, gb, iscrowd)
    for g in range(n):
        for d in range(m):
            if o[d, g] > 0:
                crowd = iscrowd is not None and iscrowd[g]
                if dt[d][1] != gt[g][1] or dt[d][2] != gt[g][2]:
                    o[d, g] = -1
                    continue
                A, B = dt[d][0], gt[g][0]
                ka, kb = len(A), len(B)
                ca = A[0]; cb = B[0]; va = vb = 0; a = b = 1; i = u = 0; ct = 1   # noqa: E702
                while ct > 0:
                    c = min(ca, cb)
                    if va or vb:
                        u += c
                        if va and vb:
                            i += c
                    ct = 0
                    ca -= c
                    if not ca and a < ka:
                        ca = A[a]; a += 1; va = not va    # noqa: E702
                    ct += ca
                    cb -= c
                    if not cb and b < kb:
                        cb = B[b]; b += 1; vb = not vb    # noqa: E702
                    ct += cb
                if i == 0:
                    u = 1
                elif crowd:
                    u = rle_area(A)
                o[d, g] = i / u
    return o


def segm_to_cnts(segm, h, w):
    """pycocotools annToRLE -> (cnts, h, w)"""
    if isinstance(segm, list):
        if len(segm[0]) == 4 if isinstance(segm[0], list) else False:
            rles = [rle_fr_bbox(p, h, w) for p in segm]
        else:
            rles = [rle_fr_poly(p, h, w) for p in segm]
        return rle_merge(rles), h, w
    if isinstance(segm['counts'], list):
        return list(segm['counts']), segm['size'][0], segm['size'][1]
    return rle_fr_string(segm['counts']), segm['size'][0], segm['size'][1]


# ----------------------------------------------------------------------------- coco.py
class COCO:
    def __init__(self, dataset):
        self.dataset = copy.deepcopy(dataset)
        self.anns, self.cats, self.imgs = {}, {}, {}
        self.imgToAnns, self.catToImgs = defaultdict(list), defaultdict(list)
        for ann in self.dataset.get('annotations', []):
            self.imgToAnns[ann['image_id']].append(ann)
            self.anns[ann['id']] = ann
        for img in self.dataset.get('images', []):
            self.imgs[img['id']] = img
        for cat in self.dataset.get('categories', []):
            self.cats[cat['id']] = cat

    def getImgIds(self):
        return list(self.imgs.keys())

    def getCatIds(self, catNms=()):
        cats = self.dataset['categories']
        if len(catNms):
            cats = [c for c in cats if c['name'] in catNms]
        return [c['id'] for c in cats]

    def getAnnIds(self, imgIds, catIds):
        lists = [self.imgToAnns[i] for i in imgIds if i in self.imgToAnns]
        anns = list(itertools.chain.from_iterable(lists))
        anns = [a for a in anns if a['category_id'] in catIds]
        return [a['id'] for a in anns], anns

    def loadRes(self, anns):
        res = COCO(dict(images=[img for img in self.dataset['images']]))
        anns = copy.deepcopy(anns)
        annsImgIds = [ann['image_id'] for ann in anns]
        assert set(annsImgIds) == (set(annsImgIds) & set(self.getImgIds()))
        if 'bbox' in anns[0] and not anns[0]['bbox'] == []:
            res.dataset['categories'] = copy.deepcopy(self.dataset['categories'])
            for id, ann in enumerate(anns):
                bb = ann['bbox']
                x1, x2, y1, y2 = [bb[0], bb[0] + bb[2], bb[1], bb[1] + bb[3]]
                if 'segmentation' not in ann:
                    ann['segmentation'] = [[x1, y1, x1, y2, x2, y2, x2, y1]]
                ann['area'] = bb[2] * bb[3]
                ann['id'] = id + 1
                ann['iscrowd'] = 0
        elif 'segmentation' in anns[0]:
            res.dataset['categories'] = copy.deepcopy(self.dataset['categories'])
            for id, ann in enumerate(anns):
                cnts, h, w = segm_to_cnts(ann['segmentation'], None, None)
                ann['area'] = rle_area(cnts)
                if 'bbox' not in ann:
                    ann['bbox'] = rle_to_bbox(cnts, h, w)
                ann['id'] = id + 1
                ann['iscrowd'] = 0
        res.dataset['annotations'] = anns
        return COCO(res.dataset)


# ----------------------------------------------------------------------------- cocoeval.py
class Params:
    def __init__(self):
        self.imgIds = []
        self.catIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1


class COCOeval:
    def __init__(self, cocoGt, cocoDt, iouType='segm'):
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.params = Params()
        self.params.iouType = iouType
        self.params.imgIds = sorted(cocoGt.getImgIds())
        self.params.catIds = sorted(cocoGt.getCatIds())
        self.eval = {}
        self.stats = []

    def _prepare(self):
        p = self.params
        _, gts = self.cocoGt.getAnnIds(p.imgIds, p.catIds)
        _, dts = self.cocoDt.getAnnIds(p.imgIds, p.catIds)
        if p.iouType == 'segm':
            for ann in gts:
                img = self.cocoGt.imgs[ann['image_id']]
                ann['_rle'] = segm_to_cnts(ann['segmentation'], img['height'], img['width'])
            for ann in dts:
                ann['_rle'] = segm_to_cnts(ann['segmentation'], None, None)
        for gt in gts:
            gt['ignore'] = gt['ignore'] if 'ignore' in gt else 0
            gt['ignore'] = 'iscrowd' in gt and gt['iscrowd']
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for gt in gts:
            self._gts[gt['image_id'], gt['category_id']].append(gt)
        for dt in dts:
            self._dts[dt['image_id'], dt['category_id']].append(dt)

    def evaluate(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self._prepare()
        self.ious = {(imgId, catId): self.computeIoU(imgId, catId) for imgId in p.imgIds for catId in p.catIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(imgId, catId, areaRng, maxDet)
                         for catId in p.catIds for areaRng in p.areaRng for imgId in p.imgIds]
        self._paramsEval = copy.deepcopy(self.params)

    def computeIoU(self, imgId, catId):
        p = self.params
        gt = self._gts[imgId, catId]
        dt = self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in inds]
        if len(dt) > p.maxDets[-1]:
            dt = dt[0:p.maxDets[-1]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        if len(dt) == 0 or len(gt) == 0:
            return []
        if p.iouType == 'segm':
            return rle_iou([d['_rle'] for d in dt], [g['_rle'] for g in gt], iscrowd)
        return bb_iou([d['bbox'] for d in dt], [g['bbox'] for g in gt], iscrowd)

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        p = self.params
        gt = self._gts[imgId, catId]
        dt = self._dts[imgId, catId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            if g['ignore'] or (g['area'] < aRng[0] or g['area'] > aRng[1]):
                g['_ignore'] = 1
            else:
                g['_ignore'] = 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        ious = self.ious[imgId, catId][:, gtind] if len(self.ious[imgId, catId]) > 0 else self.ious[imgId, catId]
        T = len(p.iouThrs)
        G = len(gt)
        D = len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gtIg = np.array([g['_ignore'] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(p.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return dict(image_id=imgId, category_id=catId, aRng=aRng, maxDet=maxDet, dtIds=[d['id'] for d in dt],
                    gtIds=[g['id'] for g in gt], dtMatches=dtm, gtMatches=gtm, dtScores=[d['score'] for d in dt],
                    gtIgnore=gtIg, dtIgnore=dtIg)

    def accumulate(self):
        p = self.params
        T = len(p.iouThrs)
        R = len(p.recThrs)
        K = len(p.catIds)
        A = len(p.areaRng)
        M = len(p.maxDets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        _pe = self._paramsEval
        setK, setA, setM, setI = set(_pe.catIds), set(map(tuple, _pe.areaRng)), set(_pe.maxDets), set(_pe.imgIds)
        k_list = [n for n, k in enumerate(p.catIds) if k in setK]
        m_list = [m for n, m in enumerate(p.maxDets) if m in setM]
        a_list = [n for n, a in enumerate(map(lambda x: tuple(x), p.areaRng)) if a in setA]
        i_list = [n for n, i in enumerate(p.imgIds) if i in setI]
        I0 = len(_pe.imgIds)
        A0 = len(_pe.areaRng)
        for k, k0 in enumerate(k_list):
            Nk = k0 * A0 * I0
            for a, a0 in enumerate(a_list):
                Na = a0 * I0
                for m, maxDet in enumerate(m_list):
                    E = [self.evalImgs[Nk + Na + i] for i in i_list]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                    inds = np.argsort(-dtScores, kind='mergesort')
                    dtScoresSorted = dtScores[inds]
                    dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e['gtIgnore'] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        tp = np.array(tp)
                        fp = np.array(fp)
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,))
                        ss = np.zeros((R,))
                        if nd:
                            recall[t, k, a, m] = rc[-1]
                        else:
                            recall[t, k, a, m] = 0
                        pr = pr.tolist()
                        q = q.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds = np.searchsorted(rc, p.recThrs, side='left')
                        try:
                            for ri, pi in enumerate(inds):
                                q[ri] = pr[pi]
                                ss[ri] = dtScoresSorted[pi]
                        except IndexError:
                            pass
                        precision[t, :, k, a, m] = np.array(q)
                        scores[t, :, k, a, m] = np.array(ss)
        self.eval = dict(precision=precision, recall=recall, scores=scores)

    def summarize(self):
        def _summarize(ap=1, iouThr=None, areaRng='all', maxDets=100):
            p = self.params
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
            if ap == 1:
                s = self.eval['precision']
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval['recall']
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, aind, mind]
            if len(s[s > -1]) == 0:
                mean_s = -1
            else:
                mean_s = np.mean(s[s > -1])
            return mean_s

        md = self.params.maxDets
        stats = np.zeros((12,))
        stats[0] = _summarize(1, maxDets=md[2])
        stats[1] = _summarize(1, iouThr=.5, maxDets=md[2])
        stats[2] = _summarize(1, iouThr=.75, maxDets=md[2])
        stats[3] = _summarize(1, areaRng='small', maxDets=md[2])
        stats[4] = _summarize(1, areaRng='medium', maxDets=md[2])
        stats[5] = _summarize(1, areaRng='large', maxDets=md[2])
        stats[6] = _summarize(0, maxDets=md[0])
        stats[7] = _summarize(0, maxDets=md[1])
        stats[8] = _summarize(0, maxDets=md[2])
        stats[9] = _summarize(0, areaRng='small', maxDets=md[2])
        stats[10] = _summarize(0, areaRng='medium', maxDets=md[2])
        stats[11] = _summarize(0, areaRng='large', maxDets=md[2])
        self.stats = stats


def coco_stats(gt_json, results, iou_type, img_ids=None, cat_ids=None, max_dets=(100, 300, 1000), iou_thrs=None):
    """mmdet CocoMetric's use of COCOeval: params.catIds / imgIds / maxDets = proposal_nums / iouThrs -> (stats, eval)"""
    gt = COCO(gt_json)
    if iou_type == 'segm':
        results = [{k: v for k, v in r.items() if k != 'bbox'} for r in results]
    dt = gt.loadRes(results)
    ev = COCOeval(gt, dt, iou_type)
    ev.params.catIds = list(cat_ids) if cat_ids is not None else gt.getCatIds()
    ev.params.imgIds = list(img_ids) if img_ids is not None else gt.getImgIds()
    ev.params.maxDets = list(max_dets)
    if iou_thrs is not None:
        ev.params.iouThrs = iou_thrs
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev.stats, ev


# ----------------------------------------------------------------------------- numpy forms for large inputs
def rle_fr_string_np(s):
    """rle_fr_string vectorised (same integer definitions): for the noise masks of seeded synthetic weights"""
    if isinstance(s, str):
        s = s.encode()
    c = np.frombuffer(s, dtype=np.uint8).astype(np.int64) - 48
    if c.size == 0:
        return []
    end = (c & 0x20) == 0
    vid = np.concatenate([[0], np.cumsum(end)[:-1]])
    start = np.concatenate([[True], end[:-1]])
    k = np.arange(c.size) - np.maximum.accumulate(np.where(start, np.arange(c.size), 0))
    n = int(end.sum())
    x = np.zeros(n, dtype=np.int64)
    np.add.at(x, vid, (c & 0x1f) << (5 * k))
    last = np.nonzero(end)[0]
    neg = (c[last] & 0x10) != 0
    x[neg] |= -1 << (5 * (k[last][neg] + 1))
    out = x.copy()
    if n > 3:
        out[3::2] = np.cumsum(x[3::2]) + x[1]
    if n > 4:
        out[4::2] = np.cumsum(x[4::2]) + x[2]
    return [int(v) for v in (out % (1 << 32))]


def rle_iou_np(dt, gt, iscrowd):
    """rle_iou on decoded masks: inter / union of pixel counts, union = |d| inside a crowd gt, 0 when inter == 0"""
    m, n = len(dt), len(gt)
    o = np.zeros((m, n))
    D = [rle_decode(c, h, w).astype(bool) for c, h, w in dt]
    G = [rle_decode(c, h, w).astype(bool) for c, h, w in gt]
    for g in range(n):
        for d in range(m):
            i = int(np.logical_and(D[d], G[g]).sum())
            if i == 0:
                continue
            u = int(D[d].sum()) if iscrowd[g] else int(D[d].sum()) + int(G[g].sum()) - i
            o[d, g] = i / u
    return o


def use_numpy_forms():
    """switch the string decode and the mask IoU of this module to their numpy forms (identical results)"""
    g = globals()
    g['rle_fr_string'], g['rle_iou'] = rle_fr_string_np, rle_iou_np


def rle_to_bbox_np(cnts, h, w):
    m = (len(cnts) // 2) * 2
    if m == 0:
        return [0.0, 0.0, 0.0, 0.0]
    cc = np.cumsum(np.asarray(cnts[:m], dtype=np.int64))
    t = cc - (np.arange(m) % 2)
    y = t % h
    x = (t - y) // h
    xs, xe, ys, ye = int(x.min()), int(x.max()), int(y.min()), int(y.max())
    if np.any(x[0::2] < x[1::2]):
        ys, ye = 0, h - 1
    return [float(xs), float(ys), float(xe - xs + 1), float(ye - ys + 1)]


def rle_area_np(cnts):
    return int(np.asarray(cnts[1::2], dtype=np.int64).sum())


def _use_numpy_forms_all():
    g = globals()
    g['rle_fr_string'], g['rle_iou'], g['rle_to_bbox'], g['rle_area'] = rle_fr_string_np, rle_iou_np, rle_to_bbox_np, \
        rle_area_np


use_numpy_forms = _use_numpy_forms_all
