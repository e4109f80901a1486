"""`DATASETS` registry with the COCO-format datasets the RSPrompter configs name (the ground truth of the
mAP runs).

Reference: mmdet/datasets/coco.py (`load_data_list`:60-100, `parse_data_info`:102-160), mmdet/rsprompter/datasets.py:5-28
(the three class lists), and the ground-truth half of the test pipeline, `LoadAnnotations(with_bbox=True, with_mask=True)`
(mmdet/datasets/transforms/loading.py:308-372).  Item i is what `apis.TestPipeline` needs (`img_path`, `img_id`) plus the
image's ground truth -- it travels NEXT TO the pipeline output, the pipeline itself is unchanged:

    bboxes        float32 [n, 4] xyxy              labels   int64 [n]
    ignore_flags  bool [n] (crowd / no valid polygon: PackDetInputs moves these to `ignored_instances`)
    masks         n COCO RLE dicts at ori_shape, dict(size=[h, w], counts=bytes) (compressed)

Polygons become RLE the way cocoapi does it (maskApi.c rleFrPoly: upsample x5, walk the edges, keep the y-boundary
crossings, downsample; then rleMerge of the parts).  This is host code: it runs once per dataset.  `anns_to_rle` is its
batched twin on the device (csrc/poly_raster.hip): many annotations in one call, the same strings.
"""
import json
import math
import os

import numpy as np

from .registry import Registry
from .rle import counts_to_string

DATASETS = Registry('dataset')


# ----------------------------------------------------------------------------- cocoapi maskApi on the host
def rle_from_poly(xy, h, w):
    """maskApi.c rleFrPoly (restated): polygon [x0, y0, x1, y1, ...] -> run counts of the h x w mask."""
    scale = 5.0
    k = len(xy) // 2
    x = [int(scale * float(xy[2 * j]) + .5) for j in range(k)]
    y = [int(scale * float(xy[2 * j + 1]) + .5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else 0.0
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            s = (xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    a = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + .5) / scale - .5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / scale - .5
        yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
        yd = math.ceil(yd)
        a.append((int(xd) * h + int(yd)) & 0xffffffff)
    a.append(h * w)
    a.sort()
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    b = [a[0]]
    j = 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return b


def rle_from_bbox(bb, h, w):
    """maskApi.c rleFrBbox: the xywh box as a 4-point polygon."""
    xs, ys = bb[0], bb[1]
    xe, ye = xs + bb[2], ys + bb[3]
    return rle_from_poly([xs, ys, xs, ye, xe, ye, xe, ys], h, w)


def rle_merge(rles):
    """maskApi.c rleMerge (union) of run-count lists of one size."""
    if not rles:
        return []
    cnts = list(rles[0])
    for B in rles[1:]:
        A = cnts
        cnts = []
        ca, cb = (A[0] if A else 0), (B[0] if B else 0)
        v = va = vb = 0
        a = b = 1
        cc, ct = 0, 1
        while ct > 0:
            c = min(ca, cb)
            cc += c
            ct = 0
            ca -= c
            if not ca and a < len(A):
                ca = A[a]
                a += 1
                va = not va
            ct += ca
            cb -= c
            if not cb and b < len(B):
                cb = B[b]
                b += 1
                vb = not vb
            ct += cb
            vp = v
            v = va or vb
            if v != vp or ct == 0:
                cnts.append(cc)
                cc = 0
    return cnts


def rle_from_string(s):
    """maskApi.c rleFrString (host twin of rsp_rle_from_string)."""
    if isinstance(s, str):
        s = s.encode()
    cnts, p = [], 0
    while p < len(s) and s[p]:
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << 5 * k
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << 5 * k
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & 0xffffffff)
    return cnts


def ann_to_rle(segm, h, w):
    """pycocotools COCO.annToRLE / frPyObjects: polygons (merged), uncompressed or compressed RLE -> dict(size, counts
    bytes) (compressed)."""
    if isinstance(segm, list):
        if len(segm) and not isinstance(segm[0], (list, tuple, np.ndarray)):
            segm = [segm]
        parts = [rle_from_bbox(p, h, w) if len(p) == 4 else rle_from_poly(p, h, w) for p in segm]
        return dict(size=[h, w], counts=counts_to_string(rle_merge(parts)))
    if isinstance(segm.get('counts'), list):
        return dict(size=list(segm['size']), counts=counts_to_string(segm['counts']))
    c = segm['counts']
    return dict(size=list(segm['size']), counts=c.encode() if isinstance(c, str) else bytes(c))


def bbox_polygon(bb):
    """maskApi.c rleFrBbox's polygon of an xywh box: [xs, ys, xs, ye, xe, ye, xe, ys]"""
    xs, ys = bb[0], bb[1]
    xe, ye = xs + bb[2], ys + bb[3]
    return [xs, ys, xs, ye, xe, ye, xe, ys]


def anns_to_rle(segms, sizes, device='cuda:0'):
    """ann_to_rle of MANY segmentations in one device call: segms[i] is what ann_to_rle takes (a COCO polygon
    list, nested or flat, a 4-number part being an xywh box; or an RLE dict, which passes through as it does there), sizes[i]
    = (h, w) of its image (one pair serves all) -> list of dict(size=[h, w], counts=bytes), equal to
    [ann_to_rle(s, h, w) for ...].  Every polygon part is rasterised by csrc/poly_raster.hip, the parts of an annotation are
    unioned in the run domain (rle.polygons_to_runs, fill='union') and the strings are written by rsp_rle_to_string."""
    import torch
    from . import ops, rle
    segms = list(segms)
    if len(sizes) == 2 and not isinstance(sizes[0], (list, tuple, np.ndarray)):
        sizes = [sizes] * len(segms)
    if len(sizes) != len(segms):
        raise ValueError(f'anns_to_rle: {len(segms)} segmentations but {len(sizes)} sizes')
    out = [None] * len(segms)
    rows, rings, ring_group, hw = [], [], [], []
    for i, segm in enumerate(segms):
        h, w = int(sizes[i][0]), int(sizes[i][1])
        if not isinstance(segm, list):
            out[i] = ann_to_rle(segm, h, w)
            continue
        if len(segm) and not isinstance(segm[0], (list, tuple, np.ndarray)):
            segm = [segm]
        if not segm:                                         # rleMerge of no parts: no counts at all
            out[i] = dict(size=[h, w], counts=b'')
            continue
        for p in segm:
            p = bbox_polygon(p) if len(p) == 4 else p
            rings.append(np.asarray(p[:2 * (len(p) // 2)], dtype=np.float64).reshape(-1, 2))
            ring_group.append(len(rows))
        rows.append(i)
        hw.append((h, w))
    if rows:
        dev = torch.device(device)
        ops.require_device(dev)
        offs = np.cumsum([0] + [len(r) for r in rings]).astype(np.int64)
        counts, n = rle.polygons_to_runs(torch.from_numpy(np.concatenate(rings).reshape(-1, 2)).to(dev),
                                         torch.from_numpy(offs).to(dev),
                                         torch.tensor(ring_group, dtype=torch.int32, device=dev),
                                         torch.tensor(hw, dtype=torch.int32, device=dev), fill='union')
        flat, soffs = rle._string_bytes(counts.contiguous(), n, 2 * len(rows) * int(counts.shape[1]) + 16)
        buf, o = flat.numpy().tobytes(), soffs.tolist()
        for j, i in enumerate(rows):
            out[i] = dict(size=[hw[j][0], hw[j][1]], counts=buf[o[j]:o[j + 1]])
    return out


def gt_mask_rle(mask_ann, h, w):
    """LoadAnnotations._process_masks + _poly2mask + encode: None when the instance is left without a valid polygon
    (polygons with fewer than 6 or an odd number of coordinates are dropped), else the compressed RLE dict."""
    if isinstance(mask_ann, list):
        polys = [p for p in mask_ann if len(p) % 2 == 0 and len(p) >= 6]
        if not polys:
            return None
        return ann_to_rle(polys, h, w)
    if isinstance(mask_ann, dict) and mask_ann.get('counts') is not None and mask_ann.get('size') is not None and \
            isinstance(mask_ann['counts'], (list, str, bytes)):
        return ann_to_rle(mask_ann, h, w)
    return None


# ----------------------------------------------------------------------------- datasets
@DATASETS.register_module()
class CocoDataset:
    """mmdet CocoDataset in test mode: images in the JSON's insertion order, instances filtered by `parse_data_info`."""
    METAINFO = dict(classes=('person', 'bicycle', 'car', 'motorcycle', 'airplane', 'bus', 'train', 'truck', 'boat',
                             'traffic light', 'fire hydrant', 'stop sign', 'parking meter', 'bench', 'bird', 'cat',
                             'dog', 'horse', 'sheep', 'cow', 'elephant', 'bear', 'zebra', 'giraffe', 'backpack',
                             'umbrella', 'handbag', 'tie', 'suitcase', 'frisbee', 'skis', 'snowboard', 'sports ball',
                             'kite', 'baseball bat', 'baseball glove', 'skateboard', 'surfboard', 'tennis racket',
                             'bottle', 'wine glass', 'cup', 'fork', 'knife', 'spoon', 'bowl', 'banana', 'apple',
                             'sandwich', 'orange', 'broccoli', 'carrot', 'hot dog', 'pizza', 'donut', 'cake', 'chair',
                             'couch', 'potted plant', 'bed', 'dining table', 'toilet', 'tv', 'laptop', 'mouse', 'remote',
                             'keyboard', 'cell phone', 'microwave', 'oven', 'toaster', 'sink', 'refrigerator', 'book',
                             'clock', 'vase', 'scissors', 'teddy bear', 'hair drier', 'toothbrush'))

    def __init__(self, ann_file='', data_root='', data_prefix=None, test_mode=True, pipeline=None, indices=None,
                 backend_args=None, filter_cfg=None, metainfo=None, lazy_init=False, serialize_data=True,
                 max_refetch=1000, return_classes=False):
        if backend_args is not None:
            raise NotImplementedError('backend_args: only local files are supported (backend_args=None)')
        if filter_cfg is not None:
            raise NotImplementedError('filter_cfg: the test datasets are not filtered (filter_cfg=None)')
        self.metainfo = dict(self.METAINFO)
        if metainfo:
            self.metainfo.update(metainfo)
        self.data_root = data_root or ''
        self.data_prefix = dict(data_prefix or dict(img=''))
        self.ann_file = ann_file if os.path.isabs(ann_file) or not self.data_root else os.path.join(self.data_root,
                                                                                                   ann_file)
        for k, v in self.data_prefix.items():
            if v and not os.path.isabs(v) and self.data_root:
                self.data_prefix[k] = os.path.join(self.data_root, v)
            elif not v:
                self.data_prefix[k] = self.data_root
        self.test_mode = test_mode
        self.pipeline = pipeline
        with open(self.ann_file) as f:
            self.coco = json.load(f)
        self._load()
        if indices is not None:
            keep = list(range(indices)) if isinstance(indices, int) else list(indices)
            self.data_list = [self.data_list[i] for i in keep]
        self._gt_cache = {}

    @property
    def dataset_meta(self):
        return self.metainfo

    def _load(self):
        classes = list(self.metainfo['classes'])
        cats = self.coco.get('categories', [])
        self.cat_ids = [c['id'] for c in cats if c['name'] in classes]          # COCO.getCatIds(catNms=...): JSON order
        self.cat2label = {cid: i for i, cid in enumerate(self.cat_ids)}
        anns_of = {}
        for ann in self.coco.get('annotations', []):
            anns_of.setdefault(ann['image_id'], []).append(ann)
        imgs = {}
        for im in self.coco.get('images', []):
            imgs[im['id']] = im                                                   # COCO.imgs: insertion order, last wins
        self.data_list = []
        for img_id, info in imgs.items():
            self.data_list.append(dict(img_path=os.path.join(self.data_prefix.get('img', ''), info['file_name']),
                                       img_id=img_id, height=info['height'], width=info['width'],
                                       raw_anns=anns_of.get(img_id, [])))

    def __len__(self):
        return len(self.data_list)

    def parse_instances(self, i):
        """parse_data_info's instance filter: list of dict(bbox xyxy, bbox_label, ignore_flag, mask)."""
        d = self.data_list[i]
        out = []
        for ann in d['raw_anns']:
            if ann.get('ignore', False):
                continue
            x1, y1, w, h = ann['bbox']
            inter_w = max(0, min(x1 + w, d['width']) - max(x1, 0))
            inter_h = max(0, min(y1 + h, d['height']) - max(y1, 0))
            if inter_w * inter_h == 0:
                continue
            if ann['area'] <= 0 or w < 1 or h < 1:
                continue
            if ann['category_id'] not in self.cat_ids:
                continue
            inst = dict(bbox=[x1, y1, x1 + w, y1 + h], bbox_label=self.cat2label[ann['category_id']],
                        ignore_flag=1 if ann.get('iscrowd', False) else 0)
            if ann.get('segmentation', None):
                inst['mask'] = ann['segmentation']
            out.append(inst)
        return out

    def ground_truth(self, i):
        """LoadAnnotations(with_bbox=True, with_mask=True) of item i (cached)."""
        g = self._gt_cache.get(i)
        if g is not None:
            return g
        d = self.data_list[i]
        h, w = d['height'], d['width']
        bboxes, labels, ignore, masks = [], [], [], []
        for inst in self.parse_instances(i):
            rle = gt_mask_rle(inst.get('mask', []), h, w)
            flag = inst['ignore_flag']
            if rle is None:
                flag = 1
                rle = dict(size=[h, w], counts=counts_to_string([h * w]))
            bboxes.append(inst['bbox'])
            labels.append(inst['bbox_label'])
            ignore.append(bool(flag))
            masks.append(rle)
        g = dict(bboxes=np.asarray(bboxes, dtype=np.float32).reshape(-1, 4), labels=np.asarray(labels, dtype=np.int64),
                 ignore_flags=np.asarray(ignore, dtype=bool), masks=masks)
        self._gt_cache[i] = g
        return g

    def __getitem__(self, i):
        d = self.data_list[i]
        out = dict(img_path=d['img_path'], img_id=d['img_id'], ori_shape=(d['height'], d['width']))
        out.update(self.ground_truth(i))
        return out


@DATASETS.register_module()
class NWPUInsSegDataset(CocoDataset):
    METAINFO = dict(classes=('airplane', 'ship', 'storage_tank', 'baseball_diamond', 'tennis_court', 'basketball_court',
                             'ground_track_field', 'harbor', 'bridge', 'vehicle'))


@DATASETS.register_module()
class WHUInsSegDataset(CocoDataset):
    METAINFO = dict(classes=('building',))


@DATASETS.register_module()
class SSDDInsSegDataset(CocoDataset):
    METAINFO = dict(classes=('ship',))
