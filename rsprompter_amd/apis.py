"""Caller APIs of the inference path: `init_detector`, `inference_detector` and a `DetInferencer`
with the reference's call surface, on top of a GPU front end for the test pipeline.

Reference: mmdet/apis/inference.py:31-119 (`init_detector`), :122-193 (`inference_detector`),
mmdet/apis/det_inferencer.py:298-417 (`DetInferencer.__call__`: chunked `preprocess -> forward -> postprocess`),
and the test pipeline every RSPrompter config declares (configs/rsprompter/_base_/rsprompter_anchor.py:231-241):
    LoadImageFromFile(to_float32=True) -> Resize(scale=crop_size, keep_ratio=True)
    -> Pad(size=crop_size, pad_val=dict(img=(0.406*255, 0.456*255, 0.485*255), masks=0)) -> [LoadAnnotations]
    -> PackDetInputs(meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor', ...))

What runs where: the image file is decoded on the host (PIL here; the reference decodes with cv2 -- decoders are not
part of the hot path and may differ by a grey level on some JPEG blocks); the decoded HWC array goes to the device as
uint8 and everything else -- float conversion, bilinear resize with cv2's INTER_LINEAR arithmetic, constant padding
-- is ONE kernel (`rsp_resize_pad`), after which `model.test_step` runs the existing DetDataPreprocessor kernel.
Annotation loading / visualisation are not part of the hot path and are skipped (a pipeline entry that is not one of
the transforms above and is not annotation-related raises).
"""
import copy
import os

import numpy as np
import torch

from . import ops, rle
from .config import Config
from .structures import DetDataSample, PixelData

_SKIPPED = ('LoadAnnotations', 'mmdet.LoadAnnotations')


def rescale_size(old_wh, scale):
    """mmcv.image.geometric.rescale_size (mmcv 2.1, the `Resize(keep_ratio=True)` path): the largest size that fits
    inside `scale` keeping the aspect ratio; mmcv rounds with +0.5 (`_scale_size`)."""
    w, h = old_wh
    if isinstance(scale, (int, float)):
        sf = float(scale)
    else:
        sf = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return (int(w * float(sf) + 0.5), int(h * float(sf) + 0.5)), sf


class TestPipeline:
    """The test pipeline as a device front end.  Built from the pipeline cfg list; callable on dict(img=ndarray) or
    dict(img_path=str) like mmcv's Compose; returns dict(inputs=fp32 [3, H, W] device tensor (BGR order, 0..255 range,
    exactly what PackDetInputs would hand on), data_samples=DetDataSample with the metainfo keys of `meta_keys`)."""

    def __init__(self, pipeline, device='cuda:0'):
        self.device = torch.device(device)
        self.scale, self.keep_ratio, self.pad_size, self.pad_val = None, True, None, (0.0, 0.0, 0.0)
        self.meta_keys = ('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor')
        self.to_float32 = False
        for t in pipeline:
            name = str(t['type']).split('.')[-1]
            if name in ('LoadImageFromFile', 'LoadImageFromNDArray', 'LoadImageFromWebcam'):
                self.to_float32 = bool(t.get('to_float32', False))
            elif name == 'Resize':
                self.scale, self.keep_ratio = tuple(t['scale']), bool(t.get('keep_ratio', False))
                if t.get('interpolation', 'bilinear') != 'bilinear' or t.get('backend', 'cv2') != 'cv2':
                    raise NotImplementedError('Resize: only cv2 bilinear (the mmcv default) is implemented')
            elif name == 'Pad':
                if t.get('size') is None or t.get('padding_mode', 'constant') != 'constant':
                    raise NotImplementedError('Pad: only a fixed `size` with constant padding is implemented')
                self.pad_size = tuple(t['size'])                      # (w, h)
                pv = t.get('pad_val', dict(img=0))
                pv = pv.get('img', 0) if isinstance(pv, dict) else pv
                self.pad_val = tuple(float(v) for v in pv) if isinstance(pv, (tuple, list)) else (float(pv),) * 3
            elif name == 'PackDetInputs':
                self.meta_keys = tuple(t.get('meta_keys', self.meta_keys))
            elif name in ('LoadAnnotations',):
                continue                                              # ground truth: not an input of predict
            else:
                raise NotImplementedError(f'test pipeline transform {t["type"]} is not implemented by the HIP front end')

    @staticmethod
    def _decode(path):
        from PIL import Image
        with Image.open(path) as im:
            rgb = np.asarray(im.convert('RGB'))
        return np.ascontiguousarray(rgb[:, :, ::-1])                  # BGR like cv2.imread / mmcv.imfrombytes

    def geometry(self, h, w):
        """resized size (nh, nw), padded size (ph, pw) and the shape metainfo the pipeline gives an [h, w] image"""
        if self.scale is not None:
            if self.keep_ratio:
                (nw, nh), _ = rescale_size((w, h), self.scale)
            else:
                nw, nh = int(self.scale[0]), int(self.scale[1])
        else:
            nw, nh = w, h
        pw, ph = self.pad_size if self.pad_size is not None else (nw, nh)
        pw, ph = max(pw, nw), max(ph, nh)                             # mmcv.impad never crops
        meta = dict(ori_shape=(h, w),
                    # Resize sets img_shape to the resized size, mmcv's Pad then overwrites it with the padded one
                    img_shape=(ph, pw) if self.pad_size is not None else (nh, nw),
                    scale_factor=(nw / w, nh / h), pad_shape=(ph, pw, 3), keep_ratio=self.keep_ratio)
        return nh, nw, ph, pw, meta

    def __call__(self, data):
        data = dict(data)
        img = data.get('img')
        if img is None:
            img = self._decode(data['img_path'])
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.ascontiguousarray(img))
        if img.dim() != 3 or img.shape[2] != 3:
            raise ValueError('expected an [H, W, 3] image')
        h, w = int(img.shape[0]), int(img.shape[1])
        dimg = img.to(self.device, non_blocking=True)
        nh, nw, ph, pw, meta = self.geometry(h, w)
        inputs = ops.resize_pad(dimg, (nh, nw), (ph, pw), self.pad_val)
        meta.update(img_id=data.get('img_id', 0), img_path=data.get('img_path'))
        sample = DetDataSample(metainfo={k: meta[k] for k in self.meta_keys if k in meta})
        return dict(inputs=inputs, data_samples=sample)


def get_test_pipeline_cfg(cfg):
    """mmdet/utils/misc.py::get_test_pipeline_cfg: the pipeline of the test dataloader's dataset."""
    ds = cfg['test_dataloader']['dataset']
    while 'dataset' in ds and 'pipeline' not in ds:
        ds = ds['dataset']
    return copy.deepcopy(ds['pipeline'])


def init_detector(config, checkpoint=None, palette='none', device='cuda:0', cfg_options=None):
    """mmdet/apis/inference.py:31-119: build the model of a config file (or Config), load a checkpoint, attach `cfg`,
    move to `device`, eval mode."""
    from . import build_model
    from .nnutil import load_checkpoint_into
    if isinstance(config, (str, os.PathLike)):
        config = Config.fromfile(str(config))
    elif not isinstance(config, dict):
        raise TypeError(f'config must be a filename or Config object, but got {type(config)}')
    if cfg_options is not None:
        config.merge_from_dict(cfg_options)
    # init_cfg of the sub-modules points at the pretrained SAM files; without them on disk the loaders are skipped
    model = build_model(config)
    if checkpoint is not None:
        load_checkpoint_into(model, checkpoint)
    model.cfg = config
    model.to(device)
    model.eval()
    return model


def inference_detector(model, imgs, test_pipeline=None, text_prompt=None, custom_entities=False):
    """mmdet/apis/inference.py:122-193: str / ndarray or a list of them -> DetDataSample (or a list of them)."""
    if text_prompt:
        raise NotImplementedError('text prompts belong to grounding detectors, not to RSPrompter')
    is_batch = isinstance(imgs, (list, tuple))
    if not is_batch:
        imgs = [imgs]
    if test_pipeline is None:
        dev = next(model.parameters()).device
        test_pipeline = TestPipeline(get_test_pipeline_cfg(model.cfg), device=dev)
    result_list = []
    for img in imgs:
        data_ = dict(img=img, img_id=0) if isinstance(img, (np.ndarray, torch.Tensor)) else dict(img_path=img, img_id=0)
        data_ = test_pipeline(data_)
        data_['inputs'] = [data_['inputs']]
        data_['data_samples'] = [data_['data_samples']]
        with torch.no_grad():
            result_list.append(model.test_step(data_)[0])
    return result_list if is_batch else result_list[0]


class DetInferencer:
    """mmdet/apis/det_inferencer.py: `DetInferencer(model=cfg_or_path, weights=..., device=...)(inputs, batch_size=1)`
    -> dict(predictions=[...], visualization=[]).  Inputs: path / ndarray / list of them / a directory.  Prediction
    dicts follow `pred2dict` (det_inferencer.py:573-627): labels, scores, bboxes (+ masks as COCO RLE)."""

    def __init__(self, model=None, weights=None, device='cuda:0', scope='mmdet', palette='none', show_progress=False):
        if isinstance(model, torch.nn.Module):
            self.model = model
        else:
            self.model = init_detector(model, weights, device=device)
        self.pipeline = TestPipeline(get_test_pipeline_cfg(self.model.cfg), device=next(self.model.parameters()).device)

    @staticmethod
    def _inputs_to_list(inputs):
        if isinstance(inputs, str) and os.path.isdir(inputs):
            exts = ('.jpg', '.jpeg', '.png', '.bmp', '.tif', '.tiff')
            return [os.path.join(inputs, f) for f in sorted(os.listdir(inputs)) if f.lower().endswith(exts)]
        return list(inputs) if isinstance(inputs, (list, tuple)) else [inputs]

    def pred2dict(self, sample, with_rle=True):
        """labels / scores / bboxes as lists (+ masks as COCO RLE) when the sample has `pred_instances` -- a detector with the
        reference's default test_cfg (panoptic_on, no instance_on) has none --, and `panoptic_seg` when it has
        `pred_panoptic_seg`: unlike the lists, that entry is the PixelData itself with its device tensors, untouched (mmdet
        writes a PNG there, which is not built; `panoptic_to_coco` turns it into the image and segments_info)."""
        from .rle import encode_mask_results
        out = {}
        p = sample.get('pred_instances')
        if p is not None:
            out.update(labels=p.labels.tolist(), scores=p.scores.tolist(), bboxes=p.bboxes.tolist())
            if with_rle and hasattr(p, 'masks') and p.masks is not None:
                out['masks'] = encode_mask_results(p.masks) if len(p.labels) else []
        if sample.get('pred_panoptic_seg') is not None:
            out['panoptic_seg'] = sample.pred_panoptic_seg
        return out

    @torch.no_grad()
    def __call__(self, inputs, batch_size=1, return_datasamples=False, no_save_pred=True, **kwargs):
        items = self._inputs_to_list(inputs)
        preds = []
        for i in range(0, len(items), batch_size):
            chunk = [self.pipeline(dict(img=x, img_id=i + j) if isinstance(x, (np.ndarray, torch.Tensor))
                                   else dict(img_path=x, img_id=i + j)) for j, x in enumerate(items[i:i + batch_size])]
            data = dict(inputs=[c['inputs'] for c in chunk], data_samples=[c['data_samples'] for c in chunk])
            for s in self.model.test_step(data):
                preds.append(s if return_datasamples else self.pred2dict(s))
        return dict(predictions=preds, visualization=[])


from .large_image import inference_large_image  # noqa: E402,F401  (sliced inference on large scenes)
from .sam_prompts import PerSam, PerSamF, SamMaskGenerator, SamSession, generate_masks, inference_prompts  # noqa: E402,F401  (promptable SAM)
from .samdet import SamHQModelHIP  # noqa: E402,F401  (HF SamHQModel on HIP kernels, DESIGN §15 "SAM-HQ")


def remove_small_regions(masks, min_area, mode='both', device='cuda:0'):
    """segment-anything's `remove_small_regions` for masks that come from elsewhere (`SamSession.predict`,
    `PerSam(output='dense')`, a detector's results): masks bool / uint8 [k, H, W] or [H, W] on the device; mode 'holes'
    (8-connected components of the background with fewer than min_area pixels are filled), 'islands' (components of the mask
    that small are removed; if all are, the largest stays) or 'both' (holes first).  Returns (masks bool of the input's
    shape, changed bool [k] or a bool).  One host read (the labelling's status).
    masks may also be a list of RLE dicts dict(size=[H, W], counts=...) of one size, compressed (bytes / str) or uncompressed
    (list) counts, canonical ones (rle.masks_to_runs): they are cleaned in the run domain (rle.clean_runs, DESIGN §14.10;
    `device` places the run table) and come back as (RLE dicts of the input's counts form, changed bool [k] on the host)."""
    if not isinstance(masks, torch.Tensor):
        counts, n, size, form = rle.masks_to_runs(masks, device, 'remove_small_regions', canonical=True)
        counts, n, n_host, _, changed = rle.clean_runs(counts, n, size, min_area, mode)
        return rle.runs_to_masks(counts, n, size, form, n_host), (changed != 0).any(1).cpu()
    single = masks.dim() == 2
    out, info = ops.remove_small_regions(masks[None] if single else masks, min_area, mode)
    ops.check_region_status(info[:, 7].cpu().tolist())
    changed = (info[:, 0] | info[:, 1]) != 0
    return (out[0], bool(changed[0])) if single else (out, changed)


# ------------------------------------------------------------------------------------------ run-domain IoU
def _iou_sides(dt, gt, iscrowd, device, what):
    """what mask_iou and boundary_iou do before their kernels: both sides as run tables, the refusals, the one unit of D x G
    pairs and the crowd flags -> ((dt counts, n), (gt counts, n), D, G, the common size or None, units, g_crowd)"""
    for t in (dt, gt):
        if isinstance(t, torch.Tensor):
            device = t.device
    dc, dn, d_sizes, _ = rle.masks_to_runs(dt, device, what, one_size=False)
    gc, gn, g_sizes, _ = rle.masks_to_runs(gt, device, what, one_size=False)
    D, G = len(d_sizes), len(g_sizes)
    sizes = set(d_sizes) | set(g_sizes)
    if D and G and len(sizes) != 1:
        raise ValueError(f'{what}: masks of different sizes in one call: {sorted(sizes)}')
    crowd = np.zeros(G, np.uint8) if iscrowd is None else np.asarray(list(iscrowd)).astype(bool).astype(np.uint8).reshape(-1)
    if crowd.shape[0] != G:
        raise ValueError(f'{what}: iscrowd has {crowd.shape[0]} entries for {G} ground truths')
    units = ops.coco_units([0], [0], [0], [D], [G], [0], dn.device)
    g_crowd = torch.from_numpy(np.concatenate([crowd, [0]]).astype(np.uint8)).to(dn.device)
    return (dc, dn), (gc, gn), D, G, sizes.pop() if D and G else None, units, g_crowd


def mask_iou(dt, gt, iscrowd=None, device='cuda:0'):
    """pycocotools' `maskUtils.iou(dt, gt, iscrowd)` on the device, in the run domain: float64 [D, G] (on the device), entry
    (d, g) = |d & g| / |d | g|, or / |d| for a crowd g, 0.0 without a common pixel (csrc/coco_iou_runs.hip).
    dt / gt: lists of RLE dicts dict(size=[H, W], counts=...) -- compressed (bytes / str) or uncompressed (list) counts,
    also side by side, any counts that sum to the canvas (zero counts anywhere) -- or bool [k, H, W] tensors on the device.
    No mask is expanded: scene-sized RLE costs its runs.  iscrowd: a bool per gt (None: none is).  Masks of different sizes
    in one call are refused (ValueError; cocoapi writes -1 there).  One device-to-host read (the pairs whose extents
    overlap), and the run capacity retry of bool tensors / compressed strings."""
    d_runs, g_runs, D, G, _, units, g_crowd = _iou_sides(dt, gt, iscrowd, device, 'mask_iou')
    return ops.coco_iou_runs(units, D * G, d_runs, g_runs, g_crowd).view(D, G)


# --------------------------------------------------------------------------------------- morphology, Boundary IoU
MORPHOLOGY_OPS = ('erode', 'dilate', 'open', 'close', 'boundary')


def _morph_radius(radius):
    if isinstance(radius, bool) or int(radius) != radius or int(radius) < 0:
        raise ValueError(f'radius must be a non-negative integer, got {radius!r}')
    return int(radius)


MORPHOLOGY_ELEMENTS = rle.MORPHOLOGY_ELEMENTS


def _morph_element(what, element, radius):
    """element and its radius: an integer for the square and the diamond, a non-negative real number for the disc"""
    if element not in MORPHOLOGY_ELEMENTS:
        raise ValueError(f'{what}: element must be one of {MORPHOLOGY_ELEMENTS}, got {element!r}')
    if element != 'disc':
        return _morph_radius(radius)
    rle.disc_r2(radius)                                     # refuses what is not a non-negative finite real number
    return radius


def _morphology(masks, op, radius, device, what, element='square'):
    fn = dict(erode=rle.erode_runs, dilate=rle.dilate_runs, open=rle.open_runs, close=rle.close_runs,
              boundary=rle.boundary_runs, buffer=rle.buffer_runs)[op]
    if isinstance(masks, torch.Tensor) and masks.dim() == 3 and masks.shape[0] == 0:
        return masks.to(torch.bool).clone()
    counts, n, size, form = rle.masks_to_runs(masks, device, what)
    counts, n, n_host, _ = fn(counts, n, size, radius, **({} if element == 'square' else dict(element=element)))
    return rle.runs_to_masks(counts, n, size, form, n_host)


def buffer_masks(masks, distance, device='cuda:0'):
    """The GIS buffer in the run domain (csrc/run_disc.hip): distance > 0 grows every mask to the pixels whose
    Euclidean distance to it is at most `distance` (the exact disc dx^2 + dy^2 <= floor(distance^2), clipped to the canvas);
    distance < 0 shrinks it to the pixels farther than |distance| from its outside, the outside of the canvas counting as set
    (the edge of a scene is not an object boundary) -- the usual way to pull touching footprints apart; 0 returns the masks
    in canonical form.  distance is a real number in pixels (metres divided by the pixel size), squared in exact arithmetic.
    Input and output forms as mask_morphology's; no mask is expanded."""
    rle._exact_fraction(distance, 'buffer_masks: distance')
    return _morphology(masks, 'buffer', distance, device, 'buffer_masks')


def mask_morphology(masks, op, radius, device='cuda:0', element='square'):
    """Morphology by the (2 radius + 1)^2 square in the run domain (csrc/run_morphology.hip): op 'erode'
    (outside the canvas counts as background), 'dilate', 'open' (erode, then dilate), 'close' (dilate, then erode with the
    outside set) or 'boundary' (the mask minus its erosion) -- cv2.erode / cv2.dilate / cv2.morphologyEx with a square kernel,
    scipy.ndimage.binary_erosion(M, ones((3, 3)), iterations=radius).  masks: bool [k, H, W] on the device -> bool [k, H, W];
    or a list of RLE dicts dict(size=[H, W], counts=...) of one size, compressed (bytes / str) or uncompressed (list) ->
    RLE dicts of the same counts form, never a dense mask (`device` places the run table); the cost is the masks' column
    pieces times log radius.  element (MORPHOLOGY_ELEMENTS): 'square'; 'disc', the exact Euclidean disc dx^2 + dy^2 <=
    floor(radius^2), radius a non-negative real number (scipy.ndimage with that footprint, the distance transform thresholded;
    not cv2's MORPH_ELLIPSE); 'diamond', |dx| + |dy| <= radius (csrc/run_disc.hip, DESIGN §14.16: the cost grows linearly
    with the radius, never with the area)."""
    if op not in MORPHOLOGY_OPS:
        raise ValueError(f'mask_morphology: op must be one of {MORPHOLOGY_OPS}, got {op!r}')
    return _morphology(masks, op, _morph_element('mask_morphology', element, radius), device, 'mask_morphology', element)


def mask_boundary(masks, dilation_ratio=0.02, radius=None, device='cuda:0', element='square'):
    """The boundary band of Boundary IoU (Cheng et al., CVPR 2021; boundary-iou-api mask_to_boundary): the pixels of each
    mask within d of its outline or of the image border, d = rle.boundary_radius(size, dilation_ratio) = max(1, round(ratio *
    diagonal)) or `radius` when given.  Input and output forms as mask_morphology's.  element: as mask_morphology's (the
    published metric is the square)."""
    if element not in MORPHOLOGY_ELEMENTS:
        raise ValueError(f'mask_boundary: element must be one of {MORPHOLOGY_ELEMENTS}, got {element!r}')
    if radius is None:
        size = tuple(masks.shape[1:]) if isinstance(masks, torch.Tensor) else None
        if size is None:
            masks = list(masks)
            if not masks:
                raise ValueError('mask_boundary: an empty list carries no canvas size; pass a bool [0, H, W] tensor instead')
            size = masks[0]['size']
        radius = rle.boundary_radius(size, dilation_ratio)
    return _morphology(masks, 'boundary', _morph_element('mask_boundary', element, radius), device, 'mask_boundary', element)


def boundary_iou(dt, gt, iscrowd=None, dilation_ratio=0.02, radius=None, min_with_mask=False, device='cuda:0'):
    """Boundary IoU of every pair: mask_iou of the boundary bands (mask_boundary) -> float64 [D, G] on the device, with the
    inputs, conventions and refusals of mask_iou (0.0 without a common band pixel, / |dt band| for a crowd gt, masks of
    different sizes refused).  min_with_mask=True returns min(mask IoU, boundary IoU), what Boundary AP matches with."""
    d_runs, g_runs, D, G, size, units, g_crowd = _iou_sides(dt, gt, iscrowd, device, 'boundary_iou')
    if not (D and G):
        return torch.zeros((D, G), dtype=torch.float64, device=g_crowd.device)
    r = rle.boundary_radius(size, dilation_ratio) if radius is None else _morph_radius(radius)
    db, gb = rle.boundary_runs(*d_runs, size, r)[:2], rle.boundary_runs(*g_runs, size, r)[:2]
    out = ops.coco_iou_runs(units, D * G, db, gb, g_crowd)
    if min_with_mask:
        out = torch.minimum(out, ops.coco_iou_runs(units, D * G, d_runs, g_runs, g_crowd))
    return out.view(D, G)


# ------------------------------------------------------------------------------------------ planar layers
def _flatten(masks, scores, order, min_ratio, device, what):
    """masks in the forms of rle.masks_to_runs -> (flattened counts, n, size, the form they came in, info)"""
    rle._flatten_min_ratio(min_ratio)
    if isinstance(masks, torch.Tensor):
        device = masks.device
    counts, n, size, came = rle.masks_to_runs(masks, device, what, canonical=False)
    k = int(n.shape[0])
    areas = ops.rle_bbox(counts, n, size[0], size[1])[1] if isinstance(order, str) and order == 'area' else None
    rank = rle.flatten_rank(k, order, scores, areas)
    counts, n, _, before, after, kept = rle.flatten_runs(counts, n, size, rank, min_ratio)
    return counts, n, size, came, dict(area_before=before, area_after=after, kept=kept, rank=rank)


def flatten_masks(masks, scores=None, order='score', min_ratio=0.0, form=None, device='cuda:0'):
    """Overlapping instances -> a planar layer: every pixel stays with ONE of the instances that cover it, the one of highest
    priority, so the results are pairwise disjoint and their union is the union of the inputs (csrc/run_flatten.hip, DESIGN
    §14.14) -- the per-pixel argmax of score x mask of MaskFormerFusionHead.panoptic_postprocess for binary masks, in the run
    domain: no mask is expanded.  masks: bool [k, H, W] on the device, or a list of RLE dicts dict(size=[H, W], counts=...) of
    one size, compressed (bytes / str) or uncompressed (list) counts, zero counts anywhere allowed (`device` places the run
    table).  order='score': the higher of `scores` wins, ties to the lower index (NaN refused); 'area': the smaller mask wins
    (the usual way to paint SAM's everything output), ties to the lower index; or an explicit rank, a permutation of 0 ..
    k - 1 where 0 wins.  min_ratio in [0, 1]: an instance that keeps less than that share of its pixels is emptied after the
    partition is made (its pixels go to nobody; float64 comparison, rle.flatten_runs).
    -> (masks, info): the masks in the form they came in, or form='rle' (compressed dicts) | 'runs' ((counts, n) on the
    device) | 'dense' (bool [k, H, W], refused above large_image.DENSE_MASK_LIMIT_BYTES); an emptied instance is an empty
    mask.  info = dict(area_before int32 [k], area_after int32 [k], kept bool [k] (device tensors), rank int32 numpy [k])."""
    if form is not None and form not in MASK_FORMS:
        raise ValueError(f'mask form {form!r}: one of {MASK_FORMS}')
    counts, n, size, came, info = _flatten(masks, scores, order, min_ratio, device, 'flatten_masks')
    if form == 'runs':
        return (counts, n), info
    out_form = came if form is None else 'strings' if form == 'rle' else 'dense'
    if out_form == 'dense' and came != 'dense':
        from .large_image import _check_dense
        _check_dense(int(n.shape[0]), size[0], size[1])
    return rle.runs_to_masks(counts, n, size, out_form), info


def masks_to_label_map(masks, scores=None, order='score', ids=None, min_ratio=0.0, device='cuda:0'):
    """Overlapping instances -> an instance-id raster: int32 [H, W] on the device, ids[i] (i + 1 when None) where instance i
    wins under flatten_masks' rules (same masks, scores, order and min_ratio), 0 for the background and for the pixels of an
    instance that min_ratio emptied.  Painted from the flattened run table (rle.runs_to_labels); 4 bytes per pixel, refused
    above large_image.DENSE_MASK_LIMIT_BYTES."""
    from .large_image import DENSE_MASK_LIMIT_BYTES
    if isinstance(masks, torch.Tensor):
        H, W = (int(s) for s in masks.shape[-2:])
    else:
        masks = list(masks)
        if not masks:
            raise ValueError('masks_to_label_map: an empty list carries no canvas size; pass a bool [0, H, W] tensor instead')
        H, W = int(masks[0]['size'][0]), int(masks[0]['size'][1])
    need = 4 * H * W
    if need > DENSE_MASK_LIMIT_BYTES:
        raise ValueError(f'a label map of a {H} x {W} scene needs {need} bytes (limit large_image.DENSE_MASK_LIMIT_BYTES = '
                         f'{DENSE_MASK_LIMIT_BYTES}): use flatten_masks(form="rle")')
    counts, n, size, _, _ = _flatten(masks, scores, order, min_ratio, device, 'masks_to_label_map')
    return rle.runs_to_labels(counts, n, size, ids)


# ------------------------------------------------------------------------------------------ polygon export
POLYGON_FORMS =('rings', 'coco', 'geojson')


def rings_to_coco(rings):
    """the rings of ONE instance -> (list of flat float lists [x0, y0, x1, y1, ...] of its OUTER rings, holes_dropped): COCO
    polygons cannot express holes, so the polygons describe the hole-filled mask and the flag says that holes were there"""
    polys = [[float(c) for c in ring.reshape(-1).tolist()] for ring, parent, area2 in rings if area2 > 0]
    return polys, any(area2 < 0 for _, _, area2 in rings)


def rings_to_geojson(rings, transform=None):
    """the rings of ONE instance -> a GeoJSON geometry dict: a Polygon for one outer ring, a MultiPolygon for several (or
    none); every polygon = [outer, hole, ...] with the holes attached by `parent`, every ring closed by repeating its first
    vertex.  transform = (a, b, c, d, e, f): pixel corner (x, y) -> (a + b x + c y, d + e x + f y), float64 on the host."""
    def coords(ring):
        xy = np.asarray(ring, np.float64).reshape(-1, 2)
        if transform is not None:
            a, b, c, d, e, f = (float(t) for t in transform)
            xy = np.stack([a + b * xy[:, 0] + c * xy[:, 1], d + e * xy[:, 0] + f * xy[:, 1]], 1)
        xy = np.concatenate([xy, xy[:1]], 0)
        return [[float(x), float(y)] for x, y in xy.tolist()]
    polys = {}
    for r, (ring, parent, area2) in enumerate(rings):
        if area2 > 0:
            polys[r] = [coords(ring)]
    for ring, parent, area2 in rings:
        if area2 < 0:
            polys[parent].append(coords(ring))
    polys = [polys[r] for r in sorted(polys)]
    if len(polys) == 1:
        return dict(type='Polygon', coordinates=polys[0])
    return dict(type='MultiPolygon', coordinates=polys)


def format_polygons(per_instance, form='rings', transform=None):
    """per-instance ring lists (rle.polygons_to_lists) in one of POLYGON_FORMS"""
    if form == 'rings':
        return per_instance
    if form == 'coco':
        out = [rings_to_coco(r) for r in per_instance]
        return [dict(polygons=p, holes_dropped=h) for p, h in out]
    if form == 'geojson':
        return [rings_to_geojson(r, transform) for r in per_instance]
    raise ValueError(f'polygon form {form!r}: one of {POLYGON_FORMS}')


def masks_to_polygons(masks, form='rings', transform=None, device='cuda:0', tolerance=None, min_ring_area=0,
                      topology='rings'):
    """Masks -> exact vector rings on the pixel-corner lattice, traced on the device in the run domain.
    masks: a bool [k, H, W] device tensor, or a list of RLE dicts dict(size=[H, W], counts=...) of one size with compressed
    counts (bytes / str, what `encode_mask_results` returns) or uncompressed ones (list, what `generate_masks` returns);
    `device` places the run table of the dict forms.
    form='rings': per instance a list of (ring int32 ndarray [m, 2] = (x, y), parent, area2): corners only, clockwise on
      screen (area2 > 0) for outer rings and counter-clockwise (area2 < 0) for holes, from the ring's smallest vertex on,
      first vertex not repeated, ordered by first vertex; parent = the outer ring around a hole, -1 for outer rings.
      Foreground is 8-connected, background 4-connected (cv2.findContours' connectivity).
    form='coco': per instance dict(polygons=[[x0, y0, x1, y1, ...], ...] of the OUTER rings only, holes_dropped=bool).
    form='geojson': per instance a Polygon / MultiPolygon geometry dict with the holes attached; `transform` = (a, b, c, d, e,
      f) maps pixel corners to X = a + b x + c y, Y = d + e x + f y.
    tolerance (pixels; None: the exact rings) simplifies every ring on the device by Douglas-Peucker before
      it reaches the host: a dropped vertex lies within `tolerance` of the kept outline; rings are simplified independently
      (they may then cross); rings of less than min_ring_area pixels, rings that collapse, and the holes of a dropped outer
      ring are dropped -- a dropped hole is filled.  Both apply to all three forms; min_ring_area alone (tolerance=None)
      filters at tolerance 0, which keeps every vertex of the rings that stay.
    topology='shared' (the masks must be pairwise disjoint, what flatten_masks returns, and min_ring_area 0;
      a tolerance is required, 0 is legal): a border between two instances is simplified once, to the same vertices in both
      rings, so neighbouring features share their border coordinates exactly -- no gaps, no slivers.  Every node (a T-junction,
      a point where three or four regions or two and the canvas border meet, a saddle) becomes a vertex, also on a straight
      wall, and a ring begins at its first node, not at its smallest vertex.  Different borders may still cross each other
      at large tolerances.  Overlapping masks are refused."""
    if form not in POLYGON_FORMS:
        raise ValueError(f'polygon form {form!r}: one of {POLYGON_FORMS}')
    if transform is not None and form != 'geojson':
        raise ValueError("transform applies to form='geojson' only")
    if rle.polygon_topology(topology, tolerance, min_ring_area):        # refused before anything runs
        counts, n, size, _ = rle.masks_to_runs(masks, device, 'masks_to_polygons', canonical=True)
        polys, _, _ = rle.simplify_coverage(counts, n, size, tolerance)
        return format_polygons(rle.polygons_to_lists(*polys), form, transform)
    simplify = tolerance is not None or min_ring_area != 0
    if simplify:                                                        # refused before anything runs
        rle.polygon_tolerance_q8(0 if tolerance is None else tolerance)
        rle.polygon_min_ring_area(min_ring_area)
    counts, n, size, _ = rle.masks_to_runs(masks, device, 'masks_to_polygons', canonical=True)
    polys = rle.runs_to_polygons(counts, n, size)
    if simplify:
        polys, _ = rle.simplify_polygons(polys, size, 0 if tolerance is None else tolerance, min_ring_area)
    return format_polygons(rle.polygons_to_lists(*polys), form, transform)


# --------------------------------------------------------------------------------------- polygon rasterisation
MASK_FORMS = ('rle', 'runs', 'dense')


def invert_transform(transform):
    """the inverse of rings_to_geojson's forward transform (a, b, c, d, e, f): a function float64 [m, 2] world -> pixel corners,
    x = (f (X - a) - c (Y - d)) / det, y = (b (Y - d) - e (X - a)) / det with det = b f - c e, in float64 on the host (exact
    for power-of-two scales without rotation); a singular transform raises"""
    a, b, c, d, e, f = (float(t) for t in transform)
    det = b * f - c * e
    if not np.isfinite(det) or det == 0.0:
        raise ValueError(f'transform {tuple(transform)!r} is singular (b f - c e = {det}): it cannot be inverted')

    def back(xy):
        X, Y = xy[:, 0] - a, xy[:, 1] - d
        return np.stack([(f * X - c * Y) / det, (b * Y - e * X) / det], 1)
    return back


def _instance_rings(inst):
    """one instance of polygons_to_masks -> (list of float64 [m, 2] rings, the default fill of its form)"""
    def ring(p):
        return np.asarray(p, np.float64).reshape(-1, 2)
    if isinstance(inst, dict):
        if 'polygons' in inst:                                          # masks_to_polygons(form='coco')
            return _instance_rings(list(inst['polygons']))
        kind = inst.get('type')
        if kind not in ('Polygon', 'MultiPolygon'):
            raise ValueError(f"polygons_to_masks: a dict is the dict(polygons=...) of form='coco' or a GeoJSON Polygon / "
                             f'MultiPolygon geometry, got type {kind!r}')
        polys = [inst['coordinates']] if kind == 'Polygon' else list(inst['coordinates'])
        rings = []
        for poly in polys:
            for r in poly:                                              # outer ring and holes alike: the fill rule tells them apart
                r = ring(r)
                if len(r) > 1 and (r[0] == r[-1]).all():                # GeoJSON closes a ring by repeating its first vertex
                    r = r[:-1]
                rings.append(r)
        return rings, 'evenodd'
    inst = list(inst)
    if inst and isinstance(inst[0], (tuple, list)) and len(inst[0]) == 3 and np.ndim(inst[0][0]) == 2:
        return [ring(r[0]) for r in inst], 'evenodd'                    # masks_to_polygons(form='rings')
    if inst and not isinstance(inst[0], (list, tuple, np.ndarray)):
        inst = [inst]                                                   # one flat COCO polygon
    from .datasets import bbox_polygon
    return [ring(bbox_polygon(p) if len(p) == 4 else list(p)[:2 * (len(p) // 2)]) for p in inst], 'union'


def polygons_to_masks(polygons, size, form='rle', fill=None, transform=None, device='cuda:0'):
    """Vector instances -> masks on one size = (H, W) canvas, rasterised on the device exactly as cocoapi's rleFrPoly does it
    (DESIGN §14.11); the reverse of masks_to_polygons.  polygons: one entry per instance, each
      a COCO polygon list [[x0, y0, x1, y1, ...], ...] or one flat list; a 4-number entry is an xywh box, as in ann_to_rle;
      the dict(polygons=...) of masks_to_polygons(form='coco');
      the [(ring [m, 2], parent, area2), ...] list of form='rings';
      a GeoJSON Polygon / MultiPolygon geometry dict (the closing vertex of every ring is dropped).
    fill='union': every ring on its own, then their union (pycocotools' annToRLE; bit-equal to datasets.ann_to_rle);
      'evenodd': the rings of an instance together, holes subtract (the exact inverse of masks_to_polygons).  None: 'union'
      for COCO lists, 'evenodd' for rings and GeoJSON; instances of both kinds in one call need an explicit fill.
    transform = (a, b, c, d, e, f): the FORWARD transform of rings_to_geojson, X = a + b x + c y, Y = d + e x + f y; the
      coordinates are taken back to pixels with its inverse, in float64 on the host.
    form='rle': list of dict(size=[H, W], counts=bytes), what every run-domain API here takes; 'runs': (counts int32
      [k, cap], n int32 [k]) on the device; 'dense': bool [k, H, W] on the device (refused above
      large_image.DENSE_MASK_LIMIT_BYTES)."""
    if form not in MASK_FORMS:
        raise ValueError(f'mask form {form!r}: one of {MASK_FORMS}')
    if fill is not None and fill not in rle.POLYGON_FILLS:
        raise ValueError(f'polygon fill {fill!r}: one of {rle.POLYGON_FILLS}')
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f'polygons_to_masks: a {H} x {W} canvas: both sides at least 1 and fewer than 2^31 pixels')
    back = invert_transform(transform) if transform is not None else None
    per = [_instance_rings(p) for p in polygons]
    k = len(per)
    if form == 'dense':
        from .large_image import _check_dense
        _check_dense(k, H, W)
    if fill is None:
        kinds = {d for rings, d in per if rings}
        if len(kinds) > 1:
            raise ValueError("polygons_to_masks: COCO lists (fill 'union') and rings / GeoJSON (fill 'evenodd') in one call: "
                             'pass fill=')
        fill = kinds.pop() if kinds else 'union'
    rings = [r if back is None else back(r) for rs, _ in per for r in rs]
    dev = torch.device(device)
    ops.require_device(dev)
    offs = np.cumsum([0] + [len(r) for r in rings]).astype(np.int64)
    verts = np.concatenate(rings + [np.zeros((0, 2))]).reshape(-1, 2)
    if not np.isfinite(verts).all():
        raise ValueError('polygons_to_masks: a coordinate is NaN or infinite')
    group = np.repeat(np.arange(k, dtype=np.int32), [len(rs) for rs, _ in per])
    counts, n = rle.polygons_to_runs(torch.from_numpy(verts).to(dev), torch.from_numpy(offs).to(dev),
                                     torch.from_numpy(group).to(dev),
                                     torch.tensor([[H, W]] * k, dtype=torch.int32, device=dev).view(k, 2), fill=fill)
    if form == 'runs':
        return counts, n
    return rle.runs_to_masks(counts, n, (H, W), 'strings' if form == 'rle' else 'dense')


# ------------------------------------------------------------------------------------------- oriented boxes
OBB_FORMS =('corners', 'xywha', 'hull', 'geojson')


def _affine(xy, transform):
    """float64 [..., 2] pixel coordinates through transform = (a, b, c, d, e, f) of rings_to_geojson"""
    if transform is None:
        return xy
    a, b, c, d, e, f = (float(t) for t in transform)
    return np.stack([a + b * xy[..., 0] + c * xy[..., 1], d + e * xy[..., 0] + f * xy[..., 1]], -1)


def obb_to_geojson(corners, transform=None):
    """float64 [k, 4, 2] corners -> per box a GeoJSON Polygon of the closed rectangle (an empty mask: no coordinates)"""
    out = []
    for c in _affine(np.asarray(corners, np.float64), transform):
        if np.isnan(c).any():
            out.append(dict(type='Polygon', coordinates=[]))
        else:
            out.append(dict(type='Polygon', coordinates=[[[float(x), float(y)] for x, y in c.tolist() + c[:1].tolist()]]))
    return out


def masks_to_obb(masks, form='corners', transform=None, device='cuda:0', per_component=False):
    """Masks -> oriented boxes: the minimum-area rectangle around each mask (all its components together), exact on the
    device in the run domain; what cv2.convexHull + cv2.minAreaRect give on a dense mask.  `masks`: a
    bool [k, H, W] device tensor, or RLE dicts of one size with compressed or uncompressed canonical counts (rle.masks_to_runs).
    form='corners': float64 [k, 4, 2], the corners in pixel-corner coordinates (pixel (x, y) covers [x, x + 1] x [y, y + 1]),
      clockwise on screen, the first side on a hull edge; NaN rows for empty masks.
    form='xywha': float64 [k, 5] = centre x, y, w >= h, angle of the w side in radians from +x towards +y in [-pi / 2, pi / 2).
    form='hull': per instance the int32 [m, 2] hull vertices, clockwise on screen from the smallest by (x, y).
    form='geojson': per instance a Polygon geometry of the closed rectangle.
    transform = (a, b, c, d, e, f) maps X = a + b x + c y, Y = d + e x + f y for 'corners' and 'geojson'; it is refused with
      'xywha' (an affine map does not keep rectangles) and 'hull' (integer vertices).
    per_component=True: a list with one entry per instance, holding in the same form the boxes or hulls of its 8-connected
      components in component order (rle.split_runs); an empty mask has an empty entry."""
    if form not in OBB_FORMS:
        raise ValueError(f'oriented-box form {form!r}: one of {OBB_FORMS}')
    if transform is not None and form not in ('corners', 'geojson'):
        raise ValueError("transform applies to form='corners' and form='geojson' only: an affine map does not keep the "
                         "rectangle of 'xywha'")
    counts, n, size, _ = rle.masks_to_runs(masks, device, 'masks_to_obb', canonical=True)
    if per_component:                                                   # one row per component, regrouped below
        counts, n, _, _, comp_offs = rle.split_runs(counts, n, size)
        co = comp_offs.tolist()
    hull_verts, hull_offs, _, edge, q = rle.runs_to_obb(counts, n, size)
    if form == 'hull':
        sizes = [int(hull_verts.numel()), int(hull_offs.numel())]
        buf = torch.cat([hull_verts.reshape(-1).to(torch.int64), hull_offs]).cpu().numpy()          # one transfer
        v, o = np.split(buf, sizes[:1])
        v, o = v.astype(np.int32).reshape(-1, 2), o.tolist()
        out = [v[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    elif form == 'xywha':
        out = rle.obb_to_numpy(edge, q, 'xywha')
    else:
        corners = rle.obb_to_numpy(edge, q, 'corners')
        out = obb_to_geojson(corners, transform) if form == 'geojson' else _affine(corners, transform)
    return [out[co[i]:co[i + 1]] for i in range(len(co) - 1)] if per_component else out


def xywha_to_corners(xywha):
    """float64 [k, 5] = (cx, cy, w, h, angle) in the convention rle.obb_to_numpy(form='xywha') writes (angle of the w side in
    radians from +x towards +y) -> float64 numpy [k, 4, 2], corners clockwise on screen from (-w / 2, -h / 2) in the box's
    frame.  Made on the host in float64: one cos / sin away from exact, where the corner form of a mask's rectangle is one
    division away."""
    b = np.asarray(xywha, np.float64).reshape(-1, 5)
    ux, uy = np.cos(b[:, 4]), np.sin(b[:, 4])
    hw, hh = b[:, 2] / 2, b[:, 3] / 2
    sa, sb = np.array([-1.0, 1.0, 1.0, -1.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    x = b[:, None, 0] + sa * (hw * ux)[:, None] - sb * (hh * uy)[:, None]
    y = b[:, None, 1] + sa * (hw * uy)[:, None] + sb * (hh * ux)[:, None]
    return np.stack([x, y], 2)


def _as_obb_corners(boxes, device, who):
    """oriented boxes in any accepted form -> float64 [k, 4, 2] on `device`: corners [k, 4, 2], xywha [k, 5] (tensor, array or
    nested list), or masks in the forms of masks_to_obb (a bool [k, H, W] device tensor, RLE dicts of one size), reduced to
    their rectangles on the device"""
    dev = torch.device(device)
    masks = (isinstance(boxes, torch.Tensor) and boxes.dtype == torch.bool) or \
        (isinstance(boxes, (list, tuple)) and len(boxes) > 0 and isinstance(boxes[0], dict))
    if masks:
        counts, n, size, _ = rle.masks_to_runs(boxes, dev, who, canonical=True)
        return rle.runs_to_obb_corners(counts, n, size)
    if isinstance(boxes, torch.Tensor) and boxes.dtype == torch.float64 and boxes.device == dev and boxes.dim() == 3 \
            and tuple(boxes.shape[1:]) == (4, 2):
        return boxes.contiguous()                                       # corners on the device already: no copy, no read
    t = boxes.detach().to(torch.float64).cpu().numpy() if isinstance(boxes, torch.Tensor) else np.asarray(boxes, np.float64)
    if t.size == 0 and t.ndim < 3:
        t = t.reshape(0, 4, 2)
    if t.ndim == 2 and t.shape[1] == 5:
        t = xywha_to_corners(t)
    if t.ndim != 3 or t.shape[1:] != (4, 2):
        raise ValueError(f'{who}: oriented boxes are corners [k, 4, 2], xywha [k, 5] or masks; got an array of shape '
                         f'{tuple(t.shape)}')
    return torch.from_numpy(np.ascontiguousarray(t)).to(dev)


def obb_iou(a, b, iscrowd=None, device='cuda:0'):
    """The IoU of every oriented box of `a` with every one of `b` -> float64 [D, G] on the device (ops.obb_iou, DESIGN
    §14.17): inter / union in fp64 with the intersection clipped as a closed polygon; a column g with iscrowd[g] set holds
    inter / area(a[d]), as COCO's crowd regions.  `a`, `b`: corners [k, 4, 2] (either orientation), xywha [k, 5] in the
    convention of masks_to_obb(form='xywha') (xywha_to_corners: one cos / sin away from exact), or masks in the forms of
    masks_to_obb, reduced to their rectangles on the device.  Degenerate boxes (NaN, zero area: empty masks) have IoU 0."""
    dev = torch.device(device)
    qa, qb = _as_obb_corners(a, dev, 'obb_iou'), _as_obb_corners(b, dev, 'obb_iou')
    D, G = int(qa.shape[0]), int(qb.shape[0])
    crowd = torch.zeros((G,), dtype=torch.uint8, device=dev) if iscrowd is None else \
        (_flat(iscrowd, dev) != 0).to(torch.uint8)
    if crowd.shape[0] != G:
        raise ValueError(f'obb_iou: iscrowd has {crowd.shape[0]} entries for {G} boxes')
    if D == 0 or G == 0:
        return torch.zeros((D, G), dtype=torch.float64, device=dev)
    # one unit per row of `a`: a unit is one block of the kernel, so a single [D] x [G] unit would run on one CU
    d = np.arange(D, dtype=np.int64)
    units = ops.coco_units(d, np.zeros(D, np.int64), d * G, np.ones(D, np.int64), np.full(D, G, np.int64),
                           np.zeros(D, np.int64), dev)
    return ops.obb_iou(units, D * G, qa, qb, crowd).view(D, G)


def nms_rotated(obb, scores, labels=None, iou_thr=0.5, device='cuda:0'):
    """mmcv.ops.nms_rotated: greedy suppression by rotated IoU > iou_thr (strict) in descending score order (ties by
    position), between boxes of one label when `labels` is given, between all otherwise -> keep int64 [m] on the device,
    indices into the input in kept order (ops.obb_nms).  `obb` in the forms of obb_iou; degenerate boxes are
    kept and suppress nothing."""
    dev = torch.device(device)
    quad = _as_obb_corners(obb, dev, 'nms_rotated')
    n = int(quad.shape[0])
    s = _flat(scores, dev).to(torch.float32)
    lab = torch.zeros((n,), dtype=torch.int32, device=dev) if labels is None else _flat(labels, dev).to(torch.int32)
    if s.shape[0] != n or lab.shape[0] != n:
        raise ValueError(f'nms_rotated: {n} boxes, {s.shape[0]} scores and {lab.shape[0]} labels')
    return ops.obb_nms(quad, s, lab, iou_thr, class_agnostic=labels is None)


def _flat(x, dev):
    """a tensor, array or list -> a flat tensor on `dev`"""
    return (x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))).reshape(-1).to(dev)


def mask_components(masks, device='cuda:0'):
    """Masks -> per instance dict(count, areas int32 [c], bboxes int32 [c, 4] = (x0, y0, x1, y1) end-exclusive) of its
    8-connected components, ordered by their first pixel in column-major order; labelled on the device in the run domain
    (rle.runs_components).  `masks` in the forms of rle.masks_to_runs.  One transfer after the labelling's two
    reads."""
    counts, n, size, _ = rle.masks_to_runs(masks, device, 'mask_components', canonical=True)
    comps = rle.runs_components(counts, n, size)
    k, C = int(n.shape[0]), int(comps.comp_area.shape[0])
    buf = torch.cat([comps.comp_offs, comps.comp_area.to(torch.int64), comps.comp_box.reshape(-1).to(torch.int64)]).cpu().numpy()
    o, area, box = buf[:k + 1].tolist(), buf[k + 1:k + 1 + C].astype(np.int32), buf[k + 1 + C:].astype(np.int32).reshape(-1, 4)
    return [dict(count=o[i + 1] - o[i], areas=area[o[i]:o[i + 1]], bboxes=box[o[i]:o[i + 1]]) for i in range(k)]


def panoptic_to_coco(pan, num_things_classes, void=None):
    """A panoptic map -- PixelData with sem_seg [1, H, W] (a detector's `pred_panoptic_seg`), or an int tensor [H, W] /
    [1, H, W] -- in COCO's panoptic form: (uint8 [H, W, 3] on the host, segments_info).  The colour of id is panopticapi's
    id2rgb (id % 256, id // 256 % 256, id // 65536), VOID pixels are (0, 0, 0); segments_info is a list of dict(id,
    category_id = id % 1000, isthing, area) in ascending id without the void id.  `void`: the id of unpainted pixels
    (num_classes); by default the `void` field the fusion head sets on its PixelData.  A plain tensor, or a PixelData without
    that field, needs the argument: a ValueError otherwise (the void id would come out as a segment).  Areas come from one device unique /
    count (plumbing)."""
    sem = pan.sem_seg if hasattr(pan, 'sem_seg') else pan
    sem = torch.as_tensor(sem)
    if sem.dim() == 3:
        sem = sem[0]
    if sem.dim() != 2 or sem.dtype not in (torch.int32, torch.int64):
        raise ValueError('panoptic_to_coco expects an int32 / int64 map [H, W] or [1, H, W]')
    if void is None and isinstance(pan, PixelData):
        void = pan.get('void')
    if void is None:
        raise ValueError('panoptic_to_coco needs the void id (num_classes): pass void=, or a PixelData that carries it')
    ids, counts = torch.unique(sem, return_counts=True)
    sem64 = sem.to(torch.int64)
    rgb = torch.stack((sem64 % 256, sem64 // 256 % 256, sem64 // 65536), -1).to(torch.uint8)
    rgb[sem64 == void] = 0                              # VOID is colour (0, 0, 0) in COCO's PNGs
    segments = []
    for i, a in zip(ids.tolist(), counts.tolist()):
        if i == void:
            continue
        cat = i % 1000
        segments.append(dict(id=i, category_id=cat, isthing=bool(cat < num_things_classes), area=a))
    return rgb.cpu().numpy(), segments


def write_panoptic_png(pan, path, void=None):
    """Write a panoptic map -- PixelData with sem_seg [1, H, W], or an int tensor [H, W] / [1, H, W], on any device -- as the
    PNG mmdet's CocoPanopticMetric writes (coco_panoptic_metric.py:295-300): the colour of id is id2rgb (id % 256, id // 256
    % 256, id // 65536), and every pixel whose label id % 1000 is a void label is black.  `void`: a label or several
    (num_classes, ignore_index); by default the `void` field of the PixelData.  Returns the uint8 [H, W, 3] image written."""
    from PIL import Image
    sem = torch.as_tensor(pan.sem_seg if hasattr(pan, 'sem_seg') else pan)
    if sem.dim() == 3:
        sem = sem[0]
    if sem.dim() != 2 or sem.dtype not in (torch.int32, torch.int64):
        raise ValueError('write_panoptic_png expects an int32 / int64 map [H, W] or [1, H, W]')
    if void is None and isinstance(pan, PixelData):
        void = pan.get('void')
    if void is None:
        raise ValueError('write_panoptic_png needs the void label (num_classes): pass void=, or a PixelData that carries it')
    sem64 = sem.to(torch.int64)
    if bool((sem64 < 0).any()) or bool((sem64 >= 1 << 24).any()):
        raise ValueError('write_panoptic_png: ids must be in [0, 2^24)')
    for v in (void if isinstance(void, (tuple, list, set)) else (void,)):
        sem64 = torch.where(sem64 % 1000 == int(v), torch.zeros_like(sem64), sem64)
    rgb = torch.stack((sem64 % 256, sem64 // 256 % 256, sem64 // 65536), -1).to(torch.uint8).cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(rgb, 'RGB').save(path, format='PNG')
    return rgb


def panoptic_quality(preds, gts, gt_segments, classes, thing_classes=None, ignore_index=None, device=None):
    """PQ / SQ / RQ of lists of maps without a metric object: the computation of evaluation.CocoPanopticMetric (per image
    ops.pq_image on the device, one ops.pq_reduce in list order, one host read, PQStat.pq_average).  preds[i]: int map [H, W]
    or [1, H, W] or PixelData, id = label + 1000 * instance, void where id % 1000 is len(classes) (or ignore_index); gts[i]:
    uint8 [H, W, 3] (a panoptic PNG's pixels) or an int id map; gt_segments[i]: that image's segments_info -- dicts of id,
    category_id (the class index), iscrowd, area (None or absent: counted).  Returns the nine numbers of parse_pq_results
    (PQ, SQ, RQ, *_th, *_st, each x 100), `n` per group and `classwise`: {class: dict(tp, fp, fn, iou, pq, sq, rq)}."""
    from .evaluation import parse_pq_results, pq_results, pq_stat_from_packed
    if not (len(preds) == len(gts) == len(gt_segments)) or len(preds) == 0:
        raise ValueError('panoptic_quality expects three lists of one length, not empty')
    classes = list(classes)
    things = set(classes if thing_classes is None else thing_classes)
    categories = {i: dict(id=i, name=n, isthing=1 if n in things else 0) for i, n in enumerate(classes)}
    rows = []
    for p, g, segs in zip(preds, gts, gt_segments):
        sem = torch.as_tensor(p.sem_seg if hasattr(p, 'sem_seg') else p)
        sem = sem[0] if sem.dim() == 3 else sem
        dev = torch.device(device) if device is not None else (sem.device if ops._is_device(sem) else torch.device('cuda', torch.cuda.current_device()))
        ops.require_device(dev)
        row = ops.pq_image(sem.to(device=dev, dtype=torch.int32).contiguous(), torch.as_tensor(g).to(dev), segs, categories,
                           len(classes), ignore_index=ignore_index)
        rows.append({k: row[k] for k in ('tp', 'fp', 'fn', 'iou', 'status')})
    stat = pq_stat_from_packed(ops.pq_reduce(rows)['packed'], list(categories))
    res = pq_results(stat, categories)
    out = parse_pq_results(res)
    out['n'] = {g: res[g]['n'] for g in ('All', 'Things', 'Stuff')}
    out['classwise'] = {classes[c]: dict(tp=stat[c][0], fp=stat[c][1], fn=stat[c][2], iou=stat[c][3], **res['classwise'][c])
                        for c in categories}
    return out
