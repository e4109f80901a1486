"""Promptable SAM for callers: `SamSession` (one image embedding, any number of point / box / mask prompts),
`inference_prompts` (the one-shot form), `generate_masks` (HF's mask-generation pipeline for the whole image) and
`SamMaskGenerator` (the same with crop layers: the image and overlapping crops of it, merged by one NMS).

What it restates: HF `SamImageProcessor` / `SamProcessor` (transformers models/sam/image_processing_sam.py:
`_get_preprocess_shape`, `_normalize_coordinates`, `post_process_masks`, `_build_point_grid`, `filter_masks`,
`_compute_stability_score`, `_batched_mask_to_box`, `_mask_to_rle`, `_post_process_for_mask_generation`) around
`SamModel.forward`.  What runs where: resize + normalise + pad is `rsp_resize_pad`, the ViT the encoder kernels, the prompts
`rsp_sam_embed_prompts`, the decoder `SamMaskDecoderHIP.decode`, full-resolution masks `rsp_mask_post_logits`, candidate
scoring `rsp_mask_score_box` (no full-resolution field is ever stored for a candidate that is not kept), run lengths
`rsp_mask_rle`, NMS `rsp_batched_nms`.  The host sees prompt coordinates, the kept count and the final results."""
import contextlib
import math
from itertools import product

import numpy as np
import torch

from . import ops, rle
from .structures import InstanceData

# SamImageProcessor defaults (IMAGENET_DEFAULT_MEAN / STD on a 0..1 image, i.e. these on 0..255)
PIXEL_MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
PIXEL_STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)


def _sam_of(model):
    """`SamModelHIP` (or `SamHQModelHIP`) of a SamModelHIP / SamHQModelHIP / RSSamModel / SAMDet."""
    for path in ((), ('sam_model',), ('segmentor', 'sam_model'), ('segmentor',)):
        m = model
        for p in path:
            m = getattr(m, p, None)
            if m is None:
                break
        if m is not None and hasattr(m, 'mask_decoder') and hasattr(m, 'prompt_encoder') and hasattr(m, 'vision_encoder'):
            return m
    raise TypeError(f'{type(model).__name__}: expected a SamModelHIP, a SamHQModelHIP, an RSSamModel or a SAMDet')


def _is_hq(sam):
    """a `SamHQModelHIP`: its decoder carries the HQ branch"""
    return hasattr(sam.mask_decoder, 'hq_features')


def _embed(sam, pixel_values):
    """(image embeddings, SAM-HQ's intermediate list or None) of either model kind"""
    emb = sam.get_image_embeddings(pixel_values)
    return emb if isinstance(emb, tuple) else (emb, None)


def _hq_kwargs(sam, intermediate, hq_token_only):
    if not _is_hq(sam):
        if hq_token_only:
            raise ValueError('hq_token_only needs a SamHQModelHIP')
        return {}
    return dict(intermediate_embeddings=intermediate, hq_token_only=bool(hq_token_only))


def preprocess_shape(hw, longest_edge):
    """HF `_get_preprocess_shape`: the longest side becomes `longest_edge`, the other one int(x + 0.5)."""
    h, w = int(hw[0]), int(hw[1])
    scale = longest_edge * 1.0 / max(h, w)
    return int(h * scale + 0.5), int(w * scale + 0.5)


def scale_coords(coords, hw, new_hw):
    """HF `_normalize_coordinates`: [..., 2] (x, y) in original pixels -> input pixels (float64 on the host)."""
    c = np.array(coords, dtype=np.float64, copy=True)
    c[..., 0] = c[..., 0] * (new_hw[1] / hw[1])
    c[..., 1] = c[..., 1] * (new_hw[0] / hw[0])
    return c


def point_grid(n_per_side):
    """HF `_build_point_grid`: n x n points evenly spaced in [0, 1]^2, [n * n, 2] as (x, y), row-major."""
    off = 1 / (2 * n_per_side)
    side = np.linspace(off, 1 - off, n_per_side)
    xs = np.tile(side[None, :], (n_per_side, 1))
    ys = np.tile(side[:, None], (1, n_per_side))
    return np.stack([xs, ys], axis=-1).reshape(-1, 2)


class SamSession:
    """One image, embedded once; `predict` answers prompts given in ORIGINAL pixel coordinates.

    `image`: [H, W, 3] RGB, uint8 or float 0..255 (numpy array or tensor).  Preprocessing has HF `SamImageProcessor`'s
    geometry and arithmetic -- longest side to `image_size` with `_get_preprocess_shape`'s rounding, ImageNet mean / std,
    zero padding at the bottom / right -- but this package's resampling filter: `rsp_resize_pad` interpolates bilinearly
    with cv2's arithmetic (as `inference_detector` does), not with PIL's antialiased filter, so `pixel_values` differ from
    HF's processor where the image is strongly minified.
    With a `SamHQModelHIP` the session also keeps the ViT's early feature, and the per-image HQ features are computed by the
    first `predict` and reused by every later one; hq_token_only=True returns the HQ mask alone (one mask per prompt set)."""

    def __init__(self, model, image, hq_token_only=False):
        self.sam = _sam_of(model)
        self.hq_token_only = bool(hq_token_only)
        _hq_kwargs(self.sam, None, hq_token_only)
        dev = next(self.sam.parameters()).device
        ops.require_device(dev)
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image))
        if image.dim() != 3 or image.shape[2] != 3:
            raise ValueError('expected an [H, W, 3] image')
        self.original_size = (int(image.shape[0]), int(image.shape[1]))
        S = self.sam.image_size
        self.input_size = preprocess_shape(self.original_size, S)
        img = image.to(dev)
        # the padding value is the mean: (mean - mean) / std = 0, HF pads the normalised image with zeros
        self.pixel_values = ops.resize_pad(img, self.input_size, (S, S), PIXEL_MEAN,
                                           normalise=(PIXEL_MEAN, PIXEL_STD, False)).unsqueeze(0)
        with torch.no_grad():
            self.image_embeddings, self.intermediate_embeddings = _embed(self.sam, self.pixel_values)
        self.device = dev

    def _low_res(self, points, labels, boxes, mask_input, multimask_output, attention_similarity=None, target_embedding=None):
        dev = self.device
        n = None
        kw = {}
        if attention_similarity is not None:
            kw['attention_similarity'] = attention_similarity
        if target_embedding is not None:
            kw['target_embedding'] = target_embedding
        if points is not None:
            p = scale_coords(points, self.original_size, self.input_size)
            if p.ndim == 2:
                p = p[None]
            if p.ndim != 3 or p.shape[-1] != 2:
                raise ValueError('points: expected [Pb, P, 2] (or [P, 2] for one prompt set)')
            n = p.shape[0]
            kw['input_points'] = torch.from_numpy(p).to(torch.float32).to(dev).unsqueeze(0)
            if labels is None:
                lab = np.ones(p.shape[:2], dtype=np.int32)
            else:
                lab = np.asarray(labels, dtype=np.int32).reshape(p.shape[:2])
            kw['input_labels'] = torch.from_numpy(lab).to(dev).unsqueeze(0)
        elif labels is not None:
            raise ValueError('labels without points')
        if boxes is not None:
            b = np.asarray(boxes, dtype=np.float64).reshape(-1, 2, 2)
            b = scale_coords(b, self.original_size, self.input_size).reshape(-1, 4)
            if n is not None and b.shape[0] != n:
                raise ValueError(f'{n} point sets but {b.shape[0]} boxes: one box per prompt set')
            n = b.shape[0]
            kw['input_boxes'] = torch.from_numpy(b).to(torch.float32).to(dev).unsqueeze(0)
        if n is None:
            raise ValueError('predict needs points or boxes')
        if mask_input is not None:
            m = torch.as_tensor(mask_input, dtype=torch.float32).to(dev)
            kw['input_masks'] = m.reshape(1, 1, m.shape[-2], m.shape[-1])
        kw.update(_hq_kwargs(self.sam, self.intermediate_embeddings, self.hq_token_only))
        out = self.sam(image_embeddings=self.image_embeddings, multimask_output=multimask_output, **kw)
        return out.pred_masks[0], out.iou_scores[0]                       # [Pb, C, 256, 256], [Pb, C]

    def full_res(self, low_res, mask_threshold=0.0, want_val=False):
        """HF `post_process_masks`: low_res [k, h, w] logits -> bilinear to the padded input, crop the padding away, bilinear
        to the original size, `> mask_threshold`.  bool [k, H, W] (and the values with want_val)."""
        S = self.sam.image_size
        return ops.mask_post_logits(low_res.contiguous(), (S, S), self.input_size, self.original_size, mask_threshold,
                                    want_val=want_val)

    @torch.no_grad()
    def predict(self, points=None, labels=None, boxes=None, mask_input=None, multimask_output=True, return_logits=False,
                mask_threshold=0.0, attention_similarity=None, target_embedding=None):
        """points [Pb, P, 2] / labels [Pb, P] (1 foreground, 0 background, -1 padding) / boxes [Pb, 4], all in original pixels;
        mask_input: [256, 256] low-resolution logits of an earlier call (shared by the prompt sets).  Returns
        (masks bool [Pb, C, H, W] -- the fp32 values with return_logits --, iou_scores [Pb, C], low_res_logits
        [Pb, C, 256, 256]); C = 3 with multimask_output, else 1.  ORDER with multimask_output: SAM's mask tokens 1, 2, 3 for a
        `SamModelHIP`; for a `SamHQModelHIP` the three masks and scores are sorted by predicted IoU, descending (HF
        `SamHQMaskDecoder`), and with the session's hq_token_only the masks are the ONE HQ mask per prompt set ([Pb, 1, ..])
        while iou_scores stays [Pb, 3].  attention_similarity [1 | Pb, 1, 1, N] / target_embedding
        [..., 256]: HF's PerSAM hooks, passed through to `SamModelHIP.forward` (device tensors)."""
        low, iou = self._low_res(points, labels, boxes, mask_input, multimask_output, attention_similarity, target_embedding)
        Pb, C, h, w = low.shape
        H, W = self.original_size
        flat = low.reshape(Pb * C, h, w)
        if return_logits:
            masks = self.full_res(flat, mask_threshold, want_val=True)[1]
        else:
            masks = self.full_res(flat, mask_threshold)
        return masks.view(Pb, C, H, W), iou, low


def inference_prompts(model, image, hq_token_only=False, **prompts):
    """One-shot `SamSession(model, image, hq_token_only).predict(**prompts)`."""
    return SamSession(model, image, hq_token_only=hq_token_only).predict(**prompts)


def filter_candidates(iou, score, pred_iou_thresh, stability_score_thresh):
    """HF `filter_masks`: keep mask of K candidates from the predicted IoU [K] and the integer scores [K, 7] of
    ops.mask_score_box (stability = pixels above thr + offset / pixels above thr - offset, int32 / int32 -> fp32 as torch
    divides; 0 / 0 is NaN and fails the comparison, as in HF)."""
    keep = torch.ones_like(iou, dtype=torch.bool)
    if pred_iou_thresh > 0.0:
        keep = keep & (iou > pred_iou_thresh)
    if stability_score_thresh > 0.0:
        keep = keep & ((score[:, 0] / score[:, 1]) > stability_score_thresh)
    return keep


def _check_region_area(min_mask_region_area):
    if int(min_mask_region_area) != min_mask_region_area or int(min_mask_region_area) < 0:
        raise ValueError(f'min_mask_region_area must be a non-negative integer, got {min_mask_region_area!r}')
    return int(min_mask_region_area)


def _region_nms(info, offsets, nms_thresh):
    """segment-anything `postprocess_small_regions` after the masks were cleaned: info int32 [m, 8] of
    ops.remove_small_regions (mode 'both') for the m survivors of the first NMS in their order, offsets int32 [m, 2] = (x0, y0)
    of every survivor's crop in the image.  A second NMS over the boxes of the CLEANED masks with score 1 for an unchanged and
    0 for a changed mask (equal scores: the lower index wins, rsp_batched_nms' rule), so that a mask which cleaning made a
    duplicate of an untouched one gives way.  Returns (sel: the kept positions ASCENDING as a host list -- a stable filter of
    the previous order, where segment-anything reorders by the 0 / 1 score --, boxes fp32 [m, 4] of the cleaned masks in the
    image frame, changed bool [m]).  One host read: the NMS's count, the kept list and the labelling's status together."""
    m = int(info.shape[0])
    dev = info.device
    changed = (info[:, 0] | info[:, 1]) != 0
    boxes = (info[:, 2:6] + torch.cat([offsets, offsets], 1)).to(torch.float32)
    r = ops.batched_nms((boxes.view(1, m, 4).contiguous(), (~changed).to(torch.float32).view(1, m),
                         torch.zeros((1, m), dtype=torch.int32, device=dev), torch.arange(m, dtype=torch.int32, device=dev).view(1, m),
                         torch.full((1,), m, dtype=torch.int32, device=dev)), 1, m, float(nms_thresh), m)
    packed = torch.cat([r['count'].to(torch.int32).view(1), r['keep'][0].to(torch.int32), info[:, 7]]).cpu().tolist()
    ops.check_region_status(packed[1 + m:])
    return sorted(packed[1:1 + packed[0]]), boxes, changed


@torch.no_grad()
def generate_masks(model, image, points_per_side=32, pred_iou_thresh=0.88, stability_score_thresh=0.95,
                   stability_score_offset=1.0, mask_threshold=0.0, crops_nms_thresh=0.7, crop_n_layers=0, output='rle',
                   mask_batch=64, session=None, _stages=None, min_mask_region_area=0, hq_token_only=False):
    """HF's mask generation (`MaskGenerationPipeline` over `SamImageProcessor.generate_crop_boxes` / `filter_masks` /
    `post_process_for_mask_generation`) for the whole image as one crop: a points_per_side^2 grid of single-point prompts,
    three masks each, filtered by predicted IoU and stability score, NMS on the mask boxes.  Returns `InstanceData` in NMS
    order: bboxes fp32 [k, 4] (x0, y0, x1, y1, inclusive maxima as HF's `_batched_mask_to_box`), scores fp32 [k] (predicted
    IoU), masks = list of uncompressed RLE dicts (output='rle') or bool [k, H, W] (output='dense').
    min_mask_region_area > 0: segment-anything's `postprocess_small_regions` on the NMS's survivors, as in `SamMaskGenerator`
    (holes and islands smaller than that are removed, a second NMS drops what became a duplicate; `region_changed` bool [k]).
    hq_token_only (a `SamHQModelHIP`): ONE candidate per point, the HQ mask, scored with the highest of the three predicted
    IoUs (the first: they come sorted); default: the three SAM + HQ masks in that order.
    session: an existing `SamSession` of the image (then `model` / `image` / hq_token_only are not read); mask_batch: full-resolution masks
    built per kernel call; _stages: a dict that receives the stage tensors (candidate logits, IoU, scores, kept indices,
    boxes) -- the stage-wise parity tests read them."""
    if crop_n_layers:
        raise NotImplementedError('generate_masks: crop_n_layers > 0 (multi-crop generation) is not implemented here, '
                                  'the image is processed as one crop; use SamMaskGenerator(model, crop_n_layers=...)')
    if output not in ('rle', 'dense'):
        raise ValueError("output must be 'rle' or 'dense'")
    area = _check_region_area(min_mask_region_area)
    s = session if session is not None else SamSession(model, image, hq_token_only=hq_token_only)
    H, W = s.original_size
    S = s.sam.image_size
    # HF _generate_crop_boxes: grid * (W, H) of the crop (= the image), then _normalize_coordinates inside predict
    pts = point_grid(points_per_side) * np.array([[W, H]], dtype=np.float64)
    low, iou = s._low_res(pts[:, None, :], None, None, None, True)
    iou = iou[:, :low.shape[1]]                                    # (hq_token_only: one mask, the best score)
    K = low.shape[0] * low.shape[1]
    low = low.reshape(K, low.shape[-2], low.shape[-1])
    iou = iou.reshape(K)
    score = ops.mask_score_box(low, (S, S), s.input_size, (H, W), mask_threshold, stability_score_offset)
    keep = filter_candidates(iou, score, pred_iou_thresh, stability_score_thresh)
    idx = keep.nonzero()[:, 0]                                     # compaction on the device; the one host read (its size)
    # (HF also drops boxes that touch a crop edge which is not an image edge; with one crop = the image there is none)
    boxes = score[idx, 3:7].to(torch.float32)
    scores = iou[idx]
    if _stages is not None:
        _stages.update(low_res=low, iou=iou, score=score, kept=idx, boxes=boxes)
    order = ops.nms_flat(boxes, scores, torch.zeros_like(idx, dtype=torch.int32), crops_nms_thresh)
    sel = idx[order]
    res = InstanceData()
    res.bboxes, res.scores = boxes[order], scores[order]
    if area and int(sel.shape[0]):
        # first pass over the survivors: only the 8 integers per cleaned mask are kept; the kept ones are built again below
        info = torch.cat([ops.remove_small_regions(s.full_res(low[sel[i:i + mask_batch]], mask_threshold), area)[1]
                          for i in range(0, int(sel.shape[0]), mask_batch)], 0)
        kept, boxes2, changed = _region_nms(info, torch.zeros((int(sel.shape[0]), 2), dtype=torch.int32, device=low.device),
                                            crops_nms_thresh)
        kept = torch.tensor(kept, dtype=torch.int64).to(low.device)
        sel = sel[kept]
        res.region_changed = changed[kept]
        res.bboxes = torch.where(res.region_changed[:, None], boxes2[kept], res.bboxes[kept])
        res.scores = res.scores[kept]
    elif area:
        res.region_changed = torch.zeros((0,), dtype=torch.bool, device=low.device)
    if _stages is not None:
        _stages['final'] = sel
    dense, rles = [], []
    for i in range(0, int(sel.shape[0]), mask_batch):
        m = s.full_res(low[sel[i:i + mask_batch]], mask_threshold)
        if area:
            m = ops.remove_small_regions(m, area)[0]
        if output == 'dense':
            dense.append(m)
        else:
            rles.extend(rle.encode_mask_dicts(m))
    if output == 'dense':
        res.masks = torch.cat(dense, 0) if dense else torch.zeros((0, H, W), dtype=torch.bool, device=low.device)
    else:
        res.masks = rles
    return res


# --------------------------------------------------------------------------------------------------- PerSAM
class PerSam:
    """PerSAM's training-free one-shot segmentation (Zhang et al., "Personalize Segment Anything Model with One Shot";
    persam.py of the paper's code) in HF terms: ONE labelled reference, then `segment` finds that object in other images.

    `sam`: whatever `SamSession` accepts; `ref_image` [H, W, 3] as for `SamSession`; `ref_mask` [H, W], non-zero = object.
    The reference is embedded once.  Its mask goes through the image's front end as a {0, 1} float image (`rsp_resize_pad`,
    pad value 0), bilinearly to the embedding grid and `> 0` -- PerSAM's cell selection --; `rsp_persam_target` gives
    `.target_embedding` [1, 1, 256] (the mean of the selected embedding rows) and `.target_feature` [256] (its unit vector).
    A mask that selects no cell is a ValueError (the one host read of the constructor).

    `segment(images, batch_size=8, output='rle', cascade=True)`: one image or a list; images of one size go through the
    encoder and every decoder pass together, `batch_size` at a time, mixed sizes are grouped by size and the results come
    back in input order.  Per batch: (1) `rsp_persam_similarity` + `rsp_persam_locate`: the cosine similarity of every cell
    with the target at image resolution is never stored, its peak becomes the positive and its trough the negative point,
    its normalised g x g resampling the `attention_similarity`; (2) first pass: both points, one mask, both hooks; (3) the
    same points + the logits of (2) as `input_masks`, three masks, the one with the highest predicted IoU (lowest index on a
    tie); (4) as (3) + the box of (3)'s mask at original resolution (`rsp_mask_score_box`, inclusive maxima; an EMPTY mask
    gives that kernel's [0, 0, 0, 0] box where PerSAM itself fails); (5) `rsp_mask_post_logits`, `rsp_mask_rle`,
    `rsp_mask_score_box`.  cascade=False stops after (2).  Between the upload of a batch and the transfer of its results
    nothing is read on the host: points, boxes and the best-of-three choices stay device tensors.

    Returns per image a dict: mask (uncompressed COCO RLE dict of size [H, W], or bool [H, W] on the device with
    output='dense'), score (predicted IoU), bbox [x0, y0, x1, y1] (inclusive maxima, zeros for an empty mask), points
    [[x+, y+], [x-, y-]] and point_sims [s+, s-] (the field's maximum and minimum), all in original pixels.  A field that
    is constant has no peak: the points are pixel 0 and the attention similarity 0.5 everywhere (PerSAM yields NaN).
    The fine-tuned variant of the paper, PerSAM-F, is `PerSamF`.  Not implemented: topk > 1, several references."""

    RLE_CAP = 4096

    def __init__(self, sam, ref_image, ref_mask):
        self.sam = _sam_of(sam)
        if _is_hq(self.sam):
            raise NotImplementedError('PerSam with a SamHQModelHIP: PerSam feeds the decoder image embeddings it has built '
                                      'itself (batched, without the ViT\'s early feature the HQ branch needs); use a SamModelHIP')
        dev = next(self.sam.parameters()).device
        ops.require_device(dev)
        self.device = dev
        S, g = self.sam.image_size, self.sam.vision_encoder.grid
        ref_image = self._as_image(ref_image)
        if isinstance(ref_mask, np.ndarray):
            ref_mask = torch.from_numpy(np.ascontiguousarray(ref_mask))
        if ref_mask.dim() != 2 or tuple(ref_mask.shape) != tuple(ref_image.shape[:2]):
            raise ValueError('ref_mask: expected [H, W], the size of ref_image')
        hw = (int(ref_image.shape[0]), int(ref_image.shape[1]))
        nhw = preprocess_shape(hw, S)
        with torch.no_grad():
            pv = ops.resize_pad(ref_image.to(dev), nhw, (S, S), PIXEL_MEAN, normalise=(PIXEL_MEAN, PIXEL_STD, False)).unsqueeze(0)
            emb = self.sam.get_image_embeddings(pv)
            self.cell_mask = self.cells_of(ref_mask.to(dev), S, g)
            te, tf, cnt = ops.persam_target(self._rows(emb), self.cell_mask.reshape(-1))
        self.cells = int(cnt.item())
        if self.cells == 0:
            raise ValueError('PerSam: the reference mask selects no cell of the embedding grid')
        self.target_feature, self.target_embedding = tf, te.view(1, 1, 256)
        self._phase = lambda name: contextlib.nullcontext()      # tools/bench_sam_prompts.py times the phases through this

    @staticmethod
    def cells_of(mask, S, g):
        """PerSAM's cell selection: mask [H, W] on the device (non-zero = object) -> bool [g, g].  The mask goes through the
        image's front end as a {0, 1} float image (rsp_resize_pad to S x S, pad value 0), bilinearly to g x g
        (rsp_resize_bilinear_nhwc = F.interpolate(mode='bilinear', align_corners=False)) and `> 0`, which is exact: with
        non-negative inputs a cell is zero only if every pixel that contributes to it is."""
        hw = (int(mask.shape[0]), int(mask.shape[1]))
        m3 = (mask != 0).to(torch.float32).unsqueeze(-1).expand(hw[0], hw[1], 3).contiguous()
        mS = ops.resize_pad(m3, preprocess_shape(hw, S), (S, S), (0.0, 0.0, 0.0))[0]        # [S, S], values in [0, 1]
        mg = ops.resize_bilinear(mS.unsqueeze(-1).expand(S, S, 4).contiguous().unsqueeze(0), (g, g))[0, :, :, 0]
        return mg > 0

    @staticmethod
    def _as_image(image):
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image))
        if image.dim() != 3 or image.shape[2] != 3:
            raise ValueError('expected an [H, W, 3] image')
        return image

    @staticmethod
    def _rows(emb):
        """[B, 256, g, g] (channels-last memory) -> contiguous rows [B * g * g, 256]"""
        B, C, gh, gw = emb.shape
        return emb.permute(0, 2, 3, 1).reshape(B * gh * gw, C).contiguous()

    @torch.no_grad()
    def segment(self, images, batch_size=8, output='rle', cascade=True, _stages=None):
        if output not in ('rle', 'dense'):
            raise ValueError("output must be 'rle' or 'dense'")
        if int(batch_size) < 1:
            raise ValueError('batch_size must be >= 1')
        single = not isinstance(images, (list, tuple))
        imgs = [self._as_image(im) for im in ([images] if single else images)]
        groups = {}
        for i, im in enumerate(imgs):
            groups.setdefault((int(im.shape[0]), int(im.shape[1])), []).append(i)
        results = [None] * len(imgs)
        for hw, idx in groups.items():
            if hw[0] * hw[1] >= 2 ** 31:
                raise ValueError(f'PerSam: a {hw[0]} x {hw[1]} image has 2^31 pixels or more')
            for b0 in range(0, len(idx), int(batch_size)):
                sel = idx[b0:b0 + int(batch_size)]
                for i, r in zip(sel, self._batch([imgs[i] for i in sel], hw, output, cascade, _stages)):
                    results[i] = r
        return results[0] if single else results

    def _best(self, out):
        """best of three by predicted IoU (first index on a tie): (logits [B, h, w], iou [B], index [B]) on the device"""
        iou = out.iou_scores[:, 0]                                                  # [B, 3]
        best = iou.argmax(1)
        ar = torch.arange(iou.shape[0], device=iou.device)
        return out.pred_masks[:, 0][ar, best].contiguous(), iou[ar, best], best

    N_POINTS = 2                 # the peak and the trough of the similarity field

    def _prompts(self, xy, scale, B):
        """(input_points [B, 1, P, 2] in input pixels, input_labels [B, 1, P]) of locate's xy: HF _normalize_coordinates
        (float64, then fp32 as the processor's tensors), on the device"""
        P = self.N_POINTS
        pts = (xy[:, :2 * P].reshape(B, 1, P, 2).to(torch.float64) * scale).to(torch.float32)
        labels = torch.tensor([[[1, 0][:P]]], dtype=torch.int32).to(xy.device).expand(B, 1, P).contiguous()
        return pts, labels

    def _box_prompt(self, low, geo, scale):
        """(box int32 [B, 4] of the mask of `low` at original resolution, the same as input_boxes [B, 1, 4])"""
        box = ops.mask_score_box(low, *geo)[:, 3:7]
        bscale = torch.cat([scale, scale])
        return box, (box.to(torch.float64) * bscale).to(torch.float32).reshape(low.shape[0], 1, 4)

    def _decode(self, emb, pts, labels, attn, geo, scale, cascade, st):
        """PerSAM's decoder passes: (logits [B, h, w], predicted IoU [B]) of the final mask; the stages go into `st`"""
        sam, phase = self.sam, self._phase
        B, g = emb.shape[0], sam.vision_encoder.grid
        with phase('decoder pass 1'):
            out = sam(image_embeddings=emb, input_points=pts, input_labels=labels, multimask_output=False,
                      attention_similarity=attn.view(B, 1, 1, g * g), target_embedding=self.target_embedding)
            low, iou = out.pred_masks[:, 0, 0].contiguous(), out.iou_scores[:, 0, 0]
        st.update(low1=low, iou1=iou)
        if cascade:
            with phase('decoder pass 2'):
                out = sam(image_embeddings=emb, input_points=pts, input_labels=labels, input_masks=low.unsqueeze(1),
                          multimask_output=True)
                low, iou, best2 = self._best(out)
                st.update(low2=out.pred_masks[:, 0], iou2=out.iou_scores[:, 0], best2=best2)
            with phase('decoder pass 3'):
                box, boxes = self._box_prompt(low, geo, scale)
                out = sam(image_embeddings=emb, input_points=pts, input_labels=labels, input_boxes=boxes,
                          input_masks=low.unsqueeze(1), multimask_output=True)
                low, iou, best3 = self._best(out)
                st.update(box2=box, boxes=boxes, low3=out.pred_masks[:, 0], iou3=out.iou_scores[:, 0], best3=best3)
        return low, iou

    def _batch(self, imgs, hw, output, cascade, _stages):
        sam, dev, phase = self.sam, self.device, self._phase
        S, g = sam.image_size, sam.vision_encoder.grid
        B, P = len(imgs), self.N_POINTS
        H, W = hw
        nhw = preprocess_shape(hw, S)
        geo = ((S, S), nhw, hw)
        with phase('front end'):
            pv = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
            for b, im in enumerate(imgs):
                ops.resize_pad(im.to(dev), nhw, (S, S), PIXEL_MEAN, out=pv[b], normalise=(PIXEL_MEAN, PIXEL_STD, False))
        with phase('encoder'):
            emb = sam.get_image_embeddings(pv)
        with phase('similarity'):
            sim, low0 = ops.persam_similarity(self._rows(emb), self.target_feature, B, g, g)
        with phase('locate'):
            stats, xy, attn = ops.persam_locate(low0, *geo, g)
            scale = torch.tensor([nhw[1] / W, nhw[0] / H], dtype=torch.float64).to(dev)
            pts, labels = self._prompts(xy, scale, B)
        st = dict(sim=sim, low_sim=low0, stats=stats, xy=xy, attn_sim=attn, points=pts)
        low, iou = self._decode(emb, pts, labels, attn, geo, scale, cascade, st)
        with phase('masks + run lengths'):
            masks = ops.mask_post_logits(low, *geo)
            score = ops.mask_score_box(low, *geo)
            if output == 'rle':
                counts = torch.empty((B, self.RLE_CAP), dtype=torch.int32, device=dev)
                ws = torch.empty((B, self.RLE_CAP), dtype=torch.int32, device=dev)
                n = torch.empty((B,), dtype=torch.int32, device=dev)
                ops.mask_rle_into(masks, counts, ws, n)
        st.update(low_final=low, iou_final=iou, masks=masks, score=score)
        if _stages is not None:
            _stages.setdefault('batches', []).append(st)
        # ---- the transfer of the batch's results: the first host reads since the upload ----
        with phase('transfer'):
            ints = torch.cat([xy[:, :2 * P], score[:, 3:7]] + ([n.view(B, 1)] if output == 'rle' else []), 1).cpu()
            flts = torch.cat([stats[:, :P], iou.reshape(B, 1)], 1).cpu()
            extra = self._extra_results()
            if output == 'rle':
                nn = ints[:, 2 * P + 4]
                if int(nn.min()) < 0:                          # a mask with more runs than RLE_CAP: again with room (rare)
                    counts, _, nn, _ = rle.encode_runs(masks, cap=ops.grown_cap(-int(nn.min())))
                counts = counts[:, :int(nn.max())].cpu()
        rles = rle.runs_to_dicts(counts, nn, hw) if output == 'rle' else None       # host lists: after the transfer phase
        res = []
        for b in range(B):
            r = dict(score=float(flts[b, P]), bbox=ints[b, 2 * P:2 * P + 4].tolist(), points=ints[b, :2 * P].reshape(P, 2).tolist(),
                     point_sims=flts[b, :P].tolist(), **extra)
            r['mask'] = rles[b] if output == 'rle' else masks[b]
            res.append(r)
        return res

    def _extra_results(self):
        """further entries of every result dict (read inside the transfer phase)"""
        return {}


# --------------------------------------------------------------------------------------------------- PerSAM-F
class PerSamF(PerSam):
    """PerSAM-F, the variant of the same paper that LEARNS which of SAM's three mask scales the object lives at (persam_f.py
    of the paper's code): two numbers, fitted on the one labelled reference, weigh the three masks of the first decoder
    pass.  Nothing is back-propagated through SAM.

    `PerSamF(sam, ref_image, ref_mask, epochs=1000, lr=1e-3)`, arguments as for `PerSam`.  The constructor (1) embeds the
    reference and selects cells as `PerSam` does (no selected cell: the same ValueError, after the constructor's only host
    read); (2) `.target_feature` = unit vector of mean(rows) / 2 + max(rows) / 2 over the selected embedding rows (the mean
    is `rsp_persam_target`'s, the masked maximum and the normalisation torch, once per reference); (3) the similarity of the
    reference with itself, `rsp_persam_locate`: its peak is the one positive point -- no negative point, no
    `attention_similarity`, no `target_embedding` anywhere here; (4) ONE decoder pass on the reference, three masks; (5)
    `rsp_persam_f_fit`: from w1 = w2 = 1 / 3 (w0 = 1 - w1 - w2), `epochs` steps of AdamW(lr, eps=1e-4, weight_decay=0.01)
    under a cosine schedule on the dice + focal loss of sigmoid(sum_k w_k field_k) against `ref_mask` at original resolution;
    a step is one traversal of the three fields and a one-wave update, the whole fit is enqueued without a host read.
    `.weights` fp32 [3] = (w0, w1, w2) and `.loss_history` fp64 [epochs, 3] = (loss, d / d w1, d / d w2) each step was taken
    from stay on the device; `.cell_mask`, `.cells` as in `PerSam`; `.ref_point` (int32 [x, y]), `.ref_point_sim` and
    `.ref_low_res` [1, 3, 4g, 4g] keep what the fit saw.

    `segment(images, batch_size=8, output='rle')`: grouping, batching and results as `PerSam.segment`.  Per batch: similarity
    and locate with the new target, the peak alone as prompt; pass 1: three masks, no hooks, `low_w = sum_k w_k low_k` in fp32
    (resampling is linear and the weights sum to 1: the field of low_w is the paper's weighted sum of the up-sampled logits
    up to rounding); pass 2: the point + the box of `field(low_w) > 0` + low_w as `input_masks`, three masks, best by
    predicted IoU (first index on a tie); pass 3: the point + the box of that mask + its logits, best by IoU; mask, score,
    box and run lengths as `PerSam` makes them.  Nothing is read on the host between a batch's upload and the transfer of
    its results.  Results as `PerSam`'s with points [[x+, y+]], point_sims [s+] and `weights` [w0, w1, w2] added.
    Not implemented: topk > 1, several references."""

    N_POINTS = 1

    def __init__(self, sam, ref_image, ref_mask, epochs=1000, lr=1e-3):
        self.sam = _sam_of(sam)
        if _is_hq(self.sam):
            raise NotImplementedError('PerSamF with a SamHQModelHIP: PerSamF feeds the decoder image embeddings it has built '
                                      'itself (batched, without the ViT\'s early feature the HQ branch needs); use a SamModelHIP')
        if int(epochs) < 1:
            raise ValueError('PerSamF: epochs must be >= 1')
        dev = next(self.sam.parameters()).device
        ops.require_device(dev)
        self.device = dev
        self._phase = lambda name: contextlib.nullcontext()
        S, g = self.sam.image_size, self.sam.vision_encoder.grid
        ref_image = self._as_image(ref_image)
        if isinstance(ref_mask, np.ndarray):
            ref_mask = torch.from_numpy(np.ascontiguousarray(ref_mask))
        if ref_mask.dim() != 2 or tuple(ref_mask.shape) != tuple(ref_image.shape[:2]):
            raise ValueError('ref_mask: expected [H, W], the size of ref_image')
        hw = (int(ref_image.shape[0]), int(ref_image.shape[1]))
        nhw = preprocess_shape(hw, S)
        geo = ((S, S), nhw, hw)
        with torch.no_grad():
            pv = ops.resize_pad(ref_image.to(dev), nhw, (S, S), PIXEL_MEAN, normalise=(PIXEL_MEAN, PIXEL_STD, False)).unsqueeze(0)
            emb = self.sam.get_image_embeddings(pv)
            gt = (ref_mask.to(dev) != 0)
            self.cell_mask = self.cells_of(gt, S, g)
            rows = self._rows(emb)
            mean, _, cnt = ops.persam_target(rows, self.cell_mask.reshape(-1))
            self.cells = int(cnt.item())
            if self.cells == 0:
                raise ValueError('PerSamF: the reference mask selects no cell of the embedding grid')
            top = torch.where(self.cell_mask.reshape(-1, 1), rows, torch.full_like(rows, float('-inf'))).amax(0)
            target = mean / 2 + top / 2
            self.target_feature = (target / target.norm()).contiguous()
            sim, low0 = ops.persam_similarity(rows, self.target_feature, 1, g, g)
            stats, xy, _ = ops.persam_locate(low0, *geo, g)
            scale = torch.tensor([nhw[1] / hw[1], nhw[0] / hw[0]], dtype=torch.float64).to(dev)
            pts, labels = self._prompts(xy, scale, 1)
            out = self.sam(image_embeddings=emb, input_points=pts, input_labels=labels, multimask_output=True)
            self.ref_low_res = out.pred_masks[:, 0].contiguous()                       # [1, 3, 4g, 4g]
            w, hist = ops.persam_f_fit(self.ref_low_res, gt.unsqueeze(0), *geo, epochs=int(epochs), lr=float(lr), want_history=True)
        self.ref_point, self.ref_point_sim = xy[0, :2], stats[0, 0]
        self.weights, self.loss_history = w[0], hist[0]

    @torch.no_grad()
    def segment(self, images, batch_size=8, output='rle', _stages=None):
        return super().segment(images, batch_size=batch_size, output=output, cascade=True, _stages=_stages)

    def _decode(self, emb, pts, labels, attn, geo, scale, cascade, st):
        sam, phase = self.sam, self._phase
        with phase('decoder pass 1'):
            out = sam(image_embeddings=emb, input_points=pts, input_labels=labels, multimask_output=True)
            low = (out.pred_masks[:, 0] * self.weights.view(1, 3, 1, 1)).sum(1).contiguous()
            st.update(low1=out.pred_masks[:, 0], iou1=out.iou_scores[:, 0], low_w=low)
        for n in (2, 3):
            with phase(f'decoder pass {n}'):
                box, boxes = self._box_prompt(low, geo, scale)
                out = sam(image_embeddings=emb, input_points=pts, input_labels=labels, input_boxes=boxes,
                          input_masks=low.unsqueeze(1), multimask_output=True)
                low, iou, best = self._best(out)
                st.update({f'box{n - 1}': box, f'boxes{n - 1}': boxes, f'low{n}': out.pred_masks[:, 0], f'iou{n}': out.iou_scores[:, 0],
                           f'best{n}': best})
        return low, iou

    def _extra_results(self):
        return dict(weights=self.weights.cpu().tolist())


# --------------------------------------------------------------------------------------------------- crop layers
def generate_crop_boxes(crop_n_layers, overlap_ratio, hw):
    """HF `_generate_per_layer_crops`: ([x0, y0, x1, y1] per crop, layer per crop); crop 0 is the image, then per layer
    `product(x0s, y0s)` -- 2^(l+1) crops per side, the last of every row and column clamped to the image."""
    H, W = int(hw[0]), int(hw[1])
    boxes, layers = [[0, 0, W, H]], [0]
    short = min(H, W)
    for l in range(crop_n_layers):
        n = 2 ** (l + 1)
        overlap = int(overlap_ratio * short * (2 / n))
        cw = int(math.ceil((overlap * (n - 1) + W) / n))
        ch = int(math.ceil((overlap * (n - 1) + H) / n))
        x0s = [int((cw - overlap) * i) for i in range(n)]
        y0s = [int((ch - overlap) * i) for i in range(n)]
        for x0, y0 in product(x0s, y0s):
            boxes.append([x0, y0, min(x0 + cw, W), min(y0 + ch, H)])
            layers.append(l + 1)
    return boxes, layers


# crops per encoder / decoder / scoring call by the encoder's width (ViT-B / L / H) when crop_batch is None: the smallest value
# after which the time per image stopped improving by more than the repetitions' spread in the sweep of
# tools/bench_sam_prompts.py (profiles/sam_prompts/multicrop.json) ...
DEFAULT_CROP_BATCH = {768: 16, 1024: 8, 1280: 16}
# ... and never more candidates per batch than the largest batch that sweep ran (4 crops x 32 x 32 points x 3 masks = 16 crops x
# 16 x 16 x 3; 3.2 GB of low-resolution logits)
DEFAULT_BATCH_CANDIDATES = 12288


class SamMaskGenerator:
    """SAM's automatic mask generation with crop layers: the image (crop 0) and, per layer l, 2^l x 2^l overlapping crops of
    it, each resized to the model's input on its own, prompted with its own point grid, filtered (predicted IoU, stability
    score, HF `_is_box_near_crop_edge`), moved into the image frame and merged by ONE NMS over all crops.

    The semantics are HF's helpers (`_generate_per_layer_crops`, `_build_point_grid`, `filter_masks`,
    `_is_box_near_crop_edge`, `_pad_masks`, `_mask_to_rle`, `_post_process_for_mask_generation`) composed per crop -- not
    HF's `MaskGenerationPipeline`, which filters only the first crop, leaves boxes in crop coordinates and scales a crop's
    grid with the whole image's resize factor.  Not implemented: segment-anything's per-crop box NMS and its
    preference for smaller crops.

    `min_mask_region_area` > 0 is segment-anything's `postprocess_small_regions` on the survivors of that NMS: in every mask
    first the holes, then the islands with fewer pixels are removed (`rsp_mask_remove_small_regions`, 8-connected, on the
    crop-sized mask), the boxes of the cleaned masks go through a second NMS in which an unchanged mask beats a changed one,
    and the survivors keep their order (segment-anything moves the unchanged ones to the front).  A kept mask that was
    changed gets its cleaned mask and that mask's box; `scores` stay the predicted IoUs; `region_changed` bool [k] tells.
    With 0 (the default) none of this runs.

    `sam`: whatever `SamSession` accepts.  `crop_batch`: crops per encoder / decoder / scoring call (all of one layer, so
    that they share the number of prompts); None picks `DEFAULT_CROP_BATCH` by the encoder's width, capped at
    `DEFAULT_BATCH_CANDIDATES` candidates per batch.  `generate(image)`
    returns `InstanceData` in NMS order, everything in IMAGE coordinates: bboxes fp32 [k, 4], scores fp32 [k], masks (list of
    uncompressed RLE dicts of size [H, W], or bool [k, H, W] with output='dense'), crop_index int64 [k].  With
    crop_n_layers=0 the result is `generate_masks`' bit for bit.  hq_token_only (a `SamHQModelHIP`): as in `generate_masks`."""

    def __init__(self, sam, points_per_side=32, pred_iou_thresh=0.88, stability_score_thresh=0.95, stability_score_offset=1.0,
                 mask_threshold=0.0, crops_nms_thresh=0.7, crop_n_layers=1, crop_overlap_ratio=512 / 1500,
                 crop_n_points_downscale_factor=1, crop_batch=None, output='rle', mask_batch=64, min_mask_region_area=0,
                 hq_token_only=False):
        if output not in ('rle', 'dense'):
            raise ValueError("output must be 'rle' or 'dense'")
        if int(crop_n_layers) < 0:
            raise ValueError('crop_n_layers must be >= 0')
        self.min_mask_region_area = _check_region_area(min_mask_region_area)
        self.sam = _sam_of(sam)
        self.hq_token_only = bool(hq_token_only)          # a SamHQModelHIP: one candidate per point (see generate_masks)
        _hq_kwargs(self.sam, None, hq_token_only)
        self.crop_n_layers, self.crop_overlap_ratio = int(crop_n_layers), float(crop_overlap_ratio)
        self.grids = []
        for l in range(self.crop_n_layers + 1):
            n = int(points_per_side / crop_n_points_downscale_factor ** l)
            if n < 1:
                raise ValueError(f'layer {l}: points_per_side={points_per_side} / crop_n_points_downscale_factor='
                                 f'{crop_n_points_downscale_factor} ** {l} leaves an empty point grid')
            self.grids.append(point_grid(n))
        self.pred_iou_thresh, self.stability_score_thresh = pred_iou_thresh, stability_score_thresh
        self.stability_score_offset, self.mask_threshold = stability_score_offset, mask_threshold
        self.crops_nms_thresh, self.output, self.mask_batch = crops_nms_thresh, output, int(mask_batch)
        if crop_batch is not None and int(crop_batch) < 1:
            raise ValueError('crop_batch must be >= 1')
        self.crop_batch = None if crop_batch is None else int(crop_batch)
        self._phase = lambda name: contextlib.nullcontext()      # tools/bench_sam_prompts.py times the phases through this

    def crop_boxes(self, hw):
        """[x0, y0, x1, y1] of every crop of an (H, W) image; crop 0 is the image."""
        return generate_crop_boxes(self.crop_n_layers, self.crop_overlap_ratio, hw)[0]

    def _batches(self, layers):
        """[(first crop, end)]: consecutive crops of ONE layer, crop_batch at a time; with crop_batch=None the default of the
        encoder's width, capped so that a batch holds at most DEFAULT_BATCH_CANDIDATES candidates"""
        out, c = [], 0
        while c < len(layers):
            nb = self.crop_batch
            if nb is None:
                width = getattr(getattr(self.sam, 'vision_encoder', None), 'D', None)
                nb = max(1, min(DEFAULT_CROP_BATCH.get(width, 8), DEFAULT_BATCH_CANDIDATES // (3 * self.grids[layers[c]].shape[0])))
            e = c
            while e < len(layers) and e - c < nb and layers[e] == layers[c]:
                e += 1
            out.append((c, e))
            c = e
        return out

    def _plan(self, hw):
        """per crop: box, layer, input size and the prompt points in the crop's input pixels; the two device tables"""
        S = self.sam.image_size
        H, W = hw
        boxes, layers = generate_crop_boxes(self.crop_n_layers, self.crop_overlap_ratio, hw)
        front, geo, pts = [], [], []
        for (x0, y0, x1, y1), l in zip(boxes, layers):
            ch, cw = y1 - y0, x1 - x0
            nh, nw = preprocess_shape((ch, cw), S)
            front.append([x0, y0, x1, y1, nh, nw])
            geo.append([S, S, nh, nw, ch, cw, x0, y0, x1, y1, W, H])
            # HF _generate_crop_images: grid * (cw, ch) = crop-local pixels; then to the crop's own input size
            p = self.grids[l] * np.array([[cw, ch]], dtype=np.float64)
            pts.append(scale_coords(p[:, None, :], (ch, cw), (nh, nw)))
        return boxes, layers, front, geo, pts

    @torch.no_grad()
    def generate(self, image, _stages=None):
        sam, phase = self.sam, self._phase
        dev = next(sam.parameters()).device
        ops.require_device(dev)
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image))
        if image.dim() != 3 or image.shape[2] != 3:
            raise ValueError('expected an [H, W, 3] image')
        H, W = int(image.shape[0]), int(image.shape[1])
        if H * W >= 2 ** 31:
            raise ValueError(f'SamMaskGenerator: a {H} x {W} image has {H * W} pixels; run counts are 32-bit (< 2^31 pixels)')
        S = sam.image_size
        boxes_c, layers, front, geo, pts = self._plan((H, W))
        img = image.to(dev)                                            # the decoded image goes up once
        front_t = torch.tensor(front, dtype=torch.int32).to(dev)
        geo_t = torch.tensor(geo, dtype=torch.int32).to(dev)
        max_out = (max(g[4] for g in geo), max(g[5] for g in geo))
        batches = self._batches(layers)
        kept_low, kept_iou, kept_box, kept_crop, kept_cand = [], [], [], [], []
        n_kept, cand0 = 0, 0
        for c0, c1 in batches:
            B, Pb = c1 - c0, pts[c0].shape[0]
            with phase('crop front end'):
                pv = ops.crops_resize_pad(img, front_t[c0:c1], (S, S), PIXEL_MEAN, normalise=(PIXEL_MEAN, PIXEL_STD, False))
            with phase('encoder'):
                emb, inter = _embed(sam, pv)
            with phase('decoder'):
                p = torch.from_numpy(np.stack(pts[c0:c1], 0)).to(torch.float32).to(dev)                 # [B, Pb, 1, 2]
                out = sam(image_embeddings=emb, input_points=p, multimask_output=True,
                          input_labels=torch.ones((B, Pb, 1), dtype=torch.int32, device=dev),
                          **_hq_kwargs(sam, inter, self.hq_token_only))
                low, iou = out.pred_masks, out.iou_scores[..., :out.pred_masks.shape[2]]
                K = B * Pb * low.shape[2]
                low, iou = low.reshape(K, low.shape[-2], low.shape[-1]), iou.reshape(K)
            with phase('scoring'):
                cidx = torch.arange(c0, c1, dtype=torch.int32, device=dev).repeat_interleave(K // B)
                score = ops.mask_score_box_crops(low, cidx, geo_t, max_out, self.mask_threshold, self.stability_score_offset,
                                                 check_index=False)
            with phase('filter + NMS'):
                keep = filter_candidates(iou, score, self.pred_iou_thresh, self.stability_score_thresh) & (score[:, 7] == 0)
                idx = keep.nonzero()[:, 0]                             # compaction; the one host read of the batch (its size)
                n_kept += int(idx.shape[0])
                if n_kept > ops.NMS_MAX_CANDIDATES:
                    raise ValueError(f'SamMaskGenerator: more than {ops.NMS_MAX_CANDIDATES} candidates pass the filters '
                                     '(ops.NMS_MAX_CANDIDATES, what rsp_batched_nms holds): raise pred_iou_thresh / '
                                     'stability_score_thresh or lower points_per_side / crop_n_layers')
                # the kept candidates' logits leave the batch's buffer here; the next batch may reuse it
                kept_low.append(low[idx]); kept_iou.append(iou[idx]); kept_box.append(score[idx, 3:7].to(torch.float32))
                kept_crop.append(cidx[idx]); kept_cand.append(idx + cand0)
            if _stages is not None:
                _stages.setdefault('batches', []).append(dict(crops=(c0, c1), low_res=low, iou=iou, score=score, kept=idx))
            cand0 += K
            del out, low, score, emb, pv
        low, scores, boxes = torch.cat(kept_low, 0), torch.cat(kept_iou, 0), torch.cat(kept_box, 0)
        crop, cand = torch.cat(kept_crop, 0), torch.cat(kept_cand, 0)
        if _stages is not None:
            _stages.update(kept=cand, kept_crop=crop, boxes=boxes, crop_boxes=boxes_c)
        res = InstanceData()
        n = int(boxes.shape[0])                                        # = n_kept, known on the host
        with phase('filter + NMS'):
            if n:
                # one NMS over all crops (candidates are numbered crop-major, then point, then mask: ties go to the lower
                # number); its count comes to the host together with the survivors' crops, in ONE read
                r = ops.batched_nms((boxes.view(1, n, 4), scores.view(1, n), torch.zeros((1, n), dtype=torch.int32, device=dev),
                                     torch.arange(n, dtype=torch.int32, device=dev).view(1, n),
                                     torch.full((1,), n, dtype=torch.int32, device=dev)), 1, n, float(self.crops_nms_thresh), n)
                order_all = r['keep'][0].clamp(0, n - 1).to(torch.int64)
                packed = torch.cat([r['count'].to(torch.int32), crop[order_all]]).cpu()
                m = int(packed[0])
                order, crop_h = order_all[:m], packed[1:1 + m].tolist()
            else:
                order, crop_h = torch.zeros((0,), dtype=torch.int64, device=dev), []
        res.bboxes, res.scores, res.crop_index = boxes[order], scores[order], crop[order].to(torch.int64)
        if self.min_mask_region_area:
            with phase('small regions'):
                if crop_h:
                    # first pass over the crop groups: the masks are cleaned and only their 8 integers kept; the second NMS
                    # decides who stays, and _masks below builds (and cleans) those again for their run lengths
                    info = self._masks(low, order, crop_h, boxes_c, geo, (H, W), dev, info_only=True)
                    kept, boxes2, changed = _region_nms(info, geo_t[crop[order].to(torch.int64), 6:8], self.crops_nms_thresh)
                    crop_h = [crop_h[i] for i in kept]
                    kept = torch.tensor(kept, dtype=torch.int64).to(dev)
                    order = order[kept]
                    res.region_changed = changed[kept]
                    res.bboxes = torch.where(res.region_changed[:, None], boxes2[kept], res.bboxes[kept])
                    res.scores, res.crop_index = res.scores[kept], res.crop_index[kept]
                else:
                    res.region_changed = torch.zeros((0,), dtype=torch.bool, device=dev)
        if _stages is not None:
            _stages['final'] = cand[order]
        with phase('masks + run lengths'):
            res.masks = self._masks(low, order, crop_h, boxes_c, geo, (H, W), dev)
        return res

    def _masks(self, low, order, crop_h, boxes_c, geo, hw, dev, info_only=False):
        """full-resolution masks of the NMS survivors, grouped by crop: rsp_mask_post_logits on the crop's geometry (cleaned by
        rsp_mask_remove_small_regions with min_mask_region_area > 0), then the run lengths of the crop-sized mask shifted into
        the image in the run domain (rsp_mask_rle -> rsp_rle_shift), or the dense paste (rsp_paste_tiles); put back in NMS
        order.  info_only: nothing but the cleaning's info int32 [m, 8] per survivor (crop-local boxes), no host read"""
        H, W = hw
        m = len(crop_h)
        area = self.min_mask_region_area
        info = torch.zeros((m, 8), dtype=torch.int32, device=dev) if info_only else None
        dense = torch.zeros((m, H, W), dtype=torch.bool, device=dev) if self.output == 'dense' and not info_only else None
        rles = [None] * m
        pending = []                                                   # (positions, counts, n) per launched group
        for c in sorted(set(crop_h)):
            pos_all = [i for i, cc in enumerate(crop_h) if cc == c]
            S0, S1, nh, nw, ch, cw, x0, y0 = geo[c][:8]
            whole = (ch, cw) == (H, W)
            for b0 in range(0, len(pos_all), self.mask_batch):
                pos = pos_all[b0:b0 + self.mask_batch]
                pos_t = torch.tensor(pos, dtype=torch.int64).to(dev)
                mk = ops.mask_post_logits(low[order[pos_t]].contiguous(), (S0, S1), (nh, nw), (ch, cw), self.mask_threshold)
                if area:
                    mk, inf = ops.remove_small_regions(mk, area)
                    if info_only:
                        info[pos_t] = inf
                        continue
                if dense is not None:
                    if whole:
                        dense[pos_t] = mk
                    else:
                        off = torch.tensor([[x0, y0]] * len(pos), dtype=torch.int32).to(dev)
                        dense[pos_t] = ops.paste_tiles(mk, off, (H, W))
                elif whole:
                    for i, d in zip(pos, rle.encode_mask_dicts(mk)):
                        rles[i] = d
                else:
                    pending.append((pos, mk, (x0, y0), (ch, cw)))
        if info_only:
            return info
        if dense is not None:
            return dense
        for pos, mk, (x0, y0), chw in pending:
            off = torch.tensor([[x0, y0]] * len(pos), dtype=torch.int32).to(dev)
            counts, n, _, _ = rle.encode_runs(mk)
            sc, _, sn_h, _ = rle.shift_runs(counts, n, off, chw, (H, W))
            for i, d in zip(pos, rle.runs_to_dicts(sc, sn_h, (H, W))):
                rles[i] = d
        return rles
