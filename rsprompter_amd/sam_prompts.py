"""Promptable SAM for callers: `SamSession` (one image embedding, any number of point / box / mask prompts),
`inference_prompts` (the one-shot form) and `generate_masks` (HF's mask-generation pipeline for the whole image).

What it restates: HF `SamImageProcessor` / `SamProcessor` (transformers models/sam/image_processing_sam.py:
`_get_preprocess_shape`, `_normalize_coordinates`, `post_process_masks`, `_build_point_grid`, `filter_masks`,
`_compute_stability_score`, `_batched_mask_to_box`, `_mask_to_rle`, `_post_process_for_mask_generation`) around
`SamModel.forward`.  What runs where: resize + normalise + pad is `rsp_resize_pad`, the ViT the encoder kernels, the prompts
`rsp_sam_embed_prompts`, the decoder `SamMaskDecoderHIP.decode`, full-resolution masks `rsp_mask_post_logits`, candidate
scoring `rsp_mask_score_box` (no full-resolution field is ever stored for a candidate that is not kept), run lengths
`rsp_mask_rle`, NMS `rsp_batched_nms`.  The host sees prompt coordinates, the kept count and the final results."""
import numpy as np
import torch

from . import ops
from .structures import InstanceData

# SamImageProcessor defaults (IMAGENET_DEFAULT_MEAN / STD on a 0..1 image, i.e. these on 0..255)
PIXEL_MEAN = (0.485 * 255, 0.456 * 255, 0.406 * 255)
PIXEL_STD = (0.229 * 255, 0.224 * 255, 0.225 * 255)


def _sam_of(model):
    """`SamModelHIP` of a SamModelHIP / RSSamModel / SAMDet."""
    for path in ((), ('sam_model',), ('segmentor', 'sam_model'), ('segmentor',)):
        m = model
        for p in path:
            m = getattr(m, p, None)
            if m is None:
                break
        if m is not None and hasattr(m, 'mask_decoder') and hasattr(m, 'prompt_encoder') and hasattr(m, 'vision_encoder'):
            return m
    raise TypeError(f'{type(model).__name__}: expected a SamModelHIP, an RSSamModel or a SAMDet')


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
    HF's processor where the image is strongly minified."""

    def __init__(self, model, image):
        self.sam = _sam_of(model)
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
            self.image_embeddings = self.sam.get_image_embeddings(self.pixel_values)
        self.device = dev

    def _low_res(self, points, labels, boxes, mask_input, multimask_output):
        dev = self.device
        n = None
        kw = {}
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
                mask_threshold=0.0):
        """points [Pb, P, 2] / labels [Pb, P] (1 foreground, 0 background, -1 padding) / boxes [Pb, 4], all in original pixels;
        mask_input: [256, 256] low-resolution logits of an earlier call (shared by the prompt sets).  Returns
        (masks bool [Pb, C, H, W] -- the fp32 values with return_logits --, iou_scores [Pb, C], low_res_logits
        [Pb, C, 256, 256]); C = 3 with multimask_output, else 1."""
        low, iou = self._low_res(points, labels, boxes, mask_input, multimask_output)
        Pb, C, h, w = low.shape
        H, W = self.original_size
        flat = low.reshape(Pb * C, h, w)
        if return_logits:
            masks = self.full_res(flat, mask_threshold, want_val=True)[1]
        else:
            masks = self.full_res(flat, mask_threshold)
        return masks.view(Pb, C, H, W), iou, low


def inference_prompts(model, image, **prompts):
    """One-shot `SamSession(model, image).predict(**prompts)`."""
    return SamSession(model, image).predict(**prompts)


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


def _rle_dicts(masks):
    """bool [k, H, W] on the device -> HF `_mask_to_rle` dicts: uncompressed column-major run lengths, first run zeros."""
    k, H, W = masks.shape
    counts, n = ops.mask_rle_counts(masks)
    counts, n = counts.cpu().numpy(), n.cpu().tolist()
    return [dict(size=[H, W], counts=counts[i, :n[i]].tolist()) for i in range(k)]


@torch.no_grad()
def generate_masks(model, image, points_per_side=32, pred_iou_thresh=0.88, stability_score_thresh=0.95,
                   stability_score_offset=1.0, mask_threshold=0.0, crops_nms_thresh=0.7, crop_n_layers=0, output='rle',
                   mask_batch=64, session=None, _stages=None):
    """HF's mask generation (`MaskGenerationPipeline` over `SamImageProcessor.generate_crop_boxes` / `filter_masks` /
    `post_process_for_mask_generation`) for the whole image as one crop: a points_per_side^2 grid of single-point prompts,
    three masks each, filtered by predicted IoU and stability score, NMS on the mask boxes.  Returns `InstanceData` in NMS
    order: bboxes fp32 [k, 4] (x0, y0, x1, y1, inclusive maxima as HF's `_batched_mask_to_box`), scores fp32 [k] (predicted
    IoU), masks = list of uncompressed RLE dicts (output='rle') or bool [k, H, W] (output='dense').
    session: an existing `SamSession` of the image (then `model` / `image` are not read); mask_batch: full-resolution masks
    built per kernel call; _stages: a dict that receives the stage tensors (candidate logits, IoU, scores, kept indices,
    boxes) -- the stage-wise parity tests read them."""
    if crop_n_layers:
        raise NotImplementedError('generate_masks: crop_n_layers > 0 (multi-crop generation) is not implemented; '
                                  'the image is processed as one crop')
    if output not in ('rle', 'dense'):
        raise ValueError("output must be 'rle' or 'dense'")
    s = session if session is not None else SamSession(model, image)
    H, W = s.original_size
    S = s.sam.image_size
    # HF _generate_crop_boxes: grid * (W, H) of the crop (= the image), then _normalize_coordinates inside predict
    pts = point_grid(points_per_side) * np.array([[W, H]], dtype=np.float64)
    low, iou = s._low_res(pts[:, None, :], None, None, None, True)
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
    dense, rles = [], []
    for i in range(0, int(sel.shape[0]), mask_batch):
        m = s.full_res(low[sel[i:i + mask_batch]], mask_threshold)
        if output == 'dense':
            dense.append(m)
        else:
            rles.extend(_rle_dicts(m))
    if output == 'dense':
        res.masks = torch.cat(dense, 0) if dense else torch.zeros((0, H, W), dtype=torch.bool, device=low.device)
    else:
        res.masks = rles
    return res
