"""-m gpu: multi-crop SAM mask generation ("crop layers") -- the two kernels (rsp_crops_resize_pad,
rsp_mask_score_box_crops) at full size, `SamMaskGenerator`'s merge on a constructed scene of discs around a stub decoder,
and the live ViT-B model per crop against HF `SamModel` on the CPU.  The oracle is HF's helpers
(transformers.models.sam.image_processing_pil_sam) composed per crop: `_generate_per_layer_crops`, `_build_point_grid`,
`_normalize_coordinates`, `_compute_stability_score`, `_batched_mask_to_box`, `_is_box_near_crop_edge`, `_pad_masks`,
`_mask_to_rle`, one NMS over all crops.  The check_* / oracle functions are shared with tests/test_sam_multicrop_cpu.py,
where `ops` is the emulated module and the device the CPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_gpu_sam_prompts import _err, _hf_helpers, _models, _smooth  # noqa: E402


def _post_s(low, S, nhw, ohw):
    """test_gpu_sam_prompts._post for any model input size S: post_process_masks' values for [k, S/4, S/4] logits"""
    m = F.interpolate(low[:, None], size=(S, S), mode='bilinear', align_corners=False)[..., :nhw[0], :nhw[1]]
    return F.interpolate(m, size=ohw, mode='bilinear', align_corners=False)[:, 0]


def _shape(hw, S):
    from transformers.models.sam.image_processing_pil_sam import SamImageProcessorPil
    return tuple(SamImageProcessorPil._get_preprocess_shape(None, hw, S))


def _test_image(hw, seed=33):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    return (F.interpolate(torch.rand(1, 3, max(H // 15, 2), max(W // 15, 2), generator=g), size=(H, W), mode='bicubic',
                          align_corners=False)[0].clamp(0, 1) * 255).permute(1, 2, 0).to(torch.uint8).contiguous()


# ------------------------------------------------------------------------------------------------- 1. crop front end
def check_crops_resize_pad(ops, dev, hw, S, boxes, identity=True):
    """crop i of ONE launch == resize_pad of the contiguous crop, bit for bit; uint8 and fp32 images, with and without the
    fused normalisation.  `boxes` holds at least three distinct sizes and (identity) one whose resize is the identity."""
    from rsprompter_amd.sam_prompts import PIXEL_MEAN, PIXEL_STD
    img8 = _test_image(hw)
    sizes = {(b[3] - b[1], b[2] - b[0]) for b in boxes}
    table = [[x0, y0, x1, y1, *_shape((y1 - y0, x1 - x0), S)] for x0, y0, x1, y1 in boxes]
    assert len(sizes) >= 3 and (not identity or any((t[3] - t[1], t[2] - t[0]) == (t[4], t[5]) for t in table))
    tab = torch.tensor(table, dtype=torch.int32).to(dev)
    for img in (img8, img8.to(torch.float32) * 0.731 + 3.0):
        for nrm in ((PIXEL_MEAN, PIXEL_STD, False), None, (PIXEL_MEAN, PIXEL_STD, True)):
            got = ops.crops_resize_pad(img.to(dev), tab, (S, S), PIXEL_MEAN, normalise=nrm)
            assert tuple(got.shape) == (len(boxes), 3, S, S) and got.dtype == torch.float32
            for i, (x0, y0, x1, y1, nh, nw) in enumerate(table):
                want = ops.resize_pad(img[y0:y1, x0:x1].contiguous().to(dev), (nh, nw), (S, S), PIXEL_MEAN, normalise=nrm)
                assert torch.equal(got[i], want), (img.dtype, nrm is not None, table[i])
    print(f'crops_resize_pad: {len(boxes)} crops of {len(sizes)} sizes of a {hw} image -> {S}^2, equal to resize_pad per crop')
    return tab


def check_crops_resize_pad_refusals(ops, dev):
    img = _test_image((40, 60)).to(dev)
    tab = torch.tensor([[0, 0, 60, 40, 21, 32]], dtype=torch.int32).to(dev)
    with pytest.raises(ValueError):
        ops.crops_resize_pad(img, tab.to(torch.int64), (32, 32))
    with pytest.raises(ValueError):
        ops.crops_resize_pad(img, tab[:, :5], (32, 32))
    with pytest.raises(ValueError):
        ops.crops_resize_pad(img[:, :, :2], tab, (32, 32))
    assert tuple(ops.crops_resize_pad(img, tab[:0], (32, 32)).shape) == (0, 3, 32, 32)
    # a box outside the image and a resized size outside the canvas are clamped by the kernel: nothing outside is touched
    wild = torch.tensor([[-5, -7, 1000, 1000, 99, 99]], dtype=torch.int32).to(dev)
    guard = torch.full((3, 3, 32, 32), 7.0).to(dev)
    ops.crops_resize_pad(img, wild, (32, 32), out=guard[1:2])
    assert float(guard[0].min()) == 7.0 == float(guard[2].max())
    assert torch.equal(guard[1], ops.resize_pad(img, (32, 32), (32, 32)))


# ------------------------------------------------------------------------------------------------- 2. scoring kernel
def _disc_logits(base, n, g):
    """n low-resolution logit maps [n, base, base]: discs in the middle and against each side, an empty and a full map"""
    yy, xx = torch.meshgrid(torch.arange(float(base)), torch.arange(float(base)), indexing='ij')
    b = float(base)
    spots = [(0.5, 0.5, 0.18), (0.06, 0.5, 0.1), (0.5, 0.05, 0.09), (0.95, 0.45, 0.1), (0.55, 0.96, 0.08), (0.3, 0.3, 0.22),
             (0.75, 0.7, 0.12)]
    out = torch.empty(n, base, base)
    for i in range(n):
        cx, cy, r = spots[i % len(spots)]
        jit = (torch.rand(3, generator=g) - 0.5) * 0.04
        out[i] = (((r + float(jit[2]) * 0.5) * b) - ((xx - (cx + float(jit[0])) * b) ** 2 + (yy - (cy + float(jit[1])) * b) ** 2).sqrt()) \
            .clamp(-32, 32)
    out = out + _smooth(g, n, 1, base, base, k=5)[:, 0] * 0.3
    out[n - 2] = -30.0
    out[n - 1] = 30.0
    return out


def score_table(hw, S, boxes):
    H, W = hw
    rows = []
    for x0, y0, x1, y1 in boxes:
        nh, nw = _shape((y1 - y0, x1 - x0), S)
        rows.append([S, S, nh, nw, y1 - y0, x1 - x0, x0, y0, x1, y1, W, H])
    return rows


def check_score_crops_kernel(ops, dev, hw, S, boxes, per_crop=9, thr=0.0, off=1.0, seed=17):
    """per crop: columns 0-2 == mask_score_box on that crop's slice, 3-6 == its box + (x0, y0, x0, y0), 7 ==
    HF _is_box_near_crop_edge; candidates of the crops interleaved, so that neighbouring blocks differ in geometry"""
    ip = _hf_helpers()
    H, W = hw
    base = S // 4
    rows = score_table(hw, S, boxes)
    ident = [(r[2], r[3]) == (r[4], r[5]) for r in rows]
    assert any(i and r[5] % 4 == 0 for i, r in zip(ident, rows)), 'an identity geometry with a 4-divisible width (strip form)'
    assert any(i and r[5] % 2 == 1 for i, r in zip(ident, rows)), 'an identity geometry with an odd width'
    assert any(not i for i in ident)
    assert any(r[6] == 0 for r in rows[1:]) and any(r[7] == 0 for r in rows[1:]) and any(r[8] == W for r in rows[1:]) and \
        any(r[9] == H for r in rows[1:]), 'a crop touching each image edge'
    g = torch.Generator().manual_seed(seed)
    C = len(boxes)
    low = torch.stack([_disc_logits(base, per_crop, g) for _ in range(C)], 1).reshape(per_crop * C, base, base).contiguous()
    cidx = torch.arange(C, dtype=torch.int32).repeat(per_crop)                       # candidate m belongs to crop m % C
    tab = torch.tensor(rows, dtype=torch.int32).to(dev)
    got = ops.mask_score_box_crops(low.to(dev), cidx.to(dev), tab, (max(r[4] for r in rows), max(r[5] for r in rows)), thr, off).cpu()
    assert got.dtype == torch.int32 and tuple(got.shape) == (per_crop * C, 8)
    flags = empties = 0
    for c, r in enumerate(rows):
        sel = (cidx == c).nonzero()[:, 0]
        one = ops.mask_score_box(low[sel].contiguous().to(dev), (S, S), (r[2], r[3]), (r[4], r[5]), thr, off).cpu()
        assert torch.equal(got[sel, :3], one[:, :3]), (c, r)
        shift = torch.tensor([[r[6], r[7], r[6], r[7]]], dtype=torch.int32)
        assert torch.equal(got[sel, 3:7], one[:, 3:7] + shift), (c, r)
        near = ip._is_box_near_crop_edge(one[:, 3:7].long(), r[6:10], [0, 0, W, H])
        assert torch.equal(got[sel, 7].bool(), near), (c, r, got[sel].tolist())
        flags += int(near.sum())
        empties += int((one[:, 2] == 0).sum())
        assert set(got[sel, 7].tolist()) <= {0, 1}
    assert 0 < flags < per_crop * C and empties >= C                                 # both flag values occur; an empty mask per crop
    assert not bool(got[cidx == 0, 7].any())                                         # crop 0 is the image: no crop edge inside it
    print(f'score_box_crops: {per_crop * C} candidates of {C} crops of a {hw} image, S = {S}: counts, boxes and {flags} near-edge '
          f'flags agree')
    return low, cidx, tab, rows


def check_score_crops_refusals(ops, dev):
    low = torch.zeros(4, 8, 8).to(dev)
    tab = torch.tensor([[32, 32, 32, 32, 16, 16, 0, 0, 16, 16, 40, 40]] * 2, dtype=torch.int32).to(dev)
    idx = torch.tensor([0, 1, 1, 0], dtype=torch.int32).to(dev)
    assert tuple(ops.mask_score_box_crops(low, idx, tab, (16, 16)).shape) == (4, 8)
    assert tuple(ops.mask_score_box_crops(low[:0], idx[:0], tab, (16, 16)).shape) == (0, 8)             # K = 0
    for bad_idx in (idx.to(torch.int64), idx[:3], idx.reshape(2, 2)):
        with pytest.raises(ValueError):
            ops.mask_score_box_crops(low, bad_idx, tab, (16, 16))
    for bad_tab in (tab.to(torch.int64), tab[:, :7], tab[:0], tab.reshape(-1)):
        with pytest.raises(ValueError):
            ops.mask_score_box_crops(low, idx, bad_tab, (16, 16))
    for out_of_range in ([0, 2, 1, 0], [0, -1, 1, 0]):
        with pytest.raises(ValueError):
            ops.mask_score_box_crops(low, torch.tensor(out_of_range, dtype=torch.int32).to(dev), tab, (16, 16))
    with pytest.raises(ValueError):
        ops.mask_score_box_crops(low[:, :, ::2], idx, tab, (16, 16))                                   # not contiguous
    with pytest.raises(ValueError):
        ops.mask_score_box_crops(low.to(torch.float64), idx, tab, (16, 16))
    if dev.type != 'cpu':
        with pytest.raises(ValueError):
            ops.mask_score_box_crops(low, idx.cpu(), tab, (16, 16))                                    # device mismatch
        with pytest.raises(ValueError):
            ops.mask_score_box_crops(low, idx, tab.cpu(), (16, 16))


# --------------------------------------------------------------------------------------------------- 3. the merge
class DiscSam(torch.nn.Module):
    """A stub of `SamModelHIP` on a constructed scene (the `_StubSession` idea of tests/test_sam_prompts_cpu.py one level
    down, so that `SamMaskGenerator`, `SamSession` and `generate_masks` all run around it): N discs in IMAGE coordinates; for a
    prompt point the disc minimising distance - radius at radius x (0.85, 1.0, 1.2), logit clamp(r - dist, -32, 32) at the image
    position of each low-resolution pixel of that crop, predicted IoU (0.90, 0.95, 0.86) + 1e-3 crop - 1e-5 disc.  It also
    checks what the generator hands over: every crop's pixel values (== resize_pad of the contiguous crop) and prompt points
    (== HF's grid of that layer, normalised to the crop's own input size)."""

    def __init__(self, ops, dev, S, image, crop_boxes, ndisc, rad_scale=1.0):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1, device=dev))
        self.mask_decoder = self.prompt_encoder = self.vision_encoder = types.SimpleNamespace(D=None)
        self.image_size, self.ops, self.dev, self.image, self.boxes = S, ops, dev, image, crop_boxes
        H, W = image.shape[:2]
        g = torch.Generator().manual_seed(5)
        self.cx = torch.rand(ndisc, generator=g) * W
        self.cy = torch.rand(ndisc, generator=g) * H
        self.rad = (12 + torch.rand(ndisc, generator=g) * 48) * rad_scale
        self.next, self.by_crop, self.calls = 0, {}, []

    def get_image_embeddings(self, pv):
        from rsprompter_amd.sam_prompts import PIXEL_MEAN, PIXEL_STD
        S = self.image_size
        B = pv.shape[0]
        assert tuple(pv.shape) == (B, 3, S, S)
        for b in range(B):
            x0, y0, x1, y1 = self.boxes[self.next + b]
            want = self.ops.resize_pad(self.image[y0:y1, x0:x1].contiguous().to(self.dev), _shape((y1 - y0, x1 - x0), S), (S, S),
                                       PIXEL_MEAN, normalise=(PIXEL_MEAN, PIXEL_STD, False))
            assert torch.equal(pv[b], want), ('pixel values of crop', self.next + b)
        ids = torch.arange(self.next, self.next + B)
        self.next += B
        return ids

    def crop_candidates(self, ci, npts):
        """(low [npts^2 * 3, S/4, S/4], iou [npts^2 * 3], disc per candidate) of crop ci on the CPU"""
        if (ci, npts) not in self.by_crop:
            ip = _hf_helpers()
            S = self.image_size
            x0, y0, x1, y1 = self.boxes[ci]
            ch, cw = y1 - y0, x1 - x0
            nh, nw = _shape((ch, cw), S)
            grid = ip._build_point_grid(npts) * np.array([[cw, ch]])
            px, py = torch.tensor(grid[:, 0] + x0).float(), torch.tensor(grid[:, 1] + y0).float()
            d = ((px[:, None] - self.cx[None]) ** 2 + (py[:, None] - self.cy[None]) ** 2).sqrt() - self.rad[None]
            di = d.argmin(1)
            u = (torch.arange(S // 4).float() + 0.5) * 4 - 0.5              # input pixel of a low-resolution pixel centre
            X = x0 + (u + 0.5) * (cw / nw) - 0.5
            Y = y0 + (u + 0.5) * (ch / nh) - 0.5
            low = torch.empty(npts * npts, 3, S // 4, S // 4)
            iou = torch.empty(npts * npts, 3)
            for c, (f, s) in enumerate(((0.85, 0.90), (1.0, 0.95), (1.2, 0.86))):
                r = self.rad[di] * f
                dist = ((X[None, None, :] - self.cx[di][:, None, None]) ** 2 + (Y[None, :, None] - self.cy[di][:, None, None]) ** 2).sqrt()
                low[:, c] = (r[:, None, None] - dist).clamp(-32, 32)
                iou[:, c] = s + 1e-3 * ci - 1e-5 * di.float()
            self.by_crop[(ci, npts)] = (low.flatten(0, 1), iou.flatten(), di.repeat_interleave(3), grid)
        return self.by_crop[(ci, npts)]

    def forward(self, image_embeddings=None, input_points=None, input_labels=None, multimask_output=True):
        ip = _hf_helpers()
        S = self.image_size
        B, Pb = input_points.shape[:2]
        assert multimask_output is True and tuple(input_points.shape) == (B, Pb, 1, 2) and image_embeddings.shape[0] == B
        assert tuple(input_labels.shape) == (B, Pb, 1) and bool((input_labels == 1).all())
        npts = int(round(Pb ** 0.5))
        lows, ious = [], []
        for b in range(B):
            ci = int(image_embeddings[b])
            x0, y0, x1, y1 = self.boxes[ci]
            low, iou, _, grid = self.crop_candidates(ci, npts)
            want = torch.from_numpy(ip._normalize_coordinates(S, grid, (y1 - y0, x1 - x0))).float()
            assert torch.equal(input_points[b, :, 0].cpu(), want), ('prompt points of crop', ci)
            lows.append(low.view(Pb, 3, S // 4, S // 4))
            ious.append(iou.view(Pb, 3))
            self.calls.append((ci, npts))
        return types.SimpleNamespace(pred_masks=torch.stack(lows).to(self.dev), iou_scores=torch.stack(ious).to(self.dev))


def oracle_multicrop(cands, crop_boxes, hw, S, t_iou, t_st, thr, off, nms_thr, want_masks=True):
    """HF's helpers per crop on the CPU.  cands: per crop (low [k, S/4, S/4], iou [k]).  Returns a dict: per candidate (crop-major
    numbering) iou, keep, undecided, near-edge flag, image-frame box; the NMS's final list; per final instance the RLE of the
    padded mask and whether a pixel of it lies within 1e-4 of the threshold; the figures of the issue's table."""
    from oracle import cops
    ip = _hf_helpers()
    H, W = hw
    rows = []
    for ci, ((x0, y0, x1, y1), (low, iou)) in enumerate(zip(crop_boxes, cands)):
        ch, cw = y1 - y0, x1 - x0
        nhw = _shape((ch, cw), S)
        st, sp, sm, bx, bp, bm = [], [], [], [], [], []
        for i in range(0, low.shape[0], 64):
            val = _post_s(low[i:i + 64], S, nhw, (ch, cw))
            st.append(ip._compute_stability_score(val, thr, off))
            sp.append(ip._compute_stability_score(val + 1e-4, thr, off))
            sm.append(ip._compute_stability_score(val - 1e-4, thr, off))
            bx.append(ip._batched_mask_to_box(val > thr))
            bp.append(ip._batched_mask_to_box(val > thr + 1e-4))
            bm.append(ip._batched_mask_to_box(val > thr - 1e-4))
        st, sp, sm, bx, bp, bm = map(torch.cat, (st, sp, sm, bx, bp, bm))
        cb, ob = [x0, y0, x1, y1], [0, 0, W, H]
        ne, nep, nem = (ip._is_box_near_crop_edge(b, cb, ob) for b in (bx, bp, bm))
        und = (nep != ne) | (nem != ne) | ((sp > t_st) != (st > t_st)) | ((sm > t_st) != (st > t_st)) | ((iou - t_iou).abs() < 1e-3)
        rows.append(dict(ci=torch.full((low.shape[0],), ci, dtype=torch.int64), iou=iou, st=st, ne=ne, und=und,
                         box=(bx + torch.tensor([[x0, y0, x0, y0]])).float()))
    cat = {k: torch.cat([r[k] for r in rows]) for k in rows[0]}
    iou, st = cat['iou'], cat['st']
    keep0 = (iou > t_iou) & (st > t_st)
    keep = keep0 & ~cat['ne']
    ko = keep.nonzero()[:, 0]
    _, nk = cops.nms(cat['box'][ko], iou[ko], nms_thr)
    final = ko[nk]
    per_crop = 0
    for c in range(len(crop_boxes)):
        kc = ko[cat['ci'][ko] == c]
        if len(kc):
            per_crop += len(cops.nms(cat['box'][kc], iou[kc], nms_thr)[1])
    o = dict(K=iou.numel(), iou=iou, keep=keep, und=cat['und'], ne=cat['ne'], box=cat['box'], ci=cat['ci'], final=final,
             edge_only=int((keep0 & cat['ne']).sum()), cross=per_crop - len(nk), nan=int(st.isnan().sum()),
             crops_with_survivor=len(set(cat['ci'][final].tolist())))
    print(f"oracle {hw}, {len(crop_boxes)} crops: K {o['K']}, undecided {int(o['und'].sum())} "
          f"({100 * float(o['und'].float().mean()):.2f} %), removed by the near-edge rule alone {o['edge_only']}, kept {len(ko)}, "
          f"instances {len(final)}, crops with a survivor {o['crops_with_survivor']}, cross-crop suppressions {o['cross']}, "
          f"NaN stability {o['nan']}")
    if want_masks:
        starts = np.cumsum([0] + [c[0].shape[0] for c in cands])
        o['rle'], o['near_thr'] = [], []
        for f in final.tolist():
            ci = int(cat['ci'][f])
            x0, y0, x1, y1 = crop_boxes[ci]
            val = _post_s(cands[ci][0][f - starts[ci]][None], S, _shape((y1 - y0, x1 - x0), S), (y1 - y0, x1 - x0))
            o['rle'].append(ip._mask_to_rle(ip._pad_masks(val > thr, crop_boxes[ci], H, W))[0])
            o['near_thr'].append(bool(((val - thr).abs() < 1e-4).any()))
    return o


def assert_oracle_conditions(o):
    """what the issue asserts on the oracle alone, before anything is compared"""
    assert float(o['und'].float().mean()) <= 0.03
    assert bool((o['ci'][o['final']] != 0).any()), 'an instance from a crop other than crop 0'
    assert o['cross'] >= 1, 'a suppression across crops'
    assert o['edge_only'] >= 1, 'a candidate removed by the near-edge rule alone'


def compare_with_oracle(res, stages, o, hw, dense=None):
    """the assertions of the issue: kept set on decided candidates, final list, boxes, scores, crop_index, run lengths"""
    ip = _hf_helpers()
    H, W = hw
    kept_d = torch.zeros(o['K'], dtype=torch.bool)
    kept_d[stages['kept'].cpu()] = True
    dec = ~o['und']
    assert torch.equal(kept_d[dec], o['keep'][dec]), (kept_d != o['keep']).nonzero()[:, 0].tolist()
    final_d = stages['final'].cpu().tolist()
    final_o = o['final'].tolist()
    k = len(final_d)
    assert k == len(res.masks) == res.bboxes.shape[0] == res.scores.shape[0] == res.crop_index.shape[0] and k > 0
    assert res.crop_index.dtype == torch.int64 and res.bboxes.dtype == torch.float32
    same = torch.equal(kept_d, o['keep'])
    print(f'kept sets differ on {int((kept_d != o["keep"]).sum())} undecided candidates; {k} instances')
    if same:
        assert final_d == final_o
    pos_o = {c: i for i, c in enumerate(final_o)}
    common = [c for c in final_d if c in pos_o and bool(dec[c])]
    assert common
    exact = 0
    for i, c in enumerate(final_d):
        if c not in pos_o or not bool(dec[c]):
            continue
        assert res.bboxes[i].cpu().tolist() == o['box'][c].tolist(), c
        assert float(res.scores[i]) == float(o['iou'][c]) or stages.get('live'), c
        assert abs(float(res.scores[i]) - float(o['iou'][c])) < 2e-3
        assert int(res.crop_index[i]) == int(o['ci'][c])
        got, want = res.masks[i], o['rle'][pos_o[c]]
        assert got['size'] == [H, W] and sum(got['counts']) == H * W
        if not o['near_thr'][pos_o[c]] and not stages.get('live'):
            assert got == want, c
            exact += 1
        else:
            a, b = ip._rle_to_mask(got), ip._rle_to_mask(want)
            assert (a & b).sum() >= 0.999 * (a | b).sum(), c
        if dense is not None:
            assert np.array_equal(dense.masks[i].cpu().numpy(), ip._rle_to_mask(got)), c
    print(f'{len(common)} instances compared, run lengths of {exact} equal to _mask_to_rle(_pad_masks(...)) exactly')
    if dense is not None:
        assert dense.masks.dtype == torch.bool and tuple(dense.masks.shape) == (k, H, W)
        assert torch.equal(dense.bboxes, res.bboxes) and torch.equal(dense.crop_index, res.crop_index)


def run_merge_case(ops, dev, hw, S, layers, n, ndisc, down=1, rad_scale=1.0, t_iou=0.88, t_st=0.8, crop_batch=2):
    """one row of the issue's table: the stub scene through SamMaskGenerator (rle and dense) against the oracle"""
    from rsprompter_amd.apis import SamMaskGenerator
    ip = _hf_helpers()
    image = _test_image(hw)
    crop_boxes, layer_idxs = ip._generate_per_layer_crops(layers, 512 / 1500, hw)
    kw = dict(points_per_side=n, pred_iou_thresh=t_iou, stability_score_thresh=t_st, stability_score_offset=1.0, mask_threshold=0.0,
              crops_nms_thresh=0.7, crop_n_layers=layers, crop_n_points_downscale_factor=down, crop_batch=crop_batch)
    sam = DiscSam(ops, dev, S, image, crop_boxes, ndisc, rad_scale)
    cands = [sam.crop_candidates(ci, int(n / down ** layer_idxs[ci]))[:2] for ci in range(len(crop_boxes))]
    o = oracle_multicrop(cands, crop_boxes, hw, S, t_iou, t_st, 0.0, 1.0, 0.7)
    assert_oracle_conditions(o)
    gen = SamMaskGenerator(sam, **kw)
    assert gen.crop_boxes(hw) == crop_boxes
    st = {}
    res = gen.generate(image.numpy(), _stages=st)
    assert [c for c, _ in sam.calls] == list(range(len(crop_boxes)))                 # every crop once, in order
    sam2 = DiscSam(ops, dev, S, image, crop_boxes, ndisc, rad_scale)
    sam2.by_crop = sam.by_crop
    dense = SamMaskGenerator(sam2, output='dense', **dict(kw, crop_batch=3)).generate(image)
    compare_with_oracle(res, st, o, hw, dense)
    return o, res


# ------------------------------------------------------------------------------------------------------- GPU tests
SCORE_BOXES = [[0, 0, 1600, 1100], [320, 40, 1344, 808], [900, 60, 1515, 1084], [1000, 500, 1600, 1100], [0, 0, 700, 560],
               [300, 200, 1100, 900]]


@pytest.mark.quick
def test_crops_resize_pad(dev):
    from rsprompter_amd import ops
    ip = _hf_helpers()
    boxes, _ = ip._generate_per_layer_crops(2, 512 / 1500, (517, 803))              # nine distinct sizes
    check_crops_resize_pad(ops, dev, (517, 803), 1024, boxes, identity=False)
    check_crops_resize_pad(ops, dev, (1100, 1600), 1024, SCORE_BOXES)               # identity crops: 1024 x 768, 615 x 1024
    check_crops_resize_pad_refusals(ops, dev)


@pytest.mark.quick
def test_score_box_crops_kernel(dev):
    from rsprompter_amd import ops
    check_score_crops_kernel(ops, dev, (1100, 1600), 1024, SCORE_BOXES)
    check_score_crops_kernel(ops, dev, (1100, 1600), 1024, SCORE_BOXES, thr=0.5, off=0.25, seed=18)
    check_score_crops_refusals(ops, dev)


@pytest.mark.parametrize('case', ('600x900_one_layer', '517x803_two_layers'))
def test_merge_on_the_disc_scene(dev, case):
    """rows 1 and 2 of the issue's table (measured there with the reference helpers only: K 960 / 576, undecided 0 / 4, removed by
    the near-edge rule alone 97 / 96, kept 453 / 240, instances 36 / 33, crops with a survivor 4 of 5 / 15 of 21, cross-crop
    suppressions 39 / 49); the test prints the figures of its run"""
    from rsprompter_amd import ops
    if case == '600x900_one_layer':
        o, _ = run_merge_case(ops, dev, (600, 900), 1024, 1, 8, 40)
        assert o['K'] == 960 and o['nan'] > 0
    else:
        o, _ = run_merge_case(ops, dev, (517, 803), 1024, 2, 8, 40, down=2, crop_batch=5)
        assert o['K'] == 576


class _ReadCounter:
    """counts the calls through which this package's host code reads from the device: Tensor.item / nonzero / cpu / tolist"""

    def __enter__(self):
        self.n = {}
        self.saved = {k: getattr(torch.Tensor, k) for k in ('item', 'nonzero', 'cpu', 'tolist')}
        for k, fn in self.saved.items():
            def wrap(t, *a, _k=k, _fn=fn, **kw):
                if t.is_cuda:
                    self.n[_k] = self.n.get(_k, 0) + 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, wrap)
        return self

    def __exit__(self, *a):
        for k, fn in self.saved.items():
            setattr(torch.Tensor, k, fn)


def test_live_model_per_crop_against_hf(dev):
    """ViT-B, seeded weights, the 600 x 900 test image, one layer, 8 x 8 grid: per crop the candidate logits and IoU predictions
    against HF SamModel on the CPU embedding the device's own pixel values (< 2e-3, two ViT-B runs apart), scores / flags / kept
    set against the oracle on HF's logits (thresholds at the medians, offset 0.25, undecided <= 3 %), the scoring call's peak
    allocation, the host reads of generate(), and crop_n_layers=0 == generate_masks bit for bit."""
    from rsprompter_amd import ops
    from rsprompter_amd.apis import SamMaskGenerator, generate_masks
    from rsprompter_amd.sam_prompts import PIXEL_MEAN, PIXEL_STD
    ip = _hf_helpers()
    hf, hip = _models(dev)
    hw, S, n, off = (600, 900), 1024, 8, 0.25
    image = _test_image(hw)
    crop_boxes, _ = ip._generate_per_layer_crops(1, 512 / 1500, hw)
    table = torch.tensor([[x0, y0, x1, y1, *_shape((y1 - y0, x1 - x0), S)] for x0, y0, x1, y1 in crop_boxes], dtype=torch.int32)
    pv = ops.crops_resize_pad(image.to(dev), table.to(dev), (S, S), PIXEL_MEAN, normalise=(PIXEL_MEAN, PIXEL_STD, False)).cpu()
    cands = []
    with torch.no_grad():
        for ci, (x0, y0, x1, y1) in enumerate(crop_boxes):
            E = hf.get_image_embeddings(pv[ci:ci + 1])
            grid = ip._build_point_grid(n) * np.array([[x1 - x0, y1 - y0]])
            pts = torch.from_numpy(ip._normalize_coordinates(S, grid, (y1 - y0, x1 - x0))).float()[None, :, None, :]
            out = hf(image_embeddings=E, input_points=pts, input_labels=torch.ones(1, n * n, 1, dtype=torch.int64), multimask_output=True)
            cands.append((out.pred_masks[0].flatten(0, 1), out.iou_scores[0].flatten()))
    iou_all = torch.cat([c[1] for c in cands])
    stab = torch.cat([ip._compute_stability_score(_post_s(low, S, _shape((b[3] - b[1], b[2] - b[0]), S), (b[3] - b[1], b[2] - b[0])),
                                                  0.0, off) for (low, _), b in zip(cands, crop_boxes)])
    t_iou, t_st = float(iou_all.median()), float(stab[~stab.isnan()].median())
    o = oracle_multicrop(cands, crop_boxes, hw, S, t_iou, t_st, 0.0, off, 0.7)
    assert float(o['und'].float().mean()) <= 0.03
    gen = SamMaskGenerator(hip, points_per_side=n, pred_iou_thresh=t_iou, stability_score_thresh=t_st, stability_score_offset=off,
                           crop_n_layers=1, crop_batch=2)
    st = {}
    gen.generate(image, _stages={})                                                  # warm: libraries, caches
    torch.cuda.synchronize()
    before_masks = {}
    masks_fn = gen._masks
    with _ReadCounter() as rc:
        gen._masks = lambda *a: (before_masks.update(rc.n), masks_fn(*a))[1]
        res = gen.generate(image, _stages=st)
    gen._masks = masks_fn
    n_batches = len(st['batches'])
    print(f'host reads of generate(): {before_masks} up to the NMS over {n_batches} crop batches, {rc.n} with the transfer of the '
          f'{len(res.masks)} results')
    # at most one read (the kept count: the compaction's size) per crop batch, plus ONE for the NMS (its count, with the survivors'
    # crops in the same transfer); none per crop.  What follows is the transfer of the results themselves (the run lengths).
    assert n_batches == 3 and before_masks == dict(nonzero=n_batches, cpu=1)
    # per crop: logits and IoU predictions
    low_d = torch.cat([b['low_res'].cpu() for b in st['batches']])
    iou_d = torch.cat([b['iou'].cpu() for b in st['batches']])
    score_d = torch.cat([b['score'].cpu() for b in st['batches']])
    k0 = 0
    for ci, (low, iou) in enumerate(cands):
        k1 = k0 + low.shape[0]
        el, ei = _err(low_d[k0:k1], low), _err(iou_d[k0:k1], iou)
        print(f'crop {ci} {crop_boxes[ci]}: low-res err {el:.2e}, iou err {ei:.2e}')
        assert el < 2e-3 and ei < 2e-3
        k0 = k1
    dec = ~o['und']
    assert torch.equal(score_d[dec, 7].bool(), o['ne'][dec])
    st['live'] = True
    compare_with_oracle(res, st, o, hw)
    # the scoring call writes no field: its peak allocation stays below its own input
    b = st['batches'][1]
    lowd = b['low_res'].contiguous()
    cidx = torch.arange(b['crops'][0], b['crops'][1], dtype=torch.int32, device=dev).repeat_interleave(lowd.shape[0] // 2)
    geo = torch.tensor(score_table(hw, S, crop_boxes), dtype=torch.int32).to(dev)
    ops.mask_score_box_crops(lowd[:4], cidx[:4], geo, hw, 0.0, off)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    sc = ops.mask_score_box_crops(lowd, cidx, geo, hw, 0.0, off, check_index=False)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print(f'mask_score_box_crops on {lowd.shape[0]} x 256^2: peak allocation grew by {grew} bytes (input {lowd.numel() * 4})')
    assert grew < lowd.numel() * 4 and torch.equal(sc, b['score'])
    # crop_n_layers = 0 is generate_masks, bit for bit
    kw = dict(points_per_side=n, pred_iou_thresh=t_iou, stability_score_thresh=t_st, stability_score_offset=off)
    for output in ('rle', 'dense'):
        a = SamMaskGenerator(hip, crop_n_layers=0, output=output, **kw).generate(image)
        w = generate_masks(hip, image, output=output, **kw)
        assert torch.equal(a.bboxes, w.bboxes) and torch.equal(a.scores, w.scores) and len(w.masks) > 0
        assert (a.masks == w.masks) if output == 'rle' else torch.equal(a.masks, w.masks)
        assert not bool(a.crop_index.any())
