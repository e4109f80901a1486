"""GPU: SAM-HQ (`SamHQModelHIP`, `SamHQMaskDecoderHIP`, rsp_sam_hq_mask) against transformers' `SamHQModel` in fp32 on the
CPU, and the fused mask-branch kernel against its composition from the package's older kernels and against fp64 torch.
Tolerance: the project's contract, 1e-3 absolute on mask logits and predicted IoU (tests/_sam_hq_ref.TOL)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _sam_hq_ref as ref

TOL = ref.TOL
H0, W0 = 96, 128


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('g,R', [(16, 5), (64, 2)])
def test_hq_mask_kernel_against_composition_and_fp64(dev, g, R):
    """g = 16: 16 tiles per prompt set, 5 prompt sets over 2 images; g = 64: the production grid (256 tiles per prompt set)"""
    from rsprompter_amd import ops
    c = ref.kernel_case(R, 2, g, seed=g + R)
    want = ref.kernel_ref_fp64(c)
    got = ref.kernel_run(ops, c, dev)
    comp = ref.kernel_composed(ops, c, dev)
    e64, ec, ecc = _err(got, want), _err(got, comp), _err(comp, want)
    print(f'rsp_sam_hq_mask g = {g}, R = {R}: vs fp64 {e64:.2e}, vs the composed kernels {ec:.2e} (those vs fp64 {ecc:.2e}); '
          f'|logit| up to {float(want.abs().max()):.1f}')
    assert tuple(got.shape) == (R, 4 * g, 4 * g)
    assert e64 < TOL and ec < TOL


def test_hq_mask_kernel_row_map_and_sam_outputs(dev):
    """`up` given once per image and read through the map; SAM's masks + mask_hq from the same tile (three hyper rows)"""
    from rsprompter_amd import ops
    from rsprompter_amd.necks import convt_weights4
    from rsprompter_amd.sam_decoder import hq_conv_weights
    R, S, g = 5, 2, 16
    c = ref.kernel_case(S, S, g, seed=7)
    gen = torch.Generator().manual_seed(8)
    rmap = torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32)
    hyper, hyper_sam = torch.randn(R, 32, generator=gen), torch.randn(R, 3, 32, generator=gen)
    full = dict(c, R=R, up=c['up'][rmap.long()], hyper=hyper, map=rmap)
    want_hq = ref.kernel_ref_fp64(full)
    u = F.gelu(F.conv_transpose2d(full['up'].double().permute(0, 3, 1, 2), c['ct_w'].double(), c['ct_b'].double(), stride=2))
    want_sam = torch.einsum('rtc,rchw->rthw', hyper_sam.double(), u) + want_hq[:, None]
    t = lambda x: x.to(dev).contiguous()
    w2, b2 = convt_weights4(t(c['ct_w']), t(c['ct_b']))
    w1, wf = hq_conv_weights(t(c['c1_w']), t(c['c2_w']))
    hq, sam = ops.sam_hq_mask(ops.to_planes(t(c['up'])), w2, b2, w1, t(c['c1_b']), t(c['ln_w']), t(c['ln_b']), 1e-6, wf,
                              t(c['c2_b']), t(hyper), t(c['feat']), t(rmap), up_map=t(rmap), hyper_sam=t(hyper_sam))
    e_hq, e_sam = _err(hq, want_hq), _err(sam, want_sam)
    print(f'mapped up + SAM outputs: mask_hq {e_hq:.2e}, masks_sam + mask_hq {e_sam:.2e}')
    assert e_hq < TOL and e_sam < TOL


# ------------------------------------------------------------------------------------------------ the decoder
_DEC = {}


def _decoders(dev):
    if 'd' not in _DEC:
        from rsprompter_amd.sam_decoder import SamHQMaskDecoderHIP
        dec, sd = ref.hf_decoder()
        hip = SamHQMaskDecoderHIP()
        hip.load_state_dict(sd, strict=True)
        _DEC['d'] = (dec, hip.to(dev).eval())
    return _DEC['d']


@pytest.mark.parametrize('seed', [0, 1])
@pytest.mark.parametrize('multimask,hq_only', [(False, False), (False, True), (True, False), (True, True)])
def test_hq_decoder_against_hf(dev, seed, multimask, hq_only):
    """g = 16, B = 2 images x 8 prompt sets of two sparse tokens, a random intermediate feature.  With multimask_output the
    masks and scores must come in HF's sorted order for EVERY prompt set."""
    dec, hip = _decoders(dev)
    emb, pe, sparse, dense, inter = ref.decoder_case(2, 8, 2, 16, seed)
    want_m, want_i = ref.hf_decode(dec, emb, pe, sparse, dense, inter, multimask, hq_only)
    d = lambda x: x.to(dev)
    got_m, got_i, _ = hip(d(emb), d(pe), d(sparse), d(dense), multimask_output=multimask, hq_token_only=hq_only,
                          intermediate_embeddings=[d(inter)])
    em, ei = _err(got_m, want_m), _err(got_i, want_i)
    print(f'HQ decoder seed {seed} multimask {multimask} hq_token_only {hq_only}: masks {em:.2e} (|logit| up to '
          f'{float(want_m.abs().max()):.1f}), iou {ei:.2e}, smallest sorted-IoU gap {ref.min_sorted_gap(want_i):.4f}')
    assert ref.min_sorted_gap(want_i) > ref.MIN_GAP                    # the order compared below is well defined
    assert tuple(got_m.shape) == tuple(want_m.shape) and tuple(got_i.shape) == tuple(want_i.shape)
    assert em < TOL and ei < TOL


def test_hq_decoder_without_intermediates_and_with_a_dense_prompt(dev):
    """HF:974-975 (only the embedding's half of hq_features) and a per-pixel dense prompt: hq_features must be formed from
    the image embedding BEFORE the dense prompt is added, the upscaled embedding from their sum"""
    dec, hip = _decoders(dev)
    emb, pe, sparse, dense, inter = ref.decoder_case(2, 8, 2, 16, 2)
    d = lambda x: x.to(dev)
    want_m, want_i = ref.hf_decode(dec, emb, pe, sparse, dense, None, True, False)
    got_m, got_i, _ = hip(d(emb), d(pe), d(sparse), d(dense), multimask_output=True, hq_token_only=False)
    e0 = (_err(got_m, want_m), _err(got_i, want_i))
    dense2 = torch.randn(2, 256, 16, 16, generator=torch.Generator().manual_seed(5))
    want_m, want_i = ref.hf_decode(dec, emb, pe, sparse, dense2, inter, True, False)
    got_m, got_i, _ = hip(d(emb), d(pe), d(sparse), d(dense2), multimask_output=True, hq_token_only=False,
                          intermediate_embeddings=[d(inter)])
    e1 = (_err(got_m, want_m), _err(got_i, want_i))
    print(f'no intermediates: masks {e0[0]:.2e}, iou {e0[1]:.2e}; per-pixel dense prompt: masks {e1[0]:.2e}, iou {e1[1]:.2e}')
    assert max(e0) < TOL and max(e1) < TOL


def test_hq_decode_memory_stays_near_plain_sam(dev):
    """g = 64, R = 64: peak memory of an HQ decode minus that of a plain SAM decode of the same prompts stays below
    4 x R x (4g)^2 x 4 B = 64 MiB (one materialised 32-channel tensor would be 512 MiB)"""
    from rsprompter_amd.sam_decoder import SamMaskDecoderHIP
    _, hq = _decoders(dev)
    _, sd = ref.hf_decoder()
    sam = SamMaskDecoderHIP()
    own = set(sam.state_dict())
    sam.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=True)
    sam = sam.to(dev).eval()
    g, R = 64, 64
    gen = torch.Generator().manual_seed(9)
    emb = torch.randn(1, 256, g, g, generator=gen).to(dev)
    pe = torch.randn(1, 256, g, g, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)   # as the model's table: no copy per call
    sparse = torch.randn(R, 2, 256, generator=gen).to(dev)
    dense = torch.randn(256, generator=gen).to(dev)
    roi = torch.zeros(R, dtype=torch.int32, device=dev)
    feat = hq.hq_features(emb, None)
    peaks = {}
    for multi in (False, True):
        for name, fn in (('sam', lambda n, m: sam.decode(emb, pe, sparse[:n], dense, roi[:n], multimask_output=m)),
                         ('hq', lambda n, m: hq.decode(emb, pe, sparse[:n], dense, roi[:n], multimask_output=m, hq_features=feat))):
            fn(2, multi)                                  # packing and per-table caches are not part of the decode
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn(R, multi)
            torch.cuda.synchronize()
            peaks[name, multi] = torch.cuda.max_memory_allocated() - base
            del out
    lim = 4 * R * (4 * g) ** 2 * 4
    for multi in (False, True):
        extra = peaks['hq', multi] - peaks['sam', multi]
        print(f'multimask {multi}: plain SAM decode peak {peaks["sam", multi] / 2 ** 20:.0f} MiB, HQ {peaks["hq", multi] / 2 ** 20:.0f} MiB, '
              f'difference {extra / 2 ** 20:.1f} MiB (limit {lim / 2 ** 20:.0f})')
        assert extra < lim


# ------------------------------------------------------------------------------------------------ the model and its callers
_PAIR = {}


def _models(dev):
    """HF SamHQModel('base') with the seeded weights and the HIP model holding the same tensors (HF ties the two Gaussian
    matrices: the HIP side loads HF's state_dict after HF loaded the seeded one)"""
    if 'pair' not in _PAIR:
        from rsprompter_amd.samdet import SamHQModelHIP
        hf, _ = ref.hf_model()
        hip = SamHQModelHIP('base')
        hip.load_state_dict(hf.state_dict(), strict=True)
        _PAIR['pair'] = (hf, hip.to(dev).eval())
    return _PAIR['pair']


@pytest.fixture(scope='module')
def scene(dev):
    """one live ViT-B run on each side (the CPU one takes seconds), shared by the model, session and generation tests"""
    from rsprompter_amd.apis import SamSession
    hf, hip = _models(dev)
    g = torch.Generator().manual_seed(34)
    img = (F.interpolate(torch.rand(1, 3, 12, 16, generator=g), size=(H0, W0), mode='bicubic', align_corners=False)[0]
           .clamp(0, 1) * 255).permute(1, 2, 0).to(torch.uint8).contiguous()
    s = SamSession(hip, img.numpy())
    pv = s.pixel_values.cpu()
    with torch.no_grad():
        E, inter = hf.get_image_embeddings(pv)
    return dict(img=img, session=s, pv=pv, E=E, inter=inter)


def _hf_call(hf, scene, pts, multi=True, hq_only=False, mask=None):
    kw = {} if mask is None else dict(input_masks=mask.reshape(1, 1, 256, 256))
    with torch.no_grad():
        o = hf(image_embeddings=scene['E'], intermediate_embeddings=scene['inter'], input_points=pts,
               input_labels=torch.ones(pts.shape[:3], dtype=torch.int64), multimask_output=multi, hq_token_only=hq_only, **kw)
    return o.pred_masks, o.iou_scores


def test_hq_model_end_to_end_and_session_cache(dev, scene):
    hf, hip = _models(dev)
    s = scene['session']
    e_emb, e_int = _err(s.image_embeddings, scene['E']), _err(s.intermediate_embeddings[0], scene['inter'][0])
    print(f'ViT-B: image embedding err {e_emb:.2e} (|x| up to {float(scene["E"].abs().max()):.1f}), intermediate (layer 2) err '
          f'{e_int:.2e} (|x| up to {float(scene["inter"][0].abs().max()):.1f})')
    assert tuple(s.intermediate_embeddings[0].shape) == (1, 64, 64, 768)
    assert e_emb < TOL and e_int < TOL
    pts = torch.tensor([[[[300.0, 200.0]], [[800.0, 500.0]]]])
    for multi, hq_only in ((True, False), (False, True)):
        want_m, want_i = _hf_call(hf, scene, pts, multi, hq_only)
        got = hip(pixel_values=s.pixel_values, input_points=pts.to(dev), multimask_output=multi, hq_token_only=hq_only)
        em, ei = _err(got.pred_masks, want_m), _err(got.iou_scores, want_i)
        print(f'pixel_values call (multimask {multi}, hq_token_only {hq_only}): pred_masks err {em:.2e} (|logit| up to '
              f'{float(want_m.abs().max()):.1f}), iou_scores err {ei:.2e}')
        assert tuple(got.pred_masks.shape) == tuple(want_m.shape) and tuple(got.iou_scores.shape) == tuple(want_i.shape)
        assert em < TOL and ei < TOL
    # HF's argument checks (HF:1424-1449)
    with pytest.raises(ValueError, match='Either pixel_values or image_embeddings'):
        hip(input_points=pts.to(dev))
    with pytest.raises(ValueError, match='4D tensor'):
        hip(image_embeddings=s.image_embeddings, input_points=pts[0].to(dev))
    # the session: two predicts on one image run the four hq_features ConvTransposes once
    hip._hq_cache = None
    n0 = hip.mask_decoder.hq_feature_calls
    p = np.array([[[40.0, 30.0]], [[100.0, 60.0]]])
    a = s.predict(points=p)
    b = s.predict(points=p[:1], multimask_output=False)
    assert hip.mask_decoder.hq_feature_calls == n0 + 1
    want_m, want_i = _hf_call(hf, scene, torch.from_numpy(p * (1024.0 / W0)).float()[None])
    el, ei = _err(a[2], want_m[0]), _err(a[1], want_i[0])
    print(f'SamSession.predict: low-res err {el:.2e}, iou err {ei:.2e}')
    assert el < TOL and ei < TOL and tuple(a[0].shape) == (2, 3, H0, W0) and tuple(b[0].shape) == (1, 1, H0, W0)
    assert bool((a[1][:, :-1] >= a[1][:, 1:]).all())                         # sorted by predicted IoU, descending


def test_hq_model_with_input_masks(dev, scene):
    """the dense-prompt path a user reaches: `input_masks` (the best low-resolution logits of a first call) through
    `SamHQModelHIP.forward` and through `SamSession.predict(mask_input=)`, against `SamHQModel`.  HF forms hq_features from the
    image embedding WITHOUT the dense prompt and the upscaled embedding from their sum: features taken from the wrong tensor,
    or a dense prompt that does not reach the upscaler, both show as a difference of whole logits."""
    hf, hip = _models(dev)
    s = scene['session']
    pts = torch.tensor([[[[300.0, 200.0]], [[800.0, 500.0]]]])
    first_m, first_i = _hf_call(hf, scene, pts)
    prev = first_m[0, 0, int(first_i[0, 0].argmax())]                        # [256, 256] logits
    base_m, _ = _hf_call(hf, scene, pts, True, True)
    for multi, hq_only in ((True, False), (False, False), (True, True)):
        want_m, want_i = _hf_call(hf, scene, pts, multi, hq_only, mask=prev)
        got = hip(image_embeddings=s.image_embeddings, intermediate_embeddings=s.intermediate_embeddings, input_points=pts.to(dev),
                  input_masks=prev.reshape(1, 1, 256, 256).to(dev), multimask_output=multi, hq_token_only=hq_only)
        em, ei = _err(got.pred_masks, want_m), _err(got.iou_scores, want_i)
        print(f'input_masks (multimask {multi}, hq_token_only {hq_only}): pred_masks err {em:.2e} (|logit| up to '
              f'{float(want_m.abs().max()):.1f}), iou_scores err {ei:.2e}')
        assert tuple(got.pred_masks.shape) == tuple(want_m.shape) and em < TOL and ei < TOL
    moved = _err(want_m, base_m)
    print(f'the dense prompt moves the HQ mask by up to {moved:.2f}')
    assert moved > 100 * TOL                                                 # (the case does exercise the dense prompt)
    # the session: original-pixel points, the same mask as `mask_input`
    p = np.array([[[300.0 / 8, 200.0 / 8]], [[800.0 / 8, 500.0 / 8]]])
    want_m, want_i = _hf_call(hf, scene, pts, True, False, mask=prev)
    got = s.predict(points=p, mask_input=prev.to(dev))
    el, ei = _err(got[2], want_m[0]), _err(got[1], want_i[0])
    print(f'SamSession.predict(mask_input=): low-res err {el:.2e}, iou err {ei:.2e}')
    assert el < TOL and ei < TOL


def _post(low, nhw, ohw):
    """post_process_masks' values for [k, 256, 256] logits"""
    m = F.interpolate(low[:, None], size=(1024, 1024), mode='bilinear', align_corners=False)[..., :nhw[0], :nhw[1]]
    return F.interpolate(m, size=ohw, mode='bilinear', align_corners=False)[:, 0]


def _gap_threshold(v):
    """a threshold nobody is near: the middle of the widest gap between neighbours of the sorted values' middle half"""
    sv = v.sort().values
    n = sv.shape[0]
    lo, hi = n // 4, 3 * n // 4
    i = lo + int((sv[lo + 1:hi + 1] - sv[lo:hi]).argmax())
    return float((sv[i] + sv[i + 1]) / 2)


def test_generate_masks_with_an_hq_model_against_hf_helpers(dev, scene):
    """points_per_side = 4 on the 96 x 128 image: 16 prompts, 48 candidates.  The oracle: HF's helpers (`_build_point_grid`,
    `_compute_stability_score`, `_batched_mask_to_box`, `_mask_to_rle`) over `SamHQModel`'s outputs.  Thresholds in the widest
    gap of the oracle's middle half of values (a median would sit ON a candidate); candidates whose oracle IoU is within 1e-3
    of its threshold or whose stability crosses its threshold when the logits move by 1e-3 are undecided: at most 1 %."""
    from oracle import cops
    from transformers.models.sam import image_processing_pil_sam as ip
    from rsprompter_amd.apis import SamMaskGenerator, generate_masks
    hf, hip = _models(dev)
    s = scene['session']
    nhw = s.input_size
    n, off, thr = 4, 0.25, 0.0
    grid = ip._build_point_grid(n) * np.array([[W0, H0]])
    pts = torch.from_numpy(ip._normalize_coordinates(1024, grid, (H0, W0))).float()[None, :, None, :]
    want_m, want_i = _hf_call(hf, scene, pts)
    low, iou = want_m[0].flatten(0, 1), want_i[0].flatten()
    K = low.shape[0]
    val = _post(low, nhw, (H0, W0))
    stab = ip._compute_stability_score(val, thr, off)
    stab_p, stab_m = ip._compute_stability_score(val + 1e-3, thr, off), ip._compute_stability_score(val - 1e-3, thr, off)
    boxes = ip._batched_mask_to_box(val > thr).float()
    t_iou, t_stab = _gap_threshold(iou), _gap_threshold(stab)
    keep_o = (iou > t_iou) & (stab > t_stab)
    undecided = ((iou - t_iou).abs() < 1e-3) | ((stab_p > t_stab) != (stab > t_stab)) | ((stab_m > t_stab) != (stab > t_stab))
    print(f'{K} candidates: iou threshold {t_iou:.3f}, stability threshold {t_stab:.3f}, oracle keeps {int(keep_o.sum())}, '
          f'undecided {int(undecided.sum())}')
    assert K == 48 and float(undecided.float().mean()) <= 0.01 and int(keep_o.sum()) > 0
    ko = keep_o.nonzero()[:, 0]
    _, nk = cops.nms(boxes[ko], iou[ko], 0.7)
    final_o = ko[nk].tolist()
    st = {}
    kw = dict(points_per_side=n, pred_iou_thresh=t_iou, stability_score_thresh=t_stab, stability_score_offset=off,
              mask_threshold=thr, crops_nms_thresh=0.7)
    res = generate_masks(hip, None, session=s, _stages=st, output='dense', **kw)
    e_low, e_iou = _err(st['low_res'], low), _err(st['iou'], iou)
    print(f'candidates: low-res err {e_low:.2e}, iou err {e_iou:.2e}')
    assert e_low < TOL and e_iou < TOL
    kept_d = torch.zeros(K, dtype=torch.bool)
    kept_d[st['kept'].cpu()] = True
    dec = ~undecided
    assert torch.equal(kept_d[dec], keep_o[dec])
    final_d = st['final'].cpu().tolist()
    if torch.equal(kept_d, keep_o):
        assert final_d == final_o
    assert res.bboxes.shape[0] == len(final_d) > 0
    for i, c in enumerate(final_d):
        assert res.bboxes[i].cpu().tolist() == boxes[c].tolist(), c
        assert abs(float(res.scores[i]) - float(iou[c])) < TOL
        mism = res.masks[i].cpu() != (val[c] > thr)
        assert bool((val[c][mism].abs() < 1e-3).all()), c          # (a pixel may differ only where the oracle's value is undecided)
    rle = generate_masks(hip, None, session=s, **kw)
    for i, c in enumerate(final_d):
        assert np.array_equal(ip._rle_to_mask(rle.masks[i]), res.masks[i].cpu().numpy()), c
    # the crop-layer generator with no crop layers: the same instances
    gen = SamMaskGenerator(hip, crop_n_layers=0, output='dense', **kw).generate(scene['img'].numpy())
    assert torch.equal(gen.bboxes, res.bboxes) and torch.equal(gen.scores, res.scores) and torch.equal(gen.masks, res.masks)
    # hq_token_only: one candidate per point
    st1 = {}
    generate_masks(hip, scene['img'].numpy(), hq_token_only=True, _stages=st1, **kw)
    hq_m, hq_i = _hf_call(hf, scene, pts, True, True)
    assert tuple(st1['low_res'].shape) == (16, 256, 256)
    assert _err(st1['low_res'], hq_m[0, :, 0]) < TOL and _err(st1['iou'], hq_i[0, :, 0]) < TOL
