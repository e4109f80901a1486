"""-m gpu: promptable SAM -- the prompt-encoder kernel, the full `SamModel` call, the mask-scoring kernel, `SamSession`
and `generate_masks` against the real HF `SamModel` on the CPU (oracle/samdet.py::build_sam_model) and HF's own mask-generation
helpers (transformers.models.sam.image_processing_pil_sam).  Weights: synth_state_dict(build_sam_model('base'), seed=0) on both
sides (HF's default initialisation gives logits of +-0.04 and a stability score of 0 everywhere)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _hf_helpers():
    from transformers.models.sam import image_processing_pil_sam as ip
    return ip


_PAIR = {}


def _models(dev):
    """HF SamModel('base') with the seeded weights and the HIP model holding the same tensors (HF ties the two Gaussian
    matrices, so the HIP side loads HF's state_dict AFTER HF loaded the seeded one)."""
    if 'pair' not in _PAIR:
        from oracle.samdet import build_sam_model
        from rsprompter_amd.samdet import SamModelHIP
        from rsprompter_amd.synth import synth_state_dict
        hf = build_sam_model('base')
        hf.load_state_dict(synth_state_dict(hf, seed=0))
        hip = SamModelHIP('base')
        res = hip.load_state_dict(hf.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        _PAIR['pair'] = (hf, hip.to(dev).eval())
    return _PAIR['pair']


def _smooth(g, *shape, k=5, scale=1.0):
    return F.avg_pool2d(torch.randn(*shape, generator=g), k, 1, k // 2) * scale


# ----------------------------------------------------------------------------------------------------- 1. prompt kernel
def prompt_cases(g):
    """(points [R,P,2] | None, labels | None, boxes [R,4] | None, input_shape (h, w))"""
    def pts(R, P, w=1024, h=1024):
        return torch.rand(R, P, 2, generator=g) * torch.tensor([w, h], dtype=torch.float32)

    def labs(R, P):
        return torch.tensor([1, 0, -1, -10])[torch.randint(0, 4, (R, P), generator=g)]

    def bxs(R, w=1024, h=1024):
        b = torch.rand(R, 4, generator=g) * torch.tensor([w, h, w, h], dtype=torch.float32) * 0.7
        b[:, 2:] = b[:, :2] + torch.rand(R, 2, generator=g) * 300
        return b
    return [(pts(7, 1), labs(7, 1), None, (1024, 1024)), (pts(5, 3), labs(5, 3), None, (1024, 1024)),
            (pts(9, 8), labs(9, 8), None, (1024, 1024)), (None, None, bxs(37), (1024, 1024)),
            (pts(6, 2), labs(6, 2), bxs(6), (1024, 1024)), (pts(4, 3, 1024, 768), labs(4, 3), bxs(4, 1024, 768), (768, 1024))]


def check_prompt_kernel(ops, dev):
    """shared with tests/test_sam_prompts_cpu.py (there `ops` is the emulated module and dev the CPU)"""
    from oracle import hf_sam
    from oracle.samdet import build_sam_model
    g = torch.Generator().manual_seed(11)
    enc = build_sam_model('base').prompt_encoder               # HF's initialisation: a Gaussian matrix of scale 128
    G = enc.shared_embedding.positional_embedding.detach()
    pe = [enc.point_embed[i].weight.detach() for i in range(4)]
    nap = enc.not_a_point_embed.weight.detach()
    for points, labels, boxes, shape in prompt_cases(g):
        enc.input_image_size = shape[0]
        if shape[0] != shape[1]:
            # HF's encoder holds one number for both sides: the non-square case goes through its positional embedding with
            # input_shape = (h, w) -- the very call _embed_points / _embed_boxes make -- and the type rows are added here
            want = _hf_sparse_nonsquare(enc, points, labels, boxes, shape)
        else:
            with torch.no_grad():
                want = enc(None if points is None else points[None], None if labels is None else labels[None],
                           None if boxes is None else boxes[None], None)[0][0]
        got = ops.sam_embed_prompts(None if points is None else points.to(dev), None if labels is None else labels.to(dev),
                                    None if boxes is None else boxes.to(dev), points is not None and boxes is None,
                                    G.to(dev), [p.to(dev) for p in pe], nap.to(dev), shape)
        coords = []
        if points is not None:
            coords.append((points + 0.5).reshape(-1, 2))
        if boxes is not None:
            coords.append((boxes + 0.5).reshape(-1, 2))
        c = torch.cat(coords, 0) / torch.tensor([shape[1], shape[0]], dtype=torch.float32)
        arg = float(((2 * c - 1) @ G).abs().max()) * 6.2832
        tol = 8 * 2.0 ** -24 * arg + 1e-5                      # the bound of tests/test_gpu_samdet.py:90-95
        e = _err(got, want)
        print(f'prompts P={0 if points is None else points.shape[1]} box={boxes is not None} shape={shape}: '
              f'max |argument| {arg:.0f} rad, tolerance {tol:.1e}, err {e:.1e}')
        assert got.shape == want.shape and e < tol
        if points is None:
            old = ops.sam_embed_boxes(boxes.to(dev), G.to(dev), pe[2].to(dev), pe[3].to(dev), shape)
            assert torch.equal(got, old)
    # the bare positional encoding (RSSamPositionalEmbedding.forward)
    from rsprompter_amd.sam_decoder import RSSamPositionalEmbedding
    m = RSSamPositionalEmbedding('sam_vit_base')
    m.shared_image_embedding.positional_embedding.data.copy_(G)
    m = m.to(dev)
    shared = hf_sam.build_positional_embedding('base')
    shared.positional_embedding.data.copy_(G)
    c = torch.rand(2, 3, 4, 2, generator=g)
    with torch.no_grad():
        assert _err(m(c.to(dev)), shared(c)) < 8 * 2.0 ** -24 * 6.2832 * float(((2 * c - 1) @ G).abs().max()) + 1e-5
        cp = c * 700
        arg = 6.2832 * float(((2 * cp / torch.tensor([900.0, 700.0]) - 1) @ G).abs().max())
        assert _err(m(cp.to(dev), (700, 900)), shared(cp, (700, 900))) < 8 * 2.0 ** -24 * arg + 1e-5


def _hf_sparse_nonsquare(enc, points, labels, boxes, shape):
    out = []
    with torch.no_grad():
        if points is not None:
            p, lab = points[None] + 0.5, labels[None]
            if boxes is None:
                p = torch.cat([p, torch.zeros(1, p.shape[1], 1, 2)], 2)
                lab = torch.cat([lab, -torch.ones(1, lab.shape[1], 1, dtype=lab.dtype)], 2)
            e = enc.shared_embedding(p, shape)
            e = torch.where(lab[..., None] == -1, enc.not_a_point_embed.weight, e)
            e = torch.where(lab[..., None] != -10, e, torch.zeros_like(e))
            e = torch.where((lab == 0)[..., None], e + enc.point_embed[0].weight[None, None], e)
            e = torch.where((lab == 1)[..., None], e + enc.point_embed[1].weight[None, None], e)
            out.append(e)
        if boxes is not None:
            ce = enc.shared_embedding((boxes[None] + 0.5).reshape(1, -1, 2, 2), shape)
            ce[:, :, 0, :] += enc.point_embed[2].weight
            ce[:, :, 1, :] += enc.point_embed[3].weight
            out.append(ce)
    return torch.cat(out, 2)[0]


@pytest.mark.quick
def test_prompt_kernel(dev):
    from rsprompter_amd import ops
    check_prompt_kernel(ops, dev)


# ------------------------------------------------------------------------------------------------------- 3. score kernel
def oracle_fields(low, img, crop, out, chunk=32):
    """HF post_process_masks' interpolation chain on the CPU, in chunks: yields (first index, fp32 [n, oh, ow])"""
    for i in range(0, low.shape[0], chunk):
        m = F.interpolate(low[i:i + chunk, None], size=img, mode='bilinear', align_corners=False)
        m = m[..., :crop[0], :crop[1]]
        yield i, F.interpolate(m, size=out, mode='bilinear', align_corners=False)[:, 0]


def check_score_kernel(ops, dev, cases, g, thr=0.0, off=1.0, base=256, near_cap=1e-4):
    """(a) bit level against ops.mask_post_logits, (b) against HF's helpers within the interpolation's value error.
    near_cap: the largest fraction of oracle pixels within 1e-4 of a threshold (tests/test_gpu_samdet.py:107); the emulator's
    small cases pass None -- 1e-4 of their 1.5k .. 16k pixels is less than two pixels, so only the count bound is asserted there"""
    ip = _hf_helpers()
    for (k, img, crop, out) in cases:
        low = _smooth(g, k, 1, base, base, k=9)[:, 0] * 20                     # the recipe of tests/test_gpu_samdet.py:102
        if k > 1:
            low[0] = -30.0                                                     # an empty mask ...
        if k > 2:
            low[1] = 30.0                                                      # ... and a full one
        sc = ops.mask_score_box(low.to(dev), img, crop, out, thr, off).cpu()
        assert sc.dtype == torch.int32 and tuple(sc.shape) == (k, 7)
        # (a) the counts are the population counts of the bits rsp_mask_post_logits writes at the three thresholds
        t32 = [float(torch.tensor(t, dtype=torch.float32)) for t in (thr + off, thr - off, thr)]
        for j, t in enumerate(t32):
            bits = ops.mask_post_logits(low.to(dev), img, crop, out, t).cpu()
            assert torch.equal(sc[:, j].long(), bits.flatten(1).sum(1)), (img, crop, out, j)
        assert torch.equal(sc[:, 3:].long(), ip._batched_mask_to_box(bits).long()), (img, crop, out)
        # (b) HF: F.interpolate twice + _compute_stability_score's counts + _batched_mask_to_box
        npx = out[0] * out[1]
        for i0, val in oracle_fields(low, img, crop, out):
            for r in range(val.shape[0]):
                v, s = val[r], sc[i0 + r]
                for j, t in enumerate(t32):
                    want = int((v > t).sum())
                    near = int(((v - t).abs() < 1e-4).sum())
                    assert (near_cap is None or near < near_cap * npx) and abs(int(s[j]) - want) <= near, (img, crop, out, i0 + r, j, int(s[j]), want, near)
                lo = ip._batched_mask_to_box((v > t32[2] + 1e-4)[None])[0]      # the smaller mask
                hi = ip._batched_mask_to_box((v > t32[2] - 1e-4)[None])[0]      # the larger mask
                b = s[3:].long()
                if int((v > t32[2] - 1e-4).sum()) == 0:
                    assert b.tolist() == [0, 0, 0, 0]
                elif int((v > t32[2] + 1e-4).sum()) == 0:
                    assert b.tolist() == [0, 0, 0, 0] or (bool((b[:2] >= hi[:2]).all()) and bool((b[2:] <= hi[2:]).all()))
                else:
                    assert bool((b[:2] <= lo[:2]).all()) and bool((b[:2] >= hi[:2]).all()) and \
                        bool((b[2:] >= lo[2:]).all()) and bool((b[2:] <= hi[2:]).all()), (b, lo, hi)
        print(f'score kernel {k} x {base}^2 -> {img} / {crop} / {out}: counts and boxes agree')


SCORE_CASES = ((3, (768, 1024), (768, 1024), (300, 400)), (2, (1024, 1024), (1024, 1024), (512, 512)),
               (1, (1024, 1024), (1000, 900), (333, 301)), (4, (1024, 1024), (1024, 1024), (1024, 1024)))


@pytest.mark.quick
def test_score_kernel_small_cases(dev):
    from rsprompter_amd import ops
    check_score_kernel(ops, dev, SCORE_CASES, torch.Generator().manual_seed(7))
    # localised masks (boxes away from the borders), a non-zero threshold and a small offset
    g = torch.Generator().manual_seed(8)
    ip = _hf_helpers()
    yy, xx = torch.meshgrid(torch.arange(256.0), torch.arange(256.0), indexing='ij')
    low = torch.stack([8.0 - ((xx - cx) ** 2 / sx + (yy - cy) ** 2 / sy) for cx, cy, sx, sy in
                       ((40.0, 200.0, 30.0, 90.0), (128.0, 128.0, 400.0, 50.0), (250.0, 3.0, 10.0, 10.0))])
    low = low + _smooth(g, 3, 1, 256, 256)[:, 0]
    for img, crop, out in ((1024, 1024), (1024, 683), (600, 400)), ((1024, 1024), (1024, 1024), (1024, 1024)):
        sc = ops.mask_score_box(low.to(dev), img, crop, out, 0.3, 0.25).cpu()
        for j, t in enumerate((0.55, 0.05, 0.3)):
            bits = ops.mask_post_logits(low.to(dev), img, crop, out, t).cpu()
            assert torch.equal(sc[:, j].long(), bits.flatten(1).sum(1))
        bx = ip._batched_mask_to_box(bits)
        assert torch.equal(sc[:, 3:].long(), bx.long()) and int(bx[0, 0]) > 0 and int(bx[0, 3]) < out[0] - 1


@pytest.mark.quick
def test_score_kernel_at_generation_scale_writes_no_field(dev):
    """3072 candidates (a 32 x 32 grid, three masks each) 256^2 -> 1024^2: bit level against rsp_mask_post_logits in batches;
    the HF leg on a sample of 48 of them; the scoring call's peak allocation grows by less than its own input (K h w 4 bytes, a
    sixteenth of the fp32 field it does not write)."""
    from rsprompter_amd import ops
    ip = _hf_helpers()
    g = torch.Generator().manual_seed(9)
    K = 3072
    low = (_smooth(g, K, 1, 256, 256, k=9)[:, 0] * 20 + torch.randn(K, 1, 1, generator=g) * 3).contiguous()
    low[5], low[6] = -30.0, 30.0
    lowd = low.to(dev)
    S = (1024, 1024)
    ops.mask_score_box(lowd[:4], S, S, S, 0.0, 1.0)                      # the library is loaded before the measurement
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    sc = ops.mask_score_box(lowd, S, S, S, 0.0, 1.0)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print(f'mask_score_box on {K} x 256^2 -> 1024^2: peak allocation grew by {grew} bytes (input {K * 256 * 256 * 4})')
    assert grew < K * 256 * 256 * 4
    cnt = torch.zeros((K, 3), dtype=torch.int64, device=dev)
    box = torch.zeros((K, 4), dtype=torch.int64)
    for i in range(0, K, 256):
        for j, t in enumerate((1.0, -1.0, 0.0)):
            bits = ops.mask_post_logits(lowd[i:i + 256], S, S, S, t)
            cnt[i:i + 256, j] = bits.flatten(1).sum(1)
        rows, cols = bits.any(2), bits.any(1)
        ar = torch.arange(1024, device=dev)
        big = 10 ** 6
        y0 = torch.where(rows, ar, big).amin(1); y1 = torch.where(rows, ar, -1).amax(1)
        x0 = torch.where(cols, ar, big).amin(1); x1 = torch.where(cols, ar, -1).amax(1)
        b = torch.stack([x0, y0, x1, y1], 1)
        b[~rows.any(1)] = 0
        box[i:i + 256] = b.cpu()
    assert torch.equal(sc[:, :3].long(), cnt) and torch.equal(sc[:, 3:].long().cpu(), box)
    sc = sc.cpu()
    assert sc[5].tolist() == [0] * 7 and sc[6].tolist() == [1 << 20] * 3 + [0, 0, 1023, 1023]
    sel = torch.arange(0, K, 64)
    for i0, val in oracle_fields(low[sel], S, S, S, chunk=16):
        for r in range(val.shape[0]):
            s = sc[sel[i0 + r]]
            for j, t in enumerate((1.0, -1.0, 0.0)):
                near = int(((val[r] - t).abs() < 1e-4).sum())
                assert near < 1e-4 * (1 << 20) and abs(int(s[j]) - int((val[r] > t).sum())) <= near
            st = float(ip._compute_stability_score(val[r][None], 0.0, 1.0)[0])
            if int(s[1]):
                assert abs(st - int(s[0]) / int(s[1])) < 1e-3


# ---------------------------------------------------------------------------------------------------------- 2. model call
MODEL_CASES = ('one_point', 'three_points_mixed', 'points_and_box', 'box_multimask', 'point_and_mask', 'pb64_b2', 'fourteen_points',
               'mask_only')


def _model_case(name, g):
    B, kw = 1, {}
    P = lambda *s: torch.rand(*s, 2, generator=g) * 1000              # noqa: E731
    if name == 'one_point':
        kw = dict(input_points=P(1, 1, 1), multimask_output=True)
    elif name == 'three_points_mixed':
        kw = dict(input_points=P(1, 2, 3), input_labels=torch.tensor([[[1, 0, 1], [0, 1, -1]]]), multimask_output=False)
    elif name == 'points_and_box':
        b = torch.rand(1, 3, 4, generator=g) * 500
        b[..., 2:] += 300
        kw = dict(input_points=P(1, 3, 2), input_labels=torch.tensor([[[1, 1], [1, 0], [0, 1]]]), input_boxes=b,
                  multimask_output=True)
    elif name == 'box_multimask':
        b = torch.rand(1, 5, 4, generator=g) * 500
        b[..., 2:] += 250
        kw = dict(input_boxes=b, multimask_output=True)
    elif name == 'point_and_mask':
        kw = dict(input_points=P(1, 2, 1), input_masks=_smooth(g, 1, 1, 256, 256, k=9) * 20, multimask_output=True)
    elif name == 'pb64_b2':
        B = 2
        kw = dict(input_points=P(2, 64, 1), multimask_output=True)
    elif name == 'fourteen_points':
        kw = dict(input_points=P(1, 1, 14), input_labels=torch.randint(0, 2, (1, 1, 14), generator=g), multimask_output=False)
    elif name == 'mask_only':                                           # no sparse prompt at all: the five output tokens alone
        kw = dict(input_masks=_smooth(g, 1, 1, 256, 256, k=9) * 20, multimask_output=True)
    E = _smooth(g, B, 256, 64, 64, k=5) * 2
    return E, kw


@pytest.mark.parametrize('name', MODEL_CASES)
def test_sam_model_call_against_hf(dev, name):
    """SamModelHIP.forward(image_embeddings=E, ...) against HF SamModel on the CPU with the same E; 1e-3 max-abs on the mask
    logits and IoU predictions (the project's contract for SAM mask logits, README / DESIGN §5)."""
    hf, hip = _models(dev)
    E, kw = _model_case(name, torch.Generator().manual_seed(21 + MODEL_CASES.index(name)))
    with torch.no_grad():
        want = hf(image_embeddings=E, **kw)
    got = hip(image_embeddings=E.to(dev), **{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()})
    assert tuple(got.pred_masks.shape) == tuple(want.pred_masks.shape)
    assert tuple(got.iou_scores.shape) == tuple(want.iou_scores.shape)
    em, ei = _err(got.pred_masks, want.pred_masks), _err(got.iou_scores, want.iou_scores)
    print(f'{name}: pred_masks err {em:.2e} (range {float(want.pred_masks.abs().max()):.1f}), iou_scores err {ei:.2e}')
    assert em < 1e-3 and ei < 1e-3
    if name == 'box_multimask':
        # get_prompt_embeddings (HF:1158-1188) and the decoder's HF signature with point_batch_size > 1
        sp, de = hip.get_prompt_embeddings(input_boxes=kw['input_boxes'].to(dev))
        with torch.no_grad():
            wsp, wde = hf.get_prompt_embeddings(input_boxes=kw['input_boxes'])
        assert _err(sp, wsp) < 1e-4 and _err(de, wde) == 0.0
        pe = hip.get_image_wide_positional_embeddings()
        m, i, _ = hip.mask_decoder(E.to(dev), pe, sp, de, multimask_output=True)
        assert _err(m, want.pred_masks) < 1e-3 and _err(i, want.iou_scores) < 1e-3
    if name == 'point_and_mask':
        # a per-pixel dense prompt through the decoder's HF signature
        sp, de = hip.get_prompt_embeddings(input_points=kw['input_points'].to(dev),
                                           input_labels=torch.ones(1, 2, 1, dtype=torch.int32, device=dev),
                                           input_masks=kw['input_masks'].to(dev))
        with torch.no_grad():
            wsp, wde = hf.get_prompt_embeddings(input_points=kw['input_points'], input_labels=torch.ones(1, 2, 1, dtype=torch.int32),
                                                input_masks=kw['input_masks'])
        assert _err(sp, wsp) < 1e-4 and _err(de, wde) < 1e-4
        m, i, _ = hip.mask_decoder(E.to(dev), hip.get_image_wide_positional_embeddings(), sp, de, multimask_output=True)
        assert _err(m, want.pred_masks) < 1e-3 and _err(i, want.iou_scores) < 1e-3


def test_sam_model_argument_checks_are_hfs(dev):
    hf, hip = _models(dev)
    E = torch.zeros(1, 256, 64, 64)
    bad = [dict(), dict(image_embeddings=E, pixel_values=torch.zeros(1, 3, 1024, 1024), input_points=torch.zeros(1, 1, 1, 2)),
           dict(image_embeddings=E, input_points=torch.zeros(1, 1, 2)), dict(image_embeddings=E, input_boxes=torch.zeros(1, 4)),
           dict(image_embeddings=E, input_points=torch.zeros(1, 2, 1, 2), input_boxes=torch.zeros(1, 3, 4)),
           dict(image_embeddings=E, input_points=torch.zeros(2, 1, 1, 2))]
    for kw in bad:
        with pytest.raises(ValueError) as want:
            hf(**kw)
        with pytest.raises(ValueError) as got:
            hip(**{k: v.to(dev) for k, v in kw.items()})
        assert got.value.args == want.value.args, kw.keys()
    with pytest.raises(NotImplementedError):
        hip(image_embeddings=E.to(dev), input_points=torch.zeros(1, 1, 1, 2, device=dev), attention_similarity=torch.zeros(1))


# ------------------------------------------------------------------------------------------- 4. / 5. session, generation
H0, W0 = 600, 900


@pytest.fixture(scope='module')
def scene(dev):
    """one live ViT-B encoder run on each side, shared by the session and the generation tests"""
    from rsprompter_amd.apis import SamSession
    hf, hip = _models(dev)
    g = torch.Generator().manual_seed(33)
    img = (F.interpolate(torch.rand(1, 3, 40, 60, generator=g), size=(H0, W0), mode='bicubic', align_corners=False)[0]
           .clamp(0, 1) * 255).permute(1, 2, 0).to(torch.uint8).contiguous()
    s = SamSession(hip, img.numpy())
    pv = s.pixel_values.cpu()
    with torch.no_grad():
        E = hf.get_image_embeddings(pv)
    return dict(img=img, session=s, pv=pv, E=E)


def test_session_preprocessing_geometry_and_pixel_values_call(dev, scene):
    ip = _hf_helpers()
    hf, hip = _models(dev)
    s = scene['session']
    from transformers.models.sam.image_processing_pil_sam import SamImageProcessorPil
    nh, nw = SamImageProcessorPil._get_preprocess_shape(None, (H0, W0), 1024)
    assert s.input_size == (nh, nw) == (683, 1024) and s.original_size == (H0, W0)
    pv = scene['pv']
    assert tuple(pv.shape) == (1, 3, 1024, 1024) and float(pv[:, :, nh:].abs().max()) == 0.0      # zero padding below
    # normalisation: the resized region is (x / 255 - mean) / std of a 0..255 image
    mean, std = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
    raw = pv[0, :, :nh] * std[:, None, None] + mean[:, None, None]
    assert float(raw.min()) > -1e-3 and float(raw.max()) < 1 + 1e-3
    e = _err(s.image_embeddings, scene['E'])
    print(f'ViT-B image embedding err {e:.2e} (range {float(scene["E"].abs().max()):.1f})')
    # the model call with pixel_values (live ViT on both sides)
    pts = torch.tensor([[[[300.0, 200.0]], [[800.0, 500.0]]]])
    with torch.no_grad():
        want = hf(image_embeddings=scene['E'], input_points=pts, multimask_output=True)
    got = hip(pixel_values=s.pixel_values, input_points=pts.to(dev), multimask_output=True)
    em, ei = _err(got.pred_masks, want.pred_masks), _err(got.iou_scores, want.iou_scores)
    print(f'pixel_values call: pred_masks err {em:.2e}, iou_scores err {ei:.2e}')
    assert em < 1e-3 and ei < 1e-3
    assert ip._normalize_coordinates(1024, np.array([[450.0, 300.0]]), (H0, W0)).tolist() == \
        __import__('rsprompter_amd.sam_prompts', fromlist=['x']).scale_coords([[450.0, 300.0]], (H0, W0), (nh, nw)).tolist()


def _post(low, nhw, ohw):
    """post_process_masks' values for [k, 256, 256] logits"""
    m = F.interpolate(low[:, None], size=(1024, 1024), mode='bilinear', align_corners=False)[..., :nhw[0], :nhw[1]]
    return F.interpolate(m, size=ohw, mode='bilinear', align_corners=False)[:, 0]


def test_session_predict_against_hf(dev, scene):
    ip = _hf_helpers()
    hf, hip = _models(dev)
    s = scene['session']
    nhw = s.input_size
    pts = np.array([[[450.0, 300.0], [100.0, 80.0]], [[700.0, 120.0], [30.0, 550.0]]])
    labs = np.array([[1, 0], [1, 1]])
    boxes = np.array([[200.0, 100.0, 700.0, 500.0], [10.0, 20.0, 300.0, 590.0]])

    def hf_call(points=None, labels=None, boxes=None, mask=None, multi=True):
        kw = {}
        if points is not None:
            kw['input_points'] = torch.from_numpy(ip._normalize_coordinates(1024, points, (H0, W0))).float()[None]
            kw['input_labels'] = torch.from_numpy(labels)[None]
        if boxes is not None:
            kw['input_boxes'] = torch.from_numpy(ip._normalize_coordinates(1024, boxes, (H0, W0), is_bounding_box=True)).float()[None]
        if mask is not None:
            kw['input_masks'] = mask.reshape(1, 1, 256, 256)
        with torch.no_grad():
            o = hf(image_embeddings=scene['E'], multimask_output=multi, **kw)
        return o.pred_masks[0], o.iou_scores[0]

    def compare(tag, got, want):
        masks, iou, low = got
        wl, wi = want
        el, ei = _err(low, wl), _err(iou, wi)
        val = _post(wl.flatten(0, 1), nhw, (H0, W0)).view(*wl.shape[:2], H0, W0)
        mism = masks.cpu() != (val > 0)
        frac = float(mism.float().mean())
        print(f'{tag}: low-res err {el:.2e}, iou err {ei:.2e}, mask mismatch {frac:.2e}')
        assert tuple(masks.shape) == tuple(val.shape) and masks.dtype == torch.bool
        assert el < 2e-3 and ei < 2e-3                          # two ViT-B runs apart (tests/test_gpu_samdet.py:377)
        assert frac < 1e-3 and bool((val[mism].abs() < 1e-3).all())
    got = s.predict(points=pts, labels=labs)
    compare('points', got, hf_call(pts, labs))
    compare('boxes, one mask', s.predict(boxes=boxes, multimask_output=False), hf_call(boxes=boxes, multi=False))
    compare('points + boxes', s.predict(points=pts, labels=labs, boxes=boxes), hf_call(pts, labs, boxes))
    # refine: the best mask's logits of the first prompt set back in, with one more click
    best = int(got[1][0].argmax())
    prev = got[2][0, best]
    pts2, labs2 = pts[:1], labs[:1]
    compare('points + mask_input', s.predict(points=pts2, labels=labs2, mask_input=prev),
            hf_call(pts2, labs2, mask=prev.cpu()))
    vals = s.predict(points=pts2, labels=labs2, return_logits=True)[0]
    assert vals.dtype == torch.float32 and tuple(vals.shape) == (1, 3, H0, W0)
    from rsprompter_amd.apis import inference_prompts
    one = inference_prompts(hip, scene['img'], points=pts, labels=labs)
    assert torch.equal(one[0], got[0])


def test_generate_masks_against_hf_pipeline(dev, scene):
    """16 x 16 grid, three masks each = 768 candidates on the 600 x 900 test image, thresholds at the oracle's medians and
    stability_score_offset = 0.25 (at 1.0 the synthetic weights give a median stability near 0).  Undecided candidates
    (oracle IoU prediction within 1e-3 of its threshold, or stability crossing its threshold when the logits move by
    +-1e-4): cap 3 %.  Measured with the encoder's real embedding of this image, HF model alone on the CPU: IoU predictions
    -0.55 .. 1.02 (median 0.083), stability 0.000 .. 0.786 (median 0.443), the oracle keeps 300, 1 candidate undecided
    (0.13 %); the test prints the figures of its run."""
    from oracle import cops
    from rsprompter_amd.apis import generate_masks
    from rsprompter_amd import ops
    ip = _hf_helpers()
    hf, hip = _models(dev)
    s = scene['session']
    nhw = s.input_size
    n, off, thr = 16, 0.25, 0.0
    grid = ip._build_point_grid(n) * np.array([[W0, H0]])
    pts = torch.from_numpy(ip._normalize_coordinates(1024, grid, (H0, W0))).float()[None, :, None, :]
    with torch.no_grad():
        o = hf(image_embeddings=scene['E'], input_points=pts, input_labels=torch.ones(1, n * n, 1, dtype=torch.int64),
               multimask_output=True)
    low, iou = o.pred_masks[0].flatten(0, 1), o.iou_scores[0].flatten()
    K = low.shape[0]
    stab, stab_p, stab_m, boxes, rles = [], [], [], [], [None] * K
    for i in range(0, K, 64):
        val = _post(low[i:i + 64], nhw, (H0, W0))
        stab.append(ip._compute_stability_score(val, thr, off))
        stab_p.append(ip._compute_stability_score(val + 1e-4, thr, off))
        stab_m.append(ip._compute_stability_score(val - 1e-4, thr, off))
        boxes.append(ip._batched_mask_to_box(val > thr))
        for j, r in enumerate(ip._mask_to_rle(val > thr)):
            rles[i + j] = r
    stab, stab_p, stab_m, boxes = torch.cat(stab), torch.cat(stab_p), torch.cat(stab_m), torch.cat(boxes).float()
    t_iou, t_stab = float(iou.median()), float(stab.median())
    keep_o = (iou > t_iou) & (stab > t_stab)
    undecided = ((iou - t_iou).abs() < 1e-3) | ((stab_p > t_stab) != (stab > t_stab)) | ((stab_m > t_stab) != (stab > t_stab))
    print(f'{K} candidates: iou {float(iou.min()):.2f} .. {float(iou.max()):.2f} (median {t_iou:.3f}), stability '
          f'{float(stab.min()):.3f} .. {float(stab.max()):.3f} (median {t_stab:.3f}), oracle keeps {int(keep_o.sum())}, '
          f'undecided {int(undecided.sum())} ({100.0 * float(undecided.float().mean()):.2f} %)')
    assert float(undecided.float().mean()) <= 0.03
    assert 0.1 * K < int(keep_o.sum()) < 0.6 * K
    # the oracle's NMS on the oracle's kept boxes; the device NMS must return its keep list
    ko = keep_o.nonzero()[:, 0]
    _, nk = cops.nms(boxes[ko], iou[ko], 0.7)
    dk = ops.nms_flat(boxes[ko].to(dev), iou[ko].to(dev), torch.zeros(ko.shape[0], dtype=torch.int32, device=dev), 0.7)
    assert dk.cpu().tolist() == nk.tolist()
    final_o = ko[nk].tolist()
    # the full device run
    st = {}
    res = generate_masks(hip, None, points_per_side=n, pred_iou_thresh=t_iou, stability_score_thresh=t_stab,
                         stability_score_offset=off, mask_threshold=thr, crops_nms_thresh=0.7, session=s, _stages=st)
    kept_d = torch.zeros(K, dtype=torch.bool)
    kept_d[st['kept'].cpu()] = True
    dec = ~undecided
    assert torch.equal(kept_d[dec], keep_o[dec]), (kept_d != keep_o).nonzero()[:, 0].tolist()
    e_low, e_iou = _err(st['low_res'], low), _err(st['iou'], iou)
    print(f'candidates: low-res err {e_low:.2e}, iou err {e_iou:.2e}; kept sets differ on {int((kept_d != keep_o).sum())} undecided')
    kd = st['kept'].cpu()
    final_d = kd[ops.nms_flat(st['boxes'], st['iou'][st['kept']], torch.zeros(kd.shape[0], dtype=torch.int32, device=dev),
                              0.7).cpu()].tolist()
    assert len(res.masks) == len(final_d) == res.bboxes.shape[0] == res.scores.shape[0] and len(final_d) > 0
    if torch.equal(kept_d, keep_o):
        assert final_d == final_o
    common = [c for c in final_d if c in set(final_o) and bool(dec[c])]
    assert common
    for c in common:
        i = final_d.index(c)
        assert res.bboxes[i].cpu().tolist() == boxes[c].tolist(), c
        assert abs(float(res.scores[i]) - float(iou[c])) < 1e-3
        assert res.masks[i]['size'] == [H0, W0] and sum(res.masks[i]['counts']) == H0 * W0
        a, b = ip._rle_to_mask(res.masks[i]), ip._rle_to_mask(rles[c])
        assert (a & b).sum() >= 0.999 * (a | b).sum(), c
    # dense output: the same instances as bool masks
    dense = generate_masks(hip, None, points_per_side=n, pred_iou_thresh=t_iou, stability_score_thresh=t_stab,
                           stability_score_offset=off, crops_nms_thresh=0.7, session=s, output='dense')
    assert dense.masks.dtype == torch.bool and tuple(dense.masks.shape) == (len(final_d), H0, W0)
    assert np.array_equal(dense.masks[0].cpu().numpy(), ip._rle_to_mask(res.masks[0]))
    with pytest.raises(NotImplementedError):
        generate_masks(hip, None, crop_n_layers=1, session=s)
