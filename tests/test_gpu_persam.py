"""-m gpu: PerSAM one-shot segmentation ("PerSAM") -- HF's `attention_similarity` / `target_embedding` hooks in
the decoder against HF `SamModel` on the CPU, the biased token -> image kernel against fp64 attention, the target /
similarity kernels against torch, the locate kernel against the materialised field (`mask_post_logits(want_val=True)`), and
`apis.PerSam`: its host flow around a stub of `SamModelHIP` on a constructed scene, and the live ViT-B procedure against the
composition of HF calls + torch that PerSAM's persam.py is.  The check_* functions are shared with
tests/test_persam_cpu.py, where `ops` is the emulated module and the device the CPU."""
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

from test_gpu_sam_multicrop import _ReadCounter, _post_s, _shape, _test_image  # noqa: E402
from test_gpu_sam_prompts import _err, _hf_helpers, _models, _smooth  # noqa: E402

TOL_LOGITS, TOL_IOU = 1e-3, 2e-3            # DESIGN §5 (SAM mask logits), the multi-crop test's bound on IoU predictions
E_SIM = 2 * 256 * 2.0 ** -24                # fp32 dot product of two unit vectors of 256 values + the two normalisations: 3.1e-5


# ------------------------------------------------------------------------------------------------- 1. hooks against HF
def hook_cases(g, B_N, size):
    """(name, B, kwargs for both models, max_prompt_sets): the issue's list -- shared / per-prompt-set similarity, each hook
    alone and both, Pb 1 and 3, points / points + box / points + input_masks, one and three masks, a chunked decode"""
    N, gs = B_N
    P = lambda *s: torch.rand(*s, 2, generator=g) * (size - 1)              # noqa: E731
    sim = lambda r: torch.randn(r, 1, 1, N, generator=g).sigmoid()          # noqa: E731  (PerSAM's attn_sim is a sigmoid)
    te = lambda *s: torch.randn(*s, 256, generator=g) * 0.5                 # noqa: E731
    box = lambda b, p: torch.cat([torch.rand(b, p, 2, generator=g) * size * 0.4,                           # noqa: E731
                                  size * 0.5 + torch.rand(b, p, 2, generator=g) * size * 0.4], -1)
    lab2 = lambda b, p: torch.tensor([1, 0]).expand(b, p, 2).contiguous()   # noqa: E731
    return [
        ('persam_first_pass', 1, dict(input_points=P(1, 1, 2), input_labels=lab2(1, 1), multimask_output=False,
                                      attention_similarity=sim(1), target_embedding=te(1, 1)), None),
        ('pb3_per_set_sim_both', 2, dict(input_points=P(2, 3, 1), multimask_output=True, attention_similarity=sim(6),
                                         target_embedding=te(1, 1)), None),
        ('box_target_alone_per_pb', 1, dict(input_points=P(1, 3, 2), input_labels=lab2(1, 3), input_boxes=box(1, 3),
                                            multimask_output=True, target_embedding=te(1, 3, 1)), None),
        ('mask_sim_alone_shared', 2, dict(input_points=P(2, 1, 2), input_labels=lab2(2, 1),
                                          input_masks=_smooth(g, 2, 1, 4 * gs, 4 * gs, k=5) * 20, multimask_output=True,
                                          attention_similarity=sim(1)), None),
        ('chunked_per_set_sim_per_image_target', 2, dict(input_points=P(2, 3, 2), input_labels=lab2(2, 3), multimask_output=False,
                                                         attention_similarity=sim(6), target_embedding=te(2, 1, 1)), 4),
    ]


def check_hooks(hf, hip, dev, gs, size, seed=70):
    """SamModelHIP.forward with the hooks against HF SamModel on the CPU, same image embedding; and HF with the hooks differs
    from HF without them by more than 10 x the tolerance, so that an ignored argument cannot pass.  Returns the distances."""
    g = torch.Generator().manual_seed(seed)
    N = gs * gs
    dec = hip.mask_decoder
    rows = []
    for name, B, kw, max_sets in hook_cases(g, (N, gs), size):
        E = _smooth(g, B, 256, gs, gs, k=5) * 2
        plain = {k: v for k, v in kw.items() if k not in ('attention_similarity', 'target_embedding')}
        with torch.no_grad():
            want = hf(image_embeddings=E, **kw)
            base = hf(image_embeddings=E, **plain)
        dec.max_prompt_sets = max_sets
        try:
            got = hip(image_embeddings=E.to(dev), **{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()})
        finally:
            dec.max_prompt_sets = None
        assert tuple(got.pred_masks.shape) == tuple(want.pred_masks.shape)
        em, ei = _err(got.pred_masks, want.pred_masks), _err(got.iou_scores, want.iou_scores)
        moved = _err(want.pred_masks, base.pred_masks)
        print(f'hooks {name}: pred_masks err {em:.2e} (range {float(want.pred_masks.abs().max()):.1f}), iou_scores err {ei:.2e}; '
              f'the hooks move HF\'s logits by {moved:.2f}')
        assert moved > 10 * TOL_LOGITS, name
        assert em < TOL_LOGITS and ei < TOL_IOU, name
        rows.append((name, em, ei, moved))
    return rows


def check_hooks_that_keep_raising(hip, dev, gs, size):
    N = gs * gs
    E = torch.zeros(1, 256, gs, gs, device=dev)
    p = torch.full((1, 1, 2, 2), size / 2.0, device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)                             # noqa: E731
    for bad in (dict(attention_similarity=z(N)),                          # 1-D
                dict(attention_similarity=z(1, 8, 1, N)),                 # per head
                dict(attention_similarity=z(1, 1, 8, N)),                 # per token
                dict(attention_similarity=z(3, 1, 1, N)),                 # neither 1 nor B * Pb rows
                dict(attention_similarity=z(1, 1, N)),                    # not 4-D
                dict(target_embedding=z(1, 1, 8, 256)),                   # per token
                dict(target_embedding=z(1, 1, 128)),
                dict(target_embedding=z(3, 1, 1, 256))):
        with pytest.raises(NotImplementedError, match='accepted forms'):
            hip(image_embeddings=E, input_points=p, **bad)
    # more than ops.SAM_T2I_MAX_TOKENS tokens with a similarity: 5 output tokens + 8 points > 12
    with pytest.raises(NotImplementedError, match='accepted forms'):
        hip(image_embeddings=E, input_points=torch.full((1, 1, 8, 2), 3.0, device=dev), attention_similarity=z(1, 1, 1, N))
    # ... the decoder's own HF signature refuses the same way
    sp = z(1, 1, 3, 256)
    with pytest.raises(NotImplementedError, match='accepted forms'):
        hip.mask_decoder(E, hip.get_image_wide_positional_embeddings(), sp, z(1, 256, gs, gs), attention_similarity=z(1))


# ------------------------------------------------------------------------------------------------- 2. biased kernel
def check_bias_kernel(ops, dev, T, N=None):
    """the input of test_sam_cross_attention_kernels (tests/test_gpu_kernels.py) + an N(0, 1) bias with Rb = 1 and R rows,
    against fp64 softmax attention under that test's bound; a zero bias gives rsp_sam_t2i_attention's bits"""
    g = torch.Generator().manual_seed(50 + T)
    R, Rimg = 5, 2
    N = N or (1000 if T != 10 else 4096)
    scale = 16 ** -0.5
    q = torch.randn(R, T, 128, generator=g)
    kv = torch.randn(Rimg, N, 256, generator=g)
    kv[..., :128] *= 2.0
    mp = torch.tensor([0, 1, 1, 0, 1], dtype=torch.int32)
    kk = kv[mp.long()][..., :128].view(R, N, 8, 16).permute(0, 2, 1, 3).double()
    vv = kv[mp.long()][..., 128:].view(R, N, 8, 16).permute(0, 2, 1, 3).double()
    qq = q.view(R, T, 8, 16).permute(0, 2, 1, 3).double()
    qd, kvd, mpd = q.view(R * T, 128).to(dev), kv.view(Rimg * N, 256).to(dev), mp.to(dev)
    errs = []
    for Rb in (1, R):
        bias = torch.randn(Rb, N, generator=g)
        ref = (((qq * scale) @ kk.transpose(-1, -2)) + bias.double()[:, None, None, :]).softmax(-1) @ vv
        ref = ref.permute(0, 2, 1, 3).reshape(R, T, 128)
        out = torch.empty(R * T, 128, device=dev)
        ops.sam_t2i_attention_bias(qd, kvd, bias.to(dev), out, R=R, T=T, N=N, scale=scale, kv_map=mpd)
        e = float((out.cpu().view(R, T, 128) - ref).abs().max())
        plain = ((qq * scale) @ kk.transpose(-1, -2)).softmax(-1) @ vv
        assert float((plain.permute(0, 2, 1, 3).reshape(R, T, 128) - ref).abs().max()) > 1e-2       # the bias matters
        print(f'biased token -> image kernel T={T} N={N} Rb={Rb}: err against fp64 {e:.2e}')
        assert e < 2e-6
        errs.append(e)
    a, b = torch.empty(R * T, 128, device=dev), torch.empty(R * T, 128, device=dev)
    ops.sam_t2i_attention(qd, kvd, a, R=R, T=T, N=N, scale=scale, kv_map=mpd)
    for Rb in (1, R):
        ops.sam_t2i_attention_bias(qd, kvd, torch.zeros(Rb, N, device=dev), b, R=R, T=T, N=N, scale=scale, kv_map=mpd)
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.sam_t2i_attention_bias(qd, kvd, torch.zeros(2, N, device=dev), b, R=R, T=T, N=N, scale=scale, kv_map=mpd)
    with pytest.raises(ValueError):
        ops.sam_t2i_attention_bias(qd, kvd, torch.zeros(1, N + 1, device=dev), b, R=R, T=T, N=N, scale=scale, kv_map=mpd)
    return errs


# ------------------------------------------------------------------------------------------------- 3. target, similarity
def check_target_and_similarity(ops, dev, S, gs, hw, B=3, seed=81):
    """the selected cell set == PerSAM's on the package's front end (torch.equal); target_embedding / target_feature / sim and
    its x 4 up-sampling against torch on the CPU within E_SIM"""
    from rsprompter_amd.sam_prompts import PerSam, preprocess_shape
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    mask = torch.zeros(H, W, dtype=torch.bool)
    mask[H // 4:H // 4 + H // 3, W // 3:W // 3 + W // 2] = True
    mask[H - 3:, :5] = True                                              # a second component at the image's lower edge
    cells = PerSam.cells_of(mask.to(dev), S, gs).cpu()
    nhw = preprocess_shape(hw, S)
    m3 = mask.float().unsqueeze(-1).expand(H, W, 3).contiguous()
    mS = ops.resize_pad(m3.to(dev), nhw, (S, S), (0.0, 0.0, 0.0))[0].cpu()
    want_cells = F.interpolate(mS[None, None], size=(gs, gs), mode='bilinear', align_corners=False)[0, 0] > 0
    assert torch.equal(cells, want_cells) and 0 < int(cells.sum()) < gs * gs
    emb = _smooth(g, B, 256, gs, gs, k=3) * 2 + torch.randn(1, 256, 1, 1, generator=g) * 0.3
    rows = emb.permute(0, 2, 3, 1).reshape(B * gs * gs, 256).contiguous()
    te, tf, cnt = ops.persam_target(rows[:gs * gs].to(dev), cells.reshape(-1).to(dev))
    feat = emb[0].permute(1, 2, 0)[want_cells]                          # persam.py: ref_feat[ref_mask > 0]
    want_te = feat.mean(0)
    want_tf = want_te / want_te.norm(dim=-1, keepdim=True)
    assert int(cnt.cpu()) == int(want_cells.sum())
    e_te, e_tf = _err(te, want_te), _err(tf, want_tf)
    assert e_te < E_SIM * float(want_te.abs().max() + 1) and e_tf < E_SIM
    sim, low = ops.persam_similarity(rows.to(dev), tf, B, gs, gs)
    f = emb / emb.norm(dim=1, keepdim=True)
    want_sim = (want_tf[None, None] @ f.reshape(B, 256, gs * gs))[:, 0]
    want_low = F.interpolate(want_sim.view(B, 1, gs, gs), scale_factor=4, mode='bilinear')[:, 0]
    e_s, e_l = _err(sim, want_sim), _err(low, want_low)
    print(f'PerSAM target / similarity S={S} g={gs} {hw}: {int(cnt.cpu())} cells, target_embedding err {e_te:.2e}, target_feature err '
          f'{e_tf:.2e}, sim err {e_s:.2e}, up-sampled err {e_l:.2e} (bound {E_SIM:.1e})')
    assert tuple(sim.shape) == (B, gs * gs) and tuple(low.shape) == (B, 4 * gs, 4 * gs)
    assert e_s < E_SIM and e_l < E_SIM
    # an empty selection: zeros and a zero count (PerSam refuses on it)
    te0, tf0, c0 = ops.persam_target(rows[:gs * gs].to(dev), torch.zeros(gs * gs, dtype=torch.bool).to(dev))
    assert int(c0.cpu()) == 0 and not bool(te0.cpu().any()) and not bool(tf0.cpu().any())
    with pytest.raises(ValueError):
        ops.persam_target(rows[:gs * gs].to(dev), cells.reshape(-1)[:-1].to(dev))
    return e_te, e_tf, e_s, e_l


# ------------------------------------------------------------------------------------------------- 4. locate kernel
def locate_fields(g, k, base, kind):
    """k low-resolution fields [k, base, base]"""
    low = _smooth(g, k, 1, base, base, k=5)[:, 0] * 0.3 + 0.4
    if kind == 'plateau':
        # a 2 x 2 block of equal maxima inside, and the extremes on the clamped border (equal pixels along the edge)
        for i in range(k):
            y, x = 3 + 2 * i, base // 2 + i
            low[i, y:y + 2, x:x + 2] = 2.0
            low[i, 0, base - 2:] = -1.5
    elif kind == 'constant':
        low[:] = 0.37
    return low.contiguous()


def check_locate(ops, dev, k, img, crop, out, gs, base, kind='smooth', seed=90, memory=False):
    """bit for bit: max / min == val.max() / val.min(), coordinates == argmax / argmin of the flattened field that
    mask_post_logits(want_val=True) writes; mean / std against fp64 within e_stat; attn_sim against
    sigmoid(F.interpolate((val - mean) / std)) within 0.25 (2 e_stat / std) + 1e-6; two runs equal"""
    g = torch.Generator().manual_seed(seed)
    low = locate_fields(g, k, base, kind).to(dev)
    if memory:
        ops.persam_locate(low[:1], img, crop, out, gs)                  # the library is loaded before the measurement
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
    stats, xy, attn = ops.persam_locate(low, img, crop, out, gs)
    if memory:
        torch.cuda.synchronize()
        grew = torch.cuda.max_memory_allocated() - before
        io = low.numel() * 4 + stats.numel() * 4 + xy.numel() * 4 + attn.numel() * 4
        print(f'persam_locate on {k} x {base}^2 -> {out}: peak allocation grew by {grew} bytes (input + outputs {io}, the field '
              f'{k * out[0] * out[1] * 4})')
        assert grew < io
    s2, x2, a2 = ops.persam_locate(low, img, crop, out, gs)
    assert torch.equal(stats, s2) and torch.equal(xy, x2) and torch.equal(attn, a2)
    val = ops.mask_post_logits(low, img, crop, out, 0.0, want_val=True)[1].cpu()
    stats, xy, attn = stats.cpu(), xy.cpu(), attn.cpu()
    H, W = out
    assert stats.dtype == torch.float32 and xy.dtype == torch.int32 and tuple(attn.shape) == (k, gs * gs)
    worst = [0.0, 0.0, 0.0]
    for i in range(k):
        v = val[i]
        assert float(stats[i, 0]) == float(v.max()) and float(stats[i, 1]) == float(v.min()), (i, stats[i], v.max(), v.min())
        imax, imin = int(v.flatten().argmax()), int(v.flatten().argmin())
        assert xy[i].tolist() == [imax % W, imax // W, imin % W, imin // W, H * W], (i, xy[i].tolist(), imax, imin)
        e_stat = 8 * 2.0 ** -24 * float(v.abs().max())
        mean, std = float(v.double().mean()), float(v.double().std())
        assert abs(float(stats[i, 2]) - mean) <= e_stat and abs(float(stats[i, 3]) - std) <= e_stat, (i, stats[i], mean, std)
        worst[0] = max(worst[0], abs(float(stats[i, 2]) - mean) / e_stat)
        worst[1] = max(worst[1], abs(float(stats[i, 3]) - std) / e_stat)
        if kind == 'constant':
            assert float(stats[i, 3]) == 0.0 and xy[i, :4].tolist() == [0, 0, 0, 0]
            assert bool((attn[i] == 0.5).all())
            continue
        want = F.interpolate(((v.double() - mean) / std)[None, None], size=(gs, gs), mode='bilinear', align_corners=False).sigmoid()
        tol = 0.25 * (2 * e_stat / std) + 1e-6
        e = float((attn[i].double() - want.flatten()).abs().max())
        worst[2] = max(worst[2], e / tol)
        assert e <= tol, (i, e, tol)
    assert not bool(attn.isnan().any())
    if kind == 'plateau' and tuple(crop) == tuple(out):
        # (identity crops: the x 4 up-sampling's weights are multiples of 1 / 8, so equal neighbours give exactly equal pixels;
        # with a second, arbitrary-scale resampling the blocks need not come out bit-equal, the rule is exercised all the same)
        for i in range(k):
            v = val[i]
            assert int((v == v.max()).sum()) > 1 and int((v == v.min()).sum()) > 1, 'the extremes are plateaus'
    print(f'persam_locate {kind} {k} x {base}^2 -> {img} / {crop} / {out}, g={gs}: extrema and positions bit for bit; mean, std, attn_sim '
          f'at {worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f} of their bounds')
    return worst


def check_locate_refusals(ops, dev):
    low = torch.zeros(2, 8, 8).to(dev)
    with pytest.raises(RuntimeError):
        ops.persam_locate(low, (32, 32), (40, 32), (16, 16), 2)           # crop larger than the resized image
    with pytest.raises(ValueError):
        ops.persam_locate(low[:, :, ::2], (32, 32), (32, 32), (16, 16), 2)
    s, x, a = ops.persam_locate(low[:0], (32, 32), (32, 32), (16, 16), 2)
    assert tuple(s.shape) == (0, 4) and tuple(x.shape) == (0, 5) and tuple(a.shape) == (0, 4)


# ------------------------------------------------------------------------------------------------- 5b. host flow, stub
class RectSam(torch.nn.Module):
    """A stub of `SamModelHIP` on a constructed scene: images are black with ONE white rectangle (or none).  The 'encoder'
    turns the brightness of a cell into a mix of two orthogonal unit vectors, so the similarity with a target taken from a
    white reference rectangle peaks inside the rectangle; the 'decoder' returns the up-sampled brightness map at three
    thresholds with fixed IoU predictions and checks what `PerSam` hands over in each of the three passes."""

    TH = (0.35, 0.5, 0.65)
    IOU2, IOU3 = (0.80, 0.95, 0.70), (0.96, 0.96, 0.50)                  # pass 3: a tie, the lower index wins

    def __init__(self, ops, dev, S, gs):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1, device=dev))
        self.image_size, self.dev, self.ops = S, dev, ops
        self.vision_encoder = types.SimpleNamespace(grid=gs, D=None)
        self.mask_decoder = self.prompt_encoder = self.vision_encoder
        g = torch.Generator().manual_seed(3)
        q, _ = torch.linalg.qr(torch.randn(256, 2, generator=g))
        self.u, self.w = q[:, 0].contiguous().to(dev), q[:, 1].contiguous().to(dev)
        self.batches, self.calls = [], []

    def bright(self, pv):
        from rsprompter_amd.sam_prompts import PIXEL_MEAN, PIXEL_STD
        top = (255.0 - PIXEL_MEAN[0]) / PIXEL_STD[0]
        return F.avg_pool2d(pv[:, :1].clamp(min=0) / top, self.image_size // self.vision_encoder.grid)      # [B, 1, g, g]

    def get_image_embeddings(self, pv):
        self.batches.append(int(pv.shape[0]))
        b = self.bright(pv)
        emb = b * self.u.view(1, 256, 1, 1) + (1 - b) * self.w.view(1, 256, 1, 1)
        return emb.contiguous(memory_format=torch.channels_last)

    def low_of(self, emb, multi):
        b = (emb * self.u.view(1, 256, 1, 1)).sum(1, keepdim=True)
        up = F.interpolate(b, scale_factor=4, mode='bilinear')                                               # [B, 1, 4g, 4g]
        ths = self.TH if multi else self.TH[1:2]
        return torch.cat([(up - t) * 16 for t in ths], 1).unsqueeze(1)                                       # [B, 1, C, 4g, 4g]

    def forward(self, image_embeddings=None, input_points=None, input_labels=None, input_boxes=None, input_masks=None,
                multimask_output=True, attention_similarity=None, target_embedding=None):
        B = image_embeddings.shape[0]
        gs = self.vision_encoder.grid
        assert tuple(input_points.shape) == (B, 1, 2, 2) and input_labels.tolist() == [[[1, 0]]] * B
        stage = 1 if input_masks is None else (2 if input_boxes is None else 3)
        if stage == 1:
            assert multimask_output is False and tuple(attention_similarity.shape) == (B, 1, 1, gs * gs)
            assert tuple(target_embedding.shape) == (1, 1, 256)
        else:
            assert multimask_output is True and attention_similarity is None and target_embedding is None
            assert tuple(input_masks.shape) == (B, 1, 4 * gs, 4 * gs)
        if stage == 3:
            assert tuple(input_boxes.shape) == (B, 1, 4)
        low = self.low_of(image_embeddings, multimask_output)
        iou = torch.tensor({1: (0.9,), 2: self.IOU2, 3: self.IOU3}[stage], device=self.dev).view(1, 1, -1).expand(B, 1, -1)
        self.calls.append(dict(stage=stage, B=B, points=input_points, masks=input_masks, boxes=input_boxes, low=low,
                               attn=attention_similarity))
        return types.SimpleNamespace(pred_masks=low, iou_scores=iou.contiguous())


def rect_image(hw, rect):
    img = torch.zeros(hw[0], hw[1], 3, dtype=torch.uint8)
    if rect is not None:
        x0, y0, x1, y1 = rect
        img[y0:y1, x0:x1] = 255
    return img


def check_host_flow(ops, dev, S, gs, sizes, scale):
    """grouping by size, batching, input order, coordinates in original pixels, a tight box, the empty-mask box.
    `sizes`: two image sizes (H, W); rectangles are given on a 60 x 90 / 50 x 70 drawing board and scaled by `scale`."""
    from rsprompter_amd.apis import PerSam
    from rsprompter_amd.sam_prompts import preprocess_shape
    ip = _hf_helpers()
    A, Bz = sizes
    sc = lambda r: None if r is None else [int(v * scale) for v in r]       # noqa: E731
    scene = [(A, sc([50, 10, 80, 40])), (Bz, sc([8, 20, 38, 44])), (A, sc([6, 30, 40, 56])), (A, None), (Bz, sc([30, 4, 66, 30]))]
    sam = RectSam(ops, dev, S, gs)
    ref_rect = sc([20, 15, 60, 45])
    ref = rect_image(A, ref_rect)
    ref_mask = ref[:, :, 0] > 0
    with pytest.raises(ValueError, match='no cell'):
        PerSam(sam, ref, torch.zeros(A, dtype=torch.bool))
    with pytest.raises(ValueError):
        PerSam(sam, ref, ref_mask[:, :-1])
    ps = PerSam(sam, ref, ref_mask)
    assert tuple(ps.target_feature.shape) == (256,) and tuple(ps.target_embedding.shape) == (1, 1, 256)
    assert float((ps.target_feature.cpu() @ sam.u.cpu())) > 0.9          # the target is the white direction
    sam.batches.clear()
    imgs = [rect_image(hw, r) for hw, r in scene]
    st = {}
    res = ps.segment(imgs, batch_size=2, output='rle', cascade=True, _stages=st)
    dense = ps.segment(imgs, batch_size=8, output='dense', cascade=True)
    # grouped by size in order of first appearance, batch_size at a time: A A | A | B B, then A A A | B B
    assert sam.batches == [2, 1, 2, 3, 2], sam.batches
    assert [c['stage'] for c in sam.calls[:9]] == [1, 2, 3] * 3
    order = [0, 2, 3, 1, 4]                                             # input index of the stage rows, batch by batch
    row = 0
    for bi, stg in enumerate(st['batches']):
        c1, c2, c3 = sam.calls[3 * bi:3 * bi + 3]
        assert torch.equal(c2['masks'][:, 0], c1['low'][:, 0, 0])       # pass 2 refines pass 1's logits
        assert stg['best2'].tolist() == [1] * c1['B'] and stg['best3'].tolist() == [0] * c1['B']
        assert torch.equal(c3['masks'][:, 0], c2['low'][:, 0, 1])       # pass 3 the best of pass 2 ...
        for b in range(c1['B']):
            i = order[row]
            hw, rect = scene[i]
            H, W = hw
            nhw = preprocess_shape(hw, S)
            r = res[i]
            # the oracle's field and masks from the stub's own tensors, torch on the CPU
            field = _post_s(stg['low_sim'][b:b + 1].cpu(), S, nhw, hw)[0]
            (xp, yp), (xn, yn) = r['points']
            want_box = ip._batched_mask_to_box(_post_s(c2['low'][b, 0, 1:2].cpu(), S, nhw, hw) > 0)[0]
            assert stg['box2'][b].tolist() == want_box.tolist()         # ... with its box at original resolution
            want_in = ip._normalize_coordinates(S, want_box.numpy().astype(np.float64), hw, is_bounding_box=True)
            assert c3['boxes'][b, 0].tolist() == torch.from_numpy(want_in).float().reshape(4).tolist()
            want_pts = ip._normalize_coordinates(S, np.array(r['points'], dtype=np.float64), hw)
            assert c1['points'][b, 0].tolist() == torch.from_numpy(want_pts).float().tolist()
            final = _post_s(c3['low'][b, 0, 0:1].cpu(), S, nhw, hw)[0]
            want_mask = final > 0
            got_mask = dense[i]['mask'].cpu()
            assert tuple(got_mask.shape) == (H, W) and got_mask.dtype == torch.bool
            assert bool(((got_mask != want_mask) <= (final.abs() < 1e-4)).all())
            assert r['mask']['size'] == [H, W] and r['mask'] == ip._mask_to_rle(got_mask[None])[0]
            assert r['bbox'] == ip._batched_mask_to_box(got_mask[None])[0].tolist() == dense[i]['bbox']
            assert abs(r['score'] - 0.96) < 1e-6 and r['points'] == dense[i]['points']
            assert float(field[yp, xp]) >= float(field.max()) - 2 * E_SIM and float(field[yn, xn]) <= float(field.min()) + 2 * E_SIM
            assert abs(r['point_sims'][0] - float(field.max())) < 2 * E_SIM and abs(r['point_sims'][1] - float(field.min())) < 2 * E_SIM
            if rect is None:
                # nothing white: an empty mask in pass 2, whose box is the scoring kernel's [0, 0, 0, 0], and an empty result
                assert r['bbox'] == [0, 0, 0, 0] and r['mask']['counts'] == [H * W] and stg['box2'][b].tolist() == [0, 0, 0, 0]
                assert not bool(c1['attn'][b].isnan().any())
            else:
                x0, y0, x1, y1 = rect
                assert x0 <= xp < x1 and y0 <= yp < y1 and not (x0 <= xn < x1 and y0 <= yn < y1), (i, r['points'], rect)
                truth = torch.zeros(H, W, dtype=torch.bool)
                truth[y0:y1, x0:x1] = True
                iou = float((got_mask & truth).sum()) / float((got_mask | truth).sum())
                cell = max(H, W) / gs
                assert iou > 0.5 and abs(r['bbox'][0] - x0) <= cell and abs(r['bbox'][1] - y0) <= cell and \
                    abs(r['bbox'][2] - (x1 - 1)) <= cell and abs(r['bbox'][3] - (y1 - 1)) <= cell, (i, iou, r['bbox'], rect)
            row += 1
    assert row == len(scene)
    # cascade=False stops after the first pass; one image instead of a list gives one dict
    n_calls = len(sam.calls)
    one = ps.segment(imgs[0], cascade=False)
    assert isinstance(one, dict) and len(sam.calls) == n_calls + 1 and sam.calls[-1]['stage'] == 1 and abs(one['score'] - 0.9) < 1e-6
    for bad in (dict(output='png'), dict(batch_size=0)):
        with pytest.raises(ValueError):
            ps.segment(imgs[0], **bad)
    with pytest.raises(ValueError):
        ps.segment(imgs[0][:, :, :2])
    return res


# ------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.parametrize('T', [7, 10, 12])
def test_biased_t2i_kernel(dev, T):
    from rsprompter_amd import ops
    check_bias_kernel(ops, dev, T)


def test_hooks_against_hf(dev):
    hf, hip = _models(dev)
    check_hooks(hf, hip, dev, 64, 1024)
    check_hooks_that_keep_raising(hip, dev, 64, 1024)


def test_session_predict_passes_the_hooks_through(dev):
    from rsprompter_amd.apis import SamSession
    hf, hip = _models(dev)
    s = SamSession(hip, _test_image((300, 450)))
    g = torch.Generator().manual_seed(5)
    pts = np.array([[[200.0, 100.0], [30.0, 250.0]]])
    sim, te = torch.randn(1, 1, 1, 4096, generator=g).sigmoid().to(dev), (torch.randn(1, 1, 256, generator=g) * 0.5).to(dev)
    a = s.predict(points=pts, labels=np.array([[1, 0]]), multimask_output=False, attention_similarity=sim, target_embedding=te)
    b = s.predict(points=pts, labels=np.array([[1, 0]]), multimask_output=False)
    want = hip(image_embeddings=s.image_embeddings, input_points=torch.tensor(
        _hf_helpers()._normalize_coordinates(1024, pts, (300, 450))).float().to(dev)[None],
        input_labels=torch.tensor([[[1, 0]]], dtype=torch.int32, device=dev), multimask_output=False,
        attention_similarity=sim, target_embedding=te)
    assert torch.equal(a[2], want.pred_masks[0]) and _err(a[2], b[2]) > 10 * TOL_LOGITS


def test_target_and_similarity(dev):
    from rsprompter_amd import ops
    check_target_and_similarity(ops, dev, 1024, 64, (600, 900))
    check_target_and_similarity(ops, dev, 1024, 64, (517, 803), B=5, seed=82)


LOCATE_CASES = (((1024, 1024), (1024, 1024), (1024, 1024)),             # strip form
                ((1024, 1024), (683, 1024), (600, 900)), ((1024, 1024), (659, 1024), (517, 803)),       # generic form
                ((1024, 1024), (1024, 1023), (1024, 1023)))             # identity with an odd width


@pytest.mark.parametrize('case', range(len(LOCATE_CASES)))
def test_locate_kernel_against_the_materialised_field(dev, case):
    from rsprompter_amd import ops
    img, crop, out = LOCATE_CASES[case]
    check_locate(ops, dev, 1, img, crop, out, 64, 256, seed=90 + case)
    check_locate(ops, dev, 5, img, crop, out, 64, 256, seed=95 + case, memory=True)
    check_locate(ops, dev, 3, img, crop, out, 64, 256, kind='plateau', seed=99)
    check_locate(ops, dev, 2, img, crop, out, 64, 256, kind='constant')
    if case == 0:
        check_locate_refusals(ops, dev)


def test_host_flow_around_a_stub(dev):
    from rsprompter_amd import ops
    check_host_flow(ops, dev, 1024, 64, ((600, 900), (500, 700)), 10)


# ---------------------------------------------------------------------------------- 5. the procedure, live ViT-B, against HF
REF = dict(hw=(600, 900), seed=7, rows=(200, 330), cols=(400, 560))
TARGETS = (((600, 900), 33), ((600, 900), 34), ((517, 803), 35), ((517, 803), 36))
UNDECIDED_GAP = 4e-3                                                     # twice the IoU bound


def oracle_persam(hf, S, gs, ref_pv, ref_cells, pv, hw, points):
    """PerSAM's persam.py as HF `SamModel` calls + torch on the CPU for ONE target image; `points` [[x+, y+], [x-, y-]] in
    original pixels are the DEVICE's (None: the oracle's own).  Returns a dict of every stage."""
    ip = _hf_helpers()
    nhw = _shape(hw, S)
    with torch.no_grad():
        ref_feat = hf.get_image_embeddings(ref_pv)[0].permute(1, 2, 0)
        target_feat = ref_feat[ref_cells]
        te = target_feat.mean(0).unsqueeze(0)
        tf = te / te.norm(dim=-1, keepdim=True)
        te = te.unsqueeze(0)
        E = hf.get_image_embeddings(pv)
        f = E[0]
        f = f / f.norm(dim=0, keepdim=True)
        sim = (tf @ f.reshape(256, gs * gs)).reshape(1, 1, gs, gs)
        low_sim = F.interpolate(sim, scale_factor=4, mode='bilinear')[0]
        field = _post_s(low_sim, S, nhw, hw)[0]
        W = hw[1]
        imax, imin = int(field.flatten().argmax()), int(field.flatten().argmin())
        own = [[imax % W, imax // W], [imin % W, imin // W]]
        pts = own if points is None else points
        norm = (field - field.mean()) / torch.std(field)
        attn = F.interpolate(norm[None, None], size=(gs, gs), mode='bilinear').sigmoid().reshape(1, 1, 1, gs * gs)
        p_in = torch.from_numpy(ip._normalize_coordinates(S, np.array(pts, dtype=np.float64), hw)).float()[None, None]
        lab = torch.tensor([[[1, 0]]])
        o1 = hf(image_embeddings=E, input_points=p_in, input_labels=lab, multimask_output=False, attention_similarity=attn,
                target_embedding=te)
        o1p = hf(image_embeddings=E, input_points=p_in, input_labels=lab, multimask_output=False)
        low1 = o1.pred_masks[0, 0, 0]
        o2 = hf(image_embeddings=E, input_points=p_in, input_labels=lab, input_masks=low1[None, None], multimask_output=True)
        b2 = int(o2.iou_scores[0, 0].argmax())
        low2 = o2.pred_masks[0, 0, b2]
        box = ip._batched_mask_to_box(_post_s(low2[None], S, nhw, hw) > 0)[0]
        b_in = torch.from_numpy(ip._normalize_coordinates(S, box.numpy().astype(np.float64), hw, is_bounding_box=True)).float()[None]
        o3 = hf(image_embeddings=E, input_points=p_in, input_labels=lab, input_boxes=b_in, input_masks=low2[None, None],
                multimask_output=True)
        b3 = int(o3.iou_scores[0, 0].argmax())
        low3 = o3.pred_masks[0, 0, b3]
        final = _post_s(low3[None], S, nhw, hw)[0]

    def gap(o):
        s = o.iou_scores[0, 0].sort(descending=True).values
        return float(s[0] - s[1])
    return dict(E=E, tf=tf[0], te=te, sim=sim[0, 0], low_sim=low_sim[0], field=field, own=own, attn=attn, low1=low1, iou1=o1.iou_scores[0, 0],
                moved=_err(o1.pred_masks, o1p.pred_masks), low2=o2.pred_masks[0, 0], iou2=o2.iou_scores[0, 0], best2=b2, box=box,
                low3=o3.pred_masks[0, 0], iou3=o3.iou_scores[0, 0], best3=b3, final=final, gap=min(gap(o2), gap(o3)))


def check_procedure(ps, hf, ops, dev, S, gs, ref, imgs, bound_sim, count_reads=True):
    """`ps.segment(imgs)` against oracle_persam with the DEVICE's points; see test_procedure_against_the_composition_of_hf"""
    import contextlib
    from rsprompter_amd.sam_prompts import PIXEL_MEAN, PIXEL_STD, preprocess_shape
    st, reads = {}, {}

    @contextlib.contextmanager
    def phase(name):
        if name == 'transfer':
            reads.setdefault('before_transfer', []).append(dict(rc.n))
        yield
        if name == 'transfer':
            rc.n.clear()                                   # the transfer's own reads do not count against the next batch
    ps._phase = phase
    with _ReadCounter() as rc:
        res = ps.segment(imgs, batch_size=8, output='dense', cascade=True, _stages=st)
    ps._phase = lambda name: contextlib.nullcontext()
    sizes = []
    for im in imgs:
        if tuple(im.shape[:2]) not in sizes:
            sizes.append(tuple(im.shape[:2]))
    print(f'host reads of segment() before the transfer of each batch: {reads["before_transfer"]}')
    assert len(st['batches']) == len(sizes)
    if count_reads:
        assert reads['before_transfer'] == [{}] * len(sizes)

    def pv_of(img):
        hw = tuple(img.shape[:2])
        return ops.resize_pad(img.to(dev), preprocess_shape(hw, S), (S, S), PIXEL_MEAN, normalise=(PIXEL_MEAN, PIXEL_STD, False))[None].cpu()
    ref_pv, ref_cells = pv_of(ref), ps.cell_mask.cpu()
    order = [i for hw in sizes for i, im in enumerate(imgs) if tuple(im.shape[:2]) == hw]       # stage rows -> input index
    oracles = {i: oracle_persam(hf, S, gs, ref_pv, ref_cells, pv_of(imgs[i]), tuple(imgs[i].shape[:2]), res[i]['points']) for i in order}
    undecided = sum(1 for o in oracles.values() if o['gap'] < UNDECIDED_GAP)
    print('oracle alone: smallest gap between the two best IoU predictions per image', [f"{oracles[i]['gap']:.3g}" for i in sorted(oracles)])
    assert undecided <= 1, 'the oracle alone: at most one undecided image'
    row = 0
    for stg in st['batches']:
        for b in range(stg['points'].shape[0]):
            k = order[row]
            hw = tuple(imgs[k].shape[:2])
            r, o = res[k], oracles[k]
            if row == 0:
                e_t = _err(ps.target_feature, o['tf'])
                print(f'target_feature err {e_t:.2e}, target_embedding err {_err(ps.target_embedding, o["te"]):.2e}')
                assert e_t < bound_sim
            e_sim, e_low = _err(stg['sim'][b].view(gs, gs), o['sim']), _err(stg['low_sim'][b], o['low_sim'])
            (xp, yp), (xn, yn) = r['points']
            f = o['field']
            d_peak, d_trough = float(f.max() - f[yp, xp]), float(f[yn, xn] - f.min())
            e_attn = _err(stg['attn_sim'][b], o['attn'].flatten())
            print(f'image {k} {hw}: sim err {e_sim:.2e} / up-sampled {e_low:.2e} (bound {bound_sim:.1e}); field std {float(f.std()):.3f}; '
                  f'device peak {r["points"][0]} is {d_peak:.1e} below the oracle\'s maximum at {o["own"][0]}, trough {r["points"][1]} '
                  f'{d_trough:.1e} above its minimum at {o["own"][1]}; attn_sim err {e_attn:.2e}; hooks move the first pass by {o["moved"]:.2f}')
            assert e_sim < bound_sim and e_low < bound_sim
            assert d_peak <= 2 * E_SIM and d_trough <= 2 * E_SIM
            e1, i1 = _err(stg['low1'][b], o['low1']), _err(stg['iou1'][b], o['iou1'])
            e2, i2 = _err(stg['low2'][b], o['low2']), _err(stg['iou2'][b], o['iou2'])
            dec = o['gap'] >= UNDECIDED_GAP
            print(f'   pass 1 err {e1:.2e} / iou {i1:.2e}; pass 2 err {e2:.2e} / iou {i2:.2e}; smallest gap between the two best IoU '
                  f'predictions {o["gap"]:.3g} ({"decided" if dec else "UNDECIDED"})')
            assert o['moved'] > 10 * TOL_LOGITS
            assert e1 < TOL_LOGITS and i1 < TOL_IOU and e2 < TOL_LOGITS and i2 < TOL_IOU
            if dec:
                assert int(stg['best2'][b]) == o['best2'] and stg['box2'][b].tolist() == o['box'].tolist()
                e3, i3 = _err(stg['low3'][b], o['low3']), _err(stg['iou3'][b], o['iou3'])
                print(f'   pass 3 err {e3:.2e} / iou {i3:.2e}; best-of-three {o["best2"]}, {o["best3"]}; box {o["box"].tolist()}')
                assert e3 < TOL_LOGITS and i3 < TOL_IOU and int(stg['best3'][b]) == o['best3']
                want = o['final'] > 0
                got = r['mask'].cpu()
                iou = float((got & want).sum()) / max(float((got | want).sum()), 1.0)
                assert iou >= 0.999, (k, iou)
                assert abs(r['score'] - float(o['iou3'][o['best3']])) < TOL_IOU
            row += 1
    assert row == len(imgs)
    return res, st


def test_procedure_against_the_composition_of_hf(dev):
    """Live ViT-B, seeded weights, one reference, four targets of two sizes.  The similarity field within E_SIM + 1.22e-5 (the
    embedding distance profiles/sam_prompts/test_gpu_sam_prompts.log records for two ViT-B runs) = 4.3e-5; the device's peak /
    trough within 2 E_SIM of the oracle's extrema on the oracle's field (not the same pixel: neighbouring pixels differ by less
    than that, the trough is a plateau -- the pixel rule is pinned bit for bit by the locate test); everything downstream with
    the DEVICE's points fed to the oracle: the three passes within 1e-3 / 2e-3, and on every decided image (the oracle's two
    best IoU predictions of both refinement passes at least 4e-3 apart; at most one image may be undecided, asserted on the
    oracle alone first) equal best-of-three indices and box, final mask at IoU >= 0.999.  No host read in segment() before the
    transfer of a batch's results.  (Not yet run on a GPU when this was written: DESIGN §15, "PerSAM".)"""
    from rsprompter_amd import ops
    from rsprompter_amd.apis import PerSam
    hf, hip = _models(dev)
    ref = _test_image(REF['hw'], seed=REF['seed'])
    ref_mask = torch.zeros(REF['hw'], dtype=torch.bool)
    ref_mask[REF['rows'][0]:REF['rows'][1], REF['cols'][0]:REF['cols'][1]] = True
    ps = PerSam(hip, ref, ref_mask)
    print(f'reference: {ps.cells} cells selected')
    imgs = [_test_image(hw, seed=s) for hw, s in TARGETS]
    check_procedure(ps, hf, ops, dev, 1024, 64, ref, imgs, E_SIM + 1.22e-5)
