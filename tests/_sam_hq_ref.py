"""Shared by tests/test_sam_hq_cpu.py (lane emulator) and tests/test_gpu_sam_hq.py (MI355X): inputs and references of the
SAM-HQ mask branch (rsp_sam_hq_mask, csrc/sam_hq.hip) and of the HQ decoder / model against transformers' `SamHQModel`."""
import functools

import torch
import torch.nn.functional as F

TOL = 1e-3        # the project's contract: mask logits and predicted IoU within 1e-3 absolute of the fp32 reference


# ------------------------------------------------------------------------------------------------ the kernel alone
def kernel_case(R, n_img, g, seed=0):
    """CPU fp32 tensors of one rsp_sam_hq_mask call: `up` [R, 2g, 2g, 64] (the upscaler after LayerNorm + GELU: GELU of a
    standard normal), the weights in torch's layouts at the scale of a default-initialised layer, hyper [R, 32], feat
    [n_img, 4g, 4g, 32] and the row map (sorted, every image used when R >= n_img)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=gen) * scale
    c = dict(R=R, g=g)
    c['up'] = F.gelu(rn(R, 2 * g, 2 * g, 64))
    c['ct_w'], c['ct_b'] = rn(64, 32, 2, 2, scale=64 ** -0.5), rn(32, scale=0.1)             # upscale_conv2
    c['c1_w'], c['c1_b'] = rn(64, 32, 3, 3, scale=288 ** -0.5), rn(64, scale=0.1)            # mask_conv1
    c['ln_w'], c['ln_b'] = 1.0 + rn(64, scale=0.1), rn(64, scale=0.1)                        # mask_norm
    c['c2_w'], c['c2_b'] = rn(32, 64, 3, 3, scale=576 ** -0.5), rn(32, scale=0.1)            # mask_conv2
    c['hyper'] = rn(R, 32)
    c['feat'] = rn(n_img, 4 * g, 4 * g, 32)
    c['map'] = ((torch.arange(R) * n_img) // R).to(torch.int32)
    return c


def kernel_ref_fp64(c):
    """ConvT -> GELU -> conv3x3 -> LN -> GELU -> conv3x3 -> + feat -> dot with hyper, in fp64: [R, 4g, 4g]"""
    d = lambda t: t.double()
    u = F.gelu(F.conv_transpose2d(d(c['up']).permute(0, 3, 1, 2), d(c['ct_w']), d(c['ct_b']), stride=2))
    v = F.conv2d(u, d(c['c1_w']), d(c['c1_b']), padding=1)
    v = F.layer_norm(v.permute(0, 2, 3, 1), (64,), d(c['ln_w']), d(c['ln_b']), 1e-6).permute(0, 3, 1, 2)
    v = F.conv2d(F.gelu(v), d(c['c2_w']), d(c['c2_b']), padding=1)
    v = v + d(c['feat'])[c['map'].long()].permute(0, 3, 1, 2)
    return torch.einsum('rc,rchw->rhw', d(c['hyper']), v)


def kernel_run(ops, c, dev):
    """the case through ops.sam_hq_mask on `dev` -> fp32 [R, 4g, 4g]"""
    from rsprompter_amd.necks import convt_weights4
    from rsprompter_amd.sam_decoder import hq_conv_weights
    t = lambda k: c[k].to(dev).contiguous()
    w2, b2 = convt_weights4(t('ct_w'), t('ct_b'))
    w1, wf = hq_conv_weights(t('c1_w'), t('c2_w'))
    up = ops.to_planes(t('up'))
    return ops.sam_hq_mask(up, w2, b2, w1, t('c1_b'), t('ln_w'), t('ln_b'), 1e-6, wf, t('c2_b'), t('hyper'), t('feat'), t('map'))


def composed_weights(ops, c, dev):
    """the packed weights of kernel_composed: (upscale_conv2 as one ConvTranspose GEMM weight + bias x4, mask_conv1, mask_conv2)"""
    from rsprompter_amd.necks import convt_weights4
    t = lambda k: c[k].to(dev).contiguous()
    pw = lambda w, b: ops.PackedWeight(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), b)
    return convt_weights4(t('ct_w'), t('ct_b')), pw(t('c1_w'), t('c1_b')), pw(t('c2_w'), t('c2_b'))


def kernel_composed(ops, c, dev):
    """the same function composed from the kernels the package already had (the issue's "second formulation"):
    conv_transpose2x2 -> gemm(conv=(3, 1, 1)) -> layernorm -> gemm(conv=(3, 1, 1)) -> + feat -> dot.  Materialises
    [R, 4g, 4g, 32 | 64] tensors, which is what the fused kernel exists to avoid."""
    t = lambda k: c[k].to(dev).contiguous()
    R, g = c['R'], c['g']
    G = 4 * g
    (w2, b2), pw1, pw2 = c.get('packed') or composed_weights(ops, c, dev)
    up = c['up_planes'] if 'up_planes' in c else ops.to_planes(t('up'))           # (a bench hands both over ready-made)
    u = ops.conv_transpose2x2(up, w2, b2, act=ops.ACT_GELU)                                           # [R, G, G, 32]
    v = ops.gemm(u, pw1, conv=(3, 1, 1))                                                              # [R * G * G, 64]
    v = ops.layernorm(v.view(-1, 64), t('ln_w'), t('ln_b'), 1e-6, act=ops.ACT_GELU)
    v = ops.gemm(v.view(R, G, G, 64), pw2, conv=(3, 1, 1)).view(R, G, G, 32)
    v = v + t('feat')[t('map').long()]
    return (v * t('hyper').view(R, 1, 1, 32)).sum(-1)


# ------------------------------------------------------------------------------------------------ decoder / model
def hf_config(arch='base'):
    from transformers import SamHQConfig
    from rsprompter_amd.nnutil import SAM_ARCH
    a = SAM_ARCH[arch]
    cfg = SamHQConfig(vision_config=dict(hidden_size=a['hidden'], num_hidden_layers=a['depth'], num_attention_heads=a['heads'],
                                         global_attn_indexes=list(a['global_idx']), mlp_dim=a['mlp']),
                      mask_decoder_config=dict(vit_dim=a['hidden']))
    for c in (cfg, cfg.vision_config, cfg.prompt_encoder_config, cfg.mask_decoder_config):
        c._attn_implementation = 'eager'
    return cfg


@functools.lru_cache(maxsize=None)
def hf_decoder(seed=0):
    """(`SamHQMaskDecoder` in fp32 on the CPU with synthetic weights, its state dict)"""
    from transformers.models.sam_hq.modeling_sam_hq import SamHQMaskDecoder
    from rsprompter_amd.synth import synth_state_dict
    dec = SamHQMaskDecoder(hf_config().mask_decoder_config).eval()
    sd = synth_state_dict(dec, seed=seed)
    dec.load_state_dict(sd, strict=True)
    return dec, sd


@functools.lru_cache(maxsize=None)
def hf_model(seed=0):
    """(`SamHQModel('base')` in fp32 on the CPU with synthetic weights, its state dict)"""
    from transformers import SamHQModel
    from rsprompter_amd.synth import synth_state_dict
    m = SamHQModel(hf_config()).eval()
    sd = synth_state_dict(m, seed=seed)
    m.load_state_dict(sd, strict=True)
    return m, sd


def decoder_case(B, Pb, n, g, seed, vit_dim=768):
    """CPU fp32 inputs of a decoder call: image embeddings [B, 256, g, g], one positional table, sparse prompts
    [B, Pb, n, 256], a constant dense prompt, an intermediate ViT feature [B, g, g, vit_dim]"""
    gen = torch.Generator().manual_seed(270 + seed)     # (inputs for which HF's sorted IoUs are MIN_GAP apart in every prompt set)
    rn = lambda *s: torch.randn(*s, generator=gen)
    emb = rn(B, 256, g, g)
    pe = rn(1, 256, g, g).expand(B, -1, -1, -1).contiguous()
    sparse = rn(B, Pb, n, 256)
    dense = rn(1, 256, 1, 1).expand(B, -1, g, g).contiguous()
    inter = rn(B, g, g, vit_dim)
    return emb, pe, sparse, dense, inter


def hf_decode(dec, emb, pe, sparse, dense, inter, multimask_output, hq_token_only):
    with torch.no_grad():
        m, i = dec(image_embeddings=emb, image_positional_embeddings=pe, sparse_prompt_embeddings=sparse,
                   dense_prompt_embeddings=dense, multimask_output=multimask_output, hq_token_only=hq_token_only,
                   intermediate_embeddings=None if inter is None else [inter])[:2]
    return m, i


MIN_GAP = 10 * TOL   # what the reference's sorted IoUs of a prompt set must be apart for its ORDER to be a fair check: any
#                      result within the tolerance keeps the order, with a margin of ten


def min_sorted_gap(iou):
    """smallest distance between neighbours of the (already sorted) IoU triples"""
    return float((iou[..., :-1] - iou[..., 1:]).abs().min()) if iou.shape[-1] > 1 else float('inf')
