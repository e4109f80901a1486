"""Bodies of the kernel property tests, shared by both kernel tiers.

One `check_<name>(ops, dev, **params)` checks one drawn example: inputs go to `dev`, outputs come back with `.cpu()`.
tests/test_wave_emu_cpu.py draws the parameters with hypothesis and calls these with the emulated `ops` on CPU tensors;
tests/test_gpu_kernel_props.py draws them from a seeded torch.Generator, at production sizes, on cuda:0.  Matmul references
run in float64 on `dev`; the other references (torch_ops_mock, oracle) stay on the CPU.

The fp64 restatements of the SAM decoder's tail (upscaler, folded token -> image attention) and the comparison helpers of
the decoder-scale tests live here too, so that tests/test_kernel_props_selfcheck_cpu.py can show that they reject known
failure signatures.  This module imports no hypothesis."""
import numpy as np
import torch
import torch.nn.functional as F

UPSCALE_TOL = 2e-5          # relative to max(1, max |ref|): the fused upscaler / the two-kernel chain (the emulator's bound)
FOLD_TOL = 2e-5             # absolute: the folded token -> image attention (test_sam_t2i_fold_matches_fp64_attention)
I2T_TOL = 2e-5              # absolute: the image -> token block (test_sam_i2t_fused_matches_composition)
FOLD_KEY_TILE = 32          # keys per tile of sam_t2i_fold_kernel (FKT, csrc/t2i_fold.hip)


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


# ---------------------------------------------------------------------------------------------------------------- comparisons
def upscale_error(got, ref):
    """max |got - ref| / max(1, max |ref|) in fp64"""
    ref = ref.to(got.device).double()
    return float((got.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def assert_upscale_close(got, ref, what=''):
    e = upscale_error(got, ref)
    assert e < UPSCALE_TOL, (what, e, UPSCALE_TOL)
    return e


def abs_error(got, ref):
    return float((got.double() - ref.to(got.device).double()).abs().max())


def assert_fold_close(got, ref, what=''):
    e = abs_error(got, ref)
    assert e < FOLD_TOL, (what, e, FOLD_TOL)
    return e


def assert_i2t_close(got, ref, what=''):
    e = abs_error(got, ref)
    assert e < I2T_TOL, (what, e, I2T_TOL)
    return e


def planes_to_f64(p, r0=0, r1=None):
    """rows r0:r1 of KB32 planes [K/32][rows][32] as fp64 [r1 - r0, K] on the planes' device"""
    r1 = p.rows if r1 is None else r1
    v = (p.hi[:, r0:r1].double() + p.lo[:, r0:r1].double()) * 2.0 ** -p.scale_log2
    return v.permute(1, 0, 2).reshape(r1 - r0, v.shape[0] * 32)


# ------------------------------------------------------------------------------------------------------- fp64 restatements
def convt2x2_f64(x, w, b):
    """ConvTranspose2d(k=2, s=2) on NHWC x [G, h, w, Cin], w [Cin, Cout, 2, 2], as the per-pixel matmul it is"""
    G, h, wd, cin = x.shape
    cout = w.shape[1]
    y = x.reshape(-1, cin) @ w.reshape(cin, cout * 4)                    # columns (co, dy, dx)
    y = y.view(G, h, wd, cout, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(G, 2 * h, 2 * wd, cout)
    return y + b


def upscale_pre_dot_f64(x, w1, b1, gamma, beta, eps, w2, b2):
    """HF:513-529 on NHWC x [G, h, w, 256]: GELU(ConvT2(GELU(LayerNorm2d(ConvT1(x))))) -> [G, 4h, 4w, 32]"""
    y = convt2x2_f64(x, w1, b1)
    y = F.gelu(F.layer_norm(y, (y.shape[-1],), gamma, beta, eps))
    return F.gelu(convt2x2_f64(y, w2, b2))


def decoder_upscale_weights(dec, dev):
    """the upscaler's fp32 parameters of a SamMaskDecoderHIP as fp64 on `dev`"""
    d = lambda t: t.detach().to(dev).double()
    return (d(dec.upscale_conv1.weight), d(dec.upscale_conv1.bias), d(dec.upscale_layer_norm.weight),
            d(dec.upscale_layer_norm.bias), 1e-6, d(dec.upscale_conv2.weight), d(dec.upscale_conv2.bias))


def upscale_ref_f64(x, wts, hyper, h, w, group=None):
    """masks [R, 4h, 4w] in fp64 of the upscaler + hyper-network product (HF:513-531).  x: [R*h*w, 256] rows or Planes
    (decoded group by group); hyper [R, 32].  Computed on hyper's device in groups of RoIs (~6 KB per input pixel)."""
    R = hyper.shape[0]
    group = group or max(1, (1 << 17) // (h * w))
    out = torch.empty((R, 4 * h, 4 * w), dtype=torch.float64, device=hyper.device)
    for r0 in range(0, R, group):
        r1 = min(R, r0 + group)
        if isinstance(x, torch.Tensor):
            xs = x[r0 * h * w:r1 * h * w].to(hyper.device).double()
        else:
            xs = planes_to_f64(x, r0 * h * w, r1 * h * w)
        u = upscale_pre_dot_f64(xs.view(r1 - r0, h, w, -1), *wts)
        out[r0:r1] = torch.einsum('ryxc,rc->ryx', u, hyper[r0:r1].double())
        del u, xs
    return out


def fold_weights(dec, pre, dev):
    """(Wk, bk, Wv, bv) of a token -> image attention of a SamMaskDecoderHIP as fp64 on `dev` (pre: 'final' or 0 / 1)"""
    at = dec.transformer.final_attn_token_to_image if pre == 'final' else dec.transformer.layers[pre].cross_attn_token_to_image
    return tuple(t.detach().to(dev).double() for t in (at.k_proj.weight, at.k_proj.bias, at.v_proj.weight, at.v_proj.bias))


def t2i_ref_f64(tq, keys, pe, wts, R, T, N, group=None, key_bias=None):
    """HF:326-331 in fp64 (k = k_proj(keys + pe), v = v_proj(keys), 8 heads x 16, scale 16^-0.5) -> [R*T, 128].  keys: [R*N, 256]
    rows or Planes; computed on tq's device in groups of RoIs.  key_bias [N]: added to every score of that key (-inf takes
    the key out of the softmax; the self-check's skipped key tile)."""
    Wk, bk, Wv, bv = wts
    dev = tq.device
    group = group or max(1, (1 << 19) // N)
    out = torch.empty((R * T, 128), dtype=torch.float64, device=dev)
    ped = pe.to(dev).double()
    for r0 in range(0, R, group):
        r1 = min(R, r0 + group)
        g = r1 - r0
        if isinstance(keys, torch.Tensor):
            ks = keys[r0 * N:r1 * N].to(dev).double()
        else:
            ks = planes_to_f64(keys, r0 * N, r1 * N)
        ks = ks.view(g, N, 256)
        K = ((ks + ped[None]) @ Wk.t() + bk).view(g, N, 8, 16).permute(0, 2, 1, 3)
        V = (ks @ Wv.t() + bv).view(g, N, 8, 16).permute(0, 2, 1, 3)
        del ks
        Q = tq[r0 * T:r1 * T].double().view(g, T, 8, 16).permute(0, 2, 1, 3)
        s = (Q * 0.25) @ K.transpose(-1, -2)
        if key_bias is not None:
            s = s + key_bias.to(dev).double()
        out[r0 * T:r1 * T] = (s.softmax(-1) @ V).permute(0, 2, 1, 3).reshape(g * T, 128)
        del K, V, s
    return out


# ---------------------------------------------------------------------------------------------------------------- properties
def check_rle_round_trip(ops, dev, k, h, w, kind, seed):
    """encode -> decode round trip of the device RLE codec (mask_rle4_kernel for W % 4 == 0, the byte-wise kernel otherwise)
    with a capacity that has to grow, against the oracle's restatement of cocoapi (rleFrString / rleDecode; the string
    pycocotools writes)"""
    from oracle import rle as orle
    from rsprompter_amd import rle as prle
    g = np.random.default_rng(seed)
    if kind == 0:
        m = g.random((k, h, w)) < 0.5                                   # noise: many runs
    elif kind == 1:
        m = np.zeros((k, h, w), bool)
    elif kind == 2:
        m = np.ones((k, h, w), bool)
    elif kind == 3:
        m = np.zeros((k, h, w), bool); m[:, :, ::2] = True               # column stripes (column-major runs of h)
    elif kind == 4:
        m = np.zeros((k, h, w), bool); m[:, ::2, :] = True               # row stripes: runs of 1
    else:
        m = np.zeros((k, h, w), bool)
        y0, x0 = int(g.integers(0, h)), int(g.integers(0, w))
        m[:, y0:y0 + int(g.integers(1, h + 1)), x0:x0 + int(g.integers(1, w + 1))] = True   # a box
    flat, offs = prle.encode_rle_strings(torch.from_numpy(m).to(dev), cap=8)     # tiny capacity: the grow-and-retry path
    buf, o = flat.cpu().numpy().tobytes(), offs.tolist()
    for i in range(k):
        s_ = buf[o[i]:o[i + 1]]
        assert s_ == orle.encode(m[i])['counts'], (k, h, w, kind, i)
        assert np.array_equal(orle.rle_decode(orle.rle_from_string(s_), h, w), m[i]), (k, h, w, kind, i)


def check_gemm_ragged(ops, dev, M, N, K, path, with_bias, with_res, act, seed):
    """C = act(A W^T + b) + res through the kernel the dispatcher picks for `path` (f32: the register-staged kernel; planes:
    gemm_f16x3_dma_kernel; s2: the persistent kernel, hint 40) against the fp64 product on `dev`"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if with_bias else None
    res = torch.randn(M, N, generator=g) if with_res else None
    a, w, b, res = _to(dev, a, w, b, res)
    ref = a.double() @ w.double().t()
    if b is not None:
        ref = ref + b.double()
    kw = {}
    if act == 1 and not with_res:
        ref, kw['act'] = F.gelu(ref), ops.ACT_GELU
    elif act == 2:
        ref, kw['act'] = F.relu(ref), ops.ACT_RELU
    if res is not None:
        ref = ref + res.double()
    pw = ops.PackedWeight(w, b, device=dev)
    if path == 'f32':
        got = ops.gemm(a, pw, res=res, dma=False, **kw)
    else:
        got = ops.gemm(ops.to_planes(a), pw, res=res, tile_hint=40 if path == 's2' else 0, **kw)
    err = float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-30))
    assert err < 3e-6, (M, N, K, path, with_bias, with_res, act, err)


def check_batched_nms(ops, dev, n, nid, thr, max_out, levels, seed):
    """greedy NMS (coordinate-offset trick) on a candidate set with duplicates and exact score ties, counts below the
    capacity, empty sets, against the oracle's restatement of mmcv batched_nms: kept indices in the same order"""
    from oracle import glue
    g = torch.Generator().manual_seed(seed)
    cap = max(n + int(torch.randint(0, 50, (1,), generator=g)), 1)
    xy = (torch.rand(cap, 2, generator=g) * 8).floor() * 16              # a coarse grid: many identical boxes
    wh = (torch.rand(cap, 2, generator=g) * 4).floor() * 16 + 16
    boxes = torch.cat([xy, xy + wh], 1)[None].contiguous()
    scores = ((torch.rand(cap, generator=g) * levels).round() / levels)[None].contiguous()     # few score levels: ties
    ids = torch.randint(0, nid, (cap,), generator=g, dtype=torch.int32)[None].contiguous()
    cand = (boxes, scores, ids, torch.arange(cap, dtype=torch.int32)[None].contiguous(), torch.tensor([n], dtype=torch.int32))
    out = ops.batched_nms(tuple(t.to(dev) for t in cand), 1, cap, thr, max_out)
    if n:
        _, keep = glue.batched_nms(boxes[0, :n], scores[0, :n], ids[0, :n].long(), thr)
        keep = keep[:max_out]
    else:
        keep = torch.zeros(0, dtype=torch.long)
    k = int(out['count'][0])
    assert k == keep.numel() and torch.equal(out['keep'][0, :k].cpu().long(), keep), (n, nid, thr, max_out)


def check_window_attention_grid(ops, dev, nw, real, nh, dh, variant):
    """rsp_vit_window_attention over a window grid: nw windows per side, `real` rows / columns in the last window of a row /
    column (the padded queries are skipped, the padded keys masked), nh heads of dh, both block counts"""
    import test_gpu_kernels as tk
    if (nh * dh) % 32:
        nh += 1                                          # the K | V planes need nh * dh % 32 == 0 (else EINVAL)
    tk.test_vit_window_attention_fused_relpos(dev, nw, real, nh, dh, 1, variant)


def check_layernorm(ops, dev, rows, C, planes, seed):
    """LayerNorm (the four-rows-per-wave kernel for C % 64 == 0 in [256, 1280] with plane outputs, the wave-per-row kernel
    otherwise), fp32 and plane outputs against fp64"""
    import test_gpu_kernels as tk
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 3 + 1
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-6)
    got = ops.layernorm(*_to(dev, x, w, b), 1e-6, planes=planes)
    if planes:
        y, pl = got if isinstance(got, tuple) else (None, got)
        assert float((tk._planes_to_f32(pl) - ref).abs().max()) < 2e-5, (rows, C)
        got = y
    if got is not None:
        assert float((got.cpu().double() - ref).abs().max()) < 2e-5, (rows, C)


def check_generic_attention(ops, dev, dh, Tq, Tk, nh):
    """rsp_attention with kv / q batch maps against fp64: ragged last tiles, one key"""
    import test_gpu_kernels as tk
    tk.test_generic_attention_with_batch_maps(dev, dh, Tq, Tk, nh)


def check_i2t_fused(ops, dev, T, N, planes_res, form):
    """rsp_sam_i2t_fused (VALU or matrix-core form) against the fp64 composition of the plain pieces"""
    import test_gpu_kernels as tk
    tk.test_sam_i2t_fused_matches_composition(dev, T, N, planes_res, form)


def check_rpn_selection(ops, dev, B, h0, w0, nms_pre, max_per_img, min_size, levels_q, seed):
    """rpn_topk -> rpn_decode -> batched NMS against the restatement of RPNHead._predict_by_feat_single on a random pyramid
    with tied (quantised) logits: identical (level, anchor) indices"""
    import torch_ops_mock as mock
    from rsprompter_amd.anchor_heads import AnchorGenerator, DeltaXYWHBBoxCoder
    g = torch.Generator().manual_seed(seed)
    strides = [4, 8, 16]
    gen = AnchorGenerator(strides=strides, ratios=[0.5, 1.0, 2.0], scales=[8])
    base = torch.stack(gen.base_anchors, 0)
    A, LD = 3, 32
    sizes = [(h0 * 4, w0 * 4), (h0 * 2, w0 * 2), (h0, w0)]
    heads = []
    for (H, W) in sizes:
        hd = torch.zeros(B * H * W, LD)
        hd[:, :A] = (torch.randn(B * H * W, A, generator=g) * 2 * levels_q).round() / levels_q      # ties
        hd[:, A:5 * A] = torch.randn(B * H * W, 4 * A, generator=g) * 0.4
        heads.append(hd.contiguous())
    img_hw = torch.tensor([[float(16 * h0), float(16 * w0)]] * B)
    coder = DeltaXYWHBBoxCoder()
    sel = ops.RpnSelector(base, strides, nms_pre, max_per_img, 0.7, min_size, coder, dev)
    got = sel([hd.to(dev) for hd in heads], sizes, LD, img_hw.to(dev))
    ref = mock.RpnSelector(base, strides, nms_pre, max_per_img, 0.7, min_size, coder, torch.device('cpu'))(heads, sizes, LD, img_hw)
    got = {key: v.cpu() for key, v in got.items()}
    for b in range(B):
        k = int(ref['count'][b])
        assert int(got['count'][b]) == k, (b, k)
        assert torch.equal(got['ids'][b, :k], ref['ids'][b, :k]) and torch.equal(got['src'][b, :k], ref['src'][b, :k]), b
        assert float((got['boxes'][b, :k] - ref['boxes'][b, :k]).abs().max() if k else 0.0) < 1e-3


def check_bbox_post(ops, dev, n, nc, thr, max_out, seed):
    """softmax + per-class decode + score threshold + multiclass NMS (rsp_bbox_post) with duplicated RoIs against the
    restatement of BBoxHead._predict_by_feat_single: the same detections (tie-aware matching, tests/_match.py)"""
    import torch_ops_mock as mock
    from _match import match_detections
    from rsprompter_amd.anchor_heads import DeltaXYWHBBoxCoder
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, 2, generator=g) * 300
    roi = torch.cat([torch.zeros(n, 1), xy, xy + torch.rand(n, 2, generator=g) * 120 + 2], 1)
    LD = (5 * nc + 1 + 3) // 4 * 4
    head = torch.zeros(n, LD)
    head[:, :nc + 1] = torch.randn(n, nc + 1, generator=g) * 2.5
    head[:, nc + 1:5 * nc + 1] = torch.randn(n, 4 * nc, generator=g)
    if n > 3:                                            # duplicated RoIs: identical boxes and scores
        roi[n // 2] = roi[0]; head[n // 2] = head[0]
    coder = DeltaXYWHBBoxCoder(target_stds=(0.1, 0.1, 0.2, 0.2))
    img_hw = torch.tensor([[400., 420.]])
    got = ops.bbox_post(head.to(dev), LD, roi.to(dev), torch.tensor([0, n]), img_hw.to(dev), nc, thr, coder, 0.5, max_out)
    ref = mock.bbox_post(head, LD, roi, torch.tensor([0, n]), img_hw, nc, thr, coder, 0.5, max_out)
    got = {key: v.cpu() for key, v in got.items()}
    k = int(ref['count'][0])
    assert int(got['count'][0]) == k, (n, nc, thr, max_out)
    pairs = match_detections(got['boxes'][0, :k], got['scores'][0, :k], got['ids'][0, :k].long(),
                             ref['boxes'][0, :k], ref['scores'][0, :k], ref['ids'][0, :k].long())
    assert len(pairs) == k, (n, nc, thr, max_out)


def check_query_topk(ops, dev, B, Nq, nc, k, seed):
    """the fusion head's top-k over (query, class) (rsp_query_topk) with an exact tie between the first and the last query
    against instance_postprocess: the same scores, the same flat indices up to the order inside runs of equal scores"""
    import torch_ops_mock as mock
    g = torch.Generator().manual_seed(seed)
    k = min(k, Nq * nc)
    cls = torch.randn(B, Nq, nc + 1, generator=g) * 2
    if Nq > 2:
        cls[:, Nq - 1] = cls[:, 0]                        # an exact tie between the first and the last query
    sc, fl = ops.query_topk(cls.contiguous().to(dev), k)
    sc, fl = sc.cpu(), fl.cpu()
    rs, rf = mock.query_topk(cls, k)
    assert float((sc - rs).abs().max()) < 1e-6, (B, Nq, nc, k)
    for b in range(B):                                   # equal up to the order inside runs of (numerically) equal scores
        bad = (fl[b] != rf[b]).nonzero()[:, 0].tolist()
        for i in bad:
            j = (rf[b] == fl[b, i]).nonzero()
            assert j.numel() == 1 and abs(float(rs[b, int(j[0, 0])]) - float(sc[b, i])) < 2e-7, (b, i)


def check_roi_align(ops, dev, K, P, seed):
    """RoIAlign with RoIs that are tiny, huge, partly or wholly outside the image, on every pyramid level, against the C
    restatement of mmcv RoIAlign
    (samples exactly on the cuts, the last row and the level thresholds: check_exact_roi_align, tests/_sampler_props.py)"""
    import torch_ops_mock as mock
    g = torch.Generator().manual_seed(seed)
    B, C = 2, 8
    strides, sizes = [4, 8, 16, 32], [(32, 40), (16, 20), (8, 10), (4, 5)]
    feats = [torch.randn(B, h, w, C, generator=g) for h, w in sizes]
    pes = [torch.randn(h, w, C, generator=g) if i % 2 == 0 else None for i, (h, w) in enumerate(sizes)]
    xy = torch.rand(K, 2, generator=g) * 200 - 30                     # some start outside the 128 x 160 image
    wh = torch.exp(torch.rand(K, 2, generator=g) * 6)                 # 1 .. 400 pixels: every level
    rois = torch.cat([torch.randint(0, B, (K, 1), generator=g).float(), xy, xy + wh], 1)
    got = ops.roi_align(_to(dev, *feats), _to(dev, *pes), rois.to(dev), P, strides).cpu()
    ref = mock.roi_align(feats, pes, rois, P, strides)
    assert float((got - ref).abs().max()) < 2e-5, (K, P)


def check_msdeform_attn(ops, dev, L, hd, seed):
    """MSDeformAttn with L levels of random sizes and sampling offsets that leave the maps"""
    import torch_ops_mock as mock
    g = torch.Generator().manual_seed(seed)
    shapes = [(int(torch.randint(1, 9, (1,), generator=g)), int(torch.randint(1, 9, (1,), generator=g))) for _ in range(L)]
    ntok, B, D = sum(h * w for h, w in shapes), 2, 8 * hd
    value = torch.randn(B * ntok, D, generator=g)
    ow = torch.cat([torch.randn(B * ntok, 8 * L * 4 * 2, generator=g) * 3, torch.randn(B * ntok, 8 * L * 4, generator=g)], 1).contiguous()
    ref_pts = torch.rand(ntok, 2, generator=g)
    got = ops.msdeform_attn(*_to(dev, value, ow, ref_pts), B, ntok, shapes, head_dim=hd).cpu()
    assert float((got - mock.msdeform_attn(value, ow, ref_pts, B, ntok, shapes, head_dim=hd)).abs().max()) < 2e-5, (L, hd)


def check_resample(ops, dev, B, h, w, ho, wo, seed):
    """bilinear resizing up and down, GroupNorm with add / ReLU, the query prompter's attention-mask rule incl. a fully
    blocked row
    (dyadic ratios, from and to 1 x 1 and logits that tie with the threshold: check_exact_interp, tests/_sampler_props.py)"""
    import torch_ops_mock as mock
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, h, w, 128, generator=g)
    xd = x.to(dev)
    assert float((ops.resize_bilinear(xd, (ho, wo)).cpu() - mock.resize_bilinear(x, (ho, wo))).abs().max()) < 1e-5
    gam, bet, add = torch.randn(128, generator=g), torch.randn(128, generator=g), torch.randn(B, h * w, 128, generator=g)
    xs, xsd = x.view(B, h * w, 128), xd.view(B, h * w, 128)
    gd, bd, ad = _to(dev, gam, bet, add)
    assert float((ops.groupnorm(xsd, gd, bd, 32, add=ad).cpu() - mock.groupnorm(xs, gam, bet, 32, add=add)).abs().max()) < 5e-5
    assert float((ops.groupnorm(xsd, gd, bd, 32, relu=True).cpu() - mock.groupnorm(xs, gam, bet, 32, relu=True)).abs().max()) < 5e-5
    mpp = torch.randn(B, 5, h, w, generator=g) * 3
    mpp[:, 0] = -5.0                                                  # a fully blocked row: cleared (models.py:439-442)
    a, b = ops.query_attn_mask(mpp.contiguous().to(dev), (ho, wo)).cpu(), mock.query_attn_mask(mpp, (ho, wo))
    diff = a != b
    if bool(diff.any()):                                              # only where the resized logit ties with the threshold
        z = F.interpolate(mpp, (ho, wo), mode='bilinear', align_corners=False).flatten(2)
        assert float(z[diff].abs().max()) < 1e-5


def check_t2i_fold(ops, dev, R, N, T):
    """the folded token -> image attention (T <= 8 and T > 8: both head-count instantiations) against fp64 and the unfolded
    kernels"""
    import test_gpu_kernels as tk
    tk.test_sam_t2i_fold_matches_fp64_attention(dev, R, N, T)


def upscale_decoder(dev, seed=3):
    """(decoder, packed weights, upscale LayerNorm) of a SamMaskDecoderHIP with seeded synthetic weights on `dev`"""
    from rsprompter_amd.sam_decoder import SamMaskDecoderHIP
    from rsprompter_amd.synth import synth_state_dict
    dec = SamMaskDecoderHIP()
    dec.load_state_dict(synth_state_dict(dec, seed))
    dec = dec.to(dev)
    dec._pack()
    return dec, dec._packed, dec.upscale_layer_norm


def check_upscaler(ops, dev, dec, R, h, w, seed):
    """sam_upscale_fused_kernel against the two-kernel form (ConvT + LN + GELU into planes, then sam_upscale2_kernel with the
    hyper-network product) for h != w, RoI sizes that are no multiple of the 128-row tile, RoIs smaller than one tile.
    dec: upscale_decoder(dev)."""
    _, P, ln = dec
    g = torch.Generator().manual_seed(seed)
    x = ops.to_planes((torch.randn(R * h * w, 256, generator=g) * 1.5).to(dev))
    hy = torch.randn(R, 32, generator=g).to(dev)
    up = ops.conv_transpose2x2(x.view(R, h, w, 256), *P['up1'], act=ops.ACT_GELU, ln=(ln.weight, ln.bias, 1e-6))
    two = ops.conv_transpose2x2(up, *P['up2'], act=ops.ACT_GELU, hyper=hy)
    one = ops.sam_upscale_fused(x, P['up1'][0], P['up1'][1], ln.weight, ln.bias, 1e-6, P['up2p'][0], P['up2p'][1], hy, h, w)
    assert one.shape == two.shape == (R, 4 * h, 4 * w)
    assert_upscale_close(one, two, (R, h, w))


def check_mask_embed(ops, dev, R, B, he, we, C, seed):
    """SamMaskEmbedding of the query prompter (mask_embed_kernel: two stride-2 convolutions with LayerNorm2d + GELU, a 1x1
    convolution, + the image embedding of the prompt set's image; models.py:305, HF:569-601) against the reference's
    torch calls"""
    import torch_ops_mock as mock
    g = torch.Generator().manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    prm = dict(conv1_w=rn(4, 1, 2, 2), conv1_b=rn(4), ln1_w=rn(4), ln1_b=rn(4), conv2_w=rn(16, 4, 2, 2) * 0.5, conv2_b=rn(16),
               ln2_w=rn(16), ln2_b=rn(16), conv3_w=rn(C, 16) * 0.3, conv3_b=rn(C))
    mpp = rn(R, 4 * he, 4 * we) * 4
    emb = rn(B * he * we, C)
    roi_img = torch.randint(0, B, (R,), generator=g).to(torch.int32)
    got = ops.sam_mask_embed(*_to(dev, mpp, emb, roi_img), {key: v.to(dev) for key, v in prm.items()}, he, we).cpu()
    ref = mock.sam_mask_embed(mpp, emb, roi_img, prm, he, we)
    assert got.shape == ref.shape and float((got - ref).abs().max()) < 5e-5 * max(1.0, float(ref.abs().max())), (R, B, he, we, C)


def check_mask_embed_refuses_narrow_channels(ops, dev):
    """a channel count that would leave lanes out of the output loop's wave shuffle is refused (C = 32 once gave wrong rows
    for every pixel beyond the 8th; the reference only has C = 256)"""
    import pytest
    prm = dict(conv1_w=torch.randn(4, 1, 2, 2), conv1_b=torch.randn(4), ln1_w=torch.randn(4), ln1_b=torch.randn(4),
               conv2_w=torch.randn(16, 4, 2, 2), conv2_b=torch.randn(16), ln2_w=torch.randn(16), ln2_b=torch.randn(16),
               conv3_w=torch.randn(32, 16), conv3_b=torch.randn(32))
    with pytest.raises(RuntimeError):
        ops.sam_mask_embed(torch.randn(2, 12, 12).to(dev), torch.randn(9, 32).to(dev), torch.zeros(2, dtype=torch.int32).to(dev),
                           {key: v.to(dev) for key, v in prm.items()}, 3, 3)


def check_gather_rows(ops, dev, n_src, n_idx, C, seed):
    """the row gather against indexing"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(n_src, C, generator=g)
    idx = torch.randint(0, n_src, (n_idx,), generator=g).to(torch.int32)
    if n_idx == 0:
        return
    assert torch.equal(ops.gather_rows(src.to(dev), idx.to(dev)).cpu(), src[idx.long()]), (n_src, n_idx, C)


# --------------------------------------------------------------------------------------------------- failure signatures
# tests/test_kernel_props_selfcheck_cpu.py applies these to an exact reference and asserts that the comparisons above
# reject them.
def drop_hyper_addend(masks, u, hyper, h, w, group32, sub, c):
    """the round-5 signature: the addend u[.., c] * hyper[r, c] of the 32-channel hyper dot is missing for pixels 16-31 of the
    32-pixel row group `group32` (flat input pixel rows r*h*w + y*w + x) in sub-pixel sub = 8 dy1 + 4 dx1 + 2 dy2 + dx2.
    masks [R, 4h, 4w]; u [R, 4h, 4w, 32]: the GELU output in front of the dot."""
    out = masks.clone()
    dy1, dx1, dy2, dx2 = (sub >> 3) & 1, (sub >> 2) & 1, (sub >> 1) & 1, sub & 1
    for p in range(32 * group32 + 16, min(32 * group32 + 32, masks.shape[0] * h * w)):
        r, rem = divmod(p, h * w)
        y, x = divmod(rem, w)
        oy, ox = 4 * y + 2 * dy1 + dy2, 4 * x + 2 * dx1 + dx2
        out[r, oy, ox] -= u[r, oy, ox, c] * hyper[r, c]
    return out


def masks_to_pixel_rows(masks, h, w):
    """[R, 4h, 4w] -> [R*h*w, 16]: the 16 outputs of every input pixel (sub-pixel 8 dy1 + 4 dx1 + 2 dy2 + dx2)"""
    R = masks.shape[0]
    return masks.view(R, h, 2, 2, w, 2, 2).permute(0, 1, 4, 2, 5, 3, 6).reshape(R * h * w, 16)


def pixel_rows_to_masks(px, R, h, w):
    return px.view(R, h, w, 2, 2, 2, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(R, 4 * h, 4 * w)


def tile_written_from(masks, h, w, t, src):
    """the output of 128-pixel tile `src` written in place of tile t (a wrong cross-tile prefetch)"""
    px = masks_to_pixel_rows(masks, h, w).clone()
    n = min(128, px.shape[0] - 128 * t, px.shape[0] - 128 * src)
    px[128 * t:128 * t + n] = px[128 * src:128 * src + n]
    return pixel_rows_to_masks(px, masks.shape[0], h, w)
