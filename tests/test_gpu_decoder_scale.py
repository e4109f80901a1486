"""GPU (`-m gpu`): the SAM decoder's per-RoI kernels at production scale, every output element against float64.

The kernel tier elsewhere checks these kernels at a few RoIs; the product runs them at R = 800 (the bench) and up to
R = 1023 per launch (decode() splits larger prompt sets into equal chunks below the folded attention's 32-bit addressing
limit).  The persistent fused upscaler only walks tiles (`tile += gridDim.x`, the next tile's pixel rows and first W1 chunk
requested inside the current tile's epilogue) once a launch has more than 256 tiles of 128 pixels.  References: float64
torch restatements on the device (tests/_kernel_props.py), computed in groups of RoIs; every test stays well under 32 GB of
device memory.  Weights: SamMaskDecoderHIP with synth_state_dict."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kernel_props as kp  # noqa: E402

pytestmark = pytest.mark.gpu


def _randn(dev, seed, *shape):
    return torch.randn(*shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


@pytest.fixture(scope='module')
def upscaler(dev):
    dec, P, ln = kp.upscale_decoder(dev, 3)
    return dec, P, ln, kp.decoder_upscale_weights(dec, dev)


@pytest.mark.parametrize('R,h,w', [(1, 1, 1),           # one pixel
                                   (2, 13, 7),          # h != w
                                   (8, 64, 64),         # 256 tiles: exactly one per block
                                   (513, 8, 16),        # 513 tiles: block 0 walks 3, the others 2
                                   (37, 45, 40),        # RoIs straddle tiles; ragged last round
                                   (800, 64, 64)])      # the bench's shape: 100 tiles per block
def test_fused_upscaler_against_fp64(dev, upscaler, R, h, w):
    """ops.sam_upscale_fused (ConvT1 -> LayerNorm2d -> GELU -> ConvT2 -> GELU -> hyper dot, HF:513-531) against fp64, a second
    launch bit-identical, and the two-kernel chain (conv_transpose2x2 with the LayerNorm epilogue, then sam_upscale2_kernel
    with the hyper-network product: the multimask path) against the same fp64 restatement and against the fused kernel"""
    from rsprompter_amd import ops
    _, P, ln, wts = upscaler
    x = ops.to_planes(_randn(dev, 1000 + R, R * h * w, 256) * 1.5)
    hy = _randn(dev, 2000 + R, R, 32)
    args = (P['up1'][0], P['up1'][1], ln.weight, ln.bias, 1e-6, P['up2p'][0], P['up2p'][1], hy, h, w)
    one = ops.sam_upscale_fused(x, *args)
    again = ops.sam_upscale_fused(x, *args)
    torch.cuda.synchronize()
    assert torch.equal(one, again), 'fused upscaler: a second launch on the same inputs differs'
    del again
    ref = kp.upscale_ref_f64(x, wts, hy, h, w)
    e_one = kp.assert_upscale_close(one, ref, ('fused vs fp64', R, h, w))
    up = ops.conv_transpose2x2(x.view(R, h, w, 256), *P['up1'], act=ops.ACT_GELU, ln=(ln.weight, ln.bias, 1e-6))
    two = ops.conv_transpose2x2(up, *P['up2'], act=ops.ACT_GELU, hyper=hy)
    del up
    e_two = kp.assert_upscale_close(two, ref, ('two kernels vs fp64', R, h, w))
    e_12 = kp.assert_upscale_close(one, two, ('fused vs two kernels', R, h, w))
    print(f'upscaler R={R} h={h} w={w}: max|ref| {float(ref.abs().max()):.2f}; relative error fused {e_one:.2e}, '
          f'two kernels {e_two:.2e}, fused vs two kernels {e_12:.2e} (bound {kp.UPSCALE_TOL:.0e})')


@pytest.fixture(scope='module')
def fold_decoder(dev):
    from rsprompter_amd.sam_decoder import SamMaskDecoderHIP
    from rsprompter_amd.synth import synth_state_dict
    dec = SamMaskDecoderHIP()
    dec.load_state_dict(synth_state_dict(dec, 21))
    dec = dec.to(dev)
    dec._pack()
    return dec


@pytest.mark.parametrize('R', [800, 1023])
@pytest.mark.parametrize('T', [10, 6])
def test_t2i_fold_against_fp64_at_scale(dev, fold_decoder, R, T):
    """folded token -> image attention (dec._t2i_folded: sam_fold_expand -> k_proj^T GEMM -> sam_t2i_fold_kernel -> v_proj
    GEMM -> sam_fold_gather) at N = 4096 against the fp64 statement of HF:326-331; R = 1023 is the largest launch the key
    planes' 32-bit byte offsets allow (R * N * 512 < 2^31).  T = 10: the <5> instantiation, T = 6: <8>."""
    from rsprompter_amd import ops
    dec, N = fold_decoder, 4096
    keys_pl = ops.to_planes(_randn(dev, 3000 + R + T, R * N, 256) * 1.5)
    pe = _randn(dev, 4000, N, 256)
    tq = _randn(dev, 5000 + R + T, R * T, 128) * 2.0
    pe_t = dec._pe_terms(pe.contiguous())
    got = dec._t2i_folded('final', tq, keys_pl, pe_t, R, T, N)
    ref = kp.t2i_ref_f64(tq, keys_pl, pe, kp.fold_weights(dec, 'final', dev), R, T, N)
    e = kp.assert_fold_close(got, ref, ('t2i fold', R, T))
    print(f't2i fold R={R} N={N} T={T}: max abs error {e:.2e} (bound {kp.FOLD_TOL:.0e}), max|ref| {float(ref.abs().max()):.2f}')


def test_t2i_fold_refuses_1024_rois(dev, fold_decoder):
    """R = 1024 at N = 4096 is 2^31 bytes of key planes: the C entry's argument check refuses it (RSP_EINVAL) and launches
    nothing; the stream stays usable"""
    from rsprompter_amd import ops
    R, N = 1024, 4096
    keys = ops.empty_planes((R * N, 256), dev)
    pek = fold_decoder._pe_terms(_randn(dev, 4000, N, 256).contiguous())['final.pek_planes']
    qp, tqx = ops.empty_planes((R * 96, 256), dev), ops.empty_planes((R * 96, 128), dev)
    with pytest.raises(RuntimeError, match='rsp_sam_t2i_fold'):
        ops.sam_t2i_fold(keys, pek, qp, tqx, R=R, N=N, ncols=80)
    torch.cuda.synchronize()


@pytest.mark.parametrize('residual', ['rows', 'planes'])
def test_i2t_fused_against_fp64_at_scale(dev, residual):
    """ops.sam_i2t_fused, matrix-core form (planes out) = LayerNorm(residual + out_proj(image -> token attention)) (HF:340-348)
    at R = 800, N = 4096, T = 10, queries through a q map over 8 images, residual as per-image fp32 rows through the same map
    (layer 0) or as the per-RoI planes (layer 1), against the fp64 formula of test_sam_i2t_fused_matches_composition"""
    from rsprompter_amd import ops
    R, N, T, B = 800, 4096, 10, 8
    g = torch.Generator().manual_seed(77)
    roi_img = torch.sort(torch.randint(0, B, (R,), generator=g))[0].to(torch.int32).to(dev)
    scale = 16 ** -0.5
    q = _randn(dev, 6000, B * N, 128) * 2
    k, v = _randn(dev, 6001, R * T, 128), _randn(dev, 6002, R * T, 128)
    wo, bo = _randn(dev, 6003, 256, 128) / 128 ** 0.5, _randn(dev, 6004, 256)
    gamma, beta = _randn(dev, 6005, 256), _randn(dev, 6006, 256)
    kw = dict(R=R, T=T, N=N, scale=scale, eps=1e-6, planes=True, f32=False, q_map=roi_img)
    if residual == 'rows':
        res = _randn(dev, 6007, B * N, 256) * 3
        out = ops.sam_i2t_fused(q, k, v, wo, bo, gamma, beta, res=res, res_map=roi_img, **kw)
    else:
        res = ops.to_planes(_randn(dev, 6008, R * N, 256) * 3)
        out = ops.sam_i2t_fused(q, k, v, wo, bo, gamma, beta, res_planes=res, **kw)
    e, G = 0.0, 64
    rim = roi_img.long()
    for r0 in range(0, R, G):
        r1 = min(R, r0 + G)
        g_ = r1 - r0
        qq = q.view(B, N, 128)[rim[r0:r1]].double()
        if residual == 'rows':
            rr = res.view(B, N, 256)[rim[r0:r1]].double()
        else:
            rr = kp.planes_to_f64(res, r0 * N, r1 * N).view(g_, N, 256)
        qh = qq.view(g_, N, 8, 16).permute(0, 2, 1, 3)
        kh = k[r0 * T:r1 * T].double().view(g_, T, 8, 16).permute(0, 2, 1, 3)
        vh = v[r0 * T:r1 * T].double().view(g_, T, 8, 16).permute(0, 2, 1, 3)
        att = ((qh * scale) @ kh.transpose(-1, -2)).softmax(-1) @ vh
        y = att.permute(0, 2, 1, 3).reshape(g_, N, 128) @ wo.double().t() + bo.double() + rr
        ref = F.layer_norm(y, (256,), gamma.double(), beta.double(), 1e-6).reshape(g_ * N, 256)
        e = max(e, kp.abs_error(kp.planes_to_f64(out, r0 * N, r1 * N), ref))
        del qq, rr, qh, att, y, ref
    print(f'sam_i2t_fused R={R} N={N} T={T} residual={residual}: max abs error {e:.2e} (bound {kp.I2T_TOL:.0e})')
    assert e < kp.I2T_TOL, (residual, e)
