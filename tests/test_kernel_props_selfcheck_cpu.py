"""CPU (`-m "not gpu"`): the comparisons of the kernel property and decoder-scale tests reject the failures this project has had.

Each test builds a small fp64 reference with the restatements of tests/_kernel_props.py, applies a known failure signature
to it and asserts that the helper the GPU tests use rejects the result -- at the fault's natural size and at a FAINT size,
a few times the bound the GPU tests apply (pinned here as FAINT, independently of the helpers' constants), so that a bound
loosened tenfold makes these tests fail.  The exact reference rounded to fp32 must pass.  The precedent is the emulator's
`lazy_dma(ignore_waits=True)` self-test."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kernel_props as kp  # noqa: E402

FAINT = 3 * 2e-5        # the faint signatures' size: 3x the 2e-5 bound of the upscaler (relative) and fold (absolute) checks


def _decoder(seed):
    from rsprompter_amd.sam_decoder import SamMaskDecoderHIP
    from rsprompter_amd.synth import synth_state_dict
    dec = SamMaskDecoderHIP()
    dec.load_state_dict(synth_state_dict(dec, seed))
    return dec


def _scale(ref):
    return max(1.0, float(ref.abs().max()))


def test_upscaler_check_rejects_a_missing_hyper_addend():
    """round 5: one addend of the 32-channel hyper dot missing for pixels 16-31 of one 32-pixel group in one sub-pixel (the
    low product of lanes 48-63 lost when two waves shared a SIMD)"""
    wts = kp.decoder_upscale_weights(_decoder(3), 'cpu')
    g = torch.Generator().manual_seed(5)
    R, h, w = 3, 12, 10                                      # 360 pixels: RoIs straddle the 32-pixel groups
    x = torch.randn(R * h * w, 256, generator=g, dtype=torch.float64) * 1.5
    hy = torch.randn(R, 32, generator=g, dtype=torch.float64)
    u = kp.upscale_pre_dot_f64(x.view(R, h, w, 256), *wts)
    ref = torch.einsum('ryxc,rc->ryx', u, hy)
    assert torch.allclose(ref, kp.upscale_ref_f64(x, wts, hy, h, w, group=1), rtol=0, atol=1e-12)
    kp.assert_upscale_close(ref.float(), ref)
    group, sub, c = 3, 6, 17                                 # pixels 112-127: RoI 0's last rows and RoI 1's first
    with pytest.raises(AssertionError):
        kp.assert_upscale_close(kp.drop_hyper_addend(ref, u, hy, h, w, group, sub, c).float(), ref)
    # faint: the dropped channel's hyper coefficients scaled so that the missing addend is FAINT x the output range
    bad = kp.drop_hyper_addend(ref, u, hy, h, w, group, sub, c)
    d = float((bad - ref).abs().max())
    hy2 = hy.clone()
    hy2[:, c] *= FAINT * _scale(ref) / d
    ref2 = torch.einsum('ryxc,rc->ryx', u, hy2)
    bad2 = kp.drop_hyper_addend(ref2, u, hy2, h, w, group, sub, c)
    assert 2.0 < float((bad2 - ref2).abs().max()) / (2e-5 * _scale(ref2)) < 5.0
    with pytest.raises(AssertionError):
        kp.assert_upscale_close(bad2, ref2)


def test_upscaler_check_rejects_a_tile_written_from_the_next_round():
    """the output of tile t + 256 written into tile t: what a wrong cross-tile prefetch of the persistent upscaler (the next
    tile's pixel rows requested at chunks 6-7, its first W1 chunk at chunk 7) would produce"""
    wts = kp.decoder_upscale_weights(_decoder(3), 'cpu')
    g = torch.Generator().manual_seed(6)
    R, h, w = 130, 16, 16                                    # 260 tiles of 128 pixels: tiles 0-3 have a next round
    t = 2
    x = torch.randn(R * h * w, 256, generator=g, dtype=torch.float64) * 1.5
    hy = torch.randn(R, 32, generator=g, dtype=torch.float64)
    ref = kp.upscale_ref_f64(x, wts, hy, h, w)
    kp.assert_upscale_close(ref.float(), ref)
    with pytest.raises(AssertionError):
        kp.assert_upscale_close(kp.tile_written_from(ref, h, w, t, t + 256), ref)
    # faint: tile t + 256's pixels (and its RoI's hyper vector) equal tile t's up to a small perturbation of the pixels,
    # sized so that the swap is FAINT x the range
    a, b = slice(128 * t, 128 * t + 128), slice(128 * (t + 256), 128 * (t + 256) + 128)
    hy2 = hy.clone()
    hy2[128 * (t + 256) // (h * w)] = hy[128 * t // (h * w)]
    noise = torch.randn(128, 256, generator=g, dtype=torch.float64)
    eps = 1e-3
    for it in range(4):
        if it:
            eps *= FAINT * _scale(ref2) / d
        x2 = x.clone()
        x2[b] = x2[a] + eps * noise
        ref2 = kp.upscale_ref_f64(x2, wts, hy2, h, w)
        d = float((kp.tile_written_from(ref2, h, w, t, t + 256) - ref2).abs().max())
    assert 2.0 < d / (2e-5 * _scale(ref2)) < 5.0
    with pytest.raises(AssertionError):
        kp.assert_upscale_close(kp.tile_written_from(ref2, h, w, t, t + 256), ref2)


def test_fold_check_rejects_a_skipped_key_tile():
    """one key tile (32 keys) left out of the folded attention's online softmax"""
    dec = _decoder(21)
    wts = kp.fold_weights(dec, 'final', 'cpu')
    g = torch.Generator().manual_seed(7)
    R, N, T, j = 2, 256, 10, 5
    keys = torch.randn(R * N, 256, generator=g, dtype=torch.float64) * 1.5
    pe = torch.randn(N, 256, generator=g, dtype=torch.float64)
    tq = torch.randn(R * T, 128, generator=g, dtype=torch.float64) * 2.0
    ref = kp.t2i_ref_f64(tq, keys, pe, wts, R, T, N)
    kp.assert_fold_close(ref.float(), ref)
    skip = torch.zeros(N, dtype=torch.float64)
    skip[kp.FOLD_KEY_TILE * j:kp.FOLD_KEY_TILE * (j + 1)] = -math.inf
    with pytest.raises(AssertionError):
        kp.assert_fold_close(kp.t2i_ref_f64(tq, keys, pe, wts, R, T, N, key_bias=skip), ref)
    # faint: the tile's scores lowered by `b` until its softmax weight moves the output by FAINT
    bias = torch.zeros(N, dtype=torch.float64)
    b = 0.0
    for it in range(6):
        if it:
            b += math.log(FAINT / d)
        bias[kp.FOLD_KEY_TILE * j:kp.FOLD_KEY_TILE * (j + 1)] = b
        ref2 = kp.t2i_ref_f64(tq, keys, pe, wts, R, T, N, key_bias=bias)
        d = float((kp.t2i_ref_f64(tq, keys, pe, wts, R, T, N, key_bias=skip) - ref2).abs().max())
    assert 2.0 < d / 2e-5 < 5.0
    with pytest.raises(AssertionError):
        kp.assert_fold_close(kp.t2i_ref_f64(tq, keys, pe, wts, R, T, N, key_bias=skip), ref2)


# ------------------------------------------------------------------------------------------------------- the mask-field checks
import _mask_field_props as mf  # noqa: E402

# the smaller exact cases: every form, both quad / pixel paths, strips below and beyond the row tile
_MF_CASES = tuple(c for c in mf.EXACT_CASES if mf.pixels(c) <= 4096)


def test_mask_field_fake_reproduces_the_oracle():
    """the stand-in's written-out bilinear resize is F.interpolate in fp64, and the unmutated stand-in passes every exact case"""
    g = torch.Generator().manual_seed(1)
    for c in mf.EXACT_CASES + mf.TOL_CASES[:1]:
        low = torch.randn(2, *c.hw, generator=g)
        f, seen = mf.FakeOps()._field(low, c.img, c.crop, c.out)
        assert bool(seen.all()) and float((f - mf.field_f64(low, c.img, c.crop, c.out)).abs().max()) < 1e-12, c
    for c in mf.EXACT_CASES:
        mf.check_exact_field(mf.FakeOps(), 'cpu', c, seed=101)
    # the crop tables: of all the cases, and of the pool the mutation below is run with -- an assertion that fails there
    # whatever `ops` does would count the mutation as rejected
    for cases in (mf.EXACT_CASES, _MF_CASES):
        for hw in mf.crop_groups(cases):
            mf.check_exact_crops(mf.FakeOps(), 'cpu', hw, seed=101, cases=cases)


@pytest.mark.parametrize('mutation', mf.MUTATIONS)
def test_exact_field_check_rejects(mutation):
    """check_exact_field raises AssertionError on at least one exact case for every mutation of the stand-in: `>=` for `>` at
    the logits threshold and the reverse in mask_post, stage 1 without the half-pixel offset, stage 2 skipped, the strip's row
    pair not refreshed, the last quad of a row / the rows beyond the last full tile not written, the highest index winning a
    tie, qidx ignored, the box maximum off by one"""
    fake = mf.FakeOps(mutation)
    rejected = []
    for c in _MF_CASES:
        try:
            mf.check_exact_field(fake, 'cpu', c, seed=101)
        except AssertionError:
            rejected.append(c)
    assert rejected, mutation
    # the threshold and index mutations change no value: only ties show them, and every case has ties
    if mutation in ('ge_at_the_logits_threshold', 'gt_in_mask_post', 'qidx_ignored', 'box_max_off_by_one'):
        assert len(rejected) == len(_MF_CASES), (mutation, len(rejected))
    # every box is shifted by its row's origin, so the crop table shows the box mutation at every (h, w)
    if mutation == 'box_max_off_by_one':
        for hw in mf.crop_groups(_MF_CASES):
            with pytest.raises(AssertionError):
                mf.check_exact_crops(fake, 'cpu', hw, seed=101, cases=_MF_CASES)


# ---------------------------------------------------------------------------------------------------------- the sampler checks
import _sampler_props as sp  # noqa: E402

# sampler -> (mutations, the exact-tier bodies that must show them, their cases); rsp_resize_pad's siblings share its family
_SAMPLERS = {
    'roi_align': (sp.ROI_MUTATIONS, ((sp.check_exact_roi_align, sp.ROI_EXACT),)),
    'paste_masks': (sp.PASTE_MUTATIONS, ((sp.check_exact_paste, sp.PASTE_EXACT),)),
    'resize_pad': (sp.RESIZE_MUTATIONS, ((sp.check_exact_resize_pad, sp.RESIZE_EXACT), (sp.check_exact_windows, sp.WINDOW_EXACT))),
    'interpolate': (sp.INTERP_MUTATIONS, ((sp.check_exact_interp, sp.INTERP_EXACT),)),
    'msdeform_attn': (sp.MSDA_MUTATIONS, ((sp.check_exact_msdeform, sp.MSDA_EXACT),)),
}


def test_sampler_fake_reproduces_the_oracles():
    """the unmutated stand-in (the fp32 restatements) passes every exact case of the five conventions -- so an
    AssertionError under a mutation below comes from the comparison with `ops`, not from a precondition of the case, which
    never looks at `ops` -- and the fp64 restatements agree with the independent statements this suite already has: the C
    restatement of mmcv RoIAlign, mmdet's mask paste and the cv2 restatement"""
    fake = sp.FakeOps()
    for muts, bodies in _SAMPLERS.values():
        assert len(muts) >= 4
        for body, cases in bodies:
            for c in cases:
                body(fake, 'cpu', c)
    import torch_ops_mock as mock
    case = sp.ROI_TOL[0]
    feats, pes, rois = sp.roi_tol_inputs(case)
    a = sp.roi_align_ref(feats, pes, rois, case.P, [4, 8, 16, 32])
    assert float((a - mock.roi_align(feats, pes, rois, case.P, [4, 8, 16, 32]).double()).abs().max()) < 1e-4
    pc = sp.PASTE_TOL[1]
    logits, labels, boxes = sp.paste_tol_inputs(pc)
    field, region = sp.paste_field(logits, labels, boxes, pc.img)
    d = sp.paste_bytes(field, region, -1.0).int() - mock.paste_masks(logits, labels, boxes, pc.img, -1.0).int()
    assert int(d.abs().max()) <= 1 and float((d != 0).float().mean()) < 2e-3
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (37, 53, 3), generator=g).to(torch.uint8)
    b = sp.resize_pad_ref(img, (50, 71), (64, 72), (1.0, 2.0, 3.0))
    assert float((b - mock.resize_pad(img, (50, 71), (64, 72), (1.0, 2.0, 3.0)).double()).abs().max()) < 1e-3


def _sampler_check_rejects(sampler, mutation):
    fake = sp.FakeOps(mutation)
    rejected = 0
    for body, cases in _SAMPLERS[sampler][1]:
        for c in cases:
            try:
                body(fake, 'cpu', c)
            except AssertionError:
                rejected += 1
    assert rejected, (sampler, mutation)


@pytest.mark.parametrize('mutation', sp.ROI_MUTATIONS)
def test_exact_roi_align_check_rejects(mutation):
    """check_exact_roi_align raises AssertionError on at least one exact case: no -0.5, an inclusive cut at H or at -1, the
    low clamp missing, the top index unclamped, a fixed 2 x 2 grid, a level one too low at an exact power of two, the PE skipped"""
    _sampler_check_rejects('roi_align', mutation)


@pytest.mark.parametrize('mutation', sp.PASTE_MUTATIONS)
def test_exact_paste_masks_check_rejects(mutation):
    """check_exact_paste: `>` for `>=`, align_corners=True, border padding, the soft mode's region without its margin, the
    label ignored, an infinite coordinate not zeroed, rounding for truncation"""
    _sampler_check_rejects('paste_masks', mutation)


@pytest.mark.parametrize('mutation', sp.RESIZE_MUTATIONS)
def test_exact_resize_pad_check_rejects(mutation):
    """check_exact_resize_pad / check_exact_windows: no half pixel, the right and bottom edge unclamped, padding not
    normalised, the mean indexed before the swap, the scale taken from the canvas, a window's origin read as (y, x)"""
    _sampler_check_rejects('resize_pad', mutation)


@pytest.mark.parametrize('mutation', sp.INTERP_MUTATIONS)
def test_exact_interpolate_check_rejects(mutation):
    """check_exact_interp: align_corners=True, no half pixel, `<=` for `<` at the threshold, the fully blocked row kept, the
    blocked-row rule taken over the batch"""
    _sampler_check_rejects('interpolate', mutation)


@pytest.mark.parametrize('mutation', sp.MSDA_MUTATIONS)
def test_exact_msdeform_attn_check_rejects(mutation):
    """check_exact_msdeform: x and y swapped, a level read from the next map's start, border padding, a softmax over the
    points of one level only, align_corners=True, offsets divided by the first level's size"""
    _sampler_check_rejects('msdeform_attn', mutation)


def test_roi_align_tolerance_check_rejects_a_dropped_level_epsilon():
    """the 1e-6 of floor(log2(sqrt(w h) / 56 + 1e-6)) moves a roi only when sqrt(w h) / 56 is within 1e-6 below a power of
    two, which no dyadic roi is: the tolerance tier carries two such rois, and its body rejects a stand-in without the epsilon"""
    sp.check_roi_align_tolerance(sp.FakeOps(), 'cpu', report=lambda line: None)
    with pytest.raises(AssertionError):
        sp.check_roi_align_tolerance(sp.FakeOps('level_epsilon_dropped'), 'cpu', report=lambda line: None)


# ------------------------------------------------------------------------------------------------ the detection selection checks
import _det_props as dp  # noqa: E402

# family -> (mutations, the exact- and sequence-tier bodies that must show them, their cases).  The 4300-row walk and the
# 16384 / 16385-row capacities repeat what smaller cases show: they are left to the device
_DET_NMS = tuple(c for c in dp.nms_cases() if c.emu)
_DET = {
    'nms': (dp.NMS_MUTATIONS, ((dp.check_nms, _DET_NMS), (dp.check_nms_flat, _DET_NMS))),
    'decode': (dp.DECODE_MUTATIONS, ((dp.check_decode, dp.decode_cases()),)),
    'bbox_post': (dp.POST_MUTATIONS, ((dp.check_post, dp.post_cases()),)),
    'rpn_topk': (dp.TOPK_MUTATIONS, ((dp.check_exact_rpn_topk, dp.RPN_TOPK),)),
    'query_topk': (dp.QUERY_MUTATIONS, ((dp.check_exact_query_topk, dp.QUERY_EXACT), (dp.check_seq_query_topk, dp.QUERY_SEQ))),
}


def test_det_fake_reproduces_the_restatements():
    """the unmutated stand-in (the fp32 sequence) passes every exact and sequence body of the five entry points -- so an
    AssertionError under a mutation below comes from the comparison with `ops`, not from a precondition of the case, which
    never looks at `ops` -- and the tolerance bodies"""
    fake = dp.FakeOps()
    for muts, bodies in _DET.values():
        for body, cases in bodies:
            for c in cases:
                body(fake, 'cpu', c)
    quiet = lambda line: None
    for body in (dp.check_decode_tolerance, dp.check_post_tolerance, dp.check_rpn_topk_tolerance, dp.check_query_topk_tolerance):
        body(fake, 'cpu', quiet)


def _det_check_rejects(family, mutation):
    """-> the names of the cases whose body raises AssertionError under the mutation"""
    fake = dp.FakeOps(mutation)
    rejected = []
    for body, cases in _DET[family][1]:
        for c in cases:
            try:
                body(fake, 'cpu', c)
            except AssertionError:
                rejected.append((body.__name__, getattr(c, 'name', c)))
    assert rejected, (family, mutation)
    return rejected


@pytest.mark.parametrize('mutation', dp.NMS_MUTATIONS)
def test_nms_check_rejects(mutation):
    """check_nms / check_nms_flat: `>=` at the IoU threshold, inter > thr * union, the IoU in fp64, a contracted id * unit + box,
    the unit without its + 1, the max taken over the capacity rows, the count ignored, ties by descending index, a suppressed box
    that suppresses, max_out counting visited rows, 0 / 0 read as suppressed -- and every case that names the mutation rejects it"""
    rejected = {name for body, name in _det_check_rejects('nms', mutation) if body == 'check_nms'}
    named = {c.name for c in _DET_NMS if mutation in c.kills}
    assert named and named <= rejected, (mutation, sorted(named - rejected))
    if mutation in ('iou_fp64', 'iou_cross_multiplied', 'offset_contracted'):   # value-preserving on dyadic inputs: the sequence tier's
        assert all(dp.nms_case(n).tier == 'seq' for n in rejected), (mutation, rejected)


@pytest.mark.parametrize('mutation', dp.DECODE_MUTATIONS)
def test_rpn_decode_check_rejects(mutation):
    """check_decode: contracted d * std + mean and pw * dx + px, the size clamped from both sides under add_ctr_clamp, the centre
    clamp skipped, a clip to size - 1, `>=` at min_bbox_size, min_bbox_size = 0 read as off"""
    rejected = {name for _, name in _det_check_rejects('decode', mutation)}
    named = {c.name for c in dp.decode_cases() if mutation in c.kills}
    assert named and named <= rejected, (mutation, sorted(named - rejected))
    if mutation in ('delta_contracted', 'centre_contracted'):
        assert all(dp.decode_case(n).tier == 'seq' for n in rejected), (mutation, rejected)


@pytest.mark.parametrize('mutation', dp.POST_MUTATIONS + ('iou_ge', 'ties_by_index_descending'))
def test_bbox_post_check_rejects(mutation):
    """check_post: `>=` at score_thr, the background column as a candidate, a softmax without its max, a division by the scale
    factor, a reciprocal that is not rounded to nearest; and two mistakes of the NMS behind it -- every case that names the mutation
    rejects it"""
    rejected = {name for _, name in _det_check_rejects('bbox_post', mutation)}
    named = {c.name for c in dp.post_cases() if mutation in c.kills}
    assert named and named <= rejected, (mutation, sorted(named - rejected))


@pytest.mark.parametrize('mutation', dp.TOPK_MUTATIONS)
def test_rpn_topk_check_rejects(mutation):
    """check_exact_rpn_topk: a -0.0 logit ranked below +0.0, ties by descending index, the ties with the k-th score taken from
    the end, a sorted level although n <= nms_pre -- every case that names the mutation (dp.topk_kills) rejects it"""
    rejected = {name for _, name in _det_check_rejects('rpn_topk', mutation)}
    named = {c.name for c in dp.RPN_TOPK if mutation in dp.topk_kills(c)}
    assert named and named <= rejected, (mutation, sorted(named - rejected))


@pytest.mark.parametrize('mutation', dp.QUERY_MUTATIONS)
def test_query_topk_check_rejects(mutation):
    """check_exact_query_topk: ties by descending index, the ties with the k-th score taken from the end, a class-major flat index;
    check_seq_query_topk: a reciprocal that is not rounded to nearest -- every case that names the mutation rejects it"""
    by_body = _det_check_rejects('query_topk', mutation)
    exact = {name for body, name in by_body if body == 'check_exact_query_topk'}
    if mutation == 'division_by_truncated_reciprocal':
        named, rejected = set(dp.QUERY_SEQ), {name for body, name in by_body if body == 'check_seq_query_topk'}
        assert not exact                                                     # 1 / 2^k is exact under any reciprocal: the exact tier cannot see it
    else:
        named, rejected = {c for c in dp.QUERY_EXACT if mutation in dp.query_kills(c)}, exact
    assert named and named <= rejected, (mutation, named - rejected)


def test_det_tolerance_checks_reject_what_only_real_arithmetic_shows():
    """the upper size clamp and the expf path are tolerance-tier only (dw != 0 has no exact form): a stand-in that clamps the size
    from both sides under add_ctr_clamp fails check_decode_tolerance on the case with dw far below -max_ratio; the tolerance
    tier's exact ties (a duplicated query) still hold the index order"""
    quiet = lambda line: None
    with pytest.raises(AssertionError):
        dp.check_decode_tolerance(dp.FakeOps('size_clamped_from_both_sides_under_ctr_clamp'), 'cpu', quiet, cases=dp.DECODE_TOL[1:2])
    with pytest.raises(AssertionError):
        dp.check_query_topk_tolerance(dp.FakeOps('ties_by_index_descending'), 'cpu', quiet)
