"""CPU (`-m "not gpu"`): the HIP kernels themselves, executed lane by lane on the host.

tests/wave_emu compiles the UNCHANGED sources of rsprompter_amd/csrc against a lane-level emulation of the gfx950
execution model (64-lane waves as fibers; MFMA 32x32x16 fragment layouts, DMA-to-LDS addressing, the transposing LDS
read, buffer-resource bounds, shuffles, barriers, divergence by EXEC mask) and these tests call `rsprompter_amd.ops`
through it on CPU tensors -- the same wrappers, descriptors and dispatch rules the GPU suite uses, at shapes that take
seconds.  They reuse the bodies of the `-m gpu` tests, so what is asserted here is what is asserted on the MI355X.
Not a product path: the package cannot load the emulated library (tests/wave_emu/harness.py swaps it in for one test)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _kernel_props as kp

DEV = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ with _Float16 vector support for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_emu_persistent_gemm_every_epilogue_form(emu):
    """gemm_f16x3_s2_kernel (buffer_load ... lds DMA ring, per-XCD tile tickets, per-wave LDS-transposed epilogues) and
    gemm_f16x3_dma_kernel: fp64 product and bit-equality between the two, specialised and run-time epilogues, ragged
    M / N, residual forms, GELU + plane outputs, column ranges, row maps with unwritten rows"""
    import test_gpu_gemm_s2 as t
    t.test_s2_plain_and_residual(DEV, 300, 64, 128)
    t.test_s2_gelu_and_plane_outputs(DEV, 200, 128, 64)
    t.test_s2_column_ranges_and_row_maps(DEV, 64, 128, 203)


def test_emu_window_attention_with_relpos_inside(emu):
    """attn_win_kernel: one-hot bias product, rel-pos tables through the matrix cores, Toeplitz gather through the per-wave
    LDS piece, lazy online softmax, transposing V reads, persistent blocks over windows incl. partly padded ones"""
    import test_gpu_kernels as t
    t.test_vit_window_attention_fused_relpos(DEV, 2, 10, 2, 64, 1, 0)
    t.test_vit_window_attention_fused_relpos(DEV, 3, 4, 2, 80, 1, 1)      # 18 (window, head) items over 16 persistent blocks


def test_emu_layernorm_and_plane_emitters(emu):
    import test_gpu_kernels as t
    t.test_layernorm(DEV)


def test_emu_detection_kernels_with_every_box_coder(emu):
    """rpn_topk / rpn_decode / bbox_post / batched NMS on the vectors of the REAL RPNHead / BBoxHead with the coder
    branches (means, stds, clip_border, add_ctr_clamp), and multiclass NMS above 16384 candidates (in-memory sort,
    32-word reduction)"""
    import test_gpu_samdet as t
    t.test_box_coder_branches_on_the_real_heads_vectors(DEV)
    t.test_bbox_post_many_classes(DEV)


def test_emu_nms_in_memory_sort_path(emu):
    """rsp_batched_nms with a capacity above the LDS sort (cap 20000 -> 32768 keys sorted in memory) and many exact score
    ties against the oracle's mmcv restatement"""
    from oracle import glue
    g = torch.Generator().manual_seed(3)
    n, cap, nid = 1500, 20000, 3
    xy = torch.rand(cap, 2, generator=g) * 300
    boxes = torch.cat([xy, xy + torch.rand(cap, 2, generator=g) * 80 + 1], 1)[None]
    scores = ((torch.rand(cap, generator=g) * 40).round() / 40)[None]
    ids = torch.randint(0, nid, (cap,), generator=g, dtype=torch.int32)[None]
    cnt = torch.tensor([n], dtype=torch.int32)
    cand = (boxes.contiguous(), scores.contiguous(), ids.contiguous(), torch.arange(cap, dtype=torch.int32)[None].contiguous(), cnt)
    out = emu.batched_nms(cand, 1, cap, 0.5, 2000)
    dets, keep = glue.batched_nms(boxes[0, :n], scores[0, :n], ids[0, :n].long(), 0.5)
    k = int(out['count'][0])
    assert k == keep.numel()
    assert torch.equal(out['keep'][0, :k].long(), keep)


def test_emu_msdeform_attn_level_counts(emu):
    import test_gpu_query as t
    t.test_msdeform_attn_level_counts(DEV, [(4, 4), (8, 6)], 128)
    t.test_msdeform_attn_level_counts(DEV, [(3, 3), (4, 6), (8, 8), (16, 12)], 128)
    t.test_msdeform_attn_level_counts(DEV, [(2, 2), (3, 3), (4, 4), (6, 6), (8, 8)], 256)


def test_emu_folded_token_to_image_attention(emu):
    """csrc/t2i_fold.hip (a kernel written and debugged on this emulator before it saw a GPU): both head-count
    instantiations against fp64 and the unfolded kernels, then the whole SAM mask decoder -- token attention, folded
    token -> image attention, the matrix-core image -> token block, ConvTranspose GEMMs with their LayerNorm epilogue, the
    upscale tail -- against the HuggingFace decoder on 16 x 16 embeddings"""
    import test_gpu_baseline_configs as tb
    import test_gpu_kernels as tk
    tk.test_sam_t2i_fold_matches_fp64_attention(DEV, 3, 64, 10)
    tk.test_sam_t2i_fold_matches_fp64_attention(DEV, 2, 64, 3)
    tb.test_anchor_mask_head_with_folded_token_to_image_attention(DEV, 16)


# (module, test function, arguments after `dev`): bodies of the `-m gpu` suite that take about a second each on the emulator
SWEEP = [
    ('test_gpu_kernels', 'test_patchify_preprocess', ()),
    ('test_gpu_kernels', 'test_gemm_conv3x3', (1,)),
    ('test_gpu_kernels', 'test_gemm_conv3x3', (2,)),
    ('test_gpu_kernels', 'test_gemm_rowmaps_and_broadcast_residual', ()),
    ('test_gpu_kernels', 'test_gemm_small_values_precision', ()),
    ('test_gpu_kernels', 'test_gemm_plane_residual', ()),
    ('test_gpu_kernels', 'test_gemm_column_range_outputs', ()),
    ('test_gpu_kernels', 'test_outlier_activations_do_not_poison_the_split', ()),
    ('test_gpu_kernels', 'test_conv_transpose_pool_add_sincos', ()),
    ('test_gpu_kernels', 'test_generic_attention_with_batch_maps', (32, 10, 10, 8)),
    ('test_gpu_kernels', 'test_generic_attention_with_batch_maps', (64, 70, 130, 2)),
    ('test_gpu_kernels', 'test_sam_cross_attention_kernels', (7,)),
    ('test_gpu_kernels', 'test_sam_cross_attention_kernels', (10,)),
    ('test_gpu_kernels', 'test_sam_i2t_fused_matches_composition', (3, 64, False, 'valu')),
    ('test_gpu_kernels', 'test_sam_i2t_fused_matches_composition', (3, 64, False, 'mfma')),
    ('test_gpu_kernels', 'test_sam_i2t_fused_matches_composition', (7, 520, True, 'mfma')),
    ('test_gpu_kernels', 'test_sam_i2t_fused_matches_composition', (10, 600, False, 'mfma')),   # T = 10: the bench's form (5 k-steps)
    ('test_gpu_kernels', 'test_sam_i2t_fused_matches_composition', (10, 1024, True, 'mfma')),
    ('test_gpu_kernels', 'test_gemm_fp8_corrected_product', (14,)),             # v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3)
    ('test_gpu_kernels', 'test_roi_align_matches_oracle', ()),
    ('test_gpu_kernels', 'test_mask_post_matches_reference_formula', ()),
    ('test_gpu_kernels', 'test_hyper_mask', ()),
    ('test_gpu_kernels', 'test_batched_nms_matches_oracle', (5000, 5, 0.7, 1000)),
    ('test_gpu_kernels', 'test_rpn_topk_ties_and_small_levels', ()),
    ('test_gpu_query', 'test_query_kernels_unit', ()),
    ('test_gpu_samdet', 'test_bbox_post_matches_real_bbox_head_with_and_without_rescale', ()),
    ('test_gpu_samdet', 'test_resnet_leaf_kernels', ()),
    ('test_gpu_samdet', 'test_rpn_softmax_objectness_on_the_real_heads_vectors', ()),   # [fg, bg] folded into the packed 1x1 head
    ('test_gpu_samdet', 'test_box_prompt_mask_post_and_scale_boxes', ()),     # box prompts' sin / cos, mask_post_logits
    ('test_gpu_apis', 'test_resize_pad_kernel_matches_cv2_restatement', ()),
    ('test_gpu_kernels', 'test_vit_attention', (14, 2, 80, 3)),               # the fp32-fed attention entry points
    ('test_gpu_kernels', 'test_vit_attention', (32, 1, 80, 2)),               # ... global form (K | V split kernel + DMA ring)
    ('test_gpu_query', 'test_fusion_head_rescale_paths', ()),
    ('test_gpu_samseg', 'test_paste_masks_kernel_matches_reference_vectors', ()),
    ('test_gpu_dist', 'test_pack_masks_matches_numpy', ()),
    ('test_gpu_dist', 'test_mask_rle_matches_coco_restatement', ()),          # byte-equal to the reference's COCO strings
    ('test_gpu_dist', 'test_all_gather_results_single_process_on_device', ()),
]


@pytest.mark.parametrize('mod,fn,args', SWEEP, ids=[f'{f}{list(a) if a else ""}' for _, f, a in SWEEP])
def test_emu_sweep_of_gpu_test_bodies(emu, mod, fn, args):
    """the fp32 / plane GEMM kernels with their loaders and epilogues (row maps, implicit-GEMM convs, ConvTranspose modes,
    plane residuals, column ranges), generic and SAM-decoder attentions, the matrix-core image -> token block, RoIAlign,
    mask post-processing, NMS, GroupNorm / resize / masked attention of the query path, ResNet leaves, mask paste"""
    import importlib
    getattr(importlib.import_module(mod), fn)(DEV, *args)


def test_emu_dma_kernels_with_latest_possible_completion(emu):
    """The DMA engine at its other extreme: LDS is written only when an `s_waitcnt vmcnt(n)` of the issuing wave demands it
    (the default mode writes at issue).  The ring kernels -- persistent GEMM (whose waits count the tile-ticket atomic),
    gemm_f16x3_dma_kernel, window / global attention, the folded attention -- must give the same results: a wait that is
    too weak, or missing in front of the barrier, reads a stale buffer here.  Self-test first: with the waits ignored the
    folded attention must come out wrong."""
    import harness
    import test_gpu_gemm_s2 as tg
    import test_gpu_kernels as tk
    with harness.lazy_dma(ignore_waits=True):
        with pytest.raises(AssertionError):
            tk.test_sam_t2i_fold_matches_fp64_attention(DEV, 3, 64, 10)
    with harness.lazy_dma():
        tg.test_s2_plain_and_residual(DEV, 300, 64, 128)
        tg.test_s2_column_ranges_and_row_maps(DEV, 64, 128, 203)
        tk.test_plane_gemm_tile_variants(DEV, 1)
        tk.test_vit_window_attention_fused_relpos(DEV, 3, 4, 2, 80, 1, 1)
        tk.test_vit_attention_planes(DEV, 32, 2, 64, 2)
        tk.test_vit_attention(DEV, 32, 1, 80, 2)                      # attn_global_kernel's K | V^T ring (fp32-fed entry point)
        tk.test_sam_t2i_fold_matches_fp64_attention(DEV, 3, 64, 10)


def test_emu_fused_upscaler_tail(emu):
    """sam_upscale_fused_kernel (csrc/upscale.hip): ConvTranspose + LayerNorm2d + GELU + ConvTranspose + GELU + hyper-network
    product in one pass over the keys -- written on the emulator at the end of round 4 and not yet run on a GPU (opt-in:
    SamMaskDecoderHIP.upscale_fused).  The whole mask decoder with it against the HuggingFace decoder, and against the
    two-kernel form."""
    from oracle import hf_sam
    from rsprompter_amd.registry import MODELS
    from rsprompter_amd.synth import synth_state_dict
    head = MODELS.build(dict(type='RSPrompterAnchorMaskHead', mask_decoder=dict(type='RSSamMaskDecoder', hf_pretrain_name='sam_vit_base'),
                             in_channels=256, roi_feat_size=14, per_pointset_point=5, with_sincos=True, multimask_output=False,
                             class_agnostic=True))
    sd = synth_state_dict(head, 5)
    head.load_state_dict(sd)
    dec = hf_sam.build_mask_decoder()
    dec.load_state_dict({k[len('mask_decoder.mask_decoder.'):]: v for k, v in sd.items() if k.startswith('mask_decoder.mask_decoder.')})
    g = torch.Generator().manual_seed(2)
    R, B, hw = 3, 2, 12                       # 144 pixels per RoI: tiles of 128 straddle RoIs, the last tile is ragged
    x = torch.randn(R, 256, 14, 14, generator=g)
    emb = torch.randn(B, 256, hw, hw, generator=g)
    ipe = torch.randn(1, 256, hw, hw, generator=g).expand(B, -1, -1, -1).contiguous()
    roi_img = torch.tensor([0, 1, 1])
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    hip = head.mask_decoder.mask_decoder
    low0, _ = head(cl(x), cl(emb), cl(ipe), roi_img)
    hip.upscale_fused = True
    low1, iou1 = head(cl(x), cl(emb), cl(ipe), roi_img)
    import harness
    with harness.lazy_dma():                      # ... and with the W1 ring's DMA completing as late as its waits allow
        low2, _ = head(cl(x), cl(emb), cl(ipe), roi_img)
    assert torch.equal(low1, low2)
    sparse = head.point_embeddings(cl(x))
    with torch.no_grad():
        ref_m, ref_i = dec(image_embeddings=emb[roi_img], image_positional_embeddings=ipe[roi_img],
                           sparse_prompt_embeddings=sparse.unsqueeze(1),
                           dense_prompt_embeddings=sd['no_mask_embed.weight'].reshape(1, -1, 1, 1).expand(R, -1, hw, hw),
                           multimask_output=False)[:2]
    ref_m = ref_m.reshape(R, 1, 4 * hw, 4 * hw)
    e0, e1 = float((low0 - ref_m).abs().max()), float((low1 - ref_m).abs().max())
    print(f'upscaler tail: two kernels vs HF {e0:.2e}, fused vs HF {e1:.2e}, fused vs two kernels {float((low0 - low1).abs().max()):.2e}')
    assert e0 < 1e-4 and e1 < 1e-4


def test_emu_rle_codec_round_trip_property(emu):
    """encode -> decode round trip of the evaluation hand-off: random masks of random sizes -- W a multiple of
    4 (mask_rle4_kernel) or not (the byte-wise kernel), blobs, stripes, empty and full masks, capacities that have to grow --
    through the DEVICE codec (rsp_mask_rle + rsp_rle_to_string on the emulator) must decode, with the oracle's restatement of
    cocoapi's rleFrString / rleDecode, to the mask again, and the string must be the one pycocotools would write."""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=120, deadline=None, derandomize=True)
    @given(st.integers(1, 3), st.integers(1, 40), st.integers(1, 45), st.integers(0, 5), st.integers(0, 2 ** 31 - 1))
    def check(k, h, w, kind, seed):
        kp.check_rle_round_trip(emu, DEV, k, h, w, kind, seed)
    check()


def test_emu_pingpong_gemm_several_tiles_per_block(emu):
    """gemm_f16x3_pp_kernel (csrc/gemm_pp.hip, round 5: one 512-thread block per CU, the two waves of a SIMD alternating
    matrix and load phases): both tiles (256 x 256: hint 200, 128 x 256: hint 201) with ONE and TWO blocks per XCD, so that a
    block walks several tiles -- the next tile's first ring stages are queued from inside the epilogue, whose LDS
    transposition lives in the wave's own DMA slots.  Bit-equal to gemm_f16x3_dma_kernel; also with the DMA completing as late
    as the kernel's s_waitcnt immediates allow."""
    import harness
    import test_gpu_gemm_s2 as t
    ops = emu
    g = torch.Generator().manual_seed(6)

    def run():
        for (M, N, K, kw, name) in [(1100, 768, 256, dict(), 'plain'),
                                    (1100, 768, 128, dict(act=ops.ACT_GELU, out_planes=True, out_f32=False), 'lin1-like'),
                                    (1100, 768, 192, 'res', 'residual'), (900, 768, 128, 'qkv', 'qkv scatter')]:
            a = torch.randn(M, K, generator=g)
            w = torch.randn(N, K, generator=g) / K ** 0.5
            b = torch.randn(N, generator=g)
            pw = ops.PackedWeight(w, b, device=DEV)
            ap = ops.to_planes(a)
            if kw == 'res':
                kw = dict(res=torch.randn(M, N, generator=g))
            if kw == 'qkv':
                perm = torch.randperm(M + 50, generator=g)[:M].to(torch.int32)
                kw = dict(c_rowmap=perm, out_rows=M + 50, out_planes=True, c_ncols=256, pl_col0=256)
            rows = kw['c_rowmap'].long() if 'c_rowmap' in kw else None
            ref = t._flat(ops.gemm(ap, pw, tile_hint=1, **kw))
            for hint in (200 | (1 << 16), 200 | (2 << 16) | (2 << 8), 201 | (1 << 16), 201 | (2 << 16) | (2 << 8)):
                assert ops.gemm(ap, pw, tile_hint=hint, plan_only='pp', **kw) == (128 if hint & 1 else 256)
                assert t._same(ref, t._flat(ops.gemm(ap, pw, tile_hint=hint, **kw)), rows), (name, hint)
    run()
    with harness.lazy_dma():
        run()


def test_emu_gemm_ragged_shapes_property(emu):
    """C = act(A W^T + b) + res for random ragged shapes through whatever kernel the dispatcher picks (fp32 A: the
    register-staged kernel; planes: gemm_f16x3_dma_kernel; hint 40: the persistent kernel) against the fp64 product"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=100, deadline=None, derandomize=True)
    @given(st.integers(1, 300), st.integers(1, 40), st.integers(1, 8), st.sampled_from(['f32', 'planes', 's2']),
           st.booleans(), st.booleans(), st.sampled_from([0, 1, 2]), st.integers(0, 2 ** 31 - 1))
    def check(M, n4, k32, path, with_bias, with_res, act, seed):
        N, K = 4 * n4, 32 * k32
        if path == 's2':
            K = max(K, 64)                                  # rsp_gemm_s2_eligible: K >= 64 (a forced hint on less is EINVAL)
        kp.check_gemm_ragged(emu, DEV, M, N, K, path, with_bias, with_res, act, seed)
    check()


def test_emu_batched_nms_property(emu):
    """greedy NMS with the coordinate-offset trick on random candidate sets -- duplicates, exact score ties, empty sets,
    counts below the capacity, one to several ids -- against the oracle's restatement of mmcv batched_nms: kept indices in
    the same order"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=100, deadline=None, derandomize=True)
    @given(st.integers(0, 400), st.integers(1, 6), st.sampled_from([0.3, 0.5, 0.7]), st.integers(1, 120), st.integers(2, 60),
           st.integers(0, 2 ** 31 - 1))
    def check(n, nid, thr, max_out, levels, seed):
        kp.check_batched_nms(emu, DEV, n, nid, thr, max_out, levels, seed)
    check()


def test_emu_window_attention_grid_property(emu):
    """rsp_vit_window_attention over random window grids: windows per side 1-3, 1-14 real rows / columns in the last window
    of a row / column (the padded queries are skipped, the padded keys masked), 1-3 heads of 64 or 80, both block counts"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=10, deadline=None, derandomize=True)
    @given(st.integers(1, 3), st.integers(1, 14), st.integers(1, 3), st.sampled_from([64, 80]), st.integers(0, 1))
    def check(nw, real, nh, dh, variant):
        kp.check_window_attention_grid(emu, DEV, nw, real, nh, dh, variant)
    check()


def test_emu_layernorm_shapes_property(emu):
    """LayerNorm over random row counts and widths (the four-rows-per-wave kernel for C % 64 == 0 in [256, 1280] with plane
    outputs, the wave-per-row kernel otherwise), fp32 and plane outputs against fp64"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=70, deadline=None, derandomize=True)
    @given(st.integers(1, 130), st.sampled_from([32, 64, 96, 128, 256, 320, 384, 512, 640, 768, 896, 1024, 1152, 1280, 1408]), st.booleans(), st.integers(0, 2 ** 31 - 1))
    def check(rows, C, planes, seed):
        kp.check_layernorm(emu, DEV, rows, C, planes, seed)
    check()


def test_emu_attention_shapes_property(emu):
    """the generic flash attention (token self attention, masked Mask2Former cross attention: rsp_attention) and the fused
    image -> token block over random token / key counts -- ragged last tiles, one key, T below and at the kernels' limits"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=25, deadline=None, derandomize=True)
    @given(st.sampled_from([16, 32, 64]), st.integers(1, 70), st.integers(1, 200), st.integers(1, 8))
    def generic(dh, Tq, Tk, nh):
        kp.check_generic_attention(emu, DEV, dh, Tq, Tk, nh)
    generic()

    @settings(max_examples=16, deadline=None, derandomize=True)
    @given(st.integers(1, 10), st.integers(1, 300), st.booleans(), st.sampled_from(['valu', 'mfma']))
    def i2t(T, N, planes_res, form):
        kp.check_i2t_fused(emu, DEV, T, N, planes_res, form)
    i2t()


def test_emu_rpn_selection_property(emu):
    """rpn_topk -> rpn_decode -> batched NMS (rsp_rpn_topk / _decode / rsp_batched_nms) against the oracle's restatement of
    RPNHead._predict_by_feat_single (pinned on the real class) on random pyramids: logits quantised so that scores TIE (the
    kernels' rule: score descending, position ascending = the reference's stable sort), nms_pre below and above the level
    sizes, the min-size filter on and off, 1-2 images -- (level, anchor) indices must be identical"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=20, deadline=None, derandomize=True)
    @given(st.integers(1, 2), st.integers(2, 12), st.integers(2, 12), st.sampled_from([5, 40, 300, 1000]), st.integers(1, 60),
           st.sampled_from([-1, 0, 8]), st.integers(1, 12), st.integers(0, 2 ** 31 - 1))
    def check(B, h0, w0, nms_pre, max_per_img, min_size, levels_q, seed):
        kp.check_rpn_selection(emu, DEV, B, h0, w0, nms_pre, max_per_img, min_size, levels_q, seed)
    check()


def test_emu_bbox_post_and_query_topk_property(emu):
    """softmax + per-class decode + score threshold + multiclass NMS (rsp_bbox_post, rsp_batched_nms) and the fusion head's
    top-k over (query, class) (rsp_query_topk) on random inputs with DUPLICATED rows (exact score ties: the rule is score
    descending, flat index ascending) against the oracle's restatements of BBoxHead._predict_by_feat_single /
    instance_postprocess: same detections (tie-aware matching, tests/_match.py), same flat indices"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=25, deadline=None, derandomize=True)
    @given(st.integers(1, 120), st.integers(1, 12), st.sampled_from([0.02, 0.05, 0.3]), st.integers(1, 60), st.integers(0, 2 ** 31 - 1))
    def bbox(n, nc, thr, max_out, seed):
        kp.check_bbox_post(emu, DEV, n, nc, thr, max_out, seed)
    bbox()

    @settings(max_examples=25, deadline=None, derandomize=True)
    @given(st.integers(1, 2), st.integers(1, 60), st.integers(1, 10), st.integers(1, 100), st.integers(0, 2 ** 31 - 1))
    def topk(B, Nq, nc, k, seed):
        kp.check_query_topk(emu, DEV, B, Nq, nc, k, seed)
    topk()


def test_emu_sampling_kernels_property(emu):
    """the gather / resample kernels on random geometry against the oracle (the reference's torch calls and the C restatement
    of mmcv RoIAlign): RoIAlign with RoIs that are tiny, huge, partly or wholly outside the image and on every pyramid level;
    MSDeformAttn with 1-5 levels of random sizes and offsets that leave the maps; GroupNorm with add / ReLU; bilinear
    resizing up and down; the query prompter's attention-mask rule incl. fully blocked rows"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=15, deadline=None, derandomize=True)
    @given(st.integers(1, 40), st.sampled_from([7, 14]), st.integers(0, 2 ** 31 - 1))
    def roi(K, P, seed):
        kp.check_roi_align(emu, DEV, K, P, seed)
    roi()

    @settings(max_examples=15, deadline=None, derandomize=True)
    @given(st.integers(1, 5), st.sampled_from([16, 32]), st.integers(0, 2 ** 31 - 1))
    def msda(L, hd, seed):
        kp.check_msdeform_attn(emu, DEV, L, hd, seed)
    msda()

    @settings(max_examples=15, deadline=None, derandomize=True)
    @given(st.integers(1, 3), st.integers(1, 12), st.integers(1, 12), st.integers(1, 20), st.integers(1, 20), st.integers(0, 2 ** 31 - 1))
    def resample(B, h, w, ho, wo, seed):
        kp.check_resample(emu, DEV, B, h, w, ho, wo, seed)
    resample()


def test_emu_decoder_tail_kernels_property(emu):
    """the two opt-in kernels of the SAM decoder's per-RoI passes on random geometry: the folded token -> image attention
    (every variant; 1-12 tokens = both head-count instantiations, key counts of 1-5 tiles) against fp64 and the unfolded
    kernels, and the fused upscaler tail against the two-kernel form for h != w, RoI sizes that are no multiple of the
    128-row tile, and a single RoI smaller than one tile"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=16, deadline=None, derandomize=True)
    @given(st.integers(1, 3), st.sampled_from([32, 64, 96, 160]), st.integers(1, 12))
    def fold(R, N, T):
        kp.check_t2i_fold(emu, DEV, R, N, T)
    fold()

    dec = kp.upscale_decoder(DEV, 3)

    @settings(max_examples=30, deadline=None, derandomize=True)
    @given(st.integers(1, 3), st.integers(1, 13), st.integers(1, 13), st.integers(0, 2 ** 31 - 1))
    def upscaler(R, h, w, seed):
        kp.check_upscaler(emu, DEV, dec, R, h, w, seed)
    upscaler()


def test_emu_query_prompt_kernels_property(emu):
    """SamMaskEmbedding of the query prompter (mask_embed_kernel: two stride-2 convolutions with LayerNorm2d + GELU, a 1x1
    convolution, + the image embedding of the prompt set's image; models.py:305, HF:569-601) and the row gather, on random
    geometry against the reference's torch calls"""
    from hypothesis import given, settings, strategies as st

    @settings(max_examples=12, deadline=None, derandomize=True)
    @given(st.integers(1, 5), st.integers(1, 2), st.integers(1, 10), st.integers(1, 10), st.sampled_from([256, 512]),
           st.integers(0, 2 ** 31 - 1))
    def embed(R, B, he, we, C, seed):
        kp.check_mask_embed(emu, DEV, R, B, he, we, C, seed)
    embed()
    kp.check_mask_embed_refuses_narrow_channels(emu, DEV)

    @settings(max_examples=20, deadline=None, derandomize=True)
    @given(st.integers(1, 50), st.integers(0, 70), st.sampled_from([4, 32, 100, 256]), st.integers(0, 2 ** 31 - 1))
    def gather(n_src, n_idx, C, seed):
        kp.check_gather_rows(emu, DEV, n_src, n_idx, C, seed)
    gather()


def test_emu_first_generation_entry_points(emu):
    """the entry points include/rsp_hip.h keeps for ABI compatibility and rsprompter_amd/ no longer calls: the natural-layout
    split (its own kernel) against its definition, and the forms that forward to their successors (rsp_vit_relpos ->
    _q -> _rows, rsp_vit_attention -> _ex, rsp_msdeform_attn -> _ex) against the successor's result through the wrappers"""
    from rsprompter_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(4)
    x = torch.cat([torch.randn(1000, generator=g) * 3, torch.tensor([0.0, 1e-9, 7e4, -7e4, 65504.0 / 64])])
    hi, lo = torch.empty(x.numel(), dtype=torch.float16), torch.empty(x.numel(), dtype=torch.float16)
    _lib.check(lib.rsp_split_f16(x.data_ptr(), hi.data_ptr(), lo.data_ptr(), x.numel(), 6, 0), 'rsp_split_f16')
    xs = x * 64.0
    want_hi = xs.clamp(-65504.0, 65504.0).to(torch.float16)
    want_lo = (xs - want_hi.float()).clamp(-65504.0, 65504.0).to(torch.float16)
    assert torch.equal(hi, want_hi) and torch.equal(lo, want_lo)
    Bp, S, nh, dh = 2, 14, 2, 64
    qkv = torch.randn(Bp, S * S, 3, nh, dh, generator=g).contiguous()
    rph, rpw = torch.randn(2 * S - 1, dh, generator=g) * 0.2, torch.randn(2 * S - 1, dh, generator=g) * 0.2
    rel = emu.vit_relpos(qkv, rph, rpw, Bp, S, nh, dh)
    rel1 = torch.empty_like(rel)
    _lib.check(lib.rsp_vit_relpos(qkv.data_ptr(), rph.data_ptr(), rpw.data_ptr(), rel1.data_ptr(), Bp, S, nh, dh, 0), 'rsp_vit_relpos')
    assert torch.equal(rel, rel1)
    out = emu.vit_attention(qkv, rel, Bp, S, nh, dh, dh ** -0.5)
    out1 = torch.empty_like(out)
    _lib.check(lib.rsp_vit_attention(qkv.data_ptr(), rel.data_ptr(), out1.data_ptr(), Bp, S, nh, dh, dh ** -0.5, 0), 'rsp_vit_attention')
    assert torch.equal(out, out1)
    shapes = [(3, 4), (6, 5)]
    ntok, B = sum(h * w for h, w in shapes), 2
    value = torch.randn(B * ntok, 128, generator=g)
    ow = torch.randn(B * ntok, 8 * 2 * 4 * 3, generator=g).contiguous()
    ref_pts = torch.rand(ntok, 2, generator=g)
    got = emu.msdeform_attn(value, ow, ref_pts, B, ntok, shapes)
    got1 = torch.empty_like(got)
    import ctypes
    hw = (ctypes.c_int * (2 * len(shapes)))(*[v for s_ in shapes for v in s_])
    _lib.check(lib.rsp_msdeform_attn(value.data_ptr(), ow.data_ptr(), ow.shape[1], ref_pts.data_ptr(), got1.data_ptr(), B, ntok,
                                     len(shapes), hw, 0), 'rsp_msdeform_attn')
    assert torch.equal(got, got1)


def test_emu_tiny_sam_encoder_end_to_end(emu, monkeypatch):
    """The whole SAM ViT encoder path -- patch embedding, a WINDOWED layer (token -> window row maps in the qkv / proj
    epilogues, bias rows of the padded tokens, window attention with rel-pos inside over 3 x 3 partly padded windows) and a
    GLOBAL layer (rel-pos kernel, plane-fed attention, S = 32), LayerNorms emitting planes, GELU + plane MLP, the neck's
    1x1 / 3x3 convolutions with LayerNorm2d -- on the emulator against the HuggingFace SamVisionEncoder: a 2-layer, 128-wide,
    2-head model at 512 x 512 (the geometry of the *-peft-512 configs), every hidden state and the image embedding"""
    from oracle import hf_sam
    from rsprompter_amd import nnutil, sam_encoder
    from rsprompter_amd.synth import synth_state_dict
    tiny = dict(hidden=128, depth=2, heads=2, global_idx=(1,), mlp=256)
    monkeypatch.setitem(nnutil.SAM_ARCH, 'tiny', tiny)
    if getattr(sam_encoder, 'SAM_ARCH', nnutil.SAM_ARCH) is not nnutil.SAM_ARCH:
        monkeypatch.setitem(sam_encoder.SAM_ARCH, 'tiny', tiny)
    monkeypatch.setitem(hf_sam.ARCH, 'tiny', dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                                  global_attn_indexes=[1]))
    enc = sam_encoder.SamVisionEncoderHIP(arch='tiny', image_size=512, output_hidden_states=True)
    sd = synth_state_dict(enc, seed=3)
    enc.load_state_dict(sd)
    o = hf_sam.build_vision_encoder('tiny', mlp_dim=256, image_size=512)
    o.load_state_dict(sd, strict=True)
    x = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(4))
    emb_ref, hs_ref = hf_sam.run_vision_encoder(o, x)
    out = enc(x)
    emb, hs = out[0], out[1]
    assert emb.shape == emb_ref.shape and len(hs) == len(hs_ref) == 3
    errs = [float((h - r).abs().max()) for h, r in zip(hs, hs_ref)]
    e_emb = float((emb - emb_ref).abs().max())
    print('tiny encoder on the emulator: hidden states', ['%.1e' % e for e in errs], 'embedding %.1e (range %.1f)' % (e_emb, float(emb_ref.abs().max())))
    assert max(errs) < 1e-4 and e_emb < 1e-4
    # the opt-in fp8-corrected product (LayerNorm / GELU / attention epilogues emit cat8 planes, the four block
    # GEMMs run fp16 hi.hi + one scaled fp8 MFMA): 16-bit-class arithmetic, so only closeness to the fp16x3 run is asked
    from rsprompter_amd import ops
    monkeypatch.setattr(ops, 'F8_CORR', True)
    enc._packed = None
    out8 = enc(x)
    e8 = [float((h - r).abs().max()) / float(r.abs().max()) for h, r in zip(out8[1], hs)] + [float((out8[0] - emb).abs().max()) / float(emb.abs().max())]
    print('... with the fp8-corrected product: relative distance to the fp16x3 run', ['%.1e' % e for e in e8])
    assert 0 < max(e8) < 2e-3


# ---------------------------------------------------------------------------------------------- prescribed score fields
# tests/_score_fields.py (the bodies of test_score_fields_* in tests/test_gpu_kernel_props.py): each case against the fp64
# restatement within max(F, 2 E32), E32 the error of the same restatement in torch float32
def test_emu_score_fields_window_attention(emu):
    """attn_win_kernel with prescribed logits: every field (staircases around the lazy maximum, straddles of LAZY_LOG2 in
    every tile, ramp, spikes at every tile edge with their known answer, lane-divergent forms, the rel-pos bias path) on a
    grid with padded queries; constant levels far below 0 at kv exponents 0 / 2 / 4 on both grids -- those returned errors
    of 0.2 while the padded keys of the last tile were masked with an absolute -60000 in the raw score domain"""
    import _score_fields as sf
    rep = sf.Report('emu')
    sf.run_window_family(emu, DEV, rep, 'window', [((2, 10), 64, 0)])
    for kv_e in (0, 2, 4):
        sf.check_vit_fields(emu, DEV, rep, 'window', 14, 9, 2, 80, next(sf.chunks(sf.window_level_cases(), 18)), kv_e, (3, 4), 1)
        sf.check_vit_fields(emu, DEV, rep, 'planes', 14, 4, 2, 80, next(sf.chunks(sf.window_level_cases(), 8)), kv_e, (2, 10))
    rep.finish()


def test_emu_score_fields_global_attention(emu):
    """attn_stream_kernel (S = 32, plane-fed) on four fields; the fp32-fed window kernel on the levels"""
    import _score_fields as sf
    rep = sf.Report('emu')
    for n, c in enumerate(sf.chunks(sf.pick(sf.global_cases(1024), sf.EMU_S32_CASES), 2)):
        sf.check_vit_fields(emu, DEV, rep, 'planes', 32, 1, 2, 64, c, seed=n)
    sf.check_vit_fields(emu, DEV, rep, 'f32', 14, 4, 2, 64, next(sf.chunks(sf.window_level_cases(), 8)))
    rep.finish()


def test_emu_score_fields_generic_and_decoder_attention(emu):
    """rsp_attention at ragged last tiles, the SAM decoder's token -> image (plain, with a bias, the field in the bias) and
    image -> token kernels (plain, fused in both forms), the folded token -> image attention under query amplitude and a
    k_proj offset"""
    import _score_fields as sf
    rep = sf.Report('emu')
    for (dh, Tq, Tk, nh) in [(16, 10, 300, 8), (64, 70, 130, 2), (32, 33, 257, 2)]:
        sf.check_generic_fields(emu, DEV, rep, dh, Tq, Tk, nh)
    for where in ('k', 'k+bias', 'bias'):
        sf.check_t2i_fields(emu, DEV, rep, 7, 600, where)
    for T in (7, 10):
        sf.check_i2t_fields(emu, DEV, rep, T, 96)
        for form in ('valu', 'mfma'):
            sf.check_i2t_fused_fields(emu, DEV, rep, T, form, 96)
    for (R, N, T, amp, offset) in [(2, 64, 7, 32.0, 20.0), (2, 96, 10, 8.0, 20.0), (2, 96, 10, 32.0, 0.0)]:
        sf.check_t2i_fold_fields(emu, DEV, rep, R, N, T, amp, offset)
    rep.finish()
