"""CPU (`-m "not gpu"`): SAM-HQ.  The fused mask-branch kernel (csrc/sam_hq.hip) and the whole `SamHQMaskDecoderHIP` run
lane by lane on the emulator (tests/wave_emu) against fp64 torch and transformers' `SamHQMaskDecoder`; the host logic
(state-dict round trip with HF, argument validation of the C entry point, PerSam's refusal, checkpoint reading) runs as is."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _sam_hq_ref as ref


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ with _Float16 vector support for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


@pytest.mark.parametrize('g', [4, 8])
def test_emu_hq_mask_kernel_against_fp64(emu, g):
    """g = 4: one 16 x 16 tile, every pixel's 3 x 3 windows touch the zero padding; g = 8: four tiles with interior halos.
    R = 3 prompt sets over 2 images: the hq_features row map.  (The tile is 16 x 16 and g % 4 == 0: no ragged tile exists;
    the kernel has no LDS-DMA ring, so there is no lazy-DMA mode to run.)"""
    c = ref.kernel_case(3, 2, g, seed=g)
    want = ref.kernel_ref_fp64(c)
    got = ref.kernel_run(emu, c, 'cpu')
    err = float((got.double() - want).abs().max())
    print(f'rsp_sam_hq_mask on the emulator, g = {g}: max |err| {err:.2e} on logits up to {float(want.abs().max()):.1f}')
    assert got.shape == want.shape and err < ref.TOL


@pytest.mark.parametrize('multimask,hq_only', [(False, False), (False, True), (True, False), (True, True)])
def test_emu_hq_decoder_against_hf(emu, multimask, hq_only):
    """the whole SamHQMaskDecoderHIP at g = 8, B = 2 images x 2 prompt sets of two point tokens, against HF's decoder"""
    from rsprompter_amd.sam_decoder import SamHQMaskDecoderHIP
    dec, sd = ref.hf_decoder()
    hip = SamHQMaskDecoderHIP()
    hip.load_state_dict(sd, strict=True)
    emb, pe, sparse, dense, inter = ref.decoder_case(2, 2, 2, 8, seed=0)
    want_m, want_i = ref.hf_decode(dec, emb, pe, sparse, dense, inter, multimask, hq_only)
    got_m, got_i, _ = hip(emb, pe, sparse, dense, multimask_output=multimask, hq_token_only=hq_only,
                          intermediate_embeddings=[inter])
    em, ei = float((got_m - want_m).abs().max()), float((got_i - want_i).abs().max())
    print(f'HQ decoder on the emulator (multimask {multimask}, hq_token_only {hq_only}): masks {em:.2e} (|logit| up to '
          f'{float(want_m.abs().max()):.1f}), iou {ei:.2e}, smallest sorted-IoU gap {ref.min_sorted_gap(want_i):.4f}')
    assert ref.min_sorted_gap(want_i) > ref.MIN_GAP                    # the order compared below is well defined
    assert got_m.shape == want_m.shape and got_i.shape == want_i.shape
    assert em < ref.TOL and ei < ref.TOL


def test_emu_hq_sort_ties_go_to_the_lower_token(emu):
    """an IoU head that answers the same value for every token: the order must stay 1, 2, 3 (HF's torch.sort is not stable
    by contract; this decoder's is)"""
    from rsprompter_amd.sam_decoder import SamHQMaskDecoderHIP
    _, sd = ref.hf_decoder()
    sd = dict(sd)
    sd['iou_prediction_head.proj_out.weight'] = torch.zeros_like(sd['iou_prediction_head.proj_out.weight'])
    sd['iou_prediction_head.proj_out.bias'] = torch.full_like(sd['iou_prediction_head.proj_out.bias'], 0.5)
    hip = SamHQMaskDecoderHIP()
    hip.load_state_dict(sd, strict=True)
    hip.keep_stages = True
    emb, pe, sparse, dense, inter = ref.decoder_case(1, 2, 1, 4, seed=3)
    m, i, _ = hip(emb, pe, sparse, dense, multimask_output=True, hq_token_only=False, intermediate_embeddings=[inter])
    assert torch.equal(i, torch.full((1, 2, 3), 0.5))
    st = hip._last_stages
    for j in range(3):
        assert torch.equal(st['hyper'][j], hip._hyper(st['tokens'], 1 + j))


def test_state_dict_round_trip_with_hf():
    from rsprompter_amd.samdet import SamHQModelHIP
    model, sd = ref.hf_model()
    hip = SamHQModelHIP('base')
    hip.load_state_dict(sd, strict=True)
    back = hip.state_dict()
    assert set(back) == set(sd)
    model.load_state_dict(back, strict=True)
    for k in ('mask_decoder.hq_token.weight', 'mask_decoder.mask_conv1.weight', 'mask_decoder.compress_vit_conv1.weight',
              'mask_decoder.hq_mask_mlp.proj_out.bias'):
        assert torch.equal(back[k], sd[k])
    assert hip.mask_decoder.n_output_tokens == 6 and hip.mask_decoder.iou_prediction_head.proj_out.weight.shape[0] == 4


def test_checkpoint_reader_takes_hf_files(tmp_path):
    """HF `.bin` (and safetensors where the package is installed) of the HQ decoder through the package's reader"""
    from rsprompter_amd.checkpoint import load_checkpoint_into
    from rsprompter_amd.sam_decoder import SamHQMaskDecoderHIP
    _, sd = ref.hf_decoder()
    paths = [str(tmp_path / 'pytorch_model.bin')]
    torch.save(sd, paths[0])
    try:
        from safetensors.torch import save_file
        paths.append(str(tmp_path / 'model.safetensors'))
        save_file({k: v.contiguous() for k, v in sd.items()}, paths[1])
    except ImportError:
        pass
    for path in paths:
        hip = SamHQMaskDecoderHIP()
        load_checkpoint_into(hip, path, strict=True)
        got = hip.state_dict()
        assert all(torch.equal(got[k], v) for k, v in sd.items()), path


def test_entry_point_validates_its_arguments_without_a_gpu():
    from rsprompter_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(R=1, g=4, up_rows=64, null=None, n_up=1, up_map=p, n_sam=0, sam=(None, None)):
        ptrs = [p] * 16
        if null is not None:
            ptrs[null] = None
        (up_hi, up_lo, w2_hi, w2_lo, bias2, w1_hi, w1_lo, bias1, gamma, beta, wf, biasf, hyper, feat, fmap, out) = ptrs
        return lib.rsp_sam_hq_mask(up_hi, up_lo, up_rows, 0, up_map, n_up, w2_hi, w2_lo, 0, bias2, w1_hi, w1_lo, 0, bias1, gamma,
                                   beta, 1e-6, wf, biasf, hyper, feat, fmap, 1, out, sam[0], sam[1], n_sam, R, g, None)
    for i in range(16):
        assert call(null=i) == -1, i
    assert call(g=6, up_rows=144) == -1 and call(g=0) == -1 and call(R=0) == -1
    assert call(R=32768, g=64, up_rows=32768 * 128 * 128) == -1          # R (4g)^2 = 2^31
    assert call(g=4, up_rows=63) == -1                                   # fewer plane rows than n_up (2g)^2
    assert call(R=2, up_map=None) == -1                                  # no map: one block of `up` per prompt set
    assert call(n_sam=1) == -1 and call(n_sam=4, sam=(p, p)) == -1 and call(n_sam=-1) == -1


def test_persam_refuses_an_hq_model():
    import numpy as np
    from rsprompter_amd.sam_prompts import PerSam
    from rsprompter_amd.samdet import SamHQModelHIP
    with pytest.raises(NotImplementedError, match='HQ'):
        PerSam(SamHQModelHIP('base'), np.zeros((32, 32, 3), np.uint8), np.ones((32, 32), np.uint8))


def test_hq_token_only_needs_an_hq_model():
    from rsprompter_amd.sam_prompts import SamMaskGenerator
    from rsprompter_amd.samdet import SamModelHIP
    with pytest.raises(ValueError, match='SamHQModelHIP'):
        SamMaskGenerator(SamModelHIP('base'), hq_token_only=True)


def test_emu_positional_terms_follow_the_table(emu):
    """the decoder caches `pe @ W^T + b` per positional table: a table changed in place, or another table that the allocator
    places at the address of a freed one, must not get the terms of the old values (the cache keeps its table alive and keys
    on its version)"""
    from rsprompter_amd.sam_decoder import SamHQMaskDecoderHIP
    dec, sd = ref.hf_decoder()
    hip = SamHQMaskDecoderHIP()
    hip.load_state_dict(sd, strict=True)
    emb, pe, sparse, dense, inter = ref.decoder_case(1, 2, 1, 4, seed=5)
    for step in range(2):
        want_m, want_i = ref.hf_decode(dec, emb, pe, sparse, dense, inter, False, False)
        got_m, got_i, _ = hip(emb, pe, sparse, dense, multimask_output=False, hq_token_only=False, intermediate_embeddings=[inter])
        assert float((got_m - want_m).abs().max()) < ref.TOL and float((got_i - want_i).abs().max()) < ref.TOL, step
        (entry,) = hip._pe_cache.values()
        assert tuple(entry['_table'].shape) == (16, 256)         # the table the terms belong to stays alive with them
        pe.mul_(-0.5)                                   # same memory, other values


def test_emu_hq_model_with_input_masks(emu):
    """`SamHQModelHIP.forward(image_embeddings=, intermediate_embeddings=, input_masks=)` at the model's 64 x 64 grid against
    `SamHQModel`: the dense-prompt path (rsp_sam_mask_embed -> one dense source per image) with hq_features formed from the
    image embedding WITHOUT the dense prompt and the upscaled embedding from their sum (about a minute on the emulator)"""
    from rsprompter_amd.samdet import SamHQModelHIP
    hf, _ = ref.hf_model()
    hip = SamHQModelHIP('base')
    hip.load_state_dict(hf.state_dict(), strict=True)
    g = torch.Generator().manual_seed(0)
    E = torch.randn(1, 256, 64, 64, generator=g)
    inter = [torch.randn(1, 64, 64, 768, generator=g)]
    pts = torch.tensor([[[[300.0, 200.0]], [[800.0, 500.0]]]])
    prev = (torch.randn(256, 256, generator=g) * 3).reshape(1, 1, 256, 256)
    kw = dict(input_points=pts, multimask_output=True, hq_token_only=False)
    with torch.no_grad():
        want = hf(image_embeddings=E, intermediate_embeddings=inter, input_labels=torch.ones(1, 2, 1, dtype=torch.int64),
                  input_masks=prev, **kw)
        base = hf(image_embeddings=E, intermediate_embeddings=inter, input_labels=torch.ones(1, 2, 1, dtype=torch.int64), **kw)
    got = hip(image_embeddings=E.contiguous(memory_format=torch.channels_last), intermediate_embeddings=inter, input_masks=prev, **kw)
    em = float((got.pred_masks - want.pred_masks).abs().max())
    ei = float((got.iou_scores - want.iou_scores).abs().max())
    moved = float((want.pred_masks - base.pred_masks).abs().max())
    print(f'input_masks on the emulator: pred_masks err {em:.2e} (|logit| up to {float(want.pred_masks.abs().max()):.1f}), '
          f'iou_scores err {ei:.2e}; the dense prompt moves the masks by up to {moved:.2f}')
    assert got.pred_masks.shape == want.pred_masks.shape and em < ref.TOL and ei < ref.TOL
    assert moved > 100 * ref.TOL
