"""-m "not gpu": PerSAM one-shot segmentation ("PerSAM") without a GPU.  The new kernels (the biased token ->
image attention, rsp_persam_target, rsp_persam_similarity, rsp_persam_locate) and the decoder with HF's two hooks run on the
lane-level emulator (tests/wave_emu) through the same check functions as the GPU suite (tests/test_gpu_persam.py), at
S = 128 / g = 8 and small images; `PerSam`'s host flow runs around a stub of `SamModelHIP` on a constructed scene."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import test_gpu_persam as pt  # noqa: E402  (the same checks the GPU runs)

CPU = torch.device('cpu')
S, G = 128, 8


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_feature_is_there():
    """fails on the parent: the entry points, their prototypes, the API, and the hook call that used to raise"""
    from rsprompter_amd import _lib, apis, ops, sam_decoder
    names = ('rsp_sam_t2i_attention_bias', 'rsp_persam_target', 'rsp_persam_similarity', 'rsp_persam_locate',
             'rsp_persam_locate_workspace_bytes')
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'rsp_hip.h')).read()
    for n in names:
        assert n in _lib.PROTOTYPES and f' {n}(' in hdr, n
    lib = _lib.load()
    assert lib.rsp_persam_locate(None, 1, 8, 8, 32, 32, 32, 32, 16, 16, 2, None, 0, None, None, None, None) == -1
    assert lib.rsp_sam_t2i_attention_bias(None, None, None, None, 1, None, 1, 7, 64, 0.25, None) == -1
    assert lib.rsp_persam_locate_workspace_bytes(2, 1024, 1024) > 0 and lib.rsp_persam_locate_workspace_bytes(1, 0, 4) == -1
    assert callable(apis.PerSam) and callable(ops.sam_t2i_attention_bias) and callable(ops.persam_locate)
    import inspect
    assert {'attention_similarity', 'target_embedding'} <= set(inspect.signature(apis.SamSession.predict).parameters)
    # the accepted forms pass the argument check, every other shape keeps raising (no device needed for either)
    N, T = 4096, 7
    bias, te = sam_decoder.persam_hooks(torch.zeros(1, 1, 1, N), torch.zeros(1, 1, 256), 2, 3, N, T)
    assert tuple(bias.shape) == (1, N) and tuple(te.shape) == (1, 256)
    bias, te = sam_decoder.persam_hooks(torch.zeros(6, 1, 1, N), torch.zeros(2, 1, 1, 256), 2, 3, N, T)
    assert tuple(bias.shape) == (6, N) and tuple(te.shape) == (6, 256)
    for bad in (dict(a=torch.zeros(1)), dict(a=torch.zeros(1, 8, 1, N)), dict(a=torch.zeros(1, 1, T, N)), dict(t=torch.zeros(1, 1, T, 256)),
                dict(t=torch.zeros(255))):
        with pytest.raises(NotImplementedError, match='accepted forms'):
            sam_decoder.persam_hooks(bad.get('a'), bad.get('t'), 2, 3, N, T)
    with pytest.raises(NotImplementedError, match='accepted forms'):
        sam_decoder.persam_hooks(torch.zeros(1, 1, 1, N), None, 2, 3, N, 13)


def _small_models():
    """HF SamModel with a two-layer encoder at image_size 128 (embedding grid 8) and SamModelHIP('base', image_size=128) holding
    its prompt encoder, positional matrix and mask decoder (seeded); the encoders are not run here"""
    from transformers.models.sam.configuration_sam import SamConfig
    from oracle import hf_sam
    from rsprompter_amd.samdet import SamModelHIP
    from rsprompter_amd.synth import synth_state_dict
    cfg = SamConfig(vision_config=dict(hidden_size=64, num_hidden_layers=1, num_attention_heads=2, global_attn_indexes=[0],
                                       image_size=S, mlp_dim=128, window_size=4),
                    prompt_encoder_config=dict(image_size=S, image_embedding_size=G))
    for c in (cfg, cfg.vision_config, cfg.mask_decoder_config, cfg.prompt_encoder_config):
        c._attn_implementation = 'eager'
    hf = hf_sam.hf.SamModel(cfg).eval()
    hf.load_state_dict(synth_state_dict(hf, seed=0))
    hip = SamModelHIP('base', image_size=S)
    sd = {k: v for k, v in hf.state_dict().items() if not k.startswith('vision_encoder.')}
    res = hip.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith('vision_encoder.') for k in res.missing_keys)
    return hf, hip.eval()


def test_hooks_against_hf_on_the_emulator(emu):
    hf, hip = _small_models()
    pt.check_hooks(hf, hip, CPU, G, S)
    pt.check_hooks_that_keep_raising(hip, CPU, G, S)


def test_biased_t2i_kernel_on_the_emulator(emu):
    for T in (7, 10, 12):
        pt.check_bias_kernel(emu, CPU, T, N=200 if T != 10 else 331)


def test_target_and_similarity_on_the_emulator(emu):
    pt.check_target_and_similarity(emu, CPU, S, G, (60, 90))
    pt.check_target_and_similarity(emu, CPU, S, G, (52, 80), B=2, seed=82)


EMU_LOCATE = (((128, 128), (128, 128), (128, 128)),                     # strip form
              ((128, 128), (85, 128), (60, 90)), ((128, 128), (83, 128), (52, 80)),             # generic form
              ((128, 128), (128, 127), (128, 127)))                     # identity with an odd width


@pytest.mark.parametrize('case', range(len(EMU_LOCATE)))
def test_locate_kernel_on_the_emulator(emu, case):
    img, crop, out = EMU_LOCATE[case]
    pt.check_locate(emu, CPU, 1, img, crop, out, G, 32, seed=90 + case)
    pt.check_locate(emu, CPU, 5, img, crop, out, G, 32, seed=95 + case)
    pt.check_locate(emu, CPU, 3, img, crop, out, G, 32, kind='plateau', seed=99)
    pt.check_locate(emu, CPU, 2, img, crop, out, G, 32, kind='constant')
    if case == 0:
        pt.check_locate_refusals(emu, CPU)


def test_host_flow_around_a_stub_on_the_emulator(emu):
    pt.check_host_flow(emu, CPU, S, G, ((60, 90), (50, 70)), 1)


def test_procedure_against_hf_on_the_emulator(emu):
    """`PerSam.segment` with the live decoder (hooks, mask and box prompts, best of three) on the emulator against the
    composition of HF calls; the encoder on both sides is HF's small one on the CPU, so the similarity bound is E_SIM alone.
    Smooth random images, one reference, three targets of two sizes."""
    from rsprompter_amd.apis import PerSam
    hf, hip = _small_models()
    hip.get_image_embeddings = lambda pv: hf.get_image_embeddings(pv).detach()
    ref = pt._test_image((60, 90), seed=7)
    ref_mask = torch.zeros(60, 90, dtype=torch.bool)
    ref_mask[15:45, 30:70] = True
    ps = PerSam(hip, ref, ref_mask)
    assert ps.cells > 1
    imgs = [pt._test_image((60, 90), seed=33), pt._test_image((52, 80), seed=35), pt._test_image((60, 90), seed=34)]
    with torch.no_grad():
        res, st = pt.check_procedure(ps, hf, emu, CPU, S, G, ref, imgs, pt.E_SIM, count_reads=False)
    assert [tuple(r['mask'].shape) for r in res] == [(60, 90), (52, 80), (60, 90)]
