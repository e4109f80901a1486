"""-m "not gpu": PerSAM-F ("PerSAM-F") without a GPU.  The fused loss / gradient kernel and the on-device fit run
on the lane-level emulator (tests/wave_emu) through the same check functions as the GPU suite (tests/test_gpu_persam_f.py), at
S = 128 / g = 8, base 32 and small images; `PerSamF`'s host flow runs around a stub of `SamModelHIP`, its procedure with the
live small decoder against the composition of HF calls."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import test_gpu_persam_f as pf  # noqa: E402  (the same checks the GPU runs)
from test_persam_cpu import EMU_LOCATE, G, S, _small_models  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_feature_is_there():
    """fails on the parent: the entry points, their prototypes, their refusals (nothing is launched) and the API"""
    import inspect
    from rsprompter_amd import _lib, apis, ops
    names = ('rsp_persam_f_loss_grad', 'rsp_persam_f_fit', 'rsp_persam_f_workspace_bytes')
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'rsp_hip.h')).read()
    for n in names:
        assert n in _lib.PROTOTYPES and f' {n}(' in hdr, n
    pf.check_refusals(_lib.load())
    assert callable(ops.persam_f_loss_grad) and callable(ops.persam_f_fit)
    assert issubclass(apis.PerSamF, apis.PerSam)
    sig = inspect.signature(apis.PerSamF.__init__).parameters
    assert list(sig)[1:] == ['sam', 'ref_image', 'ref_mask', 'epochs', 'lr'] and sig['epochs'].default == 1000 and sig['lr'].default == 1e-3
    seg = inspect.signature(apis.PerSamF.segment).parameters
    assert seg['batch_size'].default == 8 and seg['output'].default == 'rle' and 'cascade' not in seg


def test_refusals_on_the_emulator(emu):
    import harness
    pf.check_refusals(harness.load_emu(), CPU)


@pytest.mark.parametrize('case', range(len(EMU_LOCATE)))
def test_loss_and_gradient_on_the_emulator(emu, case):
    img, crop, out = EMU_LOCATE[case]
    pf.check_loss_grad(emu, CPU, img, crop, out, 32, seed=120 + 10 * case)


@pytest.mark.parametrize('case', (1, 0))
def test_fit_on_the_emulator(emu, case):
    """40 epochs at (60, 90) (generic form) and (128, 128) (strip form)"""
    img, crop, out = EMU_LOCATE[case]
    pf.check_fit(emu, CPU, img, crop, out, 32, 40, seed=130 + case, count_reads=False)


def test_host_flow_around_a_stub_on_the_emulator(emu):
    pf.check_host_flow_f(emu, CPU, S, G, ((60, 90), (50, 70)), 1)


def test_procedure_against_hf_on_the_emulator(emu):
    """`PerSamF` with the live decoder on the emulator against `oracle_persam_f`; the encoder on both sides is HF's small one on
    the CPU, so the similarity bound is E_SIM alone.  Smooth random images, one reference, three targets of two sizes, 40 epochs."""
    from rsprompter_amd.apis import PerSamF
    hf, hip = _small_models()
    hip.get_image_embeddings = lambda pv: hf.get_image_embeddings(pv).detach()
    ref = pf._test_image((60, 90), seed=7)
    ref_mask = torch.zeros(60, 90, dtype=torch.bool)
    ref_mask[15:45, 30:70] = True
    ps = PerSamF(hip, ref, ref_mask, epochs=40)
    assert ps.cells > 1
    imgs = [pf._test_image((60, 90), seed=33), pf._test_image((52, 80), seed=35), pf._test_image((60, 90), seed=34)]
    with torch.no_grad():
        res, st, _ = pf.check_procedure_f(ps, hf, emu, CPU, S, G, ref, ref_mask, imgs, pf.E_SIM, 40, count_reads=False)
    assert [tuple(r['mask'].shape) for r in res] == [(60, 90), (52, 80), (60, 90)]
