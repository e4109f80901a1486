"""CPU (`-m "not gpu"`): planar instance layers (csrc/run_flatten.hip, ops.rle_flatten / rle_label_map, rle.flatten_runs /
runs_to_labels, apis.flatten_masks / masks_to_label_map).

The kernels run lane by lane on the emulator (tests/wave_emu), the sources unchanged; the oracle is tests/_run_flatten_ref.py
(dense numpy: the definition and a restatement of panoptic_postprocess' loop, which must agree).  The bodies are
tests/_run_flatten_cases.py, the same the device tier runs.  Everything is ==."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _run_flatten_cases as cases  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_two_forms_of_the_oracle_agree():
    cases.check_oracle()


def test_hand_checked_masks(emu):
    from rsprompter_amd import rle
    cases.check_hand_checked(emu, rle, CPU)


def test_tied_scores_and_the_area_order(emu):
    from rsprompter_amd import apis
    cases.check_tied_scores(apis, CPU)


def test_wave_and_chunk_boundaries(emu):
    cases.check_wave_boundaries(emu, CPU)


def test_non_canonical_counts(emu):
    cases.check_non_canonical(emu, CPU)


def test_300_seeded_random_cases_every_input_and_output_form(emu):
    from rsprompter_amd import apis
    cases.check_random(apis, CPU)


def test_protocol_poison_capacity_retry_reads_and_second_launch(emu):
    from rsprompter_amd import rle
    cases.check_protocol(emu, rle, CPU)


def test_refusals(emu, monkeypatch):
    from rsprompter_amd import apis, rle
    cases.check_refusals(emu, rle, apis, CPU, pytest, monkeypatch)


@pytest.mark.parametrize('merge', ['nms', 'seam_mask'])
@pytest.mark.parametrize('region', [0, 6])
def test_inference_large_image_flatten_around_a_random_stub_detector(emu, merge, region):
    from rsprompter_amd import large_image as li
    assert cases.check_pipeline(li, CPU, cases.seam_cases.RandomStub((32, 32)), merge, region) >= 10


def test_inference_large_image_takes_flatten_and_refuses_it_early():
    import inspect
    from rsprompter_amd import large_image
    sig = inspect.signature(large_image.inference_large_image).parameters
    assert sig['flatten'].default is False and sig['flatten_min_ratio'].default == 0.0
    for bad in ('size', True, 1):
        with pytest.raises(ValueError, match='flatten must be'):
            large_image.inference_large_image(None, None, flatten=bad)
    with pytest.raises(ValueError, match='min_ratio'):
        large_image.inference_large_image(None, None, flatten='score', flatten_min_ratio=1.5)
    with pytest.raises(ValueError, match='flatten_min_ratio applies'):
        large_image.inference_large_image(None, None, flatten_min_ratio=0.5)
    with pytest.raises(ValueError, match='scene run table'):                         # before the first tile runs: no model
        large_image.inference_large_image(None, None, masks='dense', flatten='area')
    with pytest.raises(SystemExit):
        large_image.main(['img', 'cfg.py', 'none', '--flatten', 'size'])
    with pytest.raises(SystemExit):
        large_image.main(['img', 'cfg.py', 'none', '--flatten-min-ratio', '0.5'])   # refused without --flatten
