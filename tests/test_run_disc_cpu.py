"""CPU (`-m "not gpu"`): Euclidean buffers in the run domain (csrc/run_disc.hip, ops.rle_dilate_disc / rle_erode_disc /
rle_minus, rle.half_heights / *_runs(element=...) / buffer_runs, apis.mask_morphology(element=...) / buffer_masks,
inference_large_image(buffer=...)).

The kernels run lane by lane on the emulator (tests/wave_emu), the sources unchanged; the oracle is tests/_run_disc_ref.py
(dense numpy: scipy's footprint morphology and the thresholded integer distance transform, which must agree).  The bodies
are tests/_run_disc_cases.py, the same the device tier runs.  Everything is ==."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _run_disc_cases as cases  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# -------------------------------------------------------------------------------------------------------------- kernels
def test_the_two_forms_of_the_oracle_agree_and_the_half_heights_are_the_footprint():
    from rsprompter_amd import rle
    cases.check_oracle(rle)


def test_hand_checked_masks(emu):
    cases.check_hand_checked(emu, CPU)


def test_the_pruning_comb_checkerboard_staircase_notch_and_edges(emu):
    cases.check_pruning(emu, CPU)


def test_list_and_wave_boundaries(emu):
    cases.check_list_boundaries(emu, CPU)


def test_non_canonical_counts(emu):
    cases.check_non_canonical(emu, CPU)


def test_diamond(emu):
    from rsprompter_amd import apis, rle
    cases.check_diamond(emu, rle, apis, CPU)


def test_240_seeded_random_masks_every_operation_every_form(emu):
    from rsprompter_amd import apis
    cases.check_random(emu, apis, CPU)


def test_buffer_masks(emu):
    from rsprompter_amd import apis
    cases.check_buffer_masks(apis, CPU)


def test_protocol_capacities_reads_chunks_and_second_launch(emu, monkeypatch):
    from rsprompter_amd import rle
    cases.check_protocol(emu, rle, CPU, monkeypatch)


def test_refusals(emu):
    from rsprompter_amd import apis, rle
    cases.check_refusals(emu, rle, apis, CPU, pytest)


# ---------------------------------------------------------------------------------------------------------- large_image
def test_large_image_signature_and_refusals_before_the_first_tile():
    from rsprompter_amd import evaluate as E
    from rsprompter_amd import large_image as li
    cases.check_large_image_refusals(li, pytest)
    assert 'buffer' not in E.LARGE_IMAGE_KEYS


@pytest.mark.parametrize('merge', ['nms', 'seam_mask'])
def test_inference_large_image_buffer_around_a_random_stub_detector(emu, merge):
    from rsprompter_amd import large_image as li
    assert cases.check_pipeline(li, CPU, cases.mcases.seam_cases.RandomStub((32, 32)), merge) >= 10
