"""CPU (`-m "not gpu"`): run-domain morphology and Boundary IoU (csrc/run_morphology.hip, ops.rle_erode / rle_boundary,
rle.*_runs, apis.mask_morphology / mask_boundary / boundary_iou, CocoMetric(metric='boundary'), evaluate(boundary=...);
DESIGN §14.13).

The kernels run lane by lane on the emulator (tests/wave_emu), the sources unchanged; the oracle is
tests/_run_morphology_ref.py (dense numpy: the literal 3 x 3 minimum and scipy.ndimage, which must agree).  The bodies are
tests/_run_morphology_cases.py, the same the device tier runs.  Everything is ==."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _run_morphology_cases as cases  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# -------------------------------------------------------------------------------------------------------------- kernels
def test_the_two_forms_of_the_oracle_agree():
    cases.check_oracle()


def test_hand_checked_masks(emu):
    cases.check_hand_checked(emu, CPU)


def test_every_digit_pattern_of_the_window(emu):
    cases.check_digit_patterns(emu, CPU)


def test_list_and_wave_boundaries(emu):
    cases.check_list_boundaries(emu, CPU)


def test_non_canonical_counts(emu):
    cases.check_non_canonical(emu, CPU)


def test_300_seeded_random_masks_every_operation_every_form(emu):
    from rsprompter_amd import apis
    cases.check_random(emu, apis, CPU)


def test_protocol_capacities_reads_and_second_launch(emu):
    from rsprompter_amd import rle
    cases.check_protocol(emu, rle, CPU)


def test_refusals(emu):
    from rsprompter_amd import rle
    cases.check_refusals(emu, rle, CPU, pytest)


# ------------------------------------------------------------------------------------------------------------ API + metric
def test_boundary_iou_300_pairs_crowds_forms_and_refusals(emu):
    from rsprompter_amd import apis
    cases.check_boundary_iou(apis, CPU, pytest)


def test_coco_metric_boundary_on_the_nwpu_subset(emu, tmp_path):
    from rsprompter_amd import evaluation
    cases.check_metric_nwpu(evaluation, CPU, tmp_path, pytest)


def test_coco_metric_boundary_on_a_synthetic_scene_set(emu, tmp_path):
    from rsprompter_amd import apis, evaluation
    cases.check_metric_scenes(evaluation, apis, CPU, tmp_path, [(256, 192), (200, 240)])


# ---------------------------------------------------------------------------------------------------------------- evaluate
def test_evaluate_takes_boundary_and_dilation_ratio():
    import inspect
    from rsprompter_amd import evaluate as E
    sig = inspect.signature(E.evaluate).parameters
    assert sig['boundary'].default is False and sig['dilation_ratio'].default is None
    with pytest.raises(ValueError, match='dilation_ratio'):
        E.evaluate(None, {}, dilation_ratio=0.05)                                    # refused without boundary=True
    with pytest.raises(SystemExit):
        E.main(['cfg.py', 'none', '--dilation-ratio', '0.05'])                       # refused without --boundary
    assert E.LARGE_IMAGE_KEYS == ('patch_size', 'patch_overlap_ratio', 'merge_iou_thr', 'merge_nms_type', 'seam_iou_thr',
                                  'batch_size', 'min_mask_region_area')
