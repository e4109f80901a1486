"""-m gpu: run-domain morphology and Boundary IoU on the device (csrc/run_morphology.hip, ops.rle_erode / rle_boundary,
rle.*_runs, apis.mask_morphology / mask_boundary / boundary_iou, CocoMetric(metric='boundary'), evaluate(boundary=...);
DESIGN §14.13).  The case bodies are tests/_run_morphology_cases.py, the same the emulator tier runs, against the dense
numpy oracle of tests/_run_morphology_ref.py and the subclassed COCOeval; the scene set is scene-sized here.  Everything is
==."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cocoeval_ref as ref  # noqa: E402
import _coco_iou_runs_cases as cic  # noqa: E402
import _run_morphology_cases as cases  # noqa: E402
from test_gpu_coco_iou_runs import LARGE_IMAGE, SCENE_HW, _cfg_dict, _scene_annotations, model  # noqa: E402,F401


# -------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.quick
def test_hand_checked_masks(dev):
    from rsprompter_amd import ops
    cases.check_hand_checked(ops, dev)


@pytest.mark.quick
def test_every_digit_pattern_of_the_window(dev):
    from rsprompter_amd import ops
    cases.check_digit_patterns(ops, dev)


@pytest.mark.quick
def test_list_and_wave_boundaries(dev):
    from rsprompter_amd import ops
    cases.check_list_boundaries(ops, dev)


@pytest.mark.quick
def test_non_canonical_counts(dev):
    from rsprompter_amd import ops
    cases.check_non_canonical(ops, dev)


def test_300_seeded_random_masks_every_operation_every_form(dev):
    from rsprompter_amd import apis, ops
    cases.check_random(ops, apis, dev)


@pytest.mark.quick
def test_protocol_capacities_reads_and_second_launch(dev):
    from rsprompter_amd import ops, rle
    cases.check_protocol(ops, rle, dev)


@pytest.mark.quick
def test_refusals(dev):
    from rsprompter_amd import ops, rle
    cases.check_refusals(ops, rle, dev, pytest)


# ------------------------------------------------------------------------------------------------------------ API + metric
def test_boundary_iou_300_pairs_crowds_forms_and_refusals(dev):
    from rsprompter_amd import apis
    cases.check_boundary_iou(apis, dev, pytest)


def test_coco_metric_boundary_on_the_nwpu_subset(dev, tmp_path):
    from rsprompter_amd import evaluation
    cases.check_metric_nwpu(evaluation, dev, tmp_path, pytest)


def test_coco_metric_boundary_on_two_scenes(dev, tmp_path):
    from rsprompter_amd import apis, evaluation
    cases.check_metric_scenes(evaluation, apis, dev, tmp_path, [(1536, 2048), (2000, 1200)])


# ---------------------------------------------------------------------------------------------------------------- evaluate
def test_evaluate_large_image_with_boundary_equals_the_oracle(dev, model, tmp_path):  # noqa: F811
    """evaluate(large_image=..., boundary=True) once on the committed scene: the run route, the three metrics, the boundary
    stats of the subclassed oracle on the written result files (the weights are synthetic and the detections noise)"""
    from rsprompter_amd import evaluate as E
    from rsprompter_amd.config import Config
    ref.use_numpy_forms()
    d = _cfg_dict(_scene_annotations(tmp_path / 'scenes.json'))
    prefix = str(tmp_path / 'runs' / 'r')
    res = E.evaluate(model, Config(d), out_prefix=prefix, verbose=False, large_image=LARGE_IMAGE, boundary=True,
                     dilation_ratio=0.01)
    m = E.evaluate.last_metric
    assert m.metrics == ['bbox', 'segm', 'boundary'] and m.dilation_ratio == 0.01
    assert m.iou_domain == 'runs' == m.timings['boundary']['iou_domain']
    assert [k for k in res if 'boundary' in k][0] == 'coco/boundary_mAP'
    segm = json.load(open(f'{prefix}.segm.json'))
    assert len(segm) > 0 and all(s['segmentation']['size'] == list(SCENE_HW) for s in segm)
    saved = ref.rle_iou
    ref.rle_iou = cic.LITERAL_IOU
    try:
        want, _ = cases.boundary_oracle(m, prefix, 0.01)
    finally:
        ref.rle_iou = saved
    got = m.eval_results['boundary'].stats
    assert np.array_equal(got, want), (got, want)
    assert got[0] <= m.eval_results['segm'].stats[0]
    with pytest.raises(SystemExit):
        E.main(['cfg.py', 'none', '--dilation-ratio', '0.05'])
