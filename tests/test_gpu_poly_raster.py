"""-m gpu: polygon rasterisation on the device (csrc/poly_raster.hip, ops.poly_raster, rle.polygons_to_runs,
datasets.anns_to_rle, apis.polygons_to_masks, CocoMetric(gt_raster='device'), large_image --from-geojson).
The case bodies are tests/_poly_raster_cases.py, the same the emulator tier runs, against the restatement of cocoapi's
maskApi.c (tests/_cocoeval_ref.py); the round trip at scale needs no oracle: the rings of a run table, rasterised again, are
the run table.  Everything is exact."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cocoeval_ref as ref  # noqa: E402
import _poly_raster_cases as cases  # noqa: E402
import _seam_merge_cases as seam_cases  # noqa: E402


def test_hand_checked_answers(dev):
    from rsprompter_amd import ops
    cases.check_hand_checked(ops, dev)


def test_committed_nwpu_annotations_in_one_batched_call(dev):
    from rsprompter_amd import datasets, ops
    cases.check_nwpu_annotations(ops, datasets, dev)


def test_2000_seeded_random_polygons(dev):
    from rsprompter_amd import ops
    cases.check_random_polygons(ops, dev)


def test_degenerate_rings(dev):
    from rsprompter_amd import ops
    cases.check_degenerate(ops, dev)


def test_the_tail_rule(dev):
    from rsprompter_amd import ops
    cases.check_tail_rule(ops, dev)


def test_launch_geometry(dev):
    from rsprompter_amd import ops
    cases.check_launch_geometry(ops, dev)


def test_capacity_protocol(dev):
    from rsprompter_amd import ops
    cases.check_capacity(ops, dev)


def test_limits_are_refused(dev):
    from rsprompter_amd import ops
    cases.check_limits(ops, dev, pytest)


def test_fill_rules_and_the_input_forms(dev):
    from rsprompter_amd import apis, datasets, rle
    cases.check_fill_rules(rle, apis, datasets, dev, pytest)
    cases.check_api_refusals(apis, dev, pytest)


def test_round_trip_of_every_small_mask_through_rings_and_geojson(dev):
    from rsprompter_amd import apis, rle
    cases.check_round_trip(apis, rle, dev)


def test_round_trip_of_eight_1024_masks_of_50000_runs(dev):
    """the eight masks of tests/test_gpu_mask_polygons.py (uniform noise smoothed at sigma = 1, cut at its 95th or 5th
    percentile): about 55 000 runs, 10 000 rings and 200 000 vertices a mask -> rings -> the same run table"""
    from scipy import ndimage
    from rsprompter_amd import apis, rle
    rng = np.random.default_rng(1024)
    masks = []
    for i in range(8):
        f = ndimage.gaussian_filter(rng.random((1024, 1024)), 1.0)
        masks.append(f > np.quantile(f, 0.95 if i % 2 == 0 else 0.05))
    rings, verts = cases.check_round_trip_batch(apis, rle, dev, np.stack(masks), 'eight 1024 x 1024 masks')
    print(f'{rings} rings, {verts} vertices')
    assert rings > 40000 and verts > 400000


def test_coco_metric_gt_raster_device_gives_the_host_strings_and_stats(dev):
    from rsprompter_amd import datasets, evaluation
    ref.use_numpy_forms()
    cases.check_coco_metric_parity(evaluation, datasets, dev)


def test_cli_from_geojson_reverses_mask_format_geojson(dev, tmp_path, monkeypatch):
    from PIL import Image
    from rsprompter_amd import apis
    from rsprompter_amd import large_image as li
    scene = np.random.default_rng(16).integers(0, 256, (45, 70, 3)).astype(np.uint8)
    Image.fromarray(scene).save(tmp_path / 'scene.png')
    k = cases.check_cli(li, apis, dev, tmp_path, monkeypatch, seam_cases.RandomStub((32, 32)).to(dev), str(tmp_path / 'scene.png'),
                        ['--patch-size', '32', '--batch-size', '2', '--score-thr', '0.4'])
    print(f'{k} instances')
