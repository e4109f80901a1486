"""CPU (`-m "not gpu"`): polygon rasterisation (csrc/poly_raster.hip, ops.poly_raster, rle.polygons_to_runs,
datasets.anns_to_rle, apis.polygons_to_masks, CocoMetric(gt_raster='device'), large_image --from-geojson).

The oracle is tests/_cocoeval_ref.py, the literal restatement of cocoapi's maskApi.c; the kernels run lane by lane on the
emulator (tests/wave_emu), the sources unchanged, and must give the oracle's counts exactly.  The bodies are
tests/_poly_raster_cases.py, the same the device tier runs; the host logic (input forms, the inverse transform) is tested
here as well."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _cocoeval_ref as ref  # noqa: E402
import _poly_raster_cases as cases  # noqa: E402
import _seam_merge_cases as seam_cases  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# -------------------------------------------------------------------------------------------------------------- kernels
def test_hand_checked_answers(emu):
    cases.check_hand_checked(emu, CPU)


def test_committed_nwpu_annotations_in_one_batched_call(emu):
    from rsprompter_amd import datasets
    cases.check_nwpu_annotations(emu, datasets, CPU)


def test_2000_seeded_random_polygons(emu):
    cases.check_random_polygons(emu, CPU)


def test_degenerate_rings(emu):
    cases.check_degenerate(emu, CPU)


def test_the_tail_rule(emu):
    cases.check_tail_rule(emu, CPU)


def test_launch_geometry(emu):
    cases.check_launch_geometry(emu, CPU)


def test_capacity_protocol(emu):
    cases.check_capacity(emu, CPU)


def test_limits_are_refused(emu):
    cases.check_limits(emu, CPU, pytest)


# ------------------------------------------------------------------------------------------------------------ host + API
def test_fill_rules_and_the_input_forms(emu):
    from rsprompter_amd import apis, datasets, rle
    cases.check_fill_rules(rle, apis, datasets, CPU, pytest)
    cases.check_api_refusals(apis, CPU, pytest)


def test_round_trip_of_every_small_mask_through_rings_and_geojson(emu):
    from rsprompter_amd import apis, rle
    cases.check_round_trip(apis, rle, CPU)


def test_round_trip_of_a_batch_on_one_canvas(emu):
    from rsprompter_amd import apis, rle
    rng = np.random.default_rng(11)
    masks = np.stack([rng.random((37, 41)) < d for d in (0.0, 0.1, 0.5, 0.9, 1.0)])
    rings, verts = cases.check_round_trip_batch(apis, rle, CPU, masks, 'five noise masks')
    assert rings > 100 and verts > 1000


def test_inverse_transform_is_exact_for_power_of_two_scales_and_refuses_singular_ones():
    from rsprompter_amd import apis
    xy = np.array([[0.0, 0.0], [8191.0, 9000.0], [3.0, 7.0]])
    a, b, c, d, e, f = cases.GEO
    world = np.stack([a + b * xy[:, 0] + c * xy[:, 1], d + e * xy[:, 0] + f * xy[:, 1]], 1)
    assert np.array_equal(apis.invert_transform(cases.GEO)(world), xy)
    rot = (10.0, 0.0, 2.0, -4.0, -2.0, 0.0)                        # a quarter turn with a scale of two
    world = np.stack([rot[0] + rot[1] * xy[:, 0] + rot[2] * xy[:, 1], rot[3] + rot[4] * xy[:, 0] + rot[5] * xy[:, 1]], 1)
    assert np.array_equal(apis.invert_transform(rot)(world), xy)
    for bad in ((0, 0, 0, 0, 0, 0), (1, 2, 4, 1, 1, 2), (0, float('nan'), 0, 0, 0, 1)):
        with pytest.raises(ValueError, match='singular'):
            apis.invert_transform(bad)


def test_instance_forms_are_told_apart_on_the_host():
    from rsprompter_amd import apis
    sq = np.array([[1, 1], [3, 1], [3, 3], [1, 3]], np.int32)
    closed = [[1, 1], [3, 1], [3, 3], [1, 3], [1, 1]]
    forms = [
        ([[1, 1, 3, 1, 3, 3, 1, 3]], 'union', 1), ([1, 1, 3, 1, 3, 3, 1, 3], 'union', 1), ([[1, 1, 2, 2]], 'union', 1),
        (dict(polygons=[[1, 1, 3, 1, 3, 3, 1, 3]], holes_dropped=False), 'union', 1),
        ([(sq, -1, 8)], 'evenodd', 1), ([(sq, -1, 8), (sq, 0, -8)], 'evenodd', 2),
        (dict(type='Polygon', coordinates=[closed, closed]), 'evenodd', 2),
        (dict(type='MultiPolygon', coordinates=[[closed], [closed, closed]]), 'evenodd', 3),
        (dict(type='MultiPolygon', coordinates=[]), 'evenodd', 0), ([], 'union', 0),
    ]
    for inst, fill, count in forms:
        rings, default = apis._instance_rings(inst)
        assert default == fill and len(rings) == count, inst
        assert all(r.dtype == np.float64 and r.shape == (4, 2) for r in rings), inst
    assert apis._instance_rings([[1, 1, 2, 2]])[0][0].tolist() == [[1, 1], [1, 3], [3, 3], [3, 1]]      # rleFrBbox's order
    assert apis._instance_rings([[1, 1, 3, 1, 3, 3, 9]])[0][0].shape == (3, 2)                           # an odd tail is dropped


def test_the_host_restatement_agrees_with_the_oracle_on_the_random_polygons():
    """datasets.rle_from_poly (what gt_raster='host' runs) against tests/_cocoeval_ref.py on a slice of the seeded polygons"""
    from rsprompter_amd import datasets
    rings, sizes, want = cases.random_polygons()
    for r, (h, w), c in list(zip(rings, sizes, want))[:300]:
        assert datasets.rle_from_poly(r.reshape(-1).tolist(), h, w) == c


# ------------------------------------------------------------------------------------------------------------ CocoMetric
def test_coco_metric_gt_raster_device_gives_the_host_strings_and_stats(emu):
    from rsprompter_amd import datasets, evaluation
    ref.use_numpy_forms()
    cases.check_coco_metric_parity(evaluation, datasets, CPU)


def test_evaluate_cli_takes_gt_raster():
    import inspect
    from rsprompter_amd import evaluate as E
    assert inspect.signature(E.evaluate).parameters['gt_raster'].default is None
    with pytest.raises(SystemExit):
        E.main(['cfg.py', 'none', '--gt-raster', 'gpu'])


# ------------------------------------------------------------------------------------------------------------------ CLI
def test_cli_from_geojson_reverses_mask_format_geojson(emu, tmp_path, monkeypatch):
    from PIL import Image
    from rsprompter_amd import apis
    from rsprompter_amd import large_image as li
    scene = np.random.default_rng(16).integers(0, 256, (45, 70, 3)).astype(np.uint8)
    Image.fromarray(scene).save(tmp_path / 'scene.png')
    k = cases.check_cli(li, apis, CPU, tmp_path, monkeypatch, seam_cases.RandomStub((32, 32)), str(tmp_path / 'scene.png'),
                        ['--patch-size', '32', '--batch-size', '2', '--score-thr', '0.4'])
    print(f'{k} instances')
