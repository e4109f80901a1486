"""CPU (`-m "not gpu"`): polygon simplification (csrc/ring_simplify.hip, ops.ring_simplify, rle.simplify_polygons,
apis.masks_to_polygons(tolerance=...), large_image polygon_tolerance).

The oracle is tests/_ring_simplify_ref.py, Douglas-Peucker on a closed ring in Python integers with an explicit stack, itself
checked for its properties with fractions; the kernels run lane by lane on the emulator (tests/wave_emu), the sources
unchanged, and must agree exactly in all seven arrays.  The bodies are tests/_ring_simplify_cases.py, the same the device
tier runs."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _ring_simplify_cases as cases  # noqa: E402
import _ring_simplify_ref as sref  # noqa: E402
import _seam_merge_cases as seam_cases  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# --------------------------------------------------------------------------------------------------- the reference itself
def test_reference_holds_its_properties_on_every_case_mask():
    assert cases.check_reference() > 350


def test_reference_known_answers():
    cases.check_known_answers_of_the_reference()


# ------------------------------------------------------------------------------------------------------------ kernels
def test_known_answers(emu):
    cases.check_known_answers(emu, CPU)


def test_every_case_mask_at_every_tolerance_and_area(emu):
    cases.check_case_masks(emu, CPU)


def test_batch_with_empty_rows_and_a_second_launch(emu):
    cases.check_batch(emu, CPU)


def test_no_rings_no_rows_and_every_ring_dropped(emu):
    cases.check_empty_calls(emu, CPU)


def test_ring_lengths_around_every_path_boundary(emu):
    cases.check_lengths(emu, CPU)


def test_spiral_with_a_split_tree_64_levels_deep(emu):
    assert cases.check_deep_spiral(emu, CPU) >= 64


def test_ties_go_to_the_lowest_index(emu):
    assert cases.check_ties(emu, CPU) >= 10


def test_chains_whose_ends_coincide(emu):
    assert cases.check_zero_chords(emu, CPU) >= 1


def test_holes_go_with_their_outer_ring(emu):
    cases.check_dropped_parents(emu, CPU)


def test_ring_across_the_whole_coordinate_range_needs_128_bits(emu):
    assert cases.check_wide_coordinates(emu, CPU) > 2 ** 64


def test_bad_arguments_are_refused(emu):
    cases.check_refusals(emu, CPU, pytest)


# ---------------------------------------------------------------------------------------------------------------- API
def test_masks_to_polygons_forms_with_a_tolerance(emu):
    from rsprompter_amd import apis, rle
    cases.check_api_forms(apis, rle, CPU)


def test_masks_to_polygons_refusals(emu):
    from rsprompter_amd import apis, rle
    cases.check_api_refusals(apis, rle, CPU, pytest)


# ----------------------------------------------------------------------------------------------------------- pipeline
def _scene():
    rng = np.random.default_rng(16)
    return rng.integers(0, 256, (45, 70, 3)).astype(np.uint8)


@pytest.mark.parametrize('mode', ['nms', 'seam_mask'])
def test_inference_large_image_simplified_polygons_around_a_random_stub_detector(emu, mode):
    from rsprompter_amd import large_image as li
    kw = dict(merge_iou_thr=0.25, merge_nms_type=mode)
    if mode == 'seam_mask':
        kw['seam_iou_thr'] = 0.3
    k, before, after = cases.check_pipeline(li, CPU, _scene(), seam_cases.RandomStub((32, 32)), 32, **kw)
    assert k >= 10
    with pytest.raises(ValueError, match="masks='polygons'"):
        li.inference_large_image(seam_cases.RandomStub((32, 32)), _scene(), patch_size=32, polygon_tolerance=1.0, **kw)
    with pytest.raises(ValueError, match='tolerance'):
        li.inference_large_image(seam_cases.RandomStub((32, 32)), _scene(), patch_size=32, masks='polygons',
                                 polygon_tolerance=-1, **kw)


def test_cli_flags_and_the_unchanged_default(emu, tmp_path, monkeypatch):
    """`python -m rsprompter_amd.large_image` (its main(), in process, around the stub detector): without the new flags the
    three formats write what they wrote; with them the rings are the reference's, and `rle` refuses them"""
    from PIL import Image
    from rsprompter_amd import apis
    from rsprompter_amd import large_image as li
    model = seam_cases.RandomStub((32, 32))
    monkeypatch.setattr(apis, 'init_detector', lambda cfg, ckpt, device=None: model)
    Image.fromarray(_scene()).save(tmp_path / 'scene.png')
    src = str(tmp_path / 'scene.png')
    argv = [src, 'cfg.py', 'none', '--patch-size', '32', '--batch-size', '2', '--score-thr', '0.4']
    geo = ['--geo-transform', '100', '0.5', '0', '200', '0', '-0.5']
    exact = li.inference_large_image(model, src, 32, batch_size=2, masks='polygons')
    want = {'rle': json.dumps(li.pred2dict(li.inference_large_image(model, src, 32, batch_size=2), 0.4)),
            'polygons': json.dumps(li.pred2dict(exact, 0.4)),
            'geojson': json.dumps(li.pred2geojson(exact, 0.4, (100.0, 0.5, 0.0, 200.0, 0.0, -0.5)))}
    for i, (fmt, text) in enumerate(want.items()):                   # the defaults: unchanged output
        extra = ([] if fmt == 'rle' and i == 0 else ['--mask-format', fmt]) + (geo if fmt == 'geojson' else [])
        li.main(argv + ['--out-dir', str(tmp_path / fmt)] + extra)
        name = 'scene.geojson' if fmt == 'geojson' else 'scene.json'
        assert os.listdir(tmp_path / fmt) == [name] and (tmp_path / fmt / name).read_text() == text
    import copy
    simple = copy.copy(exact)
    simple.pred_instances = copy.copy(exact.pred_instances)
    simple.pred_instances.masks = sref.simplify_lists(exact.pred_instances.masks, sref.tol2_q8(1.5), 3)
    li.main(argv + ['--out-dir', str(tmp_path / 'p'), '--mask-format', 'polygons', '--simplify-tolerance', '1.5',
                    '--min-ring-area', '3'])
    assert (tmp_path / 'p' / 'scene.json').read_text() == json.dumps(li.pred2dict(simple, 0.4))
    assert (tmp_path / 'p' / 'scene.json').read_text() != want['polygons']
    li.main(argv + ['--out-dir', str(tmp_path / 'g'), '--mask-format', 'geojson', '--simplify-tolerance', '1.5',
                    '--min-ring-area', '3'] + geo)
    assert (tmp_path / 'g' / 'scene.geojson').read_text() == json.dumps(li.pred2geojson(simple, 0.4, (100.0, 0.5, 0.0, 200.0, 0.0, -0.5)))
    for bad in (['--simplify-tolerance', '1'], ['--min-ring-area', '2'], ['--mask-format', 'rle', '--simplify-tolerance', '1'],
                ['--mask-format', 'polygons', '--simplify-tolerance', '-1'],
                ['--mask-format', 'polygons', '--min-ring-area', '-2'], ['--mask-format', 'polygons', '--min-ring-area', '1.5']):
        with pytest.raises(SystemExit):
            li.main(argv + ['--out-dir', str(tmp_path / 'x')] + bad)
