"""CPU (`-m "not gpu"`): run-domain connected components (csrc/run_components.hip, ops.rle_components, rle.runs_components /
split_runs / clean_runs, apis.remove_small_regions on RLE dicts, apis.masks_to_obb(per_component=True), apis.mask_components,
large_image min_mask_region_area).

The oracle is tests/_run_components_ref.py, a flood fill over the dense mask with its own property checks; the kernels run lane
by lane on the emulator (tests/wave_emu), the sources unchanged, and must agree exactly.  The bodies are
tests/_run_components_cases.py, the same the device tier runs."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _run_components_cases as cases  # noqa: E402
import _run_components_ref as cref  # noqa: E402
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
    """cref.check asserts: the areas sum to the population, every pixel in exactly one component, no two components with
    8-adjacent pixels, stream order, and scipy.ndimage.label's count and sizes where scipy imports"""
    counts = [len(cref.check(m)[1]) for _, m in cases.all_cases() + cases.boundary_masks()]
    assert max(counts) >= cases.THREADS + 1 and counts.count(0) >= 2 and counts.count(1) >= 10


def test_reference_known_answers_and_the_tie_rule():
    for name, m, comps in cases.hand_checked():
        got = cref.check(m)[1]
        assert [(d['area'], d['box'], d['first']) for d in got] == comps, name
    m = np.zeros((7, 5), bool)
    m[5, 0] = m[1, 3] = True
    out, ch, cs = cref.remove_small_regions(m, 2, 'islands')
    assert (ch, cs) == (False, True) and out[1, 3] and not out[5, 0]
    assert cref.pieces(np.array([[0, 1], [1, 1], [1, 0]], bool)) == [(0, 1, 3), (1, 0, 2)]


# ------------------------------------------------------------------------------------------------------------ kernels
def test_hand_checked_answers(emu):
    cases.check_hand_checked(emu, CPU)


def test_every_case_mask_alone(emu):
    cases.check_single_masks(emu, CPU)


def test_one_row_canvases_connect_consecutive_columns_only(emu):
    cases.check_h1_columns(emu, CPU)


def test_piece_counts_around_a_block_and_a_chunk(emu):
    cases.check_block_boundaries(emu, CPU)


def test_batch_with_invalid_rows_and_a_second_launch(emu):
    cases.check_batch(emu, CPU)


def test_components_of_shifted_and_joined_run_tables(emu):
    from rsprompter_amd import rle
    cases.check_shifted_and_joined_tables(emu, rle, CPU)


def test_split_runs_gives_one_row_per_component(emu):
    from rsprompter_amd import rle
    cases.check_split(emu, rle, CPU)


@pytest.mark.parametrize('area', cases.AREAS)
def test_clean_runs_is_remove_small_regions_in_every_mode(emu, area):
    """one min_area over the three modes on the case masks, batched on one canvas with an empty row"""
    from rsprompter_amd import rle
    H, W = 66, 70
    masks = cases.batch_on_canvas(cases.small_cases(), H, W, seed=5) + [None]
    counts, n = seam_cases.rows_from_masks(masks, CPU)
    for mode in cases.MODES:
        want, flags = cases.want_clean(masks, area, mode)
        c, m, n_host, cap, ch = rle.clean_runs(counts, n, (H, W), area, mode)
        cases.assert_table(c, m, want, f'{mode} at {area}')
        assert ch.tolist() == flags and n_host.tolist() == m.tolist() and cap == c.shape[1]


def test_clean_runs_with_an_overlong_and_a_negative_row(emu):
    from rsprompter_amd import rle
    cases.check_clean_modes(emu, rle, CPU, areas=(2, 100))


def test_clean_runs_edge_cases_and_the_retry(emu):
    from rsprompter_amd import rle
    cases.check_clean_edge_cases(emu, rle, CPU)


def test_status_check_and_refusals(emu):
    from rsprompter_amd import rle
    cases.check_status_and_refusals(emu, rle, CPU, pytest)


# ---------------------------------------------------------------------------------------------------------------- API
def test_remove_small_regions_on_rle_dicts(emu):
    from rsprompter_amd import apis, rle
    cases.check_api_remove_small_regions(apis, rle, CPU)
    cases.check_api_refusals(apis, CPU, pytest)


def test_mask_components(emu):
    from rsprompter_amd import apis, rle
    cases.check_api_components(apis, rle, CPU)


def test_masks_to_obb_per_component(emu):
    from rsprompter_amd import apis, rle
    cases.check_api_obb_per_component(apis, rle, CPU)


# ----------------------------------------------------------------------------------------------------------- pipeline
def _scene():
    rng = np.random.default_rng(16)
    return rng.integers(0, 256, (45, 70, 3)).astype(np.uint8)


@pytest.mark.parametrize('mode', ['nms', 'seam_mask'])
def test_inference_large_image_cleans_the_scene_masks_around_a_random_stub_detector(emu, mode):
    from rsprompter_amd import large_image as li
    kw = dict(merge_iou_thr=0.25, merge_nms_type=mode)
    if mode == 'seam_mask':
        kw['seam_iou_thr'] = 0.3
    k, changed = cases.check_pipeline(li, CPU, _scene(), seam_cases.RandomStub((32, 32)), 32,
                                      lambda s: s.pred_instances.masks.numpy(), 6, **kw)
    print(f'{mode}: {k} instances, {changed} changed')


def test_bad_region_areas_and_dense_masks_are_refused_before_the_model_runs(emu):
    from rsprompter_amd import large_image as li

    class Never(seam_cases.RandomStub):
        def test_step(self, data):
            raise AssertionError('the model ran')
    with pytest.raises(ValueError, match='remove_small_regions'):
        li.inference_large_image(Never((32, 32)), _scene(), 32, masks='dense', min_mask_region_area=4)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match='non-negative integer'):
            li.inference_large_image(Never((32, 32)), _scene(), 32, min_mask_region_area=bad)


def test_cli_default_output_is_unchanged_and_the_flag_changes_the_masks(emu, tmp_path, monkeypatch):
    from PIL import Image
    from rsprompter_amd import apis, datasets
    from rsprompter_amd import large_image as li
    import _large_image_ref as lref
    model = seam_cases.RandomStub((32, 32))
    monkeypatch.setattr(apis, 'init_detector', lambda cfg, ckpt, device=None: model)
    Image.fromarray(_scene()).save(tmp_path / 'scene.png')
    src = str(tmp_path / 'scene.png')
    argv = [src, 'cfg.py', 'none', '--patch-size', '32', '--batch-size', '2', '--score-thr', '0.4']
    want = li.pred2dict(li.inference_large_image(model, src, 32, batch_size=2), 0.4)
    assert set(want) == {'labels', 'scores', 'bboxes', 'masks'}
    li.main(argv + ['--out-dir', str(tmp_path / 'a')])
    assert (tmp_path / 'a' / 'scene.json').read_text() == json.dumps(want)
    li.main(argv + ['--out-dir', str(tmp_path / 'b'), '--min-mask-region-area', '6'])
    got = json.loads((tmp_path / 'b' / 'scene.json').read_text())
    assert set(got) == set(want) and {k: got[k] for k in ('labels', 'scores', 'bboxes')} == {k: want[k] for k in ('labels', 'scores', 'bboxes')}
    assert got['masks'] != want['masks'] and len(got['masks']) == len(want['masks']) > 3
    for g, w in zip(got['masks'], want['masks']):
        dense = lref.counts_to_mask(datasets.rle_from_string(w['counts']), 45, 70)
        clean = cref.remove_small_regions(dense, 6, 'both')[0]
        assert (lref.counts_to_mask(datasets.rle_from_string(g['counts']), 45, 70) == clean).all()
    with pytest.raises(SystemExit):
        li.main(argv + ['--out-dir', str(tmp_path / 'c'), '--min-mask-region-area', '-3'])
