"""CPU (`-m "not gpu"`): shared-border simplification (csrc/ring_coverage.hip, ops.ring_coverage, rle.simplify_coverage,
apis.masks_to_polygons(topology='shared'), large_image polygon_topology).

The oracle is tests/_ring_coverage_ref.py, the sequential definition on a dense label map in Python integers, itself checked
for its properties (twin edges, nodes, distances with fractions, nesting, tolerance 0); the kernels run lane by lane on the
emulator (tests/wave_emu), the sources unchanged, and must agree exactly in all nine arrays.  The bodies are
tests/_ring_coverage_cases.py, the same the device tier runs."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _ring_coverage_cases as cases  # noqa: E402
import _ring_coverage_ref as cref  # noqa: E402
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
def test_reference_holds_its_properties_on_every_case():
    assert cases.check_reference() > 1500


def test_reference_counters_move_on_the_random_maps():
    stats = cases.check_random_stats()
    assert stats['ties_differ'] > 100 and stats['inserted_nodes'] > 100, stats


# ---------------------------------------------------------------------------------------------------- the discriminating test
def test_independent_rings_part_and_shared_ones_do_not(emu):
    from rsprompter_amd import apis, rle
    cases.check_shared_borders_match(apis, rle, CPU)


# ------------------------------------------------------------------------------------------------------------ kernels
def test_every_hand_built_map_at_every_tolerance(emu):
    cases.check_hand_maps(emu, CPU)


def test_closed_arcs_decide_ties_by_the_smallest_point(emu):
    stats = cases.check_closed_arcs(emu, CPU)
    assert stats['ties_differ'] >= 1


def test_closed_arc_with_one_node(emu):
    cases.check_one_node_arc(emu, CPU)


def test_ring_that_collapses_between_two_nodes(emu):
    cases.check_collapse(emu, CPU)


def test_hole_goes_with_its_outer_ring(emu):
    cases.check_hole_loses_parent(emu, CPU)


def test_no_rows_no_pixels_and_every_ring_dropped(emu):
    cases.check_empty_calls(emu, CPU)


def test_noded_lengths_around_every_path_boundary(emu):
    cases.check_lengths(emu, CPU)


def test_wall_of_80_steps_with_four_nodes(emu):
    cases.check_long_wall(emu, CPU)


def test_300_random_label_maps(emu):
    assert cases.check_random(emu, CPU) > 10000


def test_poisoned_buffers_second_launch_and_host_reads(emu):
    from rsprompter_amd import rle
    cases.check_protocol(emu, rle, CPU)


def test_bad_arguments_are_refused(emu):
    from rsprompter_amd import apis, rle
    cases.check_refusals(emu, rle, apis, CPU, pytest)


# ---------------------------------------------------------------------------------------------------------------- API
def test_masks_to_polygons_forms_with_shared_topology(emu):
    from rsprompter_amd import apis, rle
    cases.check_api_forms(apis, rle, CPU)


# ----------------------------------------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize('region', [0, 6])
@pytest.mark.parametrize('mode', ['nms', 'seam_mask'])
def test_inference_large_image_shared_borders_around_a_random_stub_detector(emu, mode, region):
    from rsprompter_amd import large_image as li
    assert cases.check_pipeline(li, CPU, seam_cases.RandomStub((32, 32)), mode, region) >= 10


def test_inference_large_image_refuses_before_the_first_tile(emu):
    from rsprompter_amd import large_image as li
    cases.check_pipeline_refusals(li, seam_cases.RandomStub((32, 32)), pytest)


def test_cli_flag_and_the_unchanged_default(emu, tmp_path, monkeypatch):
    """`python -m rsprompter_amd.large_image` (its main(), in process, around the stub detector): without the flag, and with
    `--simplify-topology rings`, the files are what they were; with `shared` the rings are the reference's"""
    from PIL import Image
    from rsprompter_amd import apis
    from rsprompter_amd import large_image as li
    import _run_flatten_cases as fcases
    model = seam_cases.RandomStub((32, 32))
    monkeypatch.setattr(apis, 'init_detector', lambda cfg, ckpt, device=None: model)
    scene = np.random.default_rng(16).integers(0, 256, (45, 70, 3)).astype(np.uint8)
    Image.fromarray(scene).save(tmp_path / 'scene.png')
    src = str(tmp_path / 'scene.png')
    argv = [src, 'cfg.py', 'none', '--patch-size', '32', '--batch-size', '2', '--score-thr', '0.4', '--flatten']
    geo = ['--geo-transform', '100', '0.5', '0', '200', '0', '-0.5']
    tr = (100.0, 0.5, 0.0, 200.0, 0.0, -0.5)
    kw = dict(batch_size=2, flatten='score')
    alone = li.inference_large_image(model, src, 32, masks='polygons', polygon_tolerance=1.5, **kw)
    want = {'polygons': json.dumps(li.pred2dict(alone, 0.4)), 'geojson': json.dumps(li.pred2geojson(alone, 0.4, tr))}
    for fmt, text in want.items():
        for extra in ([], ['--simplify-topology', 'rings']):
            out = tmp_path / (fmt + str(len(extra)))
            li.main(argv + ['--out-dir', str(out), '--mask-format', fmt, '--simplify-tolerance', '1.5'] + extra
                    + (geo if fmt == 'geojson' else []))
            name = 'scene.geojson' if fmt == 'geojson' else 'scene.json'
            assert os.listdir(out) == [name] and (out / name).read_text() == text
    shared = li.inference_large_image(model, src, 32, masks='polygons', polygon_tolerance=1.5, polygon_topology='shared', **kw)
    flat = li.inference_large_image(model, src, 32, **kw).pred_instances
    L = cref.labels_of(list(fcases._dense_of(flat.masks, 'strings', 45, 70)), 45, 70)
    cases._lists_equal(shared.pred_instances.masks, cref.lists(cases.want_of(None, L, len(flat.scores), 1.5)))
    li.main(argv + ['--out-dir', str(tmp_path / 's'), '--mask-format', 'geojson', '--simplify-tolerance', '1.5',
                    '--simplify-topology', 'shared'] + geo)
    text = (tmp_path / 's' / 'scene.geojson').read_text()
    assert text == json.dumps(li.pred2geojson(shared, 0.4, tr)) and text != want['geojson']
    for bad in (['--mask-format', 'polygons', '--simplify-topology', 'shared'],                          # no tolerance
                ['--mask-format', 'rle', '--simplify-topology', 'shared'],
                ['--mask-format', 'polygons', '--simplify-tolerance', '1', '--min-ring-area', '2', '--simplify-topology', 'shared'],
                ['--mask-format', 'polygons', '--simplify-tolerance', '1', '--simplify-topology', 'arcs']):
        with pytest.raises(SystemExit):
            li.main(argv + ['--out-dir', str(tmp_path / 'x')] + bad)
    with pytest.raises(SystemExit):                                                                      # without --flatten
        li.main(argv[:-1] + ['--out-dir', str(tmp_path / 'x'), '--mask-format', 'polygons', '--simplify-tolerance', '1',
                             '--simplify-topology', 'shared'])
