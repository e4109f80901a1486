"""-m gpu: shared-border simplification on the device (csrc/ring_coverage.hip, ops.ring_coverage, rle.simplify_coverage,
apis.masks_to_polygons(topology='shared'), inference_large_image(polygon_topology=...)).  The case bodies are
tests/_ring_coverage_cases.py, the same the emulator tier runs, against the sequential reference of
tests/_ring_coverage_ref.py; the 600-row scene is checked for its properties.  Everything is ==."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ring_coverage_cases as cases  # noqa: E402
import _ring_simplify_ref as sref  # noqa: E402


@pytest.mark.quick
def test_independent_rings_part_and_shared_ones_do_not(dev):
    from rsprompter_amd import apis, rle
    cases.check_shared_borders_match(apis, rle, dev)


@pytest.mark.quick
def test_every_hand_built_map_at_every_tolerance(dev):
    from rsprompter_amd import ops
    cases.check_hand_maps(ops, dev)


@pytest.mark.quick
def test_closed_arcs_one_node_arcs_collapse_and_lost_parents(dev):
    from rsprompter_amd import ops
    assert cases.check_closed_arcs(ops, dev)['ties_differ'] >= 1
    cases.check_one_node_arc(ops, dev)
    cases.check_collapse(ops, dev)
    cases.check_hole_loses_parent(ops, dev)
    cases.check_empty_calls(ops, dev)


@pytest.mark.quick
def test_noded_lengths_around_every_path_boundary_and_the_long_wall(dev):
    from rsprompter_amd import ops
    cases.check_lengths(ops, dev)
    cases.check_long_wall(ops, dev)


@pytest.mark.quick
def test_300_random_label_maps(dev):
    from rsprompter_amd import ops
    assert cases.check_random(ops, dev) > 10000


@pytest.mark.quick
def test_poisoned_buffers_second_launch_and_host_reads(dev):
    from rsprompter_amd import ops, rle
    cases.check_protocol(ops, rle, dev)


@pytest.mark.quick
def test_refusals(dev):
    from rsprompter_amd import apis, ops, rle
    cases.check_refusals(ops, rle, apis, dev, pytest)


@pytest.mark.quick
def test_masks_to_polygons_forms_with_shared_topology(dev):
    from rsprompter_amd import apis, rle
    cases.check_api_forms(apis, rle, dev)


@pytest.mark.quick
@pytest.mark.parametrize('merge', ['nms', 'seam_mask'])
@pytest.mark.parametrize('region', [0, 6])
def test_inference_large_image_shared_borders_around_a_random_stub_detector(dev, merge, region):
    from rsprompter_amd import large_image as li
    assert cases.check_pipeline(li, dev, cases.seam_cases.RandomStub((32, 32)).to(dev), merge, region) >= 10


# ---------------------------------------------------------------------------------------------------------------- scale
def test_voronoi_map_of_40_instances_on_256_x_256(dev):
    """40 Voronoi regions with 15 % of the pixels relabelled: about 15 000 rings (the noise makes nearly every vertex a node, so
    the arcs are short and one round decides them), against the sequential reference"""
    from rsprompter_amd import ops
    L = cases.voronoi(256, 256, 40, 40)
    want = cases.check(ops, dev, 'voronoi 256', L, 40, tolerances=(0, 1, 2))
    assert len(want[8]) > 10000 and len(want[2]) > 2000
    assert cases.twins_unmatched(want, cases.cref.lost_instances(cases.noded_of('voronoi 256', L, 40)[0][5], want)) == 0
    smooth = cases.voronoi(256, 256, 40, 41, noise=0.0)                   # the same regions without noise: long staircase arcs
    want = cases.check(ops, dev, 'voronoi 256 smooth', smooth, 40, tolerances=(0.5, 2), variants=(0, 3))
    assert cases.twins_unmatched(want) == 0 and len(want[6]) == 40
    assert int(cases.want_of('voronoi 256 smooth', smooth, 40, 0.5)[8].max()) >= 10      # split trees ten levels deep


def test_flattened_600_row_scene_keeps_its_borders_shared(dev):
    """the flattened 8 192 x 9 000 scene of 600 rows at tolerance 1: properties only"""
    from rsprompter_amd import ops, rle
    counts, n, size = cases.scene_600(rle, dev)
    exact = ops.ring_coverage(counts, n, *size, 0)
    got = ops.ring_coverage(counts, n, *size, sref.tol2_q8(1))
    labels = rle.runs_to_labels(counts, n, size)
    V2, twins, nodes = cases.check_scene_properties(got, exact, labels, 600)
    print(f'{exact[0].shape[0]} noded vertices, {V2} kept, {twins} twin edges, {nodes} node visits kept, '
          f'{exact[2].shape[0] - got[2].shape[0]} rings dropped')
    assert twins > 0 and nodes > 100
    again = ops.ring_coverage(counts, n, *size, sref.tol2_q8(1))
    assert all(torch.equal(a, b) for a, b in zip(got, again))
