"""CPU (`-m "not gpu"`): oriented boxes (csrc/mask_obb.hip, ops.mask_hull / ops.hull_min_rect, rle.runs_to_obb,
apis.masks_to_obb, large_image oriented_boxes=True).

The oracle is tests/_mask_obb_ref.py, the sequential definition in Python integers and fractions with its own property checks;
the kernels run lane by lane on the emulator (tests/wave_emu), the sources unchanged, and must agree exactly.  The bodies are
tests/_mask_obb_cases.py, the same the device tier runs."""
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _mask_obb_cases as cases  # noqa: E402
import _mask_obb_ref as oref  # noqa: E402
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
    """oref.check asserts: every pixel corner on or inside the hull, strict convexity, area2 >= 2 popcount, the rectangle
    around every hull vertex, no larger than the axis-aligned box, no rectangle flush with another edge smaller"""
    sizes = []
    for name, m in cases.all_cases() + cases.boundary_masks() + [('quarter disc 100', cases.quarter_disc_with_spike(100))]:
        ring, a2, edge, q = cases.want_of(name, m)
        sizes.append(len(ring))
        assert (edge == -1) == (not m.any())
    assert max(sizes) >= 40 and sizes.count(0) >= 3


def test_reference_known_answers_and_float_forms():
    for name, m, hull, edge, q, area in cases.known_answers():
        ring, a2, e, qq = oref.obb(m)
        assert (ring, e) == (hull, edge) and (q is None or qq == q) and oref.rect_area(qq, qq[0] ** 2 + qq[1] ** 2) == area, name
    q = (4, 4, 0, 40, -4, 4)                                   # five diagonal pixels: a 5 sqrt 2 x sqrt 2 box at 45 degrees
    assert oref.corners(q) == [[Fraction(1, 2), Fraction(-1, 2)], [Fraction(11, 2), Fraction(9, 2)], [Fraction(9, 2), Fraction(11, 2)],
                               [Fraction(-1, 2), Fraction(1, 2)]]
    cx, cy, w, h, a = oref.xywha(q)
    assert (cx, cy) == (2.5, 2.5) and abs(w - 5 * 2 ** 0.5) < 1e-14 and abs(h - 2 ** 0.5) < 1e-14 and abs(a - np.pi / 4) < 1e-15
    assert oref.xywha((1, 0, 0, 3, 0, 3)) == (1.5, 1.5, 3.0, 3.0, 0.0)                       # U == V: w along e
    assert oref.xywha((3, 0, 21, 30, 15, 120))[2:] == (35.0, 3.0, -np.pi / 2)               # V > U: w along nrm
    assert oref.obb(np.zeros((3, 3), bool)) == ([], 0, -1, (0,) * 6)


# ------------------------------------------------------------------------------------------------------------ kernels
def test_known_answers(emu):
    cases.check_known_answers(emu, CPU)


def test_every_case_mask_alone(emu):
    cases.check_single_masks(emu, CPU)


def test_ties_go_to_the_lowest_edge(emu):
    cases.check_ties(emu, CPU)


def test_column_counts_around_every_path_boundary(emu):
    rounds = cases.check_path_boundaries(emu, CPU)
    print({k: v for k, v in rounds.items()})
    assert max(max(r) for r, _ in rounds.values()) >= 3


def test_quarter_disc_with_a_spike_prunes_slowly_and_correctly(emu):
    """a strictly convex arc next to one far outlier loses one point a round.  On the lattice the first round leaves the arc's
    own hull vertices only (a quarter circle of radius 100 has about 100^(2/3) ~ 20 of them), so the rounds are about that
    many, not 100: correct, not fast"""
    rounds = cases.check_slow_pruning(emu, CPU, 100)
    print('pruning rounds (upper, lower):', rounds)
    assert rounds[0] >= 8 and rounds[1] <= 2


def test_wide_coordinates_compare_beyond_64_bits(emu):
    cases.check_wide_coordinates(emu, CPU)


def test_batch_with_invalid_rows_and_a_second_launch(emu):
    got, want = cases.check_batch(emu, CPU)
    assert sum(1 for w in want if not w[0]) >= 5 and int(got[0].shape[0]) > 300


def test_no_rows_and_no_pixels(emu):
    cases.check_no_rows_and_no_pixels(emu, CPU)


def test_hull_min_rect_on_hand_made_polygons(emu):
    cases.check_hull_min_rect(emu, CPU)


def test_bad_arguments_are_refused(emu):
    cases.check_refuses_bad_arguments(emu, CPU, pytest)


def test_boxes_of_shifted_and_joined_run_tables(emu):
    """the tables rsp_rle_shift and rsp_rle_union write are input as well: tile hull + offset, the box of a union"""
    from rsprompter_amd import rle
    rng = np.random.default_rng(2)
    tiles = [rng.random((9, 8)) < d for d in (0.3, 0.6, 1.0, 0.0)]
    counts, n = seam_cases.rows_from_masks(tiles, CPU)
    offs = torch.tensor([[3, 2], [0, 0], [12, 11], [5, 5]], dtype=torch.int32)
    H, W = 20, 20
    sc, sn, _, _ = rle.shift_runs(counts, n, offs, (9, 8), (H, W))
    placed = [cases.pcases.embed(m, H, W, o[0], o[1]) for m, o in zip(tiles, offs.tolist())]
    cases.assert_arrays_equal(rle.runs_to_obb(sc, sn, (H, W)), cases.flatten([oref.check(m) for m in placed]), 'shifted')
    uc, un, _, _ = rle.union_runs(sc, sn, (H, W), torch.tensor([0, 2, 4], dtype=torch.int32), torch.arange(4, dtype=torch.int32))
    cases.assert_arrays_equal(rle.runs_to_obb(uc, un, (H, W)),
                              cases.flatten([oref.check(placed[0] | placed[1]), oref.check(placed[2] | placed[3])]), 'union')


# ---------------------------------------------------------------------------------------------------------------- API
def test_masks_to_obb_forms(emu):
    from rsprompter_amd import apis, rle
    cases.check_api_forms(apis, rle, CPU)


def test_masks_to_obb_refusals(emu):
    from rsprompter_amd import apis, rle
    cases.check_api_refusals(apis, rle, CPU, pytest)


# ----------------------------------------------------------------------------------------------------------- pipeline
def _scene():
    rng = np.random.default_rng(16)
    return rng.integers(0, 256, (45, 70, 3)).astype(np.uint8)


@pytest.mark.parametrize('mode', ['nms', 'seam_mask'])
def test_inference_large_image_oriented_boxes_around_a_random_stub_detector(emu, mode):
    from rsprompter_amd import large_image as li
    kw = dict(merge_iou_thr=0.25, merge_nms_type=mode)
    if mode == 'seam_mask':
        kw['seam_iou_thr'] = 0.3
    k = cases.check_pipeline(li, _scene(), seam_cases.RandomStub((32, 32)), 32, lambda s: s.pred_instances.masks.numpy(), **kw)
    assert k >= 10


def test_dense_masks_with_oriented_boxes_are_refused_before_the_model_runs(emu):
    from rsprompter_amd import large_image as li

    class Never(seam_cases.RandomStub):
        def test_step(self, data):
            raise AssertionError('the model ran')
    with pytest.raises(ValueError, match='oriented_boxes'):
        li.inference_large_image(Never((32, 32)), _scene(), 32, masks='dense', oriented_boxes=True)


def test_cli_default_output_is_unchanged_and_the_obb_key_with_the_flag(emu, tmp_path, monkeypatch):
    from PIL import Image
    from rsprompter_amd import apis
    from rsprompter_amd import large_image as li
    model = seam_cases.RandomStub((32, 32))
    monkeypatch.setattr(apis, 'init_detector', lambda cfg, ckpt, device=None: model)
    Image.fromarray(_scene()).save(tmp_path / 'scene.png')
    src = str(tmp_path / 'scene.png')
    argv = [src, 'cfg.py', 'none', '--patch-size', '32', '--batch-size', '2', '--score-thr', '0.4']
    want = li.pred2dict(li.inference_large_image(model, src, 32, batch_size=2), 0.4)
    assert set(want) == {'labels', 'scores', 'bboxes', 'masks'}
    li.main(argv + ['--out-dir', str(tmp_path / 'a')])
    assert (tmp_path / 'a' / 'scene.json').read_text() == json.dumps(want)
    li.main(argv + ['--out-dir', str(tmp_path / 'b'), '--oriented-boxes'])
    got = json.loads((tmp_path / 'b' / 'scene.json').read_text())
    assert {k: got[k] for k in want} == want and set(got) == set(want) | {'obb'} and len(got['obb']) == len(want['labels']) > 3
    from rsprompter_amd import datasets
    import _large_image_ref as lref
    dense = [lref.counts_to_mask(datasets.rle_from_string(r['counts']), 45, 70) for r in want['masks']]
    wc, _ = cases.want_floats([oref.obb(m) for m in dense])
    assert cases.close(np.asarray(got['obb'], np.float64), wc)
    li.main(argv + ['--out-dir', str(tmp_path / 'c'), '--oriented-boxes', '--mask-format', 'geojson'])
    fc = json.loads((tmp_path / 'c' / 'scene.geojson').read_text())
    assert cases.close(np.asarray([f['properties']['obb'] for f in fc['features']], np.float64), wc)
