"""CPU (`-m "not gpu"`): run-domain mask IoU (csrc/coco_iou_runs.hip, ops.run_prefix / ops.coco_iou_runs,
CocoMetric(iou_domain=...), apis.mask_iou, evaluate(large_image=...)).

The kernels run lane by lane on the emulator (tests/wave_emu), the sources unchanged; the oracle is tests/_cocoeval_ref.py,
cocoapi's rleIou loop by loop.  The bodies are tests/_coco_iou_runs_cases.py, the same the device tier runs; the host logic
(the route choice, the rank bookkeeping of evaluate, the input forms of mask_iou) is tested here as well.  Everything is ==."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _coco_iou_runs_cases as cases  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# -------------------------------------------------------------------------------------------------------------- kernels
def test_hand_checked_pairs(emu):
    cases.check_hand_checked(emu, CPU)


def test_wave_and_chunk_boundaries(emu):
    cases.check_wave_boundaries(emu, CPU)


def test_non_canonical_counts(emu):
    cases.check_non_canonical(emu, CPU)


def test_crowd_ground_truths(emu):
    cases.check_crowd(emu, CPU)


def test_unit_geometry(emu):
    cases.check_unit_geometry(emu, CPU)


def test_300_seeded_random_pairs(emu):
    cases.check_random_pairs(emu, CPU)


def test_union_in_64_bits(emu):
    cases.check_union_64bit(emu, CPU)


def test_refusals(emu):
    cases.check_refusals(emu, CPU, pytest)


# ------------------------------------------------------------------------------------------------------------ metric + API
def test_coco_metric_on_the_nwpu_subset_bits_equals_runs_equals_the_oracle(emu, tmp_path):
    from rsprompter_amd import evaluation
    cases.check_metric_nwpu(evaluation, CPU, tmp_path)


def test_coco_metric_on_a_synthetic_scene_set_and_the_auto_route(emu, tmp_path, monkeypatch):
    from rsprompter_amd import apis, evaluation
    cases.check_metric_scenes(evaluation, apis, CPU, tmp_path, [(256, 192), (200, 240)], monkeypatch)


def test_an_unknown_iou_domain_is_refused():
    from rsprompter_amd import evaluation
    cases.check_metric_refusals(evaluation, pytest)


def test_mask_iou_forms_crowds_and_refusals(emu):
    from rsprompter_amd import apis
    cases.check_mask_iou(apis, CPU, pytest)


# ---------------------------------------------------------------------------------------------------------------- evaluate
def test_rank_order_and_duplicates_are_shared_by_the_tile_and_the_scene_path():
    """fabricated per-rank lists, no process group: 7 items on 3 ranks (shards padded by wrap-around to 3 each)"""
    from rsprompter_amd import dist as rdist
    from rsprompter_amd import evaluate as E
    world, n = 3, 7
    shards = [rdist.shard_indices(n, r, world) for r in range(world)]
    assert sorted(i for sh in shards for i in sh) == sorted(list(range(n)) + [0, 1])
    # the scene path: whole per-rank lists, rank after rank
    per_rank = [[f'r{r}:{i}' for i in sh] for r, sh in enumerate(shards)]
    idx, preds = E.first_predictions(E.rank_order(shards), [p for got in per_rank for p in got])
    assert idx == list(range(n))
    assert preds == ['r0:0', 'r1:1', 'r2:2', 'r0:3', 'r1:4', 'r2:5', 'r0:6']            # the wrap-around copies (r1:0, r2:1) dropped
    # the tile path: per step, image i of every rank in rank order -- the same predictions
    order, got = [], []
    for s in range(0, len(shards[0]), 2):
        step = E.step_order(shards, s, 2)
        order += step
        got += [f'r{r}:{sh[s + j]}' for j in range(2) for r, sh in enumerate(shards) if s + j < len(sh)]
    assert E.first_predictions(order, got) == (idx, preds)
    assert E.step_order([[0, 2], [1, 0]], 0, 1) == [0, 1] and E.rank_order([[0, 2], [1, 0]]) == [0, 2, 1, 0]
    with pytest.raises(ValueError, match='gathered'):
        E.first_predictions([0, 1], ['a'])


def test_evaluate_takes_large_image_and_iou_domain():
    import inspect
    from rsprompter_amd import evaluate as E
    sig = inspect.signature(E.evaluate).parameters
    assert sig['large_image'].default is None and sig['iou_domain'].default is None
    assert E.LARGE_IMAGE_KEYS == ('patch_size', 'patch_overlap_ratio', 'merge_iou_thr', 'merge_nms_type', 'seam_iou_thr',
                                  'batch_size', 'min_mask_region_area')
    with pytest.raises(ValueError, match='large_image takes'):
        E.evaluate(None, {}, large_image=dict(patch=640))
    with pytest.raises(SystemExit):
        E.main(['cfg.py', 'none', '--iou-domain', 'rle'])
    with pytest.raises(SystemExit):
        E.main(['cfg.py', 'none', '--patch-size', '640'])                            # applies to --large-image only
