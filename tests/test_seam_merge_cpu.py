"""CPU (`-m "not gpu"`): merging instances cut by tile seams (csrc/seam_merge.hip, rsprompter_amd/large_image.py
merge_nms_type='seam_mask').

The oracle is tests/_seam_merge_ref.py (the definition on dense numpy masks and its interval-domain twin) with
oracle/glue.py::batched_nms; the kernels run lane by lane on the emulator (tests/wave_emu), the sources unchanged, and
must agree exactly.  The kernel bodies are tests/_seam_merge_cases.py, the same the device tier runs."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _large_image_ref as lref  # noqa: E402
import _seam_merge_cases as cases  # noqa: E402
import _seam_merge_ref as sref  # noqa: E402

SEAM_THR, NMS_THR = 0.3, 0.25
SCENE_SEED = 16                     # the draw of the random-stub scene: test_the_random_stub_scene_... says what it must hold


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# ------------------------------------------------------------------------------------------------------- restatement
def test_restatement_interval_twin_equals_the_dense_definition():
    rng = np.random.default_rng(20)
    for _ in range(60):
        H, W = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        ms = [rng.random((H, W)) < float(rng.choice([0.0, 0.2, 0.6, 1.0])) for _ in range(3)]
        ivs = [sref.counts_to_iv(lref.rle_counts(m)) for m in ms]
        x0, x1 = sorted(rng.integers(-1, W + 2, 2).tolist())
        y0, y1 = sorted(rng.integers(-1, H + 2, 2).tolist())
        assert sref.iv_pair_overlap(ivs[0], ivs[1], (x0, y0, x1, y1), H, W) == sref.pair_overlap_dense(ms[0], ms[1], (x0, y0, x1, y1))
        assert sref.iv_union_counts(ivs, H, W) == lref.rle_counts(ms[0] | ms[1] | ms[2])
        assert sref.iv_bbox_area(ivs[2], H) == sref.bbox_area_dense(ms[2])
    assert sref.iv_union_counts([], 3, 4) == [12]
    assert sref.is_edge(3, 5, 4, 0.5) and not sref.is_edge(0, 0, 0, 0.0) and not sref.is_edge(2, 5, 4, 0.5)
    comps = sref.components(6, [(4, 5), (0, 4), (1, 2)], [0.5, 0.9, 0.9, 0.1, 0.7, 0.7])
    assert comps == [(1, [1, 2]), (3, [3]), (4, [0, 4, 5])]          # ties go to the lowest index; ascending by representative


# ------------------------------------------------------------------------------------------------------------ kernels
def test_rle_bbox_kernel(emu):
    cases.check_rle_bbox(emu, torch.device('cpu'))


def test_rle_pair_overlap_kernel(emu):
    cases.check_rle_pair_overlap(emu, torch.device('cpu'))


def test_rle_union_kernel(emu):
    cases.check_rle_union(emu, torch.device('cpu'))


def test_scenes_beyond_32_bit_counts_are_refused(emu):
    cases.check_refuses_scenes_beyond_32_bit_counts(emu, torch.device('cpu'), pytest)


# ----------------------------------------------------------------------------------------------------------- pipeline
def _random_scene(emu_ops=None):
    """the 45 x 70 scene, 32-pixel tiles, and the stub's per-tile results through the per-crop test pipeline"""
    from rsprompter_amd.apis import TestPipeline, get_test_pipeline_cfg
    rng = np.random.default_rng(SCENE_SEED)
    H, W, patch = 45, 70, 32
    scene = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    model = cases.RandomStub((patch, patch))
    pipe = TestPipeline(get_test_pipeline_cfg(model.cfg), device='cpu')
    tiles = lref.slice_bboxes(H, W, patch, patch, 0.25, 0.25)
    per_tile = []
    for x0, y0, x1, y1 in tiles:
        d = pipe(dict(img=np.ascontiguousarray(scene[y0:y1, x0:x1]), img_id=0))
        p = model.test_step(dict(inputs=[d['inputs']], data_samples=[d['data_samples']]))[0].pred_instances
        per_tile.append(dict(bboxes=p.bboxes.numpy(), scores=p.scores.numpy(), labels=p.labels.numpy(), masks=p.masks.numpy()))
    return scene, model, tiles, per_tile, patch


@pytest.fixture(scope='module')
def random_scene(emu):
    from oracle import glue
    scene, model, tiles, per_tile, patch = _random_scene()
    offsets = [(t[0], t[1]) for t in tiles]
    want = sref.seam_merge_dense(per_tile, offsets, tiles, scene.shape[:2], SEAM_THR, glue.batched_nms, NMS_THR)
    return dict(scene=scene, model=model, tiles=tiles, offsets=offsets, per_tile=per_tile, patch=patch, want=want)


def test_the_random_stub_scene_holds_what_the_pipeline_test_needs(random_scene):
    """about the draw itself, from the restatement alone: an edge, a rejected pair that does intersect, a component of
    three or more, an instance the box NMS removes after the merge"""
    w = random_scene['want']
    assert len(w['edges']) >= 1 and len(w['rejected']) >= 1
    assert max(len(m) for _, m in w['comps']) >= 3
    assert len(w['keep']) < w['n_merged']
    dens = [float(m.mean()) for r in random_scene['per_tile'] for m in r['masks']]
    assert 0.0 in dens and 1.0 in dens and any(0.4 < d < 0.6 for d in dens) and any(0.0 < d < 0.15 for d in dens)
    assert {int(v) for r in random_scene['per_tile'] for v in r['labels']} == {0, 1}


def test_seam_mask_pipeline_around_a_random_stub_detector(emu, random_scene):
    from oracle import rle as orle
    from rsprompter_amd import large_image as li
    s, w = random_scene, random_scene['want']
    H, W = s['scene'].shape[:2]
    want_strings = [orle.rle_to_string(c) for c in w['counts']]
    for bs in (1, 4):
        out = li.inference_large_image(s['model'], s['scene'], patch_size=s['patch'], batch_size=bs, merge_iou_thr=NMS_THR,
                                       merge_nms_type='seam_mask', seam_iou_thr=SEAM_THR)
        p = out.pred_instances
        assert out.keep.tolist() == w['keep'] and out.members == w['members']
        assert np.array_equal(p.bboxes.numpy(), w['bboxes']) and np.array_equal(p.scores.numpy(), w['scores'])
        assert np.array_equal(p.labels.numpy(), w['labels'])
        assert [m['counts'] for m in p.masks] == want_strings and all(m['size'] == [H, W] for m in p.masks)
    js = li.pred2dict(out, 0.5)
    assert len(js['labels']) == int((w['scores'] >= 0.5).sum()) == len(js['masks']) and all(isinstance(m['counts'], str) for m in js['masks'])
    # dense masks: equal to the decoded RLE
    dense = li.inference_large_image(s['model'], torch.from_numpy(s['scene']), patch_size=s['patch'], batch_size=3,
                                     merge_iou_thr=NMS_THR, merge_nms_type='seam_mask', seam_iou_thr=SEAM_THR, masks='dense')
    dm = dense.pred_instances.masks.numpy()
    assert dm.dtype == bool and dm.shape == (len(w['keep']), H, W) and dense.members == w['members']
    for k in range(len(w['keep'])):
        assert np.array_equal(dm[k], w['masks'][k]) and np.array_equal(dm[k], lref.counts_to_mask(w['counts'][k], H, W))


def test_merge_results_by_nms_with_the_seam_mask_config(emu, random_scene):
    from rsprompter_amd.large_image import merge_results_by_nms
    from rsprompter_amd.structures import DetDataSample, InstanceData
    s, w = random_scene, random_scene['want']
    results = []
    for r in s['per_tile']:
        d = DetDataSample(metainfo=dict(ori_shape=(s['patch'], s['patch'])))
        d.pred_instances = InstanceData(bboxes=torch.from_numpy(r['bboxes']), scores=torch.from_numpy(r['scores']),
                                        labels=torch.from_numpy(r['labels']), masks=torch.from_numpy(r['masks']))
        results.append(d)
    out = merge_results_by_nms(results, s['offsets'], s['scene'].shape[:2],
                               dict(type='seam_mask', iou_threshold=NMS_THR, seam_iou_threshold=SEAM_THR))
    p = out.pred_instances
    assert out.keep.tolist() == w['keep'] and out.members == w['members']
    assert np.array_equal(p.bboxes.numpy(), w['bboxes']) and np.array_equal(p.scores.numpy(), w['scores'])
    assert np.array_equal(p.labels.numpy(), w['labels'])
    assert all(np.array_equal(p.masks[k].numpy(), w['masks'][k]) for k in range(len(w['keep'])))


def test_nms_mode_is_unchanged_on_the_random_stub_scene(emu, random_scene):
    from oracle import glue
    from oracle import rle as orle
    from rsprompter_amd import large_image as li
    s = random_scene
    H, W = s['scene'].shape[:2]
    keep, boxes, scores, labels, tile = lref.merge(s['per_tile'], s['offsets'], (H, W), glue.batched_nms, NMS_THR)
    all_masks = [m for r in s['per_tile'] for m in r['masks']]
    want = [orle.rle_to_string(lref.rle_counts(lref.shift_masks(all_masks[i][None], s['offsets'][tile[i]], (H, W))[0])) for i in keep]
    out = li.inference_large_image(s['model'], s['scene'], patch_size=s['patch'], batch_size=4, merge_iou_thr=NMS_THR)
    p = out.pred_instances
    assert out.keep.tolist() == keep.tolist() and not hasattr(out, 'members')
    assert np.array_equal(p.bboxes.numpy(), boxes[keep]) and np.array_equal(p.scores.numpy(), scores[keep])
    assert [m['counts'] for m in p.masks] == want


def test_planted_objects_come_back_whole(emu):
    """the test that shows the feature: 8 planted objects, 19 fragments -> 8 instances; box NMS alone returns more"""
    from rsprompter_amd import large_image as li
    cases.check_planted_objects(li, torch.device('cpu'))


def test_synthetic_scene_in_the_interval_domain_small(emu):
    """the body of the device tier's test at scale, on a 90 x 120 scene: ellipses built as runs, noise masks in the overlap
    bands; all three kernels and the merge against the interval-domain restatement"""
    from rsprompter_amd import large_image as li
    info = cases.check_at_scale(emu, li, torch.device('cpu'), 90, 120, 32, 40, 7, seed=1)
    assert info['instances'] > 60 and info['kept'] < info['instances']


def test_unsupported_combinations_raise_clearly(emu):
    from rsprompter_amd import large_image as li
    from rsprompter_amd.structures import DetDataSample, InstanceData

    class NoMasks(cases.RandomStub):
        def test_step(self, data):
            res = super().test_step(data)
            for r in res:
                p = r.pred_instances
                r.pred_instances = InstanceData(bboxes=p.bboxes, scores=p.scores, labels=p.labels)
            return res
    scene = np.zeros((40, 40, 3), np.uint8)
    with pytest.raises(ValueError, match='masks'):
        li.inference_large_image(NoMasks((32, 32)), scene, patch_size=32, merge_nms_type='seam_mask')
    assert len(li.inference_large_image(NoMasks((32, 32)), scene, patch_size=32).pred_instances.scores) > 0   # 'nms' needs none
    with pytest.raises(NotImplementedError, match='soft_nms'):
        li.inference_large_image(None, scene, merge_nms_type='soft_nms', seam_iou_thr=0.3)
    d = DetDataSample(metainfo=dict(ori_shape=(8, 8)))
    d.pred_instances = InstanceData(bboxes=torch.zeros((1, 4)), scores=torch.ones(1), labels=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match='masks'):
        li.merge_results_by_nms([d], [(0, 0)], (8, 8), dict(type='seam_mask', iou_threshold=0.25))
    with pytest.raises(NotImplementedError, match='class_agnostic'):
        li.merge_results_by_nms([d], [(0, 0)], (8, 8), dict(type='seam_mask', class_agnostic=True))
    with pytest.raises(ValueError, match='10800000000'):
        li._seam_dense(torch.zeros((3, 4, 4), dtype=torch.bool), torch.zeros((3, 2), dtype=torch.int32),
                       (torch.arange(3), torch.tensor([0, 2, 3], dtype=torch.int32)), (60000, 60000))
