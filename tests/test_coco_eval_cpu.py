"""CPU (`-m "not gpu"`): COCO bbox / segm evaluation (csrc/cocoeval.hip, rsprompter_amd/evaluation.py, datasets.py).

Three legs, since pycocotools is not installed: a literal restatement of cocoapi (tests/_cocoeval_ref.py) as the oracle,
hand-derived known answers asserted on the restatement AND on the product path, and the new kernels executed lane by lane
on the emulator (tests/wave_emu) with results exactly equal to the restatement."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _coco_cases as cc  # noqa: E402
import _cocoeval_ref as ref  # noqa: E402

DEV = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def _img(i, h=200, w=200):
    return dict(id=i, height=h, width=w, file_name=f'{i}.jpg')


def _metric_on(gt, preds, classes, tmp_path, metric='bbox', ann_file=True, samples_gt=None):
    """CocoMetric through process / evaluate, on the emulated device.  preds: {img_id: (xyxy, scores, labels[, masks])}"""
    from rsprompter_amd.evaluation import CocoMetric
    kw = {}
    if ann_file:
        p = tmp_path / 'gt.json'
        p.write_text(json.dumps(gt))
        kw['ann_file'] = str(p)
    m = CocoMetric(metric=metric, device='cpu', **kw)
    m.dataset_meta = dict(classes=classes)
    samples = []
    for im in gt['images']:
        b, s, lb, *mk = preds.get(im['id'], (np.zeros((0, 4)), np.zeros(0), np.zeros(0, np.int64)))
        pi = dict(bboxes=torch.tensor(np.asarray(b, np.float32).reshape(-1, 4)), scores=torch.tensor(np.asarray(s, np.float32)),
                  labels=torch.tensor(np.asarray(lb, np.int64)))
        if mk:
            pi['masks'] = mk[0]
        smp = dict(pred_instances=pi, img_id=im['id'], ori_shape=(im['height'], im['width']))
        if samples_gt is not None:
            smp['gt_instances'] = samples_gt[im['id']]
        samples.append(smp)
    m.process(None, samples)
    return m.evaluate(len(samples)), m


def _xyxy(b):
    return [b[0], b[1], b[0] + b[2], b[1] + b[3]]


# ----------------------------------------------------------------------------- hand-derived known answers
BBOX_CASE_GT = dict(images=[_img(1)], categories=[dict(id=1, name='a')],
                    annotations=[dict(id=1, image_id=1, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0)])
BBOX_CASE_DT = [dict(image_id=1, category_id=1, bbox=[50, 50, 10, 10], score=0.9),
                dict(image_id=1, category_id=1, bbox=[0, 0, 10, 7.5], score=0.8)]
BBOX_CASE_WANT = dict(bbox_mAP=0.3, bbox_mAP_50=0.5, bbox_mAP_75=0.5, bbox_mAP_s=0.3, bbox_mAP_m=-1.0, bbox_mAP_l=-1.0)


def test_known_answer_bbox_threshold_envelope_and_empty_ranges_restatement():
    """IoU exactly 0.75 matches at t = 0.75 (`<` comparison), the FP ranked first is lifted by the envelope: AP 0.5 at
    the six thresholds up to 0.75, 0 above; medium / large have no gt: -1"""
    stats, _ = ref.coco_stats(BBOX_CASE_GT, BBOX_CASE_DT, 'bbox')
    assert ref.bb_iou([[0, 0, 10, 7.5]], [[0, 0, 10, 10]], [0])[0, 0] == 0.75
    np.testing.assert_allclose(stats[:7], [0.3, 0.5, 0.5, 0.3, -1, -1, 0.6], rtol=0, atol=1e-12)


def test_known_answer_bbox_product(emu, tmp_path):
    preds = {1: ([_xyxy(d['bbox']) for d in BBOX_CASE_DT], [d['score'] for d in BBOX_CASE_DT], [0, 0])}
    res, m = _metric_on(BBOX_CASE_GT, preds, ['a'], tmp_path)
    assert res == {f'coco/{k}': v for k, v in BBOX_CASE_WANT.items()}
    assert list(res) == [f'coco/bbox_{k}' for k in ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l')]
    assert m.eval_results['bbox'].stats[6] == ref.coco_stats(BBOX_CASE_GT, BBOX_CASE_DT, 'bbox')[0][6]
    assert abs(m.eval_results['bbox'].stats[6] - 0.6) < 1e-12


def test_known_answer_crowd_region(emu, tmp_path):
    """a detection inside a crowd region is neither TP nor FP; its IoU with the crowd gt uses the detection's area"""
    gt = dict(images=[_img(1)], categories=[dict(id=1, name='a')],
              annotations=[dict(id=1, image_id=1, category_id=1, bbox=[0, 0, 100, 100], area=10000.0, iscrowd=1),
                           dict(id=2, image_id=1, category_id=1, bbox=[150, 150, 10, 10], area=100.0, iscrowd=0)])
    dt = [dict(image_id=1, category_id=1, bbox=[10, 10, 20, 20], score=0.9),
          dict(image_id=1, category_id=1, bbox=[150, 150, 10, 10], score=0.5)]
    assert ref.bb_iou([[10, 10, 20, 20]], [[0, 0, 100, 100]], [1])[0, 0] == 1.0
    stats, _ = ref.coco_stats(gt, dt, 'bbox')
    assert round(stats[0], 3) == 1.0                             # precision tp / (tp + fp + eps)
    preds = {1: ([_xyxy(d['bbox']) for d in dt], [d['score'] for d in dt], [0, 0])}
    res, m = _metric_on(gt, preds, ['a'], tmp_path)
    assert res['coco/bbox_mAP'] == 1.0
    assert np.array_equal(m.eval_results['bbox'].stats, stats)


def test_known_answer_101st_detection_outside_ar100(emu, tmp_path):
    gt = dict(images=[_img(1, 400, 400)], categories=[dict(id=1, name='a')],
              annotations=[dict(id=1, image_id=1, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0)])
    dt = [dict(image_id=1, category_id=1, bbox=[200 + i, 200, 5, 5], score=1.0 - i * 1e-3) for i in range(100)]
    dt.append(dict(image_id=1, category_id=1, bbox=[0, 0, 10, 10], score=0.01))
    stats, _ = ref.coco_stats(gt, dt, 'bbox')
    assert stats[6] == 0.0 and stats[7] == 1.0 and stats[8] == 1.0
    preds = {1: ([_xyxy(d['bbox']) for d in dt], [d['score'] for d in dt], [0] * len(dt))}
    _, m = _metric_on(gt, preds, ['a'], tmp_path)
    s = m.eval_results['bbox'].stats
    assert s[6] == 0.0 and s[7] == 1.0 and np.array_equal(s, stats)


def test_known_answer_category_without_gt_and_all_empty(emu, tmp_path):
    gt = dict(images=[_img(1)], categories=[dict(id=1, name='a'), dict(id=2, name='b')],
              annotations=[dict(id=1, image_id=1, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0)])
    dt = [dict(image_id=1, category_id=1, bbox=[0, 0, 10, 10], score=0.9),
          dict(image_id=1, category_id=2, bbox=[50, 50, 10, 10], score=0.95)]
    stats, _ = ref.coco_stats(gt, dt, 'bbox')
    assert round(stats[0], 3) == 1.0
    preds = {1: ([_xyxy(d['bbox']) for d in dt], [d['score'] for d in dt], [0, 1])}
    res, _ = _metric_on(gt, preds, ['a', 'b'], tmp_path)
    assert res['coco/bbox_mAP'] == 1.0
    gt0 = dict(gt, annotations=[])
    stats0, _ = ref.coco_stats(gt0, dt, 'bbox')
    assert list(stats0) == [-1.0] * 12
    res0, m0 = _metric_on(gt0, preds, ['a', 'b'], tmp_path)
    assert all(v == -1.0 for v in res0.values()) and list(m0.eval_results['bbox'].stats) == [-1.0] * 12


def test_known_answer_annotation_id_zero_counts_as_false_positive(emu, tmp_path):
    """pycocotools marks matches with annotation ids: the detection matched to the gt with id 0 is a FP (ann_file path)"""
    gt = dict(images=[_img(1)], categories=[dict(id=1, name='a')],
              annotations=[dict(id=0, image_id=1, category_id=1, bbox=[0, 0, 10, 10], area=100.0, iscrowd=0)])
    dt = [dict(image_id=1, category_id=1, bbox=[0, 0, 10, 10], score=0.9)]
    stats, _ = ref.coco_stats(gt, dt, 'bbox')
    assert stats[0] == 0.0 and stats[8] == 0.0
    preds = {1: ([_xyxy(dt[0]['bbox'])], [0.9], [0])}
    res, m = _metric_on(gt, preds, ['a'], tmp_path)
    assert res['coco/bbox_mAP'] == 0.0 and np.array_equal(m.eval_results['bbox'].stats, stats)
    gt1 = dict(gt, annotations=[dict(gt['annotations'][0], id=1)])
    res1, _ = _metric_on(gt1, preds, ['a'], tmp_path)
    assert res1['coco/bbox_mAP'] == 1.0


def test_known_answer_area_on_range_boundaries(emu, tmp_path):
    """gt area exactly 32^2 (96^2) is inside both adjacent ranges (inclusive at both ends)"""
    for side, on in ((32, (3, 4)), (96, (4, 5))):
        gt = dict(images=[_img(1, 300, 300)], categories=[dict(id=1, name='a')],
                  annotations=[dict(id=1, image_id=1, category_id=1, bbox=[0, 0, side, side], area=float(side * side),
                                    iscrowd=0)])
        dt = [dict(image_id=1, category_id=1, bbox=[0, 0, side, side], score=0.9)]
        stats, _ = ref.coco_stats(gt, dt, 'bbox')
        assert round(stats[on[0]], 3) == 1.0 and round(stats[on[1]], 3) == 1.0
        preds = {1: ([_xyxy(dt[0]['bbox'])], [0.9], [0])}
        _, m = _metric_on(gt, preds, ['a'], tmp_path)
        assert np.array_equal(m.eval_results['bbox'].stats, stats)


def test_known_answer_four_exact_matches_give_one_everywhere(emu, tmp_path):
    boxes = [[10, 10, 10, 10], [50, 50, 50, 50], [0, 200, 150, 100], [300, 300, 20, 20]]
    gt = dict(images=[_img(1, 500, 500)], categories=[dict(id=1, name='a')],
              annotations=[dict(id=i + 1, image_id=1, category_id=1, bbox=b, area=float(b[2] * b[3]), iscrowd=0)
                           for i, b in enumerate(boxes)])
    dt = [dict(image_id=1, category_id=1, bbox=b, score=0.9 - 0.1 * i) for i, b in enumerate(boxes)]
    stats, _ = ref.coco_stats(gt, dt, 'bbox')
    assert list(np.round(stats, 3)) == [1.0] * 12
    preds = {1: ([_xyxy(b) for b in boxes], [d['score'] for d in dt], [0] * 4)}
    res, m = _metric_on(gt, preds, ['a'], tmp_path)
    assert np.array_equal(m.eval_results['bbox'].stats, stats) and all(v == 1.0 for v in res.values())


def test_known_answer_polygon_rasterisation():
    """rleFrPoly worked through by hand: rectangle (1,1)-(4,3) -> pixels x in {1,2,3}, y in {1,2}; triangle
    (0,0),(4,0),(0,4) on 5x5 -> the pixels whose centres lie inside (x + y <= 2): columns of 3, 2, 1; the vertex (3, 0)
    is a crossing of two edges, the zero-length run between them is merged away"""
    from rsprompter_amd import datasets
    rect, tri = [1, 1, 4, 1, 4, 3, 1, 3], [0, 0, 4, 0, 0, 4]
    assert ref.rle_fr_poly(rect, 6, 6) == [7, 2, 4, 2, 4, 2, 15]
    assert ref.rle_fr_poly(tri, 5, 5) == [0, 3, 2, 2, 3, 1, 14]
    assert datasets.rle_from_poly(rect, 6, 6) == [7, 2, 4, 2, 4, 2, 15]
    assert datasets.rle_from_poly(tri, 5, 5) == [0, 3, 2, 2, 3, 1, 14]
    # two parts merged (rleMerge) = union of the decoded parts
    a = ref.rle_fr_poly([0, 0, 3, 0, 3, 3, 0, 3], 8, 8)
    b = ref.rle_fr_poly([2, 2, 6, 2, 6, 6, 2, 6], 8, 8)
    union = np.maximum(ref.rle_decode(a, 8, 8), ref.rle_decode(b, 8, 8))
    assert ref.rle_merge([a, b]) == ref.rle_encode(union) == datasets.rle_merge([a, b])


def test_known_answer_gt_paths_differ_on_area(emu, tmp_path):
    """a gt whose JSON area (800) is below 32^2 but whose box area (40 * 40) is above: small on the ann_file path,
    medium on the default path (gt_to_coco_json uses the float32 box area)"""
    gt = dict(images=[_img(1, 300, 300)], categories=[dict(id=0, name='a')],
              annotations=[dict(id=1, image_id=1, category_id=0, bbox=[10, 10, 40, 40], area=800.0, iscrowd=0)])
    preds = {1: ([[10, 10, 50, 50]], [0.9], [0])}
    res_file, _ = _metric_on(gt, preds, ['a'], tmp_path, ann_file=True)
    assert res_file['coco/bbox_mAP_s'] == 1.0 and res_file['coco/bbox_mAP_m'] == -1.0
    gi = {1: dict(bboxes=torch.tensor([[10., 10., 50., 50.]]), labels=torch.tensor([0]),
                  masks=[cc.rle_dict(np.pad(np.ones((40, 40), np.uint8), ((10, 250), (10, 250))))])}
    res_def, _ = _metric_on(gt, preds, ['a'], tmp_path, ann_file=False, samples_gt=gi)
    assert res_def['coco/bbox_mAP_s'] == -1.0 and res_def['coco/bbox_mAP_m'] == 1.0


# ----------------------------------------------------------------------------- string codec on the reference's vectors
def test_string_codec_on_reference_vectors(emu):
    from rsprompter_amd import rle
    items = json.load(open(os.path.join(HERE, 'golden', 'coco_rle_strings.json')))['items']
    strings = [it['counts'].encode() for it in items]
    lens = np.array([len(s) for s in strings])
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    flat = torch.from_numpy(np.frombuffer(b''.join(strings), dtype=np.uint8).copy())
    counts, n = emu.rle_from_string(flat, offs, cap=8)
    k = len(strings)
    _, offs2, flat2 = emu.rle_to_string(counts, n, k, int(offs[-1]) + 16)
    assert offs2.tolist() == offs.tolist()
    assert flat2[:int(offs[-1])].numpy().tobytes() == b''.join(strings)
    for i, s in enumerate(strings):
        want = ref.rle_fr_string(s)
        assert counts[i, :int(n[i])].to(torch.int64).tolist() == [int(v) for v in want]
        assert rle.counts_to_string(want) == s == ref.rle_to_string(want)
        assert ref.rle_area(want) == items[i]['area']
    h, w = items[0]['size']
    woff = torch.tensor([0] + [(it['size'][0] * it['size'][1] + 63) // 64 for it in items], dtype=torch.int64).cumsum(0)
    _, area, _ = emu.rle_to_bits(counts, n, woff)
    assert area.tolist() == [it['area'] for it in items]


# ----------------------------------------------------------------------------- the kernels on the emulator
def test_emu_string_roundtrip_bits_and_areas(emu):
    rng = np.random.default_rng(0)
    masks = [cc.random_mask(rng, 24, 40, k) for k in ('blob', 'empty', 'full', 'pixel', 'noise', 'blob')]
    cc.check_string_roundtrip(emu, DEV, masks, cap=4)                 # cap growth: 'noise' has hundreds of runs


def test_emu_iou_masks_and_boxes(emu):
    rng = np.random.default_rng(1)
    assert cc.check_iou(emu, DEV, rng, 5, 4, 3, 20, 36, mode='segm') > 0
    assert cc.check_iou(emu, DEV, rng, 5, 6, 5, 64, 64, mode='bbox') > 0


def test_emu_match_and_accumulate_bbox(emu):
    rng = np.random.default_rng(2)
    gt, res = cc.synth_eval_case(rng, 7, 2, 6, 4, 160, 160, mode='bbox')
    cc.check_stats_equal(gt, res, 'bbox', DEV)
    cc.check_stats_equal(gt, res, 'bbox', DEV, max_dets=(1, 3, 5))      # truncation by maxDets


def test_emu_match_and_accumulate_segm(emu):
    rng = np.random.default_rng(3)
    gt, res = cc.synth_eval_case(rng, 5, 2, 4, 3, 140, 130, mode='segm')
    cc.check_stats_equal(gt, res, 'segm', DEV)


# ----------------------------------------------------------------------------- datasets and configs
def test_dataset_on_fixture_follows_json_order_and_filters():
    from rsprompter_amd.datasets import DATASETS
    ds = DATASETS.build(dict(type='NWPUInsSegDataset', data_root=cc.FIXTURE, ann_file='NWPU_instances_val_subset.json',
                             data_prefix=dict(img='imgs'), test_mode=True, pipeline=[], backend_args=None))
    d = json.load(open(cc.FIXTURE_JSON))
    assert [ds[i]['img_id'] for i in range(len(ds))] == [im['id'] for im in d['images']]
    assert [os.path.basename(ds[i]['img_path']) for i in range(len(ds))] == [im['file_name'] for im in d['images']]
    assert all(os.path.exists(ds[i]['img_path']) for i in range(len(ds)))
    cat2label = {c['id']: i for i, c in enumerate(d['categories'])}
    for i, im in enumerate(d['images']):
        item = ds[i]
        anns = [a for a in d['annotations'] if a['image_id'] == im['id']]
        assert item['bboxes'].dtype == np.float32 and item['bboxes'].shape == (len(anns), 4)
        assert item['labels'].tolist() == [cat2label[a['category_id']] for a in anns]
        for a, b, m in zip(anns, item['bboxes'], item['masks']):
            x, y, w, h = a['bbox']
            assert b.tolist() == np.asarray([x, y, x + w, y + h], np.float32).tolist()
            want = ref.rle_merge([ref.rle_fr_poly(p, im['height'], im['width']) for p in a['segmentation']])
            assert ref.rle_fr_string(m['counts']) == want and m['size'] == [im['height'], im['width']]
    with pytest.raises(NotImplementedError):
        DATASETS.build(dict(type='NWPUInsSegDataset', data_root=cc.FIXTURE, ann_file='NWPU_instances_val_subset.json',
                            backend_args=dict(backend='local')))


def test_dataset_instance_filters():
    import tempfile
    from rsprompter_amd.datasets import CocoDataset
    d = dict(images=[_img(5, 50, 50)], categories=[dict(id=3, name='a')],
             annotations=[dict(id=1, image_id=5, category_id=3, bbox=[60, 60, 5, 5], area=25, segmentation=[[0, 0, 1, 0, 1, 1]]),
                          dict(id=2, image_id=5, category_id=3, bbox=[1, 1, 5, 5], area=0, segmentation=[[1, 1, 5, 1, 5, 5]]),
                          dict(id=3, image_id=5, category_id=3, bbox=[1, 1, 0.5, 5], area=2, segmentation=[[1, 1, 5, 1, 5, 5]]),
                          dict(id=4, image_id=5, category_id=9, bbox=[1, 1, 5, 5], area=25, segmentation=[[1, 1, 5, 1, 5, 5]]),
                          dict(id=5, image_id=5, category_id=3, bbox=[1, 1, 5, 5], area=25, iscrowd=1,
                               segmentation=[[1, 1, 5, 1, 5, 5]]),
                          dict(id=6, image_id=5, category_id=3, bbox=[1, 1, 5, 5], area=25, segmentation=[[1, 1, 5, 1]]),
                          dict(id=7, image_id=5, category_id=3, bbox=[2, 2, 5, 5], area=25,
                               segmentation=[[1, 1, 5, 1, 5, 5, 1], [2, 2, 8, 2, 8, 8]])])
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, 'a.json')
        json.dump(d, open(p, 'w'))
        ds = CocoDataset(ann_file=p, metainfo=dict(classes=('a',)))
        item = ds[0]
    assert item['ignore_flags'].tolist() == [True, True, False]            # crowd, no valid polygon, kept
    assert item['bboxes'].tolist() == [[1, 1, 6, 6], [1, 1, 6, 6], [2, 2, 7, 7]]
    assert ref.rle_fr_string(item['masks'][2]['counts']) == ref.rle_fr_poly([2, 2, 8, 2, 8, 8], 50, 50)


def test_configs_build_dataset_and_evaluator():
    import _ref_configs
    from rsprompter_amd.datasets import DATASETS
    from rsprompter_amd.evaluation import METRICS, CocoMetric
    cfgs = {n: _ref_configs.reference_config(n) for n in _ref_configs.names()}
    n = 0
    for name, cfg in cfgs.items():
        if 'test_dataloader' not in cfg or 'test_evaluator' not in cfg:
            continue
        ds_cfg = dict(cfg['test_dataloader']['dataset'])
        ds_cfg.update(data_root=cc.FIXTURE, ann_file='NWPU_instances_val_subset.json', data_prefix=dict(img='imgs'))
        ds = DATASETS.build(ds_cfg)
        assert len(ds) == 6
        ev = METRICS.build(cfg['test_evaluator'])
        assert isinstance(ev, CocoMetric) and ev.metrics == ['bbox', 'segm']
        n += 1
    assert n >= 10
    with pytest.raises(NotImplementedError):
        CocoMetric(metric='proposal_fast')
