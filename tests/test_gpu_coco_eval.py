"""MI355X: COCO evaluation on the device (csrc/cocoeval.hip) at production scale, exactly equal to the cocoapi
restatement (tests/_cocoeval_ref.py), and end to end through `rsprompter_amd.evaluate` on the NWPU fixture."""
import os
import socket
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _coco_cases as cc  # noqa: E402
import _cocoeval_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = (0.406 * 255, 0.456 * 255, 0.485 * 255)


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from rsprompter_amd import ops as o
    return o


@pytest.mark.quick
def test_rle_string_roundtrip_at_scale(dev, ops):
    rng = np.random.default_rng(10)
    cc.check_string_roundtrip(ops, dev, [cc.random_mask(rng, 1024, 1024, k) for k in ('blob', 'empty', 'full', 'pixel')])
    cc.check_string_roundtrip(ops, dev, [cc.random_mask(rng, 16, 8192, k) for k in ('blob', 'noise', 'pixel')])
    cc.check_string_roundtrip(ops, dev, [cc.random_mask(rng, 96, 80, 'noise') for _ in range(3)], cap=16)  # cap growth


@pytest.mark.quick
def test_iou_at_scale_masks_and_boxes(dev, ops):
    rng = np.random.default_rng(11)
    assert cc.check_iou(ops, dev, rng, 1, 100, 300, 1024, 1024, mode='segm') > 100
    assert cc.check_iou(ops, dev, rng, 64, 12, 8, 512, 512, mode='segm') > 100
    assert cc.check_iou(ops, dev, rng, 1, 100, 300, 1024, 1024, mode='bbox') > 100
    assert cc.check_iou(ops, dev, rng, 64, 12, 8, 512, 512, mode='bbox') > 100


@pytest.mark.quick
def test_match_and_stats_on_random_units(dev):
    """forced score ties within and across images, IoUs exactly at thresholds, areas on range boundaries, more than
    100 dts per image, images without gt or dt, gt id 0"""
    rng = np.random.default_rng(12)
    gt, res = cc.synth_eval_case(rng, 24, 3, 130, 12, 320, 320, mode='bbox')
    assert max(np.unique([r['image_id'] for r in res], return_counts=True)[1]) > 100
    cc.check_stats_equal(gt, res, 'bbox', dev)
    gt, res = cc.synth_eval_case(rng, 10, 2, 30, 6, 256, 240, mode='segm')
    cc.check_stats_equal(gt, res, 'segm', dev)


def _cfg(batch_size=2):
    from rsprompter_amd.config import Config
    from rsprompter_amd.default_configs import rsprompter_anchor
    pipeline = [dict(type='LoadImageFromFile', backend_args=None, to_float32=True),
                dict(type='Resize', scale=(1024, 1024), keep_ratio=True),
                dict(type='Pad', size=(1024, 1024), pad_val=dict(img=PAD, masks=0)),
                dict(type='LoadAnnotations', with_bbox=True, with_mask=True),
                dict(type='PackDetInputs', meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'pad_shape',
                                                      'scale_factor'))]
    return Config(dict(
        model=rsprompter_anchor('base', 10),
        test_dataloader=dict(batch_size=batch_size, dataset=dict(
            type='NWPUInsSegDataset', data_root=cc.FIXTURE, ann_file='NWPU_instances_val_subset.json',
            data_prefix=dict(img='imgs'), test_mode=True, pipeline=pipeline, backend_args=None)),
        test_evaluator=dict(type='CocoMetric', metric=['bbox', 'segm'], format_only=False, backend_args=None)))


def _ref_stats_of(metric, prefix):
    """the restatement on the metric's own ground truth and its written result files"""
    import json
    out = {}
    for t in ('bbox', 'segm'):
        res = json.load(open(f'{prefix}.{t}.json'))
        out[t] = ref.coco_stats(metric.coco_gt, res, t)[0]
    return out


KEYS = [f'coco/{t}_{k}' for t in ('bbox', 'segm') for k in ('mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l')]


def test_end_to_end_anchor_vitb_on_nwpu_fixture_both_gt_paths(dev, tmp_path):
    import rsprompter_amd as ra
    from rsprompter_amd import evaluate as E
    from rsprompter_amd.synth import synth_state_dict
    ref.use_numpy_forms()
    cfg = _cfg()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = ra.build_model(cfg)
    model.load_state_dict(synth_state_dict(model, seed=0), strict=True)
    model = model.to(dev).eval()
    for path in ('default', 'ann_file'):
        prefix = str(tmp_path / path / 'r')
        res = E.evaluate(model, cfg, out_prefix=prefix, verbose=False,
                         metric_ann_file=cc.FIXTURE_JSON if path == 'ann_file' else None)
        assert list(res) == KEYS
        m = E.evaluate.last_metric
        want = _ref_stats_of(m, prefix)
        for t in ('bbox', 'segm'):
            assert np.array_equal(m.eval_results[t].stats, want[t]), (path, t, m.eval_results[t].stats, want[t])
        if path == 'default':
            assert all(a['id'] >= 1 and a['iscrowd'] == 0 for a in m.coco_gt['annotations'])
        else:
            assert any(a['id'] == 0 for a in m.coco_gt['annotations'])


class _GtModel(torch.nn.Module):
    """test_step returns the image's ground truth as predictions (descending scores)"""

    def __init__(self, ds, dev):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1, device=dev))
        self.by_id = {ds.data_list[i]['img_id']: i for i in range(len(ds))}
        self.ds = ds

    def test_step(self, data):
        from rsprompter_amd.structures import DetDataSample, InstanceData
        out = []
        for s in data['data_samples']:
            g = self.ds[self.by_id[s.metainfo['img_id']]]
            keep = ~g['ignore_flags']
            h, w = g['ori_shape']
            masks = [ref.rle_decode(ref.rle_fr_string(m['counts']), h, w) for m, k in zip(g['masks'], keep) if k]
            n = int(keep.sum())
            o = DetDataSample(metainfo=dict(s.metainfo))
            o.pred_instances = InstanceData(
                bboxes=torch.from_numpy(g['bboxes'][keep]).to(self.p.device),
                scores=torch.linspace(0.99, 0.5, max(n, 1))[:n].to(self.p.device),
                labels=torch.from_numpy(g['labels'][keep]).to(self.p.device),
                masks=torch.from_numpy(np.stack(masks) if n else np.zeros((0, h, w), np.uint8)).bool().to(self.p.device))
            out.append(o)
        return out


def test_ground_truth_as_predictions_scores_one(dev, tmp_path):
    from rsprompter_amd import evaluate as E
    ref.use_numpy_forms()
    cfg = _cfg(batch_size=4)
    ds = E.build_test_dataset(cfg)
    res = E.evaluate(_GtModel(ds, dev), cfg, out_prefix=str(tmp_path / 'r'), verbose=False)
    m = E.evaluate.last_metric
    areas = np.array([a['area'] for a in m.coco_gt['annotations']])
    has = dict(mAP=True, mAP_50=True, mAP_75=True, mAP_s=bool((areas <= 32 ** 2).any()),
               mAP_m=bool(((areas >= 32 ** 2) & (areas <= 96 ** 2)).any()), mAP_l=bool((areas >= 96 ** 2).any()))
    for k, v in res.items():
        assert v == (1.0 if has[k.split('_', 1)[1]] else -1.0), (k, v)
    want = _ref_stats_of(m, str(tmp_path / 'r'))
    for t in ('bbox', 'segm'):
        assert np.array_equal(m.eval_results[t].stats, want[t])


def _worker(rank, world, port, ret):
    os.environ.update(RANK=str(rank), LOCAL_RANK='0', WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    import torch.distributed as dist
    from rsprompter_amd import dist as rdist
    from rsprompter_amd import evaluate as E
    dev = torch.device('cuda:0')
    try:
        rdist.init_from_env(backend='gloo')
        cfg = _cfg(batch_size=2)
        ds = E.build_test_dataset(cfg)
        res = E.evaluate(_GtModelNoisy(ds, dev), cfg, verbose=False)
        ret[rank] = None if res is None else (dict(res), {t: E.evaluate.last_metric.eval_results[t].stats.tolist()
                                                          for t in ('bbox', 'segm')})
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        ret[rank] = repr(e)


class _GtModelNoisy(_GtModel):
    """ground truth with every other instance shifted and re-scored: metrics below 1, different per image"""

    def test_step(self, data):
        out = super().test_step(data)
        for o in out:
            p = o.pred_instances
            if len(p.bboxes):
                p.bboxes = p.bboxes + torch.arange(len(p.bboxes), device=p.bboxes.device)[:, None].float() % 2 * 7
                p.masks = torch.roll(p.masks, shifts=int(o.metainfo['img_id']) % 5, dims=2)
        return out


def test_two_ranks_on_one_device_equal_world_one():
    from rsprompter_amd import evaluate as E
    cfg = _cfg(batch_size=2)
    ds = E.build_test_dataset(cfg)
    one = E.evaluate(_GtModelNoisy(ds, torch.device('cuda:0')), cfg, verbose=False)
    stats1 = {t: E.evaluate.last_metric.eval_results[t].stats.tolist() for t in ('bbox', 'segm')}
    assert any(v < 1.0 for v in one.values())
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()    # noqa: E702
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    assert not isinstance(ret[0], str) and not isinstance(ret[1], str), f'{ret[0]} / {ret[1]}'
    assert ret[1] is None
    assert ret[0][0] == one and ret[0][1] == stats1
