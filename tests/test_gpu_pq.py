"""-m gpu: panoptic quality on the device -- the bodies of tests/_pq_cases.py (all ==, the doubles included), one 1024 x 1024
map with 100 segments a side, bit-reproducibility, the chain ops.panoptic_fuse -> ops.pq_image with nothing on the host in
between, and CocoPanopticMetric end to end.  Reference: tests/_pq_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pq_cases as qc  # noqa: E402
import _pq_ref as pr  # noqa: E402


@pytest.fixture(scope='module')
def ops():
    from rsprompter_amd import ops
    return ops


@pytest.fixture(scope='module')
def big():
    """1024 x 1024, 100 segments a side, and the reference's result (computed once)"""
    pan, gt, segments = qc.generate(1024, 1024, 100, 11)
    return pan, gt, segments, qc.reference(pan, gt, segments)


@pytest.mark.quick
@pytest.mark.parametrize('shape', qc.GEN_SHAPES, ids=lambda s: '%dx%d' % s[:2])
def test_generated(ops, dev, shape):
    qc.check_generated(ops, dev, shape)


@pytest.mark.quick
def test_noise(ops, dev):
    qc.check_noise(ops, dev)


@pytest.mark.quick
@pytest.mark.parametrize('check', qc.HAND_CHECKED, ids=lambda f: f.__name__[6:])
def test_hand_checked(ops, dev, check):
    check(ops, dev)


@pytest.mark.quick
@pytest.mark.parametrize('P', (70, 1024))
def test_many_segments(ops, dev, P):
    qc.check_many_segments(ops, dev, P)


@pytest.mark.quick
def test_refusals(ops, dev):
    qc.check_refusals(ops, dev, 'cpu')


@pytest.mark.quick
def test_large_map(ops, dev, big):
    pan, gt, segments, want = big
    for rgb in (False, True):
        got = qc.to_host(qc.run(ops, dev, pan, gt, segments, rgb=rgb))
        assert got['status'] == 0 and got['segments'] == want['segments'] and got['stat'] == want['stat'], rgb
    assert len(want['segments']) > 60 and min(sum(want['stat'][c][k] for c in qc.CATS) for k in range(3)) > 0


@pytest.mark.quick
def test_bit_reproducible(ops, dev, big):
    """integer atomics only and fixed orders of the double sums: two runs give the same bits in every tensor of the row"""
    pan, gt, segments, _ = big
    a = qc.run(ops, dev, pan, gt, segments, rgb=True)
    b = qc.run(ops, dev, pan, gt, segments, rgb=True)
    assert all(torch.equal(a[k], b[k]) for k in a)
    ra, rb = ops.pq_reduce([a, b, a]), ops.pq_reduce([a, b, a])
    assert torch.equal(ra['packed'], rb['packed'])


@pytest.mark.quick
def test_fuse_then_score_on_the_device(ops, dev):
    """ops.panoptic_fuse -> ops.pq_image on an exact case of tests/_mask_field_props.py with the fp64 reference map of
    tests/_panoptic_ref.py as the ground truth: the predicted map goes from one kernel to the next as a device tensor, and
    every painted class has PQ == 100 (each of its segments a TP with IoU exactly 1)"""
    import _mask_field_props as mf
    import _panoptic_cases as pc
    import _panoptic_ref as fr
    case = mf.EXACT_CASES[0]
    cls, low = pc.exact_inputs(case, pc.exact_seed(case))
    r = fr.reference(cls, low, pc.geo_of(case), pc.NTHINGS, pc.NC, **pc.EXACT_CFGS[1])
    ref_map = r['sem'].numpy().astype(np.int64)
    gt = np.where(ref_map % 1000 == pc.NC, 0, ref_map)
    ids = [int(i) for i in np.unique(gt) if i != 0]
    assert {i % 1000 for i in ids} == {0, 1, 2}                     # a stuff segment and two things: every class is painted
    cats = {c: dict(isthing=1 if c < pc.NTHINGS else 0) for c in range(pc.NC)}
    sem, _ = ops.panoptic_fuse(cls.to(dev), low.to(dev), *pc.geo_of(case), pc.NTHINGS, pc.NC, **pc.EXACT_CFGS[1])
    assert sem.is_cuda and sem.dtype == torch.int32
    row = ops.pq_image(sem, torch.from_numpy(gt).to(dev), [qc.seg(i, i % 1000) for i in ids], cats, pc.NC)
    assert all(v.is_cuda for v in row.values())
    got = qc.to_host(row, cats)
    assert got['status'] == 0 and [s[0] for s in got['segments']] == ids
    for c in cats:
        n = sum(1 for i in ids if i % 1000 == c)
        assert got['stat'][c] == [n, 0, 0, float(n)], c
    from rsprompter_amd.evaluation import pq_average
    res, per_class = pq_average({c: tuple(v) for c, v in got['stat'].items()}, cats)
    assert res['pq'] == 1.0 and all(per_class[i % 1000]['pq'] == 1.0 for i in ids)


def test_metric_end_to_end(dev, tmp_path):
    """CocoPanopticMetric on the device: device predictions, the gt once in memory and once as a PNG read by PIL"""
    from PIL import Image
    from rsprompter_amd.evaluation import CocoPanopticMetric
    classes = ('a', 'b', 'c', 'd')
    ims = [qc.generate(37, 53, 12, s) for s in (3, 4, 5)]
    cats = {i: dict(isthing=1 if i < 3 else 0) for i in range(4)}
    want = pr.nine_keys(pr.add_stats([qc.reference(*im) for im in ims], list(cats)), cats)
    m = CocoPanopticMetric(classwise=True)
    m.dataset_meta = dict(classes=classes, thing_classes=classes[:3])
    for k, (pan, gt, segments) in enumerate(ims):
        s = dict(img_id=k, img_path=f'im{k}.jpg', pred_panoptic_seg=dict(sem_seg=torch.from_numpy(pan)[None].to(dev)))
        if k == 1:
            path = os.path.join(tmp_path, 'im1.png')
            Image.fromarray(pr.id2rgb(gt), 'RGB').save(path)
            s.update(seg_map_path=path, segments_info=[dict(id=g['id'], category=g['category_id'],
                                                            is_thing=g['category_id'] < 3 and not g['iscrowd']) for g in segments])
        else:
            s.update(gt_panoptic=torch.from_numpy(gt).to(dev), segments_info=segments)
        m.process(None, [s])
    assert all(v.is_cuda for r in m.results for v in r['row'].values())
    got = m.evaluate(3)
    assert {k.split('/')[1]: v for k, v in got.items()} == want and want['PQ'] > 0
