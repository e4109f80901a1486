"""-m "not gpu": panoptic quality (csrc/panoptic_quality.hip, ops.pq_image / pq_reduce, evaluation.CocoPanopticMetric,
apis.panoptic_quality / write_panoptic_png) on the lane-level emulator (tests/wave_emu) against tests/_pq_ref.py, on maps of at
most 16k pixels, and the host layers.  The bodies (tests/_pq_cases.py) are the ones tests/test_gpu_pq.py runs on the device."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _pq_cases as qc  # noqa: E402
import _pq_ref as pr  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_two_forms_of_the_reference_agree():
    """A precondition on the reference alone (it runs no product code): tests/_pq_ref.py's loop and array form, ==, on every
    generated input, the noise map included, and the shapes are what the kernel's paths need"""
    for H, W, n in qc.GEN_SHAPES:
        for seed in (0, 1):
            qc.reference(*qc.generate(H, W, n, seed + 31 * H + W))
    qc.reference(*qc.generate(*qc.NOISE_SHAPE, 7, noise=True))
    assert {1, 2, 3} <= {W % 4 for _, W, _ in qc.GEN_SHAPES} and qc.GEN_SHAPES[:2] == ((1, 1, 1), (3, 5, 3))
    H, W, _ = qc.GEN_SHAPES[-1]
    assert H * W > 2 * 4096 and H * W % 4096 % 16 != 0 and H * W <= 16384    # blocks of 256 strips of 16: ragged twice over


def test_the_sum_of_the_order_case_depends_on_the_order():
    """A precondition on the order case alone (it runs no product code): in EACH of its three images the sum in ascending gt
    id has other bits than the sum in the map's order and than the sum in the JSON's order -- the orders a per-image kernel
    could take instead --, the reference sums in ascending id, and the total over the images in processing order has other
    bits than the totals that start with another pair of images.  So check_sum_order can tell these orders apart"""
    per_image, totals = qc.order_sums()
    ims = [qc.reference(*im) for im in qc.order_images()]
    for p, im in zip(per_image, ims):
        assert p['ascending'] != p['map'] and p['ascending'] != p['json'] and p['map'] != p['json']
        assert im['stat'][0][0] == 3 and im['stat'][0][3] == p['ascending']
    assert totals['processing'] != totals['last_two_first'] and totals['processing'] != totals['outer_two_first']
    assert pr.add_stats(ims, list(qc.CATS))[0][3] == totals['processing']


def test_pq_average_by_hand():
    """evaluation.pq_average and parse_pq_results on statistics whose averages are worked out by hand here (tests/_pq_ref.py's
    pq_average is the same restatement, so the comparisons elsewhere do not check it): three counted thing categories with
    fp / fn > 0, one of them without a TP, an empty thing category and an empty stuff group"""
    from rsprompter_amd.evaluation import parse_pq_results, pq_results
    cats = {0: dict(isthing=1), 1: dict(isthing=1), 2: dict(isthing=1), 5: dict(isthing=1), 3: dict(isthing=0)}
    stat = {0: (2, 1, 1, 1.5), 1: (0, 2, 0, 0.0), 2: (1, 0, 3, 0.75), 5: (0, 0, 0, 0.0), 3: (0, 0, 0, 0.0)}
    res = pq_results(stat, cats)
    # category 0: pq 1.5 / 3 = 0.5, sq 1.5 / 2 = 0.75, rq 2 / 3;  1: 0, 0, 0 / 1 = 0 (counted);  2: pq 0.75 / 2.5 = 0.3, sq 0.75, rq 1 / 2.5 = 0.4
    assert res['classwise'] == {0: dict(pq=0.5, sq=0.75, rq=2 / 3), 1: dict(pq=0.0, sq=0, rq=0.0), 2: dict(pq=0.75 / 2.5, sq=0.75, rq=1 / 2.5),
                                5: dict(pq=0.0, sq=0.0, rq=0.0), 3: dict(pq=0.0, sq=0.0, rq=0.0)}
    want = dict(pq=((0.5 + 0.0) + 0.75 / 2.5) / 3, sq=((0.75 + 0) + 0.75) / 3, rq=((2 / 3 + 0.0) + 1 / 2.5) / 3, n=3)
    assert res['All'] == want and res['Things'] == want and res['Stuff'] == dict(pq=0.0, sq=0.0, rq=0.0, n=0)
    nine = parse_pq_results(res)
    assert nine['PQ'] == 100 * want['pq'] and nine['SQ_th'] == 100 * want['sq'] and nine['RQ'] == 100 * want['rq'] and nine['PQ_st'] == 0.0
    assert abs(nine['PQ'] - 26.666666666666668) < 1e-12 and abs(nine['SQ'] - 50.0) < 1e-12      # 0.8 / 3 and 1.5 / 3


@pytest.mark.parametrize('shape', qc.GEN_SHAPES, ids=lambda s: '%dx%d' % s[:2])
def test_generated_on_the_emulator(emu, shape):
    qc.check_generated(emu, CPU, shape)


def test_noise_on_the_emulator(emu):
    qc.check_noise(emu, CPU)


@pytest.mark.parametrize('check', qc.HAND_CHECKED, ids=lambda f: f.__name__[6:])
def test_hand_checked_on_the_emulator(emu, check):
    check(emu, CPU)


@pytest.mark.parametrize('P', (70, 1024))
def test_many_segments_on_the_emulator(emu, P):
    qc.check_many_segments(emu, CPU, P)


def test_refusals_on_the_emulator(emu):
    qc.check_refusals(emu, CPU, 'meta')                             # the meta device stands in for "another device"


# --------------------------------------------------------------------------------------------------------------- host layers
CLASSES = ('a', 'b', 'c', 'd')
META = dict(classes=CLASSES, thing_classes=CLASSES[:3], stuff_classes=CLASSES[3:])
REF_CATS = {i: dict(isthing=1 if i < 3 else 0) for i in range(4)}


@pytest.fixture(scope='module')
def images(tmp_path_factory):
    """three generated images: (pan, gt, segments with areas listed, the gt PNG's path)"""
    from PIL import Image
    root = tmp_path_factory.mktemp('pq_gt')
    out = []
    for k, seed in enumerate((3, 4, 5)):
        pan, gt, segments = qc.generate(37, 53, 12, seed)
        for s in segments:
            s['area'] = int((gt == s['id']).sum())
        path = os.path.join(root, f'im{k}.png')
        Image.fromarray(pr.id2rgb(gt), 'RGB').save(path)
        out.append((pan, gt, segments, path))
    return root, out


def _sample(k, pan, **extra):
    return dict(img_id=100 + k, img_path=f'somewhere/im{k}.jpg', ori_shape=pan.shape,
                pred_panoptic_seg=dict(sem_seg=torch.from_numpy(pan)[None]), **extra)


def _expected(images, cats=REF_CATS, **kw):
    ims = [qc.reference(pan, gt, segments, cats=cats, **kw) for pan, gt, segments, _ in images]
    return pr.add_stats(ims, list(cats)), pr.nine_keys(pr.add_stats(ims, list(cats)), cats)


def _metric(**kw):
    from rsprompter_amd.evaluation import METRICS, CocoPanopticMetric
    assert METRICS.get('CocoPanopticMetric') is CocoPanopticMetric
    m = METRICS.build(dict(type='CocoPanopticMetric', device='cpu', **kw))
    m.dataset_meta = META
    return m


def test_metric_from_memory_and_from_the_dataset_path(emu, images):
    """gt_panoptic + segments_info (JSON form), and the data sample's segments_info (id, category, is_thing) with
    seg_map_path, areas counted: the nine keys == the reference's, under the prefix, and the per-image rows only"""
    root, ims = images
    _, want = _expected(ims)
    m = _metric()
    m.process(None, [_sample(k, pan, gt_panoptic=torch.from_numpy(gt), segments_info=segments) for k, (pan, gt, segments, _) in enumerate(ims)])
    assert len(m.results) == 3 and set(m.results[0]['row']) == {'tp', 'fp', 'fn', 'iou', 'status'}
    got = m.evaluate(3)
    assert list(got) == ['coco_panoptic/' + k for k in ('PQ', 'SQ', 'RQ', 'PQ_th', 'SQ_th', 'RQ_th', 'PQ_st', 'SQ_st', 'RQ_st')]
    assert {k.split('/')[1]: v for k, v in got.items()} == want and m.results == [] and want['PQ'] > 0
    assert 'Panoptic Evaluation Results' in m.table and 'Classwise' not in m.table
    d = _metric(prefix='val', seg_prefix=str(root))
    for k, (pan, gt, segments, path) in enumerate(ims):
        info = [dict(id=s['id'], category=s['category_id'], is_thing=s['category_id'] < 3 and not s['iscrowd']) for s in segments]
        d.process(None, [_sample(k, pan, segments_info=info, **(dict(seg_map_path=path) if k else {}))])   # k == 0: seg_prefix / name
    got = d.evaluate(3)
    assert {k.split('/')[1]: v for k, v in got.items()} == want and all(k.startswith('val/') for k in got)


def test_metric_with_an_ann_file(emu, images, tmp_path):
    """ann_file + seg_prefix: the JSON's segments_info and areas, the PNG read by PIL; category ids 10 .. 40 in an order
    that is not the classes', and a category no class has"""
    root, ims = images
    cat_of = {0: 30, 1: 10, 2: 40, 3: 20}                          # label (the JSON's order of the names) -> id
    cats = [dict(id=10, name='b', isthing=1), dict(id=50, name='zz', isthing=1), dict(id=20, name='d', isthing=0),
            dict(id=30, name='a', isthing=1), dict(id=40, name='c', isthing=1)]
    # get_cat_ids keeps the JSON's order: label 0 -> 10, 1 -> 20, 2 -> 30, 3 -> 40 (the reference's quirk)
    l2c = {0: 10, 1: 20, 2: 30, 3: 40}
    anns, with_ids = [], []
    for k, (pan, gt, segments, _) in enumerate(ims):
        segs = [dict(s, category_id=cat_of[s['category_id']]) for s in segments]
        anns.append(dict(image_id=100 + k, file_name=f'im{k}.png', segments_info=segs))
        with_ids.append((pan, gt, segs, None))
    ann = os.path.join(tmp_path, 'ann.json')
    with open(ann, 'w') as f:
        json.dump(dict(categories=cats, images=[dict(id=100 + k, file_name=f'im{k}.jpg') for k in range(3)], annotations=anns), f)
    ref_cats = {c['id']: dict(isthing=c['isthing']) for c in cats}
    stat, want = _expected(with_ids, cats=ref_cats, l2c=l2c)
    m = _metric(ann_file=ann, seg_prefix=str(root), classwise=True)
    m.process(None, [_sample(k, pan) for k, (pan, _, _, _) in enumerate(ims)])
    got = m.compute_metrics(m.results)
    assert got == want and m.pq_stat == {c: tuple(v) for c, v in stat.items()} and m.pq_stat[50] == (0, 0, 0, 0.0)
    assert list(m.classwise_results) == list(CLASSES) and 'Classwise Panoptic Evaluation Results' in m.table
    assert m.pq_results['All']['n'] == sum(1 for v in stat.values() if v[0] + v[1] + v[2])


def test_a_group_without_a_counted_category_is_zero(emu):
    """every RSPrompter dataset: no stuff class, so the Stuff group has n = 0 -> 0.0 (panopticapi would divide by zero)"""
    m = _metric()
    m.dataset_meta = dict(classes=('building',), thing_classes=('building',))
    pan = np.array([[1000, 1000, 1, 1]], dtype=np.int32)
    m.process(None, [_sample(0, pan, gt_panoptic=np.array([[7, 7, 0, 0]]), segments_info=[qc.seg(7, 0)])])
    got = m.compute_metrics(m.results)
    assert (got['PQ'], got['SQ'], got['RQ']) == (100.0, 100.0, 100.0) and (got['PQ_th'], got['PQ_st'], got['SQ_st'], got['RQ_st']) == (100.0, 0.0, 0.0, 0.0)
    assert m.pq_results['Stuff'] == dict(pq=0.0, sq=0.0, rq=0.0, n=0) and m.pq_results['Things']['n'] == 1
    assert _metric().compute_metrics([]) == dict.fromkeys(('PQ', 'SQ', 'RQ', 'PQ_th', 'SQ_th', 'RQ_th', 'PQ_st', 'SQ_st', 'RQ_st'), 0.0)


def test_a_refused_image_is_named(emu, tmp_path):
    m = _metric()
    pan = np.array([[0, 1000]], dtype=np.int32)                    # id 0 with label 0 a class: it collides with VOID
    m.process(None, [_sample(4, pan, gt_panoptic=np.array([[7, 7]]), segments_info=[qc.seg(7, 0)])])
    with pytest.raises(RuntimeError, match=r"im4\.png.*pred_id_zero"):
        m.compute_metrics(m.results)
    # format_only returns before that check: the refusal comes when the image would be written, and no file is
    prefix = os.path.join(tmp_path, 'out', 'res')
    f = _metric(outfile_prefix=prefix, format_only=True)
    with pytest.raises(RuntimeError, match=r"im4\.png.*pred_id_zero"):
        f.process(None, [_sample(4, pan, gt_panoptic=np.array([[7, 7]]), segments_info=[qc.seg(7, 0)])])
    assert f.results == [] and not os.path.exists(os.path.join(prefix + '.panoptic', 'im4.png'))
    with pytest.raises(RuntimeError):
        _metric(file_client_args=dict())
    with pytest.raises(NotImplementedError):
        _metric(backend_args=dict(backend='petrel'))


def test_format_only_writes_the_maps(emu, images, tmp_path):
    """outfile_prefix / format_only: <prefix>.panoptic/<name>.png read back by PIL is the map with void as 0, the JSON lists
    the segments of np.unique with their areas; with outfile_prefix alone the numbers are still the device's"""
    from PIL import Image
    root, ims = images
    prefix = os.path.join(tmp_path, 'out', 'res')
    m = _metric(outfile_prefix=prefix, format_only=True)
    m.process(None, [_sample(k, pan, gt_panoptic=torch.from_numpy(gt), segments_info=segments) for k, (pan, gt, segments, _) in enumerate(ims)])
    assert m.evaluate(3) == {}
    with open(prefix + '.panoptic.json') as f:
        anns = json.load(f)['annotations']
    for k, (pan, gt, segments, _) in enumerate(ims):
        back = pr.rgb2id(np.array(Image.open(os.path.join(prefix + '.panoptic', f'im{k}.png')).convert('RGB')))
        assert (back == pr.void_mapped(pan, qc.NC)).all()
        want = qc.reference(pan, gt, segments)['segments']
        assert anns[k]['image_id'] == 100 + k and anns[k]['file_name'] == f'im{k}.png'
        assert [(s['id'], s['category_id'], s['area']) for s in anns[k]['segments_info']] == want
        assert [s['isthing'] for s in anns[k]['segments_info']] == [1 if c < 3 else 0 for _, c, _ in want]
    _, want9 = _expected(ims)
    m2 = _metric(outfile_prefix=os.path.join(tmp_path, 'out2', 'res'))
    m2.process(None, [_sample(k, pan, gt_panoptic=torch.from_numpy(gt), segments_info=segments) for k, (pan, gt, segments, _) in enumerate(ims)])
    assert m2.compute_metrics(m2.results) == want9


def test_apis_panoptic_quality_and_write_png(emu, images, tmp_path):
    from PIL import Image
    from rsprompter_amd import apis
    from rsprompter_amd.structures import PixelData
    root, ims = images
    stat, want = _expected(ims)
    got = apis.panoptic_quality([torch.from_numpy(pan) for pan, _, _, _ in ims],
                                [torch.from_numpy(pr.id2rgb(gt)) if k == 1 else torch.from_numpy(gt) for k, (_, gt, _, _) in enumerate(ims)],
                                [segments for _, _, segments, _ in ims], CLASSES, CLASSES[:3])
    assert {k: got[k] for k in want} == want
    assert {c: [v['tp'], v['fp'], v['fn'], v['iou']] for c, v in got['classwise'].items()} == {CLASSES[c]: v for c, v in stat.items()}
    assert got['n']['Stuff'] == (1 if sum(stat[3][:3]) else 0)
    with pytest.raises(ValueError):
        apis.panoptic_quality([], [], [], CLASSES)
    pan = torch.tensor([[4, 1004, 70001, 3]], dtype=torch.int32)
    path = os.path.join(tmp_path, 'deep', 'x.png')
    rgb = apis.write_panoptic_png(PixelData(sem_seg=pan[None], void=4), path)
    assert (np.array(Image.open(path)) == rgb).all() and pr.rgb2id(rgb).tolist() == [[0, 0, 70001, 3]]
    assert pr.rgb2id(apis.write_panoptic_png(pan, path, void=(4, 3))).tolist() == [[0, 0, 70001, 0]]
    with pytest.raises(ValueError, match='void'):
        apis.write_panoptic_png(pan, path)
    with pytest.raises(ValueError):
        apis.write_panoptic_png(pan.float(), path, void=4)
