"""-m gpu: run-domain mask IoU on the device (csrc/coco_iou_runs.hip, ops.run_prefix / ops.coco_iou_runs,
CocoMetric(iou_domain=...), apis.mask_iou, evaluate(large_image=...)).  The case bodies are
tests/_coco_iou_runs_cases.py, the same the emulator tier runs, against cocoapi's rleIou restated loop by loop
(tests/_cocoeval_ref.py) and against the bits route; the scene set is scene-sized here.  Everything is ==."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _coco_cases as cc  # noqa: E402
import _coco_iou_runs_cases as cases  # noqa: E402
import _cocoeval_ref as ref  # noqa: E402

PAD = (0.406 * 255, 0.456 * 255, 0.485 * 255)
SCENE_DIR = os.path.join(HERE, 'golden', 'large_image')
SCENE_HW = (788, 1400)
# small holes and islands removed from the noise masks of the synthetic weights: a tenth of the runs for the host oracle to read
LARGE_IMAGE = dict(patch_size=640, batch_size=2, min_mask_region_area=100)


# -------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.quick
def test_hand_checked_pairs(dev):
    from rsprompter_amd import ops
    cases.check_hand_checked(ops, dev)


@pytest.mark.quick
def test_wave_and_chunk_boundaries(dev):
    from rsprompter_amd import ops
    cases.check_wave_boundaries(ops, dev)


@pytest.mark.quick
def test_non_canonical_counts(dev):
    from rsprompter_amd import ops
    cases.check_non_canonical(ops, dev)


@pytest.mark.quick
def test_crowd_ground_truths(dev):
    from rsprompter_amd import ops
    cases.check_crowd(ops, dev)


@pytest.mark.quick
def test_unit_geometry(dev):
    from rsprompter_amd import ops
    cases.check_unit_geometry(ops, dev)


@pytest.mark.quick
def test_300_seeded_random_pairs(dev):
    from rsprompter_amd import ops
    cases.check_random_pairs(ops, dev)


@pytest.mark.quick
def test_union_in_64_bits(dev):
    from rsprompter_amd import ops
    cases.check_union_64bit(ops, dev)


@pytest.mark.quick
def test_refusals(dev):
    from rsprompter_amd import ops
    cases.check_refusals(ops, dev, pytest)


# ------------------------------------------------------------------------------------------------------------ metric + API
def test_coco_metric_on_the_nwpu_subset_bits_equals_runs_equals_the_oracle(dev, tmp_path):
    from rsprompter_amd import evaluation
    cases.check_metric_nwpu(evaluation, dev, tmp_path)


def test_coco_metric_on_two_scenes_the_auto_route_and_mask_iou_without_a_bit_plane(dev, tmp_path, monkeypatch):
    from rsprompter_amd import apis, evaluation

    def memory(reset=False):
        torch.cuda.synchronize(dev)
        if reset:
            torch.cuda.reset_peak_memory_stats(dev)
            memory.base = torch.cuda.memory_allocated(dev)
            return 0
        return torch.cuda.max_memory_allocated(dev) - memory.base
    cases.check_metric_scenes(evaluation, apis, dev, tmp_path, [(1536, 2048), (2000, 1200)], monkeypatch, memory)


@pytest.mark.quick
def test_mask_iou_forms_crowds_and_refusals(dev):
    from rsprompter_amd import apis
    cases.check_mask_iou(apis, dev, pytest)


# ---------------------------------------------------------------------------------------------------------------- evaluate
def _model_dict():
    from rsprompter_amd.default_configs import rsprompter_anchor
    return rsprompter_anchor('base', 10)


PIPELINE = [dict(type='LoadImageFromFile', backend_args=None, to_float32=True),
            dict(type='Resize', scale=(1024, 1024), keep_ratio=True),
            dict(type='Pad', size=(1024, 1024), pad_val=dict(img=PAD, masks=0)),
            dict(type='PackDetInputs', meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor'))]


def _cfg_dict(ann_file):
    return dict(model=_model_dict(),
                test_dataloader=dict(batch_size=1, dataset=dict(
                    type='NWPUInsSegDataset', data_root=SCENE_DIR, ann_file=ann_file, data_prefix=dict(img=''),
                    test_mode=True, pipeline=PIPELINE, backend_args=None)),
                test_evaluator=dict(type='CocoMetric', metric=['bbox', 'segm'], format_only=False, backend_args=None))


def _scene_annotations(path):
    """the committed scene with 20 polygon ground truths (16-vertex ellipses) over the ten NWPU classes"""
    rng = np.random.default_rng(71)
    h, w = SCENE_HW
    th = np.linspace(0, 2 * np.pi, 16, endpoint=False)
    anns = []
    for j in range(20):
        cx, cy, rx, ry = rng.uniform(80, w - 80), rng.uniform(80, h - 80), rng.uniform(15, 70), rng.uniform(15, 70)
        poly = np.round(np.stack([cx + rx * np.cos(th), cy + ry * np.sin(th)], 1), 1).reshape(-1).tolist()
        xs, ys = poly[0::2], poly[1::2]
        anns.append(dict(id=j + 1, image_id=7, category_id=1 + j % 10, segmentation=[poly], iscrowd=0,
                         bbox=[min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys)], area=float(np.pi * rx * ry)))
    gt = dict(images=[dict(id=7, height=h, width=w, file_name='large_image.jpg')], annotations=anns,
              categories=[dict(id=i + 1, name=n) for i, n in enumerate(cc.NWPU_CLASSES)])
    path.write_text(json.dumps(gt))
    return str(path)


@pytest.fixture(scope='module')
def model(dev):
    import rsprompter_amd as ra
    from rsprompter_amd.config import Config
    from rsprompter_amd.synth import synth_state_dict
    cfg = Config(_cfg_dict(''))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = ra.build_model(cfg)
    m.load_state_dict(synth_state_dict(m, seed=0), strict=True)
    m.cfg = cfg
    return m.to(dev).eval()


@pytest.fixture(scope='module')
def scene_eval(dev, model, tmp_path_factory):
    """evaluate(large_image=...) once on the committed scene, on the default route of scenes ('runs'), for both tests below"""
    from rsprompter_amd import evaluate as E
    from rsprompter_amd.config import Config
    tmp = tmp_path_factory.mktemp('scene_eval')
    d = _cfg_dict(_scene_annotations(tmp / 'scenes.json'))
    prefix = str(tmp / 'runs' / 'r')
    res = E.evaluate(model, Config(d), out_prefix=prefix, verbose=False, large_image=LARGE_IMAGE)
    m = E.evaluate.last_metric
    assert m.iou_domain == 'runs' == m.timings['segm']['iou_domain']
    return dict(cfg=d, tmp=tmp, prefix=prefix, res=res, metric=m,
                stats={t: m.eval_results[t].stats.copy() for t in ('bbox', 'segm')})


def test_evaluate_large_image_equals_the_oracle_and_the_bits_route(dev, model, scene_eval, monkeypatch):
    """the weights are synthetic and the detections noise; the stats are the oracle's on the written result files all the
    same, and the two routes agree"""
    import time
    from rsprompter_amd import evaluate as E
    from rsprompter_amd.config import Config
    ref.use_numpy_forms()
    monkeypatch.setattr(ref, 'rle_iou', cases.LITERAL_IOU)        # the literal walk skips the pairs rleIou's bbIou skips
    prefix, m = scene_eval['prefix'], scene_eval['metric']
    segm = json.load(open(f'{prefix}.segm.json'))
    assert len(segm) > 0 and all(s['segmentation']['size'] == list(SCENE_HW) for s in segm)
    t0 = time.perf_counter()
    want = {t: ref.coco_stats(m.coco_gt, json.load(open(f'{prefix}.{t}.json')), t)[0] for t in ('bbox', 'segm')}
    t1 = time.perf_counter()
    for t in ('bbox', 'segm'):
        assert np.array_equal(scene_eval['stats'][t], want[t]), (t, scene_eval['stats'][t], want[t])
    assert json.load(open(f'{prefix}.metrics.json')) == scene_eval['res']
    res = E.evaluate(model, Config(scene_eval['cfg']), verbose=False, iou_domain='bits',
                     large_image=LARGE_IMAGE)
    print(f'{len(segm)} detections; the oracle took {t1 - t0:.2f} s, evaluate on the bits route {time.perf_counter() - t1:.2f} s')
    b = E.evaluate.last_metric
    assert b.iou_domain == 'bits' == b.timings['segm']['iou_domain'] and res == scene_eval['res']
    for t in ('bbox', 'segm'):
        assert np.array_equal(b.eval_results[t].stats, scene_eval['stats'][t]), t


def test_cli_large_image_prints_the_summary_of_both_metrics(dev, model, scene_eval, tmp_path):
    """python -m rsprompter_amd.evaluate CONFIG CKPT --large-image in a fresh child process"""
    ckpt = str(tmp_path / 'epoch_1.pth')
    torch.save(dict(meta=dict(epoch=1), state_dict={k: v.cpu() for k, v in model.state_dict().items()}), ckpt)
    (tmp_path / 'cfg.py').write_text(''.join(f'{k} = {v!r}\n' for k, v in scene_eval['cfg'].items()))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'rsprompter_amd.evaluate', str(tmp_path / 'cfg.py'), ckpt, '--large-image',
                        '--patch-size', '640', '--batch-size', '2', '--min-mask-region-area', '100', '--out-prefix', str(tmp_path / 'cli' / 'r')],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert r.stdout.count('Average Precision') == 12 and r.stdout.count('Average Recall') == 12
    assert json.load(open(tmp_path / 'cli' / 'r.metrics.json')) == scene_eval['res']
