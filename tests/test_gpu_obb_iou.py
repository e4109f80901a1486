"""-m gpu: oriented-box comparison on the device (csrc/obb_iou.hip; ops.obb_corners / obb_iou / obb_nms,
rle.runs_to_obb_corners, apis.obb_iou / nms_rotated, large_image merge_nms_type='nms_rotated', CocoMetric metric='obb';
DESIGN §14.17).  The case bodies are tests/_obb_iou_cases.py, the same the emulator tier runs: exact answers ==, everything
else within cases.BOUND of the exact reference in fractions (tests/_obb_iou_ref.py), keep lists and dtm equal to the
reference's on the exact IoUs.  On top of them: rectangles the device made from masks, at the scene's far corner."""
import os
import sys
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _obb_iou_cases as cases  # noqa: E402
import _obb_iou_ref as ref  # noqa: E402

SCENE = os.path.join(HERE, 'golden', 'large_image', 'large_image.jpg')
PAD = (0.406 * 255, 0.456 * 255, 0.485 * 255)


# ------------------------------------------------------------------------------------------------------- the case module
def test_exact_answers(dev):
    from rsprompter_amd import ops
    assert cases.check_exact_table(ops, dev) > 100


def test_every_family_within_the_bound(dev):
    from rsprompter_amd import ops
    worst = cases.check_families(ops, dev)
    print({k: f'{v:.3e}' for k, v in worst.items()}, 'BOUND', cases.BOUND)


def test_unit_shapes(dev):
    from rsprompter_amd import ops
    print(cases.check_unit_shapes(ops, dev))


def test_corners_are_bit_equal_with_obb_to_numpy(dev):
    from rsprompter_amd import ops, rle
    assert cases.check_corners(ops, rle, dev) > 40


def test_nms_sizes_across_mask_word_edges(dev):
    from rsprompter_amd import ops
    print(cases.check_nms_sizes(ops, dev))


@pytest.mark.parametrize('n', cases.NMS_GRID_SIZES)
def test_nms_grid_beyond_one_removal_word_a_lane(dev, n):
    """65 and 258 mask words: a second removal word per lane, and the large form of the walk (the keep lists are the
    construction's, pinned to the exact reference at n = 260 by tests/test_obb_iou_cpu.py)"""
    from rsprompter_amd import ops
    print(n, cases.check_nms_grid(ops, dev, n))


def test_nms_rules(dev):
    from rsprompter_amd import ops
    cases.check_nms_rules(ops, dev)


def test_bad_arguments_are_refused(dev):
    from rsprompter_amd import ops
    cases.check_refusals(ops, dev, pytest)
    if dev.type == 'cuda':                                   # (the emulated developer mode takes host tensors by design)
        cases.check_refuses_host_tensors(ops, pytest)


def test_obb_iou_and_nms_rotated_on_every_input_form(dev):
    from rsprompter_amd import apis, rle
    cases.check_api(apis, rle, dev)
    cases.check_api_refusals(apis, dev, pytest)


def test_two_ships_moored_side_by_side(dev):
    from rsprompter_amd import large_image as li
    cases.check_bars(li, dev)
    cases.check_pipeline_refusals(li, dev, pytest)


def test_metric_obb_against_the_restated_cocoeval(dev, tmp_path):
    from rsprompter_amd import apis, evaluation
    print(cases.check_metric(evaluation, apis, dev, tmp_path))
    cases.check_metric_tie(evaluation, dev)


# ---------------------------------------------------------------------------------------------------------------- scale
def _sample_pairs(quads, k, seed):
    """k pairs (i, j), i != j, of boxes whose axis-aligned bounds overlap where there are that many, random ones beyond"""
    q = np.where(np.isnan(quads), 0.0, quads)                # (an empty mask's NaN row: a point, overlapping nothing)
    lo, hi = q.min(1), q.max(1)
    hit = (hi[:, None, 0] > lo[None, :, 0]) & (hi[None, :, 0] > lo[:, None, 0]) & \
        (hi[:, None, 1] > lo[None, :, 1]) & (hi[None, :, 1] > lo[:, None, 1])
    np.fill_diagonal(hit, False)
    rng = np.random.default_rng(seed)
    pairs = np.argwhere(hit)
    pairs = pairs[rng.permutation(len(pairs))[:k]]
    extra = rng.integers(0, len(quads), (max(k - len(pairs), 0), 2))
    return np.concatenate([pairs, extra], 0)


def _check_against_exact(ops, dev, quads_d, scores, labels, thr, what):
    """IoU of a fixed sample of 2 000 pairs within the bound of the exact reference; NMS equal to the reference's"""
    quads = quads_d.cpu().numpy()
    pairs = _sample_pairs(quads, 2000, 7)
    a, b = quads_d[torch.from_numpy(pairs[:, 0]).to(dev)], quads_d[torch.from_numpy(pairs[:, 1]).to(dev)]
    n = len(pairs)
    got = ops.obb_iou(cases.pair_units(ops, dev, n), n, a.contiguous(), b.contiguous(),
                      torch.zeros(n, dtype=torch.uint8, device=dev)).cpu().tolist()
    exact = [ref.exact_iou(quads[i], quads[j]) for i, j in pairs.tolist()]
    worst = cases.assert_within_bound(got, exact, what)
    live = sum(1 for e in exact if e > 0)
    iou = ref.exact_iou_matrix(quads, quads)
    assert cases.decision_margin(iou, (thr,)) > Fraction(cases.DECISION_MARGIN)
    s, lab = scores.astype(np.float32), labels.astype(np.int32)
    for agnostic in (False, True):
        want = ref.nms(quads, s, lab, thr, agnostic, iou)
        keep = ops.obb_nms(quads_d, torch.from_numpy(s).to(dev), torch.from_numpy(lab).to(dev), thr, class_agnostic=agnostic)
        assert keep.cpu().tolist() == want, (what, agnostic)
    print(f'{what}: {n} pairs, {live} intersecting, worst |device - exact| {worst:.3e} (bound {cases.BOUND:.3e}); '
          f'NMS keeps {len(want)} of {len(quads)}')
    return live, len(want)


def test_noise_256_rectangles_against_the_exact_reference(dev):
    """the rectangles of 256 x 256 noise masks nearly coincide (the whole canvas, give or take a pixel): the family that
    breaks an intersection that is not a closed polygon"""
    from rsprompter_amd import ops, rle
    rng = np.random.default_rng(256)
    dens = np.concatenate([np.geomspace(0.0005, 0.5, 44), [0.0, 1.0, 0.00005, 0.0001]])
    masks = np.stack([rng.random((256, 256)) < d for d in dens])
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(masks).to(dev))
    quads = rle.runs_to_obb_corners(counts, n, (256, 256))
    assert cases.same_doubles(quads, rle.obb_to_numpy(*rle.runs_to_obb(counts, n, (256, 256))[3:], 'corners'))
    live, kept = _check_against_exact(ops, dev, quads, rng.random(48), rng.integers(0, 2, 48), 0.5, 'noise 256')
    assert live > 1500 and kept < 40


def test_300_tile_instances_shifted_into_a_scene(dev):
    """the 300 tile instances of DESIGN §14.9 at integer offsets near the far corner of an 8 192 x 9 000 scene, close enough
    to overlap: rectangles by rsp_obb_corners' offset, IoU and NMS against the exact reference"""
    from scipy import ndimage
    from rsprompter_amd import ops, rle
    rng = np.random.default_rng(300)
    th, tw, H, W, k = 128, 128, 8192, 9000, 300
    f = ndimage.gaussian_filter(rng.random((k, th, tw)), (0, 3, 3))
    tiles = f > np.quantile(f, 0.55)
    tiles[7], tiles[8] = True, False                                               # a full and an empty tile mask
    offs = np.stack([rng.integers(W - 1900, W - tw + 1, k), rng.integers(H - 1600, H - th + 1, k)], 1).astype(np.int32)
    offs[1] = (W - tw, H - th)
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(tiles).to(dev))
    off_d = torch.from_numpy(offs).to(dev)
    quads = rle.runs_to_obb_corners(counts, n, (th, tw), off_d)
    sc, sn, _, _ = rle.shift_runs(counts, n, off_d, (th, tw), (H, W))
    assert cases.same_doubles(quads, rle.obb_to_numpy(*rle.runs_to_obb(sc, sn, (H, W))[3:], 'corners'))
    assert bool(torch.isnan(quads[8]).all())
    live, kept = _check_against_exact(ops, dev, quads, (rng.integers(1, 100, k) / 100.0), rng.integers(0, 3, k), 0.25,
                                      '300 tile instances')
    assert live > 1000 and kept < k


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def model(dev):
    import rsprompter_amd as ra
    from rsprompter_amd.config import Config
    from rsprompter_amd.default_configs import rsprompter_anchor
    from rsprompter_amd.synth import synth_state_dict
    cfg = Config(dict(
        model=rsprompter_anchor('base', 10),
        test_dataloader=dict(dataset=dict(pipeline=[
            dict(type='LoadImageFromFile', backend_args=None, to_float32=True),
            dict(type='Resize', scale=(1024, 1024), keep_ratio=True),
            dict(type='Pad', size=(1024, 1024), pad_val=dict(img=PAD, masks=0)),
            dict(type='PackDetInputs', meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor'))]))))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = ra.build_model(cfg)
    m.load_state_dict(synth_state_dict(m, seed=0), strict=True)
    m.cfg = cfg
    return m.to(dev)


def test_demo_scene_merged_by_rotated_nms(dev, model):
    """inference_large_image on a 512 x 896 window of the committed scene (two 512-pixel tiles that share a quarter) with seeded
    synthetic weights in the new mode: keep is the reference NMS on the exact IoUs of the tile instances' rectangles, more
    than one instance stays, and everything downstream of keep is the 'nms' branch"""
    from rsprompter_amd import ops, rle
    from rsprompter_amd.apis import TestPipeline
    from rsprompter_amd.large_image import inference_large_image
    scene = np.ascontiguousarray(TestPipeline._decode(SCENE)[:512, :896])
    out, patches, start = inference_large_image(model, scene, patch_size=512, batch_size=2, merge_iou_thr=0.25,
                                                merge_nms_type='nms_rotated', return_patches=True)
    assert start == [(0, 0), (384, 0)]
    masks = torch.cat([p.pred_instances.masks for p in patches], 0).to(torch.bool)
    scores = torch.cat([p.pred_instances.scores for p in patches], 0)
    labels = torch.cat([p.pred_instances.labels for p in patches], 0)
    cnt = [len(p.pred_instances.scores) for p in patches]
    off = torch.tensor([list(s) for s, c in zip(start, cnt) for _ in range(c)], dtype=torch.int32, device=dev).view(-1, 2)
    counts, n, _, _ = rle.encode_runs(masks)
    quads = rle.runs_to_obb_corners(counts, n, tuple(masks.shape[1:]), off).cpu().numpy()
    iou = ref.exact_iou_matrix(quads, quads)
    assert cases.decision_margin(iou, (0.25,)) > Fraction(cases.DECISION_MARGIN)
    want = ref.nms(quads, scores.cpu().numpy(), labels.cpu().numpy(), 0.25, False, iou)
    K = len(want)
    assert out.keep.cpu().tolist() == want and 1 < K <= len(quads)
    p = out.pred_instances
    keep = out.keep
    assert torch.equal(p.scores, scores[keep]) and torch.equal(p.labels, labels[keep]) and len(p.masks) == K
    boxes = torch.cat([q.pred_instances.bboxes for q in patches], 0) + torch.cat([off, off], 1).to(torch.float32)
    assert torch.equal(p.bboxes, boxes[keep]) and p.bboxes.shape[1] == 4                     # axis-aligned, as before
    plain = ops.nms_flat(boxes, scores, labels, 0.25)
    print(f'{len(quads)} tile instances: nms_rotated keeps {K}, nms keeps {int(plain.shape[0])}')
