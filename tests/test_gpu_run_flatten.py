"""-m gpu: planar instance layers on the device (csrc/run_flatten.hip, ops.rle_flatten / rle_label_map, rle.flatten_runs /
runs_to_labels, apis.flatten_masks / masks_to_label_map, inference_large_image(flatten=...)).  The case bodies
are tests/_run_flatten_cases.py, the same the emulator tier runs, against the dense numpy oracle of
tests/_run_flatten_ref.py; the scale case is checked against a dense torch argmin on the device.  Everything is ==."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _run_flatten_cases as cases  # noqa: E402
from test_gpu_coco_iou_runs import SCENE_DIR, SCENE_HW, model  # noqa: E402,F401


# -------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.quick
def test_hand_checked_masks(dev):
    from rsprompter_amd import ops, rle
    cases.check_hand_checked(ops, rle, dev)


@pytest.mark.quick
def test_tied_scores_and_the_area_order(dev):
    from rsprompter_amd import apis
    cases.check_tied_scores(apis, dev)


@pytest.mark.quick
def test_wave_and_chunk_boundaries(dev):
    from rsprompter_amd import ops
    cases.check_wave_boundaries(ops, dev)


@pytest.mark.quick
def test_non_canonical_counts(dev):
    from rsprompter_amd import ops
    cases.check_non_canonical(ops, dev)


@pytest.mark.quick
def test_300_seeded_random_cases_every_input_and_output_form(dev):
    from rsprompter_amd import apis
    cases.check_random(apis, dev)


@pytest.mark.quick
def test_protocol_poison_capacity_retry_reads_and_second_launch(dev):
    from rsprompter_amd import ops, rle
    cases.check_protocol(ops, rle, dev)


@pytest.mark.quick
def test_refusals(dev, monkeypatch):
    from rsprompter_amd import apis, ops, rle
    cases.check_refusals(ops, rle, apis, dev, pytest, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- scale
def test_64_blobs_on_1024_x_1024_against_a_dense_argmin_on_the_device(dev):
    """64 discs of radius 100 .. 180 on 1024 x 1024 (each overlaps its neighbours; a pixel is covered up to ~10 deep), a
    random rank: flatten_masks and the label map against argmin over [64, 1024, 1024] in torch"""
    from rsprompter_amd import apis
    g = torch.Generator().manual_seed(64)
    k, S = 64, 1024
    cy, cx = torch.rand(k, generator=g) * S, torch.rand(k, generator=g) * S
    r = 100 + 80 * torch.rand(k, generator=g)
    yy, xx = torch.arange(S, device=dev).view(1, S, 1), torch.arange(S, device=dev).view(1, 1, S)
    masks = (yy - cy.to(dev).view(k, 1, 1)) ** 2 + (xx - cx.to(dev).view(k, 1, 1)) ** 2 < r.to(dev).view(k, 1, 1) ** 2
    rank = torch.randperm(k, generator=g)
    area = masks.view(k, -1).sum(1)
    pair = (masks.view(k, 1, -1)[:, :, ::16] & masks.view(1, k, -1)[:, :, ::16]).sum(2)
    assert float((pair.sum() - pair.diagonal().sum())) / float(pair.diagonal().sum()) > 0.3    # overlap: > 30 % of the areas
    cost = torch.where(masks, rank.to(dev).view(k, 1, 1), k)
    win = cost.argmin(0)
    want = masks & (win[None] == torch.arange(k, device=dev).view(k, 1, 1))
    got, info = apis.flatten_masks(masks, order=rank.numpy(), device=dev)
    assert got.dtype == torch.bool and torch.equal(got, want)
    assert torch.equal(info['area_before'].to(torch.int64), area) and torch.equal(info['area_after'].to(torch.int64), want.view(k, -1).sum(1))
    assert int(info['area_after'].sum()) == int(masks.any(0).sum())
    ids = torch.arange(100, 100 + k, dtype=torch.int32)
    lab = apis.masks_to_label_map(masks, order=rank.numpy(), ids=ids, device=dev)
    want_lab = torch.where(masks.any(0), ids.to(dev)[win], torch.zeros((), dtype=torch.int32, device=dev))
    assert lab.dtype == torch.int32 and torch.equal(lab, want_lab)


# ---------------------------------------------------------------------------------------------------------- integration
def _scene(model, **kw):  # noqa: F811
    from rsprompter_amd import apis
    s = apis.inference_large_image(model, os.path.join(SCENE_DIR, 'large_image.jpg'), patch_size=640, batch_size=2, **kw)
    assert s.ori_shape == SCENE_HW
    return s.pred_instances


@pytest.mark.parametrize('merge', ['nms', 'seam_mask'])
@pytest.mark.parametrize('region', [0, 100])
def test_inference_large_image_flatten_gives_a_planar_layer(dev, model, merge, region):  # noqa: F811
    """the committed scene, synthetic weights (the detections are noise that overlaps freely; under 'seam_mask' nearly all of
    them chain into one instance, so the stub test below carries that branch with K > 1): cases.check_scene_pair"""
    kw = dict(merge_nms_type=merge, min_mask_region_area=region, **(dict(seam_iou_thr=0.9) if merge == 'seam_mask' else {}))
    plain, flat = _scene(model, **kw), _scene(model, flatten='score', **kw)
    K = cases.check_scene_pair(dev, plain, flat, region, overlapping=merge == 'nms')
    print(f'{merge}, region {region}: {K} instances')
    assert K > 1 or merge == 'seam_mask'


@pytest.mark.quick
@pytest.mark.parametrize('merge', ['nms', 'seam_mask'])
@pytest.mark.parametrize('region', [0, 6])
def test_inference_large_image_flatten_around_a_random_stub_detector(dev, merge, region):
    from rsprompter_amd import large_image as li
    assert cases.check_pipeline(li, dev, cases.seam_cases.RandomStub((32, 32)).to(dev), merge, region) >= 10


def test_inference_large_image_flatten_polygons_cover_the_union_once(dev, model):  # noqa: F811
    """masks='polygons' with flatten='area': the doubled ring areas of all instances (holes negative) sum to twice the area
    of the union of the unflattened masks"""
    from rsprompter_amd import ops, rle
    plain = _scene(model)
    flat = _scene(model, masks='polygons', flatten='area')
    K = len(plain.scores)
    assert len(flat.masks) == K > 1
    area2 = sum(int(a2) for inst in flat.masks for _, _, a2 in inst)
    c, n, size, _ = rle.masks_to_runs(plain.masks, dev, 'test')
    members = torch.arange(K, dtype=torch.int32, device=c.device)
    offs = torch.tensor([0, K], dtype=torch.int32, device=c.device)
    uc, un, _, _ = rle.union_runs(c, n, size, offs, members)
    union = int(ops.rle_bbox(uc, un, *size)[1][0])
    assert area2 == 2 * union and union > 0
    assert int(flat.flatten_area[:, 1].sum()) == union
