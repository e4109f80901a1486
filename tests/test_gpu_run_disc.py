"""-m gpu: Euclidean buffers in the run domain on the device (csrc/run_disc.hip, ops.rle_dilate_disc / rle_erode_disc /
rle_minus, rle.half_heights / *_runs(element=...) / buffer_runs, apis.mask_morphology(element=...) / buffer_masks,
inference_large_image(buffer=...)).  The case bodies are tests/_run_disc_cases.py, the same the emulator tier
runs, against the dense numpy oracle of tests/_run_disc_ref.py; one check is scene-sized here.  Everything is ==."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _large_image_ref as lref  # noqa: E402
import _run_disc_cases as cases  # noqa: E402
import _run_disc_ref as dref  # noqa: E402
from test_gpu_coco_iou_runs import SCENE_DIR, SCENE_HW, model  # noqa: E402,F401


# -------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.quick
def test_hand_checked_masks(dev):
    from rsprompter_amd import ops
    cases.check_hand_checked(ops, dev)


@pytest.mark.quick
def test_the_pruning_comb_checkerboard_staircase_notch_and_edges(dev):
    from rsprompter_amd import ops
    cases.check_pruning(ops, dev)


@pytest.mark.quick
def test_list_and_wave_boundaries(dev):
    from rsprompter_amd import ops
    cases.check_list_boundaries(ops, dev)


@pytest.mark.quick
def test_non_canonical_counts(dev):
    from rsprompter_amd import ops
    cases.check_non_canonical(ops, dev)


@pytest.mark.quick
def test_diamond(dev):
    from rsprompter_amd import apis, ops, rle
    cases.check_diamond(ops, rle, apis, dev)


def test_240_seeded_random_masks_every_operation_every_form(dev):
    from rsprompter_amd import apis, ops
    cases.check_random(ops, apis, dev)


@pytest.mark.quick
def test_buffer_masks(dev):
    from rsprompter_amd import apis
    cases.check_buffer_masks(apis, dev)


@pytest.mark.quick
def test_protocol_capacities_reads_chunks_and_second_launch(dev, monkeypatch):
    from rsprompter_amd import ops, rle
    cases.check_protocol(ops, rle, dev, monkeypatch)


@pytest.mark.quick
def test_refusals(dev):
    from rsprompter_amd import apis, ops, rle
    cases.check_refusals(ops, rle, apis, dev, pytest)


# ---------------------------------------------------------------------------------------------------------------- scale
def test_three_instances_on_8192_x_9000_against_the_oracle_on_their_grown_boxes(dev):
    """r2 = 14^2 on the scene canvas: a blob in the middle, one in the top left corner, one in the bottom right corner;
    dilation and erosion (both borders) against the oracle on each instance's bounding box grown by R"""
    from rsprompter_amd import ops, rle
    H, W, r2 = 8192, 9000, 14 * 14
    rng = np.random.default_rng(8192)
    masks = []
    for (y0, x0), (h, w) in (((4000, 4400), (300, 280)), ((0, 0), (200, 260)), ((H - 240, W - 180), (240, 180))):
        m = np.zeros((H, W), bool)
        m[y0:y0 + h, x0:x0 + w] = ndi.gaussian_filter(rng.standard_normal((h, w)), 16) > 0       # features wider than 2 R
        assert m[y0:y0 + h, x0:x0 + w].any()
        masks.append(m)
    counts, n = cases.rows_from_counts([lref.rle_counts_np(m) for m in masks], dev)
    hh = rle.half_heights('disc', r2=r2, size=(H, W))[0]
    assert len(hh) == 15

    def dense(c, n_host):
        out = []
        for i, m in enumerate(n_host.tolist()):
            row = c[i, :m].cpu().numpy().astype(np.int64)
            assert row.sum() == H * W and (row[1:] > 0).all()
            out.append(np.repeat(np.arange(m) % 2 == 1, row).reshape(W, H).T)
        return out
    c, m, n_host, _ = ops.rle_dilate_disc(counts, n, H, W, hh)
    for got, mask in zip(dense(c, n_host), masks):
        assert np.array_equal(got, dref.dilate_cropped(mask, r2))
    for border in (0, 1):
        c, m, n_host, _ = ops.rle_erode_disc(counts, n, H, W, hh, border)
        for i, (got, mask) in enumerate(zip(dense(c, n_host), masks)):
            want = dref.erode_cropped(mask, r2, border)
            assert np.array_equal(got, want), (border, i)
            assert want.any()                                        # of the oracle: the comparison is not one of empties


# ---------------------------------------------------------------------------------------------------------- integration
def _scene(model, **kw):  # noqa: F811
    from rsprompter_amd import apis
    s = apis.inference_large_image(model, os.path.join(SCENE_DIR, 'large_image.jpg'), patch_size=640, batch_size=2, **kw)
    assert s.ori_shape == SCENE_HW
    return s.pred_instances


def test_inference_large_image_buffer_on_the_committed_scene(dev, model):  # noqa: F811
    """buffer=+-2.0 against the oracle applied to the decoded unbuffered result (the oracle on the grown bounding box, for the
    first instances; areas and inclusions for all, compared on the device); buffer=3 with flatten='score' gives pairwise
    disjoint masks whose union is the union of the buffered masks = the buffered union (the weights are synthetic and the
    detections noise)"""
    from rsprompter_amd import rle

    def dense(masks):
        c, n, size, _ = rle.masks_to_runs(masks, dev, 'test')
        return rle.runs_to_dense(c, n, size)
    plain, grown, shrunk = _scene(model), _scene(model, buffer=2.0), _scene(model, buffer=-2.0)
    K = len(plain.scores)
    assert K > 1 and 'buffer_area' not in plain
    base = dense(plain.masks)
    area = lambda t: t.view(K, -1).sum(1).to(torch.int32)                            # noqa: E731
    for out, sign in ((grown, 1), (shrunk, -1)):
        for key in ('bboxes', 'scores', 'labels'):
            assert torch.equal(getattr(plain, key), getattr(out, key))
        got = dense(out.masks)
        assert not ((~got & base) if sign > 0 else (got & ~base)).any()
        assert out.buffer_area.dtype == torch.int32 and torch.equal(out.buffer_area, torch.stack([area(base), area(got)], 1))
        for i in range(min(K, 8)):
            m = base[i].cpu().numpy()
            want = dref.dilate_cropped(m, 4) if sign > 0 else dref.erode_cropped(m, 4, 1)
            assert np.array_equal(got[i].cpu().numpy(), want), (sign, i)
    flat = _scene(model, buffer=3, flatten='score')
    got = dense(flat.masks)
    assert int(got.sum(0, dtype=torch.int32).max()) <= 1
    assert np.array_equal(got.any(0).cpu().numpy(), dref.dilate(base.any(0).cpu().numpy(), 9))
    assert int(flat.buffer_area[:, 1].sum()) >= int(got.sum()) == int(flat.flatten_area[:, 1].sum())


@pytest.mark.quick
@pytest.mark.parametrize('merge', ['nms', 'seam_mask'])
def test_inference_large_image_buffer_around_a_random_stub_detector(dev, merge):
    from rsprompter_amd import large_image as li
    assert cases.check_pipeline(li, dev, cases.mcases.seam_cases.RandomStub((32, 32)).to(dev), merge) >= 10
