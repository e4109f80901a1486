"""-m "not gpu": multi-crop SAM mask generation ("crop layers") without a GPU.  The two new kernels
(rsp_crops_resize_pad, rsp_mask_score_box_crops) run on the lane-level emulator (tests/wave_emu) through the same check
functions as the GPU suite (tests/test_gpu_sam_multicrop.py); `SamMaskGenerator`'s host flow (crop boxes, grids, batching,
filter, near-edge rule, one NMS over all crops, masks in the image frame) runs around a stub decoder on a constructed scene
of discs against HF's helpers composed per crop."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import test_gpu_sam_multicrop as mc  # noqa: E402  (the same checks the GPU runs)

CPU = torch.device('cpu')
EMU_HW, EMU_S = (140, 200), 128
EMU_BOXES = [[0, 0, 200, 140], [40, 10, 168, 106], [100, 12, 177, 140], [120, 60, 200, 140], [0, 0, 90, 70], [30, 20, 130, 100]]


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_feature_is_there():
    from rsprompter_amd import _lib, apis, ops
    assert 'rsp_crops_resize_pad' in _lib.PROTOTYPES and 'rsp_mask_score_box_crops' in _lib.PROTOTYPES
    assert callable(apis.SamMaskGenerator) and callable(ops.crops_resize_pad) and callable(ops.mask_score_box_crops)
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'rsp_hip.h')).read()
    assert 'int rsp_crops_resize_pad(' in hdr and 'int rsp_mask_score_box_crops(' in hdr


def test_crops_resize_pad_on_the_emulator(emu):
    # identity resizes: 128 x 96 and 77 x 128 crops at S = 128; six crops of six sizes in one launch
    mc.check_crops_resize_pad(emu, CPU, EMU_HW, EMU_S, EMU_BOXES)
    mc.check_crops_resize_pad_refusals(emu, CPU)


def test_score_box_crops_kernel_on_the_emulator(emu):
    mc.check_score_crops_kernel(emu, CPU, EMU_HW, EMU_S, EMU_BOXES)
    mc.check_score_crops_kernel(emu, CPU, EMU_HW, EMU_S, EMU_BOXES[:5], per_crop=4, thr=0.5, off=0.25, seed=18)
    mc.check_score_crops_refusals(emu, CPU)


def test_crop_boxes_and_grids_are_hfs():
    from rsprompter_amd.sam_prompts import SamMaskGenerator, generate_crop_boxes
    ip = mc._hf_helpers()
    for hw in ((600, 900), (517, 803), (240, 360), (1024, 1024), (333, 1500)):
        for layers in (0, 1, 2, 3):
            for ratio in (512 / 1500, 0.2):
                assert generate_crop_boxes(layers, ratio, hw) == ip._generate_per_layer_crops(layers, ratio, hw)
    sam = mc.DiscSam(None, CPU, 128, torch.zeros(60, 90, 3, dtype=torch.uint8), [[0, 0, 90, 60]], 3)
    gen = SamMaskGenerator(sam, points_per_side=9, crop_n_layers=2, crop_n_points_downscale_factor=2)
    assert [g.shape[0] for g in gen.grids] == [81, 16, 4]                    # int(9 / 2 ** l) per side
    assert np.array_equal(gen.grids[1], ip._build_point_grid(4))
    assert gen.crop_boxes((517, 803)) == ip._generate_per_layer_crops(2, 512 / 1500, (517, 803))[0]
    # batches: one layer each; the default is capped by the candidates per batch, an explicit crop_batch is taken as given
    layers = [0] + [1] * 4 + [2] * 16
    assert gen._batches(layers) == [(0, 1), (1, 5), (5, 13), (13, 21)]       # unknown encoder width: 8
    gen.crop_batch = 3
    assert gen._batches(layers) == [(0, 1), (1, 4), (4, 5), (5, 8), (8, 11), (11, 14), (14, 17), (17, 20), (20, 21)]
    big = SamMaskGenerator(sam, points_per_side=32, crop_n_layers=2, crop_n_points_downscale_factor=2)
    sam.vision_encoder.D = 1280
    assert big._batches(layers) == [(0, 1), (1, 5), (5, 21)]                 # 4 x 3072 and 16 x 768 candidates: the cap
    sam.vision_encoder.D = 1024
    assert big._batches(layers) == [(0, 1), (1, 5), (5, 13), (13, 21)]
    sam.vision_encoder.D = None
    with pytest.raises(ValueError, match='empty point grid'):
        SamMaskGenerator(sam, points_per_side=4, crop_n_layers=2, crop_n_points_downscale_factor=4)
    with pytest.raises(ValueError):
        SamMaskGenerator(sam, output='png')
    with pytest.raises(ValueError):
        SamMaskGenerator(sam, crop_batch=0)
    with pytest.raises(TypeError):
        SamMaskGenerator(torch.nn.Linear(1, 1))


# the issue's third row (240 x 360, S = 256, 6 x 6 grid, 20 discs at radii x 0.4) scaled by 100 / 240: the same scene geometry at
# the emulator's speed; the stability threshold is lowered to 0.6 (small discs on the coarser 32^2 logits have soft relative
# edges), not the radii further.  With the reference helpers alone: K 240, 0 undecided, 47 removed by the near-edge rule alone,
# 43 kept, 14 instances from 4 of 5 crops, 3 cross-crop suppressions, 2 NaN stabilities.
REDUCED = dict(hw=(100, 150), S=128, layers=1, n=4, ndisc=20, rad_scale=0.2, t_st=0.6)


def test_merge_on_the_disc_scene_on_the_emulator(emu):
    """a reduced case that meets the issue's four conditions on the oracle alone (asserted inside before anything is compared)"""
    o, res = mc.run_merge_case(emu, CPU, **REDUCED)
    assert o['K'] == 5 * 16 * 3


def test_no_crop_layers_is_generate_masks_bit_for_bit(emu):
    from rsprompter_amd.apis import SamMaskGenerator, generate_masks
    hw, S, n = (60, 90), 128, 4
    image = mc._test_image(hw)
    box = [[0, 0, hw[1], hw[0]]]
    kw = dict(points_per_side=n, pred_iou_thresh=0.88, stability_score_thresh=0.5)
    sams = [mc.DiscSam(emu, CPU, S, image, box, 6, 0.25) for _ in range(4)]
    for i, output in enumerate(('rle', 'dense')):
        a = SamMaskGenerator(sams[2 * i], crop_n_layers=0, output=output, **kw).generate(image)
        w = generate_masks(sams[2 * i + 1], image, output=output, **kw)
        assert torch.equal(a.bboxes, w.bboxes) and torch.equal(a.scores, w.scores) and w.bboxes.shape[0] > 1
        assert (a.masks == w.masks) if output == 'rle' else torch.equal(a.masks, w.masks)
        assert a.crop_index.dtype == torch.int64 and not bool(a.crop_index.any())


def test_refusals_and_empty_result(emu):
    from rsprompter_amd import ops
    from rsprompter_amd.apis import SamMaskGenerator, generate_masks
    hw = (60, 90)
    image = mc._test_image(hw)
    boxes = mc._hf_helpers()._generate_per_layer_crops(1, 512 / 1500, hw)[0]
    with pytest.raises(NotImplementedError, match='crop_n_layers'):
        generate_masks(mc.DiscSam(emu, CPU, 128, image, boxes, 6), image, crop_n_layers=1)
    # nothing passes the predicted-IoU filter: empty results of the right shapes
    for output in ('rle', 'dense'):
        res = SamMaskGenerator(mc.DiscSam(emu, CPU, 128, image, boxes, 6, 0.25), points_per_side=2, pred_iou_thresh=2.0,
                               output=output).generate(image)
        assert tuple(res.bboxes.shape) == (0, 4) and tuple(res.scores.shape) == (0,) and tuple(res.crop_index.shape) == (0,)
        assert res.masks == [] if output == 'rle' else tuple(res.masks.shape) == (0, 60, 90)
    with pytest.raises(ValueError):
        SamMaskGenerator(mc.DiscSam(emu, CPU, 128, image, boxes, 6), points_per_side=2).generate(image[:, :, :2])
    # more kept candidates than the NMS holds: refused before the NMS is launched
    saved = ops.NMS_MAX_CANDIDATES
    ops.NMS_MAX_CANDIDATES = 3
    try:
        with pytest.raises(ValueError, match='NMS_MAX_CANDIDATES'):
            SamMaskGenerator(mc.DiscSam(emu, CPU, 128, image, boxes, 6, 0.25), points_per_side=3, pred_iou_thresh=0.0,
                             stability_score_thresh=0.0).generate(image)
    finally:
        ops.NMS_MAX_CANDIDATES = saved
    # an image of 2^31 pixels or more: refused before anything is launched (a zero-stride view, nothing that large is allocated)
    huge = torch.zeros(1, 1, 3, dtype=torch.uint8).expand(1 << 16, 1 << 15, 3)
    with pytest.raises(ValueError, match='2\\^31'):
        SamMaskGenerator(mc.DiscSam(emu, CPU, 128, image, boxes, 6), points_per_side=2).generate(huge)
