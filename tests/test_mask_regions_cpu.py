"""-m "not gpu": `min_mask_region_area` ("small regions") without a GPU.  rsp_mask_remove_small_regions runs on the
lane-level emulator (tests/wave_emu) through the same check functions as the GPU suite (tests/test_gpu_mask_regions.py); the
generator step runs around the stub decoder of the multi-crop tests."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import test_gpu_mask_regions as mr  # noqa: E402  (the same checks the GPU runs)

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_feature_is_there():
    import inspect
    from rsprompter_amd import _lib, apis, ops
    assert 'rsp_mask_remove_small_regions' in _lib.PROTOTYPES and 'rsp_mask_regions_workspace_bytes' in _lib.PROTOTYPES
    assert callable(ops.remove_small_regions) and callable(apis.remove_small_regions)
    assert 'min_mask_region_area' in inspect.signature(apis.SamMaskGenerator.__init__).parameters
    assert 'min_mask_region_area' in inspect.signature(apis.generate_masks).parameters
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'rsp_hip.h')).read()
    assert 'int rsp_mask_remove_small_regions(' in hdr and 'int64_t rsp_mask_regions_workspace_bytes(' in hdr
    assert hasattr(_lib.load(), 'rsp_mask_remove_small_regions')


def test_known_answers_on_the_emulator(emu):
    mr.check_known_answers(emu, CPU)


def test_random_fields_on_the_emulator(emu):
    mr.check_random_fields(emu, CPU)


def test_seams_on_the_emulator(emu):
    mr.check_seams(emu, CPU)


def test_degenerate_shapes_on_the_emulator(emu):
    mr.check_degenerate(emu, CPU)


def test_masks_are_independent_on_the_emulator(emu, monkeypatch):
    mr.check_independence(emu, CPU, monkeypatch)


def test_refusals_on_the_emulator(emu):
    mr.check_refusals(emu, CPU)


def test_apis_remove_small_regions_on_the_emulator(emu):
    mr.check_apis_remove_small_regions(emu, CPU)


# the multi-crop CPU suite's reduced scene (tests/test_sam_multicrop_cpu.py REDUCED) with defects; min_mask_region_area = 30 sits
# between a speck / pinhole (one low-resolution logit: about 20 pixels) and the discs that are kept.  With the oracle alone: 16
# survivors of the first NMS, 14 kept, 2 changed by holes, 1 by islands, 11 unchanged, 2 removed by the second NMS, 2 changed
# ones from crops other than crop 0.
REDUCED = dict(hw=(100, 150), S=128, layers=1, n=4, ndisc=20, rad_scale=0.2, t_st=0.6, area=30)


def test_generator_step_on_the_emulator(emu):
    o2, res = mr.run_region_case(emu, CPU, zero_area=False, **REDUCED)      # area 0: test_zero_area_never_calls_the_kernel
    assert o2['figures']['survivors'] == 16 and o2['figures']['kept'] == 14


def test_zero_area_never_calls_the_kernel(emu):
    """min_mask_region_area = 0 (and the generator without the argument): rsp_mask_remove_small_regions is not called"""
    from rsprompter_amd import _lib
    from rsprompter_amd.apis import SamMaskGenerator, generate_masks
    mc = mr._mc()
    hw, S = (60, 90), 128
    image = mc._test_image(hw)
    boxes = mc._hf_helpers()._generate_per_layer_crops(1, 512 / 1500, hw)[0]
    kw = dict(points_per_side=3, pred_iou_thresh=0.88, stability_score_thresh=0.5)

    class Counting:
        def __init__(self, lib):
            self.lib, self.n = lib, 0

        def __getattr__(self, name):
            fn = getattr(self.lib, name)
            if name != 'rsp_mask_remove_small_regions':
                return fn

            def call(*a):
                self.n += 1
                return fn(*a)
            return call

    saved = _lib._lib
    _lib._lib = counting = Counting(saved)
    try:
        a = SamMaskGenerator(mr.speckled_disc_sam(emu, CPU, S, image, boxes, 6, 0.25), **kw).generate(image)
        b = SamMaskGenerator(mr.speckled_disc_sam(emu, CPU, S, image, boxes, 6, 0.25), min_mask_region_area=0, **kw).generate(image)
        c = generate_masks(mr.speckled_disc_sam(emu, CPU, S, image, boxes[:1], 6, 0.25), image, min_mask_region_area=0, **kw)
        assert counting.n == 0 and len(a.masks) > 1 and a.masks == b.masks and torch.equal(a.bboxes, b.bboxes) and len(c.masks) > 0
        SamMaskGenerator(mr.speckled_disc_sam(emu, CPU, S, image, boxes, 6, 0.25), min_mask_region_area=5, **kw).generate(image)
        assert counting.n > 0                                                   # the counter does see the call when it is made
    finally:
        _lib._lib = saved


def test_generate_masks_is_the_one_crop_generator_on_the_emulator(emu):
    mr.check_generate_masks_is_the_one_crop_generator(emu, CPU, (100, 150), 128, 4, 20, 30, rad_scale=0.2, t_st=0.6)
