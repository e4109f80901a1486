"""-m gpu: the ten bilinear samplers (rsp_roi_align, rsp_paste_masks, rsp_resize_pad, rsp_slice_resize_pad, rsp_crops_resize_pad,
rsp_resize_bilinear_nhwc, rsp_query_attn_mask, rsp_msdeform_attn, rsp_msdeform_attn_ex) against the fp64 restatements of
tests/_sampler_props.py on the device: bit for bit on the exact tier (samples on cell boundaries, cuts, last rows, level
thresholds, region margins, thresholds that pixels attain), within max(F, 2 E32) / the NEAR rule on the real shapes' arithmetic.
tests/test_samplers_cpu.py runs a subset of the same bodies on the emulator."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sampler_props as sp  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.quick]


@pytest.mark.parametrize('case', sp.ROI_EXACT, ids=lambda c: c.name)
def test_exact_roi_align(dev, case):
    from rsprompter_amd import ops
    sp.check_exact_roi_align(ops, dev, case)


def test_roi_align_tolerance(dev):
    from rsprompter_amd import ops
    sp.check_roi_align_tolerance(ops, dev)


@pytest.mark.parametrize('case', sp.PASTE_EXACT, ids=sp.case_id)
def test_exact_paste_masks(dev, case):
    from rsprompter_amd import ops
    sp.check_exact_paste(ops, dev, case)


@pytest.mark.parametrize('case', sp.PASTE_TOL, ids=sp.case_id)
def test_paste_masks_tolerance(dev, case):
    from rsprompter_amd import ops
    sp.check_paste_tolerance(ops, dev, case)


@pytest.mark.parametrize('case', sp.RESIZE_EXACT, ids=sp.case_id)
def test_exact_resize_pad(dev, case):
    from rsprompter_amd import ops
    sp.check_exact_resize_pad(ops, dev, case)


@pytest.mark.parametrize('case', sp.WINDOW_EXACT, ids=sp.case_id)
def test_exact_slice_and_crops_resize_pad(dev, case):
    from rsprompter_amd import ops
    sp.check_exact_windows(ops, dev, case)


def test_resize_pad_tolerance(dev):
    from rsprompter_amd import ops
    sp.check_resize_tolerance(ops, dev)


@pytest.mark.parametrize('case', sp.INTERP_EXACT, ids=sp.case_id)
def test_exact_resize_bilinear_and_attn_mask(dev, case):
    from rsprompter_amd import ops
    sp.check_exact_interp(ops, dev, case)


def test_resize_bilinear_and_attn_mask_tolerance(dev):
    from rsprompter_amd import ops
    sp.check_interp_tolerance(ops, dev)


@pytest.mark.parametrize('case', sp.MSDA_EXACT, ids=lambda c: f'L{len(c.levels)}-hd{c.hd}-' + '_'.join(f'{h}x{w}' for h, w in c.levels))
def test_exact_msdeform_attn(dev, case):
    from rsprompter_amd import ops
    sp.check_exact_msdeform(ops, dev, case)


def test_msdeform_attn_tolerance(dev):
    from rsprompter_amd import ops
    sp.check_msdeform_tolerance(ops, dev)
