"""-m gpu: the six entry points of the mask field (csrc/mask_field.h: rsp_mask_post, rsp_mask_post_logits, rsp_query_mask_post,
rsp_mask_score_box, rsp_mask_score_box_crops, rsp_persam_locate) against the fp64 field of tests/_mask_field_props.py on the
device: bit for bit on dyadic geometries with integer logits (every form x quad / pixel path, ties at the thresholds), within
the project's 1e-4 on non-dyadic ones, and with more masks than a grid has rows.  tests/test_mask_field_cpu.py runs the same
bodies on the emulator."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mask_field_props as mf  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.quick]


@pytest.mark.parametrize('case', mf.EXACT_CASES, ids=mf.case_id)
def test_exact_field(dev, case):
    from rsprompter_amd import ops
    mf.check_exact_field(ops, dev, case, seed=101)
    mf.check_exact_field(ops, dev, case, seed=202)


@pytest.mark.parametrize('hw', mf.crop_groups(), ids=lambda hw: 'x'.join(map(str, hw)))
def test_exact_crop_table(dev, hw):
    """rsp_mask_score_box_crops: all the exact cases with these logits as rows of one table"""
    from rsprompter_amd import ops
    mf.check_exact_crops(ops, dev, hw, seed=101)
    mf.check_exact_crops(ops, dev, hw, seed=202)


@pytest.mark.parametrize('case', mf.TOL_CASES, ids=mf.case_id)
def test_field_tolerance(dev, case):
    from rsprompter_amd import ops
    mf.check_field_tolerance(ops, dev, case)


def test_det_score_at_the_block_cap(dev):
    from rsprompter_amd import ops
    mf.check_det_score_at_block_cap(ops, dev)


def test_more_masks_than_grid_rows(dev):
    from rsprompter_amd import ops
    mf.check_more_masks_than_grid_rows(ops, dev)
