"""-m gpu: the detection selection kernels (rsp_rpn_topk, rsp_rpn_decode, rsp_bbox_post, rsp_batched_nms / ops.nms_flat,
rsp_query_topk) against the restatements of tests/_det_props.py on the device: bit for bit the fp64 oracle on the exact tier,
bit for bit the fp32 sequence on the sequence tier (the threshold pool, the rounded offsets, the uncontracted decode), within
max(F, 2 E32) / the NEAR_* rule on the real arithmetic.  tests/test_det_props_cpu.py runs a subset of the same bodies on the
emulator and the census of the case lists."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _det_props as dp  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
_name = lambda c: c.name


@pytest.mark.parametrize('case', dp.nms_cases(), ids=_name)
def test_batched_nms(dev, case):
    from rsprompter_amd import ops
    dp.check_nms(ops, dev, case)


@pytest.mark.parametrize('case', dp.nms_cases(), ids=_name)
def test_nms_flat(dev, case):
    from rsprompter_amd import ops
    dp.check_nms_flat(ops, dev, case)


@pytest.mark.parametrize('case', dp.decode_cases(), ids=_name)
def test_rpn_decode(dev, case):
    from rsprompter_amd import ops
    dp.check_decode(ops, dev, case)


def test_rpn_decode_tolerance(dev):
    from rsprompter_amd import ops
    dp.check_decode_tolerance(ops, dev)


@pytest.mark.parametrize('case', dp.post_cases(), ids=_name)
def test_bbox_post(dev, case):
    from rsprompter_amd import ops
    dp.check_post(ops, dev, case)


def test_bbox_post_tolerance(dev):
    from rsprompter_amd import ops
    dp.check_post_tolerance(ops, dev)


@pytest.mark.parametrize('case', dp.RPN_TOPK, ids=_name)
def test_exact_rpn_topk(dev, case):
    from rsprompter_amd import ops
    dp.check_exact_rpn_topk(ops, dev, case)


def test_rpn_topk_tolerance(dev):
    from rsprompter_amd import ops
    dp.check_rpn_topk_tolerance(ops, dev)


@pytest.mark.parametrize('case', dp.QUERY_EXACT, ids=dp.case_id)
def test_exact_query_topk(dev, case):
    from rsprompter_amd import ops
    dp.check_exact_query_topk(ops, dev, case)


@pytest.mark.parametrize('case', dp.QUERY_SEQ, ids=dp.case_id)
def test_query_topk_division_is_correctly_rounded(dev, case):
    from rsprompter_amd import ops
    dp.check_seq_query_topk(ops, dev, case)


def test_query_topk_tolerance(dev):
    from rsprompter_amd import ops
    dp.check_query_topk_tolerance(ops, dev)
