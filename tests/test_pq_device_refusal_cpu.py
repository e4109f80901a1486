"""-m "not gpu": maps on the CPU are refused by the panoptic-quality layers before anything is launched.  This file patches
nothing (tests/test_pq_cpu.py runs under the emulator harness, which replaces ops._is_device and ops.require_device), so it
sees the checks as a user does, with or without a GPU in the machine.

Each call is built so that it cannot reach a launch even if the check under test were missing: the argument the function
looks at next raises Tripwire, which is no ValueError, so the test then fails instead of handing host pointers to a kernel."""
import pytest
import torch


class Tripwire(Exception):
    pass


class TrippingList(list):
    """segments_info that may not be looked at: pq_image takes its length right after the checks of the maps"""

    def __len__(self):
        raise Tripwire('pq_image went past the device check')

    def __iter__(self):
        raise Tripwire('pq_image went past the device check')


class TrippingRow(dict):
    """a row of which only `tp` may be read: pq_reduce stacks the other entries right before its launch"""

    def __getitem__(self, key):
        if key != 'tp':
            raise Tripwire('pq_reduce went past the device check')
        return dict.__getitem__(self, key)


CATS = {0: dict(isthing=1)}


def test_pq_image_refuses_cpu_maps():
    from rsprompter_amd import ops
    pan = torch.full((4, 8), 1000, dtype=torch.int32)
    for gt in (torch.ones((4, 8), dtype=torch.int32), torch.ones((4, 8), dtype=torch.int64), torch.zeros((4, 8, 3), dtype=torch.uint8)):
        assert not pan.is_cuda and not gt.is_cuda
        with pytest.raises(ValueError, match='device'):
            ops.pq_image(pan, gt, TrippingList(), CATS, 1)


def test_pq_reduce_refuses_cpu_rows():
    from rsprompter_amd import ops
    row = TrippingRow(tp=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match='device'):
        ops.pq_reduce([row, row])


def test_metric_and_api_refuse_a_cpu_device():
    """CocoPanopticMetric(device='cpu') and apis.panoptic_quality(device='cpu') stop at require_device, before a map is moved"""
    from rsprompter_amd import apis
    from rsprompter_amd.evaluation import CocoPanopticMetric
    m = CocoPanopticMetric(device='cpu')
    m.dataset_meta = dict(classes=('a',), thing_classes=('a',))
    pan = torch.full((1, 4, 8), 1000, dtype=torch.int32)
    sample = dict(img_id=0, img_path='x.jpg', pred_panoptic_seg=dict(sem_seg=pan), gt_panoptic=torch.ones((4, 8), dtype=torch.int32),
                  segments_info=TrippingList())
    with pytest.raises(RuntimeError, match='HIP device'):
        m.process(None, [sample])
    assert m.results == []
    with pytest.raises(RuntimeError, match='HIP device'):
        apis.panoptic_quality([pan], [torch.ones((4, 8), dtype=torch.int32)], [TrippingList()], ('a',), device='cpu')
