"""-m gpu: merging instances cut by tile seams on the device (csrc/seam_merge.hip, rsprompter_amd/large_image.py
merge_nms_type='seam_mask').  The kernel bodies are tests/_seam_merge_cases.py, the same the emulator tier
runs; the test at scale compares the three kernels and the merge with the interval-domain restatement
(tests/_seam_merge_ref.py) on a scene whose dense masks would not fit, and bounds the memory the merge takes.  No model,
no checkpoint."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _seam_merge_cases as cases  # noqa: E402


def test_rle_bbox_kernel(dev):
    from rsprompter_amd import ops
    cases.check_rle_bbox(ops, dev)


def test_rle_pair_overlap_kernel(dev):
    from rsprompter_amd import ops
    cases.check_rle_pair_overlap(ops, dev)


def test_rle_union_kernel(dev):
    from rsprompter_amd import ops
    cases.check_rle_union(ops, dev)


def test_scenes_beyond_32_bit_counts_are_refused(dev):
    from rsprompter_amd import ops
    cases.check_refuses_scenes_beyond_32_bit_counts(ops, dev, pytest)


def test_seam_merge_at_scale_against_the_interval_domain_restatement(dev):
    """a 4096 x 5000 scene, 640-pixel tiles at 0.25 overlap (99 tiles), about 2 000 instances built directly as tile runs:
    ellipse fragments and 256 x 256 noise masks (tens of thousands of runs) in the overlap bands.  rle_bbox of every
    instance, rle_pair_overlap over every pair the restatement evaluates, rle_union of every component and the merge
    itself (keep, members, boxes, scores, labels, count strings) equal the restatement; the merge stays far below the
    dense form of its own output (K x H x W bytes), the condition test_gpu_large_image.py uses."""
    from rsprompter_amd import large_image as li
    from rsprompter_amd import ops
    H, W = 4096, 5000
    mem = {}

    def start():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        mem['base'] = torch.cuda.memory_allocated()

    def stop(k):
        torch.cuda.synchronize()
        mem['peak'], mem['k'] = torch.cuda.max_memory_allocated() - mem['base'], k
    info = cases.check_at_scale(ops, li, dev, H, W, 640, 580, 256, seed=0, measure=dict(start=start, stop=stop))
    print(f'seam merge at scale: {info}; merge peak {mem["peak"] / 2 ** 20:.0f} MiB, dense form of the {mem["k"]} merged masks '
          f'{mem["k"] * H * W / 2 ** 20:.0f} MiB')
    assert info['tiles'] == 99 and 1800 <= info['instances'] <= 2300 and info['max_runs'] > 20000
    assert info['merged'] < info['instances'] and info['kept'] <= info['merged']
    assert mem['peak'] < mem['k'] * H * W


def test_planted_objects_come_back_whole(dev):
    from rsprompter_amd import large_image as li
    cases.check_planted_objects(li, dev)
