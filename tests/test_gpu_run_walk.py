"""-m gpu: the device-side reader of run tables (csrc/run_table.h) at the chunk edges of its walk, through every kernel that
uses it.  The bodies are tests/_run_walk_cases.py, the same the emulator tier runs."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _run_walk_cases as cases  # noqa: E402


def test_rle_bbox(dev):
    from rsprompter_amd import ops
    cases.check_rle_bbox(ops, dev)


def test_rle_pair_overlap(dev):
    from rsprompter_amd import ops
    cases.check_rle_pair_overlap(ops, dev)


def test_rle_union(dev):
    from rsprompter_amd import ops
    cases.check_rle_union(ops, dev)


def test_mask_polygons(dev):
    from rsprompter_amd import ops
    cases.check_mask_polygons(ops, dev)


def test_rle_shift(dev):
    from rsprompter_amd import ops
    cases.check_rle_shift(ops, dev)
