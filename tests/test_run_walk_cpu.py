"""CPU (`-m "not gpu"`): the device-side reader of run tables (csrc/run_table.h) at the chunk edges of its walk, through every
kernel that uses it, lane by lane on the emulator (tests/wave_emu), the sources unchanged.  The bodies are
tests/_run_walk_cases.py, the same the device tier runs."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _run_walk_cases as cases  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_table_holds_the_chunk_edges():
    t = cases.table()
    assert sorted(n for n in t['n'] if n >= 0) == sorted(cases.ROW_LENGTHS) and min(t['n']) < 0
    assert t['cap'] == max(t['n']) + 7
    counts, n = cases.tensors(CPU, cases.POISON)
    for i, r in enumerate(t['rows']):
        assert counts[i, :len(r or [])].tolist() == (r or []) and (counts[i, len(r or []):] == cases.POISON).all()
        assert r is None or len(r) == 0 or sum(r) == cases.H * t['W']


def test_rle_bbox(emu):
    cases.check_rle_bbox(emu, CPU)


def test_rle_pair_overlap(emu):
    cases.check_rle_pair_overlap(emu, CPU)


def test_rle_union(emu):
    cases.check_rle_union(emu, CPU)


def test_mask_polygons(emu):
    cases.check_mask_polygons(emu, CPU)


def test_rle_shift(emu):
    cases.check_rle_shift(emu, CPU)
