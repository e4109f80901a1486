"""-m "not gpu": the mask-field kernels (csrc/mask_field.h and its six entry points) on the lane-level emulator (tests/wave_emu)
against the fp64 field of tests/_mask_field_props.py -- every exact case of at most 16k output pixels and the two smallest
tolerance cases; the bodies are the ones tests/test_gpu_mask_field.py runs on the device.  The input refusals of the two
post-process wrappers are host logic and are tested here only."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _mask_field_props as mf  # noqa: E402

CPU = torch.device('cpu')
EMU_PIXELS = 16384
EMU_EXACT = tuple(c for c in mf.EXACT_CASES if mf.pixels(c) <= EMU_PIXELS)
EMU_TOL = tuple(sorted(mf.TOL_CASES, key=mf.pixels)[:2])


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_cases_cover_every_form_and_path():
    """on the case lists alone: every form x quad / pixel path, both stage-1 directions, both stage-2 directions, non-square
    and non-256 logits, 1-pixel extents, strips below / between / beyond the row tiles, an item count that is no multiple of
    the block -- and the emulator's subset keeps all of it but the two-block strip"""
    for cases, emu_subset in ((mf.EXACT_CASES, False), (EMU_EXACT, True)):
        forms = {(c.form, c.out[1] % 4) for c in cases}
        assert {('ident', 1), ('ident', 2), ('ident', 3)} <= forms and ('strip', 0) in forms
        assert ('generic', 0) in forms and any(f == 'generic' and r for f, r in forms)
        for c in cases:
            assert mf.mask_form(c.crop, c.out) == c.form, c
            assert c.hw[0] / c.img[0] in (0.25, 0.5, 1, 2) and c.hw[1] / c.img[1] in (0.25, 0.5, 1, 2), c
            assert c.crop[0] <= c.img[0] and c.crop[1] <= c.img[1], c
            assert c.out in (c.crop, (c.crop[0] // 2, c.crop[1] // 2), (c.crop[0] * 2, c.crop[1] * 2)), c
            assert c.out != (c.crop[0] // 2, c.crop[1] // 2) or (c.crop[0] % 2 == 0 and c.crop[1] % 2 == 0), c
        assert any(c.img[0] < c.hw[0] for c in cases) and any(c.img[0] > c.hw[0] for c in cases)
        assert any(c.out[0] > c.crop[0] for c in cases) and any(c.out[0] < c.crop[0] for c in cases)
        assert any(c.hw[0] != c.hw[1] for c in cases) and any(c.hw == (1, 1) for c in cases)
        assert any(c.out == (1, 1) for c in cases) and any(c.out[1] == 1 and c.out[0] > 1 for c in cases)
        strips = [c for c in cases if c.form == 'strip']
        assert any(c.out[1] == 4 for c in strips) and any(c.out[0] < mf.MP_ROWS for c in strips)
        assert any(mf.MP_ROWS < c.out[0] < mf.MS_ROWS and c.out[0] % mf.MP_ROWS for c in strips)
        assert any(c.out[0] > mf.MS_ROWS and c.out[0] % mf.MS_ROWS for c in strips)
        items = [-(-c.out[0] // mf.MP_ROWS) * (c.out[1] // 4) for c in strips]
        assert any(n % 256 for n in items) and (emu_subset or any(n > 256 for n in items))
    assert all(mf.mask_form(c.crop, c.out) == c.form for c in mf.TOL_CASES)
    assert len(EMU_TOL) == 2 and EMU_TOL[0].out == (95, 77) and EMU_TOL[1].out == (100, 129)


@pytest.mark.parametrize('case', EMU_EXACT, ids=mf.case_id)
def test_exact_field_on_the_emulator(emu, case):
    mf.check_exact_field(emu, CPU, case, seed=101)


@pytest.mark.parametrize('hw', mf.crop_groups(EMU_EXACT), ids=lambda hw: 'x'.join(map(str, hw)))
def test_exact_crop_table_on_the_emulator(emu, hw):
    mf.check_exact_crops(emu, CPU, hw, seed=101, cases=EMU_EXACT)


@pytest.mark.parametrize('case', EMU_TOL, ids=mf.case_id)
def test_field_tolerance_on_the_emulator(emu, case):
    mf.check_field_tolerance(emu, CPU, case)


def test_post_process_wrappers_refuse_what_is_not_contiguous_fp32(emu):
    """ops.mask_post and ops.query_mask_post: contiguous fp32 [k, h, w] logits, and a contiguous int32 qidx on their device --
    anything else is a ValueError on the host (nothing is launched)"""
    low = torch.zeros(3, 8, 8)
    geo = ((32, 32), (32, 32), (32, 32))
    qidx, cls = torch.tensor([0, 2], dtype=torch.int32), torch.ones(2)
    for bad in (low[:, :, ::2], low.double(), low[0], low[None], low.half()):
        with pytest.raises(ValueError):
            emu.mask_post(bad, *geo, 0.5)
        with pytest.raises(ValueError):
            emu.query_mask_post(bad, qidx, cls, *geo)
    # (the meta device stands in for "another device than the logits'")
    for bad in (qidx.long(), torch.tensor([0, 9, 2, 9], dtype=torch.int32)[::2], qidx.float(), qidx[None], qidx.to('meta')):
        with pytest.raises(ValueError):
            emu.query_mask_post(low, bad, cls, *geo)
    assert tuple(emu.mask_post(low, *geo, 0.5).shape) == (3, 32, 32)
    assert tuple(emu.query_mask_post(low, qidx, cls, *geo)[0].shape) == (2, 32, 32)

