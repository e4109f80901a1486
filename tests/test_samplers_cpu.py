"""-m "not gpu": the bilinear samplers on the lane-level emulator (tests/wave_emu) against the fp64 restatements of
tests/_sampler_props.py -- a small subset of the exact cases of every entry point and the smallest tolerance cases; the bodies
are the ones tests/test_gpu_samplers.py runs on the device.  The coverage of the case lists is asserted on the reference
alone."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _sampler_props as sp  # noqa: E402

CPU = torch.device('cpu')
EMU_ROI = tuple(sp.ROI_EXACT_BY_NAME[n] for n in ('p4-c260', 'p2-c8-s4', 'p2-c8-s32'))
EMU_PASTE = sp.PASTE_EXACT[1:4]                      # H W % 4 = 1, 2, 3; C = 3, 1, 2
EMU_RESIZE = (sp.RESIZE_EXACT[1], sp.RESIZE_EXACT[2], sp.RESIZE_EXACT[4], sp.RESIZE_EXACT[7])
EMU_WINDOW = (sp.WINDOW_EXACT[1], sp.WINDOW_EXACT[3], sp.WINDOW_EXACT[4])
EMU_INTERP = (sp.INTERP_EXACT[1], sp.INTERP_EXACT[3], sp.INTERP_EXACT[4], sp.INTERP_EXACT[6])
EMU_MSDA = (sp.MSDA_EXACT[1], sp.MSDA_EXACT[3], sp.MSDA_EXACT[5])


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_roi_cases_cover_every_edge_level_and_grid():
    """on the case lists alone: samples exactly on -1, 0, n - 1 and n on both axes, beyond the cuts and inside; every level
    with sqrt(w h) exactly 56 2^k, within a pixel below and within a pixel above; grids of 1, 2, 4, 8 and 16 samples; levels
    with and without PE; C = 8, 256 and 260; P = 2, 4 and 7; strides 4 .. 32"""
    grids, exact_at, below, above = set(), set(), set(), set()
    for case in sp.ROI_EXACT:
        cen, info = {}, []
        feats, pes, rois, want = sp.roi_exact_inputs(case, 7)
        sp.roi_align_ref(feats, pes, rois, case.P, case.strides, census=cen, info=info)
        for axis in ('x', 'y'):
            assert all(cen[axis][k] > 0 for k in ('-1', '0', 'n-1', 'n', 'below', 'beyond', 'inside')), (case.name, axis, cen[axis])
        for r, (lvl, gh, gw), w in zip(rois.double(), info, want):
            if w is None:
                continue
            grids.add(gh * gw)
            if len(case.strides) == 4:
                sc = float(torch.sqrt((r[3] - r[1]) * (r[4] - r[2])))
                for k in range(4):
                    t = 56.0 * 2 ** k
                    if sc == t:
                        assert lvl == k
                        exact_at.add(k)
                    elif t - 1 <= sc < t:
                        assert lvl == max(k - 1, 0)
                        below.add(k)
                    elif t < sc <= t + 1:
                        assert lvl == k
                        above.add(k)
                assert sc < 896 or lvl == 3
        assert any(case.pe) or case.name == 'p2-c8-s32'
    assert grids == set(sp.ROI_GRIDS), grids
    assert exact_at == {0, 1, 2, 3} and above == {0, 1, 2, 3} and below == {1, 2, 3}, (exact_at, below, above)
    assert {c.C for c in sp.ROI_EXACT} == {8, 256, 260} and {c.P for c in sp.ROI_EXACT} == {2, 4, 7}
    four = [c for c in sp.ROI_EXACT if len(c.strides) == 4]
    assert all(any(c.pe[l] for c in four) and any(not c.pe[l] for c in four) for l in range(4))
    assert {s for c in sp.ROI_EXACT for s in c.strides} == {4, 8, 16, 32}
    assert any(c.C == 260 for c in EMU_ROI)


def test_the_other_case_lists_cover_what_they_claim():
    """paste: H W % 4 in {0, 1, 2, 3} with k >= 2, C > 1, both square and oblong masks; resize: ratios 1, 2, 4, 1/2, 1/4, both
    source types, targets 1 x 1 and 1 x N, padding on neither / one / both sides, both swaps; windows on every scene border and
    the u8 convert path; interpolation from and to 1 x 1; MSDeform with L in {1, 2, 4}, both head dims, non-square levels and
    samples on every edge"""
    assert {(c.img[0] * c.img[1]) % 4 for c in sp.PASTE_EXACT} == {0, 1, 2, 3} == {(c.img[0] * c.img[1]) % 4 for c in EMU_PASTE} | {0}
    assert any(c.C > 1 for c in sp.PASTE_EXACT) and any(c.mask[0] != c.mask[1] for c in sp.PASTE_EXACT)
    assert sp.paste_exact_boxes(9, 13).shape[0] >= 2
    ratios = {(c.new[0] / c.src[0], c.new[1] / c.src[1]) for c in sp.RESIZE_EXACT}
    assert {(1.0, 1.0), (2.0, 2.0), (4.0, 4.0), (0.5, 0.5), (0.25, 0.25)} <= ratios
    assert {c.u8 for c in sp.RESIZE_EXACT} == {True, False}
    assert {None if c.norm is None else c.norm[2] for c in sp.RESIZE_EXACT} == {None, True, False}
    assert any(c.new == (1, 1) for c in sp.RESIZE_EXACT) and any(c.new[0] == 1 and c.new[1] > 1 for c in sp.RESIZE_EXACT)
    pads = {(c.pad[0] > c.new[0], c.pad[1] > c.new[1]) for c in sp.RESIZE_EXACT}
    assert pads == {(False, False), (True, False), (False, True), (True, True)}
    for c in sp.WINDOW_EXACT:
        org = sp.window_origins(c.scene, c.tile)
        assert {x for x, _ in org} >= {0, c.scene[1] - c.tile[1]} and {y for _, y in org} >= {0, c.scene[0] - c.tile[0]}
    assert any(c.u8 and c.tile == c.new and c.pad[1] % 4 == 0 and c.new[1] % 16 for c in sp.WINDOW_EXACT)
    assert any(c.src == (1, 1) for c in sp.INTERP_EXACT) and any(c.out == (1, 1) for c in sp.INTERP_EXACT)
    assert {len(c.levels) for c in sp.MSDA_EXACT} == {1, 2, 4} and {c.hd for c in sp.MSDA_EXACT} == {16, 32}
    assert any(h != w for c in sp.MSDA_EXACT for h, w in c.levels)
    for c in sp.MSDA_EXACT:
        cen = {}
        sp.msda_exact_inputs(c, 23, cen)
        assert all(cen[k] > 0 for k in sp.MSDA_EDGES), (c, cen)
    assert any(c.hd == 16 for c in EMU_MSDA) and any(c.hd == 32 for c in EMU_MSDA)


@pytest.mark.parametrize('case', EMU_ROI, ids=lambda c: c.name)
def test_exact_roi_align_on_the_emulator(emu, case):
    sp.check_exact_roi_align(emu, CPU, case)


@pytest.mark.parametrize('case', EMU_PASTE, ids=sp.case_id)
def test_exact_paste_masks_on_the_emulator(emu, case):
    sp.check_exact_paste(emu, CPU, case)


def test_paste_masks_tolerance_on_the_emulator(emu):
    sp.check_paste_tolerance(emu, CPU, sp.PASTE_TOL[1])


@pytest.mark.parametrize('case', EMU_RESIZE, ids=sp.case_id)
def test_exact_resize_pad_on_the_emulator(emu, case):
    sp.check_exact_resize_pad(emu, CPU, case)


@pytest.mark.parametrize('case', EMU_WINDOW, ids=sp.case_id)
def test_exact_slice_and_crops_resize_pad_on_the_emulator(emu, case):
    sp.check_exact_windows(emu, CPU, case)


@pytest.mark.parametrize('case', EMU_INTERP, ids=sp.case_id)
def test_exact_resize_bilinear_and_attn_mask_on_the_emulator(emu, case):
    sp.check_exact_interp(emu, CPU, case)


@pytest.mark.parametrize('case', EMU_MSDA, ids=sp.case_id)
def test_exact_msdeform_attn_on_the_emulator(emu, case):
    sp.check_exact_msdeform(emu, CPU, case)
