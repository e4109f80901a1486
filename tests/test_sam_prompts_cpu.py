"""-m "not gpu": promptable SAM without a GPU.  The two new kernels (rsp_sam_embed_prompts, rsp_mask_score_box) run
on the lane-level emulator (tests/wave_emu) against HF's prompt encoder and HF's mask-generation helpers; the host logic of
rsprompter_amd/sam_prompts.py (grid, coordinate scaling, filter, ordering, outputs, refusals) runs around a stub decoder."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

from test_gpu_sam_prompts import check_prompt_kernel, check_score_kernel  # noqa: E402  (the same checks the GPU runs)

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def _ip():
    from transformers.models.sam import image_processing_pil_sam as ip
    return ip


def test_prompt_kernel_on_the_emulator(emu):
    check_prompt_kernel(emu, CPU)


def test_score_kernel_on_the_emulator(emu):
    # the four geometries of the GPU test (same aspect: identity with a 4-divisible width = strip kernel, identity crop with
    # another output size, a true crop, odd sizes) at 32^2 logits
    cases = ((3, (96, 128), (96, 128), (37, 50)), (2, (128, 128), (128, 128), (64, 64)), (1, (128, 128), (125, 112), (41, 37)),
             (4, (128, 128), (128, 128), (128, 128)), (2, (64, 66), (64, 66), (64, 66)))
    check_score_kernel(emu, CPU, cases, torch.Generator().manual_seed(7), base=32, near_cap=None)
    check_score_kernel(emu, CPU, cases[2:4], torch.Generator().manual_seed(8), thr=0.5, off=0.25, base=32, near_cap=None)


def test_score_kernel_refuses_bad_geometry(emu):
    low = torch.zeros(1, 8, 8)
    with pytest.raises(RuntimeError):
        emu.mask_score_box(low, (32, 32), (40, 32), (16, 16))              # crop larger than the resized image
    with pytest.raises(ValueError):
        emu.mask_score_box(low[:, :, ::2], (32, 32), (32, 32), (16, 16))    # not contiguous
    assert tuple(emu.mask_score_box(low[:0], (32, 32), (32, 32), (16, 16)).shape) == (0, 7)


def test_prompt_wrapper_refusals(emu):
    G, row = torch.randn(2, 128), torch.randn(1, 256)
    with pytest.raises(ValueError):
        emu.sam_embed_prompts(None, None, None, False, G, [row] * 4, row, (64, 64))
    with pytest.raises(ValueError):
        emu.sam_embed_prompts(torch.zeros(2, 3, 2), torch.zeros(2, 2), None, True, G, [row] * 4, row, (64, 64))
    with pytest.raises(ValueError):
        emu.sam_embed_prompts(torch.zeros(2, 3, 2), torch.zeros(2, 3), torch.zeros(3, 4), False, G, [row] * 4, row, (64, 64))
    with pytest.raises(RuntimeError):                                       # HF pads only without a box
        emu.sam_embed_prompts(torch.zeros(2, 3, 2), torch.zeros(2, 3), torch.zeros(2, 4), True, G, [row] * 4, row, (64, 64))


def test_geometry_helpers_are_hfs():
    from rsprompter_amd import sam_prompts as sp
    ip = _ip()
    for n in (1, 2, 16, 32):
        assert np.array_equal(sp.point_grid(n), ip._build_point_grid(n))
    for hw in ((600, 900), (1024, 1024), (1500, 333), (17, 1025), (1365, 2048)):
        nh, nw = ip.SamImageProcessorPil._get_preprocess_shape(None, hw, 1024)
        assert sp.preprocess_shape(hw, 1024) == (nh, nw)
        c = np.random.RandomState(0).rand(5, 3, 2) * 1000
        assert np.array_equal(sp.scale_coords(c, hw, (nh, nw)), ip._normalize_coordinates(1024, c, hw))
        b = np.random.RandomState(1).rand(4, 4) * 1000
        assert np.array_equal(sp.scale_coords(b.reshape(-1, 2, 2), hw, (nh, nw)).reshape(-1, 4),
                              ip._normalize_coordinates(1024, b, hw, is_bounding_box=True))


def test_filter_candidates_is_hf_filter_masks():
    from rsprompter_amd.sam_prompts import filter_candidates
    g = torch.Generator().manual_seed(3)
    iou = torch.rand(50, generator=g)
    sc = torch.randint(0, 1000, (50, 7), generator=g, dtype=torch.int32)
    sc[:, 1] = sc[:, 0] + torch.randint(0, 100, (50,), generator=g, dtype=torch.int32)
    sc[3, :2] = 0                                                           # 0 / 0: NaN fails the comparison
    for ti, ts in ((0.5, 0.9), (0.0, 0.9), (0.5, 0.0), (0.0, 0.0)):
        want = torch.ones(50, dtype=torch.bool)
        if ti > 0:
            want &= iou > ti
        if ts > 0:
            want &= (sc[:, 0] / sc[:, 1]) > ts
        assert torch.equal(filter_candidates(iou, sc, ti, ts), want)
    assert not bool(filter_candidates(iou, sc, 0.0, 0.5)[3])


class _StubSession:
    """a SamSession whose decoder returns prepared logits: `generate_masks` host logic around the emulated kernels"""

    def __init__(self, ops, hw, low_by_point, iou_by_point):
        class _Sam:
            image_size = 128
        self.sam, self.ops = _Sam(), ops
        self.original_size = hw
        from rsprompter_amd.sam_prompts import preprocess_shape
        self.input_size = preprocess_shape(hw, 128)
        self.low, self.iou, self.seen = low_by_point, iou_by_point, None

    def _low_res(self, points, labels, boxes, mask_input, multimask_output):
        assert labels is None and boxes is None and mask_input is None and multimask_output is True
        self.seen = np.asarray(points)
        return self.low, self.iou

    def full_res(self, low_res, mask_threshold=0.0, want_val=False):
        return self.ops.mask_post_logits(low_res.contiguous(), (128, 128), self.input_size, self.original_size, mask_threshold,
                                         want_val=want_val)


def _blob_logits(n, g):
    """n x n prompt points, three masks each, [n*n, 3, 32, 32]: a blob near the point at three sizes, some off"""
    yy, xx = torch.meshgrid(torch.arange(32.0), torch.arange(32.0), indexing='ij')
    out = torch.empty(n * n, 3, 32, 32)
    for i in range(n * n):
        cy, cx = (i // n + 0.5) * 21.0 / n, (i % n + 0.5) * 32.0 / n
        for j in range(3):
            r = 2.0 + 2.5 * j + float(torch.rand((), generator=g))
            amp = 3.0 if j == 1 else 12.0                                   # soft edge: low stability score
            out[i, j] = amp * (1.0 - ((xx - cx) ** 2 + (yy - cy) ** 2) / r ** 2)
    out[1] = -4.0                                                           # empty masks
    return out


@pytest.mark.parametrize('output', ('rle', 'dense'))
def test_generate_masks_host_logic_around_a_stub_decoder(emu, output):
    from oracle import cops
    from rsprompter_amd.apis import generate_masks
    ip = _ip()
    g = torch.Generator().manual_seed(5)
    n, hw = 4, (60, 90)
    low = _blob_logits(n, g)
    iou = torch.rand(n * n, 3, generator=g)
    s = _StubSession(emu, hw, low, iou)
    kw = dict(points_per_side=n, pred_iou_thresh=0.3, stability_score_thresh=0.6, stability_score_offset=1.0,
              mask_threshold=0.0, crops_nms_thresh=0.25)
    st = {}
    res = generate_masks(None, None, session=s, output=output, _stages=st, mask_batch=5, **kw)
    # the grid the decoder saw: HF's, scaled to the image (original pixels; SamSession scales to input pixels)
    assert np.array_equal(s.seen, (ip._build_point_grid(n) * np.array([[hw[1], hw[0]]]))[:, None, :])
    # HF's chain on the CPU
    nh, nw = s.input_size
    val = F.interpolate(low.flatten(0, 1)[:, None], size=(128, 128), mode='bilinear', align_corners=False)[..., :nh, :nw]
    val = F.interpolate(val, size=hw, mode='bilinear', align_corners=False)[:, 0]
    stab = ip._compute_stability_score(val, 0.0, 1.0)
    keep = (iou.flatten() > 0.3) & (stab > 0.6)
    assert ((stab - 0.6).abs() > 1e-3)[~torch.isnan(stab)].all() and 3 < int(keep.sum()) < 3 * n * n - 3
    assert st['kept'].tolist() == keep.nonzero()[:, 0].tolist()
    boxes = ip._batched_mask_to_box(val > 0).float()
    ko = keep.nonzero()[:, 0]
    _, nk = cops.nms(boxes[ko], iou.flatten()[ko], 0.25)
    final = ko[nk]
    assert 0 < final.shape[0] < ko.shape[0]                                  # the NMS removed something
    assert torch.equal(res.bboxes, boxes[final]) and torch.equal(res.scores, iou.flatten()[final])
    want = val[final] > 0
    if output == 'dense':
        assert res.masks.dtype == torch.bool and torch.equal(res.masks, want)
    else:
        assert res.masks == ip._mask_to_rle(want)


def test_generate_masks_refusals_and_empty_result(emu):
    from rsprompter_amd.apis import generate_masks
    s = _StubSession(emu, (60, 90), torch.full((4, 3, 32, 32), -4.0), torch.ones(4, 3))
    with pytest.raises(NotImplementedError, match='crop_n_layers'):
        generate_masks(None, None, session=s, crop_n_layers=1)
    with pytest.raises(ValueError):
        generate_masks(None, None, session=s, output='png')
    res = generate_masks(None, None, session=s, points_per_side=2)             # nothing passes the stability filter
    assert res.masks == [] and tuple(res.bboxes.shape) == (0, 4) and tuple(res.scores.shape) == (0,)
    d = generate_masks(None, None, session=s, points_per_side=2, output='dense')
    assert tuple(d.masks.shape) == (0, 60, 90)


def test_what_still_raises_says_where_to_go():
    from rsprompter_amd.sam_decoder import RSSamPromptEncoder
    from rsprompter_amd.sam_prompts import _sam_of
    with pytest.raises(NotImplementedError, match='get_prompt_embeddings'):
        RSSamPromptEncoder('sam_vit_base')()
    with pytest.raises(TypeError):
        _sam_of(torch.nn.Linear(1, 1))
