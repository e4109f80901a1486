"""CPU (`-m "not gpu"`): sliced inference on large scenes (csrc/large_image.hip, rsprompter_amd/large_image.py).

The oracle is tests/_large_image_ref.py (slicing, shifts, dense paste and column-major RLE counting restated on numpy)
together with oracle/glue.py::batched_nms and rsprompter_amd.rle.counts_to_string; the kernels run lane by lane on the
emulator (tests/wave_emu) and must agree exactly."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _large_image_ref as ref  # noqa: E402

MEAN = [123.675, 116.28, 103.53]
STD = [58.395, 57.12, 57.375]
PAD = (0.406 * 255, 0.456 * 255, 0.485 * 255)


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# ----------------------------------------------------------------------------------------------------------- slicing
def test_slice_bboxes_known_answers():
    from rsprompter_amd.large_image import slice_bboxes
    for f in (slice_bboxes, ref.slice_bboxes):
        assert f(788, 1400, 640, 640, 0.25, 0.25) == [[0, 0, 640, 640], [480, 0, 1120, 640], [760, 0, 1400, 640],
                                                      [0, 148, 640, 788], [480, 148, 1120, 788], [760, 148, 1400, 788]]
        assert f(300, 500, 640, 640, 0.25, 0.25) == [[0, 0, 500, 300]]
        assert len(f(2400, 3000, 1024, 1024, 0.25, 0.25)) == 12


def test_slice_bboxes_properties_over_drawn_sizes():
    from rsprompter_amd.large_image import slice_bboxes
    rng = np.random.default_rng(0)
    for _ in range(200):
        H, W = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        sh, sw = int(rng.integers(8, 200)), int(rng.integers(8, 200))
        r = float(rng.choice([0.0, 0.1, 0.25, 0.5]))
        tiles = slice_bboxes(H, W, sh, sw, r, r)
        assert tiles == ref.slice_bboxes(H, W, sh, sw, r, r)
        cover = np.zeros((H, W), bool)
        for x0, y0, x1, y1 in tiles:
            assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H
            assert (y1 - y0, x1 - x0) == (min(sh, H), min(sw, W))
            cover[y0:y1, x0:x1] = True
        assert cover.all()
        assert tiles == sorted(tiles, key=lambda t: (t[1], t[0]))                  # row-major


# ------------------------------------------------------------------------------------------------- run-domain shift
def _shift_cases():
    """(mask [h, w], (ox, oy), (H, W), name): the placements and shapes the issue lists, then drawn ones"""
    rng = np.random.default_rng(1)
    rnd = lambda h, w, d: rng.random((h, w)) < d                                    # noqa: E731
    cases = [
        (np.zeros((5, 7), bool), (2, 3), (12, 15), 'empty'),
        (np.ones((5, 7), bool), (2, 3), (12, 15), 'full'),
        (np.ones((5, 7), bool), (0, 0), (5, 7), 'full, tile == scene'),
        (rnd(9, 6, 0.5), (4, 0), (9, 14), 'h == H'),
        (np.ones((9, 6), bool), (4, 0), (9, 14), 'h == H, full'),
        (rnd(6, 8, 0.5), (3, 0), (11, 13), 'oy == 0'),
        (rnd(6, 8, 0.5), (3, 5), (11, 13), 'oy == H - h'),
        (rnd(6, 8, 0.5), (5, 2), (11, 13), 'ox + w == W'),
        (rnd(6, 8, 0.5), (5, 5), (11, 13), 'bottom-right corner'),
        (rnd(6, 8, 0.5), (0, 0), (11, 13), 'top-left corner'),
        (np.pad(np.ones((7, 4), bool), ((0, 0), (2, 3))), (1, 2), (10, 12), 'ones-run spanning several columns'),
        (rnd(7, 1, 0.6), (3, 2), (10, 6), 'w == 1'),
        (rnd(1, 9, 0.6), (2, 4), (7, 13), 'h == 1'),
        (rnd(1, 1, 1.0), (2, 4), (7, 13), 'h == w == 1'),
        (rnd(40, 37, 0.5), (11, 7), (64, 61), 'more than 256 runs: several chunks'),
        (rnd(40, 37, 0.97), (0, 3), (64, 37), 'dense, w == W'),
    ]
    for i in range(40):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        d = float(rng.choice([0.0, 0.1, 0.5, 0.9, 1.0]))
        cases.append((rnd(h, w, d), (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))), (H, W), f'drawn {i}'))
    return cases


def test_restatement_run_domain_shift_equals_dense_paste():
    """the oracle's two legs agree with each other: run-domain definition == dense paste + recount"""
    for mask, off, full, name in _shift_cases():
        h, w = mask.shape
        want = ref.rle_counts(ref.shift_masks(mask[None], off, full)[0])
        assert ref.rle_shift_counts(ref.rle_counts(mask), h, w, off, full) == want, name
        assert ref.rle_counts_np(ref.shift_masks(mask[None], off, full)[0]) == want, name
        assert ref.counts_to_mask(want, *full).tolist() == ref.shift_masks(mask[None], off, full)[0].tolist(), name


def _run_shift(ops, masks, offs, full, cap_out):
    h, w = masks[0].shape
    cap = 4096
    k = len(masks)
    cin = torch.zeros((k, cap), dtype=torch.int32)
    nin = torch.zeros((k,), dtype=torch.int32)
    for i, m in enumerate(masks):
        c = ref.rle_counts(m)
        cin[i, :len(c)] = torch.tensor(c, dtype=torch.int32)
        nin[i] = len(c)
    return ops.rle_shift(cin, nin, torch.tensor(offs, dtype=torch.int32).reshape(-1, 2), (h, w), full, cap_out)


def test_rle_shift_kernel_against_dense_paste_and_recount(emu):
    from rsprompter_amd.rle import counts_to_string
    for mask, off, full, name in _shift_cases():
        want = ref.rle_counts(ref.shift_masks(mask[None], off, full)[0])
        out, n = _run_shift(emu, [mask], [off], full, 4096)
        got = out[0, :int(n[0])].tolist()
        assert got == want, (name, got, want)
        _, offs, flat = emu.rle_to_string(out, n, 1, 8 * len(want) + 8)
        assert flat[:int(offs[1])].numpy().tobytes() == counts_to_string(want), name


def test_rle_shift_kernel_input_from_mask_rle_kernel_and_several_instances(emu):
    """the hand-off as the pipeline makes it: rsp_mask_rle -> rsp_rle_shift, one launch for instances with different offsets"""
    rng = np.random.default_rng(2)
    h, w, full = 12, 16, (30, 41)
    masks = np.stack([rng.random((h, w)) < d for d in (0.0, 0.2, 0.5, 0.8, 1.0, 0.5)])
    offs = [(0, 0), (25, 18), (7, 3), (25, 0), (0, 18), (13, 9)]
    counts, n = emu.mask_rle_counts(torch.from_numpy(masks), cap=256)
    out, no = emu.rle_shift(counts, n, torch.tensor(offs, dtype=torch.int32), (h, w), full, 512)
    for i in range(len(masks)):
        want = ref.rle_counts(ref.shift_masks(masks[i:i + 1], offs[i], full)[0])
        assert out[i, :int(no[i])].tolist() == want, i


def test_rle_shift_kernel_capacity_too_small_then_retry(emu):
    rng = np.random.default_rng(3)
    mask = rng.random((10, 12)) < 0.5
    off, full = (3, 4), (20, 22)
    want = ref.rle_counts(ref.shift_masks(mask[None], off, full)[0])
    out, n = _run_shift(emu, [mask], [off], full, 8)
    assert int(n[0]) == -len(want)
    out, n = _run_shift(emu, [mask], [off], full, len(want))                         # exactly enough
    assert int(n[0]) == len(want) and out[0, :len(want)].tolist() == want


def test_rle_shift_refuses_scene_beyond_32_bit_counts(emu):
    with pytest.raises(ValueError, match='32-bit'):
        _run_shift(emu, [np.ones((2, 2), bool)], [(0, 0)], (65536, 32768), 16)
    lib = emu._lib.load()
    z = torch.zeros((4,), dtype=torch.int32)
    assert lib.rsp_rle_shift(z.data_ptr(), z.data_ptr(), 1, 4, z.data_ptr(), 2, 2, 65536, 32768, z.data_ptr(), z.data_ptr(), 4, 0) != 0


def test_run_table_pipelines_retry_from_a_capacity_that_is_too_small(emu):
    """rle.encode_runs / shift_runs / union_runs / runs_to_strings from cap = 2 and flat_cap = 1: each retries, and the tables
    and strings are those of the default capacities and of the restatement on the dense paste"""
    import _run_table_cases as cases
    cases.check_capacity_retries(emu, torch.device('cpu'))


def test_mask_forms_round_trip_through_the_run_table(emu):
    """dense tensors, bytes / str dicts and list dicts to the run table and back (rsprompter_amd/rle.py "mask forms"): exact
    round trips, the bit planes, mixed sizes, k = 0, the capacity retry, the refusals and the host reads of every form"""
    import _run_table_cases as cases
    from rsprompter_amd import rle
    cases.check_mask_forms(emu, rle, torch.device('cpu'), pytest)


# ---------------------------------------------------------------------------------------------------- tile front end
@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
@pytest.mark.parametrize('norm', [False, True])
def test_slice_resize_pad_kernel_equals_per_crop_resize_pad(emu, dtype, norm):
    from rsprompter_amd.apis import rescale_size
    from rsprompter_amd.large_image import slice_bboxes
    rng = np.random.default_rng(4)
    normalise = (MEAN, STD, True) if norm else None
    # (scene H, W), patch, model scale (w, h): resize up, resize down, identity (convert-and-pad), scene smaller than patch
    for (H, W), patch, scale in (((45, 70), 32, (48, 48)), ((45, 70), 32, (24, 24)), ((45, 70), 32, (32, 32)),
                                 ((40, 64), 32, (48, 32)), ((20, 30), 64, (48, 48)), ((33, 47), 16, (16, 16))):
        scene = rng.integers(0, 256, (H, W, 3)).astype(dtype)
        if dtype == np.float32:
            scene += rng.random((H, W, 3)).astype(np.float32)
        tiles = slice_bboxes(H, W, patch, patch, 0.25, 0.25)
        assert any(t[2] == W for t in tiles) and any(t[3] == H for t in tiles)      # tiles touching right / bottom edges
        th, tw = min(patch, H), min(patch, W)
        (nw, nh), _ = rescale_size((tw, th), scale)
        pw, ph = max(scale[0], nw), max(scale[1], nh)
        ts = torch.from_numpy(scene)
        origins = torch.tensor([[t[0], t[1]] for t in tiles], dtype=torch.int32)
        got = emu.slice_resize_pad(ts, origins, (th, tw), (nh, nw), (ph, pw), PAD, normalise=normalise)
        assert got.shape == (len(tiles), 3, ph, pw)
        for i, (x0, y0, x1, y1) in enumerate(tiles):
            want = emu.resize_pad(ts[y0:y1, x0:x1].contiguous(), (nh, nw), (ph, pw), PAD, normalise=normalise)
            assert torch.equal(got[i], want), ((H, W), patch, scale, i)


def test_paste_tiles_kernel_equals_shift_masks(emu):
    rng = np.random.default_rng(5)
    for (h, w), full in (((6, 8), (16, 32)), ((6, 8), (11, 13)), ((5, 16), (5, 16))):
        masks = rng.random((4, h, w)) < 0.5
        offs = [(int(rng.integers(0, full[1] - w + 1)), int(rng.integers(0, full[0] - h + 1))) for _ in range(4)]
        got = emu.paste_tiles(torch.from_numpy(masks), torch.tensor(offs, dtype=torch.int32), full)
        for i in range(4):
            assert np.array_equal(got[i].numpy(), ref.shift_masks(masks[i:i + 1], offs[i], full)[0])


# ---------------------------------------------------------------------------------------------------------- merging
def _sample(boxes, scores, labels, masks=None):
    from rsprompter_amd.structures import DetDataSample, InstanceData
    s = DetDataSample(metainfo=dict(ori_shape=(8, 8)))
    s.pred_instances = InstanceData(bboxes=torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4),
                                    scores=torch.tensor(scores, dtype=torch.float32), labels=torch.tensor(labels, dtype=torch.int64))
    if masks is not None:
        s.pred_instances.masks = torch.from_numpy(masks)
    return s


def test_merge_results_by_nms_known_answers(emu):
    """by hand: tile 0 at (0, 0), tile 1 at (6, 0).  The object at scene [6, 1, 10, 5] is seen by both tiles (tile 1 sees it
    at [0, 1, 4, 5], shifted by one pixel: IoU 0.6 > 0.25) -> the 0.9 one stays, the 0.7 one goes; a second class with the
    IDENTICAL box survives next to it; an unrelated box survives; keep order is descending score."""
    from oracle import glue
    from rsprompter_amd.large_image import merge_results_by_nms, shift_predictions
    rng = np.random.default_rng(6)
    m0, m1 = rng.random((3, 8, 8)) < 0.5, rng.random((2, 8, 8)) < 0.5
    t0 = _sample([[6, 1, 10, 5], [6, 1, 10, 5], [0, 0, 2, 2]], [0.9, 0.6, 0.5], [0, 1, 0], m0)
    t1 = _sample([[1, 1, 5, 5], [2, 2, 3, 3]], [0.7, 0.8], [0, 0], m1)
    offsets, full = [(0, 0), (6, 0)], (8, 14)
    inst = shift_predictions([t0, t1], offsets, full)
    assert inst.bboxes.tolist()[3] == [7.0, 1.0, 11.0, 5.0] and inst.masks.shape == (5, 8, 14)
    assert np.array_equal(inst.masks[4].numpy(), ref.shift_masks(m1[1:2], (6, 0), full)[0])
    out = merge_results_by_nms([t0, t1], offsets, full, dict(type='nms', iou_threshold=0.25))
    p = out.pred_instances
    assert p.scores.tolist() == pytest.approx([0.9, 0.8, 0.6, 0.5])                      # 0.7 suppressed, descending
    assert p.labels.tolist() == [0, 0, 1, 0]
    assert p.bboxes.tolist() == [[6, 1, 10, 5], [8, 2, 9, 3], [6, 1, 10, 5], [0, 0, 2, 2]]
    assert np.array_equal(p.masks[1].numpy(), ref.shift_masks(m1[1:2], (6, 0), full)[0])
    # ... and the same through the restatement + the oracle's batched_nms
    tiles = [dict(bboxes=s.pred_instances.bboxes.numpy(), scores=s.pred_instances.scores.numpy(),
                  labels=s.pred_instances.labels.numpy()) for s in (t0, t1)]
    keep, boxes, *_ = ref.merge(tiles, offsets, full, glue.batched_nms, 0.25)
    assert keep.tolist() == [0, 4, 1, 2] and np.array_equal(boxes[keep], p.bboxes.numpy())


def test_unsupported_requests_raise_clearly(emu):
    from rsprompter_amd.large_image import inference_large_image, merge_results_by_nms
    t = _sample([[0, 0, 1, 1]], [0.5], [0])
    with pytest.raises(NotImplementedError, match='soft_nms'):
        merge_results_by_nms([t], [(0, 0)], (8, 8), dict(type='soft_nms', iou_threshold=0.25))
    with pytest.raises(NotImplementedError, match='soft_nms'):
        inference_large_image(None, np.zeros((4, 4, 3), np.uint8), merge_nms_type='soft_nms')
    with pytest.raises(ValueError, match='8192'):
        inference_large_image(None, np.zeros((4, 4, 3), np.uint8), patch_size=(64, 9000))
    rot = _sample([[0, 0, 1, 1]], [0.5], [0])
    rot.pred_instances.bboxes = torch.zeros((1, 5))
    with pytest.raises(NotImplementedError, match='rotated'):
        merge_results_by_nms([rot], [(0, 0)], (8, 8), dict(type='nms', iou_threshold=0.25))


def test_dense_request_beyond_the_limit_names_the_byte_count():
    from rsprompter_amd import large_image as li
    with pytest.raises(ValueError, match=str(600 * 10000 * 10000)):
        li._check_dense(600, 10000, 10000)


# --------------------------------------------------------------------------------------------------------- pipeline
class _StubDetector(torch.nn.Module):
    """a detector whose result is a seeded function of the tile's pixels: the pipeline around it is what is under test"""

    def __init__(self, scale):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.cfg = dict(test_dataloader=dict(dataset=dict(pipeline=[
            dict(type='LoadImageFromFile', to_float32=True), dict(type='Resize', scale=scale, keep_ratio=True),
            dict(type='Pad', size=scale, pad_val=dict(img=PAD, masks=0)),
            dict(type='PackDetInputs', meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor'))])))
        self.calls = []

    def test_step(self, data):
        from rsprompter_amd.structures import InstanceData
        self.calls.append(len(data['inputs']))
        for x, s in zip(data['inputs'], data['data_samples']):
            th, tw = s.metainfo['ori_shape']
            rng = np.random.default_rng(int(x.double().sum().item()) % (2 ** 31))
            k = int(rng.integers(0, 7))
            x0, y0 = rng.integers(0, tw - 4, k), rng.integers(0, th - 4, k)
            boxes = np.stack([x0, y0, x0 + rng.integers(2, 12, k), y0 + rng.integers(2, 12, k)], 1).astype(np.float32).reshape(-1, 4)
            masks = rng.random((k, th, tw)) < rng.choice([0.0, 0.05, 0.5, 1.0], k)[:, None, None]
            s.pred_instances = InstanceData(bboxes=torch.from_numpy(boxes), scores=torch.from_numpy(rng.random(k).astype(np.float32)),
                                            labels=torch.from_numpy(rng.integers(0, 2, k)), masks=torch.from_numpy(masks))
        return data['data_samples']


@pytest.mark.parametrize('shape,patch,scale', [((45, 70), 32, (32, 32)), ((45, 70), (24, 32), (48, 48)), ((20, 30), 64, (32, 32))])
def test_inference_large_image_pipeline_around_a_stub_detector(emu, shape, patch, scale):
    """the flow of inference_large_image (tile batches, metas, per-batch RLE, shift, merge, run-domain scene RLE, dense
    form, return_patches) against: per-crop resize_pad -> the same stub -> restatement shift / oracle batched_nms / dense
    paste / RLE"""
    from oracle import glue
    from rsprompter_amd import large_image as li
    from rsprompter_amd.apis import TestPipeline, get_test_pipeline_cfg
    from rsprompter_amd.rle import counts_to_string
    rng = np.random.default_rng(7)
    H, W = shape
    scene = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    ph, pw = (patch, patch) if isinstance(patch, int) else patch
    model = _StubDetector(scale)
    pipe = TestPipeline(get_test_pipeline_cfg(model.cfg), device='cpu')
    tiles = ref.slice_bboxes(H, W, ph, pw, 0.25, 0.25)
    offsets = [(t[0], t[1]) for t in tiles]
    per_tile = []
    for x0, y0, x1, y1 in tiles:
        d = pipe(dict(img=np.ascontiguousarray(scene[y0:y1, x0:x1]), img_id=0))
        assert d['data_samples'].metainfo['ori_shape'] == (min(ph, H), min(pw, W))
        p = model.test_step(dict(inputs=[d['inputs']], data_samples=[d['data_samples']]))[0].pred_instances
        per_tile.append(dict(bboxes=p.bboxes.numpy(), scores=p.scores.numpy(), labels=p.labels.numpy(), masks=p.masks.numpy()))
    keep, boxes, scores, labels, tile = ref.merge(per_tile, offsets, (H, W), glue.batched_nms, 0.25)
    all_masks = [m for r in per_tile for m in r['masks']]
    want = [counts_to_string(ref.rle_counts(ref.shift_masks(all_masks[i][None], offsets[tile[i]], (H, W))[0])) for i in keep]
    assert len(keep) > 0 and (len(tiles) == 1 or len(scores) > len(keep))       # the merge suppresses something
    for bs in (1, 4):
        model.calls = []
        out, patches, start = li.inference_large_image(model, scene, patch_size=patch, batch_size=bs, return_patches=True)
        assert start == offsets and len(patches) == len(tiles) and out.ori_shape == (H, W)
        assert model.calls == [min(bs, len(tiles) - i) for i in range(0, len(tiles), bs)]
        p = out.pred_instances
        assert out.keep.tolist() == keep.tolist() and np.array_equal(p.bboxes.numpy(), boxes[keep])
        assert np.array_equal(p.scores.numpy(), scores[keep]) and np.array_equal(p.labels.numpy(), labels[keep])
        assert [m['counts'] for m in p.masks] == want and all(m['size'] == [H, W] for m in p.masks)
    dense = li.inference_large_image(model, torch.from_numpy(scene), patch_size=patch, batch_size=3, masks='dense')
    dm = dense.pred_instances.masks.numpy()
    assert dm.shape == (len(keep), H, W)
    assert [counts_to_string(ref.rle_counts(m)) for m in dm] == want
    js = li.pred2dict(out, 0.5)
    assert len(js['labels']) == int((scores[keep] >= 0.5).sum()) == len(js['masks']) and all(isinstance(m['counts'], str) for m in js['masks'])
