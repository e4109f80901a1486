"""-m gpu: sliced inference on large scenes on the device (csrc/large_image.hip, rsprompter_amd/large_image.py): the three
kernels at scale, exact against tests/_large_image_ref.py, and `inference_large_image` end to end -- on the reference
demo's own scene (tests/golden/large_image/large_image.jpg, 1400 x 788) against the composition of the per-image API on
host-cut crops with the restatement, and on a synthetic 4096 x 5000 scene for the memory claim of the run-domain design."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import _large_image_ref as ref  # noqa: E402

MEAN = [123.675, 116.28, 103.53]
STD = [58.395, 57.12, 57.375]
PAD = (0.406 * 255, 0.456 * 255, 0.485 * 255)
SCENE = os.path.join(HERE, 'golden', 'large_image', 'large_image.jpg')


# ------------------------------------------------------------------------------------------------------------ kernels
def test_slice_resize_pad_at_scale_equals_per_crop_resize_pad(dev):
    """an 8000 x 12000 scene, 1024 tiles (176 of them): the convert-and-pad path (tile == model input), a resize down and
    a resize up, uint8 and fp32, plain and with the fused normalise; every tile torch.equal to ops.resize_pad of its crop"""
    from rsprompter_amd import ops
    from rsprompter_amd.large_image import slice_bboxes
    g = torch.Generator(device=dev).manual_seed(0)
    H, W = 8000, 12000
    scene = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    tiles = slice_bboxes(H, W, 1024, 1024, 0.25, 0.25)
    assert len(tiles) == 176 and tiles[-1] == [W - 1024, H - 1024, W, H]
    origins = torch.tensor([[t[0], t[1]] for t in tiles], dtype=torch.int32, device=dev)
    checked = 0
    for src, new_hw, pad_hw, normalise, stride in ((scene, (1024, 1024), (1024, 1024), None, 1),
                                                   (scene, (1024, 1024), (1024, 1024), (MEAN, STD, True), 5),
                                                   (scene, (640, 640), (1024, 1024), None, 3),
                                                   (scene[:3000, :4000].float() + 0.25, (1333, 1333), (1344, 1344), (MEAN, STD, True), 1)):
        sh, sw = int(src.shape[0]), int(src.shape[1])
        tl = tiles if sh == H else slice_bboxes(sh, sw, 1024, 1024, 0.25, 0.25)
        og = torch.tensor([[t[0], t[1]] for t in tl], dtype=torch.int32, device=dev)
        for b0 in range(0, len(tl), 16):
            got = ops.slice_resize_pad(src, og[b0:b0 + 16], (1024, 1024), new_hw, pad_hw, PAD, normalise=normalise)
            again = ops.slice_resize_pad(src, og[b0:b0 + 16], (1024, 1024), new_hw, pad_hw, PAD, normalise=normalise)
            assert torch.equal(got, again)                                      # a second launch is bit-identical
            for j in range(0, got.shape[0], stride):
                x0, y0, x1, y1 = tl[b0 + j]
                want = ops.resize_pad(src[y0:y1, x0:x1].contiguous(), new_hw, pad_hw, PAD, normalise=normalise)
                assert torch.equal(got[j], want), (new_hw, normalise is not None, b0 + j)
                checked += 1
    print(f'slice_resize_pad: {checked} tiles compared exactly with per-crop resize_pad')
    assert origins.shape[0] == 176 and checked > 250


def _blob_masks(k, h, w, dev, seed):
    """instance-like masks: an ellipse per instance, a rectangular hole, a sprinkle of noise in a corner; plus the edge
    cases empty / full / one pixel"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    yy = torch.arange(h, device=dev).view(1, h, 1).float()
    xx = torch.arange(w, device=dev).view(1, 1, w).float()
    cy, cx = (torch.rand(k, generator=g) * h).to(dev).view(k, 1, 1), (torch.rand(k, generator=g) * w).to(dev).view(k, 1, 1)
    ry, rx = (8 + torch.rand(k, generator=g) * h / 3).to(dev).view(k, 1, 1), (8 + torch.rand(k, generator=g) * w / 3).to(dev).view(k, 1, 1)
    m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    m &= ~(((yy - cy).abs() < ry / 4) & ((xx - cx).abs() < rx / 5))
    noise = (torch.rand((k, 48, 48), generator=g) < 0.3).to(dev)
    m[:, :48, -48:] |= noise
    m[0] = False
    m[1] = True
    m[2] = False
    m[2, h - 1, w - 1] = True
    return m


def _strings(ops, counts, n):
    k = int(n.shape[0])
    flat_cap = 2 * int(n.clamp(min=0).sum().item()) + 16
    _, offs, flat = ops.rle_to_string(counts, n, k, flat_cap)
    o = offs.cpu().tolist()
    assert o[-1] <= flat_cap
    buf = flat[:o[-1]].cpu().numpy().tobytes()
    return [buf[o[i]:o[i + 1]] for i in range(k)]


def test_rle_shift_at_scale_against_run_domain_restatement(dev):
    """300 instances of 1024 x 1024 tile masks into an 8192 x 9000 scene (a dense canvas per instance would be 74 MB, 22 GB
    in all): strings equal to the host restatement's run-domain result; placements include every border"""
    from rsprompter_amd import ops
    from rsprompter_amd.rle import counts_to_string
    k, h, w, H, W = 300, 1024, 1024, 8192, 9000
    masks = _blob_masks(k, h, w, dev, 0)
    rng = np.random.default_rng(0)
    offs = np.stack([rng.integers(0, W - w + 1, k), rng.integers(0, H - h + 1, k)], 1)
    offs[:6] = [[0, 0], [W - w, H - h], [W - w, 0], [0, H - h], [17, 0], [W - w, 33]]
    counts, n = ops.mask_rle_counts(masks, cap=4096)
    off_d = torch.tensor(offs, dtype=torch.int32, device=dev)
    out, no = ops.rle_shift(counts, n, off_d, (h, w), (H, W), 4)
    need = int((-no).max().item())
    assert need > 4                                                          # too small: reported, then the retry fits
    out, no = ops.rle_shift(counts, n, off_d, (h, w), (H, W), need)
    assert int(no.min().item()) > 0 and int(no.max().item()) == need
    out2, no2 = ops.rle_shift(counts, n, off_d, (h, w), (H, W), need)
    got = _strings(ops, out, no)
    assert got == _strings(ops, out2, no2) and torch.equal(no, no2)          # a second launch is bit-identical
    ch, nh = counts.cpu().tolist(), n.cpu().tolist()
    pieces = 0
    for i in range(k):
        want = ref.rle_shift_counts(ch[i][:nh[i]], h, w, (int(offs[i, 0]), int(offs[i, 1])), (H, W))
        assert sum(want) == H * W
        pieces += len(want)
        assert got[i] == counts_to_string(want), i
    print(f'rle_shift: {k} instances, {int(n.sum())} tile runs -> {pieces} scene runs, strings equal')


def test_rle_shift_and_paste_against_dense_paste_on_a_small_scene(dev):
    from rsprompter_amd import ops
    from rsprompter_amd.rle import counts_to_string
    k, h, w, H, W = 8, 512, 512, 1200, 1600
    masks = _blob_masks(k, h, w, dev, 1)
    offs = [(0, 0), (W - w, H - h), (W - w, 0), (0, H - h), (100, 200), (1088, 3), (511, 688), (640, 344)]
    off_d = torch.tensor(offs, dtype=torch.int32, device=dev)
    counts, n = ops.mask_rle_counts(masks, cap=4096)
    out, no = ops.rle_shift(counts, n, off_d, (h, w), (H, W), 8192)
    got = _strings(ops, out, no)
    dense = ops.paste_tiles(masks, off_d, (H, W))
    mh = masks.cpu().numpy()
    for i in range(k):
        canvas = ref.shift_masks(mh[i:i + 1], offs[i], (H, W))[0]
        assert np.array_equal(dense[i].cpu().numpy(), canvas), i
        assert got[i] == counts_to_string(ref.rle_counts_np(canvas)), i
    from rsprompter_amd.rle import encode_mask_results
    assert [r['counts'] for r in encode_mask_results(dense)] == got


def test_run_table_pipelines_retry_from_a_capacity_that_is_too_small(dev):
    """the host loops around rsp_mask_rle, rsp_rle_shift, rsp_rle_union and rsp_rle_to_string (rsprompter_amd/rle.py) on the
    device: from cap = 2 / flat_cap = 1 each retries and ends with the tables and strings of the default capacities"""
    import _run_table_cases as cases
    from rsprompter_amd import ops
    cases.check_capacity_retries(ops, dev)


def test_mask_forms_round_trip_through_the_run_table(dev):
    """the conversions between a caller's masks and the run table (rsprompter_amd/rle.py "mask forms") on the device: exact
    round trips, the bit planes, mixed sizes, k = 0, the capacity retry, the refusals and the host reads of every form"""
    import _run_table_cases as cases
    from rsprompter_amd import ops, rle
    cases.check_mask_forms(ops, rle, dev, pytest)


# --------------------------------------------------------------------------------------------------------- end to end
def _cfg():
    from rsprompter_amd.config import Config
    from rsprompter_amd.default_configs import rsprompter_anchor
    cfg = Config(dict(
        model=rsprompter_anchor('base', 10),
        test_dataloader=dict(dataset=dict(pipeline=[
            dict(type='LoadImageFromFile', backend_args=None, to_float32=True),
            dict(type='Resize', scale=(1024, 1024), keep_ratio=True),
            dict(type='Pad', size=(1024, 1024), pad_val=dict(img=PAD, masks=0)),
            dict(type='PackDetInputs', meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor'))]))))
    return cfg


@pytest.fixture(scope='module')
def model(dev):
    import rsprompter_amd as ra
    from rsprompter_amd.synth import synth_state_dict
    cfg = _cfg()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = ra.build_model(cfg)
    m.load_state_dict(synth_state_dict(m, seed=0), strict=True)
    m.cfg = cfg
    return m.to(dev)


def _rle_strings(sample):
    return [r['counts'] for r in sample.pred_instances.masks]


def test_inference_large_image_on_the_demo_scene_equals_per_crop_api_plus_restatement(dev, model):
    """expected value: apis.inference_detector on the six host-cut 640 x 640 crops (each resized to 1024 by the existing
    front end), then the restatement: shift, oracle.glue.batched_nms, dense paste, RLE.  Exact, for batch_size 1 and 4."""
    from oracle import glue
    from rsprompter_amd import apis
    from rsprompter_amd.large_image import inference_large_image
    from rsprompter_amd.rle import counts_to_string, encode_mask_results
    bgr = apis.TestPipeline._decode(SCENE)
    H, W = bgr.shape[:2]
    assert (H, W) == (788, 1400)
    tiles = ref.slice_bboxes(H, W, 640, 640, 0.25, 0.25)
    assert len(tiles) == 6
    offsets = [(t[0], t[1]) for t in tiles]
    per_tile = []
    for x0, y0, x1, y1 in tiles:
        s = apis.inference_detector(model, np.ascontiguousarray(bgr[y0:y1, x0:x1]))
        p = s.pred_instances
        per_tile.append(dict(bboxes=p.bboxes.cpu().numpy(), scores=p.scores.cpu().numpy(), labels=p.labels.cpu().numpy(),
                             masks=p.masks.cpu().numpy()))
    keep, boxes, scores, labels, tile = ref.merge(per_tile, offsets, (H, W), glue.batched_nms, 0.25)
    all_masks = [m for r in per_tile for m in r['masks']]
    want_rle = [counts_to_string(ref.rle_counts_np(ref.shift_masks(all_masks[i][None], offsets[tile[i]], (H, W))[0])) for i in keep]
    n_all, contributing = len(scores), len(set(tile[keep].tolist()))
    nonempty = sum(bool(all_masks[i].any()) for i in keep)
    print(f'demo scene: {n_all} instances from 6 tiles -> {len(keep)} kept ({n_all - len(keep)} suppressed by the merge), '
          f'{contributing} tiles contribute, {nonempty} kept masks non-empty')
    assert contributing >= 2 and len(keep) < n_all and nonempty >= 1           # non-vacuity
    for bs in (1, 4):
        out, patches, start = inference_large_image(model, SCENE, batch_size=bs, return_patches=True)
        assert start == offsets and len(patches) == 6 and out.ori_shape == (H, W)
        p = out.pred_instances
        exact = (out.keep.cpu().numpy().tolist() == keep.tolist() and np.array_equal(p.labels.cpu().numpy(), labels[keep])
                 and np.array_equal(p.scores.cpu().numpy(), scores[keep]) and np.array_equal(p.bboxes.cpu().numpy(), boxes[keep]))
        if not exact:                                                           # figures first, then the assertion
            nb = min(len(p.scores), len(keep))
            print(f'batch_size={bs}: kept {len(p.scores)} vs {len(keep)}, max |score diff| '
                  f'{np.abs(p.scores.cpu().numpy()[:nb] - scores[keep][:nb]).max():.3e}, max |box diff| '
                  f'{np.abs(p.bboxes.cpu().numpy()[:nb] - boxes[keep][:nb]).max():.3e}')
        assert exact, f'batch_size={bs}'
        got = _rle_strings(out)
        assert all(m['size'] == [H, W] for m in p.masks)
        assert got == want_rle, f'batch_size={bs}: {sum(a != b for a, b in zip(got, want_rle))} strings differ'
    dense = inference_large_image(model, bgr, batch_size=4, masks='dense')
    dm = dense.pred_instances.masks
    assert dm.dtype == torch.bool and tuple(dm.shape) == (len(keep), H, W) and dm.device.type == dev.type
    assert [r['counts'] for r in encode_mask_results(dm)] == want_rle
    assert torch.equal(dense.pred_instances.bboxes, out.pred_instances.bboxes)


def _mosaic(H, W):
    """a 4096 x 5000 scene from the committed NWPU images, repeated row by row"""
    from rsprompter_amd.apis import TestPipeline
    d = os.path.join(HERE, 'golden', 'coco_nwpu', 'imgs')
    imgs = [TestPipeline._decode(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.jpg')]
    scene = np.zeros((H, W, 3), np.uint8)
    y, i = 0, 0
    while y < H:
        x = 0
        while x < W:
            im = imgs[i % len(imgs)]
            i += 1
            hh, ww = min(im.shape[0], H - y), min(im.shape[1], W - x)
            scene[y:y + hh, x:x + ww] = im[:hh, :ww]
            x += ww
        y += 383                                                               # the shortest image: rows overlap, no gaps
    return scene


def test_inference_large_image_on_a_synthetic_scene_runs_in_less_memory_than_the_dense_form(dev, model):
    from rsprompter_amd import ops
    from rsprompter_amd.large_image import inference_large_image
    H, W = 4096, 5000
    scene = _mosaic(H, W)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = inference_large_image(model, scene, patch_size=1024, batch_size=4, masks='rle')
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    K = len(out.pred_instances.scores)
    dense_bytes = K * H * W
    print(f'synthetic {H} x {W} scene, 35 tiles of 1024: {K} kept instances; peak device memory {peak / 2 ** 20:.0f} MiB '
          f'(model and scene resident before the call: {base / 2 ** 20:.0f} MiB) against {dense_bytes / 2 ** 20:.0f} MiB for the '
          'kept masks alone in the dense form')
    assert K > 0 and len(out.pred_instances.masks) == K
    assert peak < dense_bytes
    # the strings decode to masks of the source tile masks' areas
    out2, patches, start = inference_large_image(model, scene, patch_size=1024, batch_size=4, masks='rle', return_patches=True)
    assert len(patches) == 35 and torch.equal(out2.keep, out.keep) and _rle_strings(out2) == _rle_strings(out)
    tile_area = torch.cat([p.pred_instances.masks.sum((1, 2)) for p in patches], 0)[out.keep].cpu()
    del patches, out2
    strings = _rle_strings(out)
    nw = (H * W + 63) // 64
    areas = []
    for i0 in range(0, K, 256):
        chunk = strings[i0:i0 + 256]
        offs = torch.tensor(np.cumsum([0] + [len(s) for s in chunk]), dtype=torch.int64, device=dev)
        flat = torch.frombuffer(bytearray(b''.join(chunk)), dtype=torch.uint8).to(dev)
        counts, n = ops.rle_from_string(flat, offs, cap=8192)
        woff = torch.arange(len(chunk) + 1, dtype=torch.int64, device=dev) * nw
        _, area, _ = ops.rle_to_bits(counts, n, woff)
        areas.append(area.cpu())
    areas = torch.cat(areas, 0)
    assert torch.equal(areas, tile_area.to(areas.dtype)) and int(areas.max()) > 0


def test_cli_writes_one_json_per_scene_with_the_api_counts(dev, model, tmp_path):
    """python -m rsprompter_amd.large_image in a fresh child process (config file + checkpoint on disk)"""
    from rsprompter_amd.default_configs import rsprompter_anchor
    from rsprompter_amd.large_image import inference_large_image, pred2dict
    ckpt = str(tmp_path / 'epoch_1.pth')
    torch.save(dict(meta=dict(epoch=1), state_dict={k: v.cpu() for k, v in model.state_dict().items()}), ckpt)
    (tmp_path / 'cfg.py').write_text(
        f'model = {rsprompter_anchor("base", 10)!r}\n'
        'test_dataloader = dict(dataset=dict(pipeline=[\n'
        "    dict(type='LoadImageFromFile', backend_args=None, to_float32=True),\n"
        "    dict(type='Resize', scale=(1024, 1024), keep_ratio=True),\n"
        f"    dict(type='Pad', size=(1024, 1024), pad_val=dict(img={PAD!r}, masks=0)),\n"
        "    dict(type='PackDetInputs', meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor'))]))\n")
    api = inference_large_image(model, SCENE, batch_size=2)
    thr = float(api.pred_instances.scores.median())                              # the filter keeps about half
    want = pred2dict(api, thr)
    out_dir = tmp_path / 'out'
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'rsprompter_amd.large_image', SCENE, str(tmp_path / 'cfg.py'), ckpt, '--out-dir',
                        str(out_dir), '--score-thr', repr(thr), '--batch-size', '2', '--device', str(dev)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert os.listdir(out_dir) == ['large_image.json']
    got = json.loads((out_dir / 'large_image.json').read_text())
    assert set(got) == {'labels', 'scores', 'bboxes', 'masks'}
    assert 0 < len(got['labels']) == len(want['labels']) < len(api.pred_instances.scores) and got['labels'] == want['labels']
    assert len(got['masks']) == len(got['labels']) and got['masks'][0]['size'] == [788, 1400]
    assert isinstance(got['masks'][0]['counts'], str) and got['masks'] == want['masks']
