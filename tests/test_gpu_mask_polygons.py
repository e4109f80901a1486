"""-m gpu: polygon export on the device (csrc/mask_polygons.hip, rle.runs_to_polygons, apis.masks_to_polygons, large_image
masks='polygons').  The case bodies are tests/_mask_polygons_cases.py, the same the emulator tier runs; the
tests at scale use the sequential reference where it is fast enough (256 x 256) and its vectorised properties beyond
(tests/_mask_polygons_ref.py check_properties: area identity, ring counts and parents against scipy.ndimage.label, even-odd
refill equal to the mask).  Everything is exact."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _large_image_ref as lref  # noqa: E402
import _mask_polygons_cases as cases  # noqa: E402
import _mask_polygons_ref as pref  # noqa: E402

SCENE = os.path.join(HERE, 'golden', 'large_image', 'large_image.jpg')
PAD = (0.406 * 255, 0.456 * 255, 0.485 * 255)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _per_instance(arrays, i):
    """instance i of the six device arrays as host arrays (verts, ring_offs from 0, parent, area2)"""
    verts, ring_offs, _, parent, area2, ioffs = (a.cpu().numpy() for a in arrays)
    r0, r1 = int(ioffs[i]), int(ioffs[i + 1])
    return verts[ring_offs[r0]:ring_offs[r1]], ring_offs[r0:r1 + 1] - ring_offs[r0], parent[r0:r1], area2[r0:r1]


# ------------------------------------------------------------------------------------------------------- the case module
def test_known_answers(dev):
    from rsprompter_amd import ops
    cases.check_known_answers(ops, dev)


def test_every_case_mask_alone(dev):
    from rsprompter_amd import ops
    cases.check_single_masks(ops, dev)


def test_batch_with_invalid_rows_and_a_second_launch(dev):
    from rsprompter_amd import ops
    cases.check_batch(ops, dev)


def test_no_rows_and_no_rings(dev):
    from rsprompter_amd import ops
    cases.check_no_rows_and_no_rings(ops, dev)


def test_bad_arguments_are_refused(dev):
    from rsprompter_amd import ops
    cases.check_refuses_bad_arguments(ops, dev, pytest)


def test_the_piece_table_its_two_consumers_and_their_host_reads(dev):
    from rsprompter_amd import ops
    cases.check_run_pieces(ops, dev)


def test_masks_to_polygons_forms(dev):
    from rsprompter_amd import apis, rle
    cases.check_api_forms(apis, rle, dev)
    cases.check_api_refusals(apis, dev, pytest)


# ---------------------------------------------------------------------------------------------------------------- scale
def test_noise_256_against_the_sequential_reference(dev):
    from rsprompter_amd import rle
    m = np.random.default_rng(256).random((256, 256)) < 0.5
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(m[None]).to(dev))
    got = rle.runs_to_polygons(counts, n, (256, 256))
    want = pref.check_traced(m)
    print(f'256 x 256 noise: {len(want)} rings, {sum(len(r[0]) for r in want)} vertices, longest {max(len(r[0]) for r in want)}')
    cases.assert_arrays_equal(got, pref.flatten([want]), 'noise 256')
    assert _same(got, rle.runs_to_polygons(counts, n, (256, 256)))


def test_eight_masks_of_50000_runs_hold_the_ring_properties(dev):
    """uniform noise smoothed at sigma = 1 and cut at its 95th (islands) or 5th (holes) percentile: about 55 000 runs a mask"""
    from scipy import ndimage
    from rsprompter_amd import rle
    rng = np.random.default_rng(1024)
    masks = []
    for i in range(8):
        f = ndimage.gaussian_filter(rng.random((1024, 1024)), 1.0)
        masks.append(f > np.quantile(f, 0.95 if i % 2 == 0 else 0.05))
    masks = np.stack(masks)
    counts, n, n_host, _ = rle.encode_runs(torch.from_numpy(masks).to(dev))
    print('runs per mask:', n_host.tolist())
    assert all(40000 <= int(v) <= 70000 for v in n_host.tolist())
    got = rle.runs_to_polygons(counts, n, (1024, 1024))
    assert _same(got, rle.runs_to_polygons(counts, n, (1024, 1024)))              # a second launch is bit-identical
    assert got[2].cpu().tolist() == sorted(got[2].cpu().tolist()) and int(got[5][-1]) == int(got[2].shape[0])
    outer = holes = 0
    for i in range(8):
        v, o, p, a = _per_instance(got, i)
        no, nh = pref.check_properties(masks[i], v, o, p, a)
        outer, holes = outer + no, holes + nh
    print(f'{int(got[2].shape[0])} rings ({outer} outer, {holes} holes), {int(got[0].shape[0])} vertices')
    assert outer > 20000 and holes > 20000


def test_300_tile_instances_shifted_into_a_scene(dev):
    """the run table rsp_rle_shift writes for an 8 192 x 9 000 scene: ring vertices = the tile rings + the offset"""
    from scipy import ndimage
    from rsprompter_amd import rle
    rng = np.random.default_rng(300)
    th, tw, H, W, k = 128, 128, 8192, 9000, 300
    f = ndimage.gaussian_filter(rng.random((k, th, tw)), (0, 3, 3))
    tiles = f > np.quantile(f, 0.55)
    tiles[7], tiles[8] = True, False                                               # a full and an empty tile mask
    offs = np.stack([rng.integers(0, W - tw + 1, k), rng.integers(0, H - th + 1, k)], 1).astype(np.int32)
    offs[0], offs[1], offs[2] = (0, 0), (W - tw, H - th), (W - tw, 0)               # the scene's corners
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(tiles).to(dev))
    off_d = torch.from_numpy(offs).to(dev)
    sc, sn, _, _ = rle.shift_runs(counts, n, off_d, (th, tw), (H, W))
    tile = rle.runs_to_polygons(counts, n, (th, tw))
    scene = rle.runs_to_polygons(sc, sn, (H, W))
    assert _same(scene, rle.runs_to_polygons(sc, sn, (H, W)))
    for j in (1, 2, 3, 4, 5):
        assert torch.equal(scene[j], tile[j])
    vert_inst = tile[2][torch.searchsorted(tile[1], torch.arange(tile[0].shape[0], device=dev), right=True) - 1].to(torch.int64)
    assert torch.equal(scene[0], tile[0] + off_d[vert_inst])
    for i in (0, 5, 7, 8, 299):                                                    # and the tile rings are the reference's
        v, o, p, a = _per_instance(tile, i)
        w = pref.flatten([pref.trace(tiles[i])])
        assert np.array_equal(v, w[0]) and np.array_equal(o, w[1]) and np.array_equal(p, w[3]) and np.array_equal(a, w[4])
    print(f'{k} instances: {int(scene[2].shape[0])} rings, {int(scene[0].shape[0])} vertices, widest row {int(sn.max())} runs')
    assert int(scene[5][9]) == int(scene[5][8]) and int(scene[2].shape[0]) > k


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope='module')
def model(dev):
    import rsprompter_amd as ra
    from rsprompter_amd.config import Config
    from rsprompter_amd.default_configs import rsprompter_anchor
    from rsprompter_amd.synth import synth_state_dict
    cfg = Config(dict(
        model=rsprompter_anchor('base', 10),
        test_dataloader=dict(dataset=dict(pipeline=[
            dict(type='LoadImageFromFile', backend_args=None, to_float32=True),
            dict(type='Resize', scale=(1024, 1024), keep_ratio=True),
            dict(type='Pad', size=(1024, 1024), pad_val=dict(img=PAD, masks=0)),
            dict(type='PackDetInputs', meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor'))]))))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = ra.build_model(cfg)
    m.load_state_dict(synth_state_dict(m, seed=0), strict=True)
    m.cfg = cfg
    return m.to(dev)


def refill_on(dev, per_instance, H, W):
    """the even-odd refill of tests/_mask_polygons_ref.py for a chunk of instances at once, in torch on `dev`: a signed count
    of every ring's vertical edges into [K, H + 1, W + 1], summed along y and x -> bool [K, H, W]"""
    K = len(per_instance)
    d = torch.zeros((K, H + 1, W + 1), dtype=torch.int32, device=dev)
    rings = [(i, r) for i, inst in enumerate(per_instance) for r, _, _ in inst]
    if rings:
        a = np.concatenate([r for _, r in rings], 0).astype(np.int64)
        b = np.concatenate([np.roll(r, -1, 0) for _, r in rings], 0).astype(np.int64)
        inst = np.repeat(np.array([i for i, _ in rings]), [len(r) for _, r in rings])
        v = a[:, 0] == b[:, 0]
        a, b, inst = (torch.from_numpy(t[v]).to(dev) for t in (a, b, inst))
        sign = torch.where(a[:, 1] > b[:, 1], 1, -1).to(torch.int32)
        lo, hi = torch.minimum(a[:, 1], b[:, 1]), torch.maximum(a[:, 1], b[:, 1])
        d.index_put_((inst, lo, a[:, 0]), sign, accumulate=True)
        d.index_put_((inst, hi, a[:, 0]), -sign, accumulate=True)
    return torch.cumsum(torch.cumsum(d, 1)[:, :H], 2)[:, :, :W] == 1


def decode_on(dev, ops, strings, H, W):
    """COCO strings -> bool [K, H, W] on `dev`: rsp_rle_from_string, then the run boundaries as +1 / -1 into the
    column-major stream and a running sum"""
    K = len(strings)
    offs = torch.from_numpy(np.cumsum([0] + [len(s) for s in strings]).astype(np.int64)).to(dev)
    flat = torch.from_numpy(np.frombuffer(b''.join(strings), dtype=np.uint8).copy()).to(dev)
    counts, n = ops.rle_from_string(flat, offs, cap=8192)
    ends = torch.cumsum(counts[:K].to(torch.int64), 1)
    idx = torch.arange(counts.shape[1], device=dev)[None].expand(K, -1)
    live = idx < (n[:K, None] - 1)                                                 # the last run ends at H * W: no change
    rows = torch.arange(K, device=dev)[:, None].expand_as(idx)[live]
    sign = torch.where(idx[live] % 2 == 0, 1, -1).to(torch.int32)
    d = torch.zeros((K, H * W + 1), dtype=torch.int32, device=dev)
    d.index_put_((rows, ends[live]), sign, accumulate=True)
    return (torch.cumsum(d, 1)[:, :H * W] == 1).view(K, W, H).transpose(1, 2)


def test_the_two_device_decoders_of_this_file_against_numpy(dev):
    from rsprompter_amd import ops, rle
    rng = np.random.default_rng(4)
    masks = [rng.random((13, 17)) < d for d in (0.0, 0.3, 0.6, 1.0)]
    want = torch.from_numpy(np.stack(masks)).to(dev)
    assert torch.equal(refill_on(dev, [pref.trace(m) for m in masks], 13, 17), want)
    assert torch.equal(decode_on(dev, ops, [rle.counts_to_string(lref.rle_counts_np(m)) for m in masks], 13, 17), want)


@pytest.mark.parametrize('mode', ['nms', 'seam_mask'])
def test_demo_scene_polygons_refill_to_the_rle_result(dev, model, mode):
    """inference_large_image on the committed 788 x 1400 scene with seeded synthetic weights (two 1024-pixel tiles):
    masks='polygons', refilled by the even-odd rule, equals masks='rle' of the same call, instance by instance; both sides
    are decoded on the device, 32 instances at a time"""
    from rsprompter_amd import ops
    from rsprompter_amd.large_image import inference_large_image, pred2geojson
    kw = dict(patch_size=1024, batch_size=2, merge_nms_type=mode)
    poly = inference_large_image(model, SCENE, masks='polygons', **kw)
    rle_out = inference_large_image(model, SCENE, masks='rle', **kw)
    H, W = 788, 1400
    assert torch.equal(poly.keep, rle_out.keep) and torch.equal(poly.pred_instances.bboxes, rle_out.pred_instances.bboxes)
    rings, strings = poly.pred_instances.masks, [r['counts'] for r in rle_out.pred_instances.masks]
    assert len(rings) == len(strings) > 0
    nonempty = 0
    for i0 in range(0, len(rings), 32):
        want = decode_on(dev, ops, strings[i0:i0 + 32], H, W)
        assert torch.equal(refill_on(dev, rings[i0:i0 + 32], H, W), want)
        nonempty += int(want.flatten(1).any(1).sum())
    first = next(r for r in rings if r)
    v, o, _, p, a, _ = pref.flatten([first])
    pref.check_properties(refill_on(dev, [first], H, W)[0].cpu().numpy(), v, o, p, a)
    print(f'{mode}: {len(rings)} instances ({nonempty} non-empty), {sum(len(r) for r in rings)} rings')
    assert nonempty >= 1
    fc = pred2geojson(poly, float(poly.pred_instances.scores.max()), (500000.0, 0.3, 0.0, 4000000.0, 0.0, -0.3))
    assert len(fc['features']) >= 1 and fc['features'][0]['geometry']['type'] in ('Polygon', 'MultiPolygon')
