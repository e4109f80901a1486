"""-m gpu: oriented boxes on the device (csrc/mask_obb.hip, ops.mask_hull / ops.hull_min_rect, rle.runs_to_obb,
apis.masks_to_obb, large_image oriented_boxes=True).  The case bodies are tests/_mask_obb_cases.py, the same the
emulator tier runs; the tests at scale use the sequential reference (tests/_mask_obb_ref.py) on the pixels where that is fast
enough (256 x 256) and on the vertices of the exact outer rings of DESIGN §14.7 beyond (a mask and its outer rings have one
hull).  Everything integer is exact; the float forms are held to rtol = 1e-12."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _mask_obb_cases as cases  # noqa: E402
import _mask_obb_ref as oref  # noqa: E402

SCENE = os.path.join(HERE, 'golden', 'large_image', 'large_image.jpg')
PAD = (0.406 * 255, 0.456 * 255, 0.485 * 255)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _want_from_points(points):
    """reference (hull, area2, edge, q) of a point set given as an int array [n, 2]"""
    ring = oref.hull_of_points(sorted(set(map(tuple, np.asarray(points).tolist()))))
    edge, q, _ = oref.min_rect(ring)
    return ring, (oref.area2_of(ring) if ring else 0), edge, q


def _check_hull_properties(ring, a2, edge, q, points, popcount):
    """strictly convex and canonical, around every point, area2 >= 2 popcount, the rectangle the reference's for this hull"""
    m = len(ring)
    assert m >= 4 and ring[0] == min(ring) and a2 == oref.area2_of(ring) >= 2 * popcount
    assert all(oref._cross(ring[i], ring[(i + 1) % m], ring[(i + 2) % m]) > 0 for i in range(m))
    r = np.array(ring, np.int64)
    rn = np.roll(r, -1, 0)
    pts = np.asarray(points, np.int64)
    for j in range(m):
        assert ((rn[j, 0] - r[j, 0]) * (pts[:, 1] - r[j, 1]) - (rn[j, 1] - r[j, 1]) * (pts[:, 0] - r[j, 0]) >= 0).all()
    we, wq, _ = oref.min_rect(ring)
    assert (edge, tuple(q)) == (we, tuple(wq))


# ------------------------------------------------------------------------------------------------------- the case module
def test_known_answers(dev):
    from rsprompter_amd import ops
    cases.check_known_answers(ops, dev)


def test_every_case_mask_alone(dev):
    from rsprompter_amd import ops
    cases.check_single_masks(ops, dev)


def test_ties_go_to_the_lowest_edge(dev):
    from rsprompter_amd import ops
    cases.check_ties(ops, dev)


def test_column_counts_around_every_path_boundary(dev):
    from rsprompter_amd import ops
    print(cases.check_path_boundaries(ops, dev))


def test_quarter_disc_with_a_spike_prunes_slowly_and_correctly(dev):
    from rsprompter_amd import ops
    rounds = cases.check_slow_pruning(ops, dev, 100)
    print('pruning rounds (upper, lower):', rounds)
    assert rounds[0] >= 8 and rounds[1] <= 2


def test_wide_coordinates_compare_beyond_64_bits(dev):
    from rsprompter_amd import ops
    cases.check_wide_coordinates(ops, dev)


def test_batch_with_invalid_rows_and_a_second_launch(dev):
    from rsprompter_amd import ops
    cases.check_batch(ops, dev)
    cases.check_no_rows_and_no_pixels(ops, dev)


def test_hull_min_rect_on_hand_made_polygons(dev):
    from rsprompter_amd import ops
    cases.check_hull_min_rect(ops, dev)


def test_bad_arguments_are_refused(dev):
    from rsprompter_amd import ops
    cases.check_refuses_bad_arguments(ops, dev, pytest)


def test_masks_to_obb_forms(dev):
    from rsprompter_amd import apis, rle
    cases.check_api_forms(apis, rle, dev)
    cases.check_api_refusals(apis, rle, dev, pytest)


# ---------------------------------------------------------------------------------------------------------------- scale
def test_noise_256_against_the_sequential_reference(dev):
    from rsprompter_amd import rle
    rng = np.random.default_rng(256)
    masks = [rng.random((256, 256)) < d for d in (0.5, 0.001)]
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(np.stack(masks)).to(dev))
    got = rle.runs_to_obb(counts, n, (256, 256))
    want = [oref.check(m) for m in masks]
    print('256 x 256 noise: hull vertices', [len(w[0]) for w in want], 'edges', [w[2] for w in want])
    cases.assert_arrays_equal(got, cases.flatten(want), 'noise 256')
    assert _same(got, rle.runs_to_obb(counts, n, (256, 256)))


def test_eight_masks_of_50000_runs_hold_the_hull_properties(dev):
    """the eight 1024 x 1024 masks of DESIGN §14.7 (about 55 000 runs each): properties on all eight, and mask 0 against the
    sequential reference applied to the vertices of its exact outer rings"""
    from scipy import ndimage
    from rsprompter_amd import ops, rle
    rng = np.random.default_rng(1024)
    masks = []
    for i in range(8):
        f = ndimage.gaussian_filter(rng.random((1024, 1024)), 1.0)
        masks.append(f > np.quantile(f, 0.95 if i % 2 == 0 else 0.05))
    masks = np.stack(masks)
    counts, n, n_host, _ = rle.encode_runs(torch.from_numpy(masks).to(dev))
    assert all(40000 <= int(v) <= 70000 for v in n_host.tolist())
    got = rle.runs_to_obb(counts, n, (1024, 1024))
    assert _same(got, rle.runs_to_obb(counts, n, (1024, 1024)))                    # a second launch is bit-identical
    rounds = ops.mask_hull(counts, n, 1024, 1024, with_rounds=True)[3].cpu().tolist()
    verts, offs, a2, edge, q = (t.cpu().numpy() for t in got)
    pv, po, _, _, pa, pio = (t.cpu().numpy() for t in rle.runs_to_polygons(counts, n, (1024, 1024)))
    print('hull vertices per mask:', np.diff(offs).tolist(), 'pruning rounds (upper / lower):', rounds)
    for i in range(8):
        ring = [tuple(v) for v in verts[offs[i]:offs[i + 1]].tolist()]
        r0, r1 = int(pio[i]), int(pio[i + 1])
        outer = np.concatenate([pv[po[r]:po[r + 1]] for r in range(r0, r1) if pa[r] > 0], 0)
        _check_hull_properties(ring, int(a2[i]), int(edge[i]), q[i].tolist(), outer, int(masks[i].sum()))
        if i == 0:
            assert (ring, int(a2[i]), int(edge[i]), tuple(q[i].tolist())) == _want_from_points(outer)


def test_300_tile_instances_shifted_into_a_scene(dev):
    """the run table rsp_rle_shift writes for an 8 192 x 9 000 scene: hull = tile hull + offset, the same edge, and q's amin /
    amax / bmin / bmax moved by the offset's products with e and nrm"""
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
    tile = rle.runs_to_obb(counts, n, (th, tw))
    scene = rle.runs_to_obb(sc, sn, (H, W))
    assert _same(scene, rle.runs_to_obb(sc, sn, (H, W)))
    for j in (1, 2, 3):
        assert torch.equal(scene[j], tile[j])
    vert_inst = torch.searchsorted(tile[1], torch.arange(tile[0].shape[0], device=dev), right=True) - 1
    assert torch.equal(scene[0], tile[0] + off_d[vert_inst])
    o64, ex, ey = off_d.to(torch.int64), tile[4][:, 0], tile[4][:, 1]
    da, db = o64[:, 0] * ex + o64[:, 1] * ey, o64[:, 1] * ex - o64[:, 0] * ey
    live = (tile[3] >= 0).to(torch.int64)
    moved = tile[4] + torch.stack([0 * da, 0 * da, da, da, db, db], 1) * live[:, None]
    assert torch.equal(scene[4], moved)
    for i in (0, 5, 7, 8, 299):                                                    # and the tile results are the reference's
        g = [t.cpu() for t in tile]
        ring = [tuple(v) for v in g[0][g[1][i]:g[1][i + 1]].tolist()]
        assert (ring, int(g[2][i]), int(g[3][i]), tuple(g[4][i].tolist())) == oref.obb(tiles[i])
    print(f'{k} instances: {int(scene[0].shape[0])} hull vertices, widest row {int(sn.max())} runs')
    assert int(scene[3][8]) == -1 and int(scene[1][9]) == int(scene[1][8]) and int(scene[0].shape[0]) > 4 * k


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


@pytest.mark.parametrize('mode', ['nms', 'seam_mask'])
def test_demo_scene_oriented_boxes_are_those_of_the_exact_rings(dev, model, mode):
    """inference_large_image on the committed 788 x 1400 scene with seeded synthetic weights: oriented_boxes=True with
    masks='polygons' and with masks='rle' give the same boxes; every box holds every ring vertex of its instance; for six
    instances the box is the reference's rectangle of the hull of the instance's own ring vertices (the sequential reference
    takes a second per instance of this size)"""
    from rsprompter_amd.large_image import inference_large_image, pred2dict
    kw = dict(patch_size=1024, batch_size=2, merge_nms_type=mode)
    poly = inference_large_image(model, SCENE, masks='polygons', oriented_boxes=True, **kw)
    rle_out = inference_large_image(model, SCENE, masks='rle', oriented_boxes=True, **kw)
    p = poly.pred_instances
    K = len(p.masks)
    assert p.obb.shape == (K, 4, 2) and p.obb.dtype == np.float64 and K > 0
    assert np.array_equal(p.obb, rle_out.pred_instances.obb, equal_nan=True)
    js = pred2dict(rle_out)
    assert len(js['obb']) == len(js['labels']) == K and set(js) == {'labels', 'scores', 'bboxes', 'masks', 'obb'}
    live = [i for i in range(K) if p.masks[i]]
    assert live and all(np.isnan(p.obb[i]).all() == (i not in live) for i in range(K))
    for i in live:                                        # inside all four sides, to a rounding of coordinates below 2^11
        pts = np.concatenate([r for r, _, _ in p.masks[i]], 0).astype(np.float64)
        c, cn = p.obb[i], np.roll(p.obb[i], -1, 0)
        side = (cn[None, :, 0] - c[None, :, 0]) * (pts[:, None, 1] - c[None, :, 1]) - \
            (cn[None, :, 1] - c[None, :, 1]) * (pts[:, None, 0] - c[None, :, 0])
        assert (side >= -1e-6).all(), i
    some = live[::max(len(live) // 6, 1)][:6]
    wants = [_want_from_points(np.unique(np.concatenate([r for r, _, _ in p.masks[i]], 0), axis=0)) for i in some]
    wc, _ = cases.want_floats(wants)
    assert cases.close(p.obb[some], wc)
    print(f'{mode}: {K} instances, {len(live)} non-empty, compared {some}, hull vertices {[len(w[0]) for w in wants]}')
