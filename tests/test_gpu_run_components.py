"""-m gpu: run-domain connected components on the device (csrc/run_components.hip, ops.rle_components, rle.runs_components /
split_runs / clean_runs, apis.remove_small_regions on RLE dicts, apis.masks_to_obb(per_component=True), apis.mask_components,
large_image min_mask_region_area).  The case bodies are tests/_run_components_cases.py, the same the emulator
tier runs.  At scale the flood-fill reference (tests/_run_components_ref.py) is used where it is fast enough (256 x 256);
beyond, two checks that share no code with the new kernels: the dense labelling of ops.remove_small_regions, and the exact
rings of DESIGN §14.7.  Everything is compared exactly."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _run_components_cases as cases  # noqa: E402
import _run_components_ref as cref  # noqa: E402
import _seam_merge_cases as seam_cases  # noqa: E402


# ------------------------------------------------------------------------------------------------------- the case module
def test_hand_checked_answers(dev):
    from rsprompter_amd import ops
    cases.check_hand_checked(ops, dev)
    cases.check_h1_columns(ops, dev)


def test_every_case_mask_alone(dev):
    from rsprompter_amd import ops
    cases.check_single_masks(ops, dev)


def test_piece_counts_around_a_block_and_a_chunk(dev):
    from rsprompter_amd import ops
    cases.check_block_boundaries(ops, dev)


def test_batch_with_invalid_rows_and_a_second_launch(dev):
    from rsprompter_amd import ops
    cases.check_batch(ops, dev)


def test_components_of_shifted_and_joined_run_tables(dev):
    from rsprompter_amd import ops, rle
    cases.check_shifted_and_joined_tables(ops, rle, dev)


def test_split_runs_gives_one_row_per_component(dev):
    from rsprompter_amd import ops, rle
    cases.check_split(ops, rle, dev)


def test_clean_runs_is_remove_small_regions_in_every_mode(dev):
    from rsprompter_amd import ops, rle
    cases.check_clean_modes(ops, rle, dev)
    cases.check_clean_edge_cases(ops, rle, dev)


def test_status_check_and_refusals(dev):
    from rsprompter_amd import ops, rle
    cases.check_status_and_refusals(ops, rle, dev, pytest)


def test_interface_on_rle_dicts_and_per_component_boxes(dev):
    from rsprompter_amd import apis, rle
    cases.check_api_remove_small_regions(apis, rle, dev)
    cases.check_api_refusals(apis, dev, pytest)
    cases.check_api_components(apis, rle, dev)
    cases.check_api_obb_per_component(apis, rle, dev)


@pytest.mark.parametrize('mode', ['nms', 'seam_mask'])
def test_inference_large_image_cleans_the_scene_masks(dev, mode):
    from rsprompter_amd import large_image as li
    scene = np.random.default_rng(16).integers(0, 256, (45, 70, 3)).astype(np.uint8)
    kw = dict(merge_iou_thr=0.25, merge_nms_type=mode)
    if mode == 'seam_mask':
        kw['seam_iou_thr'] = 0.3
    k, changed = cases.check_pipeline(li, dev, scene, seam_cases.RandomStub((32, 32)).to(dev), 32,
                                      lambda s: s.pred_instances.masks.cpu().numpy(), 6, **kw)
    print(f'{mode}: {k} instances, {changed} changed')


# ---------------------------------------------------------------------------------------------------------------- scale
def _rows_equal(a_counts, a_n, b_counts, b_n):
    """two run tables hold the same rows: equal n, equal counts in front of n"""
    if not torch.equal(a_n, b_n):
        return False
    w = int(a_n.max()) if a_n.numel() else 0
    live = torch.arange(w, device=a_n.device)[None] < a_n[:, None]
    return bool(((a_counts[:, :w] == b_counts[:, :w]) | ~live).all())


def test_noise_256_against_the_flood_fill(dev):
    from rsprompter_amd import rle
    rng = np.random.default_rng(256)
    masks = [rng.random((256, 256)) < d for d in (0.5, 0.05)]
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(np.stack(masks)).to(dev))
    got = rle.runs_components(counts, n, (256, 256))
    cases.assert_components(got, cases.want_arrays(masks, 256, 256), 'noise 256')
    assert cases.same_components(got, rle.runs_components(counts, n, (256, 256)))
    print('256 x 256 noise: components', np.diff(got.comp_offs.cpu().numpy()).tolist(), 'pieces', int(got.piece_comp.shape[0]))
    c, m, _, _, ch = rle.clean_runs(counts, n, (256, 256), 5, 'both')
    want = [cref.remove_small_regions(x, 5, 'both') for x in masks]
    cases.assert_table(c, m, [w[0] for w in want], 'noise 256, cleaned')
    assert ch.cpu().tolist() == [[int(w[1]), int(w[2])] for w in want]


@pytest.fixture(scope='module')
def eight_masks(dev):
    """the eight 1024 x 1024 masks of DESIGN §14.7 (about 55 000 runs each) and their run table"""
    from scipy import ndimage
    from rsprompter_amd import rle
    rng = np.random.default_rng(1024)
    masks = []
    for i in range(8):
        f = ndimage.gaussian_filter(rng.random((1024, 1024)), 1.0)
        masks.append(f > np.quantile(f, 0.95 if i % 2 == 0 else 0.05))
    dense = torch.from_numpy(np.stack(masks)).to(dev)
    counts, n, n_host, _ = rle.encode_runs(dense)
    assert all(40000 <= int(v) <= 70000 for v in n_host.tolist())
    return dense, counts, n


@pytest.mark.parametrize('mode', cases.MODES)
def test_eight_masks_clean_like_the_dense_labelling(dev, eight_masks, mode):
    """clean_runs(encode_runs(m)) == encode_runs(ops.remove_small_regions(m)) bit for bit, flags included: the dense kernels
    label pixels in tiles, the new ones column pieces"""
    from rsprompter_amd import ops, rle
    dense, counts, n = eight_masks
    out, info = ops.remove_small_regions(dense, 100, mode)
    info_h = info.cpu()
    ops.check_region_status(info_h[:, 7].tolist())
    wc, wn, _, _ = rle.encode_runs(out)
    c, m, n_host, _, ch = rle.clean_runs(counts, n, (1024, 1024), 100, mode)
    assert _rows_equal(c, m, wc, wn) and n_host.tolist() == m.cpu().tolist()
    assert torch.equal(ch.cpu(), info_h[:, :2]) and int(ch.sum()) >= 4
    print(mode, 'runs before', n.cpu().tolist(), 'after', m.cpu().tolist())


def test_eight_masks_components_are_the_outer_rings(dev, eight_masks):
    """as many components as rings with parent == -1, and each component's area = half its outer ring's area2 minus its
    holes' (DESIGN §14.7's rings come from edge links and list ranking, not from a labelling)"""
    from rsprompter_amd import rle
    _, counts, n = eight_masks
    comps = rle.runs_components(counts, n, (1024, 1024))
    assert cases.same_components(comps, rle.runs_components(counts, n, (1024, 1024)))
    _, _, ring_inst, parent, area2, inst_ring_offs = rle.runs_to_polygons(counts, n, (1024, 1024))
    outer = (parent < 0).nonzero().view(-1)
    assert int(outer.shape[0]) == int(comps.comp_area.shape[0])
    ring_idx = torch.arange(parent.shape[0], device=dev)
    owner = torch.where(parent < 0, ring_idx, inst_ring_offs[ring_inst.to(torch.int64)] + parent.to(torch.int64))
    total = torch.zeros_like(area2).index_add_(0, owner, area2)[outer]              # holes carry negative area2
    # outer rings are ordered by (instance, first vertex) = (instance, first pixel in stream order): the components' order
    assert torch.equal(ring_inst[outer], comps.comp_inst)
    assert torch.equal(total, 2 * comps.comp_area.to(torch.int64))
    print('components per mask:', np.diff(comps.comp_offs.cpu().numpy()).tolist(), 'pieces', int(comps.piece_comp.shape[0]))


def test_serpentine_and_smooth_field_twice_with_identical_bits(dev):
    """one component that winds through every column of a 1024 x 1024 canvas, and a smooth field: unions from every block
    of the grid meet in a few roots, and a second launch gives the same bits"""
    from scipy import ndimage
    from rsprompter_amd import rle
    s = cases.serpentine(1024)
    f = ndimage.gaussian_filter(np.random.default_rng(7).random((1024, 1024)), 6.0)
    masks = np.stack([s, f > np.median(f)])
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(masks).to(dev))
    a = rle.runs_components(counts, n, (1024, 1024))
    b = rle.runs_components(counts, n, (1024, 1024))
    assert cases.same_components(a, b) and int(a.status.cpu()[0]) == 0
    offs = a.comp_offs.cpu().tolist()
    assert offs[1] == 1 and int(a.comp_area[0]) == int(s.sum()) and a.comp_box[0].cpu().tolist() == [0, 0, 1024, 1024]
    assert int((a.piece_comp[:int(a.piece_offs[1])] != 0).sum()) == 0
    from scipy.ndimage import label
    lab, cnt = label(masks[1], structure=np.ones((3, 3), int))
    assert offs[2] - offs[1] == cnt
    assert sorted(a.comp_area[1:].cpu().tolist()) == sorted(np.bincount(lab[masks[1]], minlength=cnt + 1)[1:].tolist())
    c1 = rle.clean_runs(counts, n, (1024, 1024), 100, 'both')
    c2 = rle.clean_runs(counts, n, (1024, 1024), 100, 'both')
    assert _rows_equal(c1[0], c1[1], c2[0], c2[1]) and torch.equal(c1[4], c2[4])


def test_300_tile_instances_shifted_into_a_scene(dev):
    """the run table rsp_rle_shift writes for an 8 192 x 9 000 scene: the components are the tile's components moved by the
    offset"""
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
    tile = rle.runs_components(counts, n, (th, tw))
    scene = rle.runs_components(sc, sn, (H, W))
    assert cases.same_components(scene, rle.runs_components(sc, sn, (H, W)))
    for name in ('comp_offs', 'piece_comp', 'comp_area', 'comp_inst', 'piece_offs'):
        assert torch.equal(getattr(scene, name), getattr(tile, name)), name
    ci, pi = tile.comp_inst.to(torch.int64), tile.pieces[3].to(torch.int64)
    o64 = off_d.to(torch.int64)
    assert torch.equal(scene.comp_box, tile.comp_box + torch.cat([off_d, off_d], 1)[ci])
    ty, tx = tile.comp_first.to(torch.int64) // tw, tile.comp_first.to(torch.int64) % tw
    assert torch.equal(scene.comp_first.to(torch.int64), (ty + o64[ci, 1]) * W + tx + o64[ci, 0])
    moved = tile.pieces + torch.stack([off_d[pi, 0], off_d[pi, 1], off_d[pi, 1], torch.zeros_like(off_d[pi, 0])])
    assert torch.equal(scene.pieces, moved)
    for i in (0, 5, 7, 8, 299):                                                    # and the tile results are the reference's
        got = [(int(a), tuple(b), int(f)) for a, b, f in zip(
            tile.comp_area[tile.comp_offs[i]:tile.comp_offs[i + 1]].cpu().tolist(),
            tile.comp_box[tile.comp_offs[i]:tile.comp_offs[i + 1]].cpu().tolist(),
            tile.comp_first[tile.comp_offs[i]:tile.comp_offs[i + 1]].cpu().tolist())]
        assert got == [(d['area'], d['box'], d['first']) for d in cref.check(tiles[i])[1]]
    print(f'{k} instances: {int(scene.comp_area.shape[0])} components, {int(scene.piece_comp.shape[0])} pieces, widest row '
          f'{int(sn.max())} runs')
    assert int(scene.comp_offs[9] - scene.comp_offs[8]) == 0 and int(scene.comp_offs[8] - scene.comp_offs[7]) == 1
