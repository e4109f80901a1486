"""CPU (`-m "not gpu"`): polygon export (csrc/mask_polygons.hip, rle.runs_to_polygons, apis.masks_to_polygons,
large_image masks='polygons').

The oracle is tests/_mask_polygons_ref.py, the sequential ring definition on dense numpy masks, itself checked against
scipy.ndimage; the kernels run lane by lane on the emulator (tests/wave_emu), the sources unchanged, and must agree
exactly.  The bodies are tests/_mask_polygons_cases.py, the same the device tier runs."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _large_image_ref as lref  # noqa: E402
import _mask_polygons_cases as cases  # noqa: E402
import _mask_polygons_ref as pref  # noqa: E402
import _seam_merge_cases as seam_cases  # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# --------------------------------------------------------------------------------------------------- the reference itself
def test_reference_holds_its_properties_on_every_case_mask():
    """area identity, ring counts against scipy.ndimage.label (8-connected foreground, 4-connected padded background),
    parents against the component labels, even-odd refill equal to the mask, corners only"""
    seen_holes = seen_saddle = 0
    for name, m in cases.all_cases():
        rings = cases.want_of(name, m)
        seen_holes += sum(a2 < 0 for _, _, a2 in rings)
        seen_saddle += any(len({tuple(v) for v in ring.tolist()}) < len(ring) for ring, _, _ in rings)
    assert seen_holes > 100 and seen_saddle >= 5
    H, W, masks, want = cases.batch_case()
    for m, w in zip(masks, want):                              # moving a mask moves its rings
        got = pref.trace(m)
        assert len(got) == len(w) and all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(got, w))
    nested = dict(cases.all_cases())['nested frames']
    assert [p for _, p, _ in pref.trace(nested)] == [-1, 0, -1, 2, -1, 4, -1]          # parents at depth
    assert len(pref.trace(cases.arm_spiral(33))) == 1 and len(pref.trace(cases.arm_spiral(33))[0][0]) == 68


def test_reference_coco_round_trip_of_hole_free_masks():
    """the outer rings through the project's restated rleFrPoly + rleMerge give the mask back (COCO `segmentation`)"""
    from rsprompter_amd import datasets
    rng = np.random.default_rng(12)
    done = 0
    for _ in range(200):
        H, W = int(rng.integers(3, 20)), int(rng.integers(3, 20))
        m = rng.random((H, W)) < 0.4
        rings = pref.trace(m)
        if not rings or any(a2 < 0 for _, _, a2 in rings):
            continue
        polys = [[float(v) for v in ring.reshape(-1).tolist()] for ring, _, _ in rings]
        assert datasets.rle_merge([datasets.rle_from_poly(p, H, W) for p in polys]) == lref.rle_counts_np(m)
        done += 1
    assert done >= 20


# ------------------------------------------------------------------------------------------------------------ kernels
def test_known_answers(emu):
    cases.check_known_answers(emu, CPU)


def test_every_case_mask_alone(emu):
    cases.check_single_masks(emu, CPU)


def test_batch_with_invalid_rows_and_a_second_launch(emu):
    got, want = cases.check_batch(emu, CPU)
    assert int(got[1].shape[0]) - 1 > 350 and sum(1 for w in want if not w) >= 10


def test_no_rows_and_no_rings(emu):
    cases.check_no_rows_and_no_rings(emu, CPU)


def test_bad_arguments_are_refused(emu):
    cases.check_refuses_bad_arguments(emu, CPU, pytest)


def test_the_piece_table_its_two_consumers_and_their_host_reads(emu):
    cases.check_run_pieces(emu, CPU)


def test_rings_of_shifted_and_joined_run_tables(emu):
    """the tables rsp_rle_shift and rsp_rle_union write are input as well: tile rings + offset, rings of a union"""
    from rsprompter_amd import rle
    rng = np.random.default_rng(2)
    tiles = [rng.random((9, 8)) < d for d in (0.3, 0.6, 1.0, 0.0)]
    counts, n = seam_cases.rows_from_masks(tiles, CPU)
    offs = torch.tensor([[3, 2], [0, 0], [12, 11], [5, 5]], dtype=torch.int32)
    H, W = 20, 20
    sc, sn, _, _ = rle.shift_runs(counts, n, offs, (9, 8), (H, W))
    got = rle.polygons_to_lists(*rle.runs_to_polygons(sc, sn, (H, W)))
    tile = rle.polygons_to_lists(*rle.runs_to_polygons(counts, n, (9, 8)))
    for g, t, o, m in zip(got, tile, offs.tolist(), tiles):
        assert len(g) == len(t) == len(pref.trace(m))
        assert all(np.array_equal(a[0], b[0] + np.array(o, np.int32)) and a[1:] == b[1:] for a, b in zip(g, t))
    uc, un, _, _ = rle.union_runs(sc, sn, (H, W), torch.tensor([0, 2, 4], dtype=torch.int32), torch.arange(4, dtype=torch.int32))
    placed = [cases.embed(m, H, W, o[0], o[1]) for m, o in zip(tiles, offs.tolist())]
    cases.assert_arrays_equal(emu.mask_polygons(uc, un, H, W),
                              pref.flatten([pref.trace(placed[0] | placed[1]), pref.trace(placed[2] | placed[3])]), 'union')


# ---------------------------------------------------------------------------------------------------------------- API
def test_masks_to_polygons_forms(emu):
    from rsprompter_amd import apis, rle
    cases.check_api_forms(apis, rle, CPU)


def test_masks_to_polygons_refusals(emu):
    from rsprompter_amd import apis
    cases.check_api_refusals(apis, CPU, pytest)


def test_geojson_of_a_result_without_masks_says_so(emu):
    from rsprompter_amd import large_image as li
    from rsprompter_amd.structures import DetDataSample, InstanceData
    d = DetDataSample(metainfo=dict(ori_shape=(8, 8)))
    d.pred_instances = InstanceData(bboxes=torch.zeros((1, 4)), scores=torch.ones(1), labels=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match='returned no masks'):
        li.pred2geojson(d)
    d.pred_instances = InstanceData(bboxes=torch.zeros((0, 4)), scores=torch.ones(0), labels=torch.zeros(0, dtype=torch.int64))
    assert li.pred2geojson(d) == dict(type='FeatureCollection', features=[])
    d.pred_instances = InstanceData(bboxes=torch.zeros((1, 4)), scores=torch.ones(1), labels=torch.zeros(1, dtype=torch.int64),
                                    masks=[dict(size=[8, 8], counts=b'P2')])
    with pytest.raises(ValueError, match="masks='polygons'"):
        li.pred2geojson(d)


def test_pred2dict_of_dense_and_empty_results_is_as_before(emu):
    """pred_instances.masks as a bool [K, H, W] tensor (masks='dense') goes through encode_mask_results, K = 0 included"""
    from rsprompter_amd import large_image as li
    from rsprompter_amd import rle
    from rsprompter_amd.structures import DetDataSample, InstanceData
    m = torch.from_numpy(np.random.default_rng(1).random((2, 8, 8)) < 0.5)
    d = DetDataSample(metainfo=dict(ori_shape=(8, 8)))
    d.pred_instances = InstanceData(bboxes=torch.zeros((2, 4)), scores=torch.tensor([0.9, 0.2]),
                                    labels=torch.zeros(2, dtype=torch.int64), masks=m)
    want = [dict(size=[8, 8], counts=rle.counts_to_string(lref.rle_counts_np(x)).decode()) for x in m.numpy()]
    assert li.pred2dict(d)['masks'] == want and li.pred2dict(d, 0.5)['masks'] == want[:1]
    d.pred_instances = InstanceData(bboxes=torch.zeros((0, 4)), scores=torch.ones(0), labels=torch.zeros(0, dtype=torch.int64),
                                    masks=torch.zeros((0, 8, 8), dtype=torch.bool))
    assert li.pred2dict(d)['masks'] == []
    d.pred_instances = InstanceData(bboxes=torch.zeros((0, 4)), scores=torch.ones(0), labels=torch.zeros(0, dtype=torch.int64), masks=[])
    assert li.pred2dict(d)['masks'] == []


# ----------------------------------------------------------------------------------------------------------- pipeline
def _scene():
    rng = np.random.default_rng(16)
    return rng.integers(0, 256, (45, 70, 3)).astype(np.uint8)


@pytest.mark.parametrize('mode', ['nms', 'seam_mask'])
def test_inference_large_image_polygons_around_a_random_stub_detector(emu, mode):
    """masks='polygons' against the reference applied to the dense result of the same call (the dense paste / the dense
    union of the seam merge), both merge modes"""
    from rsprompter_amd import large_image as li
    kw = dict(merge_iou_thr=0.25, merge_nms_type=mode)
    if mode == 'seam_mask':
        kw['seam_iou_thr'] = 0.3
    k, rings = cases.check_pipeline(li, CPU, _scene(), seam_cases.RandomStub((32, 32)), 32,
                                    lambda s: s.pred_instances.masks.numpy(), **kw)
    assert k >= 10 and rings > k


def test_cli_default_output_is_unchanged_and_the_new_formats(emu, tmp_path, monkeypatch):
    """`python -m rsprompter_amd.large_image` (its main(), in process, around the stub detector): without --mask-format the
    file is what pred2dict of the default call gives, RLE strings; polygons and geojson write their forms"""
    from PIL import Image
    from rsprompter_amd import apis
    from rsprompter_amd import large_image as li
    model = seam_cases.RandomStub((32, 32))
    monkeypatch.setattr(apis, 'init_detector', lambda cfg, ckpt, device=None: model)
    Image.fromarray(_scene()).save(tmp_path / 'scene.png')
    src = str(tmp_path / 'scene.png')
    argv = [src, 'cfg.py', 'none', '--patch-size', '32', '--batch-size', '2', '--score-thr', '0.4']
    want = li.pred2dict(li.inference_large_image(model, src, 32, batch_size=2), 0.4)
    li.main(argv + ['--out-dir', str(tmp_path / 'a')])
    assert os.listdir(tmp_path / 'a') == ['scene.json']
    text = (tmp_path / 'a' / 'scene.json').read_text()
    assert text == json.dumps(want) and len(want['masks']) > 3 and all(isinstance(m['counts'], str) for m in want['masks'])
    li.main(argv + ['--out-dir', str(tmp_path / 'b'), '--mask-format', 'rle'])
    assert (tmp_path / 'b' / 'scene.json').read_text() == text
    li.main(argv + ['--out-dir', str(tmp_path / 'c'), '--mask-format', 'polygons'])
    got = json.loads((tmp_path / 'c' / 'scene.json').read_text())
    assert {k: got[k] for k in ('labels', 'scores', 'bboxes')} == {k: want[k] for k in ('labels', 'scores', 'bboxes')}
    for inst, r in zip(got['masks'], want['masks']):
        m = lref.counts_to_mask(__import__('rsprompter_amd.datasets', fromlist=['x']).rle_from_string(r['counts']), 45, 70)
        w = pref.trace(m)
        assert [(x['ring'], x['parent'], x['area2']) for x in inst] == [(a.tolist(), b, c) for a, b, c in w]
    li.main(argv + ['--out-dir', str(tmp_path / 'd'), '--mask-format', 'geojson', '--geo-transform', '100', '0.5', '0', '200', '0', '-0.5'])
    assert os.listdir(tmp_path / 'd') == ['scene.geojson']
    fc = json.loads((tmp_path / 'd' / 'scene.geojson').read_text())
    assert fc['type'] == 'FeatureCollection' and len(fc['features']) == len(want['labels'])
    assert [f['properties']['label'] for f in fc['features']] == want['labels']
    assert [f['properties']['bbox'] for f in fc['features']] == want['bboxes']
    first = next(f for f in fc['features'] if f['geometry']['coordinates'])
    ring = first['geometry']['coordinates'][0] if first['geometry']['type'] == 'Polygon' else first['geometry']['coordinates'][0][0]
    assert ring[0] == ring[-1] and all(100 <= x <= 135 and 177.5 <= y <= 200 for x, y in ring)
    with pytest.raises(SystemExit):
        li.main(argv + ['--geo-transform', '1', '2', '3', '4', '5', '6'])
