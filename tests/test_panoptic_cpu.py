"""-m "not gpu": panoptic fusion (csrc/panoptic_fuse.hip, ops.panoptic_fuse, the fusion heads' panoptic_on branch,
apis.panoptic_to_coco) on the lane-level emulator (tests/wave_emu) against tests/_panoptic_ref.py -- the exact cases of at
most 16k output pixels, the two smallest tolerance cases, the hand-checked semantics, the refusals, and the host layers.  The
bodies (tests/_panoptic_cases.py) are the ones tests/test_gpu_panoptic.py runs on the device."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _mask_field_props as mf  # noqa: E402
import _panoptic_cases as pc  # noqa: E402
import _panoptic_ref as pr  # noqa: E402

CPU = torch.device('cpu')
EMU_EXACT = tuple(c for c in mf.EXACT_CASES if mf.pixels(c) <= 16384)
EMU_TOL = tuple(sorted(mf.TOL_CASES, key=mf.pixels)[:2])


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


def test_the_cases_visit_every_form_and_path():
    """A precondition on the case lists alone (it runs no product code): strip, identity with ow % 4 in {1, 2, 3}, generic
    with quads and per pixel, a 1 x 1 crop, 1 x 1 logits -- in the emulator's subset too -- and the two-block strip on the device"""
    for cases in (mf.EXACT_CASES, EMU_EXACT):
        forms = {(c.form, c.out[1] % 4) for c in cases}
        assert {('strip', 0), ('ident', 1), ('ident', 2), ('ident', 3), ('generic', 0)} <= forms
        assert any(f == 'generic' and m for f, m in forms)
        assert any(c.out == (1, 1) for c in cases) and any(c.hw == (1, 1) for c in cases)
    big = mf.Case((64, 64), (256, 256), (200, 136), (200, 136), 'strip')
    assert big in mf.EXACT_CASES and big not in EMU_EXACT
    assert -(-big.out[0] // 2) * (big.out[1] // 4) > 256           # more than one block of row-pair x quad groups
    assert set(pc.EXACT_SEEDS) <= {mf.case_id(c) for c in mf.EXACT_CASES}
    assert set(pc.TOL_SEEDS) == {mf.case_id(c) for c in mf.TOL_CASES}


def test_the_two_forms_of_the_reference_agree_on_every_exact_input():
    """A precondition on the reference alone (it runs no product code): tests/_panoptic_ref.py's loop and array form, ==, on
    every exact case's inputs and both configurations (the emulator tests below go through reference() as well; this covers
    the cases only the device runs)"""
    outcomes = set()
    for case in mf.EXACT_CASES:
        cls, low = pc.exact_inputs(case, pc.exact_seed(case))
        for cfg in pc.EXACT_CFGS:
            r = pr.reference(cls, low, pc.geo_of(case), pc.NTHINGS, pc.NC, **cfg)
            assert int(pc.near_exact(r).sum()) == 0, case
            outcomes |= {s >= 0 for q, s in enumerate(r['segment']) if q in r['kept']}
    assert outcomes == {True, False}                                # queries are painted and rejected


@pytest.mark.parametrize('case', EMU_EXACT, ids=mf.case_id)
def test_exact_on_the_emulator(emu, case):
    pc.check_exact(emu, CPU, case)


@pytest.mark.parametrize('case', (mf.EXACT_CASES[0], mf.EXACT_CASES[2], mf.EXACT_CASES[8]), ids=mf.case_id)
def test_exact_ties_on_the_emulator(emu, case):
    pc.check_exact_ties(emu, CPU, case)


@pytest.mark.parametrize('check', (pc.check_two_stuff_queries_share_the_label, pc.check_rejected_thing_leaves_no_gap,
                                   pc.check_negative_everywhere, pc.check_zero_counts_as_inside, pc.check_none_kept,
                                   pc.check_filter_counts_the_area_before_it, pc.check_ratio_equal_to_the_threshold_is_kept,
                                   pc.check_more_kept_than_a_wave), ids=lambda f: f.__name__[6:])
def test_hand_checked_on_the_emulator(emu, check):
    check(emu, CPU)


def test_refusals_on_the_emulator(emu):
    pc.check_refusals(emu, CPU, 'meta')                             # the meta device stands in for "another device"


@pytest.mark.parametrize('case', EMU_TOL, ids=mf.case_id)
def test_tolerance_on_the_emulator(emu, case):
    pc.check_tolerance(emu, CPU, case)


# --------------------------------------------------------------------------------------------------------------- host layers
def _head(**test_cfg):
    from rsprompter_amd.query_heads import RSMaskFormerFusionHead
    return RSMaskFormerFusionHead(num_things_classes=pc.NTHINGS, num_stuff_classes=pc.NC - pc.NTHINGS, test_cfg=test_cfg)


def _samples(ori, scale):
    from rsprompter_amd.structures import DetDataSample
    return [DetDataSample(metainfo=dict(ori_shape=(ori, ori), img_shape=(int(ori * scale), int(ori * scale)),
                                        scale_factor=(scale, scale), batch_input_shape=(64, 64)))]


@pytest.mark.parametrize('ori,scale,rescale', ((32, 2.0, True), (32, 2.0, False), (64, 1.0, True)), ids=('whu', 'whu-crop', 'identity'))
def test_fusion_head_panoptic_branch(emu, ori, scale, rescale):
    """RSMaskFormerFusionHead.predict with panoptic_on (the reference's default): sem_seg is the reference on the same
    cls / low-resolution logits and geometry; instance results next to it are those of panoptic_on=False; semantic_on and
    a dense tensor raise as before"""
    from rsprompter_amd.query_heads import LazyUpsampledMasks, MaskFormerFusionHead
    from rsprompter_amd.structures import PixelData
    cls, low = pc.exact_inputs(mf.Case((16, 16), (64, 64), (64, 64), (64, 64), 'strip'), 5)
    masks = LazyUpsampledMasks(low[None], (64, 64))
    crop = (int(ori * scale),) * 2
    out = (ori, ori) if rescale else crop
    cfg = dict(object_mask_thr=0.8, iou_thr=0.3, filter_low_score=True)
    r = pr.reference(cls, low, ((64, 64), crop, out), pc.NTHINGS, pc.NC, **cfg)
    assert int(pc.near_exact(r).sum()) == 0 and any(s >= 0 for s in r['segment'])
    res = _head(panoptic_on=True, instance_on=True, max_per_image=10, **cfg).predict(cls[None], masks, _samples(ori, scale), rescale=rescale)[0]
    pan = res['pan_results']
    assert isinstance(pan, PixelData) and pan.sem_seg.dtype == torch.int32 and tuple(pan.sem_seg.shape) == (1,) + out
    assert torch.equal(pan.sem_seg[0], r['sem'])
    assert pan.query_segment.tolist() == r['segment'] and pan.mask_area.tolist() == r['mask_area']
    assert pan.original_area.tolist() == r['original_area'] and pan.shape == out
    only = _head(panoptic_on=False, instance_on=True, max_per_image=10).predict(cls[None], masks, _samples(ori, scale), rescale=rescale)[0]
    assert set(only) == {'ins_results'} and set(res) == {'pan_results', 'ins_results'}
    for k in ('bboxes', 'labels', 'scores', 'masks', 'query_indices'):
        assert torch.equal(getattr(res['ins_results'], k), getattr(only['ins_results'], k)), k
    # the defaults: panoptic_on, no instances (models.py:672-674); the registered subclass shares the body
    dflt = MaskFormerFusionHead(num_things_classes=pc.NTHINGS, num_stuff_classes=1, test_cfg=cfg).predict(
        cls[None], masks, _samples(ori, scale), rescale=rescale)[0]
    assert set(dflt) == {'pan_results'} and torch.equal(dflt['pan_results'].sem_seg, pan.sem_seg)
    with pytest.raises(NotImplementedError):
        _head(semantic_on=True).predict(cls[None], masks, _samples(ori, scale))
    with pytest.raises(TypeError):
        _head().predict(cls[None], torch.zeros(1, 12, 64, 64), _samples(ori, scale))


def test_panoptic_to_coco():
    """rgb2id of the image is the map with void as 0; segments_info without void, areas summing to the non-void pixels, a
    stuff class once; ids beyond 65535 use the third channel"""
    from rsprompter_amd import apis
    from rsprompter_amd.structures import PixelData
    sem = torch.full((6, 8), 3, dtype=torch.int32)
    sem[0, :4], sem[1, :3], sem[2, :2], sem[5, 6:] = 1000, 2001, 2, 2
    sem[3, :5] = 70001
    rgb, info = apis.panoptic_to_coco(PixelData(sem_seg=sem[None], void=3), 2)
    assert rgb.dtype.name == 'uint8' and rgb.shape == (6, 8, 3)
    ids = rgb[..., 0].astype('int64') + 256 * rgb[..., 1].astype('int64') + 65536 * rgb[..., 2].astype('int64')      # rgb2id
    want = sem.clone()
    want[sem == 3] = 0
    assert (torch.from_numpy(ids) == want).all()
    assert [s['id'] for s in info] == [2, 1000, 2001, 70001] and [s['area'] for s in info] == [4, 4, 3, 5]
    assert [s['category_id'] for s in info] == [2, 0, 1, 1] and [s['isthing'] for s in info] == [False, True, True, True]
    assert sum(s['area'] for s in info) == int((sem != 3).sum())
    rgb2, info2 = apis.panoptic_to_coco(sem, 2, void=3)                       # a plain tensor with the void id given
    assert (rgb2 == rgb).all() and info2 == info
    with pytest.raises(ValueError):
        apis.panoptic_to_coco(sem.float(), 2, void=3)
    for no_void in (sem, sem[None], PixelData(sem_seg=sem[None])):           # the void id would come out as a segment
        with pytest.raises(ValueError, match='void'):
            apis.panoptic_to_coco(no_void, 2)


class _StubHead:
    """stands in for the panoptic head: predict returns fixed head outputs"""

    def __init__(self, out):
        self.out = out

    def predict(self, x, batch_data_samples, **kwargs):
        return self.out


@pytest.mark.parametrize('name', ('RSPrompterQuery', 'SAMSegMask2Former'))
def test_detector_predict_sets_pred_panoptic_seg(emu, name):
    """the detectors' own predict (maskformer.py:141-146) on a stub backbone and head with the real fusion head: with the
    reference's default test_cfg the sample gets pred_panoptic_seg (the reference's map) and no pred_instances; with
    instance_on both"""
    from rsprompter_amd import query_heads
    from rsprompter_amd.query_heads import LazyUpsampledMasks, RSMaskFormerFusionHead
    from rsprompter_amd.structures import PixelData
    cls, low = pc.exact_inputs(mf.Case((16, 16), (64, 64), (64, 64), (64, 64), 'strip'), 5)
    r = pr.reference(cls, low, ((64, 64), (64, 64), (32, 32)), pc.NTHINGS, pc.NC)
    assert int(pc.near_exact(r).sum()) == 0
    det_cls = getattr(query_heads, name)
    for cfg, fields in ((None, {'pred_panoptic_seg'}), (dict(instance_on=True, max_per_image=10), {'pred_panoptic_seg', 'pred_instances'})):
        det = det_cls.__new__(det_cls)
        torch.nn.Module.__init__(det)
        det.panoptic_head = _StubHead((cls[None], LazyUpsampledMasks(low[None], (64, 64))))
        det.panoptic_fusion_head = RSMaskFormerFusionHead(num_things_classes=pc.NTHINGS, num_stuff_classes=1, test_cfg=cfg)
        det.extract_feat = (lambda inputs: (None, None, None)) if name == 'RSPrompterQuery' else (lambda inputs: None)
        s = det.predict(None, _samples(32, 2.0), rescale=True)[0]
        assert {k for k in ('pred_panoptic_seg', 'pred_instances') if s.get(k) is not None} == fields
        assert isinstance(s.pred_panoptic_seg, PixelData) and torch.equal(s.pred_panoptic_seg.sem_seg[0], r['sem'])
        assert s.pred_panoptic_seg.query_segment.tolist() == r['segment']


def test_pixel_data_and_the_inferencer_hand_the_field_on(emu):
    """DetInferencer.pred2dict hands the PixelData on (and works without pred_instances); PixelData behaves like InstanceData"""
    from rsprompter_amd import apis
    from rsprompter_amd.structures import DetDataSample, PixelData
    p = PixelData(sem_seg=torch.zeros(1, 2, 3, dtype=torch.int32))
    p.extra = 7
    assert 'sem_seg' in p and p.extra == 7 and p.get('nothing') is None and p.shape == (2, 3) and set(p.keys()) == {'sem_seg', 'extra'}
    assert p.to(torch.device('cpu')).sem_seg.dtype == torch.int32 and 'sem_seg=(1, 2, 3)' in repr(p)
    with pytest.raises(AttributeError):
        p.missing
    s = DetDataSample()
    s.pred_panoptic_seg = p
    out = apis.DetInferencer.pred2dict(None, s)
    assert out == dict(panoptic_seg=p)
    from rsprompter_amd.structures import InstanceData
    m = torch.zeros(1, 4, 8, dtype=torch.bool)
    m[0, 1:3, 2:5] = True
    s.pred_instances = InstanceData(labels=torch.tensor([1]), scores=torch.tensor([0.5]), bboxes=torch.tensor([[2.0, 1.0, 5.0, 3.0]]), masks=m)
    out = apis.DetInferencer.pred2dict(None, s)                                 # both fields: the instance entries are what they were
    assert out['panoptic_seg'] is p and out['labels'] == [1] and out['scores'] == [0.5] and len(out['masks']) == 1
    assert out['masks'][0]['size'] == [4, 8]
