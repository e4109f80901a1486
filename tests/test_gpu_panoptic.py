"""-m gpu: panoptic fusion on the device -- every exact case of tests/_mask_field_props.py (all ==), the six tolerance cases,
the hand-checked semantics, the refusals, and the two query detectors with panoptic_on against the reference evaluated on
their own head outputs.  Bodies: tests/_panoptic_cases.py; reference: tests/_panoptic_ref.py."""
import os
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _mask_field_props as mf  # noqa: E402
import _panoptic_cases as pc  # noqa: E402
import _panoptic_ref as pr  # noqa: E402


@pytest.fixture(scope='module')
def ops():
    from rsprompter_amd import ops
    return ops


@pytest.mark.parametrize('case', mf.EXACT_CASES, ids=mf.case_id)
def test_exact(ops, dev, case):
    pc.check_exact(ops, dev, case)


@pytest.mark.parametrize('case', (mf.EXACT_CASES[0], mf.EXACT_CASES[2], mf.EXACT_CASES[8], mf.EXACT_CASES[16]), ids=mf.case_id)
def test_exact_ties(ops, dev, case):
    pc.check_exact_ties(ops, dev, case)


@pytest.mark.parametrize('check', (pc.check_two_stuff_queries_share_the_label, pc.check_rejected_thing_leaves_no_gap,
                                   pc.check_negative_everywhere, pc.check_zero_counts_as_inside, pc.check_none_kept,
                                   pc.check_filter_counts_the_area_before_it, pc.check_ratio_equal_to_the_threshold_is_kept,
                                   pc.check_more_kept_than_a_wave), ids=lambda f: f.__name__[6:])
def test_hand_checked(ops, dev, check):
    check(ops, dev)


def test_refusals(ops, dev):
    pc.check_refusals(ops, dev, 'cpu')


@pytest.mark.parametrize('case', mf.TOL_CASES, ids=mf.case_id)
def test_tolerance(ops, dev, case):
    pc.check_tolerance(ops, dev, case)


def test_bit_reproducible(ops, dev):
    """integer atomics only: two runs of the largest tolerance case give the same map and the same areas"""
    case = mf.TOL_CASES[1]
    cls, low = pc.tol_inputs(case, 0)
    a, ia = ops.panoptic_fuse(cls.to(dev), low.to(dev), *pc.geo_of(case), pc.NTHINGS, pc.NC, iou_thr=0.3)
    b, ib = ops.panoptic_fuse(cls.to(dev), low.to(dev), *pc.geo_of(case), pc.NTHINGS, pc.NC, iou_thr=0.3)
    assert torch.equal(a, b) and all(torch.equal(ia[k], ib[k]) for k in ia)


# ---------------------------------------------------------------------------------------------------------------- detectors
ORI, SCALE = 256, 4.0                       # 1024^2 input of a 256^2 image: crop 1024^2, output 256^2 (the generic form)


KEEP = {'RSPrompterQuery': 5, 'SAMSegMask2Former': 3}      # kept queries: object_mask_thr sits between the KEEP-th and the next score


def distinct_queries(sd, mask_scale):
    """Test inputs, chosen on the CPU oracles' outputs alone.  With plainly seeded weights the queries of these networks are
    near-duplicates of each other (scores within 0.02, mask logits of magnitude 2 that differ little), so their products tie
    on 1 - 7 % of the pixels and no choice of seed or threshold meets the tolerance tier's cap.  The query embeddings x 50
    make the queries different, the class logits x 4 spread the scores, and the last layer of the mask branch x mask_scale
    brings the logits to the magnitude of the recipe's (17 to 30)."""
    for k in sd:
        if k in ('panoptic_head.query_feat.weight', 'panoptic_head.query_embed.weight'):
            sd[k] = sd[k] * 50.0
        elif k.startswith('panoptic_head.cls_embed.2.') or k in ('panoptic_head.cls_embed.weight', 'panoptic_head.cls_embed.bias'):
            sd[k] = sd[k] * 4.0
        elif k.startswith('panoptic_head.mask_embed.4.') or ('output_hypernetworks_mlps' in k and 'proj_out' in k):
            sd[k] = sd[k] * mask_scale
    return sd


def _check_detector(model, dev, nthings, nc):
    """one forward through the detector with panoptic_on and instance_on; then the fusion head alone on the kept head
    outputs (the network's float atomics make a second forward differ in the last bits; the fusion is bit-reproducible)"""
    from rsprompter_amd.structures import DetDataSample
    from rsprompter_amd.synth import synth_images, synth_metas
    meta = synth_metas(1, ori_shape=(ORI, ORI), scale_factor=(SCALE, SCALE))[0]
    fh = model.panoptic_fusion_head
    fh.test_cfg = dict(panoptic_on=True, instance_on=True, semantic_on=False, max_per_image=10, object_mask_thr=0.3, iou_thr=0.3)

    def sample():
        return [DetDataSample(metainfo=dict(meta))]

    first = model.test_step(dict(inputs=[im.to(dev) for im in synth_images(1)], data_samples=sample()))[0]
    cls, masks = model._last_head_out
    again = fh.predict(cls, masks, sample(), rescale=True)[0]
    assert torch.equal(first.pred_panoptic_seg.sem_seg, again['pan_results'].sem_seg)         # what the detector returns is the head's
    assert tuple(first.pred_panoptic_seg.sem_seg.shape) == (1, ORI, ORI) and torch.equal(first.pred_instances.masks, again['ins_results'].masks)
    cls0, low0 = cls[0].float().cpu(), masks.low_res[0].float().cpu()
    geo = (tuple(masks.size), (1024, 1024), (ORI, ORI))
    # thresholds from the reference alone: object_mask_thr keeps the KEEP highest non-background scores, iou_thr sits in the
    # widest gap of the kept queries' ratios
    score, label, _ = pr.select(cls0, nc, 0.0)
    top = sorted((float(s) for s, c in zip(score, label) if c != nc), reverse=True)
    keep = KEEP[type(model).__name__]
    assert len(top) > keep and top[keep - 1] - top[keep] >= 2e-5, 'the scores around the threshold are closer than fp32 resolves'
    thr = (top[keep - 1] + top[keep]) / 2
    r = pr.reference(cls0, low0, geo, nthings, nc, object_mask_thr=thr)
    iou = pc.ratio_threshold(r)
    r = pr.reference(cls0, low0, geo, nthings, nc, object_mask_thr=thr, iou_thr=iou)
    fh.test_cfg.update(object_mask_thr=thr, iou_thr=iou)
    s = fh.predict(cls, masks, sample(), rescale=True)[0]
    pan, ins = s['pan_results'], s['ins_results']
    sem = pan.sem_seg.cpu()
    assert sem.dtype == torch.int32 and tuple(sem.shape) == (1, ORI, ORI)
    near = r['gap'] <= r['pair_scores'] * mf.VALUE_TOL / 4 + 1e-6
    n = int(near.sum())
    case = mf.Case(tuple(low0.shape[-2:]), geo[0], geo[1], geo[2], 'generic')
    cap = pc.near_pixel_cap(case)                        # the tolerance tier's caps: 99 near pixels, 6 within 1e-4 of 0 at 256^2
    print(f'{type(model).__name__}: {len(r["kept"])} of {cls0.shape[0]} queries kept at {thr:.3f}, iou_thr {iou:.3f}, {n} near pixels (cap {cap}), '
          f'at most {max(r["near_zero"])} pixels within 1e-4 of 0 (cap {mf.near_cap(case)}), {int((sem[0] != r["sem"]).sum())} map pixels off the '
          f'fp64 ones, segments {sorted(set(r["segment"]))}, |logit| up to {float(low0.abs().max()):.1f}')
    assert len(r['kept']) == keep and n <= cap and max(r['near_zero']) <= mf.near_cap(case)
    for k, q in enumerate(r['kept']):
        m, o, z = r['mask_area'][q], r['original_area'][q], r['near_zero'][k]
        assert (m - n > 0 and o - z > 0 and (m - n) / (o + z) >= iou) or (o - z > 0 and (m + n) / (o - z) < iou) or (o == 0 and z == 0), \
            ('the reference decides within its slack', q, m, o, n, z, iou)
    assert pan.query_segment.cpu().tolist() == r['segment']
    assert not bool(((sem[0] != r['sem']) & ~near).any())
    assert all(abs(a - b) <= n for a, b in zip(pan.mask_area.cpu().tolist(), r['mask_area']))
    assert all(abs(pan.original_area.cpu().tolist()[q] - r['original_area'][q]) <= r['near_zero'][k] for k, q in enumerate(r['kept']))
    # the instance results next to it are those of panoptic_on=False on the same head outputs
    fh.test_cfg.update(panoptic_on=False)
    only = fh.predict(cls, masks, [DetDataSample(metainfo=dict(meta))], rescale=True)[0]
    assert set(only) == {'ins_results'}
    pi, oi = ins, only['ins_results']
    for k in ('labels', 'masks', 'bboxes', 'query_indices'):
        assert torch.equal(getattr(pi, k), getattr(oi, k)), k
    assert float((pi.scores - oi.scores).abs().max()) <= 1e-6          # fp64 atomics of the mask average: order-dependent last bits


def test_rsprompter_query_panoptic(dev):
    import rsprompter_amd as ra
    from rsprompter_amd.default_configs import rsprompter_query
    from rsprompter_amd.synth import synth_state_dict
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = ra.build_model(rsprompter_query('base', 1, (30, 5)))
    model.load_state_dict(distinct_queries(synth_state_dict(model, seed=2), 5.0), strict=True)
    _check_detector(model.to(dev), dev, 1, 1)


def test_samseg_mask2former_panoptic(dev):
    import rsprompter_amd as ra
    from rsprompter_amd.default_configs import samseg_mask2former
    from rsprompter_amd.synth import synth_state_dict
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = ra.build_model(samseg_mask2former('base', 3, 30))
    model.load_state_dict(distinct_queries(synth_state_dict(model, seed=3), 1.0), strict=True)
    _check_detector(model.to(dev), dev, model.num_things_classes, model.num_classes)


def test_default_test_cfg_returns_a_panoptic_map(ops, dev):
    """a fusion head built without panoptic_on (the reference's default is True) returns pan_results instead of raising"""
    from rsprompter_amd.query_heads import LazyUpsampledMasks, RSMaskFormerFusionHead
    from rsprompter_amd.structures import DetDataSample, PixelData
    cls, low = pc.exact_inputs(mf.EXACT_CASES[0], 0)
    head = RSMaskFormerFusionHead(num_things_classes=pc.NTHINGS, num_stuff_classes=1, test_cfg=None)
    meta = dict(ori_shape=(64, 48), img_shape=(64, 48), scale_factor=(1.0, 1.0), batch_input_shape=(64, 48))
    res = head.predict(cls[None].to(dev), LazyUpsampledMasks(low[None].to(dev), (64, 48)), [DetDataSample(metainfo=meta)], rescale=True)[0]
    r = pr.reference(cls, low, pc.geo_of(mf.EXACT_CASES[0]), pc.NTHINGS, pc.NC)
    assert set(res) == {'pan_results'} and isinstance(res['pan_results'], PixelData)
    assert torch.equal(res['pan_results'].sem_seg[0].cpu(), r['sem'])
