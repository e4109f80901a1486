"""CPU (`-m "not gpu"`): oriented-box comparison (csrc/obb_iou.hip; ops.obb_corners / obb_iou / obb_nms, rle.runs_to_obb_corners,
apis.obb_iou / nms_rotated, large_image merge_nms_type='nms_rotated', CocoMetric metric='obb').

The oracle is tests/_obb_iou_ref.py: the IoU of two convex quadrilaterals in fractions, exact for any float64 input.  The
kernels run lane by lane on the emulator (tests/wave_emu), the sources unchanged.  Values with small integer corners must
be == the exact value; everything else lies within cases.BOUND of it, a bound measured against the exact reference (never
against the kernel); decisions -- keep lists, dtm -- are equal to the reference's on the exact IoUs.  The bodies are
tests/_obb_iou_cases.py, the same the device tier runs."""
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _obb_iou_cases as cases  # noqa: E402
import _obb_iou_ref as ref  # noqa: E402

CPU = torch.device('cpu')
EMU_NMS_SIZES = cases.NMS_SIZES


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# ---------------------------------------------------------------------------------- the reference and the preconditions
def test_reference_known_answers():
    for name, a, b, crowd, want in cases.exact_table():
        assert ref.exact_iou(a, b, bool(crowd)) == want, name
        assert ref.exact_iou(a[::-1], b, bool(crowd)) == want and ref.exact_iou(a, b[::-1], bool(crowd)) == want, name
        if not crowd:
            assert ref.exact_iou(b, a) == want, name
        assert ref.twin_iou(a, b, bool(crowd)) == float(want), name              # every operation is exact on these
    # the matrix form (bounds prefilter, symmetry) is the pair form
    q = cases.nms_boxes(40, 3)[0]
    m = ref.exact_iou_matrix(q, q)
    assert all(m[i][j] == ref.exact_iou(q[i], q[j]) for i in range(40) for j in range(40))
    # greedy NMS on a chain
    chain = np.stack([cases.sq(0, 0, 10, 4), cases.sq(4, 0, 14, 4), cases.sq(8, 0, 18, 4)])
    assert ref.nms(chain, [0.9, 0.8, 0.7], [0, 0, 0], 0.3) == [0, 2]
    assert ref.nms(chain, [0.9, 0.8, 0.7], [0, 0, 0], Fraction(3, 7)) == [0, 1, 2]           # strict: 6 / 14 is not above 3 / 7


def test_the_twin_stays_within_a_sixteenth_of_the_bound():
    """the tolerance is sized by the float64 twin's distance from the EXACT value over the committed generator; no product
    code runs here"""
    errs = cases.twin_errors()
    print({k: f'{float(v):.3e}' for k, v in errs.items()}, 'BOUND', cases.BOUND)
    assert max(errs.values()) <= Fraction(cases.BOUND) / 16
    assert max(errs.values()) >= Fraction(cases.BOUND) / 64                      # ... and the bound is not padded
    assert sorted(errs) == ['lattice', 'near-identical', 'ordinary', 'slivers']
    for name, a, b, exact in cases.families():
        assert sum(1 for e in exact if e > 0) >= len(exact) // 2, name           # the families do overlap


def test_no_exact_iou_of_a_decision_case_is_near_a_threshold():
    """keep lists are compared for equality: no product code runs here"""
    worst = Fraction(1)
    for n in cases.NMS_SIZES:
        worst = min(worst, cases.decision_margin(cases.nms_case(n)[3], cases.NMS_THRS))
    print('smallest distance of an exact IoU to a threshold:', float(worst))
    assert worst > Fraction(cases.DECISION_MARGIN)
    assert cases.BOUND < cases.DECISION_MARGIN / 100


def test_the_grid_construction_is_the_reference_nms():
    """the keep lists that the sizes beyond the exact reference's reach are compared with (cases.nms_grid_case) are the
    reference's on exact IoUs where it can be run: n = 260, m = 160, both input orders; no product code runs here"""
    for q, s, lab, aware, agnostic in (cases.nms_grid_case(260, 160), cases.nms_grid_permuted(260, 160)):
        iou = ref.exact_iou_matrix(q, q)
        assert all(e is ref.ZERO or e == 1 for row in iou for e in row)           # nothing is near a threshold
        assert sum(1 for row in iou for e in row if e == 1) == 260 + 2 * cases.NMS_GRID_TAIL
        for thr in cases.NMS_THRS:
            assert ref.nms(q, s, lab, thr, False, iou) == aware
            assert ref.nms(q, s, lab, thr, True, iou) == agnostic
        assert len(aware) == 210 and len(agnostic) == 160 and aware != agnostic


# ------------------------------------------------------------------------------------------------------------ kernels
def test_exact_answers(emu):
    assert cases.check_exact_table(emu, CPU) > 100


def test_every_family_within_the_bound(emu):
    worst = cases.check_families(emu, CPU)
    print({k: f'{v:.3e}' for k, v in worst.items()}, 'BOUND', cases.BOUND)


def test_unit_shapes(emu):
    print(cases.check_unit_shapes(emu, CPU))


def test_corners_are_bit_equal_with_obb_to_numpy(emu):
    from rsprompter_amd import rle
    assert cases.check_corners(emu, rle, CPU) > 40


def test_nms_sizes_across_mask_word_edges(emu):
    print(cases.check_nms_sizes(emu, CPU, EMU_NMS_SIZES))


def test_nms_grid_with_a_second_removal_word_a_lane(emu):
    """n = 4097, 65 mask words.  The eight runs of cases.check_nms_grid take 21 s on the emulator against 3.3 s of this
    file's slowest test, so they are the device tier's (tests/test_gpu_obb_iou.py, with n = 16449); here one of them, 2.6 s:
    the permuted inputs, class-aware, so that the sort orders and the tail is kept in part"""
    q, s, lab, aware, _ = cases.nms_grid_permuted(cases.NMS_GRID_SIZES[0])
    assert cases.run_nms(emu, CPU, q, s, lab, cases.NMS_THRS[-1], False) == aware


def test_nms_rules(emu):
    cases.check_nms_rules(emu, CPU)


def test_bad_arguments_are_refused(emu):
    cases.check_refusals(emu, CPU, pytest)


def test_host_tensors_are_refused_before_a_launch(monkeypatch):
    from rsprompter_amd import ops
    monkeypatch.setattr(ops, '_is_device', lambda t: t.is_cuda)         # the product's test, whatever the emulator fixture set
    cases.check_refuses_host_tensors(ops, pytest)


def test_the_abi_version_stays_and_the_entry_points_are_declared():
    from rsprompter_amd import _lib
    assert _lib.CONST['RSP_ABI_VERSION'] == 6 and _lib.CONST['RSP_OBB_NMS_MAX'] == 32768
    for name in ('rsp_obb_corners', 'rsp_obb_iou', 'rsp_obb_nms', 'rsp_obb_nms_workspace_bytes'):
        assert name in _lib.PROTOTYPES


# ---------------------------------------------------------------------------------------------------------------- API
def test_obb_iou_and_nms_rotated_on_every_input_form(emu):
    from rsprompter_amd import apis, rle
    cases.check_api(apis, rle, CPU)
    cases.check_api_refusals(apis, CPU, pytest)


# ----------------------------------------------------------------------------------------------------------- pipeline
def test_two_ships_moored_side_by_side(emu):
    from rsprompter_amd import large_image as li
    cases.check_bars(li, CPU)


def test_nms_rotated_refusals_before_the_model_runs(emu):
    from rsprompter_amd import large_image as li
    cases.check_pipeline_refusals(li, CPU, pytest)


def test_random_stub_scene_matches_the_reference_nms(emu):
    """the merge around a random detector: keep = the reference NMS on the exact IoUs of the reference's rectangles"""
    import _large_image_ref as lref
    import _mask_obb_ref as oref
    import _seam_merge_cases as seam_cases
    from rsprompter_amd import large_image as li
    rng = np.random.default_rng(16)
    scene = rng.integers(0, 256, (45, 70, 3)).astype(np.uint8)
    model = seam_cases.RandomStub((32, 32))
    out, patches, start = li.inference_large_image(model, scene, 32, merge_iou_thr=0.25, merge_nms_type='nms_rotated',
                                                    return_patches=True)
    quads, scores, labels = [], [], []
    for p, (ox, oy) in zip(patches, start):
        pi = p.pred_instances
        for m in pi.masks.cpu().numpy():
            _, _, e, q = oref.obb(lref_embed(m, 45, 70, ox, oy))
            quads.append(np.full((4, 2), np.nan) if e < 0 else np.array([[float(v) for v in c] for c in oref.corners(q)]))
        scores += pi.scores.cpu().tolist()
        labels += pi.labels.cpu().tolist()
    quads = np.stack(quads)
    iou = ref.exact_iou_matrix(quads, quads)
    assert cases.decision_margin(iou, (0.25,)) > Fraction(cases.DECISION_MARGIN)
    want = ref.nms(quads, scores, labels, 0.25, False, iou)
    assert out.keep.cpu().tolist() == want and 3 < len(want) < len(scores)
    assert int(np.isnan(quads[:, 0, 0]).sum()) >= 1                              # empty masks among them: kept
    plain = li.inference_large_image(model, scene, 32, merge_iou_thr=0.25)
    assert plain.keep.cpu().tolist() != want


def lref_embed(m, H, W, ox, oy):
    full = np.zeros((H, W), bool)
    full[oy:oy + m.shape[0], ox:ox + m.shape[1]] = m
    return full


def test_cli_default_output_is_unchanged_and_the_new_choice(emu, tmp_path, monkeypatch):
    from PIL import Image
    import _seam_merge_cases as seam_cases
    from rsprompter_amd import apis
    from rsprompter_amd import large_image as li
    rng = np.random.default_rng(16)
    scene = rng.integers(0, 256, (45, 70, 3)).astype(np.uint8)
    model = seam_cases.RandomStub((32, 32))
    monkeypatch.setattr(apis, 'init_detector', lambda cfg, ckpt, device=None: model)
    Image.fromarray(scene).save(tmp_path / 'scene.png')
    src = str(tmp_path / 'scene.png')
    argv = [src, 'cfg.py', 'none', '--patch-size', '32', '--batch-size', '2', '--score-thr', '0.4']
    want = li.pred2dict(li.inference_large_image(model, src, 32, batch_size=2), 0.4)
    li.main(argv + ['--out-dir', str(tmp_path / 'a')])
    assert (tmp_path / 'a' / 'scene.json').read_text() == json.dumps(want)       # the default file: byte for byte
    li.main(argv + ['--out-dir', str(tmp_path / 'b'), '--merge-nms-type', 'nms_rotated'])
    rot = li.pred2dict(li.inference_large_image(model, src, 32, batch_size=2, merge_nms_type='nms_rotated'), 0.4)
    assert (tmp_path / 'b' / 'scene.json').read_text() == json.dumps(rot) and rot != want and set(rot) == set(want)


def test_evaluate_cli_passes_the_mode_and_the_metric_on(monkeypatch):
    """evaluate.py --large-image --merge-nms-type nms_rotated --obb: the mode goes through the existing large_image key, the
    flag through evaluate(obb=True)"""
    from rsprompter_amd import apis, config, evaluate
    assert evaluate.LARGE_IMAGE_KEYS[:4] == ('patch_size', 'patch_overlap_ratio', 'merge_iou_thr', 'merge_nms_type')
    seen = {}
    monkeypatch.setattr(evaluate.rdist, 'init_from_env', lambda: (0, 0, 1))
    monkeypatch.setattr(config.Config, 'fromfile', staticmethod(lambda path: config.Config(dict())))
    monkeypatch.setattr(apis, 'init_detector', lambda cfg, ckpt, device=None: 'model')
    monkeypatch.setattr(evaluate, 'evaluate', lambda model, cfg, *a, **kw: seen.update(kw, model=model) or {})
    evaluate.main(['cfg.py', 'none', '--large-image', '--merge-nms-type', 'nms_rotated', '--patch-size', '32', '--obb'])
    assert seen['obb'] is True and seen['large_image'] == dict(merge_nms_type='nms_rotated', patch_size=32)
    assert seen['model'] == 'model' and seen['boundary'] is False
    seen.clear()
    evaluate.main(['cfg.py', 'none'])
    assert seen['obb'] is False and seen['large_image'] is None                  # the defaults: nothing new is asked for
    with pytest.raises(SystemExit):
        evaluate.main(['cfg.py', 'none', '--large-image', '--merge-nms-type', 'soft_nms'])
    with pytest.raises(SystemExit):
        evaluate.main(['cfg.py', 'none', '--merge-nms-type', 'nms_rotated'])    # applies to --large-image


def test_evaluate_obb_appends_the_metric(monkeypatch):
    """evaluate(obb=True) adds 'obb' to the configured metric list once, beside boundary=True, and leaves it alone otherwise"""
    from rsprompter_amd import evaluate as E

    class Dataset:
        data_list, dataset_meta = [], dict(classes=('a',))

        def __len__(self):
            return 0
    built = []

    class Metric:
        def process(self, batch, samples):
            assert samples == []

        def evaluate(self, size):
            return {}

    class Registry:
        @staticmethod
        def build(cfg):
            built.append(dict(cfg))
            return Metric()
    monkeypatch.setattr(E, 'build_test_dataset', lambda cfg, data_root, ann_file: Dataset())
    monkeypatch.setattr(E, 'TestPipeline', lambda pipeline, device=None: None)
    monkeypatch.setattr(E, 'METRICS', Registry)
    cfg = dict(test_dataloader=dict(dataset=dict(pipeline=[]), batch_size=1), test_evaluator=dict(type='CocoMetric', metric=['bbox', 'segm']))
    for kw, want in ((dict(obb=True), ['bbox', 'segm', 'obb']), (dict(), ['bbox', 'segm']),
                     (dict(obb=True, boundary=True), ['bbox', 'segm', 'boundary', 'obb'])):
        assert E.evaluate(None, cfg, device='cpu', verbose=False, **kw) == {}
        assert built[-1]['metric'] == want, (kw, built[-1])
    cfg['test_evaluator']['metric'] = ['segm', 'obb']
    E.evaluate(None, cfg, device='cpu', verbose=False, obb=True)
    assert built[-1]['metric'] == ['segm', 'obb']


# -------------------------------------------------------------------------------------------------------------- metric
def test_no_exact_iou_of_the_metric_set_is_near_a_threshold():
    """dtm is compared for equality: the hand-made set's rectangles by the sequential reference and their exact IoUs, before
    and without any product call"""
    pairs, ties = cases.metric_precondition()
    print(f'{pairs} pairs of one image and category, none within {cases.DECISION_MARGIN} of a threshold')
    assert pairs > 300 and ties == 0


def test_metric_obb_against_the_restated_cocoeval(emu, tmp_path):
    from rsprompter_amd import apis, evaluation
    print(cases.check_metric(evaluation, apis, CPU, tmp_path))


def test_metric_obb_matches_at_exactly_the_threshold(emu):
    from rsprompter_amd import evaluation
    cases.check_metric_tie(evaluation, CPU)
    with pytest.raises(KeyError):
        evaluation.CocoMetric(metric='rotated')
    assert evaluation.CocoMetric(metric='obb').metrics == ['obb']
