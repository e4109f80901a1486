"""-m "not gpu": the detection selection kernels on the lane-level emulator (tests/wave_emu) against the restatements of
tests/_det_props.py -- a subset of every family's exact and sequence cases and the smallest tolerance case of each; the bodies
are the ones tests/test_gpu_det_props.py runs on the device.  The coverage of the case lists is asserted on the reference
alone (census), the fp32-sequence restatements are compared with the oracle's independent restatement of mmdet / mmcv
(oracle.glue), and the build flag the bit-exactness rests on is named."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'wave_emu'))

import _det_props as dp  # noqa: E402

CPU = torch.device('cpu')
F32, F64 = dp.F32, dp.F64
EMU_NMS = tuple(dp.nms_case(n) for n in ('cut-half', 'cut-717-1024ths', 'sizes-63-64', 'sizes-0-130', 'walk-300-max63', 'walk-300-max64', 'negative-unit-exact',
                                         'pool-0.7', 'negative-unit', 'pool-sizes-63-64'))
EMU_FLAT = tuple(dp.nms_case(n) for n in ('pool-0.5', 'sizes-1-65'))
EMU_DECODE = tuple(dp.decode_case(n) for n in ('dyadic-min16', 'means-stds-min0', 'ctr-clamp-exact', 'ctr-clamp-seq', 'clip-min0', 'seq-means'))
EMU_POST = tuple(dp.post_case(n) for n in ('nc3-thr0.25', 'nc1-thr0.5', 'ragged-0-first', 'seq-scaled')) + \
    tuple(c for c in dp.post_cases() if c.name.startswith('seq-odd-maxima-nc3'))
EMU_TOPK = tuple(c for c in dp.RPN_TOPK if c.emu)
EMU_QUERY = (dp.QueryCase(7, 3, 21), dp.QueryCase(64, 1, 10), dp.QueryCase(65, 1, 65), dp.QueryCase(128, 8, 100))


@pytest.fixture(scope='module')
def emu():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    import harness
    with harness.emulated_ops() as ops:
        yield ops


# --------------------------------------------------------------------------------------------------------------- the build flag
def test_the_selection_kernels_are_built_without_contraction():
    """the bit-exactness of det.hip and query.hip rests on -ffp-contract=off: global in rsprompter_amd/build.py, and no
    `// hipcc-flags:` line of either file may override it (or turn fast-math on); the emulated build carries it too"""
    from rsprompter_amd import build
    assert '-ffp-contract=off' in build.FLAGS
    assert not any(f.startswith('-ffp-contract') and f != '-ffp-contract=off' for f in build.FLAGS)
    assert not any('fast-math' in f or f == '-Ofast' for f in build.FLAGS)
    for name in ('det.hip', 'query.hip'):
        extra = build.file_flags(os.path.join(build.CSRC, name))
        assert not any('fp-contract' in f or 'fast-math' in f or f == '-Ofast' or 'unsafe-math' in f for f in extra), (name, extra)
        with open(os.path.join(build.CSRC, name)) as f:                      # ... nor a pragma inside the file
            text = f.read().lower()
        assert 'fp contract' not in text and 'fp_contract' not in text and 'fp reassociate' not in text, name
    with open(os.path.join(HERE, 'wave_emu', 'build.py')) as f:
        assert "'-ffp-contract=off'" in f.read()


# ----------------------------------------------------------------------------------------------------------------- the census
def test_the_nms_cases_cover_the_cuts_offsets_walks_and_sizes():
    from rsprompter_amd import ops
    cases = {c.name: c for c in dp.nms_cases()}
    # the threshold pool: 64 .. 128 pairs per threshold; >= 8 decided differently by the fp64 IoU, >= 8 with IoU == thr exactly,
    # one of each at every id offset; inter > thr * union decides differently somewhere
    cross = 0
    for thr in dp.POOL_THRESHOLDS:
        differ, equal, pairs = np.zeros(4, int), np.zeros(4, int), 0
        for seed, n in ((11, 64), (12, 48)):
            (boxes, _, ids), cen = dp.threshold_pool(thr, seed, n)
            pairs += n
            differ, equal, cross = differ + cen['differ'], equal + cen['equal'], cross + sum(cen['cross'])
            assert all(v >= 1 for v in cen['differ']) and all(v >= 1 for v in cen['equal']), (thr, seed, cen)
            assert set(ids.tolist()) == set(dp.IDS) and 1333 < float(boxes.max()) < 1334 and float(boxes.max()) % 1 != 0
        assert 64 <= pairs <= 128 and differ.sum() >= 8 and equal.sum() >= 8, (thr, pairs, differ, equal)
        assert cases[f'pool-{thr}'].tier == 'seq'
    assert cross >= 1
    # the offsets round: id * (max + 1) is no fp32 number for some id, and neither is box + offset
    (boxes, _, ids), _ = dp.threshold_pool(0.7, 11)
    unit = np.float32(boxes.max()) + np.float32(1)
    assert any(float(np.float32(i) * unit) != i * float(unit) for i in dp.IDS)
    off = ids.numpy().astype(np.float32) * unit
    assert ((boxes.numpy()[:, 0] + off).astype(np.float64) != boxes.numpy()[:, 0].astype(np.float64) + off.astype(np.float64)).any()
    for name in ('negative-unit', 'negative-unit-exact'):
        c = cases[name]
        assert all(float(c.boxes[b, :int(c.cnt[b])].max()) < -1 for b in range(c.B)) and len(set(c.ids[0, :int(c.cnt[0])].tolist())) > 1
    # every case: B = 2, counts below the capacity, the rows behind them poisoned with the largest coordinates and the top score
    for c in cases.values():
        assert c.B == 2
        for b in range(2):
            n = int(c.cnt[b])
            assert n < c.cap and float(c.boxes[b, n:].min()) > 9e29 and float(c.scores[b, n:].min()) > float(c.scores[b, :n].max() if n else 0)
    # order and walk: runs of equal scores longer than a block; chains inside a block, across blocks 0 -> 1, into word >= 64
    walk = cases['walk-4300']
    s = walk.scores[0, :4300]
    assert int(torch.unique(s, return_counts=True)[1].max()) > 64 and 4300 > 4096
    wref = walk.ref(F64)
    keep = set(wref['keep'][0, :int(wref['count'][0])].tolist())
    pos = torch.empty(4300, dtype=torch.long)                                # the sorted position of every row, from the case's scores
    pos[torch.sort(s, descending=True, stable=True)[1]] = torch.arange(4300)
    wb = walk.boxes[0, :4300]
    chains = []
    for b in range(4300):                                                    # a suppressed row, the row that suppresses it and the row it would suppress
        if b not in keep:
            a = next(i for i in keep if torch.equal(wb[i] + torch.tensor([4.0, 0, 4.0, 0]), wb[b]))
            c = next(i for i in range(4300) if torch.equal(wb[b] + torch.tensor([4.0, 0, 4.0, 0]), wb[i]))
            assert c in keep and pos[a] < pos[b] < pos[c]
            chains.append((int(pos[a]) // 64, int(pos[b]) // 64, int(pos[c]) // 64))
    assert any(a == b == c for a, b, c in chains), chains                    # inside one 64-row block
    assert any(a == 0 and b == 1 for a, b, c in chains), chains              # from block 0 into block 1
    assert any(a < 64 <= b for a, b, c in chains) and any(a >= 1 and b >= 64 for a, b, c in chains), chains    # into a word index >= 64
    # max_out: reached mid-block, on the last row of a block, on the first row of a block, and never (max_out > n)
    ends = {}
    for n, c in cases.items():
        if n.startswith('walk-300'):
            r = c.ref(F64)
            k = int(r['count'][0])
            sc = c.scores[0, :int(c.cnt[0])]
            p = torch.empty(sc.numel(), dtype=torch.long)
            p[torch.sort(sc, descending=True, stable=True)[1]] = torch.arange(sc.numel())
            ends[c.max_out] = (k, int(p[int(r['keep'][0, k - 1])]) % 64, int(c.cnt[0]))
    assert set(ends) == {37, 63, 64, 128, 400}
    assert ends[63][0] == 63 and ends[63][1] == 63                           # the last kept row is the last row of block 0
    assert ends[37][0] == 37 and ends[37][1] not in (0, 63) and ends[64] == (64, 0, 300)
    assert ends[400][0] < 400 and ends[400][2] < 400                         # max_out > n: the walk ends at n
    assert {int(v) for n, c in cases.items() if n.startswith('sizes') for v in c.cnt} == {0, 1, 63, 64, 65, 130}
    assert {int(v) for n, c in cases.items() if n.startswith('pool-sizes') for v in c.cnt} == {63, 64, 65, 130}     # ... the pool embedded
    assert ops.NMS_LDS_CANDIDATES == 16384 and {c.cap for c in cases.values() if c.name.startswith('pool-cap')} == {16384, 16385}
    assert (16384 + 63) // 64 <= 256 < (16385 + 63) // 64                   # the 4-word and the 32-word reduce
    # degenerate: zero-area boxes (0 / 0: kept) and identical twins
    d = cases['sizes-0-130']
    bx = d.boxes[1, :130]
    assert int(((bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1]) == 0).sum()) >= 3 and torch.equal(bx[1], bx[3]) and torch.equal(bx[2], bx[7])
    k = d.ref(F64)['keep'][1].tolist()
    assert 1 in k and 3 in k and 2 in k and 7 not in k
    # the exact cuts: both boxes of a pair at IoU == thr are kept, the pair one grid step above loses its second box
    for name, num in (('cut-half', 512), ('cut-five-16ths', 320), ('cut-717-1024ths', 717)):
        c = cases[name]
        assert c.thr == num / 1024 and float(np.float32(c.thr)) == c.thr
        kept = int(c.ref(F64)['count'][0])
        assert kept == 48 - 8, (name, kept)                                   # 24 pairs, every third one step above


def test_the_decode_cases_cover_every_coder_branch_clip_and_compaction():
    cases = {c.name: c for c in dp.decode_cases()}
    coders = [c.coder for c in cases.values()]
    assert any(any(m != 0 for m in c.means) for c in coders) and any(any(s != 1 for s in c.stds) for c in coders)
    assert {c.clip_border for c in coders} == {True, False} and {c.add_ctr_clamp for c in coders} == {True, False}
    assert {c.min_size for c in cases.values()} >= {0.0, -1.0, 16.0, dp._below(16.0)}
    assert all(c.ld > 5 * c.A and c.B == 2 for c in cases.values()) and {c.A for c in cases.values()} == {3, 6}
    # the centre clamp: pw * dx exactly at +-ctr_clamp, one ulp beyond and (sequence tier) one ulp inside; dw far below -max_ratio
    for name, inside in (('ctr-clamp-exact', False), ('ctr-clamp-seq', True)):
        c = cases[name]
        lvl0 = c.heads[0][:12 * 16]
        dxs = {float(v) * 32.0 for v in lvl0[:, c.A].tolist() if v != 77.0}
        cc = c.coder.ctr_clamp
        assert {cc, -cc, dp._above(cc), -dp._above(cc)} <= dxs and ({dp._below(cc), -dp._below(cc)} <= dxs) == inside, (name, sorted(dxs))
        assert float(lvl0[:, c.A + 2].min()) == -128.0 and c.coder.add_ctr_clamp
    # the clip: before it, x1 < 0, x2 and y2 exactly on the image's side and one ulp above, boxes wholly outside
    c = cases['clip-min0']
    raw = dp._with(c, coder=c.coder._replace(clip_border=False), min_size=-1.0).ref(F32)[0][0]
    h, w = c.img_hw[0].tolist()
    assert bool((raw[:, 0] < 0).any()) and bool((raw[:, 2] == w).any()) and bool((raw[:, 2] == dp._above(w)).any())
    assert bool((raw[:, 3] == h).any()) and bool((raw[:, 3] == dp._above(h)).any()) and bool((raw[:, 2] < 0).any()) and bool((raw[:, 0] > w).any())
    assert int(cases['clip-min0'].ref(F64)[4][0]) < int(cases['clip-min-1'].ref(F64)[4][0]) == int(c.sel_cnt[0].sum())
    # min_bbox_size: a side exactly min_size is dropped, the float below min_size keeps it
    a, b = cases['dyadic-min16'], cases['dyadic-min' + f'{dp._below(16.0):.9g}']
    assert int(a.ref(F64)[4].sum()) < int(b.ref(F64)[4].sum())
    # compaction: per-level survivors of 0, 1, 1023, 1024, 1025 (and all), an emptied level between two others, cap = L * nms_pre
    c = cases['compaction']
    ref = c.ref(F64)
    counts = {int((ref[2][b, :int(ref[4][b])] == l).sum()) for b in range(2) for l in range(3)}
    assert counts >= set(dp.COMPACTION_COUNTS) and c.cap == c.L * c.k
    assert int((ref[2][0, :int(ref[4][0])] == 1).sum()) == 0 and int(c.sel_cnt[0, 1]) > 1024
    # the sequence tier: stds (0.1, 0.1, 0.2, 0.2), dw = dh = 0, anchors whose sides are no powers of two
    for name in ('seq-real', 'seq-real-no-clip', 'seq-means'):
        c = cases[name]
        assert c.tier == 'seq' and c.coder.stds == (0.1, 0.1, 0.2, 0.2) and 'centre_contracted' in c.kills
    assert 'delta_contracted' in cases['seq-means'].kills
    # the tolerance tier: dw exactly at max_ratio, one ulp either side, beyond it; far below -max_ratio under the centre clamp
    mr = np.float32(dp.MAX_RATIO)
    for c in dp.DECODE_TOL:                                                  # fp32(d) * fp32(0.2), as the kernel and the fp32 sequence compute it
        dws = {v for hd in c.heads for a in range(c.A) for v in (hd[:, c.A + 4 * a + 2].numpy() * np.float32(0.2)).tolist()}
        assert {float(mr), float(np.nextafter(mr, np.float32(0))), float(np.nextafter(mr, np.float32(9))), float(-mr), 100.0, -100.0} <= dws, c.name
    assert any(c.coder.add_ctr_clamp for c in dp.DECODE_TOL) and any(not c.coder.clip_border for c in dp.DECODE_TOL)


def test_the_bbox_post_and_top_k_cases_cover_what_they_claim():
    posts = dp.post_cases()
    assert {c.nc for c in posts} == {1, 3, 7, 10} and all(c.B == 3 for c in posts)
    assert all(0 in (c.roi_start[1:] - c.roi_start[:-1]).tolist() for c in posts)
    assert {c.score_thr for c in posts} >= {0.5, dp._below(0.5), 0.25, dp._below(0.25)}
    for c in posts:
        assert float(c.head[:, :c.nc + 1].max()) == 100.0                     # a row of logits at 100: the max is subtracted
        ref = c.ref(F64, iou_thr=1.0)
        assert not bool((ref['ids'] == c.nc).any())                           # the background never becomes a candidate
    many = dp.post_case('many-nc10')
    assert int(many.ref(F64, iou_thr=1.0)['cand_count'].max()) > 1024 and (1100 * 10) % 1024 != 0
    sc = dp.post_case('seq-scaled')
    assert sc.tier == 'seq' and any(float(np.float32(1 / s)) * s != 1.0 or (s * 1024) % 1 != 0 for sf in sc.scale_factors for s in sf)
    # score == score_thr is dropped, one ulp above is kept: the same rows at 1/j and at the float below it
    a, b = dp.post_case('nc3-thr0.5'), dp.post_case('nc3-thr' + f'{dp._below(0.5):.9g}')
    assert a.ref(F64, iou_thr=1.0)['scores'].eq(0.5).sum() == 0 < b.ref(F64, iou_thr=1.0)['scores'].eq(0.5).sum()
    # rpn_topk: n <= k, n = k + 1, the k-th score inside runs of 2 / 1024 / 1025 ties, all-equal levels, the eight-wide scan and its tail
    seen = dict(le=0, plus1=0, n_eq=set(), equal=0, wide=0)
    for c in dp.RPN_TOPK:
        assert c.ld > 5 * c.A
        for (H, W), *pats in c.levels:
            n = H * W * c.A
            seen['le'] += n <= c.k
            seen['plus1'] += n == c.k + 1
            seen['wide'] += n > 8 * 1024 + 100 and (n - 8 * 1024) % 1024 != 0
            assert pats[0] != pats[1]                                          # the two images carry different tie patterns
            for p in pats:
                seen['equal'] += p[0] == 'equal'
                if p[0] == 'kth':
                    seen['n_eq'].add(p[2])
    assert seen['le'] and seen['plus1'] >= 2 and seen['equal'] and seen['wide'] and seen['n_eq'] >= {2, 1024, 1025}, seen
    assert {c.A for c in dp.RPN_TOPK} == {3, 6} and {c.k for c in dp.RPN_TOPK} >= {1, 1000, 1024}
    heads, _, _ = dp.topk_inputs(dp.RPN_TOPK[0])
    vals = torch.cat([h[:, :3].reshape(-1) for h in heads])
    assert bool(((vals == 0) & torch.signbit(vals)).any()) and bool(((vals == 0) & ~torch.signbit(vals)).any())
    # query_topk: k = 1 and k = Nq nc; Nq nc a power of two and one above it; nc = 1; ties across queries and classes
    div = [c for c in posts if 'division_by_truncated_reciprocal' in c.kills]
    assert len(div) >= 2 and all(c.tier == 'seq' for c in div) and {c.nc for c in div} == {3, 10}      # maxima of 3, and of 3 .. 11
    odd = dp.query_topk_ref(dp.query_exact_inputs(dp.QUERY_SEQ[0], maxima=(1, 3, 5, 6, 7, 9, 10, 11)), 400, F32)[0][0].unique().tolist()
    assert float(np.float32(1) / np.float32(3)) in odd and float(np.float32(1) / np.float32(7)) in odd
    q = dp.QUERY_EXACT
    assert any(c.k == 1 for c in q) and any(c.k == c.Nq * c.nc for c in q) and any(c.nc == 1 for c in q)
    assert {1024, 1025, 64, 65} <= {c.Nq * c.nc for c in q}
    s = dp.query_topk_ref(dp.query_exact_inputs(dp.QueryCase(128, 8, 1024)), 1024, F64, exact=True)[0][0]
    assert set(s.unique().tolist()) == {0.0, 0.25, 0.5, 1.0}


# ----------------------------------------------------------------------------------- two independent restatements that agree
def test_the_fp32_sequence_restatements_agree_with_the_oracle_glue():
    """once per case list: the same kept indices and boxes as oracle.glue's delta2bbox, batched_nms (the C restatement of mmcv
    nms), multiclass_nms / bbox_head_predict_single and rpn_predict_single"""
    from oracle import glue
    for c in dp.nms_cases():
        for b in range(c.B):
            n = int(c.cnt[b])
            want = dp.nms_keep(c.boxes[b].numpy(), c.scores[b].numpy(), c.ids[b].numpy(), n, c.thr, c.max_out, F32)
            got = glue.batched_nms(c.boxes[b, :n], c.scores[b, :n], c.ids[b, :n].long(), c.thr)[1][:c.max_out].tolist() if n else []
            assert got == want, ('batched_nms', c.name, b)
    g = torch.Generator().manual_seed(4)
    for c in dp.decode_cases() + dp.DECODE_TOL:
        xy = torch.rand(200, 2, generator=g) * 300
        an = torch.cat([xy, xy + torch.rand(200, 2, generator=g) * 200 + 1], 1)
        d = torch.cat([c.heads[0][:150, c.A:c.A + 4], torch.randn(50, 4, generator=g) * 3])
        d = torch.where(d == 77.0, torch.zeros_like(d), d)
        co = c.coder
        want = dp.decode_boxes(an, d, co, torch.tensor(333.0), torch.tensor(417.0), F32)
        got = glue.delta2bbox(an, d, co.means, co.stds, max_shape=(333.0, 417.0), clip_border=co.clip_border,
                              add_ctr_clamp=co.add_ctr_clamp, ctr_clamp=co.ctr_clamp)
        assert torch.equal(got, want), ('delta2bbox', c.name, dp._first_diff(got, want))
    for c in dp.post_cases():
        ref = c.ref(F32)
        for b in range(c.B):
            r0, r1 = int(c.roi_start[b]), int(c.roi_start[b + 1])
            if r1 == r0:
                assert int(ref['count'][b]) == 0
                continue
            co = c.coder
            dets, labels, inds = glue.bbox_head_predict_single(
                c.rois[r0:r1], c.head[r0:r1, :c.nc + 1], c.head[r0:r1, c.nc + 1:5 * c.nc + 1].contiguous(), tuple(c.img_hw[b].tolist()), c.nc,
                c.score_thr, c.iou_thr, c.max_out, stds=co.stds, scale_factor=None if c.scale_factors is None else c.scale_factors[b],
                coder=dict(means=co.means, clip_border=co.clip_border, add_ctr_clamp=co.add_ctr_clamp, ctr_clamp=co.ctr_clamp))
            m = int(ref['count'][b])
            assert dets.shape[0] == m and torch.equal(inds.int(), ref['src'][b, :m]) and torch.equal(labels.int(), ref['ids'][b, :m]), (c.name, b)
            assert torch.equal(dets[:, :4], ref['boxes'][b, :m]) and torch.equal(dets[:, 4], ref['scores'][b, :m]), (c.name, b)
    # the RPN chain on an exact top-k case: top-k -> decode -> NMS against rpn_predict_single
    case = dp.RPN_TOPK[-1]
    heads, sizes, B = dp.topk_inputs(case)
    gh = torch.Generator().manual_seed(8)
    for hd in heads:
        hd[:, case.A:5 * case.A] = torch.randn(hd.shape[0], 4 * case.A, generator=gh) * 0.5
    strides = [4.0, 8.0, 16.0]
    base = [glue.gen_base_anchors(s, [8], [0.5, 1.0, 2.0]) for s in strides]
    priors = glue.grid_priors(sizes, strides, [8], [0.5, 1.0, 2.0])
    img_hw = torch.tensor([[120.0, 160.0]] * B)
    sel = dp.rpn_topk_ref(heads, sizes, case.ld, case.A, case.k, B, F32)
    cap = len(sizes) * case.k
    cand = dp.rpn_decode_ref(heads, sizes, strides, case.ld, case.A, case.k, base, dp._CODER_DYADIC, 0.0, *sel, img_hw, cap, F32)
    out = dp.nms_ref(*cand, 0.7, 100, F32)
    for b in range(B):
        cls = [hd[b * H * W:(b + 1) * H * W, :case.A].reshape(H, W, case.A).permute(2, 0, 1) for hd, (H, W) in zip(heads, sizes)]
        reg = [hd[b * H * W:(b + 1) * H * W, case.A:5 * case.A].reshape(H, W, 4 * case.A).permute(2, 0, 1) for hd, (H, W) in zip(heads, sizes)]
        r = glue.rpn_predict_single(cls, reg, priors, tuple(img_hw[b].tolist()), nms_pre=case.k, max_per_img=100, iou_thr=0.7, min_bbox_size=0)
        m = int(out['count'][b])
        assert r['bboxes'].shape[0] == m and torch.equal(r['bboxes'], out['boxes'][b, :m]), ('rpn chain', b)
        assert torch.equal(r['level_ids'].int(), out['ids'][b, :m]) and torch.equal(r['anchor_index'].int(), out['src'][b, :m]), ('rpn chain', b)


# ------------------------------------------------------------------------------------------------------------- the emulator
@pytest.mark.parametrize('case', EMU_NMS, ids=lambda c: c.name)
def test_batched_nms_on_the_emulator(emu, case):
    dp.check_nms(emu, CPU, case)


@pytest.mark.parametrize('case', EMU_FLAT, ids=lambda c: c.name)
def test_nms_flat_on_the_emulator(emu, case):
    dp.check_nms_flat(emu, CPU, case)


@pytest.mark.parametrize('case', EMU_DECODE, ids=lambda c: c.name)
def test_rpn_decode_on_the_emulator(emu, case):
    dp.check_decode(emu, CPU, case)


@pytest.mark.parametrize('case', EMU_POST, ids=lambda c: c.name)
def test_bbox_post_on_the_emulator(emu, case):
    dp.check_post(emu, CPU, case)


@pytest.mark.parametrize('case', EMU_TOPK, ids=lambda c: c.name)
def test_exact_rpn_topk_on_the_emulator(emu, case):
    dp.check_exact_rpn_topk(emu, CPU, case)


@pytest.mark.parametrize('case', EMU_QUERY, ids=dp.case_id)
def test_exact_query_topk_on_the_emulator(emu, case):
    dp.check_exact_query_topk(emu, CPU, case)


@pytest.mark.parametrize('case', dp.QUERY_SEQ[:2], ids=dp.case_id)
def test_query_topk_division_on_the_emulator(emu, case):
    dp.check_seq_query_topk(emu, CPU, case)


def test_the_smallest_tolerance_cases_on_the_emulator(emu):
    quiet = lambda line: None
    dp.check_decode_tolerance(emu, CPU, quiet, cases=dp.DECODE_TOL[1:2])
    dp.check_post_tolerance(emu, CPU, quiet, cases=dp.BBOX_TOL[2:])
    dp.check_rpn_topk_tolerance(emu, CPU, quiet, cases=dp.RPN_TOL[:1])
    dp.check_query_topk_tolerance(emu, CPU, quiet, cases=dp.QUERY_TOL[2:])
