"""Bodies of the panoptic-fusion tests (csrc/panoptic_fuse.hip, ops.panoptic_fuse, the fusion heads' panoptic_on branch),
shared by tests/test_panoptic_cpu.py (the lane-level emulator) and tests/test_gpu_panoptic.py (the device), in the style of
tests/_mask_field_props.py, whose oracle `field_f64`, logit recipe, case lists, VALUE_TOL and NEAR they use.  The reference is
tests/_panoptic_ref.py: two forms of panoptic_postprocess on the fp64 field that must agree.

Exact tier: dyadic geometries and integer logits, so the kernel's field values are the fp64 ones bit for bit; what is left
of fp32 is the product score * sigmoid(v).  A pixel is NEAR when its two largest fp64 products differ by at most 1e-6 (8 ulp
of fp32 at 1.0: 1-2 ulp each of exp2 and rcp, a few of the softmax, half of the product) without being exact duplicates; the
seeds below have no such pixel, the bodies assert that on the reference, and then everything is ==.

Tolerance tier: non-dyadic geometries, the project's logit recipe.  NEAR is (s1 + s2) VALUE_TOL / 4 + 1e-6 (sigmoid' <= 1/4:
a field error of VALUE_TOL moves a product by at most s VALUE_TOL / 4); the map is == away from near pixels, mask_area within
the near count, original_area within the count of |v| < mf.NEAR, and iou_thr sits in the widest gap of the reference's
ratios, far enough from each that those slacks cannot change a decision (asserted), so `segment` is ==."""
import math

import torch

import _mask_field_props as mf
import _panoptic_ref as pr

NC, NTHINGS = 3, 2                      # classes 0, 1: things; 2: stuff; 3: background
EXACT_NEAR = 1e-6


def geo_of(case):
    return (case.img, case.crop, case.out)


def run(ops, dev, cls, low, geo, num_things=NTHINGS, nc=NC, **cfg):
    """ops.panoptic_fuse -> (sem int32 [oh, ow] on the CPU, info as lists)"""
    sem, info = ops.panoptic_fuse(cls.to(dev), low.to(dev), *geo, num_things, nc, **cfg)
    assert sem.dtype == torch.int32 and tuple(sem.shape) == tuple(geo[2])
    assert info['score'].dtype == torch.float32 and all(info[k].dtype == torch.int32 for k in ('segment', 'mask_area', 'original_area'))
    return sem.cpu(), {k: v.cpu().tolist() for k, v in info.items()}


def assert_same(sem, info, r, what):
    bad = (sem != r['sem']).nonzero()
    assert bad.numel() == 0, (what, 'map', int(bad.shape[0]), bad[0].tolist(), int(sem[tuple(bad[0])]), int(r['sem'][tuple(bad[0])]))
    for k in ('segment', 'mask_area', 'original_area'):
        assert info[k] == r[k], (what, k, info[k], r[k])
    err = max(abs(a - float(b)) for a, b in zip(info['score'], r['score']))
    assert err <= 1e-6, (what, 'score', err)


def near_exact(r):
    return (r['gap'] <= EXACT_NEAR) & ~r['duplicate']


def class_rows(labels, margins, seed=0):
    """[Nq, NC + 1] logits: small noise (|.| <= 0.2) with `margin` added at the query's label"""
    g = torch.Generator().manual_seed(1000 + seed)
    cls = (torch.rand(len(labels), NC + 1, generator=g) - 0.5) * 0.4
    for q, (c, m) in enumerate(zip(labels, margins)):
        cls[q, c] += m
    return cls.contiguous()


# Nq = 12: eight kept (things and stuff mixed), two under the threshold (queries 1 and 7), two background (4 and 10)
EXACT_LABELS = (0, 1, 1, 2, 3, 0, 2, 0, 1, 0, 3, 2)
EXACT_MARGINS = (2.9, 1.0, 3.2, 3.5, 4.0, 3.8, 4.1, 2.0, 4.4, 4.7, 3.0, 5.0)


def exact_inputs(case, seed, thr=0.8):
    """(cls [12, 4], low [12, h, w] integer logits); the preconditions of the tier are asserted on the reference alone"""
    cls = class_rows(EXACT_LABELS, EXACT_MARGINS)
    p = torch.softmax(cls.double(), -1)
    top = p.topk(2, -1).values
    score, label, keep = pr.select(cls, NC, thr)
    assert float((score - thr).abs().min()) >= 1e-3 and float((top[:, 0] - top[:, 1]).min()) >= 1e-3
    assert int(keep.sum()) == 8 and bool(((label != NC) & ~keep).any()) and bool((label == NC).any())
    assert label.tolist() == list(EXACT_LABELS)
    g = torch.Generator().manual_seed(seed)
    low = torch.randint(-8, 9, (12,) + tuple(case.hw), generator=g).float()
    return cls, low


# per exact case: the first seed of 0, 1, 2, ... at which no pixel is near under either configuration of check_exact (found
# on the reference alone; the body asserts it)
EXACT_CFGS = (dict(object_mask_thr=0.8, iou_thr=0.8, filter_low_score=False), dict(object_mask_thr=0.8, iou_thr=0.25, filter_low_score=True))
EXACT_SEEDS = {}                        # seed 0 has no near pixel on any of mf.EXACT_CASES


def exact_seed(case):
    return EXACT_SEEDS.get(mf.case_id(case), 0)


def check_exact(ops, dev, case, seed=None):
    cls, low = exact_inputs(case, exact_seed(case) if seed is None else seed)
    mf.assert_case_is_exact(case, low)
    outcomes = set()
    for cfg in EXACT_CFGS:
        r = pr.reference(cls, low, geo_of(case), NTHINGS, NC, **cfg)
        n = int(near_exact(r).sum())
        assert n == 0, ('the reference has', n, 'near pixels: another seed', case)
        outcomes |= {s >= 0 for q, s in enumerate(r['segment']) if q in r['kept']}
        sem, info = run(ops, dev, cls, low, geo_of(case), **cfg)
        assert_same(sem, info, r, (case, cfg))
    return outcomes


def check_exact_ties(ops, dev, case, seed=3):
    """queries 2 and 8 (both kept things) become bit-identical: 2 wins every pixel the pair leads, 8 wins none and takes no id"""
    cls, low = exact_inputs(case, seed)
    cls[8], low[8] = cls[2], low[2]
    cfg = dict(iou_thr=0.0)
    r = pr.reference(cls, low, geo_of(case), NTHINGS, NC, **cfg)
    assert int(near_exact(r).sum()) == 0, 'another seed'
    assert bool(r['duplicate'].any()), 'the pair leads no pixel: another seed'
    assert r['mask_area'][2] > 0 and r['mask_area'][8] == 0 and r['segment'][8] == -1 and r['original_area'][8] == r['original_area'][2]
    things = sorted(s // 1000 for s in r['segment'] if s >= 1000)
    assert things == list(range(1, len(things) + 1))
    sem, info = run(ops, dev, cls, low, geo_of(case), **cfg)
    assert_same(sem, info, r, ('ties', case))


# ------------------------------------------------------------------------------------------------------------ hand-checked
G11 = ((4, 4), (4, 4), (4, 4))                 # 1 x 1 logits -> 4 x 4: the field of a query is its one logit
G88 = ((32, 32), (32, 32), (32, 32))           # 8 x 8 logits -> 32 x 32


def halves(left, right):
    """[8, 8] logits: `left` in columns 0-3, `right` in columns 4-7"""
    t = torch.empty(8, 8)
    t[:, :4], t[:, 4:] = left, right
    return t


def both(ops, dev, cls, low, geo, **cfg):
    """reference and device; no near pixel; == ; returns (reference, map)"""
    r = pr.reference(cls, low, geo, NTHINGS, NC, **cfg)
    assert int(near_exact(r).sum()) == 0
    sem, info = run(ops, dev, cls, low, geo, **cfg)
    assert_same(sem, info, r, cfg)
    return r, sem


def check_two_stuff_queries_share_the_label(ops, dev):
    cls = class_rows((2, 2), (3.0, 4.0))
    low = torch.stack([halves(8.0, -8.0), halves(-8.0, 8.0)])
    r, sem = both(ops, dev, cls, low, G88)
    assert r['segment'] == [2, 2] and r['mask_area'] == [512, 512] and bool((sem == 2).all())


def check_rejected_thing_leaves_no_gap(ops, dev):
    """query 1 (a thing) is positive on the whole left half but wins only its lower quarter: rejected at 0.8; the things
    before and after it get ids 1 and 2"""
    cls = class_rows((0, 1, 0), (4.0, 3.0, 3.5))
    q0 = torch.full((8, 8), -8.0)
    q0[:6, :4] = 8.0
    low = torch.stack([q0, halves(2.0, -8.0), halves(-8.0, 8.0)])
    r, sem = both(ops, dev, cls, low, G88)
    assert r['segment'] == [1000, -1, 2000], r['segment']
    assert 0 < r['mask_area'][1] < 0.8 * r['original_area'][1] and r['original_area'][1] == 32 * 15      # columns 0 .. 14
    assert int((sem == NC).sum()) == r['mask_area'][1]                    # its pixels stay void
    r2, _ = both(ops, dev, cls, low, G88, iou_thr=0.1)
    assert r2['segment'] == [1000, 2001, 3000]


def check_negative_everywhere(ops, dev):
    """one kept query whose one logit is -3: it wins all 16 pixels, original_area is 0, nothing is painted"""
    cls = class_rows((0,), (4.0,))
    r, sem = both(ops, dev, cls, torch.full((1, 1, 1), -3.0), G11)
    assert r['mask_area'] == [16] and r['original_area'] == [0] and r['segment'] == [-1] and bool((sem == NC).all())


def check_zero_counts_as_inside(ops, dev):
    """a logit of exactly 0: sigmoid = 0.5 >= 0.5, so original_area = 16 and the query is painted, with the filter too"""
    cls = class_rows((1,), (4.0,))
    for filt in (False, True):
        r, sem = both(ops, dev, cls, torch.zeros(1, 1, 1), G11, filter_low_score=filt)
        assert r['mask_area'] == [16] and r['original_area'] == [16] and r['segment'] == [1001] and bool((sem == 1001).all())


def check_none_kept(ops, dev):
    cls = class_rows((3, 0, 1), (4.0, 1.0, 0.5))
    for geo, hw in ((G11, (1, 1)), (G88, (8, 8))):
        r, sem = both(ops, dev, cls, torch.ones((3,) + hw), geo)
        assert r['kept'] == [] and r['segment'] == [-1, -1, -1] and r['mask_area'] == [0, 0, 0] and bool((sem == NC).all())


def check_filter_counts_the_area_before_it(ops, dev):
    """query 0 wins 768 pixels, 256 of them inside its positive half of 512: 768 / 512 passes 0.8, 256 / 512 would not.  It
    is painted, on those 256 pixels; the 512 it wins with a negative field stay void"""
    cls = class_rows((0, 2), (3.0, 4.5))
    q1 = torch.full((8, 8), -8.0)
    q1[:4, :4] = 8.0                                   # takes the upper half of query 0's positive region
    low = torch.stack([halves(8.0, -6.0), q1])
    r, sem = both(ops, dev, cls, low, G88, filter_low_score=True)
    won = r['winner'] == 0
    inside = r['field'][0] >= 0
    assert r['original_area'][0] == 512 and r['mask_area'][0] / 512 >= 0.8 > int((won & inside).sum()) / 512
    assert r['segment'][0] == 1000 and int((sem == 1000).sum()) == int((won & inside).sum()) > 0
    assert bool((sem[won & ~inside] == NC).all())
    r2, sem2 = both(ops, dev, cls, low, G88, filter_low_score=False)
    assert int((sem2 == 1000).sum()) == r2['mask_area'][0]


# found by a search over small integer logits on the reference alone: query 0 (a thing) wins 4 of the 5 / 8 of the 16 pixels
# on which its field is >= 0
RATIO_Q1_45 = ((2, 8, -2, -6, 5, -4, -6, -1), (-2, 5, 5, -2, 2, -1, -7, 4), (6, 2, 7, -3, -5, -7, 6, -1), (-5, 5, 4, -4, -6, -6, -4, 3),
               (3, 0, -5, -7, 4, 7, 4, 7), (-2, 6, 4, 3, 6, 1, 1, -2), (-5, 7, 2, -3, -8, -1, -4, 1), (-2, 6, 4, -8, 4, -4, -7, -6))
RATIO_Q1_816 = ((0, -8, 6, -1, 6, -7, -2, 0), (-3, 8, 6, 1, 6, -3, 5, -1), (-6, 0, -5, -8, 3, -2, 1, 1), (-7, -8, -7, -4, -7, -2, 8, 5),
                (8, -7, 5, -3, 3, -4, 2, 8), (8, -4, 2, 7, 0, 3, 2, 8), (-8, -6, -5, 0, -6, 0, 2, -4), (-2, 2, -6, 7, 0, 0, 1, -2))


def check_ratio_equal_to_the_threshold_is_kept(ops, dev):
    cls = torch.zeros(2, NC + 1)
    cls[0, 0], cls[1, 2] = 3.0, 4.0
    for (ma, oa, thr), cells, q1 in (((4, 5, 0.8), {(1, 7): -4.0, (2, 7): 2.0}, RATIO_Q1_45),
                                     ((8, 16, 0.5), {(2, 6): 5.0, (6, 6): 7.0}, RATIO_Q1_816)):
        q0 = torch.full((8, 8), -8.0)
        for yx, v in cells.items():
            q0[yx] = v
        low = torch.stack([q0, torch.tensor(q1, dtype=torch.float32)])
        r, sem = both(ops, dev, cls, low, G88, iou_thr=thr)
        assert (r['mask_area'][0], r['original_area'][0]) == (ma, oa) and ma / oa == thr
        assert r['segment'][0] == 1000 and int((sem == 1000).sum()) == ma
        above = float(torch.nextafter(torch.tensor(thr, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64)))
        r, sem = both(ops, dev, cls, low, G88, iou_thr=above)
        assert r['segment'][0] == -1 and int((sem == 1000).sum()) == 0


# ------------------------------------------------------------------------------------------------ more kept than a wave
def wave_inputs(reject_every_third):
    """70 things, all kept: query i < 64 has +8 in cell i of the 8 x 8 logits, queries 64 .. 69 have +4 on the cell pairs
    (8 j, 8 j + 1) and lead the band between them.  reject_every_third: queries 0, 3, 6, ... are +1 instead of -8 elsewhere:
    original_area 1024, far more than they win"""
    n = 70
    cls = class_rows([i % 2 for i in range(n)], [3.0 + 0.02 * i for i in range(n)])
    low = torch.full((n, 8, 8), -8.0)
    for i in range(64):
        if reject_every_third and i % 3 == 0:
            low[i] = 1.0
        low[i, i // 8, i % 8] = 8.0
    for j in range(6):
        low[64 + j, j, 0:2] = 4.0
    return cls, low


def check_more_kept_than_a_wave(ops, dev):
    cls, low = wave_inputs(False)
    r, sem = both(ops, dev, cls, low, G88, iou_thr=0.05)
    assert len(r['kept']) == 70 and min(r['mask_area']) > 0
    assert [s // 1000 for s in r['segment']] == list(range(1, 71)), r['segment']
    cls, low = wave_inputs(True)
    r, sem = both(ops, dev, cls, low, G88, iou_thr=0.08)
    third = list(range(0, 64, 3))
    assert all(r['segment'][q] < 0 and r['mask_area'][q] > 0 and r['original_area'][q] == 1024 for q in third)     # by the ratio
    rest = [q for q in range(70) if q not in third]
    assert all((r['segment'][q] >= 0) == (r['mask_area'][q] > 0) for q in rest) and sum(r['segment'][q] >= 0 for q in rest) >= 40
    painted = [r['segment'][q] // 1000 for q in range(70) if r['segment'][q] >= 0]
    assert painted == list(range(1, len(painted) + 1))


# ---------------------------------------------------------------------------------------------------------------- refusals
def check_refusals(ops, dev, wrong_device):
    """ValueError on the host before any launch; RuntimeError from RSP_EINVAL for more queries than the cap (the kept count
    stays on the device, so the cap is on the queries) and for an invalid geometry"""
    import pytest
    cls, low = class_rows((0, 2), (3.0, 4.0)).to(dev), torch.zeros(2, 8, 8, device=dev)
    for bad in (low[:, :, ::2], low.double(), low[0], low.half(), low.to(wrong_device)):
        with pytest.raises(ValueError):
            ops.panoptic_fuse(cls, bad, *G88, NTHINGS, NC)
    cls8 = torch.zeros(2, 8, device=dev)
    for bad in (cls8[:, ::2], cls.double(), cls[0], cls[:1], cls8[:, :5].contiguous(), cls.to(wrong_device)):
        with pytest.raises(ValueError):
            ops.panoptic_fuse(bad, low, *G88, NTHINGS, NC)
    cap = ops.PANOPTIC_MAX_QUERIES
    assert cap >= 1024
    many = class_rows([0] * (cap + 1), [4.0] * (cap + 1)).to(dev)
    with pytest.raises(RuntimeError, match='rsp_panoptic_fuse'):
        ops.panoptic_fuse(many, torch.zeros(cap + 1, 1, 1, device=dev), *G11, NTHINGS, NC)
    for geo in (((32, 32), (33, 32), (32, 32)), ((32, 32), (32, 32), (0, 32)), ((32, 32), (0, 32), (32, 32))):
        with pytest.raises(RuntimeError, match='rsp_panoptic_fuse'):
            ops.panoptic_fuse(cls, low, *geo, NTHINGS, NC)
    with pytest.raises(RuntimeError, match='rsp_panoptic_fuse'):
        ops.panoptic_fuse(cls, low, *G88, NC + 1, NC)
    sem, _ = ops.panoptic_fuse(many[:cap].contiguous(), torch.zeros(cap, 1, 1, device=dev), *G11, NTHINGS, NC, iou_thr=0.0)
    assert bool((sem == 1000).all())                                      # the cap itself runs; one query wins all 16 pixels: thing 1


# ----------------------------------------------------------------------------------------------------------- tolerance tier
TOL_MARGINS = (6.0, 5.2, 4.6, 4.2, 3.8, 3.5, 3.2, 3.0)      # the query with the lowest field offset has the highest score
TOL_LABELS = (0, 2, 1, 0, 2, 1, 0, 1)
# per case of mf.TOL_CASES: the first seed of 0, 1, 2, ... at which the reference meets tol_reference's three conditions,
# with its count of near pixels (found by evaluating the reference alone)
TOL_SEEDS = {'64x48-200x150-190x150-95x77': (0, 4), '128x128-512x512-512x512-300x400': (0, 89),
             '128x96-512x384-341x384-300x338': (0, 106), '48x64-100x130-100x129-100x129': (0, 5),
             '256x256-1024x1024-1000x900-333x301': (0, 85), '96x96-64x64-64x64-200x200': (0, 28)}


def near_pixel_cap(case):
    return max(8, math.ceil(1.5e-3 * mf.pixels(case)))


def tol_inputs(case, seed):
    cls = class_rows(TOL_LABELS, TOL_MARGINS, seed=1)
    score, label, keep = pr.select(cls, NC, 0.8)
    assert bool(keep.all()) and float(score.min()) >= 0.8 + 1e-3
    low = (mf.recipe_logits(8, case.hw, seed) + torch.linspace(-4.0, 4.0, 8)[:, None, None]).contiguous()
    return cls, low


def ratio_threshold(r):
    """the middle of the widest gap between the reference's ratios (queries with both areas > 0): both outcomes occur"""
    ratios = sorted(m / o for m, o in zip(r['mask_area'], r['original_area']) if m > 0 and o > 0)
    assert len(ratios) >= 2
    gaps = [(b - a, (a + b) / 2) for a, b in zip(ratios, ratios[1:])]
    return max(gaps)[1]


def tol_reference(case, seed):
    """(cls, low, reference, near bool [oh, ow], iou_thr) or an AssertionError that names the condition the seed misses"""
    cls, low = tol_inputs(case, seed)
    iou = ratio_threshold(pr.reference(cls, low, geo_of(case), NTHINGS, NC))
    r = pr.reference(cls, low, geo_of(case), NTHINGS, NC, iou_thr=iou)
    near = r['gap'] <= r['pair_scores'] * mf.VALUE_TOL / 4 + 1e-6
    n = int(near.sum())
    assert n <= near_pixel_cap(case), ('near pixels', n, near_pixel_cap(case))
    assert max(r['near_zero']) <= mf.near_cap(case), ('pixels within NEAR of 0', r['near_zero'], mf.near_cap(case))
    outcomes = set()
    for k, q in enumerate(r['kept']):                      # the slacks cannot change a decision
        m, o, z = r['mask_area'][q], r['original_area'][q], r['near_zero'][k]
        assert o - z > 0, ('original_area could become 0', q, o, z)
        always = m - n > 0 and (m - n) / (o + z) >= iou    # painted whatever the near pixels do
        never = (m + n) / (o - z) < iou                    # rejected whatever they do (a query that wins nothing included)
        assert always or never, ('the ratio of query', q, 'is within its slack of iou_thr', m, o, n, z, iou)
        outcomes.add(always)
    assert outcomes == {True, False}
    return cls, low, r, near, iou


def check_tolerance(ops, dev, case, report=print):
    seed, committed = TOL_SEEDS[mf.case_id(case)]
    cls, low, r, near, iou = tol_reference(case, seed)
    n = int(near.sum())
    assert n == committed, ('the committed near count', committed, 'is not the reference\'s', n)
    sem, info = run(ops, dev, cls, low, geo_of(case), iou_thr=iou)
    assert info['segment'] == r['segment'], (case, info['segment'], r['segment'])
    bad = (sem != r['sem']) & ~near
    assert not bool(bad.any()), (case, int(bad.sum()), 'pixels differ away from the near ones')
    dm = [abs(a - b) for a, b in zip(info['mask_area'], r['mask_area'])]
    do = [abs(info['original_area'][q] - r['original_area'][q]) for q in r['kept']]
    report(f'panoptic {mf.case_id(case)}: {n} near pixels (cap {near_pixel_cap(case)}), {int((sem != r["sem"]).sum())} map pixels off the '
           f'fp64 ones, mask_area off by at most {max(dm)}, original_area by at most {max(do)} (|v| < 1e-4: {max(r["near_zero"])}), '
           f'iou_thr {iou:.4f}')
    assert max(dm) <= n, (case, dm, n)
    assert all(d <= z for d, z in zip(do, r['near_zero'])), (case, do, r['near_zero'])
    assert max(abs(a - float(b)) for a, b in zip(info['score'], r['score'])) <= 1e-6
