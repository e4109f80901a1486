"""Bodies of the mask-field tests (csrc/mask_field.h), shared by both kernel tiers in the style of tests/_kernel_props.py.

The six entry points that evaluate the resize -> crop -> resize chain over low-resolution logits (rsp_mask_post,
rsp_mask_post_logits, rsp_query_mask_post, rsp_mask_score_box, rsp_mask_score_box_crops, rsp_persam_locate) are compared with
ONE oracle, `field_f64`: the chain in fp64 with F.interpolate on the CPU.  Nothing here goes through another kernel,
`torch_ops_mock` or `ops` to get a reference; the one derived quantity, the near-edge flag of rsp_mask_score_box_crops in the
tolerance tier, is HF's _is_box_near_crop_edge of the box in the same output row, which is itself held to the fp64 field.

Exact tier.  A geometry is DYADIC when h / Hb and w / Wb are in {1/4, 1/2, 1, 2}, the crop is a top-left rectangle and the
output is the crop, half the crop or twice the crop.  Every interpolation coefficient is then a multiple of 1/8, so with
integer logits in [-8, 8] every intermediate value is a multiple of 2^-10 below 2^4: every fp32 operation is exact in any
evaluation order, contracted or not, and the fp64 chain is the kernel's answer bit for bit.  Thresholds drawn from the
attained values tie with real pixels, which pins `>` against `>=`.  Per case the module asserts, on the reference alone, that
the torch fp32 chain equals `field_f64` bit for bit (a case outside the rule fails as a bad case, not as a kernel bug) and that
`mask_form` of the geometry is the form the case is labelled with (every form x quad / pixel path is provably visited).

Tolerance tier.  Non-dyadic geometries on the project's logit recipe (tests/test_gpu_samdet.py:102) with its 1e-4 value bound;
a bit, count or box edge may differ from the fp64 one only where a pixel of `field_f64` is within 1e-4 of the threshold (the
rule of check_score_kernel, tests/test_gpu_sam_prompts.py).  Each case has a seed of its own, found on the reference alone,
at which no field has more than max(2, 1e-4 oh ow) such pixels at any threshold the test uses; the test asserts that.

tests/test_gpu_mask_field.py runs these on cuda:0, tests/test_mask_field_cpu.py on the lane-level emulator, and
tests/test_kernel_props_selfcheck_cpu.py shows that check_exact_field rejects ten mutations of a fake `ops`.  This module
imports no hypothesis."""
import collections
import math

import torch
import torch.nn.functional as F

Case = collections.namedtuple('Case', 'hw img crop out form')

MP_ROWS, MS_ROWS = 16, 64                   # rows per strip item of the post-process / locate and of the score kernels (csrc/samdec.hip)
VALUE_TOL = 1e-4                            # the project's bound for the recipe below (tests/test_gpu_samdet.py:107)
NEAR = 1e-4                                 # a pixel this close to a threshold may fall on either side


def _c(hw, img, crop, out, form):
    return Case(tuple(hw), tuple(img), tuple(crop), tuple(out), form)


# (h, w) / (Hb, Wb) / crop / out, and the form mask_form() must choose
EXACT_CASES = (
    _c((16, 12), (64, 48), (64, 48), (64, 48), 'strip'),        # oh == MS_ROWS: one full score tile
    _c((16, 12), (64, 48), (61, 47), (61, 47), 'ident'),        # ow % 4 == 3
    _c((16, 12), (64, 48), (64, 48), (32, 24), 'generic'),      # stage-2 down-sampling, quads
    _c((16, 12), (64, 48), (60, 44), (30, 22), 'generic'),      # ow % 4 == 2: per pixel
    _c((16, 12), (64, 48), (32, 24), (64, 48), 'generic'),      # stage-2 up-sampling, quads
    _c((64, 48), (32, 24), (32, 24), (32, 24), 'strip'),        # stage-1 down-sampling; 16 < oh < 64
    _c((64, 64), (256, 256), (200, 136), (100, 68), 'generic'),
    _c((1, 1), (4, 4), (4, 4), (4, 4), 'strip'),                # 1 x 1 logits: one quad column, four rows
    _c((7, 5), (28, 20), (27, 19), (27, 19), 'ident'),          # odd logits, ow % 4 == 3
    _c((32, 32), (128, 128), (100, 128), (100, 128), 'strip'),  # base 128; 7 x 32 = 224 items of 16 rows, 2 x 32 of 64
    _c((32, 32), (128, 128), (128, 126), (64, 63), 'generic'),  # ow % 4 == 3
    _c((8, 8), (32, 32), (1, 1), (1, 1), 'ident'),              # a 1 x 1 crop
    _c((8, 8), (32, 32), (31, 1), (31, 1), 'ident'),            # a crop one pixel wide
    # beyond the issue's list, within the dyadic rule
    _c((8, 8), (32, 32), (9, 4), (9, 4), 'strip'),              # oh < 16: one quad column, nine rows
    _c((8, 8), (32, 32), (1, 32), (1, 32), 'strip'),            # a crop one pixel high
    _c((16, 12), (64, 48), (37, 20), (37, 20), 'strip'),        # 16 < oh < 64, no multiple of 16
    _c((64, 64), (256, 256), (200, 136), (200, 136), 'strip'),  # 13 x 34 = 442 items of 16 rows: two blocks, the last ragged
    _c((7, 5), (28, 20), (26, 18), (26, 18), 'ident'),          # ow % 4 == 2
    _c((7, 5), (28, 20), (27, 17), (27, 17), 'ident'),          # ow % 4 == 1
    _c((7, 5), (28, 20), (28, 20), (14, 10), 'generic'),        # ow % 4 == 2
    _c((16, 8), (32, 32), (32, 32), (32, 32), 'strip'),         # h / Hb = 1/2 and w / Wb = 1/4
    _c((24, 20), (24, 20), (24, 20), (12, 10), 'generic'),      # stage 1 is the identity
    _c((64, 48), (32, 24), (32, 24), (64, 48), 'generic'),      # down-sampling, then up-sampling
    _c((64, 48), (32, 24), (31, 23), (31, 23), 'ident'),        # stage-1 down-sampling, per pixel
    _c((12, 16), (48, 64), (40, 30), (80, 60), 'generic'),      # stage-2 up-sampling of a true crop
)

# non-dyadic geometries; TOL_SEEDS below holds, per case, a seed at which the recipe's fields satisfy check_field_tolerance's
# condition on the reference
TOL_CASES = (
    _c((64, 48), (200, 150), (190, 150), (95, 77), 'generic'),
    _c((128, 128), (512, 512), (512, 512), (300, 400), 'generic'),
    _c((128, 96), (512, 384), (341, 384), (300, 338), 'generic'),
    _c((48, 64), (100, 130), (100, 129), (100, 129), 'ident'),      # identity, odd width, non-dyadic stage 1
    _c((256, 256), (1024, 1024), (1000, 900), (333, 301), 'generic'),
    _c((96, 96), (64, 64), (64, 64), (200, 200), 'generic'),        # down-sampling, then up-sampling
)
# found by evaluating field_f64 alone at seeds 0, 1, 2, ...: the largest count of pixels within NEAR of logit 0, of the score
# thresholds 1.5 / -0.5 / 0.5 and of probability 0.5 over the three fields is 0, 10, 6, 1, 8 and 2 against caps of 2, 12, 10,
# 2, 10 and 4
TOL_SEEDS = dict(zip(TOL_CASES, (1, 54, 17, 5, 39, 33)))
DET_K64_SEED = 11
DET_K64_CASE = _c((256, 256), (1024, 1024), (1024, 1024), (512, 512), 'generic')     # query_mask_post at its block cap of 64
CHUNK_CASE = _c((1, 1), (4, 4), (4, 4), (4, 4), 'strip')
CHUNK_K = 65537                                                  # grid.y holds 65535: a second chunk of two masks


def pixels(case):
    return case.out[0] * case.out[1]


def case_id(c):
    return '-'.join('x'.join(map(str, v)) for v in (c.hw, c.img, c.crop, c.out))


def mask_form(crop, out):
    """csrc/mask_field.h mask_form(), restated"""
    if tuple(crop) != tuple(out):
        return 'generic'
    return 'strip' if out[1] % 4 == 0 else 'ident'


# ------------------------------------------------------------------------------------------------------------------ the oracle
def _chain(low, img, crop, out):
    v = F.interpolate(low[:, None], size=tuple(img), mode='bilinear', align_corners=False)[..., :crop[0], :crop[1]]
    return F.interpolate(v, size=tuple(out), mode='bilinear', align_corners=False)[:, 0]


def field_f64(low, img, crop, out):
    """[k, h, w] -> fp64 [k, oh, ow]: bilinear to img, the top-left crop, bilinear to out (models.py:1746-1784), on the CPU"""
    return _chain(low.detach().cpu().double(), img, crop, out)


def lowest_index_of(v, value):
    """lowest flat index at which the 2-d field v equals value"""
    return int((v.flatten() == value).nonzero()[0, 0])


def _ulp32(x):
    """spacing of fp32 at |x|"""
    a = torch.tensor(abs(float(x)), dtype=torch.float32)
    return float(torch.nextafter(a, torch.tensor(math.inf)).double() - a.double())


def integer_logits(case, seed):
    """[3, h, w]: all -8, all +8, random integers in [-8, 8] with 0 in the corner -- 1 x 1 logits or a 1 x 1 crop of an
    up-sampling make one-valued fields, and 0 lets the thresholds sit between the three"""
    h, w = case.hw
    g = torch.Generator().manual_seed(seed)
    low = torch.empty(3, h, w)
    low[0], low[1] = -8.0, 8.0
    low[2] = torch.randint(-8, 9, (h, w), generator=g).float()
    low[2, 0, 0] = 0.0
    return low


def assert_case_is_exact(case, low):
    """the two preconditions on the reference alone; returns field_f64"""
    assert mask_form(case.crop, case.out) == case.form, ('mislabelled case', case)
    ref = field_f64(low, case.img, case.crop, case.out)
    f32 = _chain(low.float().cpu(), case.img, case.crop, case.out)
    assert f32.dtype == torch.float32 and torch.equal(f32.double(), ref), ('not a dyadic case: fp32 and fp64 chains differ', case)
    return ref


def tie_threshold(ref):
    """a value of the fields [k, oh, ow] that some pixel attains with pixels above and below it: the median attained value
    of the last (random) field when that has three levels, of all fields otherwise"""
    u = ref[-1].unique()
    if u.numel() < 3:
        u = ref.unique()
    assert u.numel() >= 3, 'fewer than three attained values'
    return float(u[u.numel() // 2])


def score_thresholds(ref):
    """(thr, off) with thr + off, thr - off and thr attained by the fields, thr as close to the median attained value as an
    arithmetic triple allows"""
    u = ref[-1].unique()
    if u.numel() < 3:
        u = ref.unique()
    vals = set(u.tolist())
    order = sorted(range(u.numel()), key=lambda i: abs(i - u.numel() // 2))
    for i in order:
        t = float(u[i])
        for hi in u[i + 1:].tolist():
            if 2 * t - hi in vals:
                return t, hi - t
    raise AssertionError('no attained arithmetic triple')


def _box_of(mask):
    """HF _batched_mask_to_box of one [oh, ow] mask as a list (inclusive maxima, zeros when empty), restated"""
    ys, xs = mask.any(1).nonzero()[:, 0], mask.any(0).nonzero()[:, 0]
    if ys.numel() == 0:
        return [0, 0, 0, 0]
    return [int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])]


def _hf():
    from transformers.models.sam import image_processing_pil_sam as ip
    return ip


def crop_rows(cases, hw):
    """table rows (rsp_mask_score_box_crops: Hb, Wb, crop_h, crop_w, out_h, out_w, x0, y0, x1, y1, W, H) of every case with
    logits (h, w): the crops lie on a diagonal of a 420 x 300 image, so boxes come near crop edges that are and are not image
    edges"""
    W, H = 420, 300
    group = [c for c in cases if c.hw == tuple(hw)]
    rows = []
    for i, c in enumerate(group):
        x0, y0 = min(37 * i, W - c.out[1]), min(23 * i, H - c.out[0])
        rows.append([*c.img, *c.crop, *c.out, x0, y0, x0 + c.out[1], y0 + c.out[0], W, H])
    return group, rows


# --------------------------------------------------------------------------------------------------------------- the exact tier
def check_exact_field(ops, dev, case, seed):
    """every entry point that takes one geometry, on integer logits (k = 3: all -8, all +8, random) of a dyadic geometry,
    against field_f64 with torch.equal.  rsp_mask_score_box_crops takes a table of geometries: check_exact_crops runs it once
    per (h, w) on all the cases that share those logits."""
    ip = _hf()
    from oracle.query import mask2bbox
    low = integer_logits(case, seed)
    ref = assert_case_is_exact(case, low)                                    # [3, oh, ow] fp64
    ref32 = ref.float()
    oh, ow = case.out
    geo = (case.img, case.crop, case.out)
    lowd = low.to(dev)

    # ---- mask_post_logits: values, and a threshold that pixels hit exactly (strict >: the tie is False)
    thr = tie_threshold(ref)
    tie, above, below = ref == thr, ref > thr, ref < thr
    assert bool(tie.any()) and bool(above.any()) and bool(below.any()), (case, thr)
    m, v = ops.mask_post_logits(lowd, *geo, thr, want_val=True)
    m, v = m.cpu(), v.cpu()
    assert m.dtype == torch.bool and v.dtype == torch.float32 and tuple(v.shape) == (3, oh, ow)
    assert torch.equal(v, ref32), ('mask_post_logits values', case, _first_diff(v, ref32))
    assert torch.equal(m, above), ('mask_post_logits mask at an attained threshold', case, thr, _first_diff(m, above))
    assert not bool(m[tie].any())
    assert torch.equal(ops.mask_post_logits(lowd, *geo, thr).cpu(), above), ('mask_post_logits without values', case)

    # ---- mask_post: sigmoid(0) = 0.5 exactly, and the test is >= (models.py:1779)
    zero = torch.zeros_like(lowd)
    half_up = float(torch.nextafter(torch.tensor(0.5), torch.tensor(1.0)))
    m, p = ops.mask_post(zero, *geo, 0.5, want_prob=True)
    assert torch.equal(p.cpu(), torch.full((3, oh, ow), 0.5)), ('mask_post probabilities of zero logits', case)
    assert torch.equal(m.cpu(), torch.ones(3, oh, ow, dtype=torch.bool)), ('mask_post: 0.5 >= 0.5', case)
    assert torch.equal(ops.mask_post(zero, *geo, half_up).cpu(), torch.zeros(3, oh, ow, dtype=torch.bool)), ('mask_post above 0.5', case)

    # ---- query_mask_post: the gather through qidx (a permutation with a repeat), masks (> 0), logits, boxes
    qidx = torch.tensor([2, 0, 1, 2], dtype=torch.int32)
    cls = torch.tensor([0.5, 0.25, 0.75, 1.0])
    qm, det, qb, ql = (t.cpu() for t in ops.query_mask_post(lowd, qidx.to(dev), cls.to(dev), *geo, want_logits=True))
    want = ref[qidx.long()]
    assert torch.equal(ql, want.float()), ('query_mask_post logits', case, _first_diff(ql, want.float()))
    assert torch.equal(qm, want > 0), ('query_mask_post masks', case, _first_diff(qm, want > 0))
    assert torch.equal(qb, mask2bbox(want > 0)), ('query_mask_post boxes', case, qb.tolist(), mask2bbox(want > 0).tolist())
    assert not bool((want[1] > 0).any()), 'the all -8 field is an empty mask'
    assert float(det[1]) == 0.0 and qb[1].tolist() == [0.0, 0.0, 0.0, 0.0]         # what the mock gives: 0 / (0 + 1e-6), zeros
    assert torch.equal(det > 0, (want > 0).flatten(1).any(1)), ('query_mask_post det_score sign', case, det.tolist())

    # ---- mask_score_box: the three thresholds are attained values
    t_mid, off = score_thresholds(ref)
    sc = ops.mask_score_box(lowd, *geo, t_mid, off).cpu()
    assert sc.dtype == torch.int32 and tuple(sc.shape) == (3, 7)
    want_sc = _score_rows(ip, ref, t_mid, off)
    assert torch.equal(sc, want_sc), ('mask_score_box', case, (t_mid, off), sc.tolist(), want_sc.tolist())
    assert want_sc[0].tolist() == [0] * 7, 'the all -8 field is an empty mask: box [0, 0, 0, 0]'

    # ---- persam_locate: extrema with the lowest flat index, mean to 1 ulp, std to 4 ulp, attn_sim to test_gpu_persam's bound
    gs = 4                      # a power of two: the g x g resampling's coefficients are exact too (the bound below has no term for them)
    stats, xy, attn = (t.cpu() for t in ops.persam_locate(lowd, *geo, gs))
    assert stats.dtype == torch.float32 and xy.dtype == torch.int32 and tuple(attn.shape) == (3, gs * gs)
    for i in range(3):
        f = ref[i]
        vmax, vmin = float(f.max()), float(f.min())
        imax, imin = lowest_index_of(f, vmax), lowest_index_of(f, vmin)
        assert torch.equal(stats[i, :2], torch.tensor([vmax, vmin])), ('persam_locate extrema', case, i, stats[i].tolist(), vmax, vmin)
        assert xy[i].tolist() == [imax % ow, imax // ow, imin % ow, imin // ow, oh * ow], ('persam_locate positions', case, i, xy[i].tolist(), imax, imin)
        mean = float(f.mean())
        std = float(f.std()) if oh * ow > 1 else 0.0
        assert abs(float(stats[i, 2]) - mean) <= _ulp32(mean), ('persam_locate mean', case, i, float(stats[i, 2]), mean)
        assert abs(float(stats[i, 3]) - std) <= 4 * _ulp32(std), ('persam_locate std', case, i, float(stats[i, 3]), std)
        if vmax == vmin:
            assert float(stats[i, 3]) == 0.0 and torch.equal(attn[i], torch.full((gs * gs,), 0.5)), ('a constant field', case, i)
            continue
        e_stat = 8 * 2.0 ** -24 * float(f.abs().max())                       # check_locate, tests/test_gpu_persam.py
        want_a = F.interpolate(((f - mean) / std)[None, None], size=(gs, gs), mode='bilinear', align_corners=False).sigmoid()
        tol = 0.25 * (2 * e_stat / std) + 1e-6
        e = float((attn[i].double() - want_a.flatten()).abs().max())
        assert e <= tol, ('persam_locate attn_sim', case, i, e, tol)


def _first_diff(a, b):
    d = (a != b).nonzero()
    if d.numel() == 0:
        return None
    i = tuple(d[0].tolist())
    return (int(d.shape[0]), i, a[i].item(), b[i].item())


def _score_rows(ip, ref, t_mid, off):
    """int32 [k, 7] of mask_score_box from the fp64 fields: counts above t_mid + off, t_mid - off, t_mid, HF's box"""
    k = ref.shape[0]
    out = torch.zeros(k, 7, dtype=torch.int32)
    for j, t in enumerate((t_mid + off, t_mid - off, t_mid)):
        out[:, j] = (ref > t).flatten(1).sum(1).int()
    out[:, 3:] = ip._batched_mask_to_box(ref > t_mid).int()
    return out


def crop_groups(cases=EXACT_CASES):
    """the (h, w) of the cases, each once, in order of appearance"""
    return tuple(dict.fromkeys(c.hw for c in cases))


def check_exact_crops(ops, dev, hw, seed, cases=EXACT_CASES):
    """rsp_mask_score_box_crops on one table of every case of `cases` with logits (h, w): three candidates per row,
    interleaved, so that one launch mixes strip, identity and generic blocks; counts, the shifted box and the near-edge flag
    against the fp64 fields and HF's _is_box_near_crop_edge"""
    ip = _hf()
    group, rows = crop_rows(cases, hw)
    C = len(group)
    lows = [integer_logits(c, seed + 1 + i) for i, c in enumerate(group)]
    refs = [assert_case_is_exact(c, lo) for c, lo in zip(group, lows)]
    # one pair of thresholds for the launch: attained by the first row's fields
    t_mid, off = score_thresholds(refs[0])
    low = torch.stack(lows, 1).flatten(0, 1).contiguous()                       # interleaved: candidate m = j * C + c is field j of crop c
    cidx = torch.arange(C, dtype=torch.int32).repeat(3)
    tab = torch.tensor(rows, dtype=torch.int32)
    got = ops.mask_score_box_crops(low.to(dev), cidx.to(dev), tab.to(dev), (max(r[4] for r in rows), max(r[5] for r in rows)),
                                   t_mid, off).cpu()
    assert got.dtype == torch.int32 and tuple(got.shape) == (3 * C, 8)
    for c, (case, r, ref) in enumerate(zip(group, rows, refs)):
        sel = torch.arange(3) * C + c
        want = _score_rows(ip, ref, t_mid, off)
        assert torch.equal(got[sel, :3], want[:, :3]), ('mask_score_box_crops counts', case, got[sel].tolist(), want.tolist())
        shift = torch.tensor([[r[6], r[7], r[6], r[7]]], dtype=torch.int32)
        assert torch.equal(got[sel, 3:7], want[:, 3:] + shift), ('mask_score_box_crops box', case, got[sel].tolist(), want.tolist())
        near = ip._is_box_near_crop_edge(want[:, 3:].long(), r[6:10], [0, 0, r[10], r[11]])
        assert torch.equal(got[sel, 7].bool(), near) and set(got[sel, 7].tolist()) <= {0, 1}, ('near-edge flag', case, got[sel].tolist())


# ----------------------------------------------------------------------------------------------------------- the tolerance tier
def recipe_logits(k, hw, seed):
    """the project's recipe (tests/test_gpu_samdet.py:102): avg_pool2d(randn, 9, 1, 4) * 20"""
    g = torch.Generator().manual_seed(seed)
    return (F.avg_pool2d(torch.randn(k, 1, hw[0], hw[1], generator=g), 9, 1, 4)[:, 0] * 20).contiguous()


def near_cap(case):
    return max(2, int(NEAR * pixels(case)))


def query_pixels_per_thread(k, out):
    """P of rsp_query_mask_post's grid rule: ceil(items / 256) blocks per mask, at most 64 (k >= 64), 256 (k >= 8) or 1024;
    an item is a quad of 4 pixels when ow % 4 == 0, a pixel otherwise; grid-stride"""
    per = 4 if out[1] % 4 == 0 else 1
    items = out[0] * out[1] // per
    gx = min((items + 255) // 256, 64 if k >= 64 else (256 if k >= 8 else 1024))
    return -(-items // (gx * 256)) * per


def _assert_bits(got, ref, t, cap, what):
    """a mask differs from ref > t (>= t: ge) only where ref is within NEAR of t; returns the near count per mask"""
    near = (ref - t).abs() < NEAR
    n = near.flatten(1).sum(1)
    assert int(n.max()) <= cap, (what, 'the reference has', n.tolist(), 'pixels within 1e-4 of', t, '(cap', cap, '): another seed')
    bad = (got != (ref > t)) & ~near
    assert not bool(bad.any()), (what, int(bad.sum()), 'bits differ away from the threshold')
    return n


def _assert_box_between(b, v, t, what):
    """the rule of check_score_kernel: the box lies between those of the masks v > t + NEAR and v > t - NEAR"""
    lo, hi = _box_of(v > t + NEAR), _box_of(v > t - NEAR)
    if not bool((v > t - NEAR).any()):
        assert b == [0, 0, 0, 0], (what, b)
    elif not bool((v > t + NEAR).any()):
        assert b == [0, 0, 0, 0] or (b[0] >= hi[0] and b[1] >= hi[1] and b[2] <= hi[2] and b[3] <= hi[3]), (what, b, hi)
    else:
        assert hi[0] <= b[0] <= lo[0] and hi[1] <= b[1] <= lo[1] and lo[2] <= b[2] <= hi[2] and lo[3] <= b[3] <= hi[3], (what, b, lo, hi)


def _assert_score_row(row, f, t3, cap, what):
    """counts above t3 = (t_hi, t_lo, t_mid) and the box at t_mid of one output row (a list of 7) against one fp64 field f:
    a count is off by at most the number of pixels within NEAR of its threshold, of which the reference has at most cap;
    returns those numbers"""
    ns = []
    for j, t in enumerate(t3):
        want, n = int((f > t).sum()), int(((f - t).abs() < NEAR).sum())
        assert n <= cap, (what, 'the reference has', n, 'pixels within 1e-4 of', t, '(cap', cap, '): another seed')
        assert abs(row[j] - want) <= n, (what, 'count', j, row[j], want, n)
        ns.append(n)
    _assert_box_between(row[3:7], f, t3[2], what)
    return ns


def check_field_tolerance(ops, dev, case, seed=None, report=print):
    """the six entry points on a non-dyadic geometry and the project's logit recipe (k = 3: the recipe's fields shifted by
    -4, +4 and 0, at the case's seed of TOL_SEEDS) against field_f64: values within VALUE_TOL, bits / counts / boxes exact away
    from pixels within NEAR of a threshold, of which the reference has at most near_cap(case) per mask and threshold.  Prints
    and returns the measured figures."""
    assert mask_form(case.crop, case.out) == case.form, ('mislabelled case', case)
    k = 3
    seed = TOL_SEEDS[case] if seed is None else seed
    low = recipe_logits(k, case.hw, seed)
    low[0] -= 4.0                                                             # three different foreground fractions
    low[1] += 4.0
    ref = field_f64(low, case.img, case.crop, case.out)
    oh, ow = case.out
    geo = (case.img, case.crop, case.out)
    lowd = low.to(dev)
    cap = near_cap(case)
    fig = {}

    # ---- mask_post_logits
    m, v = ops.mask_post_logits(lowd, *geo, 0.0, want_val=True)
    fig['logits_err'] = float((v.cpu().double() - ref).abs().max())
    report(f'mask field {case.hw} / {case.img} / {case.crop} / {case.out}: mask_post_logits max |value - fp64| = {fig["logits_err"]:.3e}')
    fig['near0'] = _assert_bits(m.cpu(), ref, 0.0, cap, ('mask_post_logits', case)).tolist()
    assert fig['logits_err'] <= VALUE_TOL, ('mask_post_logits values', case, fig['logits_err'])

    # ---- mask_post: the probability field
    pref = field_f64(torch.sigmoid(low.double()), case.img, case.crop, case.out)
    m, p = ops.mask_post(lowd, *geo, 0.5, want_prob=True)
    fig['prob_err'] = float((p.cpu().double() - pref).abs().max())
    report(f'    mask_post max |probability - fp64| = {fig["prob_err"]:.3e}')
    near = (pref - 0.5).abs() < NEAR
    fig['near_half'] = near.flatten(1).sum(1).tolist()
    assert max(fig['near_half']) <= cap, ('the reference has', fig['near_half'], 'pixels within 1e-4 of 0.5 (cap', cap, '): another seed')
    assert not bool(((m.cpu() != (pref >= 0.5)) & ~near).any()), ('mask_post bits', case)
    assert fig['prob_err'] <= VALUE_TOL, ('mask_post probabilities', case, fig['prob_err'])

    # ---- query_mask_post
    qidx = torch.tensor([2, 0, 1, 2], dtype=torch.int32)
    cls = torch.tensor([0.5, 0.25, 0.75, 1.0])
    fig.update(_check_query_tolerance(ops, dev, lowd, ref, qidx, cls, case, cap, report))

    # ---- mask_score_box, mask_score_box_crops (a table of this geometry at two places of an image): every row of both against
    # the fp64 field; the near-edge flag is HF's function of the (crop-local) box in the same row
    thr, off = 0.5, 1.0
    t3 = (thr + off, thr - off, thr)
    sc = ops.mask_score_box(lowd, *geo, thr, off).cpu()
    W, H = ow + 100, oh + 60
    rows = [[*case.img, *case.crop, *case.out, 0, 0, ow, oh, W, H], [*case.img, *case.crop, *case.out, 100, 60, W, H, W, H]]
    cidx = torch.tensor([0, 1, 0, 1, 0, 1], dtype=torch.int32)
    sc2 = ops.mask_score_box_crops(lowd.repeat_interleave(2, 0).contiguous(), cidx.to(dev), torch.tensor(rows, dtype=torch.int32).to(dev),
                                   case.out, thr, off).cpu()
    assert sc.dtype == torch.int32 and tuple(sc.shape) == (k, 7) and sc2.dtype == torch.int32 and tuple(sc2.shape) == (2 * k, 8)
    fig['near_score'] = []
    for i in range(k):
        fig['near_score'] += _assert_score_row(sc[i].tolist(), ref[i], t3, cap, ('mask_score_box', case, i))
        for c in range(2):
            s = sc2[2 * i + c]
            local = s[3:7] - torch.tensor([rows[c][6], rows[c][7]] * 2, dtype=torch.int32)
            _assert_score_row(s[:3].tolist() + local.tolist(), ref[i], t3, cap, ('mask_score_box_crops', case, i, c))
            flag = _hf()._is_box_near_crop_edge(local[None].long(), rows[c][6:10], [0, 0, W, H])
            assert s[7].item() in (0, 1) and bool(s[7]) == bool(flag[0]), ('near-edge flag', case, i, c, s.tolist())

    # ---- persam_locate
    gs = 8
    stats, xy, attn = (t.cpu() for t in ops.persam_locate(lowd, *geo, gs))
    worst = 0.0
    for i in range(k):
        f = ref[i]
        vmax, vmin, mean, std = float(f.max()), float(f.min()), float(f.mean()), float(f.std())
        assert abs(float(stats[i, 0]) - vmax) <= VALUE_TOL and abs(float(stats[i, 1]) - vmin) <= VALUE_TOL, ('persam_locate extrema', case, i)
        assert abs(float(stats[i, 2]) - mean) <= VALUE_TOL and abs(float(stats[i, 3]) - std) <= VALUE_TOL, ('persam_locate mean / std', case, i)
        x0, y0, x1, y1, n = xy[i].tolist()
        assert n == oh * ow and 0 <= x0 < ow and 0 <= y0 < oh and 0 <= x1 < ow and 0 <= y1 < oh
        # the positions are those of pixels within twice the value bound of the fp64 extremes
        assert float(f[y0, x0]) >= vmax - 2 * VALUE_TOL and float(f[y1, x1]) <= vmin + 2 * VALUE_TOL, ('persam_locate positions', case, i)
        # check_locate's bound (tests/test_gpu_persam.py) with the field's value bound next to e_stat
        e_stat = 8 * 2.0 ** -24 * float(f.abs().max()) + VALUE_TOL
        want_a = F.interpolate(((f - mean) / std)[None, None], size=(gs, gs), mode='bilinear', align_corners=False).sigmoid()
        tol = 0.25 * (2 * e_stat / std) + 1e-6
        e = float((attn[i].double() - want_a.flatten()).abs().max())
        worst = max(worst, e / tol)
        assert e <= tol, ('persam_locate attn_sim', case, i, e, tol)
    fig['attn_of_bound'] = worst
    report(f'    within 1e-4 of the threshold: {fig["near0"]} (logit 0), {fig["near_half"]} (probability 0.5), at most '
           f'{max(fig["near_score"])} at a score threshold (cap {cap}); det_score rel. error {fig["det_err"]:.2e} at P = {fig["P"]}, '
           f'{fig["det_flips"]} mask bits off the fp64 ones; '
           f'attn_sim at {worst:.2f} of its bound')
    return fig


DET_TOL = 1e-5          # (P + 4) 2^-24 at P ~ 160 pixels per thread: fp32 sums per thread, fp64 beyond
DET_P_MAX = 160


def _check_query_tolerance(ops, dev, lowd, ref, qidx, cls, case, cap, report):
    """masks, logits, boxes of query_mask_post under the near rule, det_score against the mock's formula on the fp64 field:
    cls * sum(sigmoid(v) [v > 0]) / (count + 1e-6), to DET_TOL.  Where the kernel's mask is the fp64 one that bound stands
    alone.  A bit that the near rule lets differ moves the mask average by at most 1 / count of its value (the pixel's sigmoid
    is 0.5 and the average lies in [0.5, 1]); that much is added per bit that DOES differ, and for no other."""
    k = int(qidx.numel())
    P = query_pixels_per_thread(k, case.out)
    assert P < DET_P_MAX, (case, k, P)
    qm, det, qb, ql = (t.cpu() for t in ops.query_mask_post(lowd, qidx.to(dev), cls.to(dev), case.img, case.crop, case.out,
                                                            want_logits=True))
    want = ref[qidx.long()]
    err = float((ql.double() - want).abs().max())
    assert err <= VALUE_TOL, ('query_mask_post logits', case, err)
    _assert_bits(qm, want, 0.0, cap, ('query_mask_post', case))
    worst, flips = 0.0, 0
    for i in range(k):
        f = want[i]
        b = qb[i].tolist()
        assert all(float(x).is_integer() for x in b)
        if b == [0.0] * 4:                                                       # mask2bbox of an empty mask
            assert not bool((f > NEAR).any()), ('query_mask_post: zero box of a non-empty mask', case, i)
        else:
            _assert_box_between([int(b[0]), int(b[1]), int(b[2]) - 1, int(b[3]) - 1], f, 0.0, ('query_mask_post box', case, i))
        pos = f > 0
        cnt = int(pos.sum())
        ms = float((f.sigmoid() * pos).sum() / (cnt + 1e-6))
        d_ref = float(cls[i]) * ms
        if cnt == 0:
            continue
        rel = abs(float(det[i]) - d_ref) / d_ref
        flipped = int((qm[i] != pos).sum())
        flips += flipped
        bound = DET_TOL + flipped / cnt
        worst = max(worst, rel)
        assert rel <= bound, ('query_mask_post det_score', case, i, float(det[i]), d_ref, rel, bound, flipped)
    return dict(query_err=err, det_err=worst, det_flips=flips, P=P)


def check_det_score_at_block_cap(ops, dev, seed=DET_K64_SEED, report=print):
    """k = 64 masks of 512 x 512: query_mask_post's grid is capped at 64 blocks per mask, P = 16 pixels per thread.  The fp64
    reference is computed in chunks of 8 masks."""
    case, k = DET_K64_CASE, 64
    P = query_pixels_per_thread(k, case.out)
    assert P == 16 and P < DET_P_MAX
    low = recipe_logits(k, case.hw, seed)
    low += torch.linspace(-6.0, 6.0, k)[:, None, None]
    g = torch.Generator().manual_seed(seed + 1)
    qidx = torch.randperm(k, generator=g).to(torch.int32)
    qidx[-1] = qidx[0]
    cls = torch.rand(k, generator=g) + 0.1
    qm, det, qb = ops.query_mask_post(low.to(dev), qidx.to(dev), cls.to(dev), case.img, case.crop, case.out)
    qm, det, qb = qm.cpu(), det.cpu(), qb.cpu()
    cap, worst, nears, flips = near_cap(case), 0.0, [], 0
    for c0 in range(0, k, 8):
        ref = field_f64(low[qidx[c0:c0 + 8].long()], case.img, case.crop, case.out)
        n = _assert_bits(qm[c0:c0 + 8], ref, 0.0, cap, ('query_mask_post k = 64', c0))
        nears += n.tolist()
        for i in range(ref.shape[0]):
            f = ref[i]
            pos = f > 0
            cnt = int(pos.sum())
            assert cnt > 0
            d_ref = float(cls[c0 + i]) * float((f.sigmoid() * pos).sum() / (cnt + 1e-6))
            rel = abs(float(det[c0 + i]) - d_ref) / d_ref
            worst = max(worst, rel)
            flipped = int((qm[c0 + i] != pos).sum())                         # the bound grows only by bits that do differ
            flips += flipped
            assert rel <= DET_TOL + flipped / cnt, ('det_score', c0 + i, float(det[c0 + i]), d_ref, rel, flipped)
            _assert_box_between([int(qb[c0 + i, 0]), int(qb[c0 + i, 1]), int(qb[c0 + i, 2]) - 1, int(qb[c0 + i, 3]) - 1], f, 0.0,
                                ('box', c0 + i))
    report(f'mask field {case.hw} / {case.img} / {case.crop} / {case.out}, k = 64: query_mask_post det_score rel. error {worst:.2e} '
           f'at P = {P}, {flips} mask bits off the fp64 ones; at most {max(nears)} pixels within 1e-4 of 0 per mask (cap {cap})')
    return worst


# ---------------------------------------------------------------------------------------------------- more masks than grid.y
def check_more_masks_than_grid_rows(ops, dev):
    """k = 65537 masks of the 1 x 1 -> 4 x 4 geometry (1 MB of output) through the three entry points that write masks: more
    than the 65535 rows a grid's y dimension holds, so the launch has to be chunked.  The last two masks differ from the
    rest, and every mask is compared with the fp64 field (for 1 x 1 logits: the logit itself)."""
    case, k = CHUNK_CASE, CHUNK_K
    low = torch.ones(k, 1, 1)
    low[-2], low[-1] = -3.0, 0.0
    ref = field_f64(low, case.img, case.crop, case.out)
    assert tuple(ref.shape) == (k, 4, 4) and torch.equal(ref, low.double().expand(k, 4, 4))
    lowd = low.to(dev)
    geo = (case.img, case.crop, case.out)
    m, v = ops.mask_post_logits(lowd, *geo, 0.0, want_val=True)
    assert torch.equal(v.cpu().double(), ref) and torch.equal(m.cpu(), ref > 0)
    pref = field_f64(torch.sigmoid(low.double()), *geo)
    assert torch.equal(ops.mask_post(lowd, *geo, 0.5).cpu(), pref >= 0.5)              # sigmoid(0) = 0.5: True
    qidx = torch.arange(k - 1, -1, -1, dtype=torch.int32)                              # reversed: the two odd masks come first
    qm, det, qb, ql = (t.cpu() for t in ops.query_mask_post(lowd, qidx.to(dev), torch.ones(k).to(dev), *geo, want_logits=True))
    want = ref[qidx.long()]
    assert torch.equal(ql.double(), want) and torch.equal(qm, want > 0)
    box = torch.tensor([0.0, 0.0, 4.0, 4.0]).expand(k, 4).clone()
    box[:2] = 0.0
    assert torch.equal(qb, box)
    assert det[:2].tolist() == [0.0, 0.0] and bool((det[2:] == det[2]).all()) and abs(float(det[2]) - 1 / (1 + math.exp(-1))) < 1e-6


# --------------------------------------------------------------------------------------------------------- failure signatures
# tests/test_kernel_props_selfcheck_cpu.py runs check_exact_field on this stand-in for `ops` and asserts that every mutation
# is rejected (and that the unmutated stand-in passes).  Its bilinear resize is written out (index, weights, gather) so that
# the half-pixel offset can be dropped; without a mutation it reproduces F.interpolate in fp64.
MUTATIONS = ('ge_at_the_logits_threshold', 'gt_in_mask_post', 'no_half_pixel_in_stage_1', 'stage_2_skipped', 'stale_strip_rows',
             'last_quad_not_written', 'ragged_rows_not_written', 'highest_index_wins', 'qidx_ignored', 'box_max_off_by_one')


def _resize64(v, size, half_pixel=True):
    """torch upsample_bilinear2d(align_corners=False) of fp64 [k, H, W] to `size`, written out"""
    def coef(n_out, n_in):
        d = torch.arange(n_out, dtype=torch.float64)
        src = (n_in / n_out) * (d + 0.5) - 0.5 if half_pixel else (n_in / n_out) * d
        src = src.clamp(min=0.0)
        i0 = src.floor().long().clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
        l1 = src - i0
        return i0, i1, 1.0 - l1, l1
    y0, y1, ly0, ly1 = coef(size[0], v.shape[1])
    x0, x1, lx0, lx1 = coef(size[1], v.shape[2])
    rows = v[:, y0] * ly0[None, :, None] + v[:, y1] * ly1[None, :, None]
    return rows[:, :, x0] * lx0 + rows[:, :, x1] * lx1


class FakeOps:
    """the six wrappers of rsprompter_amd.ops computed from the fp64 field on the CPU, with at most one mutation"""

    def __init__(self, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.mut = mutation

    def _field(self, low, img, crop, out):
        """(field fp64 [k, oh, ow], the pixels a traversal visits bool [oh, ow])"""
        (ch, cw), (oh, ow) = crop, out
        form = mask_form(crop, out)
        f = _resize64(low.double(), img, self.mut != 'no_half_pixel_in_stage_1')[:, :ch, :cw]
        if form == 'generic':
            if self.mut == 'stage_2_skipped':
                f = f[:, torch.arange(oh).clamp(max=ch - 1)][:, :, torch.arange(ow).clamp(max=cw - 1)]
            else:
                f = _resize64(f, out)
        if self.mut == 'stale_strip_rows' and form == 'strip':
            f = f[:, torch.arange(oh) // 4 * 4]                     # the cached source-row pair is kept until the next multiple of 4
        seen = torch.ones(oh, ow, dtype=torch.bool)
        if self.mut == 'last_quad_not_written' and ow % 4 == 0:
            seen[:, ow - 4:] = False
        if self.mut == 'ragged_rows_not_written' and form == 'strip':
            seen[oh // MP_ROWS * MP_ROWS:] = False
        return f, seen

    def mask_post_logits(self, low, img, crop, out, thr=0.0, want_val=False):
        f, seen = self._field(low, img, crop, out)
        m = ((f >= thr) if self.mut == 'ge_at_the_logits_threshold' else (f > thr)) & seen
        return (m, (f * seen).float()) if want_val else m

    def mask_post(self, low, img, crop, out, thr, want_prob=False):
        p, seen = self._field(torch.sigmoid(low.double()), img, crop, out)
        m = ((p > thr) if self.mut == 'gt_in_mask_post' else (p >= thr)) & seen
        return (m, (p * seen).float()) if want_prob else m

    def _box(self, mask):
        b = _hf()._batched_mask_to_box(mask).int()
        if self.mut == 'box_max_off_by_one':
            b[:, 2:] += mask.flatten(1).any(1).int()[:, None]
        return b

    def query_mask_post(self, low, qidx, cls, img, crop, out, want_logits=False):
        k = qidx.numel()
        idx = torch.arange(k) % low.shape[0] if self.mut == 'qidx_ignored' else qidx.long()
        f, seen = self._field(low[idx], img, crop, out)
        m = (f > 0) & seen
        ms = (f.sigmoid() * m).flatten(1).sum(1) / (m.flatten(1).sum(1) + 1e-6)
        box = self._box(m).float()
        box[:, 2:] += m.flatten(1).any(1).float()[:, None]          # mask2bbox: exclusive maxima, zeros when empty
        res = (m, (cls.double() * ms).float(), box)
        return res + ((f * seen).float(),) if want_logits else res

    def _score(self, f, seen, thr, off):
        out = torch.zeros(f.shape[0], 7, dtype=torch.int32)
        for j, t in enumerate((thr + off, thr - off, thr)):
            out[:, j] = ((f > t) & seen).flatten(1).sum(1).int()
        out[:, 3:] = self._box((f > thr) & seen)
        return out

    def mask_score_box(self, low, img, crop, out, mask_threshold=0.0, stability_score_offset=1.0):
        return self._score(*self._field(low, img, crop, out), mask_threshold, stability_score_offset)

    def mask_score_box_crops(self, low, crop_idx, table, max_out_hw, mask_threshold=0.0, stability_score_offset=1.0):
        res = torch.zeros(low.shape[0], 8, dtype=torch.int32)
        for m in range(low.shape[0]):
            r = table[int(crop_idx[m])].tolist()
            s = self._score(*self._field(low[m:m + 1], r[0:2], r[2:4], r[4:6]), mask_threshold, stability_score_offset)
            res[m, :3] = s[0, :3]
            res[m, 3:7] = s[0, 3:] + torch.tensor([r[6], r[7], r[6], r[7]], dtype=torch.int32)
            res[m, 7] = int(_hf()._is_box_near_crop_edge(s[:, 3:].long(), r[6:10], [0, 0, r[10], r[11]])[0])
        return res

    def persam_locate(self, low, img, crop, out, g):
        f, seen = self._field(low, img, crop, out)
        k, (oh, ow) = f.shape[0], out
        stats, xy = torch.zeros(k, 4), torch.zeros(k, 5, dtype=torch.int32)
        attn = torch.full((k, g * g), 0.5)
        flat_seen = seen.flatten().nonzero()[:, 0]
        for i in range(k):
            v = f[i].flatten()[flat_seen]
            xy[i, 4] = oh * ow
            if v.numel() == 0:
                continue
            pick = (lambda hit: int(flat_seen[hit.nonzero()[-1 if self.mut == 'highest_index_wins' else 0, 0]]))
            imax, imin = pick(v == v.max()), pick(v == v.min())
            mean, std = float(v.mean()), float(v.std()) if v.numel() > 1 else 0.0
            stats[i] = torch.tensor([float(v.max()), float(v.min()), mean, std])
            xy[i, :4] = torch.tensor([imax % ow, imax // ow, imin % ow, imin // ow], dtype=torch.int32)
            if std > 0:
                attn[i] = F.interpolate(((f[i] - mean) / std)[None, None], size=(g, g), mode='bilinear',
                                        align_corners=False).sigmoid().flatten().float()
        return stats, xy, attn
