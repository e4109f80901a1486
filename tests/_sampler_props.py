"""Bodies of the sampler tests, in the style of tests/_mask_field_props.py: the ten entry points that interpolate on a
coordinate convention of their own, each held to ONE fp64 restatement of that convention at the places where a rewrite goes
wrong -- a cell boundary, a cut, the last row, a level threshold, the first pixel outside a region, a value equal to a
threshold.

    rsp_roi_align                      mmcv RoIAlign aligned=True + SingleRoIExtractor's level map + the PE by linearity
    rsp_paste_masks                    grid_sample(bilinear, zeros, align_corners=False) of sigmoid(logit), skip-empty region
    rsp_resize_pad / rsp_slice_resize_pad / rsp_crops_resize_pad          cv2 INTER_LINEAR + pad + fused normalisation
    rsp_resize_bilinear_nhwc / rsp_query_attn_mask                        F.interpolate(align_corners=False), the mask rule
    rsp_msdeform_attn / rsp_msdeform_attn_ex                              grid_sample per level, softmax over levels x points

Every restatement takes a dtype and a mutation switch: dtype = float64 and no mutation is the ORACLE; dtype = float32 is the
"fp32 restatement" that measures what fp32 arithmetic costs (E32); with a mutation it is the stand-in of
tests/test_kernel_props_selfcheck_cpu.py.  The restatements are plain torch on the CPU (F.grid_sample / F.interpolate where
they state the convention, index arithmetic otherwise); nothing goes through `ops`, another kernel or torch_ops_mock.

Exact tier.  Integer features / logits in [-8, 8] (paste: logits in {-100, 0, 100}, i.e. probabilities 0, 1/2, 1; u8 images),
sample positions on a dyadic grid and power-of-two divisors: every fp32 operation of any correct evaluation order is exact,
so the fp64 oracle is the kernel's answer bit for bit.  Per case the body first asserts, on the reference alone, that the
fp32 restatement equals the fp64 one bit for bit (a case outside the rule fails as a bad case, not as a kernel bug).

Tolerance tier.  The real shapes' arithmetic.  Value outputs: err <= max(F, 2 E32) with E32 the distance of the fp32
restatement from the fp64 one on that case and F = 4 ulp (fp32) of the case's largest output (tests/_score_fields.py).  Bit and
byte outputs may differ from the fp64 ones only where the fp64 field is within NEAR of a decision value (the threshold; an
integer of p * 255 in the soft paste mode), and each case's seed was chosen, on the reference alone, so that at most
max(2, 1e-4 pixels) pixels of a mask are that close.

    NEAR_PASTE = 6e-6   measured: the fp32 restatement of the paste field is at most 2.78e-6 from the fp64 one over PASTE_TOL
                        (twice that is 5.6e-6)
    NEAR_QMASK = 5e-5   measured: the fp32 restatement of the resized mask logits is at most 2.02e-5 from the fp64 one over
                        QMASK_TOL (twice that is 4.05e-5; the 64 x 64 -> 50 x 70 case, the others stay below 1e-6)

Each tolerance body re-measures its case and asserts that twice the measured distance is below the constant.

tests/test_gpu_samplers.py runs these on the device, tests/test_samplers_cpu.py a subset on the lane-level emulator."""
import collections
import ctypes
import math

import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
NEAR_PASTE = 6e-6
NEAR_QMASK = 5e-5


def case_id(c):
    """a test id of a case tuple: its fields, without spaces and brackets"""
    return '-'.join(str(v) for v in c).replace(' ', '').replace('(', '').replace(')', '').replace(',', 'x')


def _first_diff(a, b):
    d = (a != b).nonzero()
    if d.numel() == 0:
        return None
    i = tuple(d[0].tolist())
    return (int(d.shape[0]), i, a[i].item(), b[i].item())


def _ulp32(x):
    a = torch.tensor(abs(float(x)), dtype=F32)
    return float(torch.nextafter(a, torch.tensor(math.inf)).double() - a.double())


def _ints(g, shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _to(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def assert_exact(got, ref, what):
    """a value output of the exact tier: fp32, and bit for bit the fp64 oracle"""
    got = got.cpu()
    assert got.dtype == F32 and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, tuple(got.shape), tuple(ref.shape))
    assert torch.equal(got.double(), ref), (what, _first_diff(got.double(), ref))


class Report:
    """value outputs of the tolerance tier: err <= max(F, 2 E32) per case; all cases are printed, then asserted"""
    prefix = 'sampler'

    def __init__(self, family, report=print):
        self.family, self.rows, self.bad, self.report = family, [], [], report

    def add(self, case, got, ref, r32):
        err = float((got.cpu().double() - ref).abs().max())
        e32 = float((r32.double() - ref).abs().max())
        floor = 4 * _ulp32(float(ref.abs().max()))
        bound = max(floor, 2.0 * e32)
        ok = err <= bound                                       # NaN fails
        self.report(f'{self.prefix} {self.family} {case}: err {err:.3e} E32 {e32:.3e} F {floor:.3e} bound {bound:.3e}{"" if ok else "  <-- FAIL"}')
        self.rows.append((case, err, e32, bound))
        if not ok:
            self.bad.append((case, err, e32, bound))

    def finish(self):
        assert not self.bad, (self.family, self.bad)
        return self.rows


# ================================================================================================================== RoIAlign
ROI_MUTATIONS = ('no_half_pixel_shift', 'inclusive_cut_at_H', 'inclusive_cut_at_minus_1', 'no_low_clamp', 'top_index_unclamped',
                 'fixed_2x2_grid', 'level_strict_at_power_of_two', 'pe_skipped')
ROI_TOL_MUTATIONS = ('level_epsilon_dropped',)                         # shows off the dyadic grid only: the tolerance tier holds it
ROI_GRIDS = (1, 2, 4, 8, 16)


def roi_level(roi4, n_levels, finest, mut=None):
    """SingleRoIExtractor.map_roi_levels of one roi (x1, y1, x2, y2; 0-dim tensors of the working dtype):
    floor(log2(sqrt(w h) / finest + 1e-6)) clamped to [0, L - 1]; a NaN scale (w h < 0) reads level 0, where such a roi has
    no sample anyway"""
    sc = torch.sqrt((roi4[2] - roi4[0]) * (roi4[3] - roi4[1]))
    if mut == 'level_strict_at_power_of_two':
        return sum(1 for k in range(1, n_levels) if bool(sc > finest * 2 ** k))
    lf = torch.floor(torch.log2(sc / finest + (0.0 if mut == 'level_epsilon_dropped' else 1e-6)))
    if bool(torch.isnan(lf)):
        return 0
    return int(lf.clamp(0, n_levels - 1))


def _roi_axis(start, size, P, n, g, dtype, mut, census=None):
    """one axis of the sampling grid of one roi -> (valid, low index, high index, low weight, high weight), each [P, g];
    the indices address a map padded by one zero line in front and two behind (what an unclamped index reads)"""
    binsz = size / P
    p = torch.arange(P, dtype=dtype)[:, None]
    i = torch.arange(g, dtype=dtype)[None, :]
    v = start + p * binsz + (i + 0.5) * binsz / g
    if census is not None:
        for name, at in (('-1', -1.0), ('0', 0.0), ('n-1', n - 1.0), ('n', float(n))):
            census[name] = census.get(name, 0) + int((v == at).sum())
        census['below'] = census.get('below', 0) + int((v < -1).sum())
        census['beyond'] = census.get('beyond', 0) + int((v > n).sum())
        census['inside'] = census.get('inside', 0) + int(((v > 0) & (v < n - 1)).sum())
    lo_cut = (v <= -1) if mut == 'inclusive_cut_at_minus_1' else (v < -1)
    hi_cut = (v >= n) if mut == 'inclusive_cut_at_H' else (v > n)
    valid = ~(lo_cut | hi_cut)
    if mut != 'no_low_clamp':
        v = v.clamp(min=0)
    v = torch.where(valid, v, torch.zeros_like(v))
    lo = v.trunc().long()                                          # (int)y
    if mut == 'top_index_unclamped':
        hi = lo + 1
    else:
        top = lo >= n - 1
        lo = torch.where(top, torch.full_like(lo, n - 1), lo)
        hi = torch.where(top, lo, lo + 1)
        v = torch.where(top, lo.to(dtype), v)
    l1 = v - lo.to(dtype)
    return valid.to(dtype), lo + 1, hi + 1, 1 - l1, l1


def roi_align_ref(feats, pes, rois, P, strides, finest=56, dtype=F64, mut=None, census=None, info=None):
    """feats: list of [B, H, W, C]; pes: list of [H, W, C] / None, or None; rois [K, 5] -> [K, P, P, C] in `dtype`.
    info (a list) receives (level, gh, gw) per roi; census (a dict) counts the samples that land on -1, 0, n - 1, n"""
    K, C, L = rois.shape[0], feats[0].shape[-1], len(feats)
    out = torch.zeros(K, P, P, C, dtype=dtype)
    r = rois.to(dtype)
    for k in range(K):
        b = int(rois[k, 0])
        lvl = roi_level(r[k, 1:], L, finest, mut)
        H, W = feats[lvl].shape[1:3]
        s = torch.tensor(1.0 / strides[lvl], dtype=F32).to(dtype)      # the descriptor holds 1 / stride as fp32
        shift = 0.0 if mut == 'no_half_pixel_shift' else 0.5
        x1, y1, x2, y2 = (r[k, 1 + j] * s - shift for j in range(4))
        rw, rh = x2 - x1, y2 - y1
        gh, gw = int(torch.ceil(rh / P)), int(torch.ceil(rw / P))
        if info is not None:
            info.append((lvl, gh, gw))
        count = max(gh * gw, 1)
        if mut == 'fixed_2x2_grid':
            gh, gw = (2 if gh > 0 else gh), (2 if gw > 0 else gw)
            count = max(gh * gw, 1)
        if gh <= 0 or gw <= 0:
            continue
        f = feats[lvl][b].to(dtype)
        if pes is not None and pes[lvl] is not None and mut != 'pe_skipped':
            f = f + pes[lvl].to(dtype)
        fp = F.pad(f, (0, 0, 1, 2, 1, 2))
        cy = None if census is None else census.setdefault('y', {})
        cx = None if census is None else census.setdefault('x', {})
        vy, yl, yh, hy, ly = _roi_axis(y1, rh, P, H, gh, dtype, mut, cy)
        vx, xl, xh, hx, lx = _roi_axis(x1, rw, P, W, gw, dtype, mut, cx)
        acc = torch.zeros(P, gh, P, gw, C, dtype=dtype)
        for yi, wy in ((yl, hy), (yh, ly)):
            for xi, wx in ((xl, hx), (xh, lx)):
                wgt = (wy * vy)[:, :, None, None] * (wx * vx)[None, None, :, :]
                acc += wgt[..., None] * fp[yi[:, :, None, None], xi[None, None, :, :]]
        out[k] = acc.sum((1, 3)) / count
    return out


RoiCase = collections.namedtuple('RoiCase', 'name P C strides maps pe shapes')
_MAPS4 = ((40, 36), (36, 34), (34, 32), (32, 34))                   # (H, W) per level: none square, all hold a 28-wide roi


def _below(s):
    return 28.0 - 7.0 / (4 * s)


def _above(s):
    return 12.25 + 1.75 / s


# shapes: (level, stride, rw, rh) in level coordinates; sqrt(rw rh) = 14 is sqrt(w h) = 56 2^level in the image
ROI_EXACT = (
    RoiCase('p7-c256', 7, 256, (4, 8, 16, 32), _MAPS4, (True, False, True, False),
            tuple((l, 4 << l, 14.0, 14.0) for l in range(4))                # exactly 56 2^l, 2 x 2 samples per bin
            + tuple((l, 4 << l, 28.0, _below(4 << l)) for l in range(3))    # 7/8 pixel below 56 2^(l+1): 4 x 4
            + tuple((l, 4 << l, 7.0, 28.0) for l in range(4))               # exactly 56 2^l, not square: 4 x 1
            + ((0, 4, 3.5, 1.75), (3, 32, 28.0, 28.0))),                    # far below level 0; 896 = 56 2^4: clamped to level 3
    RoiCase('p4-c260', 4, 260, (4, 8, 16, 32), _MAPS4, (False, True, False, True),
            tuple((l, 4 << l, 16.0, _above(4 << l)) for l in range(4))      # one pixel above 56 2^l: 4 x 4
            + tuple((l, 4 << l, 16.0, 12.25) for l in range(4))             # exactly 56 2^l, not square
            + tuple((l, 4 << l, 8.0, 32.0) for l in range(4))),             # 8 x 2
    RoiCase('p2-c8-s4', 2, 8, (4,), ((9, 13),), (True,),
            ((0, 4, 2.0, 2.0), (0, 4, 4.0, 2.0), (0, 4, 4.0, 4.0), (0, 4, 8.0, 4.0), (0, 4, 8.0, 8.0), (0, 4, 1.0, 0.5))),
    RoiCase('p2-c8-s32', 2, 8, (32,), ((12, 10),), (False,),
            ((0, 32, 2.0, 2.0), (0, 32, 8.0, 8.0), (0, 32, 4.0, 1.0))),
)
ROI_EXACT_BY_NAME = {c.name: c for c in ROI_EXACT}
# zero-area and inverted rois, in image coordinates
ROI_DEGENERATE = ((40.0, 40.0, 40.0, 80.0), (40.0, 40.0, 80.0, 40.0), (40.0, 40.0, 40.0, 40.0), (80.0, 40.0, 40.0, 90.0),
                  (80.0, 90.0, 40.0, 40.0))


def roi_exact_rois(case):
    """-> (rois [K, 5], the level each roi must map to or None).  Every shape is placed seven times on its map: first sample
    on -1 and on 0, last sample on n - 1, on n and 1/8 beyond n, inside, wholly outside -- x and y take different placements"""
    rois, want = [], []
    for lvl, s, rw, rh in case.shapes:
        H, W = case.maps[lvl]
        gw, gh = math.ceil(rw / case.P), math.ceil(rh / case.P)

        def places(size, g, n):
            first = size / case.P / g / 2
            last = size - first
            return (-1 - first, -first, n - 1 - last, n - last, n - last + 0.125, 2.25, -size - 4.0)
        xs, ys = places(rw, gw, W), places(rh, gh, H)
        for i in range(7):
            x1s, y1s = xs[i], ys[(i + 3) % 7]
            x1, y1 = (x1s + 0.5) * s, (y1s + 0.5) * s
            rois.append([float(len(rois) % 2), x1, y1, x1 + rw * s, y1 + rh * s])
            want.append(lvl)
    for d in ROI_DEGENERATE:
        rois.append([float(len(rois) % 2), *d])
        want.append(None)
    return torch.tensor(rois, dtype=F32), want


def roi_exact_inputs(case, seed):
    g = torch.Generator().manual_seed(seed)
    feats = [_ints(g, (2, h, w, case.C)) for h, w in case.maps]
    pes = [_ints(g, (h, w, case.C)) if on else None for (h, w), on in zip(case.maps, case.pe)]
    rois, want = roi_exact_rois(case)
    return feats, pes, rois, want


def assert_roi_case_is_exact(case, seed, census=None):
    """on the reference alone: levels as labelled, grids of 1 .. 16 samples, fp32 restatement == fp64 oracle; -> inputs, oracle"""
    feats, pes, rois, want = roi_exact_inputs(case, seed)
    info = []
    ref = roi_align_ref(feats, pes, rois, case.P, case.strides, dtype=F64, census=census, info=info)
    r32 = roi_align_ref(feats, pes, rois, case.P, case.strides, dtype=F32)
    assert r32.dtype == F32 and torch.equal(r32.double(), ref), \
        ('not an exact case: fp32 and fp64 differ', case.name, _first_diff(r32.double(), ref))
    for (lvl, gh, gw), w in zip(info, want):
        if w is not None:
            assert lvl == w and gh * gw in ROI_GRIDS, ('mislabelled roi', case.name, lvl, w, gh, gw)
        else:
            assert gh <= 0 or gw <= 0, ('a degenerate roi with samples', case.name, gh, gw)
    return feats, pes, rois, ref


def check_exact_roi_align(ops, dev, case, seed=7):
    feats, pes, rois, ref = assert_roi_case_is_exact(case, seed)
    got = ops.roi_align(_to(dev, *feats), _to(dev, *pes), rois.to(dev), case.P, list(case.strides))
    assert_exact(got, ref, ('roi_align', case.name))
    if any(case.pe):                                                   # PE by linearity: no PE at all is the sum without it
        ref0 = roi_align_ref(feats, None, rois, case.P, case.strides)
        assert not torch.equal(ref0, ref)
        assert_exact(ops.roi_align(_to(dev, *feats), None, rois.to(dev), case.P, list(case.strides)), ref0, ('roi_align, no PE', case.name))


RoiTol = collections.namedtuple('RoiTol', 'P C K seed')
ROI_TOL = (RoiTol(7, 256, 48, 1), RoiTol(14, 256, 24, 2), RoiTol(7, 260, 24, 3))


def roi_tol_inputs(case):
    g = torch.Generator().manual_seed(case.seed)
    sizes = [(64, 80), (32, 40), (16, 20), (8, 10)]                       # a 256 x 320 image
    feats = [torch.randn(2, h, w, case.C, generator=g) for h, w in sizes]
    pes = [torch.randn(h, w, case.C, generator=g) if i % 2 == 0 else None for i, (h, w) in enumerate(sizes)]
    K = case.K
    scale = 56.0 * 2 ** (torch.arange(K) % 4 + torch.rand(K, generator=g))      # every level in turn
    aspect = torch.exp(torch.rand(K, generator=g) * 1.4 - 0.7)
    w, h = scale * aspect, scale / aspect
    cx, cy = torch.rand(K, generator=g) * 380 - 30, torch.rand(K, generator=g) * 316 - 30     # some reach outside the image
    rois = torch.stack([(torch.arange(K) % 2).float(), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    # sqrt(w h) / 56 one fp32 ulp below 2 and below 4: the 1e-6 of the level rule lifts both onto the upper level
    eps = torch.tensor([[0.0, 0.0, 0.0, 112.0, 112.0 - 2.0 ** -17], [1.0, 0.0, 0.0, 224.0, 224.0 - 2.0 ** -16]])
    return feats, pes, torch.cat([rois, eps])


def check_roi_align_tolerance(ops, dev, report=print):
    rep = Report('roi_align', report)
    for case in ROI_TOL:
        feats, pes, rois = roi_tol_inputs(case)
        strides = [4, 8, 16, 32]
        i64, i32 = [], []
        ref = roi_align_ref(feats, pes, rois, case.P, strides, dtype=F64, info=i64)
        r32 = roi_align_ref(feats, pes, rois, case.P, strides, dtype=F32, info=i32)
        assert i64 == i32, ('a roi on a level or grid threshold: another seed', case)
        assert {l for l, _, _ in i64} == {0, 1, 2, 3} and [l for l, _, _ in i64[-2:]] == [1, 2]
        got = ops.roi_align(_to(dev, *feats), _to(dev, *pes), rois.to(dev), case.P, strides)
        rep.add(f'P={case.P} C={case.C} K={rois.shape[0]}', got, ref, r32)
    return rep.finish()


# ================================================================================================================ paste masks
PASTE_MUTATIONS = ('gt_for_ge', 'align_corners', 'border_padding', 'no_region_margin', 'label_ignored', 'inf_not_zeroed',
                   'round_not_truncate')


def paste_field(logits_nhwc, labels, boxes, img_hw, dtype=F64, mut=None):
    """-> (field [k, H, W] in `dtype`: the pasted probability inside the written region, 0 outside; region bool [k, H, W]).
    FCNMaskHead._do_paste_mask with skip_empty, one instance per chunk."""
    k, Hm, Wm, C = logits_nhwc.shape
    H, W = int(img_hw[0]), int(img_hw[1])
    field = torch.zeros(k, H, W, dtype=dtype)
    region = torch.zeros(k, H, W, dtype=torch.bool)
    bx = boxes.to(dtype)
    m = 0 if mut == 'no_region_margin' else 1
    for n in range(k):
        cls = int(labels[n]) if (labels is not None and C > 1 and mut != 'label_ignored') else 0
        prob = torch.sigmoid(logits_nhwc[n, :, :, cls].to(dtype))
        x0, y0, x1, y1 = bx[n]
        rx0, ry0 = max(int(torch.floor(x0)) - m, 0), max(int(torch.floor(y0)) - m, 0)
        rx1, ry1 = min(int(torch.ceil(x1)) + m, W), min(int(torch.ceil(y1)) + m, H)
        if rx1 <= rx0 or ry1 <= ry0:
            continue
        gx = (torch.arange(rx0, rx1, dtype=dtype) + 0.5 - x0) / (x1 - x0) * 2 - 1
        gy = (torch.arange(ry0, ry1, dtype=dtype) + 0.5 - y0) / (y1 - y0) * 2 - 1
        fill = 1e30 if mut == 'inf_not_zeroed' else 0.0                # (an infinite coordinate samples nothing)
        gx = torch.where(torch.isinf(gx), torch.full_like(gx, fill), gx)
        gy = torch.where(torch.isinf(gy), torch.full_like(gy, fill), gy)
        grid = torch.stack([gx[None, :].expand(gy.numel(), -1), gy[:, None].expand(-1, gx.numel())], -1)[None]
        v = F.grid_sample(prob[None, None], grid, mode='bilinear', padding_mode='border' if mut == 'border_padding' else 'zeros',
                          align_corners=(mut == 'align_corners'))[0, 0]
        field[n, ry0:ry1, rx0:rx1] = v
        region[n, ry0:ry1, rx0:rx1] = True
    return field, region


def paste_bytes(field, region, thr, mut=None):
    """the kernel's output from the field: bool (>= thr) or uint8 (p * 255 truncated), 0 outside the region"""
    if thr >= 0:
        return ((field > thr) if mut == 'gt_for_ge' else (field >= thr)) & region
    b = field * 255
    b = torch.floor(b + 0.5) if mut == 'round_not_truncate' else torch.floor(b)
    return (b * region).to(torch.uint8)


PasteCase = collections.namedtuple('PasteCase', 'img mask C')
PASTE_EXACT = (PasteCase((12, 16), (8, 8), 1), PasteCase((9, 13), (8, 8), 3), PasteCase((10, 11), (4, 16), 1),
               PasteCase((9, 11), (16, 4), 2), PasteCase((7, 5), (2, 2), 1))


def paste_exact_boxes(H, W):
    """sides are powers of two (or zero), origins multiples of 1/4: inside, touching and crossing every side, larger than the
    image, zero width / height, narrower than a pixel, wholly outside each side, not square"""
    return torch.tensor([
        [2.25, 1.5, 6.25, 5.5], [0.0, 0.0, 4.0, 4.0], [W - 4.0, H - 4.0, W, H], [-2.5, -1.25, 5.5, 6.75],
        [W - 3.25, H - 2.75, W + 4.75, H + 5.25], [-4.0, -4.0, 28.0, 28.0], [3.25, 2.0, 3.25, 6.0], [2.0, 3.25, 6.0, 3.25],
        [3.25, 2.0, 3.5, 6.0], [2.0, 3.75, 6.0, 4.0], [W + 3.0, 2.0, W + 7.0, 6.0], [-9.0, 2.0, -5.0, 6.0], [2.0, -9.0, 6.0, -5.0],
        [2.0, H + 1.0, 6.0, H + 5.0], [1.0, 2.0, 9.0, 4.0], [0.75, 0.25, 1.75, 4.25], [W - 1.0, H - 1.0, W, H],
    ], dtype=F32)


def paste_exact_inputs(case, seed):
    g = torch.Generator().manual_seed(seed)
    boxes = paste_exact_boxes(*case.img)
    k = boxes.shape[0]
    logits = (torch.randint(-1, 2, (k, *case.mask, case.C), generator=g) * 100).float()
    logits[0] = 100.0                                                    # a full mask: the region's margin is not 0
    labels = (torch.arange(k) % case.C).to(torch.int32) if case.C > 1 else None
    return logits, labels, boxes


def assert_paste_case_is_exact(case, seed):
    """-> (inputs, fp64 field, region, thresholds: 0.5, two more attained values that real pixels tie with, and the soft mode)"""
    logits, labels, boxes = paste_exact_inputs(case, seed)
    ref, region = paste_field(logits, labels, boxes, case.img, F64)
    r32, region32 = paste_field(logits, labels, boxes, case.img, F32)
    # sigmoid(-100) = 3.7e-44 in fp64 and 0 (or a denormal) in fp32: far below the rule's grid of 2^-17, the rest is bit-equal
    assert r32.dtype == F32 and torch.equal(region, region32) and float((r32.double() - ref).abs().max()) < 2.0 ** -100, \
        ('not an exact case: fp32 and fp64 differ', case)
    u = ref[region].unique()
    u = u[(u > 2.0 ** -20) & (u < 1)]
    assert u.numel() >= 2 and bool((u == 0.5).any()), ('the field does not attain 1/2 and another value', case)
    thrs = [0.5, float(u[0]), float(u[-1]), 1.0, 0.0, -1.0]
    for t in thrs:
        assert torch.equal(paste_bytes(r32, region32, t), paste_bytes(ref, region, t)), ('not an exact case at', t, case)
    assert (case.img[0] * case.img[1]) % 4 == 0 or boxes.shape[0] >= 2
    return (logits, labels, boxes), ref, region, thrs


def check_exact_paste(ops, dev, case, seed=11):
    (logits, labels, boxes), ref, region, thrs = assert_paste_case_is_exact(case, seed)
    ld, bd = logits.to(dev), boxes.to(dev)
    lab = None if labels is None else labels.to(dev)
    for t in thrs:
        want = paste_bytes(ref, region, t)
        got = ops.paste_masks(ld, lab, bd, case.img, t).cpu()
        assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (case, t, got.dtype)
        assert torch.equal(got, want), ('paste_masks', case, t, _first_diff(got, want))
    if case.C == 1:                                                     # labels are ignored when there is one channel
        lab1 = torch.full((boxes.shape[0],), 5, dtype=torch.int32).to(dev)
        assert torch.equal(ops.paste_masks(ld, lab1, bd, case.img, 0.5).cpu(), paste_bytes(ref, region, 0.5))


PasteTol = collections.namedtuple('PasteTol', 'img k C seed')
# seeds found on the reference alone (paste_near_counts at seeds 0, 1, 2, ...): the first at which no mask has more than
# max(2, 1e-4 H W) pixels within NEAR_PASTE of 1/2 or, in the soft mode, of an integer of p * 255
PASTE_TOL = (PasteTol((160, 200), 6, 1, 2), PasteTol((131, 177), 5, 3, 10), PasteTol((200, 300), 8, 1, 0))


def paste_tol_inputs(case, seed=None):
    g = torch.Generator().manual_seed(case.seed if seed is None else seed)
    H, W = case.img
    k = case.k
    logits = (F.avg_pool2d(torch.randn(k * case.C, 1, 28, 28, generator=g), 5, 1, 2) * 60).view(k, case.C, 28, 28)
    logits = logits.clamp(-7.5, 7.5).permute(0, 2, 3, 1).contiguous()      # p * 255 stays clear of 0 and of 255
    wh = torch.rand(k, 2, generator=g) * 30 + 12
    xy = torch.rand(k, 2, generator=g) * torch.tensor([W - 20.0, H - 20.0]) - 10      # some cross the image's sides
    boxes = torch.cat([xy, xy + wh], 1)
    labels = torch.randint(0, case.C, (k,), generator=g).to(torch.int32) if case.C > 1 else None
    return logits, labels, boxes


def paste_near(ref, region, thr):
    """bool [k, H, W]: the pixels whose fp64 field is within NEAR_PASTE of the decision values of mode `thr`"""
    if thr >= 0:
        return ((ref - thr).abs() < NEAR_PASTE) & region
    b = ref * 255
    return ((b - torch.round(b)).abs() < 255 * NEAR_PASTE) & region & (torch.round(b) >= 1)     # the truncation cannot cross 0


def paste_near_counts(case, seed=None):
    logits, labels, boxes = paste_tol_inputs(case, seed)
    ref, region = paste_field(logits, labels, boxes, case.img, F64)
    return [int(paste_near(ref, region, t).flatten(1).sum(1).max()) for t in (0.5, -1.0)]


def check_paste_tolerance(ops, dev, case, report=print):
    logits, labels, boxes = paste_tol_inputs(case)
    ref, region = paste_field(logits, labels, boxes, case.img, F64)
    r32, _ = paste_field(logits, labels, boxes, case.img, F32)
    e32 = float((r32.double() - ref).abs().max())
    assert 2 * e32 <= NEAR_PASTE, ('NEAR_PASTE is below twice the fp32 restatement distance', case, e32)
    cap = max(2, int(1e-4 * case.img[0] * case.img[1]))
    lab = None if labels is None else labels.to(dev)
    fig = dict(e32=e32, cap=cap)
    for t in (0.5, -1.0):
        near = paste_near(ref, region, t)
        n = int(near.flatten(1).sum(1).max())
        assert n <= cap, ('the reference has', n, 'pixels of a mask near a decision value (cap', cap, '): another seed', case, t)
        want = paste_bytes(ref, region, t)
        got = ops.paste_masks(logits.to(dev), lab, boxes.to(dev), case.img, t).cpu()
        assert got.dtype == want.dtype
        d = (got.int() - want.int()).abs()
        assert not bool(((d != 0) & ~near).any()), ('paste_masks differs away from a decision value', case, t, int(((d != 0) & ~near).sum()))
        assert int(d.max()) <= 1, ('a byte off by more than one', case, t)
        fig['near_hard' if t >= 0 else 'near_soft'], fig['diff_hard' if t >= 0 else 'diff_soft'] = n, int((d != 0).sum())
    report(f'sampler paste_masks {case.img} k={case.k} C={case.C}: field E32 {e32:.3e} NEAR {NEAR_PASTE:.1e}; near 1/2: {fig["near_hard"]}, '
           f'near an integer of p 255: {fig["near_soft"]} (cap {cap}); bits off {fig["diff_hard"]}, bytes off {fig["diff_soft"]}')
    return fig


# ============================================================================================================ resize and pad
RESIZE_MUTATIONS = ('no_half_pixel', 'right_bottom_unclamped', 'pad_not_normalised', 'mean_before_swap', 'scale_from_canvas',
                    'window_origin_swapped')


def _cv2_axis(n_out, n_in, n_canvas, dtype, mut):
    """cv2 INTER_LINEAR: (x + 0.5) (n_in / n_out) - 0.5 in double, a float coefficient, both ends clamped"""
    d = torch.arange(n_out, dtype=F64)
    scale = n_in / (n_canvas if mut == 'scale_from_canvas' else n_out)
    f = d * scale if mut == 'no_half_pixel' else (d + 0.5) * scale - 0.5
    if dtype == F32:
        f = f.float()
    i0 = f.floor()
    fr = f - i0
    i0 = i0.long()
    neg = i0 < 0
    i0, fr = torch.where(neg, torch.zeros_like(i0), i0), torch.where(neg, torch.zeros_like(fr), fr)
    if mut == 'right_bottom_unclamped':
        i0 = i0.clamp(max=n_in - 1)
        return i0, i0 + 1, fr.to(dtype)                                   # index n_in reads the zero line behind the image
    top = i0 >= n_in - 1
    i0, fr = torch.where(top, torch.full_like(i0, n_in - 1), i0), torch.where(top, torch.zeros_like(fr), fr)
    return i0, (i0 + 1).clamp(max=n_in - 1), fr.to(dtype)


def resize_pad_ref(img_hwc, new_hw, pad_hw, pad_val=(0.0, 0.0, 0.0), normalise=None, dtype=F64, mut=None):
    """[H, W, 3] (u8 / fp32) -> [3, Hp, Wp] in `dtype`: resize (horizontal, then vertical), pad, (swap, mean, std); the fp32
    parameters of the C call are fp32 here too"""
    H, W = img_hwc.shape[:2]
    (Hn, Wn), (Hp, Wp) = new_hw, pad_hw
    src = F.pad(img_hwc.to(dtype), (0, 0, 0, 1, 0, 1))
    x0, x1, fx = _cv2_axis(Wn, W, Wp, dtype, mut)
    y0, y1, fy = _cv2_axis(Hn, H, Hp, dtype, mut)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = src[y0][:, x0] * (1 - fx) + src[y0][:, x1] * fx
    bot = src[y1][:, x0] * (1 - fx) + src[y1][:, x1] * fx
    canvas = torch.tensor(pad_val, dtype=F32).to(dtype).expand(Hp, Wp, 3).clone()
    canvas[:Hn, :Wn] = top * (1 - fy) + bot * fy
    if normalise is not None:
        mean, std = (torch.tensor(v, dtype=F32).to(dtype) for v in normalise[:2])
        sw = [2, 1, 0] if normalise[2] else [0, 1, 2]
        out = (canvas[..., sw] - (mean[sw] if mut == 'mean_before_swap' else mean)) / std
        if mut == 'pad_not_normalised':
            out[Hn:], out[:, Wn:] = canvas[Hn:], canvas[:, Wn:]
        canvas = out
    return canvas.permute(2, 0, 1).contiguous()


ResizeCase = collections.namedtuple('ResizeCase', 'src new pad u8 norm')
_NORM_A = ((64.0, 32.0, 16.0), (8.0, 4.0, 2.0), True)                       # power-of-two std: the division is exact
_NORM_B = ((3.0, -5.0, 100.0), (0.5, 16.0, 1.0), False)
RESIZE_EXACT = (
    ResizeCase((12, 20), (12, 20), (12, 20), True, None),                    # ratio 1, no padding
    ResizeCase((12, 20), (12, 20), (16, 24), True, _NORM_A),                 # ratio 1, padded both ways, swap
    ResizeCase((12, 20), (6, 10), (6, 13), False, _NORM_B),                  # 1/2, padded on the right
    ResizeCase((12, 20), (3, 5), (7, 5), True, None),                        # 1/4, padded below
    ResizeCase((5, 7), (10, 14), (12, 16), True, _NORM_A),                   # 2, odd source
    ResizeCase((5, 7), (20, 28), (20, 31), False, None),                     # 4
    ResizeCase((6, 8), (1, 1), (1, 1), True, None),                          # to 1 x 1
    ResizeCase((5, 7), (1, 1), (3, 2), False, _NORM_B),                      # odd to 1 x 1, padded
    ResizeCase((4, 6), (1, 12), (2, 12), True, _NORM_A),                     # to 1 x N, up-sampling along x
    ResizeCase((1, 1), (4, 4), (4, 5), False, None),                         # from 1 x 1
    ResizeCase((8, 4), (4, 8), (5, 9), True, _NORM_B),                       # 1/2 down and 2 up
)
PAD_VAL = (3.0, -7.0, 11.0)


def resize_image(src, u8, seed):
    g = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (*src, 3), generator=g).to(torch.uint8)
    return _ints(g, (*src, 3))


def check_exact_resize_pad(ops, dev, case, seed=13):
    img = resize_image(case.src, case.u8, seed)
    ref = resize_pad_ref(img, case.new, case.pad, PAD_VAL, case.norm, F64)
    r32 = resize_pad_ref(img, case.new, case.pad, PAD_VAL, case.norm, F32)
    assert r32.dtype == F32 and torch.equal(r32.double(), ref), ('not an exact case: fp32 and fp64 differ', case)
    got = ops.resize_pad(img.to(dev), case.new, case.pad, PAD_VAL, normalise=case.norm)
    assert_exact(got, ref, ('resize_pad', case))


WindowCase = collections.namedtuple('WindowCase', 'scene tile new pad u8 norm')
# every tile is placed at the four corners, the middle of the four sides and inside the scene
WINDOW_EXACT = (
    WindowCase((24, 36), (8, 12), (8, 12), (8, 12), True, None),           # ratio 1, u8, Wp % 4 == 0: the convert path
    WindowCase((24, 36), (8, 20), (8, 20), (9, 24), True, _NORM_A),        # the convert path with a straddling group and padding
    WindowCase((24, 36), (8, 12), (8, 12), (8, 13), True, _NORM_A),        # ratio 1 on the general path
    WindowCase((24, 36), (8, 12), (4, 6), (6, 6), False, _NORM_B),         # 1/2
    WindowCase((24, 36), (5, 7), (10, 14), (10, 16), True, None),          # 2
    WindowCase((24, 36), (4, 8), (1, 2), (1, 2), True, None),              # 1/4 to one row
    WindowCase((24, 36), (24, 36), (24, 36), (24, 40), False, None),       # the whole scene
)


def window_origins(scene, tile):
    (SH, SW), (th, tw) = scene, tile
    xs, ys = sorted({0, (SW - tw) // 2, SW - tw}), sorted({0, (SH - th) // 2, SH - th})
    return [(x, y) for y in ys for x in xs]


def check_exact_windows(ops, dev, case, seed=17):
    """rsp_slice_resize_pad and rsp_crops_resize_pad on windows that touch every border of the scene: each tile is the fp64
    oracle of its crop and rsp_resize_pad of its crop, bit for bit"""
    scene = resize_image(case.scene, case.u8, seed)
    org = window_origins(case.scene, case.tile)
    th, tw = case.tile

    def oracle(crop):
        ref = resize_pad_ref(crop, case.new, case.pad, PAD_VAL, case.norm, F64)
        r32 = resize_pad_ref(crop, case.new, case.pad, PAD_VAL, case.norm, F32)
        assert r32.dtype == F32 and torch.equal(r32.double(), ref), ('not an exact case: fp32 and fp64 differ', case)
        return ref
    refs = [oracle(scene[y0:y0 + th, x0:x0 + tw]) for x0, y0 in org]
    ref = torch.stack(refs)
    sd = scene.to(dev)
    got = ops.slice_resize_pad(sd, torch.tensor(org, dtype=torch.int32).to(dev), case.tile, case.new, case.pad, PAD_VAL, normalise=case.norm)
    assert_exact(got, ref, ('slice_resize_pad', case))
    # crops of different sizes in one launch: the tile, and the window up to the scene's far corner resized to the same size
    SH, SW = case.scene
    table, cref = [], []
    for i, (x0, y0) in enumerate(org):
        x1, y1 = (x0 + tw, y0 + th) if i % 2 == 0 else (SW, SH)
        if (x1 - x0) not in (tw, 2 * tw, 4 * tw) or (y1 - y0) not in (th, 2 * th, 4 * th):
            x1, y1 = x0 + tw, y0 + th                                      # keep the ratio a power of two
        table.append([x0, y0, x1, y1, *case.new])
        cref.append(oracle(scene[y0:y1, x0:x1]))
    got = ops.crops_resize_pad(sd, torch.tensor(table, dtype=torch.int32).to(dev), case.pad, PAD_VAL, normalise=case.norm)
    assert_exact(got, torch.stack(cref), ('crops_resize_pad', case))
    for i, (x0, y0) in enumerate(org):
        one = ops.resize_pad(sd[y0:y0 + th, x0:x0 + tw].contiguous(), case.new, case.pad, PAD_VAL, normalise=case.norm)
        assert_exact(one, refs[i], ('resize_pad of the crop', case, i))


ResizeTol = collections.namedtuple('ResizeTol', 'src new pad u8 norm seed')
_NORM_REAL = ((123.675, 116.28, 103.53), (58.395, 57.12, 57.375), True)
RESIZE_TOL = (ResizeTol((683, 1024), (1024, 1535), (1024, 1536), True, _NORM_REAL, 1),      # 1024 / 683
              ResizeTol((300, 417), (205, 285), (224, 288), False, None, 2),
              ResizeTol((97, 131), (333, 450), (352, 450), True, None, 3))


def check_resize_tolerance(ops, dev, report=print):
    """non-integer ratios: the three entry points against the fp64 oracle (its coefficients stay double)"""
    rep = Report('resize_pad', report)
    for case in RESIZE_TOL:
        g = torch.Generator().manual_seed(case.seed)
        H, W = case.src
        if case.u8:
            img = torch.randint(0, 256, (H, W, 3), generator=g).to(torch.uint8)
        else:
            img = torch.rand(H, W, 3, generator=g) * 255
        ref = resize_pad_ref(img, case.new, case.pad, PAD_VAL, case.norm, F64)
        r32 = resize_pad_ref(img, case.new, case.pad, PAD_VAL, case.norm, F32)
        imd = img.to(dev)
        got = ops.resize_pad(imd, case.new, case.pad, PAD_VAL, normalise=case.norm)
        tag = f'{case.src} -> {case.new} in {case.pad} {"u8" if case.u8 else "f32"}'
        rep.add('resize_pad ' + tag, got, ref, r32)
        # the same image as the interior of a scene: one slice and one crop must give the same tile
        scene = torch.zeros(H + 5, W + 7, 3, dtype=img.dtype)
        scene[2:2 + H, 3:3 + W] = img
        sd = scene.to(dev)
        org = torch.tensor([[3, 2]], dtype=torch.int32).to(dev)
        got_s = ops.slice_resize_pad(sd, org, case.src, case.new, case.pad, PAD_VAL, normalise=case.norm)
        rep.add('slice_resize_pad ' + tag, got_s[0], ref, r32)
        table = torch.tensor([[3, 2, 3 + W, 2 + H, *case.new]], dtype=torch.int32).to(dev)
        got_c = ops.crops_resize_pad(sd, table, case.pad, PAD_VAL, normalise=case.norm)
        rep.add('crops_resize_pad ' + tag, got_c[0], ref, r32)
        assert torch.equal(got_s[0].cpu(), got.cpu()) and torch.equal(got_c[0].cpu(), got.cpu()), \
            ('a tile differs from resize_pad of its crop', case)
    return rep.finish()


# ================================================================================================ interpolate and the mask rule
INTERP_MUTATIONS = ('align_corners', 'no_half_pixel', 'threshold_side_flipped', 'blocked_row_kept', 'rows_summed_over_batch')


def interp_ref(x_nchw, size, dtype=F64, mut=None):
    x = x_nchw.to(dtype)
    if mut == 'no_half_pixel':                                           # src = dst * scale: nearest-corner sampling grid
        H, W = x.shape[-2:]
        ys = (torch.arange(size[0], dtype=dtype) * (H / size[0]))
        xs = (torch.arange(size[1], dtype=dtype) * (W / size[1]))
        y0, x0 = ys.floor().long(), xs.floor().long()
        y1, x1 = (y0 + 1).clamp(max=H - 1), (x0 + 1).clamp(max=W - 1)
        fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
        top = x[..., y0, :][..., x0] * (1 - fx) + x[..., y0, :][..., x1] * fx
        bot = x[..., y1, :][..., x0] * (1 - fx) + x[..., y1, :][..., x1] * fx
        return top * (1 - fy) + bot * fy
    return F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=(mut == 'align_corners'))


def resize_nhwc_ref(x_nhwc, size, dtype=F64, mut=None):
    return interp_ref(x_nhwc.permute(0, 3, 1, 2), size, dtype, mut).permute(0, 2, 3, 1).contiguous()


def attn_mask_ref(mpp, size, dtype=F64, mut=None, want_field=False):
    """models.py:381-392 + 439-442: uint8 [B, Nq, h w], 1 = blocked (sigmoid < 0.5), fully blocked rows cleared"""
    z = interp_ref(mpp, size, dtype, mut).flatten(2)
    am = (z.sigmoid() <= 0.5) if mut == 'threshold_side_flipped' else (z.sigmoid() < 0.5)
    full = am.sum(-1) == am.shape[-1]
    if mut == 'rows_summed_over_batch':
        full = full.all(0, keepdim=True).expand_as(full)
    if mut != 'blocked_row_kept':
        am = am & ~full.unsqueeze(-1)
    return (am.to(torch.uint8), z) if want_field else am.to(torch.uint8)


InterpCase = collections.namedtuple('InterpCase', 'src out C')
INTERP_EXACT = (InterpCase((6, 10), (6, 10), 8), InterpCase((6, 10), (12, 20), 4), InterpCase((5, 3), (20, 12), 8),
                InterpCase((12, 20), (6, 10), 132), InterpCase((1, 1), (4, 8), 4), InterpCase((8, 4), (1, 1), 8),
                InterpCase((7, 9), (1, 1), 4), InterpCase((4, 8), (8, 4), 128), InterpCase((16, 16), (4, 32), 4))


def check_exact_interp(ops, dev, case, seed=19):
    g = torch.Generator().manual_seed(seed)
    B = 2
    x = _ints(g, (B, *case.src, case.C))
    ref = resize_nhwc_ref(x, case.out, F64)
    r32 = resize_nhwc_ref(x, case.out, F32)
    assert r32.dtype == F32 and torch.equal(r32.double(), ref), ('not an exact case: fp32 and fp64 differ', case)
    assert_exact(ops.resize_bilinear(x.to(dev), case.out), ref, ('resize_bilinear', case))
    # the mask rule: row 0 of image 0 fully blocked (cleared), row 1 all zeros (sigmoid = 1/2: nothing blocked), row 2 fully
    # blocked but for one zero, the rest random integers whose resized values tie with 0
    Nq = 6
    mpp = _ints(g, (B, Nq, *case.src), -2, 2)
    mpp[0, 0], mpp[:, 1], mpp[:, 2] = -5.0, 0.0, -3.0
    mpp[:, 2, -1, -1] = 0.0
    want, z = attn_mask_ref(mpp, case.out, F64, want_field=True)
    w32, z32 = attn_mask_ref(mpp, case.out, F32, want_field=True)
    assert torch.equal(z32.double(), z) and torch.equal(w32, want), ('not an exact case: fp32 and fp64 differ', case)
    n = case.out[0] * case.out[1]
    assert bool((z[:, 3:] == 0).any()) or n == 1, ('no resized logit ties with the threshold', case)
    assert int(want[0, 0].sum()) == 0 and bool((z[0, 0] < 0).all()) and int(want[:, 1].sum()) == 0
    got = ops.query_attn_mask(mpp.contiguous().to(dev), case.out).cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, Nq, n)
    assert torch.equal(got, want), ('query_attn_mask', case, _first_diff(got, want))


InterpTol = collections.namedtuple('InterpTol', 'src out C seed')
INTERP_TOL = (InterpTol((25, 38), (50, 75), 128, 1), InterpTol((64, 64), (23, 31), 128, 2), InterpTol((17, 29), (100, 100), 256, 3))
# mask seeds found on the reference alone (qmask_near_count at seeds 0, 1, 2, ...): the first with at most max(2, 1e-4 h w)
# resized logits of a row within NEAR_QMASK of 0
QMASK_TOL = (InterpTol((128, 128), (32, 32), 0, 0), InterpTol((100, 136), (25, 34), 0, 0), InterpTol((64, 64), (50, 70), 0, 0))


def qmask_inputs(case, seed=None):
    g = torch.Generator().manual_seed(case.seed if seed is None else seed)
    mpp = F.avg_pool2d(torch.randn(2, 7, *case.src, generator=g), 5, 1, 2) * 15
    mpp[0, 0] = -mpp[0, 0].abs() - 1.0                                   # a fully blocked row
    return mpp.contiguous()


def qmask_near_count(case, seed=None):
    _, z = attn_mask_ref(qmask_inputs(case, seed), case.out, F64, want_field=True)
    return int((z.abs() < NEAR_QMASK).sum(-1).max())


def check_interp_tolerance(ops, dev, report=print):
    rep = Report('resize_bilinear', report)
    for case in INTERP_TOL:
        g = torch.Generator().manual_seed(case.seed)
        x = torch.randn(2, *case.src, case.C, generator=g)
        rep.add(f'{case.src} -> {case.out} C={case.C}', ops.resize_bilinear(x.to(dev), case.out), resize_nhwc_ref(x, case.out, F64),
                resize_nhwc_ref(x, case.out, F32))
    figs = []
    for case in QMASK_TOL:
        mpp = qmask_inputs(case)
        want, z = attn_mask_ref(mpp, case.out, F64, want_field=True)
        _, z32 = attn_mask_ref(mpp, case.out, F32, want_field=True)
        e32 = float((z32.double() - z).abs().max())
        assert 2 * e32 <= NEAR_QMASK, ('NEAR_QMASK is below twice the fp32 restatement distance', case, e32)
        near = z.abs() < NEAR_QMASK
        n, cap = int(near.sum(-1).max()), max(2, int(1e-4 * case.out[0] * case.out[1]))
        assert n <= cap, ('the reference has', n, 'logits of a row within NEAR_QMASK of 0 (cap', cap, '): another seed', case)
        assert int(want[0, 0].sum()) == 0 and bool((z[0, 0] < -NEAR_QMASK).all()), 'the fully blocked row'
        # a row is cleared only when every logit is negative: no other row may come within NEAR of that
        assert bool(((z > NEAR_QMASK).any(-1) | (z < -NEAR_QMASK).all(-1)).all()), ('a row that is fully blocked but for near pixels', case)
        got = ops.query_attn_mask(mpp.to(dev), case.out).cpu()
        bad = (got != want) & ~near
        assert not bool(bad.any()), ('query_attn_mask differs away from the threshold', case, int(bad.sum()))
        figs.append((case, e32, n, cap, int((got != want).sum())))
        report(f'sampler query_attn_mask {case.src} -> {case.out}: field E32 {e32:.3e} NEAR {NEAR_QMASK:.1e}; near 0: {n} (cap {cap}); '
               f'bits off {figs[-1][4]}')
    return rep.finish(), figs


# =================================================================================================================== MSDeform
MSDA_MUTATIONS = ('xy_swapped', 'level_start_off_by_one_map', 'border_padding', 'softmax_over_points_only', 'align_corners',
                  'offsets_not_normalised_per_level')
MS_H, MS_P = 8, 4


def msdeform_ref(value, offs_weights, ref_points, B, Ntok, level_hw, head_dim=16, dtype=F64, mut=None):
    """mmcv multi_scale_deformable_attn_pytorch on the kernel's packed operands: value [B Ntok, 8 D]; offs_weights
    [B Ntok, >= 8 L 4 3]: offsets (h, l, p, xy), then logits (h, l p); ref_points [Ntok, 2] -> [B Ntok, 8 D]"""
    L, D = len(level_hw), head_dim
    v = value.to(dtype).view(B, Ntok, MS_H, D)
    ow = offs_weights.to(dtype)
    off = ow[:, :MS_H * L * MS_P * 2].reshape(B, Ntok, MS_H, L, MS_P, 2)
    logit = ow[:, MS_H * L * MS_P * 2:MS_H * L * MS_P * 3].reshape(B, Ntok, MS_H, L, MS_P)
    if mut == 'softmax_over_points_only':
        w = logit.softmax(-1)
    else:
        w = logit.flatten(3).softmax(-1).view(B, Ntok, MS_H, L, MS_P)
    rp = ref_points.to(dtype)
    out = torch.zeros(B, MS_H, D, Ntok, dtype=dtype)
    start = 0
    for l, (Hl, Wl) in enumerate(level_hw):
        n = Hl * Wl
        s = min(start + n, Ntok - n) if mut == 'level_start_off_by_one_map' else start      # the next map's start
        vl = v[:, s:s + n].permute(0, 2, 3, 1).reshape(B * MS_H, D, Hl, Wl)
        start += n
        norm = torch.tensor([Wl, Hl], dtype=dtype)
        if mut == 'offsets_not_normalised_per_level':
            norm = torch.tensor([level_hw[0][1], level_hw[0][0]], dtype=dtype)
        loc = rp[None, :, None, None, :] + off[:, :, :, l] / norm                      # [B, Ntok, 8, P, 2]
        grid = (2 * loc - 1).permute(0, 2, 1, 3, 4).reshape(B * MS_H, Ntok, MS_P, 2)
        if mut == 'xy_swapped':
            grid = grid.flip(-1)
        smp = F.grid_sample(vl, grid, mode='bilinear', padding_mode='border' if mut == 'border_padding' else 'zeros',
                            align_corners=(mut == 'align_corners'))                    # [B 8, D, Ntok, P]
        wl = w[:, :, :, l].permute(0, 2, 1, 3).reshape(B * MS_H, 1, Ntok, MS_P)
        out += (smp * wl).sum(-1).view(B, MS_H, D, Ntok)
    return out.permute(0, 3, 1, 2).reshape(B * Ntok, MS_H * D).contiguous()


MsdaCase = collections.namedtuple('MsdaCase', 'levels hd')
MSDA_EXACT = (MsdaCase(((4, 8),), 16), MsdaCase(((1, 1), (2, 4)), 32), MsdaCase(((8, 8), (4, 2), (2, 2), (1, 1)), 16),
              MsdaCase(((2, 8), (8, 2), (4, 4), (1, 2)), 32), MsdaCase(((1, 1),), 32), MsdaCase(((8, 4), (1, 4)), 16))
MSDA_EDGES = ('-1', '-0.5', 'n-0.5', 'n', 'far')


def msda_exact_inputs(case, seed, census=None):
    """integer values; reference points and offsets on the 1/8 grid with every fifth sample steered onto -1, -1/2, n - 1/2,
    n (pixel coordinates, on x and on y in turn) or far outside; logits all equal in image 0 (a uniform softmax), one at 0
    and the rest at -1e4 in image 1 (one-hot)"""
    g = torch.Generator().manual_seed(seed)
    L = len(case.levels)
    ntok, B = sum(h * w for h, w in case.levels), 2
    value = _ints(g, (B * ntok, MS_H * case.hd))
    rp = torch.randint(0, 9, (ntok, 2), generator=g).float() / 8
    off = torch.randint(-24, 25, (B, ntok, MS_H, L, MS_P, 2), generator=g).float() / 8
    size = torch.tensor([[w, h] for h, w in case.levels], dtype=F32)[None, None, None, :, None, :]      # (x, y) extents
    pix = rp[None, :, None, None, None, :] * size + off - 0.5                                               # the sample's pixel coordinate
    kind = torch.randint(0, 10, pix.shape, generator=g)
    target = torch.where(kind == 0, torch.full_like(pix, -1.0), pix)
    target = torch.where(kind == 1, torch.full_like(pix, -0.5), target)
    target = torch.where(kind == 2, size - 0.5 + torch.zeros_like(pix), target)
    target = torch.where(kind == 3, size + torch.zeros_like(pix), target)
    target = torch.where(kind == 4, torch.full_like(pix, 40.0) * (1 - 2 * (pix < 0).float()), target)
    off = target + 0.5 - rp[None, :, None, None, None, :] * size
    if census is not None:
        for name, hit in zip(MSDA_EDGES, ((target == -1), (target == -0.5), (target == size - 0.5), (target == size), (target.abs() == 40))):
            census[name] = census.get(name, 0) + int(hit.sum())
    logit = torch.zeros(B, ntok, MS_H, L * MS_P)
    hot = torch.randint(0, L * MS_P, (ntok, MS_H), generator=g)
    logit[1] = -1e4
    logit[1].scatter_(-1, hot[..., None], 0.0)
    tail = torch.full((B * ntok, 3), 77.0)                                                    # ld_ow > 8 L 4 3
    ow = torch.cat([off.reshape(B * ntok, -1), logit.reshape(B * ntok, -1), tail], 1).contiguous()
    return value, ow, rp.contiguous(), B, ntok


def _msdeform_v1(ops, value, ow, rp, B, ntok, levels):
    """the first-generation entry point rsp_msdeform_attn (head dim 16), which `ops` no longer calls: through the library the
    wrappers use; a stand-in without one answers with its msdeform_attn"""
    if not hasattr(ops, '_lib'):
        return ops.msdeform_attn(value, ow, rp, B, ntok, levels, head_dim=16)
    lib = ops._lib.load()
    out = torch.empty((B * ntok, MS_H * 16), dtype=F32, device=value.device)
    hw = (ctypes.c_int * (2 * len(levels)))(*[int(v) for s in levels for v in s])
    ops._lib.check(lib.rsp_msdeform_attn(value.data_ptr(), ow.data_ptr(), ow.shape[1], rp.data_ptr(), out.data_ptr(), B, ntok,
                                         len(levels), hw, ops._stream()), 'rsp_msdeform_attn')
    return out


def check_exact_msdeform(ops, dev, case, seed=23):
    levels = [tuple(l) for l in case.levels]
    value, ow, rp, B, ntok = msda_exact_inputs(case, seed)
    ref = msdeform_ref(value, ow, rp, B, ntok, levels, case.hd, F64)
    r32 = msdeform_ref(value, ow, rp, B, ntok, levels, case.hd, F32)
    assert r32.dtype == F32 and torch.equal(r32.double(), ref), \
        ('not an exact case: fp32 and fp64 differ', case, _first_diff(r32.double(), ref))
    vd, od, rd = _to(dev, value, ow, rp)
    assert_exact(ops.msdeform_attn(vd, od, rd, B, ntok, levels, head_dim=case.hd), ref, ('msdeform_attn_ex', case))
    if case.hd == 16:
        assert_exact(_msdeform_v1(ops, vd, od, rd, B, ntok, levels), ref, ('msdeform_attn', case))


MsdaTol = collections.namedtuple('MsdaTol', 'levels hd seed')
MSDA_TOL = (MsdaTol(((32, 32), (16, 16), (8, 8)), 16, 1), MsdaTol(((25, 38), (13, 19), (7, 10)), 32, 2),
            MsdaTol(((12, 9), (6, 5), (3, 3), (2, 1), (1, 1)), 16, 3), MsdaTol(((20, 30),), 32, 4))


def check_msdeform_tolerance(ops, dev, report=print):
    rep = Report('msdeform_attn', report)
    for case in MSDA_TOL:
        g = torch.Generator().manual_seed(case.seed)
        levels = [tuple(l) for l in case.levels]
        L = len(levels)
        ntok, B = sum(h * w for h, w in levels), 2
        value = torch.randn(B * ntok, MS_H * case.hd, generator=g)
        n_lp = MS_H * L * MS_P
        ow = torch.cat([torch.randn(B * ntok, n_lp * 2, generator=g) * 3, torch.randn(B * ntok, n_lp, generator=g) * 2], 1).contiguous()
        rp = torch.rand(ntok, 2, generator=g)
        ref = msdeform_ref(value, ow, rp, B, ntok, levels, case.hd, F64)
        r32 = msdeform_ref(value, ow, rp, B, ntok, levels, case.hd, F32)
        vd, od, rd = _to(dev, value, ow, rp)
        rep.add(f'L={L} hd={case.hd} ntok={ntok} (ex)', ops.msdeform_attn(vd, od, rd, B, ntok, levels, head_dim=case.hd), ref, r32)
        if case.hd == 16:
            rep.add(f'L={L} hd=16 ntok={ntok} (v1)', _msdeform_v1(ops, vd, od, rd, B, ntok, levels), ref, r32)
    return rep.finish()


# ========================================================================================================= failure signatures
class FakeOps:
    """the wrappers of rsprompter_amd.ops for the ten entry points, computed by the fp32 restatements on the CPU with at most
    one mutation (tests/test_kernel_props_selfcheck_cpu.py)"""

    def __init__(self, mutation=None):
        known = ROI_MUTATIONS + ROI_TOL_MUTATIONS + PASTE_MUTATIONS + RESIZE_MUTATIONS + INTERP_MUTATIONS + MSDA_MUTATIONS
        assert mutation is None or mutation in known, mutation
        self.mut = mutation

    def _m(self, family):
        return self.mut if self.mut in family else None

    def roi_align(self, feats, pes, rois, P, strides, finest_scale=56):
        return roi_align_ref(feats, pes, rois, P, strides, finest_scale, F32, self._m(ROI_MUTATIONS + ROI_TOL_MUTATIONS))

    def paste_masks(self, logits_nhwc, labels, boxes, img_hw, thr=0.5):
        mut = self._m(PASTE_MUTATIONS)
        if mut == 'no_region_margin' and thr >= 0:
            mut = None                                                  # the mistake of the soft mode's fast path only
        field, region = paste_field(logits_nhwc, labels, boxes, img_hw, F32, mut)
        return paste_bytes(field, region, thr, mut)

    def resize_pad(self, img_hwc, new_hw, pad_hw, pad_val=(0.0, 0.0, 0.0), out=None, normalise=None):
        return resize_pad_ref(img_hwc, new_hw, pad_hw, pad_val, normalise, F32, self._m(RESIZE_MUTATIONS))

    def _window(self, scene, x0, y0, x1, y1):
        if self.mut == 'window_origin_swapped':
            w, h = x1 - x0, y1 - y0
            x0, y0 = min(y0, scene.shape[1] - w), min(x0, scene.shape[0] - h)
            x1, y1 = x0 + w, y0 + h
        return scene[y0:y1, x0:x1]

    def slice_resize_pad(self, scene_hwc, origins, tile_hw, new_hw, pad_hw, pad_val=(0.0, 0.0, 0.0), out=None, normalise=None):
        return torch.stack([self.resize_pad(self._window(scene_hwc, x0, y0, x0 + tile_hw[1], y0 + tile_hw[0]), new_hw, pad_hw, pad_val,
                                            normalise=normalise) for x0, y0 in origins.tolist()])

    def crops_resize_pad(self, image_hwc, table, pad_hw, pad_val=(0.0, 0.0, 0.0), out=None, normalise=None):
        return torch.stack([self.resize_pad(self._window(image_hwc, x0, y0, x1, y1), (hn, wn), pad_hw, pad_val, normalise=normalise)
                            for x0, y0, x1, y1, hn, wn in table.tolist()])

    def resize_bilinear(self, x_nhwc, size):
        mut = self._m(INTERP_MUTATIONS)
        return resize_nhwc_ref(x_nhwc, size, F32, mut if mut in ('align_corners', 'no_half_pixel') else None)

    def query_attn_mask(self, mask_pred_plus, size):
        return attn_mask_ref(mask_pred_plus, size, F32, self._m(INTERP_MUTATIONS))

    def msdeform_attn(self, value, offs_weights, ref_points, B, Ntok, level_hw, head_dim=16):
        return msdeform_ref(value, offs_weights, ref_points, B, Ntok, level_hw, head_dim, F32, self._m(MSDA_MUTATIONS))
