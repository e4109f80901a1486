"""-m gpu: `min_mask_region_area` ("small regions"): rsp_mask_remove_small_regions -- connected-component labelling
of masks on the device -- and the generator step around it, against a numpy restatement of segment-anything's
`remove_small_regions` / `postprocess_small_regions` on scipy.ndimage.label (whose labels are numbered by first pixel in raster
order: the tie rule of this project).  Every comparison is exact.  The `check_*` bodies also run on the lane-level emulator
(tests/test_mask_regions_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

MODES = {1: 'holes', 2: 'islands', 3: 'both'}
EIGHT = np.ones((3, 3), dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------- the oracle
def ref_remove_small_regions(mask, area, mode):
    """the Semantics section of the issue on one bool [H, W] array: (result, changed)"""
    from scipy import ndimage
    holes = mode == 'holes'
    working = ~mask if holes else mask
    lab, n = ndimage.label(working, structure=EIGHT)
    if n == 0:
        return mask.copy(), False
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    small = sizes < area
    if not small.any():
        return mask.copy(), False
    if holes:
        return mask | np.isin(lab, np.nonzero(small)[0] + 1), True
    keep = np.nonzero(~small)[0] + 1
    if len(keep) == 0:
        keep = [int(np.argmax(sizes)) + 1]               # the first of the largest: scipy numbers by first pixel, raster order
    return np.isin(lab, keep), True


def ref_box(mask):
    ys, xs = np.nonzero(mask)
    return [0, 0, 0, 0] if len(ys) == 0 else [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def ref_regions(masks, area, mode):
    """(out bool [k, H, W], info int32 [k, 8]) of the op for a numpy bool stack; mode 1 / 2 / 3"""
    out = np.zeros_like(masks)
    info = np.zeros((masks.shape[0], 8), dtype=np.int32)
    for i, m in enumerate(masks):
        ch = ci = False
        if mode & 1:
            m, ch = ref_remove_small_regions(m, area, 'holes')
        if mode & 2:
            m, ci = ref_remove_small_regions(m, area, 'islands')
        out[i] = m
        info[i] = [int(ch), int(ci)] + ref_box(m) + [int(m.sum()), 0]
    return out, info


def run_and_compare(ops, dev, masks, area, mode, what=''):
    """masks: numpy bool [k, H, W]; the op against the oracle, all eight info columns, exactly"""
    want, winfo = ref_regions(masks, area, mode)
    t = torch.from_numpy(masks).to(dev)
    out, info = ops.remove_small_regions(t, area, MODES[mode])
    assert out.dtype == torch.bool and tuple(out.shape) == tuple(masks.shape) and info.dtype == torch.int32
    assert tuple(info.shape) == (masks.shape[0], 8)
    assert torch.equal(t.cpu(), torch.from_numpy(masks)), 'the input is left alone'
    info_h = info.cpu()
    assert not bool(info_h[:, 7].any()), ('status', what, area, mode)
    bad = (out.cpu() != torch.from_numpy(want)).flatten(1).any(1).nonzero()[:, 0].tolist()
    assert not bad, (what, 'area', area, 'mode', mode, 'masks', bad)
    assert torch.equal(info_h, torch.from_numpy(winfo)), (what, area, mode, info_h.tolist(), winfo.tolist())
    return out, info


# ----------------------------------------------------------------------------------------- 1. known answers, by hand
def _grid(rows):
    return np.array([[c == '#' for c in r] for r in rows], dtype=bool)


def check_known_answers(ops, dev):
    def call(m, area, mode):
        out, info = ops.remove_small_regions(torch.from_numpy(m[None]).to(dev), area, mode)
        return out[0].cpu().numpy(), info[0].cpu().tolist()

    # a diagonal pair is ONE component (size 2); a component of exactly min_area = 3 stays; one of min_area - 1 = 2 goes
    m = _grid(['#........',
               '.#...###.',
               '.........',
               '.........',
               '..##.....',
               '.........'])
    assert m.shape == (6, 9)
    out, info = call(m, 2, 'islands')
    assert np.array_equal(out, m) and info == [0, 0, 0, 0, 7, 4, 7, 0]          # nothing below 2: unchanged
    out, info = call(m, 3, 'islands')
    assert np.array_equal(out, _grid(['.........', '.....###.', '.........', '.........', '.........', '.........']))
    assert info == [0, 1, 5, 1, 7, 1, 3, 0]
    # were the diagonal pair two components of size 1, min_area = 2 would remove them
    out, info = call(_grid(['#..', '.#.', '...']), 2, 'islands')
    assert out.sum() == 2 and info[:2] == [0, 0]
    # holes: a small background pocket that touches the border is filled like any other; the large background is not
    m = _grid(['..#......',
               '###......',
               '.........',
               '....###..',
               '....#.#..',
               '....###..'])
    out, info = call(m, 3, 'holes')
    want = m.copy()
    want[0, :2] = True                                                           # the pocket (size 2) at the corner
    want[4, 5] = True                                                            # the pinhole (size 1)
    assert np.array_equal(out, want) and info == [1, 0, 0, 0, 6, 5, 15, 0]
    out, info = call(m, 2, 'holes')                                              # the pocket has exactly min_area pixels: stays
    want = m.copy()
    want[4, 5] = True
    assert np.array_equal(out, want) and info[:2] == [1, 0] and info[6] == 13
    # all small, a unique largest component: it alone stays
    m = _grid(['##.......',
               '.........',
               '...###...',
               '.........',
               '.......#.',
               '.........'])
    out, info = call(m, 100, 'islands')
    assert np.array_equal(out, _grid(['.........', '.........', '...###...', '.........', '.........', '.........']))
    assert info == [0, 1, 3, 2, 5, 2, 3, 0]
    # all small, two of size 3: the one with the lower first pixel (row-major) stays -- here the one that starts in row 1,
    # although the other one reaches further left
    m = _grid(['.........',
               '......#..',
               '......#..',
               '###...#..',
               '.........',
               '....##...'])
    out, info = call(m, 100, 'islands')
    assert np.array_equal(out, _grid(['.........', '......#..', '......#..', '......#..', '.........', '.........']))
    assert info == [0, 1, 6, 1, 6, 3, 3, 0]
    # 'both': the pinhole is filled first, then the ring (now a 3 x 3 block of 9) survives min_area = 9, the bar does not
    m = _grid(['.........',
               '.###.....',
               '.#.#.....',
               '.###.....',
               '.........',
               '.....####'])
    out, info = call(m, 9, 'both')
    assert np.array_equal(out, _grid(['.........', '.###.....', '.###.....', '.###.....', '.........', '.........']))
    assert info == [1, 1, 1, 1, 3, 3, 9, 0]


# ---------------------------------------------------------------------------------------------------- 2. random fields
def smooth_noise(hw, seed, k=1, cells=9):
    """thresholded smooth noise: bool [k, H, W] (a coarse normal field, bilinearly enlarged, > 0)"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(k, 1, cells, cells, generator=g)
    f = torch.nn.functional.interpolate(z, size=hw, mode='bicubic', align_corners=False)
    f = f + 0.35 * torch.randn(k, 1, hw[0], hw[1], generator=g)
    return (f[:, 0] > 0).numpy()


def random_fields(hw=(150, 203)):
    rng = np.random.default_rng(11)
    m = [rng.random(hw) < d for d in (0.35, 0.45, 0.55, 0.65)]
    return np.stack(m + [smooth_noise(hw, 3)[0]])


def check_random_fields(ops, dev):
    masks = random_fields()
    from scipy import ndimage
    l1, n1 = ndimage.label(masks[2], structure=EIGHT)
    l0, n0 = ndimage.label(~masks[2], structure=EIGHT)
    s1, s0 = np.bincount(l1.ravel())[1:], np.bincount(l0.ravel())[1:]
    assert 0 < (s1 < 8).sum() < n1 and 0 < (s0 < 8).sum() < n0                    # both outcomes in both polarities
    for area in (0, 1, 2, 8, 50, 10 ** 9):
        for mode in (1, 2, 3):
            _, info = run_and_compare(ops, dev, masks, area, mode, 'random fields')
            if area <= 1:
                assert not bool(info[:, :2].any())


# ------------------------------------------------------------------------------------------------------------ 3. seams
def seam_patterns(ops):
    th, tw = ops.MASK_REGION_TILE
    H, W = 3 * th + 5, 3 * tw + 7
    z = lambda: np.zeros((H, W), dtype=bool)   # noqa: E731
    pats = {}
    m = z(); m[th // 2, tw - 5:tw + 6] = True; m[5, 5] = True; pats['bar over a vertical seam'] = m
    m = z(); m[th - 5:th + 6, tw // 2] = True; m[5, 5] = True; pats['bar over a horizontal seam'] = m
    m = z(); m[th - 1, tw - 1] = m[th, tw] = True; m[2 * th - 1, 2 * tw - 1] = m[2 * th, 2 * tw] = True; m[3, 9:12] = True
    pats['diagonal corner pair'] = m
    m = z(); m[th - 1, tw] = m[th, tw - 1] = True; m[2 * th - 1, 2 * tw] = m[2 * th, 2 * tw - 1] = True; m[3, 9:12] = True
    pats['anti-diagonal corner pair'] = m
    m = z()                                                                         # serpentine: rows 0, 4, 8, ... joined at alternating ends
    for i, y in enumerate(range(0, H, 4)):
        m[y, :] = True
        if y + 4 < H:
            m[y:y + 4, W - 1 if i % 2 == 0 else 0] = True
    pats['serpentine'] = m
    m = z()                                                                         # a rectangular spiral, one pixel wide, gap 1
    t, l, b, r = 0, 0, H - 1, W - 1
    m[0, :] = True
    while b - t > 4 and r - l > 4:
        m[t:b + 1, r] = True
        m[b, l:r + 1] = True
        t += 2
        m[t:b + 1, l] = True
        r -= 2
        m[t, l:r + 1] = True
        b -= 2; l += 2
    pats['spiral'] = m
    m = z(); m[:, ::2] = True; m[:-1, 1::2] = False; m[H - 1, :] = True; pats['comb joined in the last row'] = m
    return pats


def check_seams(ops, dev):
    from scipy import ndimage
    pats = seam_patterns(ops)
    assert ndimage.label(pats['serpentine'], structure=EIGHT)[1] == 1 and ndimage.label(pats['comb joined in the last row'], structure=EIGHT)[1] == 1
    assert ndimage.label(pats['diagonal corner pair'], structure=EIGHT)[1] == 3
    assert ndimage.label(pats['anti-diagonal corner pair'], structure=EIGHT)[1] == 3
    names = list(pats)
    stack = np.stack([pats[n] for n in names])
    for area in (3, 12, 10 ** 9):
        run_and_compare(ops, dev, stack, area, 2, names)
        run_and_compare(ops, dev, ~stack, area, 1, ['complement of ' + n for n in names])
        run_and_compare(ops, dev, stack, area, 3, names)


# ------------------------------------------------------------------------------------------------- 4. degenerate shapes
def check_degenerate(ops, dev):
    rng = np.random.default_rng(5)
    for hw in ((1, 1), (1, 300), (300, 1), (7, 5)) + tuple((9, w) for w in (15, 16, 17, 63, 65)) + ((70, 64), (66, 80)):
        m = np.stack([rng.random(hw) < 0.5, rng.random(hw) < 0.8, np.zeros(hw, dtype=bool), np.ones(hw, dtype=bool)])
        yy, xx = np.mgrid[:hw[0], :hw[1]]
        m = np.concatenate([m, ((yy + xx) % 2 == 0)[None]])                         # checkerboard: one component each way
        for area in (2, 4, 10 ** 9):
            for mode in (1, 2, 3):
                run_and_compare(ops, dev, m, area, mode, hw)


# ------------------------------------------------------------------------------------------------------ 5. independence
def check_independence(ops, dev, monkeypatch):
    masks = np.concatenate([random_fields((70, 83)), smooth_noise((70, 83), 8, k=2)])
    t = torch.from_numpy(masks).to(dev)
    out, info = ops.remove_small_regions(t, 8, 'both')
    for i in range(masks.shape[0]):
        o1, i1 = ops.remove_small_regions(t[i:i + 1].contiguous(), 8, 'both')
        assert torch.equal(o1[0], out[i]) and torch.equal(i1[0], info[i])
    per = 8 * 70 * 83 + 4096
    monkeypatch.setattr(ops, 'MASK_REGIONS_WORKSPACE_LIMIT_BYTES', 3 * per)         # 7 masks in chunks of at most 3
    lib = ops._lib.load()
    o2, i2 = ops.remove_small_regions(t, 8, 'both')
    assert torch.equal(o2, out) and torch.equal(i2, info)
    assert int(lib.rsp_mask_regions_workspace_bytes(3, 70, 83)) <= 3 * per < int(lib.rsp_mask_regions_workspace_bytes(4, 70, 83))
    run_and_compare(ops, dev, masks, 8, 3, 'chunked')
    monkeypatch.setattr(ops, 'MASK_REGIONS_WORKSPACE_LIMIT_BYTES', 1)              # smaller than one mask: one at a time
    o3, i3 = ops.remove_small_regions(t, 8, 'both')
    assert torch.equal(o3, out) and torch.equal(i3, info)


# ---------------------------------------------------------------------------------------------------------- 6. refusals
def check_refusals(ops, dev):
    m = torch.zeros((2, 8, 8), dtype=torch.bool, device=dev)
    lib = ops._lib.load()
    for bad in (dict(mode='both', min_area=-1), dict(mode='ring', min_area=1), dict(mode=3, min_area=1), dict(mode='both', min_area=1.5)):
        with pytest.raises(ValueError):
            ops.remove_small_regions(m, bad['min_area'], bad['mode'])
    with pytest.raises(ValueError):
        ops.remove_small_regions(m.float(), 1)
    with pytest.raises(ValueError):
        ops.remove_small_regions(m[:, :, ::2], 1)                                   # not contiguous
    with pytest.raises(ValueError):
        ops.remove_small_regions(m[0], 1)                                           # [H, W]
    with pytest.raises(ValueError, match='2\\^31'):
        ops.remove_small_regions(_huge(dev), 1)                                     # refused on the shape, nothing allocated
    out, info = ops.remove_small_regions(m[:0], 4)                                  # k = 0
    assert tuple(out.shape) == (0, 8, 8) and tuple(info.shape) == (0, 8)
    o8, _ = ops.remove_small_regions(m.to(torch.uint8) + 7, 4, 'holes')             # uint8, non-zero = set
    assert bool(o8.all())
    # the C entry point
    ws = torch.zeros(4096, dtype=torch.int64, device=dev)
    out = torch.zeros((2, 8, 8), dtype=torch.uint8, device=dev)
    info = torch.zeros((2, 8), dtype=torch.int32, device=dev)
    args = lambda **kw: [kw.get('masks', m.data_ptr()), kw.get('k', 2), kw.get('H', 8), kw.get('W', 8), kw.get('area', 1),  # noqa: E731
                         kw.get('mode', 3), ws.data_ptr(), out.data_ptr(), info.data_ptr(), None]
    for kw in (dict(mode=0), dict(mode=4), dict(area=-1), dict(H=0), dict(W=-3), dict(k=-1), dict(H=1 << 16, W=1 << 15),
               dict(masks=out.data_ptr())):
        assert lib.rsp_mask_remove_small_regions(*args(**kw)) == -1, kw
    assert lib.rsp_mask_remove_small_regions(*args(k=0)) == 0
    assert lib.rsp_mask_regions_workspace_bytes(1, 1 << 16, 1 << 15) == -1 and lib.rsp_mask_regions_workspace_bytes(2, 0, 4) == -1
    assert lib.rsp_mask_regions_workspace_bytes(64, 1024, 1024) >= 64 * 1024 * 1024 * 8
    assert lib.rsp_mask_regions_workspace_bytes(0, 4, 4) >= 0
    with pytest.raises(RuntimeError, match='iteration cap'):
        ops.check_region_status([0, 1, 0])
    ops.check_region_status([0, 0])


def _huge(dev):
    """a [1, 65536, 32768] bool view of 2^31 pixels that owns one byte"""
    return torch.zeros((1, 1, 1), dtype=torch.bool, device=dev).expand(1, 1 << 16, 1 << 15)


# ------------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.quick
def test_known_answers(dev):
    from rsprompter_amd import ops
    check_known_answers(ops, dev)


@pytest.mark.quick
def test_random_fields(dev):
    from rsprompter_amd import ops
    check_random_fields(ops, dev)


@pytest.mark.quick
def test_seams(dev):
    from rsprompter_amd import ops
    check_seams(ops, dev)


@pytest.mark.quick
def test_degenerate_shapes(dev):
    from rsprompter_amd import ops
    check_degenerate(ops, dev)


@pytest.mark.quick
def test_masks_are_independent(dev, monkeypatch):
    from rsprompter_amd import ops
    check_independence(ops, dev, monkeypatch)


@pytest.mark.quick
def test_refusals(dev):
    from rsprompter_amd import ops
    check_refusals(ops, dev)


def serpentine(hw, pitch=2):
    """one component, one pixel wide, through every tile: every `pitch`-th row, joined at alternating ends"""
    H, W = hw
    m = np.zeros(hw, dtype=bool)
    for i, y in enumerate(range(0, H, pitch)):
        m[y, :] = True
        if y + pitch < H:
            m[y:y + pitch, W - 1 if i % 2 == 0 else 0] = True
    return m


@pytest.mark.quick
@pytest.mark.parametrize('field', ('smooth_noise_8x1024', 'serpentine_1024'))
def test_blocks_that_run_concurrently(dev, field):
    """where the seam merge really is contended: 1024 x 1024 masks (256 tiles each), every mode, twice with equal bits"""
    from scipy import ndimage
    from rsprompter_amd import ops
    if field == 'smooth_noise_8x1024':
        masks = smooth_noise((1024, 1024), 21, k=8, cells=24)
    else:
        masks = serpentine((1024, 1024))[None]
        assert ndimage.label(masks[0], structure=EIGHT)[1] == 1
    for mode in (1, 2, 3):
        for area in ((100,) if field.startswith('smooth') else (100, 10 ** 9)):
            out, info = run_and_compare(ops, dev, masks, area, mode, field)
            out2, info2 = ops.remove_small_regions(torch.from_numpy(masks).to(dev), area, MODES[mode])
            assert torch.equal(out, out2) and torch.equal(info, info2)
            print(f'{field} mode {mode} area {area}: changed {info[:, :2].sum(0).tolist()} of {masks.shape[0]}, status 0')


# ------------------------------------------------------------------------------------------------- the generator step
def _mc():
    import test_gpu_sam_multicrop as mc
    return mc


def speckled_disc_sam(*a, **kw):
    mc = _mc()

    class SpeckledDiscSam(mc.DiscSam):
        """DiscSam whose candidates carry defects, decided by the disc d a prompt point falls to: d % 4 == 0 -- a pinhole (one
        low-resolution logit at the disc's centre set to -32) in every candidate of d; 1 -- a detached speck (one logit far
        from the disc set to +32) in every candidate of d; 2 -- that speck only in the candidates of odd prompt points, so that
        the same disc also has clean candidates whose box the speckled ones share once cleaned; 3 -- untouched."""

        def crop_candidates(self, ci, npts):
            if (ci, npts) not in self.by_crop:
                low, iou, dis, grid = super().crop_candidates(ci, npts)
                low = low.clone()
                S = self.image_size
                x0, y0, x1, y1 = self.boxes[ci]
                ch, cw = y1 - y0, x1 - x0
                nh, nw = mc._shape((ch, cw), S)
                gh, gw = nh // 4, nw // 4                                            # low-resolution cells inside the resized crop
                cell = lambda X, o, c, n: ((X - o + 0.5) * (n / c) - 0.5 + 0.5) / 4 - 0.5   # noqa: E731
                spots = [(fy, fx) for fy in (gh // 5, gh - 1 - gh // 5) for fx in (gw // 5, gw - 1 - gw // 5)]
                for j in range(low.shape[0]):
                    d, pt = int(dis[j]), j // 3
                    kind = d % 4
                    cxl, cyl = cell(float(self.cx[d]), x0, cw, nw), cell(float(self.cy[d]), y0, ch, nh)
                    rl = float(self.rad[d]) * 0.85 * (nw / cw) / 4                   # the smallest of the three radii, in cells
                    if kind == 0:
                        ix, iy = int(round(cxl)), int(round(cyl))
                        if rl >= 2.5 and 0 <= ix < gw and 0 <= iy < gh:
                            low[j, iy, ix] = -32.0
                    elif kind == 1 or (kind == 2 and pt % 2 == 1):
                        fy, fx = max(spots, key=lambda s: (s[0] - cyl) ** 2 + (s[1] - cxl) ** 2)
                        if ((fy - cyl) ** 2 + (fx - cxl) ** 2) ** 0.5 > float(self.rad[d]) * 1.2 * (nw / cw) / 4 + 3:
                            low[j, fy, fx] = 32.0
                self.by_crop[(ci, npts)] = (low, iou, dis, grid)
            return self.by_crop[(ci, npts)]

    return SpeckledDiscSam(*a, **kw)


def oracle_region_step(o, cands, crop_boxes, hw, S, thr, area, nms_thr):
    """the generator step of the issue in numpy on top of oracle_multicrop's result: a new oracle dict (final list, boxes, run
    lengths after the second NMS) + per final instance `changed`, and the figures the conditions are asserted on"""
    from oracle import cops
    mc = _mc()
    ip = mc._hf_helpers()
    H, W = hw
    starts = np.cumsum([0] + [c[0].shape[0] for c in cands])
    final = o['final'].tolist()
    cleaned, boxes, ch_h, ch_i = [], [], [], []
    for f in final:
        ci = int(o['ci'][f])
        x0, y0, x1, y1 = crop_boxes[ci]
        val = mc._post_s(cands[ci][0][f - starts[ci]][None], S, mc._shape((y1 - y0, x1 - x0), S), (y1 - y0, x1 - x0))
        m = (val > thr)[0].numpy()
        m, a = ref_remove_small_regions(m, area, 'holes')
        m, b = ref_remove_small_regions(m, area, 'islands')
        bx = ref_box(m)
        cleaned.append(m); ch_h.append(a); ch_i.append(b)
        boxes.append([bx[0] + x0, bx[1] + y0, bx[2] + x0, bx[3] + y0])
    changed = np.array(ch_h) | np.array(ch_i)
    boxes = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    _, keep = cops.nms(boxes, torch.from_numpy(~changed).float(), nms_thr)
    keep = sorted(keep.tolist())                                                     # a stable filter of the previous order
    o2 = dict(o)
    o2['final'] = o['final'][keep]
    o2['box'] = o['box'].clone()
    o2['rle'], o2['near_thr'], o2['changed'] = [], [], []
    for i in keep:
        f, ci = final[i], int(o['ci'][final[i]])
        if changed[i]:
            o2['box'][f] = boxes[i]
        o2['rle'].append(ip._mask_to_rle(ip._pad_masks(torch.from_numpy(cleaned[i])[None], crop_boxes[ci], H, W))[0])
        o2['near_thr'].append(o['near_thr'][i])
        o2['changed'].append(bool(changed[i]))
    kept = np.zeros(len(final), dtype=bool)
    kept[keep] = True
    ch_h, ch_i = np.array(ch_h), np.array(ch_i)
    crops = np.array([int(o['ci'][f]) for f in final])
    o2['figures'] = dict(survivors=len(final), kept=len(keep), kept_changed_by_holes=int((kept & ch_h).sum()),
                         kept_changed_by_islands=int((kept & ch_i).sum()), kept_unchanged=int((kept & ~changed).sum()),
                         removed_by_second_nms=int((~kept).sum()), changed_outside_crop0=int((kept & changed & (crops != 0)).sum()),
                         near_thr=int(np.sum(o2['near_thr'])))
    print('region step:', o2['figures'])
    return o2


def assert_region_conditions(o2):
    f = o2['figures']
    assert f['kept_changed_by_holes'] >= 1 and f['kept_changed_by_islands'] >= 1 and f['kept_unchanged'] >= 1
    assert f['removed_by_second_nms'] >= 1 and f['changed_outside_crop0'] >= 1


def region_case_oracle(hw, S, layers, n, ndisc, area, down=1, rad_scale=1.0, t_iou=0.88, t_st=0.8, ops=None, dev=None):
    mc = _mc()
    ip = mc._hf_helpers()
    image = mc._test_image(hw)
    crop_boxes, layer_idxs = ip._generate_per_layer_crops(layers, 512 / 1500, hw)
    sam = speckled_disc_sam(ops, dev, S, image, crop_boxes, ndisc, rad_scale)
    cands = [sam.crop_candidates(ci, int(n / down ** layer_idxs[ci]))[:2] for ci in range(len(crop_boxes))]
    o = mc.oracle_multicrop(cands, crop_boxes, hw, S, t_iou, t_st, 0.0, 1.0, 0.7)
    assert float(o['und'].float().mean()) <= 0.03
    o2 = oracle_region_step(o, cands, crop_boxes, hw, S, 0.0, area, 0.7)
    assert_region_conditions(o2)
    return sam, image, crop_boxes, o, o2


def run_region_case(ops, dev, hw, S, layers, n, ndisc, area, down=1, rad_scale=1.0, t_iou=0.88, t_st=0.8, crop_batch=2,
                    zero_area=True):
    """the speckled scene through SamMaskGenerator(min_mask_region_area=area), rle and dense, against the oracle"""
    from rsprompter_amd.apis import SamMaskGenerator
    mc = _mc()
    sam, image, crop_boxes, o, o2 = region_case_oracle(hw, S, layers, n, ndisc, area, down, rad_scale, t_iou, t_st, ops, dev)
    kw = dict(points_per_side=n, pred_iou_thresh=t_iou, stability_score_thresh=t_st, stability_score_offset=1.0, mask_threshold=0.0,
              crops_nms_thresh=0.7, crop_n_layers=layers, crop_n_points_downscale_factor=down, crop_batch=crop_batch)
    st = {}
    res = SamMaskGenerator(sam, min_mask_region_area=area, **kw).generate(image.numpy(), _stages=st)
    sam2 = speckled_disc_sam(ops, dev, S, image, crop_boxes, ndisc, rad_scale)
    sam2.by_crop = sam.by_crop
    dense = SamMaskGenerator(sam2, output='dense', min_mask_region_area=area, **dict(kw, crop_batch=3)).generate(image)
    decided = torch.equal(torch.zeros(o['K'], dtype=torch.bool).index_fill_(0, st['kept'].cpu(), True), o['keep'])
    if decided:
        assert st['final'].cpu().tolist() == o2['final'].tolist()                     # the kept subset, in the previous order
    mc.compare_with_oracle(res, st, o2, hw, dense)
    assert res.region_changed.dtype == torch.bool and tuple(res.region_changed.shape) == (len(res.masks),)
    assert torch.equal(dense.region_changed, res.region_changed) and torch.equal(dense.scores, res.scores)
    if decided:
        assert res.region_changed.cpu().tolist() == o2['changed']
        # compare_with_oracle compared boxes, scores, crops and run lengths exactly, except the run lengths of a mask with a
        # pixel within 1e-4 of the threshold (fp32 resize on two machines); say how many of the changed ones were exact
        n_exact = sum(1 for i, c in enumerate(o2['changed']) if c and not o2['near_thr'][i] and res.masks[i] == o2['rle'][i])
        assert n_exact == sum(1 for i, c in enumerate(o2['changed']) if c and not o2['near_thr'][i]) and n_exact >= 3
    if not zero_area:
        return o2, res
    # min_mask_region_area = 0 is the generator without the argument, bit for bit
    sams = [speckled_disc_sam(ops, dev, S, image, crop_boxes, ndisc, rad_scale) for _ in range(2)]
    for s_ in sams:
        s_.by_crop = sam.by_crop
    a = SamMaskGenerator(sams[0], **kw).generate(image)
    b = SamMaskGenerator(sams[1], min_mask_region_area=0, **kw).generate(image)
    assert torch.equal(a.bboxes, b.bboxes) and torch.equal(a.scores, b.scores) and torch.equal(a.crop_index, b.crop_index)
    assert a.masks == b.masks and 'region_changed' not in b and len(a.masks) == o2['figures']['survivors']
    return o2, res


REGION_CASES = {'600x900_one_layer': dict(hw=(600, 900), S=256, layers=1, n=8, ndisc=40, area=500),
                '517x803_two_layers': dict(hw=(517, 803), S=256, layers=2, n=8, ndisc=40, area=500, down=2, crop_batch=5)}


@pytest.mark.parametrize('case', sorted(REGION_CASES))
def test_generator_removes_small_regions(dev, case):
    from rsprompter_amd import ops
    run_region_case(ops, dev, **REGION_CASES[case])


def check_generate_masks_is_the_one_crop_generator(ops, dev, hw, S, n, ndisc, area, rad_scale=1.0, t_st=0.8):
    from rsprompter_amd.apis import SamMaskGenerator, generate_masks
    mc = _mc()
    image = mc._test_image(hw)
    box = [[0, 0, hw[1], hw[0]]]
    kw = dict(points_per_side=n, pred_iou_thresh=0.88, stability_score_thresh=t_st, min_mask_region_area=area)
    for output in ('rle', 'dense'):
        a = SamMaskGenerator(speckled_disc_sam(ops, dev, S, image, box, ndisc, rad_scale), crop_n_layers=0, output=output, **kw).generate(image)
        w = generate_masks(speckled_disc_sam(ops, dev, S, image, box, ndisc, rad_scale), image, output=output, **kw)
        assert torch.equal(a.bboxes, w.bboxes) and torch.equal(a.scores, w.scores) and w.bboxes.shape[0] > 1
        assert torch.equal(a.region_changed, w.region_changed) and bool(w.region_changed.any()) and not bool(w.region_changed.all())
        assert (a.masks == w.masks) if output == 'rle' else torch.equal(a.masks, w.masks)
    with pytest.raises(ValueError):
        generate_masks(speckled_disc_sam(ops, dev, S, image, box, ndisc), image, min_mask_region_area=-1)
    with pytest.raises(ValueError):
        SamMaskGenerator(speckled_disc_sam(ops, dev, S, image, box, ndisc), min_mask_region_area=-5)


def test_generate_masks_is_the_one_crop_generator(dev):
    from rsprompter_amd import ops
    check_generate_masks_is_the_one_crop_generator(ops, dev, (600, 900), 256, 8, 40, 500)


def check_apis_remove_small_regions(ops, dev):
    from rsprompter_amd import apis
    masks = smooth_noise((70, 83), 8, k=3)
    want, winfo = ref_regions(masks, 20, 3)
    out, changed = apis.remove_small_regions(torch.from_numpy(masks).to(dev), 20)
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and changed.cpu().tolist() == [bool(a or b) for a, b in winfo[:, :2]]
    one, ch = apis.remove_small_regions(torch.from_numpy(masks[1]).to(dev), 20, 'islands')
    w1, c1 = ref_remove_small_regions(masks[1], 20, 'islands')
    assert tuple(one.shape) == (70, 83) and torch.equal(one.cpu(), torch.from_numpy(w1)) and ch is c1


@pytest.mark.quick
def test_apis_remove_small_regions(dev):
    from rsprompter_amd import ops
    check_apis_remove_small_regions(ops, dev)
