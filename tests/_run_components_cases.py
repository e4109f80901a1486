"""Bodies of the run-domain component tests (csrc/run_components.hip, ops.rle_components / components_select /
components_union / rle_complement, rle.runs_components / split_runs / clean_runs, apis.remove_small_regions on RLE dicts,
apis.masks_to_obb(per_component=True), apis.mask_components, large_image min_mask_region_area), shared by both
tiers: tests/test_run_components_cpu.py calls them with the emulated `ops` on CPU tensors, tests/test_gpu_run_components.py with
the real ones on cuda:0.  The reference is tests/_run_components_ref.py, a flood fill over the dense mask; every integer array is
compared with torch.equal and every output table bit for bit with the numpy encoder's counts of the reference's dense answer
(tests/_large_image_ref.py rle_counts_np).  The input tables come from that encoder or are written by hand."""
import numpy as np
import torch

import _large_image_ref as lref
import _mask_obb_cases as ocases
import _mask_obb_ref as oref
import _mask_polygons_cases as pcases
import _run_components_ref as cref
import _seam_merge_cases as seam_cases

NAMES = ('comp_offs', 'piece_comp', 'comp_area', 'comp_box', 'comp_first', 'comp_inst', 'pieces', 'piece_offs')
THREADS = 256                   # RC_THREADS: the lanes of a block, the runs of one chunk of the walk, the components of one
#                                 stride of the selection
AREAS = (1, 2, 5, 100)
MODES = ('holes', 'islands', 'both')


# ----------------------------------------------------------------------------------------------------------- the masks
def _pix(h, w, pixels):
    m = np.zeros((h, w), bool)
    for x, y in pixels:
        m[y, x] = True
    return m


def hand_checked():
    """(name, mask, [(area, box, first)] in component order) worked out by hand"""
    far = np.zeros((40, 60), bool)
    far[2:5, 1:4] = True
    far[30:38, 50:59] = True
    return [
        ('one pixel', _pix(3, 3, [(1, 1)]), [(1, (1, 1, 2, 2), 4)]),
        ('two pixels diagonal across a column boundary', _pix(3, 3, [(0, 0), (1, 1)]), [(2, (0, 0, 2, 2), 0)]),
        ('the same with a one-row gap', _pix(4, 3, [(0, 0), (1, 2)]), [(1, (0, 0, 1, 1), 0), (1, (1, 2, 2, 3), 7)]),
        ('an L', _pix(4, 3, [(0, 0), (0, 1), (0, 2), (1, 2), (2, 2)]), [(5, (0, 0, 3, 3), 0)]),
        ('two far blocks', far, [(9, (1, 2, 4, 5), 121), (72, (50, 30, 59, 38), 1850)]),
        # ONE ones-run over the bottom of column 0 and the top of column 1
        ('H = 3: two components inside one run', _pix(3, 3, [(0, 2), (1, 0)]), [(1, (0, 2, 1, 3), 6), (1, (1, 0, 2, 1), 1)]),
        ('H = 4: two components inside one run', _pix(4, 4, [(0, 2), (0, 3), (1, 0)]), [(2, (0, 2, 1, 4), 8), (1, (1, 0, 2, 1), 1)]),
        ('H = 2: one component', _pix(2, 3, [(0, 1), (1, 0)]), [(2, (0, 0, 2, 2), 1)]),
    ]


def column_end_masks():
    out = [('H = 1', np.array([[0, 1, 1, 0, 1, 0]], bool)), ('H = 1 full', np.ones((1, 5), bool)),
           ('W = 1', np.array([[0], [1], [0], [1]], bool)), ('1 x 1', np.ones((1, 1), bool)), ('1 x 1 clear', np.zeros((1, 1), bool)),
           ('full canvas', np.ones((7, 5), bool))]
    m = np.zeros((6, 9), bool)
    m[4:, 1] = True
    m[:, 2:7] = True
    m[:2, 7] = True
    out.append(('a run over several full columns', m))
    return out


def propagation_masks():
    out = []
    m = np.zeros((9, 12), bool)
    m[::2, :] = True
    m[:, -1] = True
    out.append(('comb joined in the last column', m))
    out.append(('serpentine 64 x 64', serpentine(64)))
    out.append(('spiral', pcases.arm_spiral(33)))
    m = np.zeros((9, 20), bool)
    m[0, :] = m[8, :] = True
    m[:, -1] = True
    out.append(('a U that closes late', m))
    out.append(('checkerboard', np.add.outer(np.arange(16), np.arange(16)) % 2 == 0))
    m = np.zeros((64, 3), bool)
    m[:, 1] = True
    m[::2, 2] = True
    m[1::2, 0] = True
    out.append(('a full column beside alternating pixels', m))
    return out


def serpentine(n):
    """every second column full, joined alternately at the bottom and at the top: ONE component whose label travels through
    every column"""
    m = np.zeros((n, n), bool)
    m[:, ::2] = True
    for x in range(1, n, 2):
        m[0 if (x // 2) % 2 else n - 1, x] = True
    return m


def noise_masks():
    rng = np.random.default_rng(1410)
    out = []
    for d in (0.02, 0.1, 0.5, 0.9):
        m = rng.random((64, 64)) < d
        out += [(f'noise 64 x 64 at {d}', m), (f'noise 64 x 64 at {d}, complement', ~m)]
    return out


def boundary_masks():
    """piece counts of one instance, and of one column pair, around a block of lanes / a chunk of the walk"""
    out = []
    for npieces in (THREADS - 1, THREADS, THREADS + 1, 2 * THREADS - 1, 2 * THREADS, 2 * THREADS + 1):
        m = np.zeros((3, npieces), bool)
        m[1, :] = True
        m[2, ::7] = True
        out.append((f'{npieces} pieces in a row', m))
    for npieces in (THREADS - 1, THREADS, THREADS + 1):
        m = np.zeros((2 * (npieces - 1), 2), bool)
        m[::2, 0] = True                                    # npieces - 1 pieces beside one full column
        m[:, 1] = True
        out.append((f'{npieces} pieces in one column pair', m))
        iso = np.zeros((2 * npieces, 3), bool)
        iso[::2, 1] = True                                  # as many components as pieces: the selection's stride
        out.append((f'{npieces} single-pixel components', iso))
    return out


def small_cases():
    return [(nm, m) for nm, m, _ in hand_checked()] + column_end_masks() + propagation_masks() + noise_masks()


def all_cases():
    return small_cases() + pcases.named_masks()


# -------------------------------------------------------------------------------------------------------------- helpers
def want_arrays(masks, H, W):
    """the eight arrays of ops.rle_components for masks (None: an empty row) on one canvas, from the reference"""
    offs, pcomp, area, box, first, inst, pcs, poffs = [0], [], [], [], [], [], [], [0]
    for i, m in enumerate(masks):
        if m is not None:
            assert m.shape == (H, W)
            labels, comps = cref.check(m)
            base = len(area)
            for x, y0, y1 in cref.pieces(m):
                pcs.append((x, y0, y1, i))
                pcomp.append(base + int(labels[y0, x]))
            area += [d['area'] for d in comps]
            box += [d['box'] for d in comps]
            first += [d['first'] for d in comps]
            inst += [i] * len(comps)
        offs.append(len(area))
        poffs.append(len(pcs))
    return (np.array(offs, np.int64), np.array(pcomp, np.int32), np.array(area, np.int32), np.array(box, np.int32).reshape(-1, 4),
            np.array(first, np.int32), np.array(inst, np.int32), np.array(pcs, np.int32).reshape(-1, 4).T.copy(),
            np.array(poffs, np.int64))


def assert_components(got, want, what=''):
    assert int(got.status.cpu()[0]) == 0, what
    for name, w in zip(NAMES, want):
        g, w = getattr(got, name), torch.from_numpy(np.ascontiguousarray(w))
        assert g.dtype == w.dtype, f'{what}: {name} is {g.dtype}, expected {w.dtype}'
        assert tuple(g.shape) == tuple(w.shape), f'{what}: {name} has shape {tuple(g.shape)}, expected {tuple(w.shape)}'
        assert torch.equal(g.cpu(), w), f'{what}: {name} differs: {g.cpu().tolist()[:16]} != {w.tolist()[:16]}'


def same_components(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def run(ops, dev, masks, H, W):
    counts, n = seam_cases.rows_from_masks(masks, dev)
    return ops.rle_components(counts, n, H, W)


def assert_table(counts, n, masks, what=''):
    """an output run table against the dense answers: n and every row bit for bit with the numpy encoder's counts (None: an
    empty row, n = 0)"""
    rows = [[] if m is None else lref.rle_counts_np(m) for m in masks]
    assert n.dtype == torch.int32 and counts.dtype == torch.int32
    assert n.cpu().tolist() == [len(r) for r in rows], f'{what}: n {n.cpu().tolist()[:12]} != {[len(r) for r in rows][:12]}'
    c = counts.cpu()
    for i, r in enumerate(rows):
        assert c[i, :len(r)].tolist() == [int(v) for v in r], f'{what}: row {i} differs'


def batch_on_canvas(cases, H, W, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for _, m in cases:
        ox, oy = int(rng.integers(0, W - m.shape[1] + 1)), int(rng.integers(0, H - m.shape[0] + 1))
        out.append(pcases.embed(m, H, W, ox, oy))
    return out


# -------------------------------------------------------------------------------------------------------------- kernels
def check_hand_checked(ops, dev):
    for name, m, comps in hand_checked():
        H, W = m.shape
        got = run(ops, dev, [m], H, W)
        assert got.comp_offs.cpu().tolist() == [0, len(comps)], name
        assert got.comp_area.cpu().tolist() == [c[0] for c in comps], name
        assert [tuple(b) for b in got.comp_box.cpu().tolist()] == [c[1] for c in comps], name
        assert got.comp_first.cpu().tolist() == [c[2] for c in comps], name
        assert_components(got, want_arrays([m], H, W), name)
    counts, n = seam_cases.rows_from_counts([[2, 2, 5]], dev)                     # the H = 3 case is ONE ones-run
    assert int(ops.rle_components(counts, n, 3, 3).comp_area.shape[0]) == 2


def check_single_masks(ops, dev, cases=None):
    """every case mask alone (k = 1) on its own canvas"""
    for name, m in (all_cases() if cases is None else cases):
        H, W = m.shape
        got = run(ops, dev, [m], H, W)
        assert_components(got, want_arrays([m], H, W), name)
        assert all(g.device.type == torch.device(dev).type for g in got)


def check_h1_columns(ops, dev):
    """H = 1: two pixels are connected iff their columns are consecutive"""
    for row, want in (([1, 1, 0, 1], 2), ([1, 0, 1, 0, 1], 3), ([1, 1, 1, 1], 1), ([0, 0, 0], 0)):
        m = np.array([row], bool)
        got = run(ops, dev, [m], 1, len(row))
        assert int(got.comp_area.shape[0]) == want
        assert_components(got, want_arrays([m], 1, len(row)), str(row))


def check_block_boundaries(ops, dev):
    for name, m in boundary_masks():
        H, W = m.shape
        got = run(ops, dev, [m], H, W)
        assert_components(got, want_arrays([m], H, W), name)
    return [int(m.shape[0]) for _, m in boundary_masks()]


def check_batch(ops, dev):
    """every case mask on one canvas, with rows of n = 0, n < 0 and n beyond cap among them, launched twice; then k = 0"""
    H, W = 66, 70
    masks = batch_on_canvas(all_cases(), H, W)
    rows = [lref.rle_counts_np(m) for m in masks]
    cap = max(len(r) for r in rows)
    widest = max(range(len(rows)), key=lambda i: len(rows[i]))
    counts, n = seam_cases.rows_from_counts(rows, 'cpu', cap)
    order = list(range(len(rows)))
    order.insert(3, 'zero')
    order.insert(11, 'negative')
    order.insert(len(rows) // 2, 'beyond')
    out_c = torch.zeros((len(order), cap), dtype=torch.int32)
    out_n = torch.zeros((len(order),), dtype=torch.int32)
    want_masks = []
    for j, o in enumerate(order):
        if o == 'zero':
            out_c[j] = counts[0]
            want_masks.append(None)
        elif o == 'negative':
            out_c[j], out_n[j] = counts[1], -(cap + 5)
            want_masks.append(None)
        elif o == 'beyond':
            out_c[j], out_n[j] = counts[widest], cap + 7
            want_masks.append(masks[widest])
        else:
            out_c[j], out_n[j] = counts[o], n[o]
            want_masks.append(masks[o])
    got = ops.rle_components(out_c.to(dev), out_n.to(dev), H, W)
    assert_components(got, want_arrays(want_masks, H, W), 'batch')
    assert same_components(got, ops.rle_components(out_c.to(dev), out_n.to(dev), H, W))      # a second launch: the same bits
    z = ops.rle_components(torch.zeros((0, 4), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev), 5, 6)
    assert_components(z, want_arrays([], 5, 6), 'k = 0')
    e = run(ops, dev, [np.zeros((4, 3), bool), None, np.zeros((4, 3), bool)], 4, 3)
    assert_components(e, want_arrays([np.zeros((4, 3), bool), None, np.zeros((4, 3), bool)], 4, 3), 'empty masks')
    return out_c, out_n, want_masks, (H, W)


def check_shifted_and_joined_tables(ops, rle, dev):
    """the tables rsp_rle_shift and rsp_rle_union write are input as well"""
    rng = np.random.default_rng(2)
    tiles = [rng.random((9, 8)) < d for d in (0.3, 0.6, 1.0, 0.0)]
    counts, n = seam_cases.rows_from_masks(tiles, dev)
    offs = torch.tensor([[3, 2], [0, 0], [12, 11], [5, 5]], dtype=torch.int32, device=dev)
    H, W = 20, 20
    sc, sn, _, _ = rle.shift_runs(counts, n, offs, (9, 8), (H, W))
    placed = [pcases.embed(m, H, W, o[0], o[1]) for m, o in zip(tiles, offs.cpu().tolist())]
    assert_components(rle.runs_components(sc, sn, (H, W)), want_arrays(placed, H, W), 'shifted')
    uc, un, _, _ = rle.union_runs(sc, sn, (H, W), torch.tensor([0, 2, 4], dtype=torch.int32, device=dev),
                                  torch.arange(4, dtype=torch.int32, device=dev))
    joined = [placed[0] | placed[1], placed[2] | placed[3]]
    assert_components(rle.runs_components(uc, un, (H, W)), want_arrays(joined, H, W), 'union')
    for mode in MODES:                                      # ... and the cleaned union is the reference's
        c, m, _, _, ch = rle.clean_runs(uc, un, (H, W), 3, mode)
        want = [cref.remove_small_regions(j, 3, mode) for j in joined]
        assert_table(c, m, [w[0] for w in want], f'union, {mode}')
        assert ch.cpu().tolist() == [[int(w[1]), int(w[2])] for w in want]


# ------------------------------------------------------------------------------------------------------ split and clean
def split_masks(masks):
    """the reference's one mask per component, in component order, and comp_offs"""
    out, offs = [], [0]
    for m in masks:
        if m is not None:
            labels, comps = cref.check(m)
            out += [labels == c for c in range(len(comps))]
        offs.append(len(out))
    return out, offs


def check_split(ops, rle, dev):
    H, W = 66, 70
    masks = batch_on_canvas(small_cases(), H, W, seed=4) + [None]
    counts, n = seam_cases.rows_from_masks(masks, dev)
    want, offs = split_masks(masks)
    c, m, n_host, cap, comp_offs = rle.split_runs(counts, n, (H, W))
    assert comp_offs.cpu().tolist() == offs and c.shape[0] == len(want) and n_host.tolist() == m.cpu().tolist()
    assert_table(c, m, want, 'split')
    # a row holding one component comes back bit for bit
    one = [i for i in range(len(masks) - 1) if offs[i + 1] - offs[i] == 1]
    assert len(one) >= 8
    for i in one:
        ni = int(n[i])
        assert int(m[offs[i]]) == ni and torch.equal(c[offs[i], :ni], counts[i, :ni])
    # the H = 3 run gives two rows; a first capacity that is too small goes through the retry
    hc, hn = seam_cases.rows_from_counts([[2, 2, 5]], dev)
    sc, sn, _, _, so = rle.split_runs(hc, hn, (3, 3))
    assert so.cpu().tolist() == [0, 2] and sn.cpu().tolist() == [3, 3]
    assert sc[0, :3].cpu().tolist() == [2, 1, 6] and sc[1, :3].cpu().tolist() == [3, 1, 5]
    comps = rle.runs_components(counts, n, (H, W))
    calls = []
    real = ops.components_union

    def counting(*a, **k):
        calls.append(a[3])
        return real(*a, **k)
    ops.components_union = counting
    try:
        c2, m2, _, cap2, _ = rle.split_runs(counts, n, (H, W), comps=comps, cap=2)
    finally:
        ops.components_union = real
    assert len(calls) >= 2 and calls[0] == 2 and calls[-1] == cap2 >= int(m.max())
    assert torch.equal(m2, m) and all(torch.equal(c2[i, :int(m[i])], c[i, :int(m[i])]) for i in range(len(want)))
    # no rows, no components
    z = rle.split_runs(torch.zeros((0, 4), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev), (5, 6))
    assert z[0].shape[0] == 0 and z[1].shape[0] == 0 and z[4].cpu().tolist() == [0]
    ec, en = seam_cases.rows_from_masks([np.zeros((4, 3), bool), None], dev)
    e = rle.split_runs(ec, en, (4, 3))
    assert e[0].shape[0] == 0 and e[4].cpu().tolist() == [0, 0, 0]


def want_clean(masks, min_area, mode):
    out, flags = [], []
    for m in masks:
        if m is None:
            out.append(None)
            flags.append([0, 0])
        else:
            w, ch, cs = cref.remove_small_regions(m, min_area, mode)
            out.append(w)
            flags.append([int(ch), int(cs)])
    return out, flags


def check_clean_modes(ops, rle, dev, areas=AREAS):
    """every mode at every min_area on the case masks, batched on one canvas with an empty and an overlong row"""
    H, W = 66, 70
    masks = batch_on_canvas(small_cases(), H, W, seed=5)
    widest = max(masks, key=lambda m: len(lref.rle_counts_np(m)))
    masks = masks + [None, widest]
    counts, n = seam_cases.rows_from_masks(masks, dev)
    n[-1] += 9                                              # beyond cap: read up to cap, which is this row's length
    n[-2] = -4
    seen = set()
    for mode in MODES:
        for a in areas:
            want, flags = want_clean(masks, a, mode)
            c, m, n_host, cap, ch = rle.clean_runs(counts, n, (H, W), a, mode)
            assert_table(c, m, want, f'{mode} at {a}')
            assert ch.dtype == torch.int32 and ch.cpu().tolist() == flags, f'{mode} at {a}'
            assert n_host.tolist() == m.cpu().tolist() and cap == c.shape[1]
            seen |= {tuple(f) for f in flags}
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def check_clean_edge_cases(ops, rle, dev):
    # all islands small: the tie goes to the lowest ROW-MAJOR first pixel, which is not the first in stream order
    m = _pix(7, 5, [(0, 5), (3, 1)])
    counts, n = seam_cases.rows_from_masks([m], dev)
    c, k, _, _, ch = rle.clean_runs(counts, n, (7, 5), 2, 'islands')
    assert_table(c, k, [_pix(7, 5, [(3, 1)])], 'tie')
    assert ch.cpu().tolist() == [[0, 1]] and cref.remove_small_regions(m, 2, 'islands')[0][1, 3]
    # the H = 3 run: islands keeps one piece of the run and drops the other, so the output run is cut
    hc, hn = seam_cases.rows_from_counts([[2, 2, 5]], dev)                       # both pieces are one pixel: (1, 0) stays
    c, k, _, _, ch = rle.clean_runs(hc, hn, (3, 3), 2, 'islands')
    assert k.cpu().tolist() == [3] and c[0, :3].cpu().tolist() == [3, 1, 5] and ch.cpu().tolist() == [[0, 1]]
    hc, hn = seam_cases.rows_from_counts([[2, 3, 11]], dev)                      # H = 4: two pixels below, one above
    c, k, _, _, ch = rle.clean_runs(hc, hn, (4, 4), 2, 'islands')
    assert k.cpu().tolist() == [3] and c[0, :3].cpu().tolist() == [2, 2, 12] and ch.cpu().tolist() == [[0, 1]]
    # a hole that touches the border only diagonally belongs to the outer background
    m = np.ones((5, 5), bool)
    m[0, 0] = m[1, 1] = False
    m[3, 3] = False
    counts, n = seam_cases.rows_from_masks([m], dev)
    for a, filled in ((2, [(3, 3)]), (3, [(3, 3), (0, 0), (1, 1)])):
        c, k, _, _, ch = rle.clean_runs(counts, n, (5, 5), a, 'holes')
        want = m.copy()
        for x, y in filled:
            want[y, x] = True
        assert (cref.remove_small_regions(m, a, 'holes')[0] == want).all()
        assert_table(c, k, [want], f'diagonal hole at {a}')
    # the small-background case: on a 3 x 3 canvas the background itself is a small hole
    masks = [np.zeros((3, 3), bool), _pix(3, 3, [(1, 1)]), None, np.ones((3, 3), bool)]
    counts, n = seam_cases.rows_from_masks(masks, dev)
    n[2] = -7
    for mode, want, flags in (('holes', [np.ones((3, 3), bool)] * 2 + [None, np.ones((3, 3), bool)], [[1, 0], [1, 0], [0, 0], [0, 0]]),
                              ('islands', [masks[0], masks[1], None, masks[3]], [[0, 0], [0, 1], [0, 0], [0, 1]]),
                              ('both', [np.ones((3, 3), bool)] * 2 + [None, np.ones((3, 3), bool)], [[1, 1], [1, 1], [0, 0], [0, 1]])):
        ref_masks, ref_flags = want_clean(masks, 100, mode)                     # the hand-made answer is the reference's
        assert ref_flags == flags and all((a is None and b is None) or (a == b).all() for a, b in zip(ref_masks, want))
        c, k, _, _, ch = rle.clean_runs(counts, n, (3, 3), 100, mode)
        assert_table(c, k, want, f'small background, {mode}')
        assert ch.cpu().tolist() == flags, mode
    # min_area = 0: the same objects, no launch
    out = rle.clean_runs(counts, n, (3, 3), 0)
    assert out[0] is counts and out[1] is n and out[4].cpu().tolist() == [[0, 0]] * 4
    # a first capacity that is too small goes through the retry
    H, W = 66, 70
    big = batch_on_canvas(noise_masks()[:4], H, W, seed=6)
    counts, n = seam_cases.rows_from_masks(big, dev)
    a = rle.clean_runs(counts, n, (H, W), 3, 'both')
    b = rle.clean_runs(counts, n, (H, W), 3, 'both', cap=2)
    assert torch.equal(a[1], b[1]) and all(torch.equal(a[0][i, :int(a[1][i])], b[0][i, :int(a[1][i])]) for i in range(len(big)))
    assert torch.equal(a[4], b[4]) and int(a[1].max()) > 2
    assert_table(a[0], a[1], want_clean(big, 3, 'both')[0], 'retry')


def check_status_and_refusals(ops, rle, dev, pytest):
    ops.check_components_status([0])
    ops.check_components_status(torch.zeros((1,), dtype=torch.int32))
    with pytest.raises(RuntimeError, match='iteration cap'):
        ops.check_components_status(torch.tensor([1], dtype=torch.int32))
    counts, n = seam_cases.rows_from_counts([[4]], dev)
    with pytest.raises(ValueError, match='32-bit'):
        ops.rle_components(counts, n, 65536, 32768)
    with pytest.raises(ValueError, match='int32'):
        ops.rle_components(counts.to(torch.int64), n, 2, 2)
    with pytest.raises(ValueError, match='empty'):
        ops.rle_components(counts, n, 0, 4)
    with pytest.raises(ValueError, match='mode'):
        rle.clean_runs(counts, n, (2, 2), 3, 'specks')
    for bad in (-1, 1.5, 2 ** 31, True):
        with pytest.raises(ValueError, match='min_area'):
            rle.clean_runs(counts, n, (2, 2), bad)
    comps = ops.rle_components(counts, n, 2, 2)
    with pytest.raises(ValueError, match='cap_out'):
        ops.components_union(comps, 2, 2, 1)
    with pytest.raises(ValueError, match='changed'):
        ops.components_select(comps, 1, True, 0, torch.zeros((1, 3), dtype=torch.int32, device=dev))
    C = ops.CONST
    lim = C['RSP_RUN_COMPONENTS_MAX_PIECES']
    assert ops.RUN_COMPONENTS_MAX_PIECES == lim and type(ops.RUN_COMPONENTS_MAX_PIECES) is int
    lib = ops._lib.load()
    OK, EINVAL = C['RSP_OK'], C['RSP_EINVAL']
    assert lib.rsp_abi_version() == C['RSP_ABI_VERSION']
    assert lib.rsp_run_components_workspace_bytes(2, 2, lim) == 4 * lim and lib.rsp_run_components_workspace_bytes(2, 2, lim + 1) == -1
    assert lib.rsp_run_components_workspace_bytes(2, 2, 0) == 4 and lib.rsp_run_components_workspace_bytes(2, 2, -1) == -1
    assert lib.rsp_run_components_workspace_bytes(46341, 46341, 1) == -1 and lib.rsp_run_components_workspace_bytes(46340, 46341, 1) == 4
    assert lib.rsp_run_components_workspace_bytes(0, 4, 1) == -1
    p = torch.zeros((64,), dtype=torch.int64, device=dev).data_ptr()
    # a call without instances touches no array, so it is legal at the limit itself
    assert lib.rsp_run_components_label(0, 2, 2, p, lim, p, p, p, p, p, 0) == OK
    assert lib.rsp_run_components_label(0, 2, 2, p, lim + 1, p, p, p, p, p, 0) == EINVAL
    assert lib.rsp_run_components_label(0, 46341, 46341, p, 1, p, p, p, p, p, 0) == EINVAL
    assert lib.rsp_run_components_label(0, 46340, 46341, p, 1, p, p, p, p, p, 0) == OK
    # the table's writer took the run table over, and with it the refusal of a missing one and of a capacity below 1
    assert lib.rsp_run_pieces(0, p, 1, 4, 2, 2, p, 1, p, 0) == EINVAL
    assert lib.rsp_run_pieces(p, p, 1, 0, 2, 2, p, 1, p, 0) == EINVAL
    assert lib.rsp_run_components_label(1, 2, 2, p, 1, 0, p, p, p, p, 0) == EINVAL
    assert lib.rsp_run_components_label(1, 2, 2, p, 1, p, 0, p, p, p, 0) == EINVAL
    assert lib.rsp_run_components_stats(p, 0, 2, 2, p, p, p, 0, p, p, p, p, p, 0) == OK
    assert lib.rsp_run_components_stats(p, lim + 1, 2, 2, p, p, p, 0, p, p, p, p, p, 0) == EINVAL
    assert lib.rsp_run_components_stats(p, 1, 2, 2, p, p, p, 2, p, p, p, p, p, 0) == EINVAL          # more components than pieces
    assert lib.rsp_run_components_stats(p, 1, 2, 2, p, 0, p, 1, p, p, p, p, p, 0) == EINVAL
    assert lib.rsp_run_components_select(p, 0, lim, p, p, 1, 1, 0, p, p, 0) == OK
    assert lib.rsp_run_components_select(p, 0, lim + 1, p, p, 1, 1, 0, p, p, 0) == EINVAL
    assert lib.rsp_run_components_select(p, 1, 0, p, p, -1, 1, 0, p, p, 0) == EINVAL
    assert lib.rsp_run_components_select(p, 1, 0, p, p, 1, 1, 2, p, p, 0) == EINVAL
    assert lib.rsp_run_components_select(p, 1, 0, p, p, 1, 1, 0, p, 0, 0) == EINVAL


# ------------------------------------------------------------------------------------------------------------------ API
def api_masks():
    cases = dict(all_cases())
    names = ('two far blocks', 'comb', 'nested frames', 'noise 64 x 64 at 0.1', 'H = 3: two components inside one run',
             'frame with a diagonal-touching island in its hole', 'checkerboard')
    H, W = 66, 67
    return H, W, [pcases.embed(cases[nm], H, W, 1, 2) for nm in names] + [np.zeros((H, W), bool)]


def _forms(rle, masks, H, W, dev):
    dense = torch.from_numpy(np.stack(masks)).to(dev)
    lists = [dict(size=[H, W], counts=[int(v) for v in lref.rle_counts_np(m)]) for m in masks]
    strings = [dict(size=[H, W], counts=rle.counts_to_string([int(v) for v in lref.rle_counts_np(m)])) for m in masks]
    return dense, lists, strings


def check_api_remove_small_regions(apis, rle, dev):
    from rsprompter_amd import datasets
    H, W, masks = api_masks()
    _, lists, strings = _forms(rle, masks, H, W, dev)
    for mode, a in (('both', 5), ('islands', 2), ('holes', 100)):
        want, flags = want_clean(masks, a, mode)
        out, changed = apis.remove_small_regions(lists, a, mode, device=dev)
        assert [d['size'] for d in out] == [[H, W]] * len(masks) and all(isinstance(d['counts'], list) for d in out)
        assert [d['counts'] for d in out] == [[int(v) for v in lref.rle_counts_np(w)] for w in want]
        assert changed.dtype == torch.bool and changed.tolist() == [bool(f[0] or f[1]) for f in flags]
        for src in (strings, [dict(d, counts=d['counts'].decode()) for d in strings]):
            out, ch2 = apis.remove_small_regions(src, a, mode, device=dev)
            assert all(isinstance(d['counts'], bytes) for d in out) and ch2.tolist() == changed.tolist()
            assert [list(datasets.rle_from_string(d['counts'])) for d in out] == [[int(v) for v in lref.rle_counts_np(w)] for w in want]
    assert any(changed.tolist())


def check_api_refusals(apis, dev, pytest):
    with pytest.raises(ValueError, match='canonical'):
        apis.remove_small_regions([dict(size=[2, 2], counts=[2, 1, 0, 1])], 3, device=dev)
    with pytest.raises(ValueError, match='share one size'):
        apis.remove_small_regions([dict(size=[2, 2], counts=[4]), dict(size=[2, 3], counts=[6])], 3, device=dev)
    with pytest.raises(ValueError, match='canonical'):
        apis.mask_components([dict(size=[2, 2], counts=[2, 1, 0, 1])], device=dev)


def check_api_components(apis, rle, dev):
    H, W, masks = api_masks()
    dense, lists, strings = _forms(rle, masks, H, W, dev)
    want = [cref.check(m)[1] for m in masks]
    for src, kw in ((dense, {}), (lists, dict(device=dev)), (strings, dict(device=dev))):
        got = apis.mask_components(src, **kw)
        assert [g['count'] for g in got] == [len(w) for w in want]
        for g, w in zip(got, want):
            assert g['areas'].dtype == np.int32 and g['areas'].tolist() == [d['area'] for d in w]
            assert g['bboxes'].dtype == np.int32 and g['bboxes'].shape == (len(w), 4)
            assert [tuple(b) for b in g['bboxes'].tolist()] == [d['box'] for d in w]
    assert max(len(w) for w in want) > 20 and min(len(w) for w in want) == 0


def check_api_obb_per_component(apis, rle, dev):
    """masks_to_obb(per_component=True) in all four forms against tests/_mask_obb_ref.py applied per reference component"""
    H, W, masks = api_masks()
    dense, lists, strings = _forms(rle, masks, H, W, dev)
    wants = []
    for m in masks:
        labels, comps = cref.check(m)
        wants.append([oref.check(labels == c) for c in range(len(comps))])
    floats = [ocases.want_floats(w) for w in wants]
    for src, kw in ((dense, {}), (lists, dict(device=dev)), (strings, dict(device=dev))):
        c = apis.masks_to_obb(src, per_component=True, **kw)
        x = apis.masks_to_obb(src, form='xywha', per_component=True, **kw)
        h = apis.masks_to_obb(src, form='hull', per_component=True, **kw)
        assert len(c) == len(x) == len(h) == len(masks)
        for i, w in enumerate(wants):
            assert c[i].shape == (len(w), 4, 2) and x[i].shape == (len(w), 5) and len(h[i]) == len(w)
            assert ocases.close(c[i], floats[i][0]) and ocases.close(x[i], floats[i][1])
            assert all(hh.dtype == np.int32 and [tuple(v) for v in hh.tolist()] == ww[0] for hh, ww in zip(h[i], w))
    geo = apis.masks_to_obb(dense, form='geojson', per_component=True)
    assert [len(g) for g in geo] == [len(w) for w in wants] and geo[-1] == []
    for g, f in zip(geo, floats):
        for poly, corners in zip(g, f[0]):
            assert poly['type'] == 'Polygon' and ocases.close(poly['coordinates'][0][:4], corners)
    # the default is unchanged: one box around all components
    whole = apis.masks_to_obb(dense)
    assert whole.shape == (len(masks), 4, 2) and ocases.close(whole, ocases.want_floats([oref.check(m) for m in masks])[0])
    assert len(wants[0]) == 2 and not ocases.close(c[0][:1], whole[:1])


# ------------------------------------------------------------------------------------------------------------- pipeline
def check_pipeline(li, dev, scene, model, patch, dense_masks_of, area, **kw):
    """inference_large_image(min_mask_region_area=area) against the reference applied to the dense masks of the same call
    without it, for masks='rle', 'polygons' and with oriented boxes; boxes, scores and labels stay"""
    from rsprompter_amd import datasets
    base = dict(patch_size=patch, batch_size=3, **kw)
    H, W = scene.shape[:2]
    plain = li.inference_large_image(model, scene, masks='dense', **base)
    dense = dense_masks_of(plain)
    want = [cref.remove_small_regions(m, area, 'both') for m in dense]
    flags = [bool(w[1] or w[2]) for w in want]
    assert 'region_changed' not in plain.pred_instances
    assert 'region_changed' not in li.inference_large_image(model, scene, masks='rle', **base).pred_instances
    out = li.inference_large_image(model, scene, masks='rle', min_mask_region_area=area, oriented_boxes=True, **base)
    p, q = out.pred_instances, plain.pred_instances
    assert torch.equal(p.bboxes, q.bboxes) and torch.equal(p.scores, q.scores) and torch.equal(p.labels, q.labels)
    assert p.region_changed.dtype == torch.bool and p.region_changed.cpu().tolist() == flags
    got = [lref.counts_to_mask(datasets.rle_from_string(r['counts']), H, W) for r in p.masks]
    assert len(got) == len(want) and all((g == w[0]).all() for g, w in zip(got, want))
    assert [r['counts'] for r in p.masks] == [bytes(_string(lref.rle_counts_np(w[0]))) for w in want]
    assert all(g.any() == m.any() for g, m in zip(got, dense))                                   # no mask is emptied
    assert ocases.close(p.obb, ocases.want_floats([oref.obb(w[0]) for w in want])[0])
    rings = li.inference_large_image(model, scene, masks='polygons', min_mask_region_area=area, **base)
    assert rings.pred_instances.region_changed.cpu().tolist() == flags
    assert all((pcases.refill_rings(r, H, W) == w[0]).all() for r, w in zip(rings.pred_instances.masks, want))
    assert any(flags) and not all(flags) and len(dense) >= 10
    return len(dense), sum(flags)


def _string(counts):
    from rsprompter_amd import rle
    return rle.counts_to_string([int(v) for v in counts])
