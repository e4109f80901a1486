"""The host side of the run-table protocol (rsprompter_amd/rle.py over ops.fit_runs), shared by the emulator suite and the
device suite: every pipeline stage started from a capacity that is too small must retry and end with the table -- and the
strings -- of a generous first guess.  The raw kernels' overflow reports have their own tests; this is the loop around
them, which a real scene reaches only when it overflows a generous guess."""
import numpy as np
import torch

import _large_image_ref as ref

TILE_HW, SCENE_HW = (16, 12), (40, 36)
OFFSETS = [(3, 5), (10, 9), (24, 24)]                 # (ox, oy): the column crosses the checkerboard, the empty mask in a corner
GROUPS = [[0, 1], [2]]


def tile_masks():
    """checkerboard, one full column, empty"""
    h, w = TILE_HW
    yy, xx = np.mgrid[:h, :w]
    column = np.zeros((h, w), bool)
    column[:, 7] = True
    return np.stack([(yy + xx) % 2 == 1, column, np.zeros((h, w), bool)])


def _rows(counts, n_host):
    return [counts[i, :int(n_host[i])].tolist() for i in range(len(n_host))]


def check_capacity_retries(ops, dev):
    """encode_runs -> shift_runs -> union_runs -> runs_to_strings from cap = 2 / flat_cap = 1 against the same calls with the
    default capacities, and the strings against the restatement on the dense paste"""
    from oracle import rle as orle
    from rsprompter_amd import rle
    masks = tile_masks()
    (h, w), (H, W) = TILE_HW, SCENE_HW
    md = torch.from_numpy(masks).to(dev)
    off = torch.tensor(OFFSETS, dtype=torch.int32).to(dev)
    goffs = torch.tensor(np.cumsum([0] + [len(g) for g in GROUPS]).astype(np.int32)).to(dev)
    members = torch.tensor([i for g in GROUPS for i in g], dtype=torch.int32).to(dev)
    canvas = np.stack([ref.shift_masks(masks[i:i + 1], OFFSETS[i], SCENE_HW)[0] for i in range(len(masks))])
    want_tile = [ref.rle_counts(m) for m in masks]
    want_scene = [ref.rle_counts(c) for c in canvas]
    want_union = [ref.rle_counts(np.logical_or.reduce(canvas[g], 0)) for g in GROUPS]
    assert len(want_scene[0]) == 193 and len(want_tile[0]) > 2 and len(want_union[0]) > 2

    # the launchers, recorded: how often each ran and what its FIRST attempt reported
    seen = {}

    def record(name, n_of):
        f = getattr(ops, name)

        def g(*a, **k):
            r = f(*a, **k)
            seen.setdefault(name, []).append(n_of(a, r).cpu().tolist())
            return r
        setattr(ops, name, g)
        return name, f
    saved = [record('mask_rle_into', lambda a, r: a[3]), record('rle_shift', lambda a, r: r[1]),
             record('rle_union', lambda a, r: r[1]), record('rle_to_string', lambda a, r: r[1][-1:])]
    try:
        tc, tn, tn_h, tcap = rle.encode_runs(md, cap=2)
        sc, sn, sn_h, scap = rle.shift_runs(tc, tn, off, TILE_HW, SCENE_HW, cap=2)
        uc, un, un_h, ucap = rle.union_runs(sc, sn, SCENE_HW, goffs, members, cap=2)
        s_scene = rle.runs_to_strings(sc, sn, SCENE_HW, flat_cap=1)
        s_union = rle.runs_to_strings(uc, un, SCENE_HW, flat_cap=1)
        tight = {k: [len(v), v[0]] for k, v in seen.items()}
        seen.clear()
        g_tc, g_tn, g_tn_h, _ = rle.encode_runs(md)
        g_sc, g_sn, g_sn_h, _ = rle.shift_runs(g_tc, g_tn, off, TILE_HW, SCENE_HW)
        g_uc, g_un, g_un_h, _ = rle.union_runs(g_sc, g_sn, SCENE_HW, goffs, members)
        g_scene = rle.runs_to_strings(g_sc, g_sn, SCENE_HW)
        g_union = rle.runs_to_strings(g_uc, g_un, SCENE_HW)
        generous = {k: len(v) for k, v in seen.items()}
    finally:
        for name, f in saved:
            setattr(ops, name, f)
    print('attempts and first reports from cap = 2:', tight, '| attempts with the default capacities:', generous)
    # every stage retried, and its first attempt reported the row that needs most
    assert tight['mask_rle_into'] == [2, [-len(c) if len(c) > 2 else len(c) for c in want_tile]]
    assert tight['rle_shift'] == [2, [-193, -3, 1]]
    assert tight['rle_union'] == [2, [-len(want_union[0]), 1]]
    assert tight['rle_to_string'][0] == 4 and tight['rle_to_string'][1][0] > 1          # two tables, two attempts each
    assert generous == dict(mask_rle_into=1, rle_shift=1, rle_union=1, rle_to_string=2)
    assert (tcap, scap, ucap) == (ops.grown_cap(len(want_tile[0])), 256, ops.grown_cap(len(want_union[0])))
    # bit for bit the generous calls' results (a row's entries beyond its n are not written: rows are compared up to n)
    assert tc.shape == g_tc.shape == (3, len(want_tile[0])) and _rows(tc.cpu(), tn_h) == _rows(g_tc.cpu(), g_tn_h)
    for a, b in ((tn, g_tn), (tn_h, g_tn_h), (sn, g_sn), (sn_h, g_sn_h), (un, g_un), (un_h, g_un_h), (tn.cpu(), tn_h),
                 (sn.cpu(), sn_h), (un.cpu(), un_h)):
        assert torch.equal(a, b)
    assert _rows(sc.cpu(), sn_h) == _rows(g_sc.cpu(), g_sn_h) and _rows(uc.cpu(), un_h) == _rows(g_uc.cpu(), g_un_h)
    assert s_scene == g_scene and s_union == g_union
    # and the restatement's on the dense paste
    assert _rows(tc.cpu(), tn_h) == want_tile and _rows(sc.cpu(), sn_h) == want_scene and _rows(uc.cpu(), un_h) == want_union
    size = [H, W]
    assert s_scene == [dict(size=size, counts=orle.rle_to_string(c)) for c in want_scene]
    assert s_union == [dict(size=size, counts=orle.rle_to_string(c)) for c in want_union]
    assert rle.runs_to_dicts(uc, un_h, SCENE_HW) == [dict(size=size, counts=c) for c in want_union]
