"""Bodies of the seam-merge tests (csrc/seam_merge.hip, rsprompter_amd/large_image.py 'seam_mask'), shared by both tiers:
tests/test_seam_merge_cpu.py calls them with the emulated `ops` on CPU tensors, tests/test_gpu_seam_merge.py with the real
ones on cuda:0.  One `check_<name>(ops, dev)` per kernel; the references are tests/_seam_merge_ref.py (numpy) and
tests/_large_image_ref.py.  Everything is compared exactly."""
import numpy as np
import torch

import _large_image_ref as lref
import _seam_merge_ref as sref

PAD = (0.406 * 255, 0.456 * 255, 0.485 * 255)


def rows_from_counts(rows, dev, cap=None):
    """list of run-count lists -> (counts int32 [k, cap], n int32 [k]); a row given as None is an EMPTY ROW (n = 0)"""
    cap = cap or max([len(r) for r in rows if r is not None] + [1])
    counts = torch.zeros((len(rows), cap), dtype=torch.int32)
    n = torch.zeros((len(rows),), dtype=torch.int32)
    for i, r in enumerate(rows):
        if r is not None:
            counts[i, :len(r)] = torch.tensor(r, dtype=torch.int64).to(torch.int32)
            n[i] = len(r)
    return counts.to(dev), n.to(dev)


def rows_from_masks(masks, dev, cap=None):
    return rows_from_counts([None if m is None else lref.rle_counts_np(m) for m in masks], dev, cap)


def _placed(tile_mask, off, full):
    return lref.shift_masks(np.asarray(tile_mask)[None], off, full)[0]


# --------------------------------------------------------------------------------------------------------------- bbox
def bbox_cases():
    rng = np.random.default_rng(11)
    H, W = 7, 9
    z = lambda: np.zeros((H, W), bool)                                              # noqa: E731
    cases = [('empty', z()), ('full', np.ones((H, W), bool))]
    for y, x in ((0, 0), (H - 1, 0), (0, W - 1), (H - 1, W - 1)):
        m = z()
        m[y, x] = True
        cases.append((f'corner {y},{x}', m))
    m = z()
    m[:3, 0] = True
    cases.append(('pixel 0 set', m))
    m = z()
    m[4:, 2] = True
    m[:, 3] = True
    m[:2, 4] = True
    cases.append(('a run spanning columns', m))
    m = z()
    m[H - 1, 5] = True
    m[0, 6] = True
    cases.append(('a run of two pixels over a column end', m))
    for i in range(12):
        cases.append((f'drawn {i}', rng.random((H, W)) < float(rng.choice([0.05, 0.3, 0.9]))))
    return H, W, cases


def check_rle_bbox(ops, dev):
    H, W, cases = bbox_cases()
    masks = [m for _, m in cases] + [None]
    counts, n = rows_from_masks(masks, dev)
    boxes, area = ops.rle_bbox(counts, n, H, W)
    boxes, area = boxes.cpu().tolist(), area.cpu().tolist()
    for i, (name, m) in enumerate(cases):
        wb, wa = sref.bbox_area_dense(m)
        assert (boxes[i], area[i]) == (wb, wa), (name, boxes[i], area[i], wb, wa)
        assert sref.iv_bbox_area(sref.counts_to_iv(lref.rle_counts_np(m)), H) == (wb, wa), name
    assert boxes[-1] == [0, 0, 0, 0] and area[-1] == 0                              # the empty ROW
    # more than one chunk of 256 runs, H == tile height
    rng = np.random.default_rng(12)
    big = [rng.random((40, 37)) < 0.5, np.ones((40, 37), bool)]
    counts, n = rows_from_masks(big, dev)
    assert int(n[0]) > 512
    boxes, area = ops.rle_bbox(counts, n, 40, 37)
    for i, m in enumerate(big):
        assert (boxes[i].cpu().tolist(), int(area[i])) == sref.bbox_area_dense(m)
    b0, a0 = ops.rle_bbox(counts[:0], n[:0], 40, 37)
    assert b0.shape == (0, 4) and a0.shape == (0,)


# ------------------------------------------------------------------------------------------------------- pair overlap
def pair_overlap_scenes():
    """[(H, W, masks (scene-frame dense, None = empty row), pairs, rects)]: a 45 x 70 scene with 32-pixel tiles, one
    whose height equals the tile height, and 40 x 40 noise tiles (about 800 runs each: several chunks of 256)"""
    rng = np.random.default_rng(13)
    out = []
    for (H, W), (h, w) in (((45, 70), (32, 32)), ((32, 70), (32, 32)), ((45, 70), (40, 40))):
        noise = lambda d: rng.random((h, w)) < d                                    # noqa: E731
        a = noise(0.5)
        oy = H - h
        box = np.zeros((h, w), bool)
        box[5:20, 20:] = True
        left = np.zeros((h, w), bool)
        left[:, :6] = True
        masks = [_placed(a, (0, 0), (H, W)),                                        # 0
                 _placed(a, (0, 0), (H, W)),                                        # 1: identical to 0
                 _placed(noise(0.5), (24, oy), (H, W)),                             # 2: noise, overlapping tile
                 _placed(np.ones((h, w), bool), (24, 0), (H, W)),                   # 3: a full tile: ONE run when H == h
                 _placed(box, (0, 0), (H, W)),                                      # 4: a block reaching into tile (24, .)
                 _placed(left, (W - w, oy), (H, W)),                                # 5: whole columns at the far side
                 np.zeros((H, W), bool),                                            # 6: empty mask (counts = [H W])
                 None,                                                              # 7: empty row (n = 0)
                 _placed(noise(0.05), (24, oy), (H, W)),                            # 8: sparse
                 np.ones((H, W), bool),                                             # 9: the whole scene
                 _placed(np.ones((H, 1), bool), (W - 1, 0), (H, W))]                # 10: the last column: disjoint from 0
        R = (24, oy, w, h)                                                          # rect(tile at 0,0) & rect(tile at 24,oy)
        rect_list = [R, (26, 0, 27, H), (0, oy + 3, W, oy + 4), (0, 0, W, H), (30, 10, 30, 20), (5, 5, 3, 9),
                     (W - 3, 0, W, 2), (0, 0, 4, 4), (-5, -5, W + 5, H + 5)]
        pair_list = [(0, 1), (0, 2), (2, 0), (3, 2), (2, 3), (0, 5), (4, 2), (4, 3), (6, 2), (2, 6), (7, 2), (2, 7), (6, 7),
                     (8, 2), (8, 4), (9, 2), (9, 3), (0, 0), (3, 9), (0, 10), (10, 9)]
        pairs, rects = [], []
        for q, p in enumerate(pair_list):
            for r in (rect_list if q < 6 else rect_list[:1] + [rect_list[(q % 7) + 1]]):
                pairs.append(p)
                rects.append(r)
        out.append((H, W, masks, pairs, rects))
    return out


def check_rle_pair_overlap(ops, dev):
    for H, W, masks, pairs, rects in pair_overlap_scenes():
        counts, n = rows_from_masks(masks, dev)
        got = ops.rle_pair_overlap(counts, n, H, W, torch.tensor(pairs, dtype=torch.int32, device=dev),
                                   torch.tensor(rects, dtype=torch.int32, device=dev)).cpu().tolist()
        dense = [np.zeros((H, W), bool) if m is None else m for m in masks]
        ivs = [sref.counts_to_iv(lref.rle_counts_np(m)) for m in dense]
        outside = 0
        for q, ((i, j), r) in enumerate(zip(pairs, rects)):
            want = sref.pair_overlap_dense(dense[i], dense[j], r)
            assert tuple(got[q]) == want, ((H, W), (i, j), r, got[q], want)
            assert sref.iv_pair_overlap(ivs[i], ivs[j], r, H, W) == want, ((H, W), (i, j), r)
            x0, y0, x1, y1 = sref.clip_rect(r, H, W)
            inr = np.zeros((H, W), bool)
            inr[y0:max(y1, y0), x0:max(x1, x0)] = True
            outside += int((dense[i] & dense[j] & ~inr).any())
        assert outside > 10                                  # rectangles that do not contain the intersection
        none = ops.rle_pair_overlap(counts, n, H, W, torch.zeros((0, 2), dtype=torch.int32, device=dev),
                                    torch.zeros((0, 4), dtype=torch.int32, device=dev))
        assert none.shape == (0, 3)
    assert max(len(lref.rle_counts_np(m)) for m in pair_overlap_scenes()[2][2] if m is not None) > 512


# -------------------------------------------------------------------------------------------------------------- union
def union_cases():
    """(H, W, masks, groups): groups = list of member lists"""
    rng = np.random.default_rng(14)
    H, W = 23, 31
    z = lambda: np.zeros((H, W), bool)                                              # noqa: E731

    def rect(x0, y0, x1, y1):
        m = z()
        m[y0:y1, x0:x1] = True
        return m
    masks = [rect(2, 3, 9, 12), rect(6, 8, 15, 20),                 # 0, 1 overlapping
             rect(20, 0, 22, 10), rect(20, 10, 22, 23),             # 2, 3 touching without overlapping (one column run)
             rect(1, 1, 30, 22), rect(10, 10, 12, 12),              # 4, 5 nested
             z(), None,                                             # 6 empty mask, 7 empty row
             rect(0, 0, 16, 12), rect(15, 0, 31, 12), rect(0, 11, 16, 23), rect(15, 11, 31, 23),   # 8-11: a corner, full
             rng.random((H, W)) < 0.5, rng.random((H, W)) < 0.5,    # 12, 13 noise: more than 256 runs together
             rect(0, 0, 1, 1), rect(30, 22, 31, 23),                # 14 pixel 0, 15 the last pixel
             rect(5, 0, 6, 23), rect(6, 0, 7, 23)]                  # 16, 17 whole columns side by side: one run
    groups = [[i] for i in range(len(masks))]
    groups += [[0, 1], [2, 3], [4, 5], [5, 4], [6, 0], [7, 1], [6, 7], [8, 9, 10, 11], [12, 13], [12, 13, 0, 4], [14, 15],
               [16, 17], [3, 2, 16], []]
    return H, W, masks, groups


def _run_union(ops, dev, counts, n, H, W, groups, cap_out):
    offs = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    mem = torch.tensor([i for g in groups for i in g], dtype=torch.int32, device=dev)
    return ops.rle_union(counts, n, H, W, torch.from_numpy(offs).to(dev), mem, cap_out)


def check_rle_union(ops, dev):
    H, W, masks, groups = union_cases()
    counts, n = rows_from_masks(masks, dev)
    dense = [np.zeros((H, W), bool) if m is None else m for m in masks]
    want = [lref.rle_counts_np(np.logical_or.reduce([dense[i] for i in g] + [np.zeros((H, W), bool)])) for g in groups]
    assert want[len(masks) + 7] == [0, H * W] and max(len(w) for w in want) > 256       # the full canvas; many runs
    out, no = _run_union(ops, dev, counts, n, H, W, groups, 1024)
    out, no = out.cpu(), no.cpu().tolist()
    ivs = [sref.counts_to_iv(lref.rle_counts_np(m)) for m in dense]
    for g, grp in enumerate(groups):
        assert out[g, :no[g]].tolist() == want[g], (grp, out[g, :max(no[g], 0)].tolist(), want[g])
        assert sref.iv_union_counts([ivs[i] for i in grp], H, W) == want[g], grp
    for i, m in enumerate(masks):                                                  # groups of one: the member's row
        if m is not None:
            assert out[i, :no[i]].tolist() == counts[i, :int(n[i])].cpu().tolist(), i
    # short capacity: every group reports -(needed), those that fit are written; the retry at exactly the need fits
    out2, no2 = _run_union(ops, dev, counts, n, H, W, groups, 8)
    no2 = no2.cpu().tolist()
    assert no2 == [len(w) if len(w) <= 8 else -len(w) for w in want]
    need = max(len(w) for w in want)
    out3, no3 = _run_union(ops, dev, counts, n, H, W, groups, need)
    assert no3.cpu().tolist() == [len(w) for w in want]
    assert all(out3[g, :len(w)].cpu().tolist() == w for g, w in enumerate(want))
    o0, n0 = _run_union(ops, dev, counts, n, H, W, [], 16)
    assert o0.shape[0] == 0 and n0.shape[0] == 0


def check_refuses_scenes_beyond_32_bit_counts(ops, dev, pytest):
    counts, n = rows_from_counts([[4]], dev)
    z = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    H, W = 65536, 32768
    with pytest.raises(ValueError, match='32-bit'):
        ops.rle_bbox(counts, n, H, W)
    with pytest.raises(ValueError, match='32-bit'):
        ops.rle_pair_overlap(counts, n, H, W, z, torch.zeros((1, 4), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match='32-bit'):
        ops.rle_union(counts, n, H, W, torch.tensor([0, 1], dtype=torch.int32, device=dev), z[0, :1], 8)
    lib = ops._lib.load()
    p = torch.zeros((64,), dtype=torch.int64, device=dev).data_ptr()
    assert lib.rsp_rle_bbox(p, p, 1, 4, H, W, p, p, 0) != 0
    assert lib.rsp_rle_pair_overlap(p, p, 1, 4, H, W, p, p, 1, p, p, 0) != 0
    assert lib.rsp_rle_intervals(p, p, 1, 4, H, W, p, p, p, 1, 1, p, p, 0) != 0
    assert lib.rsp_rle_union(p, p, 1, p, 1, H, W, p, p, 8, 0) != 0


# ----------------------------------------------------------------------------------------------------- stub detectors
def _stub_cfg(scale):
    return dict(test_dataloader=dict(dataset=dict(pipeline=[
        dict(type='LoadImageFromFile', to_float32=True), dict(type='Resize', scale=scale, keep_ratio=True),
        dict(type='Pad', size=scale, pad_val=dict(img=PAD, masks=0)),
        dict(type='PackDetInputs', meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor'))])))


class RandomStub(torch.nn.Module):
    """a detector whose result is a seeded function of the tile's pixels: masks of density 0 / 0.05 / 0.5 / 1, two labels"""

    def __init__(self, scale):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.cfg = _stub_cfg(scale)

    def test_step(self, data):
        from rsprompter_amd.structures import InstanceData
        for x, s in zip(data['inputs'], data['data_samples']):
            th, tw = s.metainfo['ori_shape']
            rng = np.random.default_rng(int(x.double().sum().item()) % (2 ** 31))
            k = int(rng.integers(2, 7))
            x0, y0 = rng.integers(0, tw - 4, k), rng.integers(0, th - 4, k)
            boxes = np.stack([x0, y0, x0 + rng.integers(2, 12, k), y0 + rng.integers(2, 12, k)], 1).astype(np.float32).reshape(-1, 4)
            masks = rng.random((k, th, tw)) < rng.choice([0.0, 0.05, 0.5, 1.0], k)[:, None, None]
            dev = x.device
            s.pred_instances = InstanceData(bboxes=torch.from_numpy(boxes).to(dev),
                                            scores=torch.from_numpy(rng.random(k).astype(np.float32)).to(dev),
                                            labels=torch.from_numpy(rng.integers(0, 2, k)).to(dev),
                                            masks=torch.from_numpy(masks).to(dev))
        return data['data_samples']


class PlantedStub(torch.nn.Module):
    """a perfect detector of planted objects: channel 0 of the tile holds an object id per pixel; one instance per id
    present, mask = (tile == id), box = the fragment's tight box, score = a function of the id and the fragment's size"""

    def __init__(self, scale, label_of):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.cfg = _stub_cfg(scale)
        self.label_of = dict(label_of)

    def test_step(self, data):
        from rsprompter_amd.structures import InstanceData
        for x, s in zip(data['inputs'], data['data_samples']):
            th, tw = s.metainfo['ori_shape']
            ids = x[0, :th, :tw].round().to(torch.int64).cpu().numpy()
            boxes, scores, labels, masks = [], [], [], []
            for i in sorted(set(ids.reshape(-1).tolist()) - {0}):
                m = ids == i
                b, a = sref.bbox_area_dense(m)
                boxes.append(b)
                scores.append(0.25 + 0.01 * i + a / 4096.0)
                labels.append(self.label_of[i])
                masks.append(m)
            dev = x.device
            s.pred_instances = InstanceData(
                bboxes=torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4).to(dev),
                scores=torch.tensor(scores, dtype=torch.float32).to(dev), labels=torch.tensor(labels, dtype=torch.int64).to(dev),
                masks=torch.from_numpy(np.asarray(masks, bool).reshape(-1, th, tw)).to(dev))
        return data['data_samples']


def planted_scene():
    """-> (scene uint8 [80, 104, 3] with the object id in channel 0, {id: label}, patch size): 32-pixel tiles at 0.25
    overlap start at x = 0, 24, 48, 72 and y = 0, 24, 48"""
    H, W = 80, 104
    ids = np.zeros((H, W), np.uint8)
    yy, xx = np.mgrid[:H, :W]
    label_of = {}

    def plant(i, label, m):
        assert not (ids[m] != 0).any()
        ids[m] = i
        label_of[i] = label
    box = lambda x0, y0, x1, y1: (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)     # noqa: E731
    ell = lambda cx, cy, rx, ry: ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0   # noqa: E731
    plant(1, 0, box(20, 4, 40, 14))                                # crosses the seam between x-tiles 0 and 1
    plant(2, 1, ell(28, 28, 6.5, 6.5))                             # covers a tile corner: four fragments
    plant(3, 0, box(10, 60, 70, 70))                               # wider than a tile: three fragments in a chain
    plant(4, 1, box(50, 5, 54, 12))                                # wholly inside an overlap band: seen twice in full
    plant(5, 0, box(60, 10, 68, 20))                               # wholly inside one tile
    plant(6, 1, box(84, 20, 89, 50) | box(84, 45, 100, 50))        # an L over two horizontal seams
    plant(7, 0, ell(52, 40, 8, 6))                                 # crosses the seam between x-tiles 1 and 2
    plant(8, 1, box(26, 70, 30, 78))                               # inside the band of x-tiles 0 / 1, label 1
    scene = np.zeros((H, W, 3), np.uint8)
    scene[..., 0] = ids
    return scene, label_of, 32


def check_planted_objects(li, dev):
    """every planted object comes back as ONE instance with its own shape and all its fragments; box NMS alone returns
    more instances than there are objects"""
    from oracle import rle as orle
    scene, label_of, patch = planted_scene()
    H, W = scene.shape[:2]
    ids = scene[..., 0]
    model = PlantedStub((patch, patch), label_of).to(dev)
    out, patches, start = li.inference_large_image(model, scene, patch_size=patch, batch_size=4, merge_nms_type='seam_mask',
                                                    seam_iou_thr=0.5, return_patches=True)
    assert len(patches) == len(start) == 12
    frag_id = [i for (x, y) in start for i in sorted(set(ids[y:y + patch, x:x + patch].reshape(-1).tolist()) - {0})]
    p = out.pred_instances
    assert len(p.scores) == len(label_of) == len(out.members), (len(p.scores), len(label_of))
    seen = set()
    for k, rle in enumerate(p.masks):
        m = lref.counts_to_mask(orle.rle_from_string(rle['counts']), H, W)
        got_ids = set(ids[m].tolist())
        assert len(got_ids) == 1, got_ids
        i = got_ids.pop()
        assert np.array_equal(m, ids == i), i                                      # the whole planted shape
        assert sorted(out.members[k]) == [q for q, f in enumerate(frag_id) if f == i], i   # all its fragments
        assert int(p.labels[k]) == label_of[i] and int(out.keep[k]) in out.members[k]
        assert p.bboxes[k].tolist() == [float(v) for v in sref.bbox_area_dense(ids == i)[0]]
        seen.add(i)
    assert seen == set(label_of)
    assert sorted(len(m) for m in out.members) == [1, 2, 2, 2, 2, 3, 3, 4]
    plain = li.inference_large_image(model, scene, patch_size=patch, batch_size=4, merge_nms_type='nms')
    assert len(plain.pred_instances.scores) > len(label_of)
    return out


# ------------------------------------------------------------------------------------------------------------ at scale
def _merge_touching(iv):
    """sorted [start, end) intervals -> the same set with touching neighbours joined (canonical runs)"""
    if len(iv) == 0:
        return iv
    new = np.concatenate([[True], iv[1:, 0] > iv[:-1, 1]])
    first = np.flatnonzero(new)
    last = np.concatenate([first[1:] - 1, [len(iv) - 1]])
    return np.stack([iv[first, 0], iv[last, 1]], 1)


def _iv_to_counts(iv, n_px):
    iv = _merge_touching(iv)
    pos = np.concatenate([[0], iv.reshape(-1), [n_px]])
    c = np.diff(pos)
    return c[:-1].tolist() if len(iv) and iv[-1, 1] == n_px else c.tolist()


def synthetic_instances(H, W, patch, n_obj, noise, seed):
    """a scene of random ellipses (three labels) seen through patch-sized tiles at 0.25 overlap, built WITHOUT any dense
    array: per fragment its tile-frame run counts, its scene-frame intervals, its tight box as the detector's box.  `noise`
    = side of the square noise masks added in overlap bands (thousands of runs each), in pairs of tiles: one pair with the
    same noise (one object), the others with independent noise (masks that intersect and disagree)."""
    rng = np.random.default_rng(seed)
    tiles = lref.slice_bboxes(H, W, patch, patch, 0.25, 0.25)
    cx, cy = rng.uniform(0, W, n_obj), rng.uniform(0, H, n_obj)
    rx, ry = rng.uniform(patch / 32, patch / 3, n_obj), rng.uniform(patch / 32, patch / 3, n_obj)
    lab = rng.integers(0, 3, n_obj)
    per_tile = [[] for _ in tiles]

    def add(t, tile_iv, scene_iv, label, score):
        x0, y0, x1, y1 = tiles[t]
        h = y1 - y0
        box, _ = sref.iv_bbox_area(tile_iv, h)
        per_tile[t].append(dict(counts=_iv_to_counts(tile_iv, h * (x1 - x0)), iv=scene_iv, label=int(label), score=float(score),
                                bbox=[box[0] + x0, box[1] + y0, box[2] + x0, box[3] + y0]))
    for t, (x0, y0, x1, y1) in enumerate(tiles):
        h = y1 - y0
        for o in np.flatnonzero((cx + rx >= x0) & (cx - rx < x1) & (cy + ry >= y0) & (cy - ry < y1)):
            x = np.arange(max(x0, int(np.floor(cx[o] - rx[o]))), min(x1, int(np.ceil(cx[o] + rx[o])) + 1), dtype=np.int64)
            d = 1.0 - ((x - cx[o]) / rx[o]) ** 2
            x, d = x[d >= 0], d[d >= 0]
            hh = ry[o] * np.sqrt(d)
            ya = np.maximum(np.ceil(cy[o] - hh).astype(np.int64), y0)
            yb = np.minimum(np.floor(cy[o] + hh).astype(np.int64) + 1, y1)
            ok = yb > ya
            x, ya, yb = x[ok], ya[ok], yb[ok]
            if x.size:
                add(t, np.stack([(x - x0) * h + ya - y0, (x - x0) * h + yb - y0], 1), np.stack([x * H + ya, x * H + yb], 1),
                    lab[o], rng.random())
    if noise:
        pairs = [(a, b) for a in range(len(tiles)) for b in range(a + 1, len(tiles))
                 if (r := sref.rect_intersection(tiles[a], tiles[b])) and r[2] - r[0] >= noise and r[3] - r[1] >= noise]
        for q, (a, b) in enumerate(pairs[::max(1, len(pairs) // 8)][:8]):
            r = sref.rect_intersection(tiles[a], tiles[b])
            m1 = rng.random((noise, noise)) < 0.3
            m2 = m1 if q == 0 else rng.random((noise, noise)) < 0.3
            for t, m in ((a, m1), (b, m2)):
                x0, y0, x1, y1 = tiles[t]
                idx = np.flatnonzero(m.T.reshape(-1))
                col, row = idx // noise, idx % noise

                def frame(fx, fy, fh):
                    p = (r[0] - fx + col) * fh + (r[1] - fy + row)
                    brk = np.flatnonzero(np.diff(p) != 1)
                    return np.stack([p[np.concatenate([[0], brk + 1])], p[np.concatenate([brk, [len(p) - 1]])] + 1], 1)
                add(t, frame(x0, y0, y1 - y0), frame(0, 0, H), 3, 0.5 + 0.01 * q)
    return tiles, per_tile


def check_at_scale(ops, li, dev, H, W, patch, n_obj, noise, seed=0, seam_thr=0.5, nms_thr=0.25, measure=None):
    """the three kernels and the merge on synthetic_instances against the interval-domain restatement"""
    from oracle import glue
    from oracle import rle as orle
    from rsprompter_amd import rle
    tiles, per_tile = synthetic_instances(H, W, patch, n_obj, noise, seed)
    inst = [f for frs in per_tile for f in frs]
    tile = [t for t, frs in enumerate(per_tile) for _ in frs]
    N = len(inst)
    boxes = np.asarray([f['bbox'] for f in inst], np.float32).reshape(-1, 4)
    scores = np.asarray([f['score'] for f in inst], np.float32)
    labels = np.asarray([f['label'] for f in inst], np.int64)
    ivs = [f['iv'] for f in inst]
    want = sref.seam_merge_iv(ivs, boxes, scores, labels, tile, tiles, (H, W), seam_thr, glue.batched_nms, nms_thr)
    assert len(want['edges']) > 0 and len(want['rejected']) > 0 and max(len(m) for _, m in want['comps']) >= 3
    th, tw = tiles[0][3] - tiles[0][1], tiles[0][2] - tiles[0][0]
    counts, n = rows_from_counts([f['counts'] for f in inst], dev)
    origin = torch.tensor([[tiles[t][0], tiles[t][1]] for t in tile], dtype=torch.int32, device=dev)
    # kernels: shift + bbox, pair overlap over every pair the restatement evaluated, union of every component
    sc, sn = rle.shift_runs(counts, n, origin, (th, tw), (H, W))[:2]
    tb, area = ops.rle_bbox(sc, sn, H, W)
    tb, area = tb.cpu().tolist(), area.cpu().tolist()
    for i in range(N):
        assert (tb[i], area[i]) == sref.iv_bbox_area(ivs[i], H), i
    ev = [e for e in want['evaluated'] if e[3] > 0 or e[4] > 0 or e[5] > 0]
    pairs = torch.tensor([[e[0], e[1]] for e in ev], dtype=torch.int32, device=dev).reshape(-1, 2)
    rects = torch.tensor([list(e[2]) for e in ev], dtype=torch.int32, device=dev).reshape(-1, 4)
    got = ops.rle_pair_overlap(sc, sn, H, W, pairs, rects).cpu().tolist()
    assert got == [list(e[3:]) for e in ev]
    groups = [m for _, m in want['comps']]
    cap_out = max(sum(2 * len(ivs[i]) + 1 for i in g) for g in groups) + 1
    uc, un = _run_union(ops, dev, sc, sn, H, W, groups, cap_out)
    uc, un = uc.cpu(), un.cpu().tolist()
    multi = [g for g, m in enumerate(groups) if len(m) > 1]
    for g in multi + [g for g in range(len(groups)) if len(groups[g]) == 1][:40]:
        assert uc[g, :un[g]].tolist() == sref.iv_union_counts([ivs[i] for i in groups[g]], H, W), groups[g]
    if measure is not None:
        measure['start']()
    # the merge as inference_large_image runs it after the last batch
    out, keep, members, grp = li._seam_merge(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev),
                                             torch.from_numpy(labels).to(dev), torch.tensor(tile, dtype=torch.int64, device=dev),
                                             tiles, counts, n, (th, tw), (H, W), seam_thr, nms_thr)
    rles = li._seam_rle(counts, n, origin, grp, (th, tw), (H, W))
    if measure is not None:
        measure['stop'](len(rles))
    assert keep.cpu().tolist() == want['keep'] and members == want['members']
    assert np.array_equal(out.bboxes.cpu().numpy(), want['bboxes']) and np.array_equal(out.scores.cpu().numpy(), want['scores'])
    assert np.array_equal(out.labels.cpu().numpy(), want['labels'])
    assert [r['counts'] for r in rles] == [orle.rle_to_string(c) for c in want['counts']]
    return dict(instances=N, merged=want['n_merged'], kept=len(want['keep']), pairs=len(ev), edges=len(want['edges']),
                rejected=len(want['rejected']), max_runs=int(n.max()), tiles=len(tiles))
