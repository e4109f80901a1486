"""Measurements of the seam merge on one GPU, device events, both sides alternating in one run:

  python tools/bench_seam_merge.py pairs   (a) rsp_rle_pair_overlap over every candidate pair of the synthetic 4096 x 5000 scene of
                                           tests/test_gpu_seam_merge.py, against the dense torch form -- paste both masks into
                                           the scene, `(a & b).sum()`, `a[R].sum()`, `b[R].sum()` -- on a subsample of the pairs
  python tools/bench_seam_merge.py stage   (b) the merge stage of inference_large_image, 'seam_mask' against 'nms', on the ViT-B
                                           mosaic scene of tools/large_image_measure.py (seeded weights), with the instance
                                           counts before and after
  python tools/bench_seam_merge.py synthetic   the two merge stages alone on the synthetic scene of (a): instance-like masks
Each prints one JSON line (profiles/seam_merge/)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _event_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), r


def pairs(dev, n_dense=48, rounds=5):
    import _seam_merge_cases as cases
    from rsprompter_amd import large_image as li
    from rsprompter_amd import ops, rle
    H, W, patch = 4096, 5000, 640
    tiles, per_tile = cases.synthetic_instances(H, W, patch, 580, 256, 0)
    inst = [f for frs in per_tile for f in frs]
    tile = np.asarray([t for t, frs in enumerate(per_tile) for _ in frs])
    counts, n = cases.rows_from_counts([f['counts'] for f in inst], dev)
    origin = torch.tensor([[tiles[t][0], tiles[t][1]] for t in tile], dtype=torch.int32, device=dev)
    labels = torch.tensor([f['label'] for f in inst], device=dev)
    sc, sn = rle.shift_runs(counts, n, origin, (patch, patch), (H, W))[:2]
    tight, _ = ops.rle_bbox(sc, sn, H, W)
    pr, rc = li._seam_pairs(tiles, tile, tight, labels, dev)
    P = int(pr.shape[0])
    # the dense side: tile masks of the subsample's instances decoded once (not timed), then per pair paste + three sums
    sub = torch.linspace(0, P - 1, n_dense).long().tolist()
    rows = sorted({int(v) for q in sub for v in pr[q].tolist()})
    dense_tile = {}
    for i in rows:
        c = counts[i, :int(n[i])].to(torch.int64)
        e = torch.cumsum(c, 0)
        d = torch.zeros((patch * patch + 1,), dtype=torch.int32, device=dev)
        d.index_add_(0, (e - c)[1::2], torch.ones_like(c[1::2], dtype=torch.int32))
        d.index_add_(0, e[1::2], -torch.ones_like(c[1::2], dtype=torch.int32))
        dense_tile[i] = (torch.cumsum(d[:-1], 0) > 0).view(patch, patch).t().contiguous()

    def dense_form():
        out = []
        for q in sub:
            i, j = pr[q].tolist()
            x0, y0, x1, y1 = rc[q].tolist()
            m = ops.paste_tiles(torch.stack([dense_tile[i], dense_tile[j]]), origin[[i, j]].contiguous(), (H, W))
            out.append(torch.stack([(m[0] & m[1]).sum(), m[0, y0:y1, x0:x1].sum(), m[1, y0:y1, x0:x1].sum()]))
        return torch.stack(out)

    def run_domain():
        return ops.rle_pair_overlap(sc, sn, H, W, pr, rc)
    run_domain(), dense_form()
    res = dict(instances=len(inst), pairs=P, dense_pairs=len(sub), run_domain_ms=[], dense_ms=[])
    for _ in range(rounds):
        t, got = _event_ms(run_domain)
        res['run_domain_ms'].append(t)
        t, want = _event_ms(dense_form)
        res['dense_ms'].append(t)
    assert torch.equal(got[sub].to(torch.int64), want.to(torch.int64)), 'the two forms disagree'
    med = lambda v: sorted(v)[len(v) // 2]                                      # noqa: E731
    res.update(run_domain_us_per_pair=1e3 * med(res['run_domain_ms']) / P, dense_us_per_pair=1e3 * med(res['dense_ms']) / len(sub),
               with_positive_intersection=int((got[:, 0] > 0).sum()), max_runs=int(sn.max()))
    return res


def synthetic(dev, rounds=5):
    """the merge stage alone on the synthetic scene (instance-like masks: hundreds of runs, eight noise masks): the
    'seam_mask' stage (_seam_merge + _seam_rle) against the 'nms' stage (nms_flat + _scene_rle of the kept), wall clock
    around a device synchronise, alternating"""
    import _seam_merge_cases as cases
    from rsprompter_amd import large_image as li
    from rsprompter_amd import ops
    H, W, patch = 4096, 5000, 640
    tiles, per_tile = cases.synthetic_instances(H, W, patch, 580, 256, 0)
    inst = [f for frs in per_tile for f in frs]
    tile = torch.tensor([t for t, frs in enumerate(per_tile) for _ in frs], dtype=torch.int64, device=dev)
    counts, n = cases.rows_from_counts([f['counts'] for f in inst], dev)
    origin = torch.tensor([[tiles[t][0], tiles[t][1]] for t in tile.tolist()], dtype=torch.int32, device=dev)
    boxes = torch.tensor([f['bbox'] for f in inst], dtype=torch.float32, device=dev)
    scores = torch.tensor([f['score'] for f in inst], dtype=torch.float32, device=dev)
    labels = torch.tensor([f['label'] for f in inst], device=dev)

    def seam():
        out, keep, members, grp = li._seam_merge(boxes, scores, labels, tile, tiles, counts, n, (patch, patch), (H, W), 0.5, 0.25)
        return len(li._seam_rle(counts, n, origin, grp, (patch, patch), (H, W)))

    def nms():
        keep = ops.nms_flat(boxes, scores, labels, 0.25)
        return len(li._scene_rle(counts[keep], n[keep].contiguous(), origin[keep].contiguous(), (patch, patch), (H, W)))
    res = dict(instances=len(inst), median_runs=int(n.median()), max_runs=int(n.max()), seam_mask_s=[], nms_s=[])
    for r in range(rounds + 1):
        for key, f in (('nms_s', nms), ('seam_mask_s', seam)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = f()
            torch.cuda.synchronize()
            if r:
                res[key].append(time.perf_counter() - t0)
            res[key[:-2] + '_out'] = k
    return res


def stage(dev, rounds=3):
    import large_image_measure as lim
    from rsprompter_amd import large_image as li
    from rsprompter_amd import ops
    m = lim.build('base', dev)
    scene = lim.mosaic(4096, 5000)
    T = {}

    def wrap(obj, name, key):
        f = getattr(obj, name)

        def g(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = f(*a, **k)
            torch.cuda.synchronize()
            T[key] = T.get(key, 0.0) + time.perf_counter() - t
            return r
        setattr(obj, name, g)
    for obj, name, key in ((ops, 'nms_flat', 'nms_flat'), (li, '_scene_rle', 'scene_rle'), (li, '_seam_merge', 'seam_merge'),
                           (li, '_seam_rle', 'seam_rle'), (ops, 'rle_pair_overlap', 'seam_merge.pair_overlap'),
                           (ops, 'rle_union', 'seam_rle.union'), (li, '_seam_pairs', 'seam_merge.pairs'),
                           (li, '_seam_components', 'seam_merge.components')):
        wrap(obj, name, key)
    seen, plain_nms = {}, ops.nms_flat

    def counting_nms(boxes, *a):
        seen['n'] = int(boxes.shape[0])
        return plain_nms(boxes, *a)
    ops.nms_flat = counting_nms
    res = dict(tiles=35, nms=[], seam_mask=[])
    for r in range(rounds + 1):
        for mode in ('nms', 'seam_mask'):
            T.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = li.inference_large_image(m, scene, patch_size=1024, batch_size=4, merge_nms_type=mode)
            torch.cuda.synchronize()
            tot = time.perf_counter() - t0
            if r == 0:
                continue                                                        # warm-up
            stage_s = T.get('seam_merge', 0.0) + T.get('seam_rle', 0.0) if mode == 'seam_mask' else T['nms_flat'] + T.get('scene_rle', 0.0)
            res[mode].append(dict(scene_s=tot, merge_stage_s=stage_s, phases_s={k: round(v, 5) for k, v in T.items()},
                                  out=len(out.pred_instances.scores)))
            res[mode][-1]['into_box_nms'] = seen['n']                           # all instances ('nms') / merged instances
            if mode == 'seam_mask':
                res['largest_component'] = max([len(x) for x in out.members] + [0])
    return res


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('bench_seam_merge.py needs the GPU: a CPU run measures nothing')
    mode = sys.argv[1] if len(sys.argv) > 1 else 'pairs'
    print(json.dumps({mode: dict(pairs=pairs, stage=stage, synthetic=synthetic)[mode](torch.device('cuda:0'))}))
