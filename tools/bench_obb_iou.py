"""Measurements of the oriented-box comparison on one GPU, with device events: after a warm-up of every shape,
--repeats timed windows of --inner back-to-back calls each between two events, the sides alternating; medians per call.

  python tools/bench_obb_iou.py [--out profiles/obb_iou/obb_iou.json] [--repeats 10] [--inner 5] [--host-pairs 20000]

* ops.obb_iou on one unit of 300 x 300 boxes (tile instances of 128-pixel tiles near each other), the same boxes through
  apis.obb_iou (one unit a row), and on the unit load of
  DESIGN §13: 1 000 units of 100 dts x 50 gts (5 M pairs), boxes in a 512-pixel image;
* ops.obb_nms at n = 1 000, 10 000 and 32 768, the boxes clustered (a box overlaps tens of others) and spread (a handful),
  with the share of the n (n - 1) / 2 pairs whose axis-aligned bounds overlap (the pairs that are clipped) and the number
  kept; beside it ops.nms_flat on the axis-aligned bounds of the same boxes;
* the float64 twin of tests/_obb_iou_ref.py in a host loop over --host-pairs of the same pairs, per pair;
* the `obb` metric beside `segm` on §13's load (tools/bench_coco_iou_runs.py tiles_load: --metric-images images of 512 x 512,
  100 detections and 50 ground truths each): device_evaluate's timings['device'] (strings to run tables, rectangles or mask
  IoU, matching, the copy of the match tables; a host clock around work that ends in a device synchronise), both on the run
  route, alternating, medians of --metric-repeats after a warm-up of each.
Prints and writes one JSON document."""
import argparse
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


def _boxes(rng, n, side, wmax=90.0, hmax=40.0):
    cx, cy = rng.uniform(0, side, n), rng.uniform(0, side, n)
    w, h, a = rng.uniform(20, wmax, n), rng.uniform(8, hmax, n), rng.uniform(-np.pi, np.pi, n)
    ux, uy = np.cos(a), np.sin(a)
    sa, sb = np.array([-1.0, 1.0, 1.0, -1.0]), np.array([-1.0, -1.0, 1.0, 1.0])
    x = cx[:, None] + sa * (w / 2 * ux)[:, None] - sb * (h / 2 * uy)[:, None]
    y = cy[:, None] + sa * (w / 2 * uy)[:, None] + sb * (h / 2 * ux)[:, None]
    return np.stack([x, y], 2)


def _event_ms(f, inner):
    """one window: `inner` calls between two device events -> milliseconds per call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def _measure(sides, repeats, inner):
    for f in sides.values():                                   # warm-up of every shape
        f()
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(repeats):
        for k, f in sides.items():                             # alternating
            ms[k].append(_event_ms(f, inner))
    return {k: _stats(v) for k, v in ms.items()}


def _aabb(q):
    return np.concatenate([q.min(1), q.max(1)], 1).astype(np.float32)


def _overlap_share(q, chunk=2048):
    """the share of the pairs i < j whose axis-aligned bounds overlap"""
    lo, hi = torch.from_numpy(q.min(1)).cuda(), torch.from_numpy(q.max(1)).cuda()
    n, hits = len(q), 0
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        hit = (hi[s:e, None, 0] > lo[None, :, 0]) & (hi[None, :, 0] > lo[s:e, None, 0]) & \
            (hi[s:e, None, 1] > lo[None, :, 1]) & (hi[None, :, 1] > lo[s:e, None, 1])
        hits += int(hit.sum()) - (e - s)
    return hits / 2 / (n * (n - 1) / 2)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'obb_iou', 'obb_iou.json'))
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--host-pairs', type=int, default=20000)
    ap.add_argument('--nms-sizes', type=int, nargs='+', default=[1000, 10000, 32768])
    ap.add_argument('--metric-images', type=int, default=1000, help='0 skips the metric measurement')
    ap.add_argument('--metric-repeats', type=int, default=3)
    a = ap.parse_args(argv)
    import _obb_iou_ref as ref
    from rsprompter_amd import ops
    assert torch.cuda.is_available(), 'bench_obb_iou.py measures on the GPU'
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, inner=a.inner,
               clock='device events around `inner` back-to-back calls, per call', iou={}, nms={})
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)                         # noqa: E731

    # ---- IoU blocks
    q300 = _boxes(rng, 300, 1500.0, 128.0, 128.0)
    u300 = ops.coco_units([0], [0], [0], [300], [300], [0], dev)
    d300, c300 = up(q300), torch.zeros(300, dtype=torch.uint8, device=dev)
    U, nd, ng = 1000, 100, 50
    dq = np.concatenate([_boxes(rng, nd, 512.0) for _ in range(U)])
    gq = np.concatenate([_boxes(rng, ng, 512.0) for _ in range(U)])
    idx = np.arange(U, dtype=np.int64)
    units = ops.coco_units(idx * nd, idx * ng, idx * nd * ng, np.full(U, nd), np.full(U, ng), np.zeros(U, np.int64), dev)
    dd, gd, crowd = up(dq), up(gq), torch.zeros(U * ng, dtype=torch.uint8, device=dev)
    from rsprompter_amd import apis
    sides = {'300x300': lambda: ops.obb_iou(u300, 300 * 300, d300, d300, c300),
             'apis.obb_iou 300x300 (a unit a row)': lambda: apis.obb_iou(d300, d300, device=dev),
             '1000 units of 100x50': lambda: ops.obb_iou(units, U * nd * ng, dd, gd, crowd)}
    res = _measure(sides, a.repeats, a.inner)
    iou = ops.obb_iou(units, U * nd * ng, dd, gd, crowd)
    doc['iou'] = {k: dict(ms=v) for k, v in res.items()}
    doc['iou']['300x300'].update(pairs=90000, nonzero=int((ops.obb_iou(u300, 90000, d300, d300, c300) > 0).sum()))
    doc['iou']['1000 units of 100x50'].update(pairs=U * nd * ng, nonzero=int((iou > 0).sum()))
    # the float64 twin in a host loop over the first pairs of the unit load, and the device against it
    k = min(a.host_pairs, nd * ng * U)
    pi = np.arange(k)
    ui, di, gi = pi // (nd * ng), (pi % (nd * ng)) // ng, pi % ng
    t0 = time.perf_counter()
    host = [ref.twin_iou(dq[u * nd + d], gq[u * ng + g]) for u, d, g in zip(ui.tolist(), di.tolist(), gi.tolist())]
    t1 = time.perf_counter()
    doc['iou']['host twin'] = dict(pairs=k, us_per_pair=(t1 - t0) / k * 1e6,
                                   max_abs_diff_to_device=float(np.abs(np.asarray(host) - iou[:k].cpu().numpy()).max()))

    # ---- NMS
    for n in a.nms_sizes:
        for name, side in (('clustered', 12.0 * n ** 0.5), ('spread', 60.0 * n ** 0.5)):
            q = _boxes(rng, n, side)
            s = rng.random(n).astype(np.float32)
            lab = np.zeros(n, np.int32)
            qd, sd, ld, bd = up(q), up(s), up(lab), up(_aabb(q))
            sides = {'obb_nms': lambda: ops.obb_nms(qd, sd, ld, 0.25), 'nms_flat (axis-aligned bounds)':
                     lambda: ops.nms_flat(bd, sd, ld, 0.25)}
            res = _measure(sides, max(a.repeats // 2, 3), 1)
            doc['nms'][f'n={n} {name}'] = dict(ms=res, kept=int(ops.obb_nms(qd, sd, ld, 0.25).shape[0]),
                                               kept_axis_aligned=int(ops.nms_flat(bd, sd, ld, 0.25).shape[0]),
                                               pairs_passing_the_bounds_prefilter=_overlap_share(q))
    # ---- the obb metric beside segm
    if a.metric_images > 0:
        import argparse as _ap
        from bench_coco_iou_runs import THRS, tiles_load
        from rsprompter_amd import evaluation as E
        gt, dts = tiles_load(_ap.Namespace(images=a.metric_images), dev)
        img_ids, cat_ids = [im['id'] for im in gt['images']], [c['id'] for c in gt['categories']]

        def run(iou_type):
            tm = {}
            ev = E.device_evaluate(gt, dts, iou_type, img_ids, cat_ids, THRS, [100, 300, 1000], dev, timings=tm, iou_domain='runs')
            torch.cuda.synchronize()
            return ev, tm
        first = {t: run(t)[0] for t in ('segm', 'obb')}                              # the warm-up
        ms = dict(segm=[], obb=[])
        for _ in range(a.metric_repeats):
            for t in ms:
                ms[t].append(run(t)[1]['device'] * 1e3)
        doc['metric'] = dict(images=a.metric_images, detections=len(dts), ground_truths=len(gt['annotations']),
                             clock="device_evaluate timings['device']: host perf_counter, the window ends with a device-to-host copy",
                             device_ms={t: _stats(v) for t, v in ms.items()},
                             mAP={t: float(first[t].stats[0]) for t in first}, mAP_50={t: float(first[t].stats[1]) for t in first})
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
