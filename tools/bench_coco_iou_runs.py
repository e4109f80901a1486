"""Run-domain mask IoU against the bits route: the device part of the segm evaluation -- strings to IoU to
match, `device_evaluate`'s timings['device'] -- and the peak device memory of each route, both in one process on one GPU.

    python tools/bench_coco_iou_runs.py [--only ab] [--routes bits,runs] [--images 1000] [--repeats 5] [--out FILE]

(a) DESIGN §13's load: `--images` images of 512 x 512, 100 detections and 50 ground truths each (ellipses, two categories;
    the detections are jittered ground truths and spurious ones).
(b) a scene: 300 detections x 300 ground truths on 8 192 x 9 000, the instances of tools/bench_poly_raster.py's scene (b)
    (tools/bench_mask_polygons.py `_tables`), the detections the same tiles moved by a few pixels.  The bits route holds
    about 5.5 GB there.
Clock: host perf_counter around a device synchronise (inside device_evaluate the window ends with the copy of the match
tables to the host); one warm-up, then medians of `--repeats` with the range.  The IoU arrays of the two routes are compared
(==) before anything is timed.  The share of pairs that survive the extent filter is reported: it decides whether a tight-box
prefilter is worth a canvas height per row.  `--routes runs --repeats 1` under `rocprofv3 --kernel-trace --stats` gives the
walk kernel's time alone."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

THRS = np.linspace(.5, 0.95, 10)


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))


def _ellipses(p, S, dev):
    """p float32 [k, 4] = (cx, cy, rx, ry) -> bool [k, S, S] on the device"""
    yy, xx = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float32), torch.arange(S, device=dev, dtype=torch.float32),
                            indexing='ij')
    p = p.to(dev)[:, :, None, None]
    return ((xx[None] - p[:, 0]) / p[:, 2]) ** 2 + ((yy[None] - p[:, 1]) / p[:, 3]) ** 2 <= 1.0


def tiles_load(a, dev):
    """-> (gt dict, loadRes'd detections): a.images images of 512^2, 50 gts and 100 dts each"""
    from rsprompter_amd import rle
    S, rng = 512, np.random.default_rng(13)
    images, anns, dts = [], [], []
    for i in range(a.images):
        g = np.concatenate([rng.uniform(30, S - 30, (50, 2)), rng.uniform(6, 36, (50, 2))], 1).astype(np.float32)
        d = np.concatenate([g + rng.normal(0, 2, g.shape).astype(np.float32), np.concatenate(
            [rng.uniform(30, S - 30, (50, 2)), rng.uniform(6, 36, (50, 2))], 1).astype(np.float32)])
        d[:, 2:] = np.maximum(d[:, 2:], 2)
        masks = _ellipses(torch.from_numpy(np.concatenate([g, d])), S, dev)
        counts, n, _, _ = rle.encode_runs(masks)
        strings = rle.runs_to_strings(counts, n, (S, S))
        area = masks.view(150, -1).sum(1).tolist()
        images.append(dict(id=i + 1, height=S, width=S, file_name=f'{i}.png'))
        for j in range(50):
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=1 + j % 2, area=float(area[j]), iscrowd=int(j == 49),
                             bbox=[0, 0, 1, 1], segmentation=strings[j]))
        for j in range(100):
            dts.append(dict(id=len(dts) + 1, image_id=i + 1, category_id=1 + (j % 50) % 2, score=float(rng.random()), iscrowd=0,
                            segmentation=strings[50 + j]))
    return dict(images=images, annotations=anns, categories=[dict(id=1, name='a'), dict(id=2, name='b')]), dts


def scene_load(a, dev):
    from scipy import ndimage
    from rsprompter_amd import rle
    rng = np.random.default_rng(300)
    th, tw, H, W, k = 128, 128, 8192, 9000, 300
    f = ndimage.gaussian_filter(rng.random((k, th, tw)), (0, 3, 3))
    tiles = torch.from_numpy(f > np.quantile(f, 0.55)).to(dev)
    offs = np.stack([rng.integers(0, W - tw + 1, k), rng.integers(0, H - th + 1, k)], 1).astype(np.int32)
    jit = np.clip(offs + rng.integers(-6, 7, offs.shape), 0, [W - tw, H - th]).astype(np.int32)
    counts, n, _, _ = rle.encode_runs(tiles)
    out = []
    for o in (offs, jit):
        sc, sn, _, _ = rle.shift_runs(counts, n, torch.from_numpy(o).to(dev), (th, tw), (H, W))
        out.append((rle.runs_to_strings(sc, sn, (H, W)), int(sn.sum())))
    (gs, g_runs), (ds, d_runs) = out
    area = tiles.view(k, -1).sum(1).tolist()
    anns = [dict(id=j + 1, image_id=1, category_id=1, area=float(area[j]), iscrowd=0, bbox=[0, 0, 1, 1], segmentation=gs[j])
            for j in range(k)]
    dts = [dict(id=j + 1, image_id=1, category_id=1, score=float(rng.random()), iscrowd=0, segmentation=ds[j]) for j in range(k)]
    gt = dict(images=[dict(id=1, height=H, width=W, file_name='scene.png')], annotations=anns, categories=[dict(id=1, name='a')])
    return gt, dts, dict(canvas=[H, W], runs_per_mask=(g_runs + d_runs) / (2 * k))


def measure(a, gt, dts, dev):
    from rsprompter_amd import evaluation as E
    img_ids, cat_ids = [im['id'] for im in gt['images']], [c['id'] for c in gt['categories']]
    routes = a.routes.split(',')

    def run(route, keep=False):
        tm = {}
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ev = E.device_evaluate(gt, dts, 'segm', img_ids, cat_ids, THRS, [100, 300, 1000], dev, timings=tm, iou_domain=route,
                               keep_iou=keep)
        torch.cuda.synchronize()
        tm['peak_bytes'] = torch.cuda.max_memory_allocated() - base
        return ev, tm
    first = {r: run(r, keep=True) for r in routes}                     # the warm-up, and the comparison
    out = dict(detections=len(dts), ground_truths=len(gt['annotations']))
    if len(routes) == 2:
        x, y = (first[r][0].tables['iou'] for r in routes)
        out['iou_equal'] = bool(torch.equal(x.view(torch.int64), y.view(torch.int64)))
        out['stats_equal'] = bool(np.array_equal(first[routes[0]][0].stats, first[routes[1]][0].stats))
        assert out['iou_equal'] and out['stats_equal']
        out['pairs_with_iou_above_zero'] = int((x > 0).sum())
    del first
    for r in routes:
        ms, peak, tm = [], [], {}
        for _ in range(a.repeats):
            _, tm = run(r)
            ms.append(tm['device'] * 1e3)
            peak.append(tm['peak_bytes'])
        out[r] = dict(device_ms=_stats(ms), peak_bytes=int(max(peak)))
        if r == 'runs':
            out['pairs'], out['survivors'] = tm['pairs'], tm['survivors']
            out['survivor_share'] = tm['survivors'] / max(tm['pairs'], 1)
    if len(routes) == 2:
        out['bits_over_runs_time'] = out['bits']['device_ms']['median'] / out['runs']['device_ms']['median']
        out['bits_over_runs_memory'] = out['bits']['peak_bytes'] / max(out['runs']['peak_bytes'], 1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_iou_runs', 'coco_iou_runs.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--images', type=int, default=1000)
    ap.add_argument('--only', default='ab', help='which of the two measurements to run')
    ap.add_argument('--routes', default='bits,runs')
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, routes=a.routes,
               clock="device_evaluate's timings['device']: host perf_counter, strings on the host to match tables on the host")
    if 'a' in a.only:
        gt, dts = tiles_load(a, dev)
        doc['a_tiles_512'] = dict(images=a.images, **measure(a, gt, dts, dev))
        del gt, dts
    if 'b' in a.only:
        gt, dts, info = scene_load(a, dev)
        doc['b_scene_8192x9000'] = dict(info, **measure(a, gt, dts, dev))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return doc


if __name__ == '__main__':
    main(sys.argv[1:])
