"""Run-domain boundary bands and the `boundary` metric against what could be done before them, in one
process on one GPU.

    python tools/bench_run_morphology.py [--only abc] [--images 1000] [--repeats 5] [--no-baselines] [--out FILE]

(a) DESIGN §13's load (tools/bench_coco_iou_runs.py `tiles_load`): `--images` images of 512 x 512, 100 detections and 50
    ground truths each, band width d = 14.
(b) the 300 + 300 masks of the 8 192 x 9 000 scene (`scene_load`), d = 243.
(c) 16 instances about 2 000 pixels across on the same canvas, bands and erosions at d = 14 ... 243: the instances of (b)
    are smaller than their band (the erosion is empty and the work ends early), these are not.
Per load: the bands alone (ops.rle_boundary on the run table of all masks: time and peak device memory), the whole
`boundary` metric next to `segm` as device_evaluate's timings split it, and for (b) the band time at d = 14 ... 243 on the
same table (the design claim: it grows with log d).
Baselines, what a user could do without the run-domain kernels:
  dense device route -- the run table decoded to dense masks in chunks, the mask inside a ring of d zeros, 1 - max_pool(1 - m)
    over 2 d + 1 rows and then columns (stride 1), mask & ~eroded, rle.encode_runs; every mask on (a); on (b) a sample,
    scaled, and without the encode, which rsp_mask_rle refuses at that size;
  host route -- scipy.ndimage.binary_erosion(iterations=d) on a sample of `--host-sample` masks, scaled ((b): off unless
    `--host-sample-scene` asks, one scene-sized mask takes minutes).
The band tables of the dense route and of ops.rle_boundary are compared (==) before anything is timed.  Clock: host
perf_counter around a device synchronise; one warm-up, then medians of `--repeats` with the range.  `--no-baselines
--repeats 1` under `rocprofv3 --kernel-trace --stats` gives the per-kernel times."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import bench_coco_iou_runs as base  # noqa: E402

_stats = base._stats


def _timed(fn, repeats):
    """one warm-up, then `repeats` runs -> (last result, ms stats, peak bytes above what was allocated before)"""
    out = fn()
    ms, peak = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        peak.append(torch.cuda.max_memory_allocated() - held)
    return out, _stats(ms), int(max(peak))


def _rows_equal(a, b):
    (ca, na), (cb, nb) = a, b
    if not torch.equal(na, nb):
        return False
    w = int(na.max())
    live = torch.arange(w, device=na.device)[None] < na[:, None]
    return bool(((ca[:, :w] == cb[:, :w]) | ~live).all())


def dense_bands(counts, n, size, d, chunk, encode=True):
    """the dense device route -> (counts, n) of the bands, rows in order; encode=False: the dense bands of the last chunk
    (rsp_mask_rle refuses a scene-sized dense mask: the route ends there)"""
    from rsprompter_amd import rle
    import torch.nn.functional as F
    tables, ns = [], []
    for s in range(0, int(n.shape[0]), chunk):
        m = rle.runs_to_dense(counts[s:s + chunk].contiguous(), n[s:s + chunk].contiguous(), size)
        inv = 1 - F.pad(m.to(torch.float16), (d, d, d, d), value=0.0)[:, None]      # the outside of the image is background
        inv = F.max_pool2d(F.max_pool2d(inv, (2 * d + 1, 1), stride=1), (1, 2 * d + 1), stride=1)[:, 0]
        if not encode:
            last = m & (inv > 0.5)
            continue
        c, k, _, _ = rle.encode_runs(m & (inv > 0.5))
        tables.append(c)
        ns.append(k)
    return (rle.concat_runs(tables), torch.cat(ns)) if encode else last


def host_bands(counts, n, size, d, sample):
    """scipy on `sample` masks -> seconds per mask (decode and encode not counted)"""
    from scipy import ndimage as ndi
    from rsprompter_amd import rle
    idx = np.linspace(0, int(n.shape[0]) - 1, sample).astype(np.int64)
    sec = []
    for i in idx.tolist():
        m = rle.runs_to_dense(counts[i:i + 1].contiguous(), n[i:i + 1].contiguous(), size)[0].cpu().numpy()
        t0 = time.perf_counter()
        m & ~ndi.binary_erosion(m, np.ones((3, 3), bool), iterations=d, border_value=0)
        sec.append(time.perf_counter() - t0)
    return float(np.median(sec))


def measure(a, gt, dts, dev, size, d, chunk, dense_sample, host_sample, radii=()):
    from rsprompter_amd import evaluation as E
    from rsprompter_amd import ops, rle
    segms = [x['segmentation'] for x in dts] + [g['segmentation'] for g in gt['annotations']]
    counts, n = rle.strings_to_runs([s['counts'] for s in segms], dev)
    k = int(n.shape[0])
    out = dict(masks=k, canvas=list(size), d=d, runs_per_mask=float(n.sum()) / k)
    band = lambda r=d: ops.rle_boundary(counts, n, size[0], size[1], r)[:2]         # noqa: E731
    got, ms, peak = _timed(band, a.repeats)
    out['bands_run_domain'] = dict(ms=ms, peak_bytes=peak, band_runs_per_mask=float(got[1].sum()) / k)
    if radii:
        out['bands_by_radius_ms'] = {str(r): _timed(lambda r=r: band(r), a.repeats)[1] for r in radii}
    if not a.no_baselines:
        ks = k if dense_sample is None else min(dense_sample, k)
        sub = (counts[:ks].contiguous(), n[:ks].contiguous())
        encode = dense_sample is None
        dense = lambda: dense_bands(sub[0], sub[1], size, d, chunk, encode)          # noqa: E731
        want, ms_d, peak_d = _timed(dense, min(a.repeats, 2) if encode else 1)
        if encode:
            out['bands_equal_dense_route'] = _rows_equal((got[0][:ks], got[1][:ks]), want)
        else:                                                    # the last mask of the sample, pixel by pixel
            mine = rle.runs_to_dense(got[0][ks - 1:ks].contiguous(), got[1][ks - 1:ks].contiguous(), size)
            out['bands_equal_dense_route'] = bool(torch.equal(mine, want))
            out['dense_route_ends_before_encode'] = True
        assert out['bands_equal_dense_route']
        out['bands_dense_device'] = dict(ms=ms_d, peak_bytes=peak_d, masks_measured=ks, chunk=chunk,
                                         ms_scaled_to_all=ms_d['median'] * k / ks)
        if host_sample:
            sec = host_bands(counts, n, size, d, host_sample)
            out['bands_host_scipy'] = dict(sample=host_sample, seconds_per_mask=sec, seconds_scaled_to_all=sec * k)
        out['dense_over_run_domain_time'] = out['bands_dense_device']['ms_scaled_to_all'] / ms['median']
    # the whole metric
    img_ids, cat_ids = [im['id'] for im in gt['images']], [c['id'] for c in gt['categories']]

    def metric(iou_type):
        def run():
            tm = {}
            ev = E.device_evaluate(gt, dts, iou_type, img_ids, cat_ids, base.THRS, [100, 300, 1000], dev, timings=tm,
                                   iou_domain='runs')
            metric.tm, metric.stats = tm, ev.stats
            return ev
        _, ms, peak = _timed(run, a.repeats)
        tm = {k: (v * 1e3 if isinstance(v, float) else v) for k, v in metric.tm.items()}
        return dict(total_ms=ms, peak_bytes=peak, last_run_split_ms=tm, mAP=float(metric.stats[0]))
    out['metric_segm'] = metric('segm')
    out['metric_boundary'] = metric('boundary')
    return out


def large_instances(a, dev):
    """(c): 16 instances of about 2 000 pixels across on the 8 192 x 9 000 canvas, which an erosion by 243 does not empty
    (the 128-pixel instances of (b) are all band at d = 243: their erosion is empty after the first window doublings)"""
    from scipy import ndimage
    from rsprompter_amd import ops, rle
    rng = np.random.default_rng(301)
    t, H, W, k = 2048, 8192, 9000, 16
    f = ndimage.gaussian_filter(rng.random((k, t, t)).astype(np.float32), (0, 48, 48))
    yy, xx = np.mgrid[:t, :t]
    disc = ((yy - t / 2) ** 2 + (xx - t / 2) ** 2) < (0.47 * t) ** 2           # one large body with a ragged outline and holes
    tiles = torch.from_numpy((f > np.quantile(f, 0.3)) & disc[None]).to(dev)
    offs = np.stack([rng.integers(0, W - t + 1, k), rng.integers(0, H - t + 1, k)], 1).astype(np.int32)
    counts, n, _, _ = rle.encode_runs(tiles)
    sc, sn, _, _ = rle.shift_runs(counts, n, torch.from_numpy(offs).to(dev), (t, t), (H, W))
    out = dict(masks=k, canvas=[H, W], runs_per_mask=float(sn.sum()) / k, by_radius={})
    for r in (14, 29, 61, 122, 243):
        band = lambda r=r: ops.rle_boundary(sc, sn, H, W, r)[:2]                     # noqa: E731
        erode = lambda r=r: ops.rle_erode(sc, sn, H, W, r)[:2]                       # noqa: E731
        got, ms, peak = _timed(band, a.repeats)
        er, ms_e, _ = _timed(erode, a.repeats)
        out['by_radius'][str(r)] = dict(levels=ops.run_morph_levels(r, W), band_ms=ms, erode_ms=ms_e, peak_bytes=peak,
                                        band_runs_per_mask=float(got[1].sum()) / k, eroded_runs_per_mask=float(er[1].sum()) / k)
    if not a.no_baselines:                                       # one mask, pixel by pixel, at the widest band
        want = dense_bands(sc[:1].contiguous(), sn[:1].contiguous(), (H, W), 243, 1, encode=False)
        mine = rle.runs_to_dense(got[0][:1].contiguous(), got[1][:1].contiguous(), (H, W))
        out['band_243_equal_dense_route'] = bool(torch.equal(mine, want))
        assert out['band_243_equal_dense_route']
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'run_morphology', 'run_morphology.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--images', type=int, default=1000)
    ap.add_argument('--only', default='abc', help='which of the three loads to run')
    ap.add_argument('--no-baselines', action='store_true')
    ap.add_argument('--host-sample', type=int, default=20, help='masks of load (a) through scipy')
    ap.add_argument('--host-sample-scene', type=int, default=0,
                    help='masks of load (b) through scipy: 243 iterations on 74 M pixels take minutes each, off by default')
    a = ap.parse_args(argv)
    from rsprompter_amd import rle
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats,
               clock='host perf_counter around a device synchronise; one warm-up, medians with the range')
    if 'a' in a.only:
        gt, dts = base.tiles_load(a, dev)
        doc['a_tiles_512'] = dict(images=a.images, **measure(a, gt, dts, dev, (512, 512), rle.boundary_radius((512, 512)),
                                                             chunk=1500, dense_sample=None, host_sample=a.host_sample))
        del gt, dts
    if 'b' in a.only:
        gt, dts, _ = base.scene_load(a, dev)
        size = (8192, 9000)
        doc['b_scene_8192x9000'] = measure(a, gt, dts, dev, size, rle.boundary_radius(size), chunk=1, dense_sample=2, host_sample=a.host_sample_scene,
                                           radii=(14, 29, 61, 122, 243))
    if 'c' in a.only:
        doc['c_large_instances_8192x9000'] = large_instances(a, dev)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return doc


if __name__ == '__main__':
    main(sys.argv[1:])
