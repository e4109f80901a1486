"""Euclidean buffers in the run domain against what could be done before them, in one process on one GPU.

    python tools/bench_run_disc.py [--only acs] [--images 1000] [--repeats 5] [--no-baselines] [--out FILE]

(a) DESIGN §13's load (tools/bench_coco_iou_runs.py `tiles_load`): `--images` images of 512 x 512, 100 detections and 50
    ground truths each, dilated and eroded by the disc of radius 14.
(c) DESIGN §14.13's load (c) (tools/bench_run_morphology.py `large_instances`' masks): 16 instances about 2 000 pixels across
    on 8 192 x 9 000, dilated and eroded at R = 14 ... 243 -- the honest place to show that the cost grows linearly with R.
(s) the 300 detections of the 8 192 x 9 000 scene (`scene_load`) through rle.buffer_runs at +3 and -3 pixels.
Baselines, what a user could do without the kernels:
  dense device route -- the run table decoded to dense masks in chunks, a convolution with the disc footprint (fp32: the
    sums are counts up to (2 R + 1)^2, exact), > 0, rle.encode_runs; every mask on (a), one mask without the encode on (c)
    at R = 14 (a (2 R + 1)^2 footprint on 74 M pixels: the larger radii are not run);
  host route -- scipy.ndimage.binary_dilation with the footprint on `--host-sample` masks of (a), scaled; on (c) one
    distance_transform_edt of one instance's bounding box grown by R, whose cost does not depend on R.
The results of the dense route and of ops.rle_dilate_disc are compared (==) before anything is timed.  Clock: host
perf_counter around a device synchronise; one warm-up, then medians of `--repeats` with the range.  `--no-baselines
--repeats 1` under `rocprofv3 --kernel-trace --stats` gives the per-kernel times."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import bench_coco_iou_runs as base  # noqa: E402
import bench_run_morphology as morph  # noqa: E402

_timed, _rows_equal = morph._timed, morph._rows_equal


def _footprint(r2, dev):
    R = math.isqrt(r2)
    d = torch.arange(-R, R + 1, device=dev)
    return ((d[:, None] ** 2 + d[None, :] ** 2) <= r2).to(torch.float32)[None, None]


def dense_dilate(counts, n, size, r2, chunk, encode=True):
    """the dense device route -> (counts, n) of the dilations, rows in order; encode=False: the dense result of the last chunk"""
    from rsprompter_amd import rle
    import torch.nn.functional as F
    fp = _footprint(r2, n.device)
    R = math.isqrt(r2)
    tables, ns = [], []
    for s in range(0, int(n.shape[0]), chunk):
        m = rle.runs_to_dense(counts[s:s + chunk].contiguous(), n[s:s + chunk].contiguous(), size)
        out = F.conv2d(m.to(torch.float32)[:, None], fp, padding=R)[:, 0] > 0.5
        if not encode:
            last = out
            continue
        c, k, _, _ = rle.encode_runs(out)
        tables.append(c)
        ns.append(k)
    return (rle.concat_runs(tables), torch.cat(ns)) if encode else last


def _ops(counts, n, size, r2, repeats):
    """dilation and erosion (border 0) of one table at one squared radius -> their stats"""
    from rsprompter_amd import ops, rle
    H, W = size
    hh = rle.half_heights('disc', r2=r2, size=size)[0]
    k = int(n.shape[0])
    got, ms, peak = _timed(lambda: ops.rle_dilate_disc(counts, n, H, W, hh)[:2], repeats)
    er, ms_e, peak_e = _timed(lambda: ops.rle_erode_disc(counts, n, H, W, hh, 0)[:2], repeats)
    return got, dict(R=math.isqrt(r2), dilate_ms=ms, dilate_peak_bytes=peak, erode_ms=ms_e, erode_peak_bytes=peak_e,
                     dilated_runs_per_mask=float(got[1].sum()) / k, eroded_runs_per_mask=float(er[1].sum()) / k)


def tiles(a, dev):
    from scipy import ndimage as ndi
    from rsprompter_amd import rle
    gt, dts = base.tiles_load(a, dev)
    segms = [x['segmentation'] for x in dts] + [g['segmentation'] for g in gt['annotations']]
    counts, n = rle.strings_to_runs([s['counts'] for s in segms], dev)
    k, size, r2 = int(n.shape[0]), (512, 512), 14 * 14
    got, out = _ops(counts, n, size, r2, a.repeats)
    out.update(masks=k, canvas=list(size), runs_per_mask=float(n.sum()) / k)
    if not a.no_baselines:
        want, ms_d, peak_d = _timed(lambda: dense_dilate(counts, n, size, r2, 1500), min(a.repeats, 2))
        out['dilate_equal_dense_route'] = _rows_equal(got, want)
        assert out['dilate_equal_dense_route']
        out['dilate_dense_device'] = dict(ms=ms_d, peak_bytes=peak_d, chunk=1500)
        out['dense_over_run_domain_time'] = ms_d['median'] / out['dilate_ms']['median']
        fp = _footprint(r2, 'cpu')[0, 0].numpy() > 0
        sec = []
        for i in np.linspace(0, k - 1, a.host_sample).astype(np.int64).tolist():
            m = rle.runs_to_dense(counts[i:i + 1].contiguous(), n[i:i + 1].contiguous(), size)[0].cpu().numpy()
            t0 = time.perf_counter()
            ndi.binary_dilation(m, fp)
            sec.append(time.perf_counter() - t0)
        out['dilate_host_scipy'] = dict(sample=a.host_sample, seconds_per_mask=float(np.median(sec)),
                                        seconds_scaled_to_all=float(np.median(sec)) * k)
    return out


def large_instances(a, dev):
    """(c): the 16 instances of tools/bench_run_morphology.py's load (c), by radius"""
    from scipy import ndimage
    from rsprompter_amd import rle
    rng = np.random.default_rng(301)
    t, H, W, k = 2048, 8192, 9000, 16
    f = ndimage.gaussian_filter(rng.random((k, t, t)).astype(np.float32), (0, 48, 48))
    yy, xx = np.mgrid[:t, :t]
    disc = ((yy - t / 2) ** 2 + (xx - t / 2) ** 2) < (0.47 * t) ** 2
    tiles_ = (f > np.quantile(f, 0.3)) & disc[None]
    offs = np.stack([rng.integers(0, W - t + 1, k), rng.integers(0, H - t + 1, k)], 1).astype(np.int32)
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(tiles_).to(dev))
    sc, sn, _, _ = rle.shift_runs(counts, n, torch.from_numpy(offs).to(dev), (t, t), (H, W))
    out = dict(masks=k, canvas=[H, W], runs_per_mask=float(sn.sum()) / k, by_radius={})
    first = None
    for R in (14, 29, 61, 122, 243):
        got, out['by_radius'][str(R)] = _ops(sc, sn, (H, W), R * R, a.repeats)
        first = first or got
    if not a.no_baselines:                                       # one mask, pixel by pixel, at R = 14
        want, ms_d, peak_d = _timed(lambda: dense_dilate(sc[:1].contiguous(), sn[:1].contiguous(), (H, W), 196, 1, encode=False), 1)
        mine = rle.runs_to_dense(first[0][:1].contiguous(), first[1][:1].contiguous(), (H, W))
        out['dilate_14_equal_dense_route'] = bool(torch.equal(mine, want))
        assert out['dilate_14_equal_dense_route']
        out['dilate_14_dense_device_one_mask'] = dict(ms=ms_d, peak_bytes=peak_d, ms_scaled_to_all=ms_d['median'] * k)
        pad = 243
        crop = np.pad(tiles_[0], pad)
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(~crop)
        sec = time.perf_counter() - t0
        out['host_scipy_edt_one_mask_box_grown_by_243'] = dict(seconds_per_mask=sec, seconds_scaled_to_all=sec * k)
    return out


def scene(a, dev):
    from rsprompter_amd import rle
    _, dts, _ = base.scene_load(a, dev)
    size = (8192, 9000)
    counts, n = rle.strings_to_runs([x['segmentation']['counts'] for x in dts], dev)
    k = int(n.shape[0])
    out = dict(masks=k, canvas=list(size), runs_per_mask=float(n.sum()) / k)
    for d in (3, -3):
        got, ms, peak = _timed(lambda d=d: rle.buffer_runs(counts, n, size, d)[:2], a.repeats)
        out[f'buffer_{d:+d}'] = dict(ms=ms, peak_bytes=peak, runs_per_mask=float(got[1].sum()) / k)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'run_disc', 'run_disc.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--images', type=int, default=1000)
    ap.add_argument('--only', default='acs', help='which of the loads to run: a, c, s')
    ap.add_argument('--no-baselines', action='store_true')
    ap.add_argument('--host-sample', type=int, default=20, help='masks of load (a) through scipy')
    a = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats,
               clock='host perf_counter around a device synchronise; one warm-up, medians with the range')
    if 'a' in a.only:
        doc['a_tiles_512'] = dict(images=a.images, **tiles(a, dev))
    if 'c' in a.only:
        doc['c_large_instances_8192x9000'] = large_instances(a, dev)
    if 's' in a.only:
        doc['s_scene_8192x9000_buffer'] = scene(a, dev)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return doc


if __name__ == '__main__':
    main(sys.argv[1:])
