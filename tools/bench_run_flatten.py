"""Planar instance layers in the run domain against what could be done before them, in one process on one GPU.

    python tools/bench_run_flatten.py [--only ab] [--repeats 5] [--no-baselines] [--out FILE]

(a) the 8 192 x 9 000 synthetic scene of tools/bench_coco_iou_runs.py `scene_load`: its 300 ground-truth instances and the
    300 detections that are the same instances moved by up to six pixels, one table of 600 rows in which every instance
    overlaps its copy; a random rank.
(b) eight 1 024 x 1 024 noise masks (half the pixels set, about half a million runs each): every pixel is covered about
    four deep, every column holds thousands of pieces.
Per load: rle.flatten_runs (time, peak device memory, runs in and out) and rle.runs_to_labels on its result.
Baseline, the route a user had without the kernels: every row decoded to a dense mask (rle.runs_to_dense), the best rank per
pixel kept in an [H, W] map one instance at a time (the argmax of score x mask without holding [k, H, W]), each instance's
share cut out of the map and encoded again (rle.encode_runs).  Where a stage cannot run -- rsp_mask_rle refuses the width of
the scene -- that is recorded as the result and the stages before it are timed alone.  On (b) the two routes are compared
(==) before anything is timed.  Clock: host perf_counter around a device synchronise; one warm-up, then medians of
`--repeats` with the range."""
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
from bench_run_morphology import _rows_equal, _timed  # noqa: E402


def dense_route(counts, n, size, rank, encode=True):
    """decode -> per-pixel best rank -> (encode) -> (counts, n) of the flattened rows, or the [H, W] map of winners"""
    from rsprompter_amd import rle
    k, dev = int(n.shape[0]), n.device
    best = torch.full(size, k, dtype=torch.int32, device=dev)
    for i in range(k):
        m = rle.runs_to_dense(counts[i:i + 1].contiguous(), n[i:i + 1].contiguous(), size)[0]
        best = torch.where(m & (best > rank[i]), rank[i].to(torch.int32), best)
    if not encode:
        return best
    tables, ns = [], []
    for i in range(k):
        c, m, _, _ = rle.encode_runs((best == rank[i])[None], max(int(counts.shape[1]), 4096))
        tables.append(c)
        ns.append(m)
    return rle.concat_runs(tables), torch.cat(ns)


def measure(a, counts, n, size, dev, seed):
    from rsprompter_amd import rle
    k = int(n.shape[0])
    rank_np = np.random.default_rng(seed).permutation(k).astype(np.int32)
    rank = torch.from_numpy(rank_np).to(dev)
    out = dict(masks=k, canvas=list(size), runs_in=int(n.sum()))
    flat = lambda: rle.flatten_runs(counts, n, size, rank_np)                        # noqa: E731
    got, ms, peak = _timed(flat, a.repeats)
    out['flatten_run_domain'] = dict(ms=ms, peak_bytes=peak, runs_out=int(got[1].sum()), cap_out=int(got[2]),
                                     pixels_before=int(got[3].to(torch.int64).sum()), pixels_after=int(got[4].to(torch.int64).sum()))
    _, ms_l, peak_l = _timed(lambda: rle.runs_to_labels(got[0], got[1], size), a.repeats)
    out['label_map_from_runs'] = dict(ms=ms_l, peak_bytes=peak_l)
    if a.no_baselines:
        return out
    try:
        want, ms_d, peak_d = _timed(lambda: dense_route(counts, n, size, rank), min(a.repeats, 2))
        out['dense_route'] = dict(ms=ms_d, peak_bytes=peak_d, equal=_rows_equal(got[:2], want))
        assert out['dense_route']['equal']
        out['dense_over_run_domain_time'] = ms_d['median'] / ms['median']
    except (ValueError, RuntimeError) as e:                       # a size refusal of rsp_mask_rle, or memory
        out['dense_route'] = dict(refused=f'{type(e).__name__}: {e}'[:300])
        best, ms_d, peak_d = _timed(lambda: dense_route(counts, n, size, rank, encode=False), 1)
        labels = rle.runs_to_labels(got[0], got[1], size, rank_np + 1)
        out['dense_route_without_encode'] = dict(ms=ms_d, peak_bytes=peak_d,
                                                 equal=bool(torch.equal(torch.where(best == k, 0, best + 1), labels)))
        assert out['dense_route_without_encode']['equal']
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'run_flatten', 'run_flatten.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', default='ab', help='which of the two loads to run')
    ap.add_argument('--no-baselines', action='store_true')
    a = ap.parse_args(argv)
    from rsprompter_amd import rle
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats,
               clock='host perf_counter around a device synchronise; one warm-up, medians with the range')
    if 'a' in a.only:
        gt, dts, _ = base.scene_load(a, dev)
        strings = [g['segmentation']['counts'] for g in gt['annotations']] + [d['segmentation']['counts'] for d in dts]
        counts, n = rle.strings_to_runs(strings, dev)
        doc['a_scene_8192x9000'] = measure(a, counts, n, (8192, 9000), dev, 1)
        del gt, dts, counts, n
    if 'b' in a.only:
        g = torch.Generator().manual_seed(8)
        masks = (torch.rand((8, 1024, 1024), generator=g) < 0.5).to(dev)
        counts, n, _, _ = rle.encode_runs(masks, 1 << 20)
        doc['b_noise_8x1024x1024'] = measure(a, counts, n, (1024, 1024), dev, 2)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return doc


if __name__ == '__main__':
    main(sys.argv[1:])
