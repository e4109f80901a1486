"""Measurements of polygon export on one GPU: the polygon stage -- run table to per-instance ring lists on
the host, rle.runs_to_polygons + rle.polygons_to_lists -- beside rle.runs_to_strings on the same table, the cost users pay
today for the RLE form.  Both end on the host, so the clock is the host's around a device synchronise; the two sides
alternate in one run, after a warm-up of each.

  python tools/bench_mask_polygons.py [--out profiles/mask_polygons/mask_polygons.json] [--repeats 10]

Two tables: the 300 tile instances shifted into an 8 192 x 9 000 scene (rsp_rle_shift's table, the large-scene case) and
eight 1 024 x 1 024 noise masks of about 55 000 runs each (the tests/test_gpu_mask_polygons.py inputs).  Prints and writes
one JSON document with the ring and vertex counts; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _clock_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _tables(dev):
    from scipy import ndimage
    from rsprompter_amd import rle
    rng = np.random.default_rng(300)
    th, tw, H, W, k = 128, 128, 8192, 9000, 300
    f = ndimage.gaussian_filter(rng.random((k, th, tw)), (0, 3, 3))
    tiles = torch.from_numpy(f > np.quantile(f, 0.55)).to(dev)
    offs = np.stack([rng.integers(0, W - tw + 1, k), rng.integers(0, H - th + 1, k)], 1).astype(np.int32)
    counts, n, _, _ = rle.encode_runs(tiles)
    sc, sn, _, _ = rle.shift_runs(counts, n, torch.from_numpy(offs).to(dev), (th, tw), (H, W))
    yield 'scene_300_instances_8192x9000', sc, sn, (H, W)
    rng = np.random.default_rng(1024)
    masks = []
    for i in range(8):
        f = ndimage.gaussian_filter(rng.random((1024, 1024)), 1.0)
        masks.append(f > np.quantile(f, 0.95 if i % 2 == 0 else 0.05))
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(np.stack(masks)).to(dev))
    yield 'noise_8_masks_1024x1024', counts, n, (1024, 1024)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mask_polygons', 'mask_polygons.json'))
    ap.add_argument('--repeats', type=int, default=10)
    a = ap.parse_args(argv)
    from rsprompter_amd import rle
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, clock='host perf_counter around a device synchronise',
               tables={})
    for name, counts, n, size in _tables(dev):
        def polygons():
            return rle.polygons_to_lists(*rle.runs_to_polygons(counts, n, size))

        def device_only():
            return rle.runs_to_polygons(counts, n, size)

        def strings():
            return rle.runs_to_strings(counts, n, size)
        for f in (polygons, device_only, strings):
            f()
        ms = dict(polygons=[], device_only=[], strings=[])
        for _ in range(a.repeats):
            for key, f in (('polygons', polygons), ('device_only', device_only), ('strings', strings)):
                ms[key].append(_clock_ms(f)[0])
        arrays = device_only()
        doc['tables'][name] = dict(
            instances=int(n.shape[0]), canvas=list(size), runs=int(n.clamp(min=0).sum()), widest_row=int(n.max()),
            rings=int(arrays[2].shape[0]), holes=int((arrays[4] < 0).sum()), vertices=int(arrays[0].shape[0]),
            string_bytes=sum(len(d['counts']) for d in strings()),
            polygons_to_host_ms=dict(median=float(np.median(ms['polygons'])), min=float(np.min(ms['polygons']))),
            polygons_device_arrays_ms=dict(median=float(np.median(ms['device_only'])), min=float(np.min(ms['device_only']))),
            runs_to_strings_ms=dict(median=float(np.median(ms['strings'])), min=float(np.min(ms['strings']))))
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
