"""Measurements of run-domain connected components on one GPU: rle.runs_components, rle.clean_runs(min_area=100,
'both') and rle.split_runs + rle.runs_to_obb, beside ops.rle_bbox on the same run table and the route a user had before: every
instance decoded to a dense device mask (one at a time: a mask of the scene table is 73 MB), ops.remove_small_regions on it,
rle.encode_runs of the result.  Every side ends in a device synchronise (or on the host), so the clock is the host's around
it; the sides alternate in one run, after a warm-up of each; medians of --repeats (the dense route: of --dense-repeats).

  python tools/bench_run_components.py [--out profiles/run_components/run_components.json] [--repeats 10] [--dense-repeats 2]

The two tables of tools/bench_mask_polygons.py: the 300 tile instances shifted into an 8 192 x 9 000 scene and the eight
1 024 x 1 024 noise masks.  Per table also the runs, the column pieces and the components.  Where the dense route can encode
its result (rsp_mask_rle takes widths up to RSP_RLE_MAX_WIDTH) the two cleaned tables are compared for equality; where it
cannot, that is recorded and its time lacks the encoding.  Oriented boxes take sides up to 65 535, which both tables keep.
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

MIN_AREA = 100


def _clock_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def _decode(counts_row, n_row, H, W):
    """one row of a run table -> bool [H, W] on the device"""
    c = counts_row[:n_row].to(torch.int64)
    ones = (torch.arange(n_row, device=c.device) & 1).to(torch.bool)
    return torch.repeat_interleave(ones, c, output_size=H * W).view(W, H).t().contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'run_components', 'run_components.json'))
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--dense-repeats', type=int, default=2)
    a = ap.parse_args(argv)
    from bench_mask_polygons import _tables
    from rsprompter_amd import large_image, ops, rle
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, dense_repeats=a.dense_repeats, min_area=MIN_AREA,
               clock='host perf_counter around a device synchronise', tables={})
    for name, counts, n, size in _tables(dev):
        H, W = size
        n_host = n.cpu().tolist()
        can_encode = W <= large_image.MAX_PATCH_WIDTH

        def components():
            return rle.runs_components(counts, n, size)

        def clean():
            return rle.clean_runs(counts, n, size, MIN_AREA, 'both')

        def split_obb():
            sc, sn, _, _, _ = rle.split_runs(counts, n, size)
            return rle.runs_to_obb(sc, sn, size)

        def bbox():
            return ops.rle_bbox(counts, n, H, W)

        def dense_route():
            rows, infos = [], []
            for i, ni in enumerate(n_host):
                mask = _decode(counts[i], ni, H, W) if ni > 0 else torch.zeros((H, W), dtype=torch.bool, device=dev)
                out, info = ops.remove_small_regions(mask[None], MIN_AREA, 'both')
                infos.append(info[0])
                if can_encode:
                    rows.append(rle.encode_runs(out)[:2])
            infos = torch.stack(infos)
            ops.check_region_status(infos[:, 7].cpu().tolist())
            return rows, infos[:, :2].contiguous()
        sides = dict(runs_components=components, clean_runs=clean, split_runs_runs_to_obb=split_obb, rle_bbox=bbox)
        for f in sides.values():
            f()
        dense_route()
        ms = {key: [] for key in sides}
        dense_ms = []
        for it in range(a.repeats):
            for key, f in sides.items():
                ms[key].append(_clock_ms(f)[0])
            if it < a.dense_repeats:
                t, dense = _clock_ms(dense_route)
                dense_ms.append(t)
        comps = components()
        cc, cn, _, _, changed = clean()
        agree = bool(torch.equal(changed, dense[1]))
        if can_encode:
            for i, (dc, dn) in enumerate(dense[0]):
                w = int(cn[i])
                agree = agree and int(dn[0]) == w and bool(torch.equal(dc[0, :w], cc[i, :w]))
        per = (comps.comp_offs[1:] - comps.comp_offs[:-1]).cpu().numpy()
        entry = dict(instances=int(n.shape[0]), canvas=list(size), runs=int(n.clamp(min=0).sum()),
                     pieces=int(comps.piece_comp.shape[0]),
                     components=dict(total=int(per.sum()), max=int(per.max()), median=float(np.median(per))),
                     changed=dict(holes=int(changed[:, 0].sum()), islands=int(changed[:, 1].sum())),
                     runs_after_cleaning=int(cn.clamp(min=0).sum()),
                     ms={key: _stats(v) for key, v in ms.items()}, dense_route_ms=_stats(dense_ms),
                     dense_route_encodes=bool(can_encode), device_equals_dense_route=agree)
        entry['dense_route_over_clean_runs'] = entry['dense_route_ms']['median'] / entry['ms']['clean_runs']['median']
        doc['tables'][name] = entry
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
