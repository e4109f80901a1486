"""Measurements of oriented boxes on one GPU: rle.runs_to_obb with its two halves (ops.mask_hull,
ops.hull_min_rect) beside ops.rle_bbox on the same run table, and the route a user had before: rle.runs_to_polygons +
rle.polygons_to_lists + a hull and rotating calipers in Python (tests/_mask_obb_ref.py on the ring vertices of each instance).
Every side ends in a device synchronise (or on the host), so the clock is the host's around it; the sides alternate in one
run, after a warm-up of each; medians of --repeats (the Python route: of --host-repeats, it takes seconds).

  python tools/bench_mask_obb.py [--out profiles/mask_obb/mask_obb.json] [--repeats 10] [--host-repeats 3]

The two tables of tools/bench_mask_polygons.py: the 300 tile instances shifted into an 8 192 x 9 000 scene and the eight
1 024 x 1 024 noise masks.  Per table also the hull vertex counts and the pruning rounds (max, median).  The device boxes
are compared with the Python route's for equality.  Prints and writes one JSON document."""
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _clock_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mask_obb', 'mask_obb.json'))
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--host-repeats', type=int, default=3)
    a = ap.parse_args(argv)
    import _mask_obb_ref as oref
    from bench_mask_polygons import _tables
    from rsprompter_amd import ops, rle
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, host_repeats=a.host_repeats,
               clock='host perf_counter around a device synchronise', tables={})
    for name, counts, n, size in _tables(dev):
        hull = ops.mask_hull(counts, n, size[0], size[1], with_rounds=True)

        def obb():
            return rle.runs_to_obb(counts, n, size)

        def hull_only():
            return rle.runs_to_hulls(counts, n, size)

        def rect_only():
            return ops.hull_min_rect(hull[0], hull[1])

        def bbox():
            return ops.rle_bbox(counts, n, size[0], size[1])

        def obb_to_host():
            out = rle.runs_to_obb(counts, n, size)
            return rle.obb_to_numpy(out[3], out[4])

        def python_route():
            per_instance = rle.polygons_to_lists(*rle.runs_to_polygons(counts, n, size))
            out = []
            for rings in per_instance:
                pts = sorted(set(map(tuple, np.concatenate([r for r, _, _ in rings], 0).tolist()))) if rings else []
                ring = oref.hull_of_points(pts)
                out.append((ring,) + tuple(oref.min_rect(ring)[:2]))
            return out
        sides = dict(runs_to_obb=obb, mask_hull=hull_only, hull_min_rect=rect_only, rle_bbox=bbox, obb_to_numpy=obb_to_host)
        for f in sides.values():
            f()
        ms = {key: [] for key in sides}
        host_ms = []
        for it in range(a.repeats):
            for key, f in sides.items():
                ms[key].append(_clock_ms(f)[0])
            if it < a.host_repeats:
                t, host = _clock_ms(python_route)
                host_ms.append(t)
        dv, do, _, de, dq = (t.cpu().numpy() for t in obb())
        agree = all([tuple(v) for v in dv[do[i]:do[i + 1]].tolist()] == h[0] and (int(de[i]), tuple(dq[i].tolist())) == h[1:]
                    for i, h in enumerate(host))
        sizes = (hull[1][1:] - hull[1][:-1]).cpu().numpy()
        rounds = hull[3].cpu().numpy().max(0)
        entry = dict(instances=int(n.shape[0]), canvas=list(size), runs=int(n.clamp(min=0).sum()),
                     hull_vertices=dict(total=int(sizes.sum()), max=int(sizes.max()), median=float(np.median(sizes))),
                     pruning_rounds=dict(max=int(rounds.max()), median=float(np.median(rounds))),
                     ms={key: _stats(v) for key, v in ms.items()}, python_route_ms=_stats(host_ms),
                     device_equals_python_route=bool(agree))
        entry['python_route_over_runs_to_obb'] = entry['python_route_ms']['median'] / entry['ms']['obb_to_numpy']['median']
        doc['tables'][name] = entry
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
