"""Measurements of polygon simplification on one GPU: rle.simplify_polygons beside rle.runs_to_polygons on the
same run table, and the time to per-instance ring lists on the host (rle.polygons_to_lists) with and without it.  Every
side ends in a device synchronise (or on the host), so the clock is the host's around it; the sides alternate in one run,
after a warm-up of each; medians of --repeats.

  python tools/bench_ring_simplify.py [--out profiles/ring_simplify/ring_simplify.json] [--repeats 10]

Three tables: the 300 tile instances shifted into an 8 192 x 9 000 scene and the eight 1 024 x 1 024 noise masks of
tools/bench_mask_polygons.py, and the scene again with every instance replaced by a disc or a rotated rectangle, whose
outlines are real staircases.  Tolerances 0.5, 1.0 and 2.0.  Per table and tolerance: vertices and rings before and after,
the rounds of the deepest ring; at tolerance 1.0 also the launch alternatives of rsp_ring_simplify_mark (block size 128 /
256 / 512, every ring through the block path), whose results are compared for equality.  Prints and writes one JSON
document; nothing else is asserted."""
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

TOLERANCES = (0.5, 1.0, 2.0)
VARIANTS = {'wave64_block256': 0, 'wave64_block128': 1, 'wave64_block512': 2, 'block256_only': 3}


def _clock_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def shape_tiles(k=300, th=128, tw=128, seed=301):
    """k tile masks, discs and rotated rectangles in turn: outlines that are staircases"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:th, :tw].astype(np.float64)
    out = np.zeros((k, th, tw), bool)
    for i in range(k):
        cx, cy = rng.uniform(0.4 * tw, 0.6 * tw), rng.uniform(0.4 * th, 0.6 * th)
        if i % 2 == 0:
            out[i] = (xx - cx) ** 2 + (yy - cy) ** 2 <= rng.uniform(0.15 * tw, 0.38 * tw) ** 2
        else:
            t = rng.uniform(0, np.pi)
            u, v = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t), -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
            out[i] = (abs(u) <= rng.uniform(0.15 * tw, 0.36 * tw)) & (abs(v) <= rng.uniform(0.08 * th, 0.25 * th))
    return out


def _tables(dev):
    from bench_mask_polygons import _tables as export_tables
    from rsprompter_amd import rle
    yield from export_tables(dev)
    rng = np.random.default_rng(300)
    th, tw, H, W, k = 128, 128, 8192, 9000, 300
    offs = np.stack([rng.integers(0, W - tw + 1, k), rng.integers(0, H - th + 1, k)], 1).astype(np.int32)
    counts, n, _, _ = rle.encode_runs(torch.from_numpy(shape_tiles(k, th, tw)).to(dev))
    sc, sn, _, _ = rle.shift_runs(counts, n, torch.from_numpy(offs).to(dev), (th, tw), (H, W))
    yield 'scene_300_discs_and_rectangles_8192x9000', sc, sn, (H, W)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ring_simplify', 'ring_simplify.json'))
    ap.add_argument('--repeats', type=int, default=10)
    a = ap.parse_args(argv)
    from rsprompter_amd import ops, rle
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, clock='host perf_counter around a device synchronise',
               tables={})
    for name, counts, n, size in _tables(dev):
        polys = rle.runs_to_polygons(counts, n, size)
        lengths = polys[1][1:] - polys[1][:-1]
        entry = dict(instances=int(n.shape[0]), canvas=list(size), rings=int(polys[2].shape[0]), vertices=int(polys[0].shape[0]),
                     longest_ring=int(lengths.max()), rings_over_64_vertices=int((lengths > 64).sum()),
                     vertices_in_rings_over_64=int(lengths[lengths > 64].sum()), tolerances={})

        def trace():
            return rle.runs_to_polygons(counts, n, size)

        def exact_lists():
            return rle.polygons_to_lists(*rle.runs_to_polygons(counts, n, size))
        for tol in TOLERANCES:
            def simplify():
                return rle.simplify_polygons(polys, size, tol)

            def simple_lists():
                return rle.polygons_to_lists(*rle.simplify_polygons(rle.runs_to_polygons(counts, n, size), size, tol)[0])
            sides = dict(trace_device=trace, simplify_device=simplify, lists_exact=exact_lists, lists_simplified=simple_lists)
            for f in sides.values():
                f()
            ms = {key: [] for key in sides}
            for _ in range(a.repeats):
                for key, f in sides.items():
                    ms[key].append(_clock_ms(f)[0])
            q8 = rle.polygon_tolerance_q8(tol)
            out = ops.ring_simplify(*polys, q8, 0, size[0], size[1], with_rounds=True)
            t = dict(tol2_q8=q8, rings_after=int(out[2].shape[0]), vertices_after=int(out[0].shape[0]),
                     deepest_ring_rounds=int(out[7].max()) if out[7].numel() else 0,
                     ms={key: dict(median=float(np.median(v)), min=float(np.min(v))) for key, v in ms.items()})
            if tol == 1.0:
                alt = {key: (lambda v=v: ops.ring_simplify(*polys, q8, 0, size[0], size[1], variant=v)) for key, v in VARIANTS.items()}
                same = all(all(torch.equal(x, y) for x, y in zip(f(), out[:7])) for f in alt.values())          # and the warm-up
                ams = {key: [] for key in alt}
                for _ in range(a.repeats):
                    for key, f in alt.items():
                        ams[key].append(_clock_ms(f)[0])
                t['launch_alternatives_ms'] = {key: dict(median=float(np.median(v)), min=float(np.min(v))) for key, v in ams.items()}
                t['launch_alternatives_agree'] = bool(same)
            entry['tolerances'][str(tol)] = t
        doc['tables'][name] = entry
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
