"""Measurements of shared-border simplification on one GPU, beside the independent simplification of the same
rings (rle.simplify_polygons) measured in the same run.

    python tools/bench_ring_coverage.py [--only ab] [--repeats 7] [--out profiles/ring_coverage/ring_coverage.json]

(a) the 600-row 8 192 x 9 000 scene of tools/bench_run_flatten.py after rle.flatten_runs (a random rank);
(b) its eight 1 024 x 1 024 noise masks after rle.flatten_runs with the area order.
Per load and tolerance (0.5, 1, 2): the trace (rle.runs_to_polygons), the whole shared call (rle.simplify_coverage, which holds
a trace), the independent route (trace + rle.simplify_polygons), and inside the shared call the node pass
(rsp_ring_coverage_nodes_count + _write) and the mark (rsp_ring_coverage_mark), each between two device synchronises of their
own in a separate set of runs; vertices traced, noded and kept, rings dropped, the deepest ring.  Clock: host perf_counter
around a device synchronise; one warm-up of each side, then the sides alternate; medians of --repeats with the range."""
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
STAGES = {'rsp_ring_coverage_nodes_count': 'node_pass', 'rsp_ring_coverage_nodes_write': 'node_pass',
          'rsp_ring_coverage_mark': 'mark', 'rsp_ring_coverage_check': 'check'}


def _clock_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


class StageClock:
    """inside, the entry points of STAGES run between two device synchronises and their time is added up per stage"""

    def __init__(self):
        self.ms = {}

    def __enter__(self):
        from rsprompter_amd import _lib
        self.lib = _lib.load()
        clock = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(clock.lib, name)
                if name not in STAGES:
                    return fn

                def timed(*a):
                    t, r = _clock_ms(lambda: fn(*a))
                    clock.ms[STAGES[name]] = clock.ms.get(STAGES[name], 0.0) + t
                    return r
                return timed
        _lib._lib = Proxy()
        return self

    def __exit__(self, *a):
        from rsprompter_amd import _lib
        _lib._lib = self.lib


def measure(a, counts, n, size):
    from rsprompter_amd import ops, rle
    polys = rle.runs_to_polygons(counts, n, size)
    out = dict(instances=int(n.shape[0]), canvas=list(size), rings=int(polys[2].shape[0]), vertices_traced=int(polys[0].shape[0]),
               vertices_noded=int(ops.ring_coverage(counts, n, size[0], size[1], 0)[0].shape[0]), tolerances={})
    for tol in TOLERANCES:
        q8 = rle.polygon_tolerance_q8(tol)
        sides = dict(trace=lambda: rle.runs_to_polygons(counts, n, size),
                     shared_total=lambda: rle.simplify_coverage(counts, n, size, tol),
                     independent_total=lambda: rle.simplify_polygons(rle.runs_to_polygons(counts, n, size), size, tol))
        for f in sides.values():
            f()
        ms = {key: [] for key in sides}
        stages = {}
        for _ in range(a.repeats):
            for key, f in sides.items():
                ms[key].append(_clock_ms(f)[0])
            with StageClock() as sc:
                sides['shared_total']()
            for key, v in sc.ms.items():
                stages.setdefault(key, []).append(v)
        got = ops.ring_coverage(counts, n, size[0], size[1], q8, with_rounds=True)
        alone = ops.ring_simplify(*polys, q8, 0, size[0], size[1], with_rounds=True)
        t = dict(tol2_q8=q8, ms={key: _stats(v) for key, v in ms.items()}, stage_ms={key: _stats(v) for key, v in stages.items()},
                 vertices_kept=int(got[0].shape[0]), rings_dropped=out['rings'] - int(got[2].shape[0]),
                 deepest_ring_rounds=int(got[8].max()) if got[8].numel() else 0,
                 independent=dict(vertices_kept=int(alone[0].shape[0]), rings_dropped=out['rings'] - int(alone[2].shape[0]),
                                  deepest_ring_rounds=int(alone[7].max()) if alone[7].numel() else 0))
        t['shared_over_independent_time'] = t['ms']['shared_total']['median'] / t['ms']['independent_total']['median']
        t['node_pass_over_trace_time'] = t['stage_ms']['node_pass']['median'] / t['ms']['trace']['median']
        out['tolerances'][str(tol)] = t
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ring_coverage', 'ring_coverage.json'))
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--only', default='ab', help='which of the two loads to run')
    a = ap.parse_args(argv)
    from rsprompter_amd import rle
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats,
               clock='host perf_counter around a device synchronise; one warm-up, alternating sides, medians with the range')
    if 'a' in a.only:
        import bench_coco_iou_runs as base
        gt, dts, _ = base.scene_load(a, dev)
        strings = [g['segmentation']['counts'] for g in gt['annotations']] + [d['segmentation']['counts'] for d in dts]
        counts, n = rle.strings_to_runs(strings, dev)
        rank = np.random.default_rng(1).permutation(int(n.shape[0])).astype(np.int32)
        fc, fn = rle.flatten_runs(counts, n, (8192, 9000), rank)[:2]
        doc['a_scene_8192x9000_flattened'] = measure(a, fc, fn, (8192, 9000))
        del gt, dts, counts, n, fc, fn
    if 'b' in a.only:
        g = torch.Generator().manual_seed(8)
        masks = (torch.rand((8, 1024, 1024), generator=g) < 0.5).to(dev)
        counts, n, _, _ = rle.encode_runs(masks, 1 << 20)
        areas = masks.view(8, -1).sum(1)
        rank = rle.flatten_rank(8, 'area', None, areas)
        fc, fn = rle.flatten_runs(counts, n, (1024, 1024), rank)[:2]
        doc['b_noise_8x1024x1024_flattened'] = measure(a, fc, fn, (1024, 1024))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return doc


if __name__ == '__main__':
    main(sys.argv[1:])
