"""Measurements of polygon rasterisation on one GPU, each beside the host path it can replace:

  (a) the 26 committed NWPU annotations tiled to --instances (10 000): datasets.anns_to_rle on the device against the
      datasets.ann_to_rle loop on the host, both from the JSON's lists to finished RLE strings; the strings are compared.
  (b) the rings of the 300-instance 8 192 x 9 000 scene of tools/bench_mask_polygons.py back to a run table
      (rle.polygons_to_runs, fill='evenodd') beside the forward rle.runs_to_polygons of the same run; the table is compared
      with the one the rings came from.  The inverse is also split into its parts: everything up to the sorted keys (with and
      without the compaction in front of the sort), a torch.sort of as many int64 keys as there are walk points alone, and
      the last stage.
  (c) CocoMetric.compute_metrics on a synthetic load shaped like DESIGN §13's (--images of 512 x 512, 50 ground-truth
      ellipses given as 32-vertex polygons and 100 detections each, one category), gt_raster='host' against 'device'; the
      stats are compared.

  python tools/bench_poly_raster.py [--out profiles/poly_raster/poly_raster.json] [--repeats 5] [--instances 10000] [--images 1000]

Every side ends on the host or in a device synchronise, so the clock is the host's around it; device sides run --repeats
times after a warm-up and alternate with the forward direction in (b); the host loops of (a) and (c) run --host-repeats
times.  Prints and writes one JSON document; nothing is asserted but the equalities are recorded."""
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
NWPU_JSON = os.path.join(ROOT, 'tests', 'golden', 'coco_nwpu', 'NWPU_instances_val_subset.json')


def _clock_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))


def _timed(f, repeats):
    f()
    ms, r = [], None
    for _ in range(repeats):
        t, r = _clock_ms(f)
        ms.append(t)
    return _stats(ms), r


def annotations(a, dev):
    from rsprompter_amd import datasets
    with open(NWPU_JSON) as f:
        d = json.load(f)
    hw = {im['id']: (im['height'], im['width']) for im in d['images']}
    base = [(x['segmentation'], hw[x['image_id']]) for x in d['annotations']]
    items = [base[i % len(base)] for i in range(a.instances)]
    segms, sizes = [s for s, _ in items], [z for _, z in items]
    dev_ms, got = _timed(lambda: datasets.anns_to_rle(segms, sizes, dev), a.repeats)
    host = []
    for _ in range(a.host_repeats):
        t, want = _clock_ms(lambda: [datasets.ann_to_rle(s, h, w) for s, (h, w) in zip(segms, sizes)])
        host.append(t)
    out = dict(instances=a.instances, vertices=sum(len(p) // 2 for s in segms for p in s), device_ms=dev_ms,
               host_ms=_stats(host), equal=got == want)
    out['host_over_device'] = out['host_ms']['median'] / dev_ms['median']
    return out


def scene(a, dev):
    from bench_mask_polygons import _tables
    from rsprompter_amd import ops, rle
    name, counts, n, size = next(iter(_tables(dev)))
    k = int(n.shape[0])
    polys = rle.runs_to_polygons(counts, n, size)
    verts, ring_offs, ring_inst = polys[0].to(torch.float64), polys[1], polys[2]
    ghw = torch.tensor([list(size)] * k, dtype=torch.int32, device=dev)

    def forward():
        return rle.runs_to_polygons(counts, n, size)

    def inverse():
        return rle.polygons_to_runs(verts, ring_offs, ring_inst, ghw, fill='evenodd', cap=int(counts.shape[1]))

    def keys():
        return ops.poly_raster_launcher(verts, ring_offs, ring_inst, ghw)

    def keys_uncompacted():
        return ops.poly_raster_launcher(verts, ring_offs, ring_inst, ghw, compact=False)
    forward(), inverse(), keys_uncompacted()
    ms = dict(forward=[], inverse=[], inverse_up_to_sorted_keys=[],
              inverse_up_to_sorted_keys_without_compaction=[], inverse_runs_stage=[], sort_alone=[])
    launch = keys()
    T = int(launch.walk_points)
    rnd = torch.randint(0, 2 ** 40, (max(T, 1),), dtype=torch.int64, device=dev)
    for _ in range(a.repeats):
        ms['forward'].append(_clock_ms(forward)[0])
        t, (c, m) = _clock_ms(inverse)
        ms['inverse'].append(t)
        ms['inverse_up_to_sorted_keys'].append(_clock_ms(keys)[0])
        ms['inverse_up_to_sorted_keys_without_compaction'].append(_clock_ms(keys_uncompacted)[0])
        ms['inverse_runs_stage'].append(_clock_ms(lambda: launch(int(counts.shape[1])))[0])
        ms['sort_alone'].append(_clock_ms(lambda: torch.sort(rnd))[0])
    w = min(int(c.shape[1]), int(counts.shape[1]))
    live = torch.arange(w, device=dev)[None] < n[:, None]
    equal = bool(torch.equal(m, n)) and bool(torch.equal(torch.where(live, c[:, :w], 0), torch.where(live, counts[:, :w], 0)))
    out = dict(table=name, instances=k, canvas=list(size), runs=int(n.clamp(min=0).sum()), rings=int(ring_inst.shape[0]),
               vertices=int(verts.shape[0]), walk_points=T, crossings=int(launch.crossings),
               ms={key: _stats(v) for key, v in ms.items()}, equal=equal)
    out['inverse_over_forward'] = out['ms']['inverse']['median'] / out['ms']['forward']['median']
    return out


def _ellipse(rng, S, nv=32):
    cx, cy = rng.uniform(40, S - 40, 2)
    rx, ry = rng.uniform(6, 36, 2)
    th = rng.uniform(0, np.pi)
    t = np.arange(nv) * (2 * np.pi / nv)
    x, y = rx * np.cos(t), ry * np.sin(t)
    return np.stack([cx + x * np.cos(th) - y * np.sin(th), cy + x * np.sin(th) + y * np.cos(th)], 1)


def metric(a, dev, tmp):
    from rsprompter_amd import datasets
    from rsprompter_amd.evaluation import CocoMetric
    rng = np.random.default_rng(13)
    S, NG, ND = 512, 50, 100
    images, anns, dts = [], [], {}
    for i in range(a.images):
        images.append(dict(id=i + 1, height=S, width=S, file_name=f'{i}.png'))
        polys = []
        for g in range(NG):
            e = _ellipse(rng, S)
            x0, y0, x1, y1 = e[:, 0].min(), e[:, 1].min(), e[:, 0].max(), e[:, 1].max()
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=1, iscrowd=0, bbox=[x0, y0, x1 - x0, y1 - y0],
                             area=float((x1 - x0) * (y1 - y0) * np.pi / 4), segmentation=[np.round(e, 2).reshape(-1).tolist()]))
            polys.append(e)
        dts[i + 1] = [polys[j % NG] + rng.normal(0, 1.5, 2) for j in range(ND)]
    gt_file = os.path.join(tmp, 'gt.json')
    with open(gt_file, 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=1, name='building')]), f)
    flat = [p for i in sorted(dts) for p in dts[i]]
    rles = datasets.anns_to_rle([[p.reshape(-1).tolist()] for p in flat], (S, S), dev)          # set-up: the detections' masks
    samples = []
    for j, i in enumerate(sorted(dts)):
        ps = dts[i]
        boxes = np.array([[p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()] for p in ps], np.float32)
        pi = dict(bboxes=torch.from_numpy(boxes), scores=torch.from_numpy(rng.uniform(0.05, 1, ND).astype(np.float32)),
                  labels=torch.zeros((ND,), dtype=torch.int64), masks=rles[j * ND:(j + 1) * ND])
        samples.append(dict(pred_instances=pi, img_id=i, ori_shape=(S, S)))
    out = dict(images=a.images, gts=len(anns), dts=len(flat), vertices_per_polygon=32)
    stats = {}
    for how, reps in (('device', a.repeats), ('host', a.host_repeats)):
        ms, gt_ms = [], []
        for _ in range(reps + (1 if how == 'device' else 0)):
            m = CocoMetric(ann_file=gt_file, metric=['bbox', 'segm'], device=str(dev), gt_raster=how)
            m.dataset_meta = dict(classes=['building'])
            m.process(None, samples)
            t, _ = _clock_ms(lambda: m.compute_metrics(m.results))
            ms.append(t)
            gt_ms.append(_clock_ms(lambda: m._gt_with_rles(m.coco_gt, dev))[0])
            stats[how] = {k: v.stats.tolist() for k, v in m.eval_results.items()}
        skip = 1 if how == 'device' else 0                          # the device side's first pass is its warm-up
        out[how] = dict(compute_metrics_ms=_stats(ms[skip:]), ground_truth_to_rle_ms=_stats(gt_ms[skip:]))
    out['equal_stats'] = stats['host'] == stats['device']
    out['segm_mAP'] = stats['device']['segm'][0]
    out['host_over_device'] = dict(
        compute_metrics=out['host']['compute_metrics_ms']['median'] / out['device']['compute_metrics_ms']['median'],
        ground_truth_to_rle=out['host']['ground_truth_to_rle_ms']['median'] / out['device']['ground_truth_to_rle_ms']['median'])
    return out


def main(argv=None):
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'poly_raster', 'poly_raster.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-repeats', type=int, default=1)
    ap.add_argument('--instances', type=int, default=10000)
    ap.add_argument('--images', type=int, default=1000)
    ap.add_argument('--only', default='abc', help='which of the three measurements to run')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_poly_raster measures on a GPU; none is visible')
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, host_repeats=a.host_repeats,
               clock='host perf_counter around a device synchronise')
    if 'a' in a.only:
        doc['a_nwpu_annotations'] = annotations(a, dev)
    if 'b' in a.only:
        doc['b_scene_rings'] = scene(a, dev)
    if 'c' in a.only:
        with tempfile.TemporaryDirectory() as tmp:
            doc['c_coco_metric'] = metric(a, dev, tmp)
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
