"""Panoptic quality per image (csrc/panoptic_quality.hip) against the reference's routes, in one process on one GPU.

    python tools/bench_pq.py [--only big,small,noise] [--iters 50] [--out FILE] [--kernels-only]

Loads (tests/_pq_cases.generate: nearest-seed cells, void and unlisted cells, crowds):
  big    1024 x 1024, 100 segments a side;
  small  256 x 256, 30 segments a side;
  noise  1024 x 1024 where every pixel starts a run (100 ids a side): the worst case of the run compression.
Timed, each from the predicted map as a device tensor and the ground truth already where the route wants it:
  pq_image_ids / pq_image_rgb   ops.pq_image with the gt as an int32 map / as RGB bytes (five launches, nothing read back);
  host_numpy                    the map copied to the host, then the reference's procedure (tests/_pq_ref.image_loop: np.unique
                                over the map and over H * W 64-bit keys, dict loops);
  host_numpy_png                the same behind the reference's PNG round trip of the prediction (PIL encode + decode in memory);
  torch_unique                  void mapping and torch.unique(return_counts) of the 64-bit keys on the device, the pairs copied to
                                the host, the reference's dict loops there.
Every route's statistics are compared with the reference's before anything is timed.  Clock: device events around `--iters` calls
after three warm-up calls, five such windows, the median per call with the range (host routes: fewer calls); peak memory is
torch.cuda.max_memory_allocated over one call above what the inputs hold.  --kernels-only runs 20 calls of pq_image_rgb on
`big` and `noise` and nothing else: the run to put under a kernel trace."""
import argparse
import io
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

LOADS = dict(big=(1024, 1024, 100, False), small=(256, 256, 30, False), noise=(1024, 1024, 100, True))


def timed(fn, iters, windows=5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / iters)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return dict(ms=dict(median=statistics.median(per_call), min=min(per_call), max=max(per_call)), iters=iters, windows=windows,
                peak_bytes_above_inputs=torch.cuda.max_memory_allocated() - base)


def dict_loops(conf, pred, gts, cats):
    """the reference's matching on a confusion dict {(gt id, pred id): count}, pred = {id: [category, area]}"""
    stat = {c: [0, 0, 0, 0.0] for c in cats}
    gm, pm = set(), set()
    for (g, p), inter in conf.items():
        if g not in gts or p not in pred or gts[g]['iscrowd'] == 1 or gts[g]['category_id'] != pred[p][0]:
            continue
        iou = inter / (pred[p][1] + gts[g]['area'] - inter - conf.get((0, p), 0))
        if iou > 0.5:
            stat[pred[p][0]][0] += 1
            stat[pred[p][0]][3] += iou
            gm.add(g)
            pm.add(p)
    crowd = {}
    for g, s in gts.items():
        if g in gm:
            continue
        if s['iscrowd'] == 1:
            crowd[s['category_id']] = g
            continue
        stat[s['category_id']][2] += 1
    for p, (c, area) in pred.items():
        if p in pm:
            continue
        inter = conf.get((0, p), 0) + (conf.get((crowd[c], p), 0) if c in crowd else 0)
        if not inter / area > 0.5:
            stat[c][1] += 1
    return stat


def torch_unique_route(pan, gt, segments, cats, nc):
    pan = pan.to(torch.int64)
    pan0 = torch.where(pan % 1000 == nc, torch.zeros_like(pan), pan)
    keys, counts = torch.unique(gt * (1 << 32) + pan0, return_counts=True)
    keys, counts = keys.cpu().tolist(), counts.cpu().tolist()
    conf = {(k >> 32, k & 0xffffffff): n for k, n in zip(keys, counts)}
    pred = {}
    for (g, p), n in conf.items():
        if p:
            pred.setdefault(p, [p % 1000, 0])[1] += n
    return dict_loops(conf, pred, {s['id']: s for s in segments}, cats)


def png_round_trip(pan_host, nc):
    from PIL import Image
    import _pq_ref as pr
    buf = io.BytesIO()
    Image.fromarray(pr.id2rgb(pr.void_mapped(pan_host, nc)), 'RGB').save(buf, format='PNG')
    buf.seek(0)
    return pr.rgb2id(np.array(Image.open(buf).convert('RGB')))


def measure(a, name, dev):
    import _pq_cases as qc
    import _pq_ref as pr
    from rsprompter_amd import ops
    H, W, n, noise = LOADS[name]
    pan_h, gt_h, segments = qc.generate(H, W, n, 11, noise=noise)
    for s in segments:
        s['area'] = int((gt_h == s['id']).sum())
    cats = list(qc.CATS)
    want = pr.image_loop(pan_h, gt_h, segments, cats, qc.NC)
    pan = torch.from_numpy(pan_h).to(dev)
    gt_ids = torch.from_numpy(gt_h).to(torch.int32).to(dev)
    gt64 = torch.from_numpy(gt_h).to(dev)
    gt_rgb = torch.from_numpy(pr.id2rgb(gt_h)).to(dev)
    routes = dict(
        pq_image_ids=lambda: ops.pq_image(pan, gt_ids, segments, qc.CATS, qc.NC),
        pq_image_rgb=lambda: ops.pq_image(pan, gt_rgb, segments, qc.CATS, qc.NC),
        host_numpy=lambda: pr.image_loop(pan.cpu().numpy(), gt_h, segments, cats, qc.NC),
        host_numpy_png=lambda: pr.image_loop(png_round_trip(pan.cpu().numpy(), qc.NC), gt_h, segments, cats, 1 << 30),
        torch_unique=lambda: torch_unique_route(pan, gt64, segments, cats, qc.NC))
    for k in ('pq_image_ids', 'pq_image_rgb'):
        assert qc.to_host(routes[k]())['stat'] == want['stat'], k
    assert routes['host_numpy_png']()['stat'] == want['stat'] and routes['torch_unique']() == want['stat']
    res = dict(shape=[H, W], gt_segments=len(segments), predicted_segments=len(want['segments']),
               runs_per_row=float((np.diff(pan_h, axis=1) != 0).sum(1).mean() + 1))
    if a.kernels_only:
        for _ in range(20):
            routes['pq_image_rgb']()
        torch.cuda.synchronize()
        return res
    for k, fn in routes.items():
        res[k] = timed(fn, a.iters if k.startswith('pq_image') else max(a.iters // 10, 3))
    for k in ('host_numpy', 'host_numpy_png', 'torch_unique'):
        res[k + '_over_pq_image_rgb'] = res[k]['ms']['median'] / res['pq_image_rgb']['ms']['median']
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'panoptic_quality', 'panoptic_quality.json'))
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--only', default='big,small,noise')
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_pq.py measures on the GPU; there is none here')
    dev = torch.device('cuda:0')
    doc = dict(device=torch.cuda.get_device_name(0), clock='device events around `iters` calls, 3 warm-up calls, median of 5 windows per call')
    for name in a.only.split(','):
        if a.kernels_only and name == 'small':
            continue
        doc[name] = measure(a, name, dev)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out and not a.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return doc


if __name__ == '__main__':
    main(sys.argv[1:])
