"""Panoptic fusion (csrc/panoptic_fuse.hip) against the reference's dense route, in one process on one GPU.

    python tools/bench_panoptic.py [--only ab] [--iters 50] [--out FILE]

(a) Nq = 100 queries, 256 x 256 logits -> 1024 x 1024 (the shape of BASELINE.json configs[2] / [4]; crop == output: the
    strip form);
(b) the WHU shape: the same logits, crop 1024 x 1024 -> 512 x 512 (the generic form).
Inputs: tests/_mask_field_props.py's logit recipe (avg_pool2d(randn, 9, 1, 4) * 20) with offsets in [-4, 4], class rows with
scores in [0.5, 1] and a background query in ten, nc = 10 things + 5 stuff, object_mask_thr 0.8 (the default), iou_thr 0.3.
Timed: ops.panoptic_fuse (four launches, nothing read back) and the reference's route in torch on the same device
(interpolate -> crop -> interpolate -> sigmoid -> scores * sigmoid -> argmax -> the Python loop over the kept queries with its
.item() reads, maskformer_fusion_head.py:62-106).  The two maps are compared before anything is timed and the number of differing pixels is
recorded: they may differ where the two largest products tie within fp32.  Clock: device events around `--iters` calls after
three warm-up calls, five such windows, the median per call with the range; peak memory is torch.cuda.max_memory_allocated
over one call above what the inputs hold."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

NC, NTHINGS, NQ = 15, 10, 100
IOU_THR = 0.3                      # with 90 kept queries in competition the default 0.8 paints nothing; both routes use this


def inputs(dev, seed=0):
    import _mask_field_props as mf
    g = torch.Generator().manual_seed(seed)
    low = mf.recipe_logits(NQ, (256, 256), seed) + (torch.rand(NQ, generator=g) * 8 - 4)[:, None, None]
    cls = (torch.rand(NQ, NC + 1, generator=g) - 0.5) * 0.4
    label = torch.randint(0, NC, (NQ,), generator=g)
    label[::10] = NC
    cls[torch.arange(NQ), label] += torch.rand(NQ, generator=g) * 4.5 + 2.5
    return cls.contiguous().to(dev), low.contiguous().to(dev)


def dense_route(cls, low, img, crop, out, thr=0.8, iou_thr=IOU_THR):
    """the reference's route on the device it would run on: three [Nq, H, W] fp32 tensors and one host read per kept query"""
    v = F.interpolate(low[:, None], size=img, mode='bilinear', align_corners=False)[:, 0, :crop[0], :crop[1]]
    if tuple(out) != tuple(crop):
        v = F.interpolate(v[:, None], size=out, mode='bilinear', align_corners=False)[:, 0]
    scores, labels = F.softmax(cls, dim=-1).max(-1)
    prob = v.sigmoid()
    keep = labels.ne(NC) & (scores > thr)
    ks, kl, kp = scores[keep], labels[keep], prob[keep]
    sem = torch.full(tuple(out), NC, dtype=torch.int32, device=low.device)
    if kp.shape[0] == 0:
        return sem
    ids = (ks.view(-1, 1, 1) * kp).argmax(0)
    inst = 1
    for k in range(kl.shape[0]):
        c = int(kl[k].item())
        m = ids == k
        ma, oa = m.sum().item(), (kp[k] >= 0.5).sum().item()
        if ma > 0 and oa > 0 and not ma / oa < iou_thr:
            if c < NTHINGS:
                sem[m] = c + inst * 1000
                inst += 1
            else:
                sem[m] = c
    return sem


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


def measure(a, cls, low, img, crop, out):
    from rsprompter_amd import ops
    fused = lambda: ops.panoptic_fuse(cls, low, img, crop, out, NTHINGS, NC, iou_thr=IOU_THR)         # noqa: E731
    dense = lambda: dense_route(cls, low, img, crop, out)                              # noqa: E731
    sem, info = fused()
    want = dense()
    diff = int((sem != want).sum())
    res = dict(queries=NQ, kept_with_an_area=int(((info['mask_area'] > 0) | (info['original_area'] > 0)).sum()),
               painted=int((info['segment'] >= 0).sum()), logits=[256, 256], img=list(img), crop=list(crop), out=list(out),
               pixels_differing_from_the_dense_route=diff)
    res['panoptic_fuse'] = timed(fused, a.iters)
    res['dense_route_torch'] = timed(dense, max(a.iters // 10, 3))
    res['dense_over_fused_time'] = res['dense_route_torch']['ms']['median'] / res['panoptic_fuse']['ms']['median']
    res['dense_over_fused_peak'] = res['dense_route_torch']['peak_bytes_above_inputs'] / max(res['panoptic_fuse']['peak_bytes_above_inputs'], 1)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'panoptic_fuse', 'panoptic_fuse.json'))
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--only', default='ab')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_panoptic.py measures on the GPU; there is none here')
    dev = torch.device('cuda:0')
    cls, low = inputs(dev)
    doc = dict(device=torch.cuda.get_device_name(0), clock='device events around `iters` calls, 3 warm-up calls, median of 5 windows per call')
    if 'a' in a.only:
        doc['a_identity_256_to_1024'] = measure(a, cls, low, (1024, 1024), (1024, 1024), (1024, 1024))
    if 'b' in a.only:
        doc['b_whu_1024_to_512'] = measure(a, cls, low, (1024, 1024), (1024, 1024), (512, 512))
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return doc


if __name__ == '__main__':
    main(sys.argv[1:])
