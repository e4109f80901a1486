#!/usr/bin/env python
"""Measurements behind DESIGN §15 (promptable SAM), one GPU, one process:

  python tools/bench_sam_prompts.py [--arch huge] [--reps 20] [--out profiles/sam_prompts/bench.json]

ViT-`arch` with the seeded synthetic weights on one synthetic 1024 x 1024 tile; every figure is the median of `reps` timed
repetitions after 3 warm-up ones, timed with device events around the whole phase (host launch time included, as a caller sees it).
  (a) SamSession set-up (resize + encoder) and .predict for 1 / 64 / 1024 single-point prompt sets (three masks each);
  (b) generate_masks at points_per_side=32 (3072 candidates), whole and split into decode, rsp_mask_score_box, filter +
      NMS, and full-resolution masks + run lengths of the kept ones.  The thresholds sit at the medians of this image's own
      scores (the synthetic weights give no mask a stability score near SAM's default 0.95), offset 0.25;
  (c) alternating with (b)'s scoring leg, the same scores the obvious way: ops.mask_post_logits(want_val=True) in batches
      of 64 and three reductions over the fp32 field.
The scoring kernel's achieved input bytes/s and pixel evaluations/s are derived from the shapes."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='huge')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from rsprompter_amd import ops
    from rsprompter_amd.samdet import SamModelHIP
    from rsprompter_amd.sam_prompts import SamSession, filter_candidates, generate_masks, point_grid, _rle_dicts
    from rsprompter_amd.synth import synth_images, synth_state_dict
    dev = torch.device('cuda:0')
    model = SamModelHIP(a.arch)
    sd = synth_state_dict(model, seed=0)
    sd['shared_image_embedding.positional_embedding'] = sd['prompt_encoder.shared_embedding.positional_embedding']   # HF ties them
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    img = synth_images(1)[0].permute(1, 2, 0).contiguous().to(dev)                 # [1024, 1024, 3] uint8
    out = dict(arch=a.arch, device=torch.cuda.get_device_name(0), image=[1024, 1024])
    out['session_setup'] = timed(lambda: SamSession(model, img), max(5, a.reps // 4))
    s = SamSession(model, img)
    g = np.random.RandomState(0)
    out['predict'] = {}
    for n in (1, 64, 1024):
        pts = g.rand(n, 1, 2) * 1024
        out['predict'][str(n)] = timed(lambda: s.predict(points=pts), a.reps if n < 1024 else max(5, a.reps // 2))
    # ---- (b) generation, split
    n, off, S = 32, 0.25, (1024, 1024)
    pts = (point_grid(n) * 1024.0)[:, None, :]
    decode = lambda: s._low_res(pts, None, None, None, True)                       # noqa: E731
    out['generate'] = dict(points_per_side=n, candidates=3 * n * n, stability_score_offset=off)
    out['generate']['decode'] = timed(decode, max(5, a.reps // 2))
    low, iou = decode()
    K = low.shape[0] * 3
    low, iou = low.reshape(K, 256, 256).contiguous(), iou.reshape(K)
    score = ops.mask_score_box(low, S, S, S, 0.0, off)
    stab = score[:, 0] / score[:, 1]
    t_iou, t_stab = float(iou.median()), float(stab[~stab.isnan()].median())
    out['generate'].update(pred_iou_thresh=t_iou, stability_score_thresh=t_stab)

    def fused():
        return ops.mask_score_box(low, S, S, S, 0.0, off)

    def obvious():
        cnt = torch.empty((K, 3), dtype=torch.int64, device=dev)
        for i in range(0, K, 64):
            val = ops.mask_post_logits(low[i:i + 64], S, S, S, 0.0, want_val=True)[1]
            for j, t in enumerate((off, -off, 0.0)):
                cnt[i:i + 64, j] = (val > t).flatten(1).sum(1)
        return cnt
    assert torch.equal(fused()[:, :3].long(), obvious())
    fu, ob = [], []
    for _ in range(2):                                                             # alternating
        fu.append(timed(fused, a.reps))
        ob.append(timed(obvious, max(5, a.reps // 4)))
    out['generate']['score_fused'], out['generate']['score_obvious'] = fu, ob
    ms = min(f['median_ms'] for f in fu)
    out['generate']['score_kernel_rates'] = dict(
        input_bytes=K * 256 * 256 * 4, input_TB_per_s=round(K * 256 * 256 * 4 / (ms * 1e-3) / 1e12, 3),
        pixel_evaluations=K * 1024 * 1024, Gpixel_per_s=round(K * 1024 * 1024 / (ms * 1e-3) / 1e9, 1),
        field_bytes_not_written=K * 1024 * 1024 * 4)
    keep = filter_candidates(iou, score, t_iou, t_stab)
    idx = keep.nonzero()[:, 0]
    boxes, scores = score[idx, 3:7].float(), iou[idx]

    def filt_nms():
        k = filter_candidates(iou, score, t_iou, t_stab).nonzero()[:, 0]
        return ops.nms_flat(score[k, 3:7].float(), iou[k], torch.zeros_like(k, dtype=torch.int32), 0.7)
    out['generate']['filter_nms'] = timed(filt_nms, a.reps)
    order = ops.nms_flat(boxes, scores, torch.zeros_like(idx, dtype=torch.int32), 0.7)
    sel = idx[order]
    out['generate'].update(kept_by_filter=int(idx.shape[0]), kept_by_nms=int(sel.shape[0]))

    def masks_rle():
        for i in range(0, int(sel.shape[0]), 64):
            _rle_dicts(s.full_res(low[sel[i:i + 64]], 0.0))
    out['generate']['masks_and_rle_of_kept'] = timed(masks_rle, max(3, a.reps // 4))
    out['generate']['whole_call'] = timed(lambda: generate_masks(model, None, points_per_side=n, pred_iou_thresh=t_iou,
                                                                 stability_score_thresh=t_stab, stability_score_offset=off,
                                                                 session=s), max(3, a.reps // 4))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
