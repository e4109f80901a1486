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
The scoring kernel's achieved input bytes/s and pixel evaluations/s are derived from the shapes.

  python tools/bench_sam_prompts.py --multicrop [--arch huge] [--reps 5] [--crop-batches 1,2,4,8] [--out .../multicrop.json]

  (d) the crop layers (`SamMaskGenerator`): crop_n_layers 1 and 2 (downscale factor 2 at two layers), points_per_side=32, by
      phase (crop front end, encoder, decoder, scoring, filter + NMS, masks + run lengths; device events around every phase,
      summed per name), against -- alternating, same process -- the same work with what existed before the batched path: a
      host slice per crop, one SamSession per crop, rsp_mask_score_box per crop, a kept-count read per crop, the near-edge rule
      and the shift as torch expressions; then the sweep of crop_batch.  --multicrop-once runs one generate() per
      configuration and nothing else (the process to put under rocprofv3 --kernel-trace --stats).

  python tools/bench_sam_prompts.py --persam [--arch huge] [--reps 5] [--out profiles/sam_prompts/persam.json]

  (e) PerSAM (`PerSam.segment`): synthetic 1 024^2 tiles, B = 1 and B = 8, by phase (front end, encoder, similarity, locate,
      the three decoder passes, masks + run lengths, transfer), against -- alternating, same process -- the same work with what
      existed before the similarity / locate kernels and the batched flow: per image a SamSession, the similarity as torch
      expressions, mask_post_logits(want_val=True) for the field, torch argmax / argmin / mean / std / F.interpolate, and the
      three decoder passes with host-side point, best-of-three and box extraction in between; then rsp_persam_locate and
      rsp_mask_score_box alone on the same fields (pixel rates).  --persam-once: one segment() per batch size (kernel trace).

  python tools/bench_sam_prompts.py --regions [--arch huge] [--reps 20] [--out profiles/mask_regions/regions.json]

  (f) `min_mask_region_area`: ops.remove_small_regions on 64 masks of 1024 x 1024 (thresholded smooth noise plus speckle) per
      mode, after the encoder has run (warm clocks); the bytes the design moves per pixel against norm.hip's streaming rate;
      the same cleaning the host way (device -> host, scipy.ndimage.label per mask, host -> device); SamMaskGenerator.generate
      (one crop layer) with min_mask_region_area 0 and 100, alternating.  --regions-once: one call per mode (kernel trace).

  python tools/bench_sam_prompts.py --persam-f [--arch base] [--reps 5] [--out profiles/persam_f/persam_f.json]

  (g) PerSAM-F's fit (`ops.persam_f_fit`, 1000 epochs) at 1024 x 1024 (identity crop: the strip form) and at 600 x 900 (the
      generic form) on smooth logits of amplitude ~10, against -- alternating, same process -- the same fit as torch autograd
      + AdamW + CosineAnnealingLR in fp32 over the materialised fields on the same device (what the paper's code does); the
      distance of the two results; the fit's pixel evaluations/s; one encoder pass of ViT-`arch`, for scale.
      --persam-f-once: one fit per geometry (kernel trace)."""
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


def _spread(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), reps=len(ms))


class _Phases:
    """SamMaskGenerator._phase: device events around every phase, summed per name after one synchronisation"""

    def __init__(self):
        self.ev = []

    def __call__(self, name):
        import contextlib

        @contextlib.contextmanager
        def cm():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            yield
            b.record()
            self.ev.append((name, a, b))
        return cm()

    def take(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.ev:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        self.ev = []
        return out


def multicrop(model, img, a):
    from rsprompter_amd import ops
    from rsprompter_amd.sam_prompts import SamMaskGenerator, SamSession, filter_candidates, point_grid
    dev = img.device
    H, W = int(img.shape[0]), int(img.shape[1])
    S, off, n = model.image_size, 0.25, 32
    s0 = SamSession(model, img)
    low, iou = s0._low_res((point_grid(n) * np.array([[W, H]]))[:, None, :], None, None, None, True)
    K = low.shape[0] * 3
    sc = ops.mask_score_box(low.reshape(K, 256, 256), (S, S), s0.input_size, (H, W), 0.0, off)
    stab = sc[:, 0] / sc[:, 1]
    t_iou, t_stab = float(iou.median()), float(stab[~stab.isnan()].median())
    del s0, low, iou, sc
    out = dict(points_per_side=n, stability_score_offset=off, pred_iou_thresh=t_iou, stability_score_thresh=t_stab, configs={})
    kw = dict(points_per_side=n, pred_iou_thresh=t_iou, stability_score_thresh=t_stab, stability_score_offset=off)

    def loop_of(gen):
        """the same work per crop with what existed before rsp_crops_resize_pad / rsp_mask_score_box_crops"""
        boxes_c, layers, _, geo, _ = gen._plan((H, W))

        def run():
            host = img.cpu()                                                       # the decoded image is a host array
            kl, ki, kb, kc = [], [], [], []
            for ci, ((x0, y0, x1, y1), l) in enumerate(zip(boxes_c, layers)):
                s = SamSession(model, host[y0:y1, x0:x1].contiguous())              # host slice, upload, resize, encoder
                ch, cw = y1 - y0, x1 - x0
                lo, io = s._low_res((gen.grids[l] * np.array([[cw, ch]]))[:, None, :], None, None, None, True)
                k = lo.shape[0] * 3
                lo, io = lo.reshape(k, 256, 256), io.reshape(k)
                score = ops.mask_score_box(lo, (S, S), s.input_size, (ch, cw), 0.0, off)
                box = score[:, 3:7] + torch.tensor([[x0, y0, x0, y0]], dtype=torch.int32, device=dev)
                cb = torch.tensor([[x0, y0, x1, y1]], dtype=torch.int32, device=dev)
                ob = torch.tensor([[0, 0, W, H]], dtype=torch.int32, device=dev)
                near = (((box - cb).abs() <= 20) & ((box - ob).abs() > 20)).any(1)
                idx = (filter_candidates(io, score, t_iou, t_stab) & ~near).nonzero()[:, 0]   # the kept-count read of the crop
                kl.append(lo[idx]); ki.append(io[idx]); kb.append(box[idx].float())
                kc.append(torch.full((int(idx.shape[0]),), ci, dtype=torch.int32, device=dev))
            lo, io, bx, cr = torch.cat(kl), torch.cat(ki), torch.cat(kb), torch.cat(kc)
            order = ops.nms_flat(bx, io, torch.zeros_like(cr), 0.7)
            return gen._masks(lo, order, cr[order].cpu().tolist(), boxes_c, geo, (H, W), dev), bx[order]
        return run

    for layers, down in ((1, 1), (2, 2)):
        gen = SamMaskGenerator(model, crop_n_layers=layers, crop_n_points_downscale_factor=down, crop_batch=a.crop_batch, **kw)
        if a.multicrop_once:
            res = gen.generate(img)
            torch.cuda.synchronize()
            out['configs'][f'layers{layers}_down{down}'] = dict(instances=len(res.masks))
            continue
        loop = loop_of(gen)
        res = gen.generate(img)
        lm, lb = loop()
        same = tuple(res.bboxes.shape) == tuple(lb.shape) and torch.equal(res.bboxes, lb) and res.masks == lm
        ph = _Phases()
        bt, lt, phs = [], [], []
        for r in range(a.reps + 1):                                                  # alternating; the first pair is warm-up
            t = []
            for fn in (lambda: gen.generate(img), loop):
                gen._phase = ph if fn is not loop else (lambda name: __import__('contextlib').nullcontext())
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                t.append(e0.elapsed_time(e1))
                if fn is not loop:
                    p = ph.take()
            if r:
                bt.append(t[0]); lt.append(t[1]); phs.append(p)
        cfg = dict(crops=len(gen.crop_boxes((H, W))), crop_batch=gen.crop_batch, batches=gen._batches(gen._plan((H, W))[1]), instances=len(res.masks),
                   loop_returns_the_same_instances=bool(same),
                   crop_index_histogram=torch.bincount(res.crop_index.cpu(), minlength=1).tolist(),
                   batched=_spread(bt), per_crop_loop=_spread(lt),
                   phases_ms={k: round(statistics.median([p[k] for p in phs]), 3) for k in phs[0]})
        cfg['batched_minus_loop_ms'] = round(cfg['batched']['median_ms'] - cfg['per_crop_loop']['median_ms'], 3)
        cfg['loop_spread_ms'] = round(cfg['per_crop_loop']['max_ms'] - cfg['per_crop_loop']['min_ms'], 3)
        sweep = {}
        for cb in a.crop_batches:
            g2 = SamMaskGenerator(model, crop_n_layers=layers, crop_n_points_downscale_factor=down, crop_batch=cb, **kw)
            sweep[str(cb)] = timed(lambda: g2.generate(img), a.reps, warm=1)
        cfg['crop_batch_sweep'] = sweep
        out['configs'][f'layers{layers}_down{down}'] = cfg
    return out


def persam(model, a):
    import torch.nn.functional as F
    from rsprompter_amd import ops
    from rsprompter_amd.rle import encode_mask_dicts
    from rsprompter_amd.sam_prompts import PerSam, SamSession
    from rsprompter_amd.synth import synth_images
    dev = next(model.parameters()).device
    S, g = model.image_size, model.vision_encoder.grid
    tiles = [t.permute(1, 2, 0).contiguous() for t in synth_images(9)]                # [1024, 1024, 3] uint8, on the host
    H, W = int(tiles[0].shape[0]), int(tiles[0].shape[1])
    ref_mask = torch.zeros(H, W, dtype=torch.bool)
    ref_mask[300:600, 400:700] = True
    ps = PerSam(model, tiles[8], ref_mask)
    tf, te = ps.target_feature, ps.target_embedding
    out = dict(reference_cells=ps.cells, batches={})

    def parent_means(batch):
        res = []
        for img in batch:
            s = SamSession(model, img)
            f = s.image_embeddings[0]
            f = f / f.norm(dim=0, keepdim=True)
            sim = (tf @ f.reshape(256, g * g)).reshape(1, 1, g, g)
            low0 = F.interpolate(sim, scale_factor=4, mode='bilinear')[0]
            val = s.full_res(low0, want_val=True)[1][0]                               # the [H, W] field
            imax, imin = int(val.argmax()), int(val.argmin())                         # host reads
            pts = np.array([[[imax % W, imax // W], [imin % W, imin // W]]], dtype=np.float64)
            lab = np.array([[1, 0]])
            attn = F.interpolate(((val - val.mean()) / val.std())[None, None], size=(g, g), mode='bilinear').sigmoid()
            m, iou, low = s.predict(points=pts, labels=lab, multimask_output=False, attention_similarity=attn.reshape(1, 1, 1, g * g),
                                    target_embedding=te)
            m, iou, low = s.predict(points=pts, labels=lab, mask_input=low[0, 0], multimask_output=True)
            b = int(iou[0].argmax())
            ys, xs = torch.nonzero(m[0, b], as_tuple=True)
            box = [0, 0, 0, 0] if ys.numel() == 0 else [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]
            m, iou, low = s.predict(points=pts, labels=lab, boxes=np.array([box], dtype=np.float64), mask_input=low[0, b],
                                    multimask_output=True)
            b = int(iou[0].argmax())
            res.append(dict(mask=encode_mask_dicts(m[0, b][None])[0], score=float(iou[0, b]), points=pts[0].astype(int).tolist()))
        return res

    for B in (1, 8):
        batch = tiles[:B]
        if a.persam_once:
            ps.segment(batch, batch_size=B)
            torch.cuda.synchronize()
            continue
        new, old = ps.segment(batch, batch_size=B), parent_means(batch)
        same = [n['points'] == o['points'] and n['mask'] == o['mask'] for n, o in zip(new, old)]
        ph = _Phases()
        bt, lt, phs = [], [], []
        for r in range(a.reps + 1):                                                    # alternating; the first pair is warm-up
            t = []
            for which in (0, 1):
                ps._phase = ph if which == 0 else (lambda name: __import__('contextlib').nullcontext())
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ps.segment(batch, batch_size=B) if which == 0 else parent_means(batch)
                e1.record()
                e1.synchronize()
                t.append(e0.elapsed_time(e1))
                if which == 0:
                    p = ph.take()
            if r:
                bt.append(t[0]); lt.append(t[1]); phs.append(p)
        cfg = dict(batched=_spread(bt), parent_means=_spread(lt), same_points_and_masks=same,
                   phases_ms={k: round(statistics.median([p[k] for p in phs]), 3) for k in phs[0]})
        cfg['parent_spread_ms'] = round(cfg['parent_means']['max_ms'] - cfg['parent_means']['min_ms'], 3)
        out['batches'][str(B)] = cfg
    if not a.persam_once:
        low = torch.randn(8, 4 * g, 4 * g, device=dev)
        loc = timed(lambda: ops.persam_locate(low, (S, S), (S, S), (H, W), g), max(a.reps, 10))
        sco = timed(lambda: ops.mask_score_box(low, (S, S), (S, S), (H, W)), max(a.reps, 10))
        out['locate_vs_score_8_fields'] = dict(persam_locate=loc, mask_score_box=sco, pixels=8 * H * W,
                                               locate_Gpixel_per_s=round(8 * H * W / (loc['median_ms'] * 1e-3) / 1e9, 1),
                                               score_Gpixel_per_s=round(8 * H * W / (sco['median_ms'] * 1e-3) / 1e9, 1),
                                               note='whole calls (four and three launches), host launch time included')
    return out


# bytes per pixel and pass of rsp_mask_remove_small_regions as designed (regions.hip): label 1 (mask) + 4 + 4 (parent, cnt written);
# flatten 4 (cnt read); reduce 4 (parent read); write 1 + 4 + 1 (mask, parent, result) -- the reads behind a tile-local root
# (its parent, the root's size) hit a few lines per tile and are not counted, nor is the seam kernel (1 / 32 of the pixels)
REGION_BYTES_PER_PIXEL_PASS = 23
NORM_STREAM_TB_S = 4.8            # what norm.hip's plane-producing LayerNorm reaches here


def persam_f(model, a):
    import torch.nn.functional as F
    from rsprompter_amd import ops
    dev = torch.device('cuda:0')
    epochs, S = 1000, (1024, 1024)
    res = dict(epochs=epochs, cases={})

    def autograd_fit(fields, t):
        w = torch.full((2,), 1 / 3, dtype=torch.float32, device=dev, requires_grad=True)
        opt = torch.optim.AdamW([w], lr=1e-3, betas=(0.9, 0.999), eps=1e-4, weight_decay=0.01)
        sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs)
        for _ in range(epochs):
            opt.zero_grad()
            z = (1 - w[0] - w[1]) * fields[0] + w[0] * fields[1] + w[1] * fields[2]
            p = z.sigmoid()
            dice = 1 - (2 * (p * t).sum() + 1) / (p.sum() + t.sum() + 1)
            ce = F.binary_cross_entropy_with_logits(z, t, reduction='none')
            p_t = p * t + (1 - p) * (1 - t)
            loss = dice + ((0.25 * t + 0.75 * (1 - t)) * ce * (1 - p_t) ** 2).mean()
            loss.backward()
            opt.step()
            sch.step()
        wd = w.detach()
        return torch.stack([1 - wd[0] - wd[1], wd[0], wd[1]])
    for name, crop, out_hw in (('1024x1024 identity (strip form)', (1024, 1024), (1024, 1024)), ('600x900 (generic form)', (683, 1024), (600, 900))):
        g = torch.Generator().manual_seed(11)
        low = (F.avg_pool2d(torch.randn(1, 3, 256, 256, generator=g), 5, 1, 2) * 20).contiguous().to(dev)
        fields = ops.mask_post_logits(low[0], S, crop, out_hw, 0.0, want_val=True)[1]
        gt = (0.05 * fields[0] + 0.8 * fields[1] + 0.15 * fields[2]) > 2.0
        fused = lambda: ops.persam_f_fit(low, gt[None], S, crop, out_hw, epochs=epochs)       # noqa: E731
        if a.persam_f_once:
            fused()
            torch.cuda.synchronize()
            continue
        t = gt.float()
        fused(); autograd_fit(fields, t)                                                       # noqa: E702  (warm-up of both)
        ms = dict(fused=[], autograd=[])
        for _ in range(a.reps):
            for key, fn in (('fused', fused), ('autograd', lambda: autograd_fit(fields, t))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1))
        wf, wa = fused()[0].cpu(), autograd_fit(fields, t).cpu()
        c = dict(fused_fit=_spread(ms['fused']), torch_autograd_fp32_fit=_spread(ms['autograd']))
        c['speedup_of_medians'] = round(c['torch_autograd_fp32_fit']['median_ms'] / c['fused_fit']['median_ms'], 2)
        c['fused_us_per_epoch'] = round(c['fused_fit']['median_ms'] * 1e3 / epochs, 2)
        c['fused_pixel_evaluations_per_s'] = round(3.0 * out_hw[0] * out_hw[1] * epochs / (c['fused_fit']['median_ms'] * 1e-3), 0)
        c['weights_fused'], c['weights_autograd_fp32'] = wf.tolist(), wa.tolist()
        c['weights_distance'] = float((wf - wa).abs().max())
        res['cases'][name] = c
    if not a.persam_f_once:
        pv = torch.randn(1, 3, 1024, 1024, device=dev)
        with torch.no_grad():
            res['encoder_pass'] = timed(lambda: model.get_image_embeddings(pv), max(5, a.reps))
    return res


def regions_fixture(k, hw, dev, seed=0):
    """thresholded smooth noise plus speckle: bool [k, H, W] on the device"""
    g = torch.Generator().manual_seed(seed)
    z = torch.nn.functional.interpolate(torch.randn(k, 1, 24, 24, generator=g), size=hw, mode='bicubic', align_corners=False)[:, 0]
    m = z > 0
    flip = torch.rand(k, hw[0], hw[1], generator=g) < 0.002                            # pinholes and detached specks
    return (m ^ flip).to(dev).contiguous()


def regions(model, img, a):
    from rsprompter_amd import ops
    from rsprompter_amd.sam_prompts import SamMaskGenerator, SamSession, point_grid
    dev = img.device
    k, hw, area = 64, (1024, 1024), 100
    masks = regions_fixture(k, hw, dev)
    out = dict(masks=k, size=list(hw), min_area=area, modes={})
    if a.regions_once:
        for mode in ('holes', 'islands', 'both'):
            ops.remove_small_regions(masks, area, mode)
        torch.cuda.synchronize()
        return out
    for _ in range(3):                                                                 # the encoder leg: clocks are warm after it
        SamSession(model, img)
    npx = k * hw[0] * hw[1]
    for mode, passes in (('holes', 1), ('islands', 1), ('both', 2)):
        t = timed(lambda: ops.remove_small_regions(masks, area, mode), max(a.reps, 20))
        floor_ms = npx * REGION_BYTES_PER_PIXEL_PASS * passes / (NORM_STREAM_TB_S * 1e12) * 1e3
        _, info = ops.remove_small_regions(masks, area, mode)
        info = info.cpu()
        t.update(bytes_floor_ms=round(floor_ms, 3), times_the_floor=round(t['median_ms'] / floor_ms, 2),
                 Gpixel_per_s=round(npx / (t['median_ms'] * 1e-3) / 1e9, 2), masks_changed=int((info[:, :2].sum(1) > 0).sum()),
                 status_nonzero=int((info[:, 7] != 0).sum()))
        out['modes'][mode] = t
    out['bytes_floor'] = dict(bytes_per_pixel_per_pass=REGION_BYTES_PER_PIXEL_PASS, stream_TB_per_s=NORM_STREAM_TB_S,
                              formula='masks * H * W * bytes_per_pixel_per_pass * passes / stream rate; passes = 2 for both')
    # the host route this replaces: masks to the host, scipy per mask, results back
    from scipy import ndimage
    eight = np.ones((3, 3), dtype=np.int32)

    def host_clean(m, holes):
        w = ~m if holes else m
        lab, n = ndimage.label(w, structure=eight)
        if n == 0:
            return m
        sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
        small = sizes < area
        if not small.any():
            return m
        if holes:
            return m | np.isin(lab, np.nonzero(small)[0] + 1)
        keep = np.nonzero(~small)[0] + 1
        return np.isin(lab, keep if len(keep) else [int(np.argmax(sizes)) + 1])

    def host_route():
        h = masks.cpu().numpy()
        res = np.stack([host_clean(host_clean(m, True), False) for m in h])
        return torch.from_numpy(res).to(dev)
    import time
    ts = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = host_route()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    out['host_route_both'] = dict(ms=[round(t, 1) for t in ts], equal_to_the_device_result=bool(torch.equal(want, ops.remove_small_regions(masks, area)[0])),
                                  note='device -> host, scipy.ndimage.label twice per mask (one thread), host -> device')
    # the generator with and without the step, alternating in this process
    H, W = int(img.shape[0]), int(img.shape[1])
    S, off, n = model.image_size, 0.25, 32
    s0 = SamSession(model, img)
    low, iou = s0._low_res((point_grid(n) * np.array([[W, H]]))[:, None, :], None, None, None, True)
    sc = ops.mask_score_box(low.reshape(low.shape[0] * 3, 256, 256), (S, S), s0.input_size, (H, W), 0.0, off)
    stab = sc[:, 0] / sc[:, 1]
    kw = dict(points_per_side=n, pred_iou_thresh=float(iou.median()), stability_score_thresh=float(stab[~stab.isnan()].median()),
              stability_score_offset=off, crop_n_layers=1, crop_batch=a.crop_batch)
    del s0, low, iou, sc
    gens = {0: SamMaskGenerator(model, **kw), area: SamMaskGenerator(model, min_mask_region_area=area, **kw)}
    res = {ar: g.generate(img) for ar, g in gens.items()}
    ts = {ar: [] for ar in gens}
    ph, phs = _Phases(), []
    for r in range(max(3, a.reps // 4)):
        for ar, g in gens.items():
            g._phase = ph
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.generate(img)
            e1.record()
            e1.synchronize()
            ts[ar].append(e0.elapsed_time(e1))
            p = ph.take()
            if ar:
                phs.append(p)
    out['generate_layers1'] = {f'min_mask_region_area_{ar}': dict(_spread(t), instances=len(res[ar].masks)) for ar, t in ts.items()}
    out['generate_layers1']['changed'] = int(res[area].region_changed.sum())
    out['generate_layers1'][f'phases_ms_area_{area}'] = {k_: round(statistics.median([p[k_] for p in phs]), 3) for k_ in phs[0]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arch', default='huge')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--multicrop', action='store_true', help='the crop-layer phase (d) only')
    ap.add_argument('--multicrop-once', action='store_true', help='one generate() per configuration (for a kernel trace)')
    ap.add_argument('--persam', action='store_true', help='the PerSAM phase (e) only')
    ap.add_argument('--persam-once', action='store_true', help='one segment() per batch size (for a kernel trace)')
    ap.add_argument('--regions', action='store_true', help='the min_mask_region_area phase (f) only')
    ap.add_argument('--regions-once', action='store_true', help='one remove_small_regions call per mode (for a kernel trace)')
    ap.add_argument('--persam-f', action='store_true', help="the PerSAM-F phase (g) only")
    ap.add_argument('--persam-f-once', action='store_true', help='one fit per geometry (for a kernel trace)')
    ap.add_argument('--crop-batch', type=int, default=None)
    ap.add_argument('--crop-batches', type=lambda v: [int(x) for x in v.split(',')], default=[1, 2, 4, 8])
    a = ap.parse_args()
    from rsprompter_amd import ops
    from rsprompter_amd.samdet import SamModelHIP
    from rsprompter_amd.rle import encode_mask_dicts
    from rsprompter_amd.sam_prompts import SamSession, filter_candidates, generate_masks, point_grid
    from rsprompter_amd.synth import synth_images, synth_state_dict
    dev = torch.device('cuda:0')
    model = SamModelHIP(a.arch)
    sd = synth_state_dict(model, seed=0)
    sd['shared_image_embedding.positional_embedding'] = sd['prompt_encoder.shared_embedding.positional_embedding']   # HF ties them
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    img = synth_images(1)[0].permute(1, 2, 0).contiguous().to(dev)                 # [1024, 1024, 3] uint8
    out = dict(arch=a.arch, device=torch.cuda.get_device_name(0), image=[1024, 1024])
    if a.multicrop or a.multicrop_once or a.persam or a.persam_once or a.regions or a.regions_once or a.persam_f or a.persam_f_once:
        if a.persam_f or a.persam_f_once:
            out['persam_f'] = persam_f(model, a)
        elif a.regions or a.regions_once:
            out['regions'] = regions(model, img, a)
        elif a.persam or a.persam_once:
            out['persam'] = persam(model, a)
        else:
            out['multicrop'] = multicrop(model, img, a)
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write(json.dumps(out, indent=1) + '\n')
        return
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
            encode_mask_dicts(s.full_res(low[sel[i:i + 64]], 0.0))
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
