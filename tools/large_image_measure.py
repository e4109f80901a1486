"""Measurements behind DESIGN §14 (sliced inference on large scenes); needs the GPU.

  python tools/large_image_measure.py throughput   ViT-H, batch 8, a 4096 x 6400 scene (40 tiles of 1024): tiles/s of
                                                   inference_large_image against model.test_step alone on the same 40
                                                   tiles (bench.py's step), alternating, 2 warm-ups + 4 repeats each
  python tools/large_image_measure.py phases       the same call with a device synchronise around every phase (additive,
                                                   a little slower than free-running) and the peak memory of both forms
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/large_image_measure.py profile
                                                   ViT-B, batch 4, the 4096 x 5000 scene of tests/test_gpu_large_image.py, twice

The scene is a mosaic of the committed NWPU images (tests/golden/coco_nwpu); weights are the seeded synthetic ones, whose
masks are noise: tens of thousands of runs per instance, where a trained model gives hundreds."""
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAD = (0.406 * 255, 0.456 * 255, 0.485 * 255)


def mosaic(H, W):
    from rsprompter_amd.apis import TestPipeline
    d = os.path.join(ROOT, 'tests', 'golden', 'coco_nwpu', 'imgs')
    imgs = [TestPipeline._decode(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.jpg')]
    scene = np.zeros((H, W, 3), np.uint8)
    y, i = 0, 0
    while y < H:
        x = 0
        while x < W:
            im = imgs[i % len(imgs)]
            i += 1
            hh, ww = min(im.shape[0], H - y), min(im.shape[1], W - x)
            scene[y:y + hh, x:x + ww] = im[:hh, :ww]
            x += ww
        y += 383
    return scene


def build(arch, dev):
    import rsprompter_amd as ra
    from rsprompter_amd.config import Config
    from rsprompter_amd.default_configs import rsprompter_anchor
    from rsprompter_amd.synth import synth_state_dict
    cfg = Config(dict(model=rsprompter_anchor(arch, 10), test_dataloader=dict(dataset=dict(pipeline=[
        dict(type='LoadImageFromFile', backend_args=None, to_float32=True),
        dict(type='Resize', scale=(1024, 1024), keep_ratio=True),
        dict(type='Pad', size=(1024, 1024), pad_val=dict(img=PAD, masks=0)),
        dict(type='PackDetInputs', meta_keys=('img_id', 'img_path', 'ori_shape', 'img_shape', 'scale_factor'))]))))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = ra.build_model(cfg)
    m.load_state_dict(synth_state_dict(m, seed=0), strict=True)
    m.cfg = cfg
    return m.to(dev)


def plain_batches(m, scene, dev, n_tiles=40):
    """the tiles of the scene as device-resident batches of 8 + a function that runs bench.py's step over them"""
    from rsprompter_amd import ops
    from rsprompter_amd.apis import TestPipeline, get_test_pipeline_cfg
    from rsprompter_amd.large_image import slice_bboxes
    from rsprompter_amd.structures import DetDataSample
    H, W = scene.shape[:2]
    tiles = slice_bboxes(H, W, 1024, 1024, 0.25, 0.25)[:n_tiles]
    pipe = TestPipeline(get_test_pipeline_cfg(m.cfg), device=dev)
    nh, nw, ph, pw, meta = pipe.geometry(1024, 1024)
    origins = torch.tensor([[t[0], t[1]] for t in tiles], dtype=torch.int32, device=dev)
    dscene = torch.from_numpy(scene).to(dev)
    batches = [ops.slice_resize_pad(dscene, origins[i:i + 8], (1024, 1024), (nh, nw), (ph, pw), pipe.pad_val)
               for i in range(0, len(tiles), 8)]
    keys = {k: v for k, v in dict(meta, img_id=0, img_path=None).items() if k in pipe.meta_keys}

    def plain():
        for b in batches:
            m.test_step(dict(inputs=[b[j] for j in range(b.shape[0])],
                             data_samples=[DetDataSample(metainfo=dict(keys)) for _ in range(b.shape[0])]))
        torch.cuda.synchronize()
    return len(tiles), plain


def throughput(dev):
    from rsprompter_amd.large_image import inference_large_image
    m = build('huge', dev)
    scene = mosaic(4096, 6400)
    n, plain = plain_batches(m, scene, dev)

    def sliced():
        out = inference_large_image(m, scene, patch_size=1024, batch_size=8)
        torch.cuda.synchronize()
        return out
    res = dict(tiles=n, plain_s=[], sliced_s=[])
    for f in (plain, sliced, plain, sliced):
        f()
    for _ in range(4):
        for name, f in (('plain_s', plain), ('sliced_s', sliced)):
            t0 = time.perf_counter()
            f()
            res[name].append(time.perf_counter() - t0)
    med = lambda v: sorted(v)[len(v) // 2]                                      # noqa: E731
    res.update(plain_tiles_per_s=n / med(res['plain_s']), sliced_tiles_per_s=n / med(res['sliced_s']),
               overhead_pct_of_medians=100.0 * (med(res['sliced_s']) / med(res['plain_s']) - 1.0))
    return res


def phases(dev):
    from rsprompter_amd import large_image as li
    from rsprompter_amd import ops, rle
    m = build('huge', dev)
    scene = mosaic(4096, 6400)
    T = {}

    def wrap(obj, name, key):
        f = getattr(obj, name)

        def g(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = f(*a, **k)
            torch.cuda.synchronize()
            T[key] = T.get(key, 0.0) + time.perf_counter() - t
            return r
        setattr(obj, name, g)
        return obj, name, f
    for _ in range(2):
        li.inference_large_image(m, scene, patch_size=1024, batch_size=8)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    li.inference_large_image(m, scene, patch_size=1024, batch_size=8)
    torch.cuda.synchronize()
    free = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated() / 2 ** 20
    saved = [wrap(ops, 'slice_resize_pad', 'front_end'), wrap(m, 'test_step', 'model'), wrap(rle, 'encode_runs', 'tile_rle'),
             wrap(ops, 'nms_flat', 'merge_nms'), wrap(li, '_scene_rle', 'scene_rle'), wrap(ops, 'rle_shift', 'scene_rle.shift'),
             wrap(ops, 'rle_to_string', 'scene_rle.strings')]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = li.inference_large_image(m, scene, patch_size=1024, batch_size=8)
    torch.cuda.synchronize()
    tot = time.perf_counter() - t0
    for o, n, f in saved:
        setattr(o, n, f)
    T['other'] = tot - sum(v for k, v in T.items() if '.' not in k)
    p = out.pred_instances
    res = dict(free_running_s=free, synced_total_s=tot, phases_s=T, kept=len(p.scores), string_bytes=sum(len(r['counts']) for r in p.masks),
               peak_sliced_mib=peak, dense_kept_masks_mib=len(p.scores) * 4096 * 6400 / 2 ** 20)
    del out, p
    _, plain = plain_batches(m, scene, dev, n_tiles=8)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    plain()
    res['peak_plain_step_mib'] = torch.cuda.max_memory_allocated() / 2 ** 20
    return res


def profile(dev):
    from rsprompter_amd.large_image import inference_large_image
    m = build('base', dev)
    scene = mosaic(4096, 5000)
    for _ in range(2):
        out = inference_large_image(m, scene, patch_size=1024, batch_size=4)
        torch.cuda.synchronize()
    p = out.pred_instances
    return dict(calls=2, tiles=35, kept=len(p.scores), string_bytes=sum(len(r['counts']) for r in p.masks))


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('large_image_measure.py needs the GPU: a CPU run measures nothing')
    mode = sys.argv[1] if len(sys.argv) > 1 else 'throughput'
    print(json.dumps({mode: dict(throughput=throughput, phases=phases, profile=profile)[mode](torch.device('cuda:0'))}))
