"""Test-set evaluation of a config + checkpoint: the equivalent of the reference's tools/test.py / tools/dist_test.sh
(tools/dist_test.sh:10-22) with the configs' `test_evaluator = dict(type='CocoMetric', metric=['bbox', 'segm'])`.

    python -m rsprompter_amd.evaluate CONFIG CHECKPOINT [--data-root DIR] [--ann-file F] [--cfg-options k=v ...]
                                      [--out-prefix P] [--iou-domain bits|runs|auto]
                                      [--large-image [--patch-size N] [--patch-overlap-ratio R] [--merge-iou-thr T]
                                       [--merge-nms-type nms|seam_mask] [--seam-iou-thr T] [--batch-size B]
                                       [--min-mask-region-area A]]
    torchrun --nproc_per_node 8 -m rsprompter_amd.evaluate CONFIG CHECKPOINT ...

Every rank runs `model.test_step` through `apis.TestPipeline` on its DefaultSampler shard (`dist.shard_indices`) at the
config's batch size; the predictions reach rank 0 through `dist.gather_results` (device-made COCO RLE strings); rank 0
runs `CocoMetric` (device IoU + matching, host accumulate), prints pycocotools' summary and writes the metrics as JSON.
Ground truth travels next to the pipeline output: rank 0 reads it from the dataset (the same result as gathering it).

--large-image: every image of the dataset is a SCENE -- a COCO JSON whose `images` are scenes is all it
takes -- and goes through `inference_large_image(masks='rle')` instead of `test_step`; the per-scene predictions, already
host strings, reach rank 0 with `torch.distributed.gather_object`, and the metric scores them in the run domain
(`CocoMetric(iou_domain='runs')`): no scene-sized mask exists as pixels or bits anywhere on the way.
"""
import argparse
import copy
import json
import os
import sys

import torch

from . import dist as rdist
from .apis import TestPipeline
from .datasets import DATASETS
from .evaluation import METRICS


def build_test_dataset(cfg, data_root=None, ann_file=None):
    ds_cfg = copy.deepcopy(dict(cfg['test_dataloader']['dataset']))
    if data_root is not None:
        ds_cfg['data_root'] = data_root
    if ann_file is not None:
        ds_cfg['ann_file'] = ann_file
    return DATASETS.build(ds_cfg)


def _samples_for_metric(ds, order, preds):
    """(dataset index, gathered prediction dict) -> the data-sample dicts CocoMetric.process reads"""
    out = []
    for i, p in zip(order, preds):
        item = ds[i]
        keep = ~item['ignore_flags']
        gt = dict(bboxes=item['bboxes'][keep], labels=item['labels'][keep],
                  masks=[m for m, k in zip(item['masks'], keep) if k])
        out.append(dict(pred_instances=p, img_id=item['img_id'], ori_shape=item['ori_shape'], gt_instances=gt))
    return out


def step_order(shards, s, bs):
    """the dataset indices of the predictions gathered in the step that starts at position s of every shard: image i of
    every rank in rank order (mmengine collect_results' zip)"""
    return [sh[s + i] for i in range(bs) for sh in shards if s + i < len(sh)]


def rank_order(shards):
    """... of per-rank lists gathered whole (gather_object): rank after rank, each in its shard's order"""
    return [i for sh in shards for i in sh]


def first_predictions(order, preds):
    """(dataset index of every gathered prediction, the predictions) -> (the distinct indices in dataset order, the FIRST
    prediction of each): the sampler's wrap-around duplicates dropped.  Shared by the tile and the scene path."""
    if len(order) != len(preds):
        raise ValueError(f'{len(preds)} gathered predictions for {len(order)} dataset indices')
    first = {}
    for j, i in enumerate(order):
        first.setdefault(i, j)
    idx = sorted(first)
    return idx, [preds[first[i]] for i in idx]


LARGE_IMAGE_KEYS = ('patch_size', 'patch_overlap_ratio', 'merge_iou_thr', 'merge_nms_type', 'seam_iou_thr', 'batch_size',
                    'min_mask_region_area')


def _scene_predictions(model, ds, mine, large_image):
    """this rank's scenes through inference_large_image -> per scene the dict CocoMetric.process reads, on the host"""
    from .large_image import inference_large_image
    out = []
    for i in mine:
        pi = inference_large_image(model, ds.data_list[i]['img_path'], masks='rle', **large_image).pred_instances
        masks = getattr(pi, 'masks', None)
        out.append(dict(bboxes=pi.bboxes.cpu(), scores=pi.scores.cpu(), labels=pi.labels.cpu(),
                        masks=list(masks) if masks is not None else []))
    return out


@torch.no_grad()
def evaluate(model, cfg, data_root=None, ann_file=None, out_prefix=None, metric_ann_file=None, device=None,
             verbose=True, gt_raster=None, large_image=None, iou_domain=None, boundary=False, dilation_ratio=None, obb=False):
    """Run the test set of `cfg` through `model` on this rank's shard; on rank 0 return the metrics dict (mmdet's keys),
    elsewhere None.  `metric_ann_file` sets CocoMetric's ann_file (the ground-truth JSON path of the reference's metric);
    by default the metric converts the dataset's ground truth as every RSPrompter config does.  `gt_raster` ('host' /
    'device') overrides who rasterises the metric's ground-truth polygons (CocoMetric's gt_raster; None: the config's).
    `large_image`: a dict of inference_large_image keywords (LARGE_IMAGE_KEYS; {} for its defaults) -- every dataset item
    is then a scene, and the metric's iou_domain is 'runs' unless `iou_domain` ('bits' / 'runs' / 'auto') or the config says
    otherwise.  `iou_domain` alone overrides CocoMetric's on the tile path.  `boundary` appends 'boundary' (Boundary AP,
    DESIGN §14.13) to the metric list; `dilation_ratio` sets its band width and is refused without it.  `obb` appends 'obb'
    (oriented-box AP, DESIGN §14.17: segm with the IoU of the masks' minimum-area rectangles)."""
    import torch.distributed as dist
    if dilation_ratio is not None and not boundary:
        raise ValueError('evaluate: dilation_ratio applies to boundary=True')
    if large_image is not None:
        large_image = dict(large_image)
        unknown = sorted(set(large_image) - set(LARGE_IMAGE_KEYS))
        if unknown:
            raise ValueError(f'evaluate: large_image takes {LARGE_IMAGE_KEYS}, got {unknown}')
    ds = build_test_dataset(cfg, data_root, ann_file)
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    pipeline = TestPipeline(cfg['test_dataloader']['dataset']['pipeline'], device=dev)
    bs = int(cfg['test_dataloader'].get('batch_size', 1))
    shards = [rdist.shard_indices(len(ds), r, world) for r in range(world)]
    mine = shards[rank]
    order, preds = [], []
    if large_image is not None:
        scenes = _scene_predictions(model, ds, mine, large_image)
        per_rank = [scenes]
        if world > 1:
            per_rank = [None] * world if rank == 0 else None
            dist.gather_object(scenes, per_rank, dst=0)
        if rank == 0:
            order, preds = rank_order(shards), [p for got in per_rank for p in got]
    for s in range(0, len(mine) if large_image is None else 0, bs):
        chunk = [pipeline(dict(img_path=ds.data_list[i]['img_path'], img_id=ds.data_list[i]['img_id']))
                 for i in mine[s:s + bs]]
        out = model.test_step(dict(inputs=[c['inputs'] for c in chunk], data_samples=[c['data_samples'] for c in chunk]))
        got = rdist.gather_results([o.pred_instances for o in out], device=dev)
        if got is None:
            continue
        order.extend(step_order(shards, s, bs))
        preds.extend(got[j] for j in range(len(got)))
    if rank != 0:
        return None
    idx, preds = first_predictions(order, preds)
    ev_cfg = dict(cfg['test_evaluator'])
    if metric_ann_file is not None:
        ev_cfg['ann_file'] = metric_ann_file
    if out_prefix is not None and ev_cfg.get('outfile_prefix') is None:
        ev_cfg['outfile_prefix'] = out_prefix
    if gt_raster is not None:
        ev_cfg['gt_raster'] = gt_raster
    if iou_domain is not None:
        ev_cfg['iou_domain'] = iou_domain
    elif large_image is not None:
        ev_cfg.setdefault('iou_domain', 'runs')
    if boundary:
        listed = ev_cfg.get('metric', 'bbox')
        listed = list(listed) if isinstance(listed, (list, tuple)) else [listed]
        ev_cfg['metric'] = listed + [m for m in ('boundary',) if m not in listed]
        if dilation_ratio is not None:
            ev_cfg['dilation_ratio'] = dilation_ratio
    if obb:
        listed = ev_cfg.get('metric', 'bbox')
        listed = list(listed) if isinstance(listed, (list, tuple)) else [listed]
        ev_cfg['metric'] = listed + [m for m in ('obb',) if m not in listed]
    metric = METRICS.build(ev_cfg)
    metric.dataset_meta = ds.dataset_meta
    metric.device = str(dev)
    metric.process(None, _samples_for_metric(ds, idx, preds))
    res = metric.evaluate(len(idx))
    if verbose:
        print(metric.summary_table())
        for k, v in res.items():
            print(f'{k}: {v}')
    if out_prefix is not None:
        os.makedirs(os.path.dirname(os.path.abspath(out_prefix)), exist_ok=True)
        with open(f'{out_prefix}.metrics.json', 'w') as f:
            json.dump(res, f, indent=1)
    evaluate.last_metric = metric
    return res


def _parse_cfg_options(items):
    out = {}
    for it in items or []:
        k, v = it.split('=', 1)
        try:
            v = json.loads(v)
        except ValueError:
            pass
        out[k] = v
    return out


def main(argv=None):
    from .apis import init_detector
    from .config import Config
    ap = argparse.ArgumentParser(description='COCO bbox / segm evaluation of a config + checkpoint (tools/test.py)')
    ap.add_argument('config')
    ap.add_argument('checkpoint')
    ap.add_argument('--data-root', default=None, help='overrides test_dataloader.dataset.data_root')
    ap.add_argument('--ann-file', default=None, help='overrides test_dataloader.dataset.ann_file')
    ap.add_argument('--cfg-options', nargs='+', default=None, help='key=value overrides of the config')
    ap.add_argument('--out-prefix', default=None, help='writes <P>.bbox.json, <P>.segm.json and <P>.metrics.json')
    ap.add_argument('--gt-raster', choices=('host', 'device'), default=None,
                    help="who rasterises the metric's ground-truth polygons: the host loop (default) or the device")
    ap.add_argument('--iou-domain', choices=('bits', 'runs', 'auto'), default=None,
                    help="how the segm IoU reads the masks: bit planes, run tables, or by size (default: the config's; 'runs' "
                         'with --large-image)')
    ap.add_argument('--boundary', action='store_true',
                    help="adds Boundary AP (metric 'boundary': min(mask IoU, Boundary IoU) per pair) to the metric list")
    ap.add_argument('--dilation-ratio', type=float, default=None,
                    help='--boundary: the band width as a fraction of the image diagonal (default 0.02)')
    ap.add_argument('--obb', action='store_true',
                    help="adds oriented-box AP (metric 'obb': the IoU of the masks' minimum-area rectangles per pair) to the "
                         'metric list')
    ap.add_argument('--large-image', action='store_true',
                    help='every image of the dataset is a scene: sliced inference (inference_large_image) instead of test_step')
    ap.add_argument('--patch-size', type=int, default=None, help='--large-image: tile side in pixels')
    ap.add_argument('--patch-overlap-ratio', type=float, default=None)
    ap.add_argument('--merge-iou-thr', type=float, default=None)
    ap.add_argument('--merge-nms-type', choices=('nms', 'seam_mask', 'nms_rotated'), default=None)
    ap.add_argument('--seam-iou-thr', type=float, default=None)
    ap.add_argument('--batch-size', type=int, default=None, help='--large-image: tiles per forward pass')
    ap.add_argument('--min-mask-region-area', type=int, default=None)
    args = ap.parse_args(argv)
    given = {k: getattr(args, k) for k in LARGE_IMAGE_KEYS if getattr(args, k) is not None}
    if given and not args.large_image:
        ap.error('--' + sorted(given)[0].replace('_', '-') + ' applies to --large-image')
    if args.dilation_ratio is not None and not args.boundary:
        ap.error('--dilation-ratio applies to --boundary')
    rank, local, world = rdist.init_from_env()
    cfg = Config.fromfile(args.config)
    if args.cfg_options:
        cfg.merge_from_dict(_parse_cfg_options(args.cfg_options))
    model = init_detector(cfg, args.checkpoint, device=f'cuda:{local}')
    res = evaluate(model, cfg, args.data_root, args.ann_file, args.out_prefix, verbose=rank == 0, gt_raster=args.gt_raster,
                   large_image=given if args.large_image else None, iou_domain=args.iou_domain, boundary=args.boundary,
                   dilation_ratio=args.dilation_ratio, obb=args.obb)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return res


if __name__ == '__main__':
    main(sys.argv[1:])
