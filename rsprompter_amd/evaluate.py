"""Test-set evaluation of a config + checkpoint: the equivalent of the reference's tools/test.py / tools/dist_test.sh
(tools/dist_test.sh:10-22) with the configs' `test_evaluator = dict(type='CocoMetric', metric=['bbox', 'segm'])`.

    python -m rsprompter_amd.evaluate CONFIG CHECKPOINT [--data-root DIR] [--ann-file F] [--cfg-options k=v ...]
                                      [--out-prefix P]
    torchrun --nproc_per_node 8 -m rsprompter_amd.evaluate CONFIG CHECKPOINT ...

Every rank runs `model.test_step` through `apis.TestPipeline` on its DefaultSampler shard (`dist.shard_indices`) at the
config's batch size; the predictions reach rank 0 through `dist.gather_results` (device-made COCO RLE strings); rank 0
runs `CocoMetric` (device IoU + matching, host accumulate), prints pycocotools' summary and writes the metrics as JSON.
Ground truth travels next to the pipeline output: rank 0 reads it from the dataset (the same result as gathering it).
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


@torch.no_grad()
def evaluate(model, cfg, data_root=None, ann_file=None, out_prefix=None, metric_ann_file=None, device=None,
             verbose=True, gt_raster=None):
    """Run the test set of `cfg` through `model` on this rank's shard; on rank 0 return the metrics dict (mmdet's keys),
    elsewhere None.  `metric_ann_file` sets CocoMetric's ann_file (the ground-truth JSON path of the reference's metric);
    by default the metric converts the dataset's ground truth as every RSPrompter config does.  `gt_raster` ('host' /
    'device') overrides who rasterises the metric's ground-truth polygons (CocoMetric's gt_raster; None: the config's)."""
    import torch.distributed as dist
    ds = build_test_dataset(cfg, data_root, ann_file)
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    pipeline = TestPipeline(cfg['test_dataloader']['dataset']['pipeline'], device=dev)
    bs = int(cfg['test_dataloader'].get('batch_size', 1))
    shards = [rdist.shard_indices(len(ds), r, world) for r in range(world)]
    mine = shards[rank]
    order, preds = [], []
    for s in range(0, len(mine), bs):
        chunk = [pipeline(dict(img_path=ds.data_list[i]['img_path'], img_id=ds.data_list[i]['img_id']))
                 for i in mine[s:s + bs]]
        out = model.test_step(dict(inputs=[c['inputs'] for c in chunk], data_samples=[c['data_samples'] for c in chunk]))
        got = rdist.gather_results([o.pred_instances for o in out], device=dev)
        if got is None:
            continue
        # gathered step order: image i of every rank in rank order (mmengine collect_results' zip)
        step = [shards[w][s + i] for i in range(bs) for w in range(world) if s + i < len(shards[w])]
        order.extend(step)
        preds.extend(got[j] for j in range(len(got)))
    if rank != 0:
        return None
    first = {}
    for j, i in enumerate(order):
        first.setdefault(i, j)                       # the sampler's wrap-around duplicates dropped
    idx = sorted(first)
    ev_cfg = dict(cfg['test_evaluator'])
    if metric_ann_file is not None:
        ev_cfg['ann_file'] = metric_ann_file
    if out_prefix is not None and ev_cfg.get('outfile_prefix') is None:
        ev_cfg['outfile_prefix'] = out_prefix
    if gt_raster is not None:
        ev_cfg['gt_raster'] = gt_raster
    metric = METRICS.build(ev_cfg)
    metric.dataset_meta = ds.dataset_meta
    metric.device = str(dev)
    metric.process(None, _samples_for_metric(ds, idx, [preds[first[i]] for i in idx]))
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
    args = ap.parse_args(argv)
    rank, local, world = rdist.init_from_env()
    cfg = Config.fromfile(args.config)
    if args.cfg_options:
        cfg.merge_from_dict(_parse_cfg_options(args.cfg_options))
    model = init_detector(cfg, args.checkpoint, device=f'cuda:{local}')
    res = evaluate(model, cfg, args.data_root, args.ann_file, args.out_prefix, verbose=rank == 0, gt_raster=args.gt_raster)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return res


if __name__ == '__main__':
    main(sys.argv[1:])
