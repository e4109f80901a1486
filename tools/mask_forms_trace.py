"""One call of every caller-facing function that converts between mask forms (dense, RLE dicts, run table), on the wave
emulator, which runs on a CPU: the `rsp_*` entry points each call reaches, in order, and its device-to-host reads (the
counter of tests/_run_morphology_cases.py; on the emulator it also counts the reads of host tensors, the same ones on both
sides of a comparison).

    python tools/mask_forms_trace.py --out FILE

Run it at two commits and compare the files: a change that only moves the conversions leaves them equal
(profiles/mask_forms/README.md).  Only public functions are called, so the script runs at either commit."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'wave_emu'))


class _Logging:
    """the library handle with every rsp_* call appended to `calls`"""

    def __init__(self, lib):
        self.__dict__['_lib'], self.__dict__['calls'] = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('rsp_') or name.endswith('_bytes'):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    import harness
    from _run_morphology_cases import ReadCounter
    from rsprompter_amd import _lib, apis, evaluation, rle
    dev = torch.device('cpu')
    rng = np.random.default_rng(5)
    H, W = 20, 27
    yy, xx = np.mgrid[:H, :W]
    dense = np.stack([(yy - 9) ** 2 + (xx - 12) ** 2 < 40, (yy + xx) % 2 == 1, rng.random((H, W)) < 0.7,
                      np.zeros((H, W), bool)])
    dense[0, 8:11, 11:14] = False                                                       # a hole
    doc = {}
    with harness.emulated_ops():
        log = _lib._lib = _Logging(_lib._lib)

        def run(name, fn):
            del log.calls[:]
            with ReadCounter(dev) as rc:
                fn()
            doc[name] = dict(reads=rc.n, calls=list(log.calls))
        t = torch.from_numpy(dense)
        strings = rle.encode_mask_results(t)
        text = [dict(size=s['size'], counts=s['counts'].decode()) for s in strings]
        lists = rle.encode_mask_dicts(t)
        mixed = [strings[0], lists[1], text[2], lists[3]]
        forms = dict(dense=t, strings=strings, text=text, lists=lists)
        for form, m in forms.items():
            run(f'remove_small_regions/{form}', lambda: apis.remove_small_regions(m, 4, 'both', device=dev))
            run(f'masks_to_polygons/{form}', lambda: apis.masks_to_polygons(m, device=dev))
            run(f'masks_to_polygons/simplified/{form}', lambda: apis.masks_to_polygons(m, 'coco', device=dev, tolerance=1.0))
            run(f'masks_to_obb/{form}', lambda: apis.masks_to_obb(m, device=dev))
            run(f'masks_to_obb/per_component/{form}', lambda: apis.masks_to_obb(m, 'hull', device=dev, per_component=True))
            run(f'mask_components/{form}', lambda: apis.mask_components(m, device=dev))
            for op in apis.MORPHOLOGY_OPS:
                run(f'mask_morphology/{op}/{form}', lambda: apis.mask_morphology(m, op, 1, device=dev))
            run(f'mask_boundary/{form}', lambda: apis.mask_boundary(m, device=dev))
        forms['mixed'] = mixed
        for form, m in forms.items():
            crowd = [False, True, False, False]
            run(f'mask_iou/{form}', lambda: apis.mask_iou(m[:3], m, crowd, device=dev))
            run(f'boundary_iou/{form}', lambda: apis.boundary_iou(m[:3], m, crowd, device=dev))
            run(f'boundary_iou/min_with_mask/{form}', lambda: apis.boundary_iou(m[:3], m, crowd, radius=2, min_with_mask=True,
                                                                                device=dev))
        run('mask_iou/dense_against_mixed', lambda: apis.mask_iou(t, mixed, device=dev))
        run('mask_iou/empty_side', lambda: apis.mask_iou([], strings, device=dev))
        polys = apis.masks_to_polygons(t, 'coco', device=dev)
        rings = apis.masks_to_polygons(t, 'rings', device=dev)
        for form in apis.MASK_FORMS:
            run(f'polygons_to_masks/coco/{form}', lambda: apis.polygons_to_masks(polys, (H, W), form, device=dev))
            run(f'polygons_to_masks/rings/{form}', lambda: apis.polygons_to_masks(rings, (H, W), form, device=dev))
        run('encode_mask_results', lambda: rle.encode_mask_results(t))
        # device_evaluate: two images of different sizes, so that the word offsets are not a multiple of one size
        small = rle.encode_mask_results(torch.from_numpy(dense[:, :9, :15].copy()))
        gt = dict(images=[dict(id=1, height=H, width=W), dict(id=2, height=9, width=15)], categories=[dict(id=0, name='a')],
                  annotations=[dict(id=i + 1, image_id=1 + i // 4, category_id=0, area=float(d.sum()), iscrowd=int(i == 1),
                                    bbox=[0, 0, 1, 1], segmentation=s)
                               for i, (s, d) in enumerate(zip(strings + small, list(dense) + list(dense[:, :9, :15])))])
        dts = [dict(id=i + 1, image_id=1 + i // 4, category_id=0, score=1.0 - 0.1 * i, segmentation=s, bbox=[0, 0, 1, 1],
                    area=1.0) for i, s in enumerate((strings + small)[::-1][4:] + (strings + small)[::-1][:4])]
        dts = [dict(d, image_id=1 if d['segmentation']['size'] == [H, W] else 2) for d in dts]
        for iou_type in ('bbox', 'segm', 'boundary'):
            for domain in ('bits', 'runs', 'auto'):
                if iou_type == 'bbox' and domain != 'bits':
                    continue
                run(f'device_evaluate/{iou_type}/{domain}',
                    lambda: evaluation.device_evaluate(gt, dts, iou_type, [1, 2], [0], [0.5, 0.75], [1, 10, 100], dev,
                                                       timings={}, iou_domain=domain))
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps({k: [v['reads'], len(v['calls'])] for k, v in doc.items()}))
    return doc


if __name__ == '__main__':
    main(sys.argv[1:])
