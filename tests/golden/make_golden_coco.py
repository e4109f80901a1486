"""A small NWPU VHR-10 validation subset for the evaluation tests (tests/test_coco_eval_cpu.py, tests/test_gpu_coco_eval.py):
the val annotations cut down to a few images, in the JSON's own (unsorted) image order, plus those images' JPEGs.  001.jpg
is included because it carries annotation id 0 (the pycocotools match-marker quirk).  Run where the reference
is checked out:
  python tests/golden/make_golden_coco.py <reference checkout>"""
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'coco_nwpu')
FILES = ('506.jpg', '268.jpg', '274.jpg', '136.jpg', '018.jpg', '001.jpg')


def main(ref_root):
    src = os.path.join(ref_root, 'data', 'NWPU')
    with open(os.path.join(src, 'annotations', 'NWPU_instances_val.json')) as f:
        d = json.load(f)
    images = [im for im in d['images'] if im['file_name'] in FILES]          # JSON order kept
    ids = {im['id'] for im in images}
    out = dict(info=d.get('info'), licenses=d.get('licenses'), categories=d['categories'], images=images,
               annotations=[a for a in d['annotations'] if a['image_id'] in ids])
    os.makedirs(os.path.join(OUT, 'imgs'), exist_ok=True)
    with open(os.path.join(OUT, 'NWPU_instances_val_subset.json'), 'w') as f:
        json.dump(out, f)
    for im in images:
        shutil.copyfile(os.path.join(src, 'imgs', im['file_name']), os.path.join(OUT, 'imgs', im['file_name']))
    print(len(images), 'images', len(out['annotations']), 'annotations')


if __name__ == '__main__':
    main(sys.argv[1])
