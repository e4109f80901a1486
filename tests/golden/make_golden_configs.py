"""The reference's configs/rsprompter/*.py as this project's loader reads them (rsprompter_amd.Config.fromfile: `_base_`
inheritance and `_delete_` already applied), stored as plain dicts / lists / tuples / scalars in reference_configs.pt
(a `range` as {'__range__': (start, stop, step)}; tests/_ref_configs.py reads the file back into a Config), so that the
config tests run without the reference checkout.  Run where the reference is checked out:
  python tests/golden/make_golden_configs.py <reference checkout>"""
import glob
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, list):
        return [plain(v) for v in x]
    if isinstance(x, tuple):
        return tuple(plain(v) for v in x)
    if isinstance(x, range):
        return {'__range__': (x.start, x.stop, x.step)}
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    raise TypeError(f'unexpected {type(x).__name__} in a config')


def main(ref_root):
    import rsprompter_amd as ra
    out = {}
    for path in sorted(glob.glob(os.path.join(ref_root, 'configs', 'rsprompter', '*.py'))):
        out[os.path.basename(path)] = plain(dict(ra.Config.fromfile(path)))
    torch.save(out, os.path.join(HERE, 'reference_configs.pt'))
    print(sorted(out))


if __name__ == '__main__':
    main(sys.argv[1])
