"""The reference's configs/rsprompter/*.py files as rsprompter_amd.Config.fromfile read them in the container that has the
reference checkout (tests/golden/reference_configs.pt, written by tests/golden/make_golden_configs.py).  Test
infrastructure: the config tests build from these instead of reaching for the reference checkout."""
import os

import torch

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_configs.pt')


def _decode(x):
    if isinstance(x, dict):
        if set(x) == {'__range__'}:
            return range(*x['__range__'])
        return {k: _decode(v) for k, v in x.items()}
    if isinstance(x, list):
        return [_decode(v) for v in x]
    if isinstance(x, tuple):
        return tuple(_decode(v) for v in x)
    return x


def names():
    return sorted(torch.load(PATH, weights_only=True))


def reference_config(fname):
    """rsprompter_amd.Config of configs/rsprompter/<fname>"""
    from rsprompter_amd.config import Config, _to_cd
    return Config(_to_cd(_decode(torch.load(PATH, weights_only=True)[fname])))
