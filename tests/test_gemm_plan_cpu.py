"""CPU: rsp_gemm_plan (csrc/gemm_plan.hip) against the kernels that rsp_gemm was SEEN to launch on the device.

tests/golden/gemm_plan.json is the table that tools/gemm_plan_trace.py recorded under `rocprofv3 --kernel-trace`: for every
descriptor of its grid the demangled name of the kernel that ran, with its template arguments, or EINVAL, or `none`
(M == 0).  The plan reads alignments only and dereferences nothing, so here the descriptors carry made-up pointers."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'gemm_plan.json')) as _f:
    ROWS = json.load(_f)

# kernel name -> (RSP_GEMM_KERNEL_*, the plan field of every template argument; `-` = the reserved EPI of the dma kernel)
FAMILIES = {
    'gemm_f16x3_kernel': ('F32A', 'bm bn wgm wgn'),
    'gemm_f16x3_dma_kernel': ('DMA', 'bm bn wgm wgn nbuf var - pipe conv ord f8'),
    'gemm_f16x3_s2_kernel': ('S2', 'var epi'),
    'gemm_f16x3_pp_kernel': ('PP', 'epi var bm'),
}


def _desc(_lib, rec):
    d = _lib.RspGemmDesc()
    for name, v in rec.items():
        if name != 'ptrs':
            setattr(d, name, v)
    for i, p in enumerate(rec['ptrs'].split()):     # 'C' | 'C+4': a distinct 16-byte aligned address, plus the offset
        name, _, off = p.partition('+')
        setattr(d, name, ((i + 1) << 20) + int(off or 0))
    return d


def test_golden_table_covers_the_families_and_forms():
    names = {r['kernel'] for r in ROWS}
    assert 300 <= len(ROWS) and {'EINVAL', 'none'} <= names
    forms = (4, 5, 21, 12, 28, 8, 10, 6)
    assert {f'gemm_f16x3_s2_kernel<0, {e}>' for e in forms + (64,)} <= names
    assert {f'gemm_f16x3_pp_kernel<{e}, 0, {bm}>' for e in forms for bm in (128, 256)} <= names
    assert len({n for n in names if n.startswith('gemm_f16x3_dma_kernel')}) >= 26 and len({n for n in names if n.startswith('gemm_f16x3_kernel')}) == 3


@pytest.mark.parametrize('i', range(len(ROWS)))
def test_plan_is_the_kernel_that_ran(i):
    from rsprompter_amd import _lib, ops
    lib, row = _lib.load(), ROWS[i]
    K = {k[16:]: v for k, v in _lib.CONST.items() if k.startswith('RSP_GEMM_KERNEL_')}
    d, p = _desc(_lib, row['desc']), _lib.RspGemmPlan()
    rc = lib.rsp_gemm_plan(ctypes.byref(d), ctypes.byref(p))
    got = {f: getattr(p, f) for f, _ in p._fields_}
    want = dict.fromkeys(got, 0)
    if row['kernel'] not in ('EINVAL', 'none'):
        name, args = re.fullmatch(r'(\w+)<(.*)>', row['kernel']).groups()
        want['kernel'] = K[FAMILIES[name][0]]
        for f, a in zip(FAMILIES[name][1].split(), args.split(', '), strict=True):
            if f == '-':
                assert a == '0'
            else:
                want[f] = {'false': 0, 'true': 1}[a] if a in ('false', 'true') else int(a)
        if name in ('gemm_f16x3_s2_kernel', 'gemm_f16x3_pp_kernel'):     # their tile widths are constants of the files
            want['bn'] = 128 if name == 'gemm_f16x3_s2_kernel' else 256
            want['bm'] = want['bm'] or 256
    assert rc == (_lib.CONST['RSP_EINVAL'] if row['kernel'] == 'EINVAL' else 0), row['call']
    assert got == want, row['call']
    # the plan under its earlier names, and the profiler label
    assert lib.rsp_gemm_uses_s2(ctypes.byref(d)) == (p.kernel == K['S2'])
    assert lib.rsp_gemm_s2_epilogue(ctypes.byref(d)) == (p.epi if p.kernel == K['S2'] else -1)
    assert lib.rsp_gemm_uses_pp(ctypes.byref(d)) == (p.bm if p.kernel == K['PP'] else 0)
    if p.kernel == K['NONE']:
        assert ops._gemm_label(d) == 'rsp_gemm'
    else:
        name = row['kernel'].split('<')[0]
        assert ops._gemm_label(d) == f"{'gemm_f16f8_dma_kernel' if p.f8 else name}<{p.bm}x{p.bn}>"


def test_plan_refuses_null_arguments():
    from rsprompter_amd import _lib
    lib = _lib.load()
    p = _lib.RspGemmPlan(kernel=7)
    assert lib.rsp_gemm_plan(None, ctypes.byref(p)) == _lib.CONST['RSP_EINVAL'] and p.kernel == 0
    assert lib.rsp_gemm_plan(ctypes.byref(_lib.RspGemmDesc()), None) == _lib.CONST['RSP_EINVAL']
