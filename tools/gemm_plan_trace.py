"""Which kernel does rsp_gemm launch for which descriptor?  A fixed grid of descriptors, walked through ops.gemm and the
ConvTranspose wrapper ops._gemm_ct in ONE process, operands all zeros, at most one GEMM launch per row and a synchronise
after it.

    rocprofv3 --kernel-trace -f csv -d OUT -- python tools/gemm_plan_trace.py --rows OUT/rows.json
    python tools/gemm_plan_trace.py --join OUT/rows.json OUT/<...>_kernel_trace.csv --golden tests/golden/gemm_plan.json

The first command records every row (its call, the RspGemmDesc that reached rsp_gemm with pointers reduced to their
alignment, and whether the call returned or raised RuntimeError); the second zips the rows that launched with the trace's
`gemm_f16` kernels in start order and writes the table  row -> kernel name with template arguments | EINVAL | none
(M == 0: rsp_gemm returns RSP_OK and launches nothing).  tests/test_gemm_plan_cpu.py holds rsp_gemm_plan to that table
without a GPU; `--list` prints the grid without touching the device.

Rows with `set` change fields of the descriptor between the wrapper and rsp_gemm: the refusals that no wrapper call
produces.  Every one of them is a descriptor that rsp_gemm refuses before it launches anything."""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HINTS = [0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 17, 18, 19, 20, 21, 22, 31, 32, 40, 104, 200, 201,
         200 | 2 << 16, 201 | 2 << 16, 7, 8, 9, 10, 15, 16]
FORMS = [                       # the eight compile-time epilogue forms, then the run-time form by each of its causes
    dict(), dict(res='f32'), dict(res='f32', c_rowmap=1), dict(out='both'), dict(out='both', c_rowmap=1),
    dict(out='planes'), dict(out='planes', act=2), dict(act=2),
    dict(N=2052), dict(act=1), dict(res='planes'), dict(res='f32', res_bmap=1), dict(out='planes', out_f8=1),
    dict(out='both', c_ncols=32, pl_col0=32)]


def grid():
    rows = []

    def g(**kw):
        r = dict(dict(kind='gemm', M=300, N=256, K=128, hint=0), **kw)
        if 'conv' in r:             # [C, H, W] of the input: M = H W and K = 9 C follow
            del r['M'], r['K']
        rows.append(r)

    for n in (32, 33, 64, 65, 128, 129, 256, 300):                  # the N and K edges of the small tiles
        for k in (32, 64, 128, 256, 288, 512, 2048):
            g(N=n, K=k)
        for k in (32, 288):
            g(N=n, K=k, a='f32')
    for m in (16128, 16384, 32512, 32768):                          # 504 / 512 / 1016 / 1024 blocks of 256 x 256
        for k in (256, 2048):
            for h in (0, 1):
                g(M=m, N=2048, K=k, hint=h)
    for h in (0, 1):
        g(M=39200, N=1280, K=1280, hint=h)                          # the ragged round of the cost model
    g(M=32768, N=1024, K=1024)                                      # pp: 512 tiles, two full rounds
    g(M=33280, N=1024, K=1024)                                      # 520 tiles: 68 % of three rounds
    g(M=16384, N=1024, K=1024, res='f32')                           # only the 128-row tile fills the chip
    g(M=16384, N=1024, K=1024)
    g(M=32768, N=1024, K=256)
    for m, n in ((3840, 2176), (4096, 2048)):                       # 255 / 256 tiles of 256 x 128
        for k in (64, 128):
            g(M=m, N=n, K=k)
    for f in FORMS:
        for h in (0, 40, 104, 200, 201):
            g(**dict(dict(M=4096, N=2048, K=128, hint=h), **f))
    for mis in ('C', 'res', 'bias'):                                # a pointer off 16 bytes: not the persistent kernels
        for h in (0, 40):
            g(M=4096, N=2048, K=128, hint=h, res='f32', misalign=mis)
    for a in ('planes', 'f32'):                                     # 3 x 3 convolutions
        for n in (32, 64, 128, 300):
            g(N=n, conv=[32, 16, 16], a=a)
    g(N=256, conv=[32, 512, 512])                                   # 1024 blocks of 256 x 256
    g(N=256, conv=[32, 512, 511])
    g(N=64, conv=[48, 16, 16], a='f32')
    for n, m in ((64, 300), (512, 65280), (512, 65536), (256, 130816), (256, 131072)):    # fp8-corrected product
        g(M=m, N=n, K=128, f8=1)
    for h in (1, 14, 17, 18):
        g(M=300, N=300, K=128, f8=1, hint=h)
    g(N=128, conv=[32, 16, 16], f8=1)
    for n in (40, 100, 300):                                        # every hint, plain and convolution
        for h in HINTS:
            g(N=n, hint=h)
            g(N=n, hint=h, conv=[32, 16, 16])
    for h in (33, 39, 41, 168, 199, 202, 216, 217, 17 | 4 << 8, 200 | 2 << 16, 201 | 2 << 16):
        g(M=4096, N=2048, K=128, hint=h)
    g(M=0, out_rows=16)                                             # nothing to launch
    g(M=0, out_rows=16, a='f32')
    g(N=64, conv=[32, 16, 16], set=dict(M=0, conv_C=48))
    # ConvTranspose2d(k = 2, s = 2): pair form, one-weight form, hyper-network and LayerNorm epilogues, and their refusals
    ct = dict(kind='convt', M=1024, K=64, W=32)
    rows.append(dict(ct, N=64, dy=0, out='f32'))
    rows.append(dict(ct, N=64, dy=1, out='f32', a='f32'))
    rows.append(dict(ct, N=64, dy=0, out='planes'))
    rows.append(dict(ct, N=256, dy=-1, out='planes'))
    rows.append(dict(ct, N=64, dy=0, out='hyper'))
    rows.append(dict(ct, N=128, dy=-1, out='hyper'))
    rows.append(dict(ct, N=256, dy=-1, out='ln'))
    rows.append(dict(ct, N=256, dy=-1, out='planes', a='f32'))      # the one-weight form needs A planes
    rows.append(dict(ct, N=64, dy=0, out='f32', set=dict(res='buf', ldr=64)))
    rows.append(dict(ct, N=64, dy=-1, out='planes'))
    rows.append(dict(ct, N=32, dy=0, out='planes'))
    rows.append(dict(ct, N=64, dy=0, out='hyper', set=dict(hd_hyper=0)))
    rows.append(dict(ct, N=64, dy=0, out='hyper', set=dict(hd_rows=0)))
    rows.append(dict(ct, N=128, dy=0, out='hyper'))
    rows.append(dict(ct, N=64, dy=0, out='hyper', set=dict(C='buf')))
    rows.append(dict(ct, N=256, dy=-1, out='ln', set=dict(ln_beta=0)))
    rows.append(dict(ct, N=128, dy=-1, out='ln'))
    # what rsp_gemm refuses of a plain descriptor
    g(res='planes', set=dict(res_lo=0))
    g(out='both', c_ncols=30, pl_col0=32)
    g(set=dict(K=48))
    g(set=dict(N=0))
    g(set=dict(a_rows=0))
    g(set=dict(a_scale_log2=0x200))
    g(set=dict(Blo=0))
    g(set=dict(C=0))
    g(res='f32', set=dict(ldr=0))
    g(N=64, K=32, a='f32', set=dict(lda=30))
    g(N=64, K=32, a='f32', set=dict(a_scale_log2=0x102))
    g(N=64, K=32, a='f32', set=dict(c_ncols=32))
    g(N=64, conv=[32, 16, 16], set=dict(a_rowmap='buf'))
    g(N=64, conv=[32, 16, 16], set=dict(K=256))
    return rows


def label(r):
    return ' '.join(f'{k}={json.dumps(v, separators=(",", ":"))}' for k, v in r.items())


def walk(path, dry=False):
    import ctypes
    import torch
    from rsprompter_amd import _lib, ops
    dev = torch.device('cpu' if dry else 'cuda:0')
    if dry:                     # descriptors only, on host tensors: nothing is launched and every row counts as returned
        ops._stream, ops._chk_f32, ops._is_device, torch.cuda.synchronize = (lambda: 0), (lambda t, n: None), (lambda t: True), (lambda: None)
    real = _lib.load()
    rsp_gemm = real.rsp_gemm
    buf = torch.zeros(1 << 20, dtype=torch.float32, device=dev)      # what a `set` pointer names; no refused call reads it
    state = {}

    def spy(d, stream):
        for k, v in state['row'].get('set', {}).items():
            setattr(d, k, buf.data_ptr() if v == 'buf' else v)
        rec = {}
        for name, t in d._fields_:
            v = getattr(d, name)
            if t is ctypes.c_void_p:
                if v:
                    rec[name] = 'ptr' if v % 16 == 0 else f'ptr+{v % 16}'
            elif v:
                rec[name] = v
        state['desc'] = rec
        return 0 if dry else rsp_gemm(d, stream)
    real.rsp_gemm = spy

    class W:                    # a PackedWeight of zeros
        def __init__(self, n, k, f8):
            self.N, self.K, self.scale_log2, self.f8, self.bias = n, k, 0, bool(f8), torch.zeros(n + 8, device=dev)[4:]
            self.hi = torch.zeros((k // 32, n, 32), dtype=torch.float16, device=dev)
            self.lo = torch.zeros_like(self.hi)

    def planes(shape, f8=False):
        p = ops.empty_planes(shape, dev, f8=f8)
        p.hi.zero_(), p.lo.zero_()
        return p

    def f32(rows, cols, off=0):
        return torch.zeros(rows * cols + 4, device=dev)[off:off + rows * cols].view(rows, cols)

    def run(r):
        mis = r.get('misalign')
        if r['kind'] == 'convt':
            m, n, k = r['M'], r['N'], r['K']
            a = planes((m, k)) if r.get('a', 'planes') == 'planes' else f32(m, k)
            w = W(n, k, False)
            out, kw = None, {}
            cout = n // (2 if r['dy'] >= 0 else 4)
            if r['out'] == 'f32':
                out = f32(2 * m, n)                             # the output [2H, 2W, Cout] seen as [2H * W, 2 Cout]
            elif r['out'] in ('planes', 'ln'):                  # ... and as planes [4 H W, Cout] (a refused Cout: rounded up)
                kw = dict(planes_out=planes((4 * m, (cout + 31) // 32 * 32)), c_rows=4 * m)
                if r['out'] == 'ln':
                    kw['ln'] = (torch.zeros(64, device=dev), torch.zeros(64, device=dev), 1e-6)
            else:
                kw = dict(hyper=torch.zeros((1, 32), device=dev), hd_out=f32(4 * m, 1), hd_rows=m)
            return ops._gemm_ct(a, w, out, w.bias[:n], 0, r['W'], r['dy'], 2, **kw)
        f8 = bool(r.get('f8'))
        if 'conv' in r:
            c, h, wd = r['conv']
            m, k = h * wd, 9 * c
            a = planes((1, h, wd, c), f8) if r.get('a', 'planes') == 'planes' else torch.zeros((1, h, wd, c), device=dev)
            kw = dict(conv=(3, 1, 1))
        else:
            m, k = r['M'], r['K']
            rows_a = max(m, 16)
            a = planes((rows_a, k), f8) if r.get('a', 'planes') == 'planes' else f32(rows_a, k)
            kw = dict(M=m)
        n = r['N']
        w = W(n, k, f8)
        rows = r.get('out_rows', m)
        kw.update(dma=False, tile_hint=r['hint'], act=r.get('act', 0), bias=w.bias[1:1 + n] if mis == 'bias' else w.bias[:n])
        if 'out_rows' in r:
            kw['out_rows'] = rows
        if r.get('res') == 'f32':
            kw['res'] = f32(rows, n, 1 if mis == 'res' else 0)
        elif r.get('res') == 'planes':
            kw['res'] = planes((rows, n))
        if r.get('res_bmap'):
            kw.update(res_bmap=torch.zeros(rows // 256 + 1, dtype=torch.int32, device=dev), res_brows=256)
        if r.get('c_rowmap'):
            kw['c_rowmap'] = torch.arange(m, dtype=torch.int32, device=dev)
        o = r.get('out', 'f32')
        if o != 'f32':
            kw.update(out_planes=True, out_f32=o == 'both', out_f8=bool(r.get('out_f8')),
                      c_ncols=r.get('c_ncols', 0), pl_col0=r.get('pl_col0', 0))
        if o != 'planes':
            kw['out'] = f32(rows, r.get('c_ncols') or n, 1 if mis == 'C' else 0)
        return ops.gemm(a, w, **kw)

    done = []
    try:
        for r in grid():
            state.update(row=r, desc=None)
            try:
                run(r)
                torch.cuda.synchronize()
                outcome = 'returned'
            except RuntimeError as e:
                if 'librsp_hip: rsp_gemm' not in str(e):            # a device error: nothing more runs on this GPU
                    raise
                outcome = 'RuntimeError'
            if state['desc'] is None:
                raise SystemExit(f'row never reached rsp_gemm: {label(r)}')
            done.append(dict(call=label(r), desc=state['desc'], outcome=outcome))
    finally:
        with open(path, 'w') as f:
            json.dump(done, f, indent=0)
    print(f'{len(done)} rows, {sum(d["outcome"] == "returned" for d in done)} returned')


def join(rows_path, trace_path, golden):
    rows = json.load(open(rows_path))
    with open(trace_path) as f:
        ks = [k for k in csv.DictReader(f) if 'gemm_f16' in k['Kernel_Name']]
    if len({(k['Stream_Id'], k['Queue_Id']) for k in ks}) > 1:
        raise SystemExit('the GEMM kernels ran on more than one stream')
    ks.sort(key=lambda k: int(k['Start_Timestamp']))
    names = [re.search(r'gemm_f16\w+<[^>]*>', k['Kernel_Name']).group(0) for k in ks]
    launched = [r for r in rows if r['outcome'] == 'returned' and r['desc'].get('M')]
    if len(launched) != len(names):
        raise SystemExit(f'{len(launched)} rows returned with M > 0, but the trace holds {len(names)} GEMM kernels')
    it = iter(names)
    def compact(desc):          # pointers as one list "Bhi Blo C+4 ..." (name, + offset from 16 bytes); alpha is no input of the plan
        ptrs = ' '.join(k + v[3:] for k, v in desc.items() if isinstance(v, str))
        return dict({'ptrs': ptrs}, **{k: v for k, v in desc.items() if not isinstance(v, str) and k != 'alpha'})
    out = [dict(call=r['call'], desc=compact(r['desc']),
                kernel='EINVAL' if r['outcome'] != 'returned' else (next(it) if r['desc'].get('M') else 'none')) for r in rows]
    with open(golden, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(o, separators=(',', ':')) for o in out) + '\n]\n')
    print(f'{len(out)} rows -> {golden}: {len(names)} launches, {sum(o["kernel"] == "EINVAL" for o in out)} EINVAL')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', help='walk the grid on the GPU and write the row list here')
    ap.add_argument('--join', nargs=2, metavar=('ROWS', 'KERNEL_TRACE_CSV'))
    ap.add_argument('--golden', default=os.path.join(ROOT, 'tests', 'golden', 'gemm_plan.json'))
    ap.add_argument('--list', action='store_true')
    ap.add_argument('--dry', action='store_true', help='with --rows: build the descriptors on the host, launch nothing')
    a = ap.parse_args()
    if a.list:
        for r in grid():
            print(label(r))
    if a.rows:
        walk(a.rows, a.dry)
    if a.join:
        join(a.join[0], a.join[1], a.golden)
