"""CPU: the C-ABI shared library loads without a GPU and exports every entry point that
include/rsp_hip.h declares (no compute calls); argument validation paths return RSP_EINVAL."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, 'include', 'rsp_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(rsp_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    from rsprompter_amd import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/rsp_hip.h but not exported'
    assert set(_lib.PROTOTYPES) <= set(names)
    assert lib.rsp_abi_version() == 6
    assert b'gfx950' in lib.rsp_build_info()


def test_argument_validation_without_gpu():
    from rsprompter_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    assert lib.rsp_gemm(None, None) == EINVAL
    d = _lib.RspGemmDesc()
    assert lib.rsp_gemm(ctypes.byref(d), None) == EINVAL          # null operands
    assert lib.rsp_layernorm(None, None, None, None, 4, 64, 1e-6, 0, None) == EINVAL
    assert lib.rsp_roi_align(None, None) == EINVAL
    assert lib.rsp_attention(None, None) == EINVAL
    assert lib.rsp_pack_bits(None, None, 64, None) == EINVAL
    assert lib.rsp_nms_workspace_bytes(2, 5000) > 2 * 5000 * 79 * 8


def test_ctypes_struct_layout_matches_the_c_compiler():
    """Every descriptor structure that _lib derives from the header has the size and the field offsets the host C compiler
    gives the header's own declaration (field order is implied by the offsets): a stand-alone C program prints them."""
    import shutil
    import subprocess
    import tempfile
    from rsprompter_amd import _lib
    cc = '/opt/rocm/lib/llvm/bin/clang'
    cc = cc if os.path.exists(cc) else shutil.which('cc')
    if not cc:
        pytest.skip('no host C compiler')
    assert len(_lib.STRUCTS) == 9
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rsp_hip.h"', 'int main(void) {']
    for name, cls in _lib.STRUCTS.items():
        lines.append(f'  printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name} {f[0]} %zu\\n", offsetof({name}, {f[0]}));' for f in cls._fields_]
    lines += ['  return 0;', '}']
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, 'layout.c'), 'w').write('\n'.join(lines) + '\n')
        subprocess.check_call([cc, '-std=c99', '-I', os.path.join(ROOT, 'include'), os.path.join(tmp, 'layout.c'),
                               '-o', os.path.join(tmp, 'layout')])
        out = subprocess.run([os.path.join(tmp, 'layout')], capture_output=True, text=True, check=True).stdout
    want = [ln.split() for ln in out.splitlines()]
    got = []
    for name, cls in _lib.STRUCTS.items():
        got.append([name, 'sizeof', str(ctypes.sizeof(cls))])
        got += [[name, f[0], str(getattr(cls, f[0]).offset)] for f in cls._fields_]
    assert got == want
    assert ctypes.sizeof(_lib.RspGemmDesc) == 288 and _lib.RspRpnDesc.coder.offset == 128


SYNTHETIC_HEADER = r'''
/* every construct of the subset once; rsp_in_a_comment( and // in a comment are not code */
#ifndef SYNTH_H_
#define SYNTH_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define RSP_SEVEN 7
#define RSP_MINUS (-2)   /* why */
#define RSP_HEX 0x100
#define RSP_SUFFIX 5u
#define RSP_EXPR ((1LL << 40) - 3 * 2 + 0x7fffffffLL / 6)
#define RSP_LOW8(w) ((w) & 0xff)
#define RSP_TWO_LINES(w) \
  (RSP_LOW8(w) + rsp_in_a_macro(w))
typedef void* rsp_stream_t;
typedef struct RspInner { float m[4], s; int32_t flag; } RspInner;
typedef struct RspOuter {
  const float* A;          /* a comment */
  const uint16_t* hi; const uint16_t* lo;
  int32_t M, N, K;
  const float *g, *b;
  const float* level[3];
  int64_t stride; double d; int i;
  RspInner inner;
  const RspInner* ip;
} RspOuter;
typedef struct {
  int64_t a;
  int32_t b, pad;
} RspAnon;
int rsp_version(void);
const char* rsp_info(void);
int64_t rsp_bytes(int32_t n, int64_t m);
int rsp_run(const RspOuter* d, const RspAnon* units, const float* x,
            uint8_t* out, float eps, double lr, const int32_t hw[2], int32_t,
            const float* f4 /*host*/, void* ws, rsp_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif /* SYNTH_H_ */
'''


def test_header_parser_on_a_synthetic_header():
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_void_p
    from rsprompter_amd._lib import parse_header
    structs, protos, const = parse_header(SYNTHETIC_HEADER)
    assert const == dict(RSP_SEVEN=7, RSP_MINUS=-2, RSP_HEX=256, RSP_SUFFIX=5, RSP_EXPR=2 ** 40 - 6 + (2 ** 31 - 1) // 6)
    assert list(structs) == ['RspInner', 'RspOuter', 'RspAnon']
    inner, outer, anon = structs.values()
    assert all(issubclass(s, ctypes.Structure) and s.__name__ == n for n, s in structs.items())
    assert inner._fields_ == [('m', c_float * 4), ('s', c_float), ('flag', c_int)]
    assert outer._fields_ == [('A', c_void_p), ('hi', c_void_p), ('lo', c_void_p), ('M', c_int), ('N', c_int), ('K', c_int),
                              ('g', c_void_p), ('b', c_void_p), ('level', c_void_p * 3), ('stride', c_int64), ('d', c_double),
                              ('i', c_int), ('inner', inner), ('ip', POINTER(inner))]
    assert anon._fields_ == [('a', c_int64), ('b', c_int), ('pad', c_int)]
    assert protos == {
        'rsp_version': (c_int, []),
        'rsp_info': (c_char_p, []),
        'rsp_bytes': (c_int64, [c_int, c_int64]),
        'rsp_run': (c_int, [POINTER(outer), POINTER(anon), c_void_p, c_void_p, c_float, c_double, c_void_p, c_int, c_void_p,
                            c_void_p, c_void_p]),
    }


@pytest.mark.parametrize('bad, says', [
    ('typedef struct RspS { unsigned long n; } RspS;', 'struct field'),           # a declaration that does not parse
    ('typedef struct RspS { int32_t a; uint8_t flag; } RspS;', 'uint8_t'),          # a by-value type outside the map
    ('typedef struct RspS { int32_t a[N]; } RspS;', 'struct field'),
    ('int rsp_callback(void (*fn)(int), int32_t n);', 'rsp_callback'),                # a prototype the regex misses
    ('unsigned int rsp_count(int32_t n);', 'unsigned'),
    ('int rsp_twice(int32_t n);\nint rsp_twice(int32_t n);', 'rsp_twice'),
    ('int rsp_f(unsigned n);', 'unsigned'),
    ('struct RspTag { int32_t a; };', 'RspTag'),
    ('int rsp_f(int32_t n);  // a C++ comment', '//'),
    ('#define RSP_HALF 0.5f', 'RSP_HALF'),
    ('#define RSP_OTHER RSP_SEVEN', 'RSP_OTHER'),
])
def test_header_parser_fails_loudly(bad, says):
    from rsprompter_amd._lib import parse_header
    parse_header('typedef void* rsp_stream_t;\nint rsp_ok(int32_t n, rsp_stream_t s);\n')
    with pytest.raises(RuntimeError, match=re.escape(says)):
        parse_header('typedef void* rsp_stream_t;\n' + bad + '\n')


def test_binding_covers_the_header_and_the_library():
    """Whole header: the prototypes are exactly the declared entry points, every exported rsp_* symbol of the library has
    one, and nothing but the mapped ctypes types appears in them."""
    import subprocess
    from rsprompter_amd import _lib
    assert set(_lib.PROTOTYPES) == set(_declared()) and len(_lib.PROTOTYPES) >= 104
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm'
    out = subprocess.run([nm if os.path.exists(nm) else 'nm', '-D', '--defined-only', _lib.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r'\b[TW] (rsp_\w+)$', out, re.M))
    assert len(exported) >= 104 and exported <= set(_lib.PROTOTYPES), sorted(exported - set(_lib.PROTOTYPES))
    mapped = {ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p}
    mapped |= {ctypes.POINTER(s) for s in _lib.STRUCTS.values()}
    for name, (res, args) in _lib.PROTOTYPES.items():
        assert res in (ctypes.c_int, ctypes.c_int64, ctypes.c_char_p), name
        assert all(a in mapped for a in args), name
    for name, cls in _lib.STRUCTS.items():
        assert getattr(_lib, name) is cls
        for _, t in cls._fields_:
            t = t._type_ if hasattr(t, '_length_') else t
            assert t in mapped or t in _lib.STRUCTS.values(), name
    assert _lib.load().rsp_abi_version() == _lib.CONST['RSP_ABI_VERSION']


# ------------------------------------------------------------------------------------------------------------- limits
LIMITS = dict(ACT_NONE='RSP_ACT_NONE', ACT_RELU='RSP_ACT_RELU', ACT_GELU='RSP_ACT_GELU', ACT_SIGMOID='RSP_ACT_SIGMOID',
              ACT_RELU_POST='RSP_ACT_RELU_POST', PLANE_F8='RSP_PLANE_F8', SAM_T2I_MAX_TOKENS='RSP_SAM_T2I_MAX_TOKENS',
              SAM_I2T_MAX_TOKENS='RSP_SAM_I2T_MAX_TOKENS', SAM_I2T_FUSED_MAX_TOKENS='RSP_SAM_I2T_FUSED_MAX_TOKENS',
              SAM_T2I_FOLD_MAX_TOKENS='RSP_SAM_T2I_FOLD_MAX_TOKENS', NMS_LDS_CANDIDATES='RSP_NMS_LDS_CANDIDATES',
              NMS_MAX_CANDIDATES='RSP_NMS_MAX_CANDIDATES', MASK_POLYGON_MAX_PIECES='RSP_MASK_POLYGON_MAX_PIECES',
              RING_SIMPLIFY_MAX_SIDE='RSP_RING_SIMPLIFY_MAX_SIDE', RING_SIMPLIFY_MAX_TOL2_Q8='RSP_RING_SIMPLIFY_MAX_TOL2_Q8',
              MASK_OBB_MAX_SIDE='RSP_MASK_OBB_MAX_SIDE', MASK_OBB_MAX_BOUND='RSP_MASK_OBB_MAX_BOUND',
              CROP_TABLE_COLS='RSP_CROP_TABLE_COLS', COCO_IOU_BBOX='RSP_COCO_IOU_BBOX', COCO_IOU_SEGM='RSP_COCO_IOU_SEGM')


def test_python_limits_are_the_header_macros():
    from rsprompter_amd import _lib, large_image, ops
    C = _lib.CONST
    for py, macro in LIMITS.items():
        assert getattr(ops, py) == C[macro] and type(getattr(ops, py)) is int, py
    assert ops.MASK_REGION_TILE == (C['RSP_MASK_REGION_TILE_H'], C['RSP_MASK_REGION_TILE_W'])
    assert large_image.MAX_PATCH_WIDTH == C['RSP_RLE_MAX_WIDTH']
    assert ops.COCO_UNIT_BYTES == ctypes.sizeof(_lib.RspCocoUnit) == 40
    assert (C['RSP_OK'], C['RSP_EINVAL'], C['RSP_ELAUNCH']) == (0, -1, -2)
    # the two limits that bound no argument but a workspace: no device work
    lib = _lib.load()
    lds, piece_max, bound_max = C['RSP_NMS_LDS_CANDIDATES'], C['RSP_MASK_POLYGON_MAX_PIECES'], C['RSP_MASK_OBB_MAX_BOUND']
    def sort_keys(cap):     # what the workspace holds beyond boxes, order and removal words per candidate and the 256 spare bytes
        return lib.rsp_nms_workspace_bytes(1, cap) - cap * (4 * 4 + 4 + 8 * ((cap + 63) // 64)) - 256
    assert sort_keys(lds) == 0 and sort_keys(lds + 1) == 8 * 2 * lds      # in memory above the limit: the next power of two
    assert lib.rsp_mask_polygon_rank_workspace_bytes(piece_max) > 0 == lib.rsp_mask_polygon_rank_workspace_bytes(piece_max + 1)
    assert lib.rsp_mask_hull_workspace_bytes(bound_max) > 0 == lib.rsp_mask_hull_workspace_bytes(bound_max + 1)


@pytest.fixture(scope='module')
def emu_lib():
    if not os.path.exists(os.environ.get('EMU_CXX', '/opt/rocm/lib/llvm/bin/clang++')):
        pytest.skip('no host clang++ for the emulated build')
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'wave_emu'))
    import harness
    with harness.emulated_ops() as ops:
        yield ops._lib.load()


def test_shipped_library_has_no_ablation_kernels():
    """The persistent GEMM (csrc/gemm_s2.hip) is instantiated once per product epilogue form and for nothing else: the
    ablation variants (VAR != 0: no DMA, no epilogue, cache-hot sources -- wrong results on purpose) exist only in a
    development build (RSP_DEV_BUILD=1), and no tools-only entry point is exported."""
    import subprocess
    from rsprompter_amd import _lib
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm'
    out = subprocess.run([nm if os.path.exists(nm) else 'nm', '-C', _lib.LIB_PATH], capture_output=True, text=True).stdout
    inst = set(re.findall(r'gemm_f16x3_s2_kernel<(\d+), (\d+)>', out))
    assert inst, 'gemm_f16x3_s2_kernel not found in the library'
    assert {v for v, _ in inst} == {'0'}, sorted(inst)
    want = {4, 5, 21, 12, 28, 8, 10, 6, 64}       # E_C, +RES, +RES+RMAP, C+PL, C+PL+RMAP, PL, PL+GELU, C+GELU, run-time
    assert {int(e) for _, e in inst} == want, sorted(inst)
    assert 'rsp_debug_s2_trace' not in out
    # gemm_f16x3_dma_kernel<BM, BN, WGM, WGN, NBUF, ABL, ...>: ABL (6th argument) != 0 are the no-DMA / no-MFMA ablations
    abl = set(re.findall(r'gemm_f16x3_dma_kernel<\d+, \d+, \d+, \d+, \d+, (\d+),', out))
    assert abl == {'0'}, abl
    lib = _lib.load()
    d = _lib.RspGemmDesc()
    assert lib.rsp_gemm_s2_epilogue(None) == -1 and lib.rsp_gemm_s2_epilogue(ctypes.byref(d)) == -1


def test_product_code_creates_no_streams():
    """Round 5's lesson: a HIGH-priority stream anywhere in the process made every kernel launch ~75 us
    slower on this stack, and torch's pooled default-priority streams can be the very stream a caller obtains later.  The
    package therefore launches on the caller's current stream only; `bench.py` owns the one side stream of the exchange."""
    import glob
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'rsprompter_amd')
    for f in glob.glob(os.path.join(root, '*.py')):
        src = open(f).read()
        assert not re.search(r'cuda\.Stream\(|ExternalStream\(|priority\s*=', src), f


def _p(t):
    return t.data_ptr()


def test_every_limit_refuses_one_past_it_on_the_emulator(emu_lib):
    """One entry point per family of limits, run lane by lane on the emulator with tiny valid arguments: RSP_EINVAL one past
    the limit, RSP_OK at it.  Where the smallest legal call AT the limit is large (131 072 NMS candidates, 2^31 / 6 polygon
    pieces, 2^30 hull records) the accepted call keeps every other argument and takes a small value instead, so the refusal
    can only come from the limit; the coordinate bounds of the ring and hull entry points cost nothing at the limit."""
    import torch
    from rsprompter_amd import _lib
    lib, C = emu_lib, _lib.CONST
    OK, EINVAL = C['RSP_OK'], C['RSP_EINVAL']
    f32, i32, i64, u8 = torch.float32, torch.int32, torch.int64, torch.uint8
    N = 32

    def zeros(*shape, dtype=f32):
        return torch.zeros(shape, dtype=dtype)

    # token -> image attention, R = 1, N = 32
    lim = C['RSP_SAM_T2I_MAX_TOKENS']
    q, kv, out = torch.randn(1, lim + 1, 128), torch.randn(N, 256), zeros(1, lim + 1, 128)
    assert lib.rsp_sam_t2i_attention(_p(q), _p(kv), None, _p(out), 1, lim + 1, N, 0.25, None) == EINVAL
    assert lib.rsp_sam_t2i_attention(_p(q), _p(kv), None, _p(out), 1, lim, N, 0.25, None) == OK
    assert out[0, :lim].abs().sum() > 0 and torch.isfinite(out).all()
    # image -> token attention
    lim = C['RSP_SAM_I2T_MAX_TOKENS']
    q, k, v, out = torch.randn(N, 128), torch.randn(1, lim + 1, 128), torch.randn(1, lim + 1, 128), zeros(N, 128)
    assert lib.rsp_sam_i2t_attention(_p(q), None, _p(k), _p(v), _p(out), None, None, 0, 1, lim + 1, N, 0.25, None) == EINVAL
    assert lib.rsp_sam_i2t_attention(_p(q), None, _p(k), _p(v), _p(out), None, None, 0, 1, lim, N, 0.25, None) == OK
    assert out.abs().sum() > 0 and torch.isfinite(out).all()
    # ... fused with out_proj, the residual and the LayerNorm
    lim = C['RSP_SAM_I2T_FUSED_MAX_TOKENS']
    t = dict(q=q, k=k, v=v, wo=torch.randn(256, 128), bo=zeros(256), res=torch.randn(N, 256), gamma=torch.ones(256),
             beta=zeros(256), out=zeros(N, 256))
    d = _lib.RspI2tFusedDesc(**{n: _p(x) for n, x in t.items()}, eps=1e-6, R=1, T=lim + 1, N=N, scale=0.25)
    assert lib.rsp_sam_i2t_fused(ctypes.byref(d), None) == EINVAL
    d.T = lim
    assert lib.rsp_sam_i2t_fused(ctypes.byref(d), None) == OK
    assert t['out'].abs().sum() > 0 and torch.isfinite(t['out']).all()
    # the folded token -> image attention: its expand step
    lim = C['RSP_SAM_T2I_FOLD_MAX_TOKENS']
    tq, hi, lo = torch.randn(lim + 1, 128), zeros(96, 128, dtype=torch.int16), zeros(96, 128, dtype=torch.int16)
    assert lib.rsp_sam_fold_expand(_p(tq), _p(hi), _p(lo), 0, 1, lim + 1, 0.25, None) == EINVAL
    assert lib.rsp_sam_fold_expand(_p(tq), _p(hi), _p(lo), 0, 1, lim, 0.25, None) == OK
    assert hi.ne(0).any()
    # run-length encoding: one mask of one row
    lim = C['RSP_RLE_MAX_WIDTH']
    mask, ws, counts, n = zeros(1, 1, lim + 1, dtype=u8), zeros(8, dtype=i32), zeros(1, 8, dtype=i32), zeros(1, dtype=i32)
    mask[0, 0, 3:5] = 1
    assert lib.rsp_mask_rle(_p(mask), 1, 1, lim + 1, _p(ws), _p(counts), _p(n), 8, None) == EINVAL
    assert lib.rsp_mask_rle(_p(mask), 1, 1, lim, _p(ws), _p(counts), _p(n), 8, None) == OK
    assert n.tolist() == [3] and counts[0, :3].tolist() == [3, 2, lim - 5]
    # NMS: the accepted call has 4 candidates a row instead of the 131 072 of the limit
    lim = C['RSP_NMS_MAX_CANDIDATES']
    boxes = torch.tensor([[0., 0., 10., 10.], [1., 1., 10., 10.], [20., 20., 30., 30.], [0., 0., 0., 0.]])
    scores, ids, cnt = torch.tensor([.9, .8, .7, 0.]), zeros(4, dtype=i32), torch.tensor([3], dtype=i32)
    ws = zeros(lib.rsp_nms_workspace_bytes(1, 4), dtype=u8)
    keep, kc, ob, osc, oid = zeros(4, dtype=i32), zeros(1, dtype=i32), zeros(4, 4), zeros(4), zeros(4, dtype=i32)

    def nms(cap):
        return lib.rsp_batched_nms(_p(boxes), _p(scores), _p(ids), None, _p(cnt), 1, cap, 0.5, 4, _p(ws), _p(keep), _p(kc),
                                   _p(ob), _p(osc), _p(oid), None, None)
    assert nms(lim + 1) == EINVAL and nms(4) == OK and kc.tolist() == [2]
    # polygon export: a call without instances touches no array, so it is legal at the limit itself
    lim = C['RSP_MASK_POLYGON_MAX_PIECES']
    counts, n, offs = torch.tensor([[0, 1, 3]], dtype=i32), torch.tensor([3], dtype=i32), zeros(2, dtype=i64)
    pieces, ekey, eoth, succ = zeros(4, dtype=i32), zeros(6, dtype=i64), zeros(6, dtype=i32), zeros(6, dtype=i32)

    def edges(P):
        return lib.rsp_mask_polygon_edges(0, 2, 2, _p(offs), P, _p(pieces), _p(ekey), _p(eoth), _p(succ), None)
    assert edges(lim + 1) == EINVAL and edges(lim) == OK
    # polygon simplification: one square ring; both bounds are bounds on values, the call at the limit is as small
    side, tol = C['RSP_RING_SIMPLIFY_MAX_SIDE'], C['RSP_RING_SIMPLIFY_MAX_TOL2_Q8']
    verts = torch.tensor([[0, 0], [side, 0], [side, side], [0, side]], dtype=i32)
    offs = torch.tensor([0, 4], dtype=i64)
    keep, pos, kept, area2, rounds = zeros(4, dtype=u8), zeros(4, dtype=i32), zeros(1, dtype=i32), zeros(1, dtype=i64), zeros(1, dtype=i32)

    def mark(t2, H, W):
        return lib.rsp_ring_simplify_mark(_p(verts), _p(offs), 1, 4, t2, H, W, 0, _p(keep), _p(pos), _p(kept), _p(area2), _p(rounds), None)
    assert mark(tol + 1, side, side) == EINVAL and mark(tol, side + 1, side) == EINVAL and mark(tol, side, side + 1) == EINVAL
    assert mark(tol, side, side) == OK
    assert kept.tolist() == [4] and abs(int(area2[0])) == 2 * side * side
    # oriented boxes: one mask of one row whose last pixel is set
    side, bound = C['RSP_MASK_OBB_MAX_SIDE'], C['RSP_MASK_OBB_MAX_BOUND']
    counts, n = torch.tensor([[side - 1, 1]], dtype=i32), torch.tensor([2], dtype=i32)
    offs = torch.tensor([0, 3], dtype=i64)
    ws, cc, rounds = zeros(lib.rsp_mask_hull_workspace_bytes(3), dtype=u8), zeros(2, 1, dtype=i32), zeros(2, 1, dtype=i32)

    def chains(W, B):
        return lib.rsp_mask_hull_chains(_p(counts), _p(n), 1, 2, 1, W, _p(offs), B, _p(ws), _p(cc), _p(rounds), None)
    assert chains(side + 1, 3) == EINVAL and chains(side, bound + 1) == EINVAL
    assert chains(side, 3) == OK and cc.tolist() == [[2], [2]]
