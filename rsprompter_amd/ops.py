"""Thin Python wrappers: torch tensors (device memory + stream plumbing only)
-> C-ABI calls into librsp_hip.so.  No arithmetic happens in torch here.
"""
import collections
import ctypes
import math
import os

import torch

from . import _lib as _lib_real

CONST = _lib_real.CONST     # the integer macros of include/rsp_hip.h: flags and limits of the C ABI are stated there only
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SIGMOID, ACT_RELU_POST = (
    CONST['RSP_ACT_' + a] for a in ('NONE', 'RELU', 'GELU', 'SIGMOID', 'RELU_POST'))
# Power-of-two pre-scale of activation planes (x * 2^e is what gets split into fp16 hi + lo).  e = 2 keeps |x| < 16376
# exactly representable (the split saturates beyond, rsp_common.h) -- headroom for the outlier activations of real SAM
# checkpoints (MLP hidden layer, residual stream) and for the RSFeatureAggregator's running sum over 16 layers, which
# passed 1023 (the old e = 6 limit) on the ViT-H fixture and turned whole rows into NaN.  The price is that `lo` goes
# subnormal for |x| < 0.03: an absolute error floor of 7.5e-9 per element, invisible next to the 1e-5 fp32 noise floor.
DEFAULT_A_SCALE_LOG2 = 2
DEBUG_FINITE = bool(int(__import__('os').environ.get('RSP_DEBUG_FINITE', '0')))


class Profiler:
    """Per-kernel HIP-event timing on the launch stream (bench.py's roofline leg; off by default)."""

    def __init__(self):
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, flops, nbytes, e0, e1 in self.records:
            a = agg.setdefault(name, dict(ms=0.0, calls=0, flops=0.0, bytes=0.0))
            a['ms'] += e0.elapsed_time(e1)
            a['calls'] += 1
            a['flops'] += flops
            a['bytes'] += nbytes
        return agg


_prof = None


def set_profiler(p):
    global _prof
    _prof = p


_timed_depth = 0


def _timed(name, flops, nbytes, fn, detail=None):
    global _timed_depth
    if _prof is None:
        return fn()
    if detail is not None and getattr(_prof, 'shapes', False):
        name = f'{name} {detail}'
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    _timed_depth += 1
    try:
        r = fn()
    finally:
        _timed_depth -= 1
    e1.record()
    _prof.records.append((name, float(flops), float(nbytes), e0, e1))
    return r


class _ProfiledLib:
    """librsp_hip.so as seen by this module: with a profiler installed every entry point that is not already inside
    an annotated `_timed` region is bracketed by HIP events under its own symbol name, so that the per-step kernel
    table of bench.py accounts for ALL native calls, not only the ones carrying a FLOP/byte model."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if _prof is None or _timed_depth > 0 or not name.startswith('rsp_'):
            return f

        def call(*a):
            return _timed(name, 0, 0, lambda: f(*a))
        return call


class _LibModule:
    """Stand-in for the `_lib` module inside ops.py (same attributes; `load()` returns the profiled view)."""

    def __getattr__(self, name):
        return getattr(_lib_real, name)

    @staticmethod
    def load():
        return _ProfiledLib(_lib_real.load())


_lib = _LibModule()


def require_device(dev):
    if torch.device(dev).type != 'cuda':
        raise RuntimeError('rsprompter_amd runs on the HIP device only (there is no CPU fallback); '
                           'move the model with .to("cuda")')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _is_device(t):
    return t.is_cuda


def _chk_f32(t, name):
    if t.dtype != torch.float32 or not _is_device(t):
        raise ValueError(f"{name}: expected a float32 CUDA/HIP tensor, got {t.dtype} on {t.device}")


class PackedWeight:
    """A GEMM weight [N, K] pre-split into fp16 hi/lo planes on the device.

    `scale_log2` is the power-of-two applied before the split so that the
    largest |w| lands near 2^14 (well inside fp16 range, lo plane normal).
    """

    def __init__(self, w, bias=None, device=None, f8=False):
        """f8=True: the second plane is the cat8 plane of the fp8-corrected product (plane format word, rsp_hip.h)."""
        w = w.detach().to(torch.float32)
        if w.dim() != 2:
            raise ValueError("PackedWeight expects a 2-D [N, K] matrix")
        self.f8 = bool(f8)
        device = device or w.device
        n, k = w.shape
        kpad = (k + 31) // 32 * 32
        if kpad != k:
            w = torch.nn.functional.pad(w, (0, kpad - k))
        amax = float(w.abs().max()) if w.numel() else 0.0
        if amax > 0 and math.isfinite(amax):
            e = int(math.floor(math.log2(16384.0 / amax)))
            e = max(-20, min(24, e))
        else:
            e = 0
        wd = w.contiguous().to(device)
        self.N, self.K = n, kpad
        self.scale_log2 = e
        # KB32 layout [K/32][N][32]: every 32-wide K slice of the weight is one contiguous run
        self.hi = torch.empty((kpad // 32, n, 32), dtype=torch.float16, device=device)
        self.lo = torch.empty((kpad // 32, n, 32), dtype=torch.float16, device=device)
        lib = _lib.load()
        _lib.check(lib.rsp_split_f16_kb32(wd.data_ptr(), self.hi.data_ptr(), self.lo.data_ptr(),
                                          n, kpad, plane_word(e, self.f8), _stream()), "rsp_split_f16_kb32")
        self.bias = None if bias is None else bias.detach().to(torch.float32).contiguous().to(device)


PLANE_F8 = CONST['RSP_PLANE_F8']        # include/rsp_hip.h "Plane format word"
# Opt-in fast mode (RSP_F8CORR=1, or set ops.F8_CORR before the model is built / first run): the four big GEMMs of every
# encoder block run fp16 hi.hi + ONE fp8 MFMA carrying both correction terms (2 units of matrix time instead of 3).
# Measured: GEMMs 1.15-1.25x faster, image embeddings 1.0-1.4e-4 instead of 1.2-1.6e-5 off the fp32
# reference -- inside the 1e-3 budget, but the masked query decoder then flips 10 instead of 4 attention-mask decisions
# on the ViT-H + LoRA fixture, so the default stays the three-pass fp16x3 product.
# RSP_F8CORR=mlp (round 6 study): only lin1 / lin2 of every block.
F8_CORR = {'0': False, '': False, '1': True, 'all': True, 'mlp': 'mlp'}[os.environ.get('RSP_F8CORR', '0')]


def plane_word(scale_log2, f8=False):
    return (int(scale_log2) & 0xff) | (PLANE_F8 if f8 else 0)


class Planes:
    """An fp32 matrix x [rows, K] held as two fp16 tensors hi = f16(x * 2^e), lo = f16(x * 2^e - hi) in the
    K-blocked "KB32" layout [K/32][rows][32].  Same bytes as fp32; lets the GEMM stream its A operand
    HBM -> LDS with the DMA engine in contiguous 1-KiB bursts.  `shape` is the LOGICAL shape
    (leading dims are free to re-factor: rows = prod(shape[:-1])).
    f8=True: `lo` holds the cat8 plane [e4m3(lo) x 32 | e4m3(hi) x 32] of the fp8-corrected product instead (same
    bytes); such planes feed GEMMs whose weight was packed with f8=True and nothing else."""

    def __init__(self, hi, lo, shape, scale_log2=DEFAULT_A_SCALE_LOG2, f8=False):
        self.hi, self.lo, self.shape, self.scale_log2, self.f8 = hi, lo, tuple(shape), scale_log2, bool(f8)

    @property
    def word(self):
        return plane_word(self.scale_log2, self.f8)

    @property
    def device(self):
        return self.hi.device

    @property
    def rows(self):
        return self.hi.shape[1]

    def view(self, *shape):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else tuple(shape)
        n = 1
        for v in shape[:-1]:
            n *= v
        if shape[-1] != self.shape[-1] or n != self.rows:
            raise ValueError(f'cannot view planes {self.shape} as {shape}')
        return Planes(self.hi, self.lo, shape, self.scale_log2, self.f8)

    reshape = view


def empty_planes(shape, device, scale_log2=DEFAULT_A_SCALE_LOG2, f8=False):
    shape = tuple(shape)
    K = shape[-1]
    if K % 32:
        raise ValueError('planes need K % 32 == 0')
    rows = 1
    for v in shape[:-1]:
        rows *= v
    return Planes(torch.empty((K // 32, rows, 32), dtype=torch.float16, device=device),
                  torch.empty((K // 32, rows, 32), dtype=torch.float16, device=device), shape, scale_log2, f8)


def to_planes(x, scale_log2=DEFAULT_A_SCALE_LOG2, f8=False):
    """fp32 tensor -> Planes (one extra HBM pass; producers that can emit planes directly avoid it)."""
    lib = _lib.load()
    _chk_f32(x, "x")
    x = x if x.is_contiguous() else x.contiguous()
    p = empty_planes(x.shape, x.device, scale_log2, f8)
    _timed('split_f16_kernel', 0, 8.0 * x.numel(),
           lambda: _lib.check(lib.rsp_split_f16_kb32(x.data_ptr(), p.hi.data_ptr(), p.lo.data_ptr(), p.rows,
                                                     x.shape[-1], p.word, _stream()), "rsp_split_f16_kb32"))
    return p


class PlaneWeight:
    """A GEMM 'weight' that is itself an activation held as Planes (rows [r0, r0+n) of a plane tensor),
    e.g. mask_feature in `einsum('bqc,bchw->bqhw')` (models.py:357)."""

    def __init__(self, planes, r0=0, n=None):
        self.N = planes.rows - r0 if n is None else n
        self.K = planes.shape[-1]
        self.scale_log2 = planes.scale_log2
        self.f8 = planes.f8
        self.b_rows = planes.rows
        self.hi = planes.hi[:, r0:, :]
        self.lo = planes.lo[:, r0:, :]
        self.bias = None


def _gemm_plan(d):
    """RspGemmPlan of a descriptor (rsp_gemm_plan: the kernel rsp_gemm launches for it; host code, no device work), or None
    for one that rsp_gemm refuses."""
    p = _lib_real.RspGemmPlan()
    return p if _lib_real.load().rsp_gemm_plan(d, p) == 0 else None


_GEMM_KERNEL_NAMES = {CONST['RSP_GEMM_KERNEL_F32A']: 'gemm_f16x3_kernel', CONST['RSP_GEMM_KERNEL_DMA']: 'gemm_f16x3_dma_kernel',
                      CONST['RSP_GEMM_KERNEL_S2']: 'gemm_f16x3_s2_kernel', CONST['RSP_GEMM_KERNEL_PP']: 'gemm_f16x3_pp_kernel'}


def _gemm_label(d):
    """Profiler label of rsp_gemm(d): the kernel and block tile of its plan (bench.py groups its per-kernel table by it)."""
    p = _gemm_plan(d)
    if p is None or p.kernel not in _GEMM_KERNEL_NAMES:
        return 'rsp_gemm'               # refused, or M == 0: nothing is launched
    return f"{'gemm_f16f8_dma_kernel' if p.f8 else _GEMM_KERNEL_NAMES[p.kernel]}<{p.bm}x{p.bn}>"


PP_AUTO = True      # False: rsp_gemm's choice of the ping-pong kernel (csrc/gemm_pp.hip) is overridden by gemm_s2 (A/B runs)


def gemm(a, w, *, out=None, bias="auto", res=None, act=ACT_NONE, a_rowmap=None, c_rowmap=None,
         M=None, out_rows=None, res_mod=0, a_scale_log2=DEFAULT_A_SCALE_LOG2, conv=None,
         res_bmap=None, res_brows=0, out_planes=False, out_f32=True, dma="auto", tile_hint=0, c_ncols=0, pl_col0=0,
         out_f8=False, plan_only=False):
    """C = act(A @ W^T + bias) + res   (see RspGemmDesc in include/rsp_hip.h).

    plan_only launches nothing and answers from rsp_gemm_plan(desc).  True: -1 = a gemm_dma.hip / gemm.hip tile (or the
    ping-pong kernel) serves the call, otherwise the epilogue form of gemm_f16x3_s2_kernel (tests assert which
    specialisation they exercise); 'pp': the rows (256 / 128) of the gemm_f16x3_pp_kernel tile that serves it, else 0.

    a: [rows, K] fp32 (row stride = a.stride(0)) or, with conv=(k, stride, pad),
       an NHWC tensor [B, H, W, C].
    A weight packed with f8=True selects the fp8-corrected product: `a` must then be f8 Planes (or an fp32 tensor, which
    is converted); out_f8=True writes the output planes in that format for the next such GEMM.
    """
    lib = _lib.load()
    w_f8 = bool(getattr(w, 'f8', False))
    if not isinstance(a, Planes):
        _chk_f32(a, "a")
        # the DMA fast path wants fp16 planes: convert once when the GEMM is big enough to amortise it
        if (dma is True or (dma == "auto" and w.N > 64 and w.K >= 128)) and a.is_contiguous() \
                and a.shape[-1] % 32 == 0:
            a = to_planes(a, a_scale_log2, w_f8)
    is_planes = isinstance(a, Planes)
    if is_planes:
        a_scale_log2 = a.scale_log2
    if (a.f8 if is_planes else False) != w_f8:
        raise ValueError('fp8-corrected product: A planes and the weight must both be packed with f8=True')
    d = _lib.RspGemmDesc()
    if conv is not None:
        k, stride, pad = conv
        if len(a.shape) != 4 or not (is_planes or a.is_contiguous()):
            raise ValueError("conv gemm expects a contiguous NHWC tensor")
        B, H, W, C = a.shape
        Ho = (H + 2 * pad - k) // stride + 1
        Wo = (W + 2 * pad - k) // stride + 1
        m = B * Ho * Wo
        d.conv_k, d.conv_stride, d.conv_pad = k, stride, pad
        d.conv_H, d.conv_W, d.conv_C, d.conv_Ho, d.conv_Wo = H, W, C, Ho, Wo
        d.lda = C
        if w.K != k * k * C:
            raise ValueError(f"conv weight K={w.K} != {k}*{k}*{C}")
    else:
        if len(a.shape) != 2 or (not is_planes and a.stride(1) != 1):
            raise ValueError("gemm expects a 2-D row-major A")
        m = a.shape[0] if M is None else M
        if a.shape[1] != w.K:
            raise ValueError(f"A has K={a.shape[1]}, weight has K={w.K}")
        d.lda = a.shape[1] if is_planes else a.stride(0)
    n = w.N
    rows = m if out_rows is None else out_rows
    pl = None
    if (c_ncols or pl_col0) and not (is_planes and out_planes):
        raise ValueError('column-range outputs (c_ncols / pl_col0) belong to the plane path with out_planes=True')
    if out_planes:
        if isinstance(out_planes, Planes):         # a caller-owned plane tensor (rows the GEMM does not map keep their contents)
            pl = out_planes
            if tuple(pl.shape) != (rows, n - pl_col0) or pl.f8 != bool(out_f8):
                raise ValueError('out_planes: a Planes tensor of the output\'s shape and format')
        else:
            pl = empty_planes((rows, n - pl_col0), a.device, f8=out_f8)
        d.Chi, d.Clo, d.c_scale_log2, d.c_rows = pl.hi.data_ptr(), pl.lo.data_ptr(), pl.word, rows
    d.c_ncols, d.pl_col0 = c_ncols, pl_col0
    if out is None and out_f32:
        # (a scattered output leaves the rows nobody maps to unwritten: zeroed under the finite check, else never read)
        alloc = torch.zeros if (DEBUG_FINITE and c_rowmap is not None) else torch.empty
        out = alloc((rows, c_ncols or n), dtype=torch.float32, device=a.device)
    if out is not None:
        _chk_f32(out, "out")
    if bias == "auto":
        bias = w.bias
    if isinstance(res, Planes):
        if not is_planes:
            raise ValueError('a plane residual needs the plane path')
        d.res_hi, d.res_lo, d.res_scale_log2, d.res_rows = res.hi.data_ptr(), res.lo.data_ptr(), res.scale_log2, res.rows
        res = None
    if res is not None:
        _chk_f32(res, "res")
        d.ldr = res.stride(0)
    if is_planes:
        d.Ahi, d.Alo, d.a_rows = a.hi.data_ptr(), a.lo.data_ptr(), a.rows
    else:
        d.A = a.data_ptr()
    d.Bhi, d.Blo, d.C = w.hi.data_ptr(), w.lo.data_ptr(), _ptr(out)
    d.bias, d.res = _ptr(bias), _ptr(res)
    d.a_rowmap, d.c_rowmap = _ptr(a_rowmap), _ptr(c_rowmap)
    d.M, d.N, d.K = m, n, w.K
    d.ldc = out.stride(0) if out is not None else n
    d.res_mod = res_mod
    d.res_bmap, d.res_brows = _ptr(res_bmap), res_brows
    d.b_rows = getattr(w, 'b_rows', 0)
    d.tile_hint = tile_hint
    if d.c_rows == 0:
        d.c_rows = rows          # also bounds C when rows are scattered (c_rowmap)
    d.act = act
    d.a_scale_log2 = plane_word(a_scale_log2, w_f8)
    d.alpha = math.ldexp(1.0, -(a_scale_log2 + w.scale_log2))
    plan = _gemm_plan(d) if plan_only or not PP_AUTO else None
    if not PP_AUTO and tile_hint == 0 and plan is not None and plan.kernel == CONST['RSP_GEMM_KERNEL_PP']:
        d.tile_hint = 40        # A/B switch (tools/ab_bench.py "ops.PP_AUTO=False"): the round-3 kernel for these shapes
        plan = _gemm_plan(d)
    if plan_only == 'pp':       # 256 / 128: gemm_f16x3_pp_kernel (csrc/gemm_pp.hip) with that tile serves the call, else 0
        return plan.bm if plan is not None and plan.kernel == CONST['RSP_GEMM_KERNEL_PP'] else 0
    if plan_only:
        return plan.epi if plan is not None and plan.kernel == CONST['RSP_GEMM_KERNEL_S2'] else -1
    _timed(_gemm_label(d) if _prof is not None else None, 2.0 * m * n * w.K, 4.0 * (m * w.K + m * n) + 4.0 * n * w.K,
           lambda: _lib.check(lib.rsp_gemm(d, _stream()), "rsp_gemm"),
           detail=f'M={m} N={n} K={w.K}' + (' conv' if conv is not None else ''))
    if DEBUG_FINITE and out is not None and not bool(torch.isfinite(out).all()):
        raise FloatingPointError(f'rsp_gemm produced non-finite values (M={m} N={n} K={w.K})')
    if out_planes:
        return (out, pl) if out_f32 else pl
    return out


def layernorm(x, gamma, beta, eps=1e-6, act=ACT_NONE, out=None, planes=False, f32=True, f8=False):
    """planes=True additionally returns the result as fp16 Planes (f32=False: planes only; f8: cat8 second plane)."""
    lib = _lib.load()
    _chk_f32(x, "x")
    if not x.is_contiguous():
        raise ValueError("layernorm expects a contiguous tensor")
    C = x.shape[-1]
    rows = x.numel() // C
    if planes:
        pl = empty_planes(x.shape, x.device, f8=f8)
        y = torch.empty_like(x) if f32 else None
        _timed('layernorm_kernel', 0, 8.0 * x.numel() + (4.0 * x.numel() if f32 else 0),
               lambda: _lib.check(lib.rsp_layernorm_ex(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(y),
                                                       pl.hi.data_ptr(), pl.lo.data_ptr(), pl.word, rows, C,
                                                       eps, act, _stream()), "rsp_layernorm_ex"))
        return (y, pl) if f32 else pl
    if out is None:
        out = torch.empty_like(x)
    _timed('layernorm_kernel', 0, 8.0 * x.numel(),
           lambda: _lib.check(lib.rsp_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                                rows, C, eps, act, _stream()), "rsp_layernorm"))
    return out


def vit_relpos(qkv, rel_pos_h, rel_pos_w, Bp, S, nh, dh, q_ld=None, rows=None):
    """q_ld: row stride of the tensor holding q in its first nh*dh columns (default: the [.., 3, nh, dh] qkv matrix).
    rows (int32, windowed layers): only these q rows are evaluated (the real tokens of padded windows); the other rows of
    the result stay unwritten."""
    lib = _lib.load()
    rel = torch.empty((Bp * nh, S * S, 2 * S), dtype=torch.float32, device=qkv.device)
    q_ld = 3 * nh * dh if q_ld is None else q_ld
    n_rows = 0 if rows is None else int(rows.shape[0])
    _timed('vit_relpos_kernel', 2.0 * Bp * nh * S * S * 2 * S * dh, 0,
           lambda: _lib.check(lib.rsp_vit_relpos_rows(qkv.data_ptr(), q_ld, rel_pos_h.data_ptr(), rel_pos_w.data_ptr(),
                                                      rel.data_ptr(), Bp, S, nh, dh, _ptr(rows), n_rows, _stream()),
                              "rsp_vit_relpos_rows"))
    return rel


def vit_attention_planes(q, kv, rel, Bp, S, nh, dh, scale, planes=False, f8=False, win_grid=None):
    """SAM ViT attention with q as fp32 rows [Bp*T, nh*dh] and K | V as the fp16 Planes [Bp*T, 2*nh*dh] the qkv GEMM
    wrote (gemm(..., out_planes=True, c_ncols=D, pl_col0=D)).  planes=True: the output only as Planes.
    win_grid=(windows per image side, real rows / columns of the last window): the outputs of the padded tokens of
    window_partition are not computed (their rows of the result are left unwritten)."""
    lib = _lib.load()
    T, D = S * S, nh * dh
    if not isinstance(kv, Planes) or kv.shape[-1] != 2 * D or kv.rows < Bp * T:
        raise ValueError('kv must be the K | V planes of the qkv GEMM')
    _chk_f32(q, 'q')
    out = None if planes else torch.empty((Bp * T, D), dtype=torch.float32, device=q.device)
    pl = empty_planes((Bp * T, D), q.device, f8=f8) if planes else None
    hi, lo, e = (pl.hi.data_ptr(), pl.lo.data_ptr(), pl.word) if planes else (0, 0, 0)
    if kv.f8:
        raise ValueError('K | V planes are consumed as fp16 hi / lo planes (qkv GEMM: out_f8=False)')
    kind = 'global' if T >= 1024 else 'window'
    wn, wr = (int(win_grid[0]), int(win_grid[1])) if (win_grid is not None and S == 14) else (0, 0)
    _timed('attn_stream_kernel<vit,global>' if S != 14 else 'attn_win_kernel<vit,window,rel given>',
           4.0 * Bp * nh * T * T * dh, 0,
           lambda: _lib.check(lib.rsp_vit_attention_planes_ex(q.data_ptr(), q.stride(0), kv.hi.data_ptr(), kv.lo.data_ptr(),
                                                              kv.rows, kv.scale_log2, rel.data_ptr(), _ptr(out), hi, lo, e,
                                                              Bp, S, nh, dh, scale, wn, wr, _stream()),
                              "rsp_vit_attention_planes_ex"))
    return pl if planes else out


def pack_relpos_tables(rel_pos_h, rel_pos_w, S, dh):
    """the two rel-pos tables of a windowed layer ([2S-1, dh] fp32 each) as the fp16 hi / lo planes rsp_vit_window_attention
    DMAs into LDS: uint16 [2, 2, 32, dh + 8] (rsp_pack_relpos_tables; once per layer at pack time)."""
    lib = _lib.load()
    _chk_f32(rel_pos_h, 'rel_pos_h')
    _chk_f32(rel_pos_w, 'rel_pos_w')
    if tuple(rel_pos_h.shape) != (2 * S - 1, dh) or tuple(rel_pos_w.shape) != (2 * S - 1, dh):
        raise ValueError(f'rel-pos tables must be [{2 * S - 1}, {dh}]')
    out = torch.empty((2, 2, 32, dh + 8), dtype=torch.float16, device=rel_pos_h.device)
    _lib.check(lib.rsp_pack_relpos_tables(rel_pos_h.contiguous().data_ptr(), rel_pos_w.contiguous().data_ptr(), out.data_ptr(),
                                          S, dh, _stream()), 'rsp_pack_relpos_tables')
    return out


def vit_window_attention(q, kv, rel_tab, Bp, nh, dh, scale, planes=False, f8=False, win_grid=None, variant=0):
    """Windowed SamVisionAttention (HF:803-831 with get_decomposed_rel_pos HF:761-801) in ONE kernel: q fp32 rows
    [Bp*196, nh*dh], K | V as the qkv GEMM's fp16 Planes, rel_tab = pack_relpos_tables(...) of the layer; the rel-pos terms
    are computed inside (csrc/attn_win.hip).  win_grid as in vit_attention_planes."""
    lib = _lib.load()
    T, D = 196, nh * dh
    if not isinstance(kv, Planes) or kv.shape[-1] != 2 * D or kv.rows < Bp * T or kv.f8:
        raise ValueError('kv must be the fp16 K | V planes of the qkv GEMM')
    if tuple(rel_tab.shape) != (2, 2, 32, dh + 8) or rel_tab.dtype != torch.float16 or not rel_tab.is_contiguous():
        raise ValueError('rel_tab must come from pack_relpos_tables')
    _chk_f32(q, 'q')
    out = None if planes else torch.empty((Bp * T, D), dtype=torch.float32, device=q.device)
    pl = empty_planes((Bp * T, D), q.device, f8=f8) if planes else None
    hi, lo, e = (pl.hi.data_ptr(), pl.lo.data_ptr(), pl.word) if planes else (0, 0, 0)
    wn, wr = (int(win_grid[0]), int(win_grid[1])) if win_grid is not None else (0, 0)
    # flops: the padded-window figure of SURVEY section 8(d) (bench.py also quotes the evaluated-query figure); the 30 + 28
    # rel-pos / bias MFMAs per wave are not counted
    _timed('attn_win_kernel<vit,window>', 4.0 * Bp * nh * T * T * dh, 0,
           lambda: _lib.check(lib.rsp_vit_window_attention(q.data_ptr(), q.stride(0), kv.hi.data_ptr(), kv.lo.data_ptr(),
                                                           kv.rows, kv.scale_log2, rel_tab.data_ptr(), _ptr(out), hi, lo, e,
                                                           Bp, nh, dh, scale, wn, wr, variant, _stream()),
                              'rsp_vit_window_attention'))
    return pl if planes else out


SAM_I2T_FUSED_MAX_TOKENS = CONST['RSP_SAM_I2T_FUSED_MAX_TOKENS']   # rsp_sam_i2t_fused (LDS budget); more tokens: sam_i2t_attention + GEMM + layernorm


def sam_i2t_fused(q, k, v, wo, bo, gamma, beta, *, R, T, N, scale, eps=1e-6, q_map=None, res=None, res_map=None,
                  res_planes=None, planes=True, f32=False):
    """LayerNorm(residual + out_proj(image -> token attention)) in one kernel (HF:340-348), out_proj folded into the
    values.  q [Rq*N,128] (q_map: RoI -> row block), k / v [R*T,128], wo [256,128] fp32, bo [256]; residual either fp32
    rows `res` [Rres*N,256] (+ res_map) or Planes of the [R*N,256] tensor.  Returns Planes (and / or fp32)."""
    lib = _lib.load()
    for t, n in ((q, 'q'), (k, 'k'), (v, 'v'), (wo, 'wo'), (bo, 'bo'), (gamma, 'gamma'), (beta, 'beta')):
        _chk_f32(t, n)
        if not t.is_contiguous():
            raise ValueError(f'sam_i2t_fused: {n} must be contiguous')
    if tuple(wo.shape) != (256, 128) or q.shape[-1] != 128:
        raise ValueError('sam_i2t_fused expects internal width 128 and a [256, 128] out_proj weight')
    if (res is None) == (res_planes is None):
        raise ValueError('sam_i2t_fused: exactly one of res / res_planes')
    d = _lib.RspI2tFusedDesc()
    d.q, d.q_map, d.k, d.v, d.wo, d.bo = q.data_ptr(), _ptr(q_map), k.data_ptr(), v.data_ptr(), wo.data_ptr(), bo.data_ptr()
    if res is not None:
        _chk_f32(res, 'res')
        if not res.is_contiguous() or res.shape[-1] != 256:
            raise ValueError('sam_i2t_fused: res must be contiguous rows of 256')
        d.res, d.res_map = res.data_ptr(), _ptr(res_map)
    else:
        if res_planes.f8 or res_planes.rows != R * N or res_planes.shape[-1] != 256:
            raise ValueError('sam_i2t_fused: res_planes must be the fp16 hi / lo planes of the [R*N, 256] tensor')
        d.res_hi, d.res_lo, d.res_scale_log2 = res_planes.hi.data_ptr(), res_planes.lo.data_ptr(), res_planes.scale_log2
    d.gamma, d.beta, d.eps = gamma.data_ptr(), beta.data_ptr(), eps
    out = torch.empty((R * N, 256), dtype=torch.float32, device=q.device) if f32 else None
    pl = empty_planes((R * N, 256), q.device) if planes else None
    d.out = _ptr(out)
    if pl is not None:
        d.out_hi, d.out_lo, d.out_scale_log2 = pl.hi.data_ptr(), pl.lo.data_ptr(), pl.scale_log2
    d.R, d.T, d.N, d.scale = R, T, N, scale
    # algorithmic work: scores + the folded out_proj product; bytes: q + residual + result rows
    _timed('sam_i2t_fused_kernel', 2.0 * R * N * T * (128 + 8 * 256), 4.0 * R * N * (128 + 256 + 256),
           lambda: _lib.check(lib.rsp_sam_i2t_fused(d, _stream()), "rsp_sam_i2t_fused"), detail=f'R={R} T={T} N={N}')
    if planes and f32:
        return out, pl
    return pl if planes else out


_attn_ws = {}


def _attn_workspace(nbytes, device):
    """K / V^T plane scratch of the global-attention path, kept per device (layers run back to back on one stream)."""
    key = str(device)
    buf = _attn_ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        _attn_ws[key] = buf
    return buf


def vit_attention(qkv, rel, Bp, S, nh, dh, scale, planes=False):
    """planes=True: return the output only as fp16 Planes (it feeds the proj GEMM's DMA path)."""
    lib = _lib.load()
    kind = 'global' if S * S >= 1024 else 'window'
    fl = 4.0 * Bp * nh * (S * S) ** 2 * dh
    pl = empty_planes((Bp * S * S, nh * dh), qkv.device) if planes else None
    out = None if planes else torch.empty((Bp * S * S, nh * dh), dtype=torch.float32, device=qkv.device)
    hi, lo, e = (pl.hi.data_ptr(), pl.lo.data_ptr(), pl.scale_log2) if planes else (0, 0, 0)
    if S in (64, 32):
        ws = _attn_workspace(int(lib.rsp_vit_attention_global_ws_bytes(Bp, S, nh, dh)), qkv.device)
        _timed(f'attn_global_kernel<vit>', fl, 0,
               lambda: _lib.check(lib.rsp_vit_attention_global(qkv.data_ptr(), rel.data_ptr(), ws.data_ptr(), _ptr(out),
                                                               hi, lo, e, Bp, S, nh, dh, scale, _stream()),
                                  "rsp_vit_attention_global"))
    else:
        _timed(f'attn_kernel<vit,{kind}>', fl, 0,
               lambda: _lib.check(lib.rsp_vit_attention_ex(qkv.data_ptr(), rel.data_ptr(), _ptr(out), hi, lo, e, Bp, S,
                                                           nh, dh, scale, _stream()), "rsp_vit_attention_ex"))
    return pl if planes else out


def patchify(img, patch):
    """NCHW fp32 image batch -> [B*gh*gw, C*p*p] patch rows (k = (c, ky, kx))."""
    lib = _lib.load()
    _chk_f32(img, "img")
    B, C, H, W = img.shape
    out = torch.empty((B * (H // patch) * (W // patch), C * patch * patch), dtype=torch.float32,
                      device=img.device)
    _lib.check(lib.rsp_patchify(img.data_ptr(), out.data_ptr(), B, C, H, W, patch, _stream()),
               "rsp_patchify")
    return out


def preprocess(imgs, mean, std, swap_rb, pad_divisor=1, pad_value=0.0, device=None):
    """DetDataPreprocessor: list of CHW uint8/fp32 tensors -> normalised fp32 [B,3,Hp,Wp]."""
    import ctypes
    lib = _lib.load()
    device = device or imgs[0].device
    Hm = max(int(i.shape[1]) for i in imgs)
    Wm = max(int(i.shape[2]) for i in imgs)
    Hp = (Hm + pad_divisor - 1) // pad_divisor * pad_divisor
    Wp = (Wm + pad_divisor - 1) // pad_divisor * pad_divisor
    out = torch.empty((len(imgs), 3, Hp, Wp), dtype=torch.float32, device=device)
    m3 = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in std])
    for b, im in enumerate(imgs):
        im = im.to(device).contiguous()
        if im.dtype == torch.uint8:
            is_u8 = 1
        else:
            im = im.to(torch.float32)
            is_u8 = 0
        _lib.check(lib.rsp_preprocess(im.data_ptr(), is_u8, out[b].data_ptr(), int(im.shape[1]),
                                      int(im.shape[2]), Hp, Wp, m3, s3, 1 if swap_rb else 0,
                                      float(pad_value), _stream()), "rsp_preprocess")
    return out


def paste_masks(logits_nhwc, labels, boxes, img_hw, thr=0.5):
    """FCNMaskHead mask paste: logits [k, Hm, Wm, C] (NHWC), labels int [k] or None, boxes [k, 4] -> bool [k, H, W];
    thr < 0: uint8 [k, H, W], the pasted probabilities as (p * 255) truncated (fcn_mask_head.py:390-394)."""
    lib = _lib.load()
    _chk_f32(logits_nhwc, 'logits')
    k, Hm, Wm, C = logits_nhwc.shape
    H, W = int(img_hw[0]), int(img_hw[1])
    out = torch.empty((k, H, W), dtype=torch.bool if thr >= 0 else torch.uint8, device=logits_nhwc.device)
    if k:
        lab = None if labels is None else labels.to(torch.int32).contiguous()
        _lib.check(lib.rsp_paste_masks(logits_nhwc.contiguous().data_ptr(), _ptr(lab), boxes.contiguous().data_ptr(), k, Hm, Wm,
                                       C, H, W, float(thr), out.data_ptr(), _stream()), "rsp_paste_masks")
    return out


def resize_pad(img_hwc, new_hw, pad_hw, pad_val=(0.0, 0.0, 0.0), out=None, normalise=None):
    """Resize(keep_ratio) + Pad of the test pipeline on one decoded HWC image (uint8 / fp32, device tensor) ->
    fp32 [3, Hp, Wp] (see rsp_resize_pad).  normalise = (mean3, std3, swap_rb) fuses the DetDataPreprocessor step."""
    import ctypes
    lib = _lib.load()
    if img_hwc.dim() != 3 or img_hwc.shape[2] != 3 or not _is_device(img_hwc):
        raise ValueError('resize_pad expects an [H, W, 3] device tensor')
    im = img_hwc.contiguous()
    if im.dtype != torch.uint8:
        im = im.to(torch.float32)
    H, W = int(im.shape[0]), int(im.shape[1])
    Hn, Wn = int(new_hw[0]), int(new_hw[1])
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    if out is None:
        out = torch.empty((3, Hp, Wp), dtype=torch.float32, device=im.device)
    p3 = (ctypes.c_float * 3)(*[float(v) for v in pad_val])
    if normalise is None:
        m3 = s3 = None
        nrm, swap = 0, 0
    else:
        m3 = (ctypes.c_float * 3)(*[float(v) for v in normalise[0]])
        s3 = (ctypes.c_float * 3)(*[float(v) for v in normalise[1]])
        nrm, swap = 1, 1 if normalise[2] else 0
    _lib.check(lib.rsp_resize_pad(im.data_ptr(), 1 if im.dtype == torch.uint8 else 0, out.data_ptr(), H, W, Hn, Wn,
                                  Hp, Wp, p3, nrm, swap, m3, s3, _stream()), "rsp_resize_pad")
    return out


def conv_transpose2x2(x_nhwc, w_dy, bias, act=ACT_NONE, a_scale_log2=DEFAULT_A_SCALE_LOG2, out_planes=False,
                      hyper=None, ln=None):
    """ConvTranspose2d(k=2, s=2) on NHWC as GEMMs.

    x_nhwc: fp32 [B, H, W, Cin] or Planes of that logical shape.
    w_dy: a pair of PackedWeights [(dx, co), Cin] (one GEMM per output-row parity, bias tiled x2), or ONE
    PackedWeight [(dy, dx, co), Cin] (all four sub-pixels in one pass over A, bias tiled x4; plane path only).
    Returns [B, 2H, 2W, Cout] (fp32, or Planes when out_planes).  hyper [B, Cout=32]: fuse
    `sum_c act(.)[.., c] * hyper[b, c]` into the epilogue and return [B, 2H, 2W] (the SAM decoder's
    hyper-network product, HF:523-531).  ln=(gamma, beta, eps): LayerNorm2d over the Cout=64 channels of every
    output pixel before `act` (HF:519-520), one-weight form only, returns Planes."""
    B, H, W, Cin = x_nhwc.shape
    four = not isinstance(w_dy, (tuple, list))
    ws = (w_dy,) if four else tuple(w_dy)
    cout = ws[0].N // (4 if four else 2)
    dev = x_nhwc.device
    if not isinstance(x_nhwc, Planes) and (four or out_planes or hyper is not None
                                           or (Cin % 32 == 0 and B * H * W >= 4096)):
        x_nhwc = to_planes(x_nhwc.contiguous(), a_scale_log2)
    a = x_nhwc.view(B * H * W, Cin)
    dys = (-1,) if four else (0, 1)
    if hyper is not None:
        out = torch.empty((B, 2 * H, 2 * W), dtype=torch.float32, device=dev)
        if four and Cin == 64 and cout == 32 and act == ACT_GELU and bias is not None:
            # the SAM upscaler's last stage: dedicated streaming kernel (weights resident in LDS)
            lib = _lib.load()
            w = ws[0]
            rows = B * H * W
            _timed('sam_upscale2_kernel', 2.0 * rows * 128 * 64, 4.0 * rows * 64 + 4.0 * rows * 4,
                   lambda: _lib.check(lib.rsp_sam_upscale2(a.hi.data_ptr(), a.lo.data_ptr(), rows, a.scale_log2,
                                                           w.hi.data_ptr(), w.lo.data_ptr(), w.scale_log2,
                                                           bias.data_ptr(), hyper.data_ptr(), out.data_ptr(), H * W, W,
                                                           _stream()), "rsp_sam_upscale2"))
            return out
        for w, dy in zip(ws, dys):
            _gemm_ct(a, w, None, bias, act, W, dy, a_scale_log2, hyper=hyper, hd_out=out, hd_rows=H * W)
        return out
    if ln is not None:
        if not four or cout != 64:
            raise ValueError('the fused LayerNorm epilogue needs the one-weight form with Cout == 64')
        out_planes = True
    if out_planes:
        pl = empty_planes((B, 2 * H, 2 * W, cout), dev)
        for w, dy in zip(ws, dys):
            _gemm_ct(a, w, None, bias, act, W, dy, a_scale_log2, planes_out=pl, c_rows=B * 4 * H * W, ln=ln)
        return pl
    out = torch.empty((B, 2 * H, 2 * W, cout), dtype=torch.float32, device=dev)
    o2 = out.view(B * 2 * H * W, 2 * cout)
    for w, dy in zip(ws, dys):
        _gemm_ct(a, w, o2, bias, act, W, dy, a_scale_log2)
    return out


def _gemm_ct(a, w, out, bias, act, ct_W, ct_dy, a_scale_log2, planes_out=None, c_rows=0, hyper=None, hd_out=None,
             hd_rows=0, ln=None):
    lib = _lib.load()
    d = _lib.RspGemmDesc()
    is_pl = isinstance(a, Planes)
    if is_pl:
        d.Ahi, d.Alo, d.a_rows = a.hi.data_ptr(), a.lo.data_ptr(), a.rows
        a_scale_log2 = a.scale_log2
        d.lda = a.shape[1]
    else:
        d.A = a.data_ptr()
        d.lda = a.stride(0)
    d.Bhi, d.Blo, d.C = w.hi.data_ptr(), w.lo.data_ptr(), _ptr(out)
    d.bias = _ptr(bias)
    d.M, d.N, d.K = a.shape[0], w.N, w.K
    d.ldc = out.stride(0) if out is not None else w.N
    d.act = act
    d.a_scale_log2 = a_scale_log2
    d.alpha = math.ldexp(1.0, -(a_scale_log2 + w.scale_log2))
    d.ct_W, d.ct_dy = ct_W, ct_dy
    if planes_out is not None:
        # the convT output matrix is [B*2H*W rows of 2*Cout]; as planes of the NHWC tensor [.., Cout] the row index
        # doubles (dx folds into the row): handled by viewing the plane tensor as [rows, 2*Cout]
        d.Chi, d.Clo, d.c_scale_log2, d.c_rows = planes_out.hi.data_ptr(), planes_out.lo.data_ptr(), planes_out.scale_log2, c_rows
    if hd_out is not None:
        d.hd_hyper, d.hd_out, d.hd_rows = hyper.data_ptr(), hd_out.data_ptr(), hd_rows
    if ln is not None:
        d.ln_gamma, d.ln_beta, d.ln_eps = ln[0].data_ptr(), ln[1].data_ptr(), ln[2]
    _timed('gemm_f16x3_dma_kernel<convT>' if is_pl else 'gemm_f16x3_kernel<convT>', 2.0 * d.M * d.N * d.K, 4.0 * (d.M * d.K + d.M * d.N),
           lambda: _lib.check(lib.rsp_gemm(d, _stream()), "rsp_gemm(convT)"),
           detail=f'M={d.M} N={d.N} K={d.K}' + (' hyper' if hd_out is not None else '') + (' ln' if ln is not None else ''))


def attention(q, k, v, out, *, B, nh, dh, Tq, Tk, scale, q_strides, k_strides, v_strides, o_strides,
              kv_batch_map=None, q_batch_map=None, out_planes=None, mask=None):
    """Generic strided multi-head attention (RspAttnDesc). strides = (batch, token, head) in elements.
    out_planes: optional Planes receiving a KB32 copy of the dense [B*Tq, nh*dh] output (out may be None)."""
    lib = _lib.load()
    d = _lib.RspAttnDesc()
    d.q, d.k, d.v, d.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), _ptr(out)
    if out_planes is not None:
        d.out_hi, d.out_lo, d.out_scale_log2 = out_planes.hi.data_ptr(), out_planes.lo.data_ptr(), out_planes.scale_log2
    d.kv_batch_map = _ptr(kv_batch_map)
    d.q_batch_map = _ptr(q_batch_map)
    d.mask = _ptr(mask)
    d.q_bs, d.q_ts, d.q_hs = q_strides
    d.k_bs, d.k_ts, d.k_hs = k_strides
    d.v_bs, d.v_ts, d.v_hs = v_strides
    d.o_bs, d.o_ts, d.o_hs = o_strides
    d.B, d.nh, d.dh, d.Tq, d.Tk, d.scale = B, nh, dh, Tq, Tk, scale
    _timed('attn_kernel<sam_decoder>', 4.0 * B * nh * Tq * Tk * dh, 0,
           lambda: _lib.check(lib.rsp_attention(d, _stream()), "rsp_attention"),
           detail=f'B={B} nh={nh} dh={dh} Tq={Tq} Tk={Tk}')
    return out if out_planes is None else out_planes


SAM_T2I_MAX_TOKENS = CONST['RSP_SAM_T2I_MAX_TOKENS']     # rsp_sam_t2i_attention; more tokens go through the generic rsp_attention
SAM_I2T_MAX_TOKENS = CONST['RSP_SAM_I2T_MAX_TOKENS']


def sam_t2i_attention(q, kv, out, *, R, T, N, scale, kv_map=None):
    """SAM decoder token->image attention (8 heads x 16, exact fp32). q [R*T,128], kv [Rkv*N,256] = K|V, out [R*T,128]."""
    lib = _lib.load()
    for t, n in ((q, 'q'), (kv, 'kv'), (out, 'out')):
        _chk_f32(t, n)
        if not t.is_contiguous():
            raise ValueError(f'sam_t2i_attention: {n} must be contiguous')
    if q.shape[-1] != 128 or kv.shape[-1] != 256:
        raise ValueError('sam_t2i_attention expects internal width 128 (q) and fused K|V rows of 256')
    _timed('sam_t2i_kernel', 4.0 * R * T * N * 128, 4.0 * R * N * 256,
           lambda: _lib.check(lib.rsp_sam_t2i_attention(q.data_ptr(), kv.data_ptr(), _ptr(kv_map), out.data_ptr(),
                                                        R, T, N, scale, _stream()), "rsp_sam_t2i_attention"),
           detail=f'R={R} T={T} N={N}')
    return out


def sam_t2i_attention_bias(q, kv, bias, out, *, R, T, N, scale, kv_map=None):
    """sam_t2i_attention with one additive logit per key (HF:260, PerSAM's `attention_similarity`): bias [Rb, N] fp32, Rb = 1
    (shared by the R prompt sets) or R; softmax(q . k * scale + bias) v."""
    lib = _lib.load()
    for t, n in ((q, 'q'), (kv, 'kv'), (out, 'out'), (bias, 'bias')):
        _chk_f32(t, n)
        if not t.is_contiguous():
            raise ValueError(f'sam_t2i_attention_bias: {n} must be contiguous')
    if q.shape[-1] != 128 or kv.shape[-1] != 256:
        raise ValueError('sam_t2i_attention_bias expects internal width 128 (q) and fused K|V rows of 256')
    if bias.dim() != 2 or bias.shape[1] != N or bias.shape[0] not in (1, R):
        raise ValueError(f'sam_t2i_attention_bias: bias must be [1 | {R}, {N}], got {tuple(bias.shape)}')
    if T > SAM_T2I_MAX_TOKENS:
        raise ValueError(f'sam_t2i_attention_bias: at most {SAM_T2I_MAX_TOKENS} tokens')
    Rb = int(bias.shape[0])
    _timed('sam_t2i_bias_kernel', 4.0 * R * T * N * 128, 4.0 * R * N * 257,
           lambda: _lib.check(lib.rsp_sam_t2i_attention_bias(q.data_ptr(), kv.data_ptr(), _ptr(kv_map), bias.data_ptr(), Rb,
                                                             out.data_ptr(), R, T, N, scale, _stream()),
                              "rsp_sam_t2i_attention_bias"),
           detail=f'R={R} T={T} N={N} Rb={Rb}')
    return out


def sam_upscale_fused(x, w1, bias1, gamma, beta, eps, w2p, bias2, hyper, h, w):
    """x Planes [R*h*w, 256] -> masks [R, 4h, 4w] (ConvT + LN + GELU + ConvT + GELU + hyper dot in one kernel, csrc/upscale.hip);
    w1 = PackedWeight [(dy, dx, co), 256], w2p = PackedWeight [(dy2, dx2, c2), 64] with its K columns in the order
    rsp_sam_upscale_fused documents (sam_decoder._upscale2_k_order)."""
    lib = _lib.load()
    if not isinstance(x, Planes) or x.shape[-1] != 256 or x.f8:
        raise ValueError('sam_upscale_fused: x must be fp16 planes with 256 columns')
    rows = x.rows
    R = rows // (h * w)
    out = torch.empty((R, 4 * h, 4 * w), dtype=torch.float32, device=x.device)
    _timed('sam_upscale_fused_kernel', 2.0 * rows * (256 * 256 + 4 * 128 * 64), 4.0 * rows * 256 + 64.0 * rows,
           lambda: _lib.check(lib.rsp_sam_upscale_fused(x.hi.data_ptr(), x.lo.data_ptr(), x.rows, x.scale_log2,
                                                        w1.hi.data_ptr(), w1.lo.data_ptr(), w1.scale_log2, bias1.data_ptr(),
                                                        gamma.data_ptr(), beta.data_ptr(), float(eps), w2p.hi.data_ptr(),
                                                        w2p.lo.data_ptr(), w2p.scale_log2, bias2.data_ptr(),
                                                        hyper.data_ptr(), out.data_ptr(), rows, h * w, w, _stream()),
                              "rsp_sam_upscale_fused"))
    return out


def sam_hq_mask(up, w2, bias2, w1, bias1, gamma, beta, eps, wf, biasf, hyper, feat, feat_map, up_map=None, hyper_sam=None):
    """SAM-HQ's mask branch in one kernel (csrc/sam_hq.hip, HF sam_hq:1007-1037): up Planes [S, 2g, 2g, 64] (the upscaler's
    planes after LayerNorm + GELU; prompt set r reads block up_map[r], int32 [R] -- None: S == R, block r), w2 = PackedWeight
    [(dy, dx, c2), 64] of upscale_conv2 with bias2 [128], w1 = PackedWeight [64, (tap, ci) = 288] of mask_conv1 with bias1
    [64], gamma / beta / eps of mask_norm, wf fp32 [9, 64, 32] = mask_conv2 as [tap][ci][c] with biasf [32], hyper [R, 32],
    feat fp32 [n, 4g, 4g, 32] and feat_map int32 [R] -> mask_hq fp32 [R, 4g, 4g].  hyper_sam [R, n <= 3, 32]: also SAM's masks
    from the same upscaled embedding, + mask_hq: returns (mask_hq, fp32 [R, n, 4g, 4g])."""
    lib = _lib.load()
    if not isinstance(up, Planes) or up.f8 or len(up.shape) != 4 or up.shape[-1] != 64 or up.shape[1] != up.shape[2]:
        raise ValueError('sam_hq_mask: up must be fp16 planes of logical shape [S, 2g, 2g, 64]')
    S, g2 = up.shape[0], up.shape[1]
    R = hyper.shape[0]
    G = 2 * g2
    if g2 % 8:
        raise ValueError(f'sam_hq_mask: the embedding grid must be a multiple of 4, got {g2 // 2}')
    if w2.N != 128 or w2.K != 64 or w1.N != 64 or w1.K != 288 or tuple(wf.shape) != (9, 64, 32):
        raise ValueError('sam_hq_mask: weight shapes')
    if feat.dim() != 4 or tuple(feat.shape[1:]) != (G, G, 32) or tuple(hyper.shape) != (R, 32) or feat_map.numel() != R:
        raise ValueError(f'sam_hq_mask: feat {tuple(feat.shape)} / hyper {tuple(hyper.shape)} for R = {R}, 4g = {G}')
    if (up_map is None and S != R) or (up_map is not None and up_map.numel() != R):
        raise ValueError(f'sam_hq_mask: {S} blocks of up for {R} prompt sets need up_map int32 [{R}]')
    n_sam = 0
    if hyper_sam is not None:
        if hyper_sam.dim() != 3 or hyper_sam.shape[0] != R or not 1 <= hyper_sam.shape[1] <= 3 or hyper_sam.shape[2] != 32:
            raise ValueError(f'sam_hq_mask: hyper_sam {tuple(hyper_sam.shape)}, expected [{R}, 1..3, 32]')
        n_sam = hyper_sam.shape[1]
    for t, name in ((bias2, 'bias2'), (bias1, 'bias1'), (gamma, 'gamma'), (beta, 'beta'), (wf, 'wf'), (biasf, 'biasf'),
                    (hyper, 'hyper'), (feat, 'feat')) + (((hyper_sam, 'hyper_sam'),) if n_sam else ()):
        _chk_f32(t, name)
        if not t.is_contiguous():
            raise ValueError(f'sam_hq_mask: {name} must be contiguous')
    for t, name in ((feat_map, 'feat_map'), (up_map, 'up_map')):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise ValueError(f'sam_hq_mask: {name} must be contiguous int32')
    out = torch.empty((R, G, G), dtype=torch.float32, device=up.device)
    out_sam = torch.empty((R, n_sam, G, G), dtype=torch.float32, device=up.device) if n_sam else None
    npx = float(R) * G * G
    _timed('sam_hq_mask_kernel', 2.0 * npx * (1.56 * 32 * 64 + 1.27 * 288 * 64 + 576 + 32 * (1 + n_sam)),
           4.0 * R * g2 * g2 * 64 + 4.0 * npx * (33 + n_sam),
           lambda: _lib.check(lib.rsp_sam_hq_mask(up.hi.data_ptr(), up.lo.data_ptr(), up.rows, up.scale_log2, _ptr(up_map), S,
                                                  w2.hi.data_ptr(), w2.lo.data_ptr(), w2.scale_log2, bias2.data_ptr(),
                                                  w1.hi.data_ptr(), w1.lo.data_ptr(), w1.scale_log2, bias1.data_ptr(),
                                                  gamma.data_ptr(), beta.data_ptr(), float(eps), wf.data_ptr(),
                                                  biasf.data_ptr(), hyper.data_ptr(), feat.data_ptr(), feat_map.data_ptr(),
                                                  feat.shape[0], out.data_ptr(), _ptr(hyper_sam), _ptr(out_sam), n_sam, R,
                                                  g2 // 2, _stream()), "rsp_sam_hq_mask"),
           detail=f'R={R} S={S} g={g2 // 2} n_sam={n_sam}')
    return out if not n_sam else (out, out_sam)


SAM_T2I_FOLD_MAX_TOKENS = CONST['RSP_SAM_T2I_FOLD_MAX_TOKENS']    # 8 heads x T query columns fit the kernel's 96


def sam_t2i_fold(keys, pek, qp, tqx, *, R, N, ncols):
    """token -> image attention over the per-RoI key planes with the K | V projections folded in (csrc/t2i_fold.hip):
    keys Planes [R*N, 256]; pek Planes [N, 128] = k_proj(pe) without the bias; qp Planes [R*96, 256] and tqx Planes [R*96, 128] (see
    rsp_sam_t2i_fold).  Returns u fp32 [R*96, 256] = sum_n softmax[n] keys[n] per (RoI, column); the rows of the columns
    >= ncols are zero."""
    lib = _lib.load()
    for t, name, k in ((keys, 'keys', 256), (pek, 'pek', 128), (qp, 'qp', 256), (tqx, 'tqx', 128)):
        if not isinstance(t, Planes) or t.shape[-1] != k or t.f8:
            raise ValueError(f'sam_t2i_fold: {name} must be fp16 planes with {k} columns')
    if qp.rows != tqx.rows or qp.rows < R * 96 or keys.rows < R * N or pek.rows != N:
        raise ValueError('sam_t2i_fold: row counts')
    u = torch.zeros((R * 96, 256), dtype=torch.float32, device=keys.device)
    _timed('sam_t2i_fold_kernel', 2.0 * R * N * 96 * (256 + 128 + 256), 4.0 * R * N * 256,
           lambda: _lib.check(lib.rsp_sam_t2i_fold(keys.hi.data_ptr(), keys.lo.data_ptr(), keys.rows, keys.scale_log2,
                                                   pek.hi.data_ptr(), pek.lo.data_ptr(), pek.scale_log2,
                                                   qp.hi.data_ptr(), qp.lo.data_ptr(), qp.scale_log2,
                                                   tqx.hi.data_ptr(), tqx.lo.data_ptr(), tqx.scale_log2, qp.rows,
                                                   u.data_ptr(), R, N, ncols, _stream()), "rsp_sam_t2i_fold"))
    return u


def sam_fold_expand(tq, R, T, scale):
    """projected token queries tq [R*T, 128] -> Planes [R*96, 128] of the block-diagonal, pre-scaled query (rsp_sam_fold_expand)"""
    lib = _lib.load()
    _chk_f32(tq, 'tq')
    if not tq.is_contiguous() or tuple(tq.shape) != (R * T, 128):
        raise ValueError('sam_fold_expand: tq must be a contiguous [R*T, 128] tensor')
    pl = empty_planes((R * 96, 128), tq.device)
    _timed('sam_fold_expand_kernel', 0, 4.0 * tq.numel() + 4.0 * R * 96 * 128,
           lambda: _lib.check(lib.rsp_sam_fold_expand(tq.data_ptr(), pl.hi.data_ptr(), pl.lo.data_ptr(), pl.word, R, T, float(scale),
                                                      _stream()), 'rsp_sam_fold_expand'))
    return pl


def sam_fold_gather(full, R, T):
    """full [R*96, 128] (v_proj applied to every column of the folded attention's result) -> [R*T, 128]: every column's own head"""
    lib = _lib.load()
    _chk_f32(full, 'full')
    if not full.is_contiguous() or tuple(full.shape) != (R * 96, 128):
        raise ValueError('sam_fold_gather: full must be a contiguous [R*96, 128] tensor')
    ao = torch.empty((R * T, 128), dtype=torch.float32, device=full.device)
    _timed('sam_fold_gather_kernel', 0, 8.0 * ao.numel(),
           lambda: _lib.check(lib.rsp_sam_fold_gather(full.data_ptr(), ao.data_ptr(), R, T, _stream()), 'rsp_sam_fold_gather'))
    return ao


def sam_i2t_attention(q, k, v, *, R, T, N, scale, q_map=None, out=None, out_planes=None):
    """SAM decoder image->token attention. q [Rq*N,128], k/v [R*T,128]; result [R*N,128] into `out` and/or Planes."""
    lib = _lib.load()
    for t, n in ((q, 'q'), (k, 'k'), (v, 'v')):
        _chk_f32(t, n)
        if not t.is_contiguous():
            raise ValueError(f'sam_i2t_attention: {n} must be contiguous')
    hi = lo = 0
    e = 0
    if out_planes is not None:
        hi, lo, e = out_planes.hi.data_ptr(), out_planes.lo.data_ptr(), out_planes.scale_log2
    _timed('sam_i2t_kernel', 4.0 * R * T * N * 128, 4.0 * R * N * 128 * 2,
           lambda: _lib.check(lib.rsp_sam_i2t_attention(q.data_ptr(), _ptr(q_map), k.data_ptr(), v.data_ptr(),
                                                        _ptr(out), hi, lo, e, R, T, N, scale, _stream()),
                              "rsp_sam_i2t_attention"),
           detail=f'R={R} T={T} N={N}')
    return out if out_planes is None else out_planes


def roi_align(feats_nhwc, pes, rois, P, strides, finest_scale=56):
    """feats_nhwc: list of [B,H,W,C]; pes: list of [H,W,C] or None; rois [K,5] -> [K,P,P,C]."""
    lib = _lib.load()
    K = rois.shape[0]
    C = feats_nhwc[0].shape[-1]
    out = torch.empty((K, P, P, C), dtype=torch.float32, device=rois.device)
    if K == 0:
        return out
    d = _lib.RspRoiAlignDesc()
    for i, f in enumerate(feats_nhwc):
        _chk_f32(f, "feat")
        if not f.is_contiguous():
            raise ValueError("roi_align expects contiguous NHWC levels")
        d.feat[i] = f.data_ptr()
        d.pe[i] = 0 if pes is None or pes[i] is None else pes[i].data_ptr()
        d.H[i], d.W[i] = f.shape[1], f.shape[2]
        d.spatial_scale[i] = 1.0 / strides[i]
    d.rois, d.out = rois.data_ptr(), out.data_ptr()
    d.K, d.P, d.C, d.num_levels, d.finest_scale = K, P, C, len(feats_nhwc), finest_scale
    _timed('roi_align_kernel', 0, 4.0 * out.numel(),
           lambda: _lib.check(lib.rsp_roi_align(d, _stream()), "rsp_roi_align"))
    return out


def pool2(x_nhwc, mode):
    lib = _lib.load()
    B, H, W, C = x_nhwc.shape
    Ho, Wo = (H // 2, W // 2) if mode == 0 else ((H + 1) // 2, (W + 1) // 2)
    out = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x_nhwc.device)
    _lib.check(lib.rsp_pool2(x_nhwc.data_ptr(), out.data_ptr(), B, H, W, C, mode, _stream()), "rsp_pool2")
    return out


def add_rows(x, v, vmod=None, out=None):
    """x [rows, C] + v[(row % vmod), C]."""
    lib = _lib.load()
    C = x.shape[-1]
    rows = x.numel() // C
    vmod = v.numel() // C if vmod is None else vmod
    out = torch.empty_like(x) if out is None else out
    _lib.check(lib.rsp_add_rows(x.data_ptr(), v.data_ptr(), out.data_ptr(), rows, C, vmod, _stream()),
               "rsp_add_rows")
    return out


def sincos_pairs(x):
    lib = _lib.load()
    out = torch.empty(x.shape[:-1] + (x.shape[-1] // 2,), dtype=torch.float32, device=x.device)
    _lib.check(lib.rsp_sincos_pairs(x.data_ptr(), out.data_ptr(), out.numel(), _stream()), "rsp_sincos_pairs")
    return out


def gather_rows(src, idx):
    lib = _lib.load()
    C = src.shape[-1]
    out = torch.empty((idx.numel(), C), dtype=torch.float32, device=src.device)
    _lib.check(lib.rsp_gather_rows(src.data_ptr(), idx.data_ptr(), out.data_ptr(), idx.numel(), C, _stream()),
               "rsp_gather_rows")
    return out


def hyper_mask(up, hyper):
    """up [R, npix, C], hyper [R, C] -> [R, npix]."""
    lib = _lib.load()
    R, npix, C = up.shape
    out = torch.empty((R, npix), dtype=torch.float32, device=up.device)
    _lib.check(lib.rsp_hyper_mask(up.data_ptr(), hyper.data_ptr(), out.data_ptr(), R, npix, C, _stream()),
               "rsp_hyper_mask")
    return out


def _mask_logits(low_res, who, what="logits", f32=True):
    """(k, h, w) of contiguous fp32 [k, h, w] logits; anything else is a ValueError that names the caller."""
    if f32:
        _chk_f32(low_res, "low_res")
    if low_res.dim() != 3 or not low_res.is_contiguous():
        raise ValueError(f"{who} expects contiguous [k, h, w] {what}")
    return low_res.shape


def _mask_geometry(img_shape, crop_hw, out_hw):
    """Hb, Wb, crop_h, crop_w, out_h, out_w: the geometry arguments of the mask-field entry points."""
    return tuple(int(v) for hw in (img_shape, crop_hw, out_hw) for v in hw[:2])


def _score_thresholds(mask_threshold, stability_score_offset):
    """t_hi, t_lo, t_mid rounded to fp32, as torch rounds the Python scalar when it compares an fp32 tensor with it."""
    return tuple(float(torch.tensor(v, dtype=torch.float32)) for v in
                 (mask_threshold + stability_score_offset, mask_threshold - stability_score_offset, mask_threshold))


def mask_post(low_res, batch_input_shape, crop_hw, out_hw, thr, want_prob=False):
    """low_res [k, h, w] logits -> bool [k, out_h, out_w] (+ optional probabilities)."""
    lib = _lib.load()
    k, h, w = _mask_logits(low_res, "mask_post")
    out = torch.empty((k, out_hw[0], out_hw[1]), dtype=torch.bool, device=low_res.device)
    prob = torch.empty((k, out_hw[0], out_hw[1]), dtype=torch.float32, device=low_res.device) if want_prob else None
    ws = torch.empty_like(low_res)
    _lib.check(lib.rsp_mask_post(low_res.data_ptr(), ws.data_ptr(), k, h, w, *_mask_geometry(batch_input_shape, crop_hw, out_hw),
                                 thr, out.data_ptr(), _ptr(prob), _stream()), "rsp_mask_post")
    return (out, prob) if want_prob else out


def mask_post_logits(low_res, img_shape, crop_hw, out_hw, thr=0.0, want_val=False):
    """SAMDet.predict (models.py:1185-1206): low_res [k, h, w] logits -> bool [k, out_h, out_w] = resized logits > thr."""
    lib = _lib.load()
    k, h, w = _mask_logits(low_res, "mask_post_logits", f32=False)      # the dtype is the caller's business here, as it always was
    out = torch.empty((k, out_hw[0], out_hw[1]), dtype=torch.bool, device=low_res.device)
    val = torch.empty((k, out_hw[0], out_hw[1]), dtype=torch.float32, device=low_res.device) if want_val else None
    _lib.check(lib.rsp_mask_post_logits(low_res.data_ptr(), k, h, w, *_mask_geometry(img_shape, crop_hw, out_hw), thr,
                                        out.data_ptr(), _ptr(val), _stream()), "rsp_mask_post_logits")
    return (out, val) if want_val else out


def resnet_stem(x, w_taps, bias):
    """x [B,3,H,W] fp32 NCHW -> relu(bn(conv7x7 s2 p3)) as NHWC [B,Ho,Wo,64] (resnet.py:640-647)."""
    lib = _lib.load()
    _chk_f32(x, "x")
    if x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise ValueError("resnet_stem expects a contiguous [B,3,H,W] tensor")
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((B, Ho, Wo, 64), dtype=torch.float32, device=x.device)
    _timed('stem_conv_kernel', 2.0 * B * Ho * Wo * 64 * 147, 4.0 * (x.numel() + y.numel()),
           lambda: _lib.check(lib.rsp_resnet_stem(x.data_ptr(), w_taps.data_ptr(), bias.data_ptr(), y.data_ptr(), B, H, W,
                                                  _stream()), "rsp_resnet_stem"))
    return y


def maxpool_nhwc(x, k=3, s=2, p=1):
    lib = _lib.load()
    _chk_f32(x, "x")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("maxpool_nhwc expects a contiguous NHWC tensor")
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    _timed('maxpool_kernel', 0, 4.0 * (x.numel() + y.numel()),
           lambda: _lib.check(lib.rsp_maxpool_nhwc(x.data_ptr(), y.data_ptr(), B, H, W, C, k, s, p, _stream()),
                              "rsp_maxpool_nhwc"))
    return y


def upsample_nearest_add_(dst, src):
    """dst [B,H,W,C] += F.interpolate(src [B,h,w,C], size=(H,W), mode='nearest')  (fpn.py:190-204), in place."""
    lib = _lib.load()
    _chk_f32(dst, "dst"); _chk_f32(src, "src")
    if not (dst.is_contiguous() and src.is_contiguous()) or dst.shape[0] != src.shape[0] or dst.shape[3] != src.shape[3]:
        raise ValueError("upsample_nearest_add_ expects contiguous NHWC tensors of the same batch and channels")
    B, H, W, C = dst.shape
    _timed('upsample_add_kernel', 0, 4.0 * (2 * dst.numel() + src.numel()),
           lambda: _lib.check(lib.rsp_upsample_nearest_add(src.data_ptr(), dst.data_ptr(), B, src.shape[1], src.shape[2], H,
                                                           W, C, _stream()), "rsp_upsample_nearest_add"))
    return dst


def sam_embed_boxes(boxes, gauss, pe_top_left, pe_bottom_right, input_size):
    """boxes [n,4] -> [n, 2, 2F] sparse prompt embeddings (HF SamPromptEncoder._embed_boxes)."""
    lib = _lib.load()
    boxes = boxes.contiguous()
    _chk_f32(boxes, "boxes")
    n, F = boxes.shape[0], gauss.shape[1]
    out = torch.empty((n, 2, 2 * F), dtype=torch.float32, device=boxes.device)
    _lib.check(lib.rsp_sam_embed_boxes(boxes.data_ptr(), gauss.data_ptr(), pe_top_left.data_ptr(),
                                       pe_bottom_right.data_ptr(), out.data_ptr(), n, F, input_size[0], input_size[1],
                                       _stream()), "rsp_sam_embed_boxes")
    return out


def sam_embed_prompts(points, labels, boxes, pad, gauss, point_embed, not_a_point, input_size):
    """HF SamPromptEncoder.forward's sparse half (HF:613-698) for R prompt sets: points [R, P, 2] or None, labels int
    [R, P] (None with points: the bare SamPositionalEmbedding.forward, HF:552-566), boxes [R, 4] or None, `pad` appends the
    padding point (HF: no box given) -> [R, P + pad + 2 * has_boxes, 2F].  point_embed: the four [1, 2F] rows (None in the
    bare mode), not_a_point [1, 2F]; input_size (h, w)."""
    lib = _lib.load()
    if points is None and boxes is None:
        raise ValueError("sam_embed_prompts needs points or boxes")
    ref = points if points is not None else boxes
    R, P = int(ref.shape[0]), 0
    if points is not None:
        points = points.contiguous()
        _chk_f32(points, "points")
        if points.dim() != 3 or points.shape[2] != 2:
            raise ValueError("points: expected [R, P, 2]")
        P = int(points.shape[1])
        if P == 0:
            points = None
    if labels is not None:
        if points is None or tuple(labels.shape) != (R, P):
            raise ValueError("labels: expected [R, P] next to points [R, P, 2]")
        labels = labels.to(torch.int32).contiguous()
    if boxes is not None:
        boxes = boxes.contiguous()
        _chk_f32(boxes, "boxes")
        if tuple(boxes.shape) != (R, 4):
            raise ValueError("boxes: expected [R, 4], one box per prompt set")
    if points is None and boxes is None:
        raise ValueError("sam_embed_prompts needs at least one point or a box per prompt set")
    pad = 1 if pad else 0
    F = gauss.shape[1]
    T = P + pad + (2 if boxes is not None else 0)
    out = torch.empty((R, T, 2 * F), dtype=torch.float32, device=ref.device)
    pe = [None] * 4 if point_embed is None else list(point_embed)
    _lib.check(lib.rsp_sam_embed_prompts(_ptr(points), _ptr(labels), _ptr(boxes), R, P, pad, gauss.data_ptr(), _ptr(pe[0]),
                                         _ptr(pe[1]), _ptr(pe[2]), _ptr(pe[3]), _ptr(not_a_point), out.data_ptr(), F,
                                         int(input_size[0]), int(input_size[1]), _stream()), "rsp_sam_embed_prompts")
    return out


def mask_score_box(low_res, img_shape, crop_hw, out_hw, mask_threshold=0.0, stability_score_offset=1.0):
    """HF mask generation's scores of k candidate masks without the masks: low_res [k, h, w] logits, the geometry of
    mask_post_logits -> int32 [k, 7] = pixel counts above thr + offset, thr - offset and thr, then the box x0, y0, x1, y1
    of the pixels above thr (inclusive maxima, zeros for an empty mask)."""
    lib = _lib.load()
    k, h, w = _mask_logits(low_res, "mask_score_box")
    out = torch.empty((k, 7), dtype=torch.int32, device=low_res.device)
    if k == 0:
        return out
    thr = _score_thresholds(mask_threshold, stability_score_offset)
    _timed('mask_score_kernel', 0, 4.0 * low_res.numel(),
           lambda: _lib.check(lib.rsp_mask_score_box(low_res.data_ptr(), k, h, w, *_mask_geometry(img_shape, crop_hw, out_hw),
                                                     *thr, out.data_ptr(), _stream()), "rsp_mask_score_box"))
    return out


def persam_target(emb_rows, cell_mask):
    """PerSAM's target: emb_rows [N, 256] (the reference's channels-last embedding rows), cell_mask bool / uint8 [N] ->
    (target_embedding fp32 [256] = mean of the selected rows, target_feature fp32 [256] = its unit vector, count int32 [1]),
    all on the device; zeros with an empty selection."""
    lib = _lib.load()
    _chk_f32(emb_rows, "emb_rows")
    if emb_rows.dim() != 2 or emb_rows.shape[1] != 256 or not emb_rows.is_contiguous():
        raise ValueError("persam_target expects contiguous [N, 256] embedding rows")
    N = int(emb_rows.shape[0])
    if cell_mask.dtype not in (torch.bool, torch.uint8) or cell_mask.numel() != N or cell_mask.device != emb_rows.device:
        raise ValueError("cell_mask: bool or uint8 [N] on the device of emb_rows")
    cell = cell_mask.reshape(N).contiguous()
    dev = emb_rows.device
    te = torch.empty((256,), dtype=torch.float32, device=dev)
    tf = torch.empty((256,), dtype=torch.float32, device=dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    _lib.check(lib.rsp_persam_target(emb_rows.data_ptr(), cell.data_ptr(), N, te.data_ptr(), tf.data_ptr(), cnt.data_ptr(),
                                     _stream()), "rsp_persam_target")
    return te, tf, cnt


def persam_similarity(emb_rows, target_feature, B, gh, gw):
    """emb_rows [B * gh * gw, 256], target_feature [256] -> (sim [B, gh * gw] = cosine similarity of every cell with the
    target, low_res [B, 4 gh, 4 gw] = its bilinear x 4 up-sampling: what mask_post_logits / persam_locate take)."""
    lib = _lib.load()
    _chk_f32(emb_rows, "emb_rows")
    _chk_f32(target_feature, "target_feature")
    if emb_rows.dim() != 2 or emb_rows.shape[1] != 256 or emb_rows.shape[0] != B * gh * gw or not emb_rows.is_contiguous():
        raise ValueError(f"persam_similarity expects contiguous [{B * gh * gw}, 256] embedding rows")
    if target_feature.numel() != 256 or not target_feature.is_contiguous():
        raise ValueError("target_feature: contiguous [256]")
    dev = emb_rows.device
    sim = torch.empty((B, gh * gw), dtype=torch.float32, device=dev)
    low = torch.empty((B, 4 * gh, 4 * gw), dtype=torch.float32, device=dev)
    _timed('persam_similarity_kernel', 4.0 * B * gh * gw * 256, 4.0 * B * gh * gw * 256,
           lambda: _lib.check(lib.rsp_persam_similarity(emb_rows.data_ptr(), target_feature.data_ptr(), B, gh, gw, sim.data_ptr(),
                                                        low.data_ptr(), _stream()), "rsp_persam_similarity"))
    return sim, low


def persam_locate(low_res, img_shape, crop_hw, out_hw, g):
    """PerSAM's location prior of k similarity fields without the fields: low_res [k, h, w] and the geometry of
    mask_post_logits -> (stats fp32 [k, 4] = max, min, mean, unbiased std of the [out_h, out_w] field; xy int32 [k, 5] = x, y
    of the maximum, x, y of the minimum -- lowest flat index among equal values --, pixel count; attn_sim fp32 [k, g * g] =
    sigmoid((D - mean) / std) with D the bilinear g x g resampling of the field; 0.5 where std == 0)."""
    lib = _lib.load()
    k, h, w = _mask_logits(low_res, "persam_locate", "fields")
    geom = _mask_geometry(img_shape, crop_hw, out_hw)
    dev = low_res.device
    stats = torch.empty((k, 4), dtype=torch.float32, device=dev)
    xy = torch.empty((k, 5), dtype=torch.int32, device=dev)
    attn = torch.empty((k, g * g), dtype=torch.float32, device=dev)
    if k == 0:
        return stats, xy, attn
    nws = int(lib.rsp_persam_locate_workspace_bytes(k, geom[4], geom[5]))
    if nws < 0:
        raise ValueError(f"persam_locate: unsupported geometry {tuple(out_hw)} for {k} fields")
    ws = torch.empty((nws // 8,), dtype=torch.int64, device=dev)
    _timed('persam_locate_kernel', 0, 4.0 * low_res.numel(),
           lambda: _lib.check(lib.rsp_persam_locate(low_res.data_ptr(), k, h, w, *geom, int(g), ws.data_ptr(), nws, stats.data_ptr(),
                                                    xy.data_ptr(), attn.data_ptr(), _stream()), "rsp_persam_locate"))
    return stats, xy, attn


PERSAM_F_ALPHA = 0.25                      # the focal loss's alpha; gamma = 2 is fixed in the kernel
PERSAM_F_ADAMW = dict(beta1=0.9, beta2=0.999, eps=1e-4, weight_decay=0.01)


def _persam_f_args(low_res, gt, img_shape, crop_hw, out_hw, epochs, who):
    """(k, h, w, geometry, gt as uint8, workspace, bytes) of the PerSAM-F entry points"""
    lib = _lib.load()
    _chk_f32(low_res, "low_res")
    if low_res.dim() != 4 or low_res.shape[1] != 3 or not low_res.is_contiguous() or low_res.shape[0] < 1:
        raise ValueError(f"{who} expects contiguous [k, 3, h, w] logits, k >= 1")
    k, _, h, w = low_res.shape
    geom = _mask_geometry(img_shape, crop_hw, out_hw)
    if gt.dtype not in (torch.bool, torch.uint8) or tuple(gt.shape) != (k, geom[4], geom[5]) or gt.device != low_res.device:
        raise ValueError(f"gt: bool or uint8 [{k}, {geom[4]}, {geom[5]}] on the device of low_res")
    gt = gt.contiguous()
    gt = gt.view(torch.uint8) if gt.dtype == torch.bool else gt
    nws = int(lib.rsp_persam_f_workspace_bytes(k, geom[4], geom[5], int(epochs)))
    if nws < 0:
        raise ValueError(f"{who}: unsupported geometry {tuple(out_hw)} / {epochs} epochs for {k} problems")
    ws = torch.empty((nws // 8,), dtype=torch.int64, device=low_res.device)
    return lib, k, h, w, geom, gt, ws, nws


def persam_f_loss_grad(low_res, gt, img_shape, crop_hw, out_hw, weights, alpha=PERSAM_F_ALPHA):
    """PerSAM-F's loss and its gradient at given weights: low_res [k, 3, h, w] (the three logit maps of one decoder pass per
    problem), gt bool / uint8 [k, out_h, out_w], the geometry of mask_post_logits, weights fp32 [k, 2] = (w1, w2) with
    w0 = 1 - w1 - w2 -> fp64 [k, 3] = dice + focal loss of sigmoid(sum_j w_j field_j) against gt, d loss / d w1, d loss / d w2."""
    lib, k, h, w, geom, gt, ws, nws = _persam_f_args(low_res, gt, img_shape, crop_hw, out_hw, 1, "persam_f_loss_grad")
    _chk_f32(weights, "weights")
    if tuple(weights.shape) != (k, 2) or not weights.is_contiguous():
        raise ValueError(f"weights: contiguous [{k}, 2]")
    out = torch.empty((k, 3), dtype=torch.float64, device=low_res.device)
    _timed('persam_f_sums_kernel', 0, 12.0 * k * h * w + 1.0 * gt.numel(),
           lambda: _lib.check(lib.rsp_persam_f_loss_grad(low_res.data_ptr(), gt.data_ptr(), k, h, w, *geom, weights.data_ptr(),
                                                         float(alpha), ws.data_ptr(), nws, out.data_ptr(), _stream()),
                              "rsp_persam_f_loss_grad"))
    return out


def persam_f_fit(low_res, gt, img_shape, crop_hw, out_hw, epochs=1000, lr=1e-3, alpha=PERSAM_F_ALPHA, want_history=False):
    """PerSAM-F's fit of the mask weights, enqueued whole (nothing is read on the host): from w1 = w2 = 1 / 3, `epochs` steps
    of AdamW(lr, betas=(0.9, 0.999), eps=1e-4, weight_decay=0.01) under CosineAnnealingLR(T_max=epochs) on
    persam_f_loss_grad's loss.  -> weights fp32 [k, 3] = w0, w1, w2 (and, with want_history, fp64 [k, epochs, 3] = the loss
    and gradient each step was taken from)."""
    epochs = int(epochs)
    if epochs < 1:
        raise ValueError("persam_f_fit: epochs must be >= 1")
    lib, k, h, w, geom, gt, ws, nws = _persam_f_args(low_res, gt, img_shape, crop_hw, out_hw, epochs, "persam_f_fit")
    dev = low_res.device
    weights = torch.empty((k, 3), dtype=torch.float32, device=dev)
    hist = torch.empty((k, epochs, 3), dtype=torch.float64, device=dev) if want_history else None
    o = PERSAM_F_ADAMW
    _timed('persam_f_fit', 0, epochs * (12.0 * k * h * w + 1.0 * gt.numel()),
           lambda: _lib.check(lib.rsp_persam_f_fit(low_res.data_ptr(), gt.data_ptr(), k, h, w, *geom, epochs, float(lr), o['beta1'],
                                                   o['beta2'], o['eps'], o['weight_decay'], float(alpha), ws.data_ptr(), nws,
                                                   weights.data_ptr(), _ptr(hist), _stream()), "rsp_persam_f_fit"))
    return (weights, hist) if want_history else weights


CROP_TABLE_COLS = CONST['RSP_CROP_TABLE_COLS']    # rsp_mask_score_box_crops: Hb, Wb, crop_h, crop_w, out_h, out_w, x0, y0, x1, y1, W, H


def mask_score_box_crops(low_res, crop_idx, table, max_out_hw, mask_threshold=0.0, stability_score_offset=1.0,
                         check_index=True):
    """mask_score_box for the candidates of several crops in one call (rsp_mask_score_box_crops): low_res [K, h, w] logits,
    crop_idx int32 [K] (the crop of each candidate) and table int32 [n_crops, 12] = (Hb, Wb, crop_h, crop_w, out_h, out_w,
    x0, y0, x1, y1, W, H) per crop, both on the device of low_res; max_out_hw: the largest out_h and out_w of the table.
    Returns int32 [K, 8]: the three counts of mask_score_box on that crop's geometry, its box shifted into the image frame
    by (x0, y0, x0, y0), and HF `_is_box_near_crop_edge` (atol 20) of that box.  check_index reads crop_idx's extrema on the
    host and refuses an index outside the table; a caller that built the index itself passes False (no host read; the
    kernel clamps)."""
    lib = _lib.load()
    K, h, w = _mask_logits(low_res, "mask_score_box_crops")
    dev = low_res.device
    if crop_idx.dtype != torch.int32 or crop_idx.dim() != 1 or crop_idx.shape[0] != K or crop_idx.device != dev:
        raise ValueError("crop_idx: int32 [K] on the device of low_res")
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != CROP_TABLE_COLS or table.shape[0] < 1 or \
            table.device != dev:
        raise ValueError(f"table: int32 [n_crops, {CROP_TABLE_COLS}] on the device of low_res")
    out = torch.empty((K, 8), dtype=torch.int32, device=dev)
    if K == 0:
        return out
    n_crops = int(table.shape[0])
    if check_index:
        lo, hi = int(crop_idx.min().item()), int(crop_idx.max().item())
        if lo < 0 or hi >= n_crops:
            raise ValueError(f"crop_idx holds {lo} .. {hi}, the table has {n_crops} rows")
    crop_idx, table = crop_idx.contiguous(), table.contiguous()
    thr = _score_thresholds(mask_threshold, stability_score_offset)
    _timed('mask_score_crops_kernel', 0, 4.0 * low_res.numel(),
           lambda: _lib.check(lib.rsp_mask_score_box_crops(low_res.data_ptr(), K, h, w, crop_idx.data_ptr(), table.data_ptr(),
                                                           n_crops, int(max_out_hw[0]), int(max_out_hw[1]), *thr, out.data_ptr(),
                                                           _stream()), "rsp_mask_score_box_crops"))
    return out


def box_coder(coder):
    """The RspBoxCoder of a DeltaXYWHBBoxCoder-like object (`means`, `stds`, `max_ratio`, `clip_border`, `add_ctr_clamp`,
    `ctr_clamp`: delta_xywh_bbox_coder.py:71-131)."""
    c = _lib.RspBoxCoder()
    for i in range(4):
        c.means[i], c.stds[i] = float(coder.means[i]), float(coder.stds[i])
    c.max_ratio, c.ctr_clamp = float(coder.max_ratio), float(coder.ctr_clamp)
    c.clip_border, c.add_ctr_clamp = int(bool(coder.clip_border)), int(bool(coder.add_ctr_clamp))
    return c


class RpnSelector:
    """rpn_topk -> rpn_decode -> batched_nms on the device (rpn_head.py:134-304)."""

    def __init__(self, base_anchors, strides, nms_pre, max_per_img, iou_thr, min_bbox_size, coder, device):
        self.base = base_anchors.to(torch.float32).contiguous().to(device)   # [L, A, 4]
        self.strides = list(strides)
        self.L, self.A = self.base.shape[0], self.base.shape[1]
        self.nms_pre, self.max_per_img, self.iou_thr = nms_pre, max_per_img, iou_thr
        self.min_bbox_size, self.coder = min_bbox_size, box_coder(coder)

    def __call__(self, heads, sizes, ld, img_hw):
        """heads: per-level [B*H*W, ld] outputs; sizes: [(H, W)]; img_hw: device [B, 2] float."""
        lib = _lib.load()
        dev = heads[0].device
        B = img_hw.shape[0]
        d = _lib.RspRpnDesc()
        for i, (hd, (H, W)) in enumerate(zip(heads, sizes)):
            d.head[i] = hd.data_ptr()
            d.H[i], d.W[i], d.stride[i] = H, W, float(self.strides[i])
        d.ld, d.A, d.nms_pre, d.num_levels = ld, self.A, self.nms_pre, len(heads)
        d.base_anchors = self.base.data_ptr()
        d.coder, d.min_bbox_size = self.coder, float(self.min_bbox_size)
        L, k = len(heads), self.nms_pre
        sel_idx = torch.empty((B, L, k), dtype=torch.int32, device=dev)
        sel_score = torch.empty((B, L, k), dtype=torch.float32, device=dev)
        sel_cnt = torch.empty((B, L), dtype=torch.int32, device=dev)
        _lib.check(lib.rsp_rpn_topk(d, B, sel_idx.data_ptr(), sel_score.data_ptr(), sel_cnt.data_ptr(),
                                    _stream()), "rsp_rpn_topk")
        cap = L * k
        cand = _cand_buffers(B, cap, dev)
        _lib.check(lib.rsp_rpn_decode(d, B, sel_idx.data_ptr(), sel_score.data_ptr(), sel_cnt.data_ptr(),
                                      img_hw.data_ptr(), cap, *[c.data_ptr() for c in cand], _stream()),
                   "rsp_rpn_decode")
        return batched_nms(cand, B, cap, self.iou_thr, self.max_per_img)


NMS_LDS_CANDIDATES = CONST['RSP_NMS_LDS_CANDIDATES']     # rsp_batched_nms sorts up to here in LDS, in memory above
NMS_MAX_CANDIDATES = CONST['RSP_NMS_MAX_CANDIDATES']    # ... and holds this many candidates per image at most
# the pair mask of the in-memory path is quadratic: B * cap * cap / 8 bytes (200 MB per image at 40 k candidates, 2 GiB at
# the kernel's limit).  A call that would need more than this many bytes of workspace is refused with the figures in the
# message instead of failing inside the allocator (settable: a box with spare HBM may raise it).
NMS_WORKSPACE_LIMIT_BYTES = 8 << 30


def _cand_buffers(B, cap, dev):
    return (torch.empty((B, cap, 4), dtype=torch.float32, device=dev),
            torch.empty((B, cap), dtype=torch.float32, device=dev),
            torch.empty((B, cap), dtype=torch.int32, device=dev),
            torch.empty((B, cap), dtype=torch.int32, device=dev),
            torch.empty((B,), dtype=torch.int32, device=dev))


def batched_nms(cand, B, cap, iou_thr, max_out):
    """cand = (boxes [B,cap,4], scores, ids, src, cnt).  returns dict of [B, max_out] outputs + counts."""
    lib = _lib.load()
    boxes, scores, ids, src, cnt = cand
    dev = boxes.device
    ws_bytes = int(lib.rsp_nms_workspace_bytes(B, cap))
    if ws_bytes > NMS_WORKSPACE_LIMIT_BYTES:
        raise ValueError(f'batched_nms: {B} images x {cap} candidates need a {ws_bytes / 2 ** 30:.1f} GiB pair mask '
                         f'(limit ops.NMS_WORKSPACE_LIMIT_BYTES = {NMS_WORKSPACE_LIMIT_BYTES / 2 ** 30:.0f} GiB): raise score_thr, '
                         'lower the number of proposals, or run fewer images per call')
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    keep = torch.empty((B, max_out), dtype=torch.int32, device=dev)
    keep_cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    ob = torch.empty((B, max_out, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((B, max_out), dtype=torch.float32, device=dev)
    oi = torch.empty((B, max_out), dtype=torch.int32, device=dev)
    osrc = torch.empty((B, max_out), dtype=torch.int32, device=dev)
    _lib.check(lib.rsp_batched_nms(boxes.data_ptr(), scores.data_ptr(), ids.data_ptr(), src.data_ptr(),
                                   cnt.data_ptr(), B, cap, iou_thr, max_out, ws.data_ptr(), keep.data_ptr(),
                                   keep_cnt.data_ptr(), ob.data_ptr(), os_.data_ptr(), oi.data_ptr(),
                                   osrc.data_ptr(), _stream()), "rsp_batched_nms")
    return dict(boxes=ob, scores=os_, ids=oi, src=osrc, count=keep_cnt, keep=keep, cand_count=cnt)


def bbox_post(head, ld, rois, roi_start, img_hw, num_classes, score_thr, coder, iou_thr, max_out,
              scale_factors=None):
    """R-CNN head post-processing + multiclass NMS (bbox_head.py:476-571, bbox_nms.py:12-105).
    scale_factors: per image (w, h) -- `rescale=True` (bbox_head.py:549-554): the decoded, clipped boxes are divided by the
    scale factor BEFORE the NMS, as the reference does."""
    import ctypes
    lib = _lib.load()
    dev = head.device
    B = img_hw.shape[0]
    n_max = int((roi_start[1:] - roi_start[:-1]).max()) if roi_start.numel() > 1 else 0
    cap = max(n_max * num_classes, 1)
    cand = _cand_buffers(B, cap, dev)
    rs = roi_start.to(device=dev, dtype=torch.int32)
    _lib.check(lib.rsp_bbox_post(head.data_ptr(), ld, rois.data_ptr(), rs.data_ptr(), img_hw.data_ptr(), B,
                                 num_classes, score_thr, ctypes.byref(box_coder(coder)), cap, *[c.data_ptr() for c in cand],
                                 _stream()), "rsp_bbox_post")
    if cap > NMS_LDS_CANDIDATES:
        # many classes (the RSPrompter datasets have 1 or 10: never here): size the NMS by the candidates that passed the
        # score threshold -- one host sync -- instead of by RoIs x classes; its pair mask is quadratic in that size
        cmax = max(int(cand[4].max()), 1)
        if cmax > NMS_MAX_CANDIDATES:
            raise ValueError(f'bbox_post: {cmax} of {n_max} RoIs x {num_classes} classes passed score_thr={score_thr}; '
                             f'rsp_batched_nms holds {NMS_MAX_CANDIDATES} candidates per image (det.hip NMS_MAXW_LARGE)')
        if cmax < cap:
            cand = tuple(c[:, :cmax].contiguous() for c in cand[:4]) + (cand[4],)
            cap = cmax
    if scale_factors is not None:
        for b, sf in enumerate(scale_factors):
            inv = (1 / float(sf[0]), 1 / float(sf[1]))          # bbox_head.py:550: python reciprocal, then an fp32 product
            arr = (ctypes.c_float * 4)(inv[0], inv[1], inv[0], inv[1])
            bx = cand[0][b]
            _lib.check(lib.rsp_scale_boxes(bx.data_ptr(), bx.data_ptr(), bx.shape[0], arr, _stream()), "rsp_scale_boxes")
    return batched_nms(cand, B, cap, iou_thr, max_out)


def div_boxes(boxes, sf4):
    """boxes [k,4] / (sf_w, sf_h, sf_w, sf_h)."""
    import ctypes
    lib = _lib.load()
    boxes = boxes.contiguous()
    out = torch.empty_like(boxes)
    arr = (ctypes.c_float * 4)(*[float(v) for v in sf4])
    _lib.check(lib.rsp_div_boxes(boxes.data_ptr(), out.data_ptr(), boxes.shape[0], arr, _stream()), "rsp_div_boxes")
    return out


def fill_bias_rows(bias, rows, N, out=None, planes=None, c_ncols=0, pl_col0=0):
    """rows (int32 indices) of a GEMM output the GEMM did not write because their A row is zero (window padding): fp32
    columns [0, c_ncols or N) of `out` = bias, plane columns [pl_col0, N) = split(bias)  (HF:913-915: qkv(0) = bias)."""
    lib = _lib.load()
    n = int(rows.shape[0])
    if n == 0:
        return
    _lib.check(lib.rsp_fill_bias_rows(_ptr(bias), rows.data_ptr(), n, N, _ptr(out), out.stride(0) if out is not None else 0,
                                      c_ncols, planes.hi.data_ptr() if planes is not None else None,
                                      planes.lo.data_ptr() if planes is not None else None,
                                      planes.rows if planes is not None else 0, pl_col0,
                                      planes.word if planes is not None else 0, _stream()), "rsp_fill_bias_rows")


def scale_boxes(boxes, f4):
    """boxes [k,4] * (f0, f1, f2, f3) in fp32 (scale_boxes, structures/bbox/transforms.py:391-414)."""
    import ctypes
    lib = _lib.load()
    boxes = boxes.contiguous()
    out = torch.empty_like(boxes)
    arr = (ctypes.c_float * 4)(*[float(v) for v in f4])
    _lib.check(lib.rsp_scale_boxes(boxes.data_ptr(), out.data_ptr(), boxes.shape[0], arr, _stream()), "rsp_scale_boxes")
    return out


def pack_masks(masks):
    """bool [k, H, W] -> uint8 [k, H*W/8] (bit i of byte j = pixel 8j+i)."""
    lib = _lib.load()
    k = masks.shape[0]
    n = masks[0].numel() if k else 0
    if n % 8:
        raise ValueError('mask area must be a multiple of 8')
    out = torch.empty((k, n // 8), dtype=torch.uint8, device=masks.device)
    if k:
        m = masks.contiguous()
        _lib.check(lib.rsp_pack_bits(m.data_ptr(), out.data_ptr(), m.numel(), _stream()), "rsp_pack_bits")
    return out


def grown_cap(need):
    """the run capacity to retry with when a producer reported n[i] = -need: the next power of two"""
    return 1 << (int(need) - 1).bit_length()


def fit_runs(launch, cap):
    """The capacity protocol of the run-table producers (rsp_mask_rle, rsp_rle_from_string, rsp_rle_shift, rsp_rle_union:
    counts int32 [k, cap] + n int32 [k], n[i] = -(slots needed) for a row that did not fit).  `launch(cap)` enqueues one
    producer and returns (counts, n); one device-to-host read of n per attempt, again at grown_cap(the largest need)
    until every row fits (an empty n fits) -> (counts, n, n on the host, cap)."""
    while True:
        counts, n = launch(cap)
        n_host = n.cpu()
        need = int(-n_host.min()) if n_host.numel() else 0
        if need <= 0:
            return counts, n, n_host, cap
        cap = grown_cap(need)


def mask_rle_launcher(masks):
    """the `launch(cap)` of fit_runs for rsp_mask_rle on bool [k, H, W]: fresh [k, cap] buffers, no host read"""
    k, dev = masks.shape[0], masks.device

    def launch(cap):
        counts = torch.empty((k, cap), dtype=torch.int32, device=dev)
        ws = torch.empty((k, cap), dtype=torch.int32, device=dev)
        n = torch.empty((k,), dtype=torch.int32, device=dev)
        mask_rle_into(masks, counts, ws, n)
        return counts, n
    return launch


def mask_rle_counts(masks, cap=4096):
    """bool [k, H, W] -> (counts int32 [k, cap'], n int32 [k]): COCO RLE run lengths (column-major stream, first run
    counts zeros).  Retries with a larger capacity when a mask has more runs than `cap`."""
    return fit_runs(mask_rle_launcher(masks), cap)[:2]


def mask_rle_into(masks, counts, ws, n):
    """rsp_mask_rle into rows of preallocated buffers (counts / ws int32 [k, cap], n int32 [k]); nothing here touches
    the host: n[i] < 0 reports a mask with more than cap runs (-needed), checked by whoever reads n later."""
    lib = _lib.load()
    k, H, W = masks.shape
    if k:
        m = masks.contiguous()
        _lib.check(lib.rsp_mask_rle(m.data_ptr(), k, H, W, ws.data_ptr(), counts.data_ptr(), n.data_ptr(),
                                    counts.shape[1], _stream()), "rsp_mask_rle")


def rle_to_string(counts, n, k, flat_cap):
    """COCO ASCII strings of k run-length lists (rsp_rle_to_string): returns (lens int32 [k], offs int64 [k + 1],
    flat uint8 [flat_cap]) on the device, no host synchronisation; strings beyond flat_cap are not written
    (offs[k] > flat_cap tells)."""
    lib = _lib.load()
    dev = counts.device
    lens = torch.zeros((max(k, 1),), dtype=torch.int32, device=dev)
    offs = torch.zeros((k + 1,), dtype=torch.int64, device=dev)
    flat = torch.empty((max(int(flat_cap), 1),), dtype=torch.uint8, device=dev)
    _lib.check(lib.rsp_rle_to_string(counts.data_ptr(), n.data_ptr(), k, counts.shape[1], lens.data_ptr(),
                                     offs.data_ptr(), flat.data_ptr(), int(flat_cap), _stream()), "rsp_rle_to_string")
    return lens, offs, flat


# ----------------------------------------------------------------------------- large scenes (csrc/large_image.hip)
def slice_resize_pad(scene_hwc, origins, tile_hw, new_hw, pad_hw, pad_val=(0.0, 0.0, 0.0), out=None, normalise=None):
    """B tiles of a device-resident scene [H, W, 3] (uint8 / fp32) -> fp32 [B, 3, Hp, Wp], one launch
    (rsp_slice_resize_pad).  origins: int32 [B, 2] = (x0, y0) on the device; tile i is bit-identical to
    `resize_pad(scene[y0:y0 + th, x0:x0 + tw].contiguous(), new_hw, pad_hw, pad_val, normalise=normalise)`."""
    import ctypes
    lib = _lib.load()
    if scene_hwc.dim() != 3 or scene_hwc.shape[2] != 3 or not _is_device(scene_hwc):
        raise ValueError('slice_resize_pad expects an [H, W, 3] device tensor')
    im = scene_hwc.contiguous()
    if im.dtype != torch.uint8:
        im = im.to(torch.float32)
    if origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 2 or origins.device != im.device:
        raise ValueError('origins: int32 [B, 2] = (x0, y0) on the device of the scene')
    origins = origins.contiguous()
    B = int(origins.shape[0])
    SH, SW = int(im.shape[0]), int(im.shape[1])
    th, tw = int(tile_hw[0]), int(tile_hw[1])
    Hn, Wn = int(new_hw[0]), int(new_hw[1])
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    if out is None:
        out = torch.empty((B, 3, Hp, Wp), dtype=torch.float32, device=im.device)
    p3 = (ctypes.c_float * 3)(*[float(v) for v in pad_val])
    if normalise is None:
        m3 = s3 = None
        nrm, swap = 0, 0
    else:
        m3 = (ctypes.c_float * 3)(*[float(v) for v in normalise[0]])
        s3 = (ctypes.c_float * 3)(*[float(v) for v in normalise[1]])
        nrm, swap = 1, 1 if normalise[2] else 0
    _lib.check(lib.rsp_slice_resize_pad(im.data_ptr(), 1 if im.dtype == torch.uint8 else 0, SH, SW, origins.data_ptr(), B,
                                        th, tw, out.data_ptr(), Hn, Wn, Hp, Wp, p3, nrm, swap, m3, s3, _stream()),
               "rsp_slice_resize_pad")
    return out


def crops_resize_pad(image_hwc, table, pad_hw, pad_val=(0.0, 0.0, 0.0), out=None, normalise=None):
    """B crops of DIFFERENT sizes of a device-resident image [H, W, 3] (uint8 / fp32) -> fp32 [B, 3, Hp, Wp], one launch
    (rsp_crops_resize_pad).  table: int32 [B, 6] = (x0, y0, x1, y1, Hn, Wn) on the device; crop i is bit-identical to
    `resize_pad(image[y0:y1, x0:x1].contiguous(), (Hn, Wn), pad_hw, pad_val, normalise=normalise)`."""
    import ctypes
    lib = _lib.load()
    if image_hwc.dim() != 3 or image_hwc.shape[2] != 3 or not _is_device(image_hwc):
        raise ValueError('crops_resize_pad expects an [H, W, 3] device tensor')
    im = image_hwc.contiguous()
    if im.dtype != torch.uint8:
        im = im.to(torch.float32)
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 6 or table.device != im.device:
        raise ValueError('table: int32 [B, 6] = (x0, y0, x1, y1, Hn, Wn) on the device of the image')
    table = table.contiguous()
    B = int(table.shape[0])
    Hp, Wp = int(pad_hw[0]), int(pad_hw[1])
    if out is None:
        out = torch.empty((B, 3, Hp, Wp), dtype=torch.float32, device=im.device)
    if B == 0:
        return out
    p3 = (ctypes.c_float * 3)(*[float(v) for v in pad_val])
    if normalise is None:
        m3 = s3 = None
        nrm, swap = 0, 0
    else:
        m3 = (ctypes.c_float * 3)(*[float(v) for v in normalise[0]])
        s3 = (ctypes.c_float * 3)(*[float(v) for v in normalise[1]])
        nrm, swap = 1, 1 if normalise[2] else 0
    _lib.check(lib.rsp_crops_resize_pad(im.data_ptr(), 1 if im.dtype == torch.uint8 else 0, int(im.shape[0]), int(im.shape[1]),
                                        table.data_ptr(), B, out.data_ptr(), Hp, Wp, p3, nrm, swap, m3, s3, _stream()),
               "rsp_crops_resize_pad")
    return out


def rle_shift(counts, n, offsets, tile_hw, scene_hw, cap_out):
    """run counts of k tile-sized masks (counts int32 [k, cap], n int32 [k], as mask_rle_into writes them) -> run counts
    of the same masks placed at offsets (int32 [k, 2] = (ox, oy), device) in an (H, W) scene: (counts_out int32
    [k, cap_out], n_out int32 [k]); n_out[i] = -(needed) when cap_out is too small.  No host synchronisation."""
    lib = _lib.load()
    k = int(n.shape[0])
    H, W = int(scene_hw[0]), int(scene_hw[1])
    if H * W >= 2 ** 31:
        raise ValueError(f'rle_shift: a {H} x {W} scene has {H * W} pixels; COCO run counts are 32-bit (< 2^31 pixels)')
    dev = n.device
    counts = counts.contiguous()
    out = torch.empty((max(k, 1), int(cap_out)), dtype=torch.int32, device=dev)
    n_out = torch.zeros((max(k, 1),), dtype=torch.int32, device=dev)
    if k:
        _lib.check(lib.rsp_rle_shift(counts.data_ptr(), n.contiguous().data_ptr(), k, counts.shape[1],
                                     offsets.contiguous().data_ptr(), int(tile_hw[0]), int(tile_hw[1]), H, W,
                                     out.data_ptr(), n_out.data_ptr(), int(cap_out), _stream()), "rsp_rle_shift")
    return out[:k], n_out[:k]


def paste_tiles(masks, offsets, scene_hw):
    """bool [k, h, w] tile masks at offsets (int32 [k, 2] = (ox, oy), device) -> bool [k, H, W] (sahi shift_masks)."""
    lib = _lib.load()
    k, h, w = masks.shape
    H, W = int(scene_hw[0]), int(scene_hw[1])
    out = torch.empty((k, H, W), dtype=torch.bool, device=masks.device)
    for i in range(0, k, 65535):
        m = masks[i:i + 65535].contiguous()
        _lib.check(lib.rsp_paste_tiles(m.data_ptr(), offsets[i:i + 65535].contiguous().data_ptr(), m.shape[0], h, w, H, W,
                                       out[i:i + 65535].data_ptr(), _stream()), "rsp_paste_tiles")
    return out


# ----------------------------------------------------------------------------- seam merge (csrc/seam_merge.hip)
def _rle_rows(what, counts, n, H=None, W=None):
    """the common checks of the run-domain entry points: counts int32 [k, cap] / n int32 [k], on one (H, W) canvas where
    the entry point takes one -> (counts, n, k, cap, H, W)"""
    if H is not None:
        H, W = int(H), int(W)
        if H * W >= 2 ** 31:
            raise ValueError(f'{what}: a {H} x {W} scene has {H * W} pixels; COCO run counts are 32-bit (< 2^31 pixels)')
        if H < 1 or W < 1:
            raise ValueError(f'{what}: an empty {H} x {W} canvas')
    if counts.dtype != torch.int32 or counts.dim() != 2 or n.dtype != torch.int32 or n.dim() != 1 \
            or n.shape[0] != counts.shape[0] or counts.shape[1] < 1 or n.device != counts.device:
        raise ValueError(f'{what}: expected counts int32 [k, cap >= 1] and n int32 [k] on one device')
    return counts.contiguous(), n.contiguous(), int(n.shape[0]), int(counts.shape[1]), H, W


def _exclusive_total(cnt):
    """counts along the last dimension -> (exclusive sum int64 [..., len + 1], its last entries still on the device)"""
    offs = torch.cat([cnt.new_zeros(cnt.shape[:-1] + (1,), dtype=torch.int64), torch.cumsum(cnt, -1, dtype=torch.int64)], -1)
    return offs.contiguous(), offs[..., -1]


def _rle_intervals(lib, counts, n, k, cap, H, W, members, group_of, runs, total=None):
    """rsp_rle_intervals: the ones-runs of M member rows (`runs` int64 [M] of them each) as (group << 31 | pixel start, end)
    intervals -> (keys int64, ends int32, offs int64 [M + 1] = the first slot of every member, total).  total=None: their
    number is read from the device (one host read); a bound given instead reads nothing.  total == 0: no launch, no arrays."""
    ends_incl = torch.cumsum(runs, 0)
    moff = (ends_incl - runs).contiguous()
    offs = torch.cat([ends_incl.new_zeros((1,)), ends_incl]).contiguous()
    total = int(ends_incl[-1].item()) if total is None else total
    if total == 0:
        return None, None, offs, 0
    keys = torch.empty((total,), dtype=torch.int64, device=n.device)
    ends = torch.empty((total,), dtype=torch.int32, device=n.device)
    _lib.check(lib.rsp_rle_intervals(counts.data_ptr(), n.data_ptr(), k, cap, H, W, members.data_ptr(), group_of.data_ptr(),
                                     moff.data_ptr(), int(members.shape[0]), total, keys.data_ptr(), ends.data_ptr(), _stream()),
               "rsp_rle_intervals")
    return keys, ends, offs, total


def _intervals_to_runs(lib, keys, ends, total, iv_offs, G, H, W, cap_out):
    """rsp_rle_union, the one step from intervals sorted by key to a run table: the first `total` of keys / ends (None
    when there are none), iv_offs int64 [G + 1] -> (counts_out int32 [G, cap_out], n_out int32 [G]), n_out = -(needed) for
    a row that does not fit (the protocol of fit_runs).  No host read."""
    dev = iv_offs.device
    out = torch.empty((G, int(cap_out)), dtype=torch.int32, device=dev)
    n_out = torch.zeros((G,), dtype=torch.int32, device=dev)
    if G and total == 0:                                             # the entry point takes arrays of one slot at least
        keys, ends = torch.empty((1,), dtype=torch.int64, device=dev), torch.empty((1,), dtype=torch.int32, device=dev)
    if G:
        _lib.check(lib.rsp_rle_union(keys.data_ptr(), ends.data_ptr(), total, iv_offs.data_ptr(), G, H, W, out.data_ptr(),
                                     n_out.data_ptr(), int(cap_out), _stream()), "rsp_rle_union")
    return out, n_out


def _rle_index(what, name, t, cols, dev):
    if t.dtype != torch.int32 or t.device != dev or (t.dim() != 2 or t.shape[1] != cols if cols else t.dim() != 1):
        raise ValueError(f'{what}: {name} must be int32 {"[P, %d]" % cols if cols else "[n]"} on the device of the counts')
    return t.contiguous()


def rle_bbox(counts, n, H, W):
    """scene-frame run counts (as rle_shift returns them) -> (boxes int32 [k, 4] = tight (x0, y0, x1, y1), end-exclusive,
    zeros for an empty mask; area int32 [k]): maskUtils.toBbox / area in the run domain (rsp_rle_bbox).  No host read."""
    lib = _lib.load()
    counts, n, k, cap, H, W = _rle_rows('rle_bbox', counts, n, H, W)
    boxes = torch.zeros((k, 4), dtype=torch.int32, device=n.device)
    area = torch.zeros((k,), dtype=torch.int32, device=n.device)
    if k:
        _lib.check(lib.rsp_rle_bbox(counts.data_ptr(), n.data_ptr(), k, cap, H, W, boxes.data_ptr(), area.data_ptr(),
                                    _stream()), "rsp_rle_bbox")
    return boxes, area


def rle_pair_overlap(counts, n, H, W, pairs, rects):
    """for P pairs of rows (pairs int32 [P, 2], device) and rectangles (rects int32 [P, 4] = (x0, y0, x1, y1),
    end-exclusive, device): int32 [P, 3] = (|M_i & M_j|, |M_i & R|, |M_j & R|) (rsp_rle_pair_overlap); the intersection is
    NOT clipped to the rectangle.  No host read."""
    lib = _lib.load()
    counts, n, k, cap, H, W = _rle_rows('rle_pair_overlap', counts, n, H, W)
    pairs = _rle_index('rle_pair_overlap', 'pairs', pairs, 2, n.device)
    rects = _rle_index('rle_pair_overlap', 'rects', rects, 4, n.device)
    P = int(pairs.shape[0])
    if rects.shape[0] != P:
        raise ValueError('rle_pair_overlap: one rectangle per pair')
    out = torch.zeros((P, 3), dtype=torch.int32, device=n.device)
    if P and k:
        ws = torch.empty((int(lib.rsp_rle_pair_overlap_workspace_bytes(k, cap)) // 4,), dtype=torch.int32, device=n.device)
        _lib.check(lib.rsp_rle_pair_overlap(counts.data_ptr(), n.data_ptr(), k, cap, H, W, pairs.data_ptr(), rects.data_ptr(),
                                            P, ws.data_ptr(), out.data_ptr(), _stream()), "rsp_rle_pair_overlap")
    return out


def rle_union(counts, n, H, W, group_offs, members, cap_out):
    """the union of the member rows of G groups (group_offs int32 [G + 1], members int32 [M] row indices, groups
    contiguous, group_offs[0] = 0, group_offs[G] = M; both on the device) as canonical COCO run counts: (counts_out int32 [G, cap_out], n_out int32 [G]), n_out =
    -(needed) when cap_out is too small.  rsp_rle_intervals -> a device key sort of (group, start) -> rsp_rle_union.  One
    host read (the number of intervals, which sizes the sort)."""
    lib = _lib.load()
    counts, n, k, cap, H, W = _rle_rows('rle_union', counts, n, H, W)
    dev = n.device
    group_offs = _rle_index('rle_union', 'group_offs', group_offs, 0, dev)
    members = _rle_index('rle_union', 'members', members, 0, dev)
    G, M = int(group_offs.shape[0]) - 1, int(members.shape[0])
    if G < 0 or int(cap_out) < 2:
        raise ValueError('rle_union: group_offs holds G + 1 entries and cap_out is at least 2')
    if G and M and k:
        go = group_offs.to(torch.int64).clamp(0, M)
        inside = (members >= 0) & (members < k)
        runs = torch.where(inside, n[members.to(torch.int64).clamp(0, k - 1)].clamp(0, cap) // 2, 0).to(torch.int64)
        # the group of member mi: the last g with group_offs[g] <= mi (group_offs[0] = 0, group_offs[G] = M)
        group_of = torch.searchsorted(go[1:].contiguous(), torch.arange(M, dtype=torch.int64, device=dev), right=True)
        group_of = group_of.clamp(max=G - 1).to(torch.int32).contiguous()
        keys, ends, moffs, total = _rle_intervals(lib, counts, n, k, cap, H, W, members, group_of, runs)
        iv_offs = moffs[go].contiguous()
        if total:
            keys, order = torch.sort(keys)
            ends = ends[order].contiguous()
    else:
        keys, ends, total, iv_offs = None, None, 0, torch.zeros((G + 1,), dtype=torch.int64, device=dev)
    return _intervals_to_runs(lib, keys, ends, total, iv_offs, G, H, W, cap_out)


# ----------------------------------------------------------------------------- column pieces (csrc/run_pieces.hip)
RUN_PIECES_MAX_PIECES = CONST['RSP_RUN_PIECES_MAX_PIECES']          # column pieces of one call: 32-bit piece indices
RunPieces = collections.namedtuple('RunPieces', 'pieces piece_offs P widest')


def run_pieces(counts, n, H, W, *, what='run_pieces', limit=RUN_PIECES_MAX_PIECES):
    """run table (counts int32 [k, cap], n int32 [k]: k masks on one (H, W) canvas) -> its column-piece table, which polygon
    export and the components read, as RunPieces: pieces int32 [4, P] = (x, y0, y1, instance) of every ones-run
    cut at column ends, sorted by (instance, x, y0); piece_offs int64 [k + 1]; on the host P and `widest`, the pieces of the
    largest row.  A row with n <= 0 has none.  One device-to-host read (P with widest); k == 0 or P == 0 launches no write.
    what, limit: the entry point that asks, for the messages, and the most pieces it takes in one call."""
    lib = _lib.load()
    counts, n, k, cap, H, W = _rle_rows(what, counts, n, H, W)
    i32, i64 = dict(dtype=torch.int32, device=n.device), dict(dtype=torch.int64, device=n.device)
    if k == 0:
        return RunPieces(torch.zeros((4, 0), **i32), torch.zeros((1,), **i64), 0, 0)
    piece_cnt = torch.zeros((k,), **i32)
    _lib.check(lib.rsp_run_pieces_count(counts.data_ptr(), n.data_ptr(), k, cap, H, W, piece_cnt.data_ptr(), _stream()),
               "rsp_run_pieces_count")
    piece_offs, total = _exclusive_total(piece_cnt)
    P, widest = torch.stack([total, piece_cnt.max().to(torch.int64)]).tolist()                    # the read
    if P > limit:
        raise ValueError(f'{what}: {P} column pieces in one call; at most {limit} (split the rows)')
    pieces = torch.empty((4, P), **i32)
    if P:
        _lib.check(lib.rsp_run_pieces(counts.data_ptr(), n.data_ptr(), k, cap, H, W, piece_offs.data_ptr(), P, pieces.data_ptr(),
                                      _stream()), "rsp_run_pieces")
    return RunPieces(pieces, piece_offs, P, widest)


# ----------------------------------------------------------------------------- polygon export (csrc/mask_polygons.hip)
MASK_POLYGON_MAX_PIECES = CONST['RSP_MASK_POLYGON_MAX_PIECES']     # six edge slots per column piece, 32-bit slot numbers


def _log2_ceil(v):
    return max(int(v) - 1, 0).bit_length()


def mask_polygons(counts, n, H, W):
    """run table (counts int32 [k, cap], n int32 [k]: k masks on one (H, W) canvas) -> the rings of every mask on the
    pixel-corner lattice, all on the device:
      verts int32 [V, 2] = (x, y), ring_offs int64 [R + 1], ring_inst int32 [R], ring_parent int32 [R] (-1: outer ring, else the
      index within the instance of the outer ring around the hole), ring_area2 int64 [R] (> 0 outer, < 0 hole),
      inst_ring_offs int64 [k + 1].
    Rings are ordered by (instance, first vertex); a ring starts at its smallest vertex by (x, y), holds corners only and does
    not repeat its first vertex.  A row with n <= 0 has no rings.  Three device-to-host reads, whatever k is: the pieces
    (total and largest row), the number of rings (inside torch.nonzero), the number of vertices."""
    return _trace_pieces(run_pieces(counts, n, H, W, what='mask_polygons', limit=MASK_POLYGON_MAX_PIECES), H, W)   # read 1


def _trace_pieces(rp, H, W):
    """mask_polygons after its piece table (reads 2 and 3)"""
    lib = _lib.load()
    pieces, piece_offs, P, widest = rp
    k, H, W, dev = int(piece_offs.shape[0]) - 1, int(H), int(W), pieces.device
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)

    def empty():
        return (torch.zeros((0, 2), **i32), torch.zeros((1,), **i64), torch.zeros((0,), **i32), torch.zeros((0,), **i32),
                torch.zeros((0,), **i64), torch.zeros((k + 1,), **i64))
    if P == 0:
        return empty()
    E = 6 * P
    ekey, eoth, succ = torch.empty((E,), **i64), torch.empty((E,), **i32), torch.empty((E,), **i32)
    _lib.check(lib.rsp_mask_polygon_edges(k, H, W, piece_offs.data_ptr(), P, pieces.data_ptr(), ekey.data_ptr(), eoth.data_ptr(),
                                          succ.data_ptr(), _stream()), "rsp_mask_polygon_edges")
    ws = torch.empty((int(lib.rsp_mask_polygon_rank_workspace_bytes(P)) // 8 + 1,), **i64)
    ring_key, area2 = torch.empty((E,), **i64), torch.empty((E,), **i64)
    flags = torch.empty((E,), dtype=torch.uint8, device=dev)
    lastof, corners = torch.empty((E,), **i32), torch.empty((E,), **i32)
    _lib.check(lib.rsp_mask_polygon_rank(P, H, _log2_ceil(6 * widest), ekey.data_ptr(), eoth.data_ptr(), succ.data_ptr(),
                                         ws.data_ptr(), ring_key.data_ptr(), flags.data_ptr(), lastof.data_ptr(),
                                         corners.data_ptr(), area2.data_ptr(), _stream()), "rsp_mask_polygon_rank")
    # the rings = the edges that start one, sorted by (instance, first vertex); their sizes sit at each ring's last edge
    first = (flags & 1).nonzero().view(-1)                                                        # read 2 (R)
    R = int(first.shape[0])
    if R == 0:
        return empty()
    ring_inst = pieces[3][first // 6]
    ring_keys, order = torch.sort((ring_inst.to(torch.int64) << 33) | ring_key[first])
    ring_inst = ring_inst[order].contiguous()
    last = lastof[first[order]].to(torch.int64).clamp(min=0)
    ring_area2 = area2[last].contiguous()
    ring_offs = _exclusive_total(corners[last])[0]
    inst_ring_offs = torch.searchsorted(ring_inst, torch.arange(k + 1, **i32)).to(torch.int64).contiguous()
    V = int(ring_offs[-1].item())                                                                 # read 3
    verts = torch.zeros((V, 2), **i32)
    ring_parent = torch.empty((R,), **i32)
    near_ws = torch.empty((2 * R,), **i32)
    _lib.check(lib.rsp_mask_polygon_write(P, k, H, R, V, _log2_ceil(R), pieces.data_ptr(), piece_offs.data_ptr(),
                                          ekey.data_ptr(), eoth.data_ptr(), ring_key.data_ptr(), flags.data_ptr(),
                                          corners.data_ptr(), ring_keys.data_ptr(), ring_offs.data_ptr(), ring_area2.data_ptr(),
                                          inst_ring_offs.data_ptr(), near_ws.data_ptr(), verts.data_ptr(),
                                          ring_parent.data_ptr(), _stream()), "rsp_mask_polygon_write")
    return verts, ring_offs, ring_inst, ring_parent, ring_area2, inst_ring_offs


# ----------------------------------------------------------------------------- polygon simplification (csrc/ring_simplify.hip)
RING_SIMPLIFY_MAX_TOL2_Q8 = CONST['RSP_RING_SIMPLIFY_MAX_TOL2_Q8']      # tolerance^2 in 1 / 256 px^2: tolerances up to 65 536 px
RING_SIMPLIFY_MAX_SIDE = CONST['RSP_RING_SIMPLIFY_MAX_SIDE']         # coordinates in [0, 2^20]: every distance comparison fits 128-bit integers
_RING_ARRAYS = (('verts', torch.int32, 2), ('ring_offs', torch.int64, 1), ('ring_inst', torch.int32, 1),
                ('ring_parent', torch.int32, 1), ('ring_area2', torch.int64, 1), ('inst_ring_offs', torch.int64, 1))


def ring_simplify(verts, ring_offs, ring_inst, ring_parent, ring_area2, inst_ring_offs, tol2_q8, min_ring_area, H, W,
                  with_rounds=False, variant=0):
    """Douglas-Peucker on the rings of mask_polygons (the six arrays it returns, or synthetic rings in that layout with
    coordinates in [0, 2^20]), exact and on the device: every ring keeps its first vertex and the vertex
    farthest from it, then the vertices farther than the tolerance from the SEGMENT between the kept vertices around them,
    chain by chain; tol2_q8 = round(256 tolerance^2), an integer in [0, 2^40].  A ring is dropped when |ring_area2| <
    2 min_ring_area (the area BEFORE simplification), when fewer than 3 vertices are kept, when its new doubled area is 0 or
    changed sign, or when it is a hole whose outer ring was dropped.  Returns the six arrays of the surviving rings in their
    old order (ring_area2 recomputed, ring_parent re-indexed among the survivors of the instance, inst_ring_offs rebuilt) and
    ring_src int32 [R'], each survivor's index among the input rings; with_rounds=True appends rounds int32 [R], the depth of
    every INPUT ring's split tree.  One device-to-host read (R' and V', together).  `variant`: the launch alternatives of
    rsp_ring_simplify_mark (measurement only: the results are the same)."""
    lib = _lib.load()
    arrays = (verts, ring_offs, ring_inst, ring_parent, ring_area2, inst_ring_offs)
    for (name, dtype, dim), t in zip(_RING_ARRAYS, arrays):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dim or t.device != verts.device:
            raise ValueError(f'ring_simplify: {name} must be a {dtype} tensor of {dim} dimension(s) on the device of verts')
    if not _is_device(verts):
        raise ValueError('ring_simplify: the ring arrays live on the HIP device')
    R, V, k = int(ring_inst.shape[0]), int(verts.shape[0]), int(inst_ring_offs.shape[0]) - 1
    if verts.shape[1] != 2 or ring_offs.shape[0] != R + 1 or ring_parent.shape[0] != R or ring_area2.shape[0] != R or k < 0:
        raise ValueError('ring_simplify: expected verts [V, 2], ring_offs [R + 1], ring_inst / ring_parent / ring_area2 [R] '
                         'and inst_ring_offs [k + 1]')
    if isinstance(tol2_q8, bool) or not isinstance(tol2_q8, int) or not 0 <= tol2_q8 <= RING_SIMPLIFY_MAX_TOL2_Q8:
        raise ValueError(f'ring_simplify: tol2_q8 is an integer in [0, 2^40], got {tol2_q8!r}')
    if isinstance(min_ring_area, bool) or not isinstance(min_ring_area, int) or min_ring_area < 0:
        raise ValueError(f'ring_simplify: min_ring_area is a non-negative integer of pixels, got {min_ring_area!r}')
    H, W = int(H), int(W)
    if H < 1 or W < 1 or max(H, W) > RING_SIMPLIFY_MAX_SIDE:
        raise ValueError(f'ring_simplify: a {H} x {W} canvas; the sides are in [1, 2^20]')
    if V >= 2 ** 31 or R >= 2 ** 31:
        raise ValueError('ring_simplify: at most 2^31 - 1 vertices and rings in one call')
    dev = verts.device
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    verts, ring_offs, ring_inst, ring_parent, ring_area2, inst_ring_offs = (t.contiguous() for t in arrays)
    rounds = torch.zeros((0,), **i32)

    def nothing():
        out = (torch.zeros((0, 2), **i32), torch.zeros((1,), **i64), torch.zeros((0,), **i32), torch.zeros((0,), **i32),
               torch.zeros((0,), **i64), torch.zeros((k + 1,), **i64), torch.zeros((0,), **i32))
        return out + (rounds,) if with_rounds else out
    if R == 0:
        return nothing()
    keep = torch.zeros((max(V, 1),), dtype=torch.uint8, device=dev)
    pos = torch.empty((max(V, 1),), **i32)
    cnt, area2, sums = torch.empty((R,), **i32), torch.empty((R,), **i64), torch.empty((2, R), **i64)
    rounds = torch.empty((R,), **i32)
    _lib.check(lib.rsp_ring_simplify_mark(verts.data_ptr(), ring_offs.data_ptr(), R, V, tol2_q8, H, W, int(variant),
                                          keep.data_ptr(), pos.data_ptr(), cnt.data_ptr(), area2.data_ptr(), rounds.data_ptr(),
                                          _stream()), "rsp_ring_simplify_mark")
    _lib.check(lib.rsp_ring_simplify_survive(ring_inst.data_ptr(), ring_parent.data_ptr(), ring_area2.data_ptr(),
                                             inst_ring_offs.data_ptr(), R, k, min(min_ring_area, 2 ** 62), cnt.data_ptr(),
                                             area2.data_ptr(), sums.data_ptr(), _stream()), "rsp_ring_simplify_survive")
    csum = torch.cumsum(sums, 1)                      # survivors and their vertices up to every ring: one sum over both rows
    R2, V2 = csum[:, -1].tolist()                                                                   # the one read
    if R2 == 0:
        return nothing()
    out_verts = torch.zeros((V2, 2), **i32)
    out_offs, out_area2, out_inst_offs = torch.empty((R2 + 1,), **i64), torch.empty((R2,), **i64), torch.empty((k + 1,), **i64)
    out_inst, out_parent, out_src = torch.empty((R2,), **i32), torch.empty((R2,), **i32), torch.empty((R2,), **i32)
    _lib.check(lib.rsp_ring_simplify_write(verts.data_ptr(), ring_offs.data_ptr(), ring_inst.data_ptr(), ring_parent.data_ptr(),
                                           inst_ring_offs.data_ptr(), R, V, k, keep.data_ptr(), pos.data_ptr(), area2.data_ptr(),
                                           sums.data_ptr(), csum.data_ptr(), R2, V2, out_verts.data_ptr(), out_offs.data_ptr(),
                                           out_inst.data_ptr(), out_parent.data_ptr(), out_area2.data_ptr(),
                                           out_inst_offs.data_ptr(), out_src.data_ptr(), _stream()), "rsp_ring_simplify_write")
    out = (out_verts, out_offs, out_inst, out_parent, out_area2, out_inst_offs, out_src)
    return out + (rounds,) if with_rounds else out


# ----------------------------------------------------------------------------- shared borders (csrc/ring_coverage.hip)
RING_COVERAGE_MAX_SIDE = CONST['RSP_RING_COVERAGE_MAX_SIDE']         # the coordinate bound of the 128-bit distance, as above


def ring_coverage(counts, n, H, W, tol2_q8, with_rounds=False, variant=0):
    """Shared-border simplification of a planar layer: counts int32 [k, cap] / n int32 [k], k masks on one
    (H, W) canvas whose rows are pairwise DISJOINT and canonical (what rle_flatten returns), H W < 2^31, max(H, W) <= 2^20 ->
    the rings of mask_polygons with every node inserted (a lattice point where at least 3 of the 4 sides around it separate
    different owners: T-junctions, points where 3 or 4 regions meet or two meet the canvas border, saddles), each ring rotated
    to begin at its first node visit (a ring without a node stays at its smallest vertex), and every arc between two node
    visits simplified by Douglas-Peucker at tol2_q8 = round(256 tolerance^2) with rules that do not depend on the direction
    or the start of the walk -- so the two rings along a border keep the same vertices.  Every node is kept; tol2_q8 = 0 keeps
    every vertex.  A ring is dropped when fewer than 3 vertices are kept, when its new doubled area is 0 or changed sign, or
    when it is a hole whose outer ring was dropped.  Returns the six arrays of the surviving rings in the layout of
    ring_simplify, ring_src int32 [R'] and vert_other int32 [V']: the owner on the far side of the edge that leaves every
    output vertex (-1: background or the canvas border); with_rounds=True appends rounds int32 [R] of every traced ring.
    Rows that overlap, or that hold a zero count inside, are refused (ValueError).
    Five device-to-host reads, whatever k is: the pieces, the rings and the vertices of the trace (mask_polygons), the
    noded vertices together with the disjointness flags, the survivors (R' and V' together); one when the table has no
    piece.  `variant`: the launch alternatives of rsp_ring_coverage_mark (measurement only)."""
    lib = _lib.load()
    if isinstance(tol2_q8, bool) or not isinstance(tol2_q8, int) or not 0 <= tol2_q8 <= RING_SIMPLIFY_MAX_TOL2_Q8:
        raise ValueError(f'ring_coverage: tol2_q8 is an integer in [0, 2^40], got {tol2_q8!r}')
    if max(int(H), int(W)) > RING_COVERAGE_MAX_SIDE:
        raise ValueError(f'ring_coverage: a {int(H)} x {int(W)} canvas; the sides are at most 2^20')
    rp = run_pieces(counts, n, H, W, what='ring_coverage', limit=MASK_POLYGON_MAX_PIECES)                 # read 1
    k, H, W, dev, P = int(rp.piece_offs.shape[0]) - 1, int(H), int(W), rp.pieces.device, rp.P
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    rounds = torch.zeros((0,), **i32)

    def nothing():
        out = (torch.zeros((0, 2), **i32), torch.zeros((1,), **i64), torch.zeros((0,), **i32), torch.zeros((0,), **i32),
               torch.zeros((0,), **i64), torch.zeros((k + 1,), **i64), torch.zeros((0,), **i32), torch.zeros((0,), **i32))
        return out + (rounds,) if with_rounds else out
    if P == 0:
        return nothing()
    cpieces, col_offs, _ = _column_pieces(lib, rp, H, W)
    bad = torch.empty((P,), **i32)
    _lib.check(lib.rsp_ring_coverage_check(cpieces.data_ptr(), P, H, W, bad.data_ptr(), _stream()), "rsp_ring_coverage_check")
    verts, ring_offs, ring_inst, ring_parent, ring_area2, inst_ring_offs = _trace_pieces(rp, H, W)        # reads 2, 3
    R, V = int(ring_inst.shape[0]), int(verts.shape[0])
    cnt, first = torch.ones((max(V, 1),), **i32), torch.full((max(V, 1),), -1, **i32)
    table = (cpieces.data_ptr(), col_offs.data_ptr(), P, k, H, W)
    _lib.check(lib.rsp_ring_coverage_nodes_count(verts.data_ptr(), ring_offs.data_ptr(), R, V, *table, cnt.data_ptr(),
                                                 first.data_ptr(), _stream()), "rsp_ring_coverage_nodes_count")
    noff, total = _exclusive_total(cnt[:V])
    Vn, worst = torch.stack([total, bad.max().to(torch.int64)]).tolist()                                  # read 4
    if worst == 1:
        raise ValueError('ring_coverage: the rows of the table overlap; shared borders exist between disjoint instances only '
                         '(make them disjoint first: apis.flatten_masks / rle.flatten_runs)')
    if worst:
        raise ValueError('ring_coverage: a row of the table is not canonical (a zero count inside it: two ones-runs touch); '
                         'rle.flatten_runs returns canonical rows')
    if R == 0:
        return nothing()
    # every ring's first node visit: the first segment at or behind the ring's start that holds a node, and where in it
    has = (first[:V] >= 0).to(torch.int64)
    seen = torch.cumsum(has, 0)
    start = ring_offs[:-1]
    j = torch.searchsorted(seen, (seen - has)[start.clamp(max=V - 1)] + 1).clamp(max=V - 1)
    found = (j < ring_offs[1:]) & (has[j] > 0)
    rot = torch.where(found, noff[j] + first[j].clamp(min=0) - noff[start], torch.zeros_like(start)).contiguous()
    n_offs = noff[ring_offs].contiguous()
    nverts, nother = torch.empty((Vn, 2), **i32), torch.empty((Vn,), **i32)
    keep = torch.empty((Vn,), dtype=torch.uint8, device=dev)
    _lib.check(lib.rsp_ring_coverage_nodes_write(verts.data_ptr(), ring_offs.data_ptr(), R, V, *table, noff.data_ptr(),
                                                 rot.data_ptr(), Vn, nverts.data_ptr(), keep.data_ptr(), nother.data_ptr(),
                                                 _stream()), "rsp_ring_coverage_nodes_write")
    pos = torch.empty((Vn,), **i32)
    kept_cnt, area2, sums = torch.empty((R,), **i32), torch.empty((R,), **i64), torch.empty((2, R), **i64)
    rounds = torch.empty((R,), **i32)
    _lib.check(lib.rsp_ring_coverage_mark(nverts.data_ptr(), n_offs.data_ptr(), R, Vn, tol2_q8, H, W, int(variant),
                                          keep.data_ptr(), pos.data_ptr(), kept_cnt.data_ptr(), area2.data_ptr(),
                                          rounds.data_ptr(), _stream()), "rsp_ring_coverage_mark")
    _lib.check(lib.rsp_ring_simplify_survive(ring_inst.data_ptr(), ring_parent.data_ptr(), ring_area2.data_ptr(),
                                             inst_ring_offs.data_ptr(), R, k, 0, kept_cnt.data_ptr(), area2.data_ptr(),
                                             sums.data_ptr(), _stream()), "rsp_ring_simplify_survive")
    csum = torch.cumsum(sums, 1)
    R2, V2 = csum[:, -1].tolist()                                                                         # read 5
    if R2 == 0:
        return nothing()
    out_verts, out_other = torch.zeros((V2, 2), **i32), torch.empty((V2,), **i32)
    out_offs, out_area2, out_inst_offs = torch.empty((R2 + 1,), **i64), torch.empty((R2,), **i64), torch.empty((k + 1,), **i64)
    out_inst, out_parent, out_src = torch.empty((R2,), **i32), torch.empty((R2,), **i32), torch.empty((R2,), **i32)
    _lib.check(lib.rsp_ring_simplify_write(nverts.data_ptr(), n_offs.data_ptr(), ring_inst.data_ptr(), ring_parent.data_ptr(),
                                           inst_ring_offs.data_ptr(), R, Vn, k, keep.data_ptr(), pos.data_ptr(), area2.data_ptr(),
                                           sums.data_ptr(), csum.data_ptr(), R2, V2, out_verts.data_ptr(), out_offs.data_ptr(),
                                           out_inst.data_ptr(), out_parent.data_ptr(), out_area2.data_ptr(),
                                           out_inst_offs.data_ptr(), out_src.data_ptr(), _stream()), "rsp_ring_simplify_write")
    _lib.check(lib.rsp_ring_coverage_other(n_offs.data_ptr(), R, Vn, keep.data_ptr(), pos.data_ptr(), sums.data_ptr(),
                                           csum.data_ptr(), V2, nother.data_ptr(), out_other.data_ptr(), _stream()),
               "rsp_ring_coverage_other")
    out = (out_verts, out_offs, out_inst, out_parent, out_area2, out_inst_offs, out_src, out_other)
    return out + (rounds,) if with_rounds else out


# ----------------------------------------------------------------------------- oriented boxes (csrc/mask_obb.hip)
MASK_OBB_MAX_SIDE = CONST['RSP_MASK_OBB_MAX_SIDE']                # coordinates in [0, 65 535]: 16 bits each, and every product of the calipers fits 128
MASK_OBB_MAX_BOUND = CONST['RSP_MASK_OBB_MAX_BOUND']         # three records per ones-run over all rows of one call (32-bit hull offsets)


def mask_hull(counts, n, H, W, with_rounds=False):
    """run table (counts int32 [k, cap], n int32 [k]: k masks on one (H, W) canvas) -> the convex hull of every mask (the
    union of the closed unit squares of ALL its pixels), exact and on the device:
      hull_verts int32 [Vh, 2] = (x, y), hull_offs int64 [k + 1], hull_area2 int64 [k] (doubled area, > 0).
    A hull is strictly convex, starts at its smallest vertex by (x, y), runs clockwise on screen and does not repeat its
    first vertex; a non-empty mask has at least 4 vertices, a row with n <= 0 none.  with_rounds=True appends rounds int32
    [2, k], the pruning rounds of the upper and the lower chain.  Two device-to-host reads, whatever k is: the size of the
    workspace (three records per ones-run) and the number of hull vertices."""
    lib = _lib.load()
    counts, n, k, cap, H, W = _rle_rows('mask_hull', counts, n, H, W)
    if max(H, W) > MASK_OBB_MAX_SIDE:
        raise ValueError(f'mask_hull: a {H} x {W} canvas; the sides are at most {MASK_OBB_MAX_SIDE}')
    dev = n.device
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    rounds = torch.zeros((2, k), **i32)

    def empty():
        out = (torch.zeros((0, 2), **i32), torch.zeros((k + 1,), **i64), torch.zeros((k,), **i64))
        return out + (rounds,) if with_rounds else out
    if k == 0:
        return empty()
    bound = 3 * (n.clamp(0, cap) // 2).to(torch.int64)
    bound_offs, total = _exclusive_total(bound)
    B = int(total.item())                                                                           # read 1
    if B == 0:
        return empty()
    if B > MASK_OBB_MAX_BOUND:
        raise ValueError(f'mask_hull: {B // 3} ones-runs in one call; at most {MASK_OBB_MAX_BOUND // 3} (split the rows), so '
                         'that the hull vertices of one call stay below 2^31')
    ws = torch.empty((int(lib.rsp_mask_hull_workspace_bytes(B)) // 4,), **i32)
    chain_cnt = torch.zeros((2, k), **i32)
    _lib.check(lib.rsp_mask_hull_chains(counts.data_ptr(), n.data_ptr(), k, cap, H, W, bound_offs.data_ptr(), B, ws.data_ptr(),
                                        chain_cnt.data_ptr(), rounds.data_ptr(), _stream()), "rsp_mask_hull_chains")
    hull_offs, total = _exclusive_total(chain_cnt.sum(0, dtype=torch.int64))
    Vh = int(total.item())                                                                          # read 2
    verts, area2 = torch.zeros((Vh, 2), **i32), torch.zeros((k,), **i64)
    _lib.check(lib.rsp_mask_hull_write(n.data_ptr(), k, cap, bound_offs.data_ptr(), B, ws.data_ptr(), chain_cnt.data_ptr(),
                                       hull_offs.data_ptr(), Vh, verts.data_ptr(), area2.data_ptr(), _stream()),
               "rsp_mask_hull_write")
    out = (verts, hull_offs, area2)
    return out + (rounds,) if with_rounds else out


def hull_min_rect(hull_verts, hull_offs):
    """convex polygons (hull_verts int32 [Vh, 2], hull_offs int64 [k + 1]: what mask_hull returns, or any canonical strictly
    convex rings, clockwise on screen, with coordinates in [0, 65 535]) -> (edge int32 [k], q int64 [k, 6]): the
    minimum-area rectangle of each, flush with hull edge `edge` (the lowest among equals, -1 for a polygon without vertices);
    q = (ex, ey, amin, amax, bmin, bmax) in the frame of that edge (rle.obb_to_numpy turns it into corners).
    Exact 128-bit integer comparisons on the device; the coordinate range of the vertices is the caller's to keep (they are
    not read here).  No device-to-host read."""
    lib = _lib.load()
    for name, t, dtype, dim in (('hull_verts', hull_verts, torch.int32, 2), ('hull_offs', hull_offs, torch.int64, 1)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dim or t.device != hull_verts.device:
            raise ValueError(f'hull_min_rect: {name} must be a {dtype} tensor of {dim} dimension(s) on the device of hull_verts')
    if not _is_device(hull_verts):
        raise ValueError('hull_min_rect: the hull arrays live on the HIP device')
    Vh, k = int(hull_verts.shape[0]), int(hull_offs.shape[0]) - 1
    if hull_verts.shape[1] != 2 or k < 0:
        raise ValueError('hull_min_rect: expected hull_verts [Vh, 2] and hull_offs [k + 1]')
    if Vh >= 2 ** 31 or k >= 2 ** 31:
        raise ValueError('hull_min_rect: at most 2^31 - 1 vertices and polygons in one call')
    dev = hull_verts.device
    edge = torch.full((k,), -1, dtype=torch.int32, device=dev)
    q = torch.zeros((k, 6), dtype=torch.int64, device=dev)
    if k:
        hull_verts, hull_offs = hull_verts.contiguous(), hull_offs.contiguous()
        _lib.check(lib.rsp_hull_min_rect(hull_verts.data_ptr(), hull_offs.data_ptr(), k, Vh, edge.data_ptr(), q.data_ptr(),
                                         _stream()), "rsp_hull_min_rect")
    return edge, q


# ----------------------------------------------------------------------------- oriented-box comparison (csrc/obb_iou.hip)
OBB_NMS_MAX = CONST['RSP_OBB_NMS_MAX']                        # boxes of one obb_nms: an n x ceil(n / 64) word suppression mask


def _chk_quad(what, name, t, dev=None):
    """a box array: float64 [n, 4, 2] on the HIP device -> (contiguous tensor, n)"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 3 or tuple(t.shape[1:]) != (4, 2):
        raise ValueError(f'{what}: {name} must be a float64 tensor [n, 4, 2] (four corners (x, y) per box)')
    if not _is_device(t):
        raise ValueError(f'{what}: {name} lives on the HIP device')
    if dev is not None and t.device != dev:
        raise ValueError(f'{what}: {name} must be on the device of the other arrays')
    return t.contiguous(), int(t.shape[0])


def _chk_vec(what, name, t, dtype, n, dev, cols=None):
    shape = (n,) if cols is None else (n, cols)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != dev:
        raise ValueError(f'{what}: {name} must be a {dtype} tensor {list(shape)} on the device of the other arrays')
    return t.contiguous()


def obb_corners(edge, q, offsets=None):
    """(edge int32 [k], q int64 [k, 6]) as hull_min_rect returns them, offsets int32 [k, 2] = (ox, oy) or None -> float64
    [k, 4, 2] on the device: the corners of rle.obb_to_numpy(form='corners'), bit for bit, of the rectangles moved by their
    offsets in integers first; NaN rows where edge is -1 (rsp_obb_corners).  No device-to-host read."""
    lib = _lib.load()
    if not isinstance(edge, torch.Tensor) or edge.dtype != torch.int32 or edge.dim() != 1:
        raise ValueError('obb_corners: edge must be an int32 tensor [k]')
    if not _is_device(edge):
        raise ValueError('obb_corners: the rectangles live on the HIP device')
    k, dev = int(edge.shape[0]), edge.device
    q = _chk_vec('obb_corners', 'q', q, torch.int64, k, dev, 6)
    if offsets is not None:
        offsets = _chk_vec('obb_corners', 'offsets', offsets, torch.int32, k, dev, 2)
    out = torch.empty((k, 4, 2), dtype=torch.float64, device=dev)
    if k:
        _lib.check(lib.rsp_obb_corners(edge.contiguous().data_ptr(), q.data_ptr(), _ptr(offsets), k, out.data_ptr(), _stream()),
                   "rsp_obb_corners")
    return out


def obb_iou(units, n_iou, dt_quad, gt_quad, gt_crowd):
    """IoU blocks of the units (`coco_units`, ascending in out0; nwords is not read) between oriented boxes dt_quad float64
    [n_dt, 4, 2] and gt_quad float64 [n_gt, 4, 2], gt_crowd uint8 [n_gt] -> float64 [n_iou] (rsp_obb_iou):
    inter / union in fp64, inter / area_dt for a crowd gt, the intersection clipped as a closed polygon.  A degenerate box
    (a non-finite coordinate, zero area) has IoU 0.0 with everything.  No device-to-host read."""
    lib = _lib.load()
    dt_quad, n_dt = _chk_quad('obb_iou', 'dt_quad', dt_quad)
    dev = dt_quad.device
    gt_quad, n_gt = _chk_quad('obb_iou', 'gt_quad', gt_quad, dev)
    gt_crowd = _chk_vec('obb_iou', 'gt_crowd', gt_crowd, torch.uint8, n_gt, dev)
    if not isinstance(units, torch.Tensor) or units.dtype != torch.uint8 or units.dim() != 1 or units.device != dev or \
            units.numel() % COCO_UNIT_BYTES:
        raise ValueError('obb_iou: units must be the uint8 tensor of coco_units on the device of the boxes')
    n_iou = int(n_iou)
    if n_iou < 0:
        raise ValueError('obb_iou: n_iou is negative')
    iou = torch.zeros((max(n_iou, 1),), dtype=torch.float64, device=dev)
    nu = units.numel() // COCO_UNIT_BYTES
    if nu and n_iou:
        _lib.check(lib.rsp_obb_iou(_units_ptr(units.contiguous()), nu, dt_quad.data_ptr(), n_dt, gt_quad.data_ptr(), n_gt,
                                   gt_crowd.data_ptr(), iou.data_ptr(), n_iou, _stream()), "rsp_obb_iou")
    return iou[:n_iou]


def obb_nms(quad, scores, labels, iou_thr, class_agnostic=False):
    """mmcv.ops.nms_rotated on flat device tensors (rsp_obb_nms): quad float64 [n, 4, 2], scores float32 [n],
    labels int32 [n] -> keep int64 [m], indices into the inputs in kept order.  Order: score descending, original position
    ascending; a box is suppressed by a kept box ahead of it with the same label (any label with class_agnostic) and
    IoU > iou_thr (strict).  Degenerate boxes (NaN rows of empty masks) suppress nothing and are kept.  n <= OBB_NMS_MAX.
    One host read (the number kept)."""
    lib = _lib.load()
    quad, n = _chk_quad('obb_nms', 'quad', quad)
    dev = quad.device
    scores = _chk_vec('obb_nms', 'scores', scores, torch.float32, n, dev)
    labels = _chk_vec('obb_nms', 'labels', labels, torch.int32, n, dev)
    iou_thr = float(iou_thr)
    if not iou_thr >= 0.0:
        raise ValueError(f'obb_nms: iou_thr = {iou_thr}; it must be >= 0')
    if n > OBB_NMS_MAX:
        raise ValueError(f'obb_nms: {n} boxes, rsp_obb_nms holds {OBB_NMS_MAX} at most (its suppression mask has n^2 / 8 bytes)')
    if n == 0:
        return torch.zeros((0,), dtype=torch.int64, device=dev)
    ws = torch.empty((int(lib.rsp_obb_nms_workspace_bytes(n)) // 8,), dtype=torch.int64, device=dev)
    keep = torch.zeros((n,), dtype=torch.int32, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.check(lib.rsp_obb_nms(quad.data_ptr(), scores.data_ptr(), labels.data_ptr(), n, iou_thr, int(bool(class_agnostic)),
                               ws.data_ptr(), keep.data_ptr(), cnt.data_ptr(), _stream()), "rsp_obb_nms")
    return keep[:int(cnt.item())].to(torch.int64)


# ----------------------------------------------------------------------------- run-domain components (csrc/run_components.hip)
RUN_COMPONENTS_MAX_PIECES = CONST['RSP_RUN_COMPONENTS_MAX_PIECES']      # column pieces of one call: 32-bit piece indices
RunComponents = collections.namedtuple('RunComponents', 'comp_offs piece_comp comp_area comp_box comp_first comp_inst pieces '
                                       'piece_offs status')


def check_components_status(status):
    """`status` of rle_components ON THE HOST: non-zero means that a find / union loop of the labelling reached its step cap
    and the result is invalid"""
    if any(int(s) != 0 for s in list(status)):
        raise RuntimeError("rsp_run_components_label: the labelling reached its iteration cap (status != 0); the result is "
                           "invalid")


def rle_components(counts, n, H, W):
    """run table (counts int32 [k, cap], n int32 [k]: k masks on one (H, W) canvas) -> the 8-connected components of every
    mask, all on the device, as RunComponents:
      comp_offs int64 [k + 1] (the components of each instance), piece_comp int32 [P], comp_area int32 [C], comp_box int32
      [C, 4] = (x0, y0, x1, y1) end-exclusive, comp_first int32 [C] (the lowest row-major index y W + x of the component's
      pixels), comp_inst int32 [C], pieces int32 [4, P] = (x, y0, y1, instance) of the column pieces sorted by (instance, x,
      y0), piece_offs int64 [k + 1], status int32 [1].
    Components are numbered by (instance, first pixel in stream order).  A row with n <= 0 has none.  Two device-to-host
    reads, whatever k is: the pieces P, and the components C together with status (non-zero raises RuntimeError)."""
    lib = _lib.load()
    pieces, piece_offs, P, _ = run_pieces(counts, n, H, W, what='rle_components', limit=RUN_COMPONENTS_MAX_PIECES)     # read 1
    k, H, W, dev = int(piece_offs.shape[0]) - 1, int(H), int(W), pieces.device
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    status = torch.zeros((1,), **i32)
    if P == 0:
        return RunComponents(torch.zeros((k + 1,), **i64), torch.zeros((0,), **i32), torch.zeros((0,), **i32),
                             torch.zeros((0, 4), **i32), torch.zeros((0,), **i32), torch.zeros((0,), **i32), pieces, piece_offs,
                             status)
    ws = torch.empty((int(lib.rsp_run_components_workspace_bytes(H, W, P)) // 4,), **i32)
    label, root = torch.empty((P,), **i32), torch.empty((P,), **i32)
    _lib.check(lib.rsp_run_components_label(k, H, W, piece_offs.data_ptr(), P, pieces.data_ptr(), ws.data_ptr(), label.data_ptr(),
                                            root.data_ptr(), status.data_ptr(), _stream()), "rsp_run_components_label")
    root_cum = torch.cumsum(root, 0, dtype=torch.int64)
    C, bad = torch.stack([root_cum[-1], status[0].to(torch.int64)]).tolist()                         # read 2
    check_components_status([bad])
    piece_comp = torch.empty((P,), **i32)
    comp_area, comp_box = torch.empty((C,), **i32), torch.empty((C, 4), **i32)
    comp_first, comp_inst = torch.empty((C,), **i32), torch.empty((C,), **i32)
    _lib.check(lib.rsp_run_components_stats(pieces.data_ptr(), P, H, W, label.data_ptr(), root.data_ptr(), root_cum.data_ptr(),
                                            C, piece_comp.data_ptr(), comp_area.data_ptr(), comp_box.data_ptr(),
                                            comp_first.data_ptr(), comp_inst.data_ptr(), _stream()), "rsp_run_components_stats")
    comp_offs = torch.searchsorted(comp_inst, torch.arange(k + 1, **i32)).to(torch.int64).contiguous()
    return RunComponents(comp_offs, piece_comp, comp_area, comp_box, comp_first, comp_inst, pieces, piece_offs, status)


def components_select(comps, min_area, keep_largest, slot, changed):
    """which components of rle_components stay (rsp_run_components_select): keep int32 [C] = 1 for a component of at least
    min_area pixels; keep_largest: when an instance has none, its largest stays, among equals the one with the lowest
    comp_first.  changed int32 [k, 2] (device): column `slot` receives 1 where an instance has a smaller component.  No host
    read."""
    lib = _lib.load()
    k, C = int(comps.comp_offs.shape[0]) - 1, int(comps.comp_area.shape[0])
    if int(min_area) != min_area or not 0 <= int(min_area) < 2 ** 31:
        raise ValueError(f'components_select: min_area must be an integer in [0, 2^31), got {min_area!r}')
    if changed.dtype != torch.int32 or tuple(changed.shape) != (k, 2) or not changed.is_contiguous():
        raise ValueError('components_select: changed is a contiguous int32 [k, 2] tensor')
    keep = torch.zeros((C,), dtype=torch.int32, device=changed.device)
    if k:
        _lib.check(lib.rsp_run_components_select(comps.comp_offs.data_ptr(), k, C, comps.comp_area.data_ptr(),
                                                 comps.comp_first.data_ptr(), int(min_area), 1 if keep_largest else 0, int(slot),
                                                 keep.data_ptr(), changed.data_ptr(), _stream()), "rsp_run_components_select")
    return keep


def components_union(comps, H, W, cap_out, keep=None):
    """the pieces of rle_components as run tables through rsp_rle_union (its (group << 31 | pixel start, end) intervals are
    index arithmetic on the pieces and one device key sort).  keep=None: one row per COMPONENT, C rows in component order (a
    split); keep int32 [C]: one row per INSTANCE holding its components with keep != 0 (a filter; an instance without any is
    the empty mask, one count H * W).  -> (counts int32 [G, cap_out], n int32 [G]), n = -(needed) for a row that does not fit
    (the protocol of fit_runs).  No host read."""
    lib = _lib.load()
    H, W = int(H), int(W)
    dev = comps.piece_comp.device
    k, C, P = int(comps.comp_offs.shape[0]) - 1, int(comps.comp_area.shape[0]), int(comps.piece_comp.shape[0])
    G = C if keep is None else k
    if int(cap_out) < 2:
        raise ValueError('components_union: cap_out is at least 2')
    if G and P and C:
        pc = comps.piece_comp.to(torch.int64)
        x, y0, y1, inst = (comps.pieces[i].to(torch.int64) for i in range(4))
        live = pc >= 0
        if keep is None:
            group = torch.where(live, pc, G)                           # a slot no row filled sorts behind every group
        else:
            group = torch.where(live & (keep.to(torch.int64)[pc.clamp(min=0)] != 0), inst, G)
        keys, order = torch.sort((group << 31) | ((x * H + y0) & 0x7fffffff))
        ends = (x * H + y1).to(torch.int32)[order].contiguous()
        iv_offs = torch.searchsorted(keys, torch.arange(G + 1, dtype=torch.int64, device=dev) << 31).contiguous()
        total = P
    else:
        keys, ends, total, iv_offs = None, None, 0, torch.zeros((G + 1,), dtype=torch.int64, device=dev)
    return _intervals_to_runs(lib, keys, ends, total, iv_offs, G, H, W, cap_out)


def rle_complement(counts, n):
    """the complement of every row of a canonical run table: the same counts with a leading zero count added, or removed
    where the row has one, so n changes by one -> (counts int32 [k, cap + 1], n int32 [k]).  A row with n <= 0 stays empty
    (n = 0); n beyond cap is cut at cap.  Index arithmetic on the device, no host read."""
    k, cap = int(counts.shape[0]), int(counts.shape[1])
    nn = n.clamp(0, cap)
    lead0 = counts[:, 0] == 0
    added = torch.zeros((k, cap + 1), dtype=torch.int32, device=counts.device)
    added[:, 1:] = counts
    removed = torch.zeros((k, cap + 1), dtype=torch.int32, device=counts.device)
    removed[:, :cap - 1] = counts[:, 1:]
    out = torch.where(lead0[:, None], removed, added)
    n2 = torch.where(nn <= 0, torch.zeros_like(nn), torch.where(lead0, nn - 1, nn + 1))
    return out.contiguous(), n2.to(torch.int32).contiguous()


# ----------------------------------------------------------------------------- run-domain morphology (csrc/run_morphology.hip)
def _canonical_rows(lib, counts, n, k, cap, H, W):
    """every row through a group-of-one rsp_rle_union: zero counts anywhere go, touching ones-runs merge, a row with n <= 0
    becomes the empty mask (one count H * W) -> (counts int32 [k, cap + 1], n int32 [k]).  The intervals of one row are in
    key order as rsp_rle_intervals writes them, so nothing is sorted; no host read."""
    runs = (n.clamp(0, cap) // 2).to(torch.int64)
    rows = torch.arange(k, dtype=torch.int32, device=n.device)
    # total: the slots of all rows, a bound that is known without reading their sum
    keys, ends, iv_offs, total = _rle_intervals(lib, counts, n, k, cap, H, W, rows, rows, runs, total=k * (cap // 2))
    return _intervals_to_runs(lib, keys, ends, total, iv_offs, k, H, W, cap + 1)


class _RunIntervals:
    """a table of csrc/run_morphology.hip: P intervals (col, y0, y1) on strips of Wt columns per instance; the arrays hold one
    slot at least"""

    def __init__(self, P, Wt, dev, keys=False):
        self.P, self.Wt = int(P), int(Wt)
        size = (max(self.P, 1),)
        if keys:
            self.keys = torch.zeros(size, dtype=torch.int64, device=dev)
            self.ends = torch.zeros(size, dtype=torch.int32, device=dev)
        else:
            self.col, self.y0, self.y1 = (torch.zeros(size, dtype=torch.int32, device=dev) for _ in range(3))

    def offs(self, k):
        """int32 [k Wt + 1]: the first interval of every column"""
        cols = torch.arange(k * self.Wt + 1, dtype=torch.int32, device=self.col.device)
        return torch.searchsorted(self.col[:self.P], cols, out_int32=True).contiguous()


def _run_morph_join(lib, op, A, B, k, shift, span, out_shift, Wout, H, emit):
    """count pass, exclusive sum, ONE host read (the total), write pass -> _RunIntervals"""
    dev = A.col.device
    if A.P == 0:
        return _RunIntervals(0, Wout, dev, keys=emit)
    b_offs = B.offs(k)
    head = (op, A.col.data_ptr(), A.y0.data_ptr(), A.y1.data_ptr(), A.P, A.Wt, b_offs.data_ptr(), B.y0.data_ptr(),
            B.y1.data_ptr(), B.P, k, B.Wt, shift, span)
    cnt = torch.zeros((A.P,), dtype=torch.int32, device=dev)
    _lib.check(lib.rsp_run_morph_join_count(*head, out_shift, Wout, cnt.data_ptr(), _stream()), "rsp_run_morph_join_count")
    offs, total = _exclusive_total(cnt)
    out = _RunIntervals(total.item(), Wout, dev, keys=emit)                                        # the read
    tail = (0, 0, 0, out.keys.data_ptr(), out.ends.data_ptr()) if emit else \
        (out.col.data_ptr(), out.y0.data_ptr(), out.y1.data_ptr(), 0, 0)
    _lib.check(lib.rsp_run_morph_join(*head, offs.data_ptr(), out.P, out_shift, Wout, H, 1 if emit else 0, *tail, _stream()),
               "rsp_run_morph_join")
    return out


def run_morph_levels(radius, W):
    """the window doublings of an erosion by `radius` on a canvas W columns wide: floor(log2(2 min(radius, W) + 1))"""
    return (2 * min(int(radius), int(W)) + 1).bit_length() - 1


def _run_morph(what, counts, n, H, W, radius, border, band, cap):
    lib = _lib.load()
    counts, n, k, cap_in, H, W = _rle_rows(what, counts, n, H, W)
    if isinstance(radius, bool) or int(radius) != radius or int(radius) < 0:
        raise ValueError(f'{what}: radius must be a non-negative integer, got {radius!r}')
    if border not in (0, 1):
        raise ValueError(f'{what}: border must be 0 or 1, got {border!r}')
    dev = n.device
    cap = max(int(cap), 2) if cap is not None else cap_in + 2
    if k == 0:
        return torch.zeros((0, cap), dtype=torch.int32, device=dev), n, n.cpu(), cap
    # beyond the canvas nothing changes with the radius: a window W columns (H rows) to either side covers every column (row)
    rx, ry = min(int(radius), W), min(int(radius), H)
    pad = rx if border else 0
    Wt = W + 2 * pad
    if k * Wt >= 2 ** 31:
        raise ValueError(f'{what}: {k} rows x {Wt} columns; column numbers are 32-bit (< 2^31; split the rows)')
    cc, cn = _canonical_rows(lib, counts, n, k, cap_in, H, W)
    args = (cc.data_ptr(), cn.data_ptr(), k, cap_in + 1, H, W)
    shapes = [(ry, pad, int(border))] + ([(0, 0, 0)] if band else [])
    cnts = torch.zeros((len(shapes), k), dtype=torch.int32, device=dev)
    for i, s in enumerate(shapes):
        _lib.check(lib.rsp_run_morph_pieces_count(*args, *s, cnts[i].data_ptr(), _stream()), "rsp_run_morph_pieces_count")
    offs, totals = _exclusive_total(cnts)
    totals = totals.tolist()                                                                         # read 1
    if max(totals) >= 2 ** 31:
        raise ValueError(f'{what}: {max(totals)} column pieces in one call; at most 2^31 - 1 (split the rows)')
    tables = []
    for i, s in enumerate(shapes):
        t = _RunIntervals(totals[i], W + 2 * s[1], dev)
        _lib.check(lib.rsp_run_morph_pieces(*args, *s, offs[i].data_ptr(), t.P, t.col.data_ptr(), t.y0.data_ptr(),
                                            t.y1.data_ptr(), _stream()), "rsp_run_morph_pieces")
        tables.append(t)
    T, a, L = tables[0], 1, 2 * rx + 1
    while 2 * a <= L:                                           # T_2a(X) = T_a(X) & T_a(X + a): one read per level
        T = _run_morph_join(lib, 0, T, T, k, a, 2 * a, 0, Wt, H, False)
        a *= 2
    # the window [X, X + L) = two windows of `a` columns that may overlap; canvas column x = X + rx - pad
    E = _run_morph_join(lib, 0, T, T, k, L - a, L, rx - pad, W, H, not band)
    if band:
        E = _run_morph_join(lib, 1, tables[1], E, k, 0, 1, 0, W, H, True)
    iv_offs = torch.searchsorted(E.keys[:E.P], torch.arange(k + 1, dtype=torch.int64, device=dev) << 31).contiguous()

    return fit_runs(lambda cap: _intervals_to_runs(lib, E.keys, E.ends, E.P, iv_offs, k, H, W, cap), cap)


def rle_erode(counts, n, H, W, radius, border=0, cap=None):
    """erosion of every row of a run table (counts int32 [k, cap_in], n int32 [k]: k masks on one (H, W) canvas) by the
    (2 radius + 1)^2 square: a pixel stays iff every pixel within `radius` columns and rows of it is set, the
    outside of the canvas counting as `border` (0 or 1) -- scipy.ndimage.binary_erosion(M, ones((3, 3)), iterations=radius,
    border_value=border), cv2.erode on the dense mask.  Zero counts anywhere are legal input (the result is the erosion of the
    decoded stream); a row with n <= 0 is the empty mask; radius 0 returns the canonical form of the rows; radii beyond the
    canvas cost what the canvas side costs.  -> (counts int32 [k, cap'], n int32 [k], n on the host, cap') under fit_runs,
    canonical COCO run counts; cap: the first capacity (the input's plus two when None).
    Device-to-host reads, whatever k is: 2 + L + one per fit_runs attempt, L = run_morph_levels(radius, W) = floor(log2(2
    min(radius, W) + 1)): the level-1 pieces, one total per window doubling, the total of the last join."""
    return _run_morph('rle_erode', counts, n, H, W, radius, border, False, cap)


def rle_boundary(counts, n, H, W, radius, cap=None):
    """the boundary band of every row, M & ~erode(M, radius, border=0): the pixels of the mask within `radius`
    (Chebyshev) of a pixel outside it or of the canvas edge -- boundary-iou-api's mask_to_boundary with dilation = radius.
    Input and result as rle_erode's.  Device-to-host reads: 3 + L + one per fit_runs attempt (rle_erode's and the total of the
    difference)."""
    return _run_morph('rle_boundary', counts, n, H, W, radius, 0, True, cap)


# ----------------------------------------------------------------------------- Euclidean buffers (csrc/run_disc.hip)
# The most intervals one pass of rle_dilate_disc / rle_erode_disc emits and sorts: 12 bytes each as written
# (int64 key, int32 end), 32 while the sort holds its sorted copy, the permutation and the gathered ends -- 2 GiB at the limit.
# Above it the rows are processed in chunks; a single row above it is refused.
DISC_MAX_INTERVALS = 1 << 26


def _disc_hh(what, hh, H, W):
    """the half-heights of a structuring element as the kernels take them -> (hh cut to R_eff + 1 = min(R, W - 1) + 1 entries
    and to H, R_eff, the frame (columns, rows) an erosion with border 0 loses: (min(R, W), min(hh[0], H)))"""
    try:
        hh = [int(v) for v in hh]
        ok = len(hh) >= 1 and all(v >= 0 for v in hh) and all(a >= b for a, b in zip(hh, hh[1:]))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'{what}: hh must be a non-empty list of non-negative, non-increasing integers (rle.half_heights)')
    R = len(hh) - 1
    Re = min(R, W - 1)
    return [min(v, H) for v in hh[:Re + 1]], Re, (min(R, W), min(hh[0], H))


def _disc_frame(k, H, W, fc, fr, dev):
    """the complement of the rectangle [fc, W - fc) x [fr, H - fr) of every row as intervals of rsp_rle_union: what the outside
    of the canvas, read as background, takes from an erosion.  In the column-major stream the bottom of one column and the top
    of the next are one interval: W - 2 fc + 1 intervals per row, one where the rectangle is empty -> (keys int64, ends int32)"""
    i64 = dict(dtype=torch.int64, device=dev)
    if fc == 0 and fr == 0:
        return torch.zeros((0,), **i64), torch.zeros((0,), dtype=torch.int32, device=dev)
    if 2 * fc >= W or 2 * fr >= H:
        starts, stops = torch.zeros((1,), **i64), torch.full((1,), H * W, **i64)
    else:
        xs = torch.arange(fc, W - fc, **i64)
        starts = torch.cat([torch.zeros((1,), **i64), xs * H + (H - fr)])
        stops = torch.cat([xs * H + fr, torch.full((1,), H * W, **i64)])
        if fr == 0:                                                # nothing between two columns: the side strips alone
            starts, stops = starts[[0, -1]], stops[[0, -1]]
    inst = torch.arange(k, **i64)[:, None] << 31
    return (inst | starts[None, :]).reshape(-1), stops.to(torch.int32).repeat(k)


def _disc_frame_count(H, W, fc, fr):
    if fc == 0 and fr == 0:
        return 0
    if 2 * fc >= W or 2 * fr >= H:
        return 1
    return W - 2 * fc + 1 if fr > 0 else 2


def _disc_dilate(what, lib, cc, cn, k, cap_c, H, W, hh, R, frame, cap, row0):
    """canonical rows -> (counts, n, n on the host, cap) of their dilation united with the frame, or the list of row ranges to
    process one by one when the intervals exceed DISC_MAX_INTERVALS"""
    dev = cn.device
    args = (cc.data_ptr(), cn.data_ptr(), k, cap_c, H, W)
    pcnt = torch.zeros((k,), dtype=torch.int32, device=dev)
    _lib.check(lib.rsp_run_morph_pieces_count(*args, 0, 0, 0, pcnt.data_ptr(), _stream()), "rsp_run_morph_pieces_count")
    poffs, _ = _exclusive_total(pcnt)
    per_row = pcnt.tolist()                                                                          # read 1
    P = sum(per_row)
    if P >= 2 ** 31:
        raise ValueError(f'{what}: {P} column pieces in one call; at most 2^31 - 1 (split the rows)')
    n_frame = _disc_frame_count(H, W, *frame)
    T = _RunIntervals(P, W, dev)
    if P:
        _lib.check(lib.rsp_run_morph_pieces(*args, 0, 0, 0, poffs.data_ptr(), P, T.col.data_ptr(), T.y0.data_ptr(),
                                            T.y1.data_ptr(), _stream()), "rsp_run_morph_pieces")
    sides, n_side, n_emit = [], [0, 0], [0, 0]
    if P and R:
        b_offs = T.offs(k)
        X = T.col[:P] % W
        reach = (torch.clamp(W - 1 - X, max=R).to(torch.int64), torch.clamp(X, max=R).to(torch.int64))
        for d, shift in enumerate((1, -1)):                  # E+ = T(X) - T(X + 1), E- = T(X) - T(X - 1): the count passes
            head = (1, T.col.data_ptr(), T.y0.data_ptr(), T.y1.data_ptr(), P, W, b_offs.data_ptr(), T.y0.data_ptr(),
                    T.y1.data_ptr(), P, k, W, shift, 1)
            cnt = torch.zeros((P,), dtype=torch.int32, device=dev)
            _lib.check(lib.rsp_run_morph_join_count(*head, 0, W, cnt.data_ptr(), _stream()), "rsp_run_morph_join_count")
            sides.append((head, cnt))
        # per row: the parts of E+, of E-, and the intervals they emit (the pieces themselves come on top)
        per_piece = torch.stack([sides[0][1].to(torch.int64), sides[1][1].to(torch.int64),
                                 sides[0][1] * reach[0], sides[1][1] * reach[1]])
        csum = torch.cat([per_piece.new_zeros((4, 1)), torch.cumsum(per_piece, 1)], 1)
        rows = (csum[:, poffs[1:]] - csum[:, poffs[:-1]]).tolist()                                   # read 2
        n_side, n_emit = [sum(rows[0]), sum(rows[1])], [sum(rows[2]), sum(rows[3])]
        per_row = [p + a + b for p, a, b in zip(per_row, rows[2], rows[3])]
    per_row = [p + n_frame for p in per_row]
    total = sum(per_row)
    if max(n_side) >= 2 ** 31:
        raise ValueError(f'{what}: {max(n_side)} exposed pieces in one call; at most 2^31 - 1 (split the rows)')
    if total > DISC_MAX_INTERVALS:
        worst = per_row.index(max(per_row))
        if per_row[worst] > DISC_MAX_INTERVALS:
            raise ValueError(f'{what}: row {row0 + worst} alone emits {per_row[worst]} intervals; at most '
                             f'{DISC_MAX_INTERVALS} in one pass (ops.DISC_MAX_INTERVALS)')
        chunks, a, acc = [], 0, 0
        for i, v in enumerate(per_row):
            if acc + v > DISC_MAX_INTERVALS:
                chunks.append((a, i))
                a, acc = i, 0
            acc += v
        return chunks + [(a, k)]
    keys = torch.empty((max(total, 1),), dtype=torch.int64, device=dev)
    ends = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)
    hh_t = torch.tensor(hh, dtype=torch.int32, device=dev)

    def emit(t, direction, slot_offs, base):
        _lib.check(lib.rsp_run_disc_emit(t.col.data_ptr(), t.y0.data_ptr(), t.y1.data_ptr(), t.P, k, H, W, hh_t.data_ptr(), R,
                                         direction, slot_offs.data_ptr() if slot_offs is not None else 0, base, total,
                                         keys.data_ptr(), ends.data_ptr(), _stream()), "rsp_run_disc_emit")
    emit(T, 0, None, 0)
    base = P
    for d, (head, cnt) in enumerate(sides):
        offs, _ = _exclusive_total(cnt)
        E = _RunIntervals(n_side[d], W, dev)
        _lib.check(lib.rsp_run_morph_join(*head, offs.data_ptr(), E.P, 0, W, H, 0, E.col.data_ptr(), E.y0.data_ptr(),
                                          E.y1.data_ptr(), 0, 0, _stream()), "rsp_run_morph_join")
        XE = E.col[:E.P] % W
        slots, _ = _exclusive_total(torch.clamp(W - 1 - XE if d == 0 else XE, max=R))
        emit(E, 1 if d == 0 else -1, slots, base)
        base += n_emit[d]
    if n_frame:
        fk, fe = _disc_frame(k, H, W, frame[0], frame[1], dev)
        keys[total - k * n_frame:], ends[total - k * n_frame:] = fk, fe
    iv_offs = torch.zeros((k + 1,), dtype=torch.int64, device=dev)
    if total:
        keys, order = torch.sort(keys[:total])
        ends = ends[:total][order].contiguous()
        iv_offs = torch.searchsorted(keys, torch.arange(k + 1, dtype=torch.int64, device=dev) << 31).contiguous()
    return fit_runs(lambda cap: _intervals_to_runs(lib, keys, ends, total, iv_offs, k, H, W, cap), cap)


def _run_disc(what, counts, n, H, W, hh, erode, border, cap, row0=0):
    lib = _lib.load()
    counts, n, k, cap_in, H, W = _rle_rows(what, counts, n, H, W)
    if border not in (0, 1):
        raise ValueError(f'{what}: border must be 0 or 1, got {border!r}')
    hh_cut, R, frame = _disc_hh(what, hh, H, W)
    dev = n.device
    cap = max(int(cap), 2) if cap is not None else cap_in + 2
    if k == 0:
        return torch.zeros((0, cap), dtype=torch.int32, device=dev), n, n.cpu(), cap
    if k * W >= 2 ** 31:
        raise ValueError(f'{what}: {k} rows x {W} columns; column numbers are 32-bit (< 2^31; split the rows)')
    cc, cn = _canonical_rows(lib, counts, n, k, cap_in, H, W)
    if erode:                        # the complement of a canonical row is canonical; a row with n <= 0 is the empty mask by now
        cc, cn = rle_complement(cc, cn)
    out = _disc_dilate(what, lib, cc, cn, k, int(cc.shape[1]), H, W, hh_cut, R, frame if erode and not border else (0, 0), cap,
                       row0)
    if isinstance(out, list):                                    # too many intervals for one pass: row chunks, each on its own
        from .rle import concat_runs
        parts = [_run_disc(what, counts[a:b], n[a:b], H, W, hh, erode, border, cap, row0 + a) for a, b in out]
        c = concat_runs([p[0] for p in parts])
        return c, torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]), int(c.shape[1])
    if not erode:
        return out
    c, m = rle_complement(out[0], out[1])
    return c, m, m.cpu(), int(c.shape[1])


def rle_dilate_disc(counts, n, H, W, hh, cap=None):
    """dilation of every row of a run table (counts int32 [k, cap_in], n int32 [k]: k masks on one (H, W) canvas) by the
    structuring element whose half-heights are `hh` (rle.half_heights: hh[dx] = the rows it reaches above and below its centre
    at column offset dx, non-increasing; the exact disc dx^2 + dy^2 <= r2, or the diamond): a pixel is set iff
    the element centred on it meets the mask, clipped to the canvas -- scipy.ndimage.binary_dilation(M, footprint), the
    squared Euclidean distance to the mask <= r2.  Zero counts anywhere are legal input; a row with n <= 0 is the empty mask;
    hh = [0] returns the canonical form of the rows; columns of hh beyond W - 1 are not read.  -> (counts int32 [k, cap'],
    n int32 [k], n on the host, cap') under fit_runs, canonical COCO run counts; cap: the first capacity (the input's plus two
    when None).  Intervals emitted and sorted: the column pieces + R (|E+| + |E-|), E+- the parts of the pieces with no set
    pixel beside them: linear in R, never in the area.  More than DISC_MAX_INTERVALS: the rows go in chunks, each with the
    reads of a call of its own after the two that found it out; a single row above it is refused (ValueError).
    Device-to-host reads, whatever k is: 2 + one per fit_runs attempt (the pieces per row; the exposed parts and their
    intervals per row); 1 + ... for a table without pieces or with hh = [0]; k = 0 launches nothing and reads nothing."""
    return _run_disc('rle_dilate_disc', counts, n, H, W, hh, False, 1, cap)


def rle_erode_disc(counts, n, H, W, hh, border=0, cap=None):
    """erosion of every row by the same structuring element: a pixel stays iff every pixel of the element centred on it is set,
    the outside of the canvas counting as `border` (0 or 1) -- scipy.ndimage.binary_erosion(M, footprint,
    border_value=border).  It is the complement (rle_complement) of the dilation of the complement; with border 0 the outside
    takes exactly the frame of len(hh) - 1 columns and hh[0] rows, which joins the dilation as W - 2 R + 1 intervals per row
    before the sort (no dense mask; the empty mask where the canvas is no larger than two frames).  Input, result and chunking
    as rle_dilate_disc's.  Device-to-host reads: rle_dilate_disc's and one more (n of the complemented result)."""
    return _run_disc('rle_erode_disc', counts, n, H, W, hh, True, border, cap)


def rle_minus(counts_a, n_a, counts_b, n_b, H, W, cap=None):
    """row i of table A minus row i of table B, both on one (H, W) canvas (the band M - erode(M) of DESIGN §14.16): the column
    pieces of both (rsp_run_morph_pieces), rsp_run_morph_join's op 1 emitting keys, rsp_rle_union.  Zero counts anywhere are
    legal; a row with n <= 0 is the empty mask.  -> (counts, n, n on the host, cap) under fit_runs.  Device-to-host reads: 2 +
    one per fit_runs attempt (the pieces of both tables, the total of the difference); k = 0 reads nothing."""
    lib = _lib.load()
    counts_a, n_a, k, cap_a, H, W = _rle_rows('rle_minus', counts_a, n_a, H, W)
    counts_b, n_b, kb, cap_b, _, _ = _rle_rows('rle_minus', counts_b, n_b, H, W)
    if kb != k or n_b.device != n_a.device:
        raise ValueError(f'rle_minus: {k} rows minus {kb} rows; the tables pair row by row on one device')
    dev = n_a.device
    cap = max(int(cap), 2) if cap is not None else cap_a + 2
    if k == 0:
        return torch.zeros((0, cap), dtype=torch.int32, device=dev), n_a, n_a.cpu(), cap
    if k * W >= 2 ** 31:
        raise ValueError(f'rle_minus: {k} rows x {W} columns; column numbers are 32-bit (< 2^31; split the rows)')
    sides = [(_canonical_rows(lib, c, m, k, cp, H, W), cp + 1) for c, m, cp in ((counts_a, n_a, cap_a), (counts_b, n_b, cap_b))]
    cnts = torch.zeros((2, k), dtype=torch.int32, device=dev)
    for i, ((c, m), cp) in enumerate(sides):
        _lib.check(lib.rsp_run_morph_pieces_count(c.data_ptr(), m.data_ptr(), k, cp, H, W, 0, 0, 0, cnts[i].data_ptr(),
                                                  _stream()), "rsp_run_morph_pieces_count")
    offs, totals = _exclusive_total(cnts)
    totals = totals.tolist()                                                                         # read 1
    if max(totals) >= 2 ** 31:
        raise ValueError(f'rle_minus: {max(totals)} column pieces in one call; at most 2^31 - 1 (split the rows)')
    tables = []
    for i, ((c, m), cp) in enumerate(sides):
        t = _RunIntervals(totals[i], W, dev)
        _lib.check(lib.rsp_run_morph_pieces(c.data_ptr(), m.data_ptr(), k, cp, H, W, 0, 0, 0, offs[i].data_ptr(), t.P,
                                            t.col.data_ptr(), t.y0.data_ptr(), t.y1.data_ptr(), _stream()), "rsp_run_morph_pieces")
        tables.append(t)
    E = _run_morph_join(lib, 1, tables[0], tables[1], k, 0, 1, 0, W, H, True)                        # read 2
    iv_offs = torch.searchsorted(E.keys[:E.P], torch.arange(k + 1, dtype=torch.int64, device=dev) << 31).contiguous()
    return fit_runs(lambda cap: _intervals_to_runs(lib, E.keys, E.ends, E.P, iv_offs, k, H, W, cap), cap)


# ----------------------------------------------------------------------------- planar layers (csrc/run_flatten.hip)
def _flatten_rank(what, rank, k, dev):
    if not isinstance(rank, torch.Tensor) or rank.dtype != torch.int32 or rank.dim() != 1 or rank.shape[0] != k \
            or rank.device != dev:
        raise ValueError(f'{what}: rank must be int32 [{k}] on the device of the counts')
    return rank.contiguous()


def _column_pieces(lib, rp, H, W):
    """the column-ordered copy of a piece table with P > 0 pieces (one device key sort, rsp_run_flatten_columns) ->
    (cpieces int32 [4, P] sorted by (x, y0), col_offs int32 [W + 1], reach int32 [P]).  No host read."""
    P, dev = rp.P, rp.pieces.device
    px, py0 = rp.pieces[0].to(torch.int64), rp.pieces[1].to(torch.int64)
    skeys = torch.sort(((px * H + py0) << 31) | torch.arange(P, dtype=torch.int64, device=dev))[0].contiguous()
    cpieces = rp.pieces[:, skeys & 0x7fffffff].contiguous()
    col_offs = torch.empty((W + 1,), dtype=torch.int32, device=dev)
    reach = torch.empty((P,), dtype=torch.int32, device=dev)
    _lib.check(lib.rsp_run_flatten_columns(skeys.data_ptr(), cpieces.data_ptr(), P, H, W, col_offs.data_ptr(),
                                           reach.data_ptr(), _stream()), "rsp_run_flatten_columns")
    return cpieces, col_offs, reach


def rle_flatten(counts, n, H, W, rank, cap=None):
    """the rows of a run table (counts int32 [k, cap_in], n int32 [k]: k masks on one (H, W) canvas) made pairwise disjoint
    (DESIGN §14.14): rank int32 [k] on the device, a permutation of 0 .. k - 1 where 0 wins (rle.flatten_runs checks it;
    here it is only compared); row i of the result is M_i minus every M_j with rank[j] < rank[i] -- the per-pixel argmax of
    score x mask of MaskFormerFusionHead.panoptic_postprocess for binary masks, without a dense mask.  Zero counts anywhere
    are legal input; a row with n <= 0 is the empty mask.  -> (counts int32 [k, cap'], n int32 [k], cap'), canonical COCO run
    counts (an emptied row is one count H * W); cap: the first capacity (the input's plus two when None): a subtraction
    splits runs, so a row may need more counts than it came with, and fit_runs grows the capacity.
    Device-to-host reads, whatever k is: three -- the pieces (run_pieces), the survivors' total, and n per fit_runs attempt
    (one more per retry); two when the table has no piece.  One device key sort (the column order of the pieces)."""
    lib = _lib.load()
    counts, n, k, cap_in, H, W = _rle_rows('rle_flatten', counts, n, H, W)
    dev = n.device
    rank = _flatten_rank('rle_flatten', rank, k, dev)
    cap = max(int(cap), 2) if cap is not None else cap_in + 2
    if k == 0:
        return torch.zeros((0, cap), dtype=torch.int32, device=dev), n, cap
    rp = run_pieces(counts, n, H, W, what='rle_flatten')                                              # read 1
    P = rp.P
    keys, ends, total = None, None, 0
    iv_offs = torch.zeros((k + 1,), dtype=torch.int64, device=dev)
    if P:
        cpieces, col_offs, reach = _column_pieces(lib, rp, H, W)
        head =(rp.pieces.data_ptr(), cpieces.data_ptr(), col_offs.data_ptr(), reach.data_ptr(), rank.data_ptr(), P, k, H, W)
        cnt = torch.empty((P,), dtype=torch.int32, device=dev)
        _lib.check(lib.rsp_run_flatten_count(*head, cnt.data_ptr(), _stream()), "rsp_run_flatten_count")
        out_offs, total = _exclusive_total(cnt)
        total = int(total.item())                                                                    # read 2
        if total >= 2 ** 31:
            raise ValueError(f'rle_flatten: {total} surviving intervals in one call; at most 2^31 - 1 (split the canvas)')
        if total:
            keys = torch.empty((total,), dtype=torch.int64, device=dev)
            ends = torch.empty((total,), dtype=torch.int32, device=dev)
            _lib.check(lib.rsp_run_flatten_write(*head, out_offs.data_ptr(), total, keys.data_ptr(), ends.data_ptr(), _stream()),
                       "rsp_run_flatten_write")
        iv_offs = out_offs[rp.piece_offs].contiguous()
    out, n_out, _, cap = fit_runs(lambda cap: _intervals_to_runs(lib, keys, ends, total, iv_offs, k, H, W, cap), cap)
    return out, n_out, cap


def rle_label_map(counts, n, H, W, ids=None):
    """the label map of a run table whose rows are pairwise DISJOINT (what rle_flatten returns): int32 [H, W] on the device,
    ids[i] (int32 [k] on the device; i + 1 when None) on the pixels of row i, 0 elsewhere (rsp_run_flatten_paint).  The
    kernel writes the column-major stream, int32 [W, H], in which every ones-run is contiguous; the result is its .T view.
    Where rows overlap a pixel takes the id of one of them.  One device-to-host read (the number of ones-runs)."""
    lib = _lib.load()
    counts, n, k, cap, H, W = _rle_rows('rle_label_map', counts, n, H, W)
    dev = n.device
    if ids is None:
        ids = torch.arange(1, k + 1, dtype=torch.int32, device=dev)
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 1 or ids.shape[0] != k or ids.device != dev:
        raise ValueError(f'rle_label_map: ids must be int32 [{k}] on the device of the counts')
    ids = ids.contiguous()
    labels = torch.empty((W, H), dtype=torch.int32, device=dev)
    keys, ends, total = None, None, 0
    if k:
        rows = torch.arange(k, dtype=torch.int32, device=dev)
        keys, ends, _, total = _rle_intervals(lib, counts, n, k, cap, H, W, rows, rows, (n.clamp(0, cap) // 2).to(torch.int64))
    _lib.check(lib.rsp_run_flatten_paint(keys.data_ptr() if total else 0, ends.data_ptr() if total else 0, total, ids.data_ptr(),
                                         k, H, W, labels.data_ptr(), _stream()), "rsp_run_flatten_paint")
    return labels.t()


# ----------------------------------------------------------------------------- polygon rasterisation (csrc/poly_raster.hip)
POLY_RASTER_MAX_COORD = CONST['RSP_POLY_RASTER_MAX_COORD']        # |(int)(5 x + .5)| of every coordinate
POLY_RASTER_MAX_POINTS = CONST['RSP_POLY_RASTER_MAX_POINTS']      # walk points of one call
POLY_RASTER_MAX_GROUPS = CONST['RSP_POLY_RASTER_MAX_GROUPS']      # rows of one call: one block each


def poly_raster_launcher(verts, ring_offs, ring_group, group_hw, compact=True):
    """The stages of DESIGN §14.11 up to the sorted crossing keys -> the `launch(cap)` of fit_runs for rsp_poly_raster_runs.
    verts float64 [V, 2] = (x, y), ring_offs int64 [R + 1], ring_group int32 [R] (non-decreasing), group_hw int32 [G, 2] =
    (h, w) per group, all on one device.  Three device-to-host reads (are the coordinates finite; then walk points, largest
    scaled coordinate, largest canvas and the layout flags in one; then the number of crossings, inside the compaction that
    drops the slots of walk points without one in front of the sort -- compact=False sorts them along, as the last keys, and
    saves the read: tools/bench_poly_raster.py measures both); `launch` itself reads nothing.  Refuses NaN / inf (ValueError,
    before any launch) and what the C entries refuse (ValueError with the limit named)."""
    lib = _lib.load()
    dev = verts.device
    if verts.dtype != torch.float64 or verts.dim() != 2 or verts.shape[1] != 2:
        raise ValueError('poly_raster: verts must be float64 [V, 2] = (x, y)')
    if ring_offs.dtype != torch.int64 or ring_offs.dim() != 1 or ring_offs.shape[0] < 1 or ring_group.dtype != torch.int32 \
            or ring_group.dim() != 1 or ring_group.shape[0] != ring_offs.shape[0] - 1:
        raise ValueError('poly_raster: ring_offs must be int64 [R + 1] and ring_group int32 [R]')
    if group_hw.dtype != torch.int32 or group_hw.dim() != 2 or group_hw.shape[1] != 2:
        raise ValueError('poly_raster: group_hw must be int32 [G, 2] = (h, w) per group')
    if not (ring_offs.device == ring_group.device == group_hw.device == dev):
        raise ValueError('poly_raster: verts, ring_offs, ring_group and group_hw must be on one device')
    V, R, G = int(verts.shape[0]), int(ring_group.shape[0]), int(group_hw.shape[0])
    if G > POLY_RASTER_MAX_GROUPS:
        raise ValueError(f'poly_raster: {G} groups in one call; at most {POLY_RASTER_MAX_GROUPS} (split the call)')
    verts, ring_offs, ring_group, group_hw = (t.contiguous() for t in (verts, ring_offs, ring_group, group_hw))
    i64 = dict(dtype=torch.int64, device=dev)
    if V and not bool(torch.isfinite(verts).all()):
        raise ValueError('poly_raster: a polygon coordinate is NaN or infinite')
    if V and not R:
        raise ValueError('poly_raster: vertices without a ring')
    # the layout is checked on the device and read with the sizes below; the kernels clamp whatever the arrays hold
    bad_offs = (ring_offs[0] != 0) | (ring_offs[-1] != V) | (ring_offs[1:] < ring_offs[:-1]).any()
    bad_group = ((ring_group[1:] < ring_group[:-1]).any() | (ring_group[0] < 0) | (ring_group[-1] >= G)) if R else bad_offs & False
    scaled = torch.zeros((max(V, 1), 2), dtype=torch.int32, device=dev)
    edge_pts = torch.zeros((max(V, 1),), **i64)
    group_px = torch.zeros((max(G, 1),), **i64)
    _lib.check(lib.rsp_poly_raster_edges(verts.data_ptr(), ring_offs.data_ptr(), group_hw.data_ptr(), R, V, G, scaled.data_ptr(),
                                         edge_pts.data_ptr(), group_px.data_ptr(), _stream()), "rsp_poly_raster_edges")
    edge_offs, total = _exclusive_total(edge_pts[:V])
    T, coord_max, pixels_max, bad_offs, bad_group = torch.stack(
        [total, scaled.abs().max().to(torch.int64), group_px.max(), bad_offs.to(torch.int64),
         bad_group.to(torch.int64)]).tolist()
    if bad_offs:
        raise ValueError('poly_raster: ring_offs must ascend from 0 to the number of vertices')
    if bad_group:
        raise ValueError('poly_raster: ring_group must be non-decreasing and inside [0, G)')
    if pixels_max > 2 ** 31 - 1:
        raise ValueError('poly_raster: a group canvas is empty or has 2^31 pixels or more; COCO run counts are 32-bit')
    if coord_max > POLY_RASTER_MAX_COORD:
        raise ValueError(f'poly_raster: a coordinate scales beyond +-{POLY_RASTER_MAX_COORD} (5 x: |x| up to about 3.3 million px)')
    if T > POLY_RASTER_MAX_POINTS:
        raise ValueError(f'poly_raster: {T} walk points in one call; at most {POLY_RASTER_MAX_POINTS} (split the rings)')
    keys = torch.empty((max(T, 1),), **i64)
    _lib.check(lib.rsp_poly_raster_crossings(scaled.data_ptr(), ring_offs.data_ptr(), ring_group.data_ptr(), group_hw.data_ptr(),
                                             edge_offs.data_ptr(), R, V, G, T, coord_max, pixels_max, keys.data_ptr(), _stream()),
               "rsp_poly_raster_crossings")
    walk = T
    keys = keys[:T]
    if compact and T:                       # most walk points cross no pixel column: drop their slots in front of the sort
        keys = keys[keys != CONST['RSP_POLY_RASTER_NO_KEY']]
    keys = torch.sort(keys)[0].contiguous() if T else keys
    T = int(keys.shape[0])
    key_offs = torch.searchsorted(keys, torch.arange(G + 1, **i64) << 32).contiguous()

    def launch(cap):
        cap = max(int(cap), 1)
        counts = torch.empty((max(G, 1), cap), dtype=torch.int32, device=dev)
        n = torch.zeros((max(G, 1),), dtype=torch.int32, device=dev)
        _lib.check(lib.rsp_poly_raster_runs(keys.data_ptr(), T, key_offs.data_ptr(), group_hw.data_ptr(), G, pixels_max,
                                            counts.data_ptr(), n.data_ptr(), cap, _stream()), "rsp_poly_raster_runs")
        return counts[:G], n[:G]
    launch.walk_points, launch.crossings = walk, key_offs[-1]          # the walk points, and how many of them cross (on the device)
    return launch


def poly_raster(verts, ring_offs, ring_group, group_hw, cap=64):
    """rings -> (counts int32 [G, cap'], n int32 [G], n on the host, cap'): maskApi.c rleFrPoly's run counts of every group of
    rings on its own (h, w) canvas, even-odd over the rings of a group (poly_raster_launcher under fit_runs: the crossings are
    found and sorted once, only the last stage runs again when a row did not fit `cap`)."""
    return fit_runs(poly_raster_launcher(verts, ring_offs, ring_group, group_hw), cap)


# (th, tw) of rsp_mask_remove_small_regions' tile-local labelling
MASK_REGION_TILE = (CONST['RSP_MASK_REGION_TILE_H'], CONST['RSP_MASK_REGION_TILE_W'])
MASK_REGION_MODES = {'holes': 1, 'islands': 2, 'both': 3}
# the labelling keeps two int32 per pixel: 8 bytes x k x H x W of workspace.  remove_small_regions splits k so that one call
# stays under this (64 masks of 1024 x 1024 are 512 MiB); a single mask larger than that gets its workspace all the same.
MASK_REGIONS_WORKSPACE_LIMIT_BYTES = 1 << 30


def remove_small_regions(masks, min_area, mode='both'):
    """segment-anything `remove_small_regions` for k masks on the device (rsp_mask_remove_small_regions): masks bool / uint8
    [k, H, W] (non-zero = set), mode 'holes' (8-connected components of the zeros smaller than min_area are set), 'islands'
    (components of the ones smaller than min_area are cleared; if all are, the largest stays -- among equals the one with
    the lowest first pixel) or 'both' (holes, then islands of the filled mask).  Returns (out bool [k, H, W], info int32
    [k, 8] = changed by holes, changed by islands, x0, y0, x1, y1 (inclusive maxima; zeros when empty), population count,
    status).  No host read: whoever reads `info` checks that status is 0 (`check_region_status`)."""
    lib = _lib.load()
    if mode not in MASK_REGION_MODES:
        raise ValueError(f"remove_small_regions: mode must be one of {sorted(MASK_REGION_MODES)}, got {mode!r}")
    if not isinstance(masks, torch.Tensor) or masks.dtype not in (torch.bool, torch.uint8) or masks.dim() != 3:
        raise ValueError("remove_small_regions: masks must be a bool or uint8 [k, H, W] tensor")
    if not _is_device(masks):
        raise ValueError(f"remove_small_regions: masks must be on the HIP device, got {masks.device}")
    if int(min_area) != min_area or int(min_area) < 0 or int(min_area) >= 2 ** 31:
        raise ValueError(f"remove_small_regions: min_area must be an integer in [0, 2^31), got {min_area!r}")
    k, H, W = (int(s) for s in masks.shape)
    if H < 1 or W < 1:
        raise ValueError(f"remove_small_regions: empty masks ({H} x {W})")
    if H * W >= 2 ** 31:
        raise ValueError(f"remove_small_regions: a {H} x {W} mask has {H * W} pixels; labels are 32-bit (< 2^31 pixels)")
    if not masks.is_contiguous():
        raise ValueError("remove_small_regions: masks must be contiguous")
    dev = masks.device
    out = torch.empty((k, H, W), dtype=torch.bool, device=dev)
    info = torch.empty((k, 8), dtype=torch.int32, device=dev)
    if k == 0:
        return out, info
    per = int(lib.rsp_mask_regions_workspace_bytes(1, H, W))
    step = max(1, min(k, MASK_REGIONS_WORKSPACE_LIMIT_BYTES // per))
    ws = torch.empty((int(lib.rsp_mask_regions_workspace_bytes(step, H, W)) // 8,), dtype=torch.int64, device=dev)
    for i in range(0, k, step):
        kc = min(step, k - i)
        _lib.check(lib.rsp_mask_remove_small_regions(masks[i:i + kc].data_ptr(), kc, H, W, int(min_area),
                                                     MASK_REGION_MODES[mode], ws.data_ptr(), out[i:i + kc].data_ptr(),
                                                     info[i:i + kc].data_ptr(), _stream()), "rsp_mask_remove_small_regions")
    return out, info


def check_region_status(status):
    """`status` = column 7 of remove_small_regions' info, ON THE HOST (list / array / tensor): non-zero means that a find /
    union loop of the labelling reached its step cap and the result is invalid"""
    bad = [i for i, s in enumerate(list(status)) if int(s) != 0]
    if bad:
        raise RuntimeError(f"rsp_mask_remove_small_regions: the labelling of mask(s) {bad[:8]} reached its iteration cap "
                           "(status != 0); the result is invalid")


def nms_flat(boxes, scores, labels, iou_thr):
    """mmcv.ops.batched_nms(boxes [n, 4], scores [n], labels [n], dict(type='nms', iou_threshold=iou_thr)) on flat device
    tensors through rsp_batched_nms with B = 1: returns keep (int64 [m], indices into the inputs in descending score
    order).  One host read (the number kept)."""
    n = int(boxes.shape[0])
    dev = boxes.device
    if n == 0:
        return torch.zeros((0,), dtype=torch.int64, device=dev)
    if n > NMS_MAX_CANDIDATES:
        raise ValueError(f'nms_flat: {n} instances, rsp_batched_nms holds {NMS_MAX_CANDIDATES} candidates at most')
    cand = (boxes.to(torch.float32).contiguous().view(1, n, 4), scores.to(torch.float32).contiguous().view(1, n),
            labels.to(torch.int32).contiguous().view(1, n), torch.arange(n, dtype=torch.int32, device=dev).view(1, n),
            torch.full((1,), n, dtype=torch.int32, device=dev))
    r = batched_nms(cand, 1, n, float(iou_thr), n)
    m = int(r['count'][0].item())
    return r['keep'][0, :m].to(torch.int64)


# ----------------------------------------------------------------------------- COCO evaluation (csrc/cocoeval.hip)
def rle_from_string(flat, offs, cap=1024):
    """COCO compressed strings flat[offs[i]:offs[i + 1]] (uint8 / int64 device tensors) -> (counts int32 [k, cap'],
    n int32 [k]) on the device (rsp_rle_from_string); grows `cap` and retries when a string holds more counts."""
    lib = _lib.load()
    k = max(offs.shape[0] - 1, 0)
    dev = offs.device

    def launch(cap):
        counts = torch.empty((max(k, 1), cap), dtype=torch.int32, device=dev)
        n = torch.zeros((max(k, 1),), dtype=torch.int32, device=dev)
        if k:
            _lib.check(lib.rsp_rle_from_string(_ptr(flat), offs.data_ptr(), k, cap, counts.data_ptr(), n.data_ptr(),
                                               _stream()), "rsp_rle_from_string")
        return counts[:k], n[:k]
    return fit_runs(launch, cap)[:2]


def rle_to_bits(counts, n, word_offs):
    """run counts (int32 [k, cap], n int32 [k]) -> (bits int64 [word_offs[k]] (64-bit words, mask i at
    word_offs[i]..word_offs[i + 1]), area int64 [k], wrange int32 [k, 2]) (rsp_rle_to_bits)."""
    lib = _lib.load()
    k = n.shape[0]
    dev = n.device
    nw = int(word_offs[-1].item()) if k else 0
    bits = torch.empty((max(nw, 1),), dtype=torch.int64, device=dev)
    area = torch.empty((max(k, 1),), dtype=torch.int64, device=dev)
    wrange = torch.empty((max(k, 1), 2), dtype=torch.int32, device=dev)
    if k:
        _lib.check(lib.rsp_rle_to_bits(counts.data_ptr(), n.data_ptr(), k, counts.shape[1], word_offs.data_ptr(),
                                       bits.data_ptr(), area.data_ptr(), wrange.data_ptr(), _stream()), "rsp_rle_to_bits")
    return bits, area[:k], wrange[:k]


COCO_IOU_BBOX, COCO_IOU_SEGM = CONST['RSP_COCO_IOU_BBOX'], CONST['RSP_COCO_IOU_SEGM']
COCO_UNIT_BYTES = ctypes.sizeof(_lib.RspCocoUnit)


def _units_ptr(units):
    """the device address of a `coco_units` tensor as the `const RspCocoUnit*` the entry points declare"""
    return ctypes.cast(units.data_ptr(), ctypes.POINTER(_lib.RspCocoUnit))


def coco_units(dt0, gt0, out0, nd, ng, nwords, device):
    """RspCocoUnit records (include/rsp_hip.h) from per-unit numpy columns -> uint8 device tensor."""
    import numpy as np
    rec = np.zeros(len(nd), dtype=np.dtype(_lib.RspCocoUnit))
    rec['dt0'], rec['gt0'], rec['out0'], rec['nd'], rec['ng'], rec['nwords'] = dt0, gt0, out0, nd, ng, nwords
    return torch.from_numpy(rec.view(np.uint8).copy()).to(device)


def coco_iou(units, n_iou, mode, *, gt_crowd, dt_box=None, gt_box=None, dt_bits=None, gt_bits=None, dt_woff=None,
             gt_woff=None, dt_wrange=None, gt_wrange=None, dt_area=None, gt_area=None):
    """IoU blocks of the units (uint8 device tensor holding RspCocoUnit records, `coco_units`) -> float64 [n_iou]."""
    lib = _lib.load()
    dev = units.device
    iou = torch.zeros((max(n_iou, 1),), dtype=torch.float64, device=dev)
    nu = units.numel() // COCO_UNIT_BYTES
    if nu:
        _lib.check(lib.rsp_coco_iou(_units_ptr(units), nu, mode, _ptr(dt_bits), _ptr(gt_bits), _ptr(dt_woff),
                                    _ptr(gt_woff), _ptr(dt_wrange), _ptr(gt_wrange), _ptr(dt_area), _ptr(gt_area),
                                    _ptr(dt_box), _ptr(gt_box), gt_crowd.data_ptr(), iou.data_ptr(), _stream()),
                   "rsp_coco_iou")
    return iou[:n_iou]


def coco_match(units, iou, gt_area, gt_crowd, gt_id, dt_area, area_rng, thrs, n_dt):
    """evaluateImg for every unit x area range x threshold (rsp_coco_match) -> (dtm int64 [A, T, n_dt],
    dtig uint8 [A, T, n_dt], npig int32 [n_units, A]).  Per-dt / per-gt inputs hold at least one element."""
    lib = _lib.load()
    dev = units.device
    nu = units.numel() // COCO_UNIT_BYTES
    A, T = area_rng.shape[0], thrs.shape[0]
    n_gt = gt_area.shape[0]
    ws = torch.empty((max(n_gt * A * T, 1),), dtype=torch.uint8, device=dev)
    dtm = torch.zeros((A, T, max(n_dt, 1)), dtype=torch.int64, device=dev)
    dtig = torch.zeros((A, T, max(n_dt, 1)), dtype=torch.uint8, device=dev)
    npig = torch.zeros((max(nu, 1), A), dtype=torch.int32, device=dev)
    if nu:
        _lib.check(lib.rsp_coco_match(_units_ptr(units), nu, iou.data_ptr(), gt_area.data_ptr(), gt_crowd.data_ptr(),
                                      gt_id.data_ptr(), dt_area.data_ptr(), area_rng.data_ptr(), A, thrs.data_ptr(), T,
                                      n_dt, ws.data_ptr(), dtm.data_ptr(), dtig.data_ptr(), npig.data_ptr(), _stream()),
                   "rsp_coco_match")
    return dtm[:, :, :n_dt], dtig[:, :, :n_dt], npig[:nu]


# ----------------------------------------------------------------------------- run-domain mask IoU (csrc/coco_iou_runs.hip)
def run_prefix(counts, n, check=True):
    """run table (counts int32 [k, cap], n int32 [k]; any canvas, any counts) -> (workspace int32 [k, cap]: ones pixels in
    front of each ones-run and the run's pixel start, area int64 [k] = rleArea, extent int32 [k, 2] = (first set pixel, one
    past the last set pixel) of the column-major stream, (0, 0) for a row without one) (rsp_run_prefix).  A negative n is a
    row that did not fit its producer: ValueError (check=True: one device-to-host read; check=False leaves the test to the
    caller and reads nothing)."""
    lib = _lib.load()
    counts, n, k, cap = _rle_rows('run_prefix', counts, n)[:4]
    dev = n.device
    if check and k and bool((n < 0).any()):
        raise ValueError('run_prefix: a row with negative n did not fit its producer (ops.fit_runs retries those)')
    ws = torch.empty((max(int(lib.rsp_run_prefix_workspace_bytes(k, cap)) // 4, 1),), dtype=torch.int32, device=dev)
    area = torch.zeros((max(k, 1),), dtype=torch.int64, device=dev)
    extent = torch.zeros((max(k, 1), 2), dtype=torch.int32, device=dev)
    if k:
        _lib.check(lib.rsp_run_prefix(counts.data_ptr(), n.data_ptr(), k, cap, ws.data_ptr(), area.data_ptr(),
                                      extent.data_ptr(), _stream()), "rsp_run_prefix")
    return ws[:k * cap].view(k, cap), area[:k], extent[:k]


def coco_iou_runs(units, n_iou, dt_runs, gt_runs, gt_crowd, dt_prefix=None, gt_prefix=None, info=None):
    """IoU blocks of the units (`coco_units`, ascending in out0) from two run tables dt_runs / gt_runs = (counts, n) ->
    float64 [n_iou], the doubles of `coco_iou` in SEGM mode without a bit plane: run_prefix of both tables
    (or what it returned, as dt_prefix / gt_prefix), the extent filter with one lane per pair, the alive pairs compacted with
    torch, one wave per survivor for the walk.  One device-to-host read: the number of survivors, with the flags of a
    negative n (ValueError) next to it.  info (a dict) receives pairs / survivors."""
    lib = _lib.load()
    dev = units.device
    (dc, dn), (gc, gn) = _rle_rows('coco_iou_runs', *dt_runs)[:2], _rle_rows('coco_iou_runs', *gt_runs)[:2]
    iou = torch.zeros((max(n_iou, 1),), dtype=torch.float64, device=dev)
    nu = units.numel() // COCO_UNIT_BYTES
    n_dt, n_gt = int(dn.shape[0]), int(gn.shape[0])
    bad = ((dn < 0).any() if n_dt else torch.zeros((), dtype=torch.bool, device=dev)) | \
        ((gn < 0).any() if n_gt else torch.zeros((), dtype=torch.bool, device=dev))
    if not (nu and n_iou and n_dt and n_gt):
        if bool(bad):
            raise ValueError('coco_iou_runs: a row with negative n did not fit its producer (ops.fit_runs retries those)')
        if info is not None:
            info.update(pairs=0, survivors=0)
        return iou[:n_iou]
    d_ws, d_area, d_ext = dt_prefix if dt_prefix is not None else run_prefix(dc, dn, check=False)
    g_ws, g_area, g_ext = gt_prefix if gt_prefix is not None else run_prefix(gc, gn, check=False)
    alive = torch.empty((n_iou,), dtype=torch.int64, device=dev)
    _lib.check(lib.rsp_coco_iou_runs_filter(_units_ptr(units), nu, n_iou, d_ext.data_ptr(), n_dt, g_ext.data_ptr(), n_gt,
                                            alive.data_ptr(), iou.data_ptr(), _stream()), "rsp_coco_iou_runs_filter")
    live = alive >= 0
    S, bad = torch.stack([live.sum(), bad.to(torch.int64)]).tolist()      # the read of the call: the number of survivors
    if bad:
        raise ValueError('coco_iou_runs: a row with negative n did not fit its producer (ops.fit_runs retries those)')
    slots = torch.nonzero_static(live, size=S).view(-1) if S else None
    if S:
        _lib.check(lib.rsp_coco_iou_runs(slots.data_ptr(), S, n_iou, alive.data_ptr(),
                                         dc.data_ptr(), dn.data_ptr(), n_dt, int(dc.shape[1]), d_ws.data_ptr(),
                                         d_area.data_ptr(), d_ext.data_ptr(),
                                         gc.data_ptr(), gn.data_ptr(), n_gt, int(gc.shape[1]), g_ws.data_ptr(),
                                         g_area.data_ptr(), g_ext.data_ptr(), gt_crowd.data_ptr(), iou.data_ptr(),
                                         _stream()), "rsp_coco_iou_runs")
    if info is not None:
        info.update(pairs=int(n_iou), survivors=S)
    return iou[:n_iou]


# ----------------------------------------------------------------------------- query prompter ops
def groupnorm(x, gamma, beta, groups, eps=1e-5, relu=False, add=None):
    """GroupNorm on channels-last [B, ..., C]; `add` (same shape) is added after the norm."""
    lib = _lib.load()
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    y = torch.empty_like(x)
    ws = torch.empty((B * groups * 2,), dtype=torch.float64, device=x.device)
    _timed('groupnorm_kernels', 0, 12.0 * x.numel(),
           lambda: _lib.check(lib.rsp_groupnorm_nhwc(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(add),
                                                     y.data_ptr(), ws.data_ptr(), B, HW, C, groups, eps,
                                                     1 if relu else 0, _stream()), "rsp_groupnorm_nhwc"))
    return y


def resize_bilinear(x_nhwc, size):
    lib = _lib.load()
    B, H, W, C = x_nhwc.shape
    y = torch.empty((B, size[0], size[1], C), dtype=torch.float32, device=x_nhwc.device)
    _lib.check(lib.rsp_resize_bilinear_nhwc(x_nhwc.data_ptr(), y.data_ptr(), B, H, W, size[0], size[1], C, _stream()),
               "rsp_resize_bilinear_nhwc")
    return y


def msdeform_attn(value, offs_weights, ref_points, B, Ntok, level_hw, head_dim=16):
    """value [B*Ntok, 8*head_dim] -> sampled [B*Ntok, 8*head_dim] (before output_proj); head_dim 16 | 32"""
    import ctypes
    lib = _lib.load()
    if value.shape[-1] != 8 * head_dim:
        raise ValueError(f'msdeform_attn: value rows of {value.shape[-1]} channels, expected 8 x {head_dim}')
    out = torch.empty((B * Ntok, 8 * head_dim), dtype=torch.float32, device=value.device)
    arr = (ctypes.c_int * (2 * len(level_hw)))(*[int(v) for hw in level_hw for v in hw])
    _timed('msda_kernel', 0, 4.0 * out.numel() * 50,
           lambda: _lib.check(lib.rsp_msdeform_attn_ex(value.data_ptr(), offs_weights.data_ptr(), offs_weights.shape[-1],
                                                       ref_points.data_ptr(), out.data_ptr(), B, Ntok, len(level_hw), arr,
                                                       head_dim, _stream()), "rsp_msdeform_attn_ex"))
    return out


def query_attn_mask(mask_pred_plus, size):
    """mask_pred_plus [B, Nq, Hs, Ws] -> uint8 [B, Nq, h*w] (1 = blocked), fully blocked rows cleared."""
    lib = _lib.load()
    B, Nq, Hs, Ws = mask_pred_plus.shape
    m = torch.empty((B, Nq, size[0] * size[1]), dtype=torch.uint8, device=mask_pred_plus.device)
    _lib.check(lib.rsp_query_attn_mask(mask_pred_plus.data_ptr(), m.data_ptr(), B * Nq, Hs, Ws, size[0], size[1],
                                       _stream()), "rsp_query_attn_mask")
    return m


def sam_mask_embed(mask_pred_plus, emb_rows, roi_img, prm, he, we, eps=1e-6):
    """mask_pred_plus [R, 4he, 4we]; emb_rows [B*he*we, C]; prm: dict of the SamMaskEmbedding tensors."""
    lib = _lib.load()
    R = mask_pred_plus.shape[0]
    C = emb_rows.shape[-1]
    out = torch.empty((R * he * we, C), dtype=torch.float32, device=emb_rows.device)
    d = _lib.RspMaskEmbedDesc()
    d.mask_pred_plus, d.image_embeddings, d.roi_img = mask_pred_plus.data_ptr(), emb_rows.data_ptr(), roi_img.data_ptr()
    for k in ('conv1_w', 'conv1_b', 'ln1_w', 'ln1_b', 'conv2_w', 'conv2_b', 'ln2_w', 'ln2_b', 'conv3_w', 'conv3_b'):
        setattr(d, k, prm[k].data_ptr())
    d.out, d.R, d.he, d.we, d.C, d.eps = out.data_ptr(), R, he, we, C, eps
    _timed('mask_embed_kernel', 0, 4.0 * out.numel(),
           lambda: _lib.check(lib.rsp_sam_mask_embed(d, _stream()), "rsp_sam_mask_embed"))
    return out


def query_topk(cls, k):
    """cls [B, Nq, nc+1] logits -> (scores [B,k], flat index [B,k] into Nq*nc), score desc / index asc."""
    lib = _lib.load()
    B, Nq, nc1 = cls.shape
    sc = torch.empty((B, k), dtype=torch.float32, device=cls.device)
    fl = torch.empty((B, k), dtype=torch.int32, device=cls.device)
    _lib.check(lib.rsp_query_topk(cls.data_ptr(), B, Nq, nc1 - 1, k, sc.data_ptr(), fl.data_ptr(), _stream()),
               "rsp_query_topk")
    return sc, fl


def query_mask_post(low_res, qidx, cls_score, batch_input_shape, crop_hw, out_hw, want_logits=False):
    """low_res [Nq, h, w] logits of one image; qidx int32 [k]; returns (masks bool [k,oh,ow], det_scores, bboxes)."""
    lib = _lib.load()
    _, h, w = _mask_logits(low_res, "query_mask_post")
    dev = low_res.device
    if qidx.dtype != torch.int32 or qidx.dim() != 1 or not qidx.is_contiguous() or qidx.device != dev:
        raise ValueError("qidx: contiguous int32 [k] on the device of low_res")
    k = qidx.numel()
    masks = torch.empty((k, out_hw[0], out_hw[1]), dtype=torch.bool, device=dev)
    logits = torch.empty((k, out_hw[0], out_hw[1]), dtype=torch.float32, device=dev) if want_logits else None
    det = torch.empty((k,), dtype=torch.float32, device=dev)
    boxes = torch.empty((k, 4), dtype=torch.float32, device=dev)
    ws = torch.empty((max(k, 1) * 32,), dtype=torch.uint8, device=dev)
    _timed('query_mask_kernel', 0, 1.0 * masks.numel(),
           lambda: _lib.check(lib.rsp_query_mask_post(low_res.data_ptr(), qidx.data_ptr(), cls_score.data_ptr(), k, h, w,
                                                      *_mask_geometry(batch_input_shape, crop_hw, out_hw), ws.data_ptr(),
                                                      masks.data_ptr(), _ptr(logits), det.data_ptr(), boxes.data_ptr(),
                                                      _stream()), "rsp_query_mask_post"))
    return (masks, det, boxes, logits) if want_logits else (masks, det, boxes)


PANOPTIC_MAX_QUERIES = _lib.CONST['RSP_PANOPTIC_MAX_QUERIES']


def panoptic_fuse(cls, low_res, batch_input_shape, crop_hw, out_hw, num_things_classes, num_classes, object_mask_thr=0.8,
                  iou_thr=0.8, filter_low_score=False):
    """MaskFormerFusionHead.panoptic_postprocess (maskformer_fusion_head.py:41-106) of one image on the mask field of
    query_mask_post: cls [Nq, nc + 1] class logits, low_res [Nq, h, w] logits -> (sem_seg int32 [oh, ow], info) with info =
    dict(segment, mask_area, original_area: int32 [Nq]; score: fp32 [Nq]) -- the id every query painted (-1: none) and its two
    areas (0 for a query that was not kept).  Nothing is read back: four launches on the current stream."""
    lib = _lib.load()
    Nq, h, w = _mask_logits(low_res, "panoptic_fuse")
    _chk_f32(cls, "cls")
    dev = low_res.device
    if cls.dim() != 2 or not cls.is_contiguous() or cls.device != dev or cls.shape[0] != Nq or cls.shape[1] != num_classes + 1:
        raise ValueError("panoptic_fuse expects contiguous fp32 cls [Nq, num_classes + 1] on the device of low_res")
    oh, ow = int(out_hw[0]), int(out_hw[1])
    sem = torch.empty((max(oh, 0), max(ow, 0)), dtype=torch.int32, device=dev)
    info = {k: torch.empty((Nq,), dtype=torch.int32, device=dev) for k in ('segment', 'mask_area', 'original_area')}
    info['score'] = torch.empty((Nq,), dtype=torch.float32, device=dev)
    ws = torch.empty((lib.rsp_panoptic_workspace_bytes(),), dtype=torch.uint8, device=dev)
    _timed('panoptic_fuse_kernel', 0, 4.0 * low_res.numel() + 4.0 * sem.numel(),
           lambda: _lib.check(lib.rsp_panoptic_fuse(cls.data_ptr(), low_res.data_ptr(), Nq, int(num_classes),
                                                    int(num_things_classes), h, w,
                                                    *_mask_geometry(batch_input_shape, crop_hw, out_hw),
                                                    float(object_mask_thr), float(iou_thr), int(bool(filter_low_score)),
                                                    ws.data_ptr(), sem.data_ptr(), info['segment'].data_ptr(),
                                                    info['mask_area'].data_ptr(), info['original_area'].data_ptr(),
                                                    info['score'].data_ptr(), _stream()), "rsp_panoptic_fuse"))
    return sem, info


PQ_MAX_SEGMENTS = _lib.CONST['RSP_PQ_MAX_SEGMENTS']
PQ_MAX_PRED_ID = _lib.CONST['RSP_PQ_MAX_PRED_ID']
PQ_MAX_CATEGORIES = _lib.CONST['RSP_PQ_MAX_CATEGORIES']
PQ_STATUS = {v: k[len('RSP_PQ_STATUS_'):].lower() for k, v in _lib.CONST.items() if k.startswith('RSP_PQ_STATUS_')}
_PQ_LABELS = 1000                       # INSTANCE_OFFSET (panoptic_utils.py:18)


def pq_status_text(status):
    """the names of the RSP_PQ_STATUS_* bits of a row's status"""
    return ', '.join(name for bit, name in sorted(PQ_STATUS.items()) if status & bit) or 'ok'


def pq_image(pred, gt, gt_segments, categories, num_classes, ignore_index=None, label2cat=None):
    """pq_compute_single_core (panoptic_utils.py:60-169) of one image on the maps CocoPanopticMetric hands it
    (coco_panoptic_metric.py:270-297), csrc/panoptic_quality.hip.  pred int32 [H, W] on the device: id = label + 1000 *
    instance, void where id % 1000 is num_classes or ignore_index (default num_classes).  gt uint8 [H, W, 3] (a panoptic PNG:
    id = R + 256 G + 65536 B) or an int32 / int64 id map [H, W], on the device of pred (an int64 map is narrowed to int32 on
    the device without a look at its values: it must hold ids below 2^31, or a larger one wraps onto a small one).  gt_segments: the image's
    segments_info in JSON order, dicts with id, category_id, iscrowd and area (None or absent: the pixels are counted, as the
    dataset path does).  categories: the category ids, in the order of the result's columns (a dict: its keys).  label2cat:
    label -> category id (None: the label is the category id).

    Returns a row of device tensors: tp, fp, fn int32 [n_cat], iou float64 [n_cat], status int32 [1] (0, or RSP_PQ_STATUS_*
    bits -- what only the map can tell: too many segments, an id out of range, a predicted id 0 that is not void, a predicted
    label without a category, a listed non-crowd gt area below the segment's pixels in the map; the row is then zero), n_pred int32 [1] and pred_ids, pred_cat (an index into categories),
    pred_area int32 [PQ_MAX_SEGMENTS].  Nothing is read back.  What the arguments alone tell raises ValueError before a launch."""
    if not isinstance(pred, torch.Tensor) or pred.dtype != torch.int32 or pred.dim() != 2 or not pred.is_contiguous() \
            or pred.numel() == 0:
        raise ValueError("pq_image expects pred as a contiguous int32 map [H, W]")
    if not _is_device(pred):
        raise ValueError(f"pq_image expects the maps on the HIP device, got pred on {pred.device}")
    lib = _lib.load()
    H, W = int(pred.shape[0]), int(pred.shape[1])
    dev = pred.device
    if not isinstance(gt, torch.Tensor) or gt.device != dev:
        raise ValueError("pq_image expects gt on the device of pred")
    rgb = gt.dtype == torch.uint8
    if rgb:
        if gt.dim() != 3 or gt.shape[2] != 3:
            raise ValueError("pq_image expects a uint8 gt as [H, W, 3]")
    elif gt.dtype not in (torch.int32, torch.int64) or gt.dim() != 2:
        raise ValueError("pq_image expects gt as uint8 [H, W, 3] or an int32 / int64 map [H, W]")
    if tuple(gt.shape[:2]) != (H, W):
        raise ValueError(f"pq_image: the maps differ in size: pred {(H, W)}, gt {tuple(gt.shape[:2])}")
    if H * W >= 2 ** 31:
        raise ValueError("pq_image: H * W >= 2^31")
    gt = gt.contiguous() if rgb else gt.to(torch.int32).contiguous()
    if pred.data_ptr() % 16 or gt.data_ptr() % 16:
        raise ValueError("pq_image: the maps must start at 16-byte aligned addresses")
    cat_ids = list(categories.keys() if isinstance(categories, dict) else categories)
    n_cat, G = len(cat_ids), len(gt_segments)
    if not 1 <= n_cat <= PQ_MAX_CATEGORIES or len(set(cat_ids)) != n_cat:
        raise ValueError(f"pq_image: categories must be 1 .. {PQ_MAX_CATEGORIES} distinct ids")
    if G > PQ_MAX_SEGMENTS:
        raise ValueError(f"pq_image: {G} ground-truth segments, at most {PQ_MAX_SEGMENTS}")
    num_classes = int(num_classes)
    ignore_index = num_classes if ignore_index is None else int(ignore_index)
    if num_classes < 0:
        raise ValueError("pq_image: num_classes < 0")
    index = {c: i for i, c in enumerate(cat_ids)}
    ids = [int(s['id']) for s in gt_segments]
    if len(set(ids)) != G:
        raise ValueError("pq_image: duplicate ground-truth segment ids")
    if any(not 0 < i < 2 ** 31 for i in ids):
        raise ValueError("pq_image: ground-truth segment ids must be in [1, 2^31) (0 is VOID)")
    order = sorted(range(G), key=lambda k: ids[k])
    slot = {ids[k]: j for j, k in enumerate(order)}
    area = []
    for k in order:
        a = gt_segments[k].get('area')
        if a is not None and not 0 <= int(a) < 2 ** 31:
            raise ValueError("pq_image: a ground-truth area outside [0, 2^31)")
        area.append(-1 if a is None else int(a))
    # a gt category outside `categories` takes part in nothing (the reference counts it where pq_average never looks)
    gcat = [index.get(gt_segments[k]['category_id'], -1) for k in order]
    crowd = [1 if int(gt_segments[k].get('iscrowd', 0)) == 1 else 0 for k in order]
    crowd_of = [-1] * n_cat
    for s in gt_segments:                                  # JSON order: the last crowd segment of a category stays
        if int(s.get('iscrowd', 0)) == 1 and s['category_id'] in index:
            crowd_of[index[s['category_id']]] = slot[int(s['id'])]
    if label2cat is None:
        label_cat = [index.get(l, -1) for l in range(_PQ_LABELS)]
    else:
        label_cat = [-1] * _PQ_LABELS
        for l, c in label2cat.items():
            if not 0 <= int(l) < _PQ_LABELS:
                raise ValueError(f"pq_image: label {l} outside [0, {_PQ_LABELS})")
            if c not in index:
                raise ValueError(f"pq_image: label {l} maps to category {c}, which is not in categories")
            label_cat[int(l)] = index[c]
    tables = torch.tensor([ids[k] for k in order] + gcat + crowd + area + label_cat + crowd_of, dtype=torch.int32).to(dev)
    # two buffers: a caller that keeps the statistics of many images (CocoPanopticMetric) drops the segment list
    ints = torch.empty((3 * n_cat + 2,), dtype=torch.int32, device=dev)
    segs = torch.empty((3, PQ_MAX_SEGMENTS), dtype=torch.int32, device=dev)
    row = dict(tp=ints[:n_cat], fp=ints[n_cat:2 * n_cat], fn=ints[2 * n_cat:3 * n_cat], status=ints[3 * n_cat:3 * n_cat + 1],
               n_pred=ints[3 * n_cat + 1:], iou=torch.empty((n_cat,), dtype=torch.float64, device=dev),
               pred_ids=segs[0], pred_cat=segs[1], pred_area=segs[2])
    ws = torch.empty((lib.rsp_pq_workspace_bytes(G),), dtype=torch.uint8, device=dev)
    _timed('pq_image_kernel', 0, (8.0 + (6.0 if rgb else 8.0)) * H * W,
           lambda: _lib.check(lib.rsp_pq_image(pred.data_ptr(), gt.data_ptr() if rgb else 0, 0 if rgb else gt.data_ptr(), H, W,
                                               num_classes, ignore_index, tables.data_ptr(), G, n_cat, ws.data_ptr(),
                                               row['tp'].data_ptr(), row['fp'].data_ptr(), row['fn'].data_ptr(),
                                               row['iou'].data_ptr(), row['status'].data_ptr(), row['n_pred'].data_ptr(),
                                               row['pred_ids'].data_ptr(), row['pred_cat'].data_ptr(),
                                               row['pred_area'].data_ptr(), _stream()), "rsp_pq_image"))
    return row


def pq_reduce(rows):
    """PQStat.__iadd__ over the rows of pq_image in order (coco_panoptic_metric.py:529-531), on the device: dict(tp, fp, fn
    int64 [n_cat], iou float64 [n_cat] = ((0 + s1) + s2) + ..., status int32-valued int64 [n_img]) as views of ONE device
    buffer `packed` int64 [4 n_cat + n_img], so a caller reads the host once."""
    rows = list(rows)
    if not rows:
        raise ValueError("pq_reduce: no rows")
    if not isinstance(rows[0]['tp'], torch.Tensor) or not _is_device(rows[0]['tp']):
        raise ValueError("pq_reduce expects rows of ops.pq_image on the HIP device")
    lib = _lib.load()
    n_cat = rows[0]['tp'].numel()
    if any(r['tp'].numel() != n_cat or r['tp'].device != rows[0]['tp'].device for r in rows):
        raise ValueError("pq_reduce: rows of different categories or devices")
    n_img = len(rows)
    tp, fp, fn, iou, st = (torch.stack([r[k].reshape(-1) for r in rows]).contiguous() for k in ('tp', 'fp', 'fn', 'iou', 'status'))
    out = torch.empty((4 * n_cat + n_img,), dtype=torch.int64, device=tp.device)
    _lib.check(lib.rsp_pq_reduce(tp.data_ptr(), fp.data_ptr(), fn.data_ptr(), iou.data_ptr(), st.data_ptr(), n_img, n_cat,
                                 out.data_ptr(), _stream()), "rsp_pq_reduce")
    return dict(packed=out, tp=out[:n_cat], fp=out[n_cat:2 * n_cat], fn=out[2 * n_cat:3 * n_cat],
                iou=out[3 * n_cat:4 * n_cat].view(torch.float64), status=out[4 * n_cat:])
