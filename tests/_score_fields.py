"""Prescribed score fields for every attention kernel: the online softmax at its corners instead of on Gaussian scores.

The Gaussian inputs of tests/test_gpu_kernels.py pin the indexing of the attention kernels; they never reach the lazy running
maximum of csrc/attn_win.hip (LAZY_LOG2 = 8), the rescale-skip ballots, the saturating fp16 splits or a padded-key mask.
Here the LOGITS are prescribed.  Within a head

    q[i, 0] = A s_i,   k[j, 0] = f_j / (A scale),   every other coordinate of q and k = randn * 0.05,   v = randn,

so that query i sees the field s_i f_j plus small noise (A = 4; s_i a per-query sign).  The reference is the fp64 restatement
the existing tests use, evaluated on the very same tensors, so the field need not be exact.  Every (batch, head) pair of a
launch carries its own field (`slots`), so one launch checks several fields and the error is taken per field.

The bound is measured, not chosen: E32 = max abs error of the SAME restatement in plain torch float32 on the CPU against
fp64, and a case passes when  err <= max(F, 2 E32)  with F the floor the entry point is held to on Gaussian inputs (2e-5 ViT /
generic / fused, 2e-6 and 4e-6 for the fp32 and plane outputs of sam_t2i / sam_i2t).  A 100-nat ramp costs 1e-5 .. 4e-5 in any
fp32-class evaluation, so the floor alone cannot serve; the factor 2 is what the kernels needed on the wave emulator
(fp16x3 kernels 0.2 - 0.9 E32, the fp32 decoder kernels up to 1.34 E32: same arithmetic class, another summation order).

Both kernel tiers run these bodies: tests/test_gpu_kernel_props.py on the device, tests/test_wave_emu_cpu.py a subset on the
emulator.  A body runs ALL its cases, prints `case err E32 bound` for each and asserts at the end (Report.finish)."""
import math

import torch
import torch.nn.functional as F

A = 4.0                     # q[:, 0] = A s_i
LN2 = math.log(2.0)
LEVELS = (-1000.0, -300.0, -240.0, -70.0, 300.0)
F_VIT = 2e-5                # ViT, generic and fused kernels
F_SAM32, F_SAMPL = 2e-6, 4e-6


class Report:
    def __init__(self, family):
        self.family, self.rows, self.bad = family, [], []

    def add(self, case, err, e32, floor):
        bound = max(floor, 2.0 * e32)
        ok = err <= bound                                   # NaN fails
        print(f'score-field {self.family} {case}: err {err:.3e} E32 {e32:.3e} bound {bound:.3e}{"" if ok else "  <-- FAIL"}')
        self.rows.append((case, err, e32, bound))
        if not ok:
            self.bad.append((case, err, e32, bound))

    def finish(self):
        assert not self.bad, (self.family, self.bad)


# ------------------------------------------------------------------------------------------------------------------ fields
def signs(form, n):
    """s_i: 'same' +1; 'parity' +1 for even queries, -1 for odd ones; 'half' +1 for i mod 64 < 32, -1 otherwise (the two half
    waves' partner lanes split differently).  A field that is the same for every query never splits a wave's ballot."""
    i = torch.arange(n)
    if form == 'same':
        return torch.ones(n, dtype=torch.float64)
    if form == 'parity':
        return (1 - 2 * (i % 2)).double()
    if form == 'half':
        return torch.where(i % 64 < 32, 1.0, -1.0).double()
    raise ValueError(form)


def field(kind, T, tile, arg=None):
    """f [T] in nats (fp64).  tile: the kernel's key tile."""
    j = torch.arange(T)
    t = (j // tile).double()
    last0 = (T - 1) // tile * tile                          # first key of the last tile
    if kind == 'uniform':
        return torch.zeros(T, dtype=torch.float64)
    if kind == 'stair_up':                                  # a rescale at every tile
        return 6.0 * t
    if kind == 'stair_down':                                # ... then none
        return -6.0 * t
    if kind == 'stair_lazy':                                # 7.2 log2 units per tile: below LAZY_LOG2 each, above cumulatively
        return 5.0 * t
    if kind == 'straddle':                                  # arg = (tile, +-1): just over / under LAZY_LOG2 in that tile
        tt, sg = arg
        return torch.where(j // tile == tt, (8.0 + 0.01 * sg) * LN2, 0.0).double()
    if kind == 'ramp':
        return torch.linspace(0.0, 100.0, T, dtype=torch.float64)
    if kind == 'spike':
        f = torch.zeros(T, dtype=torch.float64)
        f[arg] = 40.0
        return f
    if kind == 'level':
        return torch.full((T,), float(arg), dtype=torch.float64)
    if kind == 'cold_hot':                                  # cold but the last tile's real keys hot
        f = torch.full((T,), -400.0, dtype=torch.float64)
        f[last0:] = -100.0
        return f
    raise ValueError(kind)


def spike_keys(T, tile):
    """first and last key of every tile (= the keys either side of every tile boundary) and the last real key"""
    ks = set()
    for t0 in range(0, T, tile):
        ks.add(t0)
        ks.add(min(t0 + tile, T) - 1)
    ks.add(T - 1)
    return sorted(ks)


def cases_for(T, tile, straddle_tiles=(1,), levels=LEVELS, spikes=None, divergent=True):
    """[(name, f, sign form, spike key or None)]: the field list of one key count / tile"""
    out = [('uniform', field('uniform', T, tile), 'same', None)]
    stairs = ('stair_up', 'stair_down', 'stair_lazy')
    for k in stairs:
        out.append((k, field(k, T, tile), 'same', None))
    ntile = (T + tile - 1) // tile
    strad = [(t, sg) for t in straddle_tiles if t < ntile for sg in (+1, -1)]
    for (t, sg) in strad:
        out.append((f'straddle({t},{"+" if sg > 0 else "-"})', field('straddle', T, tile, (t, sg)), 'same', None))
    out.append(('ramp', field('ramp', T, tile), 'same', None))
    for j in (spike_keys(T, tile) if spikes is None else spikes):
        out.append((f'spike({j})', field('spike', T, tile, j), 'same', j))
    for c in levels:
        out.append((f'level({c:g})', field('level', T, tile, c), 'same', None))
    out.append(('cold_but_last_tile_hot', field('cold_hot', T, tile), 'same', None))
    if divergent:
        for form in ('parity', 'half'):
            for k in stairs:
                out.append((f'{k}/{form}', field(k, T, tile), form, None))
            for (t, sg) in strad:
                out.append((f'straddle({t},{"+" if sg > 0 else "-"})/{form}', field('straddle', T, tile, (t, sg)), form, None))
    return out


PAD = ('pad', None, 'same', None)


def chunks(cases, n):
    """the case list in launches of n slots, the last one padded with uniform fields that are not reported"""
    for i in range(0, len(cases), n):
        c = list(cases[i:i + n])
        yield c + [PAD] * (n - len(c))


def fill_qkv(cases, B, Tq, Tk, nh, dh, scale, g):
    """q [B, Tq, nh, dh], k, v [B, Tk, nh, dh] fp32: slot n = (batch n // nh, head n % nh) carries cases[n]"""
    q = torch.randn(B, Tq, nh, dh, generator=g) * 0.05
    k = torch.randn(B, Tk, nh, dh, generator=g) * 0.05
    v = torch.randn(B, Tk, nh, dh, generator=g)
    assert len(cases) == B * nh
    for n, (_, f, form, _) in enumerate(cases):
        b, h = divmod(n, nh)
        q[b, :, h, 0] = (A * signs(form, Tq)).float()
        k[b, :, h, 0] = 0.0 if f is None else (f / (A * scale)).float()
    return q, k, v


def attention_ref(q, k, v, scale, dtype, bias=None):
    """softmax((q scale) k^T + bias) v of the existing tests, q [B, Tq, nh, dh], k / v [B, Tk, nh, dh] -> [B, Tq, nh, dh];
    bias [B, Tk] per key"""
    qh, kh, vh = (t.to(dtype).transpose(1, 2) for t in (q, k, v))
    s = (qh * scale) @ kh.transpose(-1, -2)
    if bias is not None:
        s = s + bias.to(dtype)[:, None, None, :]
    return (s.softmax(-1) @ vh).transpose(1, 2)


def vit_ref(qkv, rph, rpw, S, nh, dh, scale, dtype):
    """test_gpu_kernels._ref_vit_attention (HF:803-831 + 761-801) in `dtype` -> [Bp, T, nh * dh]"""
    Bp, T = qkv.shape[:2]
    q, k, v = qkv.to(dtype).permute(2, 0, 3, 1, 4).reshape(3, Bp * nh, T, dh).unbind(0)
    attn = (q * scale) @ k.transpose(-2, -1)
    idx = torch.arange(S)[:, None] - torch.arange(S)[None, :] + (S - 1)
    Rh, Rw = rph.to(dtype)[idx], rpw.to(dtype)[idx]
    rq = q.reshape(Bp * nh, S, S, dh)
    rel_h = torch.einsum('bhwc,hkc->bhwk', rq, Rh)
    rel_w = torch.einsum('bhwc,wkc->bhwk', rq, Rw)
    attn = (attn.view(Bp * nh, S, S, S, S) + rel_h[:, :, :, :, None] + rel_w[:, :, :, None, :]).view(Bp * nh, T, T)
    return (attn.softmax(-1) @ v).view(Bp, nh, S, S, dh).permute(0, 2, 3, 1, 4).reshape(Bp, T, nh * dh)


def _slot_errors(rep, cases, got, ref, r32, v, floor, tag, rows=None):
    """got / ref / r32 [B, Tq, nh, dh] (fp64 on the CPU), v [B, Tk, nh, dh]; rows [B, Tq] bool: the queries that are compared.
    A spike case also meets its known answer out[q] = v[j] (queries with s_i = +1: all of them, spikes use 'same')."""
    nh = got.shape[2]
    for n, (name, f, form, spike) in enumerate(cases):
        if f is None and name == 'pad':
            continue
        b, h = divmod(n, nh)
        sel = slice(None) if rows is None else rows[b]
        e32 = float((r32[b, sel, h] - ref[b, sel, h]).abs().max())
        rep.add(f'{tag} {name}', float((got[b, sel, h] - ref[b, sel, h]).abs().max()), e32, floor)
        if spike is not None:
            rep.add(f'{tag} {name} known-answer', float((got[b, sel, h] - v[b, spike, h].double()).abs().max()), e32, floor)


# ------------------------------------------------------------------------------------------------------------ ViT kernels
def window_rows(Bp, grid):
    """[Bp, 196] bool: the real queries of a window grid (nw, real); None: all"""
    S = 14
    if grid is None:
        return None
    nw, real = grid
    wi = torch.arange(Bp) % (nw * nw)
    rh = torch.where(wi // nw == nw - 1, real, S)
    cw = torch.where(wi % nw == nw - 1, real, S)
    yy, xx = torch.arange(S)[None, :, None], torch.arange(S)[None, None, :]
    return ((yy < rh[:, None, None]) & (xx < cw[:, None, None])).reshape(Bp, S * S)


def _vit_launch(ops, dev, entry, qkv, rph, rpw, Bp, S, nh, dh, scale, kv_e, grid, variant, planes):
    """one launch of a ViT attention entry point -> [Bp, T, nh, dh] fp64 on the CPU (unwritten rows 7.0)"""
    import test_gpu_kernels as tk
    T, D = S * S, nh * dh
    if entry == 'f32':                                       # rsp_vit_attention: fp32 qkv, -inf masks (attn.hip / attn_global.hip)
        d = qkv.to(dev).contiguous()
        rel = ops.vit_relpos(d, rph.to(dev), rpw.to(dev), Bp, S, nh, dh)
        got = ops.vit_attention(d, rel, Bp, S, nh, dh, scale, planes=planes)
    else:
        q = qkv[:, :, 0].reshape(Bp * T, D).contiguous().to(dev)
        kv = ops.to_planes(qkv[:, :, 1:].reshape(Bp * T, 2 * D).contiguous().to(dev), kv_e)
        if entry == 'window':                                # rsp_vit_window_attention: packed tables
            tab = ops.pack_relpos_tables(rph.to(dev), rpw.to(dev), S, dh)
            got = ops.vit_window_attention(q, kv, tab, Bp, nh, dh, scale, planes=planes, win_grid=grid, variant=variant)
        else:                                                # rsp_vit_attention_planes: rel tensor (S = 14: attn_win_kernel too)
            rel = ops.vit_relpos(q, rph.to(dev), rpw.to(dev), Bp, S, nh, dh, q_ld=D)
            got = ops.vit_attention_planes(q, kv, rel, Bp, S, nh, dh, scale, planes=planes, win_grid=grid)
    got = tk._planes_to_f32(got) if planes else got.cpu().double()
    return torch.nan_to_num(got, nan=7.0).view(Bp, T, nh, dh)


def check_vit_fields(ops, dev, rep, entry, S, Bp, nh, dh, cases, kv_e=2, grid=None, variant=0, planes=(False,), seed=0):
    """`cases` (Bp * nh of them) through one ViT attention entry point; planes: the output forms to run"""
    import test_gpu_kernels as tk
    g = torch.Generator().manual_seed(1000 + seed)
    T, scale = S * S, dh ** -0.5
    q, k, v = fill_qkv(cases, Bp, T, T, nh, dh, scale, g)
    qkv = torch.stack([q, k, v], 2).contiguous()
    rph = torch.randn(2 * S - 1, dh, generator=g) * 0.02
    rpw = torch.randn(2 * S - 1, dh, generator=g) * 0.02
    ref = tk._ref_vit_attention(qkv, rph, rpw, S, nh, dh, scale)[0].view(Bp, T, nh, dh)
    r32 = vit_ref(qkv, rph, rpw, S, nh, dh, scale, torch.float32).double().view(Bp, T, nh, dh)
    rows = window_rows(Bp, grid)
    for pl in planes:
        got = _vit_launch(ops, dev, entry, qkv, rph, rpw, Bp, S, nh, dh, scale, kv_e, grid, variant, pl)
        tag = f'{entry} S={S} dh={dh} kv_e={kv_e} grid={grid} v{variant} {"planes" if pl else "fp32"}'
        _slot_errors(rep, cases, got, ref, r32, v, F_VIT, tag, rows)


def check_window_relpos_bias(ops, dev, rep, entry, dh, target, grid=None, variant=0, seed=0):
    """the bias path of attn_win_kernel alone (one-hot MFMA, fp16 split of the 28 terms): zero k, Gaussian q, tables scaled
    so that the largest rel-pos term is `target` logits (kv_e = 2: the split saturates beyond 256)"""
    import test_gpu_kernels as tk
    S, nh = 14, 2
    Bp = grid[0] ** 2 if grid else 2
    g = torch.Generator().manual_seed(2000 + seed)
    T, scale = S * S, dh ** -0.5
    qkv = torch.randn(Bp, T, 3, nh, dh, generator=g)
    qkv[:, :, 1] = 0.0
    rph, rpw = torch.randn(2 * S - 1, dh, generator=g), torch.randn(2 * S - 1, dh, generator=g)
    rel = tk._ref_vit_attention(qkv, rph, rpw, S, nh, dh, scale)[1]
    rph, rpw = rph * (target / float(rel.abs().max())), rpw * (target / float(rel.abs().max()))
    ref = tk._ref_vit_attention(qkv, rph, rpw, S, nh, dh, scale)[0].view(Bp, T, nh, dh)
    r32 = vit_ref(qkv, rph, rpw, S, nh, dh, scale, torch.float32).double().view(Bp, T, nh, dh)
    rows = window_rows(Bp, grid)
    got = _vit_launch(ops, dev, entry, qkv, rph, rpw, Bp, S, nh, dh, scale, 2, grid, variant, False)
    sel = torch.ones(Bp, T, dtype=torch.bool) if rows is None else rows
    rep.add(f'{entry} dh={dh} grid={grid} v{variant} relpos(max {target:g})', float((got[sel] - ref[sel]).abs().max()),
            float((r32[sel] - ref[sel]).abs().max()), F_VIT)


def window_cases():
    """every field of the window kernel (196 keys, tile 32, last real key 195): straddles in every tile 1..6"""
    return cases_for(196, 32, straddle_tiles=(1, 2, 3, 4, 5, 6), levels=())


def window_level_cases():
    return [(f'level({c:g})', field('level', 196, 32, c), 'same', None) for c in LEVELS] + \
           [('cold_but_last_tile_hot', field('cold_hot', 196, 32), 'same', None)]


def run_window_family(ops, dev, rep, entry, configs, planes=(False,)):
    """configs: [(grid, dh, variant)], nh = 2, B = 1.  All fields at kv_e = 2, the levels at kv_e 0 / 2 / 4, the rel-pos cases."""
    for (grid, dh, variant) in configs:
        Bp = grid[0] ** 2 if grid else 4
        for n, c in enumerate(chunks(window_cases(), Bp * 2)):
            check_vit_fields(ops, dev, rep, entry, 14, Bp, 2, dh, c, 2, grid, variant, planes, seed=n)
        for kv_e in (0, 2, 4):
            for n, c in enumerate(chunks(window_level_cases(), Bp * 2)):
                check_vit_fields(ops, dev, rep, entry, 14, Bp, 2, dh, c, kv_e, grid, variant, planes, seed=50 + n)
        for target in (40.0, 120.0, 250.0):
            check_window_relpos_bias(ops, dev, rep, entry, dh, target, grid, variant)


def global_cases(T, full=True):
    """S = 32 / 64 (tile 64): the staircases, one straddle pair, the ramp, spikes at every tile edge (full) or the first / last
    tiles, the levels, the divergent forms"""
    nt = T // 64
    sp = None if full else [0, 63, 64, T - 65, T - 64, T - 1]
    return cases_for(T, 64, straddle_tiles=(1, nt - 1), spikes=sp)


S64_CASES = ['uniform', 'stair_up/parity', 'stair_lazy/half', 'straddle(1,+)', 'ramp', f'spike({64 * 64 - 1})', 'level(-1000)',
             'cold_but_last_tile_hot']                     # one per field class
EMU_S32_CASES = ['stair_up/parity', 'stair_lazy/half', 'straddle(1,+)', 'level(-1000)']


def pick(cases, names):
    by = {c[0]: c for c in cases}
    return [by[n] for n in names]


# --------------------------------------------------------------------------------------------------------- generic attention
def check_generic_fields(ops, dev, rep, dh, Tq, Tk, nh, B=None):
    """rsp_attention (attn.hip, tile 64, ragged last tile) with every field of its key count over B * nh slots"""
    cases = cases_for(Tk, 64, straddle_tiles=(1,))
    B = B or (len(cases) + nh - 1) // nh
    scale, D = dh ** -0.5, nh * dh
    for n, c in enumerate(chunks(cases, B * nh)):
        g = torch.Generator().manual_seed(3000 + n)
        q, k, v = fill_qkv(c, B, Tq, Tk, nh, dh, scale, g)
        ref = attention_ref(q, k, v, scale, torch.float64)
        r32 = attention_ref(q, k, v, scale, torch.float32).double()
        out = torch.empty(B, Tq, D, device=dev)
        ops.attention(q.to(dev), k.to(dev), v.to(dev), out, B=B, nh=nh, dh=dh, Tq=Tq, Tk=Tk, scale=scale,
                      q_strides=(Tq * D, D, dh), k_strides=(Tk * D, D, dh), v_strides=(Tk * D, D, dh), o_strides=(Tq * D, D, dh))
        _slot_errors(rep, c, out.cpu().double().view(B, Tq, nh, dh), ref, r32, v, F_VIT, f'attention dh={dh} Tq={Tq} Tk={Tk} nh={nh}')


# ------------------------------------------------------------------------------------------------------- SAM decoder kernels
def check_t2i_fields(ops, dev, rep, T=7, N=600, where='k'):
    """rsp_sam_t2i_attention (where = 'k') / rsp_sam_t2i_attention_bias (where = 'k+bias': the field in k and a small bias;
    'bias': the field in the per-key bias, one field per RoI, k small noise): T token queries over N keys, 8 heads x 16"""
    cases = cases_for(N, 64, straddle_tiles=(1,), divergent=(where != 'bias'))
    nh, dh, scale = 8, 16, 0.25
    per = 1 if where == 'bias' else nh                        # the bias is shared by the heads: one field per RoI
    R = (len(cases) + per - 1) // per
    g = torch.Generator().manual_seed(4000 + len(where))
    cs = next(chunks(cases, R * per))
    if where == 'bias':
        q, k, v = fill_qkv([PAD] * (R * nh), R, T, N, nh, dh, scale, g)
        bias = torch.stack([torch.zeros(N, dtype=torch.float64) if f is None else f for (_, f, _, _) in cs]).float()
        slot_cases = [c for c in cs for _ in range(nh)]       # every head of the RoI reports (the same field)
        slot_cases = [(f'{c[0]} h{n % nh}',) + c[1:] if c[0] != 'pad' else c for n, c in enumerate(slot_cases)]
    else:
        q, k, v = fill_qkv(cs, R, T, N, nh, dh, scale, g)
        bias = torch.randn(R, N, generator=g) * 0.02 if where == 'k+bias' else None
        slot_cases = cs
    ref = attention_ref(q, k, v, scale, torch.float64, bias)
    r32 = attention_ref(q, k, v, scale, torch.float32, bias).double()
    kv = torch.cat([k.reshape(R, N, 128), v.reshape(R, N, 128)], -1).reshape(R * N, 256).contiguous()
    out = torch.empty(R * T, 128, device=dev)
    if bias is None:
        ops.sam_t2i_attention(q.reshape(R * T, 128).to(dev), kv.to(dev), out, R=R, T=T, N=N, scale=scale)
    else:
        ops.sam_t2i_attention_bias(q.reshape(R * T, 128).to(dev), kv.to(dev), bias.contiguous().to(dev), out, R=R, T=T, N=N,
                                   scale=scale)
    _slot_errors(rep, slot_cases, out.cpu().double().view(R, T, nh, dh), ref, r32, v, F_SAM32, f'sam_t2i[{where}] T={T} N={N}')


def i2t_cases(T):
    """image -> token: T keys, tile 2 -- every key is a tile edge"""
    return cases_for(T, 2, straddle_tiles=(1,), levels=(-1000.0, -300.0, 300.0))


def check_i2t_fields(ops, dev, rep, T, N=96):
    """rsp_sam_i2t_attention: N image queries over T token keys, fp32 and plane outputs"""
    import test_gpu_kernels as tk
    cases = i2t_cases(T)
    nh, dh, scale = 8, 16, 0.25
    R = (len(cases) + nh - 1) // nh
    cs = next(chunks(cases, R * nh))
    g = torch.Generator().manual_seed(5000 + T)
    q, k, v = fill_qkv(cs, R, N, T, nh, dh, scale, g)
    ref = attention_ref(q, k, v, scale, torch.float64)
    r32 = attention_ref(q, k, v, scale, torch.float32).double()
    o32 = torch.empty(R * N, 128, device=dev)
    pl = ops.empty_planes((R * N, 128), dev)
    ops.sam_i2t_attention(q.reshape(R * N, 128).to(dev), k.reshape(R * T, 128).to(dev), v.reshape(R * T, 128).to(dev),
                          R=R, T=T, N=N, scale=scale, out=o32, out_planes=pl)
    _slot_errors(rep, cs, o32.cpu().double().view(R, N, nh, dh), ref, r32, v, F_SAM32, f'sam_i2t T={T} N={N} fp32')
    _slot_errors(rep, cs, tk._planes_to_f32(pl).view(R, N, nh, dh), ref, r32, v, F_SAMPL, f'sam_i2t T={T} N={N} planes')


def check_i2t_fused_fields(ops, dev, rep, T, form, N=96):
    """rsp_sam_i2t_fused = LayerNorm(residual + out_proj(image -> token attention)), VALU or matrix-core form: one field per
    RoI (out_proj mixes the heads), all eight heads carry it; compared after the LayerNorm, as the existing test does"""
    import test_gpu_kernels as tk
    cases = i2t_cases(T)
    nh, dh, scale = 8, 16, 0.25
    R = len(cases)
    g = torch.Generator().manual_seed(6000 + T)
    q, k, v = fill_qkv([c for c in cases for _ in range(nh)], R, N, T, nh, dh, scale, g)
    wo, bo = torch.randn(256, 128, generator=g) / 128 ** 0.5, torch.randn(256, generator=g)
    gamma, beta = torch.randn(256, generator=g), torch.randn(256, generator=g)
    res = torch.randn(R * N, 256, generator=g) * 3

    def comp(dtype):
        att = attention_ref(q, k, v, scale, dtype).reshape(R, N, 128)
        y = att @ wo.to(dtype).t() + bo.to(dtype) + res.to(dtype).view(R, N, 256)
        return F.layer_norm(y, (256,), gamma.to(dtype), beta.to(dtype), 1e-6).double()
    ref, r32 = comp(torch.float64), comp(torch.float32)
    args = [t.to(dev) for t in (q.reshape(R * N, 128), k.reshape(R * T, 128), v.reshape(R * T, 128), wo, bo, gamma, beta)]
    got = ops.sam_i2t_fused(*args, res=res.to(dev), R=R, T=T, N=N, scale=scale, eps=1e-6, planes=True, f32=(form == 'valu'))
    out, pl = got if form == 'valu' else (None, got)
    outs = [('planes', tk._planes_to_f32(pl).view(R, N, 256))] + ([('fp32', out.cpu().double().view(R, N, 256))] if out is not None else [])
    for what, o in outs:
        for r, (name, _, _, _) in enumerate(cases):
            rep.add(f'sam_i2t_fused[{form}] T={T} N={N} {what} {name}', float((o[r] - ref[r]).abs().max()),
                    float((r32[r] - ref[r]).abs().max()), F_VIT)


def check_t2i_fold_fields(ops, dev, rep, R, N, T, amp, offset, seed=21):
    """the folded token -> image attention (csrc/t2i_fold.hip): the projections sit inside, so the field is not prescribed;
    instead the token queries are scaled by `amp` and k_proj's bias gets `offset` along output direction 3 of every head
    (a per-query level of offset * tq[.., 3] / 4 logits).  Reference: the fp64 composition of the existing test."""
    from rsprompter_amd.sam_decoder import SamMaskDecoderHIP
    from rsprompter_amd.synth import synth_state_dict
    dec = SamMaskDecoderHIP()
    sd = synth_state_dict(dec, seed)
    key = 'transformer.final_attn_token_to_image.k_proj.bias'
    sd[key] = sd[key].clone()
    sd[key].view(8, 16)[:, 3] += offset
    dec.load_state_dict(sd)
    dec = dec.to(dev)
    dec._pack()
    g = torch.Generator().manual_seed(R * 1000 + N + T)
    keys = torch.randn(R * N, 256, generator=g) * 1.5
    pe = torch.randn(N, 256, generator=g)
    tq = torch.randn(R * T, 128, generator=g) * 2.0 * amp
    at = dec.transformer.final_attn_token_to_image
    wts = [t.detach().cpu() for t in (at.k_proj.weight, at.k_proj.bias, at.v_proj.weight, at.v_proj.bias)]

    def comp(dtype):
        Wk, bk, Wv, bv = (t.to(dtype) for t in wts)
        ks = keys.to(dtype).view(R, N, 256)
        K = ((ks + pe.to(dtype)[None]) @ Wk.t() + bk).view(R, N, 8, 16).permute(0, 2, 1, 3)
        V = (ks @ Wv.t() + bv).view(R, N, 8, 16).permute(0, 2, 1, 3)
        Q = tq.to(dtype).view(R, T, 8, 16).permute(0, 2, 1, 3)
        return (((Q * 0.25) @ K.transpose(-1, -2)).softmax(-1) @ V).permute(0, 2, 1, 3).reshape(R * T, 128).double()
    ref, r32 = comp(torch.float64), comp(torch.float32)
    keys_pl = ops.to_planes(keys.to(dev))
    pe_t = dec._pe_terms(pe.to(dev).contiguous())
    got = dec._t2i_folded('final', tq.to(dev), keys_pl, pe_t, R, T, N)
    rep.add(f'sam_t2i_fold R={R} N={N} T={T} amp={amp:g} offset={offset:g}', float((got.cpu().double() - ref).abs().max()),
            float((r32 - ref).abs().max()), F_VIT)
