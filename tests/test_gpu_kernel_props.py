"""GPU (`-m gpu`): the kernel property tests of tests/test_wave_emu_cpu.py on the MI355X, at production sizes.

The bodies are tests/_kernel_props.py, the same the emulator tier runs: same references, same assertions, same bounds.
Here the parameters come from a seeded torch.Generator (no hypothesis): a list of edge cases, then at least as many random
draws per property as the emulator's `max_examples`, over ranges the emulator cannot afford (RLE masks up to 1100 x 1100,
GEMMs up to 5000 x 1280 x 1280, 5000 NMS candidates, attention over 4096 keys or queries, fused upscaler launches whose
blocks walk several 128-pixel tiles).  The device is where loads complete late, waves share a SIMD and the issue timing
is real: the emulator sees none of that."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kernel_props as kp  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.quick]


class Draw:
    """seeded parameter draws: one generator per property, so that adding cases to one leaves the others' draws alone"""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def int(self, lo, hi):
        """uniform in [lo, hi]"""
        return int(torch.randint(lo, hi + 1, (1,), generator=self.g))

    def logint(self, lo, hi):
        """log-uniform in [lo, hi]: small and large sizes equally often"""
        u = float(torch.rand(1, generator=self.g))
        return min(hi, max(lo, int(math.exp(math.log(lo) + u * (math.log(hi + 1) - math.log(lo))))))

    def pick(self, seq):
        return seq[self.int(0, len(seq) - 1)]

    def bool(self):
        return self.int(0, 1) == 1

    def seed(self):
        return self.int(0, 2 ** 31 - 1)


def _ops():
    from rsprompter_amd import ops
    return ops


def test_rle_codec_round_trip(dev):
    ops, d = _ops(), Draw(101)
    cases = [(1, 1, 1, 0, 1), (1, 1, 1, 2, 2), (3, 1100, 1100, 1, 3), (1, 1100, 1100, 2, 4), (1, 1100, 1100, 0, 5),
             (1, 1099, 1097, 0, 6), (2, 1100, 1099, 3, 7), (1, 1097, 1100, 4, 8), (2, 1100, 4, 5, 9), (2, 3, 1100, 5, 10)]
    for _ in range(120):
        h, w = d.logint(1, 1100), d.logint(1, 1100)
        if d.bool():
            w = max(4, w - w % 4)                                       # half the draws: the W % 4 == 0 kernel
        cases.append((d.int(1, 3), h, w, d.int(0, 5), d.seed()))
    for (k, h, w, kind, seed) in cases:
        kp.check_rle_round_trip(ops, dev, k, h, w, kind, seed)


def test_gemm_ragged_shapes(dev):
    ops, d = _ops(), Draw(102)
    paths = ['f32', 'planes', 's2']
    cases = [(1, 4, 32, p, True, True, 0) for p in paths] + [(5000, 1280, 1280, p, True, False, 1) for p in paths]
    cases += [(4999, 1276, 1248, p, False, True, 2) for p in paths] + [(257, 132, 64, p, True, False, 0) for p in paths]
    for _ in range(100):
        path = d.pick(paths)
        M, N, K = d.logint(1, 5000), 4 * d.logint(1, 320), 32 * d.logint(1, 40)
        cases.append((M, N, K, path, d.bool(), d.bool(), d.int(0, 2)))
    for (M, N, K, path, with_bias, with_res, act) in cases:
        if path == 's2':
            K = max(K, 64)                                  # rsp_gemm_s2_eligible: K >= 64 (a forced hint on less is EINVAL)
        kp.check_gemm_ragged(ops, dev, M, N, K, path, with_bias, with_res, act, d.seed())


def test_batched_nms(dev):
    ops, d = _ops(), Draw(103)
    cases = [(0, 1, 0.5, 100, 10), (1, 1, 0.5, 1, 10), (5000, 1, 0.7, 1000, 2), (5000, 6, 0.5, 5000, 60), (5000, 80, 0.3, 300, 5),
             (4097, 3, 0.7, 2000, 3)]
    cases += [(d.logint(1, 5000), d.int(1, 80), d.pick([0.3, 0.5, 0.7]), d.logint(1, 5000), d.int(2, 60)) for _ in range(100)]
    for (n, nid, thr, max_out, levels) in cases:
        kp.check_batched_nms(ops, dev, n, nid, thr, max_out, levels, d.seed())


def test_window_attention_grid(dev):
    ops, d = _ops(), Draw(104)
    cases = [(1, 1, 1, 64, 0), (1, 14, 16, 80, 1), (5, 1, 2, 80, 1), (6, 14, 3, 64, 0)]
    cases += [(d.int(1, 6), d.int(1, 14), d.int(1, 16), d.pick([64, 80]), d.int(0, 1)) for _ in range(10)]
    for (nw, real, nh, dh, variant) in cases:
        kp.check_window_attention_grid(ops, dev, nw, real, nh, dh, variant)


LN_WIDTHS = [32, 64, 96, 128, 256, 320, 384, 512, 640, 768, 896, 1024, 1152, 1280, 1408]


def test_layernorm_shapes(dev):
    ops, d = _ops(), Draw(105)
    cases = [(1, C, p) for C in (32, 1408) for p in (False, True)] + [(5000, C, True) for C in (256, 1280, 1408)]
    cases += [(d.logint(1, 5000), d.pick(LN_WIDTHS), d.bool()) for _ in range(70)]
    for (rows, C, planes) in cases:
        kp.check_layernorm(ops, dev, rows, C, planes, d.seed())


def test_attention_shapes(dev):
    ops, d = _ops(), Draw(106)
    cases = [(16, 1, 1, 1), (64, 4096, 1, 2), (32, 1, 4096, 8), (16, 4096, 300, 8), (64, 300, 4096, 4)]
    for _ in range(25):
        big, small = d.logint(1, 4096), d.logint(1, 300)
        Tq, Tk = (big, small) if d.bool() else (small, big)
        cases.append((d.pick([16, 32, 64]), Tq, Tk, d.int(1, 8)))
    for (dh, Tq, Tk, nh) in cases:
        kp.check_generic_attention(ops, dev, dh, Tq, Tk, nh)
    cases = [(1, 1, False, 'mfma'), (10, 4096, True, 'mfma'), (10, 4096, False, 'valu'), (1, 4095, True, 'valu')]
    cases += [(d.int(1, 10), d.logint(1, 4096), d.bool(), d.pick(['valu', 'mfma'])) for _ in range(16)]
    for (T, N, planes_res, form) in cases:
        kp.check_i2t_fused(ops, dev, T, N, planes_res, form)


def test_rpn_selection(dev):
    ops, d = _ops(), Draw(107)
    cases = [(1, 2, 2, 5, 1, -1, 1), (2, 32, 32, 1000, 60, 8, 12), (2, 32, 25, 300, 1000, 0, 1)]
    # nms_pre <= 1024 (rsp_rpn_topk: TK_MAXK; the configurations' test-time value is 1000)
    cases += [(d.int(1, 2), d.int(2, 32), d.int(2, 32), d.pick([5, 40, 300, 1000, 1024]), d.logint(1, 1000), d.pick([-1, 0, 8]),
               d.int(1, 12)) for _ in range(20)]
    for (B, h0, w0, nms_pre, max_per_img, min_size, levels_q) in cases:
        kp.check_rpn_selection(ops, dev, B, h0, w0, nms_pre, max_per_img, min_size, levels_q, d.seed())


def test_bbox_post_and_query_topk(dev):
    ops, d = _ops(), Draw(108)
    cases = [(1, 1, 0.05, 1), (1000, 80, 0.02, 300), (1000, 1, 0.3, 100), (4, 80, 0.05, 100)]
    cases += [(d.logint(1, 1000), d.logint(1, 80), d.pick([0.02, 0.05, 0.3]), d.logint(1, 300)) for _ in range(25)]
    for (n, nc, thr, max_out) in cases:
        kp.check_bbox_post(ops, dev, n, nc, thr, max_out, d.seed())
    # rsp_query_topk takes Nq * nc <= 16384 (EINVAL above; the fusion head has 100 x 80)
    cases = [(1, 1, 1, 1), (2, 300, 54, 100), (2, 100, 80, 100), (1, 204, 80, 16320), (2, 3, 80, 240), (1, 100, 1, 100)]
    cases += [(d.int(1, 2), d.logint(1, 300), d.logint(1, 54), d.logint(1, 300)) for _ in range(25)]
    for (B, Nq, nc, k) in cases:
        kp.check_query_topk(ops, dev, B, Nq, nc, k, d.seed())


def test_sampling_kernels(dev):
    ops, d = _ops(), Draw(109)
    for (K, P) in [(1, 7), (1000, 14), (1000, 7)] + [(d.logint(1, 1000), d.pick([7, 14])) for _ in range(15)]:
        kp.check_roi_align(ops, dev, K, P, d.seed())
    for (L, hd) in [(1, 16), (5, 32)] + [(d.int(1, 5), d.pick([16, 32])) for _ in range(15)]:
        kp.check_msdeform_attn(ops, dev, L, hd, d.seed())
    cases = [(1, 1, 1, 1, 1), (1, 1, 1, 128, 128), (3, 64, 64, 1, 1), (2, 64, 48, 128, 96), (1, 37, 61, 16, 16)]
    cases += [(d.int(1, 3), d.logint(1, 64), d.logint(1, 64), d.logint(1, 128), d.logint(1, 128)) for _ in range(15)]
    for (B, h, w, ho, wo) in cases:
        kp.check_resample(ops, dev, B, h, w, ho, wo, d.seed())


def test_decoder_tail_kernels(dev):
    ops, d = _ops(), Draw(110)
    cases = [(1, 32, 1), (3, 4096, 12), (2, 4096, 8), (1, 4064, 9)]
    cases += [(d.int(1, 3), 32 * d.logint(1, 128), d.int(1, 12)) for _ in range(16)]
    for (R, N, T) in cases:
        kp.check_t2i_fold(ops, dev, R, N, T)
    dec = kp.upscale_decoder(dev, 3)
    # 128-pixel tiles, grid min(ntiles, 256): (40, 64, 64) = 1280 tiles, every block walks 5; (33, 63, 61) ragged
    cases = [(1, 1, 1), (1, 64, 64), (40, 64, 64), (33, 63, 61), (8, 64, 64), (2, 13, 7)]
    cases += [(d.int(1, 40), d.logint(1, 64), d.logint(1, 64)) for _ in range(30)]
    for (R, h, w) in cases:
        kp.check_upscaler(ops, dev, dec, R, h, w, d.seed())


def test_query_prompt_kernels(dev):
    ops, d = _ops(), Draw(111)
    cases = [(1, 1, 1, 1, 256), (30, 2, 64, 64, 256), (7, 2, 37, 53, 512)]
    cases += [(d.int(1, 30), d.int(1, 2), d.logint(1, 64), d.logint(1, 64), d.pick([256, 512])) for _ in range(12)]
    for (R, B, he, we, C) in cases:
        kp.check_mask_embed(ops, dev, R, B, he, we, C, d.seed())
    kp.check_mask_embed_refuses_narrow_channels(ops, dev)
    cases = [(1, 1, 4), (5000, 5000, 256), (1, 300, 100)]
    cases += [(d.logint(1, 5000), d.logint(1, 5000), d.pick([4, 32, 100, 256])) for _ in range(20)]
    for (n_src, n_idx, C) in cases:
        kp.check_gather_rows(ops, dev, n_src, n_idx, C, d.seed())


# ---------------------------------------------------------------------------------------------- prescribed score fields
# tests/_score_fields.py: the logits of every attention kernel prescribed (staircases around the lazy maximum, straddles of its
# threshold, ramps, one-key spikes with their known answer, constant levels below the old padded-key mask, lane-divergent
# forms), each case against the fp64 restatement within max(F, 2 E32).  One function per kernel family; a function runs all
# its cases, prints `case err E32 bound` for each and asserts at the end.
def test_score_fields_window_attention(dev):
    """rsp_vit_window_attention (attn_win_kernel, packed tables): every field, variants 0 / 1, no grid and grids with padded
    queries, dh 64 / 80, fp32 and plane outputs; the levels at every accepted kv exponent class (0, 2, 4); the bias path"""
    import _score_fields as sf
    rep = sf.Report('gpu')
    sf.run_window_family(_ops(), dev, rep, 'window', [(None, 64, 0), ((2, 10), 80, 1), ((3, 4), 64, 1), (None, 80, 0),
                                                      ((2, 10), 64, 0), ((3, 4), 80, 1)], planes=(False, True))
    rep.finish()


def test_score_fields_vit_attention_planes(dev):
    """rsp_vit_attention_planes: S = 14 (the rel tensor form of attn_win_kernel), S = 32 (attn_stream_kernel, tile 64) with
    every field, one S = 64 case per field class; dh 64 / 80, fp32 and plane outputs"""
    import _score_fields as sf
    ops, rep = _ops(), sf.Report('gpu')
    sf.run_window_family(ops, dev, rep, 'planes', [(None, 64, 0), ((2, 10), 80, 0)], planes=(False, True))
    for dh in (64, 80):
        for n, c in enumerate(sf.chunks(sf.global_cases(1024), 4)):
            sf.check_vit_fields(ops, dev, rep, 'planes', 32, 2, 2, dh, c, planes=(False, True) if n % 4 == 0 else (False,), seed=n)
    for kv_e in (0, 4):
        c = sf.pick(sf.global_cases(1024), ['level(-1000)', 'level(300)', 'cold_but_last_tile_hot', 'ramp'])
        sf.check_vit_fields(ops, dev, rep, 'planes', 32, 2, 2, 64, c, kv_e)
    for n, c in enumerate(sf.chunks(sf.pick(sf.global_cases(4096), sf.S64_CASES), 2)):
        sf.check_vit_fields(ops, dev, rep, 'planes', 64, 1, 2, (64, 80)[n % 2], c, planes=(False, True) if n == 0 else (False,), seed=n)
    rep.finish()


def test_score_fields_vit_attention_f32(dev):
    """rsp_vit_attention (fp32-fed: attn_window_kernel at S = 14, attn_global_kernel at S = 32)"""
    import _score_fields as sf
    ops, rep = _ops(), sf.Report('gpu')
    for dh in (64, 80):
        for n, c in enumerate(sf.chunks(sf.window_cases() + sf.window_level_cases()[:-1], 8)):
            sf.check_vit_fields(ops, dev, rep, 'f32', 14, 4, 2, dh, c, seed=n)
    for n, c in enumerate(sf.chunks(sf.global_cases(1024, full=False), 4)):
        sf.check_vit_fields(ops, dev, rep, 'f32', 32, 2, 2, (64, 80)[n % 2], c, seed=n)
    rep.finish()


def test_score_fields_generic_attention(dev):
    """rsp_attention at ragged last tiles"""
    import _score_fields as sf
    ops, rep = _ops(), sf.Report('gpu')
    for (dh, Tq, Tk, nh) in [(16, 10, 300, 8), (64, 70, 130, 2), (32, 33, 257, 2)]:
        sf.check_generic_fields(ops, dev, rep, dh, Tq, Tk, nh)
    rep.finish()


def test_score_fields_sam_cross_attention(dev):
    """rsp_sam_t2i_attention, rsp_sam_t2i_attention_bias (the field in k and in the bias), rsp_sam_i2t_attention (fp32 and
    plane outputs), rsp_sam_i2t_fused (both forms)"""
    import _score_fields as sf
    ops, rep = _ops(), sf.Report('gpu')
    for where in ('k', 'k+bias', 'bias'):
        sf.check_t2i_fields(ops, dev, rep, 7, 600, where)
    for T in (7, 10):
        sf.check_i2t_fields(ops, dev, rep, T, 96)
        for form in ('valu', 'mfma'):
            sf.check_i2t_fused_fields(ops, dev, rep, T, form, 96)
    rep.finish()


def test_score_fields_t2i_fold(dev):
    """the folded token -> image attention: query amplitude x 1 / 8 / 32, a constant offset along one k_proj output direction;
    both head-count instantiations (T <= 8, T > 8)"""
    import _score_fields as sf
    ops, rep = _ops(), sf.Report('gpu')
    for (R, N, T) in [(2, 96, 10), (2, 64, 7)]:
        for amp in (1.0, 8.0, 32.0):
            for offset in (0.0, 20.0):
                sf.check_t2i_fold_fields(ops, dev, rep, R, N, T, amp, offset)
    rep.finish()
