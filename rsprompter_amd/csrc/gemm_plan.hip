// rsp_gemm_plan: every check of an RspGemmDesc and the whole rule that picks the kernel rsp_gemm launches for it -- host
// code only, no device work, so which instantiation a descriptor gets can be tested without a GPU
// (tests/test_gemm_plan_cpu.py against the kernel names recorded on the device, tests/golden/gemm_plan.json).  rsp_gemm
// is: plan, then the chosen file's launcher.  The instantiations come from gemm_plan.h; the ORDER of the checks and
// rules below is part of the contract (M == 0 returns RSP_OK before the conv checks; a descriptor the persistent or
// ping-pong kernel takes never meets the checks of the gemm_dma.hip epilogues).
#include "rsp_common.h"
#include "gemm_plan.h"

namespace {

constexpr int BK = 32;

enum DmaTile {
#define X(ID, ...) ID,
  RSP_GEMM_DMA_TILES(X)
#undef X
};
const RspGemmPlan DMA_TILES[] = {
#define X(ID, BM, BN, WGM, WGN, NBUF, PIPE, CONV, ORD, F8, ABL) {RSP_GEMM_KERNEL_DMA, BM, BN, WGM, WGN, NBUF, PIPE, CONV, ORD, F8, 0, ABL},
    RSP_GEMM_DMA_TILES(X)
#undef X
};

bool compiled_form(int e) {
#define X(E) if (e == (E)) return true;
  RSP_GEMM_EPILOGUES(X)
#undef X
  return false;
}

// a VAR != 0 of the s2 / pp kernel exists for the form (development builds)
#define X(V, E) if (var == V && e == (E)) return true;
bool s2_variant(int var, int e) {
  RSP_GEMM_S2_VARIANTS(X)
  return false;
}
bool pp_variant(int var, int e) {
  RSP_GEMM_PP_VARIANTS(X)
  return false;
}
#undef X

// the shapes / modes gemm_f16x3_s2_kernel implements (everything else stays with gemm_dma.hip)
bool s2_eligible(const RspGemmDesc& d) {
  if (!(d.Ahi && d.Alo) || d.conv_k != 0 || d.ct_W > 0 || d.ln_gamma || d.hd_out) return false;
  if (RSP_PLANE_IS_F8(d.a_scale_log2)) return false;
  if ((d.N & 3) || (d.K & 31) || d.K < 64 || d.M <= 0 || d.a_rows <= 0) return false;
  if (d.C && ((d.ldc & 3) || (reinterpret_cast<uintptr_t>(d.C) & 15))) return false;
  if (d.res && ((d.ldr & 3) || (reinterpret_cast<uintptr_t>(d.res) & 15))) return false;
  if (d.bias && (reinterpret_cast<uintptr_t>(d.bias) & 15)) return false;
  if (d.res_hi && (!d.res_lo || d.res || d.res_rows <= 0)) return false;
  if ((d.pl_col0 & 31) || (d.c_ncols & 3) || d.pl_col0 < 0) return false;
  const long long brows = d.b_rows > 0 ? d.b_rows : d.N;
  const long long kb = d.K / 32;
  if (kb * d.a_rows * 64 >= (1LL << 31) || kb * brows * 64 >= (1LL << 31)) return false;   // 32-bit buffer offsets
  return true;
}

// the epilogue form that serves an s2-eligible descriptor (E_GENERIC: only the run-time form does)
int s2_form(const RspGemmDesc& d) {
  // the branch-free epilogue addresses every tensor it touches with 32-bit buffer offsets
  const long long GB2 = 1LL << 31;
  const long long c_bytes = d.C ? (d.c_rowmap ? (long long)d.c_rows * d.ldc * 4 : 0) : 0;   // no row map: tile-relative
  const long long pl_bytes = d.Chi ? (((long long)((d.N - d.pl_col0) >> 5) * d.c_rows) << 6) : 0;
  const long long res_bytes = d.res ? (long long)(d.res_mod > 0 ? d.res_mod : (d.c_rowmap ? d.c_rows : d.M)) * d.ldr * 4 : 0;
  const bool fast = !(d.N & 63) && !(d.c_ncols & 63) && !(d.pl_col0 & 63) && !d.res_hi &&
                    (d.act == RSP_ACT_NONE || d.act == RSP_ACT_GELU) && !(d.Chi && RSP_PLANE_IS_F8(d.c_scale_log2)) &&
                    !(d.c_rowmap && d.c_rows <= 0) && c_bytes < GB2 && pl_bytes < GB2 && res_bytes < GB2 &&
                    !(d.res && d.res_bmap) &&      /* gathered residual rows: size unknown here, generic path */
                    (long long)256 * d.ldc * 4 < GB2;
  if (!fast) return E_GENERIC;
  const int e = (d.res ? E_RES : 0) | (d.act == RSP_ACT_GELU ? E_GELU : 0) | (d.C ? E_C : 0) | (d.Chi ? E_PL : 0) |
                (d.c_rowmap ? E_RMAP : 0);
  return compiled_form(e) ? e : E_GENERIC;
}

// product rule (round 3): the two-blocks-per-CU persistent kernel wherever it has a specialised epilogue, enough tiles
// (256 x 128) to fill the 512 block slots once and K >= 128 -- 7-20 % faster than the gemm_dma.hip tiles on the ViT-H
// encoder shapes (tools/gemm_s2_exp.py).  Tile hint 1 = "the round-2 rule".
bool s2_auto(const RspGemmDesc& d) {
  if (!s2_eligible(d) || s2_form(d) == E_GENERIC) return false;
  const long long nt = (long long)((d.M + 255) / 256) * ((d.N + 127) / 128);
  return nt >= 256 && d.K >= 128;
}

// the descriptors gemm_f16x3_pp_kernel implements: gemm_s2.hip's, with one of the compile-time epilogues, K >= 128 (the
// K loop is peeled by up to five steps at its end)
bool pp_eligible(const RspGemmDesc& d) { return s2_eligible(d) && d.K >= 128 && s2_form(d) != E_GENERIC; }

// product rule (round 5): 0 = not the ping-pong kernel; 256 / 128 = the block tile's rows.  One block per CU and a static
// walk: a ragged last round idles whole CUs, and the exposed epilogue wants a long K loop.  Measured on the ViT-B / L / H
// encoder shapes (profiles/r5_gemm_pp/pp_{base,large,huge}.txt, TFLOP/s against gemm_s2): 256 x 256 wins wherever its tiles
// fill >= 2 rounds of the 256 CUs to >= 80 % (+6 ... +16 %; +1 ... 3 % at 2.5 rounds); 128 x 256 (phases of 12 MFMAs: 440
// instead of 384 cycles each) only pays for residual GEMMs whose 256-row tiles do not fill the chip (ViT-B proj / lin2:
// +3 ... 9 %).
int pp_auto(const RspGemmDesc& d) {
  if (!pp_eligible(d) || d.K < 512) return 0;
  const long long nbn = (d.N + 255) / 256;
  const long long nt256 = (long long)((d.M + 255) / 256) * nbn, r256 = (nt256 + 255) / 256;
  if (nt256 >= 512 && nt256 * 100 >= r256 * 256 * 80) return 256;
  const long long nt128 = (long long)((d.M + 127) / 128) * nbn, r128 = (nt128 + 255) / 256;
  if (d.res && nt128 >= 512 && nt128 * 100 >= r128 * 256 * 90) return 128;
  return 0;
}

// the gemm_dma.hip tile of a descriptor that passed every check: DmaTile, or -1 for a hint this build does not compile
int dma_tile(const RspGemmDesc& d) {
  const int hint = d.tile_hint & 0xff;
  auto nblk = [&](int bm, int bn) { return (long long)((d.N + bn - 1) / bn) * ((d.M + bm - 1) / bm); };
  // Tile rule (tools/gemm_sweep.py on MI355X; run-to-run spread is a few %): the register-pipelined loops win
  // everywhere; 256x256 needs >= 4 rounds of blocks over the 256 CUs, 256x128 >= 2, else 128x128 (2 blocks/CU).
  if (d.conv_k != 0) {   // implicit-GEMM convolutions: CONV instantiations of the same kernels
    if (d.N > 128 && (hint == 17 || (hint <= 1 && nblk(256, 256) >= 1024))) return C256;
    return d.N > 64 ? C128 : d.N > 32 ? C64 : C32;
  }
  int tile = hint;
  if (tile <= 1) {
    // short K (<= 8 K tiles): the block is mostly prologue + epilogue, two 128x128 blocks per CU overlap them
    // (round 2, tools/gemm_sweep.py on the SAM-decoder shapes M = 3.3 M rows: with N = 256 the 256x256 tile reads every A
    // row once instead of twice and is 7-14 % faster even at 4-8 K tiles; N = 128 stays with 128x128)
    if (d.K <= 256) tile = (d.N > 128 && nblk(256, 256) >= 1024) ? 17 : 14;
    else {
      // cost = rounds over the 256 CUs x tile area / relative efficiency (tools/gemm_sweep.py: 256x256 1.0,
      // 256x128 0.96, 128x128 0.88 with its two blocks per CU sharing the matrix pipe): the partially filled last
      // round is what separates the candidates (e.g. M = 39200, N = 1280: 7 rounds of 256x128 vs 6 of 128x128)
      auto cost = [&](int bm, int bn, int bpc, double eff) {
        const long long nb = nblk(bm, bn), slots = 256LL * bpc;
        return (double)((nb + slots - 1) / slots) * bm * bn * bpc / eff;
      };
      double best = cost(128, 128, 2, 0.88);
      tile = 14;
      if (d.N > 64) { const double c = cost(256, 128, 1, 0.96); if (c < best) { best = c; tile = 18; } }
      if (d.N > 128) { const double c = cost(256, 256, 1, 1.0); if (c <= best) { best = c; tile = 17; } }
      // round 2 (tools/gemm_exp.py, ViT-H shapes): from two full rounds of 256x256 tiles on, the big tile wins even
      // with a ragged last round (blocks do not run in lockstep): qkv 350 vs 322 TFLOP/s, lin2 368 vs 352
      // (K = 1280 with only 3 rounds -- the proj shape -- stays with the small tile: 279 vs 252)
      if (d.N > 128 && (nblk(256, 256) >= 1024 || (nblk(256, 256) >= 512 && d.K >= 2048))) tile = 17;
    }
  }
  if (RSP_PLANE_IS_F8(d.a_scale_log2)) {   // fp8-corrected product: the three tiles the rule above picks
    // with a third less matrix time per tile the big tile already pays from two rounds of blocks on, also at K = 1280
    // (proj shape, tools/gemm_f8_exp.py: 337 vs 301 TFLOP/s)
    if (hint <= 1 && d.N > 128 && nblk(256, 256) >= 512) tile = 17;
    if (tile == 17 && d.N > 128) return F256;
    if ((tile == 18 || tile == 17) && d.N > 64) return F256x128;
    return F128;
  }
  int t = -1;
  switch (tile) {       // a hinted tile is taken when N fills more than half of its width (H21 / H22: always)
#define X(N) case N: t = H##N; break;
    X(2) X(3) X(4) X(5) X(6) X(11) X(12) X(13) X(14) X(17) X(18) X(19) X(20) X(21) X(22) X(31) X(32)
#ifdef RSP_S2_ABLATIONS
    X(7) X(8) X(9) X(10) X(15) X(16)
#else
    case 7: case 8: case 9: case 10: case 15: case 16: return -1;
#endif
#undef X
    default: break;
  }
  if (t >= 0 && (DMA_TILES[t].bn == 64 || d.N > DMA_TILES[t].bn / 2)) return t;
  return d.N > 64 ? H14 : d.N > 32 ? S64 : S32;
}

}  // namespace

extern "C" int rsp_gemm_plan(const RspGemmDesc* desc, RspGemmPlan* plan) {
  if (!plan) return RSP_EINVAL;
  *plan = RspGemmPlan{};        // RSP_GEMM_KERNEL_NONE; filled only where the result is RSP_OK and something launches
  if (!desc) return RSP_EINVAL;
  const RspGemmDesc& d = *desc;
  const bool planes = d.Ahi && d.Alo;
  if (!d.Bhi || !d.Blo) return RSP_EINVAL;
  if (!d.A && !planes) return RSP_EINVAL;
  if (!d.C && !(d.Chi && d.Clo) && !d.hd_out) return RSP_EINVAL;
  if ((d.Chi == nullptr) != (d.Clo == nullptr)) return RSP_EINVAL;
  if (d.Chi && (d.c_rows <= 0 || (d.N & 31))) return RSP_EINVAL;
  if ((d.hd_out || d.ln_gamma || d.res_hi || (d.ct_W > 0 && d.ct_dy < 0)) && !planes) return RSP_EINVAL;   // the fused hyper-network epilogue lives in the plane path
  if (d.M < 0 || d.N <= 0 || d.K <= 0 || (d.K % BK) != 0) return RSP_EINVAL;
  // the fp8-corrected product lives in the plane path: with an fp32 A the cat8 plane of W would be read as a lo plane
  if (RSP_PLANE_IS_F8(d.a_scale_log2) && !planes) return RSP_EINVAL;
  // ... and so do the column-range outputs and the cat8 output planes: the fp32-A kernel writes all N columns of C and
  // plain (hi, lo) planes from column 0
  if (!planes && (d.c_ncols != 0 || d.pl_col0 != 0 || (d.Chi && RSP_PLANE_IS_F8(d.c_scale_log2)))) return RSP_EINVAL;
  if (!RSP_PLANE_WORD_VALID(d.a_scale_log2) || (d.Chi && !RSP_PLANE_WORD_VALID(d.c_scale_log2)) ||
      (d.res_hi && !RSP_PLANE_WORD_VALID(d.res_scale_log2)))
    return RSP_EINVAL;
  if (d.M == 0) return RSP_OK;
  if (d.conv_k != 0) {
    if (d.conv_C % BK != 0) return RSP_EINVAL;
    if (d.K != d.conv_k * d.conv_k * d.conv_C) return RSP_EINVAL;
    if (d.a_rowmap) return RSP_EINVAL;
  } else {
    if ((d.lda & 3) != 0) return RSP_EINVAL;
  }
  if (d.res && d.ldr <= 0) return RSP_EINVAL;
  if (!planes) {                // gemm.hip: A staged through registers, 128 x {128, 64, 32}
    const int bn = d.N > 64 ? 128 : d.N > 32 ? 64 : 32, wgm = bn == 32 ? 4 : 2;
    *plan = RspGemmPlan{RSP_GEMM_KERNEL_F32A, 128, bn, wgm, 4 / wgm};
    return RSP_OK;
  }
  if (d.a_rows <= 0) return RSP_EINVAL;
  const int hint = d.tile_hint & 0xff;
  auto persistent = [&](int kernel, int bm, int bn, int epi, int var) {
    *plan = RspGemmPlan{kernel, bm, bn, 0, 0, 0, 0, 0, 0, 0, epi, var};
    return RSP_OK;
  };
  // tile hints 40 + v: the two-blocks-per-CU persistent kernel (gemm_s2.hip), experiment variant v & 63; bit 6 of v
  // (hint 104) forces the run-time epilogue
  if (hint >= 40 && hint < 168) {
    if (!s2_eligible(d)) return RSP_EINVAL;
    const int var = (hint - 40) & 63, epi = ((hint - 40) & 64) ? E_GENERIC : s2_form(d);
    if (var != 0 && !s2_variant(var, epi)) return RSP_EINVAL;
    return persistent(RSP_GEMM_KERNEL_S2, 256, 128, epi, var);
  }
  // 200 + v: the ping-pong kernel (gemm_pp.hip), forced: bit 0 of v = the 128 x 256 tile; development builds: 4 / 8 / 12
  // ablations, 16 = time stamps (VAR 32)
  if (hint >= 200) {
    const int v = hint - 200, var = ((v & 16) ? 32 : v) & ~1;
    if (!pp_eligible(d)) return RSP_EINVAL;
    if (var != 0 && !pp_variant(var, s2_form(d))) return RSP_EINVAL;
    return persistent(RSP_GEMM_KERNEL_PP, (v & 1) ? 128 : 256, 256, s2_form(d), var);
  }
  if (hint == 0) {
    if (const int bm = pp_auto(d)) return persistent(RSP_GEMM_KERNEL_PP, bm, 256, s2_form(d), 0);
    if (s2_auto(d)) return persistent(RSP_GEMM_KERNEL_S2, 256, 128, s2_form(d), 0);
  }
  if (d.ct_W > 0 && (d.res || d.res_hi)) return RSP_EINVAL;   // no caller needs a residual on a ConvTranspose
  if (d.res_hi && (!d.res_lo || d.res || d.res_rows <= 0 || (d.N & 3))) return RSP_EINVAL;
  if (d.hd_out && (!d.hd_hyper || d.ct_W <= 0 || d.N != (d.ct_dy < 0 ? 128 : 64) || d.hd_rows <= 0)) return RSP_EINVAL;
  if (d.ct_W > 0 && d.ct_dy < 0 && (d.N & 127)) return RSP_EINVAL;
  if (d.ct_W > 0 && d.Chi && ((d.N >> (d.ct_dy < 0 ? 2 : 1)) & 31)) return RSP_EINVAL;
  if (d.conv_k != 0 && (long long)d.conv_H * d.conv_W * ((d.M + (long long)d.conv_Ho * d.conv_Wo - 1) / ((long long)d.conv_Ho * d.conv_Wo)) > 0x7fffffffLL)
    return RSP_EINVAL;   // the implicit-GEMM loader indexes input pixels with 32 bits
  if (d.ln_gamma && (!d.ln_beta || !(d.Chi && d.Clo) || d.C || d.ct_W <= 0 || d.ct_dy >= 0 || d.N != 256 || d.res ||
                     d.c_rowmap || d.hd_out))
    return RSP_EINVAL;
  if (d.hd_out && (d.C || d.Chi || d.res || d.c_rowmap)) return RSP_EINVAL;
  if ((d.pl_col0 || d.c_ncols) && (d.ct_W > 0 || (d.pl_col0 & 31) || (d.c_ncols & 3) || d.pl_col0 < 0 || (d.N & 3)))
    return RSP_EINVAL;   // column-range outputs: plain GEMMs only, plane range on a 32-column boundary
  // fp8-corrected product: the A and W "lo" planes are cat8 planes (the caller pairs them)
  if (RSP_PLANE_IS_F8(d.a_scale_log2) && (d.conv_k != 0 || d.N <= 64)) return RSP_EINVAL;
  if (RSP_PLANE_IS_F8(d.c_scale_log2) && d.Chi && ((d.N & 3) || d.ct_W > 0)) return RSP_EINVAL;
  const int t = dma_tile(d);
  if (t < 0) return RSP_EINVAL;
  *plan = DMA_TILES[t];
  return RSP_OK;
}

extern "C" int rsp_gemm(const RspGemmDesc* desc, rsp_stream_t stream) {
  RspGemmPlan p;
  const int rc = rsp_gemm_plan(desc, &p);
  if (rc != RSP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  switch (p.kernel) {
    case RSP_GEMM_KERNEL_F32A: return rsp_gemm_launch_f32a(p, *desc, s);
    case RSP_GEMM_KERNEL_DMA: return rsp_gemm_launch_dma(p, *desc, s);
    case RSP_GEMM_KERNEL_S2: return rsp_gemm_launch_s2(p, *desc, s);
    case RSP_GEMM_KERNEL_PP: return rsp_gemm_launch_pp(p, *desc, s);
    default: return RSP_OK;     // M == 0
  }
}

// the plan's answers under their earlier names (profiler labels, tests)
static RspGemmPlan plan_of(const RspGemmDesc* d) {
  RspGemmPlan p;
  rsp_gemm_plan(d, &p);         // an error leaves RSP_GEMM_KERNEL_NONE
  return p;
}
extern "C" int rsp_gemm_uses_s2(const RspGemmDesc* d) { return plan_of(d).kernel == RSP_GEMM_KERNEL_S2; }
extern "C" int rsp_gemm_s2_epilogue(const RspGemmDesc* d) {
  const RspGemmPlan p = plan_of(d);
  return p.kernel == RSP_GEMM_KERNEL_S2 ? p.epi : -1;
}
extern "C" int rsp_gemm_uses_pp(const RspGemmDesc* d) {
  const RspGemmPlan p = plan_of(d);
  return p.kernel == RSP_GEMM_KERNEL_PP ? p.bm : 0;
}
