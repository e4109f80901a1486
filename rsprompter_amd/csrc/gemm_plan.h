// rsp_gemm's kernel families in one place: the instantiations each GEMM file compiles are listed here ONCE, and both the
// rule that selects one (rsp_gemm_plan, gemm_plan.hip) and the launcher that instantiates it (rsp_gemm_launch_* in the
// kernel's own file) expand the same list -- a form or tile added here is selectable and launchable, one added anywhere else
// does not exist.  Include it after rsp_common.h (it does not include it itself: the emulated build rewrites that include).
#pragma once

// Epilogue forms of gemm_f16x3_s2_kernel / gemm_f16x3_pp_kernel (EPI template argument, RspGemmPlan.epi): bit flags of
// what the tile's outputs need; E_GENERIC = everything at run time (all modes of the descriptor, slow: branches per 4
// outputs; gemm_s2.hip only).
constexpr int E_RES = 1, E_GELU = 2, E_C = 4, E_PL = 8, E_RMAP = 16, E_GENERIC = 64;

// the compile-time forms: X(form)
#define RSP_GEMM_EPILOGUES(X)                                                                            \
  X(E_C)                    /* plain */                                                                  \
  X(E_C | E_RES)            /* proj (global layers), lin2, patch embed */                                \
  X(E_C | E_RES | E_RMAP)   /* proj of a windowed layer (row scatter) */                                 \
  X(E_C | E_PL)             /* qkv (column ranges), fp32 + planes */                                     \
  X(E_C | E_PL | E_RMAP)    /* qkv of a windowed layer: token rows scattered to window order */         \
  X(E_PL)                   /* planes only */                                                            \
  X(E_PL | E_GELU)          /* lin1 */                                                                   \
  X(E_C | E_GELU)

// Instantiations of gemm_f16x3_dma_kernel: X(id, BM, BN, WGM, WGN, NBUF, PIPE, CONV, ORD, F8, ABL).  H<n> is what tile hint
// n asks for (hints >= 4 are benchmarking variants of the same arithmetic), given N > BN / 2; S* are the narrow tiles, C*
// the implicit-GEMM convolutions, F* the fp8-corrected product.
#define RSP_GEMM_DMA_PRODUCT_TILES(X)                                                                      \
  X(H2, 256, 128, 4, 2, 3, 0, false, 0, false, 0)                                                         \
  X(H3, 256, 256, 2, 4, 2, 0, false, 0, false, 0)                                                         \
  X(H4, 256, 128, 4, 2, 2, 0, false, 0, false, 0)                                                         \
  X(H5, 128, 128, 2, 2, 4, 0, false, 0, false, 0)                                                         \
  X(H6, 128, 128, 2, 2, 3, 0, false, 0, false, 0)                                                         \
  X(H11, 256, 256, 2, 4, 2, 1, false, 0, false, 0)     /* register-pipelined loops */                     \
  X(H12, 256, 128, 4, 2, 2, 1, false, 0, false, 0)                                                        \
  X(H13, 256, 128, 4, 2, 3, 1, false, 0, false, 0)                                                        \
  X(H14, 128, 128, 2, 2, 2, 1, false, 0, false, 0)     /* also every N > 64 that no other tile takes */   \
  X(H17, 256, 256, 2, 4, 2, 2, false, 0, false, 0)     /* ... with the DMA spread out */                  \
  X(H18, 256, 128, 4, 2, 2, 2, false, 0, false, 0)                                                        \
  X(H19, 256, 128, 4, 2, 3, 2, false, 0, false, 0)                                                        \
  X(H20, 128, 128, 2, 2, 2, 2, false, 0, false, 0)                                                        \
  X(H21, 128, 64, 2, 2, 3, 1, false, 0, false, 0)      /* narrow tile, 3-deep ring; any N */              \
  X(H22, 128, 64, 2, 2, 4, 1, false, 0, false, 0)                                                         \
  X(H31, 256, 256, 2, 4, 2, 2, false, 1, false, 0)     /* pass-major MFMA order */                        \
  X(H32, 256, 128, 4, 2, 2, 2, false, 1, false, 0)                                                        \
  X(S64, 128, 64, 2, 2, 3, 0, false, 0, false, 0)                                                         \
  X(S32, 128, 32, 4, 1, 3, 0, false, 0, false, 0)                                                         \
  X(C256, 256, 256, 2, 4, 2, 2, true, 0, false, 0)                                                        \
  X(C128, 128, 128, 2, 2, 2, 1, true, 0, false, 0)                                                        \
  X(C64, 128, 64, 2, 2, 3, 0, true, 0, false, 0)                                                          \
  X(C32, 128, 32, 4, 1, 3, 0, true, 0, false, 0)                                                          \
  X(F256, 256, 256, 2, 4, 2, 2, false, 0, true, 0)                                                        \
  X(F256x128, 256, 128, 4, 2, 2, 2, false, 0, true, 0)                                                    \
  X(F128, 128, 128, 2, 2, 2, 1, false, 0, true, 0)

#ifdef RSP_S2_ABLATIONS   /* development builds only (RSP_DEV_BUILD=1): these compute WRONG results on purpose */
#define RSP_GEMM_DMA_TILES(X)                                                                              \
  RSP_GEMM_DMA_PRODUCT_TILES(X)                                                                            \
  X(H7, 128, 128, 2, 2, 2, 0, false, 0, false, 1)      /* ablation: no DMA */                             \
  X(H8, 128, 128, 2, 2, 2, 0, false, 0, false, 2)      /* ablation: no MFMA */                            \
  X(H9, 256, 256, 2, 4, 2, 0, false, 0, false, 1)                                                         \
  X(H10, 256, 256, 2, 4, 2, 0, false, 0, false, 2)                                                        \
  X(H15, 256, 256, 2, 4, 2, 1, false, 0, false, 1)     /* register-pipelined loops without the DMA */     \
  X(H16, 256, 128, 4, 2, 2, 1, false, 0, false, 1)
// experiment variants of the s2 / pp kernels beside VAR = 0: X(VAR, form); tools/gemm_s2_exp.py, tools/gemm_pp_exp.py
#define RSP_GEMM_S2_VARIANTS(X)                                                                            \
  X(1, E_C | E_RES) X(1, E_PL | E_GELU)                  /* raised priority around the DMA slots (round 4) */  \
  X(2, E_C | E_RES) X(2, E_PL | E_GELU) X(2, E_PL) X(8, E_PL)   /* no stores */                            \
  X(4, E_C | E_RES) X(4, E_PL | E_GELU)                  /* no DMA in the loop */                          \
  X(8, E_C | E_RES) X(8, E_PL | E_GELU)                  /* no epilogue */                                 \
  X(16, E_C | E_RES) X(16, E_PL | E_GELU)                /* cache-hot DMA sources */                       \
  X(32, E_C | E_RES) X(32, E_PL | E_GELU)                /* time stamps */                                 \
  X(33, E_C | E_RES) X(33, E_PL | E_GELU)                /* the six DMA slots of a step as one burst (round 4) */ \
  X(1, E_C) X(1, E_C | E_PL)
#define RSP_GEMM_PP_VARIANTS(X) /* both tile heights each */                                               \
  X(4, E_PL | E_GELU) X(32, E_PL | E_GELU) X(4, E_C | E_RES) X(32, E_C | E_RES) X(32, E_C | E_PL)
#else
#define RSP_GEMM_DMA_TILES(X) RSP_GEMM_DMA_PRODUCT_TILES(X)
#define RSP_GEMM_S2_VARIANTS(X)
#define RSP_GEMM_PP_VARIANTS(X)
#endif

// The launchers: the plan names an instantiation of the file's kernel (RSP_EINVAL for one the file does not compile);
// launch geometry -- grid, group_m, the cap bits of the hint, tickets, fastdivs -- is theirs.
int rsp_gemm_launch_f32a(const RspGemmPlan& p, const RspGemmDesc& d, hipStream_t s);   // gemm.hip
int rsp_gemm_launch_dma(const RspGemmPlan& p, const RspGemmDesc& d, hipStream_t s);    // gemm_dma.hip
int rsp_gemm_launch_s2(const RspGemmPlan& p, const RspGemmDesc& d, hipStream_t s);     // gemm_s2.hip
int rsp_gemm_launch_pp(const RspGemmPlan& p, const RspGemmDesc& d, hipStream_t s);     // gemm_pp.hip
