/*
 * rsp_hip.h -- C ABI of librsp_hip.so: the MI355X (gfx950) kernels behind the
 * RSPrompter inference hot path (SAM ViT encoder -> anchor prompter -> SAM mask
 * decoder).
 *
 * Conventions
 *   - every entry point is `extern "C"`, takes raw DEVICE pointers, explicit
 *     sizes/strides and a HIP stream handle (`void*` == hipStream_t), and
 *     returns 0 on success or a negative RSP_E* code (Python maps !=0 to
 *     RuntimeError).  No torch types, no global state.
 *   - all activations are fp32, row-major, channels-last ("NHWC": a feature map
 *     is a [B*H*W, C] matrix).  GEMM weights are passed pre-split into two fp16
 *     planes (hi, lo) produced by rsp_split_f16 (see DESIGN.md "fp16x3").
 *   - "reference" citations are relative to /root/reference, `HF:` is
 *     transformers/models/sam/modeling_sam.py (the reference's pinned
 *     third-party SAM implementation).
 */
#ifndef RSP_HIP_H_
#define RSP_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSP_OK 0
#define RSP_EINVAL (-1)   /* bad argument / unsupported shape */
#define RSP_ELAUNCH (-2)  /* hipLaunch / runtime error         */

#define RSP_ACT_NONE 0
#define RSP_ACT_RELU 1
#define RSP_ACT_GELU 2    /* exact erf GELU (torch nn.GELU default) */
#define RSP_ACT_SIGMOID 3
#define RSP_ACT_RELU_POST 4   /* C = relu(alpha*acc + bias + res): the ReLU after the shortcut of a ResNet block */

typedef void* rsp_stream_t;

/* Library / build identification (also used by the "symbols load" CPU test).  This header is the ONLY declaration of   */
/* the ABI: rsprompter_amd/_lib.py parses it at import into the ctypes prototypes, the descriptor structures and a table  */
/* of the integer macros below (limits included), so keep to the C subset that parser reads (its docstring lists it).     */
/* An addition that leaves every earlier entry point, structure and macro as it was does not change the number (under 5:  */
/* rsp_gemm_plan and the run-table, polygon, simplification, oriented-box, component and rasterisation entry points).     */
/* 6: rsp_run_pieces_count (was rsp_mask_polygon_pieces) and rsp_run_pieces write the column-piece table, which           */
/* rsp_mask_polygon_edges and rsp_run_components_label read in place of counts / n / cap;                                 */
/* 5: rsp_sam_fold_expand / rsp_sam_fold_gather; 4: rsp_sam_t2i_fold lost its `variant` argument, rsp_gemm_uses_pp;       */
/* 3: RspBoxCoder in RspRpnDesc / rsp_bbox_post; 2: RspGemmDesc gained c_ncols / pl_col0, plane format words decode       */
/* strictly.                                                                                                             */
#define RSP_ABI_VERSION 6
int rsp_abi_version(void);   /* = RSP_ABI_VERSION of the header the library was built from */
const char* rsp_build_info(void);

/* ------------------------------------------------------------------------ */
/* Plane format word                                                          */
/* ------------------------------------------------------------------------ */
/* Every `*_scale_log2` argument / descriptor field that describes a pair of fp16 planes is a FORMAT WORD:          */
/*   bits 0..7  (signed)  e: the planes hold x * 2^e                                                                  */
/*   bit  8     RSP_PLANE_F8: the second plane is not lo = f16(x*2^e - hi) but the "cat8" plane of the                */
/*              fp8-corrected product (same bytes: 64 per row and 32-wide K block):                                   */
/*                bytes  0..31  e4m3(lo[k] * 2^RSP_F8_LO_EXP)      bytes 32..63  e4m3(hi[k] * 2^-RSP_F8_HI_EXP)       */
/*              A GEMM whose A and B words both carry the bit computes                                                */
/*                a_hi b_hi  (fp16 MFMA)  +  a_lo8 b_hi8 + a_hi8 b_lo8  (ONE K=64 fp8 MFMA per 32 k, MX block scales  */
/*                2^-LO_EXP / 2^+HI_EXP undo the storage scales)                                                      */
/*              -- 2 units of matrix time instead of 3, error class 2^-15 instead of 2^-22.     */
/* Decoding is strict: a word is an F8 word only when its upper bits are exactly RSP_PLANE_F8; a plain (sign-extended)   */
/* negative exponent -- legal under the pre-format-word contract of these fields -- has all upper bits set and is NOT  */
/* mistaken for one; any other upper-bit pattern is invalid (entry points return RSP_EINVAL).                          */
#define RSP_PLANE_F8 0x100
#define RSP_PLANE_EXP(w) ((int)(int8_t)((w) & 0xff))
#define RSP_PLANE_IS_F8(w) ((((int32_t)(w)) & ~0xff) == RSP_PLANE_F8)
#define RSP_PLANE_WORD_VALID(w) \
  (RSP_PLANE_IS_F8(w) || (((int32_t)(w)) & ~0xff) == 0 || (((int32_t)(w)) & ~0xff) == ~0xff)
#define RSP_PLANE_WORD(e, f8) ((((int)(e)) & 0xff) | ((f8) ? RSP_PLANE_F8 : 0))
#define RSP_F8_LO_EXP 5
#define RSP_F8_HI_EXP 7

/* ------------------------------------------------------------------------ */
/* Weight preparation                                                        */
/* ------------------------------------------------------------------------ */
/* hi = f16(w * 2^e), lo = f16(w * 2^e - hi).  n elements.                   */
int rsp_split_f16(const float* w, uint16_t* hi, uint16_t* lo, int64_t n,
                  int scale_log2, rsp_stream_t stream);
/* same for a row-major [rows, K] matrix (K % 32 == 0), written in the KB32     */
/* plane layout [K/32][rows][32] that the DMA GEMM path consumes.               */
int rsp_split_f16_kb32(const float* w, uint16_t* hi, uint16_t* lo, int64_t rows, int32_t K,
                       int scale_log2, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* GEMM with fused prologue/epilogue: the workhorse.                          */
/*   C[crow(m), n] = act(alpha * sum_k A(m,k) * B[n,k] + bias[n]) + res       */
/* replaces: every nn.Linear / 1x1 conv / 3x3 conv / ConvTranspose2d(k2,s2)   */
/* on the path -- HF:116-128 (patch embed), HF:717,806-812 (qkv), HF:830      */
/* (proj), HF:132-143 (MLP), HF:975-992 (neck), models.py:1009-1057           */
/* (aggregator), models.py:1296-1363 (SimpleFPN), rpn_head.py:80-97,          */
/* convfc_bbox_head.py:163-217, models.py:1641-1651, HF:231-270, HF:447-450.  */
/* ------------------------------------------------------------------------ */
typedef struct RspGemmDesc {
  const float* A;          /* [*, lda] fp32 (plain mode) or NHWC image (conv) */
  const uint16_t* Bhi;     /* [N, K] fp16 hi plane of the weight              */
  const uint16_t* Blo;     /* [N, K] fp16 lo plane                            */
  float* C;                /* [*, ldc]                                        */
  const float* bias;       /* [N] or NULL                                     */
  const float* res;        /* residual [*, ldr] or NULL (added after act)     */
  const int32_t* a_rowmap; /* [M] source row of A per GEMM row, -1 => zeros   */
  const int32_t* c_rowmap; /* [M] destination row of C, -1 => drop            */
  int32_t M, N, K;         /* K % 32 == 0                                     */
  int32_t lda, ldc, ldr;
  int32_t res_mod;         /* >0: residual row = crow % res_mod (broadcast)   */
  int32_t act;             /* RSP_ACT_*                                       */
  float alpha;             /* 2^-(a_scale_log2 + weight scale_log2)           */
  int32_t a_scale_log2;    /* plane format word of A (and of W): exponent e of the   */
                           /* fp16 split, RSP_PLANE_F8 selects the fp8-corrected     */
                           /* product (A planes and W planes then both carry cat8)   */
  /* implicit-GEMM convolution over an NHWC input (conv_k == 0: plain GEMM)   */
  int32_t conv_k;          /* kernel size (3) ; K must equal conv_k^2 * conv_C */
  int32_t conv_stride, conv_pad;
  int32_t conv_H, conv_W, conv_C; /* input  spatial size / channels           */
  int32_t conv_Ho, conv_Wo;       /* output spatial size; M = B*Ho*Wo         */
  /* ConvTranspose2d(k=2,s=2) as two GEMMs (one per output row parity dy) with  */
  /* N = 2*Cout (dx, co): GEMM row (y*W + x) -> C row ((y*2 + dy)*W + x) of an   */
  /* output viewed as [B*2H*W, 2*Cout].  ct_W == 0 disables.                     */
  int32_t ct_W, ct_dy;
  /* residual batch gather: residual row = res_bmap[crow / res_brows] * res_brows */
  /* + crow % res_brows  (per-RoI rows adding their image's rows). NULL disables. */
  const int32_t* res_bmap;
  int32_t res_brows;
  /* fp16 "plane" operands/results: A given as two fp16 tensors (hi, lo) of      */
  /* x * 2^a_scale_log2 in the K-BLOCKED layout [K/32][a_rows][32] ("KB32": every 128x32 K tile   */
  /* of a plane is one contiguous 8 KiB run of full cache lines) -> the DMA fast path             */
  /* (global_load_lds, no register staging).  Weights (Bhi/Blo) use the same layout [K/32][N][32] */
  /* when A is given as planes.  Chi/Clo: additionally (or, with C == NULL, only) write the       */
  /* result pre-split, scale 2^c_scale_log2, KB32 layout [N/32][c_rows][32], for the next GEMM.   */
  const uint16_t* Ahi; const uint16_t* Alo;
  uint16_t* Chi; uint16_t* Clo;
  int32_t c_scale_log2;    /* plane format word of Chi / Clo (RSP_PLANE_F8: Clo is written as the cat8 plane) */
  int32_t a_rows, c_rows;
  int32_t b_rows;   /* rows of the Bhi/Blo plane tensors when the weight is a row slice of them (0 = N) */
  /* hyper-network epilogue (HF:523-531 fused into the last ConvTranspose of the SAM upscaler): instead of  */
  /* storing the [rows, N] tile, every 32-column group g of a row is reduced against hyper[row / hd_rows]:   */
  /* hd_out[(row / hd_rows) * hd_ostride + pix(row, g)] = sum_c act(...)[row, 32g + c] * hyper[., c]          */
  /* (pix = the sub-pixel the 32-column group writes); needs A planes, ct_W > 0 and N == 64 (ct_dy >= 0) or   */
  /* N == 128 (ct_dy < 0: columns are (dy, dx, co), all four sub-pixels from one pass over A).                */
  /* grouped-LayerNorm epilogue (HF:519-520 fused into the first ConvTranspose of the SAM upscaler): with  */
  /* ct_W > 0, ct_dy < 0 and N == 256 every 64-column group (one output sub-pixel) is normalised over its  */
  /* 64 channels (LayerNorm2d, eps ln_eps, affine ln_gamma/ln_beta [64]) BEFORE `act`; plane output only.  */
  const float* ln_gamma; const float* ln_beta; float ln_eps;
  /* residual given as fp16 planes (KB32 [N/32][res_rows][32], value * 2^res_scale_log2) instead of fp32 `res`:    */
  /* C = act(...) + (hi + lo) * 2^-e, rows mapped like `res` (res_mod / res_bmap).                                */
  const uint16_t* res_hi; const uint16_t* res_lo; int32_t res_scale_log2, res_rows;
  const float* hd_hyper; float* hd_out;
  int32_t hd_rows;    /* GEMM rows per RoI (input pixels of the ConvTranspose)                                */
  /* column-range outputs (plane path, plain GEMMs): fp32 C is written only for columns < c_ncols (0 = all, same ldc),  */
  /* the planes Chi/Clo only for columns >= pl_col0 (pl_col0 % 32 == 0) as a [c_rows, N - pl_col0] KB32 tensor.          */
  /* The SAM ViT qkv projection uses c_ncols = pl_col0 = D: q leaves as fp32 (rel-pos + attention Q operand), K | V      */
  /* as the fp16 planes the attention kernel DMAs (rsp_vit_attention_planes) -- no fp32 K / V tensor is ever written.    */
  int32_t c_ncols, pl_col0;
  int32_t tile_hint;  /* bits 0..7: 0 = auto (rsp_gemm_plan).  Benchmarking only: 1 = auto among the csrc/gemm_dma.hip   */
                      /* tiles, H<n> of the table in csrc/gemm_plan.h = tile n of that file (taken when N fills more    */
                      /* than half its width), 40 + v = gemm_s2.hip variant v (104: run-time epilogue), 200 / 201 =     */
                      /* gemm_pp.hip 256 / 128 x 256; bits 8..15: group_m, bits 16..23: gemm_pp blocks per XCD.         */
} RspGemmDesc;

int rsp_gemm(const RspGemmDesc* desc, rsp_stream_t stream);

/* The kernel rsp_gemm launches for a descriptor: every check of the descriptor and the whole selection rule, host code     */
/* only (csrc/gemm_plan.hip; no device work, nothing is dereferenced).  rsp_gemm itself is rsp_gemm_plan + the launch.      */
#define RSP_GEMM_KERNEL_NONE 0   /* M == 0: nothing to launch */
#define RSP_GEMM_KERNEL_F32A 1   /* csrc/gemm.hip gemm_f16x3_kernel<bm, bn, wgm, wgn>: fp32 A staged through registers */
#define RSP_GEMM_KERNEL_DMA 2    /* csrc/gemm_dma.hip gemm_f16x3_dma_kernel<bm, bn, wgm, wgn, nbuf, var, 0, pipe, conv, ord, f8> */
#define RSP_GEMM_KERNEL_S2 3     /* csrc/gemm_s2.hip gemm_f16x3_s2_kernel<var, epi>: persistent, two blocks per CU, 256 x 128 */
#define RSP_GEMM_KERNEL_PP 4     /* csrc/gemm_pp.hip gemm_f16x3_pp_kernel<epi, var, bm>: ping-pong, one 512-thread block per CU */
typedef struct RspGemmPlan {
  int32_t kernel;          /* RSP_GEMM_KERNEL_* */
  int32_t bm, bn;          /* block tile */
  int32_t wgm, wgn, nbuf, pipe, conv, ord, f8;   /* the gemm.hip / gemm_dma.hip instantiation; 0 elsewhere */
  int32_t epi;             /* s2 / pp: epilogue form, bit flags 1 = fp32 residual, 2 = GELU, 4 = fp32 output, 8 = plane    */
                           /* output, 16 = output row map; 64 = the run-time form that serves every other mode            */
  int32_t var;             /* experiment variant (VAR of s2 / pp, ABL of dma): 0 in every shipped library                 */
} RspGemmPlan;
/* RSP_OK / RSP_EINVAL exactly where rsp_gemm returns them; on RSP_EINVAL and for M == 0 *plan is RSP_GEMM_KERNEL_NONE.     */
int rsp_gemm_plan(const RspGemmDesc* desc, RspGemmPlan* plan);
/* The plan under its earlier names: plan.kernel == RSP_GEMM_KERNEL_S2;  plan.epi then, else -1;  plan.bm (256 / 128) when   */
/* plan.kernel == RSP_GEMM_KERNEL_PP, else 0.  tile_hint 200 / 201 force the two ping-pong tiles for every descriptor that   */
/* kernel implements (those with one of the compile-time epilogue forms and K >= 128).                                      */
int rsp_gemm_uses_s2(const RspGemmDesc* desc);
int rsp_gemm_s2_epilogue(const RspGemmDesc* desc);
int rsp_gemm_uses_pp(const RspGemmDesc* desc);

/* ------------------------------------------------------------------------ */
/* LayerNorm over the last dim of a [rows, C] matrix (C % 4 == 0, C <= 2048). */
/* replaces nn.LayerNorm(eps=1e-6) HF:894-896 and every channel LN on NHWC    */
/* data: SamLayerNorm(channels_first) HF:147-170, LN2d models.py:33-50.       */
/* act: RSP_ACT_NONE or RSP_ACT_GELU (fused LN->GELU of models.py:1299-1300,  */
/* HF:519-520).                                                               */
/* ------------------------------------------------------------------------ */
int rsp_layernorm(const float* x, const float* gamma, const float* beta, float* y,
                  int64_t rows, int32_t C, float eps, int32_t act, rsp_stream_t stream);
/* same, optionally writing the result as fp16 planes (hi, lo of y * 2^scale_log2; KB32 layout  */
/* [C/32][rows][32], C % 32 == 0) for a following plane-mode GEMM; y may then be NULL.          */
int rsp_layernorm_ex(const float* x, const float* gamma, const float* beta, float* y,
                     uint16_t* yhi, uint16_t* ylo, int32_t scale_log2, int64_t rows, int32_t C,
                     float eps, int32_t act, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* SAM ViT attention (windowed and global) with decomposed rel-pos bias.      */
/* replaces SamVisionAttention.forward HF:803-831 + get_decomposed_rel_pos    */
/* HF:761-801 (vit_sam.py:117-157, 202-221).                                  */
/* ------------------------------------------------------------------------ */
/* rel[bp*nh + h, t, 0:S]   = q(t) . Rh[qh(t) - kh + S-1]   (unscaled q)       */
/* rel[bp*nh + h, t, S:2S]  = q(t) . Rw[qw(t) - kw + S-1]                      */
/* qkv: [Bp, T, 3, nh, dh] fp32 (T = S*S), rel_pos_{h,w}: [2S-1, dh].          */
int rsp_vit_relpos(const float* qkv, const float* rel_pos_h, const float* rel_pos_w,
                   float* rel, int32_t Bp, int32_t S, int32_t nh, int32_t dh,
                   rsp_stream_t stream);

/* out[Bp, T, nh*dh] = softmax_fp32((q*scale) k^T + rel_h (+) rel_w) v         */
int rsp_vit_attention(const float* qkv, const float* rel, float* out,
                      int32_t Bp, int32_t S, int32_t nh, int32_t dh, float scale,
                      rsp_stream_t stream);
/* same with an optional fp16-plane copy of the output (KB32 layout [D/32][Bp*T][32]; feeds the  */
/* proj GEMM's DMA path)                                                                         */
int rsp_vit_attention_ex(const float* qkv, const float* rel, float* out, uint16_t* out_hi,
                         uint16_t* out_lo, int32_t out_scale_log2, int32_t Bp, int32_t S,
                         int32_t nh, int32_t dh, float scale, rsp_stream_t stream);
/* Global-attention layers (S == 64 or 32): K and V of every (image, head) are split once into fp16 hi/lo planes   */
/* rsp_vit_attention_planes: the same attention with K | V given as the KB32 fp16 planes [2D/32][kv_rows][32] of the  */
/* qkv GEMM (value * 2^kv_scale_log2) and q as fp32 rows of stride q_ld: DMA-fed key tiles, transposing LDS reads for  */
/* V (csrc/attn_stream.hip).  S = 14 (windows), 32, 64; dh = 64 / 80.  Outputs as rsp_vit_attention_ex.                */
int rsp_vit_attention_planes(const float* q, int64_t q_ld, const uint16_t* kv_hi, const uint16_t* kv_lo,
                             int64_t kv_rows, int32_t kv_scale_log2, const float* rel, float* out, uint16_t* out_hi,
                             uint16_t* out_lo, int32_t out_scale_log2, int32_t Bp, int32_t S, int32_t nh, int32_t dh,
                             float scale, rsp_stream_t stream);
/* ... with the window grid of window_partition (HF:900-922) known: the Bp windows are (image, wy, wx) over a            */
/* win_per_side x win_per_side grid whose last row / column holds only win_real_last real rows / columns (64-grid, 14:    */
/* 5 and 8).  Outputs of the padded tokens are NOT written (window_unpartition crops them); their keys / values take     */
/* part as usual.  win_per_side = 0: every query is computed (= rsp_vit_attention_planes).                                */
int rsp_vit_attention_planes_ex(const float* q, int64_t q_ld, const uint16_t* kv_hi, const uint16_t* kv_lo,
                                int64_t kv_rows, int32_t kv_scale_log2, const float* rel, float* out,
                                uint16_t* out_hi, uint16_t* out_lo, int32_t out_scale_log2, int32_t Bp, int32_t S,
                                int32_t nh, int32_t dh, float scale, int32_t win_per_side, int32_t win_real_last,
                                rsp_stream_t stream);
/* Windowed layers, rel-pos terms computed INSIDE the attention kernel (csrc/attn_win.hip; replaces the pair             */
/* rsp_vit_relpos_rows + rsp_vit_attention_planes_ex of a windowed SamVisionAttention.forward, HF:803-831 + 761-801):     */
/* rel_tab = the layer's two tables packed once by rsp_pack_relpos_tables; q / K | V planes / outputs / window grid as    */
/* above with S = 14.  The kernel is persistent (a block walks the windows of one head); variant: 0 = product (768        */
/* blocks), n > 0 = 16 n blocks (tests and measurements).                                                                 */
/* Input domain for S = 14 (both entry points).  The K | V plane exponent (kv_scale_log2) must lie in [-8, 4], else       */
/* RSP_EINVAL.  Inside the kernel scaled q travels as fp16 hi / lo of q * scale * 2^6 and every rel-pos term of a query as  */
/* fp16 hi / lo of term * 2^(6 + exponent), both through SATURATING splits: the result is fp32-class for                   */
/* |q * scale| < 1024 per element and |rel-pos term| * 2^(6 + exponent) <= 65504 (256 logits at the encoder's exponent 2,  */
/* 64 at 4, 1023 at 0); beyond that the operand is clamped silently (no error, no inf / NaN).  The level of the scores     */
/* themselves sets no limit: the 28 padded keys of the last tile are masked with -inf, their probability is exactly 0.     */
int rsp_vit_window_attention(const float* q, int64_t q_ld, const uint16_t* kv_hi, const uint16_t* kv_lo,
                             int64_t kv_rows, int32_t kv_scale_log2, const uint16_t* rel_tab, float* out,
                             uint16_t* out_hi, uint16_t* out_lo, int32_t out_scale_log2, int32_t Bp, int32_t nh,
                             int32_t dh, float scale, int32_t win_per_side, int32_t win_real_last, int32_t variant,
                             rsp_stream_t stream);
/* rel_pos_h / rel_pos_w [2S-1, dh] fp32 (2S-1 <= 32, dh % 8 == 0) -> out [2][2][32][dh + 8] fp16: per table the hi and   */
/* lo planes of table * 2^6, rows >= 2S-1 and the 8 pad columns zero (16-byte aligned, 2*2*32*(dh+8) halves)               */
int rsp_pack_relpos_tables(const float* rel_pos_h, const float* rel_pos_w, uint16_t* out, int32_t S, int32_t dh,
                           rsp_stream_t stream);
/* rsp_vit_relpos with an explicit token stride of q (q rows of [Bp*T, q_ld], head h at column h*dh)                   */
int rsp_vit_relpos_q(const float* q, int64_t q_ld, const float* rel_pos_h, const float* rel_pos_w, float* rel,
                     int32_t Bp, int32_t S, int32_t nh, int32_t dh, rsp_stream_t stream);
/* ... for a list of rows only (windowed layers): rows_map[n_rows] = the q / rel rows to compute, e.g. the real tokens  */
/* of padded windows -- the rel rows of padded queries are never read once the attention skips them                     */
/* (rsp_vit_attention_planes_ex).  rows_map = NULL: all Bp*S*S rows.                                                     */
int rsp_vit_relpos_rows(const float* q, int64_t q_ld, const float* rel_pos_h, const float* rel_pos_w, float* rel,
                        int32_t Bp, int32_t S, int32_t nh, int32_t dh, const int32_t* rows_map, int64_t n_rows,
                        rsp_stream_t stream);
/* (K as [key][dh], V transposed) inside `workspace` (rsp_vit_attention_global_ws_bytes) and the attention kernel   */
/* streams them HBM -> LDS with the DMA engine.  Same semantics and outputs as rsp_vit_attention_ex.                */
int64_t rsp_vit_attention_global_ws_bytes(int32_t Bp, int32_t S, int32_t nh, int32_t dh);
int rsp_vit_attention_global(const float* qkv, const float* rel, void* workspace, float* out, uint16_t* out_hi,
                             uint16_t* out_lo, int32_t out_scale_log2, int32_t Bp, int32_t S, int32_t nh, int32_t dh,
                             float scale, rsp_stream_t stream);

/* Generic multi-head attention out = softmax((q*scale) k^T) v with strided    */
/* operands (element strides; all multiples of 4), used by the SAM mask        */
/* decoder: SamAttention.forward HF:231-270 (self-attn dh=32, token<->image    */
/* cross-attn dh=16 with 4096 image keys).  kv_batch_map lets several query    */
/* batches (RoIs) share one K/V batch (their image).  dh in {16, 32, 64}.      */
typedef struct RspAttnDesc {
  const float* q; const float* k; const float* v; float* out;
  const int32_t* kv_batch_map;   /* [B] or NULL */
  const int32_t* q_batch_map;    /* [B] or NULL: batch b reads Q of batch q_batch_map[b] */
  int64_t q_bs, q_ts, q_hs;      /* batch / token / head strides (elements)   */
  int64_t k_bs, k_ts, k_hs;
  int64_t v_bs, v_ts, v_hs;
  int64_t o_bs, o_ts, o_hs;
  int32_t B, nh, dh, Tq, Tk;
  float scale;
  /* optional fp16-plane (KB32) copy of a dense [B*Tq, nh*dh] output; `out` may then be NULL */
  uint16_t* out_hi; uint16_t* out_lo; int32_t out_scale_log2;
  /* optional attention mask [B, Tq, Tk] bytes, non-zero = blocked, shared by all heads               */
  /* (Mask2Former masked cross-attention, mask2former_layers.py:113-121)                               */
  const uint8_t* mask;
} RspAttnDesc;
int rsp_attention(const RspAttnDesc* desc, rsp_stream_t stream);

/* SAM two-way transformer cross attentions, internal width 128 = 8 heads x 16 (HF:243-288 as used by HF:306-348 and */
/* HF:396-404), exact fp32:                                                                                          */
/*  token -> image: q [R,T,128] (T <= 12), kv [Rkv*N, 256] = image rows with K | V side by side, kv_map[r] = image    */
/*  row block of RoI r (NULL: r); out [R,T,128].                                                                      */
#define RSP_SAM_T2I_MAX_TOKENS 12        /* more tokens go through the generic rsp_attention */
int rsp_sam_t2i_attention(const float* q, const float* kv, const int32_t* kv_map, float* out, int32_t R, int32_t T,
                          int32_t N, float scale, rsp_stream_t stream);
/*  token -> image with a key bias (HF:260 `attn = attn + attention_similarity` in front of the softmax, as HF:328-330  */
/*  passes it to cross_attn_token_to_image of both two-way layers -- PerSAM's hook): bias [Rb, N], Rb = 1 (one row for  */
/*  every RoI) or R; s = q . k * scale + bias[n].  Everything else as rsp_sam_t2i_attention, whose kernels are unchanged. */
int rsp_sam_t2i_attention_bias(const float* q, const float* kv, const int32_t* kv_map, const float* bias, int32_t Rb,
                               float* out, int32_t R, int32_t T, int32_t N, float scale, rsp_stream_t stream);
/*  image -> token: q [Rq*N,128] image-side queries (q_map[r] = row block, NULL: r), k, v [R,T,128] (T <= 16);        */
/*  result [R*N,128] as fp32 `out` and/or fp16 planes (KB32, value * 2^out_scale_log2).                               */
#define RSP_SAM_I2T_MAX_TOKENS 16
int rsp_sam_i2t_attention(const float* q, const int32_t* q_map, const float* k, const float* v, float* out,
                          uint16_t* out_hi, uint16_t* out_lo, int32_t out_scale_log2, int32_t R, int32_t T, int32_t N,
                          float scale, rsp_stream_t stream);
/*  image -> token attention FUSED with out_proj, the residual and layer_norm4 (HF:340-348):                          */
/*    y = LayerNorm(residual + out_proj(attention(q, k, v)))   rows [R*N, 256]                                        */
/*  out_proj is folded into the values (exact algebra, fp32), so the [R*N,128] attention output, the K = 128 GEMM over */
/*  it and the separate LayerNorm pass are never materialised.  wo [256,128], bo [256] = out_proj; the residual is      */
/*  either fp32 rows `res` [Rres*N, 256] with res_map[r] = row block of RoI r (NULL: r) -- layer 0, one copy per image   */
/*  -- or fp16 planes res_hi / res_lo of the [R*N, 256] tensor (layer 1); result as fp32 `out` and/or fp16 planes.      */
/*  T <= RSP_SAM_I2T_FUSED_MAX_TOKENS (the LDS budget); more tokens: rsp_sam_i2t_attention + GEMM + layernorm.          */
#define RSP_SAM_I2T_FUSED_MAX_TOKENS 10
typedef struct RspI2tFusedDesc {
  const float* q; const int32_t* q_map; const float* k; const float* v;
  const float* wo; const float* bo;
  const float* res; const int32_t* res_map;
  const uint16_t* res_hi; const uint16_t* res_lo; int32_t res_scale_log2;
  const float* gamma; const float* beta; float eps;
  float* out; uint16_t* out_hi; uint16_t* out_lo; int32_t out_scale_log2;
  int32_t R, T, N; float scale;
} RspI2tFusedDesc;
int rsp_sam_i2t_fused(const RspI2tFusedDesc* desc, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* RoI feature extraction (single_level_roi_extractor.py:44-119 + mmcv RoIAlign, */
/* sampling_ratio=0, aligned=True) over <=4 NHWC levels; `pe` adds an          */
/* input-independent positional map per level (models.py:1566-1574) on the fly. */
/* out: [K, P, P, C].                                                          */
/* ------------------------------------------------------------------------ */
typedef struct RspRoiAlignDesc {
  const float* feat[4];      /* [B, H, W, C] per level                         */
  const float* pe[4];        /* [H, W, C] per level or NULL                    */
  int32_t H[4], W[4];
  float spatial_scale[4];    /* 1/stride                                       */
  const float* rois;         /* [K, 5] (batch index, x1, y1, x2, y2)           */
  float* out;
  int32_t K, P, C, num_levels, finest_scale;
} RspRoiAlignDesc;
int rsp_roi_align(const RspRoiAlignDesc* desc, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Proposal / detection selection (rpn_head.py:134-304, bbox_head.py:476-571, */
/* bbox_nms.py:12-105, delta_xywh_bbox_coder.py:264-361, mmcv batched_nms).    */
/* Deterministic: ties are (score desc, position asc).                         */
/* ------------------------------------------------------------------------ */
/* DeltaXYWHBBoxCoder.decode (delta_xywh_bbox_coder.py:71-131 -> delta2bbox,  */
/* :264-361): denormalise with stds / means, clamp, optionally clip to the    */
/* image.  Every step rounds as the reference's eager fp32 expression does.   */
typedef struct RspBoxCoder {
  float means[4], stds[4];   /* target_means / target_stds                     */
  float max_ratio;           /* |log(wh_ratio_clip)|                           */
  float ctr_clamp;           /* pixels; read when add_ctr_clamp != 0           */
  int32_t clip_border;       /* clamp to [0, w] x [0, h] of img_hw             */
  int32_t add_ctr_clamp;     /* :340-342 (YOLOF form): clamp the centre shift, */
                             /* sizes bounded from above only                  */
} RspBoxCoder;
typedef struct RspRpnDesc {
  const float* head[5];      /* per level [B*H*W, ld]: cols [0,A) objectness,  */
                             /* cols [A, 5A) deltas (anchor-major)             */
  int32_t H[5], W[5];
  float stride[5];
  int32_t ld, A, nms_pre, num_levels;
  const float* base_anchors; /* device [L, A, 4] (anchor_generator.py:161-205) */
  RspBoxCoder coder;         /* rpn_head.bbox_coder                            */
  float min_bbox_size;       /* <0 disables the w/h filter                     */
} RspRpnDesc;
/* sel_idx/sel_score [B, L, nms_pre], sel_cnt [B, L] */
int rsp_rpn_topk(const RspRpnDesc* d, int32_t B, int32_t* sel_idx, float* sel_score,
                 int32_t* sel_cnt, rsp_stream_t stream);
/* decode + min-size filter -> per-image compacted candidates (level-major)    */
int rsp_rpn_decode(const RspRpnDesc* d, int32_t B, const int32_t* sel_idx, const float* sel_score,
                   const int32_t* sel_cnt, const float* img_hw, int32_t cap, float* cand_boxes,
                   float* cand_scores, int32_t* cand_ids, int32_t* cand_src, int32_t* cand_cnt,
                   rsp_stream_t stream);
/* softmax + per-class decode + score threshold -> candidates ((roi, class) order) */
int rsp_bbox_post(const float* head, int32_t ld, const float* rois, const int32_t* roi_start,
                  const float* img_hw, int32_t B, int32_t num_classes, float score_thr,
                  const RspBoxCoder* coder /*host*/, int32_t cap, float* cand_boxes,
                  float* cand_scores, int32_t* cand_ids, int32_t* cand_src, int32_t* cand_cnt,
                  rsp_stream_t stream);
/* cap <= RSP_NMS_MAX_CANDIDATES per image; up to RSP_NMS_LDS_CANDIDATES they are sorted in LDS (128 KB), above that in */
/* memory (same block, same network), which the workspace then has to hold.                                             */
#define RSP_NMS_LDS_CANDIDATES 16384
#define RSP_NMS_MAX_CANDIDATES 131072
int64_t rsp_nms_workspace_bytes(int32_t B, int32_t cap);
/* greedy NMS per image with per-id coordinate offsets; outputs [B, max_out(,4)] */
int rsp_batched_nms(const float* boxes, const float* scores, const int32_t* ids, const int32_t* src,
                    const int32_t* cnt, int32_t B, int32_t cap, float iou_thr, int32_t max_out,
                    void* workspace, int32_t* keep, int32_t* keep_cnt, float* out_boxes,
                    float* out_scores, int32_t* out_ids, int32_t* out_src, rsp_stream_t stream);

/* Glue of the folded token -> image attention below (round 6: torch index_put / gather before).  expand: tq [R*T, 128]    */
/* (q_proj output, head h at columns 16 h ..; HF:243-262 "_separate_heads") -> fp16 planes of the block-diagonal matrix      */
/* [R*96, 128]: row r*96 + h*T + t = scale * tq[r, t, head h] in columns 16 h .. 16 h + 15, zeros elsewhere; rows of the    */
/* columns >= 8 T zero.  gather: full [R*96, 128] -> ao [R*T, 128], ao[r*T + t, 16 h + d] = full[r*96 + h*T + t, 16 h + d]    */
/* (HF:264-268 "_recombine_heads" of the columns' own heads).  T <= RSP_SAM_T2I_FOLD_MAX_TOKENS: 8 heads x T query columns   */
/* fit the 96 of a RoI.                                                                                                     */
#define RSP_SAM_T2I_FOLD_MAX_TOKENS 12
int rsp_sam_fold_expand(const float* tq, uint16_t* out_hi, uint16_t* out_lo, int32_t out_scale_log2, int32_t R, int32_t T,
                        float scale, rsp_stream_t stream);
int rsp_sam_fold_gather(const float* full, float* ao, int32_t R, int32_t T, rsp_stream_t stream);

/* Token -> image attention of the SAM two-way transformer with the K | V projections of the PER-RoI keys folded in   */
/* (HF:326-331, 397-400; csrc/t2i_fold.hip): keys = fp16 planes of [k_rows >= R*N, 256]; pek = planes of k_proj(pe),      */
/* bias left out, [N, 128] (q . bias is constant over the keys: the softmax cancels it); qp = planes of q' [q_rows >= R*96, 256] with q'[r*96 + h*T + t] = Wk_h^T tq[r, t, h] (softmax scale     */
/* inside); tqx = planes of the block-diagonal tq [q_rows, 128]; *_e = plane scale exponents.  u [R*96, 256] fp32 receives */
/* sum_n softmax(score)[n] * keys[n] per column (rows of columns >= ncols = 8 T <= 8 RSP_SAM_T2I_FOLD_MAX_TOKENS stay       */
/* untouched); the caller applies                                                                                          */
/* v_proj to it.  N % 32 == 0.                                                                                           */
int rsp_sam_t2i_fold(const uint16_t* keys_hi, const uint16_t* keys_lo, int64_t k_rows, int32_t keys_e,
                     const uint16_t* pek_hi, const uint16_t* pek_lo, int32_t pek_e, const uint16_t* qp_hi,
                     const uint16_t* qp_lo, int32_t qp_e, const uint16_t* tqx_hi, const uint16_t* tqx_lo,
                     int32_t tqx_e, int64_t q_rows, float* u, int32_t R, int32_t N, int32_t ncols,
                     rsp_stream_t stream);

/* The upscaler tail of the SAM mask decoder in one pass over the per-RoI keys (HF:513-531; csrc/upscale.hip,          */
/* sam_upscale_fused_kernel): ConvTranspose2d(256 -> 64, k2 s2) + LayerNorm2d(64) + GELU + ConvTranspose2d(64 -> 32) + GELU */
/* + <., hyper_in>.  x: planes of [x_rows >= rows, 256] (rows = R*h*w, rows_per_roi = h*w, W = w); w1: planes of the packed  */
/* weight [(dy, dx, co), 256], bias1 [256] (tiled x4); w2: planes of [(dy2, dx2, c2), 64] with its K columns in the order    */
/* k' = 16 s + 8 hh + j <- channel 32 (s >> 1) + 8 ((8 (s & 1) + j) >> 2) + 4 hh + (j & 3), bias2 [128]; out [R, 4h, 4w].   */
int rsp_sam_upscale_fused(const uint16_t* x_hi, const uint16_t* x_lo, int64_t x_rows, int32_t x_scale_log2,
                          const uint16_t* w1_hi, const uint16_t* w1_lo, int32_t w1_scale_log2, const float* bias1,
                          const float* gamma, const float* beta, float eps, const uint16_t* w2_hi,
                          const uint16_t* w2_lo, int32_t w2_scale_log2, const float* bias2, const float* hyper,
                          float* out, int64_t rows, int32_t rows_per_roi, int32_t W, rsp_stream_t stream);

/* SAM-HQ's mask branch in one kernel (HF transformers models/sam_hq/modeling_sam_hq.py:1007-1037; csrc/sam_hq.hip):          */
/*   out[r, p] = < hyper[r], mask_conv2(GELU(LN2d_64(mask_conv1(U_r))))[p] + feat[feat_map[r], p] >,                            */
/*   U_r = GELU(ConvTranspose2d(64 -> 32, k2 s2)(up_r)),  both convolutions 3 x 3 with zero padding 1.                         */
/* up: planes of [up_rows >= n_up (2g)^2, 64], the [n_up, 2g, 2g, 64] upscaler planes; U_r is formed from block up_map[r]    */
/* (int32 [R], clamped to [0, n_up); null: block r, n_up == R).  w2: planes of the packed upscale_conv2 weight                */
/* [(dy, dx, c2), 64], bias2 [128] (tiled x4); w1: planes of mask_conv1 as [64, (tap = 3 ky + kx, ci) = 288], bias1 [64];     */
/* gamma / beta / eps: mask_norm; wf: mask_conv2 as fp32 [tap][ci = 64][c = 32], biasf [32]; hyper [R, 32]; feat              */
/* [n_feat, 4g, 4g, 32] fp32 with feat_map int32 [R] (clamped to [0, n_feat)); out fp32 [R, 4g, 4g].  Optionally SAM's own    */
/* masks from the same U tile (HF:1032, 1065): hyper_sam [R, n_sam <= 3, 32] -> out_sam[r, t] = < hyper_sam[r, t], U_r > +    */
/* out[r], fp32 [R, n_sam, 4g, 4g] (both null with n_sam == 0).  Nothing else is written.  mask_conv2 and the hyper product   */
/* are folded into one 3 x 3 filter per prompt set (another summation order than HF's).                                       */
/* RSP_EINVAL: a null pointer, g % 4 != 0, R (4g)^2 >= 2^31, up_rows < n_up (2g)^2, n_sam outside 0..3.                       */
int rsp_sam_hq_mask(const uint16_t* up_hi, const uint16_t* up_lo, int64_t up_rows, int32_t up_scale_log2,
                    const int32_t* up_map, int32_t n_up,
                    const uint16_t* w2_hi, const uint16_t* w2_lo, int32_t w2_scale_log2, const float* bias2,
                    const uint16_t* w1_hi, const uint16_t* w1_lo, int32_t w1_scale_log2, const float* bias1,
                    const float* gamma, const float* beta, float eps, const float* wf, const float* biasf,
                    const float* hyper, const float* feat, const int32_t* feat_map, int32_t n_feat, float* out,
                    const float* hyper_sam, float* out_sam, int32_t n_sam, int32_t R, int32_t g, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* SAM decoder tail / mask post-process                                        */
/* ------------------------------------------------------------------------ */
/* out[r, pix] = sum_c up[r, pix, c] * hyper[r, c]     (HF:523-531)             */
/* Evaluation hand-off: COCO RLE counts of k bool masks [k,H,W] (row-major bytes), i.e. the run      */
/* lengths of the column-major pixel stream, first run = zeros (pycocotools.mask.encode as used by                   */
/* encode_mask_results, mmdet/structures/mask/utils.py:38-53).  counts [k, cap] uint32, n_counts[k] = number of runs */
/* or -(needed) when cap is too small; workspace: k*cap uint32.  W <= RSP_RLE_MAX_WIDTH (a column counter per x in   */
/* LDS).                                                                                                             */
#define RSP_RLE_MAX_WIDTH 8192
int rsp_mask_rle(const uint8_t* masks, int32_t k, int32_t H, int32_t W, void* workspace, uint32_t* counts,
                 int32_t* n_counts, int32_t cap, rsp_stream_t stream);
/* ... and their compression to COCO's ASCII strings (cocoapi maskApi.c rleToString: what encode_mask_results returns   */
/* as `counts`, structures/mask/utils.py:38-53; consumed by CocoMetric.process, coco_metric.py:346-391): for the k      */
/* instances of `counts` [k, cap] / n_counts [k] (as written by rsp_mask_rle; n_counts <= 0 gives an empty string)      */
/* lens[m] = bytes of string m, offs [k + 1] = exclusive scan of lens, flat[offs[m] .. offs[m + 1]) = string m.          */
/* Strings that would end beyond flat_cap are not written: the caller compares offs[k] with flat_cap.                    */
int rsp_rle_to_string(const uint32_t* counts, const int32_t* n_counts, int32_t k, int32_t cap, int32_t* lens,
                      int64_t* offs, uint8_t* flat, int64_t flat_cap, rsp_stream_t stream);
/* SAM upscaler tail, streaming form (HF:521-531): rows = R*H2*W2 input pixels as fp16 planes (KB32, K = 64),      */
/* weight planes [2][128][32] with rows (dy, dx, c) of ConvTranspose2d(64 -> 32, k2, s2), bias tiled x4 [128],       */
/* hyper [R, 32]; out [R, 2*H2, 2*W2] = sum_c GELU(convT)[.., c] * hyper[r, c].  rows_per_roi = H2*W2, ct_W = W2.    */
int rsp_sam_upscale2(const uint16_t* a_hi, const uint16_t* a_lo, int64_t rows, int32_t a_scale_log2,
                     const uint16_t* w_hi, const uint16_t* w_lo, int32_t w_scale_log2, const float* bias,
                     const float* hyper, float* out, int32_t rows_per_roi, int32_t ct_W, rsp_stream_t stream);
int rsp_hyper_mask(const float* up, const float* hyper, float* out, int32_t R, int32_t npix,
                   int32_t C, rsp_stream_t stream);
/* models.py:1746-1784: sigmoid, bilinear (h,w)->(Hb,Wb), crop (crop_h,crop_w),  */
/* bilinear -> (out_h,out_w), >= thr.  out_prob optional.  sig_ws: [k*h*w] scratch  */
/* (sigmoid of the logits, computed once instead of per output tap).               */
int rsp_mask_post(const float* low_res, float* sig_ws, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb,
                  int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w, float thr,
                  uint8_t* out_mask, float* out_prob, rsp_stream_t stream);
/* SAMDet.predict (models.py:1185-1206): the same resize -> crop -> resize chain on the raw low-res logits */
/* [k, h, w] of the SAM decoder, then `> thr` (strict; the reference uses 0).  out_val optional.           */
int rsp_mask_post_logits(const float* low_res, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb,
                         int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w, float thr,
                         uint8_t* out_mask, float* out_val, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* SAMDet (models.py:1061-1215): FasterRCNN R50-FPN detector + SAM box prompts  */
/* ------------------------------------------------------------------------ */
/* ResNet stem (mmdet/models/backbones/resnet.py:640-647): conv1 7x7 s2 p3 (3 -> 64) + eval-mode bn1 folded   */
/* into w / bias + ReLU.  x [B,3,H,W] fp32 NCHW, w [147][64] (tap = (c*7 + ky)*7 + kx), y [B,Ho,Wo,64] NHWC.  */
int rsp_resnet_stem(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t H, int32_t W,
                    rsp_stream_t stream);
/* nn.MaxPool2d(k, stride s, padding p) on channels-last data (resnet.py:598: k3 s2 p1); C % 4 == 0          */
int rsp_maxpool_nhwc(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s,
                     int32_t p, rsp_stream_t stream);
/* FPN top-down step (mmdet/models/necks/fpn.py:190-204): dst [B,H,W,C] += nearest-upsampled src [B,h,w,C]   */
int rsp_upsample_nearest_add(const float* src, float* dst, int32_t B, int32_t h, int32_t w, int32_t H, int32_t W,
                             int32_t C, rsp_stream_t stream);
/* HF SamPromptEncoder._embed_boxes (transformers 4.38.1 modeling_sam.py:647-656): boxes [n,4] (x1,y1,x2,y2 in  */
/* input pixels) -> sparse prompt embeddings out [n, 2, 2*num_pos_feats]; gauss [2, num_pos_feats] is the shared */
/* positional_embedding, pe_top_left / pe_bottom_right are point_embed[2] / point_embed[3] [2*num_pos_feats].    */
int rsp_sam_embed_boxes(const float* boxes, const float* gauss, const float* pe_top_left,
                        const float* pe_bottom_right, float* out, int32_t n, int32_t num_pos_feats,
                        int32_t input_h, int32_t input_w, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Query prompter (RSMask2FormerHead + MSDeformAttnPixelDecoder + fusion head)  */
/* ------------------------------------------------------------------------ */
/* GroupNorm(G) on a channels-last map x [B, HW, C] (+ReLU, + optional `add` after the norm):          */
/* mmcv ConvModule(norm_cfg=GN) of msdeformattn_pixel_decoder.py:73-111.  stats_ws: 2*B*G doubles.       */
int rsp_groupnorm_nhwc(const float* x, const float* gamma, const float* beta, const float* add, float* y,
                       double* stats_ws, int32_t B, int32_t HW, int32_t C, int32_t G, float eps,
                       int32_t relu, rsp_stream_t stream);
/* F.interpolate(bilinear, align_corners=False) on channels-last data                                    */
int rsp_resize_bilinear_nhwc(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                             int32_t C, rsp_stream_t stream);
/* mmcv MultiScaleDeformableAttention core (8 heads x 16, 3 levels, 4 points): value [B,Ntok,128];         */
/* offs_weights [B,Ntok,ld]: 192 offsets (h,l,p,xy) then 96 attention logits (h,l*p); ref [Ntok,2];         */
/* level_hw: HOST int32 [L,2] (h, w), levels concatenated along Ntok.  out [B,Ntok,128] (pre output_proj).   */
int rsp_msdeform_attn(const float* value, const float* offs_weights, int32_t ld_ow, const float* ref_points,
                      float* out, int32_t B, int32_t Ntok, int32_t num_levels, const int32_t* level_hw,
                      rsp_stream_t stream);
/* the same with head_dim 16 | 32 (value / out rows of 8*head_dim): head_dim 32 is the embed_dims=256 pixel decoder of  */
/* the standard Mask2FormerHead (configs/rsprompter/_base_/samseg-mask2former.py:101-118)                             */
int rsp_msdeform_attn_ex(const float* value, const float* offs_weights, int32_t ld_ow, const float* ref_points,
                         float* out, int32_t B, int32_t Ntok, int32_t num_levels, const int32_t* level_hw,
                         int32_t head_dim, rsp_stream_t stream);
/* mask[row, k] = sigmoid(bilinear(mask_pred_plus[row], (h,w)))[k] < 0.5, fully-blocked rows cleared        */
/* (models.py:386-391, 439-442); rows = B*Nq maps of size Hs x Ws.                                          */
int rsp_query_attn_mask(const float* mask_pred_plus, uint8_t* mask, int64_t rows, int32_t Hs, int32_t Ws,
                        int32_t h, int32_t w, rsp_stream_t stream);
/* SamMaskEmbedding (HF:584-593) of mask_pred_plus [R, 4he, 4we] fused with `image_embeddings + dense`      */
/* (HF:499): out [R, he*we, C] = emb[roi_img[r]] + conv3(gelu(ln(conv2(gelu(ln(conv1(m)))))))               */
typedef struct RspMaskEmbedDesc {
  const float* mask_pred_plus; const float* image_embeddings; const int32_t* roi_img;
  const float *conv1_w, *conv1_b, *ln1_w, *ln1_b, *conv2_w, *conv2_b, *ln2_w, *ln2_b, *conv3_w, *conv3_b;
  float* out;
  int32_t R, he, we, C;
  float eps;
} RspMaskEmbedDesc;
int rsp_sam_mask_embed(const RspMaskEmbedDesc* d, rsp_stream_t stream);   /* C % 256 == 0, else RSP_EINVAL */
/* maskformer_fusion_head.py:149-162: softmax(cls)[:, :-1], top-k over Nq*nc, (score desc, index asc)        */
int rsp_query_topk(const float* cls, int32_t B, int32_t Nq, int32_t nc, int32_t k, float* out_score,
                   int32_t* out_flat, rsp_stream_t stream);
/* models.py:652-656,684-695 + maskformer_fusion_head.py:164-176 + mask2bbox: per selected instance,         */
/* bilinear logits -> (Hb,Wb) -> crop -> (out_h,out_w); mask = logit > 0; det_score = cls_score * mean        */
/* sigmoid over the mask; bbox = mask extents.  stats_ws: k * 32 bytes.                                       */
int rsp_query_mask_post(const float* low_res, const int32_t* qidx, const float* cls_score, int32_t k, int32_t h,
                        int32_t w, int32_t Hb, int32_t Wb, int32_t crop_h, int32_t crop_w, int32_t out_h,
                        int32_t out_w, void* stats_ws, uint8_t* out_mask, float* out_logits, float* det_score,
                        float* bboxes, rsp_stream_t stream);
/* maskformer_fusion_head.py:41-106 (panoptic_postprocess) behind models.py:698-701 / maskformer_fusion_head.py:253-256   */
/* (csrc/panoptic_fuse.hip), one image: cls [Nq, nc + 1] class logits, low_res [Nq, h, w]; the geometry is      */
/* rsp_query_mask_post's.  score, label = softmax(cls).max(-1) (lowest class on a tie); kept = label != nc && score >      */
/* object_mask_thr, in query order; per output pixel the kept query with the largest score * sigmoid(field) wins (lowest    */
/* kept index on a tie); mask_area = pixels won, original_area = pixels with sigmoid(field) >= 0.5; a kept query paints its  */
/* pixels (with filter_low_score: those whose sigmoid >= 0.5) unless an area is 0 or (double)mask_area / original_area <     */
/* iou_thr; a stuff class (label >= num_things) paints label, a thing label + 1000 * instance id, ids from 1 in kept order   */
/* over the things that paint; every other pixel is nc.  Writes sem_seg int32 [out_h, out_w] and, per query [Nq]: segment    */
/* (the id painted, -1: none), mask_area, original_area (0 for a query not kept), score fp32.  Nothing is read by the host:  */
/* the kept count stays on the device, so the limit is on Nq.  RSP_EINVAL: Nq > RSP_PANOPTIC_MAX_QUERIES (the bins of the    */
/* kernel's LDS histograms), an invalid geometry, num_things > nc.  workspace: rsp_panoptic_workspace_bytes() bytes, 16-byte */
/* aligned.  Integer atomics only: bit-reproducible.                                                                        */
#define RSP_PANOPTIC_MAX_QUERIES 1024
int64_t rsp_panoptic_workspace_bytes(void);
int rsp_panoptic_fuse(const float* cls, const float* low_res, int32_t Nq, int32_t nc, int32_t num_things, int32_t h,
                      int32_t w, int32_t Hb, int32_t Wb, int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w,
                      float object_mask_thr, double iou_thr, int32_t filter_low_score, void* workspace, int32_t* sem_seg,
                      int32_t* segment, int32_t* mask_area, int32_t* original_area, float* score, rsp_stream_t stream);
/* Panoptic quality of one image: pq_compute_single_core (mmdet/evaluation/functional/panoptic_utils.py:60-169) on the maps as  */
/* CocoPanopticMetric hands them over (coco_panoptic_metric.py:270-297, :309-387), csrc/panoptic_quality.hip, DESIGN 16.1.       */
/* pred int32 [H, W]: id = label + 1000 * instance; a pixel is void when id % 1000 is num_classes or ignore_index.  The ground   */
/* truth is EITHER gt_rgb uint8 [H, W, 3] (id = R + 256 G + 65536 B) OR gt_map int32 [H, W]; the other pointer is null.          */
/* tables (device int32, written by the host): gt id ascending [G] | category index [G] | iscrowd [G] | area [G] (negative:     */
/* count the pixels) | category index of label 0..999 [1000] (-1: none) | crowd_of [n_cat] = the slot, in the ascending order,   */
/* of the LAST crowd segment of the category in JSON order (-1: none).  Listed gt ids are distinct and positive.  The predicted  */
/* segments are the distinct non-void ids ascending (np.unique); TP: iou = inter / (area_pred + area_gt - inter - void overlap)  */
/* as one double division, iou > 0.5; FN: every unmatched non-crowd gt segment; FP: an unmatched predicted segment unless        */
/* 2 * (void overlap + crowd overlap) > area_pred (the integer form of the reference's `> 0.5`).  Writes per category [n_cat]:   */
/* tp, fp, fn int32 and iou_sum double (summed in ascending gt id), status (0, or RSP_PQ_STATUS_* bits: the row is then zero),   */
/* n_pred = P and, [RSP_PQ_MAX_SEGMENTS] each, the predicted ids, their category indices and areas (-1, -1, 0 beyond P).  Five   */
/* launches, nothing read by the host; integer atomics only: bit-reproducible.  RSP_EINVAL: H * W >= 2^31, G >                   */
/* RSP_PQ_MAX_SEGMENTS, n_cat > RSP_PQ_MAX_CATEGORIES, both or neither gt pointer, a null pointer, a map or the workspace not    */
/* 16-byte aligned.  workspace: rsp_pq_workspace_bytes(G) bytes (-1 for a G the call would refuse).                              */
#define RSP_PQ_MAX_SEGMENTS 1024
#define RSP_PQ_MAX_PRED_ID (1 << 21)
#define RSP_PQ_MAX_CATEGORIES 1024
#define RSP_PQ_STATUS_TOO_MANY_SEGMENTS 1   /* more than RSP_PQ_MAX_SEGMENTS distinct predicted ids                      */
#define RSP_PQ_STATUS_PRED_ID_RANGE 2       /* a predicted id below 0 or at / above RSP_PQ_MAX_PRED_ID                   */
#define RSP_PQ_STATUS_PRED_ID_ZERO 4        /* predicted id 0 that is not void: it collides with VOID in the PNG encoding */
#define RSP_PQ_STATUS_PRED_CATEGORY 8       /* a predicted label without a category (the reference raises KeyError)      */
#define RSP_PQ_STATUS_GT_AREA 16            /* a listed non-crowd gt area below the segment's pixels in the map: a union  */
                                            /* can then be 0 and one segment can match twice                             */
int64_t rsp_pq_workspace_bytes(int32_t G);
int rsp_pq_image(const int32_t* pred, const uint8_t* gt_rgb, const int32_t* gt_map, int32_t H, int32_t W,
                 int32_t num_classes, int32_t ignore_index, const int32_t* tables, int32_t G, int32_t n_cat, void* workspace,
                 int32_t* tp, int32_t* fp, int32_t* fn, double* iou_sum, int32_t* status, int32_t* n_pred,
                 int32_t* pred_ids, int32_t* pred_cat, int32_t* pred_area, rsp_stream_t stream);
/* PQStat.__iadd__ over n_img rows in order (coco_panoptic_metric.py:529-531): tp, fp, fn int32 [n_img, n_cat], iou_sum double  */
/* [n_img, n_cat], status int32 [n_img] -> out int64 [4 n_cat + n_img]: the sums of tp | fp | fn | the bits of the double sum   */
/* ((0 + s1) + s2) + ... | the statuses, so one read serves compute_metrics.                                                     */
int rsp_pq_reduce(const int32_t* tp, const int32_t* fp, const int32_t* fn, const double* iou_sum, const int32_t* status,
                  int32_t n_img, int32_t n_cat, int64_t* out, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Data movement                                                              */
/* ------------------------------------------------------------------------ */
/* DetDataPreprocessor.forward (data_preprocessor.py:110-149 + mmengine       */
/* ImgDataPreprocessor): BGR->RGB, (x-mean)/std, pad bottom/right.  src is    */
/* one CHW image (uint8 or fp32), dst one [3, Hp, Wp] slice of the batch.     */
/* mean3/std3 are HOST pointers.                                              */
int rsp_preprocess(const void* src, int32_t src_is_u8, float* dst, int32_t H, int32_t W,
                   int32_t Hp, int32_t Wp, const float* mean3, const float* std3,
                   int32_t swap_rb, float pad_value, rsp_stream_t stream);

/* FCNMaskHead._predict_by_feat_single + _do_paste_mask (fcn_mask_head.py:276-480; the mask post-process of the       */
/* SAMSegMaskRCNN sibling model, models.py:1219-1244): logits [k, Hm, Wm, C] NHWC, labels [k] (NULL / C == 1: class   */
/* agnostic), boxes [k, 4] in output-image coordinates -> out bool [k, img_h, img_w] (sigmoid, bilinear paste, >= thr). */
/* thr < 0 (:390-394): out holds the pasted probabilities as uint8, (p * 255) truncated.                               */
int rsp_paste_masks(const float* logits, const int32_t* labels, const float* boxes, int32_t k, int32_t Hm, int32_t Wm,
                    int32_t C, int32_t img_h, int32_t img_w, float thr, uint8_t* out, rsp_stream_t stream);

/* Test-pipeline front end: `Resize(scale, keep_ratio=True)` + `Pad(size, pad_val)`                       */
/* (configs/rsprompter/_base_/rsprompter_anchor.py:231-241; mmdet/datasets/transforms/transforms.py:134-247 */
/* and :704-786 over mmcv.imrescale / cv2.resize INTER_LINEAR and mmcv.impad), optionally fused with the     */
/* DetDataPreprocessor arithmetic (data_preprocessor.py:110-149).  src: one decoded HWC image (uint8 or      */
/* fp32, 3 interleaved channels); dst: [3, Hp, Wp] fp32; (Hn, Wn) = resized size inside the padded canvas.   */
/* pad3 / mean3 / std3 are HOST pointers.                                                                    */
int rsp_resize_pad(const void* src, int32_t src_is_u8, float* dst, int32_t H, int32_t W, int32_t Hn, int32_t Wn,
                   int32_t Hp, int32_t Wp, const float* pad3, int32_t normalise, int32_t swap_rb,
                   const float* mean3, const float* std3, rsp_stream_t stream);

/* im2col of the 16x16/s16 patch-embedding conv (HF:116-128): NCHW image ->   */
/* [B*gh*gw, C*p*p] rows, k = (c, ky, kx) (the conv weight's own flattening). */
int rsp_patchify(const float* img, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                 int32_t patch, rsp_stream_t stream);
/* NHWC pooling: mode 0 = MaxPool2d(2,2) (models.py:1307), mode 1 = max_pool2d(k=1,s=2) (:1362) */
int rsp_pool2(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t mode,
              rsp_stream_t stream);
/* y[r,:] = x[r,:] + v[r % vmod, :] */
int rsp_add_rows(const float* x, const float* v, float* y, int64_t rows, int32_t C, int32_t vmod,
                 rsp_stream_t stream);
/* y[i] = sin(x[2i]) + x[2i+1]  (models.py:1672) */
int rsp_sincos_pairs(const float* x, float* y, int64_t n_out, rsp_stream_t stream);
/* out[i, j] = boxes[i, j] / sf4[j]   (bboxes /= scale_factor, models.py:1763-1764); sf4 is a HOST pointer */
int rsp_div_boxes(const float* boxes, float* out, int64_t n, const float* sf4, rsp_stream_t stream);
/* Rows of a GEMM output that the GEMM does not write because their A row is zero (window padding of window_partition,  */
/* HF:913-915: qkv(0) = bias): C[rows[i], 0:c_ncols) = bias and the planes of columns [pl_col0, N) (KB32, c_rows rows,    */
/* format word c_scale_log2 as in RspGemmDesc) = split(bias * 2^e) -- what the GEMM epilogue writes for alpha*0 + bias.    */
int rsp_fill_bias_rows(const float* bias, const int32_t* rows, int32_t n_rows, int32_t N, float* C, int32_t ldc,
                       int32_t c_ncols, uint16_t* Chi, uint16_t* Clo, int64_t c_rows, int32_t pl_col0,
                       int32_t c_scale_log2, rsp_stream_t stream);
/* scale_boxes (structures/bbox/transforms.py:391-414): out = boxes * (f0, f1, f2, f3); the R-CNN head's rescale   */
/* multiplies by fp32(1 / scale_factor) (bbox_head.py:549-552).  f4: HOST float[4].  In place allowed.               */
int rsp_scale_boxes(const float* boxes, float* out, int64_t n, const float* f4 /*host*/, rsp_stream_t stream);
/* bool bytes -> bits (little-endian in a byte) : the payload of the multi-GPU result all-gather,  */
/* replacing CocoMetric's per-rank RLE + mmengine collect_results (coco_metric.py:356-391).       */
int rsp_pack_bits(const uint8_t* src, uint8_t* dst, int64_t n_bits, rsp_stream_t stream);
/* dst[i,:] = src[idx[i],:] (idx<0 -> 0) */
int rsp_gather_rows(const float* src, const int32_t* idx, float* dst, int64_t rows, int32_t C,
                    rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* COCO evaluation (csrc/cocoeval.hip): the device part of       */
/* pycocotools COCOeval.evaluate as CocoMetric uses it                       */
/* ------------------------------------------------------------------------ */
#define RSP_COCO_IOU_BBOX 0
#define RSP_COCO_IOU_SEGM 1
/* One evaluation unit = one (image, category): its dts are [dt0, dt0 + nd) of the per-dt arrays (score-sorted,      */
/* truncated to maxDets[-1]), its gts [gt0, gt0 + ng) of the per-gt arrays (gt ranges of different units disjoint),    */
/* its IoU block iou[out0 + d * ng + g]; nwords = 64-bit words of one of its masks (segm).                            */
typedef struct {
  int64_t dt0, gt0, out0;
  int32_t nd, ng, nwords, pad;
} RspCocoUnit;
/* cocoapi maskApi.c rleFrString: string i = flat[offs[i] .. offs[i + 1]) (what rsp_rle_to_string writes) -> run      */
/* counts counts[i, 0 .. n_counts[i]) (uint32, row stride cap); n_counts[i] = -(needed) when cap is too small.        */
int rsp_rle_from_string(const uint8_t* flat, const int64_t* offs, int32_t k, int32_t cap, uint32_t* counts,
                        int32_t* n_counts, rsp_stream_t stream);
/* run counts -> bits: pixel j of the column-major RLE stream of mask i is bit (j & 63) of bits[word_offs[i] + (j >> 6)]  */
/* (word_offs [k + 1]); area[i] = sum of the odd runs (maskApi rleArea); wrange[2i .. 2i + 1] = words [lo, hi) that hold  */
/* every set bit ([0, 0) when empty; may be NULL).                                                                      */
int rsp_rle_to_bits(const uint32_t* counts, const int32_t* n_counts, int32_t k, int32_t cap, const int64_t* word_offs,
                    uint64_t* bits, int64_t* area, int32_t* wrange, rsp_stream_t stream);
/* IoU blocks of n_units units (units: DEVICE array).  SEGM: inter = popcount(d & g), union = area_d + area_g - inter   */
/* (area_d for a crowd gt), 0 when inter == 0, else (double)inter / union (maskApi rleIou).  BBOX: maskApi bbIou in fp64 */
/* on xywh boxes dt_box [n_dt, 4], gt_box [n_gt, 4].  Arrays of the other mode may be NULL.                             */
int rsp_coco_iou(const RspCocoUnit* units, int32_t n_units, int32_t mode, const uint64_t* dt_bits, const uint64_t* gt_bits,
                 const int64_t* dt_woff, const int64_t* gt_woff, const int32_t* dt_wrange, const int32_t* gt_wrange,
                 const int64_t* dt_area, const int64_t* gt_area, const double* dt_box, const double* gt_box,
                 const uint8_t* gt_crowd, double* iou, rsp_stream_t stream);
/* cocoeval.py evaluateImg for every unit x area range (area_rng [A][2], inclusive, A <= 8) x threshold (thrs [T], fp64 */
/* as the metric holds them).  gt ignore = crowd or area outside the range; dtm [A*T, n_dt] = id of the matched gt (0:    */
/* none), dtig [A*T, n_dt] as evaluateImg's dtIgnore, npig [n_units, A] = gts not ignored.  gtm_ws: n_gt * A * T bytes.  */
int rsp_coco_match(const RspCocoUnit* units, int32_t n_units, const double* iou, const double* gt_area,
                   const uint8_t* gt_crowd, const int64_t* gt_id, const double* dt_area, const double* area_rng, int32_t A,
                   const double* thrs, int32_t T, int64_t n_dt, uint8_t* gtm_ws, int64_t* dtm, uint8_t* dtig,
                   int32_t* npig, rsp_stream_t stream);
/* The same IoU blocks from RUN TABLES (csrc/coco_iou_runs.hip), for masks too large to exist as bits.    */
/* A run table is counts [k, cap] / n [k] as rsp_rle_from_string writes it (n <= 0: an empty row, n > cap: read up to     */
/* cap); no canvas size is taken anywhere, a row is its column-major stream; the counts need not be canonical (zero       */
/* counts anywhere).  rsp_run_prefix: per row the prefix workspace (int32 [k, cap], rsp_run_prefix_workspace_bytes: ones   */
/* pixels in front of each ones-run and the run's pixel start), area [k] = sum of the odd counts (maskApi rleArea) and    */
/* extent [k, 2] = (first set pixel, one past the last set pixel) of the stream, (0, 0) for a row without one.            */
int64_t rsp_run_prefix_workspace_bytes(int32_t k, int32_t cap);
int rsp_run_prefix(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, void* workspace, int64_t* area,
                   int32_t* extent, rsp_stream_t stream);
/* Filter: for every slot p of iou [0, n_iou) -- units as rsp_coco_iou takes them (DEVICE array, nwords ignored), ascending */
/* in out0 and tiling [0, n_iou) --: alive[p] = dt row << 32 | gt row when the extents of its pair overlap, else -1 and    */
/* iou[p] = 0.0 (disjoint or touching extents share no pixel: the exact stand-in of rleIou's bbIou prefilter).  No run is   */
/* read.  The caller compacts the alive slot numbers (slots int64 [n_slots], any order) and hands them to                  */
/* rsp_coco_iou_runs: one wave per slot walks the ones-runs of the row that has fewer of them inside the overlap of the     */
/* extents and looks their ends up in the other row's prefix; iou[p] = rsp_coco_iou's SEGM arithmetic (union in 64 bits).  */
/* Every slot of iou is written once, by one of the two; dt and gt are two tables with capacities of their own.            */
int rsp_coco_iou_runs_filter(const RspCocoUnit* units, int32_t n_units, int64_t n_iou, const int32_t* dt_extent,
                             int64_t n_dt, const int32_t* gt_extent, int64_t n_gt, int64_t* alive, double* iou,
                             rsp_stream_t stream);
int rsp_coco_iou_runs(const int64_t* slots, int64_t n_slots, int64_t n_iou, const int64_t* alive,
                      const uint32_t* dt_counts, const int32_t* dt_n, int64_t n_dt, int32_t dt_cap,
                      const void* dt_workspace, const int64_t* dt_area, const int32_t* dt_extent,
                      const uint32_t* gt_counts, const int32_t* gt_n, int64_t n_gt, int32_t gt_cap,
                      const void* gt_workspace, const int64_t* gt_area, const int32_t* gt_extent,
                      const uint8_t* gt_crowd, double* iou, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Sliced inference on large scenes (csrc/large_image.hip)        */
/* ------------------------------------------------------------------------ */
/* Tile front end: replaces sahi.slicing.slice_image (host crops, demo/large_image_demo.py:133-141) followed by the     */
/* test pipeline's Resize + Pad per patch (:146-160 -> inference_detector).  scene: the decoded image [SH, SW, 3]       */
/* (uint8 or fp32) on the device; origins: DEVICE int32 [B, 2] = (x0, y0) of B tiles of one size (th, tw), clamped into  */
/* the scene by the kernel; dst [B, 3, Hp, Wp] fp32.  Tile i equals rsp_resize_pad of the contiguous crop                */
/* scene[y0:y0+th, x0:x0+tw] bit for bit (one interpolation function, csrc/rsp_common.h); the remaining arguments are     */
/* rsp_resize_pad's.  th == Hn, tw == Wn on a uint8 scene is a pure convert-and-pad (16-byte accesses).  B <= 65535.     */
int rsp_slice_resize_pad(const void* scene, int32_t src_is_u8, int32_t SH, int32_t SW, const int32_t* origins,
                         int32_t B, int32_t th, int32_t tw, float* dst, int32_t Hn, int32_t Wn, int32_t Hp, int32_t Wp,
                         const float* pad3, int32_t normalise, int32_t swap_rb, const float* mean3, const float* std3,
                         rsp_stream_t stream);
/* Crop front end of SAM's multi-crop mask generation: replaces the host crop + resize per crop box of HF               */
/* image_processing_sam._generate_crop_images (`image[top:bottom, left:right]`, then `_get_preprocess_shape` + resize   */
/* + normalise + pad of every crop).  image: the decoded image [SH, SW, 3] (uint8 or fp32) on the device, uploaded once; */
/* table: DEVICE int32 [B, 6] = (x0, y0, x1, y1, Hn, Wn) per crop -- crops of DIFFERENT sizes in one launch, each        */
/* resized to its own (Hn, Wn) and padded to (Hp, Wp); the kernel clamps the box into the image and (Hn, Wn) into the    */
/* canvas.  dst [B, 3, Hp, Wp] fp32.  Crop i equals rsp_resize_pad of the contiguous crop image[y0:y1, x0:x1] bit for bit */
/* (one interpolation function, csrc/rsp_common.h); the remaining arguments are rsp_resize_pad's.  B <= 65535.          */
int rsp_crops_resize_pad(const void* image, int32_t src_is_u8, int32_t SH, int32_t SW, const int32_t* table, int32_t B,
                         float* dst, int32_t Hp, int32_t Wp, const float* pad3, int32_t normalise, int32_t swap_rb,
                         const float* mean3, const float* std3, rsp_stream_t stream);
/* Run-domain shift: replaces sahi.slicing.shift_masks (mmdet/utils/large_image.py:63-65: every instance mask padded to  */
/* the full scene as a dense array) + encode_mask_results on that array.  counts_in [k, cap_in] / n_in [k]: run counts of */
/* k masks of ONE tile size (h, w) as rsp_mask_rle writes them; offsets: DEVICE int32 [k, 2] = (ox, oy) per instance,      */
/* clamped to [0, W - w] x [0, H - h].  counts_out [k, cap_out] / n_out [k]: the COCO run counts of the same masks placed */
/* at [oy:oy+h, ox:ox+w] of a zero (H, W) canvas, same conventions: n_out = -(needed) when cap_out is too small (the row   */
/* is then undefined), n_in <= 0 gives n_out = 0.  In the column-major pixel stream: ox*H + oy zeros, the tile's stream    */
/* with H - h zeros inserted after every tile column (H - h - oy after the last), (W - ox - w)*H zeros; adjacent runs of  */
/* one value merge.  H * W >= 2^31 is refused (RSP_EINVAL): COCO's counts are 32-bit.                                     */
int rsp_rle_shift(const uint32_t* counts_in, const int32_t* n_in, int32_t k, int32_t cap_in, const int32_t* offsets,
                  int32_t h, int32_t w, int32_t H, int32_t W, uint32_t* counts_out, int32_t* n_out, int32_t cap_out,
                  rsp_stream_t stream);
/* shift_masks itself, for callers who want dense scene masks (mmdet/utils/large_image.py:27-72 shift_predictions):       */
/* out [k, H, W] bool bytes = masks [k, h, w] at offsets (DEVICE int32 [k, 2] = (ox, oy), clamped), zero elsewhere.       */
/* k <= 65535.                                                                                                           */
int rsp_paste_tiles(const uint8_t* masks, const int32_t* offsets, int32_t k, int32_t h, int32_t w, int32_t H, int32_t W,
                    uint8_t* out, rsp_stream_t stream);
/* Seam merge (csrc/seam_merge.hip): arithmetic between scene-sized masks in the run domain.  Input of all  */
/* four: counts [k, cap] / n [k] as rsp_rle_shift writes them -- COCO run counts of k masks on ONE (H, W) canvas, only    */
/* count 0 may be zero, n <= 0 = an empty row.  H * W >= 2^31 is refused (RSP_EINVAL).  Integer arithmetic, exact.        */
/* Tight box and area: replaces pycocotools maskUtils.toBbox / area on the scene-sized RLE.  boxes int32 [k, 4] =         */
/* (x0, y0, x1, y1) end-exclusive, zeros for an empty mask; area int32 [k].                                               */
int rsp_rle_bbox(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W, int32_t* boxes,
                 int32_t* area, rsp_stream_t stream);
/* Pair overlap: replaces the dense `(M_i & M_j).sum()`, `M_i[y0:y1, x0:x1].sum()`, `M_j[y0:y1, x0:x1].sum()` on masks     */
/* padded to the scene (sahi shift_masks).  pairs: DEVICE int32 [P, 2] = row indices (a row outside [0, k) counts as      */
/* empty); rects: DEVICE int32 [P, 4] = (x0, y0, x1, y1) end-exclusive, clamped into the canvas; out int32 [P, 3] =        */
/* (inter, a_i, a_j): inter is the FULL intersection, not clipped to the rectangle.  workspace: the rows' run starts and   */
/* ones prefixes, computed once per call however many pairs a row is in: rsp_rle_pair_overlap_workspace_bytes(k, cap).     */
int64_t rsp_rle_pair_overlap_workspace_bytes(int32_t k, int32_t cap);
int rsp_rle_pair_overlap(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                         const int32_t* pairs, const int32_t* rects, int32_t P, void* workspace, int32_t* out,
                         rsp_stream_t stream);
/* Union, first half: the ones-runs of M member rows as sortable intervals.  members: DEVICE int32 [M] row indices (a row  */
/* outside [0, k) has no runs), member_group int32 [M] = the group of each, member_offs int64 [M] = the first slot of       */
/* each (exclusive sum of max(min(n, cap), 0) / 2 over the members), total = all slots.  keys int64 [total] = group << 31   */
/* | pixel start, ends int32 [total] = pixel end.  The caller sorts by key (ends along) and hands them to rsp_rle_union.   */
int rsp_rle_intervals(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                      const int32_t* members, const int32_t* member_group, const int64_t* member_offs, int32_t M,
                      int64_t total, int64_t* keys, int32_t* ends, rsp_stream_t stream);
/* Union, second half: replaces the dense OR of the members' scene-sized masks + encode_mask_results.  keys / ends sorted  */
/* by key; interval_offs: DEVICE int64 [G + 1] = the intervals of group g (clamped into [0, total]).  counts_out           */
/* [G, cap_out] / n_out [G]: the canonical COCO run counts of each group's union (adjacent runs of one value merged, first  */
/* count zero iff pixel 0 is set; a group without intervals is the empty mask, one count H * W), conventions of            */
/* rsp_rle_shift: n_out = -(needed) when cap_out is too small (the row is then undefined).  A group of one valid row       */
/* reproduces that row bit for bit.                                                                                       */
int rsp_rle_union(const int64_t* keys, const int32_t* ends, int64_t total, const int64_t* interval_offs, int32_t G, int32_t H,
                  int32_t W, uint32_t* counts_out, int32_t* n_out, int32_t cap_out, rsp_stream_t stream);
/* The column-piece table of a run table (csrc/run_pieces.hip, DESIGN §14 "Its two intermediates"), which polygon export and   */
/* the run-domain components below read.  counts [k, cap] / n [k] of k masks on ONE (H, W) canvas as above (a row with n <= 0   */
/* has no pieces; n beyond cap is read up to cap); H * W >= 2^31 is refused (RSP_EINVAL).  A ones-run that crosses column ends  */
/* is one piece (x, y0, y1), y0 < y1, per column.  No call reads the host, none uses atomics.  _count: piece_cnt int32 [k];     */
/* the caller's exclusive sum is piece_offs int64 [k + 1], P = piece_offs[k] <= RSP_RUN_PIECES_MAX_PIECES (32-bit piece         */
/* indices).  rsp_run_pieces writes pieces int32 [4, P] = the planes (x, y0, y1, instance), sorted by (instance, x, y0), with   */
/* -1 as the instance of a slot that no row filled (a piece_offs that overstates a row).                                        */
#define RSP_RUN_PIECES_MAX_PIECES 0x7fffff00LL
int rsp_run_pieces_count(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                         int32_t* piece_cnt, rsp_stream_t stream);
int rsp_run_pieces(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                   const int64_t* piece_offs, int64_t P, int32_t* pieces, rsp_stream_t stream);
/* Polygon export (csrc/mask_polygons.hip): run tables -> exact rings on the pixel-corner lattice, replaces */
/* decoding every instance to a dense H x W array on the host + cv2.findContours.  Input: the piece table of k masks on    */
/* ONE (H, W) canvas, pieces / piece_offs / P as rsp_run_pieces leaves them.  H * W >= 2^31 is refused (RSP_EINVAL).  The    */
/* three calls are one pipeline after the table; the caller reads two sizes in between and sorts the rings                  */
/* (rsprompter_amd/ops.py mask_polygons).  No call reads the host, none uses atomics.                                       */
/* 1. P <= RSP_MASK_POLYGON_MAX_PIECES (six edge slots per column piece, 32-bit slot numbers), E = 6 P: ekey int64 [E] =     */
/* start x * (H + 1) + start y of the directed boundary edge in the slot, INT64_MAX for an empty slot; eoth int32 [E] = the  */
/* end vertex's other coordinate; succ int32 [E] = the slot of the next edge of the ring (saddles: foreground 8-connected). */
#define RSP_MASK_POLYGON_MAX_PIECES (0x7fffffffLL / 6)
int rsp_mask_polygon_edges(int32_t k, int32_t H, int32_t W, const int64_t* piece_offs, int64_t P, const int32_t* pieces,
                           int64_t* ekey, int32_t* eoth, int32_t* succ, rsp_stream_t stream);
/* 2. list ranking by pointer jumping, `rounds` launches per pass with 2^rounds >= the edges of the longest ring (6 x the   */
/* largest piece_cnt bounds it).  ring_key int64 [E]: the smallest ekey of the edge's ring = its first vertex; flags uint8  */
/* [E]: bit 0 the edge is its ring's first, bit 1 its start vertex is a corner; lastof int32 [E]: for a first edge the      */
/* ring's last edge; corners int32 [E] / area2 int64 [E]: the corners and the doubled signed area (positive = clockwise on   */
/* screen = outer ring) from the ring's first edge up to and including this one.  workspace:                              */
/* rsp_mask_polygon_rank_workspace_bytes(P).                                                                            */
int64_t rsp_mask_polygon_rank_workspace_bytes(int64_t P);
int rsp_mask_polygon_rank(int64_t P, int32_t H, int32_t rounds, const int64_t* ekey, const int32_t* eoth, const int32_t* succ,
                          void* workspace, int64_t* ring_key, uint8_t* flags, int32_t* lastof, int32_t* corners, int64_t* area2,
                          rsp_stream_t stream);
/* 3. ring_keys int64 [R] = instance << 33 | ring_key of the R rings, ascending; ring_offs int64 [R + 1] their vertex       */
/* offsets, V = ring_offs[R]; ring_area2 int64 [R]; inst_ring_offs int64 [k + 1].  Writes verts int32 [V, 2] = (x, y), the   */
/* corners of every ring from its smallest vertex on, and ring_parent int32 [R]: -1 for an outer ring, for a hole the index  */
/* within its instance of the outer ring of the component around it (`rounds`: 2^rounds >= R; near_ws int32 [2 R]).         */
int rsp_mask_polygon_write(int64_t P, int32_t k, int32_t H, int64_t R, int64_t V, int32_t rounds, const int32_t* pieces,
                           const int64_t* piece_offs, const int64_t* ekey, const int32_t* eoth, const int64_t* ring_key,
                           const uint8_t* flags, const int32_t* corners, const int64_t* ring_keys, const int64_t* ring_offs,
                           const int64_t* ring_area2, const int64_t* inst_ring_offs, int32_t* near_ws, int32_t* verts,
                           int32_t* ring_parent, rsp_stream_t stream);

/* Polygon simplification (csrc/ring_simplify.hip): exact Douglas-Peucker on the rings rsp_mask_polygon_write   */
/* leaves (or any rings in that layout: verts int32 [V, 2] with coordinates in [0, 2^20], ring_offs int64 [R + 1]).  A ring   */
/* is closed (v_m = v_0); v_0 and the vertex farthest from it are kept, then every chain between two kept vertices splits at  */
/* its vertex farthest from the SEGMENT between them (lowest index among equals) while 256 * distance^2 > tol2_q8, tol2_q8 =  */
/* round(256 tolerance^2) in [0, 2^40]; all comparisons are exact 128-bit integer ones.  max(H, W) <= 2^20 (the coordinate    */
/* bound) is checked.  Writes keep uint8 [V] (1: kept), pos int32 [V] (kept vertices of the ring in front of the vertex),     */
/* kept_cnt int32 [R], area2 int64 [R] (doubled area of the kept ring) and rounds int32 [R] (rounds that kept a vertex: the   */
/* depth of the ring's split tree).  Rings of up to 64 vertices take one wave each, longer ones a block each; variant 0 is    */
/* the product's choice (256 threads a block), 1 / 2 = 128 / 512 threads, 3 = every ring through the block path (the          */
/* alternatives tools/bench_ring_simplify.py measures; all give the same result).  No host read, no atomics.                  */
#define RSP_RING_SIMPLIFY_MAX_SIDE (1 << 20)         /* coordinates in [0, 2^20]: every distance comparison fits 128-bit integers */
#define RSP_RING_SIMPLIFY_MAX_TOL2_Q8 (1LL << 40)   /* tolerance^2 in 1 / 256 px^2: tolerances up to 65 536 px                   */
int rsp_ring_simplify_mark(const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V, int64_t tol2_q8, int32_t H,
                           int32_t W, int32_t variant, uint8_t* keep, int32_t* pos, int32_t* kept_cnt, int64_t* area2,
                           int32_t* rounds, rsp_stream_t stream);
/* Which rings stay (one lane per ring): |ring_area2| >= 2 min_ring_area (the area BEFORE simplification), at least 3 kept   */
/* vertices, a new doubled area that is not 0 and has the old one's sign, and for a hole a parent that stays.  Writes sums    */
/* int64 [2, R]: row 0 = 1 / 0, row 1 = the kept vertices of a ring that stays / 0.                                           */
int rsp_ring_simplify_survive(const int32_t* ring_inst, const int32_t* ring_parent, const int64_t* ring_area2,
                              const int64_t* inst_ring_offs, int64_t R, int32_t k, int64_t min_ring_area, const int32_t* kept_cnt,
                              const int64_t* area2_new, int64_t* sums, rsp_stream_t stream);
/* ... and their compaction: csum int64 [2, R] = the inclusive sums of the rows of `sums` over the rings, R2 / V2 = their     */
/* totals (the surviving rings and their vertices).  Writes verts_out int32 [V2, 2], ring_offs_out int64 [R2 + 1],            */
/* ring_inst_out / ring_parent_out (re-indexed among the survivors of the instance) / ring_src_out int32 [R2] (the survivor's */
/* index among the input rings), ring_area2_out int64 [R2] and inst_ring_offs_out int64 [k + 1].  R2 = 0 writes nothing.      */
int rsp_ring_simplify_write(const int32_t* verts, const int64_t* ring_offs, const int32_t* ring_inst, const int32_t* ring_parent,
                            const int64_t* inst_ring_offs, int64_t R, int64_t V, int32_t k, const uint8_t* keep,
                            const int32_t* pos, const int64_t* area2_new, const int64_t* sums, const int64_t* csum, int64_t R2,
                            int64_t V2, int32_t* verts_out, int64_t* ring_offs_out, int32_t* ring_inst_out,
                            int32_t* ring_parent_out, int64_t* ring_area2_out, int64_t* inst_ring_offs_out, int32_t* ring_src_out,
                            rsp_stream_t stream);

/* Shared-border simplification (csrc/ring_coverage.hip): the rings of a PLANAR layer (a run table whose rows are */
/* pairwise disjoint and canonical, what the rsp_run_flatten_* pipeline leaves) simplified so that a border between two          */
/* instances keeps the same vertices on both sides; replaces shapely.coverage_simplify / GEOS CoverageSimplifier on the host.   */
/* The table is read through the column-ordered pieces of rsp_run_flatten_columns: cpieces int32 [4, P] (x, y0, y1, instance     */
/* sorted by (x, y0)) and col_offs int32 [W + 1]; owner(x, y) = the instance of the pixel, -1 for background and outside.        */
/* Refused with RSP_EINVAL: H * W >= 2^31, a side above RSP_RING_COVERAGE_MAX_SIDE, P > RSP_RUN_PIECES_MAX_PIECES, negative      */
/* sizes, a null pointer where something is read or written.  No call reads the host, none uses atomics, every output slot is   */
/* stored once; every index read from an input array is clamped into the array it addresses.                                   */
/* 1. bad int32 [P]: 1 where a piece overlaps its successor in the column (the rows are not disjoint: in a column sorted by y0   */
/* any overlap shows there), 2 where two pieces of one instance touch (a zero count inside a row: not canonical), else 0.        */
#define RSP_RING_COVERAGE_MAX_SIDE RSP_RING_SIMPLIFY_MAX_SIDE
int rsp_ring_coverage_check(const int32_t* cpieces, int64_t P, int32_t H, int32_t W, int32_t* bad, rsp_stream_t stream);
/* 2. The noded rings.  verts / ring_offs: the rings of rsp_mask_polygon_write on that table.  A lattice point is a NODE iff at  */
/* least 3 of the 4 sides that meet in it separate different owners.  One lane per ring segment v_i -> v_{i+1}.  _count: cnt     */
/* int32 [V] = 1 + the nodes strictly inside the segment (the change points of the far-side owner), first int32 [V] = where the  */
/* segment's first node sits (0: v_i itself, 1: its first inner node, -1: none).  The caller's exclusive sum of cnt is noff      */
/* int64 [V + 1], Vn = noff[V]; rot int64 [R] = the index within the noded ring of its first node visit (0 without one).         */
/* _write: the noded rings, each rotated to begin at rot (ring r is noff[ring_offs[r]] .. noff[ring_offs[r + 1]]): nverts int32  */
/* [Vn, 2], nflag uint8 [Vn] (1: node), nother int32 [Vn] = the owner on the far side of the unit step that leaves the vertex.   */
int rsp_ring_coverage_nodes_count(const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V, const int32_t* cpieces,
                                  const int32_t* col_offs, int64_t P, int32_t k, int32_t H, int32_t W, int32_t* cnt,
                                  int32_t* first, rsp_stream_t stream);
int rsp_ring_coverage_nodes_write(const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V, const int32_t* cpieces,
                                  const int32_t* col_offs, int64_t P, int32_t k, int32_t H, int32_t W, const int64_t* noff,
                                  const int64_t* rot, int64_t Vn, int32_t* nverts, uint8_t* nflag, int32_t* nother,
                                  rsp_stream_t stream);
/* 3. rsp_ring_simplify_mark on the noded rings with three changes: `keep` is read as well as written -- a vertex whose byte is */
/* not 0 (a node) is kept from the start, with index 0; among equal distances the vertex with the smallest (x, y) wins; a chain  */
/* whose two ends are the same point splits without the tolerance test.  All three are symmetric under reversal of a chain, so   */
/* the two rings along a border keep the same vertices.  Arguments, limits, outputs and variants as rsp_ring_simplify_mark;      */
/* rsp_ring_simplify_survive (min_ring_area 0) and rsp_ring_simplify_write follow on the noded layout.                           */
int rsp_ring_coverage_mark(const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V, int64_t tol2_q8, int32_t H,
                           int32_t W, int32_t variant, uint8_t* keep, int32_t* pos, int32_t* kept_cnt, int64_t* area2,
                           int32_t* rounds, rsp_stream_t stream);
/* 4. nother compacted like the vertices: other_out int32 [V2], with keep / pos of the mark and sums / csum / V2 as               */
/* rsp_ring_simplify_write takes them (ring_offs / R / V: the noded rings).                                                      */
int rsp_ring_coverage_other(const int64_t* ring_offs, int64_t R, int64_t V, const uint8_t* keep, const int32_t* pos,
                            const int64_t* sums, const int64_t* csum, int64_t V2, const int32_t* nother, int32_t* other_out,
                            rsp_stream_t stream);

/* Oriented boxes (csrc/mask_obb.hip): the convex hull and the minimum-area rectangle of every mask of a run    */
/* table, exact in integers; replaces decoding every instance to a dense H x W array on the host + cv2.convexHull +           */
/* cv2.minAreaRect.  Pixel (x, y) covers [x, x + 1] x [y, y + 1]; an instance is the union of the squares of ALL its pixels.  */
/* counts [k, cap] / n [k]: k masks on ONE (H, W) canvas as above (n <= 0: no vertices; n beyond cap is read up to cap).      */
/* H * W >= 2^31 and max(H, W) > 65 535 are refused (RSP_EINVAL).  No call reads the host, none uses atomics.                 */
/* 1. bound_offs int64 [k + 1], ascending from 0, bound_offs[m + 1] - bound_offs[m] >= 3 * (min(n[m], cap) / 2) (a row whose   */
/* slot is smaller has no vertices), B = bound_offs[k] <= 2^30 - 1; workspace: rsp_mask_hull_workspace_bytes(B) (0: B out of   */
/* range).  One block per (instance, chain): the first / last set pixel of every column from the run stream, then the upper   */
/* and the lower hull chain by pruning rounds.  Writes chain_cnt int32 [2, k] (the vertices of the upper / lower chain, each   */
/* with both of its ends) and rounds int32 [2, k] (the pruning rounds that removed a point); the chains stay in the workspace. */
#define RSP_MASK_OBB_MAX_SIDE 65535            /* x and y fit 16 bits each: every product of the calipers fits 128 bits        */
#define RSP_MASK_OBB_MAX_BOUND 0x3fffffffLL    /* three records per ones-run over all rows of one call (32-bit hull offsets)   */
int64_t rsp_mask_hull_workspace_bytes(int64_t B);
int rsp_mask_hull_chains(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                         const int64_t* bound_offs, int64_t B, void* workspace, int32_t* chain_cnt, int32_t* rounds,
                         rsp_stream_t stream);
/* 2. hull_offs int64 [k + 1] = the exclusive sum of chain_cnt[0] + chain_cnt[1], Vh = hull_offs[k] < 2^31.  Writes hull_verts */
/* int32 [Vh, 2] = (x, y): per instance the strictly convex hull from its smallest vertex by (x, y) on, clockwise on screen,    */
/* first vertex not repeated (at least 4 vertices for a non-empty instance), and hull_area2 int64 [k], its doubled area (> 0;  */
/* 0 for an empty instance).                                                                                                  */
int rsp_mask_hull_write(const int32_t* n, int32_t k, int32_t cap, const int64_t* bound_offs, int64_t B, const void* workspace,
                        const int32_t* chain_cnt, const int64_t* hull_offs, int64_t Vh, int32_t* hull_verts,
                        int64_t* hull_area2, rsp_stream_t stream);
/* The minimum-area rectangle of k convex polygons in that layout (any strictly convex rings, clockwise on screen, coordinates */
/* in [0, 65 535]), one block per polygon.  Edge j runs from vertex j to j + 1 (cyclic): e = (ex, ey), nrm = (-ey, ex), L =     */
/* |e|^2; over the vertices p, a = p . e and b = p . nrm.  The rectangle flush with edge j has area (amax - amin) (bmax - bmin)  */
/* / L; edge int32 [k] = the edge that minimises it, compared exactly in 128-bit integers, the lowest among equals (-1 for a    */
/* polygon without vertices); q int64 [k, 6] = (ex, ey, amin, amax, bmin, bmax) of that edge (zeros for -1).                    */
int rsp_hull_min_rect(const int32_t* hull_verts, const int64_t* hull_offs, int32_t k, int64_t Vh, int32_t* edge, int64_t* q,
                      rsp_stream_t stream);

/* Oriented-box comparison (csrc/obb_iou.hip): rotated IoU and mmcv's nms_rotated.  A box is a convex          */
/* quadrilateral, double [4][2] = (x, y) of its corners in order, in pixel coordinates: the corner form of                   */
/* rle.obb_to_numpy (clockwise on screen, sum x_i y_{i+1} - x_{i+1} y_i > 0); the opposite orientation is accepted and        */
/* normalised by the sign of the doubled area.  A box with a non-finite coordinate or zero area is DEGENERATE: its IoU with   */
/* everything is 0.0, it suppresses nothing and the NMS keeps it (the NaN row of an empty mask takes this path).  No atomics; */
/* a second launch gives the same bits.                                                                                      */
/* rsp_obb_corners: edge int32 [k] / q int64 [k, 6] as rsp_hull_min_rect writes them, offset int32 [k, 2] = (ox, oy) or NULL  */
/* -> corners double [k, 4, 2].  The offset moves q in integers first (a += ox ex + oy ey, b += -ox ey + oy ex); a corner is  */
/* then ((a ex - b ey) / L, (a ey + b ex) / L) in fp64 with one division: the bits of rle.obb_to_numpy(form='corners') of the */
/* shifted table.  edge = -1 gives a NaN row.                                                                                 */
int rsp_obb_corners(const int32_t* edge, const int64_t* q, const int32_t* offset, int32_t k, double* corners,
                    rsp_stream_t stream);
/* IoU blocks of n_units units, as rsp_coco_iou takes them (units: DEVICE array, nwords ignored): iou[out0 + d * ng + g] of   */
/* dt_quad [n_dt, 4, 2] and gt_quad [n_gt, 4, 2], one lane per pair, in fp64: inter / (area_d + area_g - inter), inter /      */
/* area_d for a crowd gt, 0.0 when inter <= 0 or the union is not positive.  The intersection is a closed polygon: the gt     */
/* box clipped successively by the four half-planes of the dt box, both translated by the dt box's centre, one shoelace sum.  */
/* Pairs whose axis-aligned bounds do not overlap write 0.0 without clipping.  A unit that reaches outside n_dt, n_gt or      */
/* n_iou writes nothing.                                                                                                      */
int rsp_obb_iou(const RspCocoUnit* units, int32_t n_units, const double* dt_quad, int64_t n_dt, const double* gt_quad,
                int64_t n_gt, const uint8_t* gt_crowd, double* iou, int64_t n_iou, rsp_stream_t stream);
/* mmcv.ops.nms_rotated on flat arrays: quad double [n, 4, 2], scores float [n], labels int32 [n].  Order: score descending,  */
/* original position ascending; box j is suppressed by a KEPT box i ahead of it iff they share a label (or class_agnostic !=  */
/* 0) and iou(i, j) > iou_thr (strict; iou_thr >= 0).  keep int32 [n] = indices into the input in kept order, keep_cnt int32  */
/* [1].  n <= RSP_OBB_NMS_MAX (the n x ceil(n / 64) word suppression mask is 128 MiB there); beyond it RSP_EINVAL, and        */
/* rsp_obb_nms_workspace_bytes is -1.                                                                                         */
#define RSP_OBB_NMS_MAX 32768
int64_t rsp_obb_nms_workspace_bytes(int32_t n);
int rsp_obb_nms(const double* quad, const float* scores, const int32_t* labels, int32_t n, double iou_thr,
                int32_t class_agnostic, void* workspace, int32_t* keep, int32_t* keep_cnt, rsp_stream_t stream);

/* Run-domain connected components (csrc/run_components.hip): the 8-connected components of every mask of a     */
/* run table; replaces decoding every instance to a dense H x W array + cv2.connectedComponentsWithStats (segment-anything     */
/* utils/amg.py remove_small_regions) and the dense labelling of rsp_mask_remove_small_regions where the masks live as runs.   */
/* Input: the piece table of k masks on ONE (H, W) canvas, pieces / piece_offs / P as rsp_run_pieces leaves them.             */
/* H * W >= 2^31 and P > RSP_RUN_COMPONENTS_MAX_PIECES (32-bit piece indices) are refused (RSP_EINVAL);                        */
/* rsp_run_components_workspace_bytes(H, W, P) is -1 for what the calls refuse.  No call reads the host.  Atomics: integer     */
/* min / max / add only, so a second launch gives the same bits.                                                              */
/* 1. Writes label int32 [P] = the lowest piece index of the piece's component, -1 for a slot no row filled (pieces of columns  */
/* x and x + 1 are joined iff their closed row ranges, widened by one row, overlap), root int32 [P] = 1 where label[p] == p.    */
/* status int32 [1], zeroed by the caller: set to 1 when a find / union loop reached its step cap (the result is then invalid;  */
/* a correct run never does).                                                                                                  */
#define RSP_RUN_COMPONENTS_MAX_PIECES RSP_RUN_PIECES_MAX_PIECES
int64_t rsp_run_components_workspace_bytes(int32_t H, int32_t W, int64_t P);
int rsp_run_components_label(int32_t k, int32_t H, int32_t W, const int64_t* piece_offs, int64_t P, const int32_t* pieces,
                             void* workspace, int32_t* label, int32_t* root, int32_t* status, rsp_stream_t stream);
/* 2. root_cum int64 [P] = the inclusive sum of root, C = root_cum[P - 1]: component c is the c-th root, which orders the       */
/* components by (instance, label).  Writes piece_comp int32 [P] (-1 for an unfilled slot), comp_area int32 [C], comp_box       */
/* int32 [C, 4] = (x0, y0, x1, y1) end-exclusive as rsp_rle_bbox, comp_first int32 [C] = the lowest row-major index y W + x of  */
/* the component's pixels (the tie rule of rsp_mask_remove_small_regions), comp_inst int32 [C].                                 */
int rsp_run_components_stats(const int32_t* pieces, int64_t P, int32_t H, int32_t W, const int32_t* label, const int32_t* root,
                             const int64_t* root_cum, int64_t C, int32_t* piece_comp, int32_t* comp_area, int32_t* comp_box,
                             int32_t* comp_first, int32_t* comp_inst, rsp_stream_t stream);
/* 3. Which components stay, one block per instance over comp_offs int64 [k + 1]: keep int32 [C] = 1 for a component of at      */
/* least min_area pixels; keep_largest != 0 (islands): when an instance has none, its largest stays, the one with the lowest    */
/* comp_first among equals.  changed int32 [k, 2]: column `slot` = 1 when the instance has a smaller component.                 */
int rsp_run_components_select(const int64_t* comp_offs, int32_t k, int64_t C, const int32_t* comp_area, const int32_t* comp_first,
                              int32_t min_area, int32_t keep_largest, int32_t slot, int32_t* keep, int32_t* changed,
                              rsp_stream_t stream);

/* Run-domain morphology (csrc/run_morphology.hip): erosion of every mask of a run table by the (2 r + 1)^2      */
/* square in work proportional to the column pieces times log r; replaces cv2.erode / cv2.dilate on dense masks and, with the    */
/* difference at the end, boundary-iou-api's mask_to_boundary (decode, copyMakeBorder, d iterations of cv2.erode, encode per      */
/* mask on the host).  Input of the first two: counts [k, cap] / n [k] of k masks on ONE (H, W) canvas, CANONICAL as             */
/* rsp_rle_union writes them (rsprompter_amd/ops.py canonicalises a table with a group-of-one union first); a row with n <= 0   */
/* has no pieces, n beyond cap is read up to cap.  H * W >= 2^31 and k * (W + 2 pad) >= 2^31 are refused (RSP_EINVAL).  A TABLE  */
/* is col / y0 / y1 int32 [P]: the intervals [y0, y1) of column col = instance * Wt + X, sorted by (col, y0), disjoint and not   */
/* touching within a column.  No call reads the host, none uses atomics; every output slot is stored once.                       */
/* 1. Level 1: the column pieces of every ones-run shrunk to [y0 + ry, y1 - ry), empty ones dropped.  border = 1: an end on the  */
/* canvas edge stays and `pad` columns [0, H) stand on either side (Wt = W + 2 pad, canvas column x is X = x + pad); border = 0  */
/* takes pad = 0.  ry <= H, pad <= W.  _count: piece_cnt int32 [k] (pad columns included); the caller's exclusive sum is          */
/* piece_offs int64 [k + 1], P = piece_offs[k] < 2^31.  ry = pad = border = 0 gives the pieces themselves.                       */
int rsp_run_morph_pieces_count(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W, int32_t ry,
                               int32_t pad, int32_t border, int32_t* piece_cnt, rsp_stream_t stream);
int rsp_run_morph_pieces(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W, int32_t ry,
                         int32_t pad, int32_t border, const int64_t* piece_offs, int64_t P, int32_t* col, int32_t* y0, int32_t* y1,
                         rsp_stream_t stream);
/* 2. Join, one lane per interval of table A (PA intervals on strips of Wa columns) against column X + shift of table B (PB      */
/* intervals, strips of Wb columns, b_offs int32 [k Wb + 1] = the first interval of every column): op 0 = the intersections,     */
/* none when X + span > Wa or X + shift is outside B's strip; op 1 = A minus B (all of A where B has no such column; shift may  */
/* be negative there, op 0 takes shift >= 0).  The                                                                              */
/* output column is X + out_shift on strips of Wout columns; an interval whose output column falls outside writes nothing.       */
/* _count: cnt int32 [PA]; the caller's exclusive sum is out_offs int64 [PA + 1], total = out_offs[PA] < 2^31.  emit_keys = 0:    */
/* the result as a table (o_col, o_y0, o_y1 [total]); emit_keys = 1: as rsp_rle_union's intervals on the (H, Wout) canvas,       */
/* keys int64 [total] = instance << 31 | pixel start, ends int32 [total], in key order as they stand.                            */
int rsp_run_morph_join_count(int32_t op, const int32_t* a_col, const int32_t* a_y0, const int32_t* a_y1, int64_t PA, int32_t Wa,
                             const int32_t* b_offs, const int32_t* b_y0, const int32_t* b_y1, int64_t PB, int32_t k, int32_t Wb,
                             int32_t shift, int32_t span, int32_t out_shift, int32_t Wout, int32_t* cnt, rsp_stream_t stream);
int rsp_run_morph_join(int32_t op, const int32_t* a_col, const int32_t* a_y0, const int32_t* a_y1, int64_t PA, int32_t Wa,
                       const int32_t* b_offs, const int32_t* b_y0, const int32_t* b_y1, int64_t PB, int32_t k, int32_t Wb,
                       int32_t shift, int32_t span, const int64_t* out_offs, int64_t total, int32_t out_shift, int32_t Wout,
                       int32_t H, int32_t emit_keys, int32_t* o_col, int32_t* o_y0, int32_t* o_y1, int64_t* keys, int32_t* ends,
                       rsp_stream_t stream);

/* Euclidean buffers (csrc/run_disc.hip): dilation of every mask of a run table by the exact disc dx^2 + dy^2 <=  */
/* r2 or the diamond; replaces scipy.ndimage.binary_dilation / distance_transform_edt on dense masks and the buffer step of a      */
/* GIS after vector export.  The structuring element is hh int32 [R + 1]: hh[dx] = the rows it reaches above and below its         */
/* centre at column offset dx, NON-INCREASING, filled on the host (isqrt(r2 - dx^2), or r - dx), entries cut into [0, H]; R <=     */
/* W - 1.  One lane per (interval of a TABLE of rsp_run_morph_pieces / rsp_run_morph_join on strips of W columns, dx) stores one   */
/* interval of rsp_rle_union on the (H, W) canvas, keys = instance << 31 | pixel start, the interval [y0, y1) grown to             */
/* [max(y0 - hh[dx], 0), min(y1 + hh[dx], H)) in column X + dir * dx.  dir = 0: dx = 0 only, slot base + i for interval i.  dir =  */
/* +1 / -1: dx = 1 .. R, targets outside [0, W) are skipped, slots base + slot_offs[i] .. base + slot_offs[i + 1] in the order of  */
/* dx, slot_offs int64 [P + 1] = the caller's exclusive sum of min(R, W - 1 - X) / min(R, X).  total = the length of keys / ends;  */
/* slots at or beyond it are not written.  The intervals are NOT in key order: the caller sorts them before rsp_rle_union.  With   */
/* the table = the pieces for dir 0 and the pieces minus those of the next / previous column (rsp_run_morph_join, op 1, shift      */
/* +1 / -1) for dir +1 / -1, the union of the three calls is the dilation.  No host read, no atomics, every slot stored once.      */
/* Refused with RSP_EINVAL: H * W >= 2^31, k * W >= 2^31, P or total >= 2^31, R < 0 or R > W - 1, dir outside -1 .. 1, base        */
/* outside [0, total], a null pointer where something is read or written.                                                         */
int rsp_run_disc_emit(const int32_t* col, const int32_t* y0, const int32_t* y1, int64_t P, int32_t k, int32_t H, int32_t W,
                      const int32_t* hh, int32_t R, int32_t dir, const int64_t* slot_offs, int64_t base, int64_t total,
                      int64_t* keys, int32_t* ends, rsp_stream_t stream);

/* Planar instance layers (csrc/run_flatten.hip): the k masks of a run table made pairwise disjoint by a         */
/* priority, row i = M_i minus every M_j with rank[j] < rank[i]; replaces the per-pixel argmax over dense [k, H, W] masks of      */
/* MaskFormerFusionHead.panoptic_postprocess (mmdet maskformer_fusion_head.py:70-104) for binary masks, and decode -> argmax ->  */
/* encode on scene masks.  Input: the piece table of k masks on ONE (H, W) canvas, pieces int32 [4, P] / P as rsp_run_pieces      */
/* leaves them (planes x, y0, y1, instance, sorted by (instance, x, y0)), and the caller's copy of it sorted by column: skeys     */
/* int64 [P] = (x * H + y0) << 31 | piece index, ascending, cpieces int32 [4, P] = the same planes in that order.  rank int32 [k]: */
/* a permutation of 0 .. k - 1, 0 wins (only compared: any values give SOME answer).  Refused with RSP_EINVAL: a null pointer      */
/* where something is read or written, H * W >= 2^31, P > RSP_RUN_PIECES_MAX_PIECES, k < 0, total >= 2^31.  No call reads the      */
/* host, none uses atomics, every output slot is stored once; offsets read from col_offs / out_offs are clamped into their         */
/* arrays, whatever they hold.  No workspace.                                                                                     */
/* 1. col_offs int32 [W + 1] = the first piece of every column in the sorted copy; reach int32 [P], reach[j] = the largest y1     */
/* among the pieces of j's column at or before j (one wave per column, a max-scan with a carry).                                  */
int rsp_run_flatten_columns(const int64_t* skeys, const int32_t* cpieces, int64_t P, int32_t H, int32_t W, int32_t* col_offs,
                            int32_t* reach, rsp_stream_t stream);
/* 2. One lane per piece: the parts of the piece that no piece of a smaller rank in its column covers.  _count: cnt int32 [P];    */
/* the caller's exclusive sum is out_offs int64 [P + 1], total = out_offs[P].  _write stores them as rsp_rle_union's intervals,   */
/* keys int64 [total] = instance << 31 | pixel start, ends int32 [total], in key order as they stand; the intervals of instance   */
/* i are out_offs[piece_offs[i]] .. out_offs[piece_offs[i + 1]].  A piece whose instance is outside [0, k) has none.              */
int rsp_run_flatten_count(const int32_t* pieces, const int32_t* cpieces, const int32_t* col_offs, const int32_t* reach,
                          const int32_t* rank, int64_t P, int32_t k, int32_t H, int32_t W, int32_t* cnt, rsp_stream_t stream);
int rsp_run_flatten_write(const int32_t* pieces, const int32_t* cpieces, const int32_t* col_offs, const int32_t* reach,
                          const int32_t* rank, int64_t P, int32_t k, int32_t H, int32_t W, const int64_t* out_offs, int64_t total,
                          int64_t* keys, int32_t* ends, rsp_stream_t stream);
/* 3. The label map of DISJOINT masks given as intervals in that layout (any order): labels int32 [W, H] -- the column-major      */
/* stream of the run counts, in which every interval is contiguous; the caller reads it transposed -- zeroed, then ids[instance]  */
/* (ids int32 [k]) over every interval, one wave per interval.  Where intervals overlap a pixel takes one of their values.        */
int rsp_run_flatten_paint(const int64_t* keys, const int32_t* ends, int64_t total, const int32_t* ids, int32_t k, int32_t H,
                          int32_t W, int32_t* labels, rsp_stream_t stream);

/* Polygon rasterisation (csrc/poly_raster.hip): rings of float64 vertices -> run tables; replaces cocoapi's    */
/* maskApi.c rleFrPoly (one polygon at 5x resolution, its sort and its sequential run loop) per part, and with the caller's     */
/* grouping rleMerge / COCO.annToRLE (rsprompter_amd/rle.py polygons_to_runs).  The result is rleFrPoly's, count for count.     */
/* verts double [V, 2] = (x, y), any finite values; ring_offs int64 [R + 1] ascending from 0 to V (a ring without vertices      */
/* contributes nothing; rings of one and two vertices follow rleFrPoly); ring_group int32 [R], non-decreasing, in [0, G);        */
/* group_hw int32 [G, 2] = (h, w) of EACH group's canvas.  All rings of a group are rasterised onto one canvas with the         */
/* even-odd rule (a group of one ring is rleFrPoly of it).  The three calls are one pipeline; the caller reads three numbers     */
/* after the first and sorts the keys after the second.  No call reads the host, none uses atomics.                              */
/* Limits, refused with RSP_EINVAL: a group canvas with h < 1, w < 1 or h * w >= 2^31; a scaled coordinate (int)(5 x + .5)      */
/* beyond +-RSP_POLY_RASTER_MAX_COORD; more than RSP_POLY_RASTER_MAX_POINTS walk points; more than                               */
/* RSP_POLY_RASTER_MAX_GROUPS groups.                                                                                            */
/* 1. Writes scaled int32 [V, 2] (a value out of range is pinned to +-(RSP_POLY_RASTER_MAX_COORD + 2)), edge_pts int64 [V] =     */
/* max(|dx|, |dy|) + 1 walk points of the edge from vertex j to the next vertex of its ring (the last one to the first), and     */
/* group_px int64 [G] = h * w, 2^31 for a canvas that is refused.                                                                */
#define RSP_POLY_RASTER_MAX_COORD (1 << 24)
#define RSP_POLY_RASTER_MAX_POINTS 0x7fffffffLL
#define RSP_POLY_RASTER_MAX_GROUPS 0xffffff
#define RSP_POLY_RASTER_NO_KEY 0x7fffffffffffffffLL
int rsp_poly_raster_edges(const double* verts, const int64_t* ring_offs, const int32_t* group_hw, int64_t R, int64_t V,
                          int32_t G, int32_t* scaled, int64_t* edge_pts, int64_t* group_px, rsp_stream_t stream);
/* 2. edge_offs int64 [V + 1] = exclusive sum of edge_pts, T = edge_offs[V]; coord_max = the largest |scaled| and pixels_max =   */
/* the largest group_px, as the caller read them (they are what this call and the next refuse on).  One lane per walk point:     */
/* keys int64 [T] = group << 32 | xd * h + yd for a point that crosses a pixel column inside the canvas by rleFrPoly's rule,     */
/* RSP_POLY_RASTER_NO_KEY otherwise.                                                                                            */
int rsp_poly_raster_crossings(const int32_t* scaled, const int64_t* ring_offs, const int32_t* ring_group, const int32_t* group_hw,
                              const int64_t* edge_offs, int64_t R, int64_t V, int32_t G, int64_t T, int64_t coord_max,
                              int64_t pixels_max, int64_t* keys, rsp_stream_t stream);
/* 3. keys int64 [K] sorted ascending; key_offs int64 [G + 1] = the keys of group g (clamped into [0, K]).  counts_out            */
/* [G, cap_out] / n_out [G]: rleFrPoly's counts, conventions of rsp_rle_shift: canonical (only count 0 may be zero, the counts    */
/* sum to h * w), n_out = -(needed) when cap_out is too small (the row is then undefined); a group without keys is one count     */
/* h * w.  A position below h * w is a run boundary iff it occurs an odd number of times; h * w always is one.                    */
int rsp_poly_raster_runs(const int64_t* keys, int64_t K, const int64_t* key_offs, const int32_t* group_hw, int32_t G,
                         int64_t pixels_max, uint32_t* counts_out, int32_t* n_out, int32_t cap_out, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Promptable SAM (HF SamModel with point / box / mask prompts, mask generation) */
/* ------------------------------------------------------------------------ */
/* HF SamPromptEncoder._embed_points / _embed_boxes / forward (modeling_sam.py:613-698) over SamPositionalEmbedding.forward  */
/* (:552-566) for R prompt sets: points [R, P, 2] (x, y in input pixels; NULL when P == 0), labels int32 [R, P] (1 / 0: add  */
/* point_embed1 / point_embed0, -1: the row becomes not_a_point_embed, -10: zeros, anything else: the bare encoding), boxes  */
/* [R, 4] or NULL, pad = 1 appends the padding point (label -1; HF pads when there is no box, pad with boxes is refused) ->  */
/* out [R, P + pad + 2 * (boxes != NULL), 2 * num_pos_feats] in HF's order: points, padding point, the two box corners.      */
/* labels == NULL with points: SamPositionalEmbedding.forward itself (no + 0.5, no type embedding; pass input_h = input_w =   */
/* 1 for `input_shape=None`).  A boxes-only call returns the bits of rsp_sam_embed_boxes.                                    */
int rsp_sam_embed_prompts(const float* points, const int32_t* labels, const float* boxes, int32_t R, int32_t P, int32_t pad,
                          const float* gauss, const float* point_embed0, const float* point_embed1, const float* point_embed2,
                          const float* point_embed3, const float* not_a_point_embed, float* out, int32_t num_pos_feats,
                          int32_t input_h, int32_t input_w, rsp_stream_t stream);
/* HF mask generation's scoring (image_processing_sam: _compute_stability_score, _batched_mask_to_box over                   */
/* post_process_masks) without the masks: low_res [k, h, w] logits and the geometry of rsp_mask_post_logits.  out int32      */
/* [k, 7] = number of pixels whose resized value is > t_hi, > t_lo, > t_mid (strict, fp32: the caller forms                  */
/* float(thr + offset), float(thr - offset), thr), then x0, y0, x1, y1 of the pixels > t_mid (inclusive maxima; 0 0 0 0 for  */
/* an empty mask).  The value is the one rsp_mask_post_logits thresholds (same device code): the counts are the population  */
/* counts of its masks.  Integer reductions only: the result is independent of scheduling.  Writes nothing but `out`.       */
int rsp_mask_score_box(const float* low_res, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb, int32_t crop_h,
                       int32_t crop_w, int32_t out_h, int32_t out_w, float t_hi, float t_lo, float t_mid, int32_t* out,
                       rsp_stream_t stream);

/* rsp_mask_score_box for the candidates of several crops in one call, plus HF image_processing_sam.                     */
/* _is_box_near_crop_edge (atol = 20) and the shift of the boxes into the image frame (`_pad_masks` / the offset inside    */
/* _is_box_near_crop_edge).  crop_idx: DEVICE int32 [k], the crop of every candidate (clamped into the table by the        */
/* kernel); table: DEVICE int32 [n_crops, 12] = (Hb, Wb, crop_h, crop_w, out_h, out_w, x0, y0, x1, y1, W, H): the geometry */
/* of rsp_mask_post_logits for that crop, its box in the image, the image size.  max_out_h / max_out_w: the largest out_h  */
/* and out_w of the table (they size the grid).  out int32 [k, 8]: columns 0-2 are rsp_mask_score_box's counts for that    */
/* crop's geometry (same device functions, the strip form chosen per crop by the same condition), 3-6 its box + (x0, y0,   */
/* x0, y0) (the empty-mask box [0, 0, 0, 0] is crop-local and shifted too), 7 = 1 when a coordinate of the shifted box is  */
/* within 20 of the same coordinate of [x0, y0, x1, y1] and not within 20 of that of [0, 0, W, H].  Integer reductions     */
/* only.  A table row with a non-positive size scores as an empty mask.                                                  */
#define RSP_CROP_TABLE_COLS 12
int rsp_mask_score_box_crops(const float* low_res, int32_t k, int32_t h, int32_t w, const int32_t* crop_idx,
                             const int32_t* table, int32_t n_crops, int32_t max_out_h, int32_t max_out_w, float t_hi,
                             float t_lo, float t_mid, int32_t* out, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* PerSAM (training-free one-shot segmentation; persam.py of Zhang et al.'s code around SAM)                               */
/* ------------------------------------------------------------------------ */
/* `target_feat = ref_feat[ref_mask > 0]; target_embedding = target_feat.mean(0); target_feat = target_embedding /          */
/* target_embedding.norm()`: emb [N, 256] channels-last embedding rows of the reference, cell_mask [N] bytes (non-zero =     */
/* selected).  target_embedding, target_feature fp32 [256], count int32 [1] = selected cells, all on the device; with no     */
/* selected cell both vectors are zero (the caller refuses on the count).  Fixed summation order.                            */
int rsp_persam_target(const float* emb, const uint8_t* cell_mask, int32_t N, float* target_embedding, float* target_feature,
                      int32_t* count, rsp_stream_t stream);
/* `test_feat = test_feat / test_feat.norm(dim=0); sim = target_feat @ test_feat; sim = F.interpolate(sim, scale_factor=4,  */
/* mode='bilinear')` for B images at once: emb [B * gh * gw, 256] rows (16-byte aligned), target_feature [256].  sim         */
/* [B, gh * gw] (a zero row scores 0), low_res [B, 4 gh, 4 gw]: the layout rsp_mask_post_logits / rsp_persam_locate take.    */
int rsp_persam_similarity(const float* emb, const float* target_feature, int32_t B, int32_t gh, int32_t gw, float* sim,
                          float* low_res, rsp_stream_t stream);
/* PerSAM's `postprocess_masks(sim)` + `point_selection(sim, topk=1)` + `(sim - sim.mean()) / torch.std(sim)` +             */
/* `F.interpolate(size=(g, g), mode='bilinear').sigmoid()` without the [k, out_h, out_w] field: low_res [k, h, w] and the    */
/* geometry of rsp_mask_post_logits (the values are that entry point's `out_val`, same device functions).  stats fp32        */
/* [k, 4] = maximum, minimum, mean, unbiased standard deviation; xy int32 [k, 5] = x, y of the maximum, x, y of the minimum  */
/* (the LOWEST flat index y * out_w + x among equal values: torch.argmax / argmin of the flattened field), pixel count;     */
/* attn_sim fp32 [k, g * g] = sigmoid((D - mean) / std), D the bilinear g x g resampling of the field.  A constant field    */
/* has std 0 and 0 / 0 := 0 there: attn_sim = 0.5 (PerSAM yields NaN).  Extrema by one 64-bit integer atomic per block,     */
/* sums as fp64 block partials added in block order: no floating-point atomics, two runs give the same bits.  workspace:   */
/* rsp_persam_locate_workspace_bytes(k, out_h, out_w) bytes, 8-byte aligned (-1 for arguments the call would refuse).       */
int64_t rsp_persam_locate_workspace_bytes(int32_t k, int32_t out_h, int32_t out_w);
int rsp_persam_locate(const float* low_res, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb, int32_t crop_h,
                      int32_t crop_w, int32_t out_h, int32_t out_w, int32_t g, void* workspace, int64_t workspace_bytes,
                      float* stats, int32_t* xy, float* attn_sim, rsp_stream_t stream);

/* PerSAM-F (persam_f.py of the same code): `logits_high = (logits_high * weights).sum(0)`, `dice_loss + focal_loss` of it     */
/* against the reference mask, `loss.backward(); optimizer.step(); scheduler.step()` -- without autograd and without an        */
/* image-sized tensor.  low_res [k, 3, h, w]: per problem the three low-resolution logit maps of ONE decoder pass; the        */
/* geometry is rsp_mask_post_logits' and F_j(i) below is that entry point's `out_val` of map j (same device functions).  gt    */
/* uint8 [k, out_h, out_w], t = (gt != 0).  With w0 = 1 - w1 - w2, z = sum_j w_j F_j, p = sigmoid(z):                           */
/*   loss = 1 - (2 sum p t + 1) / (sum p + sum t + 1)                                         (dice)                          */
/*        + mean(alpha_t * BCEWithLogits(z, t) * (1 - p_t)^2)                                  (focal, gamma = 2)              */
/* and g_j = d loss / d w_j for j = 1, 2, from nine sums over the field ("PerSAM-F").  z in fp64, the rest  */
/* of a pixel in fp32 (precise expf / log1pf), sums as fp64 block partials added in block order: no floating-point atomics,  */
/* two runs give the same bits.  The k problems share one geometry and are independent.                                      */
/* rsp_persam_f_loss_grad: one evaluation at weights fp32 [k, 2] = (w1, w2); out fp64 [k, 3] = loss, g1, g2.                   */
/* rsp_persam_f_fit: the whole fit, enqueued on the stream (2 launches per epoch, no host read): w1 = w2 = fp32 1 / 3, then  */
/* `epochs` steps of torch.optim.AdamW(lr, betas, eps, weight_decay) (decoupled decay, bias-corrected, denom =                */
/* sqrt(v) / sqrt(bc2) + eps) under CosineAnnealingLR(T_max = epochs): step e uses lr / 2 (1 + cos(pi e / epochs)); the      */
/* optimiser state is fp64 on the device.  weights fp32 [k, 3] = w0, w1, w2 after the last step; history fp64                 */
/* [k, epochs, 3] or NULL = the loss and gradient each step was taken from (row 0: rsp_persam_f_loss_grad at 1 / 3).          */
/* workspace: rsp_persam_f_workspace_bytes(k, out_h, out_w, epochs) bytes, 8-byte aligned (-1 for arguments the calls would   */
/* refuse).  RSP_EINVAL: k < 1, epochs < 1, an invalid geometry, out_h * out_w >= 2^31, a null pointer (history excepted), a   */
/* workspace that is too small.                                                                                              */
int64_t rsp_persam_f_workspace_bytes(int32_t k, int32_t out_h, int32_t out_w, int32_t epochs);
int rsp_persam_f_loss_grad(const float* low_res, const uint8_t* gt, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb,
                           int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w, const float* weights, float alpha,
                           void* workspace, int64_t workspace_bytes, double* out, rsp_stream_t stream);
int rsp_persam_f_fit(const float* low_res, const uint8_t* gt, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb,
                     int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w, int32_t epochs, double lr, double beta1,
                     double beta2, double eps, double weight_decay, float alpha, void* workspace, int64_t workspace_bytes,
                     float* weights, double* history, rsp_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Small-region cleanup of masks (segment-anything utils/amg.py `remove_small_regions`, used by                            */
/* automatic_mask_generator.py `postprocess_small_regions`; there cv2.connectedComponentsWithStats on the host)           */
/* ------------------------------------------------------------------------ */
/* masks uint8 [k, H, W] (non-zero = set: what rsp_mask_post_logits writes) -> out uint8 [k, H, W] of 0 / 1, a buffer     */
/* distinct from `masks`.  mode 1 ("holes"): the 8-connected components of the ZEROS with fewer than min_area pixels are   */
/* set (the background is a component like any other); mode 2 ("islands"): the 8-connected components of the ONES with     */
/* fewer than min_area pixels are cleared -- when every component is that small the largest stays, among equals the one   */
/* that holds the lowest pixel index y * W + x (segment-anything leaves that to OpenCV's label order); mode 3: holes, then */
/* islands of the filled mask.  A mask without a small component is copied (as 0 / 1).  info int32 [k, 8] = changed by    */
/* the holes pass, changed by the islands pass (0 / 1: a small component existed), x0, y0, x1, y1 of the result (inclusive */
/* maxima, 0 0 0 0 when empty), its population count, status (non-zero: a find / union loop reached its step cap -- the    */
/* result is then invalid; a correct run never does).  A component's label is the minimum pixel index of its members and   */
/* every size, box and count an integer reduction: the result does not depend on scheduling.  workspace:                  */
/* rsp_mask_regions_workspace_bytes(k, H, W) bytes, 16-byte aligned (-1 for arguments the call would refuse).  RSP_EINVAL: */
/* mode outside 1..3, min_area < 0, H * W >= 2^31, a non-positive size; k = 0 does nothing.                                */
/* Components are labelled inside tiles of RSP_MASK_REGION_TILE_H x _W pixels first, then merged across the tile borders.   */
#define RSP_MASK_REGION_TILE_H 64
#define RSP_MASK_REGION_TILE_W 64
int64_t rsp_mask_regions_workspace_bytes(int32_t k, int32_t H, int32_t W);
int rsp_mask_remove_small_regions(const uint8_t* masks, int32_t k, int32_t H, int32_t W, int32_t min_area, int32_t mode,
                                  void* workspace, uint8_t* out, int32_t* info, rsp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSP_HIP_H_ */
