// SAM-HQ's mask branch (HF transformers models/sam_hq/modeling_sam_hq.py:1007-1037) as ONE kernel per prompt set and tile:
//   mask_hq[r, p] = < hyper_hq[r], mask_conv2( GELU( LN_64( mask_conv1(U_r) ) ) )[p] + hq_features[b(r), p] >
// with U_r = GELU(ConvTranspose2d(64 -> 32, k2 s2)(up_s(r))) the upscaled embedding [4g, 4g, 32] of prompt set r, which HF
// materialises together with the two 3x3 convolutions' [R, 64 | 32, 4g, 4g] results (8 - 16 MB each per prompt set at g = 64).
// `up` is addressed through a row map (s(r): in HF's decoder the upscaled embedding depends on the image and its dense prompt
// only, sam_decoder.py), and the kernel can emit SAM's own masks <hyper_sam[r, t], U_r> + mask_hq[r] from the same U tile.
// Here a block owns a 16 x 16 output tile of one prompt set and nothing but the [R, 4g, 4g] logits is written:
//   1. U on the tile + a 2-pixel halo (20 x 20): every U pixel depends on ONE pixel of `up` (the 10 x 10 input pixels of
//      the tile, one 32-pixel MFMA tile per wave), so the halo costs recomputation only.  GELU, zero outside the image
//      (mask_conv1's padding), fp16 hi / lo at scale 2^8 into LDS.
//   2. mask_conv1 on the 1-pixel-halo region (18 x 18 = 324 pixels, 11 MFMA tiles of 32, three per wave) as a GEMM with
//      K = 9 taps x 32 channels = 288 (18 k-steps of v_mfma_f32_32x32x16_f16, fp16x3 as everywhere): A = the weight rows
//      (resident in LDS, 2 x 64 x 288 halves), B = the U pixels read at the tap's offset, accumulator = lane <-> pixel,
//      registers <-> channels, so
//   3. LayerNorm over the 64 channels is in the lane + lane ^ 32; GELU; zero outside the image (mask_conv2's padding);
//      fp32 into LDS (over the U / weight images, which nobody reads any more).
//   4. mask_conv2 and the dot with hyper_hq are both linear, so they are ONE 3 x 3 filter with one output channel per
//      prompt set: w'[tap, ci] = sum_c hyper_hq[c] W2[c, ci, tap] (576 values, formed by the block in fp32 at its start,
//      the trick of t2i_fold.hip) -- 32 x less work than the 64 -> 32 convolution; + <hyper_hq, bias2> + <hyper_hq, hq_features>.
//      One output pixel per thread, fp32 on the vector units.
// LDS: 64 000 B (U) + 75 776 B (W1) + 2 320 B (w'): one block of four waves per CU.
#include "rsp_common.h"

namespace {

constexpr int HQ_TILE = 16;                 // output tile
constexpr int HQ_UW = HQ_TILE + 4;          // U region (2-pixel halo)
constexpr int HQ_VW = HQ_TILE + 2;          // conv1 / LN region (1-pixel halo)
constexpr int HQ_IW = HQ_UW / 2;            // input pixels per axis
constexpr int HQ_NV = HQ_VW * HQ_VW;        // 324
constexpr int HQ_U_STRIDE = 80;             // bytes per U pixel and plane (32 halves + 16: conflict-free 16-byte reads)
constexpr int HQ_U_PLANE = HQ_UW * HQ_UW * HQ_U_STRIDE;         // 32000
constexpr int HQ_W_STRIDE = 592;            // bytes per weight row and plane (288 halves + 16)
constexpr int HQ_W_PLANE = 64 * HQ_W_STRIDE;                    // 37888
constexpr int HQ_W_OFF = 2 * HQ_U_PLANE;                        // 64000
constexpr int HQ_SMEM = HQ_W_OFF + 2 * HQ_W_PLANE;              // 139776
constexpr int HQ_V_STRIDE = 68;             // floats per V pixel (64 + 4: conflict-free 16-byte reads)
// U is split at scale 2^8: the pair is exact to 22 bits for |U| < 256 (GELU of a ConvTranspose of LayerNorm-ed, GELU-ed values:
// a few units with real and synthetic weights); rsp_split4 saturates, so a larger |U| gives a clamped finite value (up to
// 512 through the lo plane), never inf / NaN
constexpr int HQ_US = 8;
static_assert(HQ_NV * HQ_V_STRIDE * 4 <= HQ_SMEM, "the V image must fit over the U and W1 images");

struct HqP {
  const half_t* Ahi; const half_t* Alo; int64_t a_rows;   // `up` planes KB32 [2][a_rows][32], rows (s, y, x) of [n_up, 2g, 2g]
  const int* up_map; int n_up;                             // [R]: the prompt set's block of `up` (null: r)
  const float* hyper_sam; float* out_sam; int n_sam;       // optional: [R, n_sam, 32] -> out_sam[r, t] = <hyper_sam[r, t], U> + out[r]
  const half_t* W2hi; const half_t* W2lo;                  // upscale_conv2 packed [(dy, dx, c2) = 128, 64]: planes [2][128][32]
  const float* bias2;                                      // [128] (tiled x4)
  const half_t* W1hi; const half_t* W1lo;                  // mask_conv1 packed [64, (tap, ci) = 288]: planes [9][64][32]
  const float* bias1; const float* gamma; const float* beta;   // [64] each
  const float* wf;                                         // mask_conv2 as [tap][ci][c] fp32 (9 x 64 x 32)
  const float* biasf;                                      // [32]
  const float* hyper;                                      // [R, 32]
  const float* feat;                                       // [n_feat, 4g, 4g, 32]
  const int* feat_map;                                     // [R]
  float* out;                                              // [R, 4g, 4g]
  int n_feat, g2, G, tiles;                                // 2g, 4g, 4g / 16
  float alpha_u, alpha_c, eps;
};

__global__ __launch_bounds__(256) void sam_hq_mask_kernel(const HqP p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[HQ_SMEM];
  __shared__ __attribute__((aligned(16))) float sWf[580];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, l31 = lane & 31;
  const int bid = blockIdx.x;
  const int tpr = p.tiles * p.tiles;
  const int r = bid / tpr, tr = bid - r * tpr;
  const int ty = tr / p.tiles, tx = tr - ty * p.tiles;
  unsigned char* sU = smem;
  unsigned char* sW1 = smem + HQ_W_OFF;
  float* sV = reinterpret_cast<float*>(smem);

  // ---- 0. mask_conv1's weight image; the prompt set's folded 3 x 3 filter ----
  for (int u = tid; u < 2 * 9 * 64 * 4; u += 256) {          // 16-byte units of [plane][kb = tap][row][4]
    const int c = u & 3, row = (u >> 2) & 63, kb = (u >> 8) % 9, pl = u / (9 * 256);
    const half_t* src = (pl == 0 ? p.W1hi : p.W1lo) + ((kb * 64 + row) * 32 + c * 8);
    *reinterpret_cast<uint4*>(sW1 + pl * HQ_W_PLANE + row * HQ_W_STRIDE + kb * 64 + c * 16) = *reinterpret_cast<const uint4*>(src);
  }
  const float* hyp = p.hyper + (int64_t)r * 32;
  for (int idx = tid; idx < 577; idx += 256) {
    const float* w = idx < 576 ? p.wf + idx * 32 : p.biasf;
    float s = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + 4 * c4);
      const f32x4 h4 = *reinterpret_cast<const f32x4*>(hyp + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s = __builtin_fmaf(w4[e], h4[e], s);
    }
    sWf[idx] = s;
  }

  // ---- 1. U = GELU(ConvT2(up)) on the 20 x 20 region: wave w owns input pixels [32 w, 32 w + 32) of the 10 x 10 ----
  {
    const int ip = wave * 32 + l31;
    const bool have = ip < HQ_IW * HQ_IW;
    const int iy = have ? ip / HQ_IW : 0, ix = have ? ip - iy * HQ_IW : 0;
    const int Iy = (HQ_TILE / 2) * ty - 1 + iy, Ix = (HQ_TILE / 2) * tx - 1 + ix;
    const bool inside = have && Iy >= 0 && Iy < p.g2 && Ix >= 0 && Ix < p.g2;
    const int cy = Iy < 0 ? 0 : (Iy >= p.g2 ? p.g2 - 1 : Iy), cx = Ix < 0 ? 0 : (Ix >= p.g2 ? p.g2 - 1 : Ix);
    int sidx = p.up_map ? p.up_map[r] : r;
    sidx = sidx < 0 ? 0 : (sidx >= p.n_up ? p.n_up - 1 : sidx);
    const int64_t row = ((int64_t)sidx * p.g2 + cy) * p.g2 + cx;        // (outside: a valid row, the result is zeroed)
    half8_t ah[4], al[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int64_t off = ((int64_t)(s >> 1) * p.a_rows + row) * 32 + ((s & 1) * 2 + hh) * 8;
      ah[s] = *reinterpret_cast<const half8_t*>(p.Ahi + off);
      al[s] = *reinterpret_cast<const half8_t*>(p.Alo + off);
    }
    const float us = ldexpf(1.0f, HQ_US);
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                        // sub-pixel (dy, dx) = (j >> 1, j & 1)
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      const int wrow = j * 32 + l31;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int off = ((s >> 1) * 128 + wrow) * 32 + ((s & 1) * 2 + hh) * 8;
        const half8_t wh = *reinterpret_cast<const half8_t*>(p.W2hi + off);
        const half8_t wl = *reinterpret_cast<const half8_t*>(p.W2lo + off);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, ah[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, al[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, ah[s], acc, 0, 0, 0);
      }
      if (have) {
        const int pu = (2 * iy + (j >> 1)) * HQ_UW + 2 * ix + (j & 1);
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int ch = 8 * g4 + 4 * hh;
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias2 + j * 32 + ch);
          f32x4 t4, rem;
#pragma unroll
          for (int e = 0; e < 4; ++e) t4[e] = acc[4 * g4 + e] * p.alpha_u + b4[e];
          t4 = rsp_gelu4(t4);
#pragma unroll
          for (int e = 0; e < 4; ++e) t4[e] = inside ? t4[e] * us : 0.f;
          half4_t h4, l4;
          rsp_split4(t4, h4, l4, rem);
          *reinterpret_cast<half4_t*>(sU + pu * HQ_U_STRIDE + ch * 2) = h4;
          *reinterpret_cast<half4_t*>(sU + HQ_U_PLANE + pu * HQ_U_STRIDE + ch * 2) = l4;
        }
      }
    }
  }
  __syncthreads();

  // ---- 2. mask_conv1 on the 18 x 18 region: wave w owns the 32-pixel tiles w, w + 4, w + 8 (tile 11 does not exist: ----
  // ----    its lanes repeat pixel 323 and store nothing)                                                            ----
  f32x16 acc[3][2];
  int pb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int q = (wave + 4 * i) * 32 + l31;
    const int qc = q < HQ_NV ? q : HQ_NV - 1;
    const int qy = qc / HQ_VW, qx = qc - qy * HQ_VW;
    pb[i] = qy * HQ_UW + qx;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][cb][e] = 0.f;
  }
#pragma unroll 2
  for (int s = 0; s < 18; ++s) {                                         // k-step: tap s >> 1, channels [16 (s & 1) + 8 hh, + 8)
    const int tap = s >> 1, ky = tap / 3, kx = tap - 3 * ky;
    const int koff = (16 * (s & 1) + 8 * hh) * 2;                        // bytes
    half8_t wh[2], wl[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const int off = (cb * 32 + l31) * HQ_W_STRIDE + tap * 64 + koff;
      wh[cb] = *reinterpret_cast<const half8_t*>(sW1 + off);
      wl[cb] = *reinterpret_cast<const half8_t*>(sW1 + HQ_W_PLANE + off);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int off = (pb[i] + ky * HQ_UW + kx) * HQ_U_STRIDE + koff;
      const half8_t uh = *reinterpret_cast<const half8_t*>(sU + off);
      const half8_t ul = *reinterpret_cast<const half8_t*>(sU + HQ_U_PLANE + off);
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        acc[i][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[cb], uh, acc[i][cb], 0, 0, 0);
        acc[i][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[cb], ul, acc[i][cb], 0, 0, 0);
        acc[i][cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[cb], uh, acc[i][cb], 0, 0, 0);
      }
    }
  }

  // ---- (optional) SAM's own masks from the same U: <hyper_sam[r, t], U[pixel]> for the thread's output pixel, while U is in LDS ----
  float sam[3] = {0.f, 0.f, 0.f};
  if (p.n_sam > 0) {
    const int pu = ((tid >> 4) + 2) * HQ_UW + (tid & 15) + 2;
    const float* hs = p.hyper_sam + (int64_t)r * p.n_sam * 32;
#pragma unroll
    for (int c8 = 0; c8 < 4; ++c8) {
      const half8_t uh = *reinterpret_cast<const half8_t*>(sU + pu * HQ_U_STRIDE + c8 * 16);
      const half8_t ul = *reinterpret_cast<const half8_t*>(sU + HQ_U_PLANE + pu * HQ_U_STRIDE + c8 * 16);
#pragma unroll
      for (int t = 0; t < 3; ++t)
        if (t < p.n_sam) {
#pragma unroll
          for (int e = 0; e < 8; ++e) sam[t] = __builtin_fmaf((float)uh[e] + (float)ul[e], hs[t * 32 + c8 * 8 + e], sam[t]);
        }
    }
    const float inv = ldexpf(1.0f, -HQ_US);
#pragma unroll
    for (int t = 0; t < 3; ++t) sam[t] *= inv;
  }

  // ---- 3. bias, LayerNorm over the pixel's 64 channels (32 here, 32 in lane ^ 32), GELU; zero outside the image ----
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int q = (wave + 4 * i) * 32 + l31;
    const int qc = q < HQ_NV ? q : HQ_NV - 1;
    const int qy = qc / HQ_VW, qx = qc - qy * HQ_VW;
    const int Vy = HQ_TILE * ty - 1 + qy, Vx = HQ_TILE * tx - 1 + qx;
    const bool inside = Vy >= 0 && Vy < p.G && Vx >= 0 && Vx < p.G;
    float sum = 0.f;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias1 + cb * 32 + 8 * g4 + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = acc[i][cb][4 * g4 + e] * p.alpha_c + b4[e];
          acc[i][cb][4 * g4 + e] = v;
          sum += v;
        }
      }
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.0f / 64.0f);
    float sq = 0.f;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int e = 0; e < 16; ++e) { const float dl = acc[i][cb][e] - mean; sq += dl * dl; }
    sq += __shfl_xor(sq, 32, 64);
    const float rstd = 1.0f / sqrtf(sq * (1.0f / 64.0f) + p.eps);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int ch = cb * 32 + 8 * g4 + 4 * hh;
        const f32x4 ga = *reinterpret_cast<const f32x4*>(p.gamma + ch);
        const f32x4 be = *reinterpret_cast<const f32x4*>(p.beta + ch);
        f32x4 t4;
#pragma unroll
        for (int e = 0; e < 4; ++e) t4[e] = (acc[i][cb][4 * g4 + e] - mean) * rstd * ga[e] + be[e];
        t4 = rsp_gelu4(t4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][cb][4 * g4 + e] = inside ? t4[e] : 0.f;
      }
  }
  __syncthreads();                                            // everybody has read U and W1: V goes over them
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int q = (wave + 4 * i) * 32 + l31;
    if (q < HQ_NV) {
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          f32x4 t4;
#pragma unroll
          for (int e = 0; e < 4; ++e) t4[e] = acc[i][cb][4 * g4 + e];
          *reinterpret_cast<f32x4*>(sV + q * HQ_V_STRIDE + cb * 32 + 8 * g4 + 4 * hh) = t4;
        }
    }
  }
  __syncthreads();

  // ---- 4. the folded 3 x 3 filter, + <hyper, bias2> + <hyper, hq_features>: one output pixel per thread ----
  {
    const int oy = tid >> 4, ox = tid & 15;
    float s0 = sWf[576], s1 = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const float* v = sV + ((oy + tap / 3) * HQ_VW + ox + tap % 3) * HQ_V_STRIDE;
      const float* w = sWf + tap * 64;
#pragma unroll
      for (int c4 = 0; c4 < 16; c4 += 2) {
        const f32x4 va = *reinterpret_cast<const f32x4*>(v + 4 * c4), wa = *reinterpret_cast<const f32x4*>(w + 4 * c4);
        const f32x4 vb = *reinterpret_cast<const f32x4*>(v + 4 * c4 + 4), wb = *reinterpret_cast<const f32x4*>(w + 4 * c4 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s0 = __builtin_fmaf(va[e], wa[e], s0);
          s1 = __builtin_fmaf(vb[e], wb[e], s1);
        }
      }
    }
    int b = p.feat_map[r];
    b = b < 0 ? 0 : (b >= p.n_feat ? p.n_feat - 1 : b);
    const int Y = HQ_TILE * ty + oy, X = HQ_TILE * tx + ox;
    const float* f = p.feat + (((int64_t)b * p.G + Y) * p.G + X) * 32;
    float s2 = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4) {
      const f32x4 f4 = *reinterpret_cast<const f32x4*>(f + 4 * c4);
      const f32x4 h4 = *reinterpret_cast<const f32x4*>(hyp + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s2 = __builtin_fmaf(f4[e], h4[e], s2);
    }
    const float hq = (s0 + s1) + s2;
    p.out[((int64_t)r * p.G + Y) * p.G + X] = hq;
#pragma unroll
    for (int t = 0; t < 3; ++t)
      if (t < p.n_sam) p.out_sam[(((int64_t)r * p.n_sam + t) * p.G + Y) * p.G + X] = sam[t] + hq;
  }
}

}  // namespace

extern "C" int rsp_sam_hq_mask(const uint16_t* up_hi, const uint16_t* up_lo, int64_t up_rows, int32_t up_scale_log2,
                               const int32_t* up_map, int32_t n_up,
                               const uint16_t* w2_hi, const uint16_t* w2_lo, int32_t w2_scale_log2, const float* bias2,
                               const uint16_t* w1_hi, const uint16_t* w1_lo, int32_t w1_scale_log2, const float* bias1,
                               const float* gamma, const float* beta, float eps, const float* wf, const float* biasf,
                               const float* hyper, const float* feat, const int32_t* feat_map, int32_t n_feat, float* out,
                               const float* hyper_sam, float* out_sam, int32_t n_sam, int32_t R, int32_t g,
                               rsp_stream_t stream) {
  if (!up_hi || !up_lo || !w2_hi || !w2_lo || !bias2 || !w1_hi || !w1_lo || !bias1 || !gamma || !beta || !wf || !biasf ||
      !hyper || !feat || !feat_map || !out || R <= 0 || g <= 0 || (g % 4) != 0 || n_feat <= 0 || n_up <= 0 ||
      (!up_map && n_up != R) || n_sam < 0 || n_sam > 3 || (n_sam > 0 && (!hyper_sam || !out_sam)))
    return RSP_EINVAL;
  const int64_t G = 4 * (int64_t)g;
  if ((int64_t)R * G * G >= (1LL << 31) || up_rows < (int64_t)n_up * (G / 2) * (G / 2)) return RSP_EINVAL;
  HqP p;
  p.Ahi = reinterpret_cast<const half_t*>(up_hi); p.Alo = reinterpret_cast<const half_t*>(up_lo); p.a_rows = up_rows;
  p.W2hi = reinterpret_cast<const half_t*>(w2_hi); p.W2lo = reinterpret_cast<const half_t*>(w2_lo); p.bias2 = bias2;
  p.W1hi = reinterpret_cast<const half_t*>(w1_hi); p.W1lo = reinterpret_cast<const half_t*>(w1_lo); p.bias1 = bias1;
  p.gamma = gamma; p.beta = beta; p.wf = wf; p.biasf = biasf; p.hyper = hyper; p.feat = feat; p.feat_map = feat_map;
  p.up_map = up_map; p.n_up = n_up; p.hyper_sam = hyper_sam; p.out_sam = out_sam; p.n_sam = n_sam;
  p.out = out; p.n_feat = n_feat; p.g2 = 2 * g; p.G = (int)G; p.tiles = (int)(G / HQ_TILE);
  p.alpha_u = ldexpf(1.0f, -(up_scale_log2 + w2_scale_log2));
  p.alpha_c = ldexpf(1.0f, -(HQ_US + w1_scale_log2));
  p.eps = eps;
  const int64_t blocks = (int64_t)R * p.tiles * p.tiles;               // < 2^23 by the check above
  hipLaunchKernelGGL(sam_hq_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
