// PerSAM (Zhang et al., "Personalize Segment Anything Model with One Shot"), the training-free variant: the two reductions over
// image embeddings that precede SAM's decoder there (persam.py of the paper's code: `target_feat = ref_feat[ref_mask > 0]`,
// its mean and L2-normalised mean; `sim = target_feat @ (test_feat / test_feat.norm(dim=0))`, then
// F.interpolate(scale_factor=4, mode='bilinear')).  The embeddings are the encoder's channels-last rows [B * N, 256]: a key is
// one 1 KiB row, read once.  The location prior itself (extrema, statistics, attn_sim of the image-resolution field) is
// rsp_persam_locate in samdec.hip, next to the mask kernels whose device functions it shares.  No inline assembly.
#include "rsp_common.h"
#include "mask_field.h"

namespace {

constexpr int C = 256;          // SAM's embedding width

// Mean of the selected rows and its unit vector.  One block: thread = (row group 0..3, channel); the four partial sums of a
// channel are added in a fixed order, so the result does not depend on scheduling.  count == 0: zeros (the caller refuses).
__global__ __launch_bounds__(1024) void persam_target_kernel(const float* __restrict__ emb, const uint8_t* __restrict__ cell, int N,
                                                             float* __restrict__ te, float* __restrict__ tf,
                                                             int32_t* __restrict__ count) {
  __shared__ float sA[4][C];
  __shared__ int sN[4];
  __shared__ float sW[4];
  const int tid = threadIdx.x, c = tid & (C - 1), grp = tid >> 8;
  float a = 0.f;
  int n = 0;
  for (int row = grp; row < N; row += 4) {
    if (cell[row]) { a += emb[(int64_t)row * C + c]; ++n; }
  }
  sA[grp][c] = a;
  if (c == 0) sN[grp] = n;
  __syncthreads();
  const int cnt = sN[0] + sN[1] + sN[2] + sN[3];
  const float mean = cnt > 0 ? ((sA[0][c] + sA[1][c]) + (sA[2][c] + sA[3][c])) / (float)cnt : 0.f;
  const float sq = rsp_wave_sum(grp == 0 ? mean * mean : 0.f);        // waves 0..3 hold group 0's 256 channels
  if (grp == 0 && (tid & 63) == 0) sW[tid >> 6] = sq;
  __syncthreads();
  if (grp == 0) {
    const float nrm = sqrtf((sW[0] + sW[1]) + (sW[2] + sW[3]));
    te[c] = mean;
    tf[c] = nrm > 0.f ? mean / nrm : 0.f;
    if (c == 0) *count = cnt;
  }
}

// sim[row] = <tf, emb[row] / |emb[row]|>: one wave per key, a lane owns 4 of the 256 channels; dot product and squared norm
// in the same pass, both wave-reduced.  A zero row scores 0 (PerSAM would divide by zero).
__global__ __launch_bounds__(256) void persam_similarity_kernel(const float* __restrict__ emb, const float* __restrict__ tf,
                                                                int64_t rows, float* __restrict__ sim) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                              // whole waves leave together
  const f32x4 t = *reinterpret_cast<const f32x4*>(tf + lane * 4);
  const f32x4 e = *reinterpret_cast<const f32x4*>(emb + row * C + lane * 4);
  float d = (t[0] * e[0] + t[1] * e[1]) + (t[2] * e[2] + t[3] * e[3]);
  float q = (e[0] * e[0] + e[1] * e[1]) + (e[2] * e[2] + e[3] * e[3]);
  d = rsp_wave_sum(d);
  q = rsp_wave_sum(q);
  if (lane == 0) sim[row] = q > 0.f ? d / sqrtf(q) : 0.f;
}

// torch upsample_bilinear2d(align_corners=False, scale_factor=4): sim [B, gh, gw] -> low [B, 4 gh, 4 gw]
__global__ __launch_bounds__(256) void persam_up4_kernel(const float* __restrict__ sim, float* __restrict__ low, int gh, int gw) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int oh = 4 * gh, ow = 4 * gw;
  if (i >= oh * ow) return;
  const int oy = i / ow, ox = i - oy * ow;
  const Lin cy = lin_coef(oy, 0.25f, gh), cx = lin_coef(ox, 0.25f, gw);
  const float* s = sim + (int64_t)b * gh * gw;
  low[(int64_t)b * oh * ow + i] = cy.l0 * (cx.l0 * s[cy.i0 * gw + cx.i0] + cx.l1 * s[cy.i0 * gw + cx.i1]) +
                                  cy.l1 * (cx.l0 * s[cy.i1 * gw + cx.i0] + cx.l1 * s[cy.i1 * gw + cx.i1]);
}

}  // namespace

extern "C" int rsp_persam_target(const float* emb, const uint8_t* cell_mask, int32_t N, float* target_embedding,
                                 float* target_feature, int32_t* count, rsp_stream_t stream) {
  if (!emb || !cell_mask || !target_embedding || !target_feature || !count || N <= 0) return RSP_EINVAL;
  hipLaunchKernelGGL(persam_target_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, emb, cell_mask, N, target_embedding,
                     target_feature, count);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_persam_similarity(const float* emb, const float* target_feature, int32_t B, int32_t gh, int32_t gw, float* sim,
                                     float* low_res, rsp_stream_t stream) {
  if (!emb || !target_feature || !sim || !low_res || B < 0 || B > 65535 || gh <= 0 || gw <= 0 || (int64_t)gh * gw > (1 << 24))
    return RSP_EINVAL;
  if (B == 0) return RSP_OK;
  if (((uintptr_t)emb | (uintptr_t)target_feature) & 15) return RSP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * gh * gw;
  hipLaunchKernelGGL(persam_similarity_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, emb, target_feature, rows, sim);
  hipLaunchKernelGGL(persam_up4_kernel, dim3((unsigned)((16 * gh * gw + 255) / 256), B), dim3(256), 0, st, sim, low_res, gh, gw);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
