// PerSAM-F (Zhang et al., "Personalize Segment Anything Model with One Shot", the fine-tuned variant; persam_f.py of the
// paper's code: `Mask_Weights` = two learnable numbers, `logits_high = logits_high * weights; logits_high = logits_high.sum(0)`,
// `dice_loss = calculate_dice_loss(..); focal_loss = calculate_sigmoid_focal_loss(..); loss = dice_loss + focal_loss`,
// `optimizer = AdamW(lr=1e-3, eps=1e-4); scheduler = CosineAnnealingLR(optimizer, train_epoch)`).  There it is torch autograd
// over image-sized tensors, about twenty element-wise launches per step; here a step is ONE traversal of the three mask
// fields (mask_field.h: the values rsp_mask_post_logits(want_val) would write, never stored) that reduces the loss and the
// gradient to nine sums, and a one-wave launch that adds the block partials in block order and takes the AdamW step on the
// device.  Nothing image-sized is written, nothing is read on the host, and no floating-point atomic is used: two runs give
// the same bits.  No inline assembly.
#include "rsp_common.h"
#include "mask_field.h"

namespace {

constexpr int NSUM = 9;      // sum p, sum p t, sum focal, sum f' D_k (k = 1, 2), sum p (1 - p) D_k, sum t p (1 - p) D_k
constexpr int NSTATE = 6;    // w1, w2, AdamW's exp_avg and exp_avg_sq of both

struct FitP {
  const float* low;            // [k, 3, h, w] logits
  const uint8_t* gt;           // [k, oh, ow], non-zero = object
  MaskGeom g;
  int k;
  double* state;               // [k, NSTATE]
  unsigned long long* cnt;     // [k] = sum t (it does not change between the epochs)
  double* part;                // [k, gx, NSUM] block partials
  int gx;
  float alpha;
};

struct FitStep {
  int epoch, epochs;           // epoch < 0: evaluate only
  double lr, beta1, beta2, eps, weight_decay;
  double* out;                 // [k, 3] loss, g1, g2, or NULL
  double* history;             // [k, epochs, 3], or NULL
  float* weights;              // [k, 3] w0, w1, w2, written after the last epoch, or NULL
};

// One pixel: z = sum_k w_k F_k = F_0 + w1 D_1 + w2 D_2 in fp64 (the weights live in fp64, D_k = F_k - F_0 is exact there),
// everything after it in fp32 with the precise expf / log1pf: e = exp(-|z|) never overflows, sigmoid(|z|) = 1 / (1 + e),
// sigmoid(-|z|) = e / (1 + e) (no cancellation in 1 - p), softplus(+-z) = max(+-z, 0) + log1p(e).  The sums are fp64.
struct FitAcc {
  double s[NSUM];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < NSUM; ++j) s[j] = 0.0;
  }
  __device__ __forceinline__ void add(float f0, float f1, float f2, bool t, double w1, double w2, float alpha) {
    const double d1 = (double)f1 - (double)f0, d2 = (double)f2 - (double)f0;
    const float z = (float)((double)f0 + w1 * d1 + w2 * d2);
    const float e = expf(-fabsf(z));
    const float l = log1pf(e);
    const float big = 1.0f / (1.0f + e), small = e * big;
    const float p = z >= 0.f ? big : small, q = z >= 0.f ? small : big;          // p = sigmoid(z), q = 1 - p
    float focal, fp;
    if (t) {
      const float sp = fmaxf(-z, 0.f) + l;                                       // softplus(-z) = -log p
      focal = alpha * (sp * (q * q));
      fp = alpha * (-2.0f * (q * q) * p * sp - q * q * q);
    } else {
      const float sp = fmaxf(z, 0.f) + l;                                        // softplus(z) = -log(1 - p)
      focal = (1.0f - alpha) * (sp * (p * p));
      fp = (1.0f - alpha) * (2.0f * (p * p) * q * sp + p * p * p);
    }
    const double pq = (double)(p * q);
    s[0] += (double)p;
    s[2] += (double)focal;
    s[3] += (double)fp * d1;
    s[4] += (double)fp * d2;
    s[5] += pq * d1;
    s[6] += pq * d2;
    if (t) {
      s[1] += (double)p;
      s[7] += pq * d1;
      s[8] += pq * d2;
    }
  }
};

// every thread of the block calls this (uniform control flow): a fixed binary tree over the 256 threads in LDS, as
// locate_block_reduce (samdec.hip); one partial row per block in memory
__device__ __forceinline__ void fit_block_reduce(const FitAcc& a, const FitP& q, int m) {
  __shared__ double sS[NSUM][MASK_BLOCK];
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < NSUM; ++j) sS[j][t] = a.s[j];
  __syncthreads();
  for (int d = MASK_BLOCK / 2; d >= 1; d >>= 1) {
    if (t < d) {
#pragma unroll
      for (int j = 0; j < NSUM; ++j) sS[j][t] = sS[j][t] + sS[j][t + d];
    }
    __syncthreads();
  }
  if (t < NSUM) q.part[((int64_t)m * q.gx + blockIdx.x) * NSUM + t] = sS[t][0];
}

template <bool IDENT>
__global__ __launch_bounds__(256) void persam_f_sums_kernel(const FitP q) {
  const int m = blockIdx.y;
  const int64_t hw = (int64_t)q.g.h * q.g.w;
  const float* low0 = q.low + (int64_t)m * 3 * hw;
  const float *low1 = low0 + hw, *low2 = low1 + hw;
  const uint8_t* gt = q.gt + (int64_t)m * q.g.oh * q.g.ow;
  const double w1 = q.state[(int64_t)m * NSTATE], w2 = q.state[(int64_t)m * NSTATE + 1];
  const MaskScales sc = mask_scales(q.g);
  FitAcc a;
  a.clear();
  mask_each_pixel(low0, q.g, IDENT, [&](float v0, int oy, int ox, int64_t i) {
    a.add(v0, mask_pixel<IDENT>(low1, q.g, sc, oy, ox), mask_pixel<IDENT>(low2, q.g, sc, oy, ox), gt[i] != 0, w1, w2, q.alpha);
  });
  fit_block_reduce(a, q, m);
}

// MASK_STRIP: a thread owns FIT_ROWS rows of one column quad; the second and third field walk down the same rows in strips
// of their own (MaskStrip: the expression tree of mask_stage1, the same bits as the pixel form)
constexpr int FIT_ROWS = 8;
__global__ __launch_bounds__(256) void persam_f_sums_strip_kernel(const FitP q) {
  const int m = blockIdx.y;
  const int64_t hw = (int64_t)q.g.h * q.g.w;
  const float* low0 = q.low + (int64_t)m * 3 * hw;
  const float *low1 = low0 + hw, *low2 = low1 + hw;
  const uint8_t* gt = q.gt + (int64_t)m * q.g.oh * q.g.ow;
  const double w1 = q.state[(int64_t)m * NSTATE], w2 = q.state[(int64_t)m * NSTATE + 1];
  const MaskScales sc = mask_scales(q.g);
  FitAcc a;
  a.clear();
  MaskStrip s1, s2;
  int sx = -1;
  mask_each_strip<FIT_ROWS, true>(low0, q.g, [&](const float v0[4], int oy, int ox) {
    if (ox != sx) { s1.init(q.g, sc, ox); s2.init(q.g, sc, ox); sx = ox; }
    float v1[4], v2[4];
    s1.row(low1, q.g, sc, oy, v1);
    s2.row(low2, q.g, sc, oy, v2);
    const uint8_t* t = gt + (int64_t)oy * q.g.ow + ox;
#pragma unroll
    for (int e = 0; e < 4; ++e) a.add(v0[e], v1[e], v2[e], t[e] != 0, w1, w2, q.alpha);
  });
  fit_block_reduce(a, q, m);
}

// state = (w1, w2, 0, 0, 0, 0), sum t = 0.  `weights` [k, 2] or NULL: fp32 1 / 3, the start of the fit
__global__ __launch_bounds__(256) void persam_f_init_kernel(const FitP q, const float* __restrict__ weights) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= q.k) return;
  double* st = q.state + (int64_t)m * NSTATE;
  st[0] = (double)(weights ? weights[m * 2] : 1.0f / 3.0f);
  st[1] = (double)(weights ? weights[m * 2 + 1] : 1.0f / 3.0f);
#pragma unroll
  for (int j = 2; j < NSTATE; ++j) st[j] = 0.0;
  q.cnt[m] = 0ull;
}

// sum t: integer, so one atomic per block
__global__ __launch_bounds__(256) void persam_f_count_kernel(const FitP q) {
  __shared__ int sN[MASK_BLOCK];
  const int m = blockIdx.y;
  const int64_t total = (int64_t)q.g.oh * q.g.ow;
  const uint8_t* gt = q.gt + (int64_t)m * total;
  int n = 0;
  for (int64_t i = (int64_t)blockIdx.x * MASK_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MASK_BLOCK) n += gt[i] != 0 ? 1 : 0;
  const int t = threadIdx.x;
  sN[t] = n;
  __syncthreads();
  for (int d = MASK_BLOCK / 2; d >= 1; d >>= 1) {
    if (t < d) sN[t] += sN[t + d];
    __syncthreads();
  }
  if (t == 0 && sN[0]) atomicAdd(q.cnt + m, (unsigned long long)sN[0]);
}

// One wave per problem: lane j < 9 adds sum j over the blocks in block order; lane 0 forms the loss and the gradient
//   dice = 1 - Nn / Dn, Nn = 2 sum p t + 1, Dn = sum p + sum t + 1;  focal = sum focal / HW
//   g_k = sum f' D_k / HW - (2 sum t p (1 - p) D_k Dn - Nn sum p (1 - p) D_k) / Dn^2
// and, in a fit, takes torch.optim.AdamW's step (decoupled decay, exp_avg.lerp_, bias corrections by beta^step,
// denom = sqrt(v) / sqrt(bc2) + eps) at CosineAnnealingLR's rate lr / 2 (1 + cos(pi e / epochs)), all in fp64.
__global__ __launch_bounds__(64) void persam_f_step_kernel(const FitP q, const FitStep u) {
  __shared__ double tot[NSUM];
  const int m = blockIdx.x, j = threadIdx.x;
  if (j < NSUM) {
    const double* pp = q.part + (int64_t)m * q.gx * NSUM + j;
    double s = 0.0;
    for (int b = 0; b < q.gx; ++b) s += pp[(int64_t)b * NSUM];
    tot[j] = s;
  }
  __syncthreads();
  if (j != 0) return;
  const double n = (double)q.g.oh * (double)q.g.ow;
  const double Dn = tot[0] + (double)q.cnt[m] + 1.0, Nn = 2.0 * tot[1] + 1.0;
  const double loss = (1.0 - Nn / Dn) + tot[2] / n;
  double g[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) g[c] = tot[3 + c] / n - (2.0 * tot[7 + c] * Dn - Nn * tot[5 + c]) / (Dn * Dn);
  if (u.out) { u.out[m * 3] = loss; u.out[m * 3 + 1] = g[0]; u.out[m * 3 + 2] = g[1]; }
  if (u.epoch < 0) return;
  if (u.history) {
    double* hh = u.history + ((int64_t)m * u.epochs + u.epoch) * 3;
    hh[0] = loss; hh[1] = g[0]; hh[2] = g[1];
  }
  double* st = q.state + (int64_t)m * NSTATE;
  const double lr = u.lr * 0.5 * (1.0 + cos(3.14159265358979323846 * (double)u.epoch / (double)u.epochs));
  const double step = (double)(u.epoch + 1);
  const double bc1 = 1.0 - pow(u.beta1, step), bc2 = 1.0 - pow(u.beta2, step);
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    double w = st[c], ma = st[2 + c], va = st[4 + c];
    w = w * (1.0 - lr * u.weight_decay);
    ma = ma + (g[c] - ma) * (1.0 - u.beta1);
    va = va * u.beta2 + (1.0 - u.beta2) * g[c] * g[c];
    const double denom = sqrt(va) / sqrt(bc2) + u.eps;
    w = w - (lr / bc1) * (ma / denom);
    st[c] = w; st[2 + c] = ma; st[4 + c] = va;
  }
  if (u.weights && u.epoch == u.epochs - 1) {
    u.weights[m * 3] = (float)(1.0 - st[0] - st[1]);
    u.weights[m * 3 + 1] = (float)st[0];
    u.weights[m * 3 + 2] = (float)st[1];
  }
}

unsigned fit_blocks(int64_t n, int64_t cap) {
  const int64_t b = (n + MASK_BLOCK - 1) / MASK_BLOCK;
  return (unsigned)(b > cap ? cap : b);
}
// blocks per problem of the traversal (also the number of partial rows per problem in the workspace)
int fit_gx(int out_h, int out_w, bool strip) {
  return (int)(strip ? fit_blocks(mask_strip_items(out_h, out_w, FIT_ROWS), 0x7fffffffLL) : fit_blocks((int64_t)out_h * out_w, 256));
}

bool fit_args_ok(const void* low_res, const void* gt, int32_t k, const MaskGeom& g, const void* workspace, int64_t workspace_bytes,
                 int32_t epochs) {
  if (!low_res || !gt || !workspace || k < 1 || epochs < 1 || !mask_geom_valid(g)) return false;
  return workspace_bytes >= rsp_persam_f_workspace_bytes(k, g.oh, g.ow, epochs) && !((uintptr_t)workspace & 7);
}

FitP fit_params(const float* low_res, const uint8_t* gt, int32_t k, const MaskGeom& g, void* workspace, float alpha) {
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(workspace);
  double* state = reinterpret_cast<double*>(cnt + k);
  return FitP{low_res, gt, g, k, state, cnt, state + (int64_t)k * NSTATE, fit_gx(g.oh, g.ow, mask_form(g) == MASK_STRIP), alpha};
}

void launch_fit_init(const FitP& q, const float* weights, hipStream_t st) {
  hipLaunchKernelGGL(persam_f_init_kernel, dim3(fit_blocks(q.k, 0x7fffffffLL)), dim3(256), 0, st, q, weights);
  const unsigned gc = fit_blocks((int64_t)q.g.oh * q.g.ow, 256);
  for_mask_chunks(q.k, [&](int32_t m0, int32_t km) {
    FitP c = q;
    c.gt += (int64_t)m0 * q.g.oh * q.g.ow;
    c.cnt += m0;
    hipLaunchKernelGGL(persam_f_count_kernel, dim3(gc, km), dim3(MASK_BLOCK), 0, st, c);
  });
}

// one evaluation at the weights in `state`, then the step (or only the loss and gradient) of every problem
void launch_fit_epoch(const FitP& q, const FitStep& u, hipStream_t st) {
  const MaskForm form = mask_form(q.g);
  for_mask_chunks(q.k, [&](int32_t m0, int32_t km) {
    FitP c = q;
    c.low += (int64_t)m0 * 3 * q.g.h * q.g.w;
    c.gt += (int64_t)m0 * q.g.oh * q.g.ow;
    c.state += (int64_t)m0 * NSTATE;
    c.part += (int64_t)m0 * q.gx * NSUM;
    switch (form) {
      case MASK_STRIP: hipLaunchKernelGGL(persam_f_sums_strip_kernel, dim3((unsigned)q.gx, km), dim3(MASK_BLOCK), 0, st, c); break;
      case MASK_IDENT: hipLaunchKernelGGL((persam_f_sums_kernel<true>), dim3((unsigned)q.gx, km), dim3(MASK_BLOCK), 0, st, c); break;
      case MASK_GENERIC: hipLaunchKernelGGL((persam_f_sums_kernel<false>), dim3((unsigned)q.gx, km), dim3(MASK_BLOCK), 0, st, c); break;
    }
  });
  hipLaunchKernelGGL(persam_f_step_kernel, dim3((unsigned)q.k), dim3(64), 0, st, q, u);
}

}  // namespace

extern "C" int64_t rsp_persam_f_workspace_bytes(int32_t k, int32_t out_h, int32_t out_w, int32_t epochs) {
  if (k < 1 || epochs < 1 || out_h <= 0 || out_w <= 0 || (int64_t)out_h * out_w > 0x7fffffffLL) return -1;
  const int gs = fit_gx(out_h, out_w, true), gg = fit_gx(out_h, out_w, false);
  return (int64_t)k * 8 * (1 + NSTATE + (int64_t)NSUM * (gs > gg ? gs : gg));
}

extern "C" int rsp_persam_f_loss_grad(const float* low_res, const uint8_t* gt, int32_t k, int32_t h, int32_t w, int32_t Hb,
                                      int32_t Wb, int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w,
                                      const float* weights, float alpha, void* workspace, int64_t workspace_bytes, double* out,
                                      rsp_stream_t stream) {
  const MaskGeom g{h, w, Hb, Wb, crop_h, crop_w, out_h, out_w};
  if (!weights || !out || !fit_args_ok(low_res, gt, k, g, workspace, workspace_bytes, 1)) return RSP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const FitP q = fit_params(low_res, gt, k, g, workspace, alpha);
  launch_fit_init(q, weights, st);
  launch_fit_epoch(q, FitStep{-1, 1, 0.0, 0.0, 0.0, 0.0, 0.0, out, nullptr, nullptr}, st);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_persam_f_fit(const float* low_res, const uint8_t* gt, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb,
                                int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w, int32_t epochs, double lr,
                                double beta1, double beta2, double eps, double weight_decay, float alpha, void* workspace,
                                int64_t workspace_bytes, float* weights, double* history, rsp_stream_t stream) {
  const MaskGeom g{h, w, Hb, Wb, crop_h, crop_w, out_h, out_w};
  if (!weights || !fit_args_ok(low_res, gt, k, g, workspace, workspace_bytes, epochs)) return RSP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const FitP q = fit_params(low_res, gt, k, g, workspace, alpha);
  launch_fit_init(q, nullptr, st);
  // the whole fit is enqueued here: the launches of an epoch follow each other in stream order, nothing waits on the host
  for (int e = 0; e < epochs; ++e)
    launch_fit_epoch(q, FitStep{e, epochs, lr, beta1, beta2, eps, weight_decay, nullptr, history, weights}, st);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
