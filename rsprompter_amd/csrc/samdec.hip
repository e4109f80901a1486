// SAM mask-decoder tail + mask post-processing (HBM-bound kernels).
//   hyper-network mask product  HF:523-531  (masks = hyper_in @ upscaled_embedding; only mask
//                               token 0 is kept because multimask_output=False, HF:537-542)
//   mask post-process           models.py:1746-1784 (sigmoid -> bilinear to batch_input_shape ->
//                               crop -> bilinear to ori_shape -> >= thr)
#include "rsp_common.h"
#include "mask_field.h"

namespace {

// out[r, pix] = sum_c up[r, pix, c] * hyper[r, c];  8 lanes per pixel (C == 32: one float4 each)
__global__ __launch_bounds__(256) void hyper_mask_kernel(const float* __restrict__ up,
                                                         const float* __restrict__ hyper,
                                                         float* __restrict__ out, int npix, int C) {
  const int r = blockIdx.y;
  const int part = threadIdx.x & 7;
  const float* hv = hyper + (int64_t)r * C;
  const float* ur = up + (int64_t)r * npix * C;
  for (int pix = blockIdx.x * 32 + (threadIdx.x >> 3); pix < npix; pix += gridDim.x * 32) {
    float acc = 0.f;
    for (int c = part * 4; c < C; c += 32) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(ur + (int64_t)pix * C + c);
      const f32x4 h = *reinterpret_cast<const f32x4*>(hv + c);
      acc += u[0] * h[0] + u[1] * h[1] + u[2] * h[2] + u[3] * h[3];
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (part == 0) out[(int64_t)r * npix + pix] = acc;
  }
}

struct MaskPostP {
  const float* low;   // [k, h, w] logits
  uint8_t* out;       // [k, oh, ow] bool
  float* prob;        // optional [k, oh, ow]
  int k;
  MaskGeom g;
  float thr;
  int strict;         // 1: value > thr (SAMDet, models.py:1206), 0: value >= thr (models.py:1779)
};

__global__ __launch_bounds__(256) void sigmoid_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = 1.0f / (1.0f + expf(-x[i]));
}

__device__ __forceinline__ bool mask_post_test(const MaskPostP& p, float v) { return p.strict ? v > p.thr : v >= p.thr; }
// four pixels of one row: one 32-bit store of the bool mask instead of four byte stores
__device__ __forceinline__ void mask_post_store4(const MaskPostP& p, int64_t o, const float v[4]) {
  uint32_t bits = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) bits |= (mask_post_test(p, v[e]) ? 1u : 0u) << (8 * e);
  *reinterpret_cast<uint32_t*>(p.out + o) = bits;
  if (p.prob) *reinterpret_cast<f32x4*>(p.prob + o) = f32x4{v[0], v[1], v[2], v[3]};
}

// `sig` = sigmoid(low-res logits) (models.py:1758)
template <bool IDENT>
__global__ __launch_bounds__(256) void mask_post_kernel(const MaskPostP p) {
  const int m = blockIdx.y;
  const float* low = p.low + (int64_t)m * p.g.h * p.g.w;
  const int64_t base = (int64_t)m * p.g.oh * p.g.ow;
  if ((p.g.ow & 3) == 0) {
    mask_each_quad<IDENT>(low, p.g,
                          [&](const float v[4], int oy, int ox) { mask_post_store4(p, base + (int64_t)oy * p.g.ow + ox, v); });
    return;
  }
  mask_each_pixel(low, p.g, IDENT, [&](float v, int, int, int64_t i) {
    const int64_t o = base + i;
    p.out[o] = mask_post_test(p, v) ? 1 : 0;
    if (p.prob) p.prob[o] = v;
  });
}

// MASK_STRIP (every 1024-px tile); the generic kernel spends ~40 VALU instructions and four gathers per pixel on it
// (1.3 ms per ViT-H step for 838 MB of masks).
constexpr int MP_ROWS = 16;
__global__ __launch_bounds__(256) void mask_post_strip_kernel(const MaskPostP p) {
  const int m = blockIdx.y;
  const int64_t base = (int64_t)m * p.g.oh * p.g.ow;
  mask_each_strip<MP_ROWS, true>(p.low + (int64_t)m * p.g.h * p.g.w, p.g,
                           [&](const float v[4], int oy, int ox) { mask_post_store4(p, base + (int64_t)oy * p.g.ow + ox, v); });
}

// Scores of K candidate masks without the masks (HF mask generation: _compute_stability_score + _batched_mask_to_box of
// image_processing_sam over post_process_masks): per mask the number of pixels of its field that are > t_hi, > t_lo and
// > t_mid, and the extents of the pixels > t_mid.  acc[m] = {n_hi, n_lo, n_mid, min x, min y, max x, max y}; integer sums and
// extrema only, so the result does not depend on the order in which blocks arrive.  Nothing of size K * oh * ow is written.
struct ScoreThr { float t_hi, t_lo, t_mid; };
struct MaskScoreP {
  const float* low;     // [k, h, w] logits
  MaskGeom g;
  int32_t* acc;         // [k, 7]
  ScoreThr t;
};

struct ScoreAcc {
  int n_hi, n_lo, n_mid, x0, y0, x1, y1;
  __device__ __forceinline__ void clear() { n_hi = n_lo = n_mid = 0; x0 = y0 = 0x7fffffff; x1 = y1 = -1; }
  __device__ __forceinline__ void add(const ScoreThr& t, float v, int oy, int ox) {
    n_hi += v > t.t_hi ? 1 : 0;
    n_lo += v > t.t_lo ? 1 : 0;
    if (v > t.t_mid) {
      n_mid += 1;
      x0 = min(x0, ox); x1 = max(x1, ox);
      y0 = min(y0, oy); y1 = max(y1, oy);
    }
  }
  __device__ __forceinline__ void add4(const ScoreThr& t, const float v[4], int oy, int ox) {
#pragma unroll
    for (int e = 0; e < 4; ++e) add(t, v[e], oy, ox + e);
  }
};

// every thread of the block calls this (uniform control flow): wave shuffles, 4 partial rows in LDS, one atomic per value
__device__ __forceinline__ void score_block_reduce(ScoreAcc a, int32_t* __restrict__ acc) {
  __shared__ int part[4][7];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    a.n_hi += __shfl_xor(a.n_hi, d, 64);
    a.n_lo += __shfl_xor(a.n_lo, d, 64);
    a.n_mid += __shfl_xor(a.n_mid, d, 64);
    a.x0 = min(a.x0, __shfl_xor(a.x0, d, 64));
    a.y0 = min(a.y0, __shfl_xor(a.y0, d, 64));
    a.x1 = max(a.x1, __shfl_xor(a.x1, d, 64));
    a.y1 = max(a.y1, __shfl_xor(a.y1, d, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[wave][0] = a.n_hi; part[wave][1] = a.n_lo; part[wave][2] = a.n_mid;
    part[wave][3] = a.x0; part[wave][4] = a.y0; part[wave][5] = a.x1; part[wave][6] = a.y1;
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < 7) {
    const int v0 = part[0][j], v1 = part[1][j], v2 = part[2][j], v3 = part[3][j];
    if (j < 3) {
      const int sum = v0 + v1 + v2 + v3;
      if (sum) atomicAdd(acc + j, sum);
    } else if (j < 5) {
      atomicMin(acc + j, min(min(v0, v1), min(v2, v3)));
    } else {
      atomicMax(acc + j, max(max(v0, v1), max(v2, v3)));
    }
  }
}

template <bool IDENT>
__global__ __launch_bounds__(256) void mask_score_kernel(const MaskScoreP q) {
  const int m = blockIdx.y;
  ScoreAcc a;
  a.clear();
  mask_each_pixel(q.low + (int64_t)m * q.g.h * q.g.w, q.g, IDENT, [&](float v, int oy, int ox, int64_t) { a.add(q.t, v, oy, ox); });
  score_block_reduce(a, q.acc + (int64_t)m * 7);
}

constexpr int MS_ROWS = 64;
__global__ __launch_bounds__(256) void mask_score_strip_kernel(const MaskScoreP q) {
  const int m = blockIdx.y;
  ScoreAcc a;
  a.clear();
  mask_each_strip<MS_ROWS, true>(q.low + (int64_t)m * q.g.h * q.g.w, q.g,
                                 [&](const float v[4], int oy, int ox) { a.add4(q.t, v, oy, ox); });
  score_block_reduce(a, q.acc + (int64_t)m * 7);
}

// rows of W = 7 (rsp_mask_score_box) or 8 (rsp_mask_score_box_crops: + the near-edge flag) accumulators
template <int W>
__global__ __launch_bounds__(256) void mask_score_init_kernel(int32_t* __restrict__ acc, int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k * W) return;
  const int j = i % W;
  acc[i] = j < 3 ? 0 : (j < 5 ? 0x7fffffff : (j < 7 ? -1 : 0));
}

// an empty mask gets the box [0, 0, 0, 0] (HF _batched_mask_to_box)
__global__ __launch_bounds__(256) void mask_score_final_kernel(int32_t* __restrict__ acc, int k) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= k) return;
  if (acc[m * 7 + 2] == 0) {
#pragma unroll
    for (int j = 3; j < 7; ++j) acc[m * 7 + j] = 0;
  }
}

// The same scores for candidates of SEVERAL crops in one launch (SAM's crop layers): candidate m belongs to crop
// crop_idx[m], and row crop_idx[m] of a device table holds that crop's geometry (Hb, Wb, crop_h, crop_w, out_h, out_w), its box
// in the image (x0, y0, x1, y1) and the image size (W, H).  A block works on ONE candidate, so the table row is wave-uniform
// (scalar loads) and mask_form() is evaluated per crop: counts and crop-local box are those of rsp_mask_score_box on that
// crop's slice.  acc is [k, 8]: the finalising launch shifts the box into the image frame and writes HF's
// _is_box_near_crop_edge into column 7.
constexpr int CROP_ROW = RSP_CROP_TABLE_COLS;
constexpr int CROP_EDGE_ATOL = 20;      // _is_box_near_crop_edge(atol=20.0); every quantity is an integer
struct MaskScoreCropsP {
  const float* low;          // [k, h, w]
  const int32_t* crop_idx;   // [k]
  const int32_t* table;      // [n_crops, CROP_ROW]
  int32_t* acc;              // [k, 8]
  int k, h, w, n_crops;
  ScoreThr t;
};

__global__ __launch_bounds__(256) void mask_score_crops_kernel(const MaskScoreCropsP c) {
  const int m = blockIdx.y;
  const int32_t* t = c.table + CROP_ROW * min(max(c.crop_idx[m], 0), c.n_crops - 1);   // clamped: never outside the table
  const MaskGeom g{c.h, c.w, t[0], t[1], t[2], t[3], t[4], t[5]};
  const float* low = c.low + (int64_t)m * c.h * c.w;
  ScoreAcc a;
  a.clear();
  // a row the host would have refused scores as an empty mask (no traversal)
  if (mask_table_row_ok(g)) {
    const MaskForm form = mask_form(g);
    if (form == MASK_STRIP)
      mask_each_strip<MS_ROWS, false>(low, g, [&](const float v[4], int oy, int ox) { a.add4(c.t, v, oy, ox); });
    else
      mask_each_pixel(low, g, form == MASK_IDENT, [&](float v, int oy, int ox, int64_t) { a.add(c.t, v, oy, ox); });
  }
  score_block_reduce(a, c.acc + (int64_t)m * 8);
}

// the empty-mask box [0, 0, 0, 0] (crop-local, shifted like any other), the shift by (x0, y0, x0, y0) and the near-edge flag:
// a coordinate hits when it is within 20 of the crop box's and not within 20 of [0, 0, W, H]'s
__global__ __launch_bounds__(256) void mask_score_crops_final_kernel(int32_t* __restrict__ acc, const int32_t* __restrict__ crop_idx,
                                                                     const int32_t* __restrict__ table, int k, int n_crops) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= k) return;
  const int32_t* t = table + CROP_ROW * min(max(crop_idx[m], 0), n_crops - 1);
  const int cb[4] = {t[6], t[7], t[8], t[9]}, ob[4] = {0, 0, t[10], t[11]};
  const bool empty = acc[m * 8 + 2] == 0;
  int flag = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int v = (empty ? 0 : acc[m * 8 + 3 + j]) + cb[j & 1];
    flag |= (abs(v - cb[j]) <= CROP_EDGE_ATOL && abs(v - ob[j]) > CROP_EDGE_ATOL) ? 1 : 0;
    acc[m * 8 + 3 + j] = v;
  }
  acc[m * 8 + 7] = flag;
}

// PerSAM's location prior (rsp_persam_locate; PerSAM persam.py `point_selection` + the normalisation of the similarity in
// front of `attn_sim`): the extrema of the IMAGE-RESOLUTION field with their positions, its mean and unbiased standard
// deviation, and the g x g resampling of the normalised field.  The field itself is never written.
//   extrema   one 64-bit integer atomic per block on a packed key (order-preserving image of the value << 32 | index): the
//             maximum carries ~index, the minimum index, so that among equal values the LOWEST flat index y * ow + x wins
//             either way (torch.argmax / argmin of the flattened field; a plateau at the extreme is the normal case for a
//             bilinear up-sampling with clamped borders).  -0 counts as +0, as it does for torch.
//   sums      fp64, of v - K with K the image's first logit (a constant field sums exact zeros), per thread, then a fixed
//             tree per block, one partial pair per block in memory, added in block order by the finalising launch: no
//             floating-point atomic, so two runs give the same bits.
struct LocateP {
  const float* low;            // [k, h, w] logits
  MaskGeom g;
  int k;
  unsigned long long* keys;    // [k, 2] packed maximum, minimum
  double* part;                // [k, gx, 2] sum, sum of squares of (v - K) per block
  int gx;
};

__device__ __forceinline__ uint32_t locate_ord(float v) {
  const uint32_t u = __float_as_uint(v + 0.0f);           // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float locate_unord(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

struct LocateAcc {
  unsigned long long kmax, kmin;
  double s, ss;
  __device__ __forceinline__ void clear() { kmax = 0ull; kmin = ~0ull; s = 0.0; ss = 0.0; }
  __device__ __forceinline__ void add(float v, int idx, float K) {
    const unsigned long long o = (unsigned long long)locate_ord(v) << 32;
    const unsigned long long a = o | (unsigned long long)(0xffffffffu - (uint32_t)idx), b = o | (unsigned long long)(uint32_t)idx;
    kmax = a > kmax ? a : kmax;
    kmin = b < kmin ? b : kmin;
    const double d = (double)v - (double)K;
    s += d;
    ss += d * d;
  }
};

// every thread of the block calls this (uniform control flow): a fixed binary tree over the 256 threads in LDS
__device__ __forceinline__ void locate_block_reduce(LocateAcc a, const LocateP& q, int m) {
  __shared__ unsigned long long sMax[256], sMin[256];
  __shared__ double sS[256], sQ[256];
  const int t = threadIdx.x;
  sMax[t] = a.kmax; sMin[t] = a.kmin; sS[t] = a.s; sQ[t] = a.ss;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (t < d) {
      sMax[t] = sMax[t + d] > sMax[t] ? sMax[t + d] : sMax[t];
      sMin[t] = sMin[t + d] < sMin[t] ? sMin[t + d] : sMin[t];
      sS[t] = sS[t] + sS[t + d];
      sQ[t] = sQ[t] + sQ[t + d];
    }
    __syncthreads();
  }
  if (t == 0) {
    atomicMax(q.keys + (int64_t)m * 2, sMax[0]);
    atomicMin(q.keys + (int64_t)m * 2 + 1, sMin[0]);
    double* pp = q.part + ((int64_t)m * q.gx + blockIdx.x) * 2;
    pp[0] = sS[0]; pp[1] = sQ[0];
  }
}

template <bool IDENT>
__global__ __launch_bounds__(256) void persam_locate_kernel(const LocateP q) {
  const int m = blockIdx.y;
  const float* low = q.low + (int64_t)m * q.g.h * q.g.w;
  const float K = low[0];
  LocateAcc a;
  a.clear();
  mask_each_pixel(low, q.g, IDENT, [&](float v, int, int, int64_t i) { a.add(v, (int)i, K); });
  locate_block_reduce(a, q, m);
}

constexpr int LOC_ROWS = 16;
__global__ __launch_bounds__(256) void persam_locate_strip_kernel(const LocateP q) {
  const int m = blockIdx.y;
  const float* low = q.low + (int64_t)m * q.g.h * q.g.w;
  const float K = low[0];
  LocateAcc a;
  a.clear();
  mask_each_strip<LOC_ROWS, true>(low, q.g, [&](const float v[4], int oy, int ox) {
#pragma unroll
    for (int e = 0; e < 4; ++e) a.add(v[e], oy * q.g.ow + ox + e, K);
  });
  locate_block_reduce(a, q, m);
}

__global__ __launch_bounds__(256) void persam_locate_init_kernel(unsigned long long* __restrict__ keys, int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k * 2) keys[i] = (i & 1) ? ~0ull : 0ull;
}

// one thread per image: the block partials in block order, then stats = {max, min, mean, std}, xy = {x+, y+, x-, y-, pixels}.
// std is torch.std's (unbiased); a constant field (max == min) has std 0 exactly, as has a field of one pixel.
__global__ __launch_bounds__(64) void persam_locate_final_kernel(const LocateP q, float* __restrict__ stats, int32_t* __restrict__ xy) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= q.k) return;
  const double* pp = q.part + (int64_t)m * q.gx * 2;
  double s = 0.0, ss = 0.0;
  for (int b = 0; b < q.gx; ++b) { s += pp[2 * b]; ss += pp[2 * b + 1]; }
  const double n = (double)q.g.oh * (double)q.g.ow;
  const double K = (double)q.low[(int64_t)m * q.g.h * q.g.w];
  const unsigned long long kmax = q.keys[(int64_t)m * 2], kmin = q.keys[(int64_t)m * 2 + 1];
  const uint32_t omax = (uint32_t)(kmax >> 32), omin = (uint32_t)(kmin >> 32);
  const int imax = (int)(0xffffffffu - (uint32_t)kmax), imin = (int)(uint32_t)kmin;
  double var = n > 1.0 ? (ss - s * s / n) / (n - 1.0) : 0.0;
  if (!(var > 0.0) || omax == omin) var = 0.0;
  stats[m * 4 + 0] = locate_unord(omax);
  stats[m * 4 + 1] = locate_unord(omin);
  stats[m * 4 + 2] = (float)(K + s / n);
  stats[m * 4 + 3] = (float)sqrt(var);
  xy[m * 5 + 0] = imax % q.g.ow; xy[m * 5 + 1] = imax / q.g.ow;
  xy[m * 5 + 2] = imin % q.g.ow; xy[m * 5 + 3] = imin / q.g.ow;
  xy[m * 5 + 4] = q.g.oh * q.g.ow;
}

// attn_sim[m, cy * g + cx] = sigmoid((D - mean) / std), D = the bilinear g x g resampling of the image-resolution field
// (F.interpolate(size=(g, g), align_corners=False): four field values per cell, evaluated here).  PerSAM normalises first and
// resamples then; the normalisation is affine and the weights sum to 1, so the order does not matter.  std == 0: 0 / 0 := 0,
// i.e. 0.5 everywhere (PerSAM itself would produce NaN).  Of `p` it reads the logits and the geometry.
__global__ __launch_bounds__(256) void persam_attn_sim_kernel(const MaskPostP p, int g, const float* __restrict__ stats,
                                                              float* __restrict__ attn) {
  const int m = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g * g) return;
  const float* low = p.low + (int64_t)m * p.g.h * p.g.w;
  const MaskScales sc = mask_scales(p.g);
  const int cy = c / g, cx = c - cy * g;
  const Lin ly = lin_coef(cy, (float)p.g.oh / (float)g, p.g.oh), lx = lin_coef(cx, (float)p.g.ow / (float)g, p.g.ow);
  float a00, a01, a10, a11;
  if (mask_form(p.g) != MASK_GENERIC) {
    a00 = mask_pixel<true>(low, p.g, sc, ly.i0, lx.i0); a01 = mask_pixel<true>(low, p.g, sc, ly.i0, lx.i1);
    a10 = mask_pixel<true>(low, p.g, sc, ly.i1, lx.i0); a11 = mask_pixel<true>(low, p.g, sc, ly.i1, lx.i1);
  } else {
    a00 = mask_pixel<false>(low, p.g, sc, ly.i0, lx.i0); a01 = mask_pixel<false>(low, p.g, sc, ly.i0, lx.i1);
    a10 = mask_pixel<false>(low, p.g, sc, ly.i1, lx.i0); a11 = mask_pixel<false>(low, p.g, sc, ly.i1, lx.i1);
  }
  const float D = ly.l0 * (lx.l0 * a00 + lx.l1 * a01) + ly.l1 * (lx.l0 * a10 + lx.l1 * a11);
  const float mean = stats[m * 4 + 2], sd = stats[m * 4 + 3];
  const float z = sd > 0.f ? (D - mean) / sd : 0.f;
  attn[(int64_t)m * g * g + c] = 1.0f / (1.0f + expf(-z));
}

// ---- launch geometry
// 256-thread blocks for n work items, at most cap
unsigned blocks256(int64_t n, int64_t cap) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b > cap ? cap : b);
}
constexpr int64_t NO_CAP = 0x7fffffffLL;
// blocks per mask of the flat scoring traversal: enough to fill the device at small k, few enough that the per-block
// reduction stays negligible
unsigned score_blocks(int32_t k, int out_h, int out_w) {
  return blocks256((int64_t)out_h * out_w, k >= 1024 ? 16 : (k >= 64 ? 64 : 1024));
}

int launch_mask_post(const MaskPostP& p, hipStream_t stream) {
  const MaskGeom& g = p.g;
  const MaskForm form = mask_form(g);
  const unsigned gx = form == MASK_STRIP ? blocks256(mask_strip_items(g.oh, g.ow, MP_ROWS), NO_CAP)
                                         : blocks256((int64_t)g.oh * g.ow / ((g.ow & 3) == 0 ? 4 : 1), 4096);
  for_mask_chunks(p.k, [&](int32_t m0, int32_t km) {
    MaskPostP c = p;
    c.low += (int64_t)m0 * g.h * g.w;
    c.out += (int64_t)m0 * g.oh * g.ow;
    if (c.prob) c.prob += (int64_t)m0 * g.oh * g.ow;
    c.k = km;
    switch (form) {
      case MASK_STRIP: hipLaunchKernelGGL(mask_post_strip_kernel, dim3(gx, km), dim3(MASK_BLOCK), 0, stream, c); break;
      case MASK_IDENT: hipLaunchKernelGGL((mask_post_kernel<true>), dim3(gx, km), dim3(MASK_BLOCK), 0, stream, c); break;
      case MASK_GENERIC: hipLaunchKernelGGL((mask_post_kernel<false>), dim3(gx, km), dim3(MASK_BLOCK), 0, stream, c); break;
    }
  });
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

}  // namespace

extern "C" int rsp_hyper_mask(const float* up, const float* hyper, float* out, int32_t R, int32_t npix,
                              int32_t C, rsp_stream_t stream) {
  if (!up || !hyper || !out || R < 0 || npix <= 0 || C <= 0 || (C & 3)) return RSP_EINVAL;
  if (R == 0) return RSP_OK;
  int gx = (npix + 31) / 32;
  if (gx > 512) gx = 512;
  hipLaunchKernelGGL(hyper_mask_kernel, dim3(gx, R), dim3(256), 0, (hipStream_t)stream, up, hyper, out, npix, C);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_mask_post(const float* low_res, float* sig_ws, int32_t k, int32_t h, int32_t w, int32_t Hb,
                             int32_t Wb, int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w, float thr,
                             uint8_t* out_mask, float* out_prob, rsp_stream_t stream) {
  const MaskGeom g{h, w, Hb, Wb, crop_h, crop_w, out_h, out_w};
  if (!low_res || !sig_ws || !out_mask || k < 0 || !mask_geom_valid(g)) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  const int64_t n = (int64_t)k * h * w;
  hipLaunchKernelGGL(sigmoid_kernel, dim3(blocks256(n, 4096)), dim3(256), 0, (hipStream_t)stream, low_res, sig_ws, n);
  return launch_mask_post(MaskPostP{sig_ws, out_mask, out_prob, k, g, thr, 0}, (hipStream_t)stream);
}

// SAMDet.predict (models.py:1185-1206): the same resize -> crop -> resize chain on the raw logits, then `> thr` (thr = 0)
extern "C" int rsp_mask_post_logits(const float* low_res, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb,
                                    int32_t crop_h, int32_t crop_w, int32_t out_h, int32_t out_w, float thr,
                                    uint8_t* out_mask, float* out_val, rsp_stream_t stream) {
  const MaskGeom g{h, w, Hb, Wb, crop_h, crop_w, out_h, out_w};
  if (!low_res || !out_mask || k < 0 || !mask_geom_valid(g)) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  return launch_mask_post(MaskPostP{low_res, out_mask, out_val, k, g, thr, 1}, (hipStream_t)stream);
}

extern "C" int rsp_mask_score_box(const float* low_res, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb, int32_t crop_h,
                                  int32_t crop_w, int32_t out_h, int32_t out_w, float t_hi, float t_lo, float t_mid,
                                  int32_t* out, rsp_stream_t stream) {
  const MaskGeom g{h, w, Hb, Wb, crop_h, crop_w, out_h, out_w};
  if (!low_res || !out || k < 0 || !mask_geom_valid(g) || (int64_t)k * 7 > 0x7fffffffLL) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((mask_score_init_kernel<7>), dim3(blocks256(k * 7, NO_CAP)), dim3(256), 0, st, out, k);
  const MaskForm form = mask_form(g);
  const unsigned gx = form == MASK_STRIP ? blocks256(mask_strip_items(out_h, out_w, MS_ROWS), NO_CAP) : score_blocks(k, out_h, out_w);
  for_mask_chunks(k, [&](int32_t m0, int32_t km) {
    const MaskScoreP q{low_res + (int64_t)m0 * h * w, g, out + (int64_t)m0 * 7, ScoreThr{t_hi, t_lo, t_mid}};
    switch (form) {
      case MASK_STRIP: hipLaunchKernelGGL(mask_score_strip_kernel, dim3(gx, km), dim3(MASK_BLOCK), 0, st, q); break;
      case MASK_IDENT: hipLaunchKernelGGL((mask_score_kernel<true>), dim3(gx, km), dim3(MASK_BLOCK), 0, st, q); break;
      case MASK_GENERIC: hipLaunchKernelGGL((mask_score_kernel<false>), dim3(gx, km), dim3(MASK_BLOCK), 0, st, q); break;
    }
  });
  hipLaunchKernelGGL(mask_score_final_kernel, dim3(blocks256(k, NO_CAP)), dim3(256), 0, st, out, k);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_mask_score_box_crops(const float* low_res, int32_t k, int32_t h, int32_t w, const int32_t* crop_idx,
                                        const int32_t* table, int32_t n_crops, int32_t max_out_h, int32_t max_out_w, float t_hi,
                                        float t_lo, float t_mid, int32_t* out, rsp_stream_t stream) {
  if (!low_res || !crop_idx || !table || !out || k < 0 || h <= 0 || w <= 0 || n_crops <= 0 || max_out_h <= 0 || max_out_w <= 0 ||
      (int64_t)max_out_h * max_out_w > 0x7fffffffLL || (int64_t)k * 8 > 0x7fffffffLL)
    return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((mask_score_init_kernel<8>), dim3(blocks256(k * 8, NO_CAP)), dim3(256), 0, st, out, k);
  // blocks per candidate as rsp_mask_score_box sizes them for the largest crop; a smaller crop's blocks find their loops empty
  const unsigned gx = score_blocks(k, max_out_h, max_out_w);
  for_mask_chunks(k, [&](int32_t m0, int32_t km) {
    const MaskScoreCropsP c{low_res + (int64_t)m0 * h * w, crop_idx + m0, table, out + (int64_t)m0 * 8, km, h, w, n_crops,
                            ScoreThr{t_hi, t_lo, t_mid}};
    hipLaunchKernelGGL(mask_score_crops_kernel, dim3(gx, km), dim3(MASK_BLOCK), 0, st, c);
  });
  hipLaunchKernelGGL(mask_score_crops_final_kernel, dim3(blocks256(k, NO_CAP)), dim3(256), 0, st, out, crop_idx, table, k, n_crops);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

namespace {
// blocks per image of rsp_persam_locate's reduction (also the number of fp64 partial pairs per image in its workspace)
int locate_gx(int out_h, int out_w, bool strip) {
  return (int)(strip ? blocks256(mask_strip_items(out_h, out_w, LOC_ROWS), NO_CAP) : blocks256((int64_t)out_h * out_w, 256));
}
}  // namespace

extern "C" int64_t rsp_persam_locate_workspace_bytes(int32_t k, int32_t out_h, int32_t out_w) {
  if (k < 0 || out_h <= 0 || out_w <= 0 || (int64_t)out_h * out_w > 0x7fffffffLL) return -1;
  const int gs = locate_gx(out_h, out_w, true), gg = locate_gx(out_h, out_w, false);
  return (int64_t)k * (16 + 16 * (int64_t)(gs > gg ? gs : gg));
}

extern "C" int rsp_persam_locate(const float* low_res, int32_t k, int32_t h, int32_t w, int32_t Hb, int32_t Wb, int32_t crop_h,
                                 int32_t crop_w, int32_t out_h, int32_t out_w, int32_t g, void* workspace,
                                 int64_t workspace_bytes, float* stats, int32_t* xy, float* attn_sim, rsp_stream_t stream) {
  const MaskGeom geom{h, w, Hb, Wb, crop_h, crop_w, out_h, out_w};
  if (!low_res || !workspace || !stats || !xy || !attn_sim || k < 0 || k > 65535 || !mask_geom_valid(geom) || g <= 0 || g > 4096)
    return RSP_EINVAL;
  if (workspace_bytes < rsp_persam_locate_workspace_bytes(k, out_h, out_w) || ((uintptr_t)workspace & 7)) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  hipStream_t st = (hipStream_t)stream;
  const MaskForm form = mask_form(geom);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(workspace);
  const LocateP q{low_res, geom, k, keys, reinterpret_cast<double*>(keys + (int64_t)k * 2),
                  locate_gx(out_h, out_w, form == MASK_STRIP)};
  hipLaunchKernelGGL(persam_locate_init_kernel, dim3(blocks256(k * 2, NO_CAP)), dim3(256), 0, st, q.keys, k);
  switch (form) {
    case MASK_STRIP: hipLaunchKernelGGL(persam_locate_strip_kernel, dim3((unsigned)q.gx, k), dim3(MASK_BLOCK), 0, st, q); break;
    case MASK_IDENT: hipLaunchKernelGGL((persam_locate_kernel<true>), dim3((unsigned)q.gx, k), dim3(MASK_BLOCK), 0, st, q); break;
    case MASK_GENERIC: hipLaunchKernelGGL((persam_locate_kernel<false>), dim3((unsigned)q.gx, k), dim3(MASK_BLOCK), 0, st, q); break;
  }
  hipLaunchKernelGGL(persam_locate_final_kernel, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, st, q, stats, xy);
  const MaskPostP field{low_res, nullptr, nullptr, k, geom, 0.f, 1};      // persam_attn_sim_kernel: logits + geometry
  hipLaunchKernelGGL(persam_attn_sim_kernel, dim3(blocks256(g * g, NO_CAP), k), dim3(256), 0, st, field, g, stats, attn_sim);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// FCNMaskHead._predict_by_feat_single + _do_paste_mask (mmdet/models/roi_heads/mask_heads/fcn_mask_head.py:276-480),
// the mask post-processing of the standard Mask R-CNN head the SAMSeg sibling models use (models.py:1219-1244):
// sigmoid of the (class-selected) 28x28 logits, F.grid_sample(bilinear, zeros, align_corners=False) of the probability
// map at every pixel centre of the image with the box as the sampling window, >= thr.  One thread per 4 output pixels.
namespace {

__global__ __launch_bounds__(256) void paste_masks_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                          const float* __restrict__ boxes, int Hm, int Wm, int C,
                                                          int img_h, int img_w, float thr, uint8_t* __restrict__ out) {
  const int n = blockIdx.y;
  const int cls = (labels && C > 1) ? labels[n] : 0;
  const float x0 = boxes[n * 4 + 0], y0 = boxes[n * 4 + 1], x1 = boxes[n * 4 + 2], y1 = boxes[n * 4 + 3];
  const float* m = logits + (int64_t)n * Hm * Wm * C + cls;          // NHWC: pixel stride C
  // the reference's CPU path pastes one instance per chunk with skip_empty=True (:390-404, :452-461): only the region
  // [floor(x0) - 1, ceil(x1) + 1) x [floor(y0) - 1, ceil(y1) + 1), clamped to the image, is written (the rest stays 0)
  const int rx0 = (int)fmaxf(floorf(x0) - 1.0f, 0.0f), ry0 = (int)fmaxf(floorf(y0) - 1.0f, 0.0f);
  const int rx1 = (int)fminf(ceilf(x1) + 1.0f, (float)img_w), ry1 = (int)fminf(ceilf(y1) + 1.0f, (float)img_h);
  const int64_t npix4 = ((int64_t)img_h * img_w + 3) / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix4; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t pix = i * 4 + e;
      if (pix >= (int64_t)img_h * img_w) break;
      const int py = (int)(pix / img_w), px = (int)(pix - (int64_t)py * img_w);
      if (px < rx0 || px >= rx1 || py < ry0 || py >= ry1) continue;
      // normalised coordinates exactly as the reference forms them: (p + 0.5 - lo) / (hi - lo) * 2 - 1, inf -> 0
      float gx = ((float)px + 0.5f - x0) / (x1 - x0) * 2.0f - 1.0f;
      float gy = ((float)py + 0.5f - y0) / (y1 - y0) * 2.0f - 1.0f;
      if (isinf(gx)) gx = 0.f;
      if (isinf(gy)) gy = 0.f;
      const float ix = ((gx + 1.0f) * (float)Wm - 1.0f) / 2.0f, iy = ((gy + 1.0f) * (float)Hm - 1.0f) / 2.0f;
      const float fx = floorf(ix), fy = floorf(iy);
      const int xw = (int)fx, yn = (int)fy;
      const float wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
      auto prob = [&](int yy, int xx) -> float {
        if (xx < 0 || xx >= Wm || yy < 0 || yy >= Hm) return 0.f;
        const float l = m[((int64_t)yy * Wm + xx) * C];
        return 1.0f / (1.0f + expf(-l));
      };
      float v = prob(yn, xw) * (wx0 * wy0);
      v += prob(yn, xw + 1) * (wx1 * wy0);
      v += prob(yn + 1, xw) * (wx0 * wy1);
      v += prob(yn + 1, xw + 1) * (wx1 * wy1);
      // thr < 0 (:390-394): the probability itself as (p * 255) truncated to uint8
      const uint32_t byte = thr >= 0.f ? (uint32_t)(v >= thr) : (uint32_t)(uint8_t)(v * 255.0f);
      word |= byte << (8 * e);
    }
    uint8_t* o = out + (int64_t)n * img_h * img_w + i * 4;
    if (i * 4 + 3 < (int64_t)img_h * img_w && ((((int64_t)n * img_h * img_w) & 3) == 0)) {
      *reinterpret_cast<uint32_t*>(o) = word;
    } else {
      for (int e = 0; e < 4 && i * 4 + e < (int64_t)img_h * img_w; ++e) o[e] = (word >> (8 * e)) & 0xffu;
    }
  }
}

}  // namespace

extern "C" int rsp_paste_masks(const float* logits, const int32_t* labels, const float* boxes, int32_t k, int32_t Hm,
                               int32_t Wm, int32_t C, int32_t img_h, int32_t img_w, float thr, uint8_t* out,
                               rsp_stream_t stream) {
  if (!logits || !boxes || !out || k < 0 || Hm <= 0 || Wm <= 0 || C <= 0 || img_h <= 0 || img_w <= 0) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  const int64_t npix4 = ((int64_t)img_h * img_w + 3) / 4;
  const unsigned gx = (unsigned)((npix4 + 255) / 256 > 1024 ? 1024 : (npix4 + 255) / 256);
  hipLaunchKernelGGL(paste_masks_kernel, dim3(gx, (unsigned)k), dim3(256), 0, (hipStream_t)stream, logits, labels, boxes, Hm, Wm,
                     C, img_h, img_w, thr, out);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Host-glue kernels of the folded token -> image attention (sam_decoder.py::_t2i_folded, csrc/t2i_fold.hip).  Round 5 built
// the block-diagonal query with torch (mul, permute, zeros, index_put, split: 6 launches) and picked every column's own head
// out of the v_proj result with an advanced index + permute (4 launches), twice per decoder call.
//   expand: tq [R*T, 128] (projected queries, head h at columns 16 h ..) -> fp16 planes of the block-diagonal matrix
//           [R*96, 128]: row r*96 + h*T + t holds scale * tq[r, t, 16 h .. 16 h + 15] in columns 16 h .., zeros elsewhere;
//           rows of columns >= 8 T are zero
//   gather: full [R*96, 128] (v_proj applied to every column) -> ao [R*T, 128] with ao[r*T + t, 16 h + d] = full[r*96 + h*T + t, 16 h + d]
namespace {
__global__ __launch_bounds__(256) void sam_fold_expand_kernel(const float* __restrict__ tq, half_t* __restrict__ hi, half_t* __restrict__ lo,
                                                                int64_t rows, int T, float scale, float pscale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;        // one thread = 4 consecutive columns of one output row
  if (i >= rows * 32) return;
  const int64_t row = i >> 5;
  const int c = (int)(i & 31) * 4;
  const int64_t r = row / 96;
  const int col = (int)(row - r * 96);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (col < 8 * T) {
    const int h = col / T, t = col - h * T;
    if ((c >> 4) == h) {
      v = *reinterpret_cast<const f32x4*>(tq + (r * T + t) * 128 + c);
    }
  }
  // element by element: `v * scale` on the vector type becomes v_pk_mul_f32 with the scalar cross-selected through op_sel,
  // the instruction class DESIGN 9.1 keeps out of every kernel that shares a SIMD (tests/test_isa_guard_cpu.py)
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (v[e] * scale) * pscale;
  rsp_store_planes4(hi, lo, ((int64_t)(c >> 5) * rows + row) * 32 + (c & 31), v, false);
}

__global__ __launch_bounds__(256) void sam_fold_gather_kernel(const float* __restrict__ full, float* __restrict__ ao, int64_t n4, int T) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;        // 4 consecutive columns of one (RoI, token) row
  if (i >= n4) return;
  const int64_t row = i >> 5;                                        // r * T + t
  const int c = (int)(i & 31) * 4;
  const int64_t r = row / T;
  const int t = (int)(row - r * T), h = c >> 4;
  *reinterpret_cast<f32x4*>(ao + row * 128 + c) = *reinterpret_cast<const f32x4*>(full + (r * 96 + h * T + t) * 128 + c);
}
}  // namespace

extern "C" int rsp_sam_fold_expand(const float* tq, uint16_t* out_hi, uint16_t* out_lo, int32_t out_scale_log2, int32_t R, int32_t T,
                                   float scale, rsp_stream_t stream) {
  if (!tq || !out_hi || !out_lo || R < 0 || T <= 0 || T > RSP_SAM_T2I_FOLD_MAX_TOKENS || !RSP_PLANE_WORD_VALID(out_scale_log2) ||
      RSP_PLANE_IS_F8(out_scale_log2))
    return RSP_EINVAL;
  if (R == 0) return RSP_OK;
  const int64_t rows = (int64_t)R * 96, n = rows * 32;
  hipLaunchKernelGGL(sam_fold_expand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tq,
                     reinterpret_cast<half_t*>(out_hi), reinterpret_cast<half_t*>(out_lo), rows, T, scale,
                     ldexpf(1.0f, RSP_PLANE_EXP(out_scale_log2)));
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_sam_fold_gather(const float* full, float* ao, int32_t R, int32_t T, rsp_stream_t stream) {
  if (!full || !ao || R < 0 || T <= 0 || T > RSP_SAM_T2I_FOLD_MAX_TOKENS) return RSP_EINVAL;
  if (R == 0) return RSP_OK;
  const int64_t n4 = (int64_t)R * T * 32;
  hipLaunchKernelGGL(sam_fold_gather_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, full, ao, n4, T);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
