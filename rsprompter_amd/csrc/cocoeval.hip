// COCO evaluation on the device: the per-pair and per-(image, category) work of pycocotools' COCOeval.
// Definitions restated from cocoapi (maskApi.c rleFrString / rleArea / rleIou / bbIou, cocoeval.py evaluateImg); the
// host keeps accumulate / summarize (rsprompter_amd/evaluation.py).
//   rsp_rle_from_string  COCO compressed strings -> run counts (the inverse of rsp_rle_to_string, rle.hip)
//   rsp_rle_to_bits      run counts -> bit-packed masks in the column-major order of the RLE stream + area + word range
//   rsp_coco_iou         IoU blocks [nd, ng] of a batch of units, masks (popcount of AND) or boxes (bbIou in fp64)
//   rsp_coco_match       evaluateImg's greedy matching for every unit x area range x IoU threshold
#include "rsp_common.h"

namespace {

// ---- strings -> counts: one lane per string (strings are a few hundred bytes; the exchange hands thousands per call)
constexpr int DEC_THREADS = 64;

__global__ __launch_bounds__(DEC_THREADS) void rle_from_string_kernel(const uint8_t* __restrict__ flat,
                                                                      const int64_t* __restrict__ offs, int k, int cap,
                                                                      uint32_t* __restrict__ counts,
                                                                      int32_t* __restrict__ n_counts) {
  const int i = blockIdx.x * DEC_THREADS + threadIdx.x;
  if (i >= k) return;
  const int64_t p0 = offs[i], p1 = offs[i + 1];
  uint32_t* out = counts + (int64_t)i * cap;
  int m = 0;
  int64_t p = p0;
  while (p < p1 && flat[p] != 0) {
    int64_t x = 0;
    int g = 0;
    bool more = true;
    while (more) {
      // a string cut inside a value reads as if the value ended there (cocoapi would read up to the terminator)
      const int c = p < p1 ? (int)flat[p] - 48 : 0;
      if (g < 12) x |= (int64_t)(c & 0x1f) << (5 * g);
      more = (c & 0x20) != 0;
      ++p;
      ++g;
      if (!more && (c & 0x10) && g < 13) x |= (int64_t)-1 << (5 * g);
    }
    if (m < cap) {
      if (m > 2) x += (int64_t)out[m - 2];
      out[m] = (uint32_t)x;
    }
    ++m;
  }
  n_counts[i] = m <= cap ? m : -m;
}

// ---- counts -> bits.  Pixel j of the column-major stream is bit (j & 63) of word j >> 6 of the mask's word range.
// One block per mask: chunks of 256 runs, start positions from a block scan; a run writes its interior words with plain
// stores (no other run touches them) and its two end words with atomicOr (neighbouring runs may share them).
constexpr int BIT_THREADS = 256;

__global__ __launch_bounds__(BIT_THREADS) void rle_to_bits_kernel(const uint32_t* __restrict__ counts,
                                                                  const int32_t* __restrict__ n_counts, int cap,
                                                                  const int64_t* __restrict__ word_offs,
                                                                  unsigned long long* __restrict__ bits,
                                                                  int64_t* __restrict__ area, int32_t* __restrict__ wrange) {
  __shared__ long long sc[BIT_THREADS];
  __shared__ long long s_base;
  __shared__ long long s_area[BIT_THREADS];
  __shared__ long long s_lo[BIT_THREADS];
  __shared__ long long s_hi[BIT_THREADS];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(n_counts[m], 0), cap);
  const uint32_t* c = counts + (int64_t)m * cap;
  const int64_t w0 = word_offs[m];
  const int64_t nw = word_offs[m + 1] - w0;
  const long long nbits = (long long)nw * 64;
  unsigned long long* wd = bits + w0;
  for (int64_t w = tid; w < nw; w += BIT_THREADS) wd[w] = 0ull;
  if (tid == 0) s_base = 0;
  __syncthreads();
  long long my_area = 0, my_lo = nbits, my_hi = 0;
  for (int i0 = 0; i0 < n; i0 += BIT_THREADS) {
    const int i = i0 + tid;
    const long long len = i < n ? (long long)c[i] : 0;
    sc[tid] = len;
    __syncthreads();
    for (int o = 1; o < BIT_THREADS; o <<= 1) {
      const long long v = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    const long long s = s_base + sc[tid] - len;
    if ((i & 1) && len > 0) {
      my_area += len;
      const long long e = min(s + len, nbits);           // counts that overrun the mask's words are cut (malformed input)
      if (s < e) {
        my_lo = min(my_lo, s);
        my_hi = max(my_hi, e);
        const long long wa = s >> 6, wb = (e - 1) >> 6;
        const unsigned long long ma = ~0ull << (s & 63);
        const unsigned long long mb = ~0ull >> (63 - ((e - 1) & 63));
        if (wa == wb) {
          atomicOr(wd + wa, ma & mb);
        } else {
          atomicOr(wd + wa, ma);
          for (long long w = wa + 1; w < wb; ++w) wd[w] = ~0ull;
          atomicOr(wd + wb, mb);
        }
      }
    }
    __syncthreads();
    if (tid == BIT_THREADS - 1) s_base += sc[tid];
    __syncthreads();
  }
  s_area[tid] = my_area;
  s_lo[tid] = my_lo;
  s_hi[tid] = my_hi;
  __syncthreads();
  if (tid == 0) {
    long long a = 0, lo = nbits, hi = 0;
    for (int t = 0; t < BIT_THREADS; ++t) {
      a += s_area[t];
      lo = min(lo, s_lo[t]);
      hi = max(hi, s_hi[t]);
    }
    area[m] = a;
    if (wrange) {                                         // words [lo, hi) hold every set bit; empty mask: [0, 0)
      wrange[2 * m] = hi > 0 ? (int32_t)(lo >> 6) : 0;
      wrange[2 * m + 1] = hi > 0 ? (int32_t)((hi + 63) >> 6) : 0;
    }
  }
}

// ---- IoU.  One block per unit.  Masks: one wave per (dt, gt) pair, lanes over the words both masks may have set;
// boxes: one lane per pair.
constexpr int IOU_THREADS = 256;

__global__ __launch_bounds__(IOU_THREADS) void coco_iou_mask_kernel(const RspCocoUnit* __restrict__ units,
                                                                    const unsigned long long* __restrict__ dt_bits,
                                                                    const unsigned long long* __restrict__ gt_bits,
                                                                    const int64_t* __restrict__ dt_woff,
                                                                    const int64_t* __restrict__ gt_woff,
                                                                    const int32_t* __restrict__ dt_wr,
                                                                    const int32_t* __restrict__ gt_wr,
                                                                    const int64_t* __restrict__ dt_area,
                                                                    const int64_t* __restrict__ gt_area,
                                                                    const uint8_t* __restrict__ gt_crowd,
                                                                    double* __restrict__ iou) {
  const RspCocoUnit u = units[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int npair = u.nd * u.ng;
  for (int p = wave; p < npair; p += IOU_THREADS / 64) {
    const int d = p / u.ng, g = p - d * u.ng;
    const int64_t di = u.dt0 + d, gi = u.gt0 + g;
    const int lo = max(dt_wr[2 * di], gt_wr[2 * gi]);
    const int hi = min(min(dt_wr[2 * di + 1], gt_wr[2 * gi + 1]), u.nwords);
    const unsigned long long* a = dt_bits + dt_woff[di];
    const unsigned long long* b = gt_bits + gt_woff[gi];
    long long inter = 0;
    for (int w = lo + lane; w < hi; w += 64) inter += __popcll(a[w] & b[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) inter += __shfl_xor(inter, o, 64);
    if (lane == 0) {
      double r = 0.0;
      if (inter > 0) {
        // maskApi.c rleIou: u = |d| + |g| - i, or |d| inside a crowd region; i == 0 -> 0 (bbox prefilter)
        const long long un = gt_crowd[gi] ? (long long)dt_area[di] : (long long)dt_area[di] + (long long)gt_area[gi] - inter;
        r = (double)inter / (double)un;
      }
      iou[u.out0 + p] = r;
    }
  }
}

__device__ __forceinline__ double bb_iou(const double* D, const double* G, bool crowd) {
#pragma clang fp contract(off)
  // maskApi.c bbIou on xywh, fp64, in cocoapi's order of operations (a fused da + ga - w*h would round differently)
  const double ga = G[2] * G[3], da = D[2] * D[3];
  const double w = fmin(D[2] + D[0], G[2] + G[0]) - fmax(D[0], G[0]);
  if (w <= 0) return 0.0;
  const double h = fmin(D[3] + D[1], G[3] + G[1]) - fmax(D[1], G[1]);
  if (h <= 0) return 0.0;
  const double i = w * h;
  const double un = crowd ? da : da + ga - i;
  return i / un;
}

__global__ __launch_bounds__(IOU_THREADS) void coco_iou_box_kernel(const RspCocoUnit* __restrict__ units,
                                                                   const double* __restrict__ dt_box,
                                                                   const double* __restrict__ gt_box,
                                                                   const uint8_t* __restrict__ gt_crowd,
                                                                   double* __restrict__ iou) {
  const RspCocoUnit u = units[blockIdx.x];
  const int npair = u.nd * u.ng;
  for (int p = threadIdx.x; p < npair; p += IOU_THREADS) {
    const int d = p / u.ng, g = p - d * u.ng;
    const int64_t di = u.dt0 + d, gi = u.gt0 + g;
    iou[u.out0 + p] = bb_iou(dt_box + 4 * di, gt_box + 4 * gi, gt_crowd[gi] != 0);
  }
}

// ---- evaluateImg (cocoeval.py): one block per unit, one lane per (area range, threshold).  The lane walks the dts in
// the given (score-sorted, truncated) order and the gts with the range's ignored ones moved to the back, stably: first
// the kept gts in input order, then the ignored ones.  gtm (matched flags) lives in a byte workspace [A*T, ng] per unit.
constexpr int MATCH_THREADS = 64;
constexpr int MATCH_MAX_A = 8;

__global__ __launch_bounds__(MATCH_THREADS) void coco_match_kernel(const RspCocoUnit* __restrict__ units,
                                                                   const double* __restrict__ iou,
                                                                   const double* __restrict__ gt_area,
                                                                   const uint8_t* __restrict__ gt_crowd,
                                                                   const int64_t* __restrict__ gt_id,
                                                                   const double* __restrict__ dt_area,
                                                                   const double* __restrict__ area_rng, int A,
                                                                   const double* __restrict__ thrs, int T,
                                                                   int64_t n_dt, uint8_t* __restrict__ gtm_ws,
                                                                   int64_t* __restrict__ dtm, uint8_t* __restrict__ dtig,
                                                                   int32_t* __restrict__ npig) {
  const RspCocoUnit u = units[blockIdx.x];
  const int nd = u.nd, ng = u.ng;
  if (threadIdx.x < A) {
    const double lo = area_rng[2 * threadIdx.x], hi = area_rng[2 * threadIdx.x + 1];
    int cnt = 0;
    for (int g = 0; g < ng; ++g) {
      const double ga = gt_area[u.gt0 + g];
      cnt += !(gt_crowd[u.gt0 + g] || ga < lo || ga > hi);
    }
    npig[(int64_t)blockIdx.x * A + threadIdx.x] = cnt;
  }
  for (int combo = threadIdx.x; combo < A * T; combo += MATCH_THREADS) {
    const int a = combo / T, t = combo - a * T;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double thr = fmin(thrs[t], 1.0 - 1e-10);
    uint8_t* gtm = gtm_ws + u.gt0 * (int64_t)(A * T) + (int64_t)combo * ng;
    for (int g = 0; g < ng; ++g) gtm[g] = 0;
    const int64_t obase = (int64_t)combo * n_dt + u.dt0;
    for (int d = 0; d < nd; ++d) {
      const double* row = iou + u.out0 + (int64_t)d * ng;
      double best = thr;
      int m = -1, m_ig = 0;
      bool stop = false;
      for (int pass = 0; pass < 2 && !stop; ++pass) {
        for (int g = 0; g < ng; ++g) {
          const int crowd = gt_crowd[u.gt0 + g] != 0;
          const double ga = gt_area[u.gt0 + g];
          const int ig = crowd || ga < lo || ga > hi;
          if (ig != pass) continue;
          if (gtm[g] && !crowd) continue;
          if (m > -1 && m_ig == 0 && ig == 1) { stop = true; break; }
          const double v = row[g];
          if (v < best) continue;
          best = v;
          m = g;
          m_ig = ig;
        }
      }
      int64_t mid = 0;
      int dig = 0;
      if (m > -1) {
        mid = gt_id[u.gt0 + m];
        dig = m_ig;
        gtm[m] = 1;
      }
      const double da = dt_area[u.dt0 + d];
      if (mid == 0 && (da < lo || da > hi)) dig = 1;   // unmatched (dtm == 0, annotation id 0 included) and outside
      dtm[obase + d] = mid;
      dtig[obase + d] = (uint8_t)dig;
    }
  }
}

}  // namespace

extern "C" int rsp_rle_from_string(const uint8_t* flat, const int64_t* offs, int32_t k, int32_t cap, uint32_t* counts,
                                   int32_t* n_counts, rsp_stream_t stream) {
  if (!flat || !offs || !counts || !n_counts || k < 0 || cap < 1) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  hipLaunchKernelGGL(rle_from_string_kernel, dim3((k + DEC_THREADS - 1) / DEC_THREADS), dim3(DEC_THREADS), 0,
                     (hipStream_t)stream, flat, offs, k, cap, counts, n_counts);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_rle_to_bits(const uint32_t* counts, const int32_t* n_counts, int32_t k, int32_t cap,
                               const int64_t* word_offs, uint64_t* bits, int64_t* area, int32_t* wrange,
                               rsp_stream_t stream) {
  if (!counts || !n_counts || !word_offs || !bits || !area || k < 0 || cap < 1) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  hipLaunchKernelGGL(rle_to_bits_kernel, dim3(k), dim3(BIT_THREADS), 0, (hipStream_t)stream, counts, n_counts, cap,
                     word_offs, reinterpret_cast<unsigned long long*>(bits), area, wrange);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_coco_iou(const RspCocoUnit* units, int32_t n_units, int32_t mode, const uint64_t* dt_bits,
                            const uint64_t* gt_bits, const int64_t* dt_woff, const int64_t* gt_woff,
                            const int32_t* dt_wrange, const int32_t* gt_wrange, const int64_t* dt_area,
                            const int64_t* gt_area, const double* dt_box, const double* gt_box, const uint8_t* gt_crowd,
                            double* iou, rsp_stream_t stream) {
  if (!units || !gt_crowd || !iou || n_units < 0) return RSP_EINVAL;
  if (mode == RSP_COCO_IOU_SEGM) {
    if (!dt_bits || !gt_bits || !dt_woff || !gt_woff || !dt_wrange || !gt_wrange || !dt_area || !gt_area)
      return RSP_EINVAL;
  } else if (mode == RSP_COCO_IOU_BBOX) {
    if (!dt_box || !gt_box) return RSP_EINVAL;
  } else {
    return RSP_EINVAL;
  }
  if (n_units == 0) return RSP_OK;
  if (mode == RSP_COCO_IOU_SEGM) {
    hipLaunchKernelGGL(coco_iou_mask_kernel, dim3(n_units), dim3(IOU_THREADS), 0, (hipStream_t)stream, units,
                       reinterpret_cast<const unsigned long long*>(dt_bits),
                       reinterpret_cast<const unsigned long long*>(gt_bits), dt_woff, gt_woff, dt_wrange, gt_wrange,
                       dt_area, gt_area, gt_crowd, iou);
  } else {
    hipLaunchKernelGGL(coco_iou_box_kernel, dim3(n_units), dim3(IOU_THREADS), 0, (hipStream_t)stream, units, dt_box,
                       gt_box, gt_crowd, iou);
  }
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_coco_match(const RspCocoUnit* units, int32_t n_units, const double* iou, const double* gt_area,
                              const uint8_t* gt_crowd, const int64_t* gt_id, const double* dt_area,
                              const double* area_rng, int32_t A, const double* thrs, int32_t T, int64_t n_dt,
                              uint8_t* gtm_ws, int64_t* dtm, uint8_t* dtig, int32_t* npig, rsp_stream_t stream) {
  if (!units || !iou || !gt_area || !gt_crowd || !gt_id || !dt_area || !area_rng || !thrs || !gtm_ws ||
      !dtm || !dtig || !npig || n_units < 0 || A < 1 || A > MATCH_MAX_A || T < 1 || n_dt < 0)
    return RSP_EINVAL;
  if (n_units == 0) return RSP_OK;
  hipLaunchKernelGGL(coco_match_kernel, dim3(n_units), dim3(MATCH_THREADS), 0, (hipStream_t)stream, units, iou, gt_area,
                     gt_crowd, gt_id, dt_area, area_rng, A, thrs, T, n_dt, gtm_ws, dtm, dtig, npig);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
