// COCO mask IoU in the run domain: the IoU blocks of RspCocoUnits from two run tables, for scenes whose
// masks never exist as bits (one 8 192 x 9 000 mask is 9.2 MB of them and about 1 300 runs).  The layout of `iou` and the
// arithmetic are rsp_coco_iou's (csrc/cocoeval.hip, coco_iou_mask_kernel), so rsp_coco_match runs behind it unchanged and
// both routes give the same doubles.
//   rsp_run_prefix           : per row the prefix workspace (run_table.h), the area and the extent of the set pixels
//   rsp_coco_iou_runs_filter : one lane per pair: disjoint or touching extents -> 0.0, else the pair is marked alive
//   rsp_coco_iou_runs        : one wave per surviving pair: the walk
// Nothing here takes a canvas size: a row is its column-major stream.  Integer arithmetic up to the one division; every
// slot of `iou` is written once by a plain store, and a second launch gives the same bits.
#include "rsp_common.h"
#include "run_table.h"

namespace {

constexpr int CR_THREADS = 256;
constexpr int CR_WAVES = CR_THREADS / 64;

// ------------------------------------------------------------------------------------------------- prefix, area, extent
// One block per row.  extent = [first set pixel, one past the last set pixel) of the stream, (0, 0) for a row without a
// set pixel; ones-runs of zero pixels (non-canonical counts) do not count.
__global__ __launch_bounds__(CR_THREADS) void run_prefix_kernel(const uint32_t* __restrict__ counts,
                                                                const int32_t* __restrict__ n_in, int cap,
                                                                int32_t* __restrict__ ws, int64_t* __restrict__ area,
                                                                int32_t* __restrict__ extent) {
  __shared__ int tmp[CR_WAVES];
  __shared__ int red[2 * CR_WAVES];
  const int m = blockIdx.x, tid = threadIdx.x;
  const RspRunRow row = rsp_run_row(counts, n_in, cap, m);
  int32_t* w_row = ws + (int64_t)m * cap;
  RspRunPrefix<CR_THREADS> p;
  for (RspRunWalk<CR_THREADS> r(row, tmp); r.next();) p.step(r, row, w_row, tmp);
  int lo = p.lo, hi = p.hi;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  if ((tid & 63) == 0) {
    red[tid >> 6] = lo;
    red[CR_WAVES + (tid >> 6)] = hi;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < CR_WAVES; ++w) {
      lo = min(lo, red[w]);
      hi = max(hi, red[CR_WAVES + w]);
    }
    area[m] = (int64_t)p.ones;
    extent[2 * m] = hi > 0 ? lo : 0;
    extent[2 * m + 1] = hi;
  }
}

// ------------------------------------------------------------------------------------------------- filter
// One lane per slot p of iou[0, n_iou), grid-strided.  Its unit is the last one with out0 <= p (units ascend in out0 and
// tile [0, n_iou) back to back, as ops.coco_units' callers build them; units without a pair share their out0 with the next
// one and are passed over).  A slot that no unit owns, or whose rows lie outside the tables, gets 0.0 like a dead pair.
// alive[p] = dt row << 32 | gt row for a pair whose extents overlap in at least one stream position, -1 otherwise: the
// exact stand-in of rleIou's bbIou prefilter (masks that share a pixel share a stream position), as wrange is on the bits
// route.  No run is read.
__global__ __launch_bounds__(CR_THREADS) void coco_iou_runs_filter_kernel(const RspCocoUnit* __restrict__ units, int n_units,
                                                                         int64_t n_iou, const int32_t* __restrict__ dt_ext,
                                                                         int64_t n_dt, const int32_t* __restrict__ gt_ext,
                                                                         int64_t n_gt, int64_t* __restrict__ alive,
                                                                         double* __restrict__ iou) {
  const int64_t stride = (int64_t)gridDim.x * CR_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * CR_THREADS + threadIdx.x; p < n_iou; p += stride) {
    int lo = -1, hi = n_units - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (units[mid].out0 <= p) lo = mid; else hi = mid - 1;
    }
    int64_t key = -1;
    if (lo >= 0) {
      const RspCocoUnit u = units[lo];
      const int64_t q = p - u.out0;
      if (u.nd > 0 && u.ng > 0 && q < (int64_t)u.nd * u.ng) {
        const int64_t d = q / u.ng, di = u.dt0 + d, gi = u.gt0 + (q - d * u.ng);
        if (di >= 0 && di < n_dt && gi >= 0 && gi < n_gt) {
          const int s = max(dt_ext[2 * di], gt_ext[2 * gi]), e = min(dt_ext[2 * di + 1], gt_ext[2 * gi + 1]);
          if (s < e) key = di << 32 | gi;
        }
      }
    }
    alive[p] = key;
    if (key < 0) iou[p] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------------- walk
__device__ __forceinline__ SmRow cr_row(const uint32_t* __restrict__ counts, const int32_t* __restrict__ n_in, int cap,
                                        const int32_t* __restrict__ ws, int64_t m) {
  return SmRow{counts + m * cap, ws + m * cap, max(min(n_in[m], cap), 0) >> 1};
}

// One wave per surviving pair, grid-strided over slots[0, n_slots) (the slot numbers p of the pairs the filter left alive).
// Only the ones-runs inside the window W = [max of the firsts, min of the ends) of the two extents are walked: in each row
// from the last run that starts at or before the window's first pixel to the last run that starts at or before its last
// pixel (sm_find).  The lanes take the runs of the row that has FEWER of them there, clip each to W and look its two ends
// up in the other row's prefix (sm_ones_before): one run against 50 000 is two searches.  The runs of a row are disjoint
// intervals whatever the counts, so the sum is |d & g| exactly; union in 64 bits (area_d + area_g passes 2^31 on a canvas
// that fits), 0.0 when inter == 0, one division: coco_iou_mask_kernel's arithmetic.
__global__ __launch_bounds__(CR_THREADS) void coco_iou_runs_walk_kernel(
    const int64_t* __restrict__ slots, int64_t n_slots, int64_t n_iou, const int64_t* __restrict__ alive,
    const uint32_t* __restrict__ dt_counts, const int32_t* __restrict__ dt_n, int dt_cap, int64_t n_dt,
    const int32_t* __restrict__ dt_ws, const int64_t* __restrict__ dt_area, const int32_t* __restrict__ dt_ext,
    const uint32_t* __restrict__ gt_counts, const int32_t* __restrict__ gt_n, int gt_cap, int64_t n_gt,
    const int32_t* __restrict__ gt_ws, const int64_t* __restrict__ gt_area, const int32_t* __restrict__ gt_ext,
    const uint8_t* __restrict__ gt_crowd, double* __restrict__ iou) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * CR_WAVES;
  for (int64_t q = (int64_t)blockIdx.x * CR_WAVES + (threadIdx.x >> 6); q < n_slots; q += stride) {
    const int64_t p = slots[q];
    if (p < 0 || p >= n_iou) continue;                                   // wave-uniform, as everything up to the run loop
    const int64_t key = alive[p];
    const int64_t di = key >> 32, gi = key & 0xffffffffLL;
    if (key < 0 || di >= n_dt || gi >= n_gt) continue;
    const SmRow D = cr_row(dt_counts, dt_n, dt_cap, dt_ws, di), G = cr_row(gt_counts, gt_n, gt_cap, gt_ws, gi);
    const int w0 = max(dt_ext[2 * di], gt_ext[2 * gi]), w1 = min(dt_ext[2 * di + 1], gt_ext[2 * gi + 1]);
    long long inter = 0;
    if (w0 < w1 && D.nr > 0 && G.nr > 0) {
      const int d0 = max(sm_find(D, w0), 0), d1 = sm_find(D, w1 - 1);
      const int g0 = max(sm_find(G, w0), 0), g1 = sm_find(G, w1 - 1);
      const bool d_walks = d1 - d0 <= g1 - g0;
      const SmRow& A = d_walks ? D : G;
      const SmRow& B = d_walks ? G : D;
      const int a0 = d_walks ? d0 : g0, a1 = d_walks ? d1 : g1;
      for (int t = a0 + lane; t <= a1; t += 64) {
        const int s0 = A.ws[2 * t + 1];
        const int s = max(s0, w0), e = min(s0 + (int)A.c[2 * t + 1], w1);
        if (s < e) inter += sm_ones_before(B, e) - sm_ones_before(B, s);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) inter += __shfl_xor(inter, o, 64);
    if (lane == 0) {
      double r = 0.0;
      if (inter > 0) {
        const long long un = gt_crowd[gi] ? (long long)dt_area[di] : (long long)dt_area[di] + (long long)gt_area[gi] - inter;
        r = (double)inter / (double)un;
      }
      iou[p] = r;
    }
  }
}

inline int cr_grid(int64_t work, int per_block) {
  const int64_t b = (work + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

extern "C" int64_t rsp_run_prefix_workspace_bytes(int32_t k, int32_t cap) {
  if (k < 0 || cap < 1) return 0;
  return (int64_t)(k > 0 ? k : 1) * cap * (int64_t)sizeof(int32_t);
}

extern "C" int rsp_run_prefix(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, void* workspace,
                              int64_t* area, int32_t* extent, rsp_stream_t stream) {
  if (k < 0 || cap < 1) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  if (!counts || !n || !workspace || !area || !extent) return RSP_EINVAL;
  hipLaunchKernelGGL(run_prefix_kernel, dim3(k), dim3(CR_THREADS), 0, (hipStream_t)stream, counts, n, cap,
                     static_cast<int32_t*>(workspace), area, extent);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_coco_iou_runs_filter(const RspCocoUnit* units, int32_t n_units, int64_t n_iou, const int32_t* dt_extent,
                                        int64_t n_dt, const int32_t* gt_extent, int64_t n_gt, int64_t* alive, double* iou,
                                        rsp_stream_t stream) {
  if (n_units < 0 || n_iou < 0 || n_dt < 0 || n_gt < 0) return RSP_EINVAL;
  if (n_units == 0 || n_iou == 0) return RSP_OK;
  if (!units || !alive || !iou || (n_dt > 0 && !dt_extent) || (n_gt > 0 && !gt_extent)) return RSP_EINVAL;
  hipLaunchKernelGGL(coco_iou_runs_filter_kernel, dim3(cr_grid(n_iou, CR_THREADS)), dim3(CR_THREADS), 0, (hipStream_t)stream,
                     units, n_units, n_iou, dt_extent, n_dt, gt_extent, n_gt, alive, iou);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_coco_iou_runs(const int64_t* slots, int64_t n_slots, int64_t n_iou, const int64_t* alive,
                                 const uint32_t* dt_counts, const int32_t* dt_n, int64_t n_dt, int32_t dt_cap,
                                 const void* dt_workspace, const int64_t* dt_area, const int32_t* dt_extent,
                                 const uint32_t* gt_counts, const int32_t* gt_n, int64_t n_gt, int32_t gt_cap,
                                 const void* gt_workspace, const int64_t* gt_area, const int32_t* gt_extent,
                                 const uint8_t* gt_crowd, double* iou, rsp_stream_t stream) {
  if (n_slots < 0 || n_iou < 0 || n_dt < 0 || n_gt < 0 || dt_cap < 1 || gt_cap < 1) return RSP_EINVAL;
  if (n_slots == 0 || n_iou == 0 || n_dt == 0 || n_gt == 0) return RSP_OK;
  if (!slots || !alive || !dt_counts || !dt_n || !dt_workspace || !dt_area || !dt_extent || !gt_counts || !gt_n ||
      !gt_workspace || !gt_area || !gt_extent || !gt_crowd || !iou)
    return RSP_EINVAL;
  hipLaunchKernelGGL(coco_iou_runs_walk_kernel, dim3(cr_grid(n_slots, CR_WAVES)), dim3(CR_THREADS), 0, (hipStream_t)stream,
                     slots, n_slots, n_iou, alive, dt_counts, dt_n, dt_cap, n_dt, static_cast<const int32_t*>(dt_workspace),
                     dt_area, dt_extent, gt_counts, gt_n, gt_cap, n_gt, static_cast<const int32_t*>(gt_workspace), gt_area,
                     gt_extent, gt_crowd, iou);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
