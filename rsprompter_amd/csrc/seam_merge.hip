// Merging instances cut by tile seams: arithmetic BETWEEN scene-sized masks in the run domain.  The dense
// form -- pad every tile mask to the scene (sahi shift_masks), then `(a & b).sum()`, `a[:, y0:y1, x0:x1].sum()`,
// `a | b` and pycocotools' toBbox / area / encode on scene-sized arrays -- never exists: one 10 000 x 10 000 mask is
// 100 MB.  Input everywhere: a scene-frame run table as rsp_rle_shift writes it, read through run_table.h.
//   rsp_rle_bbox         : tight box + area per row (maskUtils.toBbox / area)
//   rsp_rle_pair_overlap : per pair of rows (i, j) and rectangle R: |M_i & M_j|, |M_i & R|, |M_j & R|
//   rsp_rle_intervals    : the ones-runs of the member rows of G groups as (group, start) keys + ends, to be sorted by key
//   rsp_rle_union        : sorted intervals of G groups -> canonical COCO run counts of each group's union
// Integer arithmetic only; every result is exact and independent of the launch.
#include "rsp_common.h"
#include "run_table.h"

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / 64;

// block-wide EXCLUSIVE max scan of non-negative ints (identity 0); *total = the block's max
__device__ __forceinline__ int sm_excl_max_scan(int v, int* tmp, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl = max(incl, t);
  }
  int excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 0;
  if (lane == 63) tmp[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SM_WAVES; ++w) {
    const int t = tmp[w];
    if (w < wave) base = max(base, t);
    tot = max(tot, t);
  }
  *total = tot;
  __syncthreads();
  return max(base, excl);
}

enum { SM_SUM = 0, SM_MIN = 1, SM_MAX = 2 };
template <int OP>
__device__ __forceinline__ int sm_op(int a, int b) {
  return OP == SM_SUM ? a + b : (OP == SM_MIN ? min(a, b) : max(a, b));
}
// block-wide reduction, the result in every thread
template <int OP>
__device__ __forceinline__ int sm_reduce(int v, int* tmp) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = sm_op<OP>(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = tmp[0];
#pragma unroll
  for (int w = 1; w < SM_WAVES; ++w) r = sm_op<OP>(r, tmp[w]);
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------------------------------------- tight box, area
// One block per row.  A ones-run that spans columns (rsp_run_cols) reaches the last row of one and the first row of the
// next, so its rows are [0, H).
__global__ __launch_bounds__(SM_THREADS) void rle_bbox_kernel(const uint32_t* __restrict__ counts,
                                                              const int32_t* __restrict__ n_in, int cap, int H,
                                                              int32_t* __restrict__ boxes, int32_t* __restrict__ area) {
  __shared__ int tmp[SM_WAVES];
  const int m = blockIdx.x, tid = threadIdx.x;
  int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = 0, y1 = 0, a = 0;
  for (RspRunWalk<SM_THREADS> r(rsp_run_row(counts, n_in, cap, m), tmp); r.next();) {
    if ((r.i & 1) && r.c > 0) {
      const RspRunCols q = rsp_run_cols(r.s, r.c, H);
      x0 = min(x0, q.xa);
      x1 = max(x1, q.xb + 1);
      y0 = min(y0, q.xa == q.xb ? q.ra : 0);
      y1 = max(y1, q.xa == q.xb ? q.rb + 1 : H);
      a += r.c;
    }
  }
  x0 = sm_reduce<SM_MIN>(x0, tmp);
  y0 = sm_reduce<SM_MIN>(y0, tmp);
  x1 = sm_reduce<SM_MAX>(x1, tmp);
  y1 = sm_reduce<SM_MAX>(y1, tmp);
  a = sm_reduce<SM_SUM>(a, tmp);
  if (tid == 0) {
    const bool empty = a == 0;
    boxes[4 * m] = empty ? 0 : x0;
    boxes[4 * m + 1] = empty ? 0 : y0;
    boxes[4 * m + 2] = empty ? 0 : x1;
    boxes[4 * m + 3] = empty ? 0 : y1;
    area[m] = a;
  }
}

// ------------------------------------------------------------------------------------------------- pair overlap
// The prefix workspace of every row (run_table.h: RspRunPrefix; searched with sm_find / sm_ones_before from there).
// One block per row, computed once however many pairs the row appears in.
__global__ __launch_bounds__(SM_THREADS) void rle_prefix_kernel(const uint32_t* __restrict__ counts,
                                                                const int32_t* __restrict__ n_in, int cap,
                                                                int32_t* __restrict__ ws) {
  __shared__ int tmp[SM_WAVES];
  const int m = blockIdx.x;
  const RspRunRow row = rsp_run_row(counts, n_in, cap, m);
  int32_t* w_row = ws + (int64_t)m * cap;
  RspRunPrefix<SM_THREADS> p;
  for (RspRunWalk<SM_THREADS> r(row, tmp); r.next();) p.step(r, row, w_row, tmp);
}

// pixels of the ones-run [s, s + c) inside columns [x0, x1), rows [y0, y1): first / middle / last column in closed form
__device__ __forceinline__ int sm_run_in_rect(int s, int c, int H, int x0, int y0, int x1, int y1) {
  const RspRunCols q = rsp_run_cols(s, c, H);
  if (q.xa == q.xb) return (q.xa >= x0 && q.xa < x1) ? max(0, min(q.rb + 1, y1) - max(q.ra, y0)) : 0;
  int a = 0;
  if (q.xa >= x0 && q.xa < x1) a += max(0, y1 - max(q.ra, y0));
  if (q.xb >= x0 && q.xb < x1) a += max(0, min(q.rb + 1, y1) - y0);
  a += max(0, min(q.xb, x1) - max(q.xa + 1, x0)) * (y1 - y0);
  return a;
}

__device__ __forceinline__ int sm_area_in_rect(const SmRow& r, int H, int x0, int y0, int x1, int y1) {
  if (r.nr == 0 || x1 <= x0 || y1 <= y0) return 0;
  // only the runs that can touch columns [x0, x1): from the last run starting at or before the first pixel of x0 to the
  // last run starting at or before the last pixel of x1 - 1
  const int lo = max(sm_find(r, x0 * H), 0), hi = sm_find(r, x1 * H - 1);
  int a = 0;
  for (int t = lo + (int)threadIdx.x; t <= hi; t += SM_THREADS) {
    const int c = (int)r.c[2 * t + 1];
    if (c > 0) a += sm_run_in_rect(r.ws[2 * t + 1], c, H, x0, y0, x1, y1);
  }
  return a;
}

// One block per pair.  inter: the lanes walk the ones-runs of the row that has FEWER of them and look each run's two ends
// up in the other row's prefix (two binary searches): one run against 50 000 costs one lane two searches.
__global__ __launch_bounds__(SM_THREADS) void rle_pair_overlap_kernel(const uint32_t* __restrict__ counts,
                                                                      const int32_t* __restrict__ n_in, int k, int cap,
                                                                      int H, int W, const int32_t* __restrict__ ws,
                                                                      const int32_t* __restrict__ pairs,
                                                                      const int32_t* __restrict__ rects,
                                                                      int32_t* __restrict__ out) {
  __shared__ int tmp[SM_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x;
  SmRow r[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int m = pairs[2 * p + q];
    const bool ok = m >= 0 && m < k;
    const int mm = ok ? m : 0;
    r[q].c = counts + (int64_t)mm * cap;
    r[q].ws = ws + (int64_t)mm * cap;
    r[q].nr = ok ? max(min(n_in[mm], cap), 0) >> 1 : 0;
  }
  const int x0 = min(max(rects[4 * p], 0), W), y0 = min(max(rects[4 * p + 1], 0), H);
  const int x1 = min(max(rects[4 * p + 2], 0), W), y1 = min(max(rects[4 * p + 3], 0), H);
  const SmRow& A = r[0].nr <= r[1].nr ? r[0] : r[1];
  const SmRow& B = r[0].nr <= r[1].nr ? r[1] : r[0];
  int inter = 0;
  if (B.nr > 0) {
    for (int t = tid; t < A.nr; t += SM_THREADS) {
      const int s = A.ws[2 * t + 1], e = s + (int)A.c[2 * t + 1];
      inter += sm_ones_before(B, e) - sm_ones_before(B, s);
    }
  }
  const int ai = sm_area_in_rect(r[0], H, x0, y0, x1, y1), aj = sm_area_in_rect(r[1], H, x0, y0, x1, y1);
  inter = sm_reduce<SM_SUM>(inter, tmp);
  const int si = sm_reduce<SM_SUM>(ai, tmp), sj = sm_reduce<SM_SUM>(aj, tmp);
  if (tid == 0) {
    out[3 * p] = inter;
    out[3 * p + 1] = si;
    out[3 * p + 2] = sj;
  }
}

// ------------------------------------------------------------------------------------------------- union
// One block per member: ones-run t of member mi goes to slot moff[mi] + t as key = group << 31 | start, end = start + count
// (start < 2^31).  Slots at or beyond `total` are not written.
__global__ __launch_bounds__(SM_THREADS) void rle_intervals_kernel(const uint32_t* __restrict__ counts,
                                                                   const int32_t* __restrict__ n_in, int k, int cap,
                                                                   const int32_t* __restrict__ members,
                                                                   const int32_t* __restrict__ member_group,
                                                                   const int64_t* __restrict__ moff, int64_t total,
                                                                   int64_t* __restrict__ keys, int32_t* __restrict__ ends) {
  __shared__ int tmp[SM_WAVES];
  const int mi = blockIdx.x;
  const int m = members[mi];
  if (m < 0 || m >= k) return;
  const RspRunRow row = rsp_run_row(counts, n_in, cap, m);
  const int64_t g = (int64_t)member_group[mi] << 31, base = moff[mi];
  for (RspRunWalk<SM_THREADS> r(row, tmp); r.next();) {
    const int64_t q = base + (r.i >> 1);
    if (r.i < row.n && (r.i & 1) && q >= 0 && q < total) {
      keys[q] = g | (int64_t)r.s;
      ends[q] = r.s + r.c;
    }
  }
}

// One block per group over its intervals sorted by start.  With pm(q) = the largest end among the intervals in front of q,
// interval q OPENS an output ones-run iff it is the group's first or start(q) > pm(q) (touching intervals merge: adjacent
// runs of one value are one run).  Pass 1 writes the stream POSITIONS of the run boundaries -- S_0, E_0, S_1, E_1, ...,
// and N when the last run ends before it: the opener of run r knows S_r = its start and E_{r-1} = pm.  Pass 2 turns
// positions into counts, out[i] -= out[i - 1], chunk by chunk from the top so that no chunk reads what another rewrote.
__global__ __launch_bounds__(SM_THREADS) void rle_union_kernel(const int64_t* __restrict__ keys,
                                                               const int32_t* __restrict__ ends, int64_t total,
                                                               const int64_t* __restrict__ iv_offs, uint32_t N,
                                                               uint32_t* __restrict__ counts_out,
                                                               int32_t* __restrict__ n_out, int cap_out) {
  __shared__ int tmp[SM_WAVES];
  const int g = blockIdx.x, tid = threadIdx.x;
  // clamped into [0, total], whatever the array holds
  const int64_t q0 = rsp_clamp64(iv_offs[g], 0, total), q1 = rsp_clamp64(iv_offs[g + 1], q0, total);
  uint32_t* out = counts_out + (int64_t)g * cap_out;
  int carry_max = 0;
  int64_t carry_slot = 0;
  for (int64_t qb = q0; qb < q1; qb += SM_THREADS) {
    const int64_t q = qb + tid;
    const bool valid = q < q1;
    const int64_t over = q - (q1 - 1), qc = q - (over & ~(over >> 63));     // min(q, q1 - 1) and the masks below: no branch
    const int s = (int)(keys[qc] & 0x7fffffffLL) & -(int)valid, e = ends[qc] & -(int)valid;   // in front of the shuffles
    int chunk_max, chunk_open;
    const int pm = max(carry_max, sm_excl_max_scan(e, tmp, &chunk_max));
    const bool opens = (int)valid & ((int)(q == q0) | (int)(s > pm));      // bitwise: no branch between the two scans
    const int64_t slot = carry_slot + rsp_block_excl_scan<SM_THREADS>(opens ? 1 : 0, tmp, &chunk_open);
    if (opens) {
      if (2 * slot < cap_out) out[2 * slot] = (uint32_t)s;
      if (slot > 0 && 2 * slot - 1 < cap_out) out[2 * slot - 1] = (uint32_t)pm;
    }
    carry_max = max(carry_max, chunk_max);
    carry_slot += chunk_open;
  }
  const uint32_t last_e = (uint32_t)carry_max;
  const int64_t needed = carry_slot == 0 ? 1 : 2 * carry_slot + (last_e < N ? 1 : 0);
  if (needed > cap_out) {                              // caller retries with a larger capacity
    if (tid == 0) n_out[g] = (int32_t)-needed;
    return;
  }
  if (tid == 0) {
    if (carry_slot == 0) {
      out[0] = N;
    } else {
      out[2 * carry_slot - 1] = last_e;
      if (last_e < N) out[2 * carry_slot] = N;
    }
    n_out[g] = (int32_t)needed;
  }
  __syncthreads();
  for (int i1 = (int)needed; i1 > 0; i1 -= SM_THREADS) {
    const int i = i1 - SM_THREADS + tid;
    uint32_t cur = 0u, prev = 0u;
    if (i >= 0) {
      cur = out[i];
      prev = i > 0 ? out[i - 1] : 0u;
    }
    __syncthreads();
    if (i >= 0) out[i] = cur - prev;
  }
}

}  // namespace

extern "C" int rsp_rle_bbox(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                            int32_t* boxes, int32_t* area, rsp_stream_t stream) {
  if (!counts || !n || !boxes || !area || k < 0 || cap < 1 || !rsp_run_canvas_ok(H, W)) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  hipLaunchKernelGGL(rle_bbox_kernel, dim3(k), dim3(SM_THREADS), 0, (hipStream_t)stream, counts, n, cap, H, boxes, area);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int64_t rsp_rle_pair_overlap_workspace_bytes(int32_t k, int32_t cap) {
  if (k < 0 || cap < 1) return 0;
  return (int64_t)(k > 0 ? k : 1) * cap * (int64_t)sizeof(int32_t);
}

extern "C" int rsp_rle_pair_overlap(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                                    const int32_t* pairs, const int32_t* rects, int32_t P, void* workspace, int32_t* out,
                                    rsp_stream_t stream) {
  if (!counts || !n || !workspace || k < 0 || cap < 1 || P < 0 || !rsp_run_canvas_ok(H, W)) return RSP_EINVAL;
  if (P > 0 && (!pairs || !rects || !out)) return RSP_EINVAL;
  if (P == 0 || k == 0) return RSP_OK;
  hipStream_t s = (hipStream_t)stream;
  int32_t* ws = static_cast<int32_t*>(workspace);
  hipLaunchKernelGGL(rle_prefix_kernel, dim3(k), dim3(SM_THREADS), 0, s, counts, n, cap, ws);
  RSP_CHECK_LAUNCH();
  hipLaunchKernelGGL(rle_pair_overlap_kernel, dim3(P), dim3(SM_THREADS), 0, s, counts, n, k, cap, H, W, ws, pairs, rects,
                     out);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_rle_intervals(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                                 const int32_t* members, const int32_t* member_group, const int64_t* member_offs, int32_t M,
                                 int64_t total, int64_t* keys, int32_t* ends, rsp_stream_t stream) {
  if (!counts || !n || k < 0 || cap < 1 || M < 0 || total < 0 || !rsp_run_canvas_ok(H, W)) return RSP_EINVAL;
  if (M > 0 && (!members || !member_group || !member_offs)) return RSP_EINVAL;
  if (total > 0 && (!keys || !ends)) return RSP_EINVAL;
  if (M == 0 || k == 0 || total == 0) return RSP_OK;
  hipLaunchKernelGGL(rle_intervals_kernel, dim3(M), dim3(SM_THREADS), 0, (hipStream_t)stream, counts, n, k, cap, members,
                     member_group, member_offs, total, keys, ends);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_rle_union(const int64_t* keys, const int32_t* ends, int64_t total, const int64_t* interval_offs, int32_t G,
                             int32_t H, int32_t W, uint32_t* counts_out, int32_t* n_out, int32_t cap_out,
                             rsp_stream_t stream) {
  if (G < 0 || total < 0 || cap_out < 2 || !rsp_run_canvas_ok(H, W)) return RSP_EINVAL;
  if (total > 0 && (!keys || !ends)) return RSP_EINVAL;
  if (G > 0 && (!interval_offs || !counts_out || !n_out)) return RSP_EINVAL;
  if (G == 0) return RSP_OK;
  hipLaunchKernelGGL(rle_union_kernel, dim3(G), dim3(SM_THREADS), 0, (hipStream_t)stream, keys, ends, total, interval_offs,
                     (uint32_t)((int64_t)H * W), counts_out, n_out, cap_out);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
