// The column-piece table of a run table ("Its two intermediates"), which polygon export (mask_polygons.hip) and
// the run-domain components (run_components.hip) read.  Input: a run table as rsp_mask_rle / rsp_rle_shift / rsp_rle_union
// write it, read through run_table.h; a row with n <= 0 has no pieces.
// PIECES.  A ones-run that crosses a column end is split into column pieces (x, y0, y1), y0 < y1; in stream order they
// are sorted by (x, y0), and the pieces of one column of a canonical row neither overlap nor touch.  The table is pieces
// int32 [4, P] = the planes x, y0, y1, instance, sorted by (instance, x, y0), + piece_offs int64 [k + 1]; a slot that no
// row filled keeps instance -1.  Two launches with the caller's exclusive sum in between; integer arithmetic, no atomics,
// every slot stored once: a second launch is bit-identical.
// Morphology keeps a writer of its own (rm_pieces_kernel, run_morphology.hip): it shrinks every piece by the row radius,
// drops the empty ones, adds the pad columns of a set border and writes the (instance * Wt + X, y0, y1) layout of its joins.
#include "rsp_common.h"
#include "run_table.h"

namespace {

constexpr int RP_THREADS = 256;

// One block per instance: the number of column pieces of its ones-runs.
__global__ __launch_bounds__(RP_THREADS) void run_pieces_count_kernel(const uint32_t* __restrict__ counts,
                                                                      const int32_t* __restrict__ n_in, int cap, int H,
                                                                      int32_t* __restrict__ piece_cnt) {
  __shared__ int tmp[RP_THREADS / 64];
  const int m = blockIdx.x, tid = threadIdx.x;
  int pieces = 0;
  for (RspRunWalk<RP_THREADS> r(rsp_run_row(counts, n_in, cap, m), tmp); r.next();) {
    if ((r.i & 1) && r.c > 0) {
      const RspRunCols q = rsp_run_cols(r.s, r.c, H);
      pieces += q.xb - q.xa + 1;
    }
  }
  int total;
  rsp_block_excl_scan<RP_THREADS>(pieces, tmp, &total);
  if (tid == 0) piece_cnt[m] = total;
}

// One block per instance: its pieces, in stream order, into slots piece_offs[m] .. piece_offs[m + 1].
__global__ __launch_bounds__(RP_THREADS) void run_pieces_kernel(const uint32_t* __restrict__ counts,
                                                                const int32_t* __restrict__ n_in, int cap, int H,
                                                                const int64_t* __restrict__ piece_offs, int64_t P,
                                                                int32_t* __restrict__ px, int32_t* __restrict__ py0,
                                                                int32_t* __restrict__ py1, int32_t* __restrict__ pinst) {
  __shared__ int tmp[RP_THREADS / 64];
  const int m = blockIdx.x;
  const int64_t base = piece_offs[m] < 0 ? 0 : piece_offs[m], end = piece_offs[m + 1] < P ? piece_offs[m + 1] : P;
  int64_t carry_p = 0;
  for (RspRunWalk<RP_THREADS> r(rsp_run_row(counts, n_in, cap, m), tmp); r.next();) {
    const int ones = r.c & -(int)(r.i & 1);
    const RspRunCols c = rsp_run_cols(r.s, ones, H);        // not used where ones == 0
    const int np = ones > 0 ? c.xb - c.xa + 1 : 0;           // a mask and a select up to the second scan: run_table.h
    int chunk_p;
    const int64_t q0 = base + carry_p + rsp_block_excl_scan<RP_THREADS>(np, tmp, &chunk_p);
    for (int j = 0; j < np; ++j) {
      const int64_t q = q0 + j;
      if (q < base || q >= end) break;
      px[q] = c.xa + j;
      py0[q] = j == 0 ? c.ra : 0;
      py1[q] = j == np - 1 ? c.rb + 1 : H;
      pinst[q] = m;
    }
    carry_p += chunk_p;
  }
}

}  // namespace

extern "C" int rsp_run_pieces_count(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                                    int32_t* piece_cnt, rsp_stream_t stream) {
  if (!counts || !n || !piece_cnt || k < 0 || cap < 1 || !rsp_run_canvas_ok(H, W)) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  hipLaunchKernelGGL(run_pieces_count_kernel, dim3(k), dim3(RP_THREADS), 0, (hipStream_t)stream, counts, n, cap, H, piece_cnt);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_run_pieces(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                              const int64_t* piece_offs, int64_t P, int32_t* pieces, rsp_stream_t stream) {
  if (!counts || !n || !piece_offs || k < 0 || cap < 1 || P < 0 || P > RSP_RUN_PIECES_MAX_PIECES || !rsp_run_canvas_ok(H, W))
    return RSP_EINVAL;
  if (P > 0 && !pieces) return RSP_EINVAL;
  if (k == 0 || P == 0) return RSP_OK;
  hipStream_t s = (hipStream_t)stream;
  int32_t *px = pieces, *py0 = pieces + P, *py1 = pieces + 2 * P, *pinst = pieces + 3 * P;
  if (hipMemsetAsync(pinst, 0xff, (size_t)P * sizeof(int32_t), s) != hipSuccess) return RSP_ELAUNCH;
  hipLaunchKernelGGL(run_pieces_kernel, dim3(k), dim3(RP_THREADS), 0, s, counts, n, cap, H, piece_offs, P, px, py0, py1, pinst);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
