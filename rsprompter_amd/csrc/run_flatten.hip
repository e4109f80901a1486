// Planar instance layers: the masks of a run table made pairwise disjoint by a priority, in the run domain.
// With rank int32 [k] a permutation of 0 .. k - 1 (0 wins), row i of the result is F_i = M_i minus the union of the M_j with
// rank[j] < rank[i]: a pixel belongs to the covering instance of smallest rank.  No mask exists as bits; integer arithmetic,
// no atomics, every output slot stored once with a plain store: a second launch is bit-identical.
//
// INPUT.  The column-piece table of run_pieces.hip, pieces int32 [4, P] = the planes x, y0, y1, instance sorted by (instance,
// x, y0), and the caller's second copy of it sorted by column: skeys int64 [P] = (x * H + y0) << 31 | piece index, ascending
// (the keys are unique), and cpieces int32 [4, P] = the same planes in that order.  Pieces of one instance in one column do
// not overlap (they are pieces of one run stream); they may touch.
// COLUMNS (rsp_run_flatten_columns).  col_offs int32 [W + 1] = the first piece of every column in the sorted copy, by a
// search in skeys; reach int32 [P], reach[j] = the largest y1 among the pieces of j's column at or before j: a running
// maximum, non-decreasing within a column.  One wave per column, 64 pieces a chunk: a wave max-scan by shuffles and a carry.
// reach is what makes the search below valid: y1 alone is not sorted within a column (a long piece of one instance is
// followed by short pieces of others inside it), so "the first piece that ends behind y0" has no binary search; "the first
// piece up to which something ends behind y0" has, and every piece in front of it ends at or before y0.
// COUNT / WRITE (rsp_run_flatten_count, rsp_run_flatten_write).  One lane per piece (x, [y0, y1), i) in the instance-major
// order.  It searches column x for the first j with reach[j] > y0 and walks j upward while y0_j < y1 and cur < y1, cur = y0
// at first: a piece j with rank[inst_j] < rank[i] and y1_j > cur is a blocker; where y0_j > cur the interval [cur, min(y0_j,
// y1)) survives; then cur = max(cur, y1_j).  After the walk [cur, y1) survives when cur < y1.  The count pass stores the
// number of survivors, the write pass computes the same and stores them as rsp_rle_union's intervals, keys = instance << 31 |
// x * H + a, ends = x * H + b, into its own range [out_offs[p], out_offs[p + 1]).  The lanes run in piece order and a piece's
// survivors ascend, so the keys are in key order as they stand: no second sort, interval_offs[i] = out_offs[piece_offs[i]].
// A lane's work is the pieces of its column between the search point and y1: the overlap depth of the scene there; a
// column that every instance covers from end to end costs k per lane.
// PAINT (rsp_run_flatten_paint).  Intervals (instance << 31 | pixel start, pixel end) of DISJOINT masks -> an int32 label
// map, zeroed first, value ids[instance].  MEMORY ORDER: the map is written as int32 [W, H], the column-major stream of the
// run counts, in which a column interval [x * H + a, x * H + b) is contiguous: one wave per interval, lane l stores pixels
// start + l, start + l + 64, ...: consecutive lanes store consecutive words.  The caller returns the .T view ([H, W]).
// Offsets read from a caller's array are clamped, whatever the array holds: a wrong col_offs gives a wrong answer, not an
// out-of-bounds read.
#include "rsp_common.h"
#include "run_table.h"

namespace {

constexpr int RF_THREADS = 256;

// first index in [0, P) whose key is >= key (P: none)
__device__ __forceinline__ int64_t rf_lower_bound(const int64_t* __restrict__ skeys, int64_t P, int64_t key) {
  int64_t lo = 0, hi = P;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (skeys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave per column x in [0, W]; x == W only closes col_offs.
__global__ __launch_bounds__(RF_THREADS) void rf_columns_kernel(const int64_t* __restrict__ skeys,
                                                                const int32_t* __restrict__ cy1, int64_t P, int H, int W,
                                                                int32_t* __restrict__ col_offs, int32_t* __restrict__ reach) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int waves = (int)gridDim.x * (RF_THREADS / 64);
  for (int x = (int)blockIdx.x * (RF_THREADS / 64) + wave; x <= W; x += waves) {
    // every lane searches for itself: the same answer in all of them, so the trip count below is wave-uniform
    const int64_t lo = rf_lower_bound(skeys, P, ((int64_t)x * H) << 31);
    const int64_t hi = x < W ? rf_lower_bound(skeys, P, ((int64_t)(x + 1) * H) << 31) : lo;
    int carry = 0;
    for (int64_t base = lo; base < hi; base += 64) {
      const int64_t j = base + lane;
      // clamped index + masked value, no branch in front of the scan's shuffles (run_table.h); 0 is neutral: y1 >= 1
      int incl = cy1[j < hi ? j : hi - 1] & -(int)(j < hi);
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        incl = max(incl, lane >= o ? t : 0);
      }
      incl = max(incl, carry);
      carry = __shfl(incl, 63, 64);
      if (j < hi) reach[j] = incl;
    }
    if (lane == 0) col_offs[x] = (int32_t)lo;
  }
}

struct RfTables {
  const int32_t *px, *py0, *py1, *pinst;      // instance-major
  const int32_t *cy0, *cy1, *cinst;           // column-major
  const int32_t *col_offs, *reach, *rank;
  int64_t P;
  int k, H, W;
};

// the survivors [a, b) of piece p: emit(j, a, b) for the j-th; returns their number.  The count and the write pass both run it.
template <typename F>
__device__ __forceinline__ int rf_piece(const RfTables& T, int64_t p, int& inst, int& x, F emit) {
  inst = T.pinst[p];
  x = T.px[p];
  const int y0 = T.py0[p], y1 = T.py1[p];
  if (inst < 0 || inst >= T.k || x < 0 || x >= T.W || y0 < 0 || y1 > T.H || y0 >= y1) return 0;
  const int my_rank = T.rank[inst];
  const int lo = (int)rsp_clamp64(T.col_offs[x], 0, T.P), hi = (int)rsp_clamp64(T.col_offs[x + 1], lo, T.P);
  int j = lo, up = hi;                                     // the first piece of the column with reach > y0
  for (int it = 0; it < 32 && j < up; ++it) {
    const int mid = j + ((up - j) >> 1);
    if (T.reach[mid] <= y0) j = mid + 1; else up = mid;
  }
  int cur = y0, w = 0;
  for (; j < hi && cur < y1; ++j) {
    const int s = T.cy0[j];
    if (s >= y1) break;
    const int e = T.cy1[j], other = T.cinst[j];
    if (other < 0 || other >= T.k || T.rank[other] >= my_rank || e <= cur) continue;
    if (s > cur) emit(w++, cur, s);                        // s < y1 here
    cur = max(cur, e);
  }
  if (cur < y1) emit(w++, cur, y1);
  return w;
}

__global__ __launch_bounds__(RF_THREADS) void rf_count_kernel(const RfTables T, int32_t* __restrict__ cnt) {
  const int64_t stride = (int64_t)gridDim.x * RF_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x; p < T.P; p += stride) {
    int inst, x;
    cnt[p] = rf_piece(T, p, inst, x, [](int, int, int) {});
  }
}

__global__ __launch_bounds__(RF_THREADS) void rf_write_kernel(const RfTables T, const int64_t* __restrict__ out_offs,
                                                              int64_t total, int64_t* __restrict__ keys,
                                                              int32_t* __restrict__ ends) {
  const int64_t stride = (int64_t)gridDim.x * RF_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x; p < T.P; p += stride) {
    const int64_t q0 = rsp_clamp64(out_offs[p], 0, total), q1 = rsp_clamp64(out_offs[p + 1], q0, total);
    int inst = 0, x = 0;
    rf_piece(T, p, inst, x, [&](int j, int a, int b) {
      const int64_t q = q0 + j;
      if (q >= q1) return;
      const int px = x * T.H;
      keys[q] = ((int64_t)inst << 31) | (int64_t)(px + a);
      ends[q] = px + b;
    });
  }
}

// One wave per interval.
__global__ __launch_bounds__(RF_THREADS) void rf_paint_kernel(const int64_t* __restrict__ keys, const int32_t* __restrict__ ends,
                                                              int64_t total, const int32_t* __restrict__ ids, int k, int64_t HW,
                                                              int32_t* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (RF_THREADS / 64);
  for (int64_t q = (int64_t)blockIdx.x * (RF_THREADS / 64) + (threadIdx.x >> 6); q < total; q += waves) {
    const int64_t key = keys[q], inst = key >> 31;
    if (inst < 0 || inst >= k) continue;
    const int64_t s = key & 0x7fffffffLL, e = rsp_clamp64(ends[q], 0, HW);
    const int32_t v = ids[inst];
    for (int64_t p = s + lane; p < e; p += 64) labels[p] = v;
  }
}

inline int rf_grid(int64_t work, int per_block) {
  const int64_t b = (work + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

inline bool rf_shape_ok(int32_t k, int32_t H, int32_t W, int64_t P) {
  return k >= 0 && rsp_run_canvas_ok(H, W) && P >= 0 && P <= RSP_RUN_PIECES_MAX_PIECES;
}

inline bool rf_tables(const int32_t* pieces, const int32_t* cpieces, const int32_t* col_offs, const int32_t* reach,
                      const int32_t* rank, int64_t P, int32_t k, int32_t H, int32_t W, RfTables* T) {
  if (!rf_shape_ok(k, H, W, P)) return false;
  if (P > 0 && k > 0 && (!pieces || !cpieces || !col_offs || !reach || !rank)) return false;
  *T = RfTables{pieces, pieces + P, pieces + 2 * P, pieces + 3 * P, cpieces + P, cpieces + 2 * P, cpieces + 3 * P,
                col_offs, reach, rank, P, k, H, W};
  return true;
}

}  // namespace

extern "C" int rsp_run_flatten_columns(const int64_t* skeys, const int32_t* cpieces, int64_t P, int32_t H, int32_t W,
                                       int32_t* col_offs, int32_t* reach, rsp_stream_t stream) {
  if (!rf_shape_ok(0, H, W, P) || !col_offs) return RSP_EINVAL;
  if (P > 0 && (!skeys || !cpieces || !reach)) return RSP_EINVAL;
  hipLaunchKernelGGL(rf_columns_kernel, dim3(rf_grid((int64_t)W + 1, RF_THREADS / 64)), dim3(RF_THREADS), 0,
                     (hipStream_t)stream, skeys, cpieces + 2 * P, P, H, W, col_offs, reach);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_run_flatten_count(const int32_t* pieces, const int32_t* cpieces, const int32_t* col_offs,
                                     const int32_t* reach, const int32_t* rank, int64_t P, int32_t k, int32_t H, int32_t W,
                                     int32_t* cnt, rsp_stream_t stream) {
  RfTables T;
  if (!rf_tables(pieces, cpieces, col_offs, reach, rank, P, k, H, W, &T)) return RSP_EINVAL;
  if (P == 0 || k == 0) return RSP_OK;
  if (!cnt) return RSP_EINVAL;
  hipLaunchKernelGGL(rf_count_kernel, dim3(rf_grid(P, RF_THREADS)), dim3(RF_THREADS), 0, (hipStream_t)stream, T, cnt);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_run_flatten_write(const int32_t* pieces, const int32_t* cpieces, const int32_t* col_offs,
                                     const int32_t* reach, const int32_t* rank, int64_t P, int32_t k, int32_t H, int32_t W,
                                     const int64_t* out_offs, int64_t total, int64_t* keys, int32_t* ends, rsp_stream_t stream) {
  RfTables T;
  if (!rf_tables(pieces, cpieces, col_offs, reach, rank, P, k, H, W, &T) || total < 0 || total > 0x7fffffffLL) return RSP_EINVAL;
  if (P == 0 || k == 0 || total == 0) return RSP_OK;
  if (!out_offs || !keys || !ends) return RSP_EINVAL;
  hipLaunchKernelGGL(rf_write_kernel, dim3(rf_grid(P, RF_THREADS)), dim3(RF_THREADS), 0, (hipStream_t)stream, T, out_offs, total,
                     keys, ends);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_run_flatten_paint(const int64_t* keys, const int32_t* ends, int64_t total, const int32_t* ids, int32_t k,
                                     int32_t H, int32_t W, int32_t* labels, rsp_stream_t stream) {
  if (k < 0 || !rsp_run_canvas_ok(H, W) || total < 0 || total > 0x7fffffffLL || !labels) return RSP_EINVAL;
  if (total > 0 && k > 0 && (!keys || !ends || !ids)) return RSP_EINVAL;
  const int64_t HW = (int64_t)H * W;
  if (hipMemsetAsync(labels, 0, (size_t)HW * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return RSP_ELAUNCH;
  if (total == 0 || k == 0) return RSP_OK;
  hipLaunchKernelGGL(rf_paint_kernel, dim3(rf_grid(total, RF_THREADS / 64)), dim3(RF_THREADS), 0, (hipStream_t)stream, keys,
                     ends, total, ids, k, HW, labels);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
