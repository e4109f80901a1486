// Run-domain morphology: erosion of every mask of a run table by the (2 r + 1)^2 square, and with it
// dilation, opening, closing and the boundary band of Boundary IoU, in work proportional to the column pieces times log r.
// No mask exists as bits.  Input: a CANONICAL run table (rsp_rle_union's rows; ops.py canonicalises first), read through
// run_table.h; a row with n <= 0 has no pieces.
//
// TABLES.  A table is a list of intervals (col, y0, y1), y0 < y1, sorted by (col, y0), the intervals of one column disjoint
// and not touching; col = instance * Wt + X addresses column X of an instance on a strip of Wt columns, and a CSR array
// offs int32 [k Wt + 1] (the caller's searchsorted over col) gives the intervals of each column.
// LEVEL 1 (rsp_run_morph_pieces).  The column pieces of every ones-run (run_pieces.hip's cut), each shrunk to
// [y0 + ry, y1 - ry); with border = 1 an end on the canvas edge stays, and `pad` full columns [0, H) stand on either side of
// the canvas (Wt = W + 2 pad): the outside of the canvas counts as set.  Empty results are dropped.
// JOIN (rsp_run_morph_join).  One lane per interval of the left table A at column X; its partner list is column X + shift of
// the right table B, found through offs, and in it the first and last interval that overlap by two binary searches, each
// bounded by the length of the list.  op 0 writes the intersections -- with A = B = T_a and shift = a this is the window
// doubling T_2a(X) = T_a(X) & T_a(X + a), the intersection over columns [X, X + 2a); a lane whose window X + span leaves the
// strip writes nothing (never read for border = 1, empty by definition for border = 0).  Intersection is idempotent, so the
// window of 2 rx + 1 columns is T_p(X) & T_p(X + 2 rx + 1 - p) for the largest power of two p <= 2 rx + 1: two overlapping
// windows, one more join whatever the digits of 2 r + 1 are.  op 1 writes A minus B (the band: pieces minus eroded).
// Both are a count pass, the caller's exclusive sum, and a write pass that computes the same and stores every slot of its
// own range [offs[i], offs[i + 1]) once with a plain store; no atomics, a second launch gives the same bits.  The write
// pass emits either a table again or the (instance << 31 | pixel start, pixel end) intervals of rsp_rle_union, which are
// in key order as they stand.
#include "rsp_common.h"
#include "run_table.h"

namespace {

constexpr int RM_THREADS = 256;

// ------------------------------------------------------------------------------------------------------------ level 1
// the shrunk piece [a, b) of the piece [y0, y1)
__device__ __forceinline__ void rm_shrink(int y0, int y1, int H, int ry, int border, int& a, int& b) {
  a = (border & (int)(y0 == 0)) ? 0 : y0 + ry;
  b = (border & (int)(y1 == H)) ? H : y1 - ry;
}

// One block per row.  WRITE = false: cnt[m] = 2 pad + the pieces that survive the shrink.  WRITE = true: the row's slots
// [piece_offs[m], piece_offs[m + 1]): pad left columns, the surviving pieces in stream order, pad right columns.
template <bool WRITE>
__global__ __launch_bounds__(RM_THREADS) void rm_pieces_kernel(const uint32_t* __restrict__ counts,
                                                               const int32_t* __restrict__ n_in, int cap, int H, int W, int ry,
                                                               int pad, int border, const int64_t* __restrict__ piece_offs,
                                                               int64_t P, int32_t* __restrict__ cnt,
                                                               int32_t* __restrict__ col, int32_t* __restrict__ oy0,
                                                               int32_t* __restrict__ oy1) {
  __shared__ int tmp[RM_THREADS / 64];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int Wt = W + 2 * pad;
  const int col0 = m * Wt;
  int64_t base = 0, end = 0;
  if (WRITE) {
    base = rsp_clamp64(piece_offs[m], 0, P);
    end = rsp_clamp64(piece_offs[m + 1], base, P);
  }
  int am, bm;                                              // a column the run covers from end to end
  rm_shrink(0, H, H, ry, border, am, bm);
  const int mid_ok = (int)(am < bm);
  int64_t carry = 0;
  for (RspRunWalk<RM_THREADS> r(rsp_run_row(counts, n_in, cap, m), tmp); r.next();) {
    const int ones = r.c & -(int)(r.i & 1);
    const RspRunCols c = rsp_run_cols(r.s, ones, H);        // not used where ones == 0
    const int np = ones > 0 ? c.xb - c.xa + 1 : 0;           // a mask and selects up to the scan: run_table.h
    int a0, b0, a1, b1;
    rm_shrink(c.ra, np == 1 ? c.rb + 1 : H, H, ry, border, a0, b0);          // the first piece
    rm_shrink(0, c.rb + 1, H, ry, border, a1, b1);                            // the last one, when np > 1
    const int first_ok = (int)(np >= 1) & (int)(a0 < b0), last_ok = (int)(np >= 2) & (int)(a1 < b1);
    const int n_mid = np > 2 ? (np - 2) & -mid_ok : 0;
    const int ns = first_ok + last_ok + n_mid;
    int chunk;
    const int64_t q0 = base + pad + carry + rsp_block_excl_scan<RM_THREADS>(ns, tmp, &chunk);
    if (WRITE) {
      int64_t q = q0;
      if (first_ok) {
        if (q >= base && q < end) { col[q] = col0 + pad + c.xa; oy0[q] = a0; oy1[q] = b0; }
        ++q;
      }
      for (int j = 0; j < n_mid; ++j, ++q) {
        if (q < base || q >= end) break;
        col[q] = col0 + pad + c.xa + 1 + j; oy0[q] = am; oy1[q] = bm;
      }
      q = q0 + first_ok + n_mid;
      if (last_ok && q >= base && q < end) { col[q] = col0 + pad + c.xb; oy0[q] = a1; oy1[q] = b1; }
    }
    carry += chunk;
  }
  if (WRITE) {
    for (int j = tid; j < pad; j += RM_THREADS) {
      const int64_t ql = base + j, qr = base + pad + carry + j;
      if (ql < end) { col[ql] = col0 + j; oy0[ql] = 0; oy1[ql] = H; }
      if (qr >= base && qr < end) { col[qr] = col0 + pad + W + j; oy0[qr] = 0; oy1[qr] = H; }
    }
  } else if (tid == 0) {
    const int64_t total = 2 * (int64_t)pad + carry;
    cnt[m] = (int32_t)(total > 0x7fffffffLL ? 0x7fffffffLL : total);
  }
}

// ------------------------------------------------------------------------------------------------------------ join
struct RmJoin {
  const int32_t *a_col, *a_y0, *a_y1;
  int64_t PA;
  int Wa;
  const int32_t *b_offs, *b_y0, *b_y1;
  int64_t PB;
  int k, Wb, shift, span, out_shift, Wout, H;
};

// the intervals [s, e) of lane i: emit(j, s, e) for the j-th; returns their number.  The count and the write pass both run it.
template <typename F>
__device__ __forceinline__ int rm_join_lane(const RmJoin& J, int op, int64_t i, int& inst, int& xo, F emit) {
  const int c = J.a_col[i], y0 = J.a_y0[i], y1 = J.a_y1[i];
  inst = c / J.Wa;
  const int X = c - inst * J.Wa, XB = X + J.shift;
  xo = X + J.out_shift;
  if (c < 0 || inst >= J.k || y0 >= y1 || xo < 0 || xo >= J.Wout) return 0;
  const bool have_b = XB >= 0 && XB < J.Wb && X + J.span <= J.Wa;
  if (!have_b && op == 0) return 0;
  int lo = 0, hi = 0;
  if (have_b) {
    const int64_t bc = (int64_t)inst * J.Wb + XB;
    lo = (int)rsp_clamp64(J.b_offs[bc], 0, J.PB);
    hi = (int)rsp_clamp64(J.b_offs[bc + 1], lo, J.PB);
  }
  // first = the first interval of the list that ends behind y0; last = the first at or behind it that starts at or behind y1
  int first = lo, up = hi;
  for (int it = 0; it < 32 && first < up; ++it) {
    const int mid = first + ((up - first) >> 1);
    if (J.b_y1[mid] <= y0) first = mid + 1; else up = mid;
  }
  int last = first;
  up = hi;
  for (int it = 0; it < 32 && last < up; ++it) {
    const int mid = last + ((up - last) >> 1);
    if (J.b_y0[mid] < y1) last = mid + 1; else up = mid;
  }
  if (op == 0) {
    for (int j = first; j < last; ++j) emit(j - first, max(y0, J.b_y0[j]), min(y1, J.b_y1[j]));
    return last - first;
  }
  int cur = y0, w = 0;                                    // A minus B: the gaps in front of, between and behind B's intervals
  for (int j = first; j < last; ++j) {
    const int s = J.b_y0[j];
    if (s > cur) emit(w++, cur, s);
    cur = max(cur, J.b_y1[j]);
  }
  if (cur < y1) emit(w++, cur, y1);
  return w;
}

__global__ __launch_bounds__(RM_THREADS) void rm_join_count_kernel(const RmJoin J, int op, int32_t* __restrict__ cnt) {
  const int64_t stride = (int64_t)gridDim.x * RM_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x; i < J.PA; i += stride) {
    int inst, xo;
    cnt[i] = rm_join_lane(J, op, i, inst, xo, [](int, int, int) {});
  }
}

// emit = 0: a table (o_col = instance * Wout + column, o_y0, o_y1); emit = 1: rsp_rle_union's intervals (keys, ends)
__global__ __launch_bounds__(RM_THREADS) void rm_join_write_kernel(const RmJoin J, int op, const int64_t* __restrict__ offs,
                                                                   int64_t total, int emit_keys, int32_t* __restrict__ o_col,
                                                                   int32_t* __restrict__ o_y0, int32_t* __restrict__ o_y1,
                                                                   int64_t* __restrict__ keys, int32_t* __restrict__ ends) {
  const int64_t stride = (int64_t)gridDim.x * RM_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x; i < J.PA; i += stride) {
    const int64_t q0 = rsp_clamp64(offs[i], 0, total), q1 = rsp_clamp64(offs[i + 1], q0, total);
    int inst = 0, xo = 0;
    rm_join_lane(J, op, i, inst, xo, [&](int j, int s, int e) {
      const int64_t q = q0 + j;
      if (q >= q1) return;
      if (emit_keys) {
        const int px = xo * J.H;
        keys[q] = ((int64_t)inst << 31) | (int64_t)(px + s);
        ends[q] = px + e;
      } else {
        o_col[q] = inst * J.Wout + xo;
        o_y0[q] = s;
        o_y1[q] = e;
      }
    });
  }
}

inline int rm_grid(int64_t work) {
  const int64_t b = (work + RM_THREADS - 1) / RM_THREADS;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// the strip of a level-1 table: k (W + 2 pad) column numbers in 32 bits
inline bool rm_strip_ok(int32_t k, int64_t Wt) { return Wt > 0 && (int64_t)k * Wt <= 0x7fffffffLL; }

inline bool rm_pieces_args_ok(const void* counts, const void* n, int32_t k, int32_t cap, int32_t H, int32_t W, int32_t ry,
                              int32_t pad, int32_t border) {
  if (k < 0 || cap < 1 || !rsp_run_canvas_ok(H, W) || ry < 0 || ry > H || pad < 0 || pad > W || (border != 0 && border != 1))
    return false;
  if (!rm_strip_ok(k, (int64_t)W + 2 * (int64_t)pad)) return false;
  return k == 0 || (counts && n);
}

inline bool rm_join_args_ok(int32_t op, const void* a_col, const void* a_y0, const void* a_y1, int64_t PA, int32_t Wa,
                            const void* b_offs, const void* b_y0, const void* b_y1, int64_t PB, int32_t k, int32_t Wb,
                            int32_t shift, int32_t span) {
  // a negative shift: the difference with a column to the left (op 1, the E- of run_disc.hip); op 0's windows grow to the right
  if ((op != 0 && op != 1) || PA < 0 || PB < 0 || PA > 0x7fffffffLL || PB > 0x7fffffffLL || k < 0 || span < 1) return false;
  if (shift < 0 && op != 1) return false;
  if (!rm_strip_ok(k > 0 ? k : 1, Wa) || !rm_strip_ok(k > 0 ? k : 1, Wb)) return false;
  if (PA > 0 && (!a_col || !a_y0 || !a_y1 || !b_offs)) return false;
  return PB == 0 || (b_y0 && b_y1);
}

}  // namespace

extern "C" int rsp_run_morph_pieces_count(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                                          int32_t ry, int32_t pad, int32_t border, int32_t* piece_cnt, rsp_stream_t stream) {
  if (!rm_pieces_args_ok(counts, n, k, cap, H, W, ry, pad, border)) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  if (!piece_cnt) return RSP_EINVAL;
  hipLaunchKernelGGL(rm_pieces_kernel<false>, dim3(k), dim3(RM_THREADS), 0, (hipStream_t)stream, counts, n, cap, H, W, ry, pad,
                     border, (const int64_t*)nullptr, (int64_t)0, piece_cnt, (int32_t*)nullptr, (int32_t*)nullptr,
                     (int32_t*)nullptr);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_run_morph_pieces(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                                    int32_t ry, int32_t pad, int32_t border, const int64_t* piece_offs, int64_t P, int32_t* col,
                                    int32_t* y0, int32_t* y1, rsp_stream_t stream) {
  if (!rm_pieces_args_ok(counts, n, k, cap, H, W, ry, pad, border) || P < 0 || P > 0x7fffffffLL) return RSP_EINVAL;
  if (k == 0 || P == 0) return RSP_OK;
  if (!piece_offs || !col || !y0 || !y1) return RSP_EINVAL;
  hipLaunchKernelGGL(rm_pieces_kernel<true>, dim3(k), dim3(RM_THREADS), 0, (hipStream_t)stream, counts, n, cap, H, W, ry, pad,
                     border, piece_offs, P, (int32_t*)nullptr, col, y0, y1);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_run_morph_join_count(int32_t op, const int32_t* a_col, const int32_t* a_y0, const int32_t* a_y1, int64_t PA,
                                        int32_t Wa, const int32_t* b_offs, const int32_t* b_y0, const int32_t* b_y1, int64_t PB,
                                        int32_t k, int32_t Wb, int32_t shift, int32_t span, int32_t out_shift, int32_t Wout,
                                        int32_t* cnt, rsp_stream_t stream) {
  if (!rm_join_args_ok(op, a_col, a_y0, a_y1, PA, Wa, b_offs, b_y0, b_y1, PB, k, Wb, shift, span)) return RSP_EINVAL;
  if (!rm_strip_ok(k > 0 ? k : 1, Wout)) return RSP_EINVAL;
  if (PA == 0 || k == 0) return RSP_OK;
  if (!cnt) return RSP_EINVAL;
  const RmJoin J{a_col, a_y0, a_y1, PA, Wa, b_offs, b_y0, b_y1, PB, k, Wb, shift, span, out_shift, Wout, 1};
  hipLaunchKernelGGL(rm_join_count_kernel, dim3(rm_grid(PA)), dim3(RM_THREADS), 0, (hipStream_t)stream, J, op, cnt);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_run_morph_join(int32_t op, const int32_t* a_col, const int32_t* a_y0, const int32_t* a_y1, int64_t PA,
                                  int32_t Wa, const int32_t* b_offs, const int32_t* b_y0, const int32_t* b_y1, int64_t PB,
                                  int32_t k, int32_t Wb, int32_t shift, int32_t span, const int64_t* out_offs, int64_t total,
                                  int32_t out_shift, int32_t Wout, int32_t H, int32_t emit_keys, int32_t* o_col, int32_t* o_y0,
                                  int32_t* o_y1, int64_t* keys, int32_t* ends, rsp_stream_t stream) {
  if (!rm_join_args_ok(op, a_col, a_y0, a_y1, PA, Wa, b_offs, b_y0, b_y1, PB, k, Wb, shift, span)) return RSP_EINVAL;
  if (total < 0 || total > 0x7fffffffLL || H < 1 || (emit_keys != 0 && emit_keys != 1) || !rm_strip_ok(k > 0 ? k : 1, Wout))
    return RSP_EINVAL;
  if (emit_keys && !rsp_run_canvas_ok(H, Wout)) return RSP_EINVAL;
  if (PA == 0 || k == 0 || total == 0) return RSP_OK;
  if (!out_offs || (emit_keys ? (!keys || !ends) : (!o_col || !o_y0 || !o_y1))) return RSP_EINVAL;
  const RmJoin J{a_col, a_y0, a_y1, PA, Wa, b_offs, b_y0, b_y1, PB, k, Wb, shift, span, out_shift, Wout, H};
  hipLaunchKernelGGL(rm_join_write_kernel, dim3(rm_grid(PA)), dim3(RM_THREADS), 0, (hipStream_t)stream, J, op, out_offs, total,
                     emit_keys, o_col, o_y0, o_y1, keys, ends);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
