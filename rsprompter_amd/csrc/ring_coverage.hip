// Shared-border simplification: the rings of a PLANAR layer -- a run table whose rows are pairwise disjoint,
// what csrc/run_flatten.hip leaves -- simplified so that a border between two instances keeps the same vertices on both
// sides (GIS: coverage simplification).  tests/_ring_coverage_ref.py states the contract sequentially on a label map.
//
// OWNER.  owner(x, y) = the instance of pixel (x, y), -1 for background and outside the canvas.  The table is read through
// the column-ordered piece table of run_flatten.hip: cpieces int32 [4, P] = the planes x, y0, y1, instance sorted by (x, y0)
// and col_offs int32 [W + 1].  In a disjoint table the pieces of a column are disjoint and ascend in y0 AND y1, so owner is
// one binary search (the last piece with y0 <= y, which owns the pixel iff its y1 > y).  rc_check_kernel, one lane per piece,
// compares a piece with its successor in the column: bad[j] = 1 where they overlap (in a column sorted by y0 any overlap shows
// between some piece and its successor), 2 where two pieces of ONE instance touch (a zero count inside a row: not canonical).
// NODES.  A lattice point p in [0, W] x [0, H] with the pixels a = (px - 1, py - 1), b = (px, py - 1), c = (px - 1, py),
// d = (px, py) around it is a node iff [a != b] + [b != d] + [d != c] + [c != a] >= 3 on owners.  On a straight ring segment
// both inside pixels belong to the ring's instance, so a point strictly inside it is a node iff the FAR-side owner changes
// there.  Rings run clockwise on screen around the set pixel: travelling right at row Y the far pixels are row Y - 1, down at
// column X column X, left row Y, up column X - 1.
// rc_nodes_count_kernel / rc_nodes_write_kernel, one lane per ring segment v_i -> v_{i+1}: the four-pixel rule at v_i, then the
// change points of the far owner inside the segment -- a vertical segment searches the far column for its first piece and walks
// the pieces (two touching pieces of different instances are ONE change point), a horizontal one looks the owner of every unit
// step up.  count stores 1 + the change points and where the segment's first node sits (0: v_i, 1: its first change point, -1:
// none); the host's exclusive sum gives every segment its slots and every ring its first node visit; write stores the noded
// ring ROTATED to begin there: nverts int32 [Vn, 2], nflag uint8 [Vn] (1: node) and nother int32 [Vn], the far owner of the
// step that leaves the vertex.  A lane's work is the unit steps of its segment times the search (horizontal) or the pieces the
// segment passes (vertical).
// MARK.  rs_mark_wave_kernel<true> / rs_mark_block_kernel<T, true> of ring_mark.h: keep = nflag on entry.
// OTHER.  rc_other_kernel compacts nother with the pos / sums / csum of rsp_ring_simplify_survive / _write.
// Integer arithmetic, every output slot stored once with a plain store, no atomics: a second launch is bit-identical.  Every
// index read from a caller's array is clamped into the array it addresses: a wrong array gives a wrong answer, not a fault.
#include "rsp_common.h"
#include "ring_mark.h"

namespace {

constexpr int RC_THREADS = 256;

struct RcTables {
  const int32_t *cx, *cy0, *cy1, *cinst, *col_offs;      // column-major pieces
  int64_t P;
  int k, H, W;
};

__device__ __forceinline__ int rc_inst(const RcTables& T, int j) {
  const int inst = T.cinst[j];
  return inst >= 0 && inst < T.k ? inst : -1;
}
// the pieces [lo, hi) of column x (0 <= x < W)
__device__ __forceinline__ void rc_column(const RcTables& T, int x, int& lo, int& hi) {
  lo = (int)rs_clamp64(T.col_offs[x], 0, T.P);
  hi = (int)rs_clamp64(T.col_offs[x + 1], lo, T.P);
}
// the first piece of [lo, hi) with y0 > y
__device__ __forceinline__ int rc_upper(const RcTables& T, int lo, int hi, int y) {
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    if (T.cy0[mid] <= y) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int rc_owner(const RcTables& T, int x, int y) {
  if (x < 0 || x >= T.W || y < 0 || y >= T.H) return -1;
  int lo, hi;
  rc_column(T, x, lo, hi);
  const int j = rc_upper(T, lo, hi, y) - 1;
  return j >= lo && T.cy1[j] > y ? rc_inst(T, j) : -1;
}

// Segment i of the ring [s, e): emit(t, x, y, flag, other) for its vertex v_i (t = 0) and the nodes inside it (t = 1 ..) in the
// order of travel; returns their number.  *first = where the first node of the segment sits (0, 1 or -1).  nchg: the change
// points as the count pass found them (the write pass numbers a segment travelled downward in the coordinate from its end).
template <typename F>
__device__ __forceinline__ int rc_segment(const RcTables& T, const int32_t* __restrict__ verts, int64_t i, int64_t s, int64_t e,
                                          int nchg, int* first, F emit) {
  const int64_t nx = i + 1 < e ? i + 1 : s;
  const int x0 = verts[2 * i], y0 = verts[2 * i + 1], x1 = verts[2 * nx], y1 = verts[2 * nx + 1];
  const int a = rc_owner(T, x0 - 1, y0 - 1), b = rc_owner(T, x0, y0 - 1), c = rc_owner(T, x0 - 1, y0), d = rc_owner(T, x0, y0);
  const int flag0 = (a != b) + (b != d) + (d != c) + (c != a) >= 3 ? 1 : 0;
  const bool horiz = y0 == y1 && x0 != x1, vert = x0 == x1 && y0 != y1;
  const bool asc = horiz ? x1 > x0 : y1 > y0;
  int n = 0, own_lo = -1, own = -1;                          // change points; the far owner of the lowest and of the current step
  // change point q (ascending) at coordinate cc, the far owner goes from `before` to `after`
  auto change = [&](int cc, int before, int after) {
    emit(asc ? n + 1 : nchg - n, horiz ? cc : x0, horiz ? y0 : cc, 1, asc ? after : before);
    ++n;
  };
  if (horiz) {
    const int lo = max(min(x0, x1), 0), hi = min(max(x0, x1), T.W), fy = asc ? y0 - 1 : y0;
    own_lo = own = rc_owner(T, lo, fy);
    for (int x = lo + 1; x < hi; ++x) {
      const int o = rc_owner(T, x, fy);
      if (o != own) change(x, own, o);
      own = o;
    }
  } else if (vert) {
    const int lo = max(min(y0, y1), 0), hi = min(max(y0, y1), T.H), fx = asc ? x0 : x0 - 1;
    if (fx >= 0 && fx < T.W && lo < hi) {
      int pl, ph;
      rc_column(T, fx, pl, ph);
      int j = rc_upper(T, pl, ph, lo) - 1;                    // the piece that may hold row lo
      bool in_piece = j >= pl && T.cy1[j] > lo;
      if (!in_piece) ++j;                                     // else: the next piece above lo
      own_lo = own = in_piece ? rc_inst(T, j) : -1;
      while (j < ph) {                                        // j: the piece the walk is in, or the next one
        int y, o;
        if (in_piece) {
          y = T.cy1[j];
          ++j;
          in_piece = j < ph && T.cy0[j] <= y;                 // touching (or, in a table that is not disjoint, overlapping)
          o = in_piece ? rc_inst(T, j) : -1;
        } else {
          y = T.cy0[j];
          in_piece = true;
          o = rc_inst(T, j);
        }
        if (y >= hi) break;
        if (o != own && y > lo) change(y, own, o);
        own = o;
      }
    }
  }
  emit(0, x0, y0, flag0, asc ? own_lo : own);
  *first = flag0 ? 0 : (n > 0 ? 1 : -1);
  return n + 1;
}

// the ring of vertex i: the last r with ring_offs[r] <= i; [s, e) = its vertices, empty where i is in no ring
__device__ __forceinline__ int64_t rc_ring_of(const int64_t* __restrict__ ring_offs, int64_t R, int64_t V, int64_t i, int64_t& s,
                                              int64_t& e) {
  int64_t lo = 0, hi = R;
  for (int it = 0; it < 64 && hi - lo > 1; ++it) {
    const int64_t mid = (lo + hi) >> 1;
    if (ring_offs[mid] <= i) lo = mid; else hi = mid;
  }
  s = rs_clamp64(ring_offs[lo], 0, V);
  e = rs_clamp64(ring_offs[lo + 1], s, V);
  if (i < s || i >= e) s = e = i;
  return lo;
}

__global__ __launch_bounds__(RC_THREADS) void rc_check_kernel(const RcTables T, int32_t* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * RC_THREADS;
  for (int64_t j = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; j < T.P; j += stride) {
    int v = 0;
    if (j + 1 < T.P && T.cx[j] == T.cx[j + 1]) {
      if (T.cy0[j + 1] < T.cy1[j]) v = 1;
      else if (T.cy0[j + 1] == T.cy1[j] && T.cinst[j + 1] == T.cinst[j]) v = 2;
    }
    bad[j] = v;
  }
}

__global__ __launch_bounds__(RC_THREADS) void rc_nodes_count_kernel(const RcTables T, const int32_t* __restrict__ verts,
                                                                    const int64_t* __restrict__ ring_offs, int64_t R, int64_t V,
                                                                    int32_t* __restrict__ cnt, int32_t* __restrict__ first) {
  const int64_t stride = (int64_t)gridDim.x * RC_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < V; i += stride) {
    int64_t s, e;
    rc_ring_of(ring_offs, R, V, i, s, e);
    int f = -1, n = 1;
    if (s < e) n = rc_segment(T, verts, i, s, e, 0, &f, [](int, int, int, int, int) {});
    cnt[i] = n;
    first[i] = f;
  }
}

__global__ __launch_bounds__(RC_THREADS) void rc_nodes_write_kernel(const RcTables T, const int32_t* __restrict__ verts,
                                                                    const int64_t* __restrict__ ring_offs, int64_t R, int64_t V,
                                                                    const int64_t* __restrict__ noff, const int64_t* __restrict__ rot,
                                                                    int64_t Vn, int32_t* __restrict__ nverts,
                                                                    uint8_t* __restrict__ nflag, int32_t* __restrict__ nother) {
  const int64_t stride = (int64_t)gridDim.x * RC_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < V; i += stride) {
    int64_t s, e;
    const int64_t r = rc_ring_of(ring_offs, R, V, i, s, e);
    if (s >= e) continue;
    const int64_t base = rs_clamp64(noff[s], 0, Vn), end = rs_clamp64(noff[e], base, Vn), mn = end - base;
    if (mn == 0) continue;
    const int64_t j0 = rs_clamp64(noff[i] - base, 0, mn - 1), f = rs_clamp64(rot[r], 0, mn - 1);
    const int64_t have = rs_clamp64(noff[i + 1] - noff[i], 1, mn);
    int unused;
    rc_segment(T, verts, i, s, e, (int)(have - 1), &unused, [&](int t, int x, int y, int flag, int other) {
      if (t < 0 || t >= have) return;
      const int64_t slot = base + (j0 + t - f + mn) % mn;                // in [base, end): inside the arrays
      nverts[2 * slot] = x;
      nverts[2 * slot + 1] = y;
      nflag[slot] = (uint8_t)flag;
      nother[slot] = other;
    });
  }
}

// One lane per noded vertex: rs_write_kernel's slot, for nother.
__global__ __launch_bounds__(RC_THREADS) void rc_other_kernel(const int64_t* __restrict__ ring_offs, int64_t R, int64_t V,
                                                              const uint8_t* __restrict__ keep, const int32_t* __restrict__ pos,
                                                              const int64_t* __restrict__ flags, const int64_t* __restrict__ csum,
                                                              int64_t V2, const int32_t* __restrict__ nother,
                                                              int32_t* __restrict__ other_out) {
  const int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (i >= V || !keep[i]) return;
  int64_t s, e;
  const int64_t r = rc_ring_of(ring_offs, R, V, i, s, e);
  if (s >= e || !flags[r]) return;
  const int64_t end = csum[R + r], first = end - flags[R + r], slot = first + pos[i];
  if (slot >= first && slot < end && slot >= 0 && slot < V2) other_out[slot] = nother[i];
}

inline int rc_grid(int64_t work) {
  const int64_t b = (work + RC_THREADS - 1) / RC_THREADS;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

inline bool rc_canvas_ok(int32_t H, int32_t W) {
  return H >= 1 && W >= 1 && H <= RSP_RING_COVERAGE_MAX_SIDE && W <= RSP_RING_COVERAGE_MAX_SIDE && (int64_t)H * W <= 0x7fffffffLL;
}

inline bool rc_tables(const int32_t* cpieces, const int32_t* col_offs, int64_t P, int32_t k, int32_t H, int32_t W, RcTables* T) {
  if (!rc_canvas_ok(H, W) || k < 0 || P < 0 || P > RSP_RUN_PIECES_MAX_PIECES || !col_offs || (P > 0 && !cpieces)) return false;
  *T = RcTables{cpieces, cpieces + P, cpieces + 2 * P, cpieces + 3 * P, col_offs, P, k, H, W};
  return true;
}

}  // namespace

extern "C" int rsp_ring_coverage_check(const int32_t* cpieces, int64_t P, int32_t H, int32_t W, int32_t* bad,
                                       rsp_stream_t stream) {
  if (!rc_canvas_ok(H, W) || P < 0 || P > RSP_RUN_PIECES_MAX_PIECES) return RSP_EINVAL;
  if (P == 0) return RSP_OK;
  if (!cpieces || !bad) return RSP_EINVAL;
  const RcTables T{cpieces, cpieces + P, cpieces + 2 * P, cpieces + 3 * P, nullptr, P, 0, H, W};
  hipLaunchKernelGGL(rc_check_kernel, dim3(rc_grid(P)), dim3(RC_THREADS), 0, (hipStream_t)stream, T, bad);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_ring_coverage_nodes_count(const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V,
                                             const int32_t* cpieces, const int32_t* col_offs, int64_t P, int32_t k, int32_t H,
                                             int32_t W, int32_t* cnt, int32_t* first, rsp_stream_t stream) {
  RcTables T;
  if (!rc_tables(cpieces, col_offs, P, k, H, W, &T) || R < 0 || R > 0x7fffffffLL || V < 0 || V > 0x7fffffffLL) return RSP_EINVAL;
  if (V == 0 || R == 0) return RSP_OK;
  if (!verts || !ring_offs || !cnt || !first) return RSP_EINVAL;
  hipLaunchKernelGGL(rc_nodes_count_kernel, dim3(rc_grid(V)), dim3(RC_THREADS), 0, (hipStream_t)stream, T, verts, ring_offs, R, V,
                     cnt, first);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_ring_coverage_nodes_write(const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V,
                                             const int32_t* cpieces, const int32_t* col_offs, int64_t P, int32_t k, int32_t H,
                                             int32_t W, const int64_t* noff, const int64_t* rot, int64_t Vn, int32_t* nverts,
                                             uint8_t* nflag, int32_t* nother, rsp_stream_t stream) {
  RcTables T;
  if (!rc_tables(cpieces, col_offs, P, k, H, W, &T) || R < 0 || R > 0x7fffffffLL || V < 0 || V > 0x7fffffffLL || Vn < V ||
      Vn > 0x7fffffffLL)
    return RSP_EINVAL;
  if (V == 0 || R == 0) return RSP_OK;
  if (!verts || !ring_offs || !noff || !rot || !nverts || !nflag || !nother) return RSP_EINVAL;
  hipLaunchKernelGGL(rc_nodes_write_kernel, dim3(rc_grid(V)), dim3(RC_THREADS), 0, (hipStream_t)stream, T, verts, ring_offs, R, V,
                     noff, rot, Vn, nverts, nflag, nother);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_ring_coverage_mark(const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V, int64_t tol2_q8,
                                      int32_t H, int32_t W, int32_t variant, uint8_t* keep, int32_t* pos, int32_t* kept_cnt,
                                      int64_t* area2, int32_t* rounds, rsp_stream_t stream) {
  return rs_mark<true>(verts, ring_offs, R, V, tol2_q8, H, W, variant, keep, pos, kept_cnt, area2, rounds, (hipStream_t)stream);
}

extern "C" int rsp_ring_coverage_other(const int64_t* ring_offs, int64_t R, int64_t V, const uint8_t* keep, const int32_t* pos,
                                       const int64_t* sums, const int64_t* csum, int64_t V2, const int32_t* nother,
                                       int32_t* other_out, rsp_stream_t stream) {
  if (R < 0 || R > 0x7fffffffLL || V < 0 || V > 0x7fffffffLL || V2 < 0 || V2 > V) return RSP_EINVAL;
  if (V2 == 0 || R == 0) return RSP_OK;
  if (!ring_offs || !keep || !pos || !sums || !csum || !nother || !other_out) return RSP_EINVAL;
  hipLaunchKernelGGL(rc_other_kernel, dim3((unsigned)((V + RC_THREADS - 1) / RC_THREADS)), dim3(RC_THREADS), 0,
                     (hipStream_t)stream, ring_offs, R, V, keep, pos, sums, csum, V2, nother, other_out);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
