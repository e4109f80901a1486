// Polygon rasterisation: rings of float64 vertices -> the exact COCO run tables that cocoapi's maskApi.c
// rleFrPoly gives for them, one table row per GROUP of rings, every group on its own (h, w) canvas.  The inverse of
// mask_polygons.hip: the rings of a mask, rasterised as one group, give the mask's run table back bit for bit.
//
// SCALE.   A vertex (x, y) becomes (int)(5 x + .5), (int)(5 y + .5): a C truncation toward zero.  A value beyond
// +-RSP_POLY_RASTER_MAX_COORD is pinned just outside that range before the conversion, so the conversion is defined for
// every input (a NaN goes to a bound); the caller reads the largest magnitude and rsp_poly_raster_crossings refuses it.
// WALK.    Edge j of a ring runs from its vertex j to vertex j + 1 (the last one back to the first) and yields
// max(|dx|, |dy|) + 1 walk points (u, v): rleFrPoly's loop, with its `flip` order, s = (ye - ys) / dx and (int)(ys + s t + .5).
// The walk points of a ring are the concatenation of its edges' points, the end point of an edge and the first of the next
// both included, as the reference has them.
// CROSSINGS.  One lane per walk point computes its own point and its predecessor in the ring's sequence (the very first
// point of a ring has none) and applies rleFrPoly's rule: u changed; xd = (min-side u + .5) / 5 - .5 is an integer in
// [0, w - 1]; yd = the smaller v, (yd + .5) / 5 - .5 clamped into [0, h] and ceiled.  It writes the key group << 32 |
// xd h + yd, or RSP_POLY_RASTER_NO_KEY, which sorts behind every key.  The caller sorts the keys.
// RUNS.    The tail of rleFrPoly (sort the positions with h w appended, take differences, drop a zero difference and add the
// next one to the previous run) has a closed form: a position p < h w is a run boundary iff its multiplicity is odd, and h w
// always is one; the counts are the differences of the boundaries, the first one the first boundary itself.  One block per
// group: a lane holds one sorted key, is the last of its value's stretch or not, finds the stretch's start by binary search
// and takes the parity; a block scan numbers the boundaries.  Boundaries increase strictly, so only count 0 can be zero.
// All arithmetic on coordinates is the reference's, in double, with contraction off: a fused multiply-add rounds once where
// the reference rounds twice and changes (int)(ys + s t + .5) on ties.  No atomics, no host reads.
#include "rsp_common.h"
#include "run_table.h"

#pragma clang fp contract(off)

namespace {

constexpr int PR_THREADS = 256;
constexpr int64_t PR_NO_KEY = RSP_POLY_RASTER_NO_KEY;
constexpr int PR_MAX_COORD = RSP_POLY_RASTER_MAX_COORD;

__device__ __forceinline__ int64_t pr_clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the last index i in [0, n) with offs[i] <= t (offs ascending, offs[0] <= t); n >= 1
__device__ __forceinline__ int64_t pr_last_le(const int64_t* __restrict__ offs, int64_t n, int64_t t) {
  int64_t lo = 0, up = n;                            // the answer lies in [lo, up)
  for (int it = 0; it < 64 && up - lo > 1; ++it) {
    const int64_t mid = lo + ((up - lo) >> 1);
    if (offs[mid] <= t) lo = mid; else up = mid;
  }
  return lo;
}

__device__ __forceinline__ int pr_scale(double x) {
  double s = 5.0 * x + .5;
  const double bound = (double)PR_MAX_COORD + 2.0;
  s = fmin(fmax(s, -bound), bound);                  // fmax / fmin return the other operand for a NaN
  return (int)s;
}

struct PrPoint {
  int u, v;
};

// walk point d of the edge (xs, ys) -> (xe, ye), 0 <= d <= max(|dx|, |dy|): maskApi.c rleFrPoly's inner loop
__device__ __forceinline__ PrPoint pr_point(int xs, int ys, int xe, int ye, int d) {
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
  if (flip) {
    int t = xs; xs = xe; xe = t;
    t = ys; ys = ye; ye = t;
  }
  PrPoint p;
  if (dx >= dy) {
    const double s = dx == 0 ? 0.0 : (double)(ye - ys) / dx;
    const int t = flip ? dx - d : d;
    p.u = t + xs;
    p.v = (int)(ys + s * t + .5);
  } else {
    const double s = (double)(xe - xs) / dy;
    const int t = flip ? dy - d : d;
    p.v = t + ys;
    p.u = (int)(xs + s * t + .5);
  }
  return p;
}

// One lane per vertex: its scaled coordinates.
__global__ __launch_bounds__(PR_THREADS) void pr_scale_kernel(const double* __restrict__ verts, int64_t V,
                                                              int32_t* __restrict__ scaled) {
  const int64_t j = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  if (j >= V) return;
  scaled[2 * j] = pr_scale(verts[2 * j]);
  scaled[2 * j + 1] = pr_scale(verts[2 * j + 1]);
}

// the ring of vertex j: the last r with ring_offs[r] <= j (rings without vertices lie in front of it or behind it)
__device__ __forceinline__ int64_t pr_ring_of(const int64_t* __restrict__ ring_offs, int64_t R, int64_t j) {
  return pr_last_le(ring_offs, R, j);
}

// the end vertex of edge j of a ring [v0, v1)
__device__ __forceinline__ int64_t pr_next(int64_t j, int64_t v0, int64_t v1) { return j + 1 < v1 ? j + 1 : v0; }

// One lane per vertex = per edge: its walk points.
__global__ __launch_bounds__(PR_THREADS) void pr_edge_kernel(const int32_t* __restrict__ scaled,
                                                             const int64_t* __restrict__ ring_offs, int64_t R, int64_t V,
                                                             int64_t* __restrict__ edge_pts) {
  const int64_t j = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  if (j >= V) return;
  const int64_t r = pr_ring_of(ring_offs, R, j);
  const int64_t v0 = pr_clamp64(ring_offs[r], 0, j), v1 = pr_clamp64(ring_offs[r + 1], j + 1, V);
  const int64_t e = pr_next(j, v0, v1);
  const int64_t dx = llabs((int64_t)scaled[2 * e] - scaled[2 * j]), dy = llabs((int64_t)scaled[2 * e + 1] - scaled[2 * j + 1]);
  edge_pts[j] = (dx > dy ? dx : dy) + 1;
}

// One lane per group: its pixels, or 2^31 for a canvas that no run table holds.
__global__ __launch_bounds__(PR_THREADS) void pr_canvas_kernel(const int32_t* __restrict__ group_hw, int G,
                                                               int64_t* __restrict__ group_px) {
  const int64_t g = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  if (g >= G) return;
  const int64_t h = group_hw[2 * g], w = group_hw[2 * g + 1];
  group_px[g] = (h < 1 || w < 1 || h * w > 0x7fffffffLL) ? 0x80000000LL : h * w;
}

// One lane per walk point, grid-strided.
__global__ __launch_bounds__(PR_THREADS) void pr_cross_kernel(const int32_t* __restrict__ scaled,
                                                              const int64_t* __restrict__ ring_offs,
                                                              const int32_t* __restrict__ ring_group,
                                                              const int32_t* __restrict__ group_hw,
                                                              const int64_t* __restrict__ edge_offs, int64_t R, int64_t V,
                                                              int G, int64_t T, int64_t* __restrict__ keys) {
  const int64_t stride = (int64_t)gridDim.x * PR_THREADS;
  for (int64_t t = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x; t < T; t += stride) {
    int64_t key = PR_NO_KEY;
    const int64_t j = pr_last_le(edge_offs, V, t);                      // edge_offs [V + 1], edge_offs[V] = T
    const int64_t d64 = t - edge_offs[j], cnt = edge_offs[j + 1] - edge_offs[j];
    const int64_t r = pr_ring_of(ring_offs, R, j);
    const int64_t v0 = pr_clamp64(ring_offs[r], 0, j), v1 = pr_clamp64(ring_offs[r + 1], j + 1, V);
    const int g = ring_group[r];
    const bool first = j == v0 && d64 == 0;                             // the ring's first point has no predecessor
    if (!first && d64 >= 0 && d64 < cnt && cnt <= 2LL * PR_MAX_COORD + 8 && g >= 0 && g < G) {
      const int d = (int)d64;
      const int64_t e = pr_next(j, v0, v1);
      const int xs = scaled[2 * j], ys = scaled[2 * j + 1], xe = scaled[2 * e], ye = scaled[2 * e + 1];
      const PrPoint p = pr_point(xs, ys, xe, ye, d);
      PrPoint q;
      if (d > 0) {
        q = pr_point(xs, ys, xe, ye, d - 1);
      } else {                                                          // the last point of the edge in front: it ends at (xs, ys)
        const int64_t b = j - 1;
        const int xb = scaled[2 * b], yb = scaled[2 * b + 1];
        const int db = max(abs(xs - xb), abs(ys - yb));
        q = pr_point(xb, yb, xs, ys, db);
      }
      const int h = group_hw[2 * g], w = group_hw[2 * g + 1];
      if (p.u != q.u) {
        double xd = (double)(p.u < q.u ? p.u : p.u - 1);
        xd = (xd + .5) / 5.0 - .5;
        if (floor(xd) == xd && xd >= 0 && xd <= w - 1) {
          double yd = (double)(p.v < q.v ? p.v : q.v);
          yd = (yd + .5) / 5.0 - .5;
          if (yd < 0) yd = 0; else if (yd > h) yd = h;
          yd = ceil(yd);
          key = ((int64_t)g << 32) | ((int64_t)xd * h + (int64_t)yd);
        }
      }
    }
    keys[t] = key;
  }
}

// One block per group over its sorted keys [key_offs[g], key_offs[g + 1]).
__global__ __launch_bounds__(PR_THREADS) void pr_runs_kernel(const int64_t* __restrict__ keys, int64_t K,
                                                             const int64_t* __restrict__ key_offs,
                                                             const int32_t* __restrict__ group_hw,
                                                             uint32_t* __restrict__ counts_out, int32_t* __restrict__ n_out,
                                                             int cap_out) {
  __shared__ int tmp[PR_THREADS / 64];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t q0 = pr_clamp64(key_offs[g], 0, K), q1 = pr_clamp64(key_offs[g + 1], q0, K);
  const int64_t N = (int64_t)group_hw[2 * g] * group_hw[2 * g + 1];
  uint32_t* out = counts_out + (int64_t)g * cap_out;
  int64_t carry = 0;
  for (int64_t qb = q0; qb < q1; qb += PR_THREADS) {
    const int64_t q = qb + tid;
    const bool valid = q < q1;
    const int64_t over = q - (q1 - 1), qc = q - (over & ~(over >> 63));        // min(q, q1 - 1): no branch in front of the scan
    const int64_t key = keys[qc];
    const int64_t pos = key & 0xffffffffLL;
    const int64_t nxt = keys[qc + 1 < q1 ? qc + 1 : qc];
    const int last = (int)(qc + 1 >= q1) | (int)(nxt != key);                  // the last key of its value
    int64_t lo = q0, up = qc;                                                  // the first key of its value
    for (int it = 0; it < 64 && lo < up; ++it) {
      const int64_t mid = lo + ((up - lo) >> 1);
      if (keys[mid] < key) lo = mid + 1; else up = mid;
    }
    const int odd = (int)((qc - lo + 1) & 1);
    const int flag = (int)valid & last & odd & (int)(pos < N);
    int chunk;
    const int64_t slot = carry + rsp_block_excl_scan<PR_THREADS>(flag, tmp, &chunk);
    if (flag && slot < cap_out) out[slot] = (uint32_t)pos;
    carry += chunk;
  }
  const int64_t needed = carry + 1;                                            // h w is always a boundary
  if (needed > cap_out) {                                                      // the caller retries with a larger capacity
    if (tid == 0) n_out[g] = (int32_t)-(needed < 0x7fffffffLL ? needed : 0x7fffffffLL);
    return;
  }
  if (tid == 0) {
    out[carry] = (uint32_t)N;
    n_out[g] = (int32_t)needed;
  }
  __syncthreads();
  // positions -> counts, chunk by chunk from the top so that no chunk reads what another rewrote (rle_union_kernel's pass 2)
  for (int i1 = (int)needed; i1 > 0; i1 -= PR_THREADS) {
    const int i = i1 - PR_THREADS + tid;
    uint32_t cur = 0u, prev = 0u;
    if (i >= 0) {
      cur = out[i];
      prev = i > 0 ? out[i - 1] : 0u;
    }
    __syncthreads();
    if (i >= 0) out[i] = cur - prev;
  }
}

inline unsigned pr_blocks(int64_t n) { return (unsigned)((n + PR_THREADS - 1) / PR_THREADS); }

}  // namespace

extern "C" int rsp_poly_raster_edges(const double* verts, const int64_t* ring_offs, const int32_t* group_hw, int64_t R, int64_t V,
                                     int32_t G, int32_t* scaled, int64_t* edge_pts, int64_t* group_px, rsp_stream_t stream) {
  if (R < 0 || V < 0 || G < 0 || G > RSP_POLY_RASTER_MAX_GROUPS || R > 0x7fffffffLL || V > RSP_POLY_RASTER_MAX_POINTS)
    return RSP_EINVAL;
  if (!ring_offs || (V > 0 && (R == 0 || !verts || !scaled || !edge_pts)) || (G > 0 && (!group_hw || !group_px))) return RSP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (G > 0) {
    hipLaunchKernelGGL(pr_canvas_kernel, dim3(pr_blocks(G)), dim3(PR_THREADS), 0, s, group_hw, G, group_px);
    RSP_CHECK_LAUNCH();
  }
  if (V == 0) return RSP_OK;
  hipLaunchKernelGGL(pr_scale_kernel, dim3(pr_blocks(V)), dim3(PR_THREADS), 0, s, verts, V, scaled);
  RSP_CHECK_LAUNCH();
  hipLaunchKernelGGL(pr_edge_kernel, dim3(pr_blocks(V)), dim3(PR_THREADS), 0, s, scaled, ring_offs, R, V, edge_pts);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_poly_raster_crossings(const int32_t* scaled, const int64_t* ring_offs, const int32_t* ring_group,
                                         const int32_t* group_hw, const int64_t* edge_offs, int64_t R, int64_t V, int32_t G,
                                         int64_t T, int64_t coord_max, int64_t pixels_max, int64_t* keys, rsp_stream_t stream) {
  if (R < 0 || V < 0 || G < 0 || G > RSP_POLY_RASTER_MAX_GROUPS || T < 0 || R > 0x7fffffffLL || V > RSP_POLY_RASTER_MAX_POINTS)
    return RSP_EINVAL;
  if (T > RSP_POLY_RASTER_MAX_POINTS || coord_max < 0 || coord_max > RSP_POLY_RASTER_MAX_COORD || pixels_max > 0x7fffffffLL)
    return RSP_EINVAL;
  if (T < V || (V == 0) != (T == 0)) return RSP_EINVAL;                        // every edge has a walk point
  if (T == 0) return RSP_OK;
  if (!scaled || !ring_offs || !ring_group || !group_hw || !edge_offs || !keys || R == 0 || G == 0) return RSP_EINVAL;
  const int64_t blocks = (T + PR_THREADS - 1) / PR_THREADS;
  hipLaunchKernelGGL(pr_cross_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(PR_THREADS), 0, (hipStream_t)stream,
                     scaled, ring_offs, ring_group, group_hw, edge_offs, R, V, G, T, keys);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_poly_raster_runs(const int64_t* keys, int64_t K, const int64_t* key_offs, const int32_t* group_hw, int32_t G,
                                    int64_t pixels_max, uint32_t* counts_out, int32_t* n_out, int32_t cap_out,
                                    rsp_stream_t stream) {
  if (G < 0 || G > RSP_POLY_RASTER_MAX_GROUPS || K < 0 || K > RSP_POLY_RASTER_MAX_POINTS || cap_out < 1 || pixels_max > 0x7fffffffLL) return RSP_EINVAL;
  if (K > 0 && !keys) return RSP_EINVAL;
  if (G > 0 && (!key_offs || !group_hw || !counts_out || !n_out)) return RSP_EINVAL;
  if (G == 0) return RSP_OK;
  hipLaunchKernelGGL(pr_runs_kernel, dim3(G), dim3(PR_THREADS), 0, (hipStream_t)stream, keys, K, key_offs, group_hw, counts_out,
                     n_out, cap_out);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
