// Oriented-box comparison: corners from the integer rectangles of mask_obb.hip, the IoU of two convex
// quadrilaterals in fp64, and mmcv's nms_rotated on flat arrays.
//
// THE BOX.  double [4][2] = (x, y) of four corners in order around a convex quadrilateral, either orientation.  Its doubled
// area is a2 = (v1 - v0) x (v2 - v0) + (v2 - v0) x (v3 - v0), taken on the differences so that it is a property of the box
// alone, wherever it lies; a2 < 0 reverses the order (v1 <-> v3).  A box with a non-finite coordinate or a2 == 0 is DEGENERATE:
// its IoU with everything is 0.0, it suppresses nothing and is kept.
//
// THE INTERSECTION is a CLOSED polygon.  Both boxes are translated by the mean of the first box's corners; the second box is
// clipped successively by the four half-planes of the first (Sutherland-Hodgman: a vertex is inside where d = e x (v - p) >= 0,
// a crossing of the edge v -> c is (c d_v - v d_c) / (d_v - d_c), computed ONCE and shared by the two pieces of boundary that
// meet there), which leaves at most 8 vertices, and one shoelace sum gives the doubled area.  The boundary-integral form (clip
// every edge of each box by the other box, sum p x q without a vertex list) computes the crossing of two nearly parallel edges
// twice, independently, and the boundary then fails to close: 1.4e-5 of IoU on nearly coincident boxes, 2e-15 here (§14.17).
// With small integer corners every operation is exact and the one division rounds the exact quotient.
//
// The vertex list of a lane lives in LDS (two buffers of 8 vertices x 16 B per lane: 32 KiB for the 128 lanes of a block, lane
// l at [vertex][l], so a wave's access is 64 consecutive doubles); a run-time indexed register array would go to scratch.
// A lane touches its own slots only: no barrier.  No atomics, no inline assembly; the library is built with -ffp-contract=off.
//
// NMS.  The key, the sort network and the greedy walk are nms_core.h's, shared with det.hip and query.hip.  obn_sort_kernel:
// one block sorts the keys in memory into the canonical order, score descending, original position ascending.
// obn_gather_kernel: boxes and labels in that order.  obn_pair_kernel: one wave per (row i, word w) of the n x ceil(n / 64)
// suppression mask, upper triangle only; lane l is box j = 64 w + l, its bit is set iff j > i, the labels agree (or
// class_agnostic) and iou(i, j) > iou_thr (strict); the word is the wave's ballot: the mask contract of nms_core.h.
// nms_walk_kernel: the greedy walk of box NMS, one wave, launched by nms_walk_launch on one candidate set whose size the sort
// kernel has written to the workspace.  A second launch gives the same bits: every word that is read was written by exactly
// one wave of this launch.
#include "rsp_common.h"
#include "nms_core.h"

namespace {

constexpr int OI_THREADS = 128;
constexpr int OI_MAXV = 8;
constexpr int OBN_SORT_THREADS = 1024;
static_assert(RSP_OBB_NMS_MAX <= RSP_NMS_MAX_CANDIDATES, "the large form of nms_walk holds every rotated candidate set");

struct OiBox {
  double x[4], y[4];
  double a2;          // doubled area, > 0; 0: degenerate
};

__device__ __forceinline__ double oi_cross(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

__device__ __forceinline__ OiBox oi_load(const double* __restrict__ p) {
  OiBox b;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b.x[i] = p[2 * i];
    b.y[i] = p[2 * i + 1];
    finite = finite && (b.x[i] - b.x[i] == 0.0) && (b.y[i] - b.y[i] == 0.0);
  }
  const double d1x = b.x[1] - b.x[0], d1y = b.y[1] - b.y[0], d2x = b.x[2] - b.x[0], d2y = b.y[2] - b.y[0];
  const double d3x = b.x[3] - b.x[0], d3y = b.y[3] - b.y[0];
  double a2 = oi_cross(d1x, d1y, d2x, d2y) + oi_cross(d2x, d2y, d3x, d3y);
  if (a2 < 0.0) {
    const double tx = b.x[1], ty = b.y[1];
    b.x[1] = b.x[3]; b.y[1] = b.y[3];
    b.x[3] = tx; b.y[3] = ty;
    a2 = -a2;
  }
  b.a2 = (finite && a2 > 0.0) ? a2 : 0.0;
  return b;
}

__device__ __forceinline__ double oi_min4(const double* v) { return fmin(fmin(v[0], v[1]), fmin(v[2], v[3])); }
__device__ __forceinline__ double oi_max4(const double* v) { return fmax(fmax(v[0], v[1]), fmax(v[2], v[3])); }

// the area of A n B (both not degenerate); sx / sy: the block's vertex buffers, t the lane's slot
__device__ __forceinline__ double oi_inter(const OiBox& A, const OiBox& B, double* sx, double* sy, int t) {
  // axis-aligned bounds that do not overlap (or only touch): no area, and nothing is clipped
  if (oi_max4(A.x) <= oi_min4(B.x) || oi_max4(B.x) <= oi_min4(A.x) || oi_max4(A.y) <= oi_min4(B.y) ||
      oi_max4(B.y) <= oi_min4(A.y))
    return 0.0;
  const double cx = (A.x[0] + A.x[1] + A.x[2] + A.x[3]) * 0.25, cy = (A.y[0] + A.y[1] + A.y[2] + A.y[3]) * 0.25;
  double ax[4], ay[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ax[i] = A.x[i] - cx;
    ay[i] = A.y[i] - cy;
    sx[i * OI_THREADS + t] = B.x[i] - cx;
    sy[i * OI_THREADS + t] = B.y[i] - cy;
  }
  int m = 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const double* ix = sx + (e & 1) * OI_MAXV * OI_THREADS + t;
    const double* iy = sy + (e & 1) * OI_MAXV * OI_THREADS + t;
    double* ox = sx + ((e & 1) ^ 1) * OI_MAXV * OI_THREADS + t;
    double* oy = sy + ((e & 1) ^ 1) * OI_MAXV * OI_THREADS + t;
    const double px = ax[e], py = ay[e], ex = ax[(e + 1) & 3] - px, ey = ay[(e + 1) & 3] - py;
    int out = 0;
    if (m > 0) {
      double vx = ix[(m - 1) * OI_THREADS], vy = iy[(m - 1) * OI_THREADS];
      double dv = ex * (vy - py) - ey * (vx - px);
      for (int i = 0; i < m; ++i) {
        const double ux = ix[i * OI_THREADS], uy = iy[i * OI_THREADS];
        const double du = ex * (uy - py) - ey * (ux - px);
        const bool in_u = du >= 0.0, in_v = dv >= 0.0;
        if (in_u != in_v) {                                          // the edge v -> u crosses the line: one point, made once
          const double den = dv - du;
          if (out < OI_MAXV) {
            ox[out * OI_THREADS] = (ux * dv - vx * du) / den;
            oy[out * OI_THREADS] = (uy * dv - vy * du) / den;
          }
          ++out;
        }
        if (in_u) {
          if (out < OI_MAXV) {
            ox[out * OI_THREADS] = ux;
            oy[out * OI_THREADS] = uy;
          }
          ++out;
        }
        vx = ux; vy = uy; dv = du;
      }
    }
    m = out < OI_MAXV ? out : OI_MAXV;   // (a convex polygon gains at most one vertex a half-plane: 8 after four)
  }
  if (m < 3) return 0.0;
  // four clips: the list is back in the first buffer
  double s = 0.0, vx = sx[(m - 1) * OI_THREADS + t], vy = sy[(m - 1) * OI_THREADS + t];
  for (int i = 0; i < m; ++i) {
    const double ux = sx[i * OI_THREADS + t], uy = sy[i * OI_THREADS + t];
    s += vx * uy - ux * vy;
    vx = ux; vy = uy;
  }
  return 0.5 * s;
}

// iou of two boxes as loaded; crowd: the union is the first box
__device__ __forceinline__ double oi_iou(const OiBox& A, const OiBox& B, bool crowd, double* sx, double* sy, int t) {
  if (A.a2 == 0.0 || B.a2 == 0.0) return 0.0;
  const double inter = oi_inter(A, B, sx, sy, t);
  if (!(inter > 0.0)) return 0.0;
  const double aa = 0.5 * A.a2, ab = 0.5 * B.a2;
  const double un = crowd ? aa : aa + ab - inter;
  if (!(un > 0.0)) return 0.0;
  return inter / un;
}

// ------------------------------------------------------------------------------------------------------------- corners
__global__ __launch_bounds__(256) void obb_corners_kernel(const int32_t* __restrict__ edge, const int64_t* __restrict__ q,
                                                          const int32_t* __restrict__ offset, int k, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= k) return;
  double* o = out + 8 * (int64_t)i;
  if (edge[i] < 0) {
    const double nan = __builtin_nan("");
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = nan;
    return;
  }
  const int64_t* r = q + 6 * (int64_t)i;
  const int64_t iex = r[0], iey = r[1];
  int64_t amin = r[2], amax = r[3], bmin = r[4], bmax = r[5];
  if (offset) {
    const int64_t oxi = offset[2 * i], oyi = offset[2 * i + 1];
    const int64_t da = oxi * iex + oyi * iey, db = -oxi * iey + oyi * iex;
    amin += da; amax += da; bmin += db; bmax += db;
  }
  // rle.obb_to_numpy's expression: exact numerators below 2^53, one IEEE division
  const double ex = (double)iex, ey = (double)iey, L = ex * ex + ey * ey;
  const double a[4] = {(double)amin, (double)amax, (double)amax, (double)amin};
  const double b[4] = {(double)bmin, (double)bmin, (double)bmax, (double)bmax};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[2 * j] = (a[j] * ex - b[j] * ey) / L;
    o[2 * j + 1] = (a[j] * ey + b[j] * ex) / L;
  }
}

// ---------------------------------------------------------------------------------------------------------- IoU blocks
__global__ __launch_bounds__(OI_THREADS) void obb_iou_kernel(const RspCocoUnit* __restrict__ units,
                                                             const double* __restrict__ dt_quad, int64_t n_dt,
                                                             const double* __restrict__ gt_quad, int64_t n_gt,
                                                             const uint8_t* __restrict__ gt_crowd, double* __restrict__ iou,
                                                             int64_t n_iou) {
  __shared__ double sx[2 * OI_MAXV * OI_THREADS], sy[2 * OI_MAXV * OI_THREADS];
  const RspCocoUnit u = units[blockIdx.x];
  const int t = threadIdx.x;
  if (u.nd <= 0 || u.ng <= 0 || u.dt0 < 0 || u.gt0 < 0 || u.out0 < 0 || u.dt0 + u.nd > n_dt || u.gt0 + u.ng > n_gt) return;
  const int64_t npair = (int64_t)u.nd * u.ng;
  if (u.out0 + npair > n_iou) return;
  for (int64_t p = t; p < npair; p += OI_THREADS) {
    const int64_t d = p / u.ng, g = p - d * u.ng;
    const int64_t di = u.dt0 + d, gi = u.gt0 + g;
    const OiBox A = oi_load(dt_quad + 8 * di), B = oi_load(gt_quad + 8 * gi);
    iou[u.out0 + p] = oi_iou(A, B, gt_crowd[gi] != 0, sx, sy, t);
  }
}

// ----------------------------------------------------------------------------------------------------------------- NMS
__global__ __launch_bounds__(OBN_SORT_THREADS) void obn_sort_kernel(const float* __restrict__ scores, int n, int nsort,
                                                                    unsigned long long* keys, int32_t* cnt) {
  if (threadIdx.x == 0) *cnt = n;                          // the walk reads the size of its candidate set from memory
  for (int i = threadIdx.x; i < nsort; i += OBN_SORT_THREADS) keys[i] = i < n ? nms_key(scores[i], i) : 0ull;
  __syncthreads();
  nms_sort_desc(keys, nsort);
}

__global__ __launch_bounds__(256) void obn_gather_kernel(const unsigned long long* __restrict__ keys,
                                                         const double* __restrict__ quad, const int32_t* __restrict__ labels,
                                                         int n, double* __restrict__ squad, int32_t* __restrict__ slab,
                                                         int32_t* __restrict__ order) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int src = nms_key_pos(keys[i]);
  src = src < 0 ? 0 : (src >= n ? n - 1 : src);          // (a real key always is in range)
  order[i] = src;
  slab[i] = labels[src];
#pragma unroll
  for (int j = 0; j < 8; ++j) squad[8 * (int64_t)i + j] = quad[8 * (int64_t)src + j];
}

// grid (W, ceil(n / 2)): wave `wv` of block (w, by) makes word w of row i = 2 by + wv
__global__ __launch_bounds__(OI_THREADS) void obn_pair_kernel(const double* __restrict__ squad, const int32_t* __restrict__ slab,
                                                              int n, int W, double iou_thr, int class_agnostic,
                                                              unsigned long long* __restrict__ mask) {
  __shared__ double sx[2 * OI_MAXV * OI_THREADS], sy[2 * OI_MAXV * OI_THREADS];
  const int t = threadIdx.x, lane = t & 63, w = blockIdx.x;
  const int i = blockIdx.y * (OI_THREADS / 64) + (t >> 6), j = 64 * w + lane;
  const bool row = i < n;
  int over = 0;
  if (row && j > i && j < n && (class_agnostic || slab[i] == slab[j])) {
    const OiBox A = oi_load(squad + 8 * (int64_t)i), B = oi_load(squad + 8 * (int64_t)j);
    over = (int)(oi_iou(A, B, false, sx, sy, t) > iou_thr);
  }
  const unsigned long long word = __ballot(over);                            // every lane of the wave arrives here
  if (row && lane == 0 && w >= (i >> 6)) mask[(int64_t)i * W + w] = word;    // every word the walk reads, the diagonal one too
}

struct ObnLayout {
  int64_t nsort, keys, squad, slab, order, mask, cnt, total;
  int W;
};
inline bool obn_layout(int64_t n, ObnLayout* L) {
  if (n < 0 || n > RSP_OBB_NMS_MAX) return false;
  L->nsort = 1;
  while (L->nsort < n) L->nsort <<= 1;
  L->W = (int)((n + 63) / 64);
  const int64_t n8 = (n + 1) / 2 * 8;                                        // n int32, rounded up to 8 bytes
  L->keys = 0;
  L->squad = L->keys + 8 * L->nsort;
  L->slab = L->squad + 64 * n;
  L->order = L->slab + n8;
  L->mask = L->order + n8;
  L->cnt = L->mask + 8 * n * L->W;                                           // one int32: n, for the walk
  L->total = L->cnt + 8 + 256;
  return true;
}

}  // namespace

extern "C" int rsp_obb_corners(const int32_t* edge, const int64_t* q, const int32_t* offset, int32_t k, double* corners,
                               rsp_stream_t stream) {
  if (k < 0) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  if (!edge || !q || !corners) return RSP_EINVAL;
  hipLaunchKernelGGL(obb_corners_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, (hipStream_t)stream, edge, q, offset,
                     (int)k, corners);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_obb_iou(const RspCocoUnit* units, int32_t n_units, const double* dt_quad, int64_t n_dt, const double* gt_quad,
                           int64_t n_gt, const uint8_t* gt_crowd, double* iou, int64_t n_iou, rsp_stream_t stream) {
  if (n_units < 0 || n_dt < 0 || n_gt < 0 || n_iou < 0) return RSP_EINVAL;
  if (n_units == 0) return RSP_OK;
  if (!units || (n_dt > 0 && !dt_quad) || (n_gt > 0 && (!gt_quad || !gt_crowd)) || (n_iou > 0 && !iou)) return RSP_EINVAL;
  hipLaunchKernelGGL(obb_iou_kernel, dim3((unsigned)n_units), dim3(OI_THREADS), 0, (hipStream_t)stream, units, dt_quad, n_dt,
                     gt_quad, n_gt, gt_crowd, iou, n_iou);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int64_t rsp_obb_nms_workspace_bytes(int32_t n) {
  ObnLayout L;
  return obn_layout(n, &L) ? L.total : -1;
}

extern "C" int rsp_obb_nms(const double* quad, const float* scores, const int32_t* labels, int32_t n, double iou_thr,
                           int32_t class_agnostic, void* workspace, int32_t* keep, int32_t* keep_cnt, rsp_stream_t stream) {
  ObnLayout L;
  if (!obn_layout(n, &L) || !(iou_thr >= 0.0) || !keep_cnt) return RSP_EINVAL;
  if (n > 0 && (!quad || !scores || !labels || !workspace || !keep)) return RSP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0)                                                                // nothing to walk, and there may be no workspace
    return hipMemsetAsync(keep_cnt, 0, sizeof(int32_t), s) == hipSuccess ? RSP_OK : RSP_ELAUNCH;
  char* ws = (char*)workspace;
  unsigned long long* keys = (unsigned long long*)(ws + L.keys);
  double* squad = (double*)(ws + L.squad);
  int32_t* slab = (int32_t*)(ws + L.slab);
  int32_t* order = (int32_t*)(ws + L.order);
  unsigned long long* mask = (unsigned long long*)(ws + L.mask);
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  hipLaunchKernelGGL(obn_sort_kernel, dim3(1), dim3(OBN_SORT_THREADS), 0, s, scores, (int)n, (int)L.nsort, keys, cnt);
  RSP_CHECK_LAUNCH();
  hipLaunchKernelGGL(obn_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, quad, labels, (int)n, squad, slab,
                     order);
  RSP_CHECK_LAUNCH();
  hipLaunchKernelGGL(obn_pair_kernel, dim3((unsigned)L.W, (unsigned)((n + OI_THREADS / 64 - 1) / (OI_THREADS / 64))),
                     dim3(OI_THREADS), 0, s, squad, slab, (int)n, L.W, iou_thr, (int)class_agnostic, mask);
  RSP_CHECK_LAUNCH();
  // one candidate set of n boxes, n rows to a set, every kept box put out
  const NmsWalkP p = {mask, order, cnt, (int)n, L.W, (int)n, keep, keep_cnt};
  nms_walk_launch(p, 1, s);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
