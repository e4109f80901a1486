// Run-domain connected components: the 8-connected components of every mask of a run table, in work
// proportional to the number of runs.  Input: the column-piece table of a run table (run_pieces.hip); a row with n <= 0 has
// no pieces.
//
// PIECES.  As rsp_run_pieces writes them: a ones-run cut at column ends, (x, y0, y1, instance), y0 < y1, sorted by
// (instance, x, y0) in stream order; the pieces of one column neither overlap nor touch.
// ADJACENCY.  Pieces p of column x and q of column x + 1 of one instance are joined iff q.y0 <= p.y1 and q.y1 >= p.y0 (their
// closed row ranges, widened by one row, overlap: a diagonal contact joins).  The pieces of column x + 1 lie behind p in the
// sorted array; the first candidate is found by binary search on (x, y1), the rest follow it.  Two pieces of one ones-run
// that crosses a column end are joined by this rule or not at all.
// LABELLING.  Union-find over the piece indices: rc_link_kernel hangs the larger root under the smaller one with atomicMin,
// reads parents with relaxed agent-scope loads and compresses nothing; rc_flatten_kernel, a SEPARATE launch, gives every
// piece its root.  Parents only decrease and every value a slot has held is a piece of the same component, so whatever
// (older) value a read returns, the unions stay correct ("Why the seam merge is correct with incoherent L2s");
// the root is the LOWEST piece index of the component -- its first pixel in stream order -- whatever the schedule was.
// STATISTICS.  Areas, boxes and first pixels are integer add / min / max reductions: a second launch gives the same bits.
// Every find / union loop carries a step cap; reaching it sets `status` (a guard against a hang, not a path a correct run
// takes).  Every slot is checked against the row and the arrays: a non-canonical table gives a wrong answer, not a fault.
#include "rsp_common.h"
#include "run_table.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_INF = 0x7fffffff;
constexpr int64_t RC_MAX_PIECES = RSP_RUN_COMPONENTS_MAX_PIECES;

__device__ __forceinline__ int rc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(RC_THREADS) void rc_init_kernel(int P, int32_t* __restrict__ parent) {
  const int64_t p = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (p < P) parent[p] = (int32_t)p;
}

// the root of x under `cap` steps counted over the caller's whole operation; no compression: unions are in flight
__device__ __forceinline__ int rc_find(const int* parent, int P, int x, int& steps, int cap) {
  for (;;) {
    const int p = rc_ld(parent + x);
    if (p == x || p < 0 || p >= P || ++steps > cap) return x;
    x = p;
  }
}

// lock-free union (regions.hip's): the larger root goes under the smaller one; when the slot was no root any more, go on with
// what it held.  false: the cap was reached.
__device__ __forceinline__ bool rc_unite(int* parent, int P, int a, int b, int cap) {
  int steps = 0;
  for (;;) {
    a = rc_find(parent, P, a, steps, cap);
    b = rc_find(parent, P, b, steps, cap);
    if (steps > cap) return false;
    if (a == b) return true;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) return true;
    if (old < 0 || old >= P) return false;
    a = old;
    if (++steps > cap) return false;
  }
}

// One lane per piece: unions with the pieces of the next column that it touches.
__global__ __launch_bounds__(RC_THREADS) void rc_link_kernel(const int32_t* __restrict__ px, const int32_t* __restrict__ py0,
                                                             const int32_t* __restrict__ py1,
                                                             const int32_t* __restrict__ pinst,
                                                             const int64_t* __restrict__ piece_offs, int k, int P, int cap,
                                                             int32_t* __restrict__ parent, int32_t* __restrict__ status) {
  const int64_t p64 = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (p64 >= P) return;
  const int p = (int)p64;
  const int inst = pinst[p];
  if (inst < 0 || inst >= k) return;                                     // a slot no instance filled
  const int hi = (int)rsp_clamp64(piece_offs[inst + 1], 0, P);
  const int64_t xn = (int64_t)px[p] + 1;
  const int a = py0[p], b = py1[p];
  // the first piece behind p that lies in column x + 1 and reaches row a - 1 (y1 >= a), or in a later column
  int lo = p + 1, up = hi;
  for (int it = 0; it < 32 && lo < up; ++it) {
    const int mid = lo + ((up - lo) >> 1);
    const int64_t mx = px[mid];
    if (mx < xn || (mx == xn && py1[mid] < a)) lo = mid + 1; else up = mid;
  }
  bool ok = true;
  for (int q = lo; q < hi && px[q] == xn && py0[q] <= b; ++q) ok &= rc_unite(parent, P, p, q, cap);
  if (!ok) atomicMax(status, 1);
}

// SEPARATE LAUNCH, no union in flight: label = the root of every piece; root = 1 where a filled slot is its own root.
__global__ __launch_bounds__(RC_THREADS) void rc_flatten_kernel(const int32_t* __restrict__ pinst, int k, int P, int cap,
                                                                const int32_t* __restrict__ parent,
                                                                int32_t* __restrict__ label, int32_t* __restrict__ root,
                                                                int32_t* __restrict__ status) {
  const int64_t p64 = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (p64 >= P) return;
  const int p = (int)p64;
  const int inst = pinst[p];
  const bool live = inst >= 0 && inst < k;
  int steps = 0;
  const int r = live ? rc_find(parent, P, p, steps, cap) : p;
  if (steps > cap) atomicMax(status, 1);
  label[p] = live ? r : -1;
  root[p] = (live && r == p) ? 1 : 0;
}

__global__ __launch_bounds__(RC_THREADS) void rc_clear_kernel(int64_t C, int32_t* __restrict__ comp_area,
                                                              int32_t* __restrict__ comp_box, int32_t* __restrict__ comp_first,
                                                              int32_t* __restrict__ comp_inst) {
  const int64_t c = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (c >= C) return;
  comp_area[c] = 0;
  comp_box[4 * c] = RC_INF;
  comp_box[4 * c + 1] = RC_INF;
  comp_box[4 * c + 2] = 0;
  comp_box[4 * c + 3] = 0;
  comp_first[c] = RC_INF;
  comp_inst[c] = -1;
}

// One lane per piece: its component = (roots up to and including its root) - 1, and its share of the component's area,
// box and first row-major pixel.
__global__ __launch_bounds__(RC_THREADS) void rc_stats_kernel(const int32_t* __restrict__ px, const int32_t* __restrict__ py0,
                                                              const int32_t* __restrict__ py1,
                                                              const int32_t* __restrict__ pinst, int P, int W,
                                                              const int32_t* __restrict__ label,
                                                              const int32_t* __restrict__ root,
                                                              const int64_t* __restrict__ root_cum, int64_t C,
                                                              int32_t* __restrict__ piece_comp, int32_t* __restrict__ comp_area,
                                                              int32_t* __restrict__ comp_box, int32_t* __restrict__ comp_first,
                                                              int32_t* __restrict__ comp_inst) {
  const int64_t p64 = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (p64 >= P) return;
  const int p = (int)p64;
  const int r = label[p];
  int64_t c = -1;
  if (r >= 0 && r < P && root[r]) c = root_cum[r] - 1;
  if (c < 0 || c >= C) {
    piece_comp[p] = -1;
    return;
  }
  piece_comp[p] = (int32_t)c;
  const int x = px[p], a = py0[p], b = py1[p];
  atomicAdd(comp_area + c, b - a);
  atomicMin(comp_box + 4 * c, x);
  atomicMin(comp_box + 4 * c + 1, a);
  atomicMax(comp_box + 4 * c + 2, x + 1);
  atomicMax(comp_box + 4 * c + 3, b);
  atomicMin(comp_first + c, (int32_t)((int64_t)a * W + x));
  if (r == p) comp_inst[c] = pinst[p];
}

// One block per instance over its components: keep[c] = 1 for a component of at least min_area pixels; keep_largest: when
// the instance has none, its largest stays, among equals the one with the lowest comp_first (remove_small_regions' islands).
// changed[2 i + slot] = 1 when a smaller component exists.
__global__ __launch_bounds__(RC_THREADS) void rc_select_kernel(const int64_t* __restrict__ comp_offs, int64_t C,
                                                               const int32_t* __restrict__ comp_area,
                                                               const int32_t* __restrict__ comp_first, int min_area,
                                                               int keep_largest, int slot, int32_t* __restrict__ keep,
                                                               int32_t* __restrict__ changed) {
  __shared__ unsigned long long best[RC_THREADS];
  __shared__ int flags[RC_THREADS];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int64_t c0 = rsp_clamp64(comp_offs[i], 0, C), c1 = rsp_clamp64(comp_offs[i + 1], c0, C);
  unsigned long long mine = 0ull;
  int f = 0;                                                            // bit 0: a small component, bit 1: one that is not
  for (int64_t c = c0 + tid; c < c1; c += RC_THREADS) {
    const int area = comp_area[c];
    f |= area < min_area ? 1 : 2;
    const unsigned long long key = ((unsigned long long)(uint32_t)area << 32) | (0xFFFFFFFFu - (uint32_t)comp_first[c]);
    mine = key > mine ? key : mine;
  }
  best[tid] = mine;
  flags[tid] = f;
  __syncthreads();
  for (int o = RC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      best[tid] = best[tid + o] > best[tid] ? best[tid + o] : best[tid];
      flags[tid] |= flags[tid + o];
    }
    __syncthreads();
  }
  const unsigned long long top = best[0];
  const int all = flags[0];
  for (int64_t c = c0 + tid; c < c1; c += RC_THREADS) {
    const int area = comp_area[c];
    const unsigned long long key = ((unsigned long long)(uint32_t)area << 32) | (0xFFFFFFFFu - (uint32_t)comp_first[c]);
    keep[c] = (area >= min_area || (keep_largest && !(all & 2) && key == top)) ? 1 : 0;
  }
  if (tid == 0) changed[2 * i + slot] = all & 1;
}

inline unsigned rc_blocks(int64_t n) { return (unsigned)((n + RC_THREADS - 1) / RC_THREADS); }
inline int rc_step_cap(int64_t P) { return (int)(4 * P + 64 < 0x7ffffff0LL ? 4 * P + 64 : 0x7ffffff0LL); }

}  // namespace

extern "C" int64_t rsp_run_components_workspace_bytes(int32_t H, int32_t W, int64_t P) {
  if (!rsp_run_canvas_ok(H, W) || P < 0 || P > RC_MAX_PIECES) return -1;
  return (P > 0 ? P : 1) * (int64_t)sizeof(int32_t);
}

extern "C" int rsp_run_components_label(int32_t k, int32_t H, int32_t W, const int64_t* piece_offs, int64_t P, const int32_t* pieces,
                                        void* workspace, int32_t* label, int32_t* root, int32_t* status, rsp_stream_t stream) {
  if (!piece_offs || k < 0 || rsp_run_components_workspace_bytes(H, W, P) < 0) return RSP_EINVAL;
  if (P > 0 && (!pieces || !workspace || !label || !root || !status)) return RSP_EINVAL;
  if (k == 0 || P == 0) return RSP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int32_t *px = pieces, *py0 = pieces + P, *py1 = pieces + 2 * P, *pinst = pieces + 3 * P;
  int32_t* parent = static_cast<int32_t*>(workspace);
  const int steps = rc_step_cap(P);
  hipLaunchKernelGGL(rc_init_kernel, dim3(rc_blocks(P)), dim3(RC_THREADS), 0, s, (int)P, parent);
  RSP_CHECK_LAUNCH();
  hipLaunchKernelGGL(rc_link_kernel, dim3(rc_blocks(P)), dim3(RC_THREADS), 0, s, px, py0, py1, pinst, piece_offs, k, (int)P,
                     steps, parent, status);
  RSP_CHECK_LAUNCH();
  hipLaunchKernelGGL(rc_flatten_kernel, dim3(rc_blocks(P)), dim3(RC_THREADS), 0, s, pinst, k, (int)P, steps, parent, label, root,
                     status);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_run_components_stats(const int32_t* pieces, int64_t P, int32_t H, int32_t W, const int32_t* label,
                                        const int32_t* root, const int64_t* root_cum, int64_t C, int32_t* piece_comp,
                                        int32_t* comp_area, int32_t* comp_box, int32_t* comp_first, int32_t* comp_inst,
                                        rsp_stream_t stream) {
  if (rsp_run_components_workspace_bytes(H, W, P) < 0 || C < 0 || C > P) return RSP_EINVAL;
  if (P == 0) return RSP_OK;
  if (!pieces || !label || !root || !root_cum || !piece_comp) return RSP_EINVAL;
  if (C > 0 && (!comp_area || !comp_box || !comp_first || !comp_inst)) return RSP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int32_t *px = pieces, *py0 = pieces + P, *py1 = pieces + 2 * P, *pinst = pieces + 3 * P;
  if (C > 0) {
    hipLaunchKernelGGL(rc_clear_kernel, dim3(rc_blocks(C)), dim3(RC_THREADS), 0, s, C, comp_area, comp_box, comp_first, comp_inst);
    RSP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(rc_stats_kernel, dim3(rc_blocks(P)), dim3(RC_THREADS), 0, s, px, py0, py1, pinst, (int)P, W, label, root,
                     root_cum, C, piece_comp, comp_area, comp_box, comp_first, comp_inst);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_run_components_select(const int64_t* comp_offs, int32_t k, int64_t C, const int32_t* comp_area,
                                         const int32_t* comp_first, int32_t min_area, int32_t keep_largest, int32_t slot,
                                         int32_t* keep, int32_t* changed, rsp_stream_t stream) {
  if (k < 0 || C < 0 || C > RC_MAX_PIECES || min_area < 0 || slot < 0 || slot > 1) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  if (!comp_offs || !changed || (C > 0 && (!comp_area || !comp_first || !keep))) return RSP_EINVAL;
  hipLaunchKernelGGL(rc_select_kernel, dim3(k), dim3(RC_THREADS), 0, (hipStream_t)stream, comp_offs, C, comp_area, comp_first,
                     min_area, keep_largest ? 1 : 0, slot, keep, changed);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
