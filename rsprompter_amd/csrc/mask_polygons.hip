// Polygon export: run tables -> exact vector rings on the pixel-corner lattice, in work proportional to
// the number of runs.  Input: the column-piece table of a run table (run_pieces.hip); a row with n <= 0 has no rings.
//
// PIECES.  As rsp_run_pieces writes them: a ones-run cut at column ends, (x, y0, y1, instance), y0 < y1, sorted by
// (instance, x, y0); the pieces of one column neither overlap nor touch.
// EDGES.  Piece p owns six edge slots 6 p + j.  j = 0: its top side (x, y0) -> (x + 1, y0); j = 1: its bottom side
// (x + 1, y1) -> (x, y1).  j = 2 + 2 side + end: the vertical edge on line X = x (side 0, neighbour column x - 1) or
// X = x + 1 (side 1, neighbour x + 1) that begins at ya = y0 (end 0) or ya = y1 (end 1) and runs down to the next place yb
// where either column changes; it exists where exactly one of the two columns is set in between, points down (X, ya) ->
// (X, yb) with the set column on the left and up (X, yb) -> (X, ya) with it on the right, and where both columns change at
// ya the LEFT column owns it.  Such a segment changes direction only at a saddle, so every vertical edge is maximal, every
// vertical edge is followed and preceded by a horizontal one, and the corners of a ring are the two ends of its vertical
// edges.
// LINKS.  A vertical edge looks up the horizontal edge after it and the one before it (binary searches in the two columns
// next to its line; at a saddle the successor is the edge of the OTHER pixel: foreground 8-connected) and writes succ of
// both; a horizontal edge that goes straight on writes its own.  Every slot is written once, by one lane.
// RANKING.  Pointer jumping over succ gives every edge the smallest start vertex of its ring (the ring's identity and
// its first vertex, which a ring visits once); a second pass over the predecessors, cut at that vertex, gives the number
// of corners and the doubled area in front of every edge.  Both take `rounds` launches, 2^rounds >= the longest ring.
// No lane walks a ring.  Integer arithmetic; no atomics: a second launch is bit-identical.
#include "rsp_common.h"
#include "run_table.h"

namespace {

constexpr int MP_THREADS = 256;
constexpr int64_t MP_NOKEY = 0x7fffffffffffffffLL;
constexpr int MP_INF = 0x7fffffff;

struct MpCol {              // the pieces of one instance
  const int32_t* x;
  const int32_t* y0;
  const int32_t* y1;
  int lo, hi;
};

// last piece of the instance with (x, y0) <= (c, y); lo - 1: none
__device__ __forceinline__ int mp_find_le(const MpCol& P, int c, int y) {
  int lo = P.lo - 1, hi = P.hi - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo + 1) >> 1);
    const int mx = P.x[mid];
    if (mx < c || (mx == c && P.y0[mid] <= y)) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// the piece of column c whose top is y / whose bottom is y; -1: none
__device__ __forceinline__ int mp_top_at(const MpCol& P, int c, int y) {
  const int q = mp_find_le(P, c, y);
  return (q >= P.lo && P.x[q] == c && P.y0[q] == y) ? q : -1;
}
__device__ __forceinline__ int mp_bot_at(const MpCol& P, int c, int y) {
  if (y <= 0) return -1;
  const int q = mp_find_le(P, c, y - 1);
  return (q >= P.lo && P.x[q] == c && P.y1[q] == y) ? q : -1;
}
// column c just below y: set or not, the next y at which it changes (MP_INF: never), and whether it changes AT y
__device__ __forceinline__ void mp_col_state(const MpCol& P, int c, int y, bool* fg, int* next, bool* change_at) {
  const int q = mp_find_le(P, c, y);
  const bool in_col = q >= P.lo && P.x[q] == c;
  const bool more = q + 1 < P.hi && P.x[q + 1] == c;
  if (in_col && y < P.y1[q]) {
    *fg = true;
    *next = P.y1[q];
    *change_at = P.y0[q] == y;
  } else {
    *fg = false;
    *next = more ? P.y0[q + 1] : MP_INF;
    *change_at = in_col && P.y1[q] == y;
  }
}

// ------------------------------------------------------------------------------------------------- edges and links
__device__ __forceinline__ int64_t mp_min64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t mp_max64(int64_t a, int64_t b) { return a > b ? a : b; }
// the horizontal edge slot of the first piece that exists (slot 0 = top side, 1 = bottom side); -1: neither
__device__ __forceinline__ int64_t mp_pick(int p1, int slot1, int p2, int slot2) {
  return p1 >= 0 ? 6 * (int64_t)p1 + slot1 : (p2 >= 0 ? 6 * (int64_t)p2 + slot2 : -1);
}
__device__ __forceinline__ void mp_link(int32_t* succ, int64_t E, int64_t from, int64_t to) {
  if (from >= 0 && from < E && to >= 0 && to < E) succ[from] = (int32_t)to;
}

// One lane per piece.  ekey = start x * (H + 1) + start y (MP_NOKEY: the slot holds no edge); eoth = the coordinate of the
// end vertex that differs from the start's (x of a horizontal edge, y of a vertical one).
__global__ __launch_bounds__(MP_THREADS) void mp_edges_kernel(const int32_t* __restrict__ px, const int32_t* __restrict__ py0,
                                                              const int32_t* __restrict__ py1,
                                                              const int32_t* __restrict__ pinst,
                                                              const int64_t* __restrict__ piece_offs, int k, int64_t P, int H,
                                                              int64_t* __restrict__ ekey, int32_t* __restrict__ eoth,
                                                              int32_t* __restrict__ succ) {
  const int64_t p = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
  if (p >= P) return;
  const int inst = pinst[p];
  if (inst < 0 || inst >= k) {                                          // a slot no instance filled: no edges
    for (int j = 0; j < 6; ++j) { ekey[6 * p + j] = MP_NOKEY; eoth[6 * p + j] = 0; }
    return;
  }
  MpCol C;
  C.x = px; C.y0 = py0; C.y1 = py1;
  C.lo = (int)mp_max64(piece_offs[inst], 0);
  C.hi = (int)mp_min64(piece_offs[inst + 1], P);
  const int64_t E = 6 * P, H1 = (int64_t)H + 1;
  const int c = px[p], a = py0[p], b = py1[p];
  // top and bottom sides; they link themselves where the boundary goes straight on into the next column
  ekey[6 * p] = (int64_t)c * H1 + a;
  eoth[6 * p] = c + 1;
  ekey[6 * p + 1] = ((int64_t)c + 1) * H1 + b;
  eoth[6 * p + 1] = c;
  {
    const int t = mp_top_at(C, c + 1, a);
    if (t >= 0) mp_link(succ, E, 6 * p, 6 * (int64_t)t);
    const int u = mp_bot_at(C, c - 1, b);
    if (u >= 0) mp_link(succ, E, 6 * p + 1, 6 * (int64_t)u + 1);
  }
  const bool own_more = p + 1 < C.hi && px[p + 1] == c;
  for (int side = 0; side < 2; ++side) {
    const int X = c + side, nb = side ? c + 1 : c - 1;
    for (int end = 0; end < 2; ++end) {
      const int64_t e = 6 * p + 2 + 2 * side + end;
      ekey[e] = MP_NOKEY;
      eoth[e] = 0;
      const int ya = end ? b : a;
      const bool own_fg = end == 0;
      const int own_next = end ? (own_more ? py0[p + 1] : MP_INF) : b;
      bool nb_fg, nb_change;
      int nb_next;
      mp_col_state(C, nb, ya, &nb_fg, &nb_next, &nb_change);
      if ((side == 0 && nb_change) || own_fg == nb_fg) continue;       // the left column owns a shared start; no boundary
      const int yb = min(own_next, nb_next);
      if (yb == MP_INF || yb <= ya) continue;
      const bool down = side ? own_fg : nb_fg;                          // the set column is on the left of the line
      int64_t nxt, prv;
      if (down) {
        ekey[e] = (int64_t)X * H1 + ya;
        eoth[e] = yb;
        // after it: the top side of the pixel right below its end, else the bottom side of the pixel it ran along;
        // before it: the bottom side of the pixel right above its start, else the top side of the pixel it runs along
        nxt = mp_pick(mp_top_at(C, X, yb), 0, mp_bot_at(C, X - 1, yb), 1);
        prv = mp_pick(mp_bot_at(C, X, ya), 1, mp_top_at(C, X - 1, ya), 0);
      } else {
        ekey[e] = (int64_t)X * H1 + yb;
        eoth[e] = ya;
        // after it: the bottom side of the pixel left above its end, else the top side of the pixel it ran along;
        // before it: the top side of the pixel left below its start, else the bottom side of the pixel it runs along
        nxt = mp_pick(mp_bot_at(C, X - 1, ya), 1, mp_top_at(C, X, ya), 0);
        prv = mp_pick(mp_top_at(C, X - 1, yb), 0, mp_bot_at(C, X, yb), 1);
      }
      mp_link(succ, E, e, nxt);
      mp_link(succ, E, prv, e);
    }
  }
}

// ------------------------------------------------------------------------------------------------------- ranking
__global__ __launch_bounds__(MP_THREADS) void mp_min_round_kernel(int64_t E, const int64_t* __restrict__ m_in,
                                                                  const int32_t* __restrict__ j_in,
                                                                  int64_t* __restrict__ m_out, int32_t* __restrict__ j_out) {
  const int64_t e = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
  if (e >= E) return;
  const int j = j_in[e];
  int64_t m = m_in[e];
  int jj = j;
  if (j >= 0 && j < E) {
    m = mp_min64(m, m_in[j]);
    jj = j_in[j];
  }
  m_out[e] = m;
  j_out[e] = jj;
}

// flags: bit 0 = the edge starts its ring, bit 1 = its start vertex is a corner.  The predecessor list is cut in front of
// the ring's first edge, whose predecessor -- the ring's last edge -- goes to lastof.
__global__ __launch_bounds__(MP_THREADS) void mp_prep_kernel(int64_t E, int H, const int64_t* __restrict__ ekey,
                                                             const int32_t* __restrict__ eoth,
                                                             const int32_t* __restrict__ succ, const int64_t* __restrict__ m,
                                                             uint8_t* __restrict__ flags, int32_t* __restrict__ lastof,
                                                             int32_t* __restrict__ prv, int32_t* __restrict__ cw,
                                                             int64_t* __restrict__ a2) {
  const int64_t e = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
  if (e >= E) return;
  const int64_t key = ekey[e];
  if (key == MP_NOKEY) return;                                          // flags / prv / cw / a2 of an empty slot stay as cleared
  const int64_t H1 = (int64_t)H + 1;
  const int64_t sx = key / H1, sy = key - sx * H1, o = eoth[e];
  const bool vert = e % 6 >= 2;
  a2[e] = vert ? sx * (o - sy) : sy * (sx - o);
  const int t = succ[e];
  if (t < 0 || t >= E || ekey[t] == MP_NOKEY) return;
  const bool t_first = ekey[t] == m[t];
  const bool corner = vert != (t % 6 >= 2);
  flags[t] = (uint8_t)((t_first ? 1 : 0) | (corner ? 2 : 0));
  cw[t] = corner ? 1 : 0;
  if (t_first) lastof[t] = (int32_t)e; else prv[t] = (int32_t)e;
}

__global__ __launch_bounds__(MP_THREADS) void mp_rank_round_kernel(int64_t E, const int32_t* __restrict__ p_in,
                                                                   const int32_t* __restrict__ cw_in,
                                                                   const int64_t* __restrict__ a2_in,
                                                                   int32_t* __restrict__ p_out, int32_t* __restrict__ cw_out,
                                                                   int64_t* __restrict__ a2_out) {
  const int64_t e = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
  if (e >= E) return;
  const int p = p_in[e];
  int cw = cw_in[e], pp = p;
  int64_t a2 = a2_in[e];
  if (p >= 0 && p < E) {
    cw += cw_in[p];
    a2 += a2_in[p];
    pp = p_in[p];
  }
  p_out[e] = pp;
  cw_out[e] = cw;
  a2_out[e] = a2;
}

// ------------------------------------------------------------------------------------------------------- output
// first ring whose key is >= key, in [0, R]
__device__ __forceinline__ int64_t mp_ring_of(const int64_t* ring_keys, int64_t R, int64_t key) {
  int64_t lo = 0, hi = R;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ring_keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One lane per edge: a corner goes to slot ring_offs[ring] + (corners of the ring up to it) - 1.
__global__ __launch_bounds__(MP_THREADS) void mp_verts_kernel(int64_t E, int H, const int64_t* __restrict__ ekey,
                                                              const int64_t* __restrict__ m, const uint8_t* __restrict__ flags,
                                                              const int32_t* __restrict__ cw, const int32_t* __restrict__ pinst,
                                                              const int64_t* __restrict__ ring_keys,
                                                              const int64_t* __restrict__ ring_offs, int64_t R, int64_t V,
                                                              int32_t* __restrict__ verts) {
  const int64_t e = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
  if (e >= E) return;
  const int64_t key = ekey[e];
  if (key == MP_NOKEY || !(flags[e] & 2)) return;
  const int64_t rk = ((int64_t)pinst[e / 6] << 33) | m[e];
  const int64_t r = mp_ring_of(ring_keys, R, rk);
  if (r >= R || ring_keys[r] != rk) return;
  const int64_t slot = ring_offs[r] + cw[e] - 1;
  if (slot < ring_offs[r] || slot >= ring_offs[r + 1] || slot >= V) return;
  const int64_t H1 = (int64_t)H + 1;
  verts[2 * slot] = (int32_t)(key / H1);
  verts[2 * slot + 1] = (int32_t)(key % H1);
}

// One block per ring.  An outer ring points at itself.  A hole starts at the top of its leftmost side, (x0, y0), with the set
// pixel (x0 - 1, y0) on its left; going left from that pixel along row y0, the first vertical edge crossed is an upward one
// of the same foreground component: it belongs to the component's outer ring or to another of its holes, whose first vertex
// lies further left.  near[r] = that ring; following near to an outer ring (mp_jump_kernel) gives the parent.
__global__ __launch_bounds__(MP_THREADS) void mp_near_kernel(int64_t R, int64_t P, int k, int H,
                                                             const int64_t* __restrict__ ring_keys,
                                                             const int64_t* __restrict__ ring_area2,
                                                             const int32_t* __restrict__ px, const int32_t* __restrict__ py0,
                                                             const int32_t* __restrict__ py1,
                                                             const int64_t* __restrict__ piece_offs,
                                                             const int64_t* __restrict__ ekey, const int32_t* __restrict__ eoth,
                                                             const int64_t* __restrict__ m, int32_t* __restrict__ near) {
  __shared__ int64_t best[MP_THREADS];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t H1 = (int64_t)H + 1;
  const int64_t rk = ring_keys[r];
  const int inst = (int)(rk >> 33);
  if (ring_area2[r] >= 0 || inst < 0 || inst >= k) {                    // uniform over the block
    if (tid == 0) near[r] = (int32_t)r;
    return;
  }
  const int64_t vk = rk & ((1LL << 33) - 1);
  const int x0 = (int)(vk / H1), y0 = (int)(vk % H1);
  MpCol C;
  C.x = px; C.y0 = py0; C.y1 = py1;
  C.lo = (int)mp_max64(piece_offs[inst], 0);
  C.hi = (int)mp_min64(piece_offs[inst + 1], P);
  const int hi = mp_find_le(C, x0 - 1, MP_INF) + 1;                     // pieces of the columns left of x0; their lines are <= x0
  // from the nearest columns leftwards, MP_THREADS pieces at a time (the pieces are sorted by column): the pieces still to
  // come lie in columns <= the chunk's first, their lines at most one further right; a crossing found at or right of that
  // line is the nearest
  int64_t found = -1;
  for (int top = hi; top > C.lo; top -= MP_THREADS) {
    const int q = top - 1 - tid;
    int64_t mine = -1;
    if (q >= C.lo) {
#pragma unroll
      for (int j = 2; j < 6; ++j) {
        const int64_t e = 6 * (int64_t)q + j;
        const int64_t key = ekey[e];
        if (key == MP_NOKEY) continue;
        const int64_t X = key / H1;
        const int sy = (int)(key - X * H1), ey = eoth[e];
        if (X < x0 && ey <= y0 && y0 < sy) mine = mp_max64(mine, (X << 31) | e);     // upward, across row y0
      }
    }
    best[tid] = mine;
    __syncthreads();
    for (int o = MP_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) best[tid] = mp_max64(best[tid], best[tid + o]);
      __syncthreads();
    }
    found = mp_max64(found, best[0]);
    __syncthreads();
    const int first = top - MP_THREADS > C.lo ? top - MP_THREADS : C.lo;
    if (found >= 0 && (found >> 31) >= (int64_t)px[first] + 1) break;               // uniform over the block
  }
  if (tid == 0) {
    int64_t to = r;
    if (found >= 0) {
      const int64_t e = found & 0x7fffffffLL;
      const int64_t k2 = ((int64_t)inst << 33) | m[e];
      const int64_t r2 = mp_ring_of(ring_keys, R, k2);
      if (r2 < R && ring_keys[r2] == k2) to = r2;
    }
    near[r] = (int32_t)to;
  }
}

__global__ __launch_bounds__(MP_THREADS) void mp_jump_kernel(int64_t R, const int32_t* __restrict__ in, int32_t* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
  if (r >= R) return;
  const int t = in[r];
  out[r] = (t >= 0 && t < R) ? in[t] : t;
}

__global__ __launch_bounds__(MP_THREADS) void mp_parent_kernel(int64_t R, int k, const int32_t* __restrict__ ptr,
                                                               const int64_t* __restrict__ ring_keys,
                                                               const int64_t* __restrict__ ring_area2,
                                                               const int64_t* __restrict__ inst_ring_offs,
                                                               int32_t* __restrict__ parent) {
  const int64_t r = (int64_t)blockIdx.x * MP_THREADS + threadIdx.x;
  if (r >= R) return;
  const int t = ptr[r];
  const int inst = (int)(ring_keys[r] >> 33);
  int par = -1;
  if (ring_area2[r] < 0 && t >= 0 && t < R && ring_area2[t] >= 0 && inst >= 0 && inst < k) par = (int)(t - inst_ring_offs[inst]);
  parent[r] = par;
}

inline unsigned mp_blocks(int64_t n) { return (unsigned)((n + MP_THREADS - 1) / MP_THREADS); }
constexpr int64_t MP_MAX_PIECES = RSP_MASK_POLYGON_MAX_PIECES;

}  // namespace

extern "C" int rsp_mask_polygon_edges(int32_t k, int32_t H, int32_t W, const int64_t* piece_offs, int64_t P, const int32_t* pieces,
                                      int64_t* ekey, int32_t* eoth, int32_t* succ, rsp_stream_t stream) {
  if (!piece_offs || k < 0 || P < 0 || P > MP_MAX_PIECES || !rsp_run_canvas_ok(H, W)) return RSP_EINVAL;
  if (P > 0 && (!pieces || !ekey || !eoth || !succ)) return RSP_EINVAL;
  if (k == 0 || P == 0) return RSP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int32_t *px = pieces, *py0 = pieces + P, *py1 = pieces + 2 * P, *pinst = pieces + 3 * P;
  if (hipMemsetAsync(succ, 0xff, (size_t)(6 * P) * sizeof(int32_t), s) != hipSuccess) return RSP_ELAUNCH;
  hipLaunchKernelGGL(mp_edges_kernel, dim3(mp_blocks(P)), dim3(MP_THREADS), 0, s, px, py0, py1, pinst, piece_offs, k, P, H, ekey,
                     eoth, succ);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int64_t rsp_mask_polygon_rank_workspace_bytes(int64_t P) {
  if (P < 0 || P > MP_MAX_PIECES) return 0;
  const int64_t E = 6 * (P > 0 ? P : 1);
  return E * (int64_t)(2 * sizeof(int64_t) + 3 * sizeof(int32_t));
}

extern "C" int rsp_mask_polygon_rank(int64_t P, int32_t H, int32_t rounds, const int64_t* ekey, const int32_t* eoth,
                                     const int32_t* succ, void* workspace, int64_t* ring_key, uint8_t* flags, int32_t* lastof,
                                     int32_t* corners, int64_t* area2, rsp_stream_t stream) {
  if (P < 0 || P > MP_MAX_PIECES || H <= 0 || rounds < 0 || rounds > 62) return RSP_EINVAL;
  if (P == 0) return RSP_OK;
  if (!ekey || !eoth || !succ || !workspace || !ring_key || !flags || !lastof || !corners || !area2) return RSP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t E = 6 * P;
  const unsigned nb = mp_blocks(E);
  rounds = rounds < 2 ? 2 : rounds + (rounds & 1);       // an even number: the results end in the caller's arrays
  int64_t* m2 = static_cast<int64_t*>(workspace);
  int64_t* a2b = m2 + E;
  int32_t* ja = reinterpret_cast<int32_t*>(a2b + E);
  int32_t* jb = ja + E;
  int32_t* cwb = jb + E;
  // the smallest start vertex of every edge's ring
  const int64_t* m_in = ekey;
  const int32_t* j_in = succ;
  for (int r = 0; r < rounds; r += 2) {
    hipLaunchKernelGGL(mp_min_round_kernel, dim3(nb), dim3(MP_THREADS), 0, s, E, m_in, j_in, m2, jb);
    RSP_CHECK_LAUNCH();
    hipLaunchKernelGGL(mp_min_round_kernel, dim3(nb), dim3(MP_THREADS), 0, s, E, m2, jb, ring_key, ja);
    RSP_CHECK_LAUNCH();
    m_in = ring_key;
    j_in = ja;
  }
  // corners and doubled area in front of every edge, from the ring's first edge on
  if (hipMemsetAsync(flags, 0, (size_t)E, s) != hipSuccess) return RSP_ELAUNCH;
  if (hipMemsetAsync(lastof, 0xff, (size_t)E * sizeof(int32_t), s) != hipSuccess) return RSP_ELAUNCH;
  if (hipMemsetAsync(ja, 0xff, (size_t)E * sizeof(int32_t), s) != hipSuccess) return RSP_ELAUNCH;
  if (hipMemsetAsync(corners, 0, (size_t)E * sizeof(int32_t), s) != hipSuccess) return RSP_ELAUNCH;
  if (hipMemsetAsync(area2, 0, (size_t)E * sizeof(int64_t), s) != hipSuccess) return RSP_ELAUNCH;
  hipLaunchKernelGGL(mp_prep_kernel, dim3(nb), dim3(MP_THREADS), 0, s, E, H, ekey, eoth, succ, ring_key, flags, lastof, ja,
                     corners, area2);
  RSP_CHECK_LAUNCH();
  for (int r = 0; r < rounds; r += 2) {
    hipLaunchKernelGGL(mp_rank_round_kernel, dim3(nb), dim3(MP_THREADS), 0, s, E, ja, corners, area2, jb, cwb, a2b);
    RSP_CHECK_LAUNCH();
    hipLaunchKernelGGL(mp_rank_round_kernel, dim3(nb), dim3(MP_THREADS), 0, s, E, jb, cwb, a2b, ja, corners, area2);
    RSP_CHECK_LAUNCH();
  }
  return RSP_OK;
}

extern "C" int rsp_mask_polygon_write(int64_t P, int32_t k, int32_t H, int64_t R, int64_t V, int32_t rounds,
                                      const int32_t* pieces, const int64_t* piece_offs, const int64_t* ekey, const int32_t* eoth,
                                      const int64_t* ring_key, const uint8_t* flags, const int32_t* corners,
                                      const int64_t* ring_keys, const int64_t* ring_offs, const int64_t* ring_area2,
                                      const int64_t* inst_ring_offs, int32_t* near_ws, int32_t* verts, int32_t* ring_parent,
                                      rsp_stream_t stream) {
  if (P < 0 || P > MP_MAX_PIECES || k < 0 || H <= 0 || R < 0 || R > 0x7fffffffLL || V < 0 || rounds < 0 || rounds > 62)
    return RSP_EINVAL;
  if (R == 0 || P == 0) return RSP_OK;
  if (!pieces || !piece_offs || !ekey || !eoth || !ring_key || !flags || !corners || !ring_keys || !ring_offs || !ring_area2 ||
      !inst_ring_offs || !near_ws || !ring_parent || (V > 0 && !verts))
    return RSP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int64_t E = 6 * P;
  const int32_t *px = pieces, *py0 = pieces + P, *py1 = pieces + 2 * P, *pinst = pieces + 3 * P;
  hipLaunchKernelGGL(mp_verts_kernel, dim3(mp_blocks(E)), dim3(MP_THREADS), 0, s, E, H, ekey, ring_key, flags, corners, pinst,
                     ring_keys, ring_offs, R, V, verts);
  RSP_CHECK_LAUNCH();
  int32_t *na = near_ws, *nb = near_ws + R;
  hipLaunchKernelGGL(mp_near_kernel, dim3((unsigned)R), dim3(MP_THREADS), 0, s, R, P, k, H, ring_keys, ring_area2, px, py0, py1,
                     piece_offs, ekey, eoth, ring_key, na);
  RSP_CHECK_LAUNCH();
  rounds += rounds & 1;
  for (int r = 0; r < rounds; r += 2) {
    hipLaunchKernelGGL(mp_jump_kernel, dim3(mp_blocks(R)), dim3(MP_THREADS), 0, s, R, na, nb);
    RSP_CHECK_LAUNCH();
    hipLaunchKernelGGL(mp_jump_kernel, dim3(mp_blocks(R)), dim3(MP_THREADS), 0, s, R, nb, na);
    RSP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mp_parent_kernel, dim3(mp_blocks(R)), dim3(MP_THREADS), 0, s, R, k, na, ring_keys, ring_area2,
                     inst_ring_offs, ring_parent);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
