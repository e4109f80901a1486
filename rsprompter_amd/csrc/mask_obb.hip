// Oriented boxes: the convex hull and the minimum-area rectangle of every mask of a run table, exact in
// integers, on the device.  Pixel (x, y) covers [x, x + 1] x [y, y + 1], y down; an instance is the union of the closed squares
// of ALL its set pixels (components are not separated).
//
// THE CONTRACT (tests/_mask_obb_ref.py states it sequentially).  The hull is strictly convex, starts at its smallest vertex
// by (x, y) and runs clockwise on screen (area2 = sum x_i y_{i+1} - x_{i+1} y_i > 0); a non-empty instance has at least 4
// vertices.  Hull edge j runs from vertex j to j + 1 (cyclic): e = (ex, ey), nrm = (-ey, ex) points inside, L = |e|^2; over
// the hull vertices p, a = p . e and b = p . nrm, U = amax - amin, V = bmax - bmin (bmin is the edge's own b).  The rectangle
// flush with edge j has area U V / L; the chosen edge minimises it, U_j V_j L_i < U_i V_i L_j compared in unsigned 128-bit
// integers (coordinates up to 65 535: U V L < 2^101), the lowest j among equals.  q = (ex, ey, amin, amax, bmin, bmax).
//
// COLUMN EXTREMES.  A hull depends only on the first and the last set pixel of every column, and the COCO stream is column-major:
// a ones-run is the FIRST piece of its column xa iff the ones-run before it ends in an earlier column, and the LAST piece of xb
// iff the next one starts in a later column; a run across column ends also holds row 0 of the columns it enters and row H of the
// columns it leaves.  So every ones-run yields at most three records (x, top) of the upper stream and three (x, bottom) of the
// lower one, each stream ascending in x (of the full columns inside one long run only the first and the last are kept: the ones
// between them are collinear).  Work is proportional to the runs; there is no dense [k, W] array and no sort.
//
// THE HULL OF ONE CHAIN.  mo_chain_kernel runs one block per (instance, chain).  It walks the row (run_table.h), writes the
// chain's records to its slot of the workspace, then turns them into the chain's points: column x gives (x, y) and (x + 1, y),
// and where two columns meet only the outer of the two points at that abscissa stays, so x ascends STRICTLY.  Pruning rounds
// follow: a round removes every interior point that is not a strict convex turn between its two neighbours of the round, all at
// once (a removed point lies on or inside the segment between two points of the set with abscissae around its own, so it is no
// hull vertex and the hull does not change), and compacts with block scans.  The first round that removes nothing leaves the
// chain's hull.  Chains of up to MO_LDS_PTS candidate points ping-pong between two LDS buffers, longer ones between the two
// halves of the instance's workspace slot.  Rounds: a few for ordinary masks; a concave arc next to one far outlier loses one
// point a round (correct, slow: DESIGN §14.9).
//
// mo_write_kernel (one block per instance) joins the chains -- upper left to right, lower right to left -- and sums area2;
// mo_rect_kernel (one block per hull) is the rotating calipers in the quadratic form: one lane per edge, extents over all
// vertices, block reduction of (U V, L, j).  A lattice hull on a canvas of side N has O(N^(2/3)) vertices.  No atomics anywhere:
// a second launch is bit-identical.
#include "rsp_common.h"
#include "run_table.h"

namespace {

typedef unsigned __int128 mo_u128;

constexpr int MO_THREADS = 256;
constexpr int MO_LDS_PTS = 4096;             // candidate points of a chain that stay in LDS (two buffers of packed points)
constexpr int MO_RECT_LDS = 1024;            // hull vertices of mo_rect_kernel that are staged in LDS (mask hulls: a few hundred)
constexpr int32_t MO_MAX_SIDE = RSP_MASK_OBB_MAX_SIDE;       // x and y of a point fit 16 bits each; every product of the calipers fits 128
constexpr int MO_NONE = 0x7fffffff;

// a point / a record: x << 16 | y
__device__ __forceinline__ uint32_t mo_pack(int x, int y) { return ((uint32_t)x << 16) | (uint32_t)y; }
__device__ __forceinline__ int mo_x(uint32_t p) { return (int)(p >> 16); }
__device__ __forceinline__ int mo_y(uint32_t p) { return (int)(p & 0xffffu); }

// The workspace: for chain c (0 upper, 1 lower) and buffer b (0 / 1) a region of 2 B words, B = bound_offs[k]; instance m owns
// words 2 bound_offs[m] .. 2 bound_offs[m + 1] of each.  bound_offs[m + 1] - bound_offs[m] >= 3 * (runs of row m / 2), the
// most records a chain of the row can have; a chain has at most two points a record.
__device__ __forceinline__ uint32_t* mo_slot(uint32_t* ws, int64_t B, int chain, int buf, int64_t off) {
  return ws + (int64_t)(chain * 2 + buf) * 2 * B + 2 * off;
}
// the slot of row m, checked against the row and the workspace: *slot_off = its offset, returns the records it can hold (0: none)
__device__ __forceinline__ int64_t mo_slot_of(const int64_t* __restrict__ bound_offs, int64_t B, int m, int n, int64_t* slot_off) {
  const int64_t o0 = bound_offs[m], o1 = bound_offs[m + 1];
  *slot_off = o0;
  const int64_t need = 3 * (int64_t)(n > 0 ? n / 2 : 0);
  return (o0 >= 0 && o1 >= o0 && o1 <= B && o1 - o0 >= need) ? o1 - o0 : 0;
}

// ------------------------------------------------------------------------------------------------ one chain of one instance
__global__ __launch_bounds__(MO_THREADS) void mo_chain_kernel(const uint32_t* __restrict__ counts, const int32_t* __restrict__ n_in,
                                                              int cap, int H, int W, const int64_t* __restrict__ bound_offs,
                                                              int64_t B, uint32_t* ws, int k, int32_t* __restrict__ chain_cnt,
                                                              int32_t* __restrict__ rounds) {
  __shared__ uint32_t lds0[MO_LDS_PTS], lds1[MO_LDS_PTS];
  __shared__ int tmp[MO_THREADS / 64];
  const int m = blockIdx.x, chain = blockIdx.y, tid = threadIdx.x;
  const bool lower = chain != 0;
  const RspRunRow row = rsp_run_row(counts, n_in, cap, m);
  int64_t off;
  const int64_t room = mo_slot_of(bound_offs, B, m, row.n, &off);
  if (row.n <= 1 || room == 0) {                                            // uniform over the block; a row of one run is empty
    if (tid == 0) { chain_cnt[chain * k + m] = 0; rounds[chain * k + m] = 0; }
    return;
  }
  uint32_t* const gA = mo_slot(ws, B, chain, 0, off);
  uint32_t* const gB = mo_slot(ws, B, chain, 1, off);
  const int64_t HW = (int64_t)H * W;

  // 1. the records of the chain, in stream order, into gB (free until the first round writes there)
  int nrec = 0;
  for (RspRunWalk<MO_THREADS> r(row, tmp); r.next();) {
    // clamped indices and masked values up to the scan (run_table.h): the zero runs around a ones-run
    const int ones = r.c & -(int)(r.i & 1);
    const int ip = min(max(r.i - 1, 0), row.n - 1), in = min(r.i + 1, row.n - 1);
    const int64_t zp = (int64_t)row.c[ip], zn = (int64_t)row.c[in];
    const bool ok = ones > 0 && (int64_t)r.s + ones <= HW;
    const RspRunCols c = rsp_run_cols(r.s, ones, H);                        // not used where ones == 0
    const int64_t prev_end = (int64_t)r.s - zp - 1, next_start = (int64_t)r.s + ones + zn;
    const bool first = r.i < 3 || prev_end < 0 || prev_end / H < c.xa;
    const bool last = r.i + 2 >= row.n || next_start / H > c.xb;
    const int wide = (int)(c.xb > c.xa), wider = (int)(c.xb > c.xa + 1);
    const int ends = lower ? (int)last : (int)first;
    const int cnt = (ends + wide + wider) & -(int)ok;
    int chunk;
    int pos = nrec + rsp_block_excl_scan<MO_THREADS>(cnt, tmp, &chunk);
    if (cnt > 0 && (int64_t)pos + cnt <= room) {
      if (!lower) {
        if (first) gB[pos++] = mo_pack(c.xa, c.ra);
        if (wide) gB[pos++] = mo_pack(c.xa + 1, 0);
        if (wider) gB[pos++] = mo_pack(c.xb, 0);
      } else {
        if (wide) gB[pos++] = mo_pack(c.xa, H);
        if (wider) gB[pos++] = mo_pack(c.xb - 1, H);
        if (last) gB[pos++] = mo_pack(c.xb, c.rb + 1);
      }
    }
    nrec += chunk;
  }
  if ((int64_t)nrec > room) nrec = 0;                                       // (cannot happen: room holds three records a ones-run)
  if (nrec == 0) {
    if (tid == 0) { chain_cnt[chain * k + m] = 0; rounds[chain * k + m] = 0; }
    return;
  }
  __syncthreads();                                                          // the records are the block's to read

  // 2. the points: of the two at one abscissa where columns x - 1 and x meet, the outer one (the left column's among equals)
  const bool staged = 2 * nrec <= MO_LDS_PTS;
  uint32_t* cur = staged ? lds0 : gA;
  uint32_t* nxt = staged ? lds1 : gB;
  int npts = 0;
  for (int base = 0; base < nrec; base += MO_THREADS) {
    const int i = base + tid, ic = min(i, nrec - 1);
    const uint32_t rec = gB[ic], rp = gB[max(ic - 1, 0)], rn = gB[min(ic + 1, nrec - 1)];
    const int x = mo_x(rec), y = mo_y(rec);
    const int ys = lower ? -y : y, yp = lower ? -mo_y(rp) : mo_y(rp), yn = lower ? -mo_y(rn) : mo_y(rn);
    const int valid = (int)(i < nrec);
    const int el = (int)(ic == 0 || mo_x(rp) != x - 1 || ys < yp) & valid;
    const int er = (int)(ic == nrec - 1 || mo_x(rn) != x + 1 || ys <= yn) & valid;
    int chunk;
    const int pos = npts + rsp_block_excl_scan<MO_THREADS>(el + er, tmp, &chunk);
    // (gA when not staged: the records in gB are read by other threads of this loop, gA is written only)
    if (el) cur[pos] = mo_pack(x, y);
    if (er) cur[pos + el] = mo_pack(x + 1, y);
    npts += chunk;
  }
  __syncthreads();

  // 3. pruning rounds up to the fixed point
  int nr = 0;
  for (;;) {
    int out = 0;
    for (int base = 0; base < npts; base += MO_THREADS) {
      const int i = base + tid, ic = min(i, npts - 1);
      const uint32_t p = cur[ic], a = cur[max(ic - 1, 0)], b = cur[min(ic + 1, npts - 1)];
      const int64_t cr = (int64_t)(mo_x(p) - mo_x(a)) * (mo_y(b) - mo_y(a)) - (int64_t)(mo_y(p) - mo_y(a)) * (mo_x(b) - mo_x(a));
      const bool convex = lower ? cr < 0 : cr > 0;
      const int keep = (int)(ic == 0 || ic == npts - 1 || convex) & (int)(i < npts);
      int chunk;
      const int pos = out + rsp_block_excl_scan<MO_THREADS>(keep, tmp, &chunk);
      if (keep) nxt[pos] = p;
      out += chunk;
    }
    __syncthreads();
    uint32_t* const t = cur;
    cur = nxt;
    nxt = t;
    if (out == npts) break;                                                 // uniform
    npts = out;
    ++nr;
  }
  // 4. the chain's hull into the first buffer of the slot
  if (cur != gA)
    for (int i = tid; i < npts; i += MO_THREADS) gA[i] = cur[i];
  if (tid == 0) { chain_cnt[chain * k + m] = npts; rounds[chain * k + m] = nr; }
}

// ------------------------------------------------------------------------------------------------ the ring of one instance
template <int T>
__device__ __forceinline__ int64_t mo_block_sum64(int64_t v, int64_t* tmp) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t sum = 0;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) sum += tmp[w];
  __syncthreads();
  return sum;
}

__global__ __launch_bounds__(MO_THREADS) void mo_write_kernel(const int32_t* __restrict__ n_in, int cap, int k,
                                                              const int64_t* __restrict__ bound_offs, int64_t B,
                                                              const uint32_t* __restrict__ ws, const int32_t* __restrict__ chain_cnt,
                                                              const int64_t* __restrict__ hull_offs, int64_t Vh,
                                                              int32_t* __restrict__ verts, int64_t* __restrict__ area2) {
  __shared__ int64_t tmp[MO_THREADS / 64];
  const int m = blockIdx.x, tid = threadIdx.x;
  int64_t off;
  const int64_t room = mo_slot_of(bound_offs, B, m, min(n_in[m], cap), &off);
  const int cu = chain_cnt[m], cl = chain_cnt[k + m];
  const int64_t o0 = rsp_clamp64(hull_offs[m], 0, Vh), o1 = rsp_clamp64(hull_offs[m + 1], o0, Vh);
  const bool ok = room > 0 && cu >= 2 && cl >= 2 && cu <= 2 * room && cl <= 2 * room && o1 - o0 == (int64_t)cu + cl;
  int64_t a2 = 0;
  if (ok) {                                                                 // uniform over the block
    const uint32_t* up = mo_slot(const_cast<uint32_t*>(ws), B, 0, 0, off);
    const uint32_t* lo = mo_slot(const_cast<uint32_t*>(ws), B, 1, 0, off);
    const int mm = cu + cl;
    for (int j = tid; j < mm; j += MO_THREADS) {
      const int jn = j + 1 == mm ? 0 : j + 1;
      const uint32_t p = j < cu ? up[j] : lo[cl - 1 - (j - cu)], q = jn < cu ? up[jn] : lo[cl - 1 - (jn - cu)];
      verts[2 * (o0 + j)] = mo_x(p);
      verts[2 * (o0 + j) + 1] = mo_y(p);
      a2 += (int64_t)mo_x(p) * mo_y(q) - (int64_t)mo_x(q) * mo_y(p);
    }
  }
  a2 = mo_block_sum64<MO_THREADS>(a2, tmp);
  if (tid == 0) area2[m] = a2;
}

// ----------------------------------------------------------------------------------------- the minimum-area rectangle
// an edge's rectangle: P = U V (up to 2^68) and L; j = MO_NONE: no edge
struct MoBest {
  uint64_t phi, plo, L;
  int j;
};
__device__ __forceinline__ bool mo_beats(const MoBest a, const MoBest b) {   // a is the smaller rectangle, or the same at a lower edge
  if (a.j == MO_NONE) return false;
  if (b.j == MO_NONE) return true;
  const mo_u128 l = ((((mo_u128)a.phi) << 64) | a.plo) * b.L, r = ((((mo_u128)b.phi) << 64) | b.plo) * a.L;
  return l < r || (l == r && a.j < b.j);
}
// (field by field: a select between two structs would put them in scratch)
__device__ __forceinline__ MoBest mo_min(const MoBest a, const MoBest b) {
  const bool second = mo_beats(b, a);
  MoBest r;
  r.phi = second ? b.phi : a.phi;
  r.plo = second ? b.plo : a.plo;
  r.L = second ? b.L : a.L;
  r.j = second ? b.j : a.j;
  return r;
}

__global__ __launch_bounds__(MO_THREADS) void mo_rect_kernel(const int32_t* __restrict__ verts, const int64_t* __restrict__ offs,
                                                             int64_t Vh, int32_t* __restrict__ edge, int64_t* __restrict__ q) {
  constexpr int NW = MO_THREADS / 64;
  __shared__ int sx[MO_RECT_LDS], sy[MO_RECT_LDS];
  __shared__ uint64_t w_phi[NW], w_plo[NW], w_L[NW];
  __shared__ int w_j[NW];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s = rsp_clamp64(offs[r], 0, Vh), e = rsp_clamp64(offs[r + 1], s, Vh);
  const int64_t m64 = e - s;
  if (m64 < 1 || m64 > 0x7fffffffLL) {                                      // uniform over the block
    if (tid == 0) {
      edge[r] = -1;
      for (int i = 0; i < 6; ++i) q[6 * (int64_t)r + i] = 0;
    }
    return;
  }
  const int m = (int)m64;
  const int32_t* gv = verts + 2 * s;
  const bool staged = m <= MO_RECT_LDS;
  if (staged) {
    for (int j = tid; j < m; j += MO_THREADS) { sx[j] = gv[2 * j]; sy[j] = gv[2 * j + 1]; }
    __syncthreads();
  }
  auto X = [&](int j) { return staged ? sx[j] : gv[2 * j]; };
  auto Y = [&](int j) { return staged ? sy[j] : gv[2 * j + 1]; };
  MoBest best{0, 0, 0, MO_NONE};
  int64_t bex = 0, bey = 0, bamin = 0, bamax = 0, bbmin = 0, bbmax = 0;
  for (int j = tid; j < m; j += MO_THREADS) {
    const int jn = j + 1 == m ? 0 : j + 1;
    const int64_t px = X(j), py = Y(j), ex = (int64_t)X(jn) - px, ey = (int64_t)Y(jn) - py;
    int64_t amin = px * ex + py * ey, amax = amin;
    const int64_t bmin = py * ex - px * ey;
    int64_t bmax = bmin;
    for (int i = 0; i < m; ++i) {
      const int64_t vx = X(i), vy = Y(i), a = vx * ex + vy * ey, b = vy * ex - vx * ey;
      amin = a < amin ? a : amin;
      amax = a > amax ? a : amax;
      bmax = b > bmax ? b : bmax;
    }
    const mo_u128 P = (mo_u128)(uint64_t)(amax - amin) * (uint64_t)(bmax - bmin);
    const MoBest cand{(uint64_t)(P >> 64), (uint64_t)P, (uint64_t)(ex * ex + ey * ey), j};
    // Field by field, as in mo_min: every member of the thread's best is a select on the one comparison.  Written as
    // `if (mo_beats(cand, best)) { best = cand; ... }` hipcc 7.2.0 emitted gfx950 code in which a thread's second and later
    // winning edges kept the OLD best.plo (the register holding cand.plo is reused inside the comparison and restored from
    // best.plo for every lane): polygons of more than MO_THREADS edges then chose a wrong edge, on the device only.
    // tests/_mask_obb_cases.py check_hull_min_rect holds such polygons.
    const bool take = mo_beats(cand, best);
    best.phi = take ? cand.phi : best.phi;
    best.plo = take ? cand.plo : best.plo;
    best.L = take ? cand.L : best.L;
    best.j = take ? cand.j : best.j;
    bex = take ? ex : bex;
    bey = take ? ey : bey;
    bamin = take ? amin : bamin;
    bamax = take ? amax : bamax;
    bbmin = take ? bmin : bbmin;
    bbmax = take ? bmax : bbmax;
  }
  MoBest red = best;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MoBest t;
    t.phi = __shfl_xor(red.phi, o, 64);
    t.plo = __shfl_xor(red.plo, o, 64);
    t.L = __shfl_xor(red.L, o, 64);
    t.j = __shfl_xor(red.j, o, 64);
    red = mo_min(red, t);
  }
  if (lane == 0) { w_phi[wave] = red.phi; w_plo[wave] = red.plo; w_L[wave] = red.L; w_j[wave] = red.j; }
  __syncthreads();
  MoBest win{w_phi[0], w_plo[0], w_L[0], w_j[0]};
#pragma unroll
  for (int w = 1; w < NW; ++w) win = mo_min(win, MoBest{w_phi[w], w_plo[w], w_L[w], w_j[w]});
  if (win.j != MO_NONE && win.j == best.j) {                                // the one thread whose best edge won
    edge[r] = win.j;
    int64_t* o = q + 6 * (int64_t)r;
    o[0] = bex; o[1] = bey; o[2] = bamin; o[3] = bamax; o[4] = bbmin; o[5] = bbmax;
  }
}

}  // namespace

extern "C" int64_t rsp_mask_hull_workspace_bytes(int64_t B) {
  if (B < 0 || B > RSP_MASK_OBB_MAX_BOUND) return 0;
  return 8 * B * (int64_t)sizeof(uint32_t);
}

extern "C" int rsp_mask_hull_chains(const uint32_t* counts, const int32_t* n, int32_t k, int32_t cap, int32_t H, int32_t W,
                                    const int64_t* bound_offs, int64_t B, void* workspace, int32_t* chain_cnt, int32_t* rounds,
                                    rsp_stream_t stream) {
  if (k < 0 || cap < 1 || !rsp_run_canvas_ok(H, W) || H > MO_MAX_SIDE || W > MO_MAX_SIDE || B < 0 || B > RSP_MASK_OBB_MAX_BOUND)
    return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  if (!counts || !n || !bound_offs || !chain_cnt || !rounds || (B > 0 && !workspace)) return RSP_EINVAL;
  hipLaunchKernelGGL(mo_chain_kernel, dim3((unsigned)k, 2), dim3(MO_THREADS), 0, (hipStream_t)stream, counts, n, (int)cap, (int)H,
                     (int)W, bound_offs, B, (uint32_t*)workspace, (int)k, chain_cnt, rounds);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_mask_hull_write(const int32_t* n, int32_t k, int32_t cap, const int64_t* bound_offs, int64_t B,
                                   const void* workspace, const int32_t* chain_cnt, const int64_t* hull_offs, int64_t Vh,
                                   int32_t* hull_verts, int64_t* hull_area2, rsp_stream_t stream) {
  if (k < 0 || cap < 1 || B < 0 || B > RSP_MASK_OBB_MAX_BOUND || Vh < 0 || Vh > 0x7fffffffLL) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  if (!n || !bound_offs || !chain_cnt || !hull_offs || !hull_area2 || (B > 0 && !workspace) || (Vh > 0 && !hull_verts))
    return RSP_EINVAL;
  hipLaunchKernelGGL(mo_write_kernel, dim3((unsigned)k), dim3(MO_THREADS), 0, (hipStream_t)stream, n, (int)cap, (int)k, bound_offs,
                     B, (const uint32_t*)workspace, chain_cnt, hull_offs, Vh, hull_verts, hull_area2);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_hull_min_rect(const int32_t* hull_verts, const int64_t* hull_offs, int32_t k, int64_t Vh, int32_t* edge,
                                 int64_t* q, rsp_stream_t stream) {
  if (k < 0 || Vh < 0 || Vh > 0x7fffffffLL) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  if (!hull_offs || !edge || !q || (Vh > 0 && !hull_verts)) return RSP_EINVAL;
  hipLaunchKernelGGL(mo_rect_kernel, dim3((unsigned)k), dim3(MO_THREADS), 0, (hipStream_t)stream, hull_verts, hull_offs, Vh, edge,
                     q);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
