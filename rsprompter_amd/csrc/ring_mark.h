// The round machinery of Douglas-Peucker on closed rings, shared by polygon simplification (csrc/ring_simplify.hip, DESIGN
// §14.8) and shared-border simplification (csrc/ring_coverage.hip): the 128-bit distance, the wave kernel
// (rings up to 64 vertices) and the block kernel (longer rings), described in ring_simplify.hip.  Both kernels are templates on
// COV, which chooses between the two contracts at compile time:
//   COV = false  §14.8: index 0 is the one vertex kept at first, the first round splits without the tolerance test (the
//                anchor), ties go to the lowest index.
//   COV = true   §14.15: `keep` is read as well as written -- a vertex whose byte is not 0 is kept from the start (the nodes),
//                with index 0; a chain whose two ends are the same point splits without the tolerance test, in every round;
//                among equal numerators the vertex with the smallest (x, y) wins (the lowest index among equal points).
//                Both rules are symmetric under reversal of a chain, which is what makes the two sides of a border agree.
// Include it after rsp_common.h (it does not include it itself: the emulated build rewrites that include per source file).
#pragma once

namespace {

typedef unsigned __int128 rs_u128;

constexpr int RS_WAVE_THREADS = 256;          // rs_mark_wave_kernel: four rings a block
constexpr int RS_WAVE_MAX = 64;               // the longest ring of the wave path
constexpr int RS_LDS_VERTS = 2048;            // rs_mark_block_kernel: coordinates of rings up to here are staged in LDS
constexpr int RS_MAX_BLOCKS = 4096;           // rs_mark_block_kernel strides over the rings
constexpr int RS_NONE = 0x7fffffff;
constexpr int64_t RS_MAX_TOL2_Q8 = RSP_RING_SIMPLIFY_MAX_TOL2_Q8;
constexpr int32_t RS_MAX_SIDE = RSP_RING_SIMPLIFY_MAX_SIDE;

// the numerator of the squared distance from p to the segment a b; *den = its denominator
__device__ __forceinline__ rs_u128 rs_num(int ax, int ay, int bx, int by, int px, int py, uint64_t* den) {
  const int64_t dx = (int64_t)bx - ax, dy = (int64_t)by - ay, ex = (int64_t)px - ax, ey = (int64_t)py - ay;
  const uint64_t L = (uint64_t)(dx * dx + dy * dy), da = (uint64_t)(ex * ex + ey * ey);
  *den = L ? L : 1;
  if (L == 0) return (rs_u128)da;
  const int64_t t = ex * dx + ey * dy;
  if (t <= 0) return (rs_u128)da * L;
  if ((uint64_t)t >= L) {
    const int64_t fx = (int64_t)px - bx, fy = (int64_t)py - by;
    return (rs_u128)(uint64_t)(fx * fx + fy * fy) * L;
  }
  const int64_t c = ex * dy - ey * dx;
  const uint64_t ac = (uint64_t)(c < 0 ? -c : c);
  return (rs_u128)ac * ac;
}
__device__ __forceinline__ bool rs_over(uint64_t hi, uint64_t lo, uint64_t den, int64_t tol2_q8) {
  const rs_u128 num = ((rs_u128)hi << 64) | lo;
  return (num << 8) > (rs_u128)(uint64_t)tol2_q8 * den;
}
__device__ __forceinline__ int64_t rs_clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the best vertex of (part of) a chain: the largest num, among equals the first by `less` (the lowest index, or the smallest
// point); idx = RS_NONE: no vertex
struct RsBest {
  uint64_t hi, lo;
  int idx;
};
template <typename Less>
__device__ __forceinline__ bool rs_beats(uint64_t hi, uint64_t lo, int idx, const RsBest o, Less less) {
  return hi > o.hi || (hi == o.hi && (lo > o.lo || (lo == o.lo && less(idx, o.idx))));
}
// (field by field: a select between two structs would put them in scratch)
__device__ __forceinline__ RsBest rs_pick(bool second, const RsBest a, const RsBest b) {
  RsBest r;
  r.hi = second ? b.hi : a.hi;
  r.lo = second ? b.lo : a.lo;
  r.idx = second ? b.idx : a.idx;
  return r;
}
template <typename Less>
__device__ __forceinline__ RsBest rs_max(const RsBest a, const RsBest b, Less less) {
  return rs_pick(rs_beats(b.hi, b.lo, b.idx, a, less), a, b);
}

// ------------------------------------------------------------------------------------------------ one wave per ring
template <bool COV>
__global__ __launch_bounds__(RS_WAVE_THREADS) void rs_mark_wave_kernel(const int32_t* __restrict__ verts,
                                                                       const int64_t* __restrict__ ring_offs, int64_t R,
                                                                       int64_t V, int64_t tol2_q8, uint8_t* __restrict__ keep,
                                                                       int32_t* __restrict__ pos, int32_t* __restrict__ cnt,
                                                                       int64_t* __restrict__ area2, int32_t* __restrict__ rounds) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (RS_WAVE_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= R) return;                                                   // uniform over the wave, like every exit below
  const int64_t s = rs_clamp64(ring_offs[r], 0, V), e = rs_clamp64(ring_offs[r + 1], s, V);
  if (e - s > RS_WAVE_MAX) return;                                      // the block path's
  const int m = (int)(e - s);
  if (m == 0) {
    if (lane == 0) { cnt[r] = 0; area2[r] = 0; rounds[r] = 0; }
    return;
  }
  // no branch on a lane's validity in front of the shuffles: a clamped index and masked values
  const bool valid = lane < m;
  const int64_t vi = s + (valid ? lane : m - 1);
  const int x = verts[2 * vi], y = verts[2 * vi + 1];
  const uint64_t below_me = (1ull << lane) - 1, above_me = lane == 63 ? 0ull : ~((2ull << lane) - 1);
  bool kept = lane == 0;
  if constexpr (COV) kept = kept || (valid && keep[vi] != 0);
  const uint64_t xy = ((uint64_t)(uint32_t)x << 32) | (uint32_t)y;     // (COV) the order of the points
  int nr = 0;
  for (;;) {
    const uint64_t K = __ballot(kept);
    const uint64_t lo_k = K & below_me, hi_k = K & above_me;
    const int a = lo_k ? 63 - __builtin_clzll(lo_k) : 0;
    const int b = hi_k ? __builtin_ctzll(hi_k) : m;                     // m: back at v_0
    const int bl = b == m ? 0 : b;
    const int ax = __shfl(x, a, 64), ay = __shfl(y, a, 64), bx = __shfl(x, bl, 64), by = __shfl(y, bl, 64);
    uint64_t den;
    const rs_u128 num = rs_num(ax, ay, bx, by, x, y, &den);
    const bool cand = valid && !kept;
    const uint64_t hi = cand ? (uint64_t)(num >> 64) : 0ull, lo = cand ? (uint64_t)num : 0ull;
    // the largest num of the lanes a + 1 .. lane, then of the whole chain from its last lane b - 1
    // (COV: among equal nums the smallest point, so the scan carries the point with the num)
    uint64_t mh = hi, ml = lo, mq = xy;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t th = __shfl_up(mh, o, 64), tl = __shfl_up(ml, o, 64);
      bool better = th > mh || (th == mh && tl > ml);
      if constexpr (COV) {
        const uint64_t tq = __shfl_up(mq, o, 64);
        better = better || (th == mh && tl == ml && tq < mq);
        mq = lane - o > a && better ? tq : mq;
      }
      const bool take = lane - o > a && better;
      mh = take ? th : mh;
      ml = take ? tl : ml;
    }
    const int last = cand ? b - 1 : lane;
    const uint64_t ch = __shfl(mh, last, 64), cl = __shfl(ml, last, 64);
    bool wins = cand && hi == ch && lo == cl;
    if constexpr (COV) {
      const uint64_t cq = __shfl(mq, last, 64);                         // (every lane shuffles: not behind the &&)
      wins = wins && xy == cq;
    }
    const uint64_t winners = __ballot(wins);
    const uint64_t chain = (b >= 64 ? ~0ull : (1ull << b) - 1) & ~((2ull << a) - 1);      // lanes a + 1 .. b - 1 (a < 63 here)
    const uint64_t w = cand ? winners & chain : 0ull;
    const bool free_split = COV ? ax == bx && ay == by : nr == 0;       // the anchor / a chain whose ends are one point
    const bool mark = cand && w != 0 && __builtin_ctzll(w | (1ull << 63)) == lane && (free_split || rs_over(hi, lo, den, tol2_q8));
    if (__ballot(mark) == 0 || nr >= m) break;                          // (every round keeps a new vertex: at most m)
    kept = kept || mark;
    ++nr;
  }
  const uint64_t K = __ballot(kept);
  const uint64_t hi_k = K & above_me;
  const int nb = hi_k ? __builtin_ctzll(hi_k) : 0;
  const int nx = __shfl(x, nb, 64), ny = __shfl(y, nb, 64);
  int64_t a2 = kept ? (int64_t)x * ny - (int64_t)nx * y : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a2 += __shfl_xor(a2, o, 64);
  if (valid) {
    keep[s + lane] = kept ? 1 : 0;
    pos[s + lane] = __builtin_popcountll(K & below_me);
  }
  if (lane == 0) {
    cnt[r] = __builtin_popcountll(K);
    area2[r] = a2;
    rounds[r] = nr;
  }
}

// ----------------------------------------------------------------------------------------------- one block per ring
// nearest set bit below / above position `at` in a bit mask of NW words; -1 / NW * 64: none
template <int NW>
__device__ __forceinline__ int rs_bit_below(const uint64_t* mask, int at) {
  for (int w = at >> 6; w >= 0; --w) {
    uint64_t v = mask[w];
    if (w == (at >> 6)) v &= (1ull << (at & 63)) - 1;
    if (v) return w * 64 + 63 - __builtin_clzll(v);
  }
  return -1;
}
template <int NW>
__device__ __forceinline__ int rs_bit_above(const uint64_t* mask, int at) {
  for (int w = at >> 6; w < NW; ++w) {
    uint64_t v = mask[w];
    if (w == (at >> 6)) v &= (at & 63) == 63 ? 0ull : ~((2ull << (at & 63)) - 1);
    if (v) return w * 64 + __builtin_ctzll(v);
  }
  return NW * 64;
}

template <int T, bool COV>
__global__ __launch_bounds__(T) void rs_mark_block_kernel(const int32_t* __restrict__ verts, const int64_t* __restrict__ ring_offs,
                                                          int64_t R, int64_t V, int64_t tol2_q8, int64_t longer_than,
                                                          uint8_t* __restrict__ keep, int32_t* __restrict__ pos,
                                                          int32_t* __restrict__ cnt, int64_t* __restrict__ area2,
                                                          int32_t* __restrict__ rounds) {
  constexpr int NW = T / 64;
  __shared__ int sx[RS_LDS_VERTS], sy[RS_LDS_VERTS];
  __shared__ uint8_t sk[RS_LDS_VERTS];
  __shared__ int s_first[T], s_last[T];
  __shared__ uint64_t s_has[NW], w_hi[NW], w_lo[NW];
  __shared__ int w_idx[NW], w_flag[NW], s_any[2], tmp[NW];
  __shared__ int64_t s_area[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const int64_t s = rs_clamp64(ring_offs[r], 0, V), e = rs_clamp64(ring_offs[r + 1], s, V);
    if (e - s <= longer_than) continue;                                 // uniform over the block: the wave path's
    const int m = (int)(e - s);
    const bool staged = m <= RS_LDS_VERTS;
    const int32_t* gv = verts + 2 * s;
    uint8_t* kp = keep + s;
    for (int j = tid; j < m; j += T) {
      const int k0 = j == 0 || (COV && kp[j] != 0) ? 1 : 0;              // (COV: the nodes are kept from the start)
      if (staged) { sx[j] = gv[2 * j]; sy[j] = gv[2 * j + 1]; sk[j] = (uint8_t)k0; }
      else kp[j] = (uint8_t)k0;
    }
    if (tid == 0) s_any[0] = 0;
    __syncthreads();
    auto X = [&](int j) { return staged ? sx[j] : gv[2 * j]; };
    auto Y = [&](int j) { return staged ? sy[j] : gv[2 * j + 1]; };
    // the flag byte of a vertex (bit 0: kept, bit 1: the chain that starts here is closed): in LDS with the coordinates, else
    // in the keep array itself
    auto K = [&](int j) -> int { return staged ? sk[j] : kp[j]; };
    auto setK = [&](int j, int v) { if (staged) sk[j] = (uint8_t)v; else kp[j] = (uint8_t)v; };
    // which of two vertices wins among equal nums: the lowest index; COV: the smallest point (RS_NONE loses to every vertex)
    auto less = [&](int i, int j) -> bool {
      if constexpr (COV) {
        if (i != RS_NONE && j != RS_NONE) {
          const int xi = X(i), xj = X(j);
          if (xi != xj) return xi < xj;
          const int yi = Y(i), yj = Y(j);
          if (yi != yj) return yi < yj;
        }
      }
      return i < j;
    };
    const int C = (m + T - 1) / T;
    const int c0 = min(tid * C, m), c1 = min(c0 + C, m);
    int nr = 0, prev = -1, next = m;
    // chain (a, b) with its best vertex: keep it (the anchor round keeps without the test), or close the chain for good
    auto decide = [&](const RsBest best, int a, int b) {
      if (best.idx == RS_NONE || a < 0) return;
      const int bl = b == m ? 0 : b;
      const int64_t dx = (int64_t)X(bl) - X(a), dy = (int64_t)Y(bl) - Y(a);
      const uint64_t L = (uint64_t)(dx * dx + dy * dy);
      if ((COV ? L == 0 : nr == 0) || rs_over(best.hi, best.lo, L ? L : 1, tol2_q8)) {
        setK(best.idx, 1);
        s_any[nr & 1] = 1;
      } else {
        setK(a, 3);
      }
    };
    for (;;) {
      // 1. the first and last kept vertex of every chunk; the kept vertices around the chunk
      int first = m, last = -1;
      for (int j = c0; j < c1; ++j) {
        const bool kj = K(j) != 0;
        first = kj && first == m ? j : first;
        last = kj ? j : last;
      }
      const int has = last >= 0 ? 1 : 0;
      s_first[tid] = first;
      s_last[tid] = last;
      const uint64_t bal = __ballot(has);
      if (lane == 0) s_has[wave] = bal;
      __syncthreads();
      if (tid == 0) s_any[(nr + 1) & 1] = 0;
      {
        const int p = rs_bit_below<NW>(s_has, tid), q = rs_bit_above<NW>(s_has, tid);
        prev = p >= 0 ? s_last[p] : -1;
        next = q < T ? s_first[q] : m;
      }
      // 2. the chains of the chunk: `head` reaches back into lower chunks, `tail` on into higher ones, the rest is decided here
      RsBest head{0, 0, RS_NONE}, tail{0, 0, RS_NONE};
      {
        int a = prev, j = c0;
        bool in_head = true;
        while (j < c1) {
          int jb = j;
          while (jb < c1 && K(jb) == 0) ++jb;
          const int b = jb < c1 ? jb : next;
          RsBest best{0, 0, RS_NONE};
          if (jb > j && a >= 0 && !(K(a) & 2)) {
            const int bl = b == m ? 0 : b;
            const int ax = X(a), ay = Y(a), bx = X(bl), by = Y(bl);
            for (int i = j; i < jb; ++i) {
              uint64_t den;
              const rs_u128 num = rs_num(ax, ay, bx, by, X(i), Y(i), &den);
              const uint64_t hi = (uint64_t)(num >> 64), lo = (uint64_t)num;
              if (rs_beats(hi, lo, i, best, less)) { best.hi = hi; best.lo = lo; best.idx = i; }
            }
          }
          if (in_head) head = best;
          else if (jb < c1) decide(best, a, b);
          else tail = best;
          a = jb;
          in_head = false;
          j = jb + 1;
        }
      }
      // 3. over the threads: what the lower chunks hold of the chain that reaches this one (a chunk with a kept vertex
      // starts a new chain with its tail).  Wave scan by shuffles, the wave totals through LDS.
      uint64_t eh = has ? tail.hi : head.hi, el = has ? tail.lo : head.lo;
      int ei = has ? tail.idx : head.idx, ef = has;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint64_t th = __shfl_up(eh, o, 64), tl = __shfl_up(el, o, 64);
        const int ti = __shfl_up(ei, o, 64), tf = __shfl_up(ef, o, 64);
        const bool open = lane >= o && ef == 0;
        const bool take = open && (th > eh || (th == eh && (tl > el || (tl == el && less(ti, ei)))));
        eh = take ? th : eh;
        el = take ? tl : el;
        ei = take ? ti : ei;
        ef = open ? tf : ef;
      }
      if (lane == 63) { w_hi[wave] = eh; w_lo[wave] = el; w_idx[wave] = ei; w_flag[wave] = ef; }
      RsBest inc;
      inc.hi = __shfl_up(eh, 1, 64);
      inc.lo = __shfl_up(el, 1, 64);
      inc.idx = __shfl_up(ei, 1, 64);
      int inc_f = __shfl_up(ef, 1, 64);
      if (lane == 0) { inc.hi = 0; inc.lo = 0; inc.idx = RS_NONE; inc_f = 0; }
      __syncthreads();
      if (!inc_f) {
        RsBest pre{0, 0, RS_NONE};
        for (int w = 0; w < wave; ++w) {
          const RsBest t{w_hi[w], w_lo[w], w_idx[w]};
          pre = rs_pick(w_flag[w] != 0, rs_max(pre, t, less), t);
        }
        inc = rs_max(pre, inc, less);
      }
      // 4. the thread that holds a chain's right end decides it; the chain that ends at v_m is the last thread's
      if (has) decide(rs_max(inc, head, less), prev, first);
      if (tid == T - 1) decide(rs_pick(has != 0, rs_max(inc, head, less), tail), has ? last : prev, m);
      __syncthreads();
      if (!s_any[nr & 1] || nr >= m) break;                             // uniform (every round keeps a new vertex: at most m)
      ++nr;
    }
    // positions and the doubled area of the kept ring; prev / next are still those of the last round, which kept nothing
    int c = 0;
    for (int j = c0; j < c1; ++j) c += K(j) != 0;
    int total;
    int run = rsp_block_excl_scan<T>(c, tmp, &total);
    int64_t a2 = 0;
    int pk = -1;
    for (int j = c0; j < c1; ++j) {
      const bool kj = K(j) != 0;
      pos[s + j] = run;
      kp[j] = kj ? 1 : 0;
      if (kj) {
        if (pk >= 0) a2 += (int64_t)X(pk) * Y(j) - (int64_t)X(j) * Y(pk);
        pk = j;
        ++run;
      }
    }
    if (pk >= 0) {
      const int nb = next == m ? 0 : next;
      a2 += (int64_t)X(pk) * Y(nb) - (int64_t)X(nb) * Y(pk);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a2 += __shfl_xor(a2, o, 64);
    if (lane == 0) s_area[wave] = a2;
    __syncthreads();
    if (tid == 0) {
      int64_t sum = 0;
      for (int w = 0; w < NW; ++w) sum += s_area[w];
      cnt[r] = total;
      area2[r] = sum;
      rounds[r] = nr;
    }
    __syncthreads();                                                    // the next ring reuses the LDS
  }
}

template <int T, bool COV>
int rs_launch_block(hipStream_t s, unsigned grid, const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V,
                    int64_t tol2_q8, int64_t longer_than, uint8_t* keep, int32_t* pos, int32_t* cnt, int64_t* area2,
                    int32_t* rounds) {
  hipLaunchKernelGGL((rs_mark_block_kernel<T, COV>), dim3(grid), dim3(T), 0, s, verts, ring_offs, R, V, tol2_q8, longer_than, keep, pos,
                     cnt, area2, rounds);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

// the launches of rsp_ring_simplify_mark / rsp_ring_coverage_mark: rings up to RS_WAVE_MAX vertices a wave each, longer ones a
// block each; variant 0 = 256 threads a block, 1 / 2 = 128 / 512, 3 = every ring through the block path
template <bool COV>
int rs_mark(const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V, int64_t tol2_q8, int32_t H, int32_t W,
            int32_t variant, uint8_t* keep, int32_t* pos, int32_t* kept_cnt, int64_t* area2, int32_t* rounds, hipStream_t s) {
  if (R < 0 || R > 0x7fffffffLL || V < 0 || V > 0x7fffffffLL || tol2_q8 < 0 || tol2_q8 > RS_MAX_TOL2_Q8) return RSP_EINVAL;
  if (H < 1 || W < 1 || H > RS_MAX_SIDE || W > RS_MAX_SIDE || variant < 0 || variant > 3) return RSP_EINVAL;
  if (!ring_offs || (R > 0 && (!kept_cnt || !area2 || !rounds)) || (V > 0 && (!verts || !keep || !pos))) return RSP_EINVAL;
  if (R == 0) return RSP_OK;
  const int64_t longer_than = variant == 3 ? -1 : RS_WAVE_MAX;           // variant 3: every ring takes the block path
  if (variant != 3) {
    const unsigned nb = (unsigned)((R + RS_WAVE_THREADS / 64 - 1) / (RS_WAVE_THREADS / 64));
    hipLaunchKernelGGL(rs_mark_wave_kernel<COV>, dim3(nb), dim3(RS_WAVE_THREADS), 0, s, verts, ring_offs, R, V, tol2_q8, keep, pos,
                       kept_cnt, area2, rounds);
    RSP_CHECK_LAUNCH();
  }
  const unsigned grid = (unsigned)(R < RS_MAX_BLOCKS ? R : RS_MAX_BLOCKS);
  if (variant == 1) return rs_launch_block<128, COV>(s, grid, verts, ring_offs, R, V, tol2_q8, longer_than, keep, pos, kept_cnt, area2, rounds);
  if (variant == 2) return rs_launch_block<512, COV>(s, grid, verts, ring_offs, R, V, tol2_q8, longer_than, keep, pos, kept_cnt, area2, rounds);
  return rs_launch_block<256, COV>(s, grid, verts, ring_offs, R, V, tol2_q8, longer_than, keep, pos, kept_cnt, area2, rounds);
}

}  // namespace
