// The selection core shared by box NMS and RPN top-k (csrc/det.hip), query top-k (csrc/query.hip) and rotated NMS
// (csrc/obb_iou.hip): the ordered-score key, the descending bitonic sort and the greedy walk over a
// suppression mask.
//
// THE CANONICAL ORDER of every selection entry point: score descending, original position ascending.  One 64-bit key holds
// both, (ordered score << 32) | ~position, so that sorting keys DESCENDING gives exactly that order; key 0 is below every real
// key and pads a sort to a power of two.  tests/_det_props.py pins the order to exact references.
// Include it after rsp_common.h (it does not include it itself: the emulated build rewrites that include per source file).
#pragma once

namespace {

// order-preserving float -> uint and back: a < b as floats  =>  nms_f2ord(a) < nms_f2ord(b) as unsigned (and -0 below +0)
__device__ __forceinline__ uint32_t nms_f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float nms_ord2f(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}
__device__ __forceinline__ unsigned long long nms_key_ord(uint32_t ord, int pos) {    // of a score that is ordered already
  return ((unsigned long long)ord << 32) | (uint32_t)(0xffffffffu - (uint32_t)pos);
}
__device__ __forceinline__ unsigned long long nms_key(float score, int pos) { return nms_key_ord(nms_f2ord(score), pos); }
__device__ __forceinline__ int nms_key_pos(unsigned long long key) {
  return (int)(0xffffffffu - (uint32_t)(key & 0xffffffffull));
}
__device__ __forceinline__ float nms_key_score(unsigned long long key) { return nms_ord2f((uint32_t)(key >> 32)); }

// Bitonic sort of n (a power of two) 64-bit keys, DESCENDING, by all threads of the block; `keys` is LDS or global memory.
// The keys are written and a barrier passed before the call; it ends with a barrier.
__device__ __forceinline__ void nms_sort_desc(unsigned long long* keys, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = keys[i], b = keys[ixj];
          const bool desc = ((i & k) == 0);
          if (desc ? (a < b) : (a > b)) { keys[i] = b; keys[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// THE MASK CONTRACT.  n candidates in canonical order; `mask` is row-major n x words 64-bit words, words >= ceil(n / 64).
// Bit (j & 63) of word (j >> 6) of row i says that a kept i suppresses j; a set bit implies i < j < n.  A producer writes, of
// every row i < n, the words (i >> 6) .. ceil(n / 64) - 1: the diagonal word, whose bits up to and including i's own are
// clear, and everything to its right.  The words left of the diagonal are never read and need not be written.  The walk
// reads the diagonal word of every row of a block it reaches, and the words right of it of the rows it keeps.
//
// THE GREEDY WALK, one wave (a block of 64 threads) per candidate set: rows in order; a row that no kept row has suppressed
// is kept, sorder[row] is appended to `keep`, and its bits are or-ed into the removal words; at most max_out rows are kept
// and keep_cnt is their number.  Lane l holds the removal words l, l + 64, ... in NMS_MAXW registers: words <= 64 * NMS_MAXW.
// A block's inputs -- its diagonal mask word and its sort-order entry per row -- are requested one block AHEAD, and the
// rows a block keeps are propagated CH at a time with their loads in flight together: the walk is serial by nature, and its
// counters showed it 81 % of its cycles waiting for one load after the other before that.
// P is the caller's parameter struct: NmsWalkP, or one that has its fields among others (det.hip's NmsP).  A kernel, not
// a device function: DESIGN §14.18.
struct NmsWalkP {
  const unsigned long long* mask;  // [B, cap, words]
  const int32_t* sorder;           // [B, cap]  original position of the sorted candidate
  const int32_t* cnt;              // [B]       candidates of the set, <= cap
  int cap, words, max_out;
  int32_t* keep;                   // [B, max_out] original positions, canonical order
  int32_t* keep_cnt;               // [B]
};
template <int NMS_MAXW, typename P>
__global__ __launch_bounds__(64) void nms_walk_kernel(const P p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = p.cnt[b];
  const int nblk = (n + 63) / 64;
  unsigned long long remv[NMS_MAXW];
#pragma unroll
  for (int i = 0; i < NMS_MAXW; ++i) remv[i] = 0ull;
  const unsigned long long* mask = p.mask + (int64_t)b * p.cap * p.words;
  const int32_t* sorder = p.sorder + (int64_t)b * p.cap;
  int32_t* keep = p.keep + (int64_t)b * p.max_out;
  int kept = 0;
  auto load_blk = [&](int bk, unsigned long long& dm, int& so) {
    const int r = bk * 64 + lane;
    const bool ok = bk < nblk && r < n;
    dm = ok ? mask[(int64_t)r * p.words + bk] : 0ull;
    so = ok ? sorder[r] : 0;
  };
  unsigned long long dmask;
  int sord;
  load_blk(0, dmask, sord);
  for (int blk = 0; blk < nblk && kept < p.max_out; ++blk) {
    unsigned long long dnext;
    int snext;
    load_blk(blk + 1, dnext, snext);
    // removal word of this block lives in lane (blk & 63), slot (blk >> 6)
    unsigned long long mine = 0ull;
#pragma unroll
    for (int i = 0; i < NMS_MAXW; ++i) if (i == (blk >> 6)) mine = remv[i];
    const unsigned int lo = __shfl((unsigned int)(mine & 0xffffffffull), blk & 63, 64);
    const unsigned int hi = __shfl((unsigned int)(mine >> 32), blk & 63, 64);
    unsigned long long cur = ((unsigned long long)hi << 32) | lo;
    const int rows_here = min(64, n - blk * 64);
    unsigned long long kept_bits = 0ull;
    for (int t = 0; t < rows_here; ++t) {
      const unsigned int dlo = __shfl((unsigned int)(dmask & 0xffffffffull), t, 64);
      const unsigned int dhi = __shfl((unsigned int)(dmask >> 32), t, 64);
      const int so = __shfl(sord, t, 64);
      if (!((cur >> t) & 1ull)) {
        if (kept < p.max_out) {
          kept_bits |= (1ull << t);
          if (lane == 0) keep[kept] = so;
          ++kept;
          cur |= ((unsigned long long)dhi << 32) | dlo;
        }
      }
    }
    if (kept >= p.max_out) break;
    // propagate the kept rows of this block to all later words
    constexpr int CH = NMS_MAXW <= 4 ? 4 : 1;              // rows per batch of loads (register budget of the large form)
    unsigned long long kb = kept_bits;
    while (kb) {
      int tt[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        tt[j] = -1;
        if (kb) { tt[j] = __builtin_ctzll(kb); kb &= kb - 1ull; }
      }
      unsigned long long v[CH][NMS_MAXW];
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const unsigned long long* mrow = mask + (int64_t)(blk * 64 + max(tt[j], 0)) * p.words;
#pragma unroll
        for (int i = 0; i < NMS_MAXW; ++i) {
          const int w = lane + 64 * i;
          v[j][i] = (tt[j] >= 0 && w > blk && w < nblk) ? mrow[w] : 0ull;
        }
      }
#pragma unroll
      for (int j = 0; j < CH; ++j)
#pragma unroll
        for (int i = 0; i < NMS_MAXW; ++i) remv[i] |= v[j][i];
    }
    dmask = dnext;
    sord = snext;
  }
  if (lane == 0) p.keep_cnt[b] = kept;
}

// THE TWO FORMS of the walk and the one rule that chooses between them: 4 removal words a lane (64 * 4 words = 16384
// candidates, the RSPrompter sizes) where they suffice, else RSP_NMS_MAX_CANDIDATES / 4096 = 32 (131072 candidates).
// B candidate sets, a 64-thread block each; the caller checks the launch.
constexpr int NMS_MAXW_SMALL = 4;
constexpr int NMS_MAXW_LARGE = RSP_NMS_MAX_CANDIDATES / (64 * 64);
template <typename P>
inline void nms_walk_launch(const P& p, int B, hipStream_t s) {
  if (p.words <= 64 * NMS_MAXW_SMALL) hipLaunchKernelGGL((nms_walk_kernel<NMS_MAXW_SMALL, P>), dim3(B), dim3(64), 0, s, p);
  else hipLaunchKernelGGL((nms_walk_kernel<NMS_MAXW_LARGE, P>), dim3(B), dim3(64), 0, s, p);
}

}  // namespace
