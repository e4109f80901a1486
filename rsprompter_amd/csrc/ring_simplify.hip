// Polygon simplification: exact Douglas-Peucker on the rings of polygon export (csrc/mask_polygons.hip), on
// the device.  Input: verts int32 [V, 2] and ring_offs int64 [R + 1]; ring r is v_0 .. v_{m-1}, closed by v_m := v_0.
//
// THE CONTRACT (tests/_ring_simplify_ref.py states it sequentially).  Index 0 is kept; so is f = argmax |v_i - v_0|^2 over
// 0 < i < m.  A chain (a, b) of two kept indices with b - a >= 2 looks at its inner vertices: num_i / den = the squared
// distance of v_i to the SEGMENT v_a v_b (den = |v_b - v_a|^2, or 1 where the two coincide), s = argmax num_i, and splits
// at s -- s is kept, (a, s) and (s, b) go on -- iff 256 num_s > tol2_q8 den.  Lowest index among equals, everywhere.  The
// anchor f is the split of the chain (0, m) (its ends coincide, num = |v_i - v_0|^2) taken without the tolerance test.
// num reaches 2^82 for coordinates in [0, 2^20]: every product and comparison is an unsigned 128-bit integer one.
//
// ROUNDS (the two mark kernels live in ring_mark.h, which shared-border simplification instantiates with its own rules; here
// COV = false).  The chains of one ring are independent, so all of them split at once: per round every vertex that is not kept
// finds the kept pair around it from the keep flags, computes its num, a segmented arg-max gives every chain its winner,
// and the winners over the tolerance are kept.  A ring ends with the first round that keeps nothing; the whole fixed point
// runs inside one launch (the depth of the split tree depends on the data and reaches m / 2).
//   rs_mark_wave_kernel   m <= 64: one wave per ring, lane = vertex.  The keep flags are one ballot, the kept pair of a lane
//                         two bit scans of it, the arg-max a segmented shuffle scan.  No LDS, no barrier, 4 rings a block.
//   rs_mark_block_kernel  longer rings: one block per ring, a thread owns a contiguous chunk of vertices.  Chunk summaries
//                         (first / last kept vertex; the best vertex of the chains that leave the chunk) are scanned over
//                         the block through LDS; a chain inside one chunk is decided by its thread alone.  Coordinates sit
//                         and keep flags sit in LDS up to RS_LDS_VERTS vertices and in memory beyond that.  A chain that failed the
//                         test never changes again: bit 1 of its left end's flag byte lets the later rounds skip it.
// Both write the keep flag of every vertex, the number of kept vertices in front of it, the kept count and the doubled area
// of the kept ring (an int64 shoelace sum: independent of the order), and the number of rounds that kept something.
// rs_survive_kernel says which rings stay (ring survival), rs_write_kernel compacts them.  No atomics: a second
// launch is bit-identical.
#include "rsp_common.h"
#include "ring_mark.h"

namespace {

// --------------------------------------------------------------------------------------------------------- output
// Which rings stay, one lane per ring, in this order: at least min_area pixels BEFORE simplification, at least 3 kept vertices,
// a new doubled area that is not 0 and has the old one's sign, and for a hole an outer ring that stays.  A hole's parent is
// an outer ring, so one look at it is the whole rule.  sums[r] = 1 / 0, sums[R + r] = the ring's kept vertices / 0: the host
// takes ONE inclusive sum over both rows.
__device__ __forceinline__ bool rs_stays(int64_t old_a2, int64_t new_a2, int cnt, int64_t min_area) {
  const uint64_t mag = old_a2 < 0 ? 0 - (uint64_t)old_a2 : (uint64_t)old_a2;
  return (int64_t)(mag >> 1) >= min_area && cnt >= 3 && new_a2 != 0 && (new_a2 > 0) == (old_a2 > 0);
}
__global__ __launch_bounds__(256) void rs_survive_kernel(const int32_t* __restrict__ ring_inst, const int32_t* __restrict__ ring_parent,
                                                         const int64_t* __restrict__ ring_area2,
                                                         const int64_t* __restrict__ inst_ring_offs, int64_t R, int k,
                                                         int64_t min_area, const int32_t* __restrict__ cnt,
                                                         const int64_t* __restrict__ area2_new, int64_t* __restrict__ sums) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const int inst = ring_inst[r], par = ring_parent[r];
  bool ok = inst >= 0 && inst < k && rs_stays(ring_area2[r], area2_new[r], cnt[r], min_area);
  if (ok && par >= 0) {
    const int64_t pr = inst_ring_offs[inst] + par;
    ok = pr >= 0 && pr < R && rs_stays(ring_area2[pr], area2_new[pr], cnt[pr], min_area);
  }
  sums[r] = ok ? 1 : 0;
  sums[R + r] = ok ? cnt[r] : 0;
}

// One lane per vertex, per ring and per instance.  flags = the sums rows above, csum = their inclusive sums over the rings:
// ring r is survivor csum[r] - 1 and its vertices start at csum[R + r] - flags[R + r].
__global__ __launch_bounds__(256) void rs_write_kernel(const int32_t* __restrict__ verts, const int64_t* __restrict__ ring_offs,
                                                       const int32_t* __restrict__ ring_inst, const int32_t* __restrict__ ring_parent,
                                                       const int64_t* __restrict__ inst_ring_offs, int64_t R, int64_t V, int k,
                                                       const uint8_t* __restrict__ keep, const int32_t* __restrict__ pos,
                                                       const int64_t* __restrict__ area2_new, const int64_t* __restrict__ flags,
                                                       const int64_t* __restrict__ csum, int64_t R2, int64_t V2,
                                                       int32_t* __restrict__ verts_out, int64_t* __restrict__ ring_offs_out,
                                                       int32_t* __restrict__ inst_out, int32_t* __restrict__ parent_out,
                                                       int64_t* __restrict__ area2_out, int64_t* __restrict__ inst_offs_out,
                                                       int32_t* __restrict__ src_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < V && keep[i]) {
    int64_t lo = 0, hi = R;                                             // the last ring with ring_offs[r] <= i
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (ring_offs[mid] <= i) lo = mid; else hi = mid;
    }
    if (flags[lo] && i >= ring_offs[lo] && i < ring_offs[lo + 1]) {
      const int64_t end = csum[R + lo], first = end - flags[R + lo], slot = first + pos[i];
      if (slot >= first && slot < end && slot >= 0 && slot < V2) {
        verts_out[2 * slot] = verts[2 * i];
        verts_out[2 * slot + 1] = verts[2 * i + 1];
      }
    }
  }
  if (i < R && flags[i]) {
    const int64_t nr = csum[i] - 1;
    if (nr >= 0 && nr < R2) {
      const int inst = ring_inst[i], par = ring_parent[i];
      int np = -1;
      if (par >= 0 && inst >= 0 && inst < k) {
        const int64_t pr = inst_ring_offs[inst] + par, i0 = inst_ring_offs[inst];
        if (pr >= 0 && pr < R && flags[pr] && i0 >= 0 && i0 <= R) np = (int)(csum[pr] - 1 - (i0 > 0 ? csum[i0 - 1] : 0));
      }
      ring_offs_out[nr] = csum[R + i] - flags[R + i];
      inst_out[nr] = inst;
      parent_out[nr] = np;
      area2_out[nr] = area2_new[i];
      src_out[nr] = (int32_t)i;
    }
  }
  if (i <= k) {
    const int64_t o = rs_clamp64(inst_ring_offs[i], 0, R);
    inst_offs_out[i] = o > 0 ? csum[o - 1] : 0;
  }
  if (i == 0) ring_offs_out[R2] = V2;
}

}  // namespace

extern "C" int rsp_ring_simplify_mark(const int32_t* verts, const int64_t* ring_offs, int64_t R, int64_t V, int64_t tol2_q8,
                                      int32_t H, int32_t W, int32_t variant, uint8_t* keep, int32_t* pos, int32_t* kept_cnt,
                                      int64_t* area2, int32_t* rounds, rsp_stream_t stream) {
  return rs_mark<false>(verts, ring_offs, R, V, tol2_q8, H, W, variant, keep, pos, kept_cnt, area2, rounds, (hipStream_t)stream);
}

extern "C" int rsp_ring_simplify_survive(const int32_t* ring_inst, const int32_t* ring_parent, const int64_t* ring_area2,
                                         const int64_t* inst_ring_offs, int64_t R, int32_t k, int64_t min_ring_area,
                                         const int32_t* kept_cnt, const int64_t* area2_new, int64_t* sums, rsp_stream_t stream) {
  if (R < 0 || R > 0x7fffffffLL || k < 0 || min_ring_area < 0) return RSP_EINVAL;
  if (R == 0) return RSP_OK;
  if (!ring_inst || !ring_parent || !ring_area2 || !inst_ring_offs || !kept_cnt || !area2_new || !sums) return RSP_EINVAL;
  hipLaunchKernelGGL(rs_survive_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ring_inst, ring_parent,
                     ring_area2, inst_ring_offs, R, (int)k, min_ring_area, kept_cnt, area2_new, sums);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_ring_simplify_write(const int32_t* verts, const int64_t* ring_offs, const int32_t* ring_inst,
                                       const int32_t* ring_parent, const int64_t* inst_ring_offs, int64_t R, int64_t V, int32_t k,
                                       const uint8_t* keep, const int32_t* pos, const int64_t* area2_new, const int64_t* sums,
                                       const int64_t* csum, int64_t R2, int64_t V2, int32_t* verts_out, int64_t* ring_offs_out,
                                       int32_t* ring_inst_out, int32_t* ring_parent_out, int64_t* ring_area2_out,
                                       int64_t* inst_ring_offs_out, int32_t* ring_src_out, rsp_stream_t stream) {
  if (R < 0 || R > 0x7fffffffLL || V < 0 || V > 0x7fffffffLL || k < 0 || R2 < 0 || R2 > R || V2 < 0 || V2 > V) return RSP_EINVAL;
  if (R2 == 0) return RSP_OK;
  if (!verts || !ring_offs || !ring_inst || !ring_parent || !inst_ring_offs || !keep || !pos || !area2_new || !sums || !csum ||
      !ring_offs_out || !ring_inst_out || !ring_parent_out || !ring_area2_out || !inst_ring_offs_out || !ring_src_out ||
      (V2 > 0 && !verts_out))
    return RSP_EINVAL;
  int64_t n = V > R ? V : R;
  n = n > (int64_t)k + 1 ? n : (int64_t)k + 1;
  hipLaunchKernelGGL(rs_write_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, ring_offs,
                     ring_inst, ring_parent, inst_ring_offs, R, V, (int)k, keep, pos, area2_new, sums, csum, R2, V2, verts_out,
                     ring_offs_out, ring_inst_out, ring_parent_out, ring_area2_out, inst_ring_offs_out, ring_src_out);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
