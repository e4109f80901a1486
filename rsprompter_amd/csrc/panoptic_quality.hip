// Panoptic quality: pq_compute_single_core (mmdet/evaluation/functional/panoptic_utils.py:60-169) behind CocoPanopticMetric
// (mmdet/evaluation/metrics/coco_panoptic_metric.py:270-297 _parse_predictions, :309-387 _compute_batch_pq_stats, :529-531 the
// sum of the images) for one image, nothing read by the host:
//   present    void ids -> 0 (:279-281, :296-297), the distinct predicted ids as bits of a presence bitmap          (np.unique, :273)
//   rank       popcount + prefix over the bitmap: bit -> slot in np.unique order, P = the number of segments
//   confusion  the joint histogram of (gt id, pred id) over all pixels                                             (:110-117)
//   match      areas (:86-95), TP by iou > 0.5 in ascending (gt id, pred id) (:122-141), FN (:145-152), FP (:155-169)
//   reduce     PQStat.__iadd__ over the images in order                                                            (:529-531)
// The reference writes the map as a PNG, reads it back and runs np.unique over H * W 64-bit keys twice; here both maps are read
// twice as they are (the ground truth as RGB bytes with rgb2id folded into the load, or as int32 ids).  The maps are piecewise
// constant: a thread run-compresses a strip of PQ_STRIP pixels and issues one integer atomic per run.  Integer atomics only:
// the same bits on every run.  The two `> 0.5` tests: the TP test is the reference's double division (the quotient is also
// the summand); the FP test is its integer form 2 * a > b, equal for areas below 2^31.
#include "rsp_common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int PQ_MAXP = RSP_PQ_MAX_SEGMENTS;
constexpr int PQ_MAXID = RSP_PQ_MAX_PRED_ID;
constexpr int PQ_WORDS = PQ_MAXID / 32;                  // presence bitmap, 256 KiB
constexpr int PQ_STRIP = 16;                             // pixels per thread: four 16-byte loads of ids, three of RGB bytes
constexpr int PQ_LABELS = 1000;                          // INSTANCE_OFFSET (panoptic_utils.py:18): label = id % 1000

// workspace (int32 words): status | P | pad | bitmap [PQ_WORDS] | conf [(G + 2) * (PQ_MAXP + 1)] (used: (G + 2) * (P + 1)) |
// word base [PQ_WORDS] (the number of set bits in front of a word; written for non-empty words only).  Everything in front of
// the word bases starts as zero (one memset).
constexpr int WS_STATUS = 0, WS_P = 1, WS_BITS = 4, WS_CONF = WS_BITS + PQ_WORDS;
inline int64_t ws_base_of(int G) { return (int64_t)WS_CONF + (int64_t)(G + 2) * (PQ_MAXP + 1); }

// tables (int32, written by the host): gt id ascending [G] | category index [G] | iscrowd [G] | area [G] (< 0: count the row) |
// category index of a label [PQ_LABELS] (-1: none) | crowd_of [n_cat]: the slot of the last crowd segment in JSON order, -1
struct PqTables {
  const int32_t *gt_id, *gt_cat, *gt_crowd, *gt_area, *label_cat, *crowd_of;
};
inline PqTables pq_tables(const int32_t* t, int G) {
  return PqTables{t, t + G, t + 2 * G, t + 3 * G, t + 4 * G, t + 4 * G + PQ_LABELS};
}

// a raw predicted id as the evaluation sees it: 0 for void, -1 with a status bit for an id that is refused
__device__ __forceinline__ int pq_pred_id(int raw, int nc, int ign, int* bad) {
  if (raw < 0 || raw >= PQ_MAXID) { *bad |= RSP_PQ_STATUS_PRED_ID_RANGE; return -1; }
  const int label = raw % PQ_LABELS;
  if (label == nc || label == ign) return 0;
  if (raw == 0) { *bad |= RSP_PQ_STATUS_PRED_ID_ZERO; return -1; }
  return raw;
}

// the PQ_STRIP predicted ids of a strip; pixels past the end repeat the last one in front of them (no new run)
__device__ __forceinline__ void pq_load_ids(const int32_t* __restrict__ map, int64_t base, int nv, int v[PQ_STRIP]) {
  if (nv == PQ_STRIP) {
#pragma unroll
    for (int k = 0; k < PQ_STRIP / 4; ++k) {
      const i32x4 q = *reinterpret_cast<const i32x4*>(map + base + 4 * k);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * k + e] = q[e];
    }
  } else {
    int last = 0;
#pragma unroll
    for (int e = 0; e < PQ_STRIP; ++e) {
      if (e < nv) last = map[base + e];
      v[e] = last;
    }
  }
}

// ... and of an RGB map, rgb2id (R + 256 G + 65536 B) folded into the load: pixel e is the 24-bit little-endian value at byte 3 e
__device__ __forceinline__ void pq_load_rgb(const uint8_t* __restrict__ rgb, int64_t base, int nv, int v[PQ_STRIP]) {
  if (nv == PQ_STRIP) {
    unsigned w[PQ_STRIP * 3 / 4 + 1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const u32x4 q = *reinterpret_cast<const u32x4*>(rgb + base * 3 + 16 * k);
#pragma unroll
      for (int e = 0; e < 4; ++e) w[4 * k + e] = q[e];
    }
    w[PQ_STRIP * 3 / 4] = 0u;
#pragma unroll
    for (int e = 0; e < PQ_STRIP; ++e) {
      const int j = (3 * e) >> 2, s = ((3 * e) & 3) * 8;
      const uint64_t pair = ((uint64_t)w[j + 1] << 32) | w[j];
      v[e] = (int)((unsigned)(pair >> s) & 0xffffffu);
    }
  } else {
    int last = 0;
#pragma unroll
    for (int e = 0; e < PQ_STRIP; ++e) {
      if (e < nv) {
        const uint8_t* px = rgb + (base + e) * 3;
        last = (int)px[0] | ((int)px[1] << 8) | ((int)px[2] << 16);
      }
      v[e] = last;
    }
  }
}

__device__ __forceinline__ int pq_strip_pixels(int64_t base, int64_t N) {
  const int64_t left = N - base;
  return left >= PQ_STRIP ? PQ_STRIP : (left > 0 ? (int)left : 0);
}

// ----------------------------------------------------------------------------------------------------------- present
__global__ __launch_bounds__(256) void pq_present_kernel(const int32_t* __restrict__ pred, int64_t N, int nc, int ign,
                                                         int32_t* __restrict__ ws) {
  const int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PQ_STRIP;
  const int nv = pq_strip_pixels(base, N);
  if (nv == 0) return;                                     // no block-wide step in this kernel
  int v[PQ_STRIP];
  pq_load_ids(pred, base, nv, v);
  unsigned* bits = reinterpret_cast<unsigned*>(ws + WS_BITS);
  int bad = 0;
  int prev = v[0] + 1;                                     // differs from v[0]
#pragma unroll
  for (int e = 0; e < PQ_STRIP; ++e) {
    if (v[e] != prev) {
      prev = v[e];
      const int id = pq_pred_id(prev, nc, ign, &bad);
      if (id > 0) {
        const unsigned bit = 1u << (id & 31);
        // the plain read spares the atomic once the bit is there (a stale 0 only costs the atomic)
        if (!(bits[id >> 5] & bit)) atomicOr(&bits[id >> 5], bit);
      }
    }
  }
  if (bad) atomicOr(&ws[WS_STATUS], bad);
}

// -------------------------------------------------------------------------------------------------------------- rank
// one block of 1024 threads, 64 consecutive words each: the exclusive prefix of the popcounts is the np.unique slot of a word's
// first set bit.  Writes the ids in slot order, P (0 when the row is refused: the later kernels then touch nothing) and the
// status bit of P > PQ_MAXP.
__global__ __launch_bounds__(1024) void pq_rank_kernel(int32_t* __restrict__ ws, int32_t* __restrict__ word_base,
                                                       int32_t* __restrict__ pred_ids) {
  __shared__ int s_tmp[16];
  const unsigned* mine = reinterpret_cast<const unsigned*>(ws + WS_BITS) + threadIdx.x * 64;
  int c = 0;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const u32x4 q = *reinterpret_cast<const u32x4*>(mine + 4 * k);
    c += __popc(q[0]) + __popc(q[1]) + __popc(q[2]) + __popc(q[3]);
  }
  int total;
  int slot = rsp_block_excl_scan<1024>(c, s_tmp, &total);
  if (c) {
    for (int k = 0; k < 64; ++k) {
      unsigned word = mine[k];
      if (!word) continue;
      word_base[threadIdx.x * 64 + k] = slot;
      while (word) {
        const int b = __builtin_ctz(word);
        if (slot < PQ_MAXP) pred_ids[slot] = (threadIdx.x * 64 + k) * 32 + b;
        ++slot;
        word &= word - 1;
      }
    }
  }
  if (threadIdx.x == 0) {
    int st = ws[WS_STATUS];
    if (total > PQ_MAXP) st |= RSP_PQ_STATUS_TOO_MANY_SEGMENTS;
    ws[WS_STATUS] = st;
    ws[WS_P] = st ? 0 : total;
  }
}

// --------------------------------------------------------------------------------------------------------- confusion
// rows: 0 = VOID, 1 + the slot of a listed gt id, G + 1 = a gt id that is not listed; columns: 0 = void, 1 + the np.unique slot
template <bool GT_RGB>
__global__ __launch_bounds__(256) void pq_confusion_kernel(const int32_t* __restrict__ pred, const void* __restrict__ gt,
                                                           int64_t N, int nc, int ign, const int32_t* __restrict__ gt_id,
                                                           int G, int32_t* __restrict__ ws,
                                                           const int32_t* __restrict__ word_base) {
  __shared__ int s_gt[PQ_MAXP];
  if (ws[WS_STATUS]) return;                               // uniform: a refused row counts nothing
  const int stride = ws[WS_P] + 1;
  for (int i = threadIdx.x; i < G; i += 256) s_gt[i] = gt_id[i];
  __syncthreads();
  const int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PQ_STRIP;
  const int nv = pq_strip_pixels(base, N);                 // 0 past the end: every pixel dead, nothing loaded
  if (nv == 0) return;                                     // (behind the last block-wide step)
  int pv[PQ_STRIP], gv[PQ_STRIP];
  pq_load_ids(pred, base, nv, pv);
  if (GT_RGB) pq_load_rgb(static_cast<const uint8_t*>(gt), base, nv, gv);
  else pq_load_ids(static_cast<const int32_t*>(gt), base, nv, gv);
  const unsigned* bits = reinterpret_cast<const unsigned*>(ws + WS_BITS);
  int32_t* conf = ws + WS_CONF;
  auto gslot = [&](int id) {
    if (id == 0) return 0;
    int lo = 0, hi = G;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_gt[mid] < id) lo = mid + 1; else hi = mid;
    }
    return (lo < G && s_gt[lo] == id) ? lo + 1 : G + 1;
  };
  auto pslot = [&](int raw) {
    int bad = 0;
    const int id = pq_pred_id(raw, nc, ign, &bad);         // never refused here: the status is clear
    if (id <= 0) return 0;
    return 1 + word_base[id >> 5] + (int)__popc(bits[id >> 5] & ((1u << (id & 31)) - 1u));
  };
  int pg = gv[0], pp = pv[0], gs = gslot(pg), ps = pslot(pp), cnt = 0;
#pragma unroll
  for (int e = 0; e < PQ_STRIP; ++e) {
    if (e < nv) {
      if (gv[e] != pg || pv[e] != pp) {
        atomicAdd(&conf[gs * stride + ps], cnt);
        cnt = 0;
        if (gv[e] != pg) { pg = gv[e]; gs = gslot(pg); }
        if (pv[e] != pp) { pp = pv[e]; ps = pslot(pp); }
      }
      ++cnt;
    }
  }
  atomicAdd(&conf[gs * stride + ps], cnt);
}

// ------------------------------------------------------------------------------------------------------------- match
__global__ __launch_bounds__(256) void pq_match_kernel(const int32_t* __restrict__ ws, const PqTables t, int G, int n_cat,
                                                       int32_t* __restrict__ tp, int32_t* __restrict__ fp,
                                                       int32_t* __restrict__ fn, double* __restrict__ iou_sum,
                                                       int32_t* __restrict__ status, int32_t* __restrict__ n_pred,
                                                       int32_t* __restrict__ pred_ids, int32_t* __restrict__ pred_cat,
                                                       int32_t* __restrict__ pred_area) {
  __shared__ int s_area[PQ_MAXP + 1], s_void[PQ_MAXP + 1], s_pcat[PQ_MAXP + 1], s_pstate[PQ_MAXP + 1], s_gmatch[PQ_MAXP];
  __shared__ double s_giou[PQ_MAXP];
  __shared__ int s_bad;
  const int st = ws[WS_STATUS], P = ws[WS_P], stride = P + 1;
  const int32_t* conf = ws + WS_CONF;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_bad = st;
  for (int i = P + threadIdx.x; i < PQ_MAXP; i += 256) { pred_ids[i] = -1; pred_cat[i] = -1; pred_area[i] = 0; }
  // ---- predicted segments: area = the column sum (every gt id counts, listed or not), category, overlap with VOID
  int bad = 0;
  for (int p = threadIdx.x; p <= P; p += 256) {
    int a = 0;
    for (int r = 0; r < G + 2; ++r) a += conf[r * stride + p];
    int cat = -1;
    if (p >= 1) {
      cat = t.label_cat[pred_ids[p - 1] % PQ_LABELS];
      if (cat < 0) bad |= RSP_PQ_STATUS_PRED_CATEGORY;
      pred_cat[p - 1] = cat;
      pred_area[p - 1] = a;
    }
    s_area[p] = a; s_void[p] = conf[p]; s_pcat[p] = cat; s_pstate[p] = 0;
  }
  for (int g = threadIdx.x; g < G; g += 256) s_gmatch[g] = 0;
  __syncthreads();
  // ---- TP: one wave per listed gt segment; at most one pair per row and per column passes iou > 0.5, so no write conflicts
  for (int g = wave; g < G; g += 4) {
    const int32_t* row = conf + (g + 1) * stride;
    if (t.gt_crowd[g]) continue;
    int counted = 0;                                       // (pan_gt == id).sum(): the dataset path's area
    for (int p = lane; p <= P; p += 64) counted += row[p];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) counted += __shfl_xor(counted, o, 64);
    int area_g = t.gt_area[g];
    if (area_g < 0) area_g = counted;
    // a listed area below the pixels the segment has in the map is refused: with it a union can be 0 (Python divides by zero)
    // and two pairs of one row or column can pass 0.5
    if (area_g < counted) { bad |= RSP_PQ_STATUS_GT_AREA; continue; }
    const int cat = t.gt_cat[g];
    for (int p = 1 + lane; p <= P; p += 64) {
      const int inter = row[p];
      if (inter <= 0 || s_pcat[p] != cat) continue;
      const int64_t uni = (int64_t)s_area[p] + area_g - inter - s_void[p];          // >= area_g >= inter > 0
      const double iou = (double)inter / (double)uni;                // panoptic_utils.py:136
      if (iou > 0.5) { s_gmatch[g] = p; s_giou[g] = iou; s_pstate[p] = 1; }
    }
  }
  if (bad) atomicOr(&s_bad, bad);
  __syncthreads();
  // ---- FP: an unmatched segment unless more than half of it is VOID or the crowd region of its category (:155-169)
  for (int p = 1 + threadIdx.x; p <= P; p += 256) {
    if (s_pstate[p] || s_pcat[p] < 0) continue;
    const int co = t.crowd_of[s_pcat[p]];
    const int64_t ign = (int64_t)s_void[p] + (co >= 0 ? conf[(co + 1) * stride + p] : 0);
    if (!(2 * ign > (int64_t)s_area[p])) s_pstate[p] = 2;
  }
  __syncthreads();
  // ---- per category, gt in ascending id: the order of the reference's double sum
  const int refused = s_bad;
  for (int c = threadIdx.x; c < n_cat; c += 256) {
    int ntp = 0, nfp = 0, nfn = 0;
    double s = 0.0;
    for (int g = 0; g < G; ++g) {
      if (t.gt_cat[g] != c || t.gt_crowd[g]) continue;
      if (s_gmatch[g]) { ++ntp; s += s_giou[g]; } else ++nfn;
    }
    for (int p = 1; p <= P; ++p) nfp += (s_pcat[p] == c && s_pstate[p] == 2) ? 1 : 0;
    tp[c] = refused ? 0 : ntp; fp[c] = refused ? 0 : nfp; fn[c] = refused ? 0 : nfn; iou_sum[c] = refused ? 0.0 : s;
  }
  if (refused)                                             // a status found here: the segment list goes with the row
    for (int i = threadIdx.x; i < P; i += 256) { pred_ids[i] = -1; pred_cat[i] = -1; pred_area[i] = 0; }
  if (threadIdx.x == 0) { *status = refused; *n_pred = refused ? 0 : P; }
}

// ------------------------------------------------------------------------------------------------------------ reduce
// one lane per category, images in order: ((0 + s1) + s2) + ... as PQStat.__iadd__ (coco_panoptic_metric.py:529-531)
__global__ __launch_bounds__(256) void pq_reduce_kernel(const int32_t* __restrict__ tp, const int32_t* __restrict__ fp,
                                                        const int32_t* __restrict__ fn, const double* __restrict__ iou,
                                                        const int32_t* __restrict__ status, int n_img, int n_cat,
                                                        int64_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_cat) {
    int64_t a = 0, b = 0, c = 0;
    double s = 0.0;
    for (int m = 0; m < n_img; ++m) {
      const int64_t o = (int64_t)m * n_cat + i;
      a += tp[o]; b += fp[o]; c += fn[o]; s += iou[o];
    }
    out[i] = a; out[n_cat + i] = b; out[2 * n_cat + i] = c;
    out[3 * n_cat + i] = __builtin_bit_cast(int64_t, s);
  }
  if (i < n_img) out[4 * (int64_t)n_cat + i] = status[i];
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int64_t rsp_pq_workspace_bytes(int32_t G) {
  if (G < 0 || G > PQ_MAXP) return -1;
  return (ws_base_of(G) + PQ_WORDS) * 4;
}

extern "C" int rsp_pq_image(const int32_t* pred, const uint8_t* gt_rgb, const int32_t* gt_map, int32_t H, int32_t W,
                            int32_t num_classes, int32_t ignore_index, const int32_t* tables, int32_t G, int32_t n_cat,
                            void* workspace, int32_t* tp, int32_t* fp, int32_t* fn, double* iou_sum, int32_t* status,
                            int32_t* n_pred, int32_t* pred_ids, int32_t* pred_cat, int32_t* pred_area, rsp_stream_t stream) {
  if (!pred || (gt_rgb != nullptr) == (gt_map != nullptr) || !tables || !workspace || !tp || !fp || !fn || !iou_sum ||
      !status || !n_pred || !pred_ids || !pred_cat || !pred_area || H < 1 || W < 1 || (int64_t)H * W >= (1LL << 31) ||
      G < 0 || G > PQ_MAXP || n_cat < 1 || n_cat > RSP_PQ_MAX_CATEGORIES || num_classes < 0 || !aligned16(pred) ||
      !aligned16(gt_rgb) || !aligned16(gt_map) || !aligned16(workspace) || ((uintptr_t)iou_sum & 7))
    return RSP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  int32_t* ws = (int32_t*)workspace;
  int32_t* word_base = ws + ws_base_of(G);
  const int64_t N = (int64_t)H * W;
  if (hipMemsetAsync(ws, 0, (size_t)ws_base_of(G) * 4, s) != hipSuccess) return RSP_ELAUNCH;
  const unsigned grid = (unsigned)((N + 256 * PQ_STRIP - 1) / (256 * PQ_STRIP));
  const PqTables t = pq_tables(tables, G);
  hipLaunchKernelGGL(pq_present_kernel, dim3(grid), dim3(256), 0, s, pred, N, num_classes, ignore_index, ws);
  hipLaunchKernelGGL(pq_rank_kernel, dim3(1), dim3(1024), 0, s, ws, word_base, pred_ids);
  if (gt_rgb)
    hipLaunchKernelGGL(pq_confusion_kernel<true>, dim3(grid), dim3(256), 0, s, pred, (const void*)gt_rgb, N, num_classes,
                       ignore_index, t.gt_id, G, ws, (const int32_t*)word_base);
  else
    hipLaunchKernelGGL(pq_confusion_kernel<false>, dim3(grid), dim3(256), 0, s, pred, (const void*)gt_map, N, num_classes,
                       ignore_index, t.gt_id, G, ws, (const int32_t*)word_base);
  hipLaunchKernelGGL(pq_match_kernel, dim3(1), dim3(256), 0, s, (const int32_t*)ws, t, G, n_cat, tp, fp, fn, iou_sum, status,
                     n_pred, pred_ids, pred_cat, pred_area);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_pq_reduce(const int32_t* tp, const int32_t* fp, const int32_t* fn, const double* iou_sum,
                             const int32_t* status, int32_t n_img, int32_t n_cat, int64_t* out, rsp_stream_t stream) {
  if (!tp || !fp || !fn || !iou_sum || !status || !out || n_img < 1 || n_cat < 1 || n_cat > RSP_PQ_MAX_CATEGORIES ||
      ((uintptr_t)iou_sum & 7) || ((uintptr_t)out & 7))
    return RSP_EINVAL;
  const int n = n_img > n_cat ? n_img : n_cat;
  hipLaunchKernelGGL(pq_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tp, fp, fn,
                     iou_sum, status, n_img, n_cat, out);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
