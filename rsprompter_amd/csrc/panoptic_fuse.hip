// Panoptic fusion: MaskFormerFusionHead.panoptic_postprocess (maskformer_fusion_head.py:41-106) behind the panoptic_on branch
// of the fusion heads (models.py:698-701, maskformer_fusion_head.py:253-256) as four launches, nothing read by the host:
//   select    softmax-max per query, label != nc && score > object_mask_thr, ordered compaction        (:62-68)
//   fuse      per output pixel argmax_k score_k * sigmoid(field_k), the areas as integer counts        (:70, :81, :86-88)
//   decide    the area-ratio test in double, instance ids by an ordered prefix, kept index -> id       (:82-104)
//   remap     map[i] = lut[map[i]]                                                                    (:100-103)
// The reference writes [Nq, H, W] fp32 three times (logits, sigmoid, scores * sigmoid); here the fields are evaluated per
// pixel from the low-resolution logits by mask_field.h, the same functions the instance branch thresholds.  Integer atomics
// only: the result is the same bits on every run.
#include "rsp_common.h"
#include "mask_field.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int PAN_MAX = RSP_PANOPTIC_MAX_QUERIES;     // kept queries <= queries <= the bins of the LDS histograms
// rows of a strip group.  Chosen by counting, not by measurement (4 was never timed against it): at 256 -> 1024 the source-row
// pair changes at rows 2, 6, 10, ..., so rows 2t and 2t + 1 always share one -- a mask costs one horizontal interpolation per
// group, as it would with 4 rows (two pairs per group) -- while 2 rows hold half the running-best registers and give twice the
// work items of 4.
constexpr int PAN_ROWS = 2;

// workspace (int32 words): count | kept query [PAN_MAX] | label [PAN_MAX] | score bits [PAN_MAX] | mask_area [PAN_MAX] |
// original_area [PAN_MAX] | lut [2 * PAN_MAX] (second half: a winner that filter_low_score leaves unpainted)
constexpr int WS_COUNT = 0, WS_KEPT = 4, WS_LABEL = WS_KEPT + PAN_MAX, WS_SCORE = WS_LABEL + PAN_MAX,
              WS_MAREA = WS_SCORE + PAN_MAX, WS_OAREA = WS_MAREA + PAN_MAX, WS_LUT = WS_OAREA + PAN_MAX,
              WS_WORDS = WS_LUT + 2 * PAN_MAX;

// ------------------------------------------------------------------------------------------------------------ select
// one block; query q = round * 256 + thread, so the block scan of the keep flags compacts in query order.  Also the
// per-query outputs of the queries that are not kept, and the zeroes of the counters.
__global__ __launch_bounds__(256) void panoptic_select_kernel(const float* __restrict__ cls, int Nq, int nc, float thr,
                                                              int32_t* __restrict__ ws, float* __restrict__ score_out,
                                                              int32_t* __restrict__ segment, int32_t* __restrict__ mask_area,
                                                              int32_t* __restrict__ original_area) {
  __shared__ int s_tmp[4];
  for (int i = threadIdx.x; i < 2 * PAN_MAX; i += 256) ws[WS_MAREA + i] = 0;      // mask_area and original_area
  int kept = 0;
  for (int q0 = 0; q0 < Nq; q0 += 256) {
    const int q = q0 + threadIdx.x;
    const float* row = cls + (int64_t)min(q, Nq - 1) * (nc + 1);
    float m = row[0];
    for (int j = 1; j <= nc; ++j) m = fmaxf(m, row[j]);
    float s = 0.f;
    for (int j = 0; j <= nc; ++j) s += expf(row[j] - m);
    float best = -1.f;
    int label = 0;
    for (int j = 0; j <= nc; ++j) {                       // .max(-1): the lowest class index on a tie
      const float pj = expf(row[j] - m) / s;
      if (pj > best) { best = pj; label = j; }
    }
    const int keep = (q < Nq) & (label != nc) & (best > thr);
    int total;
    const int pos = kept + rsp_block_excl_scan<256>(keep, s_tmp, &total);
    if (keep) {
      ws[WS_KEPT + pos] = q;
      ws[WS_LABEL + pos] = label;
      ws[WS_SCORE + pos] = __float_as_int(best);
    }
    if (q < Nq) { score_out[q] = best; segment[q] = -1; mask_area[q] = 0; original_area[q] = 0; }
    kept += total;
  }
  if (threadIdx.x == 0) ws[WS_COUNT] = kept;
}

// -------------------------------------------------------------------------------------------------------------- fuse
struct PanP {
  const float* low;        // [Nq, h, w]
  int32_t* ws;
  int32_t* map;            // [oh, ow]: the winner's kept index, + PAN_MAX where `filter` leaves the pixel unpainted
  int filter;
  MaskGeom g;
};

template <MaskForm FORM, bool QUAD>
__global__ __launch_bounds__(256) void panoptic_fuse_kernel(const PanP p) {
  typedef MaskGroup<FORM, QUAD, PAN_ROWS> G;
  constexpr int NP = G::R * G::C;
  __shared__ int s_win[PAN_MAX], s_org[PAN_MAX];
  const int n = p.ws[WS_COUNT];                            // uniform: a scalar load and loop bound
  const int32_t* kept = p.ws + WS_KEPT;
  const float* score = reinterpret_cast<const float*>(p.ws + WS_SCORE);
  for (int i = threadIdx.x; i < n; i += MASK_BLOCK) { s_win[i] = 0; s_org[i] = 0; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  float best[NP];
  int bidx[NP];
  unsigned bpos = 0;                                       // bit i: the winner's sigmoid >= 0.5
#pragma unroll
  for (int i = 0; i < NP; ++i) { best[i] = -1.f; bidx[i] = 0; }
  mask_each_group_of_list<FORM, QUAD, PAN_ROWS>(p.low, kept, n, p.g,
    [&](int j, const float* v, unsigned live) {
      const float sj = score[j];
      int org = 0;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        // sigmoid through v_exp_f32 / v_rcp_f32, as query_mask_kernel's (1-2 ulp each)
        const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v[i] * -1.4426950408889634f));
        const bool pos = sg >= 0.5f;
        const float pr = sj * sg;
        const bool win = pr > best[i];                     // strict: the lowest kept index on an exact tie
        best[i] = win ? pr : best[i];
        bidx[i] = win ? j : bidx[i];
        bpos = win ? ((bpos & ~(1u << i)) | ((pos ? 1u : 0u) << i)) : bpos;
        org += __popcll(__ballot(pos && ((live >> (i / G::C)) & 1u)));
      }
      if (lane == 0 && org) atomicAdd(&s_org[j], org);     // original_area: one LDS add per wave and mask
    },
    [&](int oy0, int ox, unsigned live) {
      int o[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const bool on = (live >> (i / G::C)) & 1u;
        if (on && n > 0) atomicAdd(&s_win[bidx[i]], 1);    // mask_area: before the filter, as the reference counts it
        o[i] = bidx[i] + ((p.filter && !((bpos >> i) & 1u)) ? PAN_MAX : 0);
        best[i] = -1.f; bidx[i] = 0;
      }
      bpos = 0;
#pragma unroll
      for (int r = 0; r < G::R; ++r) {
        if (!((live >> r) & 1u)) continue;
        int32_t* dst = p.map + (int64_t)(oy0 + r) * p.g.ow + ox;
        if (G::C == 4) *reinterpret_cast<i32x4*>(dst) = i32x4{o[r * G::C], o[r * G::C + 1], o[r * G::C + 2], o[r * G::C + 3]};
        else dst[0] = o[r * G::C];
      }
    });
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += MASK_BLOCK) {      // one global integer atomic per non-empty bin and block
    const int a = s_win[i], b = s_org[i];
    if (a) atomicAdd(&p.ws[WS_MAREA + i], a);
    if (b) atomicAdd(&p.ws[WS_OAREA + i], b);
  }
}

// ------------------------------------------------------------------------------------------------------------ decide
// one block: kept index k = round * 256 + thread, so the block scan of "a painted thing" numbers the instances in kept order
__global__ __launch_bounds__(256) void panoptic_decide_kernel(int32_t* __restrict__ ws, int nc, int num_things, double iou_thr,
                                                              int32_t* __restrict__ segment, int32_t* __restrict__ mask_area,
                                                              int32_t* __restrict__ original_area) {
  __shared__ int s_tmp[4];
  const int n = ws[WS_COUNT];
  for (int i = threadIdx.x; i < 2 * PAN_MAX; i += 256) ws[WS_LUT + i] = nc;
  __syncthreads();
  int things = 0;
  for (int k0 = 0; k0 < n; k0 += 256) {
    const int k = k0 + threadIdx.x;
    const int kk = min(k, n - 1);
    const int ma = ws[WS_MAREA + kk], oa = ws[WS_OAREA + kk], label = ws[WS_LABEL + kk];
    // maskformer_fusion_head.py:93-95: Python's float division, `<` against the double iou_thr
    const int painted = (k < n) & (ma > 0) & (oa > 0) & !((double)ma / (double)(oa > 0 ? oa : 1) < iou_thr);
    const int thing = painted & (label < num_things);
    int total;
    const int id = things + rsp_block_excl_scan<256>(thing, s_tmp, &total) + 1;     // instance_id starts at 1
    if (k < n) {
      const int seg = label + (thing ? id * 1000 : 0);                              // INSTANCE_OFFSET, panoptic_utils.py:18
      const int q = ws[WS_KEPT + k];
      if (painted) ws[WS_LUT + k] = seg;
      segment[q] = painted ? seg : -1;
      mask_area[q] = ma;
      original_area[q] = oa;
    }
    things += total;
  }
}

// ------------------------------------------------------------------------------------------------------------- remap
__global__ __launch_bounds__(256) void panoptic_remap_kernel(int32_t* __restrict__ map, const int32_t* __restrict__ lut, int64_t total) {
  const int64_t n4 = total >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    i32x4 v = *reinterpret_cast<const i32x4*>(map + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = lut[v[e]];
    *reinterpret_cast<i32x4*>(map + i * 4) = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(total & 3)) {
    const int64_t i = (n4 << 2) + threadIdx.x;
    map[i] = lut[map[i]];
  }
}

template <MaskForm FORM, bool QUAD>
void launch_fuse(const PanP& p, hipStream_t s) {
  int64_t gx = (MaskGroup<FORM, QUAD, PAN_ROWS>::items(p.g.oh, p.g.ow) + MASK_BLOCK - 1) / MASK_BLOCK;
  if (gx > 2048) gx = 2048;                                // the grid depends on the pixel count alone
  hipLaunchKernelGGL((panoptic_fuse_kernel<FORM, QUAD>), dim3((unsigned)gx), dim3(MASK_BLOCK), 0, s, p);
}

}  // namespace

extern "C" int64_t rsp_panoptic_workspace_bytes(void) { return (int64_t)WS_WORDS * 4; }

extern "C" int rsp_panoptic_fuse(const float* cls, const float* low_res, int32_t Nq, int32_t nc, int32_t num_things,
                                 int32_t h, int32_t w, int32_t Hb, int32_t Wb, int32_t crop_h, int32_t crop_w, int32_t out_h,
                                 int32_t out_w, float object_mask_thr, double iou_thr, int32_t filter_low_score,
                                 void* workspace, int32_t* sem_seg, int32_t* segment, int32_t* mask_area,
                                 int32_t* original_area, float* score, rsp_stream_t stream) {
  const MaskGeom g{h, w, Hb, Wb, crop_h, crop_w, out_h, out_w};
  if (!cls || !low_res || !workspace || !sem_seg || !segment || !mask_area || !original_area || !score || Nq <= 0 ||
      Nq > PAN_MAX || nc <= 0 || num_things < 0 || num_things > nc || !mask_geom_valid(g))
    return RSP_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  int32_t* ws = (int32_t*)workspace;
  hipLaunchKernelGGL(panoptic_select_kernel, dim3(1), dim3(256), 0, s, cls, Nq, nc, object_mask_thr, ws, score, segment,
                     mask_area, original_area);
  const PanP p{low_res, ws, sem_seg, filter_low_score ? 1 : 0, g};
  switch (mask_form(g)) {
    case MASK_STRIP: launch_fuse<MASK_STRIP, true>(p, s); break;
    case MASK_IDENT: launch_fuse<MASK_IDENT, false>(p, s); break;
    default:
      if ((out_w & 3) == 0) launch_fuse<MASK_GENERIC, true>(p, s);
      else launch_fuse<MASK_GENERIC, false>(p, s);
  }
  hipLaunchKernelGGL(panoptic_decide_kernel, dim3(1), dim3(256), 0, s, ws, nc, num_things, iou_thr, segment, mask_area,
                     original_area);
  const int64_t total = (int64_t)out_h * out_w;
  int64_t gr = ((total >> 2) + 255) / 256;
  gr = gr > 2048 ? 2048 : (gr < 1 ? 1 : gr);
  hipLaunchKernelGGL(panoptic_remap_kernel, dim3((unsigned)gr), dim3(256), 0, s, sem_seg, ws + WS_LUT, total);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
