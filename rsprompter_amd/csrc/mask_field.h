// The mask field: the value per output pixel of the resize -> crop -> resize chain over [h, w] low-resolution logits
// (models.py:1746-1784), and the traversals of it.  Every kernel that thresholds, scores or locates on that field
// (samdec.hip, query.hip) takes its values and its loops from here, and every launcher its choice of form, so "the scores are
// those of the masks" is a property of the code.  Include it after rsp_common.h (it does not include it itself: the emulated
// build rewrites that include per source file).
#pragma once

struct Lin { int i0, i1; float l0, l1; };
// torch upsample_bilinear2d(align_corners=False) source index / weights: the one definition for every such resize in csrc
__device__ __forceinline__ Lin lin_coef(int dst, float scale, int in_size) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  Lin c;
  c.i0 = (int)src;
  if (c.i0 > in_size - 1) c.i0 = in_size - 1;
  c.i1 = c.i0 + (c.i0 < in_size - 1 ? 1 : 0);
  c.l1 = src - (float)c.i0;
  c.l0 = 1.0f - c.l1;
  return c;
}

// [h, w] logits -> bilinear to [Hb, Wb] -> the top-left [ch, cw] of that -> bilinear to [oh, ow]
struct MaskGeom { int h, w, Hb, Wb, ch, cw, oh, ow; };

// MASK_IDENT: crop == output size, so the second interpolation is the identity (src index == dst index, weight 1) and only
// stage 1 is evaluated.  MASK_STRIP: that, with rows of whole 4-pixel quads (mask_each_strip).
enum MaskForm { MASK_STRIP, MASK_IDENT, MASK_GENERIC };
__host__ __device__ inline MaskForm mask_form(const MaskGeom& g) {
  if (g.ch != g.oh || g.cw != g.ow) return MASK_GENERIC;
  return (g.ow & 3) == 0 ? MASK_STRIP : MASK_IDENT;
}

// What a row of rsp_mask_score_box_crops' device table has to satisfy (its h and w are the call's); a row that does not
// scores as an empty mask.
__host__ __device__ inline bool mask_table_row_ok(const MaskGeom& g) {
  return g.Hb > 0 && g.Wb > 0 && g.ch > 0 && g.cw > 0 && g.oh > 0 && g.ow > 0 && g.ch <= g.Hb && g.cw <= g.Wb;
}
// The geometry arguments of a C entry point; the pixel count fits the int indices of the traversals.
inline bool mask_geom_valid(const MaskGeom& g) {
  return g.h > 0 && g.w > 0 && mask_table_row_ok(g) && (int64_t)g.oh * g.ow <= 0x7fffffffLL;
}

// work items (threads) of the strip form: (tile of `rows` rows) x (column quad)
__host__ __device__ inline int64_t mask_strip_items(int oh, int ow, int rows) {
  return (int64_t)((oh + rows - 1) / rows) * (ow >> 2);
}

// launch(m0, km) for chunks of at most 65535 masks (the grid.y limit): every launcher with a mask per blockIdx.y goes through it
template <typename F>
inline void for_mask_chunks(int32_t k, F&& launch) {
  for (int32_t m0 = 0; m0 < k; m0 += 65535) launch(m0, k - m0 < 65535 ? k - m0 : 65535);
}

struct MaskScales { float s1h, s1w, s2h, s2w; };
__device__ __forceinline__ MaskScales mask_scales(const MaskGeom& g) {
  return MaskScales{(float)g.h / (float)g.Hb, (float)g.w / (float)g.Wb, (float)g.ch / (float)g.oh, (float)g.cw / (float)g.ow};
}
__device__ __forceinline__ float mask_stage1(const float* __restrict__ low, const MaskGeom& g, const MaskScales& s, int Y, int X) {
  const Lin ay = lin_coef(Y, s.s1h, g.h);
  const Lin ax = lin_coef(X, s.s1w, g.w);
  const float v00 = low[ay.i0 * g.w + ax.i0], v01 = low[ay.i0 * g.w + ax.i1];
  const float v10 = low[ay.i1 * g.w + ax.i0], v11 = low[ay.i1 * g.w + ax.i1];
  return ay.l0 * (ax.l0 * v00 + ax.l1 * v01) + ay.l1 * (ax.l0 * v10 + ax.l1 * v11);
}
template <bool IDENT>
__device__ __forceinline__ float mask_pixel(const float* __restrict__ low, const MaskGeom& g, const MaskScales& s, int oy, int ox) {
  if (IDENT) return mask_stage1(low, g, s, oy, ox);
  const Lin cy = lin_coef(oy, s.s2h, g.ch), cx = lin_coef(ox, s.s2w, g.cw);
  const float a00 = mask_stage1(low, g, s, cy.i0, cx.i0), a01 = mask_stage1(low, g, s, cy.i0, cx.i1);
  const float a10 = mask_stage1(low, g, s, cy.i1, cx.i0), a11 = mask_stage1(low, g, s, cy.i1, cx.i1);
  return cy.l0 * (cx.l0 * a00 + cx.l1 * a01) + cy.l1 * (cx.l0 * a10 + cx.l1 * a11);
}

// MASK_STRIP: a thread owns 4 consecutive output columns and walks down the rows.  The x coefficients are computed once, the
// two horizontally interpolated source rows only when the source row pair changes (every 4th output row at the usual
// 256 -> 1024), and a pixel is ay.l0 * h0 + ay.l1 * h1 -- the fp32 expression tree of mask_stage1(): the same bits.
struct MaskStrip {
  Lin ax[4];
  int r0, r1;
  float h0[4], h1[4];
  __device__ __forceinline__ void init(const MaskGeom& g, const MaskScales& s, int ox) {
#pragma unroll
    for (int e = 0; e < 4; ++e) ax[e] = lin_coef(ox + e, s.s1w, g.w);
    r0 = -1; r1 = -1;
  }
  __device__ __forceinline__ void row(const float* __restrict__ low, const MaskGeom& g, const MaskScales& s, int oy, float v[4]) {
    const Lin ay = lin_coef(oy, s.s1h, g.h);
    if (ay.i0 != r0 || ay.i1 != r1) {
      r0 = ay.i0; r1 = ay.i1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h0[e] = ax[e].l0 * low[r0 * g.w + ax[e].i0] + ax[e].l1 * low[r0 * g.w + ax[e].i1];
        h1[e] = ax[e].l0 * low[r1 * g.w + ax[e].i0] + ax[e].l1 * low[r1 * g.w + ax[e].i1];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ay.l0 * h0[e] + ay.l1 * h1[e];
  }
};

// ---- traversals of one mask's field by the blocks blockIdx.x of a grid (`low` = that mask's logits).  Every thread of every
// block returns from them, so a block reduction may follow.
// The kernels that call them are launched with MASK_BLOCK threads (their block reductions are written for 256 as well).  A
// constant, because blockDim.x read in an inlined device function is not folded to the uniform group size the way it is in a
// kernel body: the stride then lives in a vector register (+2 VGPRs in query_mask_kernel<true>, across the 64 line).
constexpr int MASK_BLOCK = 256;

// f(value, oy, ox, i) for every pixel, grid-stride over the flat index i = oy * ow + ox.  `ident` is a template constant of the
// calling kernel (the select folds away) except in mask_score_crops_kernel, where it is a property of the table row and ONE
// loop holds the select.
template <typename F>
__device__ __forceinline__ void mask_each_pixel(const float* __restrict__ low, const MaskGeom& g, bool ident, F&& f) {
  const MaskScales sc = mask_scales(g);
  const int64_t total = (int64_t)g.oh * g.ow;
  for (int64_t i = (int64_t)blockIdx.x * MASK_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * MASK_BLOCK) {
    const int oy = (int)(i / g.ow), ox = (int)(i - (int64_t)oy * g.ow);
    f(ident ? mask_pixel<true>(low, g, sc, oy, ox) : mask_pixel<false>(low, g, sc, oy, ox), oy, ox, i);
  }
}

// f(v[4], oy, ox) for every quad of 4 pixels of one row, (ow & 3) == 0, grid-stride.  The identity form shares the row
// coefficients among the four pixels (mask_stage1's expression tree).
template <bool IDENT, typename F>
__device__ __forceinline__ void mask_each_quad(const float* __restrict__ low, const MaskGeom& g, F&& f) {
  const MaskScales sc = mask_scales(g);
  const int qw = g.ow >> 2;
  const int nq = g.oh * qw;
  for (int i = blockIdx.x * MASK_BLOCK + threadIdx.x; i < nq; i += gridDim.x * MASK_BLOCK) {
    const int oy = i / qw, ox = (i - oy * qw) << 2;
    float v[4];
    if (IDENT) {
      const Lin ay = lin_coef(oy, sc.s1h, g.h);
      const float* r0 = low + ay.i0 * g.w;
      const float* r1 = low + ay.i1 * g.w;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const Lin ax = lin_coef(ox + e, sc.s1w, g.w);
        v[e] = ay.l0 * (ax.l0 * r0[ax.i0] + ax.l1 * r0[ax.i1]) + ay.l1 * (ax.l0 * r1[ax.i0] + ax.l1 * r1[ax.i1]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = mask_pixel<false>(low, g, sc, oy, ox + e);
    }
    f(v, oy, ox);
  }
}

// f(v[4], oy, ox) for every quad, MASK_STRIP geometries only: a work item is ROWS rows of one column quad (quads fastest:
// coalesced rows), grid-stride over mask_strip_items(oh, ow, ROWS).  ONCE: the grid holds a thread per item, the loop is an if.
template <int ROWS, bool ONCE, typename F>
__device__ __forceinline__ void mask_each_strip(const float* __restrict__ low, const MaskGeom& g, F&& f) {
  const MaskScales sc = mask_scales(g);
  const int qw = g.ow >> 2;
  const int nitem = (int)mask_strip_items(g.oh, g.ow, ROWS);
  for (int i = blockIdx.x * MASK_BLOCK + threadIdx.x; i < nitem; i += gridDim.x * MASK_BLOCK) {
    const int ty = i / qw, ox = (i - ty * qw) << 2;
    MaskStrip st;
    st.init(g, sc, ox);
    const int oy_end = min((ty + 1) * ROWS, g.oh);
    for (int oy = ty * ROWS; oy < oy_end; ++oy) {
      float v[4];
      st.row(low, g, sc, oy, v);
      f(v, oy, ox);
    }
    if (ONCE) break;
  }
}

// ---- every pixel x every listed mask (panoptic_fuse.hip): the traversal of the fields of `n` masks of one [*, h, w] logit
// tensor, mask j = plane list[j], by the blocks blockIdx.x of a grid.  A work item is a GROUP of R x C pixels, and a thread
// sees all n fields of its group before it moves on:
//   MASK_STRIP               R = ROWS rows of one column quad (C = 4) through MaskStrip -- the x coefficients once per group,
//                            the source-row pair once per mask and change of pair;
//   MASK_GENERIC, QUAD       one row of a quad (R = 1, C = 4) through mask_pixel<false>, (ow & 3) == 0;
//   MASK_IDENT / MASK_GENERIC, !QUAD   one pixel through mask_pixel<IDENT>.
// Per group: f(j, v[R * C], live) for j = 0 .. n - 1 in list order (v[r * C + e] = the field of mask j at row oy0 + r, column
// ox + e), then done(oy0, ox, live).  Bit r of `live` says that row r of the group exists.  EVERY lane of a block takes every
// step: a lane past the last group evaluates the last group with live == 0, and a row past the last row evaluates the last row
// with its bit clear, so that f may hold wave ballots and done a block barrier.  The values are those of mask_stage1 /
// mask_pixel, as in the traversals of one mask above.
template <MaskForm FORM, bool QUAD, int ROWS>
struct MaskGroup {
  static constexpr int R = FORM == MASK_STRIP ? ROWS : 1;
  static constexpr int C = (FORM == MASK_STRIP || QUAD) ? 4 : 1;
  static_assert(FORM != MASK_IDENT || !QUAD, "an identity geometry of whole quads is a MASK_STRIP one");
  static __host__ __device__ inline int64_t items(int oh, int ow) { return (int64_t)((oh + R - 1) / R) * (C == 4 ? ow >> 2 : ow); }
};

template <MaskForm FORM, bool QUAD, int ROWS, typename F, typename D>
__device__ __forceinline__ void mask_each_group_of_list(const float* __restrict__ low_all, const int32_t* __restrict__ list,
                                                        int n, const MaskGeom& g, F&& f, D&& done) {
  typedef MaskGroup<FORM, QUAD, ROWS> G;
  constexpr int R = G::R, C = G::C;
  const MaskScales sc = mask_scales(g);
  const int per_row = C == 4 ? g.ow >> 2 : g.ow;
  const int64_t nitem = G::items(g.oh, g.ow);
  const int64_t plane = (int64_t)g.h * g.w;
  for (int64_t base = (int64_t)blockIdx.x * MASK_BLOCK; base < nitem; base += (int64_t)gridDim.x * MASK_BLOCK) {
    const int64_t i = base + threadIdx.x;
    const int64_t ii = i < nitem ? i : nitem - 1;
    const int ty = (int)(ii / per_row), ox = (int)(ii - (int64_t)ty * per_row) * C;
    const int oy0 = ty * R;
    unsigned live = 0;
    int oy[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      live |= (i < nitem && oy0 + r < g.oh ? 1u : 0u) << r;
      oy[r] = min(oy0 + r, g.oh - 1);
    }
    MaskStrip st;
    if (FORM == MASK_STRIP) st.init(g, sc, ox);
    for (int j = 0; j < n; ++j) {
      const float* low = low_all + (int64_t)list[j] * plane;
      float v[R * C];
      if (FORM == MASK_STRIP) {
        st.r0 = -1; st.r1 = -1;          // the cached rows are another mask's
#pragma unroll
        for (int r = 0; r < R; ++r) st.row(low, g, sc, oy[r], v + r * C);
      } else {
#pragma unroll
        for (int e = 0; e < C; ++e) v[e] = mask_pixel<FORM == MASK_IDENT>(low, g, sc, oy[0], ox + e);
      }
      f(j, v, live);
    }
    done(oy0, ox, live);
  }
}
