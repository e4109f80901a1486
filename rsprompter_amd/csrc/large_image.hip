// Sliced inference on large scenes: what the reference does on the host per patch and per instance
// (demo/large_image_demo.py:133-170 over sahi.slicing.slice_image / shift_bboxes / shift_masks and
// mmdet/utils/large_image.py:27-104) as three bandwidth / latency kernels.
//   rsp_slice_resize_pad : B tiles of the device-resident scene -> the model's input batch, one launch, no crop copy
//   rsp_crops_resize_pad : the same for B crops of DIFFERENT sizes (the crop layers of SAM's mask generation):
//                          boxes and resized sizes come from a device table
//   rsp_rle_shift        : COCO run counts of tile-sized masks -> run counts of the same masks placed in the scene,
//                          in the run domain (the scene-sized dense mask of sahi's shift_masks never exists)
//   rsp_paste_tiles      : the dense form of shift_masks, for callers who ask for dense scene masks
#include "rsp_common.h"
#include "run_table.h"

namespace {

// ------------------------------------------------------------------------------------------------- tile front end
struct SliceP {
  const void* scene;
  const int32_t* origins;   // device [B, 2] = (x0, y0)
  float* dst;               // [B, 3, Hp, Wp]
  int SH, SW, th, tw, Hn, Wn, Hp, Wp, normalise, swap_rb;
  float p[3], m[3], s[3];
};

__device__ __forceinline__ void slice_origin(const SliceP& P, int b, int& x0, int& y0) {
  // clamped: a tile never reads outside the scene, whatever the origin array holds
  x0 = min(max(P.origins[2 * b], 0), P.SW - P.tw);
  y0 = min(max(P.origins[2 * b + 1], 0), P.SH - P.th);
}

__device__ __forceinline__ void slice_normalise(const SliceP& P, float v[3]) {
  if (P.normalise) {
    const float a = P.swap_rb ? v[2] : v[0], b = v[1], c2 = P.swap_rb ? v[0] : v[2];
    v[0] = (a - P.m[0]) / P.s[0]; v[1] = (b - P.m[1]) / P.s[1]; v[2] = (c2 - P.m[2]) / P.s[2];
  }
}

// general form: resize_pad_kernel's loop over the padded canvas with blockIdx.y = tile; the source window starts at the
// tile's origin and keeps the scene's row pitch
template <typename T>
__global__ __launch_bounds__(256) void slice_resize_pad_kernel(const SliceP P) {
  const int b = blockIdx.y;
  int ox, oy;
  slice_origin(P, b, ox, oy);
  const T* src = static_cast<const T*>(P.scene) + ((int64_t)oy * P.SW + ox) * 3;
  const double sx_scale = (double)P.tw / (double)P.Wn, sy_scale = (double)P.th / (double)P.Hn;
  const int64_t total = (int64_t)P.Hp * P.Wp;
  float* dst = P.dst + (int64_t)b * 3 * total;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % P.Wp), y = (int)(i / P.Wp);
    float v[3] = {P.p[0], P.p[1], P.p[2]};
    if (y < P.Hn && x < P.Wn) rsp_bilinear_px(src, (int64_t)P.SW * 3, P.th, P.tw, sx_scale, sy_scale, x, y, v);
    slice_normalise(P, v);
    dst[i] = v[0];
    dst[total + i] = v[1];
    dst[2 * total + i] = v[2];
  }
}

// tile size == resized size, uint8 scene: the interpolation weights are exactly (1, 0), so the resized pixel IS the source
// byte (v * 1 + w * 0 + ... is exact for the 256 byte values) and the kernel is convert + de-interleave + pad.  One lane
// owns 16 consecutive pixels of a row: 48 source bytes -- three 16-byte loads when the address allows, byte loads
// otherwise -- and four 16-byte stores into each of the three planes (Wp % 4 == 0: every group start is 16-byte aligned).
__global__ __launch_bounds__(256) void slice_convert_pad_kernel(const SliceP P) {
  const int b = blockIdx.y;
  int ox, oy;
  slice_origin(P, b, ox, oy);
  const uint8_t* src = static_cast<const uint8_t*>(P.scene) + ((int64_t)oy * P.SW + ox) * 3;
  const int gpr = (P.Wp + 15) >> 4;                   // groups per row
  const int64_t ngroups = (int64_t)P.Hp * gpr, total = (int64_t)P.Hp * P.Wp;
  float* dst = P.dst + (int64_t)b * 3 * total;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(g / gpr), x = (int)(g % gpr) << 4;
    const int64_t o = (int64_t)y * P.Wp + x;
    if (y < P.Hn && x + 16 <= P.Wn) {
      const uint8_t* sp = src + (int64_t)y * P.SW * 3 + x * 3;
      union { uint4 q[3]; uint8_t c[48]; } u;
      if ((reinterpret_cast<uintptr_t>(sp) & 15) == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) u.q[j] = reinterpret_cast<const uint4*>(sp)[j];
      } else {
#pragma unroll
        for (int j = 0; j < 48; ++j) u.c[j] = sp[j];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 o0, o1, o2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int px = (4 * q + e) * 3;
          float v[3] = {(float)u.c[px], (float)u.c[px + 1], (float)u.c[px + 2]};
          slice_normalise(P, v);
          o0[e] = v[0]; o1[e] = v[1]; o2[e] = v[2];
        }
        *reinterpret_cast<f32x4*>(dst + o + 4 * q) = o0;
        *reinterpret_cast<f32x4*>(dst + total + o + 4 * q) = o1;
        *reinterpret_cast<f32x4*>(dst + 2 * total + o + 4 * q) = o2;
      }
    } else {                                          // padding, the row's tail, the group that straddles Wn
      const int xe = min(x + 16, P.Wp);
      for (int xx = x; xx < xe; ++xx) {
        float v[3] = {P.p[0], P.p[1], P.p[2]};
        if (y < P.Hn && xx < P.Wn) {
          const uint8_t* sp = src + (int64_t)y * P.SW * 3 + xx * 3;
          v[0] = (float)sp[0]; v[1] = (float)sp[1]; v[2] = (float)sp[2];
        }
        slice_normalise(P, v);
        const int64_t oo = (int64_t)y * P.Wp + xx;
        dst[oo] = v[0];
        dst[total + oo] = v[1];
        dst[2 * total + oo] = v[2];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- crop front end
// B crops of different sizes (SAM's crop layers: the sizes differ between layers, and the last crop of every row and
// column is clamped to the image), each resized to its own (Hn, Wn) and padded to (Hp, Wp).  Row b of the table is
// (x0, y0, x1, y1, Hn, Wn); the kernel clamps it so that a crop never reads outside the image or writes outside its canvas.
struct CropsP {
  const void* image;
  const int32_t* table;     // device [B, 6]
  float* dst;               // [B, 3, Hp, Wp]
  int SH, SW, Hp, Wp, normalise, swap_rb;
  float p[3], m[3], s[3];
};

template <typename T>
__global__ __launch_bounds__(256) void crops_resize_pad_kernel(const CropsP P) {
  const int b = blockIdx.y;
  const int32_t* t = P.table + 6 * b;
  const int x0 = min(max(t[0], 0), P.SW - 1), y0 = min(max(t[1], 0), P.SH - 1);
  const int tw = min(max(t[2], x0 + 1), P.SW) - x0, th = min(max(t[3], y0 + 1), P.SH) - y0;
  const int Hn = min(max(t[4], 1), P.Hp), Wn = min(max(t[5], 1), P.Wp);
  const T* src = static_cast<const T*>(P.image) + ((int64_t)y0 * P.SW + x0) * 3;
  const double sx_scale = (double)tw / (double)Wn, sy_scale = (double)th / (double)Hn;
  const int64_t total = (int64_t)P.Hp * P.Wp;
  float* dst = P.dst + (int64_t)b * 3 * total;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % P.Wp), y = (int)(i / P.Wp);
    float v[3] = {P.p[0], P.p[1], P.p[2]};
    if (y < Hn && x < Wn) rsp_bilinear_px(src, (int64_t)P.SW * 3, th, tw, sx_scale, sy_scale, x, y, v);
    if (P.normalise) {
      const float a = P.swap_rb ? v[2] : v[0], c1 = v[1], c2 = P.swap_rb ? v[0] : v[2];
      v[0] = (a - P.m[0]) / P.s[0]; v[1] = (c1 - P.m[1]) / P.s[1]; v[2] = (c2 - P.m[2]) / P.s[2];
    }
    dst[i] = v[0];
    dst[total + i] = v[1];
    dst[2 * total + i] = v[2];
  }
}

// ------------------------------------------------------------------------------------------------- run-domain shift
constexpr int SHIFT_THREADS = 256;

// One block per instance.  The tile's column-major stream has pixel p at column p / h, row p % h; in the scene that pixel
// sits at stream position P(p) = (ox + p / h) * H + oy + p % h.  Runs of ONES are what survives the placement: a ones-run
// [s, e) that touches columns xa .. xb becomes xb - xa + 1 ones-runs when H > h (H - h zeros separate the columns) and
// stays one run when H == h; no two output ones-runs touch, so every zero run of the output is simply the gap between
// the end of one output ones-run and the start of the next -- the seams need no merging pass.  Per chunk of 256 input
// runs: scan of the counts (pixel starts), scan of the pieces each ones-run emits (output slots), then the pieces of the
// chunk are dealt out to the threads round-robin (a full-tile mask is ONE input run with w pieces), each finding its
// input run by a binary search over the chunk's slot prefix in LDS.
// Input: a tile-frame run table as rsp_mask_rle writes it (run_table.h).  This kernel keeps its own walk over the row and
// its own column arithmetic: on RspRunWalk the compiler lays the piece loop out differently and the kernel measured
// 9 % slower (profiles/run_walk/parent_vs_this.txt).
__global__ __launch_bounds__(SHIFT_THREADS) void rle_shift_kernel(const uint32_t* __restrict__ counts_in,
                                                                  const int32_t* __restrict__ n_in, int cap_in,
                                                                  const int32_t* __restrict__ offsets, int h, int w,
                                                                  int H, int W, uint32_t* __restrict__ counts_out,
                                                                  int32_t* __restrict__ n_out, int cap_out) {
  __shared__ int tmp[SHIFT_THREADS / 64];
  __shared__ int l_slot[SHIFT_THREADS], l_s[SHIFT_THREADS], l_e[SHIFT_THREADS], l_pe[SHIFT_THREADS];
  __shared__ uint32_t s_lastE;
  const int m = blockIdx.x, tid = threadIdx.x;
  const int n = min(n_in[m], cap_in);
  if (n <= 0) {                                       // an instance whose tile runs did not fit: nothing to place
    if (tid == 0) n_out[m] = 0;
    return;
  }
  const uint32_t* cin = counts_in + (int64_t)m * cap_in;
  uint32_t* out = counts_out + (int64_t)m * cap_out;
  const int ox = min(max(offsets[2 * m], 0), W - w), oy = min(max(offsets[2 * m + 1], 0), H - h);
  const bool whole = H == h;                          // columns stay adjacent: runs are not split
  auto place = [&](int p) -> uint32_t { const int x = p / h; return (uint32_t)(ox + x) * (uint32_t)H + (uint32_t)(oy + p - x * h); };
  if (tid == 0) s_lastE = 0u;
  int carry_pos = 0, carry_slot = 0;
  for (int i0 = 0; i0 < n; i0 += SHIFT_THREADS) {
    const int i = i0 + tid;
    const int c = i < n ? (int)cin[i] : 0;
    int chunk_px, chunk_pieces;
    const int s = carry_pos + rsp_block_excl_scan<SHIFT_THREADS>(c, tmp, &chunk_px), e = s + c;
    const bool ones = i < n && (i & 1) && c > 0;
    const int pieces = ones ? (whole ? 1 : (e - 1) / h - s / h + 1) : 0;
    l_slot[tid] = rsp_block_excl_scan<SHIFT_THREADS>(pieces, tmp, &chunk_pieces);
    l_s[tid] = s;
    l_e[tid] = e;
    l_pe[tid] = (ones && i >= 3) ? s - (int)cin[i - 1] : 0;    // pixel end of the previous ones-run (0: there is none)
    __syncthreads();
    for (int q = tid; q < chunk_pieces; q += SHIFT_THREADS) {
      int lo = 0, hi = SHIFT_THREADS - 1;             // last entry whose slot prefix is <= q: the owner of piece q
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (l_slot[mid] <= q) lo = mid; else hi = mid - 1;
      }
      const int t = q - l_slot[lo], rs = l_s[lo], re = l_e[lo], pe = l_pe[lo];
      uint32_t S, E, prevE;
      if (whole) {
        S = place(rs);
        E = place(re - 1) + 1u;
        prevE = pe > 0 ? place(pe - 1) + 1u : 0u;
      } else {
        const int xa = rs / h, xb = (re - 1) / h, x = xa + t;
        const int row0 = t == 0 ? rs - xa * h : 0, row1 = x == xb ? (re - 1) - xb * h : h - 1;
        const uint32_t col = (uint32_t)(ox + x) * (uint32_t)H + (uint32_t)oy;
        S = col + (uint32_t)row0;
        E = col + (uint32_t)row1 + 1u;
        prevE = t > 0 ? col - (uint32_t)H + (uint32_t)h : (pe > 0 ? place(pe - 1) + 1u : 0u);
      }
      const int64_t slot = (int64_t)carry_slot + q;
      if (2 * slot + 1 < cap_out) {
        out[2 * slot] = S - prevE;
        out[2 * slot + 1] = E - S;
      }
      if (q == chunk_pieces - 1) s_lastE = E;
    }
    carry_pos += chunk_px;
    carry_slot += chunk_pieces;
    __syncthreads();
  }
  if (tid == 0) {
    const uint32_t N = (uint32_t)H * (uint32_t)W, lastE = s_lastE;
    const int64_t needed = 2 * (int64_t)carry_slot + (lastE < N ? 1 : 0);
    if (needed > cap_out) {
      n_out[m] = (int32_t)-needed;                    // caller retries with a larger capacity
    } else {
      if (lastE < N) out[2 * (int64_t)carry_slot] = N - lastE;
      n_out[m] = (int32_t)needed;
    }
  }
}

// ------------------------------------------------------------------------------------------------- dense paste
// out[i, oy + y, ox + x] = masks[i, y, x], zero elsewhere; V output bytes per lane (V = 16 when W % 16 == 0)
template <int V>
__global__ __launch_bounds__(256) void paste_tiles_kernel(const uint8_t* __restrict__ masks,
                                                          const int32_t* __restrict__ offsets, int h, int w, int H,
                                                          int W, uint8_t* __restrict__ out) {
  const int m = blockIdx.y;
  const int ox = min(max(offsets[2 * m], 0), W - w), oy = min(max(offsets[2 * m + 1], 0), H - h);
  const uint8_t* mk = masks + (int64_t)m * h * w;
  uint8_t* o = out + (int64_t)m * H * W;
  const int gpr = W / V;
  const int64_t ngroups = (int64_t)H * gpr;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(g / gpr), x = (int)(g % gpr) * V;
    const int ty = y - oy;
    union { uint8_t c[V]; uint32_t d[V >= 4 ? V / 4 : 1]; } u;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int tx = x + j - ox;
      u.c[j] = (ty >= 0 && ty < h && tx >= 0 && tx < w) ? (uint8_t)(mk[(int64_t)ty * w + tx] != 0) : (uint8_t)0;
    }
    uint8_t* dp = o + (int64_t)y * W + x;
    if (V == 16) *reinterpret_cast<uint4*>(dp) = make_uint4(u.d[0], u.d[1], u.d[2], u.d[3]);
    else dp[0] = u.c[0];
  }
}

inline int li_grid(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" int rsp_slice_resize_pad(const void* scene, int32_t src_is_u8, int32_t SH, int32_t SW, const int32_t* origins,
                                    int32_t B, int32_t th, int32_t tw, float* dst, int32_t Hn, int32_t Wn, int32_t Hp,
                                    int32_t Wp, const float* pad3, int32_t normalise, int32_t swap_rb, const float* mean3,
                                    const float* std3, rsp_stream_t stream) {
  if (!scene || !origins || !dst || !pad3 || B < 0 || B > 65535 || SH <= 0 || SW <= 0 || th <= 0 || tw <= 0 || th > SH ||
      tw > SW || Hn <= 0 || Wn <= 0 || Hp < Hn || Wp < Wn)
    return RSP_EINVAL;
  if (normalise && (!mean3 || !std3)) return RSP_EINVAL;
  if (B == 0) return RSP_OK;
  SliceP P;
  P.scene = scene; P.origins = origins; P.dst = dst;
  P.SH = SH; P.SW = SW; P.th = th; P.tw = tw; P.Hn = Hn; P.Wn = Wn; P.Hp = Hp; P.Wp = Wp;
  P.normalise = normalise; P.swap_rb = swap_rb;
  for (int c = 0; c < 3; ++c) {
    P.p[c] = pad3[c];
    P.m[c] = normalise ? mean3[c] : 0.f;
    P.s[c] = normalise ? std3[c] : 1.f;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = (int64_t)Hp * Wp;
  if (src_is_u8 && th == Hn && tw == Wn && (Wp & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    hipLaunchKernelGGL(slice_convert_pad_kernel, dim3(li_grid((int64_t)Hp * ((Wp + 15) >> 4)), B), dim3(256), 0, s, P);
  } else if (src_is_u8) {
    hipLaunchKernelGGL((slice_resize_pad_kernel<uint8_t>), dim3(li_grid(total), B), dim3(256), 0, s, P);
  } else {
    hipLaunchKernelGGL((slice_resize_pad_kernel<float>), dim3(li_grid(total), B), dim3(256), 0, s, P);
  }
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_crops_resize_pad(const void* image, int32_t src_is_u8, int32_t SH, int32_t SW, const int32_t* table,
                                    int32_t B, float* dst, int32_t Hp, int32_t Wp, const float* pad3, int32_t normalise,
                                    int32_t swap_rb, const float* mean3, const float* std3, rsp_stream_t stream) {
  if (!image || !table || !dst || !pad3 || B < 0 || B > 65535 || SH <= 0 || SW <= 0 || Hp <= 0 || Wp <= 0) return RSP_EINVAL;
  if (normalise && (!mean3 || !std3)) return RSP_EINVAL;
  if (B == 0) return RSP_OK;
  CropsP P;
  P.image = image; P.table = table; P.dst = dst;
  P.SH = SH; P.SW = SW; P.Hp = Hp; P.Wp = Wp; P.normalise = normalise; P.swap_rb = swap_rb;
  for (int c = 0; c < 3; ++c) {
    P.p[c] = pad3[c];
    P.m[c] = normalise ? mean3[c] : 0.f;
    P.s[c] = normalise ? std3[c] : 1.f;
  }
  const int64_t total = (int64_t)Hp * Wp;
  if (src_is_u8)
    hipLaunchKernelGGL((crops_resize_pad_kernel<uint8_t>), dim3(li_grid(total), B), dim3(256), 0, (hipStream_t)stream, P);
  else
    hipLaunchKernelGGL((crops_resize_pad_kernel<float>), dim3(li_grid(total), B), dim3(256), 0, (hipStream_t)stream, P);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_rle_shift(const uint32_t* counts_in, const int32_t* n_in, int32_t k, int32_t cap_in,
                             const int32_t* offsets, int32_t h, int32_t w, int32_t H, int32_t W, uint32_t* counts_out,
                             int32_t* n_out, int32_t cap_out, rsp_stream_t stream) {
  if (!counts_in || !n_in || !offsets || !counts_out || !n_out || k < 0 || cap_in < 1 || cap_out < 2 || h <= 0 || w <= 0 ||
      h > H || w > W)
    return RSP_EINVAL;
  if (!rsp_run_canvas_ok(H, W)) return RSP_EINVAL;               // h <= H and w <= W above: refuses the pixel count only
  if (k == 0) return RSP_OK;
  hipLaunchKernelGGL(rle_shift_kernel, dim3(k), dim3(SHIFT_THREADS), 0, (hipStream_t)stream, counts_in, n_in, cap_in,
                     offsets, h, w, H, W, counts_out, n_out, cap_out);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}

extern "C" int rsp_paste_tiles(const uint8_t* masks, const int32_t* offsets, int32_t k, int32_t h, int32_t w, int32_t H,
                               int32_t W, uint8_t* out, rsp_stream_t stream) {
  if (!masks || !offsets || !out || k < 0 || k > 65535 || h <= 0 || w <= 0 || h > H || w > W) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  hipStream_t s = (hipStream_t)stream;
  if ((W & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    hipLaunchKernelGGL((paste_tiles_kernel<16>), dim3(li_grid((int64_t)H * (W / 16)), k), dim3(256), 0, s, masks, offsets,
                       h, w, H, W, out);
  } else {
    hipLaunchKernelGGL((paste_tiles_kernel<1>), dim3(li_grid((int64_t)H * W), k), dim3(256), 0, s, masks, offsets, h, w, H,
                       W, out);
  }
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
