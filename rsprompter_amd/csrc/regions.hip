// Connected-component cleanup of binary masks: segment-anything's `remove_small_regions` (utils/amg.py; there one mask at a
// time on the host through cv2.connectedComponentsWithStats, connectivity 8) and what `postprocess_small_regions`
// (automatic_mask_generator.py) does with it, for k masks on the device.  One pass = one polarity ("holes": the components of
// ~mask, "islands": those of mask):
//
//   region_label_kernel    one block labels one 64 x 64 tile with union-find in LDS; writes parent[p] = the tile-local root
//                          (as a MASK-LOCAL pixel index y W + x; -1 where `working` is 0) and cnt[p] = the size of the
//                          tile-local component at its root, 0 elsewhere
//   region_seam_kernel     every pixel of the first row / column of a tile unites with its up to three neighbours across the
//                          tile edge (the diagonals at four-tile corners are among them); lock-free: atomicMin on root slots
//   region_flatten_kernel  SEPARATE LAUNCH: every tile-local root finds its root, points at it and adds its size to the root's
//   region_reduce_kernel   per mask: is there a small component, is there one that is not, and the largest one
//   region_write_kernel    the result byte of every pixel (and, in the last pass, its box and population count)
//
// A root is always the LOWEST index of its set (the larger root is hung under the smaller one), so a component's label is the
// minimum row-major index of its pixels whatever the schedule was, and max over (size << 32 | 0xFFFFFFFF - label) is the largest
// component, the one with the lowest first pixel among equals.  Every size / box / count is an integer reduction.
//
// Coherence: parents only ever DECREASE, and every value a slot has held is a member of the same set.  The
// seam kernel therefore stays correct whatever (older) value a read of a parent returns -- it reads them with relaxed
// agent-scope atomic loads all the same, writes them with atomicMin only, and compresses nothing.  Compression happens in the
// flatten launch, when no union is in flight.  Every find / union loop carries an explicit step cap; reaching it sets the
// mask's `status` and leaves the loop (a guard against a hang, not a path a correct run takes).  No inline assembly.
#include "rsp_common.h"

namespace {

constexpr int TH = RSP_MASK_REGION_TILE_H, TW = RSP_MASK_REGION_TILE_W, TPX = TH * TW;      // the tile
constexpr int ACC_INTS = 16;                        // per mask: see Acc
constexpr int MAX_MASKS_PER_LAUNCH = 32768;

// per-mask accumulators in the workspace (int32 slots)
enum Acc { A_FLAGS0 = 0, A_FLAGS1 = 1, A_KEY0 = 2, A_KEY1 = 4, A_X0 = 6, A_Y0 = 7, A_X1 = 8, A_Y1 = 9, A_POP = 10, A_STATUS = 11 };
constexpr int F_SMALL = 1, F_BIG = 2;

template <int SCOPE>
__device__ __forceinline__ int ld_parent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

// the root of x; `steps` counts against `cap` over the caller's whole operation.  HALVE (LDS only, where the block is coherent):
// hang x under its grandparent on the way, by atomicMin, so that the slot still only decreases.
template <int SCOPE, bool HALVE>
__device__ __forceinline__ int find_root(int* P, int x, int& steps, int cap) {
  for (;;) {
    const int p = ld_parent<SCOPE>(P + x);
    if (p == x || ++steps > cap) return x;
    if (HALVE) {
      const int g = ld_parent<SCOPE>(P + p);
      if (g != p) atomicMin(P + x, g);
      x = g;
    } else {
      x = p;
    }
  }
}

// lock-free union: hang the larger root under the smaller one; when the slot was no root any more, go on with what it held
// (atomicMin may have replaced that by b: then the old parent is the one that still has to meet b).  false: cap reached.
template <int SCOPE, bool HALVE>
__device__ __forceinline__ bool unite(int* P, int a, int b, int cap) {
  int steps = 0;
  for (;;) {
    a = find_root<SCOPE, HALVE>(P, a, steps, cap);
    b = find_root<SCOPE, HALVE>(P, b, steps, cap);
    if (steps > cap) return false;
    if (a == b) return true;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b);
    if (old == a) return true;
    a = old;
    if (++steps > cap) return false;
  }
}

struct RegionP {
  const uint8_t* src;     // [k, H, W]; working = (src != 0) ^ holes
  uint8_t* out;           // [k, H, W] (may be src: every pixel reads its own byte only)
  int* parent;            // [k, H, W]
  int* cnt;               // [k, H, W]
  int* acc;               // [k, ACC_INTS]
  int H, W, ntx, nty;
  int holes, slot, min_area, last, vec;
};

// ---------------------------------------------------------------------------------------------------- tile-local labelling
__global__ __launch_bounds__(256) void region_label_kernel(const RegionP q) {
  __shared__ int sL[TPX];
  __shared__ int sC[TPX];
  __shared__ unsigned long long sBits[TH];
  __shared__ int sFail;
  const int tid = threadIdx.x, m = blockIdx.y;
  const int ty = blockIdx.x / q.ntx, tx = blockIdx.x - ty * q.ntx;
  const int64_t base = (int64_t)m * q.H * q.W;
  const int H = q.H, W = q.W;
  if (tid == 0) sFail = 0;

  // load: a lane owns 16 consecutive pixels of one tile row (16 bytes where the row pitch allows)
  const int row = tid >> 2, seg = tid & 3;
  const int gy = ty * TH + row, gx0 = tx * TW + seg * 16;
  uint32_t m16 = 0;
  if (gy < H && gx0 < W) {
    const uint8_t* s = q.src + base + (int64_t)gy * W + gx0;
    const int nv = min(16, W - gx0);
    if (q.vec && nv == 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(s);
      const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) m16 |= (((w4[j >> 2] >> (8 * (j & 3))) & 0xffu) != 0u ? 1u : 0u) << j;
    } else {
      for (int j = 0; j < nv; ++j) m16 |= (s[j] != 0 ? 1u : 0u) << j;
    }
    if (q.holes) m16 = ~m16 & (nv == 16 ? 0xffffu : ((1u << nv) - 1u));
  }
  reinterpret_cast<unsigned short*>(sBits)[row * 4 + seg] = (unsigned short)m16;
  {
    // initial label: the first pixel of the horizontal run inside the lane's 16 pixels
    int start = -1;
    const int li0 = row * TW + seg * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if ((m16 >> j) & 1u) {
        if (start < 0) start = li0 + j;
        sL[li0 + j] = start;
      } else {
        sL[li0 + j] = -1;
        start = -1;
      }
      sC[li0 + j] = 0;
    }
  }
  __syncthreads();

  // unions: with the previous 16 pixels of the row, and with the row above.  Of the three upper neighbours one union is
  // enough: N when it is set (NW and NE are then in N's run) -- and not even that when the left pixel is set and NW too (the
  // left pixel has met that run); else NW unless the left pixel is set (NW is ITS N), NE unless the right one is (NE is its N).
  if (m16) {
    const unsigned long long cur = sBits[row], up = row > 0 ? sBits[row - 1] : 0ull;
    bool ok = true;
    for (int j = 0; j < 16; ++j) {
      if (!((m16 >> j) & 1u)) continue;
      const int x = seg * 16 + j, li = row * TW + x;
      const bool left = x > 0 && ((cur >> (x - 1)) & 1ull), right = x < TW - 1 && ((cur >> (x + 1)) & 1ull);
      const bool n = (up >> x) & 1ull, nw = x > 0 && ((up >> (x - 1)) & 1ull), ne = x < TW - 1 && ((up >> (x + 1)) & 1ull);
      if (j == 0 && left) ok &= unite<__HIP_MEMORY_SCOPE_WORKGROUP, true>(sL, li, li - 1, 2 * TPX);
      if (n) {
        if (!(left && nw)) ok &= unite<__HIP_MEMORY_SCOPE_WORKGROUP, true>(sL, li, li - TW, 2 * TPX);
      } else {
        if (nw && !left) ok &= unite<__HIP_MEMORY_SCOPE_WORKGROUP, true>(sL, li, li - TW - 1, 2 * TPX);
        if (ne && !right) ok &= unite<__HIP_MEMORY_SCOPE_WORKGROUP, true>(sL, li, li - TW + 1, 2 * TPX);
      }
    }
    if (!ok) sFail = 1;
  }
  __syncthreads();

  // flatten inside the tile; consecutive lanes take consecutive pixels now (coalesced stores)
  const int lx = tid & 63, gx = tx * TW + lx;
#pragma unroll 1
  for (int it = 0; it < 16; ++it) {
    const int ly = it * 4 + (tid >> 6), li = ly * TW + lx, y = ty * TH + ly;
    if (y >= H || gx >= W) continue;
    int lab = -1;
    if (sL[li] >= 0) {
      int steps = 0;
      const int r = find_root<__HIP_MEMORY_SCOPE_WORKGROUP, true>(sL, li, steps, TPX);
      if (steps > TPX) sFail = 1;
      atomicAdd(&sC[r], 1);
      lab = (ty * TH + (r >> 6)) * W + tx * TW + (r & 63);
    }
    q.parent[base + (int64_t)y * W + gx] = lab;
  }
  __syncthreads();
#pragma unroll 1
  for (int it = 0; it < 16; ++it) {
    const int ly = it * 4 + (tid >> 6), li = ly * TW + lx, y = ty * TH + ly;
    if (y >= H || gx >= W) continue;
    q.cnt[base + (int64_t)y * W + gx] = ld_parent<__HIP_MEMORY_SCOPE_WORKGROUP>(sL + li) == li ? sC[li] : 0;
  }
  if (tid == 0 && sFail) atomicOr(q.acc + (int64_t)m * ACC_INTS + A_STATUS, 1);
}

// ------------------------------------------------------------------------------------------------------------- seam merge
// thread = one pixel of a tile's first row (then its partners are (y - 1, x - 1 .. x + 1)) or of a tile's first column (then
// (y - 1 .. y + 1, x - 1)).  Whether a pixel is set is parent >= 0, which no union changes.
__global__ __launch_bounds__(256) void region_seam_kernel(const RegionP q) {
  const int m = blockIdx.y, H = q.H, W = q.W;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nh = (int64_t)(q.nty - 1) * W, nv = (int64_t)(q.ntx - 1) * H;
  if (t >= nh + nv) return;
  int* P = q.parent + (int64_t)m * H * W;
  // both ends of a union only move to lower indices, so it takes fewer than 2 H W steps
  const int cap = (int)min((int64_t)2 * H * W, (int64_t)0x7ffffff0);
  int y, x, py[3], px[3];
  if (t < nh) {
    const int s = (int)(t / W);
    x = (int)(t - (int64_t)s * W);
    y = (s + 1) * TH;
    for (int e = 0; e < 3; ++e) { py[e] = y - 1; px[e] = x - 1 + e; }
  } else {
    const int64_t u = t - nh;
    const int s = (int)(u / H);
    y = (int)(u - (int64_t)s * H);
    x = (s + 1) * TW;
    for (int e = 0; e < 3; ++e) { py[e] = y - 1 + e; px[e] = x - 1; }
  }
  const int me = y * W + x;
  if (ld_parent<__HIP_MEMORY_SCOPE_AGENT>(P + me) < 0) return;
  bool ok = true;
  for (int e = 0; e < 3; ++e) {
    if (py[e] < 0 || py[e] >= H || px[e] < 0 || px[e] >= W) continue;
    const int o = py[e] * W + px[e];
    if (ld_parent<__HIP_MEMORY_SCOPE_AGENT>(P + o) < 0) continue;
    ok &= unite<__HIP_MEMORY_SCOPE_AGENT, false>(P, me, o, cap);
  }
  if (!ok) atomicOr(q.acc + (int64_t)m * ACC_INTS + A_STATUS, 1);
}

// ------------------------------------------------------------------------------------------------------ flatten and count
// cnt > 0 marks a tile-local root.  One that is no root any more points at its root from here on (an older value another lane
// may still read is an ancestor all the same) and hands its pixels to it: one atomic per tile and component.
__global__ __launch_bounds__(256) void region_flatten_kernel(const RegionP q) {
  const int m = blockIdx.y;
  const int hw = q.H * q.W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  int* P = q.parent + (int64_t)m * hw;
  int* C = q.cnt + (int64_t)m * hw;
  const int c = C[p];
  if (c <= 0) return;
  int steps = 0;
  const int r = find_root<__HIP_MEMORY_SCOPE_AGENT, false>(P, p, steps, hw);
  if (steps > hw) { atomicOr(q.acc + (int64_t)m * ACC_INTS + A_STATUS, 1); return; }
  if (r != p) {
    __hip_atomic_store(P + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(C + r, c);
  }
}

// ---------------------------------------------------------------------------------------------------- per-mask decisions
__global__ __launch_bounds__(256) void region_reduce_kernel(const RegionP q) {
  __shared__ int sFlags;
  __shared__ unsigned long long sKey;
  const int m = blockIdx.y;
  const int hw = q.H * q.W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x == 0) { sFlags = 0; sKey = 0ull; }
  __syncthreads();
  if (p < hw && q.parent[(int64_t)m * hw + p] == p) {
    const int sz = q.cnt[(int64_t)m * hw + p];
    atomicOr(&sFlags, sz < q.min_area ? F_SMALL : F_BIG);
    atomicMax(&sKey, ((unsigned long long)(uint32_t)sz << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)p));
  }
  __syncthreads();
  if (threadIdx.x == 0 && sFlags) {
    int* acc = q.acc + (int64_t)m * ACC_INTS;
    atomicOr(acc + A_FLAGS0 + q.slot, sFlags);
    atomicMax(reinterpret_cast<unsigned long long*>(acc + A_KEY0 + 2 * q.slot), sKey);
  }
}

// -------------------------------------------------------------------------------------------------------------- the result
__global__ __launch_bounds__(256) void region_write_kernel(const RegionP q) {
  __shared__ int part[4][5];
  const int m = blockIdx.y, W = q.W;
  const int hw = q.H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int64_t base = (int64_t)m * hw;
  int* acc = q.acc + (int64_t)m * ACC_INTS;
  const int flags = acc[A_FLAGS0 + q.slot];
  int o = 0;
  if (p < hw) {
    const int s = q.src[base + p] != 0 ? 1 : 0;
    o = s;
    if (flags & F_SMALL) {
      const int lab = q.parent[base + p];             // the tile-local root, which points at the root since the flatten launch
      if (lab >= 0) {
        const int root = q.parent[base + lab];
        const int sz = q.cnt[base + root];
        if (q.holes) {
          o = sz < q.min_area ? 1 : 0;                // a small hole is filled
        } else if (flags & F_BIG) {
          o = sz >= q.min_area ? 1 : 0;
        } else {                                      // every component is small: the largest stays
          const unsigned long long key = *reinterpret_cast<const unsigned long long*>(acc + A_KEY0 + 2 * q.slot);
          o = (uint32_t)root == 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull) ? 1 : 0;
        }
      }
    }
    q.out[base + p] = (uint8_t)o;
  }
  if (!q.last) return;
  int y = 0, x = 0;
  if (o) { y = p / W; x = p - y * W; }
  int v[5] = {o ? x : 0x7fffffff, o ? y : 0x7fffffff, o ? x : -1, o ? y : -1, o};
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    v[0] = min(v[0], __shfl_xor(v[0], d, 64));
    v[1] = min(v[1], __shfl_xor(v[1], d, 64));
    v[2] = max(v[2], __shfl_xor(v[2], d, 64));
    v[3] = max(v[3], __shfl_xor(v[3], d, 64));
    v[4] += __shfl_xor(v[4], d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 5; ++j) part[threadIdx.x >> 6][j] = v[j];
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < 5 && part[0][4] + part[1][4] + part[2][4] + part[3][4] > 0) {
    const int v0 = part[0][j], v1 = part[1][j], v2 = part[2][j], v3 = part[3][j];
    if (j < 2) atomicMin(acc + A_X0 + j, min(min(v0, v1), min(v2, v3)));
    else if (j < 4) atomicMax(acc + A_X0 + j, max(max(v0, v1), max(v2, v3)));
    else atomicAdd(acc + A_POP, v0 + v1 + v2 + v3);
  }
}

__global__ __launch_bounds__(256) void region_init_kernel(int* acc, int k) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= k) return;
  int* a = acc + (int64_t)m * ACC_INTS;
  for (int j = 0; j < ACC_INTS; ++j) a[j] = 0;
  a[A_X0] = a[A_Y0] = 0x7fffffff;
  a[A_X1] = a[A_Y1] = -1;
}

__global__ __launch_bounds__(256) void region_info_kernel(const int* acc, int k, int32_t* info) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= k) return;
  const int* a = acc + (int64_t)m * ACC_INTS;
  int32_t* o = info + (int64_t)m * 8;
  const bool any = a[A_POP] > 0;
  o[0] = (a[A_FLAGS0] & F_SMALL) ? 1 : 0;
  o[1] = (a[A_FLAGS1] & F_SMALL) ? 1 : 0;
  o[2] = any ? a[A_X0] : 0; o[3] = any ? a[A_Y0] : 0; o[4] = any ? a[A_X1] : 0; o[5] = any ? a[A_Y1] : 0;
  o[6] = a[A_POP];
  o[7] = a[A_STATUS];
}

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

void run_pass(RegionP q, int k, hipStream_t st) {
  const int hw = q.H * q.W;
  const dim3 px((unsigned)((hw + 255) / 256), k);
  hipLaunchKernelGGL(region_label_kernel, dim3((unsigned)(q.ntx * q.nty), k), dim3(256), 0, st, q);
  const int64_t seam = (int64_t)(q.nty - 1) * q.W + (int64_t)(q.ntx - 1) * q.H;
  if (seam > 0) hipLaunchKernelGGL(region_seam_kernel, dim3((unsigned)((seam + 255) / 256), k), dim3(256), 0, st, q);
  hipLaunchKernelGGL(region_flatten_kernel, px, dim3(256), 0, st, q);
  hipLaunchKernelGGL(region_reduce_kernel, px, dim3(256), 0, st, q);
  hipLaunchKernelGGL(region_write_kernel, px, dim3(256), 0, st, q);
}

}  // namespace

extern "C" int64_t rsp_mask_regions_workspace_bytes(int32_t k, int32_t H, int32_t W) {
  if (k < 0 || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return -1;
  const int64_t n = (int64_t)k * H * W;
  return 2 * align256(4 * n) + align256((int64_t)k * ACC_INTS * 4);
}

extern "C" int rsp_mask_remove_small_regions(const uint8_t* masks, int32_t k, int32_t H, int32_t W, int32_t min_area, int32_t mode,
                                             void* workspace, uint8_t* out, int32_t* info, rsp_stream_t stream) {
  if (k < 0 || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31) || min_area < 0 || mode < 1 || mode > 3) return RSP_EINVAL;
  if (k == 0) return RSP_OK;
  if (!masks || !workspace || !out || !info || (const uint8_t*)out == masks || ((uintptr_t)workspace & 15)) return RSP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)k * H * W;
  char* ws = static_cast<char*>(workspace);
  int* parent = reinterpret_cast<int*>(ws);
  int* cnt = reinterpret_cast<int*>(ws + align256(4 * n));
  int* acc = reinterpret_cast<int*>(ws + 2 * align256(4 * n));
  hipLaunchKernelGGL(region_init_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, acc, k);
  for (int32_t k0 = 0; k0 < k; k0 += MAX_MASKS_PER_LAUNCH) {
    const int kc = k - k0 < MAX_MASKS_PER_LAUNCH ? k - k0 : MAX_MASKS_PER_LAUNCH;
    const int64_t off = (int64_t)k0 * H * W;
    RegionP q;
    q.parent = parent + off; q.cnt = cnt + off; q.acc = acc + (int64_t)k0 * ACC_INTS;
    q.H = H; q.W = W; q.ntx = (W + TW - 1) / TW; q.nty = (H + TH - 1) / TH;
    q.min_area = min_area;
    q.out = out + off;
    if (mode & 1) {                                     // holes
      q.src = masks + off; q.holes = 1; q.slot = 0; q.last = mode == 1;
      q.vec = (W % 16 == 0) && (((uintptr_t)q.src & 15) == 0);
      run_pass(q, kc, st);
    }
    if (mode & 2) {                                     // islands (of the hole-filled mask in mode 3: in place on `out`)
      q.src = mode == 3 ? (const uint8_t*)(out + off) : masks + off; q.holes = 0; q.slot = 1; q.last = 1;
      q.vec = (W % 16 == 0) && (((uintptr_t)q.src & 15) == 0);
      run_pass(q, kc, st);
    }
  }
  hipLaunchKernelGGL(region_info_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, acc, k, info);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
