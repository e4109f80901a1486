// The device-side reader of run tables ("The run table and its one home").  A run table is counts [k, cap] +
// n [k]: the COCO run counts of k masks on ONE (H, W) canvas as rsp_mask_rle / rsp_rle_shift / rsp_rle_union write them --
// column-major stream, the first run counts zeros, only count 0 may be zero, n <= 0 = an empty row (a row that did not
// fit its producer's capacity reports n < 0).  Every kernel that needs the pixel starts of a row's runs takes the row, the
// walk and the column arithmetic of a ones-run from here (rle_shift_kernel keeps a copy of its own: see there); the ones
// prefix of a row and its two-ended search (seam merge, run-domain IoU) are at the end of the file.  Include
// it after rsp_common.h (it uses rsp_block_excl_scan and does not include it itself: the emulated build rewrites that
// include per source file).
#pragma once

// The canvas of a run table: H * W fits COCO's 32-bit counts, and with them the int pixel starts of the walk.
inline bool rsp_run_canvas_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffffLL; }

// An offset of a caller's exclusive sum (piece_offs, interval_offs, ...) cut into [lo, hi], whatever the array holds.
__device__ __forceinline__ int64_t rsp_clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Row m of a table: n is cut at the capacity, whatever the array holds.
struct RspRunRow {
  const uint32_t* c;
  int n;
};
__device__ __forceinline__ RspRunRow rsp_run_row(const uint32_t* __restrict__ counts, const int32_t* __restrict__ n_in,
                                                 int cap, int m) {
  return RspRunRow{counts + (int64_t)m * cap, min(n_in[m], cap)};
}

// Block-cooperative walk over the runs of a row, NTHREADS runs per chunk (tmp = NTHREADS / 64 ints of LDS):
//   for (RspRunWalk<NTHREADS> r(row, tmp); r.next();) { ... r.i, r.c, r.s ... }
// After next() every thread holds ITS run of the chunk: index i, count c (0 when i >= row.n: the tail of the last chunk)
// and pixel start s; run i is a ones-run iff i is odd.  All threads of the block call next() together and it holds
// __syncthreads(); the body may scan again with the same tmp, synchronise, and leave its own inner loops early.  An empty
// row has no chunk.  Slots at or beyond row.n are never read (the producer did not write them).
template <int NTHREADS>
struct RspRunWalk {
  int i, c, s;
  __device__ __forceinline__ RspRunWalk(const RspRunRow& row, int* tmp) : i(0), c(0), s(0), row_(row), tmp_(tmp), i0_(0), px_(0) {}
  __device__ __forceinline__ bool next() {
    if (i0_ >= row_.n) return false;
    i = i0_ + (int)threadIdx.x;
    // Clamped index + masked value, no branch in front of the scan's shuffles: the rule of the comment on
    // rsp_block_excl_scan (rsp_common.h).  The emulated build (tests/wave_emu) breaks on `i < n ? row[i] : 0` here.
    c = (int)row_.c[min(i, row_.n - 1)] & -(int)(i < row_.n);
    int chunk_px;
    s = px_ + rsp_block_excl_scan<NTHREADS>(c, tmp_, &chunk_px);
    px_ += chunk_px;                                  // the pixels in front of the next chunk
    i0_ += NTHREADS;
    return true;
  }

 private:
  const RspRunRow row_;
  int* const tmp_;
  int i0_, px_;
};

// The columns of the ones-run [s, s + c), c > 0, on a canvas of column height H: it touches columns xa .. xb, from row ra
// of xa to row rb of xb (inclusive); when xa < xb it covers the columns in between and reaches the last row of xa and the
// first row of xb.  xb - xa + 1 is its number of column pieces.
struct RspRunCols {
  int xa, xb, ra, rb;
};
__device__ __forceinline__ RspRunCols rsp_run_cols(int s, int c, int H) {
  const int e1 = s + c - 1, xa = s / H, xb = e1 / H;
  return RspRunCols{xa, xb, s - xa * H, e1 - xb * H};
}

// ------------------------------------------------------------------------------------------------- ones prefix of a row
// The prefix workspace of a row (int32 [cap], next to the counts row): for ones-run t (count index 2 t + 1 < n)
//   w_row[2 t]     = ones pixels in front of the run          w_row[2 t + 1] = pixel start of the run
// One step per chunk of a block's walk over the row (one block per row, tmp as for RspRunWalk):
//   RspRunPrefix<NTHREADS> p;
//   for (RspRunWalk<NTHREADS> r(row, tmp); r.next();) p.step(r, row, w_row, tmp);
// Afterwards p.ones = the ones pixels of the row (rleArea) in every thread, and p.lo / p.hi = THIS thread's part of the
// row's extent: the smallest start and the largest end of its ones-runs of at least one pixel (0x7fffffff / 0 when it has
// none), to be reduced by whoever wants the extent.
template <int NTHREADS>
struct RspRunPrefix {
  int ones, lo, hi;
  __device__ __forceinline__ RspRunPrefix() : ones(0), lo(0x7fffffff), hi(0) {}
  __device__ __forceinline__ void step(const RspRunWalk<NTHREADS>& r, const RspRunRow& row, int32_t* __restrict__ w_row,
                                       int* tmp) {
    int chunk_ones;
    const int ob = ones + rsp_block_excl_scan<NTHREADS>((r.i & 1) ? r.c : 0, tmp, &chunk_ones);
    if (r.i < row.n && (r.i & 1)) {
      w_row[r.i - 1] = ob;
      w_row[r.i] = r.s;
      lo = min(lo, r.c > 0 ? r.s : 0x7fffffff);
      hi = max(hi, r.c > 0 ? r.s + r.c : 0);
    }
    ones += chunk_ones;
  }
};

// A row with its prefix workspace.  Nothing below asks the counts to be canonical: a ones-run of zero pixels, and with it
// two ones-runs that share a start, are found and counted for what they are.
struct SmRow {
  const uint32_t* c;
  const int32_t* ws;
  int nr;                   // ones-runs
};

// last ones-run whose start is <= p; -1: none.  Among runs that share a start it is the last of them: the others hold no
// pixel, and ws[2 t] of the last one counts everything in front of the shared start.
__device__ __forceinline__ int sm_find(const SmRow& r, int p) {
  int lo = -1, hi = r.nr - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (r.ws[2 * mid + 1] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ones pixels of the row in [0, p)
__device__ __forceinline__ int sm_ones_before(const SmRow& r, int p) {
  const int t = sm_find(r, p);
  if (t < 0) return 0;
  return r.ws[2 * t] + min(p - r.ws[2 * t + 1], (int)r.c[2 * t + 1]);
}
