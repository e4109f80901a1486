// Euclidean buffers in the run domain: dilation of every mask of a run table by a structuring element that is
// given as a table of half-heights, hh[dx] = the rows the element reaches above and below its centre at column offset dx,
// non-increasing in dx -- the exact disc dx^2 + dy^2 <= r2 (hh[dx] = isqrt(r2 - dx^2), filled on the host: no square root
// runs here, so nothing can round) or the diamond (hh[dx] = r - dx).  Erosion is the complement's dilation (ops.py).
//
// The disc does not separate into a column pass and a window of columns as the square of run_morphology.hip does.  What
// keeps the work away from area x R is the pruning of the sources: with T(X) the column pieces of column X,
// E+(X) = T(X) - T(X + 1) and E-(X) = T(X) - T(X - 1) (rsp_run_morph_join's op 1 with a column shift of +-1),
//   dilate(M)(X) = grow(T(X), hh[0])  u  U_{dx = 1..R} grow(E+(X - dx), hh[dx])  u  U_{dx = 1..R} grow(E-(X + dx), hh[dx]),
// grow([a, b), h) = [max(a - h, 0), min(b + h, H)): a set pixel dx columns to the left of the target, walked to the right
// along its row while the mask lasts, ends in the target column (the dx = 0 term covers it, hh[0] >= hh[dx]) or in a pixel of
// E+ that is nearer (hh is non-increasing, so that pixel reaches at least as far).  Only pieces with a free side emit.
//
// EMIT (rsp_run_disc_emit).  One lane per (source interval, dx) stores one (instance << 31 | pixel start, pixel end) interval
// of rsp_rle_union.  dir = 0: the table itself grown by hh[0], slot = the interval's number.  dir = +1 / -1: the table is E+ /
// E-, the targets are the columns X + dx / X - dx for dx = 1 .. R that lie on the canvas, and the slots of interval i are
// slot_offs[i] .. slot_offs[i + 1], the caller's exclusive sum of min(R, W - 1 - X) / min(R, X): the number of targets is
// known from the column alone, so there is no count pass.  Consecutive lanes hold consecutive dx of one source: they read
// one interval and store neighbouring slots.  Every slot is stored once with a plain store; no atomics; a second launch gives
// the same bits.  The intervals of one target column come from up to 2 R + 1 sources, so the caller sorts the keys before
// rsp_rle_union, which merges what overlaps or touches.
#include "rsp_common.h"
#include "run_table.h"

namespace {

constexpr int RD_THREADS = 256;

__global__ __launch_bounds__(RD_THREADS) void rd_emit_kernel(const int32_t* __restrict__ col, const int32_t* __restrict__ y0,
                                                             const int32_t* __restrict__ y1, int64_t P, int k, int H, int W,
                                                             const int32_t* __restrict__ hh, int R, int dir,
                                                             const int64_t* __restrict__ slot_offs, int64_t base, int64_t total,
                                                             int64_t* __restrict__ keys, int32_t* __restrict__ ends) {
  const int per = dir == 0 ? 1 : R;                        // lanes per source interval
  const int64_t work = P * (int64_t)per, stride = (int64_t)gridDim.x * RD_THREADS;
  for (int64_t t = (int64_t)blockIdx.x * RD_THREADS + threadIdx.x; t < work; t += stride) {
    const int64_t i = t / per;
    const int j = (int)(t - i * per);
    const int dx = dir == 0 ? 0 : j + 1;
    const int c = col[i], a = y0[i], b = y1[i];
    const int inst = c / W;
    const int xt = c - inst * W + dir * dx;
    if (c < 0 || inst >= k || a >= b || a < 0 || b > H || xt < 0 || xt >= W) continue;
    int64_t q = base + i, q1 = base + i + 1;
    if (dir != 0) {
      const int64_t room = total - base;
      q1 = base + rsp_clamp64(slot_offs[i + 1], 0, room);
      q = base + rsp_clamp64(slot_offs[i], 0, room) + j;
    }
    if (q >= q1 || q >= total) continue;
    const int h = min(max(hh[dx], 0), H);
    const int px = xt * H;
    keys[q] = ((int64_t)inst << 31) | (int64_t)(px + max(a - h, 0));
    ends[q] = px + min(b + h, H);
  }
}

inline int rd_grid(int64_t work) {
  const int64_t b = (work + RD_THREADS - 1) / RD_THREADS;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

extern "C" int rsp_run_disc_emit(const int32_t* col, const int32_t* y0, const int32_t* y1, int64_t P, int32_t k, int32_t H,
                                 int32_t W, const int32_t* hh, int32_t R, int32_t dir, const int64_t* slot_offs, int64_t base,
                                 int64_t total, int64_t* keys, int32_t* ends, rsp_stream_t stream) {
  if (P < 0 || P > 0x7fffffffLL || k < 0 || !rsp_run_canvas_ok(H, W) || (int64_t)(k > 0 ? k : 1) * W > 0x7fffffffLL) return RSP_EINVAL;
  if (R < 0 || R > W - 1 || dir < -1 || dir > 1 || base < 0 || total < 0 || total > 0x7fffffffLL || base > total) return RSP_EINVAL;
  if (P == 0 || k == 0 || total == base || (dir != 0 && R == 0)) return RSP_OK;
  if (!col || !y0 || !y1 || !hh || !keys || !ends || (dir != 0 && !slot_offs)) return RSP_EINVAL;
  hipLaunchKernelGGL(rd_emit_kernel, dim3(rd_grid(P * (int64_t)(dir == 0 ? 1 : R))), dim3(RD_THREADS), 0, (hipStream_t)stream, col,
                     y0, y1, P, k, H, W, hh, R, dir, slot_offs, base, total, keys, ends);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
