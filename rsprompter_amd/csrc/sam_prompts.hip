// SAM prompt encoder for point / box prompts (HF SamPromptEncoder._embed_points / _embed_boxes / forward, modeling_sam.py:613-698,
// over SamPositionalEmbedding.forward :552-566).
//   sparse[r, t, 0:F]  = sin(2 pi (cx g[0, f] + cy g[1, f])) (+ type embedding),  sparse[r, t, F:2F] = cos(..) (+ type embedding)
//   with (cx, cy) = 2 ((coordinate + 0.5) / size) - 1 and the tokens of prompt set r in HF's order:
//   P points, the padding point (only when there is no box), the two box corners.
// The sine / cosine argument is formed exactly as embed_boxes_kernel (resnet.hip) forms it, so a boxes-only call returns the
// bits rsp_sam_embed_boxes returns.
#include "rsp_common.h"

namespace {

struct PromptP {
  const float* points;    // [R, P, 2] or null
  const int32_t* labels;  // [R, P] or null: null with points = the bare positional encoding (no + 0.5, no type embedding)
  const float* boxes;     // [R, 4] or null
  const float* g;         // [2, F]
  const float* pe[4];     // point_embed.0 .. 3, [2F] each
  const float* nap;       // not_a_point_embed [2F]
  float* out;             // [R, T, 2F]
  int R, P, pad, T, F;
  float size_w, size_h;
};

__global__ __launch_bounds__(256) void embed_prompts_kernel(const PromptP p) {
  const int F = p.F;
  const int64_t total = (int64_t)p.R * p.T * F;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    const int t = (int)((i / F) % p.T);
    const int64_t r = i / ((int64_t)F * p.T);
    float* o = p.out + (r * p.T + t) * 2 * F;
    float px, py;
    const float* add = nullptr;       // type embedding added to the positional encoding
    const float* repl = nullptr;      // ... or the row that replaces it
    bool zero = false;
    if (t < p.P) {
      px = p.points[(r * p.P + t) * 2 + 0];
      py = p.points[(r * p.P + t) * 2 + 1];
      if (p.labels) {
        px += 0.5f; py += 0.5f;                                  // HF:615
        const int lab = p.labels[r * p.P + t];
        if (lab == -1) repl = p.nap;                             // HF:627
        else if (lab == -10) zero = true;                        // HF:631
        else if (lab == 0) add = p.pe[0];                        // HF:633-637
        else if (lab == 1) add = p.pe[1];                        // HF:639-643
      }
    } else if (t < p.P + p.pad) {
      px = py = 0.f;                                             // HF:616-622: the point (0, 0) with label -1
      repl = p.nap;
    } else {
      const int corner = t - p.P - p.pad;
      px = p.boxes[r * 4 + corner * 2 + 0] + 0.5f;               // HF:649
      py = p.boxes[r * 4 + corner * 2 + 1] + 0.5f;
      add = p.pe[2 + corner];                                    // HF:654-655
    }
    if (repl) {
      o[f] = repl[f];
      o[F + f] = repl[F + f];
      continue;
    }
    if (zero) {
      o[f] = 0.f;
      o[F + f] = 0.f;
      continue;
    }
    const float x = px / p.size_w;
    const float y = py / p.size_h;
    const float cx = 2.0f * x - 1.0f, cy = 2.0f * y - 1.0f;
    float v = cx * p.g[f] + cy * p.g[F + f];
    v = 6.283185307179586f * v;
    if (add) {
      o[f] = sinf(v) + add[f];
      o[F + f] = cosf(v) + add[F + f];
    } else {
      o[f] = sinf(v);
      o[F + f] = cosf(v);
    }
  }
}

}  // namespace

extern "C" int rsp_sam_embed_prompts(const float* points, const int32_t* labels, const float* boxes, int32_t R, int32_t P,
                                     int32_t pad, const float* gauss, const float* point_embed0, const float* point_embed1,
                                     const float* point_embed2, const float* point_embed3, const float* not_a_point_embed,
                                     float* out, int32_t num_pos_feats, int32_t input_h, int32_t input_w, rsp_stream_t stream) {
  if (!gauss || !out || R < 0 || P < 0 || (pad != 0 && pad != 1) || num_pos_feats < 1 || input_h < 1 || input_w < 1)
    return RSP_EINVAL;
  if ((P > 0) != (points != nullptr)) return RSP_EINVAL;
  if (!points && !boxes) return RSP_EINVAL;
  if (labels && (!point_embed0 || !point_embed1 || !not_a_point_embed)) return RSP_EINVAL;
  if (pad && (!not_a_point_embed || boxes)) return RSP_EINVAL;          // HF pads only when there is no box
  if (boxes && (!point_embed2 || !point_embed3)) return RSP_EINVAL;
  if (R == 0) return RSP_OK;
  PromptP p;
  p.points = points; p.labels = labels; p.boxes = boxes; p.g = gauss;
  p.pe[0] = point_embed0; p.pe[1] = point_embed1; p.pe[2] = point_embed2; p.pe[3] = point_embed3;
  p.nap = not_a_point_embed; p.out = out;
  p.R = R; p.P = P; p.pad = pad; p.T = P + pad + (boxes ? 2 : 0); p.F = num_pos_feats;
  p.size_w = (float)input_w; p.size_h = (float)input_h;
  const int64_t total = (int64_t)R * p.T * num_pos_feats;
  int64_t gx = (total + 255) / 256;
  if (gx > 65535) gx = 65535;
  hipLaunchKernelGGL(embed_prompts_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, p);
  RSP_CHECK_LAUNCH();
  return RSP_OK;
}
