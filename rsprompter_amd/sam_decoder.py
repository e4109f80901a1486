"""SAM mask decoder / positional embedding / prompt-encoder leftovers on HIP kernels.

Reference wrappers: mmdet/rsprompter/models.py  RSSamPositionalEmbedding :744-759,
RSSamPromptEncoder :881-896, RSSamMaskDecoder :899-914 around HuggingFace
SamPositionalEmbedding HF:552-566, SamMaskEmbedding HF:584-593, SamMaskDecoder HF:432-543,
SamTwoWayTransformer HF:351-405, SamTwoWayAttentionBlock HF:272-348, SamAttention HF:194-270.

MI355X design: the reference repeats the [256,64,64] image embedding, its
positional encoding and the dense prompt once per RoI (`repeat_interleave`, models.py:1680-1683)
before entering the decoder.  Here the per-image tensors stay per image: RoI -> image index maps
are applied inside the kernels (attention `kv_batch_map` / `q_batch_map`, GEMM `res_bmap`), the
positional encoding enters every key/query projection as a precomputed broadcast term
`pe @ W^T + b`, and layer-0 image-side projections are computed once per image.
"""
import math

import numpy as np
import torch

from . import ops
from .nnutil import HIPModule, add_param, infer_sam_arch, nchw_view, nhwc_view
from .registry import MODELS

HID = 256          # SamMaskDecoderConfig.hidden_size
HEADS = 8
MLP_DIM = 2048
N_MASK_TOKENS = 4  # num_multimask_outputs + 1
# Both product paths since round 5 (first GPU run + A/B on one box: profiles/r5_decoder_paths_ab.txt, -0.9 ms per ViT-H
# step together): the layer-1 / final token -> image attention with the K | V projections folded in (csrc/t2i_fold.hip)
# and the upscaler tail as one kernel (csrc/upscale.hip, sam_upscale_fused_kernel).  The instance attributes `t2i_fold` /
# `upscale_fused` remain so that the parity tests can hold the fused forms against the kernel chains they replace (those
# chains also serve the shapes the fused kernels do not take: more than 12 tokens, N % 32 != 0, R * N * 512 >= 2^31).


def _upscale2_k_order():
    """input-channel order of the second ConvTranspose's packed weight for rsp_sam_upscale_fused (include/rsp_hip.h): packed
    column 16 s + 8 hh + j holds channel 32 (s >> 1) + 8 ((8 (s & 1) + j) >> 2) + 4 hh + (j & 3)"""
    return [32 * ((kp >> 4) >> 1) + 8 * ((8 * ((kp >> 4) & 1) + (kp & 7)) >> 2) + 4 * ((kp >> 3) & 1) + (kp & 3) for kp in range(64)]


def _add_linear(root, name, cout, cin):
    add_param(root, name + '.weight', (cout, cin))
    add_param(root, name + '.bias', (cout,))


def _add_ln(root, name, c):
    add_param(root, name + '.weight', (c,), 1.0)
    add_param(root, name + '.bias', (c,))


def _add_attn(root, name, internal):
    for p in ('q_proj', 'k_proj', 'v_proj'):
        _add_linear(root, f'{name}.{p}', internal, HID)
    _add_linear(root, f'{name}.out_proj', HID, internal)


def _g(root, dotted):
    for p in dotted.split('.'):
        root = getattr(root, p)
    return root


HOOK_FORMS = ('accepted forms: attention_similarity 4-D [1 | B * Pb, 1, 1, N] (one bias row over the N image positions, shared '
              'or per prompt set; no per-head, per-token or other shape), with at most ops.SAM_T2I_MAX_TOKENS = 12 tokens; '
              'target_embedding [..., 256] that broadcasts to [B, Pb, 1, 256] (every other dimension 1 or equal)')


def persam_hooks(attention_similarity, target_embedding, B, Pb, N, T):
    """HF's PerSAM hooks (`SamModel.forward(attention_similarity=, target_embedding=)`, HF:183-187, 386-387) in the forms this
    decoder takes -> (bias [1 | B * Pb, N] or None, target rows [1 | B * Pb, 256] or None) for `decode`; every other shape
    raises NotImplementedError naming the accepted ones."""
    R = B * Pb
    bias = te = None
    if attention_similarity is not None:
        a = attention_similarity
        if not torch.is_tensor(a) or a.dim() != 4 or a.shape[1] != 1 or a.shape[2] != 1 or a.shape[3] != N or \
                a.shape[0] not in (1, R):
            raise NotImplementedError(f'attention_similarity of shape {tuple(getattr(a, "shape", ()))} for B * Pb = {R}, N = {N}; '
                                      + HOOK_FORMS)
        if T > ops.SAM_T2I_MAX_TOKENS:
            raise NotImplementedError(f'attention_similarity with {T} tokens (the generic attention takes no bias); ' + HOOK_FORMS)
        bias = a.reshape(a.shape[0], N).to(torch.float32).contiguous()     # (on the caller's device, as every other input)
    if target_embedding is not None:
        t = target_embedding
        ok = torch.is_tensor(t) and 1 <= t.dim() <= 4 and t.shape[-1] == HID
        if ok:
            b, pb, tk = ((1, 1, 1) + tuple(t.shape[:-1]))[-3:]
            ok = b in (1, B) and pb in (1, Pb) and tk == 1
        if not ok:
            raise NotImplementedError(f'target_embedding of shape {tuple(getattr(t, "shape", ()))} for B = {B}, Pb = {Pb}; '
                                      + HOOK_FORMS)
        t = t.to(torch.float32).reshape(b, pb, HID)
        te = t.reshape(1, HID) if b * pb == 1 else t.expand(B, Pb, HID).reshape(R, HID)
        te = te.contiguous()
    return bias, te


class SamMaskDecoderHIP(HIPModule):
    """Parameters in HF `SamMaskDecoder` layout."""

    def __init__(self):
        super().__init__()
        add_param(self, 'iou_token.weight', (1, HID))
        add_param(self, 'mask_tokens.weight', (N_MASK_TOKENS, HID))
        for i in range(2):
            p = f'transformer.layers.{i}'
            _add_attn(self, p + '.self_attn', HID)
            _add_attn(self, p + '.cross_attn_token_to_image', HID // 2)
            _add_attn(self, p + '.cross_attn_image_to_token', HID // 2)
            for j in range(1, 5):
                _add_ln(self, f'{p}.layer_norm{j}', HID)
            _add_linear(self, p + '.mlp.lin1', MLP_DIM, HID)
            _add_linear(self, p + '.mlp.lin2', HID, MLP_DIM)
        _add_attn(self, 'transformer.final_attn_token_to_image', HID // 2)
        _add_ln(self, 'transformer.layer_norm_final_attn', HID)
        add_param(self, 'upscale_conv1.weight', (HID, HID // 4, 2, 2))
        add_param(self, 'upscale_conv1.bias', (HID // 4,))
        add_param(self, 'upscale_conv2.weight', (HID // 4, HID // 8, 2, 2))
        add_param(self, 'upscale_conv2.bias', (HID // 8,))
        _add_ln(self, 'upscale_layer_norm', HID // 4)
        for i in range(N_MASK_TOKENS):
            p = f'output_hypernetworks_mlps.{i}'
            _add_linear(self, p + '.proj_in', HID, HID)
            _add_linear(self, p + '.layers.0', HID, HID)
            _add_linear(self, p + '.proj_out', HID // 8, HID)
        _add_linear(self, 'iou_prediction_head.proj_in', HID, HID)
        _add_linear(self, 'iou_prediction_head.layers.0', HID, HID)
        _add_linear(self, 'iou_prediction_head.proj_out', N_MASK_TOKENS, HID)
        self._pe_cache = {}
        # output tokens in front of the sparse prompts: iou + the mask tokens (SamHQMaskDecoderHIP appends its hq token)
        self.n_mask_tokens = N_MASK_TOKENS
        self.n_output_tokens = 1 + N_MASK_TOKENS
        # token -> image attention of layer 1 / final with the K | V projections folded in (csrc/t2i_fold.hip)
        self.t2i_fold = True
        # the upscaler tail in one kernel (csrc/upscale.hip, sam_upscale_fused_kernel)
        self.upscale_fused = True
        # parity tests: keep the stage tensors of the last decode() (per-RoI key planes, tokens, upscaler planes, hyper-network
        # vectors) in `_last_stages` so that a failure names its kernel; pins GBs at R = 800, hence off by default
        self.keep_stages = False
        self._last_stages = None
        # tests: decode() chunks above this many prompt sets (None: the folded attention's addressing limit, 1023 at 64 x 64)
        self.max_prompt_sets = None

    # ------------------------------------------------------------------ packing
    def _pw(self, name, with_bias=True):
        m = _g(self, name)
        return ops.PackedWeight(m.weight, m.bias if with_bias else None)

    def _pack(self):
        from .necks import convt_weights4
        P = {}
        for i in range(2):
            p = f'transformer.layers.{i}'
            for a in ('self_attn', 'cross_attn_token_to_image', 'cross_attn_image_to_token'):
                for pr in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
                    P[f'{i}.{a}.{pr}'] = self._pw(f'{p}.{a}.{pr}')
            P[f'{i}.lin1'] = self._pw(p + '.mlp.lin1')
            P[f'{i}.lin2'] = self._pw(p + '.mlp.lin2')
        for pr in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
            P[f'final.{pr}'] = self._pw(f'transformer.final_attn_token_to_image.{pr}')
        P['up1'] = convt_weights4(self.upscale_conv1.weight, self.upscale_conv1.bias)
        P['up2'] = convt_weights4(self.upscale_conv2.weight, self.upscale_conv2.bias)
        # ... and with its input channels in the order the fused upscaler consumes them (ops.upscale2_k_order)
        w2 = self.upscale_conv2.weight.detach()[_upscale2_k_order()]
        P['up2p'] = convt_weights4(w2, self.upscale_conv2.bias)
        # K and V projections of the token->image attentions share their A operand: one [256 -> 128+128] GEMM
        for pre, p in (('0.cross_attn_token_to_image', 'transformer.layers.0.cross_attn_token_to_image'),
                       ('1.cross_attn_token_to_image', 'transformer.layers.1.cross_attn_token_to_image'),
                       ('final', 'transformer.final_attn_token_to_image')):
            kp, vp = _g(self, p + '.k_proj'), _g(self, p + '.v_proj')
            P[pre + '.kv_proj'] = ops.PackedWeight(torch.cat([kp.weight, vp.weight], 0))
            # the folded form (csrc/t2i_fold.hip) projects the QUERIES into key space instead: q' = Wk_h^T tq
            P[pre + '.k_projT'] = ops.PackedWeight(kp.weight.detach().t().contiguous())
        for i in range(N_MASK_TOKENS):
            for l in ('proj_in', 'layers.0', 'proj_out'):
                P[f'hyper{i}.{l}'] = self._pw(f'output_hypernetworks_mlps.{i}.{l}')
        for l in ('proj_in', 'layers.0', 'proj_out'):
            P[f'iou.{l}'] = self._pw(f'iou_prediction_head.{l}')
        self._packed = P
        self._pe_cache = {}

    def _pe_terms(self, pe_rows):
        """pe @ W^T + b for every image-side projection that consumes keys + pe (HF:326-343, 397-400)."""
        key = self._pe_key(pe_rows)
        if key not in self._pe_cache:
            P = self._packed
            t = {}
            for name in ('0.cross_attn_token_to_image.k_proj', '1.cross_attn_token_to_image.k_proj',
                         '0.cross_attn_image_to_token.q_proj', '1.cross_attn_image_to_token.q_proj',
                         'final.k_proj'):
                t[name] = ops.gemm(pe_rows, P[name])      # includes the projection bias
            for pre, p in (('0.cross_attn_token_to_image', 'transformer.layers.0.cross_attn_token_to_image'),
                           ('1.cross_attn_token_to_image', 'transformer.layers.1.cross_attn_token_to_image'),
                           ('final', 'transformer.final_attn_token_to_image')):
                vb = _g(self, p + '.v_proj').bias
                t[pre + '.kv_proj'] = torch.cat([t[pre + '.k_proj'], vb.unsqueeze(0).expand(pe_rows.shape[0], -1)],
                                                1).contiguous()
                # PEK of the folded token -> image form: k_proj(pe) WITHOUT the bias.  q . b_k is one constant per (query,
                # head), which the softmax cancels exactly; inside PEK that common level went through the fp16 split of every
                # key's row and came back as per-key logit noise of level * 2^-22 (tests/_score_fields.py: a k_proj offset)
                t[pre + '.pek_planes'] = ops.to_planes(ops.gemm(pe_rows, P[pre + '.k_proj'], bias=None))
            # the entry keeps the table it was computed from: while it is cached its memory cannot be handed to another tensor,
            # so an equal (pointer, shape, version) key means the same values.  The key is the table's NHWC rows: the models'
            # own tables are channels-last and hit on every call; a foreign NCHW-contiguous `image_pe` is copied to NHWC per
            # call (nhwc_view), so it misses every time and pays the five small pe GEMMs + to_planes again -- pass such a
            # table as `.contiguous(memory_format=torch.channels_last)` once
            t['_table'] = pe_rows
            self._pe_cache = {key: t}
        return self._pe_cache[key]

    @staticmethod
    def _pe_key(pe_rows):
        return (pe_rows.data_ptr(), tuple(pe_rows.shape), pe_rows._version)

    # ------------------------------------------------------------------ pieces
    def _ln(self, x, name, eps=1e-6, planes=False):
        m = _g(self, name)
        return ops.layernorm(x, m.weight, m.bias, eps, planes=planes)

    def _t2i(self, tq, kv, ao, R, T, N, kv_map=None, bias=None):
        """tokens -> image attention on the fused [K | V] projection (HF:326-331, 397-400); bias [1 | R, N]: HF's
        attention_similarity, added to the scaled logits (HF:260)."""
        d2, dh2 = HID // 2, (HID // 2) // HEADS
        if bias is not None:
            if T > ops.SAM_T2I_MAX_TOKENS:
                raise NotImplementedError(f'attention_similarity with {T} tokens; ' + HOOK_FORMS)
            return ops.sam_t2i_attention_bias(tq, kv, bias, ao, R=R, T=T, N=N, scale=dh2 ** -0.5, kv_map=kv_map)
        if T <= ops.SAM_T2I_MAX_TOKENS:
            return ops.sam_t2i_attention(tq, kv, ao, R=R, T=T, N=N, scale=dh2 ** -0.5, kv_map=kv_map)
        kvs = (N * 2 * d2, 2 * d2, dh2)
        return ops.attention(tq, kv, kv[:, d2:], ao, B=R, nh=HEADS, dh=dh2, Tq=T, Tk=N, scale=dh2 ** -0.5,
                             q_strides=(T * d2, d2, dh2), k_strides=kvs, v_strides=kvs,
                             o_strides=(T * d2, d2, dh2), kv_batch_map=kv_map)

    def _t2i_folded(self, pre, tq, keys_pl, pe_t, R, T, N):
        """tokens -> image attention over PER-RoI keys without their K | V projection (csrc/t2i_fold.hip): the queries are
        projected into key space (q' = Wk_h^T tq, one small GEMM on the block-diagonal tq), the kernel returns
        sum_n p[n] keys[n] per (head, token) column, v_proj is applied to that -- HF:326-331 / 397-400 re-associated.
        tq [R*T, 128] projected queries; returns the attention output [R*T, 128] (before out_proj)."""
        P = self._packed
        dh2 = (HID // 2) // HEADS
        # block diagonal: column h * T + t carries head h's 16 query values (softmax scale inside), zeros elsewhere -- one
        # kernel straight into planes (round 5: mul / permute / zeros / index_put / split in torch)
        tqx = ops.sam_fold_expand(tq, R, T, dh2 ** -0.5)
        qp = ops.gemm(tqx, P[pre + '.k_projT'], bias=None, out_planes=True, out_f32=False)      # [R*96, 256] planes
        u = ops.sam_t2i_fold(keys_pl, pe_t[pre + '.pek_planes'], qp, tqx, R=R, N=N, ncols=HEADS * T)
        full = ops.gemm(u, P[pre + '.v_proj'])                      # [R*96, 128]: every head's Wv on every column
        return ops.sam_fold_gather(full, R, T)                      # keep the column's own head: [R*T, 128]

    def _i2t(self, qi, kt, vt, ai, R, T, N, q_map=None):
        """image -> tokens attention; the result feeds the out_proj GEMM as planes (HF:340-345)."""
        d2, dh2 = HID // 2, (HID // 2) // HEADS
        if T <= ops.SAM_I2T_MAX_TOKENS:
            return ops.sam_i2t_attention(qi, kt, vt, R=R, T=T, N=N, scale=dh2 ** -0.5, q_map=q_map, out_planes=ai)
        return ops.attention(qi, kt, vt, None, B=R, nh=HEADS, dh=dh2, Tq=N, Tk=T, scale=dh2 ** -0.5,
                             q_strides=(N * d2, d2, dh2), k_strides=(T * d2, d2, dh2), v_strides=(T * d2, d2, dh2),
                             o_strides=(N * d2, d2, dh2), q_batch_map=q_map, out_planes=ai)

    def _token_attn(self, q_in, k_in, v_in, pfx, R, T, res=None):
        """SamAttention among the T prompt tokens of each RoI (self attention, internal dim 256)."""
        P = self._packed
        q = ops.gemm(q_in, P[pfx + '.q_proj'])
        k = ops.gemm(k_in, P[pfx + '.k_proj'])
        v = ops.gemm(v_in, P[pfx + '.v_proj'])
        dh = HID // HEADS
        o = torch.empty_like(q)
        st = (T * HID, HID, dh)
        ops.attention(q, k, v, o, B=R, nh=HEADS, dh=dh, Tq=T, Tk=T, scale=dh ** -0.5,
                      q_strides=st, k_strides=st, v_strides=st, o_strides=st)
        return ops.gemm(o, P[pfx + '.out_proj'], res=res)

    def decode(self, image_embeddings, image_pe, sparse, dense_vec, roi_img, want_iou=True, src_rows=None, hw=None,
               multimask_output=False, src_is_identity=False, attn_bias=None, target_rows=None, **head_kw):
        """The SAM mask decoder over R prompt sets (see _decode_chunk for the arguments).  Round 6: more prompt sets than the
        folded token -> image attention can address (R * N * 512 bytes of key planes < 2^31: 1023 at N = 4096) are decoded in
        chunks of equal size, each on the product path -- BASELINE configs[2] (16 tiles x 100 queries = 1600 prompt sets) used to
        fall back to the round-2 kernel chain (K | V projection GEMMs over all per-RoI keys + sam_t2i_kernel) for that reason.
        src_is_identity: roi_img is arange(R) over `src_rows` (the query variant: one dense-prompted source per prompt set), so a
        chunk only needs its own rows of `src_rows`.  attn_bias [1 | R, N] / target_rows [1 | R, 256]: HF's PerSAM hooks
        (persam_hooks); a per-prompt-set form is sliced with its chunk.  head_kw: further keyword arguments of `_heads` (none
        here; SamHQMaskDecoderHIP: hq_features, hq_token_only), the same for every chunk."""
        R = sparse.shape[0]
        if src_rows is None:
            N = image_embeddings.shape[-2] * image_embeddings.shape[-1]
        else:
            N = hw[0] * hw[1]
        max_r = self.max_prompt_sets or max(1, (2 ** 31 - 1) // (N * 512))
        if R <= max_r or not self.t2i_fold:
            return self._decode_chunk(image_embeddings, image_pe, sparse, dense_vec, roi_img, want_iou, src_rows, hw,
                                      multimask_output, attn_bias, target_rows, **head_kw)
        n_chunks = -(-R // max_r)
        per = -(-R // n_chunks)
        masks, ious = [], []
        for r0 in range(0, R, per):
            r1 = min(R, r0 + per)
            if src_rows is not None and src_is_identity:
                src_c = src_rows[r0 * N:r1 * N]
                map_c = roi_img[:r1 - r0]                     # arange(r1 - r0)
            else:
                src_c, map_c = src_rows, roi_img[r0:r1]
            bias_c = attn_bias if attn_bias is None or attn_bias.shape[0] == 1 else attn_bias[r0:r1].contiguous()
            te_c = target_rows if target_rows is None or target_rows.shape[0] == 1 else target_rows[r0:r1].contiguous()
            m, i = self._decode_chunk(image_embeddings, image_pe, sparse[r0:r1], dense_vec, map_c, want_iou, src_c, hw,
                                      multimask_output, bias_c, te_c, **head_kw)
            masks.append(m)
            ious.append(i)
        return torch.cat(masks, 0), (torch.cat(ious, 0) if want_iou else None)

    def _decode_chunk(self, image_embeddings, image_pe, sparse, dense_vec, roi_img, want_iou=True, src_rows=None, hw=None,
                      multimask_output=False, attn_bias=None, target_rows=None, **head_kw):
        """image_embeddings [B,256,h,w] (logical NCHW, channels-last), image_pe [1|B,256,h,w] (input
        independent; batch entry 0 is used), sparse [R, n_pts, 256], dense_vec [256] (the broadcast
        `no_mask_embed`, models.py:1680), roi_img int32 [R] image index of every RoI (sorted).
        Returns low_res_masks [R, 1, 4h, 4w] (mask token 0) and iou [R, 1]; multimask_output=True: the masks of mask
        tokens 1..3, [R, 3, 4h, 4w], and iou [R, 3] (HF:537-542).
        attn_bias [1 | R, N]: added to the logits of cross_attn_token_to_image in BOTH layers (HF:328-330), not in the final
        attention (HF:401); layer 1 then runs unfolded (K | V GEMM + the biased kernel).  target_rows [1 | R, 256]: HF:386-387
        `queries += target_embedding` is IN PLACE and at layer 0 `queries` IS `point_embeddings`, so the sum is both the
        initial queries and the token positional term of every layer and of the final attention, and layer 1 starts from
        q + target once more."""
        if self._packed is None:
            self._pack()
        P = self._packed
        if src_rows is None:
            emb = nhwc_view(image_embeddings)
            B, h, w, C = emb.shape
            dev = emb.device
        else:
            # query variant: `image_embeddings + dense prompt` already formed per source (rsp_sam_mask_embed);
            # src_rows [Bs*h*w, 256], roi_img maps every prompt set to its source
            h, w = hw
            C = src_rows.shape[-1]
            B = src_rows.shape[0] // (h * w)
            dev = src_rows.device
        N = h * w
        R, npts = sparse.shape[0], sparse.shape[1]
        T = self.n_output_tokens + npts
        pe_rows = nhwc_view(image_pe[:1]).reshape(N, C)
        if self._pe_key(pe_rows) not in self._pe_cache and image_pe.shape[0] > 1:
            # the image-wide positional embedding is ONE table repeated over the batch (models.py:85-95, 1685); its
            # projections are folded into broadcast terms below, so a caller with per-image tables must not get a
            # silently wrong answer (checked once per new table, not per step)
            if not bool((image_pe == image_pe[:1]).all()):
                raise NotImplementedError('image_positional_embeddings must be the same table for every batch entry')
        pe_t = self._pe_terms(pe_rows)
        d2, dh2 = HID // 2, (HID // 2) // HEADS

        # tokens = [iou, mask x4, sparse prompts] (HF:489-496)
        out_tok = self._output_tokens()
        tokens0 = torch.cat([out_tok.unsqueeze(0).expand(R, -1, -1), sparse.reshape(R, npts, HID)], 1)
        tokens0 = tokens0.reshape(R * T, HID).contiguous()
        te_rows = None
        if target_rows is not None:
            te_rows = target_rows if target_rows.shape[0] == 1 else \
                target_rows.unsqueeze(1).expand(R, T, HID).reshape(R * T, HID).contiguous()
            tokens0 = ops.add_rows(tokens0, te_rows)
        # keys of layer 0: image embedding + dense prompt, ONE copy per image (HF:499)
        if src_rows is None:
            src = ops.add_rows(emb.reshape(B * N, C), dense_vec.reshape(1, C), vmod=1)
        else:
            src = src_rows
        src_pl = ops.to_planes(src)

        # ---------------- layer 0 (HF:306-348 with skip_first_layer_pe) ----------------
        q = self._token_attn(tokens0, tokens0, tokens0, '0.self_attn', R, T)          # replaces queries
        q = self._ln(q, 'transformer.layers.0.layer_norm1')
        # tokens -> image
        qpe = ops.add_rows(q, tokens0)
        tq = ops.gemm(qpe, P['0.cross_attn_token_to_image.q_proj'])
        kv_img = ops.gemm(src_pl, P['0.cross_attn_token_to_image.kv_proj'], bias=None,
                          res=pe_t['0.cross_attn_token_to_image.kv_proj'], res_mod=N)    # per image, [K | V]
        ao = torch.empty_like(tq)
        self._t2i(tq, kv_img, ao, R, T, N, kv_map=roi_img, bias=attn_bias)
        q = ops.gemm(ao, P['0.cross_attn_token_to_image.out_proj'], res=q)
        q = self._ln(q, 'transformer.layers.0.layer_norm2')
        hmid = ops.gemm(q, P['0.lin1'], act=ops.ACT_RELU)
        q = ops.gemm(hmid, P['0.lin2'], res=q)
        q = self._ln(q, 'transformer.layers.0.layer_norm3')
        # image -> tokens: image-side queries are per image, keys/values per RoI
        qpe = ops.add_rows(q, tokens0)
        qi = ops.gemm(src_pl, P['0.cross_attn_image_to_token.q_proj'], bias=None,
                      res=pe_t['0.cross_attn_image_to_token.q_proj'], res_mod=N)
        kt = ops.gemm(qpe, P['0.cross_attn_image_to_token.k_proj'])
        vt = ops.gemm(q, P['0.cross_attn_image_to_token.v_proj'])
        m4 = _g(self, 'transformer.layers.0.layer_norm4')
        fused = T <= ops.SAM_I2T_FUSED_MAX_TOKENS
        ai = None
        if fused:
            # attention + out_proj (folded into the values) + residual (the per-IMAGE src rows) + layer_norm4 in one
            # kernel: neither the [R*N, 128] attention output nor the fp32 [R*N, 256] keys are ever written
            op = _g(self, 'transformer.layers.0.cross_attn_image_to_token.out_proj')
            keys_pl = ops.sam_i2t_fused(qi, kt, vt, op.weight.detach(), op.bias.detach(), m4.weight, m4.bias, R=R, T=T,
                                        N=N, scale=dh2 ** -0.5, eps=1e-6, q_map=roi_img, res=src, res_map=roi_img)
        else:
            ai = ops.empty_planes((R * N, d2), dev)  # attention output goes straight to the out_proj GEMM as planes
            self._i2t(qi, kt, vt, ai, R, T, N, q_map=roi_img)
            keys = ops.gemm(ai, P['0.cross_attn_image_to_token.out_proj'], res=src, res_bmap=roi_img, res_brows=N)
            # layer_norm4 emits planes only: they are both the A operand of layer 1's projections and (hi + lo) the
            # residual of its out_proj GEMM, so the fp32 copy of the per-RoI keys is never written
            keys_pl = ops.layernorm(keys, m4.weight, m4.bias, 1e-6, planes=True, f32=False)   # [R*N, 256] planes
            del keys
        del qi, kv_img

        # ---------------- layer 1 ----------------
        if te_rows is not None:
            q = ops.add_rows(q, te_rows)
        qpe = ops.add_rows(q, tokens0)
        q = self._token_attn(qpe, qpe, q, '1.self_attn', R, T, res=q)
        q = self._ln(q, 'transformer.layers.1.layer_norm1')
        qpe = ops.add_rows(q, tokens0)
        tq = ops.gemm(qpe, P['1.cross_attn_token_to_image.q_proj'])
        # (the kernel addresses a key plane with 32-bit byte offsets: R * N * 512 < 2^31, i.e. 1023 RoIs at N = 4096)
        fold = self.t2i_fold and T <= ops.SAM_T2I_FOLD_MAX_TOKENS and N % 32 == 0 and R * N * 512 < 2 ** 31
        kv = None
        if fold and attn_bias is None:
            ao = self._t2i_folded('1.cross_attn_token_to_image', tq, keys_pl, pe_t, R, T, N)
        else:
            # (with a similarity: the folded kernel takes no bias, so the K | V GEMM and the biased kernel; free at PerSAM's R = B)
            kv = ops.gemm(keys_pl, P['1.cross_attn_token_to_image.kv_proj'], bias=None,
                          res=pe_t['1.cross_attn_token_to_image.kv_proj'], res_mod=N)
            self._t2i(tq, kv, ao, R, T, N, bias=attn_bias)
        q = ops.gemm(ao, P['1.cross_attn_token_to_image.out_proj'], res=q)
        q = self._ln(q, 'transformer.layers.1.layer_norm2')
        hmid = ops.gemm(q, P['1.lin1'], act=ops.ACT_RELU)
        q = ops.gemm(hmid, P['1.lin2'], res=q)
        q = self._ln(q, 'transformer.layers.1.layer_norm3')
        qpe = ops.add_rows(q, tokens0)
        qi = ops.gemm(keys_pl, P['1.cross_attn_image_to_token.q_proj'], bias=None,
                      res=pe_t['1.cross_attn_image_to_token.q_proj'], res_mod=N)
        kt = ops.gemm(qpe, P['1.cross_attn_image_to_token.k_proj'])
        vt = ops.gemm(q, P['1.cross_attn_image_to_token.v_proj'])
        m4 = _g(self, 'transformer.layers.1.layer_norm4')
        if fused:
            op = _g(self, 'transformer.layers.1.cross_attn_image_to_token.out_proj')
            keys_pl = ops.sam_i2t_fused(qi, kt, vt, op.weight.detach(), op.bias.detach(), m4.weight, m4.bias, R=R, T=T,
                                        N=N, scale=dh2 ** -0.5, eps=1e-6, res_planes=keys_pl)
        else:
            self._i2t(qi, kt, vt, ai, R, T, N)
            keys = ops.gemm(ai, P['1.cross_attn_image_to_token.out_proj'], res=keys_pl)
            keys_pl = ops.layernorm(keys, m4.weight, m4.bias, 1e-6, planes=True, f32=False)   # planes only from here on
            del keys

        # ---------------- final token -> image attention (HF:396-404; LayerNorm default eps 1e-5) ----
        qpe = ops.add_rows(q, tokens0)
        tq = ops.gemm(qpe, P['final.q_proj'])
        if fold:
            ao = self._t2i_folded('final', tq, keys_pl, pe_t, R, T, N)
        else:
            kv = ops.gemm(keys_pl, P['final.kv_proj'], bias=None, res=pe_t['final.kv_proj'], res_mod=N, out=kv)
            self._t2i(tq, kv, ao, R, T, N)                       # no similarity here (HF:401)
        q = ops.gemm(ao, P['final.out_proj'], res=q)
        q = self._ln(q, 'transformer.layer_norm_final_attn', eps=1e-5)
        del kv, qi, ai
        q3 = q.view(R, T, HID)
        stages = dict(keys=keys_pl, tokens=q3, up=None, hyper=[]) if self.keep_stages else None
        hold = [keys_pl]                       # (handed over: _heads frees the keys as soon as the first ConvTranspose has read them)
        del keys_pl
        return self._heads(q3, hold, R, h, w, multimask_output, want_iou, stages, roi_img, src, **head_kw)

    def _output_tokens(self):
        """[iou, mask x4] (HF:489)"""
        return torch.cat([self.iou_token.weight, self.mask_tokens.weight], 0)

    def _hyper(self, q3, i, name=None):
        """hyper-network MLP `name` (default: output_hypernetworks_mlps.i -> packed 'hyper{i}') on output token 1 + i"""
        P = self._packed
        name = name or f'hyper{i}'
        mt = q3[:, 1 + i, :].contiguous()
        hy = ops.gemm(mt, P[name + '.proj_in'], act=ops.ACT_RELU)
        hy = ops.gemm(hy, P[name + '.layers.0'], act=ops.ACT_RELU)
        return ops.gemm(hy, P[name + '.proj_out'])

    def _iou_head(self, q3):
        P = self._packed
        it = q3[:, 0, :].contiguous()
        io = ops.gemm(it, P['iou.proj_in'], act=ops.ACT_RELU)
        io = ops.gemm(io, P['iou.layers.0'], act=ops.ACT_RELU)
        return ops.gemm(io, P['iou.proj_out'])

    def _heads(self, q3, hold, R, h, w, multimask_output, want_iou, stages, roi_img, src):
        """upscaling + hyper-networks + IoU head (HF:513-542) on the transformer's tokens q3 [R, T, 256] and the keys
        (planes, the only element of the list `hold`); roi_img: the prompt sets' image / source index into src
        [sources * h * w, 256] = image embedding + dense prompt (not read here)"""
        P = self._packed
        keys_pl = hold.pop()

        # ---------------- upscaling + hyper-network (HF:513-531) ----------------
        # mask token 0 is the only mask kept with multimask_output=False, tokens 1..3 otherwise (HF:537-542)
        toks = (1, 2, 3) if multimask_output else (0,)
        # both ConvTransposes run as one GEMM each (columns = (dy, dx, co), planes in); the second one never
        # stores its [R, 4h, 4w, 32] result: GELU and the product with hyper_in happen in its epilogue
        fused_up = self.upscale_fused and len(toks) == 1
        if not fused_up:
            up = ops.conv_transpose2x2(keys_pl.view(R, h, w, HID), *P['up1'], act=ops.ACT_GELU,
                                       ln=(self.upscale_layer_norm.weight, self.upscale_layer_norm.bias, 1e-6))
            del keys_pl                                                                 # [R, 2h, 2w, 64] planes
            if stages is not None:
                stages['up'] = up
        outs = []
        for i in toks:
            hy = self._hyper(q3, i)
            if stages is not None:
                stages['hyper'].append(hy)
            if fused_up:
                # one pass over the keys: no [R, 2h, 2w, 64] intermediate (csrc/upscale.hip, sam_upscale_fused_kernel)
                outs.append(ops.sam_upscale_fused(keys_pl, P['up1'][0], P['up1'][1], self.upscale_layer_norm.weight,
                                                  self.upscale_layer_norm.bias, 1e-6, P['up2p'][0], P['up2p'][1], hy,
                                                  h, w).view(R, 1, 4 * h, 4 * w))
                continue
            # (multimask: the last ConvTranspose is recomputed per token -- a rarely used option, no [R,4h,4w,32] tensor)
            outs.append(ops.conv_transpose2x2(up, *P['up2'], act=ops.ACT_GELU, hyper=hy).view(R, 1, 4 * h, 4 * w))
        masks = outs[0] if len(outs) == 1 else torch.cat(outs, 1)
        self._last_stages = stages
        iou = None
        if want_iou:
            io = self._iou_head(q3)
            iou = io[:, 1:4].contiguous() if multimask_output else io[:, 0:1]
        return masks, iou

    def forward(self, image_embeddings, image_positional_embeddings, sparse_prompt_embeddings,
                dense_prompt_embeddings, multimask_output=False, attention_similarity=None,
                target_embedding=None, output_attentions=None, **head_kw):
        """HF signature (HF:461-543): image_embeddings [B, 256, h, w], sparse_prompt_embeddings [B, Pb, n, 256] (or [B, n, 256]
        = point_batch_size 1), dense_prompt_embeddings [1 | B, 256, h, w] -- the broadcast `no_mask_embed` or a per-pixel one
        (SamMaskEmbedding's output).  Every batch entry is its own image and its Pb prompt sets stay mapped to it.  Returns
        (masks [B, Pb, C, 4h, 4w], iou [B, Pb, C], None) with C = 3 for multimask_output (mask tokens 1..3, HF:537-542)."""
        B = image_embeddings.shape[0]
        if sparse_prompt_embeddings.dim() == 4:
            Pb = sparse_prompt_embeddings.shape[1]
            sparse = sparse_prompt_embeddings.reshape(B * Pb, sparse_prompt_embeddings.shape[2], HID)
        else:
            Pb = 1
            sparse = sparse_prompt_embeddings
        bias, te = persam_hooks(attention_similarity, target_embedding, B, Pb,
                                image_embeddings.shape[-2] * image_embeddings.shape[-1], self.n_output_tokens + sparse.shape[1])
        dev = image_embeddings.device
        roi_img = torch.arange(B, dtype=torch.int32, device=dev)
        if Pb > 1:
            roi_img = roi_img.repeat_interleave(Pb)
        d = nhwc_view(dense_prompt_embeddings)
        if d.shape[0] not in (1, B):
            raise ValueError(f'dense_prompt_embeddings: batch {d.shape[0]} for {B} image embeddings')
        # a constant dense prompt (every pixel of every entry the same vector) keeps the per-image fast path; one host read
        const = bool((d == d[:1, :1, :1]).all())
        if const:
            masks, iou = self.decode(image_embeddings, image_positional_embeddings, sparse.contiguous(),
                                     d[0, 0, 0].contiguous(), roi_img, multimask_output=bool(multimask_output),
                                     attn_bias=bias, target_rows=te, **head_kw)
        else:
            emb = nhwc_view(image_embeddings)
            _, h, w, C = emb.shape
            # HF:499, one dense source per image (a [1, ..] dense prompt repeats over the batch: row % (h w))
            src = ops.add_rows(emb.reshape(B * h * w, C).contiguous(), d.reshape(-1, C).contiguous())
            masks, iou = self.decode(None, image_positional_embeddings, sparse.contiguous(), None, roi_img,
                                     src_rows=src, hw=(h, w), multimask_output=bool(multimask_output), attn_bias=bias,
                                     target_rows=te, **head_kw)
        C, mh, mw = masks.shape[1:]
        return masks.reshape(B, Pb, C, mh, mw), iou.reshape(B, Pb, iou.shape[1]), None


def hq_conv_weights(conv1_w, conv2_w):
    """SAM-HQ's two 3 x 3 convolutions in the forms rsp_sam_hq_mask takes: mask_conv1 [64, 32, 3, 3] -> PackedWeight
    [64, (tap = 3 ky + kx, ci) = 288]; mask_conv2 [32, 64, 3, 3] -> fp32 [tap, ci, c] = [9, 64, 32]"""
    w1 = ops.PackedWeight(conv1_w.detach().permute(0, 2, 3, 1).reshape(conv1_w.shape[0], -1))
    wf = conv2_w.detach().to(torch.float32).permute(2, 3, 1, 0).reshape(9, conv2_w.shape[1], conv2_w.shape[0]).contiguous()
    return w1, wf


class SamHQMaskDecoderHIP(SamMaskDecoderHIP):
    """HF `SamHQMaskDecoder` (transformers models/sam_hq/modeling_sam_hq.py:869-1067, "HQ:" below) in its parameter layout:
    SAM's decoder with one more output token (tokens = [iou, mask x4, hq, sparse...]) whose hyper-network vector multiplies
    `mask_conv2(GELU(LN(mask_conv1(upscaled)))) + hq_features`.  The whole tail -- second ConvTranspose, both 3 x 3
    convolutions, LayerNorm, GELUs, the HQ product and SAM's own mask products -- is one kernel launch per decode
    (csrc/sam_hq.hip); nothing of shape [R, 4g, 4g, 32 | 64] is stored.  `hq_features` [B, 4g, 4g, 32] depend on the image
    alone (four ConvTransposes over the image embedding and the early ViT feature, HQ:964-975): `hq_features()`, once per
    image.  What is upscaled follows HF's code, not SAM's: see `_heads` ("SAM-HQ")."""

    def __init__(self, vit_dim=768):
        super().__init__()
        self.vit_dim = vit_dim
        add_param(self, 'hq_token.weight', (1, HID))
        for l in ('proj_in', 'layers.0'):
            _add_linear(self, 'hq_mask_mlp.' + l, HID, HID)
        _add_linear(self, 'hq_mask_mlp.proj_out', HID // 8, HID)
        for name, cin, cmid in (('compress_vit', vit_dim, HID), ('encoder', HID, HID // 4)):
            add_param(self, f'{name}_conv1.weight', (cin, cmid, 2, 2))
            add_param(self, f'{name}_conv1.bias', (cmid,))
            _add_ln(self, f'{name}_norm', cmid)
            add_param(self, f'{name}_conv2.weight', (cmid, HID // 8, 2, 2))
            add_param(self, f'{name}_conv2.bias', (HID // 8,))
        add_param(self, 'mask_conv1.weight', (HID // 4, HID // 8, 3, 3))
        add_param(self, 'mask_conv1.bias', (HID // 4,))
        _add_ln(self, 'mask_norm', HID // 4)
        add_param(self, 'mask_conv2.weight', (HID // 8, HID // 4, 3, 3))
        add_param(self, 'mask_conv2.bias', (HID // 8,))
        self.n_output_tokens = 2 + N_MASK_TOKENS
        self.hq_feature_calls = 0            # tests: how often the per-image features were computed

    def _pack(self):
        from .necks import convt_weights4
        super()._pack()
        P = self._packed
        for l in ('proj_in', 'layers.0', 'proj_out'):
            P[f'hq.{l}'] = self._pw(f'hq_mask_mlp.{l}')
        for key, name in (('enc1', 'encoder_conv1'), ('enc2', 'encoder_conv2'), ('vit1', 'compress_vit_conv1'),
                          ('vit2', 'compress_vit_conv2')):
            m = getattr(self, name)
            P[key] = convt_weights4(m.weight, m.bias)
        P['hq_w1'], P['hq_wf'] = hq_conv_weights(self.mask_conv1.weight, self.mask_conv2.weight)

    def _output_tokens(self):
        """[iou, mask x4, hq] (HQ:977)"""
        return torch.cat([self.iou_token.weight, self.mask_tokens.weight, self.hq_token.weight], 0)

    @torch.no_grad()
    def hq_features(self, image_embeddings, vit_features=None):
        """HQ:964-975: encoder_conv2(GELU(LN(encoder_conv1(image_embeddings)))) [+ the same chain of compress_vit_* over
        vit_features [B, g, g, vit_dim], the ViT's hidden state after its first global-attention layer] -> fp32 [B, 4g, 4g, 32].
        image_embeddings [B, 256, g, g] WITHOUT the dense prompt."""
        if self._packed is None:
            self._pack()
        P = self._packed
        self.hq_feature_calls += 1
        emb = nhwc_view(image_embeddings)
        B, h, w, _ = emb.shape
        e = ops.conv_transpose2x2(emb, *P['enc1'], act=ops.ACT_GELU, ln=(self.encoder_norm.weight, self.encoder_norm.bias, 1e-6))
        f = ops.conv_transpose2x2(e, *P['enc2'])
        if vit_features is not None:
            if tuple(vit_features.shape) != (B, h, w, self.vit_dim):
                raise ValueError(f'intermediate embedding: expected [{B}, {h}, {w}, {self.vit_dim}], got {tuple(vit_features.shape)}')
            c = ops.conv_transpose2x2(vit_features.to(torch.float32).contiguous(), *P['vit1'])
            c = ops.layernorm(c.view(B * 4 * h * w, HID), self.compress_vit_norm.weight, self.compress_vit_norm.bias, 1e-6,
                              act=ops.ACT_GELU, planes=True, f32=False)
            c = ops.conv_transpose2x2(c.view(B, 2 * h, 2 * w, HID), *P['vit2'])
            f = ops.add_rows(f.view(-1, HID // 8), c.view(-1, HID // 8)).view(B, 4 * h, 4 * w, HID // 8)
        return f

    def decode(self, *args, hq_features=None, hq_token_only=False, src_is_identity=False, **kw):
        """`SamMaskDecoderHIP.decode` + hq_features fp32 [B | sources, 4h, 4w, 32] (row = the prompt set's `roi_img` entry) and
        hq_token_only.  Returns (masks, iou): masks_sam + mask_hq [R, 3 | 1, 4h, 4w], or mask_hq alone [R, 1, 4h, 4w] with
        hq_token_only; with multimask_output the three SAM masks and iou [R, 3] are ordered by predicted IoU, descending (HQ:1042-1055)."""
        if hq_features is None:
            raise ValueError('SamHQMaskDecoderHIP.decode needs hq_features (see hq_features())')
        if src_is_identity:
            # (a chunk of that form renumbers its sources from 0, which would index hq_features with chunk-local rows)
            raise NotImplementedError('SamHQMaskDecoderHIP.decode: src_is_identity (one source per prompt set) is not taken')
        return super().decode(*args, hq_features=hq_features, hq_token_only=bool(hq_token_only), **kw)

    def _heads(self, q3, hold, R, h, w, multimask_output, want_iou, stages, roi_img, src, hq_features=None, hq_token_only=False):
        """HQ:999-1065.  What is upscaled is NOT the transformer's keys: HF's HQ decoder binds the transformer's second result
        to a name it overwrites (HQ:989, 996), so HQ:999-1005 upscale the tensor the transformer was GIVEN -- image embedding
        + dense prompt, repeated per prompt set -- after `transpose(2, 3).reshape(.., h, w)`, which on that 4-D tensor is a
        spatial transpose (on SAM's [.., N, C] keys the same line restores NCHW).  Both are reproduced: this decoder computes
        what `SamHQModel` computes.  The upscaled embedding therefore depends on the SOURCE (image + dense prompt) alone; its
        first stage runs once per source and the kernel reads it through the prompt set -> source map."""
        P = self._packed
        hold.pop()                                                                      # the keys are not read (see above)
        feat, hq_only = hq_features, hq_token_only
        if h != w:
            raise NotImplementedError(f'SamHQMaskDecoderHIP: a {h} x {w} embedding grid (HQ:999 is a spatial transpose only '
                                      'for a square grid)')
        if tuple(feat.shape[1:]) != (4 * h, 4 * w, HID // 8):
            raise ValueError(f'hq_features: expected [*, {4 * h}, {4 * w}, {HID // 8}], got {tuple(feat.shape)}')
        S = src.shape[0] // (h * w)
        src_t = src.view(S, h, w, HID).transpose(1, 2).contiguous()
        up = ops.conv_transpose2x2(src_t, *P['up1'], act=ops.ACT_GELU,
                                   ln=(self.upscale_layer_norm.weight, self.upscale_layer_norm.bias, 1e-6))   # [S, 2h, 2w, 64] planes
        io = self._iou_head(q3)                                                         # [R, 4]
        hy_hq = self._hyper(q3, N_MASK_TOKENS, 'hq')
        if multimask_output:
            # HQ:1042-1055: tokens 1..3 by predicted IoU, descending (a tie goes to the lower token).  The ORDER is applied to the
            # hyper-network vectors, so the masks are produced in their final places: no gather over [R, 3, 4h, 4w], no host read
            iou, order = torch.sort(io[:, 1:4], dim=1, descending=True, stable=True)
            hy = torch.stack([self._hyper(q3, i) for i in (1, 2, 3)], 1)
            hy = torch.gather(hy, 1, order.unsqueeze(-1).expand(-1, -1, hy.shape[-1])).contiguous()
        else:
            iou = io[:, 0:1]
            hy = self._hyper(q3, 0).unsqueeze(1).contiguous()
        if stages is not None:
            stages.update(up=up, hyper_hq=hy_hq, hyper=[hy[:, j] for j in range(hy.shape[1])])
        self._last_stages = stages
        rmap = roi_img.to(torch.int32).contiguous()
        # one launch: mask_hq, and (unless hq_token_only) SAM's masks + mask_hq from the same upscaled tile (HQ:1032-1065)
        res = ops.sam_hq_mask(up, P['up2'][0], P['up2'][1], P['hq_w1'], self.mask_conv1.bias, self.mask_norm.weight,
                              self.mask_norm.bias, 1e-6, P['hq_wf'], self.mask_conv2.bias, hy_hq, feat.contiguous(), rmap,
                              up_map=rmap, hyper_sam=None if hq_only else hy)
        masks = res.view(R, 1, 4 * h, 4 * w) if hq_only else res[1]
        return masks, (iou if want_iou else None)

    def forward(self, image_embeddings, image_positional_embeddings, sparse_prompt_embeddings, dense_prompt_embeddings,
                multimask_output=False, hq_token_only=False, intermediate_embeddings=None, attention_similarity=None,
                target_embedding=None, hq_features=None):
        """HF signature (HQ:915-926) + hq_features: the result of `hq_features()` for these embeddings, when the caller kept it.
        Returns (masks [B, Pb, C, 4h, 4w], iou [B, Pb, 3 | 1], None)."""
        if hq_features is None:
            vit = intermediate_embeddings[0] if intermediate_embeddings is not None and len(intermediate_embeddings) > 0 else None
            hq_features = self.hq_features(image_embeddings, vit)
        return super().forward(image_embeddings, image_positional_embeddings, sparse_prompt_embeddings,
                               dense_prompt_embeddings, multimask_output=multimask_output,
                               attention_similarity=attention_similarity, target_embedding=target_embedding,
                               hq_features=hq_features, hq_token_only=bool(hq_token_only))


@MODELS.register_module()
class RSSamMaskDecoder(HIPModule):
    def __init__(self, hf_pretrain_name, extra_config=None, init_cfg=None):
        super().__init__()
        self.mask_decoder = SamMaskDecoderHIP()

    def forward(self, *args, **kwargs):
        return self.mask_decoder(*args, **kwargs)


def image_wide_table(G, size):
    """models.py:85-95 + HF:552-566 for the [2, F] Gaussian matrix G: logical [1, 2F, size, size] table on G's device
    (constant preparation on the host, exactly the reference's fp32 expression)."""
    g = G.detach().float().cpu()
    grid = torch.ones((size, size), dtype=torch.float32)
    y = (grid.cumsum(dim=0) - 0.5) / size
    x = (grid.cumsum(dim=1) - 0.5) / size
    c = torch.stack([x, y], dim=-1)
    c = 2 * c - 1
    c = c @ g
    c = 2 * np.pi * c
    pe = torch.cat([torch.sin(c), torch.cos(c)], dim=-1)          # [size, size, 2F] == NHWC
    return nchw_view(pe.unsqueeze(0).contiguous().to(G.device))


class _PosEmb(HIPModule):
    def __init__(self):
        super().__init__()
        add_param(self, 'positional_embedding', (2, 128))


@MODELS.register_module()
class RSSamPositionalEmbedding(HIPModule):
    """models.py:744-759.  The image-wide table (models.py:85-95 + HF:552-566) depends only on the
    [2,128] Gaussian matrix, so it is computed once per (size, weights) on the host at pack time
    (constant preparation, exactly the reference's fp32 expression) and kept on the device."""

    def __init__(self, hf_pretrain_name, extra_config=None, init_cfg=None):
        super().__init__()
        self.shared_image_embedding = _PosEmb()
        self._cache = {}

    def _apply(self, fn, *a, **kw):
        self._cache = {}
        return super()._apply(fn, *a, **kw)

    def image_wide(self, size):
        G = self.shared_image_embedding.positional_embedding
        key = (size, G.data_ptr(), G._version)
        if key not in self._cache:
            self._cache = {key: image_wide_table(G, size)}
        return self._cache[key]

    def forward(self, input_coords, input_shape=None):
        """models.py:756-759 -> HF SamPositionalEmbedding.forward (HF:552-566): input_coords [..., 2] (x, y; HF indexes a
        4-D tensor), divided by input_shape = (h, w) when given, -> [..., 256] on the device (rsp_sam_embed_prompts without
        labels: no pixel-centre shift, no type embedding)."""
        c = input_coords.to(torch.float32)
        lead = tuple(c.shape[:-1])
        out = ops.sam_embed_prompts(c.reshape(1, -1, 2), None, None, False, self.shared_image_embedding.positional_embedding,
                                    None, None, (1, 1) if input_shape is None else input_shape)
        return out.view(*lead, out.shape[-1])


class _PromptEncoder(HIPModule):
    def __init__(self):
        super().__init__()
        add_param(self, 'no_mask_embed.weight', (1, HID))
        # SamMaskEmbedding (HF:569-593), used by the query variant's sam_mask_embed (models.py:305)
        add_param(self, 'mask_embed.conv1.weight', (4, 1, 2, 2))
        add_param(self, 'mask_embed.conv1.bias', (4,))
        add_param(self, 'mask_embed.conv2.weight', (16, 4, 2, 2))
        add_param(self, 'mask_embed.conv2.bias', (16,))
        add_param(self, 'mask_embed.conv3.weight', (HID, 16, 1, 1))
        add_param(self, 'mask_embed.conv3.bias', (HID,))
        _add_ln(self, 'mask_embed.layer_norm1', 4)
        _add_ln(self, 'mask_embed.layer_norm2', 16)


@MODELS.register_module()
class RSSamPromptEncoder(HIPModule):
    """models.py:881-896; only `no_mask_embed` / `mask_embed` are used downstream (:1635, :305)."""

    def __init__(self, hf_pretrain_name, extra_config=None, init_cfg=None):
        super().__init__()
        self.prompt_encoder = _PromptEncoder()

    def forward(self, *args, **kwargs):
        raise NotImplementedError('RSSamPromptEncoder.forward: this module holds the reduced parameter set RSPrompter '
                                  'borrows (no_mask_embed / mask_embed); the full prompt encoder (points, boxes, masks) '
                                  'is SamModelHIP.get_prompt_embeddings (rsprompter_amd/samdet.py)')
