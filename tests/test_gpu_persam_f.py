"""-m gpu: PerSAM-F, the fitted mask weights of one-shot segmentation ("PerSAM-F") -- the fused loss / gradient
kernel and the on-device AdamW fit against torch autograd in fp64 over the materialised fields
(`mask_post_logits(want_val=True)`), under a tolerance MEASURED per case: twice the distance between the same autograd run in
fp32 and in fp64; `apis.PerSamF`'s host flow around a stub of `SamModelHIP`; and the live ViT-B procedure against
`oracle_persam_f`, the specification written as HF calls + torch.  The check_* functions are shared with
tests/test_persam_f_cpu.py, where `ops` is the emulated module and the device the CPU."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_gpu_persam import (E_SIM, LOCATE_CASES, REF, TARGETS, TOL_IOU, TOL_LOGITS, UNDECIDED_GAP, RectSam,  # noqa: E402
                             rect_image)
from test_gpu_sam_multicrop import _ReadCounter, _post_s, _shape, _test_image  # noqa: E402
from test_gpu_sam_prompts import _err, _hf_helpers, _models, _smooth  # noqa: E402

ALPHA = 0.25
W_THIRD = float(torch.tensor(1 / 3, dtype=torch.float32))                # the fit starts at fp32 1 / 3
WEIGHT_CASES = ((W_THIRD, W_THIRD), (0.7, -0.2), (0.8, 0.6))             # 1 / 3, well off it, and w0 = -0.4


# ------------------------------------------------------------------------------------------------- the oracle: autograd
def loss_of(Fk, t, w12, alpha=ALPHA):
    """the issue's formulas in torch: Fk [3, H, W] fields, t [H, W] in {0, 1} (Fk's dtype), w12 [2] = (w1, w2)"""
    z = (1 - w12[0] - w12[1]) * Fk[0] + w12[0] * Fk[1] + w12[1] * Fk[2]
    p = z.sigmoid()
    dice = 1 - (2 * (p * t).sum() + 1) / (p.sum() + t.sum() + 1)
    ce = F.binary_cross_entropy_with_logits(z, t, reduction='none')
    p_t = p * t + (1 - p) * (1 - t)
    a_t = alpha * t + (1 - alpha) * (1 - t)
    return dice + (a_t * ce * (1 - p_t) ** 2).mean()


def autograd_loss_grad(Fk, t, w12, dtype):
    """fp64 [3] = loss, g1, g2 by autograd in `dtype`; w12: two Python floats (fp32 values)"""
    w = torch.tensor(w12, dtype=dtype, device=Fk.device, requires_grad=True)
    with torch.enable_grad():
        loss = loss_of(Fk.to(dtype), t.to(dtype), w)
    loss.backward()
    return torch.cat([loss.detach().reshape(1), w.grad]).double().cpu()


def autograd_fit(Fk, t, epochs, dtype, lr=1e-3):
    """torch AdamW + CosineAnnealingLR + autograd in `dtype`: (weights fp64 [3] = w0, w1, w2; history fp64 [epochs, 3])"""
    Fk, t = Fk.to(dtype), t.to(dtype)
    w = torch.tensor([W_THIRD, W_THIRD], dtype=dtype, device=Fk.device, requires_grad=True)
    opt = torch.optim.AdamW([w], lr=lr, betas=(0.9, 0.999), eps=1e-4, weight_decay=0.01)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=epochs)
    hist = torch.empty(epochs, 3, dtype=dtype, device=Fk.device)
    for e in range(epochs):
        opt.zero_grad()
        with torch.enable_grad():
            loss = loss_of(Fk, t, w)
        loss.backward()
        hist[e, 0], hist[e, 1:] = loss.detach(), w.grad
        opt.step()
        sch.step()
    wd = w.detach().double()
    return torch.stack([1 - wd[0] - wd[1], wd[0], wd[1]]).cpu(), hist.double().cpu()


def fit_problems(ops, dev, k, img, crop, out, base, seed):
    """k problems: smooth logits of amplitude ~10 [k, 3, base, base] and their materialised fields [k, 3, H, W]; the ground
    truths are a smooth blob (where a fixed mix of the fields is positive: the fit has somewhere to go), then an empty and a
    full mask"""
    g = torch.Generator().manual_seed(seed)
    low = (_smooth(g, k, 3, base, base, k=5) * 20).contiguous().to(dev)
    val = ops.mask_post_logits(low.reshape(k * 3, base, base), img, crop, out, 0.0, want_val=True)[1].reshape(k, 3, out[0], out[1])
    gt = torch.zeros(k, out[0], out[1], dtype=torch.bool, device=val.device)
    gt[0] = (0.05 * val[0, 0] + 0.8 * val[0, 1] + 0.15 * val[0, 2]) > 2.0
    if k > 2:
        gt[2] = True
    return low, val, gt


# ------------------------------------------------------------------------------------------------- 1. the feature is there
def check_refusals(lib, dev=None):
    """-1 from all three entry points on every refused argument.  With `dev` (a device, or the CPU with the emulator behind
    `lib`) the buffers live there and the unaltered call returns 0, so that every -1 below is the refusal of ONE argument;
    without it nothing is launched"""
    h = w = 8
    geom = dict(Hb=32, Wb=32, ch=32, cw=24, oh=20, ow=15)
    k, epochs = 2, 3
    valid = dev is not None
    n = lib.rsp_persam_f_workspace_bytes(k, geom['oh'], geom['ow'], epochs)
    assert n > 0 and n % 8 == 0
    bufs = [torch.zeros(k * 3 * h * w), torch.zeros(k * geom['oh'] * geom['ow'], dtype=torch.uint8), torch.full((k * 3,), 1 / 3),
            torch.zeros(k * 3, dtype=torch.float64), torch.zeros(k * epochs * 3, dtype=torch.float64), torch.zeros(n // 8, dtype=torch.int64)]
    low, gt, wts, out, hist, ws = [t.to(dev) if valid else t for t in bufs]
    A = lambda t: t.data_ptr()                                               # noqa: E731

    def lg(**o):
        a = dict(low=A(low), gt=A(gt), k=k, h=h, w=w, **geom, weights=A(wts), ws=A(ws), n=n, out=A(out))
        a.update(o)
        return lib.rsp_persam_f_loss_grad(a['low'], a['gt'], a['k'], a['h'], a['w'], a['Hb'], a['Wb'], a['ch'], a['cw'], a['oh'], a['ow'],
                                          a['weights'], ALPHA, a['ws'], a['n'], a['out'], None)

    def fit(**o):
        a = dict(low=A(low), gt=A(gt), k=k, h=h, w=w, **geom, epochs=epochs, ws=A(ws), n=n, weights=A(wts), hist=A(hist))
        a.update(o)
        return lib.rsp_persam_f_fit(a['low'], a['gt'], a['k'], a['h'], a['w'], a['Hb'], a['Wb'], a['ch'], a['cw'], a['oh'], a['ow'],
                                    a['epochs'], 1e-3, 0.9, 0.999, 1e-4, 0.01, ALPHA, a['ws'], a['n'], a['weights'], a['hist'], None)
    if valid:
        assert lg() == 0 and fit() == 0 and fit(hist=None) == 0
    huge = dict(Hb=65536, Wb=65536, ch=65536, cw=32768, oh=65536, ow=32768)              # out_h * out_w = 2^31
    bad = [dict(k=0), dict(k=-1), dict(h=0), dict(ch=33), dict(cw=0), dict(ow=0), dict(oh=-2), huge, dict(low=None), dict(gt=None),
           dict(weights=None), dict(ws=None), dict(n=n - 8), dict(n=0)]
    for o in bad:
        assert lg(**o) == -1, ('loss_grad', o)
        assert fit(**o) == -1, ('fit', o)
    assert lg(out=None) == -1 and fit(epochs=0) == -1 and fit(epochs=-5) == -1
    wb = lib.rsp_persam_f_workspace_bytes
    assert wb(0, 20, 15, 3) == -1 and wb(2, 20, 15, 0) == -1 and wb(2, 0, 15, 3) == -1 and wb(2, 20, -1, 3) == -1
    assert wb(1, 65536, 32768, 1) == -1 and wb(1, 1024, 1024, 1000) > 0
    # the workspace does not depend on the number of epochs (nothing per epoch is kept)
    assert wb(2, 20, 15, 1000) == n


# ------------------------------------------------------------------------------------------------- 2. loss and gradient
def check_loss_grad(ops, dev, img, crop, out, base, seed=120):
    """k = 1 (blob) and k = 3 (blob, empty, full) at the three weight pairs, against autograd in fp64; the tolerance of a case
    is twice the distance of the same autograd in fp32 from it.  Returns the worst (kernel distance, fp32 distance)."""
    worst = (0.0, 0.0)
    for k in (1, 3):
        low, val, gt = fit_problems(ops, dev, k, img, crop, out, base, seed + k)
        for w12 in WEIGHT_CASES:
            wt = torch.tensor([w12] * k, dtype=torch.float32).to(dev)
            got = ops.persam_f_loss_grad(low, gt, img, crop, out, wt)
            again = ops.persam_f_loss_grad(low, gt, img, crop, out, wt)
            assert got.dtype == torch.float64 and tuple(got.shape) == (k, 3) and torch.equal(got, again)
            w32 = tuple(float(v) for v in wt[0].cpu())
            for m in range(k):
                r64 = autograd_loss_grad(val[m], gt[m], w32, torch.float64)
                r32 = autograd_loss_grad(val[m], gt[m], w32, torch.float32)
                d32, d = float((r32 - r64).abs().max()), float((got[m].cpu() - r64).abs().max())
                kind = ('blob', 'empty', 'full')[m]
                print(f'persam_f_loss_grad {img} / {crop} / {out} k={k} problem {m} ({kind}, {int(gt[m].sum())} px) w=({w32[0]:.3f}, '
                      f'{w32[1]:.3f}): loss {float(r64[0]):.6f} grad ({float(r64[1]):+.4e}, {float(r64[2]):+.4e}); kernel {d:.2e}, '
                      f'fp32 autograd {d32:.2e} from fp64 autograd')
                assert d <= 2 * d32, (k, m, w12, d, d32)
                if d > worst[0]:
                    worst = (d, d32)
    return worst


# ------------------------------------------------------------------------------------------------- 3. the fit
def check_fit(ops, dev, img, crop, out, base, epochs, seed=130, count_reads=True):
    """one problem (the blob): final weights and every epoch's loss and gradients against the fp64 oracle within twice the
    fp32 oracle's distance from it; the oracle alone moves by more than 100 x that distance; row 0 of the history is
    loss_grad at 1 / 3 bit for bit; two fits give equal bits; no host read inside ops.persam_f_fit"""
    low, val, gt = fit_problems(ops, dev, 1, img, crop, out, base, seed)
    w64, h64 = autograd_fit(val[0], gt[0], epochs, torch.float64)
    w32, h32 = autograd_fit(val[0], gt[0], epochs, torch.float32)
    dw32, dh32 = float((w32 - w64).abs().max()), float((h32 - h64).abs().max())
    start = torch.tensor([1 - 2 * W_THIRD, W_THIRD, W_THIRD], dtype=torch.float64)
    moved = float((w64 - start).abs().max())
    print(f'persam_f_fit {img} / {crop} / {out}, {epochs} epochs: oracle weights {w64.tolist()} moved {moved:.3e} from 1/3; loss '
          f'{float(h64[0, 0]):.5f} -> {float(h64[-1, 0]):.5f}; fp32 oracle from fp64 oracle: weights {dw32:.2e}, history {dh32:.2e}')
    assert moved > 100 * dw32, 'the oracle alone: a fit that does nothing must not pass'
    with _ReadCounter() as rc:
        w, hist = ops.persam_f_fit(low, gt, img, crop, out, epochs=epochs, want_history=True)
    assert rc.n == {} or not count_reads, rc.n
    w_b, hist_b = ops.persam_f_fit(low, gt, img, crop, out, epochs=epochs, want_history=True)
    w_c = ops.persam_f_fit(low, gt, img, crop, out, epochs=epochs)
    assert torch.equal(w, w_b) and torch.equal(hist, hist_b) and torch.equal(w, w_c)
    assert w.dtype == torch.float32 and tuple(w.shape) == (1, 3) and hist.dtype == torch.float64 and tuple(hist.shape) == (1, epochs, 3)
    first = ops.persam_f_loss_grad(low, gt, img, crop, out, torch.tensor([[W_THIRD, W_THIRD]], dtype=torch.float32).to(dev))
    assert torch.equal(hist[:, 0], first)
    dw, dh = float((w[0].cpu().double() - w64).abs().max()), float((hist[0].cpu() - h64).abs().max())
    print(f'   kernel from fp64 oracle: weights {dw:.2e} (bound {2 * dw32:.2e}), history {dh:.2e} (bound {2 * dh32:.2e}); '
          f'weights {w[0].tolist()}')
    assert dw <= 2 * dw32 and dh <= 2 * dh32, (dw, dw32, dh, dh32)
    return dw, dw32, dh, dh32


# ------------------------------------------------------------------------------------------------- 4. host flow, stub
class RectSamF(RectSam):
    """`RectSam` speaking PerSAM-F's protocol: pass 1 = one positive point, three masks, no hooks; passes 2 and 3 = the point +
    a box + `input_masks`, three masks"""
    IOU1 = (0.60, 0.70, 0.65)

    def forward(self, image_embeddings=None, input_points=None, input_labels=None, input_boxes=None, input_masks=None,
                multimask_output=True, attention_similarity=None, target_embedding=None):
        B = image_embeddings.shape[0]
        gs = self.vision_encoder.grid
        assert tuple(input_points.shape) == (B, 1, 1, 2) and input_labels.tolist() == [[[1]]] * B
        assert multimask_output is True and attention_similarity is None and target_embedding is None
        if input_masks is None:
            stage = 1
            assert input_boxes is None
        else:
            stage = 2 if self.calls[-1]['stage'] == 1 else 3
            assert tuple(input_masks.shape) == (B, 1, 4 * gs, 4 * gs) and tuple(input_boxes.shape) == (B, 1, 4)
        low = self.low_of(image_embeddings, True)
        iou = torch.tensor({1: self.IOU1, 2: self.IOU2, 3: self.IOU3}[stage], device=self.dev).view(1, 1, -1).expand(B, 1, -1)
        self.calls.append(dict(stage=stage, B=B, points=input_points, masks=input_masks, boxes=input_boxes, low=low))
        import types
        return types.SimpleNamespace(pred_masks=low, iou_scores=iou.contiguous())


def check_host_flow_f(ops, dev, S, gs, sizes, scale, epochs=12):
    """`PerSamF` around the stub: the constructor's one decoder pass and fit, then grouping by size, batching, input order,
    what each pass is handed (the weighted sum, its box, the best of three, its box), the result dict, and that `weights` is
    passed through (they are replaced after the fit by a triple nothing else could produce)"""
    from rsprompter_amd.apis import PerSamF
    from rsprompter_amd.sam_prompts import preprocess_shape
    ip = _hf_helpers()
    A, Bz = sizes
    sc = lambda r: None if r is None else [int(v * scale) for v in r]       # noqa: E731
    scene = [(A, sc([50, 10, 80, 40])), (Bz, sc([8, 20, 38, 44])), (A, sc([6, 30, 40, 56])), (A, None), (Bz, sc([30, 4, 66, 30]))]
    sam = RectSamF(ops, dev, S, gs)
    ref = rect_image(A, sc([20, 15, 60, 45]))
    ref_mask = ref[:, :, 0] > 0
    with pytest.raises(ValueError, match='no cell'):
        PerSamF(sam, ref, torch.zeros(A, dtype=torch.bool), epochs=epochs)
    with pytest.raises(ValueError):
        PerSamF(sam, ref, ref_mask[:, :-1], epochs=epochs)
    with pytest.raises(ValueError):
        PerSamF(sam, ref, ref_mask, epochs=0)
    sam.calls.clear()
    ps = PerSamF(sam, ref, ref_mask, epochs=epochs)
    assert [c['stage'] for c in sam.calls] == [1] and sam.calls[0]['B'] == 1          # ONE decoder pass on the reference
    assert tuple(ps.target_feature.shape) == (256,) and tuple(ps.weights.shape) == (3,) and ps.weights.dtype == torch.float32
    assert tuple(ps.loss_history.shape) == (epochs, 3) and ps.loss_history.dtype == torch.float64 and ps.cells > 0
    assert float((ps.target_feature.cpu() @ sam.u.cpu())) > 0.9 and abs(float(ps.target_feature.norm()) - 1) < 1e-6
    nhw_ref = preprocess_shape(A, S)
    want_w, want_h = ops.persam_f_fit(sam.calls[0]['low'][:, 0].contiguous(), ref_mask[None].to(dev), (S, S), nhw_ref, A, epochs=epochs,
                                      want_history=True)
    assert torch.equal(ps.weights, want_w[0]) and torch.equal(ps.loss_history, want_h[0])
    assert abs(float(ps.weights.sum()) - 1) < 1e-6 and float((ps.weights - 1 / 3).abs().max()) > 1e-4
    ps.weights = torch.tensor([0.25, 0.5625, 0.1875]).to(dev)                          # passed through from here on
    sam.batches.clear()
    sam.calls.clear()
    imgs = [rect_image(hw, r) for hw, r in scene]
    st = {}
    res = ps.segment(imgs, batch_size=2, output='rle', _stages=st)
    dense = ps.segment(imgs, batch_size=8, output='dense')
    assert sam.batches == [2, 1, 2, 3, 2], sam.batches
    assert [c['stage'] for c in sam.calls[:9]] == [1, 2, 3] * 3
    order = [0, 2, 3, 1, 4]
    row = 0
    wv = ps.weights.view(1, 3, 1, 1)
    for bi, stg in enumerate(st['batches']):
        c1, c2, c3 = sam.calls[3 * bi:3 * bi + 3]
        low_w = (c1['low'][:, 0] * wv).sum(1)
        assert torch.equal(c2['masks'][:, 0], low_w) and torch.equal(stg['low_w'], low_w)     # pass 2 refines the weighted sum
        assert stg['best2'].tolist() == [1] * c1['B'] and stg['best3'].tolist() == [0] * c1['B']
        assert torch.equal(c3['masks'][:, 0], c2['low'][:, 0, 1])                             # pass 3 the best of pass 2
        for b in range(c1['B']):
            i = order[row]
            hw, rect = scene[i]
            H, W = hw
            nhw = preprocess_shape(hw, S)
            r = res[i]
            assert set(r) == {'mask', 'score', 'bbox', 'points', 'point_sims', 'weights'}
            assert r['weights'] == [0.25, 0.5625, 0.1875] == dense[i]['weights']
            assert len(r['points']) == 1 and len(r['point_sims']) == 1
            field = _post_s(stg['low_sim'][b:b + 1].cpu(), S, nhw, hw)[0]
            (xp, yp), = r['points']
            want_pts = ip._normalize_coordinates(S, np.array(r['points'], dtype=np.float64), hw)
            assert c1['points'][b, 0].tolist() == torch.from_numpy(want_pts).float().tolist()
            for cc, lw, key in ((c2, low_w[b:b + 1], 'box1'), (c3, c2['low'][b, 0, 1:2], 'box2')):
                want_box = ip._batched_mask_to_box(_post_s(lw.cpu(), S, nhw, hw) > 0)[0]
                assert stg[key][b].tolist() == want_box.tolist(), (key, stg[key][b].tolist(), want_box.tolist())
                want_in = ip._normalize_coordinates(S, want_box.numpy().astype(np.float64), hw, is_bounding_box=True)
                assert cc['boxes'][b, 0].tolist() == torch.from_numpy(want_in).float().reshape(4).tolist()
            final = _post_s(c3['low'][b, 0, 0:1].cpu(), S, nhw, hw)[0]
            got_mask = dense[i]['mask'].cpu()
            assert tuple(got_mask.shape) == (H, W) and got_mask.dtype == torch.bool
            assert bool(((got_mask != (final > 0)) <= (final.abs() < 1e-4)).all())
            assert r['mask']['size'] == [H, W] and r['mask'] == ip._mask_to_rle(got_mask[None])[0]
            assert r['bbox'] == ip._batched_mask_to_box(got_mask[None])[0].tolist() == dense[i]['bbox']
            assert abs(r['score'] - 0.96) < 1e-6 and r['points'] == dense[i]['points']
            assert float(field[yp, xp]) >= float(field.max()) - 2 * E_SIM and abs(r['point_sims'][0] - float(field.max())) < 2 * E_SIM
            if rect is None:
                assert r['bbox'] == [0, 0, 0, 0] and r['mask']['counts'] == [H * W] and stg['box1'][b].tolist() == [0, 0, 0, 0]
            else:
                x0, y0, x1, y1 = rect
                assert x0 <= xp < x1 and y0 <= yp < y1, (i, r['points'], rect)
                truth = torch.zeros(H, W, dtype=torch.bool)
                truth[y0:y1, x0:x1] = True
                iou = float((got_mask & truth).sum()) / float((got_mask | truth).sum())
                assert iou > 0.5, (i, iou)
            row += 1
    assert row == len(scene)
    one = ps.segment(imgs[0])
    assert isinstance(one, dict) and one['points'] == res[0]['points']
    for bad in (dict(output='png'), dict(batch_size=0)):
        with pytest.raises(ValueError):
            ps.segment(imgs[0], **bad)
    return res


# ------------------------------------------------------------------------------------------------- 5. the procedure against HF
def oracle_fields(hf, E, point, hw, S):
    """one decoder pass of HF at `point` (original pixels), label 1, three masks: (low [3, h, w], iou [3], fields [3, H, W])"""
    ip = _hf_helpers()
    p_in = torch.from_numpy(ip._normalize_coordinates(S, np.array([point], dtype=np.float64), hw)).float()[None, None]
    o = hf(image_embeddings=E, input_points=p_in, input_labels=torch.tensor([[[1]]]), multimask_output=True)
    return o.pred_masks[0, 0], o.iou_scores[0, 0], _post_s(o.pred_masks[0, 0], S, _shape(hw, S), hw), p_in


def oracle_persam_f_ref(hf, S, gs, ref_pv, ref_cells, ref_gt, epochs, fit_dev, dev_point=None, dev_low=None):
    """the specification's "Fit, once per reference" in HF calls + torch; `fit_dev`: where the autograd loop runs (fp64).
    dev_low: the DEVICE's reference logits, for the fit that measures what the embedding distance does to the weights"""
    hw = tuple(ref_gt.shape)
    nhw = _shape(hw, S)
    with torch.no_grad():
        E = hf.get_image_embeddings(ref_pv)
        rows = E[0].permute(1, 2, 0)[ref_cells]                                        # [cells, 256]
        target = rows.mean(0) / 2 + rows.max(0).values / 2
        tf = target / target.norm()
        f = E[0] / E[0].norm(dim=0, keepdim=True)
        sim = (tf[None] @ f.reshape(256, gs * gs)).reshape(1, 1, gs, gs)
        field = _post_s(F.interpolate(sim, scale_factor=4, mode='bilinear')[0], S, nhw, hw)[0]
        imax = int(field.flatten().argmax())
        own = [imax % hw[1], imax // hw[1]]
        low, _, fields, _ = oracle_fields(hf, E, own if dev_point is None else dev_point, hw, S)
    t = ref_gt.to(fit_dev)
    w, hist = autograd_fit(fields.to(fit_dev), t, epochs, torch.float64)
    out = dict(tf=tf, field=field, own=own, low=low, weights=w, hist=hist)
    if dev_low is not None:
        fd = _post_s(dev_low.cpu(), S, nhw, hw).to(fit_dev)
        out['weights_dev_low'], _ = autograd_fit(fd, t, epochs, torch.float64)
        out['weights_dev_low32'], _ = autograd_fit(fd, t, epochs, torch.float32)
    return out


def oracle_persam_f(hf, S, gs, tf, pv, hw, point, weights, box1):
    """the specification's "Segment, per target image" for ONE image; `point` [x+, y+], `weights` fp32 [3] and `box1` (the box
    of the weighted sum, int [4]) are the DEVICE's (box1 None: the oracle's own).  The weighted sum is taken at HIGH
    resolution, as the paper does."""
    ip = _hf_helpers()
    nhw = _shape(hw, S)
    with torch.no_grad():
        E = hf.get_image_embeddings(pv)
        f = E[0] / E[0].norm(dim=0, keepdim=True)
        sim = (tf[None] @ f.reshape(256, gs * gs)).reshape(1, 1, gs, gs)
        low_sim = F.interpolate(sim, scale_factor=4, mode='bilinear')[0]
        field = _post_s(low_sim, S, nhw, hw)[0]
        imax = int(field.flatten().argmax())
        own = [imax % hw[1], imax // hw[1]]
        low1, iou1, fields, p_in = oracle_fields(hf, E, point, hw, S)
        wv = weights.view(3, 1, 1)
        own_box = ip._batched_mask_to_box(((fields * wv).sum(0) > 0)[None])[0]
        low_w = (low1 * wv).sum(0)
        lab = torch.tensor([[[1]]])

        def refine(box, low):
            b_in = torch.from_numpy(ip._normalize_coordinates(S, np.asarray(box, dtype=np.float64), hw, is_bounding_box=True)).float()
            o = hf(image_embeddings=E, input_points=p_in, input_labels=lab, input_boxes=b_in.reshape(1, 1, 4), input_masks=low[None, None],
                   multimask_output=True)
            s = o.iou_scores[0, 0].sort(descending=True).values
            return o.pred_masks[0, 0], o.iou_scores[0, 0], int(o.iou_scores[0, 0].argmax()), float(s[0] - s[1])
        low2, iou2, b2, gap2 = refine(own_box.tolist() if box1 is None else box1, low_w)
        box2 = ip._batched_mask_to_box(_post_s(low2[b2:b2 + 1], S, nhw, hw) > 0)[0]
        low3, iou3, b3, gap3 = refine(box2.tolist(), low2[b2])
        final = _post_s(low3[b3:b3 + 1], S, nhw, hw)[0]
    return dict(sim=sim[0, 0], low_sim=low_sim[0], field=field, own=own, low1=low1, iou1=iou1, low_w=low_w, own_box=own_box, low2=low2,
                iou2=iou2, best2=b2, box2=box2, low3=low3, iou3=iou3, best3=b3, final=final, gap=min(gap2, gap3))


def check_procedure_f(ps, hf, ops, dev, S, gs, ref, ref_mask, imgs, bound_sim, epochs, count_reads=True):
    """see test_procedure_against_the_composition_of_hf; returns (results, stages, the measured weight distances)"""
    from rsprompter_amd.sam_prompts import PIXEL_MEAN, PIXEL_STD, preprocess_shape
    st, reads = {}, {}

    @contextlib.contextmanager
    def phase(name):
        if name == 'transfer':
            reads.setdefault('before_transfer', []).append(dict(rc.n))
        yield
        if name == 'transfer':
            rc.n.clear()
    ps._phase = phase
    with _ReadCounter() as rc:
        res = ps.segment(imgs, batch_size=8, output='dense', _stages=st)
    ps._phase = lambda name: contextlib.nullcontext()
    sizes = []
    for im in imgs:
        if tuple(im.shape[:2]) not in sizes:
            sizes.append(tuple(im.shape[:2]))
    print(f'host reads of segment() before the transfer of each batch: {reads["before_transfer"]}')
    assert len(st['batches']) == len(sizes)
    if count_reads:
        assert reads['before_transfer'] == [{}] * len(sizes)

    def pv_of(img):
        hw = tuple(img.shape[:2])
        return ops.resize_pad(img.to(dev), preprocess_shape(hw, S), (S, S), PIXEL_MEAN, normalise=(PIXEL_MEAN, PIXEL_STD, False))[None].cpu()
    # ---- the reference: target feature, peak, weights
    ref_hw = tuple(ref.shape[:2])
    o_ref = oracle_persam_f_ref(hf, S, gs, pv_of(ref), ps.cell_mask.cpu(), ref_mask != 0, epochs, dev,
                                dev_point=ps.ref_point.cpu().tolist(), dev_low=ps.ref_low_res[0])
    e_t = _err(ps.target_feature, o_ref['tf'])
    xr, yr = ps.ref_point.cpu().tolist()
    d_ref = float(o_ref['field'].max() - o_ref['field'][yr, xr])
    e_low = _err(ps.ref_low_res[0], o_ref['low'])
    w_dev = ps.weights.cpu().double()
    d_fit = float((w_dev - o_ref['weights_dev_low']).abs().max())                      # the fit alone: same logits on both sides
    tol_fit = 2 * float((o_ref['weights_dev_low32'] - o_ref['weights_dev_low']).abs().max())
    effect = float((o_ref['weights_dev_low'] - o_ref['weights']).abs().max())          # what the embedding distance does
    d_all = float((w_dev - o_ref['weights']).abs().max())
    print(f'reference {ref_hw}: target_feature err {e_t:.2e} (bound {bound_sim:.1e}); device peak {[xr, yr]} is {d_ref:.1e} below the '
          f'oracle\'s maximum at {o_ref["own"]}; reference logits err {e_low:.2e}\n   weights: device {w_dev.tolist()}, oracle '
          f'{o_ref["weights"].tolist()}; device from the oracle\'s fit of the DEVICE\'s logits {d_fit:.2e} (bound {tol_fit:.2e}); that '
          f'fit from the oracle\'s own (the embedding distance\'s effect) {effect:.2e}; device from the oracle {d_all:.2e}')
    assert e_t < bound_sim and d_ref <= 2 * E_SIM and e_low < TOL_LOGITS
    assert d_fit <= tol_fit and d_all <= tol_fit + effect
    # ---- the targets: the device's point, weights and first box fed to the oracle
    order = [i for hw in sizes for i, im in enumerate(imgs) if tuple(im.shape[:2]) == hw]
    rows = {k: (bi, b) for k, (bi, b) in zip(order, [(bi, b) for bi, stg in enumerate(st['batches']) for b in range(stg['points'].shape[0])])}
    oracles = {}
    for k in order:
        bi, b = rows[k]
        hw = tuple(imgs[k].shape[:2])
        oracles[k] = oracle_persam_f(hf, S, gs, o_ref['tf'], pv_of(imgs[k]), hw, res[k]['points'][0], ps.weights.cpu(),
                                     st['batches'][bi]['box1'][b].cpu().tolist())
    print('oracle alone: smallest gap between the two best IoU predictions per image', [f"{oracles[i]['gap']:.3g}" for i in sorted(oracles)])
    assert sum(1 for o in oracles.values() if o['gap'] < UNDECIDED_GAP) <= 1, 'the oracle alone: at most one undecided image'
    for k in order:
        bi, b = rows[k]
        stg, r, o = st['batches'][bi], res[k], oracles[k]
        hw = tuple(imgs[k].shape[:2])
        assert r['weights'] == ps.weights.cpu().tolist()
        e_sim, e_ls = _err(stg['sim'][b].view(gs, gs), o['sim']), _err(stg['low_sim'][b], o['low_sim'])
        (xp, yp), = r['points']
        d_peak = float(o['field'].max() - o['field'][yp, xp])
        e1, i1, ew = _err(stg['low1'][b], o['low1']), _err(stg['iou1'][b], o['iou1']), _err(stg['low_w'][b], o['low_w'])
        e2, i2 = _err(stg['low2'][b], o['low2']), _err(stg['iou2'][b], o['iou2'])
        d_box = max(abs(a - c) for a, c in zip(stg['box1'][b].tolist(), o['own_box'].tolist()))
        dec = o['gap'] >= UNDECIDED_GAP
        print(f'image {k} {hw}: sim err {e_sim:.2e} / up-sampled {e_ls:.2e} (bound {bound_sim:.1e}); device peak {[xp, yp]} is {d_peak:.1e} '
              f'below the oracle\'s maximum at {o["own"]}\n   pass 1 err {e1:.2e} / iou {i1:.2e}, weighted sum err {ew:.2e}; first box '
              f'{stg["box1"][b].tolist()} vs the oracle\'s own {o["own_box"].tolist()} (high-resolution sum); pass 2 err {e2:.2e} / iou '
              f'{i2:.2e}; gap {o["gap"]:.3g} ({"decided" if dec else "UNDECIDED"})')
        assert e_sim < bound_sim and e_ls < bound_sim and d_peak <= 2 * E_SIM
        assert e1 < TOL_LOGITS and i1 < TOL_IOU and ew < TOL_LOGITS and d_box <= 1
        assert e2 < TOL_LOGITS and i2 < TOL_IOU
        if dec:
            assert int(stg['best2'][b]) == o['best2'] and stg['box2'][b].tolist() == o['box2'].tolist()
            e3, i3 = _err(stg['low3'][b], o['low3']), _err(stg['iou3'][b], o['iou3'])
            print(f'   pass 3 err {e3:.2e} / iou {i3:.2e}; best-of-three {o["best2"]}, {o["best3"]}; box {o["box2"].tolist()}')
            assert e3 < TOL_LOGITS and i3 < TOL_IOU and int(stg['best3'][b]) == o['best3']
            want, got = o['final'] > 0, r['mask'].cpu()
            iou = float((got & want).sum()) / max(float((got | want).sum()), 1.0)
            assert iou >= 0.999, (k, iou)
            assert abs(r['score'] - float(o['iou3'][o['best3']])) < TOL_IOU
    return res, st, dict(fit=d_fit, tol_fit=tol_fit, effect=effect, all=d_all)


# ------------------------------------------------------------------------------------------------- GPU tests
def test_refusals_with_a_device_behind_them(dev):
    from rsprompter_amd import _lib
    check_refusals(_lib.load(), dev)
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', range(len(LOCATE_CASES)))
def test_loss_and_gradient_against_autograd(dev, case):
    """measured on MI355X (profiles/persam_f/gpu_tests.log): see DESIGN §15, "PerSAM-F" """
    from rsprompter_amd import ops
    img, crop, out = LOCATE_CASES[case]
    check_loss_grad(ops, dev, img, crop, out, 256, seed=120 + 10 * case)


@pytest.mark.parametrize('case', (0, 1))
def test_fit_against_adamw_and_autograd(dev, case):
    """1000 epochs at the strip form (1024 x 1024) and at a generic geometry (600 x 900); the oracle's loop runs on the device"""
    from rsprompter_amd import ops
    img, crop, out = LOCATE_CASES[case]
    check_fit(ops, dev, img, crop, out, 256, 1000, seed=130 + case)


def test_host_flow_around_a_stub(dev):
    from rsprompter_amd import ops
    check_host_flow_f(ops, dev, 1024, 64, ((600, 900), (500, 700)), 10)


def test_procedure_against_the_composition_of_hf(dev):
    """Live ViT-B, seeded weights, one reference, three targets of two sizes, 1000 epochs.  Target feature and similarity
    fields within E_SIM + 1.22e-5 (two ViT-B runs apart), the device's peak within 2 E_SIM of the oracle's maximum; the
    fitted weights within the fit test's tolerance of the oracle's fit of the device's reference logits, and within that plus
    the measured effect of the embedding distance of the oracle's own fit; downstream, with the device's point, weights and
    first box fed to the oracle: first box within one pixel per coordinate of the oracle's own (taken from the weighted sum
    at HIGH resolution), pass logits within 1e-3 and IoU predictions within 2e-3, and on every decided image equal
    best-of-three indices, equal second box and a final mask at IoU >= 0.999 (at most one image undecided, asserted on the
    oracle alone first).  No host read before each batch's transfer."""
    from rsprompter_amd import ops
    from rsprompter_amd.apis import PerSamF
    hf, hip = _models(dev)
    ref = _test_image(REF['hw'], seed=REF['seed'])
    ref_mask = torch.zeros(REF['hw'], dtype=torch.bool)
    ref_mask[REF['rows'][0]:REF['rows'][1], REF['cols'][0]:REF['cols'][1]] = True
    hip.get_image_wide_positional_embeddings()             # the model's own table, built on the host at its first use
    with _ReadCounter() as rc:
        ps = PerSamF(hip, ref, ref_mask)
    print(f'reference: {ps.cells} cells selected; host reads of the constructor {rc.n}')
    assert rc.n == {'item': 1}
    imgs = [_test_image(hw, seed=s) for hw, s in TARGETS[:3]]
    check_procedure_f(ps, hf, ops, dev, 1024, 64, ref, ref_mask, imgs, E_SIM + 1.22e-5, 1000)
