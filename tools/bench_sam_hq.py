"""SAM-HQ on the MI355X (DESIGN §15 "SAM-HQ"): device-event timings, alternating the two sides of every comparison in one run.

  (a) the mask decoder for --prompts prompt sets at a 64 x 64 grid: SamMaskDecoderHIP against SamHQMaskDecoderHIP (one
      mask and three masks; the HQ side's per-image hq_features are given, as in a SamSession);
  (b) rsp_sam_hq_mask alone against the same function composed from the package's older kernels
      (tests/_sam_hq_ref.kernel_composed: conv_transpose2x2 -> gemm(conv=(3, 1, 1)) -> layernorm -> gemm(conv) -> dot),
      the composition chunked over the prompt sets so that its [chunk, 256, 256, 64] tensors fit.

    python tools/bench_sam_hq.py [--prompts 1024] [--kernel-prompts 256] [--chunk 8] [--reps 10] [--out FILE]
prints one JSON line (and writes it, indented, to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def alternate(fns, reps, warm=2):
    """{name: [ms]} -- the functions take turns inside every repetition"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), reps=reps)
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--prompts', type=int, default=1024)
    ap.add_argument('--kernel-prompts', type=int, default=256)
    ap.add_argument('--chunk', type=int, default=8)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sam_hq.py needs the GPU')
    import _sam_hq_ref as ref
    from rsprompter_amd import ops
    from rsprompter_amd.sam_decoder import SamHQMaskDecoderHIP, SamMaskDecoderHIP
    from rsprompter_amd.synth import synth_state_dict
    dev = torch.device('cuda:0')
    g, R = 64, a.prompts
    hq = SamHQMaskDecoderHIP()
    sd = synth_state_dict(hq, seed=0)
    hq.load_state_dict(sd, strict=True)
    sam = SamMaskDecoderHIP()
    sam.load_state_dict({k: v for k, v in sd.items() if k in set(sam.state_dict())}, strict=True)
    hq, sam = hq.to(dev).eval(), sam.to(dev).eval()
    gen = torch.Generator().manual_seed(0)
    emb = torch.randn(1, 256, g, g, generator=gen).to(dev)
    pe = torch.randn(1, 256, g, g, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)   # as the model's table: no copy per call
    inter = torch.randn(1, g, g, 768, generator=gen).to(dev)
    sparse = torch.randn(R, 2, 256, generator=gen).to(dev)
    dense = torch.randn(256, generator=gen).to(dev)
    roi = torch.zeros(R, dtype=torch.int32, device=dev)
    feat = hq.hq_features(emb, inter)
    out = dict(tool='bench_sam_hq', device=torch.cuda.get_device_name(0), grid=g, prompts=R, tokens_sam=7, tokens_hq=8)
    with torch.no_grad():
        for multi in (False, True):
            out[f'decoder_multimask_{multi}'] = alternate({
                'sam': lambda: sam.decode(emb, pe, sparse, dense, roi, multimask_output=multi),
                'hq': lambda: hq.decode(emb, pe, sparse, dense, roi, multimask_output=multi, hq_features=feat),
                'hq_token_only': lambda: hq.decode(emb, pe, sparse, dense, roi, multimask_output=multi, hq_features=feat,
                                                   hq_token_only=True)}, a.reps)
        out['hq_features'] = alternate({'four_conv_transposes': lambda: hq.hq_features(emb, inter)}, a.reps)
        # (b) the kernel alone
        Rk = a.kernel_prompts
        c = ref.kernel_case(Rk, 1, g, seed=1)
        cd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()}
        from rsprompter_amd.necks import convt_weights4
        from rsprompter_amd.sam_decoder import hq_conv_weights
        w2, b2 = convt_weights4(cd['ct_w'], cd['ct_b'])
        w1, wf = hq_conv_weights(cd['c1_w'], cd['c2_w'])
        up = ops.to_planes(cd['up'].contiguous())

        def fused():
            return ops.sam_hq_mask(up, w2, b2, w1, cd['c1_b'], cd['ln_w'], cd['ln_b'], 1e-6, wf, cd['c2_b'], cd['hyper'],
                                   cd['feat'], cd['map'])

        # like for like: both sides get `up` as planes, the chunks' slices and packed weights exist before the timed region
        subs = []
        for r0 in range(0, Rk, a.chunk):
            sub = dict(cd, R=min(a.chunk, Rk - r0), hyper=cd['hyper'][r0:r0 + a.chunk].contiguous(),
                       map=cd['map'][r0:r0 + a.chunk].contiguous())
            sub['up_planes'] = ops.to_planes(cd['up'][r0:r0 + a.chunk].contiguous())
            sub['packed'] = ref.composed_weights(ops, sub, dev)
            subs.append(sub)
        res = torch.empty((Rk, 4 * g, 4 * g), dtype=torch.float32, device=dev)

        def composed():
            for i, sub in enumerate(subs):
                res[i * a.chunk:i * a.chunk + sub['R']] = ref.kernel_composed(ops, sub, dev)
            return res
        diff = float((fused() - composed()).abs().max())
        k = alternate({'fused': fused, 'composed': composed}, max(3, a.reps // 2))
        flops = 2.0 * Rk * (4 * g) ** 2 * (32 * 64 + 288 * 64 + 576 * 32)          # the function's own operations (HF's form)
        k.update(prompts=Rk, chunk=a.chunk, max_abs_diff=diff, function_gflop=round(flops / 1e9, 1),
                 fused_tflops_of_function=round(flops / k['fused']['median_ms'] / 1e9, 1))
        out['kernel'] = k
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
