#!/usr/bin/env python3
"""Times forward + backward of one WHOLE embedding decoder at the reference preset's widths (in 256, inter 256, 256, 128, 128,
GroupNorm(32), n_out 7) and training shape (T = 8, 4x map 120 x 216): the device path (SqueezeExpandTrunk.forward_trainable: Conv3dFunction
and GnReluPoolFunction per stage on csrc/conv_backward.hip and csrc/decoder_backward.hip, then the folded tail) against the same decoder
written with stock torch ops on the same GPU, interleaved in one process.  Then the weight gradient alone, stage by stage, with its
fraction of the fp32 matrix peak (157 TFLOP/s) from 2 Cout Cin 27 T H W flops, and -- a separate pass with the library's event profiler
on -- the split of the device step by kernel family.  Writes profiles/decoder_backward_bench.json.

    python tools/decoder_backward_bench.py [--reps 10] [--warmup 2] [--out profiles/decoder_backward_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stem-seg_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tail_backward_bench import CIN, GROUPS, H4, INTER, T, W4, decoder, stock_tail  # noqa: E402

FP32_MATRIX_PEAK_TFLOPS = 157.0


def stock_decoder(m, feats, act, axes, grids):
    """The reference decoder with stock torch ops (fp32, autograd): conv -> GroupNorm -> ReLU -> (avg pool) per stage, then the tail."""
    from stemseg_amd.modeling.decoder_base import _BLOCK_CONVS
    flags = list(m.pool_flags)
    outs = []
    for x, stages, pools in zip(feats, m._BRANCH_STAGES, (flags, flags[:2], flags[:1], [0])):
        for k, (si, pool) in enumerate(zip(stages, pools)):
            blk, idx = _BLOCK_CONVS[si]
            conv, gn = getattr(m, blk)[idx], getattr(m, blk)[idx + 1]
            D = F.conv3d(x[None], conv.weight, conv.bias, padding=1)[0]
            if k == len(stages) - 1:
                outs.append((D, None, pool))
                break
            y = F.relu(F.group_norm(D[None], GROUPS, gn.weight, gn.bias, gn.eps))
            x = (F.avg_pool3d(y, 3, stride=(2, 1, 1), padding=1) if pool else y)[0]
    return stock_tail(m, outs, act, axes, grids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_backward_bench.json"))
    a = ap.parse_args()
    from stemseg_amd import hip
    hip.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "shape": "embedding decoder, T=8, 120x216, in 256, inter 256/256/128/128, GroupNorm(32), n_out 7",
           "what": "wall clock between device synchronisations, ms; device path and stock torch ops interleaved in one process; wgrad alone per "
                   "stage; the kernel-family split comes from a separate pass with the library's event profiler on"}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), p10_ms=sorted(v)[len(v) // 10], p90_ms=sorted(v)[-1 - len(v) // 10])
    m = decoder("embedding")
    res["precision"] = {"forward": m.precision, "wgrad": "f32", "dgrad": "bf16x6"}
    g = torch.Generator(device="cuda").manual_seed(1)
    feats = [torch.randn(CIN, T, H4 // s, W4 // s, device="cuda", generator=g) for s in (8, 4, 2, 1)]
    c = m._packed()
    act = list(m._train_acts() or c["act"])
    axes, grids = list(c["axes"]), m._grid(c, T, H4, W4, feats[0].device)
    up = torch.randn(len(act), T, H4, W4, device="cuda", generator=g)

    def clear():
        for p in m.parameters():
            p.grad = None

    def dev_fb():
        clear()
        m.forward_trainable(feats, act).backward(up)

    def dev_f():
        with torch.no_grad():
            m.run_hip(feats, 0, act)

    def stock_fb():
        clear()
        stock_decoder(m, feats, act, axes, grids).backward(up)

    def stock_f():
        with torch.no_grad():
            stock_decoder(m, feats, act, axes, grids)

    # the two are the same function: compare before timing
    dev_fb()
    gd = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    stock_fb()
    agree = {n: float((gd[n] - p.grad).abs().max() / p.grad.abs().max()) for n, p in m.named_parameters() if p.grad is not None}
    res["max_gradient_difference_device_vs_stock_rel_to_max"] = max(agree.values())
    res["parameters_with_gradients"] = len(gd)
    res["largest_gradient_differences"] = dict(sorted(agree.items(), key=lambda kv: -kv[1])[:5])
    res["median_gradient_difference"] = statistics.median(agree.values())
    for _ in range(a.warmup):
        dev_fb(), stock_fb(), dev_f(), stock_f()
    t = {k: [] for k in ("device_fwd_bwd", "stock_fwd_bwd", "device_fwd", "stock_fwd")}
    for _ in range(a.reps):                                    # interleaved: all four see the same clocks and neighbours
        t["device_fwd_bwd"].append(timed(dev_fb))
        t["stock_fwd_bwd"].append(timed(stock_fb))
        t["device_fwd"].append(timed(dev_f))
        t["stock_fwd"].append(timed(stock_f))
    res.update({k: q(v) for k, v in t.items()})
    res["stock_over_device_fwd_bwd"] = statistics.median(t["stock_fwd_bwd"]) / statistics.median(t["device_fwd_bwd"])
    print(json.dumps({k: res[k] for k in ("device_fwd_bwd", "stock_fwd_bwd", "stock_over_device_fwd_bwd")}))

    # the weight gradient alone, stage by stage
    flags = list(m.pool_flags)
    stages = []
    for s, couts, pools in ((8, INTER[:1] * 3, flags), (4, INTER[1:2] * 2, flags[:2]), (2, INTER[2:3], flags[:1]), (1, INTER[3:], [0])):
        cin, Tl = CIN, T
        for cout, pool in zip(couts, pools):
            stages.append((cin, cout, Tl, H4 // s, W4 // s))
            cin, Tl = cout, (Tl + 1) // 2 if pool else Tl
    res["wgrad_stages"] = []
    for cin, cout, Tl, h, w in stages:
        buf, geo = hip.alloc_padded(cin, Tl, h, w)
        hip.copy_to_volume(torch.randn(cin, Tl, h, w, device="cuda", generator=g), 0, hip.padded_interior_view(buf, geo, cin, Tl, h, w))
        view = hip.padded_halo_view(buf, geo, cin, Tl, h, w)
        dy = torch.randn(cout, Tl, h, w, device="cuda", generator=g)
        run = lambda: hip.conv3d_wgrad(view, dy)
        for _ in range(a.warmup):
            run()
        v = [timed(run) for _ in range(a.reps)]
        # (the same gradient from torch's own convolution backward, fp32: the agreement at the full-size shape)
        wz = torch.zeros(cout, cin, 3, 3, 3, device="cuda", requires_grad=True)
        F.conv3d(hip.padded_to_dense(buf, geo, cin, Tl, h, w)[None], wz, padding=1).backward(dy[None])
        dw = run()[0]
        agree_w = float((dw - wz.grad).abs().max() / wz.grad.abs().max())
        del wz
        flops = 2.0 * cout * cin * 27 * Tl * h * w
        r = dict(Cin=cin, Cout=cout, T=Tl, H=h, W=w, chunks=hip.conv3d_wgrad_chunks(cin, cout, Tl, h, w), gflop=flops / 1e9, max_difference_vs_torch_fp32_rel_to_max=agree_w, **q(v))
        r["tflops"] = flops / (r["median_ms"] * 1e-3) / 1e12
        r["fraction_of_fp32_matrix_peak"] = r["tflops"] / FP32_MATRIX_PEAK_TFLOPS
        res["wgrad_stages"].append(r)
        print(json.dumps(r))

    # separate pass: the library's profiler (events around the tagged launches; forward and backward of a family share its tag)
    hip.profile_enable(True)
    hip.profile_read()
    for _ in range(3):
        dev_fb()
    prof = hip.profile_read()
    hip.profile_enable(False)
    names = {40: "upsample_trilinear fwd + adjoint", 42: "gn_relu fwd + bwd (no pool)", 43: "gn_relu_pool fwd + bwd (avg pool)",
             44: "heads / level matrices fwd + bwd", 53: "conv3d wgrad (+ combine)"}
    names.update({tag: "conv3d fwd (tile class %d)" % tag for tag in hip.PROFILE_CONV_TAGS["conv3x3x3"]})
    names.update({tag: "conv3d dgrad: 1x1x1 conv of the per-tap weights (tile class %d)" % tag for tag in hip.PROFILE_CONV_TAGS["conv1x1x1"]})
    names[41] = "GroupNorm statistics (finalize)"
    res["kernel_family_ms_per_step"] = {names.get(tag, "tag %d" % tag): ms / 3 for tag, (ms, _, _) in prof.items()}
    res["kernel_family_launches_per_step"] = {names.get(tag, "tag %d" % tag): n // 3 for tag, (_, _, n) in prof.items()}
    print(json.dumps(res["kernel_family_ms_per_step"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
