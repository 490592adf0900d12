#!/usr/bin/env python3
"""Times the ResNeXt body backward at the workload's size -- F = 8 frames of 480 x 864, ResNeXt-101 32x8d with the stride in the 3x3 (stages
2-4: 4 / 23 / 3 blocks, bottleneck widths 512 / 1024 / 2048 = 32 groups of 16 / 32 / 64 channels, at 60 x 108, 30 x 54, 15 x 27) with random
weights: the device path (encoder_backward.body_backward: per stage the recompute with conv2 on hip.conv2d_grouped, then hip.conv2d_grouped_wgrad /
conv2d_grouped_dgrad and the kernels of the one-group body) against the same gradients from stock torch ops on the same GPU
(torch.autograd.grad through F.conv2d(groups=, stride=) / F.relu; the graph is built outside the timed region, so the stock side pays no
recompute), interleaved in one process, medians of the reps.  First the body alone, with given gradients of the three stage outputs; then the
FPN and the body together.  Then the grouped weight-gradient launches alone, per distinct conv2 shape: ms, GB/s over the bytes a single read of
x and dy and a single write of dw move, and the fraction of the 157.3 TFLOP/s fp32-matrix roof.  Nothing here is a pass mark.  Writes
profiles/resnext_backward_bench.json.

    python tools/resnext_backward_bench.py [--reps 5] [--warmup 2] [--frames 8] [--precision f16x3] [--out profiles/resnext_backward_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stem-seg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

H, W = 480, 864
BLOCKS = {2: 4, 3: 23, 4: 3}          # R-101
GROUPS, WIDTH = 32, 8
CF = 256
F32_MATRIX_ROOF = 157.3e12
WGRAD_TAG = 62


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--precision", default="f16x3", choices=("f16x3", "bf16x6", "f32"), help="of the recompute (the pass's)")
    ap.add_argument("--plan-frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnext_backward_bench.json"))
    a = ap.parse_args()
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward
    hip.require_gpu()
    Fr, prec = a.frames, a.precision
    maps = [(H >> (2 + k), W >> (2 + k)) for k in range(4)]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "shape": "ResNeXt body backward, F=%d, %dx%d, R-101 32x8d, stride in the 3x3, stages 2-4 (%s blocks) at %s, random weights"
                    % (Fr, H, W, list(BLOCKS.values()), maps[1:]),
           "precision": {"recompute": prec, "wgrad": "f32", "dgrad (body)": "f32", "dgrad (FPN)": "bf16x6"},
           "what": "wall clock between device synchronisations, ms, medians of the reps; the device path recomputes every stage, the stock path "
                   "(torch.autograd.grad through F.conv2d / F.relu, graph built outside the timed region) does not; interleaved in one process; no "
                   "pass mark is set on any of these numbers"}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    pack = lambda w: hip.pack_conv_weight_any(w.reshape(w.shape[0], w.shape[1], 1, w.shape[2], w.shape[3]).contiguous(), prec)

    stages, stock_w = {}, {}
    cin = 256
    for st, nb in BLOCKS.items():
        mid, cout = GROUPS * WIDTH << (st - 1), 256 << (st - 1)
        cg = mid // GROUPS
        stages[st], stock_w[st] = [], []
        for b in range(nb):
            ci = cin if b == 0 else cout
            ws = dict(w1=rnd(mid, ci, 1, 1) * (2.0 / ci) ** 0.5, w2=rnd(mid, cg, 3, 3) * (2.0 / (9 * cg)) ** 0.5, w3=rnd(cout, mid, 1, 1) * (0.5 / mid) ** 0.5)
            if b == 0:
                ws["wd"] = rnd(cout, ci, 1, 1) * (1.0 / ci) ** 0.5
            bias = {k: 0.1 * rnd(v.shape[0]) for k, v in ws.items()}
            d = dict(ws, stride=2 if b == 0 else 1, groups=GROUPS, stride_in_3x3=b == 0, conv1=(pack(ws["w1"]), bias["w1"]),
                     conv2=(hip.pack_grouped_conv_weight(ws["w2"], GROUPS, prec), bias["w2"]), conv3=(pack(ws["w3"]), bias["w3"]))
            if b == 0:
                d["down"] = (pack(ws["wd"]), bias["wd"])
            stages[st].append(d)
            stock_w[st].append(({k: v.clone().requires_grad_(True) for k, v in ws.items()}, bias))
        cin = cout
    x1 = rnd(256, Fr, *maps[0]).abs()                                   # the output of stage 1

    inputs, x = {}, x1
    for st in BLOCKS:
        inputs[st] = x
        x = encoder_backward.body_stage_forward(x, stages[st], prec, a.plan_frames)[-1]["out"]
    C_dev = [x1] + [inputs[3], inputs[4], x]

    def stock_body(xf):
        outs = []
        for st in BLOCKS:
            for b, (w, bias) in enumerate(stock_w[st]):
                a1 = F.relu(F.conv2d(xf, w["w1"], bias["w1"]))
                a2 = F.relu(F.conv2d(a1, w["w2"], bias["w2"], padding=1, stride=2 if b == 0 else 1, groups=GROUPS))
                xf = F.relu(F.conv2d(a2, w["w3"], bias["w3"]) + (F.conv2d(xf[:, :, ::2, ::2], w["wd"], bias["wd"]) if b == 0 else xf))
            outs.append(xf)
        return outs

    body_params = [w[k] for st in BLOCKS for w, _ in stock_w[st] for k in (("wd", "w1", "w2", "w3") if "wd" in w else ("w1", "w2", "w3"))]
    C_stock = stock_body(x1.permute(1, 0, 2, 3).contiguous())
    dC = {st: rnd(256 << (st - 1), Fr, *maps[st - 1]) for st in BLOCKS}
    dC_ff = [dC[st].permute(1, 0, 2, 3).contiguous() for st in BLOCKS]

    def flat(grads):
        return [g_[k] for st in BLOCKS for g_ in grads[st] for k in (("down", "conv1", "conv2", "conv3") if g_["down"] is not None else ("conv1", "conv2", "conv3"))]

    dev_body = lambda: encoder_backward.body_backward(inputs, stages, dC, prec, 2, a.plan_frames)
    stock_bwd = lambda: torch.autograd.grad(C_stock, body_params, dC_ff, retain_graph=True)
    got, ref = flat(dev_body()), stock_bwd()
    diffs = [float((p_ - r_).abs().max() / r_.abs().max()) for p_, r_ in zip(got, ref)]
    res["body_max_gradient_difference_device_vs_stock_rel_to_max"] = max(diffs)
    res["body_median_gradient_difference_device_vs_stock_rel_to_max"] = statistics.median(diffs)
    res["note_on_the_difference"] = ("the two sides differ in their FORWARD: the device recomputes in %s, stock torch in its own fp32 convolutions, so ReLU "
                                     "masks flip at near-zero activations; the tests compare on given activations (DESIGN.md 9m)" % prec)
    del got, ref
    for _ in range(a.warmup):
        dev_body(), stock_bwd()
    t = {"device_body_recompute_and_backward": [], "stock_body_backward": []}
    for _ in range(a.reps):                                              # interleaved: both see the same clocks and neighbours
        t["device_body_recompute_and_backward"].append(timed(dev_body))
        t["stock_body_backward"].append(timed(stock_bwd))
    recompute = lambda: [encoder_backward.body_stage_forward(inputs[st], stages[st], prec, a.plan_frames) for st in BLOCKS]
    t["device_recompute_alone"] = [timed(recompute) for _ in range(a.reps)]

    # the FPN on top: device laterals from stock values (the layout the encoder leaves them in)
    iw = [(rnd(CF, 256 << k, 1, 1) / (256 << k) ** 0.5).requires_grad_(True) for k in range(4)]
    ib = [(0.1 * rnd(CF)).requires_grad_(True) for _ in range(4)]
    lw = [(rnd(CF, CF, 3, 3) / (9 * CF) ** 0.5).requires_grad_(True) for _ in range(4)]
    lb = [(0.1 * rnd(CF)).requires_grad_(True) for _ in range(4)]

    def stock_fpn(Cs):
        Ls, Ps = [None] * 4, [None] * 4
        for k in (3, 2, 1, 0):
            lat = F.conv2d(Cs[k], iw[k], ib[k])
            if k < 3:
                lat = lat + F.interpolate(Ls[k + 1], scale_factor=2, mode="bilinear", align_corners=False)
            Ls[k] = lat
            Ps[k] = F.conv2d(lat, lw[k], lb[k], padding=1)
        return Ls, Ps

    Ls, Ps = stock_fpn([x1.permute(1, 0, 2, 3).contiguous()] + C_stock)
    keep, l_views = [], []
    for L, (h, w) in zip(Ls, maps):
        buf, geo = hip.alloc_padded2d(CF, Fr, h, w)
        hip.copy_to_volume(L.detach().permute(1, 0, 2, 3).contiguous(), 0, hip.padded2d_interior_view(buf, geo, CF, Fr, h, w))
        keep.append(buf)
        l_views.append(hip.padded2d_halo_view(buf, geo, CF, Fr, h, w))
    c_views = [hip.dense_volume(c) for c in C_dev]
    dP = [rnd(CF, Fr, h, w) for h, w in maps]
    dP_ff = [d.permute(1, 0, 2, 3).contiguous() for d in dP]
    lw_d, iw_d = [w.detach() for w in lw], [w.detach() for w in iw]

    def dev_all():
        out = encoder_backward.fpn_backward(c_views, l_views, dP, lw_d, "bf16x6", want_dC=(1, 2, 3), inner_weights=iw_d)
        return out, encoder_backward.body_backward(inputs, stages, {st: out[4][st - 1] for st in BLOCKS}, prec, 2, a.plan_frames)

    stock_all = lambda: torch.autograd.grad(Ps, body_params + iw + ib + lw + lb, dP_ff, retain_graph=True)
    for _ in range(a.warmup):
        dev_all(), stock_all()
    t["device_fpn_and_body"], t["stock_fpn_and_body"] = [], []
    for _ in range(a.reps):
        t["device_fpn_and_body"].append(timed(dev_all))
        t["stock_fpn_and_body"].append(timed(stock_all))
    res.update({k: q(v) for k, v in t.items()})
    med = lambda k: statistics.median(t[k])
    res["stock_over_device_body"] = med("stock_body_backward") / med("device_body_recompute_and_backward")
    res["stock_over_device_fpn_and_body"] = med("stock_fpn_and_body") / med("device_fpn_and_body")
    print(json.dumps({k: res[k] for k in list(t) + ["stock_over_device_body", "stock_over_device_fpn_and_body"]}))

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dev_body()
    torch.cuda.synchronize()
    res["device_body_peak_bytes_above_resident"] = torch.cuda.max_memory_allocated() - base
    res["resident_bytes_before"] = base

    # the grouped weight-gradient launches alone (kernel + combine), per distinct conv2 shape of the network; buffers re-used between reps
    res["grouped_wgrad"] = {}
    shapes = []
    for st in BLOCKS:
        mid = GROUPS * WIDTH << (st - 1)
        h, w = maps[st - 1]
        shapes += [("stage %d block 0 (stride 2, input %dx%d)" % (st, 2 * h, 2 * w), mid, 2, 2 * h, 2 * w), ("stage %d blocks 1.. (stride 1, %dx%d)" % (st, h, w), mid, 1, h, w)]
    for name, mid, s, hh, ww in shapes:
        buf, geo = hip.alloc_padded2d(mid, Fr, hh, ww)
        hip.copy_to_volume(rnd(mid, Fr, hh, ww).abs(), 0, hip.padded2d_interior_view(buf, geo, mid, Fr, hh, ww))
        v = hip.padded2d_halo_view(buf, geo, mid, Fr, hh, ww)
        ho, wo = (hh - 1) // s + 1, (ww - 1) // s + 1
        dy = rnd(mid, Fr, ho, wo)
        run = lambda: hip.conv2d_grouped_wgrad(v, dy, GROUPS, s)
        for _ in range(a.warmup):
            run()
        ms = statistics.median([timed(run) for _ in range(a.reps)])
        cg = mid // GROUPS
        flops = 2.0 * 9 * mid * cg * Fr * ho * wo
        nbytes = 4.0 * (mid * Fr * hh * ww + mid * Fr * ho * wo + mid * cg * 9)
        res["grouped_wgrad"][name] = dict(channels=mid, per_group=cg, stride=s, chunks=hip.conv2d_grouped_wgrad_chunks(mid, GROUPS, s, Fr, hh, ww), median_ms=ms,
                                          gflop=flops / 1e9, gb_per_s_single_read=nbytes / ms / 1e6, fraction_of_f32_matrix_roof=flops / (ms * 1e-3) / F32_MATRIX_ROOF)
    print(json.dumps(res["grouped_wgrad"]))

    # separate pass: the library's profiler on the grouped weight gradient's tag
    n_prof = 2
    hip.profile_enable(True)
    hip.profile_read()
    for _ in range(n_prof):
        dev_body()
    prof = hip.profile_read()
    hip.profile_enable(False)
    res["tagged_ms_per_backward"] = {str(t_): dict(ms=v[0] / n_prof, launches=v[2] // n_prof) for t_, v in prof.items()}
    res["grouped_wgrad_ms_per_backward"] = prof.get(WGRAD_TAG, (0.0, 0, 0))[0] / n_prof
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
