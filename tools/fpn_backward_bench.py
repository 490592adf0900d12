#!/usr/bin/env python3
"""Times the FPN backward at the workload's size -- F = 8 frames of 480 x 864 (levels 120 x 216, 60 x 108, 30 x 54, 15 x 27), R-101 channel
counts (stage outputs 256 / 512 / 1024 / 2048, 256 FPN channels): the device path (encoder_backward.fpn_backward: csrc/conv_backward.hip, the forward
1x1x1 kernel on the per-tap weights, the bilinear adjoint of csrc/decoder_backward.hip) against the same sixteen gradients from stock torch
ops on the same GPU (torch.autograd.grad through F.conv2d / F.interpolate; the graph is built outside the timed region), interleaved in one
process.  Then -- a separate pass with the library's event profiler on -- time and fraction of the fp32 matrix roof (157.3 TFLOP/s) of the
9-tap weight gradient, the 1-tap weight gradient and the per-tap convolution of the data gradient, and the peak device memory of one device
backward.  Writes profiles/fpn_backward_bench.json.

    python tools/fpn_backward_bench.py [--reps 10] [--warmup 2] [--frames 8] [--out profiles/fpn_backward_bench.json]
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

FP32_MATRIX_PEAK_TFLOPS = 157.3
H, W = 480, 864
LATERAL = (256, 512, 1024, 2048)
CF = 256


def stock_fpn(Cs, iw, ib, lw, lb):
    """fpn.py:47-69 with stock ops on frames-first maps."""
    Ls, Ps = [None] * 4, [None] * 4
    for k in (3, 2, 1, 0):
        lat = F.conv2d(Cs[k], iw[k], ib[k])
        if k < 3:
            lat = lat + F.interpolate(Ls[k + 1], scale_factor=2, mode="bilinear", align_corners=False)
        Ls[k] = lat
        Ps[k] = F.conv2d(lat, lw[k], lb[k], padding=1)
    return Ls, Ps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--precision", default="bf16x6", choices=("bf16x6", "f32"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpn_backward_bench.json"))
    a = ap.parse_args()
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward
    hip.require_gpu()
    Fr = a.frames
    maps = [(H >> (2 + k), W >> (2 + k)) for k in range(4)]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "shape": "FPN backward, F=%d, %dx%d (levels %s), stage outputs %s, %d FPN channels" % (Fr, H, W, maps, list(LATERAL), CF),
           "precision": {"wgrad": "f32", "dgrad": a.precision},
           "dgrad_scratch": "not chunked: one [9 x 256][F h w] buffer of per-tap products per level",
           "what": "wall clock between device synchronisations, ms; encoder_backward.fpn_backward and torch.autograd.grad through stock ops interleaved in one "
                   "process; the per-kernel figures come from a separate pass with the library's event profiler on"}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    Cs = [rnd(c, Fr, h, w) for c, (h, w) in zip(LATERAL, maps)]                         # channel-major, as the encoder keeps them
    iw = [(rnd(CF, c, 1, 1) / c ** 0.5).requires_grad_(True) for c in LATERAL]
    ib = [(0.1 * rnd(CF)).requires_grad_(True) for _ in LATERAL]
    lw = [(rnd(CF, CF, 3, 3) / (9 * CF) ** 0.5).requires_grad_(True) for _ in LATERAL]
    lb = [(0.1 * rnd(CF)).requires_grad_(True) for _ in LATERAL]
    dP = [rnd(CF, Fr, h, w) for h, w in maps]
    Cs_ff = [c.permute(1, 0, 2, 3).contiguous() for c in Cs]
    dP_ff = [d.permute(1, 0, 2, 3).contiguous() for d in dP]
    Ls, Ps = stock_fpn(Cs_ff, iw, ib, lw, lb)
    # the merged laterals in the encoder's zero-haloed layout
    keep, l_views = [], []
    for L, (h, w) in zip(Ls, maps):
        buf, geo = hip.alloc_padded2d(CF, Fr, h, w)
        hip.copy_to_volume(L.detach().permute(1, 0, 2, 3).contiguous(), 0, hip.padded2d_interior_view(buf, geo, CF, Fr, h, w))
        keep.append(buf)
        l_views.append(hip.padded2d_halo_view(buf, geo, CF, Fr, h, w))
    c_views = [hip.dense_volume(c) for c in Cs]
    lw_d = [w.detach() for w in lw]
    params = iw + ib + lw + lb

    dev_bwd = lambda: encoder_backward.fpn_backward(c_views, l_views, dP, lw_d, a.precision)
    stock_bwd = lambda: torch.autograd.grad(Ps, params, dP_ff, retain_graph=True)

    # the two are the same function: compare before timing
    d_layer_w, d_layer_b, d_inner_w, d_inner_b = dev_bwd()
    ref = stock_bwd()
    agree = {}
    for k in range(4):
        for name, got, want in (("fpn_inner%d.weight", d_inner_w[k], ref[k]), ("fpn_inner%d.bias", d_inner_b[k], ref[4 + k]),
                                ("fpn_layer%d.weight", d_layer_w[k], ref[8 + k]), ("fpn_layer%d.bias", d_layer_b[k], ref[12 + k])):
            agree[name % (k + 1)] = float((got - want).abs().max() / want.abs().max())
    res["max_gradient_difference_device_vs_stock_rel_to_max"] = max(agree.values())
    res["gradient_differences_device_vs_stock_rel_to_max"] = agree
    del ref, d_layer_w, d_layer_b, d_inner_w, d_inner_b
    for _ in range(a.warmup):
        dev_bwd(), stock_bwd()
    t = {"device_bwd": [], "stock_bwd": []}
    for _ in range(a.reps):                                      # interleaved: both see the same clocks and neighbours
        t["device_bwd"].append(timed(dev_bwd))
        t["stock_bwd"].append(timed(stock_bwd))
    res.update({k: q(v) for k, v in t.items()})
    res["stock_over_device_bwd"] = statistics.median(t["stock_bwd"]) / statistics.median(t["device_bwd"])
    print(json.dumps({k: res[k] for k in ("device_bwd", "stock_bwd", "stock_over_device_bwd", "max_gradient_difference_device_vs_stock_rel_to_max")}))

    # peak device memory of one device backward, above what is resident before it (inputs, the stock graph)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dev_bwd()
    torch.cuda.synchronize()
    res["device_bwd_peak_bytes_above_resident"] = torch.cuda.max_memory_allocated() - base
    res["resident_bytes_before"] = base
    res["cols_bytes_level_4x"] = 9 * CF * Fr * maps[0][0] * maps[0][1] * 4

    # separate pass: the library's profiler (events around the tagged launches)
    n_prof = 3
    hip.profile_enable(True)
    hip.profile_read()
    for _ in range(n_prof):
        dev_bwd()
    prof = hip.profile_read()
    hip.profile_enable(False)
    fam = {"wgrad9 (+ combine)": (54,), "wgrad1 (+ combine)": (55,), "per-tap convolution of the data gradient (1x1x1 forward kernel)": hip.PROFILE_CONV_TAGS["conv1x1x1"]}
    res["kernels"] = {}
    for name, tags in fam.items():
        ms = sum(prof[t_][0] for t_ in tags if t_ in prof) / n_prof
        work = sum(prof[t_][1] for t_ in tags if t_ in prof) / n_prof
        launches = sum(prof[t_][2] for t_ in tags if t_ in prof) // n_prof
        tf = work / (ms * 1e-3) / 1e12 if ms else 0.0
        res["kernels"][name] = dict(ms_per_backward=ms, gflop=work / 1e9, launches=launches, tflops=tf, fraction_of_fp32_matrix_roof=tf / FP32_MATRIX_PEAK_TFLOPS)
    res["other_tagged_ms_per_backward"] = {str(t_): v[0] / n_prof for t_, v in prof.items() if not any(t_ in tags for tags in fam.values())}
    res["wgrad_chunks"] = {"wgrad9": [hip.conv2d_wgrad_chunks(CF, CF, 9, Fr, h, w) for h, w in maps],
                           "wgrad1": [hip.conv2d_wgrad_chunks(c, CF, 1, Fr, h, w) for c, (h, w) in zip(LATERAL, maps)]}
    print(json.dumps(res["kernels"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
