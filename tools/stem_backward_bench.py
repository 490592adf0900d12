#!/usr/bin/env python3
"""Times the backward of the stem and layer1 at the workload's size -- F = 8 frames of 480 x 864, an R-101 with random weights (the stem's map
240 x 432, layer1's three blocks at 120 x 216): the max-pool backward with the ReLU mask (csrc/stem_backward.hip, both forms), the stem's
weight gradient, and the whole stem + layer1 backward (the recompute of the stem, the max-pool and layer1 from the frames, three
``bottleneck_backward``, ``stem_backward``) against the same gradients from stock torch ops on the same GPU (torch.autograd.grad through
F.conv2d / F.relu / F.max_pool2d; the graph is built outside the timed region, so the stock side pays no recompute), interleaved in one
process, medians of 7.  The pool backward is reported as GB/s of the bytes it must move beside the HBM roof, the weight gradient as the
fraction of the fp32-matrix roof.  Writes profiles/stem_backward_bench.json.

    python tools/stem_backward_bench.py [--reps 7] [--warmup 2] [--frames 8] [--precision f16x3] [--out profiles/stem_backward_bench.json]
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
HBM_ROOF_GBS = {"spec": 8000.0, "measured float4 copy": 6290.0}        # MI355X
FP32_MATRIX_ROOF_TFLOPS = 157.3                                          # v_mfma_f32_32x32x2_f32, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--precision", default="f16x3", choices=("f16x3", "bf16x6", "f32"), help="of the pass and the recompute")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stem_backward_bench.json"))
    a = ap.parse_args()
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward as EB
    from stemseg_amd.modeling.backbone import ResNetFPN
    hip.require_gpu()
    Fr, prec = a.frames, a.precision
    Ho, Wo, Hp, Wp = H // 2, W // 2, H // 4, W // 4
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "runs": "one device, one run",
           "shape": "F=%d, %dx%d, R-101: stem map %dx%d, layer1 (3 blocks) at %dx%d, random weights" % (Fr, H, W, Ho, Wo, Hp, Wp),
           "precision": {"pass and recompute": prec, "wgrad": "f32", "dgrad": "f32"},
           "what": "wall clock between device synchronisations, ms, medians of the reps; device and stock interleaved in one process; the stock "
                   "graph is built outside the timed region"}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def versus(dev_fn, stock_fn):
        for _ in range(a.warmup):
            dev_fn(), stock_fn()
        d, s = [], []
        for _ in range(a.reps):                              # interleaved: both see the same clocks and neighbours
            d.append(timed(dev_fn))
            s.append(timed(stock_fn))
        return d, s

    q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)

    torch.manual_seed(1)
    bb = ResNetFPN("R-101-FPN").eval().cuda()
    bb.precision = prec
    frames = (40.0 * rnd(Fr, 3, H, W)).contiguous()
    bb.forward_channel_major(frames)
    stem, pooled = bb.stem_forward(frames)
    specs = bb.body_stage_specs(1, bb._packed_names[prec])[1]
    scale = bb.body.stem.bn1.scale_shift()[0].detach().float().contiguous().cuda()

    # ---- the max-pool backward with the ReLU mask: x and g read, dx written
    planes = 64 * Fr
    G_pool = rnd(64, Fr, Hp, Wp)
    x3, g3 = stem.view(planes, Ho, Wo), G_pool.view(planes, Hp, Wp)
    pre = stem.permute(1, 0, 2, 3).contiguous().clone().requires_grad_(True)        # (the stock ReLU of a map that is its own ReLU: the same mask)
    pool_stock_out = F.max_pool2d(F.relu(pre), 3, 2, 1)
    G_pool_ff = G_pool.permute(1, 0, 2, 3).contiguous()
    stock_pool = lambda: torch.autograd.grad(pool_stock_out, pre, G_pool_ff, retain_graph=True)
    pool_bytes = 4.0 * planes * (2 * Ho * Wo + Hp * Wp)
    res["maxpool3x3s2_backward"] = {"bytes": pool_bytes, "hbm_roof_GBps": HBM_ROOF_GBS}
    out = torch.empty(planes, Ho, Wo, device="cuda")
    for name, form in (("vec4", hip.STREAM_FORM_VEC4), ("scalar", hip.STREAM_FORM_SCALAR)):
        d, s = versus(lambda: hip.maxpool3x3s2_backward(x3, g3, True, out=out, form=form), stock_pool)
        res["maxpool3x3s2_backward"][name] = dict(q(d), GBps=pool_bytes / statistics.median(d) / 1e6,
                                                  fraction_of_measured_hbm_roof=pool_bytes / statistics.median(d) / 1e6 / HBM_ROOF_GBS["measured float4 copy"])
        res["maxpool3x3s2_backward"]["stock (beside %s)" % name] = q(s)
    same = torch.equal(hip.maxpool3x3s2_backward(x3, g3, True)[0].view(64, Fr, Ho, Wo).permute(1, 0, 2, 3), stock_pool()[0])
    res["maxpool3x3s2_backward"]["equal_to_stock_on_this_input"] = bool(same)

    # ---- the stem's weight gradient
    g_stem = hip.maxpool3x3s2_backward(x3, g3, True)[0].view(64, Fr, Ho, Wo)
    w_leaf = bb.body.stem.conv1.weight.detach().clone().requires_grad_(True)
    conv_out = F.conv2d(frames, w_leaf, stride=2, padding=3)
    g_stem_ff = g_stem.permute(1, 0, 2, 3).contiguous()
    stock_wgrad = lambda: torch.autograd.grad(conv_out, w_leaf, g_stem_ff, retain_graph=True)
    flops = 2.0 * 64 * 147 * Fr * Ho * Wo
    d, s = versus(lambda: hip.stem_wgrad(frames, g_stem), stock_wgrad)
    dw, ref = hip.stem_wgrad(frames, g_stem), stock_wgrad()[0]
    res["stem_wgrad"] = dict(q(d), flops=flops, chunks=hip.stem_wgrad_chunks(Fr, H, W), TFLOPS=flops / statistics.median(d) / 1e9,
                             fraction_of_fp32_matrix_roof=flops / statistics.median(d) / 1e9 / FP32_MATRIX_ROOF_TFLOPS, fp32_matrix_roof_TFLOPS=FP32_MATRIX_ROOF_TFLOPS,
                             stock=q(s), stock_over_device=statistics.median(s) / statistics.median(d),
                             max_difference_device_vs_stock_rel_to_max=float((dw - ref).abs().max() / ref.abs().max()),
                             includes="the partial launch, the combine launch and the workspace allocation of hip.stem_wgrad")

    # ---- the whole: recompute of the stem, the max-pool and layer1, the three blocks' backward, the stem's
    dC1 = rnd(256, Fr, Hp, Wp)

    def dev_all(want_stem=True):
        st, po = bb.stem_forward(frames)
        stash = EB.body_stage_forward(po, specs, prec, int(bb.plan_frames))
        G, grads = dC1, []
        for b in range(len(specs) - 1, -1, -1):
            blk = specs[b]
            weights = dict(conv1=blk["w1"], conv2=blk["w2"], conv3=blk["w3"], down=blk.get("wd"), s1=blk["s1"], s2=blk["s2"], s3=blk["s3"], sd=blk.get("sd"))
            r = EB.bottleneck_backward(hip.dense_volume(stash[b]["xs"]), stash[b], G, weights, "f32", want_dx=want_stem or b > 0)
            G = r.pop("g_x")
            grads.append(r)
            stash[b] = None
        if want_stem:
            grads.append(EB.stem_backward(frames, st, G, scale))
        return grads

    folded = bb.folded_state()
    leaves = {"stem": folded["stem"][0].cuda().clone().requires_grad_(True)}
    for b in range(3):
        for n in ("conv1", "conv2", "conv3") + (("down",) if b == 0 else ()):
            leaves["b%d.%s" % (b, n)] = folded["b%d.%s" % (b, n)][0].cuda().clone().requires_grad_(True)
    bias = lambda n: folded[n][1].cuda()
    xs = F.max_pool2d(F.relu(F.conv2d(frames, leaves["stem"], bias("stem"), stride=2, padding=3)), 3, 2, 1)
    for b in range(3):
        a1 = F.relu(F.conv2d(xs, leaves["b%d.conv1" % b], bias("b%d.conv1" % b)))
        a2 = F.relu(F.conv2d(a1, leaves["b%d.conv2" % b], bias("b%d.conv2" % b), padding=1))
        sc = F.conv2d(xs, leaves["b0.down"], bias("b0.down")) if b == 0 else xs
        xs = F.relu(F.conv2d(a2, leaves["b%d.conv3" % b], bias("b%d.conv3" % b)) + sc)
    dC1_ff = dC1.permute(1, 0, 2, 3).contiguous()
    layer1_leaves = [v for k, v in leaves.items() if k != "stem"]
    stock_all = lambda: torch.autograd.grad(xs, list(leaves.values()), dC1_ff, retain_graph=True)
    stock_l1 = lambda: torch.autograd.grad(xs, layer1_leaves, dC1_ff, retain_graph=True)
    d, s = versus(dev_all, stock_all)
    res["stem_and_layer1_backward (FREEZE_AT_STAGE 0)"] = dict(device_recompute_and_backward=q(d), stock_backward=q(s),
                                                                stock_over_device=statistics.median(s) / statistics.median(d))
    d, s = versus(lambda: dev_all(False), stock_l1)
    res["layer1_backward (FREEZE_AT_STAGE 1)"] = dict(device_recompute_and_backward=q(d), stock_backward=q(s),
                                                       stock_over_device=statistics.median(s) / statistics.median(d))
    rec = [timed(lambda: EB.body_stage_forward(bb.stem_forward(frames)[1], specs, prec, int(bb.plan_frames))) for _ in range(a.reps)]
    res["device_recompute_alone (stem, max-pool, layer1)"] = q(rec)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    dev_all()
    torch.cuda.synchronize()
    res["device_peak_bytes_above_resident"] = torch.cuda.max_memory_allocated() - base
    # separate pass: the library's event profiler around the tagged launches of the existing kernels (the two new kernels carry no tag)
    tags = {"stem + max-pool (recompute)": (47, 48), "wgrad9 (+ combine)": (54,), "wgrad1 (+ combine)": (55,), "relu_backward": (56,), "col2img_relu": (57,),
            "scale_rows": (60,), "sum_partials": (61,), "1x1x1 convolutions (recompute, data gradients)": hip.PROFILE_CONV_TAGS["conv1x1x1"],
            "1x3x3 convolutions (recompute)": hip.PROFILE_CONV_TAGS["conv1x3x3"]}
    n_prof = 2
    hip.profile_enable(True)
    hip.profile_read()
    for _ in range(n_prof):
        dev_all()
    prof = hip.profile_read()
    hip.profile_enable(False)
    res["kernels_of_the_whole (profiler pass)"] = {name: dict(ms_per_backward=sum(prof[t_][0] for t_ in tg if t_ in prof) / n_prof,
                                                              launches=sum(prof[t_][2] for t_ in tg if t_ in prof) // n_prof) for name, tg in tags.items()}
    res["other_tagged_ms_per_backward"] = {str(t_): v[0] / n_prof for t_, v in prof.items() if not any(t_ in tg for tg in tags.values())}
    res["not_measured"] = ("kernel times from a profiler trace (these are call times with launch gaps and allocations in them), the LDS bank conflicts and "
                           "the matrix-pipe utilisation of stem_wgrad_kernel (no counter run), a second device or a second run (no spread between runs), "
                           "the stem + layer1 share of a whole training step")
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
