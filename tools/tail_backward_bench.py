#!/usr/bin/env python3
"""Times forward + backward of the decoders' tails -- GroupNorm -> ReLU -> (pool) of the four last conv outputs, the folded linear tail
and the heads -- at the training shape (T = 8 on 120 x 216 maps, inter channels 256, 256, 128, 128) for the embedding head (n_out 7) and
a 3-class + foreground semseg head (n_out 4): the device path (SqueezeExpandTrunk.tail_from_conv_outputs on modeling/ops.py) against the
same composition written with stock torch ops on the same GPU, interleaved in one process.  A second, separate pass with the library's
profiler on splits the device time by kernel family.  Writes profiles/tail_backward_bench.json (medians, spread, ratio, split).

    python tools/tail_backward_bench.py [--reps 20] [--warmup 3] [--out profiles/tail_backward_bench.json]
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
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

T, H4, W4, CIN, INTER, GROUPS = 8, 120, 216, 256, (256, 256, 128, 128), 32


def decoder(kind):
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder
    from stemseg_amd.modeling.semseg_decoder import SqueezeExpandDecoder
    norm = lambda c: nn.GroupNorm(GROUPS, c)
    torch.manual_seed(0)
    if kind == "embedding":
        return SqueezingExpandDecoder(CIN, INTER, 4, tanh_activation=True, seediness_output=True, experimental_dims="xyff",
                                      PoolType=nn.AvgPool3d, NormType=norm, num_frames=T).cuda()
    return SqueezeExpandDecoder(CIN, 3, INTER, (4, 8, 16, 32), foreground_channel=True, PoolType=nn.AvgPool3d, NormType=norm, num_frames=T).cuda()


def stock_tail(m, conv_outputs, act, axes, grids):
    """The folded composition of tail_from_conv_outputs with stock torch ops (fp32, autograd)."""
    mats = m._linear_tail_trainable(torch.cat([c.weight.reshape(-1, INTER[3]) for c in m._head_convs()], 0))
    z = None
    for lvl, ((D, _, pool), (blk, idx)) in enumerate(zip(conv_outputs, m._LAST_STAGE)):
        gn = getattr(m, blk)[idx + 1]
        y = F.relu(F.group_norm(D[None], GROUPS, gn.weight, gn.bias, gn.eps))
        if pool:
            y = F.avg_pool3d(y, 3, stride=(2, 1, 1), padding=1)
        zl = torch.einsum("oc,cthw->othw", mats[lvl], y[0])
        z = zl if z is None else zl + F.interpolate(z[None], scale_factor=(float(m.t_scales[lvl - 1]), 2.0, 2.0), mode="trilinear", align_corners=False)[0]
    convs = m._head_convs()
    if any(c.bias is not None for c in convs):
        z = z + torch.cat([c.bias if c.bias is not None else torch.zeros(c.out_channels, device=z.device) for c in convs])[:, None, None, None]
    return m._tail_activation(z, act, axes, grids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tail_backward_bench.json"))
    a = ap.parse_args()
    from stemseg_amd import hip
    hip.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "shape": "T=8, 120x216, inter 256/256/128/128, GroupNorm(32)",
           "what": "wall clock between device synchronisations, ms; device path and stock torch ops interleaved in one process; "
                   "the kernel-family split comes from a separate pass with the library's event profiler on", "cases": {}}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), p10_ms=sorted(v)[len(v) // 10], p90_ms=sorted(v)[-1 - len(v) // 10])
    for kind in ("embedding", "semseg"):
        m = decoder(kind)
        flags = list(m.pool_flags)
        g = torch.Generator(device="cuda").manual_seed(1)
        outs = []
        for C, Tl, s, pool in ((INTER[0], T // 4, 8, flags[2]), (INTER[1], T // 2, 4, flags[1]), (INTER[2], T, 2, flags[0]), (INTER[3], T, 1, 0)):
            D = torch.randn(C, Tl, H4 // s, W4 // s, device="cuda", generator=g)
            outs.append((D, hip.groupnorm_stats(D, GROUPS, 1e-5), pool))
        act = m._train_acts()
        c = m._packed()
        act = list(c["act"]) if act is None else list(act)
        axes, grids = list(c["axes"]), m._grid(c, T, H4, W4, outs[0][0].device)
        up = torch.randn(len(act), T, H4, W4, device="cuda", generator=g)
        leaves = [(D.clone().requires_grad_(True), st, pool) for D, st, pool in outs]

        def clear():
            for p in m.parameters():
                p.grad = None
            for D, _, _ in leaves:
                D.grad = None

        def dev_fb():
            clear()
            m.tail_from_conv_outputs(outs, act).backward(up)

        def dev_f():
            with torch.no_grad():
                m.tail_from_conv_outputs(outs, act)

        def stock_fb():
            clear()
            stock_tail(m, leaves, act, axes, grids).backward(up)

        def stock_f():
            with torch.no_grad():
                stock_tail(m, leaves, act, axes, grids)

        # the two compositions are the same function: compare before timing
        dev_fb()
        gd = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        gD = [d.grad.clone() for d in m.tail_conv_outputs]
        stock_fb()
        agree = {n: float((gd[n] - p.grad).abs().max() / p.grad.abs().max()) for n, p in m.named_parameters() if p.grad is not None}
        agree.update({"conv output %d" % i: float((a_ - l[0].grad).abs().max() / l[0].grad.abs().max()) for i, (a_, l) in enumerate(zip(gD, leaves))})
        for _ in range(a.warmup):
            dev_fb(), stock_fb(), dev_f(), stock_f()
        t = {k: [] for k in ("device_fwd_bwd", "stock_fwd_bwd", "device_fwd", "stock_fwd")}
        for _ in range(a.reps):                                # interleaved: all four see the same clocks and neighbours
            t["device_fwd_bwd"].append(timed(dev_fb))
            t["stock_fwd_bwd"].append(timed(stock_fb))
            t["device_fwd"].append(timed(dev_f))
            t["stock_fwd"].append(timed(stock_f))
        r = {k: q(v) for k, v in t.items()}
        r["stock_over_device_fwd_bwd"] = statistics.median(t["stock_fwd_bwd"]) / statistics.median(t["device_fwd_bwd"])
        r["max_gradient_difference_device_vs_stock_rel_to_max"] = max(agree.values())
        r["n_out"] = len(act)
        # separate pass: the library's profiler (events around the tagged launches; forward and backward of a family share its tag)
        hip.profile_enable(True)
        hip.profile_read()
        for _ in range(3):
            dev_fb()
        prof = hip.profile_read()
        hip.profile_enable(False)
        names = {40: "upsample_trilinear fwd + adjoint", 42: "gn_relu fwd + bwd (no pool)", 43: "gn_relu_pool fwd + bwd (avg pool)", 44: "heads / level matrices fwd + bwd"}
        r["kernel_family_ms_per_step"] = {names.get(tag, str(tag)): ms / 3 for tag, (ms, _, _) in prof.items()}
        r["kernel_family_launches_per_step"] = {names.get(tag, str(tag)): n // 3 for tag, (_, _, n) in prof.items()}
        res["cases"][kind] = r
        print(kind, json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
