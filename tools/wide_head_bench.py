#!/usr/bin/env python3
"""Times the wide linear head of the YouTube-VIS preset -- T = 8 on a 120 x 216 map, Cin = 256, n_out = 42 (41 classes + foreground) --
forward + backward: hip.wide_level_head / hip.wide_heads_backward (csrc/decoder_backward.hip) against two baselines on the same GPU,
interleaved in one process:

  (a) the same results composed from entry points the library had before: the 1x1x1 ``conv3d`` in 'f32' on the weight zero-padded to 64
      rows, ``conv2d_wgrad(taps=1)`` on dz zero-padded to 64 channels, and ``conv1x1_dgrad`` (the 1x1x1 convolution with the transposed
      weight) for dx.  The pad copies and the per-call weight packing are inside the timed region: the weights change every optimiser
      step, so the composition cannot avoid them;
  (b) stock torch ops (einsum and its autograd).

A timed window is ``--inner`` calls between two device synchronisations (one call is a fraction of a millisecond).  A second, separate
pass with the library's event profiler on gives the device time of the new backward alone, and from it the achieved rate on the
(2 Cin + n_out) V 4 bytes the backward has to move.  Writes profiles/wide_head_bench.json.

    python tools/wide_head_bench.py [--reps 30] [--warmup 5] [--inner 10] [--out profiles/wide_head_bench.json]
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

T, H, W, CIN, N_OUT, PAD = 8, 120, 216, 256, 42, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_head_bench.json"))
    a = ap.parse_args()
    from stemseg_amd import hip
    hip.require_gpu()
    V = T * H * W
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(CIN, T, H, W, device="cuda", generator=g)
    w = torch.randn(N_OUT, CIN, device="cuda", generator=g) / CIN ** 0.5
    dz = torch.randn(N_OUT, T, H, W, device="cuda", generator=g)

    def new_f():
        return hip.wide_level_head(x, w)

    def new_b():
        return hip.wide_heads_backward(x, w, dz, want_dx=True, want_db=True)

    def comp_f():
        w64 = torch.zeros(PAD, CIN, device="cuda")
        w64[:N_OUT] = w
        out = torch.empty(PAD, T, H, W, device="cuda")
        hip.conv3d(hip.flat_volume(x.view(CIN, V)), hip.pack_conv_weight_any(w64.view(PAD, CIN, 1, 1, 1), "f32"), None,
                   hip.flat_volume(out.view(PAD, V)), 1, epilogue=dict(precision="f32"))
        return out[:N_OUT]

    def comp_b():
        w64 = torch.zeros(PAD, CIN, device="cuda")
        w64[:N_OUT] = w
        dz64 = torch.zeros(PAD, T, H, W, device="cuda")
        dz64[:N_OUT] = dz
        dw, db = hip.conv2d_wgrad(hip.dense_volume(x), dz64, 1, want_db=True)
        dx = hip.conv1x1_dgrad(dz64, w64.view(PAD, CIN, 1, 1), "f32")
        return dx, dw[:N_OUT, :, 0, 0], db[:N_OUT]

    xs, ws = x.clone().requires_grad_(True), w.clone().requires_grad_(True)

    def stock_f():
        with torch.no_grad():
            return torch.einsum("oc,cthw->othw", w, x)

    def stock_fb():
        out = torch.einsum("oc,cthw->othw", ws, xs)
        dx, dw = torch.autograd.grad(out, (xs, ws), dz)
        return out, dx, dw, dz.sum((1, 2, 3))

    # the three are the same function: compare before timing
    rel = lambda p, q: float((p.double() - q.double()).abs().max() / q.double().abs().max())
    o_n, (dx_n, dw_n, db_n) = new_f(), new_b()
    o_c, (dx_c, dw_c, db_c) = comp_f(), comp_b()
    o_s, dx_s, dw_s, db_s = stock_fb()
    agree = {"new_vs_composed": dict(out=rel(o_n, o_c), dx=rel(dx_n, dx_c), dw=rel(dw_n, dw_c), db=rel(db_n, db_c)),
             "new_vs_stock": dict(out=rel(o_n, o_s), dx=rel(dx_n, dx_s), dw=rel(dw_n, dw_s), db=rel(db_n, db_s))}
    print("agreement (max |diff| / max |ref|):", json.dumps(agree))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.inner

    runs = {"new_fwd": new_f, "new_bwd": new_b, "new_fwd_bwd": lambda: (new_f(), new_b()),
            "composed_fwd": comp_f, "composed_bwd": comp_b, "composed_fwd_bwd": lambda: (comp_f(), comp_b()),
            "stock_fwd": stock_f, "stock_fwd_bwd": stock_fb}
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    t = {k: [] for k in runs}
    for _ in range(a.reps):                                    # interleaved: all see the same clocks and neighbours
        for k, fn in runs.items():
            t[k].append(timed(fn))
    q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), p10_ms=sorted(v)[len(v) // 10], p90_ms=sorted(v)[-1 - len(v) // 10])
    med = {k: statistics.median(v) for k, v in t.items()}
    # separate pass: the library's event profiler around the tagged launches of the new backward (kernel + combine)
    hip.profile_enable(True)
    hip.profile_read()
    n_prof = 20
    for _ in range(n_prof):
        new_b()
    prof = hip.profile_read()
    hip.profile_enable(False)
    dev_ms = prof[44][0] / n_prof
    nbytes = (2 * CIN + N_OUT) * V * 4
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "calls_per_timed_window": a.inner,
           "shape": "T=8, 120x216 (V=%d), Cin=%d, n_out=%d" % (V, CIN, N_OUT),
           "what": "wall clock between device synchronisations over calls_per_timed_window calls, ms per call; the three paths interleaved in "
                   "one process; composed = conv3d 1x1x1 f32 on the weight padded to 64 rows + conv2d_wgrad(taps=1) on dz padded to 64 channels "
                   "+ conv1x1_dgrad, pad copies and weight packing included; stock = torch einsum and its autograd",
           "times": {k: q(v) for k, v in t.items()},
           "composed_over_new": {k: med["composed_" + k] / med["new_" + k] for k in ("fwd", "bwd", "fwd_bwd")},
           "stock_over_new": {k: med["stock_" + k] / med["new_" + k] for k in ("fwd", "fwd_bwd")},
           "new_backward_not_slower_than_composed": bool(med["new_bwd"] <= med["composed_bwd"]),
           "new_backward": {"algorithmic_bytes": nbytes, "device_ms_event_profiler": dev_ms, "launches_per_call": prof[44][2] // n_prof,
                            "achieved_TB_per_s_device_time": nbytes / (dev_ms * 1e-3) / 1e12,
                            "achieved_TB_per_s_wall_clock": nbytes / (med["new_bwd"] * 1e-3) / 1e12,
                            "chunks": hip.wide_heads_backward_chunks(CIN, N_OUT, V),
                            "note": "the project's other streaming kernels reach 3.1-5.1 TB/s (README); an observation, not a pass mark"},
           "agreement_max_rel_to_max": agree}
    print(json.dumps(res, indent=1, sort_keys=True))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
