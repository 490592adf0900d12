#!/usr/bin/env python3
"""Times the optimiser step over the trainable tensors of an R-101 at FREEZE_AT_STAGE 2 with the FPN and the three decoders (embedding,
seediness, semseg): DeviceSGD (0.9, Nesterov, 1e-4) and DeviceAdam (csrc/optimizer.hip, one launch per step) against torch.optim.SGD /
torch.optim.Adam with their defaults on the same GPU, each with and without the clip (``grad_norm`` + ``grad_scale`` against
``torch.nn.utils.clip_grad_norm_``).  Random data; the shapes come from the model built on the CPU.

The protocol is tools/wide_head_bench.py's: every leg in one process, interleaved; a timed window is ``--inner`` steps between two device
synchronisations, so a leg's figure is wall clock per step, host work included; median and p10 .. p90 over ``--reps`` windows.  A separate
pass times the bare launches (tables cached, no Python around them) with device events: the kernels' own rate on the bytes a step has to
move -- SGD 20 B / element (reads p, g, buf; writes p, buf), Adam 28 B, the norm 4 B.  Writes profiles/optimizer_bench.json.

    python tools/optimizer_bench.py [--reps 30] [--warmup 5] [--inner 10] [--out profiles/optimizer_bench.json]
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


def trainable_shapes():
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    from stemseg_amd.training import configure_trainable
    try:
        config.load_preset("defaults")
        config.cfg.MODEL.USE_SEEDINESS_HEAD = config.cfg.MODEL.USE_SEMSEG_HEAD = True
        m = configure_trainable(build_model())
        return [tuple(p.shape) for p in m.parameters() if p.requires_grad]
    finally:
        config.load_preset("defaults")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_bench.json"))
    a = ap.parse_args()
    from stemseg_amd import hip
    from stemseg_amd.training import DeviceAdam, DeviceSGD, grad_norm
    hip.require_gpu()
    shapes = trainable_shapes()
    n_elems = sum(int(torch.Size(s).numel()) for s in shapes)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def params():
        ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen) * 0.05) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 0.01
        return ps

    sgd_kw = dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)
    adam_kw = dict(lr=1e-3, weight_decay=1e-4)
    MAX_NORM = 10.0
    legs = {}

    def leg(name, cls, kw, clip, device):
        ps = params()
        opt = cls(ps, **kw)
        if device and clip:
            def run():
                _, coef, _ = grad_norm(ps, MAX_NORM)
                opt.step(grad_scale=coef)
        elif clip:
            def run():
                torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
                opt.step()
        else:
            run = opt.step
        legs[name] = (run, opt, ps)

    for kind, dev_cls, stock_cls, kw in (("sgd", DeviceSGD, torch.optim.SGD, sgd_kw), ("adam", DeviceAdam, torch.optim.Adam, adam_kw)):
        for clip in (False, True):
            tag = kind + ("_clip" if clip else "")
            leg("device_" + tag, dev_cls, kw, clip, True)
            leg("stock_" + tag, stock_cls, kw, clip, False)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.inner

    for _ in range(a.warmup):
        for run, _, _ in legs.values():
            run()
    t = {k: [] for k in legs}
    for _ in range(a.reps):                                    # interleaved: all see the same clocks and neighbours
        for k, (run, _, _) in legs.items():
            t[k].append(timed(run))
    q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), p10_ms=sorted(v)[len(v) // 10], p90_ms=sorted(v)[-1 - len(v) // 10])
    times = {k: q(v) for k, v in t.items()}

    # the bare launches with device events: the tables of the device legs are cached by now
    def events(fn, n=20):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    sgd_opt, adam_opt = legs["device_sgd"][1], legs["device_adam"][1]
    sgd_tables, adam_tables = sgd_opt._table_cache[0][1], adam_opt._table_cache[0][1]
    side = torch.tensor([1e-3, 1.0], device="cuda").repeat(len(shapes), 1).contiguous()
    norm_tables = hip.OptTables([(p.data_ptr(), p.grad.data_ptr(), 0, 0, p.numel(), 0) for p in legs["device_sgd"][2]], 0, "cuda:0")
    kernels = {}
    for name, nbytes, fn in (("sgd_step", 20, lambda: hip.opt_sgd_step(sgd_tables, hip.opt_hyper(**sgd_kw))),
                             ("adam_step", 28, lambda: hip.opt_adam_step(adam_tables, hip.opt_hyper(weight_decay=1e-4), side)),
                             ("grad_norm", 4, lambda: hip.opt_grad_norm(norm_tables, MAX_NORM))):
        ms = events(fn)
        kernels[name] = {"device_ms_events": ms, "bytes_per_element": nbytes, "achieved_TB_per_s": nbytes * n_elems / (ms * 1e-3) / 1e12}

    verdict = {}
    for tag in ("sgd", "sgd_clip", "adam", "adam_clip"):
        d, s = times["device_" + tag], times["stock_" + tag]
        verdict[tag] = {"device_median_ms": d["median_ms"], "stock_median_ms": s["median_ms"], "stock_p10_p90_width_ms": s["p90_ms"] - s["p10_ms"],
                        "stock_over_device": s["median_ms"] / d["median_ms"],
                        "device_within_margin": bool(d["median_ms"] <= s["median_ms"] + (s["p90_ms"] - s["p10_ms"]))}
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "steps_per_timed_window": a.inner,
           "tensors": len(shapes), "elements": n_elems, "chunk_elements": hip.OPT_CHUNK, "chunks": sgd_tables.n_chunks,
           "what": "wall clock between device synchronisations over steps_per_timed_window optimiser steps, ms per step, host work included; "
                   "eight legs interleaved in one process; gradients stay in place between steps (the tables are uploaded once); stock = "
                   "torch.optim.SGD / Adam with their defaults (foreach on CUDA tensors), clip legs add clip_grad_norm_ / grad_norm + grad_scale",
           "times": times, "verdict": verdict, "kernels": kernels,
           "table_uploads": {k: getattr(legs[k][1], "table_uploads", None) for k in legs if k.startswith("device_")},
           "note": "the project's other streaming kernels reach 3.1-5.1 TB/s (README); the margin: the device median may exceed the stock "
                   "median by the stock side's own p10..p90 width"}
    print(json.dumps(res, indent=1, sort_keys=True))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
