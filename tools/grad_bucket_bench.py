#!/usr/bin/env python3
"""Times the gradient-bucket kernels of csrc/optimizer.hip on the tensor set of tools/optimizer_bench.py (the trainable tensors of an R-101
at FREEZE_AT_STAGE 2 with the FPN and the three decoders), one GPU, no process group:

  * pack_grads at scale 1 (copy) and at 1/8 (scale), against the same flatten-and-scale in stock torch on the same GPU --
    ``torch.cat`` of the flattened gradients, then ``mul_`` -- interleaved;
  * reduce_ranks at world 1, 2 and 8 over synthetic gathered buffers;
  * the DeviceSGD step reading its gradients from the bucket (``p.grad`` views) against the step reading separate ``.grad`` tensors.

Device events around ``--inner`` launches per window, median and p10 .. p90 over ``--reps`` windows, the legs interleaved.  The rates are the
bytes each kernel has to move -- pack 8 B / element (reads g, writes the bucket), reduce_ranks 4 (world + 1) B, the SGD step 20 B -- over
the time, in GB/s, beside the HBM roof (8000 GB/s by specification).  Nothing here measures more than
one GPU: the collectives between the pack and the step are not timed.  Writes profiles/grad_bucket_bench.json.

    python tools/grad_bucket_bench.py [--reps 30] [--warmup 5] [--inner 10] [--out profiles/grad_bucket_bench.json]
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

HBM_SPEC_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_bucket_bench.json"))
    a = ap.parse_args()
    from optimizer_bench import trainable_shapes
    from stemseg_amd import hip
    from stemseg_amd.training import DeviceSGD, GradBucket
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
    ps = params()
    grads = [p.grad for p in ps]
    tables = hip.BucketTables([(0, g.data_ptr(), g.numel()) for g in grads], "cuda")
    total = tables.total
    bucket = torch.zeros(total, dtype=torch.float32, device="cuda")
    EIGHTH = 0.125
    legs = {"pack_copy": (lambda: hip.opt_pack_grads(tables, bucket, 1.0), 8 * n_elems),
            "pack_scale": (lambda: hip.opt_pack_grads(tables, bucket, EIGHTH), 8 * n_elems)}
    # stock flatten-and-scale: what a caller without the kernel writes (torch.cat allocates its result each time, as it would in a loop)
    keep = {}

    def stock_flatten():
        keep["flat"] = torch.cat([g.reshape(-1) for g in grads])

    def stock_flatten_scale():
        keep["flat"] = torch.cat([g.reshape(-1) for g in grads]).mul_(EIGHTH)
    legs["stock_cat"] = (stock_flatten, 8 * n_elems)
    legs["stock_cat_mul"] = (stock_flatten_scale, 8 * n_elems)             # (the bytes the WORK needs; the stock path moves 16 B / element)
    out = torch.empty(total, dtype=torch.float32, device="cuda")
    for world in (1, 2, 8):
        gathered = torch.randn((world, total), device="cuda", generator=gen) * 0.01
        legs["reduce_ranks_world%d" % world] = ((lambda g=gathered: hip.opt_reduce_ranks(g, out)), 4 * (world + 1) * total)
    # the step: from separate .grad tensors, and from the bucket's views (same values)
    qs = params()
    gb = GradBucket([("t%d" % i, q) for i, q in enumerate(qs)])
    gb.reduce()
    opt_plain, opt_bucket = DeviceSGD(ps, **sgd_kw), DeviceSGD(qs, **sgd_kw)
    legs["sgd_step_from_grad"] = (opt_plain.step, 20 * n_elems)
    legs["sgd_step_from_bucket"] = (opt_bucket.step, 20 * n_elems)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for _ in range(a.warmup):
        for fn, _ in legs.values():
            fn()
    t = {k: [] for k in legs}
    for _ in range(a.reps):                                    # interleaved: all see the same clocks and neighbours
        for k, (fn, _) in legs.items():
            t[k].append(events(fn))
    res_legs = {}
    for k, v in t.items():
        med, nbytes = statistics.median(v), legs[k][1]
        res_legs[k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "p10_ms": sorted(v)[len(v) // 10], "p90_ms": sorted(v)[-1 - len(v) // 10],
                       "bytes": nbytes, "GB_per_s": nbytes / (med * 1e-3) / 1e9, "share_of_hbm_spec": nbytes / (med * 1e-3) / 1e9 / HBM_SPEC_GBS}
    m = lambda k: res_legs[k]["median_ms"]

    # GradBucket.reduce() end to end on the host clock (no group: the pack alone), by what happens to the gradient addresses between
    # steps: unchanged (accumulated in place), released and allocated again (zero_grad + a backward pass; the caching allocator may hand
    # the same blocks back), and moved for certain (the earlier tensors kept alive) -- the last rebuilds and uploads the pack tables
    def reduce_loop(prepare, n=10):
        rs = params()
        b = GradBucket([("t%d" % i, r) for i, r in enumerate(rs)])
        b.reduce()                                             # the first tables
        times, alive = [], []
        for _ in range(n):
            prepare(rs, alive)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.reduce()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "reduces": n, "table_uploads_after_the_first": b.table_uploads - 1}

    def in_place(rs, alive):
        for r in rs:
            r.grad.normal_()

    def reallocated(rs, alive):
        for r in rs:
            r.grad = None
        for r in rs:
            r.grad = torch.randn(r.shape, device="cuda", generator=gen) * 0.01

    def moved(rs, alive):
        alive.append([r.grad for r in rs])
        for r in rs:
            r.grad = torch.randn(r.shape, device="cuda", generator=gen) * 0.01
    reduce_host = {"gradients_in_place": reduce_loop(in_place), "gradients_released_and_reallocated": reduce_loop(reallocated),
                   "gradients_moved": reduce_loop(moved, n=5)}
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "launches_per_timed_window": a.inner,
           "tensors": len(shapes), "elements": n_elems, "bucket_elements": total, "chunks": tables.n_chunks,
           "hbm_roof_GB_per_s_specification": HBM_SPEC_GBS,
           "what": "device events around launches_per_timed_window calls, ms per call (the host's enqueue cost is inside where it exceeds the "
                   "kernel's time); all legs interleaved in one process on one GPU; bytes = what the operation has to move, not what a given "
                   "implementation moves; no process group, no collective is timed",
           "legs": res_legs,
           "comparison": {"stock_cat_over_pack_copy": m("stock_cat") / m("pack_copy"), "stock_cat_mul_over_pack_scale": m("stock_cat_mul") / m("pack_scale"),
                          "sgd_step_from_bucket_over_from_grad": m("sgd_step_from_bucket") / m("sgd_step_from_grad")},
           "grad_bucket_reduce_wall_clock": dict(reduce_host, what="GradBucket.reduce() without a group between two device synchronisations, host "
                                                                    "work included, and how many times it rebuilt and uploaded its pack tables"),
           "table_uploads": {"sgd_step_from_grad": opt_plain.table_uploads, "sgd_step_from_bucket": opt_bucket.table_uploads},
           "not_measured": "anything with more than one GPU: all-reduce / all-gather time, scaling with the number of ranks, the share of a "
                           "training step the reduction takes on a node"}
    print(json.dumps(res, indent=1, sort_keys=True))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
