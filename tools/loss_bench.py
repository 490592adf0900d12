#!/usr/bin/env python3
"""Times the embedding loss, forward + backward, at the training shape (T = 8 on 120 x 216 maps) with 6 and 20 instances: the device
path (stemseg_amd.modeling.losses.EmbeddingLoss) against the fp32 oracle (tests/loss_oracle.py) run with stock torch ops on the same
GPU, interleaved in one process.  Writes profiles/loss_bench.json (medians, spread, ratio).

    python tools/loss_bench.py [--reps 20] [--warmup 3] [--out profiles/loss_bench.json]
    python tools/loss_bench.py --trace-workload      # three device forward + backward passes, for rocprofv3 --kernel-trace --stats
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

from tests import loss_oracle as LO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_bench.json"))
    ap.add_argument("--trace-workload", action="store_true")
    a = ap.parse_args()
    from stemseg_amd import hip
    from stemseg_amd.modeling.losses import EmbeddingLoss
    hip.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "shape": "N=1, T=8, 120x216, xyt (C=7)", "reps": a.reps, "warmup": a.warmup,
           "what": "forward + backward of the weighted total, wall clock between device synchronisations, ms", "cases": {}}
    for name in ("train_i6", "train_i20"):
        E, stds, _ = LO.LARGE_CASES[name]
        x, targets = LO.make_case(name, LO.LARGE_CASES)
        x = x.cuda()
        targets = [{k: v.cuda() for k, v in t.items()} for t in targets]
        mod = EmbeddingLoss(4, EMBEDDING_SIZE=E, NBR_FREE_DIMS=len(stds), FREE_DIM_STDS=list(stds), **LO.DEFAULT_WEIGHTS).cuda()

        def dev():
            xx = x.clone().requires_grad_(True)
            od = {}
            mod(xx, targets, od)
            od["optimization_losses"]["embedding_loss"].backward()
            return xx.grad

        def stock():
            xx = x.clone().requires_grad_(True)
            comps = LO.embedding_loss(xx, targets, E, stds, torch.float32)
            LO.total_of(comps, [0, 0, 0])[0].backward()
            return xx.grad

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        if a.trace_workload:
            for _ in range(3):
                dev()
            torch.cuda.synchronize()
            continue
        for _ in range(a.warmup):
            dev(), stock()
        td, ts = [], []
        for _ in range(a.reps):                                # interleaved: both see the same clocks and neighbours
            td.append(timed(dev))
            ts.append(timed(stock))
        q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), p10_ms=sorted(v)[len(v) // 10], p90_ms=sorted(v)[-1 - len(v) // 10])
        res["cases"][name] = {"instances": int(targets[0]["masks"].shape[0]), "device": q(td), "stock_torch_fp32_oracle": q(ts),
                              "stock_over_device": statistics.median(ts) / statistics.median(td)}
        print(name, json.dumps(res["cases"][name]))
    if not a.trace_workload:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
