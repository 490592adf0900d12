#!/usr/bin/env python3
"""Times the semseg cross-entropy + foreground loss, forward + backward, at the training shape (T = 8 on 120 x 216 maps) with 3, 4 and 42
channels, and the preparation of the training targets at 8 x 480 x 864 with 6 and 20 instances: the device path
(stemseg_amd.modeling.losses.CrossEntropyLoss, hip.prepare_targets) against the fp32 oracle (tests/semseg_loss_oracle.py) run with stock
torch ops on the same GPU, interleaved in one process.  Writes profiles/semseg_loss_bench.json (medians, spread, ratio).

    python tools/semseg_loss_bench.py [--reps 30] [--warmup 5] [--out profiles/semseg_loss_bench.json]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import semseg_loss_oracle as SO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semseg_loss_bench.json"))
    a = ap.parse_args()
    from stemseg_amd import hip
    from stemseg_amd.modeling.losses import CrossEntropyLoss
    hip.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "what": "wall clock between device synchronisations, ms; device path and stock torch ops interleaved in one process",
           "loss_forward_backward": {}, "prepare_targets": {}}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def compare(dev, stock):
        for _ in range(a.warmup):
            dev(), stock()
        td, ts = [], []
        for _ in range(a.reps):                                # interleaved: both see the same clocks and neighbours
            td.append(timed(dev))
            ts.append(timed(stock))
        q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), p10_ms=sorted(v)[len(v) // 10], p90_ms=sorted(v)[-1 - len(v) // 10])
        return {"device": q(td), "stock_torch_fp32_oracle": q(ts), "stock_over_device": statistics.median(ts) / statistics.median(td)}

    crit = CrossEntropyLoss()
    for name in ("train_c3", "train_c4", "train_c42"):
        K, has_fg, _, _ = SO.LARGE_CASES[name]
        x, targets = SO.make_case(name, SO.LARGE_CASES)
        x = x.cuda()
        prep = [{k: v.cuda() for k, v in t.items()} for t in SO.prepared(targets)]

        def dev():
            xx = x.clone().requires_grad_(True)
            od = {"optimization_losses": {}, "others": {}}
            (crit.forward_with_foreground if has_fg else crit.forward)(xx.permute(0, 2, 1, 3, 4), prep, od)
            sum(od["optimization_losses"].values()).backward()
            return xx.grad

        def stock():
            xx = x.clone().requires_grad_(True)
            ce, fg = SO.semseg_losses(xx, prep, K, has_fg, torch.float32)
            (ce + fg).backward()
            return xx.grad

        r = compare(dev, stock)
        r.update(channels=K + int(has_fg), shape="N=1, T=8, 120x216")
        res["loss_forward_backward"][name] = r
        print(name, json.dumps(r))
    for n_inst in (6, 20):
        rng = np.random.default_rng(n_inst)
        _, masks, ig, cat = SO.make_sample(rng, 1, 8, 480, 864, tuple(int(c) for c in rng.integers(1, 41, n_inst)))
        masks, ig, cat = torch.from_numpy(masks).cuda(), torch.from_numpy(ig).cuda(), torch.from_numpy(cat).cuda()
        r = compare(lambda: hip.prepare_targets(masks, ig, cat), lambda: SO.prepare_targets(masks, ig, cat))
        r.update(instances=n_inst, shape="T=8, 480x864 -> 120x216")
        res["prepare_targets"]["i%d" % n_inst] = r
        print("prepare_targets i%d" % n_inst, json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
