#!/usr/bin/env python3
"""Timing of the DAVIS evaluation on the device next to the numpy oracle on the host (not part of bench.py).

    python tools/davis_eval_bench.py [--repeats 9] [--oracle-repeats 2] [--out profiles/davis_eval_bench.json]

One synthetic sequence at the size of a DAVIS one, built from a seed: 70 frames of 480 x 854, an index map with 5 proposals (drifting
ellipses), 3 objects (the first three proposals shifted by a few pixels), radius 8.  Each figure is a host clock around work that ends in
a device synchronise (the device rows) or in the result (the host row); medians over the repeats, after a warm-up call.
  counts_kernel   ``hip.davis_eval_counts``: the fill launch and the counting launch, the seven tables left on the device
  add_sequence    ``DavisEvaluator.add_sequence``: the same two launches, the one read-back of the tables, and the host statistics
  oracle_host     ``tests/davis_eval_oracle.py``: ``counts`` (boundaries and the brute-force disk dilation in numpy) and ``sequence_stats``
The device tables are checked against the oracle's, entry by entry, before anything is timed.  The bytes are what the kernel has to
read once: the index map and the planes.
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

T, H, W, KP, KG = 70, 480, 854, 5, 3


def make_sequence(seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    recipes = [(rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(30, 90), rng.uniform(40, 120), rng.uniform(-1.5, 1.5, 2))
               for _ in range(KP)]
    shift = rng.integers(-6, 7, (KG, 2))
    pred, gt = np.zeros((T, H, W), np.uint8), np.zeros((KG, T, H, W), np.uint8)
    for t in range(T):
        for k, (cy, cx, ry, rx, v) in enumerate(recipes):
            wob = 1.0 + 0.15 * np.sin(0.3 * t + k)
            pred[t][((yy - cy - v[0] * t) / (ry * wob)) ** 2 + ((xx - cx - v[1] * t) / rx) ** 2 <= 1.0] = k + 1
            if k < KG:
                gt[k, t] = ((yy - cy - v[0] * t - shift[k, 0]) / ry) ** 2 + ((xx - cx - v[1] * t - shift[k, 1]) / (rx * wob)) ** 2 <= 1.0
    return pred, gt


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--oracle-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "davis_eval_bench.json"))
    args = ap.parse_args()
    from stemseg_amd import hip
    from stemseg_amd.evaluation.davis import DavisEvaluator, radius
    from tests import davis_eval_oracle as oracle
    hip.require_gpu()
    pred, gt = make_sequence(9)
    r = radius(H, W)
    assert r == 8 and int(pred.max()) == KP
    p_dev, g_dev = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()

    def oracle_host():
        tab = oracle.counts(pred, gt, KP, r)
        return tab, oracle.sequence_stats(tab, KP, KG)
    oracle_ms = []
    for _ in range(args.oracle_repeats):
        t0 = time.perf_counter()
        want, want_stats = oracle_host()
        oracle_ms.append((time.perf_counter() - t0) * 1e3)
    tables = hip.davis_eval_counts(p_dev, g_dev, KP, r)          # (also the warm-up: code objects, allocator)
    for key, t in zip(hip.DAVIS_EVAL_TABLES, tables):
        assert np.array_equal(t.cpu().numpy().astype(np.int64), want[key]), "table %s differs from the oracle" % key
    stats = DavisEvaluator().add_sequence("bench", p_dev, g_dev, n_proposals=KP)
    assert stats["objects"] == want_stats["objects"], "the evaluator's statistics differ from the oracle's"
    variants = {"counts_kernel": lambda: hip.davis_eval_counts(p_dev, g_dev, KP, r),
                "add_sequence": lambda: DavisEvaluator().add_sequence("bench", p_dev, g_dev, n_proposals=KP)}
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            times[k].append(sync_time(fn)[0])
    times["oracle_host"] = oracle_ms
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    read_bytes = int(pred.nbytes + gt.nbytes)
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "oracle_repeats": args.oracle_repeats,
              "unit": "ms, median of the repeats; host clock around work that ends in a device synchronise (oracle_host: on the host alone)",
              "shape": {"frames": T, "h": H, "w": W, "proposals": KP, "objects": KG, "radius": r,
                        "boundary_pixels_proposals": int(want["n_p"].sum()), "boundary_pixels_objects": int(want["n_g"].sum())},
              "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in times.items()}, "max_ms": {k: round(max(v), 3) for k, v in times.items()},
              "kernel_read_bytes": read_bytes, "kernel_read_gb_per_s": round(read_bytes / (med["counts_kernel"] * 1e-3) / 1e9, 1),
              "oracle_host_over_add_sequence": round(med["oracle_host"] / med["add_sequence"], 1),
              "tables_equal_oracle": True,
              "figures": {"J-Mean": [o["J-Mean"] for o in stats["objects"]], "F-Mean": [o["F-Mean"] for o in stats["objects"]]}}
    print(json.dumps({"median_ms": med}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
