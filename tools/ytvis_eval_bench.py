#!/usr/bin/env python3
"""Timing of the YouTube-VIS evaluation on the device: the run-walking ``rle_pair_inter`` next to the rasterising alternative on the same
GPU and to the numpy oracle on the host (not part of bench.py).

    python tools/ytvis_eval_bench.py [--repeats 9] [--oracle-repeats 1] [--out profiles/ytvis_eval_bench.json]

One synthetic video at the size of a YouTube-VIS one, built from a seed: 36 frames of 720 x 1280, 10 result tracks and 3 ground-truth
tracks (drifting ellipses with a ragged edge; three categories, so that every result meets the one ground-truth track of its category in
every frame both have a mask), all as COCO RLE strings.  Each figure is a host clock around work that ends in a device synchronise (the
device rows) or in the result (the host row); medians over the repeats, after a warm-up call.
  rle_pair_inter       ``hip.rle_pair_inter`` of the video's strings and pairs: staging, the 15 launches, the tables left on the device
  add_video            ``YtvisEvaluator.add_video``: packing, that one call, the one read-back, the matching on the host
  raster_pairs_loop    the rasterising alternative: ``hip.rle_decode`` of the same strings into one plane each, then per pair
                       ``(planes[a] & planes[b]).sum()`` and per string ``planes[m].sum()`` in torch, results left on the device
  raster_pairs_batched the same with ONE gather / ``&`` / ``sum`` over all pairs instead of a loop (more memory: two planes per pair)
  oracle_host          ``tests/ytvis_eval_oracle.py``: ``video_records`` on dense numpy masks
The kernel's tables are checked against the rasterised ones and the evaluator's records against the oracle's before anything is timed.
No timing is a pass criterion.
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

from tests.data_oracle import mask_string  # noqa: E402

T, H, W, N_RES, N_GT = 36, 720, 1280, 10, 3


def make_video(seed):
    """-> (result tracks, ground-truth tracks): ellipses that drift; a result is its category's ground truth moved and rescaled, so the
    IoUs spread over the thresholds; every track misses a frame now and then."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]

    def ellipse(cy, cx, ry, rx):
        m = ((yy - cy) / float(ry)) ** 2 + ((xx - cx) / float(rx)) ** 2 <= 1.0
        m[::7, ::8] &= ((yy[::7, ::8] - cy) / float(ry)) ** 2 + ((xx[::7, ::8] - cx) / float(rx)) ** 2 <= 0.8          # a ragged edge
        return m
    base = [(200 + 160 * g, 250 + 380 * g, 90 + 30 * g, 150 + 40 * g, float(rng.uniform(-1.5, 1.5)), float(rng.uniform(2, 5))) for g in range(N_GT)]
    gt, res = [], []
    for g, (cy, cx, ry, rx, vy, vx) in enumerate(base):
        segs = [None if (t + 5 * g) % 17 == 16 else {"size": [H, W], "counts": mask_string(ellipse(cy + vy * t, cx + vx * t, ry, rx))}
                for t in range(T)]
        gt.append({"category_id": g + 1, "iscrowd": 0, "segmentations": segs})
    for k in range(N_RES):
        cy, cx, ry, rx, vy, vx = base[k % N_GT]
        dy, dx, scale = float(rng.uniform(-40, 40)) * (k // N_GT), float(rng.uniform(-60, 60)) * (k // N_GT), float(rng.uniform(0.7, 1.2))
        segs = [None if (t + 3 * k) % 13 == 12 else
                {"size": [H, W], "counts": mask_string(ellipse(cy + vy * t + dy, cx + vx * t + dx, ry * scale, rx * scale))} for t in range(T)]
        res.append({"video_id": "bench", "score": float(rng.uniform(0.1, 1.0)), "category_id": k % N_GT + 1, "segmentations": segs})
    return res, gt


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--oracle-repeats", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ytvis_eval_bench.json"))
    args = ap.parse_args()
    from stemseg_amd import hip
    from stemseg_amd.evaluation import ytvis
    from tests import ytvis_eval_oracle as oracle
    hip.require_gpu()
    res, gt = make_video(13)
    oracle_ms = []
    for _ in range(args.oracle_repeats):
        t0 = time.perf_counter()
        want = oracle.video_records(res, gt, (H, W))
        oracle_ms.append((time.perf_counter() - t0) * 1e3)
    ev = ytvis.YtvisEvaluator()
    got = ev.add_video("bench", res, gt, (H, W))                                   # (also the warm-up: code objects, allocator)
    for c in want:
        assert got[c]["scores"] == want[c]["scores"] and got[c]["matched"].tolist() == want[c]["matched"] and \
            got[c]["ignored"].tolist() == want[c]["ignored"], "the evaluator's records differ from the oracle's"
    summary = ev.summary()
    ref = oracle.summary({"bench": want})
    assert all(summary[k] == ref[k] for k in ytvis.FIGURES)

    # the strings and the pairs as the evaluator lists them: frame by frame, results then ground truth
    strings, index = [], {}
    for t in range(T):
        for side, tracks in enumerate((res, gt)):
            for n, tr in enumerate(tracks):
                if tr["segmentations"][t] is not None:
                    index[(side, n, t)] = len(strings)
                    strings.append(tr["segmentations"][t]["counts"])
    pairs = [(index[(0, d, t)], index[(1, g, t)]) for t in range(T) for d in range(N_RES) for g in range(N_GT)
             if res[d]["category_id"] == gt[g]["category_id"] and (0, d, t) in index and (1, g, t) in index]
    M, K = len(strings), len(pairs)
    pa = torch.tensor([p[0] for p in pairs], device="cuda")
    pb = torch.tensor([p[1] for p in pairs], device="cuda")

    def raster_loop():
        planes = hip.rle_decode(strings, list(range(M)), M, H, W)[0]
        inter = torch.stack([(planes[a] & planes[b]).sum() for a, b in pairs])
        return torch.stack([planes[m].sum() for m in range(M)]), inter

    def raster_batched():
        planes = hip.rle_decode(strings, list(range(M)), M, H, W)[0]
        return planes.sum(dim=(1, 2)), (planes[pa] & planes[pb]).sum(dim=(1, 2))
    area, inter, status = hip.rle_pair_inter(strings, pairs, H, W)
    for fn in (raster_loop, raster_batched):
        r_area, r_inter = fn()
        assert torch.equal(area.long(), r_area.long()) and torch.equal(inter.long(), r_inter.long()) and not bool(status.any()), \
            "rle_pair_inter differs from the rasterised planes"
    variants = {"rle_pair_inter": lambda: hip.rle_pair_inter(strings, pairs, H, W),
                "add_video": lambda: ytvis.YtvisEvaluator().add_video("bench", res, gt, (H, W)),
                "raster_pairs_loop": raster_loop, "raster_pairs_batched": raster_batched}
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            times[k].append(sync_time(fn)[0])
            torch.cuda.empty_cache()                                               # the batched variant's gather is large
    times["oracle_host"] = oracle_ms
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    n_chars = sum(len(s) for s in strings)
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "oracle_repeats": args.oracle_repeats,
              "unit": "ms, median of the repeats; host clock around work that ends in a device synchronise (oracle_host: on the host alone)",
              "shape": {"frames": T, "h": H, "w": W, "result_tracks": N_RES, "gt_tracks": N_GT, "strings": M, "pairs": K, "chars": n_chars,
                        "chars_per_string": round(n_chars / float(M), 1),
                        "workspace_bytes": hip.rle_pair_inter_workspace_bytes(n_chars, M, K), "raster_plane_bytes": M * H * W,
                        "raster_batched_gather_bytes": 2 * K * H * W},
              "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in times.items()}, "max_ms": {k: round(max(v), 3) for k, v in times.items()},
              "raster_pairs_loop_over_rle_pair_inter": round(med["raster_pairs_loop"] / med["rle_pair_inter"], 1),
              "raster_pairs_batched_over_rle_pair_inter": round(med["raster_pairs_batched"] / med["rle_pair_inter"], 1),
              "oracle_host_over_add_video": round(med["oracle_host"] / med["add_video"], 1),
              "tables_equal_rasterised": True, "records_equal_oracle": True,
              "figures": {k: summary[k] for k in ytvis.FIGURES},
              "not_measured": "device time by events or a profiler (these are host clocks, launch and staging included); several videos; "
                              "real YouTube-VIS annotations; the official toolkit"}
    print(json.dumps({"median_ms": med}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
