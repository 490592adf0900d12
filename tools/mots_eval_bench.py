#!/usr/bin/env python3
"""Timing of the KITTI-MOTS evaluation on the device next to the numpy oracle on the host (not part of bench.py).

    python tools/mots_eval_bench.py [--repeats 9] [--oracle-repeats 1] [--out profiles/mots_eval_bench.json]

One synthetic sequence at the size of a KITTI-MOTS one, built from a seed: 300 frames of 375 x 1242, 12 result tracks (drifting boxes
with a wobbling edge; cars and pedestrians), 10 ground-truth objects (the first ten results shifted by a few pixels) and an ignore
region, all as COCO RLE strings.  Each figure is a host clock around work that ends in a device synchronise (the device rows) or in the
result (the host row); medians over the repeats, after a warm-up call.
  rle_decode_labels   ``hip.rle_decode_labels`` of the results of one chunk of 128 frames: staging, the 16 launches, maps left on the device
  label_pair_counts   ``hip.label_pair_counts`` of that chunk's two label maps: the fill launch and the counting launch
  add_sequence        ``MotsEvaluator.add_sequence`` of the 300 frames: per chunk two decodes, one count, one read-back, the host half
  oracle_host         ``tests/mots_eval_oracle.py``: ``sequence_counts`` on dense numpy masks
The evaluator's counts are checked against the oracle's before anything is timed.  No timing is a pass criterion.
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

T, H, W, N_RES, N_GT = 300, 375, 1242, 12, 10


def make_sequence(seed):
    """-> (result records, ground-truth records): objects in their own vertical lanes of the frame, so that the masks of a side are
    disjoint whatever the drift."""
    rng = np.random.default_rng(seed)
    lane = W // (N_RES + 1)
    res, gt = [], []
    ignore = np.zeros((H, W), np.uint8)
    ignore[:, (N_RES - 1) * lane:N_RES * lane] = 1
    ignore_string = mask_string(ignore)
    for k in range(N_RES):
        cls = 1 if k % 3 else 2
        y0, hh, ww = int(rng.integers(70, 200)), int(rng.integers(40, 150)), int(rng.integers(lane // 3, lane - 12))
        vy, dy, dx = float(rng.uniform(-0.2, 0.2)), int(rng.integers(-4, 5)), int(rng.integers(-4, 5))
        for t in range(T):
            if (t + 7 * k) % 41 == 0:                                              # every track misses a frame now and then
                continue
            m = np.zeros((H, W), np.uint8)
            y = int(y0 + vy * t)
            x = k * lane + 6 + int(3 * np.sin(0.1 * t + k))
            m[y:y + hh, x:x + ww] = 1
            m[y:y + hh:3, x + ww - 2:x + ww] = 0                                   # a ragged edge: more runs per string
            res.append((t, (k + 1) if t < 200 or k % 4 else (k + 51), cls, H, W, mask_string(m)))          # some tracks change id at t = 200
            if k < N_GT:
                g = np.zeros((H, W), np.uint8)
                g[max(0, y + dy):y + dy + hh, max(k * lane, x + dx):min((k + 1) * lane, x + dx + ww)] = 1
                gt.append((t, cls * 1000 + k, cls, H, W, mask_string(g)))
    gt += [(t, 10000, 10, H, W, ignore_string) for t in range(T)]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mots_eval_bench.json"))
    args = ap.parse_args()
    from stemseg_amd import hip
    from stemseg_amd.evaluation import mots
    from tests import mots_eval_oracle as oracle
    hip.require_gpu()
    res, gt = make_sequence(11)
    oracle_ms = []
    for _ in range(args.oracle_repeats):
        t0 = time.perf_counter()
        want = oracle.sequence_counts(res, gt, T)
        oracle_ms.append((time.perf_counter() - t0) * 1e3)
    ev = mots.MotsEvaluator()
    got = ev.add_sequence("bench", res, gt, T)                                     # (also the warm-up: code objects, allocator)
    for cls in ("car", "ped"):
        assert {k: got[cls][k] for k in oracle.KEYS} == {k: want[cls][k] for k in oracle.KEYS}, "the evaluator's counts differ from the oracle's"
    summary = ev.summary()
    assert all(summary[k] == v for k, v in oracle.summary({"bench": want}).items())

    # one chunk of CHUNK_FRAMES frames, labelled as the evaluator labels it
    chunk = mots.CHUNK_FRAMES

    def side(records, keep):
        frames = [[] for _ in range(chunk)]
        for r in records:
            if r[0] < chunk and r[2] in keep:
                frames[r[0]].append(r)
        items = [(t, n, r[5]) for t, rs in enumerate(frames) for n, r in enumerate(sorted(rs, key=lambda r: r[1]), 1)]
        return [s for _, _, s in items], [t for t, _, _ in items], [n for _, n, _ in items], max(len(rs) for rs in frames)
    rs, gs = side(res, (1, 2)), side(gt, (1, 2, 10))
    decode = lambda s: hip.rle_decode_labels(s[0], s[1], s[2], chunk, H, W)
    map_r, map_g = decode(rs)[0], decode(gs)[0]
    variants = {"rle_decode_labels": lambda: decode(rs),
                "label_pair_counts": lambda: hip.label_pair_counts(map_r, map_g, rs[3], gs[3]),
                "add_sequence": lambda: mots.MotsEvaluator().add_sequence("bench", res, gt, T)}
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            times[k].append(sync_time(fn)[0])
    times["oracle_host"] = oracle_ms
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    pair_bytes = int(2 * 2 * chunk * H * W)
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "oracle_repeats": args.oracle_repeats,
              "unit": "ms, median of the repeats; host clock around work that ends in a device synchronise (oracle_host: on the host alone)",
              "shape": {"frames": T, "h": H, "w": W, "result_tracks": N_RES, "objects": N_GT, "ignore_regions": 1, "chunk_frames": chunk,
                        "result_strings": len(res), "gt_strings": len(gt), "result_strings_in_chunk": len(rs[0]),
                        "result_chars_in_chunk": sum(len(s) for s in rs[0])},
              "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in times.items()}, "max_ms": {k: round(max(v), 3) for k, v in times.items()},
              "label_pair_counts_read_bytes": pair_bytes, "label_pair_counts_read_gb_per_s": round(pair_bytes / (med["label_pair_counts"] * 1e-3) / 1e9, 1),
              "oracle_host_over_add_sequence": round(med["oracle_host"] / med["add_sequence"], 1),
              "counts_equal_oracle": True,
              "figures": {k: v for k, v in summary.items() if k not in ("sequences",)}}
    print(json.dumps({"median_ms": med}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
