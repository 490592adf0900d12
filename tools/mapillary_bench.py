#!/usr/bin/env python3
"""Timing of the Mapillary path's union decode against what the library could do without it (not part of bench.py).

    python tools/mapillary_bench.py [--repeats 7] [--out profiles/mapillary_bench.json]

One synthetic sample at the size of a Mapillary Vistas image, built from a seed: a 2448 x 3264 JPEG, 30 target strings and 90 ignore
strings of ellipses in the cells of a 10 x 12 grid -- non-overlapping, as the segments of a panoptic annotation.  Medians over
interleaved repeats (every variant once per round), each a host clock around work that ends in a device synchronise; the bytes are the
peak of torch's allocator above what was allocated before the call:
  union_decode    ``hip.rle_decode_union`` of the 120 strings into 31 planes (packing and the upload of the characters included)
  planes_then_any ``hip.rle_decode`` of the same strings into 120 planes, then ``torch.any`` over the 90 and a concatenation: the same
                  31 planes by the entry point the library had before
  device_collate  ``data.common.device_collate`` of the one sample under the ``kittimots_1`` preset (8 frames, 736 / 1248): decode, warp
                  at the source resolution, pre-process, resize
"""
import argparse
import io
import json
import os
import random
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

H, W, ROWS, COLS, TARGETS = 2448, 3264, 10, 12, 30


def make_sample(seed):
    """-> (JPEG bytes, the 120 strings in descending order of area: the first 30 are the targets)."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float32)
    img = np.stack([127 + 90 * np.sin(yy / (40.0 + 9 * k)) * np.cos(xx / (60.0 + 7 * k)) for k in range(3)], -1)
    buf = io.BytesIO()
    Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=90)
    ch, cw = H // ROWS, W // COLS
    blobs = []
    for r in range(ROWS):
        for c in range(COLS):
            ry, rx = rs.uniform(0.15, 0.48) * ch, rs.uniform(0.15, 0.48) * cw
            cy, cx = (r + 0.5) * ch, (c + 0.5) * cw
            y0, x0 = r * ch, c * cw
            cell = ((yy[y0:y0 + ch, x0:x0 + cw] - cy) / ry) ** 2 + ((xx[y0:y0 + ch, x0:x0 + cw] - cx) / rx) ** 2 <= 1.0
            # a wavy outline, so that a column holds more than one run
            cell &= (np.sin(yy[y0:y0 + ch, x0:x0 + cw] / 6.0 + c) * np.cos(xx[y0:y0 + ch, x0:x0 + cw] / 9.0 + r) > -0.6)
            m = np.zeros((H, W), bool)
            m[y0:y0 + ch, x0:x0 + cw] = cell
            blobs.append((int(cell.sum()), mask_string(m)))
    blobs.sort(key=lambda b: -b[0])
    return buf.getvalue(), [s for _, s in blobs]


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_bytes(fn):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapillary_bench.json"))
    args = ap.parse_args()
    from stemseg_amd import config, hip
    from stemseg_amd.data.common import device_collate
    from stemseg_amd.data.image_to_seq_augmenter import ImageToSeqAugmenter
    hip.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    config.load_preset("kittimots_1")
    T = config.cfg.INPUT.NUM_FRAMES
    jpeg, strings = make_sample(5)
    M, P = len(strings), TARGETS + 1
    union_idx = list(range(TARGETS)) + [TARGETS] * (M - TARGETS)

    def union_decode():
        return hip.rle_decode_union(strings, union_idx, P, H, W, dev)[0]

    def planes_then_any():
        planes = hip.rle_decode(strings, list(range(M)), M, H, W, dev)[0]
        return torch.cat([planes[:TARGETS], planes[TARGETS:].any(0, keepdim=True).to(torch.uint8)], 0)
    a, b = union_decode(), planes_then_any()
    assert torch.equal(a, b) and bool(a[TARGETS].any()), "the two forms must give the same 31 planes"
    del a, b
    random.seed(5)
    aug = ImageToSeqAugmenter(perspective=True, affine=True, motion_blur=True, rotation_range=(-10, 10), perspective_magnitude=0.08,
                              hue_saturation_range=(-5, 5), brightness_range=(-40, 40), motion_blur_prob=0.0, translate_range=(-0.1, 0.1))
    recipe = {"kind": "image", "frames": [jpeg], "rle": strings, "rle_planes": union_idx, "n_instances": TARGETS, "has_ignore": True, "flip": False,
              "warps": [{k: w[k] for k in ("hinv", "add", "hs", "flags", "blur")} for w in aug.sample_clip(W, H, T - 1)], "perm": list(range(T)),
              "category_ids": [1 + i % 2 for i in range(TARGETS)], "size": (W, H), "meta_info": {"seq_name": "bench", "category_labels": []}}
    variants = {"union_decode": union_decode, "planes_then_any": planes_then_any, "device_collate": lambda: device_collate([recipe], dev)}
    for fn in variants.values():          # warm-up: code objects, allocator
        fn()
    torch.cuda.empty_cache()
    memory = {k: peak_bytes(fn) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            times[k].append(sync_time(fn)[0])
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "unit": "ms, median of interleaved repeats; bytes: allocator peak above the start",
              "shape": {"h": H, "w": W, "strings": M, "characters": sum(map(len, strings)), "target_strings": TARGETS, "ignore_strings": M - TARGETS,
                        "planes": P, "frames": T, "min_dim": config.cfg.INPUT.MIN_DIM, "max_dim": config.cfg.INPUT.MAX_DIM},
              "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in times.items()}, "max_ms": {k: round(max(v), 3) for k, v in times.items()},
              "peak_bytes": memory, "planes_then_any_over_union_ms": round(med["planes_then_any"] / med["union_decode"], 2),
              "planes_then_any_over_union_bytes": round(memory["planes_then_any"] / float(memory["union_decode"]), 2)}
    print(json.dumps({"median_ms": med, "peak_bytes": memory}), flush=True)
    config.load_preset("defaults")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
