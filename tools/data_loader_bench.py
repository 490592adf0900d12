#!/usr/bin/env python3
"""Timing of the training data loader's device path against the host path it replaces (not part of bench.py).

    python tools/data_loader_bench.py [--repeats 7] [--out profiles/data_loader_bench.json]

Two batches at dataset sizes, built from a seed (moving ellipses, smooth frames written with PIL):
  ytvis   2 clips x 8 frames of 720 x 1280 JPEG, 6 instances each, no ignore region     (preset ytvis:  640 / 1196)
  kitti   1 clip  x 8 frames of 375 x 1242 PNG, 20 instances + the ignore instance      (preset kittimots: 736 / 1792)
Per batch, medians over interleaved repeats (every variant once per round, so that a busy neighbour hits all of them alike), each a host
clock around work that ends in a device synchronise:
  rle_decode      ``hip.rle_decode`` alone, all strings of the batch (packing and the upload of the characters included)
  resize_masks    ``hip.resize_masks`` alone, per sample, on the decoded planes
  device_masks    the two together: strings -> padded targets on the device
  host_masks      tests/data_oracle.py: numpy decode + torch-CPU interpolate + threshold + pad, then ``.to(device)``
  device_collate  ``data.common.device_collate`` whole (image decode and pre-processing included)
  host_collate    the oracle's whole batch (PIL decode, torch-CPU interpolate and normalise, masks as above), then ``.to(device)``
"""
import argparse
import io
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

WORKLOADS = {"ytvis": dict(preset="ytvis", clips=2, T=8, h=720, w=1280, ext="jpg", instances=6, ignore=None),
             "kitti": dict(preset="kittimots", clips=1, T=8, h=375, w=1242, ext="png", instances=21, ignore=("instance", 20))}


def make_recipes(clips, T, h, w, ext, instances, ignore, seed):
    from PIL import Image
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    recipes = []
    for c in range(clips):
        tracks = [(rs.uniform(0.15, 0.85) * h, rs.uniform(0.1, 0.9) * w, rs.uniform(0.04, 0.15) * h, rs.uniform(0.03, 0.12) * w,
                   rs.uniform(-4, 4), rs.uniform(-6, 6)) for _ in range(instances)]
        frames, rle = [], []
        for t in range(T):
            img = np.stack([127 + 90 * np.sin(yy / (40.0 + 9 * k) + 0.2 * t + c) * np.cos(xx / (60.0 + 7 * k) - 0.1 * t) for k in range(3)], -1)
            buf = io.BytesIO()
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, "JPEG" if ext == "jpg" else "PNG", **({"quality": 90} if ext == "jpg" else {}))
            frames.append(buf.getvalue())
            for i, (cy, cx, ry, rx, vy, vx) in enumerate(tracks):
                m = ((yy - cy - vy * t) / ry) ** 2 + ((xx - cx - vx * t) / rx) ** 2 <= 1.0
                if ignore is not None and i == ignore[1]:
                    m = (yy > 0.93 * h) | (xx < 0.02 * w)          # (the "don't care" border of a KITTI frame)
                if m.any():
                    rle.append((i, t, mask_string(m)))
        n_targets = instances - (1 if ignore is not None else 0)
        recipes.append({"frames": frames, "rle": rle, "n_instances": instances, "category_ids": [1 + i % 2 for i in range(n_targets)],
                        "ignore": ignore, "size": (w, h), "meta_info": {"seq_name": "bench_%d" % c}})
    return recipes


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_loader_bench.json"))
    args = ap.parse_args()
    from stemseg_amd import config, hip
    from stemseg_amd.data.common import plane_layout, compute_resize_params, device_collate
    from stemseg_amd.structures import ImageList
    from tests import data_oracle as do
    hip.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "unit": "ms, median of interleaved repeats", "workloads": {}}
    for name, wl in WORKLOADS.items():
        wl = dict(wl)
        config.load_preset(wl.pop("preset"))
        cfg = config.cfg
        recipes = make_recipes(seed=len(name), **wl)
        T, h, w = wl["T"], wl["h"], wl["w"]
        new_w, new_h, _ = compute_resize_params((h, w), cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM)
        pad_hw = ImageList.padded_size([(new_h, new_w)])
        strings, plane_idx, base = [], [], 0
        for r in recipes:
            order, _ = plane_layout(r)
            slot = {inst: j for j, inst in enumerate(order)}
            for inst, t, s in r["rle"]:
                strings.append(s)
                plane_idx.append(base + slot[inst] * T + t)
            base += r["n_instances"] * T
        per_sample = recipes[0]["n_instances"] * T

        def decode():
            return hip.rle_decode(strings, plane_idx, base, h, w, dev)

        def resize(planes):
            return [hip.resize_masks(planes[k * per_sample:(k + 1) * per_sample], (new_h, new_w), pad_hw) for k in range(len(recipes))]

        def host(with_images):
            out = do.collate(recipes, cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD, with_images=with_images)
            moved = [torch.from_numpy(t[k]).to(dev) for t in out["targets"] for k in ("masks", "ignore_masks")]
            if with_images:
                moved.append(torch.from_numpy(out["images"]).to(dev))
            return moved
        variants = {"rle_decode": decode, "resize_masks": None, "device_masks": lambda: resize(decode()[0]), "host_masks": lambda: host(False),
                    "device_collate": lambda: device_collate(recipes, dev), "host_collate": lambda: host(True)}
        planes, status = decode()
        assert not bool(status.any()), "the synthetic strings must decode"
        variants["resize_masks"] = lambda: resize(planes)
        # the two paths agree (tie rule of the tests) before anything is timed
        ref = do.collate(recipes, cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD, with_images=False)
        got = device_collate(recipes, dev)[1]
        differing = 0
        for t_dev, t_ref in zip(got, ref["targets"]):
            differing += do.check_tie_rule(t_dev["masks"].cpu().numpy().reshape((-1,) + tuple(pad_hw)), t_ref["masks"].reshape((-1,) + tuple(pad_hw)),
                                           t_ref["soft_masks"].reshape(-1, new_h, new_w), (new_h, new_w), name)
            differing += do.check_tie_rule(t_dev["ignore_masks"].cpu().numpy(), t_ref["ignore_masks"], t_ref["soft_ignore"], (new_h, new_w), name)
        for fn in variants.values():          # warm-up: code objects, allocator, PIL
            fn()
        times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                times[k].append(sync_time(fn)[0])
        med = {k: round(statistics.median(v), 3) for k, v in times.items()}
        result["workloads"][name] = {
            "shape": dict(wl, ignore=bool(wl["ignore"]), strings=len(strings), characters=sum(map(len, strings)), planes=base, resized_to=[new_h, new_w], padded_to=list(pad_hw)),
            "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in times.items()}, "max_ms": {k: round(max(v), 3) for k, v in times.items()},
            "mask_pixels_differing_in_tie_band": differing,
            "host_over_device_masks": round(med["host_masks"] / med["device_masks"], 2),
            "host_over_device_collate": round(med["host_collate"] / med["device_collate"], 2),
            "device_not_slower": bool(med["device_masks"] <= med["host_masks"] and med["device_collate"] <= med["host_collate"])}
        print(name, json.dumps(result["workloads"][name]["median_ms"]), flush=True)
    config.load_preset("defaults")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
