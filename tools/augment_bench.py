#!/usr/bin/env python3
"""Timing of the device augmentation path against the host oracle that defines it (not part of bench.py).

    python tools/augment_bench.py [--repeats 15] [--out profiles/augment_bench.json]

Two samples at dataset sizes, built from a seed:
  coco    one 480 x 640 JPEG with 6 instances -> a clip of 8 frames (the image, mirrored, and 7 warps with jitter, some of them blurred)
  ytvis   a clip of 8 frames of 720 x 1280 JPEG with ONE instance, duplicated (shifted, mirrored copy pasted into every frame)
Per sample, medians over interleaved rounds (both variants once per round), each a host clock around work that ends in a device synchronise:
  device_collate  ``data.common.device_collate`` of the recipe: decode, warp / paste, blur, masked pre-process, mask resize
  host_collate    the same batch entry from tests/augment_oracle.py and tests/data_oracle.py (numpy / torch CPU), then ``.to(device)``
  warp_clip, motion_blur, duplicate_instance   the kernels alone on the decoded frames (parameter upload included)
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stem-seg_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def coco_recipe(T=8, h=480, w=640, instances=6, seed=3):
    from data_loader_bench import make_recipes
    from stemseg_amd.data.image_to_seq_augmenter import ImageToSeqAugmenter
    video = make_recipes(1, 1, h, w, "jpg", instances, None, seed)[0]
    aug = ImageToSeqAugmenter(rotation_range=(-12, 12), perspective_magnitude=0.08, hue_saturation_range=(-5, 5), brightness_range=(-40, 40),
                              motion_blur_prob=0.25, motion_blur_kernel_sizes=(9, 11), translate_range=(-0.1, 0.1))
    random.seed(seed)
    warps = aug.sample_clip(w, h, T - 1)
    rng = random.Random(seed)
    for k, size in ((1, 9), (4, 11)):          # two blurred frames whatever the seed draws
        from stemseg_amd.data.image_to_seq_augmenter import blur_matrix
        warps[k]["blur"] = blur_matrix(size, rng.uniform(0, 360), rng.uniform(-1, 1)).tolist()
    perm = list(range(T))
    random.shuffle(perm)
    strings = [s for _, _, s in sorted(video["rle"])]
    return {"kind": "image", "frames": video["frames"], "rle": strings, "n_instances": len(strings), "has_ignore": False, "flip": True,
            "warps": [{k: wp[k] for k in ("hinv", "add", "hs", "flags", "blur")} for wp in warps], "perm": perm,
            "category_ids": [1] * len(strings), "size": (w, h), "meta_info": {"seq_name": "bench_coco", "category_labels": ["object"] * len(strings)}}


def ytvis_recipe(T=8, h=720, w=1280, seed=5):
    from data_loader_bench import make_recipes
    from stemseg_amd.data.instance_duplicator import InstanceDuplicator, rle_area_and_box
    r = make_recipes(1, T, h, w, "jpg", 1, None, seed)[0]
    boxes = [None] * T
    for _, t, s in r["rle"]:
        boxes[t] = rle_area_and_box(s, h, w)[1]
    random.seed(seed)
    decision = InstanceDuplicator()(boxes, w, h)
    assert decision is not None
    r["duplicate"] = {"boxes": boxes, "flip": True, "shifts": [sh or (0.0, 0.0) for sh in decision["shifts"]]}
    r["category_ids"] = r["category_ids"] + r["category_ids"][-1:]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    from stemseg_amd import config, hip
    from stemseg_amd.data.common import compute_resize_params, device_collate, image_clip_parameters
    from stemseg_amd.structures import ImageList
    from tests import augment_oracle as ao
    from tests import data_oracle as do
    from tests import writer_oracle as wo
    hip.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "unit": "ms, median of interleaved rounds", "workloads": {}}

    def sizes(r, cfg):
        w, h = r["size"]
        new_w, new_h, _ = compute_resize_params((h, w), cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM)
        return (new_h, new_w), ImageList.padded_size([(new_h, new_w)])

    def norm(cfg):
        return cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD, cfg.INPUT.NORMALIZE_TO_UNIT_SCALE, not cfg.INPUT.BGR_INPUT

    # ---- the image sample
    config.load_preset("davis")
    cfg = config.cfg
    cfg.INPUT.NUM_FRAMES = 8
    r = coco_recipe()
    new_hw, pad_hw = sizes(r, cfg)

    def host_image():
        src, planes, ref, blurs = ao.image_recipe_warp(r, do.decode_image)
        frames, _ = ao.motion_blur(ref["frames"], blurs)
        images = ao.preprocess_masked(frames, ref["invalid"], new_hw, pad_hw, *norm(cfg))
        every = ref["planes"].copy()
        every[:, r["perm"].index(0)] = planes
        hard, _ = do.resize_masks(every.reshape(-1, *src.shape[:2]), new_hw, pad_hw)
        return torch.from_numpy(images).to(dev), torch.from_numpy(hard).to(dev)
    frames_dev, _ = hip.decode_frames(r["frames"], dev)
    planes_dev, _ = hip.rle_decode(r["rle"], list(range(len(r["rle"]))), len(r["rle"]), r["size"][1], r["size"][0], dev)
    hinvs, jitter, blurs = image_clip_parameters(r)
    warped = hip.warp_clip(frames_dev[0], planes_dev, hinvs, jitter)[0]
    variants = {"device_collate": lambda: device_collate([r], dev), "host_collate": host_image,
                "warp_clip": lambda: hip.warp_clip(frames_dev[0], planes_dev, hinvs, jitter), "motion_blur": lambda: hip.motion_blur(warped, blurs)}
    result["workloads"]["coco"] = run(variants, args.repeats, dict(h=r["size"][1], w=r["size"][0], T=8, instances=r["n_instances"],
                                                                   blurred=sum(b is not None for b in blurs), resized_to=list(new_hw)))

    # ---- the duplicated clip
    config.load_preset("ytvis")
    cfg = config.cfg
    r2 = ytvis_recipe()
    new_hw2, pad_hw2 = sizes(r2, cfg)
    w2, h2 = r2["size"]
    dup = r2["duplicate"]

    def host_dup():
        frames = np.stack([do.decode_image(f) for f in r2["frames"]])
        mask = np.zeros((len(frames), h2, w2), np.uint8)
        for _, t, s in r2["rle"]:
            mask[t] = wo.decode(wo.string_to_counts(s), h2, w2)
        ref = ao.duplicate_instance(frames, mask, dup["boxes"], dup["flip"], dup["shifts"])
        images = ao.preprocess_masked(ref["frames"], np.zeros(mask.shape, np.uint8), new_hw2, pad_hw2, *norm(cfg))
        hard, _ = do.resize_masks(ref["masks"].reshape(-1, h2, w2), new_hw2, pad_hw2)
        return torch.from_numpy(images).to(dev), torch.from_numpy(hard).to(dev)
    frames2, _ = hip.decode_frames(r2["frames"], dev)
    mask2, _ = hip.rle_decode([s for _, _, s in r2["rle"]], [t for _, t, _ in r2["rle"]], len(r2["frames"]), h2, w2, dev)
    variants = {"device_collate": lambda: device_collate([r2], dev), "host_collate": host_dup,
                "duplicate_instance": lambda: hip.duplicate_instance(frames2, mask2, dup["boxes"], dup["flip"], dup["shifts"])}
    result["workloads"]["ytvis_duplicated"] = run(variants, args.repeats, dict(h=h2, w=w2, T=len(r2["frames"]), resized_to=list(new_hw2)))
    config.load_preset("defaults")
    result["device_not_slower"] = all(wl["device_not_slower"] for wl in result["workloads"].values())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print("wrote", args.out)


def run(variants, repeats, shape):
    for fn in variants.values():          # warm-up: code objects, allocator, PIL
        fn()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            times[k].append(sync_time(fn)[0])
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out = {"shape": shape, "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in times.items()},
           "max_ms": {k: round(max(v), 3) for k, v in times.items()}, "host_over_device_collate": round(med["host_collate"] / med["device_collate"], 2),
           "device_not_slower": bool(med["device_collate"] <= med["host_collate"])}
    print(json.dumps(out["median_ms"]), flush=True)
    return out


if __name__ == "__main__":
    main()
