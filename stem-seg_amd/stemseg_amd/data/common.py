"""What the reference's data/common.py gives the training loop -- ``compute_resize_params``, ``compute_padding``, ``targets_to``,
``collate_fn`` -- and ``device_collate``, which does the reference's ``VideoDataset.__getitem__`` + ``collate_fn`` arithmetic on the device.

A ``DataLoader`` runs ``__getitem__`` and its collate function inside worker processes, and no worker may open the GPU.  So a dataset's
``__getitem__`` returns a host *recipe* (a dict of bytes / str / int / list):

    frames        the T files' bytes
    rle           [(instance, frame, string)]: the COCO RLE annotations there are; (instance, frame) pairs without one are zero masks
    n_instances   planes per frame, the ignore instance included
    category_ids  one per instance that is a target
    ignore        None (zero ignore masks) | "background" (1 - union of the instances, DAVIS) | ("instance", i) (instance i, KITTI-MOTS)
    size          (width, height) of the frames
    meta_info     {"seq_name": ...}
    rle_planes    image recipes only, optional (mapillary_data_loader.py): the plane of each string of ``rle``, non-decreasing; strings that
                  name one plane are OR-ed into it

and ``device_collate(recipes)`` runs in the consuming process: per sample one ``decode_frames`` and one ``preprocess_frames``, per frame
size of the batch one ``rle_decode`` over every string of that size (and one ``rle_decode_union`` over the strings of the image recipes
that carry ``"rle_planes"``, Mapillary's, whose last plane is the union of many strings), per sample one ``resize_masks``.  Every upload of the mask path
(strings with their tables, category ids) goes through pinned memory without waiting, so that path synchronises once per batch, for the
strings' status bytes; ``decode_frames`` reads its decoders' status back once per sample on top of that."""
import math

import numpy as np
import torch

from ..config import cfg
from ..structures import ImageList


def compute_resize_params(image, min_dim, max_dim):
    """image: an array [H, W, ...] or its (H, W).  -> (new_width, new_height, scale_factor): the short side to ``min_dim`` unless that takes
    the long side beyond ``max_dim``, then the long side to ``max_dim``; sizes by Python's round."""
    height, width = (image.shape if hasattr(image, "shape") else image)[:2]
    low, high = float(min(height, width)), float(max(height, width))
    scale = min_dim / low
    if high * scale > max_dim:
        scale = max_dim / high
    return round(scale * width), round(scale * height), scale


def compute_padding(width, height):
    """-> (pad_right, pad_bottom) up to the next multiples of 32."""
    return int(math.ceil(width / 32)) * 32 - width, int(math.ceil(height / 32)) * 32 - height


def targets_to(targets, *args, **kwargs):
    return [{k: (v.to(*args, **kwargs) if torch.is_tensor(v) else v) for k, v in per_seq.items()} for per_seq in targets]


def collate_fn(samples):
    """The reference's collate for samples that are already tensors: (images [T,3,H,W], targets, (width, height), meta_info) each ->
    (ImageList, targets with masks zero-padded to the batch size, meta_infos)."""
    image_seqs, targets, original_dims, meta_info = zip(*samples)
    image_seqs = ImageList.from_image_sequence_list(image_seqs, original_dims)
    ph, pw = image_seqs.max_size
    for t in targets:
        h, w = t["masks"].shape[-2:]
        t["masks"] = torch.nn.functional.pad(t["masks"], (0, pw - w, 0, ph - h))
        t["ignore_masks"] = torch.nn.functional.pad(t["ignore_masks"], (0, pw - w, 0, ph - h))
    return image_seqs, targets, meta_info


def plane_layout(recipe):
    """-> (order: instance positions in plane order, the ignore instance last; n_targets).  Plane of (instance order[j], frame t) = j * T + t."""
    order = list(range(recipe["n_instances"]))
    ignore = recipe["ignore"]
    if isinstance(ignore, tuple):
        order.remove(ignore[1])
        order.append(ignore[1])
        return order, len(order) - 1
    return order, len(order)


def clip_length(recipe):
    return len(recipe["perm"]) if recipe.get("kind") == "image" else len(recipe["frames"])


def mirrored_hinv(hinv, width):
    """The inverse homography that reads the MIRRORED source: u -> (W - 1) - u, folded into the first row (fp64)."""
    h = np.asarray(hinv, np.float64).reshape(3, 3).copy()
    h[0] = (width - 1) * h[2] - h[0]
    return h


def image_clip_parameters(recipe):
    """An image recipe -> (hinv [T, 3, 3], jitter [T, 3], blur matrices [T]) in the clip's FINAL frame order: slot k shows frame
    ``perm[k]`` -- 0 is the image itself, f > 0 its warp f - 1 -- so the permutation costs no copy; with ``flip`` every frame reads the
    mirrored source."""
    hinvs, jitter, blurs = [], [], []
    for src in recipe["perm"]:
        warp = recipe["warps"][src - 1] if src > 0 else {"hinv": np.eye(3), "add": 0, "hs": 0, "flags": 0, "blur": None}
        h = np.asarray(warp["hinv"], np.float64).reshape(3, 3)
        hinvs.append(mirrored_hinv(h, recipe["size"][0]) if recipe["flip"] else h)
        jitter.append((warp["add"], warp["hs"], warp["flags"]))
        blurs.append(None if warp["blur"] is None else np.asarray(warp["blur"], np.float32))
    return np.stack(hinvs), np.asarray(jitter, np.int32), blurs


def _preprocess(hip, frames, new_hw, pad_hw, invalid=None):
    return hip.preprocess_frames(frames, new_hw, pad_hw, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD, unit_scale=cfg.INPUT.NORMALIZE_TO_UNIT_SCALE,
                                 flip_channels=not cfg.INPUT.BGR_INPUT, invalid=invalid)


def _collate_image_sample(hip, r, planes, T, new_hw, pad_hw, dev):
    """One image recipe -> (images float32 [T,3,ph,pw], masks uint8 [N,T,ph,pw], ignore_masks uint8 [T,ph,pw]): decode the one file,
    warp it T times in one launch (the image itself is the identity warp), blur, masked pre-process; the masks of the warped frames come
    from the condensed planes, those of the image itself from its own planes, overlaps kept, as in the reference."""
    N, P = r["n_instances"], r["n_instances"] + int(r["has_ignore"])
    frames, _ = hip.decode_frames(r["frames"], dev)
    if tuple(frames.shape[1:3]) != (r["size"][1], r["size"][0]):
        raise ValueError("image %s: the file is %s, the dataset says %s" % (r["meta_info"]["seq_name"], tuple(frames.shape[1:3]),
                                                                          (r["size"][1], r["size"][0])))
    hinvs, jitter, blurs = image_clip_parameters(r)
    warped, warped_planes, invalid = hip.warp_clip(frames[0], planes if P else None, hinvs, jitter)
    warped = hip.motion_blur(warped, blurs)
    images = _preprocess(hip, warped, new_hw, pad_hw, invalid)
    zeros = lambda *shape: torch.zeros(shape + tuple(pad_hw), dtype=torch.uint8, device=dev)
    if P == 0:          # (a Mapillary sample whose largest instances hold no target, and nothing to ignore either)
        return images, zeros(0, T), zeros(T)
    out = hip.resize_masks(warped_planes.view(P * T, *warped_planes.shape[2:]), new_hw, pad_hw).view(P, T, pad_hw[0], pad_hw[1])
    out[:, r["perm"].index(0)] = hip.resize_masks(planes, new_hw, pad_hw, flip_x=r["flip"])
    return images, out[:N], (out[N] if r["has_ignore"] else zeros(T))


def device_collate(recipes, device=None):
    """Recipes -> (ImageList, targets, meta_info) on the device: ``targets[n]`` = {"masks": uint8 [I,T,H,W], "ignore_masks": uint8 [T,H,W],
    "category_ids": int64 [I]} at the batch's padded size, what ``Trainer`` and ``TrainingModel`` take.  A batch may mix video recipes
    and image recipes (``"kind": "image"``, coco_data_loader.py); a video recipe with a ``"duplicate"`` decision (instance_duplicator.py)
    gets its lone instance pasted a second time between the decode and the resize.  A refused annotation string raises ValueError naming
    the sequence and the frame."""
    from .. import hip
    hip.require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    T = clip_length(recipes[0])
    is_image = [r.get("kind") == "image" for r in recipes]
    sizes, new_sizes = [], []
    for r in recipes:
        if clip_length(r) != T:
            raise ValueError("All sequences must contain the same number of images. Found {} and {}".format(T, clip_length(r)))
        width, height = r["size"]
        new_w, new_h, _ = compute_resize_params((height, width), cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM)
        sizes.append((height, width))
        new_sizes.append((new_h, new_w))
    pad_hw = ImageList.padded_size(new_sizes)

    # one decode call per frame size, over every string of the batch that has it
    groups = {}
    for n, hw in enumerate(sizes):
        groups.setdefault(hw, []).append(n)
    planes_of, statuses, origin = {}, [], []
    is_union = [is_image[n] and "rle_planes" in r for n, r in enumerate(recipes)]
    for hw, uni in [(hw, uni) for hw in groups for uni in (False, True)]:
        # (recipes whose planes are unions of strings -- Mapillary -- go through rle_decode_union, the others through rle_decode as ever)
        members = [n for n in groups[hw] if is_union[n] == uni]
        strings, plane_idx, base, bases, counts = [], [], 0, {}, {}
        for n in members:
            r = recipes[n]
            bases[n] = base
            if is_image[n]:
                own = r["rle_planes"] if uni else range(len(r["rle"]))
                counts[n] = r["n_instances"] + int(r["has_ignore"])
                if uni and (len(own) != len(r["rle"]) or any(not 0 <= q < counts[n] for q in own)):
                    raise ValueError("image %s: %d strings, %d plane indices, %d planes" % (r["meta_info"]["seq_name"], len(r["rle"]), len(own),
                                                                                          counts[n]))
                for j, s in enumerate(r["rle"]):
                    strings.append(s)
                    plane_idx.append(base + own[j])
                    origin.append((r["meta_info"]["seq_name"], 0, j))
            else:
                order, _ = plane_layout(r)
                slot = {inst: j for j, inst in enumerate(order)}
                for inst, t, s in r["rle"]:
                    strings.append(s)
                    plane_idx.append(base + slot[inst] * T + t)
                    origin.append((r["meta_info"]["seq_name"], t, inst))
                counts[n] = len(order) * T
            base += counts[n]
        if base == 0:
            continue
        planes, status = (hip.rle_decode_union if uni else hip.rle_decode)(strings, plane_idx, base, hw[0], hw[1], dev)
        statuses.append(status)
        for n in members:
            planes_of[n] = planes[bases[n]:bases[n] + counts[n]]

    images, image_targets = [], {}
    for n, (r, hw, new_hw) in enumerate(zip(recipes, sizes, new_sizes)):
        if is_image[n]:
            seq, masks, ignore_masks = _collate_image_sample(hip, r, planes_of.get(n), T, new_hw, pad_hw, dev)
            image_targets[n] = (masks, ignore_masks)
            images.append(seq)
            continue
        frames, _ = hip.decode_frames(r["frames"], dev)
        if tuple(frames.shape[1:3]) != hw:
            raise ValueError("sequence %s: the frames are %s, the dataset says %s" % (r["meta_info"]["seq_name"], tuple(frames.shape[1:3]), hw))
        dup = r.get("duplicate")
        if dup is not None:
            frames, both = hip.duplicate_instance(frames, planes_of[n], dup["boxes"], dup["flip"], dup["shifts"])
            planes_of[n] = both.view(2 * T, hw[0], hw[1])
        images.append(_preprocess(hip, frames, new_hw, pad_hw))
    image_list = ImageList(torch.stack(images, 0), new_sizes, [tuple(r["size"]) for r in recipes])

    # the category ids of the whole batch in one upload that nobody waits for
    n_cats = [len(r["category_ids"]) for r in recipes]
    cats = hip.upload(np.asarray([c for r in recipes for c in r["category_ids"]], np.int64), dev).split(n_cats)

    targets = []
    for n, (r, new_hw) in enumerate(zip(recipes, new_sizes)):
        if is_image[n]:
            if n_cats[n] != r["n_instances"]:
                raise ValueError("image %s: %d category ids for %d instances" % (r["meta_info"]["seq_name"], n_cats[n], r["n_instances"]))
            targets.append({"masks": image_targets[n][0], "ignore_masks": image_targets[n][1], "category_ids": cats[n]})
            continue
        order, n_targets = plane_layout(r)
        n_instances = r["n_instances"]
        if r.get("duplicate") is not None:
            n_targets, n_instances = n_targets + 1, n_instances + 1
        ignore = r["ignore"]
        if n_cats[n] != n_targets:
            raise ValueError("sequence %s: %d category ids for %d instances" % (r["meta_info"]["seq_name"], n_cats[n], n_targets))
        zeros = lambda *shape: torch.zeros(shape + tuple(pad_hw), dtype=torch.uint8, device=dev)
        if n_instances == 0:
            # no plane to resize: no targets, and the complement of an empty union is everything the frame covers
            masks, ignore_masks = zeros(0, T), zeros(T)
            if ignore == "background":
                ignore_masks[:, :new_hw[0], :new_hw[1]] = 1
        else:
            unions = [(t, n_targets, T) for t in range(T)] if ignore == "background" else None
            out = hip.resize_masks(planes_of[n], new_hw, pad_hw, ignore_from=unions)
            masks = out[:n_targets * T].view(n_targets, T, pad_hw[0], pad_hw[1])
            ignore_masks = out[n_targets * T:] if (unions or isinstance(ignore, tuple)) else zeros(T)
        targets.append({"masks": masks, "ignore_masks": ignore_masks, "category_ids": cats[n]})

    if statuses:
        host = torch.cat(statuses).cpu().numpy()                      # the batch's one read-back
        for m in host.nonzero()[0].tolist():
            seq, t, inst = origin[m]
            raise ValueError("sequence %s, frame %d, instance %d: the annotation is no valid COCO RLE for these frames (%s)"
                             % (seq, t, inst, hip.RLE_STATUS_NAMES.get(int(host[m]), "status %d" % host[m])))
    return image_list, targets, tuple(r["meta_info"] for r in recipes)


class DeviceCollateLoader(object):
    """An iterable over ``loader`` (a DataLoader whose workers hand back lists of recipes) that applies ``collate`` to every batch in the
    process that consumes it -- the only one that opens the GPU."""

    def __init__(self, loader, collate=device_collate):
        self.loader, self.collate = loader, collate

    def __iter__(self):
        for recipes in self.loader:
            yield self.collate(recipes)

    def __len__(self):
        return len(self.loader)
