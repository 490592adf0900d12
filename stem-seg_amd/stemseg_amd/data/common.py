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

and ``device_collate(recipes)`` runs in the consuming process: per sample one ``decode_frames`` and one ``preprocess_frames``, per frame
size of the batch one ``rle_decode`` over every string of that size, per sample one ``resize_masks``.  Every upload of the mask path
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


def device_collate(recipes, device=None):
    """Recipes -> (ImageList, targets, meta_info) on the device: ``targets[n]`` = {"masks": uint8 [I,T,H,W], "ignore_masks": uint8 [T,H,W],
    "category_ids": int64 [I]} at the batch's padded size, what ``Trainer`` and ``TrainingModel`` take.  A refused annotation string raises
    ValueError naming the sequence and the frame."""
    from .. import hip
    hip.require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    T = len(recipes[0]["frames"])
    sizes, new_sizes = [], []
    for r in recipes:
        if len(r["frames"]) != T:
            raise ValueError("All sequences must contain the same number of images. Found {} and {}".format(T, len(r["frames"])))
        width, height = r["size"]
        new_w, new_h, _ = compute_resize_params((height, width), cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM)
        sizes.append((height, width))
        new_sizes.append((new_h, new_w))
    pad_hw = ImageList.padded_size(new_sizes)

    images = []
    for r, hw, new_hw in zip(recipes, sizes, new_sizes):
        frames, _ = hip.decode_frames(r["frames"], dev)
        if tuple(frames.shape[1:3]) != hw:
            raise ValueError("sequence %s: the frames are %s, the dataset says %s" % (r["meta_info"]["seq_name"], tuple(frames.shape[1:3]), hw))
        images.append(hip.preprocess_frames(frames, new_hw, pad_hw, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD,
                                            unit_scale=cfg.INPUT.NORMALIZE_TO_UNIT_SCALE, flip_channels=not cfg.INPUT.BGR_INPUT))
    image_list = ImageList(torch.stack(images, 0), new_sizes, [tuple(r["size"]) for r in recipes])

    # one decode call per frame size, over every string of the batch that has it
    groups = {}
    for n, hw in enumerate(sizes):
        groups.setdefault(hw, []).append(n)
    planes_of, statuses, origin = {}, [], []
    for hw, members in groups.items():
        strings, plane_idx, base, bases = [], [], 0, {}
        for n in members:
            r = recipes[n]
            order, _ = plane_layout(r)
            slot = {inst: j for j, inst in enumerate(order)}
            bases[n] = base
            for inst, t, s in r["rle"]:
                strings.append(s)
                plane_idx.append(base + slot[inst] * T + t)
                origin.append((r["meta_info"]["seq_name"], t, inst))
            base += len(order) * T
        if base == 0:
            continue
        planes, status = hip.rle_decode(strings, plane_idx, base, hw[0], hw[1], dev)
        statuses.append(status)
        for n in members:
            planes_of[n] = planes[bases[n]:bases[n] + recipes[n]["n_instances"] * T]

    # the category ids of the whole batch in one upload that nobody waits for
    n_cats = [len(r["category_ids"]) for r in recipes]
    cats = hip.upload(np.asarray([c for r in recipes for c in r["category_ids"]], np.int64), dev).split(n_cats)

    targets = []
    for n, (r, new_hw) in enumerate(zip(recipes, new_sizes)):
        order, n_targets = plane_layout(r)
        ignore = r["ignore"]
        if n_cats[n] != n_targets:
            raise ValueError("sequence %s: %d category ids for %d instances" % (r["meta_info"]["seq_name"], n_cats[n], n_targets))
        zeros = lambda *shape: torch.zeros(shape + tuple(pad_hw), dtype=torch.uint8, device=dev)
        if r["n_instances"] == 0:
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
