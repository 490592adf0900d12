"""``CocoDataLoader`` (the reference's data/coco_data_loader.py) and the base it shares with ``PascalVOCDataLoader``: a clip of
INPUT.NUM_FRAMES frames made from ONE image -- the image itself (mirrored with probability 0.5) and NUM_FRAMES - 1 random warps of it,
shuffled.  ``__getitem__`` samples the warps and returns a host recipe of ``"kind": "image"``; ``data.common.device_collate`` decodes,
warps, blurs and resizes on the device.  The calls to ``random`` are the reference's in its order: one ``random.random()`` for the flip
first, one ``random.shuffle`` of the frame order last; between them one ``random.getrandbits(64)`` per warp seeds the augmenter's own
generator (the reference seeds imgaug from the wall clock there)."""
import random

import yaml
from torch.utils.data import Dataset

from ..config import cfg
from ..utils.paths import RepoPaths
from .generic_image_dataset_parser import parse_generic_image_dataset
from .image_to_seq_augmenter import ImageToSeqAugmenter


def category_tables(yaml_name, category_agnostic):
    """The metainfo table -> (ids to keep, {id: training id}, {id: label}): ``keep_davis`` and class 1 / 'object' when category agnostic,
    else ``keep_ytvis`` with ``id_ytvis`` / ``label_ytvis``."""
    with open(RepoPaths.dataset_meta_info_file(yaml_name), "r") as fh:
        details = {cat["id"]: cat for cat in yaml.load(fh, Loader=yaml.SafeLoader)}
    if category_agnostic:          # davis
        keep = [cat_id for cat_id, attribs in details.items() if attribs["keep_davis"]]
        return keep, {cat_id: 1 for cat_id in keep}, {cat_id: "object" for cat_id in keep}
    keep = [cat_id for cat_id, attribs in details.items() if attribs["keep_ytvis"]]          # youtube VIS
    return keep, {cat_id: details[cat_id]["id_ytvis"] for cat_id in keep}, {cat_id: details[cat_id]["label_ytvis"] for cat_id in keep}


class ImageSequenceDataset(Dataset):
    """What the two image loaders share.  ``samples`` hold the instances that survived the filters; a sample's ``ignore`` string, where
    it has one, travels as the last plane."""

    def __init__(self, base_dir, ids_json_file, yaml_name, category_agnostic, min_instance_size, augmenter):
        super().__init__()
        self.samples, _ = parse_generic_image_dataset(base_dir, ids_json_file)
        if min_instance_size is not None:
            for sample in self.samples:
                areas = sample.mask_areas()
                sample.keep_instances([i for i in range(len(sample.segmentations)) if areas[i] >= min_instance_size])
        cat_ids_to_keep, self.category_id_mapping, self.category_labels = category_tables(yaml_name, category_agnostic)
        for sample in self.samples:
            sample.filter_categories(cat_ids_to_keep)
        self.samples = [s for s in self.samples if len(s.segmentations) > 0]          # remove samples with 0 instances
        self.augmenter = augmenter
        self.num_frames = cfg.INPUT.NUM_FRAMES
        self.category_agnostic = category_agnostic

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        sample = self.samples[index]
        flip = random.random() < 0.5                                                   # apply_random_flip
        warps = self.augmenter.sample_clip(sample.width, sample.height, self.num_frames - 1)
        perm = list(range(self.num_frames))
        random.shuffle(perm)                                                           # apply_random_sequence_shuffle
        strings = list(sample.segmentations) + ([sample.ignore] if sample.ignore is not None else [])
        return {"kind": "image", "frames": [sample.read_image()], "rle": strings, "n_instances": len(sample.segmentations),
                "has_ignore": sample.ignore is not None, "flip": bool(flip),
                "warps": [{k: w[k] for k in ("hinv", "add", "hs", "flags", "blur")} for w in warps], "perm": perm,
                "category_ids": [int(self.category_id_mapping[c]) for c in sample.categories], "size": (int(sample.width), int(sample.height)),
                "meta_info": {"seq_name": sample.path, "category_labels": [self.category_labels[c] for c in sample.categories]}}


class CocoDataLoader(ImageSequenceDataset):
    def __init__(self, base_dir, ids_json_file, category_agnostic):
        super().__init__(base_dir, ids_json_file, "coco.yaml", category_agnostic, None, ImageToSeqAugmenter(
            perspective=True, affine=True, motion_blur=True, rotation_range=(-12, 12), perspective_magnitude=0.08, hue_saturation_range=(-5, 5),
            brightness_range=(-40, 40), motion_blur_prob=0.25, motion_blur_kernel_sizes=(9, 11), translate_range=(-0.1, 0.1)))
