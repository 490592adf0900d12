"""``MapillaryDataLoader`` (the reference's data/mapillary_data_loader.py): ``CocoDataLoader``'s clips from one Mapillary Vistas image,
with the reference's selection of targets.  An image's instances are sorted by area, largest first; of the first ``max_nbr_instances``
those of a ``keep`` category are the targets, and everything else -- the ``ignore_mask`` categories among them and every instance beyond
them -- is OR-ed into ONE ignore mask.  Nothing is decoded here: the areas come from the strings' runs, and the recipe hands the ignore
strings to the device as they are, all naming the last plane (``"rle_planes"``), where ``hip.rle_decode_union`` rasterises them straight
into that plane.  The calls to ``random`` are the reference's in its order: the flip, one ``getrandbits(64)`` per warp, the shuffle."""
import random

import yaml
from torch.utils.data import Dataset

from ..config import cfg
from ..utils.paths import RepoPaths
from .generic_image_dataset_parser import parse_generic_image_dataset
from .image_to_seq_augmenter import ImageToSeqAugmenter


def select_instances(areas, categories, cat_ids_to_ignore, max_nbr_instances):
    """The reference's ``filter_instance_masks`` on indices: -> (targets, ignored), positions into ``areas`` in descending order of area
    (a stable sort: ties keep their order).  Of the first ``max_nbr_instances`` the ones outside ``cat_ids_to_ignore`` are targets."""
    order = sorted(range(len(areas)), key=lambda i: areas[i], reverse=True)
    targets = [i for k, i in enumerate(order) if k < max_nbr_instances and categories[i] not in cat_ids_to_ignore]
    chosen = set(targets)
    return targets, [i for i in order if i not in chosen]


class MapillaryDataLoader(Dataset):
    def __init__(self, base_dir, ids_json_file, min_instance_size=30, max_nbr_instances=30):
        super().__init__()
        samples, _ = parse_generic_image_dataset(base_dir, ids_json_file)
        with open(RepoPaths.dataset_meta_info_file("mapillary.yaml"), "r") as fh:
            details = {cat["id"]: cat for cat in yaml.load(fh, Loader=yaml.SafeLoader)}
        self.cat_ids_to_keep = [cat_id for cat_id, attribs in details.items() if attribs["keep"]]
        self.cat_ids_to_ignore = [cat_id for cat_id, attribs in details.items() if attribs["ignore_mask"]]
        self.category_id_mapping = {cat_id: details[cat_id]["id_kittimots"] for cat_id in self.cat_ids_to_keep}
        self.category_labels = {cat_id: details[cat_id]["label"] for cat_id in self.cat_ids_to_keep}
        self.samples = []
        for sample in samples:
            areas = sample.mask_areas()
            sample.keep_instances([i for i in range(len(sample.segmentations)) if areas[i] >= min_instance_size])
            if not any(cat in self.cat_ids_to_keep for cat in sample.categories):
                continue          # no relevant instances present in image
            sample.filter_categories(self.cat_ids_to_keep + self.cat_ids_to_ignore)
            self.samples.append(sample)
        self.max_nbr_instances = max_nbr_instances
        self.augmenter = ImageToSeqAugmenter(perspective=True, affine=True, motion_blur=True, rotation_range=(-10, 10), perspective_magnitude=0.08,
                                             hue_saturation_range=(-5, 5), brightness_range=(-40, 40), motion_blur_prob=0.0,
                                             translate_range=(-0.1, 0.1))
        self.num_frames = cfg.INPUT.NUM_FRAMES

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        sample = self.samples[index]
        flip = random.random() < 0.5                                                   # apply_random_flip
        warps = self.augmenter.sample_clip(sample.width, sample.height, self.num_frames - 1)
        perm = list(range(self.num_frames))
        random.shuffle(perm)                                                           # apply_random_sequence_shuffle
        targets, ignored = select_instances(sample.mask_areas(), sample.categories, self.cat_ids_to_ignore, self.max_nbr_instances)
        n = len(targets)
        categories = [sample.categories[i] for i in targets]
        return {"kind": "image", "frames": [sample.read_image()], "rle": [sample.segmentations[i] for i in targets + ignored],
                "rle_planes": list(range(n)) + [n] * len(ignored), "n_instances": n, "has_ignore": len(ignored) > 0, "flip": bool(flip),
                "warps": [{k: w[k] for k in ("hinv", "add", "hs", "flags", "blur")} for w in warps], "perm": perm,
                "category_ids": [int(self.category_id_mapping[c]) for c in categories], "size": (int(sample.width), int(sample.height)),
                "meta_info": {"seq_name": sample.path, "category_labels": [self.category_labels[c] for c in categories]}}
