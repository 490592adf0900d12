"""The generic image-dataset JSON of COCO and Pascal VOC (the reference's data/generic_image_dataset_parser.py): per image its size,
path, one COCO RLE string and one category id per instance, and for Pascal VOC an ``ignore`` string.  Nothing here decodes a mask or an
image: areas come from an integer walk over the strings' runs, the file goes out as bytes, the device does the rest."""
import json
import os

from .instance_duplicator import rle_area_and_box


def parse_generic_image_dataset(base_dir, dataset_json):
    with open(dataset_json, "r") as fh:
        dataset = json.load(fh)
    meta_info = dataset["meta"]
    meta_info["category_labels"] = {int(k): v for k, v in meta_info["category_labels"].items()}
    return [GenericImageSample(base_dir, sample) for sample in dataset["images"]], meta_info


class GenericImageSample(object):
    def __init__(self, base_dir, sample):
        self.height = sample["height"]
        self.width = sample["width"]
        self.path = os.path.join(base_dir, sample["image_path"])
        self.categories = [int(cat_id) for cat_id in sample["categories"]]
        self.segmentations = list(sample["segmentations"])
        self.ignore = sample.get("ignore", None)

    def mask_areas(self):
        return [rle_area_and_box(seg, self.height, self.width)[0] for seg in self.segmentations]

    def read_image(self):
        if not os.path.isfile(self.path):
            raise ValueError("No image found at path: {}".format(self.path))
        with open(self.path, "rb") as fh:
            return fh.read()

    def keep_instances(self, idxes):
        self.segmentations = [self.segmentations[i] for i in idxes]
        self.categories = [self.categories[i] for i in idxes]

    def filter_categories(self, cat_ids_to_keep):
        self.keep_instances([i for i, cat_id in enumerate(self.categories) if cat_id in cat_ids_to_keep])
