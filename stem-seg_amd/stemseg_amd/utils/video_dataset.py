"""The inference-side view of the reference's generic video-dataset JSON (``stemseg/data/generic_video_dataset_parser.py:9-59``):
``{"meta": {"category_labels": {...}}, "sequences": [{"id", "height", "width", "image_paths": [...], ...}]}``.  Only what
``inference/main.py`` touches is kept (paths, dims, id, length, the frames for the visualisations); the annotations (RLE masks, categories)
are the training side's, ``stemseg_amd.data.generic_video_dataset_parser``, which builds on this class."""
import json


class GenericVideoSequence(object):
    def __init__(self, seq_dict, base_dir):
        self.base_dir = base_dir
        self.image_paths = list(seq_dict["image_paths"])
        self.image_dims = (seq_dict["height"], seq_dict["width"])
        self.id = self.seq_id = seq_dict["id"]
        self.instance_categories = {int(k): v for k, v in seq_dict.get("categories", {}).items()} or None

    def __len__(self):
        return len(self.image_paths)

    def load_images(self, frame_idxes=None, device=None):
        """BGR uint8 frames (generic_video_dataset_parser.py:61-72): the paths joined to ``base_dir``, read by
        ``InferenceModel.load_images``; all frames when ``frame_idxes`` is None.  With a ``device``: one uint8 tensor [F, H, W, 3]
        there, decoded on the device."""
        import os
        from ..modeling.inference_model import InferenceModel
        if frame_idxes is None:
            frame_idxes = list(range(len(self.image_paths)))
        paths = [os.path.join(self.base_dir, self.image_paths[t]) for t in frame_idxes]
        for p in paths:
            if not os.path.isfile(p):
                raise ValueError("No image found at path: {}".format(p))
        return InferenceModel.load_images(paths, device)


def parse_generic_video_dataset(base_dir, dataset_json):
    with open(dataset_json, "r") as fh:
        dataset = json.load(fh)
    meta = dataset["meta"]
    meta["category_labels"] = {int(k): v for k, v in meta["category_labels"].items()}
    return [GenericVideoSequence(s, base_dir) for s in dataset["sequences"]], meta
