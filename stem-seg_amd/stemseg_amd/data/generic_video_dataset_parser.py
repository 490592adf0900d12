"""The training side of the generic video-dataset JSON (the reference's data/generic_video_dataset_parser.py), built on the inference-side
view in ``utils/video_dataset.py``: per frame a dict {instance id: COCO RLE string}, per sequence {instance id: category id}.  Nothing
here decodes a mask or an image: ``rle_items`` hands out the strings with their (instance, frame) indices, ``read_frames`` the files'
bytes, and the device does the rest (``data.common.device_collate``)."""
import json
import os

from ..utils.video_dataset import GenericVideoSequence as _InferenceSequence


class GenericVideoSequence(_InferenceSequence):
    def __init__(self, seq_dict, base_dir):
        super().__init__(seq_dict, base_dir)
        segs = seq_dict.get("segmentations")
        self.segmentations = None if segs is None else [{int(iid): s for iid, s in seg_t.items()} for seg_t in segs]
        cats = seq_dict.get("categories")
        self.instance_categories = None if cats is None else {int(iid): c for iid, c in cats.items()}      # (in the file's order)

    @property
    def instance_ids(self):
        return list(self.instance_categories.keys())

    @property
    def category_labels(self):
        return [self.instance_categories[iid] for iid in self.instance_ids]

    def read_frames(self, frame_idxes=None):
        """The files' bytes, one per frame (all frames when ``frame_idxes`` is None)."""
        frames = []
        for t in (range(len(self)) if frame_idxes is None else frame_idxes):
            path = os.path.join(self.base_dir, self.image_paths[t])
            if not os.path.isfile(path):
                raise ValueError("No image found at path: {}".format(path))
            with open(path, "rb") as fh:
                frames.append(fh.read())
        return frames

    def rle_items(self, frame_idxes=None):
        """[(position of the instance in ``instance_ids``, position of the frame, string)] for every annotation there is; an instance
        that is absent from a frame has no item, and gets a zero mask (generic_video_dataset_parser.py:89-90)."""
        frames = list(range(len(self))) if frame_idxes is None else list(frame_idxes)
        return [(i, k, self.segmentations[t][iid]) for k, t in enumerate(frames) for i, iid in enumerate(self.instance_ids)
                if iid in self.segmentations[t]]

    def filter_categories(self, cat_ids_to_keep):
        # (as in the reference, line 97: the test is on the instance id, not on its category; none of the three loaders calls this)
        keep = sorted(iid for iid in self.instance_categories if iid in cat_ids_to_keep)
        self.segmentations = [{iid: s for iid, s in seg_t.items() if iid in keep} for seg_t in self.segmentations]

    def filter_zero_instance_frames(self):
        kept = [t for t in range(len(self)) if self.segmentations[t]]
        self.image_paths = [self.image_paths[t] for t in kept]
        self.segmentations = [self.segmentations[t] for t in kept]

    def apply_category_id_mapping(self, mapping):
        assert set(mapping.keys()) == set(self.instance_categories.keys())
        self.instance_categories = {iid: mapping[cat] for iid, cat in self.instance_categories.items()}

    def extract_subsequence(self, frame_idxes, new_id=""):
        """The frames ``frame_idxes`` as a sequence of their own.  Its instances are those annotated in any of these frames, in the order in
        which a set of their ids iterates (the reference's, lines 114-121: it fixes the order of the masks of a sample); its frames come
        in the sequence's order, whatever the order of ``frame_idxes`` (line 127)."""
        assert all(0 <= t < len(self) for t in frame_idxes)
        seen = []
        for t in frame_idxes:
            seen.extend(self.segmentations[t].keys())
        kept_ids = set(seen)
        chosen = set(frame_idxes)
        return type(self)({
            "id": new_id or self.id, "height": self.image_dims[0], "width": self.image_dims[1],
            "image_paths": [self.image_paths[t] for t in frame_idxes],
            "categories": {iid: self.instance_categories[iid] for iid in kept_ids},
            "segmentations": [{iid: s for iid, s in seg_t.items() if iid in kept_ids} for t, seg_t in enumerate(self.segmentations) if t in chosen],
        }, self.base_dir)


def parse_generic_video_dataset(base_dir, dataset_json):
    with open(dataset_json, "r") as fh:
        dataset = json.load(fh)
    meta = dataset["meta"]
    meta["category_labels"] = {int(k): v for k, v in meta["category_labels"].items()}
    seqs = [GenericVideoSequence(s, base_dir) for s in dataset["sequences"]]
    for seq in seqs:
        if seq.segmentations is not None:
            annotated = set(iid for seg_t in seq.segmentations for iid in seg_t)
            assert annotated == set(seq.instance_categories), "Instance ID mismatch: {} vs. {}".format(annotated, set(seq.instance_categories))
    return seqs, meta
