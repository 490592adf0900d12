"""``VideoDataset`` under the reference's name (data/video_dataset.py): the base of the three video loaders.  ``__getitem__`` returns a
host recipe (see ``data.common``) and never touches the device; the resize, the normalisation and the mask decoding of the reference's
``__getitem__`` happen in ``device_collate``.  The reference's video pipeline is deterministic once the clips are sampled: all three
loaders are built with ``apply_augmentation=False``, and its augmented branch cannot run as written; here ``True`` is refused."""
import math
import random

import numpy as np
from torch.utils.data import Dataset

from .generic_video_dataset_parser import parse_generic_video_dataset
from .instance_duplicator import InstanceDuplicator, rle_area_and_box


class VideoDataset(Dataset):
    def __init__(self, base_dir, vds_json, clip_length, apply_augmentations, single_instance_duplication=False, **kwargs):
        super().__init__()
        if apply_augmentations:
            raise NotImplementedError("apply_augmentation=True: the augmentations are imgaug's affine warps and blurs, which this library does "
                                      "not port; the reference builds its video loaders with apply_augmentation=False")
        self.sequences, self.meta_info = parse_generic_video_dataset(base_dir, vds_json)
        self.clip_length = clip_length
        self.apply_augmentations = False
        # (the loaders that take the switch let True through only with device_augmentation: the decision is made here, on the host, and
        # ``device_collate`` pastes the copy on the device)
        self.single_instance_duplication = bool(single_instance_duplication)
        self.instance_duplicator = InstanceDuplicator()
        self.samples = []

    def filter_zero_instance_frames(self):
        for seq in self.sequences:
            seq.filter_zero_instance_frames()
        self.sequences = [seq for seq in self.sequences if len(seq) > 0]

    def filter_categories(self, cat_ids_to_keep):
        for seq in self.sequences:
            seq.filter_categories(cat_ids_to_keep)
        self.sequences = [seq for seq in self.sequences if len(seq) > 0]

    def sample_subsequences(self, gap_lower, gap_upper, num_subsequences):
        """``create_training_subsequences`` of the three loaders, which differ in their config keys only: -> (the sampled sub-sequences,
        [(sequence id, frame indices)]).  The calls to ``random`` are the reference's, in its order -- per sequence and sample one
        ``choice`` of the span and, unless only one start fits, one ``randint``; then one ``sample`` and one ``shuffle`` over all -- so
        that a seeded run picks the same clips."""
        spans = list(range(gap_lower, gap_upper + 1))
        long_enough = [seq for seq in self.sequences if len(seq) > spans[0] + 1]
        total_frames = sum(len(seq) for seq in long_enough)
        picks = []
        for seq in long_enough:
            for _ in range(max(1, int(math.ceil(len(seq) / total_frames * num_subsequences)))):
                span = min(random.choice(spans), len(seq) - 1)
                last_start = len(seq) - span - 1
                assert last_start >= 0
                start = random.randint(0, last_start) if last_start else 0
                frames = np.round(np.linspace(start, start + span, self.clip_length)).astype(np.int32).tolist()
                assert len(set(frames)) == len(frames), "a clip of %d frames does not fit a span of %d" % (self.clip_length, span)
                picks.append((seq.id, frames))
        assert len(picks) >= num_subsequences, "{} should be >= {}".format(len(picks), num_subsequences)
        picks = random.sample(picks, num_subsequences)        # (rounding up per sequence gives too many)
        random.shuffle(picks)
        by_id = {seq.id: seq for seq in long_enough}
        return [by_id[seq_id].extract_subsequence(frames) for seq_id, frames in picks], picks

    def parse_sample_at(self, idx):
        """-> (sample: the sub-sequence, category ids of the target instances, ignore rule)"""
        raise NotImplementedError("This method must be implemented by the derived class.")

    def __getitem__(self, index):
        sample, category_ids, ignore = self.parse_sample_at(index)
        height, width = sample.image_dims
        recipe = {"frames": sample.read_frames(), "rle": sample.rle_items(), "n_instances": len(sample.instance_ids),
                  "category_ids": [int(c) for c in category_ids], "ignore": ignore, "size": (int(width), int(height)),
                  "meta_info": {"seq_name": sample.id}}
        if self.single_instance_duplication and len(sample.instance_ids) == 1:
            # youtube_vis_data_loader.py:81-87: the lone instance's boxes, read off its strings (a frame without one has no box)
            boxes = [None] * len(recipe["frames"])
            try:
                for _, t, s in recipe["rle"]:
                    boxes[t] = rle_area_and_box(s, height, width)[1]
                decision = self.instance_duplicator(boxes, width, height)
            except (ValueError, IndexError):
                # a string that is no RLE for these frames: the sample stays un-duplicated, as on any exception in the reference, and
                # ``device_collate`` reports the string by sequence, frame and instance when it decodes it
                decision = None
            if decision is not None:          # duplication was successful
                recipe["duplicate"] = {"boxes": boxes, "flip": decision["flip"], "shifts": [sh or (0.0, 0.0) for sh in decision["shifts"]]}
                recipe["category_ids"].append(recipe["category_ids"][-1])
        return recipe

    def __len__(self):
        return len(self.samples)
