"""``MOTSDataLoader`` (the reference's data/mots_data_loader.py).  Frames without a car or a pedestrian are dropped; where six of them
follow each other the sequence is cut there, so that no clip spans a long gap.  The instance of category 3, where a sample has one, is
not a target: its masks are the sample's ignore masks."""
from ..config import cfg
from .video_dataset import VideoDataset


class MOTSDataLoader(VideoDataset):
    IGNORE_MASK_CAT_ID = 3
    GAP_THAT_SPLITS = 6

    def __init__(self, base_dir, vds_json_file, samples_to_create, apply_augmentation=False):
        super().__init__(base_dir, vds_json_file, cfg.INPUT.NUM_FRAMES, apply_augmentation)
        self.sequences = [part for seq in self.sequences for part in self.split_at_gaps(seq)]
        assert samples_to_create > 0, "Number of training samples is required for train mode"
        self.samples = self.create_training_subsequences(samples_to_create)

    @classmethod
    def split_at_gaps(cls, seq):
        """-> the parts of ``seq``, ids '<id>_1', '<id>_2', ...: its frames with a car or a pedestrian, cut wherever GAP_THAT_SPLITS frames
        without one follow each other."""
        parts, frames, gap = [], [], 0
        for t in range(len(seq)):
            cats = set(seq.instance_categories[iid] for iid in seq.segmentations[t])
            if cats - {cls.IGNORE_MASK_CAT_ID}:
                gap = 0
                frames.append(t)
                continue
            gap += 1
            if gap == cls.GAP_THAT_SPLITS and frames:
                parts.append(frames)
                frames = []
        if frames:
            parts.append(frames)
        return [seq.extract_subsequence(f, "{}_{}".format(seq.id, k)) for k, f in enumerate(parts, 1)]

    def create_training_subsequences(self, num_subsequences):
        gaps = cfg.DATA.KITTI_MOTS
        samples, self.sample_idxes = self.sample_subsequences(gaps.FRAME_GAP_LOWER, gaps.FRAME_GAP_UPPER, num_subsequences)
        return samples

    def parse_sample_at(self, idx):
        sample = self.samples[idx]
        categories = sample.category_labels
        ignore = None
        if self.IGNORE_MASK_CAT_ID in categories:
            at = categories.index(self.IGNORE_MASK_CAT_ID)          # (the first one, as in the reference; a second would stay a target)
            del categories[at]
            ignore = ("instance", at)
        if not categories:
            raise ValueError("No instances exist in the masks (seq: {})".format(sample.id))
        return sample, categories, ignore
