"""``DavisDataLoader`` (the reference's data/davis_data_loader.py): every instance is category 1, and with ``background_as_ignore_region``
whatever no instance covers is ignored -- 1 - union of the instances, taken at full resolution before the resize."""
from ..config import cfg
from .video_dataset import VideoDataset


class DavisDataLoader(VideoDataset):
    def __init__(self, base_dir, vds_json_file, samples_to_create=-1, apply_augmentation=False, single_instance_duplication=False,
                 background_as_ignore_region=True, device_augmentation=False):
        if single_instance_duplication and not device_augmentation:
            raise NotImplementedError("DATA.DAVIS.SINGLE_INSTANCE_DUPLICATION: the instance duplicator is cv2.warpAffine, which this library "
                                      "does not port; set it to False, or pass device_augmentation=True, which pastes on the device")
        super().__init__(base_dir, vds_json_file, cfg.INPUT.NUM_FRAMES, apply_augmentation,
                         single_instance_duplication=single_instance_duplication)
        self.filter_zero_instance_frames()
        self.samples = self.create_training_subsequences(samples_to_create)
        self.background_as_ignore_region = background_as_ignore_region

    def create_training_subsequences(self, num_subsequences):
        gaps = cfg.DATA.DAVIS
        samples, self.sample_idxes = self.sample_subsequences(gaps.FRAME_GAP_LOWER, gaps.FRAME_GAP_UPPER, num_subsequences)
        return samples

    def parse_sample_at(self, idx):
        sample = self.samples[idx]
        return sample, [1] * len(sample.instance_ids), ("background" if self.background_as_ignore_region else None)
