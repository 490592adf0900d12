"""``YoutubeVISDataLoader`` (the reference's data/youtube_vis_data_loader.py): clips of DATA.YOUTUBE_VIS.FRAME_GAP_LOWER .. UPPER frames'
span, every instance a target, no ignore region."""
from ..config import cfg
from .video_dataset import VideoDataset


class YoutubeVISDataLoader(VideoDataset):
    def __init__(self, base_dir, vds_json_file, samples_to_create, apply_augmentation=False, category_agnostic=True,
                 single_instance_duplication=False, device_augmentation=False):
        if single_instance_duplication and not device_augmentation:
            raise NotImplementedError("DATA.YOUTUBE_VIS.SINGLE_INSTANCE_DUPLICATION: the instance duplicator is cv2.warpAffine, which this "
                                      "library does not port; set it to False, or pass device_augmentation=True, which pastes on the device")
        super().__init__(base_dir, vds_json_file, cfg.INPUT.NUM_FRAMES, apply_augmentation,
                         single_instance_duplication=single_instance_duplication)
        self.filter_zero_instance_frames()
        self.category_agnostic = category_agnostic
        assert samples_to_create > 0
        self.samples = self.create_training_subsequences(samples_to_create)

    def create_training_subsequences(self, num_subsequences):
        gaps = cfg.DATA.YOUTUBE_VIS
        assert self.clip_length <= gaps.FRAME_GAP_LOWER <= gaps.FRAME_GAP_UPPER
        samples, self.sample_idxes = self.sample_subsequences(gaps.FRAME_GAP_LOWER, gaps.FRAME_GAP_UPPER, num_subsequences)
        return samples

    def parse_sample_at(self, idx):
        sample = self.samples[idx]
        return sample, ([1] * len(sample.instance_ids) if self.category_agnostic else sample.category_labels), None
