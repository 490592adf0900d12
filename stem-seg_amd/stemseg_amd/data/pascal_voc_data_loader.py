"""``PascalVOCDataLoader`` (the reference's data/pascal_voc_data_loader.py): ``CocoDataLoader``'s clips from one image, with instances
below ``min_instance_size`` pixels dropped first (areas read off the annotation strings) and the image's ignore annotation warped along
as the last plane."""
from .coco_data_loader import ImageSequenceDataset
from .image_to_seq_augmenter import ImageToSeqAugmenter


class PascalVOCDataLoader(ImageSequenceDataset):
    def __init__(self, base_dir, ids_json_file, category_agnostic, min_instance_size=50):
        super().__init__(base_dir, ids_json_file, "pascal_voc.yaml", category_agnostic, min_instance_size, ImageToSeqAugmenter(
            perspective=True, affine=True, motion_blur=True, rotation_range=(-10, 10), perspective_magnitude=0.08, hue_saturation_range=(-5, 5),
            brightness_range=(-40, 40), motion_blur_prob=0.25, motion_blur_kernel_sizes=(9, 11), translate_range=(-0.1, 0.1)))
