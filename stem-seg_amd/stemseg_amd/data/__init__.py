"""The training data pipeline under the reference's names (stemseg.data): the three video loaders, the dataset mix and the samplers.  The
datasets return host recipes; ``common.device_collate`` turns a list of them into a batch on the device.  Nothing here imports
``stemseg_amd.hip`` at module level, so that a DataLoader's worker processes never load the HIP library."""
from .coco_data_loader import CocoDataLoader  # noqa: F401
from .concat_dataset import ConcatDataset, SparseDataset  # noqa: F401
from .davis_data_loader import DavisDataLoader  # noqa: F401
from .distributed_data_sampler import DistributedSampler  # noqa: F401
from .iteration_based_batch_sampler import IterationBasedBatchSampler  # noqa: F401
from .mapillary_data_loader import MapillaryDataLoader  # noqa: F401
from .mots_data_loader import MOTSDataLoader  # noqa: F401
from .pascal_voc_data_loader import PascalVOCDataLoader  # noqa: F401
from .video_dataset import VideoDataset  # noqa: F401
from .youtube_vis_data_loader import YoutubeVISDataLoader  # noqa: F401
