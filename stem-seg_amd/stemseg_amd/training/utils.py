"""The training side's helpers, under the reference's names (training/utils.py): ``create_optimizer``, ``create_lr_scheduler``,
``var_keys_to_str``, ``register_log_level_type``; plus what the reference leaves to its backbone's constructor and what this library's
opt-in switches need, ``configure_trainable``, and the step arithmetic of the loop, ``optimizer_step_interval``.  The dataset side,
``create_training_dataset`` and ``create_training_data_loader``, mixes the video datasets of ``stemseg_amd.data``; the image datasets
(COCO, Pascal VOC, Mapillary), the instance duplicator and the augmentations are refused by the config key that asks for them, unless
``device_augmentation`` (COCO, Pascal VOC, the duplicator) or ``device_mapillary`` (Mapillary) is passed."""
import logging

import torch
from torch.optim import lr_scheduler as torch_schedulers
from torch.utils.data import DataLoader
from torch.utils.data.sampler import BatchSampler, RandomSampler, SequentialSampler

from .. import hip
from ..config import PRESET_TRAINING_MODES, cfg as global_cfg
from ..utils import distributed as dist_utils
from ..utils.paths import DavisUnsupervisedPaths as DavisPaths, KITTIMOTSPaths, YoutubeVISPaths
from ..utils.constants import Loss
from .exponential_lr import ExponentialLR
from .optim import DeviceAdam, DeviceSGD

# what a logged value is called on the console: the reference's abbreviations, so that logs of both read alike
_SHORT_NAMES = dict(zip((Loss.EMBEDDING, Loss.SEMSEG, Loss.VARIANCE_SMOOTHNESS, Loss.LOVASZ_LOSS, Loss.SEEDINESS_LOSS, Loss.FOREGROUND),
                        "EmbL SegL VarS LovL SeedL FgL".split()))
_SPECIAL_FORMATS = {"lr": "LR: {:.2E}", "grad_norm": "GradN: {:.3f}"}       # ('grad_norm': the clip's, which the reference does not log)

_LOG_LEVELS = dict(fatal=logging.FATAL, critical=logging.CRITICAL, error=logging.ERROR, warn=logging.WARN, warning=logging.WARN,
                   info=logging.INFO, normal=logging.INFO, debug=logging.DEBUG, verbose=logging.DEBUG)
_LOG_OFF = ("no", "false", "off", "f", "0")


def var_keys_to_str(losses):
    """{key: float} -> 'EmbL: 1.234 - SegL: 0.456 - LR: 1.00E-03', in the dict's order."""
    return " - ".join(_SPECIAL_FORMATS[k].format(v) if k in _SPECIAL_FORMATS else "%s: %.3f" % (_SHORT_NAMES[k], v) for k, v in losses.items())


def register_log_level_type(parser):
    """Registers the argparse type 'LogLevel' -- a level's name in any case, or no / false / off / f / 0 for False -- and returns its name."""
    def parse(text):
        word = text.lower()
        if word in _LOG_OFF:
            return False
        if word not in _LOG_LEVELS:
            raise ValueError("'%s' is no logging level (%s, or %s)" % (text, ", ".join(sorted(_LOG_LEVELS)), " / ".join(_LOG_OFF)))
        return _LOG_LEVELS[word]
    parser.register("type", "LogLevel", parse)
    return "LogLevel"


def create_optimizer(model, cfg, print_fn=None, device_step=True):
    """cfg: the TRAINING section.  OPTIMIZER 'sgd' takes INITIAL_LR, MOMENTUM, WEIGHT_DECAY and NESTEROV, 'adam' INITIAL_LR and WEIGHT_DECAY,
    over ``model.parameters()`` (frozen ones never get a gradient and are skipped by the step).  device_step: ``DeviceSGD`` /
    ``DeviceAdam`` (one launch per step, csrc/optimizer.hip); False: the stock torch classes, with the same state dicts."""
    say = print_fn or print
    kind = cfg.OPTIMIZER.lower()
    if kind == "sgd":
        optimizer = (DeviceSGD if device_step else torch.optim.SGD)(model.parameters(), lr=cfg.INITIAL_LR, momentum=cfg.MOMENTUM,
                                                                    weight_decay=cfg.WEIGHT_DECAY, nesterov=cfg.NESTEROV)
    elif kind == "adam":
        optimizer = (DeviceAdam if device_step else torch.optim.Adam)(model.parameters(), lr=cfg.INITIAL_LR, weight_decay=cfg.WEIGHT_DECAY)
    else:
        raise ValueError("TRAINING.OPTIMIZER '%s': sgd or adam" % cfg.OPTIMIZER)
    settings = {k: v for k, v in optimizer.defaults.items() if k in ("lr", "momentum", "nesterov", "weight_decay", "betas", "eps")}
    say("optimiser: %s with %s" % (type(optimizer).__name__, ", ".join("%s %s" % kv for kv in sorted(settings.items()))))
    return optimizer


def _multistep(optimizer, cfg):
    return torch_schedulers.MultiStepLR(optimizer, milestones=cfg.LR_DECAY_STEPS, gamma=cfg.LR_DECAY_FACTOR), \
        "learning rate x %g at steps %s" % (cfg.LR_DECAY_FACTOR, list(cfg.LR_DECAY_STEPS))


def _exponential(optimizer, cfg):
    return ExponentialLR(optimizer, cfg.LR_EXP_DECAY_FACTOR, cfg.LR_EXP_DECAY_STEPS, start_at=cfg.LR_EXP_DECAY_START), \
        "learning rate falls by x %g over %d steps from step %d on" % (cfg.LR_EXP_DECAY_FACTOR, cfg.LR_EXP_DECAY_STEPS, cfg.LR_EXP_DECAY_START)


def _constant(optimizer, cfg):
    return torch_schedulers.LambdaLR(optimizer, lambda step: 1.0), "learning rate stays at %g" % cfg.INITIAL_LR


_SCHEDULERS = {"step": _multistep, "exponential": _exponential, "none": _constant}


def create_lr_scheduler(optimizer, cfg, print_fn=None):
    """cfg: the TRAINING section.  LR_DECAY_TYPE 'step' (LR_DECAY_STEPS, LR_DECAY_FACTOR), 'exponential' (LR_EXP_DECAY_FACTOR,
    LR_EXP_DECAY_STEPS, LR_EXP_DECAY_START) or 'none'."""
    if cfg.LR_DECAY_TYPE not in _SCHEDULERS:
        raise ValueError("TRAINING.LR_DECAY_TYPE '%s': %s" % (cfg.LR_DECAY_TYPE, " | ".join(_SCHEDULERS)))
    scheduler, what = _SCHEDULERS[cfg.LR_DECAY_TYPE](optimizer, cfg)
    (print_fn or print)("scheduler: " + what)
    return scheduler


def optimizer_step_interval(batch_size, max_samples_per_gpu, accumulate_gradients, num_gpus=1):
    """-> (sub-iterations per optimiser step, samples per sub-iteration), the reference's arithmetic and checks (training/main.py:134-157).
    With accumulation a batch of BATCH_SIZE samples is fed MAX_SAMPLES_PER_GPU at a time per GPU; without, it must fit in one go."""
    if not accumulate_gradients:
        if batch_size > max_samples_per_gpu:
            raise ValueError("TRAINING.BATCH_SIZE %d does not fit MAX_SAMPLES_PER_GPU %d without ACCUMULATE_GRADIENTS" % (batch_size, max_samples_per_gpu))
        return 1, batch_size
    assert batch_size >= num_gpus, "TRAINING.BATCH_SIZE %d is smaller than the number of GPUs, %d" % (batch_size, num_gpus)
    assert batch_size % max_samples_per_gpu == 0, "TRAINING.BATCH_SIZE %d is no multiple of MAX_SAMPLES_PER_GPU %d" % (batch_size, max_samples_per_gpu)
    return batch_size // (max_samples_per_gpu * num_gpus), max_samples_per_gpu


def configure_trainable(model, cfg=None, freeze_backbone=None, train_stem=False):
    """Apply TRAINING.FREEZE_BACKBONE / MODEL.BACKBONE.FREEZE_AT_STAGE to ``requires_grad`` and set the model's opt-in switches to match.

    FREEZE_BACKBONE: the whole backbone frozen, ``train_decoders`` on.  Otherwise the stem and the layers below FREEZE_AT_STAGE are frozen
    (the reference's ResNet does that in its constructor, backbone/resnet.py:92-103), everything else is trainable and ``train_decoders``,
    ``train_fpn`` and ``train_body`` are on; a FREEZE_AT_STAGE outside 2 .. 4 is refused by ``check_body_trainable`` before anything is
    changed.  ``train_wide_head`` is on when the semseg head has more than STEMSEG_MAX_HEAD_OUT output channels, ``train_resnext`` when the
    trainable body is a ResNeXt one (MODEL.RESNETS.NUM_GROUPS > 1 or STRIDE_IN_1X1 = False).
    train_stem: FREEZE_AT_STAGE 1 (the stem frozen, layer1 trainable) and 0 (everything trainable: ``stem.conv1.weight`` too) are applied as
    the reference applies them, and the model's ``train_stem`` is set; without it both stay refused.
    cfg: the whole cfg (default: the global one); freeze_backbone: overrides its TRAINING.FREEZE_BACKBONE (the Trainer passes its own
    TRAINING section's).  -> the model."""
    cfg = cfg or global_cfg
    frozen_backbone = bool(cfg.TRAINING.FREEZE_BACKBONE if freeze_backbone is None else freeze_backbone)
    freeze_at = cfg.MODEL.BACKBONE.FREEZE_AT_STAGE
    bb = model.backbone
    resnext = not frozen_backbone and (getattr(bb, "num_groups", 1) != 1 or not getattr(bb, "stride_in_1x1", True))
    if not frozen_backbone:
        bb.check_body_trainable(freeze_at, train_stem=bool(train_stem), train_resnext=resnext or getattr(bb, "train_resnext", False))
    for p in model.parameters():
        p.requires_grad_(True)
    if frozen_backbone:
        model.backbone.requires_grad_(False)
    else:
        if freeze_at >= 1:
            model.backbone.body.stem.requires_grad_(False)
        for st in range(1, freeze_at):
            getattr(model.backbone.body, "layer%d" % st).requires_grad_(False)
    model.train_decoders = True
    model.train_fpn = model.train_body = not frozen_backbone
    head = model.semseg_head
    model.train_wide_head = bool(head is not None and head.out_channels > hip.MAX_HEAD_OUT)
    model.train_resnext = resnext
    model.train_stem = bool(train_stem) and not frozen_backbone
    return model


# ------------------------------------------------------------------------------------------------ the dataset mix and its loader
def _refuse_image_datasets(section, ds_cfg, keys):
    for key in keys:
        if getattr(ds_cfg, key) > 0.0:
            raise NotImplementedError("DATA.%s.%s = %g: the image datasets (COCO, Pascal VOC, Mapillary) make their clips with imgaug's affine "
                                      "warps, which this library does not port; set the weight to 0 and let the video weights sum to 1 -- or, "
                                      "for COCO and Pascal VOC, pass device_augmentation=True (--device_augmentation), which warps on the device.  "
                                      "For Mapillary, pass device_mapillary=True (--device_mapillary), which also builds its ignore mask on the device"
                                      % (section, key, getattr(ds_cfg, key)))


def _image_datasets(total_samples, ds_cfg, category_agnostic):
    """COCO and Pascal VOC by their weights (device_augmentation only), read from utils/paths.py's CocoPaths / PascalVOCPaths."""
    from ..data import CocoDataLoader, PascalVOCDataLoader
    from ..utils.paths import CocoPaths, PascalVOCPaths
    mix = []
    if ds_cfg.COCO_WEIGHT > 0.0:
        mix.append(("COCO", ds_cfg.COCO_WEIGHT, CocoDataLoader(CocoPaths.images_dir(), CocoPaths.ids_file(), category_agnostic=category_agnostic)))
    if ds_cfg.PASCAL_VOC_WEIGHT > 0.0:
        mix.append(("PascalVOC", ds_cfg.PASCAL_VOC_WEIGHT, PascalVOCDataLoader(PascalVOCPaths.images_dir(), PascalVOCPaths.ids_file(),
                                                                                category_agnostic=category_agnostic)))
    return mix


def _mix_for_davis(total_samples, cfg, device_augmentation=False, device_mapillary=False):
    from ..data import DavisDataLoader, YoutubeVISDataLoader
    assert cfg.INPUT.NUM_CLASSES == 2
    ds_cfg = cfg.DATA.DAVIS
    if not device_augmentation:
        _refuse_image_datasets("DAVIS", ds_cfg, ("COCO_WEIGHT", "PASCAL_VOC_WEIGHT"))
    mix = _image_datasets(total_samples, ds_cfg, True) if device_augmentation else []
    if ds_cfg.YOUTUBE_VIS_WEIGHT > 0.0:
        mix.append(("YouTubeVIS", ds_cfg.YOUTUBE_VIS_WEIGHT, YoutubeVISDataLoader(
            YoutubeVISPaths.training_base_dir(), YoutubeVISPaths.train_vds_file(), int(round(total_samples * ds_cfg.YOUTUBE_VIS_WEIGHT)),
            category_agnostic=True, single_instance_duplication=cfg.DATA.YOUTUBE_VIS.SINGLE_INSTANCE_DUPLICATION,
            device_augmentation=device_augmentation)))
    if ds_cfg.DAVIS_WEIGHT > 0.0:
        # (the reference turns the duplicator on for DAVIS whatever the config says; here the config key decides, and True needs device_augmentation)
        mix.append(("Davis", ds_cfg.DAVIS_WEIGHT, DavisDataLoader(
            DavisPaths.trainval_base_dir(), DavisPaths.train_vds_file(),
            samples_to_create=int(round(cfg.TRAINING.MAX_ITERATIONS * cfg.TRAINING.BATCH_SIZE * ds_cfg.DAVIS_WEIGHT)),
            single_instance_duplication=ds_cfg.SINGLE_INSTANCE_DUPLICATION, background_as_ignore_region=True,
            device_augmentation=device_augmentation)))
    return mix


def _mix_for_youtube_vis(total_samples, cfg, device_augmentation=False, device_mapillary=False):
    from ..data import YoutubeVISDataLoader
    assert cfg.INPUT.NUM_CLASSES == 41          # 40 classes + 1 generic foreground class
    ds_cfg = cfg.DATA.YOUTUBE_VIS
    if not device_augmentation:
        _refuse_image_datasets("YOUTUBE_VIS", ds_cfg, ("COCO_WEIGHT", "PASCAL_VOC_WEIGHT"))
    mix = _image_datasets(total_samples, ds_cfg, False) if device_augmentation else []
    if ds_cfg.YOUTUBE_VIS_WEIGHT > 0.0:
        mix.append(("YouTubeVIS", ds_cfg.YOUTUBE_VIS_WEIGHT, YoutubeVISDataLoader(
            YoutubeVISPaths.training_base_dir(), YoutubeVISPaths.train_vds_file(), int(round(total_samples * ds_cfg.YOUTUBE_VIS_WEIGHT)),
            category_agnostic=False, single_instance_duplication=ds_cfg.SINGLE_INSTANCE_DUPLICATION, device_augmentation=device_augmentation)))
    return mix


def _mix_for_kitti_mots(total_samples, cfg, device_augmentation=False, device_mapillary=False):
    from ..data import MapillaryDataLoader, MOTSDataLoader
    from ..utils.paths import MapillaryPaths
    assert cfg.INPUT.NUM_CLASSES == 3          # car, pedestrian, background
    ds_cfg = cfg.DATA.KITTI_MOTS
    mix = []
    if not device_mapillary:
        _refuse_image_datasets("KITTI_MOTS", ds_cfg, ("MAPILLARY_WEIGHT",))
    elif ds_cfg.MAPILLARY_WEIGHT > 0.0:
        mix.append(("Mapillary", ds_cfg.MAPILLARY_WEIGHT, MapillaryDataLoader(MapillaryPaths.images_dir(), MapillaryPaths.ids_file())))
    if ds_cfg.KITTI_MOTS_WEIGHT > 0.0:
        mix.append(("KITTI-MOTS", ds_cfg.KITTI_MOTS_WEIGHT, MOTSDataLoader(
            KITTIMOTSPaths.train_images_dir(), KITTIMOTSPaths.train_vds_file(), int(round(total_samples * ds_cfg.KITTI_MOTS_WEIGHT)))))
    return mix


_DATASET_MIXES = {"davis": _mix_for_davis, "youtube_vis": _mix_for_youtube_vis, "kitti_mots": _mix_for_kitti_mots}


def create_training_dataset(total_samples, print_fn=None, mode=None, device_augmentation=False, device_mapillary=False):
    """The ``ConcatDataset`` of TRAINING.MODE (davis | youtube_vis | kitti_mots; ``mode`` overrides a MODE left empty, as the presets leave it):
    the video datasets with a weight above 0, read from the STEMSEG_* / *_BASE_DIR paths of ``utils/paths.py``.  A dataset whose weight is
    0 is skipped; a non-zero COCO_WEIGHT / PASCAL_VOC_WEIGHT / MAPILLARY_WEIGHT, SINGLE_INSTANCE_DUPLICATION: True and
    apply_augmentation=True raise NotImplementedError naming the key.  device_augmentation: COCO and Pascal VOC join the mix by their
    weights and the duplicator runs, both warped on the device (csrc/augment.hip; the category tables come from STEMSEG_METAINFO_DIR);
    MAPILLARY_WEIGHT and apply_augmentation=True stay refused.  device_mapillary: Mapillary joins the kitti_mots mix by its weight
    (data/mapillary_data_loader.py, read from utils/paths.py's MapillaryPaths; warped on the device, its ignore mask the union decode of
    csrc/data_loader.hip); without it MAPILLARY_WEIGHT stays refused."""
    from ..data import ConcatDataset
    say = print_fn or print
    mode = global_cfg.TRAINING.MODE or mode
    if mode not in _DATASET_MIXES:
        raise ValueError("Invalid training mode: {}".format(mode))
    mix = _DATASET_MIXES[mode](total_samples, global_cfg, bool(device_augmentation), bool(device_mapillary))
    if not mix:
        raise ValueError("TRAINING.MODE %s: every dataset weight is 0" % mode)
    say("Training datasets: {}".format(", ".join(name for name, _, _ in mix)))
    return ConcatDataset([ds for _, _, ds in mix], total_samples, [w for _, w, _ in mix])


def create_training_data_loader(dataset, batch_size, shuffle, collate_fn=None, num_workers=0, elapsed_iters=0, device_augmentation=False,
                                device_mapillary=False):
    """An iterable of ``(image_seqs, targets, meta_info)`` batches on the device.  The ``DataLoader`` inside hands out lists of host recipes
    (``collate_fn=list`` in its workers, which never open the GPU); ``collate_fn`` -- default ``data.common.device_collate`` -- is applied
    to each list in the process that iterates.  Sampler: the ``DistributedSampler`` port when a process group of more than one rank is up,
    else random / sequential by ``shuffle``; ``elapsed_iters`` > 0 wraps it in ``IterationBasedBatchSampler`` as the reference does.
    device_augmentation, device_mapillary: accepted for symmetry with ``create_training_dataset`` -- the collate dispatches on each recipe's
    kind, so a dataset built with a switch needs nothing more here."""
    from ..data import DistributedSampler, IterationBasedBatchSampler
    from ..data.common import DeviceCollateLoader, device_collate
    if dist_utils.is_distributed():
        sampler = DistributedSampler(dataset, dist_utils.get_world_size(), dist_utils.get_rank(), shuffle)
    else:
        sampler = RandomSampler(dataset) if shuffle else SequentialSampler(dataset)
    batch_sampler = BatchSampler(sampler, batch_size, drop_last=False)
    if elapsed_iters > 0:
        print("Elapsed iters: {}".format(elapsed_iters))
        batch_sampler = IterationBasedBatchSampler(batch_sampler, int(len(dataset) / batch_size), elapsed_iters)
    # (workers are spawned, not forked: by now this process has usually initialised HIP, and a forked copy of that state is not safe to keep)
    loader = DataLoader(dataset, collate_fn=list, batch_sampler=batch_sampler, num_workers=num_workers,
                        multiprocessing_context="spawn" if num_workers > 0 else None)
    return DeviceCollateLoader(loader, collate_fn or device_collate)
