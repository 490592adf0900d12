"""The handful of configuration keys the hot path reads ('Config / flags'),
with the dataset presets of the reference (config/defaults.yaml, davis_1.yaml, davis_2.yaml, youtube_vis.yaml,
kitti_mots_2.yaml).  ``cfg`` is a process-global like the reference's, but plain and mutable:
decoder topology is fixed from ``cfg.INPUT.NUM_FRAMES`` at module construction (modeling/common.py:15-24).
"""
import copy
from types import SimpleNamespace as NS


def _defaults():
    return NS(
        INPUT=NS(IMAGE_MEAN=[102.9801, 115.9465, 122.7717], IMAGE_STD=[1.0, 1.0, 1.0], MIN_DIM=800, MAX_DIM=1333,
                 NUM_FRAMES=8, NUM_CLASSES=2, BGR_INPUT=True, NORMALIZE_TO_UNIT_SCALE=False),
        MODEL=NS(
            USE_SEMSEG_HEAD=True, USE_SEEDINESS_HEAD=False, EMBEDDING_DIM_MODE="xyt",
            BACKBONE=NS(TYPE="R-101-FPN", PRETRAINED_WEIGHTS="mask_rcnn_R_101_FPN_backbone.pth", FREEZE_AT_STAGE=2),
            RESNETS=NS(BACKBONE_OUT_CHANNELS=256, NUM_GROUPS=1, WIDTH_PER_GROUP=64, STRIDE_IN_1X1=True, STEM_OUT_CHANNELS=64,
                       RES2_OUT_CHANNELS=256),      # (defaults.yaml:50-56; NUM_GROUPS / WIDTH_PER_GROUP / STRIDE_IN_1X1 select ResNeXt)
            EMBEDDINGS=NS(HEAD_TYPE="squeeze_expand_decoder", INTER_CHANNELS=[256, 256, 128, 128], SCALE=[32, 16, 8, 4],
                          EMBEDDING_SIZE=3, TANH_ACTIVATION=True, NORMALIZATION_LAYER="gn", GN_NUM_GROUPS=32, POOL_TYPE="avg"),
            SEMSEG=NS(HEAD_TYPE="squeeze_expand_decoder", FEATURE_SCALE=[4, 8, 16, 32], INTER_CHANNELS=[256, 256, 128, 128],
                      NORMALIZATION_LAYER="gn", GN_NUM_GROUPS=32, POOL_TYPE="avg", FOREGROUND_CHANNEL=True),
            SEEDINESS=NS(HEAD_TYPE="squeeze_expand_decoder", INTER_CHANNELS=[256, 256, 128, 128], FEATURE_SCALE=[32, 16, 8, 4],
                         NORMALIZATION_LAYER="gn", GN_NUM_GROUPS=32, POOL_TYPE="avg"),
        ),
        TRAINING=NS(LOSS_AT_FULL_RES=False, FREEZE_BACKBONE=False,
                    # the optimiser and the loop (defaults.yaml:11-31; stemseg_amd.training).  The presets below leave them at the defaults: a
                    # dataset's schedule (youtube_vis.yaml: exponential decay over 160 000 iterations) comes from its YAML through the overlay
                    MODE="", MIXED_PRECISION=False, MIXED_PRECISION_OPT_LEVEL="O1", BATCH_SIZE=2, WEIGHT_DECAY=0.0001, MAX_ITERATIONS=120000,
                    ACCUMULATE_GRADIENTS=True, MAX_SAMPLES_PER_GPU=1, CLIP_GRADIENTS=False, OPTIMIZER="SGD", INITIAL_LR=0.001,
                    LR_DECAY_TYPE="step", LR_DECAY_STEPS=[20000, 50000], LR_DECAY_FACTOR=0.1, LR_EXP_DECAY_FACTOR=0.001,
                    LR_EXP_DECAY_START=40000, LR_EXP_DECAY_STEPS=60000, MOMENTUM=0.9, NESTEROV=True,
                    LOSSES=NS(SEMSEG="CrossEntropy", WEIGHT_SEMSEG=1.0,        # (defaults.yaml:32-41; no preset changes the weights)
                              EMBEDDING=NS(WEIGHT_REGULARIZATION=0.001, WEIGHT_LOVASZ=1.0, WEIGHT_VARIANCE_SMOOTHNESS=10.0,
                                           WEIGHT_SEEDINESS=1.0, WEIGHT=1.0, FREE_DIM_STDS=[]))),
        # (defaults.yaml:85-113; the frame gaps, the duplication switches and the dataset weights are the training loader's, stemseg_amd.data)
        DATA=NS(DAVIS=NS(INFERENCE_FRAME_OVERLAP=6, FRAME_GAP_LOWER=16, FRAME_GAP_UPPER=16, SINGLE_INSTANCE_DUPLICATION=False,
                         COCO_WEIGHT=0.25, PASCAL_VOC_WEIGHT=0.1, YOUTUBE_VIS_WEIGHT=0.35, DAVIS_WEIGHT=0.3),
                YOUTUBE_VIS=NS(INFERENCE_FRAME_OVERLAP=4, FRAME_GAP_LOWER=8, FRAME_GAP_UPPER=8, SINGLE_INSTANCE_DUPLICATION=True,
                               COCO_WEIGHT=0.3, PASCAL_VOC_WEIGHT=0.1, YOUTUBE_VIS_WEIGHT=0.6),
                KITTI_MOTS=NS(INFERENCE_FRAME_OVERLAP=4, FRAME_GAP_LOWER=8, FRAME_GAP_UPPER=8, MAPILLARY_WEIGHT=0.0, KITTI_MOTS_WEIGHT=1.0)),
        CLUSTERING=NS(MIN_SEEDINESS_PROB=0.8, PRIMARY_PROB_THRESHOLD=0.5, SECONDARY_PROB_THRESHOLD=0.3),
    )


def _apply(c, preset):
    if preset in ("davis", "davis_2"):   # config/davis_1.yaml (NUM_FRAMES 8) / davis_2.yaml (NUM_FRAMES 16: what inference/main.py:188-195 loads
        # for --dataset davis when the checkpoint directory holds no config.yaml); the hot-path keys differ in NUM_FRAMES only
        c.INPUT.MIN_DIM, c.INPUT.MAX_DIM, c.INPUT.NUM_FRAMES = 736, 1248, (16 if preset == "davis_2" else 8)
        c.MODEL.EMBEDDING_DIM_MODE, c.MODEL.USE_SEEDINESS_HEAD, c.MODEL.USE_SEMSEG_HEAD = "xyff", True, False
        c.MODEL.EMBEDDINGS.EMBEDDING_SIZE = 4
        c.TRAINING.LOSSES.EMBEDDING.FREE_DIM_STDS = [0.3, 0.3]
    elif preset == "ytvis":         # config/youtube_vis.yaml
        c.INPUT.MIN_DIM, c.INPUT.MAX_DIM, c.INPUT.NUM_FRAMES, c.INPUT.NUM_CLASSES = 640, 1196, 8, 41
        c.MODEL.EMBEDDING_DIM_MODE, c.MODEL.USE_SEEDINESS_HEAD, c.MODEL.USE_SEMSEG_HEAD = "xyff", False, True
        c.MODEL.EMBEDDINGS.EMBEDDING_SIZE = 4
        c.MODEL.SEMSEG.INTER_CHANNELS = [256, 256, 256, 256]
        c.TRAINING.LOSSES.EMBEDDING.FREE_DIM_STDS = [0.3, 0.3]
    elif preset in ("kittimots", "kittimots_1"):     # config/kitti_mots_2.yaml / kitti_mots_1.yaml
        c.INPUT.MIN_DIM, c.INPUT.MAX_DIM, c.INPUT.NUM_FRAMES, c.INPUT.NUM_CLASSES = 736, 1792, 8, 3
        c.MODEL.EMBEDDING_DIM_MODE, c.MODEL.USE_SEEDINESS_HEAD, c.MODEL.USE_SEMSEG_HEAD = "xyt", False, True
        c.CLUSTERING.MIN_SEEDINESS_PROB = 0.95
        if preset == "kittimots_1":     # stage one of the published recipe: clips from single Mapillary images, and -- because this preset
            # exists to be trained from the command line -- the schedule of its YAML as well
            c.INPUT.MAX_DIM = 1248
            c.DATA.KITTI_MOTS.MAPILLARY_WEIGHT, c.DATA.KITTI_MOTS.KITTI_MOTS_WEIGHT = 1.0, 0.0
            t = c.TRAINING
            t.INITIAL_LR, t.LR_DECAY_TYPE, t.MAX_ITERATIONS = 0.001, "exponential", 80000
            t.LR_EXP_DECAY_FACTOR, t.LR_EXP_DECAY_START, t.LR_EXP_DECAY_STEPS = 0.1, 60000, 20000
    elif preset not in (None, "defaults"):
        raise ValueError("unknown preset '%s' (davis | davis_2 | ytvis | kittimots | kittimots_1 | defaults)" % preset)
    return c


# TRAINING.MODE of each preset's YAML (davis_1.yaml:13, youtube_vis.yaml:15, kitti_mots_2.yaml:11): the presets leave the key itself alone
PRESET_TRAINING_MODES = {"davis": "davis", "davis_2": "davis", "ytvis": "youtube_vis", "kittimots": "kitti_mots",
                         "kittimots_1": "kitti_mots"}


def make_cfg(preset=None):
    return _apply(_defaults(), preset)


cfg = make_cfg()


def load_preset(preset):
    """Re-initialise the global cfg in place (call BEFORE constructing any module)."""
    new = make_cfg(preset)
    for k, v in vars(new).items():
        setattr(cfg, k, copy.deepcopy(v))
    return cfg


# ---- external configuration sources (stemseg_amd.overlay: the reference's own global cfg) -----------------------------
_sources = []


def register_source(fn):
    """fn(cfg) copies values into ``cfg``; called by ``refresh()`` -- i.e. whenever a model is built or run."""
    if fn not in _sources:
        _sources.append(fn)


def unregister_source(fn):
    if fn in _sources:
        _sources.remove(fn)


def refresh():
    for fn in _sources:
        fn(cfg)
    return cfg
