"""GPU tests of the image datasets and the instance duplicator end to end (stemseg_amd/data/coco_data_loader.py,
pascal_voc_data_loader.py, instance_duplicator.py, ``data.common.device_collate``) on a synthetic dataset: the golden's JPEG / PNG
frames with hand-made masks, and the hand-written category tables of tests/golden/metainfo/.

A batch entry is checked in two stages, because a warped uint8 may sit one level off the fp64 oracle inside the rounding band, and one
level is far more than the 1e-4 of the pre-processing: first the device's warp (or paste) of the recipe against tests/augment_oracle.py
under its band rule; then ``device_collate``'s images against the oracle's pre-processing of those very frames within 1e-4, and its
masks against the oracle's resize of those very planes under the tie rule of tests/data_oracle.py."""
import os
import random

import numpy as np
import pytest
import torch

from tests import augment_oracle as ao
from tests import data_oracle as do

pytestmark = pytest.mark.gpu
METAINFO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metainfo")


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


@pytest.fixture(scope="module")
def gold(golden):
    return do.Golden(golden("data_pipeline"))


@pytest.fixture(scope="module")
def on_disk(gold, tmp_path_factory):
    """The golden's files, its video JSON, and two image-dataset JSONs over a 37 x 53 JPEG and a 45 x 40 PNG: three overlapping instances
    each (categories 1, 2 and the dropped 4), Pascal VOC with an ignore region and one instance below the area filter."""
    base = str(tmp_path_factory.mktemp("image_dataset"))
    vds = gold.write(base)
    ao.write_image_datasets(base)
    return base, vds


@pytest.fixture()
def cfg(gold, monkeypatch):
    from stemseg_amd import config
    config.load_preset("defaults")
    gold.configure(config.cfg)
    monkeypatch.setenv("STEMSEG_METAINFO_DIR", METAINFO)
    yield config.cfg
    config.load_preset("defaults")


def check_image_entry(hip, cfg, recipe, images, target, new_hw, pad_hw, what):
    from stemseg_amd.data.common import image_clip_parameters
    w, h = recipe["size"]
    T, N = len(recipe["perm"]), recipe["n_instances"]
    src, planes, ref, blurs = ao.image_recipe_warp(recipe, do.decode_image)
    # stage 1: the device's warp of this recipe (the mirror folded into the matrices) against the oracle's (the source mirrored first)
    raw = do.decode_image(recipe["frames"][0])
    from tests import writer_oracle as wo
    raw_planes = np.ascontiguousarray(np.stack([wo.decode(wo.string_to_counts(s), h, w) for s in recipe["rle"]]), dtype=np.uint8)
    hinvs, jitter, dev_blurs = image_clip_parameters(recipe)
    frames, wplanes, invalid = hip.warp_clip(torch.from_numpy(raw).cuda(), torch.from_numpy(raw_planes).cuda(), hinvs, jitter)
    ao.check_warp(frames.cpu().numpy(), wplanes.cpu().numpy(), invalid.cpu().numpy(), ref, what)
    assert [b is None for b in blurs] == [b is None for b in dev_blurs]
    blurred = hip.motion_blur(frames, dev_blurs)
    ref_blur, soft = ao.motion_blur(frames.cpu().numpy(), blurs)
    ao.check_u8(blurred.cpu().numpy(), ref_blur, soft, what + " blur")
    k0 = recipe["perm"].index(0)
    assert np.array_equal(blurred[k0].cpu().numpy(), src) and not invalid[k0].any(), "the image itself goes through unchanged (mirrored or not)"
    # stage 2: the batch entry against the oracle's pre-processing / resize of those frames and planes
    ref_images = ao.preprocess_masked(blurred.cpu().numpy(), invalid.cpu().numpy(), new_hw, pad_hw, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD,
                                      cfg.INPUT.NORMALIZE_TO_UNIT_SCALE, not cfg.INPUT.BGR_INPUT)
    err = float(np.abs(images.cpu().numpy() - ref_images).max())
    print("%s: images differ from the oracle's by %.3g" % (what, err))
    assert err <= 1e-4
    every = wplanes.cpu().numpy().copy()
    every[:, k0] = planes                                          # the image itself keeps its own planes, overlaps and all
    hard, soft = do.resize_masks(every.reshape(-1, h, w), new_hw, pad_hw)
    got = torch.cat([target["masks"], target["ignore_masks"][None]], 0).cpu().numpy() if recipe["has_ignore"] else target["masks"].cpu().numpy()
    assert got.shape[0] == every.shape[0]
    do.check_tie_rule(got.reshape(-1, *pad_hw), hard, soft, new_hw, what + " masks")
    if not recipe["has_ignore"]:
        assert not target["ignore_masks"].any() and tuple(target["ignore_masks"].shape) == (T,) + tuple(pad_hw)
    assert (every[:N, k0].sum(0) > 1).any(), "the case must have overlapping instances in the image itself"


@pytest.mark.parametrize("which", ("coco", "pascal_voc"))
def test_device_collate_of_image_recipes_and_a_mixed_batch(hip, gold, on_disk, cfg, which):
    from stemseg_amd.data import CocoDataLoader, PascalVOCDataLoader
    from stemseg_amd.data.common import device_collate
    base, vds = on_disk
    ds = CocoDataLoader(base, os.path.join(base, "coco.json"), True) if which == "coco" else \
        PascalVOCDataLoader(base, os.path.join(base, "pascal_voc.json"), True)
    assert len(ds) == 2 and [len(s.segmentations) for s in ds.samples] == ([3, 3] if which == "coco" else [2, 2])
    for seed in range(20):          # the first seed that gives a mirrored and a plain sample, and a blurred frame
        random.seed(seed)
        recipes = [ds[0], ds[1], ds[0]]
        if {r["flip"] for r in recipes} == {True, False} and any(w["blur"] is not None for r in recipes for w in r["warps"]):
            break
    assert {r["flip"] for r in recipes} == {True, False} and any(w["blur"] is not None for r in recipes for w in r["warps"])
    video = do.make_loader("davis", base, vds)
    video.samples = [do.pick_clip(video.sequences, "a", do.CLIP_A)]
    batch = recipes + [video[0]]
    image_seqs, targets, meta = device_collate(batch)
    torch.cuda.synchronize()
    pad_hw = tuple(image_seqs.max_size)
    for n, r in enumerate(recipes):
        assert targets[n]["category_ids"].cpu().tolist() == [1] * r["n_instances"] and r["has_ignore"] == (which == "pascal_voc")
        check_image_entry(hip, cfg, r, image_seqs.tensors[n], targets[n], tuple(image_seqs.image_sizes[n]), pad_hw, "%s %d" % (which, n))
    alone = device_collate([batch[3]])
    nh, nw = alone[0].image_sizes[0]
    assert torch.equal(alone[0].tensors[0][:, :, :nh, :nw], image_seqs.tensors[3][:, :, :nh, :nw]), "the video sample is what it is alone"
    assert torch.equal(alone[1][0]["masks"][..., :nh, :nw], targets[3]["masks"][..., :nh, :nw])
    assert meta[0]["category_labels"] == ["object"] * recipes[0]["n_instances"]


def test_category_tables_and_missing_metainfo(on_disk, cfg, monkeypatch, tmp_path):
    from stemseg_amd.data import CocoDataLoader, PascalVOCDataLoader
    base, _ = on_disk
    ds = CocoDataLoader(base, os.path.join(base, "coco.json"), False)                  # keep_ytvis: categories 1 and 2, mapped to 1 and 21
    assert [s.categories for s in ds.samples] == [[1, 2, 1]] * 2 and ds[0]["category_ids"] == [1, 21, 1]
    assert ds[0]["meta_info"]["category_labels"] == ["person", "motorbike", "person"]
    ds = PascalVOCDataLoader(base, os.path.join(base, "pascal_voc.json"), False)       # area filter drops the 15-pixel instance, keep_ytvis category 2
    assert [s.categories for s in ds.samples] == [[1]] * 2 and ds[0]["category_ids"] == [2]
    monkeypatch.setenv("STEMSEG_METAINFO_DIR", str(tmp_path))
    with pytest.raises(FileNotFoundError, match=r"coco\.yaml.*STEMSEG_METAINFO_DIR"):
        CocoDataLoader(base, os.path.join(base, "coco.json"), True)


def test_duplicated_youtube_vis_sample(hip, gold, on_disk, cfg):
    """A clip reduced to one instance, built with the duplicator on: the recipe carries the decision, the batch entry has two instances."""
    from stemseg_amd.data import YoutubeVISDataLoader
    from stemseg_amd.data.common import device_collate
    from tests import writer_oracle as wo
    base, vds = on_disk
    with pytest.raises(NotImplementedError, match=r"DATA\.YOUTUBE_VIS\.SINGLE_INSTANCE_DUPLICATION"):
        YoutubeVISDataLoader(base, vds, 3, category_agnostic=False, single_instance_duplication=True)
    ds = YoutubeVISDataLoader(base, vds, 3, category_agnostic=False, single_instance_duplication=True, device_augmentation=True)
    clip = do.pick_clip(ds.sequences, "a", do.CLIP_A)
    lone = clip.instance_ids[0]
    clip.instance_categories = {lone: clip.instance_categories[lone]}
    clip.segmentations = [{i: s for i, s in seg.items() if i == lone} for seg in clip.segmentations]
    ds.samples = [clip]
    for seed in range(20):
        random.seed(seed)
        recipe = ds[0]
        if "duplicate" in recipe:
            break
    dup = recipe["duplicate"]
    assert recipe["n_instances"] == 1 and len(recipe["category_ids"]) == 2 and recipe["category_ids"][0] == recipe["category_ids"][1]
    w, h = recipe["size"]
    T = len(recipe["frames"])
    frames = np.stack([do.decode_image(f) for f in recipe["frames"]])
    mask = np.zeros((T, h, w), np.uint8)
    for _, t, s in recipe["rle"]:
        mask[t] = wo.decode(wo.string_to_counts(s), h, w)
    assert dup["boxes"] == [ao.bbox(m) for m in mask]
    ref = ao.duplicate_instance(frames, mask, dup["boxes"], dup["flip"], dup["shifts"])
    assert ref["pasted"].any()
    got_f, got_m = hip.duplicate_instance(torch.from_numpy(frames).cuda(), torch.from_numpy(mask).cuda(), dup["boxes"], dup["flip"], dup["shifts"])
    band = ao.weight_band(ref["weight"])
    ao.check_bits(got_m[1].cpu().numpy(), ref["masks"][1], band, "copy")
    ao.check_bits(got_m[0].cpu().numpy(), ref["masks"][0], band, "original")
    agree = (got_m[1].cpu().numpy() == ref["masks"][1])[..., None]
    ao.check_u8(np.where(agree, got_f.cpu().numpy(), ref["frames"]), ref["frames"], ref["soft"], "pasted frames")
    image_seqs, targets, _ = device_collate([recipe])
    new_hw, pad_hw = tuple(image_seqs.image_sizes[0]), tuple(image_seqs.max_size)
    ref_images = ao.preprocess_masked(got_f.cpu().numpy(), np.zeros((T, h, w), np.uint8), new_hw, pad_hw, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD,
                                      cfg.INPUT.NORMALIZE_TO_UNIT_SCALE, not cfg.INPUT.BGR_INPUT)
    assert float(np.abs(image_seqs.tensors[0].cpu().numpy() - ref_images).max()) <= 1e-4
    hard, soft = do.resize_masks(got_m.cpu().numpy().reshape(-1, h, w), new_hw, pad_hw)
    assert tuple(targets[0]["masks"].shape) == (2, T) + pad_hw
    do.check_tie_rule(targets[0]["masks"].cpu().numpy().reshape(-1, *pad_hw), hard, soft, new_hw, "duplicated masks")
    assert not targets[0]["ignore_masks"].any()


def test_refusals_that_stay_with_the_switch_on(on_disk, cfg, monkeypatch):
    from stemseg_amd.data import YoutubeVISDataLoader
    from stemseg_amd.training.utils import create_training_dataset
    base, vds = on_disk
    with pytest.raises(NotImplementedError, match="apply_augmentation=True"):
        YoutubeVISDataLoader(base, vds, 3, apply_augmentation=True, device_augmentation=True)
    for var in ("YOUTUBE_VIS_BASE_DIR", "DAVIS_BASE_DIR", "KITTIMOTS_BASE_DIR", "STEMSEG_JSON_ANNOTATIONS_DIR"):
        monkeypatch.setenv(var, base)
    cfg.DATA.KITTI_MOTS.MAPILLARY_WEIGHT, cfg.DATA.KITTI_MOTS.KITTI_MOTS_WEIGHT, cfg.INPUT.NUM_CLASSES = 0.5, 0.5, 3
    with pytest.raises(NotImplementedError, match=r"DATA\.KITTI_MOTS\.MAPILLARY_WEIGHT"):
        create_training_dataset(4, mode="kitti_mots", device_augmentation=True)


CHILD = r"""
import sys
import numpy as np, torch
sys.path[:0] = [{root!r}, {pkg!r}]
from stemseg_amd import config
from tests import synth
load = config.load_preset
def small(preset):
    c = load(preset)
    c.MODEL.BACKBONE.TYPE, c.MODEL.BACKBONE.PRETRAINED_WEIGHTS = "R-50-FPN", "synthetic_r50.pth"
    c.INPUT.NUM_FRAMES, c.INPUT.MIN_DIM, c.INPUT.MAX_DIM = {frames}, {min_dim}, {max_dim}
    c.DATA.DAVIS.FRAME_GAP_LOWER, c.DATA.DAVIS.FRAME_GAP_UPPER = {davis_gap}
    c.DATA.YOUTUBE_VIS.FRAME_GAP_LOWER, c.DATA.YOUTUBE_VIS.FRAME_GAP_UPPER = {ytvis_gap}
    c.TRAINING.MAX_ITERATIONS, c.TRAINING.BATCH_SIZE = 8, 1          # (8 samples: every dataset of the mix gets at least one)
    return c
config.load_preset = small
small("davis")
from stemseg_amd.modeling.model_builder import build_model
bb = build_model().backbone
sd = synth.synth_state_dict([(k, v.shape) for k, v in bb.state_dict().items()], 11)
import os
os.makedirs(os.path.join(os.environ["STEMSEG_MODELS_DIR"], "pretrained"))
torch.save({{k: torch.from_numpy(np.asarray(v)).reshape(bb.state_dict()[k].shape) for k, v in sd.items()}},
           os.path.join(os.environ["STEMSEG_MODELS_DIR"], "pretrained", "synthetic_r50.pth"))
del bb
import runpy
sys.argv[0] = "stemseg_amd.training.main"
runpy.run_module("stemseg_amd.training.main", run_name="__main__")          # what `python -m stemseg_amd.training.main <flags>` runs
"""


def test_command_line_trains_the_davis_preset_as_shipped(hip, gold, on_disk, tmp_path):
    """``python -m stemseg_amd.training.main --cfg davis --build_data_loader --device_augmentation`` in a child process, the preset shrunk
    to the synthetic dataset (R-50 from a synthetic backbone file, the golden's frame count and sizes) but with its dataset mix AS
    SHIPPED -- COCO, Pascal VOC, YouTube-VIS with the duplicator, DAVIS: eight iterations of one sample and a checkpoint.  (Without the flag the mix is refused at the COCO weight:
    tests/test_image_datasets_host.py.)"""
    import shutil
    import subprocess
    import sys
    base, vds = on_disk
    for name in ("youtube_vis_train.json", "davis_train.json"):
        shutil.copy(vds, str(tmp_path / name))
    for name in ("coco.json", "pascal_voc.json"):
        shutil.copy(os.path.join(base, name), str(tmp_path / name))
    os.makedirs(str(tmp_path / "ytvis"))
    os.symlink(base, str(tmp_path / "ytvis" / "train"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gaps = gold.config["GAPS"]
    script = CHILD.format(root=root, pkg=os.path.join(root, "stem-seg_amd"), frames=gold.config["NUM_FRAMES"], min_dim=gold.config["MIN_DIM"],
                          max_dim=gold.config["MAX_DIM"], davis_gap=tuple(gaps["DAVIS"]), ytvis_gap=tuple(gaps["YOUTUBE_VIS"]))
    env = dict(os.environ, STEMSEG_JSON_ANNOTATIONS_DIR=str(tmp_path), YOUTUBE_VIS_BASE_DIR=str(tmp_path / "ytvis"), DAVIS_BASE_DIR=base,
               COCO_TRAIN_IMAGES_DIR=base, PASCAL_VOC_IMAGES_DIR=base, STEMSEG_METAINFO_DIR=METAINFO, STEMSEG_MODELS_DIR=str(tmp_path / "models"))
    flags = ["--model_dir", "run", "--cfg", "davis", "--num_cpu_workers", "0", "--save_interval", "8", "--display_interval", "1", "--build_data_loader"]
    r = subprocess.run([sys.executable, "-c", script] + flags + ["--device_augmentation"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "iteration 00008" in r.stderr and "Training datasets: COCO, PascalVOC, YouTubeVIS, Davis" in r.stderr, r.stderr[-3000:]
    assert "000008.pth" in os.listdir(str(tmp_path / "models" / "checkpoints" / "run"))


class Recording(torch.utils.data.Dataset):
    """One sample of ``dataset``; keeps the recipe it handed out (the image datasets draw their warps in ``__getitem__``)."""

    def __init__(self, dataset, index):
        self.dataset, self.index, self.recipes = dataset, index, []

    def __len__(self):
        return 1

    def __getitem__(self, i):
        self.recipes.append(self.dataset[self.index])
        return self.recipes[-1]


def _davis_mix(gold, base, vds, tmp_path, monkeypatch, config):
    """The davis preset shrunk to the synthetic dataset (R-50, the golden's frame count and sizes), its mix with COCO at 0.4."""
    import shutil
    from stemseg_amd.training.utils import create_training_dataset
    for name in ("youtube_vis_train.json", "davis_train.json"):
        shutil.copy(vds, str(tmp_path / name))
    for name in ("coco.json", "pascal_voc.json"):
        shutil.copy(os.path.join(base, name), str(tmp_path / name))
    os.makedirs(str(tmp_path / "ytvis"))
    os.symlink(base, str(tmp_path / "ytvis" / "train"))
    for var, value in (("YOUTUBE_VIS_BASE_DIR", str(tmp_path / "ytvis")), ("DAVIS_BASE_DIR", base), ("COCO_TRAIN_IMAGES_DIR", base),
                       ("PASCAL_VOC_IMAGES_DIR", base), ("STEMSEG_JSON_ANNOTATIONS_DIR", str(tmp_path)), ("STEMSEG_METAINFO_DIR", METAINFO)):
        monkeypatch.setenv(var, value)
    config.load_preset("davis")
    c = config.cfg
    c.MODEL.BACKBONE.TYPE = "R-50-FPN"
    gold.configure(c)
    c.TRAINING.MAX_ITERATIONS, c.TRAINING.BATCH_SIZE = 8, 1
    d = c.DATA.DAVIS
    d.COCO_WEIGHT, d.PASCAL_VOC_WEIGHT, d.YOUTUBE_VIS_WEIGHT, d.DAVIS_WEIGHT = 0.4, 0.1, 0.25, 0.25
    random.seed(1)
    said = []
    dataset = create_training_dataset(8, print_fn=said.append, mode="davis", device_augmentation=True)
    assert said == ["Training datasets: COCO, PascalVOC, YouTubeVIS, Davis"] and dataset.samples_per_dataset == [3, 1, 2, 2]
    return dataset


def _lone_instance_loader(base, vds):
    from stemseg_amd.data import YoutubeVISDataLoader
    ds = YoutubeVISDataLoader(base, vds, 3, category_agnostic=True, single_instance_duplication=True, device_augmentation=True)
    clip = do.pick_clip(ds.sequences, "a", do.CLIP_A)
    lone = clip.instance_ids[0]
    clip.instance_categories = {lone: clip.instance_categories[lone]}
    clip.segmentations = [{i: s for i, s in seg.items() if i == lone} for seg in clip.segmentations]
    ds.samples = [clip]
    return ds


def oracle_targets(hip, cfg, recipe, new_hw, pad_hw):
    """The targets of one recipe from the oracle's resize of the DEVICE's warped planes / pasted masks (which ``check_image_entry`` and
    test_duplicated_youtube_vis_sample hold to the oracle's under the band rule): (masks [I,T,ph,pw], ignore_masks [T,ph,pw])."""
    from stemseg_amd.data.common import image_clip_parameters
    from tests import writer_oracle as wo
    w, h = recipe["size"]
    if recipe.get("kind") == "image":
        T, N = len(recipe["perm"]), recipe["n_instances"]
        planes = np.ascontiguousarray(np.stack([wo.decode(wo.string_to_counts(s), h, w) for s in recipe["rle"]]), dtype=np.uint8)
        hinvs, jitter, _ = image_clip_parameters(recipe)
        raw = torch.from_numpy(do.decode_image(recipe["frames"][0])).cuda()
        every = hip.warp_clip(raw, torch.from_numpy(planes).cuda(), hinvs, jitter)[1].cpu().numpy().copy()
        every[:, recipe["perm"].index(0)] = planes[:, :, ::-1] if recipe["flip"] else planes
        hard, _ = do.resize_masks(every.reshape(-1, h, w), new_hw, pad_hw)
        hard = hard.reshape((-1, T) + tuple(pad_hw))
        return hard[:N], (hard[N] if recipe["has_ignore"] else np.zeros((T,) + tuple(pad_hw), np.uint8))
    T = len(recipe["frames"])
    frames = np.stack([do.decode_image(f) for f in recipe["frames"]])
    mask = np.zeros((T, h, w), np.uint8)
    for _, t, s in recipe["rle"]:
        mask[t] = wo.decode(wo.string_to_counts(s), h, w)
    dup = recipe["duplicate"]
    both = hip.duplicate_instance(torch.from_numpy(frames).cuda(), torch.from_numpy(mask).cuda(), dup["boxes"], dup["flip"], dup["shifts"])[1]
    hard, _ = do.resize_masks(both.cpu().numpy().reshape(-1, h, w), new_hw, pad_hw)
    return hard.reshape((2, T) + tuple(pad_hw)), np.zeros((T,) + tuple(pad_hw), np.uint8)


@pytest.mark.parametrize("which", ("coco", "pascal_voc", "duplicated"))
def test_trainer_iteration_on_the_davis_mix_equals_a_twin_fed_the_oracles_batch(hip, gold, on_disk, tmp_path, monkeypatch, which):
    """One ``Trainer`` iteration on the davis preset's mix (COCO weight 0.4; R-50, 4 frames, 64 x 96) fed by ``create_training_data_loader``
    with a COCO sample, a Pascal VOC sample (ignore region) or a duplicated YouTube-VIS clip: the logged losses are, bit for bit, those of
    a twin model fed the device's images with the ORACLE's targets.  Two-stage, as the collate tests: the oracle's targets are its resize
    of the device's warped planes, which those tests hold to the fp64 oracle; the premise that no target pixel of the loader's batch
    differs from them is asserted first, and for the image samples ``check_image_entry`` runs on the very recipe the trainer saw."""
    from stemseg_amd import config
    from stemseg_amd.data.common import device_collate
    from stemseg_amd.training import configure_trainable
    from stemseg_amd.training.model_output_manager import ModelOutputManager
    from stemseg_amd.training.utils import create_training_data_loader
    from stemseg_amd.utils.constants import ModelOutput
    from tests.test_gpu_trainer import OPTS, _build, _trainer, _training_cfg
    base, vds = on_disk
    try:
        dataset = _davis_mix(gold, base, vds, tmp_path, monkeypatch, config)
        if which == "duplicated":
            one = Recording(_lone_instance_loader(base, vds), 0)
        else:
            ds_index = 0 if which == "coco" else 1
            one = Recording(dataset, [i for i, (d, _) in enumerate(dataset.id_mapping) if d == ds_index][0])
        m = _build()
        initial = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        for seed in range(20):          # (the duplicator gives up on some draws: the first seed for which the sample is what the case names)
            random.seed(seed)
            probe = one.dataset[one.index]
            if ("duplicate" in probe) == (which == "duplicated"):
                break
        tr = _trainer(tmp_path / "session", m, _training_cfg(BATCH_SIZE=1, MAX_ITERATIONS=1))
        (tmp_path / "session").mkdir(exist_ok=True)
        tr.data_loader = create_training_data_loader(one, 1, False, num_workers=0, device_augmentation=True)
        random.seed(seed)
        tr.start(OPTS)
        torch.cuda.synchronize()
        assert tr.elapsed_iterations == 1 and len(one.recipes) == 1
        recipe = one.recipes[0]
        assert (recipe.get("kind") == "image") == (which != "duplicated") and ("duplicate" in recipe) == (which == "duplicated")
        assert recipe.get("has_ignore", False) == (which == "pascal_voc")
        point = dict(tr.logger.last_point)
        image_seqs, targets, _ = device_collate([recipe])
        new_hw, pad_hw = tuple(image_seqs.image_sizes[0]), tuple(image_seqs.max_size)
        if which != "duplicated":
            check_image_entry(hip, config.cfg, recipe, image_seqs.tensors[0], targets[0], new_hw, pad_hw, which)
        masks, ignore_masks = oracle_targets(hip, config.cfg, recipe, new_hw, pad_hw)
        same = np.array_equal(targets[0]["masks"].cpu().numpy(), masks) and np.array_equal(targets[0]["ignore_masks"].cpu().numpy(), ignore_masks)
        assert same, "the premise does not hold: a target pixel of the loader's batch differs from the oracle's, so the losses cannot be compared bit for bit"
        assert masks.any() and ignore_masks.any() == (which == "pascal_voc")
        n_targets = recipe["n_instances"] + (1 if which == "duplicated" else 0)
        assert masks.shape[0] == n_targets and recipe["category_ids"] == [1] * n_targets
        hand = [{"masks": torch.from_numpy(np.ascontiguousarray(masks)).cuda(), "ignore_masks": torch.from_numpy(np.ascontiguousarray(ignore_masks)).cuda(),
                 "category_ids": torch.tensor(recipe["category_ids"], dtype=torch.long).cuda()}]
        twin = configure_trainable(_build(initial))
        out = twin(image_seqs, hand)
        gathered = ModelOutputManager(1)
        gathered(out)
        values = gathered.reset()[0]
        assert set(out[ModelOutput.OPTIMIZATION_LOSSES]) <= set(values) <= set(point)
        for k, v in values.items():
            assert point[k] == v.item(), (k, point[k], v)
        assert len(values) >= 2 and all(np.isfinite(point[k]) for k in point)
    finally:
        config.load_preset("defaults")


def test_device_collate_names_an_image_whose_file_has_another_size(hip, gold, on_disk, cfg):
    from stemseg_amd.data import CocoDataLoader
    from stemseg_amd.data.common import device_collate
    base, _ = on_disk
    recipe = CocoDataLoader(base, os.path.join(base, "coco.json"), True)[0]
    recipe["frames"] = [gold.files["b/00001.png"]]          # 45 x 40, the json says 37 x 53
    with pytest.raises(ValueError, match=r"a/00000\.jpg.*\(45, 40\).*\(37, 53\)"):
        device_collate([recipe])
