"""CPU tests of the host half of the augmentation (stemseg_amd/data/image_to_seq_augmenter.py, instance_duplicator.py): what is sampled
stays inside its ranges and is reproducible from a seed, the calls to ``random`` are the reference's in order and number, the boxes and
areas read off the annotation strings are those of the decoded masks."""
import os
import pickle
import random

import numpy as np
import pytest

from tests import augment_oracle as ao
from tests import writer_oracle as wo


@pytest.fixture(scope="module")
def aug():
    from stemseg_amd.data import image_to_seq_augmenter as m
    return m


@pytest.fixture(scope="module")
def dup():
    from stemseg_amd.data import instance_duplicator as m
    return m


# ------------------------------------------------------------------------------------------------ ImageToSeqAugmenter.sample
def test_sampled_parameters_stay_inside_their_ranges(aug):
    a = aug.ImageToSeqAugmenter()
    seen = {"flags": set(), "blur": set(), "add": set(), "hs": set()}
    for seed in range(400):
        s = a.sample(640, 480, random.Random(seed))
        p = s["params"]
        assert s["flags"] in (1, 2, 3) and -50 <= s["add"] <= 50 and -15 <= s["hs"] <= 15
        assert (s["add"] == 0 or s["flags"] & 1) and (s["hs"] == 0 or s["flags"] & 2)
        assert -20 <= p["rotation"] <= 20 and all(-0.15 <= t <= 0.15 for t in p["translate"]) and p["scale"] == 1.0
        assert len(p["corners"]) == 4 and all(0 <= j < 1 for c in p["corners"] for j in c)
        if s["blur"] is not None:
            k, direction, angle = p["blur"]
            assert k in (7, 9) and -1 <= direction <= 1 and 0 <= angle <= 360 and np.asarray(s["blur"]).shape == (k, k)
            assert abs(np.asarray(s["blur"], np.float64).sum() - 1) < 1e-6 and np.asarray(s["blur"]).min() >= 0
        seen["flags"].add(s["flags"]); seen["blur"].add(None if s["blur"] is None else len(s["blur"]))
        seen["add"].add(s["add"]); seen["hs"].add(s["hs"])
    assert seen["flags"] == {1, 2, 3} and seen["blur"] == {None, 7, 9}
    assert {-50, 50} <= seen["add"] and {-15, 15} <= seen["hs"], "the ends of the integer ranges are drawn"
    pickle.loads(pickle.dumps(s))
    assert all(isinstance(v, (float, int)) for v in s["hinv"] + s["matrix"])


def test_composed_matrix_times_its_inverse_is_the_identity(aug):
    a = aug.ImageToSeqAugmenter()
    for seed in range(50):
        s = a.sample(640, 480, random.Random(seed))
        prod = np.asarray(s["matrix"]).reshape(3, 3) @ np.asarray(s["hinv"]).reshape(3, 3)
        assert np.abs(prod / prod[2, 2] - np.eye(3)).max() < 1e-12 * max(1.0, np.abs(np.asarray(s["matrix"])).max())
        h = np.asarray(s["hinv"])
        assert abs(h[6] * 319.5 + h[7] * 239.5 + h[8] - 1) < 1e-12, "the denominator is 1 at the frame's centre"
        u, v, inside = ao.source_coords(h, 480, 640)
        assert inside[200:280, 280:360].all(), "the middle of the frame reads inside the source"


def test_perspective_takes_the_inset_quadrilateral_to_the_frame_and_affine_turns_about_the_centre(aug):
    W, H = 53, 37
    m = aug.perspective_matrix([(0.1, 0.05), (0.02, 0.08), (0.07, 0.03), (0.04, 0.09)], W, H)
    for (x, y), (X, Y) in zip([(0.1 * 52, 0.05 * 36), (0.98 * 52, 0.08 * 36), (0.93 * 52, 0.97 * 36), (0.04 * 52, 0.91 * 36)],
                              [(0, 0), (52, 0), (52, 36), (0, 36)]):
        q = m @ [x, y, 1]
        assert abs(q[0] / q[2] - X) < 1e-9 and abs(q[1] / q[2] - Y) < 1e-9
    assert np.allclose(aug.perspective_matrix([(0, 0)] * 4, W, H), np.eye(3), atol=1e-12)
    a = aug.affine_matrix(17.0, (0, 0), 1.0, W, H)
    assert np.allclose(a @ [26, 18, 1], [26, 18, 1], atol=1e-12)
    assert np.allclose(aug.affine_matrix(0.0, (3.5, -2), 1.0, W, H), [[1, 0, 3.5], [0, 1, -2], [0, 0, 1]], atol=1e-12)
    assert np.allclose(aug.affine_matrix(90.0, (0, 0), 1.0, W, H) @ [27, 18, 1], [26, 19, 1], atol=1e-12)


def test_blur_matrix_is_a_line_at_0_and_90_degrees(aug):
    for k in (7, 9, 11):
        for direction in (-1.0, -0.3, 0.0, 0.8):
            d = (direction + 1) / 2
            line = np.linspace(d, 1 - d, k)
            m0, m90 = aug.blur_matrix(k, 0.0, direction), aug.blur_matrix(k, 90.0, direction)
            assert m0.dtype == np.float32 and abs(float(m0.sum()) - 1) < 1e-6 and abs(float(m90.sum()) - 1) < 1e-6
            assert np.count_nonzero(np.delete(m0, k // 2, axis=1)) == 0 and np.allclose(m0[:, k // 2], line / line.sum(), atol=1e-7)
            assert np.count_nonzero(np.delete(m90, k // 2, axis=0)) == 0 and np.allclose(np.sort(m90[k // 2]), np.sort(line / line.sum()), atol=1e-7)
        m = aug.blur_matrix(k, 33.0, 0.2)
        assert abs(float(m.sum()) - 1) < 1e-6 and m.min() >= 0 and np.count_nonzero(m) > k


def test_one_getrandbits_per_warp_and_seeded_runs_repeat(aug):
    a = aug.ImageToSeqAugmenter()
    random.seed(11)
    first = a.sample_clip(640, 480, 7)
    after = random.random()
    random.seed(11)
    seeds = [random.getrandbits(64) for _ in range(7)]
    assert random.random() == after, "sample_clip draws exactly one getrandbits(64) per warp from the global generator"
    assert first == [a.sample(640, 480, random.Random(s)) for s in seeds]
    random.seed(11)
    assert a.sample_clip(640, 480, 7) == first
    assert len({tuple(s["hinv"]) for s in first}) == 7


# ------------------------------------------------------------------------------------------------ boxes and areas off the strings
def test_rle_area_and_box_against_decoded_masks(dup):
    rng = np.random.RandomState(3)
    masks = [np.zeros((7, 5), np.uint8), np.ones((7, 5), np.uint8)]
    for h, w in ((7, 5), (37, 53), (45, 40)):
        for _ in range(12):
            m = np.zeros((h, w), np.uint8)
            y0, x0 = rng.randint(0, h), rng.randint(0, w)
            m[y0:rng.randint(y0, h) + 1, x0:rng.randint(x0, w) + 1] = 1
            m &= (rng.rand(h, w) < 0.8).astype(np.uint8)
            masks.append(m)
        full_cols = np.zeros((h, w), np.uint8)
        full_cols[:, 1:3] = 1                                  # one run over a column boundary
        masks.append(full_cols)
        masks.append(ao.disc_mask(1, h, w, w - 2, 2, 4, 3)[0])
    for m in masks:
        s = wo.counts_to_string(wo.encode(m))
        area, box = dup.rle_area_and_box(s, *m.shape)
        assert area == int(m.sum()) and box == ao.bbox(m), (m.shape, box, ao.bbox(m))
        assert dup.rle_area_and_box(s.encode("latin-1"), *m.shape) == (area, box)
    with pytest.raises(ValueError):
        dup.rle_area_and_box(wo.counts_to_string([3, 4]), 7, 5)


# ------------------------------------------------------------------------------------------------ the duplicator's decisions
W, H = 100, 80
DUP_CASES = {
    # name: (boxes, free multiplier / flip draws before the per-frame ones)
    "three free: small in the middle": ([(40, 30, 55, 45), (42, 30, 57, 45)], 3),
    "two free: low at the top, may still flip": ([(40, 0, 55, 10), (41, 0, 56, 10)], 2),
    "one free: narrow near the left, low near the bottom": ([(10, 60, 20, 70), (11, 60, 21, 70)], 1),
    "none free: wide on the left border, tall on the top border": ([(0, 0, 50, 40), (0, 0, 52, 40)], 0),
    "a frame without a box": ([(40, 30, 55, 45), None, (44, 30, 59, 45)], 3),
    "top and bottom: no vertical shift": ([(40, 0, 55, 80)], 2),
    "capped at 0.3 of the size": ([(5, 5, 95, 75)], 3),
}


@pytest.mark.parametrize("name", sorted(DUP_CASES))
def test_duplicator_draws_like_the_reference(dup, name):
    boxes, free = DUP_CASES[name]
    for seed in range(6):
        random.seed(seed)
        draws = [random.random() for _ in range(16)]
        expect, used = ao.duplicator_decision(boxes, W, H, draws)
        assert used == free + 2 * sum(b is not None for b in boxes), name
        random.seed(seed)
        got = dup.InstanceDuplicator()(boxes, W, H)
        assert got == expect, name
        assert random.random() == draws[used], "%s: the library drew another number of values" % name
        for b, sh in zip(boxes, got["shifts"]):
            assert (b is None) == (sh is None)
            if sh is not None:
                assert sh[0] <= np.float32(W * 0.3) and sh[1] <= np.float32(H * 0.3)
                assert 0.75 * (b[2] - b[0]) - 1e-4 <= abs(sh[0]) or sh[0] == float(np.float32(W * 0.3))
    if name.startswith("capped"):
        assert any(dup.InstanceDuplicator()(boxes, W, H)["shifts"][0][0] == float(np.float32(30.0)) for _ in range(20))
    pickle.loads(pickle.dumps(got))


def test_duplicator_gives_up_like_the_reference(dup):
    random.seed(0)
    before = random.getstate()
    assert dup.InstanceDuplicator()([(0, 10, 100, 20)], W, H) is None                      # touches left and right
    assert dup.InstanceDuplicator()([(0, 10, 30, 20), (70, 10, 100, 20)], W, H) is None    # ... in different frames
    assert random.getstate() == before, "an infeasible case draws nothing"
    assert dup.InstanceDuplicator()([(1, 2, 3)], W, H) is None                             # any exception: the sample stays as it is
    assert ao.duplicator_decision([(0, 10, 100, 20)], W, H, []) == (None, 0)


# ------------------------------------------------------------------------------------------------ the image datasets' recipes
METAINFO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metainfo")


@pytest.fixture(scope="module")
def on_disk(golden, tmp_path_factory):
    from tests import data_oracle as do
    gold = do.Golden(golden("data_pipeline"))
    base = str(tmp_path_factory.mktemp("image_dataset"))
    vds = gold.write(base)
    ao.write_image_datasets(base)
    return gold, base, vds


@pytest.fixture()
def cfg(on_disk, monkeypatch):
    from stemseg_amd import config
    config.load_preset("defaults")
    on_disk[0].configure(config.cfg)
    monkeypatch.setenv("STEMSEG_METAINFO_DIR", METAINFO)
    yield config.cfg
    config.load_preset("defaults")


def _plain(x):
    if isinstance(x, dict):
        return all(isinstance(k, str) and _plain(v) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return all(_plain(v) for v in x)
    return x is None or isinstance(x, (bytes, str, int, float, bool))


def test_image_recipes_are_plain_seeded_and_the_same_from_two_workers(on_disk, cfg):
    from torch.utils.data import DataLoader
    from stemseg_amd.data import CocoDataLoader, PascalVOCDataLoader
    gold, base, _ = on_disk
    for ds in (CocoDataLoader(base, os.path.join(base, "coco.json"), True), PascalVOCDataLoader(base, os.path.join(base, "pascal_voc.json"), True)):
        random.seed(3)
        first = [ds[0], ds[1]]
        after = random.random()
        for r in first:
            assert _plain(r) and pickle.loads(pickle.dumps(r)) == r and r["kind"] == "image"
            assert len(r["warps"]) == cfg.INPUT.NUM_FRAMES - 1 and sorted(r["perm"]) == list(range(cfg.INPUT.NUM_FRAMES))
            assert r["frames"] == [gold.files["a/00000.jpg" if r["size"] == (53, 37) else "b/00001.png"]]
            assert len(r["rle"]) == r["n_instances"] + int(r["has_ignore"]) and r["has_ignore"] == isinstance(ds, PascalVOCDataLoader)
        # the reference's order of calls: random() for the flip, [one getrandbits(64) per warp], shuffle of the permutation
        random.seed(3)
        for r in first:
            assert (random.random() < 0.5) == r["flip"]
            seeds = [random.getrandbits(64) for _ in range(cfg.INPUT.NUM_FRAMES - 1)]
            assert [w["hinv"] for w in r["warps"]] == [ds.augmenter.sample(r["size"][0], r["size"][1], random.Random(s))["hinv"] for s in seeds]
            perm = list(range(cfg.INPUT.NUM_FRAMES))
            random.shuffle(perm)
            assert perm == r["perm"]
        assert random.random() == after
    flips = set()
    for seed in range(12):
        random.seed(seed)
        flips.add(ds[0]["flip"])
    assert flips == {True, False}
    loader = DataLoader(ds, batch_size=1, collate_fn=list, num_workers=2, worker_init_fn=_seed_worker, multiprocessing_context="spawn")
    from_workers = [b[0] for b in loader]
    for i, r in enumerate(from_workers):          # sample i comes from worker i % 2, as its first sample
        random.seed(100 + i % 2)
        assert ds[i] == r


def _seed_worker(worker_id):
    random.seed(100 + worker_id)


def test_category_filters_area_filter_and_missing_metainfo(on_disk, cfg, monkeypatch, tmp_path):
    from stemseg_amd.data import CocoDataLoader, PascalVOCDataLoader
    _, base, _ = on_disk
    ds = CocoDataLoader(base, os.path.join(base, "coco.json"), True)                   # keep_davis drops category 4
    assert [s.categories for s in ds.samples] == [[1, 2, 1]] * 2 and ds[0]["category_ids"] == [1, 1, 1]
    ds = CocoDataLoader(base, os.path.join(base, "coco.json"), False)                  # keep_ytvis: categories 1 and 2 -> 1 and 21
    assert ds[0]["category_ids"] == [1, 21, 1] and ds[0]["meta_info"]["category_labels"] == ["person", "motorbike", "person"]
    ds = PascalVOCDataLoader(base, os.path.join(base, "pascal_voc.json"), True)        # the 15-pixel instance goes first, then nothing (keep_davis 1, 2)
    assert [s.categories for s in ds.samples] == [[1, 2]] * 2
    ds = PascalVOCDataLoader(base, os.path.join(base, "pascal_voc.json"), True, min_instance_size=15)
    assert [s.categories for s in ds.samples] == [[1, 2, 1]] * 2
    ds = PascalVOCDataLoader(base, os.path.join(base, "pascal_voc.json"), False)
    assert [s.categories for s in ds.samples] == [[1]] * 2 and ds[0]["category_ids"] == [2]
    monkeypatch.setenv("STEMSEG_METAINFO_DIR", str(tmp_path))
    with pytest.raises(FileNotFoundError, match=r"coco\.yaml.*STEMSEG_METAINFO_DIR"):
        CocoDataLoader(base, os.path.join(base, "coco.json"), True)


def test_refusals_without_the_switch_and_those_that_stay_with_it(on_disk, cfg, monkeypatch):
    from stemseg_amd.data import DavisDataLoader, YoutubeVISDataLoader
    from stemseg_amd.training.main import build_parser, main
    from stemseg_amd.training.utils import create_training_dataset
    _, base, vds = on_disk
    for var in ("YOUTUBE_VIS_BASE_DIR", "DAVIS_BASE_DIR", "KITTIMOTS_BASE_DIR", "STEMSEG_JSON_ANNOTATIONS_DIR"):
        monkeypatch.setenv(var, base)
    with pytest.raises(NotImplementedError, match=r"DATA\.DAVIS\.COCO_WEIGHT"):
        create_training_dataset(4, mode="davis")
    with pytest.raises(NotImplementedError, match=r"DATA\.YOUTUBE_VIS\.SINGLE_INSTANCE_DUPLICATION"):
        YoutubeVISDataLoader(base, vds, 3, single_instance_duplication=True)
    with pytest.raises(NotImplementedError, match=r"DATA\.DAVIS\.SINGLE_INSTANCE_DUPLICATION"):
        DavisDataLoader(base, vds, 3, single_instance_duplication=True)
    assert DavisDataLoader(base, vds, 3, single_instance_duplication=True, device_augmentation=True).single_instance_duplication is True
    for loader in (YoutubeVISDataLoader, DavisDataLoader):
        with pytest.raises(NotImplementedError, match="apply_augmentation=True"):
            loader(base, vds, 3, apply_augmentation=True, device_augmentation=True)
    cfg.DATA.KITTI_MOTS.MAPILLARY_WEIGHT, cfg.DATA.KITTI_MOTS.KITTI_MOTS_WEIGHT, cfg.INPUT.NUM_CLASSES = 0.5, 0.5, 3
    with pytest.raises(NotImplementedError, match=r"DATA\.KITTI_MOTS\.MAPILLARY_WEIGHT"):
        create_training_dataset(4, mode="kitti_mots", device_augmentation=True)
    args = build_parser().parse_args(["--model_dir", "x", "--cfg", "davis", "--device_augmentation"])
    with pytest.raises(ValueError, match="--build_data_loader"):
        main(args)


def test_davis_mix_builds_with_the_switch(on_disk, cfg, monkeypatch, tmp_path):
    """The davis preset's mix as shipped -- COCO, Pascal VOC, YouTube-VIS with the duplicator, DAVIS -- builds under the switch."""
    import shutil
    from stemseg_amd.training.utils import create_training_dataset
    gold, base, vds = on_disk
    for name in ("youtube_vis_train.json", "davis_train.json"):
        shutil.copy(vds, str(tmp_path / name))
    for name in ("coco.json", "pascal_voc.json"):
        shutil.copy(os.path.join(base, name), str(tmp_path / name))
    os.makedirs(os.path.join(base, "train"), exist_ok=True)
    for var, value in (("YOUTUBE_VIS_BASE_DIR", str(tmp_path / "ytvis")), ("DAVIS_BASE_DIR", base), ("COCO_TRAIN_IMAGES_DIR", base),
                       ("PASCAL_VOC_IMAGES_DIR", base), ("STEMSEG_JSON_ANNOTATIONS_DIR", str(tmp_path))):
        monkeypatch.setenv(var, value)
    os.makedirs(str(tmp_path / "ytvis"))
    os.symlink(base, str(tmp_path / "ytvis" / "train"))
    cfg.INPUT.NUM_CLASSES = 2
    cfg.TRAINING.MAX_ITERATIONS, cfg.TRAINING.BATCH_SIZE = 8, 1
    d = cfg.DATA.DAVIS
    assert d.COCO_WEIGHT > 0 and d.PASCAL_VOC_WEIGHT > 0 and cfg.DATA.YOUTUBE_VIS.SINGLE_INSTANCE_DUPLICATION is True
    said = []
    random.seed(1)
    dataset = create_training_dataset(8, print_fn=said.append, mode="davis", device_augmentation=True)
    assert said == ["Training datasets: COCO, PascalVOC, YouTubeVIS, Davis"]
    kinds = {dataset[i].get("kind", "video") for i in range(len(dataset))}
    assert kinds == {"image", "video"} and len(dataset) == 8


def test_a_malformed_string_leaves_the_clip_unduplicated(on_disk, cfg):
    """The box walk runs in the worker: a string that is no RLE for the frames must not raise there -- the sample stays as it is, and
    ``device_collate`` names sequence, frame and instance when it decodes the string."""
    from stemseg_amd.data import YoutubeVISDataLoader
    from tests import data_oracle as do
    _, base, vds = on_disk
    ds = YoutubeVISDataLoader(base, vds, 3, category_agnostic=False, single_instance_duplication=True, device_augmentation=True)
    clip = do.pick_clip(ds.sequences, "a", do.CLIP_A)
    lone = clip.instance_ids[0]
    clip.instance_categories = {lone: clip.instance_categories[lone]}
    clip.segmentations = [{i: s for i, s in seg.items() if i == lone} for seg in clip.segmentations]
    ds.samples = [clip]
    good = clip.segmentations[1][lone]
    for bad in (good[:-1], good + "0", "~~~"):
        clip.segmentations[1][lone] = bad
        before = random.getstate()
        recipe = ds[0]
        assert "duplicate" not in recipe and len(recipe["category_ids"]) == 1 and random.getstate() == before
    clip.segmentations[1][lone] = good
    assert any("duplicate" in ds[0] for _ in range(10))
