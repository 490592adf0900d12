"""Host tests of the training data pipeline (stemseg_amd.data, training/utils.py, structures/image_list.py) against
tests/golden/data_pipeline.npz, which tools/make_data_goldens.py recorded from the reference's own loaders, samplers and
``VideoDataset.__getitem__`` + ``collate_fn`` on a synthetic dataset; the C-ABI argument errors of the two data-loader entry points,
without a device call; and the validity of the GPU test's cases on the oracle alone."""
import ctypes as C
import pickle
import random

import numpy as np
import pytest
import torch

from tests import data_oracle as do

LOADERS = ("ytvis", "davis", "mots")


@pytest.fixture(scope="module")
def gold(golden):
    return do.Golden(golden("data_pipeline"))


@pytest.fixture(scope="module")
def on_disk(gold, tmp_path_factory):
    base = str(tmp_path_factory.mktemp("dataset"))
    return base, gold.write(base)


@pytest.fixture()
def cfg(gold):
    from stemseg_amd import config
    config.load_preset("defaults")
    gold.configure(config.cfg)
    yield config.cfg
    config.load_preset("defaults")


def _pair(name, on_disk):
    ds = do.make_loader(name, *on_disk)
    ds.samples = [do.pick_clip(ds.sequences, "a", do.CLIP_A), do.pick_clip(ds.sequences, "b", do.CLIP_B)]
    return ds


# ------------------------------------------------------------------------------------------------ sampling, index for index
@pytest.mark.parametrize("name", LOADERS)
def test_loaders_pick_the_references_clips(gold, on_disk, cfg, name):
    """Seeded alike, ``create_training_subsequences`` picks the reference's clips in its order; the sequences it picks from -- after the
    zero-instance filter, or for KITTI-MOTS the gap split with its '<id>_k' names -- are the reference's too."""
    random.seed(gold.config["SEED"])
    ds = do.make_loader(name, *on_disk)
    assert do.describe(ds.sequences) == gold.record[name + "_sequences"]
    assert do.describe(ds.samples) == gold.record[name + "_samples"]
    assert len(ds) == 7


def test_mots_split_cuts_at_the_gap(gold, on_disk, cfg):
    ds = do.make_loader("mots", *on_disk)
    ids = [s.id for s in ds.sequences]
    assert "a_1" in ids and "a_2" in ids and "b_1" in ids and "b_2" not in ids
    a1 = ds.sequences[ids.index("a_1")]
    assert a1.image_paths == ["a/%05d.jpg" % t for t in range(8)]


@pytest.mark.parametrize("key", ("concat_repeat", "concat_sparse"))
def test_concat_dataset_id_mapping(gold, on_disk, cfg, key):
    from stemseg_amd.data import ConcatDataset
    rec = gold.record[key]
    random.seed(gold.config["SEED"])
    parts = [do.make_loader("ytvis", *on_disk), do.make_loader("davis", *on_disk)]
    mix = ConcatDataset(parts, rec["total"], rec["weights"])
    assert [list(p) for p in mix.id_mapping] == rec["id_mapping"] and mix.samples_per_dataset == rec["samples_per_dataset"]
    assert len(mix) == rec["total"] and mix[0]["meta_info"]["seq_name"] == parts[rec["id_mapping"][0][0]].samples[rec["id_mapping"][0][1]].id


def test_distributed_sampler_indices(gold):
    from stemseg_amd.data import DistributedSampler
    assert len(gold.record["distributed_sampler"]) == 18
    for rec in gold.record["distributed_sampler"]:
        s = DistributedSampler(list(range(10)), rec["world"], rec["rank"], rec["shuffle"])
        s.set_epoch(rec["epoch"])
        assert list(s) == rec["indices"] and len(s) == len(rec["indices"]), rec


def test_iteration_based_batch_sampler(gold):
    from torch.utils.data.sampler import BatchSampler, SequentialSampler
    from stemseg_amd.data import DistributedSampler, IterationBasedBatchSampler
    rec = gold.record["iteration_sampler"]
    span = list(range(10))
    plain = IterationBasedBatchSampler(BatchSampler(SequentialSampler(span), 3, False), 9, 4)
    assert [list(b) for b in plain] == rec["plain"] and len(plain) == rec["plain_len"]
    shard = IterationBasedBatchSampler(BatchSampler(DistributedSampler(span, 2, 1, True), 2, False), 9, 3)
    assert [list(b) for b in shard] == rec["sharded"]


# ------------------------------------------------------------------------------------------------ recipes
def _plain(x):
    if isinstance(x, dict):
        return all(isinstance(k, str) and _plain(v) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return all(_plain(v) for v in x)
    return x is None or isinstance(x, (bytes, str, int, np.ndarray)) and not isinstance(x, bool)


def test_recipes_are_plain_picklable_host_data(gold, on_disk, cfg):
    ds = _pair("mots", on_disk)
    for r in (ds[0], ds[1]):
        assert _plain(r), r.keys()
        assert pickle.loads(pickle.dumps(r)) == r
        assert sorted(r) == ["category_ids", "frames", "ignore", "meta_info", "n_instances", "rle", "size"]
        assert r["frames"] == [gold.files[p] for p in (do.CLIP_A if r["meta_info"]["seq_name"].startswith("a") else do.CLIP_B)]


def test_datasets_do_not_load_the_hip_binding():
    """What a worker process imports to unpickle a dataset and run ``__getitem__`` never pulls in ``stemseg_amd.hip``."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path[:0] = [%r, %r]; import stemseg_amd.data; assert 'stemseg_amd.hip' not in sys.modules" % (
        root, os.path.join(root, "stem-seg_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_worker_processes_yield_the_same_recipes(gold, on_disk, cfg):
    from torch.utils.data import DataLoader
    random.seed(3)
    ds = do.make_loader("davis", *on_disk)
    batches = [list(DataLoader(ds, collate_fn=list, batch_size=2, shuffle=False, num_workers=k)) for k in (0, 2)]
    assert len(batches[0]) == 4 and batches[0] == batches[1]


def test_training_data_loader_wraps_the_collate_in_the_consuming_process(gold, on_disk, cfg):
    from stemseg_amd.training.utils import create_training_data_loader
    ds = _pair("ytvis", on_disk)
    seen = []
    loader = create_training_data_loader(ds, 2, False, collate_fn=lambda recipes: seen.append(recipes) or len(recipes), num_workers=0)
    assert list(loader) == [2] and len(loader) == 1 and seen[0] == [ds[0], ds[1]]
    resumed = create_training_data_loader(ds, 1, False, collate_fn=lambda recipes: recipes[0]["meta_info"]["seq_name"], elapsed_iters=1)
    assert list(resumed) == [ds[0]["meta_info"]["seq_name"]]          # (2 iterations in all, one done: one batch is left, from the start)


# ------------------------------------------------------------------------------------------------ the oracle against the reference's batch
@pytest.mark.parametrize("name", LOADERS)
def test_recipes_through_the_oracle_give_the_references_batch(gold, on_disk, cfg, name):
    """The recipes of the two clips, put together by the CPU oracle, are the batch the reference recorded: masks, ignore masks (one of the
    three rules per loader), category ids, sizes -- exactly -- and the images to float rounding."""
    ds = _pair(name, on_disk)
    rec = gold.record[name + "_batch"]
    recipes = [ds[0], ds[1]]
    assert [s.instance_ids for s in ds.samples] == rec["instance_ids"]
    assert [r["meta_info"]["seq_name"] for r in recipes] == rec["seq_names"]
    out = do.collate(recipes, cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD)
    assert [list(s) for s in out["image_sizes"]] == rec["image_sizes"] and list(out["pad"]) == rec["max_size"]
    assert [[r["size"][0], r["size"][1]] for r in recipes] == rec["original_image_sizes"]
    for n, t in enumerate(out["targets"]):
        assert t["category_ids"] == rec["category_ids"][n]
        assert np.array_equal(t["masks"], gold.npz["%s_masks_%d" % (name, n)])
        assert np.array_equal(t["ignore_masks"], gold.npz["%s_ignore_%d" % (name, n)])
    assert np.array_equal(out["images"], gold.npz["batch_images"])
    ignores = [gold.npz["%s_ignore_%d" % (name, n)] for n in (0, 1)]
    if name == "ytvis":
        assert not ignores[0].any() and not ignores[1].any()
    elif name == "davis":
        assert ignores[0].any() and ignores[1].any()
    else:
        assert ignores[0].any() and not ignores[1].any() and len(rec["category_ids"][0]) == 2          # (category 3 left the targets)


def test_image_list_against_the_golden(gold):
    from stemseg_amd.structures import ImageList
    rec = gold.record["mots_batch"]
    batch = torch.from_numpy(gold.npz["batch_images"])
    clips = [batch[n, :, :, :h, :w] for n, (h, w) in enumerate(rec["image_sizes"])]
    il = ImageList.from_image_sequence_list(clips, [tuple(s) for s in rec["original_image_sizes"]])
    assert torch.equal(il.tensors, batch) and [list(s) for s in il.image_sizes] == rec["image_sizes"]
    assert list(il.max_size) == rec["max_size"] and len(il) == il.num_seqs == 2 and il.num_frames == 4
    assert torch.equal(il[1], batch[1]) and il.to(torch.float64).tensors.dtype == torch.float64
    assert il.to(torch.float64).original_image_sizes == il.original_image_sizes
    assert ImageList.padded_size([(48, 69), (54, 48)]) == (64, 96)


def test_resize_params_and_padding():
    from stemseg_amd.data.common import compute_padding, compute_resize_params
    assert compute_resize_params(np.zeros((37, 53, 3)), 48, 80)[:2] == (69, 48)
    assert compute_resize_params((45, 40), 48, 80)[:2] == (48, 54)
    assert compute_resize_params((375, 1242), 736, 1792)[:2] == (1792, 541)          # the long side decides
    assert compute_padding(69, 48) == (27, 16) and compute_padding(64, 96) == (0, 0)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_their_keys(gold, on_disk, cfg, monkeypatch):
    from stemseg_amd import config
    from stemseg_amd.training.utils import create_training_dataset
    base, vds = on_disk
    for var in ("YOUTUBE_VIS_BASE_DIR", "DAVIS_BASE_DIR", "KITTIMOTS_BASE_DIR", "STEMSEG_JSON_ANNOTATIONS_DIR"):
        monkeypatch.setenv(var, base)
    with pytest.raises(ValueError, match="Invalid training mode"):
        create_training_dataset(4)
    with pytest.raises(NotImplementedError, match=r"DATA\.DAVIS\.COCO_WEIGHT"):
        create_training_dataset(4, mode="davis")
    cfg.DATA.DAVIS.COCO_WEIGHT = 0.0
    with pytest.raises(NotImplementedError, match=r"DATA\.DAVIS\.PASCAL_VOC_WEIGHT"):
        create_training_dataset(4, mode="davis")
    cfg.DATA.KITTI_MOTS.MAPILLARY_WEIGHT, cfg.DATA.KITTI_MOTS.KITTI_MOTS_WEIGHT, cfg.INPUT.NUM_CLASSES = 0.5, 0.5, 3
    with pytest.raises(NotImplementedError, match=r"DATA\.KITTI_MOTS\.MAPILLARY_WEIGHT"):
        create_training_dataset(4, mode="kitti_mots")
    cfg.INPUT.NUM_CLASSES = 41
    cfg.DATA.YOUTUBE_VIS.COCO_WEIGHT, cfg.DATA.YOUTUBE_VIS.PASCAL_VOC_WEIGHT, cfg.DATA.YOUTUBE_VIS.YOUTUBE_VIS_WEIGHT = 0.0, 0.0, 1.0
    assert cfg.DATA.YOUTUBE_VIS.SINGLE_INSTANCE_DUPLICATION is True
    with pytest.raises(NotImplementedError, match=r"DATA\.YOUTUBE_VIS\.SINGLE_INSTANCE_DUPLICATION"):
        create_training_dataset(4, mode="youtube_vis")
    with pytest.raises(NotImplementedError, match="apply_augmentation=True"):
        do.make_loader("mots", base, vds).__class__(base, vds, 3, apply_augmentation=True)
    with pytest.raises(NotImplementedError, match=r"DATA\.DAVIS\.SINGLE_INSTANCE_DUPLICATION"):
        from stemseg_amd.data import DavisDataLoader
        DavisDataLoader(base, vds, 3, single_instance_duplication=True)
    assert config.PRESET_TRAINING_MODES["kittimots"] == "kitti_mots"


def test_create_training_dataset_skips_zero_weights_and_mixes_the_rest(gold, on_disk, cfg, monkeypatch, tmp_path):
    """kitti_mots with its default weights (Mapillary 0, KITTI-MOTS 1) builds from the path variables; youtube_vis with the duplicator
    off and the image weights at 0 does too."""
    from stemseg_amd.training.utils import create_training_dataset
    base, _ = on_disk
    for name in ("kittimots_train.json", "youtube_vis_train.json"):
        gold.write(str(tmp_path), name)
    (tmp_path / "train").symlink_to(base, target_is_directory=True)
    monkeypatch.setenv("STEMSEG_JSON_ANNOTATIONS_DIR", str(tmp_path))
    monkeypatch.setenv("KITTIMOTS_BASE_DIR", base)
    monkeypatch.setenv("YOUTUBE_VIS_BASE_DIR", str(tmp_path))
    said = []
    cfg.INPUT.NUM_CLASSES = 3
    mix = create_training_dataset(6, print_fn=said.append, mode="kitti_mots")
    assert len(mix) == 6 and said == ["Training datasets: KITTI-MOTS"] and mix[5]["ignore"] in (None, ("instance", 0), ("instance", 1), ("instance", 2))
    cfg.INPUT.NUM_CLASSES = 41
    y = cfg.DATA.YOUTUBE_VIS
    y.COCO_WEIGHT, y.PASCAL_VOC_WEIGHT, y.YOUTUBE_VIS_WEIGHT, y.SINGLE_INSTANCE_DUPLICATION = 0.0, 0.0, 1.0, False
    mix = create_training_dataset(5, print_fn=said.append, mode="youtube_vis")
    assert len(mix) == 5 and mix[0]["ignore"] is None and said[-1] == "Training datasets: YouTubeVIS"


# ------------------------------------------------------------------------------------------------ the C ABI, no device call
@pytest.fixture(scope="module")
def raw():
    from stemseg_amd import hip
    return hip.lib(), hip


def _last(lib):
    return lib.stemseg_hip_last_error().decode()


def test_rle_decode_argument_errors(raw):
    lib, hip = raw
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any HIP call
    offs = lambda *v: np.asarray(v, np.int64).ctypes.data_as(C.c_void_p)
    idx = lambda *v: np.asarray(v, np.int32).ctypes.data_as(C.c_void_p)
    big = 1 << 30

    def call(chars=fake, n=4, offsets=None, planes_idx=None, M=2, P=3, H=7, W=5, ws=fake, ws_bytes=big, planes=fake, status=fake,
             offsets_dev=fake, planes_idx_dev=fake):
        o = offs(0, 2, 4) if offsets is None else offsets
        p = idx(0, 1) if planes_idx is None else planes_idx
        return lib.stemseg_hip_rle_decode(chars, n, o, p, offsets_dev, planes_idx_dev, M, P, H, W, ws, ws_bytes, planes, status, None)
    for kw, word in ((dict(chars=None), "null"), (dict(planes=None), "null"), (dict(ws=None), "null"), (dict(status=None), "null"),
                     (dict(offsets_dev=None), "null"), (dict(planes_idx_dev=None), "null"), (dict(offsets_dev=C.c_void_p(0x1004)), "aligned"),
                     (dict(planes_idx_dev=C.c_void_p(0x1002)), "aligned"),
                     (dict(H=65536, W=32768), "2^31"), (dict(ws_bytes=16), "workspace"), (dict(planes_idx=idx(0, 3)), "plane 3"),
                     (dict(planes_idx=idx(-1, 0)), "plane -1"), (dict(planes_idx=idx(1, 1)), "two strings"), (dict(P=1), "planes"),
                     (dict(offsets=offs(0, 5, 4)), "offsets"), (dict(offsets=offs(1, 2, 4)), "offsets"), (dict(offsets=offs(0, 2, 3)), "offsets"),
                     (dict(M=-1), "bad dims"), (dict(n=-1), "n_chars"), (dict(n=big, offsets=offs(0, 2, big)), "n_chars")):
        assert call(**kw) == -1, kw
        assert word in _last(lib), (kw, _last(lib))
    assert lib.stemseg_hip_rle_decode_workspace_bytes(4, 2, 3) > 0
    assert lib.stemseg_hip_rle_decode_workspace_bytes(-1, 2, 3) == 0 and lib.stemseg_hip_rle_decode_workspace_bytes(4, 2, 0) == 0
    assert lib.stemseg_hip_rle_decode_workspace_bytes(1000, 2, 3) < lib.stemseg_hip_rle_decode_workspace_bytes(2000, 2, 3)
    for n in ("stemseg_hip_rle_decode", "stemseg_hip_rle_decode_workspace_bytes", "stemseg_hip_resize_masks"):
        assert hasattr(lib, n) and n in hip.SIGNATURES


def test_rle_pack_keeps_foreign_characters_outside_the_alphabet(raw):
    """str and bytes alike; a character beyond one byte becomes 0xFF and a latin-1 one keeps its code, both outside 48..111, so the decoder
    reports a bad character and not whatever a replacement inside the alphabet would add up to."""
    _, hip = raw
    chars, offsets, planes = hip.rle_pack(["0a", b"7", "", "1€é2"], [3, 0, 2, 1])
    assert chars.tolist() == [48, 97, 55, 49, 0xFF, 0xE9, 50] and offsets.tolist() == [0, 2, 3, 3, 7]
    assert planes.dtype == np.int32 and planes.tolist() == [3, 0, 2, 1] and offsets.dtype == np.int64 and chars.dtype == np.uint8


def test_resize_masks_argument_errors(raw):
    lib, hip = raw
    fake = C.c_void_p(0x1000)
    rng = lambda *v: np.asarray(v, np.int32).ctypes.data_as(C.c_void_p)

    def call(planes=fake, P=4, H0=8, W0=8, nh=4, nw=4, ph=32, pw=32, ranges=None, R=0, out=fake):
        return lib.stemseg_hip_resize_masks(planes, P, H0, W0, nh, nw, ph, pw, ranges, R, 0, out, None)
    for kw, word in ((dict(planes=None), "null"), (dict(out=None), "null"), (dict(P=0), "bad dims"), (dict(ph=3), "bad dims"), (dict(nw=0), "bad dims"),
                     (dict(H0=65536, W0=32768), "2^31"), (dict(R=1), "union ranges"), (dict(R=65, ranges=rng(0, 1, 1)), "union ranges"),
                     (dict(R=1, ranges=rng(0, 5, 1)), "leaves"), (dict(R=1, ranges=rng(2, 2, 2)), "leaves"), (dict(R=1, ranges=rng(0, 0, 1)), "leaves"),
                     (dict(R=1, ranges=rng(-1, 1, 1)), "leaves"), (dict(R=1, ranges=rng(0, 2, 0)), "leaves")):
        assert call(**kw) == -1, kw
        assert word in _last(lib), (kw, _last(lib))
    assert hip.MAX_UNION_RANGES == 64 and (hip.RLE_EMPTY, hip.RLE_BAD_CHAR, hip.RLE_OPEN_GROUP, hip.RLE_BAD_COUNT, hip.RLE_BAD_SUM) == (1, 2, 4, 8, 16)
    header = open(__import__("os").path.join(__import__("os").path.dirname(do.__file__), "..", "include", "stemseg_hip.h")).read()
    for name, value in (("STEMSEG_RLE_BAD_COUNT", 8), ("STEMSEG_RLE_BAD_SUM", 16), ("STEMSEG_MAX_UNION_RANGES", 64)):
        assert "#define %s" % name in header and str(value) in header.split("#define %s" % name)[1].split("\n")[0]


# ------------------------------------------------------------------------------------------------ validity of the GPU test's cases
def test_gpu_cases_are_valid_on_the_oracle():
    """Every resize case of the GPU test: the share of pixels within 1e-6 of 0.5 without being exactly 0.5 is below 1e-3 (so the tie rule
    can excuse almost nothing); the malformed strings carry the status they are listed with; the well-formed ones decode."""
    for (h, w), new_hw, pads in do.RESIZE_SHAPES:
        hard, soft = do.resize_masks(do.resize_planes(h, w), new_hw, pads[0], [(0, 2, 1), (1, 3, 2)])
        assert do.near_tie_share(soft) < 1e-3, ((h, w), do.near_tie_share(soft))
        assert hard[:, :new_hw[0], :new_hw[1]].any() and not hard[:, new_hw[0]:].any()
    assert (do.resize_masks(do.resize_planes(96, 128), (48, 64), (64, 64))[1] == 0.5).any()          # exact ties exist at 2x
    for name, s, status in do.malformed_cases():
        assert do.string_status(s, 7, 5) == status != 0, name
    assert sorted(set(c[2] for c in do.malformed_cases())) == [1, 2, 4, 8, 16]
    for name, h, w, masks in do.rle_small_cases():
        planes, status = do.decode_strings([do.mask_string(m) for m in masks], range(len(masks)), len(masks), h, w)
        assert not status.any() and np.array_equal(planes, np.stack(masks)), name
    run_counts = set(len(do.wo.encode(m)) for _, _, _, masks in do.rle_small_cases() for m in masks)
    assert {1, 2, 3, 4, 5} <= run_counts
    strings, plane_of_string, P, h, w = do.unequal_batch()
    assert len(strings) == 300 and len(set(plane_of_string)) == 300 and max(plane_of_string) < P


def test_end_to_end_case_is_valid_on_the_oracle(gold, on_disk, cfg):
    for name in LOADERS:
        ds = _pair(name, on_disk)
        out = do.collate([ds[0], ds[1]], cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD, with_images=False)
        for t in out["targets"]:
            assert do.near_tie_share(t["soft_masks"]) < 1e-3 and do.near_tie_share(t["soft_ignore"]) < 1e-3
