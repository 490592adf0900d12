"""CPU tests of the Mapillary dataset's host half (stemseg_amd/data/mapillary_data_loader.py, the ``device_mapillary`` switch, the
``kittimots_1`` preset, the argument checks of ``rle_decode_union``) and of the validity of the cases tests/test_gpu_mapillary.py runs,
on tests/mapillary_oracle.py alone."""
import ctypes as C
import os
import pickle
import random

import numpy as np
import pytest

from tests import augment_oracle as ao
from tests import data_oracle as do
from tests import mapillary_oracle as mo

METAINFO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metainfo")


@pytest.fixture(scope="module")
def on_disk(golden, tmp_path_factory):
    gold = do.Golden(golden("data_pipeline"))
    base = str(tmp_path_factory.mktemp("mapillary"))
    vds = gold.write(base)
    return gold, base, vds, mo.write_dataset(base)


@pytest.fixture()
def cfg(on_disk, monkeypatch):
    from stemseg_amd import config
    config.load_preset("defaults")
    on_disk[0].configure(config.cfg)
    monkeypatch.setenv("STEMSEG_METAINFO_DIR", METAINFO)
    yield config.cfg
    config.load_preset("defaults")


# ------------------------------------------------------------------------------------------------ the selection rule
SELECT_CASES = {
    # name: (areas, categories, max_nbr_instances, expected targets, expected ignored)
    "area ties keep their order": ([50, 70, 50, 70, 50], [1, 2, 2, 1, 1], 3, [1, 3, 0], {2, 4}),
    "an ignore category inside the first ones": ([90, 80, 70, 60], [1, 3, 2, 1], 3, [0, 2], {1, 3}),
    "a kept category beyond them": ([10, 40, 30, 20], [1, 1, 2, 2], 2, [1, 2], {3, 0}),
    "no kept category among them": ([10, 40, 30, 20], [1, 4, 3, 2], 2, [], {0, 1, 2, 3}),
    "fewer instances than the limit": ([5, 6], [2, 1], 30, [1, 0], set()),
    "a tie across the limit": ([7, 7, 7], [1, 2, 1], 2, [0, 1], {2}),
}


@pytest.mark.parametrize("name", sorted(SELECT_CASES))
def test_selection_rule_against_the_oracle(name):
    from stemseg_amd.data.mapillary_data_loader import select_instances
    areas, cats, limit, want_targets, want_ignored = SELECT_CASES[name]
    assert mo.select(areas, cats, limit) == (want_targets, want_ignored), "the oracle itself"
    targets, ignored = select_instances(areas, cats, list(mo.IGNORE), limit)
    assert targets == want_targets and set(ignored) == want_ignored and len(ignored) == len(want_ignored)
    rs = np.random.RandomState(len(name))
    for _ in range(20):          # and on random lists with many ties
        n = rs.randint(1, 40)
        areas, cats, limit = rs.randint(30, 36, n).tolist(), rs.randint(1, 5, n).tolist(), int(rs.randint(1, 35))
        targets, ignored = select_instances(areas, cats, list(mo.IGNORE), limit)
        assert (targets, set(ignored)) == mo.select(areas, cats, limit) and len(targets) + len(ignored) == n


# ------------------------------------------------------------------------------------------------ the dataset and its recipes
def _plain(x):
    if isinstance(x, dict):
        return all(isinstance(k, str) and _plain(v) for k, v in x.items())
    if isinstance(x, (list, tuple)):
        return all(_plain(v) for v in x)
    return x is None or isinstance(x, (bytes, str, int, float, bool))


def _seed_worker(worker_id):
    random.seed(100 + worker_id)


def test_filters_and_missing_metainfo(on_disk, cfg, monkeypatch, tmp_path):
    from stemseg_amd.data import MapillaryDataLoader
    _, base, _, ids = on_disk
    entries = mo.dataset_entries()
    for min_size, limit in ((30, 30), (10, 30), (30, 2)):
        ds = MapillaryDataLoader(base, ids, min_instance_size=min_size, max_nbr_instances=limit)
        expect = [(e, mo.expected_sample(e, min_size, limit)) for e in entries]
        expect = [(e, x) for e, x in expect if x is not None]
        assert len(ds) == len(expect) == (2 if min_size == 30 else 3), "samples without a kept category (after the area filter) are dropped"
        for sample, (entry, (kept, targets, ignored)) in zip(ds.samples, expect):
            assert sample.categories == [entry[2][i] for i in kept] and set(sample.categories) <= set(mo.KEEP + mo.IGNORE)
            assert sample.segmentations == [do.mask_string(entry[1][i]) for i in kept]
            random.seed(0)
            r = ds[ds.samples.index(sample)]
            assert r["rle"][:len(targets)] == [sample.segmentations[i] for i in targets]
            assert sorted(r["rle"][len(targets):]) == sorted(sample.segmentations[i] for i in ignored)
            assert r["category_ids"] == [sample.categories[i] for i in targets], "id_kittimots of categories 1 and 2 is 1 and 2"
            assert r["meta_info"]["category_labels"] == [{1: "car", 2: "person"}[sample.categories[i]] for i in targets]
    ds = MapillaryDataLoader(base, ids)
    assert ds.max_nbr_instances == 30 and [len(s.segmentations) for s in ds.samples] == [35, 5]
    assert 41 > 35 > ds.max_nbr_instances, "the 15-pixel instance and category 5 are gone; more instances than max_nbr_instances remain"
    monkeypatch.setenv("STEMSEG_METAINFO_DIR", str(tmp_path))
    with pytest.raises(FileNotFoundError, match=r"mapillary\.yaml.*STEMSEG_METAINFO_DIR"):
        MapillaryDataLoader(base, ids)


def test_recipes_are_plain_seeded_and_the_same_from_two_workers(on_disk, cfg):
    from torch.utils.data import DataLoader
    from stemseg_amd.data import MapillaryDataLoader
    gold, base, _, ids = on_disk
    ds = MapillaryDataLoader(base, ids)
    random.seed(3)
    first = [ds[0], ds[1]]
    after = random.random()
    for r in first:
        assert _plain(r) and pickle.loads(pickle.dumps(r)) == r and r["kind"] == "image"
        assert len(r["warps"]) == cfg.INPUT.NUM_FRAMES - 1 and sorted(r["perm"]) == list(range(cfg.INPUT.NUM_FRAMES))
        assert all(w["blur"] is None for w in r["warps"]), "motion_blur_prob is 0"
        assert r["frames"] == [gold.files["a/00000.jpg" if r["size"] == (53, 37) else "b/00001.png"]]
        n = r["n_instances"]
        assert len(r["rle_planes"]) == len(r["rle"]) and all(b >= a for a, b in zip(r["rle_planes"], r["rle_planes"][1:]))
        assert r["rle_planes"][:n] == list(range(n)) and set(r["rle_planes"][n:]) == {n} and r["has_ignore"] is True
        assert len(r["category_ids"]) == n == len(r["meta_info"]["category_labels"])
    assert first[0]["n_instances"] == 16 and len(first[0]["rle"]) == 35 and first[1]["n_instances"] == 3 and len(first[1]["rle"]) == 5
    # the reference's order of calls: random() for the flip, one getrandbits(64) per warp, the shuffle of the permutation
    random.seed(3)
    for r in first:
        assert (random.random() < 0.5) == r["flip"]
        seeds = [random.getrandbits(64) for _ in range(cfg.INPUT.NUM_FRAMES - 1)]
        assert [w["hinv"] for w in r["warps"]] == [ds.augmenter.sample(r["size"][0], r["size"][1], random.Random(s))["hinv"] for s in seeds]
        perm = list(range(cfg.INPUT.NUM_FRAMES))
        random.shuffle(perm)
        assert perm == r["perm"]
    assert random.random() == after
    a = ds.augmenter
    for seed in range(200):
        p = a.sample(640, 480, random.Random(seed))["params"]
        assert -10 <= p["rotation"] <= 10 and all(-0.1 <= t <= 0.1 for t in p["translate"])
    loader = DataLoader(ds, batch_size=1, collate_fn=list, num_workers=2, worker_init_fn=_seed_worker, multiprocessing_context="spawn")
    for i, r in enumerate(b[0] for b in loader):          # sample i comes from worker i % 2, as its first sample
        random.seed(100 + i % 2)
        assert ds[i] == r
    none = MapillaryDataLoader(base, ids, max_nbr_instances=1)[1]
    assert none["n_instances"] == 0 and none["category_ids"] == [] and none["rle_planes"] == [0] * 5 and none["has_ignore"] is True


# ------------------------------------------------------------------------------------------------ the switch, the preset, the command line
def _paths(monkeypatch, gold, base, ids, tmp_path):
    import shutil
    shutil.copy(ids, str(tmp_path / "mapillary.json"))
    gold.write(str(tmp_path), "kittimots_train.json")
    for var, value in (("MAPILLARY_IMAGES_DIR", base), ("KITTIMOTS_BASE_DIR", base), ("STEMSEG_JSON_ANNOTATIONS_DIR", str(tmp_path))):
        monkeypatch.setenv(var, value)


def test_kittimots_1_mix_builds_with_the_switch_and_is_refused_without(on_disk, monkeypatch, tmp_path):
    from stemseg_amd import config
    from stemseg_amd.training.utils import create_training_dataset
    from stemseg_amd.utils.paths import MapillaryPaths
    gold, base, _, ids = on_disk
    _paths(monkeypatch, gold, base, ids, tmp_path)
    monkeypatch.setenv("STEMSEG_METAINFO_DIR", METAINFO)
    assert MapillaryPaths.images_dir() == base and MapillaryPaths.ids_file() == str(tmp_path / "mapillary.json")
    try:
        c = config.load_preset("kittimots_1")
        gold.configure(c)
        c.INPUT.NUM_CLASSES = 3
        said = []
        mix = create_training_dataset(6, print_fn=said.append, mode=config.PRESET_TRAINING_MODES["kittimots_1"], device_mapillary=True)
        assert said == ["Training datasets: Mapillary"] and len(mix) == 6
        assert all(mix[i]["kind"] == "image" and "rle_planes" in mix[i] for i in range(6))
        for kwargs in ({}, {"device_augmentation": True}):
            with pytest.raises(NotImplementedError, match=r"DATA\.KITTI_MOTS\.MAPILLARY_WEIGHT.*device_mapillary=True \(--device_mapillary\)"):
                create_training_dataset(6, mode="kitti_mots", **kwargs)
        c.DATA.KITTI_MOTS.MAPILLARY_WEIGHT, c.DATA.KITTI_MOTS.KITTI_MOTS_WEIGHT = 0.5, 0.5
        mix = create_training_dataset(6, print_fn=said.append, mode="kitti_mots", device_mapillary=True)
        assert said[-1] == "Training datasets: Mapillary, KITTI-MOTS" and mix.samples_per_dataset == [3, 3]
        assert {mix[i].get("kind", "video") for i in range(6)} == {"image", "video"}
        c.DATA.KITTI_MOTS.MAPILLARY_WEIGHT, c.DATA.KITTI_MOTS.KITTI_MOTS_WEIGHT = 0.0, 1.0
        create_training_dataset(6, print_fn=said.append, mode="kitti_mots", device_mapillary=True)
        assert said[-1] == "Training datasets: KITTI-MOTS"
    finally:
        config.load_preset("defaults")


def test_kittimots_1_preset():
    from stemseg_amd import config
    one, two = config.make_cfg("kittimots_1"), config.make_cfg("kittimots")
    assert config.PRESET_TRAINING_MODES["kittimots_1"] == "kitti_mots"
    assert (one.INPUT.MIN_DIM, one.INPUT.MAX_DIM, one.INPUT.NUM_FRAMES, one.INPUT.NUM_CLASSES) == (736, 1248, 8, 3) and two.INPUT.MAX_DIM == 1792
    assert (one.DATA.KITTI_MOTS.MAPILLARY_WEIGHT, one.DATA.KITTI_MOTS.KITTI_MOTS_WEIGHT) == (1.0, 0.0)
    assert (two.DATA.KITTI_MOTS.MAPILLARY_WEIGHT, two.DATA.KITTI_MOTS.KITTI_MOTS_WEIGHT) == (0.0, 1.0)
    t = one.TRAINING
    assert (t.INITIAL_LR, t.LR_DECAY_TYPE, t.LR_EXP_DECAY_FACTOR, t.LR_EXP_DECAY_START, t.LR_EXP_DECAY_STEPS, t.MAX_ITERATIONS) == \
        (0.001, "exponential", 0.1, 60000, 20000, 80000)
    assert two.TRAINING.LR_DECAY_TYPE == "step" and two.TRAINING.MAX_ITERATIONS == 120000, "the kittimots preset keeps the defaults"
    one.INPUT.MAX_DIM, one.DATA, one.TRAINING = two.INPUT.MAX_DIM, two.DATA, two.TRAINING

    def flat(ns):
        return {k: flat(v) if hasattr(v, "__dict__") else v for k, v in vars(ns).items()}
    assert flat(one) == flat(two), "everything else is the kittimots preset"


def test_device_mapillary_needs_build_data_loader():
    from stemseg_amd.training.main import build_parser, main
    args = build_parser().parse_args(["--model_dir", "x", "--cfg", "kittimots_1", "--device_mapillary"])
    assert args.device_mapillary is True
    with pytest.raises(ValueError, match=r"--device_mapillary.*--build_data_loader"):
        main(args)
    assert build_parser().parse_args(["--model_dir", "x", "--cfg", "kittimots"]).device_mapillary is False


# ------------------------------------------------------------------------------------------------ the C ABI, no device call
def test_rle_decode_union_argument_errors_and_exports():
    from stemseg_amd import hip
    lib = hip.lib()
    for n in ("stemseg_hip_rle_decode_union", "stemseg_hip_rle_decode_union_workspace_bytes"):
        assert hasattr(lib, n) and n in hip.SIGNATURES
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any HIP call
    offs = lambda *v: np.asarray(v, np.int64).ctypes.data_as(C.c_void_p)
    idx = lambda *v: np.asarray(v, np.int32).ctypes.data_as(C.c_void_p)
    big = 1 << 30

    def call(chars=fake, n=6, offsets=None, planes_idx=None, M=3, P=2, H=7, W=5, ws=fake, ws_bytes=big, planes=fake, status=fake,
             offsets_dev=fake, planes_idx_dev=fake):
        o = offs(0, 2, 4, 6) if offsets is None else offsets
        p = idx(0, 1, 1) if planes_idx is None else planes_idx
        return lib.stemseg_hip_rle_decode_union(chars, n, o, p, offsets_dev, planes_idx_dev, M, P, H, W, ws, ws_bytes, planes, status, None)
    for kw, word in ((dict(planes_idx=idx(1, 0, 1)), "decrease at string 1"), (dict(planes_idx=idx(0, 1, 0)), "decrease at string 2"),
                     (dict(chars=None), "null"), (dict(planes=None), "null"), (dict(ws=None), "null"), (dict(status=None), "null"),
                     (dict(offsets_dev=None), "null"), (dict(planes_idx_dev=None), "null"), (dict(offsets_dev=C.c_void_p(0x1004)), "aligned"),
                     (dict(planes_idx_dev=C.c_void_p(0x1002)), "aligned"), (dict(H=65536, W=32768), "2^31"), (dict(ws_bytes=16), "workspace"),
                     (dict(planes_idx=idx(0, 1, 2)), "plane 2"), (dict(planes_idx=idx(-1, 0, 0)), "plane -1"), (dict(P=0), "bad dims"),
                     (dict(offsets=offs(0, 5, 4, 6)), "offsets"), (dict(offsets=offs(1, 2, 4, 6)), "offsets"), (dict(offsets=offs(0, 2, 4, 5)), "offsets"),
                     (dict(M=-1), "bad dims"), (dict(n=-1), "n_chars"), (dict(n=big, offsets=offs(0, 2, 4, big)), "n_chars")):
        assert call(**kw) == -1, kw
        assert word in lib.stemseg_hip_last_error().decode() and "rle_decode_union" in lib.stemseg_hip_last_error().decode(), kw
    wsb = lib.stemseg_hip_rle_decode_union_workspace_bytes
    assert wsb(6, 3, 2) > 0 and wsb(-1, 3, 2) == 0 and wsb(6, 3, 0) == 0 and wsb(1000, 3, 2) < wsb(2000, 3, 2) and wsb(6, 3, 2) < wsb(6, 3000, 2)
    # the binding refuses a decreasing table before it asks for a device
    with pytest.raises(ValueError, match="decrease at string 2"):
        hip.rle_decode_union(["0", "0", "0"], [0, 1, 0], 2, 1, 1)
    # ... and rle_decode still refuses what the union form takes
    assert lib.stemseg_hip_rle_decode(fake, 6, offs(0, 2, 4, 6), idx(0, 1, 1), fake, fake, 3, 3, 7, 5, fake, big, fake, fake, None) == -1
    assert "two strings" in lib.stemseg_hip_last_error().decode()


# ------------------------------------------------------------------------------------------------ the validity of the GPU cases
def test_union_cases_hold_what_they_are_meant_to():
    for h, w in mo.UNION_SHAPES:
        strings, planes, P = mo.union_case(h, w)
        assert all(b >= a for a, b in zip(planes, planes[1:])) and P == 9
        per_plane = [planes.count(q) for q in range(P)]
        assert per_plane[0] == per_plane[4] == per_plane[8] == 130 and per_plane[1] == 0 and per_plane[2] == 1 and per_plane[3] == 2
        ref, status = mo.decode_union(strings, planes, P, h, w)
        singles = [do.decode_strings([s], [0], 1, h, w)[0][0] for s, q in zip(strings, planes) if q == 0]
        assert 0 < ref[0].mean() < 1 and not ref[1].any() and ref[6].all()
        if h * w > 64:
            assert (np.sum(singles, 0) > 1).any(), "overlapping strings in plane 0"
        a, b = [do.decode_strings([s], [0], 1, h, w)[0][0] for s, q in zip(strings, planes) if q == 3]
        assert a.any() and b.any() and not (a & b).any(), "disjoint strings in plane 3"
        in4 = [s for s, q in zip(strings, planes) if q == 4]
        assert do.mask_string(np.zeros((h, w), np.uint8)) in in4 and do.mask_string(np.ones((h, w), np.uint8)) in [s for s, q in zip(strings, planes) if q == 6]
        from tests import writer_oracle as wo
        assert sum(0 in wo.string_to_counts(s)[1:] for s in in4) >= 40, "strings with zero-length runs inside"
        st5 = status[[m for m, q in enumerate(planes) if q == 5]].tolist()
        assert set(st5) == {0, 1, 2, 4, 8, 16} and st5[0] == 0 and st5[-1] == 0 and all(x == 0 for x in st5[::2]) and all(x != 0 for x in st5[1::2])
        assert not status[[m for m, q in enumerate(planes) if q != 5]].any() and 0 < ref[5].mean() < 1


@pytest.mark.parametrize("name", sorted(mo.END_TO_END))
def test_end_to_end_cases_stay_inside_the_caps_of_the_band_rule_and_the_tie_rule(on_disk, cfg, name):
    """``augment_oracle.check_warp`` excuses elements inside a rounding band and ``data_oracle.check_tie_rule`` pixels near 0.5, each up to
    a cap of 1e-3 of the elements: the cases must leave the oracle itself well inside those caps, or the checks would say little."""
    from stemseg_amd.data import MapillaryDataLoader
    from stemseg_amd.data.common import compute_resize_params, compute_padding
    _, base, _, ids = on_disk
    index, limit, seed = mo.END_TO_END[name]
    ds = MapillaryDataLoader(base, ids, max_nbr_instances=limit)
    random.seed(seed)
    r = ds[index]
    w, h = r["size"]
    N, T = r["n_instances"], len(r["perm"])
    assert N == {"many": 16, "few": 3, "max2": 1, "no_target": 0}[name] and r["has_ignore"]
    src, planes, ref, _ = mo.recipe_warp(r)
    singles = np.stack([do.decode_strings([s], [0], 1, h, w)[0][0] for s in r["rle"][N:]])
    assert (singles.sum(0) > 1).any(), "overlapping ignore strings"
    assert np.array_equal(planes[N], singles.any(0)[:, ::-1] if r["flip"] else singles.any(0))
    if N:
        assert (planes[N] & planes[:N].any(0)).any(), "the ignore plane overlaps a target in the image itself"
    # (the frames' band is +-1e-3 about k + 0.5, which holds 2e-3 of any smooth distribution: there the cap binds the mismatches, not the band)
    for share, what in ((ao.weight_band(ref["weight"]).mean(), "invalid"), (ref["near_coord"].mean(), "planes")):
        assert share < ao.SHARE_CAP / 4, (name, what, share)
    assert ref["planes"][N].any() and ref["invalid"].any() and not ref["invalid"].all()
    new_w, new_h, _ = compute_resize_params((h, w), cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM)
    every = ref["planes"].copy()
    every[:, r["perm"].index(0)] = planes
    _, soft = do.resize_masks(every.reshape(-1, h, w), (new_h, new_w), (new_h + compute_padding(new_w, new_h)[1], new_w + compute_padding(new_w, new_h)[0]))
    assert do.near_tie_share(soft) < 1e-3 / 4, (name, do.near_tie_share(soft))
