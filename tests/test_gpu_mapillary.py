"""GPU tests of the Mapillary path: ``rle_decode_union`` (csrc/data_loader.hip) byte for byte against tests/mapillary_oracle.py -- planes
and status, every output between canaries -- and the dataset end to end through ``device_collate`` and one ``Trainer`` iteration on a
synthetic ``mapillary.json`` over the golden's frames.  A batch entry is checked in the two stages of tests/test_gpu_image_datasets.py:
the device's warp against tests/augment_oracle.py under its band rule, then the images within 1e-4 and the masks under the tie rule of
tests/data_oracle.py.  tests/test_mapillary_host.py checks on the oracle alone that the cases hold what they are meant to."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from tests import augment_oracle as ao
from tests import data_oracle as do
from tests import mapillary_oracle as mo

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
    base = str(tmp_path_factory.mktemp("mapillary"))
    vds = gold.write(base)
    return base, vds, mo.write_dataset(base)


@pytest.fixture()
def cfg(gold, monkeypatch):
    from stemseg_amd import config
    config.load_preset("defaults")
    gold.configure(config.cfg)
    monkeypatch.setenv("STEMSEG_METAINFO_DIR", METAINFO)
    yield config.cfg
    config.load_preset("defaults")


@pytest.fixture(scope="module")
def cases():
    """Per shape: (strings, plane_of_string, P, the oracle's planes, the oracle's status), computed once."""
    out = {}
    for h, w in mo.UNION_SHAPES:
        strings, planes, P = mo.union_case(h, w)
        out[(h, w)] = (strings, planes, P) + mo.decode_union(strings, planes, P, h, w)
    return out


def decode_union_guarded(hip, strings, plane_of_string, P, h, w, fill=0xFF):
    """``stemseg_hip_rle_decode_union`` through the C call, every buffer between canaries and the outputs pre-filled with 0xFF (NaN as
    floats, and neither 0 nor 1 as a mask) -> (planes, status) numpy."""
    from tests.test_gpu_data_loader import Guarded
    chars, offsets, pidx = hip.rle_pack(strings, plane_of_string)
    M, n = len(strings), int(chars.size)
    nbytes = hip.lib().stemseg_hip_rle_decode_union_workspace_bytes(n, M, P)
    assert nbytes > 0
    ws, planes, status = Guarded(nbytes, fill), Guarded(P * h * w, fill), Guarded(max(M, 1), fill)
    chars_dev, offs_dev, pidx_dev = Guarded(max(n, 1)), Guarded(offsets.nbytes), Guarded(max(pidx.nbytes, 4))
    if n:
        chars_dev.view[:n].copy_(torch.from_numpy(chars.copy()))
    offs_dev.view.copy_(torch.from_numpy(offsets.view(np.uint8).copy()))
    if M:
        pidx_dev.view[:pidx.nbytes].copy_(torch.from_numpy(pidx.view(np.uint8).copy()))
    rc = hip.lib().stemseg_hip_rle_decode_union(C.c_void_p(chars_dev.view.data_ptr()) if n else None, n, offsets.ctypes.data_as(C.c_void_p),
                                                pidx.ctypes.data_as(C.c_void_p) if M else None, C.c_void_p(offs_dev.view.data_ptr()),
                                                C.c_void_p(pidx_dev.view.data_ptr()) if M else None, M, P, h, w, C.c_void_p(ws.view.data_ptr()),
                                                nbytes, C.c_void_p(planes.view.data_ptr()), C.c_void_p(status.view.data_ptr()), hip.stream())
    assert rc == 0, hip.lib().stemseg_hip_last_error().decode()
    torch.cuda.synchronize()
    for name, g in (("workspace", ws), ("planes", planes), ("status", status), ("chars", chars_dev), ("offsets", offs_dev), ("plane indices", pidx_dev)):
        assert g.intact(), "a canary around the %s was overwritten" % name
    return planes.view.cpu().numpy().reshape(P, h, w), status.view[:M].cpu().numpy()


def differing(got, ref):
    return np.flatnonzero((got != ref).reshape(got.shape[0], -1).any(1)).tolist()


# ------------------------------------------------------------------------------------------------ rle_decode_union
@pytest.mark.parametrize("shape", mo.UNION_SHAPES, ids=lambda s: "%dx%d" % s)
def test_union_decode_is_byte_exact_between_canaries(hip, cases, shape):
    """Planes with 0, 1, 2 and 130 strings, the big unions first, in the middle and last, overlapping and disjoint strings, all-zero and
    all-one strings, zero-length runs, and one malformed string of each status between valid ones: planes and status byte for byte, every
    byte of the 0xFF-filled output written, no canary touched."""
    h, w = shape
    strings, plane_of_string, P, ref, ref_status = cases[shape]
    planes, status = decode_union_guarded(hip, strings, plane_of_string, P, h, w)
    assert status.tolist() == ref_status.tolist()
    assert set(np.unique(planes).tolist()) <= {0, 1}, "a byte of the planes was not written"
    assert np.array_equal(planes, ref), "planes %s differ" % differing(planes, ref)
    # the plane of the malformed strings is the union of the others
    good = [m for m, q in enumerate(plane_of_string) if q == 5 and ref_status[m] == 0]
    others, _ = mo.decode_union([strings[m] for m in good], [0] * len(good), 1, h, w)
    assert np.array_equal(planes[5], others[0]) and len(good) < plane_of_string.count(5)


def test_union_decode_through_the_binding_and_in_two_orders(hip, cases):
    h, w = 37, 53
    strings, plane_of_string, P, ref, ref_status = cases[(h, w)]
    planes, status = hip.rle_decode_union(strings, plane_of_string, P, h, w)
    assert planes.dtype == torch.uint8 and tuple(planes.shape) == (P, h, w) and status.cpu().tolist() == ref_status.tolist()
    assert np.array_equal(planes.cpu().numpy(), ref)
    order = sorted(range(len(strings)), key=lambda m: (plane_of_string[m], -m))          # every plane's strings reversed
    assert order != list(range(len(strings)))
    again, status2 = hip.rle_decode_union([strings[m] for m in order], [plane_of_string[m] for m in order], P, h, w)
    assert torch.equal(again, planes) and status2.cpu().tolist() == [int(ref_status[m]) for m in order]
    out = torch.full((P, h, w), 7, dtype=torch.uint8, device="cuda")
    assert hip.rle_decode_union(strings, plane_of_string, P, h, w, planes=out)[0] is out and torch.equal(out, planes)
    with pytest.raises(ValueError, match="decrease"):
        hip.rle_decode_union(strings[:3], [1, 1, 0], P, h, w)
    # no string at all: every plane is zero
    none, st = hip.rle_decode_union([], [], 2, h, w)
    assert not none.any() and st.numel() == 0


def test_union_decode_more_planes_than_grid_rows(hip):
    """1025 planes of 24 x 25, two or three overlapping rectangles on planes 0, 1, 1023 and 1024: the rasteriser's workgroups of plane 0
    come back for plane 1024 (tests/data_oracle.py); every plane and the status, twice."""
    strings, plane_of_string, _, P, h, w = do.strided_planes_case()
    ref, ref_status = mo.decode_union(strings, plane_of_string, P, h, w)
    assert np.flatnonzero(ref.reshape(P, -1).any(1)).tolist() == [0, 1, 1023, 1024] and not np.array_equal(ref[0], ref[1024])
    planes, status = decode_union_guarded(hip, strings, plane_of_string, P, h, w)
    assert status.tolist() == ref_status.tolist() == [0] * len(strings)
    assert np.array_equal(planes, ref), "planes %s differ" % differing(planes, ref)
    again, status2 = decode_union_guarded(hip, strings, plane_of_string, P, h, w, fill=0x00)
    assert again.tobytes() == planes.tobytes() and status2.tobytes() == status.tobytes(), "two runs, bit for bit"


def test_union_decode_of_distinct_planes_equals_rle_decode(hip):
    """The 300 unequal strings of tests/data_oracle.py over 320 planes, sorted by plane: both entry points, bit for bit."""
    strings, planes, P, h, w = do.unequal_batch()
    order = sorted(range(len(strings)), key=lambda m: planes[m])
    strings, planes = [strings[m] for m in order], [planes[m] for m in order]
    a, sa = hip.rle_decode(strings, planes, P, h, w)
    b, sb = hip.rle_decode_union(strings, planes, P, h, w)
    assert torch.equal(a, b) and torch.equal(sa, sb) and a.any()
    for name, bad, want in do.malformed_cases(7, 5):
        good = do.mask_string(do.mask_with_runs(7, 5, 4))
        a, sa = hip.rle_decode([good, bad, good], [0, 1, 3], 4, 7, 5)
        b, sb = hip.rle_decode_union([good, bad, good], [0, 1, 3], 4, 7, 5)
        assert torch.equal(a, b) and sa.cpu().tolist() == sb.cpu().tolist() == [0, want, 0], name


# ------------------------------------------------------------------------------------------------ the batch
def check_entry(hip, cfg, recipe, images, target, new_hw, pad_hw, what):
    """``check_image_entry`` of tests/test_gpu_image_datasets.py for a recipe whose last plane is a union."""
    from stemseg_amd.data.common import image_clip_parameters
    w, h = recipe["size"]
    T, N, P = len(recipe["perm"]), recipe["n_instances"], recipe["n_instances"] + int(recipe["has_ignore"])
    src, planes, ref, blurs = mo.recipe_warp(recipe)
    # stage 1: the device's warp of this recipe's planes (the device's own union decode, held to the oracle first) against the oracle's
    raw = do.decode_image(recipe["frames"][0])
    raw_planes = mo.recipe_planes(recipe)
    dev_planes, status = hip.rle_decode_union(recipe["rle"], recipe["rle_planes"], max(P, 1), h, w)
    assert not status.any() and np.array_equal(dev_planes.cpu().numpy()[:P], raw_planes)
    hinvs, jitter, dev_blurs = image_clip_parameters(recipe)
    frames, wplanes, invalid = hip.warp_clip(torch.from_numpy(raw).cuda(), dev_planes[:P] if P else None, hinvs, jitter)
    ao.check_warp(frames.cpu().numpy(), wplanes.cpu().numpy(), invalid.cpu().numpy(), ref, what)
    assert all(b is None for b in blurs) and all(b is None for b in dev_blurs)
    k0 = recipe["perm"].index(0)
    assert np.array_equal(frames[k0].cpu().numpy(), src) and not invalid[k0].any(), "the image itself goes through unchanged (mirrored or not)"
    # stage 2: the batch entry against the oracle's pre-processing / resize of those frames and planes
    ref_images = ao.preprocess_masked(frames.cpu().numpy(), invalid.cpu().numpy(), new_hw, pad_hw, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD,
                                      cfg.INPUT.NORMALIZE_TO_UNIT_SCALE, not cfg.INPUT.BGR_INPUT)
    err = float(np.abs(images.cpu().numpy() - ref_images).max())
    print("%s: images differ from the oracle's by %.3g" % (what, err))
    assert err <= 1e-4
    assert tuple(target["masks"].shape) == (N, T) + tuple(pad_hw) and tuple(target["ignore_masks"].shape) == (T,) + tuple(pad_hw)
    assert target["masks"].dtype == torch.uint8 and target["ignore_masks"].dtype == torch.uint8
    if P == 0:
        assert not target["ignore_masks"].any()
        return None
    every = wplanes.cpu().numpy().copy()
    every[:, k0] = planes                                          # the image itself keeps its own planes, overlaps and all
    hard, soft = do.resize_masks(every.reshape(-1, h, w), new_hw, pad_hw)
    got = torch.cat([target["masks"], target["ignore_masks"][None]], 0).cpu().numpy() if recipe["has_ignore"] else target["masks"].cpu().numpy()
    assert got.shape[0] == every.shape[0]
    do.check_tie_rule(got.reshape(-1, *pad_hw), hard, soft, new_hw, what + " masks")
    return every, k0


def _recipe(base, ids, name):
    from stemseg_amd.data import MapillaryDataLoader
    index, limit, seed = mo.END_TO_END[name]
    random.seed(seed)
    return MapillaryDataLoader(base, ids, max_nbr_instances=limit)[index]


def test_device_collate_of_mapillary_recipes_two_frame_sizes_in_one_batch(hip, gold, on_disk, cfg):
    """The 35-instance sample (16 targets, 19 strings in the ignore plane), the 5-instance one and a KITTI-MOTS-style video clip in one
    batch: two frame sizes, a union call and a plain call."""
    from stemseg_amd.data.common import device_collate
    base, vds, ids = on_disk
    recipes = [_recipe(base, ids, "many"), _recipe(base, ids, "few")]
    assert [r["size"] for r in recipes] == [(53, 37), (40, 45)] and [r["n_instances"] for r in recipes] == [16, 3]
    assert len(recipes[0]["rle"]) == 35 > 30, "more instances than max_nbr_instances: the rest went into the ignore plane"
    video = do.make_loader("davis", base, vds)
    video.samples = [do.pick_clip(video.sequences, "a", do.CLIP_A)]
    batch = recipes + [video[0]]
    image_seqs, targets, meta = device_collate(batch)
    torch.cuda.synchronize()
    pad_hw = tuple(image_seqs.max_size)
    for n, r in enumerate(recipes):
        assert targets[n]["category_ids"].cpu().tolist() == r["category_ids"] and set(r["category_ids"]) == {1, 2}
        assert meta[n]["category_labels"] == [{1: "car", 2: "person"}[c] for c in r["category_ids"]]
        new_hw = tuple(image_seqs.image_sizes[n])
        every, k0 = check_entry(hip, cfg, r, image_seqs.tensors[n], targets[n], new_hw, pad_hw, "mapillary %d" % n)
        N, (w, h) = r["n_instances"], r["size"]
        # the un-warped frame: the ignore mask is the resized union, overlaps with the targets kept
        union = np.stack([do.decode_strings([s], [0], 1, h, w)[0][0] for s in r["rle"][N:]]).any(0).astype(np.uint8)
        union = union[:, ::-1] if r["flip"] else union
        hard, soft = do.resize_masks(union[None], new_hw, pad_hw)
        do.check_tie_rule(targets[n]["ignore_masks"][k0][None].cpu().numpy(), hard, soft, new_hw, "the un-warped ignore mask")
        assert (every[N, k0] & every[:N, k0].any(0)).any(), "the case must have the ignore plane overlapping a target in the image itself"
        got = torch.cat([targets[n]["masks"], targets[n]["ignore_masks"][None]], 0)
        assert (got[N, k0] & got[:N, k0].any(0)).any(), "in the image itself the overlap stays"
        # a warped frame: the ignore plane is the highest plane and wins, so no target pixel lies under it (at the source resolution,
        # where the condensed map decides)
        warped = [k for k in range(len(r["perm"])) if k != k0]
        assert all(not (every[N, k] & every[:N, k].any(0)).any() for k in warped) and any(every[N, k].any() for k in warped)
    alone = device_collate([batch[2]])
    nh, nw = alone[0].image_sizes[0]
    assert torch.equal(alone[0].tensors[0][:, :, :nh, :nw], image_seqs.tensors[2][:, :, :nh, :nw]), "the video sample is what it is alone"
    assert torch.equal(alone[1][0]["masks"][..., :nh, :nw], targets[2]["masks"][..., :nh, :nw])


def test_max_nbr_instances_pushes_instances_into_the_ignore_plane(hip, on_disk, cfg):
    from stemseg_amd.data.common import device_collate
    base, _, ids = on_disk
    r = _recipe(base, ids, "max2")
    assert r["n_instances"] == 1 and r["rle_planes"] == [0, 1, 1, 1, 1] and r["category_ids"] == [1]
    image_seqs, targets, _ = device_collate([r])
    torch.cuda.synchronize()
    check_entry(hip, cfg, r, image_seqs.tensors[0], targets[0], tuple(image_seqs.image_sizes[0]), tuple(image_seqs.max_size), "max2")
    few = _recipe(base, ids, "few")
    assert set(r["rle"][1:]) > set(few["rle"][few["n_instances"]:]), "what were targets at 30 are ignore strings at 2"


def test_recipe_without_a_target_and_without_any_plane(hip, on_disk, cfg):
    from stemseg_amd.data.common import device_collate
    base, _, ids = on_disk
    r = _recipe(base, ids, "no_target")
    assert r["n_instances"] == 0 and r["has_ignore"] and r["category_ids"] == [] and len(r["rle"]) == 5
    image_seqs, targets, _ = device_collate([r])
    torch.cuda.synchronize()
    new_hw, pad_hw = tuple(image_seqs.image_sizes[0]), tuple(image_seqs.max_size)
    T = len(r["perm"])
    assert tuple(targets[0]["masks"].shape) == (0, T) + pad_hw and targets[0]["category_ids"].numel() == 0 and targets[0]["ignore_masks"].any()
    check_entry(hip, cfg, r, image_seqs.tensors[0], targets[0], new_hw, pad_hw, "no target")
    bare = dict(r, rle=[], rle_planes=[], has_ignore=False)          # no plane at all: warp_clip gets none
    image_seqs2, targets2, _ = device_collate([bare])
    torch.cuda.synchronize()
    assert torch.equal(image_seqs2.tensors, image_seqs.tensors)
    check_entry(hip, cfg, bare, image_seqs2.tensors[0], targets2[0], new_hw, pad_hw, "no plane")
    # a refused string names the image and the string's position
    broken = dict(r, rle=r["rle"][:2] + [r["rle"][2][:-1] + "~"] + r["rle"][3:])
    with pytest.raises(ValueError, match=r"b/00001\.png, frame 0, instance 2: .*48\.\.111"):
        device_collate([broken])


def test_trainer_iteration_on_the_kittimots_1_mix(hip, gold, on_disk, tmp_path, monkeypatch):
    """One ``Trainer`` iteration on the ``kittimots_1`` preset's mix (Mapillary alone; R-50, the golden's frame count and sizes) fed by
    ``create_training_data_loader``: a finite loss, changed parameters, and the batch the trainer saw passes ``check_entry``."""
    import shutil
    from stemseg_amd import config
    from stemseg_amd.data.common import device_collate
    from stemseg_amd.training.utils import create_training_data_loader, create_training_dataset
    from tests.test_gpu_image_datasets import Recording
    from tests.test_gpu_trainer import OPTS, _build, _trainer, _training_cfg
    base, _, ids = on_disk
    shutil.copy(ids, str(tmp_path / "mapillary.json"))
    for var, value in (("MAPILLARY_IMAGES_DIR", base), ("STEMSEG_JSON_ANNOTATIONS_DIR", str(tmp_path)), ("STEMSEG_METAINFO_DIR", METAINFO)):
        monkeypatch.setenv(var, value)
    try:
        c = config.load_preset("kittimots_1")
        c.MODEL.BACKBONE.TYPE = "R-50-FPN"
        gold.configure(c)
        c.TRAINING.MAX_ITERATIONS, c.TRAINING.BATCH_SIZE = 4, 1
        said = []
        dataset = create_training_dataset(4, print_fn=said.append, mode=config.PRESET_TRAINING_MODES["kittimots_1"], device_mapillary=True)
        assert said == ["Training datasets: Mapillary"]
        one = Recording(dataset, [i for i, (_, s) in enumerate(dataset.id_mapping) if s == 1][0])          # the 5-instance sample
        m = _build()
        before = {k: p.detach().cpu().clone() for k, p in m.named_parameters()}
        tr = _trainer(tmp_path / "session", m, _training_cfg(BATCH_SIZE=1, MAX_ITERATIONS=1))
        (tmp_path / "session").mkdir(exist_ok=True)
        tr.data_loader = create_training_data_loader(one, 1, False, num_workers=0, device_mapillary=True)
        random.seed(mo.END_TO_END["few"][2])
        tr.start(OPTS)
        torch.cuda.synchronize()
        assert tr.elapsed_iterations == 1 and len(one.recipes) == 1
        recipe = one.recipes[0]
        assert recipe["kind"] == "image" and recipe["n_instances"] == 3 and recipe["has_ignore"] and recipe["rle_planes"] == [0, 1, 2, 3, 3]
        point = dict(tr.logger.last_point)
        assert len(point) >= 2 and all(np.isfinite(v) for v in point.values()), point
        moved = {k for k, p in m.named_parameters() if not torch.equal(p.detach().cpu(), before[k])}
        assert moved and all(bool(torch.isfinite(p).all()) for p in m.parameters())
        image_seqs, targets, _ = device_collate([recipe])
        check_entry(hip, config.cfg, recipe, image_seqs.tensors[0], targets[0], tuple(image_seqs.image_sizes[0]), tuple(image_seqs.max_size), "trainer")
        assert targets[0]["masks"].any() and targets[0]["ignore_masks"].any()
    finally:
        config.load_preset("defaults")
