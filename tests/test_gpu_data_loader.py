"""GPU tests of the training data loader's device half (csrc/data_loader.hip) and of the loader end to end: ``rle_decode`` bit for bit
against the numpy restatement of pycocotools' rleFrString + rleDecode (tests/data_oracle.py on tests/writer_oracle.py), malformed
strings, ``resize_masks`` against torch CPU under the tie rule of tests/test_gpu_parity.py, and ``device_collate`` / the Trainer / the
command line on the golden's synthetic dataset.  Every kernel output sits between canary blocks, which are checked."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import data_oracle as do
from tests import writer_oracle as wo

pytestmark = pytest.mark.gpu
GUARD = 4096
CANARY = 0xA5


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


class Guarded(object):
    """``nbytes`` of device memory between two canary blocks; ``fill``: what the payload holds before the call."""

    def __init__(self, nbytes, fill=0x5A):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.nbytes]
        self.view.fill_(fill)

    def intact(self):
        return bool((self.buf[:GUARD] == CANARY).all()) and bool((self.buf[GUARD + self.nbytes:] == CANARY).all())


def decode_guarded(hip, strings, plane_of_string, P, h, w):
    """``stemseg_hip_rle_decode`` through the C call with planes, status and workspace each between canaries -> (planes, status) numpy."""
    chars, offsets, pidx = hip.rle_pack(strings, plane_of_string)
    M, n = len(strings), int(chars.size)
    nbytes = hip.lib().stemseg_hip_rle_decode_workspace_bytes(n, M, P)
    assert nbytes > 0
    ws, planes, status = Guarded(nbytes), Guarded(P * h * w), Guarded(max(M, 1))
    chars_dev = Guarded(max(n, 1))
    offs_dev, pidx_dev = Guarded(offsets.nbytes), Guarded(max(pidx.nbytes, 4))
    if n:
        chars_dev.view[:n].copy_(torch.from_numpy(chars.copy()))
    offs_dev.view.copy_(torch.from_numpy(offsets.view(np.uint8).copy()))
    if M:
        pidx_dev.view[:pidx.nbytes].copy_(torch.from_numpy(pidx.view(np.uint8).copy()))
    rc = hip.lib().stemseg_hip_rle_decode(C.c_void_p(chars_dev.view.data_ptr()) if n else None, n, offsets.ctypes.data_as(C.c_void_p),
                                          pidx.ctypes.data_as(C.c_void_p) if M else None, C.c_void_p(offs_dev.view.data_ptr()),
                                          C.c_void_p(pidx_dev.view.data_ptr()) if M else None, M, P, h, w, C.c_void_p(ws.view.data_ptr()), nbytes,
                                          C.c_void_p(planes.view.data_ptr()), C.c_void_p(status.view.data_ptr()), hip.stream())
    assert rc == 0, hip.lib().stemseg_hip_last_error().decode()
    torch.cuda.synchronize()
    for name, g in (("workspace", ws), ("planes", planes), ("status", status), ("chars", chars_dev), ("offsets", offs_dev), ("plane indices", pidx_dev)):
        assert g.intact(), "a canary around the %s was overwritten" % name
    return planes.view.cpu().numpy().reshape(P, h, w), status.view[:M].cpu().numpy()


def check_decode(hip, strings, plane_of_string, P, h, w, what):
    ref_planes, ref_status = do.decode_strings(strings, plane_of_string, P, h, w)
    planes, status = decode_guarded(hip, strings, plane_of_string, P, h, w)
    assert status.tolist() == ref_status.tolist(), what
    assert np.array_equal(planes, ref_planes), "%s: planes %s differ" % (what, np.flatnonzero((planes != ref_planes).reshape(P, -1).any(1)).tolist())
    return planes


# ------------------------------------------------------------------------------------------------ rle_decode
def test_rle_decode_run_count_boundary_and_tiny_planes(hip):
    """7 x 5, 1 x 1, 1 x 40 and 40 x 1: all-zero, all-one, exactly 1 .. 5 counts with and without an empty first run; one call per size,
    every second plane unnamed -- those stay zero."""
    for name, h, w, masks in do.rle_small_cases():
        strings = [do.mask_string(m) for m in masks]
        for m, s in zip(masks, strings):
            assert np.array_equal(wo.decode(wo.string_to_counts(s), h, w), m)
        planes = check_decode(hip, strings, [2 * i + 1 for i in range(len(masks))], 2 * len(masks) + 1, h, w, name)
        assert not planes[0::2].any()
        assert np.array_equal(planes[1::2], np.stack(masks))


def test_rle_decode_count_widths_and_signed_deltas(hip):
    """Counts of 1, 2, 3 and 4 characters (up to one run over 600 x 700), and deltas of both signs around the 5-bit group boundaries."""
    widths = set()
    for h, w, counts in do.rle_count_width_cases():
        s = wo.counts_to_string(counts)
        assert wo.string_to_counts(s) == counts
        widths.add(len(do.deltas_to_string([max(counts)])))
        check_decode(hip, [s], [0], 1, h, w, "counts %s" % counts[:4])
    assert {1, 2, 3, 4} <= widths
    s = wo.counts_to_string(do.rle_count_width_cases()[5][2])
    last_groups = [ord(ch) - 48 for ch in s if not (ord(ch) - 48) & 0x20]
    assert any(g & 0x10 for g in last_groups) and any(not g & 0x10 for g in last_groups)


def test_rle_decode_scans_carry_over_workgroups_and_tiles(hip):
    """The 64 x 48 column checkerboard: 3072 counts in one string, more than a workgroup's 256 threads; three of them in one call with a
    blob between them pass the scan's 4096-element tile."""
    cb = do.checkerboard()
    s = do.mask_string(cb)
    assert len(wo.string_to_counts(s)) == 3072
    blob = do.mask_string(do.blobs(64, 48, 3, 1))
    planes = check_decode(hip, [s, blob, s, s], [3, 0, 1, 4], 5, 64, 48, "checkerboard")
    assert np.array_equal(planes[3], cb) and not planes[2].any()


def test_rle_decode_many_unequal_strings_in_one_call(hip):
    strings, plane_of_string, P, h, w = do.unequal_batch()
    assert len(strings) == 300 and max(map(len, strings)) > 100 * min(map(len, strings))
    planes = check_decode(hip, strings, plane_of_string, P, h, w, "300 strings")
    unnamed = sorted(set(range(P)) - set(plane_of_string))
    assert len(unnamed) == 20 and not planes[unnamed].any()


def test_rle_decode_more_planes_than_grid_rows(hip):
    """1025 planes of 24 x 25: the rasteriser's workgroups of plane 0 come back for plane 1024 (tests/data_oracle.py); every plane, twice."""
    strings, plane_of_string, _, P, h, w = do.strided_planes_case()
    first = [plane_of_string.index(q) for q in (0, 1, 1023, 1024)]
    strings = [strings[m] for m in first]
    planes = check_decode(hip, strings, [0, 1, 1023, 1024], P, h, w, "1025 planes")
    assert np.flatnonzero(planes.reshape(P, -1).any(1)).tolist() == [0, 1, 1023, 1024] and not np.array_equal(planes[0], planes[1024])
    again, status = decode_guarded(hip, strings, [0, 1, 1023, 1024], P, h, w)
    assert again.tobytes() == planes.tobytes() and not status.any(), "two runs, bit for bit"


def test_rle_decode_two_plane_sizes_in_two_calls(hip):
    """A batch of two frame sizes is two calls; the wrapper's own allocation path (no canaries) gives the same planes."""
    for (h, w), seed in (((37, 53), 1), ((45, 40), 2)):
        masks = [do.blobs(h, w, 3, seed + i) for i in range(3)]
        strings = [do.mask_string(m) for m in masks]
        check_decode(hip, strings, [0, 2, 1], 4, h, w, "%dx%d" % (h, w))
        planes, status = hip.rle_decode(strings, [0, 2, 1], 4, h, w)
        assert status.cpu().tolist() == [0, 0, 0]
        assert np.array_equal(planes.cpu().numpy(), np.stack([masks[0], masks[2], masks[1], np.zeros((h, w), np.uint8)]))
    with pytest.raises(ValueError, match="two strings"):          # (an argument error: refused before any launch)
        hip.rle_decode(["0", "0"], [1, 1], 3, 7, 5)
    # a character beyond one byte is sent as 0xFF, outside the alphabet: the status names the character, not the sum it would spoil
    good = do.mask_string(do.mask_with_runs(7, 5, 3))
    planes, status = hip.rle_decode([good, good[:1] + "€" + good[1:], good[:1] + "é" + good[1:]], [0, 1, 2], 3, 7, 5)
    assert status.cpu().tolist() == [0, hip.RLE_BAD_CHAR, hip.RLE_BAD_CHAR] and planes[0].any() and not planes[1:].any()


@pytest.mark.parametrize("case", do.malformed_cases(), ids=lambda c: c[0])
def test_rle_decode_refuses_malformed_strings(hip, case):
    """One malformed string between two good ones: the good ones decode, the bad one's plane is zero, its status is the documented bit,
    no canary is touched.  (The kernels bound every write by construction: the only stores into the planes are at a thread's own pixel.)"""
    name, bad, expected = case
    h, w = 7, 5
    assert do.string_status(bad, h, w) == expected
    good_a, good_b = do.mask_with_runs(h, w, 5), do.mask_with_runs(h, w, 3, start_one=True)
    strings = [do.mask_string(good_a), bad, do.mask_string(good_b)]
    planes, status = decode_guarded(hip, [s.encode("latin-1") for s in strings], [2, 1, 0], 3, h, w)
    assert status.tolist() == [0, expected, 0]
    assert np.array_equal(planes[2], good_a) and np.array_equal(planes[0], good_b) and not planes[1].any()


# ------------------------------------------------------------------------------------------------ resize_masks
def resize_guarded(hip, planes, new_hw, pad_hw, ranges=()):
    P, h, w = planes.shape
    R = len(ranges)
    src, out = Guarded(planes.size), Guarded((P + R) * pad_hw[0] * pad_hw[1])
    src.view.copy_(torch.from_numpy(np.ascontiguousarray(planes).reshape(-1)))
    r = np.ascontiguousarray(ranges, np.int32).reshape(-1, 3)
    rc = hip.lib().stemseg_hip_resize_masks(C.c_void_p(src.view.data_ptr()), P, h, w, new_hw[0], new_hw[1], pad_hw[0], pad_hw[1],
                                            r.ctypes.data_as(C.c_void_p) if R else None, R, 0, C.c_void_p(out.view.data_ptr()), hip.stream())
    assert rc == 0, hip.lib().stemseg_hip_last_error().decode()
    torch.cuda.synchronize()
    assert src.intact() and out.intact(), "a canary around the resize buffers was overwritten"
    return out.view.cpu().numpy().reshape(P + R, pad_hw[0], pad_hw[1])


@pytest.mark.parametrize("shape", do.RESIZE_SHAPES, ids=lambda s: "%dx%d" % s[0])
def test_resize_masks_against_torch_cpu(hip, shape):
    (h, w), new_hw, pads = shape
    planes = do.resize_planes(h, w)
    ranges = [(0, 2, 1), (1, 3, 2)]
    for pad_hw in pads:
        hard, soft = do.resize_masks(planes, new_hw, pad_hw, ranges)
        got = resize_guarded(hip, planes, new_hw, pad_hw, ranges)
        n = do.check_tie_rule(got, hard, soft, new_hw, "%s -> %s pad %s" % ((h, w), new_hw, pad_hw))
        print("resize %s -> %s pad %s: %d mismatches in the tie band" % ((h, w), new_hw, pad_hw, n))
    if (h, w) == (96, 128):          # exact 2x: every output is the mean of a 2 x 2 block, so ties are exactly 0.5 and must come out 0
        assert (soft == 0.5).any() and n == 0
        assert not got[:, :new_hw[0], :new_hw[1]][soft == 0.5].any()


def test_resize_masks_union_complement_is_taken_before_the_resize(hip):
    """2x down: a 2 x 2 block in which the union covers exactly two pixels is a tie for the union AND for its complement, so the
    complement-then-resize of the reference gives 0 where resize-then-complement would give 1."""
    a, b = np.zeros((8, 12), np.uint8), np.zeros((8, 12), np.uint8)
    a[2, 4] = 1
    b[3, 5] = 1
    a[6:8, 0:2] = 1
    planes = np.stack([a, b])
    hard, soft = do.resize_masks(planes, (4, 6), (32, 32), [(0, 2, 1)])
    union_first = 1 - (do.resize_soft((a | b)[None], (4, 6)).numpy()[0] > 0.5)
    assert hard[2, 1, 2] == 0 and union_first[1, 2] == 1
    got = resize_guarded(hip, planes, (4, 6), (32, 32), [(0, 2, 1)])
    assert np.array_equal(got, hard)
    assert np.array_equal(hip.resize_masks(torch.from_numpy(planes).cuda(), (4, 6), (32, 32), [(0, 2, 1)]).cpu().numpy(), hard)


def test_resize_masks_flip_x_is_the_resize_of_the_mirrored_planes(hip):
    planes = do.resize_planes(37, 53, seed=3)
    hard, soft = do.resize_masks(planes[:, :, ::-1], (48, 69), (64, 96), [(0, 3, 2)])
    got = hip.resize_masks(torch.from_numpy(planes).cuda(), (48, 69), (64, 96), [(0, 3, 2)], flip_x=True).cpu().numpy()
    do.check_tie_rule(got, hard, soft, (48, 69), "flip_x")
    assert not np.array_equal(got, do.resize_masks(planes, (48, 69), (64, 96), [(0, 3, 2)])[0])


# ------------------------------------------------------------------------------------------------ end to end
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


@pytest.mark.parametrize("name", ("ytvis", "davis", "mots"))
def test_device_collate_against_the_references_batch(hip, gold, on_disk, cfg, name):
    """The golden's two clips of different frame sizes (JPEG 37 x 53 and PNG 45 x 40) through ``device_collate`` against the batch the
    reference's ``VideoDataset.__getitem__`` + ``collate_fn`` made of them: sizes and category ids equal, masks and ignore masks (one
    ignore rule per loader) under the tie rule, images within the 1e-4 of the ``preprocess_frames`` test."""
    from stemseg_amd.data.common import device_collate
    ds = do.make_loader(name, *on_disk)
    ds.samples = [do.pick_clip(ds.sequences, "a", do.CLIP_A), do.pick_clip(ds.sequences, "b", do.CLIP_B)]
    recipes = [ds[0], ds[1]]
    rec = gold.record[name + "_batch"]
    image_seqs, targets, meta = device_collate(recipes)
    torch.cuda.synchronize()
    assert [list(s) for s in image_seqs.image_sizes] == rec["image_sizes"] and list(image_seqs.max_size) == rec["max_size"]
    assert [list(s) for s in image_seqs.original_image_sizes] == rec["original_image_sizes"]
    assert [m["seq_name"] for m in meta] == rec["seq_names"]
    assert image_seqs.tensors.is_cuda and image_seqs.tensors.dtype == torch.float32
    err = float((image_seqs.tensors.cpu() - torch.from_numpy(gold.npz["batch_images"])).abs().max())
    print("%s: images differ from the reference's by %.3g" % (name, err))
    assert err <= 1e-4
    soft = do.collate(recipes, cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM, cfg.INPUT.IMAGE_MEAN, cfg.INPUT.IMAGE_STD, with_images=False)
    ph, pw = rec["max_size"]
    for n, t in enumerate(targets):
        assert t["category_ids"].dtype == torch.int64 and t["category_ids"].cpu().tolist() == rec["category_ids"][n]
        assert t["masks"].dtype == torch.uint8 and t["ignore_masks"].dtype == torch.uint8 and t["masks"].is_cuda
        ref_m, ref_i = gold.npz["%s_masks_%d" % (name, n)], gold.npz["%s_ignore_%d" % (name, n)]
        assert tuple(t["masks"].shape) == ref_m.shape and tuple(t["ignore_masks"].shape) == ref_i.shape
        new_hw = tuple(rec["image_sizes"][n])
        k = do.check_tie_rule(t["masks"].cpu().numpy().reshape(-1, ph, pw), ref_m.reshape(-1, ph, pw),
                              soft["targets"][n]["soft_masks"].reshape((-1,) + new_hw), new_hw, "%s masks %d" % (name, n))
        k += do.check_tie_rule(t["ignore_masks"].cpu().numpy(), ref_i, soft["targets"][n]["soft_ignore"], new_hw, "%s ignore %d" % (name, n))
        print("%s sample %d: %d mask pixels in the tie band differ" % (name, n, k))


def test_device_collate_names_the_sequence_and_frame_of_a_bad_annotation(hip, gold, on_disk, cfg):
    from stemseg_amd.data.common import device_collate
    ds = do.make_loader("davis", *on_disk)
    ds.samples = [do.pick_clip(ds.sequences, "b", do.CLIP_B)]
    recipe = ds[0]
    inst, t, s = recipe["rle"][3]
    recipe["rle"][3] = (inst, t, s[:-1])
    with pytest.raises(ValueError, match=r"sequence b, frame %d, instance %d" % (t, inst)):
        device_collate([recipe])


def test_device_collate_samples_without_targets(hip, gold, on_disk, cfg):
    """A sample with no instance at all next to a full one of the same frame size: no targets, and under the background rule an ignore
    mask of ones over what the frame covers (the complement of an empty union), zero in the padding.  A sample whose only instance is the
    ignore instance: no targets, its planes the ignore masks."""
    from stemseg_amd.data.common import device_collate
    ds = do.make_loader("davis", *on_disk)
    ds.samples = [do.pick_clip(ds.sequences, "b", do.CLIP_B)]
    full = ds[0]
    bare = dict(full, rle=[], n_instances=0, category_ids=[], meta_info={"seq_name": "bare"})
    only_ignore = dict(full, rle=[(0, t, s) for i, t, s in full["rle"] if i == 0], n_instances=1, category_ids=[], ignore=("instance", 0),
                       meta_info={"seq_name": "only_ignore"})
    image_seqs, targets, _ = device_collate([bare, full, only_ignore, dict(bare, ignore=None)])
    nh, nw = image_seqs.image_sizes[0]
    ph, pw = image_seqs.max_size
    assert tuple(targets[0]["masks"].shape) == (0, 4, ph, pw) and targets[0]["category_ids"].numel() == 0
    ig = targets[0]["ignore_masks"].cpu().numpy()
    assert ig[:, :nh, :nw].all() and not ig[:, nh:].any() and not ig[:, :, nw:].any()
    alone = device_collate([full])[1][0]
    assert torch.equal(targets[1]["masks"], alone["masks"]) and torch.equal(targets[1]["ignore_masks"], alone["ignore_masks"])
    assert tuple(targets[2]["masks"].shape) == (0, 4, ph, pw)
    assert torch.equal(targets[2]["ignore_masks"], alone["masks"][0])
    assert not targets[3]["ignore_masks"].any()


def _small_kitti(gold, config):
    config.load_preset("kittimots")
    config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
    gold.configure(config.cfg)


def test_trainer_iteration_fed_by_the_loader(hip, gold, on_disk, tmp_path, monkeypatch):
    """One ``Trainer`` iteration on the kittimots preset (R-50, 4 frames, 64 x 96) fed by ``create_training_data_loader`` on the golden's
    dataset: the logged losses are, bit for bit, those of a twin model fed the device's images with the ORACLE's masks -- given that no
    mask pixel of the loader's batch differs from the oracle's, which the test asserts first."""
    from stemseg_amd import config
    from stemseg_amd.data.common import device_collate
    from stemseg_amd.training import configure_trainable
    from stemseg_amd.training.model_output_manager import ModelOutputManager
    from stemseg_amd.training.utils import create_training_data_loader, create_training_dataset
    from stemseg_amd.utils.constants import ModelOutput
    from tests.test_gpu_trainer import OPTS, _build, _trainer, _training_cfg
    base, _ = on_disk
    gold.write(str(tmp_path), "kittimots_train.json")
    monkeypatch.setenv("STEMSEG_JSON_ANNOTATIONS_DIR", str(tmp_path))
    monkeypatch.setenv("KITTIMOTS_BASE_DIR", base)
    try:
        _small_kitti(gold, config)
        import random
        random.seed(7)
        dataset = create_training_dataset(4, print_fn=lambda s: None, mode="kitti_mots")
        first_a = [i for i in range(len(dataset)) if dataset[i]["meta_info"]["seq_name"].startswith("a")][0]
        one = torch.utils.data.Subset(dataset, [first_a])
        recipe = one[0]
        assert isinstance(recipe["ignore"], tuple)
        m = _build()
        initial = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        tr = _trainer(tmp_path / "session", m, _training_cfg(BATCH_SIZE=1, MAX_ITERATIONS=1))
        (tmp_path / "session").mkdir(exist_ok=True)
        tr.data_loader = create_training_data_loader(one, 1, False, num_workers=0)
        tr.start(OPTS)
        torch.cuda.synchronize()
        assert tr.elapsed_iterations == 1
        point = dict(tr.logger.last_point)
        image_seqs, targets, _ = device_collate([recipe])
        oracle = do.collate([recipe], config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM, config.cfg.INPUT.IMAGE_MEAN, config.cfg.INPUT.IMAGE_STD,
                            with_images=False)["targets"][0]
        same = np.array_equal(targets[0]["masks"].cpu().numpy(), oracle["masks"]) and \
            np.array_equal(targets[0]["ignore_masks"].cpu().numpy(), oracle["ignore_masks"])
        assert same, "the premise does not hold: a mask pixel of the loader's batch differs from the oracle's, so the losses cannot be compared bit for bit"
        hand = [{"masks": torch.from_numpy(oracle["masks"]).cuda(), "ignore_masks": torch.from_numpy(oracle["ignore_masks"]).cuda(),
                 "category_ids": torch.tensor(oracle["category_ids"], dtype=torch.long).cuda()}]
        twin = configure_trainable(_build(initial))
        out = twin(image_seqs, hand)
        gathered = ModelOutputManager(1)          # (what the loop logs: the losses and the 'others' entries, a key in both summed)
        gathered(out)
        values = gathered.reset()[0]
        assert set(out[ModelOutput.OPTIMIZATION_LOSSES]) <= set(values) <= set(point)
        for k, v in values.items():
            assert point[k] == v.item(), (k, point[k], v)
        assert len(values) >= 2 and all(np.isfinite(point[k]) for k in point)
    finally:
        config.load_preset("defaults")


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
    c.DATA.KITTI_MOTS.FRAME_GAP_LOWER, c.DATA.KITTI_MOTS.FRAME_GAP_UPPER = {lo}, {hi}
    c.TRAINING.MAX_ITERATIONS, c.TRAINING.BATCH_SIZE = 2, 1
    return c
config.load_preset = small
small("kittimots")
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


def test_command_line_builds_its_loader_and_trains(hip, gold, on_disk, tmp_path):
    """``stemseg_amd.training.main`` with --build_data_loader, in a child process: the kittimots preset shrunk to the golden's dataset
    (R-50 from a synthetic backbone file, 4 frames, 64 x 96), two iterations, a checkpoint at the end.  The command line has no flag for
    the sizes, so the child first wraps ``config.load_preset`` to shrink the preset and then runs the module as ``__main__`` with the
    flags in ``sys.argv``, which is what ``python -m stemseg_amd.training.main`` does."""
    import os
    import subprocess
    import sys
    base, _ = on_disk
    gold.write(str(tmp_path), "kittimots_train.json")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lo, hi = gold.config["GAPS"]["KITTI_MOTS"]
    script = CHILD.format(root=root, pkg=os.path.join(root, "stem-seg_amd"), frames=gold.config["NUM_FRAMES"], min_dim=gold.config["MIN_DIM"],
                          max_dim=gold.config["MAX_DIM"], lo=lo, hi=hi)
    env = dict(os.environ, STEMSEG_JSON_ANNOTATIONS_DIR=str(tmp_path), KITTIMOTS_BASE_DIR=base, STEMSEG_MODELS_DIR=str(tmp_path / "models"))
    flags = ["--model_dir", "run", "--cfg", "kittimots", "--num_cpu_workers", "0", "--save_interval", "2", "--display_interval", "1"]
    r = subprocess.run([sys.executable, "-c", script] + flags + ["--build_data_loader"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "iteration 00002" in r.stderr and "Training datasets: KITTI-MOTS" in r.stderr, r.stderr[-3000:]
    saved = os.listdir(str(tmp_path / "models" / "checkpoints" / "run"))
    assert "000002.pth" in saved, saved
