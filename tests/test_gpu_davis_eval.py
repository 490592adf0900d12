"""GPU tests of the DAVIS evaluation: ``stemseg_hip_davis_eval_counts`` (csrc/davis_eval.hip) against the numpy oracle
(tests/davis_eval_oracle.py) with exact integer equality on the cases of tests/davis_eval_cases.py, the tables between canaries, two runs
bit for bit; ``DavisEvaluator`` with ``==`` in fp64 against the oracle's statistics; ``gt_planes_from_json``; the inference driver's
``--eval_annotations``; ``make_validator`` before and after an SGD step.  Agreement of the measure with the official DAVIS toolkit is not tested: the toolkit is not available here."""
import ctypes as C
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import davis_eval_cases as cases
from tests import davis_eval_oracle as oracle

pytestmark = pytest.mark.gpu
GUARD = 4096
CANARY = 0xA5


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def to_device(pred):
    """uint8 as it is; uint16 as the int16 bits the writers' 16-bit maps travel in."""
    return torch.from_numpy(pred.view(np.int16).copy() if pred.dtype == np.uint16 else pred.copy()).cuda()


def counts_guarded(hip, pred, gt, Kp, r, fill=0x5A):
    """The C call with the tables between canaries, over a payload that holds ``fill`` bytes before -> {name: int64 array}."""
    T, H, W = pred.shape
    Kg = gt.shape[0]
    need = int(hip.lib().stemseg_hip_davis_eval_counts_size(T, Kp, Kg))
    assert need == T * (3 * Kp * Kg + 2 * Kp + 2 * Kg)
    buf = torch.full((4 * need + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + 4 * need] = fill
    p, g = to_device(pred), torch.from_numpy(gt.copy()).cuda()
    rc = hip.lib().stemseg_hip_davis_eval_counts(C.c_void_p(p.data_ptr()), pred.dtype.itemsize, C.c_void_p(g.data_ptr()), T, H, W, Kp, Kg, r,
                                                 C.c_void_p(buf.data_ptr() + GUARD), need, hip.stream())
    assert rc == 0, hip.lib().stemseg_hip_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + 4 * need:] == CANARY).all()), "a canary around the tables was overwritten"
    flat = buf[GUARD:GUARD + 4 * need].cpu().numpy().view(np.int32)
    out, at = {}, 0
    for key, shape in zip(hip.DAVIS_EVAL_TABLES, hip.davis_eval_table_shapes(T, Kp, Kg)):
        n = int(np.prod(shape))
        out[key] = flat[at:at + n].reshape(shape).astype(np.int64)
        at += n
    return out


def assert_tables(got, want, what):
    for key in oracle.TABLES:
        assert got[key].shape == want[key].shape, (what, key)
        bad = np.argwhere(got[key] != want[key])
        assert bad.size == 0, "%s: %s differs at %d entries, first (index, got, oracle) %s" % (
            what, key, len(bad), [(tuple(i), int(got[key][tuple(i)]), int(want[key][tuple(i)])) for i in bad[:4]])


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_counts_equal_the_oracle(hip, name):
    """Every table, exactly; the tables lie between canaries and start out holding garbage; a second run over another garbage gives the
    same bits (the zero fill is the call's own, the sums are integer)."""
    pred, gt, Kp, r, want = cases.case(name)
    got = counts_guarded(hip, pred, gt, Kp, r)
    assert_tables(got, want, name)
    again = counts_guarded(hip, pred, gt, Kp, r, fill=0xC3)
    for key in oracle.TABLES:
        assert np.array_equal(got[key], again[key]), (name, key)


def test_wrapper_returns_the_tables_as_views_of_one_buffer(hip):
    pred, gt, Kp, r, want = cases.case("special")
    tables = hip.davis_eval_counts(to_device(pred), torch.from_numpy(gt.copy()).cuda(), Kp, r)
    assert len(tables) == 7 and all(t.dtype == torch.int32 and t.is_cuda for t in tables)
    assert_tables({k: t.cpu().numpy().astype(np.int64) for k, t in zip(hip.DAVIS_EVAL_TABLES, tables)}, want, "wrapper")
    first = tables[0].data_ptr()
    assert [t.data_ptr() - first for t in tables] == list(4 * np.cumsum([0] + [int(np.prod(s)) for s in hip.davis_eval_table_shapes(4, 4, 3)][:-1]))
    with pytest.raises(ValueError, match="limit is 64"):
        hip.davis_eval_counts(to_device(pred), torch.from_numpy(gt.copy()).cuda(), 65, r)
    with pytest.raises(ValueError, match="radius"):
        hip.davis_eval_counts(to_device(pred), torch.from_numpy(gt.copy()).cuda(), Kp, 33)


def test_no_leak_between_frames(hip):
    """The counts of a sequence equal those of its frames evaluated alone, where a mask on the last rows of one frame and one on the
    first rows of the next are within r of each other in memory."""
    pred, gt, Kp, r, want = cases.case("frame leak")
    whole = counts_guarded(hip, pred, gt, Kp, r)
    assert_tables(whole, want, "frame leak")
    for t in range(pred.shape[0]):
        alone = counts_guarded(hip, pred[t:t + 1], gt[:, t:t + 1], Kp, r)
        for key in oracle.TABLES:
            assert np.array_equal(alone[key][0], whole[key][t]), (t, key)


# ------------------------------------------------------------------------------------------------ the evaluator
def test_evaluator_equals_the_oracle_summary(hip):
    from stemseg_amd.evaluation.davis import DavisEvaluator, radius
    ev, ref = DavisEvaluator(), {}
    for name, pred, gt, Kp in cases.evaluator_sequences():
        T, H, W = pred.shape
        stats = ev.add_sequence(name, to_device(pred), torch.from_numpy(gt).cuda(), n_proposals=Kp)
        ref[name] = oracle.sequence_stats(oracle.counts(pred, gt, Kp, oracle.radius(H, W)), Kp, gt.shape[0])
        assert radius(H, W) == oracle.radius(H, W)
        assert stats["assignment"] == ref[name]["assignment"]
        assert stats["objects"] == ref[name]["objects"]                       # fp64, ==
        assert np.array_equal(stats["J"], np.asarray(ref[name]["J"])) and np.array_equal(stats["F"], np.asarray(ref[name]["F"]))
    got, want = ev.summary(), oracle.summary(ref)
    assert list(got)[:7] == ["J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay"]
    for key, value in want.items():
        assert got[key] == value, key
    assert list(got["sequences"]) == ["more-proposals", "fewer-proposals"]
    assert -1 in ref["fewer-proposals"]["assignment"], "the second sequence must leave an object without a proposal"
    # without n_proposals the largest label of the map is read back: the same figures here, where every label occurs
    ev2 = DavisEvaluator()
    for name, pred, gt, Kp in cases.evaluator_sequences():
        assert int(pred.max()) == Kp
        ev2.add_sequence(name, to_device(pred), torch.from_numpy(gt).cuda())
    assert ev2.summary() == got
    with pytest.raises(ValueError, match="at least 3"):
        DavisEvaluator().add_sequence("short", torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda"),
                                      torch.zeros((1, 2, 8, 8), dtype=torch.uint8, device="cuda"), n_proposals=1)


def test_gt_planes_from_json_round_trips(hip):
    """A record built with the suite's RLE helpers: ids out of order in the file, an instance absent from a frame."""
    from stemseg_amd.evaluation.davis import gt_planes_from_json
    from tests import data_oracle as do
    T, H, W = 4, 37, 53
    _, planes = cases.scene(T, H, W, 1, 3, 31)
    ids = [7, 2, 11]                                    # plane k of `planes` belongs to ids[k]; ascending: 2, 7, 11
    segs = [{str(iid): do.mask_string(planes[k, t]) for k, iid in enumerate(ids) if not (iid == 7 and t == 2)} for t in range(T)]
    record = {"id": "seq", "height": H, "width": W, "image_paths": ["%05d.jpg" % t for t in range(T)],
              "categories": {str(i): 1 for i in ids}, "segmentations": segs}
    got, order = gt_planes_from_json(record, "cuda")
    assert order == [2, 7, 11] and tuple(got.shape) == (3, T, H, W) and got.dtype == torch.uint8
    want = np.stack([planes[1], planes[0], planes[2]]).copy()
    want[1, 2] = 0
    assert np.array_equal(got.cpu().numpy(), want)
    record["segmentations"][1]["2"] = "!!"
    with pytest.raises(ValueError, match="instance 2 in frame 1"):
        gt_planes_from_json(record, "cuda")


# ------------------------------------------------------------------------------------------------ the inference driver
@pytest.fixture(scope="module")
def tiny_davis(tmp_path_factory):
    """The small model of tests/test_overlay.py (davis preset, R-50, synthetic weights, 96 x 128 inputs) over one 12-frame sequence of
    90 x 120 PNG files, annotated with two drifting objects."""
    from PIL import Image
    from stemseg_amd import config
    from stemseg_amd.data.generic_video_dataset_parser import GenericVideoSequence
    from stemseg_amd.modeling.inference_model import InferenceModel
    from tests import data_oracle as do
    from tests import synth
    root = tmp_path_factory.mktemp("tiny_davis")
    T, H, W = 12, 90, 120
    frames = synth.synth_frames(T, H, W, seed=5)
    os.makedirs(str(root / "seq0"))
    for t, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(str(root / "seq0" / ("%05d.png" % t)))
    _, planes = cases.scene(T, H, W, 1, 2, 41)
    record = {"id": "seq0", "height": H, "width": W, "image_paths": ["seq0/%05d.png" % t for t in range(T)], "categories": {"3": 1, "9": 1},
              "segmentations": [{"3": do.mask_string(planes[0, t]), "9": do.mask_string(planes[1, t])} for t in range(T)]}
    vds = str(root / "val.json")
    with open(vds, "w") as fh:
        json.dump({"meta": {"category_labels": {"1": "object"}}, "sequences": [record]}, fh)
    try:
        config.load_preset("davis")
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 96, 128
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        model = InferenceModel(None, semseg_output_type=None, preload_images=True, resize_scale=1.0, semseg_generation_on_gpu=True)
        sd = model._model.state_dict()
        new = {k: torch.from_numpy(np.asarray(synth.synth_param(k, v.shape, 61))).reshape(v.shape) for k, v in sd.items()}
        new["seediness_head.conv_out.weight"] = new["seediness_head.conv_out.weight"] * 12.0
        model.load_checkpoint_state(new)
        model = model.cuda()
        paths = [str(root / p) for p in record["image_paths"]]
        probe = model(paths, [list(range(8))])["embeddings"][0].seediness.flatten()
        config.cfg.CLUSTERING.MIN_SEEDINESS_PROB = float(probe.quantile(0.75))
        yield NS(root=root, vds=vds, model=model, thr=float(probe.median()), planes=planes, record=record,
                 sequence=lambda: GenericVideoSequence(record, str(root)))
    finally:
        config.load_preset("defaults")


def _png_bytes(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


def test_driver_writes_the_evaluation_and_leaves_the_pngs_alone(hip, tiny_davis):
    from PIL import Image
    from stemseg_amd.evaluation.davis import DavisEvaluator, gt_planes_from_json
    from stemseg_amd.inference import main
    d, said = tiny_davis, []
    common = [str(d.root / "model.pth"), "--dataset", "davis", "--seediness_thresh", repr(d.thr), "--frame_overlap", "4", "--max_tracks", "10"]
    plain = main.main(main.build_parser().parse_args(common + ["-o", "plain"]), model=d.model, sequences=[d.sequence()], print_fn=said.append)
    assert plain is None and not os.path.exists(str(d.root / "plain" / "davis_eval.json"))
    got = main.main(main.build_parser().parse_args(common + ["-o", "scored", "--eval_annotations", d.vds]), model=d.model,
                    sequences=[d.sequence()], print_fn=said.append)
    a, b = _png_bytes(str(d.root / "plain" / "results" / "seq0")), _png_bytes(str(d.root / "scored" / "results" / "seq0"))
    assert len(a) == 12 and a == b, "the flag must not change a byte of the results"
    on_disk = json.load(open(str(d.root / "scored" / "davis_eval.json")))
    assert on_disk == json.loads(json.dumps(got)) and any("J&F-Mean" in str(s) for s in said)
    # the evaluator by hand on the maps the driver wrote
    maps = np.stack([np.asarray(Image.open(str(d.root / "scored" / "results" / "seq0" / ("%05d.png" % t)))) for t in range(12)])
    Kp = on_disk["sequences"]["seq0"]["proposals"]
    assert maps.dtype == np.uint8 and 2 <= int(maps.max()) <= Kp <= 10
    planes, ids = gt_planes_from_json(d.record, "cuda")
    assert ids == [3, 9] and np.array_equal(planes.cpu().numpy(), d.planes)
    ev = DavisEvaluator()
    ev.add_sequence("seq0", torch.from_numpy(maps).cuda(), planes, n_proposals=Kp)
    by_hand = ev.summary()
    assert json.loads(json.dumps(by_hand)) == on_disk
    ref = oracle.sequence_stats(oracle.counts(maps, d.planes, Kp, oracle.radius(90, 120)), Kp, 2)
    assert oracle.summary({"seq0": ref})["J&F-Mean"] == on_disk["J&F-Mean"]
    for key in ("J&F-Mean", "J-Mean", "J-Recall", "F-Mean", "F-Recall"):
        assert 0.0 <= on_disk[key] <= 1.0


# ------------------------------------------------------------------------------------------------ the Trainer's validator
def test_validator_follows_the_trainers_weights(hip, tiny_davis):
    """One call on the tiny model gives finite figures in [0, 1]; after an SGD step on the training model a second call, through the SAME
    kept inference model, gives exactly the figures of a fresh inference model loaded from the stepped state dict -- and other figures
    than before the step."""
    from stemseg_amd.evaluation.davis import DavisEvaluator, gt_planes_from_json, make_validator
    from stemseg_amd.inference import main
    from stemseg_amd.inference.output_utils import MaskMaterializer
    from stemseg_amd.modeling.inference_model import InferenceModel
    from stemseg_amd.modeling.model_builder import build_model
    d = tiny_davis
    training = build_model(restore_pretrained_backbone_wts=False)
    training.load_state_dict(d.model._model.state_dict(), strict=False)
    training = training.cuda()
    trainer = NS(model=training, local_device=torch.device("cuda", torch.cuda.current_device()))
    validate = make_validator(d.vds, str(d.root), max_tracks=10, seediness_thresh=d.thr, frame_overlap=4)
    with torch.no_grad():
        first = validate(trainer)
    assert list(first) == ["J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay"]
    assert all(np.isfinite(v) for v in first.values()) and all(0.0 <= first[k] <= 1.0 for k in first if "Decay" not in k)
    # the same weights through the driver gave davis_eval.json's figures (test above): the validator's path is the driver's
    opt = torch.optim.SGD(training.parameters(), lr=1.0)
    for p in training.parameters():
        if p.requires_grad:
            p.grad = 0.3 * p.detach()
    opt.step()
    with torch.no_grad():
        second = validate(trainer)

    fresh = InferenceModel(None, semseg_output_type=None, preload_images=True, resize_scale=1.0)
    fresh.load_checkpoint_state(training.state_dict())
    fresh = fresh.cuda()
    tracks = main.TrackGenerator(fresh, "davis", seediness_thresh=d.thr, frame_overlap=4)
    seq = d.sequence()
    emb, fg, _ = tracks.do_inference([os.path.join(seq.base_dir, p) for p in seq.image_paths])
    (track, _, life), idx = tracks.do_clustering(emb, fg)[:2]
    keep, masks = MaskMaterializer(-1).process_sequence(seq.image_dims, idx, track, life, tuple(fg.shape[-2:]), 4.0, 10)
    ev = DavisEvaluator()
    ev.add_sequence("seq0", masks, gt_planes_from_json(d.record, "cuda")[0], n_proposals=len(keep))
    want = {k: v for k, v in ev.summary().items() if k != "sequences"}
    assert second == want, "the kept model must run the stepped weights"
    assert second != first, "the step must show in the figures, or the test says nothing"
