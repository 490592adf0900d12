"""GPU tests of the YouTube-VIS evaluation: ``rle_pair_inter`` (csrc/data_loader.hip) with exact integer equality against
tests/ytvis_eval_oracle.py, outputs and workspace between canaries; ``YtvisEvaluator`` with ``==`` in fp64 against the oracle's summary;
the reader of the ground truth; the inference driver's ``--eval_ytvis_annotations``; ``make_validator``.  The cases are those of
tests/ytvis_eval_cases.py, which tests/test_ytvis_eval_host.py checks on the oracle alone."""
import ctypes as C
import json
import os
from collections import OrderedDict
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import ytvis_eval_cases as cases
from tests import ytvis_eval_oracle as oracle

pytestmark = pytest.mark.gpu
GUARD = 4096
CANARY = 0xA5
FIGURES = ("AP", "AP50", "AP75", "AR1", "AR10")


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


class Guarded(object):
    """``nbytes`` of device memory holding ``fill`` between two runs of canary bytes."""

    def __init__(self, nbytes, fill):
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.buf[GUARD:GUARD + nbytes] = fill
        self.ptr = C.c_void_p(self.buf.data_ptr() + GUARD)

    def intact(self):
        return bool((self.buf[:GUARD] == CANARY).all()) and bool((self.buf[GUARD + self.n:] == CANARY).all())

    def read(self, dtype):
        assert self.intact(), "a canary around an output was overwritten"
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().view(dtype)


# ------------------------------------------------------------------------------------------------ rle_pair_inter
def inter_guarded(hip, strings, pairs, h, w, fill):
    """The C call with area, inter, status AND the workspace (exactly ``..._workspace_bytes``) between canaries, over payloads that hold
    ``fill`` bytes before."""
    chars, offsets, _ = hip.rle_pack(strings, [])
    prs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    M, n, K = len(strings), int(chars.size), int(prs.shape[0])
    lib = hip.lib()
    nbytes = lib.stemseg_hip_rle_pair_inter_workspace_bytes(n, M, K)
    assert nbytes > 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() if a.size else torch.zeros(8, dtype=torch.uint8, device="cuda")
    d_chars, d_offs, d_pairs = dev(chars), dev(offsets), dev(prs)
    ws, area, inter, status = Guarded(nbytes, fill), Guarded(4 * M, fill), Guarded(4 * K, fill), Guarded(M, fill)
    at = lambda t: C.c_void_p(t.data_ptr())
    host = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.stemseg_hip_rle_pair_inter(at(d_chars) if n else None, n, host(offsets), host(prs) if K else None, at(d_offs),
                                        at(d_pairs) if K else None, M, K, h, w, ws.ptr, nbytes, area.ptr if M else None,
                                        inter.ptr if K else None, status.ptr if M else None, hip.stream())
    assert rc == 0, lib.stemseg_hip_last_error().decode()
    torch.cuda.synchronize()
    assert ws.intact(), "a canary around the workspace was overwritten"
    return area.read(np.int32), inter.read(np.int32), status.read(np.uint8)


def check_tables(got, want, c=None):
    for name, g, w_ in zip(("area", "inter", "status"), got, want):
        bad = np.flatnonzero(np.asarray(g, np.int64) != np.asarray(w_, np.int64))
        detail = ""
        if len(bad) and c is not None and name == "inter":
            names = {v: k for k, v in c["index"].items()}
            detail = str([(names[c["pairs"][k][0]], names[c["pairs"][k][1]], int(g[k]), int(w_[k])) for k in bad[:5]])
        assert len(bad) == 0, "%s differs at %s %s" % (name, bad[:10], detail)


@pytest.mark.parametrize("shape", cases.PAIR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_rle_pair_inter_equals_the_oracle(hip, shape):
    c = cases.pair_case(*shape)
    first = inter_guarded(hip, c["strings"], c["pairs"], c["h"], c["w"], 0xFF)
    check_tables(first, c["want"], c)
    second = inter_guarded(hip, c["strings"], c["pairs"], c["h"], c["w"], 0x00)        # other garbage before: every element is written
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes(), "two runs, bit for bit"
    # refused strings inside pairs: their area and those pairs' inter are 0, the other pairs are untouched (checked above against the
    # oracle); here the same call WITHOUT the refused strings gives the same numbers for the pairs that remain
    keep = [m for m in range(len(c["strings"])) if c["want"][2][m] == 0]
    renumber = {m: k for k, m in enumerate(keep)}
    kept_pairs = [k for k, (a, b) in enumerate(c["pairs"]) if a in renumber and b in renumber]
    clean = inter_guarded(hip, [c["strings"][m] for m in keep], [(renumber[c["pairs"][k][0]], renumber[c["pairs"][k][1]]) for k in kept_pairs],
                          c["h"], c["w"], 0x5A)
    assert np.array_equal(clean[0], first[0][keep]) and np.array_equal(clean[1], first[1][kept_pairs]) and not clean[2].any()


def test_rle_pair_inter_binding_equals_the_oracle(hip):
    """``hip.rle_pair_inter``: the three outputs are views of one buffer when none is given, and the caller's buffers otherwise."""
    c = cases.pair_case(37, 53)
    area, inter, status = hip.rle_pair_inter(c["strings"], c["pairs"], c["h"], c["w"])
    assert area.untyped_storage().data_ptr() == inter.untyped_storage().data_ptr() == status.untyped_storage().data_ptr()
    check_tables((area.cpu().numpy(), inter.cpu().numpy(), status.cpu().numpy()), c["want"], c)
    M, K = len(c["strings"]), len(c["pairs"])
    out = torch.full((4 * (M + K) + M,), 0xFF, dtype=torch.uint8, device="cuda")
    got = hip.rle_pair_inter(c["strings"], c["pairs"], c["h"], c["w"], area=out[:4 * M].view(torch.int32),
                             inter=out[4 * M:4 * (M + K)].view(torch.int32), status=out[4 * (M + K):])
    host = out.cpu().numpy()
    check_tables((host[:4 * M].view(np.int32), host[4 * M:4 * (M + K)].view(np.int32), host[4 * (M + K):]), c["want"], c)
    assert got[0].data_ptr() == out.data_ptr()
    with pytest.raises(ValueError, match="all of area, inter and status"):
        hip.rle_pair_inter(c["strings"], c["pairs"], c["h"], c["w"], area=out[:4 * M].view(torch.int32))


def test_rle_pair_inter_without_pairs_and_without_strings(hip):
    c = cases.pair_case(7, 5)
    area, inter, status = inter_guarded(hip, c["strings"], [], 7, 5, 0xFF)
    assert np.array_equal(area, c["want"][0]) and inter.size == 0 and np.array_equal(status, c["want"][2])
    area, inter, status = inter_guarded(hip, [], [], 7, 5, 0xFF)
    assert area.size == 0 and inter.size == 0 and status.size == 0
    a, i, s = hip.rle_pair_inter([], [], 7, 5)
    torch.cuda.synchronize()
    assert a.numel() == 0 and i.numel() == 0 and s.numel() == 0


def test_rle_pair_inter_seventy_thousand_pairs(hip):
    c = cases.many_pairs_case()
    got = inter_guarded(hip, c["strings"], c["pairs"], c["h"], c["w"], 0xFF)
    check_tables(got, c["want"])


def test_rle_pair_inter_more_strings_and_pairs_than_workgroups(hip):
    """4097 strings and 8193 pairs: the area kernel (4096 workgroups) and the pair kernel (8192) both serve their last element in a second
    trip through the workgroup loop, with the sum of the first trip still in LDS."""
    c = cases.many_strings_case()
    assert len(c["strings"]) == 4097 and len(c["pairs"]) == 8193 and c["pairs"][0] == (0, 4096) and c["pairs"][1] == (4096, 4096)
    area, inter, status = c["want"]
    assert (area[0], area[4096], inter[0], inter[1], inter[8192]) == (48, 40, 30, 40, 20) and status.any() and not status[[0, 3, 4096]].any()
    first = inter_guarded(hip, c["strings"], c["pairs"], c["h"], c["w"], 0xFF)
    check_tables(first, c["want"])
    second = inter_guarded(hip, c["strings"], c["pairs"], c["h"], c["w"], 0x00)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes(), "two runs, bit for bit"


# ------------------------------------------------------------------------------------------------ the evaluator
def equal_summaries(got, want):
    for key in FIGURES:
        assert got[key] == want[key], (key, got[key], want[key])                       # fp64, ==
    assert OrderedDict((int(k), v) for k, v in got["per_category"].items()) == OrderedDict((int(k), v) for k, v in want["per_category"].items())


def test_evaluator_equals_the_oracle_summary(hip):
    from stemseg_amd.evaluation import ytvis
    ev = ytvis.YtvisEvaluator()
    for fn in cases.VIDEOS:
        vid, results, truth, size, want, _ = cases.video(fn)
        rec = ev.add_video(vid, results, truth, size)
        assert list(rec) == list(want), vid
        for c in want:
            assert rec[c]["scores"] == want[c]["scores"] and rec[c]["n_gt"] == want[c]["n_gt"], (vid, c)
            assert rec[c]["matched"].reshape(10, -1).tolist() == np.asarray(want[c]["matched"]).reshape(10, -1).tolist(), (vid, c)
            assert rec[c]["ignored"].reshape(10, -1).tolist() == np.asarray(want[c]["ignored"]).reshape(10, -1).tolist(), (vid, c)
    got, want = ev.summary(), cases.oracle_summary()
    print("[ytvis eval] %s" % {k: got[k] for k in FIGURES})
    equal_summaries(got, want)
    assert got["counts"] == OrderedDict((("videos", 4), ("result_tracks", 19), ("gt_tracks", 9)))
    assert list(got) == list(FIGURES) + ["per_category", "counts"] and list(got["per_category"]) == [1, 2]
    assert 0.0 < got["AR1"] < got["AR10"] < 1.0
    # evaluate_results on the list of all results and a table of the ground truth: the same figures
    gt = OrderedDict((cases.video(fn)[0], {"size": cases.video(fn)[3], "length": 4 if cases.video(fn)[3] == (24, 40) else 3,
                                           "tracks": cases.video(fn)[2]}) for fn in cases.VIDEOS)
    everything = [tr for fn in cases.VIDEOS for tr in cases.video(fn)[1]]
    equal_summaries(ytvis.evaluate_results(everything, gt).summary(), want)
    with pytest.raises(KeyError, match="no video 'elsewhere'"):
        ytvis.evaluate_results([dict(everything[0], video_id="elsewhere")], gt)


def test_evaluator_errors_name_the_video_and_the_frame(hip):
    from stemseg_amd.evaluation import ytvis
    vid, results, truth, size, _, _ = cases.video(cases.video_other_size)
    bad = {name: s for name, s, _ in cases.do.malformed_cases(*size)}

    def with_string(tracks, n, t, value):
        out = [dict(tr, segmentations=list(tr["segmentations"])) for tr in tracks]
        out[n]["segmentations"][t] = value
        return out
    ev = ytvis.YtvisEvaluator()
    with pytest.raises(ValueError, match=r"video 'other-size', frame 2: the result mask of track 0 is refused: the counts do not sum"):
        ev.add_video(vid, with_string(results, 0, 2, {"size": list(size), "counts": bad["short_sum"]}), truth, size)
    with pytest.raises(ValueError, match=r"video 'other-size', frame 1: the ground-truth mask of track 1 is refused: a character outside"):
        ev.add_video(vid, results, with_string(truth, 1, 1, {"size": list(size), "counts": bad["bad_char_high"]}), size)
    with pytest.raises(ValueError, match=r"video 'other-size', frame 1: the result mask of track 2 is 24 x 40, the video 37 x 53"):
        ev.add_video(vid, with_string(results, 2, 1, {"size": [24, 40], "counts": oracle.mask_string(np.zeros((24, 40)))}), truth, size)
    with pytest.raises(ValueError, match=r"video 'other-size': tracks of \[2, 3\] frames"):
        ev.add_video(vid, results, [dict(truth[0], segmentations=truth[0]["segmentations"][:2])] + truth[1:], size)


def test_ground_truth_from_json_and_a_results_file(hip, tmp_path):
    from stemseg_amd.evaluation import ytvis
    recs = [cases.json_record(cases.video(fn)[0], cases.video(fn)[2], cases.video(fn)[3]) for fn in cases.VIDEOS if cases.video(fn)[2]]
    # (the video without ground truth has no record in the json, so its results stay out of the file as well)
    path = cases.write_json(str(tmp_path / "val.json"), recs)
    gt = ytvis.ground_truth_from_json(path)
    assert list(gt) == ["main", "gt-only", "other-size"] and gt["main"]["length"] == 4 and gt["other-size"]["size"] == (37, 53)
    assert [t["category_id"] for t in gt["main"]["tracks"]] == [1, 1, 2, 1, 1] and all(t["iscrowd"] == 0 for t in gt["main"]["tracks"])
    results = [tr for fn in cases.VIDEOS for tr in cases.video(fn)[1] if cases.video(fn)[2]]
    with open(str(tmp_path / "results.json"), "w") as fh:
        json.dump(results, fh)
    got = ytvis.evaluate_results(str(tmp_path / "results.json"), gt).summary()
    # the json knows no crowd: the oracle on the same tracks with iscrowd 0
    plain = OrderedDict()
    for fn in cases.VIDEOS:
        vid, res, truth, size, _, _ = cases.video(fn)
        if truth:
            plain[vid] = oracle.video_records(res, [dict(t, iscrowd=0) for t in truth], size)
    equal_summaries(got, oracle.summary(plain))
    assert got["AP"] != cases.oracle_summary()["AP"], "the crowd of 'main' counts as an object here"


# ------------------------------------------------------------------------------------------------ the inference driver
@pytest.fixture(scope="module")
def tiny_ytvis(tmp_path_factory, golden):
    """The small ytvis model of tests/test_gpu_parity.py's flow test (R-50, synthetic weights of seed 81, 96 x 128 inputs) over the
    14-frame sequence of 60 x 190 PNG files that tests/test_gpu_mots_eval.py's driver test uses, annotated with two tracks of two
    categories."""
    from PIL import Image
    from stemseg_amd import config
    from stemseg_amd.data.generic_video_dataset_parser import GenericVideoSequence
    from stemseg_amd.modeling.inference_model import InferenceModel
    from tests import synth
    root = tmp_path_factory.mktemp("tiny_ytvis")
    T, H, W = 14, 60, 190
    frames = synth.synth_frames(T, H, W, seed=91)
    os.makedirs(str(root / "0003"))
    for t, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(str(root / "0003" / ("%06d.png" % t)))
    truth = [cases.track(H, W, 1, [(5, 40, 10 + 3 * t, 70 + 3 * t) for t in range(T)]),
             cases.track(H, W, 2, [(20, 55, 120 + t, 150 + t) for t in range(T)])]
    record = cases.json_record("0003", truth, (H, W), image_paths=["0003/%06d.png" % t for t in range(T)])
    vds = cases.write_json(str(root / "val.json"), [record])
    try:
        config.load_preset("ytvis")
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 96, 320
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        config.cfg.CLUSTERING.MIN_SEEDINESS_PROB = float(golden("model_ytvis")["min_seed"])
        model = InferenceModel(None, semseg_output_type="logits", preload_images=True, resize_scale=1.0, semseg_generation_on_gpu=True)
        sd = model._model.state_dict()
        new = {k: torch.from_numpy(np.asarray(synth.synth_param(k, v.shape, 81))).reshape(v.shape) for k, v in sd.items()}
        new["embedding_head.conv_seediness.weight"] = new["embedding_head.conv_seediness.weight"] * 6.0
        model.load_checkpoint_state(new)
        model = model.cuda()
        yield NS(root=root, vds=vds, model=model, truth=truth, T=T, size=(H, W), sequence=lambda: GenericVideoSequence(record, str(root)))
    finally:
        config.load_preset("defaults")


def test_driver_writes_the_evaluation_and_leaves_the_results_alone(hip, tiny_ytvis):
    from stemseg_amd.evaluation import ytvis
    from stemseg_amd.inference import main
    d, said = tiny_ytvis, []
    common = [str(d.root / "model.pth"), "--dataset", "ytvis", "--frame_overlap", "4"]
    run = lambda extra: main.main(main.build_parser().parse_args(common + extra), model=d.model, sequences=[d.sequence()], print_fn=said.append)
    assert run(["-o", "plain"]) is None and not os.path.exists(str(d.root / "plain" / "ytvis_eval.json"))
    got = run(["-o", "scored", "--eval_ytvis_annotations", d.vds])
    a, b = open(str(d.root / "plain" / "results.json"), "rb").read(), open(str(d.root / "scored" / "results.json"), "rb").read()
    assert a == b, "the flag must not change a byte of the results"
    written = json.loads(a)
    assert len(written) > 0, "the model must find something, or the figures say nothing"
    on_disk = json.load(open(str(d.root / "scored" / "ytvis_eval.json")))
    print("[ytvis driver] %d result tracks, summary %s" % (len(written), {k: on_disk[k] for k in FIGURES}))
    assert on_disk == json.loads(json.dumps(got)) and any("AP50" in str(s) for s in said)
    gt = ytvis.ground_truth_from_json(d.vds)
    again = ytvis.evaluate_results(str(d.root / "scored" / "results.json"), gt).summary()
    assert json.loads(json.dumps(again)) == on_disk
    equal_summaries(on_disk, json.loads(json.dumps(oracle.evaluate({"0003": (written, d.truth, d.size)}))))
    assert on_disk["counts"] == {"videos": 1, "result_tracks": len(written), "gt_tracks": 2}
    # the synthetic model's categories need not be the annotated ones; scored against ITS OWN tracks as the ground truth, every
    # result with a pixel to its name is a true positive at every threshold
    own = cases.write_json(str(d.root / "own.json"), [cases.json_record("0003", written, d.size, image_paths=["0003/%06d.png" % t for t in range(d.T)])])
    perfect = run(["-o", "own", "--eval_ytvis_annotations", own])
    print("[ytvis driver] against its own tracks: %s" % {k: perfect[k] for k in FIGURES})
    assert perfect["AR10"] > 0.0 and perfect["AP50"] > 0.0 and perfect["counts"]["gt_tracks"] == len(written)
    for dataset in ("davis", "kittimots"):
        with pytest.raises(ValueError, match="--eval_ytvis_annotations.*ytvis.*%s" % dataset):
            main.main(main.build_parser().parse_args([str(d.root / "model.pth"), "--dataset", dataset, "--eval_ytvis_annotations", d.vds]),
                      model=d.model, sequences=[d.sequence()])


# ------------------------------------------------------------------------------------------------ the Trainer's validator
def test_validator_follows_the_trainers_weights(hip, tiny_ytvis, monkeypatch, tmp_path):
    """The figures of the tiny model before and after one SGD step: the five keys, values finite; the guard fires when the copy of the
    weights is skipped."""
    from stemseg_amd.evaluation import make_validator
    from stemseg_amd.modeling.inference_model import InferenceModel
    from stemseg_amd.modeling.model_builder import build_model
    import tempfile
    d = tiny_ytvis
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))                           # where the validator's directory comes and goes
    training = build_model(restore_pretrained_backbone_wts=False)
    training.load_state_dict(d.model._model.state_dict(), strict=False)
    training = training.cuda()
    trainer = NS(model=training, local_device=torch.device("cuda", torch.cuda.current_device()))
    validate = make_validator(d.vds, str(d.root), frame_overlap=4)
    with torch.no_grad():
        first = validate(trainer)
    assert list(first) == list(FIGURES) and all(np.isfinite(v) for v in first.values())
    scored = str(d.root / "scored" / "ytvis_eval.json")                               # the same weights through the driver
    if os.path.exists(scored):
        on_disk = json.load(open(scored))
        assert {k: on_disk[k] for k in FIGURES} == dict(first)
    opt = torch.optim.SGD(training.parameters(), lr=1.0)
    for p in training.parameters():
        if p.requires_grad:
            p.grad = 0.3 * p.detach()
    opt.step()
    with torch.no_grad():
        second = validate(trainer)
    assert list(second) == list(FIGURES) and all(np.isfinite(v) for v in second.values())
    assert not [n for n in os.listdir(str(tmp_path)) if n.startswith("ytvis_validation_")], "the temporary directory is removed"
    monkeypatch.setattr(InferenceModel, "load_checkpoint_state", lambda self, sd: None)
    with pytest.raises(RuntimeError, match="kept their version"):
        validate(trainer)
