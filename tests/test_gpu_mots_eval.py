"""GPU tests of the KITTI-MOTS evaluation: ``stemseg_hip_rle_decode_labels`` (csrc/data_loader.hip) and ``stemseg_hip_label_pair_counts``
(csrc/mots_eval.hip) against the numpy oracle (tests/mots_eval_oracle.py) with exact integer equality on the cases of
tests/mots_eval_cases.py, the outputs between canaries over garbage, two runs bit for bit; ``MotsEvaluator`` with ``==`` in fp64 against
the oracle's summary; the inference driver's ``--eval_mots_annotations``; ``make_validator`` before and after an SGD step.  Agreement of
the measure with the official mots_tools is not tested: they are not available here."""
import ctypes as C
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import mots_eval_cases as cases
from tests import mots_eval_oracle as oracle

pytestmark = pytest.mark.gpu
GUARD = 4096
CANARY = 0xA5


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

    def read(self, dtype):
        assert bool((self.buf[:GUARD] == CANARY).all()) and bool((self.buf[GUARD + self.n:] == CANARY).all()), "a canary around an output was overwritten"
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().view(dtype)


# ------------------------------------------------------------------------------------------------ rle_decode_labels
def decode_guarded(hip, strings, planes, labels, P, h, w, fill):
    """The C call with maps, overlap and status between canaries, over payloads that hold ``fill`` bytes before."""
    chars, offsets, pidx = hip.rle_pack(strings, planes)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    M, n = len(strings), int(chars.size)
    lib = hip.lib()
    nbytes = lib.stemseg_hip_rle_decode_labels_workspace_bytes(n, M, P)
    assert nbytes > 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() if a.size else torch.zeros(1, dtype=torch.uint8, device="cuda")
    d_chars, d_offs, d_pidx, d_lab = dev(chars), dev(offsets), dev(pidx), dev(lab)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    maps, overlap, status = Guarded(2 * P * h * w, fill), Guarded(4 * P, fill), Guarded(max(M, 1), fill)
    at = lambda t: C.c_void_p(t.data_ptr())
    host = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.stemseg_hip_rle_decode_labels(at(d_chars) if n else None, n, host(offsets), host(pidx) if M else None, host(lab) if M else None,
                                           at(d_offs), at(d_pidx) if M else None, at(d_lab) if M else None, M, P, h, w, at(ws), nbytes, maps.ptr,
                                           overlap.ptr, status.ptr if M else None, hip.stream())
    assert rc == 0, lib.stemseg_hip_last_error().decode()
    torch.cuda.synchronize()
    return maps.read(np.uint16).reshape(P, h, w), overlap.read(np.int32), status.read(np.uint8)[:M]


@pytest.mark.parametrize("shape", cases.LABEL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_rle_decode_labels_equals_the_oracle(hip, shape):
    """Every plane of the composite case (tests/mots_eval_cases.py: nobody, disjoint, two and three overlapping, all ones and all zeros,
    one refused string of each status among accepted ones, 70 strings, nobody), exactly; a second run over other garbage gives the same
    bits; the binding gives the same; on the disjoint plane ``maps == label`` is ``hip.rle_decode``'s plane of that string."""
    c = cases.label_case(*shape)
    h, w, P = c["h"], c["w"], c["P"]
    want_maps, want_overlap, want_status = c["want"]
    got = decode_guarded(hip, c["strings"], c["planes"], c["labels"], P, h, w, 0x5A)
    for q, name in enumerate(cases.PLANES):
        bad = np.argwhere(got[0][q] != want_maps[q])
        assert bad.size == 0, "%s: %d pixels differ, first (y, x, got, oracle) %s" % (
            name, len(bad), [(int(y), int(x), int(got[0][q, y, x]), int(want_maps[q, y, x])) for y, x in bad[:4]])
    assert got[1].tolist() == want_overlap.tolist() and got[2].tolist() == want_status.tolist()
    again = decode_guarded(hip, c["strings"], c["planes"], c["labels"], P, h, w, 0xC3)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))
    maps, overlap, status = hip.rle_decode_labels(c["strings"], c["planes"], c["labels"], P, h, w)
    assert maps.is_cuda and tuple(maps.shape) == (P, h, w) and overlap.dtype == torch.int32 and status.dtype == torch.uint8
    assert np.array_equal(maps.cpu().numpy().view(np.uint16), want_maps) and overlap.cpu().tolist() == want_overlap.tolist()
    assert status.cpu().tolist() == want_status.tolist()
    disjoint = [m for m, q in enumerate(c["planes"]) if q == 1]
    planes, st = hip.rle_decode([c["strings"][m] for m in disjoint], list(range(len(disjoint))), len(disjoint), h, w)
    assert not st.cpu().numpy().any()
    for k, m in enumerate(disjoint):
        assert np.array_equal(planes[k].cpu().numpy() != 0, got[0][1] == c["labels"][m]), m


def test_rle_decode_labels_more_planes_than_grid_rows(hip):
    """1025 planes of 24 x 25, two or three overlapping rectangles on planes 0, 1, 1023 and 1024 (tests/data_oracle.py): the rasteriser's
    workgroups of plane 0 come back for plane 1024, whose overlap is another number -- a sum that stayed over from plane 0 would show.
    Every map, the overlap and the status, twice."""
    from tests import data_oracle as do
    strings, planes, labels, P, h, w = do.strided_planes_case()
    want_maps, want_overlap, want_status = oracle.decode_labels(strings, planes, labels, P, h, w)
    assert np.flatnonzero(want_overlap).tolist() == [0, 1, 1023, 1024] and want_overlap[0] != want_overlap[1024] and not want_status.any()
    got = decode_guarded(hip, strings, planes, labels, P, h, w, 0x5A)
    assert np.array_equal(got[0], want_maps), "maps %s differ" % np.flatnonzero((got[0] != want_maps).reshape(P, -1).any(1)).tolist()
    assert got[1].tolist() == want_overlap.tolist() and got[2].tolist() == want_status.tolist()
    again = decode_guarded(hip, strings, planes, labels, P, h, w, 0xC3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "two runs, bit for bit"


def test_rle_decode_labels_without_strings(hip):
    maps, overlap, status = decode_guarded(hip, [], [], [], 3, 7, 5, 0x5A)
    assert not maps.any() and overlap.tolist() == [0, 0, 0] and status.size == 0
    maps, overlap, status = hip.rle_decode_labels([], [], [], 2, 1, 40)
    assert not maps.cpu().numpy().view(np.uint16).any() and overlap.cpu().tolist() == [0, 0] and status.numel() == 0


# ------------------------------------------------------------------------------------------------ label_pair_counts
def pair_guarded(hip, a, b, Ka, Kb, fill):
    T, H, W = a.shape
    need = int(hip.lib().stemseg_hip_label_pair_counts_size(T, Ka, Kb))
    assert need == T * (Ka + 1) * (Kb + 1)
    out = Guarded(4 * need, fill)
    da, db = torch.from_numpy(a.view(np.int16).copy()).cuda(), torch.from_numpy(b.view(np.int16).copy()).cuda()
    rc = hip.lib().stemseg_hip_label_pair_counts(C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), T, H, W, Ka, Kb, out.ptr, need, hip.stream())
    assert rc == 0, hip.lib().stemseg_hip_last_error().decode()
    torch.cuda.synchronize()
    return out.read(np.int32).reshape(T, Ka + 1, Kb + 1).astype(np.int64)


@pytest.mark.parametrize("name", list(cases.PAIR_CASES))
def test_label_pair_counts_equals_the_oracle(hip, name):
    """Every cell, exactly; the tables lie between canaries and start out holding garbage; a second run over other garbage gives the
    same bits; every frame's table sums to H * W; every frame alone gives its own table (no frame reads another)."""
    a, b, Ka, Kb, want = cases.pair_case(name)
    got = pair_guarded(hip, a, b, Ka, Kb, 0x5A)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d cells differ, first (t, i, j, got, oracle) %s" % (
        name, len(bad), [tuple(int(v) for v in i) + (int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:4]])
    assert (got.reshape(a.shape[0], -1).sum(1) == a.shape[1] * a.shape[2]).all()
    assert np.array_equal(pair_guarded(hip, a, b, Ka, Kb, 0xC3), got)
    for t in range(min(a.shape[0], 3)):
        assert np.array_equal(pair_guarded(hip, a[t:t + 1], b[t:t + 1], Ka, Kb, 0x5A)[0], got[t]), t
    view = hip.label_pair_counts(torch.from_numpy(a.view(np.int16).copy()).cuda(), torch.from_numpy(b.view(np.int16).copy()).cuda(), Ka, Kb)
    assert view.dtype == torch.int32 and tuple(view.shape) == want.shape and np.array_equal(view.cpu().numpy(), want)


def test_label_pair_counts_wrapper_limits(hip):
    a = torch.zeros((2, 8, 9), dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError, match="limit is 63"):
        hip.label_pair_counts(a, a, 64, 1)
    with pytest.raises(ValueError, match="int32 vector of at least"):
        hip.label_pair_counts(a, a, 2, 2, counts=torch.zeros(17, dtype=torch.int32, device="cuda"))
    full = torch.full((40,), 7, dtype=torch.int32, device="cuda")
    view = hip.label_pair_counts(a, a, 2, 2, counts=full)
    assert view.data_ptr() == full.data_ptr() and view.cpu().tolist() == [[[72, 0, 0], [0, 0, 0], [0, 0, 0]]] * 2 and full[18:].cpu().tolist() == [7] * 22


# ------------------------------------------------------------------------------------------------ the evaluator
def equal_summaries(got, want):
    for key, value in want.items():
        assert got[key] == value, (key, got[key], value)                            # integers and fp64, ==


def test_evaluator_equals_the_oracle_summary(hip):
    from stemseg_amd.evaluation.mots import MotsEvaluator
    ev, ref = MotsEvaluator(), {}
    for fn in cases.SEQUENCES:
        name, res, gt, T, h, w, want, _ = cases.sequence(fn)
        counts = ev.add_sequence(name, res, gt, T)
        ref[name] = want
        for cls in ("car", "ped"):
            assert {k: counts[cls][k] for k in oracle.KEYS} == {k: want[cls][k] for k in oracle.KEYS}, (name, cls)
            assert sorted(counts[cls]["ious"]) == sorted(want[cls]["ious"]), (name, cls)
    got = ev.summary()
    equal_summaries(got, oracle.summary(ref))
    assert list(got)[:7] == ["sMOTSA-car", "MOTSA-car", "MOTSP-car", "sMOTSA-ped", "MOTSA-ped", "MOTSP-ped", "sMOTSA-mean"]
    assert list(got["sequences"]) == ["0002", "0006", "0013"] and got["counts"]["car"]["IDS"] >= 1 and got["counts"]["ped"]["ignored"] >= 1
    json.dumps(got)
    # n_frames left out: the largest frame named + 1, here the same
    ev2 = MotsEvaluator()
    for fn in cases.SEQUENCES:
        name, res, gt = cases.sequence(fn)[:3]
        ev2.add_sequence(name, res, gt)
    assert ev2.summary() == got
    assert MotsEvaluator().add_sequence("nothing", [], [])["car"]["M"] == 0


def test_evaluator_carries_the_last_match_across_chunk_seams(hip, monkeypatch):
    from stemseg_amd.evaluation import mots
    name, res, gt, T, h, w, want, _ = cases.sequence(cases.seq_long)
    calls = []
    real = mots.hip.label_pair_counts
    monkeypatch.setattr(mots, "CHUNK_FRAMES", 4)
    monkeypatch.setattr(mots.hip, "label_pair_counts", lambda a, *args, **kw: calls.append(int(a.shape[0])) or real(a, *args, **kw))
    ev = mots.MotsEvaluator()
    ev.add_sequence(name, res, gt, T)
    assert calls == [4, 4, 3], "three chunks, one counting call each"
    got = ev.summary()
    equal_summaries(got, oracle.summary({name: want}))
    assert got["counts"]["car"]["IDS"] == 1 and got["counts"]["ped"]["IDS"] == 1
    monkeypatch.setattr(mots, "CHUNK_FRAMES", 128)
    whole = mots.MotsEvaluator()
    whole.add_sequence(name, res, gt, T)
    assert whole.summary() == got


def test_evaluator_errors_name_the_sequence_and_the_frame(hip):
    from stemseg_amd.evaluation.mots import MotsEvaluator
    name, res, gt, T, h, w = cases.sequence(cases.seq_a)[:6]
    over = gt + cases.records([(3, 1009, 1, (10, 14, 8, 20))], h, w)                 # on top of gt 1001 in frame 3
    with pytest.raises(ValueError, match=r"'0002', frame 3: the ground-truth masks overlap in \d+ pixels"):
        MotsEvaluator().add_sequence(name, res, over, T)
    over = res + cases.records([(4, 77, 2, (30, 36, 8, 14))], h, w)                  # on top of result 7 in frame 4
    with pytest.raises(ValueError, match="'0002', frame 4: the result masks overlap"):
        MotsEvaluator().add_sequence(name, over, gt, T)
    refused = res[:5] + [(2, 55, 1, h, w, "!!")] + res[5:]
    with pytest.raises(ValueError, match="'0002', frame 2: the result mask of track 55 is refused: a character outside"):
        MotsEvaluator().add_sequence(name, refused, gt, T)
    many = cases.records([(1, 3000 + k, 2, (k // 30, k // 30 + 1, 2 * (k % 30), 2 * (k % 30) + 1)) for k in range(64)], h, w)
    with pytest.raises(ValueError, match="'0002', frame 1: 64 result masks, the limit is 63"):
        MotsEvaluator().add_sequence(name, many, gt, T)
    ok = MotsEvaluator().add_sequence(name, many[:63], [r for r in gt if r[0] == 1 and r[2] == 10], T)          # 63 are fine
    assert ok["ped"]["FP"] == 63
    other = res + [(1, 99, 1, h + 1, w, res[0][5])]
    with pytest.raises(ValueError, match=r"'0002', frame 1: the result record of track 99 is 41 x 60, the sequence 40 x 60"):
        MotsEvaluator().add_sequence(name, other, gt, T)
    with pytest.raises(ValueError, match="names frame 6 of 6"):
        MotsEvaluator().add_sequence(name, res + [(6,) + res[0][1:]], gt, T)


def test_txt_and_json_ground_truth_give_equal_summaries(hip, tmp_path):
    from stemseg_amd.evaluation import mots
    os.makedirs(str(tmp_path / "gt"))
    os.makedirs(str(tmp_path / "res"))
    recs = []
    for fn in cases.SEQUENCES:
        name, res, gt, T, h, w = cases.sequence(fn)[:6]
        cases.write_txt(str(tmp_path / "gt" / (name + ".txt")), gt)
        cases.write_txt(str(tmp_path / "res" / (name + ".txt")), res)
        recs.append(cases.json_record(name, gt, T, h, w))
    vds = cases.write_json(str(tmp_path / "val.json"), recs)
    a = mots.evaluate_results(str(tmp_path / "res"), mots.ground_truth(vds)).summary()
    b = mots.evaluate_results(str(tmp_path / "res"), mots.ground_truth(str(tmp_path / "gt"))).summary()
    assert a == b
    equal_summaries(a, oracle.summary({cases.sequence(fn)[0]: cases.sequence(fn)[6] for fn in cases.SEQUENCES}))
    only = mots.evaluate_results(str(tmp_path / "res"), mots.ground_truth(vds), seqs=[6, 13]).summary()
    assert list(only["sequences"]) == ["0006", "0013"]
    os.remove(str(tmp_path / "gt" / "0013.txt"))
    with pytest.raises(KeyError, match="0013"):
        mots.evaluate_results(str(tmp_path / "res"), mots.ground_truth(str(tmp_path / "gt")))


# ------------------------------------------------------------------------------------------------ the inference driver
@pytest.fixture(scope="module")
def tiny_kitti(tmp_path_factory, golden):
    """The small kittimots model of tests/test_gpu_parity.py's flow test (R-50, synthetic weights of seed 91, 96 x 320 inputs) over one
    14-frame sequence of 60 x 190 PNG files, annotated with a car, a pedestrian and an ignore region."""
    from PIL import Image
    from stemseg_amd import config
    from stemseg_amd.data.generic_video_dataset_parser import GenericVideoSequence
    from stemseg_amd.modeling.inference_model import InferenceModel
    from tests import synth
    root = tmp_path_factory.mktemp("tiny_kitti")
    T, H, W = 14, 60, 190
    frames = synth.synth_frames(T, H, W, seed=91)
    os.makedirs(str(root / "0003"))
    for t, f in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(str(root / "0003" / ("%06d.png" % t)))
    gt = []
    for t in range(T):
        gt += [(t, 1001, 1, (5, 40, 10 + 3 * t, 70 + 3 * t)), (t, 2001, 2, (20, 55, 120 + t, 150 + t)), (t, 10000, 10, (0, 15, 150, 190))]
    gt = cases.records(gt, H, W)
    record = cases.json_record("0003", gt, T, H, W)
    vds = cases.write_json(str(root / "val.json"), [record])
    os.makedirs(str(root / "instances_txt"))
    cases.write_txt(str(root / "instances_txt" / "0003.txt"), gt)
    try:
        config.load_preset("kittimots")
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 96, 320
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        config.cfg.CLUSTERING.MIN_SEEDINESS_PROB = float(golden("model_kitti")["min_seed"])
        model = InferenceModel(None, semseg_output_type="argmax", preload_images=False, resize_scale=1.0, semseg_generation_on_gpu=True)
        sd = model._model.state_dict()
        new = {k: torch.from_numpy(np.asarray(synth.synth_param(k, v.shape, 91))).reshape(v.shape) for k, v in sd.items()}
        new["embedding_head.conv_seediness.weight"] = new["embedding_head.conv_seediness.weight"] * 6.0
        model.load_checkpoint_state(new)
        model = model.cuda()
        yield NS(root=root, vds=vds, txt_dir=str(root / "instances_txt"), model=model, gt=gt, T=T,
                 sequence=lambda: GenericVideoSequence(record, str(root)))
    finally:
        config.load_preset("defaults")


def _files(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


def test_driver_writes_the_evaluation_and_leaves_the_results_alone(hip, tiny_kitti):
    from stemseg_amd.evaluation import mots
    from stemseg_amd.inference import main
    d, said = tiny_kitti, []
    common = [str(d.root / "model.pth"), "--dataset", "kittimots", "--frame_overlap", "4"]
    run = lambda extra: main.main(main.build_parser().parse_args(common + extra), model=d.model, sequences=[d.sequence()], print_fn=said.append)
    assert run(["-o", "plain"]) is None and not os.path.exists(str(d.root / "plain" / "mots_eval.json"))
    got = run(["-o", "scored", "--eval_mots_annotations", d.vds])
    for sub in ("results", "results_nms"):
        a, b = _files(str(d.root / "plain" / sub)), _files(str(d.root / "scored" / sub))
        assert list(a) == ["0003.txt"] and a == b, "the flag must not change a byte of the results"
    assert len(_files(str(d.root / "scored" / "results"))["0003.txt"]) > 0
    print("[mots driver] results %d lines, results_nms %d lines, summary %s" % (
        len(open(str(d.root / "scored" / "results" / "0003.txt")).readlines()),
        len(open(str(d.root / "scored" / "results_nms" / "0003.txt")).readlines()), {k: v for k, v in got.items() if k != "sequences"}))
    on_disk = json.load(open(str(d.root / "scored" / "mots_eval.json")))
    assert on_disk == json.loads(json.dumps(got)) and any("sMOTSA-car" in str(s) for s in said)
    # an evaluator fed the written files, and the oracle on the same records
    records = mots.parse_mots_txt(str(d.root / "scored" / "results_nms" / "0003.txt"))
    assert len(records) > 0, "the track filters must leave something, or the figures say nothing"
    ev = mots.MotsEvaluator()
    ev.add_sequence("0003", records, d.gt, d.T)
    assert json.loads(json.dumps(ev.summary())) == on_disk
    equal_summaries(on_disk, json.loads(json.dumps(oracle.summary({"0003": oracle.sequence_counts(records, d.gt, d.T)}))))
    assert on_disk["counts"]["car"]["M"] == d.T and on_disk["counts"]["ped"]["M"] == d.T
    # the directory of txt files as ground truth: the same figures
    from_txt = run(["-o", "scored_txt", "--eval_mots_annotations", d.txt_dir])
    assert json.loads(json.dumps(from_txt)) == on_disk
    with pytest.raises(ValueError, match="--eval_mots_annotations.*kittimots.*davis"):
        main.main(main.build_parser().parse_args([str(d.root / "model.pth"), "--dataset", "davis", "--eval_mots_annotations", d.vds]), model=d.model,
                  sequences=[d.sequence()])


# ------------------------------------------------------------------------------------------------ the Trainer's validator
def test_validator_follows_the_trainers_weights(hip, tiny_kitti, monkeypatch, tmp_path):
    """The figures of the tiny model before and after one SGD step: keys present, values finite; the guard fires when the copy of the
    weights is skipped."""
    from stemseg_amd.evaluation.mots import make_validator
    from stemseg_amd.modeling.inference_model import InferenceModel
    from stemseg_amd.modeling.model_builder import build_model
    import tempfile
    d = tiny_kitti
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))                           # where the validator's directory comes and goes
    training = build_model(restore_pretrained_backbone_wts=False)
    training.load_state_dict(d.model._model.state_dict(), strict=False)
    training = training.cuda()
    trainer = NS(model=training, local_device=torch.device("cuda", torch.cuda.current_device()))
    validate = make_validator(d.vds, str(d.root), frame_overlap=4)
    keys = ["sMOTSA-car", "MOTSA-car", "MOTSP-car", "sMOTSA-ped", "MOTSA-ped", "MOTSP-ped", "sMOTSA-mean"]
    with torch.no_grad():
        first = validate(trainer)
    assert list(first) == keys and all(np.isfinite(v) for v in first.values())
    # the same weights through the driver gave mots_eval.json's figures
    scored = str(d.root / "scored" / "mots_eval.json")
    if os.path.exists(scored):
        on_disk = json.load(open(scored))
        assert {k: on_disk[k] for k in keys} == dict(first)
    opt = torch.optim.SGD(training.parameters(), lr=1.0)
    for p in training.parameters():
        if p.requires_grad:
            p.grad = 0.3 * p.detach()
    opt.step()
    with torch.no_grad():
        second = validate(trainer)
    assert list(second) == keys and all(np.isfinite(v) for v in second.values())
    assert not [n for n in os.listdir(str(tmp_path)) if n.startswith("mots_validation_")], "the temporary directory is removed"
    monkeypatch.setattr(InferenceModel, "load_checkpoint_state", lambda self, sd: None)
    with pytest.raises(RuntimeError, match="kept their version"):
        validate(trainer)
