"""Host tests of the KITTI-MOTS evaluation: the measure's definition on hand-computed examples (tests/mots_eval_oracle.py), the host half
of stemseg_amd/evaluation/mots.py fed the oracle's tables, the argument checks of ``stemseg_hip_rle_decode_labels`` and
``stemseg_hip_label_pair_counts`` with no device call, the driver's flag, and -- on the oracle alone -- that the cases of
tests/test_gpu_mots_eval.py hold what they are named after."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mots_eval_cases as cases
from tests import mots_eval_oracle as oracle

H, W = 12, 20


def one_frame(res, gt, T=1):
    """res / gt: [(frame, track, class, box)] on a 12 x 20 frame -> the oracle's counts."""
    return oracle.sequence_counts(cases.records(res, H, W), cases.records(gt, H, W), T)


def ints(c):
    return {k: v for k, v in c.items() if k != "ious"}


# ------------------------------------------------------------------------------------------------ the definition
def test_iou_of_exactly_one_half_is_no_match_and_one_pixel_more_is():
    """h = 2 x 6 = 12 pixels, g = 2 x 3 = 6 pixels inside h: inter 6, union 12, IoU exactly 0.5; 3 * 6 = 18 = 12 + 6: no match.
    g = 2 x 3 plus one more pixel of h (a second record cannot be, so g is 1 x 7 inside a 1 x 13 h): inter 7, areas 13 and 7:
    3 * 7 = 21 > 20: a match by one."""
    c = one_frame([(0, 1, 1, (0, 2, 0, 6))], [(0, 1001, 1, (0, 2, 0, 3))])["car"]
    assert ints(c) == {"TP": 0, "FP": 1, "FN": 1, "IDS": 0, "M": 1, "ignored": 0} and c["ious"] == []
    c = one_frame([(0, 1, 1, (0, 1, 0, 13))], [(0, 1001, 1, (0, 1, 0, 7))])["car"]
    assert ints(c) == {"TP": 1, "FP": 0, "FN": 0, "IDS": 0, "M": 1, "ignored": 0} and c["ious"] == [7.0 / 13.0]
    c = one_frame([(0, 1, 1, (0, 1, 0, 14))], [(0, 1001, 1, (0, 1, 0, 7))])["car"]          # 21 = 14 + 7: the threshold itself
    assert c["TP"] == 0


def test_ignore_share_of_exactly_one_half_is_an_fp_and_one_pixel_more_is_ignored():
    ignore = (0, 10000, 10, (0, 1, 0, 10))
    c = one_frame([(0, 1, 2, (0, 1, 5, 15))], [ignore])["ped"]                       # 5 of 10 pixels ignored
    assert ints(c) == {"TP": 0, "FP": 1, "FN": 0, "IDS": 0, "M": 0, "ignored": 0}
    c = one_frame([(0, 1, 2, (0, 1, 4, 15))], [ignore])["ped"]                       # 6 of 11
    assert ints(c) == {"TP": 0, "FP": 0, "FN": 0, "IDS": 0, "M": 0, "ignored": 1}
    # a MATCHED result is never looked up in the ignore region
    c = one_frame([(0, 1, 2, (0, 1, 4, 15))], [ignore, (0, 2001, 2, (1, 2, 0, 3))])["ped"]
    assert c["ignored"] == 1 and c["FN"] == 1


def test_id_switch_across_a_gap_and_none_on_the_same_id():
    box = (2, 6, 2, 8)
    gt = [(t, 1001, 1, box) for t in range(6)]
    c = one_frame([(0, 7, 1, box), (4, 8, 1, box)], gt, 6)["car"]                    # frames 1-3 unmatched, then another id
    assert ints(c) == {"TP": 2, "FP": 0, "FN": 4, "IDS": 1, "M": 6, "ignored": 0}
    c = one_frame([(0, 7, 1, box), (4, 7, 1, box), (5, 7, 1, box)], gt, 6)["car"]    # the same id again: no switch
    assert ints(c) == {"TP": 3, "FP": 0, "FN": 3, "IDS": 0, "M": 6, "ignored": 0}
    c = one_frame([(0, 7, 1, box), (1, 8, 1, box), (2, 7, 1, box)], gt, 6)["car"]    # there and back: two switches
    assert c["IDS"] == 2
    # the first match of a track is no switch, whatever other tracks were matched to
    c = one_frame([(0, 7, 1, box), (1, 8, 1, (8, 11, 10, 16))], gt + [(1, 1002, 1, (8, 11, 10, 16))], 6)["car"]
    assert c["IDS"] == 0 and c["TP"] == 2


def test_figures_zero_denominators_and_left_out_classes():
    box = (2, 6, 2, 8)
    seq = one_frame([(0, 1, 2, box), (0, 2, 3, (7, 11, 2, 8)), (0, 3, 10, (7, 11, 10, 18)), (0, 4, 1, None)], [(0, 2001, 2, box), (0, 1009, 1, None)])
    assert ints(seq["car"]) == {"TP": 0, "FP": 0, "FN": 0, "IDS": 0, "M": 0, "ignored": 0}          # zero-area masks are dropped on both sides
    assert ints(seq["ped"]) == {"TP": 1, "FP": 0, "FN": 0, "IDS": 0, "M": 1, "ignored": 0}          # classes 3 and 10 of the result are left out
    s = oracle.summary({"s": seq})
    assert (s["sMOTSA-car"], s["MOTSA-car"], s["MOTSP-car"]) == (0.0, 0.0, 0.0)
    assert (s["sMOTSA-ped"], s["MOTSA-ped"], s["MOTSP-ped"]) == (1.0, 1.0, 1.0)
    assert s["sMOTSA-mean"] == 1.0, "a class with M = 0 stays out of the mean"
    assert oracle.summary({})["sMOTSA-mean"] == 0.0


def test_figures_by_hand():
    """cars: TP 2 with IoU 7/13 and 1, FP 1, IDS 1, M 4."""
    seq = {"car": {"TP": 2, "FP": 1, "FN": 2, "IDS": 1, "M": 4, "ignored": 0, "ious": [7.0 / 13.0, 1.0]},
           "ped": {"TP": 0, "FP": 3, "FN": 2, "IDS": 0, "M": 2, "ignored": 0, "ious": []}}
    s = oracle.summary({"s": seq})
    assert s["sMOTSA-car"] == (7.0 / 13.0 + 1.0 - 1 - 1) / 4.0 and s["MOTSA-car"] == 0.0 and s["MOTSP-car"] == (7.0 / 13.0 + 1.0) / 2.0
    assert s["sMOTSA-ped"] == -1.5 and s["MOTSA-ped"] == -1.5 and s["MOTSP-ped"] == 0.0
    assert s["sMOTSA-mean"] == (s["sMOTSA-car"] + s["sMOTSA-ped"]) / 2.0


# ------------------------------------------------------------------------------------------------ the evaluator's host half
@pytest.mark.parametrize("fn", cases.SEQUENCES + (cases.seq_long,), ids=lambda f: f.__name__)
def test_host_half_on_the_oracles_tables(fn):
    from stemseg_amd.evaluation import mots
    name, res, gt, T, h, w, want, _ = cases.sequence(fn)
    counts, last = mots.new_counts(), {}
    for table, res_meta, gt_meta in oracle.frame_tables(res, gt, T):
        assert int(table.sum()) == h * w
        mots.accumulate_frame(counts, last, table, res_meta, gt_meta)
    for cls in ("car", "ped"):
        assert ints(counts[cls]) == ints(want[cls]), cls
        assert sorted(counts[cls]["ious"]) == sorted(want[cls]["ious"]), cls
    got, ref = mots.summarize({name: counts}), oracle.summary({name: want})
    for key, value in ref.items():
        assert got[key] == value, key                                                 # fp64, ==
    assert list(got)[:7] == ["sMOTSA-car", "MOTSA-car", "MOTSP-car", "sMOTSA-ped", "MOTSA-ped", "MOTSP-ped", "sMOTSA-mean"]


def test_parse_mots_txt_and_records_from_json_agree(tmp_path):
    from stemseg_amd.evaluation import mots
    name, res, gt, T, h, w, _, _ = cases.sequence(cases.seq_a)
    cases.write_txt(str(tmp_path / "0002.txt"), gt)
    assert mots.parse_mots_txt(str(tmp_path / "0002.txt")) == gt
    from_json = mots.records_from_json(cases.json_record(name, gt, T, h, w))
    assert sorted(from_json) == sorted(gt) and any(r[2] == 10 for r in from_json)
    path = cases.write_json(str(tmp_path / "val.json"), [cases.json_record(name, gt, T, h, w)])
    table = mots.ground_truth(path)
    assert list(table) == [2] and table[2][1] == T and sorted(table[2][0]) == sorted(gt)
    assert list(mots.ground_truth(str(tmp_path))) == [2] and mots.ground_truth(str(tmp_path))[2] == (gt, None)
    (tmp_path / "bad.txt").write_text("0 1 1 5 5\n")
    with pytest.raises(ValueError, match="line 1"):
        mots.parse_mots_txt(str(tmp_path / "bad.txt"))
    assert mots.CHUNK_FRAMES == 128


# ------------------------------------------------------------------------------------------------ the C ABI, no device call
def test_argument_errors_and_exports():
    from stemseg_amd import hip
    lib = hip.lib()
    names = ("stemseg_hip_rle_decode_labels", "stemseg_hip_rle_decode_labels_workspace_bytes", "stemseg_hip_label_pair_counts",
             "stemseg_hip_label_pair_counts_size")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stemseg_hip.h")).read()
    for n in names:
        assert hasattr(lib, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert lib.stemseg_hip_version() == hip.ABI_VERSION == 11 and "#define STEMSEG_HIP_ABI_VERSION 11" in header
    assert "#define STEMSEG_LABEL_PAIR_MAX_LABELS 63" in header and hip.LABEL_PAIR_MAX_LABELS == 63
    assert callable(hip.rle_decode_labels) and callable(hip.label_pair_counts)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any HIP call
    size = lib.stemseg_hip_label_pair_counts_size
    assert size(5, 20, 10) == 5 * 21 * 11 and size(1, 63, 63) == 4096 and size(70, 1, 63) == 70 * 2 * 64
    assert size(0, 1, 1) == 0 and size(1, 0, 1) == 0 and size(1, 1, 0) == 0 and size(1, 64, 1) == 0 and size(1, 1, 64) == 0

    def pair(a=fake, b=fake, T=5, H=37, W=53, Ka=20, Kb=10, counts=fake, n=1 << 30):
        return lib.stemseg_hip_label_pair_counts(a, b, T, H, W, Ka, Kb, counts, n, None)
    for kw, word in ((dict(a=None), "null"), (dict(b=None), "null"), (dict(counts=None), "null"), (dict(T=0), "bad dims"), (dict(H=0), "bad dims"),
                     (dict(W=0), "bad dims"), (dict(H=65536, W=32768), "2^31"), (dict(Ka=0), "limit is 63"), (dict(Ka=64), "limit is 63"),
                     (dict(Kb=0), "limit is 63"), (dict(Kb=64), "limit is 63"), (dict(a=C.c_void_p(0x1001)), "misaligned"),
                     (dict(b=C.c_void_p(0x1001)), "misaligned"), (dict(counts=C.c_void_p(0x1002)), "misaligned"), (dict(n=5 * 21 * 11 - 1), "int32")):
        assert pair(**kw) == -1, kw
        assert word in lib.stemseg_hip_last_error().decode() and "label_pair_counts" in lib.stemseg_hip_last_error().decode(), kw

    ws = lib.stemseg_hip_rle_decode_labels_workspace_bytes
    assert ws(100, 3, 2) == lib.stemseg_hip_rle_decode_union_workspace_bytes(100, 3, 2) > 0 and ws(-1, 1, 1) == 0 and ws(10, 1, 0) == 0
    offs = (C.c_int64 * 3)(0, 4, 9)
    planes, labels = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(1, 65535)

    def decode(chars=fake, n=9, offsets_host=offs, planes_host=planes, labels_host=labels, offsets=fake, plane_dev=fake, label_dev=fake, M=2, P=2,
               H=7, W=5, wsp=fake, ws_bytes=1 << 30, maps=fake, overlap=fake, status=fake):
        return lib.stemseg_hip_rle_decode_labels(chars, n, offsets_host, planes_host, labels_host, offsets, plane_dev, label_dev, M, P, H, W, wsp,
                                                 ws_bytes, maps, overlap, status, None)
    for kw, word in ((dict(labels_host=(C.c_int32 * 2)(1, 0)), "label 0"), (dict(labels_host=(C.c_int32 * 2)(65536, 1)), "label 65536"),
                     (dict(labels_host=(C.c_int32 * 2)(-3, 1)), "label -3"), (dict(maps=C.c_void_p(0x1001)), "misaligned"),
                     (dict(overlap=C.c_void_p(0x1002)), "misaligned"), (dict(label_dev=C.c_void_p(0x1002)), "aligned"),
                     (dict(maps=None), "null"), (dict(overlap=None), "null"), (dict(labels_host=None), "null"), (dict(label_dev=None), "null"),
                     (dict(planes_host=(C.c_int32 * 2)(1, 0)), "decrease"), (dict(planes_host=(C.c_int32 * 2)(0, 2)), "names plane 2"),
                     (dict(H=65536, W=32768), "2^31"), (dict(P=0), "bad dims"), (dict(offsets_host=(C.c_int64 * 3)(0, 4, 8)), "offsets must run"),
                     (dict(offsets=C.c_void_p(0x1004)), "aligned"), (dict(ws_bytes=16), "workspace")):
        assert decode(**kw) == -1, kw
        assert word in lib.stemseg_hip_last_error().decode() and "rle_decode_labels" in lib.stemseg_hip_last_error().decode(), kw
    # the bindings refuse what does not go together before they ask for a device
    a = torch.zeros((3, 8, 9), dtype=torch.int16)
    for x, y, word in ((a, a[:2], "do not go together"), (a[0], a[0], "do not go together"), (a.float(), a, "16-bit"), (a, a.to(torch.uint8), "16-bit")):
        with pytest.raises(ValueError, match=word):
            hip.label_pair_counts(x, y, 2, 2)
    with pytest.raises(ValueError, match="label 0"):
        hip.rle_decode_labels(["5"], [0], [0], 1, 1, 5)
    with pytest.raises(ValueError, match="decrease"):
        hip.rle_decode_labels(["5", "5"], [1, 0], [1, 2], 2, 1, 5)
    with pytest.raises(ValueError, match="2 strings, 2 plane indices, 1 labels"):
        hip.rle_decode_labels(["5", "5"], [0, 1], [1], 2, 1, 5)


# ------------------------------------------------------------------------------------------------ the driver's flag
@pytest.mark.parametrize("dataset", ["davis", "ytvis"])
def test_eval_mots_annotations_is_refused_for_other_datasets(dataset, tmp_path):
    from stemseg_amd.inference import main
    args = main.build_parser().parse_args(["model.pth", "--dataset", dataset, "--eval_mots_annotations", str(tmp_path / "val.json")])
    with pytest.raises(ValueError, match="--eval_mots_annotations.*kittimots.*%s" % dataset):
        main.main(args)
    plain = main.build_parser().parse_args(["model.pth", "--dataset", "kittimots"])
    assert plain.eval_mots_annotations is None and plain.eval_annotations is None


# ------------------------------------------------------------------------------------------------ the validity of the GPU cases
def test_evaluator_sequences_hold_every_count_for_both_classes():
    total = {cls: {k: 0 for k in oracle.KEYS} for cls in ("car", "ped")}
    ious, names = [], []
    for fn in cases.SEQUENCES:
        name, res, gt, T, h, w, counts, notes = cases.sequence(fn)
        names.append(name)
        for cls in total:
            for k in oracle.KEYS:
                total[cls][k] += counts[cls][k]
            ious += counts[cls]["ious"]
        # no decision of any sequence sits on a threshold: the cases that do are the hand-computed ones above
        for t, c, kind, x, ah, ag in notes:
            assert (3 * x != ah + ag) if kind == "pair" else (2 * x != ah), (name, t, c, kind, x, ah, ag)
    assert len(set(names)) == 3
    for cls in total:
        assert all(total[cls][k] >= 1 for k in ("TP", "FP", "FN", "IDS", "ignored")), (cls, total[cls])
        assert total[cls]["TP"] + total[cls]["FN"] == total[cls]["M"]
    assert any(v < 1.0 for v in ious) and any(v == 1.0 for v in ious)
    assert cases.sequence(cases.seq_c)[6]["car"]["M"] == 0 and len({cases.sequence(f)[4:6] for f in cases.SEQUENCES}) == 3          # three frame sizes
    # the long sequence: one switch per class, and none if the state were dropped at a chunk seam
    name, res, gt, T, h, w, counts, notes = cases.sequence(cases.seq_long)
    assert T == 11 and counts["car"]["IDS"] == 1 and counts["ped"]["IDS"] == 1
    for seam in (4, 8):
        head = oracle.sequence_counts([r for r in res if r[0] < seam], [r for r in gt if r[0] < seam], seam)
        tail = oracle.sequence_counts([(r[0] - seam,) + r[1:] for r in res if r[0] >= seam], [(r[0] - seam,) + r[1:] for r in gt if r[0] >= seam], T - seam)
        assert head["car"]["IDS"] + tail["car"]["IDS"] == 0 and head["ped"]["IDS"] + tail["ped"]["IDS"] == 0, seam


def test_label_cases_hold_what_they_are_named_after():
    for h, w in cases.LABEL_SHAPES:
        c = cases.label_case(h, w)
        maps, overlap, status = c["want"]
        planes, labels, masks = np.asarray(c["planes"]), np.asarray(c["labels"]), c["masks"]
        assert c["P"] == 8 and (np.diff(planes) >= 0).all() and set(planes.tolist()) == {1, 2, 3, 4, 5, 6}          # planes 0 and 7: nobody
        assert not maps[0].any() and not maps[7].any() and overlap[0] == 0 and overlap[7] == 0
        assert overlap[1] == 0 and {1, 65535} <= set(labels[planes == 1].tolist())
        for m in np.flatnonzero(planes == 1):
            assert np.array_equal(maps[1] == labels[m], masks[m]), (h, w, m)
        two = [m for m in np.flatnonzero(planes == 2)]
        both = masks[two[0]] & masks[two[1]]
        assert both.any() and overlap[2] == int(both.sum()) and labels[two[0]] > labels[two[1]] and (maps[2][both] == labels[two[0]]).all()
        three = [masks[m] for m in np.flatnonzero(planes == 3)]
        cover = three[0].astype(int) + three[1] + three[2]
        assert (cover == 3).any() and (cover == 2).any() and overlap[3] == int((cover > 1).sum()) and (maps[3][cover == 3] == 600).all()
        assert (maps[4] == 7).all() and overlap[4] == 0                                # all ones under label 7, all zeros under label 9
        refused = [m for m in np.flatnonzero(planes == 5) if masks[m] is None]
        assert sorted(int(status[m]) for m in refused) == [1, 2, 4, 8, 16] and not status[[m for m in range(len(masks)) if masks[m] is not None]].any()
        assert not (maps[5] == 65535).any() and (maps[5] > 0).all() and overlap[5] == 0
        assert int((planes == 6).sum()) == 70 and maps[6].any()
        assert (overlap[6] > 0) == (h * w < 700)


def test_pair_cases_hold_what_they_are_named_after():
    seen_T, seen_hw = set(), set()
    for name in cases.PAIR_CASES:
        a, b, Ka, Kb, want = cases.pair_case(name)
        seen_T.add(a.shape[0]); seen_hw.add(a.shape[1:])
        assert (want.reshape(a.shape[0], -1).sum(1) == a.shape[1] * a.shape[2]).all(), name
    assert seen_T == {1, 2, 3, 70} and {(5, 7), (37, 53), (130, 200), (70, 70)} <= seen_hw and 130 * 200 > 8192 * 3
    a, b, Ka, Kb, want = cases.pair_case("70x70 K63 every cell")
    assert (Ka, Kb) == (63, 63) and want.shape == (1, 64, 64) and (want > 0).all()
    a, b, Ka, Kb, want = cases.pair_case("130x200 T3 uniform frames")
    assert want[1, 0, 0] == 26000 and want[2, 2, 3] == 26000 and int((want[1] > 0).sum()) == 1 and int((want[2] > 0).sum()) == 1
    assert int((want[0] > 0).sum()) > 20
    a, b, Ka, Kb, want = cases.pair_case("37x53 T3 labels above K")
    assert (a > Ka).any() and (b > Kb).any() and int(b.max()) == 65535
    clean_a, clean_b = np.where(a > Ka, 0, a), np.where(b > Kb, 0, b)
    assert np.array_equal(oracle.pair_counts(clean_a, clean_b, Ka, Kb), want), "labels above K count as background"
    assert cases.pair_case("Ka1 Kb63")[4].shape == (3, 2, 64) and cases.pair_case("Ka63 Kb1")[4].shape == (3, 64, 2)
    assert np.array_equal(cases.pair_case("Ka1 Kb63")[4], cases.pair_case("Ka63 Kb1")[4].transpose(0, 2, 1))
    a, b, Ka, Kb, want = cases.pair_case("two uniform frames")
    assert want[0, 3, 1] == 37 * 53 and want[1, 1, 2] == 37 * 53 and int((want > 0).sum()) == 2
    assert cases.pair_case("5x7 T1")[0].size < 64, "a frame smaller than a wave"
