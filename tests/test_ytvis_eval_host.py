"""Host tests of the YouTube-VIS evaluation: the measure's definition on hand-computed examples (tests/ytvis_eval_oracle.py, and the host
half of stemseg_amd/evaluation/ytvis.py fed the oracle's tables: the two must agree with ``==``), the argument checks of
``stemseg_hip_rle_pair_inter`` with no device call, the exports, the driver's flag, and -- on the oracle alone -- that the cases of
tests/test_gpu_ytvis_eval.py hold what they are named after."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

from tests import ytvis_eval_cases as cases
from tests import ytvis_eval_oracle as oracle

H, W, T = 12, 20, 2
FIGURES = ("AP", "AP50", "AP75", "AR1", "AR10")
# precision is TP / (TP + FP + spacing(1)) by definition, so a precision of "one" is 1 / (1 + 2^-52) = 1 - 2^-52, the second double
# below 1.0.  A mean of n such values is math.fsum (the exact sum, rounded once: relative 2^-53) divided by n (rounded once more:
# 2^-53), so it lies within 2^-52 + 2 * 2^-53 = 2^-51 of 1.0, and never above.  Recall carries no such term: a full recall is 1.0 exactly.
ONE_ULP = 2.0 ** -51


def res(category, box, score, video="v"):
    return cases.track(H, W, category, [box] * T, score, video=video)


def gt(category, box, iscrowd=None):
    return cases.track(H, W, category, [box] * T, iscrowd=iscrowd)


def both(videos):
    """{video: (results, ground truth)} -> (the oracle's summary, its records); the evaluator's host half on the oracle's tables must
    give the same records and the same figures, bit for bit."""
    from stemseg_amd.evaluation import ytvis
    want = OrderedDict((v, oracle.video_records(r, g, (H, W))) for v, (r, g) in videos.items())
    got = OrderedDict((v, ytvis.match_video(*oracle.video_tables(r, g, (H, W)))) for v, (r, g) in videos.items())
    equal_records(got, want)
    s_want, s_got = oracle.summary(want), ytvis.summarize(got)
    for key in FIGURES + ("per_category",):
        assert s_got[key] == s_want[key], key
    return s_want, want


def equal_records(got, want):
    assert list(got) == list(want)
    for v in want:
        assert list(got[v]) == list(want[v]), v
        for c in want[v]:
            a, b = got[v][c], want[v][c]
            assert a["scores"] == b["scores"] and a["n_gt"] == b["n_gt"] and a["n_crowd"] == b["n_crowd"], (v, c)
            assert np.asarray(a["matched"]).reshape(10, -1).tolist() == np.asarray(b["matched"]).reshape(10, -1).tolist(), (v, c)
            assert np.asarray(a["ignored"]).reshape(10, -1).tolist() == np.asarray(b["ignored"]).reshape(10, -1).tolist(), (v, c)


BOX, OTHER = (2, 8, 2, 12), (9, 12, 14, 20)


# ------------------------------------------------------------------------------------------------ the definition
def test_a_perfect_result_gives_one_everywhere():
    s, _ = both({"v": ([res(1, BOX, 0.9), res(2, OTHER, 0.8)], [gt(1, BOX), gt(2, OTHER)])})
    assert s["AR1"] == 1.0 and s["AR10"] == 1.0
    for key in ("AP", "AP50", "AP75"):
        assert 1.0 - ONE_ULP <= s[key] <= 1.0, (key, s[key])
    assert list(s["per_category"]) == [1, 2]


def test_a_true_positive_ahead_of_a_false_positive_and_the_reverse():
    """TP then FP: recall [1, 1], precision [1, 1/2], every recall point reads the first: AP 'one'.  FP then TP: recall [0, 1], precision
    [0, 1/2] -> envelope [1/2, 1/2]: AP exactly 0.5 (2 + 2^-52 rounds to 2)."""
    s, _ = both({"v": ([res(1, BOX, 0.9), res(1, OTHER, 0.5)], [gt(1, BOX)])})
    assert 1.0 - ONE_ULP <= s["AP"] <= 1.0 and s["AR1"] == 1.0
    s, rec = both({"v": ([res(1, BOX, 0.5), res(1, OTHER, 0.9)], [gt(1, BOX)])})
    assert s["AP"] == 0.5 and s["AP50"] == 0.5 and s["AP75"] == 0.5
    assert s["AR1"] == 0.0 and s["AR10"] == 1.0, "at maxDet 1 only the false positive is looked at"
    assert rec["v"][1]["scores"] == [0.9, 0.5] and rec["v"][1]["matched"][0] == [False, True]


def test_a_track_iou_of_exactly_one_half_matches_at_0_50_and_not_at_0_55():
    """d = 2 x 6 = 12 pixels per frame, g = 2 x 3 = 6 pixels inside d: I = 12, U = 24, 0.5 exactly."""
    s, rec = both({"v": ([res(1, (0, 2, 0, 6), 0.9)], [gt(1, (0, 2, 0, 3))])})
    assert [row[0] for row in rec["v"][1]["matched"]] == [True] + [False] * 9
    assert 1.0 - ONE_ULP <= s["AP50"] <= 1.0 and s["AP75"] == 0.0 and s["AR10"] == 0.1
    assert abs(s["AP"] - 0.1) <= ONE_ULP


def test_a_second_result_on_a_taken_ground_truth_is_a_false_positive():
    s, rec = both({"v": ([res(1, BOX, 0.9), res(1, BOX, 0.8)], [gt(1, BOX)])})
    assert all(row == [True, False] for row in rec["v"][1]["matched"]) and not np.asarray(rec["v"][1]["ignored"]).any()


def test_a_result_matched_to_a_crowd_is_ignored():
    """The result inside the crowd has the HIGHER score: as a false positive it would halve the precision."""
    crowd = (0, 12, 13, 20)
    s, rec = both({"v": ([res(1, (2, 6, 14, 18), 0.9), res(1, (3, 7, 15, 19), 0.85), res(1, BOX, 0.8)], [gt(1, BOX), gt(1, crowd, iscrowd=1)])})
    r = rec["v"][1]
    assert r["n_gt"] == 1 and r["n_crowd"] == 1
    assert all(row == [True, True, True] for row in r["matched"]), "a crowd may be taken again"
    assert all(row == [True, True, False] for row in r["ignored"])
    assert 1.0 - ONE_ULP <= s["AP"] <= 1.0 and s["AR1"] == 0.0 and s["AR10"] == 1.0
    # a crowd alone: no ground truth that counts
    s, _ = both({"v": ([res(1, (2, 6, 14, 18), 0.9)], [gt(1, crowd, iscrowd=1)])})
    assert all(s[k] == -1.0 for k in FIGURES)


def test_a_non_crowd_match_is_not_traded_for_a_crowd_one():
    """The result lies inside the crowd (crowd IoU = I / area_d = 1.0) and covers 5 of the 6 rows of g (IoU 5 / 6): up to 0.8 it takes
    g, although the crowd's IoU is higher."""
    s, rec = both({"v": ([res(1, (2, 7, 2, 12), 0.9)], [gt(1, (2, 8, 2, 12)), gt(1, (0, 12, 0, 20), iscrowd=1)])})
    r = rec["v"][1]
    assert [row[0] for row in r["matched"]] == [True] * 10, "above 5 / 6 the crowd is what is left"
    assert [row[0] for row in r["ignored"]] == [False] * 7 + [True] * 3
    assert s["AR10"] == 0.7


def test_ar1_is_below_ar10_with_two_objects():
    s, _ = both({"v": ([res(1, BOX, 0.9), res(1, OTHER, 0.8)], [gt(1, BOX), gt(1, OTHER)])})
    assert s["AR1"] == 0.5 and s["AR10"] == 1.0


def test_no_ground_truth_gives_minus_one():
    s, _ = both({"v": ([res(1, BOX, 0.9)], [])})
    assert all(s[k] == -1.0 for k in FIGURES) and s["per_category"] == OrderedDict()
    s, _ = both({})
    assert all(s[k] == -1.0 for k in FIGURES)
    # a category without ground truth is left out of the means, it does not pull them down
    s, _ = both({"v": ([res(1, BOX, 0.9), res(2, OTHER, 0.95)], [gt(1, BOX)])})
    assert list(s["per_category"]) == [1] and s["AR1"] == 1.0


def test_results_of_two_videos_are_merged_by_score():
    """Video a holds the false positive with the higher score, video b the true positive: precision 1/2 at both objects' recall."""
    s, _ = both(OrderedDict((("a", ([res(1, OTHER, 0.9, "a")], [])), ("b", ([res(1, BOX, 0.8, "b")], [gt(1, BOX)])))))
    assert s["AP"] == 0.5 and s["AR1"] == 1.0


# ------------------------------------------------------------------------------------------------ the evaluator's host half
def test_host_half_on_the_oracles_tables_equals_the_oracle_summary():
    from stemseg_amd.evaluation import ytvis
    got = OrderedDict()
    for fn in cases.VIDEOS:
        vid, results, truth, size, want, _ = cases.video(fn)
        got[vid] = ytvis.match_video(*oracle.video_tables(results, truth, size))
        equal_records({vid: got[vid]}, {vid: want})
    s_got, s_want = ytvis.summarize(got), cases.oracle_summary()
    for key in FIGURES + ("per_category",):
        assert s_got[key] == s_want[key], key                                           # fp64, ==
    assert list(s_got)[:5] == list(FIGURES) and list(s_got)[5:] == ["per_category", "counts"]
    assert np.array_equal(ytvis.IOU_THRESHOLDS, np.linspace(0.5, 0.95, 10)) and np.array_equal(ytvis.RECALL_THRESHOLDS, np.linspace(0, 1, 101))
    assert ytvis.MAX_DETS == (1, 10, 100)


# ------------------------------------------------------------------------------------------------ the C ABI, no device call
def test_argument_errors_and_exports():
    from stemseg_amd import evaluation, hip
    from stemseg_amd.evaluation import ytvis
    lib = hip.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stemseg_hip.h")).read()
    for n in ("stemseg_hip_rle_pair_inter", "stemseg_hip_rle_pair_inter_workspace_bytes"):
        assert hasattr(lib, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert lib.stemseg_hip_version() == hip.ABI_VERSION == 11 and "#define STEMSEG_HIP_ABI_VERSION 11" in header
    assert callable(hip.rle_pair_inter) and callable(hip.rle_pair_inter_workspace_bytes)
    for name in ("YtvisEvaluator", "ground_truth_from_json", "evaluate_results", "make_validator"):
        assert getattr(evaluation, name) is getattr(ytvis, name), name
    ws = lib.stemseg_hip_rle_pair_inter_workspace_bytes
    assert ws(100, 3, 2) > 0 and ws(0, 0, 0) > 0 and ws(-1, 1, 1) == 0 and ws(1 << 30, 1, 1) == 0 and ws(10, -1, 0) == 0 and ws(10, 1, -1) == 0
    assert ws(100, 3, 2) == ws(100, 3, 70000), "the workspace holds nothing per pair"
    assert ws(100, 3, 2) == hip.rle_pair_inter_workspace_bytes(100, 3, 2)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any HIP call
    offs = (C.c_int64 * 3)(0, 4, 9)
    prs = (C.c_int32 * 4)(0, 1, 1, 1)

    def call(chars=fake, n=9, offsets_host=offs, pairs_host=prs, offsets=fake, pairs=fake, M=2, K=2, H=7, W=5, wsp=fake, ws_bytes=1 << 30,
             area=fake, inter=fake, status=fake):
        return lib.stemseg_hip_rle_pair_inter(chars, n, offsets_host, pairs_host, offsets, pairs, M, K, H, W, wsp, ws_bytes, area, inter, status, None)
    for kw, word in ((dict(K=-1), "bad dims"), (dict(M=-1), "bad dims"), (dict(H=0), "bad dims"), (dict(W=0), "bad dims"),
                     (dict(H=65536, W=32768), "2^31"), (dict(n=-1), "n_chars"), (dict(n=1 << 30), "n_chars"),
                     (dict(chars=None), "null"), (dict(offsets_host=None), "null"), (dict(offsets=None), "null"), (dict(pairs_host=None), "null"),
                     (dict(pairs=None), "null"), (dict(wsp=None), "null"), (dict(area=None), "null"), (dict(inter=None), "null"),
                     (dict(status=None), "null"),
                     (dict(offsets=C.c_void_p(0x1004)), "8-byte aligned"), (dict(pairs=C.c_void_p(0x1002)), "misaligned"),
                     (dict(area=C.c_void_p(0x1001)), "misaligned"), (dict(inter=C.c_void_p(0x1002)), "misaligned"),
                     (dict(offsets_host=(C.c_int64 * 3)(0, 4, 8)), "offsets must run"), (dict(offsets_host=(C.c_int64 * 3)(1, 4, 9)), "offsets must run"),
                     (dict(offsets_host=(C.c_int64 * 3)(0, 10, 9)), "decrease"),
                     (dict(pairs_host=(C.c_int32 * 4)(0, 1, 2, 1)), "pair 1 names strings (2, 1) of 2"),
                     (dict(pairs_host=(C.c_int32 * 4)(0, -1, 1, 1)), "pair 0 names strings (0, -1) of 2"),
                     (dict(M=0, n=0, offsets_host=(C.c_int64 * 1)(0), K=1), "pair 0 names strings (0, 1) of 0"),
                     (dict(ws_bytes=16), "workspace"), (dict(ws_bytes=ws(9, 2, 2) - 1), "workspace")):
        assert call(**kw) == -1, kw
        assert word in lib.stemseg_hip_last_error().decode() and "rle_pair_inter" in lib.stemseg_hip_last_error().decode(), (kw, lib.stemseg_hip_last_error())
    # the binding refuses a pair outside the strings before it asks for a device
    with pytest.raises(ValueError, match=r"pair 1 names strings \(0, 2\) of 2"):
        hip.rle_pair_inter(["5", "5"], [(0, 1), (0, 2)], 1, 5)
    with pytest.raises(ValueError, match=r"pair 0 names strings \(-1, 0\) of 1"):
        hip.rle_pair_inter(["5"], [(-1, 0)], 1, 5)


# ------------------------------------------------------------------------------------------------ the driver's flag
@pytest.mark.parametrize("dataset", ["davis", "kittimots"])
def test_eval_ytvis_annotations_is_refused_for_other_datasets(dataset, tmp_path):
    from stemseg_amd.inference import main
    args = main.build_parser().parse_args(["model.pth", "--dataset", dataset, "--eval_ytvis_annotations", str(tmp_path / "val.json")])
    with pytest.raises(ValueError, match="--eval_ytvis_annotations.*ytvis.*%s" % dataset):
        main.main(args)
    plain = main.build_parser().parse_args(["model.pth", "--dataset", "ytvis"])
    assert plain.eval_ytvis_annotations is None and plain.eval_mots_annotations is None and plain.eval_annotations is None


def test_ground_truth_from_json_host(tmp_path):
    """(the reader touches no device)"""
    from stemseg_amd.evaluation import ytvis
    vid, _, truth, size, _, _ = cases.video(cases.video_main)
    ids = [7, 3, 12, 5, 9]                                                              # not ascending: the reader orders them
    path = cases.write_json(str(tmp_path / "val.json"), [cases.json_record(vid, truth, size, ids=ids),
                                                         {"id": "bare", "height": 4, "width": 4, "image_paths": ["a.jpg"]}])
    table = ytvis.ground_truth_from_json(path)
    assert list(table) == [vid] and table[vid]["size"] == size and table[vid]["length"] == 4
    tracks = table[vid]["tracks"]
    assert [t["instance_id"] for t in tracks] == sorted(ids) and all(t["iscrowd"] == 0 for t in tracks)
    for t in tracks:
        src = truth[ids.index(t["instance_id"])]
        assert t["category_id"] == src["category_id"] and t["segmentations"] == src["segmentations"]
    assert [t for t in tracks if t["instance_id"] == 12][0]["segmentations"][1] is None, "a frame without the instance"


# ------------------------------------------------------------------------------------------------ the validity of the GPU cases
def test_pair_cases_hold_what_they_are_named_after():
    for h, w in cases.PAIR_SHAPES:
        c = cases.pair_case(h, w)
        area, inter, status = c["want"]
        idx, grp, strings, hw = c["index"], c["group"], c["strings"], h * w
        counts = lambda name: cases.wo.string_to_counts(strings[idx[name]])
        assert counts("zeros") == [hw] and counts("ones") == [0, hw] and counts("first-count-0")[0] == 0
        assert 0 in counts("zero-length-zero-run")[1:-1] and 0 in counts("zero-length-one-run")[1:-1]
        assert area[idx["zeros"]] == 0 and area[idx["ones"]] == hw and area[idx["zero-length-zero-run"]] == 6 and area[idx["zero-length-one-run"]] == 9
        for name in ("corner-tl", "corner-tr", "corner-bl", "corner-br"):
            assert area[idx[name]] == 1
        assert sorted(int(status[idx["refused-" + n]]) for n in cases.STATUS_CASES) == [1, 2, 4, 8, 16]
        refused = set(idx["refused-" + n] for n in cases.STATUS_CASES)
        assert not status[[m for m in range(len(strings)) if m not in refused]].any() and not area[sorted(refused)].any()
        for k in grp["self"]:
            a, b = c["pairs"][k]
            assert a == b and inter[k] == area[a]
        assert all(inter[k] == area[idx["same-a"]] > 0 for k in grp["identical"])
        assert all(inter[k] == 0 for k in grp["disjoint-extents"]) and area[idx["left"]] > 0 and area[idx["right"]] > 0
        assert all(inter[k] == 1 for k in grp["touching-extents"])
        assert all(inter[k] == 0 for k in grp["board-vs-shifted"]) and area[idx["board"]] + area[idx["board-shifted"]] == min(64, h) * min(64, w)
        assert all(inter[k] > 0 for k in grp["long-vs-board"]) and all(inter[k] > 0 for k in grp["stripes"])
        assert all(inter[k] == 0 for k in grp["refused"]) and len(grp["refused"]) == 16
        rep = [inter[k] for k in grp["repeated"]]
        assert rep[0::2] == [rep[0]] * 3 and rep[1::2] == [rep[1]] * 3 and rep[1] > 0
        assert len(c["pairs"]) > 100 and any(len(set(p)) == 2 and inter[k] > 0 for k, p in enumerate(c["pairs"]))
    big = cases.pair_case(130, 200)
    lens = sorted(len(cases.wo.string_to_counts(s)) for s, st in zip(big["strings"], big["want"][2]) if st == 0)
    assert lens[-1] > 8000 and len(cases.wo.string_to_counts(big["strings"][big["index"]["board"]])) > 4000, "thousands of runs"
    assert len(big["strings"][big["index"]["long-run-and-more"]]) > len(big["strings"][big["index"]["board"]]) > len(big["strings"][big["index"]["long-run"]])
    assert {len(g) for s in big["strings"] for g in _groups(s)} >= {1, 2, 3, 4}, "counts of one to four characters"
    many = cases.many_pairs_case()
    assert len(many["pairs"]) == 70000 > 65535 and many["want"][2].tolist() == [0, 0, 0, 0, 0, 1] and many["want"][1].max() > 0


def _groups(s):
    out, cur = [], ""
    for ch in s:
        cur += ch
        if not (ord(ch) - 48) & 0x20:
            out.append(cur)
            cur = ""
    return out


def test_evaluator_videos_hold_what_they_are_named_after():
    thresholds = np.linspace(0.5, 0.95, 10)
    sizes, cats = set(), set()
    for fn in cases.VIDEOS:
        vid, results, truth, size, rec, notes = cases.video(fn)
        sizes.add(size)
        cats |= set(rec)
        for c, d, g, inter, union, iou in notes:                                        # no decision sits on a threshold
            assert np.abs(thresholds - iou).min() > 1e-9, (vid, c, d, g, inter, union)
    assert len(sizes) == 2 and cats == {1, 2, 3}
    vid, results, truth, size, rec, notes = cases.video(cases.video_main)
    r = rec[1]
    assert len(r["scores"]) == 12 and r["n_gt"] == 3 and r["n_crowd"] == 1 and rec[3]["n_gt"] == 0 and len(rec[3]["scores"]) == 1
    assert r["scores"][1] == r["scores"][2] and r["scores"][5] == r["scores"][6], "equal scores keep the file's order"
    tp = [m and not i for m, i in zip(r["matched"][0], r["ignored"][0])]
    assert tp == [True, True] + [False] * 9 + [True], "one true positive within maxDet 1, two within 10, three within 100"
    assert r["ignored"][0] == [False, False, False, True] + [False] * 8 and all(row[3] for row in r["ignored"])
    assert sum(1 for m in r["matched"][0] if not m) == 8, "eight false positives at 0.5"
    assert not r["matched"][0][2], "the second, looser hit on a taken ground truth"
    assert any(seg is None for tr in truth for seg in tr["segmentations"]) and any(seg is None for tr in results for seg in tr["segmentations"])
    # the ground-truth tracks g0 and g1 overlap, and so do the results r0 and r2
    h, w = size
    g0, g1 = oracle.track_masks(truth[0], h, w), oracle.track_masks(truth[1], h, w)
    r0, r2 = oracle.track_masks(results[0], h, w), oracle.track_masks(results[2], h, w)
    assert (g0[0] & g1[0]).any() and (r0[0] & r2[0]).any()
    assert cases.video(cases.video_results_only)[2] == [] and cases.video(cases.video_gt_only)[1] == []
    s = cases.oracle_summary()
    assert 0.0 < s["AR1"] < s["AR10"] < 1.0 and 0.0 < s["AP75"] < s["AP"] < s["AP50"] < 1.0 and list(s["per_category"]) == [1, 2]
