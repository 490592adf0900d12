"""Host tests of the DAVIS evaluation: the measure's definition on hand-computed examples (tests/davis_eval_oracle.py and the host half of
stemseg_amd/evaluation/davis.py), the argument checks of ``stemseg_hip_davis_eval_counts`` with no device call, the driver's flag, the
Trainer's validation hook, and -- on the oracle alone -- that the cases of tests/test_gpu_davis_eval.py hold what they are named after."""
import ctypes as C
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import davis_eval_cases as cases
from tests import davis_eval_oracle as oracle


# ------------------------------------------------------------------------------------------------ the definition
def test_boundary_of_the_pinned_4x4_example():
    m = np.zeros((4, 4), np.uint8)
    m[1:3, 1:3] = 1
    want = np.array([[1, 1, 1, 0], [1, 0, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]], bool)
    assert np.array_equal(oracle.boundary(m), want)
    full = np.ones((3, 5), np.uint8)                    # a mask that fills the image has no boundary: the clamped neighbours are itself
    assert not oracle.boundary(full).any()
    last = np.zeros((3, 3), np.uint8)
    last[2, 2] = 1                                      # the bottom-right pixel never is one; its west, north and north-west neighbours are
    assert np.array_equal(oracle.boundary(last), np.array([[0, 0, 0], [0, 1, 1], [0, 1, 0]], bool))


def test_two_squares_one_and_two_pixels_apart_at_radius_1():
    """p = rows 1-2 x columns 1-2.  Its boundary is the ring rows 0-2 x columns 0-2 without (1, 1): 8 pixels.
    g one column to the right: its ring is rows 0-2 x columns 1-3 without (1, 2).  Column 1 of g's ring is whole, so every pixel of p's
    column 0 has its east neighbour on it, p's columns 1 and 2 lie on g's ring or next to its column 1: m_p = 8, and by symmetry m_g = 8.
    g two columns to the right: its ring is rows 0-2 x columns 2-4 without (1, 3).  p's column 0 is 2 away from it: 3 pixels unmatched;
    (0, 1) and (2, 1) have their east neighbours on it, column 2 lies on it: m_p = 5, and by symmetry m_g = 5."""
    for shift, inter, matched in ((1, 2, 8), (2, 0, 5)):
        pred, gt = np.zeros((1, 5, 7), np.uint8), np.zeros((1, 1, 5, 7), np.uint8)
        pred[0, 1:3, 1:3] = 1
        gt[0, 0, 1:3, 1 + shift:3 + shift] = 1
        tab = oracle.counts(pred, gt, 1, 1)
        got = {k: int(v.reshape(-1)[0]) for k, v in tab.items()}
        assert got == {"inter": inter, "m_p": matched, "m_g": matched, "area_p": 4, "n_p": 8, "area_g": 4, "n_g": 8}, shift
    assert oracle.jaccard(2, 4, 4) == 2.0 / 6.0
    assert oracle.f_measure(8, 8, 5, 5) == 2.0 * (5.0 / 8.0) * (5.0 / 8.0) / (5.0 / 8.0 + 5.0 / 8.0) == 0.625


def test_disk_membership_at_radius_5():
    d = oracle.disk(5)
    at = lambda dx, dy: bool(d[dy + 5, dx + 5])
    assert at(5, 0) and at(3, 4) and at(0, -5) and at(-4, 3)
    assert not at(4, 4) and not at(5, 1) and not at(-1, 5)
    assert d.shape == (11, 11) and int(d.sum()) == 81


def test_precision_recall_special_cases_and_empty_union():
    from stemseg_amd.evaluation.davis import measures_from_counts
    assert oracle.precision_recall(4, 8, 2, 6) == (0.5, 0.75)
    assert oracle.precision_recall(0, 8, 0, 0) == (1.0, 0.0) and oracle.f_measure(0, 8, 0, 0) == 0.0
    assert oracle.precision_recall(4, 0, 0, 0) == (0.0, 1.0) and oracle.f_measure(4, 0, 0, 0) == 0.0
    assert oracle.precision_recall(0, 0, 0, 0) == (1.0, 1.0) and oracle.f_measure(0, 0, 0, 0) == 1.0
    assert oracle.f_from_pr(0.0, 0.0) == 0.0 and oracle.f_measure(4, 8, 0, 0) == 0.0          # P + R = 0 with both boundaries present
    assert oracle.jaccard(0, 0, 0) == 1.0 and oracle.jaccard(0, 3, 0) == 0.0 and oracle.jaccard(3, 3, 3) == 1.0
    # the evaluator's vectorised form on the same rows: frames = the cases, one proposal, one object
    rows = [(4, 8, 2, 6, 3, 5, 9), (0, 8, 0, 0, 0, 0, 7), (4, 0, 0, 0, 0, 6, 0), (0, 0, 0, 0, 0, 0, 0), (4, 8, 0, 0, 0, 2, 2)]
    tab = {k: np.array([r[i] for r in rows], np.int64).reshape((-1, 1, 1) if k in ("m_p", "m_g", "inter") else (-1, 1))
           for i, k in enumerate(("n_p", "n_g", "m_p", "m_g", "inter", "area_p", "area_g"))}
    J, F = measures_from_counts(tab)
    assert F[:, 0, 0].tolist() == [oracle.f_measure(*r[:4]) for r in rows] == [0.6, 0.0, 0.0, 1.0, 0.0]
    assert J[:, 0, 0].tolist() == [oracle.jaccard(r[4], r[5], r[6]) for r in rows] == [3.0 / 11.0, 0.0, 0.0, 1.0, 0.0]


def test_decay_bins_against_hand_written_lists():
    from stemseg_amd.evaluation import davis
    hand = {4: [(0, 1), (1, 2), (2, 2), (2, 3)],               # linspace 1, 1.75, 2.5, 3.25, 4 -> 1, 2, 3, 3, 4 (2.5 + 1e-10 rounds up)
            5: [(0, 1), (1, 2), (2, 3), (3, 4)],               # 1, 2, 3, 4, 5
            10: [(0, 2), (2, 5), (5, 7), (7, 9)],              # 1, 3.25, 5.5, 7.75, 10 -> 1, 3, 6, 8, 10
            67: [(0, 17), (17, 33), (33, 50), (50, 66)]}       # 1, 17.5, 34, 50.5, 67 -> 1, 18, 34, 51, 67
    for n, bins in hand.items():
        assert oracle.decay_bins(n) == bins and davis.decay_bins(n) == bins, n
    v = np.arange(10, dtype=np.float64) / 10.0                 # decay = mean(0, .1, .2) - mean(.7, .8, .9)
    for stats in (oracle.frame_stats, davis.frame_stats):
        mean, recall, decay = stats(v)
        assert mean == float(np.mean(v)) and recall == 0.4 and decay == float(np.mean(v[0:3])) - float(np.mean(v[7:10]))


def _tables(T, Kp, Kg):
    return {k: np.zeros(s, np.int64) for k, s in zip(oracle.TABLES, [(T, Kp, Kg)] * 3 + [(T, Kp)] * 2 + [(T, Kg)] * 2)}


def test_frame_trimming_and_the_three_frame_minimum():
    from stemseg_amd.evaluation import davis
    assert oracle.counted_frames(3) == [1] and oracle.counted_frames(6) == [1, 2, 3, 4]
    for T in (0, 1, 2):
        with pytest.raises(ValueError, match="at least 3"):
            oracle.counted_frames(T)
        with pytest.raises(ValueError, match="at least 3"):
            davis.sequence_statistics(_tables(T, 1, 1), 1, 1)
    # a perfect first and last frame, nothing in between: the trimmed mean is 0
    tab = _tables(4, 1, 1)
    for t in (0, 3):
        for k in ("inter", "area_p", "area_g", "n_p", "n_g", "m_p", "m_g"):
            tab[k][t] = 5
    for t in (1, 2):
        tab["area_p"][t], tab["area_g"][t], tab["n_p"][t], tab["n_g"][t] = 5, 5, 4, 4
    for stats in (oracle.sequence_stats(tab, 1, 1), davis.sequence_statistics(tab, 1, 1)):
        assert stats["objects"][0]["J-Mean"] == 0.0 and stats["objects"][0]["F-Mean"] == 0.0
        assert np.asarray(stats["J"]).shape == (1, 2)


def _tables_from_scores(S):
    """Tables of T = 3 whose one counted frame gives the pair (p, g) the figures J = s / (200 - s) and F = s / 100, s = S[p][g]: areas and
    boundary counts of 100 each, intersection and matches of s."""
    J = S
    Kp, Kg = len(J), len(J[0])
    tab = _tables(3, Kp, Kg)
    tab["n_p"][1], tab["n_g"][1] = 100, 100
    tab["area_p"][1], tab["area_g"][1] = 100, 100
    for p in range(Kp):
        for g in range(Kg):
            tab["m_p"][1, p, g] = tab["m_g"][1, p, g] = J[p][g]          # F = J[p][g] / 100
            tab["inter"][1, p, g] = J[p][g]                              # J = s / (200 - s)
    return tab


def test_association_with_more_and_with_fewer_proposals_than_objects():
    from stemseg_amd.evaluation import davis
    pair = lambda s: (s / (200.0 - s) + s / 100.0) / 2.0
    # three proposals, two objects; pair scores at least 0.05 apart: the best total is p2 -> g0 (90) and p0 -> g1 (80), p1 is left over
    more = [[40, 80], [30, 20], [90, 70]]
    vals = sorted(pair(float(s)) for row in more for s in row)
    assert min(b - a for a, b in zip(vals, vals[1:])) >= 0.05
    for stats in (oracle.sequence_stats(_tables_from_scores(more), 3, 2), davis.sequence_statistics(_tables_from_scores(more), 3, 2)):
        assert stats["assignment"] == [2, 0]
        assert [o["F-Mean"] for o in stats["objects"]] == [oracle.f_from_pr(0.9, 0.9), oracle.f_from_pr(0.8, 0.8)] and [o["J-Mean"] for o in stats["objects"]] == [90.0 / 110.0, 80.0 / 120.0]
    # one proposal, three objects: it goes to the object it fits best, the two others score 0 on every frame
    fewer = [[30, 90, 60]]
    for stats in (oracle.sequence_stats(_tables_from_scores(fewer), 1, 3), davis.sequence_statistics(_tables_from_scores(fewer), 1, 3)):
        assert stats["assignment"] == [-1, 0, -1]
        assert [o["J-Mean"] for o in stats["objects"]] == [0.0, 90.0 / 110.0, 0.0] and [o["F-Mean"] for o in stats["objects"]] == [0.0, oracle.f_from_pr(0.9, 0.9), 0.0]
        assert [o["J-Recall"] for o in stats["objects"]] == [0.0, 1.0, 0.0]
    a, b = davis.sequence_statistics(_tables_from_scores(more), 3, 2), davis.sequence_statistics(_tables_from_scores(fewer), 1, 3)
    got, want = davis.summarize({"a": a, "b": b}), oracle.summary({"a": a, "b": b})
    assert got["J-Mean"] == want["J-Mean"] == float(np.mean(np.array([90.0 / 110.0, 80.0 / 120.0, 0.0, 90.0 / 110.0, 0.0])))
    assert got["J&F-Mean"] == (got["J-Mean"] + got["F-Mean"]) / 2.0 and got["sequences"]["b"]["assignment"] == [-1, 0, -1]
    # no proposal at all: every object scores 0
    none = davis.sequence_statistics({"area_g": np.zeros((3, 2), np.int64)}, 0, 2)
    assert none["assignment"] == [-1, -1] and all(o["J-Mean"] == 0.0 and o["F-Mean"] == 0.0 for o in none["objects"])


def test_radius_formula():
    from stemseg_amd.evaluation.davis import radius
    for (H, W), r in (((480, 854), 8), ((1080, 1920), 18), ((16, 16), 1)):
        assert radius(H, W) == r and oracle.radius(H, W) == r


# ------------------------------------------------------------------------------------------------ the C ABI, no device call
def test_davis_eval_counts_argument_errors_and_exports():
    from stemseg_amd import hip
    lib = hip.lib()
    for n in ("stemseg_hip_davis_eval_counts", "stemseg_hip_davis_eval_counts_size"):
        assert hasattr(lib, n) and n in hip.SIGNATURES
    assert lib.stemseg_hip_version() == hip.ABI_VERSION == 11
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stemseg_hip.h")).read()
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in header and "int stemseg_hip_davis_eval_counts(" in header
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below is refused before any HIP call
    size = lib.stemseg_hip_davis_eval_counts_size
    assert size(5, 20, 10) == 5 * (3 * 200 + 40 + 20) and size(1, 64, 32) > 0
    assert size(5, 65, 10) == 0 and size(5, 20, 33) == 0 and size(0, 1, 1) == 0 and size(5, 0, 1) == 0 and size(65536, 1, 1) == 0

    def call(pred=fake, index_bytes=1, gt=fake, T=5, H=37, W=53, Kp=20, Kg=10, r=2, counts=fake, n=1 << 30):
        return lib.stemseg_hip_davis_eval_counts(pred, index_bytes, gt, T, H, W, Kp, Kg, r, counts, n, None)
    for kw, word in ((dict(Kp=65), "limit is 64"), (dict(Kp=0), "limit is 64"), (dict(Kg=33), "limit is 32"), (dict(Kg=0), "limit is 32"),
                     (dict(r=0), "limits are 1 and 32"), (dict(r=33), "limits are 1 and 32"), (dict(index_bytes=4), "index_bytes"),
                     (dict(pred=None), "null"), (dict(gt=None), "null"), (dict(counts=None), "null"), (dict(T=0), "bad dims"),
                     (dict(T=65536), "bad dims"), (dict(H=0), "bad dims"), (dict(H=65536, W=32768), "2^31"), (dict(n=100), "int32"),
                     (dict(pred=C.c_void_p(0x1001), index_bytes=2), "misaligned"), (dict(counts=C.c_void_p(0x1002)), "misaligned")):
        assert call(**kw) == -1, kw
        assert word in lib.stemseg_hip_last_error().decode() and "davis_eval_counts" in lib.stemseg_hip_last_error().decode(), kw
    # the binding refuses shapes and types that do not go together before it asks for a device
    pred, gt = torch.zeros((3, 8, 9), dtype=torch.uint8), torch.zeros((2, 3, 8, 9), dtype=torch.uint8)
    for p, g, word in ((pred, gt[:, :2], "do not go together"), (pred, gt[:, :, :, :8], "do not go together"), (pred[0], gt, "do not go together"),
                       (pred.float(), gt, "not uint8 or a 16-bit"), (pred.long(), gt, "not uint8 or a 16-bit"), (pred, gt.bool(), "not uint8")):
        with pytest.raises(ValueError, match=word):
            hip.davis_eval_counts(p, g, 2, 1)
    assert hip.davis_eval_index_bytes(pred) == 1 and hip.davis_eval_index_bytes(pred.to(torch.int16)) == 2


# ------------------------------------------------------------------------------------------------ the driver's flag
@pytest.mark.parametrize("dataset", ["ytvis", "kittimots"])
def test_eval_annotations_is_refused_for_other_datasets(dataset, tmp_path):
    from stemseg_amd.inference import main
    args = main.build_parser().parse_args(["model.pth", "--dataset", dataset, "--eval_annotations", str(tmp_path / "val.json")])
    with pytest.raises(ValueError, match="--eval_annotations.*davis.*%s" % dataset):
        main.main(args)
    plain = main.build_parser().parse_args(["model.pth", "--dataset", "davis"])
    assert plain.eval_annotations is None


# ------------------------------------------------------------------------------------------------ the Trainer's hook
def _hooked_trainer(monkeypatch, tmp_path, **kw):
    from tests.test_grad_bucket_host import _Tiny, _fake_group
    from stemseg_amd.training import main
    cfg, _ = _fake_group(monkeypatch, 0, 1)
    said = []
    t = main.Trainer(cfg, str(tmp_path), NS(restore_session=None, initial_ckpt=None), NS(info=said.append, debug=said.append), model=_Tiny(), **kw)
    t.data_loader = [(torch.full((3,), float(k)), [{}], [{}]) for k in range(20)]          # batch 4 at one sample per pass: 5 steps
    return t, said


def test_trainer_calls_the_validation_hook_every_interval_steps(monkeypatch, tmp_path):
    calls = []

    def validate(trainer):
        assert not torch.is_grad_enabled()
        calls.append((trainer.elapsed_iterations, trainer.model.w.detach().clone()))
        return {"J&F-Mean": 0.25 * len(calls), "J-Mean": 0.5}
    t, said = _hooked_trainer(monkeypatch, tmp_path, validate_fn=validate)
    t.start(NS(save_interval=1000, display_interval=1, summary_interval=1, ckpts_to_keep=1, validation_interval=2))
    assert t.elapsed_iterations == 5 and [c[0] for c in calls] == [2, 4]
    assert not torch.equal(calls[0][1], calls[1][1]), "the hook must see the weights of its own step"
    assert t.logger.last_validation == {"J&F-Mean": 0.5, "J-Mean": 0.5, "iteration": 4}
    assert t.logger.last_point["iteration"] == 5 and "J&F-Mean" not in t.logger.last_point
    assert sum("validation" in str(s) and "J&F-Mean: 0.5000" in str(s) for s in said) == 1
    assert torch.is_grad_enabled()


@pytest.mark.parametrize("opts", [dict(validation_interval=0), dict()])
def test_trainer_never_validates_at_interval_0(monkeypatch, tmp_path, opts):
    calls = []
    t, _ = _hooked_trainer(monkeypatch, tmp_path, validate_fn=lambda trainer: calls.append(1) or {})
    t.start(NS(save_interval=1000, display_interval=1, summary_interval=1, ckpts_to_keep=1, **opts))
    assert t.elapsed_iterations == 5 and calls == [] and t.logger.last_validation == {}


def test_trainer_without_a_hook_ignores_the_interval(monkeypatch, tmp_path):
    from stemseg_amd.training import main
    t, _ = _hooked_trainer(monkeypatch, tmp_path)
    t.start(NS(save_interval=1000, display_interval=1, summary_interval=1, ckpts_to_keep=1, validation_interval=1))
    assert t.elapsed_iterations == 5 and t.validate_fn is None
    assert main.build_parser().parse_args(["--model_dir", "x", "--cfg", "davis"]).validation_interval == 0


def test_validation_runs_between_two_barriers_when_data_parallel(monkeypatch, tmp_path):
    from tests.test_grad_bucket_host import _fake_trainer
    for rank in (0, 1):
        calls = []
        t, seen, _ = _fake_trainer(monkeypatch, tmp_path / str(rank), rank, 2, data_parallel=True, validate_fn=lambda tr: calls.append(1) or {"x": 1.0})
        del seen[:]
        assert t.validate() == ({"x": 1.0} if rank == 0 else None)
        assert seen == ["synchronize", "synchronize"] and calls == ([1] if rank == 0 else [])


# ------------------------------------------------------------------------------------------------ the validity of the GPU cases
def test_gpu_cases_hold_what_they_are_named_after():
    seen_r, seen_kp, seen_kg, seen_T, seen_hw, seen_dtype = set(), set(), set(), set(), set(), set()
    for name in cases.GRID:
        pred, gt, Kp, r, tab = cases.case(name)
        seen_r.add(r); seen_kp.add(Kp); seen_kg.add(gt.shape[0]); seen_T.add(pred.shape[0]); seen_hw.add(pred.shape[1:]); seen_dtype.add(pred.dtype.itemsize)
        assert all(int(tab[k].sum()) > 0 for k in oracle.TABLES), name
        assert (tab["m_p"] < tab["n_p"][:, :, None]).any() and (tab["m_p"] > 0).any(), name          # matched and unmatched boundary pixels
    assert seen_r == {1, 2, 8, 19} and seen_kp == {1, 20, 64} and seen_kg == {1, 10, 32} and seen_T == {3, 5}
    assert seen_hw == {(37, 53), (45, 70)} and seen_dtype == {1, 2} and 19 > 37 / 2

    pred, gt, Kp, r, tab = cases.case("edges and corners")
    H, W = pred.shape[1:]
    for m in (pred[0] > 0, gt[:, 0].any(0)):
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and m[0, 0] and m[0, -1] and m[-1, 0] and m[-1, -1]
    assert (tab["m_p"] > 0).any(0).any(1).all(), "every edge proposal matches an object"

    pred, gt, Kp, r, tab = cases.case("special")
    assert Kp == 4 and not (pred == 3).any() and (tab["area_p"][:, 2] == 0).all() and (tab["n_p"][:, 2] == 0).all()          # label 3 never occurs
    assert not gt[2].any() and (tab["area_g"][:, 2] == 0).all()                                                              # an empty plane
    assert not pred[2].any() and not gt[:, 2].any() and all(int(tab[k][2].sum()) == 0 for k in oracle.TABLES)                # a frame with nothing
    assert (gt[0, 0] & gt[1, 0]).any() and tab["inter"][0, 0, 0] > 0 and tab["inter"][0, 0, 1] > 0                           # overlapping planes
    assert (pred == 5).any() and (pred == 200).any()                                                                         # labels above Kp ...
    clean = pred.copy()
    clean[clean > Kp] = 0
    again = oracle.counts(clean, gt, Kp, r)
    assert all(np.array_equal(again[k], tab[k]) for k in oracle.TABLES), "... count as background"
    assert oracle.boundary(pred[0] == 5).any()

    pred, gt, Kp, r, tab = cases.case("exactly r")
    nearer = oracle.counts(pred, gt, Kp, r - 1)
    assert (tab["m_p"] > 0).all() and (tab["m_g"] > 0).all() and int(nearer["m_p"].sum()) == 0 and int(nearer["m_g"].sum()) == 0

    pred, gt, Kp, r, tab = cases.case("tile seams")
    assert pred.shape[1:] == (130, 200) and r == 8
    bp, bg = oracle.boundary(pred[0] == 1), oracle.boundary(gt[0, 0])
    assert bp[:, :32].any() and not bp[:, 32:].any() and bg[:, 32:32 + r].any() and bp[:32].any() and bg[32:32 + r].any()          # across x = 32, y = 32
    hit = bp & oracle.dilate(bg & (np.arange(200)[None, :] >= 32), r)
    assert hit.any(), "a boundary pixel of the proposal left of the seam is matched by one of the object right of it"
    bp2, bg2 = oracle.boundary(pred[0] == 2), oracle.boundary(gt[1, 0])
    assert (bg2 & (np.arange(200)[None, :] < 64) & oracle.dilate(bp2 & (np.arange(200)[None, :] >= 64), r)).any(), "and the other way round at x = 64"
    assert tab["m_p"][0, 0, 0] > 0 and tab["m_g"][0, 1, 1] > 0 and tab["area_p"][0, 2] == 30 * 50

    pred, gt, Kp, r, tab = cases.case("frame leak")
    H = pred.shape[1]
    assert pred[0, H - 1].any() and gt[0, 1, 0].any() and gt[0, 1, H - 1].any() and pred[2, 0].any()
    assert int(tab["m_p"].sum()) == 0 and int(tab["m_g"].sum()) == 0 and int(tab["inter"].sum()) == 0
    stacked_p, stacked_g = np.concatenate([pred[0], pred[1]]), np.concatenate([gt[0, 0], gt[0, 1]])          # what a leak would see
    assert int(oracle.counts(stacked_p[None], stacked_g[None, None], Kp, r)["m_p"].sum()) > 0

    seqs = cases.evaluator_sequences()
    assert [(p.shape[0] >= 3, Kp > g.shape[0]) for _, p, g, Kp in seqs] == [(True, True), (True, False)]
