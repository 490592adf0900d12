"""Host side of tests/test_gpu_cluster_side.py (no GPU): every case of tests/cluster_side_cases.py is valid on the CPU oracle alone.
The clustering cases keep every probability of every round at least 1e-4 away from both thresholds, so the GPU tests may demand exact
labels of every point; the oracle finds the intended number of instances; the equal seeds sit where the tie-break has to act; the
documented scratch size covers what the gather lays out; the planted values are on both sides of every branch."""
import numpy as np
import pytest

from tests import cluster_side_cases as CS


def _check_margin(name, case, n=None):
    labels, meta = CS.run_oracle(case, n)
    m = CS.margin(meta)
    print("[cluster side] %s: N %d, K %d, smallest distance of a probability from 0.5 / 0.3: %.4g" % (
        name, labels.shape[0], len(meta["instance_labels"]), m))
    assert m >= CS.MARGIN, "%s: a probability within %g of a threshold -- pick another seed, not a band" % (name, m)
    return labels, meta


@pytest.mark.parametrize("layout", CS.LAYOUTS, ids=CS.LAYOUT_IDS)
def test_layout_cases_have_margin_and_every_instance(layout):
    E, Ev, stds, K = layout
    case = CS.layout_case(E, Ev, stds)
    assert case["emb"].shape[1] == E and case["bw"].shape[1] == Ev and Ev + len(stds) == E and 900 <= case["emb"].shape[0] <= 1700
    labels, meta = _check_margin("layout E %d Ev %d" % (E, Ev), case)
    assert len(meta["instance_labels"]) == K
    assert (labels == -1).any() and all(m.any() for m in meta["instance_masks"])


@pytest.mark.parametrize("max_instances,K,exhausted", CS.MAX_INSTANCES)
def test_max_instances_cases(max_instances, K, exhausted):
    case = CS.max_instances_case(max_instances)
    labels, meta = _check_margin("max_instances %d" % max_instances, case)
    s = CS.oracle_summary(case, labels, meta)
    assert (s["K"], s["exhausted"]) == (K, exhausted)
    if max_instances == 64:
        assert s["n_unassigned_last"] > 0                        # the loop ended on seediness: the outliers remain
    else:                                                        # out of rounds: the stale mask and the secondary pass see many points
        assert s["n_unassigned_last"] >= 1000
        final_round = meta["instance_masks"][-1]
        assert final_round.any() and np.array_equal(labels[final_round], np.full(int(final_round.sum()), case["label_start"] + K - 1))


def test_tie_case_winners_are_lowest_index_maxima_far_apart():
    case, winners = CS.tie_case()
    seed = case["seed"]
    assert case["emb"].shape == (CS.TIE_N, 4) and CS.TIE_N > 262144
    lev = np.round(seed * 16).astype(int)
    assert np.array_equal((lev / 16.0).astype(np.float32), seed)                # multiples of 1/16
    assert np.bincount(lev, minlength=17)[13:].min() >= 1000                     # thousands of equal values at the levels that can seed
    labels, meta = _check_margin("ties", case)
    assert len(meta["instance_labels"]) == CS.TIE_BLOBS
    picked = CS.expected_winners(case, meta)
    assert sorted(picked) == sorted(winners) and picked != sorted(picked)       # rounds do not walk the index range in order
    assert np.array_equal(np.array(meta["instance_centers"], np.float32), case["emb"][picked])
    assert len(set(w // 256 for w in winners)) == len(winners) and max(winners) - min(winners) > 262144
    for r, w in enumerate(picked):
        for o in CS.TIE_OFFSETS:
            assert seed[w + o] == seed[w]
        assert w % 293 < 37                                                      # the winner's thread owns w and w + 256
        assert (seed[:w][labels[:w] == case["label_start"] + r] < seed[w]).all()   # earlier points of the blob: lower seediness
    assert (labels == -1).sum() > 10_000                                         # outliers stay: the secondary pass runs over them


@pytest.mark.parametrize("n", CS.N_POINTS_DEV)
def test_n_points_prefixes_have_margin(n):
    case = CS.n_points_case()
    assert case["emb"].shape[0] == CS.N_POINTS_MAX
    k = min(n, CS.N_POINTS_MAX)
    labels, meta = _check_margin("n_points %d" % n, case, k)
    assert labels.shape[0] == k and (len(meta["instance_labels"]) >= 6 if k > 4000 else len(meta["instance_labels"]) <= 1)


def test_documented_scratch_covers_the_layout():
    with open(CS.HEADER) as f:
        text = f.read()
    assert text.count("scratch: >= " + CS.SCRATCH_DOC + " bytes") == 1
    for V in list(range(1, 5000)) + [17160, 1_050_000, 2 ** 31 - 1] + [1024 * k + d for k in (1, 2, 3, 7, 1025, 1026) for d in (-1, 0, 1)]:
        assert CS.scratch_bytes_documented(V) >= CS.scratch_bytes_needed(V), V
    assert CS.scratch_bytes_needed(17160) == 216 and CS.scratch_bytes_needed(1_050_000) == 12320
    assert [np.prod(s) for s in CS.SCRATCH_CASES] == [17160, 1_050_000]


def test_gather_cases_reach_the_branches():
    assert [np.prod(s[1:]) for s in CS.GATHER_SHAPES] == [45, 1023, 1024, 1]
    T, H, W = CS.CARRY_SHAPE
    assert -(-T * H * W // 1024) == 1026                         # more blocks than one pass of the scan takes
    fg = CS.fg_mask(T, H, W, 0.3)
    vox, offs = CS.compact_twin(fg)
    assert offs[1] > 0 and offs[2] - offs[1] > 0 and vox.size == offs[-1]
    assert fg.reshape(-1)[1024 * 1024:].any()                    # foreground in the blocks of the second pass
    small = CS.compact_twin(CS.fg_mask(7, 5, 9, 0.4))[1]
    assert np.all(np.diff(small) > 0)                            # seven non-empty frames inside one block


@pytest.mark.parametrize("Ka,Kb", CS.OVERLAP_CASES)
def test_overlap_cases_sit_at_the_switch_and_hold_stray_ids(Ka, Kb):
    la, lb, ids_a, ids_b = CS.overlap_case(Ka, Kb)
    nh = Ka * Kb + Ka + Kb
    assert {(95, 127): nh == CS.OVERLAP_LDS_CELLS - 1, (96, 127): nh > CS.OVERLAP_LDS_CELLS}.get((Ka, Kb), nh <= CS.OVERLAP_LDS_CELLS)
    for lab, ids in ((la, ids_a), (lb, ids_b)):
        assert len(ids) == len(set(ids)) and set(ids) <= set(lab.tolist())
        top = max(ids) if ids else 0
        assert 0.15 < (lab == -1).mean() < 0.25
        assert (lab == top + 1).any() and (lab > top + 1).any()                  # at lut_len - 1 and beyond it
        assert not ids or ((lab > 0) & (lab < top) & ~np.isin(lab, ids)).any()    # inside the LUT, not listed


def test_label_statistics_cases():
    for cap in CS.PRESENCE_CAPS:
        arrs = CS.presence_arrays(cap)
        present, mx = CS.presence_twin(np.concatenate(arrs["mixed"]), cap)
        assert present[cap] == 1 and mx == cap + 701 and present[:cap].all()
        p, m = CS.presence_twin(arrs["beyond_cap_only"][0], cap)
        assert not p.any() and m == 2 ** 40 + 1
        p, m = CS.presence_twin(arrs["negative_only"][0], cap)
        assert p.sum() == 1 and p[cap] == 1 and m == 0
        assert np.array_equal(np.concatenate(arrs["three_arrays"]), arrs["mixed"][0])
    for map_len in CS.RELABEL_MAP_LENS:
        labels, mapping = CS.relabel_case(map_len)
        out = CS.relabel_twin(labels, mapping)
        inside = (labels >= -1) & (labels <= map_len - 2)
        assert np.array_equal(out[~inside], labels[~inside]) and (~inside).any() and (labels < -1).any() and (labels >= map_len - 1).any()
        assert not inside.any() or (out[inside] != labels[inside]).all()


@pytest.mark.parametrize("B", CS.CODE_BINS)
def test_code_cases_cover_every_clamp(B):
    from tests.oracle_ops import OracleChainerOps
    fg, labels, n_dev = CS.codes_case(B)
    vox, offs = CS.compact_twin(fg)
    n = int(offs[-1])
    assert 0 < n_dev < n == labels.shape[0]
    codes = CS.codes_twin(labels, vox, n_dev, CS.CODE_LABEL_START, fg.size)
    assert (codes[vox[n_dev:]] == 0).all() and (codes[vox[:n_dev]] != 0).all()
    got = set(codes.tolist())
    assert {0, 1, 2, B - 2, B - 1, 254, 255} <= got and (B == 66 or 101 in got)
    below, above = labels[:n_dev] >= 0, labels[:n_dev] > CS.CODE_LABEL_START + 253
    below &= labels[:n_dev] < CS.CODE_LABEL_START
    assert below.any() and above.any() and (codes[vox[:n_dev]][below | above] == 254).all()
    assert (OracleChainerOps._bins(np.array([254, 255, B - 1, B - 2], np.uint8), B) == [B - 1, B - 1, B - 1, B - 2]).all()


def test_many_items_case_spans_two_launches():
    codes, plane_a, plane_b, vox, items, lut, n_out = CS.many_items_case()
    n = CS.MANY_ITEMS
    assert n == 65536 + 3 > 65535 and plane_a.shape == plane_b.shape == (n,) and items.shape == (n, 5) and lut.shape == (n, CS.MANY_B)
    assert (plane_a == -1).any() and {254, 255, 0, 1, 2, 100} <= set(codes.reshape(-1).tolist())
    assert n * CS.MANY_B * CS.MANY_B * 4 > 2_300_000
    src, cnt, vbase, plane, dst = items.T
    assert (cnt[65535:] > 0).any() and n_out == cnt.sum() and np.array_equal(dst, np.cumsum(cnt) - cnt)
    assert len({(a, b) for a, b in zip(plane_a[65535:].tolist(), plane_b[65535:].tolist())}) == 4
    for k in (0, 65534, 65535, n - 1):                           # every item reads its own plane's voxels only
        v = vox[src[k]:src[k] + cnt[k]].astype(np.int64) - vbase[k]
        assert ((v >= 0) & (v < CS.MANY_HW)).all()
    v = vox[np.repeat(src, cnt) + (np.arange(n_out) - np.repeat(dst, cnt))].astype(np.int64) - np.repeat(vbase, cnt)
    assert ((v >= 0) & (v < CS.MANY_HW)).all()


def test_accumulator_and_mask_cases():
    for C in CS.ACC_CHANNELS:
        clips = CS.accumulate_case(C)
        acc, counts = CS.accumulate_twin(clips, CS.ACC_HW)
        assert counts == [2, 1, 3, 1]
        a63, _ = CS.accumulate_twin(clips, 63)
        assert np.array_equal(a63, acc[..., :63])
        # the order of the adds matters for these values: summing a frame's three contributions backwards differs somewhere
        back = clips[1][:, 1] + clips[1][:, 0] + clips[0][:, 2]
        assert not np.array_equal(back, acc[2])
    acc, counts = CS.mask_frames_case()
    m = CS.mask_frames_twin(acc, counts, CS.MASK_FRAMES_THR)
    assert not m[0].any() and acc[0].max() > 1
    for f in range(1, len(counts)):
        assert m[f, 10] == 0 and m[f, 12] == 1 and 0 < m[f].mean() < 1         # one ulp below / above the product decides


@pytest.mark.parametrize("HW", CS.FG_CLIP_HW)
@pytest.mark.parametrize("C", CS.FG_CLIP_CHANNELS)
def test_fg_clip_reference_leaves_out_few_pixels(C, HW):
    x = CS.fg_clip_case(C, HW)
    p = CS.fg_clip_reference(x)
    left_out = CS.fg_clip_band(p)
    assert p.shape == (CS.FG_CLIP_T, 1, HW)
    assert p[0, 0, 5] == 0.5 and not left_out[0, 0, 5]           # exactly thr is not left out: the mask there is 0 on both sides
    assert left_out.mean() <= CS.FG_CLIP_LEFT_OUT
    if C == 2:
        assert p[0, 0, 6] == 0 and p[1, 0, 7] == 1 and np.isnan(p[1, 0, 8]) and np.isnan(p).sum() == 1
    else:
        assert p[0, 0, 6] == 0 and p[1, 0, 7] == 1 and not np.isnan(p).any()
    assert 0.3 < (p > 0.5).mean() < 0.7
