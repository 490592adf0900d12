"""GPU tests of everything downstream of the heads, kernel by kernel, at the layouts and edges the flows never reach: clustering at every
(E, Ev) the distance sum distinguishes, max_instances at both ends, more than one point per thread with equal seeds, n_points on the
device; the gather / compaction with frames smaller than a block and with a scan that carries over passes, on a scratch region of
exactly the documented size; the label statistics at the LDS / global switch and at every clamp; the stitching kernels over more items
than one launch takes; the semseg / seediness accumulators on the scalar and the vector path.  References: the CPU oracle and numpy;
every case comes from tests/cluster_side_cases.py, whose validity tests/test_cluster_side_host.py asserts without a GPU (in
particular: no probability of any clustering case lies within 1e-4 of a threshold, so labels are demanded exactly of every point)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cluster_side_cases as CS
from tests.oracle_ops import OracleChainerOps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


_oracle = {}


def oracle(key, case, n=None):
    """The CPU oracle's (labels, meta) of a case, computed once per module."""
    if key not in _oracle:
        _oracle[key] = CS.run_oracle(case, n)
    return _oracle[key]


def _params(hip, case):
    return hip.make_cluster_params(0.5, 0.3, case["min_seed"], case["max_instances"], list(case["stds"]))


def _cluster(hip, case, want=True):
    """hip.cluster on a whole case -> labels, record, primary masks [K, N], probabilities [K, N] (numpy)."""
    labels, meta_dev, masks, probs = hip.cluster(dev(case["emb"]), dev(case["bw"]), dev(case["seed"]), _params(hip, case), case["label_start"],
                                                 None, want, want)
    meta = hip.read_cluster_meta(meta_dev)
    return (labels.cpu().numpy(), meta, masks[:meta.K].cpu().numpy().astype(bool) if want else None,
            probs[:meta.K].cpu().numpy() if want else None)


def _ref_masks(meta, n):
    return np.stack(meta["instance_masks"]) if meta["instance_masks"] else np.zeros((0, n), bool)


# ------------------------------------------------------------------------------------------------ 1. clustering
@pytest.mark.parametrize("layout", CS.LAYOUTS, ids=CS.LAYOUT_IDS)
def test_cluster_layout_matrix(hip, layout):
    """Every (E, Ev, free dims) the distance sum tells apart -- its own order for E = 5, one 16-byte load for E = 4, a sequential sum
    otherwise, no bandwidth tensor at all for Ev = 0 -- through SequentialClustering (hip.cluster with an empty bw for Ev = 0): labels,
    instance list, primary masks and centres equal to the oracle's, probabilities and stds within 1e-6.  (On this margin data a
    different summation order moves no label: the test pins the layouts, not the order of the E = 5 sum.)"""
    from stemseg_amd.inference.clusterers import SequentialClustering
    E, Ev, stds, K = layout
    case = CS.layout_case(E, Ev, stds)
    ref_labels, ref = oracle(("layout", E, Ev), case)
    n = case["emb"].shape[0]
    cl = SequentialClustering(0.5, 0.3, case["min_seed"], len(stds), list(stds), "cuda:0", max_instances=case["max_instances"])
    if Ev > 0:
        labels, meta = cl(dev(case["emb"]), bandwidths=dev(case["bw"]), seediness=dev(case["seed"])[:, None],
                          cluster_label_start=case["label_start"], return_label_masks=True, return_probs=True)
        labels = labels.cpu().numpy()
    else:
        empty_bw = torch.empty(n, 0, dtype=torch.float32, device="cuda")
        labels, meta_dev, masks, probs = hip.cluster(dev(case["emb"]), empty_bw, dev(case["seed"]), _params(hip, case), case["label_start"],
                                                     None, True, True)
        meta = cl.meta_to_dict(hip.read_cluster_meta(meta_dev), E, case["label_start"], masks, probs, n)
        labels = labels.cpu().numpy()
    assert meta["instance_labels"] == ref["instance_labels"] and len(meta["instance_labels"]) == K
    bad = np.flatnonzero(labels != ref_labels)
    assert bad.size == 0, "%d label mismatches, first at %s" % (bad.size, bad[:5])
    assert np.array_equal(np.array(meta["instance_centers"], np.float32), np.array(ref["instance_centers"], np.float32))
    assert np.array_equal(np.stack([m.numpy() for m in meta["instance_masks"]]), _ref_masks(ref, n))
    perr = float(np.abs(np.stack([p.numpy() for p in meta["instance_probs"]]).astype(np.float64) - np.stack(ref["instance_probs"])).max())
    serr = float(np.abs(np.array(meta["instance_stds"], np.float64) - np.array(ref["instance_stds"], np.float64)).max())
    print("[cluster side] E %d Ev %d: probabilities within %.3g, stds within %.3g of the oracle" % (E, Ev, perr, serr))
    assert perr <= CS.PROB_TOL and serr <= CS.PROB_TOL


@pytest.mark.parametrize("max_instances,K,exhausted", CS.MAX_INSTANCES)
def test_cluster_max_instances_extremes(hip, max_instances, K, exhausted):
    """max_instances = 64 (STEMSEG_MAX_INSTANCES: 30 instances found, the loop ends on seediness), 7 and 1 (out of rounds: the stale
    availability mask and the secondary pass act on more than a thousand left-over points): labels, K, exhausted, n_unassigned_last
    and the primary masks equal to the oracle's."""
    case = CS.max_instances_case(max_instances)
    ref_labels, ref = oracle(("max_instances", max_instances), case)
    exp = CS.oracle_summary(case, ref_labels, ref)
    labels, meta, masks, probs = _cluster(hip, case)
    assert (meta.K, meta.exhausted, meta.n_unassigned_last, meta.n_points) == (K, exhausted, exp["n_unassigned_last"], ref_labels.shape[0])
    assert exp["K"] == K
    bad = np.flatnonzero(labels != ref_labels)
    assert bad.size == 0, "%d label mismatches, first at %s" % (bad.size, bad[:5])
    assert np.array_equal(masks, _ref_masks(ref, labels.shape[0]))
    assert float(np.abs(probs.astype(np.float64) - np.stack(ref["instance_probs"])).max()) <= CS.PROB_TOL


def test_cluster_ties_with_several_points_per_thread(hip):
    """300 000 points in one set (beyond 262 144 a thread owns more than one) with seediness in sixteenths: every round picks among
    thousands of equal maxima, and the lowest index has to win inside a thread's loop, a wave, a block and across the 1024 partials.
    Labels, masks, instance list exact; every centre is the embedding of the lowest-index maximal-seed point.  Then the same set
    next to two small ones in one cluster_batch call (three live sets: two points per thread everywhere): torch.equal with the lone call."""
    case, _ = CS.tie_case()
    ref_labels, ref = oracle("ties", case)
    winners = CS.expected_winners(case, ref)
    params = _params(hip, case)
    e, b, s = dev(case["emb"]), dev(case["bw"]), dev(case["seed"])
    labels, meta_dev, masks, probs = hip.cluster(e, b, s, params, case["label_start"], None, True, True)
    meta = hip.read_cluster_meta(meta_dev)
    assert meta.K == CS.TIE_BLOBS == len(ref["instance_labels"]) and meta.exhausted == 0 and meta.n_points == CS.TIE_N
    centres = np.array([[meta.centers[k][d] for d in range(4)] for k in range(meta.K)], np.float32)
    assert np.array_equal(centres, case["emb"][winners]), "a round's seed is not the lowest-index maximum"
    assert np.array_equal(np.array([meta.seed_prob[k] for k in range(meta.K)], np.float32), case["seed"][winners])
    got = labels.cpu().numpy()
    bad = np.flatnonzero(got != ref_labels)
    assert bad.size == 0, "%d label mismatches, first at %s" % (bad.size, bad[:5])
    assert np.array_equal(masks[:meta.K].cpu().numpy().astype(bool), _ref_masks(ref, CS.TIE_N))
    assert float((probs[:meta.K].cpu() - torch.from_numpy(np.stack(ref["instance_probs"]))).abs().max()) <= CS.PROB_TOL
    small = [CS.small_set(3000, 5, 11), CS.small_set(700, 3, 12)]
    sets = [(e, b, s, None)] + [(dev(c["emb"]), dev(c["bw"]), dev(c["seed"]), None) for c in small]
    out = hip.cluster_batch(sets, params, case["label_start"])
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], labels) and torch.equal(out[0][1], meta_dev)
    for c, (l2, m2), (e2, b2, s2, _) in zip(small, out[1:], sets[1:]):
        l1, m1, _, _ = hip.cluster(e2, b2, s2, params, case["label_start"])
        assert torch.equal(l1, l2) and torch.equal(m1, m2) and hip.read_cluster_meta(m2).K >= 3


@pytest.mark.parametrize("n", CS.N_POINTS_DEV)
def test_cluster_n_points_on_the_device(hip, n):
    """*n_points_dev = 0, 1, n_max - 3, n_max and beyond n_max (clamped): the first N labels are the oracle's on the first N points,
    the rest are -1, the record says min(N, n_max), and the columns of the mask / probability buffers beyond N keep what they held."""
    case = CS.n_points_case()
    n_max, M = CS.N_POINTS_MAX, case["max_instances"]
    k = min(n, n_max)
    ref_labels, ref = oracle(("n_points", k), case, k)
    K = len(ref["instance_labels"])
    e, b, s = dev(case["emb"]), dev(case["bw"]), dev(case["seed"])
    params = _params(hip, case)
    labels = torch.full((n_max,), -77, dtype=torch.int64, device="cuda")
    meta_dev = torch.full((ctypes.sizeof(hip.ClusterMeta),), 0xEE, dtype=torch.uint8, device="cuda")
    masks = torch.full((M, n_max), 7, dtype=torch.uint8, device="cuda")
    probs = torch.full((M, n_max), -7.0, dtype=torch.float32, device="cuda")
    ws_bytes = hip.lib().stemseg_hip_cluster_workspace_bytes(n_max)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    n_dev = dev(np.array([n], np.int64))
    hip.check(hip.lib().stemseg_hip_cluster(hip.ptr(e), hip.ptr(b), hip.ptr(s), n_max, hip.ptr(n_dev), 4, 2, ctypes.byref(params),
                                            case["label_start"], hip.ptr(labels), hip.ptr(meta_dev), hip.ptr(masks), hip.ptr(probs),
                                            hip.ptr(ws), ws_bytes, hip.stream()))
    meta = hip.read_cluster_meta(meta_dev)
    assert meta.n_points == k and meta.K == K and (n > 0 or K == 0)
    got = labels.cpu().numpy()
    assert np.array_equal(got[:k], ref_labels) and (got[k:] == -1).all()
    masks, probs = masks.cpu().numpy(), probs.cpu().numpy()
    assert (masks[:, k:] == 7).all() and (probs[:, k:] == -7.0).all()
    if K:
        assert np.array_equal(masks[:K, :k].astype(bool), _ref_masks(ref, k))
        assert float(np.abs(probs[:K, :k].astype(np.float64) - np.stack(ref["instance_probs"])).max()) <= CS.PROB_TOL


# ------------------------------------------------------------------------------------------------ 2. gather and compaction
def _check_gather(hip, T, H, W, fg, E, Ev, seed=0):
    emb, bw, sd = CS.head_outputs(T, H, W, E, Ev, seed)
    from oracle import pipeline as opipe
    e, b, s, counts = opipe.gather_fg(emb, bw, sd, fg)
    ge, gb, gs, vox, offs = hip.fg_gather(dev(emb), dev(bw), dev(sd), dev(fg))
    rvox, roffs = CS.compact_twin(fg)
    n = int(roffs[-1])
    assert np.array_equal(offs.cpu().numpy(), roffs) and np.array_equal(np.diff(roffs), counts)
    assert np.array_equal(vox[:n].cpu().numpy(), rvox)
    assert np.array_equal(ge[:n].cpu().numpy(), e) and np.array_equal(gb[:n].cpu().numpy(), b) and np.array_equal(gs[:n].cpu().numpy(), s[:, 0])


@pytest.mark.parametrize("density", CS.GATHER_DENSITIES)
@pytest.mark.parametrize("shape", CS.GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_and_compact_small_and_ragged_frames(hip, shape, density):
    """Frames of 45, 1023, 1024 and 1 voxels (several frame starts inside one 1024-voxel block; a frame one short of a block) with no,
    all and 40 % foreground: fg_compact and fg_gather (E 5 / Ev 3 and E 1 / Ev 1) bit-exact vs the oracle."""
    T, H, W = shape
    fg = CS.fg_mask(T, H, W, density, seed=H)
    vox, offs = hip.fg_compact(dev(fg))
    rvox, roffs = OracleChainerOps().compact(torch.from_numpy(fg))
    n = int(roffs[-1])
    assert n == {0.0: 0, 1.0: T * H * W}.get(density, n)
    assert np.array_equal(offs.cpu().numpy(), roffs.numpy()) and np.array_equal(vox.cpu().numpy()[:n], rvox.numpy()[:n])
    for E, Ev in CS.GATHER_LAYOUTS:
        _check_gather(hip, T, H, W, fg, E, Ev, seed=E)


def test_gather_scan_carries_across_passes(hip):
    """V = 1 050 000: 1 026 blocks, so the single-block scan takes two passes of 1 024 and the second starts from the first's total."""
    T, H, W = CS.CARRY_SHAPE
    fg = CS.fg_mask(T, H, W, 0.3)
    rvox, roffs = OracleChainerOps().compact(torch.from_numpy(fg))
    n = int(roffs[-1])
    vox, offs = hip.fg_compact(dev(fg))
    assert np.array_equal(offs.cpu().numpy(), roffs.numpy()) and np.array_equal(vox.cpu().numpy()[:n], rvox.numpy()[:n])
    _check_gather(hip, T, H, W, fg, 4, 2)


@pytest.mark.parametrize("shape", CS.SCRATCH_CASES, ids=lambda s: "x".join(map(str, s)))
def test_gather_scratch_of_exactly_the_documented_size(hip, shape):
    """stemseg_hip_fg_compact and stemseg_hip_fg_gather through the C entry points with a scratch region of exactly the bytes
    include/stemseg_hip.h asks for, a canary right behind it in the same allocation: the canary survives and the results are exact.
    (With the header's earlier `8 * (V/1024 + 2)` -- 144 bytes at V = 17 160 against the 216 laid out, 8 216 against 12 320 at
    V = 1 050 000 -- the offsets table ran over the canary.)"""
    T, H, W = shape
    V, HW = T * H * W, H * W
    nbytes, guard = CS.scratch_bytes_documented(V), 4096
    assert CS.scratch_bytes_needed(V) <= nbytes + guard          # whatever the header says: every write stays inside this allocation
    fg = CS.fg_mask(T, H, W, 0.3, seed=5)
    rvox, roffs = CS.compact_twin(fg)
    n = int(roffs[-1])
    fg_d = dev(fg)
    lib = hip.lib()

    def region():
        return torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    buf = region()
    vox = torch.empty(V, dtype=torch.int32, device="cuda")
    offs = torch.empty(T + 1, dtype=torch.int64, device="cuda")
    hip.check(lib.stemseg_hip_fg_compact(hip.ptr(fg_d), T, HW, hip.ptr(vox), hip.ptr(offs), hip.ptr(buf), hip.stream()))
    assert bool((buf[nbytes:] == 0xA5).all()), "fg_compact wrote behind the documented scratch size"
    assert np.array_equal(offs.cpu().numpy(), roffs) and np.array_equal(vox[:n].cpu().numpy(), rvox)
    emb, bw, sd = CS.head_outputs(T, H, W, 4, 2)
    buf = region()
    eo, bo = torch.empty(V, 4, device="cuda"), torch.empty(V, 2, device="cuda")
    so, vox = torch.empty(V, device="cuda"), torch.empty(V, dtype=torch.int32, device="cuda")
    offs = torch.empty(T + 1, dtype=torch.int64, device="cuda")
    emb_d, bw_d, sd_d = dev(emb), dev(bw), dev(sd)
    hip.check(lib.stemseg_hip_fg_gather(hip.ptr(emb_d), hip.ptr(bw_d), hip.ptr(sd_d), hip.ptr(fg_d), 4, 2, T, HW, hip.ptr(eo), hip.ptr(bo),
                                        hip.ptr(so), hip.ptr(vox), hip.ptr(offs), hip.ptr(buf), hip.stream()))
    assert bool((buf[nbytes:] == 0xA5).all()), "fg_gather wrote behind the documented scratch size"
    assert np.array_equal(offs.cpu().numpy(), roffs) and np.array_equal(vox[:n].cpu().numpy(), rvox)
    m = fg.astype(bool)
    assert np.array_equal(eo[:n].cpu().numpy(), np.moveaxis(emb, 0, -1)[m]) and np.array_equal(bo[:n].cpu().numpy(), np.moveaxis(bw, 0, -1)[m])
    assert np.array_equal(so[:n].cpu().numpy(), sd[0][m])


# ------------------------------------------------------------------------------------------------ 3. label statistics
@pytest.mark.parametrize("Ka,Kb", CS.OVERLAP_CASES)
def test_overlap_counts_at_the_lds_global_switch(hip, Ka, Kb):
    """95 x 127 ids: 12 287 cells, the largest LDS table with both sides non-empty; 96 x 127: the first on global atomics; an empty
    side each way.  Labels hold ids a LUT does not list, the id at lut_len - 1 and ids beyond it.  Exact vs the numpy twin."""
    from stemseg_amd.inference.online_chainer import HipChainerOps
    la, lb, ids_a, ids_b = CS.overlap_case(Ka, Kb)
    got = HipChainerOps().overlap_counts(dev(la), dev(lb), ids_a, ids_b)
    exp = OracleChainerOps().overlap_counts(torch.from_numpy(la), torch.from_numpy(lb), ids_a, ids_b)
    for g, x in zip(got, exp):
        assert g.shape == x.shape and np.array_equal(g, x)
    assert int(exp[1].sum()) > 0 or Ka == 0


@pytest.mark.parametrize("cap", CS.PRESENCE_CAPS)
def test_label_presence_raw_entry_point(hip, cap):
    """stemseg_hip_label_presence with cap = 0, 1, 300: labels >= cap raise max_plus_1 and set no byte, byte `cap` is the negative
    flag, nothing is written behind it; only-negative and empty input; accumulate = 1 over several arrays equals one call on their
    concatenation."""
    lib = hip.lib()
    for name, arrays in CS.presence_arrays(cap).items():
        buf = torch.full((cap + 1 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        mx = torch.full((1,), -5, dtype=torch.int64, device="cuda")
        for k, a in enumerate(arrays):
            t = dev(a) if a.size else None
            hip.check(lib.stemseg_hip_label_presence(hip.ptr(t), a.size, hip.ptr(buf), cap, hip.ptr(mx), int(k > 0), hip.stream()))
        present, m = CS.presence_twin(np.concatenate(arrays), cap)
        got = buf.cpu().numpy()
        assert np.array_equal(got[:cap + 1], present), name
        assert (got[cap + 1:] == 0xEE).all() and int(mx.item()) == m, name


@pytest.mark.parametrize("map_len", CS.RELABEL_MAP_LENS)
def test_relabel_leaves_labels_outside_the_map(hip, map_len):
    labels, mapping = CS.relabel_case(map_len)
    t = dev(labels.copy())
    hip.relabel(t, dev(mapping))
    assert np.array_equal(t.cpu().numpy(), CS.relabel_twin(labels, mapping))


@pytest.mark.parametrize("B", CS.CODE_BINS)
def test_codes_tables_and_lut_gather_at_every_clamp(hip, B):
    """labels_to_codes with labels below label_start and above label_start + 253 (code 254), negative (255), codes at and above
    B - 1 and n_points_dev < n_max; pair_tables with plane_a = -1 and codes_to_labels on those planes: exact vs the numpy twins."""
    ref = OracleChainerOps()
    fg, labels, n_dev = CS.codes_case(B)
    vox, offs = CS.compact_twin(fg)
    T, HW, V = fg.shape[0], fg[0].size, fg.size
    vox_d, nd = dev(vox), dev(np.array([n_dev], np.int64))
    codes = torch.full((2, V), 9, dtype=torch.uint8, device="cuda")
    labels2 = np.roll(labels, 7)
    hip.labels_to_codes(dev(labels), vox_d, nd, CS.CODE_LABEL_START, codes[0])
    hip.labels_to_codes(dev(labels2), vox_d, None, 1, codes[1])
    exp = np.stack([CS.codes_twin(labels, vox, n_dev, CS.CODE_LABEL_START, V), CS.codes_twin(labels2, vox, labels.size, 1, V)])
    assert np.array_equal(codes.cpu().numpy(), exp)
    planes, rplanes = codes.view(2 * T, HW), torch.from_numpy(exp).view(2 * T, HW)
    pa, pb = [-1, 1, 2, 3, 4, -1], [T, T + 1, T + 2, 0, 1, 2]
    tabs = hip.pair_tables(planes, dev(np.array(pa, np.int32)), dev(np.array(pb, np.int32)), B)
    rt = ref.pair_tables(rplanes, pa, pb, B).numpy()
    assert np.array_equal(tabs.cpu().numpy(), rt) and rt[:, :, B - 1].sum() > 0 and rt[:, B - 1, :].sum() > 0
    rs = np.random.RandomState(B)
    items, cur = [], 0
    for plane in range(2 * T):
        t = plane % T
        items.append((int(offs[t]), int(offs[t + 1] - offs[t]), t * HW, plane, cur))
        cur += items[-1][1]
    items = np.array(items, np.int64)
    lut = rs.randint(-1, 1 << 40, (len(items), B)).astype(np.int64)
    out = hip.codes_to_labels(planes, vox_d, dev(items), dev(lut), int(items[:, 1].max()), cur)
    assert np.array_equal(out.cpu().numpy(), ref.labels_from_codes(rplanes, torch.from_numpy(vox), items, lut, int(items[:, 1].max()), cur).numpy())


def test_pair_tables_and_lut_gather_over_two_launches(hip):
    """65 536 + 3 items in one call of each: the entry points cut them into launches of 65 535 and offset the plane lists, the tables,
    the items and the LUT rows for the second; every item, those of the second launch included, equals the numpy twin's."""
    ref = OracleChainerOps()
    codes, pa, pb, vox, items, lut, n_out = CS.many_items_case()
    codes_d = dev(codes)
    tabs = hip.pair_tables(codes_d, dev(pa), dev(pb), CS.MANY_B).cpu().numpy()
    combos, inv = np.unique(np.stack([pa, pb], 1), axis=0, return_inverse=True)
    exp = ref.pair_tables(torch.from_numpy(codes), combos[:, 0].tolist(), combos[:, 1].tolist(), CS.MANY_B).numpy()[inv.reshape(-1)]
    assert tabs.shape == exp.shape == (CS.MANY_ITEMS, CS.MANY_B, CS.MANY_B)
    assert np.array_equal(tabs[:65535], exp[:65535]) and np.array_equal(tabs[65535:], exp[65535:]) and exp[65535:].sum() > 0
    out = hip.codes_to_labels(codes_d, dev(vox), dev(items), dev(lut), int(items[:, 1].max()), n_out).cpu().numpy()
    exp = ref.labels_from_codes(torch.from_numpy(codes), torch.from_numpy(vox), items, lut, int(items[:, 1].max()), n_out).numpy()
    first = int(items[65535, 4])
    assert np.array_equal(out[:first], exp[:first]) and np.array_equal(out[first:], exp[first:]) and first < n_out


# ------------------------------------------------------------------------------------------------ 4. accumulators and masks
def _accumulate(hip, clips, path):
    """The clips of CS.ACC_CLIPS into a [F, C, 1, hw] accumulator on the path named -> numpy."""
    from stemseg_amd.modeling.inference_model import InferenceModel
    C = clips[0].shape[0]
    hw = 63 if path == "scalar_hw63" else CS.ACC_HW
    n = CS.ACC_FRAMES * C * hw
    if path == "scalar_acc_misaligned":
        acc = torch.zeros(n + 1, device="cuda")[1:].view(CS.ACC_FRAMES, C, 1, hw)
        assert acc.data_ptr() % 16 == 4 and acc.is_contiguous()
    else:
        acc = torch.zeros(CS.ACC_FRAMES, C, 1, hw, device="cuda")
        assert acc.data_ptr() % 16 == 0
    counts = [0] * CS.ACC_FRAMES
    for x, sub in zip(clips, CS.ACC_CLIPS):
        x = np.ascontiguousarray(x[..., :hw])
        if path == "scalar_clip_misaligned":
            xd = torch.zeros(x.size + 1, device="cuda")[1:].view(x.shape)
            xd.copy_(torch.from_numpy(x))
            assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
        else:
            xd = dev(x)
            assert xd.data_ptr() % 16 == 0
        if -1 in sub:
            hip.semseg_accumulate(acc, xd, sub)
            for t in sub:
                if t >= 0:
                    counts[t] += 1
        else:
            InferenceModel._accumulate_semseg(acc, counts, xd, sub)           # a repeated frame: one call per repetition
    return acc.cpu().numpy(), counts


@pytest.mark.parametrize("C", CS.ACC_CHANNELS)
def test_semseg_accumulate_every_path(hip, C):
    """HW = 63 (scalar), HW = 64 with the accumulator or the clip starting 4 bytes into its allocation (scalar by alignment), HW = 64
    aligned (16-byte accesses), with skipped slots and a clip that repeats a frame: bit-equal to sequential numpy fp32 adds in slot
    order, and the paths bit-equal to one another on the same data."""
    clips = CS.accumulate_case(C)
    ref, ref_counts = CS.accumulate_twin(clips, CS.ACC_HW)
    got = {}
    for path in CS.ACC_PATHS:
        got[path], counts = _accumulate(hip, clips, path)
        assert counts == ref_counts
        assert np.array_equal(got[path], ref[..., :got[path].shape[-1]]), path
    assert np.array_equal(got["scalar_hw63"], got["vector"][..., :63])
    assert np.array_equal(got["scalar_acc_misaligned"], got["vector"]) and np.array_equal(got["scalar_clip_misaligned"], got["vector"])


def test_semseg_masks_single_channel(hip):
    """C = 1 (the foreground logit alone, as the clip-parallel path exchanges it): fg within 1e-6 of the fp64 sigmoid of the fp32 mean;
    any multi-class output type is the documented argument error."""
    acc, counts = CS.accumulate_twin(CS.accumulate_case(1), CS.ACC_HW)
    cnt = np.array(counts, np.float32)
    fg, mc = hip.semseg_masks(dev(acc), dev(cnt), None)
    assert mc is None and fg.shape == (CS.ACC_FRAMES, 1, CS.ACC_HW)
    err = float(np.abs(fg.cpu().numpy().astype(np.float64) - CS.sigmoid_mean_f64(acc[:, 0], cnt)).max())
    print("[cluster side] semseg_masks C = 1: fg within %.3g of the fp64 sigmoid" % err)
    assert err <= 1e-6
    for kind in ("logits", "probs", "argmax"):
        with pytest.raises(RuntimeError, match="single channel"):
            hip.semseg_masks(dev(acc), dev(cnt), kind)


def test_fg_mask_frames_at_the_threshold(hip):
    """Five frames seen by 0, 1, 2, 3 and 7 clips; sums planted at thr * count and one ulp to either side: the frame nobody saw is
    background, the others equal (acc / count > thr) in numpy fp32 exactly."""
    acc, counts = CS.mask_frames_case()
    m = hip.fg_mask_frames(dev(acc.reshape(len(counts), 7, 11)), dev(counts), CS.MASK_FRAMES_THR).cpu().numpy().reshape(acc.shape)
    assert not m[0].any()
    assert np.array_equal(m, CS.mask_frames_twin(acc, counts, CS.MASK_FRAMES_THR))


@pytest.mark.parametrize("HW", CS.FG_CLIP_HW)
@pytest.mark.parametrize("C", CS.FG_CLIP_CHANNELS)
def test_semseg_fg_clip_probability_and_mask(hip, C, HW):
    """C = 2 (softmax[1]), 3 and 43 (sigmoid of the last channel) with and without the probability output: the probability within 1e-6
    of fp64, the mask equal to (probability > thr) on the device's own probability bit for bit and to the fp64 reference's mask
    except within 2e-6 of thr (the host test caps that share at 1 in 1 000); planted logits of exactly 0 (0.5: not foreground) and
    +-inf (0, 1, and NaN -- mask 0 -- for softmax of (0, +inf), as in the reference)."""
    x = CS.fg_clip_case(C, HW)
    p_ref = CS.fg_clip_reference(x)[:, 0]
    mask, prob = hip.semseg_fg_clip(dev(x), CS.FG_CLIP_THR, want_prob=True)
    mask_only, none = hip.semseg_fg_clip(dev(x), CS.FG_CLIP_THR, want_prob=False)
    assert none is None and torch.equal(mask, mask_only)
    mask, prob = mask.cpu().numpy()[:, 0], prob.cpu().numpy()[:, 0]
    nan = np.isnan(p_ref)
    assert np.array_equal(np.isnan(prob), nan) and int(nan.sum()) == (1 if C == 2 else 0)
    err = float(np.abs(prob.astype(np.float64) - p_ref)[~nan].max())
    print("[cluster side] semseg_fg_clip C %d HW %d: probability within %.3g of fp64" % (C, HW, err))
    assert err <= 1e-6
    with np.errstate(invalid="ignore"):
        assert np.array_equal(mask, (prob > np.float32(CS.FG_CLIP_THR)).astype(np.uint8))
        keep = ~CS.fg_clip_band(p_ref)
        assert np.array_equal(mask[keep], (p_ref > CS.FG_CLIP_THR).astype(np.uint8)[keep])
    assert prob[0, 5] == 0.5 and mask[0, 5] == 0 and (prob[0, 6], prob[1, 7]) == (0.0, 1.0) and (mask[0, 6], mask[1, 7]) == (0, 1)
