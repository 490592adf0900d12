"""Inputs of tests/test_gpu_cluster_side.py (the clustering / stitching / accumulator kernels at every layout and edge) and the numpy
twins that tests/oracle_ops.py does not have.  Pure numpy + torch CPU: tests/test_cluster_side_host.py asserts on the CPU, for every case
built here, what the GPU tests rely on (threshold margin, the oracle's K, where the equal seeds sit, the share of pixels left out).
Nothing here depends on what a kernel returns."""
import functools
import os

import numpy as np
import torch

from oracle import pipeline as opipe
from oracle.clusterer import sequential_clustering
from tests import synth

F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stemseg_hip.h")

# ------------------------------------------------------------------------------------------------ 1. clustering
MARGIN = 1e-4          # smallest allowed |p - 0.5| and |p - 0.3| of any oracle probability: exact labels may be demanded of every point
PROB_TOL = 1e-6        # probabilities and stds vs the oracle (the bound of test_cluster_adversarial_band)

# (E, Ev, free stds, instances the oracle has to find).  E = 1 keeps one coordinate of synth_cluster_case's 2 x 2 lattice: the blobs of
# lattice row 0 share it, so 3 boxes are 2 instances; every other layout separates its 9 boxes.
LAYOUTS = [(1, 1, (), 2), (2, 1, (.3,), 9), (2, 0, (.3, .3), 9), (3, 3, (), 9), (4, 2, (.3, .3), 9), (5, 3, (.3, .3), 9),
           (5, 2, (.3, .3, .3), 9), (6, 3, (.3, .3, .3), 9), (6, 2, (.3, .3, .3, .3), 9), (7, 4, (.3, .3, .3), 9),
           (8, 4, (.3, .3, .3, .3), 9)]
LAYOUT_IDS = ["E%d-Ev%d" % (l[0], l[1]) for l in LAYOUTS]


def _case(emb, bw, seed, stds, max_instances=20, min_seed=0.8, label_start=1):
    return dict(emb=np.ascontiguousarray(emb, F32), bw=np.ascontiguousarray(bw, F32), seed=np.ascontiguousarray(seed, F32).reshape(-1),
                stds=tuple(stds), max_instances=int(max_instances), min_seed=float(min_seed), label_start=int(label_start))


def run_oracle(case, n=None):
    """-> (labels, meta with masks and probs) of the first n points (all by default)."""
    n = case["emb"].shape[0] if n is None else n
    return sequential_clustering(case["emb"][:n], case["bw"][:n], case["seed"][:n], label_start=case["label_start"],
                                 min_seediness=case["min_seed"], free_dim_stds=case["stds"], max_instances=case["max_instances"],
                                 return_masks=True, return_probs=True)


def margin(meta):
    """Smallest distance of any probability of any round from the two thresholds (inf without rounds)."""
    m = np.inf
    for p in meta["instance_probs"]:
        m = min(m, float(np.abs(p - F32(0.5)).min()), float(np.abs(p - F32(0.3)).min()))
    return m


def oracle_summary(case, labels, meta):
    """K / exhausted / n_unassigned_last as StemsegClusterMeta states them, replayed from the oracle's labels and primary masks: the
    count at the last loop header that was evaluated."""
    K, n = len(meta["instance_labels"]), case["emb"].shape[0]
    claimed = np.zeros(n, bool)
    header_counts = []
    for k in range(K):
        header_counts.append(int((~claimed).sum()))
        claimed |= meta["instance_masks"][k]
    exhausted = int(K == case["max_instances"])
    n_un_last = header_counts[-1] if exhausted else int((~claimed).sum())
    if K == 0:
        n_un_last = n
    return dict(K=K, exhausted=exhausted, n_unassigned_last=n_un_last)


@functools.lru_cache(maxsize=None)
def layout_case(E, Ev, stds):
    K = 3 if E == 1 else 9
    emb, bw, sd, fg = synth.synth_cluster_case(3, 24, 40, K, E=E, Ev=Ev, seed=40 + E)
    e, b, s, _ = opipe.gather_fg(emb, bw, sd, fg)
    return _case(e, b, s, stds)


MAX_INSTANCES = [(64, 30, 0), (7, 7, 1), (1, 1, 1)]           # (max_instances, K the oracle finds, exhausted)


@functools.lru_cache(maxsize=None)
def max_instances_case(max_instances):
    emb, bw, sd, fg = synth.synth_cluster_case(3, 24, 40, 30, seed=44)
    e, b, s, _ = opipe.gather_fg(emb, bw, sd, fg)
    return _case(e, b, s, (.3, .3), max_instances=max_instances)


def _blob_points(rs, which, centers, noise):
    n = which.shape[0]
    emb = (10.0 + 3.0 * rs.standard_normal((n, 4))).astype(F32)            # outliers (which == -1): far from every blob
    inb = which >= 0
    emb[inb] = (centers[which[inb]] + noise * rs.standard_normal((int(inb.sum()), 4))).astype(F32)
    bw = (20 + rs.uniform(0, 5, (n, 2))).astype(F32)
    return emb, bw


def _lattice(k):
    return np.array([[(i % 4) - 1.5, (i // 4) - 1.0, 0.6 * ((i * 7) % 5 - 2), 0.6 * ((i * 3) % 5 - 2)] for i in range(k)], F32)


TIE_N, TIE_BLOBS = 300_000, 12
TIE_TOP = [16, 14, 16, 15, 16, 15, 14, 16, 15, 16, 15, 16]       # each blob's highest seediness level (sixteenths)
TIE_OFFSETS = (0, 1, 64, 256, 293)                                # the winner, then: next lane, next wave, the same thread's second point
#                                                                   (a lone set of 300 000 points is cut into 1024 blocks of 293, whose first
#                                                                   37 threads own two points 256 apart) and the next block -- all equal


@functools.lru_cache(maxsize=None)
def tie_case():
    """300 000 points, 12 blobs laid out one after the other with 8 % outliers sprinkled in, seediness in sixteenths.  Every blob's best
    level occurs at about 1 500 of its points; the lowest-index one (the winner) sits >= 500 points into the blob, where its index
    modulo 293 is below 37, and the points TIE_OFFSETS behind it carry the same value.  Blobs share their best level in groups, so a
    round picks among thousands of equal maxima spread over the whole index range.  -> (case, winners per blob)."""
    rs = np.random.RandomState(4242)
    n, k = TIE_N, TIE_BLOBS
    per = n // k
    which = np.repeat(np.arange(k), per)
    which[rs.uniform(size=n) < 0.08] = -1
    winners = []
    for b in range(k):
        w = b * per + 500
        while w % 293 >= 37:
            w += 1
        winners.append(w)
        for o in TIE_OFFSETS:
            which[w + o] = b
    emb, bw = _blob_points(rs, which, _lattice(k), 0.03)
    lev = rs.randint(0, 16, n)
    lev[which < 0] = rs.randint(0, 4, int((which < 0).sum()))                # outliers never seed an instance
    for b in range(k):
        idx = np.flatnonzero(which == b)
        lev[idx] = np.minimum(lev[idx], TIE_TOP[b] - 1)
        after = idx[idx > winners[b]]
        lev[after[rs.uniform(size=after.size) < 1 / 16.]] = TIE_TOP[b]
        for o in TIE_OFFSETS:
            lev[winners[b] + o] = TIE_TOP[b]
    seed = (lev / 16.0).astype(F32)                                           # exact in fp32
    return _case(emb, bw, seed, (.3, .3)), winners


def expected_winners(case, meta):
    """Per round: the lowest index among the unassigned points whose seediness equals their maximum (recomputed from the oracle's
    primary masks, not taken from its argmax)."""
    claimed = np.zeros(case["emb"].shape[0], bool)
    out = []
    for m in meta["instance_masks"]:
        idx = np.flatnonzero(~claimed)
        out.append(int(idx[np.flatnonzero(case["seed"][idx] == case["seed"][idx].max())[0]]))
        claimed |= m
    return out


def small_set(n, k, seed):
    rs = np.random.RandomState(seed)
    which = rs.randint(0, k, n)
    which[rs.uniform(size=n) < 0.05] = -1
    emb, bw = _blob_points(rs, which, _lattice(k), 0.03)
    sd = np.where(which >= 0, rs.uniform(0.3, 1.0, n), rs.uniform(0, 0.2, n)).astype(F32)
    return _case(emb, bw, sd, (.3, .3))


N_POINTS_MAX = 5000
N_POINTS_DEV = [0, 1, 4997, 5000, 9999]


@functools.lru_cache(maxsize=None)
def n_points_case():
    return small_set(N_POINTS_MAX, 6, 77)


# ------------------------------------------------------------------------------------------------ 2. gather / compaction
GATHER_SHAPES = [(7, 5, 9), (3, 31, 33), (2, 32, 32), (1, 1, 1)]
GATHER_DENSITIES = [0.0, 1.0, 0.4]
GATHER_LAYOUTS = [(5, 3), (1, 1)]
CARRY_SHAPE = (2, 700, 750)                                      # V = 1 050 000: 1 026 blocks of 1 024 voxels, two passes of the scan
SCRATCH_CASES = [(8, 33, 65), CARRY_SHAPE]                       # V = 17 160 and the carry shape
SCRATCH_DOC = "16 * (V/1024 + 2)"                                # the header's wording of scratch_bytes_documented


def fg_mask(T, H, W, density, seed=0):
    rs = np.random.RandomState(900 + seed)
    return (rs.uniform(size=(T, H, W)) < density).astype(np.uint8)


def head_outputs(T, H, W, E, Ev, seed=0):
    rs = np.random.RandomState(700 + seed)
    return (rs.standard_normal((E, T, H, W)).astype(F32), rs.uniform(20, 25, (Ev, T, H, W)).astype(F32),
            rs.uniform(0, 1, (1, T, H, W)).astype(F32))


def compact_twin(fg):
    """voxel_index [N] and frame_offsets [T + 1] of a mask (masks_to_coord_list order: frame-major, row-major)."""
    f = np.asarray(fg).reshape(fg.shape[0], -1).astype(bool)
    return np.flatnonzero(f.reshape(-1)).astype(np.int32), np.concatenate([[0], np.cumsum(f.sum(1))]).astype(np.int64)


def scratch_bytes_needed(V):
    """What stemseg_hip_fg_gather / _fg_compact lay out: [nb] int32 counts, padded to 8 bytes, then [nb + 1] int64 offsets."""
    nb = -(-V // 1024)
    return (4 * nb + 7) // 8 * 8 + 8 * (nb + 1)


def scratch_bytes_documented(V):
    """What include/stemseg_hip.h asks a caller to provide (SCRATCH_DOC)."""
    return 16 * (V // 1024 + 2)


# ------------------------------------------------------------------------------------------------ 3. label statistics
OVERLAP_CASES = [(95, 127), (96, 127), (0, 40), (40, 0)]
OVERLAP_LDS_CELLS = 12288                                        # Ka * Kb + Ka + Kb up to here is counted in LDS


def overlap_case(Ka, Kb, n=50_000):
    """-> (la, lb, ids_a, ids_b): 20 % outliers, every id of both sides occurs, plus ids inside a LUT's range that it does not list and
    ids at and beyond its end (the LUT of HipChainerOps.overlap_counts has max(ids) + 2 entries: label max(ids) + 1 is lut_len - 1)."""
    rs = np.random.RandomState(1000 * Ka + Kb)

    def side(K):
        ids = sorted(rs.choice(np.arange(1, 3 * K + 2), K, replace=False).tolist()) if K else []
        top = max(ids) if ids else 0
        stray = [i for i in range(1, top) if i not in ids][:7] + [top + 1, top + 2, top + 1000, 2 ** 40]
        pool = np.array(ids + stray, np.int64)
        lab = pool[rs.randint(0, pool.size, n)]
        lab[:pool.size] = pool                                   # every id and every stray occurs
        lab[rs.uniform(size=n) < 0.2] = -1
        return lab, ids
    la, ids_a = side(Ka)
    lb, ids_b = side(Kb)
    return la, lb, ids_a, ids_b


def presence_twin(labels, cap):
    labels = np.asarray(labels, np.int64).reshape(-1)
    present = np.zeros(cap + 1, np.uint8)
    inr = labels[(labels >= 0) & (labels < cap)]
    present[inr] = 1
    present[cap] = 1 if (labels < 0).any() else 0
    pos = labels[labels >= 0]
    return present, int(pos.max()) + 1 if pos.size else 0


PRESENCE_CAPS = [0, 1, 300]


def presence_arrays(cap):
    """name -> list of int64 arrays (one call each, accumulated)."""
    rs = np.random.RandomState(31 + cap)
    mixed = np.concatenate([rs.randint(0, cap + 5, 4000), [cap, cap + 1, cap + 700], np.full(50, -1)]).astype(np.int64)
    rs.shuffle(mixed)
    return {"mixed": [mixed], "beyond_cap_only": [np.array([cap, cap + 9, 2 ** 40], np.int64)], "negative_only": [np.array([-1, -5, -1], np.int64)],
            "empty": [np.zeros(0, np.int64)],
            "three_arrays": [mixed[:1500], np.zeros(0, np.int64), mixed[1500:1501], mixed[1501:]]}


def relabel_twin(labels, mapping):
    labels, mapping = np.asarray(labels, np.int64), np.asarray(mapping, np.int64)
    out = labels.copy()
    k = labels + 1
    ok = (k >= 0) & (k < mapping.size)
    out[ok] = mapping[k[ok]]
    return out


RELABEL_MAP_LENS = [0, 1, 9]


def relabel_case(map_len):
    rs = np.random.RandomState(50 + map_len)
    pool = np.array([-5, -1] + list(range(0, map_len + 4)), np.int64)
    labels = pool[rs.randint(0, pool.size, 3000)]
    labels[:pool.size] = pool
    return labels, rs.randint(1, 10_000, map_len).astype(np.int64) * 1000           # values no label has


def codes_twin(labels, vox, n, label_start, V):
    """stemseg_hip_labels_to_codes: 0 everywhere, then for the first n points 255 (negative label), label - label_start + 1 when that
    is in 1 .. 254, else 254 (out of range)."""
    codes = np.zeros(V, np.uint8)
    lab = np.asarray(labels, np.int64)[:n]
    c = lab - label_start + 1
    codes[np.asarray(vox)[:n]] = np.where(lab < 0, 255, np.where((c < 1) | (c > 254), 254, c)).astype(np.uint8)
    return codes


CODE_BINS = [3, 66]
CODE_LABEL_START = 7


def codes_case(B):
    """Three 8 x 8 frames; labels on both sides of every clamp: negative, below label_start, codes below / at / above B - 1, at
    label_start + 253 and above it; the last five points lie beyond n_points_dev.  -> fg, labels [n], n_dev."""
    rs = np.random.RandomState(60 + B)
    fg = fg_mask(3, 8, 8, 0.6, seed=B)
    vox, offs = compact_twin(fg)
    n = int(offs[-1])
    ls = CODE_LABEL_START
    pool = np.array([-1, -3, 0, ls - 1, ls, ls + 1, ls + B - 3, ls + B - 2, ls + B - 1, ls + 100, ls + 252, ls + 253, ls + 254, ls + 5000, 2 ** 40],
                    np.int64)
    labels = pool[rs.randint(0, pool.size, n)]
    labels[:pool.size] = pool
    return fg, labels, n - 5


MANY_ITEMS = 65536 + 3
MANY_PLANES, MANY_HW, MANY_B = 6, 64, 3


@functools.lru_cache(maxsize=None)
def many_items_case():
    """65 539 items (two launches of 65 535 and 4) over 6 code planes of 64 voxels at B = 3.  -> codes [6, 64], plane_a, plane_b [n],
    vox (all planes' foreground, plane-major), items [n, 5], lut [n, 3], n_out."""
    rs = np.random.RandomState(65)
    n = MANY_ITEMS
    pool = np.array([0, 0, 1, 1, 2, 3, 100, 254, 255], np.uint8)
    codes = pool[rs.randint(0, pool.size, (MANY_PLANES, MANY_HW))]
    plane_a = rs.randint(-1, MANY_PLANES, n).astype(np.int32)
    plane_b = rs.randint(0, MANY_PLANES, n).astype(np.int32)
    plane_a[-4:], plane_b[-4:] = [-1, 2, 5, 0], [5, 0, 3, 4]     # the second launch's items differ from one another
    vox, offs = compact_twin(codes.reshape(MANY_PLANES, 8, 8) != 0)
    plane = rs.randint(0, MANY_PLANES, n)
    avail = (offs[1:] - offs[:-1])[plane]
    skip = rs.randint(0, 4, n)
    cnt = np.clip(np.minimum(rs.randint(0, 9, n), avail - skip), 0, None)
    dst = np.concatenate([[0], np.cumsum(cnt)])
    items = np.stack([offs[plane] + np.minimum(skip, avail), cnt, plane * MANY_HW, plane, dst[:-1]], 1).astype(np.int64)
    lut = rs.randint(-1, 1 << 40, (n, MANY_B)).astype(np.int64)
    return codes, plane_a, plane_b, vox, items, lut, int(dst[-1])


# ------------------------------------------------------------------------------------------------ 4. accumulators and masks
ACC_CHANNELS = [1, 3, 5]
ACC_T, ACC_FRAMES, ACC_HW = 3, 4, 64
ACC_PATHS = ["scalar_hw63", "scalar_acc_misaligned", "scalar_clip_misaligned", "vector"]
ACC_CLIPS = [[0, 1, 2], [2, 2, 3], [-1, 0, -1]]      # frame of every slot; the second repeats a frame (split into two calls), the third skips slots


def accumulate_case(C):
    rs = np.random.RandomState(80 + C)
    return [rs.standard_normal((C, ACC_T, 1, ACC_HW)).astype(F32) * F32(10) for _ in ACC_CLIPS]


def accumulate_twin(clips, hw):
    """Sequential fp32 adds in slot order, starting from the float 0."""
    C = clips[0].shape[0]
    acc, counts = np.zeros((ACC_FRAMES, C, 1, hw), F32), [0] * ACC_FRAMES
    for x, sub in zip(clips, ACC_CLIPS):
        for i, t in enumerate(sub):
            if t >= 0:
                acc[t] = acc[t] + x[:, i, :, :hw]
                counts[t] += 1
    return acc, counts


def sigmoid_mean_f64(acc, counts):
    """sigmoid in fp64 of the fp32 mean acc[f] / counts[f]."""
    mean = (np.asarray(acc, F32) / np.asarray(counts, F32).reshape(-1, *([1] * (np.ndim(acc) - 1)))).astype(F32)
    return 1.0 / (1.0 + np.exp(-mean.astype(np.float64)))


MASK_FRAMES_COUNTS = [0, 1, 2, 3, 7]
MASK_FRAMES_HW = 77
MASK_FRAMES_THR = 0.3                                 # not a power of two: thr * count rounds, acc / count rounds again


def mask_frames_case():
    """acc [5, 77]: random sums, and in every frame the fp32 product thr * count with its two fp32 neighbours."""
    rs = np.random.RandomState(90)
    acc = np.stack([rs.uniform(0, 0.6, MASK_FRAMES_HW).astype(F32) * F32(max(c, 1)) for c in MASK_FRAMES_COUNTS])
    for f, c in enumerate(MASK_FRAMES_COUNTS):
        at = F32(MASK_FRAMES_THR) * F32(c)
        acc[f, 10:13] = [np.nextafter(at, F32(-np.inf)), at, np.nextafter(at, F32(np.inf))]
    acc[0, 20] = F32(5.0)                             # a large sum in the frame no clip contains
    return acc, np.array(MASK_FRAMES_COUNTS, F32)


def mask_frames_twin(acc, counts, thr):
    out = np.zeros(acc.shape, np.uint8)
    for f, c in enumerate(counts):
        if c > 0:
            out[f] = (acc[f] / F32(c)) > F32(thr)      # fp32 division, correctly rounded on both sides
    return out


FG_CLIP_CHANNELS = [2, 3, 43]
FG_CLIP_HW = [63, 4096]
FG_CLIP_T = 2
FG_CLIP_THR = 0.5
FG_CLIP_BAND = 2e-6                                    # pixels whose fp64 probability is this close to thr may differ in the mask
FG_CLIP_LEFT_OUT = 1e-3                                # ... and may be at most this share of the pixels


def fg_clip_case(C, HW):
    """logits [C, 2, 1, HW] = 3 * randn with planted values in the channels that decide the foreground: exactly 0 (p = 0.5, not > 0.5)
    and +-inf.  With two channels (softmax[1] of (x0, x1)): (0, 0) -> 0.5, (0, -inf) -> 0, (-inf, 0) -> 1, (0, +inf) -> NaN (inf - inf,
    as in the reference's softmax), mask 0."""
    rs = np.random.RandomState(100 * C + HW % 97)
    x = (3 * rs.standard_normal((C, FG_CLIP_T, 1, HW))).astype(F32)
    if C == 2:
        x[:, 0, 0, 5], x[:, 0, 0, 6], x[:, 1, 0, 7], x[:, 1, 0, 8] = [0, 0], [0, -np.inf], [-np.inf, 0], [0, np.inf]
    else:
        x[C - 1, 0, 0, 5], x[C - 1, 0, 0, 6], x[C - 1, 1, 0, 7] = 0, -np.inf, np.inf
    return x


def fg_clip_reference(x):
    """fp64 foreground probability [T, 1, HW]: softmax[1] with two channels, sigmoid of the last channel otherwise."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if x.shape[0] == 2:
            m = np.maximum(x[0], x[1])
            e0, e1 = np.exp(x[0] - m), np.exp(x[1] - m)
            return e1 / (e0 + e1)
        return 1.0 / (1.0 + np.exp(-x[-1]))


def fg_clip_band(p_ref):
    """Pixels left out of the mask comparison with the fp64 reference: within FG_CLIP_BAND of thr but not exactly thr (there the mask
    is 0 on both sides: sigmoid(0) and softmax of equal logits are exactly 0.5 in fp32 too)."""
    return (np.abs(p_ref - FG_CLIP_THR) < FG_CLIP_BAND) & (p_ref != FG_CLIP_THR)


def to_torch(a):
    return torch.from_numpy(np.ascontiguousarray(a))
