"""The KITTI-MOTS evaluation restated by brute force on dense numpy masks: label maps and overlap counts from COCO RLE strings (decoded by
the suite's numpy RLE restatement, tests/data_oracle.py), pair tables, and the measure of include/stemseg_hip.h with plain loops over
masks.  It shares no code with stemseg_amd/evaluation/mots.py and does not import it.

The measure follows Voigtlaender et al., "MOTS", CVPR 2019; agreement with the official mots_tools is not tested anywhere."""
import math
from collections import OrderedDict

import numpy as np

from tests import data_oracle as do

CLASS_NAMES = OrderedDict(((1, "car"), (2, "ped")))
IGNORE = 10
KEYS = ("TP", "FP", "FN", "IDS", "M", "ignored")


# ------------------------------------------------------------------------------------------------ the kernels
def decode_labels(strings, plane_of_string, label_of_string, P, h, w):
    """-> (maps uint16 [P, h, w], overlap int32 [P], status uint8 [M]): what ``hip.rle_decode_labels`` documents."""
    maps, cover = np.zeros((P, h, w), np.uint16), np.zeros((P, h, w), np.int64)
    status = np.zeros(len(strings), np.uint8)
    for m, (s, q, label) in enumerate(zip(strings, plane_of_string, label_of_string)):
        plane, st = do.decode_strings([s], [0], 1, h, w)
        status[m] = st[0]
        if st[0] == 0:
            on = plane[0] != 0
            maps[q][on] = np.maximum(maps[q][on], label)
            cover[q] += on
    return maps, (cover > 1).reshape(P, -1).sum(1).astype(np.int32), status


def pair_counts(a, b, Ka, Kb):
    """-> int64 [T, Ka + 1, Kb + 1], one pixel at a time; labels above K count as 0."""
    T = a.shape[0]
    out = np.zeros((T, Ka + 1, Kb + 1), np.int64)
    for t in range(T):
        for la, lb in zip(a[t].reshape(-1).tolist(), b[t].reshape(-1).tolist()):
            out[t, la if la <= Ka else 0, lb if lb <= Kb else 0] += 1
    return out


# ------------------------------------------------------------------------------------------------ the measure, on dense masks
def decode(record):
    t, track, c, h, w, s = record
    assert do.string_status(s, h, w) == 0, record[:5]
    return do.decode_strings([s], [0], 1, h, w)[0][0] != 0


def frame_lists(records, n_frames, keep):
    frames = [[] for _ in range(n_frames)]
    for r in records:
        if r[2] in keep:
            frames[r[0]].append((r[1], r[2], decode(r)))
    return frames


def sequence_counts(result_records, gt_records, n_frames=None, notes=None):
    """-> {class name: {TP, FP, FN, IDS, M, ignored, ious}}.  notes: a list that receives (frame, class, kind, numbers) of every
    decision, for the tests that check what a case holds."""
    everything = list(result_records) + list(gt_records)
    counts = OrderedDict((n, dict([(k, 0) for k in KEYS] + [("ious", [])])) for n in CLASS_NAMES.values())
    if not everything:
        return counts
    if n_frames is None:
        n_frames = max(r[0] for r in everything) + 1
    res, gt = frame_lists(result_records, n_frames, (1, 2)), frame_lists(gt_records, n_frames, (1, 2, IGNORE))
    last = {}
    for t in range(n_frames):
        for side in (res[t], gt[t]):
            for x in range(len(side)):
                for y in range(x + 1, len(side)):
                    assert not (side[x][2] & side[y][2]).any(), "frame %d: overlapping masks" % t
        ignore = np.zeros((everything[0][3], everything[0][4]), bool)
        for _, c, m in gt[t]:
            if c == IGNORE:
                ignore = ignore | m
        for c, name in CLASS_NAMES.items():
            acc = counts[name]
            H = [(track, m) for track, cc, m in res[t] if cc == c and m.any()]
            G = [(track, m) for track, cc, m in gt[t] if cc == c and m.any()]
            matched_h, tp = set(), 0
            for g_track, g in G:
                for k, (h_track, h) in enumerate(H):
                    inter, ah, ag = int((h & g).sum()), int(h.sum()), int(g.sum())
                    if notes is not None:
                        notes.append((t, c, "pair", inter, ah, ag))
                    if 3 * inter > ah + ag:
                        tp += 1
                        matched_h.add(k)
                        acc["ious"].append(inter / float(ah + ag - inter))
                        if (c, g_track) in last and last[(c, g_track)] != h_track:
                            acc["IDS"] += 1
                        last[(c, g_track)] = h_track
            acc["TP"] += tp
            acc["M"] += len(G)
            acc["FN"] += len(G) - tp
            for k, (h_track, h) in enumerate(H):
                if k not in matched_h:
                    ign, ah = int((h & ignore).sum()), int(h.sum())
                    if notes is not None:
                        notes.append((t, c, "unmatched", ign, ah, 0))
                    if 2 * ign > ah:
                        acc["ignored"] += 1
                    else:
                        acc["FP"] += 1
    return counts


def summary(per_sequence):
    out, smotsa = OrderedDict(), []
    for name in CLASS_NAMES.values():
        tot = {k: sum(s[name][k] for s in per_sequence.values()) for k in KEYS}
        soft = math.fsum(v for s in per_sequence.values() for v in s[name]["ious"])
        M, TP = tot["M"], tot["TP"]
        out["sMOTSA-" + name] = (soft - tot["FP"] - tot["IDS"]) / float(M) if M else 0.0
        out["MOTSA-" + name] = float(TP - tot["FP"] - tot["IDS"]) / float(M) if M else 0.0
        out["MOTSP-" + name] = soft / float(TP) if TP else 0.0
        if M > 0:
            smotsa.append(out["sMOTSA-" + name])
    out["sMOTSA-mean"] = sum(smotsa) / float(len(smotsa)) if smotsa else 0.0
    out["sequences"] = OrderedDict((seq, OrderedDict((name, {k: s[name][k] for k in KEYS}) for name in CLASS_NAMES.values()))
                                   for seq, s in per_sequence.items())
    return out


# ------------------------------------------------------------------------------------------------ tables for the evaluator's host half
def frame_tables(result_records, gt_records, n_frames):
    """Per frame (table, res_meta, gt_meta) as the evaluator builds them: labels local to the frame, in ascending track order."""
    out = []
    for t in range(n_frames):
        sides = []
        for records, keep in ((result_records, (1, 2)), (gt_records, (1, 2, IGNORE))):
            sides.append(sorted(((r[1], r[2], decode(r)) for r in records if r[0] == t and r[2] in keep), key=lambda x: x[0]))
        h, w = everything_size(result_records, gt_records)
        maps = []
        for side in sides:
            m = np.zeros((1, h, w), np.uint16)
            for n, (_, _, mask) in enumerate(side, 1):
                m[0][mask] = n
            maps.append(m)
        table = pair_counts(maps[0], maps[1], max(1, len(sides[0])), max(1, len(sides[1])))[0]
        out.append((table, [(tr, c) for tr, c, _ in sides[0]], [(tr, c) for tr, c, _ in sides[1]]))
    return out


def everything_size(result_records, gt_records):
    r = (list(gt_records) + list(result_records))[0]
    return r[3], r[4]
