"""The YouTube-VIS evaluation restated by brute force on dense numpy masks with plain loops: the tables of ``hip.rle_pair_inter``, the
track IoU, the matching and the accumulation of include/stemseg_hip.h.  Strings come from and go to masks through tests/writer_oracle.py
(``encode``, ``decode``, ``counts_to_string``, ``string_to_counts``); the status of a string is tests/data_oracle.py's restatement of the
header's list.  It shares no code with stemseg_amd/evaluation/ytvis.py and does not import it.

The measure is COCOeval's lifted to tracks (Yang et al., "Video Instance Segmentation", ICCV 2019); agreement with the official server
and toolkit is not tested anywhere."""
import math
from collections import OrderedDict

import numpy as np

from tests import data_oracle as do
from tests import writer_oracle as wo

THRESHOLDS =[float(v) for v in np.linspace(0.5, 0.95, 10)]
RECALL_POINTS = [float(v) for v in np.linspace(0.0, 1.0, 101)]
MAX_DETS = (1, 10, 100)


# ------------------------------------------------------------------------------------------------ strings and the kernel's tables
mask_string = do.mask_string


def string_mask(s, h, w):
    return wo.decode(wo.string_to_counts(s if isinstance(s, str) else s.decode("ascii")), h, w) != 0


def pair_tables(strings, pairs, h, w):
    """-> (area int64 [M], inter int64 [n_pairs], status uint8 [M]): what ``hip.rle_pair_inter`` documents, one pixel at a time."""
    status = np.asarray([do.string_status(s, h, w) for s in strings], np.uint8).reshape(-1)
    masks = [string_mask(s, h, w) if st == 0 else None for s, st in zip(strings, status)]
    area = np.asarray([0 if m is None else int(m.sum()) for m in masks], np.int64).reshape(-1)
    inter = np.zeros(len(pairs), np.int64)
    for k, (a, b) in enumerate(pairs):
        if masks[a] is not None and masks[b] is not None:
            inter[k] = int(np.logical_and(masks[a], masks[b]).sum())
    return area, inter, status


# ------------------------------------------------------------------------------------------------ the measure, on dense masks
def track_masks(track, h, w):
    """The T masks of a track, a missing one all False."""
    out = []
    for seg in track["segmentations"]:
        if seg is None:
            out.append(np.zeros((h, w), bool))
        else:
            s = seg["counts"] if isinstance(seg, dict) else seg
            assert do.string_status(s, h, w) == 0
            out.append(string_mask(s, h, w))
    return out


def iou_of_tracks(d_masks, g_masks, crowd):
    inter = sum(int((a & b).sum()) for a, b in zip(d_masks, g_masks))
    if crowd:
        union = sum(int(a.sum()) for a in d_masks)
    else:
        union = sum(int(a.sum()) + int(b.sum()) - int((a & b).sum()) for a, b in zip(d_masks, g_masks))
    return (float(inter) / float(union) if union else 0.0), inter, union


def video_records(results, gt_tracks, size, notes=None):
    """-> {category: dict(scores, matched [10][n], ignored [10][n], n_gt, n_crowd)}.  notes: receives (category, result, ground truth,
    inter, union, iou) of every pair looked at."""
    h, w = size
    out = OrderedDict()
    cats = sorted(set([int(r["category_id"]) for r in results] + [int(g["category_id"]) for g in gt_tracks]))
    for c in cats:
        dets = [(i, r) for i, r in enumerate(results) if int(r["category_id"]) == c]
        dets = sorted(dets, key=lambda ir: (-float(ir[1]["score"]), ir[0]))[:100]          # descending, ties in the file's order
        gts = [(j, g) for j, g in enumerate(gt_tracks) if int(g["category_id"]) == c]
        gts = [x for x in gts if not x[1].get("iscrowd", 0)] + [x for x in gts if x[1].get("iscrowd", 0)]
        crowd = [bool(g.get("iscrowd", 0)) for _, g in gts]
        d_masks = [track_masks(r, h, w) for _, r in dets]
        g_masks = [track_masks(g, h, w) for _, g in gts]
        iou = [[0.0] * len(gts) for _ in dets]
        for a in range(len(dets)):
            for b in range(len(gts)):
                iou[a][b], inter, union = iou_of_tracks(d_masks[a], g_masks[b], crowd[b])
                if notes is not None:
                    notes.append((c, dets[a][0], gts[b][0], inter, union, iou[a][b]))
        matched, ignored = [], []
        for thr in THRESHOLDS:
            taken = [False] * len(gts)
            row_m, row_i = [], []
            for a in range(len(dets)):
                best, pick = min(thr, 1 - 1e-10), None
                for b in range(len(gts)):
                    if taken[b] and not crowd[b]:
                        continue
                    if pick is not None and not crowd[pick] and crowd[b]:
                        break
                    if iou[a][b] < best:
                        continue
                    best, pick = iou[a][b], b
                row_m.append(pick is not None)
                row_i.append(pick is not None and crowd[pick])
                if pick is not None:
                    taken[pick] = True
            matched.append(row_m)
            ignored.append(row_i)
        out[c] = dict(scores=[float(r["score"]) for _, r in dets], matched=matched, ignored=ignored, n_gt=crowd.count(False),
                      n_crowd=crowd.count(True))
    return out


def mean(values):
    return math.fsum(values) / float(len(values)) if values else -1.0


def summary(videos):
    """{video: ``video_records``} -> AP, AP50, AP75, AR1, AR10 and per_category."""
    cats = sorted(set(c for rec in videos.values() for c in rec))
    precision, recall = {}, {}
    for c in cats:
        recs = [rec[c] for rec in videos.values() if c in rec]
        n_gt = sum(r["n_gt"] for r in recs)
        if n_gt == 0:
            continue
        for max_det in MAX_DETS:
            for k in range(len(THRESHOLDS)):
                merged = []
                for v, r in enumerate(recs):
                    for i in range(min(max_det, len(r["scores"]))):
                        merged.append((-r["scores"][i], v, i, r["matched"][k][i], r["ignored"][k][i]))
                merged.sort(key=lambda x: x[:3])                                           # by score, ties in (video, rank) order: stable
                tp = fp = 0
                rc, pr = [], []
                for _, _, _, m, ig in merged:
                    if not ig:
                        tp += 1 if m else 0
                        fp += 0 if m else 1
                    rc.append(float(tp) / float(n_gt))
                    pr.append(float(tp) / (float(fp) + float(tp) + float(np.spacing(1))))
                for i in range(len(pr) - 2, -1, -1):
                    pr[i] = max(pr[i], pr[i + 1])
                samples = []
                for point in RECALL_POINTS:
                    i = 0
                    while i < len(rc) and rc[i] < point:                                   # searchsorted(side="left")
                        i += 1
                    samples.append(pr[i] if i < len(pr) else 0.0)
                precision[(c, max_det, k)] = samples
                recall[(c, max_det, k)] = rc[-1] if rc else 0.0
    counted = [c for c in cats if (c, 100, 0) in precision]
    K = range(len(THRESHOLDS))
    out = OrderedDict()
    out["AP"] = mean([v for c in counted for k in K for v in precision[(c, 100, k)]])
    out["AP50"] = mean([v for c in counted for v in precision[(c, 100, 0)]])
    out["AP75"] = mean([v for c in counted for v in precision[(c, 100, 5)]])
    out["AR1"] = mean([recall[(c, 1, k)] for c in counted for k in K])
    out["AR10"] = mean([recall[(c, 10, k)] for c in counted for k in K])
    out["per_category"] = OrderedDict((c, mean([v for k in K for v in precision[(c, 100, k)]])) for c in counted)
    return out


def evaluate(videos):
    """{video: (results, gt_tracks, size)} -> the summary."""
    return summary(OrderedDict((vid, video_records(res, gt, size)) for vid, (res, gt, size) in videos.items()))


# ------------------------------------------------------------------------------------------------ tables for the evaluator's host half
def video_tables(results, gt_tracks, size):
    """-> (res_meta, gt_meta, area_d [D, T], area_g [G, T], inter [D, G, T]) as the evaluator builds them from the kernel's output; the
    cells of pairs of different categories stay 0 (the evaluator never lists those pairs)."""
    h, w = size
    T = len((results + gt_tracks)[0]["segmentations"]) if results or gt_tracks else 0
    d_masks, g_masks = [track_masks(r, h, w) for r in results], [track_masks(g, h, w) for g in gt_tracks]
    area_d = np.asarray([[int(m.sum()) for m in ms] for ms in d_masks], np.int64).reshape(len(results), T)
    area_g = np.asarray([[int(m.sum()) for m in ms] for ms in g_masks], np.int64).reshape(len(gt_tracks), T)
    inter = np.zeros((len(results), len(gt_tracks), T), np.int64)
    for d, r in enumerate(results):
        for g, gt in enumerate(gt_tracks):
            if int(r["category_id"]) == int(gt["category_id"]):
                inter[d, g] = [int((a & b).sum()) for a, b in zip(d_masks[d], g_masks[g])]
    return ([(float(r["score"]), int(r["category_id"])) for r in results],
            [(int(g["category_id"]), int(g.get("iscrowd", 0))) for g in gt_tracks], area_d, area_g, inter)
