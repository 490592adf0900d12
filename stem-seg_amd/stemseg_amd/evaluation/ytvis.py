"""YouTube-VIS measures AP, AP50, AP75, AR1 and AR10 of a result (mask AP over TRACKS), counted on the device by ``hip.rle_pair_inter``
(csrc/data_loader.hip: the intersection of two COCO RLE strings on their runs, no plane) and finished on the host: integer sums over the
frames, the matching and the accumulation in fp64.

The measure is DEFINED in include/stemseg_hip.h and here: COCOeval's (Lin et al., "Microsoft COCO", ECCV 2014; pycocotools' evaluate /
accumulate / summarize) lifted to tracks as in Yang et al., "Video Instance Segmentation", ICCV 2019.  The youtubevos cocoapi and the
evaluation server are not available to this project, so agreement with their numbers is UNVERIFIED.  tests/ytvis_eval_oracle.py restates
it on dense numpy masks.

    a result track: {video_id, score, category_id, segmentations: T entries, each {"size": [h, w], "counts": string} or None};
    a ground-truth track: {category_id, iscrowd (default 0), segmentations: T strings / such dicts / None}.  A missing mask is empty.
    track IoU of result d and ground truth g: I = sum_t inter_t; U = sum_t (area_d,t + area_g,t - inter_t), for a crowd g
      U = sum_t area_d,t; iou = I / U in fp64, 0.0 when U = 0.  Pairs only within one video and one category.
    IoU thresholds linspace(0.5, 0.95, 10); recall thresholds linspace(0, 1, 101); maxDets (1, 10, 100); NO area ranges.
    matching per (video, category): results by score descending (stable), the first 100; ground truth non-crowd first (stable); per
      threshold t every result in turn takes the ground truth of highest IoU >= the running bound, which starts at min(t, 1 - 1e-10),
      among those not taken (a crowd may be taken again); it never trades a non-crowd match for a crowd one; matched to a crowd it is
      ignored; unmatched it is an FP.
    accumulation per (category, threshold, maxDet): from every video the first maxDet results of that one matching, merged by score
      (descending, stable); cumulative TP and FP over the non-ignored; recall = TP / n_gt (non-crowd ground-truth tracks); precision =
      TP / (TP + FP + spacing(1)), made monotone from the right, sampled at the recall points with searchsorted(side="left"), 0 beyond
      the last.  A category with n_gt = 0 is left out.
    AP: the mean over thresholds, categories and recall points at maxDet 100; AP50 / AP75: at one threshold; AR1 / AR10: the mean final
      recall over thresholds and categories at that maxDet; -1.0 when no category counts.  Every mean is math.fsum / the number of terms.
"""
import json
import math
import os
import tempfile
from collections import OrderedDict

import numpy as np
import torch

from .. import hip

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)
RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101)
MAX_DETS = (1, 10, 100)
FIGURES = ("AP", "AP50", "AP75", "AR1", "AR10")


# ------------------------------------------------------------------------------------------------ the host half
def track_iou(inter, area_d, area_g, crowd):
    """The integers summed over the frames -> the track IoU in fp64."""
    union = int(area_d) if crowd else int(area_d) + int(area_g) - int(inter)
    return float(int(inter)) / float(union) if union else 0.0


def match_video(res_meta, gt_meta, area_d, area_g, inter):
    """The integer tables of one video -> its matching records.  res_meta: [(score, category)] per result track, in the file's order;
    gt_meta: [(category, iscrowd)] per ground-truth track; area_d int [D, T], area_g int [G, T]: the masks' areas (0: no mask);
    inter int [D, G, T]: the intersections (only cells of one category are read).  -> {category: {"scores": [n], "matched": bool
    [thresholds, n], "ignored": bool [thresholds, n], "n_gt": the non-crowd tracks, "n_crowd"}} with n <= 100 results in matching order."""
    def table(a, *lead):                                         # (a side without a track leaves the number of frames open)
        a, n = np.asarray(a, dtype=np.int64), int(np.prod(lead))
        return a.reshape(lead + (a.size // n if n else 0,))
    area_d, area_g = table(area_d, len(res_meta)), table(area_g, len(gt_meta))
    inter = table(inter, len(res_meta), len(gt_meta))
    out = OrderedDict()
    for c in sorted(set(int(m[1]) for m in res_meta) | set(int(m[0]) for m in gt_meta)):
        ds = [d for d, (_, cd) in enumerate(res_meta) if int(cd) == c]
        ds = sorted(ds, key=lambda d: -float(res_meta[d][0]))[:MAX_DETS[-1]]
        gs = [g for g, (cg, _) in enumerate(gt_meta) if int(cg) == c]
        gs = sorted(gs, key=lambda g: 1 if gt_meta[g][1] else 0)
        crowd = [bool(gt_meta[g][1]) for g in gs]
        ious = [[track_iou(inter[d, g].sum(), area_d[d].sum(), area_g[g].sum(), crowd[j]) for j, g in enumerate(gs)] for d in ds]
        matched = np.zeros((len(IOU_THRESHOLDS), len(ds)), bool)
        ignored = np.zeros((len(IOU_THRESHOLDS), len(ds)), bool)
        for k, thr in enumerate(IOU_THRESHOLDS):
            taken = [False] * len(gs)
            for i in range(len(ds)):
                bound, m = min(float(thr), 1 - 1e-10), -1
                for j in range(len(gs)):
                    if taken[j] and not crowd[j]:
                        continue
                    if m > -1 and not crowd[m] and crowd[j]:
                        break
                    if ious[i][j] < bound:
                        continue
                    bound, m = ious[i][j], j
                if m > -1:
                    taken[m], matched[k, i], ignored[k, i] = True, True, crowd[m]
        out[c] = {"scores": [float(res_meta[d][0]) for d in ds], "matched": matched, "ignored": ignored,
                  "n_gt": sum(1 for x in crowd if not x), "n_crowd": sum(1 for x in crowd if x)}
    return out


def _mean(values):
    return math.fsum(values) / float(len(values)) if len(values) else -1.0


def summarize(videos, counts=None):
    """{video: what ``match_video`` returns} -> the figures, ``per_category`` and ``counts``."""
    categories = sorted(set(c for rec in videos.values() for c in rec))
    n_thr, n_rec = len(IOU_THRESHOLDS), len(RECALL_THRESHOLDS)
    precision, recall = {}, {}                                   # (category, maxDet) -> [thresholds][recall points] / [thresholds]
    for c in categories:
        recs = [rec[c] for rec in videos.values() if c in rec]
        n_gt = sum(r["n_gt"] for r in recs)
        if n_gt == 0:
            continue
        for max_det in MAX_DETS:
            scores = np.asarray([s for r in recs for s in r["scores"][:max_det]], dtype=np.float64)
            order = np.argsort(-scores, kind="mergesort")
            matched = np.concatenate([r["matched"][:, :max_det] for r in recs], axis=1)[:, order]
            ignored = np.concatenate([r["ignored"][:, :max_det] for r in recs], axis=1)[:, order]
            tps = np.cumsum(matched & ~ignored, axis=1, dtype=np.float64)
            fps = np.cumsum(~matched & ~ignored, axis=1, dtype=np.float64)
            prec, rec_last = [], []
            for k in range(n_thr):
                tp, fp = tps[k], fps[k]
                rc = tp / float(n_gt)
                pr = (tp / (fp + tp + np.spacing(1))).tolist()
                rec_last.append(float(rc[-1]) if len(tp) else 0.0)
                for i in range(len(pr) - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                at = np.searchsorted(rc, RECALL_THRESHOLDS, side="left")
                prec.append([pr[i] if i < len(pr) else 0.0 for i in at])
            precision[(c, max_det)], recall[(c, max_det)] = prec, rec_last
    counted = [c for c in categories if (c, MAX_DETS[-1]) in precision]
    top = MAX_DETS[-1]
    k50, k75 = 0, 5
    assert abs(IOU_THRESHOLDS[k75] - 0.75) < 1e-12 and n_rec == 101
    out = OrderedDict()
    out["AP"] = _mean([v for c in counted for row in precision[(c, top)] for v in row])
    out["AP50"] = _mean([v for c in counted for v in precision[(c, top)][k50]])
    out["AP75"] = _mean([v for c in counted for v in precision[(c, top)][k75]])
    out["AR1"] = _mean([v for c in counted for v in recall[(c, 1)]])
    out["AR10"] = _mean([v for c in counted for v in recall[(c, 10)]])
    out["per_category"] = OrderedDict((c, _mean([v for row in precision[(c, top)] for v in row])) for c in counted)
    out["counts"] = OrderedDict(counts if counts is not None else (("videos", len(videos)),))
    return out


# ------------------------------------------------------------------------------------------------ the evaluator
def _counts_of(seg):
    """One entry of ``segmentations`` -> (string or None, size or None)."""
    if seg is None:
        return None, None
    if isinstance(seg, dict):
        size = seg.get("size")
        return seg["counts"], (None if size is None else (int(size[0]), int(size[1])))
    return seg, None


class YtvisEvaluator(object):
    """Collects videos and reports the YouTube-VIS figures.  ``add_video`` packs the strings of both sides frame by frame, lists per frame
    every (result, ground truth) pair of one category in which both have a mask, makes ONE ``hip.rle_pair_inter`` call and ONE read-back
    of the buffer that holds ``area``, ``inter`` and ``status``, and matches on the host (``match_video``)."""

    def __init__(self, device=None):
        self.device = device
        self.videos = OrderedDict()
        self.n_results = self.n_gt = 0

    def add_video(self, video_id, results, gt_tracks, size):
        """results / gt_tracks: the tracks of ONE video (see the module's head); size: (height, width) of the video.  -> the video's
        matching records.  ValueError, naming the video and the frame, for a refused string and for a record of another size."""
        results, gt_tracks = list(results), list(gt_tracks)
        H, W = int(size[0]), int(size[1])
        lengths = set(len(tr["segmentations"]) for tr in results + gt_tracks)
        if len(lengths) > 1:
            raise ValueError("video %r: tracks of %s frames; every track of a video must have one entry per frame" % (video_id, sorted(lengths)))
        T = lengths.pop() if lengths else 0
        strings, where = [], []                                  # where[m] = (side, track, frame)
        index = [np.full((len(side), T), -1, np.int64) for side in (results, gt_tracks)]
        for t in range(T):
            for k, (what, side) in enumerate((("result", results), ("ground-truth", gt_tracks))):
                for n, tr in enumerate(side):
                    s, sz = _counts_of(tr["segmentations"][t])
                    if s is None:
                        continue
                    if sz is not None and sz != (H, W):
                        raise ValueError("video %r, frame %d: the %s mask of track %d is %d x %d, the video %d x %d"
                                         % ((video_id, t, what, n) + sz + (H, W)))
                    index[k][n, t] = len(strings)
                    strings.append(s)
                    where.append((what, n, t))
        res_meta = [(float(tr["score"]), int(tr["category_id"])) for tr in results]
        gt_meta = [(int(tr["category_id"]), int(tr.get("iscrowd", 0) or 0)) for tr in gt_tracks]
        pairs, cell = [], []
        for t in range(T):
            for d, (_, cd) in enumerate(res_meta):
                if index[0][d, t] < 0:
                    continue
                for g, (cg, _) in enumerate(gt_meta):
                    if cg == cd and index[1][g, t] >= 0:
                        pairs.append((index[0][d, t], index[1][g, t]))
                        cell.append((d, g, t))
        M, K = len(strings), len(pairs)
        area_d, area_g = np.zeros((len(results), T), np.int64), np.zeros((len(gt_tracks), T), np.int64)
        inter = np.zeros((len(results), len(gt_tracks), T), np.int64)
        if M:
            dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
            out = torch.empty(4 * (M + K) + M, dtype=torch.uint8, device=dev)                      # area | inter | status bytes
            hip.rle_pair_inter(strings, pairs, H, W, device=dev, area=out[:4 * M].view(torch.int32),
                               inter=out[4 * M:4 * (M + K)].view(torch.int32), status=out[4 * (M + K):])
            host = out.cpu().numpy()                                                               # (the one read-back)
            status = host[4 * (M + K):]
            bad = np.flatnonzero(status)
            if len(bad):
                what, n, t = where[int(bad[0])]
                st = int(status[int(bad[0])])
                raise ValueError("video %r, frame %d: the %s mask of track %d is refused: %s"
                                 % (video_id, t, what, n, hip.RLE_STATUS_NAMES.get(st, "status %d" % st)))
            area = host[:4 * M].view(np.int32)
            for m, (what, n, t) in enumerate(where):
                (area_d if what == "result" else area_g)[n, t] = area[m]
            for v, (d, g, t) in zip(host[4 * M:4 * (M + K)].view(np.int32).tolist(), cell):
                inter[d, g, t] = v
        record = match_video(res_meta, gt_meta, area_d, area_g, inter)
        self.videos[video_id] = record
        self.n_results += len(results)
        self.n_gt += len(gt_tracks)
        return record

    def summary(self):
        """-> OrderedDict: AP, AP50, AP75, AR1, AR10, "per_category" (AP per category id that counts) and "counts" (videos, result
        tracks, ground-truth tracks)."""
        return summarize(self.videos, (("videos", len(self.videos)), ("result_tracks", self.n_results), ("gt_tracks", self.n_gt)))


# ------------------------------------------------------------------------------------------------ files
def ground_truth_from_json(path, base_dir=""):
    """A video-dataset json WITH segmentations (the format of ``parse_generic_video_dataset``) -> {str(sequence id): {"size": (h, w),
    "length": T, "tracks": [ground-truth track]}}: one track per instance, instance ids ascending, its category from ``categories``,
    iscrowd 0, a frame without the instance None.  Sequences without segmentations are left out."""
    from ..data.generic_video_dataset_parser import parse_generic_video_dataset
    out = OrderedDict()
    for seq in parse_generic_video_dataset(base_dir, path)[0]:
        if seq.segmentations is None:
            continue
        h, w = (int(v) for v in seq.image_dims)
        tracks = [{"instance_id": iid, "category_id": int(seq.instance_categories[iid]), "iscrowd": 0,
                   "segmentations": [({"size": [h, w], "counts": seg_t[iid]} if iid in seg_t else None) for seg_t in seq.segmentations]}
                  for iid in sorted(seq.instance_categories)]
        out[str(seq.id)] = {"size": (h, w), "length": len(seq.segmentations), "tracks": tracks}
    return out


def evaluate_results(results, gt, device=None, videos=None):
    """results: the path of a ``results.json`` or its list of result tracks; gt: what ``ground_truth_from_json`` returns.  videos: the
    ids to evaluate (None: all of ``gt``); one without a result track has no result.  A result of a video without ground truth is an
    error.  -> the evaluator."""
    if isinstance(results, (str, bytes, os.PathLike)):
        with open(results) as fh:
            results = json.load(fh)
    wanted = list(gt) if videos is None else [str(v) for v in videos]
    per_video = OrderedDict()
    for tr in results:
        per_video.setdefault(str(tr["video_id"]), []).append(tr)
    for vid in [v for v in per_video if v not in gt] + [v for v in wanted if v not in gt]:
        raise KeyError("no video %r in the ground truth" % (vid,))
    evaluator = YtvisEvaluator(device)
    for vid in wanted:
        tracks = per_video.get(vid, [])
        for tr in tracks:
            if len(tr["segmentations"]) != gt[vid]["length"]:
                raise ValueError("video %r: a result track of %d frames, the ground truth has %d" % (vid, len(tr["segmentations"]), gt[vid]["length"]))
        evaluator.add_video(vid, tracks, gt[vid]["tracks"], gt[vid]["size"])
    return evaluator


def make_validator(json_path, base_dir, seqs=None, max_tracks=10, seediness_thresh=0.25, frame_overlap=-1, resize_scale=1.0,
                   clustering_device=None, preload_images=True):
    """-> ``validate_fn(trainer)`` for ``training.main.Trainer(validate_fn=...)``: the YouTube-VIS figures of the trainer's CURRENT
    weights on the annotated sequences of ``json_path`` (a video-dataset json with segmentations; image paths relative to ``base_dir``;
    ``seqs``: the ids to keep).  As ``evaluation.mots.make_validator``: each call copies ``trainer.model.state_dict()`` in place into one
    ``InferenceModel`` kept between calls, and a parameter whose version counter did not move is an error, not a stale figure.  The
    sequences go through the driver's per-sequence path with a ``YoutubeVISOutputGenerator`` into a temporary directory, ``save()``
    writes ``results.json``, that file is evaluated against the json and the directory is removed.  A sequence in which nothing is
    detected has no result.  -> {"AP", "AP50", "AP75", "AR1", "AR10"}."""
    from ..data.generic_video_dataset_parser import parse_generic_video_dataset
    chosen = None if seqs is None else set(str(s) for s in seqs)
    parsed, meta = parse_generic_video_dataset(base_dir, json_path)
    sequences = [s for s in parsed if s.segmentations is not None and (chosen is None or str(s.id) in chosen)]
    if not sequences:
        raise ValueError("make_validator: no sequence of %s is selected" % json_path)
    gt = ground_truth_from_json(json_path, base_dir)
    state = {}

    def validate(trainer):
        from ..inference import main as driver
        from ..inference.online_chainer import OnlineChainer
        from ..inference.output_utils import YoutubeVISOutputGenerator
        from ..modeling.inference_model import InferenceModel
        device = trainer.local_device
        with torch.cuda.device(device):
            model = state.get("model")
            if model is None:
                model = state["model"] = InferenceModel(None, semseg_output_type="logits", preload_images=preload_images,
                                                        resize_scale=resize_scale).to(device)
            params = dict(model._model.named_parameters())
            before = {k: p._version for k, p in params.items()}
            model.load_checkpoint_state(trainer.model.state_dict())
            stale = [k for k, p in params.items() if p._version <= before[k]]
            if stale:
                raise RuntimeError("make_validator: %d parameters kept their version after the copy (e.g. %s): the packed-weight caches "
                                   "would serve the weights of an earlier call" % (len(stale), stale[:3]))
            with tempfile.TemporaryDirectory(prefix="ytvis_validation_") as tmp:
                writer = YoutubeVISOutputGenerator(tmp, OnlineChainer.OUTLIER_LABEL, False, None, meta.get("category_labels"),
                                                   upscaled_inputs=float(resize_scale) != 1.0)
                tracks = driver.TrackGenerator(model, "ytvis", resize_scale=resize_scale, seediness_thresh=seediness_thresh,
                                               frame_overlap=frame_overlap, clustering_device=clustering_device or str(device))
                for sequence in sequences:
                    driver.run_sequence(tracks, sequence, writer, max_tracks)
                writer.save()
                summary = evaluate_results(os.path.join(tmp, "results.json"), gt, videos=[s.id for s in sequences], device=device).summary()
            return OrderedDict((k, summary[k]) for k in FIGURES)
    return validate
