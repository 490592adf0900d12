"""KITTI-MOTS measures sMOTSA, MOTSA and MOTSP of a result, counted on the device (``hip.rle_decode_labels`` and
``hip.label_pair_counts``: csrc/data_loader.hip, csrc/mots_eval.hip) and finished on the host with integer bookkeeping and a handful of
fp64 divisions.

The measure is DEFINED in include/stemseg_hip.h and here, after Voigtlaender et al., "MOTS: Multi-Object Tracking and Segmentation",
CVPR 2019; the official ``mots_tools`` are not available to this project, so agreement with their numbers is UNVERIFIED.
tests/mots_eval_oracle.py restates it on dense numpy masks.

    classes 1 (car) and 2 (pedestrian), each evaluated separately, totals over all added sequences.
    per frame t: H_t the result masks of the class with non-zero area, G_t the ground-truth masks of the class with non-zero area, I_t the
      union of the ground-truth masks of the ignore class (10 in MOTS txt files; category 3 of a video-dataset json becomes 10 here).
      The masks of one side of one frame, ignore included, must be pairwise disjoint.  Result records of other classes are left out.
    h and g match iff 3 * inter > area_h + area_g (IoU > 0.5 strictly, in integers); disjoint masks match at most once each.
    TP = matched pairs; FN = |G_t| - TP_t; an unmatched h is ignored iff 2 * |h n I_t| > area_h, otherwise an FP;
    IDS = matched g whose ground-truth track was last matched in an earlier frame, however long ago, to a different result track id;
    M = sum_t |G_t|; TPs = math.fsum of the matched pairs' inter / (area_h + area_g - inter) in fp64.
    sMOTSA = (TPs - FP - IDS) / M, MOTSA = (TP - FP - IDS) / M, MOTSP = TPs / TP; a zero denominator gives 0.0.
    sMOTSA-mean = the plain mean of the classes' sMOTSA over the classes with M > 0.
"""
import math
import os
import tempfile
from collections import OrderedDict
from glob import glob

import numpy as np
import torch

from .. import hip

CHUNK_FRAMES = 128                                   # frames per device round of ``add_sequence``: memory does not grow with the sequence
CLASSES = OrderedDict(((1, "car"), (2, "ped")))
IGNORE_CLASS = 10                                    # MOTS txt: class 10, id 10000
JSON_IGNORE_CATEGORY = 3                             # the video-dataset json's category of the same regions
COUNT_KEYS = ("TP", "FP", "FN", "IDS", "M", "ignored")
FIGURES = ("sMOTSA", "MOTSA", "MOTSP")


# ------------------------------------------------------------------------------------------------ records
def parse_mots_txt(path):
    """A MOTS txt file (``frame id class h w rle`` per line) -> [(frame, track_id, class_id, h, w, rle_string)]."""
    records = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            f = line.strip().split(" ")
            if f == [""]:
                continue
            if len(f) != 6:
                raise ValueError("%s, line %d: %d fields, not the 6 of 'frame id class h w rle'" % (path, n, len(f)))
            records.append(tuple(int(v) for v in f[:5]) + (f[5],))
    return records


def records_from_json(seq_record):
    """The same records from one sequence of a video-dataset json (the dict, or a parsed ``GenericVideoSequence``): the track id is the
    instance id, the class its category, category 3 (ignore) becoming class 10."""
    from ..data.generic_video_dataset_parser import GenericVideoSequence
    seq = seq_record if isinstance(seq_record, GenericVideoSequence) else GenericVideoSequence(seq_record, "")
    if seq.segmentations is None:
        raise ValueError("sequence %r has no 'segmentations': nothing to evaluate against" % (seq.id,))
    H, W = seq.image_dims
    cls = {iid: (IGNORE_CLASS if int(c) == JSON_IGNORE_CATEGORY else int(c)) for iid, c in seq.instance_categories.items()}
    return [(t, iid, cls[iid], H, W, s) for t, seg_t in enumerate(seq.segmentations) for iid, s in sorted(seg_t.items())]


# ------------------------------------------------------------------------------------------------ the host half
def new_counts():
    return OrderedDict((name, dict([(k, 0) for k in COUNT_KEYS] + [("ious", [])])) for name in CLASSES.values())


def accumulate_frame(counts, last_match, table, res_meta, gt_meta):
    """One frame's pair table into the counts.  table: integers [>= len(res_meta) + 1, >= len(gt_meta) + 1], cell (i, j) = the pixels
    with result label i and ground-truth label j (row / column 0: background); res_meta[i - 1] / gt_meta[j - 1] = (track id, class) of
    label i / j.  last_match: {(class, ground-truth track): result track id}, carried from frame to frame of ONE sequence."""
    table = np.asarray(table, dtype=np.int64)
    area_h, area_g = table.sum(axis=1), table.sum(axis=0)
    ignore_cols = [j for j, (_, c) in enumerate(gt_meta, 1) if c == IGNORE_CLASS]
    for c, name in CLASSES.items():
        acc = counts[name]
        hs = [i for i, (_, ci) in enumerate(res_meta, 1) if ci == c and area_h[i] > 0]
        gs = [j for j, (_, cj) in enumerate(gt_meta, 1) if cj == c and area_g[j] > 0]
        matched = set()
        for j in gs:
            for i in hs:
                inter, both = int(table[i, j]), int(area_h[i]) + int(area_g[j])
                if 3 * inter > both:
                    matched.add(i)
                    acc["TP"] += 1
                    acc["ious"].append(float(inter) / float(both - inter))
                    key, track = (c, gt_meta[j - 1][0]), res_meta[i - 1][0]
                    if key in last_match and last_match[key] != track:
                        acc["IDS"] += 1
                    last_match[key] = track
        acc["M"] += len(gs)
        acc["FN"] += len(gs) - len(matched)
        for i in hs:
            if i not in matched:
                ignored = sum(int(table[i, j]) for j in ignore_cols)
                if 2 * ignored > int(area_h[i]):
                    acc["ignored"] += 1
                else:
                    acc["FP"] += 1


def figures(TP, FP, IDS, M, ious):
    """-> (sMOTSA, MOTSA, MOTSP, TPs), fp64; a zero denominator gives 0.0."""
    soft = math.fsum(ious)
    return ((soft - FP - IDS) / float(M) if M else 0.0, float(TP - FP - IDS) / float(M) if M else 0.0, soft / float(TP) if TP else 0.0, soft)


def summarize(per_sequence):
    """{name: counts of one sequence (``new_counts`` filled)} -> the figures, the totals and the per-sequence table of integers."""
    out, totals, smotsa = OrderedDict(), OrderedDict(), []
    for name in CLASSES.values():
        tot = {k: sum(s[name][k] for s in per_sequence.values()) for k in COUNT_KEYS}
        ious = [v for s in per_sequence.values() for v in s[name]["ious"]]
        fig = figures(tot["TP"], tot["FP"], tot["IDS"], tot["M"], ious)
        for key, value in zip(FIGURES, fig):
            out["%s-%s" % (key, name)] = value
        tot["TPs"] = fig[3]
        totals[name] = tot
        if tot["M"] > 0:
            smotsa.append(fig[0])
    out["sMOTSA-mean"] = sum(smotsa) / float(len(smotsa)) if smotsa else 0.0
    out["counts"] = totals
    out["sequences"] = OrderedDict((seq, OrderedDict((name, {k: s[name][k] for k in COUNT_KEYS}) for name in CLASSES.values()))
                                   for seq, s in per_sequence.items())
    return out


# ------------------------------------------------------------------------------------------------ the evaluator
def _side(name, what, records, keep, n_frames, size):
    """The records of one side -> per frame the list of (track, class, string) in ascending track order."""
    frames = [[] for _ in range(n_frames)]
    seen = set()
    for (t, track, c, h, w, s) in records:
        if not 0 <= t < n_frames:
            raise ValueError("sequence %r: a %s record names frame %d of %d" % (name, what, t, n_frames))
        if (h, w) != size:
            raise ValueError("sequence %r, frame %d: the %s record of track %d is %d x %d, the sequence %d x %d" % ((name, t, what, track, h, w) + size))
        if c not in keep:
            continue
        if (t, track) in seen:
            raise ValueError("sequence %r, frame %d: two %s records of track %d" % (name, t, what, track))
        seen.add((t, track))
        frames[t].append((track, c, s))
    for t, items in enumerate(frames):
        items.sort(key=lambda r: r[0])
        if len(items) > hip.LABEL_PAIR_MAX_LABELS:
            raise ValueError("sequence %r, frame %d: %d %s masks, the limit is %d per frame and side"
                             % (name, t, len(items), what, hip.LABEL_PAIR_MAX_LABELS))
    return frames


class MotsEvaluator(object):
    """Collects sequences and reports the KITTI-MOTS figures.  ``add_sequence`` works through the frames in chunks of ``CHUNK_FRAMES``;
    a chunk makes two ``rle_decode_labels`` calls (results; ground truth with ignore), one ``label_pair_counts`` call and ONE read-back,
    of the tables, the overlap counts and the status bytes in their one buffer.  The labels are local to a frame (1 .. the number of
    masks of the side in that frame, in ascending track order), so 63 masks per side and frame is the only limit a sequence meets."""

    def __init__(self, device=None):
        self.device = device
        self.sequences = OrderedDict()

    def add_sequence(self, name, result_records, gt_records, n_frames=None):
        """result_records, gt_records: (frame, track_id, class_id, h, w, rle_string) as ``parse_mots_txt`` / ``records_from_json`` give
        them.  n_frames: the sequence's length (None: the largest frame named + 1).  -> the sequence's counts.  ValueError, naming the
        sequence and the frame, for a refused string, overlapping masks on one side, more than 63 masks of a side in a frame, a record
        of another size than the sequence's, a frame outside the sequence."""
        result_records, gt_records = list(result_records), list(gt_records)
        everything = gt_records + result_records
        counts, last_match = new_counts(), {}
        self.sequences[name] = counts
        if not everything:
            return counts
        if n_frames is None:
            n_frames = max(r[0] for r in everything) + 1
        size = (int(everything[0][3]), int(everything[0][4]))
        sides = (("result", _side(name, "result", result_records, set(CLASSES), n_frames, size)),
                 ("ground-truth", _side(name, "ground-truth", gt_records, set(CLASSES) | {IGNORE_CLASS}, n_frames, size)))
        dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        for t0 in range(0, n_frames, CHUNK_FRAMES):
            t1 = min(n_frames, t0 + CHUNK_FRAMES)
            if not any(frames[t] for _, frames in sides for t in range(t0, t1)):
                continue
            self._chunk(name, sides, t0, t1, size, dev, counts, last_match)
        return counts

    def _chunk(self, name, sides, t0, t1, size, dev, counts, last_match):
        P, (H, W) = t1 - t0, size
        items = [[(t, n, s) for t in range(t0, t1) for n, (_, _, s) in enumerate(frames[t], 1)] for _, frames in sides]
        K = [max([1] + [len(frames[t]) for t in range(t0, t1)]) for _, frames in sides]
        n_counts = P * (K[0] + 1) * (K[1] + 1)
        o_overlap, o_status = 4 * n_counts, 4 * (n_counts + 2 * P)
        m_pad = [max(len(it), 1) for it in items]
        out = torch.empty(o_status + m_pad[0] + m_pad[1], dtype=torch.uint8, device=dev)          # tables | overlaps | status bytes
        maps = []
        for k in (0, 1):
            overlap = out[o_overlap + 4 * P * k:o_overlap + 4 * P * (k + 1)].view(torch.int32)
            status = out[o_status + m_pad[0] * k:o_status + m_pad[0] * k + m_pad[k]]
            maps.append(hip.rle_decode_labels([s for _, _, s in items[k]], [t - t0 for t, _, _ in items[k]], [n for _, n, _ in items[k]], P, H, W,
                                              device=dev, overlap=overlap, status=status)[0])
        hip.label_pair_counts(maps[0], maps[1], K[0], K[1], counts=out[:o_overlap].view(torch.int32))
        host = out.cpu().numpy()                                                                  # (the one read-back)
        for k, (what, frames) in enumerate(sides):
            status = host[o_status + m_pad[0] * k:o_status + m_pad[0] * k + len(items[k])]
            bad = np.flatnonzero(status)
            if len(bad):
                t, n, _ = items[k][int(bad[0])]
                st = int(status[int(bad[0])])
                raise ValueError("sequence %r, frame %d: the %s mask of track %d is refused: %s"
                                 % (name, t, what, frames[t][n - 1][0], hip.RLE_STATUS_NAMES.get(st, "status %d" % st)))
            overlap = host[o_overlap + 4 * P * k:o_overlap + 4 * P * (k + 1)].view(np.int32)
            bad = np.flatnonzero(overlap)
            if len(bad):
                raise ValueError("sequence %r, frame %d: the %s masks overlap in %d pixels; the masks of one side of a frame must be disjoint"
                                 % (name, t0 + int(bad[0]), what, int(overlap[int(bad[0])])))
        tables = host[:o_overlap].view(np.int32).reshape(P, K[0] + 1, K[1] + 1)
        for t in range(t0, t1):
            accumulate_frame(counts, last_match, tables[t - t0], [(track, c) for track, c, _ in sides[0][1][t]],
                             [(track, c) for track, c, _ in sides[1][1][t]])

    def summary(self):
        """-> OrderedDict: sMOTSA-car, MOTSA-car, MOTSP-car, sMOTSA-ped, MOTSA-ped, MOTSP-ped, sMOTSA-mean, "counts" (per class the
        totals TP, FP, FN, IDS, M, ignored and TPs) and "sequences" (per sequence and class the integer counts)."""
        return summarize(self.sequences)


# ------------------------------------------------------------------------------------------------ files
def ground_truth(path, base_dir=""):
    """PATH of ``--eval_mots_annotations`` -> {int sequence id: (records, n_frames or None)}: a video-dataset json, or a directory of
    ``NNNN.txt`` MOTS ground-truth files."""
    if os.path.isdir(path):
        files = sorted(glob(os.path.join(path, "*.txt")))
        if not files:
            raise ValueError("%s holds no NNNN.txt ground-truth file" % path)
        return OrderedDict((int(os.path.splitext(os.path.basename(f))[0]), (parse_mots_txt(f), None)) for f in files)
    from ..data.generic_video_dataset_parser import parse_generic_video_dataset
    return OrderedDict((int(s.id), (records_from_json(s), len(s))) for s in parse_generic_video_dataset(base_dir, path)[0]
                       if s.segmentations is not None)


def evaluate_results(results_dir, gt, seqs=None, device=None):
    """Every ``NNNN.txt`` of ``results_dir`` against ``gt`` (what ``ground_truth`` returns).  seqs: the int sequence ids to evaluate
    (None: all of ``gt``); one without a result file has no result.  A result file without ground truth is an error.  -> the evaluator."""
    wanted = list(gt) if seqs is None else [int(s) for s in seqs]
    results = {int(os.path.splitext(os.path.basename(f))[0]): f for f in glob(os.path.join(results_dir, "*.txt"))}
    for sid in sorted(set(results) - set(gt)) + sorted(set(wanted) - set(gt)):
        raise KeyError("no sequence %04d in the ground truth" % sid)
    evaluator = MotsEvaluator(device)
    for sid in wanted:
        records, n_frames = gt[sid]
        evaluator.add_sequence("%04d" % sid, parse_mots_txt(results[sid]) if sid in results else [], records, n_frames)
    return evaluator


def make_validator(json_path, base_dir, seqs=None, max_tracks=1000, seediness_thresh=0.25, frame_overlap=-1, resize_scale=1.0,
                   clustering_device=None, preload_images=False):
    """-> ``validate_fn(trainer)`` for ``training.main.Trainer(validate_fn=...)``: the KITTI-MOTS figures of the trainer's CURRENT weights
    on the annotated sequences of ``json_path`` (a video-dataset json with segmentations; image paths relative to ``base_dir``; ``seqs``:
    the ids to keep).  As ``evaluation.davis.make_validator``: each call copies ``trainer.model.state_dict()`` in place into one
    ``InferenceModel`` kept between calls, and a parameter whose version counter did not move is an error, not a stale figure.  The
    sequences go through the driver's per-sequence path with ``KittiMOTSOutputGenerator`` into a temporary directory, ``save()`` applies
    the track filters, the filtered files are evaluated against the json and the directory is removed.  A sequence in which nothing is
    detected has no result.  -> {"sMOTSA-car", "MOTSA-car", "MOTSP-car", "sMOTSA-ped", "MOTSA-ped", "MOTSP-ped", "sMOTSA-mean"}."""
    from ..data.generic_video_dataset_parser import parse_generic_video_dataset
    chosen = None if seqs is None else set(str(s) for s in seqs)
    sequences = [s for s in parse_generic_video_dataset(base_dir, json_path)[0] if chosen is None or str(s.id) in chosen]
    if not sequences:
        raise ValueError("make_validator: no sequence of %s is selected" % json_path)
    gt = OrderedDict((int(s.id), (records_from_json(s), len(s))) for s in sequences)
    state = {}

    def validate(trainer):
        from ..inference import main as driver
        from ..inference.online_chainer import OnlineChainer
        from ..inference.output_utils import KittiMOTSOutputGenerator
        from ..modeling.inference_model import InferenceModel
        device = trainer.local_device
        with torch.cuda.device(device):
            model = state.get("model")
            if model is None:
                model = state["model"] = InferenceModel(None, semseg_output_type="argmax", preload_images=preload_images,
                                                        resize_scale=resize_scale).to(device)
            params = dict(model._model.named_parameters())
            before = {k: p._version for k, p in params.items()}
            model.load_checkpoint_state(trainer.model.state_dict())
            stale = [k for k, p in params.items() if p._version <= before[k]]
            if stale:
                raise RuntimeError("make_validator: %d parameters kept their version after the copy (e.g. %s): the packed-weight caches "
                                   "would serve the weights of an earlier call" % (len(stale), stale[:3]))
            with tempfile.TemporaryDirectory(prefix="mots_validation_") as tmp:
                writer = KittiMOTSOutputGenerator(tmp, OnlineChainer.OUTLIER_LABEL, False, upscaled_inputs=float(resize_scale) != 1.0, keep_masks=False)
                tracks = driver.TrackGenerator(model, "kittimots", resize_scale=resize_scale, seediness_thresh=seediness_thresh,
                                               frame_overlap=frame_overlap, clustering_device=clustering_device or str(device))
                os.makedirs(writer.results_output_dir, exist_ok=True)
                for sequence in sequences:
                    try:
                        driver.run_sequence(tracks, sequence, writer, max_tracks)
                    except ValueError as e:                      # (the writer's word for a sequence without a single instance)
                        if "Zero instances detected" not in str(e):
                            raise
                writer.save()
                summary = evaluate_results(writer.results_output_dir + "_nms", gt, device=device).summary()
            return OrderedDict((k, v) for k, v in summary.items() if k not in ("counts", "sequences"))
    return validate
