"""DAVIS region (J) and boundary (F) measures of a result, counted on the device (``hip.davis_eval_counts``, csrc/davis_eval.hip) and
divided on the host in fp64.

The measure is DEFINED in include/stemseg_hip.h and here, after the published DAVIS 2017 "unsupervised" protocol; the DAVIS toolkit is
not available to this project, so agreement with the official toolkit's numbers is UNVERIFIED.  tests/davis_eval_oracle.py restates it
in numpy.

    per frame and (proposal p, object g):   J = inter / (area_p + area_g - inter), 1 on an empty union
                                            P, R = m_p / n_p, m_g / n_g when both boundaries have pixels;
                                                   (1, 0) when only p's is empty, (0, 1) when only g's is, (1, 1) when both are
                                            F = 2 P R / (P + R), 0 when P + R = 0
    per sequence: frames 1 .. T - 2 count; the score of a pair is the mean over them of (J + F) / 2; the zero-padded square score
    matrix goes through the exact Hungarian solver the chainer uses (scipy's ``linear_sum_assignment``), maximising; an object that
    gets no proposal scores 0 on every frame.  Per object and measure: Mean, Recall (the share of frames above 0.5) and Decay (the mean
    of the first of four frame bins minus the mean of the last, bins at round(linspace(1, n, 5) + 1e-10) - 1, both ends inclusive).
    Dataset figures are means over all objects of all sequences; J&F-Mean = (J-Mean + F-Mean) / 2.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from .. import hip

STATS = ("J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay")


def radius(H, W):
    """The dilation radius of an H x W frame: ceil(0.008 x the diagonal), in fp64 (8 at 480 x 854)."""
    return int(math.ceil(0.008 * math.sqrt(float(H) * float(H) + float(W) * float(W))))


def counted_frames(T):
    if T < 3:
        raise ValueError("a sequence of %d frames: the first and the last frame are left out, so at least 3 are needed" % T)
    return slice(1, T - 1)


def measures_from_counts(tab):
    """tab: the seven integer tables (numpy, name -> array) -> (J, F), fp64 [T, Kp, Kg]."""
    inter, m_p, m_g = (np.asarray(tab[k], dtype=np.int64) for k in ("inter", "m_p", "m_g"))
    area_p, n_p = (np.asarray(tab[k], dtype=np.int64)[:, :, None] for k in ("area_p", "n_p"))
    area_g, n_g = (np.asarray(tab[k], dtype=np.int64)[:, None, :] for k in ("area_g", "n_g"))
    union = area_p + area_g - inter
    J = np.where(union == 0, 1.0, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64))
    both = (n_p > 0) & (n_g > 0)
    P = np.where(both, m_p.astype(np.float64) / np.maximum(n_p, 1).astype(np.float64), np.where(n_p == 0, 1.0, 0.0))
    R = np.where(both, m_g.astype(np.float64) / np.maximum(n_g, 1).astype(np.float64), np.where(n_g == 0, 1.0, 0.0))
    s = P + R
    F = np.where(s == 0, 0.0, 2.0 * P * R / np.where(s == 0, 1.0, s))
    return J, F


def _mean(v):
    return float(np.mean(np.ascontiguousarray(v, dtype=np.float64)))          # (one contiguous vector: numpy's pairwise sum, whatever the view was)


def decay_bins(n):
    ids = [int(v) for v in np.round(np.linspace(1, n, 5) + 1e-10) - 1]
    return [(ids[i], ids[i + 1]) for i in range(4)]


def frame_stats(values):
    """(mean, recall, decay) of one object's per-frame values over the counted frames."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    bins = decay_bins(len(v))
    return _mean(v), _mean((v > 0.5).astype(np.float64)), _mean(v[bins[0][0]:bins[0][1] + 1]) - _mean(v[bins[3][0]:bins[3][1] + 1])


def sequence_statistics(tab, Kp, Kg):
    """The host half for one sequence.  tab: the tables over ALL T frames (Kp may be 0: ``tab`` is then not read) ->
    {"assignment": [Kg] proposal index or -1, "J" / "F": fp64 [Kg, frames], "objects": [Kg] dicts of the six statistics}."""
    from scipy.optimize import linear_sum_assignment
    T = int(np.asarray(tab["area_g"]).shape[0])
    frames = counted_frames(T)
    n_frames = T - 2
    assignment = [-1] * Kg
    if Kp > 0:
        J, F = (m[frames] for m in measures_from_counts(tab))
        pair = (J + F) / 2.0
        n = max(Kp, Kg)
        score = np.zeros((n, n), np.float64)
        for p in range(Kp):
            for g in range(Kg):
                score[p, g] = _mean(pair[:, p, g])
        rows, cols = linear_sum_assignment(score, maximize=True)
        for p, g in zip(rows, cols):
            if p < Kp and g < Kg:
                assignment[g] = int(p)
    Jg, Fg = np.zeros((Kg, n_frames), np.float64), np.zeros((Kg, n_frames), np.float64)
    for g, p in enumerate(assignment):
        if p >= 0:
            Jg[g], Fg[g] = J[:, p, g], F[:, p, g]
    objects = [dict(zip(STATS, frame_stats(Jg[g]) + frame_stats(Fg[g]))) for g in range(Kg)]
    return {"assignment": assignment, "J": Jg, "F": Fg, "objects": objects}


def summarize(per_sequence):
    """{name: sequence_statistics(...)} -> the dataset figures and the per-sequence table."""
    objs = [o for s in per_sequence.values() for o in s["objects"]]
    if not objs:
        raise ValueError("DavisEvaluator.summary: no object in any sequence")
    out = OrderedDict((k, _mean([o[k] for o in objs])) for k in STATS)
    out["J&F-Mean"] = (out["J-Mean"] + out["F-Mean"]) / 2.0
    out.move_to_end("J&F-Mean", last=False)
    table = OrderedDict()
    for name, s in per_sequence.items():
        if s["objects"]:
            j, f = _mean([o["J-Mean"] for o in s["objects"]]), _mean([o["F-Mean"] for o in s["objects"]])
            table[name] = {"J-Mean": j, "F-Mean": f, "J&F-Mean": (j + f) / 2.0, "objects": len(s["objects"]), "proposals": s.get("n_proposals"),
                           "assignment": list(s["assignment"])}
    out["sequences"] = table
    return out


class DavisEvaluator(object):
    """Collects sequences and reports the DAVIS figures.  ``add_sequence`` launches the counting kernel and makes ONE read-back, of the
    seven tables in their one buffer; everything after is host arithmetic on integers."""

    def __init__(self):
        self.sequences = OrderedDict()

    def add_sequence(self, name, pred_maps, gt_planes, n_proposals=None):
        """pred_maps: index map [T,H,W] on the device (uint8 or 16-bit; labels 1 .. n_proposals are the proposals), gt_planes: uint8
        [Kg,T,H,W] on the device.  n_proposals: the number of proposals the map was written with (a writer knows it; labels that never
        occur are proposals all the same); None: the largest label of the map, which costs one more small read-back.  -> the
        sequence's statistics.  ValueError beyond the kernel's limits (64 proposals, 32 objects, radius 32) and for T < 3."""
        if pred_maps.dim() != 3 or gt_planes.dim() != 4 or tuple(gt_planes.shape[1:]) != tuple(pred_maps.shape):
            raise ValueError("DavisEvaluator.add_sequence(%r): the index map %s [T,H,W] and the planes %s [Kg,T,H,W] do not go together"
                             % (name, tuple(pred_maps.shape), tuple(gt_planes.shape)))
        T, H, W = (int(v) for v in pred_maps.shape)
        Kg = int(gt_planes.shape[0])
        counted_frames(T)
        if n_proposals is None:
            wide = pred_maps if pred_maps.dtype == torch.uint8 else pred_maps.to(torch.int32) & 0xffff
            n_proposals = int(wide.max()) if pred_maps.numel() else 0
        Kp = int(n_proposals)
        tab = {"area_g": np.zeros((T, Kg), np.int64)}
        if Kp > 0 and Kg > 0:
            shapes = hip.davis_eval_table_shapes(T, Kp, Kg)
            counts = torch.empty(sum(int(np.prod(s)) for s in shapes), dtype=torch.int32, device=pred_maps.device)
            hip.davis_eval_counts(pred_maps.contiguous(), gt_planes.contiguous(), Kp, radius(H, W), counts=counts)
            host, at = counts.cpu().numpy(), 0          # (the one read-back)
            for key, shape in zip(hip.DAVIS_EVAL_TABLES, shapes):
                n = int(np.prod(shape))
                tab[key] = host[at:at + n].reshape(shape).astype(np.int64)
                at += n
        stats = sequence_statistics(tab, Kp if Kg > 0 else 0, Kg)
        stats["n_proposals"], stats["radius"] = Kp, radius(H, W)
        self.sequences[name] = stats
        return stats

    def summary(self):
        """-> OrderedDict: J&F-Mean, J-Mean, J-Recall, J-Decay, F-Mean, F-Recall, F-Decay, and "sequences": the per-sequence table
        (J-Mean, F-Mean, J&F-Mean over the sequence's objects, the numbers of objects and of proposals, and the proposal given to each)."""
        return summarize(self.sequences)


def gt_planes_from_json(seq_record, device=None):
    """The ground truth of one sequence record of the reference's video-dataset json (``{"id", "height", "width", "image_paths",
    "categories", "segmentations": [per frame {instance id: COCO RLE string}]}``, or the parsed
    ``data.generic_video_dataset_parser.GenericVideoSequence``) -> (planes uint8 [Kg,T,H,W] on the device, the instance ids in the
    planes' order: ascending).  An instance that is absent from a frame has a zero plane there.  A string the decoder refuses is an
    error naming the instance and the frame."""
    from ..data.generic_video_dataset_parser import GenericVideoSequence
    seq = seq_record if isinstance(seq_record, GenericVideoSequence) else GenericVideoSequence(seq_record, "")
    if seq.segmentations is None:
        raise ValueError("sequence %r has no 'segmentations': nothing to evaluate against" % (seq.id,))
    ids = sorted(set(iid for seg_t in seq.segmentations for iid in seg_t))
    plane = {iid: k for k, iid in enumerate(ids)}
    T, (H, W) = len(seq), seq.image_dims
    items = [(plane[iid], t, s) for t, seg_t in enumerate(seq.segmentations) for iid, s in sorted(seg_t.items())]
    if not ids:
        return torch.zeros((0, T, H, W), dtype=torch.uint8, device=device if device is not None else "cuda"), ids
    planes, status = hip.rle_decode([s for _, _, s in items], [k * T + t for k, t, _ in items], len(ids) * T, H, W, device)
    bad = np.flatnonzero(status.cpu().numpy()) if items else []
    if len(bad):
        k, t, _ = items[int(bad[0])]
        raise ValueError("sequence %r: the mask of instance %d in frame %d is refused: %s"
                         % (seq.id, ids[k], t, hip.RLE_STATUS_NAMES.get(int(status[int(bad[0])]), "status %d" % int(status[int(bad[0])]))))
    return planes.view(len(ids), T, H, W), ids


def make_validator(json_path, base_dir, seqs=None, max_tracks=20, seediness_thresh=0.25, frame_overlap=-1, resize_scale=1.0,
                   clustering_device=None):
    """-> ``validate_fn(trainer)`` for ``training.main.Trainer(validate_fn=...)``: the DAVIS figures of the trainer's CURRENT weights on
    the annotated sequences of ``json_path`` (a video-dataset json with segmentations; image paths relative to ``base_dir``; ``seqs``: the
    ids to keep).  Each call copies ``trainer.model.state_dict()`` into one ``InferenceModel`` kept between calls -- built on the first
    call under the global cfg, i.e. the trainer's preset -- and runs the driver's per-sequence path (``inference.main.run_sequence``)
    with a writer that materialises the index maps, hands them to the evaluator and writes no file.  The copy is in place, so every
    parameter's version counter moves and the packed-weight caches of the backbone and the decoders, which are keyed on it, repack;
    a parameter whose counter did not move is an error, not a stale figure.  -> {"J&F-Mean", "J-Mean", "J-Recall", "J-Decay", "F-Mean",
    "F-Recall", "F-Decay"}."""
    from ..data.generic_video_dataset_parser import parse_generic_video_dataset
    from ..inference.output_utils.generators import _OutputGeneratorBase
    sequences = [s for s in parse_generic_video_dataset(base_dir, json_path)[0] if seqs is None or s.id in set(seqs)]
    if not sequences:
        raise ValueError("make_validator: no sequence of %s is selected" % json_path)
    annotations = {s.id: s for s in sequences}
    state = {}

    class IndexMapsOnly(_OutputGeneratorBase):
        index_map_hook = None

        def process_sequence(self, sequence, track_mask_idxes, track_mask_labels, instance_pt_counts, instance_lifetimes, category_masks,
                             mask_dims, mask_scale, max_tracks, device="cpu"):
            keep, masks = self._materialize(sequence, track_mask_idxes, track_mask_labels, instance_lifetimes, mask_dims, mask_scale,
                                            max_tracks, device)
            self.index_map_hook(sequence, keep, masks)
            return keep, dict()

    def validate(trainer):
        from ..inference import main as driver
        from ..inference.online_chainer import OnlineChainer
        from ..modeling.inference_model import InferenceModel
        device = trainer.local_device
        with torch.cuda.device(device):
            model = state.get("model")
            if model is None:
                model = state["model"] = InferenceModel(None, semseg_output_type=None, preload_images=True, resize_scale=resize_scale).to(device)
            params = dict(model._model.named_parameters())
            before = {k: p._version for k, p in params.items()}
            model.load_checkpoint_state(trainer.model.state_dict())
            stale = [k for k, p in params.items() if p._version <= before[k]]
            if stale:
                raise RuntimeError("make_validator: %d parameters kept their version after the copy (e.g. %s): the packed-weight caches "
                                   "would serve the weights of an earlier call" % (len(stale), stale[:3]))
            writer = IndexMapsOnly("", OnlineChainer.OUTLIER_LABEL, False, upscaled_inputs=float(resize_scale) != 1.0)
            evaluator = driver.attach_evaluator(writer, annotations)
            tracks = driver.TrackGenerator(model, "davis", resize_scale=resize_scale, seediness_thresh=seediness_thresh, frame_overlap=frame_overlap,
                                           clustering_device=clustering_device or str(device))
            for sequence in sequences:
                driver.run_sequence(tracks, sequence, writer, max_tracks)
            return {k: v for k, v in evaluator.summary().items() if k != "sequences"}
    return validate
