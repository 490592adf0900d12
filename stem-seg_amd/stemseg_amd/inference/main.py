"""Clip windowing, fg mask from seediness, and the per-sequence driver.

Counterpart of ``stemseg/inference/main.py``: get_subsequence_frames :23-49, TrackGenerator :52-170
(create_clusterer :84-91, get_fg_masks_from_seediness :93-103, do_inference :132-149, do_clustering :151-170).
The reference's own driver runs unchanged on this hot path through ``stemseg_amd.overlay``.  The small driver at the end of this module
(``run_sequence`` / ``run_sequences`` / ``main``, ``python -m stemseg_amd.inference.main``) is this library's: the reference's flags for
the three datasets over the native parser and writers, plus one opt-in, ``--eval_annotations <video-dataset json>`` for ``--dataset
davis``: every sequence's index maps go to ``evaluation.davis.DavisEvaluator`` before they are freed, the summary is logged and written
as ``davis_eval.json`` beside the results.  ``--dataset kittimots`` has an opt-in of its own, ``--eval_mots_annotations <video-dataset
json | directory of NNNN.txt>``: after the writer's ``save()`` the filtered ``results_nms/*.txt`` are evaluated by
``evaluation.mots.MotsEvaluator`` (sMOTSA, MOTSA, MOTSP), the summary is logged and written as ``mots_eval.json``.  ``--dataset ytvis``
has ``--eval_ytvis_annotations <video-dataset json>``: after ``save()`` the instances that were written are evaluated by
``evaluation.ytvis.YtvisEvaluator`` (AP, AP50, AP75, AR1, AR10), the summary is logged and written as ``ytvis_eval.json``.  Without the
flags nothing else happens than before.
"""
import argparse
import json
import os

import torch

from .. import hip
from ..config import cfg
from ..modeling.embedding_utils import get_nb_free_dims
from .clusterers import SequentialClustering
from .online_chainer import OnlineChainer

_OVERLAP_KEY = {"davis": "DAVIS", "ytvis": "YOUTUBE_VIS", "kittimots": "KITTI_MOTS"}


def get_subsequence_frames(seq_len, subseq_len, dataset_name, frame_overlap=-1):
    """-> (list of frame-index lists, padded-flags or None).  Stride subseq_len - overlap, plus one tail clip that
    ends on the last frame; videos shorter than a clip repeat frame 0 on the left."""
    if dataset_name not in _OVERLAP_KEY:
        raise NotImplementedError()
    if frame_overlap <= 0:                     # 0 and negatives mean "dataset default" (main.py:27-31)
        frame_overlap = getattr(cfg.DATA, _OVERLAP_KEY[dataset_name]).INFERENCE_FRAME_OVERLAP
    assert frame_overlap < subseq_len
    if seq_len < subseq_len:
        n_pad = subseq_len - seq_len
        return [[0] * n_pad + list(range(seq_len))], [True] * n_pad + [False] * seq_len
    starts = list(range(0, seq_len - subseq_len + 1, subseq_len - frame_overlap))
    clips = [list(range(t, t + subseq_len)) for t in starts]
    if not clips or clips[-1][-1] != seq_len - 1:
        clips.append(list(range(seq_len - subseq_len, seq_len)))
    return clips, None


@torch.no_grad()
def fg_masks_from_seediness(embedding_maps, threshold, device=None):
    """Mean seediness over the clips containing each frame, > threshold -> uint8 [n_frames, h, w] on the device
    (inference/main.py:93-103).  One accumulate launch per clip (its T planes go to their frames' sums; clip order = the
    reference's ``+=`` order) and ONE mask launch for the whole sequence."""
    hip.require_gpu()
    frames_all = sorted({t for entry in embedding_maps for t in entry[0]})
    index = {t: i for i, t in enumerate(frames_all)}
    acc, counts = None, [0.0] * len(frames_all)
    for entry in embedding_maps:
        frames, seed = list(entry[0]), entry[3]
        seed = (seed if seed.is_cuda else seed.to(device if device is not None else "cuda")).contiguous().float()
        if acc is None:
            acc = torch.zeros((len(frames_all), 1) + tuple(seed.shape[-2:]), dtype=torch.float32, device=seed.device)
        assert len(set(frames)) == len(frames) and seed.shape[1] == len(frames)
        hip.semseg_accumulate(acc, seed, [index[t] for t in frames])
        for t in frames:
            counts[index[t]] += 1.0
    if acc is None:
        return torch.zeros(0, dtype=torch.uint8)
    return hip.fg_mask_frames(acc[:, 0], torch.tensor(counts, dtype=torch.float32).to(acc.device), threshold)


class TrackGenerator(object):
    """Sequence -> clips -> head outputs -> fg mask -> clustering + stitching (no dataset / writer plumbing)."""

    def __init__(self, model, dataset_name, resize_scale=1.0, **kwargs):
        self.model = model
        self.dataset_name = dataset_name
        self.resize_scale = resize_scale
        self.seediness_fg_threshold = kwargs.get("seediness_thresh", 0.25)
        self.frame_overlap = kwargs.get("frame_overlap", -1)
        self.clustering_device = kwargs.get("clustering_device", "cuda:0")
        ops = kwargs.get("ops")
        if ops is None:
            from .online_chainer import HipChainerOps
            ops = HipChainerOps(self.clustering_device)
        self.chainer = OnlineChainer(self.create_clusterer(), embedding_resize_factor=resize_scale, ops=ops)

    def create_clusterer(self):
        c = cfg.CLUSTERING
        return SequentialClustering(primary_prob_thresh=c.PRIMARY_PROB_THRESHOLD, secondary_prob_thresh=c.SECONDARY_PROB_THRESHOLD,
                                    min_seediness_prob=c.MIN_SEEDINESS_PROB, n_free_dims=get_nb_free_dims(cfg.MODEL.EMBEDDING_DIM_MODE),
                                    free_dim_stds=cfg.TRAINING.LOSSES.EMBEDDING.FREE_DIM_STDS, device=self.clustering_device)

    def get_fg_masks_from_seediness(self, inference_output):
        return fg_masks_from_seediness(inference_output['embeddings'], self.seediness_fg_threshold, self.clustering_device)

    def do_inference(self, frames):
        n = len(frames)
        subseq_idxes, _ = get_subsequence_frames(n, cfg.INPUT.NUM_FRAMES, self.dataset_name, self.frame_overlap)
        out = self.model(frames, subseq_idxes)
        fg_masks = out["fg_masks"]
        if torch.is_tensor(fg_masks):            # semseg head present: its foreground probability > 0.5 (main.py:142-144)
            fg_masks = fg_masks if fg_masks.is_cuda else fg_masks.to(self.clustering_device)
            fg_masks = torch.stack([hip.fg_mask(p.contiguous(), 1.0, 0.5) for p in fg_masks], 0)
        else:                                    # otherwise the seediness map, averaged over clips, > threshold (:145-147)
            fg_masks = self.get_fg_masks_from_seediness(out)
        return out["embeddings"], fg_masks, out["multiclass_masks"]

    def do_clustering(self, all_embeddings, fg_masks):
        dicts = [{"frames": f, "embeddings": e, "bandwidths": b, "seediness": s} for (f, e, b, s) in all_embeddings]
        return self.chainer.process(fg_masks, dicts)

    def process_sequence(self, frames):
        embeddings, fg_masks, _ = self.do_inference(frames)
        return self.do_clustering(embeddings, fg_masks)


# ------------------------------------------------------------------------------------------------ the driver
# per --dataset: the preset the reference loads without a config.yaml (main.py:188-195), the semseg output its writer reads, and
# MAX_INFERENCE_TRACKS (defaults.yaml)
DATASETS = {"davis": ("davis_2", None, 20), "ytvis": ("ytvis", "logits", 10), "kittimots": ("kittimots", "argmax", 1000)}


def run_sequence(track_generator, sequence, output_generator, max_tracks):
    """One sequence from its image files to the writer (inference/main.py:105-130,151-170) -> what the writer's ``process_sequence``
    returns."""
    paths = [os.path.join(sequence.base_dir, p) for p in sequence.image_paths]
    embeddings, fg_masks, multiclass_masks = track_generator.do_inference(paths)
    (track_labels, pt_counts, lifetimes), mask_idxes = track_generator.do_clustering(embeddings, fg_masks)[:2]
    return output_generator.process_sequence(sequence, mask_idxes, track_labels, pt_counts, lifetimes, multiclass_masks,
                                             tuple(fg_masks.shape[-2:]), 4.0, max_tracks, device=track_generator.clustering_device)


def attach_evaluator(output_generator, annotations):
    """Seat a ``DavisEvaluator`` on a DAVIS writer's ``index_map_hook``.  annotations: {sequence id: sequence record or parsed sequence of
    the video-dataset json}.  A sequence without annotations is an error, not a silent gap in the mean."""
    from ..evaluation.davis import DavisEvaluator, gt_planes_from_json
    evaluator = DavisEvaluator()

    def hook(sequence, keep, masks):
        if sequence.id not in annotations:
            raise KeyError("--eval_annotations: no sequence %r in the annotations" % (sequence.id,))
        planes, _ = gt_planes_from_json(annotations[sequence.id], masks.device)
        if tuple(planes.shape[1:]) != tuple(masks.shape):
            raise ValueError("--eval_annotations: sequence %r is annotated as %s [T,H,W], the result is %s"
                             % (sequence.id, tuple(planes.shape[1:]), tuple(masks.shape)))
        evaluator.add_sequence(sequence.id, masks, planes, n_proposals=len(keep))
    output_generator.index_map_hook = hook
    return evaluator


def evaluate_mots(output_generator, sequences, mots_annotations, output_dir, print_fn=print):
    """The filtered KITTI-MOTS result files of the sequences that were run against ``mots_annotations`` (a video-dataset json or a
    directory of ``NNNN.txt``); the summary is logged and written to <output_dir>/mots_eval.json.  Reads the result files only."""
    from ..evaluation import mots
    evaluator = mots.evaluate_results(output_generator.results_output_dir + "_nms", mots.ground_truth(mots_annotations),
                                      seqs=[int(s.id) for s in sequences])
    summary = evaluator.summary()
    print_fn("KITTI-MOTS evaluation over %d sequences (this library's restatement of the measure; agreement with mots_tools is "
             "unverified): %s" % (len(summary["sequences"]),
                                  " - ".join("%s: %.4f" % (k, v) for k, v in summary.items() if k not in ("counts", "sequences"))))
    path = os.path.join(output_dir, "mots_eval.json")
    with open(path, "w") as fh:
        json.dump(summary, fh, indent=1)
    print_fn("evaluation written to %s" % path)
    return summary


def evaluate_ytvis(output_generator, sequences, ytvis_annotations, output_dir, print_fn=print):
    """The YouTube-VIS instances that the writer has just saved, of the sequences that were run, against ``ytvis_annotations`` (a
    video-dataset json with segmentations); the summary is logged and written to <output_dir>/ytvis_eval.json.  Reads the instances only."""
    from ..evaluation import ytvis
    evaluator = ytvis.evaluate_results(output_generator.instances, ytvis.ground_truth_from_json(ytvis_annotations), videos=[s.id for s in sequences])
    summary = evaluator.summary()
    print_fn("YouTube-VIS evaluation over %d videos (this library's restatement of the measure; agreement with the official server and "
             "toolkit is unverified): %s" % (summary["counts"]["videos"], " - ".join("%s: %.4f" % (k, summary[k]) for k in ytvis.FIGURES)))
    path = os.path.join(output_dir, "ytvis_eval.json")
    with open(path, "w") as fh:
        json.dump(summary, fh, indent=1)
    print_fn("evaluation written to %s" % path)
    return summary


def run_sequences(track_generator, sequences, output_generator, max_tracks, output_dir, annotations=None, print_fn=print, mots_annotations=None,
                  ytvis_annotations=None):
    """Every sequence through ``run_sequence``, then the writer's ``save()``.  annotations (DAVIS only): see ``attach_evaluator``; the
    summary is logged and written to <output_dir>/davis_eval.json.  mots_annotations (KITTI-MOTS only): see ``evaluate_mots``;
    ytvis_annotations (YouTube-VIS only): see ``evaluate_ytvis``.
    -> the summary, or None."""
    evaluator = attach_evaluator(output_generator, annotations) if annotations is not None else None
    for n, sequence in enumerate(sequences, 1):
        print_fn("sequence %d / %d: %s (%d frames)" % (n, len(sequences), sequence.id, len(sequence)))
        run_sequence(track_generator, sequence, output_generator, max_tracks)
    output_generator.save()
    if mots_annotations is not None:
        return evaluate_mots(output_generator, sequences, mots_annotations, output_dir, print_fn)
    if ytvis_annotations is not None:
        return evaluate_ytvis(output_generator, sequences, ytvis_annotations, output_dir, print_fn)
    if evaluator is None:
        return None
    summary = evaluator.summary()
    print_fn("DAVIS evaluation over %d sequences (this library's restatement of the measure; agreement with the official toolkit is "
             "unverified): %s" % (len(summary["sequences"]), " - ".join("%s: %.4f" % (k, v) for k, v in summary.items() if k != "sequences")))
    path = os.path.join(output_dir, "davis_eval.json")
    with open(path, "w") as fh:
        json.dump(summary, fh, indent=1)
    print_fn("evaluation written to %s" % path)
    return summary


def build_parser():
    """The reference's command line (inference/main.py:289-310), and --eval_annotations."""
    parser = argparse.ArgumentParser(description="run a STEm-Seg model over a dataset's sequences on one MI355X")
    parser.add_argument("model_path")
    parser.add_argument("--output_dir", "-o", required=False)
    parser.add_argument("--seqs", nargs="*", required=False)
    parser.add_argument("--dataset", "-d", required=True)
    parser.add_argument("--max_tracks", type=int, required=False)
    parser.add_argument("--frame_overlap", "-fo", type=int, default=-1)
    parser.add_argument("--seediness_thresh", "-st", type=float, default=0.25)
    parser.add_argument("--min_dim", type=int, required=False)
    parser.add_argument("--max_dim", type=int, required=False)
    parser.add_argument("--resize_embeddings", action="store_true")
    parser.add_argument("--min_seediness_prob", "-msp", type=float, required=False)
    parser.add_argument("--clustering_device", default="cuda:0")
    parser.add_argument("--save_vis", action="store_true")
    # this library's opt-in, --dataset davis only: a video-dataset json WITH segmentations; the J and F measures of every sequence
    parser.add_argument("--eval_annotations", type=str, required=False)
    # this library's opt-in, --dataset kittimots only: a video-dataset json WITH segmentations or a directory of NNNN.txt ground-truth
    # files; sMOTSA, MOTSA and MOTSP of the filtered results
    parser.add_argument("--eval_mots_annotations", type=str, required=False)
    # this library's opt-in, --dataset ytvis only: a video-dataset json WITH segmentations; AP, AP50, AP75, AR1 and AR10 of the instances
    parser.add_argument("--eval_ytvis_annotations", type=str, required=False)
    return parser


def _dataset(name):
    from ..utils import paths
    from ..utils.video_dataset import parse_generic_video_dataset
    where = {"davis": (paths.DavisUnsupervisedPaths.trainval_base_dir, paths.DavisUnsupervisedPaths.val_vds_file),
             "ytvis": (paths.YoutubeVISPaths.val_base_dir, paths.YoutubeVISPaths.val_vds_file),
             "kittimots": (paths.KITTIMOTSPaths.train_images_dir, paths.KITTIMOTSPaths.val_vds_file)}[name]
    return parse_generic_video_dataset(where[0](), where[1]())


def main(args, model=None, sequences=None, print_fn=print):
    """model: an ``InferenceModel`` to run instead of loading ``args.model_path`` (the configuration is then the caller's: no preset is
    loaded); sequences: the parsed sequences to run instead of the dataset's of ``utils/paths.py``.  -> the evaluation summary, or None."""
    from .. import config
    from ..modeling.inference_model import InferenceModel
    from .output_utils import DavisOutputGenerator, KittiMOTSOutputGenerator, YoutubeVISOutputGenerator
    if args.dataset not in DATASETS:
        raise ValueError("Invalid dataset name {} provided: davis | ytvis | kittimots".format(args.dataset))
    if args.eval_annotations is not None and args.dataset != "davis":
        raise ValueError("--eval_annotations computes the DAVIS J and F measures and goes with --dataset davis only, not with --dataset %s" % args.dataset)
    if args.eval_mots_annotations is not None and args.dataset != "kittimots":
        raise ValueError("--eval_mots_annotations computes the KITTI-MOTS measures sMOTSA, MOTSA and MOTSP and goes with --dataset kittimots only, "
                         "not with --dataset %s" % args.dataset)
    if args.eval_ytvis_annotations is not None and args.dataset != "ytvis":
        raise ValueError("--eval_ytvis_annotations computes the YouTube-VIS measures AP, AP50, AP75, AR1 and AR10 and goes with --dataset ytvis only, "
                         "not with --dataset %s" % args.dataset)
    preset, semseg_output_type, max_tracks = DATASETS[args.dataset]
    if model is None:
        config.load_preset(preset)
        if args.min_seediness_prob:
            cfg.CLUSTERING.MIN_SEEDINESS_PROB = args.min_seediness_prob
        if args.min_dim or args.max_dim:          # one of the two: the other keeps the preset's ratio (main.py:201-226)
            ratio = float(cfg.INPUT.MAX_DIM) / float(cfg.INPUT.MIN_DIM)
            cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM = (args.min_dim or int(round(args.max_dim / ratio)), args.max_dim or int(round(args.min_dim * ratio)))
    output_dir = args.output_dir or "inference"
    if not os.path.isabs(output_dir):
        output_dir = os.path.join(os.path.dirname(args.model_path), output_dir)
    os.makedirs(output_dir, exist_ok=True)
    full_scale = bool(cfg.TRAINING.LOSS_AT_FULL_RES or args.resize_embeddings)
    resize_scale = 4.0 if full_scale else 1.0
    meta = {}
    if sequences is None:
        sequences, meta = _dataset(args.dataset)
    if args.seqs:
        sequences = [s for s in sequences if str(s.id) in set(args.seqs)]
    annotations = None
    if args.eval_annotations is not None:
        from ..data.generic_video_dataset_parser import parse_generic_video_dataset
        annotations = {s.id: s for s in parse_generic_video_dataset("", args.eval_annotations)[0]}
    if args.dataset == "davis":
        generator = DavisOutputGenerator(output_dir, OnlineChainer.OUTLIER_LABEL, args.save_vis, upscaled_inputs=full_scale)
    elif args.dataset == "ytvis":
        generator = YoutubeVISOutputGenerator(output_dir, OnlineChainer.OUTLIER_LABEL, args.save_vis, None, meta.get("category_labels"),
                                              upscaled_inputs=full_scale)
    else:
        generator = KittiMOTSOutputGenerator(output_dir, OnlineChainer.OUTLIER_LABEL, args.save_vis, upscaled_inputs=full_scale)
    if model is None:
        model = InferenceModel(args.model_path, semseg_output_type=semseg_output_type, preload_images=args.dataset != "kittimots",
                               resize_scale=resize_scale, semseg_generation_on_gpu=not (args.dataset != "davis" and full_scale)).cuda()
    tracks = TrackGenerator(model, args.dataset, resize_scale=resize_scale, seediness_thresh=args.seediness_thresh,
                            frame_overlap=args.frame_overlap, clustering_device=args.clustering_device)
    summary = run_sequences(tracks, sequences, generator, args.max_tracks or max_tracks, output_dir, annotations, print_fn,
                            mots_annotations=args.eval_mots_annotations, ytvis_annotations=args.eval_ytvis_annotations)
    print_fn("Results saved to {}".format(output_dir))
    return summary


if __name__ == "__main__":
    main(build_parser().parse_args())
