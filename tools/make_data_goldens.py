#!/usr/bin/env python3
"""Golden vectors of the training data pipeline.  Runs ONLY in the build container: it imports the reference through tools/ref_shim.py
(which stubs cv2 / pycocotools / imgaug) and runs the reference's own loaders, samplers and ``VideoDataset.__getitem__`` + ``collate_fn``
on a synthetic dataset that this tool writes, with ``load_images`` / ``load_masks`` replaced by this tool's arrays (the files decoded with
PIL, the RLE strings decoded with tests/writer_oracle.py).  Writes tests/golden/data_pipeline.npz.  Data only: no reference source text.

    python tools/make_data_goldens.py
"""
import io
import json
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT]

NUM_FRAMES, MIN_DIM, MAX_DIM = 4, 48, 80
GAPS = {"DAVIS": (4, 6), "YOUTUBE_VIS": (4, 5), "KITTI_MOTS": (4, 6)}
SEED = 1234
CLIP_A = ["a/%05d.jpg" % t for t in (0, 2, 4, 6)]
CLIP_B = ["b/%05d.png" % t for t in (1, 3, 5, 8)]


def synth_image(h, w, t, seed):
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    rs = np.random.RandomState(seed)
    ph = rs.rand(3) * 6.0
    img = np.stack([127 + 100 * np.sin(yy / (5.0 + c) + ph[c] + 0.3 * t) * np.cos(xx / (7.0 + 2 * c) - 0.2 * t) for c in range(3)], -1)
    img[(yy - h / 2 - t) ** 2 + (xx - w / 3 - 2 * t) ** 2 < (min(h, w) / 5.0) ** 2] += 40
    return np.clip(img, 0, 255).astype(np.uint8)


def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.ogrid[:h, :w]
    return (((yy - cy) / float(ry)) ** 2 + ((xx - cx) / float(rx)) ** 2 <= 1.0).astype(np.uint8)


def make_dataset():
    """-> (dataset dict, {path: file bytes})"""
    from PIL import Image
    from tests import data_oracle as do
    files, seqs = {}, []

    def add(seq_id, h, w, n, ext, cats, present):
        paths, segs = [], []
        for t in range(n):
            path = "%s/%05d.%s" % (seq_id, t, ext)
            buf = io.BytesIO()
            Image.fromarray(synth_image(h, w, t, len(seqs))).save(buf, "JPEG" if ext == "jpg" else "PNG", **({"quality": 90} if ext == "jpg" else {}))
            files[path] = buf.getvalue()
            paths.append(path)
            seg = {}
            for k, iid in enumerate(cats):
                if present(t, iid):
                    m = ellipse(h, w, h * (0.3 + 0.2 * k) + t, w * (0.25 + 0.25 * k) + 1.5 * t, 4 + 2 * k, 6 + k)
                    seg[str(iid)] = do.mask_string(m)
            segs.append(seg)
        seqs.append({"id": seq_id, "height": h, "width": w, "image_paths": paths, "categories": {str(i): c for i, c in cats.items()},
                     "segmentations": segs})

    # a: 37 x 53 JPEG, 20 frames; instance 7 is the ignore category 3; frames 8..14 hold nothing but it (a gap that splits), instance 4
    #    is absent from frame 2
    add("a", 37, 53, 20, "jpg", {4: 1, 2: 2, 7: 3}, lambda t, iid: iid == 7 or (not 8 <= t <= 14 and not (iid == 4 and t == 2)))
    # b: 45 x 40 PNG, 10 frames; frame 4 has no annotation at all
    add("b", 45, 40, 10, "png", {9: 2, 5: 1}, lambda t, iid: t != 4 and not (iid == 9 and t == 8))
    add("c", 45, 40, 3, "png", {1: 1}, lambda t, iid: True)                      # too short for any clip
    add("d", 45, 40, 7, "png", {3: 2, 1: 1}, lambda t, iid: iid == 1 or t % 2 == 0)
    return {"meta": {"category_labels": {"1": "car", "2": "person", "3": "ignore"}}, "sequences": seqs}, files


def main():
    import ref_shim
    cfg = ref_shim.install(num_frames=NUM_FRAMES)
    import torch
    from PIL import Image
    from torch.utils.data.sampler import BatchSampler, SequentialSampler
    from tests import writer_oracle as wo
    from stemseg.data import DavisDataLoader, MOTSDataLoader, YoutubeVISDataLoader
    from stemseg.data.common import collate_fn
    from stemseg.data.concat_dataset import ConcatDataset
    from stemseg.data.distributed_data_sampler import DistributedSampler
    from stemseg.data.generic_video_dataset_parser import GenericVideoSequence
    from stemseg.data.iteration_based_batch_sampler import IterationBasedBatchSampler

    cfg.INPUT.update_param("MIN_DIM", MIN_DIM)
    cfg.INPUT.update_param("MAX_DIM", MAX_DIM)
    for section, (lo, hi) in GAPS.items():
        cfg.DATA[section].update_param("FRAME_GAP_LOWER", lo)
        cfg.DATA[section].update_param("FRAME_GAP_UPPER", hi)

    dataset, files = make_dataset()
    decoded = {p: np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))[:, :, ::-1]) for p, b in files.items()}      # BGR

    def load_images(self, frame_idxes=None):
        idx = range(len(self.image_paths)) if frame_idxes is None else frame_idxes
        return [decoded[self.image_paths[t]].copy() for t in idx]

    def load_masks(self, frame_idxes=None):
        idx = range(len(self.image_paths)) if frame_idxes is None else frame_idxes
        h, w = self.image_dims
        return [[np.ascontiguousarray(wo.decode(wo.string_to_counts(self.segmentations[t][iid]), h, w).astype(np.uint8))
                 if iid in self.segmentations[t] else np.zeros((h, w), np.uint8) for iid in self.instance_ids] for t in idx]
    GenericVideoSequence.load_images, GenericVideoSequence.load_masks = load_images, load_masks

    out = {"dataset_json": np.array(json.dumps(dataset)), "config": np.array(json.dumps({"NUM_FRAMES": NUM_FRAMES, "MIN_DIM": MIN_DIM, "MAX_DIM": MAX_DIM, "GAPS": GAPS, "SEED": SEED})),
           "file_names": np.array(sorted(files)), "file_sizes": np.array([len(files[p]) for p in sorted(files)], np.int64),
           "file_bytes": np.frombuffer(b"".join(files[p] for p in sorted(files)), np.uint8)}

    def pick(sequences, seq_id, paths):
        for seq in sequences:
            if (seq.id == seq_id or str(seq.id).startswith(seq_id + "_")) and all(p in seq.image_paths for p in paths):
                return seq.extract_subsequence([seq.image_paths.index(p) for p in paths])
        raise KeyError(seq_id)

    def describe(seqs):
        return [{"id": s.id, "image_paths": s.image_paths, "instance_ids": s.instance_ids, "category_labels": s.category_labels} for s in seqs]

    record, images_seen, loaders = {}, None, {}
    with tempfile.TemporaryDirectory() as tmp:
        vds = os.path.join(tmp, "dataset.json")
        with open(vds, "w") as fh:
            json.dump(dataset, fh)
        makers = {"ytvis": lambda: YoutubeVISDataLoader(tmp, vds, 7, category_agnostic=False),
                  "davis": lambda: DavisDataLoader(tmp, vds, samples_to_create=7),
                  "mots": lambda: MOTSDataLoader(tmp, vds, 7)}
        for name, make in makers.items():
            random.seed(SEED)
            ds = loaders[name] = make()
            record[name + "_samples"] = describe(ds.samples)
            record[name + "_sequences"] = describe(ds.sequences)
            sampled, ds_pair = ds.samples, ds
            ds_pair.samples = [pick(ds.sequences, "a", CLIP_A), pick(ds.sequences, "b", CLIP_B)]
            image_seqs, targets, meta = collate_fn([ds_pair[0], ds_pair[1]])
            pair_ids = [s.instance_ids for s in ds_pair.samples]
            ds.samples = sampled
            imgs = image_seqs.tensors.numpy().astype(np.float32)
            assert images_seen is None or np.array_equal(images_seen, imgs)
            images_seen = imgs
            record[name + "_batch"] = {"image_sizes": [list(map(int, s)) for s in image_seqs.image_sizes],
                                       "original_image_sizes": [list(map(int, s)) for s in image_seqs.original_image_sizes],
                                       "max_size": list(map(int, image_seqs.max_size)), "seq_names": [m["seq_name"] for m in meta],
                                       "category_ids": [t["category_ids"].tolist() for t in targets],
                                       "instance_ids": pair_ids}
            for n, t in enumerate(targets):
                out["%s_masks_%d" % (name, n)] = t["masks"].numpy().astype(np.uint8)
                out["%s_ignore_%d" % (name, n)] = t["ignore_masks"].numpy().astype(np.uint8)
        out["batch_images"] = images_seen

        # the dataset mix: a dataset smaller than its share (repeated and topped up) and one larger (thinned)
        for key, total, weights in (("concat_repeat", 20, [0.6, 0.4]), ("concat_sparse", 10, [0.5, 0.5])):
            random.seed(SEED)
            mix = ConcatDataset([loaders["ytvis"], loaders["davis"]], total, weights)
            record[key] = {"total": total, "weights": weights, "id_mapping": [list(map(int, p)) for p in mix.id_mapping],
                           "samples_per_dataset": mix.samples_per_dataset}

    span = list(range(10))
    record["distributed_sampler"] = [{"world": world, "rank": rank, "shuffle": shuffle, "epoch": epoch, "indices": idx}
                                     for world in (1, 2, 3) for rank in range(world) for shuffle, epoch in ((True, 0), (True, 3), (False, 0))
                                     for idx in [_sampler_indices(DistributedSampler, span, world, rank, shuffle, epoch)]]
    plain = IterationBasedBatchSampler(BatchSampler(SequentialSampler(span), 3, False), 9, 4)
    shard = IterationBasedBatchSampler(BatchSampler(DistributedSampler(span, 2, 1, True), 2, False), 9, 3)
    record["iteration_sampler"] = {"plain": [list(b) for b in plain], "plain_len": len(plain), "sharded": [list(b) for b in shard]}
    out["record_json"] = np.array(json.dumps(record))

    path = os.path.join(ROOT, "tests", "golden", "data_pipeline.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d kB, %d files, %d keys" % (path, os.path.getsize(path) // 1024, len(files), len(out)))


def _sampler_indices(cls, span, world, rank, shuffle, epoch):
    s = cls(span, world, rank, shuffle)
    s.set_epoch(epoch)
    return list(map(int, s))


if __name__ == "__main__":
    main()
