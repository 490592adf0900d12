"""Per-dataset output generators with the reference's call contract (``inference/main.py:166-169,248-262``):
``process_sequence(sequence, track_mask_idxes, track_mask_labels, instance_pt_counts, instance_lifetimes, category_masks,
mask_dims, mask_scale, max_tracks, device)`` and ``save()``.

The device-side half (instances to keep, labels -> full-resolution masks) is ``MaskMaterializer``.  The DAVIS writer writes an
indexed PNG per frame (``output_utils/davis.py:108-121``).  The YouTube-VIS json and KITTI-MOTS txt writers take the COCO RLE
strings, areas and per-instance class statistics from the device (``hip.rle_encode``, ``hip.instance_class_stats``): one copy of
the strings to the host per sequence; string and file handling stay on the host.

``save_visualization=True`` (the reference's ``--save_vis``) also writes one overlay JPEG per frame, at the reference's paths:
``<output_dir>/vis/<seq.id>/`` (DAVIS, YouTube-VIS) and ``<output_dir>/vis/<int(seq.id):04d>/`` (KITTI-MOTS), ``{t:05d}.jpg``.
The frames come from ``sequence.load_images(frame_idxes)`` (BGR uint8, as cv2 reads them) in chunks of ``VIS_CHUNK`` frames; each
chunk makes one copy to the device, where the overlay of the condensed map the writer already holds (``hip.vis_composite``) and
the JPEG encode (``hip.jpeg_encode``: the bytes of libjpeg-turbo / cv2.imwrite at quality 95) run, then one copy of the files
back.  Colours: ``pascal_color_map()[n % 256]`` for kept instance n in all three formats.  Out of scope:
the box outline, label plate and Hershey text that the reference's YouTube-VIS / KITTI-MOTS writers draw with cv2 per instance
(``output_utils/common.py:23-56``) -- those images get the overlays without the annotations.  A sequence without
``load_images`` gets its results and a warning, no ``vis/``.
"""
import json
import inspect
import os
import warnings
from collections import OrderedDict
from glob import glob
from zipfile import ZipFile

import numpy as np
import torch

from ... import hip
from . import coco_rle
from .masks import MaskMaterializer, instances_to_keep


def pascal_color_map(n=256):
    """The PASCAL-VOC / DAVIS palette: bit-interleaved colours, uint8 [n, 3]."""
    cmap = np.zeros((n, 3), np.uint8)
    for i in range(n):
        c, rgb = i, [0, 0, 0]
        for j in range(8):
            for ch in range(3):
                rgb[ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
        cmap[i] = rgb
    return cmap


VIS_CHUNK = 16          # frames per load / copy / encode round of the visualisations (bounds host and device memory)
VIS_QUALITY = 95        # cv2.imwrite's default JPEG quality


def _device(device):
    return "cuda" if str(device) == "cpu" else device               # the kernels run on the GPU whatever the writer asked for


class _OutputGeneratorBase(object):
    def __init__(self, output_dir, outlier_label, save_visualization, *args, **kwargs):
        self.results_output_dir = os.path.join(output_dir, "results")
        self.vis_output_dir = os.path.join(output_dir, "vis")
        self.outlier_label = outlier_label
        self.save_visualization = save_visualization
        self.upscaled_inputs = bool(kwargs.get("upscaled_inputs"))
        self.sequences = {}

    def _materialize(self, sequence, track_mask_idxes, track_mask_labels, instance_lifetimes, mask_dims, mask_scale, max_tracks, device,
                     keep=None):
        m = MaskMaterializer(self.outlier_label, self.upscaled_inputs)
        return m.process_sequence(sequence.image_dims, track_mask_idxes, track_mask_labels, instance_lifetimes, mask_dims,
                                  mask_scale, max_tracks, _device(device), keep=keep)

    def save(self, *args, **kwargs):
        pass

    device_decode = True        # the frames of the visualisations are decoded on the device when the sequence can (False: host)

    def _save_visualizations(self, sequence, index_map, colors, out_dir):
        """Overlay JPEGs of every frame of ``sequence`` into ``out_dir``: index_map [T, H, W] (device, uint8 / int16-as-uint16),
        colors [K+1, 3] uint8 (row n = colour of instance n)."""
        load = getattr(sequence, "load_images", None)
        if load is None:
            warnings.warn("save_visualization: sequence %r has no load_images(); no visualisations written" % (sequence.id,))
            return
        os.makedirs(out_dir, exist_ok=True)
        T, H, W = (int(v) for v in index_map.shape)
        cols = torch.from_numpy(np.ascontiguousarray(colors, dtype=np.uint8)).to(index_map.device)
        on_device = self.device_decode and "device" in inspect.signature(load).parameters
        for t0 in range(0, T, VIS_CHUNK):
            idx = list(range(t0, min(T, t0 + VIS_CHUNK)))
            images = load(idx, device=index_map.device) if on_device else load(idx)
            assert len(images) == len(idx), "Got {} images for {} frames".format(len(images), len(idx))
            for im in images:
                assert tuple(im.shape) == (H, W, 3), "Image has shape {} while the sequence has dims {}".format(tuple(im.shape), (H, W))
            if torch.is_tensor(images):                    # decoded on the device: composited and encoded there, never copied
                frames = images.contiguous()
            else:
                frames = torch.from_numpy(np.stack(images).astype(np.uint8, copy=False)).to(index_map.device)
            data, offsets = hip.jpeg_encode(hip.vis_composite(frames, index_map[t0:idx[-1] + 1], cols), VIS_QUALITY)
            for i, t in enumerate(idx):
                with open(os.path.join(out_dir, "{:05d}.jpg".format(t)), "wb") as fh:
                    fh.write(data[offsets[i]:offsets[i + 1]].tobytes())


class DavisOutputGenerator(_OutputGeneratorBase):
    """``index_map_hook``: None, or ``hook(sequence, keep, masks)`` called with every sequence's index maps (uint8 / 16-bit [T,H,W] on the
    device, label n = ``keep[n - 1]``) after its PNGs are written and before the maps are freed -- the evaluator's seat
    (``inference/main.py --eval_annotations``)."""
    index_map_hook = None

    def process_sequence(self, sequence, track_mask_idxes, track_mask_labels, instance_pt_counts, instance_lifetimes,
                         category_masks, mask_dims, mask_scale, max_tracks, device="cpu"):
        from PIL import Image
        keep, masks = self._materialize(sequence, track_mask_idxes, track_mask_labels, instance_lifetimes, mask_dims, mask_scale,
                                        max_tracks, device)
        out_dir = os.path.join(self.results_output_dir, str(sequence.id))
        os.makedirs(out_dir, exist_ok=True)
        palette = pascal_color_map().flatten().tolist()
        for t, m in enumerate(masks.cpu().numpy()):
            im = Image.fromarray(m)
            im.putpalette(palette)
            im.save(os.path.join(out_dir, "{:05d}.png".format(t)))
        if self.save_visualization:
            self._save_visualizations(sequence, masks, pascal_color_map()[:len(keep) + 1],
                                      os.path.join(self.vis_output_dir, str(sequence.id)))
        if self.index_map_hook is not None:
            self.index_map_hook(sequence, keep, masks)
        return keep, dict()


class _RleGenerator(_OutputGeneratorBase):
    """Shared device half of the RLE writers: the condensed index map of the kept instances, their per-frame point counts and
    class statistics (one launch sequence for all frames), and the COCO RLE of every (frame, kept instance) plane.

    ``keep_masks`` (default True): keep the materialised masks in ``.sequences[seq_id]`` as before the writers existed; pass
    False for dataset-scale runs."""

    def __init__(self, output_dir, outlier_label, save_visualization, *args, **kwargs):
        self.keep_masks = kwargs.pop("keep_masks", True)
        super().__init__(output_dir, outlier_label, save_visualization, *args, **kwargs)

    def _device_pass(self, sequence, track_mask_idxes, track_mask_labels, instance_lifetimes, category_masks, mask_dims, mask_scale,
                     keep, device, logits=None, argmax=None, n_votes=0):
        dev = _device(device)
        keep, masks = self._materialize(sequence, track_mask_idxes, track_mask_labels, instance_lifetimes, mask_dims, mask_scale,
                                        len(keep), dev, keep=keep)
        if self.keep_masks:
            self.sequences[sequence.id] = dict(instances=keep, masks=masks, category_masks=category_masks)   # plane n: masks == n + 1
        K = len(keep)
        lut = MaskMaterializer(self.outlier_label)._lut(keep, masks.device)
        sizes = [int(l.numel()) for l in track_mask_labels]
        cat = lambda ts: torch.cat([t.to(device=masks.device, dtype=torch.int64).reshape(-1) for t in ts]) if ts else \
            torch.zeros(0, dtype=torch.int64, device=masks.device)
        ys, xs = cat([c[0] for c in track_mask_idxes]), cat([c[1] for c in track_mask_idxes])
        labels = cat(track_mask_labels)
        points, sums, votes = hip.instance_class_stats(ys, xs, labels, sizes, lut, K, tuple(mask_dims), logits=logits, argmax=argmax,
                                                       n_votes=n_votes)
        extra = [points] + [t for t in (sums, votes) if t is not None]
        rle, host = hip.rle_encode(masks, K, with_counts=False, extra=extra)      # (the one copy to the host)
        return keep, rle, host, masks


class YoutubeVISOutputGenerator(_RleGenerator):
    """YouTube-VIS results (output_utils/youtube_vis.py:51-239): per kept instance (lifetime ranking, ``max_tracks`` < 256) a
    score = point count / the largest kept point count, a category = 1 + arg-max of softmax(class sums / area) over the
    multi-class maps' channels 1..C-1 (ties: the lowest id), and one RLE per frame.  ``save()`` writes ``results.json`` and
    ``results.zip`` to the output directory.  ``category_masks``: float [T, C, h, w] (the "logits" semseg output)."""

    def __init__(self, output_dir, outlier_label, save_visualization, category_mapping=None, category_names=None, *args, **kwargs):
        super().__init__(output_dir, outlier_label, save_visualization, *args, **kwargs)
        self.category_mapping, self.category_names = category_mapping, category_names
        self.output_dir = output_dir
        self.instances = []
        os.makedirs(output_dir, exist_ok=True)

    def process_sequence(self, sequence, track_mask_idxes, track_mask_labels, instance_pt_counts, instance_lifetimes,
                         category_masks, mask_dims, mask_scale, max_tracks, device="cpu"):
        assert len(track_mask_idxes) == len(track_mask_labels)
        assert max_tracks < 256
        if not torch.is_tensor(category_masks):
            raise TypeError("YoutubeVISOutputGenerator needs the dense multi-class maps, a float tensor [T, C, h, w]")
        assert category_masks.shape[0] == len(track_mask_idxes) and tuple(category_masks.shape[-2:]) == tuple(mask_dims), \
            "Shape mismatch between semantic masks {} and embedding masks {}".format(tuple(category_masks.shape), tuple(mask_dims))
        keep = instances_to_keep(instance_lifetimes, self.outlier_label, max_tracks)
        if not keep:
            return None
        logits = category_masks.to(device=_device(device), dtype=torch.float32).contiguous()
        keep, rle, (points, sums), masks = self._device_pass(sequence, track_mask_idxes, track_mask_labels, instance_lifetimes,
                                                             category_masks, mask_dims, mask_scale, keep, device, logits=logits)
        pts = {k: instance_pt_counts[k] for k in keep}
        max_pts = float(max(pts.values()))
        area = points.sum(0).astype(np.float32)                       # points per instance over the sequence (float, as :124)
        image_h, image_w = sequence.image_dims
        for n, k in enumerate(keep, 1):
            probs = torch.from_numpy(sums[n - 1].astype(np.float32) / area[n - 1]).softmax(0).numpy()
            self.instances.append({
                "video_id": sequence.id,
                "score": float(pts[k]) / max_pts,
                "category_id": int(np.argmax(probs)) + 1,              # first maximum: the stable descending sort of :171-175
                "segmentations": [{"size": [image_h, image_w], "counts": rle.strings[rle.plane(f, n)]} for f in range(rle.F)],
            })
        if self.save_visualization:
            self._save_visualizations(sequence, masks, pascal_color_map()[np.arange(len(keep) + 1) % 256],
                                      os.path.join(self.vis_output_dir, str(sequence.id)))
        return keep, dict()

    def save(self, *args, **kwargs):
        path = os.path.join(self.output_dir, "results.json")
        with open(path, "w") as fh:
            json.dump(self.instances, fh)
        with ZipFile(os.path.join(self.output_dir, "results.zip"), "w") as zf:
            zf.write(path, arcname="results.json")


class KittiMOTSOutputGenerator(_RleGenerator):
    """KITTI-MOTS results (output_utils/kitti_mots.py:31-248): the ``max_tracks`` instances with the most points, ordered by
    ascending lifetime, mapped to ids 1..N; one line ``frame cat*1000+id cat h w rle`` per (instance, frame) in which the instance
    has points, grouped by id, then by frame, in ``results/{seq.id:04d}.txt``; category = the arg-max vote of classes (1, 2) over
    the instance's points (ties: 1).  ``save()`` applies the track filters of kitti_mots_postprocessing.py into ``results_nms/``.
    ``category_masks``: int64 [T, h, w] (the "argmax" semseg output)."""
    CATEGORIES = (1, 2)

    def process_sequence(self, sequence, track_mask_idxes, track_mask_labels, instance_pt_counts, instance_lifetimes,
                         category_masks, mask_dims, mask_scale, max_tracks, device="cpu"):
        assert len(track_mask_idxes) == len(track_mask_labels)
        if not torch.is_tensor(category_masks):
            raise TypeError("KittiMOTSOutputGenerator needs the dense class arg-max maps, an int64 tensor [T, h, w]")
        assert category_masks.shape[0] == len(track_mask_idxes) and tuple(category_masks.shape[-2:]) == tuple(mask_dims), \
            "Shape mismatch between semantic masks {} and embedding masks {}".format(tuple(category_masks.shape), tuple(mask_dims))
        keep = instances_to_keep(instance_pt_counts, self.outlier_label, max_tracks)         # by point count (:56-61)
        keep = sorted(keep, key=lambda k: instance_lifetimes[k])                              # then ascending lifetime (:66)
        if not keep:
            raise ValueError("Zero instances detected in sequence: {}".format(sequence.id))
        argmax = category_masks.to(device=_device(device), dtype=torch.int64).contiguous()
        n_votes = max(self.CATEGORIES) + 1
        keep, rle, (points, votes), masks = self._device_pass(sequence, track_mask_idxes, track_mask_labels, instance_lifetimes,
                                                              category_masks, mask_dims, mask_scale, keep, device, argmax=argmax,
                                                              n_votes=n_votes)
        image_h, image_w = sequence.image_dims
        lines = []
        for n in range(1, len(keep) + 1):
            cat = max(self.CATEGORIES, key=lambda c: votes[n - 1][c])          # first maximum: category 1 on ties (:179-180)
            for t in range(rle.F):
                if points[t][n - 1] > 0:
                    lines.append("{} {} {} {} {} {}\n".format(t, cat * 1000 + n, cat, image_h, image_w, rle.strings[rle.plane(t, n)]))
        os.makedirs(self.results_output_dir, exist_ok=True)
        with open(os.path.join(self.results_output_dir, "{:04d}.txt".format(int(sequence.id))), "w") as fh:
            fh.writelines(lines)
        if self.save_visualization:
            # kitti_mots.py:230 colours by the frame instance's "instance_id", which is the mapped id n (:169), not cat * 1000 + n
            self._save_visualizations(sequence, masks, pascal_color_map()[np.arange(len(keep) + 1) % 256],
                                      os.path.join(self.vis_output_dir, "{:04d}".format(int(sequence.id))))
        return keep, {n: k for n, k in enumerate(keep, 1)}

    def save(self, *args, **kwargs):
        kitti_mots_filter(self.results_output_dir)


# ------------------------------------------------------------------------------------------------ KITTI-MOTS track filters
KITTI_FILTER_DEFAULTS = dict(min_car_area=150, min_person_area=250, min_track_length_car=3, min_track_length_person=10,
                             min_area_ratio_car=0.35, min_area_ratio_person=0.2, max_time_break_ratio_car=0.3,
                             max_time_break_ratio_person=0.5)


class _Detection(object):
    __slots__ = ("frame_id", "track_id", "class_id", "h", "w", "counts_str", "area", "bbox_area")

    def __init__(self, line):
        f = line.strip().split(" ")
        self.frame_id, self.track_id, self.class_id, self.h, self.w = (int(v) for v in f[:5])
        self.counts_str = f[5]
        c = coco_rle.string_to_counts(self.counts_str)
        self.area = coco_rle.area(c)
        _, _, bw, bh = coco_rle.to_bbox(c, self.h)
        self.bbox_area = bw * bh

    def ratio(self):
        return 0.0 if self.bbox_area == 0 else float(self.area) / float(self.bbox_area)

    def as_txt(self):
        return "{} {} {} {} {} {}".format(self.frame_id, self.track_id, self.class_id, self.h, self.w, self.counts_str)


def _tracks(dets):
    by_id = OrderedDict()
    for d in dets:
        by_id.setdefault(d.track_id, []).append(d)
    return [sorted(v, key=lambda d: d.frame_id) for v in by_id.values()]


def _filter_tracks(dets, keep_track):
    return [d for t in _tracks(dets) if keep_track(t) for d in t]


def kitti_mots_filter(results_dir, output_dir_suffix="nms", **kwargs):
    """kitti_mots_postprocessing.py:145-180 on every ``results_dir/????.txt`` -> ``results_dir_<suffix>/``: per-detection area
    and area / bbox-area filters, then per-track time-break and length filters (classes 1 = car, 2 = pedestrian)."""
    p = dict(KITTI_FILTER_DEFAULTS, **kwargs)
    out_dir = results_dir + "_" + output_dir_suffix
    os.makedirs(out_dir, exist_ok=True)
    for path in sorted(glob(os.path.join(results_dir, "????.txt"))):
        with open(path) as fh:
            dets = [_Detection(l) for l in fh.readlines()]
        dets = [d for d in dets if (d.class_id == 1 and d.area >= p["min_car_area"]) or (d.class_id == 2 and d.area >= p["min_person_area"])]
        dets = [d for d in dets if (d.class_id == 1 and d.ratio() > p["min_area_ratio_car"]) or
                (d.class_id == 2 and d.ratio() > p["min_area_ratio_person"])]

        def breaks_ok(t):
            r = float(sum(int(t[i + 1].frame_id - t[i].frame_id > 1) for i in range(len(t) - 1))) / float(len(t))
            return not ((t[0].class_id == 1 and r > p["max_time_break_ratio_car"]) or (t[0].class_id == 2 and r > p["max_time_break_ratio_person"]))

        def length_ok(t):
            return not ((t[0].class_id == 1 and len(t) < p["min_track_length_car"]) or
                        (t[0].class_id == 2 and len(t) < p["min_track_length_person"]))
        dets = _filter_tracks(dets, breaks_ok)
        dets = _filter_tracks(dets, length_ok)
        with open(os.path.join(out_dir, os.path.basename(path)), "w") as fh:
            fh.writelines([d.as_txt() + "\n" for d in dets])
    return out_dir
