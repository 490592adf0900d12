"""Labels -> masks in the original image size, on the device.

Mirrors ``DavisOutputGenerator.process_sequence`` (output_utils/davis.py:38-116) up to the point where it hands the
condensed uint8 map to PIL; ``YoutubeVISOutputGenerator`` / ``KittiMOTSOutputGenerator`` run the same chain per instance
(youtube_vis.py:118-155, kitti_mots.py:89-130) -- their binary planes are ``condensed == n + 1``.
Two HIP launches per frame (scatter, fused resample); nothing is synchronised.  More than 255 kept instances (KITTI-MOTS keeps up
to 1000 tracks) switch the map to 16 bits (int16 tensors holding the uint16 bits; ``hip.index_bytes_for``).
"""
import torch

from ... import hip
from ... import config as _config
from ...config import cfg
from ...modeling.inference_model import compute_resize_params_2


def instances_to_keep(instance_lifetimes, outlier_label, max_tracks):
    """Ids by descending lifetime -- stable, so ties keep the dict's order -- without the outlier id, first ``max_tracks``
    (davis.py:57-66)."""
    ranked = sorted([(k, v) for k, v in instance_lifetimes.items()], key=lambda x: x[1], reverse=True)
    return [k for k, _ in ranked if k != outlier_label][:max_tracks]


class MaskMaterializer(object):
    def __init__(self, outlier_label=-1, upscaled_inputs=False):
        self.outlier_label = outlier_label
        self.upscaled_inputs = upscaled_inputs

    def _lut(self, keep, device):
        """(label + 1) -> index in ``keep`` + 1, 0 for everything else (built on the host: a few dozen integers)."""
        top = max([k for k in keep if k >= 0] + [0])
        lut = [0] * (top + 2)
        for n, k in enumerate(keep):
            if k >= 0:
                lut[k + 1] = n + 1
        return torch.tensor(lut, dtype=torch.int32).to(device)

    @torch.no_grad()
    def process_sequence(self, image_dims, track_mask_idxes, track_mask_labels, instance_lifetimes, mask_dims, mask_scale=4.0,
                         max_tracks=10, device="cuda", keep=None):
        """image_dims (height, width) of the original frames; track_mask_idxes[t] = (ys, xs) int64 tensors of frame t's
        foreground points at mask resolution ``mask_dims`` (h, w); track_mask_labels[t] their stitched track ids.
        ``keep``: the instance ids to materialise, in order (default: the lifetime ranking, ``max_tracks`` of them).
        Returns (instances_to_keep, [F, image_height, image_width] on the device: n + 1 where instance instances_to_keep[n]
        covers the pixel) -- uint8 while at most 255 instances are kept, else int16 holding uint16 values."""
        hip.require_gpu()
        _config.refresh()
        assert len(track_mask_idxes) == len(track_mask_labels)
        mask_h, mask_w = mask_dims
        image_h, image_w = image_dims
        if keep is None:
            keep = instances_to_keep(instance_lifetimes, self.outlier_label, max_tracks)
        keep = list(keep)
        ib = hip.index_bytes_for(len(keep))
        lut = self._lut(keep, device)
        rw, rh, _ = compute_resize_params_2((image_w, image_h), cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM)
        scale = 1.0 if self.upscaled_inputs else mask_scale
        out = []
        for (ys, xs), labels in zip(track_mask_idxes, track_mask_labels):
            ys, xs, labels = (t.to(device=device, dtype=torch.int64).contiguous() for t in (ys, xs, labels))
            if ib == 1:
                dense = hip.scatter_instance_index(ys, xs, labels, lut, mask_h, mask_w)
                out.append(hip.resample_instance_masks(dense, scale, (rh, rw), (image_h, image_w)))
            else:
                dense = hip.scatter_instance_index_ex(ys, xs, labels, lut, mask_h, mask_w, ib)
                out.append(hip.resample_instance_masks_ex(dense, scale, (rh, rw), (image_h, image_w), ib))
        return keep, (torch.stack(out, 0) if out else torch.zeros(0, image_h, image_w, dtype=hip.INDEX_DTYPES[ib], device=device))
