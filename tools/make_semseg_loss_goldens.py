#!/usr/bin/env python3
"""Golden vectors of the training targets, the semseg cross-entropy and the foreground loss.  Runs ONLY in the build container: it
imports the reference through tools/ref_shim.py and runs the reference's own TrainingModel.resize_masks (with
instance_masks_to_semseg_mask), CrossEntropyLoss and TrainingModel.compute_fg_loss on the CPU on the deterministic inputs of
tests/semseg_loss_oracle.py (FIXTURE_CASES), split and called as the tail of the reference's forward does.  Writes
tests/golden/semseg_loss.npz: per case the combined logits [N, C, T, h, w], per sample the bit-packed full-resolution masks and ignore
mask, the category ids, the prepared targets (bit-packed 1/4-scale masks and ignore mask, the semantic mask as uint8), the three loss
values (OTHERS semseg, OPTIMIZATION_LOSSES semseg, foreground) and the gradient of (OPTIMIZATION_LOSSES semseg + foreground) with
respect to the combined logits.  Data only: no reference source text is stored.

    python tools/make_semseg_loss_goldens.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import ref_shim
    cfg = ref_shim.install()
    import torch
    from stemseg.modeling.losses import CrossEntropyLoss
    from stemseg.modeling.model_builder import TrainingModel
    from stemseg.utils import LossConsts, ModelOutputConsts
    from tests import semseg_loss_oracle as SO
    out = {"cases": np.array(sorted(SO.FIXTURE_CASES))}
    for name in sorted(SO.FIXTURE_CASES):
        K, has_fg, weight, _ = SO.FIXTURE_CASES[name]
        cfg.TRAINING.LOSSES.update_param("WEIGHT_SEMSEG", float(weight))
        x, targets = SO.make_case(name)
        # the attributes resize_masks and compute_fg_loss read, without building a network
        model = types.SimpleNamespace(output_resize_scale=1.0, embedding_head_output_scale=4, semseg_output_scale=4, semseg_head=object())
        small = TrainingModel.resize_masks(model, [{"masks": t["masks"].clone(), "ignore_masks": t["ignore_masks"].clone(),
                                                    "category_ids": t["category_ids"].clone()} for t in targets])
        xx = x.clone().requires_grad_(True)
        logits = xx.permute(0, 2, 1, 3, 4)                             # [N, T, C, h, w] as forward_embeddings_and_semseg returns it
        od = {ModelOutputConsts.OPTIMIZATION_LOSSES: {}, ModelOutputConsts.OTHERS: {}}
        if has_fg:
            logits, fg_logits = logits.split((logits.shape[2] - 1, 1), dim=2)
            TrainingModel.compute_fg_loss(model, fg_logits.squeeze(2), small, od)
        CrossEntropyLoss()(logits, small, od)
        opt = od[ModelOutputConsts.OPTIMIZATION_LOSSES]
        total = opt[LossConsts.SEMSEG] + (opt[LossConsts.FOREGROUND] if has_fg else 0.)
        total.backward()
        vals = [float(od[ModelOutputConsts.OTHERS][LossConsts.SEMSEG]), float(opt[LossConsts.SEMSEG]),
                float(opt[LossConsts.FOREGROUND]) if has_fg else 0.]
        out[name + "/x"] = x.numpy()
        out[name + "/losses"] = np.array(vals, np.float64)            # fp32 values, held exactly
        out[name + "/grad"] = xx.grad.numpy()
        out[name + "/n_classes"], out[name + "/has_fg"], out[name + "/weight_semseg"] = np.array(K), np.array(has_fg), np.array(weight)
        for n, (t, s) in enumerate(zip(targets, small)):
            m = t["masks"].numpy()
            assert s["masks"].dtype == torch.uint8 and s["ignore_masks"].dtype == torch.uint8 and s["semseg_masks"].dtype == torch.int64
            assert int(s["masks"].max()) <= 1 and 0 <= int(s["semseg_masks"].min()) and int(s["semseg_masks"].max()) <= 255
            out["%s/masks%d_shape" % (name, n)] = np.array(m.shape)
            out["%s/masks%d" % (name, n)] = np.packbits(m.reshape(-1))
            out["%s/ignore%d" % (name, n)] = np.packbits(t["ignore_masks"].numpy().reshape(-1))
            out["%s/category_ids%d" % (name, n)] = t["category_ids"].numpy()
            out["%s/small_masks%d" % (name, n)] = np.packbits(s["masks"].numpy().reshape(-1))
            out["%s/small_ignore%d" % (name, n)] = np.packbits(s["ignore_masks"].numpy().reshape(-1))
            out["%s/semseg%d" % (name, n)] = s["semseg_masks"].numpy().astype(np.uint8)
        print("%-22s semseg %.7g weighted %.7g foreground %.7g  grad NaNs %d" % (name, *vals, int(np.isnan(out[name + "/grad"]).sum())))
    cfg.TRAINING.LOSSES.update_param("WEIGHT_SEMSEG", 1.0)
    path = os.path.join(ROOT, "tests", "golden", "semseg_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote %s %.1f kB" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
