#!/usr/bin/env python3
"""Golden vectors of the embedding loss.  Runs ONLY in the build container: it imports the reference through tools/ref_shim.py, runs
the reference's own EmbeddingLoss on the CPU on the deterministic inputs of tests/loss_oracle.py (FIXTURE_CASES) and writes
tests/golden/embedding_loss.npz: per case the input, the masks and ignore masks of every sample, the four loss values (total, lovasz,
smoothness, seediness) and the gradient of the total with respect to the input.  Data only: no reference source text is stored.

    python tools/make_loss_goldens.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WEIGHTS = dict(WEIGHT_REGULARIZATION=0.001, WEIGHT_LOVASZ=1.0, WEIGHT_VARIANCE_SMOOTHNESS=10.0, WEIGHT_SEEDINESS=1.0, WEIGHT=1.0)


def main():
    import ref_shim
    ref_shim.install()
    import torch
    from stemseg.modeling.losses import EmbeddingLoss
    from stemseg.utils import LossConsts, ModelOutputConsts
    from tests import loss_oracle as LO
    out = {"cases": np.array(sorted(LO.FIXTURE_CASES))}
    for name in sorted(LO.FIXTURE_CASES):
        E, stds, _ = LO.FIXTURE_CASES[name]
        x, targets = LO.make_case(name)
        loss = EmbeddingLoss(4, EMBEDDING_SIZE=E, NBR_FREE_DIMS=len(stds), FREE_DIM_STDS=list(stds), **WEIGHTS)
        xx = x.clone().requires_grad_(True)
        od = {}
        loss(xx, targets, od)
        total = od[ModelOutputConsts.OPTIMIZATION_LOSSES][LossConsts.EMBEDDING]
        total.backward()
        others = od[ModelOutputConsts.OTHERS]
        vals = [float(total)] + [float(others[k]) for k in (LossConsts.LOVASZ_LOSS, LossConsts.VARIANCE_SMOOTHNESS, LossConsts.SEEDINESS_LOSS)]
        out[name + "/x"] = x.numpy()
        out[name + "/losses"] = np.array(vals, np.float64)           # fp32 values, held exactly
        out[name + "/grad"] = xx.grad.numpy()
        out[name + "/embedding_size"] = np.array(E)
        out[name + "/free_dim_stds"] = np.array(stds, np.float64)
        for n, t in enumerate(targets):
            m = t["masks"].numpy()
            out["%s/masks%d_shape" % (name, n)] = np.array(m.shape)
            out["%s/masks%d" % (name, n)] = np.packbits(m.reshape(-1))
            out["%s/ignore%d" % (name, n)] = np.packbits(t["ignore_masks"].numpy().reshape(-1))
        print("%-28s total %.7g lovasz %.7g smoothness %.7g seediness %.7g" % (name, *vals))
    path = os.path.join(ROOT, "tests", "golden", "embedding_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote %s %.1f kB" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
