"""``CrossEntropyLoss`` (modeling/losses/cross_entropy.py:9-48) and the foreground loss of ``TrainingModel.compute_fg_loss``
(modeling/model_builder.py:210-244): value and gradient with respect to the semseg head's output, on the device
(csrc/semseg_loss.hip).  Both come from ONE forward and one backward launch per sample over the head's combined logits.

Reference behaviour kept on purpose: ``F.cross_entropy`` runs with its default 'mean' reduction, so the ignore mask does not mask the
cross-entropy -- it is the mean over every voxel of the sample, and NaN (0 / 0) when every voxel is ignored.  The foreground loss is
masked.  Not kept: ``F.cross_entropy`` skips targets equal to -100; here a target id outside the class channels raises ValueError."""
import torch
import torch.nn as nn

from ... import hip
from ...config import cfg
from ...utils.constants import Loss as LossConsts, ModelOutput as ModelOutputConsts


def _class_ids(t, device):
    """The semantic mask as uint8 class ids on ``device``; an id outside 0..254 becomes 255, which no head has (the device flags it)."""
    t = t.to(device)
    if t.dtype == torch.uint8:
        return t.contiguous()
    assert t.dtype in (torch.int64, torch.int32, torch.int16, torch.int8), "semseg_masks must hold integer class ids, got %s" % t.dtype
    return torch.where((t < 0) | (t > 254), torch.full_like(t, 255), t).to(torch.uint8).contiguous()


class SemsegLossFunction(torch.autograd.Function):
    """(logits [N,C,T,H,W] float32 in any strides, semseg masks list, ignore masks list, class channels K, has_foreground_channel)
    -> (cross-entropy, foreground loss): two fp32 scalars, each the mean over the N samples.  C = K + has_foreground_channel; K = 0 is
    the foreground channel alone.  ``backward`` writes each sample's gradient once, in the strides of the input."""

    @staticmethod
    def forward(ctx, logits, semseg_masks, ignore_masks, n_classes, has_fg):
        assert logits.dtype == torch.float32 and logits.dim() == 5
        x = logits.detach()
        N, Cn, T, H, W = x.shape
        assert Cn == n_classes + int(has_fg), "Expected {} channels in input tensor, got {}".format(n_classes + int(has_fg), Cn)
        assert len(semseg_masks) == N and len(ignore_masks) == N
        dev = x.device
        samples, outs, flags = [], [], []
        with torch.cuda.device(dev):
            for n in range(N):
                sem, ig = _class_ids(semseg_masks[n], dev), ignore_masks[n].to(dev)
                assert tuple(sem.shape) == (T, H, W), "Shape mismatch between ground truth semseg masks {} and predicted semseg masks {}".format(
                    tuple(sem.shape), tuple(x.shape))
                assert tuple(ig.shape) == (T, H, W), "Shape mismatch between ground truth semseg masks {} and ignore masks {} ".format(
                    tuple(sem.shape), tuple(ig.shape))
                desc = hip.semseg_loss_desc(n_classes, has_fg, T, H, W, x[n].stride())
                out, flag, ws = hip.semseg_loss_forward(desc, x[n], sem, ig)
                outs.append(out)
                flags.append(flag)
                samples.append((desc, sem, ig, ws))
            if int(torch.cat(flags).max()):                    # the one readback
                raise ValueError("semseg_masks holds a class id outside the %d class channels of the logits" % n_classes)
        ctx.samples, ctx.n_classes, ctx.has_fg = samples, n_classes, bool(has_fg)
        ctx.set_materialize_grads(False)                       # backward tells "not differentiated" (None) from an upstream of zero
        ctx.save_for_backward(x)
        s = torch.stack(outs)                                  # fp64 [N, 4]: ce sum, voxels, fg sum, non-ignored voxels
        ce = torch.where(s[:, 3] > 0, s[:, 0] / s[:, 1], torch.full_like(s[:, 0], float("nan")))
        r = (torch.stack([ce.sum(), (s[:, 2] / s[:, 3]).sum()]) / N).float()
        return r[0], r[1]

    @staticmethod
    def backward(ctx, g_ce, g_fg):
        x, = ctx.saved_tensors
        if g_ce is None and g_fg is None:
            return None, None, None, None, None
        grad = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
        up = torch.stack([torch.zeros((), device=x.device) if g is None else g.detach().float().reshape(()) for g in (g_ce, g_fg)]).contiguous()
        with torch.cuda.device(x.device):
            for n, (desc, sem, ig, ws) in enumerate(ctx.samples):
                hip.semseg_loss_backward(desc, x[n], sem, ig, ws, up, x.shape[0], grad[n])
        # a loss that is not part of the differentiated scalar leaves exact zeros in its channels, as autograd does for the reference --
        # also next to an all-ignored sample, where an upstream of ZERO still gives 0 * NaN = NaN (the kernel's answer)
        if g_ce is None and ctx.n_classes:
            grad[:, :ctx.n_classes] = 0
        if g_fg is None and ctx.has_fg:
            grad[:, ctx.n_classes:] = 0
        return grad, None, None, None, None


class CrossEntropyLoss(nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, semseg_logits, targets, output_dict):
        """semseg_logits [N, T, cls, H, W] (the permuted view of the head's [N, cls, T, H, W] is read in place); targets: list of dicts
        with 'semseg_masks' [T, H, W] and 'ignore_masks' [T, H, W]; adds the reference's two entries to output_dict."""
        hip.require_gpu()
        loss, _ = SemsegLossFunction.apply(semseg_logits.permute(0, 2, 1, 3, 4), [t["semseg_masks"] for t in targets],
                                           [t["ignore_masks"] for t in targets], semseg_logits.shape[2], False)
        self._store(loss, output_dict)

    def forward_with_foreground(self, combined_logits, targets, output_dict):
        """combined_logits [N, T, cls + 1, H, W], the foreground channel last: the cross-entropy of the class channels and the
        foreground loss from one pass over the tensor (what the reference computes from its two slices)."""
        hip.require_gpu()
        loss, fg = SemsegLossFunction.apply(combined_logits.permute(0, 2, 1, 3, 4), [t["semseg_masks"] for t in targets],
                                            [t["ignore_masks"] for t in targets], combined_logits.shape[2] - 1, True)
        output_dict[ModelOutputConsts.OPTIMIZATION_LOSSES][LossConsts.FOREGROUND] = fg
        self._store(loss, output_dict)

    @staticmethod
    def _store(loss, output_dict):
        output_dict[ModelOutputConsts.OTHERS][LossConsts.SEMSEG] = loss
        output_dict[ModelOutputConsts.OPTIMIZATION_LOSSES][LossConsts.SEMSEG] = loss * cfg.TRAINING.LOSSES.WEIGHT_SEMSEG


def foreground_loss(fg_logits, targets, output_dict):
    """``TrainingModel.compute_fg_loss`` on its own: fg_logits [N, T, H, W]."""
    hip.require_gpu()
    _, fg = SemsegLossFunction.apply(fg_logits.unsqueeze(1), [t["semseg_masks"] for t in targets], [t["ignore_masks"] for t in targets], 0, True)
    output_dict[ModelOutputConsts.OPTIMIZATION_LOSSES][LossConsts.FOREGROUND] = fg
