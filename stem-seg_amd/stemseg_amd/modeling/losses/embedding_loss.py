"""``EmbeddingLoss`` (modeling/losses/embedding_loss.py:10-185): the Lovasz hinge on per-instance Gaussian probability maps, the
bandwidth-smoothness term and the two seediness regressions, value and gradient with respect to the head output, on the device
(csrc/embedding_loss.hip).  Nothing else of training is here: no decoder or encoder backward, no optimiser."""
import torch
import torch.nn as nn

from ... import hip
from ...utils.constants import Loss as LossConsts, ModelOutput as ModelOutputConsts


class EmbeddingLossFunction(torch.autograd.Function):
    """(embedding_map [N,C,T,H,W], masks list, ignore_masks list, embedding_size, free_dim_bandwidths) -> (lovasz, smoothness,
    seediness), three fp32 scalars already divided as the reference divides them.  ``backward`` hands the three upstream gradients to
    one backward call per sample, which writes that sample's slice of the input gradient."""

    @staticmethod
    def forward(ctx, embedding_map, masks, ignore_masks, embedding_size, free_dim_bandwidths):
        assert embedding_map.dtype == torch.float32 and embedding_map.dim() == 5
        x = embedding_map.detach().contiguous()
        N, _, T, H, W = x.shape
        dev = x.device
        samples, outs, total = [], [], 0
        with torch.cuda.device(dev):
            for n in range(N):
                m = masks[n]
                if m.numel() == 0:                             # (embedding_loss.py:65-66)
                    continue
                ig = ignore_masks[n]
                assert m.shape[-2:] == ig.shape[-2:], "Masks tensor has shape {} while ignore mask has shape {}".format(m.shape, ig.shape)
                assert tuple(m.shape[1:]) == (T, H, W), "Masks tensor has shape {} while embedding map has shape {}".format(m.shape, x.shape)
                m, ig = m.to(dev), ig.to(dev)
                desc = hip.embedding_loss_desc(embedding_size, free_dim_bandwidths, m.shape[0], T, H, W)
                out, K, _, ws = hip.embedding_loss_forward(desc, x[n], m, ig)
                if K == 0:
                    print("[ WARN] No valid mask points exist in sample.")
                    continue
                total += K
                outs.append(out)
                samples.append((n, desc, m, ig, ws))
        ctx.samples, ctx.total = samples, total
        ctx.save_for_backward(x)
        if total == 0:
            print("Zero instances case occurred embedding loss")
            z = torch.zeros(3, dtype=torch.float32, device=dev)
            return z[0], z[1], z[2]
        s = torch.stack(outs).sum(0)                           # fp64 [4]: three scalars per sample, combined as the reference does
        div = torch.tensor([float(total), float(N), float(total + 1)], dtype=torch.float64, device=dev)
        r = (s[:3] / div).float()
        return r[0], r[1], r[2]

    @staticmethod
    def backward(ctx, g_lovasz, g_smooth, g_seed):
        x, = ctx.saved_tensors
        grad = torch.zeros_like(x)
        if ctx.total > 0:
            up = torch.stack([torch.zeros((), device=x.device) if g is None else g.detach().float().reshape(()) for g in (g_lovasz, g_smooth, g_seed)])
            with torch.cuda.device(x.device):
                for n, desc, m, ig, ws in ctx.samples:
                    hip.embedding_loss_backward(desc, x[n], m, ig, ws, up.contiguous(), ctx.total, x.shape[0], grad[n])
        return grad, None, None, None, None


class EmbeddingLoss(nn.Module):
    """Constructor keys (any case), attributes and assertions of the reference's EmbeddingLoss (embedding_loss.py:11-33)."""

    def __init__(self, embedding_map_scale, **kwargs):
        super().__init__()
        kw = {k.lower(): v for k, v in kwargs.items()}
        self.embedding_map_scale = embedding_map_scale
        self.embedding_size, self.n_free_dims = kw["embedding_size"], kw["nbr_free_dims"]
        self.w_lovasz, self.w_variance_smoothness, self.w_seediness = kw["weight_lovasz"], kw["weight_variance_smoothness"], kw["weight_seediness"]
        self.w_regularization, self.w = kw["weight_regularization"], kw["weight"]
        stds = kw["free_dim_stds"]
        assert len(stds) == self.n_free_dims, "List of std values {} does not match number of free dims {}".format(len(stds), self.n_free_dims)
        if self.n_free_dims > 0:                               # [1, n_free_dims], 1 / std^2 in fp32 as the reference's buffer
            self.register_buffer("free_dim_bandwidths", 1. / torch.tensor(stds).float().unsqueeze(0) ** 2)
        self.split_sizes = (self.embedding_size, self.embedding_size - self.n_free_dims, 1)
        self.num_input_channels = sum(self.split_sizes)
        self._free_bw = self.free_dim_bandwidths[0].tolist() if self.n_free_dims > 0 else []

    def forward(self, embedding_map, targets, output_dict, *args, **kwargs):
        """embedding_map [N, C, T, H, W] (C = embedding + variance + seediness channels); targets: list (length N) of dicts with
        'masks' [I, T, H, W] and 'ignore_masks' [T, H, W]; fills output_dict as the reference does (embedding_loss.py:144-157)."""
        assert embedding_map.shape[1] == self.num_input_channels, "Expected {} channels in input tensor, got {}".format(
            self.num_input_channels, embedding_map.shape[1])
        hip.require_gpu()
        lovasz, smoothness, seediness = EmbeddingLossFunction.apply(
            embedding_map, [t["masks"] for t in targets], [t["ignore_masks"] for t in targets], self.embedding_size, self._free_bw)
        total = lovasz * self.w_lovasz + smoothness * self.w_variance_smoothness + seediness * self.w_seediness
        output_dict[ModelOutputConsts.OPTIMIZATION_LOSSES] = {LossConsts.EMBEDDING: total * self.w}
        output_dict[ModelOutputConsts.OTHERS] = {LossConsts.LOVASZ_LOSS: lovasz, LossConsts.VARIANCE_SMOOTHNESS: smoothness,
                                                 LossConsts.SEEDINESS_LOSS: seediness}
