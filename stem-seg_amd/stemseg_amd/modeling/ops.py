"""The differentiable ops of the decoders: the 3x3x3 convolution, GroupNorm -> ReLU -> (pool), the trilinear up-sampling and the 1x1x1
heads, each a ``torch.autograd.Function`` with its forward on the inference kernel and its backward on csrc/conv_backward.hip and
csrc/decoder_backward.hip.  One sample per call ([C, T, H, W] tensors), fp32, on the device; there is no other implementation behind
them.  ``EncoderFunction`` is the encoder over one pass of frames: the forward is the encoder pass itself, the backward the FPN's
(csrc/conv_backward.hip) and, with a ``freeze_at``, the body's stages freeze_at .. 4 behind it (csrc/bottleneck_backward.hip)."""
import torch

from .. import hip
from . import encoder_backward


def _f32(t):
    return t.detach().contiguous().float()


class Conv3dFunction(torch.autograd.Function):
    """(x [Cin, T, H, W], weight [Cout, Cin, 3, 3, 3], bias [Cout] | None, packed_w, precision, gn_groups, eps) -> (D [Cout, T, H, W],
    GroupNorm statistics of D [2 gn_groups] | None): Conv3d(3, padding=1) on the inference kernel with the caller's packing of ``weight``
    for ``precision``.  The statistics ride along as ``GnReluPoolFunction`` expects them and carry no gradient (that Function's x
    gradient accounts for them).  Gradients: weight and bias from csrc/conv_backward.hip on the saved zero-haloed input; x -- only when
    asked for -- from ``hip.conv3d_dgrad`` (the forward 1x1x1 kernel on the per-tap weights, the taps summed in fp64).  The backward never runs in 'f16x3' (gradients have no
    bounded magnitude): the data gradient is 'f32' for an 'f32' forward and 'bf16x6' otherwise.  An optional eighth argument is a split-K
    scratch tensor for the forward kernel, an optional ninth the decoder's ``plan_clips``: with the inference decoder's scratch size and
    planning clip count the kernel takes the inference decoder's K partition, so D has the bits ``run_hip`` computes; an optional tenth the
    ``tile_cfg`` of the launch (the decoder's block_4x stage passes ``hip.TILE_CFG_DEEP``, as the inference decoder does)."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed_w, precision, gn_groups, eps, *splitk_scratch):
        x = _f32(x)
        Cin, T, H, W = x.shape
        Cout = weight.shape[0]
        with torch.cuda.device(x.device):
            buf, g = hip.alloc_padded(Cin, T, H, W, device=x.device)
            hip.copy_to_volume(x, 0, hip.padded_interior_view(buf, g, Cin, T, H, W))
            D = torch.empty(Cout, T, H, W, dtype=torch.float32, device=x.device)
            stats = hip.conv3d_zero_t_halo(hip.padded_halo_view(buf, g, Cin, T, H, W), packed_w, None if bias is None else _f32(bias),
                                           hip.dense_volume(D), 3, splitk_scratch=splitk_scratch[0] if splitk_scratch else None,
                                           precision=precision, gn_groups=gn_groups, eps=eps, plan_clips=int(splitk_scratch[1]) if len(splitk_scratch) > 1 else 0,
                                           tile_cfg=int(splitk_scratch[2]) if len(splitk_scratch) > 2 else 0)
        ctx.n_extra = len(splitk_scratch)
        ctx.save_for_backward(buf, weight)
        ctx.geom = (g, Cin, T, H, W)
        ctx.has_bias = bias is not None
        ctx.dgrad_precision = "f32" if precision == "f32" else "bf16x6"
        if stats is None:
            return D, None
        ctx.mark_non_differentiable(stats)
        return D, stats

    @staticmethod
    def backward(ctx, dD, _dstats=None):
        buf, weight = ctx.saved_tensors
        g, Cin, T, H, W = ctx.geom
        dx = dw = db = None
        with torch.cuda.device(buf.device):
            dy = _f32(dD)
            if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
                dw, db = hip.conv3d_wgrad(hip.padded_halo_view(buf, g, Cin, T, H, W), dy, want_db=ctx.has_bias and ctx.needs_input_grad[2])
            if ctx.needs_input_grad[0]:
                dx = hip.conv3d_dgrad(dy, weight, ctx.dgrad_precision)
        return (dx, dw if ctx.needs_input_grad[1] else None, db, None, None, None, None) + (None,) * ctx.n_extra


class GnReluPoolFunction(torch.autograd.Function):
    """(x [C, T, H, W] conv output, stats [2 groups] (mean, rstd), gamma [C], beta [C], groups, pool) -> relu(GroupNorm(x)), average-pooled
    over (3, 3, 3) windows with stride (2, 1, 1) when ``pool`` is 1: [C, To, H, W].  ``groups`` 0 is NORMALIZATION_LAYER 'none' (gamma,
    beta, stats None).  Gradients: x, gamma, beta -- the statistics are a function of x and the x gradient accounts for them."""

    @staticmethod
    def forward(ctx, x, stats, gamma, beta, groups, pool):
        if pool not in (0, 1):
            raise NotImplementedError("POOL_TYPE 'max' (pool code %r): the max pool has no backward kernel; every shipped config uses 'avg'" % (pool,))
        x = _f32(x)
        Cn, T, H, W = x.shape
        with torch.cuda.device(x.device):
            if groups:
                st, ga, be = _f32(stats), _f32(gamma), _f32(beta)
            else:                                            # mean 0, rstd 1, scale 1, shift 0: the apply kernel computes fma(x, 1, 0)
                st = torch.tensor([0.0, 1.0], dtype=torch.float32, device=x.device)
                ga, be = torch.ones(Cn, dtype=torch.float32, device=x.device), torch.zeros(Cn, dtype=torch.float32, device=x.device)
            out = torch.empty(Cn, (T + 1) // 2 if pool else T, H, W, dtype=torch.float32, device=x.device)
            hip.gn_relu_pool(x, groups or 1, st, ga, be, pool, hip.dense_volume(out))
        ctx.save_for_backward(x, st, ga, be)
        ctx.groups, ctx.pool = groups, pool
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, st, ga, be = ctx.saved_tensors
        with torch.cuda.device(x.device):
            dx, dgamma, dbeta = hip.gn_relu_pool_backward(x, ctx.groups, st, ga, be, ctx.pool, _f32(d_out))
        return dx, None, dgamma, dbeta, None, None


class UpsampleTrilinearFunction(torch.autograd.Function):
    """x [C, T, H, W] -> [C, T st, H sy, W sx] (align_corners=False); the backward is the exact adjoint (st 1 | 2, sy = sx 2 | 4)."""

    @staticmethod
    def forward(ctx, x, st, sy, sx):
        ctx.scale = (int(st), int(sy), int(sx))
        x = _f32(x)
        with torch.cuda.device(x.device):
            return hip.upsample_trilinear(x, *ctx.scale)

    @staticmethod
    def backward(ctx, d_out):
        with torch.cuda.device(d_out.device):
            return hip.upsample_trilinear_backward(_f32(d_out), *ctx.scale), None, None, None


class HeadsFunction(torch.autograd.Function):
    """(x [Cin, T, H, W], w [n_out, Cin], bias [n_out] | None, act, grid_axis, grids) -> [n_out, T, H, W].

    ``act`` a list of activation codes (with ``grid_axis`` and ``grids`` = (gt, gy, gx) | None): the fused heads, act_o(w x + bias);
    W % 4 == 0.  ``act`` None: one level matrix of the folded linear tail, w x, any shape -- the activation then sits behind the sum of
    the levels and the caller applies it.  Gradients: x (only when asked for), w, bias.

    A wide head, hip.MAX_HEAD_OUT < n_out <= hip.MAX_WIDE_HEAD_OUT (the 42-channel YouTube-VIS semseg head), is linear only: ``act`` None,
    or all codes 0 with no grid, and no bias (the caller adds it, as the folded tail does); it runs ``hip.wide_level_head`` /
    ``hip.wide_heads_backward``.  Anything wider, or a wide head with an activation, is refused."""

    @staticmethod
    def forward(ctx, x, w, bias, act, grid_axis, grids):
        x, w = _f32(x), _f32(w)
        n_out = w.shape[0]
        if n_out > hip.MAX_WIDE_HEAD_OUT:
            raise NotImplementedError("heads with %d output channels: the backward kernels serve at most %d (fused heads, with activations) "
                                      "and %d (wide linear heads)" % (n_out, hip.MAX_HEAD_OUT, hip.MAX_WIDE_HEAD_OUT))
        ctx.wide = n_out > hip.MAX_HEAD_OUT
        if ctx.wide:
            if act is not None and (any(act) or any(grid_axis or ()) or grids is not None):
                raise NotImplementedError("a wide head (%d output channels, more than %d) with an activation or a grid: the wide heads' kernels "
                                          "are linear (raw class logits)" % (n_out, hip.MAX_HEAD_OUT))
            if bias is not None:
                raise NotImplementedError("a wide head (%d output channels) with a bias: the wide heads' kernels are w x; the caller adds the bias, "
                                          "as the folded tail does" % n_out)
            with torch.cuda.device(x.device):
                out = hip.wide_level_head(x, w)
            ctx.save_for_backward(x, w)
            return out
        gt, gy, gx = grids if grids is not None else (None, None, None)
        with torch.cuda.device(x.device):
            if act is None:
                assert bias is None, "a level matrix of the folded tail has no bias"
                out = hip.level_head(x, w)
            else:
                out = hip.heads(x, w, None if bias is None else _f32(bias), list(act), list(grid_axis), gt, gy, gx)
        ctx.save_for_backward(x, w, out)
        ctx.spec = (None if act is None else list(act), None if act is None else list(grid_axis), gt, gy, gx, bias is not None)
        return out

    @staticmethod
    def backward(ctx, d_out):
        if ctx.wide:
            x, w = ctx.saved_tensors
            with torch.cuda.device(x.device):
                dx, dw, _ = hip.wide_heads_backward(x, w, _f32(d_out), want_dx=ctx.needs_input_grad[0], want_db=False)
            return dx, dw, None, None, None, None
        x, w, out = ctx.saved_tensors
        act, axis, gt, gy, gx, has_bias = ctx.spec
        with torch.cuda.device(x.device):
            dx, dw, db = hip.heads_backward(x, w, _f32(d_out), out if act is not None else None, act, axis, gt, gy, gx,
                                            want_dx=ctx.needs_input_grad[0], want_db=has_bias)
        return dx, dw, db, None, None, None


class EncoderFunction(torch.autograd.Function):
    """(backbone, frames [F, 3, H, W], freeze_at, *params) -> the four FPN maps [256, F, h, w] (4x .. 32x) of
    ``backbone.forward_channel_major(frames)``: the very same encoder pass, so the same bits.  ``freeze_at`` None: the FPN alone; ``params`` is
    the sixteen FPN tensors in ``ResNetFPN.fpn_parameter_list`` order, and the frames and the body get no gradient (nor is the body asked
    whether it could: a ResNeXt backbone trains its FPN too).  Otherwise ``params`` is the convolution weights of layer{freeze_at} .. layer4 in
    ``ResNetFPN.body_parameter_list`` order, then the sixteen; the frames, the stem and the stages below ``freeze_at`` get none.
    Gradients: the FPN's sixteen from ``encoder_backward.fpn_backward`` on the stage outputs and merged laterals the pass left in its workspace
    -- with a body it also returns dC_k, the gradient of the stage outputs; the body's from ``encoder_backward.body_backward``, which recomputes
    one stage at a time from those stage outputs (with the pass's packed weights, precision and plan_frames) and joins dC_k on the way down.
    The FPN's data gradient is 'f32' for an 'f32' pass and 'bf16x6' otherwise, never 'f16x3'; the body's are 'f32' arithmetic in every pass
    precision.  ``freeze_at`` 1 or 0 (``backbone.train_stem``): layer1, and with 0 ``stem.conv1.weight`` in front of it, join the body's list;
    their backward recomputes the stem and the pooled map from the frames (``ResNetFPN.stem_forward``).  The workspace is shared by every pass
    of the same shape on the same lane: if another one has run since the forward, the backward refuses (it would read that pass's maps)."""

    @staticmethod
    def forward(ctx, backbone, frames, freeze_at, *params):
        n_body = 0 if freeze_at is None else len(backbone.body_parameter_list(freeze_at))
        assert len(params) == n_body + 16, "the body weights of ResNetFPN.body_parameter_list(freeze_at), then the sixteen of fpn_parameter_list()"
        with torch.cuda.device(frames.device):
            outs = backbone.forward_channel_major(frames)
        ctx.backbone, ctx.key, ctx.freeze_at, ctx.n_body = backbone, backbone.workspace_key(frames), freeze_at, n_body
        ctx.passes = backbone._ws_passes[ctx.key]
        ctx.precision, ctx.plan_frames = backbone.precision, int(backbone.plan_frames)
        ctx.names = backbone._packed_names[backbone.precision]          # the packed weights of THIS pass
        ctx.shapes = [tuple(o.shape) for o in outs]
        fpn = params[n_body:]
        ctx.save_for_backward(*(fpn[8:12] + (fpn[0:4] if freeze_at is not None else ()) + ((frames,) if freeze_at is not None and freeze_at < 2 else ())))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *d_outs):
        bb, fa = ctx.backbone, ctx.freeze_at
        c_views, l_views, passes = bb.fpn_workspace_views(ctx.key)
        if passes != ctx.passes:
            raise RuntimeError("EncoderFunction.backward: %d more encoder passes have run on the workspace %r (frames, height, width, device, lane, "
                               "windows, plan_frames) since this graph's forward, so it no longer holds the stage outputs and laterals the backward "
                               "needs; give the training model a lane of its own (backbone.lane) or run backward() before the next pass of this shape"
                               % (passes - ctx.passes, ctx.key))
        layer_w = [_f32(w) for w in ctx.saved_tensors[:4]]
        dev = layer_w[0].device
        dprec = "f32" if ctx.precision == "f32" else "bf16x6"
        body = []
        with torch.cuda.device(dev):
            d = [_f32(g) if g is not None else torch.zeros(s, dtype=torch.float32, device=dev) for g, s in zip(d_outs, ctx.shapes)]
            if fa is None:
                d_layer_w, d_layer_b, d_inner_w, d_inner_b = encoder_backward.fpn_backward(c_views, l_views, d, layer_w, dprec)
            else:
                frames = ctx.saved_tensors[8] if fa < 2 else None
                lo = max(fa, 1)                                      # the lowest stage of bottleneck blocks with a gradient
                d_layer_w, d_layer_b, d_inner_w, d_inner_b, dC = encoder_backward.fpn_backward(
                    c_views, l_views, d, layer_w, dprec, want_dC=range(lo - 1, 4), inner_weights=[_f32(w) for w in ctx.saved_tensors[4:8]])
                inputs = bb.body_stage_inputs(ctx.key, fa, frames, ctx.precision)
                stem = None
                if fa < 2:
                    stem = dict(frames=frames, stem_map=inputs.pop(0), bn_scale=bb.body.stem.bn1.scale_shift()[0].detach().float().contiguous().to(dev))
                grads = encoder_backward.body_backward(inputs, bb.body_stage_specs(fa, ctx.names), {st: dC[st - 1] for st in range(lo, 5)}, ctx.precision,
                                                       fa, ctx.plan_frames, stem=stem)
                body = [grads[0]] if fa == 0 else []
                for st in range(lo, 5):
                    for g in grads[st]:
                        body += ([g["down"]] if g["down"] is not None else []) + [g["conv1"], g["conv2"], g["conv3"]]
        assert len(body) == ctx.n_body
        return (None, None, None) + tuple(body) + tuple(d_inner_w) + tuple(d_inner_b) + tuple(d_layer_w) + tuple(d_layer_b)
