"""Shared machinery of the two squeeze-expand decoders: reference-compatible parameter containers
(state-dict keys of SURVEY.md section 5) + the call into ``stemseg_hip_decoder_forward``.

The ``nn.Conv3d`` / ``nn.GroupNorm`` objects created here are *parameter holders only* -- they give
checkpoints the reference's key names (``block_32x.0.weight`` ... ``conv_4.weight``); ``forward`` never
calls them.  All arithmetic happens in libstemseg_hip.so.
"""
import ctypes as C

import torch
import torch.nn as nn

from .. import hip
from ..config import cfg
from .common import POOL_TABLE, TSCALE_TABLE

_BLOCK_CONVS = (("block_32x", 0), ("block_32x", 4), ("block_32x", 8), ("block_16x", 0), ("block_16x", 4),
                ("block_8x", 0), ("block_4x", 0))


def _stage(cin, cout, NormType, pool_creator):
    # Conv3d(3, p=1) -> Norm -> ReLU -> Pool|Identity   (indices 0,1,2,3 within the block)
    return [nn.Conv3d(cin, cout, 3, stride=1, padding=1), NormType(cout), nn.ReLU(inplace=True),
            pool_creator(3, stride=(2, 1, 1), padding=1) if pool_creator else None]


class SqueezeExpandTrunk(nn.Module):
    """Parameter layout + HIP execution shared by embedding_decoder / seediness_decoder."""

    def __init__(self, in_channels, inter_channels, PoolType=nn.AvgPool3d, NormType=nn.Identity, num_frames=None):
        super().__init__()
        assert len(inter_channels) == 4
        self.num_frames = cfg.INPUT.NUM_FRAMES if num_frames is None else num_frames
        if self.num_frames not in POOL_TABLE:
            raise NotImplementedError("clip length %r" % (self.num_frames,))
        if PoolType not in (nn.AvgPool3d, nn.MaxPool3d):      # the two entries of POOL_TYPE (model_builder.py:29-33)
            raise NotImplementedError("HIP decoder implements POOL_TYPE 'avg' (AvgPool3d) and 'max' (MaxPool3d)")
        self.pool_code = 2 if PoolType is nn.MaxPool3d else 1
        self.pool_flags, self.t_scales = POOL_TABLE[self.num_frames], TSCALE_TABLE[self.num_frames]
        probe = NormType(inter_channels[0])
        if isinstance(probe, nn.GroupNorm):
            self.gn_groups, self.gn_eps = probe.num_groups, probe.eps
        elif isinstance(probe, nn.Identity):                 # NORMALIZATION_LAYER 'none'
            self.gn_groups, self.gn_eps = 0, 0.0
        else:
            raise NotImplementedError("HIP decoder implements NORMALIZATION_LAYER 'gn' (GroupNorm) and 'none' (Identity)")
        self.in_channels, self.inter_channels = in_channels, list(inter_channels)

        def pools(n):
            return [(PoolType if on else (lambda *a, **k: nn.Identity())) for on in self.pool_flags[:n]]
        c32, c16, c8, c4 = inter_channels

        def block(cins, cout, poolers):
            mods = []
            for ci, pc in zip(cins, poolers):
                mods += [m for m in _stage(ci, cout, NormType, pc) if m is not None]
            return nn.Sequential(*mods)
        self.block_32x = block([in_channels, c32, c32], c32, pools(3))
        self.block_16x = block([in_channels, c16], c16, pools(2))
        self.block_8x = block([in_channels], c8, pools(1))
        self.block_4x = nn.Sequential(*[m for m in _stage(in_channels, c4, NormType, None) if m is not None])
        self.conv_16 = nn.Conv3d(c32 + c16, c16, 1, bias=False)
        self.conv_8 = nn.Conv3d(c16 + c8, c8, 1, bias=False)
        self.conv_4 = nn.Conv3d(c8 + c4, c4, 1, bias=False)
        self._cache = {}          # precision -> packed weights (valid while the parameter versions match)
        self.fold_conv4 = True    # conv_4 folded into the heads at load (see _fold; False: the two-step form, for A/B and exactness checks)
        self.fold_linear_tail = True     # the whole linear tail folded into per-level head matrices (see _linear_tail; narrow heads only)
        self._retired = []        # superseded packings, kept alive for captured graphs
        self._workspaces, self._ws_desc = {}, {}     # (T, H4, W4, layout, device, lane) -> workspace tensor / the descriptor it was sized for
        self.input_layout = 0     # 0: [C,T,h,w] per sample (reference API); 2: caller passes zero-haloed buffers
        self.concurrency = 1      # 0: single stream; k>=1: branch streams of the library's set k-1 (see stemseg_hip.h)
        self.detached = False     # True: the call does not join; ``join()`` must follow (twin-decoder overlap)
        self.precision = hip.DEFAULT_PRECISION    # hip.PRECISIONS: "f16x3" | "bf16x6" | "f32"
        self.lane = 0             # selects one of several independent workspaces (one per in-flight step / stream)
        # Clips every convolution's split-K factor is PLANNED for (StemsegDecoderDesc.plan_clips), the counterpart of ResNetFPN.plan_frames =
        # 32 (4 clips x 8 frames): a constant of the model, never the clip count of the call, so a clip's maps are the same bits alone and
        # in any batch.  0 / 1: planned on one clip (every small-map stage of a 4-clip step then splits 2 .. 16 ways for nothing).
        self.plan_clips = 4
        # block_4x, the decoder's largest launch, asks for the deep 3x3x3 tile (StemsegDecoderDesc.reserved = 0: eight planes of an 8 x 8 patch per
        # workgroup, every input plane staged once; f16x3 and 8-frame clips, anything else runs as before).  False restores the automatic choice
        # for A/B runs: the same convolution output, the stage's GroupNorm statistics in another summation order.
        self.deep_block4x = True
        self.train_wide_head = False     # opt-in (TrainingModel.train_wide_head): the trainable paths take a wide linear head (11 .. 64 channels) in the folded form

    @staticmethod
    def _narrow_head(n_out):
        """The one rule for where an n_out-channel head runs (the library's STEMSEG_MAX_HEAD_OUT): True -> the fused heads kernel, with
        an activation / grid table per channel and the linear tail foldable into per-level matrices; False -> the 1x1x1 MFMA conv on
        output channels zero-padded to a multiple of 32 (wide linear heads, no activation).  n_out is the logical width or, for a
        packed wide head, the padded one: both lie on the same side."""
        return n_out <= hip.MAX_HEAD_OUT

    # ---- to be provided by the concrete decoder ---------------------------------------------------
    def _head_spec(self):
        """-> (weight [n_out, c4] tensor, bias [n_out] tensor, act codes, grid_axis codes)"""
        raise NotImplementedError

    def _linear_tail(self, w_head):
        """Between the last GroupNorm + ReLU of every branch and the heads' activations the reference applies only linear maps (trilinear
        up-sampling, concatenation, the bias-free 1x1x1 convs conv_16 / conv_8 / conv_4, the 1x1x1 heads; embedding_decoder.py:64-80,112-143), and
        channel mixing commutes with up-sampling:  heads(x) = up(up(up(M32 x32) + M16 y16) + M8 y8) + M4 y4.  -> the four level matrices
        [n_out, c32], [n_out, c16], [n_out, c8], [n_out, c4] as fp64 products rounded once (StemsegDecoderWeights: fuse_w[0..2] = NULL,
        head_w = [M32 | M16 | M8 | M4])."""
        return [m.detach().contiguous() for m in self._tail_matrices(w_head.detach(), detach=True)]

    def _tail_matrices(self, w_head, detach=False):
        """The products of ``_linear_tail``; with ``detach`` False on the live parameters, so that autograd carries the gradients of the four
        matrices back to the head weights and conv_16 / conv_8 / conv_4 (``_linear_tail_trainable``).  Same operations either way: the values
        are the same bits."""
        c32, c16, c8, c4 = self.inter_channels
        par = (lambda p: p.detach()) if detach else (lambda p: p)
        wh = w_head.double()
        w4 = par(self.conv_4.weight).reshape(c4, c8 + c4).double()
        w8 = par(self.conv_8.weight).reshape(c8, c16 + c8).double()
        w16 = par(self.conv_16.weight).reshape(c16, c32 + c16).double()
        m4 = wh @ w4[:, c8:]
        a = wh @ w4[:, :c8]
        m8 = a @ w8[:, c16:]
        b = a @ w8[:, :c16]
        m16 = b @ w16[:, c32:]
        m32 = b @ w16[:, :c32]
        return [m.float() for m in (m32, m16, m8, m4)]

    def _linear_tail_trainable(self, w_head):
        """The differentiable twin of ``_linear_tail``: plain torch, fp64 products, rounded once."""
        return self._tail_matrices(w_head, detach=False)

    def _fold(self, w_head):
        """conv_4 (1x1x1, no bias, no activation: embedding_decoder.py:80,129) feeds nothing but the 1x1x1 heads: with ``fold_conv4`` the head
        weights are multiplied by conv_4's at load (fp64 product, rounded once) and the decoder applies them to the last concat buffer directly
        (StemsegDecoderWeights.fuse_w[2] = NULL) -- one linear map for two, like FrozenBN folded into its convolution; the inter[3]-channel
        map is never computed, written or read.  w_head: dense [n_out, inter[3]] -> [n_out, inter[2] + inter[3]] (unchanged without the fold)."""
        if self.fold_linear_tail and self._narrow_head(w_head.shape[0]):
            return torch.cat([m.reshape(-1) for m in self._linear_tail(w_head)])      # (flat [M32 | M16 | M8 | M4]: the narrow heads' form)
        if not self.fold_conv4:
            return w_head
        w4 = self.conv_4.weight.detach().reshape(self.conv_4.out_channels, -1)
        return (w_head.detach().double() @ w4.double()).float()

    # ---- weights --------------------------------------------------------------------------------------
    def _param_signature(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters()) + (bool(self.fold_conv4), bool(self.fold_linear_tail))

    def _packed(self):
        # one packing per precision: an overflow re-run in bf16x6 (ClipPipeline.step_checked, GraphedStep.collect) must not throw the
        # f16x3 packing away and pack it again on the way back.  A packing superseded by a parameter update is RETIRED, not freed: a
        # captured hipGraph holds raw pointers into it (a replay then computes with the old weights -- re-capture after an update -- but
        # never reads freed memory)
        sig = self._param_signature()
        c = self._cache.setdefault(self.precision, {})
        if c.get("sig") != sig:
            dev = next(self.parameters()).device
            conv_w, conv_b, gn_w, gn_b = [], [], [], []
            for blk, idx in _BLOCK_CONVS:
                conv, gn = getattr(self, blk)[idx], getattr(self, blk)[idx + 1]
                conv_w.append(hip.pack_conv_weight_any(conv.weight.detach().float(), self.precision))
                conv_b.append(conv.bias.detach().float().contiguous())
                if self.gn_groups:
                    gn_w.append(gn.weight.detach().float().contiguous())
                    gn_b.append(gn.bias.detach().float().contiguous())
                else:                                        # no normalisation layer: scale 1, shift 0
                    gn_w.append(torch.ones(conv.out_channels, dtype=torch.float32, device=dev))
                    gn_b.append(torch.zeros(conv.out_channels, dtype=torch.float32, device=dev))
            hw, hb, act, axes = self._head_spec()
            lin = self.fold_linear_tail and self._narrow_head(len(act))          # (the wide semseg head keeps conv_16 / conv_8 and folds conv_4 only)
            fuse = [None if lin else hip.pack_conv_weight_any(m.weight.detach().float(), self.precision) for m in (self.conv_16, self.conv_8)]
            fuse.append(None if (lin or self.fold_conv4) else hip.pack_conv_weight_any(self.conv_4.weight.detach().float(), self.precision))
            if c:
                self._retired.append(dict(c))
            c.clear()
            c.update(sig=sig, conv_w=conv_w, conv_b=conv_b, gn_w=gn_w, gn_b=gn_b, fuse=fuse,
                     head_w=hw.detach().float().contiguous().to(dev), head_b=hb.detach().float().contiguous().to(dev),
                     act=list(act), axes=list(axes), grids={})
        return c

    def _desc(self, T, H4, W4, layout, act):
        d = hip.DecoderDesc()
        d.struct_bytes = C.sizeof(hip.DecoderDesc)
        d.in_channels = self.in_channels
        for i in range(4):
            d.inter[i] = self.inter_channels[i]
        d.T, d.H4, d.W4 = T, H4, W4
        d.gn_groups, d.gn_eps = self.gn_groups, self.gn_eps
        for i in range(3):
            d.pool[i], d.t_scale[i] = self.pool_flags[i] * self.pool_code, self.t_scales[i]
        d.n_out = len(act)
        d.plan_clips = int(self.plan_clips)
        d.reserved = 0 if self.deep_block4x else 1
        return d

    def _grid(self, c, T, H4, W4, dev):
        return None, None, None

    def check_workspaces(self):
        """Debug check (synchronises): clobbered guard words over all cached workspaces (stemseg_hip_decoder_check_workspace)."""
        bad, where = 0, []
        for key, ws in self._workspaces.items():
            n, first = C.c_int32(0), C.c_int64(-1)
            with torch.cuda.device(ws.device):
                hip.check(hip.lib().stemseg_hip_decoder_check_workspace(C.byref(self._ws_desc[key]), hip.ptr(ws), ws.numel(), C.byref(n), C.byref(first), hip.stream()))
            if n.value:
                bad += n.value
                where.append((key, first.value))
        return bad, where

    def join(self):
        """Make the current stream wait for a detached forward of this decoder."""
        hip.check(hip.lib().stemseg_hip_decoder_join(int(self.concurrency), hip.stream()))

    @torch.no_grad()
    def run_hip(self, feats, input_layout=None, act_override=None, clip_batch=None):
        """feats: 4 device tensors (32x,16x,8x,4x) for ONE sample: dense [C,T,h,w] (layout 0), dense [T,C,h,w]
        (layout 1) or zero-haloed flat buffers (layout 2, then T/H4/W4 must be given via ``feats_shape``).
        Returns [n_out, T, H4, W4].
        ``clip_batch = (n, strides)``: layout 2 only -- ``feats`` are clip 0's buffers and clip c's lie ``strides[level] * c`` floats
        further (hip.alloc_padded_batch); all n clips go through ONE launch per decoder stage (StemsegDecoderDesc.n_clips) and the
        result is [n, n_out, T, H4, W4].  A clip's output is bit-identical to its single-clip call."""
        hip.require_gpu()
        layout = self.input_layout if input_layout is None else input_layout
        nb = 1
        if clip_batch is not None:
            nb, bstrides = int(clip_batch[0]), [int(v) for v in clip_batch[1]]
            if layout != 2 or nb < 1 or len(bstrides) != 4:
                raise ValueError("clip_batch needs zero-haloed inputs (layout 2) and one stride per level")
        if layout == 2:
            bufs, (T, H4, W4) = feats
        else:
            bufs = [f.contiguous().float() for f in feats]
            f4 = bufs[3]
            T, H4, W4 = (f4.shape[1], f4.shape[2], f4.shape[3]) if layout == 0 else (f4.shape[0], f4.shape[2], f4.shape[3])
        if T != self.num_frames:
            raise ValueError("decoder built for %d-frame clips, got %d" % (self.num_frames, T))
        dev = bufs[0].device
        c = self._packed()
        act = list(c["act"]) if act_override is None else list(act_override)
        d = self._desc(T, H4, W4, layout, act)
        for o in range(d.n_out if self._narrow_head(d.n_out) else 0):     # wide linear heads (n_out % 32 == 0) carry no activation table
            d.act[o], d.grid_axis[o] = act[o], c["axes"][o]
        d.input_layout = layout
        d.concurrency = int(self.concurrency)
        d.detached = int(bool(self.detached) and self.concurrency >= 1)
        d.precision = hip.PRECISIONS[self.precision]
        if nb > 1:
            d.n_clips = nb
            for i in range(4):
                d.feat_clip_stride[i] = bstrides[i]
        key = (T, H4, W4, layout, dev.index, self.lane, nb)      # (plan_clips moves no offset of the workspace)
        ws = self._workspaces.get(key)
        if ws is None:
            nbytes = hip.lib().stemseg_hip_decoder_workspace_bytes(C.byref(d))
            if nbytes == 0:
                raise RuntimeError("decoder: " + hip.lib().stemseg_hip_last_error().decode())
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            hip.check(hip.lib().stemseg_hip_decoder_init_workspace(C.byref(d), hip.ptr(ws), nbytes, hip.stream()))
            self._workspaces[key] = ws
            self._ws_desc[key] = d
        w = hip.DecoderWeights()
        for i in range(7):
            w.conv_w[i], w.conv_b[i] = c["conv_w"][i].data_ptr(), c["conv_b"][i].data_ptr()
            w.gn_w[i], w.gn_b[i] = c["gn_w"][i].data_ptr(), c["gn_b"][i].data_ptr()
        for i in range(3):
            w.fuse_w[i] = c["fuse"][i].data_ptr() if c["fuse"][i] is not None else None      # (conv_4 folded into the heads: NULL)
        w.head_w, w.head_b = c["head_w"].data_ptr(), c["head_b"].data_ptr()
        gt, gy, gx = self._grid(c, T, H4, W4, dev)
        if gt is not None:
            w.grid_t, w.grid_y, w.grid_x = gt.data_ptr(), gy.data_ptr(), gx.data_ptr()
        out = torch.empty((nb, d.n_out, T, H4, W4) if clip_batch is not None else (d.n_out, T, H4, W4), dtype=torch.float32, device=dev)
        fp = (C.c_void_p * 4)(*[b.data_ptr() for b in bufs])
        hip.check(hip.lib().stemseg_hip_decoder_forward(C.byref(d), C.byref(w), fp, hip.ptr(out), hip.ptr(ws), ws.numel(), hip.stream()))
        return out

    # ---- fine-tuning the tail -----------------------------------------------------------------------------
    # Behind the last 3x3x3 convolution of every branch the decoder applies GroupNorm -> ReLU -> (pool) and the linear tail; those are
    # differentiable here (modeling/ops.py on csrc/decoder_backward.hip); ``forward_tail_trainable`` stops there, ``forward_trainable`` goes on
    # through the seven 3x3x3 stages (csrc/conv_backward.hip).  Nothing before the decoder has a backward.
    _LAST_STAGE = (("block_32x", 8), ("block_16x", 4), ("block_8x", 0), ("block_4x", 0))
    _BRANCH_STAGES = ((0, 1, 2), (3, 4), (5,), (6,))          # indices into _BLOCK_CONVS, per input level (32x, 16x, 8x, 4x)

    def _head_convs(self):
        """The 1x1x1 convs whose outputs, concatenated, are the head's channels (the concrete decoder's)."""
        raise NotImplementedError

    def _trunk_order(self, x):
        return x

    def _train_acts(self):
        return None

    def tail_parameter_names(self):
        """State-dict keys (relative to this decoder) of the parameters ``forward_tail_trainable`` is differentiable in: the heads,
        conv_16 / conv_8 / conv_4 and the affine parameters of the last GroupNorm of each branch."""
        convs = self._head_convs()
        names = []
        for n, m in self.named_children():
            if any(m is c for c in convs):
                names += [n + ".weight"] + ([n + ".bias"] if m.bias is not None else [])
        names += ["conv_16.weight", "conv_8.weight", "conv_4.weight"]
        if self.gn_groups:
            for blk, idx in self._LAST_STAGE:
                names += ["%s.%d.weight" % (blk, idx + 1), "%s.%d.bias" % (blk, idx + 1)]
        return names

    def _check_tail_trainable(self):
        if self.pool_code == 2 and any(self.pool_flags):
            raise NotImplementedError("POOL_TYPE 'max': the max pool has no backward kernel (every shipped config uses 'avg')")
        n_out = sum(c.out_channels for c in self._head_convs())
        if self._narrow_head(n_out):
            return
        if not self.train_wide_head:
            raise NotImplementedError("a head of %d output channels (INPUT.NUM_CLASSES / conv_out.weight wider than %d): the heads' backward "
                                      "kernel serves the fused narrow heads only; the wide linear heads' kernels (up to %d channels) are "
                                      "behind the switch train_wide_head (TrainingModel.train_wide_head)"
                                      % (n_out, hip.MAX_HEAD_OUT, hip.MAX_WIDE_HEAD_OUT))
        if n_out > hip.MAX_WIDE_HEAD_OUT:
            raise NotImplementedError("a head of %d output channels (INPUT.NUM_CLASSES / conv_out.weight wider than %d): train_wide_head serves "
                                      "wide linear heads of at most %d channels" % (n_out, hip.MAX_WIDE_HEAD_OUT, hip.MAX_WIDE_HEAD_OUT))

    @torch.no_grad()
    def _last_conv_outputs(self, c, feats):
        """The seven 3x3x3 stages of one sample up to the LAST convolution of each branch: -> per branch (conv output dense [C, T', h, w],
        GroupNorm statistics | None, pool code of the stage).  The inference building blocks, one after the other."""
        outs = []
        flags = [f * self.pool_code for f in self.pool_flags]
        G = self.gn_groups
        for x, stages, pools in zip(feats, self._BRANCH_STAGES, (flags, flags[:2], flags[:1], [0])):
            cin, T, h, w = x.shape
            buf, g = hip.alloc_padded(cin, T, h, w, device=x.device)
            hip.copy_to_volume(x, 0, hip.padded_interior_view(buf, g, cin, T, h, w))
            for k, (si, pool) in enumerate(zip(stages, pools)):
                cout = c["conv_b"][si].numel()
                D = torch.empty(cout, T, h, w, dtype=torch.float32, device=x.device)
                stats = hip.conv3d_zero_t_halo(hip.padded_halo_view(buf, g, cin, T, h, w), c["conv_w"][si], c["conv_b"][si], hip.dense_volume(D), 3,
                                               precision=self.precision, gn_groups=G, eps=self.gn_eps)
                if k == len(stages) - 1:
                    outs.append((D, stats, pool))
                    break
                if stats is None:
                    stats = torch.tensor([0.0, 1.0], dtype=torch.float32, device=x.device)
                To = (T + 1) // 2 if pool else T
                buf, g = hip.alloc_padded(cout, To, h, w, device=x.device)
                hip.gn_relu_pool(D, G or 1, stats, c["gn_w"][si], c["gn_b"][si], pool, hip.padded_interior_view(buf, g, cout, To, h, w))
                cin, T = cout, To
        return outs

    def forward_tail_trainable(self, feats, act=None):
        """One sample, differentiable in ``tail_parameter_names()``: feats = 4 dense [C, T, h, w] device tensors (32x, 16x, 8x, 4x) ->
        [n_out, T, H4, W4], the function ``run_hip`` computes.  The 3x3x3 stages run without a graph; from the last conv output of
        each branch on, the folded form  act(up(up(up(M32 y32) + M16 y16) + M8 y8) + M4 y4 + b)  runs through the autograd Functions
        of modeling/ops.py, the four matrices through ``_linear_tail_trainable``.  ``self.tail_conv_outputs`` holds the four last conv
        outputs (32x .. 4x) as leaves: after ``backward()`` their ``.grad`` is where a convolution backward would start."""
        self._check_tail_trainable()
        hip.require_gpu()
        bufs = [f.detach().contiguous().float() for f in feats]
        T, H4, W4 = bufs[3].shape[1:]
        if T != self.num_frames:
            raise ValueError("decoder built for %d-frame clips, got %d" % (self.num_frames, T))
        dev = bufs[0].device
        with torch.cuda.device(dev):
            c = self._packed()
            return self.tail_from_conv_outputs(self._last_conv_outputs(c, bufs), act)

    def forward_trainable(self, feats, act=None):
        """The fully differentiable twin of ``forward_tail_trainable``: one sample, differentiable in EVERY parameter of the decoder.  The
        seven stages run as ``Conv3dFunction`` -> ``GnReluPoolFunction`` (weight and bias gradients from csrc/conv_backward.hip, the data
        gradient from ``hip.conv3d_dgrad``), then the folded tail as there.  A feature map that requires no gradient is a constant -- the
        backbone is frozen -- and the first stage of its branch computes no data gradient; one that does stays attached to its graph.  The convolutions get a split-K scratch of the size
        the inference decoder gives its branches (16, 4, 4, 2 output maps: csrc/decoder.hip) and its ``plan_clips``, so they take its K partition, and block_4x its tile request (``deep_block4x``)."""
        from .ops import Conv3dFunction, GnReluPoolFunction
        self._check_tail_trainable()
        hip.require_gpu()
        # (a map that requires a gradient -- the FPN's, with TrainingModel.train_fpn -- stays attached, and the first stage of its branch computes its data gradient)
        bufs = [f if (torch.is_grad_enabled() and f.requires_grad) else f.detach().contiguous().float() for f in feats]
        T = bufs[3].shape[1]
        if T != self.num_frames:
            raise ValueError("decoder built for %d-frame clips, got %d" % (self.num_frames, T))
        flags = [f * self.pool_code for f in self.pool_flags]
        with torch.cuda.device(bufs[0].device):
            c = self._packed()
            outs = []
            for x, stages, pools, slabs, cb in zip(bufs, self._BRANCH_STAGES, (flags, flags[:2], flags[:1], [0]), (16, 4, 4, 2), self.inter_channels):
                scratch = torch.empty(slabs * cb * T * x.shape[2] * x.shape[3], dtype=torch.float32, device=x.device)
                for k, (si, pool) in enumerate(zip(stages, pools)):
                    blk, idx = _BLOCK_CONVS[si]
                    conv, gn = getattr(self, blk)[idx], (getattr(self, blk)[idx + 1] if self.gn_groups else None)
                    D, stats = Conv3dFunction.apply(x, conv.weight, conv.bias, c["conv_w"][si], self.precision, self.gn_groups, self.gn_eps, scratch, int(self.plan_clips),
                                                      hip.TILE_CFG_DEEP if (si == 6 and self.deep_block4x) else 0)
                    if k == len(stages) - 1:
                        outs.append((D, stats, pool))
                    else:
                        x = GnReluPoolFunction.apply(D, stats, gn.weight if gn is not None else None, gn.bias if gn is not None else None,
                                                     self.gn_groups, pool)
            return self.tail_from_conv_outputs(outs, act, attached=True)

    def tail_from_conv_outputs(self, conv_outputs, act=None, attached=False):
        """The differentiable part of ``forward_tail_trainable`` on its own: conv_outputs = per branch (32x .. 4x) the triple (last conv
        output [C, T', h, w], its GroupNorm statistics | None, the pool code behind it) -> [n_out, T, H4, W4].  ``attached``: the conv
        outputs stay part of the graph they come from (``forward_trainable``) instead of becoming leaves."""
        from .ops import GnReluPoolFunction, HeadsFunction, UpsampleTrilinearFunction
        self._check_tail_trainable()
        T, H4, W4 = conv_outputs[3][0].shape[1:]
        dev = conv_outputs[3][0].device
        with torch.cuda.device(dev):
            c = self._packed()
            act = list(c["act"]) if act is None else list(act)
            axes = list(c["axes"])
            grids = self._grid(c, T, H4, W4, dev)
            convs = self._head_convs()
            c4 = self.inter_channels[3]
            w_head = torch.cat([m.weight.reshape(-1, c4) for m in convs], 0)
            bias = None
            if any(m.bias is not None for m in convs):
                bias = torch.cat([m.bias if m.bias is not None else torch.zeros(m.out_channels, device=dev) for m in convs], 0).float()
            mats = self._linear_tail_trainable(w_head)
            ys, leaves = [], []
            for (D, stats, pool), (blk, idx) in zip(conv_outputs, self._LAST_STAGE):
                if not attached:
                    D = D.detach().requires_grad_(True)
                leaves.append(D)
                gn = getattr(self, blk)[idx + 1] if self.gn_groups else None
                ys.append(GnReluPoolFunction.apply(D, stats, gn.weight if gn is not None else None, gn.bias if gn is not None else None,
                                                   self.gn_groups, pool))
            self.tail_conv_outputs = leaves
            z = None
            for lvl in range(4):
                zl = HeadsFunction.apply(ys[lvl], mats[lvl], None, None, None, None)
                z = zl if z is None else zl + UpsampleTrilinearFunction.apply(z, self.t_scales[lvl - 1], 2, 2)
            if bias is not None:
                z = z + bias[:, None, None, None]
            return self._tail_activation(z, act, axes, grids)

    @staticmethod
    def _tail_activation(z, act, axes, grids):
        """The heads' activations (csrc/heads.hip head_act) on the summed pre-activation [n_out, T, H, W]: the one place of the folded form
        where they can sit, on maps of at most 10 channels (a wide linear head, ``train_wide_head``, has none: z is returned as it is)."""
        if not any(act):
            return z
        shapes = {1: (-1, 1, 1), 2: (1, -1, 1), 3: (1, 1, -1)}
        outs = []
        for o, (a, ax) in enumerate(zip(act, axes)):
            zo = z[o]
            grid = grids[ax - 1].reshape(shapes[ax]) if (a in (1, 4) and ax) else None
            if a == 1:
                zo = torch.tanh(0.25 * zo)
            elif a == 2:
                zo = torch.sigmoid(zo)
            elif a == 3:
                zo = torch.exp(zo) * 10.0
            outs.append(zo if grid is None else zo + grid)
        return torch.stack(outs, 0)

    def forward_stacks_trainable(self, x, full=False):
        """``forward`` with a graph: list of 4 feature stacks [N, C, T, h, w] in the decoder's own order -> [N, n_out, T, H/4, W/4], sample
        by sample through ``forward_tail_trainable`` or, with ``full``, through ``forward_trainable``."""
        assert len(x) == 4, "Expected 4 feature maps, got {}".format(len(x))
        x = self._trunk_order(x)
        run = self.forward_trainable if full else self.forward_tail_trainable
        return torch.stack([run([f[n] for f in x], self._train_acts()) for n in range(x[0].shape[0])], 0)
