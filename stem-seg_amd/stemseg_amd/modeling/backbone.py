"""2-D encoder: ResNet-50/101 / ResNeXt (FrozenBN, stride in the first 1x1 or in the 3x3) + FPN on the HIP implicit-GEMM kernels.

Counterpart of the reference's stemseg/modeling/backbone/* (ResNet resnet.py:49-113, Bottleneck :194-282,
BaseStem :285-304, FPN fpn.py:8-69, FrozenBatchNorm2d make_layers.py:37-63) and of
TrainingModel.run_backbone (model_builder.py:154-169).  State-dict keys follow the reference
(``body.stem.conv1.weight``, ``body.layerL.B.{conv1,bn1,...}``, ``fpn.fpn_{inner,layer}K.{weight,bias}``) so real
checkpoints load; the ``nn.Conv2d`` / ``FrozenBatchNorm2d`` objects are parameter holders only.  ``num_groups`` /
``width_per_group`` / ``stride_in_1x1`` are MODEL.RESNETS.NUM_GROUPS / WIDTH_PER_GROUP / STRIDE_IN_1X1 (resnet.py:64-89, :227-249):
the bottleneck width of stage s is num_groups * width_per_group * 2^s and conv2 a grouped 3x3 convolution (csrc/grouped_conv.hip).

Execution (``stemseg_hip_encoder_forward``, csrc/encoder.hip): all T frames of a clip form the T axis of one
[C][T][H][W] volume, every FrozenBN (eps = 0, make_layers.py:43) is folded into its convolution once at load time, and
bias / ReLU / residual add run in the conv epilogue.  The four FPN maps come out channel-major ([256][T][h][w]) -- or
are written straight into the decoders' zero-haloed input buffers (``run_backbone_into``).
"""
import ctypes as C
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import hip
from ..utils.global_registry import GlobalRegistry

STAGE_BLOCKS = {"R-50-FPN": (3, 4, 6, 3), "R-101-FPN": (3, 4, 23, 3)}
GROUP_WIDTHS = (4, 8)        # WIDTH_PER_GROUP with NUM_GROUPS > 1: 4 .. 64 channels per group over the four stages (the kernel's widths)


def check_resnet_arch(num_groups, width_per_group):
    """Raise NotImplementedError (naming the key) for a bottleneck width the HIP encoder does not run."""
    g, w = int(num_groups), int(width_per_group)
    if g < 1:
        raise NotImplementedError("MODEL.RESNETS.NUM_GROUPS=%d" % g)
    if g == 1 and w != 64:
        raise NotImplementedError("MODEL.RESNETS.WIDTH_PER_GROUP=%d with NUM_GROUPS=1 (64 only)" % w)
    if g > 1 and (w not in GROUP_WIDTHS or (g * w) % 32):
        raise NotImplementedError("MODEL.RESNETS.WIDTH_PER_GROUP=%d with NUM_GROUPS=%d (per-group widths %s, NUM_GROUPS x WIDTH_PER_GROUP a "
                                  "multiple of 32)" % (w, g, GROUP_WIDTHS))


class FrozenBatchNorm2d(nn.Module):
    """Per-channel affine with fixed statistics (make_layers.py:37-63); holds buffers, folded away at load time."""

    def __init__(self, n, epsilon=0.0):
        super().__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))
        self.epsilon = epsilon

    def scale_shift(self):
        scale = self.weight * (self.running_var + self.epsilon).rsqrt()
        return scale, self.bias - self.running_mean * scale


def _conv(cin, cout, k, stride=1, bias=False, groups=1):
    m = nn.Conv2d(cin, cout, k, stride=stride, padding=(k - 1) // 2, bias=bias, groups=groups)
    nn.init.kaiming_uniform_(m.weight, a=1)
    if bias:
        nn.init.constant_(m.bias, 0)
    return m


class _Bottleneck(nn.Module):
    def __init__(self, cin, mid, cout, stride, groups=1, stride_in_1x1=True):
        super().__init__()
        self.downsample = None
        if cin != cout:
            self.downsample = nn.Sequential(_conv(cin, cout, 1, stride), FrozenBatchNorm2d(cout))
        s1, s3 = (stride, 1) if stride_in_1x1 else (1, stride)           # STRIDE_IN_1X1 (defaults.yaml:55, resnet.py:227-238)
        self.conv1, self.bn1 = _conv(cin, mid, 1, s1), FrozenBatchNorm2d(mid)
        self.conv2, self.bn2 = _conv(mid, mid, 3, s3, groups=groups), FrozenBatchNorm2d(mid)
        self.conv3, self.bn3 = _conv(mid, cout, 1), FrozenBatchNorm2d(cout)
        self.stride, self.groups = stride, groups
        self.stride_in_3x3 = stride > 1 and not stride_in_1x1


class _Stem(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        nn.init.kaiming_uniform_(self.conv1.weight, a=1)
        self.bn1 = FrozenBatchNorm2d(64)


class _Body(nn.Module):
    def __init__(self, blocks, num_groups=1, width_per_group=64, stride_in_1x1=True):
        super().__init__()
        self.stem = _Stem()
        cin = 64
        for li, n in enumerate(blocks, 1):
            mid, cout = num_groups * width_per_group * 2 ** (li - 1), 256 * 2 ** (li - 1)      # resnet.py:64-89
            layer = []
            for bi in range(n):
                layer.append(_Bottleneck(cin, mid, cout, 2 if (bi == 0 and li > 1) else 1, num_groups, stride_in_1x1))
                cin = cout
            setattr(self, "layer%d" % li, nn.Sequential(*layer))


class _FPN(nn.Module):
    def __init__(self, out_channels=256):
        super().__init__()
        for k in (1, 2, 3, 4):
            setattr(self, "fpn_inner%d" % k, _conv(256 * 2 ** (k - 1), out_channels, 1, bias=True))
            setattr(self, "fpn_layer%d" % k, _conv(out_channels, out_channels, 3, bias=True))


class ResNetFPN(nn.Module):
    """``forward([N,3,H,W]) -> tuple of 4 maps [N,256,H/s,W/s], highest resolution first`` (fpn.py:67-69)."""

    def __init__(self, backbone_type="R-101-FPN", out_channels=256, num_groups=1, width_per_group=64, stride_in_1x1=True):
        super().__init__()
        if backbone_type not in STAGE_BLOCKS:
            raise KeyError(backbone_type)       # "X-101-FPN" is registered but has no stage spec (resnet.py:352-355)
        check_resnet_arch(num_groups, width_per_group)
        self.stage_blocks = STAGE_BLOCKS[backbone_type]
        self.num_groups, self.width_per_group, self.stride_in_1x1 = int(num_groups), int(width_per_group), bool(stride_in_1x1)
        self.body = _Body(self.stage_blocks, self.num_groups, self.width_per_group, self.stride_in_1x1)
        self.fpn = _FPN(out_channels)
        self.out_channels, self.is_3d = out_channels, False
        self._packed, self._ws, self._ws_desc = {}, {}, {}     # precision -> (parameter signatures, packed weights, body tensors kept); workspaces (+ their descriptors) by shape / lane
        self._ws_passes = {}      # workspace key -> passes run on it (EncoderFunction's guard: its backward reads the maps its own forward left there)
        self._packed_names = {}   # precision -> {folded_state name: (packed weight, bias, folded weight)} of the body's convolutions, as the pass uses them (the body backward's recompute)
        self.precision = hip.DEFAULT_PRECISION    # hip.PRECISIONS: "f16x3" | "bf16x6" | "f32"
        self.lane = 0             # selects one of several independent workspaces (one per in-flight step / stream)
        # Every convolution of a pass decides its tile shape and split-K factor as if the pass held this many frames
        # (StemsegEncoderDesc.plan_frames): a frame's maps are then bit-identical whether it passes alone, in a batch of clips or in
        # the union of overlapping windows -- the K-partition of a split-K launch is a summation order, and the clusterer downstream is
        # a chain of hard thresholds (clusterers.py:106-146).  32 = four 8-frame clips per pass, the shape bench.py and
        # ClipPipeline.embed_many run; a job whose ranks must agree bit for bit keeps ONE value on all of them.  0: plan every pass on
        # its own frame count (fastest for a lone small pass; results then depend on the batch).
        self.plan_frames = 32
        # f16x3: conv3 (+ identity + ReLU) of a bottleneck block and conv1 of the next in one back-to-back kernel (StemsegEncoderDesc.fuse_tail):
        # bit-identical to the separate launches wherever those run un-split; True / 7: stages 1-3, a bit mask (1, 2, 4) picks stages,
        # False / 0: three launches per block everywhere (A/B, tests)
        self.fuse_tail = True
        self.train_resnext = False       # opt-in (TrainingModel.train_resnext): check_body_trainable lets grouped and stride-in-3x3 bodies pass
        self.train_stem = False          # opt-in (TrainingModel.train_stem): check_body_trainable lets FREEZE_AT_STAGE 0 and 1 pass (csrc/stem_backward.hip)
        self.stem_s2d = True             # f16x3 mode: the stem as space-to-depth + 4x4 conv on the split-staged MFMA kernel (False: the exact fp32-MFMA stem; A/B)

    # ---- FrozenBN folding: w' = w * scale[:, None, None, None], b' = shift (exact: eps == 0) -------------------
    def _signature(self):
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    @staticmethod
    def _fold(conv, bn):
        s, b = bn.scale_shift()
        return (conv.weight * s.reshape(-1, 1, 1, 1)).detach().float(), b.detach().float()

    def blocks(self):
        for li in (1, 2, 3, 4):
            for blk in getattr(self.body, "layer%d" % li):
                yield blk

    @torch.no_grad()
    def folded_state(self):
        """{name: (weight [Cout,Cin,kh,kw], bias [Cout])} with every FrozenBN folded in; plain tensor math, no conv."""
        f = OrderedDict()
        f["stem"] = self._fold(self.body.stem.conv1, self.body.stem.bn1)
        for i, blk in enumerate(self.blocks()):
            f["b%d.conv1" % i] = self._fold(blk.conv1, blk.bn1)
            f["b%d.conv2" % i] = self._fold(blk.conv2, blk.bn2)
            f["b%d.conv3" % i] = self._fold(blk.conv3, blk.bn3)
            if blk.downsample is not None:
                f["b%d.down" % i] = self._fold(blk.downsample[0], blk.downsample[1])
        for k in (1, 2, 3, 4):
            for kind in ("inner", "layer"):
                m = getattr(self.fpn, "fpn_%s%d" % (kind, k))
                f["fpn_%s%d" % (kind, k)] = (m.weight.detach().float(), m.bias.detach().float())
        return f

    def _signature_of(self, module):
        return tuple((t.data_ptr(), t._version) for t in list(module.parameters()) + list(module.buffers()))

    def _pack_fpn(self, w, keep):
        """Pack the eight FPN convolutions into ``w``; the device tensors behind the raw pointers go to ``keep``."""
        for k in (1, 2, 3, 4):
            for kind, ws, bs in (("inner", w.fpn_inner_w, w.fpn_inner_b), ("layer", w.fpn_layer_w, w.fpn_layer_b)):
                m = getattr(self.fpn, "fpn_%s%d" % (kind, k))
                wt, b = m.weight.detach().float().contiguous().cuda(), m.bias.detach().float().contiguous().cuda()
                pw = hip.pack_conv_weight_any(wt, self.precision)
                keep += [wt, pw, b]
                ws[k - 1], bs[k - 1] = pw.data_ptr(), b.data_ptr()

    def _pack(self):
        # two signatures: a training step that changed only FPN parameters re-packs only those, and the body's packed tensors stay the same objects
        sig = ((self._signature_of(self.body), bool(self.stem_s2d)), self._signature_of(self.fpn))
        hit = self._packed.get(self.precision)
        if hit is not None and hit[0] == sig:      # (one packing per precision: an overflow re-run in bf16x6 keeps the f16x3 one)
            return hit[1]
        hip.require_gpu()
        if hit is not None and hit[0][0] == sig[0]:
            (w, keep), n_body = hit[1], hit[2]
            del keep[n_body:]
            self._pack_fpn(w, keep)
            self._packed[self.precision] = (sig, (w, keep), n_body)
            return w, keep
        f = self.folded_state()
        keep = []                           # device tensors referenced by raw pointers below
        names = {}                          # the same tensors by name
        w = hip.EncoderWeights()

        def dev(t):
            t = t.contiguous().cuda()
            keep.append(t)
            return t

        def packed(name):
            wt, b = f[name]
            wd = dev(wt)
            pw, pb = hip.pack_conv_weight_any(wd, self.precision), dev(b)
            keep.append(pw)
            names[name] = (pw, pb, wd)
            return pw.data_ptr(), pb.data_ptr()
        sw, sb = f["stem"]
        w.stem_w = dev(sw.reshape(64, 147).t()).data_ptr()
        w.stem_b = dev(sb).data_ptr()
        if self.precision == "f16x3" and self.stem_s2d:
            # the stem as a stride-1 4x4 convolution over the space-to-depth image (csrc/encoder.hip, stem_s2d_kernel):
            # W2[co][(p*2+q)*3+c][a][b] = w[co][c][2a+p-1][2b+q-1], zero where an index is -1
            w8 = torch.zeros(64, 3, 8, 8, dtype=torch.float32, device=sw.device)
            w8[:, :, 1:, 1:] = sw.reshape(64, 3, 7, 7)
            w2 = w8.reshape(64, 3, 4, 2, 4, 2).permute(0, 3, 5, 1, 2, 4).reshape(64, 12, 1, 4, 4)      # [co][p][q][c][a][b]
            pw2 = hip.pack_conv_weight_any(dev(w2), "f16x3")
            keep.append(pw2)
            w.stem_w_s2d = pw2.data_ptr()
        for i, blk in enumerate(self.blocks()):
            w.conv1_w[i], w.conv1_b[i] = packed("b%d.conv1" % i)
            if blk.groups > 1 or blk.stride_in_3x3:           # conv2 on the grouped kernel (StemsegEncoderWeights.conv2_w)
                wt, b = f["b%d.conv2" % i]
                wd = dev(wt)
                pw, pb = hip.pack_grouped_conv_weight(wd, blk.groups, self.precision), dev(b)
                keep.append(pw)
                names["b%d.conv2" % i] = (pw, pb, wd)         # (the body backward's recompute and data gradient: train_resnext)
                w.conv2_w[i], w.conv2_b[i] = pw.data_ptr(), pb.data_ptr()
            else:
                w.conv2_w[i], w.conv2_b[i] = packed("b%d.conv2" % i)
            w.conv3_w[i], w.conv3_b[i] = packed("b%d.conv3" % i)
            if blk.downsample is not None:
                w.down_w[i], w.down_b[i] = packed("b%d.down" % i)
        n_body = len(keep)
        self._pack_fpn(w, keep)
        self._packed[self.precision] = (sig, (w, keep), n_body)
        self._packed_names[self.precision] = names
        return w, keep

    def _desc(self, T, H, W, n_clips=1, clip_frames=0, clip_stride=0):
        d = hip.EncoderDesc()
        d.struct_bytes = C.sizeof(hip.EncoderDesc)
        for i, n in enumerate(self.stage_blocks):
            d.blocks[i] = n
        d.T, d.H, d.W, d.out_channels = T, H, W, self.out_channels
        d.precision = hip.PRECISIONS[self.precision]
        d.n_clips, d.clip_frames, d.clip_stride = n_clips, clip_frames, clip_stride
        d.plan_frames = int(self.plan_frames)
        d.fuse_tail = 7 if self.fuse_tail is True else int(self.fuse_tail)      # (bit s - 1: stage s)
        d.conv2_groups, d.width_per_group, d.stride_in_3x3 = self.num_groups, self.width_per_group, int(not self.stride_in_1x1)
        return d

    @torch.no_grad()
    def run_backbone_into(self, frames, out_volumes, window=None):
        """frames: float32 [T,3,H,W] on the device; out_volumes: 4 ``hip.Volume`` (4x, 8x, 16x, 32x), each
        [256][T][H/s][W/s] -- e.g. the interiors of the decoders' zero-haloed inputs.  With 4 * n volumes the T frames are n
        consecutive clips of T / n frames sharing one encoder pass; volumes 4c .. 4c+3 receive clip c.  ``window`` =
        (clip_frames, clip_stride): the n clips are overlapping windows of the pass (shared frames go through the trunk once)."""
        hip.require_gpu()
        frames = frames.contiguous().float()
        T, _, H, W = frames.shape
        w, _keep = self._pack()
        n = len(out_volumes) // 4
        assert len(out_volumes) % 4 == 0
        if window is None:
            assert T % n == 0
            d = self._desc(T, H, W, n)
        else:
            assert (n - 1) * window[1] + window[0] == T, "windows do not cover the pass"
            d = self._desc(T, H, W, n, int(window[0]), int(window[1]))
        key = (T, H, W, frames.device.index, self.lane, None if window is None else (n, int(window[0]), int(window[1])), int(self.plan_frames))
        ws = self._ws.get(key)
        if ws is None:
            nbytes = hip.lib().stemseg_hip_encoder_workspace_bytes(C.byref(d))
            if nbytes == 0:
                raise RuntimeError("encoder: " + hip.lib().stemseg_hip_last_error().decode())
            ws = torch.empty(nbytes, dtype=torch.uint8, device=frames.device)
            hip.check(hip.lib().stemseg_hip_encoder_init_workspace(C.byref(d), hip.ptr(ws), nbytes, hip.stream()))
            self._ws[key] = ws
        self._ws_desc[key] = d              # (of THIS pass: the key holds no precision, and the stage-end tails depend on it)
        vols = (hip.Volume * len(out_volumes))(*out_volumes)
        hip.check(hip.lib().stemseg_hip_encoder_forward(C.byref(d), C.byref(w), hip.ptr(frames), vols, hip.ptr(ws), ws.numel(), hip.stream()))
        self._ws_passes[key] = self._ws_passes.get(key, 0) + 1

    def workspace_key(self, frames):
        """The key of the workspace a plain pass (one clip, no windows) over ``frames`` [T, 3, H, W] runs on, on the current lane."""
        T, _, H, W = frames.shape
        return (T, H, W, frames.device.index, self.lane, None, int(self.plan_frames))

    def fpn_workspace_views(self, key):
        """What the last pass on the workspace ``key`` left there for the FPN backward: -> (the stage outputs Cst[k] as 4 dense views
        [256 << k][T][h_k][w_k], the merged laterals L[k] as 4 y/x-zero-haloed views [256][T][h_k + 2][w_k + 2], the number of passes run on
        the workspace so far).  No later step of a pass re-uses either slot (csrc/encoder.hip make_encoder_plan), in any precision, with or
        without the fused tails."""
        if key not in self._ws or key[5] is not None:
            raise KeyError("no plain pass has run on workspace %r" % (key,))
        T, H, W = key[:3]
        offs = (C.c_int64 * 25)()
        hip.check(hip.lib().stemseg_hip_encoder_plan_offsets(C.byref(self._ws_desc[key]), offs))
        ws = self._ws[key]
        c_views, l_views = [], []
        for k in range(4):
            cn, h, w = 256 << k, H >> (2 + k), W >> (2 + k)
            c_views.append(hip.Volume(ws.data_ptr() + 4 * offs[4 + k], T * h * w, h * w, w, cn, T, h, w, cn * T * h * w))
            l_views.append(hip.padded2d_halo_view(ws, hip.padded2d_geometry(self.out_channels, T, h, w), self.out_channels, T, h, w, offset=offs[15 + k]))
        return c_views, l_views, self._ws_passes[key]

    def fpn_parameter_list(self):
        """The sixteen tensors of the eight FPN convolutions in EncoderFunction's order: inner weights, inner biases, layer weights, layer biases."""
        mods = [getattr(self.fpn, "fpn_%s%d" % (kind, k)) for kind in ("inner", "layer") for k in (1, 2, 3, 4)]
        return [m.weight for m in mods[:4]] + [m.bias for m in mods[:4]] + [m.weight for m in mods[4:]] + [m.bias for m in mods[4:]]

    def forward_trainable_fpn(self, frames):
        """frames [F, 3, H, W] -> the four maps [F, 256, h, w] of ``forward`` (the same encoder pass: the same bits) attached to the graph of
        the FPN's parameters (modeling/ops.py EncoderFunction: the backward reads the pass's stage outputs and merged laterals from its workspace,
        so no other pass may run on that workspace -- shape, device and ``lane`` -- between this call and ``backward()``).  The body is
        frozen: the frames and the body's parameters get no gradient."""
        return self._forward_trainable(frames, None, self.fpn_parameter_list())

    # ---- the body's backward: stages freeze_at .. 4 (modeling/ops.py EncoderFunction, encoder_backward.body_backward) ----
    def check_body_trainable(self, freeze_at, train_stem=None, train_resnext=None):
        """Raise NotImplementedError, naming the config key, for a body whose backward does not exist.  ``train_resnext`` lets grouped and
        stride-in-3x3 bodies pass (hip.conv2d_grouped_wgrad / conv2d_grouped_dgrad), ``train_stem`` FREEZE_AT_STAGE 0 and 1
        (hip.maxpool3x3s2_backward / stem_wgrad).  The keywords stand in for the backbone's own switches for this one question."""
        train_stem = self.train_stem if train_stem is None else train_stem
        train_resnext = self.train_resnext if train_resnext is None else train_resnext
        if self.num_groups != 1 and not train_resnext:
            raise NotImplementedError("MODEL.RESNETS.NUM_GROUPS=%d: the body's backward has no grouped-convolution backward (NUM_GROUPS=1 only)" % self.num_groups)
        if not self.stride_in_1x1 and not train_resnext:
            raise NotImplementedError("MODEL.RESNETS.STRIDE_IN_1X1=False: the body's backward has no backward of the stride-2 3x3 convolution "
                                      "(STRIDE_IN_1X1=True only)")
        if freeze_at not in ((0, 1, 2, 3, 4) if train_stem else (2, 3, 4)):
            raise NotImplementedError("MODEL.BACKBONE.FREEZE_AT_STAGE=%r: the body's backward covers layer2 .. layer4 (FREEZE_AT_STAGE 2, 3 or 4); "
                                      "below that it would need the backward of the max-pool and the stem" % (freeze_at,))

    def _stage_blocks_of(self, st):
        """[(index among ``blocks()``, block)] of layer ``st``."""
        first = sum(self.stage_blocks[:st - 1])
        return [(first + b, blk) for b, blk in enumerate(getattr(self.body, "layer%d" % st))]

    def body_parameter_list(self, freeze_at=2):
        """The convolution weights of layer{freeze_at} .. layer4 in network order (per block: downsample.0 where there is one, conv1, conv2,
        conv3; FrozenBN holds buffers only): what EncoderFunction takes and returns gradients for.  R-50, freeze_at 2: 13 + 19 + 10 tensors.
        With ``train_stem``: freeze_at 1 starts at layer1 (10 more on an R-50), freeze_at 0 at ``stem.conv1.weight``, then layer1."""
        self.check_body_trainable(freeze_at)
        out = [self.body.stem.conv1.weight] if freeze_at == 0 else []
        for st in range(max(freeze_at, 1), 5):
            for _, blk in self._stage_blocks_of(st):
                out += ([blk.downsample[0].weight] if blk.downsample is not None else []) + [blk.conv1.weight, blk.conv2.weight, blk.conv3.weight]
        return out

    def body_stage_specs(self, freeze_at, names):
        """{stage: per block the dict ``encoder_backward.body_backward`` takes}: the pass's packed weights and biases and folded weights from ``names``
        (``_packed_names[precision]``), the FrozenBN scales, the stride.  The stages max(freeze_at, 1) .. 4."""
        dev = next(iter(names.values()))[0].device
        scale = lambda bn: bn.scale_shift()[0].detach().float().contiguous().to(dev)
        specs = {}
        for st in range(max(freeze_at, 1), 5):
            specs[st] = []
            for i, blk in self._stage_blocks_of(st):
                c1, c2, c3 = (names["b%d.conv%d" % (i, j)] for j in (1, 2, 3))
                d = dict(conv1=c1[:2], conv2=c2[:2], conv3=c3[:2], w1=c1[2], w2=c2[2], w3=c3[2], s1=scale(blk.bn1), s2=scale(blk.bn2), s3=scale(blk.bn3),
                         stride=blk.stride, groups=blk.groups, stride_in_3x3=blk.stride_in_3x3)
                if blk.downsample is not None:
                    dn = names["b%d.down" % i]
                    d.update(down=dn[:2], wd=dn[2], sd=scale(blk.downsample[1]))
                specs[st].append(d)
        return specs

    def stem_forward(self, frames, precision=None):
        """frames [T, 3, H, W] -> (the stem's output after its ReLU [64, T, H/2, W/2], the pooled map [64, T, H/4, W/4]) as a plain pass
        over these frames in ``precision`` (default: the backbone's current one; a backward hands in its own pass's) computes them: the
        pass's own stem code again (``stemseg_hip_encoder_stem_forward``) with a descriptor and the packed weights of that precision,
        into fresh tensors.  (The descriptor is built here, not taken from the workspace's: the workspace key holds no precision.)  The pass's own slices of both maps are re-used by the stage-end tails
        (csrc/encoder.hip make_encoder_plan), so the backward of the stem and of layer1 recomputes them.  Only the space-to-depth slice of
        the workspace is written."""
        hip.require_gpu()
        frames = frames.detach().contiguous().float()
        key = self.workspace_key(frames)
        if key not in self._ws:
            raise KeyError("no plain pass has run on workspace %r" % (key,))
        T, _, H, W = frames.shape
        if precision is not None and precision not in hip.PRECISIONS:
            raise ValueError("stem_forward: precision %r" % (precision,))
        own, self.precision = self.precision, precision or self.precision
        try:
            (w, _keep), d = self._pack(), self._desc(T, H, W)
        finally:
            self.precision = own
        ws = self._ws[key]
        stem = torch.empty(64, T, H // 2, W // 2, dtype=torch.float32, device=frames.device)
        pooled = torch.empty(64, T, H // 4, W // 4, dtype=torch.float32, device=frames.device)
        hip.check(hip.lib().stemseg_hip_encoder_stem_forward(C.byref(d), C.byref(w), hip.ptr(frames), hip.ptr(stem), hip.ptr(pooled), hip.ptr(ws), ws.numel(),
                                                             hip.stream()))
        return stem, pooled

    def body_stage_inputs(self, key, freeze_at, frames=None, precision=None):
        """{stage: the input of the stage as the last pass on workspace ``key`` left it}: Cst[stage - 2], a tensor view [C, T, h, w] of the
        workspace (no copy; valid until the next pass on it).  ``freeze_at`` 0 or 1 (``train_stem``): stage 1's input is the pooled map,
        which the pass does not keep -- recomputed from ``frames`` in the pass's ``precision`` (``stem_forward``), with the stem's output as
        entry 0."""
        c_views, _, _ = self.fpn_workspace_views(key)
        ws = self._ws[key].view(torch.float32)
        out = {}
        if freeze_at < 2:
            if frames is None:
                raise ValueError("body_stage_inputs: freeze_at %d needs the frames (the stem and the pooled map are recomputed)" % freeze_at)
            out[0], out[1] = self.stem_forward(frames, precision)
        for st in range(max(freeze_at, 2), 5):
            v = c_views[st - 2]
            off = (v.ptr - ws.data_ptr()) // 4
            out[st] = ws[off:off + v.C * v.T * v.H * v.W].view(v.C, v.T, v.H, v.W)
        return out

    def forward_trainable_body(self, frames, freeze_at=2):
        """frames [F, 3, H, W] -> the four maps [F, 256, h, w] of ``forward`` (the same encoder pass: the same bits) attached to the graph of
        the FPN's parameters and of the convolution weights of layer{freeze_at} .. layer4 (modeling/ops.py EncoderFunction; the rule of
        ``forward_trainable_fpn`` about the workspace holds).  The stem and the layers below ``freeze_at`` (2, 3 or 4) are frozen.  With
        ``train_stem`` also 1 (layer1 .. layer4) and 0 (the stem's conv1 as well)."""
        return self._forward_trainable(frames, int(freeze_at), self.body_parameter_list(freeze_at) + self.fpn_parameter_list())

    def _forward_trainable(self, frames, freeze_at, params):
        from .ops import EncoderFunction
        hip.require_gpu()
        return tuple(o.permute(1, 0, 2, 3) for o in EncoderFunction.apply(self, frames.detach().contiguous().float(), freeze_at, *params))

    def check_workspaces(self):
        """Debug check (synchronises): clobbered guard words over all cached workspaces -- 0 unless some kernel wrote outside its
        slice (stemseg_hip_encoder_check_workspace).  -> (n_bad, [(workspace key, first bad float offset)])"""
        bad, where = 0, []
        for key, ws in self._ws.items():
            n, first = C.c_int32(0), C.c_int64(-1)
            with torch.cuda.device(ws.device):
                hip.check(hip.lib().stemseg_hip_encoder_check_workspace(C.byref(self._ws_desc[key]), hip.ptr(ws), ws.numel(), C.byref(n), C.byref(first), hip.stream()))
            if n.value:
                bad += n.value
                where.append((key, first.value))
        return bad, where

    @torch.no_grad()
    def forward_channel_major(self, frames):
        """-> 4 dense tensors [256, T, H/s, W/s] (s = 4, 8, 16, 32)."""
        T, _, H, W = frames.shape
        outs = [torch.empty(self.out_channels, T, H // s, W // s, dtype=torch.float32, device=frames.device) for s in (4, 8, 16, 32)]
        self.run_backbone_into(frames, [hip.dense_volume(o) for o in outs])
        return outs

    @torch.no_grad()
    def forward(self, x):
        return tuple(o.permute(1, 0, 2, 3) for o in self.forward_channel_major(x))

    @torch.no_grad()
    def run_backbone(self, frames):
        """frames [T,3,H,W] -> OrderedDict {4,8,16,32: [T,256,H/s,W/s]} (model_builder.py:154-169)."""
        return OrderedDict(zip((4, 8, 16, 32), self.forward(frames)))


def build_resnet_fpn_backbone(cfg):
    if cfg.MODEL.BACKBONE.TYPE not in STAGE_BLOCKS:
        raise KeyError(cfg.MODEL.BACKBONE.TYPE)        # "X-101-FPN" (resnet.py:352-355)
    r = cfg.MODEL.RESNETS
    # keys a cfg may lack take the reference's defaults (defaults.yaml:50-60)
    num_groups, width = getattr(r, "NUM_GROUPS", 1), getattr(r, "WIDTH_PER_GROUP", 64)
    stride_in_1x1 = getattr(r, "STRIDE_IN_1X1", True)
    if getattr(r, "STEM_OUT_CHANNELS", 64) != 64:
        raise NotImplementedError("MODEL.RESNETS.STEM_OUT_CHANNELS=%s (64 only)" % r.STEM_OUT_CHANNELS)
    if getattr(r, "RES2_OUT_CHANNELS", 256) != 256:
        raise NotImplementedError("MODEL.RESNETS.RES2_OUT_CHANNELS=%s (256 only)" % r.RES2_OUT_CHANNELS)
    fpn = getattr(cfg.MODEL, "FPN", None)
    for key in ("USE_GN", "USE_RELU"):
        if fpn is not None and getattr(fpn, key, False):
            raise NotImplementedError("MODEL.FPN.%s=True" % key)
    check_resnet_arch(num_groups, width)
    return ResNetFPN(cfg.MODEL.BACKBONE.TYPE, cfg.MODEL.RESNETS.BACKBONE_OUT_CHANNELS, num_groups, width, stride_in_1x1)


BACKBONE_REGISTRY = GlobalRegistry.get("Backbone")
BACKBONE_REGISTRY.add("R-50-FPN", build_resnet_fpn_backbone)
BACKBONE_REGISTRY.add("R-101-FPN", build_resnet_fpn_backbone)
BACKBONE_REGISTRY.add("X-101-FPN", build_resnet_fpn_backbone)
