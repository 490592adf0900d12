"""``build_model`` and ``TrainingModel``: backbone + heads from the global cfg, and the loss side of training.

Counterpart of ``stemseg/modeling/model_builder.py``: ``build_model`` :247-369 (registry look-ups by the cfg's type strings,
constructor contracts of SURVEY.md section 8(b)), the inference-time surface of ``TrainingModel`` :37-73,154-169 that
``modeling/inference_model.py`` uses (``backbone``, the three heads, their feature-map scale lists, ``run_backbone``), and its loss
side :101-152,210-244: ``resize_masks`` (the training targets at 1/4 scale), ``compute_fg_loss`` and ``compute_losses`` on the device
(csrc/semseg_loss.hip, csrc/embedding_loss.hip), value and gradient with respect to the heads' outputs.  ``forward`` is the reference's
forward; the graph it builds is decided once, by ``TrainingModel.trainable_scope()``, the first level of this table that applies:

  level       what must be set                               what may be trainable                     which kernels carry it
  ----------  ---------------------------------------------  ----------------------------------------  ------------------------------------------
  None        gradients disabled, or nothing trainable       --                                        the no-grad pass (validation)
  "body"      train_decoders, train_fpn, train_body and a    the decoders, the FPN, body_parameters(   csrc/bottleneck_backward.hip (and, with
              trainable backbone.body parameter              fa): layer2 .. 4; with train_stem also    train_stem, csrc/stem_backward.hip) behind
                                                             layer1 and stem.conv1 (fa 1, 0)           ResNetFPN.forward_trainable_body
  "fpn"       train_decoders, train_fpn and a trainable      decoder_parameters(), fpn_parameters()    csrc/conv_backward.hip behind
              FPN parameter                                                                            ResNetFPN.forward_trainable_fpn
  "decoders"  train_decoders                                 decoder_parameters()                      the 3x3x3 convolutions' backward,
                                                                                                       csrc/conv_backward.hip (modeling/ops.py)
  "tail"      --                                             tail_parameters()                         csrc/decoder_backward.hip

A trainable parameter outside its level's set is refused.  Orthogonal to the levels, ``train_wide_head`` lets every one of them take a wide
linear semseg head (11 .. 64 channels: the 42 of the YouTube-VIS preset; csrc/decoder_backward.hip's wide heads' kernels), and
``train_resnext`` lets "body" take a ResNeXt body (grouped conv2 and / or the stride in the 3x3: csrc/conv_backward.hip's grouped weight
gradient).
"""
import os
from collections import OrderedDict, namedtuple

import torch
import torch.nn as nn

from .. import config as _config
from .. import hip
from ..config import cfg
from ..utils.constants import Loss as LossConsts, ModelOutput
from ..utils.global_registry import GlobalRegistry
from ..utils.paths import ModelPaths
from .backbone import BACKBONE_REGISTRY
from .embedding_decoder import EMBEDDING_HEAD_REGISTRY
from .embedding_utils import get_nb_free_dims
from .losses import CrossEntropyLoss, EmbeddingLoss
from .losses.cross_entropy import foreground_loss
from .seediness_decoder import SEEDINESS_HEAD_REGISTRY
from .semseg_decoder import SEMSEG_HEAD_REGISTRY

SEMSEG_LOSS_REGISTRY = GlobalRegistry.get("SemsegLoss")
SEMSEG_LOSS_REGISTRY.add("CrossEntropy", CrossEntropyLoss)

# what ``TrainingModel.trainable_scope`` returns: level None | "tail" | "decoders" | "fpn" | "body"; freeze_at with "body" only
TrainableScope = namedtuple("TrainableScope", "level freeze_at")


def _frames_of(image_seqs):
    """ImageList-like (``.tensors`` [N,T,3,H,W]) or a float tensor [..., 3, H, W] -> the frames [N*T, 3, H, W], contiguous fp32."""
    x = image_seqs.tensors if hasattr(image_seqs, "tensors") else image_seqs
    return x.reshape((-1,) + tuple(x.shape[-3:])).contiguous().float()


def _mirrored(name, child, only_with=None):
    """A bool switch of the model that is handed on to ``child``'s attribute of the same name (when the child is there and, with
    ``only_with``, has that attribute)."""
    def setter(self, on):
        setattr(self, "_" + name, bool(on))
        target = getattr(self, child)
        if target is not None and (only_with is None or hasattr(target, only_with)):
            setattr(target, name, bool(on))
    return property(lambda self: getattr(self, "_" + name), setter)


class InferenceOnlyModel(nn.Module):
    """State-dict compatible with the reference's TrainingModel (keys ``backbone.*``, ``embedding_head.*``,
    ``seediness_head.*``, ``semseg_head.*``)."""

    def __init__(self):
        super().__init__()
        self.backbone = None
        self.embedding_head = self.seediness_head = self.semseg_head = None
        self.embedding_head_feature_map_scale = self.seediness_head_feature_map_scale = self.semseg_feature_map_scale = None

    embedding_head_output_scale = property(lambda self: min(self.embedding_head_feature_map_scale))
    semseg_output_scale = property(lambda self: min(self.semseg_feature_map_scale) if self.semseg_feature_map_scale else 4)
    feature_map_scales = (4, 8, 16, 32)

    @torch.no_grad()
    def run_backbone(self, image_seqs):
        """ImageList-like (``.tensors`` [N,T,3,H,W]) or a float tensor [..., 3, H, W] -> OrderedDict {4, 8, 16, 32: [N*T, 256,
        H/s, W/s]} (model_builder.py:154-169)."""
        return OrderedDict(zip(self.feature_map_scales, self.backbone(_frames_of(image_seqs))))

    def forward(self, image_seqs, targets):
        raise NotImplementedError("training is outside the MI355X hot path (SURVEY.md section 2); use InferenceModel")


class TrainingModel(InferenceOnlyModel):
    """The reference's TrainingModel (model_builder.py:37-244): its constructor arguments and attributes, the state-dict keys of the
    backbone and the heads, and the loss side on the device.  One difference in the state dict: ``embedding_loss_criterion``'s
    ``free_dim_bandwidths`` buffer (1 / std^2 of the cfg's FREE_DIM_STDS) is not persistent here, so ``state_dict()`` holds the weights
    only, as before; a reference checkpoint carries that buffer and ``InferenceModel.load_checkpoint_state`` ignores it."""

    def __init__(self, backbone, embedding_head, embedding_head_feature_map_scale, embedding_loss_criterion, semseg_head,
                 semseg_feature_map_scale, semseg_loss_criterion, seediness_head, seediness_head_feature_map_scale,
                 multiclass_semseg_output, output_resize_scale, logger):
        super().__init__()
        self.backbone = backbone
        self.embedding_head = embedding_head
        self.embedding_head_feature_map_scale = list(embedding_head_feature_map_scale)
        if embedding_loss_criterion is not None and "free_dim_bandwidths" in dict(embedding_loss_criterion.named_buffers(recurse=False)):
            bw = embedding_loss_criterion.free_dim_bandwidths
            del embedding_loss_criterion.free_dim_bandwidths
            embedding_loss_criterion.register_buffer("free_dim_bandwidths", bw, persistent=False)
        self.embedding_loss_criterion = embedding_loss_criterion
        self.semseg_head = semseg_head
        self.semseg_feature_map_scale = list(semseg_feature_map_scale) if semseg_head is not None else None
        self.semseg_loss_criterion = semseg_loss_criterion
        self.seediness_head = seediness_head
        self.seediness_head_feature_map_scale = list(seediness_head_feature_map_scale)
        self.multiclass_semseg_output = multiclass_semseg_output
        self.output_resize_scale = output_resize_scale
        self.logger = logger
        # the opt-in switches of the levels "decoders", "fpn" and "body" (the module docstring's table): each counts only together with the
        # ones before it; all False, only the decoders' tails can be trainable
        self.train_decoders = self.train_fpn = self.train_body = False
        # opt-in, orthogonal to the three above (it counts with any of them, the tail-only path included): True lets the trainable paths take a
        # WIDE linear semseg head -- 11 .. 64 output channels, the 42 of the YouTube-VIS preset -- through the folded tail on
        # csrc/decoder_backward.hip's wide heads' kernels.  False: such a head is refused, as ever.  Set it here, not on the head: the
        # property hands it to ``semseg_head.train_wide_head``.
        self.train_wide_head = False
        # opt-in, counts with ``train_body``: True lets the body's backward take a ResNeXt backbone -- MODEL.RESNETS.NUM_GROUPS > 1 and / or
        # STRIDE_IN_1X1 = False -- on the grouped weight gradient of csrc/conv_backward.hip.  False: such a body is refused, as ever.  The
        # property hands it to ``backbone.train_resnext``.
        self.train_resnext = False
        # opt-in, counts with ``train_body``: True lets the body's backward go on below layer2 -- layer1 and, when it holds a trainable
        # parameter, the stem's conv1 behind the max-pool (MODEL.BACKBONE.FREEZE_AT_STAGE 1 and 0; csrc/stem_backward.hip).  False: a
        # trainable parameter there is refused, as ever.  The property hands it to ``backbone.train_stem``.
        self.train_stem = False

    train_stem = _mirrored("train_stem", "backbone", only_with="check_body_trainable")
    train_resnext = _mirrored("train_resnext", "backbone", only_with="check_body_trainable")
    train_wide_head = _mirrored("train_wide_head", "semseg_head")

    def train(self, mode=True):
        self.training = mode
        for name, module in self.named_children():
            if name == "backbone" and cfg.TRAINING.FREEZE_BACKBONE:
                continue
            module.train(mode)
        return self

    def run_backbone(self, image_seqs, scope=None):
        """``InferenceOnlyModel.run_backbone``; at the levels "body" and "fpn" of ``scope`` (default: ``trainable_scope(refuse=False)``), and
        the backbone not frozen by TRAINING.FREEZE_BACKBONE, the same pass with the four maps attached to the graph of the backbone's parameters."""
        scope = self.trainable_scope(refuse=False) if scope is None else scope
        if scope.level not in ("body", "fpn") or cfg.TRAINING.FREEZE_BACKBONE:
            return super().run_backbone(image_seqs)
        x = _frames_of(image_seqs)
        maps = self.backbone.forward_trainable_body(x, scope.freeze_at) if scope.level == "body" else self.backbone.forward_trainable_fpn(x)
        return OrderedDict(zip(self.feature_map_scales, maps))

    @torch.no_grad()
    def resize_masks(self, targets):
        """Per target dict, in place as the reference (model_builder.py:128-152): 'masks' [I,T,H,W] and 'ignore_masks' [T,H,W] at
        full resolution -> 1/4 scale, uint8; with a semseg head, 'semseg_masks' [T,H/4,W/4] from 'category_ids' [I] -- uint8 class
        ids here (int64 in the reference; the losses take both), the largest category over the instances set at a pixel.  One launch
        per sample (hip.prepare_targets); bool or uint8 inputs, non-zero is set; inputs on another device are moved to the model's."""
        assert self.embedding_head_output_scale == self.semseg_output_scale == 4
        self._refuse_full_res()
        dev = next(self.parameters()).device
        flags = []
        with torch.cuda.device(dev):
            for target in targets:
                masks, ignore = target["masks"].to(dev), target["ignore_masks"].to(dev)
                cats = target["category_ids"] if self.semseg_head is not None else torch.zeros(masks.shape[0], dtype=torch.int32)
                target["masks"], target["ignore_masks"], sem, flag = hip.prepare_targets(masks, ignore, cats)
                if self.semseg_head is not None:
                    target["semseg_masks"] = sem
                    flags.append(flag)
            if flags and int(torch.cat(flags).max()):
                raise ValueError("category_ids outside 0..255")
        return targets

    def _refuse_full_res(self):
        if self.output_resize_scale != 1.0:
            raise NotImplementedError("cfg.TRAINING.LOSS_AT_FULL_RES: True (output_resize_scale %r): the x4 trilinear up-sampling of the "
                                      "head outputs has no adjoint kernel here" % (self.output_resize_scale,))

    def compute_fg_loss(self, fg_logits, targets, output_dict):
        """fg_logits [N, T, H, W] -> output_dict[OPTIMIZATION_LOSSES][FOREGROUND] (model_builder.py:210-244)."""
        foreground_loss(fg_logits, targets, output_dict)

    def compute_losses(self, embeddings_map, semseg_logits, targets):
        """The tail of the reference's forward (model_builder.py:110-126): embeddings_map [N, C, T, h, w], semseg_logits
        [N, T, cls(+1), h, w] or None, prepared targets -> the output dict.  With a foreground channel the foreground loss and the
        cross-entropy come from one pass over the combined logits, not from two slices."""
        output = {ModelOutput.INFERENCE: {ModelOutput.EMBEDDINGS: embeddings_map, ModelOutput.SEMSEG_MASKS: semseg_logits}}
        self.embedding_loss_criterion(embeddings_map, targets, output)
        if self.semseg_head is not None:
            if self.semseg_head.has_foreground_channel and isinstance(self.semseg_loss_criterion, CrossEntropyLoss):
                self.semseg_loss_criterion.forward_with_foreground(semseg_logits, targets, output)
            else:
                if self.semseg_head.has_foreground_channel:
                    semseg_logits, fg_logits = semseg_logits.split((semseg_logits.shape[2] - 1, 1), dim=2)
                    self.compute_fg_loss(fg_logits.squeeze(2), targets, output)
                self.semseg_loss_criterion(semseg_logits, targets, output)
        return output

    def forward_embeddings_and_semseg(self, features, num_seqs, num_frames, scope=None):
        """features {scale: [N*T, C, h, w]} -> (embeddings_map [N, C, T, h, w] with RAW bandwidth channels, semseg_logits
        [N, T, cls, h, w] or None) through the heads' forward kernels (model_builder.py:171-208).  scope: default
        ``trainable_scope(refuse=False)``."""
        self._refuse_full_res()
        scope = self.trainable_scope(refuse=False) if scope is None else scope

        def stacks(scales):
            return [features[s].reshape((num_seqs, num_frames) + tuple(features[s].shape[1:])).permute(0, 2, 1, 3, 4) for s in scales]

        # a trainable graph, at any level, on the autograd Functions of modeling/ops.py: the whole decoders from "decoders" up, else their tails
        full = scope.level in ("decoders", "fpn", "body")
        run = (lambda head, x: head.forward_stacks_trainable(x, full)) if scope.level is not None else (lambda head, x: head(x))
        semseg_logits = None
        if self.semseg_head is not None:
            self.semseg_head.train_wide_head = self.train_wide_head          # (a head assigned after the switch was set)
            semseg_logits = run(self.semseg_head, stacks(self.semseg_feature_map_scale)).permute(0, 2, 1, 3, 4)
        fused, self.embedding_head.fuse_bandwidth_activation = self.embedding_head.fuse_bandwidth_activation, False
        try:
            embeddings_map = run(self.embedding_head, stacks(self.embedding_head_feature_map_scale))
        finally:
            self.embedding_head.fuse_bandwidth_activation = fused
        if self.seediness_head is not None:
            embeddings_map = torch.cat((embeddings_map, run(self.seediness_head, stacks(self.seediness_head_feature_map_scale))), dim=1)
        return embeddings_map, semseg_logits

    def tail_parameters(self):
        """{state-dict key: parameter} of what can be fine-tuned on frozen convolutions: per decoder the heads, conv_16 / conv_8 / conv_4
        and the affine parameters of the last GroupNorm of each branch (``SqueezeExpandTrunk.tail_parameter_names``)."""
        out = OrderedDict()
        for prefix in ("embedding_head", "seediness_head", "semseg_head"):
            head = getattr(self, prefix)
            if head is not None:
                params = dict(head.named_parameters())
                for n in head.tail_parameter_names():
                    out[prefix + "." + n] = params[n]
        return out

    def tail_only_trainable(self):
        """True when at least one parameter requires a gradient and every one that does is a tail parameter: what ``forward`` can build
        a graph for."""
        return self._only_trainable(self.tail_parameters())

    def _only_trainable(self, *groups):
        """Something is trainable and all of it lies in the union of these {key: parameter} groups."""
        ok = {id(p) for group in groups for p in group.values()}
        trainable = [p for p in self.parameters() if p.requires_grad]
        return bool(trainable) and all(id(p) in ok for p in trainable)

    def decoder_parameters(self):
        """{state-dict key: parameter} of every parameter of the three heads: what ``train_decoders`` makes trainable on a frozen backbone."""
        out = OrderedDict()
        for prefix in ("embedding_head", "seediness_head", "semseg_head"):
            head = getattr(self, prefix)
            if head is not None:
                for n, p in head.named_parameters():
                    out[prefix + "." + n] = p
        return out

    def decoders_only_trainable(self):
        """True when at least one parameter requires a gradient and every one that does is a decoder parameter: what ``forward`` can build
        a graph for when ``train_decoders`` is set."""
        return self._only_trainable(self.decoder_parameters())

    def fpn_parameters(self):
        """{state-dict key: parameter} of the FPN's eight convolutions (``backbone.fpn.*``, weight and bias each): what ``train_fpn`` makes
        trainable on top of the decoders."""
        return OrderedDict(("backbone.fpn." + n, p) for n, p in self.backbone.fpn.named_parameters())

    def fpn_and_decoders_only_trainable(self):
        """True when at least one parameter requires a gradient and every one that does is a decoder or an FPN parameter: what ``forward``
        can build a graph for when ``train_decoders`` and ``train_fpn`` are set."""
        return self._only_trainable(self.decoder_parameters(), self.fpn_parameters())

    def body_parameters(self, freeze_at=2):
        """{state-dict key: parameter} of the convolution weights of ``backbone.body.layer{freeze_at}`` .. ``layer4`` (FrozenBN holds buffers):
        what ``train_body`` makes trainable on top of the FPN and the decoders.  An R-50 from layer2 on: 13 + 19 + 10.  With ``train_stem``,
        ``freeze_at`` 1 adds layer1 (10 on an R-50) and 0 ``backbone.body.stem.conv1.weight`` in front of it."""
        self.backbone.check_body_trainable(freeze_at)
        out = OrderedDict()
        if freeze_at == 0:
            out["backbone.body.stem.conv1.weight"] = self.backbone.body.stem.conv1.weight
        for st in range(max(freeze_at, 1), 5):
            for n, p in getattr(self.backbone.body, "layer%d" % st).named_parameters():
                out["backbone.body.layer%d.%s" % (st, n)] = p
        return out

    def body_fpn_and_decoders_only_trainable(self, freeze_at=2):
        """True when at least one parameter requires a gradient and every one that does is a decoder, an FPN or a ``body_parameters(freeze_at)``
        parameter: what ``forward`` can build a graph for when the three switches are set."""
        return self._only_trainable(self.decoder_parameters(), self.fpn_parameters(), self.body_parameters(freeze_at))

    def _body_wanted(self):
        """The three switches are set and a parameter of the body requires a gradient."""
        return bool(self.train_decoders and self.train_fpn and self.train_body and any(p.requires_grad for p in self.backbone.body.parameters()))

    def body_freeze_at(self):
        """The lowest of layer2 .. layer4 that holds a trainable parameter (the reference's MODEL.BACKBONE.FREEZE_AT_STAGE, which the caller
        applied with ``requires_grad_``); 4 when none does.  With ``train_stem``: 0 when the stem holds a trainable parameter, 1 when
        layer1 does."""
        if self.train_stem:
            if any(p.requires_grad for p in self.backbone.body.stem.parameters()):
                return 0
            if any(p.requires_grad for p in self.backbone.body.layer1.parameters()):
                return 1
        for st in (2, 3, 4):
            if any(p.requires_grad for p in getattr(self.backbone.body, "layer%d" % st).parameters()):
                return st
        return 4

    def trainable_scope(self, refuse=True):
        """Which graph a forward builds now: ``TrainableScope(level, freeze_at)``, the first level of the module docstring's table that
        applies; ``freeze_at`` (``body_freeze_at()``) with "body" only.  A trainable parameter outside the level's set is refused with
        NotImplementedError -- with ``refuse=False`` that is ``(None, None)``, no graph.  A body whose backward does not exist is refused by
        ``backbone.check_body_trainable`` either way."""
        trainable = [(n, p) for n, p in self.named_parameters() if p.requires_grad] if torch.is_grad_enabled() else []
        if not trainable:
            return TrainableScope(None, None)
        freeze_at = None
        if self._body_wanted():
            fa = self.body_freeze_at() if self.train_stem else 2           # the lowest stage the switches let the backward reach
            self.backbone.check_body_trainable(fa)
            level, freeze_at, allowed = "body", self.body_freeze_at(), (self.decoder_parameters(), self.fpn_parameters(), self.body_parameters(fa))
            if self.train_stem:
                message = ("TrainingModel.forward with train_decoders, train_fpn, train_body and train_stem: %d parameters outside "
                           "the decoders, the FPN and the body's convolution weights require a gradient (%s, ...)")
            else:
                message = ("TrainingModel.forward with train_decoders, train_fpn and train_body: the backward pass of the stem, the "
                           "max-pool and layer1 is not implemented (MODEL.BACKBONE.FREEZE_AT_STAGE >= 2), and %d parameters there "
                           "require a gradient (%s, ...); freeze them (requires_grad_(False) on backbone.body.stem and "
                           "backbone.body.layer1)")
        elif self.train_decoders and self.train_fpn:
            allowed = (self.decoder_parameters(), self.fpn_parameters())
            level = "fpn" if any(p.requires_grad for p in allowed[1].values()) else "decoders"
            message = ("TrainingModel.forward with train_decoders and train_fpn: behind the FPN the encoder backward pass is not "
                       "implemented, and %d parameters outside the decoders and the FPN require a gradient (%s, ...); the "
                       "backbone's body must be frozen (requires_grad_(False) on backbone.body)")
        elif self.train_decoders:
            level, allowed = "decoders", (self.decoder_parameters(),)
            message = ("TrainingModel.forward with train_decoders: the encoder backward pass is not implemented, and %d "
                       "parameters outside the decoders require a gradient (%s, ...); freeze the backbone "
                       "(TRAINING.FREEZE_BACKBONE)")
        else:
            level, allowed = "tail", (self.tail_parameters(),)
            message = ("TrainingModel.forward with gradients: the decoder and encoder backward passes are not implemented; "
                       "call it under torch.no_grad() (validation), or use compute_losses for the loss gradients with "
                       "respect to the head outputs")
        ok = {id(p) for group in allowed for p in group.values()}
        other = [n for n, p in trainable if id(p) not in ok]
        if not other:
            return TrainableScope(level, freeze_at)
        if not refuse:
            return TrainableScope(None, None)
        raise NotImplementedError(message % (len(other), other[0]) if level != "tail" else message)

    def forward(self, image_seqs, targets):
        """The reference's forward (model_builder.py:101-126), with the graph of ``trainable_scope()``: none (validation), or the one of its
        level (the module docstring's table); a trainable parameter that level does not reach is refused before anything runs."""
        scope = self.trainable_scope()
        targets = self.resize_masks(targets)
        x = image_seqs.tensors if hasattr(image_seqs, "tensors") else image_seqs
        num_seqs, num_frames = x.shape[0], x.shape[1]
        features = self.run_backbone(image_seqs, scope)
        embeddings_map, semseg_logits = self.forward_embeddings_and_semseg(features, num_seqs, num_frames, scope)
        return self.compute_losses(embeddings_map, semseg_logits, targets)


# model_builder.py:29-33 (POOLER_REGISTRY / NORM_REGISTRY of the reference)
_POOLERS = {"avg": nn.AvgPool3d, "max": nn.MaxPool3d}


def _norm(kind, groups):
    if kind == "gn":
        return lambda c: nn.GroupNorm(groups, c)
    if kind == "none":
        return lambda c: nn.Identity()
    raise ValueError("NORMALIZATION_LAYER '%s' (gn | none)" % kind)


def build_model(restore_pretrained_backbone_wts=False, logger=None):
    """backbone + heads + loss criteria from the global cfg (model_builder.py:247-369).  restore_pretrained_backbone_wts: load
    ``ModelPaths.pretrained_backbones_dir() / cfg.MODEL.BACKBONE.PRETRAINED_WEIGHTS`` strictly into the backbone; ValueError when the file
    is missing (model_builder.py:264-273)."""
    _config.refresh()
    if cfg.INPUT.NUM_CLASSES > 2:
        assert cfg.MODEL.USE_SEMSEG_HEAD, "Number of object classes > 2, but 'USE_SEMSEG_HEAD' option is set to False"
    m = InferenceOnlyModel()                                          # (a holder for the parts; the model is assembled below)
    m.backbone = BACKBONE_REGISTRY[cfg.MODEL.BACKBONE.TYPE](cfg)
    if restore_pretrained_backbone_wts:
        wts_file = os.path.join(ModelPaths.pretrained_backbones_dir(), cfg.MODEL.BACKBONE.PRETRAINED_WEIGHTS)
        (logger.info if logger is not None else print)("Restoring backbone weights from '{}'".format(wts_file))
        if not os.path.exists(wts_file):
            raise ValueError("Could not find pre-trained backbone weights file at expected location: '{}'".format(wts_file))
        m.backbone.load_state_dict(torch.load(wts_file, map_location="cpu"), strict=True)
    e = cfg.MODEL.EMBEDDINGS
    norm = _norm(e.NORMALIZATION_LAYER, e.GN_NUM_GROUPS)
    m.embedding_head = EMBEDDING_HEAD_REGISTRY[e.HEAD_TYPE](
        m.backbone.out_channels, e.INTER_CHANNELS, e.EMBEDDING_SIZE, tanh_activation=e.TANH_ACTIVATION,
        seediness_output=not cfg.MODEL.USE_SEEDINESS_HEAD, experimental_dims=cfg.MODEL.EMBEDDING_DIM_MODE,
        PoolType=_POOLERS[e.POOL_TYPE], NormType=norm)
    m.seediness_head = None
    if cfg.MODEL.USE_SEEDINESS_HEAD:
        s = cfg.MODEL.SEEDINESS
        m.seediness_head = SEEDINESS_HEAD_REGISTRY[s.HEAD_TYPE](
            m.backbone.out_channels, s.INTER_CHANNELS, PoolType=_POOLERS[s.POOL_TYPE], NormType=_norm(s.NORMALIZATION_LAYER, s.GN_NUM_GROUPS))
    m.semseg_head = None
    if cfg.MODEL.USE_SEMSEG_HEAD:
        g = cfg.MODEL.SEMSEG
        m.semseg_head = SEMSEG_HEAD_REGISTRY[g.HEAD_TYPE](
            m.backbone.out_channels, cfg.INPUT.NUM_CLASSES, inter_channels=g.INTER_CHANNELS, feature_scales=g.FEATURE_SCALE,
            foreground_channel=g.FOREGROUND_CHANNEL, PoolType=_POOLERS[g.POOL_TYPE], NormType=_norm(g.NORMALIZATION_LAYER, g.GN_NUM_GROUPS))
        m.semseg_feature_map_scale = list(g.FEATURE_SCALE)
    embedding_loss_criterion = EmbeddingLoss(min(e.SCALE), embedding_size=e.EMBEDDING_SIZE, nbr_free_dims=get_nb_free_dims(cfg.MODEL.EMBEDDING_DIM_MODE),
                                             **vars(cfg.TRAINING.LOSSES.EMBEDDING))
    semseg_loss_criterion = SEMSEG_LOSS_REGISTRY[cfg.TRAINING.LOSSES.SEMSEG]() if m.semseg_head is not None else None
    return TrainingModel(
        backbone=m.backbone, embedding_head=m.embedding_head, embedding_head_feature_map_scale=e.SCALE,
        embedding_loss_criterion=embedding_loss_criterion, semseg_head=m.semseg_head, semseg_feature_map_scale=cfg.MODEL.SEMSEG.FEATURE_SCALE,
        semseg_loss_criterion=semseg_loss_criterion, seediness_head=m.seediness_head,
        seediness_head_feature_map_scale=cfg.MODEL.SEEDINESS.FEATURE_SCALE, multiclass_semseg_output=cfg.INPUT.NUM_CLASSES > 2,
        output_resize_scale=4.0 if cfg.TRAINING.LOSS_AT_FULL_RES else 1.0, logger=logger)
