"""The encoder's backward, composed on the binding's one-call ops (``hip``): the FPN's parameter gradients, one bottleneck block of the
body (plain, grouped, or with the stride in the 3x3), the recompute of a stage for its backward, the body's stages 4 .. freeze_at, and
the stem's weight gradient behind the max-pool.  What knows the network's structure lives here; every single convolution's gradient and
every streaming kernel is a function of ``hip`` (csrc/conv_backward.hip, csrc/bottleneck_backward.hip, csrc/stem_backward.hip).
``modeling/ops.py`` puts ``fpn_backward`` and ``body_backward`` behind autograd."""
import torch

from .. import hip

ENCODER_PLAN_SK_FLOATS = 32 << 20          # csrc/encoder.hip ENC_PLAN_SK_FLOATS: the split-K scratch a planned launch of the encoder counts on
_body_scratch = {}


def fpn_backward(C_views, L_halo_views, d_out, layer_weights, precision="bf16x6", want_dC=False, inner_weights=None):
    """Parameter gradients of the FPN (fpn.py:47-69) over F frames, levels k = 0..3 (4x .. 32x), each half the size of the one before:

        L_3 = inner_3(C_3),  L_k = inner_k(C_k) + up(L_{k+1}),  P_k = layer_k(L_k)          (up: bilinear x2, align_corners=False)

    C_views: the stage outputs, 4 views [Cin_k][F][h_k][w_k]; L_halo_views: the merged laterals, 4 y/x-zero-haloed views [Cf][F][h_k + 2]
    [w_k + 2]; d_out: the 4 upstream gradients dP_k [Cf, F, h_k, w_k]; layer_weights: the 4 ``fpn_layer`` weights [Cf, Cf, 3, 3].  For
    k = 0, 1, 2, 3:  d layer_k = wgrad9(L_k, dP_k);  G_k = dgrad9(dP_k, layer_k.weight) + up^T(G_{k-1});  d inner_k = wgrad1(C_k, G_k).
    -> (d_layer_w[4], d_layer_b[4], d_inner_w[4], d_inner_b[4]).  The gradient of C_k is not computed.  'bf16x6' or 'f32' (the data
    gradient's arithmetic; the weight gradients are fp32-input MFMA with fp64 across chunks in either).
    ``want_dC``: True, or the levels wanted -- additionally returns, as a fifth list, dC_k = inner_k^T G_k [Cin_k, F, h_k, w_k], the data
    gradient of the lateral 1x1 with respect to the stage output (``hip.conv1x1_dgrad`` on ``inner_weights[k]`` [Cf, Cin_k, 1, 1]; None at
    the levels not asked for): what the body's backward consumes.  The four lists are the same bits with or without it."""
    hip._backward_precision("fpn_backward", precision)
    dC_levels = () if not want_dC else ((0, 1, 2, 3) if want_dC is True else tuple(want_dC))
    if dC_levels and (inner_weights is None or len(inner_weights) != 4):
        raise ValueError("fpn_backward: want_dC needs inner_weights, the 4 lateral weights")
    for name, arg in (("C_views", C_views), ("L_halo_views", L_halo_views), ("d_out", d_out), ("layer_weights", layer_weights)):
        if len(arg) != 4:
            raise ValueError("fpn_backward: %s holds %d levels, expected 4" % (name, len(arg)))
    Cf, F = d_out[0].shape[0], d_out[0].shape[1]
    for k in range(4):
        g, w, c, l = d_out[k], layer_weights[k], C_views[k], L_halo_views[k]
        if g.dim() != 4 or g.shape[0] != Cf or g.shape[1] != F:
            raise ValueError("fpn_backward: d_out[%d] %s, expected [%d, %d, h, w]" % (k, tuple(g.shape), Cf, F))
        h, wd = g.shape[2], g.shape[3]
        if k and (2 * h, 2 * wd) != tuple(d_out[k - 1].shape[2:]):
            raise ValueError("fpn_backward: d_out[%d] %s is not half of level %d's %s" % (k, tuple(g.shape), k - 1, tuple(d_out[k - 1].shape)))
        if tuple(w.shape) != (Cf, Cf, 3, 3):
            raise ValueError("fpn_backward: layer_weights[%d] %s, expected %s" % (k, tuple(w.shape), (Cf, Cf, 3, 3)))
        if (c.T, c.H, c.W) != (F, h, wd):
            raise ValueError("fpn_backward: C_views[%d] (%d, %d, %d) against d_out[%d] %s" % (k, c.T, c.H, c.W, k, tuple(g.shape)))
        if (l.C, l.T, l.H, l.W) != (Cf, F, h + 2, wd + 2):
            raise ValueError("fpn_backward: L_halo_views[%d] [%d](%d, %d, %d) is not the haloed view of d_out[%d] %s" % (k, l.C, l.T, l.H, l.W, k, tuple(g.shape)))
    d_layer_w, d_layer_b, d_inner_w, d_inner_b, dC = [], [], [], [], []
    G = None
    for k in range(4):
        dP = d_out[k].detach().contiguous().float()
        dw, db = hip.conv2d_wgrad(L_halo_views[k], dP, 9)
        d_layer_w.append(dw)
        d_layer_b.append(db)
        G = hip.conv2d_dgrad(dP, layer_weights[k], precision, addend=None if G is None else hip.upsample_trilinear_backward(G, 1, 2, 2))
        dw, db = hip.conv2d_wgrad(C_views[k], G, 1)
        d_inner_w.append(dw)
        d_inner_b.append(db)
        if dC_levels:
            dC.append(hip.conv1x1_dgrad(G, inner_weights[k], precision) if k in dC_levels else None)
    if dC_levels:
        return d_layer_w, d_layer_b, d_inner_w, d_inner_b, dC
    return d_layer_w, d_layer_b, d_inner_w, d_inner_b


def bottleneck_backward(x_view, acts, G, weights, precision="bf16x6", want_dx=True, addend_x=None):
    """Backward of one bottleneck block with FrozenBN folded in (resnet.py:194-282):

        a1 = relu(conv1(x)),  a2 = relu(conv2(a1)),  out = relu(conv3(a2) + sc),   sc = down(xs) (projection block) or xs (identity block)
        g3 = relu'(out) G;  dW3 = wgrad1(a2, g3);  g_a2 = relu'(a2) dgrad1(g3, W3);  dW2 = wgrad9(a1, g_a2);  g_a1 = relu'(a1) dgrad9(g_a2, W2)
        dW1 = wgrad1(x, g_a1);  dWd = wgrad1(xs, g3);  g_x = dgrad1(g_a1, W1) + side

    G [Cout, F, h, w]: the gradient of out.  weights: dict(conv1, conv2, conv3, down -- the FOLDED weights [mid, Cin, 1, 1], [mid, mid /
    groups, 3, 3], [Cout, mid, 1, 1], [Cout, Cin, 1, 1] or None; optionally s1, s2, s3, sd -- the FrozenBN scales [Cout'] of each: the
    gradients returned are then those of the un-folded weights, dW[co] = s[co] dW_folded[co]; optionally ``groups`` and ``stride_in_3x3``).
    Cin, mid and Cout multiples of 32.  Two switches, both off by default:

      grouped (``groups`` > 1, or ``stride_in_3x3``): conv2's pair is ``hip.conv2d_grouped_wgrad`` / ``hip.conv2d_grouped_dgrad`` instead
        of ``hip.conv2d_wgrad(.., 9)`` / ``hip.conv2d_dgrad``.
      ``stride_in_3x3`` (the first block of a stage; a projection block): the block's stride 2 sits in conv2, so conv1 and a1 are at the
        stage input's resolution [2h, 2w]; xs = acts['xs2'] = subsample2(x); side = scatter2(dgrad1(g3, Wd), addend_x), so g_x [Cin, F, 2h,
        2w] is already at the lower stage's resolution and ``addend_x`` (the FPN's gradient of that stage's output) joins in the same pass.
        Without it the stride is already taken (x = xs, by ``subsample2`` before conv1) and side = dgrad1(g3, Wd), or g3 on an identity block.

    x_view: a view [Cin][F][H][W] of x; acts: dict(a1=(buffer, geometry) in the y/x-zero-haloed layout ``hip.alloc_padded2d``, a2, out dense
    tensors, xs2 dense with the stride in the 3x3).
    -> dict(conv1, conv2, conv3, down (None without a projection), g_x (None with want_dx=False: the first block of the lowest trainable
    stage; the weight gradients are the same bits)).  No bias gradient exists: the BN shift is a buffer.  'bf16x6' or 'f32'."""
    hip._backward_precision("bottleneck_backward", precision)
    groups, s3 = int(weights.get("groups", 1)), bool(weights.get("stride_in_3x3", False))
    grouped, stride = groups != 1 or s3, 2 if s3 else 1
    if addend_x is not None and not s3:
        raise ValueError("bottleneck_backward: addend_x joins the gradient of a stride-in-3x3 block only")
    w1, w2, w3, wd = weights["conv1"], weights["conv2"], weights["conv3"], weights.get("down")
    mid, Cin, Cout = w1.shape[0], w1.shape[1], w3.shape[0]
    for name, n in (("Cin", Cin), ("mid", mid), ("Cout", Cout)):
        if n % 32:
            raise ValueError("bottleneck_backward: %s = %d is no multiple of 32" % (name, n))
    Cg = hip._grouped_shape("bottleneck_backward", mid, groups, stride)
    if tuple(w2.shape) != (mid, Cg, 3, 3) or tuple(w3.shape) != (Cout, mid, 1, 1) or tuple(w1.shape[2:]) != (1, 1):
        raise ValueError("bottleneck_backward: conv1 %s, conv2 %s, conv3 %s are no bottleneck of %d groups" % (tuple(w1.shape), tuple(w2.shape), tuple(w3.shape), groups))
    if wd is None and (Cin != Cout or s3):
        raise ValueError("bottleneck_backward: an identity block needs Cin == Cout and no stride, got %d and %d%s" % (Cin, Cout, ", stride in the 3x3" if s3 else ""))
    if wd is not None and tuple(wd.shape) != (Cout, Cin, 1, 1):
        raise ValueError("bottleneck_backward: down %s, expected %s" % (tuple(wd.shape), (Cout, Cin, 1, 1)))
    if G.dim() != 4 or G.shape[0] != Cout:
        raise ValueError("bottleneck_backward: G %s, expected [%d, F, h, w]" % (tuple(G.shape), Cout))
    _, F, h, w = G.shape
    H, W = (2 * h, 2 * w) if s3 else (h, w)
    if (x_view.C, x_view.T, x_view.H, x_view.W) != (Cin, F, H, W):
        raise ValueError("bottleneck_backward: x_view [%d](%d, %d, %d) against G %s%s" % (x_view.C, x_view.T, x_view.H, x_view.W, tuple(G.shape),
                                                                                       " (stride in the 3x3: twice its map)" if s3 else ""))
    a1_buf, a1_g = acts["a1"]
    a2, out = acts["a2"], acts["out"]
    if tuple(a2.shape) != (mid, F, h, w) or tuple(out.shape) != (Cout, F, h, w) or a1_g != hip.padded2d_geometry(mid, F, H, W):
        raise ValueError("bottleneck_backward: acts do not have the block's shapes (a2 %s, out %s)" % (tuple(a2.shape), tuple(out.shape)))
    xs2 = acts.get("xs2") if s3 else None
    if s3 and (xs2 is None or tuple(xs2.shape) != (Cin, F, h, w)):
        raise ValueError("bottleneck_backward: a stride-in-3x3 block needs acts['xs2'] = subsample2(x) [%d, %d, %d, %d]" % (Cin, F, h, w))
    if addend_x is not None and tuple(addend_x.shape) != (Cin, F, H, W):
        raise ValueError("bottleneck_backward: addend_x %s, expected %s" % (tuple(addend_x.shape), (Cin, F, H, W)))
    G = G.detach().contiguous().float()
    g3 = hip.relu_backward(hip.dense_volume(out), G)
    res = dict(down=None, g_x=None)
    res["conv3"] = hip.conv2d_wgrad(hip.dense_volume(a2), g3, 1, want_db=False)[0]
    g_a2 = hip.conv1x1_dgrad(g3, w3, precision)
    hip.relu_backward(hip.dense_volume(a2), g_a2, out=g_a2)
    a1_halo, a1_mask = hip.padded2d_halo_view(a1_buf, a1_g, mid, F, H, W), hip.padded2d_interior_view(a1_buf, a1_g, mid, F, H, W)
    if grouped:
        res["conv2"] = hip.conv2d_grouped_wgrad(a1_halo, g_a2, groups, stride)
        g_a1 = hip.conv2d_grouped_dgrad(g_a2, w2, groups, stride, precision, mask=a1_mask)
    else:
        res["conv2"] = hip.conv2d_wgrad(a1_halo, g_a2, 9, want_db=False)[0]
        g_a1 = hip.conv2d_dgrad(g_a2, w2, precision, mask=a1_mask)
    res["conv1"] = hip.conv2d_wgrad(x_view, g_a1, 1, want_db=False)[0]
    if wd is not None:
        res["down"] = hip.conv2d_wgrad(hip.dense_volume(xs2) if s3 else x_view, g3, 1, want_db=False)[0]
    if want_dx:
        side = g3 if wd is None else hip.conv1x1_dgrad(g3, wd, precision)
        if s3:
            side = hip.scatter2(side, None if addend_x is None else addend_x.detach().contiguous().float())
        res["g_x"] = hip.conv1x1_dgrad(g_a1, w1, precision, addend=side)
    for name, key in (("conv1", "s1"), ("conv2", "s2"), ("conv3", "s3"), ("down", "sd")):
        if res[name] is not None and weights.get(key) is not None:
            hip.scale_rows(res[name], weights[key])
    return res


def body_stage_forward(x, blocks, precision, plan_frames=0):
    """The recompute of one stage of the body for its backward, in the three-launch block form of the encoder (csrc/encoder.hip) on
    ``hip.conv3d`` with (1, 1, 1) and (1, 3, 3): x [Cin, F, H, W] the stage's input (the previous stage's output), blocks: per block a dict
    with the PACKED weights of the pass and their biases, conv1 / conv2 / conv3 / down = (packed, bias) (down: the first block only), and
    ``stride`` (2: the first block of stages 2-4 reads ``subsample2(x)``; the stride is in the first 1x1).  precision: the pass's own;
    plan_frames: the pass's planning frame count (every launch decides its tile and split-K as the pass's did).
    A block dict may carry ``groups`` (default 1) and ``stride_in_3x3`` (default False); with either, conv2 = (the grouped packing, bias)
    runs on ``hip.conv2d_grouped``.  Stride in the 3x3 (the first block of a stage, which needs its projection): conv1 at the input's
    resolution, conv2 at stride 2, the shortcut on ``subsample2(x)``, which the stash then also holds as ``xs2``.
    -> the stash: per block dict(xs, a1=(haloed buffer, geometry), a2, out); xs of block b > 0 is block b - 1's out."""
    if precision not in hip.PRECISIONS:
        raise ValueError("body_stage_forward: precision %r" % (precision,))
    dev = x.device
    F = x.shape[1]
    scratch, plan = None, (0, 0, 0)
    if plan_frames > 0:
        n = ENCODER_PLAN_SK_FLOATS * max(1, -(-F // int(plan_frames)))
        scratch = _body_scratch.get(dev.index)
        if scratch is None or scratch.numel() < n:
            scratch = _body_scratch[dev.index] = torch.empty(n, dtype=torch.float32, device=dev)
        plan = (F, int(plan_frames), ENCODER_PLAN_SK_FLOATS)
    e = lambda **kw: dict(precision=precision, plan=plan, **kw)
    stash = []
    cur = x.contiguous()
    for b, blk in enumerate(blocks):
        groups, first = int(blk.get("groups", 1)), b == 0 and blk.get("stride", 1) == 2
        grouped = groups != 1 or bool(blk.get("stride_in_3x3", False))
        s3 = bool(blk.get("stride_in_3x3", False)) and first
        xs = hip.subsample2(cur) if (first and not s3) else cur
        Cin, _, H, W = xs.shape
        if s3 and (H % 2 or W % 2):
            raise ValueError("body_stage_forward: a stride-in-3x3 block needs an even input map, got %d x %d" % (H, W))
        if s3 and blk.get("down") is None:
            raise ValueError("body_stage_forward: a stride-in-3x3 block needs its projection shortcut")
        h, w = (H // 2, W // 2) if s3 else (H, W)
        V = F * h * w
        (p1, b1), (p2, b2), (p3, b3) = blk["conv1"], blk["conv2"], blk["conv3"]
        mid, Cout = b1.numel(), b3.numel()
        a1_buf, g = hip.alloc_padded2d(mid, F, H, W, dev)
        a2 = torch.empty(mid, F, h, w, dtype=torch.float32, device=dev)
        out = torch.empty(Cout, F, h, w, dtype=torch.float32, device=dev)
        hip.conv3d(hip.flat_volume(xs.view(Cin, F * H * W)), p1, b1, hip.padded2d_interior_view(a1_buf, g, mid, F, H, W), 1, splitk_scratch=scratch,
                   epilogue=e(relu=1, decode=(H, W)))
        a1_halo = hip.padded2d_halo_view(a1_buf, g, mid, F, H, W)
        if grouped:
            hip.conv2d_grouped(a1_halo, p2, b2, hip.dense_volume(a2), groups, 2 if s3 else 1, True, precision, plan_frames)
        else:
            hip.conv3d(a1_halo, p2, b2, hip.dense_volume(a2), (1, 3, 3), splitk_scratch=scratch, epilogue=e(relu=1))
        xs2 = hip.subsample2(cur) if s3 else xs
        idt = xs2
        if blk.get("down") is not None:
            idt = torch.empty(Cout, F, h, w, dtype=torch.float32, device=dev)
            hip.conv3d(hip.flat_volume(xs2.view(Cin, V)), blk["down"][0], blk["down"][1], hip.flat_volume(idt.view(Cout, V)), 1, splitk_scratch=scratch, epilogue=e())
        hip.conv3d(hip.flat_volume(a2.view(mid, V)), p3, b3, hip.flat_volume(out.view(Cout, V)), 1, splitk_scratch=scratch,
                   epilogue=e(relu=1, residual=idt, res_strides=(V, 0, 0)))
        stash.append(dict(xs=xs, a1=(a1_buf, g), a2=a2, out=out))
        if s3:
            stash[-1]["xs2"] = xs2
        cur = out
    return stash


def stem_backward(frames, stem_map, G_pooled, bn_scale=None):
    """Weight gradient of the stem (resnet.py:292-304: conv1 7x7 stride 2 -> FrozenBN -> ReLU -> max-pool 3x3 stride 2):

        g = relu'(stem_map) maxpool^T(G_pooled)   (one pass: ``hip.maxpool3x3s2_backward`` with ``mask_relu``);   dW = stem_wgrad(frames, g)

    frames [F, 3, H, W] as the pass read them; stem_map [64, F, H/2, W/2] the stem's output after its ReLU (the recompute's,
    ``ResNetFPN.stem_forward``); G_pooled [64, F, H/4, W/4] the gradient of the pooled map (layer1's g_x); bn_scale [64] | None: the
    FrozenBN scale, dW[co] *= s[co] (``hip.scale_rows``: the gradient of the un-folded weight).  -> dW [64, 3, 7, 7].  The frames get no
    gradient and the BN shift is a buffer."""
    if stem_map.dim() != 4 or stem_map.shape[0] != 64 or stem_map.shape[2] % 2 or stem_map.shape[3] % 2:
        raise ValueError("stem_backward: stem_map %s, expected [64, F, H/2, W/2] with even extents" % (tuple(stem_map.shape),))
    _, F, Ho, Wo = stem_map.shape
    if tuple(G_pooled.shape) != (64, F, Ho // 2, Wo // 2):
        raise ValueError("stem_backward: G_pooled %s, expected %s" % (tuple(G_pooled.shape), (64, F, Ho // 2, Wo // 2)))
    if tuple(frames.shape) != (F, 3, 2 * Ho, 2 * Wo):
        raise ValueError("stem_backward: frames %s, expected %s" % (tuple(frames.shape), (F, 3, 2 * Ho, 2 * Wo)))
    G = G_pooled.detach().contiguous().float()
    g, _ = hip.maxpool3x3s2_backward(stem_map.contiguous().view(64 * F, Ho, Wo), G.view(64 * F, Ho // 2, Wo // 2), mask_relu=True)
    dw = hip.stem_wgrad(frames.detach().contiguous().float(), g.view(64, F, Ho, Wo))
    if bn_scale is not None:
        hip.scale_rows(dw, bn_scale)
    return dw


def body_backward(stage_inputs, stages, dC, precision, freeze_at=2, plan_frames=0, dgrad_precision="f32", stem=None):
    """Weight gradients of the body's stages 4 .. ``freeze_at`` (2, 3 or 4; with ``stem`` also 1 or 0, below), one stage at a time: recompute the stage from its input
    (``body_stage_forward``: the fused forward leaves no per-block activations), run ``bottleneck_backward`` over its blocks last to first,
    free the stash, and hand the gradient down through ``hip.scatter2``, whose addend joins the FPN's dC of the level below.

    stage_inputs: {stage: the input of the stage [Cin, F, 2h, 2w] = the output of stage - 1}; stages: {stage: per block dict(conv1, conv2,
    conv3, down = (packed, bias) for the recompute; w1, w2, w3, wd = the folded weights; s1, s2, s3, sd = the FrozenBN scales or None;
    stride)}; dC: {stage: the gradient of the stage's output from the FPN lateral [Cout, F, h, w], or None}.  precision: the forward's
    ('f16x3' | 'bf16x6' | 'f32': the recompute's).  dgrad_precision: the arithmetic of the data gradients, 'f32' (the fp32-input MFMA) whatever
    the pass ran in: a gradient crosses three data-gradient convolutions per block, up to 13 (R-50) or 30 (R-101) blocks deep, and over
    such a chain the error of 'bf16x6' -- fp32-level on one convolution -- grew linearly with the depth instead of averaging out: the
    gradients of layer2 stood at 3 - 4 x the tests' bound (6.5e-6 of max|g|), with 'f32'
    at 0.65.
    -> {stage: per block dict(conv1, conv2, conv3, down)} for the stages freeze_at .. 4.  The first block of stage ``freeze_at`` computes no
    data gradient.
    A block dict may carry ``groups`` (default 1) and ``stride_in_3x3`` (default False), as in ``body_stage_forward``.  The gradient a
    stride-in-3x3 first block hands down is already at the lower stage's resolution: the FPN's dC of the level below joins inside that
    block, and nothing is scattered a second time.
    ``stem``: None, or a dict -- the stem path is on, and ``freeze_at`` may be 1 or 0 as well: stage 1 (layer1: a stride-1 projection block
    first, no ``subsample2``) is recomputed from ``stage_inputs[1]``, the recomputed pooled map, and stage 2's first block hands its gradient
    down as every stage does, joined with ``dC[1]``.  With 1 the first block of layer1 computes no data gradient.  With 0 it does, and
    ``stem_backward(stem['frames'], stem['stem_map'], that gradient, stem.get('bn_scale'))`` gives the result's entry 0, the stem's dW."""
    if freeze_at not in ((0, 1, 2, 3, 4) if stem is not None else (2, 3, 4)):
        raise NotImplementedError("body_backward: freeze_at = %r; stages below 2 need the backward of the max-pool and the stem "
                                  "(MODEL.BACKBONE.FREEZE_AT_STAGE >= 2)" % (freeze_at,))
    hip._backward_precision("body_backward", dgrad_precision)
    for key in ("frames", "stem_map") if freeze_at == 0 else ():
        if stem.get(key) is None:
            raise ValueError("body_backward: freeze_at 0 needs stem[%r]" % key)
    grads = {}
    G = None
    for st in (4, 3, 2, 1):
        if st < freeze_at:
            break
        blocks = stages[st]
        stash = body_stage_forward(stage_inputs[st], blocks, precision, plan_frames)
        if st == 4:
            G = dC.get(4)
            if G is None:
                G = torch.zeros_like(stash[-1]["out"])
        if tuple(G.shape) != tuple(stash[-1]["out"].shape):
            raise ValueError("body_backward: the gradient of stage %d's output %s against the output %s" % (st, tuple(G.shape), tuple(stash[-1]["out"].shape)))
        out = [None] * len(blocks)
        handed_down = "xs2" in stash[0]                    # a stride-in-3x3 first block: its g_x is the lower stage's gradient, dC joined
        for b in range(len(blocks) - 1, -1, -1):
            blk, s = blocks[b], stash[b]
            weights = dict(conv1=blk["w1"], conv2=blk["w2"], conv3=blk["w3"], down=blk.get("wd"), s1=blk.get("s1"), s2=blk.get("s2"), s3=blk.get("s3"),
                           sd=blk.get("sd"), groups=blk.get("groups", 1), stride_in_3x3="xs2" in s)
            kw = {}
            if "xs2" in s and st > freeze_at and dC.get(st - 1) is not None:
                kw["addend_x"] = dC[st - 1]                # (g_x is already at the lower stage's resolution: the FPN's dC joins here)
            r = bottleneck_backward(hip.dense_volume(s["xs"]), s, G, weights, dgrad_precision, want_dx=not (b == 0 and st == freeze_at), **kw)
            G = r.pop("g_x")
            out[b] = r
            stash[b] = None                                # (the block's activations are not needed again)
        grads[st] = out
        del stash
        if st > max(freeze_at, 1) and not handed_down:
            lower = dC.get(st - 1)
            if blocks[0].get("stride", 1) != 2:
                raise ValueError("body_backward: stage %d does not start with a stride-2 block" % st)
            G = hip.scatter2(G, lower.detach().contiguous().float() if lower is not None else None)
    if freeze_at == 0:
        grads[0] = stem_backward(stem["frames"], stem["stem_map"], G, stem.get("bn_scale"))
    return grads
