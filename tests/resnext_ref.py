"""Test helper: the folded encoder (``ResNetFPN.folded_state()``, every FrozenBN folded into its conv) restated in float64 torch ops,
with grouped / strided conv2 -- the check that ``ResNetFPN``'s folding and its architecture knobs (NUM_GROUPS, WIDTH_PER_GROUP,
STRIDE_IN_1X1) describe the reference's network (resnet.py:194-304, fpn.py:47-69).  Plain test infrastructure, not a product path."""
import torch
import torch.nn.functional as F


@torch.no_grad()
def folded_resnet_fpn_f64(bb, images):
    """bb: a ``ResNetFPN``; images [N,3,H,W] -> {4, 8, 16, 32: float64 [N,256,H/s,W/s]}."""
    f = {k: (w.double(), b.double()) for k, (w, b) in bb.folded_state().items()}
    x = torch.as_tensor(images).double()
    w, b = f["stem"]
    x = F.max_pool2d(F.relu(F.conv2d(x, w, b, stride=2, padding=3)), kernel_size=3, stride=2, padding=1)
    feats, i = [], 0
    for li in (1, 2, 3, 4):
        for blk in getattr(bb.body, "layer%d" % li):
            s1, s3 = (1, blk.stride) if blk.stride_in_3x3 else (blk.stride, 1)
            out = F.relu(F.conv2d(x, *f["b%d.conv1" % i], stride=s1))
            out = F.relu(F.conv2d(out, *f["b%d.conv2" % i], stride=s3, padding=1, groups=blk.groups))
            out = F.conv2d(out, *f["b%d.conv3" % i])
            idt = F.conv2d(x, *f["b%d.down" % i], stride=blk.stride) if blk.downsample is not None else x
            x = F.relu(out + idt)
            i += 1
        feats.append(x)
    last = F.conv2d(feats[3], *f["fpn_inner4"])
    outs = {32: F.conv2d(last, *f["fpn_layer4"], padding=1)}
    for k, scale in ((3, 16), (2, 8), (1, 4)):
        top = F.interpolate(last, scale_factor=2, mode="bilinear", align_corners=False)
        last = F.conv2d(feats[k - 1], *f["fpn_inner%d" % k]) + top
        outs[scale] = F.conv2d(last, *f["fpn_layer%d" % k], padding=1)
    return outs
