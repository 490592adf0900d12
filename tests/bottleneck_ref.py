"""Test helper: the stem and the bottleneck stages of the folded encoder (``ResNetFPN.folded_state()``) in float64 torch ops on the CPU,
keeping what the encoder's kernels leave in its workspace: every block's output and every block's conv1 output (resnet.py:262-304, one
group, stride in the 1x1).  No FPN: tests/resnext_ref.py has the whole network.  Plain test infrastructure, not a product path."""
import torch
import torch.nn.functional as F


@torch.no_grad()
def bottleneck_stages_f64(bb, images, folded=None):
    """bb: a ``ResNetFPN`` (its block list); images [N,3,H,W]; folded: ``bb.folded_state()`` taken elsewhere (e.g. from the device copy the
    kernels were packed from), default: taken here.  -> dict(stem=[N,64,H/4,W/4], block_out=[one [N,C,h,w] per block], conv1_out=[one
    [N,mid,h,w] per block], stage_out=[4 maps]), all float64."""
    f = {k: (w.detach().cpu().double(), b.detach().cpu().double()) for k, (w, b) in (folded or bb.folded_state()).items()}
    x = torch.as_tensor(images).detach().cpu().double()
    x = F.max_pool2d(F.relu(F.conv2d(x, *f["stem"], stride=2, padding=3)), kernel_size=3, stride=2, padding=1)
    out = dict(stem=x, block_out=[], conv1_out=[], stage_out=[])
    for i, blk in enumerate(bb.blocks()):
        assert blk.groups == 1 and not blk.stride_in_3x3
        z = F.relu(F.conv2d(x, *f["b%d.conv1" % i], stride=blk.stride))
        m = F.relu(F.conv2d(z, *f["b%d.conv2" % i], padding=1))
        idt = F.conv2d(x, *f["b%d.down" % i], stride=blk.stride) if blk.downsample is not None else x
        x = F.relu(F.conv2d(m, *f["b%d.conv3" % i]) + idt)
        out["conv1_out"].append(z)
        out["block_out"].append(x)
    i = 0
    for n in bb.stage_blocks:
        i += n
        out["stage_out"].append(out["block_out"][i - 1])
    return out
