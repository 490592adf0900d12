"""The oracle of the stem backward tests: the max-pool backward's window rule restated in numpy, and torch on the CPU with autograd --
``F.max_pool2d`` and ``F.conv2d(stride=2, padding=3)`` -- in the dtype asked for.  Gradients are held to the rule of
tests/decoder_tail_oracle.py (``check`` / ``bound``: the device may be FACTOR = 4 times a case's own fp32-vs-fp64 spread away from the fp64
result); the pool backward is compared bit for bit.  The composed oracle is linearised around the device's recomputed activations, as
tests/body_backward_oracle.py does (``given``), so the ReLU masks and the arg-max positions are the device's."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import body_backward_oracle as BO
from tests import resnext_backward_oracle as RO


# ------------------------------------------------------------------------------------------------ the max-pool backward
def pool_backward_rule(x, g, mask_relu=False):
    """dx of ``max_pool2d(x, 3, 2, 1)`` by the rule the kernel states: per window, rows then columns of the window clipped to the map, the
    running value starts as the first element and a value replaces it when it is greater or a NaN; g is added at the arg-max, the windows in
    ascending (oy, ox) order, in fp32 from +0.  mask_relu: then 0 where x <= 0 (+-0.0 and negatives blocked, NaN lets through)."""
    x, g = np.asarray(x, np.float32), np.asarray(g, np.float32)
    planes, H, W = x.shape
    dx = np.zeros_like(x)
    with np.errstate(invalid="ignore"):
        for p in range(planes):
            for oy in range(H // 2):
                for ox in range(W // 2):
                    y0, y1, x0, x1 = max(2 * oy - 1, 0), min(2 * oy + 1, H - 1), max(2 * ox - 1, 0), min(2 * ox + 1, W - 1)
                    by, bx, best = y0, x0, x[p, y0, x0]
                    for yy in range(y0, y1 + 1):
                        for xx in range(x0, x1 + 1):
                            v = x[p, yy, xx]
                            if v > best or v != v:
                                by, bx, best = yy, xx, v
                    dx[p, by, bx] = np.float32(dx[p, by, bx] + g[p, oy, ox])
        if mask_relu:
            dx = np.where(x <= 0, np.float32(0), dx)
    return dx


def pool_backward_torch(x, g, mask_relu=False):
    """The same by torch's CPU backward (and ``threshold_backward`` for the mask), fp32."""
    xt = torch.from_numpy(np.asarray(x, np.float32))[None].clone().requires_grad_(True)
    F.max_pool2d(xt, 3, 2, 1).backward(torch.from_numpy(np.asarray(g, np.float32))[None])
    dx = xt.grad[0]
    if mask_relu:
        dx = torch.ops.aten.threshold_backward(dx, xt.detach()[0], 0)
    return dx


def bits(a):
    a = a.detach().cpu().contiguous() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return a.view(torch.int32)


# ------------------------------------------------------------------------------------------------ the stem's weight gradient
def wgrad_oracle(frames, g, dtype, w=None):
    """dw [64, 3, 7, 7] as float64 numpy of <g, conv2d(frames; w, stride 2, padding 3)> by autograd in ``dtype`` (g channel-major)."""
    wt = (torch.zeros(64, 3, 7, 7) if w is None else torch.from_numpy(np.asarray(w))).to(dtype).requires_grad_(True)
    out = F.conv2d(torch.from_numpy(np.asarray(frames)).to(dtype), wt, stride=2, padding=3)
    out.backward(torch.from_numpy(np.asarray(g)).to(dtype).permute(1, 0, 2, 3))
    return wt.grad.double().numpy()


def stem_patch(frames, f, oy, ox):
    """The 3 x 7 x 7 patch of frame f under output pixel (oy, ox), zero outside the frame: dw[co] of a one-hot upstream."""
    padded = np.pad(np.asarray(frames)[f], ((0, 0), (3, 3), (3, 3)))
    return padded[:, 2 * oy:2 * oy + 7, 2 * ox:2 * ox + 7]


# ------------------------------------------------------------------------------------------------ the stem and the body behind it
def stem_forward(frames, live, dtype, given=None):
    """frames [F, 3, H, W] in ``dtype``; live: dict(w, s, b) of the stem.  -> (the stem's map after its ReLU -- the device's value and mask when
    ``given`` (channel-major) --, the pooled map), frames first."""
    lin = F.conv2d(frames, live["w"], stride=2, padding=3) * live["s"].view(1, -1, 1, 1) + live["b"].view(1, -1, 1, 1)
    stem = BO._given(lin, given, dtype)
    return stem, F.max_pool2d(stem, 3, 2, 1)


def body_forward(x, live_stages, dtype, given=None, stage_in=None, groups=1):
    """``BO.body_forward`` from layer1 on: the first stage's first block has stride 1, the others' stride 2 (in the first 1x1).  x [F, 64, h, w]
    frames first; stage_in: per stage the VALUE its input takes (channel-major) or None.  -> per stage the output, frames first."""
    outs = []
    for k, blocks in enumerate(live_stages):
        if stage_in is not None and stage_in[k] is not None:
            v = BO.frames_first(torch.as_tensor(stage_in[k])).to(dtype)
            x = x + (v - x).detach()
        for b, live in enumerate(blocks):
            _, _, x = RO.block_forward(x, live, 2 if (b == 0 and k > 0) else 1, dtype, None if given is None else given[k][b], groups)
        outs.append(x)
    return outs


def stem_body_gradients(case, dtype, given_stem, given, freeze_at):
    """{'stem' | (stage index, block, conv): gradient as float64 numpy} of sum_k <C_k, g_k> over the four stage outputs of
    ``stem_backward_cases.stem_body_case``, the stem's weight included when ``freeze_at`` is 0."""
    live = [[BO.live_params(p, dtype) for p in blocks] for blocks in case["stages"]]
    stem = {n: torch.from_numpy(v).to(dtype) for n, v in case["stem"].items()}
    stem["w"].requires_grad_(freeze_at == 0)
    _, pooled = stem_forward(torch.from_numpy(case["frames"]).to(dtype), stem, dtype, given_stem)
    outs = body_forward(pooled, live, dtype, given, groups=case["groups"])
    sum((o * BO.frames_first(torch.from_numpy(g)).to(dtype)).sum() for o, g in zip(outs, case["g"])).backward()
    grads = {}
    if freeze_at == 0:
        grads["stem"] = stem["w"].grad.double().numpy()
    for k, blocks in enumerate(live):
        for b, lp in enumerate(blocks):
            for c in BO.CONVS:
                if c in lp:
                    grads[(k, b, c)] = lp[c].grad.detach().double().numpy()
    return grads
