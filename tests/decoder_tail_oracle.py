"""The oracle of the decoder-tail backward tests: torch on the CPU with autograd, in the dtype asked for (the tests run it in fp32 and in
fp64 on the same input: the fp32-versus-fp64 spread of a case is the yardstick its device error is held to).  Stock ops only:
``F.group_norm``, ``relu``, ``avg_pool3d``, ``F.interpolate(mode='trilinear')``, 1x1x1 convolutions as matrix products, the heads'
activations; plus the case builders the host and the GPU tests share."""
import numpy as np
import torch
import torch.nn.functional as F

FACTOR = 4                     # the device may be this many times a case's own fp32-vs-fp64 spread away from the fp64 result
FP32_ROUNDING = 2.0 ** -24     # rounding a result to fp32 alone: the least spread a case is credited with
RELU_MARGIN = 1e-4             # no pre-ReLU value of a GroupNorm case lies closer to 0 (its sign decides a whole gradient term)


def max_norm_err(g, ref):
    """max |g - ref| / max |ref| (max |g| when the reference is all zero)."""
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    m = np.abs(ref).max() if ref.size else 0.0
    return float(np.abs(g - ref).max() / m) if m else float(np.abs(g).max() if g.size else 0.0)


def bound(spread, ref):
    """FACTOR x the case's spread, floored at fp32 rounding; 0 for a term that is exactly zero in the oracle."""
    return 0.0 if not np.abs(np.asarray(ref)).max() else FACTOR * max(spread, FP32_ROUNDING)


def check(name, what, dev, r32, r64, bad):
    """Prints spread, bound and device error of one result; appends to ``bad`` when the device misses the bound."""
    spread, err = max_norm_err(r32, r64), max_norm_err(dev, r64)
    b = bound(spread, r64)
    print("%s %-8s spread %.2e bound %.2e device %.2e" % (name, what, spread, b, err))
    if not err <= b:
        bad.append((name, what, err, b))
    return spread, b, err


# ------------------------------------------------------------------------------------------------ heads
HEAD_TABLES = {1: ([2], [0]), 4: ([1, 2, 3, 4], [3, 0, 0, 2]), 10: ([1, 1, 1, 2, 3, 4, 4, 4, 0, 0], [1, 2, 3, 0, 0, 1, 2, 3, 0, 0])}
HEAD_DIMS = ((2, 5, 7), (1, 1, 4099))          # V = 70: no multiple of 4 or 64; V = 4099: several workgroups, a ragged last one
HEAD_CIN = (4, 64, 256)


def heads_case(Cin, n_out, dims, seed=0):
    T, H, W = dims
    rng = np.random.default_rng(1000 * Cin + 10 * n_out + T + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    act, axis = HEAD_TABLES[n_out]
    g = f(n_out, T, H, W)
    g[rng.random(g.shape) < 0.1] = 0.0
    return dict(x=f(Cin, T, H, W), w=(f(n_out, Cin) / np.sqrt(Cin)).astype(np.float32), b=(f(n_out) * 0.1).astype(np.float32), act=act, axis=axis, g=g,
                gt=np.linspace(-1, 1, T, dtype=np.float32), gy=np.linspace(-1.5, 1.5, H, dtype=np.float32),
                gx=np.linspace(-2, 2, W, dtype=np.float32))


def activate(z, act, axis, gt, gy, gx):
    """csrc/heads.hip head_act per channel on z [n_out, T, H, W]."""
    grids = {1: gt[:, None, None], 2: gy[None, :, None], 3: gx[None, None, :]}
    outs = []
    for o, (a, ax) in enumerate(zip(act, axis)):
        zo = z[o]
        grid = grids[ax] if (a in (1, 4) and ax) else 0.0
        zo = torch.tanh(0.25 * zo) if a == 1 else torch.sigmoid(zo) if a == 2 else torch.exp(zo) * 10.0 if a == 3 else zo
        outs.append(zo + grid)
    return torch.stack(outs, 0)


def heads_oracle(case, dtype, with_act=True):
    """-> dict(out, dx, dw, db) as float64 numpy; with_act False: the linear level matrix (no bias, no activation; g is dz)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    x, w, b = t(case["x"]).requires_grad_(True), t(case["w"]).requires_grad_(True), t(case["b"]).requires_grad_(True)
    z = torch.einsum("oc,cthw->othw", w, x)
    if with_act:
        out = activate(z + b[:, None, None, None], case["act"], case["axis"], t(case["gt"]), t(case["gy"]), t(case["gx"]))
    else:
        out = z
    out.backward(t(case["g"]))
    n = lambda a: a.detach().double().numpy()
    return dict(out=n(out), dx=n(x.grad), dw=n(w.grad), db=n(b.grad) if with_act else None)


# ------------------------------------------------------------------------------------------------ trilinear
UP_SCALES = ((1, 2, 2), (2, 2, 2), (1, 4, 4))


def up_case(scale, T, H, W, C=3):
    rng = np.random.default_rng(100000 * scale[0] + 10000 * scale[1] + 1000 * T + 10 * H + W)
    return rng.standard_normal((C, T, H, W)).astype(np.float32), \
        rng.standard_normal((C, T * scale[0], H * scale[1], W * scale[2])).astype(np.float32)


def up_oracle(x, g, scale, dtype):
    xx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = F.interpolate(xx[None], scale_factor=tuple(float(s) for s in scale), mode="trilinear", align_corners=False)[0]
    out.backward(torch.from_numpy(g).to(dtype))
    return out.detach().double().numpy(), xx.grad.double().numpy()


# ------------------------------------------------------------------------------------------------ GroupNorm + ReLU + pool
GN_CG = ((8, 2), (32, 32), (32, 8), (8, 0))
GN_HW = ((3, 5), (6, 10), (4, 8))              # (4, 8): W % 4 == 0, the kernels' 16-byte path
GN_T = (1, 2, 3, 4, 5)
GN_EPS = 1e-5


def gn_forward(x, gamma, beta, groups, pool, eps=GN_EPS):
    """-> (pre-ReLU y, output) of GroupNorm -> ReLU -> (AvgPool3d(3, (2, 1, 1), 1)) on x [C, T, H, W]; groups 0: no normalisation."""
    y = F.group_norm(x[None], groups, gamma, beta, eps)[0] if groups else x
    out = F.relu(y)
    if pool:
        # (padding=1, count_include_pad, written as explicit zero padding: avg_pool3d itself refuses T = 1 against a kernel of 3)
        out = F.avg_pool3d(F.pad(out[None], (1, 1, 1, 1, 1, 1)), 3, stride=(2, 1, 1), padding=0)[0]
    return y, out


def gn_case(C, groups, T, H, W, pool):
    """x, gamma, beta, upstream g (with zeros and negatives) such that no pre-ReLU value lies within RELU_MARGIN of 0 in fp64: the
    first seed of a fixed sequence that gives it."""
    To = (T + 1) // 2 if pool else T
    for k in range(200):
        rng = np.random.default_rng(7919 * k + 1000 * C + 100 * groups + 10 * T + H + pool)
        x = (rng.standard_normal((C, T, H, W)) * 1.5 + 0.3).astype(np.float32)
        gamma = (1.0 + 0.5 * rng.standard_normal(C)).astype(np.float32)
        beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
        g = rng.standard_normal((C, To, H, W)).astype(np.float32)
        g[rng.random(g.shape) < 0.15] = 0.0
        t = lambda a: torch.from_numpy(a).double()
        y, _ = gn_forward(t(x), t(gamma), t(beta), groups, pool)
        if float(y.abs().min()) >= RELU_MARGIN:
            return dict(x=x, gamma=gamma, beta=beta, g=g, groups=groups, pool=pool, min_abs_y=float(y.abs().min()))
    raise AssertionError("no seed keeps the pre-ReLU values away from 0")


def gn_oracle(case, dtype):
    t = lambda a: torch.from_numpy(a).to(dtype)
    x, gamma, beta = t(case["x"]).requires_grad_(True), t(case["gamma"]).requires_grad_(True), t(case["beta"]).requires_grad_(True)
    _, out = gn_forward(x, gamma, beta, case["groups"], case["pool"])
    out.backward(t(case["g"]))
    n = lambda a: a.detach().double().numpy()
    if not case["groups"]:
        return dict(out=n(out), dx=n(x.grad))
    return dict(out=n(out), dx=n(x.grad), dgamma=n(gamma.grad), dbeta=n(beta.grad))


def gn_stats(x, groups, eps=GN_EPS):
    """(mean, rstd) per group from fp64, as fp32 [2 groups]: what the forward's statistics kernels hand to the backward."""
    xg = torch.from_numpy(x).double().reshape(groups, -1)
    return torch.stack([xg.mean(1), 1.0 / torch.sqrt(xg.var(1, unbiased=False) + eps)], 1).reshape(-1).float()


# ------------------------------------------------------------------------------------------------ the composed tail
def unfolded_tail(trunk, convouts, act, axes, grids, t_scales, pools, dtype):
    """The reference decoder from the last conv output of each branch on, step by step (embedding_decoder.py:64-80,112-143) in ``dtype``:
    GroupNorm -> ReLU -> (pool) per branch, up-sample, concat, conv_16 / conv_8 / conv_4, the heads with their activations.
    ``trunk``: a CPU copy of the decoder in ``dtype`` (its live parameters: they receive the gradients); convouts: the four last conv
    outputs (32x .. 4x) as leaf tensors.  -> (output [n_out, T, H4, W4], the pre-ReLU maps)."""
    ys, pre = [], []
    for D, (blk, idx), pool in zip(convouts, trunk._LAST_STAGE, pools):
        gn = getattr(trunk, blk)[idx + 1]
        y, out = gn_forward(D, gn.weight if trunk.gn_groups else None, gn.bias if trunk.gn_groups else None, trunk.gn_groups, pool,
                            trunk.gn_eps or GN_EPS)
        ys.append(out)
        pre.append(y)
    up = lambda v, ts: F.interpolate(v[None], scale_factor=(float(ts), 2.0, 2.0), mode="trilinear", align_corners=False)[0]
    mix = lambda conv, v: torch.einsum("oc,cthw->othw", conv.weight.reshape(conv.out_channels, -1), v)
    x = up(ys[0], t_scales[0])
    x = mix(trunk.conv_16, torch.cat((x, ys[1]), 0))
    x = up(x, t_scales[1])
    x = mix(trunk.conv_8, torch.cat((x, ys[2]), 0))
    x = up(x, t_scales[2])
    x = mix(trunk.conv_4, torch.cat((x, ys[3]), 0))
    zs = []
    for conv in trunk._head_convs():
        z = mix(conv, x)
        zs.append(z + conv.bias[:, None, None, None] if conv.bias is not None else z)
    gt, gy, gx = grids if grids[0] is not None else (torch.zeros(1, dtype=dtype),) * 3
    return activate(torch.cat(zs, 0), act, axes, gt.to(dtype), gy.to(dtype), gx.to(dtype)), pre
