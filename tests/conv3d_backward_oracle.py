"""The oracle of the 3x3x3 convolution backward and of the decoder-training tests: torch on the CPU with autograd, in the dtype asked for
(the tests run it in fp32 and in fp64 on the same input; the fp32-versus-fp64 spread of a case is the yardstick its device error is held
to -- tests/decoder_tail_oracle.py, whose ``check`` / ``bound`` / ``max_norm_err`` these tests use).  ``F.conv3d`` for the convolution;
the whole reference decoder -- conv -> GroupNorm -> ReLU -> (avg pool) per stage, up-sampling, concat, conv_16 / conv_8 / conv_4, heads,
activations (embedding_decoder.py:20-143) -- from stock ops, optionally with every convolution operand rounded to the 22-bit significand
the f16x3 mode keeps (tests/test_f16x3_arithmetic.py: two fp16 terms)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import decoder_tail_oracle as TO

# ------------------------------------------------------------------------------------------------ one convolution
WGRAD_CHANNELS = ((4, 32), (32, 32), (64, 32), (32, 96))       # (Cin, Cout)
DGRAD_CHANNELS = tuple(c for c in WGRAD_CHANNELS if c[0] % 32 == 0)
CONV_T = (1, 2, 3, 5)
CONV_HW = ((1, 2), (3, 5), (6, 10), (8, 16))
# the smallest enlargement of the 8 x 16 map (T = 5, rows added) that the chunk rule cuts into >= 3 chunks with a short last one: tiles of
# 4 rows x 16 columns, 8 tiles to a chunk -- 12 rows are 15 tiles (2 chunks), 13 rows are 20 tiles: 8 + 8 + 4
CHUNKED_SHAPE = (32, 32, 5, 13, 16)                            # (Cin, Cout, T, H, W)
# the tile shapes the small maps above do not reach -- 2 rows x 32 columns (16 < W <= 32), 1 row x 64 columns (W > 32), several tiles along x
# with a ragged last one -- a second, partly filled tile of input channels (36 = 32 + 4) and of output channels (160 = 128 + 32)
WIDE_SHAPES = ((36, 32, 1, 5, 20), (32, 160, 2, 3, 70), (32, 32, 1, 2, 130))       # (Cin, Cout, T, H, W)
CORNERS_AND_INTERIOR = lambda T, H, W: sorted({(t, y, x) for t in (0, T - 1) for y in (0, H - 1) for x in (0, W - 1)} | {(T // 2, H // 2, W // 2)})


def conv_case(Cin, Cout, T, H, W, seed=0):
    rng = np.random.default_rng(100003 * Cin + 1009 * Cout + 101 * T + 11 * H + W + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    g = f(Cout, T, H, W)
    g[rng.random(g.shape) < 0.1] = 0.0
    return dict(x=f(Cin, T, H, W), w=(f(Cout, Cin, 3, 3, 3) / np.sqrt(27 * Cin)).astype(np.float32), b=(0.1 * f(Cout)).astype(np.float32), g=g)


def conv_oracle(case, dtype):
    """-> dict(out, dx, dw, db) as float64 numpy: F.conv3d(padding=1) and its autograd in ``dtype``."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
    x, w, b = t(case["x"]), t(case["w"]), t(case["b"])
    out = F.conv3d(x[None], w, b, padding=1)[0]
    out.backward(torch.from_numpy(case["g"]).to(dtype))
    n = lambda a: a.detach().double().numpy()
    return dict(out=n(out), dx=n(x.grad), dw=n(w.grad), db=n(b.grad))


def flipped_transposed(w):
    """W'[ci][co][kt][ky][kx] = W[co][ci][2 - kt][2 - ky][2 - kx]: conv3d(dy, W', padding=1) is the data gradient."""
    return w.flip(2, 3, 4).transpose(0, 1).contiguous()


def neighbourhood(x, t, y, xx):
    """The 3 x 3 x 3 neighbourhood of voxel (t, y, xx) in x [Cin, T, H, W], zeros outside the volume: [Cin, 3, 3, 3]."""
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (1, 1)))[:, t:t + 3, y:y + 3, xx:xx + 3]


# ------------------------------------------------------------------------------------------------ the whole decoder
class _Round22(torch.autograd.Function):
    """hi + lo with hi = fp16(v / s) and lo = fp16(v / s - hi), s the power of two that brings the tensor's largest magnitude to [2^13,
    2^14): 22 significand bits, as the f16x3 operand pair; the gradient passes straight through."""

    @staticmethod
    def forward(ctx, v):
        m = float(v.abs().max())
        s = 2.0 ** (np.floor(np.log2(m)) - 13) if m > 0 else 1.0
        u = v / s
        hi = u.to(torch.float16).to(v.dtype)
        lo = (u - hi).to(torch.float16).to(v.dtype)
        return (hi + lo) * s

    @staticmethod
    def backward(ctx, g):
        return g


def round22(v):
    return _Round22.apply(v)


def make_decoder(kind, T):
    """The decoders of the composed tests: in = inter = 32 channels, GroupNorm(8); 'embedding' = 'xyff' with tanh and the seediness output
    (7 channels), 'semseg' = 3 classes + the foreground channel."""
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder
    from stemseg_amd.modeling.semseg_decoder import SqueezeExpandDecoder
    norm = lambda c: nn.GroupNorm(8, c)
    if kind == "embedding":
        return SqueezingExpandDecoder(32, (32, 32, 32, 32), 4, tanh_activation=True, seediness_output=True, experimental_dims="xyff",
                                      PoolType=nn.AvgPool3d, NormType=norm, num_frames=T)
    return SqueezeExpandDecoder(32, 3, (32, 32, 32, 32), (4, 8, 16, 32), foreground_channel=True, PoolType=nn.AvgPool3d, NormType=norm, num_frames=T)


def init_decoder(kind, T):
    """A decoder with fixed weights: the constructors' initialisation under a fixed seed, every GroupNorm's affine parameters and the
    variance bias moved off their trivial values."""
    torch.manual_seed(11)
    m = make_decoder(kind, T)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.GroupNorm):
                mod.weight.copy_(1.0 + 0.3 * torch.randn(mod.num_channels))
                mod.bias.copy_(0.2 * torch.randn(mod.num_channels))
        if kind == "embedding":
            m.conv_variance.bias.copy_(0.1 * torch.randn(2))
    return m


MAP_SIZES = ((1, 2), (2, 4), (4, 8), (8, 16))                  # 32x .. 4x
RELU_MARGIN = 2e-5                                             # no pre-ReLU value of any of the seven stages lies closer to 0 in the fp64 oracle
SEEDS = range(16)


def features(T, seed):
    g = torch.Generator().manual_seed(100 * T + seed)
    return [torch.randn(32, T, h, w, generator=g) for h, w in MAP_SIZES]


def decoder_conv_outputs(trunk, feats, dtype, rounded=False):
    """The seven 3x3x3 stages of the reference decoder on one sample in ``dtype``: trunk a CPU copy of the decoder in that dtype (its live
    parameters receive the gradients), feats the four feature maps (32x .. 4x).  rounded: every convolution sees its two operands through
    ``round22``.  -> (the last conv output of each branch, the pre-ReLU maps of the stages before them)."""
    from stemseg_amd.modeling.decoder_base import _BLOCK_CONVS
    r = round22 if rounded else (lambda v: v)
    flags = list(trunk.pool_flags)
    G = trunk.gn_groups
    convouts, pre = [], []
    for x, stages, pools in zip(feats, trunk._BRANCH_STAGES, (flags, flags[:2], flags[:1], [0])):
        x = x.to(dtype)
        for k, (si, pool) in enumerate(zip(stages, pools)):
            blk, idx = _BLOCK_CONVS[si]
            conv, gn = getattr(trunk, blk)[idx], getattr(trunk, blk)[idx + 1]
            D = F.conv3d(r(x)[None], r(conv.weight), conv.bias, padding=1)[0]
            if k == len(stages) - 1:
                convouts.append(D)
            else:
                y, x = TO.gn_forward(D, gn.weight if G else None, gn.bias if G else None, G, pool, trunk.gn_eps or TO.GN_EPS)
                pre.append(y)
    return convouts, pre


def last_stage_pools(trunk):
    return [trunk.pool_flags[2], trunk.pool_flags[1], trunk.pool_flags[0], 0]


def decoder_forward(trunk, feats, act, axes, grids, dtype, rounded=False):
    """The whole reference decoder: the stages above, then tests/decoder_tail_oracle.py's unfolded tail with the heads' activation tables
    (act, axes, grids as the device module holds them).  -> (output [n_out, T, H4, W4], the pre-ReLU maps of all seven stages)."""
    convouts, pre = decoder_conv_outputs(trunk, feats, dtype, rounded)
    out, pre_last = TO.unfolded_tail(trunk, convouts, act, axes, grids, trunk.t_scales, last_stage_pools(trunk), dtype)
    return out, pre + pre_last


def select_seed(kind, T, m=None):
    """The first of SEEDS whose features keep every pre-ReLU value of all seven stages at least RELU_MARGIN from 0 in the fp64 oracle.
    (The heads' activations play no part in it.)  -> (seed, its margin, the margins of all seeds tried)."""
    m = init_decoder(kind, T) if m is None else m
    t64 = make_decoder(kind, T).double()
    t64.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    G = t64.gn_groups
    tried = []
    with torch.no_grad():
        for seed in SEEDS:
            convouts, pre = decoder_conv_outputs(t64, features(T, seed), torch.float64)
            for D, (blk, idx), pool in zip(convouts, t64._LAST_STAGE, last_stage_pools(t64)):
                gn = getattr(t64, blk)[idx + 1]
                pre.append(TO.gn_forward(D, gn.weight if G else None, gn.bias if G else None, G, pool, t64.gn_eps or TO.GN_EPS)[0])
            tried.append(min(float(p.abs().min()) for p in pre))
            if tried[-1] >= RELU_MARGIN:
                return seed, tried[-1], tried
    raise AssertionError("no seed of %r keeps the pre-ReLU values %g away from 0: %s" % (SEEDS, RELU_MARGIN, tried))


def decoder_gradients(m, kind, T, feats, up, act, axes, grids, dtype, rounded=False):
    """{parameter name: gradient as float64 numpy} of sum(out * up) for the decoder with m's weights, evaluated in ``dtype``."""
    trunk = make_decoder(kind, T).to(dtype)
    trunk.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    out, _ = decoder_forward(trunk, feats, act, axes, grids, dtype, rounded)
    out.backward(up.to(dtype))
    return {n: p.grad.detach().double().numpy() for n, p in trunk.named_parameters() if p.grad is not None}, out.detach().double().numpy()
