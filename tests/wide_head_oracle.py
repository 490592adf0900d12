"""The wide composed decoder of the wide heads' tests and its oracle: tests/conv3d_backward_oracle.py's ``select_seed`` and
``decoder_gradients`` restated for a decoder ``make_decoder`` there does not build (it is fixed to two kinds) -- in = inter = 32 channels,
GroupNorm(8), 41 classes + the foreground channel: the 42 output channels of the YouTube-VIS semseg head.  Everything else is that
module's: ``decoder_forward``, ``decoder_conv_outputs``, ``features``, ``MAP_SIZES``, ``RELU_MARGIN``, ``SEEDS``."""
import torch
import torch.nn as nn

from tests import conv3d_backward_oracle as CO
from tests import decoder_tail_oracle as TO

NUM_CLASSES = 41
N_OUT = NUM_CLASSES + 1


def make_wide_decoder(T):
    from stemseg_amd.modeling.semseg_decoder import SqueezeExpandDecoder
    return SqueezeExpandDecoder(32, NUM_CLASSES, (32, 32, 32, 32), (4, 8, 16, 32), foreground_channel=True, PoolType=nn.AvgPool3d,
                                NormType=lambda c: nn.GroupNorm(8, c), num_frames=T)


def init_wide_decoder(T):
    """The constructor's initialisation under ``torch.manual_seed(11)``; the trunk is constructed before ``conv_out``, so its convolutions
    draw what the 3-class case of ``CO.init_decoder`` draws.  The GroupNorms' affine parameters there are drawn after ``conv_out``, whose
    size differs here: they are copied from that case, so that the whole trunk -- and every pre-ReLU map -- is the 3-class case's
    (tests/test_wide_head_host.py asserts it)."""
    small = CO.init_decoder("semseg", T)
    torch.manual_seed(11)
    m = make_wide_decoder(T)
    with torch.no_grad():
        for (n, mod), (n2, mod2) in zip(m.named_modules(), small.named_modules()):
            if isinstance(mod, nn.GroupNorm):
                assert n == n2
                mod.weight.copy_(mod2.weight)
                mod.bias.copy_(mod2.bias)
    return m


def _copy(m, T, dtype):
    t = make_wide_decoder(T).to(dtype)
    t.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    return t


def select_seed(T, m=None):
    """``CO.select_seed`` for the wide decoder: the first of CO.SEEDS whose features keep every pre-ReLU value of all seven stages at least
    CO.RELU_MARGIN from 0 in the fp64 oracle.  -> (seed, its margin, the margins of all seeds tried)."""
    t64 = _copy(init_wide_decoder(T) if m is None else m, T, torch.float64)
    G = t64.gn_groups
    tried = []
    with torch.no_grad():
        for seed in CO.SEEDS:
            convouts, pre = CO.decoder_conv_outputs(t64, CO.features(T, seed), torch.float64)
            for D, (blk, idx), pool in zip(convouts, t64._LAST_STAGE, CO.last_stage_pools(t64)):
                gn = getattr(t64, blk)[idx + 1]
                pre.append(TO.gn_forward(D, gn.weight, gn.bias, G, pool, t64.gn_eps or TO.GN_EPS)[0])
            tried.append(min(float(p.abs().min()) for p in pre))
            if tried[-1] >= CO.RELU_MARGIN:
                return seed, tried[-1], tried
    raise AssertionError("no seed of %r keeps the pre-ReLU values %g away from 0: %s" % (CO.SEEDS, CO.RELU_MARGIN, tried))


def decoder_gradients(m, T, feats, up, dtype, rounded=False):
    """({parameter name: gradient as float64 numpy} of sum(out * up), out as float64 numpy) for the wide decoder with m's weights in
    ``dtype``: raw logits, no activation, no grid."""
    trunk = _copy(m, T, dtype)
    out, _ = CO.decoder_forward(trunk, feats, [0] * N_OUT, [0] * N_OUT, (None, None, None), dtype, rounded)
    out.backward(up.to(dtype))
    return {n: p.grad.detach().double().numpy() for n, p in trunk.named_parameters() if p.grad is not None}, out.detach().double().numpy()
