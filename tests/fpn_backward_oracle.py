"""The oracle of the FPN backward tests: torch on the CPU with autograd, in the dtype asked for (the tests run it in fp32 and in fp64 on the
same input; the fp32-versus-fp64 spread of a case is the yardstick its device error is held to -- tests/decoder_tail_oracle.py, whose
``check`` / ``bound`` / ``max_norm_err`` these tests use).  ``F.conv2d`` for the 3x3 (padding 1) and the 1x1 convolutions over F frames,
``F.interpolate(mode='bilinear', align_corners=False)`` for the top-down path, and the whole FPN (fpn.py:47-69) from them:

    L_3 = inner_3(C_3),  L_k = inner_k(C_k) + up(L_{k+1}),  P_k = layer_k(L_k)          levels k = 0..3 (4x .. 32x)

Maps are channel-major here as on the device, [C, F, h, w]; the frames are the batch of the stock ops."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import conv3d_backward_oracle as CO

# ------------------------------------------------------------------------------------------------ one convolution
CONV_F = (1, 3)
CONV_HW = ((1, 2), (3, 5), (6, 10), (8, 16))                   # narrower than a tile, ragged rows and columns, an odd pixel count (F 1 / 3 x 3 x 5)
WGRAD9_CHANNELS = ((4, 32), (64, 96), (36, 160))               # (Cin, Cout): a mostly empty channel tile; two ci tiles, three of four waves; a second co workgroup
WGRAD9_WIDE = tuple((ci, co, t, h, w) for ci, co, t, h, w in CO.WIDE_SHAPES)           # (Cin, Cout, F, H, W): the 32- and 64-column tiles, a ragged last tile along x
WGRAD9_CHUNKED = (32, 32, 5, 13, 16)                           # 5 x 4 x 1 = 20 tiles of 4 rows x 16 columns, at least 8 to a chunk: 8 + 8 + 4
WGRAD1_CIN, WGRAD1_COUT = (4, 68), (32, 96, 160)
WGRAD1_FHW = ((1, 3, 5), (1, 1, 2), (2, 12, 16))               # F h w = 15 (odd), 2, 384
WGRAD1_WIDEST = (2048, 256, 2, 1, 2)                           # the real widest lateral: the grid's widest extent along ci
WGRAD1_CHUNKED = (68, 96, 2, 19, 32)                           # 1216 voxels = 38 tiles of 32, at least 16 to a chunk: 16 + 16 + 6
DGRAD_CHANNELS = ((32, 32), (64, 96))                          # (Cin, Cout)
FPN_MAPS = ((8, 16), (4, 8), (2, 4), (1, 2))                   # levels 0..3
FPN_LATERAL = (32, 64, 128, 256)


def conv_case(Cin, Cout, Fr, H, W, taps=9, seed=0):
    rng = np.random.default_rng(100003 * Cin + 1009 * Cout + 101 * Fr + 11 * H + W + 7 * taps + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    k = 3 if taps == 9 else 1
    g = f(Cout, Fr, H, W)
    g[rng.random(g.shape) < 0.1] = 0.0
    return dict(x=f(Cin, Fr, H, W), w=(f(Cout, Cin, k, k) / np.sqrt(taps * Cin)).astype(np.float32), b=(0.1 * f(Cout)).astype(np.float32), g=g,
                a=f(Cin, Fr, H, W))                            # a: an addend of the data gradient


def frames_first(v):
    return v.permute(1, 0, 2, 3)


def conv_oracle(case, dtype):
    """-> dict(out, dx, dw, db) as float64 numpy, channel-major: F.conv2d (padding 1 for a 3x3 weight, 0 for a 1x1) over the frames and its autograd."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
    x, w, b = t(case["x"]), t(case["w"]), t(case["b"])
    out = frames_first(F.conv2d(frames_first(x), w, b, padding=w.shape[-1] // 2))
    out.backward(torch.from_numpy(case["g"]).to(dtype))
    n = lambda a: a.detach().double().numpy()
    return dict(out=n(out), dx=n(x.grad), dw=n(w.grad), db=n(b.grad))


def neighbourhood(x, f, y, xx):
    """The 3 x 3 neighbourhood of pixel (y, xx) of frame f in x [Cin, F, H, W], zeros outside the frame: [Cin, 3, 3]."""
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))[:, f, y:y + 3, xx:xx + 3]


def corners(H, W):
    return sorted({(y, x) for y in (0, H - 1) for x in (0, W - 1)})


# ------------------------------------------------------------------------------------------------ the top-down path
def up2(v):
    """Bilinear x2 of [C, F, h, w], align_corners=False."""
    return F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)


def up2_adjoint(g):
    """The adjoint of ``up2``: [C, F, 2h, 2w] -> [C, F, h, w], from autograd (up2 is linear)."""
    z = torch.zeros(g.shape[0], g.shape[1], g.shape[2] // 2, g.shape[3] // 2, dtype=g.dtype, requires_grad=True)
    up2(z).backward(g)
    return z.grad


# ------------------------------------------------------------------------------------------------ the whole FPN
NAMES = ["fpn_%s%d.%s" % (kind, k + 1, part) for kind in ("layer", "inner") for part in ("weight", "bias") for k in range(4)]


def fpn_params(lateral=FPN_LATERAL, channels=32, seed=0):
    """{'fpn_inner1.weight': ..., ...} as float32 numpy, in the state dict's names (level k is number k + 1)."""
    rng = np.random.default_rng(977 * channels + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    p = {}
    for k, cin in enumerate(lateral):
        p["fpn_inner%d.weight" % (k + 1)] = (f(channels, cin, 1, 1) / np.sqrt(cin)).astype(np.float32)
        p["fpn_inner%d.bias" % (k + 1)] = (0.1 * f(channels)).astype(np.float32)
        p["fpn_layer%d.weight" % (k + 1)] = (f(channels, channels, 3, 3) / np.sqrt(9 * channels)).astype(np.float32)
        p["fpn_layer%d.bias" % (k + 1)] = (0.1 * f(channels)).astype(np.float32)
    return p


def fpn_case(Fr=2, maps=FPN_MAPS, lateral=FPN_LATERAL, channels=32, seed=0, levels=(0, 1, 2, 3)):
    """Stage outputs C_k [lateral_k, F, h_k, w_k], parameters, and an upstream gradient on the maps of ``levels`` (zeros elsewhere)."""
    rng = np.random.default_rng(31 * Fr + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    Cs = [f(c, Fr, h, w) for c, (h, w) in zip(lateral, maps)]
    ups = [f(channels, Fr, h, w) if k in levels else np.zeros((channels, Fr, h, w), np.float32) for k, (h, w) in enumerate(maps)]
    return dict(C=Cs, params=fpn_params(lateral, channels, seed), g=ups)


def fpn_forward(Cs, params, dtype, L_data=None, P_data=None):
    """-> (L[4], P[4]) channel-major torch tensors in ``dtype``; Cs tensors or arrays [Cin_k, F, h, w], params tensors (live: they receive the
    gradients) or arrays.  L_data: the VALUES the merged laterals take (the device's own, read back) -- the graph stays the FPN's, so the
    gradients flow as ever, and the output convolutions and their weight gradients see exactly these maps.  P_data: likewise the values of
    the output maps (what a consumer behind the FPN is fed)."""
    t = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).to(dtype)
    Ls, Ps = [None] * 4, [None] * 4
    for k in (3, 2, 1, 0):
        lat = F.conv2d(frames_first(t(Cs[k])), t(params["fpn_inner%d.weight" % (k + 1)]), t(params["fpn_inner%d.bias" % (k + 1)]))
        if k < 3:
            lat = lat + up2(Ls[k + 1])
        if L_data is not None:
            lat = lat + (frames_first(t(L_data[k])) - lat).detach()
        Ls[k] = lat
        Ps[k] = F.conv2d(lat, t(params["fpn_layer%d.weight" % (k + 1)]), t(params["fpn_layer%d.bias" % (k + 1)]), padding=1)
        if P_data is not None:
            Ps[k] = Ps[k] + (frames_first(t(P_data[k])) - Ps[k]).detach()
    return [frames_first(v) for v in Ls], [frames_first(v) for v in Ps]


def fpn_gradients(Cs, params, ups, dtype, L_data=None):
    """{name: gradient as float64 numpy} of sum_k <P_k, ups_k> for the sixteen FPN parameters, evaluated in ``dtype``; plus (L, P) values."""
    live = {n: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for n, v in params.items()}
    Ls, Ps = fpn_forward(Cs, live, dtype, L_data)
    sum((P * torch.from_numpy(np.asarray(u)).to(dtype)).sum() for P, u in zip(Ps, ups)).backward()
    grads = {n: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().double().numpy() for n, v in live.items()}
    return grads, [v.detach() for v in Ls], [v.detach() for v in Ps]


# ------------------------------------------------------------------------------------------------ the FPN feeding a decoder
def decoder_margin(m, T, feats):
    """min |pre-ReLU| over all seven stages of the fp64 reference decoder with m's weights on ``feats`` (32x .. 4x): the condition of
    tests/conv3d_backward_oracle.py select_seed, on given features."""
    from tests import decoder_tail_oracle as TO
    t64 = CO.make_decoder("embedding", T).double()
    t64.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    G = t64.gn_groups
    with torch.no_grad():
        convouts, pre = CO.decoder_conv_outputs(t64, feats, torch.float64)
        for D, (blk, idx), pool in zip(convouts, t64._LAST_STAGE, CO.last_stage_pools(t64)):
            gn = getattr(t64, blk)[idx + 1]
            pre.append(TO.gn_forward(D, gn.weight if G else None, gn.bias if G else None, G, pool, t64.gn_eps or TO.GN_EPS)[0])
    return min(float(p.abs().min()) for p in pre)


def select_fpn_seed(m, T):
    """The first of CO.SEEDS whose FPN case (F = T frames, 32 channels everywhere) gives maps that keep every pre-ReLU value of the decoder
    CO.RELU_MARGIN from 0 in fp64.  -> (seed, the case, L and P of the fp64 FPN rounded to fp32, the margin)."""
    tried = []
    for seed in CO.SEEDS:
        case = fpn_case(Fr=T, lateral=(32, 32, 32, 32), seed=seed)
        L64, P64 = fpn_forward(case["C"], case["params"], torch.float64)
        L, P = [v.float() for v in L64], [v.float() for v in P64]
        tried.append(decoder_margin(m, T, P[::-1]))
        if tried[-1] >= CO.RELU_MARGIN:
            return seed, case, L, P, tried[-1]
    raise AssertionError("no seed of %r keeps the pre-ReLU values %g away from 0: %s" % (CO.SEEDS, CO.RELU_MARGIN, tried))


def fpn_decoder_gradients(m, T, case, L, P, up, act, axes, grids, dtype):
    """{name: gradient} of sum(decoder(FPN(C)) * up) for the sixteen FPN parameters (and, under 'decoder.', the decoder's), the chain evaluated
    in ``dtype`` with the FPN's laterals and maps taking the values L, P."""
    live = {n: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for n, v in case["params"].items()}
    _, Ps = fpn_forward(case["C"], live, dtype, L, P)
    trunk = CO.make_decoder("embedding", T).to(dtype)
    trunk.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    out, _ = CO.decoder_forward(trunk, Ps[::-1], act, axes, grids, dtype)
    out.backward(up.to(dtype))
    g = {n: v.grad.detach().double().numpy() for n, v in live.items()}
    g.update({"decoder." + n: p.grad.detach().double().numpy() for n, p in trunk.named_parameters() if p.grad is not None})
    return g
