"""The oracle of the body backward tests: torch on the CPU with autograd, ``F.conv2d`` over the frames, in the dtype asked for (the tests run it
in fp32 and in fp64 on the same input; the fp32-versus-fp64 spread of a case is the yardstick its device error is held to --
tests/decoder_tail_oracle.py, whose ``check`` / ``bound`` / ``max_norm_err`` these tests use).

One ``BottleneckWithFixedBatchNorm`` block with the FrozenBN written out, y = s * conv(x; w) + b (s, b constant buffers, the gradient is w's):

    xs = x[::2, ::2] (stride 2) | x,   a1 = relu(bn1(conv1(xs))),  a2 = relu(bn2(conv2(a1))),  out = relu(bn3(conv3(a2)) + sc),   sc = bnd(down(xs)) | xs

The device's own (recomputed) activations can be GIVEN: an activation then takes the device's value and the device's ReLU mask,
a = a_dev + [a_dev > 0 or NaN] * (lin - lin.detach()), so both oracle runs and the device see the same masks and the same inputs of the
weight gradients: no forward-precision term and no mask flip at a near-zero activation enters the comparison.  Maps are channel-major
here as on the device, [C, F, h, w]; the frames are the batch of the stock ops."""
import numpy as np
import torch
import torch.nn.functional as F

CONVS = ("conv1", "conv2", "conv3", "down")

# one block: (kind, Cin, mid, Cout, stride)
BLOCKS = (("projection", 64, 32, 128, 1), ("identity", 128, 32, 128, 1), ("projection2", 128, 64, 256, 2))
BLOCK_F = (1, 3)
BLOCK_HW = ((1, 2), (3, 5), (8, 16))                       # after the stride
# the composed body: the input of the first stage, then three stages (the analogues of layer2 .. layer4)
BODY_IN = 32
BODY_STAGES = ((2, 32, 64), (3, 32, 128), (2, 64, 256))    # (blocks, mid, Cout)
BODY_F, BODY_HW = 2, (16, 32)                              # the input map; the stages run at 8x16, 4x8, 2x4


def frames_first(v):
    return v.permute(1, 0, 2, 3)


def block_params(rng, Cin, mid, Cout, projection):
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    p = {"conv1": (f(mid, Cin, 1, 1) * np.sqrt(2.0 / Cin)).astype(np.float32), "conv2": (f(mid, mid, 3, 3) * np.sqrt(2.0 / (9 * mid))).astype(np.float32),
         "conv3": (f(Cout, mid, 1, 1) * np.sqrt(1.0 / mid)).astype(np.float32)}
    if projection:
        p["down"] = (f(Cout, Cin, 1, 1) * np.sqrt(1.0 / Cin)).astype(np.float32)
    for n in list(p):
        co = p[n].shape[0]
        p[n + ".s"] = rng.uniform(0.5, 1.5, co).astype(np.float32)            # the FrozenBN scale
        p[n + ".b"] = (0.2 * f(co)).astype(np.float32)                        # ... and shift
    return p


def folded(p, name):
    """The weight with the scale folded in, as ``ResNetFPN._fold`` forms it: one fp32 multiply."""
    return (p[name] * p[name + ".s"][:, None, None, None]).astype(np.float32)


def block_case(kind, Cin, mid, Cout, stride, Fr, h, w, seed=0):
    rng = np.random.default_rng(7919 * Cin + 131 * mid + 17 * Cout + 1000003 * Fr + 101 * h + w + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    g = f(Cout, Fr, h, w)
    g[rng.random(g.shape) < 0.1] = 0.0
    return dict(x=f(Cin, Fr, h * stride, w * stride), params=block_params(rng, Cin, mid, Cout, kind != "identity"), g=g, stride=stride)


def _given(lin, dev_value, dtype):
    """relu(lin), or the device's value with the device's mask on lin's graph."""
    if dev_value is None:
        return F.relu(lin)
    a = frames_first(torch.as_tensor(dev_value)).to(dtype)
    mask = (~(a <= 0)).to(dtype)
    return a + mask * (lin - lin.detach())


def block_forward(x, live, stride, dtype, given=None):
    """x [F, Cin, H, W] (frames first, in ``dtype``, possibly with a graph); live: {name: tensor in dtype} of the block's parameters (the
    weights may require a gradient); given: dict(a1, a2, out) channel-major device values or None.  -> (a1, a2, out) frames first."""
    conv = lambda v, n, pad=0: (F.conv2d(v, live[n], padding=pad) * live[n + ".s"].view(1, -1, 1, 1) + live[n + ".b"].view(1, -1, 1, 1))
    g = given or {}
    xs = x[:, :, ::2, ::2] if stride == 2 else x
    a1 = _given(conv(xs, "conv1"), g.get("a1"), dtype)
    a2 = _given(conv(a1, "conv2", 1), g.get("a2"), dtype)
    sc = conv(xs, "down") if "down" in live else xs
    out = _given(conv(a2, "conv3") + sc, g.get("out"), dtype)
    return a1, a2, out


def live_params(p, dtype):
    return {n: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(n in CONVS) for n, v in p.items()}


def block_gradients(case, dtype, given=None):
    """-> dict(conv1, conv2, conv3, down (when there is one), g_x = the gradient of xs [Cin, F, h, w]) as float64 numpy, and the
    activations dict(a1, a2, out) channel-major."""
    live = live_params(case["params"], dtype)
    x = frames_first(torch.from_numpy(case["x"])).to(dtype).requires_grad_(True)
    a1, a2, out = block_forward(x, live, case["stride"], dtype, given)
    out.backward(frames_first(torch.from_numpy(case["g"])).to(dtype))
    n = lambda a: a.detach().double().numpy()
    gx = frames_first(x.grad)
    if case["stride"] == 2:
        assert not bool(gx[:, :, 1::2].any()) and not bool(gx[:, :, :, 1::2].any())
        gx = gx[:, :, ::2, ::2]
    grads = {k: n(live[k].grad) for k in CONVS if k in live}
    grads["g_x"] = n(gx)
    return grads, {k: frames_first(v).detach() for k, v in (("a1", a1), ("a2", a2), ("out", out))}


# ------------------------------------------------------------------------------------------------ the composed body
def body_case(levels=(1, 2, 3), seed=0, stages=BODY_STAGES, cin=BODY_IN, Fr=BODY_F, hw=BODY_HW):
    """The input of the first stage, per stage the blocks' parameters (the first block a stride-2 projection), and an upstream gradient on
    the outputs of the stages of ``levels`` (1 .. 3: the stages in order; zeros elsewhere)."""
    rng = np.random.default_rng(4241 + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    h, w = hw
    case = dict(x=np.abs(f(cin, Fr, h, w)), stages=[], g=[])
    for k, (nb, mid, cout) in enumerate(stages, 1):
        case["stages"].append([block_params(rng, cin if b == 0 else cout, mid, cout, b == 0) for b in range(nb)])
        cin, h, w = cout, h // 2, w // 2
        case["g"].append(f(cout, Fr, h, w) if k in levels else np.zeros((cout, Fr, h, w), np.float32))
    return case


def body_forward(x, live_stages, dtype, given=None, stage_in=None):
    """x [F, C, H, W] frames first; live_stages: per stage per block the live parameters; given: per stage per block dict(a1, a2, out) device
    values; stage_in: per stage the VALUE its input takes (channel-major; None: the value computed) -- the device's recompute of a stage
    starts from the stage output the pass left, not from its own recompute of the stage before.  -> per stage the output, frames first."""
    outs = []
    for k, blocks in enumerate(live_stages):
        if stage_in is not None and stage_in[k] is not None:
            v = frames_first(torch.as_tensor(stage_in[k])).to(dtype)
            x = x + (v - x).detach()
        for b, live in enumerate(blocks):
            _, _, x = block_forward(x, live, 2 if b == 0 else 1, dtype, None if given is None else given[k][b])
        outs.append(x)
    return outs


def body_gradients(case, dtype, given=None, first_stage=0):
    """{(stage index, block, conv): gradient as float64 numpy} of sum_k <C_k, g_k> for the stages from ``first_stage`` on (the stages below
    are frozen: their parameters get no gradient), evaluated in ``dtype``."""
    live = [[live_params(p, dtype) for p in blocks] for blocks in case["stages"]]
    x = frames_first(torch.from_numpy(case["x"])).to(dtype)
    outs = body_forward(x, live, dtype, given)
    sum((o * frames_first(torch.from_numpy(g)).to(dtype)).sum() for o, g in zip(outs, case["g"])).backward()
    grads = {}
    for k, blocks in enumerate(live):
        if k < first_stage:
            continue
        for b, lp in enumerate(blocks):
            for c in CONVS:
                if c in lp:
                    grads[(k, b, c)] = (lp[c].grad if lp[c].grad is not None else torch.zeros_like(lp[c])).detach().double().numpy()
    return grads
