"""The oracle of the ResNeXt backward tests: torch on the CPU with autograd, ``F.conv2d(..., groups=, stride=)`` over the frames, in the dtype
asked for (fp32 and fp64 on the same input; the spread between the two is the yardstick, tests/decoder_tail_oracle.py ``check`` / ``bound``).
tests/body_backward_oracle.py with two more block properties: ``groups`` (conv2 is [mid, mid / groups, 3, 3]) and ``stride_in_3x3`` (the
stride of a stage's first block sits in conv2: conv1 runs on the un-subsampled input, the shortcut on the subsampled one).  Maps are
channel-major as on the device, [C, F, h, w]; the device's recomputed activations can be GIVEN as there."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import body_backward_oracle as BO

CONVS = BO.CONVS
frames_first = BO.frames_first


# ------------------------------------------------------------------------------------------------ one convolution
def conv_case(groups, cg, stride, Fr, H, W, seed=0):
    """x [C, F, H, W] (about half of it zero, as after a ReLU), w [C, cg, 3, 3], the upstream g [C, F, Ho, Wo] with zeros, and a ReLU mask's
    activation m [C, F, H, W] (zeros block)."""
    Cn = groups * cg
    rng = np.random.default_rng(100003 * groups + 1009 * cg + 97 * stride + 31 * Fr + 7 * H + W + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = f(Cn, Fr, Ho, Wo)
    g[rng.random(g.shape) < 0.1] = 0.0
    return dict(x=np.maximum(f(Cn, Fr, H, W), 0), w=(f(Cn, cg, 3, 3) * np.sqrt(2.0 / (9 * cg))).astype(np.float32), g=g, m=np.maximum(f(Cn, Fr, H, W), 0),
                groups=groups, stride=stride)


def conv_oracle(case, dtype):
    """-> dict(y, dw, dx) as float64 numpy: autograd through F.conv2d(padding=1, stride=, groups=)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    x, w = frames_first(t(case["x"])).requires_grad_(True), t(case["w"]).requires_grad_(True)
    y = F.conv2d(x, w, padding=1, stride=case["stride"], groups=case["groups"])
    y.backward(frames_first(t(case["g"])))
    n = lambda a: a.detach().double().numpy()
    return dict(y=n(frames_first(y)), dw=n(w.grad), dx=n(frames_first(x.grad)))


def dw_formula(case):
    """dW[co][cj][ky][kx] = sum_{f, y, x} dy[co][f, y, x] * x[g(co) Cg + cj][f, s y + ky, s x + kx] (x zero-haloed), written out in fp64."""
    x, g, s, groups = case["x"].astype(np.float64), case["g"].astype(np.float64), case["stride"], case["groups"]
    Cn, cg = case["w"].shape[:2]
    _, Fr, Ho, Wo = g.shape
    xh = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dw = np.zeros((Cn, cg, 3, 3))
    for ky in range(3):
        for kx in range(3):
            win = xh[:, :, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s].reshape(groups, cg, Fr, Ho, Wo)
            dw[:, :, ky, kx] = np.einsum("gofyx,gcfyx->goc", g.reshape(groups, cg, Fr, Ho, Wo), win).reshape(Cn, cg)
    return dw


def dgrad_weight(w, groups):
    """W'[g Cg + cj][co_j][ky][kx] = w[g Cg + co_j][cj][2 - ky][2 - kx]."""
    Cn, cg = w.shape[:2]
    return np.ascontiguousarray(w.reshape(groups, cg, cg, 3, 3).transpose(0, 2, 1, 3, 4)[:, :, :, ::-1, ::-1]).reshape(Cn, cg, 3, 3)


def dx_formula(case, H, W):
    """The data gradient as the issue composes it, in fp64: the forward grouped convolution (stride 1, padding 1, the same groups) of dy --
    zero-dilated to H x W for stride 2 -- with ``dgrad_weight``."""
    g, s = torch.from_numpy(case["g"]).double(), case["stride"]
    Cn, Fr = g.shape[:2]
    d = torch.zeros(Cn, Fr, H, W, dtype=torch.float64)
    d[:, :, ::s, ::s] = g
    wp = torch.from_numpy(dgrad_weight(case["w"].astype(np.float64), case["groups"]))
    return frames_first(F.conv2d(frames_first(d), wp, padding=1, groups=case["groups"])).numpy()


# ------------------------------------------------------------------------------------------------ one block
def block_params(rng, Cin, mid, Cout, projection, groups=1):
    p = BO.block_params(rng, Cin, mid, Cout, projection)
    if groups != 1:
        cg = mid // groups
        p["conv2"] = (rng.standard_normal((mid, cg, 3, 3)) * np.sqrt(2.0 / (9 * cg))).astype(np.float32)
    return p


def block_case(kind, Cin, mid, Cout, stride, groups, s3, Fr, h, w, seed=0):
    rng = np.random.default_rng(7919 * Cin + 131 * mid + 17 * Cout + 1000003 * Fr + 101 * h + w + 13 * groups + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    g = f(Cout, Fr, h, w)
    g[rng.random(g.shape) < 0.1] = 0.0
    return dict(x=f(Cin, Fr, h * stride, w * stride), params=block_params(rng, Cin, mid, Cout, "identity" not in kind, groups), g=g, stride=stride,
                groups=groups, stride_in_3x3=bool(s3))


def block_forward(x, live, stride, dtype, given=None, groups=1, stride_in_3x3=False):
    """BO.block_forward with the two properties.  x [F, Cin, H, W] frames first.  -> (a1, a2, out) frames first."""
    conv = lambda v, n, pad=0, s=1, g=1: (F.conv2d(v, live[n], padding=pad, stride=s, groups=g) * live[n + ".s"].view(1, -1, 1, 1) + live[n + ".b"].view(1, -1, 1, 1))
    gv = given or {}
    s3 = stride == 2 and stride_in_3x3
    xs = x[:, :, ::2, ::2] if stride == 2 else x
    a1 = BO._given(conv(x if s3 else xs, "conv1"), gv.get("a1"), dtype)
    a2 = BO._given(conv(a1, "conv2", 1, 2 if s3 else 1, groups), gv.get("a2"), dtype)
    sc = conv(xs, "down") if "down" in live else xs
    out = BO._given(conv(a2, "conv3") + sc, gv.get("out"), dtype)
    return a1, a2, out


def block_gradients(case, dtype, given=None):
    """-> dict(conv1, conv2, conv3, down (when there is one), g_x) as float64 numpy, and the activations channel-major.  g_x is the gradient of
    the block's input where the device returns it: of xs [Cin, F, h, w] with the stride in the 1x1, of x [Cin, F, 2h, 2w] with it in the 3x3."""
    live = BO.live_params(case["params"], dtype)
    x = frames_first(torch.from_numpy(case["x"])).to(dtype).requires_grad_(True)
    a1, a2, out = block_forward(x, live, case["stride"], dtype, given, case["groups"], case["stride_in_3x3"])
    out.backward(frames_first(torch.from_numpy(case["g"])).to(dtype))
    n = lambda a: a.detach().double().numpy()
    gx = frames_first(x.grad)
    if case["stride"] == 2 and not case["stride_in_3x3"]:
        gx = gx[:, :, ::2, ::2]
    grads = {k: n(live[k].grad) for k in CONVS if k in live}
    grads["g_x"] = n(gx)
    return grads, {k: frames_first(v).detach() for k, v in (("a1", a1), ("a2", a2), ("out", out))}


# ------------------------------------------------------------------------------------------------ the composed body
def body_case(groups, s3, stages, levels=(1, 2, 3), seed=0, cin=BO.BODY_IN, Fr=BO.BODY_F, hw=BO.BODY_HW):
    """BO.body_case with grouped conv2 weights; the first block of every stage is a stride-2 projection, with the stride where ``s3`` says."""
    rng = np.random.default_rng(5297 + seed + 11 * groups + int(s3))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    h, w = hw
    case = dict(x=np.abs(f(cin, Fr, h, w)), stages=[], g=[], groups=groups, stride_in_3x3=bool(s3))
    for k, (nb, mid, cout) in enumerate(stages, 1):
        case["stages"].append([block_params(rng, cin if b == 0 else cout, mid, cout, b == 0, groups) for b in range(nb)])
        cin, h, w = cout, h // 2, w // 2
        case["g"].append(f(cout, Fr, h, w) if k in levels else np.zeros((cout, Fr, h, w), np.float32))
    return case


def body_gradients(case, dtype, given=None, first_stage=0):
    """BO.body_gradients for such a body: {(stage index, block, conv): gradient as float64 numpy} of sum_k <C_k, g_k>."""
    live = [[BO.live_params(p, dtype) for p in blocks] for blocks in case["stages"]]
    x = frames_first(torch.from_numpy(case["x"])).to(dtype)
    outs = []
    for k, blocks in enumerate(live):
        for b, lp in enumerate(blocks):
            _, _, x = block_forward(x, lp, 2 if b == 0 else 1, dtype, None if given is None else given[k][b], case["groups"], case["stride_in_3x3"])
        outs.append(x)
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
