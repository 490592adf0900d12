"""The decoders' output stage at every width it serves, against fp64 references on the CPU.

Three layers: the fused heads kernel called directly (NOUT = 1..10, every activation and grid axis, the smallest legal shape,
ragged shapes, a grid-stride wrap, the LDS bound), the whole decoder at every head width the product can build (semseg
1..256 channels through the heads kernel or the 1x1x1 MFMA conv, every admitted embedding head, the seediness head; three fold
modes x three precisions), and the semseg mask kernel at new class counts.

Every float comparison has the form of tests/test_gpu_bf16x6.py: the HIP error against fp64, e_hip = max |hip - ref64| /
max(1, |ref64|), must stay within K times the error of plain fp32 torch on the CPU computing the same thing from the same
inputs (e32), or FLOOR where fp32 itself is nearly exact.  A 1e-3 bound would let a 10-bit error through.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import decoder as odec
from tests import synth

pytestmark = pytest.mark.gpu

# Measured on MI355X: worst e_hip / e32 3.9 for the heads kernel (Cin 2048 at the LDS bound: one fp32 accumulator summed in channel
# order against torch's blocked sums), 2.8 for the whole decoders (every precision), 1.0 for the mask kernel.  Rounding the linear-tail
# matrices to bf16, or scaling one wide-head weight row by 1 + 2^-12, fails every decoder width it touches.
K, FLOOR = 4.0, 1e-6
LDS_BYTES = 48 * 1024        # launch_heads' dynamic-LDS cap: (n_out + 2) * Cin floats


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def rel_err(got, ref64):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    return float((np.abs(got - ref64) / np.maximum(1.0, np.abs(ref64))).max())


def check(name, e_hip, e32, k=K):
    print("[heads] %-58s e_hip %.3e  e32 %.3e  ratio %.2f" % (name, e_hip, e32, e_hip / max(e32, 1e-30)))
    assert np.isfinite(e_hip) and e_hip <= max(k * e32, FLOOR), "%s: error %.3e vs fp64, fp32 CPU %.3e" % (name, e_hip, e32)


# ------------------------------------------------------------------------------------------------ a. hip.heads directly
def _act_ref(z, act, axis, G):
    """The heads' activations (embedding_decoder.py:131-143, inference_model.py:148) in z's dtype; G: axis -> grid [T,H,W]."""
    out = []
    for o in range(z.shape[0]):
        g = G[axis[o]] if act[o] in (1, 4) and axis[o] else 0.0
        a = act[o]
        out.append((z[o] * 0.25).tanh() + g if a == 1 else z[o].sigmoid() if a == 2 else z[o].exp() * 10 if a == 3 else z[o] + g if a == 4 else z[o])
    return torch.stack(out)


def _heads_refs(x, w, b, act, axis, grid):
    Cin, T, H, W = x.shape
    refs = []
    for dt in (torch.float64, torch.float32):
        gt, gy, gx = [g.to(dt) for g in grid]
        G = {1: gt[:, None, None].expand(T, H, W), 2: gy[None, :, None].expand(T, H, W), 3: gx[None, None, :].expand(T, H, W)}
        z = (torch.from_numpy(w).to(dt) @ torch.from_numpy(x).to(dt).reshape(Cin, -1) + torch.from_numpy(b).to(dt)[:, None]).reshape(-1, T, H, W)
        refs.append(_act_ref(z, act, axis, G).numpy())
    return refs


def _heads_case(rs, n, Cin, T, H, W):
    x = rs.standard_normal((Cin, T, H, W)).astype(np.float32)
    w = (rs.standard_normal((n, Cin)) / np.sqrt(Cin)).astype(np.float32)
    b = (0.1 * rs.standard_normal(n)).astype(np.float32)
    return x, w, b, odec.grid_vectors(H, W, T, 1.3)


def _rotation(n, r):
    """Channel o gets (act, axis) pair (o + r) % 20 of the 5 x 4: over r = 0..19 every channel meets every pair."""
    idx = [(o + r) % 20 for o in range(n)]
    return [i % 5 for i in idx], [i // 5 for i in idx]


def _cin_bound(n):
    return LDS_BYTES // ((n + 2) * 4) // 4 * 4


def _raw_heads(hip, x, w, b, act, axis, grid, out):
    Cin, T, H, W = x.shape
    n = w.shape[0]
    gt, gy, gx = [g.cuda() for g in grid]
    return hip.lib().stemseg_hip_heads(hip.ptr(x), Cin, T, H, W, hip.ptr(w), hip.ptr(b), n, (ctypes.c_int32 * n)(*act), (ctypes.c_int32 * n)(*axis),
                                       hip.ptr(gt), hip.ptr(gy), hip.ptr(gx), hip.ptr(out), hip.stream())


@pytest.mark.parametrize("n", list(range(1, 11)))
def test_heads_kernel_vs_fp64(hip, n):
    """Every NOUT instantiation of heads_kernel: the smallest legal shape and a ragged one under all 20 (act, axis) rotations, a
    4-channel map of 2.1 M voxels (more float4 groups than 2048 blocks x 256 threads: the grid-stride loop wraps), and Cin at the
    LDS bound.  Wider Cin than the bound is an argument error that leaves the output alone."""
    rs = np.random.RandomState(1000 + n)
    worst = 0.0
    for (Cin, T, H, W), rots in (((4, 1, 1, 4), range(20)), ((132, 3, 7, 12), range(20)), ((4, 8, 256, 1028), [n]), ((_cin_bound(n), 2, 3, 8), [n, n + 7])):
        x, w, b, grid = _heads_case(rs, n, Cin, T, H, W)
        xd, wd, bd = dev(x), dev(w), dev(b)
        e_hip = e32 = 0.0
        for r in rots:
            act, axis = _rotation(n, r)
            got = hip.heads(xd, wd, bd, act, axis, *[g.cuda() for g in grid]).cpu().numpy()
            assert got.shape == (n, T, H, W)
            ref64, ref32 = _heads_refs(x, w, b, act, axis, grid)
            e_hip, e32 = max(e_hip, rel_err(got, ref64)), max(e32, rel_err(ref32, ref64))
        check("heads n=%d Cin=%d T=%d H=%d W=%d (%d rotations)" % (n, Cin, T, H, W, len(rots)), e_hip, e32)
        worst = max(worst, e_hip / max(e32, 1e-30))
    print("[heads] n=%d: worst e_hip / e32 %.2f" % (n, worst))
    # one row of LDS past the bound: refused before the launch, the output untouched
    Cin = _cin_bound(n) + 4
    x, w, b, grid = _heads_case(rs, n, Cin, 1, 2, 4)
    out = torch.full((n, 1, 2, 4), 7.0, device="cuda")
    act, axis = _rotation(n, 0)
    rc = _raw_heads(hip, dev(x), dev(w), dev(b), act, axis, grid, out)
    torch.cuda.synchronize()
    assert rc == -1 and b"LDS" in hip.lib().stemseg_hip_last_error(), (rc, hip.lib().stemseg_hip_last_error())
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError):
        hip.heads(dev(x), dev(w), dev(b), act, axis, *[g.cuda() for g in grid])


@pytest.mark.parametrize("n", [1, 3, 10])
def test_heads_kernel_nan_stays_in_its_voxel(hip, n):
    """One NaN input value makes exactly its voxel's outputs NaN, in every channel whatever the activation; the other three voxels of
    its float4 group and every other voxel stay finite."""
    rs = np.random.RandomState(2000 + n)
    Cin, T, H, W = 132, 3, 7, 12
    x, w, b, grid = _heads_case(rs, n, Cin, T, H, W)
    t, y, xx = 1, 3, 5                                  # voxel 125: lane 1 of its float4 group
    x[37, t, y, xx] = np.nan
    for r in (0, 5, 10, 15):
        act, axis = _rotation(n, r)
        got = hip.heads(dev(x), dev(w), dev(b), act, axis, *[g.cuda() for g in grid]).cpu().numpy()
        want = np.zeros(got.shape, bool)
        want[:, t, y, xx] = True
        assert np.array_equal(np.isnan(got), want) and np.isfinite(got[~want]).all(), (n, r)


# ------------------------------------------------------------------------------------------------ b. whole decoders at every width
CIN, INTER = 256, (256, 256, 128, 128)
H32, W32 = 3, 3                                     # 4x map 24 x 24 (AvgPool3d(3) needs 3 x 3 at 32x)
FOLDS = (("default", True, True), ("conv_4 only", False, True), ("step by step", False, False))
PRECISIONS = ("f32", "bf16x6", "f16x3")
SEMSEG_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 31, 32, 33, 41, 42, 64, 65, 96, 256)


@pytest.fixture(scope="module")
def trunk():
    """(T, norm) -> shared trunk: state dict, features, and the trunk output (conv_4's) in fp64 and in fp32, both by the oracle on the
    CPU.  Only the heads vary across widths."""
    cache = {}

    def get(T, norm):
        if (T, norm) not in cache:
            names = [(k, s) for k, s in odec.decoder_param_shapes("", inter=INTER, cin=CIN, kind="seediness") if not k.startswith("conv_out")]
            sd = synth.synth_state_dict(names, 300 + T, prefix="trunk.")
            if norm == "none":          # seven stacked convs without normalisation: keep the activations in range
                sd = {k: (v * np.float32(0.35) if v.ndim == 5 and v.shape[-1] == 3 else v) for k, v in sd.items()}
            feats = synth.synth_features(T, H32, W32, C=CIN, seed=400 + T)
            odec.VARIANT.update(norm=norm)
            try:
                x = [odec.trunk([torch.from_numpy(f).to(dt)[None] for f in feats], {k: torch.from_numpy(v).to(dt) for k, v in sd.items()}, "", T)[0]
                     for dt in (torch.float64, torch.float32)]
            finally:
                odec.VARIANT.update(norm="gn")
            cache[(T, norm)] = dict(sd=sd, feats=feats, x64=x[0], x32=x[1], dev=[dev(f) for f in feats])
        return cache[(T, norm)]
    return get


def _module(kind, T, norm, cfg):
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder as Emb
    from stemseg_amd.modeling.seediness_decoder import SqueezingExpandDecoder as Seed
    from stemseg_amd.modeling.semseg_decoder import SqueezeExpandDecoder as Sem
    Norm = (lambda c: nn.GroupNorm(32, c)) if norm == "gn" else (lambda c: nn.Identity())
    if kind == "semseg":
        return Sem(CIN, cfg["ncls"], list(INTER), (4, 8, 16, 32), foreground_channel=cfg["fg"], NormType=Norm, num_frames=T)
    if kind == "embedding":
        return Emb(CIN, list(INTER), cfg["E"], cfg.get("tanh", True), cfg["seed"], cfg["mode"], NormType=Norm, num_frames=T)
    return Seed(CIN, list(INTER), NormType=Norm, num_frames=T)


def _load(m, tr, head_seed, time_scale=1.0):
    """Trunk weights from the shared state dict, head weights (He-normal, biases 0.1 N(0, 1)) from a seed of their own."""
    sd, heads = {}, {}
    for k, v in m.state_dict().items():
        if k in tr["sd"]:
            sd[k] = torch.from_numpy(tr["sd"][k])
        elif k == "time_scale":
            sd[k] = torch.tensor(time_scale, dtype=torch.float32)
        else:
            rs = np.random.RandomState(head_seed + 7919 * len(heads))
            a = rs.standard_normal(tuple(v.shape))
            a = a * np.sqrt(2.0 / INTER[3]) if a.ndim == 5 else 0.1 * a
            heads[k] = a.astype(np.float32)
            sd[k] = torch.from_numpy(heads[k])
    m.load_state_dict(sd)
    return m.cuda().eval(), heads


def _decoder_ref(kind, cfg, x, heads, dt):
    """The heads of semseg_decoder.py:116 / seediness_decoder.py:112 / embedding_decoder.py:131-143 (+ inference_model.py:148 when the
    bandwidth activation is fused) applied to the trunk output x [c4, T, H, W] in dtype dt."""
    c4, T, H, W = x.shape
    X = x.to(dt).reshape(c4, -1)

    def lin(key):
        return (torch.from_numpy(heads[key]).to(dt).reshape(-1, c4) @ X).reshape(-1, T, H, W)
    if kind == "semseg":
        return lin("conv_out.weight")
    if kind == "seediness":
        return lin("conv_out.weight").sigmoid()
    emb = lin("conv_embedding.weight")
    if cfg.get("tanh", True):
        emb = (emb * 0.25).tanh()
    outs = [odec.add_offset(emb, cfg["mode"], cfg.get("ts", 1.0))]            # (fp32 linspace grid, promoted to dt)
    var = lin("conv_variance.weight") + torch.from_numpy(heads["conv_variance.bias"]).to(dt)[:, None, None, None]
    outs.append(var.exp() * 10 if cfg.get("fuse_bw") else var)
    if cfg["seed"]:
        outs.append(lin("conv_seediness.weight").sigmoid())
    return torch.cat(outs, 0)


def _clip_batch_check(hip, m, tr, n_out, T):
    """Three clips through one clip-batched call (layout 2, hip.alloc_padded_batch) == three single-clip calls, bit for bit."""
    N = 3
    levels = [hip.alloc_padded_batch(N, CIN, T, H32 * s, W32 * s, "cuda") for s in (1, 2, 4, 8)]
    for c in range(N):
        for (bufs, g, _), f, s in zip(levels, tr["feats"], (1, 2, 4, 8)):
            hip.copy_to_volume(dev(np.roll(f, c, axis=0)), 0, hip.padded_interior_view(bufs[c], g, CIN, T, H32 * s, W32 * s))
    shape = (T, H32 * 8, W32 * 8)
    singles = [m.forward_single(([lv[0][c] for lv in levels], shape), 2).clone() for c in range(N)]
    batch = m.forward_single(([lv[0][0] for lv in levels], shape), 2, clip_batch=(N, [lv[2] for lv in levels]))
    torch.cuda.synchronize()
    assert tuple(batch.shape) == (N, n_out) + shape
    assert not torch.equal(singles[0], singles[1])
    for c in range(N):
        assert torch.equal(batch[c], singles[c]), "clip %d of the batch differs from its single-clip call" % c


def _sweep(hip, trunk, kind, cfgs, n_out):
    """Every config at T = 4 and 8, three precisions x three fold modes, against fp64; the worst e_hip / e32 per precision is printed."""
    worst = {p: 0.0 for p in PRECISIONS}
    for ci, cfg in enumerate(cfgs):
        for T in (4, 8):
            tr = trunk(T, cfg.get("norm", "gn"))
            m, heads = _load(_module(kind, T, cfg.get("norm", "gn"), cfg), tr, 5000 + 31 * n_out + ci, cfg.get("ts", 1.0))
            if kind == "embedding":
                m.fuse_bandwidth_activation = bool(cfg.get("fuse_bw"))
            ref64 = _decoder_ref(kind, cfg, tr["x64"], heads, torch.float64).numpy()
            e32 = rel_err(_decoder_ref(kind, cfg, tr["x32"], heads, torch.float32).numpy(), ref64)
            shape = (n_out, T, H32 * 8, W32 * 8)
            assert ref64.shape == shape
            outs = {}
            for prec in PRECISIONS:
                for fname, lin, c4 in FOLDS:
                    m.precision, m.fold_linear_tail, m.fold_conv4 = prec, lin, c4
                    out = m.forward_single(tr["dev"], 0)
                    assert tuple(out.shape) == shape, (tuple(out.shape), shape)
                    outs[(prec, fname)] = got = out.cpu().numpy()
                    e_hip = rel_err(got, ref64)
                    check("%s %s T=%d %s %s" % (kind, cfg.get("name", ""), T, prec, fname), e_hip, e32)
                    worst[prec] = max(worst[prec], e_hip / max(e32, 1e-30))
            m.precision, m.fold_linear_tail, m.fold_conv4 = "f16x3", True, True
            assert np.array_equal(m.forward_single(tr["dev"], 0).cpu().numpy(), outs[("f16x3", "default")])
            if T == 8 and ci == 0:
                _clip_batch_check(hip, m, tr, n_out, T)
    print("[heads] %s width %d: worst e_hip / e32 per precision: %s" % (kind, n_out, ", ".join("%s %.2f" % kv for kv in worst.items())))


@pytest.mark.parametrize("n_out", SEMSEG_WIDTHS)
def test_semseg_decoder_every_width_vs_fp64(hip, trunk, n_out):
    """Semseg heads of n_out channels, through num_classes with and without the foreground channel: n_out <= 10 on the fused heads
    kernel (9 and 10 used to fail to build), wider on the 1x1x1 MFMA conv padded to a multiple of 32 -- unpadded at 32 / 64 / 96 /
    256, padded otherwise; only n_out channels come back."""
    cfgs = [dict(ncls=n_out, fg=False, name="%d classes" % n_out)]
    if n_out >= 2:
        cfgs.append(dict(ncls=n_out - 1, fg=True, name="%d classes + fg" % (n_out - 1)))
    _sweep(hip, trunk, "semseg", cfgs, n_out)


def _embedding_configs():
    """width -> the (EMBEDDING_DIM_MODE, EMBEDDING_SIZE, seediness) heads embedding_utils admits with at most 10 channels and at least
    one variance channel (widths 3..10): every one whose EMBEDDING_SIZE is at most the mode's embedding dims (every reference config
    has them equal), and at least two per width -- topped up with the widest modes' larger sizes (width 9 and 10 need them)."""
    by_width, extra = {}, {}
    for mode, nb in odec._NB_DIMS.items():
        nf = odec.nb_free_dims(mode)
        for E in range(nf + 1, 11):
            for so in (False, True):
                w = nb + (E - nf) + int(so)
                if w <= 10:
                    c = dict(mode=mode, E=E, seed=so, name="%s E=%d%s" % (mode, E, " +seed" if so else ""))
                    (by_width if E <= nb else extra).setdefault(w, []).append(c)
    for w, cs in extra.items():
        cs.sort(key=lambda c: (-odec._NB_DIMS[c["mode"]], c["E"]))
        by_width.setdefault(w, [])
        by_width[w] += cs[:max(0, 2 - len(by_width[w]))]
    # the head variants, once each: plain grid offset, fused bandwidth, time_scale != 1, no normalisation layer
    for w, mode, E, so, extra in ((6, "xyff", 4, False, dict(tanh=False)), (7, "xyff", 4, True, dict(fuse_bw=True)),
                                  (8, "xytff", 5, False, dict(ts=1.75)), (9, "xytff", 5, True, dict(norm="none"))):
        c = next(c for c in by_width[w] if (c["mode"], c["E"], c["seed"]) == (mode, E, so))
        c.update(extra)
        c["name"] += " " + ",".join("%s=%s" % kv for kv in extra.items())
    return by_width


EMBEDDING_CONFIGS = _embedding_configs()


@pytest.mark.parametrize("n_out", sorted(EMBEDDING_CONFIGS))
def test_embedding_decoder_every_width_vs_fp64(hip, trunk, n_out):
    _sweep(hip, trunk, "embedding", EMBEDDING_CONFIGS[n_out], n_out)


def test_seediness_decoder_vs_fp64(hip, trunk):
    _sweep(hip, trunk, "seediness", [dict(name="sigmoid")], 1)


def test_embedding_head_wider_than_10_is_refused(hip):
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder as Emb
    with pytest.raises(NotImplementedError):
        Emb(CIN, list(INTER), 7, True, True, "xytff", num_frames=8)          # 5 + 5 + 1 = 11


# ------------------------------------------------------------------------------------------------ c. semseg masks at new widths
@pytest.mark.parametrize("C", [2, 3, 9, 10, 11, 42])
def test_semseg_masks_vs_fp64(hip, C):
    """inference_model.py:197-231 on mean logits: C > 2 -> sigmoid of the last channel, softmax / logits / argmax of the rest;
    C == 2 -> softmax channel 1.  Argmax is compared where the top two fp64 means lie more than 1e-5 apart."""
    rs = np.random.RandomState(3000 + C)
    Fn, H, W = 5, 9, 13
    counts = np.array([1, 2, 3, 4, 7], np.float32)
    sums = (3 * rs.standard_normal((Fn, C, H, W)) * counts[:, None, None, None]).astype(np.float32)
    mean64 = sums.astype(np.float64) / counts.astype(np.float64)[:, None, None, None]
    mean32 = torch.from_numpy(sums) / torch.from_numpy(counts)[:, None, None, None]
    for kind in (None, "logits", "probs", "argmax"):
        fg, mc = hip.semseg_masks(dev(sums), dev(counts), kind)
        fg = fg.cpu().numpy()
        if C == 2:
            e = np.exp(mean64 - mean64.max(1, keepdims=True))
            check("masks C=2 fg %s" % kind, rel_err(fg, e[:, 1] / e.sum(1)), rel_err(torch.softmax(mean32, 1)[:, 1].numpy(), e[:, 1] / e.sum(1)))
            assert mc is None
            continue
        fg64 = 1 / (1 + np.exp(-mean64[:, -1]))
        check("masks C=%d fg %s" % (C, kind), rel_err(fg, fg64), rel_err(mean32[:, -1].sigmoid().numpy(), fg64))
        cls64, cls32 = mean64[:, :-1], mean32[:, :-1]
        if kind is None:
            assert mc is None
        elif kind == "logits":
            check("masks C=%d logits" % C, rel_err(mc.cpu().numpy(), cls64), rel_err(cls32.numpy(), cls64))
        elif kind == "probs":
            e = np.exp(cls64 - cls64.max(1, keepdims=True))
            p64 = e / e.sum(1, keepdims=True)
            check("masks C=%d probs" % C, rel_err(mc.cpu().numpy(), p64), rel_err(torch.softmax(cls32, 1).numpy(), p64))
        else:
            got = mc.cpu().numpy()
            assert got.dtype == np.int64 and got.shape == (Fn, H, W)
            srt = np.sort(cls64, 1)
            safe = (srt[:, -1] - srt[:, -2]) > 1e-5
            assert safe.mean() > 0.99
            assert np.array_equal(got[safe], cls64.argmax(1)[safe])
