"""GPU tests of the wide linear heads (n_out 11 .. 64, the 42-channel YouTube-VIS semseg head): hip.wide_level_head and
hip.wide_heads_backward (csrc/decoder_backward.hip, v_mfma_f32_32x32x2_f32) against torch on the CPU, ``HeadsFunction`` on them, the wide
composed decoder behind ``SqueezeExpandTrunk.train_wide_head`` against the fp64 restatement of the reference decoder
(tests/wide_head_oracle.py), and ``TrainingModel.train_wide_head`` on the ``ytvis`` preset.

The tolerance is tests/decoder_tail_oracle.py's rule, imported: FACTOR x max(the case's own fp32-versus-fp64 spread, 2^-24) on the max norm;
in the composed f16x3 case the fp64 oracle's own change under 22-bit operands enters the max as well, as in
tests/test_gpu_decoder_training.py.  Every check prints spread, bound and device error before it asserts."""
import functools

import numpy as np
import pytest
import torch

from tests import conv3d_backward_oracle as CO
from tests import decoder_tail_oracle as TO
from tests import wide_head_cases as WC
from tests import wide_head_oracle as WO

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


@functools.lru_cache(maxsize=None)
def _ref(Cin, n_out, dims):
    c = WC.case(Cin, n_out, dims)
    return c, WC.oracle(c, torch.float32), WC.oracle(c, torch.float64)


def _run(hip, c):
    d = lambda a: torch.from_numpy(a).cuda()
    x, w, g, add = d(c["x"]), d(c["w"]), d(c["g"]), d(c["add"])
    dx, dw, db = hip.wide_heads_backward(x, w, g, want_dx=True, want_db=True)
    return dict(out=hip.wide_level_head(x, w), out_add=hip.wide_level_head(x, w, add), dx=dx, dw=dw, db=db), (x, w, g, add)


def _check_case(hip, Cin, n_out, dims):
    c, r32, r64 = _ref(Cin, n_out, dims)
    got, (x, w, g, add) = _run(hip, c)
    name = "Cin %d n_out %d %s" % (Cin, n_out, dims)
    bad = []
    for what in ("out", "out_add", "dx", "dw", "db"):
        assert got[what].shape == r64[what].shape
        TO.check(name, what, host(got[what]), r32[what], r64[what], bad)
    # the optional results leave the others the same bits; two runs are the same bits
    _, dw2, none = hip.wide_heads_backward(x, w, g, want_dx=False, want_db=False)
    assert none is None and _ is None and torch.equal(dw2, got["dw"])
    dx3, dw3, db3 = hip.wide_heads_backward(x, w, g, want_dx=True, want_db=True)
    assert torch.equal(dx3, got["dx"]) and torch.equal(dw3, got["dw"]) and torch.equal(db3, got["db"])
    assert torch.equal(hip.wide_level_head(x, w, add), got["out_add"]) and torch.equal(hip.wide_level_head(x, w), got["out"])
    # adjoint: <W x, g> = <x, W^T g>, both from the device results in fp64, within the rule's bound on the scale of the terms' sum
    lhs, rhs = float((host(got["out"]) * c["g"]).sum()), float((c["x"].astype(np.float64) * host(got["dx"])).sum())
    scale = float(np.abs(r64["out"] * c["g"]).sum())
    spread = max(TO.max_norm_err(r32["out"], r64["out"]), TO.max_norm_err(r32["dx"], r64["dx"]))
    b = TO.FACTOR * max(spread, TO.FP32_ROUNDING)
    print("%s adjoint  <Wx, g> %.9e <x, W^T g> %.9e |diff| / sum|terms| %.2e bound %.2e" % (name, lhs, rhs, abs(lhs - rhs) / scale, b))
    if not abs(lhs - rhs) <= b * scale:
        bad.append((name, "adjoint", abs(lhs - rhs) / scale, b))
    assert not bad, bad


@pytest.mark.parametrize("Cin", WC.CIN)
@pytest.mark.parametrize("n_out", WC.N_OUT)
def test_forward_and_backward_vs_torch(hip, n_out, Cin):
    """V = 2, 30 (rows without 16-byte alignment) and 512 (16 one-tile chunks): forward with and without ``add``, dx, dw, db by the rule;
    dx and db optional without changing the rest; reruns bit-equal; the adjoint identity."""
    for dims in WC.DIMS:
        _check_case(hip, Cin, n_out, dims)


@pytest.mark.parametrize("dims", WC.CHUNKED_DIMS)
def test_three_and_more_chunks_with_a_ragged_last_one(hip, dims):
    V = dims[0] * dims[1] * dims[2]
    n = hip.wide_heads_backward_chunks(256, 42, V)
    print("V %d: %d chunks" % (V, n))
    assert n >= 3 and V % WC.TILE and n == WC.expected_chunks(V)
    _check_case(hip, 256, 42, dims)
    _check_case(hip, 36, 33, dims)


@pytest.mark.parametrize("n_out,Cin", [(11, 4), (42, 36), (64, 256), (33, 256)])
def test_one_hot_upstream_is_exact(hip, n_out, Cin):
    """dz one at a single (o, v): dx[:, v] == w[o, :] and dw[o, :] == x[:, v] bit for bit, everything else exactly zero; db[o] == 1."""
    dims = (2, 3, 5) if Cin < 256 else (4, 8, 16)
    c = WC.case(Cin, n_out, dims)
    x, w = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["w"]).cuda()
    for o, t, y, xx in WC.one_hot_positions(n_out, dims):
        g = torch.zeros((n_out,) + dims, device="cuda")
        g[o, t, y, xx] = 1.0
        dx, dw, db = hip.wide_heads_backward(x, w, g, want_dx=True, want_db=True)
        edx, edw, edb = torch.zeros_like(x), torch.zeros_like(w), torch.zeros(n_out, device="cuda")
        edx[:, t, y, xx] = w[o]
        edw[o] = x[:, t, y, xx]
        edb[o] = 1.0
        assert torch.equal(dx, edx) and torch.equal(dw, edw) and torch.equal(db, edb), (o, t, y, xx)


@pytest.mark.parametrize("n_out,Cin,dims", [(42, 36, (2, 3, 5)), (33, 256, (1, 7, 11)), (11, 4, (1, 1, 2)), (64, 256, (4, 8, 16)),
                                             (42, 256, (1, 5, 20)), (32, 36, (1, 5, 20))])
def test_padding_rows_and_bounds(hip, n_out, Cin, dims):
    """x, dz, w and add each in a larger allocation whose remainder is NaN; every output in front of guard words: the results are finite and
    the bits of the plain-allocation run, the guards untouched (nothing behind the n_out rows or the V voxels is read or written)."""
    from stemseg_amd.hip import check, lib, ptr, stream
    c = WC.case(Cin, n_out, dims)
    plain, _ = _run(hip, c)
    V = dims[0] * dims[1] * dims[2]
    GUARD, SENT = 4096, -12345.0

    def in_nan(a):
        buf = torch.full((a.size + GUARD,), float("nan"), device="cuda")
        buf[:a.size] = torch.from_numpy(a).cuda().reshape(-1)
        return buf

    def guarded(n):
        return torch.full((n + GUARD,), SENT, device="cuda")
    x, w, g, add = in_nan(c["x"]), in_nan(c["w"]), in_nan(c["g"]), in_nan(c["add"])
    out, out_add, dx, dw, db = guarded(n_out * V), guarded(n_out * V), guarded(Cin * V), guarded(n_out * Cin), guarded(n_out)
    nb = lib().stemseg_hip_wide_heads_backward_workspace_bytes(Cin, n_out, V)
    ws = torch.full((nb // 4 + GUARD,), SENT, device="cuda")
    check(lib().stemseg_hip_wide_level_head(ptr(x), Cin, V, ptr(w), n_out, None, ptr(out), stream()))
    check(lib().stemseg_hip_wide_level_head(ptr(x), Cin, V, ptr(w), n_out, ptr(add), ptr(out_add), stream()))
    check(lib().stemseg_hip_wide_heads_backward(ptr(x), Cin, V, ptr(w), n_out, ptr(g), ptr(dx), ptr(dw), ptr(db), ptr(ws), nb, stream()))
    for name, buf, n in (("out", out, n_out * V), ("out_add", out_add, n_out * V), ("dx", dx, Cin * V), ("dw", dw, n_out * Cin), ("db", db, n_out)):
        assert bool(torch.isfinite(buf[:n]).all()), name
        assert torch.equal(buf[:n], plain[name].reshape(-1)), name
        assert bool((buf[n:] == SENT).all()), name + ": guard words overwritten"
    assert bool((ws[nb // 4:] == SENT).all()), "workspace guard words overwritten"
    assert bool(torch.isfinite(ws[:nb // 4].view(torch.float64)).all()), "every workspace slot is written"


def test_heads_function_runs_the_wide_entry_points(hip):
    from stemseg_amd.modeling.ops import HeadsFunction
    c = WC.case(36, 42, (2, 3, 5))
    d = lambda a: torch.from_numpy(a).cuda()
    x, w, g = d(c["x"]).requires_grad_(True), d(c["w"]).requires_grad_(True), d(c["g"])
    for act, axes in ((None, None), ([0] * 42, [0] * 42)):
        out = HeadsFunction.apply(x, w, None, act, axes, None)
        assert torch.equal(out, hip.wide_level_head(x.detach(), w.detach()))
        gx, gw = torch.autograd.grad(out, (x, w), g)
        dx, dw, _ = hip.wide_heads_backward(x.detach(), w.detach(), g)
        assert torch.equal(gx, dx) and torch.equal(gw, dw)
    out = HeadsFunction.apply(x.detach(), w, None, None, None, None)      # x needs no gradient: dx is not computed, dw the same bits
    assert torch.equal(torch.autograd.grad(out, w, g)[0], dw)
    with pytest.raises(NotImplementedError, match="with an activation"):
        HeadsFunction.apply(x, w, None, [0] * 41 + [2], [0] * 42, None)
    with pytest.raises(NotImplementedError, match="65 output channels"):
        HeadsFunction.apply(x, torch.zeros(65, 36, device="cuda"), None, None, None, None)


# ------------------------------------------------------------------------------------------------ the composed decoder
@functools.lru_cache(maxsize=None)
def _composed(T):
    """The wide decoder, its input and the oracle's output and gradients (fp32, fp64, fp64 on rounded operands): once per T."""
    m = WO.init_wide_decoder(T).cuda()
    m.train_wide_head = True
    seed, margin, tried = WO.select_seed(T, m)
    print("wide T %d: seed %d, min |pre-ReLU| %.2e" % (T, seed, margin))
    feats = CO.features(T, seed)
    H4, W4 = CO.MAP_SIZES[3]
    up = torch.randn((WO.N_OUT, T, H4, W4), generator=torch.Generator().manual_seed(7))
    grad = lambda dt, rounded=False: WO.decoder_gradients(m, T, feats, up, dt, rounded)
    return dict(m=m, feats=feats, up=up, r32=grad(torch.float32), r64=grad(torch.float64), r22=grad(torch.float64, True))


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("T", [4, 8])
def test_wide_composed_decoder_vs_the_reference_decoder(hip, T, precision):
    """in = inter = 32 channels, GroupNorm(8), 41 classes + foreground, a 4x map of 8 x 16, switch on.  forward_trainable (folded) against
    the fp64 oracle within the rule's bound b and against run_hip(...)[:42] (step by step, padded MFMA head) within 2 b -- both lie within
    b of fp64; the gradient of every parameter against the oracle by the rule, the key set complete; the same bits on a second pass."""
    k = _composed(T)
    m = k["m"]
    m.precision = precision
    for p in m.parameters():
        p.grad = None
    feats = [f.cuda() for f in k["feats"]]
    (g32, o32), (g64, o64), (g22, o22) = k["r32"], k["r64"], k["r22"]
    out = m.forward_trainable(feats)
    assert tuple(out.shape) == o64.shape == (42, T) + CO.MAP_SIZES[3]
    spread, change = TO.max_norm_err(o32, o64), (TO.max_norm_err(o22, o64) if precision == "f16x3" else 0.0)
    b = TO.bound(max(spread, change), o64)
    err = TO.max_norm_err(host(out), o64)
    ref = m.run_hip(feats, 0)[:42]
    dist = TO.max_norm_err(host(out), host(ref))
    print("wide T %d %s forward: spread %.2e 22-bit change %.2e bound %.2e device %.2e; vs run_hip %.2e (bound %.2e); run_hip vs fp64 %.2e"
          % (T, precision, spread, change, b, err, dist, 2 * b, TO.max_norm_err(host(ref), o64)))
    bad = []
    if not err <= b:
        bad.append(("forward", err, b))
    if not dist <= 2 * b:
        bad.append(("forward vs run_hip", dist, 2 * b))
    out.backward(k["up"].cuda())
    got = {n: host(p.grad) for n, p in m.named_parameters() if p.grad is not None}
    assert set(got) == set(g64) == {n for n, _ in m.named_parameters()}, sorted(set(got) ^ set(g64))
    for n in sorted(got):
        r64 = g64[n]
        spread, err = TO.max_norm_err(g32[n], r64), TO.max_norm_err(got[n], r64)
        change = TO.max_norm_err(g22[n], r64) if precision == "f16x3" else 0.0
        b = TO.bound(max(spread, change), r64)
        print("wide T %d %s %-28s spread %.2e 22-bit change %.2e bound %.2e device %.2e" % (T, precision, n, spread, change, b, err))
        if not err <= b:
            bad.append((n, err, b))
    for p in m.parameters():
        p.grad = None
    out2 = m.forward_trainable(feats)
    out2.backward(k["up"].cuda())
    assert torch.equal(out2, out)
    assert all(np.array_equal(host(p.grad), got[n]) for n, p in m.named_parameters()), "reruns differ"
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def ytvis(hip):
    """ytvis preset, R-50, one clip of 8 frames of 96 x 128 built as in tests/test_gpu_decoder_training.py; backbone frozen,
    ``train_decoders`` on: the refusal with ``train_wide_head`` off, then forward, the summed losses' backward and one SGD step with it on;
    then ``train_fpn`` and ``train_body`` on as well, one forward and backward.  Computed once for the tests below."""
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    from stemseg_amd.utils.constants import ModelOutput
    from tests import semseg_loss_oracle as SO
    from tests import synth
    E, S = ModelOutput.EMBEDDINGS, ModelOutput.SEMSEG_MASKS
    r = {}
    try:
        config.load_preset("ytvis")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        m = build_model()
        sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], 11)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()})
        m = m.cuda().eval()
        r["n_out"] = m.semseg_head.out_channels
        dec = m.decoder_parameters()
        for p in m.parameters():
            p.requires_grad_(False)
        for p in dec.values():
            p.requires_grad_(True)
        frames = (torch.from_numpy(synth.synth_frames(8, 96, 128, seed=3).astype(np.float32)).permute(0, 3, 1, 2) -
                  torch.tensor(config.cfg.INPUT.IMAGE_MEAN)[None, :, None, None])[None].cuda()
        _, masks, ig, cat = SO.make_sample(np.random.default_rng(5), 1, 8, 96, 128, (1, 17, 40))     # (category ids up to the last of the 40 classes)
        raw = lambda: [{"masks": torch.from_numpy(masks).cuda(), "ignore_masks": torch.from_numpy(ig).cuda(), "category_ids": torch.from_numpy(cat).cuda()}]
        m.train_decoders = True
        r["default"] = m.train_wide_head
        try:
            m(frames, raw())                                     # train_wide_head is off by default
        except NotImplementedError as e:
            r["refusal"] = str(e)
        m.train_wide_head = True
        with torch.no_grad():
            before = m(frames, raw())[ModelOutput.INFERENCE]
        out = m(frames, raw())
        loss = sum(out["optimization_losses"].values())
        r["loss_ok"] = bool(loss.requires_grad and torch.isfinite(loss))
        loss.backward()
        named = dict(m.named_parameters())
        r["decoder_keys"] = set(dec)
        r["filled"] = {k for k, p in named.items() if p.grad is not None}
        r["finite"] = all(bool(torch.isfinite(named[k].grad).all()) for k in r["filled"])
        r["all_zero"] = [k for k in r["filled"] if not named[k].grad.any()]
        torch.optim.SGD(list(dec.values()), lr=1e-3).step()
        with torch.no_grad():
            after = m(frames, raw())[ModelOutput.INFERENCE]
        r["moved"] = not torch.equal(after[E], before[E]) and not torch.equal(after[S], before[S])
        r["semseg_shape"] = tuple(after[S].shape)
        print("loss %.6f; %d decoder parameters, %d gradients, all-zero: %s" % (float(loss.detach()), len(dec), len(r["filled"]), r["all_zero"]))
        # ... and with the FPN and the body trainable too
        m.train_fpn = m.train_body = True
        want = dict(dec)
        want.update(m.fpn_parameters())
        want.update(m.body_parameters())
        for p in m.parameters():
            p.requires_grad_(False)
            p.grad = None
        for p in want.values():
            p.requires_grad_(True)
        out = m(frames, raw())
        sum(out["optimization_losses"].values()).backward()
        r["deep_keys"] = set(want)
        r["deep_filled"] = {k for k, p in named.items() if p.grad is not None}
        r["deep_finite"] = all(bool(torch.isfinite(named[k].grad).all()) for k in r["deep_filled"])
    finally:
        config.load_preset("defaults")
    return r


def test_ytvis_takes_a_training_step(ytvis):
    """Off by default: the NUM_CLASSES refusal.  On: a finite loss with a graph, .grad on exactly ``decoder_parameters()``, all finite, none
    all-zero, and after one SGD(lr = 1e-3) step the no-grad forward has moved."""
    assert ytvis["n_out"] == 42 and ytvis["default"] is False
    assert "NUM_CLASSES" in ytvis["refusal"] and "42 output channels" in ytvis["refusal"]
    assert ytvis["loss_ok"]
    assert ytvis["filled"] == ytvis["decoder_keys"], sorted(ytvis["filled"] ^ ytvis["decoder_keys"])
    assert ytvis["finite"] and not ytvis["all_zero"], ytvis["all_zero"]
    assert ytvis["moved"] and ytvis["semseg_shape"] == (1, 8, 42, 24, 32)


def test_ytvis_with_fpn_and_body_trainable_fills_exactly_their_gradients(ytvis):
    assert ytvis["deep_filled"] == ytvis["deep_keys"], sorted(ytvis["deep_filled"] ^ ytvis["deep_keys"])
    assert ytvis["deep_finite"] and any(k.startswith("backbone.body.") for k in ytvis["deep_keys"])
