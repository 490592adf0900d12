"""csrc/optimizer.hip behind DeviceSGD / DeviceAdam / grad_norm against torch.optim.SGD / Adam on the CPU.

The rule is tests/decoder_tail_oracle.py's: the device may lie 4 x max(the case's own fp32-vs-fp64 spread, 2^-24) from the fp64 result,
max-norm per tensor; the fp64 result is the stock optimiser on the CPU in fp64, the spread the same in fp32, both from the identical fp32
inputs.  One parameter group of sizes 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 7, all stepped, plus one more tensor with
``grad = None``.  The CHUNK + 1 parameter, its gradient and its state are views at a storage offset of one element (4-byte aligned only: the
scalar path over two chunks); the CHUNK - 1 parameter has only its state there (a misaligned state alone must take the scalar path too).
Every tensor the kernels touch -- parameters, gradients, and the state tensors: Adam's from the first step on, SGD's momentum buffers from
the second (the optimiser allocates them itself in the first) -- sits in a NaN-filled buffer with guard words around it.  p, g ~ N(0, 1), lr 0.1: every term of the update lies far above the bound when it is wrong or missing."""
import math

import numpy as np
import pytest
import torch

from tests import decoder_tail_oracle as TO

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard words on either side of every tensor
LRS = (0.1, 0.05, 0.2)          # a changing learning rate over the three steps
SCALE = 0.37


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip
    hip.require_gpu()
    return hip


def sizes(hip):
    CH = hip.OPT_CHUNK
    return [1, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 7, 7]          # the issue's eight sizes, all stepped, and one more tensor that is skipped


UNALIGNED = 6                   # index of the size whose parameter, gradient and state lie one element into their storage (CHUNK + 1: two chunks on the scalar path)
STATE_SHIFTED = 4               # index of the size whose state alone lies one element into its storage (CHUNK - 1)
SKIPPED = 8                     # index of the parameter without a gradient
LAST_STEPPED = 7                # the last tensor that has a gradient


class Guarded(object):
    """A tensor of n floats inside a NaN-filled device buffer: GUARD words, (one more word for the 4-byte-aligned view,) the n elements,
    GUARD words."""

    def __init__(self, n, shift=0):
        self.buf = torch.full((GUARD + shift + n + GUARD + 3,), float("nan"), dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        lead = GUARD + shift
        self.view = self.buf[lead:lead + n]
        self.lead, self.n = lead, n
        assert self.view.data_ptr() % 16 == (4 * shift) % 16 and self.view.is_contiguous()

    def intact(self):
        b = self.buf
        return bool(torch.isnan(b[:self.lead]).all()) and bool(torch.isnan(b[self.lead + self.n:]).all())


def fresh_inputs(hip, seed):
    rng = np.random.default_rng(seed)
    ns = sizes(hip)
    p0 = [rng.standard_normal(n).astype(np.float32) for n in ns]
    gs = [[rng.standard_normal(n).astype(np.float32) for n in ns] for _ in LRS]
    return ns, p0, gs


def device_params(ns, p0):
    holders, params = [], []
    for i, (n, v) in enumerate(zip(ns, p0)):
        h = Guarded(n, shift=1 if i == UNALIGNED else 0)
        h.view.copy_(torch.from_numpy(v))
        p = torch.nn.Parameter(h.view)
        assert p.data_ptr() == h.view.data_ptr()
        holders.append(h)
        params.append(p)
    return holders, params


def set_grads(ns, params, g, holders):
    for i, (p, v) in enumerate(zip(params, g)):
        if i == SKIPPED:
            p.grad = None
            continue
        h = Guarded(ns[i], shift=1 if i == UNALIGNED else 0)
        h.view.copy_(torch.from_numpy(v))
        p.grad = h.view
        holders.append(h)


def guarded_like(i, n, values=None):
    """A state tensor for parameter ``i`` inside a guarded buffer: zeros, or a copy of ``values``."""
    h = Guarded(n, shift=1 if i in (UNALIGNED, STATE_SHIFTED) else 0)
    h.view.zero_() if values is None else h.view.copy_(values)
    return h


def guard_states(kind, opt, params, ns, holders):
    """Move the optimiser's state tensors into guarded buffers.  Adam: before the first step (zeros and a zero step count, as the class
    itself would start).  SGD: the momentum buffers the first step allocated, with their values."""
    for i, p in enumerate(params):
        if i == SKIPPED:
            continue
        if kind == "adam" and p not in opt.state:
            hs = [guarded_like(i, ns[i]), guarded_like(i, ns[i])]
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": hs[0].view, "exp_avg_sq": hs[1].view}
            holders += hs
        elif kind == "sgd" and p in opt.state and opt.state[p].get("momentum_buffer") is not None and not getattr(opt.state[p]["momentum_buffer"], "_guarded", False):
            h = guarded_like(i, ns[i], opt.state[p]["momentum_buffer"])
            h.view._guarded = True
            opt.state[p]["momentum_buffer"] = h.view
            holders.append(h)


def cpu_run(kind, kw, p0, gs, dtype, scale):
    """The stock optimiser on the CPU in ``dtype`` -> per step ([p], {name: [state]}).  The gradient scale is the first operation of the
    device's chain, so each oracle applies it in its own precision to the same fp32 g and fp32 scale."""
    params = [torch.nn.Parameter(torch.from_numpy(v).to(dtype).clone()) for v in p0]          # (a copy: the step writes in place)
    opt = (torch.optim.SGD if kind == "sgd" else torch.optim.Adam)(params, lr=LRS[0], **kw)
    steps = []
    for lr, g in zip(LRS, gs):
        opt.param_groups[0]["lr"] = lr
        for i, (p, v) in enumerate(zip(params, g)):
            gv = torch.from_numpy(v).to(dtype)
            p.grad = None if i == SKIPPED else (gv * torch.tensor(np.float32(scale)).to(dtype) if scale is not None else gv)
        opt.step()
        names = sorted({k for p in params for k in opt.state.get(p, {}) if k != "step"})
        steps.append(([p.detach().double().numpy().copy() for p in params],
                      {k: [opt.state[p][k].detach().double().numpy().copy() if k in opt.state.get(p, {}) and opt.state[p][k] is not None else None
                           for p in params] for k in names}))
    return steps


def device_run(hip, kind, kw, ns, p0, gs, scale):
    from stemseg_amd.training import DeviceAdam, DeviceSGD
    holders, params = device_params(ns, p0)
    opt = (DeviceSGD if kind == "sgd" else DeviceAdam)(params, lr=LRS[0], **kw)
    s = None if scale is None else torch.full((1,), scale, dtype=torch.float32, device="cuda")
    steps, grad_holders = [], []
    for lr, g in zip(LRS, gs):
        opt.param_groups[0]["lr"] = lr
        guard_states(kind, opt, params, ns, grad_holders)
        set_grads(ns, params, g, grad_holders)
        versions = [p._version for p in params]
        g_before = [None if p.grad is None else p.grad.clone() for p in params]
        opt.step(grad_scale=s)
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            if i == SKIPPED:
                assert p._version == versions[i] and p not in opt.state, "the parameter without a gradient was touched"
            else:
                assert p._version > versions[i], "the version counter of a stepped parameter did not move"
                assert torch.equal(p.grad.view(torch.int32), g_before[i].view(torch.int32)), "the step wrote into a gradient"
        names = sorted({k for p in params for k in opt.state.get(p, {}) if k != "step"})
        steps.append(([p.detach().cpu() for p in params],
                      {k: [opt.state[p][k].detach().cpu() if p in opt.state and k in opt.state[p] else None for p in params] for k in names}))
    assert all(h.intact() for h in holders + grad_holders), "a guard word was overwritten"
    return steps, opt, params


SGD_CASES = [(0.0, False, 0.0, 0.0), (0.9, False, 0.0, 0.0), (0.9, True, 1e-4, 0.0), (0.9, False, 1e-2, 0.5)]


def _check(name, hip, kind, kw, scale):
    ns, p0, gs = fresh_inputs(hip, 11)
    r32, r64 = cpu_run(kind, kw, p0, gs, torch.float32, scale), cpu_run(kind, kw, p0, gs, torch.float64, scale)
    dev, opt, params = device_run(hip, kind, kw, ns, p0, gs, scale)
    bad = []
    for step, ((dp, ds), (p32, s32), (p64, s64)) in enumerate(zip(dev, r32, r64)):
        assert sorted(ds) == sorted(s64), (sorted(ds), sorted(s64))
        for i, n in enumerate(ns):
            tag = "%s step %d n=%d" % (name, step, n)
            if i == SKIPPED:
                assert np.array_equal(dp[i].numpy(), p0[i]) and all(ds[k][i] is None and s64[k][i] is None for k in ds)
                continue
            TO.check(tag, "p", dp[i].numpy(), p32[i], p64[i], bad)
            for k in ds:
                assert ds[k][i] is not None and s64[k][i] is not None, (tag, k)
                TO.check(tag, k, ds[k][i].numpy(), s32[k][i], s64[k][i], bad)
    assert not bad, bad
    # same start, same bits
    again, _, _ = device_run(hip, kind, kw, ns, p0, gs, scale)
    for (dp, ds), (ap, as_) in zip(dev, again):
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(dp, ap)), "reruns differ"
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for k in ds for a, b in zip(ds[k], as_[k]) if a is not None)
    return opt


@pytest.mark.parametrize("scale", [None, SCALE])
@pytest.mark.parametrize("mu,nesterov,wd,dampening", SGD_CASES)
def test_sgd_three_steps_vs_torch(hip, mu, nesterov, wd, dampening, scale):
    opt = _check("sgd mu=%g nes=%d wd=%g damp=%g scale=%s" % (mu, nesterov, wd, dampening, scale), hip, "sgd",
                 dict(momentum=mu, nesterov=nesterov, weight_decay=wd, dampening=dampening), scale)
    if mu == 0.0:
        assert len(opt.state) == 0, "momentum 0 keeps no buffer"
    # every step of this test hands over freshly allocated gradients, so the key may change with each: at most one upload per step
    # (test_tables_are_kept_while_pointers_and_flags_stay pins the count when the pointers stay)
    assert opt.table_uploads <= len(LRS)


@pytest.mark.parametrize("scale", [None, SCALE])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_three_steps_vs_torch(hip, wd, scale):
    opt = _check("adam wd=%g scale=%s" % (wd, scale), hip, "adam", dict(weight_decay=wd), scale)
    steps = {float(s["step"]) for s in opt.state.values()}
    assert steps == {3.0} and all(not s["step"].is_cuda for s in opt.state.values())


def test_tables_are_kept_while_pointers_and_flags_stay(hip):
    """Gradients written in place (``zero_grad(set_to_none=False)``): one upload with fresh momentum buffers, one more once they are
    initialised, none after that whatever the learning rate."""
    from stemseg_amd.training import DeviceSGD
    ns, p0, gs = fresh_inputs(hip, 3)
    _, params = device_params(ns, p0)
    opt = DeviceSGD(params, lr=0.1, momentum=0.9, nesterov=True)
    for p in params:
        p.grad = torch.randn_like(p)
    for k in range(4):
        opt.param_groups[0]["lr"] = 0.1 / (k + 1)
        opt.step()
        opt.zero_grad(set_to_none=False)
        for p in params:
            p.grad.normal_()
    assert opt.table_uploads == 2


def test_zero_gradient_leaves_the_parameter_bits(hip):
    from stemseg_amd.training import DeviceSGD
    ns, p0, _ = fresh_inputs(hip, 5)
    for kw in (dict(momentum=0.9, nesterov=True), dict(momentum=0.0), dict(momentum=0.9)):
        _, params = device_params(ns, p0)
        for p in params:
            p.grad = torch.zeros_like(p)
        DeviceSGD(params, lr=0.1, weight_decay=0.0, **kw).step()
        torch.cuda.synchronize()
        for p, v in zip(params, p0):
            assert np.array_equal(p.detach().cpu().numpy().view(np.int32), v.view(np.int32))


def test_non_contiguous_gradient_is_read_through_a_copy(hip):
    from stemseg_amd.training import DeviceSGD
    p = torch.nn.Parameter(torch.randn(6, 4, device="cuda"))
    q = torch.nn.Parameter(p.detach().clone())
    g = torch.randn(4, 6, device="cuda").t()
    assert not g.is_contiguous()
    p.grad, q.grad = g, g.contiguous()
    DeviceSGD([p], lr=0.1, momentum=0.9).step()
    DeviceSGD([q], lr=0.1, momentum=0.9).step()
    assert torch.equal(p, q) and torch.equal(p.grad, g)


# ------------------------------------------------------------------------------------------------ gradient norm
def _norm_params(hip, seed, poison=None):
    ns, _, gs = fresh_inputs(hip, seed)
    holders, params = device_params(ns, [np.zeros(n, np.float32) for n in ns])
    g = [v.copy() for v in gs[0]]
    if poison is not None:
        g[LAST_STEPPED][-1] = poison                    # the last element of the last tensor that has a gradient
    set_grads(ns, params, g, holders)
    used = [v for i, v in enumerate(g) if i != SKIPPED]
    return params, used, holders


@pytest.mark.parametrize("max_norm_factor", [None, 0.5, 2.0])
def test_grad_norm_and_clip_coefficient(hip, max_norm_factor):
    """The norm within n 2^-52 relative of the exactly rounded fp64 value (every term is non-negative and every square exact, so each of the
    n - 1 additions adds at most 2^-53 relative, the square root halves that and adds its own rounding); coef within 2^-23 relative of the
    fp64 formula, exactly 1.0 for a norm below max_norm; no flag."""
    from stemseg_amd.training import grad_norm
    params, used, holders = _norm_params(hip, 21)
    n = sum(v.size for v in used)
    exact = math.sqrt(math.fsum(float(x) * float(x) for v in used for x in v.astype(np.float64)))
    max_norm = None if max_norm_factor is None else exact * max_norm_factor
    before = [p.grad.clone() for p in params if p.grad is not None]
    norm, coef, flag = grad_norm(params, max_norm)
    assert norm.dtype == torch.float64 and coef.dtype == torch.float32 and flag.dtype == torch.int32 and norm.is_cuda and coef.is_cuda and flag.is_cuda
    rel = abs(float(norm) - exact) / exact
    print("n %d norm %.17g exact %.17g rel %.3e bound %.3e" % (n, float(norm), exact, rel, n * 2.0 ** -52))
    assert rel <= n * 2.0 ** -52
    want = 1.0 if max_norm is None else min(1.0, max_norm / (exact + 1e-6))
    print("coef %.9g want %.9g" % (float(coef), want))
    if want == 1.0:
        assert float(coef) == 1.0
    else:
        assert abs(float(coef) - want) <= 2.0 ** -23 * want
    assert int(flag) == 0
    assert all(torch.equal(a, p.grad) for a, p in zip(before, [p for p in params if p.grad is not None]))
    assert all(h.intact() for h in holders)
    n2, c2, _ = grad_norm(params, max_norm)
    assert torch.equal(n2, norm) and torch.equal(c2, coef)              # same bits


@pytest.mark.parametrize("poison", [float("inf"), float("nan")])
def test_grad_norm_flags_a_non_finite_element(hip, poison):
    from stemseg_amd.training import grad_norm
    params, _, _ = _norm_params(hip, 22, poison)
    norm, coef, flag = grad_norm(params, 1.0)
    assert int(flag) == 1 and not math.isfinite(float(norm))
    params, _, _ = _norm_params(hip, 22)
    assert int(grad_norm(params, 1.0)[2]) == 0


def test_clip_coefficient_feeds_the_step_without_a_readback(hip):
    """grad_norm's coef handed to the step equals a step on coef * g."""
    from stemseg_amd.training import DeviceSGD, grad_norm
    ns, p0, gs = fresh_inputs(hip, 31)
    _, a = device_params(ns, p0)
    _, b = device_params(ns, p0)
    ha, hb = [], []
    set_grads(ns, a, gs[0], ha)
    set_grads(ns, b, gs[0], hb)
    _, coef, _ = grad_norm(a, 1.0)
    assert 0.0 < float(coef) < 1.0
    DeviceSGD(a, lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4).step(grad_scale=coef)
    for p in b:
        if p.grad is not None:
            p.grad = p.grad * coef
    DeviceSGD(b, lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4).step()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
