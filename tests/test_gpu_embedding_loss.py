"""GPU tests of the embedding loss (csrc/embedding_loss.hip behind stemseg_amd.modeling.losses.EmbeddingLoss): the device against the
golden values of the reference's own EmbeddingLoss and against the fp64 oracle (tests/loss_oracle.py) on every fixture, at the training
shape (T = 8 on 120 x 216 maps, 6 and 20 instances), at N = 2 and with free dims -- both at 8 x 60 x 108 and on two cases of three and
four sort tiles with small instances --, each component's gradient on its own.

Bounds, per case.  The yardstick is the reference arithmetic's own fp32-versus-fp64 spread ON THE SAME INPUT: every test runs the
oracle in fp32 and in fp64 on its input and allows the device 4 x that case's own spread (its reductions run in another order), no
more; on the fixtures the reference's golden values against the fp64 oracle give the spread for the comparison with the goldens.
Errors are relative for a loss and max-norm over every element, relative to max|g|, for a gradient.  One floor, from the number
format: the device returns fp32 losses and gradient elements, and rounding a value to fp32 alone moves it by up to 2^-24 = 6.0e-8
relative, so a spread below 2^-24 (a case where the fp32 oracle happens to round well) counts as 2^-24.

Why the Lovasz gradient's spread grows with the instance size: the reference takes first differences of jaccard values in fp32; the
values are O(1), so each difference carries about 6e-8 absolute error while the differences themselves shrink like 1 / union.  At the
training shape 26 - 30 % of the non-zero Lovasz gradient elements of the fp32 oracle already differ from the fp64 one by more than
1e-4 max|g|.  The device divides in fp32 as the reference does, so it sits at about 1 x the spread.

    measured spread (CPU)      loss lovasz / smooth / seed     gradient lovasz / smooth / seed    device gradient error (MI355X)
    all_empty_batch            0 / 0 / 0                       0 / 0 / 0                          0 / 0 / 0
    empty_first_two            0 / 5.3e-8 / 3.1e-8             0 / 4.9e-8 / 3.8e-8                0 / 4.9e-8 / 3.9e-8
    empty_middle               2.6e-8 / 7.8e-8 / 1.4e-7        3.0e-6 / 6.7e-8 / 2.3e-7           2.9e-6 / 5.1e-8 / 6.6e-8
    n2_overlap                 1.8e-8 / 3.1e-8 / 4.7e-8        2.9e-6 / 9.3e-8 / 1.1e-7           3.0e-6 / 8.1e-8 / 6.4e-8
    sample_without_instances   1.2e-8 / 4.6e-8 / 5.8e-8        1.4e-6 / 8.3e-8 / 1.6e-7           1.3e-6 / 8.3e-8 / 1.7e-7
    xyff_free_dims             1.0e-8 / 6.2e-8 / 4.3e-8        2.2e-6 / 8.6e-8 / 2.6e-7           2.3e-6 / 4.8e-8 / 1.3e-7
    xyt                        8.7e-8 / 4.0e-8 / 1.3e-8        8.7e-6 / 5.4e-8 / 6.4e-8           8.7e-6 / 5.4e-8 / 6.5e-8
    xytf_n2                    4.7e-8 / 1.5e-8 / 3.4e-8        1.7e-6 / 8.4e-8 / 1.5e-7           1.7e-6 / 6.1e-8 / 1.4e-7
    tiles3_n2   (3 tiles)      5.4e-9 / 2.0e-9 / 1.5e-8        2.2e-5 / 7.8e-8 / 1.6e-7           2.2e-5 / 7.8e-8 / 9.1e-8
    tiles4_free_dims (4 tiles) 1.6e-7 / 3.6e-8 / 9.4e-8        7.0e-6 / 5.4e-8 / 1.7e-7           7.0e-6 / 5.3e-8 / 1.0e-7
    free_dims_mid (8x60x108)   9.1e-9 / 5.2e-8 / 6.0e-8        2.5e-4 / 8.4e-8 / 1.0e-7           2.4e-4 / 6.3e-8 / 7.8e-8
    n2_mid      (8x60x108)     2.3e-8 / 3.1e-8 / 4.4e-8        4.2e-4 / 9.1e-8 / 1.1e-7           4.2e-4 / 1.1e-7 / 1.0e-7
    train_i6    (8x120x216)    9.1e-8 / 1.2e-8 / 5.1e-8        1.5e-3 / 8.9e-8 / 1.1e-7           1.5e-3 / 6.8e-8 / 8.9e-8
    train_i20   (8x120x216)    1.4e-7 / 9.2e-8 / 7.2e-8        1.3e-3 / 8.3e-8 / 1.2e-7           1.3e-3 / 7.0e-8 / 1.3e-7
"""
import os

import numpy as np
import pytest
import torch

from tests import loss_oracle as LO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = LO.load_fixtures(os.path.join(ROOT, "tests", "golden", "embedding_loss.npz"))
FACTOR = 4                     # the device may be this many times the case's own fp32-vs-fp64 spread away from the fp64 oracle
FP32_ROUNDING = 2.0 ** -24     # rounding a result to fp32: the least spread a case is credited with (see the header)
NAMES = ("lovasz", "smoothness", "seediness")


def _module(E, stds):
    from stemseg_amd.modeling.losses import EmbeddingLoss
    return EmbeddingLoss(4, EMBEDDING_SIZE=E, NBR_FREE_DIMS=len(stds), FREE_DIM_STDS=list(stds), **LO.DEFAULT_WEIGHTS).cuda()


def _dev_targets(targets):
    return [{k: v.cuda() for k, v in t.items()} for t in targets]


def device_components(x, targets, E, stds):
    """-> (losses float64 numpy [3], three component gradients as float64 numpy) through the autograd function."""
    from stemseg_amd.modeling.losses import EmbeddingLossFunction
    mod = _module(E, stds)
    xx = x.cuda().requires_grad_(True)
    t = _dev_targets(targets)
    comps = EmbeddingLossFunction.apply(xx, [a["masks"] for a in t], [a["ignore_masks"] for a in t], E, mod._free_bw)
    grads = []
    for c in comps:
        g, = torch.autograd.grad(c, xx, retain_graph=True)
        grads.append(g.double().cpu().numpy())
    return np.array([float(c.detach()) for c in comps]), grads


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def _grad_err(g, ref):
    gmax = np.abs(ref).max()
    return np.abs(g - ref).max() / gmax if gmax else np.abs(g).max()


def _bound(spread):
    return FACTOR * max(spread, FP32_ROUNDING) if spread else 0.0      # (a zero spread is an exactly-zero term: the device must give 0 too)


def check_against_oracle(name, x, targets, E, stds):
    losses, grads = device_components(x, targets, E, stds)
    l32, g32 = LO.losses_and_grads(x, targets, E, stds, torch.float32)
    l64, g64 = LO.losses_and_grads(x, targets, E, stds, torch.float64)
    bad = []
    for k in range(3):
        lb, gb = _bound(_rel(l32[k], l64[k])), _bound(_grad_err(g32[k], g64[k]))
        rel, gerr = _rel(losses[k], l64[k]), _grad_err(grads[k], g64[k])
        print("%s %-10s loss %.9g (fp64 %.9g) rel %.2e (bound %.2e) | grad err / max|g| %.2e (bound %.2e)"
              % (name, NAMES[k], losses[k], l64[k], rel, lb, gerr, gb))
        if not rel <= lb:
            bad.append((NAMES[k], "loss", rel, lb))
        if not gerr <= gb:
            bad.append((NAMES[k], "grad", gerr, gb))
    assert not bad, bad
    return losses, grads, (l64, g64)


@pytest.mark.parametrize("name", sorted(LO.FIXTURE_CASES))
def test_fixture_vs_reference_and_fp64_oracle(name):
    f = FIXTURES[name]
    losses, grads, (l64, g64) = check_against_oracle(name, f["x"], f["targets"], f["E"], f["stds"])
    total, gtotal = LO.total_of(losses, grads)
    t64, gt64 = LO.total_of(l64, g64)
    for got, want, exact, what in zip([total] + list(losses), f["losses"], [t64] + list(l64), ("total",) + NAMES):
        rel, bound = _rel(got, want), _bound(_rel(want, exact))             # the reference's own distance from fp64 on this case
        print("%s %-10s device %.9g reference %.9g rel %.2e (bound %.2e)" % (name, what, got, want, rel, bound))
        assert rel <= bound, (what, got, want)
    gerr, bound = _grad_err(gtotal, f["grad"]), _bound(_grad_err(f["grad"], gt64))
    print("%s total grad vs reference: err / max|g| %.2e (bound %.2e)" % (name, gerr, bound))
    assert gerr <= bound


@pytest.mark.parametrize("name", sorted(LO.LARGE_CASES))
def test_large_vs_fp64_oracle(name):
    E, stds, _ = LO.LARGE_CASES[name]
    x, targets = LO.make_case(name, LO.LARGE_CASES)
    check_against_oracle(name, x, targets, E, stds)


def test_zero_instance_cases_give_exact_zeros():
    f = FIXTURES["all_empty_batch"]
    losses, grads = device_components(f["x"], f["targets"], f["E"], f["stds"])
    assert not losses.any() and not any(g.any() for g in grads)
    mod = _module(f["E"], f["stds"])
    xx = f["x"].cuda().requires_grad_(True)
    od = {}
    mod(xx, _dev_targets(f["targets"]), od)
    total = od["optimization_losses"]["embedding_loss"]
    total.backward()
    assert float(total.detach()) == 0 and all(float(v.detach()) == 0 for v in od["others"].values())
    assert xx.grad is not None and not xx.grad.any()
    # a sample without instances next to a regular one leaves its slice of the gradient at zero
    f = FIXTURES["sample_without_instances"]
    _, grads = device_components(f["x"], f["targets"], f["E"], f["stds"])
    assert all(not g[0].any() and not g[2].any() for g in grads) and grads[0][1].any()


@pytest.mark.parametrize("name", ["n2_overlap", "train_i6"])
def test_two_runs_give_identical_bits(name):
    if name in FIXTURES:
        f = FIXTURES[name]
        x, targets, E, stds = f["x"], f["targets"], f["E"], f["stds"]
    else:
        E, stds, _ = LO.LARGE_CASES[name]
        x, targets = LO.make_case(name, LO.LARGE_CASES)
    mod = _module(E, stds)
    t = _dev_targets(targets)
    runs = []
    for _ in range(2):
        xx = x.cuda().requires_grad_(True)
        od = {}
        mod(xx, t, od)
        od["optimization_losses"]["embedding_loss"].backward()
        runs.append((od["optimization_losses"]["embedding_loss"].detach(), [od["others"][k].detach() for k in sorted(od["others"])], xx.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert torch.equal(runs[0][2], runs[1][2])


def test_module_backward_equals_direct_c_abi_call():
    from stemseg_amd import hip
    f = FIXTURES["xytf_n2"]
    mod = _module(f["E"], f["stds"])
    t = _dev_targets(f["targets"])
    xx = f["x"].cuda().requires_grad_(True)
    od = {}
    mod(xx, t, od)
    od["optimization_losses"]["embedding_loss"].backward()
    x = f["x"].cuda()
    N, _, T, H, W = x.shape
    w = LO.DEFAULT_WEIGHTS
    up = torch.tensor([w["WEIGHT_LOVASZ"], w["WEIGHT_VARIANCE_SMOOTHNESS"], w["WEIGHT_SEEDINESS"]], dtype=torch.float32, device="cuda") * w["WEIGHT"]
    state, total = [], 0
    for n in range(N):
        desc = hip.embedding_loss_desc(f["E"], mod._free_bw, t[n]["masks"].shape[0], T, H, W)
        out, K, kept, ws = hip.embedding_loss_forward(desc, x[n], t[n]["masks"], t[n]["ignore_masks"])
        assert K == int((t[n]["masks"].reshape(t[n]["masks"].shape[0], -1).sum(1) > 0).sum()) and 0 < kept <= K
        total += K
        state.append((desc, ws, out))
    grad = torch.full_like(x, float("nan"))                          # every element is written
    for n, (desc, ws, _) in enumerate(state):
        hip.embedding_loss_backward(desc, x[n], t[n]["masks"], t[n]["ignore_masks"], ws, up, total, N, grad[n])
    assert torch.equal(grad, xx.grad)
    s = torch.stack([o for _, _, o in state]).sum(0).cpu()
    assert float(od["others"]["lovasz_loss"].detach()) == float(torch.tensor(float(s[0]) / total, dtype=torch.float64).float())
