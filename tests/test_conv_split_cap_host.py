"""The derived per-element cap of tests/test_gpu_conv_split.py, checked on the CPU before the device is held to it: the numpy restatement of each
split mode's arithmetic (tests/conv_split_oracle.py), accumulated in fp32 one product at a time, stays inside the cap on the inputs of every case
of conv_cases.SPLIT_CASES -- the stress inputs included.  If it did not, the cap would be wrong, not the inputs."""
import numpy as np
import pytest

from tests import conv_cases as cc
from tests import conv_f32_oracle as oracle
from tests import conv_split_oracle as so

_DONE = {}


def test_bf16_rounding_and_the_stress_inputs():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -7 + 2.0 ** -9), 3.0e38, 1e-30], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), 3.0e38, 1e-30], np.float32)
    got = so.bf16(a)
    assert np.array_equal(got[:4], want[:4]) and np.all(got.view(np.uint32) & 0xffff == 0) and np.all(np.abs(got - a) <= 2.0 ** -8 * np.abs(a))
    x = oracle.stress_activations(np.random.RandomState(3), (8, 1, 1, 4096)).ravel()
    assert (x == 0).sum() >= 2 * (x.size // 16) and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    assert np.abs(x).max() < 2.6e5 and np.isfinite(so.f16(x * np.float32(0.25))).all() and (np.abs(x[x != 0]).min() < 2.0 ** -19)
    xs = x.astype(np.float64) / 4
    r = (xs - so.f16(x * np.float32(0.25)).astype(np.float64)) * 2048.0
    lo = r.astype(np.float16).astype(np.float64)
    ties = np.abs(np.abs(r - lo) - 0.5 * np.spacing(np.abs(lo).astype(np.float16)).astype(np.float64)) == 0
    assert (ties & (r != 0)).sum() >= x.size // 16, "values whose scaled remainder is an exact tie"


@pytest.mark.parametrize("name,prec", cc.SPLIT_RUNS)
def test_restated_arithmetic_stays_inside_the_cap(name, prec):
    sc = cc.SPLIT_BY_NAME[name]
    case, ksplit = sc.case, sc.want[prec].ksplit
    key = (oracle.data_key(case), prec)
    if key not in _DONE:                                       # (cases that share their data share the restatement)
        d = oracle.reference(case)
        (t, y, x), out = so.restate(case, prec)
        err = np.abs(out.astype(np.float64) - d["ref"][:, t, y, x])
        S = d["S"][:, t, y, x]
        fl = so.floor_term(case, prec)
        fl = fl[:, t, y, x] if prec == "f16x3" else 0.0
        _DONE[key] = (err, S, fl, d["K"])
    err, S, fl, K = _DONE[key]
    bound = ((so.PRODUCTS[prec] * K + 1 + 4) * 2.0 ** -23 + so.C_MODE[prec]) * S + fl          # (ksplit 1: the tightest form of the cap)
    worst = float((err / (bound + 1e-300)).max())
    split_only = float((err / (so.C_MODE[prec] * S + fl + 1e-300)).max())
    print("CAP %-30s %-6s K %5d  max err/cap %.4f   (err over the split terms alone: %.3f)" % (name, prec, K, worst, split_only))
    assert np.isfinite(err).all() and (err <= bound).all(), "the restatement leaves the cap: worst %.3g x" % worst
    assert ksplit >= 1
