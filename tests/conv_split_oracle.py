"""The split modes' arithmetic restated in numpy, and the derived per-element cap of tests/test_gpu_conv_split.py -- CPU only.

The restatements follow csrc/split_operand.h and the MFMA stream of csrc/conv_igemm.h (`mm` in compute6):

  f16x3   activations xs = x / 4 = hx + lx, hx = fp16(xs), the low term stored as lx' = fp16((xs - hx) 2^11); weights ws = w S[co] (S a power of
          two per output channel, max|ws| in [2^13, 2^14)), hw = fp16(ws), lw = fp16(ws - hw), third operand hs = fp16(hw 2^-11).  Per k three
          exact products, in this order: lw hx, hs lx', hw hx.  The sum is scaled back by 1 / (S / 4), exactly.
  bf16x6  x = hx + mx + lx and w = hw + mw + lw, three bf16 terms each, exactly.  Per k six exact products, smallest first:
          lw hx, hw lx, mw mx, mw hx, hw mx, hw hx.

``restate`` accumulates them in fp32 the worst plausible way -- ONE accumulator per output, one product at a time in k order -- then bias,
residual and ReLU in fp32.  ``cap`` is the bound that run must respect (tests/test_conv_split_cap_host.py) before the device is held to it.

THE CAP.  |dev - ref64| <= (n_acc 2^-23 + c_mode) S + floor, per output, with S = sum_k |x_k| |w_k| + |b| + |res| (fp64):

  n_acc   accumulation steps: 3 K (f16x3) or 6 K (bf16x6) products added, K = Cin x taps, plus the ksplit slab additions and 4 for descale, bias,
          residual and the final store.  Each step rounds once, at most 2^-24 relative to a partial sum that never exceeds (1 + 2^-10) S; the cap
          grants 2^-23 per step as tests/test_gpu_conv_f32.py does, which also pays for that factor and for the O(n^2 u^2) terms.
  c_mode  what the products that are NOT formed amount to, relative to |x_k| |w_k|.
          f16x3: ws = hw + lw + ew and xs = hx + lx + ex with |lw| <= 2^-11 (1 + 2^-11) |ws|, |ew| <= 2^-22 |ws| (two roundings of 11 bits), the
          same for x.  Formed: lw hx + hw lx + hw hx.  ws xs minus that = lw lx + ew xs + ex ws - ew ex, at most
          (2^-22 (1 + 2^-11)^2 + 2 x 2^-22 + 2^-44) |ws xs| < 3 x 2^-22 (1 + 2^-10) |ws xs|.                                c_f16x3 = 3 x 2^-22 (1 + 2^-10)
          bf16x6: the split is exact (24 bits in three round-to-nearest terms of 8), |mx| <= 2^-9 (1 + 2^-9) |x|, |lx| <= 2^-18 |x|.  Dropped:
          mw lx + lw mx + lw lx <= (2 x 2^-27 (1 + 2^-9) + 2^-36) |w x| < 2^-26 (1 + 2^-8) |w x|.                               c_bf16x6 = 2^-26 (1 + 2^-8)
  floor   f16x3 only: where a term leaves fp16's normal range its rounding is absolute, 2^-25 (half a subnormal step).
          Activations: |xs| < 2^-14 gives |xs - hx| <= 2^-25 and then |lx 2^11| < 2^-14, so |ex| <= 2^-36 -- the same when only the low term is
          tiny.  In units of x that is 2^-34 per activation, times |w_k|; lw lx adds at most as much again in that case: 2 x 2^-34 |w_k| per k.
          Weights: |ew| <= 2^-25 when lw is subnormal, and hs = hw 2^-11 + eta with |eta| <= 2^-25 when |hw| < 2^-3.  Each meets at most |xs| =
          |x| / 4 and is scaled back by 4 / S[co], and 1 / S[co] <= 2^-13 max|w[co]|: 2 x 2^-38 max|w[co]| |x_k| per k.
          floor = 2^-33 sum_k |w_k| + 2^-37 max|w[co]| sum_k |x_k|.  (On N(0, 1) activations it is ~1e-3 of the cap; it carries the stress cases.)
          bf16x6: the terms have fp32's exponent range: no floor."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_cases as cc
from tests import conv_f32_oracle as oracle

PRODUCTS = {"f16x3": 3, "bf16x6": 6}
C_MODE = {"f16x3": 3 * 2.0 ** -22 * (1 + 2.0 ** -10), "bf16x6": 2.0 ** -26 * (1 + 2.0 ** -8)}
ACT_SCALE, LO_SCALE = np.float32(0.25), np.float32(2048.0)          # F16X3_ACT_SCALE, F16X3_LO_SCALE
_FLOOR = {}


def f16(a):
    return a.astype(np.float16).astype(np.float32)


def bf16(a):
    """Round-to-nearest-even to bf16, as fp32 (finite values)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7fff))) & np.uint32(0xffff0000)).view(np.float32)


def weight_scale(w2):
    """[Cout, K] -> [Cout] float32: f16x3_weight_scale of max|w[co]| (a power of two; 1 for an all-zero or non-finite channel)."""
    bits = np.abs(w2).max(1).astype(np.float32).view(np.uint32)
    e = ((bits >> 23) & 0xff).astype(np.int64)
    return np.where((e == 0) | (e == 0xff), 1.0, 2.0 ** np.clip(13 - (e - 127), -126, 127).astype(np.float64)).astype(np.float32)


def split_planes(prec, A, B):
    """A [P, K] activations, B [K, Cout] weights -> (list of (weight plane [K, Cout], activation plane [P, K]) in the kernel's product order,
    descale [Cout] float32)."""
    if prec == "f16x3":
        S = weight_scale(B.T)
        ws = B * S[None, :]
        hw = f16(ws)
        lw = f16(ws - hw)
        hs = f16(hw * np.float32(1.0 / 2048.0))
        xs = A * ACT_SCALE
        hx = f16(xs)
        lx = f16((xs - hx) * LO_SCALE)
        return [(lw, hx), (hs, lx), (hw, hx)], np.float32(1.0) / (S * ACT_SCALE)
    hw = bf16(B); r = B - hw; mw = bf16(r); lw = r - mw
    hx = bf16(A); r = A - hx; mx = bf16(r); lx = r - mx
    assert np.array_equal(bf16(lw), lw) and np.array_equal(bf16(lx), lx), "the third bf16 term is exact"
    return [(lw, hx), (hw, lx), (mw, mx), (mw, hx), (hw, mx), (hw, hx)], np.ones(B.shape[1], np.float32)


def subset(case, n=24):
    """A few of the yardstick's positions (corners and edges are among them), every channel."""
    t, y, x = oracle.subset_positions(case)
    pick = np.unique(np.r_[np.linspace(0, t.size - 1, n).astype(np.int64), 0, t.size - 1])
    return t[pick], y[pick], x[pick]


def restate(case, prec):
    """(positions, out [Cout][P] float32): the mode's arithmetic on the subset, accumulated sequentially in fp32."""
    d = oracle.reference(case)
    kt, kh, kw = cc.TAPS[case.kind]
    t, y, x = pos = subset(case)
    A = np.empty((t.size, case.Cin, kt * kh * kw), np.float32)
    for dt in range(kt):
        for dy in range(kh):
            for dx in range(kw):
                A[:, :, (dt * kh + dy) * kw + dx] = d["x"][:, t + dt, y + dy, x + dx].T
    A = A.reshape(t.size, d["K"])
    B = np.ascontiguousarray(d["w"].reshape(case.Cout, d["K"]).T)
    terms, descale = split_planes(prec, A, B)
    acc = np.zeros((t.size, case.Cout), np.float32)
    for k in range(d["K"]):
        for wp, xp in terms:
            prod = xp[:, k, None] * wp[k, None, :]                 # (exact: 22 / 16 significand bits)
            acc += prod
    acc *= descale[None, :]
    if d["b"] is not None:
        acc += d["b"][None, :]
    if d["res"] is not None:
        acc += d["res"][:, t, y, x].T
    if d["relu"]:
        acc = np.maximum(acc, np.float32(0))
    assert acc.dtype == np.float32
    return pos, acc.T


def floor_term(case, prec):
    """[Cout][T][H][W] fp64 (or 0.0): the absolute part of the cap."""
    if prec != "f16x3":
        return 0.0
    key = oracle.data_key(case)
    if key not in _FLOOR:
        d = oracle.reference(case)
        w2 = np.abs(d["w"].reshape(case.Cout, -1)).astype(np.float64)
        ones = torch.ones((1,) + d["w"].shape[1:], dtype=torch.float64)
        sum_x = F.conv3d(torch.from_numpy(np.abs(d["x"])).double()[None], ones)[0].numpy()          # [1][T][H][W]: sum_k |x_k|
        fl = 2.0 ** -33 * w2.sum(1)[:, None, None, None] + 2.0 ** -37 * w2.max(1)[:, None, None, None] * sum_x
        fl.setflags(write=False)
        _FLOOR[key] = fl
    return _FLOOR[key]


def cap(case, prec, ksplit):
    """The derived bound on |dev - ref64|, every output: (n_acc 2^-23 + c_mode) S + floor."""
    d = oracle.reference(case)
    n_acc = PRODUCTS[prec] * d["K"] + ksplit + 4
    return (n_acc * 2.0 ** -23 + C_MODE[prec]) * d["S"] + floor_term(case, prec)
