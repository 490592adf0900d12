"""References of tests/test_gpu_conv_f32.py, all on the CPU: the inputs of a case, their fp64 convolution, the fp64 convolution of the
magnitudes (the scale of the derived rounding bound), and the yardstick -- a plain fp32 restatement of the same sum, one accumulator per
output, the K = Cin x taps products added one at a time.  Everything is computed once per (shape, epilogue) and shared by the cases that
differ in tile, split-K or layout only; the cached arrays are read-only."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_cases as cc

_DATA, _YARD = {}, {}


def data_key(case):
    e = cc.epi_set(case)
    key = (case.kind, case.Cin, case.Cout, case.T, case.H, case.W, case.inp == "dense", "nobias" in e, "relu" in e, bool(e & {"res", "reshalo"}))
    return key + (("stress",) if "stress" in e else ())          # (appended only where asked: every other case keeps its key, hence its random stream)


def _frozen(a):
    a.setflags(write=False)
    return a


def stress_activations(rs, shape):
    """Activations that stress the f16x3 split (csrc/split_operand.h: x / 4 = hi + lo in fp16, lo stored as lo * 2^11): signed magnitudes mixed
    log-uniformly over 2^-20 .. 2^17 in one tensor (hi subnormal below 2^-12), and a sixteenth of the elements each of +0, -0, values whose
    remainder * 2^11 is an exact tie between two fp16 numbers, values whose x / 4 is itself such a tie, and values just under 2.6e5 (hi at the top
    of fp16's range).  Every value is an exact fp32 number by construction."""
    n = int(np.prod(shape))
    sign = rs.choice([-1.0, 1.0], n)
    x = sign * 2.0 ** rs.uniform(-20.0, 17.0, n)
    idx, k = rs.permutation(n), n // 16
    e, m, q = rs.randint(-10, 14, k), rs.randint(0, 1024, k), rs.randint(0, 1023, k)
    s = sign[idx[:k]]
    x[idx[:k]] = 0.0
    x[idx[k:2 * k]] = -0.0
    x[idx[2 * k:3 * k]] = 4.0 * s * ((1024 + m) * 2.0 ** (e - 10) + (1024 + q + 0.5) * 2.0 ** (e - 22))      # hi = (1024 + m) 2^(e - 10), lo a tie
    x[idx[3 * k:4 * k]] = 4.0 * s * (1024 + m + 0.5) * 2.0 ** (e - 10)                                       # hi a tie
    x[idx[4 * k:5 * k]] = s * rs.uniform(2.55e5, 2.6e5, k)
    x32 = x.astype(np.float32)
    tie = np.r_[idx[2 * k:4 * k]]
    assert np.array_equal(x32[tie].astype(np.float64), x[tie]), "the tie values are fp32 numbers"
    return x32.reshape(shape)


def reference(case):
    """dict: x (the input VIEW's values, halo included: [Cin][T + kt - 1][H + kh - 1][W + kw - 1]; 1x1: [Cin][1][1][V]), w, b, res (or None),
    ref (fp64, the epilogue folded in), S (fp64: |x| conv |w| + |b| + |res|), K."""
    key = data_key(case)
    if key in _DATA:
        return _DATA[key]
    kind, Cin, Cout, T, H, W, dense_in, nobias, relu, has_res = key[:10]
    kt, kh, kw = cc.TAPS[kind]
    rs = np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)
    K = Cin * kt * kh * kw
    if kind == "k1":
        V = T * H * W
        x = rs.standard_normal((Cin, 1, 1, V)).astype(np.float32)
        if "stress" in key:
            x = stress_activations(rs, x.shape)
        oshape = (Cout, 1, 1, V)
    else:
        x = rs.standard_normal((Cin, T + kt - 1, H + 2, W + 2)).astype(np.float32)
        if "stress" in key:
            x = stress_activations(rs, x.shape)
        if not dense_in:                                   # the zero halo: what makes the valid cross-correlation a padding = 1 convolution
            halo = np.ones(x.shape[1:], bool)
            halo[(1 if kt == 3 else 0):(T + 1 if kt == 3 else T), 1:H + 1, 1:W + 1] = False
            x[:, halo] = 0.0
        oshape = (Cout, T, H, W)
    w = (rs.standard_normal((Cout, Cin, kt, kh, kw)) / np.sqrt(K)).astype(np.float32)
    b = None if nobias else rs.standard_normal(Cout).astype(np.float32)
    res = rs.standard_normal(oshape).astype(np.float32) if has_res else None
    xt, wt = torch.from_numpy(x).double()[None], torch.from_numpy(w).double()
    ref = F.conv3d(xt, wt)[0].numpy()
    S = F.conv3d(xt.abs(), wt.abs())[0].numpy()
    if b is not None:
        ref += b.astype(np.float64)[:, None, None, None]
        S += np.abs(b).astype(np.float64)[:, None, None, None]
    if res is not None:
        ref += res
        S += np.abs(res)
    if relu:
        ref = np.maximum(ref, 0.0)                         # (1-Lipschitz: every bound on the pre-activation error holds behind it)
    assert ref.shape == oshape
    d = dict(x=_frozen(x), w=_frozen(w), b=None if b is None else _frozen(b), res=None if res is None else _frozen(res), ref=_frozen(ref), S=_frozen(S),
             K=K, relu=relu)
    _DATA[key] = d
    return d


def subset_positions(case, seam_rows=()):
    """Output positions (t, y, x) the yardstick is evaluated on: K x Cout x positions <= 5e8 (at least 512, at most all), fixed random, always with
    the four corners of the first and last plane, one position on every edge of each, and -- row cuts -- eight positions on every seam row per plane."""
    T, H, W = (1, 1, case.T * case.H * case.W) if case.kind == "k1" else (case.T, case.H, case.W)
    K = case.Cin * int(np.prod(cc.TAPS[case.kind]))
    n_all = T * H * W
    n = int(min(n_all, max(512, 5e8 // (K * case.Cout))))
    rs = np.random.RandomState(12345)
    flat = set(rs.choice(n_all, size=n, replace=False).tolist())
    for t in sorted({0, T - 1}):
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, rs.randint(W)), (H - 1, rs.randint(W)), (rs.randint(H), 0), (rs.randint(H), W - 1)):
            flat.add((t * H + y) * W + x)
    for t in range(T):
        for y in seam_rows:
            for x in [0, W - 1] + rs.randint(W, size=6).tolist():
                flat.add((t * H + y) * W + x)
    flat = np.array(sorted(flat), np.int64)
    return flat // (H * W), (flat // W) % H, flat % W


def yardstick(case, seam_rows=()):
    """(positions, seq [Cout][P] fp32, e_seq): the sequential fp32 sum on the subset and its max-norm error against fp64."""
    key = (data_key(case), tuple(seam_rows))
    if key in _YARD:
        return _YARD[key]
    d = reference(case)
    kt, kh, kw = cc.TAPS[case.kind]
    t, y, x = pos = subset_positions(case, seam_rows)
    Cin, Cout = case.Cin, case.Cout
    # im2col on the subset: A[p][ci * taps + tap] = x[ci][t + dt][y + dy][x + dx], B[k][co] = w[co][k]
    A = np.empty((t.size, Cin, kt * kh * kw), np.float32)
    for dt in range(kt):
        for dy in range(kh):
            for dx in range(kw):
                A[:, :, (dt * kh + dy) * kw + dx] = d["x"][:, t + dt, y + dy, x + dx].T
    A = A.reshape(t.size, d["K"])
    B = np.ascontiguousarray(d["w"].reshape(Cout, d["K"]).T)
    acc = np.zeros((t.size, Cout), np.float32)
    for k in range(d["K"]):                                # one fp32 accumulator per output, two roundings per term
        acc += A[:, k, None] * B[k, None, :]
    if d["b"] is not None:
        acc += d["b"][None, :]
    if d["res"] is not None:
        acc += d["res"][:, t, y, x].T
    if d["relu"]:
        acc = np.maximum(acc, np.float32(0))
    assert acc.dtype == np.float32
    seq = acc.T
    e_seq = float(np.abs(seq.astype(np.float64) - d["ref"][:, t, y, x]).max())
    out = (pos, _frozen(seq), e_seq)
    _YARD[key] = out
    return out
