"""Plain references for the encoder's streaming passes (csrc/encoder.hip: space-to-depth, max-pool, stride-2 copy, FPN top-down add), the
launch functions' predicates restated in Python, and the inputs the tests of both sides share.  torch CPU and numpy only.

Top-down add, two references:
  (a) ``up2_restated``: up2_blend step by step in numpy -- m = f32(wx c01), h = f32(f64(1 - wx) f64(c00) + f64(m)) per coarse row, the same
      over the rows, then f32(fine + v); taps and weights from the scalar kernel's fp32 coordinate arithmetic.  The fp64 sum equals the
      correctly rounded FMA as long as it is exact: ``exact_fma_input`` draws |value| in [2^-8, 2^8] or 0, so a product (a quarter weight
      times a 24-bit value) and the rounded product it is added to span at most 44 significant bits.  Bit-exact yardstick.
  (b) ``up2_fp64``: fp64 fine + F.interpolate(coarse, scale_factor=2, bilinear, align_corners=False).  The expression rounds five times
      (two products and two FMAs of magnitude <= max|coarse|, one add of magnitude <= max|coarse| + max|fine|), each by at most 2^-24
      relative: ``up2_bound`` = 6 * 2^-24 * (max|coarse| + max|fine|).  Measured for (a) on such inputs from 2x2 to 30x54: at most 1.26 *
      2^-24 of that scale.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ predicates (csrc/encoder.hip, restated)
STREAM_SCALAR, STREAM_VEC4 = 1, 2
UP2_SCALAR, UP2_VEC4X2, UP2_DENSE = 1, 2, 3


def stride2_form(planes, H, W, aligned=True):
    """Max-pool and stride-2 copy of [planes][H][W]: the 16-byte form where a row is whole groups of eight inputs."""
    return STREAM_VEC4 if W % 8 == 0 and planes * (H // 2) * (W // 8) < 2 ** 31 and aligned else STREAM_SCALAR


def padded2d(C, T, H, W):
    """The encoder's y/x-zero-haloed layout [C][T][H + 2][pitch]."""
    pitch = (W + 2 + 3) // 4 * 4
    ts = (H + 2) * pitch
    return dict(pitch=pitch, ts=ts, cs=T * ts, total=C * T * ts + 64, interior=pitch + 1)


def up2_groups(W):
    return (W + 1) // 4 + 1


def up2_form(planes, H, W, ts, pitch, aligned=True, dense=False, dense_aligned=True):
    """Top-down add into a fine map [planes][H][W] (H, W even) of haloed geometry (ts, pitch).  dense: the fine term comes from a dense map,
    which only the dense form reads (0: it does not apply)."""
    gq = up2_groups(W)
    common = pitch % 4 == 0 and 4 * gq <= pitch and aligned and ts % 4 == 0
    if dense:
        return UP2_DENSE if common and W % 4 == 0 and planes * (H // 2 + 1) * gq < 2 ** 32 - 256 and dense_aligned else 0
    return UP2_VEC4X2 if common and planes * H * gq < 2 ** 32 - 256 else UP2_SCALAR


def encoder_stream_forms(T, H, W):
    """What stemseg_hip_encoder_stream_forms reports: max-pool, stride-2 copy of stages 2-4, top-down add of levels 4x, 8x, 16x."""
    out = [stride2_form(64 * T, H // 2, W // 2)]
    out += [stride2_form((256 << (st - 1)) * T, H >> (1 + st), W >> (1 + st)) for st in (1, 2, 3)]
    for k in range(3):
        h, w = H >> (2 + k), W >> (2 + k)
        g = padded2d(256, T, h, w)
        out.append(up2_form(256 * T, h, w, g["ts"], g["pitch"], dense=True) or up2_form(256 * T, h, w, g["ts"], g["pitch"]))
    return out


# ------------------------------------------------------------------------------------------------ max-pool, stride-2 copy, space-to-depth
def maxpool_ref(x):
    """[planes, H, W] float32 -> torch CPU max_pool2d(3, 2, 1) in fp32 (NaN propagates)."""
    return F.max_pool2d(torch.from_numpy(np.ascontiguousarray(x))[None], 3, 2, 1)[0].numpy()


def subsample_ref(x):
    return np.ascontiguousarray(x[:, ::2, ::2])


def s2d_geometry(T, H, W):
    pitch = (W // 2 + 3 + 3) // 4 * 4
    ts = (H // 2 + 3) * pitch
    return dict(pitch=pitch, ts=ts, cs=T * ts, floats=12 * T * ts)


def s2d_ref(frames, fill=0.0):
    """frames [T, 3, H, W] -> [12, T, H/2 + 3, pitch]: S[(p*2+q)*3+c][t][Y + 2][X + 2] = frames[t][c][2Y + p][2X + q], ``fill`` elsewhere."""
    T, _, H, W = frames.shape
    H2, W2 = H // 2, W // 2
    s2d = torch.from_numpy(np.ascontiguousarray(frames)).reshape(T, 3, H2, 2, W2, 2).permute(3, 5, 1, 0, 2, 4).reshape(12, T, H2, W2)
    buf = np.full((12, T, H2 + 3, s2d_geometry(T, H, W)["pitch"]), fill, np.float32)
    buf[:, :, 2:2 + H2, 2:2 + W2] = s2d.numpy()
    return buf


def nonfinite_planes(H, W, rows, cols, seed, base=None):
    """[3 * positions, H, W]: one of +inf, -inf, NaN per plane, at every (row, column) of ``rows`` x ``cols`` that exists and one interior
    point; the rest of a plane is random (or ``base``'s generator)."""
    pos = sorted({(y, x) for y in rows for x in cols if 0 <= y < H and 0 <= x < W} | {(H // 2, W // 2)})
    vals = (np.inf, -np.inf, np.nan)
    x = (base or rand)((len(vals) * len(pos), H, W), seed)
    for i, (v, (py, px)) in enumerate((v, p) for v in vals for p in pos):
        x[i, py, px] = v
    return x


def rand(shape, seed, scale=1.0, shift=0.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale + shift).astype(np.float32)


# ------------------------------------------------------------------------------------------------ top-down add
def exact_fma_input(shape, seed):
    """|value| in [2^-8, 2^8], or exactly 0 (one in nine), either sign: see the module docstring."""
    rs = np.random.RandomState(seed)
    v = np.exp2(rs.uniform(-8.0, 8.0, shape)) * rs.choice([-1.0, 1.0], shape)
    v[rs.randint(0, 9, shape) == 0] = 0.0
    v = v.astype(np.float32)
    a = np.abs(v[v != 0])
    assert a.size == 0 or (a.min() >= 2.0 ** -8 and a.max() <= 2.0 ** 8)
    return v


def _taps(n_fine, n_coarse):
    """The scalar kernel's fp32 coordinate arithmetic -> (i0, i1, w) per fine index."""
    i = np.arange(n_fine, dtype=np.float32)
    s = np.float32(0.5) * (i + np.float32(0.5)) - np.float32(0.5)
    s = np.where(s < 0, np.float32(0), s).astype(np.float32)
    i0 = s.astype(np.int32)
    i1 = i0 + (i0 < n_coarse - 1)
    return i0, i1, (s - i0.astype(np.float32)).astype(np.float32)


def _blend(a, b, w):
    """f32 fma(1 - w, a, f32(w b)) along the last axis' weights (w broadcasts)."""
    m = (w.astype(np.float64) * b.astype(np.float64)).astype(np.float32)                  # exact product, one rounding
    return ((np.float32(1) - w).astype(np.float64) * a.astype(np.float64) + m.astype(np.float64)).astype(np.float32)


def up2_restated(fine, coarse):
    """(a): fine [..., H, W] + bilinear_x2(coarse [..., H/2, W/2]) with up2_blend's rounding steps."""
    H, W = fine.shape[-2:]
    y0, y1, wy = _taps(H, coarse.shape[-2])
    x0, x1, wx = _taps(W, coarse.shape[-1])
    with np.errstate(invalid="ignore", over="ignore"):
        h0 = _blend(coarse[..., y0, :][..., x0], coarse[..., y0, :][..., x1], wx)
        h1 = _blend(coarse[..., y1, :][..., x0], coarse[..., y1, :][..., x1], wx)
        v = _blend(h0, h1, wy[:, None])
        return (fine + v).astype(np.float32)


def up2_fp64(fine, coarse):
    """(b): fp64 fine + F.interpolate(coarse, scale_factor=2, mode="bilinear", align_corners=False)."""
    c = torch.from_numpy(np.ascontiguousarray(coarse)).double().reshape((1, -1) + coarse.shape[-2:])
    up = F.interpolate(c, scale_factor=2, mode="bilinear", align_corners=False).reshape(fine.shape)
    return (torch.from_numpy(np.ascontiguousarray(fine)).double() + up).numpy()


def up2_bound(fine, coarse):
    return 6.0 * U * (float(np.abs(coarse).max()) + float(np.abs(fine).max()))


# (C, T, H, W) of the fine map: coarse 1x1; one row / one column of coarse; odd plane counts; W % 4 of 0 and 2; several groups per row
UP2_SHAPES = [(3, 1, 2, 2), (2, 1, 2, 4), (2, 1, 4, 2), (1, 3, 4, 6), (2, 2, 6, 12), (5, 1, 8, 8), (2, 1, 12, 20), (2, 2, 30, 54), (1, 2, 60, 108)]
# more elements than the 4096 x 256 threads of the scalar kernels' clamped grid
UP2_BIG = (4, 2, 256, 520)


def up2_inputs(shape, seed=None):
    C, T, H, W = shape
    seed = 1000 + H * W + C if seed is None else seed
    return exact_fma_input((C, T, H, W), seed), exact_fma_input((C, T, H // 2, W // 2), seed + 1)


def up2_nonfinite_inputs(H, W, where, seed=7):
    """-> (fine [P, 1, H, W], coarse [P, 1, H/2, W/2]) with one of inf, -inf, NaN per plane in ``where`` ('coarse' | 'fine'): rows {0, 1, n - 1} x
    columns {0, 1, n - 1} of that map and one interior point."""
    Hc, Wc = H // 2, W // 2
    if where == "coarse":
        c = nonfinite_planes(Hc, Wc, (0, 1, Hc - 1), (0, 1, Wc - 1), seed, exact_fma_input)
        f = exact_fma_input((c.shape[0], H, W), seed + 1)
    else:
        f = nonfinite_planes(H, W, (0, 1, H - 1), (0, 1, W - 1), seed, exact_fma_input)
        c = exact_fma_input((f.shape[0], Hc, Wc), seed + 1)
    return f[:, None], c[:, None]
