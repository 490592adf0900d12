"""The cases of the wide linear heads' tests (csrc/decoder_backward.hip wide_level_head_kernel / wide_heads_bwd_kernel), shared by
tests/test_wide_head_host.py and tests/test_gpu_wide_heads.py.  The oracle is torch on the CPU in the dtype asked for; the yardstick is
tests/decoder_tail_oracle.py's rule (``check`` / ``bound``): FACTOR x max(the case's own fp32-versus-fp64 spread, 2^-24) on the max norm."""
import numpy as np
import torch

N_OUT = (11, 32, 33, 42, 64)       # the narrowest wide head, one full MFMA block, one row into the second, the YouTube-VIS head, two full blocks
CIN = (4, 36, 256)                 # less than one channel block of a wave, one and a bit, two workgroup blocks of 128
DIMS = ((1, 1, 2), (2, 3, 5), (4, 8, 16))      # V = 2, 30 (no multiple of 4: rows lose their 16-byte alignment), 512 (16 tiles of 32)
TILE = 32                          # voxels per tile of the kernels
MAX_CHUNKS = 256                   # the plan cuts V into at most this many chunks of whole tiles
# Up to 256 tiles a chunk is one tile.  The smallest shapes with at least three chunks and a ragged last one: V = 77 is three one-tile chunks,
# the last 13 voxels long; V = 17751 is 555 tiles, 3 to a chunk -- 185 chunks, whose last tile holds 23 voxels (the multi-tile path).  V = 100
# (four chunks, the last 4 voxels long) is a multiple of 4: the forward's 16-byte path with lanes past the end, which the other two (odd V) and
# V = 512 (whole groups) do not reach.
CHUNKED_DIMS = ((1, 7, 11), (1, 5, 20), (3, 61, 97))


def expected_chunks(V):
    tiles = -(-V // TILE)
    tpc = -(-tiles // MAX_CHUNKS)
    return -(-tiles // tpc)


def case(Cin, n_out, dims, seed=0):
    T, H, W = dims
    rng = np.random.default_rng(100003 * Cin + 1009 * n_out + 101 * T + 11 * H + W + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    g = f(n_out, T, H, W)
    g[rng.random(g.shape) < 0.1] = 0.0
    return dict(x=f(Cin, T, H, W), w=(f(n_out, Cin) / np.sqrt(Cin)).astype(np.float32), add=f(n_out, T, H, W), g=g)


def oracle(c, dtype):
    """-> dict(out, out_add, dx, dw, db) as float64 numpy: out = w x, out_add = w x + add, the gradients of sum(out * g)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    x, w = t(c["x"]).requires_grad_(True), t(c["w"]).requires_grad_(True)
    out = torch.einsum("oc,cthw->othw", w, x)
    out.backward(t(c["g"]))
    n = lambda a: a.detach().double().numpy()
    return dict(out=n(out), out_add=n(out + t(c["add"])), dx=n(x.grad), dw=n(w.grad), db=n(t(c["g"]).sum((1, 2, 3))))


def one_hot_positions(n_out, dims):
    """(o, t, y, x): the corners and an interior voxel, at o = 0, n_out - 1 and 32 where it exists."""
    T, H, W = dims
    vox = sorted({(t, y, x) for t in (0, T - 1) for y in (0, H - 1) for x in (0, W - 1)} | {(T // 2, H // 2, W // 2)})
    return [(o,) + v for o in sorted({0, n_out - 1} | ({32} if n_out > 32 else set())) for v in vox]
