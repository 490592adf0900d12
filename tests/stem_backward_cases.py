"""The cases of the stem backward tests (csrc/stem_backward.hip), shared by the host and the GPU tests: the max-pool backward's maps and
upstreams, the shapes of the stem's weight gradient with a restatement of its chunk plan, and the composed stem + body case."""
import numpy as np

# ------------------------------------------------------------------------------------------------ the max-pool backward
# (planes, H, W): one window; odd Wo; odd Ho; several workgroups and rows that are no multiple of 4; the 16-byte form over several workgroups; and
# the 16-byte form's edges: one group a row and one row pair (no neighbour on any side), two groups (a left and a right edge, odd Ho), three (a group
# with neighbours on both sides)
POOL_CASES = ((1, 2, 2), (2, 4, 6), (3, 6, 10), (4, 34, 70), (5, 64, 128), (2, 2, 4), (3, 6, 8), (2, 10, 12))
SPECIALS = np.array([0.0, -0.0, 1e-45, 1e-40, np.inf, np.nan, 0.5, 1.0], np.float32)


def pool_input(planes, H, W, seed=0):
    """A map after a ReLU, quantised to halves so that most windows hold ties: about a third zeros, positive ties, +0.0 and -0.0, denormals,
    inf and NaN; where the map is large enough, two NaNs in one window (side by side and one above the other) and an inf beside a NaN."""
    rng = np.random.default_rng(1000 * planes + 10 * H + W + seed)
    x = (np.maximum(rng.standard_normal((planes, H, W)), 0.0) * 4).round().astype(np.float32) / 2
    flat = x.reshape(-1)
    n = max(1, min(flat.size // 4, 3 * SPECIALS.size)) if flat.size >= 8 else 0
    pos = rng.permutation(flat.size)[:n]
    flat[pos] = SPECIALS[np.arange(n) % SPECIALS.size]
    if H >= 4 and W >= 6:
        x[0, 1, 1] = x[0, 1, 2] = np.nan                      # one window, two NaNs in a row: the last one wins
        x[-1, 2, 3] = x[-1, 3, 3] = np.nan                    # ... one above the other
        x[-1, 0, 4], x[-1, 0, 5] = np.inf, np.nan
    return x


def pool_upstream(planes, H, W, seed=0):
    """g [planes, H/2, W/2]: normal values, a fifth of them zero, one -0.0."""
    rng = np.random.default_rng(77 + 1000 * planes + 10 * H + W + seed)
    g = rng.standard_normal((planes, H // 2, W // 2)).astype(np.float32)
    g[rng.random(g.shape) < 0.2] = 0.0
    g.reshape(-1)[-1] = -0.0
    return g


# ------------------------------------------------------------------------------------------------ the stem's weight gradient
WGRAD_HW = ((8, 8), (14, 22), (64, 96))                       # Ho x Wo = 4 x 4 (one ragged tile), 7 x 11 (ragged rows and columns), 32 x 48 (two tile columns, the second ragged)
WGRAD_F = (1, 2, 3)
WGRAD_SEVERAL = (3, 40, 72)                                   # 30 tiles: 8 chunks, the last of 2 tiles
WGRAD_CASES = tuple((Fr, H, W) for H, W in WGRAD_HW for Fr in WGRAD_F) + (WGRAD_SEVERAL,)
TILE_ROWS, TILE_COLS, MIN_TILES_PER_CHUNK, MAX_TILES_PER_CHUNK, TARGET_WORKGROUPS = 4, 32, 4, 8, 1024


def wgrad_plan(Fr, H, W):
    """-> (tiles, tiles per chunk, chunks): csrc/stem_backward.hip stem_wgrad_plan restated."""
    tiles = Fr * -(-(H // 2) // TILE_ROWS) * -(-(W // 2) // TILE_COLS)
    per = min(MAX_TILES_PER_CHUNK, max(MIN_TILES_PER_CHUNK, -(-tiles // TARGET_WORKGROUPS)))
    return tiles, per, -(-tiles // per)


def wgrad_case(Fr, H, W, seed=0):
    """frames [F, 3, H, W] like mean-subtracted pixels, and g [64, F, H/2, W/2] with a tenth of it zero."""
    rng = np.random.default_rng(31 * Fr + 7 * H + W + seed)
    frames = (rng.integers(0, 256, (Fr, 3, H, W)).astype(np.float32) - 110.0)
    g = rng.standard_normal((64, Fr, H // 2, W // 2)).astype(np.float32)
    g[rng.random(g.shape) < 0.1] = 0.0
    return frames, g


# ------------------------------------------------------------------------------------------------ the composed stem + body
STEM_F, STEM_HW = 2, (32, 64)                                 # the frames; the stem's map 16 x 32, layer1 on 8 x 16, then 4 x 8, 2 x 4, 1 x 2
STEM_STAGES = ((2, 64, 256), (2, 128, 512), (2, 256, 1024), (2, 512, 2048))      # (blocks, mid, Cout): an R-50's widths, two blocks a stage
RESNEXT_STAGES = ((2, 128, 256), (2, 256, 512), (2, 512, 1024), (2, 1024, 2048))  # a ResNeXt 32x4d's (32 groups of 4, 8, 16, 32 channels)


def stem_body_case(seed=0, groups=1, stages=STEM_STAGES):
    """frames, the stem's parameters (w [64, 3, 7, 7], FrozenBN scale and shift), per stage the blocks' parameters (the first block a
    projection; stride 2 from stage 2 on) and an upstream gradient on every stage output."""
    from tests import resnext_backward_oracle as RO
    rng = np.random.default_rng(9001 + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    H, W = STEM_HW
    case = dict(frames=(40.0 * f(STEM_F, 3, H, W)).astype(np.float32), stages=[], g=[], groups=groups,
                stem={"w": (f(64, 3, 7, 7) * np.sqrt(2.0 / 147) / 40.0).astype(np.float32), "s": rng.uniform(0.5, 1.5, 64).astype(np.float32),
                      "b": (0.2 * f(64)).astype(np.float32)})
    cin, h, w = 64, H // 4, W // 4
    for k, (nb, mid, cout) in enumerate(stages):
        if k:
            h, w = h // 2, w // 2
        case["stages"].append([RO.block_params(rng, cin if b == 0 else cout, mid, cout, b == 0, groups) for b in range(nb)])
        cin = cout
        case["g"].append(f(cout, STEM_F, h, w))
    return case
