"""Torch restatement of the reference's training-target preparation (modeling/model_builder.py:128-152, data/common.py:195-210), semseg
cross-entropy (modeling/losses/cross_entropy.py:9-48) and foreground loss (model_builder.py:210-244), in fp32 or fp64, differentiable by
autograd.  Runs on the CPU (the yardstick of the tests) and, for timing only, on the GPU with stock torch ops
(tools/semseg_loss_bench.py).  Also the deterministic inputs of the fixtures (tools/make_semseg_loss_goldens.py) and of the GPU tests.

Three behaviours of the reference that this file restates and the goldens pin:
  1. bilinear interpolation by 1/4 (align_corners = False) of a 0 / 1 mask, cast to uint8, is the AND of source pixels
     (4y + 1 | 4y + 2, 4x + 1 | 4x + 2); output size floor(H / 4) x floor(W / 4), no tap is ever clamped;
  2. the semantic mask is the largest category id over the instances whose downscaled mask is set, 0 where none is;
  3. the cross-entropy is reduced with 'mean' BEFORE the ignore mask multiplies it: it is not masked, the mask only turns it into NaN
     (0 / 0) when every voxel of a sample is ignored, and autograd then gives NaN for every gradient element of that sample.  The
     foreground loss is masked."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ the three pieces
def prepare_targets(masks, ignore_masks, category_ids):
    """masks [I, T, H, W], ignore_masks [T, H, W] (0 / 1 or bool), category_ids [I] -> (masks uint8 [I, T, h, w], ignore uint8 [T, h, w],
    semantic mask int64 [T, h, w]), h = H // 4, w = W // 4."""
    def quarter(m):
        m = m != 0
        h, w = m.shape[-2] // 4, m.shape[-1] // 4
        taps = [m[..., dy:dy + 4 * h:4, dx:dx + 4 * w:4][..., :h, :w] for dy in (1, 2) for dx in (1, 2)]
        return taps[0] & taps[1] & taps[2] & taps[3]
    m, ig = quarter(masks), quarter(ignore_masks)
    cats = torch.as_tensor(category_ids).long().to(m.device)
    sem = torch.zeros(ig.shape, dtype=torch.int64, device=m.device)
    for i in range(m.shape[0]):
        sem = torch.where(m[i], torch.maximum(sem, cats[i]), sem)
    return m.to(torch.uint8), ig.to(torch.uint8), sem


def semseg_losses(logits, targets, n_classes, has_fg, dtype=torch.float32):
    """logits [N, C, T, h, w] (C = n_classes + has_fg, the foreground channel last); targets: prepared dicts with 'semseg_masks' and
    'ignore_masks' [T, h, w] -> (cross-entropy, foreground loss): scalars of ``dtype``, each the mean over the N samples (the foreground
    loss is 0 without that channel)."""
    x = logits.to(dtype)
    N, K = x.shape[0], n_classes
    ce, fg = x.sum() * 0, x.sum() * 0
    for n in range(N):
        sem = targets[n]["semseg_masks"].to(x.device).long()
        keep = 1. - (targets[n]["ignore_masks"].to(x.device) != 0).to(dtype)
        logp = torch.log_softmax(x[n, :K], 0)
        seq = -logp.gather(0, sem[None]).mean()                    # 'mean' over every voxel, ignored or not
        ce = ce + (seq * keep).sum() / keep.sum()
        if has_fg:
            z, y = x[n, K], (sem > 0).to(dtype)
            bce = z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))
            fg = fg + (bce * keep).sum() / keep.sum()
    return ce / N, fg / N


def losses_and_grads(logits, targets, n_classes, has_fg, dtype, device="cpu"):
    """-> (losses float64 numpy [2] = cross-entropy, foreground; their two gradients with respect to the logits as float64 numpy)."""
    xx = logits.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    comps = semseg_losses(xx, targets, n_classes, has_fg, dtype)
    grads = []
    for c in comps:
        g, = torch.autograd.grad(c, xx, retain_graph=True, allow_unused=True)
        grads.append(np.zeros(tuple(logits.shape)) if g is None else g.detach().double().cpu().numpy())
    return np.array([float(c.detach()) for c in comps]), grads


# ------------------------------------------------------------------------------------------------ deterministic inputs
def _blob(rng, T, H, W, lo=0.3):
    m = np.zeros((T, H, W), np.uint8)
    h, w = max(6, int(H * (lo + 0.3 * rng.random()))), max(6, int(W * (lo + 0.3 * rng.random())))
    y0, x0 = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
    m[rng.integers(0, max(1, T // 2)):, y0:y0 + h, x0:x0 + w] = 1
    return m & (rng.random((T, H, W)) < 0.93)                      # holes: the four taps of an output pixel disagree somewhere


def make_sample(rng, n_channels, T, H, W, cats, empty=False, overlap=True, ignore="part"):
    """-> (logits float32 [C, T, H // 4, W // 4], masks uint8 [I, T, H, W], ignore bool [T, H, W], category ids int64 [I]) at full
    resolution H x W.  overlap: False (the first instance wins a pixel) | True (as the boxes fall) | 'big' (boxes of 60 - 90 % of each
    axis: every pair overlaps).  ignore: 'part' | 'none' | 'all'."""
    I = len(cats)
    masks = np.zeros((I, T, H, W), np.uint8)
    if not empty:
        for i in range(I):
            masks[i] = _blob(rng, T, H, W, 0.6) if overlap == "big" else _blob(rng, T, H, W)
        if not overlap:
            seen = np.zeros((T, H, W), bool)
            for i in range(I):
                masks[i][seen] = 0
                seen |= masks[i] > 0
    if ignore == "all":
        ig = np.ones((T, H, W), bool)
    elif ignore == "none":
        ig = np.zeros((T, H, W), bool)
    else:
        ig = np.zeros((T, H, W), bool)
        ig[:, :H // 3, W // 4:] = rng.random((T, H // 3, W - W // 4)) < 0.9
    x = (2.0 * rng.standard_normal((n_channels, T, H // 4, W // 4))).astype(np.float32)
    return x, masks, ig, np.array(cats, np.int64)


# name -> (class channels K, foreground channel, WEIGHT_SEMSEG, [per-sample (T, H, W, category ids, empty, overlap, ignore)])
FIXTURE_CASES = {
    "k2_fg_n1": (2, True, 1.0, [(3, 32, 48, (1, 1), False, False, "part")]),
    "k3_fg_n2_kitti": (3, True, 1.0, [(2, 24, 40, (1, 2, 2), False, True, "part"), (2, 24, 40, (2, 1), False, False, "none")]),
    "k41_fg_ytvis_width": (41, True, 1.0, [(2, 24, 32, (40, 7, 23), False, True, "part")]),
    "k5_no_fg": (5, False, 1.0, [(2, 24, 32, (4, 2, 1), False, True, "part")]),
    "no_instances": (3, True, 1.0, [(2, 24, 32, (1, 2), True, False, "part"), (2, 24, 32, (2,), False, False, "part")]),
    "overlap_max_rule": (6, True, 1.0, [(2, 32, 32, (2, 5, 3, 4), False, "big", "none")]),
    "odd_18x23": (3, True, 1.0, [(3, 18, 23, (1, 2), False, True, "part")]),
    "odd_30x41_n2": (4, False, 1.0, [(2, 30, 41, (3, 1), False, True, "part"), (2, 30, 41, (2,), False, True, "none")]),
    "ignore_partly": (3, True, 1.0, [(2, 24, 32, (1, 2), False, True, "part")]),
    "ignore_all_n2": (3, True, 1.0, [(2, 24, 32, (1, 2), False, True, "all"), (2, 24, 32, (2, 1), False, True, "part")]),
    "weight_semseg_2p5": (3, True, 2.5, [(2, 24, 32, (2, 1), False, True, "part")]),
}

# T = 8 on 120 x 216 maps (480 x 864 frames) at the three head widths (KITTI without and with the foreground channel, YouTube-VIS), and N = 2
LARGE_CASES = {
    "train_c3": (3, False, 1.0, [(8, 480, 864, (1, 2, 2, 1, 2, 1), False, True, "part")]),
    "train_c4": (3, True, 1.0, [(8, 480, 864, (1, 2, 2, 1, 2, 1), False, True, "part")]),
    "train_c42": (41, True, 1.0, [(8, 480, 864, (40, 7, 23, 1, 12, 33), False, True, "part")]),
    "n2_c4": (3, True, 1.0, [(8, 240, 432, (1, 2, 2), False, True, "part"), (8, 240, 432, (2, 1), False, False, "none")]),
}


def make_case(name, cases=None, seed=None):
    """-> (logits float32 [N, C, T, h, w], raw targets: dicts with 'masks' uint8 [I, T, H, W], 'ignore_masks' bool [T, H, W] and
    'category_ids' int64 [I] at full resolution) for a case of FIXTURE_CASES (or of ``cases``)."""
    K, has_fg, _, samples = (cases or FIXTURE_CASES)[name]
    rng = np.random.default_rng(sum(map(ord, name)) if seed is None else seed)
    xs, targets = [], []
    for s in samples:
        x, masks, ig, cats = make_sample(rng, K + int(has_fg), *s)
        xs.append(x)
        targets.append({"masks": torch.from_numpy(masks), "ignore_masks": torch.from_numpy(ig), "category_ids": torch.from_numpy(cats)})
    return torch.from_numpy(np.stack(xs)), targets


def prepared(targets):
    """Raw targets -> new dicts with the oracle's 1/4-scale 'masks', 'ignore_masks' and 'semseg_masks' (the inputs stay as they are)."""
    out = []
    for t in targets:
        m, ig, sem = prepare_targets(t["masks"], t["ignore_masks"], t["category_ids"])
        out.append({"masks": m, "ignore_masks": ig, "semseg_masks": sem, "category_ids": t["category_ids"]})
    return out


def load_fixtures(path):
    """tests/golden/semseg_loss.npz -> {name: dict(K, has_fg, weight, x, targets (raw), prepared (the reference's), losses
    [others semseg, optimization semseg, foreground], grad (of optimization semseg + foreground))}."""
    z = np.load(path)
    out = {}
    for name in [str(c) for c in z["cases"]]:
        x = torch.from_numpy(z[name + "/x"])
        targets, prep = [], []
        for n in range(x.shape[0]):
            shp = tuple(int(v) for v in z["%s/masks%d_shape" % (name, n)])
            I, T, H, W = shp
            h, w = H // 4, W // 4
            bits = lambda key, s: np.unpackbits(z["%s/%s%d" % (name, key, n)])[:int(np.prod(s))].reshape(s)
            cats = torch.from_numpy(z["%s/category_ids%d" % (name, n)])
            targets.append({"masks": torch.from_numpy(bits("masks", shp)), "ignore_masks": torch.from_numpy(bits("ignore", (T, H, W)).astype(bool)),
                            "category_ids": cats})
            prep.append({"masks": torch.from_numpy(bits("small_masks", (I, T, h, w))), "ignore_masks": torch.from_numpy(bits("small_ignore", (T, h, w))),
                         "semseg_masks": torch.from_numpy(z["%s/semseg%d" % (name, n)].astype(np.int64)), "category_ids": cats})
        out[name] = dict(K=int(z[name + "/n_classes"]), has_fg=bool(z[name + "/has_fg"]), weight=float(z[name + "/weight_semseg"]), x=x,
                         targets=targets, prepared=prep, losses=z[name + "/losses"], grad=z[name + "/grad"])
    return out
