"""Torch restatement of the reference's embedding loss (modeling/losses/embedding_loss.py:35-185 on the Lovasz hinge,
_lovasz.py:51-63,130-147), in fp32 or fp64, differentiable by autograd, with the device's tie order: a STABLE sort, descending error,
ascending voxel index.  Runs on the CPU (the yardstick of the tests) and, for timing only, on the GPU with stock torch ops
(tools/loss_bench.py).  Also the deterministic inputs of the fixtures (tools/make_loss_goldens.py) and of the GPU tests."""
import numpy as np
import torch


def lovasz_hinge(logits, labels):
    """logits [P], labels [P] (0 / 1, same dtype as logits)."""
    err = 1. - logits * (2. * labels - 1.)
    err_sorted, perm = torch.sort(err, descending=True, stable=True)
    gt = labels[perm]
    total = gt.sum()
    jaccard = 1. - (total - gt.cumsum(0)) / (total + (1. - gt).cumsum(0))
    grad = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
    return torch.dot(torch.relu(err_sorted), grad)


def embedding_loss(embedding_map, targets, embedding_size, free_dim_stds=(), dtype=torch.float32):
    """embedding_map [N, C, T, H, W]; targets: list of dicts with 'masks' [I, T, H, W] and 'ignore_masks' [T, H, W].
    -> (lovasz, smoothness, seediness) scalars of ``dtype``, divided as the reference divides them."""
    E, nf = embedding_size, len(free_dim_stds)
    B = E - nf
    x = embedding_map.to(dtype)
    N = x.shape[0]
    dev = x.device
    free_bw = 1. / torch.tensor(list(free_dim_stds), dtype=dtype, device=dev) ** 2
    zero = (x.sum() * 0)
    lovasz, smooth, seedl, total = zero, zero, zero, 0
    for n in range(N):
        masks = targets[n]["masks"].to(dev)
        if masks.numel() == 0:
            continue
        ignore = targets[n]["ignore_masks"].to(dev).bool().reshape(-1)
        m = (masks.reshape(masks.shape[0], -1) != 0)
        counts = m.sum(1)
        present = [i for i in range(m.shape[0]) if int(counts[i]) > 0]
        if not present:
            continue
        emb = x[n, :E].reshape(E, -1).t()                      # [P, E]
        bw = x[n, E:E + B].reshape(B, -1).t()                  # [P, B] raw
        seed = x[n, E + B].reshape(-1)                         # [P]
        total += len(present)
        bg = ~m.any(0)
        bg_term = seed[bg] ** 2
        seedl = seedl + torch.where(ignore[bg], torch.zeros_like(bg_term), bg_term).mean()
        s = zero
        for i in present:
            b_i = bw[m[i]]
            s = s + ((b_i.mean(0, keepdim=True) - b_i) ** 2).mean()
        smooth = smooth + s / float(len(present))
        for k, i in enumerate(present):                        # centre of the k-th present instance, target masks[k]
            centre = emb[m[i]].mean(0, keepdim=True)
            beta = (bw[m[i]].exp() * 10.).mean(0, keepdim=True)
            if nf:
                beta = torch.cat((beta, free_bw[None]), 1)
            p = torch.exp(-0.5 * (((emb - centre) ** 2) * beta).sum(-1))
            if int(counts[k]) == 0:
                continue
            lovasz = lovasz + lovasz_hinge(p * 2. - 1., m[k].to(dtype))
            seedl = seedl + ((seed[m[i]] - p[m[i]].detach()) ** 2).mean()
    if total == 0:
        return zero, zero, zero
    return lovasz / total, smooth / N, seedl / float(total + 1)


# ------------------------------------------------------------------------------------------------ deterministic inputs
def _blob(rng, T, H, W, frac=0.3):
    """A box-shaped instance covering about ``frac`` of each axis."""
    m = np.zeros((T, H, W), np.uint8)
    h, w = max(2, int(H * frac)), max(2, int(W * frac))
    y0, x0 = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
    t0 = rng.integers(0, max(1, T // 2))
    m[t0:, y0:y0 + h, x0:x0 + w] = 1
    return m


def make_sample(rng, E, nf, T, H, W, n_inst, empty=(), overlap=False, noise=0.04, frac=None):
    """-> (x float32 [C, T, H, W], masks uint8 [I, T, H, W], ignore bool [T, H, W]): grid-like embeddings + noise (an instance is
    compact in them), per-instance constants in the free dims, raw bandwidths around 0.2, seediness in (0, 1)."""
    B = E - nf
    masks = np.zeros((n_inst, T, H, W), np.uint8)
    for i in range(n_inst):
        if i not in empty:
            masks[i] = _blob(rng, T, H, W, 0.25 + 0.2 * rng.random() if frac is None else frac)
    if not overlap:                                            # first instance wins
        seen = np.zeros((T, H, W), bool)
        for i in range(n_inst):
            masks[i][seen] = 0
            seen |= masks[i] > 0
    grid = np.meshgrid(np.linspace(-0.2, 0.2, T), np.linspace(-0.56, 0.56, H), np.linspace(-1, 1, W), indexing="ij")
    order = [2, 1, 0]                                          # x, y, t
    x = np.zeros((E + B + 1, T, H, W), np.float32)
    for e in range(E):
        if e < min(B, 3):
            x[e] = grid[order[e]] + noise * rng.standard_normal((T, H, W))
        else:
            x[e] = 0.1 * rng.standard_normal((T, H, W))
            for i in range(n_inst):
                x[e][masks[i] > 0] += rng.uniform(-1, 1)
    x[E:E + B] = 0.2 + 0.3 * rng.standard_normal((B, T, H, W))
    fg = masks.any(0) if n_inst else np.zeros((T, H, W), bool)
    x[E + B] = np.clip(np.where(fg, 0.6, 0.15) + 0.2 * rng.standard_normal((T, H, W)), 0.01, 0.99)
    ignore = np.zeros((T, H, W), bool)
    ignore[:, :max(1, H // 6), :] = rng.random((T, max(1, H // 6), W)) < 0.7
    return x.astype(np.float32), masks, ignore


# name -> (embedding_size, free_dim_stds, [per-sample (T, H, W, n_inst, empty, overlap) | "none" (masks.numel() == 0)])
FIXTURE_CASES = {
    "xyt": (3, (), [(4, 24, 40, 3, (), False)]),
    "xyff_free_dims": (4, (0.3, 0.4), [(3, 12, 16, 3, (), False)]),
    "xytf_n2": (4, (0.5,), [(2, 12, 20, 2, (), False), (2, 12, 20, 3, (), True)]),
    "n2_overlap": (3, (), [(3, 12, 16, 3, (), True), (3, 12, 16, 2, (), True)]),
    "empty_middle": (3, (), [(3, 12, 16, 5, (1, 3), True)]),
    "empty_first_two": (3, (), [(2, 12, 16, 3, (0, 1), False)]),
    "sample_without_instances": (3, (), ["none", (2, 12, 16, 2, (), False), (2, 12, 16, 2, (0, 1), False)]),
    "all_empty_batch": (3, (), ["none", (2, 12, 16, 2, (0, 1), False)]),
}


def make_case(name, cases=None, seed=None):
    """-> (x float32 [N, C, T, H, W], targets) for a case of FIXTURE_CASES (or of ``cases``)."""
    E, stds, samples = (cases or FIXTURE_CASES)[name]
    rng = np.random.default_rng(sum(map(ord, name)) if seed is None else seed)
    dims = next(s for s in samples if s != "none")[:3]
    xs, targets = [], []
    for s in samples:
        if s == "none":
            T, H, W = dims
            x, _, ig = make_sample(rng, E, len(stds), T, H, W, 1)
            masks = np.zeros((0, T, H, W), np.uint8)
        else:
            x, masks, ig = make_sample(rng, E, len(stds), *s)
        xs.append(x)
        targets.append({"masks": torch.from_numpy(masks), "ignore_masks": torch.from_numpy(ig)})
    return torch.from_numpy(np.stack(xs)), targets


# the training shape (T = 8 on 120 x 216 maps) at two instance counts, N = 2, and free dims at a mid size
LARGE_CASES = {
    "train_i6": (3, (), [(8, 120, 216, 6, (), True)]),
    "train_i20": (3, (), [(8, 120, 216, 20, (), True)]),
    "n2_mid": (3, (), [(8, 60, 108, 5, (2,), True), (8, 60, 108, 3, (), False)]),
    "free_dims_mid": (4, (0.3, 0.4), [(8, 60, 108, 6, (), True)]),
    # three and four sort tiles of 4096 voxels, small enough for few near-ties of the sort: N = 2 with the index shift, and free dims
    "tiles3_n2": (3, (), [(4, 48, 64, 4, (1,), True, 0.04, 0.12), (4, 48, 64, 3, (), False, 0.04, 0.12)]),
    "tiles4_free_dims": (4, (0.3, 0.4), [(8, 32, 64, 5, (), True, 0.04, 0.12)]),
}


def losses_and_grads(x, targets, E, stds, dtype, device="cpu"):
    """-> (losses float64 numpy [3], grads: three numpy arrays [N, C, T, H, W], one per component) of the oracle in ``dtype``."""
    xx = x.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)      # (a copy: the caller's tensor stays a plain input)
    comps = embedding_loss(xx, targets, E, stds, dtype)
    grads = []
    for c in comps:
        g, = torch.autograd.grad(c, xx, retain_graph=True, allow_unused=True)
        grads.append(np.zeros(tuple(x.shape)) if g is None else g.detach().double().cpu().numpy())
    return np.array([float(c.detach()) for c in comps]), grads


DEFAULT_WEIGHTS = dict(WEIGHT_REGULARIZATION=0.001, WEIGHT_LOVASZ=1.0, WEIGHT_VARIANCE_SMOOTHNESS=10.0, WEIGHT_SEEDINESS=1.0, WEIGHT=1.0)


def load_fixtures(path):
    """tests/golden/embedding_loss.npz -> {name: dict(x, targets, losses [total, lovasz, smoothness, seediness], grad, E, stds)}."""
    z = np.load(path)
    out = {}
    for name in [str(c) for c in z["cases"]]:
        x = torch.from_numpy(z[name + "/x"])
        T, H, W = x.shape[2:]
        targets = []
        for n in range(x.shape[0]):
            shp = tuple(int(v) for v in z["%s/masks%d_shape" % (name, n)])
            m = np.unpackbits(z["%s/masks%d" % (name, n)])[:int(np.prod(shp))].reshape(shp)
            ig = np.unpackbits(z["%s/ignore%d" % (name, n)])[:T * H * W].reshape(T, H, W).astype(bool)
            targets.append({"masks": torch.from_numpy(m.astype(np.uint8)), "ignore_masks": torch.from_numpy(ig)})
        out[name] = dict(x=x, targets=targets, losses=z[name + "/losses"], grad=z[name + "/grad"], E=int(z[name + "/embedding_size"]),
                         stds=tuple(float(v) for v in z[name + "/free_dim_stds"]))
    return out


def total_of(losses, grads, w=DEFAULT_WEIGHTS):
    """Weighted total of the three components (values or gradients), as EmbeddingLoss combines them."""
    ws = (w["WEIGHT_LOVASZ"], w["WEIGHT_VARIANCE_SMOOTHNESS"], w["WEIGHT_SEEDINESS"])
    return sum(l * k for l, k in zip(losses, ws)) * w["WEIGHT"], sum(g * k for g, k in zip(grads, ws)) * w["WEIGHT"]
