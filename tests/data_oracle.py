"""Test-side restatement of the training data path on the CPU: COCO RLE strings -> planes -> bilinear resize -> > 0.5 -> zero pad
(the reference's generic_video_dataset_parser.py:74-94, structures/mask.py:32-40, data/common.py:58-74), built on torch CPU and on
``tests/writer_oracle.py``'s ``string_to_counts`` / ``decode``.  Also the cases the GPU test and the host test share, so that the host test
can check the cases' validity without a device."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import writer_oracle as wo

EMPTY, BAD_CHAR, OPEN_GROUP, BAD_COUNT, BAD_SUM = 1, 2, 4, 8, 16
MAX_GROUPS = 12


# ------------------------------------------------------------------------------------------------ RLE strings
def deltas_to_string(deltas):
    """rleToString's character stage alone: every value goes out as written (no i - 2 subtraction), so a test can write any delta."""
    out = []
    for x in deltas:
        x, more = int(x), True
        while more:
            g = x & 0x1f
            x >>= 5
            more = (x != -1) if (g & 0x10) else (x != 0)
            out.append(chr((g | 0x20 if more else g) + 48))
    return "".join(out)


def string_status(s, h, w):
    """The first check of include/stemseg_hip.h's list that the string fails, or 0."""
    if isinstance(s, bytes):
        s = s.decode("latin-1")
    if len(s) == 0:
        return EMPTY
    codes = [ord(ch) for ch in s]
    if any(c < 48 or c > 111 for c in codes):
        return BAD_CHAR
    if (codes[-1] - 48) & 0x20:
        return OPEN_GROUP
    groups, n = [], 0
    for c in codes:
        n += 1
        if not (c - 48) & 0x20:
            groups.append(n)
            n = 0
    if max(groups) > MAX_GROUPS:
        return BAD_COUNT
    counts = wo.string_to_counts(s)
    deltas = [c - (counts[i - 2] if i > 2 else 0) for i, c in enumerate(counts)]
    if any(abs(d) > 2 ** 31 for d in deltas) or any(c < 0 or c > h * w for c in counts):
        return BAD_COUNT
    if sum(counts) != h * w:
        return BAD_SUM
    return 0


def decode_strings(strings, plane_of_string, P, h, w):
    """-> (planes uint8 [P, h, w], status uint8 [M]): what ``hip.rle_decode`` documents."""
    planes = np.zeros((P, h, w), np.uint8)
    status = np.zeros(len(strings), np.uint8)
    for m, (s, q) in enumerate(zip(strings, plane_of_string)):
        status[m] = string_status(s, h, w)
        if status[m] == 0:
            planes[q] = wo.decode(wo.string_to_counts(s if isinstance(s, str) else s.decode("ascii")), h, w)
    return planes, status


def mask_string(mask):
    """The COCO RLE string of a mask (non-zero is 1): ``wo.counts_to_string(wo.encode(mask))`` with the run lengths taken by numpy, since
    the benches under tools/ encode full frames and a per-pixel loop takes a second on one (tests/test_rle_checks_host.py compares)."""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)          # column-major: p = x * H + y
    bounds = np.concatenate(([0], np.flatnonzero(flat[1:] != flat[:-1]) + 1, [flat.size]))
    return wo.counts_to_string(([0] if flat[0] else []) + np.diff(bounds).tolist())


# ------------------------------------------------------------------------------------------------ resize + pad
def union_complement(planes, ranges):
    """[R, H, W] uint8: 1 - any(planes[start + k * stride], k < count) per (start, count, stride)."""
    planes = np.asarray(planes)
    return np.stack([1 - planes[[s + k * st for k in range(c)]].any(0).astype(np.uint8) for s, c, st in ranges], 0) if len(ranges) else \
        np.zeros((0,) + planes.shape[1:], np.uint8)


@torch.no_grad()
def resize_soft(planes, new_hw):
    """float32 [P, new_h, new_w]: the bilinear values before the threshold."""
    return F.interpolate(torch.as_tensor(np.asarray(planes)).float()[None], tuple(int(v) for v in new_hw), mode="bilinear", align_corners=False)[0]


def resize_masks(planes, new_hw, pad_hw, ignore_from=None):
    """-> (hard uint8 [P + R, pad_h, pad_w], soft float32 [P + R, new_h, new_w]) as numpy: what ``hip.resize_masks`` documents."""
    planes = np.asarray(planes, np.uint8)
    every = np.concatenate([planes, union_complement(planes, ignore_from or [])], 0)
    soft = resize_soft(every, new_hw)
    hard = torch.zeros((every.shape[0], int(pad_hw[0]), int(pad_hw[1])), dtype=torch.uint8)
    hard[:, :new_hw[0], :new_hw[1]] = (soft > 0.5).to(torch.uint8)
    return hard.numpy(), soft.numpy()


def near_tie_share(soft, band=1e-6):
    """Share of the pixels whose soft value lies within ``band`` of 0.5 without being exactly 0.5."""
    d = np.abs(np.asarray(soft, np.float64) - 0.5)
    return float(((d <= band) & (d != 0)).mean())


def check_tie_rule(got, hard, soft, new_hw, what=""):
    """The rule tests/test_gpu_parity.py holds the DAVIS mask materialisation to: a pixel may differ from the oracle only where the
    oracle's soft value lies within 1e-6 of 0.5, fewer than 1e-3 of the pixels may, and the padding is exactly zero.  -> mismatches."""
    got, hard = np.asarray(got), np.asarray(hard)
    assert got.shape == hard.shape, (what, got.shape, hard.shape)
    nh, nw = new_hw
    assert not got[:, nh:, :].any() and not got[:, :, nw:].any(), "%s: the padding is not zero" % what
    assert set(np.unique(got).tolist()) <= {0, 1}, what
    diff = got[:, :nh, :nw] != hard[:, :nh, :nw]
    n = int(diff.sum())
    if n:
        assert (np.abs(soft[diff].astype(np.float64) - 0.5) <= 1e-6).all(), "%s: %d pixels differ away from the 0.5 band" % (what, n)
        assert n < 1e-3 * diff.size, "%s: %d of %d pixels differ" % (what, n, diff.size)
    return n


# ------------------------------------------------------------------------------------------------ a batch from recipes, on the host
def resize_params(height, width, min_dim, max_dim):
    """-> (new_h, new_w): data/common.py:162-173."""
    scale = min_dim / float(min(height, width))
    if max(height, width) * scale > max_dim:
        scale = max_dim / float(max(height, width))
    return round(scale * height), round(scale * width)


def decode_image(data):
    """File bytes -> BGR uint8 [H, W, 3], as cv2.imread gives it (PIL rides on the same libjpeg-turbo / libpng)."""
    import io
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


@torch.no_grad()
def collate(recipes, min_dim, max_dim, mean, std, unit_scale=False, bgr=True, with_images=True):
    """The reference's ``VideoDataset.__getitem__`` + ``collate_fn`` from host recipes (stemseg_amd/data/common.py), on the CPU: ->
    {"images" float32 [N,T,3,ph,pw] | None, "image_sizes", "pad", "targets": [{"masks", "ignore_masks" (uint8), "category_ids",
    "soft_masks", "soft_ignore" (float32, unpadded)}]}."""
    new_sizes = [resize_params(r["size"][1], r["size"][0], min_dim, max_dim) for r in recipes]
    ph, pw = [int(np.ceil(max(s[d] for s in new_sizes) / 32.0)) * 32 for d in (0, 1)]
    T = len(recipes[0]["frames"])
    images = torch.zeros((len(recipes), T, 3, ph, pw)) if with_images else None
    targets = []
    for n, (r, (nh, nw)) in enumerate(zip(recipes, new_sizes)):
        w, h = r["size"]
        if with_images:
            x = torch.from_numpy(np.stack([decode_image(f) for f in r["frames"]])).permute(0, 3, 1, 2).float()
            x = F.interpolate(x, (nh, nw), mode="bilinear", align_corners=False)
            if unit_scale:
                x = x / 255.0
            x = (x - torch.tensor(mean, dtype=torch.float32)[None, :, None, None]) / torch.tensor(std, dtype=torch.float32)[None, :, None, None]
            images[n, :, :, :nh, :nw] = x if bgr else x.flip(dims=[1])
        planes = np.zeros((r["n_instances"], T, h, w), np.uint8)
        for inst, t, s in r["rle"]:
            assert string_status(s, h, w) == 0, (r["meta_info"], inst, t)
            planes[inst, t] = wo.decode(wo.string_to_counts(s), h, w)
        ignore = r["ignore"]
        keep = [i for i in range(r["n_instances"]) if not (isinstance(ignore, tuple) and i == ignore[1])]
        if ignore == "background":
            ign = 1 - planes.any(0).astype(np.uint8)
        elif isinstance(ignore, tuple):
            ign = planes[ignore[1]]
        else:
            ign = np.zeros((T, h, w), np.uint8)
        hard_m, soft_m = resize_masks(planes[keep].reshape(-1, h, w), (nh, nw), (ph, pw))
        hard_i, soft_i = resize_masks(ign, (nh, nw), (ph, pw))
        targets.append({"masks": hard_m.reshape(len(keep), T, ph, pw), "ignore_masks": hard_i, "category_ids": list(r["category_ids"]),
                        "soft_masks": soft_m.reshape(len(keep), T, nh, nw), "soft_ignore": soft_i})
    return {"images": None if images is None else images.numpy(), "image_sizes": new_sizes, "pad": (ph, pw), "targets": targets}


# ------------------------------------------------------------------------------------------------ the golden's synthetic dataset
class Golden(object):
    """tests/golden/data_pipeline.npz (tools/make_data_goldens.py): the synthetic dataset and what the reference made of it."""

    def __init__(self, npz):
        import json
        self.npz = npz
        self.record = json.loads(str(npz["record_json"]))
        self.config = json.loads(str(npz["config"]))
        self.dataset_json = str(npz["dataset_json"])
        ends = np.cumsum(npz["file_sizes"])
        blob = npz["file_bytes"].tobytes()
        self.files = {str(name): blob[e - s:e] for name, s, e in zip(npz["file_names"], npz["file_sizes"], ends)}

    def write(self, directory, json_name="dataset.json"):
        """The image files and the dataset JSON below ``directory`` -> the JSON's path."""
        import os
        for name, data in self.files.items():
            os.makedirs(os.path.dirname(os.path.join(directory, name)), exist_ok=True)
            with open(os.path.join(directory, name), "wb") as fh:
                fh.write(data)
        path = os.path.join(directory, json_name)
        with open(path, "w") as fh:
            fh.write(self.dataset_json)
        return path

    def configure(self, cfg):
        """The tool's settings on ``stemseg_amd.config.cfg`` (the caller restores the preset)."""
        cfg.INPUT.NUM_FRAMES, cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM = (self.config[k] for k in ("NUM_FRAMES", "MIN_DIM", "MAX_DIM"))
        for section, (lo, hi) in self.config["GAPS"].items():
            getattr(cfg.DATA, section).FRAME_GAP_LOWER, getattr(cfg.DATA, section).FRAME_GAP_UPPER = lo, hi


def pick_clip(sequences, seq_id, paths):
    """The sub-sequence of the frames ``paths`` of the sequence ``seq_id`` (or of its part '<seq_id>_k' that holds them)."""
    for seq in sequences:
        if (seq.id == seq_id or str(seq.id).startswith(seq_id + "_")) and all(p in seq.image_paths for p in paths):
            return seq.extract_subsequence([seq.image_paths.index(p) for p in paths])
    raise KeyError(seq_id)


CLIP_A = ["a/%05d.jpg" % t for t in (0, 2, 4, 6)]
CLIP_B = ["b/%05d.png" % t for t in (1, 3, 5, 8)]


def make_loader(name, base_dir, vds, n_samples=7):
    from stemseg_amd.data import DavisDataLoader, MOTSDataLoader, YoutubeVISDataLoader
    if name == "ytvis":
        return YoutubeVISDataLoader(base_dir, vds, n_samples, category_agnostic=False)
    if name == "davis":
        return DavisDataLoader(base_dir, vds, samples_to_create=n_samples)
    return MOTSDataLoader(base_dir, vds, n_samples)


def describe(seqs):
    return [{"id": s.id, "image_paths": s.image_paths, "instance_ids": s.instance_ids, "category_labels": s.category_labels} for s in seqs]


# ------------------------------------------------------------------------------------------------ shared cases
def mask_with_runs(h, w, n_runs, start_one=False, seed=0):
    """A [h, w] mask whose RLE has exactly n_runs counts (the first may be the empty zero run when start_one)."""
    rs = np.random.RandomState(seed + 31 * n_runs + h * w)
    n_real = n_runs - 1 if start_one else n_runs
    assert 1 <= n_real <= h * w
    cuts = np.sort(rs.choice(np.arange(1, h * w), n_real - 1, replace=False)) if n_real > 1 else np.zeros(0, int)
    lens = np.diff(np.concatenate([[0], cuts, [h * w]])).tolist()
    counts = ([0] if start_one else []) + lens
    assert len(counts) == n_runs and sum(counts) == h * w
    return wo.decode(counts, h, w).astype(np.uint8)


def blobs(h, w, n, seed):
    rs = np.random.RandomState(seed)
    m = np.zeros((h, w), np.uint8)
    for _ in range(n):
        y, x = rs.randint(0, h), rs.randint(0, w)
        ry, rx = rs.randint(1, max(2, h // 3)), rs.randint(1, max(2, w // 3))
        yy, xx = np.ogrid[:h, :w]
        m |= (((yy - y) / float(ry)) ** 2 + ((xx - x) / float(rx)) ** 2 <= 1.0).astype(np.uint8)
    return m


def rle_small_cases():
    """[(name, h, w, [masks])]: the run-count boundary, all-zero / all-one, a plane starting with a 1."""
    cases = []
    for h, w in ((7, 5), (1, 1), (1, 40), (40, 1)):
        masks = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)]
        for n_runs in (1, 2, 3, 4, 5):
            for start_one in (False, True):
                if 1 <= (n_runs - 1 if start_one else n_runs) <= h * w:
                    masks.append(mask_with_runs(h, w, n_runs, start_one))
        cases.append(("%dx%d" % (h, w), h, w, masks))
    return cases


def rle_count_width_cases():
    """[(h, w, counts)]: counts that take 1, 2, 3 and 4 characters, and deltas of both signs around the group boundaries."""
    return [(4, 5, [3, 15, 2]),                                   # one character each
            (20, 30, [100, 400, 100]),                            # two characters
            (100, 200, [2000, 16000, 2000]),                      # three characters
            (600, 700, [420000]),                                 # one run of four characters
            (600, 700, [1, 419999]),
            (30, 40, [5, 20, 2, 3, 18, 36, 1, 4, 600, 16, 17, 31, 1, 433, 13]),      # deltas -17, +16, +16, -17, +1, +598, -20, ... and 16 / 17 / 31 (an extra group for bit 0x10)
            (30, 40, [0, 1, 1, 2, 3, 1, 592, 600])]                                   # first count 0; deltas +1, +2, -1, +589, +599


def checkerboard():
    h, w = 64, 48
    return ((np.arange(h * w) & 1).reshape(w, h).T).astype(np.uint8)          # p = x * h + y odd -> 1: 3072 counts of 1


def unequal_batch():
    """(strings, plane_of_string, P, h, w): 300 strings of very unequal length, scattered over 320 planes."""
    h, w, M, P = 20, 16, 300, 320
    rs = np.random.RandomState(5)
    masks = []
    for m in range(M):
        kind = m % 5
        if kind == 0:
            masks.append(np.zeros((h, w), np.uint8))
        elif kind == 1:
            masks.append((rs.rand(h, w) < 0.5).astype(np.uint8))            # ~ 160 counts
        elif kind == 2:
            masks.append(blobs(h, w, 2, 100 + m))
        elif kind == 3:
            masks.append(((np.arange(h * w) & 1).reshape(w, h).T).astype(np.uint8))      # 320 counts
        else:
            masks.append(np.ones((h, w), np.uint8))
    planes = rs.permutation(P)[:M].tolist()
    return [mask_string(m) for m in masks], planes, P, h, w


def strided_planes_case():
    """(strings, plane_of_string, label_of_string, P, h, w) for the raster kernels' plane loop: 1025 planes, one more than the grid has
    rows, so the workgroups of plane 0 come back for plane 1024; 24 x 25 = 600 pixels are three workgroups, the last one ragged.  Only
    planes 0, 1, 1023 and 1024 are named, each by two or three overlapping rectangles; the overlap of plane 0 is not that of plane 1024."""
    P, h, w = 1025, 24, 25
    boxes = [(0, 5, (2, 14, 3, 15)), (0, 9, (8, 20, 10, 22)), (0, 2, (0, 10, 12, 25)),
             (1, 40000, (0, 24, 0, 5)), (1, 3, (5, 9, 2, 20)),
             (1023, 7, (3, 21, 4, 20)), (1023, 65535, (10, 24, 0, 8)),
             (1024, 1, (1, 9, 1, 9)), (1024, 300, (5, 13, 5, 13)), (1024, 8, (7, 24, 7, 25))]
    strings = []
    for _, _, (y0, y1, x0, x1) in boxes:
        m = np.zeros((h, w), np.uint8)
        m[y0:y1, x0:x1] = 1
        strings.append(mask_string(m))
    return strings, [b[0] for b in boxes], [b[1] for b in boxes], P, h, w


def malformed_cases(h=7, w=5):
    """[(name, string, expected status)] for a h x w plane."""
    good = mask_string(mask_with_runs(h, w, 4))
    return [("bad_char_high", good[:1] + chr(112) + good[1:], BAD_CHAR),
            ("bad_char_low", good[:1] + " " + good[1:], BAD_CHAR),
            ("open_group", good + chr(48 + 0x20 + 3), OPEN_GROUP),
            ("negative_count", deltas_to_string([3, 2, 4, -5, h * w - 6]), BAD_COUNT),       # count 3 = 2 - 5
            ("negative_first", deltas_to_string([-1, h * w + 1]), BAD_COUNT),
            ("count_above_plane", deltas_to_string([h * w + 1]), BAD_COUNT),
            ("overlong_count", chr(48 + 0x20) * 12 + chr(48), BAD_COUNT),                    # 13 characters for one zero
            ("huge_delta", deltas_to_string([2 ** 40]), BAD_COUNT),
            ("short_sum", deltas_to_string([3, 2]), BAD_SUM),
            ("long_sum", deltas_to_string([h * w, 1]), BAD_SUM),
            ("empty", "", EMPTY)]


RESIZE_SHAPES = [((37, 53), (48, 69), [(64, 96), (96, 128)]),
                 ((96, 128), (48, 64), [(64, 64), (64, 96)]),
                 ((45, 40), (80, 71), [(96, 96), (128, 96)]),
                 ((375, 1242), (193, 640), [(224, 640), (256, 672)])]


def resize_planes(h, w, seed=0):
    """uint8 [6, h, w]: random blobs, single pixels (corners and interior), full rows and columns at the borders, noise."""
    rs = np.random.RandomState(seed + h)
    single = np.zeros((h, w), np.uint8)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2), (h // 3, w // 4)):
        single[y, x] = 1
    rows = np.zeros((h, w), np.uint8)
    rows[0, :] = rows[h - 1, :] = 1
    cols = np.zeros((h, w), np.uint8)
    cols[:, 0] = cols[:, w - 1] = 1
    return np.stack([blobs(h, w, 4, seed + 1), blobs(h, w, 9, seed + 2), single, rows, cols, (rs.rand(h, w) < 0.3).astype(np.uint8)], 0)
