"""Test-side restatement of the Mapillary path on the CPU (the reference's data/mapillary_data_loader.py): the union decode as the OR of
``data_oracle.decode_strings`` per string, the selection rule of ``filter_instance_masks`` on lists of (area, category), a synthetic
``mapillary.json`` over the golden's 37 x 53 JPEG and 45 x 40 PNG, and the cases the GPU test and the host test share, so that the host
test can check the cases' validity without a device."""
import json
import os

import numpy as np

from tests import augment_oracle as ao
from tests import data_oracle as do

KEEP, IGNORE = (1, 2), (3, 4)          # tests/golden/metainfo/mapillary.yaml; 5 is neither
UNION_SHAPES = ((7, 5), (37, 53), (1, 64), (64, 1), (200, 300))


# ------------------------------------------------------------------------------------------------ the union decode
def decode_union(strings, plane_of_string, P, h, w):
    """-> (planes uint8 [P, h, w], status uint8 [M]): plane p = OR of the accepted strings that name p; refused strings are left out."""
    planes = np.zeros((P, h, w), np.uint8)
    status = np.zeros(len(strings), np.uint8)
    for m, (s, q) in enumerate(zip(strings, plane_of_string)):
        one, st = do.decode_strings([s], [0], 1, h, w)
        status[m] = st[0]
        if st[0] == 0:
            planes[q] |= one[0]
    return planes, status


# ------------------------------------------------------------------------------------------------ the selection rule
def select(areas, categories, max_nbr_instances, ignore_ids=IGNORE):
    """filter_instance_masks on positions: -> (targets, ignored) as lists of positions, the targets in the reference's order (descending
    area, ties in their original order, which is what Python's stable ``sorted(..., reverse=True)`` gives), the ignored as a set."""
    order = [i for i, _ in sorted([(i, a) for i, a in enumerate(areas)], key=lambda x: x[1], reverse=True)]
    targets, ignored = [], []
    for k, i in enumerate(order):
        if k < max_nbr_instances and categories[i] not in ignore_ids:
            targets.append(i)
        else:
            ignored.append(i)
    return targets, set(ignored)


# ------------------------------------------------------------------------------------------------ a synthetic dataset
def disc(h, w, cy, cx, r):
    y, x = np.mgrid[0:h, 0:w]
    return ((y - cy) ** 2 + (x - cx) ** 2 <= r * r).astype(np.uint8)


def dataset_entries():
    """[(image path, masks [N, h, w], categories)]:
    0  a/00000.jpg  40 overlapping discs with categories cycling through 1 .. 5 (35 remain without category 5: more than 30), and one
                    instance of 15 pixels, below the area filter
    1  b/00001.png  six discs, the LARGEST of an ignore category (so max_nbr_instances=1 leaves no target), two overlapping ignore discs
    2  a/00000.jpg  ignore and other categories alone: dropped
    3  b/00001.png  its one kept instance has 15 pixels: dropped"""
    rs = np.random.RandomState(7)
    h, w = 37, 53
    cycle = [1, 3, 2, 4, 1, 5, 2, 3]
    many = [disc(h, w, rs.uniform(5, h - 5), rs.uniform(5, w - 5), rs.uniform(3.5, 8.0)) for _ in range(40)]
    tiny = np.zeros((h, w), np.uint8)
    tiny[1:4, 1:6] = 1
    first = ("a/00000.jpg", np.stack(many + [tiny]), [cycle[i % 8] for i in range(40)] + [1])
    h, w = 45, 40
    six = [disc(h, w, 22, 18, 14), disc(h, w, 10, 10, 6), disc(h, w, 30, 28, 7), disc(h, w, 28, 12, 8), disc(h, w, 12, 30, 5), disc(h, w, 40, 5, 4)]
    second = ("b/00001.png", np.stack(six), [3, 1, 2, 1, 4, 5])          # by area: 3, 1 (r = 8), 2, 1, 4; the last disc is dropped
    third = ("a/00000.jpg", np.stack(many[:3]), [3, 5, 4])
    tiny = np.zeros((h, w), np.uint8)
    tiny[1:4, 1:6] = 1
    fourth = ("b/00001.png", np.stack([six[0], tiny]), [3, 2])
    return [first, second, third, fourth]


def write_dataset(base):
    """mapillary.json below ``base`` (where ``data_oracle.Golden.write`` has put the frames).  -> its path."""
    path = os.path.join(base, "mapillary.json")
    with open(path, "w") as fh:
        json.dump(ao.image_dataset_json([(p, m, c, None) for p, m, c in dataset_entries()]), fh)
    return path


def expected_sample(entry, min_instance_size, max_nbr_instances):
    """What the loader keeps of an entry, by the reference's steps on decoded masks: None when the sample is dropped, else
    (kept positions into the entry, targets, ignored) -- the latter two positions into the kept list."""
    _, masks, cats = entry
    kept = [i for i in range(len(cats)) if int(masks[i].sum()) >= min_instance_size]
    if not any(cats[i] in KEEP for i in kept):
        return None
    kept = [i for i in kept if cats[i] in KEEP + IGNORE]
    targets, ignored = select([int(masks[i].sum()) for i in kept], [cats[i] for i in kept], max_nbr_instances)
    return kept, targets, ignored


# ------------------------------------------------------------------------------------------------ a batch entry from a recipe, on the host
def recipe_planes(recipe):
    """uint8 [P, h, w] (un-mirrored): the targets and, last, the union of the ignore strings."""
    w, h = recipe["size"]
    P = recipe["n_instances"] + int(recipe["has_ignore"])
    planes, status = decode_union(recipe["rle"], recipe["rle_planes"], P, h, w)
    assert not status.any()
    return planes


def recipe_warp(recipe):
    """``augment_oracle.image_recipe_warp`` for a recipe with ``rle_planes``: -> (mirrored source, its planes, the oracle's warp, blurs)."""
    src, pl = do.decode_image(recipe["frames"][0]), recipe_planes(recipe)
    if recipe["flip"]:
        src, pl = np.ascontiguousarray(src[:, ::-1]), np.ascontiguousarray(pl[:, :, ::-1])
    hinvs, jit, blurs = [], [], []
    for k in recipe["perm"]:
        wp = recipe["warps"][k - 1] if k else None
        hinvs.append(np.asarray(wp["hinv"]) if k else ao.identity())
        jit.append((wp["add"], wp["hs"], wp["flags"]) if k else (0, 0, 0))
        blurs.append(None if not k or wp["blur"] is None else np.asarray(wp["blur"], np.float32))
    return src, pl, ao.warp_clip(src, pl, np.stack(hinvs), jit), blurs


# (dataset index, max_nbr_instances, seed for ``random``): the end-to-end cases of tests/test_gpu_mapillary.py; tests/test_mapillary_host.py
# asserts on the oracle alone that each stays inside the caps of the band rule and the tie rule
END_TO_END = {"many": (0, 30, 0), "few": (1, 30, 1), "max2": (1, 2, 2), "no_target": (1, 1, 3)}


# ------------------------------------------------------------------------------------------------ cases of rle_decode_union
def mask_counts(mask):
    """The run lengths of a [h, w] mask in column-major order, the first a run of zeros (``writer_oracle.encode``, vectorised: the
    200 x 300 cases hold 400 masks)."""
    flat = np.asarray(mask, bool).T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    return ([0] if flat[0] else []) + np.diff(np.concatenate([[0], change, [flat.size]])).tolist()


def zero_run_string(mask):
    """The mask's RLE with zero-length runs spliced in: after every fourth count a pair (0, 0) -- an empty run of the other value, then an
    empty run of this one -- and the string opens with (0, 0) as well.  It decodes to the same mask."""
    from tests import writer_oracle as wo
    counts = [0, 0]
    for k, c in enumerate(mask_counts(mask)):
        counts.append(int(c))
        if k % 4 == 3:
            counts += [0, 0]
    assert sum(counts) == mask.size
    return wo.counts_to_string(counts)


def union_case(h, w, seed=0):
    """(strings, plane_of_string, P) for one shape: planes with 0, 1, 2 and 130 strings; the big union first, in the middle and last;
    overlapping and disjoint strings; an all-zero and an all-one string inside unions; strings with zero-length runs; one malformed
    string of each status between valid ones in one plane.
       plane 0  130 strings (blobs, overlapping)          plane 1  nothing          plane 2  one string
       plane 3  two disjoint strings (left / right half)   plane 4  130 strings, among them an all-zero one and zero-run strings
       plane 5  valid, then each malformed string followed by a valid one
       plane 6  an all-one string between two blobs        plane 7  zero-length runs at a string's ends          plane 8  130 strings"""
    from tests import writer_oracle as wo
    rs = np.random.RandomState(seed + h * 1000 + w)
    allowed = rs.rand(h, w) < 0.5          # tiny shapes: single pixels out of a fixed half, so that a union of 130 does not fill the plane

    def blob():
        if h * w <= 64:
            m = np.zeros((h, w), np.uint8)
            ys, xs = np.nonzero(allowed)
            k = rs.randint(len(ys))
            m[ys[k], xs[k]] = 1
            return m
        return disc(h, w, rs.uniform(0, h), rs.uniform(0, w), rs.uniform(1, max(2.0, min(h, w) / 12.0)))
    strings, planes = [], []

    def add(q, s):
        strings.append(s if isinstance(s, str) else wo.counts_to_string(mask_counts(s)))
        planes.append(q)
    for _ in range(130):
        add(0, blob())
    add(2, blob())
    left = np.zeros((h, w), np.uint8)
    left[:, :max(w // 2, 1)] = 1
    if w == 1:
        left[h // 2:] = 0
    right = (1 - left) * (rs.rand(h, w) < 0.7).astype(np.uint8)
    add(3, left)
    add(3, right)
    for k in range(130):
        add(4, np.zeros((h, w), np.uint8) if k == 64 else (zero_run_string(blob()) if k % 3 == 0 else blob()))
    add(5, blob())
    for _, bad, _ in do.malformed_cases(h, w):
        add(5, bad)
        add(5, blob())
    add(6, blob())
    add(6, np.ones((h, w), np.uint8))
    add(6, blob())
    hw = h * w
    for counts in ([3, 2, hw - 5, 0], [0, 0, 0, 2, hw - 2], [hw - 1, 1], [hw - 1, 1, 0], [0, 1, hw - 1]):          # runs of length 0 at the ends
        add(7, wo.counts_to_string(counts))
    for _ in range(130):
        add(8, blob())
    return strings, planes, 9
