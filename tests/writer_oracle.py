"""Test-side restatement of the YouTube-VIS / KITTI-MOTS writers, numpy only.

The reference writers cannot produce goldens here (they need pycocotools), so the formats are restated from their
descriptions.  The COCO RLE functions restate pycocotools 2.0 ``maskApi.c`` semantics (rleEncode, rleDecode, rleToString,
rleFrString, rleArea, rleToBbox) in this file's own words; the writer assembly restates the reference files cited per function.
"""
import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ COCO RLE (maskApi.c semantics)
def encode(mask):
    """rleEncode: binary [H, W] -> counts of alternating runs in column-major order, the first run counting zeros (possibly 0)."""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)          # column-major: p = x * H + y
    counts, cur, run = [], False, 0
    for v in flat:
        if v != cur:
            counts.append(run)
            run, cur = 0, v
        run += 1
    counts.append(run)
    return counts


def decode(counts, h, w):
    """rleDecode: counts -> binary [H, W]."""
    flat = np.zeros(h * w, dtype=bool)
    p, v = 0, False
    for c in counts:
        flat[p:p + c] = v
        p += c
        v = not v
    assert p == h * w, "counts sum to %d, not %d" % (p, h * w)
    return flat.reshape(w, h).T


def counts_to_string(counts):
    """rleToString: count i is sent as x = cnts[i], minus cnts[i-2] when i > 2; x goes out in 5-bit groups, least significant
    first, with an arithmetic shift; a group gets 0x20 while more follow ('more' is x != -1 after a group with bit 0x10 set, else
    x != 0); every group + 48 is one character."""
    out = []
    for i, c in enumerate(counts):
        x = int(c) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            g = x & 0x1f
            x >>= 5                                            # Python's >> is arithmetic on negative ints, as the C long
            more = (x != -1) if (g & 0x10) else (x != 0)
            if more:
                g |= 0x20
            out.append(chr(g + 48))
    return "".join(out)


def string_to_counts(s):
    """rleFrString: the inverse of counts_to_string."""
    counts, p = [], 0
    while p < len(s):
        x, shift, more = 0, 0, True
        while more:
            g = ord(s[p]) - 48
            p += 1
            x |= (g & 0x1f) << shift
            shift += 5
            more = bool(g & 0x20)
            if not more and (g & 0x10):
                x -= 1 << shift                                # sign-extend the last group
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def area(counts):
    """rleArea: the foreground runs are the odd-indexed counts."""
    return int(sum(counts[1::2]))


def to_bbox(counts, h):
    """rleToBbox, one run at a time: only an even number of counts is used; none -> zeros; x / y of the first and last pixel
    of every foreground run widen the box, and a run whose first and last pixel lie in different columns makes y span [0, h)."""
    m = (len(counts) // 2) * 2
    if m == 0:
        return [0, 0, 0, 0]
    xs, ys, xe, ye, cc, xp = None, None, None, None, 0, 0
    for j in range(m):
        cc += counts[j]
        t = cc - (j % 2)
        y, x = t % h, t // h
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys, ye = 0, h - 1
        xs = x if xs is None else min(xs, x)
        xe = x if xe is None else max(xe, x)
        ys = y if ys is None else min(ys, y)
        ye = y if ye is None else max(ye, y)
    return [xs, ys, xe - xs + 1, ye - ys + 1]


def encode_map(cmap, K):
    """All K planes of one condensed map [H, W] (value n = instance n): [(counts, string, area, bbox)] for n = 1..K."""
    h = cmap.shape[0]
    out = []
    for n in range(1, K + 1):
        c = encode(cmap == n)
        out.append((c, counts_to_string(c), area(c), to_bbox(c, h)))
    return out


# ------------------------------------------------------------------------------------------------ masks
@torch.no_grad()
def condensed_masks_wide(label_maps, keep, image_hw, crop_hw, mask_scale=4.0):
    """The mask chain of davis.py:79-110 / youtube_vis.py:140-155 with an int32 result, for more than 255 instances: one-hot
    planes -> bilinear x mask_scale -> crop -> bilinear resize -> > 0.5; later instances overwrite earlier ones."""
    maps = torch.as_tensor(np.asarray(label_maps))
    ih, iw = image_hw
    rh, rw = crop_hw
    out = []
    for t in range(maps.shape[0]):
        m = torch.stack([maps[t] == i for i in keep], 0).unsqueeze(0).float()
        m = F.interpolate(m, scale_factor=mask_scale, mode="bilinear", align_corners=False)[:, :, :rh, :rw]
        m = (F.interpolate(m, (ih, iw), mode="bilinear", align_corners=False) > 0.5)[0]
        cond = torch.zeros(ih, iw, dtype=torch.int32)
        for n in range(len(keep)):
            cond = torch.where(m[n], torch.tensor(n + 1, dtype=torch.int32), cond)
        out.append(cond)
    return torch.stack(out, 0).numpy()


# ------------------------------------------------------------------------------------------------ YouTube-VIS (youtube_vis.py)
def ytvis_keep(lifetimes, outlier, max_tracks):
    """youtube_vis.py:77-84: ids by descending lifetime (stable), outlier dropped, the first max_tracks."""
    ranked = sorted(lifetimes.items(), key=lambda kv: kv[1], reverse=True)
    return [k for k, _ in ranked if k != outlier][:max_tracks]


def ytvis_instances(seq_id, keep, pt_counts, label_maps, class_maps, masks):
    """youtube_vis.py:110-195 from the label maps at mask resolution [T, h, w] (0 = no point), the multi-class maps
    [T, C, h, w] and the condensed full-size masks [T, H, W]: score = points / the largest kept count; category = 1 + the first
    arg-max of softmax(sum over the instance's points of channels 1..C-1 / its point count); one RLE per frame."""
    max_pts = float(max(pt_counts[k] for k in keep))
    H, W = masks.shape[1:]
    out = []
    for n, k in enumerate(keep, 1):
        sel = label_maps == k                                               # [T, h, w]
        sums = np.stack([class_maps[:, c][sel].astype(np.float64).sum() for c in range(1, class_maps.shape[1])])
        probs = torch.from_numpy((sums / sel.sum()).astype(np.float32)).softmax(0).numpy()
        out.append({"video_id": seq_id, "score": float(pt_counts[k]) / max_pts, "category_id": int(np.argmax(probs)) + 1,
                    "segmentations": [{"size": [int(H), int(W)], "counts": counts_to_string(encode(masks[t] == n))}
                                      for t in range(masks.shape[0])]})
    return out


# ------------------------------------------------------------------------------------------------ KITTI-MOTS (kitti_mots.py)
def kitti_keep(pt_counts, lifetimes, outlier, max_tracks):
    """kitti_mots.py:56-66: the max_tracks ids with the most points (stable), then ordered by ascending lifetime (stable)."""
    ranked = [k for k, _ in sorted(pt_counts.items(), key=lambda kv: kv[1], reverse=True) if k != outlier][:max_tracks]
    return sorted(ranked, key=lambda k: lifetimes[k])


def kitti_lines(keep, label_maps, argmax_maps, masks):
    """kitti_mots.py:96-208: mapped id n = position in keep + 1; a line per frame in which the instance has points (even if its
    full-size mask is empty), grouped by id then frame; category = the most voted of (1, 2) over the instance's points, 1 on ties."""
    H, W = masks.shape[1:]
    lines = []
    for n, k in enumerate(keep, 1):
        sel = label_maps == k
        votes = {c: int((argmax_maps[sel] == c).sum()) for c in (1, 2)}
        cat = 1 if votes[1] >= votes[2] else 2
        for t in range(masks.shape[0]):
            if sel[t].any():
                lines.append("%d %d %d %d %d %s" % (t, cat * 1000 + n, cat, H, W, counts_to_string(encode(masks[t] == n))))
    return lines


def kitti_filter_lines(lines, min_car_area=150, min_person_area=250, min_len_car=3, min_len_person=10, min_ratio_car=0.35,
                       min_ratio_person=0.2, max_break_car=0.3, max_break_person=0.5):
    """kitti_mots_postprocessing.py:145-180 on the lines of one file: area >= the class minimum, area / bbox area > the class
    minimum (0 for an empty box), then per track (first-appearance order, frames ascending) time breaks / length <= the class
    maximum and length >= the class minimum."""
    dets = []
    for l in lines:
        f = l.split()
        c = string_to_counts(f[5])
        bb = to_bbox(c, int(f[3]))
        dets.append((int(f[0]), int(f[1]), int(f[2]), area(c), bb[2] * bb[3], l.strip()))
    dets = [d for d in dets if (d[2] == 1 and d[3] >= min_car_area) or (d[2] == 2 and d[3] >= min_person_area)]
    ratio = lambda d: 0.0 if d[4] == 0 else d[3] / float(d[4])
    dets = [d for d in dets if (d[2] == 1 and ratio(d) > min_ratio_car) or (d[2] == 2 and ratio(d) > min_ratio_person)]

    def by_track(ds):
        order, groups = [], {}
        for d in ds:
            if d[1] not in groups:
                order.append(d[1])
                groups[d[1]] = []
            groups[d[1]].append(d)
        return [sorted(groups[i], key=lambda d: d[0]) for i in order]
    kept = []
    for t in by_track(dets):
        br = sum(1 for a, b in zip(t, t[1:]) if b[0] - a[0] > 1) / float(len(t))
        if (t[0][2] == 1 and br > max_break_car) or (t[0][2] == 2 and br > max_break_person):
            continue
        kept.extend(t)
    out = []
    for t in by_track(kept):
        if (t[0][2] == 1 and len(t) < min_len_car) or (t[0][2] == 2 and len(t) < min_len_person):
            continue
        out.extend(t)
    return [d[5] for d in out]
