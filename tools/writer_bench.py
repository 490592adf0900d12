#!/usr/bin/env python3
"""Timing of the YouTube-VIS / KITTI-MOTS writers (not part of bench.py).

    python tools/writer_bench.py [--repeats 3] [--out profiles/writer_bench.json]

Synthetic sequences at dataset sizes -- moving boxes at mask resolution, the chainer's per-point inputs -- through the writers'
``process_sequence`` + ``save()``:
  ytvis        36 frames 720x1280, 10 tracks (max_tracks 10)
  kitti        300 frames 375x1242, 20 tracks
  kitti_u16    300 frames 375x1242, 300 tracks (uint16 index maps)
Per workload: the RLE plan + encode kernels alone (hipEvents, per frame), the writer's wall clock per sequence (and hipEvents
from its first to its last launch), and for comparison a numpy host encode of the same masks (copy to the host + vectorised
column-major run lengths + the string codec; timed on up to 36 frames, scaled to the sequence).
For ``ytvis`` and ``kitti`` also the visualisations (``save_visualization=True``): the overlay composite and the JPEG plan + encode
kernels alone on one chunk of the writer's frames (hipEvents, per frame), the writer's wall clock per sequence with the
visualisations on (frames served from memory: no image decode), and for comparison PIL's host encode (libjpeg-turbo, quality 95,
one thread) of the same composited frames.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stem-seg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synth(F, h, w, n_tracks, C, seed):
    rs = np.random.RandomState(seed)
    boxes = [(rs.randint(0, h - h // 4), rs.randint(0, w - w // 4), rs.randint(h // 16, h // 4), rs.randint(w // 16, w // 4),
              rs.randint(-2, 3), rs.randint(-3, 4)) for _ in range(n_tracks)]
    idx, lab, maps = [], [], np.zeros((F, h, w), np.int64)
    for t in range(F):
        m = maps[t]
        for k, (y, x, hh, ww, vy, vx) in enumerate(boxes, 1):
            yy, xx = int(np.clip(y + vy * t // 4, 0, h - hh)), int(np.clip(x + vx * t // 4, 0, w - ww))
            m[yy:yy + hh, xx:xx + ww] = k
        ys, xs = np.nonzero(m)
        idx.append((torch.from_numpy(ys).cuda(), torch.from_numpy(xs).cuda()))
        lab.append(torch.from_numpy(m[ys, xs]).cuda())
    counts = {k: int((maps == k).sum()) for k in range(1, n_tracks + 1)}
    life = {k: int((maps == k).reshape(F, -1).any(1).sum()) for k in counts}
    return maps, idx, lab, counts, life


def host_encode(masks_dev, K, max_frames):
    """numpy reference cost: D2H of the masks, then per (frame, instance) the column-major run lengths and the string.  Runs on
    the first ``max_frames`` frames and is scaled to the sequence (the Python string loop is slow)."""
    F = masks_dev.shape[0]
    n = min(F, max_frames)
    t0 = time.perf_counter()
    m = masks_dev[:n].cpu().numpy()
    if m.dtype == np.int16:
        m = m.view(np.uint16)
    out = 0
    for f in range(n):
        col = np.ascontiguousarray(m[f].T).reshape(-1)
        for k in range(1, K + 1):
            b = col == k
            ch = np.flatnonzero(b[1:] != b[:-1]) + 1
            pos = np.concatenate(([0] if b[0] else [], ch)).astype(np.int64)
            counts = np.diff(np.concatenate(([0], pos, [b.size])))
            s = []
            for i, c in enumerate(counts.tolist()):
                x = c - (int(counts[i - 2]) if i > 2 else 0)
                more = True
                while more:
                    g = x & 0x1f
                    x >>= 5
                    more = (x != -1) if (g & 0x10) else (x != 0)
                    s.append(chr((g | (0x20 if more else 0)) + 48))
            out += len(s)
    return (time.perf_counter() - t0) * F / n, out, n


def encode_kernels_ms(hip, masks, K, repeats):
    """plan + encode launches alone (buffers allocated once), hipEvents."""
    F, H, W = masks.shape
    ib = 1 if masks.dtype == torch.uint8 else 2
    r = hip.rle_encode(masks, K)
    cap = max(int(r.count_offsets[-1]) - F * K, 1) + 16
    l = hip.lib()
    ws_bytes = l.stemseg_hip_rle_workspace_bytes(F, H, W, K, cap)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    pc = torch.empty(F * K, dtype=torch.int32, device="cuda")
    pch = torch.empty(F * K, dtype=torch.int64, device="cuda")
    tot = torch.empty(3, dtype=torch.int64, device="cuda")
    counts = torch.empty(int(r.count_offsets[-1]) + 1, dtype=torch.int32, device="cuda")
    chars = torch.empty(len(r.chars) + 1, dtype=torch.uint8, device="cuda")
    cof = torch.empty(F * K + 1, dtype=torch.int64, device="cuda")
    chof = torch.empty(F * K + 1, dtype=torch.int64, device="cuda")
    area = torch.empty(F * K, dtype=torch.int32, device="cuda")
    bb = torch.empty(F * K * 4, dtype=torch.int32, device="cuda")
    P = hip.ptr
    times = []
    for _ in range(repeats + 1):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        hip.check(l.stemseg_hip_rle_plan(P(masks), ib, F, H, W, K, cap, P(ws), ws_bytes, P(pc), P(pch), P(tot), hip.stream()))
        e1.record()
        hip.check(l.stemseg_hip_rle_encode(P(masks), ib, F, H, W, K, cap, P(ws), ws_bytes, P(counts), P(cof), P(chars), P(chof), P(area),
                                           P(bb), hip.stream()))
        e2.record()
        torch.cuda.synchronize()
        times.append((e0.elapsed_time(e1), e1.elapsed_time(e2)))
    assert int(tot[0]) >= 0
    times = times[1:]
    plan = float(np.median([t[0] for t in times]))
    enc = float(np.median([t[1] for t in times]))
    return plan, enc


def synth_frames(n, ih, iw, seed):
    """Smooth BGR frames (gradients, a few soft blobs, mild noise): closer to video than uniform noise."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:ih, 0:iw].astype(np.float32)
    out = np.empty((n, ih, iw, 3), np.uint8)
    for t in range(n):
        img = np.stack([xx / iw * 180 + 30, yy / ih * 160 + 40, (xx + yy) / (ih + iw) * 120 + 60], 2)
        for _ in range(6):
            cy, cx, r = rs.uniform(0, ih), rs.uniform(0, iw), rs.uniform(20, 120)
            img += (rs.uniform(-60, 60, 3) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))[..., None])
        img += rs.randn(ih, iw, 3) * 3
        out[t] = np.clip(img, 0, 255).astype(np.uint8)
    return out


class FrameSequence(object):
    """A sequence whose frames come from memory (the writer's visualisation path without the image decode)."""

    def __init__(self, seq_id, frames, T):
        self.id, self.frames, self.T = seq_id, frames, T
        self.image_dims = tuple(frames.shape[1:3])

    def load_images(self, frame_idxes=None):
        return [self.frames[t % len(self.frames)] for t in (frame_idxes if frame_idxes is not None else range(self.T))]


def vis_kernels_ms(hip, masks, colors, frames, repeats):
    """composite and jpeg plan + encode launches alone on one chunk of frames, hipEvents; and the composited frames (host)."""
    n, H, W = frames.shape[:3]
    fr = torch.from_numpy(frames).cuda()
    m = masks[:n].contiguous()
    cols = torch.from_numpy(colors).cuda()
    l, P = hip.lib(), hip.ptr
    ws_bytes = l.stemseg_hip_jpeg_workspace_bytes(n, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    over = hip.vis_composite(fr, m, cols)
    data, _ = hip.jpeg_encode(over, 95)
    out = torch.empty(len(data) + 1, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ib = 1 if m.dtype == torch.uint8 else 2
    times = []
    for _ in range(repeats + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        hip.check(l.stemseg_hip_vis_composite(P(fr), P(m), ib, n, H, W, P(cols), cols.shape[0] - 1, P(over), hip.stream()))
        e[1].record()
        hip.check(l.stemseg_hip_jpeg_plan(P(over), n, H, W, 95, P(ws), ws_bytes, P(sizes), P(sizes[n:]), hip.stream()))
        e[2].record()
        hip.check(l.stemseg_hip_jpeg_encode(n, H, W, 95, P(ws), ws_bytes, P(out), out.numel(), P(offs), hip.stream()))
        e[3].record()
        torch.cuda.synchronize()
        times.append([e[i].elapsed_time(e[i + 1]) for i in range(3)])
    med = np.median(np.array(times[1:]), axis=0)
    return [float(v) / n for v in med], over.cpu().numpy(), len(data) / n


def host_pil_ms(over):
    import io
    from PIL import Image
    t0 = time.perf_counter()
    for f in over:
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(io.BytesIO(), "JPEG", quality=95)
    return 1e3 * (time.perf_counter() - t0) / len(over)


def run(name, fmt, F, ih, iw, n_tracks, max_tracks, repeats):
    from stemseg_amd import config, hip
    from stemseg_amd.inference.output_utils import KittiMOTSOutputGenerator, YoutubeVISOutputGenerator
    from stemseg_amd.modeling.inference_model import compute_resize_params_2
    config.load_preset(fmt)
    cfg = config.cfg
    rw, rh, _ = compute_resize_params_2((iw, ih), cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM)
    h, w = (rh + 31) // 32 * 32 // 4, (rw + 31) // 32 * 32 // 4
    C = 40 if fmt == "ytvis" else 3
    maps, idx, lab, counts, life = synth(F, h, w, n_tracks, C, seed=F + n_tracks)
    if fmt == "ytvis":
        cat = torch.randn(F, C, h, w, device="cuda")
    else:
        cat = torch.randint(0, 3, (F, h, w), device="cuda", dtype=torch.int64)
    seq = types.SimpleNamespace(id=1, image_dims=(ih, iw))
    walls, gpu = [], []
    with tempfile.TemporaryDirectory() as d:
        for i in range(repeats + 1):
            gen = (YoutubeVISOutputGenerator(d, -1, False) if fmt == "ytvis" else KittiMOTSOutputGenerator(d, -1, False))
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            keep, _ = gen.process_sequence(seq, idx, lab, counts, life, cat, (h, w), 4.0, max_tracks, device="cuda:0")
            e1.record()
            gen.save()
            torch.cuda.synchronize()
            if i:
                walls.append(time.perf_counter() - t0)
                gpu.append(e0.elapsed_time(e1))
        masks = gen.sequences[1]["masks"]
    K = len(keep)
    plan_ms, enc_ms = encode_kernels_ms(hip, masks, K, repeats)
    host_s, n_chars, host_frames = host_encode(masks, K, 36)
    res = dict(workload=name, frames=F, image=[ih, iw], mask=[h, w], tracks=n_tracks, kept=K, index_bytes=hip.index_bytes_for(K),
               rle_plan_ms=plan_ms, rle_encode_ms=enc_ms, rle_kernels_us_per_frame=1e3 * (plan_ms + enc_ms) / F,
               writer_wall_ms_per_sequence=1e3 * float(np.median(walls)), writer_events_ms_process_sequence=float(np.median(gpu)),
               host_numpy_encode_ms_per_sequence=1e3 * host_s,
               host_numpy_frames_timed=host_frames)
    if name in ("ytvis", "kitti"):
        from stemseg_amd.inference.output_utils.generators import VIS_CHUNK, pascal_color_map
        frames = synth_frames(VIS_CHUNK, ih, iw, seed=F)
        colors = pascal_color_map()[np.arange(K + 1) % 256]
        (comp, plan, enc), over, jpg_bytes = vis_kernels_ms(hip, masks, colors, frames, repeats)
        vseq = FrameSequence(1, frames, F)
        vwalls = []
        with tempfile.TemporaryDirectory() as d:
            for i in range(repeats + 1):
                gen = (YoutubeVISOutputGenerator(d, -1, True) if fmt == "ytvis" else KittiMOTSOutputGenerator(d, -1, True))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gen.process_sequence(vseq, idx, lab, counts, life, cat, (h, w), 4.0, max_tracks, device="cuda:0")
                gen.save()
                torch.cuda.synchronize()
                if i:
                    vwalls.append(time.perf_counter() - t0)
            n_jpg = len(os.listdir(os.path.join(d, "vis", "1" if fmt == "ytvis" else "0001")))
        assert n_jpg == F
        pil = host_pil_ms(over)
        res.update(vis_composite_us_per_frame=1e3 * comp, vis_jpeg_plan_us_per_frame=1e3 * plan, vis_jpeg_encode_us_per_frame=1e3 * enc,
                   vis_jpeg_kernels_us_per_frame=1e3 * (plan + enc), vis_jpeg_bytes_per_frame=jpg_bytes,
                   vis_writer_wall_ms_per_sequence=1e3 * float(np.median(vwalls)), vis_frames_per_kernel_call=len(frames),
                   host_pil_encode_ms_per_frame=pil, host_pil_encode_ms_per_sequence=pil * F)
    config.load_preset("defaults")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    a = ap.parse_args()
    from stemseg_amd import hip
    hip.require_gpu()
    wl = [("ytvis", "ytvis", 36, 720, 1280, 10, 10), ("kitti", "kittimots", 300, 375, 1242, 20, 1000),
          ("kitti_u16", "kittimots", 300, 375, 1242, 300, 1000)]
    out = dict(device=torch.cuda.get_device_name(0), results=[])
    for w in wl:
        if a.only and w[0] not in a.only.split(","):
            continue
        r = run(*w, repeats=a.repeats)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
