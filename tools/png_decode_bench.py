#!/usr/bin/env python3
"""Device PNG decode (hip.png_decode) against PIL, and the end-to-end effect on forward(paths, subseq_idxes).

    python tools/png_decode_bench.py [--out profiles/png_decode_bench.json] [--quick]

Frames are PIL-written RGB PNGs at its default level of textured gradients (the matrix content of the tests), at 1242x375
(KITTI-MOTS) and 854x480.
  decode    : per F in 1, 8, 16, 64: the wall time of hip.png_decode (chunk walk, pinned upload, kernels, the status read) and
              the time between two hipEvents on its stream around the same whole call, per frame; median of the repetitions.  The
              kernels alone: the rocprofv3 breakdown below
  backstop  : the share of frames in which the serial backstop decoded a block
  pil / cv2 : the single-threaded host decode (Image.open(...).convert("RGB"); cv2.imdecode where cv2 is installed) per frame
  forward   : model(paths, subseq_idxes) wall time with device_decode on and off on a KITTI-shaped sequence (40 PNG frames at
              1242x375, kittimots preset, T = 8 clips with overlap 4); synthetic weights.  Outputs are compared bit for bit.
The kernel breakdown per stage comes from a separate rocprofv3 --kernel-trace --stats run of this script with --quick.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "stem-seg_amd")]

from tests import png_fixtures as X  # noqa: E402


def med(xs):
    return float(np.median(xs))


def frame_file(H, W, s):
    return X.pil_png(X.pixels(H, W, 2, s))


def bench_decode(hip, H, W, F, reps):
    files = [frame_file(H, W, s) for s in range(F)]
    hip.png_decode(files)
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out, st = hip.png_decode(files)
        e1.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        dev.append(e0.elapsed_time(e1) / 1e3)
    ok = all(torch.equal(out[i].cpu(), torch.from_numpy(X.pil_bgr(files[i]))) for i in range(min(F, 4)))
    mb = sum(len(f) for f in files) / 1e6
    return {"H": H, "W": W, "F": F, "compressed_MB": round(mb, 3), "wall_ms_per_frame": round(1e3 * med(wall) / F, 4),
            "call_ms_per_frame_events": round(1e3 * med(dev) / F, 4), "status_corrupt_or_host": int((st & 0x81).astype(bool).sum()),
            "backstop_share": float(((st & hip.PNG_STATUS_BACKSTOP) != 0).mean()), "equal_to_pil": bool(ok)}


def host_ms(H, W, n=10):
    from PIL import Image
    files = [frame_file(H, W, s) for s in range(n)]
    res = {}
    ts = []
    for f in files:
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        ts.append(time.perf_counter() - t0)
    res["pil"] = round(1e3 * med(ts), 3)
    try:
        import cv2
    except ImportError:
        return res
    ts = []
    for f in files:
        t0 = time.perf_counter()
        cv2.imdecode(np.frombuffer(f, np.uint8), cv2.IMREAD_COLOR)
        ts.append(time.perf_counter() - t0)
    res["cv2"] = round(1e3 * med(ts), 3)
    return res


def clips(n, T, overlap):
    out, s = [], 0
    while True:
        out.append(list(range(s, min(s + T, n))))
        if s + T >= n:
            break
        s += T - overlap
    return out


def bench_forward(n, H, W, overlap, tmp):
    from stemseg_amd import config
    from stemseg_amd.modeling.inference_model import InferenceModel
    from tests import synth
    config.load_preset("kittimots")
    try:
        model = InferenceModel()
        names = [(k, v.shape) for k, v in model._model.state_dict().items()]
        sd = synth.synth_state_dict(names, 7)
        model._model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(model._model.state_dict()[k].shape) for k, v in sd.items()})
        model = model.cuda()
        paths = []
        for t in range(n):
            p = os.path.join(tmp, "kitti_%06d.png" % t)
            with open(p, "wb") as fh:
                fh.write(frame_file(H, W, 200 + t))
            paths.append(p)
        sub = clips(n, 8, overlap)
        res = {}
        outs = {}
        for flag in (False, True, False, True):
            model.device_decode = flag
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = model(paths, sub)
            torch.cuda.synchronize()
            res["device_decode" if flag else "host_decode"] = round(time.perf_counter() - t0, 4)     # the second (warm) run is kept
            outs[flag] = o
        same = all(torch.equal(a.embeddings, b.embeddings) and torch.equal(a.seediness, b.seediness)
                   for a, b in zip(outs[True]["embeddings"], outs[False]["embeddings"]))
        return {"preset": "kittimots", "frames": n, "H": H, "W": W, "clips": len(sub), "wall_s": res, "outputs_equal": bool(same)}
    finally:
        config.load_preset("defaults")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_bench.json"))
    ap.add_argument("--quick", action="store_true", help="the decode cases only, few repetitions (for the rocprofv3 run)")
    a = ap.parse_args()
    from stemseg_amd import hip
    hip.require_gpu()
    res = {"decode": [], "host_ms_per_frame": {}, "forward": []}
    for (H, W) in ((375, 1242), (480, 854)):
        for F in (1, 8, 16, 64):
            res["decode"].append(bench_decode(hip, H, W, F, 3 if a.quick else 10))
            print(json.dumps(res["decode"][-1]), flush=True)
        if a.quick:
            continue
        res["host_ms_per_frame"]["%dx%d" % (W, H)] = host_ms(H, W)
        print(json.dumps(res["host_ms_per_frame"]), flush=True)
    if not a.quick:
        with tempfile.TemporaryDirectory() as tmp:
            res["forward"].append(bench_forward(40, 375, 1242, 4, tmp))
            print(json.dumps(res["forward"][-1]), flush=True)
        res["device"] = torch.cuda.get_device_name(0)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print("OK")


if __name__ == "__main__":
    main()
