#!/usr/bin/env python3
"""Device JPEG decode (hip.jpeg_decode) against PIL, and the end-to-end effect on forward(paths, subseq_idxes).

    python tools/jpeg_decode_bench.py [--out profiles/jpeg_decode_bench.json] [--quick]

Frames are PIL-written q90 4:2:0 JPEGs of textured gradients (the matrix content of the tests), at 854x480 and 1280x720.
  decode    : per F in 1, 8, 64: the wall time of hip.jpeg_decode (marker parse, pinned upload, kernels, the status read) and the
              device time of the same call between two hipEvents on its stream, per frame; median of the repetitions
  sync      : the share of frames whose synchronisation took more than one round, and that reached the serial backstop,
              for the same content and for noise at q100
  pil       : PIL's single-threaded decode (Image.open(...).convert("RGB")) per frame on this host
  forward   : model(paths, subseq_idxes) wall time with device_decode on and off: a DAVIS-shaped sequence (70 frames at 854x480,
              davis preset, T = 8 clips with overlap 6) and a YouTube-VIS-shaped one (36 frames at 1280x720, ytvis preset, overlap
              4); synthetic weights.  Outputs are compared bit for bit.
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

from tests import jpeg_fixtures as X  # noqa: E402


def med(xs):
    return float(np.median(xs))


def bench_decode(hip, H, W, F, reps):
    files = [X.encode(X.content(H, W, s), 2, 90) for s in range(F)]
    hip.jpeg_decode(files)
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out, st = hip.jpeg_decode(files)
        e1.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        dev.append(e0.elapsed_time(e1) / 1e3)
    ok = all(torch.equal(out[i].cpu(), torch.from_numpy(X.pil_bgr(files[i]))) for i in range(min(F, 4)))
    mb = sum(len(f) for f in files) / 1e6
    return {"H": H, "W": W, "F": F, "compressed_MB": round(mb, 3), "wall_ms_per_frame": round(1e3 * med(wall) / F, 4),
            "device_ms_per_frame": round(1e3 * med(dev) / F, 4), "compressed_GB_per_s_device": round(mb / 1e3 / med(dev), 3),
            "status_corrupt_or_host": int((st & 0x81).astype(bool).sum()), "equal_to_pil": bool(ok)}


def sync_stats(hip, H, W, F, noise):
    files = [X.encode(X.content(H, W, s, noise=noise), 2, 100 if noise else 90) for s in range(F)]
    _, st = hip.jpeg_decode(files)
    return {"H": H, "W": W, "F": F, "content": "noise q100" if noise else "texture q90",
            "share_more_than_one_round": float(((st & hip.JPEG_STATUS_MULTI_ROUND) != 0).mean()),
            "frames_serial_backstop": int(((st & hip.JPEG_STATUS_BACKSTOP) != 0).sum())}


def pil_ms(H, W, n=10):
    from PIL import Image
    files = [X.encode(X.content(H, W, s), 2, 90) for s in range(n)]
    ts = []
    for f in files:
        t0 = time.perf_counter()
        np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        ts.append(time.perf_counter() - t0)
    return round(1e3 * med(ts), 3)


def clips(n, T, overlap):
    out, s = [], 0
    while True:
        out.append(list(range(s, min(s + T, n))))
        if s + T >= n:
            break
        s += T - overlap
    return out


def bench_forward(preset, n, H, W, overlap, tmp):
    from stemseg_amd import config
    from stemseg_amd.modeling.inference_model import InferenceModel
    from tests import synth
    config.load_preset(preset)
    try:
        model = InferenceModel(resize_scale=4.0 if preset == "ytvis" else 1.0)
        names = [(k, v.shape) for k, v in model._model.state_dict().items()]
        sd = synth.synth_state_dict(names, 7)
        model._model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(model._model.state_dict()[k].shape) for k, v in sd.items()})
        model = model.cuda()
        paths = []
        for t in range(n):
            p = os.path.join(tmp, "%s_%05d.jpg" % (preset, t))
            with open(p, "wb") as fh:
                fh.write(X.encode(X.content(H, W, 200 + t), 2, 90))
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
        return {"preset": preset, "frames": n, "H": H, "W": W, "clips": len(sub), "wall_s": res, "outputs_equal": bool(same)}
    finally:
        config.load_preset("defaults")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_bench.json"))
    ap.add_argument("--quick", action="store_true", help="the decode cases only, few repetitions (for the rocprofv3 run)")
    a = ap.parse_args()
    from stemseg_amd import hip
    hip.require_gpu()
    res = {"decode": [], "sync": [], "pil_ms_per_frame": {}, "forward": []}
    for (H, W) in ((480, 854), (720, 1280)):
        for F in (1, 8, 64):
            res["decode"].append(bench_decode(hip, H, W, F, 3 if a.quick else 10))
            print(json.dumps(res["decode"][-1]), flush=True)
        if a.quick:
            continue
        res["pil_ms_per_frame"]["%dx%d" % (W, H)] = pil_ms(H, W)
        for noise in (False, True):
            res["sync"].append(sync_stats(hip, H, W, 16, noise))
            print(json.dumps(res["sync"][-1]), flush=True)
    if not a.quick:
        with tempfile.TemporaryDirectory() as tmp:
            res["forward"].append(bench_forward("davis", 70, 480, 854, 6, tmp))
            print(json.dumps(res["forward"][-1]), flush=True)
            res["forward"].append(bench_forward("ytvis", 36, 720, 1280, 4, tmp))
            print(json.dumps(res["forward"][-1]), flush=True)
        res["device"] = torch.cuda.get_device_name(0)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print("OK")


if __name__ == "__main__":
    main()
