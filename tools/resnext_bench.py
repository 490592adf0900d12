#!/usr/bin/env python3
"""Times the ResNeXt-101 32x8d encoder (MODEL.RESNETS.NUM_GROUPS 32, WIDTH_PER_GROUP 8, STRIDE_IN_1X1 False) at 480x864, T = 8 x 4 clips
(32 frames in one pass), in each precision: ms per pass by CUDA events, plus the in-library profiler's time of the grouped 3x3 launches
(tag 51).  Prints one JSON line; --out writes it to a file.  Under ``rocprofv3 --kernel-trace --stats`` (a run of its own, --modes one
mode) the per-kernel table gives the grouped kernel's us per launch; --roofline FILE then reads that run's kernel_stats.csv and puts
bytes and FLOPs of the 33 grouped launches against their roofs.
    python tools/resnext_bench.py [--modes f16x3,bf16x6,f32] [--passes 6] [--out profiles/resnext101_32x8d_encoder.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/resnext_bench.py --modes f16x3 --passes 3
    python tools/resnext_bench.py --roofline DIR/run_results.db --modes f16x3     (the rocpd database, or a kernel_stats.csv)"""
import argparse
import csv
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "stem-seg_amd"))

# MI355X roofs (MI355X_MICROARCH.md): HBM3E 8 TB/s; fp32-input MFMA 157.3 TFLOP/s; dense bf16 / fp16 MFMA 2.5 PFLOP/s
HBM_BPS, F32_FLOPS, F16_FLOPS = 8.0e12, 157.3e12, 2.5e15
BLOCKS = (3, 4, 23, 3)


def grouped_launches(T=32, H=480, W=864, groups=32, width=8):
    """(Cout, channels per group, stride, Ho, Wo) of the 33 grouped conv2 launches of one pass, with their algorithmic FLOPs and the
    bytes an ideal kernel moves (input read once, output written once, fp32)."""
    out = []
    for st, n in enumerate(BLOCKS):
        mid, cg = groups * width << st, width << st
        h, w = H >> (2 + st), W >> (2 + st)
        for b in range(n):
            s = 2 if (b == 0 and st > 0) else 1
            hi, wi = h * s, w * s
            flops = 2.0 * mid * cg * 9 * T * h * w
            nbytes = 4.0 * mid * T * (hi * wi + h * w)
            out.append(dict(stage=st + 1, Cout=mid, cg=cg, stride=s, Ho=h, Wo=w, flops=flops, bytes=nbytes))
    return out


def roofline(path, mode):
    if path.endswith(".db"):
        rows = sqlite3.connect(path).execute("select count(*), sum(duration) from kernels where name like '%grouped_conv3x3_kernel%'").fetchall()
        calls, ns = int(rows[0][0]), float(rows[0][1] or 0)
    else:
        g = [r for r in csv.DictReader(open(path)) if "grouped_conv3x3_kernel" in r.get("Name", r.get("KernelName", ""))]
        calls, ns = sum(int(r["Calls"]) for r in g), sum(float(r["TotalDurationNs"]) for r in g)
    if not calls:
        raise SystemExit("no grouped_conv3x3_kernel dispatch in %s" % path)
    L = grouped_launches()
    passes = calls // len(L)
    flops, nbytes = sum(x["flops"] for x in L) * passes, sum(x["bytes"] for x in L) * passes
    peak = F32_FLOPS if mode == "f32" else F16_FLOPS
    # issued matrix work: bf16x6 6 products, f16x3 3 (x 10/9 tap padding), f32 1; groups of 8 channels: 2x (block-diagonal 16-row blocks)
    issued = {"f32": 1.0, "bf16x6": 6.0 * 10 / 9, "f16x3": 3.0 * 10 / 9}[mode]
    wide = [x for x in L if x["cg"] >= 16]
    narrow = [x for x in L if x["cg"] < 16]
    issued_flops = issued * (sum(x["flops"] for x in wide) + sum(x["flops"] * 16 / x["cg"] for x in narrow)) * passes
    t_mem, t_mfma = nbytes / HBM_BPS, issued_flops / peak
    t = ns * 1e-9
    return dict(mode=mode, kernel_calls=calls, passes=passes, us_per_launch=ns / calls / 1e3, total_ms=ns / 1e6,
                algorithmic_tflops=flops / t / 1e12, bytes_tbps=nbytes / t / 1e12,
                roof="hbm" if t_mem >= t_mfma else "matrix", roof_time_fraction=max(t_mem, t_mfma) / t,
                hbm_fraction=t_mem / t, matrix_fraction=t_mfma / t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f16x3,bf16x6,f32")
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--roofline", default=None, help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    a = ap.parse_args()
    modes = a.modes.split(",")
    if a.roofline:
        res = [roofline(a.roofline, m) for m in modes]
        line = json.dumps(dict(metric="resnext101_32x8d_grouped_conv_roofline", results=res))
    else:
        import torch
        from stemseg_amd import hip
        from stemseg_amd.modeling.backbone import ResNetFPN
        hip.require_gpu()
        torch.manual_seed(1)
        bb = ResNetFPN("R-101-FPN", 256, 32, 8, False).eval()
        with torch.no_grad():
            for _, p_ in bb.named_parameters():
                if p_.dim() >= 2:
                    p_.normal_(0, (2.0 / p_[0].numel()) ** 0.5)
        bb = bb.cuda()
        T, H, W = 32, 480, 864
        x = torch.randn(T, 3, H, W, device="cuda")       # (random He-initialised trunks grow deep activations: at x 50 they leave f16x3's range)
        outs = [torch.empty(256, 8, H // s, W // s, device="cuda") for _ in range(4) for s in (4, 8, 16, 32)]
        vols = [hip.dense_volume(o) for o in outs]
        res = []
        for m in modes:
            bb.precision = m
            for _ in range(2):
                bb.run_backbone_into(x, vols)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.passes + 1)]
            ev[0].record()
            for i in range(a.passes):
                bb.run_backbone_into(x, vols)
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.passes))
            hip.profile_enable(True)
            bb.run_backbone_into(x, vols)
            prof = hip.profile_read(64)
            hip.profile_enable(False)
            finite = all(bool(torch.isfinite(o).all()) for o in outs)
            g_ms, g_fl, g_n = prof.get(51, (0.0, 0.0, 0))
            res.append(dict(mode=m, median_ms_per_pass=ms[len(ms) // 2], min_ms=ms[0], frames_per_s=T * 1e3 / ms[len(ms) // 2], finite=finite,
                            grouped_launches=int(g_n), grouped_ms_profiled=g_ms, grouped_tflops_profiled=(g_fl / (g_ms * 1e-3) / 1e12) if g_ms else None))
        L = grouped_launches()
        line = json.dumps(dict(metric="resnext101_32x8d_encoder_pass", T=T, H=H, W=W, clips=4, results=res,
                               grouped_gflop_per_frame=sum(x["flops"] for x in L) / T / 1e9, grouped_gb_per_frame=sum(x["bytes"] for x in L) / T / 1e9,
                               device=torch.cuda.get_device_name(0)))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
