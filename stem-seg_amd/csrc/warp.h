// Shared by the augmentation kernels (augment.hip): the colour jitter of one pixel and the rounding of a resampled value, in unfused
// fp32 with a fixed operation order -- the discipline of bilinear.h -- so that tests/augment_oracle.py restates them bit for bit in
// numpy float32.
#pragma once
#include "common.h"

// __fmul_rn / __fadd_rn / __dmul_rn / ... are plain operators to this compiler, compiled in its header under HIP's default contraction:
// inlined, a product and the sum it feeds fuse into an FMA.  From here to the end of the translation unit (augment.hip alone includes
// this file) nothing is contracted, and the kernels do their arithmetic through the helpers below, which are compiled under that rule.
#pragma clang fp contract(off)

namespace stemseg {
namespace {

__device__ __forceinline__ float fmul(float a, float b) { return a * b; }
__device__ __forceinline__ float fadd(float a, float b) { return a + b; }
__device__ __forceinline__ float fsub(float a, float b) { return a - b; }
__device__ __forceinline__ float fdiv(float a, float b) { return a / b; }          // (correctly rounded: hipcc's default for fp32 division)
__device__ __forceinline__ double dmul(double a, double b) { return a * b; }
__device__ __forceinline__ double dadd(double a, double b) { return a + b; }
__device__ __forceinline__ double dsub(double a, double b) { return a - b; }
__device__ __forceinline__ double ddiv(double a, double b) { return a / b; }

struct Bgr { int b, g, r; };

__device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// floor(v + 0.5) clamped to 0 .. 255 (v is finite: a weighted sum of bytes)
__device__ __forceinline__ int round_u8(float v) {
    const float f = floorf(fadd(v, 0.5f));
    return f < 0.f ? 0 : (f > 255.f ? 255 : (int)f);
}

// (b, g, r) -> (b, g, r): stemseg_hip.h "jitter of a pixel".  add and hs are taken clamped to +-255.
//   HSV by cv2's documented 8-bit convention: V = max, S = 255 (V - min) / V, H = (60 (g - b) / (V - min) | 120 + 60 (b - r) / .. |
//   240 + 60 (r - g) / ..) by which of r, g, b is the maximum (in that order), + 360 if negative, halved; each rounded to nearest.
__device__ __forceinline__ Bgr jitter_pixel(int b, int g, int r, int add, int hs, int flags) {
    add = add < -255 ? -255 : (add > 255 ? 255 : add);
    hs = hs < -255 ? -255 : (hs > 255 ? 255 : hs);
    if (flags & STEMSEG_JITTER_ADD) {
        b = clamp_u8(b + add); g = clamp_u8(g + add); r = clamp_u8(r + add);
    }
    if (flags & STEMSEG_JITTER_HUE_SAT) {
        const int V = max(b, max(g, r)), diff = V - min(b, min(g, r));
        int S = 0, Hh = 0;
        if (V > 0) S = (int)floorf(fadd(fdiv(fmul(255.f, (float)diff), (float)V), 0.5f));
        if (diff > 0) {
            const float fd = (float)diff;
            float h;
            if (V == r) h = fdiv(fmul(60.f, (float)(g - b)), fd);
            else if (V == g) h = fadd(120.f, fdiv(fmul(60.f, (float)(b - r)), fd));
            else h = fadd(240.f, fdiv(fmul(60.f, (float)(r - g)), fd));
            if (h < 0.f) h = fadd(h, 360.f);
            Hh = (int)floorf(fadd(fmul(h, 0.5f), 0.5f));
            if (Hh >= 180) Hh -= 180;
        }
        Hh = ((Hh + (hs * 180) / 255) % 180 + 180) % 180;          // (integer division truncates towards zero)
        S = clamp_u8(S + hs);
        const int sector = Hh / 30;
        const float f = fdiv((float)(Hh - 30 * sector), 30.f), s = fdiv((float)S, 255.f), v = (float)V;
        const float p = fmul(v, fsub(1.f, s));
        const float q = fmul(v, fsub(1.f, fmul(s, f)));
        const float t = fmul(v, fsub(1.f, fmul(s, fsub(1.f, f))));
        float rr, gg, bb;
        switch (sector) {
            case 0: rr = v; gg = t; bb = p; break;
            case 1: rr = q; gg = v; bb = p; break;
            case 2: rr = p; gg = v; bb = t; break;
            case 3: rr = p; gg = q; bb = v; break;
            case 4: rr = t; gg = p; bb = v; break;
            default: rr = v; gg = p; bb = q; break;
        }
        b = round_u8(bb); g = round_u8(gg); r = round_u8(rr);
    }
    Bgr o;
    o.b = b; o.g = g; o.r = r;
    return o;
}

// the four taps of a bilinear read at (u, v), -1 < u < W and -1 < v < H: corner (x0, y0) = (floor u, floor v), fp32 weights from the
// fp64 fractions; tap (a, b) is pixel (x0 + b, y0 + a) with weight wy[a] * wx[b]
struct Taps4 { int x0, y0; float wx[2], wy[2]; };
__device__ __forceinline__ Taps4 make_taps4(double u, double v) {
    const double fu = floor(u), fv = floor(v);
    Taps4 t;
    t.x0 = (int)fu; t.y0 = (int)fv;
    t.wx[1] = (float)dsub(u, fu); t.wy[1] = (float)dsub(v, fv);
    t.wx[0] = fsub(1.f, t.wx[1]); t.wy[0] = fsub(1.f, t.wy[1]);
    return t;
}

}  // namespace
}  // namespace stemseg
