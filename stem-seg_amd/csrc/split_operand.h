// The split-operand format of the f16x3 / bf16x6 precisions: the ONE definition of its arithmetic and of the packed-weight layout.
//
//   bf16x6  every fp32 operand is split EXACTLY into three bf16 terms, x = hi + mid + lo (both remainders are exact fp32 subtractions)
//   f16x3   activations: x * 2^-2 = hi + lo in fp16, the low term stored as lo * 2^11; weights: w * S[co] = hi + lo in fp16 with a power-of-two
//           scale per output channel, and hi * 2^-11 as the third A operand (it meets the activations' lo * 2^11 plane)
//
// Consumers: conv_igemm.h (staging, pair-plane epilogue, descale), conv_pack.hip (packing, byte counts), bottleneck_fused.hip (pair split,
// inv tables, tile byte sizes) and grouped_conv.hip (the arithmetic only: its packed layout is a different format, with window channels).
#pragma once
#include "common.h"

namespace stemseg {

constexpr float F16X3_ACT_SCALE = 0.25f;      // f16x3: activations are split as fp16 terms of x * 2^-2
constexpr float F16X3_LO_SCALE = 2048.0f;     // f16x3: the activations' low term is stored as lo * 2^11, the weights supply hi_w * 2^-11 for it

// ---- arithmetic ------------------------------------------------------------------------------------------------------------------

// f16x3 split of the same position of a channel pair (x0: channel 2p, x1: channel 2p + 1) into the two words the staged planes hold:
// hw = (hi(x0), hi(x1)), lw = (lo(x0), lo(x1)) with hi = fp16(x / 4), lo = fp16((x / 4 - hi) * 2^11) -- the arithmetic of split_act_f16,
// bit for bit (x / 4 and the remainder are exact in fp32, so each term is rounded once), as six mixed-precision FMAs that write
// the fp16 halves in place: per value 3 VALU instructions instead of 6.5 (multiply, two conversions, subtract, scale-and-convert, pack).
// The staging of a 1x1 tile is ~150 VALU instructions per 24 MFMAs, two thirds of them this split.
__device__ __forceinline__ void split_pair_f16(const float x0, const float x1, unsigned int& hw, unsigned int& lw) {
    const float qs = F16X3_ACT_SCALE, ks = F16X3_LO_SCALE;            // (neither is an inline constant: one SGPR each)
    unsigned int h, l;
    float r0, r1;
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h) : "v"(x0), "s"(qs));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h) : "v"(x1), "s"(qs));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(r0) : "v"(x0), "s"(qs), "v"(h));
    asm("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r1) : "v"(x1), "s"(qs), "v"(h));
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(l) : "v"(r0), "s"(ks));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(l) : "v"(r1), "s"(ks));
    hw = h;
    lw = l;
}

// f16x3, one activation: x * 2^-2 = hi + lo with the low term stored as lo * 2^11: hi is a normal fp16 number for
// 2.5e-4 <= |x| < 2.6e5 and the pair keeps 22 significand bits there (2^-36 absolute when the low term is tiny, and below the range),
// inf above (and the result says so).  The accumulators are scaled back once, after the chunk loop.
__device__ __forceinline__ void split_act_f16(const float x, unsigned short& hi, unsigned short& lo) {
    const float xs = x * F16X3_ACT_SCALE;
    const _Float16 fh = (_Float16)xs;
    const _Float16 fl = (_Float16)((xs - (float)fh) * F16X3_LO_SCALE);
    hi = __builtin_bit_cast(unsigned short, fh);
    lo = __builtin_bit_cast(unsigned short, fl);
}

// exact three-way split of an fp32 value into bf16 terms (both remainders are exact fp32 subtractions): activations and weights alike
__device__ __forceinline__ void split_bf16x3(const float x, __bf16& hi, __bf16& mid, __bf16& lo) {
    hi = (__bf16)x;
    const float r1 = x - (float)hi;
    mid = (__bf16)r1;
    lo = (__bf16)(r1 - (float)mid);
}
__device__ __forceinline__ void split_bf16x3(const float x, unsigned short& hi, unsigned short& mid, unsigned short& lo) {      // the terms' bits
    __bf16 bh, bm, bl;
    split_bf16x3(x, bh, bm, bl);
    hi = __builtin_bit_cast(unsigned short, bh);
    mid = __builtin_bit_cast(unsigned short, bm);
    lo = __builtin_bit_cast(unsigned short, bl);
}

// f16x3 weight scale S[co] = 2^(13 - floor(log2(max|w[co]|))) PER OUTPUT CHANNEL, from the bits of max|w[co]| -- each channel's largest
// weight lands in [2^13, 2^14), so all three terms of every weight within 2^-16 of its channel's largest are normal fp16 numbers.
// (A scale per LAYER, as in round 3, loses bits on every channel whose weights sit far below the layer's largest: FrozenBN folded
// with eps = 0 multiplies each output channel by gamma / sqrt(var), make_layers.py:51-63, which spans orders of magnitude in
// trained checkpoints.)
__device__ __forceinline__ float f16x3_weight_scale(unsigned int max_bits) {
    const int e = (int)((max_bits >> 23) & 0xff);               // biased exponent of max|w| (0: zero / subnormal weights only -> scale 1)
    if (e == 0 || e == 0xff) return 1.0f;
    return __uint_as_float((unsigned int)min(max(127 + 13 - (e - 127), 1), 254) << 23);
}
// what the kernels multiply their accumulator rows by: 1 / (weight scale of the output channel x activation scale)
__device__ __forceinline__ float f16x3_inv_scale(unsigned int max_bits) { return 1.0f / (f16x3_weight_scale(max_bits) * F16X3_ACT_SCALE); }

// 16-bit plane `pl` of one packed weight.  f16x3 (x = w * S[co]): hi, lo, hi * 2^-11; bf16x6: hi, mid, lo
template <int PREC>
__device__ __forceinline__ unsigned short pack_split_weight(const float x, const int pl) {
    static_assert(PREC == STEMSEG_PRECISION_BF16X6 || PREC == STEMSEG_PRECISION_F16X3, "split-operand precisions");
    if constexpr (PREC == STEMSEG_PRECISION_F16X3) {
        const _Float16 hi = (_Float16)x;
        const _Float16 lo = (_Float16)(x - (float)hi);
        const _Float16 his = (_Float16)((float)hi * (1.0f / F16X3_LO_SCALE));
        return __builtin_bit_cast(unsigned short, pl == 0 ? hi : (pl == 1 ? lo : his));
    } else {
        __bf16 hi, mid, lo;
        split_bf16x3(x, hi, mid, lo);
        return __builtin_bit_cast(unsigned short, pl == 0 ? hi : (pl == 1 ? mid : lo));
    }
}

// ---- packed-weight layout --------------------------------------------------------------------------------------------------------
// [channel chunk][k-group][plane][lane half][Cout] x 16 B (eight 16-bit values); element j of (k-group grp, half) is channel
// cg * 2 CPH + half * CPH + j % CPH of the chunk, tap tg * TPG + j / CPH (cg = grp / NTG, tg = grp % NTG; zero beyond the last tap /
// channel); group-major so that a weight PHASE -- a run of k-groups -- is one contiguous LDS image.  f16x3: behind the last slab
// float inv[Cout] (f16x3_inv_scale), then uint32 max_bits[Cout] (bits of max|w[co]|, pack-time scratch).

// channel chunk by tap class: 27 taps 4, 9 taps 8 (f16x3: 16 -- a k-group is then ONE tap x 16 channels and the nine taps fill nine
// groups exactly; bf16x6's three planes of 16 channels do not fit the LDS), 16 taps (the stem) 16, 1 tap 32
constexpr int split_chunk_channels(int taps, int prec) { return taps == 27 ? 4 : (taps == 9 ? (prec == STEMSEG_PRECISION_F16X3 ? 16 : 8) : (taps == 16 ? 16 : 32)); }

struct SplitLayout {
    int CK;          // channels per chunk
    int TPG;         // taps per k-group of 16 (27 taps: 4 x 2 channels per lane half, 9 taps: 2 x 4, 1 tap: 1 x 8;
                     //   9 or 16 taps in 16-channel chunks: one tap x 16 channels per group, no padded tap slot)
    int CPH;         // channels per lane half of a k-group
    int NTG, NCG;    // tap groups, channel groups per chunk
    int G;           // k-groups per chunk
    int NPL;         // 16-bit planes of the staged weights (f16x3: hi, lo -- the third A operand is made in registers)
    constexpr SplitLayout(int taps, int prec, int ck)
        : CK(ck), TPG(taps >= 27 ? 4 : ((taps >= 9 && ck < 16) ? 2 : 1)), CPH(8 / TPG), NTG((taps + TPG - 1) / TPG), NCG(ck / (2 * CPH)),
          G(NTG * NCG), NPL(prec == STEMSEG_PRECISION_BF16X6 ? 3 : 2) {}
    constexpr SplitLayout(int taps, int prec) : SplitLayout(taps, prec, split_chunk_channels(taps, prec)) {}
    constexpr int chunks(int Cin) const { return (Cin + CK - 1) / CK; }
    constexpr int chunk_pieces() const { return NPL * G * 2; }                          // 16-B pieces of one chunk, per output channel
    constexpr int64_t slab_bytes(int Cout, int Cin) const { return (int64_t)chunks(Cin) * chunk_pieces() * Cout * 16; }
    constexpr int64_t inv_offset(int Cout, int Cin) const { return slab_bytes(Cout, Cin); }                       // f16x3: float inv[Cout]
    constexpr int64_t max_bits_offset(int Cout, int Cin) const { return slab_bytes(Cout, Cin) + 4 * (int64_t)Cout; }   // f16x3: uint32 max_bits[Cout]
    constexpr int64_t bytes(int Cout, int Cin) const { return slab_bytes(Cout, Cin) + (NPL == 2 ? 8 * (int64_t)Cout : 0); }      // (two planes = f16x3: + inv and max_bits)
};

}  // namespace stemseg
