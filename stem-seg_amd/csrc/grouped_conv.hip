// Grouped 3x3 convolution (stride 1 or 2, pad 1) on the matrix cores: the bottleneck conv2 of a ResNeXt backbone
// (/root/reference/stemseg/modeling/backbone/resnet.py:240-249, groups = NUM_GROUPS) and the stride-in-3x3 conv2 of
// STRIDE_IN_1X1 = False (:227-238), + bias (the folded bn2) + ReLU (:273-275).
//
// GEMM view per 16-output-channel block:  D[co][pixel] = sum_{k = (window channel, tap)} A[co][k] * B[k][pixel].
// A block of 16 output channels reads a WINDOW of Kc = max(16, Cin_g) input channels:
//   * Cout_g = Cin_g >= 16: the window is the block's own group, no zero in A;
//   * Cin_g = 4 or 8: the block holds 16 / Cin_g whole groups whose inputs are the 16 consecutive channels of the window, and A is
//     block-diagonal there: 2x the algorithmic MFMA work at 8 channels per group, 4x at 4 (a dense block-diagonal GEMM over all
//     channels would be `groups` x);
//   * groups = 1 (the un-grouped stride-in-3x3 conv): the window is every input channel.
// The window is staged 16 channels at a time into LDS -- already split into the precision's operand planes, once per chunk -- and
// every tap is a shifted read of that tile; with stride 2 the reads step two columns, so only kept outputs are computed.
// Products on v_mfma_f32_16x16x4_f32 (f32: exact fp32 products), v_mfma_f32_16x16x32_bf16 (bf16x6: three exact bf16 terms, the six
// products of conv_igemm.h in the same order) or v_mfma_f32_16x16x32_f16 (f16x3: the power-of-two-scaled two-term fp16 split of
// conv_igemm.h, per-output-channel weight scale); fp32 accumulation.  One workgroup = one 16-channel block x 4 output rows x
// 32 output columns of one frame (a wave per row, two 16-column MFMA blocks per wave).  Every output's summation order is fixed by
// the chunk / tap / k order alone: no split-K, no decision on the frame count, so the bits do not depend on the batch.
#include "common.h"
#include "split_operand.h"
#include <algorithm>
#include <type_traits>

namespace stemseg {

constexpr int GC_TR = 4, GC_TC = 32, GC_CK = 16;   // output rows (= waves), output columns, input channels per staged chunk

typedef float gc_f32x4 __attribute__((ext_vector_type(4)));

struct GroupedConvParams {
    const float* in;              // zero-haloed input: element (c, t, Y, X) of the haloed view at in + c*in_cs + t*in_ts + Y*in_ys + X
    int64_t in_cs, in_ts, in_ys;
    int in_H, in_W;               // haloed extents (input rows / columns + 2)
    const void* wpk;
    const float* bias;
    float* out;
    int64_t out_cs, out_ts, out_ys;
    int Cout, Kc, T, Ho, Wo, relu;
    int tiles_x, tiles_y, n_cob;
};

template <int S>
struct GcGeom {
    static constexpr int PR = S * (GC_TR - 1) + 3;                 // staged input rows
    static constexpr int PC = S * (GC_TC - 1) + 3;                 // staged input columns
    static constexpr int PCP = (PC + 3) / 4 * 4;                   // LDS row pitch (words)
    static constexpr int PLANE = PR * PCP;                          // words of one channel (f32) / one channel pair (split modes)
};

// PREC: 0 f32, 2 bf16x6, 3 f16x3 (STEMSEG_PRECISION_*); S: stride
template <int PREC, int S>
__global__ __launch_bounds__(256) void grouped_conv3x3_kernel(const GroupedConvParams p) {
    using G = GcGeom<S>;
    constexpr bool SPLIT = PREC != 0;
    constexpr int NPX = PREC == 2 ? 3 : 2;                          // staged input planes of the split modes (bf16x6: hi, mid, lo; f16x3: hi, lo * 2^11)
    constexpr int NPL = 3;                                          // weight planes (bf16x6: hi, mid, lo; f16x3: hi, lo, hi * 2^-11)
    constexpr int LDS_WORDS = SPLIT ? NPX * (GC_CK / 2) * G::PLANE : GC_CK * G::PLANE;
    __shared__ __attribute__((aligned(16))) unsigned int lds[LDS_WORDS];

    int b = blockIdx.x;
    const int cob = b % p.n_cob; b /= p.n_cob;
    const int tx = b % p.tiles_x; b /= p.tiles_x;
    const int ty = b % p.tiles_y;
    const int t = b / p.tiles_y;
    const int co0 = cob * 16, y0 = ty * GC_TR, x0 = tx * GC_TC;
    const int kb = (co0 / p.Kc) * p.Kc;                             // first input channel of the block's window
    const int nck = p.Kc / GC_CK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, c16 = lane & 15;
    const float* in_t = p.in + (int64_t)t * p.in_ts;
    const int Y0 = S * y0, X0 = S * x0;                             // haloed origin of the staged patch

    // three accumulator sets -- f32: one per tap row dy, split modes: k-step s into set s % 3 -- added in fixed order at the end: chains a
    // third as long (over 1152 k-values of a one-group conv the fp32 accumulation error of a single chain exceeds 3x that of a blocked sum)
    // and independent MFMAs to cover the dependent latency
    gc_f32x4 acc[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) acc[k][nb] = gc_f32x4{0.f, 0.f, 0.f, 0.f};

    // per-lane LDS word offset of output (row = wave, column 16 nb + c16) at tap (0, 0)
    const int bbase = (S * wave) * G::PCP + S * c16;

    for (int ch = 0; ch < nck; ++ch) {
        const int cbase = kb + ch * GC_CK;
        // ---- A fragments of the chunk (global; the same slab serves every tile of the block) ----
        if constexpr (!SPLIT) {
            const float* wa = reinterpret_cast<const float*>(p.wpk) + ((int64_t)cob * nck + ch) * (9 * 4 * 64) + lane;
            float a[36];
#pragma unroll
            for (int s = 0; s < 36; ++s) a[s] = wa[s * 64];
            __syncthreads();                                        // the previous chunk's fragment reads are done
            for (int i = threadIdx.x; i < GC_CK * G::PR * G::PC; i += 256) {
                const int col = i % G::PC, r = i / G::PC, row = r % G::PR, c = r / G::PR;
                const int Y = Y0 + row, X = X0 + col;
                float v = 0.f;
                if (Y < p.in_H && X < p.in_W) v = in_t[(int64_t)(cbase + c) * p.in_cs + (int64_t)Y * p.in_ys + X];
                reinterpret_cast<float*>(lds)[c * G::PLANE + row * G::PCP + col] = v;
            }
            __syncthreads();
            const float* bl = reinterpret_cast<const float*>(lds) + bbase;
            // k-step s = (tap, i): lane quad q holds window channel 4 i + q
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int dy = tap / 3, dx = tap % 3;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float* bp = bl + (4 * i + q) * G::PLANE + dy * G::PCP + dx;
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb)
                        acc[dy][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[tap * 4 + i], bp[S * 16 * nb], acc[dy][nb], 0, 0, 0);
                }
            }
        } else {
            typedef typename std::conditional<PREC == 3, _Float16, __bf16>::type h16;
            typedef h16 h16x8 __attribute__((ext_vector_type(8)));
            const uint4* wa = reinterpret_cast<const uint4*>(p.wpk) + ((int64_t)cob * nck + ch) * (5 * NPL * 64) + lane;
            uint4 a[5][NPL];
#pragma unroll
            for (int s = 0; s < 5; ++s)
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) a[s][pl] = wa[(s * NPL + pl) * 64];
            __syncthreads();
            // stage: one item = the same position of a channel pair, split into the planes' words (low half: the even channel)
            for (int i = threadIdx.x; i < (GC_CK / 2) * G::PR * G::PC; i += 256) {
                const int col = i % G::PC, r = i / G::PC, row = r % G::PR, pr = r / G::PR;
                const int Y = Y0 + row, X = X0 + col;
                float v0 = 0.f, v1 = 0.f;
                if (Y < p.in_H && X < p.in_W) {
                    const float* src = in_t + (int64_t)(cbase + 2 * pr) * p.in_cs + (int64_t)Y * p.in_ys + X;
                    v0 = src[0];
                    v1 = src[p.in_cs];
                }
                unsigned int w[NPX];
                float vv[2] = {v0, v1};
                unsigned short hs[2][3];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float x = vv[k];
                    if constexpr (PREC == 3) {
                        split_act_f16(x, hs[k][0], hs[k][1]);
                        hs[k][2] = 0;
                    } else split_bf16x3(x, hs[k][0], hs[k][1], hs[k][2]);
                }
#pragma unroll
                for (int pl = 0; pl < NPX; ++pl) w[pl] = (unsigned int)hs[0][pl] | ((unsigned int)hs[1][pl] << 16);
#pragma unroll
                for (int pl = 0; pl < NPX; ++pl) lds[(pl * (GC_CK / 2) + pr) * G::PLANE + row * G::PCP + col] = w[pl];
            }
            __syncthreads();
            // k-step s (32 k): lane quad q holds tap 2 s + (q >> 1) (the tenth tap slot: zero weights, tap 8's address), window
            // channels 8 (q & 1) + 0..7 = pairs 4 (q & 1) + 0..3
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const int tap = min(2 * s + (q >> 1), 8), dy = tap / 3, dx = tap % 3;
                const unsigned int* bl = lds + (4 * (q & 1)) * G::PLANE + bbase + dy * G::PCP + dx;
                h16x8 bf[NPX][2];
#pragma unroll
                for (int pl = 0; pl < NPX; ++pl)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        uint4 w4;
                        const unsigned int* bp = bl + pl * (GC_CK / 2) * G::PLANE + S * 16 * nb;
                        w4.x = bp[0]; w4.y = bp[G::PLANE]; w4.z = bp[2 * G::PLANE]; w4.w = bp[3 * G::PLANE];
                        bf[pl][nb] = __builtin_bit_cast(h16x8, w4);
                    }
                h16x8 af[NPL];
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) af[pl] = __builtin_bit_cast(h16x8, a[s][pl]);
                if constexpr (PREC == 3) {
#define SS_GC_TERM(PA, PB)                                                                                          \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) acc[s % 3][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[PA], bf[PB][nb], acc[s % 3][nb], 0, 0, 0);
                    SS_GC_TERM(1, 0) SS_GC_TERM(2, 1) SS_GC_TERM(0, 0)      // lo_w * hi_x, (hi_w 2^-11) * (lo_x 2^11), hi_w * hi_x
#undef SS_GC_TERM
                } else {
#define SS_GC_TERM(PA, PB)                                                                                          \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) acc[s % 3][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[PA], bf[PB][nb], acc[s % 3][nb], 0, 0, 0);
                    SS_GC_TERM(2, 0) SS_GC_TERM(0, 2) SS_GC_TERM(1, 1) SS_GC_TERM(1, 0) SS_GC_TERM(0, 1) SS_GC_TERM(0, 0)   // smallest first
#undef SS_GC_TERM
                }
            }
        }
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) acc[0][nb] = (acc[0][nb] + acc[1][nb]) + acc[2][nb];
    // ---- epilogue: C/D layout col = lane & 15 (output column), row = 4 q + r (output channel) ----
    const int y = y0 + wave;
    if (y >= p.Ho) return;
    float sc[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (PREC == 3) {
        // undo the operand scales (powers of two: exact): 1 / (weight scale of the channel x activation scale), behind the slabs
        const float* invp = reinterpret_cast<const float*>(reinterpret_cast<const uint4*>(p.wpk) + (int64_t)p.n_cob * nck * (5 * NPL * 64));
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[r] = invp[co0 + 4 * q + r];
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int x = x0 + 16 * nb + c16;
        if (x >= p.Wo) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + 4 * q + r;
            float v = acc[0][nb][r];
            if constexpr (PREC == 3) v *= sc[r];
            v += p.bias ? p.bias[co] : 0.f;
            if (p.relu) v = relu_keep_nan(v);
            p.out[(int64_t)co * p.out_cs + (int64_t)t * p.out_ts + (int64_t)y * p.out_ys + x] = v;
        }
    }
}

// ---- packing: [Cout][Cin_g][3][3] -> per (16-channel block, 16-channel chunk of the window) the A fragments in lane order --------
// f32:    [blk][chunk][tap 9][i 4][lane 64] floats: lane (q, row) holds w(co = 16 blk + row, window channel 16 chunk + 4 i + q, tap)
// split:  [blk][chunk][step 5][plane 3][lane 64][8 x 16 bit]: element j of lane (q, row) is tap 2 step + (q >> 1) (zero for the tenth),
//         window channel 16 chunk + 8 (q & 1) + j; f16x3 then holds float inv[Cout] and uint32 max_bits[Cout]
struct GcPackDims { int Cout, Cg, Kc, nck; };

__device__ __forceinline__ float gc_window_weight(const float* __restrict__ w, const GcPackDims d, int co, int kchan, int tap) {
    if (tap > 8) return 0.f;
    const int kb = ((co & ~15) / d.Kc) * d.Kc, a = kb + kchan, g = co / d.Cg;
    if (a < g * d.Cg || a >= (g + 1) * d.Cg) return 0.f;          // another group's channel: the block-diagonal zero
    return w[((int64_t)co * d.Cg + (a - g * d.Cg)) * 9 + tap];
}

__global__ void gc_pack_f32_kernel(const float* __restrict__ w, float* __restrict__ packed, const GcPackDims d) {
    const int64_t n = (int64_t)(d.Cout / 16) * d.nck * 9 * 4 * 64;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int l = (int)(i & 63);
        int64_t r = i >> 6;
        const int ii = (int)(r & 3);
        r >>= 2;
        const int tap = (int)(r % 9);
        r /= 9;
        const int chunk = (int)(r % d.nck), blk = (int)(r / d.nck);
        packed[i] = gc_window_weight(w, d, blk * 16 + (l & 15), chunk * 16 + 4 * ii + (l >> 4), tap);
    }
}

// f16x3: per-output-channel weight scale and inv[co] = 1 / (S[co] x activation scale), as split_operand.h defines them
__global__ void gc_f16_scale_kernel(const float* __restrict__ w, float* __restrict__ inv, unsigned int* __restrict__ max_bits, const GcPackDims d) {
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= d.Cout) return;
    unsigned int m = 0;
    for (int k = 0; k < d.Cg * 9; ++k) m = max(m, __float_as_uint(fabsf(w[(int64_t)co * d.Cg * 9 + k])));
    max_bits[co] = m;
    inv[co] = f16x3_inv_scale(m);
}

template <int PREC>
__global__ void gc_pack_split_kernel(const float* __restrict__ w, uint4* __restrict__ packed, const unsigned int* __restrict__ max_bits, const GcPackDims d) {
    const int64_t n = (int64_t)(d.Cout / 16) * d.nck * 5 * 3 * 64;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int l = (int)(i & 63);
        int64_t r = i >> 6;
        const int pl = (int)(r % 3);
        r /= 3;
        const int step = (int)(r % 5);
        r /= 5;
        const int chunk = (int)(r % d.nck), blk = (int)(r / d.nck);
        const int co = blk * 16 + (l & 15), qq = l >> 4;
        const float S = PREC == 3 ? f16x3_weight_scale(max_bits[co]) : 1.0f;
        unsigned short v[8];
        for (int j = 0; j < 8; ++j) {
            const float x = gc_window_weight(w, d, co, chunk * 16 + 8 * (qq & 1) + j, 2 * step + (qq >> 1)) * S;
            v[j] = pack_split_weight<PREC>(x, pl);
        }
        uint4 o;
        o.x = v[0] | ((unsigned)v[1] << 16); o.y = v[2] | ((unsigned)v[3] << 16);
        o.z = v[4] | ((unsigned)v[5] << 16); o.w = v[6] | ((unsigned)v[7] << 16);
        packed[i] = o;
    }
}

// Per-group widths the kernel takes: 4, 8, 16, 32, 64 (ResNeXt 32x4d, 32x8d, 64x4d at every stage); one group: any multiple of 16.
static bool gc_width_ok(int Cg, int groups) {
    if (groups == 1) return Cg >= 16 && Cg % 16 == 0;
    return Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32 || Cg == 64;
}
static int gc_dims(int Cout, int Cin_g, int groups, GcPackDims& d) {
    SS_CHECK_ARG(groups >= 1 && Cout >= 16 && Cout % groups == 0, "grouped conv: Cout=%d, groups=%d", Cout, groups);
    const int Cg = Cout / groups;
    SS_CHECK_ARG(Cin_g == Cg, "grouped conv: Cin per group (%d) must equal Cout per group (%d)", Cin_g, Cg);
    SS_CHECK_ARG(gc_width_ok(Cg, groups), "grouped conv: %d channels per group unsupported (4, 8, 16, 32, 64; one group: a multiple of 16)", Cg);
    SS_CHECK_ARG(Cout % 16 == 0, "grouped conv: Cout=%d (multiple of 16)", Cout);
    d.Cout = Cout; d.Cg = Cg; d.Kc = std::max(16, Cg); d.nck = d.Kc / GC_CK;
    return STEMSEG_OK;
}
static int64_t gc_packed_bytes(const GcPackDims& d, int precision) {
    const int64_t blocks = (int64_t)(d.Cout / 16) * d.nck;
    if (precision == STEMSEG_PRECISION_F32) return blocks * 9 * 4 * 64 * 4;
    if (precision == STEMSEG_PRECISION_BF16X6) return blocks * 5 * 3 * 64 * 16;
    if (precision == STEMSEG_PRECISION_F16X3) return blocks * 5 * 3 * 64 * 16 + 8 * (int64_t)d.Cout;
    return 0;
}

int launch_grouped_conv(const StemsegVolume& in, const void* packed_w, const float* bias, const StemsegVolume& out, int groups, int stride,
                        int relu, int precision, hipStream_t s) {
    SS_CHECK_ARG(in.ptr && packed_w && out.ptr, "grouped conv: null pointer");
    SS_CHECK_ARG(stride == 1 || stride == 2, "grouped conv: stride %d (1 or 2)", stride);
    SS_CHECK_ARG(precision == STEMSEG_PRECISION_F32 || precision == STEMSEG_PRECISION_BF16X6 || precision == STEMSEG_PRECISION_F16X3,
                 "grouped conv: precision must be 0 (f32), 2 (bf16x6) or 3 (f16x3)");
    GcPackDims d;
    SS_CHECK_ARG(groups >= 1 && in.C % groups == 0, "grouped conv: %d input channels in %d groups", in.C, groups);
    int rc = gc_dims(out.C, in.C / groups, groups, d);
    if (rc) return rc;
    const int Hin = in.H - 2, Win = in.W - 2;
    SS_CHECK_ARG(Hin >= 1 && Win >= 1 && in.T >= 1, "grouped conv: the input is the zero-haloed view (H, W = map + 2)");
    const int Ho = (Hin - 1) / stride + 1, Wo = (Win - 1) / stride + 1;
    SS_CHECK_ARG(out.T == in.T && out.H == Ho && out.W == Wo, "grouped conv: output must be [%d][%d][%d][%d] (got [%d][%d][%d][%d])", out.C, in.T, Ho, Wo,
                 out.C, out.T, out.H, out.W);
    // every element the kernel reads / writes lies inside the caller's limits (staged reads stop at the haloed extents)
    const int64_t in_last = (int64_t)(in.C - 1) * in.c_stride + (int64_t)(in.T - 1) * in.t_stride + (int64_t)(in.H - 1) * in.y_stride + in.W - 1;
    const int64_t out_last = (int64_t)(out.C - 1) * out.c_stride + (int64_t)(out.T - 1) * out.t_stride + (int64_t)(out.H - 1) * out.y_stride + out.W - 1;
    SS_CHECK_ARG(in_last < in.limit && out_last < out.limit, "grouped conv: volume extents exceed their limits");
    GroupedConvParams p;
    p.in = in.ptr; p.in_cs = in.c_stride; p.in_ts = in.t_stride; p.in_ys = in.y_stride; p.in_H = in.H; p.in_W = in.W;
    p.wpk = packed_w; p.bias = bias; p.out = out.ptr; p.out_cs = out.c_stride; p.out_ts = out.t_stride; p.out_ys = out.y_stride;
    p.Cout = out.C; p.Kc = d.Kc; p.T = in.T; p.Ho = Ho; p.Wo = Wo; p.relu = relu ? 1 : 0;
    p.tiles_x = (int)ceil_div(Wo, GC_TC); p.tiles_y = (int)ceil_div(Ho, GC_TR); p.n_cob = out.C / 16;
    const int64_t wgs = (int64_t)p.n_cob * p.tiles_x * p.tiles_y * in.T;
    SS_CHECK_ARG(wgs < (1ll << 31), "grouped conv: too many tiles");
    const double flops = 2.0 * out.C * d.Cg * 9.0 * in.T * Ho * Wo;
    void* ev = profile_begin(51, flops, s);
#define SS_GC_LAUNCH(PREC, S) hipLaunchKernelGGL((grouped_conv3x3_kernel<PREC, S>), dim3((unsigned)wgs), dim3(256), 0, s, p)
    if (precision == STEMSEG_PRECISION_F32) { if (stride == 1) SS_GC_LAUNCH(0, 1); else SS_GC_LAUNCH(0, 2); }
    else if (precision == STEMSEG_PRECISION_BF16X6) { if (stride == 1) SS_GC_LAUNCH(2, 1); else SS_GC_LAUNCH(2, 2); }
    else { if (stride == 1) SS_GC_LAUNCH(3, 1); else SS_GC_LAUNCH(3, 2); }
#undef SS_GC_LAUNCH
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

}  // namespace stemseg

using namespace stemseg;

extern "C" int64_t stemseg_hip_packed_grouped_weight_bytes(int32_t Cout, int32_t Cin_g, int32_t groups, int32_t precision) {
    GcPackDims d;
    if (gc_dims(Cout, Cin_g, groups, d) != STEMSEG_OK) return 0;
    return gc_packed_bytes(d, precision);
}

extern "C" int stemseg_hip_pack_grouped_conv_weight(const float* w, void* packed, int32_t Cout, int32_t Cin_g, int32_t groups, int32_t precision,
                                                    void* stream) {
    SS_CHECK_ARG(w && packed, "pack_grouped_conv_weight: null pointer");
    GcPackDims d;
    int rc = gc_dims(Cout, Cin_g, groups, d);
    if (rc) return rc;
    SS_CHECK_ARG(gc_packed_bytes(d, precision) > 0, "pack_grouped_conv_weight: precision must be 0 (f32), 2 (bf16x6) or 3 (f16x3)");
    hipStream_t s = as_stream(stream);
    if (precision == STEMSEG_PRECISION_F32) {
        const int64_t n = gc_packed_bytes(d, precision) / 4;
        hipLaunchKernelGGL(gc_pack_f32_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(n, 256), 4096)), dim3(256), 0, s, w, reinterpret_cast<float*>(packed), d);
        SS_LAUNCH_CHECK();
        return STEMSEG_OK;
    }
    const int64_t n = (int64_t)(d.Cout / 16) * d.nck * 5 * 3 * 64;
    const int blocks = (int)std::min<int64_t>(ceil_div(n, 256), 4096);
    uint4* slabs = reinterpret_cast<uint4*>(packed);
    if (precision == STEMSEG_PRECISION_BF16X6) {
        hipLaunchKernelGGL(gc_pack_split_kernel<2>, dim3(blocks), dim3(256), 0, s, w, slabs, (const unsigned int*)nullptr, d);
    } else {
        float* inv = reinterpret_cast<float*>(slabs + n);
        unsigned int* max_bits = reinterpret_cast<unsigned int*>(inv + d.Cout);
        hipLaunchKernelGGL(gc_f16_scale_kernel, dim3((unsigned)ceil_div(d.Cout, 256)), dim3(256), 0, s, w, inv, max_bits, d);
        SS_LAUNCH_CHECK();
        hipLaunchKernelGGL(gc_pack_split_kernel<3>, dim3(blocks), dim3(256), 0, s, w, slabs, (const unsigned int*)max_bits, d);
    }
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_conv2d_grouped(const StemsegVolume* in, const void* packed_w, const float* bias, const StemsegVolume* out, int32_t groups,
                                          int32_t stride, int32_t relu, int32_t precision, int32_t plan_frames, void* stream) {
    SS_CHECK_ARG(in && out, "conv2d_grouped: null volume");
    SS_CHECK_ARG(plan_frames >= 0, "conv2d_grouped: plan_frames=%d", plan_frames);   // (no split-K: the bits never depend on it)
    return launch_grouped_conv(*in, packed_w, bias, *out, groups, stride, relu, precision, as_stream(stream));
}
