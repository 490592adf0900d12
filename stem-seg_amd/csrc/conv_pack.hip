// Weight packing for conv_igemm.h: the fp32-input layout [Cin/4][taps][4][Cout], and the split-operand layout of split_operand.h
// (bf16x6, f16x3).
#include "common.h"
#include "split_operand.h"
#include <algorithm>

namespace stemseg {

// [Cout][Cin][taps] -> [Cin/4][taps][4][Cout]
__global__ void pack_conv_weight_kernel(const float* __restrict__ w, float* __restrict__ packed, int Cout, int Cin, int taps) {
    const int64_t n = (int64_t)Cout * Cin * taps;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % Cout);
        int64_t r = i / Cout;
        const int c4 = (int)(r & 3);
        r >>= 2;
        const int tap = (int)(r % taps);
        const int chunk = (int)(r / taps);
        const int ci = chunk * 4 + c4;
        packed[i] = w[((int64_t)co * Cin + ci) * taps + tap];
    }
}

// f16x3: bits of max|w[co]| per output channel (the weight scale comes from them, split_operand.h)
__global__ __launch_bounds__(256) void absmax_rows_kernel(const float* __restrict__ w, int64_t row_len, unsigned int* __restrict__ out) {
    __shared__ unsigned int red[4];
    const float* r = w + (int64_t)blockIdx.x * row_len;
    unsigned int m = 0;
    for (int64_t i = threadIdx.x; i < row_len; i += 256) m = max(m, __float_as_uint(fabsf(r[i])));   // (non-negative floats order like their bit patterns; NaN / inf end up on top)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, (unsigned int)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = max(max(red[0], red[1]), max(red[2], red[3]));
}

// [Cout][Cin][taps] fp32 -> the packed split-operand layout (split_operand.h); the host passes the layout's channel chunk and taps per k-group
__global__ void pack_conv_weight_bf16x6_kernel(const float* __restrict__ w, uint4* __restrict__ packed, int Cout, int Cin, int taps,
                                                int CK, int TPG) {
    const int CPH = 8 / TPG, NTG = (taps + TPG - 1) / TPG, NCG = CK / (2 * CPH), G = NTG * NCG;
    const int nchunks = (Cin + CK - 1) / CK;
    const int64_t n = (int64_t)nchunks * G * 3 * 2 * Cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % Cout);
        int64_t r = i / Cout;
        const int h = (int)(r & 1);
        r >>= 1;
        const int pl = (int)(r % 3);
        r /= 3;
        const int grp = (int)(r % G);
        const int chunk = (int)(r / G);
        const int cg = grp / NTG, tg = grp % NTG;
        unsigned short v[8];
        for (int j = 0; j < 8; ++j) {
            const int tapi = j / CPH, chl = j % CPH;
            const int tap = tg * TPG + tapi, ci = chunk * CK + cg * 2 * CPH + h * CPH + chl;
            float x = 0.f;
            if (tap < taps && ci < Cin) x = w[((int64_t)co * Cin + ci) * taps + tap];
            v[j] = pack_split_weight<STEMSEG_PRECISION_BF16X6>(x, pl);
        }
        uint4 o;
        o.x = v[0] | ((unsigned)v[1] << 16); o.y = v[2] | ((unsigned)v[3] << 16);
        o.z = v[4] | ((unsigned)v[5] << 16); o.w = v[6] | ((unsigned)v[7] << 16);
        packed[i] = o;
    }
}

// f16x3: the same slab order with the planes of w * S[co]; writes inv[Cout] and reads max_bits[Cout] behind the slabs
__global__ void pack_conv_weight_f16x3_kernel(const float* __restrict__ w, uint4* __restrict__ packed, int Cout, int Cin, int taps,
                                               int CK, int TPG) {
    const int CPH = 8 / TPG, NTG = (taps + TPG - 1) / TPG, NCG = CK / (2 * CPH), G = NTG * NCG;
    const int nchunks = (Cin + CK - 1) / CK;
    constexpr int NPLW = SplitLayout(1, STEMSEG_PRECISION_F16X3).NPL;      // planes: hi, lo
    const int64_t n = (int64_t)nchunks * G * NPLW * 2 * Cout;
    float* inv = reinterpret_cast<float*>(packed + n);
    const unsigned int* max_bits = reinterpret_cast<const unsigned int*>(inv + Cout);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i % Cout);
        const float S = f16x3_weight_scale(max_bits[co]);
        if (i < Cout) inv[co] = 1.0f / (S * F16X3_ACT_SCALE);
        int64_t r = i / Cout;
        const int h = (int)(r & 1);
        r >>= 1;
        const int pl = (int)(r % NPLW);
        r /= NPLW;
        const int grp = (int)(r % G);
        const int chunk = (int)(r / G);
        const int cg = grp / NTG, tg = grp % NTG;
        unsigned short v[8];
        for (int j = 0; j < 8; ++j) {
            const int tapi = j / CPH, chl = j % CPH;
            const int tap = tg * TPG + tapi, ci = chunk * CK + cg * 2 * CPH + h * CPH + chl;
            float x = 0.f;
            if (tap < taps && ci < Cin) x = w[((int64_t)co * Cin + ci) * taps + tap] * S;
            v[j] = pack_split_weight<STEMSEG_PRECISION_F16X3>(x, pl);
        }
        uint4 o;
        o.x = v[0] | ((unsigned)v[1] << 16); o.y = v[2] | ((unsigned)v[3] << 16);
        o.z = v[4] | ((unsigned)v[5] << 16); o.w = v[6] | ((unsigned)v[7] << 16);
        packed[i] = o;
    }
}

static bool split_taps_ok(int32_t taps, int32_t precision) {
    return taps == 27 || taps == 9 || taps == 1 || (taps == 16 && precision == STEMSEG_PRECISION_F16X3);      // (16: the f16x3 stem)
}

}  // namespace stemseg

extern "C" int stemseg_hip_pack_conv_weight(const float* w, float* packed, int32_t Cout, int32_t Cin, int32_t taps, void* stream) {
    using namespace stemseg;
    SS_CHECK_ARG(w && packed, "pack_conv_weight: null pointer");
    SS_CHECK_ARG(Cin % 4 == 0 && Cout % 32 == 0 && taps > 0, "pack_conv_weight: Cin %% 4, Cout %% 32 (got %d, %d)", Cin, Cout);
    const int64_t n = (int64_t)Cout * Cin * taps;
    const int blocks = (int)std::min<int64_t>(ceil_div(n, 256), 4096);
    hipLaunchKernelGGL(pack_conv_weight_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), w, packed, Cout, Cin, taps);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int64_t stemseg_hip_packed_weight_bytes_prec(int32_t Cout, int32_t Cin, int32_t taps, int32_t precision) {
    using namespace stemseg;
    if (Cout <= 0 || Cin <= 0 || !split_taps_ok(taps, precision)) return 0;
    if (precision != STEMSEG_PRECISION_BF16X6 && precision != STEMSEG_PRECISION_F16X3) return 0;
    return SplitLayout(taps, precision).bytes(Cout, Cin);
}

extern "C" int stemseg_hip_pack_conv_weight_prec(const float* w, void* packed, int32_t Cout, int32_t Cin, int32_t taps, int32_t precision, void* stream) {
    using namespace stemseg;
    SS_CHECK_ARG(precision == STEMSEG_PRECISION_BF16X6 || precision == STEMSEG_PRECISION_F16X3, "pack_conv_weight_prec: precision must be 2 (bf16x6) or 3 (f16x3)");
    SS_CHECK_ARG(w && packed, "pack_conv_weight_prec: null pointer");
    SS_CHECK_ARG(split_taps_ok(taps, precision), "pack_conv_weight_prec: taps must be 27, 9 or 1 (16: f16x3, the stem)");
    SS_CHECK_ARG(Cin % 4 == 0 && Cout % 32 == 0, "pack_conv_weight_prec: Cin %% 4, Cout %% 32 (got %d, %d)", Cin, Cout);
    const SplitLayout sl(taps, precision);
    const int64_t n = sl.slab_bytes(Cout, Cin) / 16;
    const int blocks = (int)std::min<int64_t>(ceil_div(n, 256), 4096);
    if (precision == STEMSEG_PRECISION_BF16X6) {
        hipLaunchKernelGGL(pack_conv_weight_bf16x6_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), w, reinterpret_cast<uint4*>(packed), Cout, Cin, taps, sl.CK, sl.TPG);
        SS_LAUNCH_CHECK();
        return STEMSEG_OK;
    }
    unsigned int* max_bits = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(packed) + sl.max_bits_offset(Cout, Cin));
    hipLaunchKernelGGL(absmax_rows_kernel, dim3((unsigned)Cout), dim3(256), 0, as_stream(stream), w, (int64_t)Cin * taps, max_bits);
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(pack_conv_weight_f16x3_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), w, reinterpret_cast<uint4*>(packed), Cout, Cin, taps, sl.CK, sl.TPG);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
