// Backward of the decoders' tails: the 1x1x1 heads (and the per-level matrices of the folded linear tail), the trilinear up-sampling and
// GroupNorm -> ReLU -> (average pool).  Everything behind the last 3x3x3 convolution of a decoder branch; the convolutions themselves
// have no backward here.
//
// Forward counterparts: heads.hip (heads_kernel, level_head_kernel), resample.hip (upsample_trilinear_kernel), norm_pool.hip
// (gn_relu_pool_kernel).  All HBM-bound.  No floating-point atomics anywhere: a sum that crosses workgroups goes through per-workgroup
// fp64 partials in the caller's workspace and one fixed-order combine (the scheme of gn_partial_kernel / gn_finalize_kernel), and every
// partial slot is written by every call, so the workspace needs no initialisation and two runs give the same bits.  No call
// synchronises or allocates.
#include "common.h"
#include <algorithm>

namespace stemseg {

__device__ __forceinline__ double bwd_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// 4 consecutive floats of a row, element 4 q onward: one 16-B access when the row is 16-B aligned (VEC: base aligned and the row stride a
// multiple of 4), else bounds-checked scalars (zeros past the end, stores dropped there)
template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* row, int64_t q, int64_t n) {
    if (VEC) return reinterpret_cast<const float4*>(row)[q];
    const int64_t v = q * 4;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (v < n) r.x = row[v];
    if (v + 1 < n) r.y = row[v + 1];
    if (v + 2 < n) r.z = row[v + 2];
    if (v + 3 < n) r.w = row[v + 3];
    return r;
}
template <bool VEC>
__device__ __forceinline__ void st4(float* row, int64_t q, int64_t n, const float4 val) {
    if (VEC) { reinterpret_cast<float4*>(row)[q] = val; return; }
    const int64_t v = q * 4;
    if (v < n) row[v] = val.x;
    if (v + 1 < n) row[v + 1] = val.y;
    if (v + 2 < n) row[v + 2] = val.z;
    if (v + 3 < n) row[v + 3] = val.w;
}
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ================================================================================================ heads
// dz = d_out * act'(z), the derivative recovered from the forward OUTPUT (heads.hip head_act): identity (+ grid) 1; tanh(0.25 z) + grid
// 0.25 (1 - tanh^2) with tanh = out - grid; sigmoid out (1 - out); exp(z) * 10 out.
struct HeadsDzParams {
    const float* out;
    const float* d_out;
    float* dz;
    const float* gt;
    const float* gy;
    const float* gx;
    int T, H, W, n_out;
    int64_t V, nq;
    int act[STEMSEG_MAX_HEAD_OUT];
    int axis[STEMSEG_MAX_HEAD_OUT];
};

template <bool VEC>
__global__ __launch_bounds__(256) void heads_dz_kernel(HeadsDzParams p) {
    const int o = blockIdx.y;
    const int act = p.act[o], ax = p.axis[o];
    const float* yo = p.out + (int64_t)o * p.V;
    const float* go = p.d_out + (int64_t)o * p.V;
    float* zo = p.dz + (int64_t)o * p.V;
    const int64_t HW = (int64_t)p.H * p.W;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < p.nq; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 g4 = ld4<VEC>(go, q, p.V);
        if (act == 0 || act == 4) { st4<VEC>(zo, q, p.V, g4); continue; }
        const float4 y4 = ld4<VEC>(yo, q, p.V);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w}, y[4] = {y4.x, y4.y, y4.z, y4.w};
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (act == 2) r[j] = g[j] * (y[j] * (1.f - y[j]));
            else if (act == 3) r[j] = g[j] * y[j];
            else {
                float grid = 0.f;
                const int64_t v = q * 4 + j;
                if (ax != 0 && v < p.V) {
                    const int t = (int)(v / HW);
                    const int64_t rem = v - (int64_t)t * HW;
                    const int yy = (int)(rem / p.W);
                    grid = ax == 1 ? p.gt[t] : (ax == 2 ? p.gy[yy] : p.gx[(int)(rem - (int64_t)yy * p.W)]);
                }
                const float th = y[j] - grid;
                r[j] = g[j] * (0.25f * (1.f - th * th));
            }
        }
        st4<VEC>(zo, q, p.V, make_float4(r[0], r[1], r[2], r[3]));
    }
}

// The two products of the backward in one read of x:  dx[c][v] = sum_o w[o][c] dz[o][v]  and the partials of  dw[o][c] = sum_v dz[o][v] x[c][v],
// db[o] = sum_v dz[o][v].  grid = (voxel chunks, ceil(Cin / 32)); a workgroup owns 32 input channels, wave k eight of them, over one chunk of
// voxels; a lane takes 4 consecutive voxels per step (16-B loads along x) and keeps NOUT x 8 fp32 accumulators over its handful of steps.
// The waves of a workgroup read the same dz rows (n_out of them, against Cin of x: they stay in cache).  At the end of the chunk every
// accumulator is summed over the wave in fp64 and lane 0 writes the slot part[chunk][o][c] (c == Cin: the bias slot).
constexpr int HB_CPW = 8;             // channels per wave
constexpr int HB_CPB = 4 * HB_CPW;    // channels per workgroup
constexpr int HB_MAX_CHUNKS = 256;

struct HeadsBwdParams {
    const float* x;
    const float* w;
    const float* dz;
    float* dx;
    double* part;
    int Cin;
    int64_t V, nq, qpc;               // voxels, 4-voxel steps, steps per chunk
};

template <int NOUT, bool VEC>
__global__ __launch_bounds__(256) void heads_bwd_kernel(HeadsBwdParams p) {
    __shared__ float w_lds[NOUT][HB_CPB];
    const int c_blk = blockIdx.y * HB_CPB;
    for (int i = threadIdx.x; i < NOUT * HB_CPB; i += 256) {
        const int o = i / HB_CPB, k = i - o * HB_CPB;
        w_lds[o][k] = c_blk + k < p.Cin ? p.w[(int64_t)o * p.Cin + c_blk + k] : 0.f;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c0 = c_blk + wave * HB_CPW;
    const int64_t qb = (int64_t)blockIdx.x * p.qpc, qe = qb + p.qpc < p.nq ? qb + p.qpc : p.nq;
    const bool do_b = blockIdx.y == 0 && wave == 0;
    float acc[NOUT][HB_CPW], accb[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
        accb[o] = 0.f;
#pragma unroll
        for (int k = 0; k < HB_CPW; ++k) acc[o][k] = 0.f;
    }
    if (c0 < p.Cin) {                                        // (wave-uniform)
        for (int64_t q = qb + lane; q < qe; q += 64) {
            float4 dz[NOUT];
#pragma unroll
            for (int o = 0; o < NOUT; ++o) dz[o] = ld4<VEC>(p.dz + (int64_t)o * p.V, q, p.V);
            if (do_b) {
#pragma unroll
                for (int o = 0; o < NOUT; ++o) accb[o] += (dz[o].x + dz[o].y) + (dz[o].z + dz[o].w);
            }
#pragma unroll
            for (int k = 0; k < HB_CPW; ++k) {
                const int c = c0 + k;
                if (c >= p.Cin) continue;                    // (Cin % 4 == 0: the last wave's tile may be half full)
                const float4 xv = ld4<VEC>(p.x + (int64_t)c * p.V, q, p.V);
                float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int o = 0; o < NOUT; ++o) {
                    acc[o][k] += (dz[o].x * xv.x + dz[o].y * xv.y) + (dz[o].z * xv.z + dz[o].w * xv.w);
                    const float wv = w_lds[o][wave * HB_CPW + k];
                    d.x += wv * dz[o].x; d.y += wv * dz[o].y; d.z += wv * dz[o].z; d.w += wv * dz[o].w;
                }
                if (p.dx) st4<VEC>(p.dx + (int64_t)c * p.V, q, p.V, d);
            }
        }
    }
    double* pr = p.part + (int64_t)blockIdx.x * NOUT * (p.Cin + 1);
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
#pragma unroll
        for (int k = 0; k < HB_CPW; ++k) {
            const double s = bwd_wave_sum((double)acc[o][k]);
            if (lane == 0 && c0 + k < p.Cin) pr[(int64_t)o * (p.Cin + 1) + c0 + k] = s;
        }
        if (do_b) {
            const double s = bwd_wave_sum((double)accb[o]);
            if (lane == 0) pr[(int64_t)o * (p.Cin + 1) + p.Cin] = s;
        }
    }
}

// one thread per (o, c) slot: the chunks' partials in chunk order -> dw / db
__global__ __launch_bounds__(256) void heads_bwd_combine_kernel(const double* __restrict__ part, int nchunks, int n_out, int Cin,
                                                                float* __restrict__ dw, float* __restrict__ db) {
    const int n = n_out * (Cin + 1);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < nchunks; ++k) s += part[(int64_t)k * n + i];
    const int o = i / (Cin + 1), c = i - o * (Cin + 1);
    if (c < Cin) dw[(int64_t)o * Cin + c] = (float)s;
    else if (db) db[o] = (float)s;
}

struct HeadsBwdPlan {
    int64_t nq, qpc, dz_floats;
    int nchunks;
    size_t bytes;
};
static int heads_bwd_plan(int Cin, int n_out, int64_t V, HeadsBwdPlan& pl) {
    SS_CHECK_ARG(n_out >= 1 && n_out <= STEMSEG_MAX_HEAD_OUT, "heads_backward: n_out=%d unsupported (1..%d)", n_out, STEMSEG_MAX_HEAD_OUT);
    SS_CHECK_ARG(Cin > 0 && Cin % 4 == 0 && Cin <= 512, "heads_backward: Cin %% 4 == 0 and Cin <= 512 required (Cin=%d)", Cin);
    SS_CHECK_ARG(V > 0 && V < (1ll << 40), "heads_backward: bad voxel count");
    pl.nq = ceil_div(V, 4);
    pl.qpc = round_up(ceil_div(pl.nq, HB_MAX_CHUNKS), 64);
    pl.nchunks = (int)ceil_div(pl.nq, pl.qpc);
    pl.dz_floats = round_up((int64_t)n_out * V, 64);         // (the partials behind it stay 256-B aligned)
    pl.bytes = (size_t)pl.dz_floats * sizeof(float) + (size_t)pl.nchunks * n_out * (Cin + 1) * sizeof(double);
    return STEMSEG_OK;
}

template <int NOUT>
static void launch_heads_bwd_n(const HeadsBwdParams& p, int nchunks, bool vec, hipStream_t s) {
    const dim3 grid((unsigned)nchunks, (unsigned)ceil_div(p.Cin, HB_CPB));
    if (vec) hipLaunchKernelGGL((heads_bwd_kernel<NOUT, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((heads_bwd_kernel<NOUT, false>), grid, dim3(256), 0, s, p);
}

// ================================================================================================ wide linear heads (n_out 11 .. 64)
// The same three products for a head too wide for NOUT x 8 VALU accumulators (the 42-channel YouTube-VIS semseg head), on v_mfma_f32_32x32x2_f32:
// exact products, fp32 accumulation, the library's "f32" arithmetic.  Lane l of an MFMA holds A[row l & 31][k = l >> 5] and B[k = l >> 5][col l & 31];
// register r of the result is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.  w is the plain dense [n_out][Cin] matrix of the narrow kernels,
// read through LDS; the rows n_out .. of the last 32-row block are zeros written into LDS, never read from memory.  No activation table: a wide
// head is raw class logits.
typedef float wh_f32x16 __attribute__((ext_vector_type(16)));
constexpr int WH_TV = 32;                 // voxels per tile: one MFMA block along v
constexpr int WH_STRIDE = WH_TV + 1;      // odd LDS row stride: the 32 lanes of a half wave read 32 rows at one voxel
constexpr int WH_CB = 128;                // backward: input channels per workgroup, wave k the 32 from 32 k
constexpr int WH_KC = 64;                 // forward: input channels per staged slab of w
constexpr int WH_FLUSH = 16;              // backward: voxels whose dw products are summed in fp32 before they move to fp64 (conv_backward.hip's 1-tap rule)
constexpr int WH_MAX_CHUNKS = 256;
constexpr int WH_FWD_MAX_BLOCKS = 16384;

__device__ __forceinline__ int wh_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

struct WideFwdParams {
    const float* x;
    const float* w;
    const float* add;
    float* out;
    int Cin, n_out;
    int64_t V, ngroups;                   // voxels, groups of 128 NT voxels (32 NT per wave, NT = 4 / MB)
};

// Forward  out[o][v] = sum_c w[o][c] x[c][v] (+ add[o][v]):  M = o (MB blocks of 32), N = v, K = c.  A wave owns 32 NT consecutive voxels as NT
// tiles of 32, NT = 4 / MB (64 accumulator registers either way): lane column j holds voxels NT j .. NT j + NT - 1 and tile t is the voxels
// NT j + t -- the columns of a product are independent, so a tile may be any 32 voxels -- which makes the lane's B operands of its tiles one 16-B
// (8-B for MB = 2) load of x[c] (VEC: V % 4 == 0 and 16-B aligned maps; else scalar loads at clamped addresses) and its results one such
// store per output row.  The loads of a batch of FB k-steps are issued ahead of the previous batch's MFMAs.  A is a slab of WH_KC columns of w, staged transposed
// ([c][o], odd stride: staging and operand reads are both conflict-free) in one of two LDS buffers while the other is read -- the next slab's
// loads are in flight during the MFMAs, one barrier per slab.
template <int MB, bool VEC>
__global__ __launch_bounds__(256, VEC ? 2 : 1) void wide_level_head_kernel(WideFwdParams p) {
    constexpr int WS = MB * 32 + 1, NW = WH_KC * MB * 32 / 256, NT = 4 / MB;
    constexpr int FB = VEC && MB == 1 ? 8 : 4;                                      // k-steps (pairs of channels) per batch of loads
    typedef float vecn __attribute__((ext_vector_type(NT)));
    __shared__ float w_lds[2][WH_KC * WS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
    float wr[NW];
    auto load_w = [&](int kc) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = threadIdx.x + 256 * i, c = idx & (WH_KC - 1), o = idx / WH_KC;
            wr[i] = (o < p.n_out && kc + c < p.Cin) ? p.w[(int64_t)o * p.Cin + kc + c] : 0.f;
        }
    };
    int buf = 0;
    load_w(0);
    for (int64_t g = blockIdx.x; g < p.ngroups; g += gridDim.x) {
        const int64_t v0 = (g * 4 + wave) * (NT * WH_TV) + NT * col;     // this lane's voxels: v0 + t
        int64_t vc[NT];                                                  // (a voxel past the end: the last one is read, nothing is stored)
#pragma unroll
        for (int t = 0; t < NT; ++t) vc[t] = v0 + t < p.V ? v0 + t : p.V - 1;
        const int64_t vq = v0 < p.V ? v0 : p.V - NT;                     // (VEC: V % 4 == 0, so v0 < V means v0 + NT - 1 < V, and V - NT is aligned)
        float bx[2][FB][NT];
        auto load_b = [&](int cb, float (&b)[FB][NT]) {                  // channels cb .. cb + 2 FB - 1 (no branch around a load: a clamped address, then a select)
#pragma unroll
            for (int s = 0; s < FB; ++s) {
                const int c = cb + 2 * s + half;
                const float* row = p.x + (int64_t)(c < p.Cin ? c : p.Cin - 1) * p.V;
                const bool on = c < p.Cin;
                if (VEC) {
                    const vecn q = *reinterpret_cast<const vecn*>(row + vq);
#pragma unroll
                    for (int t = 0; t < NT; ++t) b[s][t] = on ? q[t] : 0.f;
                } else {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const float q = row[vc[t]];
                        b[s][t] = on ? q : 0.f;
                    }
                }
            }
        };
        load_b(0, bx[0]);
        wh_f32x16 acc[NT][MB];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][mb][r] = 0.f;
        for (int kc = 0; kc < p.Cin; kc += WH_KC) {
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const int idx = threadIdx.x + 256 * i;
                w_lds[buf][(idx & (WH_KC - 1)) * WS + idx / WH_KC] = wr[i];
            }
            __syncthreads();                                             // (the other buffer was last read before the previous barrier)
            const int kn = kc + WH_KC < p.Cin ? kc + WH_KC : 0;          // the next slab: of this group, or the first of the next group
            if (kn || g + gridDim.x < p.ngroups) load_w(kn);
            const float* wl = w_lds[buf];
#pragma unroll
            for (int h = 0; h < WH_KC; h += 2 * FB) {                    // (a slab that ends at Cin: zero columns of w against zeros for x)
                constexpr int NB = WH_KC / (2 * FB);                     // (even: the batch in h / (2 FB) & 1 is a compile-time choice)
                const int cur = (h / (2 * FB)) & 1;
                if (kc + h + 2 * FB < p.Cin) load_b(kc + h + 2 * FB, bx[cur ^ 1]);       // the next batch, of this slab or the next, ahead of these MFMAs
                static_assert(NB % 2 == 0, "batches per slab");
                if (kc + h < p.Cin) {                                    // (uniform; a batch wholly past Cin was never loaded)
#pragma unroll
                    for (int s = 0; s < FB; ++s)
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) {
                            const float a = wl[(h + 2 * s + half) * WS + mb * 32 + col];
#pragma unroll
                            for (int t = 0; t < NT; ++t) acc[t][mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bx[cur][s][t], acc[t][mb], 0, 0, 0);
                        }
                }
                __builtin_amdgcn_sched_barrier(0);                       // (the batch after the next stays behind these MFMAs: the registers of two batches)
            }
            buf ^= 1;
        }
        if (v0 >= p.V) continue;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = mb * 32 + wh_row(r, half);
                if (o >= p.n_out) continue;
                float* orow = p.out + (int64_t)o * p.V;
                if (VEC) {
                    vecn val;
#pragma unroll
                    for (int t = 0; t < NT; ++t) val[t] = acc[t][mb][r];
                    if (p.add) val += *reinterpret_cast<const vecn*>(p.add + (int64_t)o * p.V + v0);
                    *reinterpret_cast<vecn*>(orow + v0) = val;
                } else {
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (v0 + t < p.V) orow[v0 + t] = p.add ? acc[t][mb][r] + p.add[(int64_t)o * p.V + v0 + t] : acc[t][mb][r];
                }
            }
    }
}

struct WideBwdParams {
    const float* x;
    const float* w;
    const float* dz;
    float* dx;
    double* part;
    int Cin, n_out;
    int64_t V, ntiles, tpc;               // voxels, 32-voxel tiles, tiles per chunk
};

// Backward, grid = (voxel chunks, ceil(Cin / 128)): a workgroup owns 128 input channels (wave k: 32) over one chunk of tiles and reads x once; the
// dz rows are read by every channel block (n_out of them against Cin of x: they stay in cache).  Per tile, x [128][32] and dz [32 MB][32] are
// staged in LDS once (the next tile's loads are in flight meanwhile) and read in both orientations:
//     dx[c][v] = sum_o w[o][c] dz[o][v]     M = c, N = v, K = o     A = w_lds[o][c on the lane],  B = dz_lds[o][v on the lane]
//     dw[o][c] = sum_v dz[o][v] x[c][v]     M = o, N = c, K = v     A = dz_lds[o on the lane][v], B = x_lds[c on the lane][v]
// The fp32 sums of dw cover WH_FLUSH voxels (a 16-voxel chain) and are then added to fp64 registers, as conv_backward.hip's 1-tap kernel does; at the
// end of the chunk they are the slots part[chunk][o][c].  db: the thread that stages dz[o][v] sums it, 32 lanes per row, the slot c == Cin.
template <int MB>
__global__ __launch_bounds__(256, 2) void wide_heads_bwd_kernel(WideBwdParams p) {
    __shared__ float x_lds[WH_CB * WH_STRIDE];
    __shared__ float dz_lds[MB * 32 * WH_STRIDE];
    __shared__ float w_lds[MB * 32 * WH_CB];
    const int c_blk = blockIdx.y * WH_CB;
    for (int i = threadIdx.x; i < MB * 32 * WH_CB; i += 256) {
        const int c = i & (WH_CB - 1), o = i / WH_CB;
        w_lds[i] = (o < p.n_out && c_blk + c < p.Cin) ? p.w[(int64_t)o * p.Cin + c_blk + c] : 0.f;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
    const int sv = threadIdx.x & 31, sr = threadIdx.x >> 5;              // staging: voxel of the tile, first row (then every 8th)
    const int c0 = c_blk + wave * 32;
    const bool wave_on = c0 < p.Cin;                                     // (Cin % 4 == 0: the last channel block may end early)
    const int ko = (p.n_out + 1) & ~1;                                   // (an odd n_out: row n_out is a zero row of both LDS images)
    const int64_t t0 = (int64_t)blockIdx.x * p.tpc, t1 = t0 + p.tpc < p.ntiles ? t0 + p.tpc : p.ntiles;
    float xr[WH_CB / 8], zr[MB * 4], accb[MB * 4];
    double dacc[MB][16];
#pragma unroll
    for (int i = 0; i < MB * 4; ++i) accb[i] = 0.f;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[mb][r] = 0.0;
    auto load_tile = [&](int64_t t) {
        const int64_t v = t * WH_TV + sv;
        const bool ok = v < p.V;
#pragma unroll
        for (int i = 0; i < WH_CB / 8; ++i) {
            const int c = c_blk + sr + 8 * i;
            xr[i] = (ok && c < p.Cin) ? p.x[(int64_t)c * p.V + v] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < MB * 4; ++i) {
            const int o = sr + 8 * i;
            zr[i] = (ok && o < p.n_out) ? p.dz[(int64_t)o * p.V + v] : 0.f;
        }
    };
    load_tile(t0);
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();                                                 // (the previous tile is read; first pass: w_lds is staged)
#pragma unroll
        for (int i = 0; i < WH_CB / 8; ++i) x_lds[(sr + 8 * i) * WH_STRIDE + sv] = xr[i];
#pragma unroll
        for (int i = 0; i < MB * 4; ++i) {
            dz_lds[(sr + 8 * i) * WH_STRIDE + sv] = zr[i];
            accb[i] += zr[i];
        }
        __syncthreads();
        if (t + 1 < t1) load_tile(t + 1);
        if (!wave_on) continue;                                          // (wave-uniform; the wave still stages and meets the barriers)
        if (p.dx) {
            wh_f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            for (int k = 0; k < ko; k += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w_lds[(k + half) * WH_CB + wave * 32 + col], dz_lds[(k + half) * WH_STRIDE + col], acc, 0, 0, 0);
            const int64_t v = t * WH_TV + col;
            if (v < p.V) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = c0 + wh_row(r, half);
                    if (c < p.Cin) p.dx[(int64_t)c * p.V + v] = acc[r];
                }
            }
        }
        for (int k0 = 0; k0 < WH_TV; k0 += WH_FLUSH) {                   // (no fp32 chain of dw longer than WH_FLUSH voxels)
            wh_f32x16 aw[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) aw[mb][r] = 0.f;
#pragma unroll
            for (int k = k0; k < k0 + WH_FLUSH; k += 2) {
                const float b = x_lds[(wave * 32 + col) * WH_STRIDE + k + half];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
                    aw[mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(dz_lds[(mb * 32 + col) * WH_STRIDE + k + half], b, aw[mb], 0, 0, 0);
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int r = 0; r < 16; ++r) dacc[mb][r] += (double)aw[mb][r];
        }
    }
    const int64_t n = (int64_t)p.n_out * (p.Cin + 1);
    double* pr = p.part + (int64_t)blockIdx.x * n;
    if (wave_on && c0 + col < p.Cin) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = mb * 32 + wh_row(r, half);
                if (o < p.n_out) pr[(int64_t)o * (p.Cin + 1) + c0 + col] = dacc[mb][r];
            }
    }
    if (blockIdx.y == 0) {
#pragma unroll
        for (int i = 0; i < MB * 4; ++i) {
            double s = (double)accb[i];
#pragma unroll
            for (int m = 16; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);  // (the 32 lanes that staged this row)
            const int o = sr + 8 * i;
            if (sv == 0 && o < p.n_out) pr[(int64_t)o * (p.Cin + 1) + p.Cin] = s;
        }
    }
}

struct WidePlan {
    int64_t ntiles, tpc;
    int nchunks;
    size_t bytes;
};
static int wide_plan(const char* who, int Cin, int n_out, int64_t V, WidePlan& pl) {
    SS_CHECK_ARG(n_out > STEMSEG_MAX_HEAD_OUT && n_out <= STEMSEG_MAX_WIDE_HEAD_OUT, "%s: n_out=%d unsupported (%d..%d; narrower heads: the fused heads' entry points)",
                 who, n_out, STEMSEG_MAX_HEAD_OUT + 1, STEMSEG_MAX_WIDE_HEAD_OUT);
    SS_CHECK_ARG(Cin > 0 && Cin % 4 == 0 && Cin <= 512, "%s: Cin %% 4 == 0 and Cin <= 512 required (Cin=%d)", who, Cin);
    SS_CHECK_ARG(V > 0 && V < (1ll << 40), "%s: bad voxel count V=%lld (0 < V < 2^40)", who, (long long)V);
    pl.ntiles = ceil_div(V, WH_TV);
    pl.tpc = ceil_div(pl.ntiles, WH_MAX_CHUNKS);                         // a function of the shape only
    pl.nchunks = (int)ceil_div(pl.ntiles, pl.tpc);
    pl.bytes = (size_t)pl.nchunks * n_out * (Cin + 1) * sizeof(double);
    return STEMSEG_OK;
}

// ================================================================================================ trilinear adjoint
// resample.hip's src_index: ATen's area_pixel_compute_source_index(align_corners = false), scale 1 a copy
__device__ __forceinline__ void up_src_index(int dst, float rscale, int n, int& i0, int& i1, float& w1) {
    float src = __fsub_rn(__fmul_rn(rscale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 + ((i0 < n - 1 && rscale != 1.f) ? 1 : 0);
    w1 = __fsub_rn(src, (float)i0);
}

// Input index i of an axis up-sampled by S is read by the outputs  S i - S/2 + k,  k = 0 .. NT - 1  (NT = 2 S; 1 for S = 1): the ones whose
// i0 or i1 is i, the border clamps included (outputs below S/2 clamp their source to 0, outputs of the last input have i1 = i0).  wk[k] is
// the weight the forward gave input i in output k -- (1 - w1) as i0, w1 as i1, both when the two coincide -- and 0 for a k outside the map.
// The weights are multiples of 1/8, so their products are exact.
template <int S>
__device__ __forceinline__ void up_taps(int i, float rscale, int n, float* wk) {
    constexpr int NT = S == 1 ? 1 : 2 * S;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int o = S * i - S / 2 + k;
        float wgt = 0.f;
        if (o >= 0 && o < n * S) {
            int i0, i1;
            float w1;
            up_src_index(o, rscale, n, i0, i1, w1);
            if (i0 == i) wgt += __fsub_rn(1.f, w1);
            if (i1 == i) wgt += w1;
        }
        wk[k] = wgt;
    }
}

struct UpBwdParams {
    const float* d_out;
    float* d_in;
    int C, T, H, W;
    float rt, rs;                      // 1 / scale (t; y and x)
};

// Gather form: one thread per INPUT voxel, x fastest; its (at most) 4 x 2S x 2S outputs in fixed order t, y, x, summed in fp64 and rounded
// once.  VEC (d_out 16-B aligned; output rows are 4 W or 2 W floats, the window starts at S x - S / 2): the middle S taps are one aligned
// 16-B (S = 4) or 8-B (S = 2) load and for S = 4 so are the two flanks; else scalar loads, coalesced across the lanes all the same.
template <int ST, int S, bool VEC>
__global__ __launch_bounds__(256) void upsample_bwd_kernel(UpBwdParams p) {
    constexpr int NTT = ST == 1 ? 1 : 2 * ST, NS = 2 * S;
    const int To = p.T * ST, Ho = p.H * S, Wo = p.W * S;
    const int64_t HW = (int64_t)p.H * p.W, per_c = (int64_t)p.T * HW, total = per_c * p.C;
    const int64_t HWo = (int64_t)Ho * Wo;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i / per_c);
        int64_t r = i - (int64_t)c * per_c;
        const int t = (int)(r / HW);
        r -= (int64_t)t * HW;
        const int y = (int)(r / p.W), x = (int)(r - (int64_t)y * p.W);
        float wt[NTT], wy[NS], wx[NS];
        up_taps<ST>(t, p.rt, p.T, wt);
        up_taps<S>(y, p.rs, p.H, wy);
        up_taps<S>(x, p.rs, p.W, wx);
        const float* gc = p.d_out + (int64_t)c * To * HWo;
        const int xo0 = S * x - S / 2;
        double acc = 0.0;
#pragma unroll
        for (int kt = 0; kt < NTT; ++kt) {
            const int to = ST * t - ST / 2 + kt;
            if (to < 0 || to >= To) continue;
#pragma unroll
            for (int ky = 0; ky < NS; ++ky) {
                const int yo = S * y - S / 2 + ky;
                if (yo < 0 || yo >= Ho) continue;
                const float wty = wt[kt] * wy[ky];
                const float* row = gc + (int64_t)to * HWo + (int64_t)yo * Wo;
                float v[NS];
                if constexpr (VEC && S == 4) {
                    const float2 l = x > 0 ? *reinterpret_cast<const float2*>(row + xo0) : make_float2(0.f, 0.f);
                    const float4 m = *reinterpret_cast<const float4*>(row + xo0 + 2);
                    const float2 rr = x + 1 < p.W ? *reinterpret_cast<const float2*>(row + xo0 + 6) : make_float2(0.f, 0.f);
                    v[0] = l.x; v[1] = l.y; v[2] = m.x; v[3] = m.y; v[4] = m.z; v[5] = m.w; v[6] = rr.x; v[7] = rr.y;
                } else if constexpr (VEC && S == 2) {
                    const float2 m = *reinterpret_cast<const float2*>(row + xo0 + 1);
                    v[0] = x > 0 ? row[xo0] : 0.f; v[1] = m.x; v[2] = m.y; v[3] = x + 1 < p.W ? row[xo0 + 3] : 0.f;
                } else {
#pragma unroll
                    for (int kx = 0; kx < NS; ++kx) v[kx] = (xo0 + kx >= 0 && xo0 + kx < Wo) ? row[xo0 + kx] : 0.f;
                }
#pragma unroll
                for (int kx = 0; kx < NS; ++kx) acc += (double)(wty * wx[kx]) * (double)v[kx];
            }
        }
        p.d_in[i] = (float)acc;
    }
}

template <int ST, int S>
static void launch_up_bwd(const UpBwdParams& p, bool vec, hipStream_t s) {
    const int64_t total = (int64_t)p.C * p.T * p.H * p.W;
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(total, 256), 256 * 16);
    if (vec) hipLaunchKernelGGL((upsample_bwd_kernel<ST, S, true>), dim3(blocks), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((upsample_bwd_kernel<ST, S, false>), dim3(blocks), dim3(256), 0, s, p);
}

// ================================================================================================ GroupNorm + ReLU + pool
struct GnBwdParams {
    const float* x;
    const float* stats;
    const float* gamma;
    const float* beta;
    const float* d_out;
    float* dx;
    double* part;                      // [C][split][2]: sum dy, sum dy xhat
    double* coef;                      // [groups][2]: mean_g(gamma dy), mean_g(gamma dy xhat)
    int C, T, H, W, To, cpg, groups, pool, split;
};

// the adjoint of AvgPool3d(3, stride (2, 1, 1), padding 1, / 27 always) at input voxel (t, y, x): the sum over the pooled outputs whose
// window holds it -- planes t >> 1 .. (t + 1) >> 1 (one for an even t, two for an odd one), rows y - 1 .. y + 1, columns x - 1 .. x + 1,
// inside the map -- in that order, in fp64, / 27
__device__ __forceinline__ float pool_adjoint(const float* gc, int t, int y, int x, int To, int H, int W) {
    const int t_hi = min((t + 1) >> 1, To - 1);
    double acc = 0.0;
    for (int to = t >> 1; to <= t_hi; ++to)
        for (int yy = max(y - 1, 0); yy <= min(y + 1, H - 1); ++yy) {
            const float* row = gc + ((int64_t)to * H + yy) * W;
            for (int xx = max(x - 1, 0); xx <= min(x + 1, W - 1); ++xx) acc += (double)row[xx];
        }
    return (float)(acc * (1.0 / 27.0));
}
// ... of 4 consecutive voxels of one row (W % 4 == 0, x0 % 4 == 0): per pooled row one aligned 16-B load and the two neighbours
__device__ __forceinline__ float4 pool_adjoint4(const float* gc, int t, int y, int x0, int To, int H, int W) {
    const int t_hi = min((t + 1) >> 1, To - 1);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int to = t >> 1; to <= t_hi; ++to)
        for (int yy = max(y - 1, 0); yy <= min(y + 1, H - 1); ++yy) {
            const float* row = gc + ((int64_t)to * H + yy) * W;
            const float4 m = *reinterpret_cast<const float4*>(row + x0);
            const float l = x0 > 0 ? row[x0 - 1] : 0.f, r = x0 + 4 < W ? row[x0 + 4] : 0.f;
            a0 += ((double)l + (double)m.x) + (double)m.y;
            a1 += ((double)m.x + (double)m.y) + (double)m.z;
            a2 += ((double)m.y + (double)m.z) + (double)m.w;
            a3 += ((double)m.z + (double)m.w) + (double)r;
        }
    const double k = 1.0 / 27.0;
    return make_float4((float)(a0 * k), (float)(a1 * k), (float)(a2 * k), (float)(a3 * k));
}

// Pass 1, grid = (split, C): dy = pool^T(d_out) [y > 0] into dx, with y the forward's own expression relu(fma(x, rstd gamma, beta - mean rstd
// gamma)) (gn_relu_pool_kernel: the same bits decide the mask; a NaN y passes no gradient, as in torch), and the workgroup's fp64 partials
// of sum dy and sum dy xhat, xhat = (x - mean) rstd.
template <bool VEC>
__global__ __launch_bounds__(256) void gn_bwd_dy_kernel(GnBwdParams p) {
    const int c = blockIdx.y, sp = blockIdx.x;
    float a = 1.f, b = 0.f, mean = 0.f, rstd = 1.f;
    if (p.groups > 0) {
        const int g = c / p.cpg;
        mean = p.stats[2 * g]; rstd = p.stats[2 * g + 1];
        a = rstd * p.gamma[c];
        b = p.beta[c] - mean * a;
    }
    const int64_t HW = (int64_t)p.H * p.W, S = (int64_t)p.T * HW;
    const int64_t per = ((S + p.split - 1) / p.split + 3) & ~int64_t(3);
    const int64_t beg = (int64_t)sp * per, end = beg + per < S ? beg + per : S;
    const float* xc = p.x + (int64_t)c * S;
    const float* gc = p.d_out + (int64_t)c * p.To * HW;
    float* dc = p.dx + (int64_t)c * S;
    double s1 = 0.0, s2 = 0.0;
    auto one = [&](float xv, float g) {
        const float dy = fmaf(xv, a, b) > 0.f ? g : 0.f;
        s1 += (double)dy;
        s2 += (double)dy * (double)((xv - mean) * rstd);
        return dy;
    };
    if (VEC) {                                               // W % 4 == 0: 4 voxels of one row per step
        for (int64_t v = beg + 4 * (int64_t)threadIdx.x; v < end; v += 4 * 256) {
            const float4 xv = *reinterpret_cast<const float4*>(xc + v);
            float4 g4;
            if (p.pool) {
                const int t = (int)(v / HW);
                const int64_t r = v - (int64_t)t * HW;
                const int y = (int)(r / p.W);
                g4 = pool_adjoint4(gc, t, y, (int)(r - (int64_t)y * p.W), p.To, p.H, p.W);
            } else g4 = *reinterpret_cast<const float4*>(gc + v);
            float4 d;
            d.x = one(xv.x, g4.x); d.y = one(xv.y, g4.y); d.z = one(xv.z, g4.z); d.w = one(xv.w, g4.w);
            *reinterpret_cast<float4*>(dc + v) = d;
        }
    } else {
        for (int64_t v = beg + threadIdx.x; v < end; v += 256) {
            float g;
            if (p.pool) {
                const int t = (int)(v / HW);
                const int64_t r = v - (int64_t)t * HW;
                const int y = (int)(r / p.W);
                g = pool_adjoint(gc, t, y, (int)(r - (int64_t)y * p.W), p.To, p.H, p.W);
            } else g = gc[v];
            dc[v] = one(xc[v], g);
        }
    }
    if (p.groups == 0) return;                               // 'none' normalisation: dx = dy, no parameter gradients (uniform exit)
    __shared__ double red[2][4];
    s1 = bwd_wave_sum(s1);
    s2 = bwd_wave_sum(s2);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[0][w] = s1; red[1][w] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* pr = p.part + ((int64_t)c * p.split + sp) * 2;
        pr[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        pr[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// one wave per group: a lane sums its channels' split partials in split order -> dbeta, dgamma; the group's gamma-weighted sums over the
// wave -> the two means of the apply pass
__global__ __launch_bounds__(64) void gn_bwd_finalize_kernel(GnBwdParams p, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int g = blockIdx.x;
    double A = 0.0, B = 0.0;
    for (int k = threadIdx.x; k < p.cpg; k += 64) {
        const int c = g * p.cpg + k;
        const double* pr = p.part + (int64_t)c * p.split * 2;
        double s1 = 0.0, s2 = 0.0;
        for (int sp = 0; sp < p.split; ++sp) { s1 += pr[2 * sp]; s2 += pr[2 * sp + 1]; }
        dbeta[c] = (float)s1;
        dgamma[c] = (float)s2;
        A += (double)p.gamma[c] * s1;
        B += (double)p.gamma[c] * s2;
    }
    A = bwd_wave_sum(A);
    B = bwd_wave_sum(B);
    if (threadIdx.x == 0) {
        const double n = (double)p.cpg * (double)p.T * (double)p.H * (double)p.W;
        p.coef[2 * g] = A / n;
        p.coef[2 * g + 1] = B / n;
    }
}

// Pass 2, grid = (blocks, C), in place over the dy of pass 1:  dx = rstd (gamma dy - mean_g(gamma dy) - xhat mean_g(gamma dy xhat))
template <bool VEC>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(GnBwdParams p) {
    const int c = blockIdx.y, g = c / p.cpg;
    const float mean = p.stats[2 * g], rstd = p.stats[2 * g + 1], gam = p.gamma[c];
    const float A = (float)p.coef[2 * g], B = (float)p.coef[2 * g + 1];
    const int64_t S = (int64_t)p.T * p.H * p.W;
    const float* xc = p.x + (int64_t)c * S;
    float* dc = p.dx + (int64_t)c * S;
    auto one = [&](float xv, float dy) { return rstd * ((gam * dy - A) - ((xv - mean) * rstd) * B); };
    if (VEC) {
        for (int64_t v = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x); v < S; v += 4 * 256 * (int64_t)gridDim.x) {
            const float4 xv = *reinterpret_cast<const float4*>(xc + v);
            float4 d = *reinterpret_cast<const float4*>(dc + v);
            d.x = one(xv.x, d.x); d.y = one(xv.y, d.y); d.z = one(xv.z, d.z); d.w = one(xv.w, d.w);
            *reinterpret_cast<float4*>(dc + v) = d;
        }
    } else {
        for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < S; v += 256 * (int64_t)gridDim.x) dc[v] = one(xc[v], dc[v]);
    }
}

struct GnBwdPlan {
    int split;
    size_t bytes;
};
static int gn_bwd_plan(int C, int T, int H, int W, int groups, GnBwdPlan& pl) {
    SS_CHECK_ARG(C > 0 && T > 0 && H > 0 && W > 0 && C <= 65535, "gn_relu_pool_backward: bad dims");
    SS_CHECK_ARG(groups >= 0 && (groups == 0 || C % groups == 0), "gn_relu_pool_backward: C=%d not divisible by groups=%d", C, groups);
    const int64_t S = (int64_t)T * H * W;
    SS_CHECK_ARG(S < (1ll << 40), "gn_relu_pool_backward: bad dims");
    pl.split = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(S, 4096), 64));      // a function of the shape only
    pl.bytes = ((size_t)C * pl.split * 2 + (size_t)std::max(groups, 1) * 2) * sizeof(double);
    return STEMSEG_OK;
}

}  // namespace stemseg

using namespace stemseg;

extern "C" int stemseg_hip_level_head(const float* x, int32_t Cin, int64_t V, const float* w, int32_t n_out, const float* add, float* out,
                                      void* stream) {
    return launch_level_head(x, Cin, V, w, n_out, add, out, as_stream(stream), 1, 0, 0, 0);
}

extern "C" size_t stemseg_hip_heads_backward_workspace_bytes(int32_t Cin, int32_t n_out, int64_t V) {
    HeadsBwdPlan pl;
    return heads_bwd_plan(Cin, n_out, V, pl) == STEMSEG_OK ? pl.bytes : 0;
}

extern "C" int stemseg_hip_heads_backward(const float* x, int32_t Cin, int32_t T, int32_t H, int32_t W, const float* w, const float* bias,
                                          int32_t n_out, const int32_t* act_host, const int32_t* grid_axis_host, const float* grid_t,
                                          const float* grid_y, const float* grid_x, const float* out, const float* d_out, float* dx,
                                          float* dw, float* db, void* workspace, size_t ws_bytes, void* stream) {
    (void)bias;                                              // (the forward output carries it; accepted so the call mirrors stemseg_hip_heads)
    SS_CHECK_ARG(T > 0 && H > 0 && W > 0, "heads_backward: bad dims");
    const int64_t V = (int64_t)T * H * W;
    HeadsBwdPlan pl;
    int rc = heads_bwd_plan(Cin, n_out, V, pl);
    if (rc) return rc;
    SS_CHECK_ARG(x && w && d_out && dw && workspace, "heads_backward: null pointer");
    SS_CHECK_ARG((act_host != nullptr) == (grid_axis_host != nullptr), "heads_backward: act and grid_axis tables go together");
    SS_CHECK_ARG(!act_host || out, "heads_backward: null pointer (the forward output is required with an activation table)");
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "heads_backward: workspace must be 256-byte aligned");
    if (ws_bytes < pl.bytes) {
        set_error("heads_backward: workspace too small (%zu < %zu bytes)", ws_bytes, pl.bytes);
        return STEMSEG_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    float* dz_ws = reinterpret_cast<float*>(workspace);
    const float* dz = d_out;                                 // act tables NULL: d_out IS dz (a level matrix of the folded tail)
    HeadsDzParams q;
    if (act_host) {
        q.out = out; q.d_out = d_out; q.dz = dz_ws; q.gt = grid_t; q.gy = grid_y; q.gx = grid_x;
        q.T = T; q.H = H; q.W = W; q.n_out = n_out; q.V = V; q.nq = pl.nq;
        for (int o = 0; o < STEMSEG_MAX_HEAD_OUT; ++o) { q.act[o] = 0; q.axis[o] = 0; }
        for (int o = 0; o < n_out; ++o) {
            q.act[o] = act_host[o];
            q.axis[o] = grid_axis_host[o];
            SS_CHECK_ARG(q.act[o] >= 0 && q.act[o] <= 4 && q.axis[o] >= 0 && q.axis[o] <= 3, "heads_backward: bad act/axis code for channel %d", o);
            if (q.act[o] != 1) q.axis[o] = 0;                // (only the tanh needs the grid back: out - grid)
            SS_CHECK_ARG(q.axis[o] == 0 || (grid_t && grid_y && grid_x), "heads_backward: grid vectors required for channel %d", o);
        }
    }
    void* ev = profile_begin(44, 4.0 * (double)V * ((dx ? 2 : 1) * Cin + n_out), s);
    if (act_host) {
        const bool vec = V % 4 == 0 && aligned16(out) && aligned16(d_out);
        const dim3 grid((unsigned)std::min<int64_t>(ceil_div(pl.nq, 256), 4096), (unsigned)n_out);
        if (vec) hipLaunchKernelGGL(heads_dz_kernel<true>, grid, dim3(256), 0, s, q);
        else hipLaunchKernelGGL(heads_dz_kernel<false>, grid, dim3(256), 0, s, q);
        SS_LAUNCH_CHECK();
        dz = dz_ws;
    }
    HeadsBwdParams p;
    p.x = x; p.w = w; p.dz = dz; p.dx = dx; p.Cin = Cin; p.V = V; p.nq = pl.nq; p.qpc = pl.qpc;
    p.part = reinterpret_cast<double*>(dz_ws + pl.dz_floats);
    const bool vec = V % 4 == 0 && aligned16(x) && aligned16(dz) && (!dx || aligned16(dx));
    switch (n_out) {
        case 1: launch_heads_bwd_n<1>(p, pl.nchunks, vec, s); break;
        case 2: launch_heads_bwd_n<2>(p, pl.nchunks, vec, s); break;
        case 3: launch_heads_bwd_n<3>(p, pl.nchunks, vec, s); break;
        case 4: launch_heads_bwd_n<4>(p, pl.nchunks, vec, s); break;
        case 5: launch_heads_bwd_n<5>(p, pl.nchunks, vec, s); break;
        case 6: launch_heads_bwd_n<6>(p, pl.nchunks, vec, s); break;
        case 7: launch_heads_bwd_n<7>(p, pl.nchunks, vec, s); break;
        case 8: launch_heads_bwd_n<8>(p, pl.nchunks, vec, s); break;
        case 9: launch_heads_bwd_n<9>(p, pl.nchunks, vec, s); break;
        default: launch_heads_bwd_n<10>(p, pl.nchunks, vec, s); break;
    }
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(heads_bwd_combine_kernel, dim3((unsigned)ceil_div((int64_t)n_out * (Cin + 1), 256)), dim3(256), 0, s,
                       (const double*)p.part, pl.nchunks, n_out, Cin, dw, db);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_wide_level_head(const float* x, int32_t Cin, int64_t V, const float* w, int32_t n_out, const float* add, float* out,
                                           void* stream) {
    WidePlan pl;
    int rc = wide_plan("wide_level_head", Cin, n_out, V, pl);
    if (rc) return rc;
    SS_CHECK_ARG(x && w && out, "wide_level_head: null pointer");
    WideFwdParams p;
    p.x = x; p.w = w; p.add = add; p.out = out; p.Cin = Cin; p.n_out = n_out; p.V = V; p.ngroups = ceil_div(V, (n_out <= 32 ? 16 : 8) * WH_TV);
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)std::min<int64_t>(p.ngroups, WH_FWD_MAX_BLOCKS));
    void* ev = profile_begin(44, 4.0 * (double)V * (Cin + (add ? 2 : 1) * n_out), s);
    const bool vec = V % 4 == 0 && aligned16(x) && aligned16(out) && (!add || aligned16(add));
    if (n_out <= 32) {
        if (vec) hipLaunchKernelGGL((wide_level_head_kernel<1, true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((wide_level_head_kernel<1, false>), grid, dim3(256), 0, s, p);
    } else {
        if (vec) hipLaunchKernelGGL((wide_level_head_kernel<2, true>), grid, dim3(256), 0, s, p);
        else hipLaunchKernelGGL((wide_level_head_kernel<2, false>), grid, dim3(256), 0, s, p);
    }
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" size_t stemseg_hip_wide_heads_backward_workspace_bytes(int32_t Cin, int32_t n_out, int64_t V) {
    WidePlan pl;
    return wide_plan("wide_heads_backward", Cin, n_out, V, pl) == STEMSEG_OK ? pl.bytes : 0;
}

extern "C" int stemseg_hip_wide_heads_backward_chunks(int32_t Cin, int32_t n_out, int64_t V) {
    WidePlan pl;
    return wide_plan("wide_heads_backward", Cin, n_out, V, pl) == STEMSEG_OK ? pl.nchunks : 0;
}

extern "C" int stemseg_hip_wide_heads_backward(const float* x, int32_t Cin, int64_t V, const float* w, int32_t n_out, const float* dz, float* dx,
                                               float* dw, float* db, void* workspace, size_t ws_bytes, void* stream) {
    WidePlan pl;
    int rc = wide_plan("wide_heads_backward", Cin, n_out, V, pl);
    if (rc) return rc;
    SS_CHECK_ARG(x && w && dz && dw && workspace, "wide_heads_backward: null pointer");
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "wide_heads_backward: workspace must be 256-byte aligned");
    if (ws_bytes < pl.bytes) {
        set_error("wide_heads_backward: workspace too small (%zu < %zu bytes)", ws_bytes, pl.bytes);
        return STEMSEG_E_WORKSPACE;
    }
    WideBwdParams p;
    p.x = x; p.w = w; p.dz = dz; p.dx = dx; p.part = reinterpret_cast<double*>(workspace);
    p.Cin = Cin; p.n_out = n_out; p.V = V; p.ntiles = pl.ntiles; p.tpc = pl.tpc;
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)pl.nchunks, (unsigned)ceil_div(Cin, WH_CB));
    void* ev = profile_begin(44, 4.0 * (double)V * ((dx ? 2 : 1) * Cin + n_out), s);
    if (n_out <= 32) hipLaunchKernelGGL(wide_heads_bwd_kernel<1>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(wide_heads_bwd_kernel<2>, grid, dim3(256), 0, s, p);
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(heads_bwd_combine_kernel, dim3((unsigned)ceil_div((int64_t)n_out * (Cin + 1), 256)), dim3(256), 0, s,
                       (const double*)p.part, pl.nchunks, n_out, Cin, dw, db);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" int stemseg_hip_upsample_trilinear_backward(const float* d_out, int32_t C, int32_t T, int32_t H, int32_t W, int32_t st, int32_t sy,
                                                       int32_t sx, float* d_in, void* stream) {
    SS_CHECK_ARG(d_out && d_in, "upsample_backward: null pointer");
    SS_CHECK_ARG(C > 0 && T > 0 && H > 0 && W > 0 && (int64_t)C * T * st * H * sy * W * sx < (1ll << 40), "upsample_backward: bad dims");
    SS_CHECK_ARG((st == 1 || st == 2) && sy == sx && (sx == 2 || sx == 4),
                 "upsample_backward: scale (%d, %d, %d) unsupported: st 1 or 2, sy = sx 2 or 4", st, sy, sx);
    UpBwdParams p;
    p.d_out = d_out; p.d_in = d_in; p.C = C; p.T = T; p.H = H; p.W = W;
    p.rt = 1.0f / (float)st; p.rs = 1.0f / (float)sx;
    hipStream_t s = as_stream(stream);
    const bool vec = aligned16(d_out);                       // (output rows are sx W floats, sx even: every row then starts 8-B aligned, 16-B for sx = 4)
    void* ev = profile_begin(40, 4.0 * (double)C * T * H * W * (1.0 + (double)st * sy * sx), s);
    if (st == 1 && sx == 2) launch_up_bwd<1, 2>(p, vec, s);
    else if (st == 2 && sx == 2) launch_up_bwd<2, 2>(p, vec, s);
    else if (st == 1) launch_up_bwd<1, 4>(p, vec, s);
    else launch_up_bwd<2, 4>(p, vec, s);
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}

extern "C" size_t stemseg_hip_gn_relu_pool_backward_workspace_bytes(int32_t C, int32_t T, int32_t H, int32_t W, int32_t groups) {
    GnBwdPlan pl;
    return gn_bwd_plan(C, T, H, W, groups, pl) == STEMSEG_OK ? pl.bytes : 0;
}

extern "C" int stemseg_hip_gn_relu_pool_backward(const float* x, int32_t C, int32_t T, int32_t H, int32_t W, int32_t groups, const float* stats,
                                                 const float* gamma, const float* beta, int32_t pool, const float* d_out, float* dx,
                                                 float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, void* stream) {
    GnBwdPlan pl;
    int rc = gn_bwd_plan(C, T, H, W, groups, pl);
    if (rc) return rc;
    SS_CHECK_ARG(pool == 0 || pool == 1, "gn_relu_pool_backward: pool code %d (0 none, 1 average; the max pool has no backward here)", pool);
    SS_CHECK_ARG(x && d_out && dx, "gn_relu_pool_backward: null pointer");
    SS_CHECK_ARG(groups == 0 || (stats && gamma && beta && dgamma && dbeta && workspace), "gn_relu_pool_backward: null pointer");
    SS_CHECK_ARG(groups == 0 || reinterpret_cast<uintptr_t>(workspace) % 256 == 0, "gn_relu_pool_backward: workspace must be 256-byte aligned");
    if (groups > 0 && ws_bytes < pl.bytes) {
        set_error("gn_relu_pool_backward: workspace too small (%zu < %zu bytes)", ws_bytes, pl.bytes);
        return STEMSEG_E_WORKSPACE;
    }
    GnBwdParams p;
    p.x = x; p.stats = stats; p.gamma = gamma; p.beta = beta; p.d_out = d_out; p.dx = dx;
    p.C = C; p.T = T; p.H = H; p.W = W; p.To = pool ? (T + 1) / 2 : T; p.cpg = groups > 0 ? C / groups : C; p.groups = groups;
    p.pool = pool; p.split = pl.split;
    p.part = reinterpret_cast<double*>(workspace);
    p.coef = p.part ? p.part + (int64_t)C * pl.split * 2 : nullptr;
    hipStream_t s = as_stream(stream);
    const int64_t S = (int64_t)T * H * W;
    const bool vec = W % 4 == 0 && aligned16(x) && aligned16(d_out) && aligned16(dx);
    void* ev = profile_begin(pool ? 43 : 42, 4.0 * (double)C * ((groups ? 5.0 : 2.0) * S + (double)p.To * H * W), s);
    if (vec) hipLaunchKernelGGL(gn_bwd_dy_kernel<true>, dim3((unsigned)pl.split, (unsigned)C), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(gn_bwd_dy_kernel<false>, dim3((unsigned)pl.split, (unsigned)C), dim3(256), 0, s, p);
    SS_LAUNCH_CHECK();
    if (groups > 0) {
        hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((unsigned)groups), dim3(64), 0, s, p, dgamma, dbeta);
        SS_LAUNCH_CHECK();
        const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(S, 256 * 16), 4096));
        if (vec) hipLaunchKernelGGL(gn_bwd_apply_kernel<true>, dim3(bx, (unsigned)C), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(gn_bwd_apply_kernel<false>, dim3(bx, (unsigned)C), dim3(256), 0, s, p);
    }
    profile_end(ev, s);
    SS_LAUNCH_CHECK();
    return STEMSEG_OK;
}
