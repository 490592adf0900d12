// The fp32-input tiles of conv_igemm.h (exact fp32 on v_mfma_f32_32x32x2_f32), the split-K reduce kernel, and launch_conv3d: argument checks, the
// planning shape, and the dispatch to the three tile families.
#include "conv_igemm.h"

namespace stemseg {

// grid = (blocks per channel, channels).  One thread per output float4 (VEC: W % 4 == 0 and 16-B aligned output / residual
// rows) or per output float; 32-bit index math.  Partial slabs are dense [C][T][H][W], so their reads are coalesced 16-B
// loads in the VEC form.  With gn_part every block also leaves the (sum, sum of squares) of the values it wrote in its own
// slot (gn_slot0 + (c % cpg) * gridDim.x + blockIdx.x) of the channel's group -- fixed-order tree, no atomics.
template <bool VEC>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const SplitReduceParams p) {
    constexpr int VW = VEC ? 4 : 1;
    const unsigned wq = (unsigned)p.W / VW;
    const unsigned c = blockIdx.y;
    const unsigned j = blockIdx.x * 256u + threadIdx.x;        // item within the channel
    const bool active = j < p.per_c;
    const float* const partial = p.partial + (int64_t)blockIdx.z * p.part_bs;
    float* const outp = p.out + (int64_t)blockIdx.z * p.out_bs;
    float s1 = 0.f, s2 = 0.f;
    if (active) {
        const unsigned r2 = j / wq, x = (j - r2 * wq) * VW;    // r2 = t * H + y
        const unsigned t = r2 / (unsigned)p.H, y = r2 - t * (unsigned)p.H;
        const int64_t i = (int64_t)c * p.V + (int64_t)r2 * p.W + x;
        const int64_t o = (int64_t)c * p.out_cs + (int64_t)t * p.out_ts + (int64_t)y * p.out_ys + x;
        if constexpr (VEC) {
            float4 acc = *reinterpret_cast<const float4*>(partial + i);
            for (int z = 1; z < p.ksplit; ++z) {
                const float4 v = *reinterpret_cast<const float4*>(partial + (int64_t)z * p.slab + i);
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
            if (p.bias) { const float b = p.bias[c]; acc.x += b; acc.y += b; acc.z += b; acc.w += b; }
            if (p.res) {
                const float4 r = *reinterpret_cast<const float4*>(p.res + (int64_t)c * p.res_cs + (int64_t)t * p.res_ts + (int64_t)y * p.res_ys + x);
                acc.x += r.x; acc.y += r.y; acc.z += r.z; acc.w += r.w;
            }
            if (p.relu) { acc.x = relu_keep_nan(acc.x); acc.y = relu_keep_nan(acc.y); acc.z = relu_keep_nan(acc.z); acc.w = relu_keep_nan(acc.w); }
            *reinterpret_cast<float4*>(outp + o) = acc;
            s1 = (acc.x + acc.y) + (acc.z + acc.w);
            s2 = (acc.x * acc.x + acc.y * acc.y) + (acc.z * acc.z + acc.w * acc.w);
        } else {
            float acc = partial[i];
            for (int z = 1; z < p.ksplit; ++z) acc += partial[(int64_t)z * p.slab + i];
            if (p.bias) acc += p.bias[c];
            if (p.res) acc += p.res[(int64_t)c * p.res_cs + (int64_t)t * p.res_ts + (int64_t)y * p.res_ys + x];
            if (p.relu) acc = relu_keep_nan(acc);
            outp[o] = acc;
            s1 = acc;
            s2 = acc * acc;
        }
    }
    if (p.gn_part) {                                           // (uniform)
        __shared__ double red[2][4];
        double d1 = (double)s1, d2 = (double)s2;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { d1 += __shfl_xor(d1, o, 64); d2 += __shfl_xor(d2, o, 64); }
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = d1; red[1][threadIdx.x >> 6] = d2; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int g = (int)c / p.gn_cpg, slot = p.gn_slot0 + ((int)c % p.gn_cpg) * (int)gridDim.x + (int)blockIdx.x;
            double* o = p.gn_part + (int64_t)blockIdx.z * p.gn_bs + ((size_t)g * p.gn_cap + slot) * 2;
            o[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
            o[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        }
    }
}

void launch_splitk_reduce(const SplitReduceParams& rp, bool vec, unsigned blocks_per_channel, unsigned clips, hipStream_t s) {
    if (vec) hipLaunchKernelGGL(splitk_reduce_kernel<true>, dim3(blocks_per_channel, (unsigned)rp.C, clips), dim3(256), 0, s, rp);
    else hipLaunchKernelGGL(splitk_reduce_kernel<false>, dim3(blocks_per_channel, (unsigned)rp.C, clips), dim3(256), 0, s, rp);
}

// tile shapes --------------------------------------------------------------------------------------
//                       KT KH KW  CK  MI NI WM WN COLS
// fp32-input MFMA mode (STEMSEG_PRECISION_F32)
using K3Big = ConvCfg<3, 3, 3, 4, 4, 2, 1, 4, 1>;          // 128 co x (8 rows x 32 cols): the big tile's generic form (unaligned volumes, Cout % 128 != 0)
using K3BigGL = ConvCfg<3, 3, 3, 2, 4, 2, 1, 4, 1, false, 0, true, 0, true>;   // same tile, 2-channel chunks, two LDS buffers filled by LDS-DMA
using K3Med = ConvCfg<3, 3, 3, 4, 2, 2, 2, 2, 1, true>;    // 128 co x (4 rows x 32 cols)
using K3Small = ConvCfg<3, 3, 3, 4, 2, 1, 2, 2, 1, true>;  // 128 co x (2 rows x 32 cols)
using K1Big = ConvCfg<1, 1, 1, 32, 4, 2, 1, 4, 8, true>;   // 128 co x 256 voxels
using K1Small = ConvCfg<1, 1, 1, 32, 2, 2, 2, 2, 4, true>; // 128 co x 128 voxels
using K1M64 = ConvCfg<1, 1, 1, 32, 2, 2, 1, 4, 8, true>;   //  64 co x 256 voxels
using K1BigGL = ConvCfg<1, 1, 1, 16, 4, 2, 1, 4, 8, false, 0, true, 0, true>;     // direct-to-LDS twins of the 1x1 tiles (half the chunk: two buffers in the same LDS)
using K1SmallGL = ConvCfg<1, 1, 1, 16, 2, 2, 2, 2, 4, false, 0, true, 0, true>;
using K1M64GL = ConvCfg<1, 1, 1, 16, 2, 2, 1, 4, 8, false, 0, true, 0, true>;
// 2-D convolutions of the encoder: the frames of a clip are the T axis, KT = 1
using K2Big = ConvCfg<1, 3, 3, 8, 4, 2, 1, 4, 1, true>;    // 128 co x (8 rows x 32 cols)
using K2Med = ConvCfg<1, 3, 3, 8, 2, 2, 2, 2, 1, true>;    // 128 co x (4 rows x 32 cols)
using K2Small = ConvCfg<1, 3, 3, 8, 2, 1, 2, 2, 1, true>;  // 128 co x (2 rows x 32 cols)
using K2M64 = ConvCfg<1, 3, 3, 8, 2, 2, 1, 4, 1, true>;    //  64 co x (8 rows x 32 cols)
// flat-tile forms for maps whose width wastes >= 10 % of a 32-column tile (8x / 16x maps: pitch 112 / 56; the staged run is
// tile + 2 * PMAX + 8 floats per channel plane, so a tighter PMAX stages less)
using K2FlatBig = ConvCfg<1, 3, 3, 8, 4, 2, 1, 4, 8, true, 0, false, 112>;     // 128 co x 256 flat positions
using K2FlatMed = ConvCfg<1, 3, 3, 8, 2, 2, 2, 2, 4, true, 0, false, 112>;     // 128 co x 128
using K3FlatMed = ConvCfg<3, 3, 3, 4, 2, 2, 2, 2, 4, true, 0, false, 112>;     // 128 co x 128
using K3FlatSmall = ConvCfg<3, 3, 3, 4, 2, 1, 2, 2, 2, true, 0, false, 112>;   // 128 co x 64
using K2FlatBig56 = ConvCfg<1, 3, 3, 8, 4, 2, 1, 4, 8, true, 0, false, 56>;
using K2FlatMed56 = ConvCfg<1, 3, 3, 8, 2, 2, 2, 2, 4, true, 0, false, 56>;
using K3FlatMed56 = ConvCfg<3, 3, 3, 4, 2, 2, 2, 2, 4, true, 0, false, 56>;
using K3FlatSmall56 = ConvCfg<3, 3, 3, 4, 2, 1, 2, 2, 2, true, 0, false, 56>;

template <class Flat, class Tile2D>
static bool prefer_flat(const ConvKParams& p, int tile_cfg) {
    if (!p.vec4 || tile_cfg > 0 || p.dec_W > 0 || p.in_ys > Flat::PMAX || p.in_ys % 4 != 0 || p.W + 2 > p.in_ys) return false;
    return flat_tile_efficiency<Flat>(p) > 1.08 * tile_efficiency<Tile2D>(p.H, p.W);
}

// GL twin when the launch meets its contract, else the register-staged form
template <class GLCfg, class Cfg>
static int launch_gl(const ConvKParams& p, const LaunchCtx& L) {
    if (p.vec4 && p.Cin % GLCfg::CK == 0 && p.Cout % GLCfg::MT == 0) return launch_cfg<GLCfg>(p, L);
    return launch_cfg<Cfg>(p, L);
}

int launch_conv3d(const StemsegVolume& in, const float* packed_w, const float* bias, const StemsegVolume& out,
                  int kt, int kh, int kw, int tile_cfg, hipStream_t s, float* scratch, int64_t scratch_floats, const ConvEpilogue* epi) {
    SS_CHECK_ARG(in.ptr && out.ptr && packed_w, "conv3d: null pointer");
    // the request for the deep 3x3x3 tile is a request on top of the automatic choice: everything but launch_split_family's eligibility test sees tile_cfg 0
    const bool deep_tile = tile_cfg == STEMSEG_TILE_CFG_DEEP;
    if (deep_tile) tile_cfg = 0;
    const int prec = epi ? epi->precision : STEMSEG_PRECISION_F32;
    SS_CHECK_ARG(prec == STEMSEG_PRECISION_F32 || prec == STEMSEG_PRECISION_BF16X6 || prec == STEMSEG_PRECISION_F16X3,
                 "conv3d: precision %d (0 f32, 2 bf16x6, 3 f16x3)", prec);
    const bool k3 = (kt == 3 && kh == 3 && kw == 3), k1 = (kt == 1 && kh == 1 && kw == 1), k2 = (kt == 1 && kh == 3 && kw == 3);
    const bool k4 = (kt == 1 && kh == 4 && kw == 4);        // (f16x3 only: the space-to-depth form of the 7x7 stride-2 stem)
    SS_CHECK_ARG(k3 || k1 || k2 || (k4 && prec == STEMSEG_PRECISION_F16X3), "conv3d: kernel %dx%dx%d unsupported (3x3x3, 1x3x3, 1x1x1; 1x4x4 in f16x3 mode)", kt, kh, kw);
    const bool flat = epi && epi->dec_W > 0;
    if (flat) {
        SS_CHECK_ARG(k1 && in.T == 1 && in.H == 1 && epi->dec_H > 0 && (int64_t)out.T * out.H * out.W == in.W &&
                     out.H == epi->dec_H && out.W == epi->dec_W, "conv3d: flat-decode epilogue needs a 1x1x1 conv on a [C][V] input with V == T*H*W of `out`");
    } else {
        SS_CHECK_ARG(in.T == out.T + kt - 1 && in.H == out.H + kh - 1 && in.W == out.W + kw - 1,
                     "conv3d: input extents (%d,%d,%d) must be output (%d,%d,%d) + kernel - 1", in.T, in.H, in.W, out.T, out.H, out.W);
    }
    SS_CHECK_ARG(in.C % 4 == 0 && out.C % 32 == 0, "conv3d: Cin %% 4 == 0 and Cout %% 32 == 0 required (got %d, %d)", in.C, out.C);
    ConvKParams p;
    p.in = in.ptr; p.in_cs = in.c_stride; p.in_ts = in.t_stride; p.in_ys = in.y_stride; p.in_limit = in.limit; p.in_H = in.H;
    p.wpk = packed_w; p.bias = bias;
    p.out = out.ptr; p.out_cs = out.c_stride; p.out_ts = out.t_stride; p.out_ys = out.y_stride;
    p.Cin = in.C; p.Cout = out.C; p.T = out.T; p.H = out.H; p.W = out.W;
    if (flat) { p.T = 1; p.H = 1; p.W = in.W; }
    p.relu = epi ? epi->relu : 0;
    p.res = epi ? epi->res : nullptr;
    p.res_cs = epi ? epi->res_cs : 0; p.res_ts = epi ? epi->res_ts : 0; p.res_ys = epi ? epi->res_ys : 0;
    p.dec_H = flat ? epi->dec_H : 0; p.dec_W = flat ? epi->dec_W : 0;
    p.gn_part = epi ? epi->gn_part : nullptr;
    p.gn_cpg = epi ? epi->gn_cpg : 0; p.gn_cap = epi ? epi->gn_cap : 0; p.gn_slot0 = 0;
    p.gn_used_host = epi ? epi->gn_used : nullptr;
    p.zero_t_halo = (epi && epi->zero_t_halo && k3) ? 1 : 0;
    p.out_p16 = nullptr;
    if (epi && epi->p16_out) {
        const bool dense = out.t_stride == (int64_t)out.H * out.W && out.y_stride == out.W && out.c_stride == (int64_t)out.T * out.H * out.W;
        SS_CHECK_ARG(epi->p16_done && dense && !flat && !epi->res && !epi->gn_part && out.C % 8 == 0 && prec == STEMSEG_PRECISION_F16X3 && (!epi || epi->nb <= 1),
                     "conv3d: the pair-plane output needs f16x3, a dense output volume, no residual / statistics / clip batch");
        *epi->p16_done = 0;
        p.out_p16 = epi->p16_out;
        p.gn_used_host = epi->p16_done;                    // (see ConvKParams::out_p16)
    }
    p.nb = (epi && epi->nb > 1) ? epi->nb : 1;
    p.in_bs = p.nb > 1 ? epi->in_bs : 0; p.out_bs = p.nb > 1 ? epi->out_bs : 0; p.gn_bs = p.nb > 1 ? epi->gn_bs : 0;
    SS_CHECK_ARG(p.nb == 1 || (!p.res && p.nb <= 65535 && p.in_bs % 4 == 0 && p.out_bs % 4 == 0), "conv3d: a clip batch takes no residual and 16-byte aligned clip strides");
    SS_CHECK_ARG(!p.gn_part || ((p.gn_cpg == 4 || p.gn_cpg == 8) && p.gn_used_host && p.Cout % p.gn_cpg == 0 && !(epi->relu || epi->res)),
                 "conv3d: fused GroupNorm statistics need groups of 4 or 8 channels and a plain (bias-only) epilogue");
    auto al16 = [](const void* ptr, int64_t cs, int64_t ts, int64_t ys, int T, int H) {
        return (reinterpret_cast<uintptr_t>(ptr) % 16 == 0) && (cs % 4 == 0) && (T == 1 || ts % 4 == 0) && (H == 1 || ys % 4 == 0);
    };
    p.vec_epi = (!flat && p.W % 4 == 0 && al16(p.out, p.out_cs, p.out_ts, p.out_ys, p.T, p.H) &&
                 (!p.res || al16(p.res, p.res_cs, p.res_ts, p.res_ys, p.T, p.H))) ? 1 : 0;
    p.tiles_x = p.tiles_y = 0;
    p.t_fastest = 1;
    p.flat_t = 0; p.T_all = p.T;
    const bool aligned = (reinterpret_cast<uintptr_t>(in.ptr) % 16 == 0) && (in.c_stride % 4 == 0) &&
                         (in.T == 1 || in.t_stride % 4 == 0) && (in.H == 1 || in.y_stride % 4 == 0);
    p.vec4 = aligned ? 1 : 0;
    SS_CHECK_ARG(reinterpret_cast<uintptr_t>(packed_w) % 16 == 0, "conv3d: packed weights must be 16-byte aligned");
    // planning shape (see PlanCtx): `frames` frames in this launch, planned as `plan_frames`
    PlanCtx pc_store;
    const PlanCtx* pc = nullptr;
    if (epi && epi->plan_frames > 0) {
        SS_CHECK_ARG(epi->frames > 0 && epi->plan_scratch_floats >= 0, "conv3d: plan_frames needs the launch's own frame count");
        pc_store.shape = p;
        pc_store.scratch_floats = epi->plan_scratch_floats;
        if (p.T == 1 && p.H == 1) {                        // a flat [C][V] launch: V = frames x (voxels per frame)
            SS_CHECK_ARG(p.W % epi->frames == 0, "conv3d: flat volume of %d voxels is not %d whole frames", p.W, epi->frames);
            const int64_t Wp = (int64_t)(p.W / epi->frames) * epi->plan_frames;
            SS_CHECK_ARG(Wp < (1ll << 31), "conv3d: planning volume too large");
            pc_store.shape.W = (int)Wp;
        } else {
            SS_CHECK_ARG(p.T == epi->frames, "conv3d: launch of %d t-planes announced as %d frames", p.T, epi->frames);
            pc_store.shape.T = epi->plan_frames;
        }
        pc_store.shape.T_all = pc_store.shape.T;
        pc = &pc_store;
    }
    const ConvKParams& d = pc ? pc->shape : p;
    SS_CHECK_ARG(!epi || (epi->plan_clips >= 0 && epi->plan_clips <= 4096), "conv3d: plan_clips %d", epi ? epi->plan_clips : 0);
    const LaunchCtx L{s, scratch, scratch_floats, pc, epi && epi->p16_keep_plan, epi ? epi->plan_sink : nullptr, epi && epi->plan_clips > 1 ? epi->plan_clips : 1, deep_tile};
    if (k4) return launch_stem_f16x3(p, L);
    if (prec == STEMSEG_PRECISION_BF16X6) return launch_split_family<2>(p, d, L, tile_cfg, k3, k2);
    if (prec == STEMSEG_PRECISION_F16X3) return launch_split_family<3>(p, d, L, tile_cfg, k3, k2);
    const bool auto_cfg = tile_cfg <= 0 || tile_cfg > 3;
    if (k3) {
        int cfg = tile_cfg;
        if (auto_cfg) {
            // largest tile that still gives every CU two workgroups
            if (tile_workgroups<K3Big>(d) >= 512) cfg = 1;
            else if (tile_workgroups<K3Med>(d) >= 384) cfg = 2;
            else cfg = 3;
        }
        if (cfg == 2 && prefer_flat<K3FlatMed56, K3Med>(p, tile_cfg)) return launch_cfg<K3FlatMed56>(p, L);
        if (cfg == 3 && prefer_flat<K3FlatSmall56, K3Small>(p, tile_cfg)) return launch_cfg<K3FlatSmall56>(p, L);
        if (cfg == 2 && prefer_flat<K3FlatMed, K3Med>(p, tile_cfg)) return launch_cfg<K3FlatMed>(p, L);
        if (cfg == 3 && prefer_flat<K3FlatSmall, K3Small>(p, tile_cfg)) return launch_cfg<K3FlatSmall>(p, L);
        if (cfg == 1 && p.vec4 && p.Cout % 128 == 0) {          // (Cin % 2 == 0 holds: Cin % 4 == 0 above)
            if (auto_cfg) return launch_planned<K3BigGL, K3Med>(p, d, L, 2, 2);
            return launch_cfg<K3BigGL>(p, L);
        }
        if (cfg == 1 && auto_cfg) return launch_planned<K3Big, K3Med>(p, d, L, 2, 2);
        if (cfg == 1) return launch_cfg<K3Big>(p, L);
        if (cfg == 2) return launch_cfg<K3Med>(p, L);
        return launch_cfg<K3Small>(p, L);
    }
    if (k2) {
        if (p.Cout <= 64) return launch_cfg<K2M64>(p, L);
        int cfg = tile_cfg;
        if (auto_cfg) {   // biggest tile (best weight reuse) that split-K can still spread over the chip
            const int64_t need = scratch ? 96 : 384;
            if (tile_workgroups<K2Big>(d) >= need) cfg = 1;
            else if (tile_workgroups<K2Med>(d) >= need) cfg = 2;
            else cfg = 3;
        }
        if (cfg == 1 && prefer_flat<K2FlatBig56, K2Big>(p, tile_cfg)) return launch_cfg<K2FlatBig56>(p, L);
        if (cfg >= 2 && prefer_flat<K2FlatMed56, K2Med>(p, tile_cfg)) return launch_cfg<K2FlatMed56>(p, L);
        if (cfg == 1 && prefer_flat<K2FlatBig, K2Big>(p, tile_cfg)) return launch_cfg<K2FlatBig>(p, L);
        if (cfg >= 2 && prefer_flat<K2FlatMed, K2Med>(p, tile_cfg)) return launch_cfg<K2FlatMed>(p, L);
        if (cfg == 1 && auto_cfg && tile_workgroups<K2Big>(d) >= 512) return launch_planned<K2Big, K2Med>(p, d, L, 3, 3);
        if (cfg == 1) return launch_cfg<K2Big>(p, L);
        if (cfg == 2) return launch_cfg<K2Med>(p, L);
        return launch_cfg<K2Small>(p, L);
    }
    if (p.Cout <= 64) return launch_gl<K1M64GL, K1M64>(p, L);
    int cfg = tile_cfg;
    if (cfg <= 0 || cfg > 2) {
        cfg = (tile_workgroups<K1Big>(d) >= (scratch ? 96 : 512)) ? 1 : 2;
        // expansion convs with a short K (<= 8 channel chunks) are bound by their output / residual traffic: the 128-voxel
        // tile keeps twice as many workgroups in flight (measured, tools/conv_sweep.py: 64->256 +res 233 -> 167 us)
        // -- up to ~2000 workgroups of the big tile; beyond that (several clips per encoder pass) the big tile wins again
        // (T = 32 sweep: 64->256 +res 532 vs 570 us, 128->512 +res 372 vs 438 us)
        if (p.Cin <= 256 && p.Cout >= 4 * p.Cin && tile_workgroups<K1Big>(d) < 2048) cfg = 2;
    }
    if (cfg == 1) return launch_gl<K1BigGL, K1Big>(p, L);
    return launch_gl<K1SmallGL, K1Small>(p, L);
}

int launch_conv3d_gn(const StemsegVolume& in, const float* packed_w, const float* bias, const StemsegVolume& out, int kt, int kh, int kw,
                     int tile_cfg, hipStream_t s, float* splitk_scratch, int64_t splitk_scratch_floats, const ConvEpilogue* epi, int groups,
                     float eps, float* stats, double* gn_scratch, int64_t stats_bs) {
    SS_CHECK_ARG(stats && gn_scratch && groups > 0 && out.C % groups == 0, "conv3d_gn: bad GroupNorm arguments");
    const int cpg = out.C / groups;
    const int64_t S = (int64_t)out.T * out.H * out.W;
    const bool dense = out.t_stride == (int64_t)out.H * out.W && out.y_stride == out.W && out.c_stride == S;
    // upper bound of the slots any tile choice can need: smallest 2-D tile (2 rows x 32 columns) + a fully split-K launch
    const int64_t slot_bound = ceil_div(out.W, 32) * ceil_div(out.H, 2) * out.T + (int64_t)cpg * ceil_div(S, 256);
    if ((cpg != 4 && cpg != 8) || slot_bound > GN_SLOT_CAP || (epi && (epi->relu || epi->res || epi->dec_W > 0))) {
        SS_CHECK_ARG(dense, "conv3d_gn: the separate statistics pass needs a dense output");
        PlanSink* const sink = epi ? epi->plan_sink : nullptr;
        const int rec0 = sink ? sink->n : 0;
        int rc = launch_conv3d(in, packed_w, bias, out, kt, kh, kw, tile_cfg, s, splitk_scratch, splitk_scratch_floats, epi);
        if (sink) {                                        // dry run: the statistics would be a pass of their own over the output
            for (int i = rec0; i < sink->n && i < sink->cap; ++i) sink->rec[i].gn = 3;
            return rc;
        }
        const int nb = (epi && epi->nb > 1) ? epi->nb : 1;
        for (int b = 0; b < nb && !rc; ++b)
            rc = launch_gn_stats(out.ptr + (nb > 1 ? b * epi->out_bs : 0), out.C, S, groups, eps, stats + (int64_t)b * stats_bs, gn_scratch + (nb > 1 ? b * epi->gn_bs : 0), s);
        return rc;
    }
    ConvEpilogue e = epi ? *epi : ConvEpilogue();
    int used = 0;
    e.gn_part = gn_scratch; e.gn_cpg = cpg; e.gn_cap = GN_SLOT_CAP; e.gn_used = &used;
    const int rc = launch_conv3d(in, packed_w, bias, out, kt, kh, kw, tile_cfg, s, splitk_scratch, splitk_scratch_floats, &e);
    if (rc || e.plan_sink) return rc;
    return launch_gn_finalize_slots(gn_scratch, groups, GN_SLOT_CAP, used, (double)cpg * (double)S, eps, stats, s, e.nb, e.gn_bs, stats_bs);
}

static ConvEpilogue epilogue_from_abi(const StemsegConvEpilogue* epilogue) {
    ConvEpilogue e;
    if (epilogue) {
        e.relu = epilogue->relu; e.res = epilogue->residual; e.res_cs = epilogue->res_c_stride; e.res_ts = epilogue->res_t_stride;
        e.res_ys = epilogue->res_y_stride; e.dec_H = epilogue->decode_H; e.dec_W = epilogue->decode_W;
        e.precision = epilogue->precision;
        e.frames = epilogue->frames; e.plan_frames = epilogue->plan_frames; e.plan_scratch_floats = epilogue->plan_scratch_floats;
    }
    return e;
}

}  // namespace stemseg

extern "C" int64_t stemseg_hip_conv3d_gn_scratch_doubles(int32_t Cout, int32_t groups) {
    return (Cout > 0 && groups > 0) ? stemseg::gn_scratch_doubles(Cout, groups) : 0;
}

extern "C" int stemseg_hip_conv3d_gn(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                                     int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, float* splitk_scratch, int64_t splitk_scratch_floats,
                                     int32_t precision, int32_t groups, float eps, float* stats, double* gn_scratch, void* stream) {
    using namespace stemseg;
    SS_CHECK_ARG(in && out, "conv3d_gn: null volume");
    ConvEpilogue e;
    e.precision = precision;
    return launch_conv3d_gn(*in, packed_w, bias, *out, kt, kh, kw, tile_cfg, as_stream(stream), splitk_scratch, splitk_scratch_floats, &e, groups,
                            eps, stats, gn_scratch);
}

extern "C" int stemseg_hip_conv3d(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                                  int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, float* splitk_scratch,
                                  int64_t splitk_scratch_floats, const StemsegConvEpilogue* epilogue, void* stream) {
    using namespace stemseg;
    SS_CHECK_ARG(in && out, "conv3d: null volume");
    ConvEpilogue e = epilogue_from_abi(epilogue);
    return launch_conv3d(*in, packed_w, bias, *out, kt, kh, kw, tile_cfg, as_stream(stream), splitk_scratch, splitk_scratch_floats,
                         epilogue ? &e : nullptr);
}

// stemseg_hip_conv3d with the caller's promise that planes 0 and T + 1 of `in` are all zero (ConvEpilogue::zero_t_halo); with `stats`, the
// GroupNorm statistics of the output as stemseg_hip_conv3d_gn leaves them
static int conv3d_zero_t_halo(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out, int32_t kt, int32_t kh,
                              int32_t kw, int32_t tile_cfg, float* splitk_scratch, int64_t splitk_scratch_floats, const StemsegConvEpilogue* epilogue,
                              int32_t groups, float eps, float* stats, double* gn_scratch, int32_t plan_clips, void* stream) {
    using namespace stemseg;
    SS_CHECK_ARG(in && out, "conv3d_zero_t_halo: null volume");
    SS_CHECK_ARG(kt == 3, "conv3d_zero_t_halo: the promise is about the temporal halo planes of a kernel with kt == 3 (got %d)", kt);
    ConvEpilogue e = epilogue_from_abi(epilogue);
    e.zero_t_halo = 1;
    e.plan_clips = plan_clips;
    if (stats)
        return launch_conv3d_gn(*in, packed_w, bias, *out, kt, kh, kw, tile_cfg, as_stream(stream), splitk_scratch, splitk_scratch_floats, &e, groups,
                                eps, stats, gn_scratch);
    return launch_conv3d(*in, packed_w, bias, *out, kt, kh, kw, tile_cfg, as_stream(stream), splitk_scratch, splitk_scratch_floats, &e);
}

extern "C" int stemseg_hip_conv3d_zero_t_halo(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                                              int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, float* splitk_scratch,
                                              int64_t splitk_scratch_floats, const StemsegConvEpilogue* epilogue, int32_t groups, float eps,
                                              float* stats, double* gn_scratch, void* stream) {
    return conv3d_zero_t_halo(in, packed_w, bias, out, kt, kh, kw, tile_cfg, splitk_scratch, splitk_scratch_floats, epilogue, groups, eps, stats, gn_scratch, 0, stream);
}

// ... one stage of a decoder on its own, with the split-K factor that decoder's plan_clips gives it (the trainable decoder forward: its maps are
// then the bits stemseg_hip_decoder_forward computes)
extern "C" int stemseg_hip_conv3d_zero_t_halo_clips(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                                                    int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, float* splitk_scratch,
                                                    int64_t splitk_scratch_floats, const StemsegConvEpilogue* epilogue, int32_t groups, float eps,
                                                    float* stats, double* gn_scratch, int32_t plan_clips, void* stream) {
    return conv3d_zero_t_halo(in, packed_w, bias, out, kt, kh, kw, tile_cfg, splitk_scratch, splitk_scratch_floats, epilogue, groups, eps, stats, gn_scratch, plan_clips,
                              stream);
}

// ... on a CLIP BATCH, as a decoder stage of n_clips clips launches it: the clip is a grid dimension, clip c's volumes lie c * in_clip_stride /
// c * out_clip_stride floats behind clip 0's.  No split-K scratch and no statistics: the launch is un-split.
extern "C" int stemseg_hip_conv3d_zero_t_halo_batch(const StemsegVolume* in, const float* packed_w, const float* bias, const StemsegVolume* out,
                                                    int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg, const StemsegConvEpilogue* epilogue,
                                                    int32_t n_clips, int64_t in_clip_stride, int64_t out_clip_stride, void* stream) {
    using namespace stemseg;
    SS_CHECK_ARG(in && out, "conv3d_zero_t_halo_batch: null volume");
    SS_CHECK_ARG(kt == 3, "conv3d_zero_t_halo: the promise is about the temporal halo planes of a kernel with kt == 3 (got %d)", kt);
    SS_CHECK_ARG(n_clips >= 1 && n_clips <= 4096 && in_clip_stride >= 0 && out_clip_stride >= 0, "conv3d_zero_t_halo_batch: n_clips=%d", n_clips);
    ConvEpilogue e = epilogue_from_abi(epilogue);
    e.zero_t_halo = 1;
    e.nb = n_clips; e.in_bs = in_clip_stride; e.out_bs = out_clip_stride;
    return launch_conv3d(*in, packed_w, bias, *out, kt, kh, kw, tile_cfg, as_stream(stream), nullptr, 0, &e);
}

// the launch decision of the entries above, recorded instead of run (include/stemseg_hip.h): the same launch_conv3d / launch_conv3d_gn
// with a sink in the epilogue, so the plan is what runs by construction
static int conv3d_plan(const StemsegVolume* in, const float* bias, const StemsegVolume* out, int32_t kt, int32_t kh, int32_t kw, int32_t tile_cfg,
                       const float* splitk_scratch, int64_t splitk_scratch_floats, const StemsegConvEpilogue* epilogue, int32_t form,
                       int32_t gn_groups, int32_t plan_clips, StemsegConvPlanRecord* records, int32_t capacity, int32_t* count) {
    using namespace stemseg;
    SS_CHECK_ARG(in && out && count && capacity >= 0 && (records || capacity == 0), "conv3d_plan: null volume / record array");
    SS_CHECK_ARG((form & ~(STEMSEG_PLAN_GN | STEMSEG_PLAN_ZERO_T_HALO)) == 0, "conv3d_plan: form %d", form);
    alignas(16) static float no_weights[4];                // (never read: the dispatch asks for a non-null, 16-byte aligned address)
    alignas(16) static double no_table[2];
    PlanSink sink{records, capacity, 0};
    ConvEpilogue e;
    const bool gn = (form & STEMSEG_PLAN_GN) != 0, zth = (form & STEMSEG_PLAN_ZERO_T_HALO) != 0;
    if (gn && !zth) e.precision = epilogue ? epilogue->precision : STEMSEG_PRECISION_F32;      // stemseg_hip_conv3d_gn takes the precision alone
    else e = epilogue_from_abi(epilogue);
    if (zth) {
        SS_CHECK_ARG(kt == 3, "conv3d_zero_t_halo: the promise is about the temporal halo planes of a kernel with kt == 3 (got %d)", kt);
        e.zero_t_halo = 1;
    }
    e.plan_sink = &sink;
    e.plan_clips = plan_clips;
    float* const scratch = const_cast<float*>(splitk_scratch);
    const int rc = gn ? launch_conv3d_gn(*in, no_weights, bias, *out, kt, kh, kw, tile_cfg, nullptr, scratch, splitk_scratch_floats, &e, gn_groups, 1e-5f,
                                         no_weights, no_table)
                      : launch_conv3d(*in, no_weights, bias, *out, kt, kh, kw, tile_cfg, nullptr, scratch, splitk_scratch_floats, &e);
    *count = sink.n;
    return rc;
}

extern "C" int stemseg_hip_conv3d_plan(const StemsegVolume* in, const float* bias, const StemsegVolume* out, int32_t kt, int32_t kh, int32_t kw,
                                       int32_t tile_cfg, const float* splitk_scratch, int64_t splitk_scratch_floats,
                                       const StemsegConvEpilogue* epilogue, int32_t form, int32_t gn_groups, StemsegConvPlanRecord* records,
                                       int32_t capacity, int32_t* count) {
    return conv3d_plan(in, bias, out, kt, kh, kw, tile_cfg, splitk_scratch, splitk_scratch_floats, epilogue, form, gn_groups, 0, records, capacity, count);
}

// ... as a stage of a decoder whose descriptor carries `plan_clips` decides it (StemsegDecoderDesc.plan_clips)
extern "C" int stemseg_hip_conv3d_plan_clips(const StemsegVolume* in, const float* bias, const StemsegVolume* out, int32_t kt, int32_t kh, int32_t kw,
                                             int32_t tile_cfg, const float* splitk_scratch, int64_t splitk_scratch_floats,
                                             const StemsegConvEpilogue* epilogue, int32_t form, int32_t gn_groups, int32_t plan_clips,
                                             StemsegConvPlanRecord* records, int32_t capacity, int32_t* count) {
    return conv3d_plan(in, bias, out, kt, kh, kw, tile_cfg, splitk_scratch, splitk_scratch_floats, epilogue, form, gn_groups, plan_clips, records, capacity, count);
}
